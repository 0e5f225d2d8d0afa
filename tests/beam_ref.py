"""NumPy restatement of the beam select's order (include/dpsx.h: dpsx_topk_seg_f32), independent of the kernels.

Within a segment particle a comes before particle b exactly when the select's argmin_better(a, b) holds: a NaN cost
before every number (among NaNs the lower index first), then the lower value, equal values (-0.0 == +0.0) by the lower
index.  Top-b is the first b particles of the segment in that order; rank 0 is torch.argmin's answer."""
import math

import numpy as np


def order(v):
    """the indices of the 1-D cost vector v, sorted by the select's order"""
    v = [float(c) for c in np.asarray(v, dtype=np.float32).reshape(-1)]
    return sorted(range(len(v)), key=lambda i: (0, 0.0, i) if math.isnan(v[i]) else (1, v[i], i))


def topb(costs, segments, b):
    """costs [segments * L] -> int64 [segments * b]: the global indices of every segment's first b particles, rank-major"""
    costs = np.asarray(costs, dtype=np.float32).reshape(-1)
    segments, b = int(segments), int(b)
    if segments < 1 or costs.size == 0 or costs.size % segments:
        raise ValueError(f"{costs.size} costs do not split into {segments} non-empty segments")
    L = costs.size // segments
    if not 1 <= b <= L:
        raise ValueError(f"b = {b} does not lie in [1, {L}]")
    out = [m * L + i for m in range(segments) for i in order(costs[m * L:(m + 1) * L])[:b]]
    return np.asarray(out, dtype=np.int64)
