"""NumPy restatement of the library's resampling draw (include/dpsx.h, "resampling draw", steps 1 to 5) -- the reference
the device kernels are compared with.  Integer arithmetic from the weights on, so `draw` reproduces the kernels' ids
exactly from (q, u); `weights` uses NumPy's fp32 exp, which may differ from the device's expf in the last bits."""
import numpy as np

TWO24 = 1 << 24


def weights(d, inv_scale):
    """steps 1-3: integer weights q [K] (uint32 values in [0, 2^24]) of one segment of distances d [K]"""
    d = np.asarray(d, dtype=np.float32)
    finite = np.isfinite(d)
    q = np.zeros(d.shape, dtype=np.int64)
    if finite.any():
        d_min = d[finite].min()
        with np.errstate(over="ignore", invalid="ignore"):
            x = (d[finite] - d_min) * np.float32(inv_scale)                 # fp32 throughout, no fused multiply-add
            w = np.exp(-x).astype(np.float32)
        w = np.where(w >= 0, np.minimum(w, np.float32(1)), np.float32(0))   # inert for a finite inv_scale >= 0
        q[finite] = np.rint(w * np.float32(TWO24)).astype(np.int64)
    return q


def uniform_ints(u):
    """ui = clamp((uint32)(u * 2^24), 0, 2^24 - 1); a NaN counts as 0"""
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.asarray(u, dtype=np.float32) * np.float32(TWO24)             # exact: a power-of-two scaling
    s = np.where(s > 0, np.minimum(s, np.float32(TWO24 - 1)), np.float32(0))      # NaN fails s > 0
    return s.astype(np.uint64)


def draw(q, u):
    """steps 4-5 for one segment: q [K] integer weights, u [K] uniforms -> local ids [K]"""
    q = np.asarray(q).astype(np.uint64)
    k = q.size
    if (q == q[0]).all():                                                   # the flat rule (k = 1, all zero included)
        return np.arange(k, dtype=np.int64)
    cdf = np.cumsum(q, dtype=np.uint64)
    target = (cdf[-1] * uniform_ints(u)) >> np.uint64(24)                   # total <= k 2^24: no overflow for k <= 65536
    return np.minimum(np.searchsorted(cdf, target, side="right"), k - 1).astype(np.int64)   # smallest i: cdf_i > target


def draw_segments(q, u, segments):
    """global ids [N] for q, u [N] split into `segments` equal segments"""
    q, u = np.asarray(q).reshape(segments, -1), np.asarray(u, dtype=np.float32).reshape(segments, -1)
    k = q.shape[1]
    return np.concatenate([m * k + draw(q[m], u[m]) for m in range(segments)])
