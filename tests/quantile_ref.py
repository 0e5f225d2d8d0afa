"""Float64 restatement of the order statistics (include/dpsx.h "order statistics"): the reference of
tests/test_quantile_gpu.py and the subject of tests/test_quantile_cpu.py.  numpy only.

Everything is per image and per element: the element's K values are sorted by the integer key s ^ ((s >> 31) & 0x7fffffff)
of their bit patterns (IEEE order with -0.0 before +0.0, a total order), the quantiles interpolate between neighbours in
float64 with one rounding per operation, the rank counts the particles strictly below the label, and the CRPS is the
sorted-order form (1/K) sum |x_(i) - y| - (1/K^2) sum (2 i - K + 1) x_(i)."""
import numpy as np

QNAN_BITS = np.int32(0x7fc00000)
MAX_K, MAX_Q = 512, 8


def order_key(x):
    """the integer key of fp32 values: signed comparison of the keys is the definition's order; the map is its own inverse"""
    s = np.ascontiguousarray(x, dtype=np.float32).view(np.int32)
    return s ^ ((s >> 31) & np.int32(0x7fffffff))


def sort_particles(x):
    """x [K, d] fp32 -> the values sorted along axis 0 in the definition's order, bits kept"""
    keys = np.sort(order_key(x), axis=0)
    return (keys ^ ((keys >> 31) & np.int32(0x7fffffff))).view(np.float32)


def positions(probs, k):
    """-> [(lo, hi, f)] per probability: h = p (K - 1) in double, lo = floor(h), hi = min(lo + 1, K - 1), f = h - lo"""
    out = []
    for p in probs:
        h = float(p) * float(k - 1)
        lo = int(np.floor(h))
        out.append((lo, min(lo + 1, k - 1), h - lo))
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def quantiles_sorted(xs, nan, probs):
    """xs [K, d] sorted, nan [d] bool -> [q, d] fp32"""
    k, d = xs.shape
    out = np.empty((len(probs), d), dtype=np.int32)
    for i, (lo, hi, f) in enumerate(positions(probs, k)):
        a, b = xs[lo], xs[hi]
        if f == 0.0:
            r = _bits(a).copy()
        else:
            with np.errstate(all="ignore"):
                a64, b64 = a.astype(np.float64), b.astype(np.float64)
                v = (a64 + f * (b64 - a64)).astype(np.float32)       # three float64 roundings, then one to fp32
                same = a == b
            r = np.where(np.isnan(v), QNAN_BITS, _bits(v))
            r = np.where(same, _bits(a), r)
        out[i] = np.where(nan, QNAN_BITS, r)
    return out.view(np.float32)


def crps_sorted(xs, y):
    """xs [K, d] sorted, y [d] -> crps_e [d] fp32 (meaningless where the element is invalid)"""
    k = xs.shape[0]
    y64 = y.astype(np.float64)
    s1, s2 = np.zeros(xs.shape[1]), np.zeros(xs.shape[1])
    with np.errstate(all="ignore"):
        for i in range(k):                                   # both sums in sorted order
            xi = xs[i].astype(np.float64)
            s1 = s1 + np.abs(xi - y64)
            s2 = s2 + float(2 * i - k + 1) * xi
        return (s1 / float(k) - s2 / (float(k) * float(k))).astype(np.float32)


def order_stats(x, images=1, probs=(0.05, 0.5, 0.95), label=None):
    """x [n, ...] fp32 image-major, label [images, ...] or None -> {"quantiles" [M, q, ...], "info" [M, 4]} and, with a
    label, "hist" [M, K + 2] int32, "crps" [M], "crps_e" [M, d] (per element, NaN where invalid)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = x.shape[0]
    if images < 1 or n < 1 or n % images:
        raise ValueError(f"{n} particles do not split into {images} images")
    k, shape = n // images, x.shape[1:]
    if k > MAX_K:
        raise ValueError(f"K = {k} > {MAX_K}")
    probs = [float(p) for p in probs]
    if not 1 <= len(probs) <= MAX_Q or any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError(f"bad probabilities {probs}")
    flat = x.reshape(images, k, -1)
    d = flat.shape[2]
    y = None if label is None else np.ascontiguousarray(label, dtype=np.float32).reshape(images, d)
    quant = np.empty((images, len(probs), d), dtype=np.float32)
    info = np.empty((images, 4), dtype=np.float32)
    hist = np.zeros((images, k + 2), dtype=np.int32)
    crps_e = np.full((images, d), np.nan, dtype=np.float32)
    for m in range(images):
        xs = sort_particles(flat[m])
        nan = np.isnan(flat[m]).any(axis=0)
        quant[m] = quantiles_sorted(xs, nan, probs)
        with np.errstate(all="ignore"):
            width = quant[m, -1] - quant[m, 0]               # one fp32 subtraction
        fin = np.isfinite(width)
        with np.errstate(all="ignore"):
            info[m, 1] = np.float32(width[fin].astype(np.float64).sum() / float(fin.sum())) if fin.any() else np.nan
        info[m, 3] = k
        if y is None:
            info[m, 0], info[m, 2] = np.nan, 0.0
            continue
        invalid = nan | np.isnan(y[m])
        with np.errstate(all="ignore"):
            rank = (flat[m] < y[m][None]).sum(axis=0)
        hist[m] = np.bincount(np.where(invalid, k + 1, rank), minlength=k + 2)
        ce = crps_sorted(xs, y[m])
        crps_e[m] = np.where(invalid, np.nan, ce)
        valid = ~invalid
        info[m, 0] = np.float32(ce[valid].astype(np.float64).sum() / float(valid.sum())) if valid.any() else np.nan
        info[m, 2] = invalid.sum()
    res = {"quantiles": quant.reshape((images, len(probs)) + shape), "info": info}
    if y is not None:
        res.update(hist=hist, crps=info[:, 0].copy(), crps_e=crps_e)
    return res


def interval_coverage(hist, lo_rank, hi_rank):
    """the fraction of the valid elements with lo_rank <= rank <= hi_rank"""
    h = np.asarray(hist, dtype=np.int64)
    k = h.shape[-1] - 2
    return h[..., lo_rank:hi_rank + 1].sum(axis=-1) / h[..., :k + 1].sum(axis=-1)


def calibration_bounds(d, k, sigmas=5.0):
    """a calibrated set: every one of the K + 1 valid bins is Binomial(d, 1 / (K + 1)) -> (mean, allowed deviation)"""
    p = 1.0 / (k + 1)
    return d * p, sigmas * np.sqrt(d * p * (1.0 - p))


# ------------------------------------------------------------------ the input sets of the tests
SETS = ("rand", "img", "dup", "same", "ties", "inf")


def make_set(kind, images, k, shape, seed=0):
    """-> (x [images k, *shape], y [images, *shape]) fp32.  rand: normal; img: smooth values in [-1, 1]; dup: every
    particle a copy of one of two (what a resampling leaves); same: every particle a copy of one; ties: values from
    {-1, -0.0, +0.0, 1}; inf: normal with +-Inf sprinkled in (particles and label)"""
    rng = np.random.default_rng(1000 * seed + 17 * k + images + sum(shape))
    full = (images, k) + tuple(shape)
    y = rng.standard_normal((images,) + tuple(shape)).astype(np.float32)
    if kind == "rand":
        x = rng.standard_normal(full)
    elif kind == "img":
        c, h, w = shape
        yy, xx = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 2, w), indexing="ij")
        base = np.sin(yy)[None] * np.cos(xx + np.arange(c)[:, None, None])
        x = np.clip(base[None, None] + 0.2 * rng.standard_normal(full), -1, 1)
        y = np.clip(np.broadcast_to(base, y.shape) + 0.2 * y, -1, 1)
    elif kind in ("dup", "same"):
        src = rng.standard_normal((images, 2) + tuple(shape))
        pick = rng.integers(0, 2, size=(images, k)) if kind == "dup" else np.zeros((images, k), dtype=np.int64)
        x = np.stack([src[m][pick[m]] for m in range(images)])
    elif kind == "ties":
        vals = np.array([-1.0, -0.0, 0.0, 1.0], dtype=np.float32)
        x = vals[rng.integers(0, 4, size=full)]
        y = vals[rng.integers(0, 4, size=y.shape)]
    elif kind == "inf":
        x = rng.standard_normal(full)
        r = rng.random(full)
        x[r < 0.05] = np.inf
        x[r > 0.95] = -np.inf
        ry = rng.random(y.shape)
        y[ry < 0.03] = np.inf
        y[ry > 0.97] = -np.inf
    else:
        raise ValueError(kind)
    x = np.ascontiguousarray(x, dtype=np.float32).reshape((images * k,) + tuple(shape))
    return x, np.ascontiguousarray(y, dtype=np.float32)
