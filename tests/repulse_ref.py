"""Float64 restatement of particle repulsion (include/dpsx.h "particle repulsion"): the reference of tests/test_repulse_gpu.py
and the subject of tests/test_repulse_cpu.py.  numpy only.

x [N, ...] float32 particles, image-major: M = images images of K = N / M particles, D elements each.  Per image:
    d2[i][j] = sum_e (x_i[e] - x_j[e])^2                                  the difference form
    mean     = sum_{i<j} d2[i][j] / (K (K - 1) / 2)                       K = 1: 0;   min: the smallest pair, K = 1: +inf
    h        = bandwidth D if bandwidth > 0 else mean / ln(K + 1)
    w[i][j]  = exp(-d2[i][j] / h), w[i][i] = 0
    gain     = 2 c / h
    out_i    = x_i + gain sum_j w[i][j] (x_i - x_j)
The image is stepped iff K > 1, mean is finite, h > 0, h is finite and gain is finite in float32; otherwise it is copied, its
w is 0 and its gain is reported as 0.  c and bandwidth are taken as the float32 values the library receives."""
import numpy as np


def sqdist(x, images=1):
    """-> d2 [M, K, K] float64, the difference form"""
    x = np.asarray(x)
    n = x.shape[0]
    k = n // images
    v = x.reshape(images, k, -1).astype(np.float64)
    d2 = np.zeros((images, k, k))
    for m in range(images):
        for i in range(k):
            diff = v[m, i][None, :] - v[m, i + 1:]
            d2[m, i, i + 1:] = np.einsum("je,je->j", diff, diff)
            d2[m, i + 1:, i] = d2[m, i, i + 1:]
    return d2


def repulse(x, c, images=1, bandwidth=None):
    """-> dict(out, delta [N, ...] float64 (out - x; exactly 0 for a copied image), d2, w [M, K, K], info [M, 4] = (h, gain,
    mean, min), applied [M] bool)"""
    x = np.asarray(x)
    n = x.shape[0]
    k = n // images
    c = float(np.float32(c))
    bw = 0.0 if bandwidth is None else float(np.float32(bandwidth))
    v = x.reshape(images, k, -1).astype(np.float64)
    dim = v.shape[2]
    with np.errstate(all="ignore"):
        d2 = sqdist(x, images)
        w, delta = np.zeros((images, k, k)), np.zeros_like(v)
        info, applied = np.zeros((images, 4)), np.zeros(images, dtype=bool)
        iu = np.triu_indices(k, 1)
        for m in range(images):
            pairs = d2[m][iu]
            mean = pairs.sum() / len(pairs) if k > 1 else 0.0
            mn = (np.nan if np.isnan(pairs).any() else pairs.min()) if k > 1 else np.inf
            h = bw * dim if bw > 0 else mean / np.log(k + 1.0)
            gain = np.float64(2.0 * c) / np.float64(h) if h != 0 else (np.inf if c > 0 else np.nan)
            ok = k > 1 and np.isfinite(mean) and h > 0 and np.isfinite(h) and np.isfinite(np.float32(gain))
            info[m], applied[m] = (h, gain if ok else 0.0, mean, mn), ok
            if not ok:
                continue
            w[m] = np.exp(-d2[m] / h)
            np.fill_diagonal(w[m], 0.0)
            for i in range(k):
                delta[m, i] = gain * (w[m, i][:, None] * (v[m, i][None, :] - v[m])).sum(axis=0)
    delta = delta.reshape(x.shape)
    return {"out": x.astype(np.float64) + delta, "delta": delta, "d2": d2, "w": w, "info": info, "applied": applied}


# ------------------------------------------------------------------ the input sets (seeded)
SETS = ("rand", "img", "neardup", "dup", "far")


def make_set(name, images, k, shape, seed=0):
    """[images * k, *shape] float32.  rand: N(0, 1); img: sqrt(1/2) base + sqrt(1/2) noise (the image's particles share
    base); neardup: base + 1e-3 noise per particle; dup: rand with particle K - 1 of every image given particle 0's bits
    (K >= 2); far: rand with particle K - 1 at 50 x scale, so its weights underflow"""
    rng = np.random.RandomState(seed)
    noise = rng.randn(images, k, *shape)
    base = rng.randn(images, 1, *shape)
    if name in ("rand", "dup", "far"):
        x = noise
    elif name == "img":
        x = np.sqrt(0.5) * base + np.sqrt(0.5) * noise
    elif name == "neardup":
        x = base + 1e-3 * noise
    else:
        raise ValueError(name)
    x = np.ascontiguousarray(x.astype(np.float32))
    if name == "dup":
        x[:, k - 1] = x[:, 0]
    if name == "far":
        x[:, k - 1] *= np.float32(50.0)
    return x.reshape(images * k, *shape)


def sqdist_f32_difference(x, images=1):
    """the difference form in float32 numpy (what the kernels compute, up to the order of the sum)"""
    x = np.asarray(x, dtype=np.float32)
    k = x.shape[0] // images
    v = x.reshape(images, k, -1)
    d = v[:, :, None, :] - v[:, None, :, :]
    return np.einsum("mije,mije->mij", d, d, dtype=np.float32)


def sqdist_f32_gram(x, images=1):
    """the Gram form G_ii + G_jj - 2 G_ij in float32 numpy: what the definition rules out"""
    x = np.asarray(x, dtype=np.float32)
    k = x.shape[0] // images
    v = x.reshape(images, k, -1)
    g = np.einsum("mie,mje->mij", v, v, dtype=np.float32)
    diag = np.einsum("mii->mi", g)
    return diag[:, :, None] + diag[:, None, :] - np.float32(2.0) * g
