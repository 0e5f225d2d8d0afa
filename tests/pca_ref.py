"""Float64 restatement of the principal components (include/dpsx.h "principal components"): the reference of
tests/test_pca_gpu.py and the subject of tests/test_pca_cpu.py.  numpy only.

Per image: centre the K particles, G = Xc Xc^T, eigh in descending order, the null rule l_j <= K 2^-23 l_0, the sign rule
(the entry of largest magnitude of every eigenvector is positive, the lowest index wins ties), coords = sqrt(l_j) v_ij,
dirs = (sum_i c_ij (x_i - x_0)) / l_j.  The degenerate images are decided as the header states them: one particle or all
particles equal -> zeros and rank 0; a NaN or Inf in the image -> NaN and rank -1."""
import numpy as np

MAX_K, MAX_Q = 128, 8
SETS = ("planted", "iid", "dup", "same", "nan")
NAN_AT = (1, 2, 5)          # set `nan`: (image, particle, element), each clipped to what exists
SEED = 3                    # `planted` draws its scores: at this seed its first four components keep a relative eigen-gap
                            # >= 0.005 on every shape of tests/test_pca_gpu.py (asserted by tests/test_pca_cpu.py)


def null_threshold(k, lam0):
    return k * 2.0 ** -23 * lam0


def image_pca(x, q):
    """x [K, d] (any float dtype) -> dict of float64 arrays: evals [q], coords [K, q], dirs [q, d], info [4] =
    (trace, rank, nan, K), lam [K] (all eigenvalues, descending), gap [q] (the relative gap of component j to its
    neighbours among all K eigenvalues, inf for a null component)"""
    x64 = np.asarray(x, dtype=np.float64)
    k, d = x64.shape
    out = {"evals": np.zeros(q), "coords": np.zeros((k, q)), "dirs": np.zeros((q, d)), "lam": np.zeros(k),
           "gap": np.full(q, np.inf)}
    if not np.isfinite(x64).all() and k > 1:
        for key in ("evals", "coords", "dirs"):
            out[key][...] = np.nan
        out["info"] = np.array([np.nan, -1.0, np.nan, k])
        return out
    if k == 1 or (x64 == x64[0]).all():
        out["info"] = np.array([0.0, 0.0, np.nan, k])
        return out
    xc = x64 - x64.mean(axis=0)
    lam, v = np.linalg.eigh(xc @ xc.T)
    order = np.argsort(-lam, kind="stable")
    lam, v = lam[order], v[:, order]
    live = lam > null_threshold(k, lam[0])
    out["lam"] = lam
    out["info"] = np.array([float((xc * xc).sum()), float(live.sum()), np.nan, k])
    for j in range(min(q, k)):
        if not live[j]:
            continue
        vj = v[:, j]
        if vj[np.argmax(np.abs(vj))] < 0:
            vj = -vj
        c = np.sqrt(lam[j]) * vj
        out["evals"][j] = lam[j]
        out["coords"][:, j] = c
        out["dirs"][j] = (c @ (x64 - x64[0])) / lam[j]
        near = [lam[j - 1] - lam[j]] if j > 0 else []
        if j + 1 < k:
            near.append(lam[j] - lam[j + 1])
        out["gap"][j] = min(near) / lam[0]
    return out


def pca(x, images=1, components=4):
    """x [n, ...] image-major -> the outputs of kernels.particle_pca in float64 (dirs flat: [M, q, d]) plus "lam" [M, K]
    and "gap" [M, q]; info[:, 2] (the sweeps) is NaN: the restatement has none"""
    x = np.asarray(x)
    n = x.shape[0]
    if images < 1 or n < 1 or n % images:
        raise ValueError(f"{n} particles do not split into {images} images")
    k = n // images
    if k > MAX_K or not 1 <= components <= MAX_Q:
        raise ValueError(f"K <= {MAX_K} and 1 <= q <= {MAX_Q} (got {k}, {components})")
    per = [image_pca(x[m * k:(m + 1) * k].reshape(k, -1), components) for m in range(images)]
    res = {key: np.stack([p[key] for p in per]) for key in ("evals", "coords", "dirs", "info", "lam", "gap")}
    with np.errstate(all="ignore"):
        res["var"] = res["evals"] / k
        res["explained"] = res["evals"] / res["info"][:, 0:1]
    return res


def make_set(name, m, k, shape, seed=SEED):
    """-> x [m k, *shape] float32, image-major.
    planted: a base image in [-1, 1] + six orthonormal directions with amplitudes 0.2 sqrt(D) 2^-j times N(0, 1) scores +
    0.002 N(0, 1); iid: base + 0.1 N(0, 1); dup: copies of two particles (the first ceil(K / 2) are one, the rest the
    other); same: copies of one; nan: planted with one NaN at NAN_AT"""
    if name not in SETS:
        raise ValueError(name)
    d = int(np.prod(shape))
    x = np.empty((m, k, d), dtype=np.float32)
    for b in range(m):
        r = np.random.default_rng([seed, b, k, d])
        base = r.uniform(-1.0, 1.0, d)
        if name in ("planted", "nan"):
            nd = min(6, d)
            u, _ = np.linalg.qr(r.standard_normal((d, nd)))
            amp = 0.2 * np.sqrt(d) * 0.5 ** np.arange(nd)
            x[b] = base + (r.standard_normal((k, nd)) * amp) @ u.T + 0.002 * r.standard_normal((k, d))
        elif name == "iid":
            x[b] = base + 0.1 * r.standard_normal((k, d))
        elif name == "dup":
            two = (base + 0.1 * r.standard_normal((2, d))).astype(np.float32)
            x[b] = two[(np.arange(k) >= (k + 1) // 2).astype(int)]
        else:
            x[b] = base.astype(np.float32)
    if name == "nan":
        x[min(NAN_AT[0], m - 1), min(NAN_AT[1], k - 1), min(NAN_AT[2], d - 1)] = np.nan
    return x.reshape((m * k,) + tuple(shape))


def dup_counts(k):
    """set `dup`: (n_a, n_b)"""
    return (k + 1) // 2, k - (k + 1) // 2
