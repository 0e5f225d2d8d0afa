"""Float64 restatement of the ensemble statistics (include/dpsx.h "ensemble statistics"): the reference of
tests/test_ensemble_gpu.py and the subject of tests/test_ensemble_cpu.py.  numpy only.

x [N, ...] float32 particles, image-major: M = images images of K = N / M particles, D elements each.  Per image:
    w_i      = 1, or with E: exp(-(E_i - E_min)) (the difference in float32, E_min over the finite entries, w_i = 0 for a
               non-finite E_i), normalised by W = sum w and rounded to float32; no finite E_i: the uniform form
    ESS      = W^2 / sum w^2 (uniform: T)
    c        = mean0 with a prior, else the image's first particle
    S1, S2   = sum w (x - c), sum w (x - c)^2
    uniform  T = count0 + K: mean = c + S1 / T, var = max((var0 count0 + S2 - S1^2 / T) / T, 0)
    weighted mean = c + S1, var = max(S2 - S1^2, 0)
    curve[n - 1] = mean_e (c + (sum_{i <= n} (x_i - c)) r_n - y)^2, r_n = 1 / (count0 + n) rounded to double once,
                   n = 1 .. K; final_mse the same for `mean`
    info     = (ESS, mean_e var, final_mse or NaN, T)
Everything is float64 (mean and var are NOT rounded to float32 here); NaN passes through the max."""
import numpy as np


def weights(e, images=1):
    """-> (w [M, K] float64 holding the float32 normalised weights, ess [M], uniform [M] bool)"""
    e = np.asarray(e, dtype=np.float32).reshape(images, -1)
    k = e.shape[1]
    w, ess, uni = np.ones((images, k)), np.full(images, float(k)), np.zeros(images, dtype=bool)
    for m in range(images):
        fin = np.isfinite(e[m])
        if not fin.any():
            uni[m] = True
            continue
        diff = np.where(fin, e[m] - e[m][fin].min(), np.float32(0)).astype(np.float32)
        raw = np.where(fin, np.exp(-diff.astype(np.float64)), 0.0)
        tot = 0.0
        for v in raw:                      # index order
            tot += v
        ess[m] = tot * tot / float((raw * raw).sum())
        w[m] = (raw / tot).astype(np.float32).astype(np.float64)
    return w, ess, uni


def _clamp0(v):
    return np.where(v < 0, 0.0, v)         # max(v, 0); NaN passes


def ensemble(x, images=1, label=None, e=None, prior=None):
    """-> dict(mean, var [M, ...] float64, info [M, 4], count, and with a label curve [M, K], final_mse [M])"""
    x = np.asarray(x)
    n = x.shape[0]
    k = n // images
    shape = (images,) + x.shape[1:]
    v = x.reshape(images, k, -1).astype(np.float64)
    d = v.shape[2]
    if e is not None and prior is not None:
        raise ValueError("weights with a prior")
    count0, mean0, var0 = (0, None, None) if prior is None else prior
    count0 = float(count0)
    total = count0 + k
    w, ess, uni = weights(e, images) if e is not None else (None, np.full(images, total), np.ones(images, dtype=bool))
    mean, var = np.zeros((images, d)), np.zeros((images, d))
    curve, final = np.zeros((images, k)), np.full(images, np.nan)
    y = None
    if label is not None:
        y = np.broadcast_to(np.asarray(label, dtype=np.float64).reshape(-1, d), (images, d))
    with np.errstate(all="ignore"):
        for m in range(images):
            c = np.asarray(mean0, dtype=np.float64).reshape(images, d)[m] if count0 > 0 else v[m, 0]
            diff = v[m] - c[None, :]
            if uni[m]:
                s1, s2 = diff.sum(axis=0), (diff * diff).sum(axis=0)
                m2 = (np.asarray(var0, dtype=np.float64).reshape(images, d)[m] * count0 if count0 > 0 else 0.0) + s2 \
                    - s1 * s1 / total
                mean[m], var[m] = c + s1 / total, _clamp0(m2 / total)
            else:
                s1, s2 = (w[m][:, None] * diff).sum(axis=0), (w[m][:, None] * diff * diff).sum(axis=0)
                mean[m], var[m] = c + s1, _clamp0(s2 - s1 * s1)
            if y is not None:
                pm = c[None, :] + np.cumsum(diff, axis=0) * (1.0 / (count0 + np.arange(1, k + 1)))[:, None]
                curve[m] = ((pm - y[m][None, :]) ** 2).mean(axis=1)
                final[m] = ((mean[m] - y[m]) ** 2).mean()
    info = np.stack([ess if e is not None else np.full(images, total), var.mean(axis=1), final, np.full(images, total)], axis=1)
    res = {"mean": mean.reshape(shape), "var": var.reshape(shape), "info": info, "count": int(total)}
    if y is not None:
        res["curve"], res["final_mse"] = curve, final
    return res


def two_pass_variance(x, images=1):
    """the biased variance in long double, two passes: what the shifted sums are measured against"""
    v = np.asarray(x).reshape(images, x.shape[0] // images, -1).astype(np.longdouble)
    mu = v.mean(axis=1, keepdims=True)
    return ((v - mu) ** 2).mean(axis=1)


def mean_of_n_psnr(curve, data_range):
    """10 log10(L^2 / curve) per image row, L as metrics.compute_psnr defines it (max - min of the label)"""
    with np.errstate(all="ignore"):
        return 10.0 * np.log10(np.asarray(data_range, dtype=np.float64).reshape(-1, 1) ** 2 / np.asarray(curve, dtype=np.float64))
