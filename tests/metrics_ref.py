"""The image metrics of include/dpsx.h ("reconstruction metrics") restated in numpy, float64 by default: the yardstick of
tests/test_metrics_cpu.py and tests/test_metrics_gpu.py.  dtype=np.float32 evaluates the same expression in fp32 (every
array and every operation): how far fp32 arithmetic alone moves a result, the scale a kernel's error is read against."""
import numpy as np

WIN, SIGMA = 11, 1.5


def taps():
    """g_k ~ exp(-(k - 5)^2 / (2 sigma^2)), k = 0 .. 10, normalised to sum 1, in double"""
    k = np.arange(WIN, dtype=np.float64) - (WIN - 1) / 2
    g = np.exp(-(k * k) / (2.0 * SIGMA * SIGMA))
    return g / g.sum()


def label_range(label, data_range=None):
    """L per label row [M]: data_range if given above 0, else max - min of the (fp32) label, one fp32 subtraction"""
    label = np.asarray(label)
    m = label.shape[0]
    if data_range is not None and data_range > 0:
        return np.full(m, np.float32(data_range), dtype=np.float32)
    flat = label.reshape(m, -1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (flat.max(axis=1) - flat.min(axis=1)).astype(np.float32)


def _rows(x, label):
    x, label = np.asarray(x), np.asarray(label)
    if label.ndim == 3:
        label = label[None]
    n, m = x.shape[0], label.shape[0]
    assert x.ndim == 4 and label.shape[1:] == x.shape[1:] and m >= 1 and n % m == 0
    return x, label, np.arange(n) // (n // m)


def mse(x, label, dtype=np.float64):
    x, label, row = _rows(x, label)
    d = x.astype(dtype) - label[row].astype(dtype)
    return (d * d).reshape(x.shape[0], -1).mean(axis=1, dtype=dtype)


def psnr(x, label, data_range=None, dtype=np.float64):
    """10 log10(L^2 / mse) as written: mse = 0 gives +inf, L = 0 gives -inf or NaN"""
    x, label, row = _rows(x, label)
    L = label_range(label, data_range)[row].astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(L * L / mse(x, label, dtype))


def _window_valid(a, g):
    """the separable window over the last two axes at the positions where it lies inside: horizontal, then vertical, the
    taps added in order k = 0 .. 10"""
    h, w = a.shape[-2:]
    t = np.zeros(a.shape[:-1] + (w - WIN + 1,), dtype=a.dtype)
    for k in range(WIN):
        t = t + g[k] * a[..., k:k + w - WIN + 1]
    o = np.zeros(a.shape[:-2] + (h - WIN + 1, w - WIN + 1), dtype=a.dtype)
    for k in range(WIN):
        o = o + g[k] * t[..., k:k + h - WIN + 1, :]
    return o


def ssim_map(x, label, data_range=None, dtype=np.float64):
    """s at every window position: [N, C, H - 10, W - 10]"""
    x, label, row = _rows(x, label)
    assert x.shape[-2] >= WIN and x.shape[-1] >= WIN
    g = taps().astype(dtype)
    L = label_range(label, data_range)[row].astype(np.float64)
    c1 = ((0.01 * L) ** 2).astype(dtype)[:, None, None, None]
    c2 = ((0.03 * L) ** 2).astype(dtype)[:, None, None, None]
    a, b = x.astype(dtype), label[row].astype(dtype)
    mx, my = _window_valid(a, g), _window_valid(b, g)
    exx, eyy, exy = _window_valid(a * a, g), _window_valid(b * b, g), _window_valid(a * b, g)
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    two = dtype(2.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ((two * mx * my + c1) * (two * cxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim(x, label, data_range=None, dtype=np.float64):
    s = ssim_map(x, label, data_range, dtype)
    return s.reshape(s.shape[0], -1).mean(axis=1, dtype=dtype)


def metrics(x, label, data_range=None):
    """{"mse", "psnr", "ssim"} in float64 (ssim only where the window fits)"""
    out = {"mse": mse(x, label), "psnr": psnr(x, label, data_range)}
    if np.asarray(x).shape[-2] >= WIN and np.asarray(x).shape[-1] >= WIN:
        out["ssim"] = ssim(x, label, data_range)
    return out
