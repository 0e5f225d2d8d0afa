"""CPU suite of the device image metrics: the float64 restatement tests/metrics_ref.py (the reference of the GPU suite)
against a brute-force window and against SciPy's Gaussian filter, its fixed points, best_of_n_curve, the two names in the
header / the exports / the ctypes table, every refusal of dpsx_image_metrics_f32 without a GPU, and the driver's flag."""
import ctypes
import os
import re
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import metrics_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dpsx_metrics_workspace_bytes", "dpsx_image_metrics_f32")


# ----------------------------------------------------------------- the restatement
def _brute_ssim(x, y, L):
    """the definition as a direct 11 x 11 double loop per position (one plane pair)"""
    g = metrics_ref.taps()
    h, w = x.shape
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    total = 0.0
    for i in range(h - 10):
        for j in range(w - 10):
            mx = my = exx = eyy = exy = 0.0
            for a in range(11):
                for b in range(11):
                    wt, u, v = g[a] * g[b], float(x[i + a, j + b]), float(y[i + a, j + b])
                    mx += wt * u
                    my += wt * v
                    exx += wt * u * u
                    eyy += wt * v * v
                    exy += wt * u * v
            vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
            total += (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    return total / ((h - 10) * (w - 10))


def test_restatement_equals_the_brute_force_window():
    rng = np.random.RandomState(0)
    y = rng.uniform(-1, 1, (1, 1, 13, 17)).astype(np.float32)
    x = (y + 0.1 * rng.randn(*y.shape)).astype(np.float32)
    assert abs(metrics_ref.taps().sum() - 1.0) < 1e-15
    for dr in (None, 2.0):
        L = float(metrics_ref.label_range(y, dr)[0])
        assert abs(metrics_ref.ssim(x, y, dr)[0] - _brute_ssim(x[0, 0], y[0, 0], L)) < 1e-13


def test_restatement_equals_scipy_gaussian_filter():
    """skimage's construction: gaussian_filter(sigma=1.5, truncate=3.5) -- an 11-tap window -- cropped by 5 on each side"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.RandomState(1)
    y = rng.uniform(-1, 1, (1, 3, 40, 52))
    x = y + 0.2 * rng.randn(*y.shape)
    L = 2.0
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2

    def f(a):
        return np.stack([gaussian_filter(p, sigma=1.5, truncate=3.5, mode="reflect")[5:-5, 5:-5] for p in a])
    mx, my = f(x[0]), f(y[0])
    vx, vy, cxy = f(x[0] * x[0]) - mx * mx, f(y[0] * y[0]) - my * my, f(x[0] * y[0]) - mx * my
    s = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
    ours = metrics_ref.ssim_map(x, y, L)[0]
    assert ours.shape == s.shape == (3, 30, 42)
    assert np.abs(ours - s).max() <= 1e-12
    assert abs(metrics_ref.ssim(x, y, L)[0] - s.mean()) <= 1e-12


def test_restatement_fixed_points():
    rng = np.random.RandomState(2)
    y = rng.uniform(-1, 1, (2, 3, 16, 20)).astype(np.float32)
    assert np.abs(metrics_ref.ssim(y, y) - 1.0).max() < 1e-12
    assert np.abs(metrics_ref.ssim(np.repeat(y, 2, axis=0), y) - 1.0).max() < 1e-12        # image-major rows
    # by hand: label 0 / 1 halves (range 1), x = label + 0.1 everywhere: mse = 0.01, psnr = 10 log10(1 / 0.01) = 20 dB
    lab = np.zeros((1, 1, 4, 4), dtype=np.float32)
    lab[..., 2:] = 1.0
    x = lab.astype(np.float64) + 0.1
    assert abs(metrics_ref.mse(x, lab)[0] - 0.01) < 1e-15 and abs(metrics_ref.psnr(x, lab)[0] - 20.0) < 1e-12
    assert abs(metrics_ref.psnr(x, lab, data_range=2.0)[0] - (20.0 + 20.0 * np.log10(2.0))) < 1e-12
    assert metrics_ref.psnr(lab, lab)[0] == np.inf
    const = np.full((1, 1, 4, 4), 0.5, dtype=np.float32)                                   # L = 0
    assert metrics_ref.psnr(const + 0.1, const)[0] == -np.inf and np.isnan(metrics_ref.psnr(const, const)[0])
    # the fp32 form of the same expression exists and is close
    y32 = rng.uniform(-1, 1, (1, 1, 24, 24)).astype(np.float32)
    x32 = (y32 + 0.1 * rng.randn(*y32.shape)).astype(np.float32)
    lo = metrics_ref.ssim(x32, y32, dtype=np.float32)
    assert lo.dtype == np.float32 and abs(float(lo[0]) - metrics_ref.ssim(x32, y32)[0]) < 1e-5


def test_best_of_n_curve_by_hand():
    from dps_ttc_amd.metrics import best_of_n_curve
    nan = float("nan")
    #        pick: 0    0    2    2 (tie: first)  4 (NaN first)  4    4 (first NaN stays)
    d = np.array([3.0, 5.0, 2.0, 2.0, nan, 1.0, nan])
    v = np.array([10.0, 11.0, 12.0, 13.0, 14.0, 15.0, 16.0])
    want = np.array([10.0, 10.0, 12.0, 12.0, 14.0, 14.0, 14.0])
    got = best_of_n_curve(d, v)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(got, np.array([v[np.argmin(d[:n])] for n in range(1, len(d) + 1)]))    # the prefix rule itself
    rng = np.random.RandomState(3)
    d = rng.randint(0, 5, 40).astype(np.float32)
    d[rng.rand(40) < 0.1] = nan
    v = rng.randn(40).astype(np.float32)
    got = best_of_n_curve(d, v)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([v[np.argmin(d[:n])] for n in range(1, 41)]))
    with pytest.raises(ValueError):
        best_of_n_curve(d, v[:-1])


# ----------------------------------------------------------------- the ABI
def test_header_export_and_signature():
    from dps_ttc_amd import _lib
    hdr_full = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    assert "compute_metrics.py:77-90" in hdr_full and "best_of_n_simple.py:20-40" in hdr_full
    p, i64 = ctypes.c_void_p, ctypes.c_int64
    assert _lib.SIGNATURES[NAMES[0]] == (i64, [i64] * 5)
    assert _lib.SIGNATURES[NAMES[1]] == (ctypes.c_int, [p, p, i64, ctypes.c_float, p, p, p, i64, i64, i64, i64, p, i64, p])


def test_image_metrics_refuses_on_the_host():
    """every DPSX_EINVAL / DPSX_EWORKSPACE / DPSX_EUNSUPPORTED of dpsx_image_metrics_f32, with pointers that must never be
    dereferenced: there is no GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, q = _lib.lib(), c_void_p(0x1000)

    def call(x=q, label=q, m=1, dr=0.0, mse=q, psnr=q, ssim=q, n=4, c=3, h=16, w=16, ws=q, wsb=None):
        if wsb is None:
            wsb = max(int(lib.dpsx_metrics_workspace_bytes(n, max(m, 1), c, h, w)), 0)
        return lib.dpsx_image_metrics_f32(x, label, m, dr, mse, psnr, ssim, n, c, h, w, ws, wsb, None)

    for kw in (dict(x=None), dict(label=None), dict(ws=None), dict(mse=None, psnr=None, ssim=None), dict(m=0), dict(m=-1),
               dict(m=3), dict(dr=-1.0), dict(dr=float("nan")), dict(dr=float("inf")), dict(dr=float("-inf")),
               dict(h=10), dict(w=10), dict(h=10, mse=None, psnr=None), dict(c=0), dict(h=0), dict(n=-1)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(wsb=0) == _lib.EWORKSPACE
    need = int(lib.dpsx_metrics_workspace_bytes(4, 1, 3, 16, 16))
    assert need > 0 and call(wsb=need - 1) == _lib.EWORKSPACE
    assert call(n=65536, wsb=1 << 40) == _lib.EUNSUPPORTED
    assert call(n=0) == _lib.OK                                    # nothing to do, nothing launched
    # the workspace grows with the batch, not with its split into images beyond the range partials
    assert lib.dpsx_metrics_workspace_bytes(8, 2, 3, 64, 64) >= lib.dpsx_metrics_workspace_bytes(4, 1, 3, 64, 64)
    assert lib.dpsx_metrics_workspace_bytes(4, 3, 3, 16, 16) == _lib.EINVAL
    assert lib.dpsx_metrics_workspace_bytes(65536, 1, 3, 16, 16) == _lib.EUNSUPPORTED


def test_front_end_refuses_bad_arguments_before_the_library():
    from dps_ttc_amd import kernels
    x = torch.zeros(4, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        kernels.image_metrics(x, x[:1])
    for want in ((), ("lpips",), ("psnr", "psnr")):
        with pytest.raises(ValueError, match="want"):
            kernels.image_metrics(x, x[:1], want=want)


# ----------------------------------------------------------------- the driver
def _driver():
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    return drv


def test_driver_path_metrics_defaults_to_torch():
    drv = _driver()
    assert drv.parse_args([]).path_metrics == "torch"
    assert drv.parse_args(["--path_metrics", "device"]).path_metrics == "device"
    with pytest.raises(SystemExit):
        drv.parse_args(["--path_metrics", "host"])


def test_driver_rejects_device_path_metrics_on_several_ranks_before_gpu_work(tmp_path, monkeypatch):
    drv = _driver()

    def no_gpu(*a, **kw):
        raise AssertionError("the driver touched the GPU before rejecting the arguments")
    for fn in ("is_available", "set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    monkeypatch.setenv("WORLD_SIZE", "2")
    argv = ["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config",
            os.path.join(ROOT, "configs", "diffusion_config.yaml"), "--task_config",
            os.path.join(ROOT, "configs", "gaussian_deblur_config.yaml"), "--save_dir", str(tmp_path / "out")]
    with pytest.raises(SystemExit) as e:
        drv.main(argv + ["--path_metrics", "device"])
    msg = str(e.value)
    assert "--path_metrics device" in msg and "WORLD_SIZE=2" in msg and "\n" not in msg
    with pytest.raises(SystemExit) as e:
        drv.parse_args(["--path_metrics", "device"])
    assert "one rank only" in str(e.value)


def test_driver_writes_the_curves_in_path_order(tmp_path):
    drv = _driver()
    d = np.array([3.0, 1.0, 2.0], dtype=np.float32)
    drv.save_path_metrics(str(tmp_path), "00007", d, [20.0, 30.0, 25.0], [0.5, 0.9, 0.7])
    assert np.array_equal(np.load(tmp_path / "00007_pathwise_psnr.npy"), np.array([20.0, 30.0, 25.0], dtype=np.float32))
    assert np.array_equal(np.load(tmp_path / "00007_best_of_n_psnr.npy"), np.array([20.0, 30.0, 30.0], dtype=np.float32))
    assert np.array_equal(np.load(tmp_path / "00007_best_of_n_ssim.npy"), np.array([0.5, 0.9, 0.9], dtype=np.float32))
    assert np.load(tmp_path / "00007_pathwise_ssim.npy").shape == d.shape
