"""CPU suite of the order statistics (include/dpsx.h "order statistics"): the float64 restatement tests/quantile_ref.py
against numpy's sort and quantile and against closed forms, the calibration property on the restatement (the GPU test
repeats it with the same seed, so it cannot be the one that decides it), the names in the header / the exports / the ctypes
table, every refusal of the entry points without a GPU, and the driver's flag and refusals."""
import ctypes
import importlib
import os
import re
from ctypes import c_double, c_void_p

import numpy as np
import pytest
import torch

import quantile_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dpsx_quantiles_workspace_bytes", "dpsx_quantiles_f32")
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)
CAL = dict(images=1, k=16, shape=(3, 32, 32), seed=7)        # the calibration case, shared with tests/test_quantile_gpu.py


def ulp_distance(a, b):
    """distance in fp32 steps between finite values of equal sign or zero"""
    ka, kb = Q.order_key(a).astype(np.int64), Q.order_key(b).astype(np.int64)
    return np.abs(ka - kb)


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("k", (1, 2, 3, 16, 65))
def test_restatement_against_numpy(k):
    """on data without NaN and without signed zeros: the sorted values are np.sort's, the quantiles np.quantile's (linear,
    float64 on the fp32 values) to 1 ulp of fp32"""
    x, _ = Q.make_set("rand", 2, k, (1, 5, 7), seed=k)
    r = Q.order_stats(x, images=2, probs=PROBS)
    flat = x.reshape(2, k, -1)
    for m in range(2):
        assert np.array_equal(Q.sort_particles(flat[m]), np.sort(flat[m], axis=0))
        ref = np.quantile(flat[m].astype(np.float64), PROBS, axis=0, method="linear").astype(np.float32)
        got = r["quantiles"][m].reshape(len(PROBS), -1)
        assert ulp_distance(got, ref).max() <= 1
        assert np.array_equal(got[0], flat[m].min(axis=0)) and np.array_equal(got[-1], flat[m].max(axis=0))
    assert (r["info"][:, 3] == k).all() and np.isnan(r["info"][:, 0]).all() and (r["info"][:, 2] == 0).all()
    assert "hist" not in r


def test_closed_forms():
    x, y = Q.make_set("rand", 1, 2, (1, 4, 4), seed=1)                      # K = 2, p = 0.5: the midpoint
    r = Q.order_stats(x, probs=(0.5,), label=y)
    a, b = x.astype(np.float64)
    assert np.array_equal(r["quantiles"][0, 0], ((a + b) / 2).astype(np.float32))
    # K = 2 CRPS: (|a - y| + |b - y|) / 2 - |a - b| / 4
    want = (np.abs(a - y[0]) + np.abs(b - y[0])) / 2 - np.abs(a - b) / 4
    np.testing.assert_allclose(r["crps_e"][0], want.reshape(-1), rtol=2e-7, atol=1e-12)
    x1, y1 = Q.make_set("rand", 1, 1, (1, 4, 4), seed=2)                    # K = 1: every quantile is x, crps = |x - y|
    r = Q.order_stats(x1, probs=PROBS, label=y1)
    assert all(np.array_equal(r["quantiles"][0, i], x1[0]) for i in range(len(PROBS)))
    assert np.array_equal(r["crps_e"][0], np.abs(x1[0] - y1[0]).reshape(-1))
    assert r["info"][0, 1] == 0 and r["hist"].shape == (1, 3) and r["hist"][0, :2].sum() == 16


@pytest.mark.parametrize("k", (2, 5, 64, 130))
def test_equal_particles(k):
    """every quantile equals the value, bits kept, crps_e = |x - y| exactly, width exactly 0"""
    x, y = Q.make_set("same", 2, k, (1, 6, 5), seed=k)
    r = Q.order_stats(x, images=2, probs=PROBS, label=y)
    for m in range(2):
        for i in range(len(PROBS)):
            assert np.array_equal(r["quantiles"][m, i].view(np.int32), x[m * k].view(np.int32))
        assert np.array_equal(r["crps_e"][m], np.abs(x[m * k].astype(np.float64) - y[m]).astype(np.float32).reshape(-1))
    assert (r["info"][:, 1] == 0).all() and not np.signbit(r["info"][:, 1]).any()


@pytest.mark.parametrize("kind", Q.SETS)
def test_histogram(kind):
    k, shape = 6, (1, 9, 11)
    d = int(np.prod(shape))
    x, y = Q.make_set(kind, 2, k, shape, seed=4)
    r = Q.order_stats(x, images=2, label=y)
    assert r["hist"].shape == (2, k + 2) and (r["hist"].sum(axis=1) == d).all()
    lo = Q.order_stats(x, images=2, label=np.full_like(y, -np.inf))["hist"]
    hi = Q.order_stats(x, images=2, label=np.full_like(y, np.inf))["hist"]
    if kind != "inf":                      # a particle at +Inf is not below a label at +Inf
        assert (lo[:, 0] == d).all() and (hi[:, k] == d).all()
    else:
        assert (lo[:, 0] == d).all() and (hi[:, :k + 1].sum(axis=1) == d).all() and (hi[:, k] < d).all()
    assert Q.interval_coverage(r["hist"], 0, k).tolist() == [1.0, 1.0]


def test_nan_goes_to_its_own_bin_and_its_own_element():
    k, shape = 5, (1, 4, 6)
    x, y = Q.make_set("rand", 3, k, shape, seed=5)
    clean = Q.order_stats(x, images=3, probs=PROBS, label=y)
    xn, yn = x.copy(), y.copy()
    xn[k + 2, 0, 1, 3] = np.nan            # a particle of image 1
    yn[2, 0, 3, 5] = np.nan                # the label of image 2
    r = Q.order_stats(xn, images=3, probs=PROBS, label=yn)
    assert r["hist"][:, k + 1].tolist() == [0, 1, 1] and (r["hist"].sum(axis=1) == 24).all()
    assert (r["quantiles"][1, :, 0, 1, 3].view(np.int32) == 0x7fc00000).all()
    mask = np.ones(r["quantiles"].shape, dtype=bool)
    mask[1, :, 0, 1, 3] = False
    assert np.array_equal(r["quantiles"].view(np.int32)[mask], clean["quantiles"].view(np.int32)[mask])
    assert not np.isnan(r["quantiles"][2]).any()           # a NaN label leaves the quantiles alone
    assert r["info"][:, 2].tolist() == [0, 1, 1] and r["info"][0].tolist() == clean["info"][0].tolist()
    assert np.isfinite(r["info"][:, :2]).all()


def test_signed_zeros_are_ordered():
    x = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], dtype=np.float32).reshape(6, 1, 1, 1)
    xs = Q.sort_particles(x.reshape(6, 1))
    assert np.signbit(xs[:, 0]).tolist() == [True, True, True, False, False, False] and xs[0, 0] == -1 and xs[5, 0] == 1
    r = Q.order_stats(x, probs=(0.2, 0.3, 0.4, 0.6), label=np.zeros((1, 1, 1, 1), dtype=np.float32))
    got = r["quantiles"].reshape(-1)
    assert (got == 0).all() and np.signbit(got).tolist() == [True, True, True, False]     # a == b keeps a's bits
    assert r["hist"][0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]                                # only -1 is below +0.0


def test_infinities_follow_ieee():
    x = np.array([-np.inf, -np.inf, 1.0, np.inf], dtype=np.float32).reshape(4, 1, 1, 1)
    r = Q.order_stats(x, probs=(0.0, 0.2, 0.5, 0.9, 1.0))
    got = r["quantiles"].reshape(-1)
    assert got[0] == -np.inf and got[1] == -np.inf and got[3] == np.inf and got[4] == np.inf
    assert got[2:3].view(np.int32)[0] == 0x7fc00000        # -Inf + 0.5 (1 - -Inf) = -Inf + Inf
    r = Q.order_stats(np.array([-np.inf, np.inf], dtype=np.float32).reshape(2, 1, 1, 1), probs=(0.5,))
    assert r["quantiles"].view(np.int32).reshape(-1).tolist() == [0x7fc00000]
    assert np.isnan(r["info"][0, 1])       # no element of finite width


def test_calibration_of_the_restatement():
    """i.i.d. normal particles and label: every one of the K + 1 valid bins holds d / (K + 1) within 5 standard deviations
    of the binomial count; interval_coverage is the integer arithmetic it says it is"""
    from dps_ttc_amd import metrics
    x, y = Q.make_set("rand", CAL["images"], CAL["k"], CAL["shape"], seed=CAL["seed"])
    k, d = CAL["k"], int(np.prod(CAL["shape"]))
    hist = Q.order_stats(x, label=y)["hist"]
    mean, dev = Q.calibration_bounds(d, k)
    print(f"bins {hist[0, :k + 1].tolist()} against {mean:.1f} +- {dev:.1f}")
    assert hist[0, k + 1] == 0 and (np.abs(hist[0, :k + 1] - mean) <= dev).all()
    cov = metrics.interval_coverage(hist, 1, k - 1)
    assert cov.shape == (1,) and cov[0] == hist[0, 1:k].sum() / d == Q.interval_coverage(hist, 1, k - 1)[0]
    assert metrics.interval_coverage(torch.from_numpy(hist[0]), 0, k) == 1.0
    with pytest.raises(ValueError):
        metrics.interval_coverage(hist, 3, 2)
    with pytest.raises(ValueError):
        metrics.interval_coverage(hist.astype(np.float32), 0, 1)


def test_restatement_refuses():
    x = np.zeros((4, 1, 2, 2), dtype=np.float32)
    for kw in (dict(images=3), dict(probs=()), dict(probs=(0.1,) * 9), dict(probs=(1.5,)), dict(probs=(float("nan"),))):
        with pytest.raises(ValueError):
            Q.order_stats(x, **kw)


# ------------------------------------------------------------------ the ABI
def test_header_exports_and_signatures():
    from dps_ttc_amd import _lib
    text = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    assert re.search(r"/\* ---- order statistics", text)
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    assert _lib.SIGNATURES["dpsx_quantiles_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["dpsx_quantiles_f32"][1]) == 13
    assert "quantile.hip" in open(os.path.join(ROOT, "dps_ttc_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_on_the_host():
    """every DPSX_EINVAL / DPSX_EUNSUPPORTED / DPSX_EWORKSPACE, with pointers that must never be dereferenced: there is no
    GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, p = _lib.lib(), c_void_p(0x100000)
    big = 1 << 40

    def call(x=p, y=p, probs=(0.05, 0.5, 0.95), q=None, quant=p, hist=p, info=p, n=8, d=64, images=2, ws=p, wsb=big):
        arr = None if probs is None else (c_double * max(len(probs), 1))(*probs)
        return lib.dpsx_quantiles_f32(x, y, arr, len(probs) if q is None else q, quant, hist, info, n, d, images, ws, wsb, None)

    nan = float("nan")
    for kw in (dict(x=None), dict(quant=None), dict(info=None), dict(ws=None), dict(probs=None, q=3), dict(probs=(), q=0),
               dict(probs=(0.5,) * 9), dict(q=-1), dict(probs=(0.5, 1.0000001)), dict(probs=(-1e-9,)), dict(probs=(nan,)),
               dict(y=None, hist=p), dict(n=0), dict(n=-2), dict(n=9), dict(n=7), dict(d=0), dict(images=0)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(n=513, images=1) == _lib.EUNSUPPORTED and call(n=3 * 513, images=3) == _lib.EUNSUPPORTED
    assert call(d=1 << 31) == _lib.EUNSUPPORTED and call(n=65536, images=65536) == _lib.EUNSUPPORTED
    assert call(wsb=16) == _lib.EWORKSPACE and call(y=None, hist=None, wsb=16) == _lib.EWORKSPACE
    wsb = lib.dpsx_quantiles_workspace_bytes
    assert wsb(513, 64, 1) == _lib.EUNSUPPORTED and wsb(9, 64, 2) == _lib.EINVAL and wsb(8, 0, 2) == _lib.EINVAL
    assert wsb(512, 16, 1) > 0 and wsb(8, 64, 2) > 0
    assert call(wsb=wsb(8, 64, 2) - 1) == _lib.EWORKSPACE
    assert call(probs=(0.5, nan), wsb=16) == _lib.EINVAL       # the arguments come before the workspace


def test_front_ends_refuse_cpu_tensors_and_bad_options():
    from dps_ttc_amd import kernels, metrics
    x = torch.zeros(4, 3, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        kernels.order_stats(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        metrics.posterior_quantiles(torch.zeros(1, 3, 16, 16), x)
    with pytest.raises(ValueError, match="reference images"):
        metrics.posterior_quantiles(torch.zeros(1, 3, 16, 16), x, n_images=2)
    assert kernels.QUANTILE_MAX_K == 512 and kernels.QUANTILE_MAX_Q == 8
    assert kernels.QUANTILE_INFO == ("crps", "width", "invalid", "count")
    assert kernels.quantile_probs((0.05, 0.5)) == [0.05, 0.5] and kernels.quantile_probs(0.5) == [0.5]
    for bad in ((), (0.5,) * 9, (1.5,), (-0.1,), (float("nan"),)):
        with pytest.raises(ValueError):
            kernels.quantile_probs(bad)


# ------------------------------------------------------------------ the driver
def _driver():
    import sys
    sys.path.insert(0, ROOT)
    return importlib.import_module("sample_condition_batched_ttc")


def test_driver_flag():
    drv = _driver()
    a = drv.parse_args([])
    assert a.posterior_quantiles is None and drv.check_posterior_quantiles(a, "ddpm") is None
    assert drv.check_posterior_quantiles(a, "search_ddpm", world=4) is None          # off: nothing is checked
    for name in ("ddpm", "ddim", "ttc_ddim", "smc_ddpm", None):
        ok = drv.parse_args(["--posterior_quantiles", "5,50,95", "--n_paths", "8", "--batch_size", "8"])
        assert drv.check_posterior_quantiles(ok, name) is None
    assert drv.quantile_percentages("5,50,95") == [5.0, 50.0, 95.0]
    both = drv.parse_args(["--posterior_quantiles", "0,100", "--posterior_summary", "--n_paths", "512", "--batch_size", "512"])
    assert drv.check_posterior_quantiles(both, "ddpm") is None and drv.check_posterior_summary(both, "ddpm") is None

    def refused(argv, match, sampler="ddpm", world=1):
        with pytest.raises(SystemExit) as e:
            drv.check_posterior_quantiles(drv.parse_args(argv), sampler, world)
        assert re.search(match, str(e.value)) and "\n" not in str(e.value), e.value

    one = ["--n_paths", "8", "--batch_size", "8"]
    refused(["--posterior_quantiles", "5,50,95"] + one, "one rank only", world=2)
    refused(["--posterior_quantiles", "5,50,95", "--n_paths", "8", "--batch_size", "4"], "one particle group")
    refused(["--posterior_quantiles", "50", "--n_paths", "513", "--batch_size", "513"], "512")
    refused(["--posterior_quantiles", "1,2,3,4,5,6,7,8,9"] + one, "between 1 and 8")
    refused(["--posterior_quantiles", ""] + one, "between 1 and 8")
    refused(["--posterior_quantiles", "5,101"] + one, r"\[0, 100\]")
    refused(["--posterior_quantiles", "-1"] + one, r"\[0, 100\]")
    refused(["--posterior_quantiles", "nan"] + one, r"\[0, 100\]")
    refused(["--posterior_quantiles", "5,x"] + one, "separated by commas")
    refused(["--posterior_quantiles", "50"] + one, "search_ddpm", sampler="search_ddpm")


def test_driver_refuses_before_any_gpu_work(monkeypatch, tmp_path):
    """main() itself: the refusal comes before the device is asked for anything (there is none here) and writes nothing"""
    drv = _driver()
    diff = os.path.join(ROOT, "configs", "diffusion_config.yaml")
    for argv, match in ((["--posterior_quantiles", "5,50,95", "--n_paths", "8", "--batch_size", "4"], "one particle group"),
                        (["--posterior_quantiles", "150", "--n_paths", "4", "--batch_size", "4"], "0, 100")):
        with pytest.raises(SystemExit, match=match):
            drv.main(["--diffusion_config", diff, "--save_dir", str(tmp_path / "out")] + argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank only"):
        drv.main(["--diffusion_config", diff, "--save_dir", str(tmp_path / "out"), "--posterior_quantiles", "50",
                  "--n_paths", "4", "--batch_size", "4"])
    assert not (tmp_path / "out").exists()
