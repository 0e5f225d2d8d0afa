"""CPU suite of the ensemble statistics (include/dpsx.h "ensemble statistics"): the float64 restatement
tests/ensemble_ref.py against closed forms and against the pairwise distances of tests/repulse_ref.py, the names in the
header / the exports / the ctypes table, every refusal of the entry points without a GPU, the mean-of-n PSNR of a
hand-made example, and the driver's flags and refusals."""
import ctypes
import importlib
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import ensemble_ref as E
import repulse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dpsx_ensemble_workspace_bytes", "dpsx_ensemble_f32", "dpsx_ensemble_ex_f32")


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", R.SETS)
def test_shifted_sums_reproduce_the_two_pass_variance(name):
    """every input set is finite and its shifted double sums give the long-double two-pass variance to under 1e-14
    relative, element by element (an element of equal values: exactly 0 in both)"""
    x = R.make_set(name, 2, 6, (1, 7, 9), seed=3)
    assert np.isfinite(x).all()
    r = E.ensemble(x, images=2)
    ref = E.two_pass_variance(x, images=2)
    var = r["var"].reshape(2, -1)
    nz = ref > 0
    assert (var[~nz] == 0).all()
    err = np.asarray(np.abs(var - ref)[nz] / ref[nz], dtype=np.float64)
    print(f"{name}: shifted sums vs long-double two-pass, max relative error of var = {err.max():.3g}")
    assert (err < 1e-14).all()
    mu = x.reshape(2, 6, -1).astype(np.longdouble).mean(axis=1)
    assert np.abs(r["mean"].reshape(2, -1) - mu).max() <= 1e-14 * np.abs(x).max()


def test_closed_forms():
    x = R.make_set("rand", 1, 1, (1, 5, 5), seed=1)                        # K = 1: mean = x, var = 0
    r = E.ensemble(x, label=x[0] * 0.5)
    assert np.array_equal(r["mean"], x.astype(np.float64)) and (r["var"] == 0).all() and list(r["info"][0][[0, 1, 3]]) == [1, 0, 1]
    assert r["curve"].shape == (1, 1) and r["curve"][0, 0] == pytest.approx(float((0.25 * x.astype(np.float64) ** 2).mean()), rel=1e-14)
    x = R.make_set("rand", 1, 2, (1, 5, 5), seed=2)                        # K = 2: midpoint, (a - b)^2 / 4
    r = E.ensemble(x)
    a, b = x.astype(np.float64)
    np.testing.assert_allclose(r["mean"][0], (a + b) / 2, rtol=0, atol=1e-15)
    np.testing.assert_allclose(r["var"][0], (a - b) ** 2 / 4, rtol=1e-14, atol=0)
    assert np.isnan(r["info"][0, 2]) and "curve" not in r
    eq = np.repeat(R.make_set("rand", 2, 1, (1, 4, 4), seed=3), 5, axis=0)  # equal particles: +0.0 exactly
    r = E.ensemble(eq, images=2)
    assert (r["var"] == 0).all() and not np.signbit(r["var"]).any() and np.array_equal(r["mean"], eq[::5].astype(np.float64))


@pytest.mark.parametrize("name", R.SETS)
def test_variance_is_the_mean_pairwise_distance(name):
    """mean off-diagonal d2 = 2 K / (K - 1) sum_e var"""
    k = 7
    x = R.make_set(name, 2, k, (1, 6, 5), seed=4)
    d2 = R.sqdist(x, images=2)
    iu = np.triu_indices(k, 1)
    want = d2[:, iu[0], iu[1]].mean(axis=1)
    got = 2.0 * k / (k - 1) * E.ensemble(x, images=2)["var"].reshape(2, -1).sum(axis=1)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def test_merging_two_groups_through_the_prior():
    x = R.make_set("img", 2, 16, (1, 6, 6), seed=5).reshape(2, 16, -1)
    y = R.make_set("rand", 2, 1, (1, 6, 6), seed=6)
    whole = E.ensemble(x.reshape(32, 1, 6, 6), images=2, label=y)
    a = E.ensemble(x[:, :8].reshape(16, 1, 6, 6), images=2, label=y)
    b = E.ensemble(x[:, 8:].reshape(16, 1, 6, 6), images=2, label=y, prior=(a["count"], a["mean"], a["var"]))
    assert b["count"] == 16 and (b["info"][:, 3] == 16).all() and (b["info"][:, 0] == 16).all()
    for key in ("mean", "var"):
        np.testing.assert_allclose(b[key], whole[key], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(np.concatenate([a["curve"], b["curve"]], axis=1), whole["curve"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(b["final_mse"], whole["final_mse"], rtol=1e-12, atol=0)
    with pytest.raises(ValueError):
        E.ensemble(x.reshape(32, 1, 6, 6), images=2, e=np.zeros(32), prior=(a["count"], a["mean"], a["var"]))


def test_weights():
    x = R.make_set("rand", 2, 4, (1, 5, 5), seed=7)
    y = R.make_set("rand", 2, 1, (1, 5, 5), seed=8)
    e = np.array([np.inf, 3.5, np.nan, -np.inf, np.nan, np.inf, np.inf, np.nan], dtype=np.float32)
    r, uni = E.ensemble(x, images=2, label=y, e=e), E.ensemble(x, images=2, label=y)
    assert np.array_equal(r["mean"][0], x[1].astype(np.float64)) and (r["var"][0] == 0).all()      # one finite E: that particle
    assert r["info"][0, 0] == 1.0
    for key in ("mean", "var", "curve", "final_mse"):                                              # no finite E: uniform
        assert np.array_equal(r[key][1], uni[key][1]), key
    assert r["info"][1, 0] == 4.0
    assert np.array_equal(r["curve"], uni["curve"])                                                # always the uniform prefix
    w, ess, _ = E.weights(np.log(np.array([1.0, 2.0, 4.0, 8.0], dtype=np.float32)))                # w ~ 8, 4, 2, 1 (reversed)
    np.testing.assert_allclose(w[0], np.array([8, 4, 2, 1]) / 15.0, rtol=1e-6)
    assert ess[0] == pytest.approx(15.0 ** 2 / 85.0, rel=1e-6)
    flat = E.ensemble(x, images=2, e=np.full(8, 2.5, dtype=np.float32))                            # equal E: the uniform numbers
    np.testing.assert_allclose(flat["mean"], uni["mean"], rtol=0, atol=1e-15)
    np.testing.assert_allclose(flat["var"], uni["var"], rtol=1e-12, atol=1e-16)
    assert (flat["info"][:, 0] == 4.0).all()


def test_the_last_curve_entry_is_the_mse_of_the_mean():
    x = R.make_set("img", 3, 5, (3, 4, 4), seed=9)
    y = R.make_set("rand", 3, 1, (3, 4, 4), seed=10)
    r = E.ensemble(x, images=3, label=y)
    mse = ((r["mean"] - y.astype(np.float64)) ** 2).reshape(3, -1).mean(axis=1)
    np.testing.assert_allclose(r["curve"][:, -1], mse, rtol=1e-12, atol=0)
    np.testing.assert_allclose(r["final_mse"], mse, rtol=1e-15, atol=0)
    np.testing.assert_allclose(r["info"][:, 2], mse, rtol=1e-15, atol=0)
    first = ((x.reshape(3, 5, -1)[:, 0].astype(np.float64) - y.reshape(3, -1)) ** 2).mean(axis=1)
    np.testing.assert_allclose(r["curve"][:, 0], first, rtol=1e-14, atol=0)


def test_non_finite_values_stay_where_the_definition_puts_them():
    x = R.make_set("rand", 3, 4, (1, 4, 4), seed=11)
    y = R.make_set("rand", 3, 1, (1, 4, 4), seed=12)
    clean = E.ensemble(x, images=3, label=y)
    for bad in (np.nan, np.inf, -np.inf):
        z = x.copy()
        z[6, 0, 1, 2] = bad                                    # image 1, particle 2, element 6
        r = E.ensemble(z, images=3, label=y)
        keep = np.ones(16, dtype=bool)
        keep[6] = False
        for key in ("mean", "var"):
            got, ref = r[key].reshape(3, 16), clean[key].reshape(3, 16)
            assert np.array_equal(got[[0, 2]], ref[[0, 2]]) and np.array_equal(got[1][keep], ref[1][keep])
            assert not np.isfinite(got[1, 6])
        assert np.array_equal(r["curve"][[0, 2]], clean["curve"][[0, 2]]) and np.array_equal(r["curve"][1, :2], clean["curve"][1, :2])
        assert not np.isfinite(r["curve"][1, 2:]).any()
        if np.isnan(bad):
            assert np.isnan(r["curve"][1, 2:]).all()


def test_mean_of_n_psnr_of_a_hand_made_example():
    """three paths of two pixels against the label (0, 1): L = 1.  Prefix means (1, 1), (0.5, 1), (0, 1):
    mse 0.5, 0.125, 0 -> PSNR 10 log10(2), 10 log10(8), +inf"""
    from dps_ttc_amd import metrics
    label = np.array([0.0, 1.0], dtype=np.float32).reshape(1, 1, 1, 2)
    x = np.array([[1.0, 1.0], [0.0, 1.0], [-1.0, 1.0]], dtype=np.float32).reshape(3, 1, 1, 2)
    r = E.ensemble(x, label=label)
    np.testing.assert_allclose(r["curve"][0], [0.5, 0.125, 0.0], rtol=0, atol=1e-16)
    want = np.array([10 * np.log10(2.0), 10 * np.log10(8.0), np.inf])
    np.testing.assert_allclose(E.mean_of_n_psnr(r["curve"], [1.0])[0], want, rtol=1e-15)
    got = metrics.mean_of_n_psnr(torch.from_numpy(r["curve"].astype(np.float32)), torch.from_numpy(label))
    assert got.shape == (1, 3) and got.dtype == torch.float32
    np.testing.assert_allclose(got.numpy()[0], want, rtol=1e-6)


# ------------------------------------------------------------------ the ABI
def test_header_exports_and_signatures():
    from dps_ttc_amd import _lib
    text = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    assert re.search(r"/\* ---- ensemble statistics", text)
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    assert _lib.SIGNATURES["dpsx_ensemble_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["dpsx_ensemble_f32"][1]) == 14 and len(_lib.SIGNATURES["dpsx_ensemble_ex_f32"][1]) == 16
    assert "ensemble.hip" in open(os.path.join(ROOT, "dps_ttc_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_on_the_host():
    """every DPSX_EINVAL / DPSX_EUNSUPPORTED / DPSX_EWORKSPACE, with pointers that must never be dereferenced: there is no
    GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, q = _lib.lib(), c_void_p(0x100000)
    big = 1 << 40

    def ens(x=q, y=q, e=None, count0=0, mean=q, var=q, curve=q, info=q, n=8, d=64, images=2, ws=q, wsb=big):
        return lib.dpsx_ensemble_f32(x, y, e, count0, mean, var, curve, info, n, d, images, ws, wsb, None)

    for kw in (dict(x=None), dict(mean=None), dict(var=None), dict(info=None), dict(ws=None), dict(n=9), dict(n=7), dict(n=0),
               dict(n=-2), dict(d=0), dict(images=0), dict(e=q, count0=8), dict(count0=-1), dict(y=None, curve=q)):
        assert ens(**kw) == _lib.EINVAL, kw
    ex = lambda lo_m, lo_v, **kw: lib.dpsx_ensemble_ex_f32(q, q, None, kw.get("count0", 0), q, q, lo_m, lo_v, q, q,
                                                             kw.get("n", 8), 64, 2, q, kw.get("wsb", big), None)
    assert ex(q, None) == _lib.EINVAL and ex(None, q) == _lib.EINVAL and ex(q, q, n=9) == _lib.EINVAL
    assert ex(q, q, count0=-1) == _lib.EINVAL and ex(q, q, wsb=16) == _lib.EWORKSPACE and ex(None, None, wsb=16) == _lib.EWORKSPACE
    assert ex(q, q, n=2 * 4097) == _lib.EUNSUPPORTED
    assert ens(n=4097, images=1) == _lib.EUNSUPPORTED and ens(n=3 * 4097, images=3) == _lib.EUNSUPPORTED
    assert ens(d=1 << 31) == _lib.EUNSUPPORTED
    assert ens(wsb=16) == _lib.EWORKSPACE and ens(e=q, wsb=16) == _lib.EWORKSPACE and ens(count0=8, wsb=16) == _lib.EWORKSPACE
    wsb = lib.dpsx_ensemble_workspace_bytes
    assert wsb(4097, 64, 1) == _lib.EUNSUPPORTED and wsb(9, 64, 2) == _lib.EINVAL and wsb(8, 0, 2) == _lib.EINVAL
    assert wsb(4096, 16, 1) > 0 and wsb(8, 64, 2) > 0
    assert ens(wsb=wsb(8, 64, 2) - 1) == _lib.EWORKSPACE
    assert wsb(16, 3 * 256 * 256, 1) < wsb(64, 3 * 256 * 256, 4) <= 4 * wsb(16, 3 * 256 * 256, 1)


def test_front_ends_refuse_cpu_tensors_and_bad_options():
    from dps_ttc_amd import kernels, metrics
    x = torch.zeros(4, 3, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        kernels.ensemble_stats(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        metrics.posterior_summary(torch.zeros(1, 3, 16, 16), x)
    with pytest.raises(ValueError, match="reference images"):
        metrics.posterior_summary(torch.zeros(1, 3, 16, 16), x, n_images=2)
    assert kernels.ENSEMBLE_MAX_K == 4096 and kernels.ENSEMBLE_INFO == ("ess", "mean_var", "mse", "count")


# ------------------------------------------------------------------ the driver
def _driver():
    import sys
    sys.path.insert(0, ROOT)
    return importlib.import_module("sample_condition_batched_ttc")


def test_driver_flags():
    drv = _driver()
    a = drv.parse_args([])
    assert (a.posterior_summary, a.posterior_weights) == (False, "uniform")
    assert drv.check_posterior_summary(a, "ddpm") is None
    for name in ("ddpm", "ddim", "ttc_ddim", "search_ddpm", "smc_ddpm"):
        assert drv.check_posterior_summary(drv.parse_args(["--posterior_summary", "--n_paths", "8", "--batch_size", "4"]), name) is None
    ok = drv.parse_args(["--posterior_summary", "--posterior_weights", "smc", "--n_paths", "4096", "--batch_size", "4096"])
    assert drv.check_posterior_summary(ok, "smc_ddpm") is None
    with pytest.raises(SystemExit):
        drv.parse_args(["--posterior_weights", "ess"])

    def refused(argv, match, sampler="ddpm", world=1):
        with pytest.raises(SystemExit) as e:
            drv.check_posterior_summary(drv.parse_args(argv), sampler, world)
        assert re.search(match, str(e.value)) and "\n" not in str(e.value), e.value

    refused(["--posterior_summary"], "one rank only", world=2)
    refused(["--posterior_summary", "--posterior_weights", "smc"], "smc_ddpm", sampler="ddpm")
    refused(["--posterior_summary", "--posterior_weights", "smc", "--n_paths", "8", "--batch_size", "4"], "one particle group",
            sampler="smc_ddpm")
    refused(["--posterior_summary", "--n_paths", "4097", "--batch_size", "4097"], "4096")
    refused(["--posterior_weights", "smc"], "needs --posterior_summary", sampler="smc_ddpm")


def test_driver_refuses_before_any_gpu_work(monkeypatch, tmp_path):
    """main() itself: the refusal comes before the device is asked for anything (there is none here) and writes nothing"""
    drv = _driver()
    diff = os.path.join(ROOT, "configs", "diffusion_config.yaml")
    for argv, match in ((["--posterior_summary", "--posterior_weights", "smc"], "smc_ddpm"),
                        (["--posterior_summary", "--n_paths", "5000", "--batch_size", "5000"], "4096")):
        with pytest.raises(SystemExit, match=match):
            drv.main(["--diffusion_config", diff, "--save_dir", str(tmp_path / "out")] + argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank only"):
        drv.main(["--diffusion_config", diff, "--save_dir", str(tmp_path / "out"), "--posterior_summary"])
    assert not (tmp_path / "out").exists()
