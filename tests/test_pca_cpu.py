"""CPU suite of the principal components (include/dpsx.h "principal components"): the float64 restatement
tests/pca_ref.py against a direct covariance eigendecomposition, the conditions the GPU suite relies on (the eigen-gaps of
the set `planted` on its shapes, the closed form of `dup`), every refusal of the entry points through ctypes without a GPU,
the driver's flag checks and metrics.pc_panels."""
import ctypes
import importlib
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import pca_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dpsx_pca_workspace_bytes", "dpsx_pca_f32")
# the shapes of tests/test_pca_gpu.py: M, K, (C, H, W)
GPU_SHAPES = [(1, 1, (1, 8, 8)), (1, 2, (1, 1, 7)), (2, 3, (1, 33, 47)), (1, 9, (1, 1, 7)), (3, 16, (3, 32, 32)),
              (1, 64, (3, 16, 16)), (1, 127, (3, 16, 16)), (1, 128, (3, 16, 16)), (1, 8, (3, 256, 256))]
MIN_GAP = 0.005


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ("planted", "iid"))
@pytest.mark.parametrize("k,shape", [(2, (1, 1, 7)), (5, (1, 3, 4)), (9, (1, 1, 7)), (12, (1, 2, 5))])
def test_restatement_against_the_covariance(name, k, shape):
    """the K x K route gives the eigenpairs of the D x D sample covariance: same eigenvalues (times K), same directions up
    to sign, scores = the projections of the centred particles"""
    x = P.make_set(name, 2, k, shape, seed=3).astype(np.float64).reshape(2, k, -1)
    q = 4
    ref = P.pca(x.reshape(2 * k, *shape), images=2, components=q)
    for b in range(2):
        xc = x[b] - x[b].mean(axis=0)
        lam, u = np.linalg.eigh(xc.T @ xc / k)
        lam, u = lam[::-1], u[:, ::-1]
        rank = int(ref["info"][b, 1])
        assert rank == int((lam > P.null_threshold(k, lam[0])).sum()) <= min(k - 1, xc.shape[1])     # the null rule
        assert ref["info"][b, 3] == k
        assert np.allclose(ref["info"][b, 0], (xc ** 2).sum(), rtol=1e-12)
        for j in range(min(q, rank)):
            assert np.isclose(ref["var"][b, j], lam[j], rtol=1e-9) and np.isclose(ref["evals"][b, j], k * lam[j], rtol=1e-9)
            uj = ref["dirs"][b, j]
            assert abs(np.linalg.norm(uj) - 1) < 1e-9 and abs(abs(uj @ u[:, j]) - 1) < 1e-7
            assert np.allclose(xc @ uj, ref["coords"][b, :, j], atol=1e-9 * np.sqrt(ref["evals"][b, 0]))
            c = ref["coords"][b, :, j]
            assert c[np.argmax(np.abs(c))] > 0 and abs(c.sum()) < 1e-9 * np.sqrt(ref["evals"][b, 0])
        assert np.allclose(ref["explained"][b, :rank].sum(), ref["evals"][b, :rank].sum() / ref["info"][b, 0])
        for j in range(rank, q):                 # null components
            assert ref["evals"][b, j] == 0 and not ref["dirs"][b, j].any() and not ref["coords"][b, :, j].any()


def test_restatement_reconstructs_the_particles():
    x = P.make_set("iid", 1, 6, (1, 3, 5), seed=1)
    ref = P.pca(x, components=8)
    flat = x.reshape(6, -1).astype(np.float64)
    assert ref["info"][0, 1] == 5 and (ref["evals"][0, 5:] == 0).all()
    assert np.allclose(ref["coords"][0] @ ref["dirs"][0], flat - flat.mean(axis=0), atol=1e-12)


def test_degenerate_sets_in_the_restatement():
    same = P.pca(P.make_set("same", 2, 5, (1, 4, 4)), images=2)
    for key in ("evals", "coords", "dirs"):
        assert not same[key].any()
    assert (same["info"][:, :2] == 0).all() and (same["info"][:, 3] == 5).all()
    one = P.pca(P.make_set("planted", 2, 1, (1, 4, 4)), images=2)
    assert not one["dirs"].any() and (one["info"][:, 1] == 0).all()
    x = P.make_set("nan", 3, 5, (1, 4, 4))
    assert np.isnan(x).sum() == 1 and np.isnan(x.reshape(3, 5, -1)[1, 2, 5])
    nan, clean = P.pca(x, images=3), P.pca(P.make_set("planted", 3, 5, (1, 4, 4)), images=3)
    assert np.isnan(nan["evals"][1]).all() and np.isnan(nan["dirs"][1]).all() and np.isnan(nan["coords"][1]).all()
    assert nan["info"][1, 1] == -1 and np.isnan(nan["info"][1, 0])
    for key in ("evals", "coords", "dirs"):
        assert np.array_equal(nan[key][[0, 2]], clean[key][[0, 2]])
    for kw in (dict(images=2), dict(components=0), dict(components=9)):
        with pytest.raises(ValueError):
            P.pca(np.zeros((5, 1, 2, 2), dtype=np.float32), **kw)
    with pytest.raises(ValueError):
        P.pca(np.zeros((129, 1, 2, 2), dtype=np.float32))


@pytest.mark.parametrize("m,k,shape", [s for s in GPU_SHAPES if s[1] >= 5], ids=lambda v: str(v).replace(" ", ""))
def test_planted_gaps_on_the_gpu_shapes(m, k, shape):
    """the direction comparison of the GPU suite divides by the relative eigen-gap: on `planted` the first four
    components keep min(l_{j-1} - l_j, l_j - l_{j+1}) / l_0 >= 0.005 on every shape with K >= 5"""
    ref = P.pca(P.make_set("planted", m, k, shape), images=m, components=4)
    print(f"{m}x{k}x{shape}: gaps {np.array2string(ref['gap'], precision=4)}")
    assert (ref["info"][:, 1] >= 4).all() and (ref["gap"] >= MIN_GAP).all()


@pytest.mark.parametrize("k", (2, 3, 9, 16, 127, 128))
def test_dup_closed_form(k):
    """copies of two particles a, b (n_a and n_b of them): one component, l_0 = |a - b|^2 n_a n_b / K"""
    x = P.make_set("dup", 2, k, (1, 5, 7))
    ref = P.pca(x, images=2, components=3)
    na, nb = P.dup_counts(k)
    flat = x.reshape(2, k, -1).astype(np.float64)
    for b in range(2):
        want = ((flat[b, 0] - flat[b, -1]) ** 2).sum() * na * nb / k
        assert ref["info"][b, 1] == 1 and np.isclose(ref["evals"][b, 0], want, rtol=1e-12) and not ref["evals"][b, 1:].any()
        assert np.isclose(ref["info"][b, 0], want, rtol=1e-12)


# ------------------------------------------------------------------ the ABI
def test_header_exports_and_signatures():
    from dps_ttc_amd import _lib
    text = open(os.path.join(ROOT, "include", "dpsx.h")).read()
    assert re.search(r"/\* ---- principal components", text)
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    assert _lib.SIGNATURES["dpsx_pca_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib.SIGNATURES["dpsx_pca_f32"][1]) == 13
    assert "pca.hip" in open(os.path.join(ROOT, "dps_ttc_amd", "csrc", "Makefile")).read()


def test_entry_points_refuse_on_the_host():
    """every DPSX_EINVAL / DPSX_EUNSUPPORTED / DPSX_EWORKSPACE, with pointers that must never be dereferenced: there is no
    GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, p = _lib.lib(), c_void_p(0x100000)
    big = 1 << 40

    def call(x=p, q=4, dirs=p, evals=p, coords=p, info=p, d2=p, n=8, d=64, images=2, ws=p, wsb=big):
        return lib.dpsx_pca_f32(x, q, dirs, evals, coords, info, d2, n, d, images, ws, wsb, None)

    for kw in (dict(x=None), dict(dirs=None), dict(evals=None), dict(coords=None), dict(info=None), dict(ws=None),
               dict(q=0), dict(q=9), dict(q=-1), dict(n=0), dict(n=-2), dict(n=9), dict(n=7), dict(d=0), dict(d=-1),
               dict(images=0), dict(images=-1)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(n=129, images=1) == _lib.EUNSUPPORTED and call(n=3 * 129, images=3) == _lib.EUNSUPPORTED
    assert call(d=1 << 31) == _lib.EUNSUPPORTED and call(n=65536, images=65536) == _lib.EUNSUPPORTED
    assert call(wsb=16) == _lib.EWORKSPACE and call(d2=None, wsb=16) == _lib.EWORKSPACE
    wsb = lib.dpsx_pca_workspace_bytes
    assert wsb(129, 64, 1) == _lib.EUNSUPPORTED and wsb(9, 64, 2) == _lib.EINVAL and wsb(8, 0, 2) == _lib.EINVAL
    assert wsb(8, 64, 0) == _lib.EINVAL and wsb(0, 64, 1) == _lib.EINVAL
    assert wsb(128, 16, 1) > 0 and wsb(8, 64, 2) > 0
    assert wsb(8, 64, 2) >= lib.dpsx_repulse_workspace_bytes(8, 64, 2) + 2 * 4 * 4 * 4        # the distances' own + d2
    assert call(wsb=wsb(8, 64, 2) - 1) == _lib.EWORKSPACE
    assert call(q=9, wsb=16) == _lib.EINVAL and call(n=129, images=1, wsb=16) == _lib.EUNSUPPORTED     # arguments first


def test_front_ends_refuse_cpu_tensors_and_bad_options():
    from dps_ttc_amd import kernels, metrics
    x = torch.zeros(4, 3, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        kernels.particle_pca(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        metrics.posterior_pca(x)
    assert kernels.PCA_MAX_K == 128 and kernels.PCA_MAX_Q == 8 and kernels.PCA_INFO == ("trace", "rank", "sweeps", "count")
    assert kernels.pca_components(1) == 1 and kernels.pca_components(np.int64(8)) == 8
    for bad in (0, 9, -1, 2.0, True, None, "3"):
        with pytest.raises(ValueError):
            kernels.pca_components(bad)


def test_pc_panels():
    from dps_ttc_amd import metrics
    g = torch.Generator().manual_seed(0)
    mean, dirs = torch.randn(2, 3, 4, 5, generator=g), torch.randn(2, 3, 3, 4, 5, generator=g)
    var = torch.tensor([[4.0, 1.0, 0.0], [0.25, 9.0, 1.0]])
    minus, plus = metrics.pc_panels(mean, dirs, var)
    assert minus.shape == plus.shape == dirs.shape
    for b in range(2):
        for j in range(3):
            step = 2.0 * float(var[b, j]) ** 0.5 * dirs[b, j]
            assert torch.allclose(plus[b, j], mean[b] + step, atol=1e-6) and torch.allclose(minus[b, j], mean[b] - step, atol=1e-6)
    assert torch.equal(plus[0, 2], mean[0]) and torch.equal(minus[0, 2], mean[0])    # zero variance: the mean itself
    m3, p3 = metrics.pc_panels(mean, dirs, var, n_sigma=3.0)
    assert torch.allclose(p3 - mean.unsqueeze(1), 1.5 * (plus - mean.unsqueeze(1)), atol=1e-5)
    assert torch.allclose(m3 + p3, 2 * mean.unsqueeze(1).expand_as(p3), atol=1e-5)
    for bad in ((mean[:1], dirs, var), (mean, dirs[:, :2], var), (mean, dirs[0], var)):
        with pytest.raises(ValueError):
            metrics.pc_panels(*bad)


# ------------------------------------------------------------------ the driver
def _driver():
    import sys
    sys.path.insert(0, ROOT)
    return importlib.import_module("sample_condition_batched_ttc")


def test_driver_flag():
    drv = _driver()
    a = drv.parse_args([])
    assert a.posterior_pca is None and drv.check_posterior_pca(a, "ddpm") is None
    assert drv.check_posterior_pca(a, "search_ddpm", world=4) is None          # off: nothing is checked
    for name in ("ddpm", "ddim", "ttc_ddim", "smc_ddpm", None):
        for q in ("1", "8"):
            ok = drv.parse_args(["--posterior_pca", q, "--n_paths", "128", "--batch_size", "128"])
            assert drv.check_posterior_pca(ok, name) is None
    both = drv.parse_args(["--posterior_pca", "3", "--posterior_summary", "--posterior_quantiles", "50", "--n_paths", "8",
                           "--batch_size", "8"])
    assert drv.check_posterior_pca(both, "ddpm") is None and drv.check_posterior_quantiles(both, "ddpm") is None

    def refused(argv, match, sampler="ddpm", world=1):
        with pytest.raises(SystemExit) as e:
            drv.check_posterior_pca(drv.parse_args(argv), sampler, world)
        assert re.search(match, str(e.value)) and "\n" not in str(e.value), e.value

    one = ["--n_paths", "8", "--batch_size", "8"]
    refused(["--posterior_pca", "3"] + one, "one rank only", world=2)
    refused(["--posterior_pca", "3", "--n_paths", "8", "--batch_size", "4"], "one particle group")
    refused(["--posterior_pca", "3", "--n_paths", "129", "--batch_size", "129"], "128")
    refused(["--posterior_pca", "0"] + one, "between 1 and 8")
    refused(["--posterior_pca", "9"] + one, "between 1 and 8")
    refused(["--posterior_pca", "-2"] + one, "between 1 and 8")
    refused(["--posterior_pca", "3"] + one, "search_ddpm", sampler="search_ddpm")


def test_driver_refuses_before_any_gpu_work(monkeypatch, tmp_path):
    """main() itself: the refusal comes before the device is asked for anything (there is none here) and writes nothing"""
    drv = _driver()
    diff = os.path.join(ROOT, "configs", "diffusion_config.yaml")
    for argv, match in ((["--posterior_pca", "3", "--n_paths", "8", "--batch_size", "4"], "one particle group"),
                        (["--posterior_pca", "12", "--n_paths", "4", "--batch_size", "4"], "between 1 and 8"),
                        (["--posterior_pca", "2", "--n_paths", "256", "--batch_size", "256"], "128")):
        with pytest.raises(SystemExit, match=match):
            drv.main(["--diffusion_config", diff, "--save_dir", str(tmp_path / "out")] + argv)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank only"):
        drv.main(["--diffusion_config", diff, "--save_dir", str(tmp_path / "out"), "--posterior_pca", "2",
                  "--n_paths", "4", "--batch_size", "4"])
    assert not (tmp_path / "out").exists()
