"""CPU suite of particle repulsion (include/dpsx.h "particle repulsion"): the float64 restatement tests/repulse_ref.py
against the definition's own properties, the input set that tells the difference form from the Gram form, the names in
the header / the exports / the ctypes table, every refusal of the entry points without a GPU, what the samplers refuse
before the device is asked for anything, and the driver's flag checks."""
import ctypes
import importlib
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch

import repulse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"          # operators build their device handle lazily: constructing them needs no GPU
NAMES = ("dpsx_repulse_workspace_bytes", "dpsx_pairwise_sqdist_f32", "dpsx_repulse_f32")


# ------------------------------------------------------------------ the restatement
def test_two_particles_closed_form():
    x = R.make_set("rand", 1, 2, (3, 8, 8), seed=1)
    for bw in (None, 0.7):
        r = R.repulse(x, 0.3, bandwidth=bw)
        h, gain, mean, mn = r["info"][0]
        d2 = float(((x[0].astype(np.float64) - x[1]) ** 2).sum())
        assert mean == mn == r["d2"][0, 0, 1] == d2
        assert h == pytest.approx(float(np.float32(bw)) * x[0].size if bw else d2 / np.log(3.0), rel=1e-15)
        assert gain == pytest.approx(2 * float(np.float32(0.3)) / h, rel=1e-15)
        w01 = np.exp(-d2 / h)
        assert r["w"][0, 0, 1] == pytest.approx(w01, rel=1e-15) and r["w"][0, 0, 0] == 0.0
        if bw is None:
            assert w01 == pytest.approx(1.0 / 3.0, rel=1e-12)            # at the typical distance a weight is 1 / (K + 1)
        diff = x[0].astype(np.float64) - x[1]
        np.testing.assert_allclose(r["out"][0] - r["out"][1], diff * (1.0 + 2.0 * gain * w01), rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["rand", "img", "neardup", "far"])
def test_symmetry_and_the_mean_is_kept(name):
    x = R.make_set(name, 2, 5, (1, 7, 9), seed=2)
    r = R.repulse(x, 0.2, images=2)
    assert np.array_equal(r["d2"], r["d2"].transpose(0, 2, 1)) and np.array_equal(r["w"], r["w"].transpose(0, 2, 1))
    assert (np.einsum("mii->mi", r["d2"]) == 0).all() and (np.einsum("mii->mi", r["w"]) == 0).all() and r["applied"].all()
    delta = r["delta"].reshape(2, 5, -1)
    each = np.linalg.norm(delta, axis=2).sum(axis=1)
    assert (each > 0).all() and (np.linalg.norm(delta.sum(axis=1), axis=1) <= 1e-12 * each).all()
    # the push is repulsive: every pairwise distance grows
    grown = R.sqdist(r["out"], 2)
    iu = np.triu_indices(5, 1)
    assert (grown[:, iu[0], iu[1]] > r["d2"][:, iu[0], iu[1]]).all()
    # an image's numbers are its own
    one = R.repulse(x[5:], 0.2)
    assert np.array_equal(one["out"], r["out"][5:]) and np.array_equal(one["info"][0], r["info"][1])


def test_copy_rules():
    shape = (1, 4, 4)
    one = R.repulse(R.make_set("rand", 1, 1, shape), 0.5)                      # K = 1
    assert not one["applied"][0] and (one["delta"] == 0).all() and one["info"][0, 3] == np.inf and one["info"][0, 1] == 0
    eq = np.repeat(R.make_set("rand", 1, 1, shape, seed=3), 4, axis=0)         # all particles equal: h = 0
    r = R.repulse(eq, 0.5)
    assert not r["applied"][0] and (r["delta"] == 0).all() and r["info"][0, 0] == 0 and (r["w"] == 0).all()
    r = R.repulse(eq, 0.5, bandwidth=1.0)                                      # ... a fixed bandwidth steps it by nothing
    assert r["applied"][0] and (r["delta"] == 0).all() and (r["w"][0][~np.eye(4, dtype=bool)] == 1).all()
    for bad in (np.nan, np.inf):                                               # a non-finite value: its own image only
        for bw in (None, 1.0):
            x = R.make_set("rand", 3, 4, shape, seed=4)
            x[5, 0, 1, 2] = bad
            r = R.repulse(x, 0.5, images=3, bandwidth=bw)
            assert list(r["applied"]) == [True, False, True] and (r["delta"][4:8] == 0).all()
            assert np.isfinite(r["out"][:4]).all() and np.isfinite(r["out"][8:]).all() and (r["w"][1] == 0).all()
    d = R.repulse(R.make_set("dup", 1, 4, shape, seed=5), 0.5)                 # duplicates: min = 0, still stepped
    assert d["d2"][0, 0, 3] == 0 and d["info"][0, 3] == 0 and d["applied"][0] and np.array_equal(d["out"][0], d["out"][3])
    far = R.repulse(R.make_set("far", 1, 4, shape, seed=6), 0.5, bandwidth=0.5)         # all its weights underflow
    assert (far["w"][0, 3] == 0).all() and (far["delta"][3] == 0).all() and far["applied"][0]


def test_neardup_tells_the_difference_form_from_the_gram_form():
    """the set that makes the GPU bound |d2 - ref| <= 1e-5 ref a test of the form: float32 numpy in the difference form
    stays inside it (observed 6.0e-7 with einsum's plain float32 accumulation over 3072 elements), in the Gram form it does
    not (observed 0.67)"""
    x = R.make_set("neardup", 1, 16, (3, 32, 32), seed=7)
    ref = R.sqdist(x)
    off = ~np.eye(16, dtype=bool)
    err = lambda d2: float((np.abs(d2[0].astype(np.float64) - ref[0])[off] / ref[0][off]).max())
    diff, gram = err(R.sqdist_f32_difference(x)), err(R.sqdist_f32_gram(x))
    print(f"neardup: difference form {diff:.3g}, Gram form {gram:.3g} (max relative error of d2)")
    assert diff <= 1e-5 < gram
    assert (np.einsum("ii->i", R.sqdist_f32_difference(x)[0]) == 0).all()


# ------------------------------------------------------------------ the ABI
def test_header_exports_and_signatures():
    from dps_ttc_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpsx.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and hasattr(raw, name) and name in _lib.SIGNATURES, name
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    assert _lib.SIGNATURES["dpsx_repulse_f32"][1][:2] == [ctypes.c_float, ctypes.c_float]
    assert _lib.SIGNATURES["dpsx_repulse_workspace_bytes"][0] is ctypes.c_int64


def test_entry_points_refuse_on_the_host():
    """every DPSX_EINVAL / DPSX_EUNSUPPORTED / DPSX_EWORKSPACE, with pointers that must never be dereferenced: there is no
    GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, q, o = _lib.lib(), c_void_p(0x100000), c_void_p(0x900000)
    big = 1 << 40

    def rep(c=0.1, bw=0.0, x=q, out=o, n=8, chw=64, seg=2, ws=q, wsb=big):
        return lib.dpsx_repulse_f32(c, bw, x, out, None, None, None, None, n, chw, seg, ws, wsb, None)

    def dist(x=q, d2=o, n=8, chw=64, seg=2, ws=q, wsb=big):
        return lib.dpsx_pairwise_sqdist_f32(x, d2, None, n, chw, seg, ws, wsb, None)

    for kw in (dict(x=None), dict(out=None), dict(ws=None), dict(n=-1), dict(chw=0), dict(seg=0), dict(n=9, seg=2),
               dict(n=7, seg=2), dict(c=-0.1), dict(c=float("nan")), dict(c=float("inf")), dict(bw=-1.0),
               dict(bw=float("nan")), dict(bw=float("inf")), dict(out=q), dict(out=c_void_p(0x100000 + 4 * 64))):
        assert rep(**kw) == _lib.EINVAL, kw
    for kw in (dict(x=None), dict(d2=None), dict(ws=None), dict(n=9, seg=2), dict(chw=0)):
        assert dist(**kw) == _lib.EINVAL, kw
    for call in (rep, dist):
        assert call(n=513, seg=1) == _lib.EUNSUPPORTED and call(n=3 * 513, seg=3) == _lib.EUNSUPPORTED
        assert call(wsb=16) == _lib.EWORKSPACE
        assert call(n=0) == _lib.OK                                        # nothing to do, nothing launched
    assert lib.dpsx_repulse_workspace_bytes(513, 64, 1) == _lib.EUNSUPPORTED
    assert lib.dpsx_repulse_workspace_bytes(9, 64, 2) == _lib.EINVAL
    assert lib.dpsx_repulse_workspace_bytes(512, 64, 1) > 0 and lib.dpsx_repulse_workspace_bytes(8, 64, 2) > 0
    # the size depends on the images only through their count
    assert lib.dpsx_repulse_workspace_bytes(16, 3 * 256 * 256, 1) < lib.dpsx_repulse_workspace_bytes(64, 3 * 256 * 256, 4)


def test_front_ends_refuse_cpu_tensors_and_bad_options():
    from dps_ttc_amd import kernels
    x = torch.zeros(4, 3, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        kernels.pairwise_sqdist(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        kernels.repulse(x, 0.1)
    for bad in (-1.0, float("nan"), float("inf"), None, "a", True):
        with pytest.raises(ValueError, match="strength"):
            kernels.repulse(x, bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bandwidth"):
            kernels.repulse(x, 0.1, bandwidth=bad)


# ------------------------------------------------------------------ the samplers
def _sampler(name="ddpm", respacing="20", eta=None):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    kw = {} if eta is None else {"eta": eta}
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing, **kw)


def test_samplers_refuse_before_the_device_is_asked():
    """CPU tensors and a model that raises when called: every refusal comes first, with its reason in the message"""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator

    def model(*a, **kw):
        raise AssertionError("the model was called")

    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.3)
    x, y = torch.zeros(4, 3, 64, 64), torch.zeros(1, 3, 64, 64)

    def loop(smp, x=x, y=y, **kw):
        return smp.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=cm.conditioning, record=False,
                                 save_root=None, **kw)

    def on(name="ddpm", **attrs):
        smp = _sampler(name)
        assert smp.repulsion_scale == 0.0 and smp.repulsion_bandwidth is None and smp.repulsion_stop == 0.0
        smp.repulsion_scale = 0.5
        for k, v in attrs.items():
            setattr(smp, k, v)
        return smp

    with pytest.raises(NotImplementedError, match="particle_groups = 2"):
        loop(on(particle_groups=2))
    with pytest.raises(NotImplementedError, match="smc_ddpm"):
        loop(on("smc_ddpm"))
    with pytest.raises(NotImplementedError, match="search_ddpm"):
        loop(on("search_ddpm"), operator=op)
    with pytest.raises(NotImplementedError, match="search_ddpm"):
        loop(on("search_ddpm", beam_width=2), operator=op)
    with pytest.raises(NotImplementedError, match="several ranks"):
        loop(on("ttc_ddim", global_resample=True))
    with pytest.raises(NotImplementedError, match="rng_parity"):
        loop(on(rng_parity=True))
    for name in ("ddpm", "ddim", "ttc_ddim"):
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="repulsion_scale"):
                loop(on(name, repulsion_scale=bad))
            with pytest.raises(ValueError, match="repulsion_bandwidth"):
                loop(on(name, repulsion_bandwidth=bad))
        for bad in (-0.1, 1.1, float("nan"), None):
            with pytest.raises(ValueError, match="repulsion_stop"):
                loop(on(name, repulsion_stop=bad))
    with pytest.raises(NotImplementedError, match="513 particles per image"):
        loop(on(), x=torch.zeros(513, 1, 16, 16), y=torch.zeros(1, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="513 particles per image"):
        loop(on("ddim"), x=torch.zeros(1026, 1, 16, 16), y=torch.zeros(2, 1, 16, 16))
    # accepted: the loop then asks for the device; the option off refuses nothing
    for smp in (on(), on("ddim"), on("ttc_ddim"), on(repulsion_bandwidth=0.5, repulsion_stop=0.3), _sampler("smc_ddpm")):
        with pytest.raises(RuntimeError, match="MI355X"):
            loop(smp)
    with pytest.raises(RuntimeError, match="MI355X"):
        loop(on(), x=torch.zeros(1024, 1, 16, 16), y=torch.zeros(2, 1, 16, 16))      # 2 images x 512


def test_the_step_runs_on_the_right_steps():
    """_repulse is the identity at idx = 0, below repulsion_stop and with the option off (no device needed for that)"""
    smp = _sampler(respacing="10")
    x = torch.zeros(2, 1, 4, 4)
    assert all(smp._repulse(x, idx, 1) is x for idx in range(10)) and smp._repulse_out is None
    smp.repulsion_scale, smp.repulsion_stop = 0.5, 0.35
    for idx in range(10):
        if idx == 0 or idx / 10 < 0.35:
            assert smp._repulse(x, idx, 1) is x
        else:
            with pytest.raises(RuntimeError, match="MI355X"):
                smp._repulse(x, idx, 1)
    assert smp._repulse_out is None                    # nothing was allocated on the way to the refusal
    smp.repulsion_stop = 0.0
    assert smp._repulse(x, 0, 1) is x                  # never on the last step


# ------------------------------------------------------------------ the driver
def test_driver_flags():
    import sys
    sys.path.insert(0, ROOT)
    drv = importlib.import_module("sample_condition_batched_ttc")
    a = drv.parse_args([])
    assert (a.repulsion_scale, a.repulsion_bandwidth, a.repulsion_stop, a.path_diversity) == (0.0, None, 0.0, False)
    assert drv.repulsion_flags(a) == [] and drv.check_repulsion(a, "ddpm") is None
    ok = drv.parse_args(["--repulsion_scale", "0.5", "--repulsion_bandwidth", "0.1", "--repulsion_stop", "0.2"])
    for name in ("ddpm", "ddim", "ttc_ddim"):
        assert drv.check_repulsion(ok, name) is None
    assert drv.check_repulsion(drv.parse_args(["--path_diversity", "--batch_size", "512"]), "search_ddpm") is None

    def refused(argv, match, sampler="ddpm", world=1):
        with pytest.raises(SystemExit) as e:
            drv.check_repulsion(drv.parse_args(argv), sampler, world)
        assert re.search(match, str(e.value)) and "\n" not in str(e.value), e.value

    refused(["--repulsion_scale", "-1"], "not negative")
    refused(["--repulsion_scale", "nan"], "finite")
    refused(["--repulsion_scale", "1", "--repulsion_bandwidth", "inf"], "finite")
    refused(["--repulsion_scale", "1", "--repulsion_stop", "1.5"], r"\[0, 1\]")
    refused(["--repulsion_bandwidth", "0.1"], "needs --repulsion_scale")
    refused(["--repulsion_stop", "0.1"], "needs --repulsion_scale")
    refused(["--repulsion_scale", "1"], "search_ddpm", sampler="search_ddpm")
    refused(["--repulsion_scale", "1"], "smc_ddpm", sampler="smc_ddpm")
    refused(["--repulsion_scale", "1", "--particle_groups", "2"], "particle_groups")
    refused(["--repulsion_scale", "1"], "one rank", sampler="ttc_ddim", world=2)
    refused(["--repulsion_scale", "1", "--batch_size", "513"], "512")
    refused(["--path_diversity", "--batch_size", "513"], "512")


def test_driver_path_diversity_is_single_rank(monkeypatch):
    import sys
    sys.path.insert(0, ROOT)
    drv = importlib.import_module("sample_condition_batched_ttc")
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank only"):
        drv.parse_args(["--path_diversity"])
    assert drv.parse_args([]).path_diversity is False
