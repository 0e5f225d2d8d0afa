"""CPU suite of the particle weights and the smc_ddpm sampler: the three names in the header / the exports / the ctypes
table, every refusal of the two entry points without a GPU, the sampler registry, the restatement tests/smc_ref.py (the
reference of the GPU suite) against the direct density difference and the proposal ratio's integral, what the sampler and
the driver refuse before any launch."""
import ctypes
import importlib
import os
import re
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch

import smc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"          # operators build their device handle lazily: constructing them needs no GPU
NAMES = ("dpsx_corr_slots", "dpsx_step_update_corr_f32", "dpsx_smc_accum_f32")


def test_header_exports_and_signatures_hold_the_three_names():
    from dps_ttc_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpsx.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    i, i64, p, f = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_float
    assert _lib.SIGNATURES["dpsx_corr_slots"] == (i, [i64])
    base = list(_lib.SIGNATURES["dpsx_step_update_f32"][1])            # sample, g_model_out, g_unet | x_next, n, chw, coefs, stream
    assert _lib.SIGNATURES["dpsx_step_update_corr_f32"] == (
        i, base[:3] + [p, p, ctypes.POINTER(_lib.RngRec)] + base[3:4] + [p] + base[4:])
    assert _lib.SIGNATURES["dpsx_smc_accum_f32"] == (i, [p, p, p, p, i, p, i64, i64, f, i, f, p])


def test_corr_slots_is_a_function_of_the_particle_size():
    from dps_ttc_amd import _lib, kernels
    lib = _lib.lib()
    assert lib.dpsx_corr_slots(-1) == _lib.EINVAL
    for chw, want in ((0, 1), (1, 1), (1024, 1), (1025, 2), (1 * 33 * 47, 2), (3 * 64 * 64, 12), (3 * 256 * 256, 192),
                      (1 * 520 * 520, 256), (1 << 40, 256)):
        assert lib.dpsx_corr_slots(chw) == want == kernels.corr_slots(chw), chw


def _coefs(mode=1, b=2.0, sigma=-9.0):
    from dps_ttc_amd import kernels
    c = kernels.make_coefs(1.5, b, 0.5, 0.5, sigma, -4.0, True)
    c.add_noise = mode
    return c


def test_update_corr_refuses_on_the_host():
    """every DPSX_EINVAL of dpsx_step_update_corr_f32, with pointers that must never be dereferenced: no GPU here"""
    from dps_ttc_amd import _lib
    lib, q = _lib.lib(), c_void_p(0x1000)
    rng, ok = _lib.RngRec(1, 2, 0, 0, 0), _coefs()

    def call(sample=q, g=q, gu=q, mo=q, noise=q, r=None, out=q, part=q, n=2, chw=8, c=ok):
        return lib.dpsx_step_update_corr_f32(sample, g, gu, mo, noise, None if r is None else byref(r), out, part, n, chw,
                                             None if c is None else byref(c), None)

    assert call(noise=q, r=rng) == _lib.EINVAL                        # both noise sources
    assert call(noise=None, r=None) == _lib.EINVAL                    # neither
    assert call(c=_coefs(mode=0), noise=None, r=None) == _lib.EINVAL  # ... whatever the step
    for kw in (dict(sample=None), dict(g=None), dict(out=None), dict(part=None), dict(c=None), dict(n=-1), dict(chw=-1),
               dict(mo=None)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(c=_coefs(b=0.0)) == _lib.EINVAL
    for sigma in (0.0, -0.1, float("nan")):                           # a DDIM record that adds noise with no variance
        assert call(c=_coefs(mode=3, sigma=sigma)) == _lib.EINVAL, sigma
    assert call(noise=None, r=_lib.RngRec(1, 2, 0, -1, 0)) == _lib.EINVAL          # a bad rng record
    assert call(noise=None, r=_lib.RngRec(1, 2, 0, 0xffffffff, 0)) == _lib.EINVAL  # particle ids past 32 bits
    assert call(n=65536) == _lib.EUNSUPPORTED
    assert call(n=0) == _lib.OK and call(chw=0) == _lib.OK            # nothing to do, nothing launched


def test_smc_accum_refuses_on_the_host():
    from dps_ttc_amd import _lib
    lib, q = _lib.lib(), c_void_p(0x1000)

    def call(E=q, dp=q, dc=q, part=q, slots=12, reset=None, segments=1, n=4, ts=0.01, power=1, pw=1.0):
        return lib.dpsx_smc_accum_f32(E, dp, dc, part, slots, reset, segments, n, ts, power, pw, None)

    for kw in (dict(E=None), dict(dp=None), dict(dc=None), dict(n=-1), dict(power=0), dict(power=3), dict(segments=0),
               dict(segments=3), dict(slots=0), dict(ts=float("nan")), dict(ts=float("inf")), dict(pw=float("nan"))):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(n=65536) == _lib.EUNSUPPORTED
    assert call(n=0) == _lib.OK


def _sampler(name="smc_ddpm", respacing="20"):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing)


def test_sampler_registry():
    from dps_ttc_amd import gaussian_diffusion as GD
    assert sorted(GD.__SAMPLER__) == ["ddim", "ddpm", "search_ddpm", "ttc_ddim"]       # the reference's four
    assert sorted(GD.__EXTENSION_SAMPLER__) == ["smc_ddpm"]
    cls = GD.get_sampler("smc_ddpm")
    assert issubclass(cls, GD.DDPM) and GD.get_sampler("ddpm") is GD.DDPM
    with pytest.raises(NameError, match="already registered"):
        GD.register_sampler(name="smc_ddpm", extension=True)(object)
    with pytest.raises(NameError, match="already registered"):
        GD.register_sampler(name="ddpm", extension=True)(object)
    with pytest.raises(NameError, match="not defined"):
        GD.get_sampler("no_such_sampler")
    smp = _sampler()
    assert isinstance(smp, cls) and smp.num_timesteps == 20 and smp.hip_posterior
    assert (smp.twist_scale, smp.twist_power, smp.proposal_weight, smp.resample_every) == (0.01, 1, 1.0, 10)
    assert (smp.resample_scheme, smp.resample_ess) == ("multinomial", None)
    assert smp.last_neg_log_weights is None and smp.last_resample_ids is None and smp.last_resample_flags is None


def test_sampler_refuses_before_any_launch():
    """CPU tensors: anything that reached a launch would raise RuntimeError (no CPU fallback), not these"""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    noiser = get_noise("gaussian", sigma=0.05)
    ps = get_conditioning_method("ps", op, noiser, scale=0.5)
    x, y = torch.zeros(4, 3, 64, 64), torch.zeros(1, 3, 64, 64)

    def loop(smp, cm=ps, **kw):
        return smp.p_sample_loop(model=None, x_start=x, measurement=y, measurement_cond_fn=cm.conditioning, record=False,
                                 save_root=None, **kw)

    for attr, value, exc, word in (("particle_groups", 2, ValueError, "particle_groups"),
                                   ("rng_parity", True, ValueError, "rng_parity"),
                                   ("global_resample", True, NotImplementedError, "global"),
                                   ("twist_power", 3, ValueError, "twist_power"),
                                   ("twist_scale", float("nan"), ValueError, "twist_scale"),
                                   ("proposal_weight", float("inf"), ValueError, "proposal_weight"),
                                   ("resample_every", 0, ValueError, "resample_every"),
                                   ("resample_scheme", "residual", ValueError, "scheme"),
                                   ("resample_ess", 1.5, ValueError, "ESS")):
        smp = _sampler()
        setattr(smp, attr, value)
        with pytest.raises(exc, match=word):
            loop(smp)
    for name in ("cg", "mcg"):                                         # no fused plan
        with pytest.raises(NotImplementedError, match="fused"):
            loop(_sampler(), get_conditioning_method(name, op, noiser, **({} if name == "cg" else {"scale": 0.5})))
    with pytest.raises(NotImplementedError, match="fused"):
        _sampler().p_sample_loop(model=None, x_start=x, measurement=y, measurement_cond_fn=lambda **kw: None, record=False,
                                 save_root=None)
    odd = _sampler()
    odd.hip_posterior = False                                          # another mean / variance parametrisation
    with pytest.raises(NotImplementedError, match="posterior"):
        loop(odd)
    with pytest.raises(RuntimeError, match="MI355X"):                  # everything accepted: the loop asks for the device
        loop(_sampler())


# ------------------------------------------------------------------ the restatement
def _records(oracle):
    sched = oracle.tables.schedule(1000)
    recs = {f"ddpm{t}": oracle.tables.step_coefs(sched, t) for t in (500, 1)}
    recs["ddim500"] = oracle.tables.ddim_step_coefs(sched, 500, 0.5)
    return recs


def test_correction_is_the_density_difference(oracle):
    """corr = log p_u(x_next) - log q(x_next) with x_next = mean_u + sd z - s: pins the sign and the definition"""
    rng = np.random.RandomState(0)
    shape = (3, 2, 9, 7)
    for name, c in _records(oracle).items():
        g_eps, g_unet = (1e-3 * rng.randn(*shape)).astype(np.float32), (1e-3 * rng.randn(*shape)).astype(np.float32)
        v, z = rng.uniform(-1, 1, shape).astype(np.float32), rng.randn(*shape).astype(np.float32)
        mean_u = rng.randn(*shape)
        s = smc_ref.update(g_eps, g_unet, c).astype(np.float64)
        sd = smc_ref.sd(v, c)
        x_next = mean_u + sd * z.astype(np.float64) - s
        corr, scale = smc_ref.correction(g_eps, g_unet, v, z, c)
        want = smc_ref.density_difference(x_next, mean_u, s, sd)
        assert np.all(np.abs(corr) > 0) and np.all(scale >= np.abs(corr)), name
        assert np.allclose(corr, want, rtol=0, atol=1e-9 * scale.max()), (name, corr, want)
    still = dict(_records(oracle)["ddpm500"], add_noise=0)             # a step without noise: 0 by definition
    corr, scale = smc_ref.correction(g_eps, g_unet, v, z, still)
    assert np.array_equal(corr, np.zeros(3)) and np.array_equal(scale, np.zeros(3))
    assert np.array_equal(smc_ref.update(g_eps, None, still), smc_ref.update(g_eps, np.zeros_like(g_eps), still))


def test_proposal_ratio_integrates_to_one():
    """one element with q = 0.5: E_z exp(corr) = E exp(q z - q^2 / 2) = 1.  200,000 seeded normals; the standard error is
    sqrt((e^{q^2} - 1) / n) = 0.0012, the bound five of them"""
    z = np.random.RandomState(7).randn(200_000, 1).astype(np.float32)
    c = {"a": 1.0, "b": -2.0, "c1": 0, "c2": 0, "min_log": 1.0, "max_log": 0.0, "add_noise": 3}   # sd = 1, s = 0.5 g_eps
    corr, _ = smc_ref.correction(np.ones_like(z), None, np.zeros_like(z), z, c)
    assert np.allclose(corr, 0.5 * (z[:, 0].astype(np.float64) - 0.25), atol=1e-12)
    mean = float(np.exp(corr).mean())
    print(f"mean exp(corr) = {mean:.5f}")
    assert abs(mean - 1.0) <= 0.006


def test_accum_restatement():
    E, dp = np.array([1.0, -2.0, 0.5, 0.0], np.float32), np.array([3.0, 4.0, 5.0, 6.0], np.float32)
    dc = np.array([2.0, 5.0, 5.0, 1.0], np.float32)
    part = np.array([[1.0, 2.0], [0.0, -1.0], [0.5, 0.5], [0.0, 0.0]], np.float32)
    e1, d1, mag = smc_ref.accum(E, dp, dc, part, [0, 1], 2, 0.5, 1, 1.0)
    assert np.array_equal(d1, dc)
    assert np.allclose(e1, [1.0 + 0.5 * -1.0 - 3.0, -2.0 + 0.5 * 1.0 + 1.0, 0.0 + 0.0 - 1.0, 0.0 + 0.5 * -5.0 - 0.0])
    assert np.allclose(mag, [1 + 1 + 1.5 + 3, 2 + 2.5 + 2 + 1, 0 + 2.5 + 2.5 + 1, 0 + 0.5 + 3 + 0])
    e2, _, _ = smc_ref.accum(E, dp, dc, None, None, 1, 0.5, 2, 0.0)
    assert np.allclose(e2, E + 0.5 * (dc ** 2 - dp ** 2))


# ------------------------------------------------------------------ the driver
def test_driver_flags_and_refusals(monkeypatch, tmp_path):
    import sys
    sys.path.insert(0, ROOT)
    drv = importlib.import_module("sample_condition_batched_ttc")
    args = drv.parse_args([])
    assert (args.smc_twist_scale, args.smc_twist_power, args.smc_proposal_weight) == (None, None, None)
    assert drv.smc_flags(args) == [] and drv.check_smc(args, "ddpm") is None and drv.check_smc(args, "smc_ddpm") is None
    smc = ["--smc_twist_scale", "0.02", "--smc_twist_power", "2", "--smc_proposal_weight", "0.5"]
    args = drv.parse_args(smc)
    assert drv.smc_flags(args) == [("--smc_twist_scale", 0.02), ("--smc_twist_power", 2), ("--smc_proposal_weight", 0.5)]
    assert drv.check_smc(args, "smc_ddpm") is None
    for k in range(3):                                                   # with another sampler: a one-line refusal
        with pytest.raises(SystemExit) as e:
            drv.check_smc(drv.parse_args(smc[2 * k:2 * k + 2]), "ttc_ddim")
        assert smc[2 * k] in str(e.value) and "smc_ddpm" in str(e.value) and "ttc_ddim)" in str(e.value)
        assert "\n" not in str(e.value)
    with pytest.raises(SystemExit):
        drv.parse_args(["--smc_twist_power", "3"])
    with pytest.raises(SystemExit, match="finite"):
        drv.check_smc(drv.parse_args(["--smc_twist_scale", "nan"]), "smc_ddpm")
    with pytest.raises(SystemExit, match="particle_groups"):
        drv.check_smc(drv.parse_args(["--particle_groups", "2"]), "smc_ddpm")
    with pytest.raises(SystemExit, match="one rank"):
        drv.check_smc(drv.parse_args([]), "smc_ddpm", world=2)
    # the three resampling flags: accepted for smc_ddpm without --resample_draw device, refused as before elsewhere
    rs = ["--resample_scheme", "systematic", "--resample_ess", "0.5", "--ttc_resample_every", "3"]
    assert drv.check_resample_scheme(drv.parse_args(rs), "smc_ddpm") is None
    assert drv.check_resample_scheme(drv.parse_args(["--resample_draw", "device"] + rs), "smc_ddpm") is None
    with pytest.raises(SystemExit, match="--resample_draw device"):
        drv.check_resample_scheme(drv.parse_args(rs), "ttc_ddim")
    with pytest.raises(SystemExit) as e:
        drv.check_resample_scheme(drv.parse_args(["--resample_draw", "device"] + rs), "ddpm")
    assert "is an option of sampler ttc_ddim, the loop that resamples (the diffusion config names ddpm)" in str(e.value)
    with pytest.raises(SystemExit, match="--resample_ess"):
        drv.check_resample_scheme(drv.parse_args(["--resample_ess", "1.5"]), "smc_ddpm")
    with pytest.raises(SystemExit, match="--ttc_resample_every"):
        drv.check_resample_scheme(drv.parse_args(["--ttc_resample_every", "0"]), "smc_ddpm")

    # main(): refusals come before anything touches the GPU; the shipped smc config passes the checks
    def no_gpu(*a, **kw):
        raise AssertionError("the check touched the GPU")
    for fn in ("set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    plain = os.path.join(ROOT, "configs", "diffusion_config.yaml")
    shipped = os.path.join(ROOT, "configs", "diffusion_config_smc.yaml")
    with pytest.raises(SystemExit, match="--smc_proposal_weight"):
        drv.main(["--diffusion_config", plain, "--smc_proposal_weight", "0"])
    with pytest.raises(SystemExit, match="no CPU fallback"):             # accepted: the run itself then needs the device
        drv.main(["--diffusion_config", shipped] + smc + rs)
    with pytest.raises(SystemExit, match="particle_groups"):
        drv.main(["--diffusion_config", shipped, "--particle_groups", "2"])
    import yaml
    a, b = (yaml.load(open(f), Loader=yaml.FullLoader) for f in (plain, shipped))
    assert b["sampler"] == "smc_ddpm" and {k: v for k, v in a.items() if k != "sampler"} == \
        {k: v for k, v in b.items() if k != "sampler"}
