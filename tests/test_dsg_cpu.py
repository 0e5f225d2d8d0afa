"""CPU suite of spherical-Gaussian guidance (`dsg`): the name in the header / the exports / the ctypes table, every
refusal of dpsx_step_update_dsg_f32 without a GPU, the method's registry entry, its fused_spec, the shipped YAMLs, what
the samplers and the driver refuse before the model is called, and the float64 restatement tests/dsg_ref.py (the
reference of the GPU suite) against the method's geometry."""
import ctypes
import importlib
import os
import re
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch
import yaml

import dsg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"          # operators build their device handle lazily: constructing them needs no GPU
NAME = "dpsx_step_update_dsg_f32"


def test_header_export_and_signature():
    from dps_ttc_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpsx.h")).read(), flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", hdr) and hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    p = ctypes.c_void_p
    corr = list(_lib.SIGNATURES["dpsx_step_update_corr_f32"][1])        # ..., noise, rng | x_next, partials, n, chw, coefs, stream
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, corr[:6] + [ctypes.c_float] + corr[6:])
    assert corr[6:8] == [p, p]


def _coefs(mode=1, b=2.0, sigma=-9.0):
    from dps_ttc_amd import kernels
    c = kernels.make_coefs(1.5, b, 0.5, 0.5, sigma, -4.0, True)
    c.add_noise = mode
    return c


def test_update_dsg_refuses_on_the_host():
    """every DPSX_EINVAL / DPSX_EUNSUPPORTED of dpsx_step_update_dsg_f32, with pointers that must never be dereferenced:
    there is no GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, q = _lib.lib(), c_void_p(0x1000)
    rng, ok = _lib.RngRec(1, 2, 0, 0, 0), _coefs()

    def call(sample=q, g=q, gu=q, mo=q, noise=q, r=None, rate=0.1, out=q, stats=q, n=2, chw=8, c=ok):
        return lib.dpsx_step_update_dsg_f32(sample, g, gu, mo, noise, None if r is None else byref(r), rate, out, stats, n,
                                            chw, None if c is None else byref(c), None)

    assert call(noise=q, r=rng) == _lib.EINVAL                        # both noise sources
    assert call(noise=None, r=None) == _lib.EINVAL                    # neither
    assert call(c=_coefs(mode=0), noise=None, r=None) == _lib.EINVAL  # ... whatever the step
    for kw in (dict(sample=None), dict(g=None), dict(out=None), dict(stats=None), dict(c=None), dict(n=-1), dict(chw=-1),
               dict(mo=None)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(c=_coefs(b=0.0)) == _lib.EINVAL
    for rate in (-0.01, 1.01, float("nan"), float("inf"), float("-inf")):
        assert call(rate=rate) == _lib.EINVAL, rate
    for sigma in (0.0, -0.1, float("nan")):                           # a DDIM record that adds noise on a sphere of radius 0
        assert call(c=_coefs(mode=3, sigma=sigma)) == _lib.EINVAL, sigma
    assert call(noise=None, r=_lib.RngRec(1, 2, 0, -1, 0)) == _lib.EINVAL          # a bad rng record
    assert call(noise=None, r=_lib.RngRec(1, 2, 0, 0xffffffff, 0)) == _lib.EINVAL  # particle ids past 32 bits
    assert call(n=65536) == _lib.EUNSUPPORTED
    for rate in (0.0, 1.0):
        assert call(n=0, rate=rate) == _lib.OK and call(chw=0, rate=rate) == _lib.OK       # nothing to do, nothing launched


# ------------------------------------------------------------------ the method
def _method(name="gaussian_blur", noise=("gaussian", dict(sigma=0.05)), **params):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    kw = {"gaussian_blur": dict(kernel_size=61, intensity=3.0), "inpainting": {}}[name]
    return get_conditioning_method("dsg", get_operator(name, device=DEV, **kw), get_noise(noise[0], **noise[1]), **params)


def test_registry_rate_and_fused_spec():
    from dps_ttc_amd import condition_methods as CM
    # not in the table that mirrors the reference's, and apart from the extensions whose conditioning() a loop calls
    assert "dsg" not in CM.__CONDITIONING_METHOD__ and "dsg" not in CM.__EXTENSION_METHOD__
    assert CM.__FUSED_ONLY_METHOD__ == {"dsg": CM.SphericalGaussianGuidance}
    for kw in (dict(extension=True), dict(extension=True, fused_only=True), {}):
        with pytest.raises(NameError, match="already registered"):
            CM.register_conditioning_method(name="dsg", **kw)(object)
    with pytest.raises(NameError, match="already registered"):
        CM.register_conditioning_method(name="cg", extension=True, fused_only=True)(object)
    with pytest.raises(ValueError, match="fused_only"):
        CM.register_conditioning_method(name="other", fused_only=True)
    cm = _method()
    assert isinstance(cm, CM.ConditioningMethod) and cm.returns_gradient is False and cm.guidance_rate == 0.1
    assert cm.fused_spec() == {"scale": 1.0, "power": 1, "dsg": 0.1}
    assert cm.fused_spec(beta_scale=0.3, t=0.5, norm_exp=2) == {"scale": 1.0, "power": 1, "dsg": 0.1}
    assert _method(guidance_rate=0.0).fused_spec()["dsg"] == 0.0 and _method(guidance_rate=1).fused_spec()["dsg"] == 1.0
    assert _method(noise=("poisson", dict(rate=1.0))).fused_spec() is None
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance_rate"):
            _method(guidance_rate=bad)
    with pytest.raises(NotImplementedError, match="fused"):
        cm.conditioning(x_t=torch.zeros(1, 3, 8, 8), measurement=torch.zeros(1, 3, 8, 8))


def test_shipped_yamls():
    from dps_ttc_amd.gaussian_diffusion import DDIM, create_sampler
    load = lambda f: yaml.load(open(os.path.join(ROOT, "configs", f)), Loader=yaml.FullLoader)
    for f, op in (("gaussian_deblur_config_dsg.yaml", "gaussian_blur"), ("super_resolution_config_dsg.yaml", "super_resolution")):
        cfg = load(f)
        assert cfg["conditioning"] == {"method": "dsg", "params": {"guidance_rate": 0.1}}
        assert cfg["measurement"]["operator"]["name"] == op and cfg["measurement"]["noise"]["name"] == "gaussian"
        plain = load(f.replace("_dsg", ""))
        assert {k: v for k, v in cfg.items() if k != "conditioning"} == {k: v for k, v in plain.items() if k != "conditioning"}
    diff = load("diffusion_config_dsg.yaml")
    assert diff["sampler"] == "ddim" and diff["timestep_respacing"] == "ddim100" and diff["eta"] == 1.0
    smp = create_sampler(**diff)
    assert isinstance(smp, DDIM) and smp.num_timesteps == 100 and smp.eta == 1.0 and smp.hip_posterior
    ck = smp.sample_coefs(50)
    assert ck.add_noise == 3 and ck.min_log > 0                        # every noisy step has a sphere to sit on
    # eta is the ddim samplers' option, in [0, 1]
    with pytest.raises(ValueError, match="eta"):
        create_sampler(**dict(diff, sampler="ddpm"))
    with pytest.raises(ValueError, match="eta"):
        create_sampler(**dict(diff, eta=1.5))
    assert create_sampler(**{k: v for k, v in diff.items() if k != "eta"}).eta == 0.0


def _sampler(name="ddpm", respacing="20", var="learned_range", eta=None):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    kw = {} if eta is None else {"eta": eta}
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type=var,
                          dynamic_threshold=False, clip_denoised=True, rescale_timesteps=True, timestep_respacing=respacing,
                          **kw)


def test_samplers_refuse_before_the_model_is_called():
    """CPU tensors and a model that raises when called: every refusal must come first, with its reason in the message"""
    def model(*a, **kw):
        raise AssertionError("the model was called")

    x, y = torch.zeros(4, 3, 64, 64), torch.zeros(1, 3, 64, 64)

    def loop(smp, fn, x=x, **kw):
        return smp.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, record=False, save_root=None,
                                 **kw)

    cm = _method()
    with pytest.raises(NotImplementedError, match="fixed-variance"):                  # no fused plan: the model's variance
        loop(_sampler(var="fixed_small"), cm.conditioning)
    with pytest.raises(NotImplementedError, match="Gaussian noiser"):                 # ... the noiser
        loop(_sampler(), _method(noise=("poisson", dict(rate=1.0))).conditioning)
    inp = _method("inpainting")
    with pytest.raises(NotImplementedError, match="mask"):                            # ... inpainting without its mask
        loop(_sampler(), inp.conditioning)
    import functools
    odd = torch.zeros(2, 3, 33, 47)
    with pytest.raises(NotImplementedError, match="float4 grid"):                     # ... inpainting off the float4 grid
        loop(_sampler(), functools.partial(inp.conditioning, mask=torch.ones(1, 1, 33, 47)), x=odd)
    for name in ("ddim", "ttc_ddim"):                                                 # eta = 0: r = 0
        with pytest.raises(ValueError, match="eta = 0"):
            loop(_sampler(name), cm.conditioning)
    with pytest.raises(NotImplementedError, match="smc_ddpm"):                        # the Gaussian-shift proposal
        loop(_sampler("smc_ddpm"), cm.conditioning)
    # accepted: the loop then asks for the device (rng_parity included: that path supplies the noise tensor)
    par = _sampler()
    par.rng_parity = True
    for smp in (_sampler(), par, _sampler("ddim", eta=1.0), _sampler("ttc_ddim", eta=0.5)):
        with pytest.raises(RuntimeError, match="MI355X"):
            loop(smp, cm.conditioning)


def test_driver_flag(monkeypatch):
    import sys
    sys.path.insert(0, ROOT)
    drv = importlib.import_module("sample_condition_batched_ttc")
    assert drv.parse_args([]).dsg_guidance_rate is None and drv.check_dsg(drv.parse_args([]), "ps") is None
    args = drv.parse_args(["--dsg_guidance_rate", "0.25"])
    assert args.dsg_guidance_rate == 0.25 and drv.check_dsg(args, "dsg") is None
    with pytest.raises(SystemExit) as e:
        drv.check_dsg(args, "ps")
    assert "--dsg_guidance_rate" in str(e.value) and "method dsg" in str(e.value) and "ps)" in str(e.value)
    assert "\n" not in str(e.value)
    for bad in ("-0.1", "1.5", "nan"):
        with pytest.raises(SystemExit, match="\\[0, 1\\]"):
            drv.check_dsg(drv.parse_args(["--dsg_guidance_rate", bad]), "dsg")

    # main(): the refusal comes before anything touches the GPU; the shipped configs pass the checks
    def no_gpu(*a, **kw):
        raise AssertionError("the check touched the GPU")
    for fn in ("set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = lambda f: os.path.join(ROOT, "configs", f)
    with pytest.raises(SystemExit, match="method dsg"):
        drv.main(["--diffusion_config", cfg("diffusion_config_dsg.yaml"), "--task_config", cfg("gaussian_deblur_config.yaml"),
                  "--dsg_guidance_rate", "0.2"])
    with pytest.raises(SystemExit, match="no CPU fallback"):             # accepted: the run itself then needs the device
        drv.main(["--diffusion_config", cfg("diffusion_config_dsg.yaml"),
                  "--task_config", cfg("gaussian_deblur_config_dsg.yaml"), "--dsg_guidance_rate", "0.2"])


# ------------------------------------------------------------------ the restatement
REC = dict(a=1.4, b=0.98, c1=0.2, c2=0.8, min_log=-6.0, max_log=-4.5, add_noise=1)
DDIM_REC = dict(REC, min_log=0.07, add_noise=3)


def _inputs(seed, n=3, shape=(2, 9, 7)):
    rng = np.random.RandomState(seed)
    full = (n,) + shape
    f = np.float32
    return dict(sample=rng.randn(*full).astype(f), g_eps=(1e-3 * rng.randn(*full)).astype(f),
                g_unet=(1e-3 * rng.randn(*full)).astype(f), v=rng.uniform(-1, 1, full).astype(f), z=rng.randn(*full).astype(f))


def _flat_norm(a):
    return np.sqrt((a.reshape(a.shape[0], -1) ** 2).sum(axis=1))


@pytest.mark.parametrize("rec", [REC, DDIM_REC], ids=["ddpm", "ddim"])
def test_restatement_has_the_methods_geometry(rec):
    d = _inputs(3)
    import smc_ref
    s = smc_ref.update(d["g_eps"], d["g_unet"], rec).astype(np.float64)
    bc = lambda a: a.reshape(-1, 1, 1, 1)
    for g in (0.0, float(np.float32(0.1)), 0.5, 1.0):                    # the rate travels as one fp32
        out = dsg_ref.restate(d["sample"], d["g_eps"], d["g_unet"], d["v"], d["z"], rec, g)
        mean = d["sample"].astype(np.float64) - out["n"]
        r = out["r"]
        assert np.all(r > 0) and np.allclose(out["R"], r ** 2)
        # on the sphere of radius r around the mean, whatever g
        assert np.allclose(_flat_norm(out["x_next"] - mean), r, rtol=1e-12)
        assert np.allclose(out["x_next"] - mean, out["D"], rtol=0, atol=1e-14)
        # D = r m / ||m||, m = n + g (d* - n), d* = -r s / ||s||
        m = out["n"] + g * (-bc(r) * s / bc(_flat_norm(s)) - out["n"])
        assert np.allclose(out["D"], bc(r) * m / bc(_flat_norm(m)), rtol=1e-11, atol=1e-15)
        if g == 1.0:
            assert np.allclose(out["x_next"], mean - bc(r) * s / bc(_flat_norm(s)), rtol=1e-12, atol=1e-15)
        if g == 0.0:
            assert np.allclose(out["x_next"], mean + bc(r) * out["n"] / bc(_flat_norm(out["n"])), rtol=1e-12, atol=1e-15)
    if rec["add_noise"] & 2:                                              # a DDIM record: sd = sigma for every element
        assert np.allclose(out["R"], d["z"][0].size * np.float64(np.float32(rec["min_log"])) ** 2)


def test_restatement_degenerate_cases():
    d = _inputs(4)
    zero = np.zeros_like(d["g_eps"])
    out = dsg_ref.restate(d["sample"], zero, zero, d["v"], d["z"], REC, 0.3)           # S = 0
    assert np.array_equal(out["x_next"], d["sample"].astype(np.float64)) and np.all(out["S"] == 0)
    assert np.all(out["alpha"] == 1) and np.all(out["beta"] == 0)
    out = dsg_ref.restate(d["sample"], zero, None, d["v"], d["z"], REC, 0.3)
    assert np.array_equal(out["x_next"], d["sample"].astype(np.float64))
    out = dsg_ref.restate(d["sample"], d["g_eps"], d["g_unet"], d["v"], d["z"], dict(REC, add_noise=0), 0.3)   # r = 0
    assert np.array_equal(out["x_next"], d["sample"].astype(np.float64))
    assert all(np.all(out[k] == 0) for k in ("S", "Nn", "C", "R"))
    g_nan = d["g_unet"].copy()                                            # a NaN stays inside its particle
    g_nan[1, 0, 2, 2] = np.nan
    clean = dsg_ref.restate(d["sample"], d["g_eps"], d["g_unet"], d["v"], d["z"], REC, 0.3)
    out = dsg_ref.restate(d["sample"], d["g_eps"], g_nan, d["v"], d["z"], REC, 0.3)
    assert np.array_equal(out["x_next"][[0, 2]], clean["x_next"][[0, 2]])
    assert np.array_equal(out["x_next"][1], d["sample"][1].astype(np.float64))        # S is NaN: not > 0
