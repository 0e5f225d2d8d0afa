"""CPU suite of the DPM-Solver++(2M) option of the ddim samplers: the identities that make the DDIM record its first-order
step, the order the multistep term buys on an analytic model (tests/dpmpp_ref.py, float64), the log-SNR spacing, the new
entry point's surface and every refusal of it without a GPU, what the samplers and the driver refuse before the model is
called, and guidance_gain = "span"."""
import ctypes
import functools
import importlib
import os
import re
from ctypes import byref, c_void_p

import numpy as np
import pytest
import torch
import yaml

import dpmpp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"          # operators build their device handle lazily: constructing them needs no GPU
NAME = "dpsx_step_update_ms_f32"
BETAS = np.linspace(1e-4, 2e-2, 1000, dtype=np.float64)


def _sampler(name="ddim", respacing="logsnr20", var="learned_range", **kw):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type=var,
                          dynamic_threshold=False, clip_denoised=True, rescale_timesteps=True, timestep_respacing=respacing,
                          **kw)


# ------------------------------------------------------------------ 1: the identities
@pytest.mark.parametrize("respacing", ["logsnr20", "ddim50"])
def test_the_ddim_record_is_the_first_order_step(respacing):
    """float64, 1e-12 relative, every kept step: eta = 0: (c1, c2) = (alpha_t, sigma_t) of the landing point, i.e.
    x_t = alpha_t x0 + sigma_t eps = (sigma_t / sigma_s) x_s - alpha_t (e^{-h} - 1) x0; eta = 1: the record's noise
    variance is sigma_t^2 (1 - e^{-2h})"""
    smp = _sampler(respacing=respacing)
    abar = smp.alphas_cumprod
    assert np.allclose(abar, np.cumprod(1.0 - BETAS)[smp.timestep_map], rtol=1e-13, atol=0)   # re-multiplied betas
    lam = dpmpp_ref.lambdas(abar)
    close = lambda a, b: abs(a - b) <= 1e-12 * abs(b)
    for i in range(1, len(abar)):
        alpha_t, sigma_t = np.sqrt(abar[i - 1]), np.sqrt(1.0 - abar[i - 1])
        alpha_s, sigma_s = np.sqrt(abar[i]), np.sqrt(1.0 - abar[i])
        h = lam[i - 1] - lam[i]
        assert h > 0
        _, _, c1, c2, sigma = dpmpp_ref.ddim_record(abar, i, 0.0)
        assert sigma == 0.0 and close(c1, alpha_t) and close(c2, sigma_t)
        # ... which is the exponential-integrator form: the coefficient of x_s and of x0 with eps = (x_s - alpha_s x0) / sigma_s
        assert close(c2 / sigma_s, sigma_t / sigma_s) and close(c1 - c2 * alpha_s / sigma_s, -alpha_t * np.expm1(-h))
        _, _, _, _, sigma = dpmpp_ref.ddim_record(abar, i, 1.0)
        assert close(sigma ** 2, sigma_t ** 2 * -np.expm1(-2.0 * h))


# ------------------------------------------------------------------ 2: the order
def _err(n, order, eta=0.0):
    """RMS error of the state entering the last step against the exact probability-flow solution (4096 elements, seed 0)"""
    abar = np.cumprod(1.0 - BETAS)[dpmpp_ref.logsnr_steps(BETAS, n)]
    g = dpmpp_ref.GaussModel(abar, m=0.2, v=0.04)
    x_T = g.draw(len(abar) - 1, 4096, seed=0)
    got = dpmpp_ref.loop_f64(abar, g.eps, x_T, order, eta=eta, stop=1)
    return float(np.sqrt(np.mean((got - g.flow(x_T, len(abar) - 1, 0)) ** 2)))


def test_the_multistep_term_buys_an_order():
    e1 = {n: _err(n, 1) for n in (10, 20, 40)}
    e2 = {n: _err(n, 2) for n in (10, 20, 25, 40, 100)}
    print("order 1:", e1, "order 2:", e2)
    for n in (10, 20, 40):
        assert e2[n] <= 0.2 * e1[n], (n, e1[n], e2[n])
    assert e2[100] <= e2[25] / 4
    assert e1[40] <= 0.6 * e1[20]


# ------------------------------------------------------------------ 3: the spacing and the table
def test_logsnr_spacing_and_the_coefficients():
    from dps_ttc_amd.gaussian_diffusion import logsnr_timesteps, space_timesteps
    for n in (2, 10, 20, 25, 40, 100, 1000):
        kept = sorted(logsnr_timesteps(BETAS, n))
        assert kept == dpmpp_ref.logsnr_steps(BETAS, n)
        assert kept[0] == 0 and kept[-1] == 999 and len(kept) <= n and len(set(kept)) == len(kept)
        smp = _sampler(respacing=f"logsnr{n}")
        assert smp.timestep_map == kept and smp.num_timesteps == len(kept)
    assert len(logsnr_timesteps(BETAS, 20)) == 20 and len(logsnr_timesteps(BETAS, 40)) == 39
    for bad in ("logsnr1", "logsnr0"):
        with pytest.raises(ValueError, match="at least 2"):
            _sampler(respacing=bad)
    # every other spec is untouched
    assert space_timesteps(1000, "ddim50") == set(range(0, 1000, 20)) and _sampler(respacing="ddim50").num_timesteps == 50
    assert _sampler(respacing="250").timestep_map == sorted(space_timesteps(1000, "250"))
    assert sorted(space_timesteps(1000, "250"))[:3] == [0, 4, 8] and len(space_timesteps(1000, "250")) == 250
    with pytest.raises(ValueError):
        space_timesteps(1000, "logsnr20")                                 # the betas are create_sampler's
    # c: the restatement's, rounded to fp32 once; 0 at both ends, positive between; order 1: 0 everywhere
    for respacing in ("logsnr20", "ddim50"):
        for eta in (0.0, 1.0):
            smp = _sampler(respacing=respacing, eta=eta, solver_order=2)
            n = smp.num_timesteps
            want = dpmpp_ref.c32(smp.alphas_cumprod, eta)
            got = np.array([smp.solver_coef(i) for i in range(n)])
            assert np.array_equal(got.astype(np.float32), want) and np.array_equal(got, want.astype(np.float64))
            assert got[0] == 0 and got[n - 1] == 0 and np.all(got[1:n - 1] > 0)
            smp.solver_order = 1
            assert all(smp.solver_coef(i) == 0.0 for i in range(n))
            assert smp.sample_coefs(3) is _sampler(respacing=respacing, eta=eta).sample_coefs(3) or \
                bytes(smp.sample_coefs(3)) == bytes(_sampler(respacing=respacing, eta=eta).sample_coefs(3))


# ------------------------------------------------------------------ 4: the surface
def test_header_export_and_signature():
    from dps_ttc_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpsx.h")).read(), flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", hdr) and hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    p, upd = ctypes.c_void_p, list(_lib.SIGNATURES["dpsx_step_update_f32"][1])   # sample, g, gu | x_next, n, chw, coefs, stream
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, upd[:3] + [p, p, ctypes.c_float] + upd[3:])


def _coefs(b=2.0):
    from dps_ttc_amd import kernels
    return kernels.make_ddim_coefs(1.5, b, 0.5, 0.6, 0.0, True)


def test_update_ms_refuses_on_the_host():
    """every DPSX_EINVAL / DPSX_EUNSUPPORTED of the entry point, with pointers that must never be dereferenced: there is no
    GPU here, so a launch would show"""
    from dps_ttc_amd import _lib
    lib, q, ok = _lib.lib(), c_void_p(0x1000), _coefs()

    def call(sample=q, g=q, gu=q, cur=q, prev=q, c=0.25, out=q, n=2, chw=8, k=ok):
        return lib.dpsx_step_update_ms_f32(sample, g, gu, cur, prev, c, out, n, chw, None if k is None else byref(k), None)

    for kw in (dict(sample=None), dict(g=None), dict(out=None), dict(k=None), dict(n=-1), dict(chw=0), dict(chw=-1),
               dict(cur=None), dict(prev=None), dict(cur=None, prev=None)):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(k=_coefs(b=0.0)) == _lib.EINVAL
    for c in (float("nan"), float("inf"), float("-inf")):
        assert call(c=c) == _lib.EINVAL, c
        assert call(c=c, cur=None, prev=None) == _lib.EINVAL, c
    for c in (0.25, 0.0, -0.05):
        assert call(c=c, n=65536) == _lib.EUNSUPPORTED
    assert call(n=-1, chw=0, c=float("nan")) == _lib.EINVAL and call(n=65536, chw=0) == _lib.EINVAL   # EINVAL comes first
    for c in (0.25, 0.0):
        assert call(n=0, c=c) == _lib.OK                                  # nothing to do, nothing launched
    assert call(n=0, c=0.0, cur=None, prev=None, gu=None) == _lib.OK      # c = 0 takes null histories


# ------------------------------------------------------------------ 5: the refusals
def _method(name="ps", op="gaussian_blur", noise=("gaussian", dict(sigma=0.05)), **params):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    kw = {"gaussian_blur": dict(kernel_size=61, intensity=3.0), "inpainting": {}}[op]
    if not params:
        params = {"ps": dict(scale=0.3), "mcg": dict(scale=0.3), "cg": dict(rho_scale=1.0, iters=3),
                  "dsg": dict(guidance_rate=0.2)}[name]
    return get_conditioning_method(name, get_operator(op, device=DEV, **kw), get_noise(noise[0], **noise[1]), **params)


def test_create_sampler_options():
    from dps_ttc_amd.gaussian_diffusion import DDIM
    smp = _sampler()
    assert isinstance(smp, DDIM) and smp.solver_order == 1 and smp.guidance_gain == "unit" and smp.eta == 0.0
    assert _sampler(solver_order=2).solver_order == 2 and _sampler("ttc_ddim", solver_order=2, eta=1.0).solver_order == 2
    assert _sampler(solver_order=1, eta=0.5).solver_order == 1            # order 1 takes any eta
    for name in ("ddpm", "search_ddpm", "smc_ddpm"):
        for order in (1, 2):
            with pytest.raises(ValueError, match="solver_order"):
                _sampler(name, solver_order=order)
    for eta in (0.5, 0.999):
        with pytest.raises(ValueError, match="eta = 0"):
            _sampler(eta=eta, solver_order=2)
    for bad in (0, 3, 2.5, "2", True):
        with pytest.raises(ValueError, match="solver_order must be 1 or 2"):
            _sampler(solver_order=bad)
    # the shipped config goes through create_sampler(**diffusion_config)
    load = lambda f: yaml.load(open(os.path.join(ROOT, "configs", f)), Loader=yaml.FullLoader)
    cfg, dsg = load("diffusion_config_dpmpp.yaml"), load("diffusion_config_dsg.yaml")
    assert (cfg["sampler"], cfg["timestep_respacing"], cfg["eta"], cfg["solver_order"]) == ("ddim", "logsnr20", 0.0, 2)
    drop = ("timestep_respacing", "eta", "solver_order")
    assert {k: v for k, v in cfg.items() if k not in drop} == {k: v for k, v in dsg.items() if k not in drop}
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    smp = create_sampler(**cfg)
    assert smp.solver_order == 2 and smp.num_timesteps == 20 and smp.solver_coef(10) > 0 and smp.hip_posterior


def test_samplers_refuse_before_the_model_is_called():
    """CPU tensors and a model that raises when called: every refusal must come first, with its reason in the message"""
    def model(*a, **kw):
        raise AssertionError("the model was called")

    x, y = torch.zeros(4, 3, 64, 64), torch.zeros(1, 3, 64, 64)

    def loop(smp, fn, x=x, **kw):
        return smp.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, record=False, save_root=None,
                                 **kw)

    def second(name="ddim", **kw):
        return _sampler(name, solver_order=2, **kw)

    ps, NI = _method("ps"), NotImplementedError
    for name in ("ddim", "ttc_ddim"):
        with pytest.raises(NI, match="solver_order = 2.*per-op methods"):                # a per-op method
            loop(second(name), _method("mcg").conditioning)
        with pytest.raises(NI, match="solver_order = 2.*fixed-variance"):                # the model's variance
            loop(second(name, var="fixed_small"), ps.conditioning)
        with pytest.raises(NI, match="solver_order = 2.*Gaussian noiser"):               # the noiser
            loop(second(name), _method("ps", noise=("poisson", dict(rate=1.0))).conditioning)
        with pytest.raises(NI, match="solver_order = 2.*cg step"):
            loop(second(name), _method("cg").conditioning)
        with pytest.raises(NI, match="solver_order = 2.*dsg"):
            loop(second(name, eta=1.0), _method("dsg").conditioning)
    inp = _method("ps", op="inpainting")
    with pytest.raises(NI, match="solver_order = 2.*mask"):                              # inpainting without its mask
        loop(second(), inp.conditioning)
    odd = torch.zeros(2, 3, 33, 47)
    with pytest.raises(NI, match="solver_order = 2.*float4 grid"):                       # ... off the float4 grid
        loop(second(), functools.partial(inp.conditioning, mask=torch.ones(1, 1, 33, 47)), x=odd)
    with pytest.raises(NI, match="solver_order = 2.*project=True"):                      # DiffStateGrad
        loop(second(), ps.conditioning, project=True)
    glob = second("ttc_ddim")
    glob.global_resample = True
    with pytest.raises(NI, match="solver_order = 2.*multi-rank"):
        loop(glob, ps.conditioning)
    # the attributes set after construction are checked by the loops too
    smp = _sampler(eta=0.5)
    smp.solver_order = 2
    with pytest.raises(ValueError, match="eta = 0"):
        loop(smp, ps.conditioning)
    smp = _sampler("ddpm", respacing="20")
    smp.solver_order = 2
    with pytest.raises(ValueError, match="ddim samplers"):
        loop(smp, ps.conditioning)
    smp = _sampler()
    smp.guidance_gain = "double"
    with pytest.raises(ValueError, match="guidance_gain"):
        loop(smp, ps.conditioning)
    # guidance_gain = "span": no fused plan, dsg, cg
    for name, respacing in (("ddim", "logsnr20"), ("ttc_ddim", "logsnr20"), ("ddpm", "20")):
        def span(**kw):
            smp = _sampler(name, respacing=respacing, **kw)
            smp.guidance_gain = "span"
            return smp
        with pytest.raises(NI, match="guidance_gain = 'span'.*per-op methods"):
            loop(span(), _method("mcg").conditioning)
        with pytest.raises(NI, match="guidance_gain = 'span'.*fixed-variance"):
            loop(span(var="fixed_small"), ps.conditioning)
        with pytest.raises(NI, match="guidance_gain = 'span'.*dsg"):
            loop(span(**({} if name == "ddpm" else {"eta": 1.0})), _method("dsg").conditioning)   # (dsg wants noise)
        with pytest.raises(NI, match="guidance_gain = 'span'.*cg step"):
            loop(span(), _method("cg").conditioning)
        with pytest.raises(RuntimeError, match="MI355X"):                                # accepted: the loop asks for the device
            loop(span(), ps.conditioning)
    # accepted: order 2 with eta 0 and 1, rng_parity, particle groups
    par = second()
    par.rng_parity = True
    grp = second(eta=1.0)
    grp.particle_groups = 2
    for smp in (second(), second(eta=1.0), par, grp, second("ttc_ddim"), second("ttc_ddim", eta=1.0)):
        with pytest.raises(RuntimeError, match="MI355X"):
            loop(smp, ps.conditioning)


def test_guidance_gain_span_scales_the_spec():
    ps = _method("ps")
    for name, respacing in (("ddim", "logsnr20"), ("ddim", "ddim50"), ("ddpm", "250"), ("ttc_ddim", "logsnr10")):
        smp = _sampler(name, respacing=respacing)
        tm, n = smp.timestep_map, smp.num_timesteps
        spans = [tm[0] + 1] + [tm[i] - tm[i - 1] for i in range(1, n)]
        assert sum(spans) == tm[-1] + 1 and [smp._step_span(i) for i in range(n)] == spans
        unit = [smp._step_spec(i, ps, {}, None) for i in range(n)]
        assert all(s == {"scale": 0.3, "power": 1} for s in unit)
        smp.guidance_gain = "span"
        for i in range(n):
            assert smp._step_spec(i, ps, {}, None) == {"scale": 0.3 * spans[i], "power": 1}
            assert smp._step_spec(i, ps, {}, {}) == {"scale": 0.3 * spans[i], "power": 1}
        assert ps.fused_spec() == {"scale": 0.3, "power": 1}              # the method's own spec is not touched
    full = _sampler("ddpm", respacing="")                                # the full schedule: the identity
    full.guidance_gain = "span"
    assert all(full._step_spec(i, ps, {}, None) == {"scale": 0.3, "power": 1} for i in (0, 1, 500, 999))


def test_driver_flags(monkeypatch):
    import sys
    sys.path.insert(0, ROOT)
    drv = importlib.import_module("sample_condition_batched_ttc")
    none = drv.parse_args([])
    assert none.solver_order is None and none.guidance_gain is None and drv.check_solver(none, "ddpm", "ps") is None
    args = drv.parse_args(["--solver_order", "2", "--guidance_gain", "span"])
    assert args.solver_order == 2 and args.guidance_gain == "span"
    for name in ("ddim", "ttc_ddim"):
        assert drv.check_solver(args, name, "ps") is None and drv.check_solver(args, name, "ps", eta=1.0) is None
    for bad in (["--solver_order", "3"], ["--solver_order", "0"], ["--guidance_gain", "twice"]):
        with pytest.raises(SystemExit):
            drv.parse_args(bad)
    two = drv.parse_args(["--solver_order", "2"])
    for name in ("ddpm", "search_ddpm", "smc_ddpm", None):
        with pytest.raises(SystemExit) as e:
            drv.check_solver(two, name, "ps")
        assert "--solver_order" in str(e.value) and "ddim" in str(e.value) and "\n" not in str(e.value)
    for method in ("cg", "dsg"):
        with pytest.raises(SystemExit, match=f"--solver_order 2.*{method}"):
            drv.check_solver(two, "ddim", method)
        with pytest.raises(SystemExit, match=f"--guidance_gain span.*{method}"):
            drv.check_solver(drv.parse_args(["--guidance_gain", "span"]), "ddpm", method)
    with pytest.raises(SystemExit, match="eta 0 or 1"):
        drv.check_solver(two, "ddim", "ps", eta=0.5)
    with pytest.raises(SystemExit, match="several ranks"):
        drv.check_solver(two, "ttc_ddim", "ps", world=2)
    assert drv.check_solver(two, "ddim", "ps", world=2) is None
    assert drv.check_solver(drv.parse_args(["--solver_order", "1"]), "ddim", "dsg", eta=0.5) is None

    # main(): the refusal comes before anything touches the GPU; the shipped config passes the checks
    def no_gpu(*a, **kw):
        raise AssertionError("the check touched the GPU")
    for fn in ("set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = lambda f: os.path.join(ROOT, "configs", f)
    with pytest.raises(SystemExit, match="samplers ddim and ttc_ddim"):
        drv.main(["--diffusion_config", cfg("diffusion_config.yaml"), "--task_config", cfg("gaussian_deblur_config.yaml"),
                  "--solver_order", "2"])
    with pytest.raises(SystemExit, match="method dsg"):
        drv.main(["--diffusion_config", cfg("diffusion_config_dpmpp.yaml"),
                  "--task_config", cfg("gaussian_deblur_config_dsg.yaml"), "--solver_order", "2"])
    with pytest.raises(SystemExit, match="no CPU fallback"):             # accepted: the run itself then needs the device
        drv.main(["--diffusion_config", cfg("diffusion_config_dpmpp.yaml"),
                  "--task_config", cfg("gaussian_deblur_config.yaml"), "--solver_order", "2", "--guidance_gain", "span"])
