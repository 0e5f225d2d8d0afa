"""CPU suite of pseudoinverse guidance on the CG solve (`pgdm`): the registry entry, the parameter errors, the host scalars
against the float64 formulas, the push-through identity and the analytic model in tests/pgdm_ref.py (the definition's
reference), the shipped YAMLs, and what the samplers and the driver refuse before the model or the device is asked for
anything (the entry point's own refusals need an operator handle, hence a device: tests/test_pgdm_gpu.py)."""
import ctypes
import functools
import importlib
import os
import re
from ctypes import c_void_p

import numpy as np
import pytest
import torch
import yaml

import pgdm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"          # operators build their device handle lazily: constructing them needs no GPU
NAME = "dpsx_cg_pullback_f32"


def _method(name="gaussian_blur", noise=("gaussian", dict(sigma=0.05)), **params):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    kw = {"gaussian_blur": dict(kernel_size=61, intensity=3.0), "inpainting": {}, "phase_retrieval": dict(oversample=2.0)}[name]
    return get_conditioning_method("pgdm", get_operator(name, device=DEV, **kw), get_noise(noise[0], **noise[1]), **params)


def _sampler(name="ddpm", respacing="20", var="learned_range", eta=None):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    kw = {} if eta is None else {"eta": eta}
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type=var,
                          dynamic_threshold=False, clip_denoised=True, rescale_timesteps=True, timestep_respacing=respacing,
                          **kw)


# ------------------------------------------------------------------ 1. the registry
def test_registry_and_abi():
    from dps_ttc_amd import _lib
    from dps_ttc_amd import condition_methods as CM
    cm = _method()
    assert isinstance(cm, CM.PseudoInverseGuidance) and isinstance(cm, CM.ConditioningMethod)
    assert cm.returns_gradient is False and cm.fused_spec() is None
    assert (cm.iters, cm.weighting, cm.weight, cm.noise_sigma) == (5, "score", 1.0, 0.05)
    # absent from the three pinned tables, which keep what they had
    for table in (CM.__CONDITIONING_METHOD__, CM.__EXTENSION_METHOD__, CM.__FUSED_ONLY_METHOD__):
        assert "pgdm" not in table
    assert sorted(CM.__EXTENSION_METHOD__) == ["cg"] and sorted(CM.__FUSED_ONLY_METHOD__) == ["dsg"]
    assert CM.__LATER_EXTENSION_METHOD__["pgdm"] is CM.PseudoInverseGuidance
    # one name, once, across all tables -- in every direction
    for kw in ({}, dict(extension=True), dict(extension=True, fused_only=True), dict(extension=True, later=True)):
        with pytest.raises(NameError, match="already registered"):
            CM.register_conditioning_method(name="pgdm", **kw)(object)
    for name in ("ps", "cg", "dsg"):
        with pytest.raises(NameError, match="already registered"):
            CM.register_conditioning_method(name=name, extension=True, later=True)(object)
    with pytest.raises(ValueError, match="later"):
        CM.register_conditioning_method(name="other", later=True)
    with pytest.raises(NameError, match="not defined"):
        CM.get_conditioning_method("no_such_method", cm.operator, cm.noiser)
    with pytest.raises(NotImplementedError, match="model's graph"):
        cm.conditioning(x_t=torch.zeros(1, 3, 8, 8), measurement=torch.zeros(1, 3, 8, 8))
    # the entry point: header, export, ctypes; the ABI stays 3
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dpsx.h")).read(), flags=re.S)
    assert re.search(r"\b" + NAME + r"\s*\(", hdr) and hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    assert "#define DPSX_ABI_VERSION 3" in hdr and _lib.lib().dpsx_abi_version() == _lib.ABI_VERSION == 3
    cg = list(_lib.SIGNATURES["dpsx_cg_step_f32"][1])        # op, x0_hat, sample, y, y_n, rho, iters, coefs, x_next, ...
    assert _lib.SIGNATURES[NAME] == (ctypes.c_int, cg[:7] + [ctypes.c_float] + cg[8:])


# ------------------------------------------------------------------ 2. parameter errors
def test_parameter_errors():
    for bad in (-1, 65, 2.5, "5", True, None):
        with pytest.raises(ValueError, match="iters"):
            _method(iters=bad)
    assert _method(iters=0).iters == 0 and _method(iters=64).iters == 64
    for bad in ("ddpm", "", None, 1):
        with pytest.raises(ValueError, match="weighting"):
            _method(weighting=bad)
    assert _method(weighting="paper").weighting == "paper"
    for bad in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="weight"):
            _method(weight=bad)
    assert _method(weight=2).weight == 2.0 and _method(weight=-0.5).weight == -0.5
    with pytest.raises(NotImplementedError, match="linear"):
        _method("phase_retrieval")
    with pytest.raises(NotImplementedError, match="Gaussian measurement noise"):
        _method(noise=("poisson", dict(rate=1.0)))
    assert _method(noise=("clean", {})).noise_sigma == 0.0
    assert _method(noise=("gaussian", dict(sigma=0.01))).noise_sigma == 0.01      # no floor
    with pytest.raises(ValueError, match="sigma"):
        _method(noise=("gaussian", dict(sigma=-0.1)))


# ------------------------------------------------------------------ 3. host scalars
@pytest.mark.parametrize("name,eta", [("ddpm", None), ("ddim", 0.0), ("ddim", 0.5)])
def test_host_scalars(name, eta):
    """rho_t and gain_t are the float64 formulas of the restatement, each rounded to fp32 once"""
    smp = _sampler(name, eta=eta)
    tb = pgdm_ref.tables(smp.betas)
    n = smp.num_timesteps
    assert n == 20
    for idx in (0, n // 2, n - 1):
        rec = pgdm_ref.record(tb, idx, eta)
        ck = smp.sample_coefs(idx)
        # the restatement's record is the sampler's own (fp32-rounded by different routes: within a few ulps)
        for k, v in (("a", ck.a), ("b", ck.b), ("c1", ck.c1), ("c2", ck.c2)):
            assert abs(rec[k] - v) <= 4e-7 * max(abs(v), 1e-3), (idx, k, rec[k], v)
        assert bool(ck.add_noise & 2) == rec["ddim"]
        for weighting in ("score", "paper"):
            for sigma, weight in ((0.05, 1.0), (0.5, 0.3)):
                cm = _method(noise=("gaussian", dict(sigma=sigma)), weighting=weighting, weight=weight)
                rho64, gain64 = pgdm_ref.scalars(tb, idx, rec, sigma, weighting, weight)
                rho, gain = smp.pgdm_scalars(idx, cm)
                assert rho == float(np.float32(rho64)) and gain == float(np.float32(gain64)), (idx, weighting, sigma)
                assert rho > 0 and np.isfinite(gain)
            clean = _method(noise=("clean", {}), weighting=weighting)
            assert smp.pgdm_scalars(idx, clean)[0] == 0.0
    # the formulas themselves, spelled out once at the middle step
    idx = n // 2
    rec = pgdm_ref.record(tb, idx, eta)
    abar, abar_prev = tb["abar"][idx], tb["abar_prev"][idx]
    kappa = rec["c1"] - rec["c2"] / rec["b"] if eta is not None else rec["c1"]
    assert pgdm_ref.scalars(tb, idx, rec, 0.5, "score", 2.0) == (0.25 / (1.0 - abar), 2.0 * kappa * rec["a"] * rec["b"])
    assert np.isclose(pgdm_ref.scalars(tb, idx, rec, 0.5, "paper")[1], np.sqrt(abar_prev) * np.sqrt(abar) * rec["b"],
                      rtol=1e-14)
    if eta == 0.0:          # DDIM, eta = 0: kappa = sqrt(abar_s) - sqrt(1 - abar_s) / b
        assert np.isclose(kappa, np.sqrt(abar_prev) - np.sqrt(1 - abar_prev) / rec["b"], rtol=1e-14)


# ------------------------------------------------------------------ 4. the push-through identity
def _dense_ops(oracle):
    rng = np.random.RandomState(5)
    mask = (rng.rand(1, 1, 8, 8) < 0.5).astype(np.float32)
    return [("blur3", oracle.make_operator("gaussian_blur", kernel_size=3, intensity=1.0)),
            ("sr2", oracle.make_operator("super_resolution", in_shape=(1, 1, 8, 8), scale_factor=2)),
            ("mask", oracle.make_operator("inpainting", mask=mask))]


@pytest.mark.parametrize("sigma_y", [0.05, 0.5])
def test_push_through_identity(oracle, sigma_y):
    rng = np.random.RandomState(11)
    tb = pgdm_ref.tables(np.linspace(1e-4, 0.02, 1000))
    for tag, op in _dense_ops(oracle):
        A = pgdm_ref.dense_matrix(op, (1, 8, 8))
        assert A.shape[1] == 64 and A.shape[0] == op.forward(np.zeros((1, 1, 8, 8), np.float32)).size
        # A^T is the oracle's adjoint (the CG restatements rely on it)
        u = rng.randn(1, *op.forward(np.zeros((1, 1, 8, 8), np.float32)).shape[1:]).astype(np.float32)
        assert np.allclose(A.T @ u.reshape(-1).astype(np.float64), op.adjoint(u, (8, 8)).reshape(-1), rtol=0, atol=1e-5)
        r = rng.randn(A.shape[0])
        for idx in (50, 500, 999):
            r2 = 1.0 - tb["abar"][idx]
            rho = sigma_y ** 2 / r2
            lhs, rhs = pgdm_ref.pinv_form(A, r, r2, sigma_y), pgdm_ref.normal_form(A, r, rho)
            rel = np.linalg.norm(lhs - rhs) / np.linalg.norm(rhs)
            assert rel <= 1e-10, (tag, idx, rel)
            cg = pgdm_ref.cg_dense(A, r, rho, 64)
            rel = np.linalg.norm(cg - rhs) / np.linalg.norm(rhs)
            assert rel <= 1e-6, (tag, idx, rel)


# ------------------------------------------------------------------ 5. the definition on the analytic model
def test_definition_on_the_analytic_model():
    """"score" converges to the exact posterior at first order in the step count; "paper" collapses onto y"""
    err = {n: pgdm_ref.analytic_error(n, "score")[0] for n in (20, 50, 100, 1000)}
    paper, paper_to_y = pgdm_ref.analytic_error(1000, "paper")
    print("score:", err, "paper:", paper, "paper to y:", paper_to_y)
    assert err[50] <= 0.5 * err[20]
    assert err[100] <= 0.6 * err[50]
    assert err[1000] <= 5e-3
    assert paper >= 10 * err[1000]
    assert paper_to_y <= 0.1 * paper          # ... onto y


# ------------------------------------------------------------------ 6. refusals
def test_entry_refuses_without_an_operator():
    """an operator handle needs the device, so the host alone reaches the first refusal only (the rest: test_pgdm_gpu's
    test_argument_errors_touch_nothing); the pointers here must never be dereferenced"""
    from dps_ttc_amd import _lib
    lib, q = _lib.lib(), c_void_p(0x1000)
    for n in (4, 0, 65536):
        assert lib.dpsx_cg_pullback_f32(None, q, q, q, 1, 0.25, 5, 0.5, q, q, q, n, 3, 8, 8, q, 1 << 30, None) == _lib.EINVAL


def test_samplers_refuse_before_the_model_is_called():
    """CPU tensors and a model that raises when called: every refusal must come first, with its reason in the message"""
    def model(*a, **kw):
        raise AssertionError("the model was called")

    x, y = torch.zeros(4, 3, 64, 64), torch.zeros(1, 3, 64, 64)

    def loop(smp, fn, x=x, **kw):
        return smp.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=fn, record=False, save_root=None,
                                 **kw)

    cm = _method()
    grouped = _sampler()
    grouped.particle_groups = 2
    with pytest.raises(NotImplementedError, match="particle_groups = 2"):
        loop(grouped, cm.conditioning)
    second = _sampler("ddim", eta=0.0)
    second.solver_order = 2
    with pytest.raises(NotImplementedError, match="solver_order = 2.*pgdm.*its own weight"):
        loop(second, cm.conditioning)
    span = _sampler()
    span.guidance_gain = "span"
    with pytest.raises(NotImplementedError, match="guidance_gain = 'span'.*pgdm.*its own weight"):
        loop(span, cm.conditioning)
    with pytest.raises(NotImplementedError, match="pgdm.*smc_ddpm"):
        loop(_sampler("smc_ddpm"), cm.conditioning)
    with pytest.raises(NotImplementedError, match="pgdm.*project=True"):
        loop(_sampler(), cm.conditioning, project=True)
    with pytest.raises(NotImplementedError, match="pgdm.*fixed-variance"):                # no HIP S1: the model's variance
        loop(_sampler(var="fixed_small"), cm.conditioning)
    with pytest.raises(NotImplementedError, match="pgdm.*mask"):
        loop(_sampler(), _method("inpainting").conditioning)
    # accepted: the loop then asks for the device
    inp = functools.partial(_method("inpainting").conditioning, mask=torch.ones(1, 1, 64, 64))
    for smp, fn in ((_sampler(), cm.conditioning), (_sampler("ddim", eta=0.0), cm.conditioning),
                    (_sampler("ddim", "logsnr10", eta=1.0), cm.conditioning), (_sampler("ttc_ddim", eta=0.5), cm.conditioning),
                    (_sampler(), inp), (_sampler(), _method(noise=("clean", {})).conditioning)):
        with pytest.raises(RuntimeError, match="MI355X"):
            loop(smp, fn)


def test_shipped_yamls():
    from dps_ttc_amd.gaussian_diffusion import DDIM, create_sampler
    load = lambda f: yaml.load(open(os.path.join(ROOT, "configs", f)), Loader=yaml.FullLoader)
    for f, op in (("gaussian_deblur_config_pgdm.yaml", "gaussian_blur"), ("super_resolution_config_pgdm.yaml", "super_resolution")):
        cfg = load(f)
        assert cfg["conditioning"] == {"method": "pgdm", "params": {"iters": 5, "weighting": "score", "weight": 1.0}}
        assert cfg["measurement"]["operator"]["name"] == op and cfg["measurement"]["noise"]["name"] == "gaussian"
        plain = load(f.replace("_pgdm", ""))
        assert {k: v for k, v in cfg.items() if k != "conditioning"} == {k: v for k, v in plain.items() if k != "conditioning"}
    diff = load("diffusion_config_pgdm.yaml")
    assert diff["sampler"] == "ddim" and diff["timestep_respacing"] == "logsnr50" and diff["eta"] == 1.0
    smp = create_sampler(**diff)
    assert isinstance(smp, DDIM) and 45 <= smp.num_timesteps <= 50 and smp.eta == 1.0 and smp.hip_posterior     # (nearest base steps: some coincide)


def test_driver_flags(monkeypatch):
    import sys
    sys.path.insert(0, ROOT)
    drv = importlib.import_module("sample_condition_batched_ttc")
    none = drv.parse_args([])
    assert (none.pgdm_iters, none.pgdm_weighting, none.pgdm_weight) == (None, None, None)
    assert drv.check_pgdm(none, "ps") is None and drv.check_pgdm(none, "pgdm") is None
    args = drv.parse_args(["--pgdm_iters", "3", "--pgdm_weighting", "paper", "--pgdm_weight", "0.5"])
    assert (args.pgdm_iters, args.pgdm_weighting, args.pgdm_weight) == (3, "paper", 0.5)
    assert drv.check_pgdm(args, "pgdm") is None
    for flags in (["--pgdm_iters", "3"], ["--pgdm_weighting", "paper"], ["--pgdm_weight", "0.5"]):
        with pytest.raises(SystemExit) as e:
            drv.check_pgdm(drv.parse_args(flags), "ps")
        assert flags[0] in str(e.value) and "method pgdm" in str(e.value) and "\n" not in str(e.value)
    for flags, what in ((["--pgdm_iters", "65"], "\\[0, 64\\]"), (["--pgdm_iters", "-1"], "\\[0, 64\\]"),
                        (["--pgdm_weight", "nan"], "finite"), (["--pgdm_weight", "inf"], "finite")):
        with pytest.raises(SystemExit, match=what):
            drv.check_pgdm(drv.parse_args(flags), "pgdm")
    with pytest.raises(SystemExit):                                       # argparse's own choices
        drv.parse_args(["--pgdm_weighting", "other"])

    # main(): the refusals come before anything touches the GPU; the shipped configs pass the checks
    def no_gpu(*a, **kw):
        raise AssertionError("the check touched the GPU")
    for fn in ("set_device", "device_count"):
        monkeypatch.setattr(torch.cuda, fn, no_gpu)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cfg = lambda f: os.path.join(ROOT, "configs", f)
    pg = ["--diffusion_config", cfg("diffusion_config_pgdm.yaml"), "--task_config", cfg("gaussian_deblur_config_pgdm.yaml")]
    with pytest.raises(SystemExit, match="method pgdm"):
        drv.main(["--diffusion_config", cfg("diffusion_config_pgdm.yaml"), "--task_config", cfg("gaussian_deblur_config.yaml"),
                  "--pgdm_iters", "3"])
    with pytest.raises(SystemExit, match="solver_order 2.*method pgdm"):
        drv.main(pg + ["--solver_order", "2"])
    with pytest.raises(SystemExit, match="guidance_gain span.*method pgdm"):
        drv.main(pg + ["--guidance_gain", "span"])
    with pytest.raises(SystemExit, match="pgdm.*particle_groups"):
        drv.main(pg + ["--particle_groups", "2"])
    with pytest.raises(SystemExit, match="pgdm.*smc_ddpm"):
        drv.check_pgdm(none, "pgdm", "smc_ddpm")
    assert drv.check_pgdm(none, "pgdm", "ddim") is None and drv.check_pgdm(none, "ps", "smc_ddpm") is None
    with pytest.raises(SystemExit, match="no CPU fallback"):             # accepted: the run itself then needs the device
        drv.main(pg + ["--pgdm_iters", "3", "--pgdm_weighting", "paper"])
