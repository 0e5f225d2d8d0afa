"""CPU suite of the `cg` conditioning method: registry, rho, kappa, refusals, and the restatement tests/cg_ref.py (the
reference of the GPU suite) against a dense float64 solve, the closed forms and the monotone objective."""
import numpy as np
import pytest
import torch

import cg_ref
from standin import rel_l2, synthetic_motion_kernel

DEV = "cuda:0"          # operators build their device handle lazily: constructing them needs no GPU


def _method(name="gaussian_blur", **params):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    kw = {"gaussian_blur": dict(kernel_size=61, intensity=3.0), "phase_retrieval": dict(oversample=2.0),
          "noise": {}, "inpainting": {}}[name]
    return get_conditioning_method("cg", get_operator(name, device=DEV, **kw), get_noise("gaussian", sigma=0.05), **params)


def test_registry_defaults_and_rho():
    from dps_ttc_amd import condition_methods as CM
    from dps_ttc_amd.condition_methods import ConditioningMethod
    # a method the reference does not have: found by name like the others, kept out of the table that mirrors the reference's
    assert sorted(CM.__EXTENSION_METHOD__) == ["cg"] and "cg" not in CM.__CONDITIONING_METHOD__
    with pytest.raises(NameError, match="already registered"):
        CM.register_conditioning_method(name="cg", extension=True)(object)
    with pytest.raises(NameError, match="already registered"):
        CM.register_conditioning_method(name="ps", extension=True)(object)
    cm = _method()
    assert isinstance(cm, ConditioningMethod) and cm.returns_gradient is False
    assert cm.rho_scale == 1.0 and cm.iters == 5 and cm.fused_spec() is None and cm.fused_spec(beta_scale=0.1, t=0.5) is None
    assert cm.noise_sigma == 0.05
    for b in (0.01, 1.0, 37.5):
        assert cm.rho(b) == 1.0 * 0.05 ** 2 / b ** 2
    cm = _method(rho_scale=2.5, iters=3)
    assert cm.iters == 3 and cm.rho(2.0) == 2.5 * 0.05 ** 2 / 4.0
    from dps_ttc_amd.measurements import get_noise, get_operator
    from dps_ttc_amd.condition_methods import get_conditioning_method
    quiet = get_conditioning_method("cg", get_operator("noise", device=DEV), get_noise("gaussian", sigma=0.01))
    assert quiet.noise_sigma == 0.05                       # the floor of ps_anneal
    for bad in (dict(iters=-1), dict(iters=65), dict(rho_scale=-1.0), dict(rho_scale=float("nan"))):
        with pytest.raises(ValueError):
            _method(**bad)


@pytest.mark.parametrize("t", [0, 500, 999])
def test_kappa_is_the_slope_of_the_sample(oracle, t):
    """sample is affine in x0_hat with slope kappa: DDPM c1, DDIM (eps re-derived from x0_hat) c1 - c2 / b"""
    from dps_ttc_amd import kernels
    sched = oracle.tables.schedule(1000)
    c = oracle.tables.step_coefs(sched, t)
    ck = kernels.make_coefs(c["a"], c["b"], c["c1"], c["c2"], c["min_log"], c["max_log"], c["add_noise"])
    assert kernels.cg_kappa(ck) == float(np.float32(c["c1"])) == float(cg_ref.kappa(c))
    x, x0 = 0.37, np.array([-0.8, 0.1, 0.9])
    mean = lambda v: float(ck.c1) * v + float(ck.c2) * x                                       # posterior mean
    assert np.allclose((mean(x0 + 1.0) - mean(x0)), kernels.cg_kappa(ck), rtol=1e-12)
    for eta in (0.0, 0.5, 1.0):
        cd = oracle.tables.ddim_step_coefs(sched, t, eta)
        kd = kernels.make_ddim_coefs(sched["sqrt_recip_alphas_cumprod"][t], sched["sqrt_recipm1_alphas_cumprod"][t],
                                     sched["alphas_cumprod"][t], sched["alphas_cumprod_prev"][t], eta, t != 0)
        k = kernels.cg_kappa(kd)
        assert k == float(np.float32(kd.c1) - np.float32(kd.c2) / np.float32(kd.b)) == float(cg_ref.kappa(cd))
        ddim = lambda v: v * float(kd.c1) + float(kd.c2) * ((float(kd.a) * x - v) / float(kd.b))   # DDIM mean
        assert np.allclose(ddim(x0 + 1.0) - ddim(x0), k, rtol=1e-6, atol=1e-7)
        if t == 0:
            assert k == 1.0
    if t == 0:
        assert kernels.cg_kappa(ck) == 1.0


def test_refusals():
    with pytest.raises(NotImplementedError, match="linear"):
        _method("phase_retrieval")
    cm = _method()
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(ValueError, match="loop supplies"):
        cm.conditioning(x_t=x, x_0_hat=x, measurement=x)
    with pytest.raises(ValueError, match="loop supplies"):
        cm.conditioning(x, x, x, mask=None)


def test_abi_names_are_bound():
    from dps_ttc_amd import _lib
    lib = _lib.lib()
    for name in ("dpsx_cg_workspace_bytes", "dpsx_cg_step_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dpsx_cg_workspace_bytes(None, 1, 3, 8, 8) == _lib.EINVAL          # no operator: refused on the host


# ------------------------------------------------------------------ the restatement
def _ops16(oracle):
    mask = (np.random.RandomState(3).rand(1, 1, 16, 16) < 0.6).astype(np.float32)
    return {"gauss": oracle.make_operator("gaussian_blur", kernel_size=9, intensity=1.0),
            "mask": oracle.make_operator("inpainting", mask=mask)}


def _problem(op, shape, seed=0):
    rng = np.random.RandomState(seed)
    xs = rng.uniform(-1, 1, shape).astype(np.float32)
    ax = op.forward(xs)
    y = (ax + 0.05 * rng.randn(*ax.shape)).astype(np.float32)
    x0 = np.clip(xs + 0.3 * rng.randn(*shape), -1, 1).astype(np.float32)
    return x0, y


@pytest.mark.parametrize("name", ["gauss", "mask"])
def test_restatement_against_a_dense_solve(oracle, name):
    """1 x 16 x 16, rho = 0.25: the matrix of A from the oracle applied to the basis, (A^T A + rho I) d = A^T (y - A x0)
    by numpy.linalg.solve in float64; 60 iterations of the restatement agree to 1e-5 rel-L2 (observed: gauss 1.1e-7,
    mask 2.5e-8 -- the oracle rounds every operator application to fp32)."""
    op, rho = _ops16(oracle)[name], 0.25
    basis = np.eye(256, dtype=np.float32).reshape(256, 1, 16, 16)
    a = op.forward(basis).reshape(256, -1).T.astype(np.float64)            # column j = A e_j
    x0, y = _problem(op, (1, 1, 16, 16))
    rhs = a.T @ (y.reshape(-1).astype(np.float64) - a @ x0.reshape(-1).astype(np.float64))
    want = np.linalg.solve(a.T @ a + rho * np.eye(256), rhs).reshape(1, 1, 16, 16)
    got, dist = cg_ref.solve(op, x0, y, rho, 60)
    err = rel_l2(got, want)
    print(f"{name}: CG(60) vs dense solve rel-L2 {err:.3e}")
    assert err <= 1e-5
    assert np.allclose(dist, np.linalg.norm(y.reshape(-1).astype(np.float64) - a @ x0.reshape(-1)), rtol=1e-6)
    assert np.array_equal(cg_ref.solve(op, x0, y, rho, 0)[0], np.zeros_like(want))


def _ops64(oracle, golden):
    g = golden("operators")
    return {"gauss": oracle.make_operator("gaussian_blur", kernel_size=61, intensity=3.0),
            "motion": oracle.make_operator("motion_blur", kernel=g["motion.kernel"]),
            "sr4": oracle.make_operator("super_resolution", in_shape=(1, 3, 64, 64), scale_factor=4),
            "mask": oracle.make_operator("inpainting", mask=g["inpaint.mask"]),
            "ident": oracle.make_operator("noise")}


@pytest.mark.parametrize("name", ["mask", "ident"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_closed_form_of_projections(oracle, golden, name, dtype):
    """A = diag(m), m in {0, 1} (the identity: m = 1): A^T A = A, so CG converges in one iteration to
    d = m (y - m x0) / (1 + rho), and further iterations leave it there"""
    op = _ops64(oracle, golden)[name]
    x0, y = _problem(op, (3, 3, 64, 64), seed=1)
    m = op.forward(np.ones((1, 3, 64, 64), dtype=np.float32)).astype(np.float64)
    for rho in (0.25, 4.0):
        want = m * (y.astype(np.float64) - m * x0) / (1.0 + rho)
        for iters in (1, 5):
            err = rel_l2(cg_ref.solve(op, x0, y, rho, iters, dtype=dtype)[0], want)
            assert err <= 1e-6, (rho, iters, err)


@pytest.mark.parametrize("name", ["gauss", "motion", "sr4", "mask", "ident"])
def test_objective_never_increases(oracle, golden, name):
    op = _ops64(oracle, golden)[name]
    x0, y = _problem(op, (3, 3, 64, 64), seed=2)
    for rho in (0.01, 0.25, 4.0):
        for dtype in (np.float64, np.float32):
            j = [cg_ref.objective(op, x0, y, cg_ref.solve(op, x0, y, rho, k, dtype=dtype)[0], rho) for k in range(6)]
            for a, b in zip(j, j[1:]):
                assert (b <= a * (1 + 1e-6)).all(), (rho, dtype, j)
            assert (j[1] < j[0]).all()


def test_fp32_and_float64_vectors_agree(oracle, golden):
    """the restatement's own precision on the GPU suite's parity cases: fp32 vectors against float64 ones"""
    for name, op in _ops64(oracle, golden).items():
        x0, y = _problem(op, (3, 3, 64, 64), seed=3)
        for rho in (0.25, 4.0):
            for iters in (1, 5):
                d64, dist64 = cg_ref.solve(op, x0, y, rho, iters)
                d32, dist32 = cg_ref.solve(op, x0, y, rho, iters, dtype=np.float32)
                assert rel_l2(d32, d64) <= 1e-6, (name, rho, iters)
                assert np.allclose(dist32, dist64, rtol=1e-6)
