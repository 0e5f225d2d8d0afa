"""GPU suite (-m gpu): the separable blur kernels' regular-geometry loader and fused adjoint epilogue.

What these guard: every halo unit of the regular loader is one 16-byte load whose mirror reversal happens on the loaded
registers; the halo unit -> (row, column) map is evaluated per deal with a multiply-shift division; K1's S1 runs on packed
pairs; the fused adjoint epilogue is compiled with and without the extra cotangent.  None of that may move a result.

Gates are the suite's own (test_hip_parity.py): rel-L2 <= 1e-5 against the oracle on operator outputs, adjoints, norms and
gradients, <= 1e-6 on `sample` / x_{t-1}, bit-exact x0_hat and clamp gate.

Shapes: 192 x 192 is the smallest regular geometry with corner, edge and interior tiles; 128 x 192 has border tiles only
and is not square.  One sigma per radius bucket RR = 4 .. 32 (the filter reaches 4 sigma; 32 < 128, the shorter side).
The Gaussian itself takes the symmetric adjoint; the same taps skewed along both axes (still rank 1) take the general
one with its fold terms.  160 x 160 (ragged tiles) and 64 x 128 (one tile on an axis) fall back to the general loader.
"""
import numpy as np
import pytest
import torch

from standin import rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"
REGULAR = [(192, 192), (128, 192)]
FALLBACK = [(160, 160), (64, 128)]
# (kernel size, sigma): reach = 4 sigma, RR = 4, 8, ..., 32
BUCKETS = [(61, 1.0), (61, 2.0), (61, 3.0), (61, 4.0), (61, 5.0), (61, 6.0), (61, 7.0), (65, 8.0)]


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def _kernel2d(oracle, ks, sigma, skew):
    k2 = oracle.tables.gaussian_kernel2d(ks, sigma)
    if skew:
        k2 = k2 * (1.0 + 0.3 * np.linspace(-1, 1, ks))[None, :] * (1.0 - 0.2 * np.linspace(-1, 1, ks))[:, None]
    return k2.astype(np.float32)


def _handle(K, k2, ks, sigma):
    h = K.OpHandle.blur(k2, DEV)
    assert h.kind == K._lib.KIND_SEP
    return h


def _coefs(K, oracle, t):
    c = oracle.tables.step_coefs(oracle.tables.schedule(1000), t)
    return c, K.make_coefs(c["a"], c["b"], c["c1"], c["c2"], c["min_log"], c["max_log"], c["add_noise"])


def _step_inputs(oracle, orc, c, n, hw, seed, extra):
    rng = np.random.RandomState(seed)
    shape = (n, 3) + tuple(hw)
    x_prev = rng.randn(*shape).astype(np.float32)
    target = 1.4 * np.tanh(rng.randn(*shape))          # about a third of the pixels leave [-1, 1]: both sides of the gate
    eps = ((c["a"] * x_prev - target) / c["b"]).astype(np.float32)
    mo = np.concatenate([eps, rng.uniform(-1, 1, eps.shape).astype(np.float32)], axis=1)
    noise = rng.randn(*shape).astype(np.float32)
    y = orc.forward(rng.uniform(-1, 1, (1, 3) + tuple(hw)).astype(np.float32))
    y = (y + 0.05 * rng.randn(*y.shape)).astype(np.float32)
    g_unet = (1e-2 * rng.randn(*shape)).astype(np.float32)
    g_extra = (0.05 * rng.randn(*shape)).astype(np.float32) if extra else None
    return x_prev, mo, noise, y, g_unet, g_extra


def _fused_step(K, oracle, handle, k2, hw, t, extra, seed, n=3):
    """the three launches against oracle.dps_step; t = 0 is the add_noise = 0 record, any other t add_noise = 1"""
    c, ck = _coefs(K, oracle, t)
    assert c["add_noise"] == (0 if t == 0 else 1)
    orc = oracle.make_operator("motion_blur", kernel=k2)          # the oracle's blur with the taps as given
    x_prev, mo, noise, y, g_unet, g_extra = _step_inputs(oracle, orc, c, n, hw, seed, extra)
    ref = oracle.dps_step(orc, x_prev, mo, noise, y, c, scale=0.7, power=1, g_unet_fn=lambda g: g_unet, g_x0_extra=g_extra)
    buf = K.StepBuffers(handle, n, 3, hw[0], hw[1], DEV)
    K.step_fwd(handle, buf, dev(x_prev), dev(mo), dev(noise), dev(y), ck)
    K.step_bwd(handle, buf, dev(y), 0.7, 1, ck, g_x0_extra=None if g_extra is None else dev(g_extra))
    x_next = K.step_update(buf, dev(g_unet), ck)
    np.testing.assert_array_equal(host(buf.x0_hat), ref["x0_hat"])
    np.testing.assert_array_equal(buf.inside.cpu().numpy(), ref["inside"])
    assert rel_l2(host(buf.sample), ref["sample"]) < 1e-6
    assert rel_l2(host(buf.norm), ref["norm"]) < TOL
    assert rel_l2(host(buf.g_model_out), ref["g_model_out"]) < TOL
    assert np.all(host(buf.g_model_out)[:, 3:] == 0)
    assert rel_l2(host(x_next), ref["x_next"]) < 1e-6


@pytest.mark.parametrize("skew", [False, True], ids=["sym", "skew"])
@pytest.mark.parametrize("ks,sigma", BUCKETS)
@pytest.mark.parametrize("hw", REGULAR, ids=lambda s: "%dx%d" % s)
def test_regular_loader_every_bucket(K, oracle, hw, ks, sigma, skew):
    """plain forward / adjoint and the fused step (one with, one without the extra cotangent; one per add_noise mode)"""
    rng = np.random.RandomState(int(10 * sigma) + hw[0] + skew)
    k2 = _kernel2d(oracle, ks, sigma, skew)
    h = _handle(K, k2, ks, sigma)
    x = rng.randn(3, 3, *hw).astype(np.float32)
    assert rel_l2(host(h.forward(dev(x))), oracle.blur_fwd(x, k2)) < TOL
    assert rel_l2(host(h.adjoint(dev(x), in_hw=hw)), oracle.blur_adj(x, k2)) < TOL
    _fused_step(K, oracle, h, k2, hw, 500, extra=False, seed=hw[0] + ks)
    _fused_step(K, oracle, h, k2, hw, 0, extra=True, seed=hw[1] + ks + 1)


@pytest.mark.parametrize("t,extra", [(500, True), (0, False)])
@pytest.mark.parametrize("ks,sigma", BUCKETS[:3])
@pytest.mark.parametrize("hw", REGULAR, ids=lambda s: "%dx%d" % s)
def test_epilogue_forms_and_noise_modes(K, oracle, hw, ks, sigma, t, extra):
    """the other two (add_noise, extra cotangent) pairs on the buckets RR = 4, 8, 12: with the test above, all four"""
    k2 = _kernel2d(oracle, ks, sigma, False)
    _fused_step(K, oracle, _handle(K, k2, ks, sigma), k2, hw, t, extra, seed=hw[0] + t + ks)


@pytest.mark.parametrize("skew", [False, True], ids=["sym", "skew"])
@pytest.mark.parametrize("t", [500, 0])
@pytest.mark.parametrize("hw", REGULAR + FALLBACK, ids=lambda s: "%dx%d" % s)
def test_specialised_epilogue_equals_general(K, oracle, hw, t, skew):
    """g_x0_extra = zeros (the epilogue that loads and adds the cotangent) against g_x0_extra = None (the one compiled
    without it), same inputs: bit for bit, zeros' signs included.  One particle's residual is set to the smallest negative
    denormal, so that coef * A^T r underflows to -0.0 there: the case in which leaving out `+ 0.0` would show (with the add
    the gradient is -b * (+0.0), without it -b * (-0.0))."""
    c, ck = _coefs(K, oracle, t)
    k2 = _kernel2d(oracle, 61, 3.0, skew)
    h = _handle(K, k2, 61, 3.0)
    orc = oracle.make_operator("motion_blur", kernel=k2)
    x_prev, mo, noise, y, _, _ = _step_inputs(oracle, orc, c, 3, hw, hw[0] + t, False)
    out = []
    for g_extra in (None, torch.zeros(3, 3, *hw, device=DEV)):
        buf = K.StepBuffers(h, 3, 3, hw[0], hw[1], DEV)
        K.step_fwd(h, buf, dev(x_prev), dev(mo), dev(noise), dev(y), ck)
        # (a blur operator's step scratch is the fp32 residual, [N, C, H, W]: dpsx_step_resid_bytes)
        buf.resid[:4 * 9 * hw[0] * hw[1]].view(torch.float32).view(3, 3, *hw)[1].fill_(-1e-45)
        K.step_bwd(h, buf, dev(y), 0.7, 1, ck, g_x0_extra=g_extra)
        torch.cuda.synchronize()
        out.append(buf.g_model_out.clone())
    a, b = (o.view(torch.int32) for o in out)
    assert torch.equal(a, b)
    assert bool((out[0][0, :3] != 0).any())          # the launch did write a gradient


@pytest.mark.parametrize("hw", FALLBACK, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("ks,sigma", BUCKETS[:3])
def test_general_loader_shapes_still_agree(K, oracle, hw, ks, sigma):
    """ragged tiles / a single-tile axis: not the new code, the dispatch around it"""
    rng = np.random.RandomState(ks + hw[1])
    k2 = _kernel2d(oracle, ks, sigma, False)
    h = _handle(K, k2, ks, sigma)
    x = rng.randn(2, 3, *hw).astype(np.float32)
    assert rel_l2(host(h.forward(dev(x))), oracle.blur_fwd(x, k2)) < TOL
    assert rel_l2(host(h.adjoint(dev(x), in_hw=hw)), oracle.blur_adj(x, k2)) < TOL
    _fused_step(K, oracle, h, k2, hw, 500, extra=True, seed=hw[0] + ks)
    _fused_step(K, oracle, h, k2, hw, 0, extra=False, seed=hw[1] + ks)
