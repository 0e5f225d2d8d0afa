"""GPU suite: degenerate VALUES through the fused step -- a particle whose residual is exactly zero, a spectrum too dim for
the transcendental unit, a NaN or an infinity in one particle.

Layout shared by every test: N particles with one measurement per particle (y [N, ...]), particle P = 1 is the special one.
The same inputs run "clean" and "special" in fresh StepBuffers.  Comparators: the CPU oracle with the suite's gates (TOL
= 1e-5 rel-L2, 1e-6 on sample / x_{t-1}, bit-exact x0_hat and clamp gate), or torch.equal against the clean run for the
particles that must not notice.

The zero-norm rule (torch: the gradient of a norm at zero is zero) is `nv == 0 ? 0 : -gn / nv`; every fused backward half
carries its own copy of it next to a `|z| == 0` rule, and one 0 / 0 in any of them would put NaN into x_{t-1} of a particle
that already matches its measurement.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from standin import rel_l2, synthetic_motion_kernel
from test_hip_parity import DEV, TOL, K, coefs_of, dev, host, make_oracle_op, make_product_op  # noqa: F401 (K: fixture)

pytestmark = pytest.mark.gpu
P = 1                       # the special particle
FIELDS = ("sample", "inside", "x0_hat", "norm", "g_model_out", "x_next")


def _case(K, oracle, name, hw, n, t=500, seed=0):
    """clean inputs of one fused step, one measurement per particle"""
    rng = np.random.RandomState(seed + hw)
    c, ck = coefs_of(K, oracle, t)
    kernel = synthetic_motion_kernel(61, 4)
    mask = (np.random.RandomState(7).rand(1, 1, hw, hw) < 0.5).astype(np.float32)
    op, fkw = make_product_op(name, hw=hw, kernel=kernel, mask=mask)
    orc = make_oracle_op(oracle, name, hw=hw, kernel=kernel, mask=mask)
    x = rng.randn(n, 3, hw, hw).astype(np.float32)
    eps = ((c["a"] * x - 1.4 * np.tanh(rng.randn(n, 3, hw, hw))) / c["b"]).astype(np.float32)
    mo = np.concatenate([eps, rng.uniform(-1, 1, eps.shape).astype(np.float32)], axis=1)
    noise = rng.randn(n, 3, hw, hw).astype(np.float32)
    y = orc.forward(rng.uniform(-1, 1, (1, 3, hw, hw)).astype(np.float32))
    y = (np.repeat(y, n, axis=0) + 0.05 * rng.randn(n, *y.shape[1:])).astype(np.float32)
    g_unet = (1e-2 * rng.randn(n, 3, hw, hw)).astype(np.float32)
    g_extra = (0.05 * rng.randn(n, 3, hw, hw)).astype(np.float32)
    handle = op.hip_handle_for(fkw["mask"]) if name == "inpaint" else op.hip_handle(dev(x))
    return SimpleNamespace(name=name, hw=hw, n=n, c=c, ck=ck, op=op, fkw=fkw, orc=orc, handle=handle, x=x, mo=mo, noise=noise,
                           y=y, g_unet=g_unet, g_extra=g_extra)


def _hip(K, cs, x, mo, noise, y, scale, power, finalize=False, extra=None):
    """the three launches in fresh buffers -> the six tensors of FIELDS (device clones)"""
    buf = K.StepBuffers(cs.handle, cs.n, 3, cs.hw, cs.hw, DEV)
    yd = dev(y)
    K.step_fwd(cs.handle, buf, dev(x), dev(mo), dev(noise), yd, cs.ck, finalize_norm=finalize)
    K.step_bwd(cs.handle, buf, yd, scale, power, cs.ck, g_x0_extra=None if extra is None else dev(extra))
    x_next = K.step_update(buf, dev(cs.g_unet), cs.ck)
    torch.cuda.synchronize()
    return SimpleNamespace(sample=buf.sample.clone(), inside=buf.inside.clone(), x0_hat=buf.x0_hat.clone(),
                           norm=buf.norm.clone(), g_model_out=buf.g_model_out.clone(), x_next=x_next.clone())


def _others(n):
    return [q for q in range(n) if q != P]


def _assert_usual_gates(out, ref, rows):
    """the gates of test_hip_parity._fused_case on the particles `rows`"""
    np.testing.assert_array_equal(host(out.x0_hat)[rows], ref["x0_hat"][rows])
    np.testing.assert_array_equal(out.inside.cpu().numpy()[rows], ref["inside"][rows])
    assert rel_l2(host(out.sample)[rows], ref["sample"][rows]) < 1e-6
    assert rel_l2(host(out.norm)[rows], ref["norm"][rows]) < TOL
    assert rel_l2(host(out.g_model_out)[rows], ref["g_model_out"][rows]) < TOL
    assert rel_l2(host(out.x_next)[rows] - ref["sample"][rows], ref["x_next"][rows] - ref["sample"][rows]) < TOL
    assert rel_l2(host(out.x_next)[rows], ref["x_next"][rows]) < 1e-6


# ----------------------------------------------------------------- zero residual
@pytest.mark.parametrize("name,hw,n", [("denoise", 17, 4), ("inpaint", 64, 4), ("gauss", 64, 4), ("gauss", 46, 4), ("motion", 64, 4),
                                       ("sr4", 64, 4), ("phase", 32, 4), ("phase", 36, 4), ("phase", 256, 2)])
@pytest.mark.parametrize("power", [1, 2])
def test_zero_residual_particle(K, oracle, name, hw, n, power):
    """particle P matches its measurement exactly: norm 0, zero measurement gradient (not 0 / 0), finite x_{t-1}; with an
    extra cotangent only that term remains; the per-op autograd route agrees; the other particles pass the usual gates"""
    cs = _case(K, oracle, name, hw, n)
    x, mo, y = cs.x.copy(), cs.mo.copy(), cs.y.copy()
    if name in ("denoise", "inpaint"):       # x0_hat is bit-exact against the oracle's and mask * value is exact
        x0 = oracle.posterior_fwd(x, mo, cs.noise, cs.c)["x0_hat"]
        y[P] = cs.orc.forward(x0[P:P + 1])[0]
    else:                                    # x0_hat[P] == 0 and A(0) == 0 exactly
        x[P], mo[P, :3], y[P] = 0.0, 0.0, 0.0
    scale = 0.5
    ref = oracle.dps_step(cs.orc, x, mo, cs.noise, y, cs.c, scale=scale, power=power, g_unet_fn=lambda g: cs.g_unet)
    assert ref["norm"][P] == 0.0 and not ref["g_model_out"][P].any()
    rest = _others(n)
    for finalize in (False, True):
        out = _hip(K, cs, x, mo, cs.noise, y, scale, power, finalize=finalize)
        assert float(out.norm[P]) == 0.0
        assert not bool(out.g_model_out[P].any()), "measurement gradient at a zero norm"
        assert bool(torch.isfinite(out.x_next[P]).all())
        assert rel_l2(host(out.x_next[P]), ref["x_next"][P]) < 1e-6
        np.testing.assert_array_equal(host(out.x0_hat[P]), ref["x0_hat"][P])
        _assert_usual_gates(out, ref, rest)
    # extra cotangent: -b * gate * extra is all that is left for P (the oracle on that particle alone)
    one = slice(P, P + 1)
    ref_e = oracle.dps_step(cs.orc, x[one], mo[one], cs.noise[one], y[one], cs.c, scale=scale, power=power,
                            g_unet_fn=lambda g: cs.g_unet[one], g_x0_extra=cs.g_extra[one])
    for finalize in (False, True):
        out = _hip(K, cs, x, mo, cs.noise, y, scale, power, finalize=finalize, extra=cs.g_extra)
        assert float(out.norm[P]) == 0.0 and bool(out.g_model_out[P].any())
        assert rel_l2(host(out.g_model_out[P]), ref_e["g_model_out"][0]) < TOL
        assert rel_l2(host(out.x_next[P]), ref_e["x_next"][0]) < 1e-6
    # per-op route: operator under autograd, then the residual norm's VJP
    x0d = out.x0_hat.clone().requires_grad_()
    norm = K.ResidualNormFn.apply(cs.op.forward(x0d, **cs.fkw), dev(y))
    (g,) = torch.autograd.grad((norm ** 2 if power == 2 else norm).sum(), x0d)
    assert float(norm[P]) == 0.0 and not bool(g[P].any()) and bool(torch.isfinite(g).all())
    assert all(bool(g[q].any()) for q in rest)


# ----------------------------------------------------------------- dim spectrum (phase retrieval)
@pytest.mark.parametrize("side", [256, 32])          # 256: the hand-written spectral step; 32: the library transforms
def test_phase_dim_spectrum(K, oracle, side):
    """x0_hat[P] ~ 7e-22: every |X|^2 of its spectrum lies below FLT_MIN, where the raw reciprocal square root returns
    +inf (it takes fp32 denormals as zero).  The modulus there is zero to 1e-19, so norm[P] = ||y[P]||; everything stays
    finite; particle 0 does not notice.
    The measurement gradient of P itself is pinned as finite only, and the two routes differ there on purpose: the
    spectral step gives such bins the zero rule of |z| == 0 (a zero gradient for P), while the library-transform route
    and the oracle still divide by the tiny modulus (a gradient of magnitude ~0.07 along a direction that carries no
    information at |x0_hat| ~ 1e-21)."""
    n = 2
    cs = _case(K, oracle, "phase", side, n, seed=3)
    x, mo = cs.x.copy(), cs.mo.copy()
    x[P] = (1e-22 * np.random.RandomState(side).randn(3, side, side)).astype(np.float32)
    mo[P, :3] = 0.0
    ref = oracle.dps_step(cs.orc, x, mo, cs.noise, cs.y, cs.c, scale=0.5, power=1, g_unet_fn=lambda g: cs.g_unet)
    assert 0 < np.abs(ref["x0_hat"][P]).max() < 1e-20
    assert abs(ref["norm"][P] / np.linalg.norm(cs.y[P].astype(np.float64)) - 1.0) < 1e-6
    clean = _hip(K, cs, cs.x, cs.mo, cs.noise, cs.y, 0.5, 1)
    for finalize in (False, True):
        out = _hip(K, cs, x, mo, cs.noise, cs.y, 0.5, 1, finalize=finalize)
        got = float(out.norm[P])
        assert rel_l2(host(out.norm[P:P + 1]), ref["norm"][P:P + 1]) < TOL, f"norm[P] = {got!r}, oracle {float(ref['norm'][P])!r}"
        assert bool(torch.isfinite(out.g_model_out[P]).all()), "g_model_out[P] is not finite"
        assert bool(torch.isfinite(out.x_next[P]).all()), "x_next[P] is not finite"
        for f in FIELDS:
            assert torch.equal(getattr(out, f)[0], getattr(clean, f)[0]), f
        _assert_usual_gates(out, ref, [0])


# ----------------------------------------------------------------- non-finite values stay in their particle
CONFINED = [("gauss", 64, 4), ("motion", 64, 4), ("sr4", 64, 4), ("inpaint", 64, 4), ("denoise", 17, 4), ("phase", 32, 4),
            ("phase", 256, 2)]


@pytest.mark.parametrize("name,hw,n", CONFINED)
def test_nan_in_one_particle_stays_there(K, oracle, name, hw, n):
    """x_t[P, 1, h/2, w/2] = NaN: every output of every other particle is bit for bit the clean run's; norm[P] is NaN.
    (Which pixels of P turn NaN is not pinned: the kernels skip zero taps that torch's conv multiplies.)"""
    cs = _case(K, oracle, name, hw, n, seed=5)
    x = cs.x.copy()
    x[P, 1, hw // 2, hw // 2] = np.nan
    rest = _others(n)
    for power, finalize in ((1, False), (2, True)):
        clean = _hip(K, cs, cs.x, cs.mo, cs.noise, cs.y, 0.5, power, finalize=finalize)
        out = _hip(K, cs, x, cs.mo, cs.noise, cs.y, 0.5, power, finalize=finalize)
        for q in rest:
            for f in FIELDS:
                assert torch.equal(getattr(out, f)[q], getattr(clean, f)[q]), (f, q)
        assert bool(torch.isnan(out.norm[P]))
    # best-of-N over the same batch: NaN wins the select (torch.argmin), the other costs do not move
    xd, xc, yd = dev(x), dev(cs.x), dev(cs.y)
    costs, best, val = cs.handle.score_argmin(xd, yd)
    c_clean, b_clean, _ = cs.handle.score_argmin(xc, yd)
    assert int(best) == P == int(torch.argmin(costs)) and bool(torch.isnan(val).all()) and bool(torch.isnan(costs[P]))
    assert torch.equal(costs[rest], c_clean[rest]) and int(b_clean) == int(torch.argmin(c_clean))
    prev = dev(np.random.RandomState(1).rand(n).astype(np.float32) * 50)
    _, net = cs.handle.resample_cost(xd, yd, prev, "min")
    _, net_clean = cs.handle.resample_cost(xc, yd, prev, "min")
    assert torch.equal(net[rest], net_clean[rest]) and bool(torch.isnan(net[P]))
    # two images of K = 2 particles each (segments = 2): the select of the image without the NaN is untouched.  The N = 2
    # case gets two more particles for this (reversed copies, so that the second image's two candidates differ).
    mo, z = dev(cs.mo), dev(cs.noise)
    if n == 2:
        xd, xc, mo, z, yd = (torch.cat([t, t.flip(0)]).contiguous() for t in (xd, xc, mo, z, yd))
        xd[2:] = xc[2:]                     # the NaN stays in image 0 alone
    m = xd.shape[0]
    assert m == 4
    y2 = yd[[0, 2]].contiguous()
    others = [q for q in range(m) if q != P]
    _, _, c2, best2, val2 = cs.handle.search_step(xd, mo, z, y2, cs.ck, segments=2)
    _, _, c2c, best2c, val2c = cs.handle.search_step(xc, mo, z, y2, cs.ck, segments=2)
    assert int(best2[1]) == int(best2c[1]) == 2 + int(torch.argmin(c2c[2:])) and float(val2[1]) == float(val2c[1])
    assert float(c2c[2]) != float(c2c[3])
    assert int(best2[0]) == P and bool(torch.isnan(val2[0]))
    assert torch.equal(c2[others], c2c[others])


@pytest.mark.parametrize("name,hw,n", CONFINED)
def test_infinite_noise_touches_one_element(K, oracle, name, hw, n):
    """noise[P, 0, 0, 0] = +inf: the noise enters only the sample, so norm and g_model_out -- of P too -- x0_hat and the
    clamp gate are the clean run's bit for bit, and sample / x_{t-1} are non-finite at that one element alone"""
    cs = _case(K, oracle, name, hw, n, seed=6)
    noise = cs.noise.copy()
    noise[P, 0, 0, 0] = np.inf
    for power, finalize in ((1, True), (2, False)):
        clean = _hip(K, cs, cs.x, cs.mo, cs.noise, cs.y, 0.5, power, finalize=finalize)
        out = _hip(K, cs, cs.x, cs.mo, noise, cs.y, 0.5, power, finalize=finalize)
        for f in ("norm", "g_model_out", "x0_hat", "inside"):
            assert torch.equal(getattr(out, f), getattr(clean, f)), f
        for f in ("sample", "x_next"):
            a, b = getattr(out, f), getattr(clean, f)
            bad = ~torch.isfinite(a)
            assert int(bad.sum()) == 1 and bool(bad[P, 0, 0, 0])
            assert torch.equal(a[~bad], b[~bad]), f
