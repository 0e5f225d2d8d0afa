"""GPU suite of the CG data-consistency step (dpsx_cg_step_f32, OpHandle.cg_step, the `cg` method and its loops).

Reference: tests/cg_ref.py (float64 vectors over the oracle's operators).  Inputs as in the CPU suite: y = A x* + 0.05
noise, x0_hat = clip(x* + 0.3 noise), one measurement row unless a test says otherwise.  Bounds: rel-L2 <= 1e-4 on d and
on x_next against the restatement (BASELINE.md's gate for x_{t-1}; the restatement with operators 1e-5 off stays under
4e-5 on these inputs), 1e-6 against the closed forms, torch.equal where the same launches must give the same bits."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cg_ref
from standin import StandInModel, rel_l2
from test_hip_parity import DEV, K, coefs_of, ddim_coefs_of, dev, host  # noqa: F401 (K: fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7.25


def _ops(K, oracle, golden, name, c, h, w):
    """-> (product operator, its handle, forward kwargs, oracle operator)"""
    from dps_ttc_amd.measurements import get_operator
    g = golden("operators")
    fkw = {}
    if name in ("gauss", "gauss_taps", "gauss9"):
        ks, sig = (9, 1.0) if name == "gauss9" else (61, 3.0)
        op = get_operator("gaussian_blur", kernel_size=ks, intensity=sig, device=DEV)
        orc = oracle.make_operator("gaussian_blur", kernel_size=ks, intensity=sig)
        handle = K.OpHandle.blur(op._weights, DEV, force_taps=True) if name == "gauss_taps" else op.hip_handle()
    elif name == "motion":
        op = get_operator("motion_blur", kernel_size=61, intensity=0.5, device=DEV)
        op._set_weights(g["motion.kernel"])
        orc, handle = oracle.make_operator("motion_blur", kernel=g["motion.kernel"]), op.hip_handle()
    elif name == "sr4":
        op = get_operator("super_resolution", in_shape=(1, c, h, w), scale_factor=4, device=DEV)
        orc, handle = oracle.make_operator("super_resolution", in_shape=(1, c, h, w), scale_factor=4), op.hip_handle()
    elif name == "mask":
        op = get_operator("inpainting", device=DEV)
        fkw = {"mask": dev(g["inpaint.mask"])}
        orc, handle = oracle.make_operator("inpainting", mask=g["inpaint.mask"]), op.hip_handle_for(fkw["mask"])
    elif name == "ident":
        op = get_operator("noise", device=DEV)
        orc, handle = oracle.make_operator("noise"), op.hip_handle()
    else:
        raise KeyError(name)
    return op, handle, fkw, orc


_CASES = {}


def _case(K, oracle, golden, name, n, c, h, w, y_n=1, seed=0):
    """inputs of one step (built once per shape and shared; nothing modifies them)"""
    key = (name, n, c, h, w, y_n, seed)
    if key not in _CASES:
        op, handle, fkw, orc = _ops(K, oracle, golden, name, c, h, w)
        rng = np.random.RandomState(seed + h + n)
        xs = rng.uniform(-1, 1, (y_n, c, h, w)).astype(np.float32)
        ax = orc.forward(xs)
        y = (ax + 0.05 * rng.randn(*ax.shape)).astype(np.float32)
        x0 = np.clip(cg_ref.rows(xs, n) + 0.3 * rng.randn(n, c, h, w), -1, 1).astype(np.float32)
        sample = rng.randn(n, c, h, w).astype(np.float32)
        _CASES[key] = SimpleNamespace(op=op, handle=handle, fkw=fkw, orc=orc, y=y, x0=x0, sample=sample, n=n,
                                      shape=(n, c, h, w), refs={})
    return _CASES[key]


def _ref(cs, rho, iters):
    if (rho, iters) not in cs.refs:
        cs.refs[(rho, iters)] = cg_ref.solve(cs.orc, cs.x0, cs.y, rho, iters)
    return cs.refs[(rho, iters)]


def _run(cs, rho, iters, ck, x0=None, sample=None, y=None, handle=None):
    """one cg_step -> host copies (x_next, dist, d)"""
    out = (handle or cs.handle).cg_step(dev(cs.x0 if x0 is None else x0), dev(cs.sample if sample is None else sample),
                                        dev(cs.y if y is None else y), rho, iters, ck, want_d=True)
    torch.cuda.synchronize()
    return tuple(host(t).copy() for t in out)


def _records(K, oracle):
    """t = 500: the DDPM record and the DDIM record with eta = 0.5, each with the oracle's dict"""
    c, ck = coefs_of(K, oracle, 500)
    cd, ckd = ddim_coefs_of(K, oracle, 500, 0.5)
    return [("ddpm", c, ck), ("ddim", cd, ckd)]


# ------------------------------------------------------------------ 1. parity with the restatement
SMALL = [(name, 3, 3, 64, 64) for name in ("gauss", "gauss_taps", "motion", "sr4", "mask", "ident")]
PARITY = [(*s, rho, iters) for s in SMALL for rho in (0.25, 4.0) for iters in (1, 5)] + \
         [("gauss", 2, 3, 128, 128, rho, iters) for rho in (0.25, 4.0) for iters in (1, 5)] + \
         [("gauss9", 2, 1, 33, 47, rho, iters) for rho in (0.25, 4.0) for iters in (1, 5)] + \
         [("gauss", 2, 3, 256, 256, 0.25, 5)]


@pytest.mark.parametrize("name,n,c,h,w,rho,iters", PARITY)
def test_parity_with_the_restatement(K, oracle, golden, name, n, c, h, w, rho, iters):
    cs = _case(K, oracle, golden, name, n, c, h, w)
    d_ref, dist_ref = _ref(cs, rho, iters)
    for tag, c_rec, ck in _records(K, oracle):
        x_next, dist, d = _run(cs, rho, iters, ck)
        kappa = float(cg_ref.kappa(c_rec))
        assert kappa == K.cg_kappa(ck)
        x_ref = cs.sample.astype(np.float64) + kappa * d_ref
        e_d, e_x, e_n = rel_l2(d, d_ref), rel_l2(x_next, x_ref), rel_l2(dist, dist_ref)
        print(f"parity {name} {n}x{c}x{h}x{w} rho={rho} iters={iters} {tag}: d {e_d:.2e} x_next {e_x:.2e} dist {e_n:.2e}")
        # dist: the suite grants A x0_hat 1e-5 rel-L2, and ||A x0_hat|| is below 10 ||r_y|| on these inputs
        assert e_d <= 1e-4 and e_x <= 1e-4 and e_n <= 1e-4
        # x_next is sample + kappa d of the device's own d, two roundings
        assert np.array_equal(x_next, cs.sample + np.float32(kappa) * d)


# ------------------------------------------------------------------ 2. closed forms
@pytest.mark.parametrize("name", ["mask", "ident"])
@pytest.mark.parametrize("iters", [1, 5])
def test_closed_forms(K, oracle, golden, name, iters):
    cs = _case(K, oracle, golden, name, 3, 3, 64, 64)
    m = cs.orc.forward(np.ones((1, 3, 64, 64), dtype=np.float32)).astype(np.float64)
    _, ck = coefs_of(K, oracle, 500)
    for rho in (0.25, 4.0):
        want = m * (cs.y.astype(np.float64) - m * cs.x0) / (1.0 + rho)
        err = rel_l2(_run(cs, rho, iters, ck)[2], want)
        print(f"closed form {name} rho={rho} iters={iters}: {err:.2e}")
        assert err <= 1e-6


# ------------------------------------------------------------------ 3. bit-exact properties
@pytest.mark.parametrize("name", ["gauss", "sr4", "mask"])
def test_batch_equals_single_particles(K, oracle, golden, name):
    cs = _case(K, oracle, golden, name, 5, 3, 64, 64)
    _, ck = ddim_coefs_of(K, oracle, 500, 0.5)
    x_next, dist, d = _run(cs, 0.25, 5, ck)
    for p in range(5):
        xp, np_, dp = _run(cs, 0.25, 5, ck, x0=cs.x0[p:p + 1], sample=cs.sample[p:p + 1])
        assert np.array_equal(xp[0], x_next[p]) and np.array_equal(dp[0], d[p]) and np_[0] == dist[p], p


@pytest.mark.parametrize("y_n", [4, 2])
def test_measurement_rows(K, oracle, golden, y_n):
    """y with N rows, and with M = 2 rows for N = 4 (image-major), equals the separate calls"""
    cs = _case(K, oracle, golden, "gauss", 4, 3, 64, 64, y_n=y_n)
    _, ck = coefs_of(K, oracle, 500)
    x_next, dist, d = _run(cs, 0.25, 5, ck)
    k = 4 // y_n
    for m in range(y_n):
        sl = slice(m * k, (m + 1) * k)
        xm, nm, dm = _run(cs, 0.25, 5, ck, x0=cs.x0[sl], sample=cs.sample[sl], y=cs.y[m:m + 1])
        assert np.array_equal(xm, x_next[sl]) and np.array_equal(dm, d[sl]) and np.array_equal(nm, dist[sl]), m
    assert not np.array_equal(d[0], d[3])


@pytest.mark.parametrize("name", ["gauss", "sr4", "mask", "gauss9"])
def test_zero_iterations(K, oracle, golden, name):
    shape = (2, 1, 33, 47) if name == "gauss9" else (3, 3, 64, 64)
    cs = _case(K, oracle, golden, name, *shape)
    _, ck = coefs_of(K, oracle, 500)
    x_next, dist, d = _run(cs, 0.25, 0, ck)
    assert np.array_equal(x_next, cs.sample) and not d.any()
    ax = cs.handle.forward(dev(cs.x0))
    _, norm = K.residual_norm(dev(cs.y), ax, want_residual=False)
    assert np.array_equal(dist, host(norm))


def test_identity_at_the_measurement(K, oracle, golden):
    """y = x0_hat of particle 0 under the identity: that particle's residual is exactly zero"""
    cs = _case(K, oracle, golden, "ident", 3, 3, 64, 64)
    _, ck = ddim_coefs_of(K, oracle, 500, 0.5)
    for iters in (1, 5):
        x_next, dist, d = _run(cs, 0.25, iters, ck, y=cs.x0[0:1])
        assert not d[0].any() and np.array_equal(x_next[0], cs.sample[0]) and dist[0] == 0.0
        assert np.isfinite(x_next).all() and np.isfinite(d).all() and np.isfinite(dist).all()
        assert d[1].any() and dist[1] > 0


@pytest.mark.parametrize("name,shape", [("motion", (3, 3, 64, 64)), ("gauss9", (2, 1, 33, 47))])
def test_two_calls_same_bits(K, oracle, golden, name, shape):
    cs = _case(K, oracle, golden, name, *shape)
    _, ck = coefs_of(K, oracle, 500)
    a, b = _run(cs, 0.25, 5, ck), _run(cs, 0.25, 5, ck)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


# ------------------------------------------------------------------ 4. degenerate values
@pytest.mark.parametrize("name", ["gauss", "sr4", "mask"])
def test_nan_stays_in_its_particle(K, oracle, golden, name):
    cs = _case(K, oracle, golden, name, 3, 3, 64, 64)
    _, ck = coefs_of(K, oracle, 500)
    clean = _run(cs, 0.25, 5, ck)
    x0 = cs.x0.copy()
    x0[1, 1, 20, 31] = np.nan
    bad = _run(cs, 0.25, 5, ck, x0=x0)
    for q in (0, 2):
        assert all(np.array_equal(u[q], v[q]) for u, v in zip(clean, bad)), q
    assert np.isnan(bad[1][1]) and np.isnan(bad[0][1]).any()


# ------------------------------------------------------------------ 5. the objective
@pytest.mark.parametrize("name", ["gauss", "motion"])
def test_objective_monotone(K, oracle, golden, name):
    cs = _case(K, oracle, golden, name, 3, 3, 64, 64)
    _, ck = coefs_of(K, oracle, 500)
    rho = 0.01
    j = [cg_ref.objective(cs.orc, cs.x0, cs.y, _run(cs, rho, k, ck)[2], rho) for k in range(6)]
    print(f"objective {name}: " + " ".join(f"{v[0]:.6e}" for v in j))
    for a, b in zip(j, j[1:]):
        assert (b <= a * (1 + 1e-6)).all(), j
    assert (j[1] < j[0]).all()              # and the first iteration does descend


# ------------------------------------------------------------------ 6. refusals before any launch
def test_argument_errors_touch_nothing(K, oracle, golden):
    from dps_ttc_amd import _lib
    from dps_ttc_amd.measurements import get_operator
    cs = _case(K, oracle, golden, "gauss", 4, 3, 64, 64)
    _, ck = coefs_of(K, oracle, 500)
    lib = _lib.lib()
    x0, sample, y = dev(cs.x0), dev(cs.sample), dev(cs.y)
    x_next, d = torch.full_like(sample, SENTINEL), torch.full_like(sample, SENTINEL)
    dist = torch.full((4,), SENTINEL, device=DEV)
    ws = torch.empty(int(lib.dpsx_cg_workspace_bytes(cs.handle._h, 4, 3, 64, 64)), dtype=torch.uint8, device=DEV)

    def call(handle, rho=0.25, iters=5, y_t=y, y_n=1, ws_bytes=None, shape=(4, 3, 64, 64)):
        return lib.dpsx_cg_step_f32(handle._h, _lib.ptr(x0), _lib.ptr(sample), _lib.ptr(y_t), y_n, rho, iters,
                                    ck, _lib.ptr(x_next), _lib.ptr(dist), _lib.ptr(d), *shape, _lib.ptr(ws),
                                    ws.numel() if ws_bytes is None else ws_bytes, _lib.stream_of(x0))

    assert call(cs.handle, iters=-1) == _lib.EINVAL and call(cs.handle, iters=65) == _lib.EINVAL
    assert call(cs.handle, rho=-0.5) == _lib.EINVAL
    assert call(cs.handle, rho=float("nan")) == _lib.EINVAL and call(cs.handle, rho=float("inf")) == _lib.EINVAL
    assert call(cs.handle, y_n=3) == _lib.EINVAL
    assert call(cs.handle, ws_bytes=ws.numel() - 256) == _lib.EWORKSPACE
    phase = get_operator("phase_retrieval", oversample=2.0, device=DEV).hip_handle(x0)
    assert call(phase) == _lib.EUNSUPPORTED
    assert lib.dpsx_cg_workspace_bytes(phase._h, 4, 3, 64, 64) == _lib.EUNSUPPORTED
    with pytest.raises(_lib.DpsxError, match="unsupported"):
        phase.cg_step(x0, sample, y, 0.25, 5, ck)
    torch.cuda.synchronize()
    for t in (x_next, d, dist):
        assert bool((t == SENTINEL).all())
    assert call(cs.handle, iters=2) == _lib.OK                              # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not bool((x_next == SENTINEL).any()) and not bool((dist == SENTINEL).any())


# ------------------------------------------------------------------ 7. the loops
def _sampler(name, respacing="6"):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    s = create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                       model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                       rescale_timesteps=True, timestep_respacing=respacing)
    if name != "ddpm":
        s.eta = 0.5
        for t in range(s.num_timesteps):
            s.sample_coefs(t)
    return s


def _patch_rng(smp, bank, ubank, offset, n=None):
    """noise and uniforms of particle p: row offset + p of the banks' next step.  n: only draws of n rows are the step noise
    (the per-op route also draws q_sample's noise, shaped like the measurement, whose result `vanilla` does not use: it gets
    zeros and consumes nothing, so both routes see the same step noise)"""
    it = {"z": 0, "u": 0}

    def rnd(like, stride=None, shape=None):
        cnt = (tuple(shape) if shape is not None else tuple(like.shape))[0]
        if n is not None and cnt != n:
            return torch.zeros(tuple(shape) if shape is not None else tuple(like.shape), device=DEV)
        z = bank[it["z"], offset:offset + cnt].contiguous()
        it["z"] += 1
        return z

    def uni(n, like):
        v = ubank[it["u"], offset:offset + n].contiguous()
        it["u"] += 1
        return v
    smp._randn, smp._rand = rnd, uni
    return it


class Spy(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.grad_enabled, self.requires_grad = inner, [], []

    def forward(self, x, t):
        self.grad_enabled.append(torch.is_grad_enabled())
        self.requires_grad.append(bool(x.requires_grad))
        return self.inner(x, t)


def _loop_setup(K, hw=64, n=4, rows=1, masks=False, seed=11):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    gen = torch.Generator(device=DEV).manual_seed(seed)
    noiser = get_noise("gaussian", sigma=0.05)
    if masks:
        op = get_operator("inpainting", device=DEV)
        mk = torch.from_numpy((np.random.RandomState(3).rand(rows, 1, hw, hw) < 0.5).astype(np.float32)).to(DEV)
    else:
        op, mk = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV), None
    ys = []
    for m in range(rows):
        fkw = {} if mk is None else {"mask": mk[m:m + 1]}
        ys.append(op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1, **fkw).detach())
    y = torch.cat(ys).contiguous()
    y = y + 0.05 * torch.randn(y.shape, device=DEV, generator=gen)
    x_start = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
    bank = torch.randn(6, n, 3, hw, hw, device=DEV, generator=gen)
    ubank = torch.rand(1, n, device=DEV, generator=gen)
    cm = get_conditioning_method("cg", op, noiser, rho_scale=1.0, iters=5)
    vanilla = get_conditioning_method("vanilla", op, noiser)
    return SimpleNamespace(op=op, masks=mk, y=y, x_start=x_start, bank=bank, ubank=ubank, cm=cm, vanilla=vanilla,
                           model=StandInModel().to(DEV))


def _loop(smp, s, fn, x=None, y=None, model=None):
    out = smp.p_sample_loop(model=model or s.model, x_start=(s.x_start if x is None else x).clone(),
                            measurement=s.y if y is None else y, measurement_cond_fn=fn, record=False, save_root=None)
    return out[0], out[1]


@pytest.mark.parametrize("name", ["ddpm", "ddim", "ttc_ddim"])
def test_loops_equal_the_composed_steps(K, name):
    s = _loop_setup(K)
    smp, spy = _sampler(name), Spy(s.model)
    it = _patch_rng(smp, s.bank, s.ubank, 0)
    img, dist = _loop(smp, s, s.cm.conditioning, model=spy)
    assert it["z"] == 6 and len(spy.grad_enabled) == 6
    assert not any(spy.grad_enabled) and not any(spy.requires_grad)
    assert not img.requires_grad and dist.shape == (4,)
    # the same steps from the pieces, on the same noise
    handle, ref, d_ref = s.op.hip_handle(), s.x_start.clone(), None
    for i, idx in enumerate(range(5, -1, -1)):
        coefs = smp.sample_coefs(idx)
        with torch.no_grad():
            mo = s.model(ref, smp._model_timesteps(ref.device)[idx:idx + 1])
        x0_hat, sample = K.posterior_fwd(ref, mo, s.bank[i].contiguous(), coefs)
        ref, d_ref = handle.cg_step(x0_hat, sample, s.y, s.cm.rho(coefs.b), s.cm.iters, coefs)
        ref, d_ref = ref.clone(), d_ref.clone()
        if name == "ttc_ddim" and idx % 10 == 0:
            torch.manual_seed(5)
            ref, d_ref = smp._resample(ref, d_ref, 100)
    if name == "ttc_ddim":                      # the loop's multinomial draw is torch's: rerun it from the same seed
        torch.manual_seed(5)
        smp2 = _sampler(name)
        _patch_rng(smp2, s.bank, s.ubank, 0)
        img, dist = _loop(smp2, s, s.cm.conditioning)
    assert torch.equal(img, ref) and torch.equal(dist, d_ref)
    assert bool(torch.isfinite(img).all()) and bool((dist > 0).all())


@pytest.mark.parametrize("name", ["ddpm", "ddim", "ttc_ddim"])
def test_loops_end_closer_than_vanilla(K, name):
    """final ||y - A x|| per particle, same start and noise.  ttc_ddim has no vanilla form (its loop unpacks two return
    values): it is compared with the unconditioned ddim run, whose steps it shares."""
    s = _loop_setup(K)
    smp = _sampler(name)
    _patch_rng(smp, s.bank, s.ubank, 0)
    torch.manual_seed(5)
    img, _ = _loop(smp, s, s.cm.conditioning)
    base = _sampler("ddim" if name == "ttc_ddim" else name)
    _patch_rng(base, s.bank, s.ubank, 0, n=4)
    free, _ = _loop(base, s, s.vanilla.conditioning)
    handle = s.op.hip_handle()
    d_cg, d_free = handle.score(img, s.y), handle.score(free, s.y)
    print(f"{name}: cg {d_cg.tolist()} vanilla {d_free.tolist()}")
    assert bool((d_cg < d_free).all())


@pytest.mark.parametrize("name", ["ddpm", "ddim"])
def test_device_noise_splits_by_path(K, name):
    s = _loop_setup(K)

    def run(x, base):
        smp = _sampler(name)
        smp.noise_draw, smp.noise_seed, smp.path_base = "device", 9, base
        return _loop(smp, s, s.cm.conditioning, x=x)

    img, dist = run(s.x_start, 0)
    for lo in (0, 2):
        img_h, dist_h = run(s.x_start[lo:lo + 2], lo)
        assert torch.equal(img[lo:lo + 2], img_h) and torch.equal(dist[lo:lo + 2], dist_h), lo
    assert not torch.equal(img[0], img[2])


@pytest.mark.parametrize("name,masks", [("ddpm", False), ("ddim", True), ("ttc_ddim", False), ("ttc_ddim", True)])
def test_loops_multi_image(K, name, masks):
    """M = 2 images x K = 2 particles, one measurement (and one mask) per image = the two single-image loops"""
    s = _loop_setup(K, rows=2, masks=masks)

    def run(x, y, mk, offset):
        smp = _sampler(name)
        smp.resample_draw = "device"
        it = _patch_rng(smp, s.bank, s.ubank, offset)
        fn = s.cm.conditioning if mk is None else functools.partial(s.cm.conditioning, mask=mk)
        out = _loop(smp, s, fn, x=x, y=y)
        assert it["z"] == 6 and it["u"] == (1 if name == "ttc_ddim" else 0)
        return out

    img, dist = run(s.x_start, s.y, s.masks, 0)
    assert img.shape == s.x_start.shape and dist.shape == (4,)
    for m in range(2):
        sl = slice(2 * m, 2 * m + 2)
        img_m, dist_m = run(s.x_start[sl], s.y[m:m + 1], None if s.masks is None else s.masks[m:m + 1], 2 * m)
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m), m


def test_particle_groups_run_one_chain(K):
    s = _loop_setup(K)
    a = _sampler("ddpm")
    _patch_rng(a, s.bank, s.ubank, 0)
    b = _sampler("ddpm")
    b.particle_groups = 2
    _patch_rng(b, s.bank, s.ubank, 0)
    assert torch.equal(_loop(a, s, s.cm.conditioning)[0], _loop(b, s, s.cm.conditioning)[0])


# ------------------------------------------------------------------ 8. graph capture
def test_cg_step_is_graph_capturable(K, oracle, golden):
    """One chain allocates nothing and never synchronises: captured on a single side stream and replayed twice, it gives
    the eager call's bits."""
    cs = _case(K, oracle, golden, "gauss", 3, 3, 64, 64)
    _, ck = ddim_coefs_of(K, oracle, 500, 0.5)
    x0, sample, y = dev(cs.x0), dev(cs.sample), dev(cs.y)

    def step():
        return cs.handle.cg_step(x0, sample, y, 0.25, 5, ck, want_d=True)

    ref = [t.clone() for t in step()]            # eager (also the warm-up: buffers, kernel attributes)
    step()                                       # leave the alternating output where the capture will start
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in out:
            t.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, ref))
    x0.mul_(0.5)                                 # new inputs in the same buffers, same graph
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out[0], ref[0])
    replayed = [t.clone() for t in out]
    assert all(torch.equal(a, b) for a, b in zip(step(), replayed))


# ------------------------------------------------------------------ 9. the driver
def test_driver_end_to_end_cg(tmp_path):
    from test_driver_gpu import _setup
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    tpath, dpath = _setup(tmp_path, "gaussian_deblur_config_cg.yaml", "ddim")
    out = tmp_path / "results"
    drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
              "--task_config", tpath, "--save_dir", str(out), "--n_paths", "2", "--batch_size", "2",
              "--ref_image_idxs", "0", "--timestep_respacing", "3", "--seed", "0", "--gpu", "0"])
    sub = [d for d in os.listdir(out)]
    assert len(sub) == 1 and "cg_rho_scale_1.0_iters_5" in sub[0]
    root = out / sub[0]
    assert (root / "input" / "00000.png").exists() and (root / "label" / "00000.png").exists()
    assert (root / "recon_paths" / "00000" / "path#1.png").exists() and (root / "recon_paths" / "00000" / "path#2.png").exists()
    assert (root / "best_of_n" / "00000.png").exists()
    d = np.load(root / "00000_pathwise_distances.npy")
    assert d.shape == (2,) and np.isfinite(d).all() and (d > 0).all()
