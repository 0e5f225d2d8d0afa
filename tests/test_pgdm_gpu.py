"""GPU suite of pseudoinverse guidance on the CG solve (dpsx_cg_pullback_f32, OpHandle.cg_pullback, the `pgdm` method and its
loops).

References: dpsx_cg_step_f32 for d and dist (bit for bit: the chains differ in the last launch only), numpy fp32 for the
launch's element expression (bit for bit), tests/pgdm_ref.py over the oracle's operators for the values (float64).
Inputs: cg's shapes and measurements (test_cg_gpu._case); x0_hat and the clamp gate are what the device's S1 makes of a
target 0.45 sigma around the image, so a few percent of the elements are clamped.  Records: DDPM t = 500 and t = 0, DDIM
eta = 0.5 t = 500; rho in {0, 0.25, 4}; iters in {0, 1, 5}.
Bounds: 1e-4 rel-L2 per particle against float64 (the bound test_cg_gpu holds d to), 1e-6 against the closed forms,
equality where the same launches must give the same bits.  The float64 solve at 2 x 3 x 256 x 256 costs ten seconds on the
host, so that shape is compared with float64 at one record and rho (as test_cg_gpu does) and bit for bit with
dpsx_cg_step_f32 at all of them.

Observed on an MI355X (g against float64, maximum over the cases): see DESIGN.md, "Pseudoinverse guidance"."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pgdm_ref
from placement import Buf
from standin import rel_l2
from test_cg_gpu import SENTINEL, Spy, _case, _loop_setup, _patch_rng, _sampler
from test_hip_parity import DEV, K, coefs_of, ddim_coefs_of, dev, host  # noqa: F401 (K: fixture)

pytestmark = pytest.mark.gpu
RHOS, ITERS = (0.0, 0.25, 4.0), (0, 1, 5)
SMALL = [(name, 3, 3, 64, 64) for name in ("gauss", "gauss_taps", "motion", "sr4", "mask", "ident")]
ODD = ("gauss9", 2, 1, 33, 47)
BIG = ("gauss", 2, 3, 256, 256)
RECORDS = ("ddpm500", "ddpm0", "ddim500")


def _lib():
    from dps_ttc_amd import _lib as L
    return L.lib(), L


def _record(K, oracle, tag):
    """-> (the oracle's record, the dpsx_coefs record, gain) -- gain: the "score" scalar of that record from the float64
    restatement, rounded to fp32 once"""
    sched = oracle.tables.schedule(1000)
    t = 0 if tag == "ddpm0" else 500
    c, ck = ddim_coefs_of(K, oracle, t, 0.5) if tag == "ddim500" else coefs_of(K, oracle, t)
    tb = pgdm_ref.tables(sched["betas"])
    rec = pgdm_ref.record(tb, t, 0.5 if tag == "ddim500" else None)
    _, gain = pgdm_ref.scalars(tb, t, rec, 0.05, "score", 1.0)
    return c, ck, float(np.float32(gain))


_S1 = {}


def _s1(K, oracle, golden, shape, tag, y_n=1):
    """the case's x0_hat, sample and clamp gate from the device's S1 under record `tag` (built once, shared, host copies)"""
    key = (shape, tag, y_n)
    if key not in _S1:
        cs = _case(K, oracle, golden, *shape, y_n=y_n)
        c, ck, gain = _record(K, oracle, tag)
        rng = np.random.RandomState(len(tag) + shape[3])
        target = cs.x0 + 0.45 * rng.randn(*cs.shape)
        x_t = rng.randn(*cs.shape).astype(np.float32)
        eps = ((c["a"] * x_t - target) / c["b"]).astype(np.float32)
        mo = np.concatenate([eps, rng.uniform(-1, 1, eps.shape).astype(np.float32)], axis=1)
        x0, sample, inside = K.posterior_fwd(dev(x_t), dev(mo), dev(rng.randn(*cs.shape).astype(np.float32)), ck,
                                             want_inside=True)
        torch.cuda.synchronize()
        frac = 1.0 - float(inside.float().mean())
        assert 0.005 < frac < 0.5, frac                        # some elements are clamped, most are not
        _S1[key] = SimpleNamespace(cs=cs, ck=ck, gain=gain, x0=host(x0).copy(), sample=host(sample).copy(),
                                   inside=inside.cpu().numpy().copy(), refs={})
    return _S1[key]


def _off(t, off):
    """a copy of t whose address is `off` bytes past a 16-byte boundary"""
    if not off:
        return t.contiguous()
    size = t.element_size()
    flat = torch.empty(t.numel() + off // size, dtype=t.dtype, device=t.device)
    view = flat[off // size:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == off
    return view


def _pull(s, rho, iters, gain=None, x0=None, inside=None, y=None, rows=None, off=0, fill=SENTINEL, stream=None, d_out=True):
    """one dpsx_cg_pullback_f32 on buffers of this call's own -> host copies (g_model_out, dist, d).  off: every buffer
    that many bytes off the 16-byte grid.  fill: what g_model_out holds before the call."""
    lib, L = _lib()
    sl = slice(None) if rows is None else rows
    x0 = dev((s.x0 if x0 is None else x0)[sl])
    n, c, h, w = x0.shape
    x0 = _off(x0, off)
    ins = _off(dev((s.inside if inside is None else inside)[sl]), off)
    yt = _off(dev(s.cs.y if y is None else y), off)
    g = _off(torch.full((n, 2 * c, h, w), fill, device=DEV), off)
    dist, d = _off(torch.full((n,), SENTINEL, device=DEV), off), _off(torch.full((n, c, h, w), SENTINEL, device=DEV), off)
    need = int(lib.dpsx_cg_workspace_bytes(s.cs.handle._h, n, c, h, w))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    st = L.stream_of(x0) if stream is None else stream
    rc = lib.dpsx_cg_pullback_f32(s.cs.handle._h, L.ptr(x0), L.ptr(ins), L.ptr(yt), yt.shape[0], rho, iters,
                                  s.gain if gain is None else gain, L.ptr(g), L.ptr(dist), L.ptr(d) if d_out else None,
                                  n, c, h, w, L.ptr(ws), need, st)
    assert rc == L.OK, rc
    torch.cuda.synchronize()
    return host(g).copy(), host(dist).copy(), host(d).copy()


def _cg(s, rho, iters, rows=None, y=None, x0=None):
    """dpsx_cg_step_f32 on the same inputs -> host copies (dist, d): the reference of d_out and dist"""
    sl = slice(None) if rows is None else rows
    x0 = (s.x0 if x0 is None else x0)[sl]
    _, dist, d = s.cs.handle.cg_step(dev(x0), dev(s.sample[sl]), dev(s.cs.y if y is None else y), rho, iters, s.ck,
                                     want_d=True)
    torch.cuda.synchronize()
    return host(dist).copy(), host(d).copy()


def _check_bits(s, out, rho, iters, rows=None, gain=None, **kw):
    """the three bit-for-bit statements of one call: d_out and dist are dpsx_cg_step_f32's, the eps half is numpy fp32
    where(inside, gain * d_out, +0.0), the variance half still holds the sentinel"""
    g, dist, d = out
    gain = np.float32(s.gain if gain is None else gain)
    sl = slice(None) if rows is None else rows
    dist_ref, d_ref = _cg(s, rho, iters, rows, **kw)
    assert np.array_equal(d.view(np.uint32), d_ref.view(np.uint32)) and np.array_equal(dist.view(np.uint32), dist_ref.view(np.uint32))
    c = d.shape[1]
    want = np.where(s.inside[sl] != 0, gain * d, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(g[:, :c].view(np.uint32), want.view(np.uint32))
    assert np.all(g[:, c:] == SENTINEL)


def _ref(s, rho):
    """float64 d after 1 and 5 iterations and dist: one 5-iteration solve per (inputs, rho) -> {iters: (d, dist)}"""
    if rho not in s.refs:
        ds, dist = pgdm_ref.solve_at(s.cs.orc, s.x0, s.cs.y, rho, (1, 5))
        s.refs[rho] = {k: (d, dist) for k, d in ds.items()}
    return s.refs[rho]


# ------------------------------------------------------------------ 1. against cg_step, the expression, float64
@pytest.mark.parametrize("tag", RECORDS)
@pytest.mark.parametrize("shape", SMALL + [ODD], ids=lambda s: s[0])
def test_against_cg_step_and_float64(K, oracle, golden, shape, tag):
    s = _s1(K, oracle, golden, shape, tag)
    off = 4 if shape is ODD else 0                              # the scalar form, every buffer 4 bytes off the grid
    worst = 0.0
    for rho in RHOS:
        for iters in ITERS:
            out = _pull(s, rho, iters, off=off)
            _check_bits(s, out, rho, iters)
            g, dist, d = out
            c = d.shape[1]
            if iters == 0:
                assert not d.any() and not g[:, :c].any() and not np.signbit(g[:, :c]).any()
                continue
            d_ref, dist_ref = _ref(s, rho)[iters]
            g_ref = np.where(s.inside != 0, float(np.float32(s.gain)) * d_ref, 0.0)
            errs = [rel_l2(g[p, :c], g_ref[p]) for p in range(g.shape[0])]
            worst = max(worst, *errs)
            assert max(errs) <= 1e-4, (rho, iters, errs)
            assert rel_l2(dist, dist_ref) <= 1e-4
    print(f"g against float64 {shape[0]} {tag}: max rel-L2 per particle {worst:.2e}")


@pytest.mark.parametrize("tag", RECORDS)
def test_192_slots_against_cg_step(K, oracle, golden, tag):
    s = _s1(K, oracle, golden, BIG, tag)
    for rho in RHOS:
        for iters in ITERS:
            _check_bits(s, _pull(s, rho, iters), rho, iters)
    if tag == "ddpm500":
        g, dist, d = _pull(s, 0.25, 5)
        g_ref, _, dist_ref = pgdm_ref.pullback(s.cs.orc, s.x0, s.cs.y, s.inside, 0.25, 5, s.gain)
        errs = [rel_l2(g[p, :3], g_ref[p]) for p in range(2)]
        print(f"g against float64 256x256: {errs}")
        assert max(errs) <= 1e-4 and rel_l2(dist, dist_ref) <= 1e-4


def test_without_d_out_and_with_the_handle(K, oracle, golden):
    """d_out = NULL gives the same g; OpHandle.cg_pullback returns the same bits with a zero variance half"""
    s = _s1(K, oracle, golden, SMALL[0], "ddim500")
    a = _pull(s, 0.25, 5)
    b = _pull(s, 0.25, 5, d_out=False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.all(b[2] == SENTINEL)
    for iters in (5, 0):
        a = _pull(s, 0.25, iters, fill=0.0)
        g, dist, d = s.cs.handle.cg_pullback(dev(s.x0), dev(s.inside), dev(s.cs.y), 0.25, iters, s.gain, want_d=True)
        torch.cuda.synchronize()
        assert np.array_equal(host(g), a[0]) and np.array_equal(host(dist), a[1]) and np.array_equal(host(d), a[2])
        assert not host(g)[:, 3:].any()


# ------------------------------------------------------------------ 2. closed forms
@pytest.mark.parametrize("name", ["mask", "ident"])
def test_closed_forms(K, oracle, golden, name):
    """mask and identity: D = m (y - x0_hat) / (1 + rho) after one iteration"""
    s = _s1(K, oracle, golden, (name, 3, 3, 64, 64), "ddpm500")
    m = s.cs.orc.forward(np.ones((1, 3, 64, 64), dtype=np.float32)).astype(np.float64)
    for rho in RHOS:
        for iters in (1, 5):
            g, _, d = _pull(s, rho, iters)
            want = m * (s.cs.y.astype(np.float64) - m * s.x0) / (1.0 + rho)
            err = rel_l2(d, want)
            err_g = rel_l2(g[:, :3], np.where(s.inside != 0, float(np.float32(s.gain)) * want, 0.0))
            print(f"closed form {name} rho={rho} iters={iters}: d {err:.2e} g {err_g:.2e}")
            assert err <= 1e-6 and err_g <= 1e-6


# ------------------------------------------------------------------ 3. the gate
def test_all_outside_particle_keeps_the_sample(K, oracle, golden):
    """a particle whose gate is all zero: g = +0.0 everywhere and, through K3 with g_unet = 0, x_next is `sample` bit for bit
    (-0.0 kept)"""
    lib, L = _lib()
    s = _s1(K, oracle, golden, SMALL[0], "ddpm500")
    inside = s.inside.copy()
    inside[1] = 0
    g, _, d = _pull(s, 0.25, 5, inside=inside, fill=0.0)
    assert d[1].any() and not g[1].any() and not np.signbit(g[1]).any()
    assert g[0, :3].any() and g[2, :3].any()
    sample = s.sample.copy()
    sample[1, 0, 0, :8] = -0.0
    for gu in (torch.zeros(s.cs.shape, device=DEV), None):
        out = torch.full(s.cs.shape, SENTINEL, device=DEV)
        st, gt = dev(sample), dev(g)
        assert lib.dpsx_step_update_f32(L.ptr(st), L.ptr(gt), L.ptr(gu), L.ptr(out), 3, 3 * 64 * 64, s.ck,
                                        L.stream_of(out)) == L.OK
        torch.cuda.synchronize()
        assert np.array_equal(host(out)[1].view(np.uint32), sample[1].view(np.uint32))
        assert not np.array_equal(host(out)[0], sample[0])


# ------------------------------------------------------------------ 4. bit-for-bit properties
@pytest.mark.parametrize("shape", [SMALL[0], SMALL[3], SMALL[4], ODD], ids=lambda s: s[0])
def test_batch_equals_single_particles(K, oracle, golden, shape):
    s = _s1(K, oracle, golden, shape, "ddim500")
    g, dist, d = _pull(s, 0.25, 5)
    for p in range(shape[1]):
        gp, np_, dp = _pull(s, 0.25, 5, rows=slice(p, p + 1))
        assert np.array_equal(gp[0], g[p]) and np.array_equal(dp[0], d[p]) and np_[0] == dist[p], p


@pytest.mark.parametrize("y_n", [4, 2])
def test_measurement_rows(K, oracle, golden, y_n):
    """y with N rows, and with M = 2 rows for N = 4 (image-major), equals the separate calls"""
    s = _s1(K, oracle, golden, ("gauss", 4, 3, 64, 64), "ddpm500", y_n=y_n)
    g, dist, d = _pull(s, 0.25, 5)
    k = 4 // y_n
    for m in range(y_n):
        sl = slice(m * k, (m + 1) * k)
        gm, nm, dm = _pull(s, 0.25, 5, rows=sl, y=s.cs.y[m:m + 1])
        assert np.array_equal(gm, g[sl]) and np.array_equal(dm, d[sl]) and np.array_equal(nm, dist[sl]), m
    assert not np.array_equal(d[0], d[3])


@pytest.mark.parametrize("shape", [SMALL[0], SMALL[3], SMALL[4]], ids=lambda s: s[0])
def test_nan_stays_in_its_particle(K, oracle, golden, shape):
    s = _s1(K, oracle, golden, shape, "ddpm500")
    clean = _pull(s, 0.25, 5)
    x0 = s.x0.copy()
    x0[1, 1, 20, 31] = np.nan
    bad = _pull(s, 0.25, 5, x0=x0)
    for q in (0, 2):
        assert all(np.array_equal(u[q], v[q]) for u, v in zip(clean, bad)), q
    assert np.isnan(bad[1][1]) and np.isnan(bad[0][1, :3]).any() and np.all(bad[0][1, 3:] == SENTINEL)


def test_stream_argument(K, oracle, golden):
    """the chain runs on the stream it is given: a side stream that is not torch's current one gives the same bits"""
    import ctypes
    s = _s1(K, oracle, golden, SMALL[2], "ddim500")
    ref = _pull(s, 0.25, 5)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    out = _pull(s, 0.25, 5, stream=ctypes.c_void_p(side.cuda_stream))
    assert all(np.array_equal(a, b) for a, b in zip(ref, out))


def test_graph_capture(K, oracle, golden):
    """One chain allocates nothing and never synchronises: captured on a side stream and replayed twice, it gives the eager
    call's bits -- the 5-iteration chain and the iters = 0 chain (whose eps half is a strided memset)"""
    s = _s1(K, oracle, golden, SMALL[0], "ddim500")
    x0, inside, y = dev(s.x0), dev(s.inside), dev(s.cs.y)
    for iters in (5, 0):
        def step():
            return s.cs.handle.cg_pullback(x0, inside, y, 0.25, iters, s.gain, want_d=True)

        ref = [t.clone() for t in step()]        # eager (also the warm-up: buffers, kernel attributes)
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                out = step()
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(2):
            for t in (out[1], out[2]):
                t.fill_(SENTINEL)
            out[0][:, :3].fill_(SENTINEL)
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(out, ref))


# ------------------------------------------------------------------ 5. refusals before any launch
def test_argument_errors_touch_nothing(K, oracle, golden):
    from dps_ttc_amd.measurements import get_operator
    lib, L = _lib()
    s = _s1(K, oracle, golden, ("gauss", 4, 3, 64, 64), "ddpm500")
    x0, inside, y = dev(s.x0), dev(s.inside), dev(s.cs.y)
    g, d = torch.full((4, 6, 64, 64), SENTINEL, device=DEV), torch.full((4, 3, 64, 64), SENTINEL, device=DEV)
    dist = torch.full((4,), SENTINEL, device=DEV)
    ws = torch.empty(int(lib.dpsx_cg_workspace_bytes(s.cs.handle._h, 4, 3, 64, 64)), dtype=torch.uint8, device=DEV)

    def call(handle, rho=0.25, iters=5, gain=0.5, y_n=1, ws_bytes=None, ins=inside):
        return lib.dpsx_cg_pullback_f32(handle._h, L.ptr(x0), L.ptr(ins), L.ptr(y), y_n, rho, iters, gain, L.ptr(g),
                                        L.ptr(dist), L.ptr(d), 4, 3, 64, 64, L.ptr(ws),
                                        ws.numel() if ws_bytes is None else ws_bytes, L.stream_of(x0))

    h = s.cs.handle
    assert call(h, iters=-1) == L.EINVAL and call(h, iters=65) == L.EINVAL
    assert call(h, rho=-0.5) == L.EINVAL and call(h, rho=float("nan")) == L.EINVAL and call(h, rho=float("inf")) == L.EINVAL
    assert call(h, gain=float("nan")) == L.EINVAL and call(h, gain=float("inf")) == L.EINVAL
    assert call(h, y_n=3) == L.EINVAL and call(h, ins=None) == L.EINVAL
    assert call(h, ws_bytes=ws.numel() - 256) == L.EWORKSPACE
    phase = get_operator("phase_retrieval", oversample=2.0, device=DEV).hip_handle(x0)
    assert call(phase) == L.EUNSUPPORTED
    with pytest.raises(L.DpsxError, match="unsupported"):
        phase.cg_pullback(x0, inside, y, 0.25, 5, 0.5)
    torch.cuda.synchronize()
    for t in (g, d, dist):
        assert bool((t == SENTINEL).all())
    assert call(h, iters=2) == L.OK                                         # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert not bool((g[:, :3] == SENTINEL).any()) and bool((g[:, 3:] == SENTINEL).all())
    assert not bool((dist == SENTINEL).any()) and not bool((d == SENTINEL).any())


# ------------------------------------------------------------------ 6. placement
def _placement_tags():
    from test_placement_gpu import LINEAR
    return LINEAR


@pytest.mark.parametrize("tag", _placement_tags())
def test_placement(K, oracle, golden, tag):
    """exact-size buffers between guard bands and the workspace at exactly the queried size: aligned, all off the grid,
    each pointer alone; every output element written, no guard byte touched, the variance half left as it was.  (The
    operators' own launches take other forms off the grid, so d agrees across placements within the bound, not bit for bit;
    inside one placement g is the expression on that placement's d, bit for bit.)"""
    import cg_ref
    from test_placement_gpu import F32, U8, Step, _setup, _stream, run_case, ws_refused
    lib, L = _lib()
    s = _setup(K, oracle, golden, tag)
    n, c, h, w = s.shape
    rho, iters, gain = 0.25, 3, np.float32(0.37)
    need = int(lib.dpsx_cg_workspace_bytes(s.hp, n, c, h, w))
    x0 = np.clip(s.x + 0.3 * s.g_extra * 20, -1, 1).astype(np.float32)
    inside = (np.abs(x0) < 1).astype(np.uint8)
    assert 0 < inside.mean() < 1
    d_ref, dist_ref = cg_ref.solve(s.orc, x0, s.y, rho, iters)
    g_ref = np.where(inside != 0, float(gain) * d_ref, 0.0)
    g0 = np.full((n, 2 * c, h, w), SENTINEL, dtype=np.float32)
    bufs = [Buf("x0_hat", s.shape, F32, "in"), Buf("inside", s.shape, U8, "in"), Buf("y", (1,) + s.mshape, F32, "in"),
            Buf("g", (n, 2 * c, h, w), F32, "inout"), Buf("dist", (n,), F32, "out"), Buf("d", s.shape, F32, "out"),
            Buf("ws", (need,), U8, "ws")]

    def verify(out, ptag):
        g = out["g"]
        errs = [rel_l2(g[p, :c], g_ref[p]) for p in range(n)] + [rel_l2(out["d"], d_ref), rel_l2(out["dist"], dist_ref)]
        assert max(errs) <= 1e-4, (ptag, errs)
        want = np.where(inside != 0, gain * out["d"], np.float32(0.0)).astype(np.float32)
        assert np.array_equal(g[:, :c].view(np.uint32), want.view(np.uint32)), ptag
        assert np.all(g[:, c:] == SENTINEL), ptag

    run_case(f"{tag} pgdm", bufs, {"x0_hat": x0, "inside": inside, "y": s.y, "g": g0},
             [Step("dpsx_cg_pullback_f32", lambda a, wb: lib.dpsx_cg_pullback_f32(
                 s.hp, a.ptr("x0_hat"), a.ptr("inside"), a.ptr("y"), 1, rho, iters, float(gain), a.ptr("g"), a.ptr("dist"),
                 a.ptr("d"), n, c, h, w, a.ptr("ws"), wb, _stream()), ["dist", "d"], ws_refused(True))],
             verify, ws="ws")


# ------------------------------------------------------------------ 7. the loops
def _pgdm_setup(K, **kw):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    s = _loop_setup(K, **kw)
    s.pg = get_conditioning_method("pgdm", s.op, get_noise("gaussian", sigma=0.05), iters=5)
    return s


def _loop(smp, s, fn, x=None, y=None, model=None):
    out = smp.p_sample_loop(model=model or s.model, x_start=(s.x_start if x is None else x).clone(),
                            measurement=s.y if y is None else y, measurement_cond_fn=fn, record=False, save_root=None)
    return out[0], out[1]


def _ddim(name, eta, respacing="6"):
    smp = _sampler(name, respacing)
    if name != "ddpm":
        smp.eta = eta
    return smp


@pytest.mark.parametrize("name,eta,respacing", [("ddpm", None, "6"), ("ddim", 0.0, "logsnr10"), ("ddim", 0.5, "logsnr10"),
                                                ("ttc_ddim", 0.5, "6")])
def test_loops_equal_the_composed_steps(K, name, eta, respacing):
    """the loop against the launches composed by hand: the stand-in model with a graph, posterior_fwd, the entry,
    autograd.grad, dpsx_step_update_f32 -- with the host scalars of the float64 restatement"""
    lib, L = _lib()
    s = _pgdm_setup(K)
    smp, spy = _ddim(name, eta, respacing), Spy(s.model)
    steps = smp.num_timesteps
    bank = torch.randn(steps, *s.x_start.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    if name == "ttc_ddim":
        smp.resample_draw = "device"
    it = _patch_rng(smp, bank, s.ubank, 0)
    img, dist = _loop(smp, s, s.pg.conditioning, model=spy)
    assert it["z"] == steps and len(spy.grad_enabled) == steps and it["u"] == (1 if name == "ttc_ddim" else 0)
    assert all(spy.grad_enabled) and all(spy.requires_grad)
    assert not img.requires_grad and dist.shape == (4,)
    handle, ref, d_ref = s.op.hip_handle(), s.x_start.clone(), None
    tb = pgdm_ref.tables(smp.betas)
    n, chw = ref.shape[0], ref[0].numel()
    _patch_rng(smp, bank, s.ubank, 0)
    for i, idx in enumerate(range(steps - 1, -1, -1)):
        coefs = smp.sample_coefs(idx)
        rho, gain = pgdm_ref.scalars(tb, idx, pgdm_ref.record(tb, idx, eta), 0.05)
        x = ref.detach().requires_grad_()
        with torch.enable_grad():
            mo = s.model(x, smp._model_timesteps(x.device)[idx:idx + 1])
        x0_hat, sample, inside = K.posterior_fwd(x.detach(), mo.detach(), bank[i].contiguous(), coefs, want_inside=True)
        g, d_ref = handle.cg_pullback(x0_hat, inside, s.y, float(np.float32(rho)), 5, float(np.float32(gain)))
        (gu,) = torch.autograd.grad(mo, x, grad_outputs=g)
        ref = torch.empty_like(sample)
        assert lib.dpsx_step_update_f32(L.ptr(sample), L.ptr(g), L.ptr(gu.contiguous()), L.ptr(ref), n, chw, coefs,
                                        L.stream_of(ref)) == L.OK
        d_ref = d_ref.clone()
        if name == "ttc_ddim" and idx % 10 == 0:
            ref, d_ref = smp._resample(ref, d_ref, 100)
    torch.cuda.synchronize()
    assert torch.equal(img, ref) and torch.equal(dist, d_ref)
    assert bool(torch.isfinite(img).all()) and bool((dist > 0).all())


@pytest.mark.parametrize("name,masks", [("ddpm", False), ("ddim", True), ("ttc_ddim", False)])
def test_loops_multi_image(K, name, masks):
    """M = 2 images x K = 2 particles, one measurement (and one mask) per image = the two single-image loops"""
    s = _pgdm_setup(K, rows=2, masks=masks)

    def run(x, y, mk, offset):
        smp = _ddim(name, 0.5)
        smp.resample_draw = "device"
        it = _patch_rng(smp, s.bank, s.ubank, offset)
        fn = s.pg.conditioning if mk is None else functools.partial(s.pg.conditioning, mask=mk)
        out = _loop(smp, s, fn, x=x, y=y)
        assert it["z"] == 6 and it["u"] == (1 if name == "ttc_ddim" else 0)
        return out

    img, dist = run(s.x_start, s.y, s.masks, 0)
    assert img.shape == s.x_start.shape and dist.shape == (4,)
    for m in range(2):
        sl = slice(2 * m, 2 * m + 2)
        img_m, dist_m = run(s.x_start[sl], s.y[m:m + 1], None if s.masks is None else s.masks[m:m + 1], 2 * m)
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m), m


@pytest.mark.parametrize("name", ["ddpm", "ddim"])
def test_device_noise_splits_by_path(K, name):
    """noise_draw = "device": 4 paths in one batch = 2 + 2"""
    s = _pgdm_setup(K)

    def run(x, base):
        smp = _ddim(name, 0.5)
        smp.noise_draw, smp.noise_seed, smp.path_base = "device", 9, base
        return _loop(smp, s, s.pg.conditioning, x=x)

    img, dist = run(s.x_start, 0)
    for lo in (0, 2):
        img_h, dist_h = run(s.x_start[lo:lo + 2], lo)
        assert torch.equal(img[lo:lo + 2], img_h) and torch.equal(dist[lo:lo + 2], dist_h), lo
    assert not torch.equal(img[0], img[2])


def test_loop_with_repulsion_and_clean_noiser(K):
    """repulsion runs on the pgdm route as on cg's, and a clean measurement (rho = 0) runs"""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    s = _pgdm_setup(K)
    plain, pushed = _ddim("ddpm", None), _ddim("ddpm", None)
    pushed.repulsion_scale = 0.5
    _patch_rng(plain, s.bank, s.ubank, 0)
    _patch_rng(pushed, s.bank, s.ubank, 0)
    a, b = _loop(plain, s, s.pg.conditioning)[0], _loop(pushed, s, s.pg.conditioning)[0]
    assert bool(torch.isfinite(b).all()) and not torch.equal(a, b)
    clean = get_conditioning_method("pgdm", s.op, get_noise("clean"), iters=2)
    smp = _ddim("ddim", 0.0)
    _patch_rng(smp, s.bank, s.ubank, 0)
    img, dist = _loop(smp, s, clean.conditioning)
    assert bool(torch.isfinite(img).all()) and bool((dist > 0).all())
