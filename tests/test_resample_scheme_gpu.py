"""GPU suite: the resampling schemes and the ESS trigger (dpsx_resample_draw_seg_ex_f32 / dpsx_resample_seg_ex_f32).
Ids and flags are compared EXACTLY with the integer restatement (tests/resample_scheme_ref.py) evaluated on the kernel's
own weights; the defaults with the plain entry points; the fused launch with draw + gathers and a segmented launch with
one launch per image; and the loops with the same images run one by one -- all bit for bit (torch.equal)."""
import os
import sys

import numpy as np
import pytest
import torch

import resample_ref as R
import resample_scheme_ref as S
import test_resample_device_gpu as D          # its input builders (_case, _particles) and loop helpers
from standin import StandInModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = D.ROOT
INV = D.INV
SCHEMES = ("multinomial", "stratified", "systematic")


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).reshape(-1)


def _raw_draw(d, u, M, k, scheme, ess_q16, inv=INV):
    """the raw entry point: (rc, ids, q, flags, ess)"""
    from dps_ttc_amd import _lib
    n = M * k
    ids, q = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    flags, ess = torch.empty(M, dtype=torch.uint8, device=DEV), torch.empty(M, dtype=torch.float32, device=DEV)
    rc = _lib.lib().dpsx_resample_draw_seg_ex_f32(_lib.ptr(d), _lib.ptr(u), M, k, inv, _lib.ptr(ids), _lib.ptr(q),
                                                  scheme, ess_q16, _lib.ptr(flags), _lib.ptr(ess), _lib.stream_of(d))
    return rc, ids, q, flags, ess


# ----------------------------------------------------------------- 1: exact ids, flags, ESS
@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("k", [1, 2, 5, 64, 257, 512, 4096])
@pytest.mark.parametrize("M", [1, 3])
def test_draw_equals_the_restatement(K, M, k, scheme, tau):
    d, u = D._case(M, k, 1000 * M + k)
    ids, q, flags, ess = K.resample_draw(_dev(d), _dev(u), M, INV, want_weights=True, scheme=scheme, ess=tau,
                                         want_flags=True)
    assert ids.dtype == torch.int64 and flags.dtype == torch.uint8 and ess.dtype == torch.float32
    assert ids.shape == (M * k,) and q.shape == (M * k,) and flags.shape == (M,) and ess.shape == (M,)
    ids, q, flags, ess = ids.cpu().numpy(), q.cpu().numpy(), flags.cpu().numpy(), ess.cpu().numpy()
    r_ids, r_flags, r_ess = S.draw_segments(q, u, M, S.SCHEMES[scheme], S.ess_q16_of(tau))
    assert np.array_equal(flags, r_flags)
    assert np.array_equal(ids, r_ids)
    print(f"M={M} K={k} {scheme} tau={tau}: flags {flags.tolist()} max rel ESS error "
          f"{np.abs(ess - r_ess).max() / max(float(r_ess.max()), 1.0):.2e}")
    assert np.allclose(ess, r_ess, rtol=1e-6, atol=0)
    assert (ids // k == np.repeat(np.arange(M), k)).all()                   # every id inside its own segment
    for m in range(M):
        seg, loc = q[m * k:(m + 1) * k], ids[m * k:(m + 1) * k] - m * k
        if not flags[m]:
            assert np.array_equal(loc, np.arange(k))
            continue
        assert (seg[loc] > 0).all()                                         # a zero weight is never drawn
        if scheme != "multinomial":
            assert (np.diff(loc) >= 0).all()
            lo, hi = S.count_bounds(seg, S.SCHEMES[scheme])
            n = S.counts(loc, k)
            assert (n >= lo).all() and (n <= hi).all()
        if scheme == "systematic":                                          # the best particle(s) survive
            assert (S.counts(loc, k)[seg == R.TWO24] >= 1).all()
    if tau == 1.0 and k >= 5:                                               # the case resamples somewhere
        assert flags.any()
    # without the optional outputs: the same ids
    assert np.array_equal(K.resample_draw(_dev(d), _dev(u), M, INV, scheme=scheme, ess=tau).cpu().numpy(), ids)


# ----------------------------------------------------------------- 2: 128-bit products
def test_products_beyond_64_bits(K):
    """K = 4096 with every q_i within a few thousand units of 2^24: T ~ 2^36, T * (j 2^24 + ui) ~ 2^72, T^2 * 65536 ~ 2^88"""
    M, k = 2, 4096
    rng = np.random.RandomState(11)
    d = (50.0 + 1e-3 * rng.randn(M, k)).astype(np.float32)
    u = rng.rand(M, k).astype(np.float32)
    for m in range(M):                                                      # on the CPU first: not a flat segment
        q_ref = R.weights(d[m], np.float32(INV))
        assert q_ref.min() != q_ref.max() and q_ref.min() > R.TWO24 - 10000
    for scheme in ("stratified", "systematic"):
        ids, q, flags, _ = K.resample_draw(_dev(d), _dev(u), M, INV, want_weights=True, scheme=scheme, want_flags=True)
        q = q.cpu().numpy()
        assert q.min() > R.TWO24 - 10000 and int(q[:k].astype(np.int64).sum()) > (1 << 36) - (1 << 26)
        r_ids, r_flags, _ = S.draw_segments(q, u, M, S.SCHEMES[scheme])
        assert r_flags.all() and np.array_equal(flags.cpu().numpy(), r_flags)
        assert np.array_equal(ids.cpu().numpy(), r_ids)       # (nearly flat weights: close to the identity, by the count bounds)
        ids9, flags9, _ = K.resample_draw(_dev(d), _dev(u), M, INV, scheme=scheme, ess=0.999, want_flags=True)
        r_ids9, r_flags9, _ = S.draw_segments(q, u, M, S.SCHEMES[scheme], S.ess_q16_of(0.999))
        assert np.array_equal(flags9.cpu().numpy(), r_flags9) and np.array_equal(ids9.cpu().numpy(), r_ids9)


# ----------------------------------------------------------------- 3: the threshold boundary
@pytest.mark.parametrize("k", [2, 16, 512])
def test_threshold_boundary(K, k):
    rng = np.random.RandomState(77 + k)
    d, u = (50.0 + 30.0 * rng.randn(k)).astype(np.float32), rng.rand(k).astype(np.float32)      # no ties: not flat
    dd, uu = _dev(d), _dev(u)
    _, q = K.resample_draw(dd, uu, 1, INV, want_weights=True)
    q = q.cpu().numpy()
    star = S.min_trigger(q)                     # a non-flat segment has T^2 < K S2, so 1 <= star <= 65536
    assert not (q == q[0]).all() and 1 <= star <= 65536
    seen = []
    for e in (star - 1, star, min(star + 1, 65536)):
        rc, ids, q_e, flags, _ = _raw_draw(dd, uu, 1, k, S.SYSTEMATIC, e)
        assert rc == 0 and np.array_equal(q_e.cpu().numpy(), q)
        assert bool(flags.item()) == S.need(q, e)
        assert np.array_equal(ids.cpu().numpy(), S.draw(q, u, S.SYSTEMATIC, e))
        seen.append(int(flags.item()))
    print(f"K={k}: the smallest ess_q16 that triggers is {star} (ESS / K = {float(S.ess(q)) / k:.4f})")
    assert seen == [0, 1, 1]


# ----------------------------------------------------------------- 4: the defaults' bits
@pytest.mark.parametrize("M,k", [(1, 8), (3, 5), (2, 512)])
def test_scheme_0_tau_1_equals_the_plain_entry_points(K, M, k):
    d, u = D._case(M, k, 13 * M + k)
    dd, uu = _dev(d), _dev(u)
    x = D._particles(M * k, (3, 16, 16), 3 * k)
    ids, q = K.resample_draw(dd, uu, M, INV, want_weights=True)
    ids_n, q_n, flags, _ = K.resample_draw(dd, uu, M, INV, want_weights=True, ess=1.0, want_flags=True)
    assert torch.equal(ids_n, ids) and torch.equal(q_n, q)
    dst, d_out, ids_f, q_f = K.resample(x, dd, uu, M, INV, want_weights=True)
    dst_n, d_n, ids_fn, q_fn, flags_f, _ = K.resample(x, dd, uu, M, INV, want_weights=True, ess=1.0, want_flags=True)
    assert torch.equal(ids_fn, ids_f) and torch.equal(q_fn, q_f) and torch.equal(dst_n, dst)
    assert torch.equal(d_n.view(torch.int32), d_out.view(torch.int32)) and torch.equal(flags_f, flags)
    qn = q.cpu().numpy().reshape(M, k)
    assert flags.tolist() == [int(not (qn[m] == qn[m, 0]).all()) for m in range(M)]       # the flat rule


def test_wrapper_defaults_call_the_plain_symbols(K, monkeypatch):
    from dps_ttc_amd import _lib
    L = _lib.lib()
    called = []
    for name in ("dpsx_resample_draw_seg_f32", "dpsx_resample_seg_f32", "dpsx_resample_draw_seg_ex_f32",
                 "dpsx_resample_seg_ex_f32"):
        def spy(*a, _fn=getattr(L, name), _name=name):
            called.append(_name)
            return _fn(*a)
        monkeypatch.setattr(L, name, spy)
    d, u, x = torch.rand(6, device=DEV) * 90, torch.rand(6, device=DEV), torch.rand(6, 4, device=DEV)
    K.resample_draw(d, u, 2, INV)
    K.resample_draw(d, u, 2, INV, want_weights=True, scheme="multinomial", ess=None, want_flags=False)
    K.resample(x, d, u, 2, INV)
    assert called == ["dpsx_resample_draw_seg_f32"] * 2 + ["dpsx_resample_seg_f32"]
    del called[:]
    K.resample_draw(d, u, 2, INV, scheme="stratified")
    K.resample_draw(d, u, 2, INV, ess=1.0)
    K.resample_draw(d, u, 2, INV, want_flags=True)
    K.resample(x, d, u, 2, INV, scheme="systematic", ess=0.5)
    assert called == ["dpsx_resample_draw_seg_ex_f32"] * 3 + ["dpsx_resample_seg_ex_f32"]


def test_refusals(K):
    from dps_ttc_amd import _lib
    d, u = torch.rand(8, device=DEV), torch.rand(8, device=DEV)
    for scheme, e in ((3, 65536), (-1, 65536), (0, -1), (2, 65537)):
        assert _raw_draw(d, u, 1, 8, scheme, e)[0] == _lib.EINVAL
    x, dst = torch.rand(8, 4, device=DEV), torch.empty(8, 4, device=DEV)
    ids, d_out = torch.empty(8, dtype=torch.int64, device=DEV), torch.empty(8, device=DEV)

    def fused(src, dst, d_out, scheme=2, e=32768, n=8):
        return _lib.lib().dpsx_resample_seg_ex_f32(_lib.ptr(d), _lib.ptr(u), 1, 8, INV, _lib.ptr(src), _lib.ptr(dst),
                                                   _lib.ptr(d_out), _lib.ptr(ids), None, n, 4, scheme, e, None, None, None)
    assert fused(x, dst, d_out) == _lib.OK                                  # both diagnostics are nullable
    assert fused(x, dst, d_out, scheme=3) == _lib.EINVAL and fused(x, dst, d_out, e=65537) == _lib.EINVAL
    assert fused(x, x, d_out) == _lib.EINVAL and fused(x, dst, d) == _lib.EINVAL and fused(x, dst, d_out, n=9) == _lib.EINVAL
    with pytest.raises(_lib.DpsxError):                                     # K = 4097: above the LDS CDF's cap
        K.resample_draw(torch.rand(4097, device=DEV), torch.rand(4097, device=DEV), 1, INV, scheme="systematic")
    with pytest.raises(ValueError):
        K.resample_draw(d, u, 1, INV, scheme="residual")
    with pytest.raises(ValueError):
        K.resample(x, d, u, 1, INV, ess=1.5)
    torch.cuda.synchronize()


# ----------------------------------------------------------------- 5: the fused launch
@pytest.mark.parametrize("shape,unaligned", [((3, 64, 64), False), ((3, 63, 63), False), ((3, 64, 64), True)])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_fused_equals_draw_then_gather_and_image_by_image(K, scheme, shape, unaligned):
    M, k = 3, 5
    n = M * k
    d, u = D._case(M, k, 7 * n + shape[-1])
    d, u = _dev(d), _dev(u)
    x = D._particles(n, shape, n + shape[-1], unaligned)
    for tau in (1.0, 0.97):
        ids, q, flags, ess = K.resample_draw(d, u, M, INV, want_weights=True, scheme=scheme, ess=tau, want_flags=True)
        dst, d_out, ids_f, q_f, flags_f, ess_f = K.resample(x, d, u, M, INV, want_weights=True, scheme=scheme, ess=tau,
                                                            want_flags=True)
        assert torch.equal(ids_f, ids) and torch.equal(q_f, q) and torch.equal(flags_f, flags) and torch.equal(ess_f, ess)
        assert dst.shape == x.shape and torch.equal(dst, K.gather(x, ids))
        assert torch.equal(d_out.view(torch.int32), K.gather(d.reshape(n, 1), ids).reshape(n).view(torch.int32))
        dst2, d2, ids2 = K.resample(x, d, u, M, INV, scheme=scheme, ess=tau)       # without the optional outputs
        assert torch.equal(dst2, dst) and torch.equal(ids2, ids) and torch.equal(d2.view(torch.int32), d_out.view(torch.int32))
        for m in range(M):                                                  # one launch per image fed its slice of u
            sl = slice(m * k, (m + 1) * k)
            dst_m, d_m, ids_m, q_m, flags_m, ess_m = K.resample(x[sl], d[sl], u[sl], 1, INV, want_weights=True,
                                                                scheme=scheme, ess=tau, want_flags=True)
            assert torch.equal(ids[sl] - m * k, ids_m) and torch.equal(q[sl], q_m) and torch.equal(dst[sl], dst_m), m
            assert torch.equal(d_out[sl].view(torch.int32), d_m.view(torch.int32)), m
            assert torch.equal(flags[m:m + 1], flags_m) and torch.equal(ess[m:m + 1], ess_m), m
            assert torch.equal(ids[sl] - m * k, K.resample_draw(d[sl], u[sl], 1, INV, scheme=scheme, ess=tau)), m
    assert flags.tolist()[1] == 0                                           # the flat image in the middle
    assert not torch.equal(K.resample(x, d, u, M, INV, scheme=scheme)[2], torch.arange(n, device=DEV))


# ----------------------------------------------------------------- 6: bad uniforms, no finite distance
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bad_uniforms_and_a_segment_without_a_finite_distance(K, scheme):
    nan, inf = float("nan"), float("inf")
    d = torch.tensor([5.0, nan, 7.0, inf, nan, inf, -inf, nan], device=DEV)
    u = torch.tensor([nan, -3.0, 1.0, inf, -3.0, nan, inf, 1.0], device=DEV)
    x = torch.rand(8, 3, device=DEV)
    ids, q, flags, ess = K.resample_draw(d, u, 2, INV, want_weights=True, scheme=scheme, want_flags=True)
    r_ids, r_flags, _ = S.draw_segments(q.cpu().numpy(), u.cpu().numpy(), 2, S.SCHEMES[scheme])
    assert np.array_equal(ids.cpu().numpy(), r_ids) and flags.tolist() == r_flags.tolist() == [1, 0]
    assert ids[4:].tolist() == [4, 5, 6, 7] and set(ids[:4].tolist()) <= {0, 2}
    assert ess[1].item() == 0.0 and 1.0 <= ess[0].item() <= 2.0
    dst, d_out, ids_f, flags_f, _ = K.resample(x, d, u, 2, INV, scheme=scheme, want_flags=True)
    assert torch.equal(ids_f, ids) and torch.equal(flags_f, flags) and torch.equal(dst, x[ids])


# ----------------------------------------------------------------- 7: mean counts
@pytest.mark.parametrize("scheme", ["stratified", "systematic"])
def test_mean_counts_are_unbiased(K, scheme):
    M, k = S.MEAN_M, S.MEAN_K
    torch.manual_seed(0)
    u = torch.rand(M * k)
    d = torch.tensor(S.MEAN_D, dtype=torch.float32).repeat(M)
    ids, q, flags, _ = K.resample_draw(d.to(DEV), u.to(DEV), M, INV, want_weights=True, scheme=scheme, want_flags=True)
    assert bool(flags.all())
    err = S.mean_count_error(ids.cpu().numpy(), q.cpu().numpy(), M, k)
    bound = S.MEAN_BOUND[S.SCHEMES[scheme]]
    print(f"{scheme}: max |mean n_i - K q_i / T| = {err:.4f} (bound {bound:.4f})")
    assert err <= bound


# ----------------------------------------------------------------- 8: graph capture
HIP_GRAPH_NODE_TYPE_KERNEL = 0                  # hipGraphNodeTypeKernel


def _graph_node_types(graph):
    """the node types (hipGraphNodeType) of a torch.cuda.CUDAGraph captured with keep_graph=True, read from the HIP
    runtime that torch itself loaded"""
    import ctypes
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    handle = ctypes.c_void_p(int(graph.raw_cuda_graph()))
    count = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(handle, None, ctypes.byref(count)) == 0
    nodes = (ctypes.c_void_p * max(count.value, 1))()
    assert hip.hipGraphGetNodes(handle, nodes, ctypes.byref(count)) == 0
    types = []
    for i in range(count.value):
        t = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(nodes[i], ctypes.byref(t)) == 0
        types.append(t.value)
    return types


def test_fused_launch_captures_into_a_graph(K):
    M, k, shape = 4, 16, (3, 64, 64)
    n = M * k
    gen = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((n,) + shape, device=DEV, generator=gen)
    d, u = torch.empty(n, device=DEV), torch.empty(n, device=DEV)

    def fill(seed):
        g = torch.Generator(device=DEV).manual_seed(seed)
        d.copy_(torch.rand(n, device=DEV, generator=g) * 800)          # spread out: ESS / K around 1/4, below tau = 0.5
        d[k:2 * k] = 12.5                                               # ... and a flat one never resamples
        u.copy_(torch.rand(n, device=DEV, generator=g))

    def step():
        return K.resample(x, d, u, M, INV, want_weights=True, scheme="systematic", ess=0.5, want_flags=True)
    fill(0)
    step()                                       # warm-up
    graph, side = torch.cuda.CUDAGraph(keep_graph=True), torch.cuda.Stream()     # keep_graph: the captured graph stays readable
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = step()
    torch.cuda.current_stream().wait_stream(side)
    types = _graph_node_types(graph)
    print("node types of the captured graph:", types)
    assert types == [HIP_GRAPH_NODE_TYPE_KERNEL]          # ONE launch: no copy, no memset, no second kernel
    seen = []
    for seed in (1, 2):
        fill(seed)
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref = step()
        assert all(torch.equal(a, b) for a, b in zip(out, ref)), seed
        seen.append(out[4].tolist())
        assert out[4][1].item() == 0
    print("flags of the two replays:", seen)
    assert any(any(f) for f in seen)


# ----------------------------------------------------------------- 9: loops
def _ttc_inputs(M, k, hw, steps):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    n = M * k
    gen = torch.Generator(device=DEV).manual_seed(29)
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    y = torch.cat([op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
    x0 = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
    bank = torch.randn(steps, n, 3, hw, hw, device=DEV, generator=torch.Generator(device=DEV).manual_seed(31))
    ubank = torch.rand(steps, n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(37))
    return cm, y.contiguous(), x0, bank, ubank


def _ttc_run(cm, model, x, yy, bank, ubank, offset, respacing, resamples, **attrs):
    smp = D._sampler("ttc_ddim", respacing)
    smp.resample_draw = "device"
    for name, value in attrs.items():
        setattr(smp, name, value)
    it = D._patch_rng(smp, bank, ubank, offset)
    seen, flags = [], []
    orig = smp._resample

    def spy(*a, **kw):
        r = orig(*a, **kw)
        seen.append(smp.last_resample_ids.clone())
        flags.append(None if smp.last_resample_flags is None else smp.last_resample_flags.clone())
        return r
    smp._resample = spy
    img, dist = smp.p_sample_loop(model=model, x_start=x.clone(), measurement=yy, measurement_cond_fn=cm.conditioning,
                                  record=False, save_root=None)
    assert it["u"] == resamples and len(seen) == resamples
    return img, dist, torch.stack(seen), flags, smp


@pytest.mark.parametrize("tau,spread", [(0.5, False), (1.0, False), (0.95, True)])
def test_ttc_ddim_loop_multi_image(K, tau, spread):
    """spread: image 0's particles start at constant offsets 0 / 0.5 / 1.5 / 4, so its x0_hat sit near 0, 0.5, 1, 1 and its
    distances near ||y||, 60, 110, 110 (weights exp(-d / 100): ESS / K about 0.87), while image 1 keeps the nearly flat
    weights of random starts (ESS / K above 0.9999): tau = 0.95 then separates the two images inside one launch"""
    M, k, hw, steps = 2, 4, 64, 6
    n = M * k
    cm, y, x0, bank, ubank = _ttc_inputs(M, k, hw, steps)
    if spread:
        x0 = x0.clone()
        x0[:k] = torch.tensor([0.0, 0.5, 1.5, 4.0], device=DEV).view(k, 1, 1, 1) + 0.1 * x0[:k]
    model = StandInModel().to(DEV)
    kw = dict(resample_scheme="systematic", resample_ess=tau, resample_every=2)
    img, dist, ids, flags, smp = _ttc_run(cm, model, x0, y, bank, ubank, 0, str(steps), 3, **kw)    # idx 4, 2, 0
    assert ids.shape == (3, n) and (ids // k == torch.arange(n, device=DEV) // k).all()
    assert all(f.shape == (M,) and f.dtype == torch.uint8 and f.device.type == "cuda" for f in flags)
    assert smp.last_resample_ess.shape == (M,) and bool((smp.last_resample_ess > 0).all())
    print(f"tau={tau} spread={spread}: flags per resampling step {[f.tolist() for f in flags]}, last ESS "
          f"{smp.last_resample_ess.tolist()}, ids {ids.tolist()}")
    for f, i in zip(flags, ids):                                            # an image that did not resample kept its order
        for m in range(M):
            if not f[m]:
                assert torch.equal(i[m * k:(m + 1) * k], torch.arange(m * k, (m + 1) * k, device=DEV))
    if tau == 1.0:                              # distinct distances: every image resamples at every resampling step (the
        assert all(bool(f.all()) for f in flags)                            # systematic draw may still keep every particle)
    if spread:                                  # one launch, two decisions: image 0 resamples, image 1 does not
        assert [1, 0] in [f.tolist() for f in flags]
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        img_m, dist_m, ids_m, flags_m, _ = _ttc_run(cm, model, x0[sl], y[m:m + 1], bank, ubank, m * k, str(steps), 3, **kw)
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m), m
        assert torch.equal(ids[:, sl] - m * k, ids_m), m
        assert [f[m].item() for f in flags] == [f[0].item() for f in flags_m], m


def test_ttc_ddim_explicit_defaults_equal_the_device_loop_and_tau_0_never_resamples(K):
    M, k, hw, steps = 2, 4, 64, 20
    n = M * k
    cm, y, x0, bank, ubank = _ttc_inputs(M, k, hw, steps)
    model = StandInModel().to(DEV)
    img, dist, ids, flags, _ = _ttc_run(cm, model, x0, y, bank, ubank, 0, "20", 2)                  # idx 10 and 0
    assert flags == [None, None]
    img_e, dist_e, ids_e, flags_e, _ = _ttc_run(cm, model, x0, y, bank, ubank, 0, "20", 2, resample_scheme="multinomial",
                                                resample_ess=1.0, resample_every=10)
    assert torch.equal(img_e, img) and torch.equal(dist_e, dist) and torch.equal(ids_e, ids)
    assert all(f is not None for f in flags_e)
    _, _, ids_0, flags_0, smp = _ttc_run(cm, model, x0, y, bank, ubank, 0, "20", 2, resample_ess=0.0)
    assert torch.equal(smp.last_resample_ids, torch.arange(n, device=DEV)) and (ids_0 == torch.arange(n, device=DEV)).all()
    assert smp.last_resample_flags.tolist() == [0] * M and all(f.tolist() == [0] * M for f in flags_0)


def test_sampler_refusals_name_the_option(K):
    from dps_ttc_amd.measurements import get_operator
    cm, y, x0, bank, ubank = _ttc_inputs(1, 2, 64, 3)
    model = StandInModel().to(DEV)

    def loop(**attrs):
        smp = D._sampler("ttc_ddim", "3")
        for name, value in attrs.items():
            setattr(smp, name, value)
        return smp.p_sample_loop(model=model, x_start=x0.clone(), measurement=y, measurement_cond_fn=cm.conditioning,
                                 record=False, save_root=None)
    with pytest.raises(ValueError, match=r"resample_scheme.*resample_draw"):
        loop(resample_scheme="systematic")
    with pytest.raises(ValueError, match=r"resample_ess.*resample_draw"):
        loop(resample_ess=0.5)
    with pytest.raises(NotImplementedError, match=r"resample_scheme.*global"):
        loop(resample_draw="device", resample_scheme="stratified", global_resample=True)
    with pytest.raises(ValueError, match="resample_every"):
        loop(resample_draw="device", resample_every=0)
    op = get_operator("super_resolution", in_shape=(1, 3, 64, 64), scale_factor=4, device=DEV)
    with pytest.raises(ValueError, match=r"resample_scheme.*resample_draw"):
        D._sampler("search_ddpm", "3").resample_update(x0, x0, op, op.forward(x0[:1]).detach(), prev_costs=torch.rand(2, device=DEV),
                                                       resample_scheme="systematic")


def test_resample_update_multi_image(K):
    from dps_ttc_amd.measurements import get_operator
    M, k, hw = 3, 5, 64
    n = M * k
    gen = torch.Generator(device=DEV).manual_seed(43)
    op = get_operator("super_resolution", in_shape=(1, 3, hw, hw), scale_factor=4, device=DEV)
    y = torch.cat([op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
    cand = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
    den = torch.rand(n, 3, hw, hw, device=DEV, generator=gen) * 2 - 1
    prev = torch.rand(n, device=DEV, generator=gen) * 40
    prev[:k] = prev[:k] * 4                               # the first image: costs up to 160, weights down to e^-16: degenerate
    prev[k:2 * k] = prev[k:2 * k] * 0.05                  # the middle image: nearly flat weights, above tau = 0.5
    ubank = torch.rand(1, n, device=DEV, generator=gen)

    def run(c, dn, yy, pc, offset, **kw):
        smp = D._sampler("search_ddpm")
        smp.resample_draw, smp.resample_scheme, smp.resample_ess = "device", "systematic", 0.5
        D._patch_rng(smp, None, ubank, offset)
        out, net = smp.resample_update(c, dn, op, yy, rs_temp=0.1, prev_costs=pc, potential_type="min", steps_done=3, **kw)
        return out, net, smp.last_resample_ids, smp.last_curr_costs, smp.last_resample_flags, smp.last_resample_ess

    out, net, ids, curr, flags, ess = run(cand, den, y, prev, 0)
    r_ids, r_flags, r_ess = K.resample_draw(prev, ubank[0], M, 0.1, scheme="systematic", ess=0.5, want_flags=True)
    assert torch.equal(ids, r_ids) and torch.equal(flags, r_flags) and torch.equal(ess, r_ess)
    assert torch.equal(out, K.gather(cand, ids))
    print(f"flags {flags.tolist()} ESS {ess.tolist()}")
    assert flags[0].item() == 1 and bool((ids[:k] != torch.arange(k, device=DEV)).any())      # one launch, mixed decisions
    assert flags[1].item() == 0 and torch.equal(ids[k:2 * k], torch.arange(k, 2 * k, device=DEV))
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        out_m, net_m, ids_m, curr_m, flags_m, ess_m = run(cand[sl], den[sl], y[m:m + 1], prev[sl], m * k)
        assert torch.equal(out[sl], out_m) and torch.equal(net[sl], net_m) and torch.equal(curr[sl], curr_m), m
        assert torch.equal(ids[sl] - m * k, ids_m) and torch.equal(flags[m:m + 1], flags_m), m
        assert torch.equal(ess[m:m + 1], ess_m), m
    # the keywords select scheme and ESS as the attributes do
    smp = D._sampler("search_ddpm")
    D._patch_rng(smp, None, ubank, 0)
    out_k, net_k = smp.resample_update(cand, den, op, y, rs_temp=0.1, prev_costs=prev, potential_type="min", steps_done=3,
                                       resample_draw="device", resample_scheme="systematic", resample_ess=0.5)
    assert torch.equal(out_k, out) and torch.equal(net_k, net)


# ----------------------------------------------------------------- 10: driver
def test_driver_systematic_ess_images_per_batch(tmp_path):
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    tpath, dpath = D._setup(tmp_path)
    out = tmp_path / "out"
    drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
              "--task_config", tpath, "--n_paths", "2", "--batch_size", "2", "--timestep_respacing", "3", "--seed", "0",
              "--gpu", "0", "--resample_draw", "device", "--resample_scheme", "systematic", "--resample_ess", "0.5",
              "--ttc_resample_every", "1", "--save_dir", str(out), "--ref_image_idxs", "0,1", "--images_per_batch", "2"])
    (sub,) = os.listdir(out)
    root = out / sub
    for fname in ("00000", "00001"):
        assert (root / "input" / f"{fname}.png").exists() and (root / "label" / f"{fname}.png").exists()
        for k in (1, 2):
            assert (root / "recon_paths" / fname / f"path#{k}.png").exists()
            assert (root / "recon_paths_y" / fname / f"path#{k}_y_space.png").exists()
        d = np.load(root / f"{fname}_pathwise_distances.npy")
        assert d.shape == (2,) and np.isfinite(d).all() and (d > 0).all()
        assert (root / "best_of_n" / f"{fname}.png").exists()
