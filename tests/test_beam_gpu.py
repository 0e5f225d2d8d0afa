"""GPU suite: beam search for search_ddpm -- the segmented top-B select (dpsx_topk_seg_f32), the beam step
(dpsx_search_step_beam_f32) and SearchDDPM's beam loop.  Every comparison is exact (torch.equal / equal bit patterns):
the order is restated in tests/beam_ref.py, the step is composed from launches the rest of the suite pins (S1, the
scoring launch, the gather), and B = 1 is compared with the existing single-state and replicated steps."""
import numpy as np
import pytest
import torch

import beam_ref
from standin import StandInModel, synthetic_motion_kernel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def _sampler(name="search_ddpm", respacing=""):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing)


def _operator(name, c, h, w, M, seed=0):
    """-> (operator, per-image masks [M,1,H,W] or None)"""
    from dps_ttc_amd.measurements import get_operator
    if name == "gauss9":
        return get_operator("gaussian_blur", kernel_size=9, intensity=1.0, device=DEV), None
    if name == "motion":
        op = get_operator("motion_blur", kernel_size=61, intensity=0.5, device=DEV)
        op._set_weights(synthetic_motion_kernel(61, 3))
        return op, None
    if name == "sr4":
        return get_operator("super_resolution", in_shape=(1, c, h, w), scale_factor=4, device=DEV), None
    if name in ("inpaint", "mask1"):       # one mask per image / one mask for all
        masks = (np.random.RandomState(seed).rand(1 if name == "mask1" else M, 1, h, w) < 0.5).astype(np.float32)
        return get_operator("inpainting", device=DEV), torch.from_numpy(masks).to(DEV)
    raise KeyError(name)


def _handle(op, masks, x):
    return op.hip_handle_for(masks) if masks is not None else op.hip_handle(x)


def _measurements(op, masks, M, c, h, w, gen):
    ys = []
    for m in range(M):
        fkw = {} if masks is None else {"mask": masks[min(m, masks.shape[0] - 1):][:1]}
        ys.append(op.forward(torch.rand(1, c, h, w, device=DEV, generator=gen) * 2 - 1, **fkw).detach())
    return torch.cat(ys).contiguous()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """equal bit patterns (NaN costs included)"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ----------------------------------------------------------------- 1, 2: the select
CASES = [(1, 1, 1), (1, 5, 2), (3, 64, 4), (2, 1000, 7), (1, 4096, 4096), (1, 4096, 1), (4, 96, 96)]
SPECIALS = [NAN, INF, -INF, -0.0, 0.0, NAN, NAN]


def _vectors(segments, L):
    """the four cost vectors of a case, [segments * L] each.  `special`: random values with three NaNs, +inf, -inf, -0.0
    and +0.0 spread over every segment (a segment shorter than seven holds the first L of them)"""
    g = torch.Generator().manual_seed(1000 * segments + L)
    rnd = torch.randn(segments, L, generator=g)
    special = torch.randn(segments, L, generator=g).round()            # rounded: ties between ordinary values too
    pos = [(j * L) // len(SPECIALS) for j in range(len(SPECIALS))] if L >= len(SPECIALS) else list(range(L))
    for m in range(segments):
        for j, p in enumerate(pos):
            special[m, (p + m) % L] = SPECIALS[j]
    desc = torch.arange(segments * L, 0, -1, dtype=torch.float32).reshape(segments, L)
    return {"random": rnd, "equal": torch.full((segments, L), 2.5), "special": special, "descending": desc}


@pytest.mark.parametrize("segments,L,b", CASES)
def test_topk_seg_equals_the_restatement(K, segments, L, b):
    for kind, v in _vectors(segments, L).items():
        ref = torch.from_numpy(beam_ref.topb(v.numpy(), segments, b))
        idx, val = K.topk_seg(v.to(DEV), segments, b, want_value=True)
        assert idx.dtype == torch.int64 and idx.shape == (segments * b,)
        assert torch.equal(idx.cpu(), ref), f"{kind}: ids"
        assert _same(val.cpu(), v.reshape(-1)[ref]), f"{kind}: values"
        assert torch.equal(K.topk_seg(v.to(DEV), segments, b).cpu(), ref), f"{kind}: ids without the values"


def test_topk_seg_refusals(K):
    from dps_ttc_amd import _lib
    v = torch.zeros(4097, device=DEV)
    with pytest.raises(_lib.DpsxError) as e:
        K.topk_seg(v, 1, 1)
    assert e.value.code == _lib.EUNSUPPORTED
    for b in (0, 9):
        with pytest.raises(_lib.DpsxError) as e:
            K.topk_seg(v[:16], 2, b)
        assert e.value.code == _lib.EINVAL


@pytest.mark.parametrize("segments,L,b", CASES)
def test_topk_seg_b1_equals_argmin_seg(K, segments, L, b):
    for kind, v in _vectors(segments, L).items():
        v = v.to(DEV)
        i1, v1 = K.topk_seg(v, segments, 1, want_value=True)
        i0, v0 = K.argmin_seg(v, segments, want_value=True)
        assert torch.equal(i1, i0) and _same(v1, v0), kind


# ----------------------------------------------------------------- 3: B = 1 is the existing steps
@pytest.mark.parametrize("name", ["gauss9", "mask1"])
def test_beam_one_equals_the_existing_steps(K, name):
    n, M, c, hw = 8, 2, 3, 64
    gen = torch.Generator(device=DEV).manual_seed(31)
    mk = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    op, masks = _operator(name, c, hw, hw, M)
    x, mo, z = mk(n, c, hw, hw), mk(n, 2 * c, hw, hw) * 0.4, mk(n, c, hw, hw)
    x1, mo1 = x[:M].contiguous(), mo[:M].contiguous()
    y = _measurements(op, masks, M, c, hw, hw, gen)
    ck = _sampler().step_coefs[400]
    h = _handle(op, masks, x)
    # one state per image, with the noise given and with the noise drawn in S1's launch
    ref = h.search_step_one(x1, mo1, z, y, ck, segments=M)
    got = h.search_step_beam(x1, mo1, z, y, ck, n=n, beam=1, segments=M)
    for a, b, what in zip(got, ref, ("winners", "sample", "costs", "best", "costs[best]")):
        assert a.shape == b.shape and torch.equal(a, b), f"noise=: {what}"
    rng = K.Rng(7, 3, K.Rng.TAG_STEP, 0, n // M)
    ref = h.search_step_one(x1, mo1, None, y, ck, segments=M, rng=rng, n=n)
    got = h.search_step_beam(x1, mo1, None, y, ck, n=n, beam=1, segments=M, rng=rng)
    for a, b, what in zip(got, ref, ("winners", "sample", "costs", "best", "costs[best]")):
        assert a.shape == b.shape and torch.equal(a, b), f"rng=: {what}"
    assert not torch.equal(got[1], h.search_step_beam(x1, mo1, z, y, ck, n=n, beam=1, segments=M)[1])
    # one state per particle
    _, smp, costs, best, val = h.search_step(x, mo, z, y, ck, replicate=False, segments=M)
    w, smp_b, costs_b, best_b, val_b = h.search_step_beam(x, mo, z, y, ck, n=n, beam=1, segments=M)
    assert torch.equal(smp_b, smp) and torch.equal(costs_b, costs) and torch.equal(best_b, best) and torch.equal(val_b, val)
    assert torch.equal(w, smp[best])


# ----------------------------------------------------------------- 4: the step is its launches
COMPOSE = [("gauss9", 3, 64, 64, 24, 3), ("motion", 3, 64, 64, 24, 3), ("sr4", 3, 64, 64, 24, 3), ("inpaint", 3, 64, 64, 24, 3),
           ("gauss9", 1, 33, 47, 12, 2)]        # the last: chw % 4 != 0 -- the scalar S1, gather and scoring loaders


@pytest.fixture(scope="module", params=COMPOSE, ids=lambda p: f"{p[0]}-{p[1]}x{p[2]}x{p[3]}")
def composed(request, K):
    """one beam step of M = 2 images per operator, computed once and left unchanged"""
    name, c, h, w, n, B = request.param
    M = 2
    S = M * B
    k = n // S
    gen = torch.Generator(device=DEV).manual_seed(41 + n)
    mk = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    op, masks = _operator(name, c, h, w, M)
    xs, ms, z = mk(S, c, h, w), mk(S, 2 * c, h, w) * 0.4, mk(n, c, h, w)
    y = _measurements(op, masks, M, c, h, w, gen)
    ck = _sampler().step_coefs[400]
    handle = _handle(op, masks, xs)
    out = handle.search_step_beam(xs, ms, z, y, ck, n=n, beam=B, segments=M)
    return dict(op=op, masks=masks, handle=handle, xs=xs, ms=ms, z=z, y=y, ck=ck, n=n, B=B, M=M, k=k, out=out,
                shape=(c, h, w))


def test_beam_step_shapes(composed):
    d = composed
    winners, sample, costs, best, val = d["out"]
    assert winners.shape == (d["M"] * d["B"],) + d["shape"] and sample.shape == (d["n"],) + d["shape"]
    assert costs.shape == (d["n"],) and best.shape == val.shape == (d["M"] * d["B"],) and best.dtype == torch.int64
    assert bool(torch.isfinite(costs).all()) and bool((costs > 0).all())


def test_beam_step_sample_is_s1_on_the_repeated_states(K, composed):
    d = composed
    _, ref = K.posterior_fwd(d["xs"].repeat_interleave(d["k"], 0), d["ms"].repeat_interleave(d["k"], 0), d["z"], d["ck"],
                             want_x0=False)
    assert torch.equal(d["out"][1], ref)


def test_beam_step_costs_are_the_scoring_launch(composed):
    d = composed
    assert torch.equal(d["out"][2], d["handle"].score(d["out"][1], d["y"]))


def test_beam_step_ids_winners_and_values(composed):
    d = composed
    winners, sample, costs, best, val = d["out"]
    ref = torch.from_numpy(beam_ref.topb(costs.cpu().numpy(), d["M"], d["B"])).to(DEV)
    assert torch.equal(best, ref)
    assert torch.equal(winners, sample[best]) and torch.equal(val, costs[best])
    per = d["n"] // d["M"]
    assert all(m * per <= int(i) < (m + 1) * per for m in range(d["M"]) for i in best[m * d["B"]:(m + 1) * d["B"]])


def test_beam_step_tie_takes_the_lower_index(composed):
    d = composed
    per = d["n"] // d["M"]
    z = d["z"].clone()
    z[1] = z[0]                                   # proposals 0 and 1 share a state (k >= 2) and now their noise
    z[per + 2] = z[per + 1]
    _, sample, costs, best, _ = d["handle"].search_step_beam(d["xs"], d["ms"], z, d["y"], d["ck"], n=d["n"], beam=per,
                                                             segments=d["M"])
    assert d["k"] >= 3 and torch.equal(sample[0], sample[1]) and _same(costs[0:1], costs[1:2])
    assert _same(costs[per + 1:per + 2], costs[per + 2:per + 3])
    order = best.tolist()
    assert order.index(1) == order.index(0) + 1 and order.index(per + 2) == order.index(per + 1) + 1
    assert order == beam_ref.topb(costs.cpu().numpy(), d["M"], per).tolist()


def test_beam_step_nan_ranks_first_and_stays_in_its_particle(composed):
    d = composed
    per, bad = d["n"] // d["M"], 5
    z = d["z"].clone()
    z[bad] = NAN
    _, sample, costs, best, val = d["handle"].search_step_beam(d["xs"], d["ms"], z, d["y"], d["ck"], n=d["n"], beam=d["B"],
                                                               segments=d["M"])
    assert bool(torch.isnan(costs[bad])) and int(best[0]) == bad and bool(torch.isnan(val[0]))
    keep = torch.arange(d["n"], device=DEV) != bad
    assert torch.equal(costs[keep], d["out"][2][keep]) and torch.equal(sample[keep], d["out"][1][keep])
    assert torch.equal(best[d["B"]:], d["out"][3][d["B"]:])                  # the other image's select is untouched
    assert best.tolist() == beam_ref.topb(costs.cpu().numpy(), d["M"], d["B"]).tolist()


# ----------------------------------------------------------------- 5: images do not see each other
@pytest.mark.parametrize("draw", ["noise", "rng"])
def test_beam_step_two_images_equal_two_calls(K, composed, draw):
    d = composed
    M, B, n, k = d["M"], d["B"], d["n"], d["k"]
    per = n // M
    if draw == "rng":
        full = d["handle"].search_step_beam(d["xs"], d["ms"], None, d["y"], d["ck"], n=n, beam=B, segments=M,
                                            rng=K.Rng(11, 2, K.Rng.TAG_STEP, 0, per))
    else:
        full = d["out"]
    for m in range(M):
        ss, sl = slice(m * B, (m + 1) * B), slice(m * per, (m + 1) * per)
        xs, ms = d["xs"][ss].contiguous(), d["ms"][ss].contiguous()
        hm = _handle(d["op"], None if d["masks"] is None else d["masks"][m:m + 1], xs)
        kw = dict(rng=K.Rng(11, 2, K.Rng.TAG_STEP, 0, 0)) if draw == "rng" else {}
        part = hm.search_step_beam(xs, ms, None if draw == "rng" else d["z"][sl].contiguous(), d["y"][m:m + 1], d["ck"],
                                   n=per, beam=B, **kw)
        assert torch.equal(full[0][ss], part[0]) and torch.equal(full[1][sl], part[1]) and torch.equal(full[2][sl], part[2])
        assert torch.equal(full[3][ss] - m * per, part[3]) and torch.equal(full[4][ss], part[4])


# ----------------------------------------------------------------- 6: graph capture
def test_beam_step_captures_into_a_graph(composed):
    d = composed

    def step():
        return d["handle"].search_step_beam(d["xs"], d["ms"], d["z"], d["y"], d["ck"], n=d["n"], beam=d["B"],
                                            segments=d["M"])
    ref = [t.clone() for t in step()]            # eager (also the warm-up: workspace, kernel attributes)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            out = step()
    torch.cuda.current_stream().wait_stream(side)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, ref))
    assert all(torch.equal(a, b) for a, b in zip(ref, d["out"]))


# ----------------------------------------------------------------- 7: the loop
STEPS, HW = 6, 64


def _patch_randn(smp, bank):
    """the sampler's noise: the bank's next step (the first rows of it, for a draw of fewer particles)"""
    it = {"k": 0}

    def rnd(like, stride=None, shape=None):
        cnt = (tuple(shape) if shape is not None else tuple(like.shape))[0]
        z = bank[it["k"], :cnt].contiguous()
        it["k"] += 1
        return z
    smp._randn = rnd


def _loop_inputs(M, n):
    from dps_ttc_amd.measurements import get_operator
    gen = torch.Generator(device=DEV).manual_seed(51 + M)
    op = get_operator("gaussian_blur", kernel_size=9, intensity=1.0, device=DEV)
    y = _measurements(op, None, M, 3, HW, HW, gen)
    x0 = torch.randn(n, 3, HW, HW, device=DEV, generator=gen)
    bank = torch.randn(STEPS, n, 3, HW, HW, device=DEV, generator=gen)
    return op, y, x0, bank, StandInModel().to(DEV)


@pytest.mark.parametrize("M,n", [(1, 12), (2, 24)])
def test_beam_loop_equals_its_steps(M, n):
    B = 3
    k = n // M // B
    op, y, x0, bank, model = _loop_inputs(M, n)
    kw = {} if M == 1 else {"n_images": M}
    smp = _sampler(respacing=str(STEPS))
    assert smp.num_timesteps == STEPS
    smp.beam_width = B
    _patch_randn(smp, bank)
    bests, inner = [], smp.search_step_beam

    def spy(*a, **k_):
        r = inner(*a, **k_)
        bests.append((smp.last_best.clone(), smp.last_parents.clone()))
        return r
    smp.search_step_beam = spy
    out = smp.p_sample_loop(model=model, x_start=x0.clone(), measurement=y, measurement_cond_fn=None, record=False,
                            save_root=None, operator=op, trace=True, **kw)
    torch.cuda.synchronize()
    # the same steps by hand
    handle, ref = op.hip_handle(x0), _sampler(respacing=str(STEPS))
    state = x0
    for j, idx in enumerate(range(STEPS - 1, -1, -1)):
        with torch.no_grad():
            mo = ref._call_model(model, state, idx)
        # the step without noise (the last one) proposes once per state: K equal proposals would fill the beam with copies
        n_j = n if ref.step_coefs[idx].add_noise & 1 else state.shape[0]
        per_j, k_j = n_j // M, max(n_j // M // B, 1)
        state, _, costs, best, val = handle.search_step_beam(state, mo, bank[j, :n_j].contiguous(), y, ref.step_coefs[idx],
                                                             n=n_j, beam=B, segments=None if M == 1 else M)
        assert torch.equal(smp.best_costs[j], costs), f"step {j}: costs"
        assert torch.equal(bests[j][0], best), f"step {j}: ids"
        assert best.tolist() == beam_ref.topb(costs.cpu().numpy(), M, B).tolist(), f"step {j}: ids against the order"
        assert torch.equal(bests[j][1], (best % per_j) // k_j), f"step {j}: parents"
    assert n_j == M * B and [int(c.numel()) for c in smp.best_costs] == [n] * (STEPS - 1) + [M * B]
    assert len(bests) == STEPS and smp.last_best.shape == (M * B,)
    assert torch.equal(smp.last_parents, smp.last_best % B)
    assert bool((smp.last_parents >= 0).all()) and bool((smp.last_parents < B).all())
    assert torch.equal(smp.beam_states, state) and torch.equal(smp.beam_costs, val)
    assert smp.beam_states.shape == (M * B, 3, HW, HW)
    for m in range(M):
        rows = smp.beam_states[m * B:(m + 1) * B]
        assert all(not torch.equal(rows[i], rows[j]) for i in range(B) for j in range(i + 1, B))
    assert out.shape == x0.shape and torch.equal(out, smp.beam_states.repeat_interleave(k, 0))


@pytest.mark.parametrize("M,n", [(1, 12), (2, 24)])
def test_beam_width_one_is_the_greedy_loop(M, n):
    per = n // M
    op, y, x0, bank, model = _loop_inputs(M, n)
    kw = {} if M == 1 else {"n_images": M}
    seg = None if M == 1 else M
    smp = _sampler(respacing=str(STEPS))
    smp.beam_width = 1
    _patch_randn(smp, bank)
    out = smp.p_sample_loop(model=model, x_start=x0.clone(), measurement=y, measurement_cond_fn=None, record=False,
                            save_root=None, operator=op, **kw)
    handle, ref = op.hip_handle(x0), _sampler(respacing=str(STEPS))
    with torch.no_grad():
        mo = ref._call_model(model, x0, STEPS - 1)
    x_next = handle.search_step(x0, mo, bank[0], y, ref.step_coefs[STEPS - 1], segments=seg)[0]
    state = x_next[::per].contiguous()
    for j, idx in enumerate(range(STEPS - 2, -1, -1), start=1):
        with torch.no_grad():
            mo = ref._call_model(model, state, idx)
        state = handle.search_step_one(state, mo, bank[j], y, ref.step_coefs[idx], segments=seg)[0]
    assert torch.equal(out, state.repeat_interleave(per, 0))


# ----------------------------------------------------------------- 8: keep all
def test_beam_keep_all_sorts_the_proposals(K):
    n, M, c, hw = 8, 2, 3, 64
    L = n // M
    gen = torch.Generator(device=DEV).manual_seed(61)
    mk = lambda *shape: torch.randn(*shape, device=DEV, generator=gen)
    op, _ = _operator("gauss9", c, hw, hw, M)
    x, mo, z = mk(n, c, hw, hw), mk(n, 2 * c, hw, hw) * 0.4, mk(n, c, hw, hw)
    y = _measurements(op, None, M, c, hw, hw, gen)
    h = op.hip_handle(x)
    winners, sample, costs, best, val = h.search_step_beam(x, mo, z, y, _sampler().step_coefs[400], n=n, beam=L, segments=M)
    assert winners.shape == sample.shape and torch.equal(winners, sample[best]) and torch.equal(val, costs[best])
    for m in range(M):
        ids = best[m * L:(m + 1) * L]
        assert sorted(ids.tolist()) == list(range(m * L, (m + 1) * L))
        assert bool((val[m * L:(m + 1) * L].diff() >= 0).all())
    assert best.tolist() == beam_ref.topb(costs.cpu().numpy(), M, L).tolist()
