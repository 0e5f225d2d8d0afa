"""GPU suite of particle repulsion (dpsx_pairwise_sqdist_f32, dpsx_repulse_f32, the samplers' repulsion_scale).  The
distances, the bandwidth, the weights and the displacement are compared with the float64 restatement tests/repulse_ref.py
inside the bounds stated at each test; the copies, the batch / NaN properties, the graph replay, the stream argument and
the loops bit for bit (torch.equal).

Shapes (M images x K particles x shape), each reaching one code path: 1 x 3 x 3 x 64 x 64 (float4 units); 2 x 2 x
1 x 33 x 47 (scalar units, the second particle's base unaligned, a ragged last block); 1 x 4 x 3 x 256 x 256 (the full slot
count, 192); 3 x 16 x 3 x 32 x 32 (several images, three tile pairs); 1 x 65 x 1 x 16 x 16 (K crosses a tile of 8 and of 64,
odd, a ragged last tile); 1 x 512 x 1 x 8 x 8 (the cap: 2080 tile pairs, one slot, a quarter of a wave at work);
1 x 1 x 3 x 64 x 64 (K = 1)."""
import numpy as np
import pytest
import torch

import repulse_ref as R
from standin import StandInModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"f4": (1, 3, (3, 64, 64)), "odd": (2, 2, (1, 33, 47)), "slots": (1, 4, (3, 256, 256)),
          "multi": (3, 16, (3, 32, 32)), "k65": (1, 65, (1, 16, 16)), "cap": (1, 512, (1, 8, 8))}
BW = 2.0                 # the fixed bandwidth: the mean squared per-element difference of two N(0, 1) particles
C_REL = {"rand": 0.25, "img": 0.25, "far": 0.25, "neardup": 25.0}      # the strength as a multiple of h (see the test)


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


_X, _D2 = {}, {}


def _x(key, name):
    if (key, name) not in _X:
        m, k, shape = SHAPES[key]
        _X[key, name] = R.make_set(name, m, k, shape, seed=11 + len(_X))
    return _X[key, name]


def _d2(key, name):
    """the float64 distances of a set, computed once"""
    if (key, name) not in _D2:
        _D2[key, name] = R.sqdist(_x(key, name), SHAPES[key][0])
    return _D2[key, name]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _rel(got, ref):
    """max |got - ref| / ref over the entries with ref != 0 (0 where there are none)"""
    nz = ref != 0
    return float((np.abs(got.astype(np.float64) - ref)[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0


# ----------------------------------------------------------------- 1: distances, bandwidth
@pytest.mark.parametrize("key", list(SHAPES))
def test_distances_against_the_restatement(K, key):
    """|d2 - ref| <= 1e-5 ref on every set (per term at most three roundings, at most 12 more in the block sum, 5 x margin:
    the bound the neardup set of test_repulse_cpu.py shows to reject the Gram form); symmetric, +0.0 on the diagonal and
    the dup pair exactly 0, bit for bit; h, mean and min within 1e-5 relative"""
    m, k, shape = SHAPES[key]
    for name in R.SETS:
        x, ref = _x(key, name), _d2(key, name)
        d2, info = K.pairwise_sqdist(dev(x), images=m, want_info=True)
        assert d2.shape == (m, k, k) and info.shape == (m, 4)
        d2, info = host(d2), host(info)
        err = _rel(d2, ref)
        print(f"{key} {name}: d2 max rel err {err:.3g}")
        assert np.isfinite(d2).all() and err <= 1e-5, (name, err)
        assert np.array_equal(d2.view(np.uint32), d2.transpose(0, 2, 1).copy().view(np.uint32)), name
        assert (np.einsum("mii->mi", d2).view(np.uint32) == 0).all(), name             # +0.0
        iu = np.triu_indices(k, 1)
        pairs = ref[:, iu[0], iu[1]]
        mean, mn = pairs.mean(axis=1), pairs.min(axis=1)
        if name == "dup":
            assert (d2[:, 0, k - 1].view(np.uint32) == 0).all() and (info[:, 3] == 0).all() and (ref[:, 0, k - 1] == 0).all()
        else:
            assert (d2[:, iu[0], iu[1]] > 0).all() and _rel(info[:, 3], mn) <= 1e-5, name
        assert _rel(info[:, 2], mean) <= 1e-5 and _rel(info[:, 0], mean / np.log(k + 1.0)) <= 1e-5, name
        assert (info[:, 1] == 0).all()


# ----------------------------------------------------------------- 2: weights, displacement
@pytest.mark.parametrize("bw", [None, BW])
@pytest.mark.parametrize("key", list(SHAPES))
def test_weights_and_displacement_against_the_restatement(K, key, bw):
    """w: |w - ref| <= (2e-5 u + 2e-7) ref + 2^-150, u = d2 / h: the two 1e-5 bounds on the exponent, one rounding to
    float32, and that rounding's absolute size where w is subnormal or underflows (u > 87: the far particle).
    Delta = out - x, per particle: ||Delta - ref|| <= 1e-4 ||ref|| + ||ulp(out_ref) / 2||.  The first term is the project's
    parity gate; the second is what the float32 grid of `out` alone costs a displacement recovered from it, and it matters
    only for a particle whose weights underflow (Delta_ref ~ 0 beside x = 50).  For the bound to bind everywhere else the
    strength is chosen per set as a multiple of h (C_REL) that makes Delta a few per cent of x or more: 0.25 h moves a
    particle by about half its distance from the image's mean, and neardup (spread 1e-3) takes 25 h.
    Also: sum_i Delta_i is within 1e-5 of sum_i ||Delta_i||, and the info record matches."""
    m, k, shape = SHAPES[key]
    dim = int(np.prod(shape))
    iu = np.triu_indices(k, 1)
    for name in ("rand", "img", "neardup", "far"):
        x, d2 = _x(key, name), _d2(key, name)
        h = BW * dim if bw else float(d2[0][iu].mean() / np.log(k + 1.0))
        c = float(np.float32(C_REL[name] * h))
        ref = R.repulse(x, c, images=m, bandwidth=bw)
        assert ref["applied"].all()
        out, rec = K.repulse(dev(x), c, images=m, bandwidth=bw, want_info=True)
        out, w, info = host(out).astype(np.float64), host(rec["w"]), host(rec["info"])
        assert np.array_equal(host(rec["d2"]), host(K.pairwise_sqdist(dev(x), images=m)))
        assert (host(rec["applied"]) == 1).all() and _rel(info[:, :3], ref["info"][:, :3]) <= 1e-5, name
        # the weights
        u = ref["d2"] / ref["info"][:, 0][:, None, None]
        tol = (2e-5 * u + 2e-7) * ref["w"] + 2.0 ** -150
        werr = np.abs(w.astype(np.float64) - ref["w"])
        print(f"{key} {name} bw={bw}: w worst err / tol {float((werr / tol).max()):.3g}, u max {float(u.max()):.3g}")
        assert (werr <= tol).all(), name
        assert np.array_equal(w.view(np.uint32), w.transpose(0, 2, 1).copy().view(np.uint32))
        assert (np.einsum("mii->mi", w).view(np.uint32) == 0).all()
        # the displacement
        delta = (out - x.astype(np.float64)).reshape(m * k, -1)
        dref = ref["delta"].reshape(m * k, -1)
        floor = np.linalg.norm(0.5 * np.spacing(ref["out"].astype(np.float32)).astype(np.float64).reshape(m * k, -1), axis=1)
        err, nref = np.linalg.norm(delta - dref, axis=1), np.linalg.norm(dref, axis=1)
        # every particle with a neighbour inside the kernel's reach (a weight >= 1e-3) moves by 1 % of its norm or more: for
        # those the floor is nothing beside the first term
        moved = nref >= 1e-2 * np.linalg.norm(x.reshape(m * k, -1).astype(np.float64), axis=1)
        paired = ref["w"].max(axis=2).reshape(-1) >= 1e-3
        worst = float((err[moved] / nref[moved]).max()) if moved.any() else 0.0
        print(f"{key} {name} bw={bw}: Delta rel-L2 worst {worst:.3g} over {int(moved.sum())} of {m * k} particles")
        assert moved[paired].all() and (paired.any() or (name == "far" and k == 2)), name
        assert (err <= 1e-4 * nref + floor).all() and worst <= 1e-4, name
        per = delta.reshape(m, k, -1)
        total = np.linalg.norm(per.sum(axis=1), axis=1)
        assert (total <= 1e-5 * np.linalg.norm(per, axis=2).sum(axis=1)).all(), name
        if name == "far" and bw:                       # all weights of the far particle underflow: it stays where it is
            far = np.arange(m) * k + k - 1
            assert (w[:, k - 1] == 0).all() and np.array_equal(out[far], x[far].astype(np.float64))
        if name == "rand":                             # the push is repulsive: every pairwise distance grows
            grown = R.sqdist(out, m)
            assert (grown[:, iu[0], iu[1]] > d2[:, iu[0], iu[1]]).all()


def test_two_particles_closed_form(K):
    """K = 2: out_0 - out_1 = (x_0 - x_1) (1 + 2 gain w01), to 1e-5 of its norm; both scalar and float4 units"""
    for shape in ((1, 33, 47), (3, 64, 64)):
        x = R.make_set("rand", 1, 2, shape, seed=5)
        out, rec = K.repulse(dev(x), 0.3 * x[0].size, want_info=True)
        o, info, w = host(out).astype(np.float64), host(rec["info"]).astype(np.float64), host(rec["w"]).astype(np.float64)
        want = (x[0].astype(np.float64) - x[1]) * (1.0 + 2.0 * info[0, 1] * w[0, 0, 1])
        assert abs(w[0, 0, 1] - 1.0 / 3.0) < 1e-5 and info[0, 1] > 0
        assert np.linalg.norm((o[0] - o[1]) - want) <= 1e-5 * np.linalg.norm(want)


def test_zero_strength_and_underflow_give_x(K):
    x = dev(_x("multi", "rand"))
    out, rec = K.repulse(x, 0.0, images=3, want_info=True)
    assert torch.equal(out, x) and (rec["applied"] == 1).all() and (rec["info"][:, 1] == 0).all()
    out, rec = K.repulse(x, 1.0, images=3, bandwidth=1e-3, want_info=True)            # u = 2000: every weight is 0
    assert torch.equal(out, x) and (rec["w"] == 0).all() and (rec["applied"] == 1).all()


# ----------------------------------------------------------------- 3: copies, bit for bit
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_copies_are_bit_for_bit(K):
    # K = 1
    x = dev(R.make_set("rand", 1, 1, (3, 64, 64), seed=3))
    x[0, 0, 0, :2] = torch.tensor([-0.0, float("nan")], device=DEV)
    keep = x.clone()
    out, rec = K.repulse(x, 0.5, want_info=True)
    assert torch.equal(_bits(out), _bits(keep)) and torch.equal(_bits(x), _bits(keep))
    assert rec["applied"].tolist() == [0] and rec["info"][0, 1] == 0 and rec["info"][0, 3] == float("inf")
    assert rec["d2"].tolist() == [[[0.0]]] and rec["w"].tolist() == [[[0.0]]]
    d2 = K.pairwise_sqdist(x)
    assert d2.shape == (1, 1, 1) and d2.item() == 0
    # all particles equal, a -0.0 among their values: h = 0
    for shape in ((3, 32, 32), (1, 33, 47)):
        one = R.make_set("rand", 1, 1, shape, seed=4)
        one[0, 0, 0, 0] = -0.0
        x = dev(np.repeat(one, 5, axis=0))
        keep = x.clone()
        out, rec = K.repulse(x, 0.5, want_info=True)
        assert torch.equal(_bits(out), _bits(keep)) and torch.equal(_bits(x), _bits(keep))
        assert rec["applied"].tolist() == [0] and (rec["d2"] == 0).all() and (rec["w"] == 0).all()
        assert rec["info"][0].tolist() == [0.0, 0.0, 0.0, 0.0]
    # a NaN / Inf image inside a 3-image batch: copied with its bits, the other two images as without it
    m, k, shape = SHAPES["multi"]
    clean = dev(_x("multi", "rand"))
    for bw in (None, BW):
        want, want_rec = K.repulse(clean, 0.5, images=m, bandwidth=bw, want_info=True)
        for bad in (float("nan"), float("inf"), float("-inf")):
            x = clean.clone()
            x[k + 3, 1, 7, 9] = bad
            x[k + 5, 0, 0, 0] = -0.0
            keep = x.clone()
            out, rec = K.repulse(x, 0.5, images=m, bandwidth=bw, want_info=True)
            assert rec["applied"].tolist() == [1, 0, 1], (bw, bad)
            assert torch.equal(_bits(out[k:2 * k]), _bits(keep[k:2 * k])) and torch.equal(_bits(x), _bits(keep))
            for sl in (slice(0, k), slice(2 * k, 3 * k)):
                assert torch.equal(out[sl], want[sl]) and torch.isfinite(out[sl]).all()
            for name in ("d2", "w", "info"):
                assert torch.equal(rec[name][0], want_rec[name][0]) and torch.equal(rec[name][2], want_rec[name][2])
            assert (rec["w"][1] == 0).all() and rec["info"][1, 1] == 0


# ----------------------------------------------------------------- 4: properties, bit for bit
@pytest.mark.parametrize("key", ["odd", "multi"])
def test_an_image_does_not_depend_on_the_batch(K, key):
    m, k, shape = SHAPES[key]
    x = dev(_x(key, "img"))
    out, rec = K.repulse(x, 0.4, images=m, want_info=True)
    d2 = K.pairwise_sqdist(x, images=m)
    for i in range(m):
        sl = slice(i * k, (i + 1) * k)
        # (a slice of the odd shape starts off the 16-byte grid: the scalar units either way)
        out_i, rec_i = K.repulse(x[sl], 0.4, want_info=True)
        assert torch.equal(out[sl], out_i), i
        for name in ("d2", "w", "info", "applied"):
            assert torch.equal(rec[name][i], rec_i[name][0]), (i, name)
        assert torch.equal(d2[i], K.pairwise_sqdist(x[sl])[0])
    assert not torch.equal(out, x)


def test_the_three_launches_capture_into_a_graph(K):
    m, k, shape = SHAPES["multi"]
    x = dev(_x("multi", "img"))
    out = torch.empty_like(x)

    def step():
        return K.repulse(x, 0.4, images=m, out=out, want_info=True)

    _, rec = step()                                                        # eager (also the warm-up)
    want, want_rec = out.clone(), {name: v.clone() for name, v in rec.items()}
    assert torch.isfinite(want).all() and not torch.equal(want, x)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _, rec = step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        out.zero_()
        for v in rec.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and all(torch.equal(rec[name], want_rec[name]) for name in rec)


def test_stream_argument(K):
    m, k, shape = SHAPES["multi"]
    x = dev(_x("multi", "rand"))
    want, want_d2 = K.repulse(x, 0.4, images=m), K.pairwise_sqdist(x, images=m)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    out = K.repulse(x, 0.4, images=m, stream=side)
    d2 = K.pairwise_sqdist(x, images=m, stream=side)
    side.synchronize()
    assert torch.equal(out, want) and torch.equal(d2, want_d2)


def test_refusals(K):
    from dps_ttc_amd import _lib
    with pytest.raises(_lib.DpsxError) as e:
        K.repulse(torch.zeros(513, 1, 4, 4, device=DEV), 0.1)
    assert e.value.code == _lib.EUNSUPPORTED
    with pytest.raises(_lib.DpsxError) as e:
        K.pairwise_sqdist(torch.zeros(2 * 513, 4, device=DEV), images=2)
    assert e.value.code == _lib.EUNSUPPORTED
    x = torch.zeros(9, 1, 4, 4, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    out = torch.empty_like(x)
    rc = _lib.lib().dpsx_repulse_f32(0.1, 0.0, _lib.ptr(x), _lib.ptr(out), None, None, None, None, 9, 16, 2, _lib.ptr(ws),
                                     ws.numel(), None)
    assert rc == _lib.EINVAL                                               # N not divisible by segments
    assert _lib.lib().dpsx_pairwise_sqdist_f32(_lib.ptr(x), _lib.ptr(out), None, 9, 16, 2, _lib.ptr(ws), ws.numel(),
                                               None) == _lib.EINVAL
    with pytest.raises(ValueError, match="images"):
        K.repulse(x, 0.1, images=2)
    with pytest.raises(ValueError, match="out must"):
        K.repulse(x, 0.1, out=torch.empty(9, 1, 4, 5, device=DEV))
    with pytest.raises(_lib.DpsxError) as e:                               # out overlapping x
        K.repulse(x, 0.1, out=x)
    assert e.value.code == _lib.EINVAL


# ----------------------------------------------------------------- 5: the loops (stand-in model, 64 x 64, 4 steps)
HW, STEPS, SCALE = 64, 4, 400.0


def _sampler(name, respacing=str(STEPS), eta=None):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing, **({} if eta is None else {"eta": eta}))


@pytest.fixture(scope="module")
def task():
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    gen = torch.Generator(device=DEV).manual_seed(47)
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    noiser = get_noise("gaussian", sigma=0.05)
    M, k = 2, 4
    y = torch.cat([op.forward(torch.rand(1, 3, HW, HW, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
    return {"op": op, "y": y.contiguous(), "M": M, "k": k, "model": StandInModel().to(DEV),
            "ps": get_conditioning_method("ps", op, noiser, scale=0.5),
            "cg": get_conditioning_method("cg", op, noiser, rho_scale=1.0, iters=3),
            "mcg": get_conditioning_method("mcg", op, noiser, scale=0.5),
            "x0": torch.randn(M * k, 3, HW, HW, device=DEV, generator=gen),
            "bank": torch.randn(2 * STEPS, M * k, 3, HW, HW, device=DEV, generator=gen),
            "ubank": torch.rand(STEPS, M * k, device=DEV, generator=gen)}


def _patch_rng(smp, task):
    """the sampler's torch draws replaced by the banks' next entries"""
    it = {"z": 0, "u": 0}

    def rnd(like, stride=None, shape=None):
        z = task["bank"][it["z"], :like.shape[0]].contiguous()
        it["z"] += 1
        return z

    def uni(n, like):
        v = task["ubank"][it["u"], :n].contiguous()
        it["u"] += 1
        return v
    smp._randn, smp._rand = rnd, uni
    return it


def _loop(smp, task, cm, x, y, **kw):
    return smp.p_sample_loop(model=task["model"], x_start=x.clone(), measurement=y, measurement_cond_fn=cm.conditioning,
                             record=False, save_root=None, **kw)


def _spy(K, monkeypatch):
    """kernels.repulse as the loops call it, recorded: (strength, images, bandwidth)"""
    calls, orig = [], K.repulse

    def spy(x, strength, images=1, bandwidth=None, **kw):
        calls.append((strength, images, bandwidth))
        return orig(x, strength, images, bandwidth, **kw)
    monkeypatch.setattr(K, "repulse", spy)
    return calls


def _fused_by_hand(K, ref, task, x0, y, loop_kw, after):
    """K1, K2, the model's VJP and K3 composed here on the noise of bank[k], then after(idx, x, dist)"""
    n, model, cm = x0.shape[0], task["model"], task["ps"]
    handle = task["op"].hip_handle(x0)
    buf = K.StepBuffers(handle, n, 3, HW, HW, DEV)
    x, dist = x0.clone(), None
    for step, idx in enumerate(range(ref.num_timesteps - 1, -1, -1)):
        xp = x.detach().requires_grad_()
        with torch.enable_grad():
            model_out = ref._call_model(model, xp, idx)
        mo, ck, noise = model_out.detach().contiguous(), ref.sample_coefs(idx), task["bank"][step, :n].contiguous()
        spec = cm.fused_spec(**(loop_kw(idx) if loop_kw else {}))
        K.step_fwd(handle, buf, xp.detach(), mo, noise, y, ck, want_x0=False)
        K.step_bwd(handle, buf, y, spec["scale"], spec["power"], ck)
        (g_unet,) = torch.autograd.grad(model_out, xp, grad_outputs=buf.g_model_out)
        x = K.step_update(buf, g_unet.contiguous(), ck)
        x, dist = after(idx, x, buf.norm)
    return x, dist


@pytest.mark.parametrize("bw,stop", [(None, 0.0), (0.5, 0.5)])
def test_ddpm_fused_loop_equals_its_parts(K, task, monkeypatch, bw, stop):
    """ddpm + ps, K = 4 particles of one image: the fused step's launches and kernels.repulse composed by hand.  With
    repulsion_stop = 0.5 the steps idx = 3, 2 launch and idx = 1 does not; idx = 0 never does"""
    x0, y = task["x0"][:4], task["y"][:1]
    smp = _sampler("ddpm")
    smp.repulsion_scale, smp.repulsion_bandwidth, smp.repulsion_stop = SCALE, bw, stop
    it, calls = _patch_rng(smp, task), _spy(K, monkeypatch)
    img, dist, _ = _loop(smp, task, task["ps"], x0, y)
    ran = [idx for idx in range(STEPS - 1, 0, -1) if idx / STEPS >= stop]
    assert it["z"] == STEPS and calls == [(SCALE * smp.betas[idx], 1, bw) for idx in ran] and len(ran) == (3 if not stop else 2)
    monkeypatch.undo()
    ref = _sampler("ddpm")

    def after(idx, x, d):
        return (K.repulse(x, SCALE * ref.betas[idx], 1, bw) if idx in ran else x), d

    want, want_d = _fused_by_hand(K, ref, task, x0, y, lambda idx: dict(beta_scale=ref.betas[idx], t=idx / STEPS), after)
    assert torch.equal(img, want) and torch.equal(dist, want_d) and torch.isfinite(img).all()
    # and it is not the loop without the option, which launches what it always did and keeps no buffer
    off = _sampler("ddpm")
    _patch_rng(off, task)
    plain, _, _ = _loop(off, task, task["ps"], x0, y)
    assert off._repulse_out is None and smp._repulse_out is not None and not torch.equal(plain, img)
    d_on, d_off = K.pairwise_sqdist(img, want_info=True)[1], K.pairwise_sqdist(plain, want_info=True)[1]
    print(f"ddpm bw={bw} stop={stop}: mean d2 of the final particles {d_off[0, 2].item():.4g} without, "
          f"{d_on[0, 2].item():.4g} with the option")


def test_ddim_cg_loop_equals_its_parts(K, task, monkeypatch):
    x0, y = task["x0"][:4], task["y"][:1]
    smp = _sampler("ddim", eta=1.0)
    smp.repulsion_scale = SCALE
    it, calls = _patch_rng(smp, task), _spy(K, monkeypatch)
    img, dist, _ = _loop(smp, task, task["cg"], x0, y)
    assert it["z"] == STEPS and len(calls) == STEPS - 1
    monkeypatch.undo()
    ref = _sampler("ddim", eta=1.0)
    x, d = x0.clone(), None
    for step, idx in enumerate(range(STEPS - 1, -1, -1)):
        x, d = ref.cg_step(task["model"], x, idx, y, task["cg"], {}, noise=task["bank"][step, :4].contiguous())
        if idx > 0:
            x = K.repulse(x, SCALE * ref.betas[idx])
    assert torch.equal(img, x) and torch.equal(dist, d) and torch.isfinite(img).all()


def test_per_op_loop_equals_its_parts(K, task, monkeypatch):
    """ddpm + mcg: p_sample under autograd and the conditioning function, then the repulsion"""
    x0, y = task["x0"][:4], task["y"][:1]
    smp = _sampler("ddpm")
    smp.repulsion_scale = SCALE
    it, calls = _patch_rng(smp, task), _spy(K, monkeypatch)
    img, dist, _ = _loop(smp, task, task["mcg"], x0, y)
    assert len(calls) == STEPS - 1
    monkeypatch.undo()
    ref = _sampler("ddpm")
    it2 = _patch_rng(ref, task)
    x, d = x0.clone(), None
    for idx in range(STEPS - 1, -1, -1):
        _, ret = ref._per_op_step(task["model"], x, idx, y, task["mcg"].conditioning, None, None)
        x, d = ret[0].detach(), ret[1]
        if idx > 0:
            x = K.repulse(x, SCALE * ref.betas[idx])
    assert it2 == it and torch.equal(img, x) and torch.equal(dist, d) and torch.isfinite(img).all()


def test_ttc_ddim_two_images_equals_its_parts(K, task, monkeypatch):
    """ttc_ddim (eta = 1, the device draw, resample_every = 2: after idx 2 and idx 0), 2 images x 4 particles: the push
    comes before the resampling block and is per image"""
    M, k, x0, y = task["M"], task["k"], task["x0"], task["y"]

    def make():
        smp = _sampler("ttc_ddim", eta=1.0)
        smp.resample_draw, smp.resample_every = "device", 2
        return smp

    smp = make()
    smp.repulsion_scale = SCALE
    it, calls = _patch_rng(smp, task), _spy(K, monkeypatch)
    img, dist = _loop(smp, task, task["ps"], x0, y)
    assert it["z"] == STEPS and it["u"] == 2 and calls == [(SCALE * smp.betas[idx], M, None) for idx in (3, 2, 1)]
    monkeypatch.undo()
    ref, nu = make(), {"u": 0}

    def after(idx, x, d):
        if idx > 0:
            x = K.repulse(x, SCALE * ref.betas[idx], M)
        if idx % 2 == 0:
            x, d, _ = K.resample(x, d, task["ubank"][nu["u"]].contiguous(), M, 1.0 / 100)
            nu["u"] += 1
        return x, d

    want, want_d = _fused_by_hand(K, ref, task, x0, y, None, after)
    assert nu["u"] == 2 and torch.equal(img, want) and torch.equal(dist, want_d) and torch.isfinite(img).all()
    # image by image: the two single-image loops fed their image's particles and uniforms
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        one = make()
        one.repulsion_scale = SCALE
        sub = dict(task, bank=task["bank"][:, sl], ubank=task["ubank"][:, sl])
        _patch_rng(one, sub)
        img_m, dist_m = _loop(one, sub, task["ps"], x0[sl], y[m:m + 1])
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m), m
