"""GPU suite of the DPM-Solver++(2M) multistep update (dpsx_step_update_ms_f32, the ddim samplers' solver_order = 2).
The kernel's expression is fully specified, so x_next is compared with the numpy float32 restatement tests/dpmpp_ref.py
bit for bit; the c = 0 form with dpsx_step_update_f32 bit for bit; placements, batches, streams, graph replay and the
loops bit for bit; the end-to-end run against the float64 loop inside the bound stated there.

Shapes (each reaches one code path): N = 3, 3 x 64 x 64 (float4 units, 12 slots); N = 2, 1 x 33 x 47 (chw = 1551: scalar
units, the second particle's base unaligned, a ragged last block); N = 1, 1 x 520 x 520 (the slot count is capped at 256
there: several units per thread); N = 2, 3 x 256 x 256 (192 slots)."""
import numpy as np
import pytest
import torch

import dpmpp_ref
from placement import Arena, Buf, placements
from standin import StandInModel, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"64": (3, (3, 64, 64)), "odd": (2, (1, 33, 47)), "520": (1, (1, 520, 520)), "256": (2, (3, 256, 256))}
RECORDS = ("eta0", "eta1", "last")
CS = (0.0, 0.37, -0.05)
NAMES = ("sample", "g_mo", "g_unet", "x0_cur", "x0_prev")


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def _sampler(name="ddim", respacing="logsnr20", **kw):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing, **kw)


_REC = {}


def _record(name):
    """DDIM records of the logsnr20 sampler: eta = 0 and eta = 1 at a middle step, the step onto the clean image"""
    if not _REC:
        smp = _sampler()
        _REC.update(eta0=smp.sample_coefs(10, eta=0.0), eta1=smp.sample_coefs(10, eta=1.0), last=smp.sample_coefs(0))
        assert _REC["eta1"].min_log > 0 and _REC["eta0"].min_log == 0 and _REC["last"].add_noise == 2
    return _REC[name]


_IN = {}


def _inputs(key):
    """seeded O(1) normals of one shape (built once; g_mo's variance half is zero as in the loop)"""
    if key not in _IN:
        n, (c, h, w) = SHAPES[key]
        rng = np.random.RandomState(300 + len(key) + n)
        full = (n, c, h, w)
        g_mo = np.zeros((n, 2 * c, h, w), np.float32)
        g_mo[:, :c] = rng.randn(*full)
        d = {"sample": rng.randn(*full).astype(np.float32), "g_mo": g_mo, "g_unet": rng.randn(*full).astype(np.float32),
             "x0_cur": rng.randn(*full).astype(np.float32), "x0_prev": rng.randn(*full).astype(np.float32)}
        d["t"] = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
        _IN[key] = d
    return _IN[key]


def _raw(K, t, ck, c, out=None, g_unet=True, hist=True, stream=None, n=None):
    """the entry point itself on the tensors t (a dict like _inputs' "t"; x0_* None or absent with hist=False)"""
    from ctypes import byref
    sample = t["sample"]
    n = sample.shape[0] if n is None else n
    out = torch.full_like(sample, float("nan")) if out is None else out
    rc = K.lib().dpsx_step_update_ms_f32(
        K.ptr(sample), K.ptr(t["g_mo"]), K.ptr(t["g_unet"]) if g_unet else None, K.ptr(t["x0_cur"]) if hist else None,
        K.ptr(t["x0_prev"]) if hist else None, float(c), K.ptr(out), n, sample[0].numel(), byref(ck),
        K._stream_arg(stream, sample))
    return rc, out


def _ref32(d, ck, c, g_unet=True, rows=slice(None)):
    ch = d["sample"].shape[1]
    return dpmpp_ref.update_f32(d["sample"][rows], d["g_mo"][rows, :ch], d["g_unet"][rows] if g_unet else None,
                                d["x0_cur"][rows], d["x0_prev"][rows], c, ck.a, ck.b)


def _bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _k3(K, t, ck, g_unet=True):
    buf = K.StepBuffers(None, *t["sample"].shape, DEV)
    buf.sample.copy_(t["sample"])
    buf.g_model_out.copy_(t["g_mo"])
    return K.step_update(buf, t["g_unet"] if g_unet else None, ck)


# ----------------------------------------------------------------- 1: the restatement, bit for bit
@pytest.mark.parametrize("rec", RECORDS)
@pytest.mark.parametrize("key", list(SHAPES))
def test_update_equals_the_restatement_bit_for_bit(K, key, rec):
    """x_next against numpy float32, operation by operation (bit for bit: the inputs are O(1) normals, every intermediate
    is a normal number or an exact zero), and against the float64 evaluation within 1e-6 rel-L2 (five fp32 roundings of
    6e-8 each on O(1) values)"""
    d, ck = _inputs(key), _record(rec)
    ch = d["sample"].shape[1]
    for c in CS:
        for g_unet in (True, False):
            rc, x = _raw(K, d["t"], ck, c, g_unet=g_unet)
            assert rc == 0
            want = _ref32(d, ck, c, g_unet)
            assert np.isfinite(want).all() and np.array_equal(_bits(x), _bits(want)), (c, g_unet)
            f64 = dpmpp_ref.update_f64(d["sample"], d["g_mo"][:, :ch], d["g_unet"] if g_unet else None, d["x0_cur"],
                                       d["x0_prev"], c, ck.a, ck.b)
            assert rel_l2(x.cpu().numpy(), f64) < 1e-6, (c, g_unet)
    # the front end: the histories are the buffers' own, x_next flips as step_update's does
    n, shape = SHAPES[key]
    buf = K.StepBuffers(None, n, *shape, DEV)
    buf.sample.copy_(d["t"]["sample"])
    buf.g_model_out.copy_(d["t"]["g_mo"])
    buf.x0_hat.copy_(d["t"]["x0_prev"])
    assert buf.advance_x0() is buf.x0_prev and buf.x0_hat is not buf.x0_prev
    buf.x0_hat.copy_(d["t"]["x0_cur"])
    for c in CS:
        flip = buf.flip
        x = K.step_update_ms(buf, d["t"]["g_unet"], ck, c)
        assert x is buf.x_next[flip] and buf.flip == flip ^ 1
        assert np.array_equal(_bits(x), _bits(_ref32(d, ck, c)))
    with pytest.raises(ValueError, match="previous step"):
        K.step_update_ms(K.StepBuffers(None, n, *shape, DEV), None, ck, 0.37)


# ----------------------------------------------------------------- 2: c = 0
@pytest.mark.parametrize("key", ["64", "odd", "520"])
def test_c_zero_is_k3_bit_for_bit(K, key):
    """c = 0 against dpsx_step_update_f32, with elements where sample - s is -0.0 and a NaN among the inputs; unchanged
    with both histories full of NaN; accepted with null histories"""
    d, ck = _inputs(key), _record("eta0")
    t = {k: v.clone() for k, v in d["t"].items()}
    n = t["sample"].shape[0]
    s, g, u = t["sample"].view(n, -1), t["g_mo"].view(n, 2, -1)[:, 0], t["g_unet"].view(n, -1)
    g[:, :8] = 0.0                    # ratio * 0 = -0.0 (ratio < 0): s = -0.0 + g_unet
    u[:, :2] = -0.0                   # s = -0.0 with g_unet, +0.0 without (-0.0 + 0.0f)
    u[:, 2:8] = 0.0                   # s = +0.0
    s[:, :4] = -0.0                   # -0.0 - (+0.0) = -0.0 ;  -0.0 - (-0.0) = +0.0
    s[:, 4:8] = 0.0
    s[0, 11] = float("nan")
    u[0, 13] = float("-inf")
    for g_unet in (True, False):
        want = _k3(K, t, ck, g_unet)
        assert torch.isnan(want.view(-1)[11]) and (not g_unet or want.view(-1)[13] == float("inf"))
        rc, x = _raw(K, t, ck, 0.0, g_unet=g_unet)
        assert rc == 0 and np.array_equal(_bits(x), _bits(want))
        signs = _bits(want).reshape(n, -1)[:, :8] >> 31
        assert signs.any() and not signs.all()                          # -0.0 and +0.0 among the results
        nan = dict(t, x0_cur=torch.full_like(t["sample"], float("nan")), x0_prev=torch.full_like(t["sample"], float("nan")))
        rc, x = _raw(K, nan, ck, 0.0, g_unet=g_unet)
        assert rc == 0 and np.array_equal(_bits(x), _bits(want))
        rc, x = _raw(K, t, ck, 0.0, g_unet=g_unet, hist=False)
        assert rc == 0 and np.array_equal(_bits(x), _bits(want))
        rc, x = _raw(K, t, ck, -0.0, g_unet=g_unet, hist=False)                          # -0.0 == 0
        assert rc == 0 and np.array_equal(_bits(x), _bits(want))


def ch_of(d):
    return d["sample"].shape[1]


# ----------------------------------------------------------------- 3: every buffer 4 bytes off the grid
@pytest.mark.parametrize("key", ["64", "odd"])
def test_an_unaligned_view_gives_the_aligned_bits(K, key):
    d, ck = _inputs(key), _record("eta1")

    def off4(v):
        flat = torch.empty(v.numel() + 1, dtype=torch.float32, device=DEV)
        w = flat[1:].view(v.shape)
        w.copy_(v)
        assert w.data_ptr() % 16 == 4
        return w

    for c in (0.37, 0.0):
        _, want = _raw(K, d["t"], ck, c)
        for name in NAMES + ("x_next",):
            t = dict(d["t"])
            out = None
            if name == "x_next":
                out = off4(torch.full_like(want, float("nan")))
            else:
                t[name] = off4(t[name])
            rc, x = _raw(K, t, ck, c, out=out)
            assert rc == 0 and np.array_equal(_bits(x), _bits(want)), (c, name)
            for k in NAMES:                                             # inputs are never written
                assert np.array_equal(_bits(t[k]), _bits(d[k])), (c, name, k)


# ----------------------------------------------------------------- 4: a non-finite value stays in its element
@pytest.mark.parametrize("key", ["64", "odd"])
def test_a_non_finite_value_reaches_its_own_element_only(K, key):
    d, ck = _inputs(key), _record("eta0")
    n = SHAPES[key][0]
    _, clean = _raw(K, d["t"], ck, 0.37)
    per = clean[0].numel()
    for name in ("x0_cur", "x0_prev", "g_unet", "g_mo"):
        for j, bad in enumerate((float("nan"), float("inf"), float("-inf"))):
            t = {k: v.clone() for k, v in d["t"].items()}
            e = 5 + 7 * j
            t[name][1].view(-1)[e] = bad                                # particle 1, element e (of g_mo's eps half)
            _, x = _raw(K, t, ck, 0.37)
            hit = torch.zeros(n, per, dtype=torch.bool, device=DEV)
            hit[1, e] = True
            assert not torch.isfinite(x.view(n, per)[1, e]), (name, bad)
            assert np.array_equal(_bits(x.view(n, per)[~hit]), _bits(clean.view(n, per)[~hit])), (name, bad)


# ----------------------------------------------------------------- 5: batches, streams, graphs
@pytest.mark.parametrize("key", ["64", "odd"])
def test_rows_streams_and_graph_replay(K, key):
    d, ck = _inputs(key), _record("eta1")
    t = d["t"]
    n = SHAPES[key][0]
    _, want = _raw(K, t, ck, 0.37)
    for p in range(n):                                                  # a row of the batch against its own call
        row = {k: v[p:p + 1].contiguous() for k, v in t.items()}
        _, x = _raw(K, row, ck, 0.37)
        assert np.array_equal(_bits(x), _bits(want[p:p + 1])), p
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    rc, x = _raw(K, t, ck, 0.37, stream=side)
    side.synchronize()
    assert rc == 0 and torch.equal(x, want)
    buf = K.StepBuffers(None, *t["sample"].shape, DEV)
    buf.sample.copy_(t["sample"])
    buf.g_model_out.copy_(t["g_mo"])
    buf.advance_x0()
    buf.x0_hat.copy_(t["x0_cur"])
    buf.x0_prev.copy_(t["x0_prev"])
    side.wait_stream(torch.cuda.current_stream())
    x = K.step_update_ms(buf, t["g_unet"], ck, 0.37, stream=side)
    side.synchronize()
    assert torch.equal(x, want)

    def step():
        buf.flip = 0
        return K.step_update_ms(buf, t["g_unet"], ck, 0.37)

    assert torch.equal(step(), want)                                    # eager (also the warm-up)
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x = step()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(x, want)


# ----------------------------------------------------------------- 6: placement
@pytest.mark.parametrize("c", [0.37, 0.0])
@pytest.mark.parametrize("key", ["64", "odd"])
def test_placement(K, key, c):
    """the call's buffers at their exact sizes between guard bands, aligned / all off the grid / each alone: guards
    untouched, every element of x_next written, the aligned placement's bits (and the restatement's); a refusal writes
    nothing"""
    from ctypes import byref
    d, ck = _inputs(key), _record("eta0")
    n, (ch, h, w) = SHAPES[key]
    F = torch.float32
    full = (n, ch, h, w)
    bufs = [Buf("sample", full, F, "in"), Buf("g_mo", (n, 2 * ch, h, w), F, "in"), Buf("g_unet", full, F, "in"),
            Buf("x0_cur", full, F, "in"), Buf("x0_prev", full, F, "in"), Buf("x_next", full, F, "out")]
    lib = K.lib()

    def call(a, c=c, n=n):
        rc = lib.dpsx_step_update_ms_f32(a.ptr("sample"), a.ptr("g_mo"), a.ptr("g_unet"), a.ptr("x0_cur"), a.ptr("x0_prev"),
                                         c, a.ptr("x_next"), n, ch * h * w, byref(ck), K.stream_of(a.mem))
        torch.cuda.synchronize()
        return rc

    want = _bits(_ref32(d, ck, c))
    for tag, offs in placements([b.name for b in bufs], lambda name: 4):
        a = Arena(bufs, offs, device=DEV)
        for name in NAMES:
            a.put(name, d[name])
        assert call(a) == 0, tag
        assert a.violations(True, written=["x_next"]) == [], tag
        assert np.array_equal(_bits(a.get("x_next")), want), tag
        for name in NAMES:
            assert np.array_equal(_bits(a.get(name)), _bits(d[name])), (tag, name)
        before = a.snapshot()
        from dps_ttc_amd import _lib
        assert call(a, n=65536) == _lib.EUNSUPPORTED and a.violations(False, before=before) == [], tag
        assert call(a, c=float("nan")) == _lib.EINVAL and a.violations(False, before=before) == [], tag


# ----------------------------------------------------------------- 7: the loops (stand-in model, Gaussian blur, 3 x 64 x 64)
HW, RESPACING, STEPS = 64, "logsnr10", 10


@pytest.fixture(scope="module")
def task():
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    gen = torch.Generator(device=DEV).manual_seed(47)
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.3)
    M, k = 2, 2
    y = torch.cat([op.forward(torch.rand(1, 3, HW, HW, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
    assert _sampler(respacing=RESPACING).num_timesteps == STEPS
    return {"op": op, "cm": cm, "y": y.contiguous(), "M": M, "k": k, "model": StandInModel().to(DEV),
            "x0": torch.randn(M * k, 3, HW, HW, device=DEV, generator=gen),
            "bank": torch.randn(STEPS, M * k, 3, HW, HW, device=DEV, generator=gen),
            "ubank": torch.rand(STEPS, M * k, device=DEV, generator=gen)}


def _patch_rng(smp, bank, ubank):
    """the sampler's torch draws replaced by the banks' next entries"""
    it = {"z": 0, "u": 0}

    def rnd(like, stride=None, shape=None):
        z = bank[it["z"], :like.shape[0]].contiguous()
        it["z"] += 1
        return z

    def uni(n, like):
        v = ubank[it["u"], :n].contiguous()
        it["u"] += 1
        return v
    smp._randn, smp._rand = rnd, uni
    return it


def _loop(smp, task, x, y, **kw):
    return smp.p_sample_loop(model=task["model"], x_start=x.clone(), measurement=y, measurement_cond_fn=task["cm"].conditioning,
                             record=False, save_root=None, **kw)


def _by_hand(K, ref, task, x0, y, order, after=None):
    """K1, K2, the model's VJP and the update composed here: the noise of step k is bank[k], c is the restatement's, the
    histories are this function's own tensors and the entry point is called directly"""
    n, model = x0.shape[0], task["model"]
    handle = task["op"].hip_handle(x0)
    buf = K.StepBuffers(handle, n, 3, HW, HW, DEV)
    spec = task["cm"].fused_spec()
    cs = dpmpp_ref.c32(ref.alphas_cumprod, float(ref.eta))
    x, dist, prev = x0.clone(), None, None
    for k, idx in enumerate(range(ref.num_timesteps - 1, -1, -1)):
        xp = x.detach().requires_grad_()
        with torch.enable_grad():
            model_out = ref._call_model(model, xp, idx)
        mo, ck, noise = model_out.detach().contiguous(), ref.sample_coefs(idx), task["bank"][k, :n].contiguous()
        K.step_fwd(handle, buf, xp.detach(), mo, noise, y, ck, want_x0=order == 2)
        K.step_bwd(handle, buf, y, spec["scale"], spec["power"], ck)
        (g_unet,) = torch.autograd.grad(model_out, xp, grad_outputs=buf.g_model_out)
        if order == 2:
            cur = buf.x0_hat.clone()
            c = float(cs[idx])
            assert (c == 0.0) == (prev is None or idx == 0)
            t = {"sample": buf.sample, "g_mo": buf.g_model_out, "g_unet": g_unet.contiguous(), "x0_cur": cur, "x0_prev": prev}
            rc, x = _raw(K, t, ck, c, hist=c != 0.0)
            assert rc == 0
            prev = cur
        else:
            x = K.step_update(buf, g_unet.contiguous(), ck).clone()
        dist = buf.norm.clone()
        if after is not None:
            x, dist, prev = after(idx, x, dist, prev)
    return x, dist


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ddim_loop_equals_its_parts(K, task, eta):
    """ddim, logsnr10, order 2 against the launches composed by hand, bit for bit; order 1 through the same loop against
    the loop's launches of today (K1 without the x0_hat store, K3); the two orders differ"""
    n = 3
    x0, y = task["x0"][:n], task["y"][:1]
    outs = {}
    for order in (2, 1):
        smp = _sampler(respacing=RESPACING, eta=eta, solver_order=order)
        it = _patch_rng(smp, task["bank"], task["ubank"])
        img, dist, _ = _loop(smp, task, x0, y)
        assert it["z"] == STEPS
        want, want_d = _by_hand(K, _sampler(respacing=RESPACING, eta=eta), task, x0, y, order)
        assert torch.equal(img, want) and torch.equal(dist, want_d), order
        assert torch.isfinite(img).all() and not torch.equal(img, x0)
        outs[order] = img
    assert not torch.equal(outs[1], outs[2])
    # a second trajectory on the same sampler (the buffers and their alternation are reused)
    smp = _sampler(respacing=RESPACING, eta=eta, solver_order=2)
    for _ in range(2):
        _patch_rng(smp, task["bank"], task["ubank"])
        assert torch.equal(_loop(smp, task, x0, y)[0], outs[2])


def test_particle_groups_equal_one_chain(K, task):
    x0, y = task["x0"], task["y"][:1]
    outs = []
    for groups in (1, 2):
        smp = _sampler(respacing=RESPACING, eta=1.0, solver_order=2)
        smp.particle_groups = groups
        _patch_rng(smp, task["bank"], task["ubank"])
        outs.append(_loop(smp, task, x0, y))
        torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_multi_image_equals_image_by_image(K, task):
    """M = 2 images x K = 2 particles in one loop against the two single-image loops fed their image's paths"""
    M, k, x0, y = task["M"], task["k"], task["x0"], task["y"]

    def run(x, yy):
        smp = _sampler(respacing=RESPACING, eta=1.0, solver_order=2)
        smp.noise_draw, smp.noise_seed, smp.path_base = "device", 9, 100
        return _loop(smp, task, x, yy)

    img, dist, _ = run(x0, y)
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        img_m, dist_m, _ = run(x0[sl], y[m:m + 1])
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m), m
    assert not torch.equal(img[:k], img[k:])


def test_device_noise_does_not_depend_on_the_batch(K, task):
    """noise_draw = "device", eta = 1: N = 4 equals 2 + 2 with path_base"""
    x0, y = task["x0"], task["y"][:1]

    def run(x, base):
        smp = _sampler(respacing=RESPACING, eta=1.0, solver_order=2)
        smp.noise_draw, smp.noise_seed, smp.path_base = "device", 11, base
        return _loop(smp, task, x, y)

    img, dist, _ = run(x0, 40)
    for lo in (0, 2):
        img2, dist2, _ = run(x0[lo:lo + 2], 40 + lo)
        assert torch.equal(img[lo:lo + 2], img2) and torch.equal(dist[lo:lo + 2], dist2), lo


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_ttc_ddim_gathers_the_history_with_the_drawn_ids(K, task, eta):
    """ttc_ddim (the device draw, resample_every = 2) against a hand-composed loop whose history is gathered with the ids
    each resampling drew; at least one resampling permuted the particles"""
    x0, y = task["x0"], task["y"][:1]

    def make(order):
        smp = _sampler("ttc_ddim", respacing=RESPACING, eta=eta, solver_order=order)
        smp.resample_draw, smp.resample_every = "device", 2
        return smp

    smp = make(2)
    it = _patch_rng(smp, task["bank"], task["ubank"])
    img, dist = _loop(smp, task, x0, y)
    assert it["z"] == STEPS and it["u"] == STEPS // 2
    nu, moved = {"u": 0}, []

    def after(idx, x, d, prev):
        if idx % 2:
            return x, d, prev
        x, d, ids = K.resample(x, d, task["ubank"][nu["u"]].contiguous(), 1, 1.0 / 100)
        nu["u"] += 1
        moved.append(not torch.equal(ids, torch.arange(ids.numel(), device=DEV)))
        return x, d, K.gather(prev, ids)

    want, want_d = _by_hand(K, make(1), task, x0, y, 2, after=after)
    assert nu["u"] == STEPS // 2 and any(moved[:-1])                    # (the last one, after idx 0, has no later step)
    assert torch.equal(img, want) and torch.equal(dist, want_d)
    assert torch.isfinite(img).all()

    # without the gather the result differs: the test sees the history
    def stale(idx, x, d, prev):
        x, d, _ = after(idx, x, d, prev)
        return x, d, prev
    nu["u"] = 0
    other, _ = _by_hand(K, make(1), task, x0, y, 2, after=stale)
    assert not torch.equal(other, want)


# ----------------------------------------------------------------- 8: end to end on the analytic model
class GaussEps(torch.nn.Module):
    """the closed-form eps of data ~ N(m, v) per element under the linear 1000-step schedule, zero variance channels"""

    def __init__(self, m=0.2, v=0.04):
        super().__init__()
        abar = np.cumprod(1.0 - np.linspace(1e-4, 2e-2, 1000, dtype=np.float64))
        self.register_buffer("k", torch.tensor(np.sqrt(1.0 - abar) / (abar * v + 1.0 - abar), dtype=torch.float32))
        self.register_buffer("mean", torch.tensor(np.sqrt(abar) * m, dtype=torch.float32))

    def forward(self, x, t):
        idx = t.float().round().long().clamp(0, 999)
        eps = self.k[idx].view(-1, 1, 1, 1) * (x - self.mean[idx].view(-1, 1, 1, 1))
        return torch.cat([eps, torch.zeros_like(eps)], dim=1)


def test_end_to_end_on_the_analytic_model(K):
    """`ps` at scale 0, N = 2 at 3 x 64 x 64, logsnr20, order 2, eta = 0: the loop's result within 1e-4 rel-L2 of the
    float64 loop of tests/dpmpp_ref.py -- the bound test_dsg_gpu / test_cg_gpu use for an fp32 chain against float64.
    Observed: 2.5e-7 (the DPM-Solver++ subsection)."""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    gen = torch.Generator(device=DEV).manual_seed(53)
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.0)
    y = op.forward(torch.rand(1, 3, HW, HW, device=DEV, generator=gen) * 2 - 1).detach().contiguous()
    x_T = torch.randn(2, 3, HW, HW, device=DEV, generator=gen)
    smp = _sampler(respacing="logsnr20", eta=0.0, solver_order=2)
    img, _, _ = smp.p_sample_loop(model=GaussEps().to(DEV), x_start=x_T.clone(), measurement=y,
                                  measurement_cond_fn=cm.conditioning, record=False, save_root=None)
    g = dpmpp_ref.GaussModel(smp.alphas_cumprod, m=0.2, v=0.04)
    want = dpmpp_ref.loop_f64(smp.alphas_cumprod, g.eps, x_T.cpu().numpy().astype(np.float64), 2, eta=0.0)
    err = rel_l2(img.cpu().numpy(), want)
    print("end to end, logsnr20 order 2: rel-L2 against the float64 loop", err)
    assert np.isfinite(want).all() and err <= 1e-4, err
    first = dpmpp_ref.loop_f64(smp.alphas_cumprod, g.eps, x_T.cpu().numpy().astype(np.float64), 1, eta=0.0)
    assert rel_l2(first, want) > 1e-3                                   # the two orders are apart by far more than the bound
