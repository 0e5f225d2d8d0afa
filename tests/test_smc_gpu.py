"""GPU suite of the particle weights (dpsx_step_update_corr_f32, dpsx_smc_accum_f32) and the smc_ddpm loop.
x_next is compared bit for bit with K3's, the correction with the float64 restatement tests/smc_ref.py inside the bound
derived below, the batch / rng / NaN properties and the loops bit for bit (torch.equal).

Shapes: the smallest that reach each code path -- N = 3, 3 x 64 x 64 (12 slots, float4 units); N = 2, 1 x 33 x 47 (scalar
units, the second particle's base unaligned, a ragged last block); N = 2, 3 x 256 x 256 (192 slots, the loop's geometry);
N = 1, 1 x 520 x 520 (the slot count is capped at 256 there: the first size where a block walks more than one range)."""
import numpy as np
import pytest
import torch

import smc_ref
from standin import StandInModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"64": (3, (3, 64, 64)), "odd": (2, (1, 33, 47)), "256": (2, (3, 256, 256)), "520": (1, (1, 520, 520))}
RECORDS = ("ddpm500", "ddpm1", "ddim500")


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def _sampler(name, respacing=""):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing)


_REC = {}


def _record(name):
    """records from the samplers' own tables: DDPM at t = 500, 1 and 0 (no noise), DDIM at t = 500 with eta = 0.5"""
    if not _REC:
        ddpm, ddim = _sampler("ddpm"), _sampler("ddim")
        _REC.update(ddpm500=ddpm.step_coefs[500], ddpm1=ddpm.step_coefs[1], ddpm0=ddpm.step_coefs[0],
                    ddim500=ddim.sample_coefs(500, eta=0.5))
        assert _REC["ddim500"].add_noise == 3 and _REC["ddim500"].min_log > 0 and _REC["ddpm0"].add_noise == 0
    return _REC[name]


_IN = {}


def _inputs(key):
    """seeded inputs of one shape (built once): g_eps and g_unet about 1e-3 N(0, 1), v uniform in (-1, 1), z N(0, 1)"""
    if key not in _IN:
        n, (c, h, w) = SHAPES[key]
        rng = np.random.RandomState(100 + len(key) + n)
        full = (n, c, h, w)
        g_mo = np.zeros((n, 2 * c, h, w), np.float32)
        g_mo[:, :c] = 1e-3 * rng.randn(*full)
        d = {"sample": rng.randn(*full).astype(np.float32), "g_mo": g_mo,
             "g_unet": (1e-3 * rng.randn(*full)).astype(np.float32),
             "mo": np.concatenate([rng.randn(*full), rng.uniform(-1, 1, full)], axis=1).astype(np.float32),
             "z": rng.randn(*full).astype(np.float32)}
        d["t"] = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
        _IN[key] = d
    return _IN[key]


def _buf(K, t, rows=None):
    """StepBuffers holding (the rows `rows` of) the inputs' sample and g_model_out"""
    sl = slice(None) if rows is None else rows
    sample, g_mo = t["sample"][sl], t["g_mo"][sl]
    buf = K.StepBuffers(None, *sample.shape, DEV)
    buf.sample.copy_(sample)
    buf.g_model_out.copy_(g_mo)
    return buf


def _corr(K, t, ck, rows=None, noise=True, rng=None, g_unet=True):
    sl = slice(None) if rows is None else rows
    buf = _buf(K, t, rows)
    x, part = K.step_update_corr(buf, t["g_unet"][sl].contiguous() if g_unet else None, ck, t["mo"][sl].contiguous(),
                                 noise=t["z"][sl].contiguous() if noise and rng is None else None, rng=rng)
    return x, part


# ----------------------------------------------------------------- 1 + 2: x_next bits, corr against the restatement
@pytest.mark.parametrize("rec", RECORDS)
@pytest.mark.parametrize("key", list(SHAPES))
def test_x_next_bits_and_correction(K, key, rec):
    """|corr - ref| <= 1e-5 S, S = sum |q| (|z| + |q| / 2).  Per term: __expf's documented 4e-7 enters q once and q^2
    twice, three roundings of 6e-8 add to that; the fp32 block sum of at most 1024 terms adds at most 12 roundings (four
    serial, an eight-level tree): under 2e-6 S together, the bound is 5 x that."""
    d, ck = _inputs(key), _record(rec)
    t = d["t"]
    n, (c, h, w) = SHAPES[key]
    want_x = K.step_update(_buf(K, t), t["g_unet"], ck)
    x, part = _corr(K, t, ck)
    assert part.shape == (n, K.corr_slots(c * h * w)) and part.dtype == torch.float32
    assert torch.equal(x, want_x)
    ref, scale = smc_ref.correction(d["g_mo"][:, :c], d["g_unet"], d["mo"][:, c:], d["z"], ck)
    got = part.double().sum(dim=1).cpu().numpy()
    ratio = np.abs(got - ref) / scale
    print(f"{key} {rec}: corr {got.tolist()} ref {ref.tolist()} S {scale.tolist()} |corr - ref| / S max {ratio.max():.3e}")
    assert np.all(scale > 0) and np.all(np.isfinite(got))
    assert np.all(np.abs(got - ref) <= 1e-5 * scale)
    # without g_unet: K3's bits again
    x0, _ = _corr(K, t, ck, g_unet=False)
    assert torch.equal(x0, K.step_update(_buf(K, t), None, ck))


@pytest.mark.parametrize("key", ["64", "odd"])
def test_zero_update_and_noiseless_step_give_exact_zeros(K, key):
    t = _inputs(key)["t"]
    zero = dict(t, g_mo=torch.zeros_like(t["g_mo"]), g_unet=torch.zeros_like(t["g_unet"]))
    for rec in RECORDS:
        x, part = _corr(K, zero, _record(rec))
        assert torch.equal(part, torch.zeros_like(part)) and torch.equal(x, t["sample"])
    # a record without noise: zeros, and model_out / noise are not read
    nan = dict(t, mo=torch.full_like(t["mo"], float("nan")), z=torch.full_like(t["z"], float("nan")))
    ck = _record("ddpm0")
    x, part = _corr(K, nan, ck)
    assert torch.equal(part, torch.zeros_like(part))
    assert torch.equal(x, K.step_update(_buf(K, t), t["g_unet"], ck))
    x, part = _corr(K, nan, ck, rng=K.Rng(3, 0))
    assert torch.equal(part, torch.zeros_like(part)) and torch.isfinite(x).all()


# ----------------------------------------------------------------- 3: bit-for-bit properties
@pytest.mark.parametrize("key", ["64", "odd"])
def test_partials_do_not_depend_on_the_batch(K, key):
    t, ck = _inputs(key)["t"], _record("ddpm500")
    n = SHAPES[key][0]
    x, part = _corr(K, t, ck)
    for j in range(n):
        xj, pj = _corr(K, t, ck, rows=slice(j, j + 1))
        assert torch.equal(pj[0], part[j]) and torch.equal(xj[0], x[j]), j


@pytest.mark.parametrize("rec", ["ddpm500", "ddim500"])
@pytest.mark.parametrize("key", ["64", "odd", "520"])
def test_rng_form_equals_pointer_form(K, key, rec):
    t, ck = _inputs(key)["t"], _record(rec)
    n, shape = SHAPES[key]
    rng = K.Rng(seed=0x1234567890, step=500, tag=K.Rng.TAG_STEP, particle_base=5)
    z = K.randn((n,) + shape, rng, DEV)
    x_p, part_p = _corr(K, dict(t, z=z), ck)
    x_r, part_r = _corr(K, t, ck, rng=rng)
    assert torch.equal(part_r, part_p) and torch.equal(x_r, x_p)
    assert bool((part_p != _corr(K, t, ck)[1]).any())                     # the draw is not the seeded z
    if n > 1:                                                             # the particle-id rule: row 1 alone at base + 1
        _, p1 = _corr(K, t, ck, rows=slice(1, 2), rng=rng.offset(1))
        assert torch.equal(p1[0], part_r[1])


def test_a_nan_stays_inside_its_particle(K):
    t, ck = _inputs("64")["t"], _record("ddpm500")
    n, shape = SHAPES["64"]
    _, clean = _corr(K, t, ck)
    g = t["g_unet"].clone()
    g[1, 2, 17, 5] = float("nan")
    _, part = _corr(K, dict(t, g_unet=g), ck)
    keep = [0, 2]
    assert torch.equal(part[keep], clean[keep]) and bool(torch.isnan(part[1]).any())
    d = torch.tensor([50.0, 40.0, 60.0], device=DEV)
    st, st_clean = K.SmcState(n, shape, DEV), K.SmcState(n, shape, DEV)
    st.corr_partials.copy_(part)
    st_clean.corr_partials.copy_(clean)
    K.smc_accum(st, d), K.smc_accum(st_clean, d)
    assert bool(torch.isnan(st.E[1])) and torch.equal(st.E[keep], st_clean.E[keep]) and torch.isfinite(st_clean.E).all()
    assert torch.equal(st.d_prev, d)
    # a NaN weight is never drawn
    ids = K.resample_draw(st.E, torch.rand(n, device=DEV), 1, 1.0)
    assert 1 not in ids.tolist()


# ----------------------------------------------------------------- 4: the recurrence
@pytest.mark.parametrize("power", [1, 2])
def test_accum_against_the_restatement(K, power):
    """four chained calls, two segments of three particles, a reset mask on one segment at the third call: every E within
    2 ulp of the float64 restatement's rounded value or 1e-6 of the terms' summed magnitudes; d_prev bit-equal to d_cur"""
    n, segments, shape = 6, 2, (3, 64, 64)
    st = K.SmcState(n, shape, DEV)
    rng = np.random.RandomState(11 + power)
    E, dp = np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for call in range(4):
        dc = (50.0 + 10.0 * rng.randn(n)).astype(np.float32)
        part = (3.0 * rng.randn(n, st.slots)).astype(np.float32)
        reset = np.array([0, 1], np.uint8) if call == 2 else (np.zeros(2, np.uint8) if call == 3 else None)
        ts, pw = (0.01, 1.0) if call < 3 else (0.37, 0.25)
        st.corr_partials.copy_(torch.from_numpy(part))
        out = K.smc_accum(st, torch.from_numpy(dc).to(DEV), None if reset is None else torch.from_numpy(reset).to(DEV),
                          segments, ts, power, pw)
        assert out is st.E
        E, dp, mag = smc_ref.accum(E, dp, dc, part, reset, segments, ts, power, pw)
        got = st.E.cpu().numpy()
        err = np.abs(got.astype(np.float64) - E.astype(np.float64))
        bound = np.maximum(2 * np.spacing(np.abs(E)).astype(np.float64), 1e-6 * mag)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (call, got, E)
        assert np.array_equal(st.d_prev.cpu().numpy(), dc)
        E = got                                                           # chain on the kernel's own state
    print(f"power {power}: largest error / bound {worst:.3f}")
    # proposal_weight = 0 drops the term: NaN partials are not read
    st.corr_partials.fill_(float("nan"))
    before = st.E.clone()
    K.smc_accum(st, st.d_prev.clone(), None, segments, 0.0, power, 0.0)
    assert torch.equal(st.E, before)


# ----------------------------------------------------------------- the loops (stand-in model, 64 x 64, 12 steps)
HW, STEPS = 64, 12


@pytest.fixture(scope="module")
def task():
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    gen = torch.Generator(device=DEV).manual_seed(41)
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    M, k = 2, 4
    y = torch.cat([op.forward(torch.rand(1, 3, HW, HW, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
    return {"op": op, "cm": cm, "y": y.contiguous(), "M": M, "k": k, "model": StandInModel().to(DEV),
            "x0": torch.randn(M * k, 3, HW, HW, device=DEV, generator=gen),
            "bank": torch.randn(STEPS, M * k, 3, HW, HW, device=DEV, generator=gen),
            "ubank": torch.rand(STEPS, M * k, device=DEV, generator=gen)}


def _patch_rng(smp, bank, ubank, offset=0):
    """noise and uniforms of particle p: row offset + p of the banks' next entry"""
    it = {"z": 0, "u": 0}

    def rnd(like, stride=None, shape=None):
        z = bank[it["z"], offset:offset + like.shape[0]].contiguous()
        it["z"] += 1
        return z

    def uni(n, like):
        v = ubank[it["u"], offset:offset + n].contiguous()
        it["u"] += 1
        return v
    smp._randn, smp._rand = rnd, uni
    return it


def _loop(smp, task, x, y, **kw):
    return smp.p_sample_loop(model=task["model"], x_start=x.clone(), measurement=y, measurement_cond_fn=task["cm"].conditioning,
                             record=False, save_root=None, **kw)


@pytest.mark.parametrize("tau", [0.5, 1.0])
def test_loop_equals_its_parts(K, task, tau):
    """smc_ddpm (N = 8, 12 steps, resample_every = 3, systematic, tau = 0.5) against the same launches composed here;
    tau = 1.0 besides: with these inputs no image falls below half its particles at the three looks (observed flags 0, 0, 0),
    and the reset / gathered d_prev route wants a loop that does resample"""
    n = 8
    x0, y, model, cm = task["x0"], task["y"][:1], task["model"], task["cm"]
    smp = _sampler("smc_ddpm", str(STEPS))
    smp.resample_every, smp.resample_scheme, smp.resample_ess = 3, "systematic", tau
    it = _patch_rng(smp, task["bank"], task["ubank"])
    img, dist = _loop(smp, task, x0, y)
    assert it["z"] == STEPS and it["u"] == 3                             # resampling after idx 9, 6, 3
    assert img.shape == x0.shape and dist.shape == (n,)

    ref = _sampler("smc_ddpm", str(STEPS))
    handle = task["op"].hip_handle(x0)
    buf, st = K.StepBuffers(handle, n, 3, HW, HW, DEV), K.SmcState(n, (3, HW, HW), DEV)
    x, reset, ids, flags, nz, nu, all_flags = x0.clone(), None, None, None, 0, 0, []
    for idx in range(STEPS - 1, -1, -1):
        xp = x.detach().requires_grad_()
        with torch.enable_grad():
            model_out = ref._call_model(model, xp, idx)
        mo, ck, noise = model_out.detach().contiguous(), ref.sample_coefs(idx), task["bank"][nz].contiguous()
        nz += 1
        spec = cm.fused_spec(beta_scale=ref.betas[idx], t=idx / ref.num_timesteps)
        K.step_fwd(handle, buf, xp.detach(), mo, noise, y, ck, want_x0=False)
        K.step_bwd(handle, buf, y, spec["scale"], spec["power"], ck)
        (g_unet,) = torch.autograd.grad(model_out, xp, grad_outputs=buf.g_model_out)
        x, _ = K.step_update_corr(buf, g_unet.contiguous(), ck, mo, noise=noise, state=st)
        K.smc_accum(st, buf.norm, reset, 1, 0.01, 1, 1.0)
        reset = None
        if idx % 3 == 0 and idx > 0:
            x, _, ids, flags, _ = K.resample(x, st.E, task["ubank"][nu].contiguous(), 1, 1.0, scheme="systematic", ess=tau,
                                             want_flags=True)
            nu += 1
            st.d_prev = K.gather(st.d_prev.reshape(n, 1), ids, validate=False).reshape(n)
            reset = flags
            all_flags.append(int(flags[0]))
    print(f"tau {tau}: flags {all_flags} E {st.E.tolist()}")
    assert tau < 1.0 or any(all_flags)
    assert torch.equal(img, x) and torch.equal(dist, buf.norm)
    assert torch.equal(smp.last_neg_log_weights, st.E) and torch.isfinite(st.E).all()
    assert torch.equal(smp.last_resample_ids, ids) and torch.equal(smp.last_resample_flags, flags)
    assert smp.last_resample_ess.shape == (1,)


def test_neutral_settings_are_the_ddpm_loop(K, task, monkeypatch):
    """twist_scale = 0 and proposal_weight = 0: E stays 0, no image ever resamples, the particles are the ddpm loop's"""
    x0, y = task["x0"], task["y"][:1]
    smp = _sampler("smc_ddpm", str(STEPS))
    smp.twist_scale, smp.proposal_weight, smp.resample_every = 0.0, 0.0, 1
    smp.noise_draw, smp.noise_seed = "device", 5
    seen, orig = [], K.resample

    def spy(*a, **kw):
        r = orig(*a, **kw)
        seen.append((r[2].clone(), r[3].clone()))
        return r
    monkeypatch.setattr(K, "resample", spy)
    img, dist = _loop(smp, task, x0, y)
    assert len(seen) == STEPS - 1
    assert torch.equal(smp.last_neg_log_weights, torch.zeros(8, device=DEV))
    for ids, flags in seen:
        assert not bool(flags.any()) and torch.equal(ids, torch.arange(8, device=DEV))
    base = _sampler("ddpm", str(STEPS))
    base.noise_draw, base.noise_seed = "device", 5
    want, want_d, _ = _loop(base, task, x0, y)
    assert torch.equal(img, want) and torch.equal(dist, want_d)


def test_multi_image_equals_image_by_image(K, task):
    """M = 2 images x K = 4 in one loop against the two single-image loops fed their image's paths and uniforms"""
    M, k, x0, y = task["M"], task["k"], task["x0"], task["y"]

    def run(x, yy, offset, **kw):
        smp = _sampler("smc_ddpm", str(STEPS))
        smp.resample_every, smp.resample_scheme = 3, "systematic"
        smp.noise_draw, smp.noise_seed, smp.path_base = "device", 9, 100
        it = _patch_rng(smp, None, task["ubank"], offset)
        out = _loop(smp, task, x, yy, **kw)
        assert it["u"] == 3
        return out + (smp.last_neg_log_weights, smp.last_resample_ids, smp.last_resample_flags)

    img, dist, E, ids, flags = run(x0, y, 0)
    assert flags.shape == (M,) and (ids // k == torch.arange(M * k, device=DEV) // k).all()
    assert torch.equal(run(x0, y, 0, n_images=M)[0], img)
    moved = 0
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        img_m, dist_m, E_m, ids_m, flags_m = run(x0[sl], y[m:m + 1], m * k)
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m) and torch.equal(E[sl], E_m), m
        assert torch.equal(ids[sl] - m * k, ids_m) and torch.equal(flags[m:m + 1], flags_m), m
        moved += int((ids_m != torch.arange(k, device=DEV)).any())
    print(f"flags {flags.tolist()} ids {ids.tolist()}")
    assert moved >= 1                                                     # somebody moved, else this shows little


# ----------------------------------------------------------------- 8: graph capture
def test_update_corr_and_accum_capture_into_a_graph(K):
    t, ck = _inputs("64")["t"], _record("ddpm500")
    n, shape = SHAPES["64"]
    buf, st = _buf(K, t), K.SmcState(n, shape, DEV)
    d = torch.tensor([50.0, 40.0, 60.0], device=DEV)
    reset = torch.zeros(1, dtype=torch.uint8, device=DEV)

    def step():
        x, _ = K.step_update_corr(buf, t["g_unet"], ck, t["mo"], noise=t["z"], state=st)
        K.smc_accum(st, d, reset, 1, 0.01, 1, 1.0)
        return x

    want_x = step().clone()                                               # eager (also the warm-up)
    want_E, want_part = st.E.clone(), st.corr_partials.clone()
    assert torch.isfinite(want_E).all() and bool((want_E != 0).all())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x = step()
    torch.cuda.current_stream().wait_stream(side)
    st.E.zero_(), st.d_prev.zero_(), st.corr_partials.zero_(), x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(st.E, want_E) and torch.equal(st.corr_partials, want_part)
    assert torch.equal(st.d_prev, d)

