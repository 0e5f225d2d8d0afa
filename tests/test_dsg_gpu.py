"""GPU suite of spherical-Gaussian guidance (dpsx_step_update_dsg_f32, the `dsg` conditioning method).  The four sums and
the update are compared with the float64 restatement tests/dsg_ref.py inside the bounds stated at each test; the
degenerate cases, the rng form, the batch / NaN properties, the loops and the graph replay bit for bit (torch.equal).

Shapes (those of test_smc_gpu.py, each reaches one code path): N = 3, 3 x 64 x 64 (12 slots, float4 units); N = 2,
1 x 33 x 47 (scalar units, the second particle's base unaligned, a ragged last block); N = 2, 3 x 256 x 256 (192 slots);
N = 1, 1 x 520 x 520 (the slot count is capped at 256 there)."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

import dsg_ref
from standin import StandInModel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SHAPES = {"64": (3, (3, 64, 64)), "odd": (2, (1, 33, 47)), "256": (2, (3, 256, 256)), "520": (1, (1, 520, 520))}
RECORDS = ("ddpm500", "ddpm1", "ddim500")
RATES = (0.1, 0.5, 1.0)


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def _sampler(name, respacing="", eta=None):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    smp = create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing=respacing, **({} if eta is None else {"eta": eta}))
    return smp


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
        rng = np.random.RandomState(200 + len(key) + n)
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


def _dsg(K, t, ck, g, rows=None, rng=None, g_unet=True):
    sl = slice(None) if rows is None else rows
    x, stats = K.step_update_dsg(_buf(K, t, rows), t["g_unet"][sl].contiguous() if g_unet else None, ck,
                                 t["mo"][sl].contiguous(), g, noise=t["z"][sl].contiguous() if rng is None else None, rng=rng)
    return x, stats


def _flat_norm(a):
    return np.sqrt((a.reshape(a.shape[0], -1) ** 2).sum(axis=1))


# ----------------------------------------------------------------- 1 + 2: the sums and the update against the restatement
@pytest.mark.parametrize("rec", RECORDS)
@pytest.mark.parametrize("key", list(SHAPES))
def test_sums_and_update_against_the_restatement(K, key, rec):
    """Sums: each of S, Nn, C, R (the stats partials added in double) within 1e-5 sum |terms| of the restatement -- the bound
    test_smc_gpu.py derives for the same reduction and the same __expf input.  Per term: s is the restatement's own fp32
    value, so s^2 carries one rounding (6e-8); sd carries __expf's documented 4e-7, which enters s n once and n^2, sd^2
    twice (8e-7), plus two or three roundings of 6e-8; the fp32 block sum of at most 1057 terms adds at most 12 roundings
    (four serial per lane, an eight-level tree): under 2e-6 sum |terms| together, the bound is 5 x that.
    Update: D = x_next - (sample - n_ref) within 1e-4 rel-L2 (the project's parity gate) of the restatement's r m / ||m||,
    and | ||D|| - r | <= 1e-4 r, for g in {0.1, 0.5, 1.0}; g = 0 for the radius alone (its displacement from `sample` is too
    small for a relative bound).  D and not x_next: `sample` would hide the error."""
    d, ck = _inputs(key), _record(rec)
    t = d["t"]
    n, (c, h, w) = SHAPES[key]
    args = (d["sample"], d["g_mo"][:, :c], d["g_unet"], d["mo"][:, c:], d["z"], ck)
    seen = None
    for g in (0.0,) + RATES:
        x, stats = _dsg(K, t, ck, g)
        assert stats.shape == (n, K.corr_slots(c * h * w), 4) and stats.dtype == torch.float32
        seen = stats if seen is None else seen
        assert torch.equal(stats, seen)                                   # the sums do not depend on the rate
        ref = dsg_ref.restate(*args, g)
        got = stats.double().sum(dim=1).cpu().numpy()
        assert np.all(np.isfinite(got))
        for j, name in enumerate(("S", "Nn", "C", "R")):
            err, mag = np.abs(got[:, j] - ref[name]), ref["mag"][name]
            if g == 0.0:
                print(f"{key} {rec} {name}: |sum - ref| / sum|terms| max {(err / mag).max():.3e}")
            assert np.all(mag > 0) and np.all(err <= 1e-5 * mag), (name, got[:, j], ref[name])
        D = x.double().cpu().numpy() - (d["sample"].astype(np.float64) - ref["n"])
        rad = np.abs(_flat_norm(D) - ref["r"]) / ref["r"]
        rel = _flat_norm(D - ref["D"]) / _flat_norm(ref["D"])
        print(f"{key} {rec} g {g}: D rel-L2 max {rel.max():.3e}   | ||D|| - r | / r max {rad.max():.3e}")
        assert np.all(rad <= 1e-4)
        if g > 0.0:
            assert np.all(rel <= 1e-4)


# ----------------------------------------------------------------- 3: exact cases
@pytest.mark.parametrize("key", ["64", "odd"])
def test_noiseless_step_and_zero_gradient_give_sample(K, key):
    t = _inputs(key)["t"]
    # a record without noise: `sample` and zero stats; model_out, the noise and the gradients are not read
    nan = {k: (v if k == "sample" else torch.full_like(v, float("nan"))) for k, v in t.items()}
    for kw in ({}, {"rng": K.Rng(3, 0)}):
        x, stats = _dsg(K, nan, _record("ddpm0"), 0.5, **kw)
        assert torch.equal(x, t["sample"]) and torch.equal(stats, torch.zeros_like(stats))
    # a zero gradient: S = 0, the particle keeps `sample` (its -0.0 included)
    sample = t["sample"].clone()
    sample.view(-1)[::7] = -0.0
    zero = dict(t, sample=sample, g_mo=torch.zeros_like(t["g_mo"]))
    for rec in RECORDS:
        for g in (0.0, 0.1, 1.0):
            x, stats = _dsg(K, zero, _record(rec), g, g_unet=False)
            assert torch.equal(x.view(torch.int32), sample.view(torch.int32)), (rec, g)
            assert bool((stats[..., 0] == 0).all()) and bool((stats[..., 3] > 0).all())


@pytest.mark.parametrize("rec", ["ddpm500", "ddim500"])
@pytest.mark.parametrize("key", ["64", "odd", "520"])
def test_rng_form_equals_pointer_form(K, key, rec):
    t, ck = _inputs(key)["t"], _record(rec)
    n, shape = SHAPES[key]
    rng = K.Rng(seed=0x1234567890, step=500, tag=K.Rng.TAG_STEP, particle_base=5)
    z = K.randn((n,) + shape, rng, DEV)
    x_p, st_p = _dsg(K, dict(t, z=z), ck, 0.1)
    x_r, st_r = _dsg(K, t, ck, 0.1, rng=rng)
    assert torch.equal(st_r, st_p) and torch.equal(x_r, x_p)
    assert bool((st_p != _dsg(K, t, ck, 0.1)[1]).any())                   # the draw is not the seeded z
    if n > 1:                                                             # the particle-id rule: row 1 alone at base + 1
        x1, s1 = _dsg(K, t, ck, 0.1, rows=slice(1, 2), rng=rng.offset(1))
        assert torch.equal(s1[0], st_r[1]) and torch.equal(x1[0], x_r[1])


@pytest.mark.parametrize("key", ["64", "odd"])
def test_a_particle_does_not_depend_on_the_batch(K, key):
    t, ck = _inputs(key)["t"], _record("ddpm500")
    x, stats = _dsg(K, t, ck, 0.1)
    for j in range(SHAPES[key][0]):
        xj, sj = _dsg(K, t, ck, 0.1, rows=slice(j, j + 1))
        assert torch.equal(sj[0], stats[j]) and torch.equal(xj[0], x[j]), j


def test_a_nan_stays_inside_its_particle(K):
    t, ck = _inputs("64")["t"], _record("ddpm500")
    x_clean, st_clean = _dsg(K, t, ck, 0.1)
    g = t["g_unet"].clone()
    g[1, 2, 17, 5] = float("nan")
    x, stats = _dsg(K, dict(t, g_unet=g), ck, 0.1)
    keep = [0, 2]
    assert torch.equal(x[keep], x_clean[keep]) and torch.equal(stats[keep], st_clean[keep])
    assert bool(torch.isnan(stats[1]).any()) and torch.isfinite(x_clean).all()
    assert torch.equal(x[1], t["sample"][1])                              # S is NaN, not > 0: the particle keeps `sample`


# ----------------------------------------------------------------- 4: argument errors
def test_argument_errors_return_their_code_and_launch_nothing(K):
    from ctypes import byref
    from dps_ttc_amd import _lib
    t = _inputs("64")["t"]
    n, (c, h, w) = SHAPES["64"]
    lib, p = _lib.lib(), _lib.ptr
    out = torch.full_like(t["sample"], 7.0)
    stats = torch.full((n, K.corr_slots(c * h * w), 4), 7.0, device=DEV)
    gu = t["g_unet"].contiguous()
    ok, ok_rng = _record("ddpm500"), K.Rng(1, 2).rec()

    def call(sample=t["sample"], g=t["g_mo"], mo=t["mo"], noise=t["z"], r=None, rate=0.1, x=out, st=stats, n=n, ck=ok):
        return lib.dpsx_step_update_dsg_f32(p(sample), p(g), p(gu), p(mo), p(noise), None if r is None else byref(r), rate,
                                            p(x), p(st), n, c * h * w, None if ck is None else byref(ck),
                                            _lib.stream_of(out))

    zero_b = K.make_coefs(ok.a, 0.0, ok.c1, ok.c2, ok.min_log, ok.max_log, True)
    eta0 = _sampler("ddim").sample_coefs(500, eta=0.0)
    assert eta0.add_noise == 3 and eta0.min_log == 0.0
    for kw in (dict(sample=None), dict(g=None), dict(x=None), dict(st=None), dict(ck=None), dict(mo=None),
               dict(noise=None), dict(r=ok_rng), dict(ck=zero_b), dict(ck=eta0), dict(n=-1),
               dict(rate=-0.5), dict(rate=1.5), dict(rate=float("nan")), dict(rate=float("inf")),
               dict(noise=None, r=K.Rng(1, 2, 0, 0xffffffff).rec())):
        assert call(**kw) == _lib.EINVAL, kw
    assert call(n=65536) == _lib.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 7.0).all())        # nothing was launched
    assert call() == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(out, _dsg(K, t, ok, 0.1)[0])
    with pytest.raises(ValueError, match="stats"):
        K.step_update_dsg(_buf(K, t), gu, ok, t["mo"], 0.1, noise=t["z"], stats=stats[:, :, :3])
    with pytest.raises(ValueError, match="exactly one"):
        K.step_update_dsg(_buf(K, t), gu, ok, t["mo"], 0.1)


# ----------------------------------------------------------------- 5: the loops (stand-in model, 64 x 64, 4 steps)
HW, STEPS = 64, 4


@pytest.fixture(scope="module", params=["gaussian_blur", "super_resolution"])
def task(request):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    gen = torch.Generator(device=DEV).manual_seed(43)
    if request.param == "gaussian_blur":
        op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    else:
        op = get_operator("super_resolution", in_shape=(1, 3, HW, HW), scale_factor=4, device=DEV)
    cm = get_conditioning_method("dsg", op, get_noise("gaussian", sigma=0.05), guidance_rate=0.2)
    M, k = 2, 2
    y = torch.cat([op.forward(torch.rand(1, 3, HW, HW, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
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


def _by_hand(K, ref, task, x0, y, after=None):
    """K1, K2, the model's VJP and step_update_dsg composed here, the noise of step k = bank[k]"""
    n, model = x0.shape[0], task["model"]
    handle = task["op"].hip_handle(x0)
    buf = K.StepBuffers(handle, n, 3, HW, HW, DEV)
    x, dist = x0.clone(), None
    for k, idx in enumerate(range(ref.num_timesteps - 1, -1, -1)):
        xp = x.detach().requires_grad_()
        with torch.enable_grad():
            model_out = ref._call_model(model, xp, idx)
        mo, ck, noise = model_out.detach().contiguous(), ref.sample_coefs(idx), task["bank"][k, :n].contiguous()
        K.step_fwd(handle, buf, xp.detach(), mo, noise, y, ck, want_x0=False)
        K.step_bwd(handle, buf, y, 1.0, 1, ck)
        (g_unet,) = torch.autograd.grad(model_out, xp, grad_outputs=buf.g_model_out)
        x, _ = K.step_update_dsg(buf, g_unet.contiguous(), ck, mo, task["cm"].guidance_rate, noise=noise)
        dist = buf.norm
        if after is not None:
            x, dist = after(idx, x, dist)
    return x, dist


@pytest.mark.parametrize("name", ["ddpm", "ddim"])
def test_loop_equals_its_parts(K, task, name):
    """ddpm + dsg and ddim (eta = 1) + dsg against the same launches composed by hand, bit for bit; the result moved and is
    finite"""
    n = 3
    x0, y = task["x0"][:n], task["y"][:1]
    eta = 1.0 if name == "ddim" else None
    smp = _sampler(name, str(STEPS), eta=eta)
    it = _patch_rng(smp, task["bank"], task["ubank"])
    img, dist, _ = _loop(smp, task, x0, y)
    assert it["z"] == STEPS
    want, want_d = _by_hand(K, _sampler(name, str(STEPS), eta=eta), task, x0, y)
    assert torch.equal(img, want) and torch.equal(dist, want_d)
    assert torch.isfinite(img).all() and not torch.equal(img, x0)


def test_particle_groups_equal_one_chain(K, task):
    x0, y = task["x0"], task["y"][:1]
    outs = []
    for groups in (1, 2):
        smp = _sampler("ddpm", str(STEPS))
        smp.particle_groups = groups
        _patch_rng(smp, task["bank"], task["ubank"])
        outs.append(_loop(smp, task, x0, y))
        torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    # and with the noise drawn inside the launches
    outs = []
    for groups in (1, 2):
        smp = _sampler("ddpm", str(STEPS))
        smp.particle_groups, smp.noise_draw, smp.noise_seed = groups, "device", 7
        outs.append(_loop(smp, task, x0, y))
        torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_multi_image_equals_image_by_image(K, task):
    """M = 2 images x K = 2 particles in one loop against the two single-image loops fed their image's paths"""
    M, k, x0, y = task["M"], task["k"], task["x0"], task["y"]

    def run(x, yy):
        smp = _sampler("ddim", str(STEPS), eta=1.0)
        smp.noise_draw, smp.noise_seed, smp.path_base = "device", 9, 100
        return _loop(smp, task, x, yy)

    img, dist, _ = run(x0, y)
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        img_m, dist_m, _ = run(x0[sl], y[m:m + 1])
        assert torch.equal(img[sl], img_m) and torch.equal(dist[sl], dist_m), m
    assert not torch.equal(img[:k], img[k:])


def test_device_noise_does_not_depend_on_the_batch_size(K, task):
    x0, y = task["x0"], task["y"][:1]

    def run(x):
        smp = _sampler("ddpm", str(STEPS))
        smp.noise_draw, smp.noise_seed = "device", 11
        return _loop(smp, task, x, y)

    img, dist, _ = run(x0)
    img2, dist2, _ = run(x0[:2])
    assert torch.equal(img[:2], img2) and torch.equal(dist[:2], dist2)


def test_ttc_ddim_with_a_device_resampling_step_equals_its_parts(K, task):
    """ttc_ddim (eta = 1, the device draw, resample_every = 2: after idx 2 and idx 0) against its parts"""
    x0, y = task["x0"], task["y"][:1]

    def make():
        smp = _sampler("ttc_ddim", str(STEPS), eta=1.0)
        smp.resample_draw, smp.resample_every = "device", 2
        return smp

    smp = make()
    it = _patch_rng(smp, task["bank"], task["ubank"])
    img, dist = _loop(smp, task, x0, y)
    assert it["z"] == STEPS and it["u"] == 2
    nu = {"u": 0}

    def after(idx, x, d):
        if idx % 2:
            return x, d
        x, d, _ = K.resample(x, d, task["ubank"][nu["u"]].contiguous(), 1, 1.0 / 100)
        nu["u"] += 1
        return x, d

    want, want_d = _by_hand(K, make(), task, x0, y, after=after)
    assert nu["u"] == 2 and torch.equal(img, want) and torch.equal(dist, want_d)
    assert torch.isfinite(img).all()


# ----------------------------------------------------------------- 6: graph capture
def test_the_two_launches_capture_into_a_graph(K):
    t, ck = _inputs("64")["t"], _record("ddpm500")
    buf = _buf(K, t)
    stats = buf.dsg_stats()

    def step():
        buf.flip = 0
        return K.step_update_dsg(buf, t["g_unet"], ck, t["mo"], 0.1, noise=t["z"], stats=stats)[0]

    want_x = step().clone()                                               # eager (also the warm-up)
    want_stats = stats.clone()
    assert torch.isfinite(want_x).all() and not torch.equal(want_x, t["sample"])
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            x = step()
    torch.cuda.current_stream().wait_stream(side)
    stats.zero_(), x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, want_x) and torch.equal(stats, want_stats)


# ----------------------------------------------------------------- 7: the driver
def test_driver_runs_the_shipped_dsg_configs(tmp_path):
    """configs/gaussian_deblur_config_dsg.yaml + configs/diffusion_config_dsg.yaml (ddim, eta = 1) with the random-init
    model, 3 steps, in the manner of test_driver_gpu.py (its 256 x 256 images: the shipped model config's size): the
    reference's output tree"""
    from PIL import Image
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    data = tmp_path / "data"
    data.mkdir()
    rng = np.random.RandomState(0)
    img = np.kron(rng.rand(8, 8, 3), np.ones((32, 32, 1)))               # 256 x 256 blocky image
    Image.fromarray((img * 255).astype(np.uint8)).save(data / "00000.png")
    cfg = yaml.load(open(os.path.join(ROOT, "configs", "gaussian_deblur_config_dsg.yaml")), Loader=yaml.FullLoader)
    cfg["data"]["root"] = str(data)
    tpath = tmp_path / "task.yaml"
    yaml.dump(cfg, open(tpath, "w"))
    out = tmp_path / "results"
    drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"),
              "--diffusion_config", os.path.join(ROOT, "configs", "diffusion_config_dsg.yaml"),
              "--task_config", str(tpath), "--save_dir", str(out), "--n_paths", "2", "--batch_size", "2",
              "--ref_image_idxs", "0", "--timestep_respacing", "3", "--seed", "0", "--gpu", "0",
              "--dsg_guidance_rate", "0.2"])
    (sub,) = os.listdir(out)
    assert sub == "gaussian_blur_noise_sigma_0.05_dsg_guidance_rate_0.2"
    root = out / sub
    assert (root / "input" / "00000.png").exists() and (root / "label" / "00000.png").exists()
    assert (root / "recon_paths" / "00000" / "path#1.png").exists() and (root / "recon_paths" / "00000" / "path#2.png").exists()
    assert (root / "best_of_n" / "00000.png").exists()
    d = np.load(root / "00000_pathwise_distances.npy")
    assert d.shape == (2,) and np.isfinite(d).all() and (d > 0).all()
