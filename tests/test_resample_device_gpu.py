"""GPU suite: the device resampling draw (dpsx_resample_draw_seg_f32 / dpsx_resample_seg_f32).  The kernels' ids are
compared EXACTLY with the NumPy restatement of the draw rule (tests/resample_ref.py) given the kernel's own integer
weights; the fused launch with draw + gather; a segmented launch with one launch per image; and the multi-image
ttc_ddim loop / resample_update / driver with the same images run one by one -- all bit for bit (torch.equal)."""
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch
import yaml

import resample_ref as R
from standin import StandInModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = 0.01                     # 1 / resample_scale of ttc_ddim
ONE_BELOW = float(np.float32(1) - np.float32(2.0 ** -24))          # the largest fp32 below 1


@pytest.fixture(scope="module")
def K():
    from dps_ttc_amd import kernels
    return kernels


def _case(M, k, seed):
    """seeded distances [M, k] with ties, a flat segment next to non-flat ones and NaN / inf entries; uniforms [M, k]
    holding 0 and the largest fp32 below 1"""
    rng = np.random.RandomState(seed)
    d = (50.0 + 30.0 * rng.randn(M, k)).astype(np.float32)
    if k >= 2:
        d[:, 1] = d[:, 0]                                  # a tie
    if k >= 5:
        d[0, 2], d[0, 3] = np.nan, np.inf                  # never drawn
        d[-1, 4] = -np.inf
        d[:, k // 2] = d.min(axis=1, where=np.isfinite(d), initial=np.inf)      # a tie at the minimum
    if M >= 3:
        d[1, :] = 12.5                                     # a flat segment between two non-flat ones
    u = rng.rand(M, k).astype(np.float32)
    u[:, 0] = 0.0
    u[:, -1] = ONE_BELOW
    return d, u


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("k", [1, 2, 5, 64, 512, 4096])
def test_draw_equals_the_restatement(K, M, k):
    d, u = _case(M, k, 1000 * M + k)
    ids, q = K.resample_draw(torch.from_numpy(d).to(DEV), torch.from_numpy(u).to(DEV), M, INV, want_weights=True)
    ids, q = ids.cpu().numpy(), q.cpu().numpy()
    assert ids.dtype == np.int64 and q.dtype == np.int32 and ids.shape == (M * k,) and q.shape == (M * k,)
    # ids: exact, from the kernel's own integer weights and the same uniforms
    assert np.array_equal(ids, R.draw_segments(q, u, M))
    assert (ids // k == np.repeat(np.arange(M), k)).all()                   # every id inside its own segment
    for m in range(M):                          # a zero weight is never drawn (a flat segment keeps its particles)
        seg = q[m * k:(m + 1) * k]
        if (seg == seg[0]).all():
            assert np.array_equal(ids[m * k:(m + 1) * k], m * k + np.arange(k))
        else:
            assert (seg[ids[m * k:(m + 1) * k] - m * k] > 0).all()
    # q: against the restatement's fp32 weights.  Both sides compute x = (d - d_min) * inv_scale in IEEE fp32 (the library
    # is built without fused contraction) and w = exp(-x) in (0, 1].  HIP's expf is documented at 1 ulp, NumPy's SIMD exp at
    # 4 ulp at most; below 1 an ulp of w is at most 2^-24 = one unit of q, so the two w differ by at most 5 units, and the
    # two roundings to integers add at most 1/2 each: |q - q_ref| <= 6 (an integer).  w = 1 (x = 0) is exact on both sides.
    q_ref = np.concatenate([R.weights(d[m], np.float32(INV)) for m in range(M)])
    diff = np.abs(q.astype(np.int64) - q_ref)
    print(f"M={M} K={k}: max |q - q_ref| = {diff.max()} units of 2^-24")
    assert diff.max() <= 6
    flat_d = d.reshape(-1)
    assert (q[~np.isfinite(flat_d)] == 0).all()
    for m in range(M):                                                      # the best particle(s): weight exactly 2^24
        seg = d[m]
        if np.isfinite(seg).any():
            assert (q[m * k:(m + 1) * k][seg == seg[np.isfinite(seg)].min()] == R.TWO24).all()
    # without the weights: the same ids
    assert np.array_equal(K.resample_draw(torch.from_numpy(d).to(DEV), torch.from_numpy(u).to(DEV), M, INV).cpu().numpy(), ids)


def test_draw_moves_particles_and_handles_bad_uniforms(K):
    d = torch.tensor([5.0, float("nan"), 7.0, float("inf")], device=DEV)
    u = torch.linspace(0, 1, 4 * 256 + 1, device=DEV)[:-1]
    ids = K.resample_draw(d.repeat(256), u, 256, INV).reshape(256, 4) - 4 * torch.arange(256, device=DEV)[:, None]
    assert set(ids.unique().tolist()) == {0, 2}                             # index 1 and 3 are never drawn
    bad = torch.tensor([float("nan"), -3.0, 1.0, float("inf")], device=DEV)
    ids, q = K.resample_draw(d, bad, 1, INV, want_weights=True)
    assert np.array_equal(ids.cpu().numpy(), R.draw(q.cpu().numpy(), bad.cpu().numpy())) and ids.tolist() == [0, 0, 2, 2]


def test_refusals(K):
    from dps_ttc_amd import _lib
    from dps_ttc_amd._lib import DpsxError
    d = torch.rand(4097, device=DEV)
    with pytest.raises(DpsxError) as e:                                    # K = 4097: above the LDS CDF's cap
        K.resample_draw(d, torch.rand(4097, device=DEV), 1, INV)
    assert e.value.code in (_lib.EINVAL, _lib.EUNSUPPORTED)
    with pytest.raises(DpsxError):
        K.resample(torch.rand(4097, 4, device=DEV), d, torch.rand(4097, device=DEV), 1, INV)
    assert K.resample_draw(d[:4096], torch.rand(4096, device=DEV), 1, INV).shape == (4096,)
    with pytest.raises(DpsxError):                                         # the raw entry point: 10 does not split into 3
        ids = torch.empty(10, dtype=torch.int64, device=DEV)
        x = torch.rand(10, 8, device=DEV)
        _lib.check(_lib.lib().dpsx_resample_seg_f32(_lib.ptr(d), _lib.ptr(d), 3, 3, INV, _lib.ptr(x), _lib.ptr(torch.empty_like(x)),
                                                    _lib.ptr(torch.empty(10, device=DEV)), _lib.ptr(ids), None, 10, 8, None),
                   "dpsx_resample_seg_f32")
    with pytest.raises(ValueError):                                        # N not divisible by segments
        K.resample_draw(d[:10], torch.rand(10, device=DEV), 3, INV)
    with pytest.raises(ValueError):
        K.resample(torch.rand(10, 8, device=DEV), d[:10], torch.rand(10, device=DEV), 3, INV)
    with pytest.raises(ValueError):                                        # one uniform per particle
        K.resample_draw(d[:10], torch.rand(9, device=DEV), 2, INV)
    # aliased src / dst (in place, and overlapping by one particle) through the raw entry point
    n, chw = 8, 16
    buf = torch.rand(n + 1, chw, device=DEV)
    dd, uu = torch.rand(n, device=DEV), torch.rand(n, device=DEV)
    ids, d_out = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, device=DEV)
    for src, dst in ((buf[:n], buf[:n]), (buf[:n], buf[1:]), (buf[1:], buf[:n])):
        rc = _lib.lib().dpsx_resample_seg_f32(_lib.ptr(dd), _lib.ptr(uu), 1, n, INV, _lib.ptr(src), _lib.ptr(dst),
                                              _lib.ptr(d_out), _lib.ptr(ids), None, n, chw, None)
        assert rc == _lib.EINVAL
        with pytest.raises(DpsxError):
            _lib.check(rc, "dpsx_resample_seg_f32")
    rc = _lib.lib().dpsx_resample_seg_f32(_lib.ptr(dd), _lib.ptr(uu), 1, n, INV, _lib.ptr(buf[:n]), _lib.ptr(torch.empty(n, chw, device=DEV)),
                                          _lib.ptr(dd), _lib.ptr(ids), None, n, chw, None)
    assert rc == _lib.EINVAL                                               # d_out on top of d
    with pytest.raises(DpsxError):                                         # a negative or NaN inv_scale
        K.resample_draw(dd, uu, 1, -1.0)
    with pytest.raises(DpsxError):
        K.resample_draw(dd, uu, 1, float("nan"))
    torch.cuda.synchronize()


def _particles(n, shape, seed, unaligned=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if not unaligned:
        return torch.randn((n,) + shape, device=DEV, generator=g)
    flat = torch.randn(n * int(np.prod(shape)) + 1, device=DEV, generator=g)
    x = flat[1:].reshape((n,) + shape)             # contiguous, 4 bytes off a 16-byte boundary
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    return x


@pytest.mark.parametrize("shape,unaligned", [((3, 64, 64), False), ((3, 256, 256), False), ((3, 63, 63), False),
                                             ((3, 64, 64), True), ((3, 255, 255), False), ((3, 256, 256), True),
                                             ((1, 1, 4), False), ((1, 1, 1), False)])
@pytest.mark.parametrize("M,k", [(1, 8), (3, 5)])
def test_fused_equals_draw_then_gather(K, shape, unaligned, M, k):
    n = M * k
    d, u = _case(M, k, 7 * n + shape[-1])
    d, u = torch.from_numpy(d).to(DEV).reshape(-1), torch.from_numpy(u).to(DEV).reshape(-1)
    x = _particles(n, shape, n + shape[-1], unaligned)
    ids, q = K.resample_draw(d, u, M, INV, want_weights=True)
    assert not torch.equal(ids, torch.arange(n, device=DEV))                # the case moves particles
    dst, d_out, ids_f, q_f = K.resample(x, d, u, M, INV, want_weights=True)
    assert torch.equal(ids_f, ids) and torch.equal(q_f, q)
    assert dst.shape == x.shape and torch.equal(dst, K.gather(x, ids))
    assert torch.equal(d_out.view(torch.int32), K.gather(d.reshape(n, 1), ids).reshape(n).view(torch.int32))   # NaN by bits
    dst2, d2, ids2 = K.resample(x, d, u, M, INV)
    assert torch.equal(dst2, dst) and torch.equal(ids2, ids) and torch.equal(d2.view(torch.int32), d_out.view(torch.int32))


@pytest.mark.parametrize("M,k,shape", [(3, 4, (3, 64, 64)), (4, 16, (3, 256, 256)), (2, 512, (3, 16, 16)),
                                       (3, 4096, (1, 2, 2)), (5, 7, (3, 63, 63))])
def test_segmented_equals_image_by_image(K, M, k, shape):
    n = M * k
    d, u = _case(M, k, 31 * M + k)
    d, u = torch.from_numpy(d).to(DEV).reshape(-1), torch.from_numpy(u).to(DEV).reshape(-1)
    x = _particles(n, shape, 5 * n)
    dst, d_out, ids, q = K.resample(x, d, u, M, INV, want_weights=True)
    ids_d = K.resample_draw(d, u, M, INV)
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        dst_m, d_m, ids_m, q_m = K.resample(x[sl], d[sl], u[sl], 1, INV, want_weights=True)
        assert torch.equal(ids[sl] - m * k, ids_m), m
        assert torch.equal(q[sl], q_m) and torch.equal(dst[sl], dst_m), m
        assert torch.equal(d_out[sl].view(torch.int32), d_m.view(torch.int32)), m
        assert torch.equal(ids_d[sl] - m * k, K.resample_draw(d[sl], u[sl], 1, INV)), m


# ----------------------------------------------------------------- loops
def _sampler(name, respacing="20"):
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    return create_sampler(sampler=name, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                          model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                          rescale_timesteps=True, timestep_respacing=respacing)


def _patch_rng(smp, bank, ubank, offset):
    """noise and uniforms of particle p: row offset + p of the banks' next step (as test_multi_image_gpu._patch_randn)"""
    it = {"z": 0, "u": 0}

    def rnd(like, stride=None, shape=None):
        cnt = (tuple(shape) if shape is not None else tuple(like.shape))[0]
        z = bank[it["z"], offset:offset + cnt].contiguous()
        it["z"] += 1
        return z

    def uni(n, like):
        v = ubank[it["u"], offset:offset + n].contiguous()
        it["u"] += 1
        return v
    smp._randn, smp._rand = rnd, uni
    return it


def _spy_resample(smp):
    seen = []
    orig = smp._resample

    def spy(*a, **kw):
        r = orig(*a, **kw)
        seen.append(smp.last_resample_ids.clone())
        return r
    smp._resample = spy
    return seen


@pytest.mark.parametrize("task", ["gauss", "inpaint"])
def test_ttc_ddim_loop_multi_image(K, task):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    M, k, hw = 3, 4, 64
    n = M * k
    gen = torch.Generator(device=DEV).manual_seed(29)
    masks = None
    if task == "gauss":
        op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    else:
        op = get_operator("inpainting", device=DEV)
        masks = torch.from_numpy((np.random.RandomState(3).rand(M, 1, hw, hw) < 0.5).astype(np.float32)).to(DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    ys = []
    for m in range(M):
        fkw = {} if masks is None else {"mask": masks[m:m + 1]}
        ys.append(op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1, **fkw).detach())
    y = torch.cat(ys).contiguous()
    x0 = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
    bank = torch.randn(20, n, 3, hw, hw, device=DEV, generator=torch.Generator(device=DEV).manual_seed(31))
    ubank = torch.rand(2, n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(37))
    model = StandInModel().to(DEV)

    def run(x, yy, mk, offset, **kw):
        smp = _sampler("ttc_ddim")
        smp.resample_draw = "device"
        it = _patch_rng(smp, bank, ubank, offset)
        seen = _spy_resample(smp)
        fn = cm.conditioning if mk is None else partial(cm.conditioning, mask=mk)
        img, dist = smp.p_sample_loop(model=model, x_start=x.clone(), measurement=yy, measurement_cond_fn=fn, record=False,
                                      save_root=None, **kw)
        assert it["z"] == 20 and it["u"] == 2 and len(seen) == 2           # 20 steps, resampling at idx 10 and 0
        return img, dist, torch.stack(seen)

    img, dist, ids = run(x0, y, masks, 0)
    assert img.shape == x0.shape and dist.shape == (n,) and ids.shape == (2, n)
    assert (ids // k == torch.arange(n, device=DEV) // k).all()             # nobody left its image
    assert bool((ids != torch.arange(n, device=DEV)).any())                 # ... and somebody moved, else this shows nothing
    img_n, dist_n, ids_n = run(x0, y, masks, 0, n_images=M)                 # n_images names the same split
    assert torch.equal(img_n, img) and torch.equal(ids_n, ids)
    moved = 0
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        img_m, dist_m, ids_m = run(x0[sl], y[m:m + 1], None if masks is None else masks[m:m + 1], m * k)
        assert torch.equal(img[sl], img_m), m
        assert torch.equal(dist[sl], dist_m), m
        assert torch.equal(ids[:, sl] - m * k, ids_m), m
        moved += int((ids_m != torch.arange(k, device=DEV)).any())
    assert moved >= 1


def test_ttc_ddim_device_draw_single_image_matches_the_unfused_pieces(K):
    """one image, "device": the loop's fused launch = resample_draw + two gathers on the step's outputs"""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    k, hw = 6, 64
    gen = torch.Generator(device=DEV).manual_seed(41)
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.5)
    y = op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1).detach()
    x0 = torch.randn(k, 3, hw, hw, device=DEV, generator=gen)
    smp = _sampler("ttc_ddim")
    smp.resample_draw = "device"
    calls = []
    orig = K.resample

    def spy(src, d, u, segments, inv_scale, want_weights=False):
        out = orig(src, d, u, segments, inv_scale, want_weights)
        ids = K.resample_draw(d, u, segments, inv_scale)
        calls.append((segments, inv_scale, torch.equal(out[2], ids), torch.equal(out[0], K.gather(src, ids)),
                      torch.equal(out[1], K.gather(d.reshape(-1, 1), ids).reshape(-1))))
        return out
    K.resample = spy
    try:
        img, dist = smp.p_sample_loop(model=StandInModel().to(DEV), x_start=x0, measurement=y,
                                      measurement_cond_fn=cm.conditioning, record=False, save_root=None)
    finally:
        K.resample = orig
    assert calls == [(1, 0.01, True, True, True)] * 2
    assert torch.isfinite(img).all() and torch.isfinite(dist).all() and smp.last_resample_ids.shape == (k,)


def test_ttc_ddim_refusals_name_the_option(K):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise, get_operator
    M, k, hw = 2, 2, 64
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    y = torch.rand(M, 3, hw, hw, device=DEV)
    x0 = torch.randn(M * k, 3, hw, hw, device=DEV)
    model = StandInModel().to(DEV)
    noiser = get_noise("gaussian", sigma=0.05)
    ps = get_conditioning_method("ps", op, noiser, scale=0.5)

    def loop(smp, cm, **kw):
        return smp.p_sample_loop(model=model, x_start=x0.clone(), measurement=y, measurement_cond_fn=cm.conditioning,
                                 record=False, save_root=None, **kw)
    with pytest.raises(NotImplementedError, match=r"ttc_ddim.*resample_draw"):         # the default draw
        loop(_sampler("ttc_ddim", "3"), ps)
    smp = _sampler("ttc_ddim", "3")
    smp.resample_draw = "device"
    with pytest.raises(NotImplementedError, match=r"ttc_ddim.*multi-image"):           # the per-op path
        loop(smp, get_conditioning_method("mcg", op, noiser, scale=0.5))
    smp.global_resample = True
    with pytest.raises(NotImplementedError, match=r"ttc_ddim.*global"):                # several ranks
        loop(smp, ps)
    smp.global_resample = False
    with pytest.raises(ValueError):                                                    # n_images against the rows of y
        loop(smp, ps, n_images=4)
    with pytest.raises(NotImplementedError, match=r"resample_update.*resample_draw"):
        _sampler("search_ddpm", "3").resample_update(x0, x0, op, y)
    img, dist = loop(smp, ps)                                                          # and the supported form runs
    assert img.shape == x0.shape and dist.shape == (M * k,)


@pytest.mark.parametrize("potential", ["min", "mean"])
def test_resample_update_multi_image(K, potential):
    from dps_ttc_amd.measurements import get_operator
    M, k, hw = 3, 5, 64
    n = M * k
    gen = torch.Generator(device=DEV).manual_seed(43)
    op = get_operator("super_resolution", in_shape=(1, 3, hw, hw), scale_factor=4, device=DEV)
    y = torch.cat([op.forward(torch.rand(1, 3, hw, hw, device=DEV, generator=gen) * 2 - 1).detach() for _ in range(M)])
    cand = torch.randn(n, 3, hw, hw, device=DEV, generator=gen)
    den = torch.rand(n, 3, hw, hw, device=DEV, generator=gen) * 2 - 1
    prev = torch.rand(n, device=DEV, generator=gen) * 40
    ubank = torch.rand(1, n, device=DEV, generator=gen)

    def run(c, dn, yy, pc, offset, **kw):
        smp = _sampler("search_ddpm")
        _patch_rng(smp, None, ubank, offset)
        out, net = smp.resample_update(c, dn, op, yy, rs_temp=0.1, prev_costs=pc, potential_type=potential, steps_done=3,
                                       **kw)
        return out, net, smp.last_resample_ids, smp.last_curr_costs

    out, net, ids, curr = run(cand, den, y, prev, 0, resample_draw="device")
    assert bool((ids != torch.arange(n, device=DEV)).any()) and (ids // k == torch.arange(n, device=DEV) // k).all()
    inv = 0.1 / 3 if potential == "mean" else 0.1
    assert torch.equal(ids, K.resample_draw(prev, ubank[0], M, inv)) and torch.equal(out, K.gather(cand, ids))
    for m in range(M):
        sl = slice(m * k, (m + 1) * k)
        out_m, net_m, ids_m, curr_m = run(cand[sl], den[sl], y[m:m + 1], prev[sl], m * k, resample_draw="device")
        assert torch.equal(out[sl], out_m) and torch.equal(net[sl], net_m) and torch.equal(curr[sl], curr_m), m
        assert torch.equal(ids[sl] - m * k, ids_m), m
    # the attribute selects the draw as the keyword does
    smp = _sampler("search_ddpm")
    smp.resample_draw = "device"
    _patch_rng(smp, None, ubank, 0)
    out_a, net_a = smp.resample_update(cand, den, op, y, rs_temp=0.1, prev_costs=prev, potential_type=potential, steps_done=3)
    assert torch.equal(out_a, out) and torch.equal(net_a, net)


# ----------------------------------------------------------------- driver
def _setup(tmp_path):
    from PIL import Image
    data = tmp_path / "data"
    data.mkdir()
    rng = np.random.RandomState(0)
    for i in range(2):
        img = np.kron(rng.rand(8, 8, 3), np.ones((32, 32, 1)))
        Image.fromarray((img * 255).astype(np.uint8)).save(data / f"{i:05d}.png")
    cfg = yaml.load(open(os.path.join(ROOT, "configs", "gaussian_deblur_config.yaml")), Loader=yaml.FullLoader)
    cfg["data"]["root"] = str(data)
    tpath = tmp_path / "task.yaml"
    yaml.dump(cfg, open(tpath, "w"))
    diff = yaml.load(open(os.path.join(ROOT, "configs", "diffusion_config.yaml")), Loader=yaml.FullLoader)
    diff["sampler"] = "ttc_ddim"
    dpath = tmp_path / "diffusion.yaml"
    yaml.dump(diff, open(dpath, "w"))
    return str(tpath), str(dpath)


def _tree(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_driver_ttc_ddim_images_per_batch(tmp_path):
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    tpath, dpath = _setup(tmp_path)
    common = ["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
              "--task_config", tpath, "--n_paths", "2", "--batch_size", "2", "--timestep_respacing", "3", "--seed", "0",
              "--gpu", "0", "--resample_draw", "device"]
    batched, single = tmp_path / "batched", tmp_path / "single"
    drv.main(common + ["--save_dir", str(batched), "--ref_image_idxs", "0,1", "--images_per_batch", "2"])
    for idx in ("0", "1"):                                                  # what two single-image runs name
        drv.main(common + ["--save_dir", str(single), "--ref_image_idxs", idx])
    (sub,) = os.listdir(batched)
    assert os.listdir(single) == [sub]
    assert _tree(batched) == _tree(single)
    root = batched / sub
    for fname in ("00000", "00001"):
        assert (root / "input" / f"{fname}.png").exists() and (root / "label" / f"{fname}.png").exists()
        for k in (1, 2):
            assert (root / "recon_paths" / fname / f"path#{k}.png").exists()
            assert (root / "recon_paths_y" / fname / f"path#{k}_y_space.png").exists()
        d = np.load(root / f"{fname}_pathwise_distances.npy")
        assert d.shape == (2,) and np.isfinite(d).all() and (d > 0).all()
        best = int(np.argmin(d))
        a = open(root / "best_of_n" / f"{fname}.png", "rb").read()
        assert a == open(root / "recon_paths" / fname / f"path#{best + 1}.png", "rb").read()
    with pytest.raises(SystemExit, match="ttc_ddim"):                       # without the flag: the refusal of the default
        drv.main([a for a in common if a not in ("--resample_draw", "device")]
                 + ["--save_dir", str(tmp_path / "no"), "--ref_image_idxs", "0,1", "--images_per_batch", "2"])
