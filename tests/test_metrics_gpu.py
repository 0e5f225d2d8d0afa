"""GPU suite of the device image metrics (kernels.image_metrics -> dpsx_image_metrics_f32) against the float64
restatement tests/metrics_ref.py.

Bounds: |mse - ref| <= 1e-5 ref; |psnr - ref| <= 1e-4 dB (under 20 fp32 roundings per partial chain: about 1e-6 relative
on the sum, 5e-6 dB); |ssim - ref| <= 1e-5 on the `rand` / `smooth` inputs and <= 1e-4 on the ill-conditioned set (a label
of 0.9 or 0.9 + 1e-3 noise, where E[x^2] - mu^2 cancels against a C2 of 9e-4): 500x and 10x what the restatement's own
expression loses when evaluated in fp32 numpy on these families (2.0e-8 and 1.03e-5).  Every comparison prints the
kernel's error beside that fp32 figure on the same input."""
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

import metrics_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SIGMAS = (0.0, 0.01, 0.1, 0.5)                       # particle p of a batch of 4 carries SIGMAS[p]
# window positions per side: 1 | 23 x 37 (one ragged tile, two across) | 54 (two tiles, ragged) | 65 x 129 (the 32-position
# tile crossed by one on both axes, several tiles) -- and 5 x 7 for the PSNR-only scalar unit
SHAPES = [(1, 11, 11), (1, 33, 47), (3, 64, 64), (3, 75, 139)]


def _label(kind, m, shape, rng):
    a = rng.uniform(-1, 1, (m,) + shape)
    if kind == "smooth":
        a = rng.randn(m, *shape)
        for _ in range(3):                               # a few box-blur passes of noise, scaled to +-1
            p = np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge")
            a = sum(p[..., i:i + shape[1], j:j + shape[2]] for i in range(3) for j in range(3)) / 9.0
        a = a / np.abs(a).reshape(m, -1).max(axis=1)[:, None, None, None]
    return a.astype(np.float32)


def _particles(label, n, rng, sigmas=SIGMAS):
    m = label.shape[0]
    rows = np.arange(n) // (n // m)
    noise = rng.randn(n, *label.shape[1:])
    sig = np.array([sigmas[p % len(sigmas)] for p in range(n)])[:, None, None, None]
    return (label[rows] + sig * noise).astype(np.float32)


_cases = {}


def _case(shape, kind, m, n=4):
    """(x, label) of one family, built once and left unchanged"""
    key = (shape, kind, m, n)
    if key not in _cases:
        rng = np.random.RandomState(abs(hash((shape, m, n))) % (2 ** 31) + (7 if kind == "smooth" else 0))
        label = _label(kind, m, shape, rng)
        _cases[key] = (_particles(label, n, rng), label)
    return _cases[key]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(x, label, data_range=None, want=("mse", "psnr", "ssim")):
    from dps_ttc_amd import kernels
    out = kernels.image_metrics(_dev(x), _dev(label), data_range=data_range, want=want)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _close_or_same(got, ref, tol, rel=False):
    """finite references within tol; infinite / NaN ones reproduced as they are"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin, inf = np.isfinite(ref), np.isinf(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[inf], ref[inf]), (got, ref)
    err = np.abs(got[fin] - ref[fin])
    assert np.all(err <= (tol * np.abs(ref[fin]) if rel else tol)), (got, ref)
    if not err.size:
        return 0.0
    return float((err / np.maximum(np.abs(ref[fin]), 1e-300)).max()) if rel else float(err.max())


def _check(x, label, data_range, ssim_tol, tag):
    ref = metrics_ref.metrics(x, label, data_range)
    want = ("mse", "psnr", "ssim") if "ssim" in ref else ("mse", "psnr")
    got = _run(x, label, data_range, want)
    e_mse = _close_or_same(got["mse"], ref["mse"], 1e-5, rel=True)
    e_psnr = _close_or_same(got["psnr"], ref["psnr"], 1e-4)
    line = f"{tag}: mse rel {e_mse:.2e}  psnr {e_psnr:.2e} dB"
    e_ssim = e32 = 0.0
    if "ssim" in ref:
        e32 = float(np.abs(metrics_ref.ssim(x, label, data_range, dtype=np.float32).astype(np.float64) - ref["ssim"]).max())
        e_ssim = float(np.abs(got["ssim"].astype(np.float64) - ref["ssim"]).max())
        line += f"  ssim {e_ssim:.2e} (fp32 restatement {e32:.2e})"
    print(line)
    if "ssim" in ref:
        assert e_ssim <= ssim_tol, line
    return e_mse, e_psnr, e_ssim, e32


@pytest.mark.parametrize("kind", ["rand", "smooth"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_restatement(shape, kind):
    for m in (1, 2, 4):
        x, label = _case(shape, kind, m)
        for dr in (None, 2.0, 1.0):
            _check(x, label, dr, 1e-5, f"{shape} {kind} M={m} range={dr}")


def test_the_real_size_once():
    x, label = _case((3, 256, 256), "smooth", 1, n=2)
    _check(x, label, None, 1e-5, "3x256x256 smooth N=2")


def test_unaligned_particles_take_the_scalar_unit():
    """a particle batch that starts 4 bytes past a 16-byte boundary: the scalar instantiation of both partial-sum launches"""
    from dps_ttc_amd import kernels
    x, label = _case((3, 64, 64), "rand", 2)
    flat = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    xd = flat[1:].view(x.shape)
    xd.copy_(_dev(x))
    assert xd.data_ptr() % 16 == 4
    ref = metrics_ref.metrics(x, label)
    got = {k: v.cpu().numpy() for k, v in kernels.image_metrics(xd, _dev(label)).items()}
    _close_or_same(got["mse"], ref["mse"], 1e-5, rel=True)
    _close_or_same(got["psnr"], ref["psnr"], 1e-4)
    assert np.abs(got["ssim"] - ref["ssim"]).max() <= 1e-5
    only = {k: v.cpu().numpy() for k, v in kernels.image_metrics(xd, _dev(label), want=("mse", "psnr")).items()}
    assert np.array_equal(only["mse"], got["mse"]) and np.array_equal(only["psnr"], got["psnr"])


def test_psnr_only_on_a_shape_without_a_window():
    """1 x 5 x 7: 35 elements, no multiple of 4 -- the scalar unit of the PSNR-only stream; ssim is refused"""
    from dps_ttc_amd import _lib, kernels
    x, label = _case((1, 5, 7), "rand", 2)
    for dr in (None, 2.0, 1.0):
        _check(x, label, dr, 0.0, f"1x5x7 range={dr}")
    with pytest.raises(_lib.DpsxError) as e:
        kernels.image_metrics(_dev(x), _dev(label))
    assert e.value.code == _lib.EINVAL


@pytest.mark.parametrize("shape", [(3, 64, 64), (1, 33, 47)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("jitter", [0.0, 1e-3])
def test_the_ill_conditioned_set(shape, jitter):
    """label 0.9 (+ 1e-3 noise), the range given: the variances cancel against a small C2"""
    rng = np.random.RandomState(5)
    label = (0.9 + jitter * rng.randn(1, *shape)).astype(np.float32)
    x = _particles(label, 3, rng, sigmas=(0.01, 0.1, 0.5))
    for dr in (1.0, 2.0):
        _check(x, label, dr, 1e-4, f"{shape} ill jitter={jitter} range={dr}")


def test_exact_cases():
    x, label = _case((3, 64, 64), "smooth", 2)
    rows = label[np.arange(4) // 2]
    got = _run(rows, label)
    assert np.all(got["mse"] == 0.0) and np.all(got["psnr"] == np.inf) and np.abs(got["ssim"] - 1.0).max() <= 1e-6
    # a constant label, the range from the label: L = 0 -> psnr is -inf (mse > 0) or NaN (mse = 0), as the formula gives
    const = np.full((1, 3, 64, 64), 0.25, dtype=np.float32)
    xs = np.concatenate([const, const + 0.1, x[:2]]).astype(np.float32)
    ref = metrics_ref.psnr(xs, const)
    got = _run(xs, const, want=("mse", "psnr"))
    assert np.isnan(ref[0]) and np.all(ref[1:] == -np.inf)
    assert np.array_equal(np.isnan(got["psnr"]), np.isnan(ref))
    assert np.array_equal(np.sign(got["psnr"][1:]), np.sign(ref[1:])) and np.all(np.isinf(got["psnr"][1:]))
    assert got["mse"][0] == 0.0


def _bits(d):
    return {k: v.view(np.uint32) for k, v in d.items()}


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    a, b = _bits(a), _bits(b)
    assert sorted(a) == sorted(b)
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in a)


@pytest.mark.parametrize("shape", [(3, 75, 139), (1, 33, 47)], ids=lambda s: "x".join(map(str, s)))
def test_batch_independence_bit_for_bit(shape):
    x, label = _case(shape, "rand", 2)
    full = _run(x, label)
    for p in range(4):                                       # particle p of the batch == the same particle alone
        assert _same(full, _run(x[p:p + 1], label[p // 2:p // 2 + 1]), slice(p, p + 1)), p
    for b in range(2):                                       # one call with M = 2 == two calls with M = 1
        assert _same(full, _run(x[2 * b:2 * b + 2], label[b:b + 1]), slice(2 * b, 2 * b + 2)), b
    only = _run(x, label, want=("mse", "psnr"))              # the PSNR-only call == the full call's mse and psnr
    assert np.array_equal(only["mse"].view(np.uint32), full["mse"].view(np.uint32))
    assert np.array_equal(only["psnr"].view(np.uint32), full["psnr"].view(np.uint32))
    given = _run(x, label, 2.0)
    assert _same({"mse": given["mse"]}, {"mse": full["mse"]})


def test_nan_stays_where_the_definition_puts_it():
    x, label = _case((3, 75, 139), "smooth", 2)
    clean = _run(x, label)
    assert all(np.isfinite(v[1:]).all() for v in clean.values())
    bad = x.copy()
    bad[1, 2, 70, 135] = np.nan                              # in the last rows / columns: centres no window, in 1 window
    got = _run(bad, label)
    assert all(np.isnan(v[1]) for v in got.values())
    assert _same(got, clean, [0, 2, 3], [0, 2, 3])
    lab = label.copy()
    lab[1, 0, 3, 3] = np.nan                                 # label 1: image 1's particles only, range included
    got = _run(x, lab)
    assert _same(got, clean, slice(0, 2), slice(0, 2))
    assert all(np.isnan(v[2:]).all() for v in got.values())


def test_graph_capture_replays_the_eager_call():
    from dps_ttc_amd import kernels
    x, label = _case((3, 64, 64), "rand", 2)
    xd, ld = _dev(x), _dev(label)
    eager = {k: v.clone() for k, v in kernels.image_metrics(xd, ld).items()}      # also allocates the workspace
    out = {k: torch.zeros(4, dtype=torch.float32, device=DEV) for k in eager}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        kernels.image_metrics(xd, ld, out=out)
    for _ in range(2):
        for v in out.values():
            v.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in eager)


def test_compute_psnr_parity_and_the_front_ends():
    from dps_ttc_amd import metrics
    x, label = _case((3, 64, 64), "smooth", 1)
    xd, ld = _dev(x[1:]), _dev(label)
    pm = metrics.pathwise_metrics(ld, xd)
    assert sorted(pm) == ["mse", "psnr", "ssim"] and all(v.shape == (3,) and v.is_cuda for v in pm.values())
    for i in range(3):
        assert abs(float(pm["psnr"][i]) - float(metrics.compute_psnr(ld, xd[i:i + 1]))) <= 1e-4
    assert abs(float(metrics.compute_ssim(ld, xd)) - float(pm["ssim"].mean())) <= 1e-6
    assert abs(float(metrics.compute_ssim(ld[0], xd, data_range=2.0)) -
               float(metrics_ref.ssim(x[1:], label, 2.0).mean())) <= 1e-5
    with pytest.raises(ValueError):
        metrics.pathwise_metrics(ld, xd, n_images=3)


# ----------------------------------------------------------------- the per-step trace (stand-in model, 64 x 64, 4 steps)
def _trace_task(method="ps", sampler="ddpm", **params):
    from standin import StandInModel
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    from dps_ttc_amd.measurements import get_noise, get_operator
    op = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    cm = get_conditioning_method(method, op, get_noise("gaussian", sigma=0.05), **(params or dict(scale=0.3)))
    smp = create_sampler(sampler=sampler, steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="4")
    gen = torch.Generator(device=DEV).manual_seed(9)
    label = torch.rand(1, 3, 64, 64, device=DEV, generator=gen) * 2 - 1
    y = op.forward(label).detach().contiguous()
    x0 = torch.randn(3, 3, 64, 64, device=DEV, generator=gen)
    return {"op": op, "cm": cm, "smp": smp, "model": StandInModel().to(DEV), "label": label, "y": y, "x0": x0}


def _trace_loop(t, smp=None, seed=21, **kw):
    torch.manual_seed(seed)
    smp = smp or t["smp"]
    return smp.p_sample_loop(model=t["model"], x_start=t["x0"].clone().requires_grad_(), measurement=t["y"],
                             measurement_cond_fn=t["cm"].conditioning, record=False, save_root=None, **kw)


def test_metric_trace_rows():
    from dps_ttc_amd import kernels
    t = _trace_task()
    smp = t["smp"]
    plain, d_plain, _ = _trace_loop(t)
    smp.metric_trace = tr1 = kernels.MetricTrace(t["label"], every=1)
    img, d, _ = _trace_loop(t)
    assert torch.equal(img, plain) and torch.equal(d, d_plain)             # the trace changes no downstream bit
    assert tr1.data.shape == (4, 3, 4) and tr1.COLUMNS == ("mse", "psnr", "ssim", "distance")
    assert bool(torch.isfinite(tr1.data).all())
    # the last step's row (idx 0): image_metrics of the x0_hat buffer that step left, and its distance
    last = kernels.image_metrics(smp._bufs[1].x0_hat, t["label"])
    for j, k in enumerate(kernels.METRIC_NAMES):
        assert torch.equal(tr1.data[0, :, j], last[k]), k
    assert torch.equal(tr1.data[0, :, 3], smp.last_measurement_distance)
    ref = metrics_ref.metrics(smp._bufs[1].x0_hat.cpu().numpy(), t["label"].cpu().numpy())
    assert np.abs(tr1.data[0, :, 2].cpu().numpy() - ref["ssim"]).max() <= 1e-5
    assert len({float(v) for v in tr1.data[:, 0, 0]}) == 4                 # every step wrote its own row
    smp.metric_trace = tr2 = kernels.MetricTrace(t["label"], every=2)
    img2, _, _ = _trace_loop(t)
    assert torch.equal(img2, plain) and tr2.data.shape == (2, 3, 4)
    assert torch.equal(tr2.data, tr1.data[0::2])                           # idx 0 and 2: the even rows of every = 1
    smp.metric_trace = None
    assert torch.equal(_trace_loop(t)[0], plain)


def test_metric_trace_refusals_come_before_the_first_step():
    from dps_ttc_amd import kernels

    class Untouched(torch.nn.Module):
        def forward(self, *a, **kw):
            raise AssertionError("the model was called before the trace was refused")

    def refused(t, **kw):
        t["model"] = Untouched()
        t["smp"].metric_trace = kernels.MetricTrace(t["label"], every=1)
        with pytest.raises(NotImplementedError, match="metric_trace"):
            _trace_loop(t, **kw)
        assert t["smp"].metric_trace.data is None                          # nothing was allocated either

    refused(_trace_task("mcg", scale=0.3))                                 # no fused plan
    refused(_trace_task("cg", rho_scale=1.0, iters=2))                     # a cg plan
    # a DiffStateGrad projection (of a method that hands the loop its gradient: ps_semantic)
    refused(_trace_task("ps_semantic", scale=0.3, sem_guid_scale=0.0), project=True, period=2)
    t = _trace_task()
    t["smp"].particle_groups = 2
    refused(t)
    for sampler, kw in (("search_ddpm", dict(operator=None)), ("ttc_ddim", {}), ("smc_ddpm", {})):
        refused(_trace_task(sampler=sampler), **kw)
    with pytest.raises(ValueError):
        kernels.MetricTrace(None, every=0)


# ----------------------------------------------------------------- the driver
def _drive(tmp_path, caplog, name, extra):
    from test_driver_gpu import _setup
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    work = tmp_path / name
    work.mkdir()
    tpath, dpath = _setup(work, "gaussian_deblur_config.yaml", "ddpm")
    out = work / "results"
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="DPS"):
        drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
                  "--task_config", tpath, "--save_dir", str(out), "--n_paths", "4", "--batch_size", "2",
                  "--timestep_respacing", "3", "--seed", "0", "--gpu", "0",
                  *(extra if "--ref_image_idxs" in extra else ("--ref_image_idxs", "0", *extra))])
    (sub,) = os.listdir(out)
    return out / sub, [r.getMessage() for r in caplog.records]


def test_driver_device_path_metrics(tmp_path, caplog):
    root0, log0 = _drive(tmp_path, caplog, "torch", ())
    root1, log1 = _drive(tmp_path, caplog, "device", ("--path_metrics", "device"))
    npy = lambda root: sorted(f for f in os.listdir(root) if f.endswith(".npy"))
    assert npy(root0) == ["00000_pathwise_distances.npy"]                       # the default run's files are today's
    assert npy(root1) == sorted(["00000_pathwise_distances.npy"] + [f"00000_{a}_{b}.npy" for a in ("pathwise", "best_of_n")
                                                                    for b in ("psnr", "ssim")])
    assert not any("SSIM" in ln for ln in log0)
    d = np.load(root1 / "00000_pathwise_distances.npy")
    v = {f[6:-4]: np.load(root1 / f) for f in npy(root1)}
    assert all(a.shape == d.shape == (4,) for a in v.values())
    logged = [float(re.search(r"/ PSNR: (\S+) /", ln).group(1)) for ln in log0 if ln.startswith("Path#")]
    assert len(logged) == 4 and np.abs(v["pathwise_psnr"] - np.array(logged)).max() <= 1e-3
    lines = [ln for ln in log1 if ln.startswith("Path#")]
    assert len(lines) == 4 and all(re.search(r"/ PSNR: \S+ / SSIM: \S+ / distance: ", ln) for ln in lines)
    best = int(np.argmin(d))
    assert v["best_of_n_psnr"][-1] == v["pathwise_psnr"][best] and v["best_of_n_ssim"][-1] == v["pathwise_ssim"][best]
    assert v["best_of_n_psnr"][0] == v["pathwise_psnr"][0]
    assert np.all((v["pathwise_ssim"] > -1.0) & (v["pathwise_ssim"] <= 1.0))


def test_driver_device_path_metrics_multi_image(tmp_path, caplog):
    """--images_per_batch 2: each image's vectors in its own path order (group-major), against the default run's log"""
    multi = ("--ref_image_idxs", "0,1", "--images_per_batch", "2")
    _, log0 = _drive(tmp_path, caplog, "torch", multi)
    root1, log1 = _drive(tmp_path, caplog, "device", multi + ("--path_metrics", "device"))
    for fname in ("00000", "00001"):
        d = np.load(root1 / f"{fname}_pathwise_distances.npy")
        psnr, ssim = np.load(root1 / f"{fname}_pathwise_psnr.npy"), np.load(root1 / f"{fname}_pathwise_ssim.npy")
        assert d.shape == psnr.shape == ssim.shape == (4,)
        logged = {int(m.group(1)): float(m.group(2)) for m in
                  (re.match(rf"Image {fname} Path#(\d+) \|.*/ PSNR: (\S+) /", ln) for ln in log0) if m}
        assert sorted(logged) == [1, 2, 3, 4]
        assert np.abs(psnr - np.array([logged[k] for k in (1, 2, 3, 4)])).max() <= 1e-3
        assert sum(bool(re.match(rf"Image {fname} Path#\d+ \|.*/ SSIM: \S+ / distance: ", ln)) for ln in log1) == 4
        best = int(np.argmin(d))
        assert np.load(root1 / f"{fname}_best_of_n_psnr.npy")[-1] == psnr[best]
        assert np.load(root1 / f"{fname}_best_of_n_ssim.npy")[-1] == ssim[best]
