"""GPU suite of the ensemble statistics (include/dpsx.h "ensemble statistics"): dpsx_ensemble_f32 against the float64
restatement tests/ensemble_ref.py, against the library's own pairwise distances and image metrics, bit for bit across
batch shapes / unit forms / streams / graph replays, the prior, and the front ends up to the driver.

Bounds against the restatement (the largest observed ratio of each is printed):
    mean      |d| <= 2^-23 |ref| + 2^-149          one rounding of a double result, 2 x margin
    weighted  |d| <= 1e-6 sum w |x - c| / sum w + 2^-23 |ref|        the K weight roundings, 8 x margin
    var       |d| <= 2.4e-7 ref + 2^-149           uniform and weighted alike
    curve, final mse, ESS, mean variance           1e-5 relative (the project's mse bound)"""
import logging
import os
import sys

import numpy as np
import pytest
import torch

import ensemble_ref as E
import repulse_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TINY = 2.0 ** -149
# M, K, shape: what it exercises
SHAPES = [(1, 3, (3, 64, 64)),          # float4 units
          (2, 2, (1, 33, 47)),          # scalar units, unaligned second particle, ragged last block
          (1, 4, (3, 256, 256)),        # full slot count
          (3, 16, (3, 32, 32)),         # several images
          (1, 65, (1, 16, 16)),         # K crosses the load batch and 64
          (1, 512, (1, 8, 8)),          # one slot
          (1, 4096, (1, 4, 4)),         # the cap
          (2, 1, (1, 16, 16))]          # a single particle
SETS_OF = {(3, 256, 256): ("img",)}     # the large shape once; every other shape on every set
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(m, k, shape, name, seed=0):
    """(x, label, float64 reference), computed once per case and never written"""
    key = (m, k, shape, name, seed)
    if key not in _cache:
        if name == "dup" and k == 1:
            name = "rand"
        x = R.make_set(name, m, k, shape, seed=seed)
        y = R.make_set("rand", m, 1, shape, seed=seed + 100)
        _cache[key] = (x, y, E.ensemble(x, images=m, label=y))
    return _cache[key]


def _run(x, m, label=None, **kw):
    from dps_ttc_amd import kernels
    r = kernels.ensemble_stats(_dev(x) if isinstance(x, np.ndarray) else x, images=m,
                               label=None if label is None else (_dev(label) if isinstance(label, np.ndarray) else label), **kw)
    torch.cuda.synchronize()
    return r


def _np(r):
    return {k: (v.cpu().numpy().astype(np.float64) if torch.is_tensor(v) else v) for k, v in r.items()}


def _ratio(got, ref, bound):
    """max of |got - ref| / bound over the finite reference entries (0 / 0 counts as 0)"""
    err = np.abs(got - ref)
    with np.errstate(all="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q)) if q.size else 0.0


def _check(got, ref, tag, scale=1.0, wsum=None):
    """the bounds of the module docstring, `scale` times (the prior test: 4 x); -> the observed ratios"""
    g = _np(got)
    mean_b = 2.0 ** -23 * np.abs(ref["mean"]) + TINY
    var_b = 2.4e-7 * ref["var"] + TINY
    if wsum is not None:                       # sum w |x - c| / sum w per element
        mean_b = 1e-6 * wsum + 2.0 ** -23 * np.abs(ref["mean"])
    out = {"mean": _ratio(g["mean"], ref["mean"], mean_b), "var": _ratio(g["var"], ref["var"], var_b),
           "ess": _ratio(g["info"][:, 0], ref["info"][:, 0], 1e-5 * ref["info"][:, 0]),
           "mean_var": _ratio(g["info"][:, 1], ref["info"][:, 1], 1e-5 * ref["info"][:, 1] + TINY)}
    assert np.array_equal(g["info"][:, 3], ref["info"][:, 3])
    if "curve" in ref:
        out["curve"] = _ratio(g["curve"], ref["curve"], 1e-5 * ref["curve"])
        out["final"] = max(_ratio(g["final_mse"], ref["final_mse"], 1e-5 * ref["final_mse"]),
                           _ratio(g["info"][:, 2], ref["final_mse"], 1e-5 * ref["final_mse"]))
    else:
        assert np.isnan(g["info"][:, 2]).all() and "curve" not in g
    print(f"{tag}: observed / bound " + ", ".join(f"{k} {v:.3g}" for k, v in out.items()))
    assert all(v <= scale for v in out.values()), (tag, out)
    return out


# ------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("m,k,shape", SHAPES, ids=[f"{m}x{k}x{'x'.join(map(str, s))}" for m, k, s in SHAPES])
def test_against_the_restatement(m, k, shape):
    for name in SETS_OF.get(shape, R.SETS):
        x, y, ref = _case(m, k, shape, name)
        got = _run(x, m, y)
        assert got["mean"].shape == (m,) + shape and got["var"].shape == (m,) + shape and got["curve"].shape == (m, k)
        assert got["final_mse"].shape == (m,) and got["info"].shape == (m, 4) and got["count"] == k
        _check(got, ref, f"{m}x{k}x{shape} {name}")
        if name == "dup" and k == 2 or k == 1:         # all-equal images: +0.0 bit for bit
            assert torch.equal(got["var"].view(torch.int32), torch.zeros_like(got["var"], dtype=torch.int32))
            assert float(got["info"][:, 1].abs().max()) == 0.0
        if k == 1:
            assert torch.equal(got["mean"], _dev(x))


def test_without_a_label():
    x, _, _ = _case(3, 16, (3, 32, 32), "img")
    ref = E.ensemble(x, images=3)
    got = _run(x, 3)
    _check(got, ref, "no label")
    full = _run(x, 3, _case(3, 16, (3, 32, 32), "img")[1])
    assert torch.equal(got["mean"], full["mean"]) and torch.equal(got["var"], full["var"])


@pytest.mark.parametrize("m,k,shape", [(2, 5, (3, 32, 32)), (1, 65, (1, 16, 16)), (1, 4096, (1, 4, 4))])
def test_weights_against_the_restatement(m, k, shape):
    rng = np.random.RandomState(5)
    e = (3.0 * rng.randn(m * k) + 40.0).astype(np.float32)
    e[1] = np.inf
    e[m * k - 1] = np.nan
    w = E.weights(e, m)[0]
    for name in R.SETS:
        x, y, _ = _case(m, k, shape, name)
        ref = E.ensemble(x, images=m, label=y, e=e)
        v = x.reshape(m, k, -1).astype(np.float64)
        wsum = (w[:, :, None] * np.abs(v - v[:, :1])).sum(axis=1).reshape((m,) + shape)
        got = _run(x, m, y, neg_log_weights=_dev(e))
        _check(got, ref, f"weighted {m}x{k}x{shape} {name}", wsum=wsum)
        assert torch.equal(got["curve"], _run(x, m, y)["curve"])          # always the uniform prefix


def test_weight_edge_cases_bit_for_bit():
    m, k, shape = 3, 4, (3, 16, 16)
    x, y, _ = _case(m, k, shape, "rand")
    e = np.full(m * k, np.inf, dtype=np.float32)
    e[4:8] = [np.nan, -np.inf, np.inf, np.nan]                            # images 0, 1: no finite E; image 2: one
    e[10] = 7.25
    got, uni = _run(x, m, y, neg_log_weights=_dev(e)), _run(x, m, y)
    for key in ("mean", "var", "curve", "final_mse"):
        assert torch.equal(got[key][:2], uni[key][:2]), key
    assert torch.equal(got["info"][:2], uni["info"][:2]) and got["info"][:2, 0].tolist() == [4.0, 4.0]
    assert torch.equal(got["mean"][2], _dev(x)[10]) and float(got["var"][2].abs().max()) == 0.0
    assert float(got["info"][2, 0]) == 1.0
    from dps_ttc_amd import kernels
    with pytest.raises(ValueError, match="prior"):
        kernels.ensemble_stats(_dev(x), images=m, neg_log_weights=_dev(e), prior=(4, uni["mean"], uni["var"]))


# ------------------------------------------------------------------ against code that already exists
@pytest.mark.parametrize("m,k,shape,name", [(3, 16, (3, 32, 32), "img"), (1, 65, (1, 16, 16), "rand"), (1, 512, (1, 8, 8), "neardup"),
                                            (1, 3, (3, 64, 64), "far")])
def test_cross_checks(m, k, shape, name):
    from dps_ttc_amd import kernels
    x, y, _ = _case(m, k, shape, name)
    got = _run(x, m, y)
    d = int(np.prod(shape))
    _, info = kernels.pairwise_sqdist(_dev(x), images=m, want_info=True)
    want = info[:, 2].double().cpu().numpy()
    have = 2.0 * k / (k - 1) * d * got["info"][:, 1].double().cpu().numpy()
    r1 = _ratio(have, want, 3e-5 * want)
    pm = kernels.image_metrics(got["mean"], _dev(y), want=("mse",))["mse"].double().cpu().numpy()
    r2 = _ratio(got["curve"][:, k - 1].double().cpu().numpy(), pm, 2e-5 * pm)
    r3 = _ratio(got["final_mse"].double().cpu().numpy(), pm, 2e-5 * pm)
    print(f"{m}x{k}x{shape} {name}: observed / bound: pairwise mean {r1:.3g}, curve[K - 1] {r2:.3g}, final {r3:.3g}")
    assert max(r1, r2, r3) <= 1.0


# ------------------------------------------------------------------ bit for bit
_KEYS = ("mean", "var", "curve", "final_mse", "info")


@pytest.mark.parametrize("m,k,shape", [(3, 16, (3, 32, 32)), (2, 2, (1, 33, 47)), (3, 5, (3, 64, 64))])
def test_batch_independence_bit_for_bit(m, k, shape):
    x, y, _ = _case(m, k, shape, "img")
    before = x.copy()
    xd = _dev(x)
    whole = _run(xd, m, y)
    assert torch.equal(xd, _dev(before))                                   # x is never written
    for i in range(m):                                                     # M images in one call against M calls
        one = _run(x[i * k:(i + 1) * k], 1, y[i:i + 1])
        for key in _KEYS:
            assert torch.equal(one[key][0], whole[key][i]), (key, i)
    big = np.concatenate([x[k:2 * k]] * 3 + [x[:k]])                       # an image inside a larger batch against alone
    r = _run(big, 4, np.concatenate([y[1:2]] * 3 + [y[:1]]))
    for key in _KEYS:
        assert torch.equal(r[key][3], whole[key][0]) and torch.equal(r[key][1], whole[key][1]), key


@pytest.mark.parametrize("m,k,shape", [(2, 3, (3, 64, 64)), (1, 9, (1, 32, 32))])
def test_the_scalar_form_gives_the_float4_forms_mean_and_variance(m, k, shape):
    from dps_ttc_amd import kernels
    x, y, _ = _case(m, k, shape, "img")
    xd = _dev(x)
    pad = torch.zeros(xd.numel() + 1, dtype=torch.float32, device=DEV)
    view = pad[1:].view(xd.shape)
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    a, b = _run(xd, m, y), kernels.ensemble_stats(view, images=m, label=_dev(y))
    assert torch.equal(a["mean"], b["mean"]) and torch.equal(a["var"], b["var"])
    _check(b, _case(m, k, shape, "img")[2], f"unaligned {m}x{k}x{shape}")


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_a_non_finite_value_stays_where_the_definition_puts_it(bad):
    """one element of particle 2 of the middle image of three.  The curve of that image is non-finite exactly from that
    particle on: NaN for a NaN; for an infinity the prefix mean of the element is that infinity, its squared error +inf and
    so is the mean over the elements (the float64 restatement gives the same classes)"""
    m, k, shape = 3, 4, (3, 32, 32)
    x, y, _ = _case(m, k, shape, "img")
    clean = _run(x, m, y)
    z = x.copy()
    z[k + 2, 1, 7, 9] = bad
    got, ref = _run(z, m, y), E.ensemble(z, images=m, label=y)
    keep = torch.ones((m,) + shape, dtype=torch.bool, device=DEV)
    keep[1, 1, 7, 9] = False
    for key in ("mean", "var"):
        assert torch.equal(got[key][keep], clean[key][keep]), key
    assert not bool(torch.isfinite(got["mean"][1, 1, 7, 9])) and bool(torch.isnan(got["var"][1, 1, 7, 9]))
    for key in ("curve", "final_mse", "info"):
        assert torch.equal(got[key][[0, 2]], clean[key][[0, 2]]), key
    assert torch.equal(got["curve"][1, :2], clean["curve"][1, :2])
    tail = got["curve"][1, 2:].cpu().numpy()
    assert np.isnan(tail).all() if bad != bad else (tail == np.inf).all()
    assert np.array_equal(np.isnan(tail), np.isnan(ref["curve"][1, 2:])) and not np.isfinite(ref["curve"][1, 2:]).any()
    assert not bool(torch.isfinite(got["final_mse"][1])) and not bool(torch.isfinite(got["info"][1, 1]))


def test_graph_capture_and_the_stream_argument():
    from dps_ttc_amd import kernels
    m, k, shape = 2, 9, (3, 32, 32)
    x, y, _ = _case(m, k, shape, "img")
    xd, yd = _dev(x), _dev(y)
    e = _dev((np.random.RandomState(1).randn(m * k) * 2).astype(np.float32))
    earlier = kernels.ensemble_stats(_dev(_case(m, k, shape, "rand")[0]), images=m, label=yd)      # a prior with low parts
    keys = _KEYS + ("mean_lo", "var_lo")
    for kw in ({}, {"neg_log_weights": e}, {"prior": earlier}, {"prior": (9, earlier["mean"], earlier["var"])}):
        eager = kernels.ensemble_stats(xd, images=m, label=yd, **kw)      # also allocates the workspace
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        on_side = kernels.ensemble_stats(xd, images=m, label=yd, stream=side, **kw)
        side.synchronize()
        for key in keys:
            assert torch.equal(on_side[key], eager[key]), key
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = kernels.ensemble_stats(xd, images=m, label=yd, **kw)
        for _ in range(2):
            for key in keys:
                out[key].fill_(-7.0)
            g.replay()
            torch.cuda.synchronize()
            for key in keys:
                assert torch.equal(out[key], eager[key]), key


# ------------------------------------------------------------------ the prior
def _two_groups(name):
    m, shape = 2, (3, 32, 32)
    x, y, ref = _case(m, 16, shape, name)
    v = x.reshape(m, 16, *shape)
    first = _run(v[:, :8].reshape(m * 8, *shape), m, y)
    second = _run(v[:, 8:].reshape(m * 8, *shape), m, y, prior=first)
    return v, y, ref, first, second


@pytest.mark.parametrize("name", R.SETS)
def test_two_groups_merged_through_the_prior(name):
    """Two groups of 8 against one call of 16, at 4 x the single-call bounds.  The prior is the first call's dict: its fp32
    mean and var with the low parts their rounding dropped.  (The fp32 triple alone would miss: 2^-25 |mean8| against
    2^-21 |mean16| where the two group means nearly cancel; the pooled M2 where the variance is 1e-6 of mean^2.)"""
    m, shape = 2, (3, 32, 32)
    v, y, ref, first, second = _two_groups(name)
    assert second["count"] == 16 and first["count"] == 8
    merged = dict(second)
    merged["curve"] = torch.cat([first["curve"], second["curve"]], dim=1)         # the curve continues at n = 9
    _check(merged, ref, f"prior {name}", scale=4.0)


def test_the_prior_forms_and_the_prior_is_not_written():
    """a call depends on its arguments alone: the five-tuple equals the dict whatever ran in between, and nothing the
    prior holds is written"""
    m, shape = 2, (3, 32, 32)
    v, y, ref, first, second = _two_groups("img")
    b = v[:, 8:].reshape(m * 8, *shape)
    keep = {key: first[key].clone() for key in ("mean", "var", "mean_lo", "var_lo")}
    _run(_case(m, 8, shape, "rand")[0], m, y)                              # another call of the same shape in between
    again = _run(b, m, y, prior=(8, first["mean"], first["var"], first["mean_lo"], first["var_lo"]))
    assert all(torch.equal(again[key], second[key]) for key in _KEYS + ("mean_lo", "var_lo"))
    assert all(torch.equal(first[key], keep[key]) for key in keep)
    lo = first["mean_lo"].double().abs().cpu().numpy()                     # a low part is below half an ulp of its fp32 value
    assert (lo <= 2.0 ** -24 * np.abs(first["mean"].double().cpu().numpy()) + TINY).all()
    from dps_ttc_amd import kernels
    with pytest.raises(ValueError, match="pair"):
        kernels.ensemble_stats(_dev(b), images=m, prior=(8, first["mean"], first["var"], first["mean_lo"], None))


def test_the_fp32_triple_alone():
    """a prior without low parts is the definition with the fp32 mean0 / var0 as they are: the restatement fed the same
    triple, at the single-call bounds"""
    m, shape = 2, (3, 32, 32)
    for name in ("img", "neardup"):
        v, y, _, first, second = _two_groups(name)
        b = v[:, 8:].reshape(m * 8, *shape)
        ref = E.ensemble(b, images=m, label=y, prior=(8, first["mean"].cpu().numpy(), first["var"].cpu().numpy()))
        got = _run(b, m, y, prior=(8, first["mean"], first["var"]))
        _check(got, ref, f"fp32 triple, {name}")
        zeros = torch.zeros_like(first["mean"])
        same = _run(b, m, y, prior=(8, first["mean"], first["var"], zeros, zeros))
        assert all(torch.equal(same[key], got[key]) for key in _KEYS)


# ------------------------------------------------------------------ the front ends
def test_posterior_summary():
    from dps_ttc_amd import kernels, metrics
    m, k, shape = 2, 6, (3, 32, 32)
    x, y, _ = _case(m, k, shape, "img")
    xd, yd = _dev(x), _dev(y)
    s = metrics.posterior_summary(yd, xd, n_images=m)
    st = kernels.ensemble_stats(xd, images=m, label=yd)
    pm = kernels.image_metrics(st["mean"], yd)
    assert torch.equal(s["mean"], st["mean"]) and torch.equal(s["std"], torch.sqrt(st["var"]))
    assert torch.equal(s["mean_psnr"], pm["psnr"]) and torch.equal(s["mean_ssim"], pm["ssim"])
    assert torch.equal(s["ess"], st["info"][:, 0]) and s["ess"].tolist() == [6.0, 6.0]
    want = E.mean_of_n_psnr(st["curve"].cpu().numpy(), (y.reshape(m, -1).max(axis=1) - y.reshape(m, -1).min(axis=1)))
    assert s["mean_of_n_psnr"].shape == (m, k) and np.abs(s["mean_of_n_psnr"].cpu().numpy() - want).max() <= 1e-4
    # the mean beats the paths it is made of (img: independent noise around a shared base)
    paths = kernels.image_metrics(xd, yd, want=("psnr",))["psnr"].reshape(m, k)
    assert bool((s["mean_of_n_psnr"][:, -1] > paths.max(dim=1).values).all())
    nxt = metrics.posterior_summary(yd, xd, n_images=m, prior=s)
    assert nxt["count"] == 2 * k and torch.equal(nxt["ess"], torch.full((m,), 2.0 * k, device=DEV))


def test_smc_weights_through_the_driver_helper():
    """one smc_ddpm loop with the stand-in model (64 x 64, 4 steps): --posterior_weights smc's arrays are ensemble_stats
    called by hand on the returned samples and last_neg_log_weights"""
    from test_metrics_gpu import _trace_loop, _trace_task
    from dps_ttc_amd import kernels, metrics
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    t = _trace_task(sampler="smc_ddpm")
    out = _trace_loop(t)
    sample = (out[0] if isinstance(out, tuple) else out).detach()
    e = t["smp"].last_neg_log_weights
    assert e is not None and e.shape == (3,)
    acc = drv.PosteriorSummary(t["label"], "smc")
    acc.add(sample, t["smp"])
    st = kernels.ensemble_stats(sample, images=1, label=t["label"], neg_log_weights=e)
    assert torch.equal(acc.last["mean"], st["mean"]) and torch.equal(acc.last["std"], torch.sqrt(st["var"]))
    assert torch.equal(acc.last["ess"], st["info"][:, 0]) and 1.0 <= float(st["info"][0, 0]) <= 3.0
    uni = kernels.ensemble_stats(sample, images=1, label=t["label"])
    assert torch.equal(acc.curves[0], metrics.mean_of_n_psnr(uni["curve"], t["label"]))
    if not bool((e == e[0]).all()):
        assert not torch.equal(uni["mean"], st["mean"])


def _drive(tmp_path, monkeypatch, name, extra):
    """the tiny settings of test_metrics_gpu.py's driver tests; -> (the run's output root, the particle groups the summary saw)"""
    from test_driver_gpu import _setup
    from dps_ttc_amd import metrics
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    seen, orig = [], metrics.posterior_summary

    def spy(refs, samples, **kw):
        seen.append((refs.clone(), samples.detach().clone()))
        return orig(refs, samples, **kw)
    monkeypatch.setattr(metrics, "posterior_summary", spy)
    work = tmp_path / name
    work.mkdir()
    tpath, dpath = _setup(work, "gaussian_deblur_config.yaml", "ddpm")
    out = work / "results"
    logging.getLogger("DPS").setLevel(logging.WARNING)
    drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
              "--task_config", tpath, "--save_dir", str(out), "--n_paths", "4", "--batch_size", "2",
              "--timestep_respacing", "3", "--seed", "0", "--gpu", "0",
              *(extra if "--ref_image_idxs" in extra else ("--ref_image_idxs", "0", *extra))])
    (sub,) = os.listdir(out)
    return out / sub, seen


_FILES = ("posterior_std", "mean_of_n_psnr", "posterior_summary")


def _by_hand(seen, images):
    from dps_ttc_amd import kernels, metrics
    assert len(seen) == 2                                                  # two particle groups of two paths per image
    refs = seen[0][0]
    a = kernels.ensemble_stats(seen[0][1], images=images, label=refs)
    b = kernels.ensemble_stats(seen[1][1], images=images, label=refs, prior=a)
    pm = kernels.image_metrics(b["mean"], refs, want=("psnr", "ssim"))
    curve = metrics.mean_of_n_psnr(torch.cat([a["curve"], b["curve"]], dim=1), refs)
    std = torch.sqrt(b["var"])
    rec = torch.stack([pm["psnr"], pm["ssim"], b["info"][:, 0], std.flatten(1).mean(dim=1)], dim=1)
    return std.cpu().numpy(), curve.cpu().numpy(), rec.cpu().numpy()


def test_driver_posterior_summary(tmp_path, monkeypatch):
    root0, seen0 = _drive(tmp_path, monkeypatch, "off", ())
    assert not seen0 and not (root0 / "posterior_mean").exists()           # off: nothing launched, nothing written
    assert not [f for f in os.listdir(root0) if any(k in f for k in _FILES)]
    root, seen = _drive(tmp_path, monkeypatch, "on", ("--posterior_summary",))
    std, curve, rec = _by_hand(seen, 1)
    assert (root / "posterior_mean" / "00000.png").exists()
    got = {k: np.load(root / f"00000_{k}.npy") for k in _FILES}
    assert got["posterior_std"].shape == (3, 256, 256) and got["mean_of_n_psnr"].shape == (4,) and got["posterior_summary"].shape == (4,)
    assert np.load(root / "00000_pathwise_distances.npy").shape == got["mean_of_n_psnr"].shape
    assert np.array_equal(got["posterior_std"], std[0]) and np.array_equal(got["mean_of_n_psnr"], curve[0])
    assert np.array_equal(got["posterior_summary"], rec[0]) and got["posterior_summary"][2] == 4.0
    assert sorted(os.listdir(root0 / "recon_paths" / "00000")) == sorted(os.listdir(root / "recon_paths" / "00000"))


def test_driver_posterior_summary_multi_image(tmp_path, monkeypatch):
    root, seen = _drive(tmp_path, monkeypatch, "multi", ("--ref_image_idxs", "0,1", "--images_per_batch", "2", "--posterior_summary"))
    std, curve, rec = _by_hand(seen, 2)
    for b, fname in enumerate(("00000", "00001")):
        assert (root / "posterior_mean" / f"{fname}.png").exists()
        got = {k: np.load(root / f"{fname}_{k}.npy") for k in _FILES}
        assert got["posterior_std"].shape == (3, 256, 256) and got["mean_of_n_psnr"].shape == (4,)
        assert np.array_equal(got["posterior_std"], std[b]) and np.array_equal(got["mean_of_n_psnr"], curve[b])
        assert np.array_equal(got["posterior_summary"], rec[b])
