"""GPU suite of the order statistics (include/dpsx.h "order statistics"): dpsx_quantiles_f32 against the float64
restatement tests/quantile_ref.py -- quantiles and rank histogram bit for bit, CRPS and width to 1e-5 relative (+ 1e-30),
the project's bound for its fp32-partials-then-double means -- bit for bit across batch shapes / alignments / streams /
graph replays, a planted NaN, the calibration property, and the front ends up to the driver.

The shapes sit on both sides of the register / LDS boundary (K = 64 | 65) and of the LDS route's paddings (128 | 129, 512);
the input set `dup` (every particle a copy of one of two) is joined by `same` (copies of one), on which the CRPS is
mean |x - y| and the width exactly 0.  Largest observed error as a fraction of the 1e-5 bound (each is printed): CRPS
0.012, width 0.010, CRPS of equal particles against mean |x - y| 0.005."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

import quantile_ref as Q
from test_quantile_cpu import CAL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
PROBS = (0.0, 0.05, 0.5, 0.95, 1.0)
# M, K, shape: what it exercises
SHAPES = [(1, 1, (1, 8, 8)),            # a single particle (padded to 2)
          (1, 2, (1, 8, 8)),            # the smallest network
          (2, 3, (1, 33, 47)),          # d % 4 != 0, K not a power of two, ragged last tile, unaligned second image
          (3, 16, (3, 32, 32)),         # several images, several blocks
          (1, 64, (1, 16, 16)),         # the register route's cap
          (1, 65, (1, 16, 16)),         # the LDS route's first K: two runs, 63 padded
          (1, 128, (1, 16, 16)),        # two full runs, several tiles
          (1, 129, (1, 8, 8)),          # padded to 256: a run of padding only
          (1, 512, (1, 8, 8)),          # the cap: 128 KiB of LDS
          (1, 4, (3, 256, 256))]        # the slot cap is not reached (768 blocks); the flagship image size
SETS_OF = {(3, 256, 256): ("img",)}     # the large shape once; every other shape on every set
_cache = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(m, k, shape, name, seed=0, probs=PROBS):
    """(x, label, restatement), computed once per case and never written"""
    key = (m, k, shape, name, seed, probs)
    if key not in _cache:
        x, y = Q.make_set(name, m, k, shape, seed=seed)
        _cache[key] = (x, y, Q.order_stats(x, images=m, probs=probs, label=y))
    return _cache[key]


def _run(x, m, label=None, probs=PROBS, **kw):
    from dps_ttc_amd import kernels
    r = kernels.order_stats(_dev(x) if isinstance(x, np.ndarray) else x, images=m, probs=probs,
                            label=None if label is None else (_dev(label) if isinstance(label, np.ndarray) else label), **kw)
    torch.cuda.synchronize()
    return r


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else t
    return a.view(np.int32) if a.dtype == np.float32 else a


def _close(got, ref, tag):
    """1e-5 relative + 1e-30; -> the error as a fraction of the bound"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (tag, got, ref)
    ok = ~np.isnan(ref)
    ratio = np.abs(got[ok] - ref[ok]) / (1e-5 * np.abs(ref[ok]) + 1e-30)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{tag}: error / bound = {worst:.3g}")
    assert worst <= 1.0, (tag, got, ref)
    return worst


def _check(got, ref, tag):
    assert np.array_equal(_bits(got["quantiles"]), _bits(ref["quantiles"])), tag
    if "hist" in ref:
        assert got["hist"].dtype == torch.int32 and np.array_equal(got["hist"].cpu().numpy(), ref["hist"]), tag
        _close(got["crps"].cpu().numpy(), ref["crps"], tag + " crps")
        assert torch.equal(got["crps"], got["info"][:, 0])
    info = got["info"].cpu().numpy()
    _close(info[:, 0], ref["info"][:, 0], tag + " info.crps")
    _close(info[:, 1], ref["info"][:, 1], tag + " width")
    assert np.array_equal(info[:, 2:], ref["info"][:, 2:]), tag


@pytest.mark.parametrize("m,k,shape", SHAPES, ids=[f"{m}x{k}x{'x'.join(map(str, s))}" for m, k, s in SHAPES])
def test_against_the_restatement(m, k, shape):
    for name in SETS_OF.get(shape, Q.SETS):
        x, y, ref = _case(m, k, shape, name)
        xd = _dev(x)
        got = _run(xd, m, y)
        _check(got, ref, f"{m}x{k} {name}")
        assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32))          # x is not written
        q = _bits(got["quantiles"]).reshape(m, len(PROBS), -1)
        flat = x.reshape(m, k, -1)
        if name not in ("ties",):             # p = 0 and p = 1: the minimum and the maximum with their bits
            assert np.array_equal(q[:, 0], flat.min(axis=1).view(np.int32)) and np.array_equal(q[:, -1], flat.max(axis=1).view(np.int32))


@pytest.mark.parametrize("m,k,shape", [(2, 3, (1, 33, 47)), (1, 65, (1, 16, 16))])
def test_without_a_label(m, k, shape):
    x, y, ref = _case(m, k, shape, "rand")
    got = _run(x, m)
    assert set(got) == {"quantiles", "info"}
    _check(got, Q.order_stats(x, images=m, probs=PROBS), "no label")
    assert np.array_equal(_bits(got["quantiles"]), _bits(ref["quantiles"]))               # the label changes no quantile
    info = got["info"].cpu().numpy()
    assert np.isnan(info[:, 0]).all() and (info[:, 2] == 0).all() and (info[:, 3] == k).all()


@pytest.mark.parametrize("k", (5, 64, 129))
def test_one_and_eight_probabilities(k):
    m, shape = 2, (1, 9, 13)
    eight = (1.0, 0.0, 0.5, 0.25, 0.75, 0.999, 1 / 3, 0.5)              # unordered, repeated: the width may be negative
    for probs in (eight, (0.3,)):
        for name in ("rand", "ties", "inf"):
            x, y, ref = _case(m, k, shape, name, probs=probs)
            _check(_run(x, m, y, probs=probs), ref, f"q={len(probs)} K={k} {name}")


@pytest.mark.parametrize("k", (4, 64, 65, 512))
def test_equal_particles(k):
    """`same`: crps = mean |x - y| and the width is exactly 0"""
    m, shape = 2, (1, 8, 8)
    x, y, ref = _case(m, k, shape, "same")
    got = _run(x, m, y)
    _check(got, ref, f"same K={k}")
    mad = np.abs(x.reshape(m, k, -1)[:, 0].astype(np.float64) - y.reshape(m, -1)).mean(axis=1)
    _close(got["crps"].cpu().numpy(), mad, f"same K={k} crps vs mean |x - y|")
    width = got["info"][:, 1].cpu().numpy()
    assert (width == 0).all() and not np.signbit(width).any()
    for i in range(len(PROBS)):
        assert np.array_equal(_bits(got["quantiles"][:, i]), x.reshape(m, k, *shape)[:, 0].view(np.int32))


_KEYS = ("quantiles", "hist", "info")


@pytest.mark.parametrize("m,k,shape", [(3, 16, (3, 32, 32)), (2, 3, (1, 33, 47)), (3, 65, (1, 16, 16)), (2, 129, (1, 8, 8))])
def test_batch_independence_bit_for_bit(m, k, shape):
    """M images in one call against M calls, and an image moved to another place in the batch"""
    x, y, _ = _case(m, k, shape, "inf")
    xd, yd = _dev(x).reshape(m, k, *shape), _dev(y)
    whole = _run(xd.reshape(m * k, *shape), m, yd)
    for b in range(m):
        one = _run(xd[b].contiguous(), 1, yd[b:b + 1].contiguous())
        for key in _KEYS:
            assert _same_bits(one[key][0], whole[key][b]), (key, b)
    perm = list(range(1, m)) + [0]
    moved = _run(xd[perm].contiguous().reshape(m * k, *shape), m, yd[perm].contiguous())
    for key in _KEYS:
        assert _same_bits(moved[key], whole[key][perm]), key


@pytest.mark.parametrize("m,k,shape", [(2, 8, (3, 32, 32)), (1, 65, (1, 16, 16))])
def test_an_unaligned_view_gives_the_aligned_copys_bits(m, k, shape):
    x, y, ref = _case(m, k, shape, "rand")
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].reshape(x.shape)
    view.copy_(_dev(x))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    ybuf = torch.empty(y.size + 3, dtype=torch.float32, device=DEV)
    yview = ybuf[3:].reshape(y.shape)
    yview.copy_(_dev(y))
    got, aligned = _run(view, m, yview), _run(x, m, y)
    for key in _KEYS:
        assert _same_bits(got[key], aligned[key]), key
    _check(got, ref, "unaligned")


@pytest.mark.parametrize("k", (5, 65))
def test_a_planted_nan_stays_in_its_element(k):
    m, shape = 3, (1, 12, 12)
    x, y, _ = _case(m, k, shape, "rand")
    clean = _run(x, m, y)
    xn = x.copy()
    xn[k + 2, 0, 7, 5] = np.nan                      # one particle of image 1
    got = _run(xn, m, y)
    _check(got, Q.order_stats(xn, images=m, probs=PROBS, label=y), f"nan K={k}")
    q, qc = _bits(got["quantiles"]), _bits(clean["quantiles"])
    assert (q[1, :, 0, 7, 5] == 0x7fc00000).all()
    mask = np.ones(q.shape, dtype=bool)
    mask[1, :, 0, 7, 5] = False
    assert np.array_equal(q[mask], qc[mask])
    hist, hc = got["hist"].cpu().numpy(), clean["hist"].cpu().numpy()
    assert hist[:, k + 1].tolist() == [0, 1, 0] and np.array_equal(hist[[0, 2]], hc[[0, 2]])
    assert (hist.sum(axis=1) == 144).all() and (hc[1] - hist[1])[:k + 1].sum() == 1
    assert torch.equal(got["info"][[0, 2]], clean["info"][[0, 2]]) and got["info"][1, 2] == 1
    yn = y.copy()
    yn[2, 0, 3, 3] = np.nan                          # a NaN label: the quantiles stay, the element is invalid
    got = _run(x, m, yn)
    assert np.array_equal(_bits(got["quantiles"]), qc) and got["hist"][:, k + 1].tolist() == [0, 0, 1]
    assert torch.equal(got["info"][:2], clean["info"][:2]) and bool(torch.isfinite(got["info"]).all())


@pytest.mark.parametrize("m,k,shape", [(2, 9, (3, 32, 32)), (1, 130, (1, 8, 8))])
def test_graph_capture_and_the_stream_argument(m, k, shape):
    from dps_ttc_amd import kernels
    x, y, _ = _case(m, k, shape, "img" if shape[0] == 3 else "rand")
    xd, yd = _dev(x), _dev(y)
    for label in (yd, None):
        keys = _KEYS if label is not None else ("quantiles", "info")
        eager = kernels.order_stats(xd, images=m, probs=PROBS, label=label)       # also allocates the workspace
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        on_side = kernels.order_stats(xd, images=m, probs=PROBS, label=label, stream=side)
        side.synchronize()
        for key in keys:
            assert _same_bits(on_side[key], eager[key]), key
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = kernels.order_stats(xd, images=m, probs=PROBS, label=label)
        for _ in range(2):
            for key in keys:
                out[key].fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            for key in keys:
                assert _same_bits(out[key], eager[key]), key


def _same_bits(a, b):
    """torch.equal with NaN == NaN (info[0] without a label)"""
    return np.array_equal(_bits(a), _bits(b))


def test_refusals_come_as_value_errors_before_any_launch():
    from dps_ttc_amd import kernels
    x = torch.zeros(6, 1, 4, 4, device=DEV)
    for kw in (dict(images=4), dict(images=0), dict(probs=()), dict(probs=(0.5,) * 9), dict(probs=(1.01,)),
               dict(probs=(float("nan"),)), dict(label=torch.zeros(1, 1, 4, 5, device=DEV)),
               dict(images=3, label=torch.zeros(2, 1, 4, 4, device=DEV))):
        with pytest.raises(ValueError):
            kernels.order_stats(x, **kw)
    with pytest.raises(ValueError, match="512"):
        kernels.order_stats(torch.zeros(513, 1, 2, 2, device=DEV))
    with pytest.raises(ValueError):
        kernels.order_stats(torch.zeros(6, 16, device=DEV))


def test_calibration():
    """the one statistical check: i.i.d. normal particles and label from the seed the CPU suite already passed on the
    restatement; the K + 1 = 17 valid bins each hold d / 17 within 5 standard deviations of the binomial count"""
    from dps_ttc_amd import metrics
    m, k, shape = CAL["images"], CAL["k"], CAL["shape"]
    x, y, ref = _case(m, k, shape, "rand", seed=CAL["seed"], probs=(0.05, 0.5, 0.95))
    d = int(np.prod(shape))
    got = metrics.posterior_quantiles(_dev(y), _dev(x), n_images=m)
    hist = got["hist"].cpu().numpy()
    assert np.array_equal(hist, ref["hist"]) and np.array_equal(_bits(got["quantiles"]), _bits(ref["quantiles"]))
    mean, dev = Q.calibration_bounds(d, k)
    assert hist[0, k + 1] == 0 and (np.abs(hist[0, :k + 1] - mean) <= dev).all()
    cov = metrics.interval_coverage(got["hist"], 1, k - 1)
    assert cov[0] == hist[0, 1:k].sum() / d


# ------------------------------------------------------------------ the driver
_FILES = ("posterior_quantiles", "rank_hist", "quantile_summary")


def _drive(tmp_path, monkeypatch, name, extra, paths=4):
    """the tiny settings of test_ensemble_gpu.py's driver tests, one particle group; -> (the run's output root, what
    metrics.posterior_quantiles saw, the number of order_stats calls)"""
    from test_driver_gpu import _setup
    from dps_ttc_amd import kernels, metrics
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    seen, calls, orig, orig_k = [], [], metrics.posterior_quantiles, kernels.order_stats

    def spy(refs, samples, **kw):
        seen.append((refs.clone(), samples.detach().clone(), kw))
        return orig(refs, samples, **kw)

    def spy_k(*a, **kw):
        calls.append(1)
        return orig_k(*a, **kw)
    monkeypatch.setattr(metrics, "posterior_quantiles", spy)
    monkeypatch.setattr(kernels, "order_stats", spy_k)
    work = tmp_path / name
    work.mkdir()
    tpath, dpath = _setup(work, "gaussian_deblur_config.yaml", "ddpm")
    out = work / "results"
    logging.getLogger("DPS").setLevel(logging.WARNING)
    drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
              "--task_config", tpath, "--save_dir", str(out), "--n_paths", str(paths), "--batch_size", str(paths),
              "--timestep_respacing", "3", "--seed", "0", "--gpu", "0",
              *(extra if "--ref_image_idxs" in extra else ("--ref_image_idxs", "0", *extra))])
    (sub,) = os.listdir(out)
    return out / sub, seen, calls


def _by_hand(seen, images, probs, paths=4):
    from dps_ttc_amd import kernels
    assert len(seen) == 1 and seen[0][1].shape[0] == paths * images         # one particle group of `paths` paths per image
    return kernels.order_stats(seen[0][1], images=images, probs=probs, label=seen[0][0])


def test_driver_posterior_quantiles(tmp_path, monkeypatch):
    root0, seen0, calls0 = _drive(tmp_path, monkeypatch, "off", ())
    assert not seen0 and not calls0 and not (root0 / "posterior_median").exists()      # off: nothing called, nothing written
    assert not [f for f in os.listdir(root0) if any(k in f for k in _FILES)]
    root, seen, calls = _drive(tmp_path, monkeypatch, "on", ("--posterior_quantiles", "5,50,95"))
    assert len(calls) == 1 and list(seen[0][2]["probs"]) == [0.05, 0.5, 0.95]
    want = _by_hand(seen, 1, (0.05, 0.5, 0.95))
    assert (root / "posterior_median" / "00000.png").exists()
    got = {k: np.load(root / f"00000_{k}.npy") for k in _FILES}
    assert got["posterior_quantiles"].shape == (3, 3, 256, 256) and got["posterior_quantiles"].dtype == np.float32
    assert got["rank_hist"].shape == (6,) and got["rank_hist"].dtype == np.int32 and got["rank_hist"].sum() == 3 * 256 * 256
    assert got["quantile_summary"].shape == (4,) and got["quantile_summary"][3] == 4.0
    assert np.array_equal(_bits(got["posterior_quantiles"]), _bits(want["quantiles"][0]))
    assert np.array_equal(got["rank_hist"], want["hist"][0].cpu().numpy())
    assert np.array_equal(_bits(got["quantile_summary"]), _bits(want["info"][0]))
    assert sorted(os.listdir(root0 / "recon_paths" / "00000")) == sorted(os.listdir(root / "recon_paths" / "00000"))


def test_driver_posterior_quantiles_multi_image(tmp_path, monkeypatch):
    root, seen, calls = _drive(tmp_path, monkeypatch, "multi",
                               ("--ref_image_idxs", "0,1", "--images_per_batch", "2", "--posterior_quantiles", "5,50,95"), paths=2)
    assert len(calls) == 1
    want = _by_hand(seen, 2, (0.05, 0.5, 0.95), paths=2)
    for b, fname in enumerate(("00000", "00001")):
        assert (root / "posterior_median" / f"{fname}.png").exists()
        got = {k: np.load(root / f"{fname}_{k}.npy") for k in _FILES}
        assert got["posterior_quantiles"].shape == (3, 3, 256, 256) and got["rank_hist"].shape == (4,)
        assert np.array_equal(_bits(got["posterior_quantiles"]), _bits(want["quantiles"][b]))
        assert np.array_equal(got["rank_hist"], want["hist"][b].cpu().numpy())
        assert np.array_equal(_bits(got["quantile_summary"]), _bits(want["info"][b]))
