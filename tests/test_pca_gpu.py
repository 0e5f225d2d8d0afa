"""GPU suite of the principal components (include/dpsx.h "principal components"): dpsx_pca_f32 against the float64
restatement tests/pca_ref.py, its own consistency (scores against directions, reconstruction, total variance against
kernels.ensemble_stats, d2 against kernels.pairwise_sqdist), the degenerate sets, bit-for-bit equality across batch
shapes / calls / streams / graph replays, and the front ends up to the driver.

The bounds are 4 x the largest value observed on the MI355X over all cases, rounded up to one digit; every test prints
`error / bound` before it asserts.  Observed -> bound:
    eigenvalues  |l_j - l_ref,j| / l_ref,0                      4.6e-6 -> 2e-5
    directions   |u_j -+ u_ref,j| gap_j (first four, planted)   3.7e-7 -> 2e-6
    norms        | |u_j| - 1 |                                  2.4e-6 -> 1e-5
    angles       |u_i . u_j| gap_ij                             1.8e-6 -> 7e-6
all four at K = 127 / 128.  The first is rounding in an fp32 Jacobi method on a K x K matrix (a value above 1e-4 would be a
wrong kernel, not an imprecise one); the others inherit it through the eigenvectors.  The scores against the returned
directions (observed 1.4e-6) and the reconstruction (3.0e-6) are held to the eigenvalue bound times sqrt(l_0)."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

import pca_ref as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TAU_L, TAU_U, TAU_N, TAU_O = 2e-5, 2e-6, 1e-5, 7e-6
MAX_SWEEPS = 24
QNAN = 0x7fc00000
# M, K, shape: what it exercises
SHAPES = [(1, 1, (1, 8, 8)),            # a single particle: zeros
          (1, 2, (1, 1, 7)),            # one rotation
          (2, 3, (1, 33, 47)),          # odd K (a bye per round), d % 4 != 0, unaligned second image
          (1, 9, (1, 1, 7)),            # rank limited by D: the null rule
          (3, 16, (3, 32, 32)),         # several images, several blocks
          (1, 64, (3, 16, 16)),         # the 64-wide instantiation's cap
          (1, 127, (3, 16, 16)),        # odd K in the 128-wide instantiation
          (1, 128, (3, 16, 16)),        # the cap: 129 KiB of LDS
          (1, 8, (3, 256, 256))]        # several element ranges, the flagship image size
SETS_OF = {(3, 256, 256): ("planted",)}      # the large shape once
IDS = [f"{m}x{k}x{'x'.join(map(str, s))}" for m, k, s in SHAPES]
_cache, _worst = {}, {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(m, k, shape, name, q=4):
    """(x, restatement), computed once per case and never written"""
    key = (m, k, shape, name, q)
    if key not in _cache:
        x = P.make_set(name, m, k, shape)
        _cache[key] = (x, P.pca(x, images=m, components=q))
    return _cache[key]


def _run(x, m, q=4, **kw):
    from dps_ttc_amd import kernels
    r = kernels.particle_pca(_dev(x) if isinstance(x, np.ndarray) else x, images=m, components=q, **kw)
    torch.cuda.synchronize()
    return r


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else t
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _bound(value, bound, tag, what):
    """print error / bound (and the largest so far of its kind), then assert"""
    ratio = float(value) / bound
    _worst[what] = max(_worst.get(what, 0.0), float(value))
    print(f"{tag} {what}: {float(value):.3g} = {ratio:.3g} of the bound (largest so far {_worst[what]:.3g})")
    assert ratio <= 1.0, (tag, what, value, bound)


def _healthy(got, k, tag):
    info = got["info"].cpu().numpy()
    assert (info[:, 3] == k).all() and (info[:, 1] >= 0).all(), (tag, info)
    assert (info[:, 2] < MAX_SWEEPS).all(), (tag, info)


_KEYS = ("dirs", "evals", "var", "explained", "coords", "info")


@pytest.mark.parametrize("m,k,shape", SHAPES, ids=IDS)
def test_against_the_restatement(m, k, shape):
    """eigenvalues, directions (planted), norms and angles against the float64 restatement; scores against the returned
    directions; the trace against the ensemble's variance"""
    from dps_ttc_amd import kernels
    for name in SETS_OF.get(shape, ("planted", "iid")):
        tag = f"{m}x{k} {name}"
        x, ref = _case(m, k, shape, name)
        xd = _dev(x)
        got = _run(xd, m)
        _healthy(got, k, tag)
        assert _same_bits(xd, x)                                                           # x is not written
        ev, dirs, coords, info = _np(got["evals"]), _np(got["dirs"]).reshape(m, 4, -1), _np(got["coords"]), _np(got["info"])
        flat = x.reshape(m, k, -1).astype(np.float64)
        if k == 1:
            for key in ("dirs", "evals", "coords"):
                assert not _bits(got[key]).any(), key
            assert (info[:, :3] == 0).all()
            continue
        ens = kernels.ensemble_stats(xd, images=m)
        total = _np(ens["info"])[:, 1] * flat.shape[2]
        assert np.allclose(info[:, 0] / k, total, rtol=1e-5, atol=0), (tag, info[:, 0] / k, total)
        assert np.allclose(info[:, 0], ref["info"][:, 0], rtol=1e-5, atol=0)
        assert np.allclose(_np(got["var"]), ev / k, rtol=1e-6) and np.allclose(_np(got["explained"]), ev / info[:, 0:1], rtol=1e-6)
        for b in range(m):
            l0, live = ref["evals"][b, 0], ev[b] > 0
            _bound(np.abs(ev[b] - ref["evals"][b]).max() / l0, TAU_L, f"{tag}[{b}]", "eigenvalue")
            assert (np.diff(ev[b]) <= 0).all()
            if name == "planted":
                for j in range(min(4, int(ref["info"][b, 1]))):
                    err = min(np.linalg.norm(dirs[b, j] - ref["dirs"][b, j]), np.linalg.norm(dirs[b, j] + ref["dirs"][b, j]))
                    _bound(err * ref["gap"][b, j], TAU_U, f"{tag}[{b}] u{j}", "direction")
            xc = flat[b] - flat[b].mean(axis=0)
            for j in np.flatnonzero(live):
                _bound(abs(np.linalg.norm(dirs[b, j]) - 1), TAU_N, f"{tag}[{b}] u{j}", "norm")
                for i in range(j):
                    gap = abs(ref["lam"][b, i] - ref["lam"][b, j]) / l0
                    _bound(abs(dirs[b, i] @ dirs[b, j]) * gap, TAU_O, f"{tag}[{b}] u{i}.u{j}", "angle")
                c = coords[b, :, j]
                _bound(np.abs(c - xc @ dirs[b, j]).max() / np.sqrt(l0), TAU_L, f"{tag}[{b}] c{j}", "score")
                assert c[np.argmax(np.abs(c))] > 0
            for j in np.flatnonzero(~live):                                                # null: +0.0 everywhere
                assert not _bits(got["dirs"][b, j]).any() and not _bits(got["coords"][b, :, j]).any()


@pytest.mark.parametrize("m,k,shape", [s for s in SHAPES if 2 <= s[1] <= 9], ids=[i for i, s in zip(IDS, SHAPES) if 2 <= s[1] <= 9])
def test_reconstruction(m, k, shape):
    """q = 8 >= rank: x_i - mean = sum_j c_ij u_j"""
    for name in SETS_OF.get(shape, ("planted", "iid")):
        x, ref = _case(m, k, shape, name, q=8)
        got = _run(x, m, q=8)
        _healthy(got, k, f"{m}x{k} {name}")
        assert (ref["info"][:, 1] <= 8).all()
        flat = x.reshape(m, k, -1).astype(np.float64)
        dirs, coords = _np(got["dirs"]).reshape(m, 8, -1), _np(got["coords"])
        for b in range(m):
            assert got["info"][b, 1] == ref["info"][b, 1]
            res = flat[b] - flat[b].mean(axis=0) - coords[b] @ dirs[b]
            _bound(np.linalg.norm(res, axis=1).max() / np.sqrt(ref["evals"][b, 0]), TAU_L, f"{m}x{k} {name}[{b}]", "reconstruction")
            _bound(np.abs(_np(got["evals"])[b] - ref["evals"][b]).max() / ref["evals"][b, 0], TAU_L, f"{m}x{k} {name}[{b}] q=8", "eigenvalue")


@pytest.mark.parametrize("m,k,shape", SHAPES[:-1], ids=IDS[:-1])
def test_d2_is_pairwise_sqdist(m, k, shape):
    from dps_ttc_amd import kernels
    x, _ = _case(m, k, shape, "iid")
    xd = _dev(x)
    got = _run(xd, m, want_d2=True)
    want = kernels.pairwise_sqdist(xd, images=m)
    torch.cuda.synchronize()
    assert got["d2"].shape == (m, k, k) and _same_bits(got["d2"], want)
    plain = _run(xd, m)
    assert "d2" not in plain
    for key in _KEYS:
        assert _same_bits(plain[key], got[key]), key


@pytest.mark.parametrize("m,k,shape", SHAPES[:-1], ids=IDS[:-1])
def test_degenerate_sets(m, k, shape):
    """same: +0.0 everywhere, rank 0.  dup: one component, l_0 = |a - b|^2 n_a n_b / K.  nan: the flagged image is the
    canonical NaN with rank -1, every other image keeps the clean run's bits"""
    q = 3
    got = _run(P.make_set("same", m, k, shape), m, q=q)
    for key in ("dirs", "evals", "coords", "var"):
        assert not _bits(got[key]).any(), key
    info = got["info"].cpu().numpy()
    assert not _bits(info[:, :3]).any() and (info[:, 3] == k).all()

    x = P.make_set("dup", m, k, shape)
    got = _run(x, m, q=q)
    info, ev = _np(got["info"]), _np(got["evals"])
    flat = x.reshape(m, k, -1).astype(np.float64)
    if k == 1:
        assert (info[:, 1] == 0).all() and not ev.any()
    else:
        _healthy(got, k, "dup")
        na, nb = P.dup_counts(k)
        for b in range(m):
            want = ((flat[b, 0] - flat[b, -1]) ** 2).sum() * na * nb / k
            assert info[b, 1] == 1 and not _bits(got["evals"][b, 1:]).any() and not _bits(got["dirs"][b, 1:]).any()
            _bound(abs(ev[b, 0] - want) / want, TAU_L, f"dup {m}x{k}[{b}]", "eigenvalue")
            u = _np(got["dirs"][b, 0]).reshape(-1)
            step = (flat[b, 0] - flat[b, -1]) / np.linalg.norm(flat[b, 0] - flat[b, -1])
            assert abs(abs(u @ step) - 1) <= TAU_N

    xn = P.make_set("nan", m, k, shape)
    clean, got = _run(P.make_set("planted", m, k, shape), m, q=q), _run(xn, m, q=q)
    bad = min(P.NAN_AT[0], m - 1)
    if k == 1:                                   # one particle: zeros whatever it holds
        assert not _bits(got["dirs"]).any() and (got["info"][:, 1] == 0).all()
        return
    for key in ("dirs", "evals", "coords"):
        assert (_bits(got[key][bad]) == QNAN).all(), key
    assert torch.isnan(got["var"][bad]).all() and torch.isnan(got["explained"][bad]).all()
    info = got["info"].cpu().numpy()
    assert _bits(info[bad, 0:1])[0] == QNAN and info[bad, 1] == -1 and info[bad, 2] == 0 and info[bad, 3] == k
    rest = [b for b in range(m) if b != bad]
    for key in _KEYS:
        assert _same_bits(got[key][rest], clean[key][rest]), key


@pytest.mark.parametrize("m,k,shape", [(3, 16, (3, 32, 32)), (2, 3, (1, 33, 47)), (3, 65, (1, 16, 16))])
def test_batch_independence_bit_for_bit(m, k, shape):
    """M images in one call against M calls, an image moved to another place in the batch, and the same call twice"""
    x = P.make_set("planted", m, k, shape)
    xd = _dev(x).reshape(m, k, *shape)
    whole, again = _run(xd.reshape(m * k, *shape), m, want_d2=True), _run(xd.reshape(m * k, *shape), m, want_d2=True)
    _healthy(whole, k, "whole")
    for key in _KEYS + ("d2",):
        assert _same_bits(whole[key], again[key]), key
    for b in range(m):
        one = _run(xd[b].contiguous(), 1, want_d2=True)
        for key in _KEYS + ("d2",):
            assert _same_bits(one[key][0], whole[key][b]), (key, b)
    perm = list(range(1, m)) + [0]
    moved = _run(xd[perm].contiguous().reshape(m * k, *shape), m)
    for key in _KEYS:
        assert _same_bits(moved[key], whole[key][perm]), key


@pytest.mark.parametrize("m,k,shape,q", [(2, 9, (3, 32, 32), 4), (1, 100, (1, 9, 13), 8)])
def test_graph_capture_and_the_stream_argument(m, k, shape, q):
    from dps_ttc_amd import kernels
    xs = [_dev(P.make_set(name, m, k, shape)) for name in ("planted", "iid")]
    xd = xs[0].clone()
    eager = [kernels.particle_pca(x, images=m, components=q, want_d2=True) for x in xs]    # also allocates the workspace
    torch.cuda.synchronize()
    keys = _KEYS + ("d2",)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    on_side = kernels.particle_pca(xd, images=m, components=q, want_d2=True, stream=side)
    side.synchronize()
    for key in keys:
        assert _same_bits(on_side[key], eager[0][key]), key
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = kernels.particle_pca(xd, images=m, components=q, want_d2=True)
    for turn in (1, 0):                          # the inputs are rewritten between the replays
        xd.copy_(xs[turn])
        for key in keys:
            out[key].fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        for key in keys:
            assert _same_bits(out[key], eager[turn][key]), (key, turn)


def test_refusals_come_as_value_errors_before_any_launch():
    from dps_ttc_amd import kernels
    x = torch.zeros(6, 1, 4, 4, device=DEV)
    for kw in (dict(images=4), dict(images=0), dict(components=0), dict(components=9), dict(components=2.5)):
        with pytest.raises(ValueError):
            kernels.particle_pca(x, **kw)
    with pytest.raises(ValueError, match="128"):
        kernels.particle_pca(torch.zeros(129, 1, 2, 2, device=DEV))
    with pytest.raises(ValueError):
        kernels.particle_pca(torch.zeros(6, 16, device=DEV))


def test_the_workspace_cache_keeps_the_families_apart():
    """particle_pca and pairwise_sqdist on the same six particles: the same d2 bits (include/dpsx.h), from two workspaces --
    the one cache keys on the size query's name, not on the shape alone"""
    from dps_ttc_amd import kernels
    x = _dev(P.make_set("planted", 1, 6, (3, 16, 16)))
    mine = lambda query: {k: v for k, v in kernels._workspaces.items() if k[0] == query and k[2:] == (6, 768, 1)}
    got = _run(x, 1, want_d2=True)
    d2 = kernels.pairwise_sqdist(x, images=1)
    torch.cuda.synchronize()
    assert _same_bits(got["d2"], d2)
    pca_ws, rep_ws = mine("dpsx_pca_workspace_bytes"), mine("dpsx_repulse_workspace_bytes")
    assert len(pca_ws) == len(rep_ws) == 1
    (a,), (b,) = pca_ws.values(), rep_ws.values()
    assert a is not b and a.data_ptr() != b.data_ptr() and a.numel() == 1536 and b.numel() == 1280
    again = _run(x, 1, want_d2=True)                                     # a hit: the same tensor, the same bits
    assert [id(v) for v in mine("dpsx_pca_workspace_bytes").values()] == [id(a)]
    assert all(_same_bits(again[k], got[k]) for k in ("d2", "dirs", "evals", "coords", "info"))


def test_the_labels_of_the_images():
    """kernels._label_rows(label, x, images): one label serves every image (expanded), otherwise one per image"""
    from dps_ttc_amd import kernels
    x = torch.zeros(6, 1, 4, 4, device=DEV)
    one, three = torch.rand(1, 4, 4, device=DEV), torch.rand(3, 1, 4, 4, device=DEV)
    got = kernels._label_rows(one, x, 3)
    assert got.shape == (3, 1, 4, 4) and got.is_contiguous() and all(torch.equal(got[i], one) for i in range(3))
    assert torch.equal(kernels._label_rows(three, x, 3), three) and kernels._label_rows(one, x, 1).shape == (1, 1, 4, 4)
    assert kernels._label_rows(three, x).shape == (3, 1, 4, 4)            # without `images`: M | N is all that is asked
    with pytest.raises(ValueError, match=r"^3 labels given for 2 images$"):
        kernels._label_rows(three, x, 2)
    with pytest.raises(ValueError, match=r"^3 labels given for 1 images$"):
        kernels._label_rows(three, x, 1)
    with pytest.raises(ValueError, match=r"^4 labels do not divide 6 particles$"):
        kernels._label_rows(torch.zeros(4, 1, 4, 4, device=DEV), x, 4)
    with pytest.raises(ValueError, match="does not match particles"):
        kernels._label_rows(torch.zeros(1, 4, 5, device=DEV), x, 3)
    with pytest.raises(ValueError, match="for particles on"):
        kernels._label_rows(torch.zeros(1, 4, 4, device=DEV), x.cpu(), 3)


def test_front_ends():
    from dps_ttc_amd import kernels, metrics
    m, k, shape = 2, 9, (3, 32, 32)
    x, _ = _case(m, k, shape, "planted")
    xd = _dev(x)
    got, want = metrics.posterior_pca(xd, n_images=m, components=3), _run(xd, m, q=3)
    for key in _KEYS:
        assert _same_bits(got[key], want[key]), key
    mean = kernels.ensemble_stats(xd, images=m)["mean"]
    minus, plus = metrics.pc_panels(mean, got["dirs"], got["var"])
    torch.cuda.synchronize()
    step = (2.0 * torch.sqrt(got["var"])).reshape(m, 3, 1, 1, 1) * got["dirs"]
    assert torch.allclose(plus - mean.unsqueeze(1), step, atol=1e-6) and torch.allclose(mean.unsqueeze(1) - minus, step, atol=1e-6)


# ------------------------------------------------------------------ the driver
_FILES = ("posterior_pcs", "pca_summary", "pca_coords")


def _drive(tmp_path, monkeypatch, name, extra, paths=4):
    """the tiny settings of test_quantile_gpu.py's driver tests, one particle group; -> (the run's output root, what
    metrics.posterior_pca saw, the number of particle_pca calls)"""
    from test_driver_gpu import _setup
    from dps_ttc_amd import kernels, metrics
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    seen, calls, orig, orig_k = [], [], metrics.posterior_pca, kernels.particle_pca

    def spy(samples, **kw):
        seen.append((samples.detach().clone(), kw))
        return orig(samples, **kw)

    def spy_k(*a, **kw):
        calls.append(1)
        return orig_k(*a, **kw)
    monkeypatch.setattr(metrics, "posterior_pca", spy)
    monkeypatch.setattr(kernels, "particle_pca", spy_k)
    work = tmp_path / name
    work.mkdir()
    tpath, dpath = _setup(work, "gaussian_deblur_config.yaml", "ddpm")
    out = work / "results"
    logging.getLogger("DPS").setLevel(logging.WARNING)
    drv.main(["--model_config", os.path.join(ROOT, "configs", "model_config.yaml"), "--diffusion_config", dpath,
              "--task_config", tpath, "--save_dir", str(out), "--n_paths", str(paths), "--batch_size", str(paths),
              "--timestep_respacing", "3", "--seed", "0", "--gpu", "0", "--ref_image_idxs", "0", *extra])
    (sub,) = os.listdir(out)
    return out / sub, seen, calls


def test_driver_posterior_pca(tmp_path, monkeypatch):
    from dps_ttc_amd import kernels
    root0, seen0, calls0 = _drive(tmp_path, monkeypatch, "off", (), paths=1)
    assert not seen0 and not calls0 and not (root0 / "posterior_pca").exists()            # off: nothing called, nothing written
    assert not [f for f in os.listdir(root0) if any(k in f for k in _FILES)]
    root, seen, calls = _drive(tmp_path, monkeypatch, "on", ("--posterior_pca", "3"))
    assert len(calls) == 1 and len(seen) == 1 and seen[0][1] == dict(n_images=1, components=3) and seen[0][0].shape[0] == 4
    want = kernels.particle_pca(seen[0][0], images=1, components=3)
    got = {k: np.load(root / f"00000_{k}.npy") for k in _FILES}
    assert got["posterior_pcs"].shape == (3, 3, 256, 256) and got["posterior_pcs"].dtype == np.float32
    assert got["pca_summary"].shape == (3, 2) and got["pca_coords"].shape == (4, 3)
    assert _same_bits(got["posterior_pcs"], want["dirs"][0]) and _same_bits(got["pca_coords"], want["coords"][0])
    assert _same_bits(got["pca_summary"][:, 0], want["var"][0]) and _same_bits(got["pca_summary"][:, 1], want["explained"][0])
    assert sorted(os.listdir(root / "posterior_pca")) == sorted(f"00000_pc{j}_{s}.png" for j in range(3) for s in ("minus", "plus"))
    assert len(os.listdir(root / "recon_paths" / "00000")) == 4                           # the paths themselves as without it
