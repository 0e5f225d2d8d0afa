"""GPU suite: the driver's one image loop (run_images) without a UNet -- two images as one batch of two (--images_per_batch
2) and as two batches of one (the default mode) write the same files."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
HW, K = 64, 2
#: what the stand-in sampler adds to an image's label: AMP[g, i] x one fixed pattern for particle i of group g, so the
#: distances order as AMP does (the blur is linear) -- group-major: path#3, #2, #4, #1
AMP = ((0.30, 0.10), (0.05, 0.20))


def _driver():
    sys.path.insert(0, ROOT)
    import sample_condition_batched_ttc as drv
    return drv


def _labels():
    rng = np.random.RandomState(0)
    imgs = [np.kron(rng.rand(3, 8, 8), np.ones((1, HW // 8, HW // 8))) for _ in range(2)]        # blocky, as the driver tests'
    return [torch.from_numpy((2.0 * img - 1.0).astype(np.float32)) for img in imgs]


def _standin(labels, operator):
    """-> (sample_fn, calls).  sample_fn ignores x_start: it finds the images of the call by their measurements (the
    noiser adds nothing) and returns, image-major, label_b + AMP[g, i] * pattern for the g-th call with these images"""
    dev_labels = torch.stack(labels).to(DEV)
    ys = [operator.forward(dev_labels[j:j + 1]) for j in range(len(labels))]
    pattern = torch.from_numpy(np.random.RandomState(1).randn(3, HW, HW).astype(np.float32)).to(DEV)
    calls, seen = [], {}

    def sample_fn(x_start, measurement, record, save_root, **kw):
        images = tuple(next(j for j, y in enumerate(ys) if torch.equal(y[0], m)) for m in measurement)
        assert x_start.shape == (len(images) * K, 3, HW, HW) and record is False
        g = seen.get(images, 0)
        seen[images] = g + 1
        calls.append((images, g, kw))
        return torch.stack([dev_labels[j] + AMP[g][i] * pattern for j in images for i in range(K)]).contiguous()
    return sample_fn, calls


def run_mode(drv, out_path, per_batch, n_paths, flags, call=None):
    """the two images through the driver's loop in batches of `per_batch` -> (log lines, the stand-in's calls).  call: how
    one batch is run (default: drv.run_images)"""
    from dps_ttc_amd.measurements import get_operator
    labels = _labels()
    operator = get_operator("gaussian_blur", kernel_size=61, intensity=3.0, device=DEV)
    sample_fn, calls = _standin(labels, operator)
    args = drv.parse_args(["--batch_size", str(K), "--n_paths", str(n_paths), "--images_per_batch", str(per_batch),
                           "--ref_image_idxs", "0,1", *flags])
    for d in ("input", "recon_paths", "label", "best_of_n"):
        os.makedirs(os.path.join(out_path, d))
    lines = []
    logger = SimpleNamespace(info=lines.append)
    sampler = SimpleNamespace(last_neg_log_weights=None)
    for n, batch in enumerate(drv.image_batches([0, 1], per_batch)):
        if call is not None:
            call(args, logger, labels, batch, operator, sample_fn, n_paths // K, out_path, sampler)
            continue
        run = drv.Run(args, logger, torch.device(DEV), 0, 1, labels, operator, lambda y: y, "gaussian_blur", None, None,
                      sample_fn, None, sampler, "ddpm", n_paths // K, out_path)
        drv.run_images(run, batch, n)
    return lines, calls


def tree(root):
    """{relative path: bytes} of every file under root"""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("n_paths,flags", [
    (2 * K, ("--path_metrics", "device", "--path_diversity", "--posterior_summary")),
    (K, ("--posterior_quantiles", "5,50,95", "--posterior_pca", "2")),
])
def test_one_batch_of_two_images_equals_two_batches_of_one(tmp_path, n_paths, flags):
    """Every file of the two modes is equal byte for byte -- inputs, labels, the PNGs of every path, best_of_n, the
    distances and every analysis file of the two flag sets: the driver before run_images (its run_image_batch against the
    loop in its main(), same stand-ins) already wrote equal bytes in its two modes for all of them, so no file needs a
    tolerance.  The best path is the argmin of the saved distances in group-major path order."""
    drv = _driver()
    groups = n_paths // K
    lines_b, calls_b = run_mode(drv, str(tmp_path / "batch"), 2, n_paths, flags)
    lines_s, calls_s = run_mode(drv, str(tmp_path / "single"), 1, n_paths, flags)
    # the sampler is told the number of images only in the multi-image mode; a batch's measurements come in pick order
    assert [(c[0], c[1]) for c in calls_b] == [((0, 1), g) for g in range(groups)]
    assert all(c[2] == {"n_images": 2} for c in calls_b)
    assert [(c[0], c[1]) for c in calls_s] == [((j,), g) for j in (0, 1) for g in range(groups)]
    assert all(c[2] == {} for c in calls_s)
    batch, single = tree(tmp_path / "batch"), tree(tmp_path / "single")
    assert sorted(batch) == sorted(single)
    for fname in ("00000", "00001"):
        for name in [f"{fname}_pathwise_distances.npy", f"best_of_n/{fname}.png", f"input/{fname}.png", f"label/{fname}.png",
                     *(f"recon_paths/{fname}/path#{p + 1}.png" for p in range(n_paths)),
                     *(f"recon_paths_y/{fname}/path#{p + 1}_y_space.png" for p in range(n_paths))]:
            assert name in batch, name
    if "--posterior_summary" in flags:
        for name in ("00000_pathwise_psnr.npy", "00001_best_of_n_ssim.npy", "00000_path_diversity.npy",
                     "posterior_mean/00001.png", "00000_posterior_std.npy", "00001_mean_of_n_psnr.npy",
                     "00000_posterior_summary.npy"):
            assert name in batch, name
    else:
        for name in ("00000_posterior_quantiles.npy", "posterior_median/00001.png", "00000_rank_hist.npy",
                     "00001_quantile_summary.npy", "00000_posterior_pcs.npy", "00001_pca_summary.npy", "00000_pca_coords.npy",
                     "posterior_pca/00001_pc1_plus.png"):
            assert name in batch, name
    differ = [name for name in sorted(batch) if batch[name] != single[name]]
    assert not differ, differ
    order = np.argsort(np.asarray(AMP[:groups]).reshape(-1))
    for lines, tag in ((lines_b, "Image {}: "), (lines_s, "")):
        for j, fname in enumerate(("00000", "00001")):
            d = np.load(tmp_path / "batch" / f"{fname}_pathwise_distances.npy")
            assert d.shape == (n_paths,) and d.dtype == np.float32 and np.array_equal(np.argsort(d), order)
            best = int(np.argmin(d))
            said = [ln for ln in lines if ln.startswith(tag.format(fname) + f"best-of-{n_paths} = ")]
            assert len(said) == (1 if tag else 2) and said[0 if tag else j].startswith(
                tag.format(fname) + f"best-of-{n_paths} = path#{best + 1} | PSNR: "), said
            assert batch[f"best_of_n/{fname}.png"] == batch[f"recon_paths/{fname}/path#{best + 1}.png"]
    assert lines_b[0] == f"Inference for images 00000, 00001 (2 x {K} particles per call)"
    assert [ln for ln in lines_s if ln.startswith("Inference")] == ["Inference for image 0", "Inference for image 1"]
    assert sum(ln.startswith("Image 00001 Path#") for ln in lines_b) == n_paths
    assert sum(ln.startswith("Path#") for ln in lines_s) == 2 * n_paths
