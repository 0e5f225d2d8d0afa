"""Reconstruction metrics the driver logs.  PSNR as torchmetrics' PeakSignalNoiseRatio() computes it with its
defaults (compute_metrics.py:77-90): data range = max(target) - min(target).  SSIM, the per-path vectors and the
best-of-n curve (the prefix rule of best_of_n_simple.py:20-40) come from one device call (kernels.image_metrics).
LPIPS / FID need downloaded networks and stay out of scope."""
import numpy as np
import torch


def compute_psnr(real_images, fake_images):
    real, fake = real_images.float(), fake_images.float()
    mse = torch.mean((fake - real) ** 2)
    data_range = real.max() - real.min()
    return 10.0 * torch.log10(data_range ** 2 / mse)


def compute_psnr_manual(real_images, fake_images):
    mse = torch.mean((real_images - fake_images) ** 2)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def compute_ssim(real_images, fake_images, data_range=None):
    """Mean SSIM of fake_images [N, C, H, W] against real_images ([C, H, W], [1, ...] or [M, ...], M | N): the 11 x 11
    Gaussian window (sigma 1.5), unpadded, C1 = (0.01 L)^2, C2 = (0.03 L)^2 -- skimage's and torchmetrics' convention;
    data_range None: each label's max - min, as compute_psnr.  One device call (kernels.image_metrics); the per-path
    values come from pathwise_metrics."""
    from . import kernels
    return kernels.image_metrics(fake_images, real_images, data_range=data_range, want=("ssim",))["ssim"].mean()


def pathwise_metrics(refs, samples, n_images=1):
    """The per-path metrics of samples [N, C, H, W] against refs [n_images, C, H, W] (image-major: path p belongs to
    image p // (N // n_images)) -> {"mse", "psnr", "ssim"}: [N] device tensors.  One device call, no host read; psnr is
    compute_psnr's definition per path."""
    from . import kernels
    if refs.dim() == 3:
        refs = refs.unsqueeze(0)
    if refs.shape[0] != n_images:
        raise ValueError(f"{refs.shape[0]} reference images given for n_images = {n_images}")
    return kernels.image_metrics(samples.detach(), refs)


def mean_of_n_psnr(curve, refs):
    """10 log10(L^2 / curve) for curve [M, K] (the mse of the mean of the first n paths, kernels.ensemble_stats) against
    refs [M, C, H, W]: the PSNR of the mean-of-n estimate, L = max - min of each label as compute_psnr defines it"""
    flat = refs.float().reshape(refs.shape[0], -1)
    data_range = (flat.max(dim=1).values - flat.min(dim=1).values).reshape(-1, 1)
    return 10.0 * torch.log10(data_range ** 2 / curve)


def posterior_summary(refs, samples, n_images=1, neg_log_weights=None, prior=None):
    """What the particles say together: samples [N, C, H, W] (image-major, n_images images) against refs [n_images, C, H, W]
    -> {"mean", "std" [M, C, H, W] (std = sqrt of the biased per-pixel variance), "mean_psnr", "mean_ssim", "ess" [M],
    "mean_of_n_psnr" [M, K], and the call's "var", "mean_lo", "var_lo", "info", "count" (so that the dict is the `prior` of the next particle
    group of the same images: the groups are merged, the curve continues)}.  neg_log_weights: SMC's (uniform if None).
    Two device calls (kernels.ensemble_stats, then kernels.image_metrics on the M means, each one "particle" of its own
    label), no host read."""
    from . import kernels
    if refs.dim() == 3:
        refs = refs.unsqueeze(0)
    if refs.shape[0] != n_images:
        raise ValueError(f"{refs.shape[0]} reference images given for n_images = {n_images}")
    st = kernels.ensemble_stats(samples.detach(), images=n_images, label=refs, neg_log_weights=neg_log_weights, prior=prior)
    pm = kernels.image_metrics(st["mean"], refs, want=("psnr", "ssim"))
    return {"mean": st["mean"], "std": torch.sqrt(st["var"]), "var": st["var"], "mean_lo": st["mean_lo"],
            "var_lo": st["var_lo"], "info": st["info"], "count": st["count"],
            "mean_psnr": pm["psnr"], "mean_ssim": pm["ssim"], "ess": st["info"][:, 0],
            "mean_of_n_psnr": mean_of_n_psnr(st["curve"], refs)}


def posterior_quantiles(refs, samples, n_images=1, probs=(0.05, 0.5, 0.95)):
    """The order statistics of the particles: samples [N, C, H, W] (image-major, n_images images of K <= 512 particles)
    against refs [n_images, C, H, W] -> {"quantiles" [M, q, C, H, W] (probs in [0, 1], at most 8), "hist" [M, K + 2] int32
    (the rank histogram of the label among the particles; bin K + 1: NaN), "crps" [M], "info" [M, 4] = (mean CRPS, mean
    width quantiles[-1] - quantiles[0], invalid elements, K)}.  One device call (kernels.order_stats), no host read."""
    from . import kernels
    if refs.dim() == 3:
        refs = refs.unsqueeze(0)
    if refs.shape[0] != n_images:
        raise ValueError(f"{refs.shape[0]} reference images given for n_images = {n_images}")
    return kernels.order_stats(samples.detach(), images=n_images, probs=probs, label=refs)


def posterior_pca(samples, n_images=1, components=4):
    """The principal directions of the particles' posterior uncertainty: samples [N, C, H, W] (image-major, n_images images
    of K <= 128 particles) -> {"dirs" [M, q, C, H, W], "evals", "var", "explained" [M, q], "coords" [M, K, q], "info"
    [M, 4] = (trace, rank, sweeps, K)}.  One device call (kernels.particle_pca), no host read."""
    from . import kernels
    return kernels.particle_pca(samples.detach(), images=n_images, components=components)


def pc_panels(mean, dirs, var, n_sigma=2.0):
    """(minus, plus) = mean -+ n_sigma sqrt(var_j) u_j: mean [M, C, H, W], dirs [M, q, C, H, W], var [M, q] -> two
    [M, q, C, H, W] tensors, the panels that show what component j changes in the image.  Device ops, no host read."""
    if dirs.dim() != 5 or tuple(mean.shape) != (dirs.shape[0],) + tuple(dirs.shape[2:]) or tuple(var.shape) != tuple(dirs.shape[:2]):
        raise ValueError(f"mean [M, C, H, W], dirs [M, q, C, H, W] and var [M, q] are taken (got {tuple(mean.shape)}, "
                         f"{tuple(dirs.shape)}, {tuple(var.shape)})")
    step = (float(n_sigma) * torch.sqrt(var)).reshape(*var.shape, 1, 1, 1) * dirs
    return mean.unsqueeze(1) - step, mean.unsqueeze(1) + step


def interval_coverage(hist, lo_rank, hi_rank):
    """The fraction of an image's valid elements whose label's rank lies in lo_rank .. hi_rank (both included): hist
    [M, K + 2] or [K + 2] integer rank histograms (bin K + 1, the invalid elements, is left out of the divisor) -> [M] or a
    scalar, float64.  Host arithmetic on integers: with ranks 1 .. K - 1 this is how often the label fell strictly inside
    the particles' range; a calibrated set of K particles gives (hi_rank - lo_rank + 1) / (K + 1)."""
    h = np.asarray(hist.cpu() if torch.is_tensor(hist) else hist)
    if not np.issubdtype(h.dtype, np.integer) or h.ndim not in (1, 2) or h.shape[-1] < 3:
        raise ValueError(f"hist must be an integer [M, K + 2] or [K + 2] array (got {h.dtype} {h.shape})")
    k = h.shape[-1] - 2
    lo_rank, hi_rank = int(lo_rank), int(hi_rank)
    if not 0 <= lo_rank <= hi_rank <= k:
        raise ValueError(f"ranks must satisfy 0 <= lo_rank <= hi_rank <= {k} (got {lo_rank}, {hi_rank})")
    h = h.astype(np.int64)
    inside, valid = h[..., lo_rank:hi_rank + 1].sum(axis=-1), h[..., :k + 1].sum(axis=-1)
    return inside / valid


def best_of_n_curve(distances, metric):
    """curve[n - 1] = metric[argmin(distances[:n])] for n = 1 .. len: the metric of the best-of-n pick over the first n
    paths.  The pick is np.argmin's: a NaN distance first, then the smallest, the first index among equals -- the
    library's select order."""
    d, v = np.asarray(distances).reshape(-1), np.asarray(metric).reshape(-1)
    if d.shape != v.shape:
        raise ValueError(f"{d.size} distances for {v.size} metric values")
    curve = np.empty_like(v)
    best = 0
    for n in range(d.size):
        # the prefix's pick moves only when the new path comes strictly before the current one in the select's order
        if not np.isnan(d[best]) and (np.isnan(d[n]) or d[n] < d[best]):
            best = n
        curve[n] = v[best]
    return curve
