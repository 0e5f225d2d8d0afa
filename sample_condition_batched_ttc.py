#!/usr/bin/env python3
"""Driver counterpart of the reference's sample_condition_batched_ttc.py (same CLI, same three YAML files, same
output tree) on the MI355X hot path.

    python sample_condition_batched_ttc.py --model_config=configs/model_config.yaml \
        --diffusion_config=configs/diffusion_config.yaml --task_config=configs/gaussian_deblur_config.yaml \
        --n_paths=64 --batch_size=64 --ref_image_idxs=0 --gpu=0

For every reference image: y = A(x) + n once, then `n_paths // batch_size` particle groups of `batch_size`
particles through `sampler.p_sample_loop` (fused DPS loop for `sampler: ddpm`, per-step best-of-N for
`sampler: search_ddpm`), PSNR per particle, PNGs of input / label / every path, and the best-of-N pick by
measurement distance (best_of_n_simple.py semantics, on device).

Differences from the reference script, all fixes of things that crash there: `--l1` exists,
the sampler returns a tensor for this call signature, LPIPS is logged only if torchmetrics is installed.
`--images_per_batch M` runs up to M reference images per sampler call, `batch_size` particles each, with one
measurement (and, for inpainting, one mask) per image: M x batch_size particles in one launch sequence, the select of
`search_ddpm` and the best-of-N per image.  One rank only; not with `--embedder`; `ttc_ddim` needs
`--resample_draw device` (its per-image resampling draw).
With `torchrun --nproc-per-node G` (the reference shards by hand: run0.sh:12 / run1.sh:13 start one process per GPU
with its own --path_start_idx) the particle groups are sharded contiguously over the ranks and the best-of-N pick is
global: RCCL all-gather of the distances, winner broadcast from its owner.  `sampler: search_ddpm` then selects over
all ranks' particles at every step and `sampler: ttc_ddim` resamples over all of them (SURVEY.md 8e ii-iii).
"""
import argparse
import math
import os
from functools import partial
from typing import NamedTuple

# read by the HSA runtime when it initialises (first HIP call): must be in the environment before that, i.e. before anything
# below touches the GPU -- the host driver only supports dmabuf IPC, RCCL fails with hipIpcGetMemHandle otherwise
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")          # one hardware queue per HIP stream (particle groups, RCCL)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from dps_ttc_amd import distributed as dd  # noqa: E402
from dps_ttc_amd.condition_methods import get_conditioning_method  # noqa: E402
from dps_ttc_amd.data import get_dataset, to_minus1_1  # noqa: E402
from dps_ttc_amd.gaussian_diffusion import create_sampler  # noqa: E402
from dps_ttc_amd.img_utils import clear_color, mask_generator  # noqa: E402
from dps_ttc_amd.measurements import get_noise, get_operator  # noqa: E402
from dps_ttc_amd.metrics import compute_psnr, pathwise_metrics  # noqa: E402
from dps_ttc_amd.unet import create_model  # noqa: E402


def load_yaml(file_path: str) -> dict:
    with open(file_path) as f:
        return yaml.load(f, Loader=yaml.FullLoader)     # the task files carry !!python/tuple tags


def get_logger():
    import logging
    logger = logging.getLogger(name='DPS')
    if not logger.handlers:
        logger.setLevel(logging.INFO)
        h = logging.StreamHandler()
        h.setFormatter(logging.Formatter("%(asctime)s [%(name)s] >> %(message)s"))
        logger.addHandler(h)
    return logger


def imsave(path, array):
    try:
        import matplotlib.pyplot as plt
        plt.imsave(path, array)
    except ImportError:
        from PIL import Image
        a = (np.clip(array, 0, 1) * 255).astype(np.uint8)
        Image.fromarray(a).save(path)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--model_config', type=str)
    p.add_argument('--diffusion_config', type=str)
    p.add_argument('--task_config', type=str)
    p.add_argument('--gpu', type=int, default=0)
    p.add_argument('--save_dir', type=str, default='./results_search')
    p.add_argument('--n_data_samples', type=int, default=1)
    p.add_argument('--n_paths', type=int, default=1)
    p.add_argument('--resample_every_steps', type=int, default=10)
    p.add_argument('--potential_type', type=str, default='curr')
    p.add_argument('--rs_temp', type=float, default=0.1)
    p.add_argument('--start_idx', type=int, default=0)
    p.add_argument('--path_start_idx', type=int, default=0)
    p.add_argument('--batch_size', type=int, default=1)
    p.add_argument('--anneal_scale', type=float, default=10)
    p.add_argument('--anneal_amp', type=float, default=1)
    p.add_argument('--anneal_loc', type=float, default=0.5)
    p.add_argument('--kernel_idx', type=int, default=0)
    p.add_argument('--ref_image_idxs', type=str, default='4')
    # additions
    p.add_argument('--l1', type=float, default=0.0, help='(the reference reads args.l1 without defining it)')
    p.add_argument('--timestep_respacing', type=str, default=None, help='override the diffusion YAML (e.g. "100")')
    p.add_argument('--seed', type=int, default=None)
    p.add_argument('--embedder', type=str, default=None,
                   help="'module:factory' -- factory(device) returns the embedding network of the semantic-guidance term "
                        "(ps_semantic with sem_guid_scale != 0); default: facenet_pytorch's InceptionResnetV1 as in the reference")
    p.add_argument('--guid_image', type=str, default=None,
                   help='guidance image for --embedder (PNG, 256x256); default: the reference image itself (oracle guidance, '
                        'for plumbing runs)')
    p.add_argument('--particle_groups', type=int, default=1,
                   help='run the batch_size particles of a fused DPS loop as this many independent sub-batches, each on its '
                        'own HIP stream with its own operator handle (kernels.ParticleGroups; results per particle unchanged)')
    p.add_argument('--images_per_batch', type=int, default=1,
                   help='run up to this many reference images per sampler call, batch_size particles each, with one '
                        'measurement (and inpainting mask) per image; selects and best-of-N stay per image')
    p.add_argument('--resample_draw', type=str, default='multinomial', choices=('multinomial', 'device'),
                   help='the resampling draw of ttc_ddim: torch.multinomial over all particles (default, the '
                        "reference's draw) or the library's per-image draw fused with the particle gather "
                        '(one launch; required for --images_per_batch > 1 with ttc_ddim)')
    p.add_argument('--resample_scheme', type=str, default='multinomial', choices=('multinomial', 'stratified', 'systematic'),
                   help='the scheme of the device draw: independent uniforms (default), one uniform per stratum, or one '
                        'uniform per image (systematic: never loses the best particle); needs --resample_draw device')
    p.add_argument('--resample_ess', type=float, default=None,
                   help='resample an image only while its effective sample size is below this fraction of its particles '
                        '(in [0, 1]; default: whenever its weights differ); decided on the device; needs --resample_draw device')
    p.add_argument('--ttc_resample_every', type=int, default=10,
                   help='ttc_ddim resamples after every step whose index is a multiple of this (1 with --resample_ess 0.5: '
                        'adaptive SMC)')
    p.add_argument('--noise_draw', type=str, default='torch', choices=('torch', 'device'),
                   help="the step noise and x_start: torch.randn over the whole batch (default) or the library's "
                        'counter-based draw keyed on (--seed, step, path id, element): a path then draws the same noise '
                        'whatever --batch_size, --particle_groups, --images_per_batch and the number of ranks are')
    p.add_argument('--smc_twist_scale', type=float, default=None,
                   help='smc_ddpm: the weight of the distance difference in the particle log-weights (default 0.01)')
    p.add_argument('--smc_twist_power', type=int, default=None, choices=(1, 2),
                   help='smc_ddpm: the power of the distance in the twist (default 1)')
    p.add_argument('--smc_proposal_weight', type=float, default=None,
                   help='smc_ddpm: the weight of the proposal correction log p_model - log q_guided (default 1: the exact '
                        'twisted-SMC weight; 0: the difference potential alone)')
    p.add_argument('--dsg_guidance_rate', type=float, default=None,
                   help='dsg: overrides the task config\'s guidance_rate in [0, 1] (0: the drawn noise direction, 1: the '
                        'steepest-descent direction)')
    p.add_argument('--pgdm_iters', type=int, default=None,
                   help='pgdm: overrides the task config\'s iters, the CG iterations of the solve per step, in [0, 64]')
    p.add_argument('--pgdm_weighting', type=str, default=None, choices=('score', 'paper'),
                   help='pgdm: overrides the task config\'s weighting (score: consistent with the guided score; paper: '
                        'the weights of the PiGDM paper)')
    p.add_argument('--pgdm_weight', type=float, default=None,
                   help='pgdm: overrides the task config\'s weight, a multiplier on the guidance term (1: the method\'s own)')
    p.add_argument('--solver_order', type=int, default=None, choices=(1, 2),
                   help='ddim / ttc_ddim: overrides the diffusion config\'s solver_order (1: the DDIM rule, 2: the '
                        'DPM-Solver++(2M) multistep update; eta 0 or 1, ps-type methods, one rank for ttc_ddim)')
    p.add_argument('--guidance_gain', type=str, default=None, choices=('unit', 'span'),
                   help='unit: every kept step shifts by scale * gradient (the reference); span: scale is multiplied by '
                        'the base timesteps the kept step covers (a heuristic for respaced loops; not for dsg / cg)')
    p.add_argument('--beam_width', type=int, default=1,
                   help='search_ddpm: keep this many best proposals per image and step instead of one (beam search); '
                        'must divide batch_size; one rank only')
    p.add_argument('--path_metrics', type=str, default='torch', choices=('torch', 'device'),
                   help='torch: PSNR per path in a host loop (one read per particle).  device: PSNR and SSIM of a particle '
                        'group in one device call and one copy; also writes {fname}_pathwise_psnr.npy / _pathwise_ssim.npy '
                        'and the best-of-n curves {fname}_best_of_n_psnr.npy / _best_of_n_ssim.npy; one rank only')
    p.add_argument('--repulsion_scale', type=float, default=0.0,
                   help='ddpm / ddim / ttc_ddim: after every step push the particles of an image apart (kernel-weighted '
                        'particle repulsion) with strength repulsion_scale * beta_t; 0: off')
    p.add_argument('--repulsion_bandwidth', type=float, default=None,
                   help='the repulsion kernel\'s bandwidth as a mean squared per-element difference (default: the mean '
                        'squared distance of the image\'s particles / ln(K + 1))')
    p.add_argument('--repulsion_stop', type=float, default=0.0,
                   help='no repulsion on the steps with t / T below this fraction (the last steps of the trajectory)')
    p.add_argument('--path_diversity', action='store_true',
                   help='write {fname}_path_diversity.npy: per particle group the [mean, min] RMS per-element distance '
                        'between its final samples (min 0: duplicates); one rank only')
    p.add_argument('--posterior_summary', action='store_true',
                   help='per image write posterior_mean/{fname}.png, {fname}_posterior_std.npy (per-pixel std of the paths), '
                        '{fname}_mean_of_n_psnr.npy (PSNR of the mean of the first n paths, in the path order of '
                        '{fname}_pathwise_distances.npy) and {fname}_posterior_summary.npy = [mean PSNR, mean SSIM, ESS, '
                        'mean std]; one device call per particle group; one rank only')
    p.add_argument('--posterior_weights', type=str, default='uniform', choices=('uniform', 'smc'),
                   help='--posterior_summary: uniform, or smc: the final importance weights of sampler smc_ddpm '
                        '(one particle group only)')
    p.add_argument('--posterior_quantiles', type=str, default=None, metavar='P1,P2,...',
                   help='percentages in [0, 100], at most 8 (e.g. 5,50,95): per image write {fname}_posterior_quantiles.npy '
                        '[q, C, H, W] (per-pixel quantiles of the paths), posterior_median/{fname}.png (with 50 among them), '
                        '{fname}_rank_hist.npy (rank histogram of the label among the paths, [K + 2]) and '
                        '{fname}_quantile_summary.npy = [mean CRPS, mean width, invalid pixels, K]; one particle group of at '
                        'most 512 paths; one rank only')
    p.add_argument('--posterior_pca', type=int, default=None, metavar='Q',
                   help='1 <= Q <= 8 principal components of the paths per image: write {fname}_posterior_pcs.npy [Q, C, H, W] '
                        '(unit directions), {fname}_pca_summary.npy [Q, 2] = (variance along it, share of the total variance), '
                        '{fname}_pca_coords.npy [K, Q] (the score of every path) and '
                        'posterior_pca/{fname}_pc{j}_{minus,plus}.png = mean -+ 2 sigma_j u_j; one particle group of at most '
                        '128 paths; one rank only')
    args = p.parse_args(argv)
    if args.path_diversity and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise SystemExit("--path_diversity runs on one rank only: the per-group distances are not gathered between ranks "
                         f"(WORLD_SIZE={os.environ['WORLD_SIZE']})")
    if args.path_metrics == 'device' and int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise SystemExit("--path_metrics device runs on one rank only: the per-path metric vectors are not gathered between "
                         f"ranks (WORLD_SIZE={os.environ['WORLD_SIZE']})")
    return args


def save_path_metrics(out_path, fname, distances, psnr, ssim):
    """--path_metrics device: the per-path metrics in the path order of {fname}_pathwise_distances.npy and the
    best-of-n curves over that order"""
    from dps_ttc_amd.metrics import best_of_n_curve
    for name, v in (("psnr", psnr), ("ssim", ssim)):
        v = np.asarray(v, dtype=np.float32)
        np.save(os.path.join(out_path, f'{fname}_pathwise_{name}.npy'), v)
        np.save(os.path.join(out_path, f'{fname}_best_of_n_{name}.npy'), best_of_n_curve(distances, v))


class PathMetrics:
    """--path_metrics device: PSNR and SSIM of a particle group in one device call and one copy with the group's distances
    (`host` [3, B K]: rows psnr, ssim, distance of the last group, image-major: what its per-path log lines print) and, at
    the end, save_path_metrics per image"""

    def __init__(self, refs):
        self.refs, self.host, self.groups = refs, None, []

    def add(self, sample, sampler=None, dist_g=None):
        B = self.refs.shape[0]
        pm = pathwise_metrics(self.refs, sample, n_images=B)
        self.host = torch.stack([pm["psnr"], pm["ssim"], dist_g.reshape(-1).float()]).cpu().numpy()
        self.groups.append(self.host.reshape(3, B, -1))

    def save(self, out_path, fnames):
        rows = np.concatenate(self.groups, axis=2)        # [groups][3, B, K] -> [3, B, n_paths]: group-major, the path order
        for b, fname in enumerate(fnames):
            save_path_metrics(out_path, fname, rows[2, b], rows[0, b], rows[1, b])


def start_particles(args, sampler, g, shape, device, per_image=0):
    """x_start of particle group g.  --noise_draw device: the sampler is told the group's first path id (global over the
    ranks: the groups shard contiguously) and x_start is the tag-1 draw of those paths; else torch.randn"""
    if args.noise_draw != 'device':
        return torch.randn(shape, device=device).requires_grad_()
    from dps_ttc_amd import kernels
    sampler.path_base = args.path_start_idx + g * args.batch_size
    rng = kernels.Rng(sampler.noise_seed, 0, kernels.Rng.TAG_X_START, sampler.path_base, per_image)
    return kernels.randn(shape, rng, device).requires_grad_()


def image_batches(picks, m):
    """the picked reference images in pick order as batches of up to m images (the last one may be smaller)"""
    m = max(1, int(m))
    return [picks[i:i + m] for i in range(0, len(picks), m)]


def check_images_per_batch(args, sampler_name, world):
    """--images_per_batch > 1: reject what this mode does not support, before any GPU work (one-line message)"""
    m = args.images_per_batch
    if m < 1:
        raise SystemExit(f"--images_per_batch must be at least 1 (got {m})")
    if m == 1:
        return
    if world > 1:
        raise SystemExit("--images_per_batch > 1 runs on one rank only: sharding a multi-image batch over "
                         f"WORLD_SIZE={world} ranks is not supported")
    if sampler_name == 'ttc_ddim' and args.resample_draw != 'device':
        raise SystemExit("--images_per_batch > 1 is not supported with sampler ttc_ddim: its resampling would mix the "
                         "particles of different images (--resample_draw device draws per image)")
    if args.embedder is not None:
        raise SystemExit("--images_per_batch > 1 is not supported with --embedder: semantic guidance has one target "
                         "for all particles")


def check_resample_scheme(args, sampler_name=None):
    """--resample_scheme / --resample_ess / --ttc_resample_every: reject bad combinations before any GPU work (one-line
    message); sampler_name: also reject them for a sampler whose loop never resamples, instead of ignoring them.
    smc_ddpm takes the three flags too and always draws on the device: --resample_draw need not be given for it"""
    if (args.resample_scheme, args.resample_ess, args.ttc_resample_every) == ('multinomial', None, 10):
        return
    if args.ttc_resample_every < 1:
        raise SystemExit(f"--ttc_resample_every must be at least 1 (got {args.ttc_resample_every})")
    if args.resample_ess is not None and not 0.0 <= args.resample_ess <= 1.0:
        raise SystemExit(f"--resample_ess is a fraction of the particle count in [0, 1] (got {args.resample_ess})")
    for flag, value, default in (("--resample_scheme", args.resample_scheme, "multinomial"),
                                 ("--resample_ess", args.resample_ess, None)):
        if value != default and args.resample_draw != 'device' and sampler_name != 'smc_ddpm':
            raise SystemExit(f"{flag} {value} needs --resample_draw device: the schemes and the ESS trigger are options "
                             "of the library's per-image draw")
    if sampler_name is not None and sampler_name not in ('ttc_ddim', 'smc_ddpm'):
        for flag, value, default in (("--resample_scheme", args.resample_scheme, "multinomial"),
                                     ("--resample_ess", args.resample_ess, None),
                                     ("--ttc_resample_every", args.ttc_resample_every, 10)):
            if value != default:
                raise SystemExit(f"{flag} {value} is an option of sampler ttc_ddim, the loop that resamples (the diffusion "
                                 f"config names {sampler_name})")


def smc_flags(args):
    """the --smc_* flags that were given, as (flag, value) pairs"""
    return [(f"--smc_{k}", getattr(args, f"smc_{k}")) for k in ("twist_scale", "twist_power", "proposal_weight")
            if getattr(args, f"smc_{k}") is not None]


def check_smc(args, sampler_name, world=1):
    """--smc_*: options of sampler smc_ddpm; reject them for another sampler, and what that loop does not support, before any
    GPU work (one-line message)"""
    if not smc_flags(args) and sampler_name != 'smc_ddpm':
        return
    for flag, value in smc_flags(args):
        if sampler_name != 'smc_ddpm':
            raise SystemExit(f"{flag} {value} is an option of sampler smc_ddpm (the diffusion config names {sampler_name})")
        if value != value or value in (float("inf"), float("-inf")):
            raise SystemExit(f"{flag} must be finite (got {value})")
    if sampler_name == 'smc_ddpm':
        if world > 1:
            raise SystemExit(f"sampler smc_ddpm runs on one rank only: its weights and resampling are not exchanged between "
                             f"ranks (WORLD_SIZE={world})")
        if args.particle_groups > 1:
            raise SystemExit("sampler smc_ddpm does not run with --particle_groups > 1: the weights and the resampling are "
                             "over the whole particle set")


def check_dsg(args, method_name):
    """--dsg_guidance_rate: an option of conditioning method dsg; reject it for another method, and a value outside [0, 1],
    before any GPU work (one-line message)"""
    g = args.dsg_guidance_rate
    if g is None:
        return
    if method_name != 'dsg':
        raise SystemExit(f"--dsg_guidance_rate {g} is an option of conditioning method dsg (the task config names "
                         f"{method_name})")
    if not 0.0 <= g <= 1.0:
        raise SystemExit(f"--dsg_guidance_rate must be in [0, 1] (got {g})")


def pgdm_flags(args):
    return [(f"--pgdm_{k}", getattr(args, f"pgdm_{k}")) for k in ("iters", "weighting", "weight")
            if getattr(args, f"pgdm_{k}") is not None]


def check_pgdm(args, method_name, sampler_name=None):
    """--pgdm_*: options of conditioning method pgdm; reject them for another method, values outside their range, and what
    the pgdm step does not run under, before any GPU work (one-line message)"""
    for flag, value in pgdm_flags(args):
        if method_name != 'pgdm':
            raise SystemExit(f"{flag} {value} is an option of conditioning method pgdm (the task config names {method_name})")
    if method_name != 'pgdm':
        return
    if args.pgdm_iters is not None and not 0 <= args.pgdm_iters <= 64:
        raise SystemExit(f"--pgdm_iters must be in [0, 64] (got {args.pgdm_iters})")
    if args.pgdm_weight is not None and not math.isfinite(args.pgdm_weight):
        raise SystemExit(f"--pgdm_weight must be finite (got {args.pgdm_weight})")
    if sampler_name == 'smc_ddpm':
        raise SystemExit("conditioning method pgdm does not run under sampler smc_ddpm (its weights assume the fused ps "
                         "step's proposal)")
    if args.particle_groups > 1:
        raise SystemExit("conditioning method pgdm does not run with --particle_groups > 1 (groups exist under a fused plan "
                         "only, pgdm runs one chain)")


def check_solver(args, sampler_name, method_name, world=1, eta=None):
    """--solver_order / --guidance_gain: reject what the sampling loops would refuse, before any GPU work (one-line
    message).  eta: the diffusion config's (None: the sampler's default 0)"""
    order, gain = args.solver_order, args.guidance_gain
    if order is None and gain is None:
        return
    if order is not None and sampler_name not in ('ddim', 'ttc_ddim'):
        raise SystemExit(f"--solver_order {order} is an option of samplers ddim and ttc_ddim (the diffusion config names "
                         f"{sampler_name})")
    if order == 2:
        if method_name in ('cg', 'dsg', 'pgdm'):
            raise SystemExit(f"--solver_order 2 is not supported with conditioning method {method_name} (it has its own "
                             "update)")
        if float(eta or 0.0) not in (0.0, 1.0):
            raise SystemExit(f"--solver_order 2 needs eta 0 or 1 in the diffusion config (got {eta})")
        if sampler_name == 'ttc_ddim' and world > 1:
            raise SystemExit("--solver_order 2 with ttc_ddim on several ranks is not supported (the history does not "
                             "travel between ranks)")
    if gain == 'span' and method_name in ('cg', 'dsg', 'pgdm'):
        raise SystemExit(f"--guidance_gain span is not supported with conditioning method {method_name} (it has no scale "
                         "per step)")


def check_beam_width(args, sampler_name, world):
    """--beam_width: reject what the beam loop does not support, before any GPU work (one-line message)"""
    b = args.beam_width
    if b < 1:
        raise SystemExit(f"--beam_width must be at least 1 (got {b})")
    if b == 1:
        return
    if sampler_name != 'search_ddpm':
        raise SystemExit(f"--beam_width > 1 is an option of sampler search_ddpm (the diffusion config names {sampler_name})")
    if args.batch_size % b:
        raise SystemExit(f"--beam_width {b} does not divide --batch_size {args.batch_size}, the particles per image")
    if world > 1:
        raise SystemExit("--beam_width > 1 runs on one rank only: the multi-rank select exchanges one winner, not the "
                         f"best {b} (WORLD_SIZE={world})")


def repulsion_flags(args):
    """the --repulsion_* options given on the command line: [(flag, value)]"""
    given = [("--repulsion_scale", args.repulsion_scale if args.repulsion_scale != 0.0 else None),
             ("--repulsion_bandwidth", args.repulsion_bandwidth),
             ("--repulsion_stop", args.repulsion_stop if args.repulsion_stop != 0.0 else None)]
    return [(flag, v) for flag, v in given if v is not None]


def check_repulsion(args, sampler_name, world=1):
    """--repulsion_* and --path_diversity: reject what the loops refuse, before any GPU work (one-line message)"""
    import math
    if not repulsion_flags(args) and not args.path_diversity:
        return
    for flag, value in repulsion_flags(args):
        if not math.isfinite(value) or value < 0.0:
            raise SystemExit(f"{flag} must be finite and not negative (got {value})")
    if not 0.0 <= args.repulsion_stop <= 1.0:
        raise SystemExit(f"--repulsion_stop is a fraction of the trajectory in [0, 1] (got {args.repulsion_stop})")
    if args.batch_size > 512 and (args.repulsion_scale > 0.0 or args.path_diversity):
        raise SystemExit(f"--repulsion_scale / --path_diversity take at most 512 particles per image (--batch_size "
                         f"{args.batch_size})")
    if not args.repulsion_scale > 0.0:
        for flag, value in repulsion_flags(args):
            raise SystemExit(f"{flag} {value} needs --repulsion_scale > 0")
        return
    if sampler_name in ('search_ddpm', 'smc_ddpm'):
        raise SystemExit(f"--repulsion_scale is an option of samplers ddpm, ddim and ttc_ddim (the diffusion config names "
                         f"{sampler_name})")
    if args.particle_groups > 1:
        raise SystemExit("--repulsion_scale does not run with --particle_groups > 1: the step crosses the groups")
    if world > 1 and sampler_name == 'ttc_ddim':
        raise SystemExit("--repulsion_scale with sampler ttc_ddim runs on one rank only: with the multi-rank resampling an "
                         f"image's particles live on several ranks (WORLD_SIZE={world})")


class PathDiversity:
    """--path_diversity: per particle group the (mean, min) RMS per-element distance between the final samples of every
    image, one device call (kernels.pairwise_sqdist) and one copy; at the end {fname}_path_diversity.npy [groups, 2]"""

    def __init__(self, n_images):
        self.n_images, self.groups = n_images, []

    def add(self, sample, sampler=None, dist_g=None):
        from dps_ttc_amd import kernels
        _, info = kernels.pairwise_sqdist(sample.detach(), images=self.n_images, want_info=True)
        self.groups.append(torch.sqrt(info[:, 2:4] / sample[0].numel()).cpu().numpy())      # [B, 2]

    def save(self, out_path, fnames):
        for b, fname in enumerate(fnames):       # [groups][B, 2] -> image b's [groups, 2]
            np.save(os.path.join(out_path, f'{fname}_path_diversity.npy'), np.stack([v[b] for v in self.groups]))


def refuse_particle_set(flag, world, args=None, sampler_name=None, noun=None, max_k=None):
    """what the flags that analyse an image's particles refuse alike (one-line messages): more than one rank and, for a
    flag that needs the whole set in one call (noun: what it computes, max_k: the most paths it takes), sampler search_ddpm,
    more than one particle group per image and more than max_k paths"""
    if world > 1:
        raise SystemExit(f"{flag} runs on one rank only: the particles of an image are not gathered between "
                         f"ranks (WORLD_SIZE={world})")
    if noun is None:
        return
    if sampler_name == 'search_ddpm':
        raise SystemExit(f"{flag} needs a particle set: sampler search_ddpm keeps one state per image")
    if args.n_paths != args.batch_size:
        raise SystemExit(f"{flag} takes one particle group per image: the {noun} of two groups do not "
                         f"merge (n_paths {args.n_paths}, batch_size {args.batch_size})")
    if args.batch_size > max_k:
        raise SystemExit(f"{flag} takes at most {max_k} paths per image (--batch_size {args.batch_size})")


def check_posterior_summary(args, sampler_name, world=1):
    """--posterior_summary / --posterior_weights: reject what they do not support, before any GPU work (one-line message)"""
    if not args.posterior_summary:
        if args.posterior_weights != 'uniform':
            raise SystemExit(f"--posterior_weights {args.posterior_weights} needs --posterior_summary")
        return
    refuse_particle_set("--posterior_summary", world)
    if args.batch_size > 4096:
        raise SystemExit(f"--posterior_summary takes at most 4096 paths per particle group (--batch_size {args.batch_size})")
    if args.posterior_weights == 'smc':
        if sampler_name != 'smc_ddpm':
            raise SystemExit("--posterior_weights smc reads the weights of sampler smc_ddpm (the diffusion config names "
                             f"{sampler_name})")
        if args.n_paths // args.batch_size != 1:
            raise SystemExit("--posterior_weights smc takes one particle group: the weights of two groups share no reference "
                             f"level (n_paths / batch_size = {args.n_paths // args.batch_size})")


class PosteriorSummary:
    """--posterior_summary: the particle groups of the same images merged one by one (metrics.posterior_summary with the
    previous group as the prior) and, at the end, the four files per image"""

    def __init__(self, refs, weights='uniform'):
        self.refs, self.weights, self.last, self.curves = refs, weights, None, []

    def add(self, sample, sampler=None, dist_g=None):
        from dps_ttc_amd.metrics import posterior_summary
        e = sampler.last_neg_log_weights if self.weights == 'smc' else None
        self.last = posterior_summary(self.refs, sample, n_images=self.refs.shape[0], neg_log_weights=e, prior=self.last)
        self.curves.append(self.last["mean_of_n_psnr"])

    def save(self, out_path, fnames):
        s = self.last
        os.makedirs(os.path.join(out_path, 'posterior_mean'), exist_ok=True)
        curve = torch.cat(self.curves, dim=1).cpu().numpy()              # [M, n_paths]: group-major, the path order
        rec = torch.stack([s["mean_psnr"], s["mean_ssim"], s["ess"], s["std"].flatten(1).mean(dim=1)], dim=1).cpu().numpy()
        std = s["std"].cpu().numpy()
        for b, fname in enumerate(fnames):
            imsave(os.path.join(out_path, 'posterior_mean', fname + '.png'), clear_color(s["mean"][b:b + 1]))
            np.save(os.path.join(out_path, f'{fname}_posterior_std.npy'), std[b])
            np.save(os.path.join(out_path, f'{fname}_mean_of_n_psnr.npy'), curve[b])
            np.save(os.path.join(out_path, f'{fname}_posterior_summary.npy'), rec[b])


def quantile_percentages(text):
    """--posterior_quantiles: 'P1,P2,...' -> the percentages as floats (ValueError for anything that is not a number)"""
    return [float(v) for v in str(text).split(',') if v.strip() != '']


def check_posterior_quantiles(args, sampler_name, world=1):
    """--posterior_quantiles: reject what it does not support, before any GPU work (one-line message)"""
    if args.posterior_quantiles is None:
        return
    try:
        pct = quantile_percentages(args.posterior_quantiles)
    except ValueError:
        raise SystemExit(f"--posterior_quantiles takes percentages separated by commas (got {args.posterior_quantiles!r})")
    if not 1 <= len(pct) <= 8:
        raise SystemExit(f"--posterior_quantiles takes between 1 and 8 percentages (got {len(pct)})")
    if any(not (0.0 <= v <= 100.0) for v in pct):
        raise SystemExit(f"--posterior_quantiles takes percentages in [0, 100] (got {args.posterior_quantiles})")
    refuse_particle_set("--posterior_quantiles", world, args, sampler_name, "order statistics", 512)


class PosteriorQuantiles:
    """--posterior_quantiles: the order statistics of the one particle group (metrics.posterior_quantiles) and the files
    per image"""

    def __init__(self, refs, text):
        self.refs, self.pct, self.last = refs, quantile_percentages(text), None

    def add(self, sample, sampler=None, dist_g=None):
        from dps_ttc_amd.metrics import posterior_quantiles
        self.last = posterior_quantiles(self.refs, sample, n_images=self.refs.shape[0], probs=[v / 100.0 for v in self.pct])

    def save(self, out_path, fnames):
        s = self.last
        quant, hist, info = s["quantiles"].cpu().numpy(), s["hist"].cpu().numpy(), s["info"].cpu().numpy()
        if 50.0 in self.pct:
            os.makedirs(os.path.join(out_path, 'posterior_median'), exist_ok=True)
        for b, fname in enumerate(fnames):
            np.save(os.path.join(out_path, f'{fname}_posterior_quantiles.npy'), quant[b])
            np.save(os.path.join(out_path, f'{fname}_rank_hist.npy'), hist[b])
            np.save(os.path.join(out_path, f'{fname}_quantile_summary.npy'), info[b])
            if 50.0 in self.pct:
                imsave(os.path.join(out_path, 'posterior_median', fname + '.png'),
                       clear_color(s["quantiles"][b:b + 1, self.pct.index(50.0)]))


def check_posterior_pca(args, sampler_name, world=1):
    """--posterior_pca: reject what it does not support, before any GPU work (one-line message)"""
    if args.posterior_pca is None:
        return
    if not 1 <= args.posterior_pca <= 8:
        raise SystemExit(f"--posterior_pca takes between 1 and 8 components (got {args.posterior_pca})")
    refuse_particle_set("--posterior_pca", world, args, sampler_name, "components", 128)


class PosteriorPca:
    """--posterior_pca: the principal components of the one particle group (metrics.posterior_pca), the panels around the
    group's mean (kernels.ensemble_stats) and the files per image"""

    def __init__(self, n_images, components):
        self.n_images, self.q, self.last, self.panels = n_images, components, None, None

    def add(self, sample, sampler=None, dist_g=None):
        from dps_ttc_amd import kernels
        from dps_ttc_amd.metrics import pc_panels, posterior_pca
        self.last = posterior_pca(sample, n_images=self.n_images, components=self.q)
        mean = kernels.ensemble_stats(sample.detach(), images=self.n_images)["mean"]
        self.panels = pc_panels(mean, self.last["dirs"], self.last["var"])

    def save(self, out_path, fnames):
        s = self.last
        dirs, coords = s["dirs"].cpu().numpy(), s["coords"].cpu().numpy()
        rec = torch.stack([s["var"], s["explained"]], dim=2).cpu().numpy()
        os.makedirs(os.path.join(out_path, 'posterior_pca'), exist_ok=True)
        for b, fname in enumerate(fnames):
            np.save(os.path.join(out_path, f'{fname}_posterior_pcs.npy'), dirs[b])
            np.save(os.path.join(out_path, f'{fname}_pca_summary.npy'), rec[b])
            np.save(os.path.join(out_path, f'{fname}_pca_coords.npy'), coords[b])
            for j in range(self.q):
                for side, panel in zip(('minus', 'plus'), self.panels):
                    imsave(os.path.join(out_path, 'posterior_pca', f'{fname}_pc{j}_{side}.png'),
                           clear_color(panel[b:b + 1, j]))


def preflight(args, world):
    """every refusal that needs no GPU, in one fixed order: a command line that is wrong in two ways gets the message of
    the first check it fails; each check returns at once when its flags are not given.  -> (diffusion config, task
    config), each file read once, None where its path is not given: the checks that need no sampler or method name
    still run"""
    diffusion_config = load_yaml(args.diffusion_config) if args.diffusion_config else None
    task_config = load_yaml(args.task_config) if args.task_config else None
    sampler_name = diffusion_config['sampler'] if args.diffusion_config else None
    method_name = task_config['conditioning']['method'] if args.task_config else None
    check_resample_scheme(args, sampler_name)
    check_smc(args, sampler_name, world)
    check_dsg(args, method_name)
    check_pgdm(args, method_name, sampler_name)
    check_solver(args, sampler_name, method_name, world, diffusion_config.get('eta') if args.diffusion_config else None)
    check_beam_width(args, sampler_name, world)
    check_repulsion(args, sampler_name, world)
    check_images_per_batch(args, sampler_name, world)
    check_posterior_summary(args, sampler_name, world)
    check_posterior_quantiles(args, sampler_name, world)
    check_posterior_pca(args, sampler_name, world)
    return diffusion_config, task_config


def main(argv=None):
    args = parse_args(argv)
    logger = get_logger()
    rank, world = int(os.environ.get("RANK", 0)), int(os.environ.get("WORLD_SIZE", 1))
    diffusion_config, task_config = preflight(args, world)
    if world > 1:
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", 0)) % max(torch.cuda.device_count(), 1)
        torch.cuda.set_device(local)
        backend = os.environ.get("DPSX_DIST_BACKEND", "nccl")      # "nccl" is RCCL; "gloo" only to rehearse on one GPU
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
        args.gpu = local
    if not torch.cuda.is_available():
        raise SystemExit("dps_ttc_amd runs the DPS hot path on an MI355X only (no CPU fallback by design)")
    device = torch.device(f"cuda:{args.gpu}")
    torch.cuda.set_device(device)
    logger.info(f"Device set to {device}.")

    model_config = load_yaml(args.model_config)
    if args.timestep_respacing is not None:
        diffusion_config['timestep_respacing'] = args.timestep_respacing
    if args.solver_order is not None:            # check_solver: the sampler is a ddim one
        diffusion_config['solver_order'] = args.solver_order
    if args.seed is not None:
        torch.manual_seed(args.seed + rank)

    model = create_model(**model_config).to(device).eval()

    measure_config = task_config['measurement']
    np.random.seed(args.kernel_idx)                     # selects the motion kernel / inpainting mask
    operator = get_operator(device=device, **measure_config['operator'])
    noiser = get_noise(**measure_config['noise'])
    op_name = measure_config['operator']['name']
    logger.info(f"Operation: {op_name} / Noise: {measure_config['noise']['name']}")

    cond_config = task_config['conditioning']
    cond_params = dict(cond_config['params'])
    if args.dsg_guidance_rate is not None:       # check_dsg: the method is dsg
        cond_params['guidance_rate'] = args.dsg_guidance_rate
    for flag, value in pgdm_flags(args):         # check_pgdm: the method is pgdm
        cond_params[flag[len("--pgdm_"):]] = value
    embedder = None
    if args.embedder is not None:
        import importlib
        mod_name, _, fn_name = args.embedder.partition(':')
        embedder = getattr(importlib.import_module(mod_name), fn_name)(device)
        cond_params['embedder'] = embedder
    cond_method = get_conditioning_method(cond_config['method'], operator, noiser, **cond_params)
    measurement_cond_fn = cond_method.conditioning
    logger.info(f"Conditioning method : {cond_config['method']}")
    logger.info(f"Sampling: {diffusion_config['sampler']} / Steps: {diffusion_config['steps']}")

    sampler = create_sampler(**diffusion_config)
    sampler.particle_groups = max(1, args.particle_groups)
    sampler.resample_draw = args.resample_draw
    sampler.resample_scheme, sampler.resample_ess = args.resample_scheme, args.resample_ess
    sampler.resample_every = args.ttc_resample_every
    sampler.noise_draw = args.noise_draw
    sampler.beam_width = args.beam_width
    if args.guidance_gain is not None:
        sampler.guidance_gain = args.guidance_gain
    sampler.repulsion_scale, sampler.repulsion_stop = args.repulsion_scale, args.repulsion_stop
    sampler.repulsion_bandwidth = args.repulsion_bandwidth
    for flag, value in smc_flags(args):          # check_smc: the sampler is smc_ddpm
        setattr(sampler, flag[len("--smc_"):], value)
    sampler.noise_seed = args.seed or 0          # the same on every rank: the path id tells the ranks' particles apart
    groups = args.n_paths // args.batch_size
    if world > 1 and diffusion_config['sampler'] in ('search_ddpm', 'ttc_ddim'):
        # these loops exchange particles at every select / resample point: every rank runs the same number of groups
        if groups % world != 0:
            raise SystemExit(f"sampler {diffusion_config['sampler']} on {world} ranks needs n_paths / batch_size "
                             f"(= {groups} particle groups) to be a multiple of the number of ranks")
        if diffusion_config['sampler'] == 'search_ddpm':
            sampler.global_select = dd.GlobalSelect()
        else:
            sampler.global_resample = True
            # same stream on all ranks; a DEVICE generator: the draw runs on the GPU (as the reference's does), no host read
            sampler.resample_generator = torch.Generator(device=device).manual_seed(args.seed or 0)
    sample_fn = partial(sampler.p_sample_loop, model=model, measurement_cond_fn=measurement_cond_fn,
                        operator=operator, resample_every_steps=args.resample_every_steps,
                        potential_type=args.potential_type, rs_temp=args.rs_temp, anneal_scale=args.anneal_scale,
                        anneal_loc=args.anneal_loc, anneal_amp=args.anneal_amp)

    sigma = measure_config['noise'].get('sigma', 0)
    if cond_config['method'] == 'ps_anneal':
        dir_name = f"{op_name}_noise_sigma_{sigma}_dps_anneal_amp_{args.anneal_amp}"
    elif cond_config['method'] == 'cg':
        dir_name = (f"{op_name}_noise_sigma_{sigma}_cg_rho_scale_{cond_method.rho_scale}_iters_{cond_method.iters}")
    elif cond_config['method'] == 'dsg':
        dir_name = f"{op_name}_noise_sigma_{sigma}_dsg_guidance_rate_{cond_method.guidance_rate}"
    elif cond_config['method'] == 'pgdm':
        dir_name = (f"{op_name}_noise_sigma_{sigma}_pgdm_{cond_method.weighting}_iters_{cond_method.iters}_weight_"
                    f"{cond_method.weight}")
    else:
        dir_name = f"{op_name}_noise_sigma_{sigma}_dps_scale_{cond_config['params']['scale']}"
    out_path = os.path.join(args.save_dir, dir_name)
    for img_dir in ['input', 'recon_paths', 'label', 'best_of_n']:
        os.makedirs(os.path.join(out_path, img_dir), exist_ok=True)

    dataset = get_dataset(**task_config['data'], transforms=to_minus1_1)
    picks = [int(i) for i in args.ref_image_idxs.split(',')]
    mask_gen = mask_generator(**measure_config['mask_opt']) if op_name == 'inpainting' else None
    if op_name == 'motion_blur' and rank == 0:
        imsave(os.path.join(out_path, f'kernel_{str(args.kernel_idx).zfill(5)}.png'), clear_color(operator.get_kernel()))
    run = Run(args, logger, device, rank, world, dataset, operator, noiser, op_name, cond_method, embedder, sample_fn,
              mask_gen, sampler, diffusion_config['sampler'], groups, out_path)
    for n, batch in enumerate(image_batches(picks, args.images_per_batch)):
        run_images(run, batch, n)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


class Run(NamedTuple):
    """what main() built once and every batch of images runs with"""
    args: argparse.Namespace
    logger: object
    device: torch.device
    rank: int
    world: int
    dataset: object
    operator: object
    noiser: object
    op_name: str
    cond_method: object
    embedder: object
    sample_fn: object
    mask_gen: object
    sampler: object
    sampler_name: str
    groups: int
    out_path: str


def select_winners(run, distances, finals, refs):
    """best-of-N per image: argmin of the final measurement distance over every path of the image.  distances / finals:
    this rank's groups' [B K] scores and [B K, C, H, W] particles (image-major) -> per image (winner [1, C, H, W], path
    index, the image's distances in path order on the host)"""
    B, K = refs.shape[0], run.args.batch_size
    if run.args.images_per_batch > 1:
        # the [groups, B, K] distances in image-major path order, one segmented argmin, one gather
        from dps_ttc_amd import kernels
        n_paths = run.groups * K
        d_img = torch.stack(distances).reshape(run.groups, B, K).transpose(0, 1).reshape(B * n_paths).contiguous()
        best = kernels.argmin_seg(d_img, B)                                   # [B]: b * n_paths + path
        path = best - torch.arange(B, device=best.device) * n_paths
        src = (path // K) * (B * K) + torch.arange(B, device=best.device) * K + path % K    # index into the groups' concat
        winners = kernels.gather(torch.cat(finals).detach(), src, validate=False)
        d_host, path_host = d_img.reshape(B, n_paths).cpu().numpy(), path.cpu().numpy()
        return [(winners[b:b + 1], int(path_host[b]), d_host[b]) for b in range(B)]
    # over every particle of every rank.  The groups shard contiguously: the rank-major order of the gathered scores is the
    # path order.  Every rank enters (a rank without groups contributes an empty shard and still receives the winner).
    counts = [c * K for c in dd.shard_counts(run.groups, run.world)]
    scores_local = torch.cat(distances) if distances else torch.empty(0, device=run.device)
    particles_local = torch.cat(finals) if finals else torch.empty((0,) + refs.shape[1:], device=run.device)
    winner, best, all_d = dd.global_best_of_n(scores_local, particles_local, counts)
    return [(winner, best, all_d.cpu().numpy())]


def run_images(run, batch, n=0):
    """The B = len(batch) reference images of `batch` (the n-th batch of the run) as one multi-image batch per particle
    group -- B x batch_size particles, image-major (particles [b K, (b + 1) K) belong to image b), y [B, ...] -- their
    analyses, the per-image best-of-N and the saves.  The default mode is batches of one image."""
    args, logger, device, operator, op_name, out_path = run.args, run.logger, run.device, run.operator, run.op_name, run.out_path
    B, K = len(batch), args.batch_size
    fnames = [str(i).zfill(5) for i in batch]
    # what differs between the modes: --images_per_batch > 1 tells the sampler and the x_start draw how many images the
    # batch holds (n_images = 1 would take search_ddpm through its segmented entry points) and names the image on every log
    # line; only the default mode runs on several ranks (the groups sharded over them, rank 0's measurement, rank 0 writes),
    # with semantic guidance, and selects over all ranks (select_winners)
    multi = args.images_per_batch > 1
    sample_kw, start_kw = ({'n_images': B}, {'per_image': K}) if multi else ({}, {})
    tags = [(f"Image {f} ", f"Image {f}: ") for f in fnames] if multi else [("", "")]
    if multi:
        logger.info(f"Inference for images {', '.join(fnames)} ({B} x {K} particles per call)")
    else:
        logger.info(f"Inference for image {args.start_idx + n}")
    my_groups = range(*dd.shard_range(run.groups, run.rank, run.world))

    refs = torch.stack([run.dataset[min(i, len(run.dataset) - 1)] for i in batch]).to(device)
    C, H, W = refs.shape[1:]
    if run.embedder is not None and hasattr(run.cond_method, 'guid_image_emb'):      # B = 1 (check_images_per_batch)
        guid = refs
        if args.guid_image is not None:
            from PIL import Image
            guid = to_minus1_1(Image.open(args.guid_image).convert('RGB')).unsqueeze(0).to(device)
        with torch.no_grad():
            run.cond_method.guid_image_emb = run.embedder(guid).unsqueeze(0)        # [1, n_guid = 1, D]
    masks, ys = [], []
    for b in range(B):             # per image in pick order: its mask, then its noisy measurement
        fkw = {}
        if op_name == 'inpainting':
            masks.append(run.mask_gen(refs[b:b + 1])[:, 0, :, :].unsqueeze(dim=0).contiguous())
            fkw = {'mask': masks[-1]}
        if run.world > 1:       # every rank must see the same measurement: rank 0 draws the noise
            gen_state = torch.random.get_rng_state()
        with torch.no_grad():
            ys.append(run.noiser(operator.forward(refs[b:b + 1], **fkw)).contiguous())
        if run.world > 1:
            import torch.distributed as dist
            dist.broadcast(ys[-1], src=0)
            torch.random.set_rng_state(gen_state)
    y = torch.cat(ys).contiguous()
    fkw, sample_fn = {}, run.sample_fn
    if op_name == 'inpainting':
        mask = torch.cat(masks).contiguous()                     # [B, 1, H, W]: particle p uses mask p // K
        fkw = {'mask': mask}
        sample_fn = partial(sample_fn, measurement_cond_fn=partial(run.cond_method.conditioning, mask=mask, l1=args.l1),
                            mask=mask)
    for b, fname in enumerate(fnames):
        os.makedirs(os.path.join(out_path, 'recon_paths', fname), exist_ok=True)
        os.makedirs(os.path.join(out_path, 'recon_paths_y', fname), exist_ok=True)
        if run.rank == 0:
            imsave(os.path.join(out_path, 'input', fname + '.png'), clear_color(y[b:b + 1]))
            imsave(os.path.join(out_path, 'label', fname + '.png'), clear_color(refs[b:b + 1]))

    # one rank for every analysis (parse_args, the checks); the order is the order of their device calls per group
    metrics = PathMetrics(refs) if args.path_metrics == 'device' else None
    outputs = [o for o in (PathDiversity(B) if args.path_diversity else None,
                           PosteriorSummary(refs, args.posterior_weights) if args.posterior_summary else None,
                           PosteriorQuantiles(refs, args.posterior_quantiles) if args.posterior_quantiles is not None else None,
                           PosteriorPca(B, args.posterior_pca) if args.posterior_pca is not None else None,
                           metrics) if o is not None]
    distances, finals = [], []
    for g in my_groups:
        x_start = start_particles(args, run.sampler, g, (B * K, C, H, W), device, **start_kw)
        sample = sample_fn(x_start=x_start, measurement=y, record=False, save_root=out_path, **sample_kw)
        if isinstance(sample, tuple):       # ttc_ddim hands back (particles, distances) (reference :707)
            sample = sample[0]
        with torch.no_grad():
            y_space = operator.forward(sample, **fkw)                      # for the PNGs
            handle = operator.hip_handle_for(fkw['mask']) if op_name == 'inpainting' else operator.hip_handle(sample)
            dist_g = handle.score(sample, y)                               # ||y_{p // K} - A(x_p)||_2 per particle (HIP)
        distances.append(dist_g)
        finals.append(sample)
        for o in outputs:
            o.add(sample, run.sampler, dist_g)
        for b, fname in enumerate(fnames):
            for i in range(K):
                p, path_idx = b * K + i, args.path_start_idx + g * K + i
                if metrics is not None:
                    psnr, ssim, d = metrics.host[:, p]
                    logger.info(f"{tags[b][0]}Path#{path_idx + 1} | Method:{run.sampler_name} / PSNR: {psnr:.4f} / "
                                f"SSIM: {ssim:.4f} / distance: {d:.4f}")
                else:
                    psnr = compute_psnr(refs[b:b + 1], sample[p].unsqueeze(0))
                    logger.info(f"{tags[b][0]}Path#{path_idx + 1} | Method:{run.sampler_name} / PSNR: {float(psnr):.4f} / "
                                f"distance: {float(dist_g[p]):.4f}")
                imsave(os.path.join(out_path, 'recon_paths', fname, f'path#{path_idx + 1}.png'),
                       clear_color(sample[p].unsqueeze(0)))
                imsave(os.path.join(out_path, 'recon_paths_y', fname, f'path#{path_idx + 1}_y_space.png'),
                       clear_color(y_space[p].unsqueeze(0)))
    picked = select_winners(run, distances, finals, refs)
    if run.rank != 0:
        return
    for fname, ref, tag, (winner, k, d) in zip(fnames, refs.split(1), tags, picked):
        logger.info(f"{tag[1]}best-of-{d.size} = path#{args.path_start_idx + k + 1} | PSNR: "
                    f"{float(compute_psnr(ref, winner)):.4f} | distance: {float(d[k]):.4f}")
        imsave(os.path.join(out_path, 'best_of_n', fname + '.png'), clear_color(winner))
        np.save(os.path.join(out_path, f'{fname}_pathwise_distances.npy'), d)
    for o in outputs:
        o.save(out_path, fnames)


if __name__ == '__main__':
    main()

