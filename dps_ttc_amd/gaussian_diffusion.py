"""Samplers and the DPS / test-time-compute loops -- the reference's sampler API
(guided_diffusion/gaussian_diffusion.py) driving the HIP hot path.

    create_sampler(sampler, steps, noise_schedule, model_mean_type, model_var_type, dynamic_threshold,
                   clip_denoised, rescale_timesteps, timestep_respacing="") -> s        (reference :34-56)
    s.p_sample_loop(model=, x_start=, measurement=, measurement_cond_fn=, record=, save_root=, **kw)
    s.p_sample(model, x, t) -> {'sample', 'pred_xstart'};  s.q_sample(x0, t);  s.num_timesteps;  s.betas

Per step the host does: one UNet forward (PyTorch-ROCm), three fused HIP launches
(kernels.step_fwd / step_bwd / step_update), one UNet VJP (torch.autograd.grad with the
HIP-produced cotangent).  No table upload, no `.item()`, no host sync inside the loop.

Deliberate differences from the reference snapshot:
  * the base loop applies the *intended* DPS update for every conditioning method: methods that
    return the updated x_t ('ps', 'ps_anneal', ...) are taken at their word, methods that return
    the gradient ('ps_semantic') have it subtracted -- the reference loop does the latter for
    both and so zeroes the image under 'ps';
  * called with the test-time-compute driver's keyword set (operator=...), p_sample_loop returns
    the bare [N,C,H,W] tensor that driver expects (sample_condition_batched_ttc.py:181-183);
    the per-particle distances are kept in `sampler.last_measurement_distance`.
"""
import functools
import math
import os
from operator import index as _index
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import kernels
from .condition_methods import (ConditioningMethod, ConjugateGradientConsistency, PseudoInverseGuidance,
                                SphericalGaussianGuidance)
from .diffstategrad_utils import apply_diffstategrad, compute_svd_and_adaptive_rank
from .posterior_mean_variance import get_mean_processor, get_var_processor

__SAMPLER__ = {}                  # the reference's samplers, under the reference's names
__EXTENSION_SAMPLER__ = {}        # samplers the reference does not have ('smc_ddpm'): same lookup, their own table


def register_sampler(name: str, extension: bool = False):
    """extension=True: a sampler that is not in the reference; it is found by get_sampler like the others and kept out of
    the table that mirrors the reference's"""
    def wrapper(cls):
        if __SAMPLER__.get(name, None) or __EXTENSION_SAMPLER__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        (__EXTENSION_SAMPLER__ if extension else __SAMPLER__)[name] = cls
        return cls
    return wrapper


def get_sampler(name: str):
    cls = __SAMPLER__.get(name, None) or __EXTENSION_SAMPLER__.get(name, None)
    if cls is None:
        raise NameError(f"Name {name} is not defined!")
    return cls


def create_sampler(sampler, steps, noise_schedule, model_mean_type, model_var_type, dynamic_threshold,
                   clip_denoised, rescale_timesteps, timestep_respacing="", eta=None, solver_order=None):
    """eta (not in the reference, whose DDIM loops never pass it): the DDIM samplers' `eta` attribute -- sigma's scale,
    0 the deterministic sampler, 1 the DDPM-like one the `dsg` method wants; a sampler without that attribute refuses it.
    solver_order (not in the reference): the DDIM samplers' `solver_order` attribute, 1 (the DDIM rule) or 2 (the
    DPM-Solver++(2M) multistep update, eta 0 or 1 only); any other sampler refuses it.
    timestep_respacing "logsnr{n}" (not in the reference): at most n timesteps uniform in log-SNR (logsnr_timesteps);
    every other spec is space_timesteps'."""
    cls = get_sampler(name=sampler)
    betas = get_named_beta_schedule(noise_schedule, steps)
    if not timestep_respacing:
        timestep_respacing = [steps]
    if isinstance(timestep_respacing, str) and timestep_respacing.startswith("logsnr"):
        use_timesteps = logsnr_timesteps(betas, int(timestep_respacing[len("logsnr"):]))
    else:
        use_timesteps = space_timesteps(steps, timestep_respacing)
    smp = cls(use_timesteps=use_timesteps, betas=betas,
              model_mean_type=model_mean_type, model_var_type=model_var_type,
              dynamic_threshold=dynamic_threshold, clip_denoised=clip_denoised,
              rescale_timesteps=rescale_timesteps)
    if eta is not None:
        if not isinstance(smp, DDIM):
            raise ValueError(f"eta is an option of the ddim samplers (got sampler {sampler!r})")
        if not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"eta must be in [0, 1] (got {eta!r})")
        smp.eta = float(eta)
    if solver_order is not None:
        if not isinstance(smp, DDIM):
            raise ValueError(f"solver_order is an option of the ddim samplers (got sampler {sampler!r})")
        smp.solver_order = solver_order
        smp._check_solver_order()
    return smp


# ------------------------------------------------------------------ schedules
def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps,
                                   lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    n = num_diffusion_timesteps
    return np.array([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)])


def space_timesteps(num_timesteps, section_counts):
    """Subset of the base timesteps kept by a respacing spec ("", "250", "10,15,20", "ddim50")."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            want = int(section_counts[len("ddim"):])
            for stride in range(1, num_timesteps):
                if len(range(0, num_timesteps, stride)) == want:
                    return set(range(0, num_timesteps, stride))
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    elif isinstance(section_counts, int):
        section_counts = [section_counts]
    per, extra = divmod(num_timesteps, len(section_counts))
    start, kept = 0, []
    for i, count in enumerate(section_counts):
        size = per + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        pos = 0.0
        for _ in range(count):
            kept.append(start + round(pos))
            pos += stride
        start += size
    return set(kept)


def logsnr_timesteps(betas, n):
    """The base timesteps kept by "logsnr{n}": with lambda_t = 0.5 ln(abar_t / (1 - abar_t)) over the base schedule, n
    values uniform from lambda_0 to lambda_{T-1} inclusive, each replaced by the base index with the nearest lambda (a
    tie: the lower index), plus indices 0 and T - 1, duplicates dropped -- so AT MOST n timesteps (where the base
    schedule is coarse in lambda, neighbouring values share an index).  n < 2 raises ValueError."""
    n = int(n)
    if n < 2:
        raise ValueError(f"logsnr{n}: a log-SNR spacing needs at least 2 timesteps")
    abar = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64))
    lam = 0.5 * np.log(abar / (1.0 - abar))
    kept = {0, len(lam) - 1}
    for v in np.linspace(lam[0], lam[-1], n):
        kept.add(int(np.argmin(np.abs(lam - v))))          # argmin: the first of equal minima
    return kept


# ------------------------------------------------------------------ base class
class _Trajectory(NamedTuple):
    """what GaussianDiffusion._trajectory settles for a guided loop before its first step"""
    img: torch.Tensor                   # x_start, detached
    n: int                              # its particles
    method: object                      # the conditioning function's ConditioningMethod, or None
    plan: Optional[tuple]               # _fusion_plan's (method, kw, handle)
    cg: Optional[tuple]                 # _cg_plan's (method, kw): the `cg` method's, or `pgdm`'s on the same route
    images: Optional[int]               # the images of the batch (the base loop: None for one)
    y: Optional[torch.Tensor]           # the measurement, contiguous fp32; None on the per-op route


class GaussianDiffusion:
    def __init__(self, betas, model_mean_type, model_var_type, dynamic_threshold, clip_denoised,
                 rescale_timesteps):
        betas = np.array(betas, dtype=np.float64)           # float64 tables, fp32 at the point of use
        self.betas = betas
        assert betas.ndim == 1, "betas must be 1-D"
        assert (0 < betas).all() and (betas <= 1).all(), "betas must be in (0..1]"
        self.num_timesteps = int(betas.shape[0])
        self.rescale_timesteps = rescale_timesteps

        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1],
                                                               self.posterior_variance[1:]))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)

        self.model_mean_type, self.model_var_type = model_mean_type, model_var_type
        self.dynamic_threshold, self.clip_denoised = dynamic_threshold, clip_denoised
        self.mean_processor = get_mean_processor(model_mean_type, betas=betas, dynamic_threshold=dynamic_threshold,
                                                 clip_denoised=clip_denoised)
        self.var_processor = get_var_processor(model_var_type, betas=betas)
        # the configuration every shipped YAML uses runs S1 as one HIP kernel
        self.hip_posterior = (model_mean_type == 'epsilon' and model_var_type == 'learned_range'
                              and clip_denoised and not dynamic_threshold)
        log_betas = np.log(betas)
        self.step_coefs = [kernels.make_coefs(self.sqrt_recip_alphas_cumprod[t], self.sqrt_recipm1_alphas_cumprod[t],
                                              self.posterior_mean_coef1[t], self.posterior_mean_coef2[t],
                                              self.posterior_log_variance_clipped[t], log_betas[t], t != 0)
                           for t in range(self.num_timesteps)]
        #: draw noise on the host generator in the reference's order (parity tests); default: on the device
        self.rng_parity = False
        #: strides of the reference run's measurement tensor (only read when rng_parity is set)
        self.parity_measurement_stride = None
        #: the resampling draw of ttc_ddim / resample_update: "multinomial" (torch.multinomial over all N weights, the
        #: reference's draw) or "device" (kernels.resample: a pure function of the distances and one torch.rand per slot,
        #: computed per image on the device and fused with the particle gather -- the draw multi-image batches need)
        self.resample_draw = "multinomial"
        #: the device draw's scheme ("multinomial", "stratified", "systematic") and ESS trigger (tau in [0, 1]: an image
        #: resamples only while its effective sample size is below tau K; None = 1.0: whenever its weights differ) --
        #: include/dpsx.h "resampling schemes and the ESS trigger".  Anything but the defaults needs resample_draw = "device".
        self.resample_scheme = "multinomial"
        self.resample_ess = None
        #: after a resampling step with a non-default scheme / ESS: [images] uint8 (1: the image resampled) and its ESS
        self.last_resample_flags = None
        self.last_resample_ess = None
        #: the step noise: "torch" (torch.randn, one stream over the whole batch) or "device" (kernels.Rng: a counter-based
        #: draw keyed on (noise_seed, loop index, path id, element), drawn inside the fused launches where the operator has
        #: that form -- a path's noise then does not depend on the batch it runs in, the particle groups, the images per
        #: batch or the ranks).  Batch row p is path path_base + p (path_base + p % K in a multi-image batch of K per image).
        self.noise_draw = "torch"
        self.noise_seed = 0
        self.path_base = 0
        self.progress = False
        self.last_measurement_distance = None
        self.last_semantic_distance = None
        self._ts_cache = {}
        self._bufs = None
        self._step_semantic = None
        #: > 1: the fused base loop runs its N particles as this many independent sub-batches, each a whole chain (model
        #: call, three HIP launches, model VJP) on its own HIP stream with its own operator handle (kernels.ParticleGroups):
        #: the tile kernels' load / compute / store phases add up inside one chain, side by side they fill each other's gaps.
        #: Per-particle results do not depend on it (the noise is still drawn for the whole batch, in the same order).
        #: Groups exist only under a fused plan: the `cg` method has none and runs one chain whatever this says.
        self.particle_groups = 1
        self._pgroups = None
        #: a kernels.MetricTrace: the fused base loop writes mse / psnr / ssim of x0_hat against the trace's label and the
        #: step's distance into it every `every` steps (evaluation only; None: the loop launches what it always did)
        self.metric_trace = None
        #: particle repulsion (include/dpsx.h "particle repulsion"; Corso et al. 2023): > 0, after every step with idx > 0
        #: and idx / num_timesteps >= repulsion_stop the particles of an image are pushed apart by kernels.repulse with
        #: strength repulsion_scale * betas[idx] and bandwidth repulsion_bandwidth (a mean squared per-element difference;
        #: None: the mean-distance heuristic).  An option of the base loop (ddpm / ddim, every route) and of ttc_ddim, where
        #: the push comes before the resampling block.  0: the loops launch what they always did and allocate nothing.
        self.repulsion_scale = 0.0
        self.repulsion_bandwidth = None
        self.repulsion_stop = 0.0
        self._repulse_out = None
        #: "unit" (the reference: every kept step shifts by scale * gradient) or "span": the fused step's scale is
        #: multiplied by the base steps the kept step covers (timestep_map[i] - timestep_map[i - 1]; timestep_map[0] + 1
        #: at i = 0), so a respaced loop guides as much in total as the full schedule with the same scale.  A heuristic:
        #: the quality it gives is not pinned by any test.  Fused plans only; dsg has no scale and refuses it.
        self.guidance_gain = "unit"

    #: the order of the update (DDIM.solver_order); every other sampler steps at first order
    solver_order = 1

    def _step_span(self, idx):
        """the base timesteps the kept step at loop index idx covers"""
        tm = getattr(self, "timestep_map", None)
        if tm is None:
            return 1
        return int(tm[idx] - tm[idx - 1]) if idx > 0 else int(tm[0]) + 1

    def _check_solver(self, measurement_cond_fn, x_start, project, plan=False):
        """solver_order = 2 and guidance_gain = "span" run only where every step of the loop is the fused step with K3's
        update: anything else is refused here, from the host's knowledge alone, before the first step (and before the model
        or the device is asked for anything).  plan: the loop's fusion plan once it has one (None: refused whatever the
        reason), as in _check_dsg."""
        gain = self.guidance_gain
        if gain not in ("unit", "span"):
            raise ValueError(f"guidance_gain must be 'unit' or 'span' (got {gain!r})")
        order = self._check_solver_order()
        if gain == "unit" and order == 1:
            return
        method, kw = self._unwrap_cond_fn(measurement_cond_fn)
        what = "solver_order = 2" if order == 2 else "guidance_gain = 'span'"
        why = None
        if isinstance(method, ConjugateGradientConsistency):
            why = "the cg step has no fused plan (it replaces x0_hat by x0_hat + d and has its own update)"
        elif isinstance(method, SphericalGaussianGuidance):
            why = "dsg puts x_next on a sphere: it has no step size to scale and no update to add a history term to"
        elif isinstance(method, PseudoInverseGuidance):
            why = ("pgdm has no fused plan and its own weight (w_t follows from the step's record: there is no scale to "
                   "multiply and no x0_hat history)")
        else:
            why = {"sampler": "no fused plan: it needs a DDPM / DDIM sampler with the epsilon / learned_range / clip_denoised "
                              "posterior (a fixed-variance model has no fused step)",
                   "method": "no fused plan: it needs a ps-type conditioning method (per-op methods have no fused step) with "
                             f"a Gaussian noiser (got {getattr(getattr(method, 'noiser', None), '__name__', None)!r})",
                   "mask": "no fused plan: inpainting needs its mask bound to the conditioning function",
                   }.get(self._no_plan_reason(method, kw))
        if why is None and method.operator.name == 'inpainting' and not kernels.OpHandle._mask_fuses(*x_start.shape[-2:]):
            why = (f"no fused plan: the fused inpainting step exists on the float4 grid only, H * W a multiple of 4 (got "
                   f"{x_start.shape[-2]} x {x_start.shape[-1]})")
        if why is None and plan is None:
            why = f"no fused plan: {type(method.operator).__name__} has no fused step at {tuple(x_start.shape)}"
        if why is None and order == 2 and project:
            why = "a DiffStateGrad projection (project=True) takes the per-op path on its steps, which keeps no x0_hat history"
        if why is None and order == 2 and getattr(self, "global_resample", False):
            why = "with global (multi-rank) resampling the history would have to travel between ranks with the particles"
        if why is not None:
            raise NotImplementedError(f"{what} is not supported here: {why}")

    def _check_solver_order(self):
        if self.solver_order != 1:
            raise ValueError(f"solver_order is an option of the ddim samplers (sampler {type(self).__name__})")
        return 1

    def _check_repulsion(self, n=None, measurement=None, n_images=False):
        """The repulsion options, checked from the host's knowledge alone before the first step (and before the device is
        asked for anything); n, measurement, n_images: the trajectory's, for the particles per image (a loop that has no
        trajectory to settle passes none: it refuses the option whatever its shape)."""
        scale = kernels.repulse_strength(self.repulsion_scale, "repulsion_scale")
        if self.repulsion_bandwidth is not None:
            kernels.repulse_strength(self.repulsion_bandwidth, "repulsion_bandwidth")
        stop = self.repulsion_stop
        if isinstance(stop, bool) or not isinstance(stop, (int, float)) or not 0.0 <= stop <= 1.0:
            raise ValueError(f"repulsion_stop must be a number in [0, 1] (got {stop!r})")
        if scale == 0.0:
            return
        why = None
        if isinstance(self, SearchDDPM):
            why = "search_ddpm keeps one state per image: there is nothing to push apart"
        elif isinstance(self, SMC_DDPM):
            why = "smc_ddpm's proposal correction assumes the unrepulsed proposal"
        elif getattr(self, "global_resample", False):
            why = "with global (multi-rank) resampling an image's particles live on several ranks"
        elif self.particle_groups > 1:
            why = f"particle_groups = {self.particle_groups}: the step crosses the groups"
        elif self.rng_parity:
            why = "rng_parity replays the reference's loop, which has no such step"
        if why is not None:
            raise NotImplementedError(f"repulsion_scale = {self.repulsion_scale} is not supported here: {why}")
        if n_images is False:
            images = self._measurement_images(measurement, n) or 1
        else:
            images = self._segments(measurement, n, n_images)
        if n // images > kernels.REPULSE_MAX_K:
            raise NotImplementedError(f"repulsion_scale = {self.repulsion_scale}: {n // images} particles per image, the "
                                      f"repulsion step takes at most {kernels.REPULSE_MAX_K}")

    def _repulse(self, img, idx, images):
        """the repulsion step on the state a loop's step returned (repulsion_scale > 0; checked by _check_repulsion): the
        particles of every image pushed apart with strength repulsion_scale * betas[idx], on the steps with idx > 0 and
        idx / num_timesteps >= repulsion_stop; elsewhere img as it is.  -> a persistent buffer, valid until the next step"""
        if not self.repulsion_scale or idx <= 0 or idx / self.num_timesteps < self.repulsion_stop:
            return img
        img = kernels.f32c(img.detach(), "particles")
        out = self._repulse_out
        if out is None or out.shape != img.shape or out.device != img.device:
            out = self._repulse_out = torch.empty_like(img)
        return kernels.repulse(img, self.repulsion_scale * self.betas[idx], images or 1, self.repulsion_bandwidth, out=out)

    def _check_metric_trace(self, plan=None, cg=None, projecting=False, base_loop=True):
        """sampler.metric_trace runs in the fused branch of the base loop, one chain: anything else is refused before the
        first step"""
        if self.metric_trace is None:
            return
        why = None
        if not base_loop:
            why = f"sampler {type(self).__name__} has its own loop"
        elif cg is not None and isinstance(cg[0], PseudoInverseGuidance):
            why = "the pgdm step has no fused plan (its x0_hat lives in no step buffer)"
        elif cg is not None:
            why = "the cg step has no fused plan (x0_hat + d is its own quantity)"
        elif plan is None:
            why = "this sampler / conditioning method / shape has no fused plan (only the fused step leaves x0_hat in a buffer)"
        elif projecting:
            why = "a DiffStateGrad projection takes the per-op path on its steps"
        elif self.particle_groups > 1:
            why = f"particle_groups = {self.particle_groups} (the trace follows one chain)"
        if why is not None:
            raise NotImplementedError(f"metric_trace is an option of the fused base loop (ddpm / ddim, ps-type methods and "
                                      f"dsg), one chain: {why}")

    # -- RNG ---------------------------------------------------------------
    def _randn(self, like, stride=None, shape=None):
        """standard-normal draw shaped like `like` (or `shape` on like's device: no dummy tensor is allocated)"""
        if shape is not None:
            if self.rng_parity:
                return torch.randn(tuple(shape), dtype=torch.float32).to(like.device)
            return torch.randn(tuple(shape), dtype=torch.float32, device=like.device)
        if self.rng_parity:
            # replay of the reference's host RNG stream (tests): torch's CPU normal_() consumes the
            # generator differently for non-contiguous tensors, so the layout is part of the stream
            proxy = torch.empty(like.shape, dtype=torch.float32) if stride is None else \
                torch.empty_strided(tuple(like.shape), tuple(stride), dtype=torch.float32)
            return torch.randn_like(proxy).contiguous().to(like.device)
        return torch.randn_like(like, dtype=torch.float32)

    def _rand(self, n, like):
        """n uniforms in [0, 1) on like's device (fp32: multiples of 2^-24) -- the device resampling draw's input"""
        if self.rng_parity:
            return torch.rand(int(n), dtype=torch.float32).to(like.device)
        return torch.rand(int(n), dtype=torch.float32, device=like.device)

    @staticmethod
    def _check_resample_draw(value):
        if value not in ("multinomial", "device"):
            raise ValueError(f"resample_draw must be 'multinomial' or 'device' (got {value!r})")
        return value

    def _check_resample_scheme(self, draw, scheme=None, ess=None):
        """(scheme, ess) for kernels.resample / resample_draw, or None for the defaults (the plain entry points)"""
        scheme = self.resample_scheme if scheme is None else scheme
        ess = self.resample_ess if ess is None else ess
        kernels.resample_scheme_args(scheme, ess)                      # ValueError on an unknown scheme / tau outside [0, 1]
        if scheme == "multinomial" and ess is None:
            return None
        if getattr(self, "global_resample", False):
            raise NotImplementedError(f"resample_scheme = {scheme!r} / resample_ess = {ess!r} with global (multi-rank) "
                                      "resampling is not supported: the exchange keeps its own multinomial draw")
        if draw != "device":
            raise ValueError(f"resample_scheme = {scheme!r} / resample_ess = {ess!r} need resample_draw = 'device' "
                             f"(got {draw!r}): the schemes and the ESS trigger are the device draw's")
        return scheme, ess

    def _device_resample(self, n, d, segments, inv_scale, opts, src=None):
        """One resampling step of the device draw over d [n]: n uniforms (one per slot whatever the weights turn out to
        be, so the stream position does not depend on data and nothing is read back), then kernels.resample_draw ->
        ids, or with src kernels.resample (the draw and both gathers in one launch) -> (src[ids], d[ids], ids).
        opts: (scheme, ess), or None for the plain entry points.  Records last_resample_ids / _flags / _ess (the
        diagnostics are None without opts)."""
        kw = {} if opts is None else dict(scheme=opts[0], ess=opts[1], want_flags=True)
        u = self._rand(n, d)
        if src is None:
            out = kernels.resample_draw(d, u, segments, inv_scale, **kw)
            out = (out,) if opts is None else out                       # the bare ids without diagnostics
        else:
            out = kernels.resample(src, d, u, segments, inv_scale, **kw)
        out, diag = (out, (None, None)) if opts is None else (out[:-2], out[-2:])
        self.last_resample_ids, (self.last_resample_flags, self.last_resample_ess) = out[-1], diag
        return out[-1] if src is None else out

    @staticmethod
    def _check_noise_draw(value):
        if value not in ("torch", "device"):
            raise ValueError(f"noise_draw must be 'torch' or 'device' (got {value!r})")
        return value

    def _step_rng(self, idx, n, images=None):
        """the kernels.Rng of loop index idx for a batch of n rows (images=M: M images x n / M paths), or None with
        noise_draw = 'torch'.  Checked on every call, so a loop refuses a bad setting before its first launch."""
        if self._check_noise_draw(self.noise_draw) == "torch":
            return None
        if self.rng_parity:
            raise ValueError("noise_draw = 'device' draws its own stream: it cannot replay the reference's host RNG "
                             "(rng_parity)")
        per = n // int(images) if images is not None and int(images) > 1 else 0
        return kernels.Rng(self.noise_seed, idx, kernels.Rng.TAG_STEP, self.path_base, per)

    # -- q ------------------------------------------------------------------
    def q_sample(self, x_start, t):
        """reference :134-151 (two scalars times tensors: not worth a kernel, result unused by ps*)"""
        noise = self._randn(x_start, self.parity_measurement_stride)
        t = int(t)
        return float(np.float32(self.sqrt_alphas_cumprod[t])) * x_start + \
            float(np.float32(self.sqrt_one_minus_alphas_cumprod[t])) * noise

    # -- model timestep -----------------------------------------------------
    def _model_timesteps(self, device):
        """device tensor [T] of what the UNet receives as t for each loop index (reference :333-336)"""
        key = str(device)
        if key not in self._ts_cache:
            ts = np.arange(self.num_timesteps, dtype=np.float64)
            ts = ts * (1000.0 / self.num_timesteps) if self.rescale_timesteps else ts
            self._ts_cache[key] = torch.tensor(ts, dtype=torch.float32 if self.rescale_timesteps else torch.int64,
                                               device=device)
        return self._ts_cache[key]

    def _call_model(self, model, x, idx):
        return model(x, self._model_timesteps(x.device)[idx:idx + 1])

    # -- S1 -------------------------------------------------------------------
    def p_mean_variance(self, model, x, t):
        idx = int(t)
        model_output = self._call_model(model, x, idx)
        if model_output.shape[1] == 2 * x.shape[1]:
            model_output, model_var_values = torch.split(model_output, x.shape[1], dim=1)
        else:
            model_var_values = model_output
        model_mean, pred_xstart = self.mean_processor.get_mean_and_xstart(x, idx, model_output)
        model_variance, model_log_variance = self.var_processor.get_variance(model_var_values, idx)
        return {'mean': model_mean, 'variance': model_variance, 'log_variance': model_log_variance,
                'pred_xstart': pred_xstart}

    def p_sample(self, model, x, t, noise=None):
        raise NotImplementedError

    def sample_coefs(self, idx):
        """struct dpsx_coefs of this sampler's step at loop index idx (DDPM record; DDIM overrides)"""
        return self.step_coefs[idx]

    def _scale_timesteps(self, t):
        return t.float() * (1000.0 / self.num_timesteps) if self.rescale_timesteps else t

    # -- fusion plan ----------------------------------------------------------
    @staticmethod
    def _unwrap_cond_fn(fn):
        """-> (ConditioningMethod or None, bound keyword arguments)"""
        kw = {}
        while isinstance(fn, functools.partial):
            kw = {**fn.keywords, **kw}
            fn = fn.func
        method = getattr(fn, '__self__', None)
        if isinstance(method, ConditioningMethod) and getattr(fn, '__name__', '') == 'conditioning':
            return method, kw
        return None, kw

    def _no_plan_reason(self, method, kw):
        """The fusion rule, as far as the host alone knows it: which condition of a fused step this sampler and
        conditioning function (unwrapped: method, kw) miss -- "sampler", "method" or "mask" -- or None.  The shape is the
        handle's to judge (OpHandle.fuses_step)."""
        if not (self.hip_posterior and isinstance(self, (DDPM, DDIM))):
            return "sampler"            # another sampler, or a posterior the HIP S1 does not compute
        if method is None or method.fused_spec(**kw) is None:
            return "method"             # not a ConditioningMethod's conditioning, or one without a fused form
        if method.operator.name == 'inpainting' and kw.get('mask', None) is None:
            return "mask"               # inpainting without its mask bound to the conditioning function
        return None

    @staticmethod
    def _op_handle(operator, mask, like):
        """the operator's HIP handle: inpainting's belongs to the mask, every other to the operator (and like's shape)"""
        return operator.hip_handle_for(mask) if operator.name == 'inpainting' else operator.hip_handle(like)

    def _fusion_plan(self, measurement_cond_fn, x_start):
        method, kw = self._unwrap_cond_fn(measurement_cond_fn)
        if self._no_plan_reason(method, kw) is not None:
            return None
        op = method.operator
        if op.name != 'inpainting' and not hasattr(op, 'hip_handle'):
            return None
        handle = self._op_handle(op, kw.get('mask', None), x_start)
        # a shape the fused launches refuse (inpainting with H * W off the float4 grid): decided here, before the first
        # step, so the loop -- and the particle groups, which exist only under a plan -- takes the per-op path
        if not handle.fuses_step(*x_start.shape[1:]):
            return None
        return method, kw, handle

    def _check_dsg(self, measurement_cond_fn, x_start, plan=False):
        """The `dsg` method runs only where every step of a loop is the fused step and adds noise: anything else is refused
        here, from the host's knowledge alone, before the first step (and before the model or the device is asked for
        anything).  plan: the loop's fusion plan once it has one (None: refused whatever the reason).
        rng_parity needs no refusal: the fused step takes that path's host-drawn noise tensor, and the update reads the
        same tensor."""
        method, kw = self._unwrap_cond_fn(measurement_cond_fn)
        if not isinstance(method, SphericalGaussianGuidance):
            return
        if isinstance(self, SMC_DDPM):
            raise NotImplementedError("dsg under smc_ddpm is not supported: the weights' proposal correction assumes the "
                                      "Gaussian-shift proposal x_next = sample - s, and dsg's x_next is a point on a sphere")
        why = {"sampler": "it needs a DDPM / DDIM sampler with the epsilon / learned_range / clip_denoised posterior (a "
                          "fixed-variance model has no fused step)",
               "method": f"it needs a Gaussian noiser (got {getattr(method.noiser, '__name__', method.noiser)!r})",
               "mask": "inpainting needs its mask bound to the conditioning function",
               }.get(self._no_plan_reason(method, kw))
        # the shape is the handle's to judge (plan is None); inpainting's rule is said here, while there is no handle yet
        if why is None and method.operator.name == 'inpainting' and not kernels.OpHandle._mask_fuses(*x_start.shape[-2:]):
            why = (f"the fused inpainting step exists on the float4 grid only, H * W a multiple of 4 (got "
                   f"{x_start.shape[-2]} x {x_start.shape[-1]})")
        if why is None and plan is None:
            why = f"{type(method.operator).__name__} has no fused step at {tuple(x_start.shape)}"
        if why is not None:
            raise NotImplementedError("dsg has no fused plan here and runs nowhere else (the update needs the step's sd and "
                                      f"noise, which only the fused step has): {why}")
        if isinstance(self, DDIM) and not float(self.eta) > 0.0:
            raise ValueError(f"dsg under {type(self).__name__} with eta = {self.eta}: the step adds no noise, the sphere "
                             "has radius 0 and no guidance is possible (set eta > 0; eta = 1 is the method's setting)")

    def _buffers(self, handle, x):
        n, c, h, w = x.shape
        b = self._bufs
        if b is None or b[0] is not handle or b[1].shape != (n, c, h, w) or b[1].x0_hat.device != x.device:
            self._bufs = (handle, kernels.StepBuffers(handle, n, c, h, w, x.device))
        return self._bufs[1]

    def _loop_kw(self, idx, loop_kw):
        """the keyword arguments the calling loop passes to measurement_cond_fn besides the tensors (loop_kw=None, the base
        loop: beta_scale, t -- reference :230-236; ttc_ddim: none, {} -- :678-682)"""
        if loop_kw is None:
            return {'beta_scale': self.betas[idx], 't': idx / self.num_timesteps}
        return loop_kw

    def _step_spec(self, idx, method, cond_kw, loop_kw):
        """the method's fused_spec at loop index idx.  loop_kw: see _loop_kw"""
        spec = method.fused_spec(**self._loop_kw(idx, loop_kw), **cond_kw)
        if self.guidance_gain == "span" and spec is not None and "scale" in spec:
            spec = dict(spec, scale=spec["scale"] * self._step_span(idx))
        return spec

    def _fused_step(self, model, x_prev, idx, y, spec, handle, buf, stream, noise, rng, want_x0, corr_state=None):
        """The fused DPS step of one chain of particles -- model call, K1, [semantic term], K2, model VJP, K3 -- on `stream`
        (None: torch's current stream).  x_prev, noise, y and rng are the chain's own (already sliced); -> (x_next, the
        semantic term's distance or None).  K3 is kernels.step_update, step_update_dsg where the spec says "dsg" (refused
        with corr_state: _check_dsg), step_update_ms with solver_order = 2 (the ddim samplers; K1 then stores x0_hat on
        every step beside the previous step's), or step_update_corr with corr_state."""
        x_prev = x_prev.detach().requires_grad_()
        with torch.enable_grad():
            model_out = self._call_model(model, x_prev, idx)
        mo = kernels.f32c(model_out.detach(), "model output")
        if mo.shape[1] != 2 * x_prev.shape[1]:
            raise ValueError("the fused DPS step needs a learned-sigma model ([N, 2C, H, W] output)")
        coefs = self.sample_coefs(idx)
        if noise is None and rng is None:
            noise = self._randn(x_prev)
        multistep = self.solver_order == 2
        if multistep:                     # K1 writes this step's x0_hat beside the previous step's (no copy)
            buf.advance_x0()
        # x0_hat is consumed inside K1 (A(x0_hat), the clamp gate): the image itself is written out only when something
        # reads it afterwards -- the semantic term's embedder, a progress snapshot (want_x0), the multistep update
        kernels.step_fwd(handle, buf, kernels.f32c(x_prev.detach(), "x_t"), mo, noise, y, coefs,
                         want_x0=want_x0 or multistep or "semantic" in spec, stream=stream, rng=rng)
        g_sem = sem = None
        if "semantic" in spec:            # embedder forward + VJP on x0_hat (torch), between the two HIP halves
            g_sem, sem = spec["semantic"](buf.x0_hat)
        kernels.step_bwd(handle, buf, y, spec["scale"], spec["power"], coefs, g_x0_extra=g_sem, stream=stream)
        g_unet = None
        if model_out.requires_grad:
            (g_unet,) = torch.autograd.grad(model_out, x_prev, grad_outputs=buf.g_model_out.to(model_out.dtype))
            g_unet = kernels.f32c(g_unet, "UNet VJP")
        if "dsg" in spec:                 # the point on the sphere in K3's place
            x_next, _ = kernels.step_update_dsg(buf, g_unet, coefs, mo, spec["dsg"], noise=noise, rng=rng,
                                                stats=buf.dsg_stats(), stream=stream)
        elif multistep:                   # K3 + c (x0_hat - the previous step's), c = 0 on the first and the last step
            x_next = kernels.step_update_ms(buf, g_unet, coefs, self.solver_coef(idx), stream=stream)
        elif corr_state is None:
            x_next = kernels.step_update(buf, g_unet, coefs, stream=stream)
        else:
            x_next, _ = kernels.step_update_corr(buf, g_unet, coefs, mo, noise=noise, rng=rng, state=corr_state,
                                                 stream=stream)
        return x_next, sem

    def dps_step(self, model, x_prev, idx, measurement, method, cond_kw, handle, noise=None, loop_kw=None,
                 want_x0=False, rng=None, corr_state=None):
        """One fused DPS step at loop index idx.  Returns (x_next, norm[N]) -- device tensors that live in the
        sampler's persistent step buffers (valid until the next step; the loops clone what they hand out).
        loop_kw: see _step_spec.  corr_state (a kernels.SmcState; smc_ddpm): K3 is kernels.step_update_corr, which also
        leaves the step's proposal correction in corr_state.corr_partials."""
        buf = self._buffers(handle, x_prev)
        x_next, self._step_semantic = self._fused_step(
            model, x_prev, idx, kernels.f32c(measurement, "measurement"), self._step_spec(idx, method, cond_kw, loop_kw),
            handle, buf, None, noise, rng, want_x0, corr_state)
        return x_next, buf.norm

    def _particle_group_set(self, method, cond_kw, x, images=None):
        """the sampler's kernels.ParticleGroups for this operator / batch shape (built once, reused across trajectories);
        images=M: a multi-image batch, the groups hold whole images"""
        n, c, h, w = x.shape
        op, mask = method.operator, cond_kw.get('mask', None)
        key = (id(op), None if mask is None else (mask.data_ptr(), mask._version), (n, c, h, w), str(x.device),
               int(self.particle_groups), images)
        if self._pgroups is None or self._pgroups[0] != key:
            self._pgroups = (key, kernels.ParticleGroups(op, n, c, h, w, x.device, self.particle_groups, mask=mask, like=x,
                                                         images=images))
        return self._pgroups[1]

    @staticmethod
    def _measurement_images(measurement, n):
        """M when `measurement` holds one row per image of a multi-image batch (1 < M < N, particles [m K, (m + 1) K)
        belong to image m), None for one broadcast measurement or one per particle"""
        y_n = measurement.shape[0] if torch.is_tensor(measurement) and measurement.dim() > 0 else 1
        if y_n in (1, n):
            return None
        if y_n < 1 or n % y_n:
            raise ValueError(f"a measurement of {y_n} rows does not split {n} particles into whole images")
        return y_n

    def _segments(self, measurement, n, n_images, infer=True, refuse_multi=None):
        """The images of a call's particle set: M images x n / M particles, image-major.  The policy is the loop's:
        infer=True (the resampling loops): M is the measurement's row count where it holds one row per image, else
        n_images, else 1; refuse_multi: why this call cannot take M > 1 (NotImplementedError).
        infer=False (search_ddpm): only n_images= makes a multi-image batch, of a measurement with 1 or M rows; -> None
        without it."""
        if not infer:
            if n_images is None:
                if self._measurement_images(measurement, n) is not None:
                    raise ValueError(f"a measurement of {measurement.shape[0]} rows for {n} particles: pass n_images= for "
                                     "a multi-image batch")
                return None
            segments, y_n = int(n_images), measurement.shape[0]
            if segments < 1 or n % segments or y_n not in (1, segments):
                raise ValueError(f"n_images={segments}: {n} particles and a measurement of {y_n} rows do not form "
                                 f"{segments} images")
            return segments
        images, n_images = self._measurement_images(measurement, n), int(n_images or 1)
        if images is not None and n_images > 1 and images != n_images:
            raise ValueError(f"n_images={n_images} with a measurement of {images} rows")
        segments = images or n_images
        if segments > 1 and refuse_multi:
            raise NotImplementedError(refuse_multi)
        if segments < 1 or n % segments:
            raise ValueError(f"{n} particles do not split into {segments} images")
        return segments

    def _check_multi_image(self, plan, method, projecting, images, n, prefix=""):
        """a multi-image batch runs the fused ps / ps_anneal / ps_semantic-without-embedder step only (and `cg`, whose
        loops do not come here: every launch of its step takes one measurement row and one mask per image).
        prefix: what a sampler with a loop of its own puts in front of the refusal ("ttc_ddim: ")"""
        name = type(method).__name__ if method is not None else "this conditioning function"
        if plan is None or projecting:
            raise NotImplementedError(
                f"{prefix}multi-image batch ({images} measurements for {n} particles): {name} runs the per-op path, which "
                "takes one measurement or one per particle; only the fused ps / ps_anneal / ps_semantic (no embedder) step "
                "and DiffStateGrad off support one measurement per image")
        last = self.num_timesteps - 1
        if "semantic" in plan[0].fused_spec(beta_scale=self.betas[last], t=last / self.num_timesteps, **plan[1]):
            raise NotImplementedError(
                f"{prefix}multi-image batch ({images} images): semantic guidance has one target for all particles; "
                "per-image targets are not supported (set sem_guid_scale = 0 or run one image per call)")

    def dps_step_grouped(self, model, img, idx, measurement, method, cond_kw, pg, noise, loop_kw=None, want_x0=False,
                         rng=None):
        """dps_step over kernels.ParticleGroups: every group's whole step (_fused_step) is enqueued on the group's own
        stream; nothing is joined between steps (group j's next step reads only what group j wrote).  img, noise, rng: the
        full batch's; measurement: contiguous fp32 and alive until pg.join() (the loops convert it once per trajectory).
        Returns (x_next [N, C, H, W], norm [N]) -- views of the group set's full-batch buffers, valid on the CALLER's stream
        only after pg.join()."""
        y = kernels.f32c(measurement, "measurement")
        if y is not measurement and pg.record_streams:       # a direct caller's layout: the copy outlives the groups' work
            for stream in pg.streams:
                y.record_stream(stream)
        spec = self._step_spec(idx, method, cond_kw, loop_kw)
        pg.fork()                 # the noise (and, on the first step, x_start) was produced on the caller's stream
        sems = []
        for j in range(len(pg)):
            handle, buf, stream, noise_j, y_j, rng_j = pg.group_args(j, noise, y, rng)
            with torch.cuda.stream(stream):
                _, sem = self._fused_step(model, img[pg.slices[j]], idx, y_j, spec, handle, buf, stream, noise_j, rng_j,
                                          want_x0)
            if sem is not None:
                sems.append(sem)
        self._step_semantic = sems if sems else None
        return pg.x_next(), pg.full.norm

    # -- pseudoinverse guidance ('pgdm'): the cg route with the model's graph ------
    def _check_pgdm(self, measurement_cond_fn, project=False):
        """The `pgdm` method runs on the `cg` route of the ddpm / ddim / ttc_ddim loops, one chain: anything else is refused
        here, from the host's knowledge alone, before the first step (and before the model or the device is asked for
        anything)."""
        method, kw = self._unwrap_cond_fn(measurement_cond_fn)
        if not isinstance(method, PseudoInverseGuidance):
            return
        why = None
        if isinstance(self, SMC_DDPM):
            why = ("smc_ddpm's weights assume the Gaussian-shift proposal of the fused ps step, whose correction the pgdm "
                   "step does not compute")
        elif not (self.hip_posterior and isinstance(self, (DDPM, DDIM))):
            why = ("it needs a DDPM / DDIM sampler with the epsilon / learned_range / clip_denoised posterior (the HIP S1 and "
                   "its clamp gate; a fixed-variance model has none)")
        elif self.particle_groups > 1:
            why = f"particle_groups = {self.particle_groups}: groups exist under a fused plan only, pgdm runs one chain"
        elif project:
            why = ("a DiffStateGrad projection (project=True) projects the step's gradient as a tensor of its own, which the "
                   "pgdm step does not form (K3 applies its two terms directly)")
        elif method.operator.name == 'inpainting' and kw.get('mask', None) is None:
            why = "inpainting needs its mask bound to the conditioning function"
        if why is not None:
            raise NotImplementedError(f"pgdm is not supported here: {why}")

    def _pgdm_record(self, idx):
        """the step's record in float64, from the sampler's tables -> (a, b, c1, c2, ddim, abar, abar_prev)"""
        return (self.sqrt_recip_alphas_cumprod[idx], self.sqrt_recipm1_alphas_cumprod[idx], self.posterior_mean_coef1[idx],
                self.posterior_mean_coef2[idx], False, self.alphas_cumprod[idx], self.alphas_cumprod_prev[idx])

    def pgdm_scalars(self, idx, method):
        """(rho_t, gain_t) of the pgdm step at loop index idx: float64 from the tables, one fp32 rounding each
        (kernels.pgdm_scalars)"""
        key = (idx, float(getattr(self, "eta", 0.0)), method.noise_sigma, method.weighting, method.weight)
        cache = self.__dict__.setdefault('_pgdm_scalars', {})
        if key not in cache:
            *rec, abar, abar_prev = self._pgdm_record(idx)
            cache[key] = kernels.pgdm_scalars(abar, abar_prev, rec, method.noise_sigma, method.weighting, method.weight)
        return cache[key]

    def pgdm_step(self, model, x_prev, idx, measurement, method, cond_kw, noise=None, rng=None):
        """One `pgdm` step at loop index idx: the model forward with a graph, S1 with its clamp gate, the CG solve ended in
        the cotangent on the model's eps output (OpHandle.cg_pullback), the model VJP, K3.  Returns (x_next, dist[N]) in the
        operator handle's persistent buffers (valid until the next step; the loops clone what they hand out)."""
        x_prev = x_prev.detach().requires_grad_()
        with torch.enable_grad():
            model_out = self._call_model(model, x_prev, idx)
        mo = kernels.f32c(model_out.detach(), "model output")
        if mo.shape[1] != 2 * x_prev.shape[1]:
            raise ValueError("the pgdm step needs a learned-sigma model ([N, 2C, H, W] output)")
        coefs = self.sample_coefs(idx)
        if noise is None and rng is None:
            noise = self._randn(x_prev)
        x0_hat, sample, inside = kernels.posterior_fwd(kernels.f32c(x_prev.detach(), "x_t"), mo, noise, coefs,
                                                       want_inside=True, rng=rng)
        handle = self._op_handle(method.operator, cond_kw.get('mask', None), x0_hat)
        rho, gain = self.pgdm_scalars(idx, method)
        g_mo, dist = handle.cg_pullback(x0_hat, inside, kernels.f32c(measurement, "measurement"), rho, method.iters, gain)
        g_unet = None
        if model_out.requires_grad:
            (g_unet,) = torch.autograd.grad(model_out, x_prev, grad_outputs=g_mo.to(model_out.dtype))
            g_unet = kernels.f32c(g_unet, "UNet VJP")
        buf = handle.cg_buffers(*x0_hat.shape, x0_hat.device)
        buf.sample = sample
        return kernels.step_update(buf, g_unet, coefs), dist

    # -- the Jacobian-free step ('cg') -----------------------------------------
    def _cg_plan(self, measurement_cond_fn):
        """-> (method, bound keyword arguments) when measurement_cond_fn is the `cg` method's conditioning or `pgdm`'s
        (which runs on the same route: _check_pgdm has passed), else None"""
        method, kw = self._unwrap_cond_fn(measurement_cond_fn)
        if isinstance(method, PseudoInverseGuidance):
            return method, kw
        if not isinstance(method, ConjugateGradientConsistency):
            return None
        if self._no_plan_reason(method, kw) == "sampler":
            raise NotImplementedError("cg needs the epsilon / learned_range / clip_denoised posterior (the HIP S1) under a "
                                      "DDPM or DDIM sampler")
        return method, kw

    def cg_step(self, model, x_prev, idx, measurement, method, cond_kw, noise=None, rng=None):
        """One `cg` step at loop index idx: the model forward without a graph, S1, then method.conditioning (the CG solve
        and the sampler's step with x0_hat + d).  Returns (x_next, dist[N]) in the operator handle's persistent buffers
        (valid until the next step; the loops clone what they hand out)."""
        with torch.no_grad():
            x = kernels.f32c(x_prev.detach(), "x_t")
            mo = kernels.f32c(self._call_model(model, x, idx), "model output")
            if mo.shape[1] != 2 * x.shape[1]:
                raise ValueError("the cg step needs a learned-sigma model ([N, 2C, H, W] output)")
            coefs = self.sample_coefs(idx)
            if noise is None and rng is None:
                noise = self._randn(x)
            x0_hat, sample = kernels.posterior_fwd(x, mo, noise, coefs, rng=rng)
            return method.conditioning(x_t=sample, x_0_hat=x0_hat, measurement=kernels.f32c(measurement, "measurement"),
                                       coefs=coefs, **cond_kw)

    def _loop_step(self, model, img, idx, y, images, plan, cg=None, pg=None, **step_kw):
        """A loop's step where it is the `cg` step (cg given) or the fused step (plan; over the groups pg where given):
        the step's noise -- the counters of _step_rng or, with noise_draw = 'torch', a draw for the whole batch -- then the
        step.  y: the measurement, contiguous fp32 (converted once per trajectory).  -> (x_next, distance [N])"""
        rng = self._step_rng(idx, img.shape[0], images)
        noise = self._randn(img) if rng is None else None
        if self.rng_parity:
            self._randn(y, self.parity_measurement_stride)      # the reference's q_sample draw (:224, :668), result unused
        if cg is not None:
            step = self.pgdm_step if isinstance(cg[0], PseudoInverseGuidance) else self.cg_step
            return step(model, img, idx, y, cg[0], cg[1], noise=noise, rng=rng)
        if pg is not None:
            return self.dps_step_grouped(model, img, idx, y, plan[0], plan[1], pg, noise, rng=rng, **step_kw)
        return self.dps_step(model, img, idx, y, plan[0], plan[1], plan[2], noise=noise, rng=rng, **step_kw)

    def _per_op_step(self, model, img, idx, measurement, measurement_cond_fn, images, loop_kw):
        """A loop's step where it is neither of _loop_step's: p_sample with a graph back to x_t, the noisy measurement, and
        the conditioning function as the reference calls it (loop_kw: see _loop_kw).  The noise is p_sample's own torch
        draw or, with noise_draw = 'device', the same counters as the fused step's, filled by the stand-alone launch.
        -> (p_sample's dict, what measurement_cond_fn returned)"""
        img = img.detach().requires_grad_()
        rng = self._step_rng(idx, img.shape[0], images)
        out = self.p_sample(x=img, t=torch.tensor([idx], device=img.device), model=model,
                            noise=None if rng is None else kernels.randn(img.shape, rng, img.device))
        noisy_measurement = self.q_sample(measurement, t=idx)
        return out, measurement_cond_fn(x_t=out['sample'], measurement=measurement, noisy_measurement=noisy_measurement,
                                        x_prev=img, x_0_hat=out['pred_xstart'], **self._loop_kw(idx, loop_kw))

    def _trajectory(self, x_start, measurement, measurement_cond_fn, n_images=False, refuse_multi=None, project=False,
                    prefix=""):
        """What a guided loop settles before its first step, refusals first: `dsg` from the host's knowledge alone, the
        device, the fusion plan (and `dsg` again, now with it), the `cg` plan, the images of the batch and what a
        multi-image batch can run, noise_draw, and the measurement converted once (alive until a loop's groups are joined;
        None on the per-op route, which takes `measurement` as given).  The loop's policy:
        n_images: False (the base loop) -- the images are the measurement's rows, None for one image; else the call's
        n_images= for _segments (the resampling loops: always a count), with refuse_multi, why the call takes one image only;
        project: a DiffStateGrad projection is asked for (its steps take the per-op path);
        prefix: the sampler's name in front of a multi-image refusal."""
        img = x_start.detach()
        n = img.shape[0]
        self._check_dsg(measurement_cond_fn, img)
        self._check_pgdm(measurement_cond_fn, project)
        self._check_solver(measurement_cond_fn, img, project)
        self._check_repulsion(n, measurement, n_images)
        kernels.require_cuda(img, "x_start")
        plan = self._fusion_plan(measurement_cond_fn, img)
        self._check_dsg(measurement_cond_fn, img, plan)
        self._check_solver(measurement_cond_fn, img, project, plan)
        cg = self._cg_plan(measurement_cond_fn)
        method, _ = self._unwrap_cond_fn(measurement_cond_fn)
        if n_images is False:
            images = self._measurement_images(measurement, n)
        else:
            images = self._segments(measurement, n, n_images, refuse_multi=refuse_multi)
        if (images or 1) > 1 and cg is None:
            projecting = project and (method is None or method.returns_gradient)
            self._check_multi_image(plan, method, projecting, images, n, prefix)
        self._step_rng(0, n, images)      # validates noise_draw before the first step
        y = kernels.f32c(measurement, "measurement") if cg is not None or plan is not None else None
        return _Trajectory(img, n, method, plan, cg, images, y)

    # -- the base loop (reference :175-303) -------------------------------------
    def p_sample_loop(self, model, x_start, measurement, measurement_cond_fn, record, save_root, **kwargs):
        # DiffStateGrad (reference :203-204, 240-251): off by default; a projected step needs the gradient
        # itself, so it takes the per-op path; every other step keeps the fused launches
        period, project = kwargs.get('period', 20), kwargs.get('project', False)
        tr = self._trajectory(x_start, measurement, measurement_cond_fn, project=project)
        img, n, plan, cg, images, y = tr.img, tr.n, tr.plan, tr.cg, tr.images, tr.y
        ttc_driver_call = 'operator' in kwargs      # sample_condition_batched_ttc.py:91-100
        returns_gradient = True if tr.method is None else tr.method.returns_gradient
        project = project and returns_gradient
        distance, semantic = None, torch.zeros((), device=img.device)
        steps = range(self.num_timesteps - 1, -1, -1)
        if self.progress:
            from tqdm.auto import tqdm
            steps = tqdm(list(steps))
        self._check_metric_trace(plan, cg, project)
        trace = None if self.metric_trace is None else self.metric_trace.start(self.num_timesteps, img)
        # particle groups on streams (sampler.particle_groups > 1): only where every step is a fused step
        pg = None
        if plan is not None and self.particle_groups > 1 and n > 1 and not project:
            pg = self._particle_group_set(plan[0], plan[1], img, images=images)
        for idx in steps:
            projecting = project and period != 0 and idx % period == 0
            if cg is not None:
                img, distance = self._loop_step(model, img, idx, y, images, plan, cg=cg)
            elif plan is not None and not projecting:
                snapshot = bool(record) and idx % 100 == 0
                tracing = trace is not None and idx % trace.every == 0
                img, distance = self._loop_step(model, img, idx, y, images, plan, pg=pg, want_x0=snapshot or tracing)
                if tracing:               # one chain (_check_metric_trace): x0_hat and the distance are the step buffers'
                    trace.record(idx, self._bufs[1].x0_hat, distance)
                if snapshot and pg is not None:
                    pg.join()
                if self._step_semantic is not None:
                    semantic = self._step_semantic
            else:
                out, ret = self._per_op_step(model, img, idx, measurement, measurement_cond_fn, images, None)
                if not isinstance(ret, tuple):
                    ret = (ret,)
                if returns_gradient:
                    grad = ret[0].detach()
                    if projecting:
                        U, sv, Vh, rank = compute_svd_and_adaptive_rank(z_t=out['sample'].detach(), var_cutoff=0.99)
                        grad = apply_diffstategrad(norm_grad=grad, iteration_count=idx, period=period, U=U, s=sv,
                                                   Vh=Vh, adaptive_rank=rank)
                        if grad.shape[0] != out['sample'].shape[0]:       # [1, C, H, W] broadcasts at :255
                            grad = grad.expand_as(out['sample']).contiguous()
                    img = kernels.update(out['sample'].detach(), grad)                # :255
                else:
                    img = ret[0].detach()
                distance = ret[1] if len(ret) > 1 else None
                semantic = ret[2] if len(ret) > 2 and returns_gradient else semantic
            img = self._repulse(img, idx, images)
            if record and idx % 100 == 0:
                self._record(save_root, kwargs.get('path_curr_group_idx', 0), idx)
        if pg is not None:
            pg.join()
            if isinstance(semantic, list):
                semantic = torch.cat([v.reshape(-1) for v in semantic])
        # the fused step hands back views of the persistent ping-pong / norm buffers, which the next trajectory on
        # this sampler overwrites: what leaves the loop is a copy (one per 1000-step trajectory)
        img = img.clone()
        distance = distance.clone() if torch.is_tensor(distance) else distance
        self.last_measurement_distance, self.last_semantic_distance = distance, semantic
        if ttc_driver_call:
            return img
        return img, distance, semantic

    def _record(self, save_root, group, idx):
        """x0_hat snapshot of particle 0 every 100 steps (reference :296-301); best effort, off the hot path"""
        try:
            import matplotlib.pyplot as plt
        except ImportError:
            return
        if self._pgroups is not None and self.particle_groups > 1:
            x0 = self._pgroups[1].full.x0_hat[0]
        else:
            x0 = self._bufs[1].x0_hat[0] if self._bufs is not None else None
        if x0 is None or save_root is None:
            return
        a = x0.detach().float().cpu().numpy().transpose(1, 2, 0)
        a = (a - a.min()) / max(float(a.max() - a.min()), 1e-12)
        path = os.path.join(save_root, f"progress/path#{group + 1}")
        os.makedirs(path, exist_ok=True)
        plt.imsave(os.path.join(path, f"x_{str(idx).zfill(4)}.png"), a)


class SpacedDiffusion(GaussianDiffusion):
    """A diffusion process that keeps a subset of the base timesteps (reference :395-445)."""

    def __init__(self, use_timesteps, **kwargs):
        self.use_timesteps = set(use_timesteps)
        self.original_num_steps = len(kwargs["betas"])
        base_abar = np.cumprod(1.0 - np.array(kwargs["betas"], dtype=np.float64))
        self.timestep_map, new_betas, last = [], [], 1.0
        for i, abar in enumerate(base_abar):
            if i in self.use_timesteps:
                new_betas.append(1 - abar / last)
                last = abar
                self.timestep_map.append(i)
        kwargs["betas"] = np.array(new_betas)
        super().__init__(**kwargs)

    def _model_timesteps(self, device):
        key = str(device)
        if key not in self._ts_cache:
            ts = np.array(self.timestep_map, dtype=np.float64)
            if self.rescale_timesteps:                                   # reference :455-463
                self._ts_cache[key] = torch.tensor(ts, dtype=torch.float32, device=device) * \
                    (1000.0 / self.original_num_steps)
            else:
                self._ts_cache[key] = torch.tensor(ts, dtype=torch.int64, device=device)
        return self._ts_cache[key]

    def _scale_timesteps(self, t):
        return t


@register_sampler(name='ddpm')
class DDPM(SpacedDiffusion):
    def p_sample(self, model, x, t, noise=None):
        """reference :466-476.  The noise is drawn whether or not it is used (t == 0), as there."""
        idx = int(t)
        if noise is None:
            noise = self._randn(x)
        if self.hip_posterior:
            model_output = self._call_model(model, x, idx)
            x0, sample = kernels.PosteriorStepFn.apply(x, model_output, noise, self.step_coefs[idx])
            return {'sample': sample, 'pred_xstart': x0}
        out = self.p_mean_variance(model, x, t)
        sample = out['mean']
        if idx != 0:
            sample = sample + torch.exp(0.5 * out['log_variance']) * noise
        return {'sample': sample, 'pred_xstart': out['pred_xstart']}


@register_sampler(name='ddim')
class DDIM(SpacedDiffusion):
    #: the reference's p_sample takes eta per call and never passes it (:481); kept as the default
    eta = 0.0

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        # the default-eta records of every step, built once here (numpy fp32 scalar arithmetic, ~30 us each): built lazily
        # inside the loop they cost ten times that on the host once a process group's threads are alive (measured with a
        # one-rank RCCL group: 234 us of host time per step instead of 29)
        for t in range(self.num_timesteps):
            self.sample_coefs(t)
        self._solver_c = {0.0: self._solver_table(1.0), 1.0: self._solver_table(2.0)}

    #: 1: the DDIM rule; 2: DPM-Solver++(2M) (Lu et al. 2022) -- the DDIM step (its first-order form: eta = 0 the ODE, eta = 1
    #: the SDE) plus solver_coef(idx) * (x0_hat - the previous step's x0_hat), one launch in K3's place
    #: (kernels.step_update_ms).  Order 2 runs under a fused plan only, with eta 0 or 1; the loops refuse the rest.
    solver_order = 1

    def _solver_table(self, m):
        """c_i of the 2M step for every loop index, float64 rounded to fp32 once: with lambda = 0.5 ln(abar / (1 - abar)),
        h_i = lambda_{i-1} - lambda_i (the step from i lands on abar_{i-1}) and r_i = h_{i+1} / h_i,
            c_i = sqrt(abar_{i-1}) (1 - e^{-m h_i}) / (2 r_i)        m = 1: eta = 0 (ODE), m = 2: eta = 1 (SDE)
        and c = 0 at i = n - 1 (no history) and i = 0 (the step onto the clean image is first order)"""
        n, abar = self.num_timesteps, self.alphas_cumprod
        lam = 0.5 * np.log(abar / (1.0 - abar))
        c = np.zeros(n, dtype=np.float64)
        for i in range(1, n - 1):
            h, h_prev = lam[i - 1] - lam[i], lam[i] - lam[i + 1]
            c[i] = np.sqrt(abar[i - 1]) * (1.0 - np.exp(-m * h)) / (2.0 * (h_prev / h))
        return [float(np.float32(v)) for v in c]

    def _check_solver_order(self):
        order = self.solver_order
        if isinstance(order, bool) or order not in (1, 2):
            raise ValueError(f"solver_order must be 1 or 2 (got {order!r})")
        if order == 2 and float(self.eta) not in (0.0, 1.0):
            raise ValueError(f"solver_order = 2 is defined for eta = 0 (the ODE form) and eta = 1 (the SDE form), got eta = "
                             f"{self.eta}")
        return int(order)

    def solver_coef(self, idx):
        """the host scalar c of the multistep update at loop index idx (fp32-rounded; 0 at order 1)"""
        if self._check_solver_order() == 1:
            return 0.0
        return self._solver_c[float(self.eta)][idx]

    def sample_coefs(self, idx, eta=None):
        eta = self.eta if eta is None else eta
        key = (idx, float(eta))
        cache = self.__dict__.setdefault('_ddim_coefs', {})
        if key not in cache:
            cache[key] = kernels.make_ddim_coefs(self.sqrt_recip_alphas_cumprod[idx],
                                                 self.sqrt_recipm1_alphas_cumprod[idx], self.alphas_cumprod[idx],
                                                 self.alphas_cumprod_prev[idx], eta, idx != 0)
        return cache[key]

    def _pgdm_record(self, idx):
        abar, abar_prev, eta = self.alphas_cumprod[idx], self.alphas_cumprod_prev[idx], np.float64(self.eta)
        sigma = eta * np.sqrt((1.0 - abar_prev) / (1.0 - abar)) * np.sqrt(1.0 - abar / abar_prev)
        return (self.sqrt_recip_alphas_cumprod[idx], self.sqrt_recipm1_alphas_cumprod[idx], np.sqrt(abar_prev),
                np.sqrt(max(1.0 - abar_prev - sigma ** 2, 0.0)), True, abar, abar_prev)

    def p_sample(self, model, x, t, eta=None, noise=None):
        """reference :479-509.  The noise is drawn whether or not it is used, as there (:493)."""
        idx = int(t)
        if noise is None:
            noise = self._randn(x)
        if self.hip_posterior:
            model_output = self._call_model(model, x, idx)
            x0, sample = kernels.PosteriorStepFn.apply(x, model_output, noise, self.sample_coefs(idx, eta))
            return {'sample': sample, 'pred_xstart': x0}
        # other mean / variance parameterisations: device tensor arithmetic in the reference's op order
        eta = self.eta if eta is None else eta
        out = self.p_mean_variance(model, x, t)
        a = float(np.float32(self.sqrt_recip_alphas_cumprod[idx]))
        b = float(np.float32(self.sqrt_recipm1_alphas_cumprod[idx]))
        eps = (a * x - out['pred_xstart']) / b
        abar = float(np.float32(self.alphas_cumprod[idx]))
        abar_prev = float(np.float32(self.alphas_cumprod_prev[idx]))
        sigma = eta * math.sqrt((1 - abar_prev) / (1 - abar)) * math.sqrt(1 - abar / abar_prev)
        sample = out['pred_xstart'] * math.sqrt(abar_prev) + math.sqrt(1 - abar_prev - sigma ** 2) * eps
        if idx != 0:
            sample = sample + sigma * noise
        return {'sample': sample, 'pred_xstart': out['pred_xstart']}


@register_sampler(name='search_ddpm')
class SearchDDPM(DDPM):
    """Best-of-N per step: every particle is replaced by the one whose proposal is closest to y
    (reference :592-641).  Scoring, argmin and the winner's replication are HIP; the winner's index
    never leaves the device."""

    #: optional hook for multi-GPU runs: callable(costs_local, particles_local, n_out=None) -> n_out copies of the
    #: global winner (default: as many as particles_local)
    global_select = None
    #: After a select every particle is a copy of the winner (reference :633), so from the second step on the loop keeps
    #: ONE state particle: one model evaluation per step instead of N, S1 reads the state once for all N proposals, the
    #: winner is copied out once (dpsx_search_step_one_f32).  Results are those of the replicated form (the per-particle
    #: noise draws, costs and winner indices are the same); False keeps N copies as the reference does.
    single_state = True

    #: Beam search: B > 1 keeps the B best proposals of every image per step instead of one (dpsx_search_step_beam_f32).
    #: The first step scores the N given particles; every later step runs from the [images * B] surviving states -- one
    #: model evaluation per state, N / (images * B) proposals from each, the per-image top-B select on the device (the
    #: step without noise: one proposal per state, the select ranks the B survivors).  1: the greedy loop below, untouched.
    beam_width = 1

    @property
    def last_parents(self):
        """[images * B] int64: the beam (0 .. B - 1, inside its image) whose proposal each survivor of the last beam step
        was -- (last_best % per) // K with per = N / images proposals per image, K = per / B per beam (per = B, K = 1 at
        the step without noise, where every state proposes once)"""
        per, k = self._beam_geom
        return (self.last_best % per) // k

    def _proposal_noise(self, like, n, idx, segments, noise):
        """the noise source of a step's n proposals -> (noise, rng): the caller's tensor; else the record of the in-launch
        draw (noise_draw = 'device'); else a torch draw [n, C, H, W] on like's device"""
        rng = self._step_rng(idx, n, segments) if noise is None else None
        if noise is None and rng is None:
            noise = self._randn(like, shape=None if like.shape[0] == n else (n,) + tuple(like.shape[1:]))
        return noise, rng

    def _search(self, launch, model, states, proposals, idx, measurement, noise, segments, **kw):
        """the body of the three steps below: the model on `states`, the noise source of the proposals, then `launch` (a
        handle's search_step*: S1 -> scoring launch -> costs + select -> the winners' copy: one library call, nothing
        leaves the device) -> its (winners, sample, costs, best, costs[best]), best kept in last_best"""
        with torch.no_grad():
            model_out = self._call_model(model, states, idx)
        noise, rng = self._proposal_noise(states, proposals, idx, segments, noise)
        out = launch(states, model_out, noise, measurement, self.step_coefs[idx], segments=segments, rng=rng, **kw)
        self.last_best = out[3]
        return out

    def search_step(self, model, img, idx, measurement, handle, noise=None, segments=None):
        local = self.global_select is None
        x_next, sample, costs, _, _ = self._search(handle.search_step, model, img, img.shape[0], idx, measurement, noise,
                                                   segments, replicate=local)
        if not local:
            return self.global_select(costs, sample), costs
        return x_next, costs

    def search_step_one(self, model, state, n, idx, measurement, handle, noise=None, segments=None):
        """One step from the single state particle `state` [1,C,H,W] -> (winner [1,C,H,W], costs [n]).
        segments=M: one state per image, [M,C,H,W] -> (winners [M,C,H,W], costs [n])."""
        local = self.global_select is None
        # n=: read with the in-launch draw only (a noise tensor brings its own count)
        winner, sample, costs, _, _ = self._search(handle.search_step_one, model, state, n, idx, measurement, noise,
                                                   segments, want_winner=local, n=n)
        if not local:
            winner = self.global_select(costs, sample, n_out=1)
        return winner, costs

    def search_step_beam(self, model, states, n, idx, measurement, handle, noise=None, segments=None):
        """One beam step from `states` [S,C,H,W] (S = n on the first step, images * beam_width after it): n proposals,
        n / S per state -> (survivors [images * beam_width, C, H, W], costs [n], their costs [images * beam_width])."""
        winners, _, costs, _, val = self._search(handle.search_step_beam, model, states, n, idx, measurement, noise,
                                                 segments, n=n, beam=self.beam_width)
        return winners, costs, val

    def _beam_loop(self, model, x_start, measurement, operator, **kwargs):
        """p_sample_loop with beam_width = B > 1"""
        img, n = x_start.detach(), x_start.shape[0]
        beam = int(self.beam_width)
        segments = self._segments(measurement, n, kwargs.get('n_images', None), infer=False)
        per = n // (segments or 1)
        if beam < 1 or per % beam:
            raise ValueError(f"beam_width = {beam} does not divide the {per} particles per image")
        if self.global_select is not None:
            raise NotImplementedError("beam_width > 1 with a global (multi-rank) select is not supported: the champion "
                                      "exchange picks one winner, not the B best across ranks")
        if not self.single_state:
            raise ValueError("beam_width > 1 runs from the surviving states only: single_state = False does not apply")
        kernels.require_cuda(img, "x_start")
        if not self.hip_posterior:
            raise NotImplementedError("search_ddpm runs the epsilon / learned_range / clip configuration")
        handle = self._op_handle(operator, kwargs.get('mask', None), img)
        self.best_paths, self.best_costs = [], []
        self._step_rng(0, n, segments)    # validates noise_draw before the first step
        state = img                       # the first step: n states, one proposal each; then [images * beam]
        for idx in range(self.num_timesteps - 1, -1, -1):
            # the step that adds no noise (the last one): the proposals of one state would all be equal and fill the beam
            # with copies of the best state's, so every state proposes once and the select only ranks the survivors
            m = n if self.step_coefs[idx].add_noise & 1 else state.shape[0]
            self._beam_geom = (m // (segments or 1), max(m // (segments or 1) // beam, 1))
            state, costs, kept = self.search_step_beam(model, state, m, idx, measurement, handle, segments=segments)
            if kwargs.get('trace', False):
                self.best_costs.append(costs)
        self.beam_states, self.beam_costs = state, kept
        return state.repeat_interleave(per // beam, dim=0)     # image-major, then rank-major: the call's [N, ...] shape

    def p_sample_loop(self, model, x_start, measurement, measurement_cond_fn, record, save_root, operator,
                      potential_type='min', resample_every_steps=10, rs_temp=0.1, **kwargs):
        self._check_metric_trace(base_loop=False)
        self._check_repulsion()
        if self.beam_width != 1:
            return self._beam_loop(model, x_start, measurement, operator, **kwargs)
        img = x_start.detach()
        kernels.require_cuda(img, "x_start")
        if not self.hip_posterior:
            raise NotImplementedError("search_ddpm runs the epsilon / learned_range / clip configuration")
        handle = self._op_handle(operator, kwargs.get('mask', None), img)
        self.best_paths, self.best_costs = [], []
        n = img.shape[0]
        # n_images=M: M images x n / M particles (image-major), measurement [1 or M, ...]: every select is per image
        # (last_best: [M] global particle indices) and the state is one particle per image
        segments = self._segments(measurement, n, kwargs.get('n_images', None), infer=False)
        if (segments or 1) > 1 and self.global_select is not None:
            raise NotImplementedError("n_images > 1 with a global (multi-rank) select is not supported: the champion "
                                      "exchange picks one winner for all particles")
        per = n // (segments or 1)
        self._step_rng(0, n, segments)    # validates noise_draw before the first step
        state = None                      # the single state particle(s), once a select has made all particles equal
        for idx in range(self.num_timesteps - 1, -1, -1):
            if state is None:
                img, costs = self.search_step(model, img, idx, measurement, handle, segments=segments)
                if self.single_state and per > 1:
                    state = img[::per] if segments is not None else img[:1]
            else:
                state, costs = self.search_step_one(model, state, n, idx, measurement, handle, segments=segments)
            if kwargs.get('trace', False):
                self.best_costs.append(costs)
        if state is not None:             # the reference returns N copies of the final winner
            return state.repeat_interleave(per, dim=0) if segments is not None else state.repeat(n, 1, 1, 1)
        return img.clone()

    @torch.no_grad()
    def resample_update(self, candidates, denoised_candidates, operator, measurement, resample=True, rs_temp=0.01,
                        prev_costs=None, potential_type='min', steps_done=1, **kwargs):
        """reference :515-587 (defined there, never called by its loops): multinomial resampling on the accumulated
        costs, then the cost update.  The draw is torch.multinomial ([N] weights, RNG parity); the particle gathers
        and the cost update -- ||y - A(x)||_1^2 / CHW per particle combined with the previous costs by
        `potential_type` -- are HIP (dpsx_gather_f32, dpsx_resample_cost_f32: one launch).
        kwargs: `mask` for inpainting (the reference calls operator.forward without it and raises there)."""
        if potential_type not in ('mean', 'min', 'diff', 'curr'):
            raise NotImplementedError
        n = denoised_candidates.shape[0]
        draw = self._check_resample_draw(kwargs.get('resample_draw', None) or self.resample_draw)
        segments = self._segments(measurement, n, kwargs.get('n_images', None), refuse_multi=None if draw == "device" else (
            "resample_update over a multi-image batch is not supported: the multinomial draw would mix particles of "
            "different images (it needs a per-image RNG stream policy; resample_draw='device' draws per image)"))
        opts = self._check_resample_scheme(draw, kwargs.get('resample_scheme', None), kwargs.get('resample_ess', None))
        ids = None                        # stays None where nothing is drawn: the particles keep their places
        if resample and prev_costs is not None and draw == "device":
            # a flat segment keeps its particles: the draw's identity rule
            inv = rs_temp / steps_done if potential_type == 'mean' else rs_temp
            ids = self._device_resample(n, prev_costs, segments, inv, opts)
        elif resample and prev_costs is not None:
            pot = torch.exp(-rs_temp * prev_costs / steps_done) if potential_type == 'mean' \
                else torch.exp(-rs_temp * prev_costs)
            if pot.max() != pot.min():                                                     # :545
                ids = torch.multinomial(pot.cpu(), n, replacement=True).to(pot.device) if self.rng_parity \
                    else torch.multinomial(pot, n, replacement=True)
                self.last_resample_ids = ids
        if ids is not None:               # drawn over [0, n) either way: nothing to validate
            candidates = kernels.gather(candidates, ids, validate=False)
            denoised_candidates = kernels.gather(denoised_candidates, ids, validate=False)
            prev_costs = kernels.gather(prev_costs.reshape(n, 1), ids, validate=False).reshape(n)
        handle = self._op_handle(operator, kwargs.get('mask', None), denoised_candidates)
        self.last_curr_costs, net = handle.resample_cost(denoised_candidates, measurement, prev_costs, potential_type)
        return candidates, net


@register_sampler(name='ttc_ddim')
class TTC_DDIM(DDIM):
    """DDIM + multinomial particle resampling every 10 steps (reference :644-707).

    Multi-GPU (SURVEY.md 8e iii): with `global_resample` set (the driver does when WORLD_SIZE > 1) the weights of
    all ranks' particles are all-gathered, every rank draws the same ids from `resample_generator` (a host
    generator seeded identically on all ranks) and fetches its slots of the resampled set -- the same particle
    set one process holding all particles would produce from that generator.

    `resample_draw = "device"`: the draw is the library's own (include/dpsx.h "resampling draw": integer weights
    normalised by the best particle, an exact integer CDF, one torch.rand per slot) and runs with both gathers in ONE
    launch (kernels.resample).  It is defined per image, so a measurement with one row per image (or `n_images = M`)
    is accepted in that mode: image m's particles are resampled among themselves, and fed the same uniforms they are
    what a single-image run draws, bit for bit.  The default stays torch.multinomial over all N weights, and
    `global_resample` (several ranks) keeps its own multinomial draw whatever this option says.

    `resample_scheme` ("stratified", "systematic") and `resample_ess` (tau: an image resamples only while its effective
    sample size is below tau K, decided inside the launch) are options of the device draw; `resample_every` is the
    loop's resampling period.  After a resampling step with a non-default scheme or tau, `last_resample_flags` /
    `last_resample_ess` hold the per-image diagnostics."""

    global_resample = False
    resample_generator = None
    #: how the drawn particles travel between ranks: "selected" (one all-to-all of the drawn ones, each once per
    #: destination), "all" (all-gather of every state, no host read of device ids) or "auto" (distributed.resample_particles)
    resample_fetch = "auto"
    #: the loop resamples after every step whose index is a multiple of this (the reference's hard-coded 10);
    #: resample_every = 1 with resample_ess = 0.5 is adaptive SMC: look at every step, shuffle only degenerate images
    resample_every = 10
    _resample_segments = 1
    _resample_opts = None
    _drawn_ids = None

    def p_sample_loop(self, model, x_start, measurement, measurement_cond_fn, record, save_root, **kwargs):
        self._check_metric_trace(base_loop=False)
        draw = self._check_resample_draw(self.resample_draw)
        resample_every_steps, resample_scale = self._check_resample_every(self.resample_every), 100
        self._resample_opts = self._check_resample_scheme(draw)
        refuse_multi = None               # why this call's particles are one image's
        if draw != "device":
            refuse_multi = ("ttc_ddim over a multi-image batch is not supported: its resampling would mix particles of "
                            "different images (it needs a per-image RNG stream policy: resample_draw = 'device' draws "
                            "per image)")
        elif self.global_resample:
            refuse_multi = ("ttc_ddim over a multi-image batch with global (multi-rank) resampling is not supported: the "
                            "exchange draws over all ranks' particles as one set")
        # 'ps'-type methods run the three fused launches with the DDIM variant of S1; the rest (e.g. 'mcg', the
        # method whose two return values fit the reference loop's unpacking at :672) go through the per-op path
        tr = self._trajectory(x_start, measurement, measurement_cond_fn, n_images=kwargs.get('n_images', None),
                              refuse_multi=refuse_multi, prefix="ttc_ddim: ")
        img, plan, cg, segments, y = tr.img, tr.plan, tr.cg, tr.images, tr.y
        distance = None
        self.last_resample_ids = self.last_resample_flags = self.last_resample_ess = None
        self._resample_segments = segments      # the images of this trajectory's particle set (_resample draws per image)
        for idx in range(self.num_timesteps - 1, -1, -1):
            if cg is not None:
                img, distance = self._loop_step(model, img, idx, y, segments, plan, cg=cg)
            elif plan is not None:
                # this loop passes no beta_scale / t to the conditioning method (:678-682): same on both routes
                img, distance = self._loop_step(model, img, idx, y, segments, plan, loop_kw={})
            else:
                _, ret = self._per_op_step(model, img, idx, measurement, measurement_cond_fn, segments, {})
                img, distance = ret[0].detach(), ret[1].detach()
            img = self._repulse(img, idx, segments)
            if idx % resample_every_steps == 0:
                img, distance = self._resample(img, distance, resample_scale)
                ids = self._drawn_ids
                if self.solver_order == 2 and ids is not None:
                    # the x0_hat the next step reads as its history moves with the particles: this resampling's ids
                    buf = self._bufs[1]
                    buf.set_x0_history(kernels.gather(buf.x0_hat, ids, validate=False))
        return img.clone(), distance.clone()

    @staticmethod
    def _check_resample_every(value):
        try:
            if isinstance(value, bool):
                raise TypeError
            every = _index(value)
        except TypeError:
            every = 0
        if every < 1:
            raise ValueError(f"resample_every must be a positive integer (got {value!r})")
        return every

    def _resample(self, img, distance, resample_scale):
        """_resample_block -> (particles, distances); the ids THIS call drew (None where it drew none: a skipped
        resampling leaves last_resample_ids as it was) are handed back in `_drawn_ids`"""
        img, distance, self._drawn_ids = self._resample_block(img, distance, resample_scale)
        return img, distance

    def _resample_block(self, img, distance, resample_scale):
        """the resampling block (:685-698): w = exp(-d / 100), multinomial with replacement, skipped when all
        weights are equal.  By default the draw is torch.multinomial (RNG parity) and the particle gather is HIP; with
        resample_draw = "device" the draw and both gathers are one launch (_device_resample), and with global_resample
        the ranks' exchange draws.  -> (particles, distances, the ids this call drew or None where it drew none)"""
        n = len(distance)
        if self.global_resample:
            from . import distributed as dd
            img, distance, ids = dd.global_resample(img, distance, resample_scale, self.resample_generator,
                                                     fetch=self.resample_fetch)
            self.last_resample_ids = ids if ids is not None else self.last_resample_ids
            return img, distance, ids
        if self.resample_draw == "device":
            # one launch: per-image draw + both gathers.  img / distance are views of the persistent step buffers on the
            # fused route (the launch's src / d), the results are fresh tensors
            return self._device_resample(n, distance, self._resample_segments, 1.0 / resample_scale, self._resample_opts,
                                         src=img)[:3]
        if n <= 1:
            return img, distance, None
        weights = torch.exp(-distance / resample_scale)
        if self.rng_parity:                      # replay of the reference's host RNG stream (tests)
            if weights.max() == weights.min():
                return img, distance, None
            ids = torch.multinomial(weights.cpu(), n, replacement=True).to(img.device)
        else:
            # no host read: when all weights are equal the draw is replaced by the identity on the device
            # ([N]-sized glue; an all-zero weight vector must not reach multinomial)
            flat = weights.max() == weights.min()
            drawn = torch.multinomial(torch.where(flat, torch.ones_like(weights), weights), n, replacement=True)
            ids = torch.where(flat, torch.arange(n, device=img.device), drawn)
        self.last_resample_ids = ids
        return (kernels.gather(img, ids, validate=False),
                kernels.gather(distance.reshape(n, 1), ids, validate=False).reshape(n), ids)


@register_sampler(name='smc_ddpm', extension=True)
class SMC_DDPM(DDPM):
    """The DDPM DPS loop as a sequential Monte Carlo sampler: every particle carries the twisted-SMC log-weight of the
    guided step (include/dpsx.h "particle weights"; Wu et al. 2023) and the particles of an image are resampled from
    those weights.  Per step the negative log-weight E gains

        twist_scale (d^p - d_prev^p)  -  proposal_weight (log p_model(x_{t-1} | x_t) - log q_guided(x_{t-1} | x_t))

    with d = ||y - A(x0_hat)|| the step's distance.  The second term is summed inside the update launch
    (kernels.step_update_corr in K3's place), the recurrence is one small launch (kernels.smc_accum), and after every step
    whose index is a positive multiple of `resample_every` the device draw (kernels.resample, inv_scale = 1 on E) resamples
    each image's particles; an image that resampled restarts from E = 0.  The DDPM noise keeps resampled copies apart.

    Options: twist_scale (0.01: ttc_ddim's 1 / 100), twist_power (1 or 2), proposal_weight (1: the exact weight; 0: the
    Feynman-Kac "difference" potential alone), and ttc_ddim's resample_scheme / resample_ess / resample_every.  The draw
    is always the device draw.  After a loop: last_neg_log_weights (E after the last step, not reset), last_resample_ids /
    last_resample_flags / last_resample_ess (the last resampling).  Returns (particles, distances) like ttc_ddim.
    Needs a fused plan; refuses particle_groups > 1, rng_parity and global (multi-rank) resampling before any launch."""

    twist_scale = 0.01
    twist_power = 1
    proposal_weight = 1.0
    resample_every = 10
    last_neg_log_weights = None
    last_resample_ids = None

    def _smc_options(self):
        """the validated options -> (twist_scale, twist_power, proposal_weight, resample_every, scheme, ess)"""
        scale, weight = float(self.twist_scale), float(self.proposal_weight)
        if not (math.isfinite(scale) and math.isfinite(weight)):
            raise ValueError(f"twist_scale and proposal_weight must be finite (got {self.twist_scale!r}, "
                             f"{self.proposal_weight!r})")
        if isinstance(self.twist_power, bool) or self.twist_power not in (1, 2):
            raise ValueError(f"twist_power must be 1 or 2 (got {self.twist_power!r})")
        every = TTC_DDIM._check_resample_every(self.resample_every)
        if self.particle_groups > 1:
            raise ValueError("smc_ddpm with particle_groups > 1 is not supported: the weights and the resampling are over "
                             "the whole particle set")
        if self.rng_parity:
            raise ValueError("smc_ddpm has no reference loop whose host RNG stream rng_parity could replay")
        if getattr(self, "global_resample", False):
            raise NotImplementedError("smc_ddpm with global (multi-rank) resampling is not supported: the weights live on "
                                      "one rank")
        kernels.resample_scheme_args(self.resample_scheme, self.resample_ess)       # ValueError: unknown scheme / tau
        return scale, int(self.twist_power), weight, every, self.resample_scheme, self.resample_ess

    def p_sample_loop(self, model, x_start, measurement, measurement_cond_fn, record, save_root, **kwargs):
        self._check_metric_trace(base_loop=False)
        self._check_repulsion()
        scale, power, weight, every, scheme, ess = self._smc_options()
        method, kw = self._unwrap_cond_fn(measurement_cond_fn)
        self._check_pgdm(measurement_cond_fn)
        if self._no_plan_reason(method, kw) in ("sampler", "method"):
            name = type(method).__name__ if method is not None else "this conditioning function"
            raise NotImplementedError(f"smc_ddpm needs the fused ps / ps_anneal / ps_semantic step under the epsilon / "
                                      f"learned_range / clip_denoised posterior: {name} has no fused plan")
        tr = self._trajectory(x_start, measurement, measurement_cond_fn, n_images=kwargs.get('n_images', None),
                              prefix="smc_ddpm: ")
        img, n, plan, segments, y = tr.img, tr.n, tr.plan, tr.images, tr.y
        if plan is None:                  # the rest of the rule: inpainting's mask unbound, a shape the handle refuses
            raise NotImplementedError(f"smc_ddpm: {type(method).__name__} on {tuple(img.shape)} particles has no fused plan "
                                      "(the per-op path computes no proposal correction)")
        state = kernels.SmcState(n, img.shape[1:], img.device)
        reset, distance = None, None
        self.last_resample_ids = self.last_resample_flags = self.last_resample_ess = None
        for idx in range(self.num_timesteps - 1, -1, -1):
            img, distance = self._loop_step(model, img, idx, y, segments, plan, corr_state=state)
            kernels.smc_accum(state, distance, reset, segments, scale, power, weight)
            reset = None
            if idx % every == 0 and idx > 0:
                # one launch: per-image draw on E + the particle gather; the flags reset the resampled images' weights in
                # the next smc_accum, which also brings the increment still missing through the gathered d_prev
                img, _, ids = self._device_resample(n, state.E, segments, 1.0, (scheme, ess), src=img)
                reset = self.last_resample_flags
                state.d_prev = kernels.gather(state.d_prev.reshape(n, 1), ids, validate=False).reshape(n)
        self.last_neg_log_weights = state.E
        self.last_measurement_distance = distance.clone()
        return img.clone(), distance.clone()
