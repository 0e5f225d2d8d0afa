"""Conditioning methods -- the reference's registry API
(guided_diffusion/condition_methods.py) over the HIP kernels.

    get_conditioning_method(name, operator, noiser, **params) -> cm     (condition_methods.py:18)
    cm.conditioning(x_prev=, x_t=, x_0_hat=, measurement=, **kw)
        'ps' / 'ps_anneal' / 'mcg' / 'ps+'  -> (x_t_updated, norm, ...)  (:85-106, 206-232)
        'ps_semantic'                       -> (norm_grad, measurement_err, semantic_err)   (:190-195)
        'cg' (not in the reference)         -> (x_{t-1}, dist): needs coefs= from the loop, no autograd graph
        'dsg' (not in the reference)        -> raises: it runs inside the fused step only (kernels.step_update_dsg)
        'pgdm' (not in the reference)       -> raises: it needs the model's graph (GaussianDiffusion.pgdm_step)

Called on tensors that came out of this package's p_sample (PosteriorStepFn) and
operator.forward (OperatorFn), `torch.autograd.grad` walks:  UNet  <-  [HIP S1 VJP]
<-  [HIP A^T]  <-  [HIP norm VJP].  The samplers in gaussian_diffusion.py bypass
this per-op chain with the three fused launches when `fused_spec()` allows it.
"""
import functools
import math
from abc import ABC, abstractmethod

import torch

from .kernels import ResidualNormFn
from .measurements import LinearOperator

__CONDITIONING_METHOD__ = {}      # the reference's methods, under the reference's names
__EXTENSION_METHOD__ = {}         # methods the reference does not have ('cg'): same lookup, their own table
__FUSED_ONLY_METHOD__ = {}        # extensions that exist inside the fused step only ('dsg'): conditioning() raises
# every later extension ('pgdm' onwards), whatever route it runs on: the class says how it runs, not the table.  The three
# tables above stay as they are; this one is open and is consulted last.
__LATER_EXTENSION_METHOD__ = {}
_TABLES = (__CONDITIONING_METHOD__, __EXTENSION_METHOD__, __FUSED_ONLY_METHOD__, __LATER_EXTENSION_METHOD__)


def register_conditioning_method(name: str, extension: bool = False, fused_only: bool = False, later: bool = False):
    """extension=True: a method that is not in the reference; it is found by get_conditioning_method like the others
    and kept out of the table that mirrors the reference's registry.
    fused_only=True (extensions only): a method with no per-op form -- its conditioning() cannot be called, the sampling
    loops run it through its fused_spec() -- listed apart from the extensions whose conditioning() a loop calls
    later=True (extensions only): the open table of the extensions added after `cg` and `dsg`
    A name is registered once across all tables."""
    if fused_only and not extension:
        raise ValueError("fused_only is an option of extension methods: every method of the reference has a per-op form")
    if later and (fused_only or not extension):
        raise ValueError("later is an option of extension methods, and the open table has no fused_only part")

    def wrapper(cls):
        if any(t.get(name, None) for t in _TABLES):
            raise NameError(f"Name {name} is already registered!")
        table = __LATER_EXTENSION_METHOD__ if later else \
            __FUSED_ONLY_METHOD__ if fused_only else (__EXTENSION_METHOD__ if extension else __CONDITIONING_METHOD__)
        table[name] = cls
        return cls
    return wrapper


def get_conditioning_method(name: str, operator, noiser, **kwargs):
    cls = None
    for table in _TABLES:
        cls = cls or table.get(name, None)
    if cls is None:
        raise NameError(f"Name {name} is not defined!")
    return cls(operator=operator, noiser=noiser, **kwargs)


class ConditioningMethod(ABC):
    #: True when conditioning() returns the gradient (the loop subtracts it), False when it
    #: returns the already-updated x_t
    returns_gradient = False

    def __init__(self, operator, noiser, **kwargs):
        self.operator = operator
        self.noiser = noiser
        self.l1 = kwargs.get('l1', 0.0)

    def project(self, data, noisy_measurement, **kwargs):
        return self.operator.project(data=data, measurement=noisy_measurement, **kwargs)

    def measurement_norm(self, x_0_hat, measurement, **kwargs):
        """||y - A(x0_hat)||_2 per particle (condition_methods.py:36-39), differentiable through HIP VJPs."""
        Ax = self.operator.forward(x_0_hat, **kwargs)
        return ResidualNormFn.apply(Ax, measurement)

    def grad_and_value(self, x_prev, x_0_hat, measurement, **kwargs):
        if self.noiser.__name__ == 'gaussian':
            norm = self.measurement_norm(x_0_hat, measurement, **kwargs)
            norm_power = norm ** 2 if kwargs.get('norm_exp', 1) == 2 else norm      # :41-47
            norm_grad = torch.autograd.grad(outputs=norm_power.sum(), inputs=x_prev)[0]
        elif self.noiser.__name__ == 'poisson':
            # not on the hot path of any shipped config (:50-55); same formula, A through the HIP operator
            Ax = self.operator.forward(x_0_hat, **kwargs)
            difference = measurement - Ax
            norm = (torch.linalg.norm(difference) / measurement.abs()).mean()
            norm_grad = torch.autograd.grad(outputs=norm, inputs=x_prev)[0]
        else:
            raise NotImplementedError
        return norm_grad, norm

    def fused_spec(self, **kwargs):
        """None, or dict(scale, power) when one step of this method is exactly
        x_{t-1} = sample - grad_{x_prev}[ scale * ||y - A(x0_hat)||^power ]  with a Gaussian noiser."""
        return None

    @abstractmethod
    def conditioning(self, x_t, measurement, noisy_measurement=None, **kwargs):
        pass


@register_conditioning_method(name='vanilla')
class Identity(ConditioningMethod):
    def conditioning(self, x_t, *args, **kwargs):
        return x_t


@register_conditioning_method(name='projection')
class Projection(ConditioningMethod):
    def conditioning(self, x_t, noisy_measurement, **kwargs):
        return self.project(data=x_t, noisy_measurement=noisy_measurement)


@register_conditioning_method(name='mcg')
class ManifoldConstraintGradient(ConditioningMethod):
    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.scale = kwargs.get('scale', 1.0)

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, noisy_measurement, **kwargs):
        norm_grad, norm = self.grad_and_value(x_prev=x_prev, x_0_hat=x_0_hat, measurement=measurement, **kwargs)
        x_t = x_t - norm_grad * self.scale
        x_t = self.project(data=x_t, noisy_measurement=noisy_measurement, **kwargs)
        return x_t, norm


def _drop_loop_kwargs(kwargs):
    """kwargs the loop passes that are not operator.forward arguments"""
    return {k: v for k, v in kwargs.items() if k == 'mask'}


@register_conditioning_method(name='ps')
class PosteriorSampling(ConditioningMethod):
    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.scale = kwargs.get('scale', 0.3)
        self.operator_name = operator.name

    def fused_spec(self, **kwargs):
        if self.noiser.__name__ != 'gaussian':
            return None
        return {"scale": float(self.scale), "power": 2 if kwargs.get('norm_exp', 1) == 2 else 1}

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        norm_exp = kwargs.get('norm_exp', 1)
        norm_grad, norm = self.grad_and_value(x_prev=x_prev, x_0_hat=x_0_hat, measurement=measurement,
                                              norm_exp=norm_exp, **_drop_loop_kwargs(kwargs))
        x_t = x_t - norm_grad * self.scale          # out of place: x_t is an autograd output here
        net_scaling = self.scale / 2 / norm         # condition_methods.py:105
        return x_t, norm.detach(), net_scaling.detach()


@register_conditioning_method(name='ps_semantic')
class PosteriorSamplingSemanticGuid(ConditioningMethod):
    returns_gradient = True

    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.operator_name = operator.name
        self.scale = kwargs.get('scale', 0.3)
        self.sem_guid_scale = kwargs.get('sem_guid_scale', 0.5)
        self.anneal_factor = kwargs.get('anneal_factor', 1.0)
        self.norm_exp = kwargs.get('norm_exp', 1)
        self.guid_images = kwargs.get('guid_images', None)
        # pluggable face-embedding network: embedder(x0_hat[N,3,H,W]) -> [N, D]; the reference hard-wires
        # facenet_pytorch's InceptionResnetV1('vggface2') on cuda:0 (condition_methods.py:126-141)
        self.embedder = kwargs.get('embedder', None)
        self.guid_image_emb = kwargs.get('guid_image_emb', None)
        if self.guid_images is None or self.sem_guid_scale == 0:
            self.n_guid_images = 1
        else:
            self.n_guid_images = len(self.guid_images)
        if self.sem_guid_scale != 0 and self.embedder is None:
            from facenet_pytorch import MTCNN, InceptionResnetV1  # same dependency as the reference
            device = getattr(operator, 'device', 'cuda:0')
            mtcnn = MTCNN(image_size=256, margin=10, min_face_size=20, device=device)
            self.embedder = InceptionResnetV1(pretrained='vggface2', device=device).eval()
            with torch.no_grad():
                cropped = torch.stack(mtcnn(self.guid_images)).to(device)
                self.guid_image_emb = self.embedder(cropped).unsqueeze(0)

    def semantic_scale(self, t):
        """condition_methods.py:155"""
        return self.sem_guid_scale * (1 + (self.anneal_factor - 1) / (1 + math.exp(-10 * (0.3 - t))))

    def fused_spec(self, **kwargs):
        if self.noiser.__name__ != 'gaussian':
            return None
        # the measurement term is first-power whatever norm_exp says (:177-184)
        spec = {"scale": float(self.scale), "power": 1}
        if self.sem_guid_scale != 0:
            # the semantic term depends on x0_hat only: its cotangent on x0_hat joins coef * A^T r in the fused
            # backward launch (dpsx_step_bwd_extra_f32), the embedder and its VJP stay torch
            spec["semantic"] = functools.partial(self.semantic_cotangent, t=kwargs.get('t', 1))
        return spec

    def semantic_cotangent(self, x_0_hat, t=1):
        """-> (d [sem_guid_scale_t * semantic_loss.sum()] / d x0_hat, sem_guid_norm[N])   (:150-175)"""
        x = x_0_hat.detach().requires_grad_()
        with torch.enable_grad():
            emb = self.embedder(x).unsqueeze(1)
            sem_diff = (emb - self.guid_image_emb).reshape(emb.shape[0], -1)
            sem_guid_norm = torch.norm(sem_diff, dim=-1) / self.n_guid_images
            semantic_loss = sem_guid_norm ** 2 if self.norm_exp == 2 else sem_guid_norm
            (g,) = torch.autograd.grad((self.semantic_scale(t) * semantic_loss).sum(), x)
        return g, sem_guid_norm.detach()

    def measurement_semantic_guidance(self, x_prev, x_0_hat, measurement, **kwargs):
        if self.sem_guid_scale == 0:
            sem_guid_norm = torch.tensor(0.0).to(x_0_hat.device)
            sem_guid_scale_t = 0
        else:
            sem_guid_scale_t = self.semantic_scale(kwargs.get('t', 1))
            emb = self.embedder(x_0_hat).unsqueeze(1)
            sem_diff = (emb - self.guid_image_emb).reshape(emb.shape[0], -1)
            sem_guid_norm = torch.norm(sem_diff, dim=-1) / self.n_guid_images
        semantic_loss = sem_guid_norm ** 2 if self.norm_exp == 2 else sem_guid_norm
        if self.noiser.__name__ != 'gaussian':
            raise NotImplementedError
        measurement_guid_norm = self.measurement_norm(x_0_hat, measurement, **_drop_loop_kwargs(kwargs))
        net_loss = self.scale * measurement_guid_norm + sem_guid_scale_t * semantic_loss
        norm_grad = torch.autograd.grad(outputs=net_loss.sum(), inputs=x_prev)[0]
        return norm_grad, measurement_guid_norm.detach(), sem_guid_norm.detach()

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        return self.measurement_semantic_guidance(x_prev=x_prev, x_0_hat=x_0_hat, measurement=measurement, **kwargs)


@register_conditioning_method(name='ps_anneal')
class PosterorSamplingAnnealing(ConditioningMethod):
    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.noise_sigma = max(noiser.sigma, 0.05)
        self.scale = kwargs.get('scale', 0.3)
        self.operator_name = operator.name

    def net_scaling(self, **kwargs):
        beta_scale = kwargs.get('beta_scale', self.scale)
        anneal = kwargs.get('anneal', 1.0)
        return beta_scale / (anneal * self.noise_sigma ** 2)            # condition_methods.py:209

    def fused_spec(self, **kwargs):
        if self.noiser.__name__ != 'gaussian':
            return None
        return {"scale": float(self.net_scaling(**kwargs)), "power": 2}

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        net_scaling = torch.tensor(self.net_scaling(**kwargs)).to(x_t.device)
        grad, norm = self.grad_and_value(x_prev=x_prev, x_0_hat=x_0_hat, measurement=measurement, norm_exp=2,
                                         **_drop_loop_kwargs(kwargs))
        x_t = x_t - net_scaling * grad
        return x_t, norm.detach(), net_scaling


@register_conditioning_method(name='ps+')
class PosteriorSamplingPlus(ConditioningMethod):
    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.num_sampling = kwargs.get('num_sampling', 5)
        self.scale = kwargs.get('scale', 1.0)

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        norm = 0
        for _ in range(self.num_sampling):
            x_0_hat_noise = x_0_hat + 0.05 * torch.rand_like(x_0_hat)
            norm = norm + torch.linalg.norm(measurement - self.operator.forward(x_0_hat_noise)) / self.num_sampling
        norm_grad = torch.autograd.grad(outputs=norm, inputs=x_prev)[0]
        x_t = x_t - norm_grad * self.scale
        return x_t, norm


@register_conditioning_method(name='cg', extension=True)
class ConjugateGradientConsistency(ConditioningMethod):
    """Jacobian-free conditioning (not in the reference; the proximal step of DiffPIR / DDS): per particle, `iters`
    conjugate-gradient iterations on (A^T A + rho I)(x0_hat + d) = A^T y + rho x0_hat from d = 0, then the sampler's own
    step with x0_hat + d in place of x0_hat: x_{t-1} = sample + kappa d.  It needs A and its exact adjoint only: the
    model runs under no_grad.  rho = rho_scale * sigma_n^2 / b^2 with b = sqrt(1 / abar_t - 1) and
    sigma_n = max(noiser.sigma, 0.05) as in ps_anneal.  Linear operators only."""
    returns_gradient = False

    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        if not isinstance(operator, LinearOperator):
            raise NotImplementedError(
                f"cg solves a linear system in A^T A: {getattr(operator, 'name', type(operator).__name__)} is not a linear "
                "operator")
        self.rho_scale = float(kwargs.get('rho_scale', 1.0))
        self.iters = int(kwargs.get('iters', 5))
        if not 0 <= self.iters <= 64:
            raise ValueError(f"cg: iters must be in [0, 64] (got {self.iters})")
        if not (self.rho_scale >= 0 and math.isfinite(self.rho_scale)):
            raise ValueError(f"cg: rho_scale must be finite and not negative (got {self.rho_scale})")
        self.noise_sigma = max(getattr(noiser, 'sigma', 0.0), 0.05)
        self.operator_name = operator.name

    def rho(self, b):
        """the regulariser of the step whose record carries b (float64 on the host; the launch takes it as one fp32)"""
        return self.rho_scale * float(self.noise_sigma) ** 2 / float(b) ** 2

    def conditioning(self, x_t, x_0_hat, measurement, *, coefs=None, **kwargs):
        """x_t: the sampler's unconditioned `sample`; coefs: the step's dpsx_coefs record.  -> (x_{t-1}, dist[N]) in the
        operator handle's persistent buffers (valid until the next call)."""
        if coefs is None:
            raise ValueError("cg.conditioning needs coefs= (the step's dpsx_coefs record): the sampling loop supplies it")
        op, mask = self.operator, kwargs.get('mask', None)
        if op.name == 'inpainting':
            if mask is None:
                raise ValueError("Require mask")
            handle = op.hip_handle_for(mask)
        else:
            handle = op.hip_handle(x_0_hat)
        return handle.cg_step(x_0_hat, x_t, measurement, self.rho(coefs.b), self.iters, coefs)


@register_conditioning_method(name='dsg', extension=True, fused_only=True)
class SphericalGaussianGuidance(ConditioningMethod):
    """Spherical-Gaussian guidance (not in the reference; Yang et al. 2024, "Guidance with Spherical Gaussian Constraint
    for Conditional Diffusion"): the DPS gradient's direction only.  x_{t-1} is put on the sphere of radius ||sigma_t||
    around the model's mean, `guidance_rate` in [0, 1] of the way from the drawn noise direction to the steepest-descent
    direction, so there is no step size to tune and DDIM at 50-100 steps with eta = 1 stays on the shell the model expects.
    The same K1 / K2 / UNet-VJP launches as `ps`; kernels.step_update_dsg runs in K3's place."""
    returns_gradient = False

    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.guidance_rate = float(kwargs.get('guidance_rate', 0.1))
        if not 0.0 <= self.guidance_rate <= 1.0:          # NaN fails both comparisons
            raise ValueError(f"dsg: guidance_rate must be in [0, 1] (got {kwargs.get('guidance_rate')!r})")
        self.operator_name = operator.name

    def fused_spec(self, **kwargs):
        if self.noiser.__name__ != 'gaussian':
            return None
        # only the direction of the gradient is used: unit scale, first power
        return {"scale": 1.0, "power": 1, "dsg": self.guidance_rate}

    def conditioning(self, x_t, measurement, noisy_measurement=None, **kwargs):
        raise NotImplementedError("dsg needs the step's sd and noise, which only the fused step has: it runs inside the "
                                  "sampling loops (kernels.step_update_dsg), not through conditioning()")


@register_conditioning_method(name='pgdm', extension=True, later=True)
class PseudoInverseGuidance(ConditioningMethod):
    """Pseudoinverse guidance (not in the reference; PiGDM, Song, Vahdat, Mardani, Kautz 2023) on the CG solve: the
    measurement's noise-aware, preconditioned residual d = (A^T A + rho_t I)^-1 A^T (y - A x0_hat), rho_t = sigma_y^2 /
    (1 - abar_t), pulled back through the model, x_{t-1} = sample + weight w_t J^T d (include/dpsx.h:
    dpsx_cg_pullback_f32).  No per-operator step size; sigma_y is the noiser's (0 for `clean`, no floor).
    weighting: "score" (w_t = kappa a: consistent with the guided score, first-order accurate in the step count) or "paper"
    (w_t = sqrt(abar_prev) / a: the paper's weights).  Linear operators, `gaussian` and `clean` noisers."""
    returns_gradient = False

    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        if not isinstance(operator, LinearOperator):
            raise NotImplementedError(
                f"pgdm solves a linear system in A^T A: {getattr(operator, 'name', type(operator).__name__)} is not a "
                "linear operator")
        kind = getattr(noiser, '__name__', None)
        if kind not in ('gaussian', 'clean'):
            raise NotImplementedError(f"pgdm is defined for Gaussian measurement noise (noisers `gaussian` and `clean`; got "
                                      f"{kind!r})")
        iters = kwargs.get('iters', 5)
        if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= 64:
            raise ValueError(f"pgdm: iters must be an integer in [0, 64] (got {iters!r})")
        self.iters = iters
        self.weighting = kwargs.get('weighting', 'score')
        if self.weighting not in ('score', 'paper'):
            raise ValueError(f"pgdm: weighting must be 'score' or 'paper' (got {self.weighting!r})")
        weight = kwargs.get('weight', 1.0)
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(weight):
            raise ValueError(f"pgdm: weight must be a finite number (got {weight!r})")
        self.weight = float(weight)
        self.noise_sigma = float(noiser.sigma) if kind == 'gaussian' else 0.0
        if not (self.noise_sigma >= 0 and math.isfinite(self.noise_sigma)):
            raise ValueError(f"pgdm: the noiser's sigma must be finite and not negative (got {noiser.sigma!r})")
        self.operator_name = operator.name

    def conditioning(self, x_t, measurement, noisy_measurement=None, **kwargs):
        raise NotImplementedError("pgdm needs the model's graph (the solve's d is pulled back through the UNet): it runs "
                                  "inside the sampling loops (GaussianDiffusion.pgdm_step), not through conditioning()")
