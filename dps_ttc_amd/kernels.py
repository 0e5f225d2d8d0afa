"""torch-tensor front end of the C ABI (include/dpsx.h) + the autograd glue.

Every function here enqueues hand-written HIP kernels on torch's current
stream; tensors are only the owners of device memory.  Nothing in this module
computes with torch ops.
"""
import contextlib
import ctypes
from ctypes import byref, c_int64, c_void_p

import numpy as np
import os

import torch

from . import _lib
from ._lib import Coefs, RngRec, check, f32c, lib, ptr, require_cuda, stream_of


def make_coefs(a, b, c1, c2, min_log, max_log, add_noise):
    return Coefs(float(a), float(b), float(c1), float(c2), float(min_log), float(max_log), int(bool(add_noise)))


def make_ddim_coefs(a, b, abar, abar_prev, eta, add_noise):
    """struct dpsx_coefs of one DDIM step (reference gaussian_diffusion.py:481-509).  The reference evaluates
    sigma and the two square roots as fp32 tensor arithmetic on .float()-cast table entries, one rounding per
    op; numpy float32 scalars reproduce that bit for bit."""
    one, ab, abp = np.float32(1.0), np.float32(abar), np.float32(abar_prev)
    sigma = np.float32(eta) * np.sqrt((one - abp) / (one - ab)) * np.sqrt(one - ab / abp)
    return Coefs(float(np.float32(a)), float(np.float32(b)), float(np.sqrt(abp)),
                 float(np.sqrt(one - abp - sigma ** 2)), float(sigma), 0.0, 2 | int(bool(add_noise)))


# ------------------------------------------------------------------ counter-based normals
class Rng:
    """struct dpsx_rng: the normals of one step as a pure function of (seed, step, tag, particle id, element) -- see
    include/dpsx.h.  Batch row p has particle id particle_base + (p % per_image if per_image > 0 else p); tag 0 is the step
    noise, tag 1 x_start.  The same distribution as torch.randn, not the same stream."""

    TAG_STEP, TAG_X_START = 0, 1

    def __init__(self, seed, step, tag=0, particle_base=0, per_image=0):
        self.seed, self.step, self.tag = int(seed), int(step), int(tag)
        self.particle_base, self.per_image = int(particle_base), int(per_image)
        if not 0 <= self.seed < 1 << 64 or not 0 <= self.step < 1 << 32 or not 0 <= self.tag < 1 << 32:
            raise ValueError("Rng: seed must fit 64 bits, step and tag 32 bits")
        if self.particle_base < 0 or self.per_image < 0:
            raise ValueError("Rng: particle_base and per_image must not be negative")

    def offset(self, rows):
        """the record of the batch rows [rows, ...) of this one (a particle group's slice; with per_image set the slice
        starts at an image boundary, so the id of a row stays particle_base + p % per_image)"""
        if self.per_image > 0:
            if rows % self.per_image:
                raise ValueError("a slice of a multi-image batch must start at an image boundary")
            return self
        return Rng(self.seed, self.step, self.tag, self.particle_base + int(rows), 0)

    def rec(self):
        return RngRec(self.seed, self.step, self.tag, self.particle_base, self.per_image)

    def __repr__(self):
        return (f"Rng(seed={self.seed}, step={self.step}, tag={self.tag}, particle_base={self.particle_base}, "
                f"per_image={self.per_image})")


def randn(shape, rng, device, want_bits=False, out=None):
    """[N, ...] fp32 normals of `rng` on `device`, one launch (dpsx_randn_f32).  want_bits: also the Philox words,
    uint32 as an int32 tensor [N, 4 * ceil(chw / 4)].  out: fill this contiguous tensor instead of a new one."""
    shape = tuple(int(v) for v in shape)
    if out is None:
        _cuda_device(device)
        out = torch.empty(shape, dtype=torch.float32, device=device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous fp32 tensor of the requested shape")
    require_cuda(out, "randn output")
    n = shape[0] if shape else 1
    chw = out.numel() // n if n else 0
    bits = torch.empty((n, 4 * ((chw + 3) // 4)), dtype=torch.int32, device=out.device) if want_bits else None
    check(lib().dpsx_randn_f32(ptr(out), ptr(bits), n, chw, byref(rng.rec()), stream_of(out)), "dpsx_randn_f32")
    return (out, bits) if want_bits else out


def _noise_or_rng(noise, rng):
    if (noise is None) == (rng is None):
        raise ValueError("give exactly one of noise= and rng=")


# ------------------------------------------------------------------ S1
def posterior_fwd(x_t, model_out, noise=None, coefs=None, want_inside=False, want_x0=True, rng=None):
    """p_mean_variance + DDPM.p_sample (gaussian_diffusion.py:308-330, 466-476) -> (x0_hat, sample[, inside]).
    want_x0=False skips the x0_hat store (search_ddpm only consumes the sample): x0_hat is then None.
    rng= (instead of noise=): the noise is drawn inside the launch."""
    if coefs is None:
        raise ValueError("coefs is required")
    if rng is not None and noise is not None:
        raise ValueError("give exactly one of noise= and rng=")
    x_t, model_out = f32c(x_t, "x_t"), f32c(model_out, "model_out")
    noise = None if noise is None else f32c(noise, "noise")
    n, chw = x_t.shape[0], x_t[0].numel() if x_t.shape[0] else 0
    if model_out.shape[0] != n or (n and model_out[0].numel() != 2 * chw):
        raise ValueError(f"model_out {tuple(model_out.shape)} does not hold 2x the channels of x {tuple(x_t.shape)}")
    x0, sample = (torch.empty_like(x_t) if want_x0 else None), torch.empty_like(x_t)
    inside = torch.empty(x_t.shape, dtype=torch.uint8, device=x_t.device) if want_inside else None
    tail = (ptr(x0), ptr(sample), ptr(inside), n, chw, byref(coefs), stream_of(x_t))
    if rng is not None:
        check(lib().dpsx_posterior_fwd_rng_f32(ptr(x_t), ptr(model_out), byref(rng.rec()), *tail), "dpsx_posterior_fwd_rng_f32")
    else:
        check(lib().dpsx_posterior_fwd_f32(ptr(x_t), ptr(model_out), ptr(noise), *tail), "dpsx_posterior_fwd_f32")
    return (x0, sample, inside) if want_inside else (x0, sample)


def posterior_bwd(g_x0, g_sample, x_t, model_out, noise, coefs):
    x_t, model_out = f32c(x_t), f32c(model_out)
    g_x0 = None if g_x0 is None else f32c(g_x0)
    g_sample = None if g_sample is None else f32c(g_sample)
    noise = None if noise is None else f32c(noise)
    n, chw = x_t.shape[0], x_t[0].numel() if x_t.shape[0] else 0
    g_x, g_mo = torch.empty_like(x_t), torch.empty_like(model_out)
    check(lib().dpsx_posterior_bwd_f32(ptr(g_x0), ptr(g_sample), ptr(x_t), ptr(model_out), ptr(noise), ptr(g_x),
                                       ptr(g_mo), n, chw, byref(coefs), stream_of(x_t)), "dpsx_posterior_bwd_f32")
    return g_x, g_mo


class PosteriorStepFn(torch.autograd.Function):
    """(x_t, model_out) -> (x0_hat, sample) with the HIP VJP, so torch.autograd only sees UNet -> [HIP tail]."""

    @staticmethod
    def forward(ctx, x_t, model_out, noise, coefs):
        x0, sample = posterior_fwd(x_t, model_out, noise, coefs)
        ctx.save_for_backward(x_t, model_out, noise if noise is not None else x_t.new_empty(0))
        ctx.coefs = coefs
        return x0, sample

    @staticmethod
    def backward(ctx, g_x0, g_sample):
        x_t, model_out, noise = ctx.saved_tensors
        g_x, g_mo = posterior_bwd(g_x0, g_sample, x_t, model_out, noise if noise.numel() else None, ctx.coefs)
        return g_x, g_mo, None, None


# ------------------------------------------------------------------ operator handles
class OpHandle:
    """Owns one dpsx_op (constant tables on the device) and its scratch workspace."""

    def __init__(self, handle, device, keep=()):
        self._h = handle
        self.device = device
        self._keep = keep          # tensors the op borrows (mask)
        self._ws = None
        self._cg = None            # CgBuffers of the last cg_step shape
        self.kind = lib().dpsx_op_kind(self._h)

    @classmethod
    def blur(cls, kernel2d, device, force_taps=False):
        k = np.ascontiguousarray(np.asarray(kernel2d, dtype=np.float32))
        if k.ndim != 2 or k.shape[0] != k.shape[1]:
            raise ValueError("blur kernel must be square")
        _cuda_device(device)
        h = c_void_p()
        check(lib().dpsx_op_create_blur(k.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), k.shape[0],
                                        _lib.BLUR_FORCE_TAPS if force_taps else _lib.BLUR_AUTO, byref(h)),
              "dpsx_op_create_blur")
        return cls(h, device)

    @classmethod
    def resize(cls, in_h, in_w, w_h, i_h, w_w, i_w, device):
        w_h = np.ascontiguousarray(w_h, dtype=np.float32)
        w_w = np.ascontiguousarray(w_w, dtype=np.float32)
        i_h = np.ascontiguousarray(i_h, dtype=np.int64)
        i_w = np.ascontiguousarray(i_w, dtype=np.int64)
        _cuda_device(device)
        h = c_void_p()
        fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64)
        check(lib().dpsx_op_create_resize(in_h, in_w, w_h.ctypes.data_as(fp), i_h.ctypes.data_as(ip),
                                          w_h.shape[0], w_h.shape[1], w_w.ctypes.data_as(fp),
                                          i_w.ctypes.data_as(ip), w_w.shape[0], w_w.shape[1], byref(h)),
              "dpsx_op_create_resize")
        return cls(h, device)

    @classmethod
    def mask(cls, mask, device):
        """mask [1,1,H,W] (broadcast over the particles) or [M,1,H,W], one per image of a multi-image batch: particle p
        of N uses mask p / (N / M)"""
        m = f32c(mask.to(device), "mask")
        hh, ww = m.shape[-2:]
        mask_n = m.shape[0] if m.dim() == 4 else 1
        if m.numel() != mask_n * hh * ww:
            raise ValueError("mask must be [1,1,H,W] or [M,1,H,W]")
        h = c_void_p()
        if mask_n == 1:
            check(lib().dpsx_op_create_mask(ptr(m), hh, ww, byref(h)), "dpsx_op_create_mask")
        else:
            check(lib().dpsx_op_create_mask_n(ptr(m), mask_n, hh, ww, byref(h)), "dpsx_op_create_mask_n")
        obj = cls(h, device, keep=(m,))
        obj.mask_n = mask_n
        return obj

    @classmethod
    def identity(cls, device):
        _cuda_device(device)
        h = c_void_p()
        check(lib().dpsx_op_create_identity(byref(h)), "dpsx_op_create_identity")
        return cls(h, device)

    @classmethod
    def phase(cls, side, pad, max_planes, device):
        _cuda_device(device)
        h = c_void_p()
        check(lib().dpsx_op_create_phase(side, pad, max_planes, byref(h)), "dpsx_op_create_phase")
        obj = cls(h, device)
        # the hand-written spectral step (256 + 2 x 64 = 384 points) consumes x0_hat inside its first pass
        obj.spectral = (side, pad) == (256, 64) and "DPSX_PHASE_LIBRARY_FFT" not in os.environ
        return obj

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        try:
            if h and _lib._lib is not None:
                _lib._lib.dpsx_op_destroy(h)
        except (AttributeError, TypeError):     # interpreter shutdown: module globals are already gone
            pass

    # -- geometry / scratch
    def fuses_step(self, c, h, w):
        """whether step_fwd / step_bwd take this handle at [N, c, h, w] (mirror of mask_fused_ok in csrc/api.hip for buffers
        torch allocated): the inpainting step exists in its float4 form only, H * W a multiple of 4; every other operator
        has a scalar form.  Where this is False the launches return DPSX_EUNSUPPORTED and the loops take the per-op path
        (GaussianDiffusion._fusion_plan asks before the first step)."""
        return self.kind != _lib.KIND_MASK or self._mask_fuses(h, w)

    @staticmethod
    def _mask_fuses(h, w):
        """fuses_step's shape test for an inpainting handle, askable before there is a handle (or a device)"""
        return (int(h) * int(w)) % 4 == 0

    def draws_in_kernel(self, c, h, w):
        """whether step_fwd(rng=) draws the noise inside this handle's K1 at [N, c, h, w] (dpsx_step_draws_in_kernel, for
        buffers torch allocated): both blur kernels on whole 64 x 64 tiles, the row-streaming resize kernel, inpainting
        in its float4 form, the identity.
        Elsewhere that call declines and step_fwd fills a persistent noise buffer with `randn` and runs the pointer
        launch -- the same bits."""
        return bool(lib().dpsx_step_draws_in_kernel(self._h, int(c), int(h), int(w)))

    def out_hw(self, h, w):
        oh, ow = c_int64(), c_int64()
        check(lib().dpsx_op_out_shape(self._h, h, w, byref(oh), byref(ow)), "dpsx_op_out_shape")
        return oh.value, ow.value

    def workspace(self, n, c, h, w, device):
        need = lib().dpsx_op_workspace_bytes(self._h, n, c, h, w)
        if need < 0:
            check(int(need), "dpsx_op_workspace_bytes")
        if self._ws is None or self._ws.numel() < need or self._ws.device != device:
            self._ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=device)
        return self._ws

    # -- A and A^T
    def forward(self, x):
        x = _nchw(f32c(x, "operator input"))
        n, c, h, w = x.shape
        oh, ow = self.out_hw(h, w)
        y = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
        ws = self.workspace(n, c, h, w, x.device)
        check(lib().dpsx_op_forward_f32(self._h, ptr(x), ptr(y), n, c, h, w, ptr(ws), ws.numel(), stream_of(x)),
              "dpsx_op_forward_f32")
        return y

    def adjoint(self, u, x=None, in_hw=None):
        u = _nchw(f32c(u, "cotangent"))
        n, c = u.shape[:2]
        h, w = in_hw if in_hw is not None else x.shape[-2:]
        x = None if x is None else f32c(x)
        g = torch.empty((n, c, h, w), dtype=torch.float32, device=u.device)
        ws = self.workspace(n, c, h, w, u.device)
        check(lib().dpsx_op_adjoint_f32(self._h, ptr(u), ptr(x), ptr(g), n, c, h, w, ptr(ws), ws.numel(),
                                        stream_of(u)), "dpsx_op_adjoint_f32")
        return g

    def score(self, x, y):
        """costs[p] = ||y - A(x_p)||_2 (gaussian_diffusion.py:626-630) without materialising A x."""
        x, y = _nchw(f32c(x)), f32c(y)
        n, c, h, w = x.shape
        costs = torch.empty(n, dtype=torch.float32, device=x.device)
        ws = self.workspace(n, c, h, w, x.device)
        check(lib().dpsx_score_f32(self._h, ptr(x), ptr(y), y.shape[0], ptr(costs), n, c, h, w, ptr(ws),
                                   ws.numel(), stream_of(x)), "dpsx_score_f32")
        return costs

    def score_argmin(self, x, y):
        """-> (costs [N], best int64 scalar, costs[best] [1]): scoring launch + one small launch that finishes the
        per-particle norms and the torch.argmin-order select (gaussian_diffusion.py:626-632); all on the device."""
        x, y = _nchw(f32c(x)), f32c(y)
        n, c, h, w = x.shape
        if n == 0:
            raise ValueError("best-of-N over an empty particle set")
        costs = torch.empty(n, dtype=torch.float32, device=x.device)
        best = torch.empty((), dtype=torch.int64, device=x.device)
        val = torch.empty(1, dtype=torch.float32, device=x.device)
        ws = self.workspace(n, c, h, w, x.device)
        check(lib().dpsx_score_argmin_f32(self._h, ptr(x), ptr(y), y.shape[0], ptr(costs), ptr(best), ptr(val),
                                          n, c, h, w, ptr(ws), ws.numel(), stream_of(x)), "dpsx_score_argmin_f32")
        return costs, best, val

    def _search(self, x, model_out, noise, rng, y, coefs, n, n_out, segments, one):
        """The library call of search_step / search_step_one: x [N or states, C, H, W] and model_out as checked by them,
        n proposals, x_next / winner of n_out rows (0: not wanted) -> (x_next or None, sample, costs, best, costs[best]).
        The entry point follows from the arguments: _one for one state per image, _seg with segments= (and for every
        rng= call: the in-launch draw exists in the segmented forms only, one segment being the whole set)."""
        c, h, w = x.shape[1:]
        dev = x.device
        seg = 1 if segments is None else int(segments)
        sample = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
        x_next = torch.empty((n_out, c, h, w), dtype=torch.float32, device=dev) if n_out else None
        costs = torch.empty(n, dtype=torch.float32, device=dev)
        best = torch.empty(seg if segments is not None else (), dtype=torch.int64, device=dev)
        val = torch.empty(seg, dtype=torch.float32, device=dev)
        ws = self.workspace(n, c, h, w, dev)
        segmented = segments is not None or rng is not None
        name = f"dpsx_search_step{'_one' if one else ''}{'_seg' if segmented else ''}{'_rng' if rng is not None else ''}_f32"
        check(getattr(lib(), name)(self._h, ptr(x), ptr(model_out), ptr(noise) if rng is None else byref(rng.rec()), ptr(y),
                                   y.shape[0], ptr(sample), ptr(costs), ptr(best), ptr(val), ptr(x_next),
                                   *((seg,) if segmented else ()), n, c, h, w, byref(coefs), ptr(ws), ws.numel(),
                                   stream_of(x)), name)
        return x_next, sample, costs, best, val

    def search_step(self, x_t, model_out, noise=None, y=None, coefs=None, replicate=True, segments=None, rng=None):
        """One search_ddpm step (gaussian_diffusion.py:618-633): S1, costs of the proposals, select and -- with
        replicate=True -- the winner copied over all particles.  -> (x_next or None, sample, costs, best, costs[best]);
        one library call, nothing leaves the device.
        segments=M: a multi-image batch of M images x N / M particles (image-major), y [1 or M, ...]: the select runs per
        image, best / costs[best] are [M] (global particle indices) and each image's winner is replicated over its own
        particles.
        rng= (instead of noise=): S1 draws the noise inside its launch."""
        _noise_or_rng(noise, rng)
        x_t, model_out, y = _nchw(f32c(x_t, "x_t")), f32c(model_out, "model_out"), f32c(y, "measurement")
        noise = None if noise is None else f32c(noise, "noise")
        n, c, h, w = x_t.shape
        if n == 0:
            raise ValueError("best-of-N over an empty particle set")
        if model_out.shape[0] != n or model_out[0].numel() != 2 * c * h * w:
            raise ValueError(f"model_out {tuple(model_out.shape)} does not hold 2x the channels of x {tuple(x_t.shape)}")
        return self._search(x_t, model_out, noise, rng, y, coefs, n, n if replicate else 0, segments, one=False)

    def search_step_one(self, x_one, model_out_one, noise=None, y=None, coefs=None, want_winner=True, segments=None,
                        rng=None, n=None):
        """The same step from ONE state particle (after a select all particles are copies of the winner): x_one
        [1,C,H,W], model_out_one [1,2C,H,W], noise [N,C,H,W] -> (winner [1,C,H,W] or None, sample [N,...], costs,
        best, costs[best]).  Bit-identical to search_step on N copies of the state; one model evaluation per step.
        segments=M: M images, one state each (x_one [M,C,H,W], model_out_one [M,2C,H,W]); proposal p reads state p / (N / M),
        the select runs per image and winner / best / costs[best] are [M, ...] (best: global particle indices).
        rng= with n= (instead of noise=): the N proposals' noise is drawn inside S1's launch."""
        _noise_or_rng(noise, rng)
        x_one, model_out_one, y = _nchw(f32c(x_one, "x_t")), f32c(model_out_one, "model_out"), f32c(y, "measurement")
        states = 1 if segments is None else int(segments)
        if rng is not None:
            if n is None:
                raise ValueError("search_step_one(rng=) needs n=, the number of proposals")
            n, (c, h, w) = int(n), x_one.shape[1:]
            what, whole = f"{n} proposals", states > 0 and n % states == 0
        else:
            noise = _nchw(f32c(noise, "noise"))
            n, c, h, w = noise.shape
            what, whole = f"noise {tuple(noise.shape)}", True      # the library refuses n % states != 0
        if n < 1:
            raise ValueError("best-of-N over an empty particle set")
        if x_one.shape != (states, c, h, w) or model_out_one.shape[0] != states or \
                model_out_one[0].numel() != 2 * c * h * w or not whole:
            raise ValueError(f"{states} state particle(s) expected: x {tuple(x_one.shape)}, "
                             f"model_out {tuple(model_out_one.shape)}, {what}")
        return self._search(x_one, model_out_one, noise, rng, y, coefs, n, states if want_winner else 0, segments, one=True)

    def search_step_beam(self, x_states, model_out_states, noise=None, y=None, coefs=None, *, n, beam, segments=None,
                         rng=None, want_winners=True):
        """The beam step (include/dpsx.h: dpsx_search_step_beam_f32): x_states [S, C, H, W] and model_out_states
        [S, 2C, H, W] feed n proposals, n / S consecutive ones per state; every image (segments=M, default 1; M divides S)
        keeps its `beam` best proposals under the select's order -> (winners [M * beam, C, H, W] or None, sample [n, ...],
        costs [n], best [M * beam] global particle indices, rank-major inside an image, costs[best]).
        S == n is a loop's first step, S == M * beam every later one; noise= [n, C, H, W] or rng=."""
        _noise_or_rng(noise, rng)
        x, mo, y = _nchw(f32c(x_states, "x_t")), f32c(model_out_states, "model_out"), f32c(y, "measurement")
        noise = None if noise is None else _nchw(f32c(noise, "noise"))
        n, beam, seg = int(n), int(beam), 1 if segments is None else int(segments)
        states, (c, h, w) = x.shape[0], x.shape[1:]
        if n < 1:
            raise ValueError("beam search over an empty particle set")
        if seg < 1 or states < 1 or n % states or states % seg or mo.shape[0] != states or \
                mo[0].numel() != 2 * c * h * w or (noise is not None and noise.shape != (n, c, h, w)):
            raise ValueError(f"{n} proposals from {states} state(s) of {seg} image(s) expected: x {tuple(x.shape)}, "
                             f"model_out {tuple(mo.shape)}" + ("" if noise is None else f", noise {tuple(noise.shape)}"))
        if not 1 <= beam <= n // seg:
            raise ValueError(f"beam = {beam} does not lie in [1, {n // seg}], the proposals per image")
        dev = x.device
        sample = torch.empty((n, c, h, w), dtype=torch.float32, device=dev)
        winners = torch.empty((seg * beam, c, h, w), dtype=torch.float32, device=dev) if want_winners else None
        costs = torch.empty(n, dtype=torch.float32, device=dev)
        best = torch.empty(seg * beam, dtype=torch.int64, device=dev)
        val = torch.empty(seg * beam, dtype=torch.float32, device=dev)
        ws = self.workspace(n, c, h, w, dev)
        check(lib().dpsx_search_step_beam_f32(self._h, ptr(x), ptr(mo), ptr(noise), None if rng is None else byref(rng.rec()),
                                              ptr(y), y.shape[0], ptr(sample), ptr(costs), ptr(best), ptr(val), ptr(winners),
                                              seg, states, beam, n, c, h, w, byref(coefs), ptr(ws), ws.numel(), stream_of(x)),
              "dpsx_search_step_beam_f32")
        return winners, sample, costs, best, val

    def cg_step(self, x0_hat, sample, y, rho, iters, coefs, want_d=False):
        """The CG data-consistency step (include/dpsx.h: dpsx_cg_step_f32): `iters` conjugate-gradient iterations per
        particle on (A^T A + rho I)(x0_hat + d) = A^T y + rho x0_hat from d = 0, then x_next = sample + kappa d with the
        slope kappa of the sampler's step in x0_hat (cg_kappa).  -> (x_next [N, C, H, W], dist [N] = ||y - A x0_hat||_2
        [, d]).  One chain of launches on the current stream, no host read.  The results live in this handle's persistent
        CgBuffers (x_next alternates between two buffers; dist and d are overwritten by the next call): callers clone
        what they keep."""
        x0_hat, sample, y = _nchw(f32c(x0_hat, "x0_hat")), _nchw(f32c(sample, "sample")), f32c(y, "measurement")
        if sample.shape != x0_hat.shape:
            raise ValueError(f"sample {tuple(sample.shape)} and x0_hat {tuple(x0_hat.shape)} differ in shape")
        n, c, h, w = x0_hat.shape
        buf = self.cg_buffers(n, c, h, w, x0_hat.device)
        out = buf.x_next[buf.flip]
        buf.flip ^= 1
        d = buf.d_buffer() if want_d else None
        check(lib().dpsx_cg_step_f32(self._h, ptr(x0_hat), ptr(sample), ptr(y), y.shape[0], float(rho), int(iters),
                                     byref(coefs), ptr(out), ptr(buf.dist), ptr(d), n, c, h, w, ptr(buf.ws),
                                     buf.ws.numel(), stream_of(x0_hat)), "dpsx_cg_step_f32")
        return (out, buf.dist, d) if want_d else (out, buf.dist)

    def cg_buffers(self, n, c, h, w, device):
        """this handle's CgBuffers for (N, C, H, W) on `device` (one set: another shape replaces it)"""
        buf = self._cg
        if buf is None or buf.shape != (n, c, h, w) or buf.dist.device != torch.device(device):
            buf = self._cg = CgBuffers(self, n, c, h, w, device)
        return buf

    def cg_pullback(self, x0_hat, inside, y, rho, iters, gain, want_d=False):
        """Pseudoinverse guidance's cotangent (include/dpsx.h: dpsx_cg_pullback_f32): cg_step's solve for d, ended in
        g_model_out[:, :C] = inside ? gain d : +0 in place of x_next = sample + kappa d.  inside: S1's clamp gate
        (posterior_fwd(..., want_inside=True)); rho, gain: the step's host scalars (pgdm_scalars).
        -> (g_model_out [N, 2C, H, W] with a zero variance half, dist [N] = ||y - A x0_hat||_2 [, d]) in this handle's
        persistent CgBuffers (overwritten by the next call): callers clone what they keep."""
        x0_hat, y = _nchw(f32c(x0_hat, "x0_hat")), f32c(y, "measurement")
        require_cuda(inside, "clamp gate")
        if inside.dtype != torch.uint8 or inside.numel() != x0_hat.numel() or not inside.is_contiguous():
            raise ValueError(f"the clamp gate must be a contiguous uint8 tensor of x0_hat's size (got {inside.dtype}, "
                             f"{tuple(inside.shape)})")
        n, c, h, w = x0_hat.shape
        buf = self.cg_buffers(n, c, h, w, x0_hat.device)
        g = buf.g_model_out_buffer()
        d = buf.d_buffer() if want_d else None
        check(lib().dpsx_cg_pullback_f32(self._h, ptr(x0_hat), ptr(inside), ptr(y), y.shape[0], float(rho), int(iters),
                                         float(gain), ptr(g), ptr(buf.dist), ptr(d), n, c, h, w, ptr(buf.ws),
                                         buf.ws.numel(), stream_of(x0_hat)), "dpsx_cg_pullback_f32")
        return (g, buf.dist, d) if want_d else (g, buf.dist)

    def resample_cost(self, x, y, prev_costs=None, potential_type='min'):
        """SearchDDPM.resample_update's cost update (gaussian_diffusion.py:556-585) in one launch:
        curr[p] = ||y - A(x_p)||_1^2 / (C H W), net = combine(curr, prev_costs) -> (curr, net)."""
        if potential_type not in _lib.POTENTIALS:
            raise NotImplementedError(potential_type)
        x, y = _nchw(f32c(x)), f32c(y)
        n, c, h, w = x.shape
        prev = None if prev_costs is None else f32c(prev_costs.reshape(-1), "prev_costs")
        if prev is not None and prev.numel() != n:
            raise ValueError("prev_costs must hold one cost per particle")
        curr = torch.empty(n, dtype=torch.float32, device=x.device)
        net = torch.empty(n, dtype=torch.float32, device=x.device)
        ws = self.workspace(n, c, h, w, x.device)
        check(lib().dpsx_resample_cost_f32(self._h, ptr(x), ptr(y), y.shape[0], ptr(prev),
                                           _lib.POTENTIALS[potential_type], ptr(curr), ptr(net), n, c, h, w,
                                           ptr(ws), ws.numel(), stream_of(x)), "dpsx_resample_cost_f32")
        return curr, net


def _cuda_device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"dps_ttc_amd operators need an MI355X device, got {dev} (no CPU fallback by design)")
    torch.cuda.set_device(dev)
    torch.cuda.current_stream(dev)   # make sure the HIP context exists before libdpsx allocates


def _nchw(t):
    if t.dim() != 4:
        raise ValueError(f"expected an [N,C,H,W] tensor, got {tuple(t.shape)}")
    return t


class OperatorFn(torch.autograd.Function):
    """operator.forward with its exact HIP adjoint as the VJP."""

    @staticmethod
    def forward(ctx, x, handle):
        ctx.handle = handle
        ctx.in_hw = tuple(x.shape[-2:])
        if handle.kind == _lib.KIND_PHASE:
            ctx.save_for_backward(x)
        return handle.forward(x)

    @staticmethod
    def backward(ctx, u):
        x = ctx.saved_tensors[0] if ctx.handle.kind == _lib.KIND_PHASE else None
        return ctx.handle.adjoint(u, x=x, in_hw=ctx.in_hw), None


# ------------------------------------------------------------------ residual norm
def residual_norm(y, ax, want_residual=True):
    y, ax = f32c(y, "measurement"), f32c(ax, "A x")
    n = ax.shape[0]
    m = ax[0].numel() if n else 0
    y_n = y.shape[0]
    if (y_n not in (1, n) and (y_n < 1 or n % y_n)) or (n and y[0].numel() != m):
        raise ValueError(f"measurement {tuple(y.shape)} does not broadcast against {tuple(ax.shape)}")
    r = torch.empty_like(ax) if want_residual else None
    norm = torch.empty(n, dtype=torch.float32, device=ax.device)
    ws = torch.empty(max(n * 256, 1), dtype=torch.float32, device=ax.device)
    check(lib().dpsx_residual_norm_f32(ptr(y), y_n, ptr(ax), ptr(r), ptr(norm), n, m, ptr(ws), ws.numel() * 4,
                                       stream_of(ax)), "dpsx_residual_norm_f32")
    return r, norm


def norm_bwd(r, norm, g_norm, power=1):
    r, norm, g_norm = f32c(r), f32c(norm), f32c(g_norm)
    n = r.shape[0]
    g = torch.empty_like(r)
    check(lib().dpsx_norm_bwd_f32(ptr(r), ptr(norm), ptr(g_norm), power, ptr(g), n, r[0].numel() if n else 0,
                                  stream_of(r)), "dpsx_norm_bwd_f32")
    return g


class ResidualNormFn(torch.autograd.Function):
    """norm[p] = ||y - ax_p||_2 per particle  (condition_methods.py:37-39); VJP w.r.t. ax only."""

    @staticmethod
    def forward(ctx, ax, y):
        r, norm = residual_norm(y, ax)
        ctx.save_for_backward(r, norm)
        return norm

    @staticmethod
    def backward(ctx, g_norm):
        r, norm = ctx.saved_tensors
        return norm_bwd(r, norm, g_norm, 1), None


# ------------------------------------------------------------------ update / select
def update(sample, g_a, g_b=None):
    sample, g_a = f32c(sample), f32c(g_a)
    g_b = None if g_b is None else f32c(g_b)
    out = torch.empty_like(sample)
    check(lib().dpsx_update_f32(ptr(sample), ptr(g_a), ptr(g_b), ptr(out), sample.numel(), stream_of(sample)),
          "dpsx_update_f32")
    return out


def argmin(v, want_value=False):
    """torch.argmin semantics on the device, result stays on the device (int64 scalar tensor).
    want_value: also return v[argmin] as a [1] fp32 device tensor (no host index, no sync)."""
    v = f32c(v.reshape(-1), "scores")
    if v.numel() == 0:
        raise ValueError("argmin of an empty score vector")
    out = torch.empty((), dtype=torch.int64, device=v.device)
    val = torch.empty(1, dtype=torch.float32, device=v.device) if want_value else None
    check(lib().dpsx_argmin_f32(ptr(v), v.numel(), ptr(out), ptr(val), stream_of(v)), "dpsx_argmin_f32")
    return (out, val) if want_value else out


def argmin_seg(v, segments, want_value=False):
    """v [segments * K] (or [segments, K]) -> [segments] int64 global indices m * K + argmin(v[m]) (torch.argmin order
    within each segment: first minimum, NaN counts as the minimum), on the device in one launch -- the per-image best-of-N
    of a multi-image batch.  want_value: also the [segments] minima."""
    v = f32c(v.reshape(-1), "scores")
    segments = int(segments)
    if segments < 1 or v.numel() == 0 or v.numel() % segments:
        raise ValueError(f"{v.numel()} scores do not split into {segments} non-empty segments")
    out = torch.empty(segments, dtype=torch.int64, device=v.device)
    val = torch.empty(segments, dtype=torch.float32, device=v.device) if want_value else None
    check(lib().dpsx_argmin_seg_f32(ptr(v), segments, v.numel() // segments, ptr(out), ptr(val), stream_of(v)),
          "dpsx_argmin_seg_f32")
    return (out, val) if want_value else out


def topk_seg(v, segments, b, want_value=False):
    """v [segments * K] (or [segments, K]) -> [segments * b] int64 global indices: the first b entries of every segment
    under argmin_seg's order (NaN first, then the lower value, ties by the lower index), in that order; b = 1 is argmin_seg.
    On the device in one launch.  want_value: also the [segments * b] values."""
    v = f32c(v.reshape(-1), "scores")
    segments, b = int(segments), int(b)
    if segments < 1 or v.numel() == 0 or v.numel() % segments:
        raise ValueError(f"{v.numel()} scores do not split into {segments} non-empty segments")
    out = torch.empty(segments * max(b, 0), dtype=torch.int64, device=v.device)
    val = torch.empty(segments * max(b, 0), dtype=torch.float32, device=v.device) if want_value else None
    check(lib().dpsx_topk_seg_f32(ptr(v), segments, v.numel() // segments, b, ptr(out), ptr(val), stream_of(v)),
          "dpsx_topk_seg_f32")
    return (out, val) if want_value else out


def gather(src, ids, validate=True):
    """src[ids] for an [N, ...] fp32 tensor and int64 ids (gaussian_diffusion.py:697).  validate=True (the default for
    ids that arrive through the public API) adds torch's IndexError check -- two host reads; the package's own loops pass
    validate=False for ids they drew themselves (torch.multinomial over [0, N)): no host sync, and the kernel never reads
    out of bounds anyway (a bad id yields a NaN particle)."""
    src = f32c(src)
    ids = ids.to(device=src.device, dtype=torch.int64).contiguous()
    if validate and ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= src.shape[0]):
        raise IndexError("gather index out of range")
    dst = torch.empty((ids.numel(),) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    chw = src[0].numel() if src.shape[0] else 0
    check(lib().dpsx_gather_f32(ptr(src), ptr(ids), ptr(dst), ids.numel(), src.shape[0], chw, stream_of(src)),
          "dpsx_gather_f32")
    return dst


def replicate(src, idx_dev, n_out=None):
    """img[best.repeat(n)] (gaussian_diffusion.py:633): idx stays on the device, no host sync."""
    src = f32c(src)
    n_out = src.shape[0] if n_out is None else n_out
    idx_dev = idx_dev.to(device=src.device, dtype=torch.int64).reshape(1).contiguous()
    dst = torch.empty((n_out,) + tuple(src.shape[1:]), dtype=torch.float32, device=src.device)
    chw = src[0].numel() if src.shape[0] else 0
    check(lib().dpsx_replicate_f32(ptr(src), ptr(idx_dev), ptr(dst), n_out, src.shape[0], chw, stream_of(src)),
          "dpsx_replicate_f32")
    return dst


def _resample_args(d, u, segments):
    d = f32c(d if d.dim() == 1 else d.reshape(-1), "distances")
    u = f32c(u if u.dim() == 1 else u.reshape(-1), "uniforms")
    segments = int(segments)
    n = d.numel()
    if segments < 1 or n == 0 or n % segments:
        raise ValueError(f"{n} distances do not split into {segments} non-empty segments")
    if u.numel() != n:
        raise ValueError(f"the draw takes one uniform per particle ({u.numel()} for {n})")
    if u.device != d.device:
        raise ValueError("distances and uniforms live on different devices")
    return d, u, segments, n


RESAMPLE_SCHEMES = {"multinomial": 0, "stratified": 1, "systematic": 2}     # DPSX_RESAMPLE_* of include/dpsx.h


def resample_scheme_args(scheme, ess):
    """(scheme id, ess_q16) of include/dpsx.h "resampling schemes and the ESS trigger": ess is tau in [0, 1] (None: 1.0,
    every segment whose weights are not all equal resamples) -> tau * 65536 rounded to nearest"""
    if scheme not in RESAMPLE_SCHEMES:
        raise ValueError(f"resample scheme must be one of {sorted(RESAMPLE_SCHEMES)} (got {scheme!r})")
    tau = 1.0 if ess is None else float(ess)
    if not 0.0 <= tau <= 1.0:                                       # NaN fails both comparisons
        raise ValueError(f"the ESS threshold is a fraction of the particle count in [0, 1] (got {ess!r})")
    return RESAMPLE_SCHEMES[scheme], int(tau * 65536.0 + 0.5)


_RESAMPLE_SYMBOLS = (("dpsx_resample_draw_seg_ex_f32", "dpsx_resample_draw_seg_f32"),       # [fused][plain]
                     ("dpsx_resample_seg_ex_f32", "dpsx_resample_seg_f32"))


def _resample(src, d, u, segments, inv_scale, want_weights, scheme, ess, want_flags):
    """The front end of resample_draw (src None) and resample (src contiguous fp32): argument checks, allocation, ONE
    launch and the result tuple ([src[ids], d[ids],] ids[, q][, flags, ess]).  The defaults take the plain entry point,
    anything else the scheme / ESS one."""
    fused = src is not None
    d, u, segments, n = _resample_args(d, u, segments)
    if fused:
        if src.dim() < 1 or src.shape[0] != n or src.device != d.device:
            raise ValueError(f"{n} distances for particles of shape {tuple(src.shape)} on {src.device}")
        chw = src.numel() // n                                      # n >= 1 particles of chw elements
        if chw == 0:
            raise ValueError("empty particles")
    ids = torch.empty(n, dtype=torch.int64, device=d.device)
    q = torch.empty(n, dtype=torch.int32, device=d.device) if want_weights else None
    plain = scheme == "multinomial" and ess is None and not want_flags
    ex, flags, ess_out = (), None, None
    if not plain:
        sid, ess_q16 = resample_scheme_args(scheme, ess)
        if want_flags:
            flags = torch.empty(segments, dtype=torch.uint8, device=d.device)
            ess_out = torch.empty(segments, dtype=torch.float32, device=d.device)
        ex = (sid, ess_q16, ptr(flags), ptr(ess_out))
    gather, size, out = (), (), (ids,)
    if fused:
        dst, d_out = torch.empty_like(src), torch.empty_like(d)
        gather, size, out = (ptr(src), ptr(dst), ptr(d_out)), (n, chw), (dst, d_out, ids)
    name = _RESAMPLE_SYMBOLS[fused][plain]
    check(getattr(lib(), name)(ptr(d), ptr(u), segments, n // segments, float(inv_scale), *gather, ptr(ids), ptr(q), *size,
                               *ex, stream_of(src if fused else d)), name)
    return out + ((q,) if want_weights else ()) + ((flags, ess_out) if want_flags else ())


def resample_draw(d, u, segments, inv_scale, want_weights=False, scheme="multinomial", ess=None, want_flags=False):
    """The resampling draw of include/dpsx.h per segment of K = N / segments particles: d [N] distances, u [N] uniforms in
    [0, 1) (one per output slot, e.g. torch.rand) -> ids [N] int64 global particle indices, each inside its own segment;
    a pure function of (d, u), one launch, nothing read back.  want_weights: also the integer weights q [N] int32.
    scheme "stratified" / "systematic", ess (tau in [0, 1]: a segment resamples only while its effective sample size is
    below tau K, else it keeps its particles) or want_flags (also flags [segments] uint8, 1 where the segment resampled,
    and its ESS [segments] fp32) take the scheme / ESS entry point; the defaults take the plain one."""
    out = _resample(None, d, u, segments, inv_scale, want_weights, scheme, ess, want_flags)
    return out if len(out) > 1 else out[0]


def resample(src, d, u, segments, inv_scale, want_weights=False, scheme="multinomial", ess=None, want_flags=False):
    """resample_draw fused with the gathers, ONE launch: -> (src[ids], d[ids], ids[, q][, flags, ess]) for src [N, ...]
    fp32.  The results are fresh tensors (the launch does not work in place); a segment that does not resample is copied."""
    return _resample(f32c(src, "particles"), d, u, segments, inv_scale, want_weights, scheme, ess, want_flags)


def pack_champion(particles, costs=None, best=None, best_val=None, out=None):
    """This rank's record for the champion exchange (distributed._exchange_champions): [C*H*W floats of particles[best] |
    cost, (float)best, 0, 0] in ONE launch.  best=None: the torch.argmin-order select over `costs` runs inside the launch."""
    particles = f32c(particles)
    n, chw = particles.shape[0], particles[0].numel()
    costs = None if costs is None else f32c(costs.reshape(-1), "costs")
    if costs is not None and costs.numel() != n:
        raise ValueError("one cost per particle")
    best = None if best is None else best.to(device=particles.device, dtype=torch.int64).reshape(1).contiguous()
    best_val = None if best_val is None else f32c(best_val.reshape(1), "best_val")
    if out is None:
        out = torch.empty(chw + 4, dtype=torch.float32, device=particles.device)
    check(lib().dpsx_pack_champion_f32(ptr(particles), ptr(costs), ptr(best), ptr(best_val), ptr(out), n, chw,
                                       stream_of(particles)), "dpsx_pack_champion_f32")
    return out


def select_champion(table, shape, n_out=1, want_index=False):
    """table [world, C*H*W + 4] as gathered -> n_out copies of the winning rank's champion [n_out, *shape]
    (first minimum over table[:, chw], lowest rank wins ties); want_index: also (winner rank, its local index) as device
    int64 scalars.  ONE launch, nothing read on the host."""
    table = f32c(table)
    world, chw = table.shape[0], table.shape[1] - 4
    dst = torch.empty((int(n_out),) + tuple(shape), dtype=torch.float32, device=table.device)
    if dst[0].numel() != chw:
        raise ValueError("table rows do not hold a particle of this shape plus its header")
    wr = torch.empty((), dtype=torch.int64, device=table.device) if want_index else None
    wl = torch.empty((), dtype=torch.int64, device=table.device) if want_index else None
    check(lib().dpsx_select_champion_f32(ptr(table), world, chw, ptr(dst), int(n_out), ptr(wr), ptr(wl), stream_of(table)),
          "dpsx_select_champion_f32")
    return (dst, wr, wl) if want_index else dst


# ------------------------------------------------------------------ fused DPS step
class StepBuffers:
    """Persistent per-(N, C, H, W) device buffers of the fused step (resident in HBM across steps).
    parent / offset: the buffers are the particle slice [offset, offset + n) of another StepBuffers (ParticleGroups: the
    groups' sample / x_next / norm / g_model_out are contiguous slices of one full-batch set, so the UNet and the select see
    [N, ...] tensors without a copy); the op-defined residual scratch is always the group's own."""

    def __init__(self, handle, n, c, h, w, device, parent=None, offset=0):
        self.shape = (n, c, h, w)
        f = dict(dtype=torch.float32, device=device)
        if parent is None:
            self.x0_hat = torch.empty((n, c, h, w), **f)
            self.sample = torch.empty((n, c, h, w), **f)
            self.inside = torch.empty((n, c, h, w), dtype=torch.uint8, device=device)
            self.norm = torch.empty(n, **f)
            # variance half of the UNet-output cotangent is identically zero for the DPS loss: zeroed once
            self.g_model_out = torch.zeros((n, 2 * c, h, w), **f)
            self.x_next = [torch.empty((n, c, h, w), **f), torch.empty((n, c, h, w), **f)]
        else:
            if tuple(parent.shape[1:]) != (c, h, w) or offset < 0 or offset + n > parent.shape[0]:
                raise ValueError("particle slice outside the parent buffers")
            sl = slice(offset, offset + n)
            self.x0_hat, self.sample, self.inside = parent.x0_hat[sl], parent.sample[sl], parent.inside[sl]
            self.norm, self.g_model_out = parent.norm[sl], parent.g_model_out[sl]
            self.x_next = [parent.x_next[0][sl], parent.x_next[1][sl]]
        rb = 0
        if handle is not None:
            rb = lib().dpsx_step_resid_bytes(handle._h, n, c, h, w)
            if rb < 0:
                check(int(rb), "dpsx_step_resid_bytes")
        self.resid = torch.empty(max(int(rb), 256), dtype=torch.uint8, device=device)
        self.flip = 0
        self._noise = None
        self._dsg_stats = None
        # the multistep update's history (step_update_ms): the second x0_hat buffer exists from the first advance_x0() on
        self._parent, self._offset = parent, offset
        self._x0_pair, self._x0_at = None, 0
        self._x0_moved = None
        self.x0_prev = None

    def _x0_buffers(self):
        """the two buffers x0_hat alternates between (the second one allocated on first use; a group's are its slices of
        the parent's pair)"""
        if self._x0_pair is None:
            if self._parent is None:
                self._x0_pair = [self.x0_hat, torch.empty_like(self.x0_hat)]
            else:
                sl = slice(self._offset, self._offset + self.shape[0])
                self._x0_pair = [v[sl] for v in self._parent._x0_buffers()]
        return self._x0_pair

    def advance_x0(self):
        """A step that keeps the previous step's x0_hat as history starts here: x0_hat becomes the other buffer of the
        pair (K1 writes the new x0_hat over the one no longer needed, nothing is copied) and x0_prev what it was -- or the
        tensor set_x0_history() put in its place.  Everything that reads buf.x0_hat during or after the step reads the
        current one; a parent's x0_hat follows its groups (which advance together)."""
        pair = self._x0_buffers()
        self.x0_prev = pair[self._x0_at] if self._x0_moved is None else self._x0_moved
        self._x0_moved = None
        self._x0_at ^= 1
        self.x0_hat = pair[self._x0_at]
        if self._parent is not None:
            self._parent.x0_hat = self._parent._x0_buffers()[self._x0_at]
        return self.x0_prev

    def set_x0_history(self, x0):
        """the next advance_x0() hands out `x0` [n, c, h, w] as x0_prev instead of the current x0_hat (a resampling moved
        the particles: the history moves with them)"""
        if tuple(x0.shape) != tuple(self.shape):
            raise ValueError(f"history of shape {tuple(x0.shape)} for step buffers of shape {self.shape}")
        self._x0_moved = f32c(x0, "x0 history")

    def dsg_stats(self):
        """[n, corr_slots, 4] partial sums of step_update_dsg, the buffers' own (allocated on first use)"""
        if self._dsg_stats is None:
            n, c, h, w = self.shape
            self._dsg_stats = torch.empty((n, corr_slots(c * h * w), 4), dtype=torch.float32, device=self.sample.device)
        return self._dsg_stats

    def noise_buffer(self):
        """[n, c, h, w] scratch that step_fwd(rng=) fills for operators without an in-kernel draw (allocated on first use)"""
        if self._noise is None:
            self._noise = torch.empty(self.shape, dtype=torch.float32, device=self.sample.device)
        return self._noise


class CgBuffers:
    """Persistent device buffers of OpHandle.cg_step / cg_pullback for one (N, C, H, W): the two x_next buffers they
    alternate between, dist, the solve's workspace (dpsx_cg_workspace_bytes) and, on first request, d and g_model_out
    ([N, 2C, H, W], zeroed once: the pullback writes the eps half only).  `sample` is the pgdm step's S1 sample, which
    step_update reads beside g_model_out.  One allocation per (handle, shape), reused across steps and trajectories."""

    def __init__(self, handle, n, c, h, w, device):
        self.shape = (n, c, h, w)
        f = dict(dtype=torch.float32, device=device)
        need = lib().dpsx_cg_workspace_bytes(handle._h, n, c, h, w)
        if need < 0:
            check(int(need), "dpsx_cg_workspace_bytes")
        self.ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=device)
        self.x_next = [torch.empty((n, c, h, w), **f), torch.empty((n, c, h, w), **f)]
        self.dist = torch.empty(n, **f)
        self.flip = 0
        self._d = None
        self.g_model_out = None
        self.sample = None

    def d_buffer(self):
        if self._d is None:
            self._d = torch.empty(self.shape, dtype=torch.float32, device=self.dist.device)
        return self._d

    def g_model_out_buffer(self):
        if self.g_model_out is None:
            n, c, h, w = self.shape
            self.g_model_out = torch.zeros((n, 2 * c, h, w), dtype=torch.float32, device=self.dist.device)
        return self.g_model_out


def cg_kappa(coefs):
    """the slope of the sampler's `sample` in x0_hat, as dpsx_cg_step_f32 evaluates it (fp32, in this order): c1 for a
    DDPM record, c1 - c2 / b for a DDIM record (eps is re-derived from x0_hat; the variance does not depend on it)"""
    c1, c2, b = np.float32(coefs.c1), np.float32(coefs.c2), np.float32(coefs.b)
    return float(c1 - c2 / b) if coefs.add_noise & 2 else float(c1)


def pgdm_scalars(abar, abar_prev, coefs_f64, sigma_y, weighting="score", weight=1.0):
    """Pseudoinverse guidance's host scalars of one step (include/dpsx.h: dpsx_cg_pullback_f32), formed in float64 and
    rounded to fp32 once each -> (rho, gain).  abar, abar_prev: the sampler's abar_t and the abar the step lands on;
    coefs_f64: the step's record in float64, (a, b, c1, c2, ddim) with ddim = the record re-derives eps (bit 1 of add_noise).
        rho  = sigma_y^2 / (1 - abar)
        gain = weight w b ,  w = kappa a ("score": kappa = c1, or c1 - c2 / b for a DDIM record) | sqrt(abar_prev) / a ("paper")"""
    a, b, c1, c2, ddim = coefs_f64
    a, b, c1, c2 = np.float64(a), np.float64(b), np.float64(c1), np.float64(c2)
    if weighting == "score":
        w = (c1 - c2 / b if ddim else c1) * a
    elif weighting == "paper":
        w = np.sqrt(np.float64(abar_prev)) / a
    else:
        raise ValueError(f"pgdm: weighting must be 'score' or 'paper' (got {weighting!r})")
    rho = np.float64(sigma_y) ** 2 / (1.0 - np.float64(abar))
    return float(np.float32(rho)), float(np.float32(np.float64(weight) * w * b))


def _stream_arg(stream, t):
    """stream: None (torch's current stream on t's device -- a 4.5 us lookup per launch) or a torch.cuda.Stream, whose
    raw handle a caller that drives several particle groups passes explicitly instead of entering a stream context
    (another 8 us per group and step: three groups cost the host 96 us per step that way, 35 this way).
    torch's caching allocator does not know about work enqueued this way: every tensor handed to a launch on a side stream
    must outlive that stream's work or be marked with `t.record_stream(stream)` (ParticleGroups does both for what it
    owns / is handed per step)."""
    if stream is None:
        return stream_of(t)
    if stream.device != t.device:
        raise ValueError(f"stream on {stream.device} given for tensors on {t.device}")
    return ctypes.c_void_p(stream.cuda_stream)


def step_fwd(handle, buf, x_t, model_out, noise=None, y=None, coefs=None, finalize_norm=False, want_x0=True, stream=None,
             rng=None):
    """K1.  finalize_norm=False (the loop's setting): buf.norm is filled by the following step_bwd, whose prologue
    finalises the per-tile partial sums this launch leaves in the workspace.  finalize_norm=True: the launch finishes
    buf.norm itself (each particle's last block re-sums the partials in the same fixed order -- same bits) and
    step_bwd reads one float per particle; measured at N = 64: K1 +4.8 us, K2 -3.3 us, so the loop does not use it.
    want_x0=False (blur and resize operators): x0_hat is consumed inside the launch and not written to buf.x0_hat --
    the `ps` step reads it nowhere afterwards (the backward half works from the clamp gate); other operators ignore
    the flag.
    rng= (instead of noise=): the noise of kernels.Rng is drawn inside the launch where the operator has that form
    (handle.draws_in_kernel); elsewhere a persistent buffer of buf is filled by `randn` on the same stream and the pointer
    launch runs -- the same bits either way."""
    _noise_or_rng(noise, rng)
    n, c, h, w = buf.shape
    ws = handle.workspace(n, c, h, w, x_t.device)
    buf.norm_ready = bool(finalize_norm)
    optional = handle.kind in (_lib.KIND_SEP, _lib.KIND_TAPS, _lib.KIND_RESIZE) or \
        (handle.kind == _lib.KIND_PHASE and (h, w) == (256, 256) and getattr(handle, "spectral", False))
    x0_out = None if optional and not want_x0 else buf.x0_hat
    if rng is not None:
        if handle.draws_in_kernel(c, h, w):
            rc = lib().dpsx_step_fwd_rng_f32(handle._h, ptr(x_t), ptr(model_out), byref(rng.rec()), ptr(y), y.shape[0],
                                             ptr(x0_out), ptr(buf.sample), ptr(buf.inside), ptr(buf.resid),
                                             ptr(buf.norm) if finalize_norm else None,
                                             n, c, h, w, byref(coefs), ptr(ws), ws.numel(), _stream_arg(stream, x_t))
            if rc != _lib.EUNSUPPORTED:      # declined (nothing was launched, e.g. an unaligned view): the pointer form
                check(rc, "dpsx_step_fwd_rng_f32")
                return
        noise = buf.noise_buffer()
        if coefs.add_noise & 1:          # the t = 0 step reads no noise
            check(lib().dpsx_randn_f32(ptr(noise), None, n, c * h * w, byref(rng.rec()), _stream_arg(stream, x_t)),
                  "dpsx_randn_f32")
    check(lib().dpsx_step_fwd_f32(handle._h, ptr(x_t), ptr(model_out), ptr(noise), ptr(y), y.shape[0],
                                  ptr(x0_out), ptr(buf.sample), ptr(buf.inside), ptr(buf.resid),
                                  ptr(buf.norm) if finalize_norm else None,
                                  n, c, h, w, byref(coefs), ptr(ws), ws.numel(), _stream_arg(stream, x_t)),
          "dpsx_step_fwd_f32")


def step_bwd(handle, buf, y, scale, power, coefs, g_x0_extra=None, stream=None):
    """K2.  g_x0_extra: optional [N, C, H, W] cotangent on x0_hat of a further loss term (the semantic-guidance
    term's VJP through the embedder), added to coef * A^T r before the clamp gate."""
    n, c, h, w = buf.shape
    ws = handle.workspace(n, c, h, w, buf.x0_hat.device)
    ready = getattr(buf, "norm_ready", True)
    if g_x0_extra is not None:
        g_x0_extra = f32c(g_x0_extra, "g_x0_extra")
        if tuple(g_x0_extra.shape) != (n, c, h, w):
            raise ValueError("g_x0_extra must have the particle batch's shape")
    check(lib().dpsx_step_bwd_extra_f32(handle._h, ptr(buf.resid), ptr(buf.norm) if ready else None, ptr(buf.norm),
                                        ptr(buf.inside), ptr(buf.x0_hat),
                                        ptr(y), y.shape[0], float(scale), int(power), ptr(g_x0_extra),
                                        ptr(buf.g_model_out),
                                        n, c, h, w, byref(coefs), ptr(ws), ws.numel(), _stream_arg(stream, buf.x0_hat)),
          "dpsx_step_bwd_extra_f32")
    buf.norm_ready = True


def step_update(buf, g_unet, coefs, stream=None):
    n, c, h, w = buf.shape
    out = buf.x_next[buf.flip]
    buf.flip ^= 1
    check(lib().dpsx_step_update_f32(ptr(buf.sample), ptr(buf.g_model_out), ptr(g_unet), ptr(out), n, c * h * w,
                                     byref(coefs), _stream_arg(stream, buf.sample)), "dpsx_step_update_f32")
    return out


def step_update_ms(buf, g_unet, coefs, c, stream=None):
    """step_update's twin for a multistep (DPM-Solver++ 2M) step, one launch (dpsx_step_update_ms_f32):
    x_next = sample - s + c (buf.x0_hat - buf.x0_prev), c a host scalar (DDIM.solver_coef).  c == 0: the histories are
    not read (buf.x0_prev may be None) and x_next has step_update's bits.  buf.x0_prev is what buf.advance_x0() left at
    the start of the step; x_next flips as in step_update."""
    n, ch, h, w = buf.shape
    c = float(c)
    if c != 0.0 and buf.x0_prev is None:
        raise ValueError("step_update_ms with c != 0 needs the previous step's x0_hat (buf.advance_x0() before K1)")
    hist = (ptr(buf.x0_hat), ptr(buf.x0_prev)) if c != 0.0 else (None, None)
    out = buf.x_next[buf.flip]
    buf.flip ^= 1
    check(lib().dpsx_step_update_ms_f32(ptr(buf.sample), ptr(buf.g_model_out), ptr(g_unet), *hist, c, ptr(out), n,
                                        ch * h * w, byref(coefs), _stream_arg(stream, buf.sample)),
          "dpsx_step_update_ms_f32")
    return out


# ------------------------------------------------------------------ particle weights (include/dpsx.h: "particle weights")
def corr_slots(chw):
    """partial slots per particle of step_update_corr: a function of the particle size only (dpsx_corr_slots)"""
    slots = lib().dpsx_corr_slots(int(chw))
    if slots < 0:
        check(int(slots), "dpsx_corr_slots")
    return int(slots)


class SmcState:
    """The weights of one particle set [N, *shape]: E [N] the negative log-weights, d_prev [N] the last step's distances
    (both start at 0) and corr_partials [N, corr_slots] that step_update_corr fills and smc_accum consumes."""

    def __init__(self, n, shape, device):
        self.n, self.shape = int(n), tuple(int(v) for v in shape)
        self.slots = corr_slots(int(np.prod(self.shape, dtype=np.int64)))
        f = dict(dtype=torch.float32, device=device)
        self.E, self.d_prev = torch.zeros(self.n, **f), torch.zeros(self.n, **f)
        self.corr_partials = torch.empty((self.n, self.slots), **f)


def _update_place(buf, model_out, noise, rng):
    """what the launches in K3's place share: exactly one noise source, model_out against the buffers' shape, the x_next
    buffer of this step (the ping-pong flips) and the rng record's pointer -> (out, rng pointer or None)"""
    _noise_or_rng(noise, rng)
    n, c, h, w = buf.shape
    if model_out is not None and (model_out.shape[0] != n or (n and model_out[0].numel() != 2 * c * h * w)):
        raise ValueError(f"model_out {tuple(model_out.shape)} does not hold 2x the channels of {buf.shape}")
    out = buf.x_next[buf.flip]
    buf.flip ^= 1
    return out, None if rng is None else byref(rng.rec())


def step_update_corr(buf, g_unet, coefs, model_out, noise=None, rng=None, state=None, stream=None):
    """K3 with the proposal correction's partial sums, one launch (dpsx_step_update_corr_f32): -> (x_next, corr_partials).
    x_next has step_update's bits; corr_partials [N, corr_slots] (state.corr_partials, or a fresh tensor) holds
    sum q (z - q / 2), q = s / sd, per block.  model_out is the UNet output K1 read (its variance half gives sd); the noise
    is K1's: noise= or the same rng=, exactly one of them."""
    n, c, h, w = buf.shape
    part = state.corr_partials if state is not None else \
        torch.empty((n, corr_slots(c * h * w)), dtype=torch.float32, device=buf.sample.device)
    if tuple(part.shape) != (n, corr_slots(c * h * w)):
        raise ValueError(f"SmcState of {tuple(part.shape)} partials for step buffers of shape {buf.shape}")
    out, rec = _update_place(buf, model_out, noise, rng)
    check(lib().dpsx_step_update_corr_f32(ptr(buf.sample), ptr(buf.g_model_out), ptr(g_unet), ptr(model_out), ptr(noise), rec,
                                          ptr(out), ptr(part), n, c * h * w, byref(coefs), _stream_arg(stream, buf.sample)),
          "dpsx_step_update_corr_f32")
    return out, part


def smc_accum(state, d_cur, reset=None, segments=1, twist_scale=0.01, power=1, proposal_weight=1.0, stream=None):
    """state.E += twist_scale (d_cur^power - d_prev^power) - proposal_weight corr; state.d_prev = d_cur, in place, one small
    launch (dpsx_smc_accum_f32).  corr is the fixed-order double sum of state.corr_partials; proposal_weight = 0 drops the
    term (the partials are then not read).  reset [segments] uint8 (the flags of the last resampling, or None): a flagged
    segment's particles restart from E = 0."""
    d_cur = f32c(d_cur.reshape(-1), "distances")
    if d_cur.numel() != state.n or d_cur.device != state.E.device:
        raise ValueError(f"{d_cur.numel()} distances on {d_cur.device} for the weights of {state.n} particles")
    segments = int(segments)
    if reset is not None and (reset.dtype != torch.uint8 or reset.numel() != segments or not reset.is_contiguous()):
        raise ValueError(f"reset must be a contiguous uint8 tensor with one flag per segment ({segments})")
    part = state.corr_partials if float(proposal_weight) != 0.0 else None
    check(lib().dpsx_smc_accum_f32(ptr(state.E), ptr(state.d_prev), ptr(d_cur), ptr(part), state.slots, ptr(reset), segments,
                                   state.n, float(twist_scale), int(power), float(proposal_weight),
                                   _stream_arg(stream, state.E)), "dpsx_smc_accum_f32")
    return state.E


# ------------------------------------------------------------------ spherical-Gaussian guidance (include/dpsx.h)
def step_update_dsg(buf, g_unet, coefs, model_out, guidance_rate, noise=None, rng=None, stats=None, stream=None):
    """DSG in K3's place, two launches (dpsx_step_update_dsg_f32): -> (x_next, stats).  x_next lies on the sphere of radius
    ||sd|| around the model's mean, between the drawn noise direction (guidance_rate = 0) and the steepest-descent direction
    of s = (-a/b) g_eps + g_unet (guidance_rate = 1); stats [N, corr_slots, 4] (the given tensor, or a fresh one) holds the
    per-block partials of (sum s^2, sum n^2, sum s n, sum sd^2).  model_out is the UNet output K1 read (its variance half
    gives sd); the noise is K1's: noise= or the same rng=, exactly one of them."""
    n, c, h, w = buf.shape
    want = (n, corr_slots(c * h * w), 4)
    if stats is None:
        stats = torch.empty(want, dtype=torch.float32, device=buf.sample.device)
    if tuple(stats.shape) != want or stats.dtype != torch.float32 or not stats.is_contiguous() or \
            stats.device != buf.sample.device:
        raise ValueError(f"stats must be a contiguous float32 {want} tensor on {buf.sample.device} for step buffers of "
                         f"shape {buf.shape}")
    out, rec = _update_place(buf, model_out, noise, rng)
    check(lib().dpsx_step_update_dsg_f32(ptr(buf.sample), ptr(buf.g_model_out), ptr(g_unet), ptr(model_out), ptr(noise), rec,
                                         float(guidance_rate), ptr(out), ptr(stats), n, c * h * w, byref(coefs),
                                         _stream_arg(stream, buf.sample)), "dpsx_step_update_dsg_f32")
    return out, stats


# ------------------------------------------------------------------ what the analysis calls share
# (metrics, repulsion, ensemble, order statistics, principal components): the cache of the calls' workspaces, the shape rule
# of an image-major particle set and the labels of its images
# (size query, device, the query's arguments) -> the call's workspace, as StepBuffers keeps its buffers per shape; the
# query's name is in the key: two families never share a buffer
_workspaces = {}


def _workspace(query, device, *shape):
    """the cached workspace of an analysis call: lib().<query>(*shape) bytes on `device` (a refusal raises under the
    query's name); serves one stream at a time"""
    key = (query, device) + shape
    ws = _workspaces.get(key)
    if ws is None:
        need = getattr(lib(), query)(*shape)
        if need < 0:
            check(int(need), query)
        ws = _workspaces[key] = torch.empty(max(int(need), 256), dtype=torch.uint8, device=device)
    return ws


def _particle_shape(shape, images, nchw=True, allow_empty=False):
    """the shape rule of an image-major particle set: `shape` [N, C, H, W] (nchw False: [N, ...]) splits into `images`
    images of K = N / images consecutive particles of D elements -> (N, K, D, images).  allow_empty: N == 0 is a set"""
    if len(shape) != 4 if nchw else len(shape) < 2:
        raise ValueError(f"particles must be {'[N, C, H, W]' if nchw else '[N, ...]'} (got {tuple(shape)})")
    n, images = int(shape[0]), int(images)
    if images < 1 or n % images or (n < 1 and not allow_empty):
        raise ValueError(f"{n} particles do not split into {images} images")
    return n, n // images, int(np.prod(shape[1:], dtype=np.int64)), images


def _particle_set(x, images, nchw=True, allow_empty=False):
    """x as the library takes a particle set (contiguous float32 on the device) and its shape -> (x, N, K, D, images)"""
    x = f32c(x, "particles")
    return (x,) + _particle_shape(x.shape, images, nchw, allow_empty)


def _label_rows(label, x, images=None):
    """label as [M, C, H, W] for particles x [N, C, H, W]: [C, H, W], [1, ...] or [M, ...] with M | N.  images: the labels
    of `images` images -- one label serves them all (expanded), otherwise the counts must match"""
    label = f32c(label, "label")
    if label.dim() == 3:
        label = label.unsqueeze(0)
    if label.dim() != 4 or tuple(label.shape[1:]) != tuple(x.shape[1:]):
        raise ValueError(f"label {tuple(label.shape)} does not match particles {tuple(x.shape)}")
    if label.device != x.device:
        raise ValueError(f"label on {label.device} for particles on {x.device}")
    m = label.shape[0]
    if m < 1 or x.shape[0] % m:
        raise ValueError(f"{m} labels do not divide {x.shape[0]} particles")
    if images is not None:
        if m == 1 and images > 1:
            label = label.expand((images,) + tuple(x.shape[1:])).contiguous()
        if label.shape[0] != images:
            raise ValueError(f"{label.shape[0]} labels given for {images} images")
    return label


# ------------------------------------------------------------------ image metrics (include/dpsx.h: "reconstruction metrics")
METRIC_NAMES = ("mse", "psnr", "ssim")


def image_metrics(x, label, data_range=None, want=METRIC_NAMES, out=None, stream=None):
    """Per-particle mse / psnr / ssim of x [N, C, H, W] against its label row, one device call (dpsx_image_metrics_f32):
    -> {name: [N] float32 tensor} for the names in `want`.  label: [C, H, W], [1, ...] or [M, ...] with M | N, image-major
    (particle p belongs to label p // (N // M)).  data_range None: each label's max - min, as metrics.compute_psnr.
    out: a dict of preallocated contiguous float32 [N] tensors to write into (names missing from it are allocated).
    No host read; the workspace is cached per shape and serves one stream at a time."""
    want = tuple(want)
    if not want or any(k not in METRIC_NAMES for k in want) or len(set(want)) != len(want):
        raise ValueError(f"want must name some of {METRIC_NAMES} once each (got {want})")
    x = _particle_set(x, 1, allow_empty=True)[0]             # the images are the label's rows: M | N is _label_rows' rule
    label = _label_rows(label, x)
    n, c, h, w = (int(v) for v in x.shape)
    m = int(label.shape[0])
    res = {}
    for k in want:
        t = out.get(k) if out is not None else None
        if t is None:
            t = torch.empty(n, dtype=torch.float32, device=x.device)
        elif tuple(t.shape) != (n,) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != x.device:
            raise ValueError(f"out[{k!r}] must be a contiguous float32 [{n}] tensor on {x.device}")
        res[k] = t
    ws = _workspace("dpsx_metrics_workspace_bytes", x.device, n, m, c, h, w)
    check(lib().dpsx_image_metrics_f32(ptr(x), ptr(label), m, 0.0 if data_range is None else float(data_range),
                                       ptr(res.get("mse")), ptr(res.get("psnr")), ptr(res.get("ssim")), n, c, h, w,
                                       ptr(ws), ws.numel(), _stream_arg(stream, x)), "dpsx_image_metrics_f32")
    return res


class MetricTrace:
    """A per-step view of x0_hat's true quality beside the measurement distance the selects steer by, for the fused base
    loop (sampler.metric_trace = MetricTrace(label, every=k)): on the steps with idx % every == 0 the loop has K1 write
    x0_hat and calls record(), which puts image_metrics(x0_hat) and the step's distance into row idx // every of
    `data` [rows, N, 4] (columns COLUMNS; rows of steps that did not run stay NaN).  One device call and one small
    device copy per traced step, no host read; evaluation only -- the label never reaches the sampler's arithmetic."""

    COLUMNS = ("mse", "psnr", "ssim", "distance")

    def __init__(self, label, every=1, data_range=None):
        if isinstance(every, bool) or int(every) != every or every < 1:
            raise ValueError(f"every must be a positive integer (got {every!r})")
        self.label, self.every, self.data_range = label, int(every), data_range
        self.data = self._store = None

    def start(self, num_steps, x):
        """allocate `data` for a loop of num_steps steps over particles shaped like x (checks the label against them)"""
        self.label = _label_rows(self.label, x)
        rows = (int(num_steps) - 1) // self.every + 1
        # stored [rows, 4, N] so that a row's columns are the call's contiguous [N] outputs; `data` is the [rows, N, 4] view
        self._store = torch.full((rows, 4, x.shape[0]), float("nan"), dtype=torch.float32, device=x.device)
        self.data = self._store.permute(0, 2, 1)
        return self

    def record(self, idx, x0_hat, distance, stream=None):
        row = self._store[idx // self.every]
        image_metrics(x0_hat, self.label, data_range=self.data_range, out={k: row[j] for j, k in enumerate(METRIC_NAMES)},
                      stream=stream)
        row[3].copy_(distance.reshape(-1))


# ------------------------------------------------------------------ particle repulsion (include/dpsx.h: "particle repulsion")
REPULSE_MAX_K = 512      # particles per image (DPSX_EUNSUPPORTED above)
REPULSE_INFO = ("h", "gain", "mean", "min")      # the columns of info [M, 4]


def _repulse_args(x, images):
    x, n, _, chw, images = _particle_set(x, images, nchw=False, allow_empty=True)
    return x, n, chw, images, _workspace("dpsx_repulse_workspace_bytes", x.device, n, chw, images)


def pairwise_sqdist(x, images=1, want_info=False, stream=None):
    """The squared distances between the particles of every image, one device call (dpsx_pairwise_sqdist_f32): x [N, ...],
    image-major, `images` images of K = N / images particles -> d2 [images, K, K] float32 (symmetric bit for bit, +0.0 on
    the diagonal, exactly 0 between particles with equal bits).  want_info: -> (d2, info [images, 4]) with the columns
    REPULSE_INFO: the mean heuristic's bandwidth h, 0, the mean and the minimum off-diagonal distance (0: duplicates).
    K <= 512.  No host read; the workspace is cached per shape and serves one stream at a time."""
    x, n, chw, images, ws = _repulse_args(x, images)
    k = n // images
    d2 = torch.empty((images, k, k), dtype=torch.float32, device=x.device)
    info = torch.empty((images, 4), dtype=torch.float32, device=x.device) if want_info else None
    check(lib().dpsx_pairwise_sqdist_f32(ptr(x), ptr(d2), ptr(info), n, chw, images, ptr(ws), ws.numel(),
                                         _stream_arg(stream, x)), "dpsx_pairwise_sqdist_f32")
    return (d2, info) if want_info else d2


def repulse_strength(value, what="strength"):
    """a strength / bandwidth of the repulsion step as the library takes it: a finite float >= 0 (ValueError otherwise)"""
    try:
        v = float(value)
    except (TypeError, ValueError):
        v = float("nan")
    if isinstance(value, bool) or not (v >= 0.0) or v == float("inf"):
        raise ValueError(f"{what} must be a finite number >= 0 (got {value!r})")
    return v


def repulse(x, strength, images=1, bandwidth=None, out=None, want_info=False, stream=None):
    """The repulsion step (dpsx_repulse_f32, three launches): every particle of an image is pushed away from the image's
    other particles, out_i = x_i + gain sum_j w_ij (x_i - x_j) with w_ij = exp(-d2_ij / h), gain = 2 strength / h and
    h = bandwidth * D (bandwidth: a mean squared per-element difference) or, with bandwidth None / 0, mean d2 / ln(K + 1).
    x [N, ...] image-major, `images` images of K = N / images <= 512 particles; x is not written.  An image of one
    particle, of equal particles, or with a NaN / Inf in it is copied.  out: a contiguous float32 tensor shaped like x that
    does not overlap it (default: a fresh one).  want_info: -> (out, {"d2": [M, K, K], "w": [M, K, K], "info": [M, 4]
    (REPULSE_INFO), "applied": [M] uint8}).  No host read; the workspace is cached per shape and serves one stream at a time."""
    c = repulse_strength(strength)
    bw = 0.0 if bandwidth is None else repulse_strength(bandwidth, "bandwidth")
    x, n, chw, images, ws = _repulse_args(x, images)
    if out is None:
        out = torch.empty_like(x)
    elif tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32 or not out.is_contiguous() or \
            out.device != x.device:
        raise ValueError(f"out must be a contiguous float32 {tuple(x.shape)} tensor on {x.device}")
    k = n // images
    rec = None
    if want_info:
        f = dict(dtype=torch.float32, device=x.device)
        rec = {"d2": torch.empty((images, k, k), **f), "w": torch.empty((images, k, k), **f),
               "info": torch.empty((images, 4), **f), "applied": torch.empty(images, dtype=torch.uint8, device=x.device)}
    g = rec.get if rec else (lambda name: None)
    check(lib().dpsx_repulse_f32(c, bw, ptr(x), ptr(out), ptr(g("d2")), ptr(g("w")), ptr(g("info")), ptr(g("applied")),
                                 n, chw, images, ptr(ws), ws.numel(), _stream_arg(stream, x)), "dpsx_repulse_f32")
    return (out, rec) if want_info else out


# ------------------------------------------------------------------ ensemble statistics (include/dpsx.h: "ensemble statistics")
ENSEMBLE_MAX_K = 4096    # particles per image (DPSX_EUNSUPPORTED above)
ENSEMBLE_INFO = ("ess", "mean_var", "mse", "count")      # the columns of info [M, 4]


def ensemble_stats(x, images=1, label=None, neg_log_weights=None, prior=None, stream=None):
    """Mean, per-pixel variance and mean-of-n curve of every image's particles, one device call (dpsx_ensemble_ex_f32, at
    most three launches): x [N, C, H, W] image-major, `images` images of K = N / images <= 4096 particles; x is not written.
    label: [C, H, W], [1, ...] or [images, ...] (None: no curve).  neg_log_weights [N]: SMC's negative log-weights (None:
    uniform); a non-finite entry is weight 0, an image with none finite takes the uniform form.  prior: an earlier group of
    the same images, merged in (not together with weights): (count0, mean0, var0), (count0, mean0, var0, mean_lo, var_lo)
    or the dict an earlier call returned (the count being the same for every image).  mean0 and var0 are fp32; the low
    parts are what that rounding dropped, and with them groups merged call after call come out as one call over all of
    them would.  The prior's tensors are not written.
    -> {"mean", "var", "mean_lo", "var_lo": [M, C, H, W], "info": [M, 4] (ENSEMBLE_INFO), "count": T} and, with a label,
    "curve": [M, K] (curve[m][n - 1]: mse of the mean of the first n paths) and "final_mse": [M] (the returned mean's).
    No host read; the workspace is cached per shape and serves one stream at a time."""
    x, n, k, d, images = _particle_set(x, images)
    shape = (images,) + tuple(x.shape[1:])
    if label is not None:
        label = _label_rows(label, x, images)
    e = None
    if neg_log_weights is not None:
        if prior is not None:
            raise ValueError("neg_log_weights cannot be combined with a prior: two calls share no reference level")
        e = f32c(neg_log_weights, "neg_log_weights").reshape(-1)
        if e.numel() != n or e.device != x.device:
            raise ValueError(f"neg_log_weights must hold {n} values on {x.device}")
    count0 = 0
    new = lambda: torch.empty(shape, dtype=torch.float32, device=x.device)
    if prior is not None:
        if isinstance(prior, dict):
            prior = (prior["count"], prior["mean"], prior["var"], prior.get("mean_lo"), prior.get("var_lo"))
        count0, mean0, var0, lo_m, lo_v = tuple(prior) + (None, None) * (len(prior) == 3)
        if isinstance(count0, bool) or int(count0) != count0 or count0 < 0:
            raise ValueError(f"the prior's count must be an integer >= 0 (got {count0!r})")
        if (lo_m is None) != (lo_v is None):
            raise ValueError("the prior's low parts come as a pair: mean_lo and var_lo")
        count0, given = int(count0), [("mean0", mean0), ("var0", var0)] + ([("mean_lo", lo_m), ("var_lo", lo_v)] if lo_m is not None else [])
        for name, t in given:
            if tuple(t.shape) != shape or t.device != x.device:
                raise ValueError(f"the prior's {name} must be {shape} on {x.device} (got {tuple(t.shape)} on {t.device})")
        # in/out: the caller's prior stays
        mean, var = f32c(mean0, "mean0").clone(), f32c(var0, "var0").clone()
        mean_lo, var_lo = (f32c(lo_m, "mean_lo").clone(), f32c(lo_v, "var_lo").clone()) if lo_m is not None else \
            (torch.zeros_like(mean), torch.zeros_like(var))
    else:
        mean, var, mean_lo, var_lo = new(), new(), new(), new()
    ws = _workspace("dpsx_ensemble_workspace_bytes", x.device, n, d, images)
    curve = torch.empty((images, k + 1), dtype=torch.float32, device=x.device) if label is not None else None
    info = torch.empty((images, 4), dtype=torch.float32, device=x.device)
    check(lib().dpsx_ensemble_ex_f32(ptr(x), ptr(label), ptr(e), count0, ptr(mean), ptr(var), ptr(mean_lo), ptr(var_lo),
                                     ptr(curve), ptr(info), n, d, images, ptr(ws), ws.numel(), _stream_arg(stream, x)),
          "dpsx_ensemble_ex_f32")
    res = {"mean": mean, "var": var, "mean_lo": mean_lo, "var_lo": var_lo, "info": info, "count": count0 + k}
    if curve is not None:
        res["curve"], res["final_mse"] = curve[:, :k], curve[:, k]
    return res


# ------------------------------------------------------------------ order statistics (include/dpsx.h: "order statistics")
QUANTILE_MAX_K = 512     # particles per image (DPSX_EUNSUPPORTED above)
QUANTILE_MAX_Q = 8       # probabilities per call
QUANTILE_INFO = ("crps", "width", "invalid", "count")    # the columns of info [M, 4]


def quantile_probs(probs):
    """the probabilities of an order_stats call as the library takes them: 1 .. 8 floats in [0, 1] (ValueError otherwise)"""
    try:
        p = [float(v) for v in probs]
    except TypeError:
        p = [float(probs)]
    if not 1 <= len(p) <= QUANTILE_MAX_Q:
        raise ValueError(f"between 1 and {QUANTILE_MAX_Q} probabilities are taken (got {len(p)})")
    if any(not (0.0 <= v <= 1.0) for v in p):
        raise ValueError(f"probabilities must lie in [0, 1] (got {p})")
    return p


def order_stats(x, images=1, probs=(0.05, 0.5, 0.95), label=None, stream=None):
    """Per-pixel quantiles of every image's particles and, with a label, the rank histogram and the CRPS, one device call
    (dpsx_quantiles_f32, two launches): x [N, C, H, W] image-major, `images` images of K = N / images <= 512 particles; x
    is not written.  probs: 1 .. 8 probabilities in [0, 1] (linear interpolation between the order statistics, numpy's
    default).  label: [C, H, W], [1, ...] or [images, ...].
    -> {"quantiles": [M, q, C, H, W], "info": [M, 4] (QUANTILE_INFO)} and, with a label, "hist": [M, K + 2] int32 (bin r:
    the elements whose label exceeds exactly r particles; bin K + 1: a NaN in the label or a particle) and "crps": [M].
    An element with a NaN particle is NaN in all q maps.  The library's refusals are raised as ValueError before any
    launch.  No host read; the workspace is cached per shape and serves one stream at a time."""
    x, n, k, d, images = _particle_set(x, images)
    if k > QUANTILE_MAX_K:
        raise ValueError(f"order statistics take at most {QUANTILE_MAX_K} particles per image (got {k})")
    if d < 1 or images > 65535 or d >= 2 ** 31:
        raise ValueError(f"order statistics take 1 <= C H W < 2^31 and at most 65535 images (got {d}, {images})")
    p = quantile_probs(probs)
    q = len(p)
    if label is not None:
        label = _label_rows(label, x, images)
    ws = _workspace("dpsx_quantiles_workspace_bytes", x.device, n, d, images)
    quant = torch.empty((images, q) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    hist = torch.empty((images, k + 2), dtype=torch.int32, device=x.device) if label is not None else None
    info = torch.empty((images, 4), dtype=torch.float32, device=x.device)
    check(lib().dpsx_quantiles_f32(ptr(x), ptr(label), (ctypes.c_double * q)(*p), q, ptr(quant), ptr(hist), ptr(info), n, d,
                                   images, ptr(ws), ws.numel(), _stream_arg(stream, x)), "dpsx_quantiles_f32")
    res = {"quantiles": quant, "info": info}
    if label is not None:
        res["hist"], res["crps"] = hist, info[:, 0]
    return res


# ------------------------------------------------------------------ principal components (include/dpsx.h: "principal components")
PCA_MAX_K = 128          # particles per image (DPSX_EUNSUPPORTED above): the eigensolver's matrices live in LDS
PCA_MAX_Q = 8            # components per call
PCA_INFO = ("trace", "rank", "sweeps", "count")          # the columns of info [M, 4]


def pca_components(value, what="components"):
    """the component count of a particle_pca call as the library takes it: an integer in 1 .. 8 (ValueError otherwise)"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= PCA_MAX_Q:
        raise ValueError(f"{what} must be an integer in 1 .. {PCA_MAX_Q} (got {value!r})")
    return int(value)


def particle_pca(x, images=1, components=4, want_d2=False, stream=None):
    """The principal components of every image's particles, one device call (dpsx_pca_f32, four launches): x [N, C, H, W]
    image-major, `images` images of K = N / images <= 128 particles; x is not written.  components: q in 1 .. 8.
    -> {"dirs": [M, q, C, H, W] (unit directions u_j, descending variance), "evals": [M, q] (eigenvalues of the centred
    Gram matrix), "var": [M, q] (evals / K: the biased variance along u_j), "explained": [M, q] (evals / trace),
    "coords": [M, K, q] (the score of particle i along u_j), "info": [M, 4] (PCA_INFO)} and, with want_d2, "d2": [M, K, K]
    (kernels.pairwise_sqdist's bits).  A component below the solver's resolution is all zero; an image of equal particles
    is all zero with rank 0 (its `explained` is 0 / 0 = NaN); an image with a NaN / Inf in it is NaN with rank -1.  The
    library's refusals are raised as ValueError before any launch.  No host read; the workspace is cached per shape and
    serves one stream at a time."""
    x, n, k, d, images = _particle_set(x, images)
    if k > PCA_MAX_K:
        raise ValueError(f"principal components take at most {PCA_MAX_K} particles per image (got {k})")
    if d < 1 or images > 65535 or d >= 2 ** 31:
        raise ValueError(f"principal components take 1 <= C H W < 2^31 and at most 65535 images (got {d}, {images})")
    q = pca_components(components)
    ws = _workspace("dpsx_pca_workspace_bytes", x.device, n, d, images)
    f = dict(dtype=torch.float32, device=x.device)
    dirs = torch.empty((images, q) + tuple(x.shape[1:]), **f)
    evals, coords, info = torch.empty((images, q), **f), torch.empty((images, k, q), **f), torch.empty((images, 4), **f)
    d2 = torch.empty((images, k, k), **f) if want_d2 else None
    check(lib().dpsx_pca_f32(ptr(x), q, ptr(dirs), ptr(evals), ptr(coords), ptr(info), ptr(d2), n, d, images, ptr(ws),
                             ws.numel(), _stream_arg(stream, x)), "dpsx_pca_f32")
    with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():    # the derived columns follow the launches
        var, explained = evals / float(k), evals / info[:, 0:1]
    res = {"dirs": dirs, "evals": evals, "var": var, "explained": explained, "coords": coords, "info": info}
    if want_d2:
        res["d2"] = d2
    return res


# ------------------------------------------------------------------ particle groups on streams
class ParticleGroups:
    """The N particles of a fused DPS loop as `groups` independent sub-batches, each with its own operator handle,
    residual scratch and HIP stream (an operator handle, its workspace and its tail counters serve ONE stream at a time).

    The three launches of a step depend on each other, the particles do not (no collective, no cross-particle term in
    reference gaussian_diffusion.py:207-257), and the counters say every tile kernel's load / compute / store phases add
    up inside one chain: side by side, the bandwidth-bound launch of one group fills the
    arithmetic-bound phase of another.  Per-particle results do not depend on the grouping, bit for bit.
    Used by `GaussianDiffusion.p_sample_loop` (sampler.particle_groups), the driver (--particle_groups) and bench.py.

    All groups' sample / gate / norm / g_model_out / x_next are contiguous particle slices of ONE full-batch StepBuffers
    (`self.full`): `self.full.norm` is the [N] distance vector and `self.x_next()` the [N, C, H, W] state, no copy."""

    def __init__(self, operator, n, c, h, w, device, groups, mask=None, like=None, record_streams=True, images=None):
        """record_streams=False: the caller keeps every tensor it hands to the launches alive until the groups are joined
        (bench.py's device-resident rings), so the per-launch `record_stream` calls (about 1 us of host time each) are
        skipped.
        images=M (> 1): a multi-image batch of M images x N / M particles: the groups hold whole images (groups <= M) and
        each group reads its own images' rows of a [M, ...] measurement (`y_rows`) and of a [M, 1, H, W] mask."""
        device = torch.device(device)
        self.record_streams = bool(record_streams)
        self.images = int(images) if images is not None and int(images) > 1 else None
        if self.images is None:
            groups = max(1, min(int(groups), max(n, 1)))
            self.sizes = [n // groups + (1 if j < n % groups else 0) for j in range(groups)]   # may differ by one particle
            self.rows = None
        else:
            M = self.images
            if n % M:
                raise ValueError(f"{n} particles do not split into {M} images")
            groups = max(1, min(int(groups), M))
            per_img = [M // groups + (1 if j < M % groups else 0) for j in range(groups)]
            first = [sum(per_img[:j]) for j in range(groups)]
            self.rows = [slice(f, f + k) for f, k in zip(first, per_img)]          # each group's images
            self.sizes = [k * (n // M) for k in per_img]
        self.n, self.shape = n, (n, c, h, w)
        self.starts = [sum(self.sizes[:j]) for j in range(groups)]
        self.slices = [slice(s, s + m) for s, m in zip(self.starts, self.sizes)]
        self.full = StepBuffers(None, n, c, h, w, device)
        probe = like if like is not None else self.full.sample
        self.handles = [operator.new_hip_handle(probe, mask=self._group_mask(j, mask)) for j in range(groups)]
        self.bufs = [StepBuffers(hd, m, c, h, w, device, parent=self.full, offset=s)
                     for hd, m, s in zip(self.handles, self.sizes, self.starts)]
        self.streams = [torch.cuda.Stream(device=device) for _ in range(groups)]
        self.device = device

    def __len__(self):
        return len(self.bufs)

    def _group_mask(self, j, mask):
        if mask is None or self.images is None or mask.shape[0] == 1:
            return mask
        if mask.shape[0] != self.images:
            raise ValueError(f"{mask.shape[0]} masks for {self.images} images")
        return mask[self.rows[j]]

    def y_rows(self, j, y):
        """group j's measurement: y itself (one broadcast row, or a single-image batch), else its images' rows"""
        if self.images is None or y.shape[0] == 1:
            return y
        if y.shape[0] != self.images:
            raise ValueError(f"measurement of {y.shape[0]} rows for {self.images} images")
        return y[self.rows[j]]

    # -- ordering against the caller's stream
    def fork(self, stream=None):
        """every group's stream waits for the work enqueued so far on `stream` (default: torch's current stream)"""
        cur = torch.cuda.current_stream(self.device) if stream is None else stream
        for s in self.streams:
            s.wait_stream(cur)

    def join(self, stream=None):
        """`stream` (default: torch's current stream) waits for every group's work"""
        cur = torch.cuda.current_stream(self.device) if stream is None else stream
        for s in self.streams:
            cur.wait_stream(s)

    def _slice(self, j, t):
        """the group's particles of a full-batch tensor (a contiguous view); a tensor that already has the group's
        size is taken as it is.  Tensors the caller allocates per step on its own stream are marked as in use by the
        group's stream (the caching allocator would otherwise hand their memory out again while the launch reads it)."""
        if t is None:
            return None
        if t.shape[0] == self.n and self.sizes[j] != self.n:
            v = t[self.slices[j]]
        elif t.shape[0] == self.sizes[j]:
            v = t
        else:
            raise ValueError(f"tensor of {t.shape[0]} particles handed to a group of {self.sizes[j]} (batch of {self.n})")
        if self.record_streams:
            v.record_stream(self.streams[j])
        return v

    # -- the three launches of group j, on its stream
    def step_fwd(self, j, x_t, model_out, noise=None, y=None, coefs=None, want_x0=True, rng=None):
        """rng= (instead of noise=): the record of the WHOLE batch; the group's slice start is added to its particle_base"""
        _noise_or_rng(noise, rng)
        step_fwd(self.handles[j], self.bufs[j], self._slice(j, x_t), self._slice(j, model_out), self._slice(j, noise),
                 self.y_rows(j, y), coefs, want_x0=want_x0, stream=self.streams[j],
                 rng=None if rng is None else rng.offset(self.starts[j]))

    def step_bwd(self, j, y, scale, power, coefs, g_x0_extra=None):
        step_bwd(self.handles[j], self.bufs[j], self.y_rows(j, y), scale, power, coefs,
                 g_x0_extra=self._slice(j, g_x0_extra), stream=self.streams[j])

    def step_update(self, j, g_unet, coefs):
        return step_update(self.bufs[j], self._slice(j, g_unet), coefs, stream=self.streams[j])

    def group_args(self, j, noise=None, y=None, rng=None):
        """what a caller that enqueues group j's launches itself passes to step_fwd / step_bwd / step_update*:
        -> (handle, buffers, stream, the group's noise rows, its measurement rows, the record offset to its first particle)
        of the full batch's noise / y / rng (each may be None)"""
        return (self.handles[j], self.bufs[j], self.streams[j], self._slice(j, noise),
                None if y is None else self.y_rows(j, y), None if rng is None else rng.offset(self.starts[j]))

    def x_next(self):
        """[N, C, H, W]: the state the groups' last step_update calls wrote (all groups flip together)"""
        flips = {b.flip for b in self.bufs}
        if len(flips) != 1:
            raise RuntimeError("the groups are not at the same step")
        return self.full.x_next[flips.pop() ^ 1]
