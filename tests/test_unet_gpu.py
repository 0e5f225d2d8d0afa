"""GPU suite (-m gpu): the denoiser on the device against the reference's UNet under shared synthetic weights.

The UNet runs through PyTorch-ROCm (MIOpen convolutions and GroupNorm, hipBLASLt, the attention backend torch picks,
the backward of the nearest upsample); none of it was ever compared with anything.  The truth is the float64 twin of
the REFERENCE's architecture in tests/golden/unet.npz (see tests/unet_ref.py, tests/test_unet_cpu.py); the gate is the
suite's TOL = 1e-5 rel-L2, where the reference's own fp32 (e_ref) sits at 7e-7 .. 1.8e-6 and a structural fault at
0.1 .. 1.  Every check prints `err`, `e_ref` and their ratio; profiles/unet_parity.txt holds the measured table.

Then the first tests whose cotangent goes through a denoiser that mixes pixels and channels: one conditioning call
against the reference's, and a free-running loop, fused launches against the per-op path.
"""
import contextlib

import numpy as np
import pytest
import torch

import unet_ref as U
from standin import rel_l2
from test_hip_parity import DEV, K, _sampler, dev, host, make_product_op  # noqa: F401 (K: fixture)

pytestmark = pytest.mark.gpu

_models = {}


def product(name):
    """the product's UNet with the shared weights, on the device (built once per variant)"""
    if name not in _models:
        from dps_ttc_amd.unet import create_model
        _models[name] = U.fill_weights(create_model(**U.config(name))).eval().to(DEV)
    return _models[name]


@pytest.fixture(scope="module")
def ref(golden):
    yield golden("unet")
    _models.clear()


def backend(which):
    if which == "default":
        return contextlib.nullcontext()
    from torch.nn.attention import SDPBackend, sdpa_kernel
    return sdpa_kernel(SDPBackend.MATH)


def run(name, n=None, only=None):
    x, t, w, labels = U.inputs(name, n)
    sl = slice(None) if only is None else slice(only, only + 1)
    to = lambda a: None if a is None else dev(a[sl])
    y, g = U.forward_and_vjp(product(name), to(x), to(t), to(w), to(labels))
    return host(y), host(g)


def check(ref, name, which, y, g):
    whole = U.stored_whole(name)
    bad = []
    for what, a, tag in (("out", y, "y"), ("grad", g, "g")):
        err = rel_l2(U.pick(f"{name}.{tag}", a, whole), ref[f"{name}.{tag}64"])
        e_ref = float(ref[f"{name}.e_ref_{what}"])
        line = f"unet {name:5s} gpu {which:7s} {what:4s}: err {err:.3e}  e_ref {e_ref:.3e}  ratio {err / e_ref:.2f}"
        print(line)
        if not err <= U.TOL:
            bad.append(line)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("which", ["default", "math"])
@pytest.mark.parametrize("name", U.CPU_VARIANTS)
def test_unet_gpu_matches_reference_float64(ref, name, which):
    """fp32 on the device, output and VJP against the float64 twin of the reference -- with the attention backend torch
    picks, and with the math backend forced: both have to pass"""
    with backend(which):
        y, g = run(name)
    check(ref, name, which, y, g)


def test_unet_gpu_ffhq_matches_reference_float64(ref):
    """configs/model_config.yaml as shipped (93.6 M parameters), one particle at 256 x 256"""
    y, g = run("FFHQ")
    check(ref, "FFHQ", "default", y, g)


@pytest.mark.parametrize("name", ["A", "B"])
def test_unet_gpu_particles_are_independent(ref, name):
    """Three particles in one batch against each particle alone, within the gate.  NOT bit for bit: MIOpen and
    hipBLASLt may pick other algorithms for another batch size, and both results are fp32 evaluations of the same
    function."""
    yb, gb = run(name, n=3)
    for i in range(3):
        y1, g1 = run(name, n=3, only=i)
        e_out, e_grad = rel_l2(yb[i:i + 1], y1), rel_l2(gb[i:i + 1], g1)
        print(f"unet {name:5s} gpu particle {i} of 3 against alone: out {e_out:.3e}  grad {e_grad:.3e}")
        assert e_out <= U.TOL and e_grad <= U.TOL, (name, i, e_out, e_grad)


def test_unet_gpu_conditioning_call_golden(K, ref):
    """The reference's conditioning call (`ps`, Gaussian blur, 64 x 64, N = 2) with a real denoiser, A64, through the
    product: p_sample + conditioning as in test_conditioning_per_call_golden.  Each field is gated at the gate it has
    there plus 4 x e_call, the call's own sensitivity to fp32-level denoiser error as measured on the reference alone
    (fp32 run against the run with the float64 twin as the model).  x0_hat is not bit-exact with a real denoiser; it is
    gated like `sample`."""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    from dps_ttc_amd.measurements import get_noise
    c = U.CALL
    op, fkw = make_product_op("gauss", hw=c["hw"])
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=c["sigma"]), scale=c["scale"])
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    model, y = product(c["variant"]), dev(ref["call.y"])
    base = {"x0_hat": 1e-6, "sample": 1e-6, "ret0": U.TOL, "ret1": U.TOL}
    bad = []
    for t in c["ts"]:
        _, _, x_prev0, noise = U.call_inputs(t)
        assert U.crc(x_prev0) == ref[f"call.t{t}.x_prev_crc"] and U.crc(noise) == ref[f"call.t{t}.noise_crc"]
        x_prev = dev(x_prev0).requires_grad_()
        out = smp.p_sample(model=model, x=x_prev, t=torch.tensor([t]), noise=dev(noise))
        got = {"x0_hat": host(out["pred_xstart"]).copy(), "sample": host(out["sample"]).copy()}
        ret = cm.conditioning(x_prev=x_prev, x_t=out["sample"], x_0_hat=out["pred_xstart"], measurement=y,
                              noisy_measurement=y, beta_scale=float(smp.betas[t]), t=t / 1000.0, **fkw)
        got["ret0"], got["ret1"] = host(ret[0]), host(ret[1])
        for f in U.CALL_FIELDS:
            got[f] = U.pick(f"call.t{t}", got[f], whole=(f == "ret1"))          # one set of positions per call
            e_call = float(ref[f"call.t{t}.e_call_{f}"])
            gate = base[f] + 4 * e_call
            err = rel_l2(got[f], ref[f"call.t{t}.{f}"])
            line = f"unet call t={t:3d} {f:6s}: err {err:.3e}  gate {gate:.3e} = {base[f]:.0e} + 4 x {e_call:.3e}"
            print(line)
            if not err <= gate:
                bad.append(line)
        # the guidance term alone, scale * grad = sample - ret0: about 1e-3 of `sample`, so ret0's gate would let a
        # gradient that is wrong by a percent through.  Each side of the comparison is a difference of two stored fp32
        # numbers of sample's size, rounded to 2^-24 relative each: that rounding, over the term's size, plus the
        # suite's gate for a gradient.
        gd, rd = got["sample"] - got["ret0"], ref[f"call.t{t}.sample"] - ref[f"call.t{t}.ret0"]
        size = np.linalg.norm(rd) / np.linalg.norm(ref[f"call.t{t}.sample"])
        gate, err = U.TOL + 4 * 2.0 ** -24 / size, rel_l2(gd, rd)
        line = f"unet call t={t:3d} sample - ret0: err {err:.3e}  gate {gate:.3e}  ({size:.3e} of sample)"
        print(line)
        if not (err <= gate and size > 1e-4):
            bad.append(line)
    assert not bad, "; ".join(bad)


def test_unet_gpu_loop_fused_matches_per_op(K, ref):
    """Free-running ddpm loop (5 steps, `ps`, Gaussian blur, 64 x 64, N = 2) with A64 as the denoiser: the fused
    launches against the per-op autograd path (a foreign callable), as in test_ttc_ddim_fused_matches_per_op.  The
    first loop whose g_model_out goes through a VJP that is not diagonal; final image and last norm within 1e-4, the
    gate of test_base_loop_golden."""
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise
    c = U.CALL
    op, _ = make_product_op("gauss", hw=c["hw"])
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=c["sigma"]), scale=c["scale"])
    model, y = product(c["variant"]), dev(ref["call.y"])
    x_start = dev(U.call_inputs(c["ts"][0])[2])

    def per_op(**kw):
        """the base loop takes a callable it does not know as the reference's loop takes every callable: the first
        return value is the gradient, and the loop subtracts it from the sample.  `ps` returns the guided sample."""
        sample = kw["x_t"].detach().clone()
        guided, norm, net_scaling = cm.conditioning(**kw)
        return sample - guided.detach(), norm, net_scaling

    res = []
    for fused in (True, False):
        smp = _sampler("ddpm", "5")
        cond = cm.conditioning if fused else per_op
        assert (smp._fusion_plan(cond, x_start) is not None) == fused
        torch.manual_seed(5)
        img, dist, _ = smp.p_sample_loop(model=model, x_start=x_start.clone().requires_grad_(), measurement=y,
                                         measurement_cond_fn=cond, record=False, save_root=None)
        res.append((host(img).copy(), host(dist).copy()))
    e_img, e_norm = rel_l2(res[0][0], res[1][0]), rel_l2(res[0][1], res[1][1])
    print(f"unet loop fused against per-op: final image {e_img:.3e}  last norm {e_norm:.3e}")
    assert np.isfinite(res[0][0]).all() and rel_l2(res[0][0], host(x_start)) > 0.1
    assert e_img <= 1e-4 and e_norm <= 1e-4
