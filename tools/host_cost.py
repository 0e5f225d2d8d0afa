#!/usr/bin/env python3
"""Host cost of enqueueing one fused DPS step (three launches) -- with the current-stream lookup, inside a stream context,
and with the stream handed to the launches explicitly -- at a particle count small enough that the GPU is never the limit;
plus a cProfile of the plain form.   python tools/host_cost.py
--loop: the host cost per step of GaussianDiffusion.p_sample_loop instead (`ps`, a two-multiply stand-in for the UNet, 100
steps, 3 particles: the device is never the limit), as one chain and as --groups particle groups, three rounds each."""
import os, sys, time
sys.path.insert(0, os.environ.get("GRAFT_REPO_ROOT", "."))
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import torch, bench
from dps_ttc_amd import kernels
from dps_ttc_amd.gaussian_diffusion import create_sampler
dev = torch.device("cuda", 0)
smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type="learned_range",
                     dynamic_threshold=False, clip_denoised=True, rescale_timesteps=True, timestep_respacing="")
n = 3
op, fkw = bench.build_operator("gaussian_blur", dev)


def loop_cost(groups):
    from dps_ttc_amd.condition_methods import get_conditioning_method
    from dps_ttc_amd.measurements import get_noise

    class Model(torch.nn.Module):                      # [N, 2C, H, W] out, a graph back to x: the step's host work, no more
        def forward(self, x, t):
            return torch.cat([x * 0.5, x * 0.1], dim=1)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="100")
    cm = get_conditioning_method("ps", op, get_noise("gaussian", sigma=0.05), scale=0.3)
    x_t, ring, truth, mn = bench.synth_inputs(n, 2, dev, 1)
    y = (op.forward(truth.to(dev)).detach() + mn.to(dev)[..., :256, :256]).contiguous()
    model = Model().to(dev)
    for g in (1, groups):
        smp.particle_groups = g
        rounds = []
        for r in range(4):                             # the first trajectory builds the buffers: not counted
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            smp.p_sample_loop(model=model, x_start=x_t, measurement=y, measurement_cond_fn=cm.conditioning, record=False,
                              save_root=None)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if r:
                rounds.append((t1 - t0) / smp.num_timesteps * 1e6)
        print("loop groups=%d host %.1f us/step  (rounds %s)" % (g, sum(rounds) / len(rounds),
                                                               " / ".join("%.1f" % v for v in rounds)), flush=True)


if "--loop" in sys.argv:
    loop_cost(int(sys.argv[sys.argv.index("--groups") + 1]) if "--groups" in sys.argv else 3)
    sys.exit(0)
x_t, ring, truth, mn = bench.synth_inputs(n, 2, dev, 1)
y = (op.forward(truth.to(dev)).detach() + mn.to(dev)[..., :256, :256]).contiguous()
h = op.hip_handle(x_t); buf = kernels.StepBuffers(h, n, 3, 256, 256, dev)
ck = smp.step_coefs[500]; s = ring[0]
st = torch.cuda.Stream()
def step(x):
    kernels.step_fwd(h, buf, x, s["model_out"], s["noise"], y, ck, want_x0=False)
    kernels.step_bwd(h, buf, y, 0.3, 1, ck)
    return kernels.step_update(buf, s["g_unet"], ck)
def step_explicit(x):
    kernels.step_fwd(h, buf, x, s["model_out"], s["noise"], y, ck, want_x0=False, stream=st)
    kernels.step_bwd(h, buf, y, 0.3, 1, ck, stream=st)
    return kernels.step_update(buf, s["g_unet"], ck, stream=st)
for mode in ("plain", "with_stream", "explicit"):
    x = x_t
    for _ in range(50): x = step(x)
    torch.cuda.synchronize()
    K = 3000
    t0 = time.perf_counter()
    for _ in range(K):
        if mode == "plain": x = step(x)
        elif mode == "explicit": x = step_explicit(x)
        else:
            with torch.cuda.stream(st): x = step(x)
    t1 = time.perf_counter(); torch.cuda.synchronize(); t2 = time.perf_counter()
    print(mode, "enqueue %.1f us/step" % ((t1 - t0) / K * 1e6), "total %.1f us/step" % ((t2 - t0) / K * 1e6))
import cProfile, pstats
pr = cProfile.Profile(); pr.enable()
for _ in range(2000): x = step(x)
pr.disable(); torch.cuda.synchronize()
pstats.Stats(pr).sort_stats("tottime").print_stats(12)
