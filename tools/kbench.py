#!/usr/bin/env python3
"""Kernel micro-bench: time each launch of the fused DPS step (and the plain operator calls) in isolation.

    python tools/kbench.py [--operator gaussian_blur] [--particles 64] [--reps 30] [--only fwd,bwd,upd,op,adj]
    python tools/kbench.py --operator super_resolution --particles 16 --images 4     (multi-image batches)

Prints one line per launch: avg / min microseconds and achieved GB/s against the algorithmic bytes
(SURVEY.md 8d).  Used under rocprofv3 for the per-kernel profiles in profiles/.
    python tools/kbench.py --resample [--images M]                                    (the resampling step, 256^2)
--images M: the step's three launches (fwd, bwd, upd) for a multi-image batch of M images x --particles K with one
measurement (and inpainting mask) per image, as ONE sequence of N = M K particles, against M sequential K-particle
sequences with y[m] (and mask[m]) in the same process: us per step and particle-steps per second of both.
--resample: the resampling step of ttc_ddim on [N, 3, 256, 256] particles, its forms alternated in one process:
(a) torch.multinomial + its [N]-sized glue + two gathers (resample_draw = "multinomial", the non-parity branch),
(b) kernels.resample_draw + two gathers, (c) the fused kernels.resample, (d-f) the fused scheme / ESS launch
(dpsx_resample_seg_ex_f32: multinomial tau = 1, systematic tau = 1, systematic tau = 0.5); single image at
K = 16 / 64 / 512 and M (default 4) images x K = 16, there also against M single-image calls of each form.
    python tools/kbench.py --noise-draw                                               (the step noise, 256^2, N = --particles)
--noise-draw: K1 of every operator and the single-state search step with the step noise drawn three ways, alternated in
one process: (a) torch.randn + the pointer launch (noise_draw = "torch"), (b) kernels.randn (dpsx_randn_f32) + the pointer
launch, (c) the draw inside the launch (step_fwd(rng=) / search_step_one(rng=)); a route without an in-kernel form is
marked and its (c) is the front end's fallback, which is (b).
    python tools/kbench.py --cg                                                       (the CG data-consistency step, 256^2)
    python tools/kbench.py --pgdm                                                     (cg_pullback beside cg_step, 256^2)
--cg: OpHandle.cg_step at iters = 1 and 5 beside the fused `ps` step (K1 + K2 + K3) and the plain A / A^T / K3 launches,
N = 64 and 16, Gaussian / motion / SR x4 / inpainting, 3 x --reps repetitions alternated in one process.  Per launch: the
step's time over its enqueued launches (5 + 5 iters - 1).  The vector side of one middle iteration (||t||^2, the d / r
update, the p update: (9 + m / e) P by shape arithmetic) is priced as (t(5) - t(1)) / 4 - t(A) - t(A^T), beside K3's rate.
    python tools/kbench.py --smc                                                      (the particle weights' launches, 256^2)
--smc: K3 beside the launch that also sums the proposal correction, N = 64 and 16, Gaussian sigma = 3, 3 x --reps repetitions
alternated in one process: (a) K3 alone (4 P by shape arithmetic), (b) kernels.step_update_corr with a noise pointer (6 P),
(c) the same with rng= (5 P), (d) K3 + the correction as torch ops + a torch sum, and kernels.smc_accum alone.  Rates are
against the bytes by shape arithmetic; (b) and (c) also as a fraction of K3's rate in the same run.
    python tools/kbench.py --dsg                                                      (spherical-Gaussian guidance, 256^2)
--dsg: K3 beside kernels.step_update_dsg's two launches, N = 64 and 16, Gaussian sigma = 3, 3 x --reps repetitions alternated
in one process: (a) K3 alone (4 P), (b) step_update_corr with a noise pointer (6 P), (c) step_update_dsg with a noise pointer
(stats 4 P + apply 6 P), (d) the same with rng= (3 P + 5 P).  Per form: the time as a multiple of K3's and the rate against
the bytes by shape arithmetic as a fraction of K3's rate, all from the same run.
    python tools/kbench.py --dpmpp                                                    (the DPM-Solver++(2M) update, 256^2)
--dpmpp: K3 beside kernels.step_update_ms, N = 64 and 16, Gaussian sigma = 3, 3 x --reps repetitions alternated in one
process: (a) K3 alone (4 P), (b) step_update_ms with c != 0 (6 P), (c) the same with c = 0 (4 P), (d) K3 + the correction as
two torch ops, and K1 without / with the x0_hat store.  (b) and (c): the time as a multiple of K3's and the rate against the
bytes by shape arithmetic as a fraction of K3's rate, all from the same run.
    python tools/kbench.py --metrics                                                  (per-path PSNR / SSIM, 256^2)
--metrics: the per-path metrics of [N, 3, 256, 256] particles, N = 64 with M = 1 and M = 4 labels and N = 512 with M = 1,
3 x --reps repetitions alternated in one process: (a) the driver's per-particle metrics.compute_psnr loop with its host
read (PSNR only), (b) PSNR and SSIM as batched torch ops (five depthwise conv2d with the 11 x 11 window, the elementwise map,
the means), (c) kernels.image_metrics with all three outputs and its PSNR-only call.  (b) is the yardstick of (c).
    python tools/kbench.py --repulse                                                  (particle repulsion, 256^2)
--repulse: [M K, 3, 256, 256] particles, M = 4 x K = 16, M = 1 x K = 64 and M = 1 x K = 512, 3 x --reps repetitions alternated
in one process: (a) kernels.pairwise_sqdist (the pair partials and the finisher's distance half), (b) kernels.repulse (all
three launches), (c) the same mathematics as torch ops (torch.cdist on the flattened particles, exp, one matmul), (d) K3 at the
same N for scale.  (a) and (b) are stated against both floors by shape arithmetic -- bytes at 8 TB/s with every particle moved
once, fp32 operations at the vector peak -- with the one that binds and how often the tiling fetches a particle.  The three
launches apart come from a kernel trace (rocprofv3 --kernel-trace) of the same call in a run of its own.
    python tools/kbench.py --ensemble                                                 (ensemble statistics, 256^2)
--ensemble: [M K, 3, 256, 256] particles and M labels, M = 4 x K = 16, M = 1 x K = 64 and M = 1 x K = 512, 3 x --reps
repetitions alternated in one process: (a) kernels.ensemble_stats with the label (stream + finisher) and (a') with weights too
(all three launches), (b) torch ops giving the same outputs (var_mean; cumsum / n - y, squared, mean), (c) the byte floor
((K + 1) D 4 read + 2 D 4 written per image at 8 TB/s), (d) K3 at the same N for scale: (a)'s rate against its floor's bytes
is also stated as a fraction of K3's rate in the same run.
    python tools/kbench.py --quantiles                                                (order statistics, 256^2)
--quantiles: the same three shapes, 3 x --reps repetitions alternated in one process: (a) kernels.order_stats with the label
(quantiles 5 / 50 / 95 %, rank histogram, CRPS: element pass + finisher) and (a') without the label and with one probability
(the loads and the sort alone, so the difference to (a) is the sweep's and the emit's), (b) the same outputs as torch ops
(torch.sort along the particle axis, the gathers and the interpolation, the rank count, the sorted-order CRPS), (c) the byte
floor ((K + 1) D 4 read once per image at 8 TB/s), (d) K3 at the same N for scale.
    python tools/kbench.py --pca [--pca-shape I]                                      (principal components, 256^2)
--pca: M = 4 x K = 16, K = 64, K = 128 (or shape I of them alone), q = 4, particles = base + 6 planted directions + noise,
3 x --reps repetitions alternated in one process: (a) kernels.particle_pca (four launches), (b) kernels.pairwise_sqdist (its
first two), (c) the same computation as torch ops (centre, X X^T, torch.linalg.eigh, the top q, one matmul), (d) K3 at the
same N for scale.  The launches apart come from a kernel trace of the same run (rocprofv3 --kernel-trace -d DIR -- ...):
    python tools/kbench.py --pca-trace DIR --pca-shape I
prints every launch's average and the projection's rate against its (K + q) D 4 bytes per image beside K3's 4 P per particle.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--operator", default="gaussian_blur")
    ap.add_argument("--particles", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", default="fwd,bwd,upd,op,adj,score")
    ap.add_argument("--sigma", type=float, default=3.0, help="gaussian_blur only: another radius bucket")
    ap.add_argument("--norm-in-fwd", action="store_true", help="K1 finishes the norm itself (last block of a particle)")
    ap.add_argument("--no-x0", action="store_true", help="K1 does not write x0_hat out (blur / resize; the `ps` loop's setting)")
    ap.add_argument("--images", type=int, default=None, help="time the multi-image step of M images x --particles")
    ap.add_argument("--resample", action="store_true", help="time the resampling step (multinomial / draw + gathers / fused)")
    ap.add_argument("--noise-draw", action="store_true", help="time the step noise: torch.randn / device fill / in-kernel draw")
    ap.add_argument("--cg", action="store_true", help="time the CG data-consistency step beside the fused ps step")
    ap.add_argument("--pgdm", action="store_true", help="time OpHandle.cg_pullback beside cg_step (iters = 5) and K3")
    ap.add_argument("--smc", action="store_true", help="time K3 beside step_update_corr (pointer / rng / torch ops) and smc_accum")
    ap.add_argument("--dsg", action="store_true", help="time step_update_dsg's two launches (pointer / rng) beside K3")
    ap.add_argument("--dpmpp", action="store_true", help="time step_update_ms (c != 0 / c = 0 / torch ops) beside K3, and K1's x0_hat store")
    ap.add_argument("--metrics", action="store_true", help="time per-path PSNR / SSIM: host loop / torch ops / image_metrics")
    ap.add_argument("--repulse", action="store_true", help="time particle repulsion: the distances / the whole call / torch ops / K3")
    ap.add_argument("--ensemble", action="store_true", help="time the ensemble statistics: the call / torch ops / the byte floor / K3")
    ap.add_argument("--quantiles", action="store_true", help="time the order statistics: the call / torch ops / the byte floor / K3")
    ap.add_argument("--pca", action="store_true", help="time the principal components: the call / the distances / torch ops / K3")
    ap.add_argument("--pca-shape", type=int, default=None, help="--pca / --pca-trace: one of the three shapes (0, 1, 2)")
    ap.add_argument("--pca-trace", default=None, metavar="DIR", help="the per-launch table from a kernel trace of a --pca run")
    args = ap.parse_args()
    if args.pca_trace:
        return pca_trace(args)
    if args.pca:
        return pca_step(args)
    if args.quantiles:
        return quantiles_step(args)
    if args.ensemble:
        return ensemble_step(args)
    if args.repulse:
        return repulse_step(args)
    if args.metrics:
        return metrics_step(args)
    if args.dpmpp:
        return dpmpp_step(args)
    if args.dsg:
        return dsg_step(args)
    if args.smc:
        return smc_step(args)
    if args.pgdm:
        return pgdm_step(args)
    if args.cg:
        return cg_step(args)
    if args.noise_draw:
        return noise_draw(args)
    if args.resample:
        return resample_step(args)
    if args.images is not None:
        return multi_image(args)
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    n = args.particles
    op, fkw = bench.build_operator(args.operator, dev, sigma=args.sigma)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    x_t, ring, truth, meas_noise = bench.synth_inputs(n, 2, dev, 1234)
    yy = op.forward(truth.to(dev), **fkw).detach()
    mn = meas_noise.to(dev)
    if mn.shape[-1] < yy.shape[-1]:                      # phase retrieval measures on the oversampled grid
        mn = 0.05 * torch.randn(yy.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    y = (yy + mn[..., :yy.shape[-2], :yy.shape[-1]]).contiguous()
    handle = op.hip_handle_for(fkw["mask"]) if args.operator == "inpainting" else op.hip_handle(x_t)
    buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
    ck = smp.step_coefs[500]
    P = bench.P_BYTES
    # one byte table for bench.py and this tool (bench.algo_p): the configuration launched (x0_hat store on / off)
    tbl = bench.algo_p(args.operator, x0_store=not args.no_x0)["algorithmic"]
    rho = bench.RHO[args.operator]
    u = torch.randn((n,) + tuple(y.shape[1:]), device=dev)
    cases = {
        "fwd": (lambda i: kernels.step_fwd(handle, buf, x_t, ring[i % 2]["model_out"], ring[i % 2]["noise"], y, ck,
                                           finalize_norm=args.norm_in_fwd, want_x0=not args.no_x0), tbl["fwd"] * P),
        # as in the loop: the norm is finalised from the forward half's partials (--norm-in-fwd: by K1's own tail)
        "bwd": (lambda i: (setattr(buf, "norm_ready", args.norm_in_fwd), kernels.step_bwd(handle, buf, y, 0.3, 1, ck)),
                tbl["bwd"] * P),
        "upd": (lambda i: kernels.step_update(buf, ring[i % 2]["g_unet"], ck), tbl["upd"] * P),
        "op": (lambda i: handle.forward(x_t), (1 + rho) * P),
        "adj": (lambda i: handle.adjoint(u, x=x_t, in_hw=(256, 256)), (1 + rho) * P),
        "score": (lambda i: handle.score(x_t, y), 1 * P),
    }
    cases["fwd"][0](0)           # partial sums for a stand-alone "bwd"
    for name in args.only.split(","):
        fn, bytes_pp = cases[name]
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        ts = np.array([a.elapsed_time(b) for a, b in evs]) * 1e3
        label = f", x0_hat store {'off' if args.no_x0 else 'on'}" if name in ("fwd", "bwd") else ""
        # the rate is on the bytes the launch MOVES (PMC, profiles/traffic.json: N = 64, x0_hat store off, sigma = 3) where
        # they are on file -- the survey's compulsory bytes include streams this design never writes (the zero variance
        # half of g_model_out, grad_x_direct), so priced on them a short launch would read as faster than the memory
        moved = bench.load_traffic(args.operator).get(name) if (args.no_x0 and args.sigma == 3.0 and not args.norm_in_fwd) else None
        if moved:
            moved = moved * n / 64.0
            print(f"{name:6s} avg {ts.mean():8.1f} us  min {ts.min():8.1f} us   {moved / ts.mean() / 1e3:8.1f} GB/s moved "
                  f"({moved / n / P:.2f} P/particle by PMC; algorithmic {bytes_pp / P:.2f} P{label})", flush=True)
        else:
            print(f"{name:6s} avg {ts.mean():8.1f} us  min {ts.min():8.1f} us   "
                  f"{bytes_pp * n / ts.mean() / 1e3:8.1f} GB/s algorithmic ({bytes_pp / P:.2f} P/particle{label})", flush=True)


def multi_image(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    M, k = max(1, args.images), args.particles
    n = M * k
    op, fkw = bench.build_operator(args.operator, dev, sigma=args.sigma)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    x_t, ring, truth, _ = bench.synth_inputs(n, 2, dev, 1234)
    # M different images (shifted copies of the synthetic truth) and, for inpainting, M different masks
    masks = torch.cat([fkw["mask"].roll(13 * m, dims=-1) for m in range(M)]).contiguous() if "mask" in fkw else None
    ys = []
    for m in range(M):
        kw = {} if masks is None else {"mask": masks[m:m + 1]}
        ys.append(op.forward(truth.to(dev).roll(7 * m, dims=-1), **kw).detach())
    y = torch.cat(ys).contiguous()
    ck = smp.step_coefs[500]
    want_x0 = not args.no_x0

    def new_handle(mask_rows, x):
        return kernels.OpHandle.mask(mask_rows, dev) if mask_rows is not None else op.new_hip_handle(x)

    # one sequence of N = M K particles
    h_all = new_handle(masks, x_t)
    buf_all = kernels.StepBuffers(h_all, n, 3, 256, 256, dev)
    # M sequences of K particles: own handle and buffers per image (particle slices of the same inputs)
    hs = [new_handle(None if masks is None else masks[m:m + 1], x_t[:k]) for m in range(M)]
    bufs = [kernels.StepBuffers(hs[m], k, 3, 256, 256, dev) for m in range(M)]
    sl = [slice(m * k, (m + 1) * k) for m in range(M)]
    xs = [x_t[s].contiguous() for s in sl]
    rs = [[{key: r[key][s].contiguous() for key in ("model_out", "noise", "g_unet")} for s in sl] for r in ring]

    def one(i):
        r = ring[i % 2]
        kernels.step_fwd(h_all, buf_all, x_t, r["model_out"], r["noise"], y, ck, want_x0=want_x0)
        kernels.step_bwd(h_all, buf_all, y, 0.3, 1, ck)
        kernels.step_update(buf_all, r["g_unet"], ck)

    def seq(i):
        for m in range(M):
            r = rs[i % 2][m]
            kernels.step_fwd(hs[m], bufs[m], xs[m], r["model_out"], r["noise"], y[m:m + 1], ck, want_x0=want_x0)
            kernels.step_bwd(hs[m], bufs[m], y[m:m + 1], 0.3, 1, ck)
            kernels.step_update(bufs[m], r["g_unet"], ck)

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    res = {}
    for rep in range(3):                           # alternated: both forms see the same box state
        for name, fn in (("one", one), ("seq", seq)):
            res.setdefault(name, []).append(timed(fn))
    for name, label in (("one", f"one sequence of N = {n}"), ("seq", f"{M} sequences of K = {k}")):
        ts = np.concatenate(res[name])
        print(f"images {args.operator} M={M} K={k} {label:28s} avg {ts.mean():8.1f} us/step  min {ts.min():8.1f}  "
              f"{n / ts.mean():8.3f} M particle-steps/s (x0_hat store {'off' if args.no_x0 else 'on'})", flush=True)


def cg_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    P = bench.P_BYTES
    rho = 0.05 ** 2 / float(ck.b) ** 2                    # the method's default: rho_scale = 1, sigma_n = 0.05

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for n in (64, 16):
        for name in ("gaussian_blur", "motion_blur", "super_resolution", "inpainting"):
            op, fkw = bench.build_operator(name, dev, sigma=args.sigma)
            x_t, ring, truth, meas_noise = bench.synth_inputs(n, 2, dev, 1234)
            yy = op.forward(truth.to(dev), **fkw).detach()
            y = (yy + meas_noise.to(dev)[..., :yy.shape[-2], :yy.shape[-1]]).contiguous()
            handle = op.hip_handle_for(fkw["mask"]) if name == "inpainting" else op.hip_handle(x_t)
            buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
            u = torch.randn((n,) + tuple(y.shape[1:]), device=dev)
            x0_hat = truth.to(dev).expand(n, -1, -1, -1).contiguous()
            x0_hat = (x0_hat + 0.3 * torch.randn_like(x0_hat)).clamp_(-1, 1)

            def ps(i):
                r = ring[i % 2]
                kernels.step_fwd(handle, buf, x_t, r["model_out"], r["noise"], y, ck, want_x0=False)
                kernels.step_bwd(handle, buf, y, 0.3, 1, ck)
                kernels.step_update(buf, r["g_unet"], ck)

            ps(0)
            forms = {"ps": ps,
                     "cg1": lambda i: handle.cg_step(x0_hat, buf.sample, y, rho, 1, ck),
                     "cg5": lambda i: handle.cg_step(x0_hat, buf.sample, y, rho, 5, ck),
                     "A": lambda i: handle.forward(x_t),
                     "At": lambda i: handle.adjoint(u, x=x_t, in_hw=(256, 256)),
                     "K3": lambda i: kernels.step_update(buf, ring[i % 2]["g_unet"], ck)}
            res = {}
            for rep in range(3):                       # alternated: every form sees the same box state
                for key, fn in forms.items():
                    res.setdefault(key, []).append(timed(fn))
            t = {key: float(np.concatenate(v).mean()) for key, v in res.items()}
            lo = {key: float(np.concatenate(v).min()) for key, v in res.items()}
            m_over_e = y[0].numel() / x_t[0].numel()
            vec_us = (t["cg5"] - t["cg1"]) / 4 - t["A"] - t["At"]
            vec_bytes = (9 + m_over_e) * P * n
            k3_bytes = bench.algo_p(name, x0_store=False)["algorithmic"]["upd"] * P * n
            tag = f"cg {name:16s} N={n:2d}"
            runs = {key: " / ".join(f"{r.mean():.1f}" for r in v) for key, v in res.items()}
            print(f"{tag} ps step (K1+K2+K3) avg {t['ps']:8.1f} us  min {lo['ps']:8.1f}  (runs {runs['ps']})", flush=True)
            for it, key in ((1, "cg1"), (5, "cg5")):
                launches = 5 + 5 * it - 1
                print(f"{tag} cg_step iters={it}     avg {t[key]:8.1f} us  min {lo[key]:8.1f}  (runs {runs[key]})   {launches:2d} launches, "
                      f"{t[key] / launches:6.1f} us each   {t[key] / t['ps']:5.2f} x the ps step", flush=True)
            print(f"{tag} A {t['A']:7.1f} us  A^T {t['At']:7.1f} us  K3 {t['K3']:7.1f} us = {k3_bytes / t['K3'] / 1e3:7.1f} GB/s"
                  f"   vector side of one iteration {vec_us:7.1f} us = {vec_bytes / max(vec_us, 1e-3) / 1e3:7.1f} GB/s "
                  f"({9 + m_over_e:.2f} P/particle) = {vec_bytes / max(vec_us, 1e-3) / (k3_bytes / t['K3']):4.2f} x K3's rate",
                  flush=True)


def pgdm_step(args):
    """OpHandle.cg_pullback beside OpHandle.cg_step at iters = 5 (the chains differ in the last launch only: k_cg_pullback
    in k_cg_final's place) and K3, 3 x --reps alternated.  The last launch alone is the difference of the iters = 1 chains
    from their common part, so it is read from a kernel trace (rocprofv3 --kernel-trace --stats) of this same run instead:
    bytes per particle 3.25 P with d_out off (d, p, the gate; g_eps), K3's from bench.algo_p."""
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    P = bench.P_BYTES
    rho, gain = kernels.pgdm_scalars(smp.alphas_cumprod[500], smp.alphas_cumprod_prev[500], smp._pgdm_record(500)[:5], 0.05)

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for n in (64, 16):
        for name in ("gaussian_blur", "motion_blur", "super_resolution", "inpainting"):
            op, fkw = bench.build_operator(name, dev, sigma=args.sigma)
            x_t, ring, truth, meas_noise = bench.synth_inputs(n, 2, dev, 1234)
            yy = op.forward(truth.to(dev), **fkw).detach()
            y = (yy + meas_noise.to(dev)[..., :yy.shape[-2], :yy.shape[-1]]).contiguous()
            handle = op.hip_handle_for(fkw["mask"]) if name == "inpainting" else op.hip_handle(x_t)
            buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
            x0_hat, sample, inside = kernels.posterior_fwd(x_t, ring[0]["model_out"], ring[0]["noise"], ck, want_inside=True)
            buf.sample.copy_(sample)
            forms = {"cg5": lambda i: handle.cg_step(x0_hat, sample, y, rho, 5, ck),
                     "pgdm5": lambda i: handle.cg_pullback(x0_hat, inside, y, rho, 5, gain),
                     "K3": lambda i: kernels.step_update(buf, ring[i % 2]["g_unet"], ck)}
            res = {}
            for rep in range(3):                       # alternated: every form sees the same box state
                for key, fn in forms.items():
                    res.setdefault(key, []).append(timed(fn))
            t = {key: float(np.concatenate(v).mean()) for key, v in res.items()}
            lo = {key: float(np.concatenate(v).min()) for key, v in res.items()}
            runs = {key: " / ".join(f"{r.mean():.1f}" for r in v) for key, v in res.items()}
            spread = max(max(r.mean() for r in res[k]) - min(r.mean() for r in res[k]) for k in ("cg5", "pgdm5"))
            k3_bytes = bench.algo_p(name, x0_store=False)["algorithmic"]["upd"] * P * n
            tag = f"pgdm {name:16s} N={n:2d}"
            for key, label in (("cg5", "cg_step     iters=5"), ("pgdm5", "cg_pullback iters=5")):
                print(f"{tag} {label} avg {t[key]:8.1f} us  min {lo[key]:8.1f}  (runs {runs[key]})", flush=True)
            print(f"{tag} cg_pullback - cg_step {t['pgdm5'] - t['cg5']:+7.1f} us (the rounds' spread {spread:.1f} us)   "
                  f"K3 {t['K3']:7.1f} us = {k3_bytes / t['K3'] / 1e3:7.1f} GB/s   inside: {100 * float(inside.float().mean()):.1f} % "
                  f"of the elements", flush=True)


def smc_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    P = bench.P_BYTES
    ratio, lo_log, hi_log = -float(ck.a) / float(ck.b), float(ck.min_log), float(ck.max_log)

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for n in (64, 16):
        op, fkw = bench.build_operator("gaussian_blur", dev, sigma=args.sigma)
        x_t, ring, truth, meas_noise = bench.synth_inputs(n, 2, dev, 1234)
        yy = op.forward(truth.to(dev), **fkw).detach()
        y = (yy + meas_noise.to(dev)[..., :yy.shape[-2], :yy.shape[-1]]).contiguous()
        handle = op.hip_handle(x_t)
        buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
        st = kernels.SmcState(n, (3, 256, 256), dev)
        r0 = ring[0]
        kernels.step_fwd(handle, buf, x_t, r0["model_out"], r0["noise"], y, ck, want_x0=False)     # sample, g_model_out
        kernels.step_bwd(handle, buf, y, 0.3, 1, ck)
        rng = kernels.Rng(7, 500)

        def torch_ops(i):
            r = ring[i % 2]
            kernels.step_update(buf, r["g_unet"], ck)
            s = ratio * buf.g_model_out[:, :3] + r["g_unet"]
            frac = (r["model_out"][:, 3:] + 1.0) * 0.5
            q = s / torch.exp(0.5 * (frac * hi_log + (1.0 - frac) * lo_log))
            return (q * (r["noise"] - 0.5 * q)).flatten(1).sum(dim=1)

        forms = {"a K3": lambda i: kernels.step_update(buf, ring[i % 2]["g_unet"], ck),
                 "b update_corr, noise pointer": lambda i: kernels.step_update_corr(
                     buf, ring[i % 2]["g_unet"], ck, ring[i % 2]["model_out"], noise=ring[i % 2]["noise"], state=st),
                 "c update_corr, rng": lambda i: kernels.step_update_corr(
                     buf, ring[i % 2]["g_unet"], ck, ring[i % 2]["model_out"], rng=rng, state=st),
                 "d K3 + torch ops + torch sum": torch_ops,
                 "smc_accum": lambda i: kernels.smc_accum(st, buf.norm)}
        nbytes = {"a K3": 4 * P * n, "b update_corr, noise pointer": 6 * P * n, "c update_corr, rng": 5 * P * n}
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for key, fn in forms.items():
                res.setdefault(key, []).append(timed(fn))
        k3 = nbytes["a K3"] / float(np.concatenate(res["a K3"]).mean())
        for key in forms:
            ts = np.concatenate(res[key])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[key])
            rate = ""
            if key in nbytes:
                bps = nbytes[key] / ts.mean()
                rate = f"  {bps / 1e3:7.1f} GB/s ({nbytes[key] / n / P:.0f} P/particle) = {bps / k3:4.2f} x K3's rate"
            print(f"smc 256^2 N={n:2d} {key:30s} avg {ts.mean():8.1f} us  min {ts.min():8.1f}  (runs {runs}){rate}", flush=True)
        del buf, st, handle, op


def dsg_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    P = bench.P_BYTES

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for n in (64, 16):
        op, fkw = bench.build_operator("gaussian_blur", dev, sigma=args.sigma)
        x_t, ring, truth, meas_noise = bench.synth_inputs(n, 2, dev, 1234)
        yy = op.forward(truth.to(dev), **fkw).detach()
        y = (yy + meas_noise.to(dev)[..., :yy.shape[-2], :yy.shape[-1]]).contiguous()
        handle = op.hip_handle(x_t)
        buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
        st = kernels.SmcState(n, (3, 256, 256), dev)
        stats = buf.dsg_stats()
        r0 = ring[0]
        kernels.step_fwd(handle, buf, x_t, r0["model_out"], r0["noise"], y, ck, want_x0=False)     # sample, g_model_out
        kernels.step_bwd(handle, buf, y, 1.0, 1, ck)
        rng = kernels.Rng(7, 500)
        forms = {"a K3": lambda i: kernels.step_update(buf, ring[i % 2]["g_unet"], ck),
                 "b update_corr, noise pointer": lambda i: kernels.step_update_corr(
                     buf, ring[i % 2]["g_unet"], ck, ring[i % 2]["model_out"], noise=ring[i % 2]["noise"], state=st),
                 "c update_dsg, noise pointer": lambda i: kernels.step_update_dsg(
                     buf, ring[i % 2]["g_unet"], ck, ring[i % 2]["model_out"], 0.1, noise=ring[i % 2]["noise"], stats=stats),
                 "d update_dsg, rng": lambda i: kernels.step_update_dsg(
                     buf, ring[i % 2]["g_unet"], ck, ring[i % 2]["model_out"], 0.1, rng=rng, stats=stats)}
        # bytes by shape arithmetic: stats reads 4 P (3 P with rng), apply reads 5 P (4 P) and writes 1 P
        nbytes = {"a K3": 4 * P * n, "b update_corr, noise pointer": 6 * P * n, "c update_dsg, noise pointer": 10 * P * n,
                  "d update_dsg, rng": 8 * P * n}
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for key, fn in forms.items():
                res.setdefault(key, []).append(timed(fn))
        t_k3 = float(np.concatenate(res["a K3"]).mean())
        k3 = nbytes["a K3"] / t_k3
        for key in forms:
            ts = np.concatenate(res[key])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[key])
            bps = nbytes[key] / ts.mean()
            print(f"dsg 256^2 N={n:2d} {key:30s} avg {ts.mean():8.1f} us  min {ts.min():8.1f}  (runs {runs})  "
                  f"{ts.mean() / t_k3:4.2f} x K3's time  {bps / 1e3:7.1f} GB/s ({nbytes[key] / n / P:.0f} P/particle) = "
                  f"{bps / k3:4.2f} x K3's rate", flush=True)
        del buf, st, handle, op


def dpmpp_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddim", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="logsnr20", eta=0.0, solver_order=2)
    ck, c = smp.sample_coefs(10), smp.solver_coef(10)
    P = bench.P_BYTES

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for n in (64, 16):
        op, fkw = bench.build_operator("gaussian_blur", dev, sigma=args.sigma)
        x_t, ring, truth, meas_noise = bench.synth_inputs(n, 2, dev, 1234)
        yy = op.forward(truth.to(dev), **fkw).detach()
        y = (yy + meas_noise.to(dev)[..., :yy.shape[-2], :yy.shape[-1]]).contiguous()
        handle = op.hip_handle(x_t)
        buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
        r0 = ring[0]
        buf.advance_x0()
        kernels.step_fwd(handle, buf, x_t, r0["model_out"], r0["noise"], y, ck, want_x0=True)      # a history to read
        buf.advance_x0()
        kernels.step_fwd(handle, buf, x_t, r0["model_out"], r0["noise"], y, ck, want_x0=True)      # sample, x0_hat
        kernels.step_bwd(handle, buf, y, 0.3, 1, ck)

        def torch_ops(i):
            x = kernels.step_update(buf, ring[i % 2]["g_unet"], ck)
            return x.add_(buf.x0_hat - buf.x0_prev, alpha=c)

        def fwd(store):
            return lambda i: kernels.step_fwd(handle, buf, x_t, ring[i % 2]["model_out"], ring[i % 2]["noise"], y, ck,
                                              want_x0=store)

        forms = {"a K3": lambda i: kernels.step_update(buf, ring[i % 2]["g_unet"], ck),
                 "b update_ms, c != 0": lambda i: kernels.step_update_ms(buf, ring[i % 2]["g_unet"], ck, c),
                 "c update_ms, c = 0": lambda i: kernels.step_update_ms(buf, ring[i % 2]["g_unet"], ck, 0.0),
                 "d K3 + two torch ops": torch_ops,
                 "K1 without the x0_hat store": fwd(False), "K1 with the x0_hat store": fwd(True)}
        nbytes = {"a K3": 4 * P * n, "b update_ms, c != 0": 6 * P * n, "c update_ms, c = 0": 4 * P * n}
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for key, fn in forms.items():
                res.setdefault(key, []).append(timed(fn))
        t_k3 = float(np.concatenate(res["a K3"]).mean())
        k3 = nbytes["a K3"] / t_k3
        for key in forms:
            ts = np.concatenate(res[key])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[key])
            rate = ""
            if key in nbytes:
                bps = nbytes[key] / ts.mean()
                rate = (f"  {ts.mean() / t_k3:4.2f} x K3's time  {bps / 1e3:7.1f} GB/s ({nbytes[key] / n / P:.0f} P/particle) = "
                        f"{bps / k3:4.2f} x K3's rate")
            print(f"dpmpp 256^2 N={n:2d} {key:30s} avg {ts.mean():8.1f} us  min {ts.min():8.1f}  (runs {runs}){rate}",
                  flush=True)
        del buf, handle, op


def metrics_step(args):
    from dps_ttc_amd import kernels, metrics
    dev = torch.device("cuda", 0)
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / (2 * 1.5 * 1.5))
    g = (g / g.sum()).float().to(dev)
    win = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    def torch_ops(x, label, per):
        """the same three numbers as batched torch ops (no host read)"""
        y = label.repeat_interleave(per, dim=0)
        flat = label.reshape(label.shape[0], -1)
        L = (flat.max(dim=1).values - flat.min(dim=1).values).repeat_interleave(per)
        mse = ((x - y) ** 2).reshape(x.shape[0], -1).mean(dim=1)
        psnr = 10.0 * torch.log10(L * L / mse)
        f = lambda a: torch.nn.functional.conv2d(a, win, groups=3)
        mx, my = f(x), f(y)
        vx, vy, cxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
        c1, c2 = ((0.01 * L) ** 2)[:, None, None, None], ((0.03 * L) ** 2)[:, None, None, None]
        s = (2 * mx * my + c1) * (2 * cxy + c2) / ((mx * mx + my * my + c1) * (vx + vy + c2))
        return mse, psnr, s.reshape(x.shape[0], -1).mean(dim=1)

    for n, m in ((64, 1), (64, 4), (512, 1)):
        torch.manual_seed(n + m)
        label = torch.rand(m, 3, 256, 256, device=dev) * 2 - 1
        x = (label.repeat_interleave(n // m, dim=0) + 0.1 * torch.randn(n, 3, 256, 256, device=dev)).contiguous()
        out = {name: torch.empty(n, dtype=torch.float32, device=dev) for name in kernels.METRIC_NAMES}
        both = {name: out[name] for name in ("mse", "psnr")}

        def host_loop(i):
            for p in range(n):
                float(metrics.compute_psnr(label[p // (n // m):p // (n // m) + 1], x[p].unsqueeze(0)))

        forms = {"a compute_psnr loop, host reads (PSNR only)": host_loop,
                 "b torch ops: 5 depthwise conv2d + map + means": lambda i: torch_ops(x, label, n // m),
                 "c image_metrics, mse + psnr + ssim": lambda i: kernels.image_metrics(x, label, out=out),
                 "c image_metrics, PSNR only": lambda i: kernels.image_metrics(x, label, want=("mse", "psnr"), out=both)}
        ref, got = torch_ops(x, label, n // m), kernels.image_metrics(x, label)
        agree = " ".join(f"{name} {float((got[name] - r).abs().max()):.1e}" for name, r in zip(kernels.METRIC_NAMES, ref))
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for key, fn in forms.items():
                res.setdefault(key, []).append(timed(fn))
        t_b = float(np.concatenate(res["b torch ops: 5 depthwise conv2d + map + means"]).mean())
        for key in forms:
            ts = np.concatenate(res[key])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[key])
            print(f"metrics 256^2 N={n:3d} M={m} {key:46s} avg {ts.mean():9.1f} us  min {ts.min():9.1f}  (runs {runs})  "
                  f"{ts.mean() / t_b:6.3f} x (b)'s time", flush=True)
        print(f"metrics 256^2 N={n:3d} M={m} max |(c) - (b)|: {agree}", flush=True)
        del x, label, out


def resample_step(args):
    from dps_ttc_amd import kernels
    dev = torch.device("cuda", 0)
    M4 = max(1, args.images or 4)
    scale = 100.0
    gen = torch.Generator(device=dev).manual_seed(1234)

    def multinomial(img, distance, u, segments):      # TTC_DDIM._resample, resample_draw = "multinomial", no rng_parity
        n = len(distance)
        weights = torch.exp(-distance / scale)
        flat = weights.max() == weights.min()
        drawn = torch.multinomial(torch.where(flat, torch.ones_like(weights), weights), n, replacement=True)
        ids = torch.where(flat, torch.arange(n, device=img.device), drawn)
        return kernels.gather(img, ids, validate=False), kernels.gather(distance.reshape(n, 1), ids, validate=False).reshape(n)

    def draw_gather(img, distance, u, segments):
        n = len(distance)
        ids = kernels.resample_draw(distance, u, segments, 1.0 / scale)
        return kernels.gather(img, ids, validate=False), kernels.gather(distance.reshape(n, 1), ids, validate=False).reshape(n)

    def fused(img, distance, u, segments):
        return kernels.resample(img, distance, u, segments, 1.0 / scale)

    def fused_ex(img, distance, u, segments, scheme, ess):       # dpsx_resample_seg_ex_f32; the same outputs as c
        return kernels.resample(img, distance, u, segments, 1.0 / scale, scheme=scheme, ess=ess)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in evs:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for M, k in ((1, 16), (1, 64), (1, 512), (M4, 16)):
        n = M * k
        img = torch.randn(n, 3, 256, 256, device=dev, generator=gen)
        distance = 50.0 + 30.0 * torch.randn(n, device=dev, generator=gen)
        u = torch.rand(n, device=dev, generator=gen)
        sl = [slice(m * k, (m + 1) * k) for m in range(M)]
        parts = [(img[s], distance[s], u[s]) for s in sl]           # contiguous views: no copy in the timed region
        forms = []
        if M == 1:
            forms.append(("a multinomial + 2 gathers", lambda: multinomial(img, distance, u, 1)))
        forms += [("b draw + 2 gathers", lambda: draw_gather(img, distance, u, M)),
                  ("c fused", lambda: fused(img, distance, u, M)),
                  ("d fused ex, multinomial tau 1", lambda: fused_ex(img, distance, u, M, "multinomial", 1.0)),
                  ("e fused ex, systematic tau 1", lambda: fused_ex(img, distance, u, M, "systematic", 1.0)),
                  ("f fused ex, systematic tau 0.5", lambda: fused_ex(img, distance, u, M, "systematic", 0.5))]
        if M > 1:
            forms += [(f"a multinomial + 2 gathers, {M} calls", lambda: [multinomial(*p, 1) for p in parts]),
                      (f"b draw + 2 gathers, {M} calls", lambda: [draw_gather(*p, 1) for p in parts]),
                      (f"c fused, {M} calls", lambda: [fused(*p, 1) for p in parts])]
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for name, fn in forms:
                res.setdefault(name, []).append(timed(fn))
        moved = 2.0 * n * (img[0].numel() + 1) * 4      # particles and distances, read once and written once
        for name, _ in forms:
            ts = np.concatenate(res[name])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[name])
            print(f"resample 256^2 M={M} K={k:3d} {name:36s} avg {ts.mean():8.1f} us  min {ts.min():8.1f}  (runs {runs})  "
                  f"{moved / ts.mean() / 1e6:6.2f} TB/s = {moved / ts.mean() / 1e6 / 8.0:.2f} of 8 TB/s", flush=True)
        del img, parts


def repulse_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    c, h, w = 3, 256, 256
    D, P = c * h * w, c * h * w * 4

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for M, k in ((4, 16), (1, 64), (1, 512)):
        n = M * k
        gen = torch.Generator(device=dev).manual_seed(1234)
        base = torch.randn(M, 1, c, h, w, device=dev, generator=gen)
        x = (np.sqrt(0.5) * base + np.sqrt(0.5) * torch.randn(M, k, c, h, w, device=dev, generator=gen)).reshape(n, c, h, w)
        x = x.contiguous()
        out = torch.empty_like(x)
        strength = 0.05 * D
        buf = kernels.StepBuffers(None, n, c, h, w, dev)
        buf.sample.copy_(x)
        g_unet = 1e-3 * torch.randn(n, c, h, w, device=dev, generator=gen)
        eye = torch.eye(k, device=dev, dtype=torch.bool)

        def a_dist(i):
            kernels.pairwise_sqdist(x, images=M)

        def b_whole(i):
            kernels.repulse(x, strength, images=M, out=out)

        def c_torch(i):
            xf = x.view(M, k, D)
            d2 = torch.cdist(xf, xf) ** 2
            hh = d2.sum(dim=(1, 2), keepdim=True) / (k * (k - 1)) / np.log(k + 1.0)
            wt = torch.exp(-d2 / hh).masked_fill(eye, 0.0)
            return xf + (2.0 * strength / hh) * (wt.sum(dim=2, keepdim=True) * xf - torch.matmul(wt, xf))

        def d_k3(i):
            kernels.step_update(buf, g_unet, ck)

        forms = (("a pairwise_sqdist (pairs + finisher)", a_dist), ("b repulse (all three launches)", b_whole),
                 ("c torch cdist + exp + matmul", c_torch), ("d K3 (step_update) for scale", d_k3))
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for name, fn in forms:
                res.setdefault(name, []).append(timed(fn))
        # the floors by shape arithmetic: bytes at 8 TB/s (each particle once; the apply also writes), fp32 vector operations
        # at 157 TFLOP/s (the packed-fma rate; the launches issue sub + fma per element and pair)
        pair_flop, apply_flop = 3.0 * D * M * k * (k - 1) / 2, 3.0 * D * M * k * k
        floors = {"a": (n * P / 8e6, pair_flop / 157e6), "b": (3 * n * P / 8e6, (pair_flop + apply_flop) / 157e6)}
        tiles = (k + 7) // 8
        for name, _ in forms:
            ts = np.concatenate(res[name])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[name])
            note = ""
            if name[0] in floors:
                fb, ff = floors[name[0]]
                note = (f"  floors: bytes {fb:.1f} us, fp32 {ff:.1f} us ({'fp32' if ff > fb else 'bytes'} binds: "
                        f"{max(fb, ff) / ts.mean():.2f} of it); a particle is fetched {tiles + 1} x by the pairs"
                        + (f", {tiles} x by the apply" if name[0] == "b" else ""))
            print(f"repulse 256^2 M={M} K={k:3d} {name:38s} avg {ts.mean():9.1f} us  min {ts.min():9.1f}  (runs {runs}){note}",
                  flush=True)
        del x, out, buf, g_unet, base


def ensemble_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    c, h, w = 3, 256, 256
    D, P = c * h * w, c * h * w * 4

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for M, k in ((4, 16), (1, 64), (1, 512)):
        n = M * k
        gen = torch.Generator(device=dev).manual_seed(1234)
        y = torch.randn(M, c, h, w, device=dev, generator=gen)
        x = (np.sqrt(0.5) * y[:, None] + np.sqrt(0.5) * torch.randn(M, k, c, h, w, device=dev, generator=gen)).reshape(n, c, h, w)
        x = x.contiguous()
        e = 3.0 * torch.randn(n, device=dev, generator=gen)
        g_unet = 1e-3 * torch.randn(n, c, h, w, device=dev, generator=gen)
        buf = kernels.StepBuffers(None, n, c, h, w, dev)
        buf.sample.copy_(x)
        cnt = torch.arange(1, k + 1, device=dev, dtype=torch.float32).view(1, k, 1)

        def a_call(i):
            kernels.ensemble_stats(x, images=M, label=y)

        def a_weighted(i):
            kernels.ensemble_stats(x, images=M, label=y, neg_log_weights=e)

        def b_torch(i):
            xf = x.view(M, k, D)
            var, mean = torch.var_mean(xf, dim=1, unbiased=False)
            curve = ((torch.cumsum(xf, dim=1) / cnt - y.view(M, 1, D)) ** 2).mean(dim=2)
            return mean, var, curve, var.mean(dim=1)

        def d_k3(i):
            kernels.step_update(buf, g_unet, ck)

        forms = (("a ensemble_stats (stream + finisher)", a_call), ("a' ensemble_stats with weights (3 launches)", a_weighted),
                 ("b torch var_mean + cumsum curve", b_torch), ("d K3 (step_update) for scale", d_k3))
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for name, fn in forms:
                res.setdefault(name, []).append(timed(fn))
        floor_bytes = M * ((k + 1) * P + 2 * P)
        t_k3 = float(np.concatenate(res["d K3 (step_update) for scale"]).mean())
        k3_rate = 4 * P * n / t_k3
        for name, _ in forms:
            ts = np.concatenate(res[name])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[name])
            note = ""
            if name[0] == "a":
                rate = floor_bytes / ts.mean()
                note = (f"  c floor {floor_bytes / 8e6:.1f} us ({floor_bytes / 8e6 / ts.mean():.2f} of it); {rate / 1e3:.0f} GB/s = "
                        f"{rate / k3_rate:.2f} x K3's rate")
            elif name[0] == "d":
                note = f"  {k3_rate / 1e3:.0f} GB/s (4 P/particle)"
            print(f"ensemble 256^2 M={M} K={k:3d} {name:44s} avg {ts.mean():9.1f} us  min {ts.min():9.1f}  (runs {runs}){note}",
                  flush=True)
        del x, y, e, buf, g_unet


def quantiles_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    c, h, w = 3, 256, 256
    D, P = c * h * w, c * h * w * 4
    probs = (0.05, 0.5, 0.95)

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    for M, k in ((4, 16), (1, 64), (1, 512)):
        n = M * k
        gen = torch.Generator(device=dev).manual_seed(1234)
        y = torch.randn(M, c, h, w, device=dev, generator=gen)
        x = (np.sqrt(0.5) * y[:, None] + np.sqrt(0.5) * torch.randn(M, k, c, h, w, device=dev, generator=gen)).reshape(n, c, h, w)
        x = x.contiguous()
        g_unet = 1e-3 * torch.randn(n, c, h, w, device=dev, generator=gen)
        buf = kernels.StepBuffers(None, n, c, h, w, dev)
        buf.sample.copy_(x)
        pos = [(int(np.floor(p * (k - 1))), min(int(np.floor(p * (k - 1))) + 1, k - 1), p * (k - 1) - np.floor(p * (k - 1)))
               for p in probs]
        coef = (2.0 * torch.arange(k, device=dev, dtype=torch.float64) - k + 1).view(1, k, 1)

        def a_call(i):
            kernels.order_stats(x, images=M, probs=probs, label=y)

        def a_sort(i):
            kernels.order_stats(x, images=M, probs=(0.5,))

        def b_torch(i):
            xf, yf = x.view(M, k, D), y.view(M, 1, D)
            xs = torch.sort(xf, dim=1).values
            quant = torch.stack([(xs[:, lo].double() + f * (xs[:, hi].double() - xs[:, lo].double())).float()
                                 for lo, hi, f in pos], dim=1)
            rank = (xf < yf).sum(dim=1)
            hist = torch.zeros(M, k + 2, device=dev, dtype=torch.int64).scatter_add_(1, rank, torch.ones_like(rank))
            xd = xs.double()
            crps = ((xd - yf.double()).abs().sum(dim=1) / k - (coef * xd).sum(dim=1) / (k * k)).float().mean(dim=1)
            return quant, hist, crps, (quant[:, -1] - quant[:, 0]).mean(dim=1)

        def d_k3(i):
            kernels.step_update(buf, g_unet, ck)

        forms = (("a order_stats with the label (pass + finisher)", a_call), ("a' order_stats, no label, one probability", a_sort),
                 ("b torch sort + gathers + rank count + CRPS", b_torch), ("d K3 (step_update) for scale", d_k3))
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for name, fn in forms:
                res.setdefault(name, []).append(timed(fn))
        floor_bytes = M * (k + 1) * P
        t_k3 = float(np.concatenate(res["d K3 (step_update) for scale"]).mean())
        k3_rate = 4 * P * n / t_k3
        for name, _ in forms:
            ts = np.concatenate(res[name])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[name])
            note = ""
            if name[0] == "a":
                rate = floor_bytes / ts.mean()
                note = (f"  c floor {floor_bytes / 8e6:.1f} us ({floor_bytes / 8e6 / ts.mean():.2f} of it); {rate / 1e3:.0f} GB/s = "
                        f"{rate / k3_rate:.2f} x K3's rate")
            elif name[0] == "d":
                note = f"  {k3_rate / 1e3:.0f} GB/s (4 P/particle)"
            print(f"quantiles 256^2 M={M} K={k:3d} {name:48s} avg {ts.mean():9.1f} us  min {ts.min():9.1f}  (runs {runs}){note}",
                  flush=True)
        del x, y, buf, g_unet


PCA_SHAPES = ((4, 16), (1, 64), (1, 128))      # M, K at 3 x 256^2
PCA_Q = 4


def pca_step(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    c, h, w = 3, 256, 256
    D, P, q = c * h * w, c * h * w * 4, PCA_Q

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    shapes = PCA_SHAPES if args.pca_shape is None else (PCA_SHAPES[args.pca_shape],)
    for M, k in shapes:
        n = M * k
        gen = torch.Generator(device=dev).manual_seed(1234)
        base = torch.rand(M, 1, D, device=dev, generator=gen) * 2 - 1
        u = torch.linalg.qr(torch.randn(M, D, 6, device=dev, generator=gen)).Q
        amp = 0.2 * np.sqrt(D) * 0.5 ** torch.arange(6, device=dev)
        x = base + (torch.randn(M, k, 6, device=dev, generator=gen) * amp) @ u.transpose(1, 2) + \
            0.05 * torch.randn(M, k, D, device=dev, generator=gen)
        x = x.reshape(n, c, h, w).contiguous()
        g_unet = 1e-3 * torch.randn(n, c, h, w, device=dev, generator=gen)
        buf = kernels.StepBuffers(None, n, c, h, w, dev)
        buf.sample.copy_(x)

        def a_call(i):
            return kernels.particle_pca(x, images=M, components=q)

        def b_dist(i):
            return kernels.pairwise_sqdist(x, images=M)

        def c_torch(i):
            xf = x.view(M, k, D)
            mean = xf.mean(dim=1, keepdim=True)
            xc = xf - mean
            lam, v = torch.linalg.eigh(xc @ xc.transpose(1, 2))
            lam, v = lam[:, -q:].flip(1), v[:, :, -q:].flip(2)
            coords = v * lam.clamp_min(0).sqrt().unsqueeze(1)
            return (coords.transpose(1, 2) @ xc) / lam.unsqueeze(2), lam, coords

        def d_k3(i):
            kernels.step_update(buf, g_unet, ck)

        sweeps = a_call(0)["info"][:, 2].cpu().numpy()
        forms = (("a particle_pca (distances + eigensolver + projection)", a_call), ("b pairwise_sqdist (the distances alone)", b_dist),
                 ("c torch centre + X X^T + eigh + matmul", c_torch), ("d K3 (step_update) for scale", d_k3))
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for name, fn in forms:
                res.setdefault(name, []).append(timed(fn))
        t_k3 = float(np.concatenate(res["d K3 (step_update) for scale"]).mean())
        for name, _ in forms:
            ts = np.concatenate(res[name])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[name])
            note = f"  sweeps {sweeps.tolist()}" if name[0] == "a" else (f"  {4 * P * n / t_k3 / 1e3:.0f} GB/s (4 P/particle)" if name[0] == "d" else "")
            print(f"pca 256^2 M={M} K={k:3d} q={q} {name:54s} avg {ts.mean():9.1f} us  min {ts.min():9.1f}  (runs {runs}){note}",
                  flush=True)
        del x, buf, g_unet


def pca_trace(args):
    """the launches of a traced `--pca --pca-shape I` run, by kernel and grid; rates by shape arithmetic"""
    import collections
    import csv
    import glob
    import re
    M, k = PCA_SHAPES[args.pca_shape]
    P = 3 * 256 * 256 * 4
    acc = collections.defaultdict(list)
    for f in glob.glob(f"{args.pca_trace}/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", "")).replace("void dpsx::", "")
            if re.search(r"k_pca|k_repulse|k_step_update", name):
                acc[name].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, v in sorted(acc.items()):
        v = np.array(v)
        note = ""
        if "k_pca_project" in name:
            note = f"  {M * (k + PCA_Q) * P / v.mean() / 1e3:.0f} GB/s ((K + q) D 4 bytes per image)"
        elif "k_step_update" in name:
            note = f"  {4 * P * M * k / v.mean() / 1e3:.0f} GB/s (4 P/particle)"
        print(f"pca 256^2 M={M} K={k:3d} q={PCA_Q} launch {name:44s} calls {v.size:4d}  avg {v.mean():9.1f} us  min {v.min():9.1f}{note}")


def noise_draw(args):
    from dps_ttc_amd import kernels
    from dps_ttc_amd.gaussian_diffusion import create_sampler
    dev = torch.device("cuda", 0)
    n = args.particles
    smp = create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                         model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True,
                         rescale_timesteps=True, timestep_respacing="")
    ck = smp.step_coefs[500]
    x_t, ring, truth, _ = bench.synth_inputs(n, 2, dev, 1234)
    shape = tuple(x_t.shape)

    def timed(fn):
        for i in range(3):
            fn(i)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for i, (a, b) in enumerate(evs):
            a.record()
            fn(i)
            b.record()
        torch.cuda.synchronize()
        return np.array([a.elapsed_time(b) for a, b in evs]) * 1e3

    def report(tag, forms, note):
        res = {}
        for rep in range(3):                           # alternated: every form sees the same box state
            for name, fn in forms:
                res.setdefault(name, []).append(timed(fn))
        for name, _ in forms:
            ts = np.concatenate(res[name])
            runs = " / ".join(f"{r.mean():.1f}" for r in res[name])
            print(f"noise 256^2 N={n} {tag:18s} {name:30s} avg {ts.mean():8.1f} us  min {ts.min():8.1f}  (runs {runs})  {note}",
                  flush=True)

    for name in ("gaussian_blur", "motion_blur", "super_resolution", "inpainting", "phase_retrieval"):
        op, fkw = bench.build_operator(name, dev)
        y = op.forward(truth.to(dev), **fkw).detach().contiguous()
        handle = op.hip_handle_for(fkw["mask"]) if name == "inpainting" else op.hip_handle(x_t)
        buf = kernels.StepBuffers(handle, n, 3, 256, 256, dev)
        fill = buf.noise_buffer()
        want_x0 = name in ("inpainting", "phase_retrieval")            # as the `ps` loop: x0_hat is stored only where K2 reads it
        in_kernel = handle.draws_in_kernel(3, 256, 256)

        def a_torch(i):
            kernels.step_fwd(handle, buf, x_t, ring[i % 2]["model_out"], torch.randn(shape, device=dev), y, ck, want_x0=want_x0)

        def b_fill(i):
            kernels.randn(shape, kernels.Rng(7, i), dev, out=fill)
            kernels.step_fwd(handle, buf, x_t, ring[i % 2]["model_out"], fill, y, ck, want_x0=want_x0)

        def c_rng(i):
            kernels.step_fwd(handle, buf, x_t, ring[i % 2]["model_out"], None, y, ck, want_x0=want_x0, rng=kernels.Rng(7, i))

        report(name + " K1", (("a torch.randn + pointer", a_torch), ("b device fill + pointer", b_fill),
                              ("c in-kernel draw", c_rng)), "in-kernel" if in_kernel else "declines: c is the fallback, = b")
        del buf, handle, op

    # the single-state search step (S1 from one state for N proposals, scoring, select, the winner's copy)
    op, fkw = bench.build_operator("gaussian_blur", dev)
    y = op.forward(truth.to(dev), **fkw).detach().contiguous()
    handle = op.hip_handle(x_t)
    x1 = x_t[:1].contiguous()
    fill = torch.empty(shape, device=dev)

    def sa(i):
        handle.search_step_one(x1, ring[i % 2]["model_out"][:1], torch.randn(shape, device=dev), y, ck)

    def sb(i):
        kernels.randn(shape, kernels.Rng(7, i), dev, out=fill)
        handle.search_step_one(x1, ring[i % 2]["model_out"][:1], fill, y, ck)

    def sc(i):
        handle.search_step_one(x1, ring[i % 2]["model_out"][:1], None, y, ck, rng=kernels.Rng(7, i), n=n)

    report("search_step_one", (("a torch.randn + pointer", sa), ("b device fill + pointer", sb), ("c in-kernel draw", sc)),
           "in-kernel (S1)")


if __name__ == "__main__":
    main()
