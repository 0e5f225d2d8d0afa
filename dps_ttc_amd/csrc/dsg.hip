// The two launches of spherical-Gaussian guidance (include/dpsx.h: dpsx_step_update_dsg_f32; Yang et al. 2024, "Guidance
// with Spherical Gaussian Constraint for Conditional Diffusion"): K3's place on a step whose x_{t-1} is put on the sphere of
// radius r = ||sd|| around the model's mean instead of being moved by scale * gradient.
//
// THE expression (tests/dsg_ref.py restates it in float64; the bit-for-bit tests follow it).  Per element e of particle p,
// every operation one fp32 rounding (__fmul_rn / __fadd_rn / __fsub_rn; no contraction):
//     s_e  = fadd(fmul(ratio, g_eps_e), g_unet_e)        ratio = -a / b (fp32, host); g_unet absent: + 0.0f (k_step_update)
//     sd_e = __expf(fmul(0.5f, post_logvar(v_e)))        DDPM record (S1's device functions); DDIM record: sd_e = min_log
//     n_e  = fmul(sd_e, z_e)                             z from `noise`, or rng_unit / rng_elem with S1's counters
//   k_dsg_stats   four sums per block, each term one fmul, added with fadd in a fixed order (per lane: units in index
//                 order, the lanes of a unit 0..3; then block_sum's tree):
//                     S = sum fmul(s, s)   Nn = sum fmul(n, n)   C = sum fmul(s, n)   R = sum fmul(sd, sd)
//                 -> stats[p][slot][0..3] = (S, Nn, C, R); a step without noise writes zeros and reads nothing.
//   k_dsg_apply   every block adds its particle's slots x 4 partials in double in slots_sum's order, then in double, g the
//                 guidance rate:
//                     r  = sqrt(R)
//                     mm = (1 - g)^2 Nn + g^2 R - 2 g (1 - g) r C / sqrt(S)         (= ||m||^2, m = n + g (d* - n), d* = -r s / ||s||)
//                     alpha = r (1 - g) / sqrt(mm)        beta = r r g / (sqrt(mm) sqrt(S))
//                 alpha and beta are rounded to fp32 once each, am1 = fsub(alpha, 1.0f), and
//                     x_next_e = fsub(fadd(sample_e, fmul(am1, n_e)), fmul(beta, s_e))        (= mean + r m / ||m||)
//                 A step without noise, S not > 0 or mm not > 0 (NaN included): x_next_e = sample_e, copied (no arithmetic:
//                 the bits of sample, -0.0 included); a step without noise does not read the partials either.
//
// The pass is particle_pass.h's: grid (slots, n), block (q, p) owns one contiguous range of particle p; the first three
// lines above are its update streams (UpdateArgs, UpdateLoader, update_elem; smc.hip reads the same).  k_dsg_apply reads
// its inputs for the last time of the step: non-temporal loads; k_dsg_stats leaves them to the cache for k_dsg_apply.
#include "particle_pass.h"

namespace dpsx {

namespace {

template <bool VEC, bool RNG>
__global__ __launch_bounds__(kPassThreads) void k_dsg_stats(const UpdateArgs a)
{
    constexpr int W = Unit<VEC>::W;
    __shared__ float red[4][kPassThreads / kWave];
    const int64_t p = blockIdx.y;
    float *out = a.part + (p * gridDim.x + blockIdx.x) * 4;
    if (!(a.k.add_noise & 1)) {                                                // launch-uniform: r = 0, nothing is read
        if (threadIdx.x < 4) out[threadIdx.x] = 0.0f;
        return;
    }
    const bool ddim = a.k.add_noise & 2;
    const Range blk = block_range(a.chw / W, a.per);
    const uint32_t pid = RNG ? rng_particle(a.rng, (unsigned)p) : 0u;
    UpdateLoader<VEC, RNG, false, false> in(a, p, true, ddim);
    int64_t u = blk.lo + threadIdx.x;
    if (u < blk.hi) in.load(u);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    while (u < blk.hi) {
        if constexpr (RNG) in.zv = draw<VEC>(a.rng, u, pid);
        float t[W][4];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            float s, sd, nz;
            update_elem(lane(in.gv, j), lane(in.uv, j), lane(in.vv, j), lane(in.zv, j), ddim, a, s, sd, nz);
            t[j][0] = __fmul_rn(s, s);
            t[j][1] = __fmul_rn(nz, nz);
            t[j][2] = __fmul_rn(s, nz);
            t[j][3] = __fmul_rn(sd, sd);
        }
        u += kPassThreads;
        if (u < blk.hi) in.load(u);
#pragma unroll
        for (int j = 0; j < W; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], t[j][c]);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float sum = block_sum(acc[c], red[c]);
        if (threadIdx.x == 0) out[c] = sum;
    }
}

template <bool VEC, bool RNG>
__global__ __launch_bounds__(kPassThreads) void k_dsg_apply(const UpdateArgs a)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float coef[2];           // am1, beta
    __shared__ int copy;                // the particle keeps `sample`
    const int64_t p = blockIdx.y, base = p * a.chw;
    const Range blk = block_range(a.chw / W, a.per);
    const bool noisy = a.k.add_noise & 1, ddim = a.k.add_noise & 2;            // launch-uniform
    if (noisy && threadIdx.x < kWave) {
        // the particle's four sums: slots_sum's order (lane i adds slots i, i + 64, ... in index order, then the tree)
        const float *part = a.part + p * gridDim.x * 4;
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < (int)gridDim.x; i += kWave)
#pragma unroll
            for (int c = 0; c < 4; ++c) sum[c] += (double)part[i * 4 + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) wave_sum_f64(sum[c]);
        if (threadIdx.x == 0) {
            const double S = sum[0], Nn = sum[1], C = sum[2], R = sum[3], g = (double)a.rate;
            const double r = sqrt(R), rs = sqrt(S);
            const double mm = (1.0 - g) * (1.0 - g) * Nn + g * g * R - 2.0 * g * (1.0 - g) * r * C / rs;
            const bool ok = S > 0.0 && mm > 0.0;                               // false for NaN
            const double rm = sqrt(mm);
            coef[0] = ok ? __fsub_rn((float)(r * (1.0 - g) / rm), 1.0f) : 0.0f;
            coef[1] = ok ? (float)(r * r * g / (rm * rs)) : 0.0f;
            copy = !ok;
        }
    }
    __syncthreads();
    int64_t u = blk.lo + threadIdx.x;
    if (!noisy || copy) {                                                      // block-uniform
        for (; u < blk.hi; u += kPassThreads)
            st<T>(a.out + base + u * W, ld_last<T>(a.sample + base + u * W));
        return;
    }
    const float am1 = coef[0], beta = coef[1];
    const uint32_t pid = RNG ? rng_particle(a.rng, (unsigned)p) : 0u;
    UpdateLoader<VEC, RNG, true, true> in(a, p, true, ddim);
    if (u < blk.hi) in.load(u);
    while (u < blk.hi) {
        if constexpr (RNG) in.zv = draw<VEC>(a.rng, u, pid);
        T xn;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            float s, sd, nz;
            update_elem(lane(in.gv, j), lane(in.uv, j), lane(in.vv, j), lane(in.zv, j), ddim, a, s, sd, nz);
            set(xn, j, __fsub_rn(__fadd_rn(lane(in.sv, j), __fmul_rn(am1, nz)), __fmul_rn(beta, s)));
        }
        st<T>(a.out + base + u * W, xn);
        u += kPassThreads;
        if (u < blk.hi) in.load(u);
    }
}

}  // namespace

int step_update_dsg(const float *sample, const float *g_mo, const float *g_unet, const float *mo, const float *z,
                    bool use_rng, const RngK &r, float rate, float *x_next, float *stats, int64_t n, int64_t chw,
                    const Coefs &k, hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const UpdatePass u = update_pass(sample, g_mo, g_unet, mo, z, use_rng, r, rate, x_next, stats, n, chw, k);
    return dispatch(u.vec, use_rng, [&](auto V, auto R) {
        k_dsg_stats<V.value, R.value><<<u.grid, kPassThreads, 0, s>>>(u.a);
        const int rc = check_launch();
        if (rc != DPSX_OK) return rc;
        k_dsg_apply<V.value, R.value><<<u.grid, kPassThreads, 0, s>>>(u.a);
        return check_launch();
    });
}

}  // namespace dpsx
