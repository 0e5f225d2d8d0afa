// The two launches of the particle weights (include/dpsx.h: dpsx_step_update_corr_f32, dpsx_smc_accum_f32).
//
//   k_step_update_corr   K3 (x_next = sample - s, s = (-a/b) g_eps + g_unet: k_step_update's expression, the same two
//                        roundings) + the proposal correction's partial sums, one launch:
//                            corr = sum_e q_e (z_e - q_e / 2),   q_e = s_e / sd_e
//                        sd is S1's own (post_logvar + __expf(0.5 .); a DDIM record: sigma) and z S1's own noise (the pointer,
//                        or the same counter through rng_unit / rng_elem), so sample = mean + sd z is the sample K1 built.
//   k_smc_accum          E += twist_scale (d_cur^p - d_prev^p) - proposal_weight corr;  d_prev = d_cur   (one wave per particle)
//
// The pass is particle_pass.h's: grid (slots, n), one fp32 partial per block (the fixed tree of block_sum) in slot q;
// k_smc_accum adds a particle's slots in double with common.h's slots_sum.  The streams, their loader and s / sd are
// particle_pass.h's update streams (dsg.hip reads the same).  A unit's loads are issued before its arithmetic (and before
// the Philox rounds of the rng form); every input stream is read here for the last time of its step: non-temporal loads.
#include "particle_pass.h"

namespace dpsx {

template <bool VEC, bool RNG>
__global__ __launch_bounds__(kPassThreads) void k_step_update_corr(const UpdateArgs a)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float red[kPassThreads / kWave];
    const int64_t p = blockIdx.y, base = p * a.chw;
    const Range r = block_range(a.chw / W, a.per);
    const bool noisy = a.k.add_noise & 1, ddim = a.k.add_noise & 2;          // launch-uniform
    const uint32_t pid = RNG ? rng_particle(a.rng, (unsigned)p) : 0u;
    UpdateLoader<VEC, RNG, true, true> in(a, p, noisy, ddim);
    int64_t u = r.lo + threadIdx.x;
    if (u < r.hi) in.load(u);
    float acc = 0.0f;
    while (u < r.hi) {
        if constexpr (RNG)
            if (noisy) in.zv = draw<VEC>(a.rng, u, pid);
        T xn;
        float t[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float s = update_s(lane(in.gv, j), lane(in.uv, j), a);
            set(xn, j, lane(in.sv, j) - s);
            t[j] = 0.0f;
            if (noisy) {
                const float q = __fdiv_rn(s, update_sd(lane(in.vv, j), ddim, a));
                t[j] = __fmul_rn(q, __fsub_rn(lane(in.zv, j), __fmul_rn(0.5f, q)));
            }
        }
        st<T>(a.out + base + u * W, xn);
#pragma unroll
        for (int j = 0; j < W; ++j) acc = __fadd_rn(acc, t[j]);
        u += kPassThreads;
        if (u < r.hi) in.load(u);
    }
    const float sum = block_sum(acc, red);
    if (threadIdx.x == 0) a.part[p * gridDim.x + blockIdx.x] = noisy ? sum : 0.0f;
}

// one wave per particle
__global__ __launch_bounds__(kWave) void k_smc_accum(float *__restrict__ e, float *__restrict__ d_prev,
                                                     const float *__restrict__ d_cur, const float *__restrict__ part,
                                                     int slots, const uint8_t *__restrict__ reset, int per_segment,
                                                     float twist_scale, int power, float proposal_weight)
{
    const int64_t p = blockIdx.x;
    const double corr = part ? slots_sum(part + p * slots, slots) : 0.0;
    if (threadIdx.x != 0) return;
    const double base = (reset && reset[p / per_segment]) ? 0.0 : (double)e[p];
    const float dcf = d_cur[p];
    const double dc = dcf, dp = d_prev[p];
    const double twist = power == 2 ? dc * dc - dp * dp : dc - dp;
    double v = base + (double)twist_scale * twist;
    if (part) v -= (double)proposal_weight * corr;
    e[p] = (float)v;
    d_prev[p] = dcf;
}

int step_update_corr(const float *sample, const float *g_mo, const float *g_unet, const float *mo, const float *z,
                     bool use_rng, const RngK &r, float *x_next, float *partials, int64_t n, int64_t chw, const Coefs &k,
                     hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const UpdatePass u = update_pass(sample, g_mo, g_unet, mo, z, use_rng, r, 0.0f, x_next, partials, n, chw, k);
    return dispatch(u.vec, use_rng, [&](auto V, auto R) {
        k_step_update_corr<V.value, R.value><<<u.grid, kPassThreads, 0, s>>>(u.a);
        return check_launch();
    });
}

int smc_accum(float *e, float *d_prev, const float *d_cur, const float *partials, int slots, const uint8_t *reset,
              int64_t segments, int64_t n, float twist_scale, int power, float proposal_weight, hipStream_t s)
{
    if (n == 0) return DPSX_OK;
    k_smc_accum<<<(unsigned)n, kWave, 0, s>>>(e, d_prev, d_cur, partials, slots, reset, (int)(n / segments), twist_scale,
                                              power, proposal_weight);
    return check_launch();
}

}  // namespace dpsx
