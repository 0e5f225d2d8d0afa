// The two launches of the particle weights (include/dpsx.h: dpsx_step_update_corr_f32, dpsx_smc_accum_f32).
//
//   k_step_update_corr   K3 (x_next = sample - s, s = (-a/b) g_eps + g_unet: k_step_update's expression, the same two
//                        roundings) + the proposal correction's partial sums, one launch:
//                            corr = sum_e q_e (z_e - q_e / 2),   q_e = s_e / sd_e
//                        sd is S1's own (post_logvar + __expf(0.5 .); a DDIM record: sigma) and z S1's own noise (the pointer,
//                        or the same counter through rng_unit / rng_elem), so sample = mean + sd z is the sample K1 built.
//   k_smc_accum          E += twist_scale (d_cur^p - d_prev^p) - proposal_weight corr;  d_prev = d_cur   (one wave per particle)
//
// The reduction is cg.hip's: grid (slots, n); block (q, p) owns a contiguous range of particle p and leaves ONE fp32 partial
// (the fixed tree of block_sum) in slot q; slots = cg_slots(chw) depends on the particle size only, so a particle's partials
// do not depend on the batch it runs in.  k_smc_accum adds a particle's slots in double with common.h's slots_sum.  No
// atomics, no fences: the launch boundary orders the partials.  Everything a particle reads is its own, so a non-finite
// value stays inside its particle.
//
// Units: 16 bytes per lane where the particle size is a multiple of 4 and the buffers are 16-byte aligned; otherwise the
// scalar instantiation of the same body (chosen on the host).  A unit's loads are issued before its arithmetic (and before
// the Philox rounds of the rng form); every input stream is read here for the last time of its step: non-temporal loads.
#include "common.h"

namespace dpsx {

namespace {

constexpr int kSmcThreads = 256;

typedef float smc_f4 __attribute__((ext_vector_type(4)));

template <bool VEC> struct SmcUnit { typedef float T; static constexpr int W = 1; };
template <> struct SmcUnit<true> { typedef smc_f4 T; static constexpr int W = 4; };

template <class T> __device__ __forceinline__ T smc_ld_last(const float *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const T *>(p));
}

__device__ __forceinline__ float smc_lane(float v, int) { return v; }
__device__ __forceinline__ float smc_lane(const smc_f4 &v, int j) { return v[j]; }
__device__ __forceinline__ void smc_set(float &v, int, float x) { v = x; }
__device__ __forceinline__ void smc_set(smc_f4 &v, int j, float x) { v[j] = x; }

// the noise of unit u (VEC) / element u (scalar) of the particle with id pid: S1's draw (k_posterior_fwd and the fused K1s)
template <bool VEC> __device__ __forceinline__ typename SmcUnit<VEC>::T smc_draw(const RngK &r, int64_t u, uint32_t pid)
{
    if constexpr (VEC) {
        const float4 z = rng_unit(r, (uint32_t)u, pid);
        return smc_f4{z.x, z.y, z.z, z.w};
    } else {
        return rng_elem(r, u, pid);
    }
}

}  // namespace

struct CorrArgs {
    const float *sample, *g_mo, *gu, *mo, *z;
    float *out, *part;
    int64_t chw, per;       // per: work items (float4 units or elements) per block
    float ratio;            // -a / b
    Coefs k;
    RngK rng;
};

template <bool VEC, bool RNG>
__global__ __launch_bounds__(kSmcThreads) void k_step_update_corr(const CorrArgs a)
{
    using T = typename SmcUnit<VEC>::T;
    constexpr int W = SmcUnit<VEC>::W;
    __shared__ float red[kSmcThreads / kWave];
    const int64_t p = blockIdx.y, base = p * a.chw, mbase = p * 2 * a.chw;
    const int64_t units = a.chw / W, lo = (int64_t)blockIdx.x * a.per, hi = min(units, lo + a.per);
    const bool noisy = a.k.add_noise & 1, ddim = a.k.add_noise & 2;          // launch-uniform
    const bool has_u = a.gu != nullptr, ld_v = noisy && !ddim, ld_z = noisy && !RNG;
    const uint32_t pid = RNG ? rng_particle(a.rng, (unsigned)p) : 0u;
    int64_t u = lo + threadIdx.x;
    T sv = T{}, gv = T{}, uv = T{}, vv = T{}, zv = T{};
    auto load = [&](int64_t unit) {
        const int64_t i = unit * W;
        sv = smc_ld_last<T>(a.sample + base + i);
        gv = smc_ld_last<T>(a.g_mo + mbase + i);
        if (has_u) uv = smc_ld_last<T>(a.gu + base + i);
        if (ld_v) vv = smc_ld_last<T>(a.mo + mbase + a.chw + i);
        if (ld_z) zv = smc_ld_last<T>(a.z + base + i);
    };
    if (u < hi) load(u);
    float acc = 0.0f;
    while (u < hi) {
        if constexpr (RNG)
            if (noisy) zv = smc_draw<VEC>(a.rng, u, pid);
        T xn;
        float t[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float s = a.ratio * smc_lane(gv, j) + smc_lane(uv, j);       // k_step_update's expression
            smc_set(xn, j, smc_lane(sv, j) - s);
            t[j] = 0.0f;
            if (noisy) {
                const float sd = ddim ? a.k.min_log : __expf(__fmul_rn(0.5f, post_logvar(smc_lane(vv, j), a.k)));
                const float q = __fdiv_rn(s, sd);
                t[j] = __fmul_rn(q, __fsub_rn(smc_lane(zv, j), __fmul_rn(0.5f, q)));
            }
        }
        *reinterpret_cast<T *>(a.out + base + u * W) = xn;
#pragma unroll
        for (int j = 0; j < W; ++j) acc = __fadd_rn(acc, t[j]);
        u += kSmcThreads;
        if (u < hi) load(u);
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
    const bool noisy = k.add_noise & 1;
    const bool vec = chw % 4 == 0 && aligned16(sample) && aligned16(g_mo) && aligned16(g_unet) && aligned16(x_next) &&
                     (!noisy || (aligned16(mo) && (use_rng || aligned16(z))));
    const int64_t units = vec ? chw / 4 : chw, slots = cg_slots(chw);
    CorrArgs a{sample, g_mo, g_unet, mo, z, x_next, partials, chw, (units + slots - 1) / slots, -k.a / k.b, k, r};
    const dim3 grid((unsigned)slots, (unsigned)n);
    if (vec && use_rng) k_step_update_corr<true, true><<<grid, kSmcThreads, 0, s>>>(a);
    else if (vec) k_step_update_corr<true, false><<<grid, kSmcThreads, 0, s>>>(a);
    else if (use_rng) k_step_update_corr<false, true><<<grid, kSmcThreads, 0, s>>>(a);
    else k_step_update_corr<false, false><<<grid, kSmcThreads, 0, s>>>(a);
    return check_launch();
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
