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
// The reduction is smc.hip's: grid (slots, n), slots = cg_slots(chw) a function of the particle size only; block (q, p) owns
// one contiguous range of particle p; no atomics, no fences: the launch boundary orders the partials.  Everything a
// particle reads is its own, so a non-finite value stays inside its particle.  Units are 16 bytes per lane where the
// particle size is a multiple of 4 and the buffers are 16-byte aligned, else the scalar instantiation of the same body
// (chosen on the host by step_update_corr's rule).  k_dsg_apply reads its inputs for the last time of the step:
// non-temporal loads; k_dsg_stats leaves them to the cache for k_dsg_apply.
#include "common.h"

namespace dpsx {

namespace {

constexpr int kDsgThreads = 256;

typedef float dsg_f4 __attribute__((ext_vector_type(4)));

template <bool VEC> struct DsgUnit { typedef float T; static constexpr int W = 1; };
template <> struct DsgUnit<true> { typedef dsg_f4 T; static constexpr int W = 4; };

template <class T, bool LAST> __device__ __forceinline__ T dsg_ld(const float *p)
{
    if constexpr (LAST) return __builtin_nontemporal_load(reinterpret_cast<const T *>(p));
    else return *reinterpret_cast<const T *>(p);
}

__device__ __forceinline__ float dsg_lane(float v, int) { return v; }
__device__ __forceinline__ float dsg_lane(const dsg_f4 &v, int j) { return v[j]; }
__device__ __forceinline__ void dsg_set(float &v, int, float x) { v = x; }
__device__ __forceinline__ void dsg_set(dsg_f4 &v, int j, float x) { v[j] = x; }

// the noise of unit u (VEC) / element u (scalar) of the particle with id pid: S1's draw
template <bool VEC> __device__ __forceinline__ typename DsgUnit<VEC>::T dsg_draw(const RngK &r, int64_t u, uint32_t pid)
{
    if constexpr (VEC) {
        const float4 z = rng_unit(r, (uint32_t)u, pid);
        return dsg_f4{z.x, z.y, z.z, z.w};
    } else {
        return rng_elem(r, u, pid);
    }
}

struct DsgArgs {
    const float *sample, *g_mo, *gu, *mo, *z;
    float *out, *stats;     // stats [n, slots, 4]
    int64_t chw, per;       // per: work items (float4 units or elements) per block
    float ratio, rate;      // -a / b, the guidance rate
    Coefs k;
    RngK rng;
};

// s, sd and n of one element (the header's first three lines)
__device__ __forceinline__ void dsg_elem(float g, float u, float v, float z, bool ddim, const DsgArgs &a, float &s, float &sd,
                                         float &nz)
{
    s = __fadd_rn(__fmul_rn(a.ratio, g), u);
    sd = ddim ? a.k.min_log : __expf(__fmul_rn(0.5f, post_logvar(v, a.k)));
    nz = __fmul_rn(sd, z);
}

// the gradient / variance / noise streams of one unit; LAST: this launch is their last reader
template <bool VEC, bool RNG, bool LAST> struct DsgLoader {
    using T = typename DsgUnit<VEC>::T;
    static constexpr int W = DsgUnit<VEC>::W;
    const DsgArgs &a;
    const int64_t base, mbase;
    const bool has_u, ld_v;
    T gv = T{}, uv = T{}, vv = T{}, zv = T{};
    __device__ __forceinline__ DsgLoader(const DsgArgs &args, int64_t p, bool ddim)
        : a(args), base(p * args.chw), mbase(p * 2 * args.chw), has_u(args.gu != nullptr), ld_v(!ddim) {}
    __device__ __forceinline__ void load(int64_t unit)
    {
        const int64_t i = unit * W;
        gv = dsg_ld<T, LAST>(a.g_mo + mbase + i);
        if (has_u) uv = dsg_ld<T, LAST>(a.gu + base + i);
        if (ld_v) vv = dsg_ld<T, LAST>(a.mo + mbase + a.chw + i);
        if constexpr (!RNG) zv = dsg_ld<T, LAST>(a.z + base + i);
    }
};

template <bool VEC, bool RNG>
__global__ __launch_bounds__(kDsgThreads) void k_dsg_stats(const DsgArgs a)
{
    constexpr int W = DsgUnit<VEC>::W;
    __shared__ float red[4][kDsgThreads / kWave];
    const int64_t p = blockIdx.y;
    float *out = a.stats + (p * gridDim.x + blockIdx.x) * 4;
    if (!(a.k.add_noise & 1)) {                                                // launch-uniform: r = 0, nothing is read
        if (threadIdx.x < 4) out[threadIdx.x] = 0.0f;
        return;
    }
    const bool ddim = a.k.add_noise & 2;
    const int64_t units = a.chw / W, lo = (int64_t)blockIdx.x * a.per, hi = min(units, lo + a.per);
    const uint32_t pid = RNG ? rng_particle(a.rng, (unsigned)p) : 0u;
    DsgLoader<VEC, RNG, false> in(a, p, ddim);
    int64_t u = lo + threadIdx.x;
    if (u < hi) in.load(u);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    while (u < hi) {
        if constexpr (RNG) in.zv = dsg_draw<VEC>(a.rng, u, pid);
        float t[W][4];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            float s, sd, nz;
            dsg_elem(dsg_lane(in.gv, j), dsg_lane(in.uv, j), dsg_lane(in.vv, j), dsg_lane(in.zv, j), ddim, a, s, sd, nz);
            t[j][0] = __fmul_rn(s, s);
            t[j][1] = __fmul_rn(nz, nz);
            t[j][2] = __fmul_rn(s, nz);
            t[j][3] = __fmul_rn(sd, sd);
        }
        u += kDsgThreads;
        if (u < hi) in.load(u);
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
__global__ __launch_bounds__(kDsgThreads) void k_dsg_apply(const DsgArgs a)
{
    using T = typename DsgUnit<VEC>::T;
    constexpr int W = DsgUnit<VEC>::W;
    __shared__ float coef[2];           // am1, beta
    __shared__ int copy;                // the particle keeps `sample`
    const int64_t p = blockIdx.y, base = p * a.chw;
    const int64_t units = a.chw / W, lo = (int64_t)blockIdx.x * a.per, hi = min(units, lo + a.per);
    const bool noisy = a.k.add_noise & 1, ddim = a.k.add_noise & 2;            // launch-uniform
    if (noisy && threadIdx.x < kWave) {
        // the particle's four sums: slots_sum's order (lane i adds slots i, i + 64, ... in index order, then the tree)
        const float *st = a.stats + p * gridDim.x * 4;
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = threadIdx.x; i < (int)gridDim.x; i += kWave)
#pragma unroll
            for (int c = 0; c < 4; ++c) sum[c] += (double)st[i * 4 + c];
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
    int64_t u = lo + threadIdx.x;
    if (!noisy || copy) {                                                      // block-uniform
        for (; u < hi; u += kDsgThreads)
            *reinterpret_cast<T *>(a.out + base + u * W) = dsg_ld<T, true>(a.sample + base + u * W);
        return;
    }
    const float am1 = coef[0], beta = coef[1];
    const uint32_t pid = RNG ? rng_particle(a.rng, (unsigned)p) : 0u;
    DsgLoader<VEC, RNG, true> in(a, p, ddim);
    T sv = T{};
    if (u < hi) {
        sv = dsg_ld<T, true>(a.sample + base + u * W);
        in.load(u);
    }
    while (u < hi) {
        if constexpr (RNG) in.zv = dsg_draw<VEC>(a.rng, u, pid);
        T xn;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            float s, sd, nz;
            dsg_elem(dsg_lane(in.gv, j), dsg_lane(in.uv, j), dsg_lane(in.vv, j), dsg_lane(in.zv, j), ddim, a, s, sd, nz);
            dsg_set(xn, j, __fsub_rn(__fadd_rn(dsg_lane(sv, j), __fmul_rn(am1, nz)), __fmul_rn(beta, s)));
        }
        *reinterpret_cast<T *>(a.out + base + u * W) = xn;
        u += kDsgThreads;
        if (u < hi) {
            sv = dsg_ld<T, true>(a.sample + base + u * W);
            in.load(u);
        }
    }
}

template <bool VEC, bool RNG> int dsg_launch(const DsgArgs &a, dim3 grid, hipStream_t s)
{
    k_dsg_stats<VEC, RNG><<<grid, kDsgThreads, 0, s>>>(a);
    int rc = check_launch();
    if (rc != DPSX_OK) return rc;
    k_dsg_apply<VEC, RNG><<<grid, kDsgThreads, 0, s>>>(a);
    return check_launch();
}

}  // namespace

int step_update_dsg(const float *sample, const float *g_mo, const float *g_unet, const float *mo, const float *z,
                    bool use_rng, const RngK &r, float rate, float *x_next, float *stats, int64_t n, int64_t chw,
                    const Coefs &k, hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const bool noisy = k.add_noise & 1;
    const bool vec = chw % 4 == 0 && aligned16(sample) && aligned16(g_mo) && aligned16(g_unet) && aligned16(x_next) &&
                     (!noisy || (aligned16(mo) && (use_rng || aligned16(z))));
    const int64_t units = vec ? chw / 4 : chw, slots = cg_slots(chw);
    const DsgArgs a{sample, g_mo, g_unet, mo, z, x_next, stats, chw, (units + slots - 1) / slots, -k.a / k.b, rate, k, r};
    const dim3 grid((unsigned)slots, (unsigned)n);
    if (vec && use_rng) return dsg_launch<true, true>(a, grid, s);
    if (vec) return dsg_launch<true, false>(a, grid, s);
    if (use_rng) return dsg_launch<false, true>(a, grid, s);
    return dsg_launch<false, false>(a, grid, s);
}

}  // namespace dpsx
