// The per-segment resampling draw and its fusion with the gathers (include/dpsx.h "resampling draw", "resampling
// schemes and the ESS trigger"): one kernel body per launch shape, k_resample_draw_seg<EX> (one block per segment) and
// k_resample_seg<U, PER, EX> (one block per slice of a destination particle).  EX = false is the plain entry points'
// form: a segment whose weights are all equal keeps its particles, every other one draws multinomially, nothing else
// is stored.  EX = true takes a scheme and the ESS trigger and stores the per-segment diagnostics.
//
// The draw is a pure function of (distances, uniforms): integer weights
// q_i = rint(exp(-(d_i - d_min) * inv_scale) * 2^24), an exact 64-bit integer CDF, slot j takes the smallest i with
// cdf_i > (total * ui_j) >> 24.  Integer adds are associative, so the shape of the scan below (wave shuffles, tiles of
// kThreads, per-wave totals through LDS) cannot change a result: a segmented launch and one launch per image agree
// bit for bit, and so does a serial restatement on the host.
#include "common.h"

#include <type_traits>

namespace dpsx {

constexpr int kThreads = 256;
constexpr float kTwo24 = 16777216.0f;

__device__ __forceinline__ uint32_t resample_weight(float dv, float d_min, float inv_scale)
{
    if (!(fabsf(dv) <= 3.402823466e38f)) return 0u;               // NaN / inf: never drawn
    float w = expf(-((dv - d_min) * inv_scale));
    if (!(w >= 0.0f)) w = 0.0f;                                   // inert for finite inv_scale >= 0 (the entry points'
    if (w > 1.0f) w = 1.0f;                                       // contract): keeps q inside [0, 2^24] whatever comes in
    return (uint32_t)rintf(w * kTwo24);
}

__device__ __forceinline__ uint32_t resample_ui(float u)
{
    const float s = u * kTwo24;                                   // exact: a power-of-two scaling
    if (!(s > 0.0f)) return 0u;                                   // NaN, negative, zero
    return s >= 16777215.0f ? 16777215u : (uint32_t)s;
}

// Steps 1-4 for one segment d[0 .. k): fills cdf[0 .. k) (LDS) and returns the flat flag (block-uniform).
// q_all: the segment's q_out (every weight is stored) or nullptr; q_one / one: store the weight of particle `one` only
// (the fused launch's writer block of slot `one`).  All kThreads threads of the block must call it.
// S2 (the scheme / ESS form only): *s2 = sum of q_i^2 instead of the flat flag (one more exact integer reduction of
// the same shape; q_i^2 <= 2^48 and k <= 4096, so it stays below 2^60) and the return value is unspecified.
template <bool S2 = false>
__device__ __forceinline__ bool resample_cdf(const float *__restrict__ d, const int k, const float inv_scale,
                                             unsigned long long *__restrict__ cdf, int32_t *__restrict__ q_all,
                                             int32_t *__restrict__ q_one, const int one,
                                             unsigned long long *__restrict__ s2 = nullptr)
{
    __shared__ float s_min[kThreads / kWave];
    __shared__ unsigned long long s_tot[kThreads / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    constexpr int nw = kThreads / kWave;
    const float inf = __builtin_inff();
    // 1. the minimum over the finite distances (the first tile's value stays in a register for step 2)
    const float d0 = tid < k ? d[tid] : inf;
    float mn = fabsf(d0) <= 3.402823466e38f ? d0 : inf;
    for (int i = tid + kThreads; i < k; i += kThreads) {
        const float v = d[i];
        if (fabsf(v) <= 3.402823466e38f) mn = fminf(mn, v);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o, kWave));
    if (lane == 0) s_min[wave] = mn;
    __syncthreads();
    mn = s_min[0];
#pragma unroll
    for (int w = 1; w < nw; ++w) mn = fminf(mn, s_min[w]);
    // 2. + 3. integer weights, scanned tile by tile
    unsigned long long carry = 0, sq = 0;
    uint32_t q_lo = 0xffffffffu, q_hi = 0u;
    for (int base = 0; base < k; base += kThreads) {
        const int i = base + tid;
        uint32_t q = 0u;
        if (i < k) {
            q = resample_weight(base == 0 ? d0 : d[i], mn, inv_scale);
            q_lo = min(q_lo, q);
            q_hi = max(q_hi, q);
            if (q_all) q_all[i] = (int32_t)q;
            if (q_one && i == one) *q_one = (int32_t)q;
        }
        unsigned long long x = q;
        if constexpr (S2) sq += x * x;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const unsigned long long y = __shfl_up(x, o, kWave);
            if (lane >= o) x += y;
        }
        if (lane == kWave - 1) s_tot[wave] = x;
        __syncthreads();
        unsigned long long off = carry, tile = 0;
#pragma unroll
        for (int w = 0; w < nw; ++w) {
            const unsigned long long t = s_tot[w];
            if (w < wave) off += t;
            tile += t;
        }
        if (i < k) cdf[i] = x + off;
        carry += tile;
        __syncthreads();                                          // s_tot is rewritten by the next tile; cdf is complete
    }
    if constexpr (S2) {                                           // the trigger's second moment replaces step 4
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) sq += __shfl_xor(sq, o, kWave);
        if (lane == 0) s_tot[wave] = sq;                          // free since the last tile's closing barrier
        __syncthreads();
        sq = 0;
#pragma unroll
        for (int w = 0; w < nw; ++w) sq += s_tot[w];
        *s2 = sq;
        return false;
    }
    // 4. flat: every q of the segment equals q_0 (threads without a particle agree with anything)
    const uint32_t q0 = (uint32_t)cdf[0];
    return __syncthreads_and(q_lo > q_hi || (q_lo == q_hi && q_lo == q0)) != 0;
}

// 5. the slot's pick from the finished CDF: the smallest i with cdf_i > target, inside [0, k - 1]
__device__ __forceinline__ int resample_search(const unsigned long long *__restrict__ cdf, const int k,
                                               const unsigned long long target)
{
    int lo = 0, hi = k - 1;                                       // hi = k - 1: the clamp to the segment's last index
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > target) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// Everything below is integer arithmetic on the finished CDF, so it inherits the draw's independence of the launch shape.
// trigger: (sum q)^2 * 65536 < ess_q16 * k * sum q^2, both sides up to 2^88: compared as (high, low) 64-bit pairs
__device__ __forceinline__ bool resample_need(const unsigned long long total, const unsigned long long s2, const int k,
                                              const int ess_q16)
{
    const unsigned long long t_hi = __umul64hi(total, total), t_lo = total * total;    // total^2 <= 2^72
    const unsigned long long l_hi = (t_hi << 16) | (t_lo >> 48), l_lo = t_lo << 16;
    const unsigned long long a = (unsigned long long)ess_q16 * (unsigned long long)k;  // <= 2^28
    const unsigned long long r_hi = __umul64hi(a, s2), r_lo = a * s2;
    return l_hi < r_hi || (l_hi == r_hi && l_lo < r_lo);
}

// slot j's pick from its uniform u: multinomial (total * ui) >> 24; stratified / systematic
// ((total * (j 2^24 + ui)) >> 24) / k, the product up to 2^72, its shifted value below 2^48.  The caller hands the
// systematic scheme the first slot's u for every j.  The plain form passes the multinomial scheme as a constant and
// compiles to the first branch alone.
__device__ __forceinline__ int resample_pick(const unsigned long long *__restrict__ cdf, const int k, const int j,
                                             const float u, const int scheme)
{
    const unsigned long long total = cdf[k - 1];
    const uint32_t ui = resample_ui(u);
    unsigned long long target;
    if (scheme == DPSX_RESAMPLE_MULTINOMIAL) {
        target = (total * (unsigned long long)ui) >> 24;
    } else {
        const unsigned long long pos = ((unsigned long long)j << 24) + ui;
        const unsigned long long hi = __umul64hi(total, pos), lo = total * pos;
        target = ((hi << 40) | (lo >> 24)) / (unsigned long long)k;
    }
    return resample_search(cdf, k, target);
}

__device__ __forceinline__ float resample_ess(const unsigned long long total, const unsigned long long s2)
{
    return s2 ? (float)((double)total * (double)total / (double)s2) : 0.0f;
}

// one block per segment: ids (global particle indices) for every slot of the segment, and the weights when asked;
// EX: also the segment's flag and ESS (nullable).  scheme .. ess_out are not read without EX.
template <bool EX>
__global__ __launch_bounds__(kThreads) void k_resample_draw_seg(const float *__restrict__ d, const float *__restrict__ u,
                                                                const int k, const float inv_scale,
                                                                int64_t *__restrict__ ids, int32_t *__restrict__ q_out,
                                                                const int scheme, const int ess_q16,
                                                                uint8_t *__restrict__ flag_out,
                                                                float *__restrict__ ess_out)
{
    extern __shared__ unsigned long long s_cdf[];
    const int64_t lo = (int64_t)blockIdx.x * k;
    int32_t *__restrict__ q_all = q_out ? q_out + lo : nullptr;
    if constexpr (EX) {
        unsigned long long s2;
        resample_cdf<true>(d + lo, k, inv_scale, s_cdf, q_all, nullptr, -1, &s2);
        const unsigned long long total = s_cdf[k - 1];
        const bool need = resample_need(total, s2, k, ess_q16);
        if (threadIdx.x == 0) {
            if (flag_out) flag_out[blockIdx.x] = need ? 1 : 0;
            if (ess_out) ess_out[blockIdx.x] = resample_ess(total, s2);
        }
        const bool systematic = scheme == DPSX_RESAMPLE_SYSTEMATIC;
        for (int j = threadIdx.x; j < k; j += kThreads)
            ids[lo + j] = lo + (need ? resample_pick(s_cdf, k, j, u[systematic ? lo : lo + j], scheme) : j);
    } else {
        const bool flat = resample_cdf<false>(d + lo, k, inv_scale, s_cdf, q_all, nullptr, -1);
        for (int j = threadIdx.x; j < k; j += kThreads)
            ids[lo + j] = lo + (flat ? j : resample_pick(s_cdf, k, j, u[lo + j], DPSX_RESAMPLE_MULTINOMIAL));
    }
}

// The draw AND the gathers in one launch.  Block (x, p): repeats the draw of p's segment for slot p (k distances from the
// L2, the scan above, one binary search by thread 0) and copies slice x of the drawn particle to dst[p]; the block with
// x == 0 also stores ids_out[p], d_out[p] = d[id] and q_out[p].  U = 4: float4 units (chw % 4 == 0, 16-byte aligned
// bases), PER of them per lane with all loads issued before the stores; U = 1: the same over single floats.
constexpr int kResampleVecPer = 8;            // 256 lanes x 8 x 16 B = 32 KB per block: the repeated scan is a small part
constexpr int kResampleScalarPer = 32;
// slice blockIdx.x of particle `id` of src to particle p of dst, in units of U floats
template <int U, int PER>
__device__ __forceinline__ void resample_copy(const float *__restrict__ src, float *__restrict__ dst, const int64_t id,
                                              const int64_t p, const int64_t units)
{
    using V = typename std::conditional<U == 4, float4, float>::type;
    const V *__restrict__ s = reinterpret_cast<const V *>(src) + id * units;
    V *__restrict__ t = reinterpret_cast<V *>(dst) + p * units;
    const int64_t b0 = (int64_t)blockIdx.x * (kThreads * PER), i0 = b0 + threadIdx.x;
    if (b0 + kThreads * PER <= units) {                           // a whole slice (block-uniform): loads first, then stores
        V v[PER];
#pragma unroll
        for (int e = 0; e < PER; ++e) v[e] = s[i0 + (int64_t)e * kThreads];
#pragma unroll
        for (int e = 0; e < PER; ++e) t[i0 + (int64_t)e * kThreads] = v[e];
    } else {                                                      // the particle's last, partial slice
        for (int64_t i = i0; i < units; i += kThreads) t[i] = s[i];
    }
}

// EX: block (0, first slot of a segment) also stores the segment's flag and ESS (nullable); a segment that does not
// resample is copied as it is.  scheme .. ess_out are not read without EX.
template <int U, int PER, bool EX>
__global__ __launch_bounds__(kThreads) void k_resample_seg(const float *__restrict__ d, const float *__restrict__ u,
                                                           const int k, const float inv_scale,
                                                           const float *__restrict__ src, float *__restrict__ dst,
                                                           float *__restrict__ d_out, int64_t *__restrict__ ids,
                                                           int32_t *__restrict__ q_out, const int64_t units,
                                                           const int scheme, const int ess_q16,
                                                           uint8_t *__restrict__ flag_out, float *__restrict__ ess_out)
{
    extern __shared__ unsigned long long s_cdf[];
    __shared__ int s_pick;
    const int64_t p = blockIdx.y;
    const int64_t m = p / k, lo = m * k;
    const int j = (int)(p - lo);
    const bool writer = blockIdx.x == 0;
    int32_t *__restrict__ q_one = writer && q_out ? q_out + p : nullptr;
    if constexpr (EX) {
        const float uj = u[scheme == DPSX_RESAMPLE_SYSTEMATIC ? lo : p];
        unsigned long long s2;
        resample_cdf<true>(d + lo, k, inv_scale, s_cdf, nullptr, q_one, j, &s2);
        if (threadIdx.x == 0) {
            const unsigned long long total = s_cdf[k - 1];
            const bool need = resample_need(total, s2, k, ess_q16);
            s_pick = need ? resample_pick(s_cdf, k, j, uj, scheme) : j;
            if (writer && j == 0) {
                if (flag_out) flag_out[m] = need ? 1 : 0;
                if (ess_out) ess_out[m] = resample_ess(total, s2);
            }
        }
    } else {
        const float uj = u[p];
        const bool flat = resample_cdf<false>(d + lo, k, inv_scale, s_cdf, nullptr, q_one, j);
        if (threadIdx.x == 0) s_pick = flat ? j : resample_pick(s_cdf, k, j, uj, DPSX_RESAMPLE_MULTINOMIAL);
    }
    __syncthreads();
    const int64_t id = lo + s_pick;                               // inside the segment by construction
    if (writer && threadIdx.x == 0) {
        ids[p] = id;
        d_out[p] = d[id];
    }
    resample_copy<U, PER>(src, dst, id, p, units);
}

int resample_draw_seg(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, int64_t *ids,
                      int32_t *q_out, const ResampleOpts *opts, hipStream_t s)
{
    const ResampleOpts o = opts ? *opts : ResampleOpts{};
    const auto kernel = opts ? k_resample_draw_seg<true> : k_resample_draw_seg<false>;
    kernel<<<(unsigned)segments, kThreads, (size_t)k * sizeof(unsigned long long), s>>>(
        d, u, (int)k, inv_scale, ids, q_out, o.scheme, o.ess_q16, o.flag_out, o.ess_out);
    return check_launch();
}

int resample_seg(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, const float *src,
                 float *dst, float *d_out, int64_t *ids, int32_t *q_out, int64_t chw, const ResampleOpts *opts,
                 hipStream_t s)
{
    const ResampleOpts o = opts ? *opts : ResampleOpts{};
    const bool vec = vec_ok(chw, {src, dst});
    const int64_t units = vec ? chw / 4 : chw;
    const int64_t per_block = (int64_t)kThreads * (vec ? kResampleVecPer : kResampleScalarPer);
    const dim3 grid((unsigned)((units + per_block - 1) / per_block), (unsigned)(segments * k));
    const auto kernel = vec ? (opts ? k_resample_seg<4, kResampleVecPer, true> : k_resample_seg<4, kResampleVecPer, false>)
                            : (opts ? k_resample_seg<1, kResampleScalarPer, true>
                                    : k_resample_seg<1, kResampleScalarPer, false>);
    kernel<<<grid, kThreads, (size_t)k * sizeof(unsigned long long), s>>>(
        d, u, (int)k, inv_scale, src, dst, d_out, ids, q_out, units, o.scheme, o.ess_q16, o.flag_out, o.ess_out);
    return check_launch();
}

}  // namespace dpsx
