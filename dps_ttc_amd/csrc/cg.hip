// Vector side of the per-particle conjugate-gradient data-consistency step (include/dpsx.h: dpsx_cg_step_f32).
//
// A and A^T are the operators' plain forward / adjoint launches; the kernels here are the streams between them:
//   k_cg_init     p = r,                                  ||r||^2 partials
//   k_cg_sumsq    ||t||^2 partials                        (t = A p, measurement-sized)
//   k_cg_update   alpha (prologue); d += alpha p; r -= alpha (s + rho p); ||r||^2 partials
//   k_cg_pupdate  beta (prologue);  p = r + beta p;       ||p||^2 partials (the next iteration's rho ||p||^2)
//   k_cg_final    alpha (prologue); x_next = sample + kappa (d + alpha p)       (the last iteration: no r, p update)
//
// Reductions: grid (slots, n); block (q, p) owns a contiguous range of particle p and leaves ONE fp32 partial (the
// fixed tree of block_sum) in slot q.  The slot count depends on the particle size only (cg_slots), so a particle's
// sums do not depend on the batch it runs in.  The consumer launch's prologue adds a particle's slots in double with
// common.h's slots_sum (lane-strided, fixed shuffle tree); every block of a particle gets the same bits.
// No atomics, no fences: launch boundaries order the partials.  Everything a particle reads is its own, so a
// non-finite value stays inside its particle.
//
// Units: 16 bytes per lane where the particle size is a multiple of 4 and the buffers are 16-byte aligned (every
// particle's base is then aligned too); otherwise the scalar instantiation of the same body (chosen on the host).
// A unit's loads are issued before the prologue and before its arithmetic; streams read for the last time are
// non-temporal loads.
#include "common.h"

#include <algorithm>

namespace dpsx {

namespace {

constexpr int kCgThreads = 256;
constexpr int kCgMaxSlots = 256;

typedef float cg_f4 __attribute__((ext_vector_type(4)));

template <bool VEC> struct CgUnit { typedef float T; static constexpr int W = 1; };
template <> struct CgUnit<true> { typedef cg_f4 T; static constexpr int W = 4; };

__device__ __forceinline__ float cg_sq(float x, float acc) { return fmaf(x, x, acc); }
__device__ __forceinline__ float cg_sq(cg_f4 x, float acc)
{
    acc = fmaf(x.x, x.x, acc);
    acc = fmaf(x.y, x.y, acc);
    acc = fmaf(x.z, x.z, acc);
    return fmaf(x.w, x.w, acc);
}

template <class T> __device__ __forceinline__ T cg_ld(const float *p) { return *reinterpret_cast<const T *>(p); }
template <class T> __device__ __forceinline__ T cg_ld_last(const float *p)
{
    return __builtin_nontemporal_load(reinterpret_cast<const T *>(p));
}
template <class T> __device__ __forceinline__ void cg_st(float *p, T v) { *reinterpret_cast<T *>(p) = v; }

// alpha = rs / (||t||^2 + rho ||p||^2), formed in double, rounded once.  out[0] = alpha, out[1] = rs, out[2] = pq;
// called by all threads, valid after the next __syncthreads()
__device__ __forceinline__ void cg_alpha_to_lds(const float *rs, const float *tt, const float *pp, int slots, int slots_m,
                                                float rho, float *out)
{
    if (threadIdx.x < kWave) {
        const double a = slots_sum(rs, slots), b = slots_sum(tt, slots_m), c = slots_sum(pp, slots);
        if (threadIdx.x == 0) {
            const double pq = b + (double)rho * c;
            out[0] = (float)(pq > 0.0 ? a / pq : 0.0);
            out[1] = (float)a;
            out[2] = (float)pq;
        }
    }
}

struct CgRange { int64_t lo, hi; };
__device__ __forceinline__ CgRange cg_range(int64_t units, int64_t per)
{
    const int64_t lo = (int64_t)blockIdx.x * per;
    return CgRange{lo, min(units, lo + per)};
}

// ------------------------------------------------------------------ p = r, ||r||^2
template <bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_init(const float *__restrict__ r, float *__restrict__ p,
                                                        float *__restrict__ rs_part, int64_t e, int64_t per)
{
    using T = typename CgUnit<VEC>::T;
    constexpr int W = CgUnit<VEC>::W;
    __shared__ float red[kCgThreads / kWave];
    const int64_t base = (int64_t)blockIdx.y * e;
    const CgRange g = cg_range(e / W, per);
    float acc = 0.0f;
    for (int64_t u = g.lo + threadIdx.x; u < g.hi; u += kCgThreads) {
        const T v = cg_ld<T>(r + base + u * W);
        cg_st<T>(p + base + u * W, v);
        acc = cg_sq(v, acc);
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) rs_part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// ------------------------------------------------------------------ ||t||^2 (t is read for the last time)
template <bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_sumsq(const float *__restrict__ t, float *__restrict__ part,
                                                         int64_t m, int64_t per)
{
    using T = typename CgUnit<VEC>::T;
    constexpr int W = CgUnit<VEC>::W;
    __shared__ float red[kCgThreads / kWave];
    const int64_t base = (int64_t)blockIdx.y * m;
    const CgRange g = cg_range(m / W, per);
    float acc = 0.0f;
    for (int64_t u = g.lo + threadIdx.x; u < g.hi; u += kCgThreads) acc = cg_sq(cg_ld_last<T>(t + base + u * W), acc);
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ------------------------------------------------------------------ d += alpha p ; r -= alpha (s + rho p) ; ||r||^2
// first: d is zero and not read (iteration one)
template <bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_update(float *__restrict__ d, const float *__restrict__ p,
                                                          float *__restrict__ r, const float *__restrict__ s,
                                                          const float *__restrict__ rs_old, const float *__restrict__ tt,
                                                          const float *__restrict__ pp, float *__restrict__ rs_new,
                                                          float *__restrict__ scal, float rho, int first, int slots_m,
                                                          int64_t e, int64_t per)
{
    using T = typename CgUnit<VEC>::T;
    constexpr int W = CgUnit<VEC>::W;
    __shared__ float red[kCgThreads / kWave];
    __shared__ float sc[3];
    const int64_t q = blockIdx.y, base = q * e;
    const int slots = gridDim.x;
    const CgRange g = cg_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T dv = T{}, pv = T{}, rv = T{}, sv = T{};
    if (u < g.hi) {
        const int64_t o = base + u * W;
        if (!first) dv = cg_ld<T>(d + o);
        pv = cg_ld<T>(p + o);
        rv = cg_ld<T>(r + o);
        sv = cg_ld_last<T>(s + o);
    }
    cg_alpha_to_lds(rs_old + q * slots, tt + q * slots_m, pp + q * slots, slots, slots_m, rho, sc);
    __syncthreads();
    const float alpha = sc[0];
    float acc = 0.0f;
    while (u < g.hi) {
        const int64_t o = base + u * W;
        const T ap = alpha * pv;
        const T dn = first ? ap : dv + ap;
        const T rn = rv - alpha * (sv + rho * pv);
        cg_st<T>(d + o, dn);
        cg_st<T>(r + o, rn);
        acc = cg_sq(rn, acc);
        u += kCgThreads;
        if (u < g.hi) {
            const int64_t o2 = base + u * W;
            if (!first) dv = cg_ld<T>(d + o2);
            pv = cg_ld<T>(p + o2);
            rv = cg_ld<T>(r + o2);
            sv = cg_ld_last<T>(s + o2);
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) {
        rs_new[q * slots + blockIdx.x] = t;
        if (blockIdx.x == 0) {
            scal[q * 4 + 0] = sc[1];
            scal[q * 4 + 1] = sc[2];
            scal[q * 4 + 2] = alpha;
        }
    }
}

// ------------------------------------------------------------------ p = r + beta p ; ||p||^2
template <bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_pupdate(const float *__restrict__ r, float *__restrict__ p,
                                                           const float *__restrict__ rs_old,
                                                           const float *__restrict__ rs_new, float *__restrict__ pp,
                                                           float *__restrict__ scal, int64_t e, int64_t per)
{
    using T = typename CgUnit<VEC>::T;
    constexpr int W = CgUnit<VEC>::W;
    __shared__ float red[kCgThreads / kWave];
    __shared__ float sc[1];
    const int64_t q = blockIdx.y, base = q * e;
    const int slots = gridDim.x;
    const CgRange g = cg_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T pv = T{}, rv = T{};
    if (u < g.hi) {
        rv = cg_ld<T>(r + base + u * W);
        pv = cg_ld<T>(p + base + u * W);
    }
    if (threadIdx.x < kWave) {
        const double a = slots_sum(rs_old + q * slots, slots), b = slots_sum(rs_new + q * slots, slots);
        if (threadIdx.x == 0) sc[0] = (float)(a > 0.0 ? b / a : 0.0);
    }
    __syncthreads();
    const float beta = sc[0];
    float acc = 0.0f;
    while (u < g.hi) {
        const T pn = rv + beta * pv;
        cg_st<T>(p + base + u * W, pn);
        acc = cg_sq(pn, acc);
        u += kCgThreads;
        if (u < g.hi) {
            rv = cg_ld<T>(r + base + u * W);
            pv = cg_ld<T>(p + base + u * W);
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) {
        pp[q * slots + blockIdx.x] = t;
        if (blockIdx.x == 0) scal[q * 4 + 3] = beta;
    }
}

// ------------------------------------------------------------------ x_next = sample + kappa (d + alpha p)
// x_next may be sample, d_out (nullable) may be d: each lane reads its unit before it writes it, so no __restrict__ there
template <bool VEC>
__global__ __launch_bounds__(kCgThreads) void k_cg_final(const float *sample, const float *d, const float *__restrict__ p,
                                                         float *x_next, float *d_out, const float *__restrict__ rs,
                                                         const float *__restrict__ tt, const float *__restrict__ pp,
                                                         float *__restrict__ scal, float rho, float kappa, int first,
                                                         int slots, int slots_m, int64_t e, int64_t per)
{
    using T = typename CgUnit<VEC>::T;
    constexpr int W = CgUnit<VEC>::W;
    __shared__ float sc[3];
    const int64_t q = blockIdx.y, base = q * e;
    const CgRange g = cg_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T dv = T{}, pv = T{}, sv = T{};
    if (u < g.hi) {
        const int64_t o = base + u * W;
        if (!first) dv = cg_ld_last<T>(d + o);
        pv = cg_ld_last<T>(p + o);
        sv = cg_ld_last<T>(sample + o);
    }
    cg_alpha_to_lds(rs + q * slots, tt + q * slots_m, pp + q * slots, slots, slots_m, rho, sc);
    __syncthreads();
    const float alpha = sc[0];
    while (u < g.hi) {
        const int64_t o = base + u * W;
        const T ap = alpha * pv;
        const T dn = first ? ap : dv + ap;
        if (d_out) cg_st<T>(d_out + o, dn);
        cg_st<T>(x_next + o, sv + kappa * dn);
        u += kCgThreads;
        if (u < g.hi) {
            const int64_t o2 = base + u * W;
            if (!first) dv = cg_ld_last<T>(d + o2);
            pv = cg_ld_last<T>(p + o2);
            sv = cg_ld_last<T>(sample + o2);
        }
    }
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        scal[q * 4 + 0] = sc[1];
        scal[q * 4 + 1] = sc[2];
        scal[q * 4 + 2] = alpha;
    }
}

bool all_aligned16(std::initializer_list<const void *> ptrs)
{
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return false;
    return true;
}

// work items (float4 units or elements) per block: the particle's items split evenly over its slots
int64_t cg_per_block(int64_t e, bool vec)
{
    const int64_t units = vec ? e / 4 : e, slots = cg_slots(e);
    return (units + slots - 1) / slots;
}

}  // namespace

int cg_slots(int64_t e) { return (int)std::min<int64_t>(kCgMaxSlots, std::max<int64_t>(1, (e + 1023) / 1024)); }

int cg_init(const float *r, float *p, float *rs_part, int64_t n, int64_t e, hipStream_t s)
{
    const bool vec = e % 4 == 0 && all_aligned16({r, p});
    const dim3 grid((unsigned)cg_slots(e), (unsigned)n);
    if (vec) k_cg_init<true><<<grid, kCgThreads, 0, s>>>(r, p, rs_part, e, cg_per_block(e, true));
    else k_cg_init<false><<<grid, kCgThreads, 0, s>>>(r, p, rs_part, e, cg_per_block(e, false));
    return check_launch();
}

int cg_sumsq(const float *t, float *part, int64_t n, int64_t m, hipStream_t s)
{
    const bool vec = m % 4 == 0 && aligned16(t);
    const dim3 grid((unsigned)cg_slots(m), (unsigned)n);
    if (vec) k_cg_sumsq<true><<<grid, kCgThreads, 0, s>>>(t, part, m, cg_per_block(m, true));
    else k_cg_sumsq<false><<<grid, kCgThreads, 0, s>>>(t, part, m, cg_per_block(m, false));
    return check_launch();
}

int cg_update(float *d, const float *p, float *r, const float *sv, const float *rs_old, const float *tt, const float *pp,
              float *rs_new, float *scal, float rho, bool first, int64_t n, int64_t e, int64_t m, hipStream_t s)
{
    const bool vec = e % 4 == 0 && all_aligned16({d, p, r, sv});
    const dim3 grid((unsigned)cg_slots(e), (unsigned)n);
    if (vec)
        k_cg_update<true><<<grid, kCgThreads, 0, s>>>(d, p, r, sv, rs_old, tt, pp, rs_new, scal, rho, first, cg_slots(m), e,
                                                      cg_per_block(e, true));
    else
        k_cg_update<false><<<grid, kCgThreads, 0, s>>>(d, p, r, sv, rs_old, tt, pp, rs_new, scal, rho, first, cg_slots(m), e,
                                                       cg_per_block(e, false));
    return check_launch();
}

int cg_pupdate(const float *r, float *p, const float *rs_old, const float *rs_new, float *pp, float *scal, int64_t n,
               int64_t e, hipStream_t s)
{
    const bool vec = e % 4 == 0 && all_aligned16({r, p});
    const dim3 grid((unsigned)cg_slots(e), (unsigned)n);
    if (vec) k_cg_pupdate<true><<<grid, kCgThreads, 0, s>>>(r, p, rs_old, rs_new, pp, scal, e, cg_per_block(e, true));
    else k_cg_pupdate<false><<<grid, kCgThreads, 0, s>>>(r, p, rs_old, rs_new, pp, scal, e, cg_per_block(e, false));
    return check_launch();
}

int cg_final(const float *sample, const float *d, const float *p, float *x_next, float *d_out, const float *rs,
             const float *tt, const float *pp, float *scal, float rho, float kappa, bool first, int64_t n, int64_t e,
             int64_t m, hipStream_t s)
{
    const bool vec = e % 4 == 0 && all_aligned16({sample, d, p, x_next, d_out});
    const dim3 grid((unsigned)cg_slots(e), (unsigned)n);
    if (vec)
        k_cg_final<true><<<grid, kCgThreads, 0, s>>>(sample, d, p, x_next, d_out, rs, tt, pp, scal, rho, kappa, first,
                                                     cg_slots(e), cg_slots(m), e, cg_per_block(e, true));
    else
        k_cg_final<false><<<grid, kCgThreads, 0, s>>>(sample, d, p, x_next, d_out, rs, tt, pp, scal, rho, kappa, first,
                                                      cg_slots(e), cg_slots(m), e, cg_per_block(e, false));
    return check_launch();
}

}  // namespace dpsx
