// Vector side of the per-particle conjugate-gradient data-consistency step (include/dpsx.h: dpsx_cg_step_f32).
//
// A and A^T are the operators' plain forward / adjoint launches; the kernels here are the streams between them:
//   k_cg_init     p = r,                                  ||r||^2 partials
//   k_cg_sumsq    ||t||^2 partials                        (t = A p, measurement-sized)
//   k_cg_update   alpha (prologue); d += alpha p; r -= alpha (s + rho p); ||r||^2 partials
//   k_cg_pupdate  beta (prologue);  p = r + beta p;       ||p||^2 partials (the next iteration's rho ||p||^2)
//   k_cg_final    alpha (prologue); x_next = sample + kappa (d + alpha p)       (the last iteration: no r, p update)
//   k_cg_pullback alpha (prologue); g_eps = inside ? gain (d + alpha p) : +0    (dpsx_cg_pullback_f32's last launch)
//
// Every launch is particle_pass.h's per-particle slotted pass: one fp32 partial per block (the fixed tree of block_sum) in
// its slot; the consumer launch's prologue adds a particle's slots in double with common.h's slots_sum (lane-strided,
// fixed shuffle tree), so every block of a particle gets the same bits.  A unit's loads are issued before the prologue
// and before its arithmetic; streams read for the last time are non-temporal loads.
#include "particle_pass.h"

#include <algorithm>

namespace dpsx {

namespace {

constexpr int kCgMaxSlots = 256;

__device__ __forceinline__ float cg_sq(float x, float acc) { return fmaf(x, x, acc); }
__device__ __forceinline__ float cg_sq(f4 x, float acc)
{
    acc = fmaf(x.x, x.x, acc);
    acc = fmaf(x.y, x.y, acc);
    acc = fmaf(x.z, x.z, acc);
    return fmaf(x.w, x.w, acc);
}

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

// ------------------------------------------------------------------ p = r, ||r||^2
template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_cg_init(const float *__restrict__ r, float *__restrict__ p,
                                                        float *__restrict__ rs_part, int64_t e, int64_t per)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float red[kPassThreads / kWave];
    const int64_t base = (int64_t)blockIdx.y * e;
    const Range g = block_range(e / W, per);
    float acc = 0.0f;
    for (int64_t u = g.lo + threadIdx.x; u < g.hi; u += kPassThreads) {
        const T v = ld<T>(r + base + u * W);
        st<T>(p + base + u * W, v);
        acc = cg_sq(v, acc);
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) rs_part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// ------------------------------------------------------------------ ||t||^2 (t is read for the last time)
template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_cg_sumsq(const float *__restrict__ t, float *__restrict__ part,
                                                         int64_t m, int64_t per)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float red[kPassThreads / kWave];
    const int64_t base = (int64_t)blockIdx.y * m;
    const Range g = block_range(m / W, per);
    float acc = 0.0f;
    for (int64_t u = g.lo + threadIdx.x; u < g.hi; u += kPassThreads) acc = cg_sq(ld_last<T>(t + base + u * W), acc);
    const float s = block_sum(acc, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

// ------------------------------------------------------------------ d += alpha p ; r -= alpha (s + rho p) ; ||r||^2
// first: d is zero and not read (iteration one)
template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_cg_update(float *__restrict__ d, const float *__restrict__ p,
                                                          float *__restrict__ r, const float *__restrict__ s,
                                                          const float *__restrict__ rs_old, const float *__restrict__ tt,
                                                          const float *__restrict__ pp, float *__restrict__ rs_new,
                                                          float *__restrict__ scal, float rho, int first, int slots_m,
                                                          int64_t e, int64_t per)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float red[kPassThreads / kWave];
    __shared__ float sc[3];
    const int64_t q = blockIdx.y, base = q * e;
    const int slots = gridDim.x;
    const Range g = block_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T dv = T{}, pv = T{}, rv = T{}, sv = T{};
    if (u < g.hi) {
        const int64_t o = base + u * W;
        if (!first) dv = ld<T>(d + o);
        pv = ld<T>(p + o);
        rv = ld<T>(r + o);
        sv = ld_last<T>(s + o);
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
        st<T>(d + o, dn);
        st<T>(r + o, rn);
        acc = cg_sq(rn, acc);
        u += kPassThreads;
        if (u < g.hi) {
            const int64_t o2 = base + u * W;
            if (!first) dv = ld<T>(d + o2);
            pv = ld<T>(p + o2);
            rv = ld<T>(r + o2);
            sv = ld_last<T>(s + o2);
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
__global__ __launch_bounds__(kPassThreads) void k_cg_pupdate(const float *__restrict__ r, float *__restrict__ p,
                                                           const float *__restrict__ rs_old,
                                                           const float *__restrict__ rs_new, float *__restrict__ pp,
                                                           float *__restrict__ scal, int64_t e, int64_t per)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float red[kPassThreads / kWave];
    __shared__ float sc[1];
    const int64_t q = blockIdx.y, base = q * e;
    const int slots = gridDim.x;
    const Range g = block_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T pv = T{}, rv = T{};
    if (u < g.hi) {
        rv = ld<T>(r + base + u * W);
        pv = ld<T>(p + base + u * W);
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
        st<T>(p + base + u * W, pn);
        acc = cg_sq(pn, acc);
        u += kPassThreads;
        if (u < g.hi) {
            rv = ld<T>(r + base + u * W);
            pv = ld<T>(p + base + u * W);
        }
    }
    const float t = block_sum(acc, red);
    if (threadIdx.x == 0) {
        pp[q * slots + blockIdx.x] = t;
        if (blockIdx.x == 0) scal[q * 4 + 3] = beta;
    }
}

// ------------------------------------------------------------------ the last iteration (k_cg_final, k_cg_pullback)
// the prologue both finishers share: alpha into sc (cg_alpha_to_lds), the barrier, and the particle's scalars left by its
// first block; -> alpha
__device__ __forceinline__ float cg_last_alpha(const float *rs, const float *tt, const float *pp, float *scal, float *sc,
                                               float rho, int slots, int slots_m, int64_t q)
{
    cg_alpha_to_lds(rs + q * slots, tt + q * slots_m, pp + q * slots, slots, slots_m, rho, sc);
    __syncthreads();
    const float alpha = sc[0];
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        scal[q * 4 + 0] = sc[1];
        scal[q * 4 + 1] = sc[2];
        scal[q * 4 + 2] = alpha;
    }
    return alpha;
}

// d of the last iteration: d + alpha p, two roundings (first: d is zero and was not read)
template <class T> __device__ __forceinline__ T cg_last_d(T dv, T pv, float alpha, int first)
{
    const T ap = alpha * pv;
    return first ? ap : dv + ap;
}

// ------------------------------------------------------------------ x_next = sample + kappa (d + alpha p)
// x_next may be sample, d_out (nullable) may be d: each lane reads its unit before it writes it, so no __restrict__ there
template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_cg_final(const float *sample, const float *d, const float *__restrict__ p,
                                                         float *x_next, float *d_out, const float *__restrict__ rs,
                                                         const float *__restrict__ tt, const float *__restrict__ pp,
                                                         float *__restrict__ scal, float rho, float kappa, int first,
                                                         int slots, int slots_m, int64_t e, int64_t per)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float sc[3];
    const int64_t q = blockIdx.y, base = q * e;
    const Range g = block_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T dv = T{}, pv = T{}, sv = T{};
    if (u < g.hi) {
        const int64_t o = base + u * W;
        if (!first) dv = ld_last<T>(d + o);
        pv = ld_last<T>(p + o);
        sv = ld_last<T>(sample + o);
    }
    const float alpha = cg_last_alpha(rs, tt, pp, scal, sc, rho, slots, slots_m, q);
    while (u < g.hi) {
        const int64_t o = base + u * W;
        const T dn = cg_last_d(dv, pv, alpha, first);
        if (d_out) st<T>(d_out + o, dn);
        st<T>(x_next + o, sv + kappa * dn);
        u += kPassThreads;
        if (u < g.hi) {
            const int64_t o2 = base + u * W;
            if (!first) dv = ld_last<T>(d + o2);
            pv = ld_last<T>(p + o2);
            sv = ld_last<T>(sample + o2);
        }
    }
}

// ------------------------------------------------------------------ g_eps = inside ? gain (d + alpha p) : +0
// The cotangent on the model's eps output in k_cg_final's place: the eps half of g_model_out [n, 2 chw] (the variance half is
// not touched).  The gate is read 4 bytes per unit (VEC) or one byte per element; d and p are read for the last time.
// d_out (nullable) may be d: each lane reads its unit before it writes it
template <bool VEC> struct Gate { typedef uint8_t T; };
template <> struct Gate<true> { typedef uchar4 T; };
__device__ __forceinline__ float cg_gated(uint8_t in, float gain, float dn) { return in ? gain * dn : 0.0f; }
__device__ __forceinline__ f4 cg_gated(uchar4 in, float gain, f4 dn)
{
    return f4{cg_gated(in.x, gain, dn.x), cg_gated(in.y, gain, dn.y), cg_gated(in.z, gain, dn.z), cg_gated(in.w, gain, dn.w)};
}

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_cg_pullback(const float *d, const float *__restrict__ p,
                                                            const uint8_t *__restrict__ inside, float *__restrict__ g_mo,
                                                            float *d_out, const float *__restrict__ rs,
                                                            const float *__restrict__ tt, const float *__restrict__ pp,
                                                            float *__restrict__ scal, float rho, float gain, int first,
                                                            int slots, int slots_m, int64_t e, int64_t per)
{
    using T = typename Unit<VEC>::T;
    using G = typename Gate<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ float sc[3];
    const int64_t q = blockIdx.y, base = q * e, mbase = q * 2 * e;
    const Range g = block_range(e / W, per);
    int64_t u = g.lo + threadIdx.x;
    T dv = T{}, pv = T{};
    G in = G{};
    if (u < g.hi) {
        const int64_t o = base + u * W;
        if (!first) dv = ld_last<T>(d + o);
        pv = ld_last<T>(p + o);
        in = *reinterpret_cast<const G *>(inside + o);
    }
    const float alpha = cg_last_alpha(rs, tt, pp, scal, sc, rho, slots, slots_m, q);
    while (u < g.hi) {
        const int64_t i = u * W;
        const T dn = cg_last_d(dv, pv, alpha, first);
        if (d_out) st<T>(d_out + base + i, dn);
        st<T>(g_mo + mbase + i, cg_gated(in, gain, dn));
        u += kPassThreads;
        if (u < g.hi) {
            const int64_t o2 = base + u * W;
            if (!first) dv = ld_last<T>(d + o2);
            pv = ld_last<T>(p + o2);
            in = *reinterpret_cast<const G *>(inside + o2);
        }
    }
}

}  // namespace

int cg_slots(int64_t e) { return (int)std::min<int64_t>(kCgMaxSlots, std::max<int64_t>(1, (e + 1023) / 1024)); }

int cg_init(const float *r, float *p, float *rs_part, int64_t n, int64_t e, hipStream_t s)
{
    const bool vec = vec_ok(e, {r, p});
    const PassGeom g = pass_geom(e, vec, n);
    return dispatch(vec, [&](auto V) {
        k_cg_init<V.value><<<g.grid, kPassThreads, 0, s>>>(r, p, rs_part, e, g.per);
        return check_launch();
    });
}

int cg_sumsq(const float *t, float *part, int64_t n, int64_t m, hipStream_t s)
{
    const bool vec = vec_ok(m, {t});
    const PassGeom g = pass_geom(m, vec, n);
    return dispatch(vec, [&](auto V) {
        k_cg_sumsq<V.value><<<g.grid, kPassThreads, 0, s>>>(t, part, m, g.per);
        return check_launch();
    });
}

int cg_update(float *d, const float *p, float *r, const float *sv, const float *rs_old, const float *tt, const float *pp,
              float *rs_new, float *scal, float rho, bool first, int64_t n, int64_t e, int64_t m, hipStream_t s)
{
    const bool vec = vec_ok(e, {d, p, r, sv});
    const PassGeom g = pass_geom(e, vec, n);
    return dispatch(vec, [&](auto V) {
        k_cg_update<V.value><<<g.grid, kPassThreads, 0, s>>>(d, p, r, sv, rs_old, tt, pp, rs_new, scal, rho, first,
                                                             cg_slots(m), e, g.per);
        return check_launch();
    });
}

int cg_pupdate(const float *r, float *p, const float *rs_old, const float *rs_new, float *pp, float *scal, int64_t n,
               int64_t e, hipStream_t s)
{
    const bool vec = vec_ok(e, {r, p});
    const PassGeom g = pass_geom(e, vec, n);
    return dispatch(vec, [&](auto V) {
        k_cg_pupdate<V.value><<<g.grid, kPassThreads, 0, s>>>(r, p, rs_old, rs_new, pp, scal, e, g.per);
        return check_launch();
    });
}

int cg_final(const float *sample, const float *d, const float *p, float *x_next, float *d_out, const float *rs,
             const float *tt, const float *pp, float *scal, float rho, float kappa, bool first, int64_t n, int64_t e,
             int64_t m, hipStream_t s)
{
    const bool vec = vec_ok(e, {sample, d, p, x_next, d_out});
    const PassGeom g = pass_geom(e, vec, n);
    return dispatch(vec, [&](auto V) {
        k_cg_final<V.value><<<g.grid, kPassThreads, 0, s>>>(sample, d, p, x_next, d_out, rs, tt, pp, scal, rho, kappa, first,
                                                            cg_slots(e), cg_slots(m), e, g.per);
        return check_launch();
    });
}

int cg_pullback(const float *d, const float *p, const uint8_t *inside, float *g_mo, float *d_out, const float *rs,
                const float *tt, const float *pp, float *scal, float rho, float gain, bool first, int64_t n, int64_t e,
                int64_t m, hipStream_t s)
{
    const bool vec = vec_ok(e, {d, p, g_mo, d_out}) && aligned4(inside);
    const PassGeom g = pass_geom(e, vec, n);
    return dispatch(vec, [&](auto V) {
        k_cg_pullback<V.value><<<g.grid, kPassThreads, 0, s>>>(d, p, inside, g_mo, d_out, rs, tt, pp, scal, rho, gain, first,
                                                               cg_slots(e), cg_slots(m), e, g.per);
        return check_launch();
    });
}

}  // namespace dpsx
