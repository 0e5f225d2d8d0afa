// The per-particle slotted pass of cg.hip, smc.hip, dsg.hip, dpmpp.hip and metrics.hip (repulse.hip, whose blocks own particle tiles, takes
// the units, the loads, the block range and the host rules from here; no other translation unit includes this header).
//
// Grid (slots, n): block (q, p) owns one contiguous range of particle p's work items and leaves its partial sums in slot
// q; slots = cg_slots(size) is a function of the particle size only, so a particle's partials do not depend on the batch it
// runs in.  The consumer adds a particle's slots in double in a fixed order (common.h: slots_sum).  No atomics, no fences:
// launch boundaries order the partials.  Everything a particle reads is its own, so a non-finite value stays inside it.
//
// Work items are units of 16 bytes per lane where the particle size is a multiple of 4 and every buffer read or written is
// 16-byte aligned (every particle's base is then aligned too), else single elements: the scalar instantiation of the same
// body, chosen on the host (common.h: vec_ok).
#pragma once

#include "common.h"

#include <type_traits>

namespace dpsx {

constexpr int kPassThreads = 256;

typedef float f4 __attribute__((ext_vector_type(4)));

template <bool VEC> struct Unit { typedef float T; static constexpr int W = 1; };
template <> struct Unit<true> { typedef f4 T; static constexpr int W = 4; };

__device__ __forceinline__ float lane(float v, int) { return v; }
__device__ __forceinline__ float lane(const f4 &v, int j) { return v[j]; }
__device__ __forceinline__ void set(float &v, int, float x) { v = x; }
__device__ __forceinline__ void set(f4 &v, int j, float x) { v[j] = x; }

// LAST: the stream is read for the last time of its step (a non-temporal load)
template <class T, bool LAST = false> __device__ __forceinline__ T ld(const float *p)
{
    if constexpr (LAST) return __builtin_nontemporal_load(reinterpret_cast<const T *>(p));
    else return *reinterpret_cast<const T *>(p);
}
template <class T> __device__ __forceinline__ T ld_last(const float *p) { return ld<T, true>(p); }
template <class T> __device__ __forceinline__ void st(float *p, T v) { *reinterpret_cast<T *>(p) = v; }

// the noise of unit u (VEC) / element u (scalar) of the particle with id pid: S1's draw (k_posterior_fwd and the fused K1s)
template <bool VEC> __device__ __forceinline__ typename Unit<VEC>::T draw(const RngK &r, int64_t u, uint32_t pid)
{
    if constexpr (VEC) {
        const float4 z = rng_unit(r, (uint32_t)u, pid);
        return f4{z.x, z.y, z.z, z.w};
    } else {
        return rng_elem(r, u, pid);
    }
}

// the block's work items [lo, hi) of its particle's `units`, `per` to a block
struct Range { int64_t lo, hi; };
__device__ __forceinline__ Range block_range(int64_t units, int64_t per)
{
    const int64_t lo = (int64_t)blockIdx.x * per;
    return Range{lo, min(units, lo + per)};
}

// ------------------------------------------------------------------ host side
// the launch geometry: the particle's work items (float4 units or elements) split evenly over its slots
struct PassGeom { int64_t per; dim3 grid; };
inline PassGeom pass_geom(int64_t size, bool vec, int64_t n)
{
    const int64_t units = vec ? size / 4 : size, slots = cg_slots(size);
    return PassGeom{(units + slots - 1) / slots, dim3((unsigned)slots, (unsigned)n)};
}

// run-time flags -> template arguments: f(V) / f(V, R) with std::bool_constant values, e.g.
//     dispatch(vec, use_rng, [&](auto V, auto R) { k<V.value, R.value><<<...>>>(...); return check_launch(); })
template <class F> int dispatch(bool vec, F &&f) { return vec ? f(std::true_type{}) : f(std::false_type{}); }
template <class F> int dispatch(bool vec, bool use_rng, F &&f)
{
    return dispatch(vec, [&](auto V) { return dispatch(use_rng, [&](auto R) { return f(V, R); }); });
}

// ------------------------------------------------------------------ the update streams (smc.hip, dsg.hip, dpmpp.hip)
// K3's inputs as the launches in K3's place read them.  Per element e of particle p, every operation one fp32 rounding:
//     s_e  = ratio g_eps_e + g_unet_e                    g_unet absent: + 0.0f
//     sd_e = __expf(0.5f post_logvar(v_e))               DDPM record (S1's device functions); DDIM record: sd_e = min_log
//     n_e  = sd_e z_e                                    z from `z`, or draw<VEC> with S1's counters
struct UpdateArgs {
    const float *sample, *g_mo, *gu, *mo, *z;
    float *out, *part;      // part: the launch's partials, [n, slots] (smc.hip) or [n, slots, 4] (dsg.hip)
    int64_t chw, per;       // per: work items per block
    float ratio, rate;      // -a / b; dsg's guidance rate
    Coefs k;
    RngK rng;
};

// the record, the form and the grid of a launch over them
struct UpdatePass { UpdateArgs a; dim3 grid; bool vec; };
inline UpdatePass update_pass(const float *sample, const float *g_mo, const float *g_unet, const float *mo, const float *z,
                              bool use_rng, const RngK &r, float rate, float *x_next, float *part, int64_t n, int64_t chw,
                              const Coefs &k)
{
    const bool noisy = k.add_noise & 1;                    // a step without noise reads neither the variance nor z
    const bool vec = vec_ok(chw, {sample, g_mo, g_unet, x_next, noisy ? mo : nullptr, noisy && !use_rng ? z : nullptr});
    const PassGeom g = pass_geom(chw, vec, n);
    return UpdatePass{{sample, g_mo, g_unet, mo, z, x_next, part, chw, g.per, -k.a / k.b, rate, k, r}, g.grid, vec};
}

__device__ __forceinline__ float update_s(float g, float u, const UpdateArgs &a)
{
    return __fadd_rn(__fmul_rn(a.ratio, g), u);            // k_step_update's expression (elementwise.hip)
}
__device__ __forceinline__ float update_sd(float v, bool ddim, const UpdateArgs &a)
{
    return ddim ? a.k.min_log : __expf(__fmul_rn(0.5f, post_logvar(v, a.k)));
}
// s, sd and n of one element of a step with noise (k_step_update_corr, which also runs the step without, takes the parts)
__device__ __forceinline__ void update_elem(float g, float u, float v, float z, bool ddim, const UpdateArgs &a, float &s,
                                            float &sd, float &nz)
{
    s = update_s(g, u, a);
    sd = update_sd(v, ddim, a);
    nz = __fmul_rn(sd, z);
}

// one unit of particle p's streams, each load issued where load() is called: [sample,] g_eps, g_unet, the variance, z.
// SAMPLE: `sample` is read too; LAST: this launch is the streams' last reader of the step; noisy / ddim: launch-uniform
template <bool VEC, bool RNG, bool SAMPLE, bool LAST> struct UpdateLoader {
    using T = typename Unit<VEC>::T;
    static constexpr int W = Unit<VEC>::W;
    const UpdateArgs &a;
    const int64_t base, mbase;
    const bool has_u, ld_v, ld_z;
    T sv = T{}, gv = T{}, uv = T{}, vv = T{}, zv = T{};
    __device__ __forceinline__ UpdateLoader(const UpdateArgs &args, int64_t p, bool noisy, bool ddim)
        : a(args), base(p * args.chw), mbase(p * 2 * args.chw), has_u(args.gu != nullptr), ld_v(noisy && !ddim),
          ld_z(noisy && !RNG) {}
    __device__ __forceinline__ void load(int64_t unit)
    {
        const int64_t i = unit * W;
        if constexpr (SAMPLE) sv = ld<T, LAST>(a.sample + base + i);
        gv = ld<T, LAST>(a.g_mo + mbase + i);
        if (has_u) uv = ld<T, LAST>(a.gu + base + i);
        if (ld_v) vv = ld<T, LAST>(a.mo + mbase + a.chw + i);
        if (ld_z) zv = ld<T, LAST>(a.z + base + i);
    }
};

}  // namespace dpsx
