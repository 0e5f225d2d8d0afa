// dpsx internal helpers (gfx950 only: wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../include/dpsx.h"

namespace dpsx {

constexpr int kWave = 64;

// -------------------------------------------------------------------- errors
void set_last_hip_error(hipError_t e);

inline int check_launch()
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_last_hip_error(e);
        return DPSX_ELAUNCH;
    }
    return DPSX_OK;
}

#define DPSX_HIP_TRY(expr)                                   \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) {                              \
            ::dpsx::set_last_hip_error(_e);                  \
            return _e == hipErrorOutOfMemory ? DPSX_ENOMEM : DPSX_ELAUNCH; \
        }                                                    \
    } while (0)

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }   // the clamp gate's bytes, read as uchar4

// THE rule of the 16-byte (float4) form of a launch: `size` -- the particle, the plane or the row, whatever the kernel
// steps through in units of four -- is a multiple of 4 and every buffer of the launch is 16-byte aligned; ptrs: every
// buffer read or written, null = not read (counts as aligned).  Sites with a further condition state it beside the call.
inline bool vec_ok(int64_t size, std::initializer_list<const void *> ptrs)
{
    if (size % 4) return false;
    for (const void *p : ptrs)
        if (p && !aligned16(p)) return false;
    return true;
}

// -------------------------------------------------------------------- host: workspaces and particle sets
// Every region of a caller-provided workspace starts on a 256-byte boundary of it.
inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

// Walks a workspace layout: take<T>(count) is the next region as a typed pointer and advances by align256(count * sizeof(T));
// bytes() is the total so far.  base == nullptr: sizes only (every pointer is null).  A layout is ONE function that takes
// its regions from a Carver, so a size query (null base) and the launch path (the caller's base) cannot disagree.
// Owns and allocates nothing.
class Carver {
public:
    explicit Carver(void *base) : base_(static_cast<char *>(base)) {}
    template <class T> T *take(int64_t count)
    {
        char *p = base_ ? base_ + off_ : nullptr;
        off_ += align256(count * (int64_t)sizeof(T));
        return reinterpret_cast<T *>(p);
    }
    int64_t bytes() const { return off_; }

private:
    char *base_;
    int64_t off_ = 0;
};

// a workspace of `bytes` at ws serves a call that needs `need`: what a size query returned, so a negative value is the
// query's refusal (DPSX_E*) and is passed on
inline int workspace_check(const void *ws, int64_t bytes, int64_t need)
{
    if (need < 0) return (int)need;
    return !ws || bytes < need || !aligned16(ws) ? DPSX_EWORKSPACE : DPSX_OK;
}

// THE shape rule of an image-major particle set: n particles of d elements each, `images` images of K = n / images
// consecutive particles.  images is a grid dimension and d is indexed in 32 bits; max_k is the family's limit on K;
// allow_empty: n == 0 is a valid (empty) set.
inline int particle_set_shape(int64_t n, int64_t d, int64_t images, int64_t max_k, bool allow_empty)
{
    if (n < (allow_empty ? 0 : 1) || d < 1 || images < 1 || n % images) return DPSX_EINVAL;
    if (n / images > max_k || images > 65535 || d > INT32_MAX) return DPSX_EUNSUPPORTED;
    return DPSX_OK;
}

// -------------------------------------------------------------------- host: launches with large dynamic LDS
// Dynamic LDS above 64 KiB needs the attribute once per kernel symbol: the kernel is a template argument, so every symbol
// has its own flag.  launch_lds<k_name<...>>(grid, threads, lds_bytes, stream, kernel arguments...)
constexpr int kMaxDynamicLds = 144 * 1024;
template <auto Kernel, class... Args>
int launch_lds(dim3 grid, unsigned threads, size_t lds, hipStream_t s, const Args &...args)
{
    static bool attr_done = false;
    if (!attr_done) {
        DPSX_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         kMaxDynamicLds));
        attr_done = true;
    }
    hipLaunchKernelGGL(Kernel, grid, dim3(threads), lds, s, args...);
    return check_launch();
}

// -------------------------------------------------------------------- host: an operator's device tables
// Owns the read-only tables an operator uploads when it is created and frees them when it goes.  upload() returns the
// device copy (one element is allocated for an empty table) or null after a failure; rc() is the first failure's code,
// so a constructor uploads everything and asks once.
class DeviceTables {
public:
    DeviceTables() = default;
    DeviceTables(const DeviceTables &) = delete;
    DeviceTables &operator=(const DeviceTables &) = delete;
    ~DeviceTables() { for (void *p : allocs_) (void)hipFree(p); }
    template <class T> const T *upload(const std::vector<T> &v)
    {
        void *p = nullptr;
        if (rc_ == DPSX_OK) rc_ = put(&p, v.data(), v.size() * sizeof(T));
        return rc_ == DPSX_OK ? static_cast<const T *>(p) : nullptr;
    }
    int rc() const { return rc_; }

private:
    int put(void **p, const void *src, size_t bytes)
    {
        DPSX_HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
        allocs_.push_back(*p);
        if (bytes) DPSX_HIP_TRY(hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice));
        return DPSX_OK;
    }
    std::vector<void *> allocs_;
    int rc_ = DPSX_OK;
};

// -------------------------------------------------------------------- S1 point math
// Reference op order, one rounding per ATen op (no FMA contraction), so the
// element-wise chain is bit-identical to torch eager:
//   posterior_mean_variance.py:120-123 (x0 from eps), :43-44 (clamp),
//   :116-118 (mean), :239-240 (log-variance), gaussian_diffusion.py:472-474.
struct Coefs {
    float a, b, c1, c2, min_log, max_log;
    int add_noise;
};

inline Coefs to_coefs(const dpsx_coefs *c)
{
    return Coefs{c->a, c->b, c->c1, c->c2, c->min_log, c->max_log, c->add_noise};
}

__device__ __forceinline__ float post_x0(float x, float e, const Coefs &c, bool &inside)
{
    float pre = __fsub_rn(__fmul_rn(c.a, x), __fmul_rn(c.b, e));
    inside = (pre >= -1.0f) && (pre <= 1.0f);
    return pre < -1.0f ? -1.0f : (pre > 1.0f ? 1.0f : pre);
}

__device__ __forceinline__ float post_logvar(float v, const Coefs &c)
{
    float frac = __fmul_rn(__fadd_rn(v, 1.0f), 0.5f);   // == (v + 1) / 2 bit for bit (exact scaling by 2^-1)
    return __fadd_rn(__fmul_rn(frac, c.max_log), __fmul_rn(__fsub_rn(1.0f, frac), c.min_log));
}

// add_noise: bit 0 = add the noise term (t != 0); bit 1 = DDIM step (gaussian_diffusion.py:479-509) with
// c1 = sqrt(abar_prev), c2 = sqrt(1 - abar_prev - sigma^2), min_log = sigma; eps is re-derived from the
// clamped x0_hat as predict_eps_from_x_start does (:506-509), one rounding per reference op.
__device__ __forceinline__ float post_sample(float x, float x0, float v, float z, const Coefs &c)
{
    if (c.add_noise & 2) {
        const float eps = __fdiv_rn(__fsub_rn(__fmul_rn(c.a, x), x0), c.b);
        const float mean = __fadd_rn(__fmul_rn(x0, c.c1), __fmul_rn(c.c2, eps));
        return (c.add_noise & 1) ? __fadd_rn(mean, __fmul_rn(c.min_log, z)) : mean;
    }
    float mean = __fadd_rn(__fmul_rn(c.c1, x0), __fmul_rn(c.c2, x));
    if (!c.add_noise) return mean;
    // exp(x) = 2^(x log2 e) on the transcendental unit (v_exp_f32); |x| <= ~10 here, error ~4e-7 relative
    float sd = __expf(__fmul_rn(0.5f, post_logvar(v, c)));
    return __fadd_rn(mean, __fmul_rn(sd, z));
}

// The same arithmetic on one float4 unit, two lanes of data per instruction: v_pk_mul_f32 / v_pk_add_f32 round each
// operation exactly as their scalar forms do (no contraction: -ffp-contract=off; scalar x vector broadcasts), so x0_hat,
// the clamp gate and the sample come out bit for bit as from post_x0 / post_sample -- at about half the vector
// instructions (the tap-list forward launch spent more of them on S1 and its loader than on its tap loop:
// profiles/r03_valu_taps.txt).  The gate test is |pre| <= 1: one compare with the abs modifier, false for NaN like the
// closed-interval pair.  DDIM records (a division per element) take the scalar forms.
typedef float s1v2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float s1_clamp(float pre) { return pre < -1.0f ? -1.0f : (pre > 1.0f ? 1.0f : pre); }

// (the coefficients are splat into explicit pairs from by-value scalars: taking them through the Coefs reference made the
// compiler keep the struct in scratch memory and reload it -- behind a vmcnt(0) that also drained the tile's loads)
__device__ __forceinline__ s1v2 s1_splat(float v) { return s1v2{v, v}; }
// a launch-uniform scalar, made opaque: without this the compiler turns a pair built from two adjacent Coefs fields into ONE
// 8-byte load of the struct -- which forces the by-value kernel argument into scratch memory (28 bytes per lane, reloaded
// behind s_waitcnt vmcnt(0), which also drains the tile's loads in flight: +11 us on the tap-list forward launch)
__device__ __forceinline__ float s1_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
__device__ __forceinline__ s1v2 s1_lo(s1v2 p) { return __builtin_shufflevector(p, p, 0, 0); }   // op_sel: no instruction
__device__ __forceinline__ s1v2 s1_hi(s1v2 p) { return __builtin_shufflevector(p, p, 1, 1); }

// x0_hat of a unit (halo units: no sample, no gate)
__device__ __forceinline__ float4 post_x0_unit(const float4 &x, const float4 &e, const float ca, const float cb)
{
    const s1v2 AB{s1_uniform(ca), s1_uniform(cb)};
    const s1v2 p0 = s1_lo(AB) * s1v2{x.x, x.y} - s1_hi(AB) * s1v2{e.x, e.y}, p1 = s1_lo(AB) * s1v2{x.z, x.w} - s1_hi(AB) * s1v2{e.z, e.w};
    return make_float4(s1_clamp(p0.x), s1_clamp(p0.y), s1_clamp(p1.x), s1_clamp(p1.y));
}
__device__ __forceinline__ float4 post_x0_unit(const float4 &x, const float4 &e, const Coefs &c)
{
    return post_x0_unit(x, e, c.a, c.b);
}

__device__ __forceinline__ void post_unit(const float4 &x, const float4 &e, const float4 &v, const float4 &z, const Coefs &c,
                                          float4 &x0, float4 &sm, uchar4 &gate)
{
    // the six coefficients as three register pairs; a packed instruction broadcasts either half of a pair (op_sel)
    const s1v2 AB{s1_uniform(c.a), s1_uniform(c.b)}, CC{s1_uniform(c.c1), s1_uniform(c.c2)}, LL{s1_uniform(c.max_log), s1_uniform(c.min_log)};
    const int mode = c.add_noise;
    const s1v2 xa{x.x, x.y}, xb{x.z, x.w};
    const s1v2 p0 = s1_lo(AB) * xa - s1_hi(AB) * s1v2{e.x, e.y}, p1 = s1_lo(AB) * xb - s1_hi(AB) * s1v2{e.z, e.w};
    gate = make_uchar4(fabsf(p0.x) <= 1.0f, fabsf(p0.y) <= 1.0f, fabsf(p1.x) <= 1.0f, fabsf(p1.y) <= 1.0f);
    x0 = make_float4(s1_clamp(p0.x), s1_clamp(p0.y), s1_clamp(p1.x), s1_clamp(p1.y));
    if (mode & 2) {                 // DDIM: launch-uniform
        sm = make_float4(post_sample(x.x, x0.x, v.x, z.x, c), post_sample(x.y, x0.y, v.y, z.y, c),
                         post_sample(x.z, x0.z, v.z, z.z, c), post_sample(x.w, x0.w, v.w, z.w, c));
        return;
    }
    const s1v2 m0 = s1_lo(CC) * s1v2{x0.x, x0.y} + s1_hi(CC) * xa, m1 = s1_lo(CC) * s1v2{x0.z, x0.w} + s1_hi(CC) * xb;
    if (!mode) {
        sm = make_float4(m0.x, m0.y, m1.x, m1.y);
        return;
    }
    const s1v2 one = s1_splat(1.0f), hlf = s1_splat(0.5f);
    const s1v2 f0 = (s1v2{v.x, v.y} + one) * hlf, f1 = (s1v2{v.z, v.w} + one) * hlf;
    const s1v2 h0 = hlf * (f0 * s1_lo(LL) + (one - f0) * s1_hi(LL)), h1 = hlf * (f1 * s1_lo(LL) + (one - f1) * s1_hi(LL));
    const s1v2 s0 = m0 + s1v2{__expf(h0.x), __expf(h0.y)} * s1v2{z.x, z.y};
    const s1v2 s1 = m1 + s1v2{__expf(h1.x), __expf(h1.y)} * s1v2{z.z, z.w};
    sm = make_float4(s0.x, s0.y, s1.x, s1.y);
}

// -------------------------------------------------------------------- counter-based normals (include/dpsx.h: dpsx_rng)
// Philox4x32-10 keyed on the seed; counter = (float4 unit inside the particle, particle id, step, tag); one call gives
// the four normals of one unit.  The ONLY implementation: the stand-alone fill and every in-kernel draw call this
// function, so a counter yields the same bits wherever it is evaluated (no contraction: -ffp-contract=off).
struct RngK {                  // launch form of dpsx_rng (by-value kernel argument -> SGPRs)
    uint32_t k0, k1, step, tag;
    uint32_t base, per;        // particle id of batch row p: base + (per ? p % per : p)
};

__device__ __forceinline__ uint32_t rng_particle(const RngK &r, unsigned p) { return r.base + (r.per ? p % r.per : p); }

__device__ __forceinline__ uint4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1;
        c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}

// Box-Muller on one word pair: u1 = ((ra >> 8) + 1) 2^-24 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1) (both exact in fp32);
// rad = sqrt(-2 ln u1) from v_log_f32 (log2; u1 >= 2^-24 is normal) and v_sqrt_f32; v_cos_f32 / v_sin_f32 take
// revolutions, so u2 feeds them as it is.  |z| <= sqrt(48 ln 2) = 5.77; no infinity, no NaN.
__device__ __forceinline__ void rng_pair(uint32_t ra, uint32_t rb, float &za, float &zb)
{
    const float u1 = __fmul_rn((float)((ra >> 8) + 1u), 0x1p-24f), u2 = __fmul_rn((float)(rb >> 8), 0x1p-24f);
    const float rad = __builtin_amdgcn_sqrtf(__fmul_rn(__builtin_amdgcn_logf(u1), -1.3862943611198906f));   // -2 ln 2
    za = __fmul_rn(rad, __builtin_amdgcn_cosf(u2));
    zb = __fmul_rn(rad, __builtin_amdgcn_sinf(u2));
}

__device__ __forceinline__ float4 rng_unit(const RngK &r, uint32_t unit, uint32_t particle, uint4 *bits = nullptr)
{
    const uint4 w = philox4x32_10(unit, particle, r.step, r.tag, r.k0, r.k1);
    if (bits) *bits = w;
    float4 z;
    rng_pair(w.x, w.y, z.x, z.y);
    rng_pair(w.z, w.w, z.z, z.w);
    return z;
}

// element e of a particle (scalar kernels): word e % 4 of unit e / 4
__device__ __forceinline__ float rng_elem(const RngK &r, int64_t e, uint32_t particle)
{
    const float4 z = rng_unit(r, (uint32_t)(e >> 2), particle);
    const int q = (int)(e & 3);
    return q == 0 ? z.x : (q == 1 ? z.y : (q == 2 ? z.z : z.w));
}

// -------------------------------------------------------------------- reductions
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;
}

// NaN-propagating minimum / maximum: torch's min / max return NaN if any element is NaN
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// Deterministic block sum (fixed shuffle tree, waves added in index order).
// Result valid in thread 0.  `scratch` holds >= blockDim.x/64 floats.
__device__ __forceinline__ float block_sum(float v, float *scratch)
{
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) scratch[wv] = v;
    __syncthreads();
    float t = 0.0f;
    if (threadIdx.x == 0)
        for (int i = 0; i < nw; ++i) t += scratch[i];
    return t;
}

// The shuffle tree that ends every fixed-order sum: 32 ... 1, result valid in lane 0.  In place, by reference: returning
// the sum by value compiled the backward blur kernels to other register counts.
__device__ __forceinline__ void wave_sum_f64(double &v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
}

// THE fixed-order sum of one particle's partial slots, in double: lane i adds slots i, i + 64, ... in index order, then
// wave_sum_f64.  The one definition: every finisher of a per-particle sum -- k_finalize_norm, the backward prologues, the
// in-launch norm, the cost finalisation, the CG scalars -- goes through it or, where the loads are unrolled by hand, adds
// in this order and ends in wave_sum_f64, so they all produce the same bits.
// Called by wave 0 (threadIdx.x < kWave); the result is valid in lane 0.  ld: how a slot is read (plain by default).
template <class Ld>
__device__ __forceinline__ double slots_sum(const float *slots, int cnt, Ld &&ld)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < cnt; i += kWave) acc += (double)ld(slots + i);
    wave_sum_f64(acc);
    return acc;
}
__device__ __forceinline__ double slots_sum(const float *slots, int cnt)
{
    return slots_sum(slots, cnt, [](const float *p) { return *p; });
}

// Per-particle norm from the per-block partial sums of squares the forward half left behind (slots_sum: every block of a
// particle -- and the stand-alone finalisation -- get the bit-identical value).  Called by all threads; the result is
// valid in *slot after the next __syncthreads().
__device__ __forceinline__ void particle_norm_to_lds(const float *partials, int parts, int64_t n, float *slot)
{
    if (threadIdx.x < kWave) {
        const double acc = slots_sum(partials + n * parts, parts);
        if (threadIdx.x == 0) *slot = (float)sqrt(acc);
    }
}

// The same value in two halves, so the partial loads fly together with the caller's tile loads instead of
// costing a memory round trip at the top of every block: *_issue starts them (wave 0, <= 4 per lane, fixed
// slots), *_reduce adds them in the order of slots_sum (adding the +0.0 of an absent slot is exact).
// Only for parts <= 4 * kWave (block-uniform test by the caller).
struct NormPartials { float v[4]; };
__device__ __forceinline__ NormPartials particle_norm_issue(const float *partials, int parts, int64_t n)
{
    NormPartials p;
    const float *base = partials + n * parts;
#pragma unroll
    for (int j = 0; j < 4; ++j)      // every lane loads (clamped address): no branch, nothing waits here
        p.v[j] = base[min((int)(threadIdx.x & (kWave - 1)) + j * kWave, parts - 1)];
    return p;
}
__device__ __forceinline__ void particle_norm_reduce(const NormPartials &p, int parts, float *slot)
{
    if (threadIdx.x < kWave) {
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += (int)threadIdx.x + j * kWave < parts ? (double)p.v[j] : 0.0;
        wave_sum_f64(acc);
        if (threadIdx.x == 0) *slot = (float)sqrt(acc);
    }
}

// -------------------------------------------------------------------- select (torch.argmin order)
// (value, index) pairs under a total order -- NaN before everything, then the smaller value, then the smaller
// index -- so the result does not depend on the reduction shape.
struct ArgMin {
    float v;
    int64_t i;   // -1: empty
};

__device__ __forceinline__ bool argmin_better(const ArgMin &a, const ArgMin &b)   // a strictly before b
{
    if (a.i < 0) return false;
    if (b.i < 0) return true;
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an != bn) return an;
    if (an) return a.i < b.i;
    return a.v < b.v || (a.v == b.v && a.i < b.i);
}

// -------------------------------------------------------------------- the cost finalisation's arguments
// What the small finalisation launches (k_finalize_select, k_finalize_select_copy, k_finalize_topb) take: where a
// scoring launch left its partial sums, how a particle's sum becomes its cost, and where costs and select go.  Built by
// api.hip: cost_args(); the scoring launches themselves only leave partial sums.
enum { COST_L2 = 0,      // value = sqrt(sum of squares)                      ||y - A x||_2
       COST_L1SQ = 1 };  // value = (sum of |.|)^2 * l1_scale                 ||y - A x||_1^2 / (C H W)
enum { POT_NONE = 0, POT_MEAN = 1, POT_MIN = 2, POT_DIFF = 3, POT_CURR = 4 };   // SearchDDPM.resample_update :565-585

struct CostArgs {
    const float *partials = nullptr;
    int parts = 0;
    int mode = COST_L2;
    float l1_scale = 0.0f;
    const float *prev = nullptr;    // [n] previous costs (nullable) and how to combine them with the new value
    int potential = POT_NONE;
    float *raw_out = nullptr;       // [n] the uncombined value (nullable)
    float *out = nullptr;           // [n]
    int64_t *best_idx = nullptr;    // argmin over out[0..n) (nullable)
    float *best_val = nullptr;      // out[argmin] (nullable)
    int n = 0;
};

// -------------------------------------------------------------------- the in-launch norm ("last block done")
// dpsx_step_fwd_f32(norm != NULL) finishes the per-particle norm inside its forward launch -- the only user of this
// route: every block that wrote a partial sum of a particle arrives at that particle's counter; the last one re-sums ALL
// of the particle's partials with slots_sum (so the value is bit-identical to k_finalize_norm's and independent of which
// block came last) and writes the norm.  Nothing waits on anything: a block that is not last just leaves.  Counters are
// zero between launches (the last arriver resets its counter; the host wrapper clears them if a launch fails).  One launch
// at a time per counter array (= per dpsx_op): an operator handle serves ONE stream at a time, as its workspace does.
// NormTail travels by value in the argument block of the forward kernels (resize.hip converts it into the older record its
// fused forward kernels were left with: see LegacyTail there); the scoring instantiations of the blur and resize kernels
// (POST == false) do not contain the route at all.  (The field order is chosen by compiling both: with the
// pointers first an RNG instantiation of k_blur_sep_fwd took more scratch memory -- profiles/tail_split_kernel_stats.txt.)
struct NormTail {
    unsigned *counters = nullptr;   // [kTailMaxParticles]: blocks of particle p arrived; null: no in-launch norm
    int blocks_per_particle = 0;
    const float *partials = nullptr;
    int parts = 0;
    float *out = nullptr;           // [n] the norms
};

constexpr int kTailMaxParticles = 1 << 16;    // counters allocated per operator handle: one per particle
constexpr size_t kNormCounterBytes = (size_t)kTailMaxParticles * sizeof(unsigned);
__device__ __forceinline__ unsigned *norm_counter(const NormTail &t, int particle) { return t.counters + particle; }

// Visibility across the 8 XCDs (one L2 each) WITHOUT a device-scope release fence: on gfx950 that fence is a write-back
// of the whole L2 (`buffer_wbl2`), and with megabytes of freshly written x0_hat / sample lines dirty in it, one fence per
// block cost 535 us per launch (measured, N = 64).  The hand-off is instead the write-through form MI355X_MICROARCH.md
// lists as valid and measured ("Valid forms", first table row): every handed-off word -- the partial sums, the finished
// values -- is stored `sc1` (agent-scope atomic store: write-through past the XCD's L2) by ONE lane, which drains its
// stores with an `asm volatile("s_waitcnt vmcnt(0)" ::: "memory")` -- the asm form, because the compiler may drop or move a
// builtin wait, and its "memory" clobber keeps the store and the counter add in program order -- before ONE agent-scope
// atomic add signals for the block; the block whose add returned last (N blocks per launch) takes an agent-scope acquire
// (an L2 invalidate, no write-back) and reads every word back with `sc1` loads (agent-scope atomic loads).
// Not the C++ memory model's release / acquire pair (there is no release on the writer side by design: it IS the 535 us
// write-back); it relies on the documented gfx950 behaviour of sc1 stores, which is why this library targets gfx950 only.
// The default loops do not take this path (the norm is finalised in the backward launch's prologue, the costs by
// k_finalize_select); it serves `dpsx_step_fwd_f32(norm != NULL)`.
__device__ __forceinline__ float tail_ld(const float *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// a partial sum: read by a later launch (plain store: launch boundaries order it) or, with an in-launch tail, by the last
// block of its particle (write-through store)
__device__ __forceinline__ void tail_publish(float *p, float v, bool in_launch_reader)
{
    if (in_launch_reader) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}
__device__ __forceinline__ void tail_drain_stores()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Called by ALL threads of every block that wrote a partial of `particle`, after the write (block-uniform call site).
__device__ __forceinline__ void tail_arrive(const NormTail &t, int particle)
{
    if (!t.counters) return;                                    // launch-uniform
    __shared__ __attribute__((aligned(16))) int s_last[4];      // one flag, padded: dynamic LDS behind it stays 16-byte aligned
    if (threadIdx.x == 0) {                                     // the thread that published the partial
        tail_drain_stores();                                    // ... whose write-through store has completed
        const unsigned prev = __hip_atomic_fetch_add(norm_counter(t, particle), 1u, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
        const int last = prev == (unsigned)t.blocks_per_particle - 1u;
        if (last) __hip_atomic_store(norm_counter(t, particle), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last[0] = last;
    }
    __syncthreads();
    if (!s_last[0]) return;                                     // block-uniform
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");          // invalidate, no write-back; N blocks per launch
    if (threadIdx.x < kWave) {
        const double acc = slots_sum(t.partials + (int64_t)particle * t.parts, t.parts, tail_ld);
        if (threadIdx.x == 0)
            __hip_atomic_store(t.out + particle, (float)sqrt(acc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// -------------------------------------------------------------------- measurement / mask rows
// A table of `rows` entries (measurements y, inpainting masks) with rows | n: particle p reads entry p / (n / rows), so one
// entry is broadcast, n entries are one per particle, and M entries serve M images of n / M particles each (image-major).
// The launch carries the divisor `div` = n / rows, or 0 for one broadcast entry: the two old cases (0, 1) take no division;
// the others one 32-bit division per tile / block, never per element.
inline unsigned row_div(int64_t rows, int64_t n) { return rows == 1 ? 0u : (unsigned)(n / rows); }

__device__ __forceinline__ unsigned meas_row(unsigned p, unsigned div)
{
    return div == 0 ? 0u : (div == 1 ? p : p / div);
}

// ReflectionPad2d index map (no edge repeat); valid while |overhang| < n.
__device__ __forceinline__ int reflect_idx(int i, int n)
{
    i = i < 0 ? -i : i;
    return i >= n ? 2 * (n - 1) - i : i;
}

}  // namespace dpsx

// -------------------------------------------------------------------- op object
// dpsx_op is the kind, the arrival counters and one typed owner per kind.  Each kind's state is built, owned and read by
// its own translation unit -- blur.hip (blur_create: the tap tables), resize.hip (resize_create: the gather tables and
// blockings), phase.hip (phase_create: plans and twiddles) -- and api.hip reads only the shapes declared here.
enum { OP_TAPS = 0, OP_SEP = 1, OP_RESIZE = 2, OP_MASK = 3, OP_IDENT = 4, OP_PHASE = 5 };

constexpr int kMaxRadius = 32;  // kernel side <= 65

// L (4 or 2) vertically consecutive taps of one kernel column (zero padded): out[r][c] += sum_j w[j] * in[r + dy0 + j][c + dx].
// A lane that owns 8 rows x 2 adjacent columns reads the (8 + L - 1) x 2 inputs of a run once, as 8-byte LDS reads,
// and issues 8 L packed FMAs on them (blur.hip: tap_runs_pk).  dy0 is shifted so that dy0 .. dy0 + L - 1 stays inside
// the staged halo.  Runs are stored grouped by class: [even dx, L=4 | even dx, L=2 | odd dx, L=4 | odd dx, L=2].
struct TapRun {
    int dy0, dx, pad0, pad1;
    float w[4];
};

struct SepTaps {  // passed by value -> SGPRs
    float h[2 * kMaxRadius + 1];
    float v[2 * kMaxRadius + 1];
};

namespace dpsx {

// What blur.hip: blur_tables() derives from (kernel, ks, mode) on the host, no HIP call.  The run tables are what the
// tap-list kernels iterate over: every blur has them (a separable one takes them for shapes the 16-byte loader cannot take)
struct BlurTables {
    bool separable = false;               // rank 1 (and not DPSX_BLUR_FORCE_TAPS): OP_SEP, else OP_TAPS
    int radius = 0;                       // ks / 2 = the reflection pad
    int reach = 0, radius4 = 0;           // reach: largest |offset| of a non-zero tap; radius4: reach rounded up to 4 (>= 4)
    SepTaps sep{};                        // centred at index radius4 (zero padded); separable only
    std::vector<TapRun> fwd, adj;         // the runs by class (see TapRun), the same count in both
    int nrun[4] = {0, 0, 0, 0};           // runs per class (even/odd dx) x (4/2 taps), in table order: always even
    // the ADJOINT table is sorted by dx, descending, inside each class: its first nrun_adj_pos[c] runs have dx >= 1 (the only
    // ones a left-border strip can use), its last nrun_adj_neg[c] have dx <= -1 (right border)
    int nrun_adj_pos[4] = {0, 0, 0, 0}, nrun_adj_neg[4] = {0, 0, 0, 0};
    // halo the tap list actually needs on each side of a tile (rows as they are, columns rounded up to 4): a motion
    // path usually leaves the centre in one direction, so this is about half of radius4 per axis
    int halo_t = 0, halo_b = 0, halo_l = 0, halo_r = 0;
};

struct BlurOp {                            // blur.hip
    BlurTables t;
    const TapRun *d_runs_fwd = nullptr, *d_runs_adj = nullptr;
    DeviceTables tables;
};

struct ResizeOp {                          // resize.hip extends it with its tables and blockings (ResizeHost)
    int64_t in_h = 0, in_w = 0, out_h = 0, out_w = 0, taps_h = 0, taps_w = 0;
};

struct PhaseOp {                           // phase.hip extends it with its plans and twiddles (PhaseHost)
    int64_t h = 0, pad = 0, planes = 0;    // image side, zero pad per side, the batch the first plan is built for
};

struct MaskOp {                            // [rows, h, w] on the device, not owned: particle p of n uses row p / (n / rows)
    const float *mask = nullptr;
    int64_t rows = 1, h = 0, w = 0;
};

}  // namespace dpsx

struct dpsx_op {
    int kind = OP_IDENT;
    dpsx::BlurOp *blur = nullptr;          // OP_SEP, OP_TAPS
    dpsx::ResizeOp *resize = nullptr;      // OP_RESIZE
    dpsx::PhaseOp *phase = nullptr;        // OP_PHASE
    dpsx::MaskOp mask{};                   // OP_MASK (every other kind: one row, so row_div(mask.rows, n) == 0)
    // "last block done" arrival counters (see NormTail): kNormCounterBytes, zero between launches
    unsigned *d_counters = nullptr;
};

// kernels implemented across the .hip files (all enqueue on `s`, return a DPSX_* code)
namespace dpsx {

struct StepFwdArgs {
    const float *x_t, *model_out, *noise, *y;
    int64_t y_n;
    float *x0_hat, *sample;
    uint8_t *inside;
    float *resid;
    float *partials;  // [n * parts_per_particle] sums of squares, finalized into norm by the caller
    int64_t n, c, h, w;
    Coefs k;
    NormTail tail{};  // the norm finished inside the launch (tail.counters == nullptr: not requested / not supported)
    unsigned y_div = 0, mask_div = 0;   // row_div(y_n, n), row_div(op->mask.rows, n)
    bool use_rng = false;               // draw the noise in the kernel from `rng` (noise is then null)
    RngK rng{};
};

struct StepBwdArgs {
    const float *resid, *norm;   // norm == nullptr: derive it from `partials` (parts per particle) and write norm_out
    const float *partials;
    int parts;
    float *norm_out;
    const uint8_t *inside;
    const float *x0_hat, *y;
    int64_t y_n;
    float scale;
    int power;
    float *g_model_out;
    int64_t n, c, h, w;
    Coefs k;
    const float *g_extra = nullptr;   // optional extra cotangent on x0_hat [n, c, h, w], added before the clamp gate
    unsigned y_div = 0, mask_div = 0;   // row_div(y_n, n), row_div(op->mask.rows, n)
};

// blur.hip
BlurTables blur_tables(const float *kernel_host, int ks, int mode);        // pure host: 1 <= ks <= 2 kMaxRadius + 1, odd
int blur_create(dpsx_op *op, const float *kernel_host, int ks, int mode);  // sets op->kind and op->blur
void blur_destroy(dpsx_op *op);
int blur_forward(const dpsx_op *op, const float *x, float *y, int64_t planes, int64_t h, int64_t w, hipStream_t s);
int blur_adjoint(const dpsx_op *op, const float *u, float *g, int64_t planes, int64_t h, int64_t w, float *scratch,
                 int64_t scratch_bytes, hipStream_t s);
int64_t blur_adjoint_scratch_bytes(const dpsx_op *op, int64_t planes, int64_t h, int64_t w);
int blur_step_fwd(const dpsx_op *op, const StepFwdArgs &a, hipStream_t s);
bool blur_step_draws_in_kernel(const dpsx_op *op, int64_t h, int64_t w);   // blur_step_fwd takes StepFwdArgs::use_rng
int blur_step_bwd(const dpsx_op *op, const StepBwdArgs &a, float *scratch, int64_t scratch_bytes, hipStream_t s);
// l1: partials are sums of |r| instead of r^2
int blur_score(const dpsx_op *op, const float *x, const float *y, int64_t y_n, float *partials,
               int64_t n, int64_t c, int64_t h, int64_t w, int l1, hipStream_t s);
int64_t blur_parts_per_particle(const dpsx_op *op, int64_t c, int64_t h, int64_t w);


// resize.hip
// shape: the sizes and tap counts (checked by the caller); the tables are host arrays [taps, out]
int resize_create(dpsx_op *op, const ResizeOp &shape, const float *w_h, const int64_t *i_h, const float *w_w,
                  const int64_t *i_w);
void resize_destroy(dpsx_op *op);
int64_t resize_parts_per_particle(const dpsx_op *op, int64_t c);
int resize_forward(const dpsx_op *op, const float *x, float *y, int64_t planes, hipStream_t s);
int resize_adjoint(const dpsx_op *op, const float *u, float *g, int64_t planes, hipStream_t s);
int resize_step_fwd(const dpsx_op *op, const StepFwdArgs &a, hipStream_t s);
bool resize_step_draws_in_kernel(const dpsx_op *op);                        // resize_step_fwd takes StepFwdArgs::use_rng
int resize_step_bwd(const dpsx_op *op, const StepBwdArgs &a, hipStream_t s);
int resize_score(const dpsx_op *op, const float *x, const float *y, int64_t y_n, float *partials,
                 int64_t n, int64_t c, int l1, hipStream_t s);

// elementwise.hip
// one_state: x [states, chw] and mo [states, 2 chw] feed all n particles, n / states consecutive particles per state
// (z, x0, sample, inside stay per particle)
// the noise: read from z, or with use_rng drawn in the kernel from r (common.h: rng_unit; z is then not read) -- the
// trio StepFwdArgs carries
int posterior_fwd(const float *x, const float *mo, const float *z, bool use_rng, const RngK &r, float *x0, float *sample,
                  uint8_t *inside, int64_t n, int64_t chw, const Coefs &k, hipStream_t s, bool one_state = false,
                  int64_t states = 1);
// out [n, chw] normals of the counters (unit, particle id of row p, r.step, r.tag); bits (nullable) [n, 4 ceil(chw / 4)]
int randn_f32(float *out, uint32_t *bits, int64_t n, int64_t chw, const RngK &r, hipStream_t s);
int posterior_bwd(const float *g_x0, const float *g_s, const float *x, const float *mo, const float *z,
                  float *g_x, float *g_mo, int64_t n, int64_t chw, const Coefs &k, hipStream_t s);
// mask [mask_n, hw]: plane q (of n * c) uses mask meas_row(q / c, mask_div), mask_div = row_div(mask_n, n)
int mask_mul(const float *x, const float *mask, float *y, int64_t planes, int64_t hw, hipStream_t s, int64_t c = 1,
             unsigned mask_div = 0);
// sums of squares of (y - ax) per particle in `parts` chunks -> partials[n*parts]; r optional.  tail: the identity
// operator's fused forward step finishes the norm inside the launch (see NormTail); scoring passes none
int residual_partials(const float *y, int64_t y_n, const float *ax, float *r, float *partials,
                      int64_t n, int64_t m, int parts, hipStream_t s, int l1 = 0, const float *mask = nullptr,
                      int64_t hw = 0, int64_t mask_n = 1, const NormTail &tail = NormTail{});
int finalize_norm(const float *partials, int parts, float *norm, int64_t n, hipStream_t s);
// one small launch: per-particle values from the partials (t.partials / parts / mode / prev / potential -> raw_out, out)
// and, if t.best_idx, the torch.argmin-order select over them.  The select runs per segment:
// `segments` consecutive groups of t.n / segments particles (1: the whole set); t.best_idx / t.best_val are [segments]
// and receive each segment's winner as a global particle index.  _copy: dst[m] = src[best[m]] (chw % 4 == 0, aligned)
int finalize_select(const CostArgs &t, int segments, hipStream_t s);
int finalize_select_copy(const CostArgs &t, int segments, const float *src, float *dst, int64_t chw, hipStream_t s);
// costs + the first b particles of every segment (of t.n / segments <= kTopbMaxK particles) under the select's order:
// t.best_idx / t.best_val (nullable) are [segments, b]
constexpr int kTopbMaxK = 4096;          // a segment's keys and costs live in 12 k bytes of LDS (48 KB at the cap)
int finalize_topb(const CostArgs &t, int segments, int b, hipStream_t s);
// segmented argmin over v [segments, k] -> idx[m] = m * k + argmin (torch.argmin order), val[m] (nullable)
int argmin_seg_f32(const float *v, int64_t segments, int64_t k, int64_t *idx, float *val, hipStream_t s);
int topk_seg_f32(const float *v, int64_t segments, int64_t k, int64_t b, int64_t *idx, float *val, hipStream_t s);
// dst[p] = src[ids[p / per]] for p < n_out (per = particles per id); an id outside [0, n_src) fills dst[p] with NaN
int replicate_seg_f32(const float *src, const int64_t *ids, float *dst, int64_t n_out, int64_t per, int64_t n_src,
                      int64_t chw, hipStream_t s);
int norm_bwd(const float *r, const float *norm, const float *g_norm, int power, float *g_ax,
             int64_t n, int64_t m, hipStream_t s);
// g_model_out[:, :c] = -b * (inside ? coef_p * g_x0 : 0),  g_x0 = A^T r
int clamp_scale_to_eps(const float *g_x0, const float *norm, const uint8_t *inside, float scale, int power,
                       float *g_model_out, int64_t n, int64_t chw, const Coefs &k, hipStream_t s,
                       const float *g_extra = nullptr);
int step_update(const float *sample, const float *g_mo, const float *g_unet, float *x_next,
                int64_t n, int64_t chw, const Coefs &k, hipStream_t s);
int plain_update(const float *sample, const float *ga, const float *gb, float *out, int64_t count, hipStream_t s);
int mask_step_fwd(const dpsx_op *op, const StepFwdArgs &a, int parts, hipStream_t s);
int mask_step_bwd(const dpsx_op *op, const StepBwdArgs &a, hipStream_t s);
int gather_f32(const float *src, const int64_t *ids, float *dst, int64_t n_out, int64_t n_src, int64_t chw, hipStream_t s);
int pack_champion(const float *particles, const float *costs, const int64_t *best, const float *val, float *out, int64_t n,
                  int64_t chw, hipStream_t s);
int select_champion(const float *table, int world, int64_t chw, float *dst, int64_t n_out, int64_t *win_rank,
                    int64_t *win_local, hipStream_t s);

// resample.hip: the per-segment resampling draw (include/dpsx.h): d, u [segments * k]; ids [segments * k] global
// particle indices, q_out (nullable) the integer weights.  resample_seg: the draw + dst[p] = src[ids[p]] +
// d_out[p] = d[ids[p]] in one launch (chw >= 1, src and dst do not alias; the caller checked k <= 4096 and the grid
// limits).  opts == nullptr: the plain entry points' form (a flat segment keeps its particles, the others draw
// multinomially); else the same launch with a scheme (DPSX_RESAMPLE_*), the ESS trigger ess_q16 in [0, 65536] and
// the per-segment diagnostics flag_out / ess_out [segments] (nullable); the caller checked scheme and ess_q16
constexpr int kResampleMaxK = 4096;           // 8 B of LDS per particle of a segment: 32 KB
struct ResampleOpts {
    int scheme;
    int ess_q16;
    uint8_t *flag_out;
    float *ess_out;
};
int resample_draw_seg(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, int64_t *ids,
                      int32_t *q_out, const ResampleOpts *opts, hipStream_t s);
int resample_seg(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, const float *src,
                 float *dst, float *d_out, int64_t *ids, int32_t *q_out, int64_t chw, const ResampleOpts *opts,
                 hipStream_t s);

// cg.hip: the vector launches of dpsx_cg_step_f32 (the recurrence is stated in include/dpsx.h).  Particles of e image
// elements and m measurement elements; every sum of squares is left as cg_slots(size) fp32 partials per particle
// ([n, cg_slots] arrays) and finished in double by the prologue of the launch that consumes it.
constexpr int kCgMaxIters = 64;
int cg_slots(int64_t size);                     // partial slots per particle: a function of the size only (<= 256)
int cg_init(const float *r, float *p, float *rs_part, int64_t n, int64_t e, hipStream_t s);          // p = r, ||r||^2
int cg_sumsq(const float *t, float *part, int64_t n, int64_t m, hipStream_t s);                      // ||t||^2
// alpha = rs / (tt + rho pp); d += alpha p (first: d = alpha p); r -= alpha (sv + rho p); ||r||^2 -> rs_new
int cg_update(float *d, const float *p, float *r, const float *sv, const float *rs_old, const float *tt, const float *pp,
              float *rs_new, float *scal, float rho, bool first, int64_t n, int64_t e, int64_t m, hipStream_t s);
// beta = rs_new / rs_old; p = r + beta p; ||p||^2 -> pp
int cg_pupdate(const float *r, float *p, const float *rs_old, const float *rs_new, float *pp, float *scal, int64_t n,
               int64_t e, hipStream_t s);
// alpha as above; x_next = sample + kappa (d + alpha p); d_out (nullable) = d + alpha p.  x_next may be sample, d_out may be d
int cg_final(const float *sample, const float *d, const float *p, float *x_next, float *d_out, const float *rs,
             const float *tt, const float *pp, float *scal, float rho, float kappa, bool first, int64_t n, int64_t e,
             int64_t m, hipStream_t s);
// dpsx_cg_pullback_f32's finisher, in cg_final's place: alpha as above; g_mo[:, :e] = inside ? gain (d + alpha p) : +0 (the
// eps half of [n, 2 e]; the other half is not touched); d_out (nullable) = d + alpha p, cg_final's bits.  d_out may be d
int cg_pullback(const float *d, const float *p, const uint8_t *inside, float *g_mo, float *d_out, const float *rs,
                const float *tt, const float *pp, float *scal, float rho, float gain, bool first, int64_t n, int64_t e,
                int64_t m, hipStream_t s);

// smc.hip: the particle weights' two launches (the recurrence is stated in include/dpsx.h)
// K3 + the proposal correction's partials [n, cg_slots(chw)]; the noise is z, or with use_rng the counters of r
int step_update_corr(const float *sample, const float *g_mo, const float *g_unet, const float *mo, const float *z,
                     bool use_rng, const RngK &r, float *x_next, float *partials, int64_t n, int64_t chw, const Coefs &k,
                     hipStream_t s);
// E += twist_scale (d_cur^power - d_prev^power) - proposal_weight sum(partials); d_prev = d_cur; reset [segments] (nullable)
int smc_accum(float *e, float *d_prev, const float *d_cur, const float *partials, int slots, const uint8_t *reset,
              int64_t segments, int64_t n, float twist_scale, int power, float proposal_weight, hipStream_t s);

// dsg.hip: spherical-Gaussian guidance in K3's place, two launches (the expression is stated in dsg.hip's header)
// stats [n, cg_slots(chw), 4]: the per-block partials of (S, Nn, C, R); the noise is z, or with use_rng the counters of r
int step_update_dsg(const float *sample, const float *g_mo, const float *g_unet, const float *mo, const float *z,
                    bool use_rng, const RngK &r, float rate, float *x_next, float *stats, int64_t n, int64_t chw,
                    const Coefs &k, hipStream_t s);

// dpmpp.hip: K3 plus the multistep term c (x0_cur - x0_prev), one launch (the expression is stated in dpmpp.hip's header);
// c == 0: neither history is read (both may be null) and x_next has step_update's bits
int step_update_ms(const float *sample, const float *g_mo, const float *g_unet, const float *x0_cur, const float *x0_prev,
                   float c, float *x_next, int64_t n, int64_t chw, const Coefs &k, hipStream_t s);

// metrics.hip: per-particle mse / psnr / ssim against the particle's label row (the definition is stated in include/dpsx.h);
// the caller checked the arguments and the workspace size
bool metrics_shape_ok(int64_t c, int64_t h, int64_t w);      // the index arithmetic fits
int64_t metrics_workspace_bytes(int64_t n, int64_t m, int64_t c, int64_t h, int64_t w);
int image_metrics(const float *x, const float *label, int64_t m, float data_range, float *mse, float *psnr, float *ssim,
                  int64_t n, int64_t c, int64_t h, int64_t w, void *workspace, hipStream_t s);

// repulse.hip: the K x K squared distances of every image's particles and, with apply, the repulsion step (the definition
// is stated in include/dpsx.h); the caller checked the arguments (segments | n, n / segments <= kRepulseMaxK) and the
// workspace size.  d2, w, info, applied: nullable (the workspace holds what the launches need of them)
constexpr int kRepulseMaxK = 512;
int64_t repulse_workspace_bytes(int64_t n, int64_t chw, int64_t segments);
int repulse(bool apply, float c, float bandwidth, const float *x, float *out, float *d2, float *w, float *info,
            uint8_t *applied, int64_t n, int64_t chw, int64_t segments, void *workspace, hipStream_t s);

// ensemble.hip: mean, variance, mean-of-n curve and info of every image's particles (the definition is stated in
// include/dpsx.h); the caller checked the arguments (images | n, 1 <= n / images <= kEnsMaxK) and the workspace size.
// y, e, curve: nullable; count0 > 0: mean / var hold the prior; mean_lo, var_lo: both or neither, the low parts (in/out)
constexpr int kEnsMaxK = 4096;
int64_t ensemble_workspace_bytes(int64_t n, int64_t d, int64_t images);
int ensemble(const float *x, const float *y, const float *e, int64_t count0, float *mean, float *var, float *mean_lo,
             float *var_lo, float *curve, float *info, int64_t n, int64_t d, int64_t images, void *workspace, hipStream_t s);

// quantile.hip: per-element quantiles, the label's rank histogram and the CRPS of every image's particles (the definition
// is stated in include/dpsx.h); the caller checked the arguments (images | n, 1 <= n / images <= kQuantMaxK, 1 <= q <=
// kQuantMaxQ, probs in [0, 1]) and the workspace size.  y, hist: nullable.  K <= kQuantRegK sorts in registers, above in LDS
constexpr int kQuantMaxK = 512;
constexpr int kQuantMaxQ = 8;
constexpr int kQuantRegK = 64;
int64_t quantiles_workspace_bytes(int64_t n, int64_t d, int64_t images);
int quantiles(const float *x, const float *y, const double *probs, int64_t q, float *quant, int32_t *hist, float *info,
              int64_t n, int64_t d, int64_t images, void *workspace, hipStream_t s);

// pca.hip: the top q principal components of every image's particles (the definition is stated in include/dpsx.h); the
// caller checked the arguments (images | n, 1 <= n / images <= kPcaMaxK, 1 <= q <= kPcaMaxQ) and the workspace size.
// d2: nullable (the workspace holds it).  G and V of the eigensolver live in LDS: two kPcaMaxK x (kPcaMaxK + 1) fp32 matrices
constexpr int kPcaMaxK = 128;
constexpr int kPcaMaxQ = 8;
int64_t pca_workspace_bytes(int64_t n, int64_t d, int64_t images);
int pca(const float *x, int64_t q, float *dirs, float *evals, float *coords, float *info, float *d2, int64_t n, int64_t d,
        int64_t images, void *workspace, hipStream_t s);

// phase.hip
int phase_create(dpsx_op *op, const PhaseOp &shape);
void phase_destroy(dpsx_op *op);
int64_t phase_workspace_bytes(const dpsx_op *op, int64_t planes);
// amp = |F(pad(x))| ; spec (optional) receives the centred complex spectrum, interleaved re/im
int phase_forward(dpsx_op *op, const float *x, float *amp, float *spec, int64_t planes,
                  void *ws, int64_t ws_bytes, hipStream_t s);
// g = Re crop F^H (u * z/|z|), z = spectrum at x (recomputed)
int phase_adjoint(dpsx_op *op, const float *u, const float *x, float *g, int64_t planes,
                  void *ws, int64_t ws_bytes, hipStream_t s);
// fused step halves: fwd leaves w = (y-|z|) z/|z| (complex) in resid_c and the sums of squares in partials;
// bwd turns resid_c into g_x0 = Re crop F^H w (unit cotangent) -- caller applies coef / clamp / -b
int phase_step_fwd(dpsx_op *op, const StepFwdArgs &f, float *resid_c, hipStream_t s);   // S1 included
bool phase_vec4_ok(const dpsx_op *op);
bool phase_is_spectral(const dpsx_op *op);
bool phase_norm_in_bwd(const dpsx_op *op);   // the backward launch finalises the norm from the partial sums itself
int phase_step_bwd_fused(dpsx_op *op, float *resid_c, const StepBwdArgs &b, hipStream_t s);
int phase_step_bwd(dpsx_op *op, float *resid_c, float *g_x0, int64_t planes, hipStream_t s);
int64_t phase_parts_per_particle(const dpsx_op *op, int64_t c);
int64_t phase_step_resid_bytes(const dpsx_op *op, int64_t planes);

}  // namespace dpsx
