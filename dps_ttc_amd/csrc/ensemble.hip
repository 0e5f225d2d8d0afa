// Ensemble statistics of every image's K particles (include/dpsx.h: "ensemble statistics"): the posterior mean, the
// per-pixel variance, the mean-of-n curve against the label and the info record, at most three launches:
//
//   k_ens_weights  only with E: one block per image; the K normalised weights, ESS and the "no finite E" flag
//   k_ens_stream   grid (cg_slots(D), M) in particle_pass.h's layout (units, range, slots: functions of D only).  A lane
//                  owns units of 16 bytes (float4; the scalar instantiation where D % 4 != 0 or a buffer is unaligned) of
//                  its block's range and walks the image's particles j = 0 .. K - 1 in index order, two batches of kEnsBatch
//                  last-use loads, the next issued before the current is used (a row is a coalesced 1 KiB per wave).  S1, S2 and the
//                  uniform prefix sum are double accumulators per component; mean and variance are written from the
//                  lane's own registers, so their bits depend on neither the unit form nor the block shape.  Per n the
//                  lane adds the squared errors of its components serially in fp32; the wave adds them in wave_sum's tree
//                  and its lane 0 adds the result into the wave's row of an LDS table (unit passes in order); at the end
//                  the block adds the four rows in wave order: one fp32 partial per (block, n) in part[M][slots][K + 1].
//                  Column K (the final mean's error) and the variance sum go through block_sum.
//   k_ens_finish   one wave per (image, kEnsCols columns): a column's slots are added in double in slots_sum's order,
//                  divided by D and rounded once; the wave that owns column K also writes info.
//
// The low parts (optional, dpsx_ensemble_ex_f32): mean_lo = mean - fp32(mean) and var_lo = var - fp32(var), fp32 each.  A
// prior is fp32 and its rounding alone can exceed what a merged number may be off by (where two groups' means cancel, or
// the variance is tiny against the mean); a caller that hands a call's low parts to the next call as part of the prior gets
// groups merged call after call to the accuracy of one call over all of them.  Arguments like the others: no state.
// The weights, the reciprocals 1 / (count0 + n) (double) and the four curve rows live in dynamic LDS: 28 K + 16 bytes.
// No atomics, no fence, no host read; a block reads its image only, so a non-finite value stays in its image and, lanes
// being independent, in its element.
#include "particle_pass.h"

#include <cmath>

namespace dpsx {

constexpr int kEnsBatch = 8;      // particle rows in flight per lane
constexpr int kEnsCols = 16;      // curve columns per finisher wave
constexpr int kEnsWaves = kPassThreads / kWave;

struct EnsArgs {
    const float *x, *y;           // y null: no curve
    const float *w;               // [n] normalised weights (k_ens_weights) or null
    const int *uniform;           // [M] with w: 1 = the image has no finite E and takes the uniform form
    const float *ess;             // [M] with w
    float *mean, *var;            // [M, D]; read as the prior when count0 > 0
    float *part, *varpart;        // [M, slots, K + 1], [M, slots]
    float *curve, *info;          // [M, K + 1] (nullable), [M, 4]
    float *mean_lo, *var_lo;      // [M, D] both or neither: what the fp32 roundings of mean / var drop; read with a prior
    int64_t d, per;
    int k, slots;
    double count0;
};

// ------------------------------------------------------------------ the weights
__global__ __launch_bounds__(kPassThreads) void k_ens_weights(const float *__restrict__ e_all, float *__restrict__ w_all,
                                                              int *__restrict__ uniform, float *__restrict__ ess, int k)
{
    __shared__ double s_w[kEnsMaxK];
    __shared__ float s_min[kEnsWaves];
    __shared__ double s_tot[2];
    const int64_t m = blockIdx.x;
    const float *e = e_all + m * k;
    float *w = w_all + m * k;

    float mn = INFINITY;                                     // over the finite entries: exact, any order
    for (int j = threadIdx.x; j < k; j += kPassThreads) {
        const float v = e[j];
        if (__builtin_isfinite(v)) mn = fminf(mn, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_down(mn, o, kWave));
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = mn;
    __syncthreads();
    mn = s_min[0];
    for (int i = 1; i < kEnsWaves; ++i) mn = fminf(mn, s_min[i]);
    const bool none = !(mn < INFINITY);                      // block-uniform: no finite E

    for (int j = threadIdx.x; j < k; j += kPassThreads) {
        const float v = e[j];
        s_w[j] = !none && __builtin_isfinite(v) ? exp(-(double)__fsub_rn(v, mn)) : 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                  // W and sum w^2 in index order
        double t1 = 0.0, t2 = 0.0;
        for (int j = 0; j < k; ++j) {
            const double v = s_w[j];
            t1 += v;
            t2 += v * v;
        }
        s_tot[0] = t1;
        s_tot[1] = t2;
    }
    __syncthreads();
    const double tot = s_tot[0];
    for (int j = threadIdx.x; j < k; j += kPassThreads) w[j] = none ? 1.0f : (float)(s_w[j] / tot);
    if (threadIdx.x == 0) {
        uniform[m] = none;
        ess[m] = none ? (float)k : (float)(tot * tot / s_tot[1]);
    }
}

// ------------------------------------------------------------------ the stream
__device__ __forceinline__ double ens_clamp0(double v) { return v < 0.0 ? 0.0 : v; }      // max(v, 0); NaN passes

template <bool VEC, bool WEIGHTED, bool CURVE>
__device__ __forceinline__ void ens_block(const EnsArgs &a, const double *s_rcp, float *s_curve, const float *s_w, float *red)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    const int64_t m = blockIdx.y, units = a.d / W;
    const int k = a.k, cols = k + 1;
    const Range r = block_range(units, a.per);
    const float *xi = a.x + m * k * a.d;
    const bool prior = a.count0 > 0.0;                       // launch-uniform
    const double total = a.count0 + (double)k;
    float *crow = s_curve + (threadIdx.x >> 6) * cols;
    float vsum = 0.0f, fsum = 0.0f;

    for (int64_t base = r.lo; base < r.hi; base += kPassThreads) {
        const int64_t u = base + threadIdx.x;
        const bool on = u < r.hi;                            // a lane past the range computes on zeros and adds zeros
        const int64_t e0 = u * W;
        T cv = T{}, yv = T{}, pv = T{}, lm = T{}, lv = T{};
        if (on) {
            cv = prior ? ld<T>(a.mean + m * a.d + e0) : ld<T>(xi + e0);
            if (prior) pv = ld<T>(a.var + m * a.d + e0);
            if constexpr (CURVE) yv = ld<T>(a.y + m * a.d + e0);
            if (prior && a.mean_lo) {                        // launch-uniform
                lm = ld<T>(a.mean_lo + m * a.d + e0);
                lv = ld<T>(a.var_lo + m * a.d + e0);
            }
        }
        // the prior's particles about c: their sum count0 (mean0 - c) = count0 ml, their squares count0 (var0 + ml^2)
        double c[W], s1[W], s2[W], p[W], ml[W], v0[W];
#pragma unroll
        for (int q = 0; q < W; ++q) {
            c[q] = (double)lane(cv, q);
            ml[q] = (double)lane(lm, q);
            v0[q] = (double)lane(pv, q) + (double)lane(lv, q);
            s1[q] = a.count0 * ml[q];
            s2[q] = p[q] = 0.0;
        }
        // two batches of rows: the next one's loads are issued before the current one is used, so a wave that is alone on
        // its SIMD (slots <= 256 blocks per image) still has loads in flight while it computes
        T v[kEnsBatch], nx[kEnsBatch];
        auto fetch = [&](T(&dst)[kEnsBatch], int j0) {
#pragma unroll
            for (int i = 0; i < kEnsBatch; ++i) {
                const int jj = min(j0 + i, k - 1);
                dst[i] = on ? ld_last<T>(xi + (int64_t)jj * a.d + e0) : T{};
            }
        };
        fetch(nx, 0);
        for (int j0 = 0; j0 < k; j0 += kEnsBatch) {
#pragma unroll
            for (int i = 0; i < kEnsBatch; ++i) v[i] = nx[i];
            if (j0 + kEnsBatch < k) fetch(nx, j0 + kEnsBatch);       // launch-uniform
#pragma unroll
            for (int i = 0; i < kEnsBatch; ++i) {
                const int j = j0 + i;
                if (j < k) {                                 // launch-uniform
                    float acc = 0.0f;
                    [[maybe_unused]] double wj = 1.0, rn = 0.0;
                    if constexpr (WEIGHTED) wj = (double)s_w[j];
                    if constexpr (CURVE) rn = s_rcp[j];
#pragma unroll
                    for (int q = 0; q < W; ++q) {
                        const double dq = (double)lane(v[i], q) - c[q];
                        if constexpr (WEIGHTED) {
                            const double wd = wj * dq;
                            s1[q] += wd;
                            s2[q] = fma(wd, dq, s2[q]);
                            p[q] += dq;
                        } else {
                            s1[q] += dq;
                            s2[q] = fma(dq, dq, s2[q]);
                        }
                        if constexpr (CURVE) {
                            const double er = fma(WEIGHTED ? p[q] : s1[q], rn, c[q]) - (double)lane(yv, q);
                            acc = __fadd_rn(acc, (float)(er * er));
                        }
                    }
                    if constexpr (CURVE) {
                        acc = wave_sum(on ? acc : 0.0f);
                        if ((threadIdx.x & 63) == 0) crow[j] = __fadd_rn(crow[j], acc);
                    }
                }
            }
        }
        T mo = T{}, vo = T{}, mlo = T{}, vlo = T{};
#pragma unroll
        for (int q = 0; q < W; ++q) {
            double mean, var;
            if constexpr (WEIGHTED) {
                mean = c[q] + s1[q];
                var = s2[q] - s1[q] * s1[q];
            } else {
                mean = c[q] + s1[q] / total;
                const double m2 = (prior ? (v0[q] + ml[q] * ml[q]) * a.count0 : 0.0) + s2[q] - s1[q] * s1[q] / total;
                var = m2 / total;
            }
            const double vc = ens_clamp0(var);
            const float mf = (float)mean, vf = (float)vc;
            set(mo, q, mf);
            set(vo, q, vf);
            set(mlo, q, __builtin_isfinite(mf) ? (float)(mean - (double)mf) : 0.0f);
            set(vlo, q, __builtin_isfinite(vf) ? (float)(vc - (double)vf) : 0.0f);
            vsum = __fadd_rn(vsum, on ? vf : 0.0f);
            if constexpr (CURVE) {
                const double er = mean - (double)lane(yv, q);
                fsum = __fadd_rn(fsum, on ? (float)(er * er) : 0.0f);
            }
        }
        if (on) {
            st<T>(a.mean + m * a.d + e0, mo);
            st<T>(a.var + m * a.d + e0, vo);
            if (a.mean_lo) {
                st<T>(a.mean_lo + m * a.d + e0, mlo);
                st<T>(a.var_lo + m * a.d + e0, vlo);
            }
        }
    }

    const int64_t slot = m * a.slots + blockIdx.x;
    if constexpr (CURVE) {
        __syncthreads();
        for (int n = threadIdx.x; n < k; n += kPassThreads) {
            float t = s_curve[n];
#pragma unroll
            for (int wv = 1; wv < kEnsWaves; ++wv) t = __fadd_rn(t, s_curve[wv * cols + n]);
            a.part[slot * cols + n] = t;
        }
        const float fs = block_sum(fsum, red);
        if (threadIdx.x == 0) a.part[slot * cols + k] = fs;
    }
    const float vs = block_sum(vsum, red);
    if (threadIdx.x == 0) a.varpart[slot] = vs;
}

template <bool VEC, bool CURVE>
__global__ __launch_bounds__(kPassThreads) void k_ens_stream(const EnsArgs a)
{
    extern __shared__ double s_dyn[];
    __shared__ float red[kEnsWaves];
    const int k = a.k, cols = k + 1;
    double *s_rcp = s_dyn;                                                     // [k]               (CURVE)
    float *s_curve = reinterpret_cast<float *>(s_dyn + (CURVE ? k : 0));       // [kEnsWaves, cols] (CURVE)
    float *s_w = s_curve + (CURVE ? kEnsWaves * cols : 0);                     // [k]               (with weights)
    const bool weighted = a.w && !a.uniform[blockIdx.y];                       // block-uniform
    if constexpr (CURVE) {
        for (int j = threadIdx.x; j < k; j += kPassThreads) s_rcp[j] = 1.0 / (a.count0 + (double)(j + 1));
        for (int j = threadIdx.x; j < kEnsWaves * cols; j += kPassThreads) s_curve[j] = 0.0f;
    }
    if (weighted)
        for (int j = threadIdx.x; j < k; j += kPassThreads) s_w[j] = a.w[(int64_t)blockIdx.y * k + j];
    __syncthreads();
    if (weighted) ens_block<VEC, true, CURVE>(a, s_rcp, s_curve, s_w, red);
    else ens_block<VEC, false, CURVE>(a, s_rcp, s_curve, s_w, red);
}

// ------------------------------------------------------------------ the finisher
__global__ __launch_bounds__(kWave) void k_ens_finish(const EnsArgs a)
{
    const int64_t m = blockIdx.y;
    const int k = a.k, cols = a.y ? k + 1 : 0;
    const int lo = blockIdx.x * kEnsCols, hi = min(cols, lo + kEnsCols);
    float last = NAN;
    for (int col = lo; col < hi; ++col) {
        double acc = 0.0;                                    // slots_sum's order over a strided column
        for (int i = threadIdx.x; i < a.slots; i += kWave) acc += (double)a.part[(m * a.slots + i) * (k + 1) + col];
        wave_sum_f64(acc);
        last = (float)(acc / (double)a.d);
        if (threadIdx.x == 0 && a.curve) a.curve[m * (k + 1) + col] = last;
    }
    if (blockIdx.x != gridDim.x - 1) return;                 // the wave that owns column K
    const double vs = slots_sum(a.varpart + m * a.slots, a.slots);
    if (threadIdx.x != 0) return;
    const double total = a.count0 + (double)k;
    float *o = a.info + m * 4;
    o[0] = a.w ? a.ess[m] : (float)total;
    o[1] = (float)(vs / (double)a.d);
    o[2] = cols ? last : NAN;
    o[3] = (float)total;
}

// ------------------------------------------------------------------ host side
// THE workspace layout: the stream launch's partials, then what the weights launch leaves (a.w, a.ess, a.uniform: set
// here, kept only with E); returns the bytes (the size query and the launch path both walk it)
static int64_t ens_layout(EnsArgs &a, Carver cv, int64_t n, int64_t d, int64_t images)
{
    const int64_t k = n / images, slots = cg_slots(d);
    a.part = cv.take<float>(images * slots * (k + 1));
    a.varpart = cv.take<float>(images * slots);
    a.w = cv.take<float>(n);
    a.ess = cv.take<float>(images);
    a.uniform = cv.take<int>(images);
    return cv.bytes();
}

int64_t ensemble_workspace_bytes(int64_t n, int64_t d, int64_t images)
{
    EnsArgs a{};
    return ens_layout(a, Carver(nullptr), n, d, images);
}

int ensemble(const float *x, const float *y, const float *e, int64_t count0, float *mean, float *var, float *mean_lo,
             float *var_lo, float *curve, float *info, int64_t n, int64_t d, int64_t images, void *workspace, hipStream_t s)
{
    const int64_t k = n / images;
    const bool vec = vec_ok(d, {x, y, mean, var, mean_lo, var_lo});
    const PassGeom g = pass_geom(d, vec, images);
    EnsArgs a{};
    ens_layout(a, Carver(workspace), n, d, images);
    a.x = x;
    a.y = y;
    a.mean = mean;
    a.var = var;
    a.curve = curve;
    a.mean_lo = mean_lo;
    a.var_lo = var_lo;
    a.info = info;
    a.d = d;
    a.per = g.per;
    a.k = (int)k;
    a.slots = cg_slots(d);
    a.count0 = (double)count0;
    if (e) {                                                 // the one launch that writes what the others only read
        k_ens_weights<<<(unsigned)images, kPassThreads, 0, s>>>(e, const_cast<float *>(a.w), const_cast<int *>(a.uniform),
                                                                const_cast<float *>(a.ess), (int)k);
        const int rc = check_launch();
        if (rc != DPSX_OK) return rc;
    } else {
        a.w = a.ess = nullptr;
        a.uniform = nullptr;
    }
    const size_t lds = (y ? k * sizeof(double) + kEnsWaves * (k + 1) * sizeof(float) : 0) + (e ? k * sizeof(float) : 0);
    int rc = dispatch(vec, y != nullptr, [&](auto V, auto C) { return launch_lds<k_ens_stream<V.value, C.value>>(g.grid, kPassThreads, lds, s, a); });
    if (rc != DPSX_OK) return rc;
    const int64_t cols = y ? k + 1 : 0;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, (cols + kEnsCols - 1) / kEnsCols);
    k_ens_finish<<<dim3(blocks, (unsigned)images), kWave, 0, s>>>(a);
    return check_launch();
}

}  // namespace dpsx
