// Element-wise / reduction kernels of the DPS step (HBM-bound; 16 B per lane).
//
// Layout: particles are the outer dimension; one particle = chw contiguous
// fp32; model_out holds 2*chw per particle (eps | v).  Fast paths need
// chw % 4 == 0 and 16-byte aligned bases (torch allocations are), otherwise a
// scalar kernel with identical arithmetic runs.
#include "common.h"

#include <type_traits>

namespace dpsx {

constexpr int kThreads = 256;

static inline dim3 grid_for(int64_t work_per_particle, int64_t n)
{
    int64_t bx = (work_per_particle + kThreads - 1) / kThreads;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)n, 1);
}

// ===================================================================== S1 forward
// RNG: the noise is drawn in the kernel (common.h: rng_unit) where S1 consumes it; `z` is then the RngK record instead of
// the pointer, so the pointer instantiations keep their signature and their code
template <bool VEC, bool RNG = false>
__global__ __launch_bounds__(kThreads) void k_posterior_fwd(const float *__restrict__ x,
                                                            const float *__restrict__ mo,
                                                            const std::conditional_t<RNG, RngK, const float *__restrict__> z,
                                                            float *__restrict__ x0o, float *__restrict__ so,
                                                            uint8_t *__restrict__ ins, int64_t chw, Coefs k,
                                                            unsigned sdiv)
{
    // sdiv: particles per state of x / model_out -- 1: one state per particle; 0: ONE state feeds all particles
    // (search_ddpm); else n / states: consecutive groups of sdiv particles share a state (search_ddpm over several images)
    const int64_t p = blockIdx.y;
    const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= chw) return;
    const int64_t st = meas_row((unsigned)p, sdiv);
    const float *xp = x + st * chw + i, *ep = mo + st * 2 * chw + i, *vp = ep + chw;
    const int64_t o = p * chw + i;
    if constexpr (VEC) {
        const float4 xv = *reinterpret_cast<const float4 *>(xp);
        const float4 ev = *reinterpret_cast<const float4 *>(ep);
        float4 vv = make_float4(0, 0, 0, 0), zv = vv;
        if (k.add_noise & 1) {
            vv = *reinterpret_cast<const float4 *>(vp);
            if constexpr (!RNG) zv = *reinterpret_cast<const float4 *>(z + o);
        }
        bool b0, b1, b2, b3;
        float4 x0, sm;
        x0.x = post_x0(xv.x, ev.x, k, b0);
        x0.y = post_x0(xv.y, ev.y, k, b1);
        x0.z = post_x0(xv.z, ev.z, k, b2);
        x0.w = post_x0(xv.w, ev.w, k, b3);
        if constexpr (RNG)
            if (k.add_noise & 1) zv = rng_unit(z, (uint32_t)(i >> 2), rng_particle(z, (unsigned)p));
        sm.x = post_sample(xv.x, x0.x, vv.x, zv.x, k);
        sm.y = post_sample(xv.y, x0.y, vv.y, zv.y, k);
        sm.z = post_sample(xv.z, x0.z, vv.z, zv.z, k);
        sm.w = post_sample(xv.w, x0.w, vv.w, zv.w, k);
        if (x0o) *reinterpret_cast<float4 *>(x0o + o) = x0;
        if (so) *reinterpret_cast<float4 *>(so + o) = sm;
        if (ins) *reinterpret_cast<uchar4 *>(ins + o) = make_uchar4(b0, b1, b2, b3);
    } else {
        bool b;
        float x0 = post_x0(*xp, *ep, k, b);
        float zs = 0.f;
        if (k.add_noise & 1) {
            if constexpr (RNG) zs = rng_elem(z, i, rng_particle(z, (unsigned)p));
            else zs = z[o];
        }
        float sm = post_sample(*xp, x0, (k.add_noise & 1) ? *vp : 0.f, zs, k);
        if (x0o) x0o[o] = x0;
        if (so) so[o] = sm;
        if (ins) ins[o] = b;
    }
}

int posterior_fwd(const float *x, const float *mo, const float *z, bool use_rng, const RngK &r, float *x0, float *sample,
                  uint8_t *inside, int64_t n, int64_t chw, const Coefs &k, hipStream_t s, bool one_state, int64_t states)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const unsigned xs = one_state ? row_div(states, n) : 1u;
    const bool vec = chw % 4 == 0 && aligned16(x) && aligned16(mo) && (use_rng || aligned16(z)) && aligned16(x0) &&
                     aligned16(sample) && (reinterpret_cast<uintptr_t>(inside) & 3u) == 0;
    const dim3 grid = grid_for(vec ? chw / 4 : chw, n);
    if (vec && use_rng) k_posterior_fwd<true, true><<<grid, kThreads, 0, s>>>(x, mo, r, x0, sample, inside, chw, k, xs);
    else if (vec) k_posterior_fwd<true><<<grid, kThreads, 0, s>>>(x, mo, z, x0, sample, inside, chw, k, xs);
    else if (use_rng) k_posterior_fwd<false, true><<<grid, kThreads, 0, s>>>(x, mo, r, x0, sample, inside, chw, k, xs);
    else k_posterior_fwd<false><<<grid, kThreads, 0, s>>>(x, mo, z, x0, sample, inside, chw, k, xs);
    return check_launch();
}

// ===================================================================== stand-alone normal fill
// out [n, chw]: one float4 unit per lane (the last unit of a particle with chw % 4 != 0 is cut); bits (nullable)
// [n, 4 * units] receives the four Philox words of every unit
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_randn(float *__restrict__ out, uint32_t *__restrict__ bits, int64_t chw,
                                                    int64_t units, RngK r)
{
    const int64_t p = blockIdx.y;
    const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= units) return;
    uint4 w;
    const float4 z = rng_unit(r, (uint32_t)u, rng_particle(r, (unsigned)p), &w);
    const int64_t i = 4 * u, o = p * chw + i;
    if constexpr (VEC) {
        *reinterpret_cast<float4 *>(out + o) = z;
    } else {
        out[o] = z.x;
        if (i + 1 < chw) out[o + 1] = z.y;
        if (i + 2 < chw) out[o + 2] = z.z;
        if (i + 3 < chw) out[o + 3] = z.w;
    }
    if (bits) {
        uint32_t *b = bits + (p * units + u) * 4;
        b[0] = w.x; b[1] = w.y; b[2] = w.z; b[3] = w.w;
    }
}

int randn_f32(float *out, uint32_t *bits, int64_t n, int64_t chw, const RngK &r, hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const int64_t units = (chw + 3) / 4;
    if (chw % 4 == 0 && aligned16(out)) k_randn<true><<<grid_for(units, n), kThreads, 0, s>>>(out, bits, chw, units, r);
    else k_randn<false><<<grid_for(units, n), kThreads, 0, s>>>(out, bits, chw, units, r);
    return check_launch();
}

// ===================================================================== S1 backward
// g_pre = [pre in [-1,1]] * (g_x0 + c1 g_s);  g_x = a g_pre + c2 g_s;
// g_eps = -b g_pre;  g_v = g_s * z * sd * (max_log - min_log) / 4
template <int U>      // U = 4: one float4 unit per lane (chw % 4 == 0, 16-byte aligned planes); U = 1: scalar
__global__ __launch_bounds__(kThreads) void k_posterior_bwd(const float *__restrict__ g_x0,
                                                            const float *__restrict__ g_s,
                                                            const float *__restrict__ x,
                                                            const float *__restrict__ mo,
                                                            const float *__restrict__ z,
                                                            float *__restrict__ g_x, float *__restrict__ g_mo,
                                                            int64_t chw, Coefs k)
{
    const int64_t p = blockIdx.y;
    const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * U;
    if (i >= chw) return;
    const int64_t o = p * chw + i, e = p * 2 * chw + i;
    float xv[U], ev[U], vv[U], zv[U], g0v[U], gsv[U], ox[U], oe[U], ov[U];
    const bool noisy = k.add_noise == 1 && g_s;
    if constexpr (U == 4) {
        auto ld4 = [](const float *q, float (&d)[U]) {
            const float4 t = *reinterpret_cast<const float4 *>(q);
            d[0] = t.x; d[1] = t.y; d[2] = t.z; d[3] = t.w;
        };
        ld4(x + o, xv);
        ld4(mo + e, ev);
        if (g_x0) ld4(g_x0 + o, g0v);
        if (g_s) ld4(g_s + o, gsv);
        if (noisy) { ld4(mo + e + chw, vv); ld4(z + o, zv); }
    } else {
        xv[0] = x[o]; ev[0] = mo[e];
        if (g_x0) g0v[0] = g_x0[o];
        if (g_s) gsv[0] = g_s[o];
        if (noisy) { vv[0] = mo[e + chw]; zv[0] = z[o]; }
    }
    // d sample / d x0_hat and d sample / d x (direct): DDPM c1, c2;  DDIM c1 - c2 / b, c2 a / b
    const bool ddim = k.add_noise & 2;
    const float ds_dx0 = ddim ? k.c1 - k.c2 / k.b : k.c1, ds_dx = ddim ? k.c2 * k.a / k.b : k.c2;
#pragma unroll
    for (int q = 0; q < U; ++q) {
        bool in;
        (void)post_x0(xv[q], ev[q], k, in);
        const float gs = g_s ? gsv[q] : 0.0f;
        const float g0 = (g_x0 ? g0v[q] : 0.0f) + ds_dx0 * gs;
        const float gp = in ? g0 : 0.0f;
        ox[q] = k.a * gp + ds_dx * gs;
        oe[q] = -k.b * gp;
        ov[q] = 0.0f;
        if (noisy) {
            const float sd = expf(0.5f * post_logvar(vv[q], k));
            ov[q] = gs * zv[q] * sd * (0.25f * (k.max_log - k.min_log));
        }
    }
    if constexpr (U == 4) {
        *reinterpret_cast<float4 *>(g_x + o) = make_float4(ox[0], ox[1], ox[2], ox[3]);
        *reinterpret_cast<float4 *>(g_mo + e) = make_float4(oe[0], oe[1], oe[2], oe[3]);
        *reinterpret_cast<float4 *>(g_mo + e + chw) = make_float4(ov[0], ov[1], ov[2], ov[3]);
    } else {
        g_x[o] = ox[0];
        g_mo[e] = oe[0];
        g_mo[e + chw] = ov[0];
    }
}

int posterior_bwd(const float *g_x0, const float *g_s, const float *x, const float *mo, const float *z,
                  float *g_x, float *g_mo, int64_t n, int64_t chw, const Coefs &k, hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const bool vec = chw % 4 == 0 && aligned16(g_x0) && aligned16(g_s) && aligned16(x) && aligned16(mo) && aligned16(z) &&
                     aligned16(g_x) && aligned16(g_mo);
    if (vec) k_posterior_bwd<4><<<grid_for(chw / 4, n), kThreads, 0, s>>>(g_x0, g_s, x, mo, z, g_x, g_mo, chw, k);
    else k_posterior_bwd<1><<<grid_for(chw, n), kThreads, 0, s>>>(g_x0, g_s, x, mo, z, g_x, g_mo, chw, k);
    return check_launch();
}

// ===================================================================== inpainting mask
// mask_div = row_div(mask_n, n): plane q = (particle, channel) reads mask row meas_row(q / c, mask_div)
__global__ __launch_bounds__(kThreads) void k_mask_mul(const float *__restrict__ x, const float *__restrict__ m,
                                                       float *__restrict__ y, int64_t hw, unsigned c, unsigned mask_div)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= hw) return;
    const int64_t o = (int64_t)blockIdx.y * hw + i;
    const float *mp = mask_div ? m + (int64_t)meas_row(blockIdx.y / c, mask_div) * hw : m;   // launch-uniform
    y[o] = __fmul_rn(x[o], mp[i]);
}

int mask_mul(const float *x, const float *mask, float *y, int64_t planes, int64_t hw, hipStream_t s, int64_t c,
             unsigned mask_div)
{
    if (planes == 0 || hw == 0) return DPSX_OK;
    k_mask_mul<<<grid_for(hw, planes), kThreads, 0, s>>>(x, mask, y, hw, (unsigned)c, mask_div);
    return check_launch();
}

// ===================================================================== residual + norm
// grid (parts, n): block (q, p) reduces elements [q*chunk, (q+1)*chunk) of particle p.
// mask (nullable, hw elements, broadcast over particles and channels): the inpainting operator applied on the fly,
// d = y - mask * ax with the product rounded once, exactly as mask_mul + this kernel did in two launches (the search
// step's scoring of a masked proposal: 44 -> one launch without the 2P round trip through scratch).
// y_div = row_div(y_n, n); mask [mask_n, hw] with mask_div = row_div(mask_n, n) (per-image masks)
__global__ __launch_bounds__(kThreads) void k_residual_partials(const float *__restrict__ y, unsigned y_div,
                                                                const float *__restrict__ ax,
                                                                float *__restrict__ r,
                                                                float *__restrict__ partials, int64_t m,
                                                                int64_t chunk, int l1, NormTail tail,
                                                                const float *__restrict__ mask, int hw, unsigned mask_div)
{
    __shared__ float scratch[kThreads / kWave];
    const int64_t p = blockIdx.y, q = blockIdx.x;
    const float *yp = y + (int64_t)meas_row((unsigned)p, y_div) * m, *ap = ax + p * m;
    const int64_t lo = q * chunk, hi = min(m, lo + chunk);
    float acc = 0.0f;
    if (mask) {
        mask += (int64_t)meas_row((unsigned)p, mask_div) * hw;
        int mi = (int)((lo + threadIdx.x) % hw);                 // walks the mask plane with the element index
        const int step = kThreads % hw;
        for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
            const float d = __fsub_rn(yp[i], __fmul_rn(ap[i], mask[mi]));
            if (r) r[p * m + i] = d;
            acc = l1 ? acc + fabsf(d) : fmaf(d, d, acc);
            mi += step;
            if (mi >= hw) mi -= hw;
        }
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += kThreads) {
            const float d = __fsub_rn(yp[i], ap[i]);
            if (r) r[p * m + i] = d;
            acc = l1 ? acc + fabsf(d) : fmaf(d, d, acc);
        }
    }
    const float t = block_sum(acc, scratch);
    if (threadIdx.x == 0) tail_publish(&partials[p * gridDim.x + q], t, tail.counters != nullptr);
    tail_arrive(tail, (int)p);
}

int residual_partials(const float *y, int64_t y_n, const float *ax, float *r, float *partials, int64_t n,
                      int64_t m, int parts, hipStream_t s, int l1, const float *mask, int64_t hw, int64_t mask_n,
                      const NormTail &tail)
{
    if (n == 0) return DPSX_OK;
    if (mask && (hw < 1 || hw > (1 << 30))) return DPSX_EINVAL;
    const int64_t chunk = (m + parts - 1) / parts;
    NormTail t = tail;
    t.blocks_per_particle = parts;
    k_residual_partials<<<dim3(parts, (unsigned)n), kThreads, 0, s>>>(y, row_div(y_n, n), ax, r, partials, m, chunk, l1, t,
                                                                     mask, (int)hw, row_div(mask_n, n));
    return check_launch();
}

// one wave per particle: common.h's slots_sum
__global__ __launch_bounds__(kWave) void k_finalize_norm(const float *__restrict__ partials, int parts,
                                                         float *__restrict__ norm)
{
    const int64_t p = blockIdx.x;
    const double acc = slots_sum(partials + p * parts, parts);
    if (threadIdx.x == 0) norm[p] = (float)sqrt(acc);
}

int finalize_norm(const float *partials, int parts, float *norm, int64_t n, hipStream_t s)
{
    if (n == 0) return DPSX_OK;
    k_finalize_norm<<<(unsigned)n, kWave, 0, s>>>(partials, parts, norm);
    return check_launch();
}

// Finalisation + select in ONE small launch (replaces k_finalize_norm + k_argmin after a scoring launch, and does the
// cost combine of SearchDDPM.resample_update): wave w finishes particles w, w + nw, ... in the order of k_finalize_norm
// (bit-identical values), then the block runs the torch.argmin-order select over them.
// Measured and removed (r02): finishing inside the scoring launch (a "last block done" arrival, as common.h's NormTail
// still does for the fused forward step's norm) cost every short scoring block two dependent memory round trips while it
// held its LDS -- 42 us instead of ~25 us at N = 64.  The scoring launches leave partial sums only.
constexpr int kSelThreads = 1024;
// the cost-finishing loop of the finalisation launches (k_finalize_select*, k_finalize_topb): one copy, so a particle's
// cost is the same bits whichever of them finishes it.  `writer`: this block stores the costs.  [lo, hi): the particles this
// block finishes.  each(v, p): called by lane 0 of the wave that finished particle p, with its (combined) cost.
template <class Each>
__device__ __forceinline__ void finalize_costs(const CostArgs &t, const bool writer, const int lo, const int hi, Each &&each)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = kSelThreads / kWave;
    constexpr int B = 4;          // particles per wave in flight: their partial loads are issued together (one latency);
                                  // each particle's adds are in the order of common.h's slots_sum
    for (int p0 = lo + wave; p0 < hi; p0 += nw * B) {
        double acc[B];
#pragma unroll
        for (int b = 0; b < B; ++b) acc[b] = 0.0;
        for (int i = lane; i < t.parts; i += kWave) {
            float v[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const int p = min(p0 + b * nw, hi - 1);              // surplus slots re-read the last particle
                v[b] = t.partials[(int64_t)p * t.parts + i];
            }
#pragma unroll
            for (int b = 0; b < B; ++b) acc[b] += (double)v[b];
        }
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const int p = p0 + b * nw;
            if (p >= hi) break;                                       // wave-uniform
            double a = acc[b];
            wave_sum_f64(a);
            float v = t.mode == COST_L1SQ ? (float)(a * a * (double)t.l1_scale) : (float)sqrt(a);
            if (lane == 0) {
                if (t.raw_out && writer) t.raw_out[p] = v;
                if (t.prev) {
                    const float q = t.prev[p];
                    if (t.potential == POT_MEAN) v = v + q;
                    else if (t.potential == POT_MIN) v = (v != v || q != q) ? __builtin_nanf("") : fminf(v, q);
                    else if (t.potential == POT_DIFF) v = v - q;
                }
                if (writer) t.out[p] = v;
                each(v, p);
            }
        }
    }
}

// the body of the finalisation + select; `writer`: this block stores the costs / the select's outputs (with several blocks
// -- k_finalize_select_copy -- every block computes the same values in the same order and ONE of them stores).
// -> the winner's index (block-uniform, valid in every thread), -1 when no select was asked for.
// [lo, hi): the particles this block finishes and selects over (a segment of a multi-image batch; 0, t.n otherwise) -- each
// particle's value comes out of the same loads and adds whatever the range, so segmented and whole launches agree bit for
// bit; the winner (a global particle index) goes to best_idx[slot] / best_val[slot].
__device__ __forceinline__ int64_t finalize_select_body(const CostArgs &t, const bool writer, const int lo, const int hi,
                                                        const int slot)
{
    __shared__ float s_v[kSelThreads / kWave];
    __shared__ int64_t s_i[kSelThreads / kWave];
    __shared__ int64_t s_best;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave, nw = kSelThreads / kWave;
    ArgMin best{0.0f, -1};
    finalize_costs(t, writer, lo, hi, [&](float v, int p) {
        const ArgMin c{v, p};
        if (argmin_better(c, best)) best = c;
    });
    if (!t.best_idx) return -1;
    if (lane == 0) { s_v[wave] = best.v; s_i[wave] = best.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) {
            const ArgMin c{s_v[w], s_i[w]};
            if (argmin_better(c, best)) best = c;
        }
        s_best = best.i < 0 ? lo : best.i;
        if (writer) {
            t.best_idx[slot] = s_best;
            if (t.best_val) t.best_val[slot] = best.v;
        }
    }
    __syncthreads();
    return s_best;
}

// block m finishes and selects over the particles [m k, (m + 1) k) of segment m (one block and k = t.n: the whole set)
__global__ __launch_bounds__(kSelThreads) void k_finalize_select(CostArgs t, int k)
{
    const int m = blockIdx.x;
    (void)finalize_select_body(t, true, m * k, (m + 1) * k, m);
}

// the same + ONE copy of each segment's winner (the single-state search step): block (x, m) finishes segment m's costs
// and select for itself (k * parts floats from the L2 -- 12 KB at N = 64) and copies slice x of its winner to dst[m];
// one launch and one launch boundary less than finalisation + dpsx_replicate_f32(n_out = 1)
__global__ __launch_bounds__(kSelThreads) void k_finalize_select_copy(CostArgs t, int k, const float *__restrict__ src,
                                                                      float *__restrict__ dst, int64_t chw4)
{
    const int m = blockIdx.y;
    const int64_t b = finalize_select_body(t, blockIdx.x == 0, m * k, (m + 1) * k, m);
    const int64_t i = (int64_t)blockIdx.x * kSelThreads + threadIdx.x;
    if (i < chw4)
        (reinterpret_cast<float4 *>(dst) + (int64_t)m * chw4)[i] = (reinterpret_cast<const float4 *>(src) + b * chw4)[i];
}

int finalize_select(const CostArgs &t, int segments, hipStream_t s)
{
    if (t.n == 0) return DPSX_OK;
    k_finalize_select<<<(unsigned)segments, kSelThreads, 0, s>>>(t, t.n / segments);
    return check_launch();
}

int finalize_select_copy(const CostArgs &t, int segments, const float *src, float *dst, int64_t chw, hipStream_t s)
{
    if (t.n == 0) return DPSX_OK;
    const int64_t chw4 = chw / 4;
    const dim3 grid((unsigned)((chw4 + kSelThreads - 1) / kSelThreads), (unsigned)segments);
    k_finalize_select_copy<<<grid, kSelThreads, 0, s>>>(t, t.n / segments, src, dst, chw4);
    return check_launch();
}

// ---- top-B select: the first b particles of a segment under argmin_better's total order, in that order (rank 0 is what
// the selects above return).  The order as integers: an order-preserving uint32 key of the cost (NaN -> 0, below -inf's
// 0x007fffff; -0.0 and +0.0 share a key), ties broken by the lower index -- (key << 32 | index) as one 64-bit integer.
// Rank r is the particle with r such integers below its own: a property of the segment, not of how the work is split, and
// every output slot has exactly one writer (no atomics).  Two forms, chosen by the segment length (measured: DESIGN.md
// "beam search"): up to kTopbCountMax particles a thread per candidate COUNTS the pairs before its own (every lane reads the
// same LDS words: broadcasts, no barrier after the load); above it the block SORTS the 64-bit integers (LDS bitonic
// network), since the count grows with the square of the length.
#ifndef DPSX_TOPB_COUNT_MAX
#define DPSX_TOPB_COUNT_MAX 512          // overridden only to measure one form alone over all lengths
#endif
constexpr int kTopbCountMax = DPSX_TOPB_COUNT_MAX;

__device__ __forceinline__ uint32_t order_key(float v)
{
    if (v != v) return 0u;
    if (v == 0.0f) return 0x80000000u;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// one segment's select state in LDS: the costs, and the keys -- uint32 [k] for the count, uint64 (key << 32 | index) [the
// power of two >= k] for the sort
struct TopbLds {
    unsigned long long sort[kTopbMaxK];
    float val[kTopbMaxK];
};

__device__ __forceinline__ int topb_pow2(const int k)
{
    int p = 1;
    while (p < k) p <<= 1;
    return p;
}

// entry j of the segment (any thread, each j once)
__device__ __forceinline__ void topb_put(TopbLds &l, const int k, const int j, const float v)
{
    l.val[j] = v;
    if (k > kTopbCountMax) l.sort[j] = ((unsigned long long)order_key(v) << 32) | (unsigned)j;
    else reinterpret_cast<uint32_t *>(l.sort)[j] = order_key(v);
}

// the count.  keys[0 .. k rounded up to 4): the surplus holds 0xffffffff (no cost has that key).  Candidate i's wave reads
// the keys in three runs -- all j below its 64 candidates (j < i: key <= counts), its own 64 (the full comparison), all j
// above (key < counts) -- so the long runs cost one compare and one add per pair.
__device__ __forceinline__ void topb_count_store(const TopbLds &l, const int k, const int b, const int64_t base,
                                                 int64_t *idx, float *val)
{
    const uint32_t *keys = reinterpret_cast<const uint32_t *>(l.sort);
    const uint4 *k4 = reinterpret_cast<const uint4 *>(l.sort);
    const int n4 = (k + 3) / 4;
    for (int i = threadIdx.x; i < k; i += kSelThreads) {
        const uint32_t ki = keys[i];
        const int q0 = __builtin_amdgcn_readfirstlane(i) / kWave * (kWave / 4), q1 = min(q0 + kWave / 4, n4);
        int cnt = 0;
        for (int q = 0; q < q0; ++q) {
            const uint4 c = k4[q];
            cnt += (c.x <= ki) + (c.y <= ki) + (c.z <= ki) + (c.w <= ki);
        }
        for (int q = q0; q < q1; ++q) {
            const uint4 c = k4[q];
            const int j = 4 * q;
            cnt += (c.x < ki || (c.x == ki && j < i)) + (c.y < ki || (c.y == ki && j + 1 < i)) +
                   (c.z < ki || (c.z == ki && j + 2 < i)) + (c.w < ki || (c.w == ki && j + 3 < i));
        }
        for (int q = q1; q < n4; ++q) {
            const uint4 c = k4[q];
            cnt += (c.x < ki) + (c.y < ki) + (c.z < ki) + (c.w < ki);
        }
        if (cnt < b) {
            idx[cnt] = base + i;
            if (val) val[cnt] = l.val[i];
        }
    }
}

// the sort: an ascending bitonic network over sort[0 .. n2), n2 the power of two >= k, the surplus holding all ones (above
// every entry); the integers are distinct, so the outcome is the one sorted sequence
__device__ __forceinline__ void topb_sort_store(TopbLds &l, const int k, const int b, const int64_t base, int64_t *idx,
                                                float *val)
{
    const int n2 = topb_pow2(k);
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n2 / 2; t += kSelThreads) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;      // the pair t of this stage
                const unsigned long long x = l.sort[lo], y = l.sort[hi];
                if ((x > y) == ((lo & size) == 0)) { l.sort[lo] = y; l.sort[hi] = x; }
            }
            __syncthreads();
        }
    for (int r = threadIdx.x; r < b; r += kSelThreads) {
        const int i = (int)(unsigned)l.sort[r];
        idx[r] = base + i;
        if (val) val[r] = l.val[i];
    }
}

// all threads, after every entry has been put: the surplus keys, the barrier, the select
__device__ __forceinline__ void topb_select_store(TopbLds &l, const int k, const int b, const int64_t base, int64_t *idx,
                                                  float *val)
{
    if (k > kTopbCountMax) {               // block-uniform
        for (int j = k + threadIdx.x; j < topb_pow2(k); j += kSelThreads) l.sort[j] = ~0ull;
        __syncthreads();
        topb_sort_store(l, k, b, base, idx, val);
    } else {
        for (int j = k + threadIdx.x; j < ((k + 3) & ~3); j += kSelThreads) reinterpret_cast<uint32_t *>(l.sort)[j] = 0xffffffffu;
        __syncthreads();
        topb_count_store(l, k, b, base, idx, val);
    }
}

// block m finishes the costs of segment m ([m k, (m + 1) k), k <= kTopbMaxK) exactly as k_finalize_select does and stores
// its first b particles: best_idx[m b + r] (global index) / best_val[m b + r] for rank r
__global__ __launch_bounds__(kSelThreads) void k_finalize_topb(CostArgs t, int k, int b)
{
    __shared__ __attribute__((aligned(16))) TopbLds l;
    const int m = blockIdx.x, lo = m * k;
    finalize_costs(t, true, lo, lo + k, [&](float v, int p) { topb_put(l, k, p - lo, v); });
    topb_select_store(l, k, b, lo, t.best_idx + (int64_t)m * b, t.best_val ? t.best_val + (int64_t)m * b : nullptr);
}

// the same select over given values: v [segments, k] -> idx / val (nullable) [segments, b]
__global__ __launch_bounds__(kSelThreads) void k_topk_seg(const float *__restrict__ v, int k, int b, int64_t *__restrict__ idx,
                                                          float *__restrict__ val)
{
    __shared__ __attribute__((aligned(16))) TopbLds l;
    const int64_t m = blockIdx.x, lo = m * k;
    for (int j = threadIdx.x; j < k; j += kSelThreads) topb_put(l, k, j, v[lo + j]);
    topb_select_store(l, k, b, lo, idx + m * b, val ? val + m * b : nullptr);
}

int finalize_topb(const CostArgs &t, int segments, int b, hipStream_t s)
{
    if (t.n == 0) return DPSX_OK;
    k_finalize_topb<<<(unsigned)segments, kSelThreads, 0, s>>>(t, t.n / segments, b);
    return check_launch();
}

int topk_seg_f32(const float *v, int64_t segments, int64_t k, int64_t b, int64_t *idx, float *val, hipStream_t s)
{
    k_topk_seg<<<(unsigned)segments, kSelThreads, 0, s>>>(v, (int)k, (int)b, idx, val);
    return check_launch();
}

__device__ __forceinline__ float norm_coef(float nv, float gn, int power)
{
    // d(gn * norm^power)/d(ax) = -coef * r ;  torch yields 0 where norm == 0
    return power == 2 ? -2.0f * gn : (nv == 0.0f ? 0.0f : -gn / nv);
}

__global__ __launch_bounds__(kThreads) void k_norm_bwd(const float *__restrict__ r, const float *__restrict__ norm,
                                                       const float *__restrict__ g_norm, int power,
                                                       float *__restrict__ g_ax, int64_t m)
{
    const int64_t p = blockIdx.y, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    g_ax[p * m + i] = norm_coef(norm[p], g_norm[p], power) * r[p * m + i];
}

int norm_bwd(const float *r, const float *norm, const float *g_norm, int power, float *g_ax, int64_t n,
             int64_t m, hipStream_t s)
{
    if (n == 0 || m == 0) return DPSX_OK;
    k_norm_bwd<<<grid_for(m, n), kThreads, 0, s>>>(r, norm, g_norm, power, g_ax, m);
    return check_launch();
}

// ===================================================================== unfused tail of step_bwd
__global__ __launch_bounds__(kThreads) void k_clamp_scale(const float *__restrict__ g_x0,
                                                          const float *__restrict__ norm,
                                                          const uint8_t *__restrict__ ins, float scale, int power,
                                                          float *__restrict__ g_mo, int64_t chw, Coefs k,
                                                          const float *__restrict__ g_extra)
{
    const int64_t p = blockIdx.y, i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= chw) return;
    const float coef = norm_coef(norm[p], scale, power);  // g_x0 holds A^T r; cotangent is coef * A^T r
    float g0 = coef * g_x0[p * chw + i];
    if (g_extra) g0 += g_extra[p * chw + i];
    const float gp = ins[p * chw + i] ? g0 : 0.0f;
    g_mo[p * 2 * chw + i] = -k.b * gp;
}

int clamp_scale_to_eps(const float *g_x0, const float *norm, const uint8_t *inside, float scale, int power,
                       float *g_model_out, int64_t n, int64_t chw, const Coefs &k, hipStream_t s,
                       const float *g_extra)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    k_clamp_scale<<<grid_for(chw, n), kThreads, 0, s>>>(g_x0, norm, inside, scale, power, g_model_out, chw, k,
                                                        g_extra);
    return check_launch();
}

// ===================================================================== S4 update
// x_{t-1} = sample - (a*g_pre + g_unet),  a*g_pre = (-a/b) * g_eps
template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_step_update(const float *__restrict__ sm,
                                                          const float *__restrict__ g_mo,
                                                          const float *__restrict__ gu, float *__restrict__ out,
                                                          int64_t chw, float ratio)
{
    const int64_t p = blockIdx.y;
    const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * (VEC ? 4 : 1);
    if (i >= chw) return;
    const int64_t o = p * chw + i, e = p * 2 * chw + i;
    if constexpr (VEC) {
        const float4 s4 = *reinterpret_cast<const float4 *>(sm + o);
        const float4 g4 = *reinterpret_cast<const float4 *>(g_mo + e);
        float4 u4 = make_float4(0, 0, 0, 0);
        if (gu) u4 = *reinterpret_cast<const float4 *>(gu + o);
        float4 r4;
        r4.x = s4.x - (ratio * g4.x + u4.x);
        r4.y = s4.y - (ratio * g4.y + u4.y);
        r4.z = s4.z - (ratio * g4.z + u4.z);
        r4.w = s4.w - (ratio * g4.w + u4.w);
        *reinterpret_cast<float4 *>(out + o) = r4;
    } else {
        out[o] = sm[o] - (ratio * g_mo[e] + (gu ? gu[o] : 0.0f));
    }
}

int step_update(const float *sample, const float *g_mo, const float *g_unet, float *x_next, int64_t n,
                int64_t chw, const Coefs &k, hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    const float ratio = -k.a / k.b;
    const bool vec = chw % 4 == 0 && aligned16(sample) && aligned16(g_mo) && aligned16(g_unet) && aligned16(x_next);
    if (vec)
        k_step_update<true><<<grid_for(chw / 4, n), kThreads, 0, s>>>(sample, g_mo, g_unet, x_next, chw, ratio);
    else
        k_step_update<false><<<grid_for(chw, n), kThreads, 0, s>>>(sample, g_mo, g_unet, x_next, chw, ratio);
    return check_launch();
}

__global__ __launch_bounds__(kThreads) void k_plain_update(const float *__restrict__ sm,
                                                           const float *__restrict__ ga,
                                                           const float *__restrict__ gb, float *__restrict__ out,
                                                           int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    const float g = gb ? __fadd_rn(ga[i], gb[i]) : ga[i];
    out[i] = __fsub_rn(sm[i], g);
}

int plain_update(const float *sample, const float *ga, const float *gb, float *out, int64_t count, hipStream_t s)
{
    if (count == 0) return DPSX_OK;
    k_plain_update<<<(unsigned)((count + kThreads - 1) / kThreads), kThreads, 0, s>>>(sample, ga, gb, out, count);
    return check_launch();
}

// index of element i of a [C, H, W] particle in the [H, W] mask.  A 64-bit remainder by a run-time divisor is a software
// routine of a hundred-odd instructions -- more than the rest of these kernels; particles below 2^32 elements (all of them)
// take the 32-bit form.
__device__ __forceinline__ int64_t mask_index(int64_t i, int64_t chw, int64_t hw)
{
    if (chw <= 0xffffffffll) return (int64_t)((unsigned)i % (unsigned)hw);      // launch-uniform
    return i % hw;
}

// ===================================================================== inpainting fused step
// fwd: S1 + r = y - mask*x0 (not stored) + norm partials.   bwd: recompute r from x0_hat.
template <bool RNG>       // the noise drawn in the kernel from a.rng (common.h: rng_unit) instead of read from a.noise
__global__ __launch_bounds__(kThreads) void k_mask_step_fwd(StepFwdArgs a, const float *__restrict__ mask,
                                                            int64_t chw, int64_t hw)
{
    __shared__ float scratch[kThreads / kWave];
    const int64_t p = blockIdx.y;
    float acc = 0.0f;
    // each block covers 4*kThreads consecutive elements of one particle
    const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (i < chw) {
        const int64_t o = p * chw + i, e = p * 2 * chw + i;
        const float4 xv = *reinterpret_cast<const float4 *>(a.x_t + o);
        const float4 ev = *reinterpret_cast<const float4 *>(a.model_out + e);
        float4 vv = make_float4(0, 0, 0, 0), zv = vv;
        if (a.k.add_noise & 1) {
            vv = *reinterpret_cast<const float4 *>(a.model_out + e + chw);
            if constexpr (!RNG) zv = *reinterpret_cast<const float4 *>(a.noise + o);
        }
        const float4 mv = *reinterpret_cast<const float4 *>(mask + (int64_t)meas_row((unsigned)p, a.mask_div) * hw +
                                                            mask_index(i, chw, hw));
        const float4 yv = *reinterpret_cast<const float4 *>(a.y + (int64_t)meas_row((unsigned)p, a.y_div) * chw + i);
        bool b0, b1, b2, b3;
        float4 x0, sm;
        x0.x = post_x0(xv.x, ev.x, a.k, b0);
        x0.y = post_x0(xv.y, ev.y, a.k, b1);
        x0.z = post_x0(xv.z, ev.z, a.k, b2);
        x0.w = post_x0(xv.w, ev.w, a.k, b3);
        if constexpr (RNG)
            if (a.k.add_noise & 1) zv = rng_unit(a.rng, (uint32_t)(i >> 2), rng_particle(a.rng, (unsigned)p));
        sm.x = post_sample(xv.x, x0.x, vv.x, zv.x, a.k);
        sm.y = post_sample(xv.y, x0.y, vv.y, zv.y, a.k);
        sm.z = post_sample(xv.z, x0.z, vv.z, zv.z, a.k);
        sm.w = post_sample(xv.w, x0.w, vv.w, zv.w, a.k);
        *reinterpret_cast<float4 *>(a.x0_hat + o) = x0;
        *reinterpret_cast<float4 *>(a.sample + o) = sm;
        *reinterpret_cast<uchar4 *>(a.inside + o) = make_uchar4(b0, b1, b2, b3);
        const float d0 = __fsub_rn(yv.x, __fmul_rn(x0.x, mv.x)), d1 = __fsub_rn(yv.y, __fmul_rn(x0.y, mv.y));
        const float d2 = __fsub_rn(yv.z, __fmul_rn(x0.z, mv.z)), d3 = __fsub_rn(yv.w, __fmul_rn(x0.w, mv.w));
        acc = d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
    }
    const float t = block_sum(acc, scratch);
    if (threadIdx.x == 0) tail_publish(&a.partials[p * gridDim.x + blockIdx.x], t, a.tail.counters != nullptr);
    tail_arrive(a.tail, (int)p);
}

int mask_step_fwd(const dpsx_op *op, const StepFwdArgs &f, int parts, hipStream_t s)
{
    const int64_t chw = f.c * f.h * f.w;
    StepFwdArgs a = f;
    a.tail.blocks_per_particle = parts;
    if (a.use_rng) k_mask_step_fwd<true><<<dim3(parts, (unsigned)a.n), kThreads, 0, s>>>(a, op->mask, chw, a.h * a.w);
    else k_mask_step_fwd<false><<<dim3(parts, (unsigned)a.n), kThreads, 0, s>>>(a, op->mask, chw, a.h * a.w);
    return check_launch();
}

__global__ __launch_bounds__(kThreads) void k_mask_step_bwd(StepBwdArgs a, const float *__restrict__ mask,
                                                            int64_t chw, int64_t hw)
{
    __shared__ float s_nrm[1];
    const int64_t p = blockIdx.y;
    const int64_t i = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (!a.norm) {                                   // block-uniform: derive the norm from the forward half's partials
        particle_norm_to_lds(a.partials, a.parts, p, s_nrm);
        __syncthreads();
        if (a.norm_out && blockIdx.x == 0 && threadIdx.x == 0) a.norm_out[p] = s_nrm[0];
    }
    if (i >= chw) return;
    const int64_t o = p * chw + i;
    const float coef = norm_coef(a.norm ? a.norm[p] : s_nrm[0], a.scale, a.power);  // cotangent on A x0 is coef * r
    const float4 x0 = *reinterpret_cast<const float4 *>(a.x0_hat + o);
    const float4 mv = *reinterpret_cast<const float4 *>(mask + (int64_t)meas_row((unsigned)p, a.mask_div) * hw +
                                                        mask_index(i, chw, hw));
    const float4 yv = *reinterpret_cast<const float4 *>(a.y + (int64_t)meas_row((unsigned)p, a.y_div) * chw + i);
    const uchar4 in = *reinterpret_cast<const uchar4 *>(a.inside + o);
    float4 g;
    // A^T = multiply by mask again; then clamp gate; then d/d eps = -b
    float4 ex = make_float4(0, 0, 0, 0);
    if (a.g_extra) ex = *reinterpret_cast<const float4 *>(a.g_extra + o);     // block-uniform
    g.x = in.x ? -a.k.b * (coef * __fsub_rn(yv.x, __fmul_rn(x0.x, mv.x)) * mv.x + ex.x) : 0.0f;
    g.y = in.y ? -a.k.b * (coef * __fsub_rn(yv.y, __fmul_rn(x0.y, mv.y)) * mv.y + ex.y) : 0.0f;
    g.z = in.z ? -a.k.b * (coef * __fsub_rn(yv.z, __fmul_rn(x0.z, mv.z)) * mv.z + ex.z) : 0.0f;
    g.w = in.w ? -a.k.b * (coef * __fsub_rn(yv.w, __fmul_rn(x0.w, mv.w)) * mv.w + ex.w) : 0.0f;
    *reinterpret_cast<float4 *>(a.g_model_out + p * 2 * chw + i) = g;
}

int mask_step_bwd(const dpsx_op *op, const StepBwdArgs &a, hipStream_t s)
{
    const int64_t chw = a.c * a.h * a.w;
    k_mask_step_bwd<<<grid_for(chw / 4, a.n), kThreads, 0, s>>>(a, op->mask, chw, a.h * a.w);
    return check_launch();
}

// ===================================================================== select
// torch.argmin: first minimum; NaN is the minimum.  One block per segment; k is small (<= a few thousand).
// (value, index) pairs are reduced with a total order -- NaN before everything, then the smaller value, then the
// smaller index -- by wave shuffles and one LDS hop, so the result does not depend on the reduction shape.
// (ArgMin / argmin_better: common.h, shared with the in-launch tail)
// block m selects over v[m k .. (m + 1) k) and stores the global index (one segment: the plain argmin)
__global__ __launch_bounds__(kThreads) void k_argmin_seg(const float *__restrict__ v, int64_t k, int64_t *__restrict__ out,
                                                         float *__restrict__ val_out)
{
    __shared__ float s_val[kThreads / kWave];
    __shared__ int64_t s_idx[kThreads / kWave];
    const int64_t m = blockIdx.x;
    ArgMin best{0.0f, -1};
    for (int64_t i = threadIdx.x; i < k; i += kThreads) {
        const ArgMin c{v[m * k + i], i};
        if (argmin_better(c, best)) best = c;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        ArgMin c;
        c.v = __shfl_down(best.v, o, kWave);
        c.i = __shfl_down(best.i, o, kWave);
        if (argmin_better(c, best)) best = c;
    }
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) { s_val[wave] = best.v; s_idx[wave] = best.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads / kWave; ++w) {
            const ArgMin c{s_val[w], s_idx[w]};
            if (argmin_better(c, best)) best = c;
        }
        out[m] = m * k + (best.i < 0 ? 0 : best.i);
        if (val_out) val_out[m] = best.v;
    }
}

int argmin_seg_f32(const float *v, int64_t segments, int64_t k, int64_t *idx, float *val, hipStream_t s)
{
    k_argmin_seg<<<(unsigned)segments, kThreads, 0, s>>>(v, k, idx, val);
    return check_launch();
}

__global__ __launch_bounds__(kThreads) void k_gather(const float *__restrict__ src, const int64_t *__restrict__ ids,
                                                     float *__restrict__ dst, int64_t n_src, int64_t chw4)
{
    const int64_t p = blockIdx.y;
    const int64_t sidx = ids[p];
    float4 *d4 = reinterpret_cast<float4 *>(dst) + p * chw4;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= chw4) return;
    // never read out of bounds: an id outside [0, n_src) poisons its destination particle with NaN (visible in every
    // later score) instead of faulting -- the ids come from the device (argmin / multinomial), no host check
    if (sidx < 0 || sidx >= n_src) {
        const float q = __builtin_nanf("");
        d4[i] = make_float4(q, q, q, q);
        return;
    }
    d4[i] = (reinterpret_cast<const float4 *>(src) + sidx * chw4)[i];
}

__global__ __launch_bounds__(kThreads) void k_gather_scalar(const float *__restrict__ src,
                                                            const int64_t *__restrict__ ids,
                                                            float *__restrict__ dst, int64_t n_src, int64_t chw)
{
    const int64_t p = blockIdx.y;
    const int64_t sidx = ids[p];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= chw) return;
    dst[p * chw + i] = (sidx < 0 || sidx >= n_src) ? __builtin_nanf("") : src[sidx * chw + i];
}

// replication (k_replicate_seg, k_select_champion): one block per (slice, group of kRepl destination particles) -- 8x
// fewer, fatter blocks than one per destination particle
constexpr int kRepl = 8;

// ---- the device half of the per-rank champion exchange (distributed.py: _exchange_champions)
// pack: out[0 .. chw) = particles[best], out[chw] = value (costs[best] or *val), out[chw + 1] = (float)best, two zeros --
// what ONE all-gather then carries to every rank.  best == nullptr: the torch.argmin-order select over costs runs here
// (every block recomputes it: n <= a few thousand floats from L2, cheaper than a launch of its own).
__global__ __launch_bounds__(kThreads) void k_pack_champion(const float *__restrict__ particles, const float *__restrict__ costs,
                                                            const int64_t *__restrict__ best_in,
                                                            const float *__restrict__ val_in, float *__restrict__ out,
                                                            int64_t n, int64_t chw4)
{
    __shared__ float s_val[kThreads / kWave];
    __shared__ int64_t s_idx[kThreads / kWave];
    __shared__ float s_bv;
    __shared__ int64_t s_bi;
    if (best_in) {
        if (threadIdx.x == 0) {         // (an index outside [0, n) yields a NaN record, never an out-of-bounds read)
            const int64_t bi = best_in[0];
            s_bi = bi;
            s_bv = val_in ? val_in[0] : ((bi >= 0 && bi < n) ? costs[bi] : __builtin_nanf(""));
        }
    } else {
        ArgMin best{0.0f, -1};
        for (int64_t i = threadIdx.x; i < n; i += kThreads) {
            const ArgMin c{costs[i], i};
            if (argmin_better(c, best)) best = c;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            ArgMin c;
            c.v = __shfl_down(best.v, o, kWave);
            c.i = __shfl_down(best.i, o, kWave);
            if (argmin_better(c, best)) best = c;
        }
        const int wave = threadIdx.x / kWave;
        if (threadIdx.x % kWave == 0) { s_val[wave] = best.v; s_idx[wave] = best.i; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kThreads / kWave; ++w) {
                const ArgMin c{s_val[w], s_idx[w]};
                if (argmin_better(c, best)) best = c;
            }
            s_bi = best.i < 0 ? 0 : best.i;
            s_bv = best.v;
        }
    }
    __syncthreads();
    const int64_t b = s_bi;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    float4 *o4 = reinterpret_cast<float4 *>(out);
    if (i < chw4) {
        const float q = __builtin_nanf("");
        o4[i] = (b < 0 || b >= n) ? make_float4(q, q, q, q) : (reinterpret_cast<const float4 *>(particles) + b * chw4)[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) o4[chw4] = make_float4(s_bv, (float)b, 0.0f, 0.0f);
}

// select: table [world][chw + 4] as gathered; winner rank = torch.argmin order over table[r][chw] (first minimum, NaN
// counts as the minimum: lowest rank wins ties); dst[p] = table[winner][0 .. chw) for p < n_out; optional outputs: the
// winner's rank and its local index (table[winner][chw + 1]).
__global__ __launch_bounds__(kThreads) void k_select_champion(const float *__restrict__ table, int world, int64_t chw4,
                                                              float *__restrict__ dst, int64_t n_out,
                                                              int64_t *__restrict__ win_rank, int64_t *__restrict__ win_local)
{
    __shared__ int s_w;
    if (threadIdx.x < kWave) {
        ArgMin best{0.0f, -1};
        for (int r = threadIdx.x; r < world; r += kWave) {
            const ArgMin c{table[(int64_t)r * (chw4 + 1) * 4 + chw4 * 4], (int64_t)r};
            if (argmin_better(c, best)) best = c;
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            ArgMin c;
            c.v = __shfl_down(best.v, o, kWave);
            c.i = __shfl_down(best.i, o, kWave);
            if (argmin_better(c, best)) best = c;
        }
        if (threadIdx.x == 0) s_w = best.i < 0 ? 0 : (int)best.i;
    }
    __syncthreads();
    const int wr = s_w;
    const float4 *src = reinterpret_cast<const float4 *>(table) + (int64_t)wr * (chw4 + 1);
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (win_rank) *win_rank = wr;
        if (win_local) *win_local = (int64_t)src[chw4].y;
    }
    if (i >= chw4) return;
    const float4 v = src[i];
    const int64_t p0 = (int64_t)blockIdx.y * kRepl;
    float4 *d4 = reinterpret_cast<float4 *>(dst) + p0 * chw4 + i;
#pragma unroll
    for (int k = 0; k < kRepl; ++k)
        if (p0 + k < n_out) d4[(int64_t)k * chw4] = v;
}

int pack_champion(const float *particles, const float *costs, const int64_t *best, const float *val, float *out, int64_t n,
                  int64_t chw, hipStream_t s)
{
    const int64_t chw4 = chw / 4;
    k_pack_champion<<<(unsigned)((chw4 + kThreads - 1) / kThreads), kThreads, 0, s>>>(particles, costs, best, val, out, n, chw4);
    return check_launch();
}

int select_champion(const float *table, int world, int64_t chw, float *dst, int64_t n_out, int64_t *win_rank,
                    int64_t *win_local, hipStream_t s)
{
    const int64_t chw4 = chw / 4;
    const dim3 grid((unsigned)((chw4 + kThreads - 1) / kThreads), (unsigned)((n_out + kRepl - 1) / kRepl));
    k_select_champion<<<grid, kThreads, 0, s>>>(table, world, chw4, dst, n_out, win_rank, win_local);
    return check_launch();
}

// dst[p] = src[ids[p / per]]: each segment's winner replicated over its own particles (per = n_out: ONE winner over all).
// Measured (profiles/search_unify_ab.txt): a kernel of its own for the one-winner case, which read the winner once per
// kRepl destinations, was indistinguishable from this one at N = 64 and was removed.
__global__ __launch_bounds__(kThreads) void k_replicate_seg(const float *__restrict__ src, const int64_t *__restrict__ ids,
                                                            float *__restrict__ dst, int64_t n_out, unsigned per,
                                                            int64_t n_src, int64_t chw4)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= chw4) return;
    const int64_t p0 = (int64_t)blockIdx.y * kRepl;
    float4 *d4 = reinterpret_cast<float4 *>(dst) + p0 * chw4 + i;
    const float q = __builtin_nanf("");
#pragma unroll
    for (int k = 0; k < kRepl; ++k) {
        if (p0 + k >= n_out) break;
        const int64_t sidx = ids[(unsigned)(p0 + k) / per];
        d4[(int64_t)k * chw4] = (sidx < 0 || sidx >= n_src) ? make_float4(q, q, q, q)
                                                             : (reinterpret_cast<const float4 *>(src) + sidx * chw4)[i];
    }
}

__global__ __launch_bounds__(kThreads) void k_replicate_seg_scalar(const float *__restrict__ src,
                                                                   const int64_t *__restrict__ ids, float *__restrict__ dst,
                                                                   unsigned per, int64_t n_src, int64_t chw)
{
    const int64_t p = blockIdx.y;
    const int64_t sidx = ids[(unsigned)p / per];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= chw) return;
    dst[p * chw + i] = (sidx < 0 || sidx >= n_src) ? __builtin_nanf("") : src[sidx * chw + i];
}

int replicate_seg_f32(const float *src, const int64_t *ids, float *dst, int64_t n_out, int64_t per, int64_t n_src,
                      int64_t chw, hipStream_t s)
{
    if (n_out == 0 || chw == 0) return DPSX_OK;
    if (chw % 4 == 0 && aligned16(src) && aligned16(dst)) {
        const dim3 grid((unsigned)((chw / 4 + kThreads - 1) / kThreads), (unsigned)((n_out + kRepl - 1) / kRepl));
        k_replicate_seg<<<grid, kThreads, 0, s>>>(src, ids, dst, n_out, (unsigned)per, n_src, chw / 4);
    } else {
        k_replicate_seg_scalar<<<grid_for(chw, n_out), kThreads, 0, s>>>(src, ids, dst, (unsigned)per, n_src, chw);
    }
    return check_launch();
}

int gather_f32(const float *src, const int64_t *ids, float *dst, int64_t n_out, int64_t n_src, int64_t chw, hipStream_t s)
{
    if (n_out == 0 || chw == 0) return DPSX_OK;
    if (chw % 4 == 0 && aligned16(src) && aligned16(dst))
        k_gather<<<grid_for(chw / 4, n_out), kThreads, 0, s>>>(src, ids, dst, n_src, chw / 4);
    else
        k_gather_scalar<<<grid_for(chw, n_out), kThreads, 0, s>>>(src, ids, dst, n_src, chw);
    return check_launch();
}

// ===================================================================== per-segment resampling draw (+ fused gather)
// The draw is a pure function of (distances, uniforms), include/dpsx.h "resampling draw": integer weights
// q_i = rint(exp(-(d_i - d_min) * inv_scale) * 2^24), an exact 64-bit integer CDF, slot j takes the smallest i with
// cdf_i > (total * ui_j) >> 24.  Integer adds are associative, so the shape of the scan below (wave shuffles, tiles of
// kThreads, per-wave totals through LDS) cannot change a result: a segmented launch and one launch per image agree
// bit for bit, and so does a serial restatement on the host.
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
// S2 (the scheme / ESS launches only): *s2 = sum of q_i^2 instead of the flat flag (one more exact integer reduction of
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

// 5. the slot's pick from the finished CDF: the smallest i with cdf_i > (total * ui) >> 24, inside [0, k - 1]
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

__device__ __forceinline__ int resample_pick(const unsigned long long *__restrict__ cdf, const int k, const float u)
{
    return resample_search(cdf, k, (cdf[k - 1] * (unsigned long long)resample_ui(u)) >> 24);
}

// The scheme / ESS forms (include/dpsx.h "resampling schemes and the ESS trigger").  Everything below is integer
// arithmetic on the finished CDF, so it inherits the draw's independence of the launch shape.
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

// slot j's pick: multinomial (total * ui) >> 24; stratified / systematic ((total * (j 2^24 + ui)) >> 24) / k, the product
// up to 2^72, its shifted value below 2^48.  The caller hands the systematic scheme the first slot's ui for every j.
__device__ __forceinline__ int resample_pick_scheme(const unsigned long long *__restrict__ cdf, const int k, const int j,
                                                    const uint32_t ui, const int scheme)
{
    const unsigned long long total = cdf[k - 1];
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

// one block per segment: ids (global particle indices) for every slot of the segment, and the weights when asked
__global__ __launch_bounds__(kThreads) void k_resample_draw_seg(const float *__restrict__ d, const float *__restrict__ u,
                                                                const int k, const float inv_scale,
                                                                int64_t *__restrict__ ids, int32_t *__restrict__ q_out)
{
    extern __shared__ unsigned long long s_cdf[];
    const int64_t lo = (int64_t)blockIdx.x * k;
    const bool flat = resample_cdf(d + lo, k, inv_scale, s_cdf, q_out ? q_out + lo : nullptr, nullptr, -1);
    for (int j = threadIdx.x; j < k; j += kThreads)
        ids[lo + j] = lo + (flat ? j : resample_pick(s_cdf, k, u[lo + j]));
}

// The draw AND the gathers in one launch.  Block (x, p): repeats the draw of p's segment for slot p (k distances from the
// L2, the scan above, one binary search by thread 0) and copies slice x of the drawn particle to dst[p]; the block with
// x == 0 also stores ids_out[p], d_out[p] = d[id] and q_out[p].  U = 4: float4 units (chw % 4 == 0, 16-byte aligned
// bases), PER of them per lane with all loads issued before the stores; U = 1: the same over single floats.
constexpr int kResampleVecPer = 8;            // 256 lanes x 8 x 16 B = 32 KB per block: the repeated scan is a small part
constexpr int kResampleScalarPer = 32;
// slice blockIdx.x of particle `id` of src to particle p of dst, in units of U floats (the fused launches' copy)
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

template <int U, int PER>
__global__ __launch_bounds__(kThreads) void k_resample_seg(const float *__restrict__ d, const float *__restrict__ u,
                                                           const int k, const float inv_scale,
                                                           const float *__restrict__ src, float *__restrict__ dst,
                                                           float *__restrict__ d_out, int64_t *__restrict__ ids,
                                                           int32_t *__restrict__ q_out, const int64_t units)
{
    extern __shared__ unsigned long long s_cdf[];
    __shared__ int s_pick;
    const int64_t p = blockIdx.y;
    const int64_t lo = (p / k) * k;
    const int j = (int)(p - lo);
    const bool writer = blockIdx.x == 0;
    const float uj = u[p];
    const bool flat = resample_cdf(d + lo, k, inv_scale, s_cdf, nullptr, writer && q_out ? q_out + p : nullptr, j);
    if (threadIdx.x == 0) s_pick = flat ? j : resample_pick(s_cdf, k, uj);
    __syncthreads();
    const int64_t id = lo + s_pick;                               // inside the segment by construction
    if (writer && threadIdx.x == 0) {
        ids[p] = id;
        d_out[p] = d[id];
    }
    resample_copy<U, PER>(src, dst, id, p, units);
}

// k_resample_draw_seg with a scheme and the ESS trigger: the same grid, plus the segment's flag and ESS (nullable)
__global__ __launch_bounds__(kThreads) void k_resample_draw_seg_ex(const float *__restrict__ d, const float *__restrict__ u,
                                                                   const int k, const float inv_scale,
                                                                   int64_t *__restrict__ ids, int32_t *__restrict__ q_out,
                                                                   const int scheme, const int ess_q16,
                                                                   uint8_t *__restrict__ flag_out,
                                                                   float *__restrict__ ess_out)
{
    extern __shared__ unsigned long long s_cdf[];
    const int64_t lo = (int64_t)blockIdx.x * k;
    unsigned long long s2;
    resample_cdf<true>(d + lo, k, inv_scale, s_cdf, q_out ? q_out + lo : nullptr, nullptr, -1, &s2);
    const unsigned long long total = s_cdf[k - 1];
    const bool need = resample_need(total, s2, k, ess_q16);
    if (threadIdx.x == 0) {
        if (flag_out) flag_out[blockIdx.x] = need ? 1 : 0;
        if (ess_out) ess_out[blockIdx.x] = resample_ess(total, s2);
    }
    const bool systematic = scheme == DPSX_RESAMPLE_SYSTEMATIC;
    for (int j = threadIdx.x; j < k; j += kThreads)
        ids[lo + j] = lo + (need ? resample_pick_scheme(s_cdf, k, j, resample_ui(u[systematic ? lo : lo + j]), scheme) : j);
}

// k_resample_seg with a scheme and the ESS trigger: the same grid; block (0, first slot of a segment) also stores the
// segment's flag and ESS.  A segment that does not resample is copied as it is.
template <int U, int PER>
__global__ __launch_bounds__(kThreads) void k_resample_seg_ex(const float *__restrict__ d, const float *__restrict__ u,
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
    const float uj = u[scheme == DPSX_RESAMPLE_SYSTEMATIC ? lo : p];
    unsigned long long s2;
    resample_cdf<true>(d + lo, k, inv_scale, s_cdf, nullptr, writer && q_out ? q_out + p : nullptr, j, &s2);
    if (threadIdx.x == 0) {
        const unsigned long long total = s_cdf[k - 1];
        const bool need = resample_need(total, s2, k, ess_q16);
        s_pick = need ? resample_pick_scheme(s_cdf, k, j, resample_ui(uj), scheme) : j;
        if (writer && j == 0) {
            if (flag_out) flag_out[m] = need ? 1 : 0;
            if (ess_out) ess_out[m] = resample_ess(total, s2);
        }
    }
    __syncthreads();
    const int64_t id = lo + s_pick;                               // inside the segment by construction
    if (writer && threadIdx.x == 0) {
        ids[p] = id;
        d_out[p] = d[id];
    }
    resample_copy<U, PER>(src, dst, id, p, units);
}

int resample_draw_seg_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, int64_t *ids,
                          int32_t *q_out, hipStream_t s)
{
    k_resample_draw_seg<<<(unsigned)segments, kThreads, (size_t)k * sizeof(unsigned long long), s>>>(
        d, u, (int)k, inv_scale, ids, q_out);
    return check_launch();
}

int resample_seg_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, const float *src,
                     float *dst, float *d_out, int64_t *ids, int32_t *q_out, int64_t chw, hipStream_t s)
{
    const int64_t n = segments * k;
    const size_t lds = (size_t)k * sizeof(unsigned long long);
    if (chw % 4 == 0 && aligned16(src) && aligned16(dst)) {
        const int64_t units = chw / 4, per_block = (int64_t)kThreads * kResampleVecPer;
        const dim3 grid((unsigned)((units + per_block - 1) / per_block), (unsigned)n);
        k_resample_seg<4, kResampleVecPer><<<grid, kThreads, lds, s>>>(d, u, (int)k, inv_scale, src, dst, d_out, ids,
                                                                        q_out, units);
    } else {
        const int64_t per_block = (int64_t)kThreads * kResampleScalarPer;
        const dim3 grid((unsigned)((chw + per_block - 1) / per_block), (unsigned)n);
        k_resample_seg<1, kResampleScalarPer><<<grid, kThreads, lds, s>>>(d, u, (int)k, inv_scale, src, dst, d_out, ids,
                                                                           q_out, chw);
    }
    return check_launch();
}

int resample_draw_seg_ex_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, int64_t *ids,
                             int32_t *q_out, int scheme, int ess_q16, uint8_t *flag_out, float *ess_out, hipStream_t s)
{
    k_resample_draw_seg_ex<<<(unsigned)segments, kThreads, (size_t)k * sizeof(unsigned long long), s>>>(
        d, u, (int)k, inv_scale, ids, q_out, scheme, ess_q16, flag_out, ess_out);
    return check_launch();
}

int resample_seg_ex_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, const float *src,
                        float *dst, float *d_out, int64_t *ids, int32_t *q_out, int64_t chw, int scheme, int ess_q16,
                        uint8_t *flag_out, float *ess_out, hipStream_t s)
{
    const int64_t n = segments * k;
    const size_t lds = (size_t)k * sizeof(unsigned long long);
    if (chw % 4 == 0 && aligned16(src) && aligned16(dst)) {
        const int64_t units = chw / 4, per_block = (int64_t)kThreads * kResampleVecPer;
        const dim3 grid((unsigned)((units + per_block - 1) / per_block), (unsigned)n);
        k_resample_seg_ex<4, kResampleVecPer><<<grid, kThreads, lds, s>>>(d, u, (int)k, inv_scale, src, dst, d_out, ids,
                                                                           q_out, units, scheme, ess_q16, flag_out, ess_out);
    } else {
        const int64_t per_block = (int64_t)kThreads * kResampleScalarPer;
        const dim3 grid((unsigned)((chw + per_block - 1) / per_block), (unsigned)n);
        k_resample_seg_ex<1, kResampleScalarPer><<<grid, kThreads, lds, s>>>(d, u, (int)k, inv_scale, src, dst, d_out,
                                                                              ids, q_out, chw, scheme, ess_q16, flag_out,
                                                                              ess_out);
    }
    return check_launch();
}

}  // namespace dpsx
