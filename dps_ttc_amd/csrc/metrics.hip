// Per-particle MSE / PSNR / SSIM against the particle's label row (include/dpsx.h: dpsx_image_metrics_f32), at most
// three launches:
//
//   k_label_range   per-image min / max of the label (only when the range is not given), grid (kRangeSlots(chw), m): one
//                   (min, max) pair per block, NaN-propagating like torch's min / max, fixed tree
//   k_metrics_sse   PSNR only: a float4 stream in particle_pass.h's layout, grid (cg_slots(chw), n), one fp32 partial of
//                   sum (x - y)^2 per block (the scalar unit when chw % 4 != 0 or a pointer is unaligned)
//   k_metrics_tile  SSIM (and the same squared-error partials): grid (tiles, n), one 32 x 32 tile of window positions of one
//                   plane per block.  The 42 x 42 inputs of x and of the label row go through LDS as (x, y) pairs; the
//                   horizontal pass (item: a row x 4 outputs) forms x^2, y^2, xy in registers, once per pixel it reads,
//                   and leaves the five 42 x 32 row-filtered maps in LDS -- (E[x], E[y]) and (E[x^2], E[y^2]) as pairs,
//                   so that two maps share one v_pk_fma_f32 with the tap broadcast, E[xy] apart; the vertical pass
//                   (item: a position row x 4 columns) reads them back 16 bytes at a time and evaluates s at its four
//                   positions.  Every tap is an explicit fma in tap order k = 0 .. 10 (a packed fma rounds each half as
//                   fmaf does).  One fp32 partial of sum s per block.
//   k_metrics_finish one wave per particle: slots_sum of both partial arrays in double, mse / psnr / ssim formed in double,
//                   each rounded to fp32 once.
//
// The squared error is a sum in a fixed order, and the full call must give the bits of the PSNR-only call.  So the tile
// launch does not add (x - y)^2 over its staged pixels: block q also runs stream slot q (q + tiles, ...) of k_metrics_sse
// -- the same ranges, the same lanes, the same tree (sse_slot below is the one definition) -- and every pixel, the last 10
// rows and columns included, belongs to exactly one slot.  The extra read of x comes from the cache the tile loads fill.
//
// Slot counts, tile grid and the range split are functions of (c, h, w) only and a block reads only its particle and its
// label row: a particle's numbers do not depend on n, m or its place in the batch, and a NaN stays where the definition puts it.
#include "particle_pass.h"

#include <cmath>

namespace dpsx {

constexpr int kWin = 11, kApron = kWin - 1;
constexpr int kTile = 32;                        // window positions per tile side
constexpr int kReg = kTile + kApron;             // staged inputs per tile side: 42
constexpr int kRawStride = 2 * kReg;             // (x, y) pairs: 84 words, rows stay 16-byte aligned
constexpr int kPairStride = 2 * kTile + 4;       // a row of a pair of maps
constexpr int kMapStride = kTile + 4;

typedef float m2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ m2f pk_fma(float g, m2f v, m2f acc) { return __builtin_elementwise_fma(m2f{g, g}, v, acc); }
constexpr int kRangeMax = 64;                    // range partials per image: one per lane of the wave that joins them

struct SsimTaps { float g[kWin]; };              // by value -> SGPRs

struct MetricsArgs {
    const float *x, *label;
    const float *range_part;     // [m, range_slots, 2] (min, max); null: data_range is given
    float *sse_part, *ssim_part; // [n, sse_slots], [n, tiles] (either nullable: not wanted)
    float *mse, *psnr, *ssim;    // [n] each, nullable
    int64_t chw, per;            // per: work items (float4 units or elements) per squared-error slot
    int c, h, w, tiles_y, tiles_x, tiles, sse_slots, range_slots;
    unsigned div;                // row_div(m, n)
    float data_range;
    SsimTaps taps;
};

// ------------------------------------------------------------------ the label range
// (common.h: nan_min / nan_max -- a NaN in the label is a NaN range, as torch's max - min)
__device__ __forceinline__ void wave_minmax(float &mn, float &mx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = nan_min(mn, __shfl_down(mn, o, kWave));
        mx = nan_max(mx, __shfl_down(mx, o, kWave));
    }
}

__global__ __launch_bounds__(kPassThreads) void k_label_range(const float *__restrict__ label, float *__restrict__ part,
                                                              int64_t chw, int64_t per)
{
    __shared__ float s_mn[kPassThreads / kWave], s_mx[kPassThreads / kWave];
    const float *y = label + (int64_t)blockIdx.y * chw;
    const Range r = block_range(chw, per);
    float mn = INFINITY, mx = -INFINITY;
    for (int64_t i = r.lo + threadIdx.x; i < r.hi; i += kPassThreads) {
        const float v = y[i];
        mn = nan_min(mn, v);
        mx = nan_max(mx, v);
    }
    wave_minmax(mn, mx);
    if ((threadIdx.x & 63) == 0) {
        s_mn[threadIdx.x >> 6] = mn;
        s_mx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < kPassThreads / kWave; ++i) {
            mn = nan_min(mn, s_mn[i]);
            mx = nan_max(mx, s_mx[i]);
        }
        float *o = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        o[0] = mn;
        o[1] = mx;
    }
}

// L of the particle's image: the given range, or max - min of the label from the range launch's partials (one fp32
// subtraction, as real.max() - real.min()).  Called by wave 0; valid in lane 0.  The one definition: the tile launch and
// the finisher get the same bits.
__device__ __forceinline__ float image_range(const MetricsArgs &a, unsigned row)
{
    if (!a.range_part) return a.data_range;              // launch-uniform
    const float *p = a.range_part + (int64_t)row * a.range_slots * 2;
    const bool have = (int)threadIdx.x < a.range_slots;
    float mn = have ? p[2 * threadIdx.x] : INFINITY, mx = have ? p[2 * threadIdx.x + 1] : -INFINITY;
    wave_minmax(mn, mx);
    return __fsub_rn(mx, mn);
}

// ------------------------------------------------------------------ the squared error
// slot q of particle p: the lane's serial sum over its work items, then block_sum; valid in thread 0
template <bool VEC>
__device__ __forceinline__ float sse_slot(const float *__restrict__ xp, const float *__restrict__ yp, int q,
                                          const MetricsArgs &a, float *red)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    const int64_t units = a.chw / W, lo = (int64_t)q * a.per, hi = min(units, lo + a.per);
    float acc = 0.0f;
    for (int64_t u = lo + threadIdx.x; u < hi; u += kPassThreads) {
        const T xv = ld<T>(xp + u * W), yv = ld<T>(yp + u * W);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float d = __fsub_rn(lane(xv, j), lane(yv, j));
            acc = __fadd_rn(acc, __fmul_rn(d, d));
        }
    }
    return block_sum(acc, red);
}

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_metrics_sse(const MetricsArgs a)
{
    __shared__ float red[kPassThreads / kWave];
    const int64_t p = blockIdx.y;
    const float *xp = a.x + p * a.chw, *yp = a.label + (int64_t)meas_row((unsigned)p, a.div) * a.chw;
    const float sum = sse_slot<VEC>(xp, yp, (int)blockIdx.x, a, red);
    if (threadIdx.x == 0) a.sse_part[p * a.sse_slots + blockIdx.x] = sum;
}

// ------------------------------------------------------------------ the window
// Logical slot of a lane for the two LDS passes: 16 consecutive slots are one hardware group of ds_read_b128
// (MI355X_MICROARCH.md, LDS; the dealing of blur_sep.h: sep_slot)
__device__ __forceinline__ int metrics_slot()
{
    const int t = threadIdx.x, l5 = t & 31, q = l5 >> 2;
    const int grp = 2 * ((t >> 5) & 1) + (__popc(q) & 1), pos = 4 * (q >> 1) + (l5 & 3);
    return (t & ~63) | (16 * grp + pos);
}

__device__ __forceinline__ float ssim_point(float mx, float my, float exx, float eyy, float exy, float c1, float c2)
{
    const float mxx = __fmul_rn(mx, mx), myy = __fmul_rn(my, my), mxy = __fmul_rn(mx, my);
    const float vx = __fsub_rn(exx, mxx), vy = __fsub_rn(eyy, myy), cxy = __fsub_rn(exy, mxy);
    const float num = __fmul_rn(__fadd_rn(__fmul_rn(2.0f, mxy), c1), __fadd_rn(__fmul_rn(2.0f, cxy), c2));
    const float den = __fmul_rn(__fadd_rn(__fadd_rn(mxx, myy), c1), __fadd_rn(__fadd_rn(vx, vy), c2));
    return __fdiv_rn(num, den);
}

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_metrics_tile(const MetricsArgs a)
{
    // the staged inputs as (x, y) pairs and the row-filtered maps as (E[x], E[y]) and (E[x^2], E[y^2]) pairs: a 16-byte LDS
    // read is then two operands of v_pk_fma_f32 as they come (two maps per instruction, the tap broadcast), E[xy] apart
    __shared__ __attribute__((aligned(16))) float s_in[kReg * kRawStride];
    __shared__ __attribute__((aligned(16))) float s_m1[kReg * kPairStride], s_m2[kReg * kPairStride], s_mxy[kReg * kMapStride];
    __shared__ float red[kPassThreads / kWave];
    __shared__ float s_l;
    const int64_t p = blockIdx.y;
    const unsigned row = meas_row((unsigned)p, a.div);
    const float *xp = a.x + p * a.chw, *yp = a.label + (int64_t)row * a.chw;

    if (threadIdx.x < kWave) {
        const float l = image_range(a, row);
        if (threadIdx.x == 0) s_l = l;
    }

    // ---- stage the tile's 42 x 42 inputs (zeros outside the image: they feed only positions that are not counted)
    const int t = blockIdx.x, ch = t / (a.tiles_y * a.tiles_x), rem = t - ch * (a.tiles_y * a.tiles_x);
    const int i0 = (rem / a.tiles_x) * kTile, j0 = (rem % a.tiles_x) * kTile;
    const float *xpl = xp + (int64_t)ch * a.h * a.w, *ypl = yp + (int64_t)ch * a.h * a.w;
    // every load of the lane is issued before anything waits (a rolled loop paid one memory round trip per pass: the
    // launch was bound by it); the squared-error slots run while they fly
    constexpr int kStage = (kReg * kReg + kPassThreads - 1) / kPassThreads;
    m2f staged[kStage];
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = threadIdx.x + j * kPassThreads, r = i / kReg, c = i - r * kReg, gr = i0 + r, gc = j0 + c;
        const bool in = i < kReg * kReg && gr < a.h && gc < a.w;
        staged[j] = m2f{in ? xpl[gr * a.w + gc] : 0.0f, in ? ypl[gr * a.w + gc] : 0.0f};
    }

    // ---- the squared-error slots this block runs (from global memory, in k_metrics_sse's order)
    if (a.sse_part)
        for (int q = blockIdx.x; q < a.sse_slots; q += a.tiles) {
            const float sum = sse_slot<VEC>(xp, yp, q, a, red);
            if (threadIdx.x == 0) a.sse_part[p * a.sse_slots + q] = sum;
        }
#pragma unroll
    for (int j = 0; j < kStage; ++j) {
        const int i = threadIdx.x + j * kPassThreads, r = i / kReg, c = i - r * kReg;
        if (i < kReg * kReg) *reinterpret_cast<m2f *>(s_in + r * kRawStride + 2 * c) = staged[j];
    }
    __syncthreads();

    // ---- horizontal pass: item = (row, 4 adjacent outputs); the products once per pixel the item reads
    const int slot = metrics_slot();
    for (int it = slot; it < kReg * (kTile / 4); it += kPassThreads) {
        const int r = it / (kTile / 4), g = it - r * (kTile / 4);
        m2f pv[4 + kApron], qv[4 + kApron];              // (x, y) and (x^2, y^2) of the item's 14 pixels
        float xy[4 + kApron];
#pragma unroll
        for (int j = 0; j < (4 + kApron) / 2; ++j) {
            const float4 v = *reinterpret_cast<const float4 *>(s_in + r * kRawStride + 8 * g + 4 * j);
            pv[2 * j] = m2f{v.x, v.y};
            pv[2 * j + 1] = m2f{v.z, v.w};
        }
#pragma unroll
        for (int k = 0; k < 4 + kApron; ++k) {
            qv[k] = pv[k] * pv[k];
            xy[k] = __fmul_rn(pv[k].x, pv[k].y);
        }
        m2f o1[4], o2[4];
        float o3[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            m2f h1{0.0f, 0.0f}, h2{0.0f, 0.0f};
            float h3 = 0.0f;
#pragma unroll
            for (int k = 0; k < kWin; ++k) {
                const float gk = a.taps.g[k];
                h1 = pk_fma(gk, pv[e + k], h1);
                h2 = pk_fma(gk, qv[e + k], h2);
                h3 = fmaf(gk, xy[e + k], h3);
            }
            o1[e] = h1; o2[e] = h2; o3[e] = h3;
        }
        float *d1 = s_m1 + r * kPairStride + 8 * g, *d2 = s_m2 + r * kPairStride + 8 * g;
        *reinterpret_cast<float4 *>(d1) = make_float4(o1[0].x, o1[0].y, o1[1].x, o1[1].y);
        *reinterpret_cast<float4 *>(d1 + 4) = make_float4(o1[2].x, o1[2].y, o1[3].x, o1[3].y);
        *reinterpret_cast<float4 *>(d2) = make_float4(o2[0].x, o2[0].y, o2[1].x, o2[1].y);
        *reinterpret_cast<float4 *>(d2 + 4) = make_float4(o2[2].x, o2[2].y, o2[3].x, o2[3].y);
        *reinterpret_cast<float4 *>(s_mxy + r * kMapStride + 4 * g) = make_float4(o3[0], o3[1], o3[2], o3[3]);
    }
    __syncthreads();

    // ---- vertical pass and s: item = (position row, 4 adjacent columns), one per thread
    const int i = slot / (kTile / 4), cg = slot - i * (kTile / 4);
    m2f a1[4], a2[4], a3[2];                             // per column (E[x], E[y]), (E[x^2], E[y^2]); E[xy] of column pairs
#pragma unroll
    for (int c = 0; c < 4; ++c) a1[c] = a2[c] = m2f{0.0f, 0.0f};
    a3[0] = a3[1] = m2f{0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
        const float gk = a.taps.g[k];
        const float *m1 = s_m1 + (i + k) * kPairStride + 8 * cg, *m2 = s_m2 + (i + k) * kPairStride + 8 * cg;
        const float4 u0 = *reinterpret_cast<const float4 *>(m1), u1 = *reinterpret_cast<const float4 *>(m1 + 4);
        const float4 w0 = *reinterpret_cast<const float4 *>(m2), w1 = *reinterpret_cast<const float4 *>(m2 + 4);
        const float4 z = *reinterpret_cast<const float4 *>(s_mxy + (i + k) * kMapStride + 4 * cg);
        a1[0] = pk_fma(gk, m2f{u0.x, u0.y}, a1[0]);
        a1[1] = pk_fma(gk, m2f{u0.z, u0.w}, a1[1]);
        a1[2] = pk_fma(gk, m2f{u1.x, u1.y}, a1[2]);
        a1[3] = pk_fma(gk, m2f{u1.z, u1.w}, a1[3]);
        a2[0] = pk_fma(gk, m2f{w0.x, w0.y}, a2[0]);
        a2[1] = pk_fma(gk, m2f{w0.z, w0.w}, a2[1]);
        a2[2] = pk_fma(gk, m2f{w1.x, w1.y}, a2[2]);
        a2[3] = pk_fma(gk, m2f{w1.z, w1.w}, a2[3]);
        a3[0] = pk_fma(gk, m2f{z.x, z.y}, a3[0]);
        a3[1] = pk_fma(gk, m2f{z.z, z.w}, a3[1]);
    }
    // C1 = (0.01 L)^2, C2 = (0.03 L)^2: formed in double, rounded to fp32 once
    const double l = (double)s_l;
    const float c1 = (float)((0.01 * l) * (0.01 * l)), c2 = (float)((0.03 * l) * (0.03 * l));
    const int pi = i0 + i, pj = j0 + 4 * cg, ph = a.h - kApron, pw = a.w - kApron;
    const bool rok = pi < ph;
    float sum = 0.0f;
    {
        const float s0 = ssim_point(a1[0].x, a1[0].y, a2[0].x, a2[0].y, a3[0].x, c1, c2);
        const float s1 = ssim_point(a1[1].x, a1[1].y, a2[1].x, a2[1].y, a3[0].y, c1, c2);
        const float s2 = ssim_point(a1[2].x, a1[2].y, a2[2].x, a2[2].y, a3[1].x, c1, c2);
        const float s3 = ssim_point(a1[3].x, a1[3].y, a2[3].x, a2[3].y, a3[1].y, c1, c2);
        sum = __fadd_rn(sum, rok && pj < pw ? s0 : 0.0f);
        sum = __fadd_rn(sum, rok && pj + 1 < pw ? s1 : 0.0f);
        sum = __fadd_rn(sum, rok && pj + 2 < pw ? s2 : 0.0f);
        sum = __fadd_rn(sum, rok && pj + 3 < pw ? s3 : 0.0f);
    }
    const float total = block_sum(sum, red);
    if (threadIdx.x == 0) a.ssim_part[p * a.tiles + blockIdx.x] = total;
}

// ------------------------------------------------------------------ the finisher: one wave per particle
__global__ __launch_bounds__(kWave) void k_metrics_finish(const MetricsArgs a)
{
    const int64_t p = blockIdx.x;
    const double sse = a.sse_part ? slots_sum(a.sse_part + p * a.sse_slots, a.sse_slots) : 0.0;
    const double ssum = a.ssim_part ? slots_sum(a.ssim_part + p * a.tiles, a.tiles) : 0.0;
    const float lf = a.psnr ? image_range(a, meas_row((unsigned)p, a.div)) : 0.0f;
    if (threadIdx.x != 0) return;
    const double mse = sse / (double)a.chw;
    if (a.mse) a.mse[p] = (float)mse;
    if (a.psnr) {
        const double l = (double)lf;
        a.psnr[p] = (float)(10.0 * log10(l * l / mse));
    }
    if (a.ssim) a.ssim[p] = (float)(ssum / ((double)a.c * (double)(a.h - kApron) * (double)(a.w - kApron)));
}

// ------------------------------------------------------------------ host side
static int range_slots(int64_t chw) { return (int)std::min<int64_t>(kRangeMax, cg_slots(chw)); }
static int64_t tiles_of(int64_t extent) { return extent < kWin ? 0 : (extent - kApron + kTile - 1) / kTile; }
static int64_t tile_count(int64_t c, int64_t h, int64_t w) { return c * tiles_of(h) * tiles_of(w); }

// THE workspace layout: the partials of the three launches; returns the bytes (the size query and the launch path both
// walk it)
static int64_t metrics_layout(MetricsArgs &a, Carver cv, int64_t n, int64_t m, int64_t c, int64_t h, int64_t w)
{
    const int64_t chw = c * h * w;
    a.range_part = cv.take<float>(m * range_slots(chw) * 2);
    a.sse_part = cv.take<float>(n * cg_slots(chw));
    a.ssim_part = cv.take<float>(std::max<int64_t>(1, n * tile_count(c, h, w)));
    return cv.bytes();
}

bool metrics_shape_ok(int64_t c, int64_t h, int64_t w)
{
    return c >= 1 && h >= 1 && w >= 1 && h <= INT32_MAX / c && w <= INT32_MAX / (c * h) &&
           tile_count(c, h, w) <= INT32_MAX;
}

int64_t metrics_workspace_bytes(int64_t n, int64_t m, int64_t c, int64_t h, int64_t w)
{
    MetricsArgs a{};
    return metrics_layout(a, Carver(nullptr), n, m, c, h, w);
}

int image_metrics(const float *x, const float *label, int64_t m, float data_range, float *mse, float *psnr, float *ssim,
                  int64_t n, int64_t c, int64_t h, int64_t w, void *workspace, hipStream_t s)
{
    if (n == 0) return DPSX_OK;
    const int64_t chw = c * h * w;
    const bool want_sse = mse || psnr, want_range = !(data_range > 0.0f) && (psnr || ssim);
    const bool vec = vec_ok(chw, {x, label});
    MetricsArgs a{};
    metrics_layout(a, Carver(workspace), n, m, c, h, w);
    float *range_part = const_cast<float *>(a.range_part);       // written by the range launch, read by the others
    if (!want_range) a.range_part = nullptr;                     // a region that is not wanted is not launched on
    if (!want_sse) a.sse_part = nullptr;
    if (!ssim) a.ssim_part = nullptr;
    a.x = x;
    a.label = label;
    a.mse = mse;
    a.psnr = psnr;
    a.ssim = ssim;
    a.chw = chw;
    a.sse_slots = cg_slots(chw);
    a.per = pass_geom(chw, vec, n).per;
    a.c = (int)c;
    a.h = (int)h;
    a.w = (int)w;
    a.tiles_y = (int)tiles_of(h);
    a.tiles_x = (int)tiles_of(w);
    a.tiles = (int)tile_count(c, h, w);
    a.range_slots = range_slots(chw);
    a.div = row_div(m, n);
    a.data_range = data_range;
    double g[kWin], total = 0.0;                       // the window's taps in double, normalised to sum 1
    for (int k = 0; k < kWin; ++k) total += g[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < kWin; ++k) a.taps.g[k] = (float)(g[k] / total);

    if (want_range) {
        const int64_t per = (chw + a.range_slots - 1) / a.range_slots;
        k_label_range<<<dim3((unsigned)a.range_slots, (unsigned)m), kPassThreads, 0, s>>>(
            label, range_part, chw, per);
        int rc = check_launch();
        if (rc != DPSX_OK) return rc;
    }
    int rc = dispatch(vec, [&](auto V) {
        if (ssim) k_metrics_tile<V.value><<<dim3((unsigned)a.tiles, (unsigned)n), kPassThreads, 0, s>>>(a);
        else k_metrics_sse<V.value><<<dim3((unsigned)a.sse_slots, (unsigned)n), kPassThreads, 0, s>>>(a);
        return check_launch();
    });
    if (rc != DPSX_OK) return rc;
    k_metrics_finish<<<(unsigned)n, kWave, 0, s>>>(a);
    return check_launch();
}

}  // namespace dpsx
