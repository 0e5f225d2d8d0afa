// Order statistics of every image's K particles (include/dpsx.h: "order statistics"): per-element quantiles, the rank
// histogram of the label among the particles and the CRPS, two launches:
//
//   element pass   grid (quant_slots(d, K), M).  A lane owns one element and holds the element's K values as integer keys
//                  (k = s ^ ((s >> 31) & 0x7fffffff) on the bit pattern s: signed comparison of the keys is the order of
//                  the definition, -0.0 before +0.0, and the map is its own inverse); a wave reads 256 contiguous bytes of
//                  each particle row with last-use loads, every byte once, the loads of a batch issued before the first
//                  use.  The sorted column gives the q quantiles, the label's rank (strict IEEE comparison on the values)
//                  and the two CRPS sums in one sweep.  Two routes, chosen by K alone:
//     register     K <= kQuantRegK = 64: tiles of 256 elements, K padded to Kp in {2, 4, 8, 16, 32, 64} with keys above
//                  +Inf; a fully unrolled bitonic network of v_min_i32 / v_max_i32 on Kp VGPRs, every index a compile-time
//                  constant (k_quant_reg<Kp>; no scratch: profiles/quantile_kernel_stats.txt).
//     LDS          64 < K <= 512: tiles of 64 elements, K padded to Kp in {128, 256, 512}; the tile's columns live in
//                  dynamic LDS column-major (value k of element l at k * 64 + l: a wave's access touches 64 consecutive
//                  dwords), 256 Kp bytes: 32 / 64 / 128 KiB, so 4 / 2 / 1 blocks share a CU.  A block is four waves, one per
//                  SIMD, that share the tile's work: lane l of every wave works on element l.  Runs of 64 are sorted in
//                  registers by the same network on their way into LDS, a run per wave at a time (odd runs descending:
//                  their keys are complemented around the network); each bitonic merge of 128, 256 and 512 then takes its
//                  strides >= 64 on the 2 / 4 / 8 values that lie 64 apart and its strides 32 .. 1 run by run, both in
//                  registers, with a barrier between the passes.  From the sorted column wave 0 takes sum |x_(i) - y| and
//                  the rank, wave 2 the other CRPS sum (each in sorted order) and wave 1 the quantiles.  (One wave per
//                  block, which needs no barrier, ran K = 512 at 3.4 ms per 3 x 256^2 image against 0.73: one SIMD of four.)
//                  Per block: the histogram's counts in LDS (integer atomics: exact in any order), the lanes' CRPS and
//                  width sums through block_sum; one row of K + 3 counts and two fp32 partials per block.  No memset: every
//                  slot is written by every call.
//   k_quant_finish one wave per (image, kQuantCols histogram columns): a column's slots are added as integers; the last
//                  wave of an image also adds the CRPS and width slots in double in slots_sum's order, divides once and
//                  writes info.
//
// No global atomics, no fence, no host read; a block reads its image only and a lane its element only, so a NaN stays in
// its element of its image.  x is read with scalar dword loads: its alignment does not matter.
#include "particle_pass.h"

#include <climits>
#include <cmath>

namespace dpsx {

constexpr int kQuantThreads = 256;    // register route: elements per tile = lanes per block
constexpr int kQuantCols = 16;        // histogram columns per finisher wave
constexpr int kQuantMaxSlots = 1024;  // blocks per image
constexpr int kQuantPad = INT_MAX;    // the padding key: above +Inf's (0x7f800000)

struct QuantArgs {
    const float *x, *y;           // y null: no rank, no CRPS
    float *quant;                 // [M, q, d]
    int *ipart;                   // [M, slots, K + 3]: the bins 0 .. K + 1, then the elements of finite width
    float *cpart, *wpart;         // [M, slots] each: CRPS and width partials
    int32_t *hist;                // [M, K + 2] nullable
    float *info;                  // [M, 4]
    int64_t d, tiles;
    int per;                      // tiles per block
    int k, kp, q, slots;
    int lo[kQuantMaxQ];           // floor(p (K - 1))
    double f[kQuantMaxQ];         // p (K - 1) - lo
};

__device__ __forceinline__ int quant_key(float v)
{
    const int s = __float_as_int(v);
    return s ^ ((s >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float quant_val(int key) { return __int_as_float(key ^ ((key >> 31) & 0x7fffffff)); }

// a last-use load at a wave-uniform base plus the lane's byte offset: the scalar-base form of the global load (one VGPR of
// address per lane for all rows in flight; the compiler still falls back to a VGPR pair per row where it runs out of
// scalar registers, as in k_quant_reg<64>).  The base is made a scalar explicitly and the pointer is rebuilt in the global
// address space: left to itself the compiler re-associates base + offset into one 64-bit VGPR address per row.
__device__ __forceinline__ float quant_ld(const float *&base, unsigned byte_off)
{
    typedef const char __attribute__((address_space(1))) *gchar;
    typedef const float __attribute__((address_space(1))) *gfloat;
    const uint64_t u = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)u), hi = __builtin_amdgcn_readfirstlane((uint32_t)(u >> 32));
    const uint64_t uni = ((uint64_t)hi << 32) | lo;
    base = reinterpret_cast<const float *>(uni);
    return __builtin_nontemporal_load((gfloat)((gchar)uni + byte_off));
}

__device__ __forceinline__ void quant_cex(int &lo, int &hi)
{
    const int a = min(lo, hi), b = max(lo, hi);
    lo = a;
    hi = b;
}

// the bitonic network's stages for the sizes FIRST, 2 FIRST, .. KP on v[0 .. KP): FIRST == 2 sorts, FIRST == KP merges
// two runs of KP / 2 (the first ascending, the second descending).  Ascending result; every index is a constant.
template <int KP, int FIRST> __device__ __forceinline__ void quant_network(int (&v)[KP])
{
#pragma unroll
    for (int size = FIRST; size <= KP; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const int p = i ^ stride;
                if (p > i) {
                    if ((i & size) == 0 || size == KP) quant_cex(v[i], v[p]);
                    else quant_cex(v[p], v[i]);
                }
            }
        }
    }
}

// v[idx] for a launch-uniform idx without a run-time register index: a binary tree of KP - 1 selects on idx's bits
template <int KP> __device__ __forceinline__ int quant_pick(const int (&v)[KP], int idx)
{
    if constexpr (KP == 1) {
        return v[0];
    } else {
        // (a bitwise select: written as `odd ? v[2 i + 1] : v[2 i]` the compiler turns the pair of reads into one read at a
        // run-time index, which sends the array to scratch memory)
        int t[KP / 2];
        const int odd = -(idx & 1);
#pragma unroll
        for (int i = 0; i < KP / 2; ++i) t[i] = (v[2 * i + 1] & odd) | (v[2 * i] & ~odd);
        return quant_pick<KP / 2>(t, idx >> 1);
    }
}

// what the sweep over the sorted column leaves
struct QuantSweep {
    double s1 = 0.0, s2 = 0.0;    // sum |x_(i) - y|, sum (2 i - K + 1) x_(i), in sorted order
    int rank = 0;                 // #{x_j < y}
};
__device__ __forceinline__ void quant_sweep_s1(QuantSweep &w, float x, float y)
{
    w.s1 = __dadd_rn(w.s1, fabs(__dsub_rn((double)x, (double)y)));
    w.rank += x < y;
}
__device__ __forceinline__ void quant_sweep_s2(QuantSweep &w, int i, float x, int k)
{
    // (the coefficient passes through an empty asm: as a plain expression of K its double form is loop-invariant, and the
    // unrolled register route keeps all Kp of them in VGPR pairs across its tile loop)
    int coef = 2 * i - k + 1;
    asm volatile("" : "+s"(coef));
    w.s2 = __dadd_rn(w.s2, __dmul_rn((double)coef, (double)x));
}
__device__ __forceinline__ void quant_sweep(QuantSweep &w, int i, float x, float y, int k)
{
    quant_sweep_s1(w, x, y);
    quant_sweep_s2(w, i, x, k);
}

// one quantile from its two neighbours
__device__ __forceinline__ float quant_lerp(float a, float b, double f)
{
    if (f == 0.0 || a == b) return a;
    const float r = (float)__dadd_rn((double)a, __dmul_rn(f, __dsub_rn((double)b, (double)a)));
    return r != r ? __int_as_float(0x7fc00000) : r;
}

// the q positions in LDS, so that the loop over them stays rolled and reads them at a run-time index
struct QuantPos {
    double f[kQuantMaxQ];
    int lo[kQuantMaxQ];
};
__device__ __forceinline__ void quant_pos_init(const QuantArgs &a, QuantPos &s_pos)
{
#pragma unroll
    for (int i = 0; i < kQuantMaxQ; ++i) {
        if (threadIdx.x == i) {
            s_pos.f[i] = a.f[i];
            s_pos.lo[i] = a.lo[i];
        }
    }
}

// the element's outputs from its sorted column (pick(i): the value at sorted position i, i wave-uniform) and the sweep: the
// quantile stores, the histogram's bin, and the lane's CRPS / width sums (quantiles / ranks: the halves a wave takes, both
// on the register route).  The loop over the positions is kept rolled: unrolled, the register route's pick trees of all
// positions are scheduled side by side (8 Kp VGPRs of temporaries).
template <class Pick>
__device__ __forceinline__ void quant_emit(const QuantArgs &a, const QuantPos &s_pos, int64_t m, int64_t e, bool on, bool nan,
                                           float yv, Pick &&pick, const QuantSweep &w, int *s_hist, float &csum, float &wsum,
                                           bool quantiles = true, bool ranks = true)
{
    const int k = a.k;
    float first = 0.0f, last = 0.0f;
#pragma unroll 1
    for (int i = 0; i < (quantiles ? a.q : 0); ++i) {
        const int lo = __builtin_amdgcn_readfirstlane(s_pos.lo[i]);
        const float qa = pick(lo), qb = pick(min(lo + 1, k - 1));
        const float r = nan ? __int_as_float(0x7fc00000) : quant_lerp(qa, qb, s_pos.f[i]);
        if (i == 0) first = r;
        last = r;
        if (on) a.quant[(m * a.q + i) * a.d + e] = r;
    }
    if (!on) return;
    const float width = __fsub_rn(last, first);
    if (quantiles && __builtin_isfinite(width)) {
        wsum = __fadd_rn(wsum, width);
        atomicAdd(&s_hist[k + 2], 1);
    }
    if (!a.y || !ranks) return;                              // wave-uniform
    const bool invalid = nan || yv != yv;
    atomicAdd(&s_hist[invalid ? k + 1 : w.rank], 1);
    if (!invalid) {
        const double kd = (double)k;
        const double crps = __dsub_rn(w.s1 / kd, w.s2 / __dmul_rn(kd, kd));
        csum = __fadd_rn(csum, (float)crps);
    }
}

__device__ __forceinline__ void quant_block_end(const QuantArgs &a, int64_t m, const int *s_hist, float csum, float wsum,
                                                float *red)
{
    const int cols = a.k + 3;
    const int64_t slot = m * a.slots + blockIdx.x;
    __syncthreads();
    for (int j = threadIdx.x; j < cols; j += blockDim.x) a.ipart[slot * cols + j] = s_hist[j];
    const float cs = block_sum(csum, red);
    if (threadIdx.x == 0) a.cpart[slot] = cs;
    const float ws = block_sum(wsum, red);
    if (threadIdx.x == 0) a.wpart[slot] = ws;
}

// ------------------------------------------------------------------ the register route
template <int KP>
__global__ __launch_bounds__(kQuantThreads) void k_quant_reg(const QuantArgs a)
{
    extern __shared__ int s_dyn[];                           // [K + 3] the block's counts
    __shared__ float red[kQuantThreads / kWave];
    __shared__ QuantPos s_pos;
    int *s_hist = s_dyn;
    quant_pos_init(a, s_pos);
    const int64_t m = blockIdx.y;
    const int k = a.k;
    for (int j = threadIdx.x; j < k + 3; j += kQuantThreads) s_hist[j] = 0;
    __syncthreads();
    const float *xi = a.x + m * k * a.d;
    float csum = 0.0f, wsum = 0.0f;
    const int64_t t0 = (int64_t)blockIdx.x * a.per, t1 = min(a.tiles, t0 + a.per);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t e = t * kQuantThreads + threadIdx.x;
        const bool on = e < a.d;                             // a lane past the end sorts padding and stores nothing
        // a row's address is a wave-uniform base plus the lane's 32-bit offset; a lane past the end reads element d - 1
        // (the row pointer steps from row to row and stops at row K - 1, which the padding positions re-read)
        const float *row = xi + t * kQuantThreads;
        const unsigned off = (unsigned)(min(e, a.d - 1) - t * kQuantThreads) * 4u;
        float raw[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            raw[j] = quant_ld(row, off);
            row += j + 1 < k ? a.d : 0;
        }
        const float *yrow = a.y + m * a.d + t * kQuantThreads;
        const float yv = a.y ? quant_ld(yrow, off) : 0.0f;
        int v[KP];
        bool nan = false;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            nan |= raw[j] != raw[j];
            v[j] = j < k ? quant_key(raw[j]) : kQuantPad;    // launch-uniform
        }
        quant_network<KP, 2>(v);

        QuantSweep w;
        if (a.y) {                                           // launch-uniform
#pragma unroll
            for (int j = 0; j < KP; ++j)
                if (j < k) quant_sweep(w, j, quant_val(v[j]), yv, k);
        }
        quant_emit(a, s_pos, m, e, on, nan, yv, [&](int i) { return quant_val(quant_pick<KP>(v, i)); }, w, s_hist, csum, wsum);
    }
    quant_block_end(a, m, s_hist, csum, wsum, red);
}

// ------------------------------------------------------------------ the LDS route
constexpr int kQuantRun = 64;         // a run: what the register network sorts at once
constexpr int kQuantLdsWaves = 4;     // the waves that share a tile's work, one per SIMD

// one pass of a merge's strides >= 64: the G = size / 64 values of a lane that lie 64 apart merge in registers
template <int G> __device__ __forceinline__ void quant_merge_far(int *col, int size, int kp, int wave)
{
    for (int it = wave; it < kp / G; it += kQuantLdsWaves) {
        const int base = (it / kQuantRun) * size + (it % kQuantRun), flip = (base & size) != 0 && size != kp ? -1 : 0;
        int v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = col[(base + g * kQuantRun) * kWave] ^ flip;
        quant_network<G, G>(v);
#pragma unroll
        for (int g = 0; g < G; ++g) col[(base + g * kQuantRun) * kWave] = v[g] ^ flip;
    }
}

__global__ __launch_bounds__(kQuantLdsWaves * kWave) void k_quant_lds(const QuantArgs a)
{
    extern __shared__ int s_dyn[];                           // [Kp, 64] the tile's columns, then [K + 3] the block's counts
    __shared__ float red[kQuantLdsWaves];
    __shared__ double s_s2[kWave];                           // wave 2's sum on its way to wave 0
    __shared__ QuantPos s_pos;
    quant_pos_init(a, s_pos);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int *col = s_dyn + lane;                                 // value i of this lane's element: col[i * kWave]
    int *s_hist = s_dyn + a.kp * kWave;
    const int64_t m = blockIdx.y;
    const int k = a.k, kp = a.kp, runs = kp / kQuantRun;
    for (int j = threadIdx.x; j < k + 3; j += blockDim.x) s_hist[j] = 0;
    const float *xi = a.x + m * k * a.d;
    float csum = 0.0f, wsum = 0.0f;
    const int64_t t0 = (int64_t)blockIdx.x * a.per, t1 = min(a.tiles, t0 + a.per);
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t e = t * kWave + lane;
        const bool on = e < a.d;
        const unsigned off = (unsigned)(min(e, a.d - 1) - t * kWave) * 4u;       // a lane past the end reads element d - 1
        __syncthreads();                                     // the previous tile's readers are done (first tile: the counts are zero)
        // runs of 64 sorted in registers, even runs ascending and odd ones descending (the network's size-64 stage)
        for (int c = wave; c < runs; c += kQuantLdsWaves) {
            const int j0 = c * kQuantRun, flip = c & 1 ? -1 : 0;
            if (j0 >= k) {                                   // a run of padding, already in order
                for (int j = 0; j < kQuantRun; ++j) col[(j0 + j) * kWave] = kQuantPad;
                continue;
            }
            const float *row = xi + t * kWave + (int64_t)j0 * a.d;                   // stops at row K - 1
            int v[kQuantRun];
#pragma unroll
            for (int j = 0; j < kQuantRun; ++j) {
                v[j] = __float_as_int(quant_ld(row, off));
                row += j0 + j + 1 < k ? a.d : 0;
            }
#pragma unroll
            for (int j = 0; j < kQuantRun; ++j) v[j] = (j0 + j < k ? quant_key(__int_as_float(v[j])) : kQuantPad) ^ flip;
            quant_network<kQuantRun, 2>(v);
#pragma unroll
            for (int j = 0; j < kQuantRun; ++j) col[(j0 + j) * kWave] = v[j] ^ flip;
        }
        // the merges of 128, 256, 512: strides >= 64 on the values 64 apart, strides 32 .. 1 run by run, both in registers
        for (int size = 2 * kQuantRun; size <= kp; size <<= 1) {
            __syncthreads();
            if (size == 2 * kQuantRun) quant_merge_far<2>(col, size, kp, wave);
            else if (size == 4 * kQuantRun) quant_merge_far<4>(col, size, kp, wave);
            else quant_merge_far<8>(col, size, kp, wave);
            __syncthreads();
            for (int c = wave; c < runs; c += kQuantLdsWaves) {
                const int j0 = c * kQuantRun, flip = (j0 & size) != 0 && size != kp ? -1 : 0;
                int v[kQuantRun];
#pragma unroll
                for (int j = 0; j < kQuantRun; ++j) v[j] = col[(j0 + j) * kWave] ^ flip;
                quant_network<kQuantRun, kQuantRun>(v);
#pragma unroll
                for (int j = 0; j < kQuantRun; ++j) col[(j0 + j) * kWave] = v[j] ^ flip;
            }
        }
        __syncthreads();
        // the sorted column: wave 0 takes the first CRPS sum and the rank, wave 2 the second sum (each in sorted order),
        // wave 1 the quantiles and the width; then wave 0 the bins and the CRPS
        // a NaN sorts to an end: below -Inf's key with the sign bit set, above +Inf's without (the padding lies behind K - 1)
        const bool nan = col[0] < (int)0x807fffff || col[(k - 1) * kWave] > 0x7f800000;
        float yv = 0.0f;
        QuantSweep w;
        if (a.y && (wave == 0 || wave == 2)) {
            const float *yrow = a.y + m * a.d + t * kWave;
            yv = quant_ld(yrow, off);
            if (wave == 0) {
                for (int j = 0; j < k; ++j) quant_sweep_s1(w, quant_val(col[j * kWave]), yv);
            } else {
                for (int j = 0; j < k; ++j) quant_sweep_s2(w, j, quant_val(col[j * kWave]), k);
                s_s2[lane] = w.s2;
            }
        }
        if (wave == 1)
            quant_emit(a, s_pos, m, e, on, nan, yv, [&](int i) { return quant_val(col[i * kWave]); }, w, s_hist, csum, wsum, true, false);
        __syncthreads();
        if (wave == 0) {
            w.s2 = s_s2[lane];
            quant_emit(a, s_pos, m, e, on, nan, yv, [&](int i) { return quant_val(col[i * kWave]); }, w, s_hist, csum, wsum, false, true);
        }
    }
    quant_block_end(a, m, s_hist, csum, wsum, red);
}

// ------------------------------------------------------------------ the finisher
__device__ __forceinline__ int quant_colsum(const QuantArgs &a, int64_t m, int col)       // valid in lane 0
{
    const int cols = a.k + 3;
    int acc = 0;
    for (int i = threadIdx.x; i < a.slots; i += kWave) acc += a.ipart[(m * a.slots + i) * cols + col];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, kWave);
    return acc;
}

__global__ __launch_bounds__(kWave) void k_quant_finish(const QuantArgs a)
{
    const int64_t m = blockIdx.y;
    const int k = a.k;
    if (a.hist) {                                            // launch-uniform
        const int lo = blockIdx.x * kQuantCols, hi = min(k + 2, lo + kQuantCols);
        for (int col = lo; col < hi; ++col) {
            const int s = quant_colsum(a, m, col);
            if (threadIdx.x == 0) a.hist[m * (k + 2) + col] = s;
        }
    }
    if (blockIdx.x != gridDim.x - 1) return;                 // the image's last wave writes info
    const int invalid = quant_colsum(a, m, k + 1), finite = quant_colsum(a, m, k + 2);
    const double cs = slots_sum(a.cpart + m * a.slots, a.slots), ws = slots_sum(a.wpart + m * a.slots, a.slots);
    if (threadIdx.x != 0) return;
    float *o = a.info + m * 4;
    o[0] = a.y ? (float)(cs / (double)(a.d - invalid)) : NAN;
    o[1] = (float)(ws / (double)finite);
    o[2] = a.y ? (float)invalid : 0.0f;
    o[3] = (float)k;
}

// ------------------------------------------------------------------ host side
static int quant_tile(int64_t k) { return k <= kQuantRegK ? kQuantThreads : kWave; }
static int64_t quant_tiles(int64_t d, int64_t k) { return (d + quant_tile(k) - 1) / quant_tile(k); }
// blocks per image: a function of (d, K) only
static int quant_slots(int64_t d, int64_t k) { return (int)std::min<int64_t>(kQuantMaxSlots, quant_tiles(d, k)); }
static int quant_pad(int64_t k)
{
    int kp = 2;
    while (kp < k) kp <<= 1;
    return kp;
}

// THE workspace layout: the three partial arrays of the sort launch; returns the bytes (the size query and the launch path
// both walk it)
static int64_t quant_layout(QuantArgs &a, Carver cv, int64_t n, int64_t d, int64_t images)
{
    const int64_t k = n / images, slots = quant_slots(d, k);
    a.ipart = cv.take<int>(images * slots * (k + 3));
    a.cpart = cv.take<float>(images * slots);
    a.wpart = cv.take<float>(images * slots);
    return cv.bytes();
}

int64_t quantiles_workspace_bytes(int64_t n, int64_t d, int64_t images)
{
    QuantArgs a{};
    return quant_layout(a, Carver(nullptr), n, d, images);
}

template <int KP> static int quant_launch_reg(const QuantArgs &a, dim3 grid, hipStream_t s)
{
    k_quant_reg<KP><<<grid, kQuantThreads, (size_t)(a.k + 3) * sizeof(int), s>>>(a);
    return check_launch();
}

int quantiles(const float *x, const float *y, const double *probs, int64_t q, float *quant, int32_t *hist, float *info,
              int64_t n, int64_t d, int64_t images, void *workspace, hipStream_t s)
{
    const int64_t k = n / images;
    QuantArgs a{};
    quant_layout(a, Carver(workspace), n, d, images);
    a.x = x;
    a.y = y;
    a.quant = quant;
    a.hist = hist;
    a.info = info;
    a.d = d;
    a.tiles = quant_tiles(d, k);
    a.slots = quant_slots(d, k);
    a.per = (int)((a.tiles + a.slots - 1) / a.slots);
    a.k = (int)k;
    a.kp = quant_pad(k);
    a.q = (int)q;
    for (int64_t i = 0; i < q; ++i) {                        // the positions, once, in double
        const double h = probs[i] * (double)(k - 1), lo = std::floor(h);
        a.lo[i] = (int)lo;
        a.f[i] = h - lo;
    }
    const dim3 grid((unsigned)a.slots, (unsigned)images);
    int rc;
    if (k <= kQuantRegK) {
        switch (a.kp) {
        case 2: rc = quant_launch_reg<2>(a, grid, s); break;
        case 4: rc = quant_launch_reg<4>(a, grid, s); break;
        case 8: rc = quant_launch_reg<8>(a, grid, s); break;
        case 16: rc = quant_launch_reg<16>(a, grid, s); break;
        case 32: rc = quant_launch_reg<32>(a, grid, s); break;
        default: rc = quant_launch_reg<64>(a, grid, s); break;
        }
    } else {
        const size_t lds = ((size_t)a.kp * kWave + (size_t)(k + 3)) * sizeof(int);
        rc = launch_lds<k_quant_lds>(grid, kQuantLdsWaves * kWave, lds, s, a);
    }
    if (rc != DPSX_OK) return rc;
    const unsigned blocks = (unsigned)((k + 2 + kQuantCols - 1) / kQuantCols);
    k_quant_finish<<<dim3(blocks, (unsigned)images), kWave, 0, s>>>(a);
    return check_launch();
}

}  // namespace dpsx
