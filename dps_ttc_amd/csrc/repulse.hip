// Kernel-weighted particle repulsion per image (include/dpsx.h: "particle repulsion"; Corso et al. 2023, particle guidance
// with a fixed RBF potential in x_t space), three launches, and the K x K squared-distance matrix of an image on its own
// (the first two).  The definition is stated in include/dpsx.h and restated in float64 in tests/repulse_ref.py.
//
//   k_repulse_pairs   grid (slots, tile pairs, images).  The K particles of an image are cut into tiles of kRepTile = 8;
//                     a block owns one tile pair (ta <= tb) and one contiguous element range of the image, lanes across
//                     elements (a float4 unit each, or an element: the scalar instantiation).  Per unit the lane loads the
//                     8 (ta == tb) or 16 particles' values, all loads before the first use, and adds into one fp32
//                     accumulator per pair of the tile pair: d = fsub(x_i, x_j), acc = fmaf(d, d, acc) -- the difference
//                     form; a unit's four elements in index order, the lane's units in index order.  At the end of the
//                     range every accumulator is summed over the block in a fixed tree (inside a wave lanes l and l ^ 32,
//                     then ^ 16, ... ^ 1; then the waves in index order) and
//                     the pairs i < j < K are written to part[image][slot][pair(i, j)].  A diagonal tile pair computes the
//                     pairs i < j only.  Rows of a ragged tile read particle K - 1 again (no read outside the image) and
//                     are not written.
//   k_repulse_finish  one block per image.  Per pair i < j: the slots added in double in index order, rounded to fp32
//                     once, written to d2[i][j] and d2[j][i] (the diagonal is +0.0).  The sum and the minimum of the
//                     pairs: every thread takes the pairs of the matrix entries t, t + 1024, ... in index order, then
//                     wave_sum_f64's tree and the waves in index order.  Thread 0 forms mean, h, gain and the flag in
//                     double; then all threads form w (exp in double, rounded once) into the launch's padded copy
//                     [K][Kp], Kp = K rounded up to 8, and into the caller's [K][K].
//   k_repulse_apply   grid (slots, tiles, images): a block owns 8 output particles and an element range, holds their
//                     values in registers, and streams j = 0 .. K - 1 in index order: acc_i = fmaf(w[j][i], fsub(x_i, x_j),
//                     acc_i), the eight weights of a j read from LDS as two 16-byte broadcasts (the tile's K x 8 weights are
//                     staged there once from the padded copy; w is symmetric bit for bit, so row j holds column j);
//                     out_i = fmaf(gain, acc_i, x_i).  j = i adds fmaf(0, 0, acc).
//                     An image whose flag is 0 is copied, no arithmetic.
//
// The slot count of the pair partials is rep_slots(D, K): a function of the particle size and the particles per image only,
// so an image's numbers do not depend on the images beside it.  Everything an image's blocks read is the image's own.
// A particle's bytes are fetched by every tile pair its tile belongs to, ceil(K / 8) + 1 times in the pair launch and
// ceil(K / 8) times in the apply launch; the blocks of one element range run side by side and share them through the cache.
#include "particle_pass.h"

#include <algorithm>
#include <cmath>

namespace dpsx {

namespace {

constexpr int kRepTile = 8;
constexpr int kRepBlocks = 2048;                 // the blocks per image a launch aims for when it picks its slot count
constexpr int kRepFinishThreads = 1024;

struct RepArgs {
    const float *x;
    float *out;
    float *part;                 // [images, slots, K (K - 1) / 2]
    float *d2;                   // [images, K, K]
    float *wpad;                 // [images, K, Kp] (null: the distance half only)
    float *w;                    // [images, K, K] the caller's (nullable)
    float *info;                 // [images, 4]
    uint8_t *applied;            // [images]
    int64_t chw, per, aper;      // per / aper: work items per block of the pair / apply launch
    int k, kp, nt, slots;
    float c, bandwidth;
};

__device__ __forceinline__ int rep_pair_index(int i, int j, int k) { return i * k - (i * (i + 1)) / 2 + (j - i - 1); }

// the accumulators of one tile pair over the block's range; DIAG: ta == tb, the pairs i < j only
template <bool VEC, bool DIAG>
__device__ __forceinline__ void rep_tile_pair(const float *__restrict__ img, int64_t chw, int k, int ia0, int ib0,
                                              const Range r, float (&acc)[kRepTile][kRepTile])
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    const float *pa[kRepTile], *pb[kRepTile];
#pragma unroll
    for (int t = 0; t < kRepTile; ++t) {
        pa[t] = img + (int64_t)min(ia0 + t, k - 1) * chw;
        pb[t] = img + (int64_t)min(ib0 + t, k - 1) * chw;
    }
    for (int64_t u = r.lo + threadIdx.x; u < r.hi; u += kPassThreads) {
        T av[kRepTile], bv[kRepTile];
#pragma unroll
        for (int t = 0; t < kRepTile; ++t) av[t] = ld<T>(pa[t] + u * W);
#pragma unroll
        for (int t = 0; t < kRepTile; ++t) bv[t] = DIAG ? av[t] : ld<T>(pb[t] + u * W);
#pragma unroll
        for (int i = 0; i < kRepTile; ++i)
#pragma unroll
            for (int j = DIAG ? i + 1 : 0; j < kRepTile; ++j)
#pragma unroll
                for (int l = 0; l < W; ++l) {
                    const float d = __fsub_rn(lane(av[i], l), lane(bv[j], l));
                    acc[i][j] = fmaf(d, d, acc[i][j]);
                }
    }
}

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_repulse_pairs(const RepArgs a)
{
    constexpr int W = Unit<VEC>::W;
    constexpr int kWaves = kPassThreads / kWave;
    __shared__ float red[kRepTile * kRepTile][kWaves];
    const int k = a.k;
    const int64_t m = blockIdx.z;
    int ta = 0, rem = blockIdx.y;                            // tile pair blockIdx.y of the upper triangle, row-major
    while (rem >= a.nt - ta) {
        rem -= a.nt - ta;
        ++ta;
    }
    const int tb = ta + rem, ia0 = ta * kRepTile, ib0 = tb * kRepTile;
    const float *img = a.x + m * k * a.chw;
    const Range r = block_range(a.chw / W, a.per);
    float acc[kRepTile][kRepTile];
#pragma unroll
    for (int i = 0; i < kRepTile; ++i)
#pragma unroll
        for (int j = 0; j < kRepTile; ++j) acc[i][j] = 0.0f;
    if (ta == tb) rep_tile_pair<VEC, true>(img, a.chw, k, ia0, ib0, r, acc);       // block-uniform
    else rep_tile_pair<VEC, false>(img, a.chw, k, ia0, ib0, r, acc);

    // The wave's 64 sums in 63 exchanges instead of 64 trees (a block of a small image has one unit per lane, and 64
    // wave_sums cost more than its loads and fmas): at the step with lane distance d = 32, 16, ... 1 a lane keeps the even
    // half of its values if its bit d is clear, else the odd half, and adds what its partner (lane ^ d) kept out of the
    // same half.  A fixed tree: lanes l and l ^ 32 first, then ^ 16, ... ^ 1.  After the last step lane l holds the wave's
    // sum of accumulator bitrev6(l).  Then the waves in index order, as block_sum adds them.
    const int ln = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    float v[kRepTile * kRepTile];
#pragma unroll
    for (int i = 0; i < kRepTile; ++i)
#pragma unroll
        for (int j = 0; j < kRepTile; ++j) v[i * kRepTile + j] = acc[i][j];
#pragma unroll
    for (int d = 32, cnt = 32; d > 0; d >>= 1, cnt >>= 1) {
        const bool odd = ln & d;
#pragma unroll
        for (int q = 0; q < cnt; ++q) {
            const float keep = odd ? v[2 * q + 1] : v[2 * q], send = odd ? v[2 * q] : v[2 * q + 1];
            v[q] = keep + __shfl_xor(send, d, kWave);
        }
    }
    red[__brev((unsigned)ln) >> 26][wv] = v[0];
    __syncthreads();
    if (threadIdx.x < kRepTile * kRepTile) {
        float t = 0.0f;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) t += red[threadIdx.x][q];
        const int i = ia0 + (int)threadIdx.x / kRepTile, j = ib0 + (int)threadIdx.x % kRepTile;
        if (i < j && j < k) {
            const int64_t npairs = (int64_t)k * (k - 1) / 2;
            a.part[(m * a.slots + blockIdx.x) * npairs + rep_pair_index(i, j, k)] = t;
        }
    }
}

__global__ __launch_bounds__(kRepFinishThreads) void k_repulse_finish(const RepArgs a)
{
    constexpr int kWaves = kRepFinishThreads / kWave;
    __shared__ double s_sum[kWaves];
    __shared__ float s_min[kWaves];
    __shared__ double s_h;
    __shared__ int s_ok;
    const int k = a.k, kk = k * k;
    const int64_t m = blockIdx.x, npairs = (int64_t)k * (k - 1) / 2;
    const float *part = a.part + m * a.slots * npairs;
    float *d2 = a.d2 + m * kk;

    double sum = 0.0;
    float mn = INFINITY;                                     // nan_min: a NaN distance shows in the record
    for (int idx = threadIdx.x; idx < kk; idx += kRepFinishThreads) {
        const int i = idx / k, j = idx - i * k;
        if (i == j) d2[idx] = 0.0f;
        if (i >= j) continue;
        const float *p = part + rep_pair_index(i, j, k);
        double acc = 0.0;
        for (int s0 = 0; s0 < a.slots; s0 += 16) {           // 16 loads in flight, added in index order (+0.0 past the end)
            float t[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) t[q] = s0 + q < a.slots ? p[(s0 + q) * npairs] : 0.0f;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc += (double)t[q];
        }
        const float v = (float)acc;
        d2[idx] = v;
        d2[j * k + i] = v;
        sum += (double)v;
        mn = nan_min(mn, v);
    }
    wave_sum_f64(sum);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mn = nan_min(mn, __shfl_down(mn, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_min[threadIdx.x >> 6] = mn;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int q = 0; q < kWaves; ++q) {
            total += s_sum[q];
            if (q) mn = nan_min(mn, s_min[q]);
        }
        const double mean = k > 1 ? total / (double)npairs : 0.0;
        const double h = a.bandwidth > 0.0f ? (double)a.bandwidth * (double)a.chw : mean / log((double)(k + 1));
        const float gain = (float)(2.0 * (double)a.c / h);
        const bool ok = k > 1 && isfinite(mean) && h > 0.0 && isfinite(h) && isfinite(gain);    // false for NaN
        float *info = a.info + m * 4;
        info[0] = (float)h;
        info[1] = ok ? gain : 0.0f;
        info[2] = (float)mean;
        info[3] = mn;
        if (a.applied) a.applied[m] = ok ? 1 : 0;
        s_h = h;
        s_ok = ok;
    }
    if (!a.wpad) return;                                     // launch-uniform: the distance half only
    __syncthreads();                                         // d2 of this block's other threads, h, the flag
    const double h = s_h;
    const bool ok = s_ok;
    float *wpad = a.wpad + m * k * a.kp, *w = a.w ? a.w + m * kk : nullptr;
    for (int idx = threadIdx.x; idx < k * a.kp; idx += kRepFinishThreads) {
        const int i = idx / a.kp, j = idx - i * a.kp;
        const float v = ok && j < k && i != j ? (float)exp(-(double)d2[i * k + j] / h) : 0.0f;
        wpad[idx] = v;
        if (w && j < k) w[i * k + j] = v;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_repulse_apply(const RepArgs a)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    const int k = a.k, i0 = blockIdx.y * kRepTile;
    const int64_t m = blockIdx.z;
    const float *__restrict__ img = a.x + m * k * a.chw;
    float *__restrict__ out = a.out + m * k * a.chw;
    const Range r = block_range(a.chw / W, a.aper);
    int64_t row[kRepTile];
#pragma unroll
    for (int t = 0; t < kRepTile; ++t) row[t] = (int64_t)min(i0 + t, k - 1) * a.chw;
    if (!a.applied[m]) {                                     // block-uniform: the image is copied
        for (int64_t u = r.lo + threadIdx.x; u < r.hi; u += kPassThreads)
#pragma unroll
            for (int t = 0; t < kRepTile; ++t)
                if (i0 + t < k) st<T>(out + row[t] + u * W, ld<T>(img + row[t] + u * W));
        return;
    }
    const float gain = a.info[m * 4 + 1];
    // the tile's weights, row j = w[j][i0 .. i0 + 7], staged once: every lane then reads the same 32 bytes per j (a broadcast)
    __shared__ __attribute__((aligned(16))) float s_w[kRepulseMaxK * kRepTile];
    const float *wcol = a.wpad + (m * k) * a.kp + i0;
    for (int idx = threadIdx.x; idx < k * kRepTile; idx += kPassThreads)
        s_w[idx] = wcol[(int64_t)(idx / kRepTile) * a.kp + idx % kRepTile];
    __syncthreads();
    for (int64_t u = r.lo + threadIdx.x; u < r.hi; u += kPassThreads) {
        T xi[kRepTile], acc[kRepTile];
#pragma unroll
        for (int t = 0; t < kRepTile; ++t) {
            xi[t] = ld<T>(img + row[t] + u * W);
            acc[t] = T{};
        }
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
            const T xj = ld<T>(img + (int64_t)j * a.chw + u * W);
            const float4 w0 = *reinterpret_cast<const float4 *>(s_w + j * kRepTile);
            const float4 w1 = *reinterpret_cast<const float4 *>(s_w + j * kRepTile + 4);
            const float wj[kRepTile] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
            for (int t = 0; t < kRepTile; ++t) {
                const float wt = wj[t];
#pragma unroll
                for (int l = 0; l < W; ++l)
                    set(acc[t], l, fmaf(wt, __fsub_rn(lane(xi[t], l), lane(xj, l)), lane(acc[t], l)));
            }
        }
#pragma unroll
        for (int t = 0; t < kRepTile; ++t) {
            if (i0 + t >= k) continue;
            T o;
#pragma unroll
            for (int l = 0; l < W; ++l) set(o, l, fmaf(gain, lane(acc[t], l), lane(xi[t], l)));
            st<T>(out + row[t] + u * W, o);
        }
    }
}

int rep_tiles(int64_t k) { return (int)std::max<int64_t>(1, (k + kRepTile - 1) / kRepTile); }
int rep_fill(int64_t chw, int64_t blocks_y)      // slots that bring a launch of blocks_y blocks per range to kRepBlocks
{
    return (int)std::min<int64_t>(cg_slots(chw), std::max<int64_t>(1, (kRepBlocks + blocks_y - 1) / blocks_y));
}
// the partial slots of a pair: a function of (D, K) only
int rep_slots(int64_t chw, int64_t k)
{
    const int64_t nt = rep_tiles(k);
    return rep_fill(chw, nt * (nt + 1) / 2);
}

// THE workspace layout: the pair partials, then what the launches need of d2, w (padded), info and applied when the
// caller keeps none; returns the bytes (the size query and the launch path both walk it)
int64_t rep_layout(RepArgs &a, Carver cv, int64_t segments, int64_t k, int64_t chw)
{
    const int64_t kp = rep_tiles(k) * kRepTile, npairs = k * (k - 1) / 2;
    a.part = cv.take<float>(std::max<int64_t>(1, segments * rep_slots(chw, k) * npairs));
    a.d2 = cv.take<float>(segments * k * k);
    a.wpad = cv.take<float>(segments * k * kp);
    a.info = cv.take<float>(segments * 4);
    a.applied = cv.take<uint8_t>(segments);
    return cv.bytes();
}

}  // namespace

int64_t repulse_workspace_bytes(int64_t n, int64_t chw, int64_t segments)
{
    RepArgs a{};
    return rep_layout(a, Carver(nullptr), segments, n / segments, chw);
}

int repulse(bool apply, float c, float bandwidth, const float *x, float *out, float *d2, float *w, float *info,
            uint8_t *applied, int64_t n, int64_t chw, int64_t segments, void *workspace, hipStream_t s)
{
    if (n == 0) return DPSX_OK;
    const int64_t k = n / segments;
    const int nt = rep_tiles(k);
    const bool vec = vec_ok(chw, {x, out});
    const int64_t units = vec ? chw / 4 : chw;
    RepArgs a{};
    rep_layout(a, Carver(workspace), segments, k, chw);
    a.x = x;
    a.out = out;
    if (d2) a.d2 = d2;                                       // the caller's buffers take the place of the workspace's
    if (!apply) a.wpad = nullptr;
    a.w = apply ? w : nullptr;
    if (info) a.info = info;
    if (applied) a.applied = applied;
    a.chw = chw;
    a.k = (int)k;
    a.kp = nt * kRepTile;
    a.nt = nt;
    a.slots = rep_slots(chw, k);
    a.per = (units + a.slots - 1) / a.slots;
    const int aslots = rep_fill(chw, nt);
    a.aper = (units + aslots - 1) / aslots;
    a.c = c;
    a.bandwidth = bandwidth;

    int rc = DPSX_OK;
    if (k > 1) {
        rc = dispatch(vec, [&](auto V) {
            k_repulse_pairs<V.value><<<dim3((unsigned)a.slots, (unsigned)(nt * (nt + 1) / 2), (unsigned)segments),
                                       kPassThreads, 0, s>>>(a);
            return check_launch();
        });
        if (rc != DPSX_OK) return rc;
    }
    k_repulse_finish<<<(unsigned)segments, kRepFinishThreads, 0, s>>>(a);
    rc = check_launch();
    if (rc != DPSX_OK || !apply) return rc;
    return dispatch(vec, [&](auto V) {
        k_repulse_apply<V.value><<<dim3((unsigned)aslots, (unsigned)nt, (unsigned)segments), kPassThreads, 0, s>>>(a);
        return check_launch();
    });
}

}  // namespace dpsx
