// Principal components of every image's particles (include/dpsx.h: "principal components"): the top q eigenpairs of the
// K x K centred Gram matrix and their directions in image space, four launches.  The definition is stated in
// include/dpsx.h and restated in float64 in tests/pca_ref.py.
//
//   repulse(false, ...)  the two distance launches of repulse.hip as they are: d2 [M, K, K] in the difference form.
//   k_pca_eig<KP>        one workgroup of 8 KP threads per image, KP = 32 / 64 / 128 >= K.  G and Vt (V transposed) live in
//                        LDS in fp32, both with a row pitch of KP + 1 words.  Prologue: d2 -> LDS, the row means and the
//                        mean in double in index order, G in place (entry (i, j) is formed from (min, max), so G is
//                        symmetric bit for bit), the trace, the degenerate cases (block-uniform exits).  Then the cyclic
//                        Jacobi method in the round-robin order: ne = K rounded up to even players, ne - 1 rounds per sweep;
//                        round r pairs player r with player ne - 1 and player (r + t) mod (ne - 1) with (r - t) mod (ne - 1),
//                        t = 1 .. ne / 2 - 1; the pair that holds player K of an odd K sits the round out.  Per round:
//                        thread t forms pair t's rotation from (g_pp, g_qq, g_pq) | barrier | rows p, q of G and of Vt are
//                        rotated (lanes across the columns) | barrier | columns p, q of G are rotated (lanes across the
//                        rows), g_pq and g_qp are set to 0 | barrier.  The pairs of a round are disjoint, so every word has
//                        one writer per phase and the result depends on K and G only.  After every sweep the off-diagonal
//                        and the total sum of squares are added in double in a fixed order; the sweeps end when
//                        off <= K 2^-46 total or at kPcaMaxSweeps.  Epilogue: every eigenvalue's place in the
//                        descending order (ties: the lower index first), the null rule, the selected eigenvectors centred and
//                        renormalised, the sign rule, evals / coords / info.
//   k_pca_project        grid (cg_slots(d), M), lanes across elements (float4 units or elements, as particle_pass.h's users).
//                        The image's coords, padded to 8 columns with zeros, and 1 / lambda_j sit in LDS; the K particles are
//                        streamed once, acc_j = fma(c_ij, x_i - x_0, acc_j) for all 8 columns, dirs_j = acc_j (1 / lambda_j).
//
// Bank conflicts: the row phase reads consecutive words of a row, the column phase walks a column with a stride of the
// pitch; KP + 1 is odd, so the 32 lanes of a half wave fall on 32 banks in both.  V is held transposed: its update is the
// row phase's access pattern and shares that phase's pair loop.
#include "particle_pass.h"

#include <algorithm>
#include <cmath>

namespace dpsx {

namespace {

constexpr int kPcaMaxSweeps = 24;
constexpr int kPcaPairs = kPcaMaxK / 2;
constexpr int kPcaCols = kPcaMaxQ;                // the projection's accumulators per element: q padded with zero columns
constexpr unsigned kPcaNaN = 0x7fc00000u;

struct PcaArgs {
    const float *x;
    const float *d2;             // [images, K, K]
    float *dirs, *evals, *coords, *info;
    int64_t d, per;              // per: work items per block of the projection
    int k, q;
};

__device__ __forceinline__ float pca_nan() { return __uint_as_float(kPcaNaN); }

// every output of a degenerate image but dirs (the projection writes those from evals): v everywhere, (trace, rank, 0, K)
__device__ __forceinline__ void pca_fill(const PcaArgs &a, int64_t m, float v, float rank)
{
    const int k = a.k, q = a.q;
    for (int idx = threadIdx.x; idx < k * q; idx += blockDim.x) a.coords[m * k * q + idx] = v;
    if ((int)threadIdx.x < q) a.evals[m * q + threadIdx.x] = v;
    if (threadIdx.x == 0) {
        float *o = a.info + m * 4;
        o[0] = v;
        o[1] = rank;
        o[2] = 0.0f;
        o[3] = (float)k;
    }
}

template <int KP>
__global__ __launch_bounds__(KP * 8) void k_pca_eig(const PcaArgs a)
{
    constexpr int T = KP * 8, P = KP + 1, kWaves = T / kWave, kGroups = T / KP;
    extern __shared__ float s_mat[];
    float *G = s_mat, *Vt = s_mat + KP * P;
    __shared__ double s_r[KP];                   // the row means of d2
    __shared__ double s_red[2][kWaves];
    __shared__ double s_t, s_trace;
    __shared__ float s_c[kPcaPairs], s_s[kPcaPairs];
    __shared__ int s_p[kPcaPairs], s_q[kPcaPairs];
    __shared__ int s_sel[kPcaCols];              // the column of V in place j of the order
    __shared__ float s_lam[kPcaCols], s_sgn[kPcaCols];
    __shared__ float s_lam0;

    const int k = a.k, q = a.q, tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    if (k == 1) {                                // launch-uniform
        pca_fill(a, m, 0.0f, 0.0f);
        return;
    }
    if (tid < kPcaCols) s_sel[tid] = 0;          // places past K are never selected
    const int lane_j = tid % KP, grp = tid / KP;

    // ---- prologue: d2 -> G in place, Vt = I
    const float *d2 = a.d2 + m * k * k;
    for (int i = grp; i < k; i += kGroups)
        if (lane_j < k) {
            G[i * P + lane_j] = d2[i * k + lane_j];
            Vt[i * P + lane_j] = i == lane_j ? 1.0f : 0.0f;
        }
    __syncthreads();
    if (tid < k) {
        double acc = 0.0;
        for (int j = 0; j < k; ++j) acc += (double)G[tid * P + j];
        s_r[tid] = acc / (double)k;
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < k; ++i) acc += s_r[i];
        s_t = acc / (double)k;
    }
    __syncthreads();
    const double t = s_t;
    if (t == 0.0) {                              // block-uniform: all particles equal
        pca_fill(a, m, 0.0f, 0.0f);
        return;
    }
    if (!isfinite(t)) {                          // block-uniform: a NaN or Inf in the image
        pca_fill(a, m, pca_nan(), -1.0f);
        return;
    }
    for (int i = grp; i < k; i += kGroups)
        if (lane_j < k) {
            const int lo = min(i, lane_j), hi = max(i, lane_j);
            G[i * P + lane_j] = (float)(-0.5 * ((((double)G[i * P + lane_j] - s_r[lo]) - s_r[hi]) + t));
        }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < k; ++i) acc += (double)G[i * P + i];
        s_trace = acc;
    }

    // ---- the sweeps
    const int ne = k + (k & 1), np = ne / 2, nr = ne - 1;
    const double tol2 = (double)k * 0x1p-46;     // (sqrt(K) 2^-23)^2
    int sweeps = 0;
    bool converged;
    for (;;) {
        double off = 0.0, dg = 0.0;
        for (int i = grp; i < k; i += kGroups)
            if (lane_j < k) {
                const double v = (double)G[i * P + lane_j];
                if (i == lane_j) dg += v * v;
                else off += v * v;
            }
        wave_sum_f64(off);
        wave_sum_f64(dg);
        __syncthreads();                         // the previous measure's readers are done with s_red
        if ((tid & (kWave - 1)) == 0) {
            s_red[0][tid >> 6] = off;
            s_red[1][tid >> 6] = dg;
        }
        __syncthreads();
        off = 0.0;
        dg = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            off += s_red[0][w];
            dg += s_red[1][w];
        }
        converged = off <= tol2 * (off + dg);    // block-uniform: every thread adds the same words in the same order
        if (converged || sweeps == kPcaMaxSweeps) break;

        for (int r = 0; r < nr; ++r) {
            if (tid < np) {
                int p = tid == 0 ? r : (r + tid) % nr, qq = tid == 0 ? ne - 1 : (r + nr - tid) % nr;
                if (p > qq) {
                    const int sw = p;
                    p = qq;
                    qq = sw;
                }
                float c = 1.0f, s = 0.0f;
                if (qq < k) {                    // else: the bye of an odd K
                    const float gpq = G[p * P + qq], gpp = G[p * P + p], gqq = G[qq * P + qq];
                    if (fabsf(gpq) > 0x1p-24f * sqrtf(fabsf(gpp * gqq))) {
                        const float th = (gqq - gpp) / (2.0f * gpq);
                        const float tn = copysignf(1.0f, th) / (fabsf(th) + sqrtf(fmaf(th, th, 1.0f)));
                        c = 1.0f / sqrtf(fmaf(tn, tn, 1.0f));
                        s = tn * c;
                    }
                }
                s_p[tid] = p;
                s_q[tid] = qq;
                s_c[tid] = c;
                s_s[tid] = s;
            }
            __syncthreads();
            for (int pr = grp; pr < np; pr += kGroups) {         // rows p, q of G and of Vt
                const float s = s_s[pr];
                if (s == 0.0f || lane_j >= k) continue;
                const float c = s_c[pr];
                const int p = s_p[pr] * P + lane_j, qq = s_q[pr] * P + lane_j;
                const float gp = G[p], gq = G[qq], vp = Vt[p], vq = Vt[qq];
                G[p] = fmaf(-s, gq, c * gp);
                G[qq] = fmaf(s, gp, c * gq);
                Vt[p] = fmaf(-s, vq, c * vp);
                Vt[qq] = fmaf(s, vp, c * vq);
            }
            __syncthreads();
            for (int pr = grp; pr < np; pr += kGroups) {         // columns p, q of G; lane_j is the row
                const float s = s_s[pr];
                if (s == 0.0f || lane_j >= k) continue;
                const float c = s_c[pr];
                const int p = s_p[pr], qq = s_q[pr];
                const float gp = G[lane_j * P + p], gq = G[lane_j * P + qq];
                G[lane_j * P + p] = lane_j == qq ? 0.0f : fmaf(-s, gq, c * gp);
                G[lane_j * P + qq] = lane_j == p ? 0.0f : fmaf(s, gp, c * gq);
            }
            __syncthreads();
        }
        ++sweeps;
    }

    // ---- epilogue: the order, the null rule, the sign rule
    if (tid < k) {
        const float li = G[tid * P + tid];
        int pos = 0;
        for (int j = 0; j < k; ++j) {
            const float lj = G[j * P + j];
            pos += lj > li || (lj == li && j < tid);
        }
        if (pos < kPcaCols) s_sel[pos] = tid;
        if (pos == 0) s_lam0 = li;
    }
    __syncthreads();
    const float thr = __fmul_rn(__fmul_rn((float)k, 0x1p-23f), s_lam0);
    if (tid < q) {
        float lam = 0.0f, sgn = 1.0f;
        if (tid < k) {
            const int col = s_sel[tid];
            const float l = G[col * P + col];
            if (l > thr && l > 0.0f) {
                lam = l;
                // an eigenvector of a non-zero eigenvalue is orthogonal to the constant vector; what rounding leaves of
                // it (about 2^-23 l_0 / l_j) would enter dirs multiplied by (mean - x_0) / sqrt(l_j): centre, renormalise.
                // The rotations' roundings also let |v| drift from 1 (1e-5 at K = 128); the diagonal is v^T G v of that v
                float *v_col = Vt + col * P;
                double sum = 0.0, sq = 0.0;
                for (int i = 0; i < k; ++i) sum += (double)v_col[i];
                const double mean = sum / (double)k;
                for (int i = 0; i < k; ++i) {
                    const double v = (double)v_col[i] - mean;
                    sq += v * v;
                }
                const double scale = 1.0 / sqrt(sq);
                lam = (float)((double)l / sq);                   // the Rayleigh quotient of the unit vector
                for (int i = 0; i < k; ++i) v_col[i] = (float)(((double)v_col[i] - mean) * scale);
                float best = -1.0f;
                for (int i = 0; i < k; ++i) {
                    const float v = v_col[i];
                    if (fabsf(v) > best) {
                        best = fabsf(v);
                        sgn = v < 0.0f ? -1.0f : 1.0f;
                    }
                }
            }
        }
        s_lam[tid] = lam;
        s_sgn[tid] = sgn;
        a.evals[m * q + tid] = lam;
    }
    if (tid == 0) {
        int rank = 0;
        for (int i = 0; i < k; ++i) {
            const float l = G[i * P + i];
            rank += l > thr && l > 0.0f;
        }
        float *o = a.info + m * 4;
        o[0] = (float)s_trace;
        o[1] = converged ? (float)rank : -2.0f;
        o[2] = (float)sweeps;
        o[3] = (float)k;
    }
    __syncthreads();
    float *coords = a.coords + m * k * q;
    for (int idx = tid; idx < k * q; idx += T) {
        const int i = idx / q, j = idx - i * q;
        const float lam = s_lam[j];
        coords[idx] = lam > 0.0f ? sqrtf(lam) * (s_sgn[j] * Vt[s_sel[j] * P + i]) : 0.0f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_pca_project(const PcaArgs a)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    __shared__ __attribute__((aligned(16))) float s_c[kPcaMaxK * kPcaCols];
    __shared__ float s_rcp[kPcaCols];
    __shared__ int s_kind[kPcaCols];             // 0: null, 1: a component, 2: the image is flagged (NaN)
    const int k = a.k, q = a.q;
    const int64_t m = blockIdx.y;
    const float *__restrict__ img = a.x + m * k * a.d;
    const float *coords = a.coords + m * k * q;
    for (int idx = threadIdx.x; idx < k * kPcaCols; idx += kPassThreads) {
        const int i = idx / kPcaCols, j = idx % kPcaCols;
        s_c[idx] = j < q ? coords[i * q + j] : 0.0f;
    }
    if (threadIdx.x < kPcaCols) {
        const float lam = (int)threadIdx.x < q ? a.evals[m * q + threadIdx.x] : 0.0f;
        s_kind[threadIdx.x] = lam != lam ? 2 : (lam > 0.0f ? 1 : 0);
        s_rcp[threadIdx.x] = lam > 0.0f ? __fdiv_rn(1.0f, lam) : 0.0f;
    }
    __syncthreads();
    const Range r = block_range(a.d / W, a.per);
    const bool plain = s_kind[0] != 1;           // block-uniform: component 0 is null or flagged, and so is every other
    for (int64_t u = r.lo + threadIdx.x; u < r.hi; u += kPassThreads) {
        T acc[kPcaCols];
#pragma unroll
        for (int j = 0; j < kPcaCols; ++j) acc[j] = T{};
        if (!plain) {
            const T x0 = ld<T>(img + u * W);
#pragma unroll 4
            for (int i = 0; i < k; ++i) {
                const T xi = ld<T>(img + (int64_t)i * a.d + u * W);
                const float4 c0 = *reinterpret_cast<const float4 *>(s_c + i * kPcaCols);
                const float4 c1 = *reinterpret_cast<const float4 *>(s_c + i * kPcaCols + 4);
                const float cj[kPcaCols] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                T df;
#pragma unroll
                for (int l = 0; l < W; ++l) set(df, l, __fsub_rn(lane(xi, l), lane(x0, l)));
#pragma unroll
                for (int j = 0; j < kPcaCols; ++j)
#pragma unroll
                    for (int l = 0; l < W; ++l) set(acc[j], l, fmaf(cj[j], lane(df, l), lane(acc[j], l)));
            }
        }
#pragma unroll
        for (int j = 0; j < kPcaCols; ++j) {
            if (j >= q) break;                   // launch-uniform
            const int kind = s_kind[j];
            const float rcp = s_rcp[j];
            T o;
#pragma unroll
            for (int l = 0; l < W; ++l)
                set(o, l, kind == 1 ? __fmul_rn(lane(acc[j], l), rcp) : (kind == 2 ? pca_nan() : 0.0f));
            st<T>(a.dirs + (m * q + j) * a.d + u * W, o);
        }
    }
}

// THE workspace layout: [the distance launches' own workspace | d2 [images, K, K] when the caller keeps none]; returns the
// bytes (the size query and the launch path both walk it).  The first region starts at the base: repulse() is handed the
// workspace as it is
int64_t pca_layout(float *&d2, Carver cv, int64_t n, int64_t d, int64_t images)
{
    const int64_t k = n / images;
    cv.take<char>(repulse_workspace_bytes(n, d, images));
    d2 = cv.take<float>(images * k * k);
    return cv.bytes();
}

}  // namespace

int64_t pca_workspace_bytes(int64_t n, int64_t d, int64_t images)
{
    float *d2;
    return pca_layout(d2, Carver(nullptr), n, d, images);
}

int pca(const float *x, int64_t q, float *dirs, float *evals, float *coords, float *info, float *d2, int64_t n, int64_t d,
        int64_t images, void *workspace, hipStream_t s)
{
    const int64_t k = n / images;
    float *dist;
    pca_layout(dist, Carver(workspace), n, d, images);
    if (d2) dist = d2;
    int rc = repulse(false, 0.0f, 0.0f, x, nullptr, dist, nullptr, nullptr, nullptr, n, d, images, workspace, s);
    if (rc != DPSX_OK) return rc;

    const bool vec = vec_ok(d, {x, dirs});
    const PassGeom g = pass_geom(d, vec, images);
    PcaArgs a{};
    a.x = x;
    a.d2 = dist;
    a.dirs = dirs;
    a.evals = evals;
    a.coords = coords;
    a.info = info;
    a.d = d;
    a.per = g.per;
    a.k = (int)k;
    a.q = (int)q;
    const auto eig = [&](auto KP) {
        constexpr int kp = decltype(KP)::value;
        return launch_lds<k_pca_eig<kp>>(dim3((unsigned)images), kp * 8, 2 * kp * (kp + 1) * sizeof(float), s, a);
    };
    rc = k <= 32 ? eig(std::integral_constant<int, 32>{})
                 : (k <= 64 ? eig(std::integral_constant<int, 64>{}) : eig(std::integral_constant<int, 128>{}));
    if (rc != DPSX_OK) return rc;
    return dispatch(vec, [&](auto V) {
        k_pca_project<V.value><<<g.grid, kPassThreads, 0, s>>>(a);
        return check_launch();
    });
}

}  // namespace dpsx
