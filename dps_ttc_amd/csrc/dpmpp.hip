// The multistep update of DPM-Solver++(2M) in K3's place (include/dpsx.h: dpsx_step_update_ms_f32; Lu et al. 2022,
// "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models").
//
// THE expression (tests/dpmpp_ref.py restates it in numpy float32; the bit-for-bit tests follow it).  Per element e of
// particle p, every operation one fp32 rounding (__fmul_rn / __fadd_rn / __fsub_rn; no contraction):
//     s_e      = fadd(fmul(ratio, g_eps_e), g_unet_e)        ratio = -a / b (fp32, host); g_unet absent: + 0.0f (k_step_update)
//     u_e      = fsub(sample_e, s_e)                         K3's x_next
//     x_next_e = c == 0 ? u_e : fadd(u_e, fmul(c, fsub(x0_cur_e, x0_prev_e)))
// c is a host scalar, so c == 0 is launch-uniform: that call IS K3 -- step_update's own launch (elementwise.hip), which
// has no history pointer to read.  (This file's body without the history term gives the same bits but took 34.9 us against
// k_step_update's 31.4 us at N = 64, 256^2: profiles/dpmpp_kbench.txt, the first table.)
//
// The pass is particle_pass.h's: grid (slots, n), block (q, p) owns one contiguous range of particle p; sample and the two
// gradients are its update streams (UpdateArgs, UpdateLoader, update_s; smc.hip and dsg.hip read the same), read for the
// last time of the step, as is x0_prev: non-temporal loads.  x0_cur is the next step's x0_prev: a plain load.  The next
// unit's loads are issued right after a unit's store.  No partials, no atomics: one launch.
#include "particle_pass.h"

namespace dpsx {

namespace {

template <bool VEC>
__global__ __launch_bounds__(kPassThreads) void k_step_update_ms(const UpdateArgs a, const float *__restrict__ x0_cur,
                                                                 const float *__restrict__ x0_prev, float c)
{
    using T = typename Unit<VEC>::T;
    constexpr int W = Unit<VEC>::W;
    const int64_t p = blockIdx.y, base = p * a.chw;
    const Range r = block_range(a.chw / W, a.per);
    UpdateLoader<VEC, false, true, true> in(a, p, false, false);
    T cv = T{}, pv = T{};
    int64_t u = r.lo + threadIdx.x;
    if (u < r.hi) {
        in.load(u);
        cv = ld<T>(x0_cur + base + u * W);
        pv = ld_last<T>(x0_prev + base + u * W);
    }
    while (u < r.hi) {
        T xn;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float x = __fsub_rn(lane(in.sv, j), update_s(lane(in.gv, j), lane(in.uv, j), a));
            set(xn, j, __fadd_rn(x, __fmul_rn(c, __fsub_rn(lane(cv, j), lane(pv, j)))));
        }
        st<T>(a.out + base + u * W, xn);
        u += kPassThreads;
        if (u < r.hi) {
            in.load(u);
            cv = ld<T>(x0_cur + base + u * W);
            pv = ld_last<T>(x0_prev + base + u * W);
        }
    }
}

}  // namespace

int step_update_ms(const float *sample, const float *g_mo, const float *g_unet, const float *x0_cur, const float *x0_prev,
                   float c, float *x_next, int64_t n, int64_t chw, const Coefs &k, hipStream_t s)
{
    if (n == 0 || chw == 0) return DPSX_OK;
    if (c == 0.0f) return step_update(sample, g_mo, g_unet, x_next, n, chw, k, s);      // the histories are not read
    const bool vec = vec_ok(chw, {sample, g_mo, g_unet, x_next, x0_cur, x0_prev});
    const PassGeom g = pass_geom(chw, vec, n);
    const UpdateArgs a{sample, g_mo, g_unet, nullptr, nullptr, x_next, nullptr, chw, g.per, -k.a / k.b, 0.0f, k, RngK{}};
    return dispatch(vec, [&](auto V) {
        k_step_update_ms<V.value><<<g.grid, kPassThreads, 0, s>>>(a, x0_cur, x0_prev, c);
        return check_launch();
    });
}

}  // namespace dpsx
