// C ABI of libdpsx (see include/dpsx.h): argument checks, operator objects and
// dispatch to the kernels.  No torch types, no allocation on the launch path.
#include <cmath>
#include <cstring>
#include <new>
#include <algorithm>
#include <vector>

#include "common.h"

using namespace dpsx;

namespace dpsx {
static thread_local char g_hip_err[256] = "";
void set_last_hip_error(hipError_t e)
{
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", hipGetErrorName(e), hipGetErrorString(e));
}
}  // namespace dpsx

#pragma GCC visibility push(default)
extern "C" {

int dpsx_abi_version(void) { return DPSX_ABI_VERSION; }

const char *dpsx_strerror(int code)
{
    switch (code) {
    case DPSX_OK: return "ok";
    case DPSX_EINVAL: return "invalid argument";
    case DPSX_EUNSUPPORTED: return "unsupported configuration";
    case DPSX_ELAUNCH: return "HIP launch/runtime error";
    case DPSX_ENOMEM: return "out of device memory";
    case DPSX_EWORKSPACE: return "workspace too small";
    }
    return "unknown error";
}

const char *dpsx_last_hip_error(void) { return g_hip_err; }

// ------------------------------------------------------------------ S1
int dpsx_posterior_fwd_f32(const float *x_t, const float *model_out, const float *noise, float *x0_hat,
                           float *sample, uint8_t *inside, int64_t n, int64_t chw,
                           const dpsx_coefs *coefs_host, void *stream)
{
    if (!coefs_host || n < 0 || chw < 0) return DPSX_EINVAL;
    if (n == 0 || chw == 0) return DPSX_OK;   // empty particle set: nothing to do (pointers may be null)
    if (!x_t || !model_out) return DPSX_EINVAL;
    if ((coefs_host->add_noise & 1) && !noise) return DPSX_EINVAL;
    return posterior_fwd(x_t, model_out, noise, false, RngK{}, x0_hat, sample, inside, n, chw, to_coefs(coefs_host),
                         (hipStream_t)stream);
}

int dpsx_posterior_bwd_f32(const float *g_x0, const float *g_sample, const float *x_t, const float *model_out,
                           const float *noise, float *g_x, float *g_model_out, int64_t n, int64_t chw,
                           const dpsx_coefs *coefs_host, void *stream)
{
    if (!coefs_host || n < 0 || chw < 0) return DPSX_EINVAL;
    if (n == 0 || chw == 0) return DPSX_OK;
    if (!x_t || !model_out || !g_x || !g_model_out) return DPSX_EINVAL;
    if ((coefs_host->add_noise & 1) && g_sample && !noise) return DPSX_EINVAL;
    return posterior_bwd(g_x0, g_sample, x_t, model_out, noise, g_x, g_model_out, n, chw, to_coefs(coefs_host),
                         (hipStream_t)stream);
}

// ------------------------------------------------------------------ counter-based normals
// dpsx_rng -> the launch record; every particle id of the n rows must fit 32 bits
static int to_rngk(const dpsx_rng *r, int64_t n, RngK &o)
{
    if (!r || r->particle_base < 0 || r->per_image < 0) return DPSX_EINVAL;
    const int64_t rows = std::max<int64_t>(n, 1);
    const int64_t per = (r->per_image > 0 && r->per_image < rows) ? r->per_image : 0;   // per >= n: p % per == p
    if (r->particle_base + (per ? per : rows) - 1 > 0xffffffffll) return DPSX_EINVAL;
    o = RngK{(uint32_t)(r->seed & 0xffffffffu), (uint32_t)(r->seed >> 32), r->step, r->tag,
             (uint32_t)r->particle_base, (uint32_t)per};
    return DPSX_OK;
}

int dpsx_randn_f32(float *out, uint32_t *bits_out, int64_t n, int64_t chw, const dpsx_rng *rng_host, void *stream)
{
    if (n < 0 || chw < 0 || n > 65535) return DPSX_EINVAL;
    RngK r;
    int rc = to_rngk(rng_host, n, r);
    if (rc != DPSX_OK) return rc;
    if (n == 0 || chw == 0) return DPSX_OK;
    if (!out) return DPSX_EINVAL;
    return randn_f32(out, bits_out, n, chw, r, (hipStream_t)stream);
}

int dpsx_posterior_fwd_rng_f32(const float *x_t, const float *model_out, const dpsx_rng *rng_host, float *x0_hat,
                               float *sample, uint8_t *inside, int64_t n, int64_t chw,
                               const dpsx_coefs *coefs_host, void *stream)
{
    if (!coefs_host || n < 0 || chw < 0) return DPSX_EINVAL;
    RngK r;
    int rc = to_rngk(rng_host, n, r);
    if (rc != DPSX_OK) return rc;
    if (n == 0 || chw == 0) return DPSX_OK;
    if (!x_t || !model_out) return DPSX_EINVAL;
    return posterior_fwd(x_t, model_out, nullptr, true, r, x0_hat, sample, inside, n, chw, to_coefs(coefs_host),
                         (hipStream_t)stream);
}

// ------------------------------------------------------------------ operator objects
// arrival counters of the in-launch norm (common.h: NormTail); zero between launches
static int alloc_counters(dpsx_op *op)
{
    DPSX_HIP_TRY(hipMalloc((void **)&op->d_counters, kNormCounterBytes));
    DPSX_HIP_TRY(hipMemset(op->d_counters, 0, kNormCounterBytes));
    return DPSX_OK;
}

static dpsx_op *new_op(int kind)
{
    dpsx_op *op = new (std::nothrow) dpsx_op();
    if (op) op->kind = kind;
    return op;
}

// what every constructor ends with; rc: the kind's own construction (blur.hip, resize.hip, phase.hip)
static int finish_create(dpsx_op *op, int rc, dpsx_op **out)
{
    if (rc == DPSX_OK) rc = alloc_counters(op);
    if (rc != DPSX_OK) { dpsx_op_destroy(op); return rc; }
    *out = op;
    return DPSX_OK;
}

int dpsx_op_create_blur(const float *kernel_host, int ks, int mode, dpsx_op **out)
{
    if (!kernel_host || !out || ks < 1 || ks % 2 == 0 || ks > 2 * kMaxRadius + 1) return DPSX_EINVAL;
    dpsx_op *op = new_op(OP_TAPS);       // blur_create: OP_SEP for a rank-1 kernel
    if (!op) return DPSX_ENOMEM;
    return finish_create(op, blur_create(op, kernel_host, ks, mode), out);
}

int dpsx_op_create_resize(int64_t in_h, int64_t in_w, const float *w_h_host, const int64_t *i_h_host,
                          int64_t taps_h, int64_t out_h, const float *w_w_host, const int64_t *i_w_host,
                          int64_t taps_w, int64_t out_w, dpsx_op **out)
{
    if (!w_h_host || !i_h_host || !w_w_host || !i_w_host || !out) return DPSX_EINVAL;
    if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || taps_h < 1 || taps_w < 1) return DPSX_EINVAL;
    if (in_h > 16384 || in_w > 16384) return DPSX_EUNSUPPORTED;
    dpsx_op *op = new_op(OP_RESIZE);
    if (!op) return DPSX_ENOMEM;
    const ResizeOp shape{in_h, in_w, out_h, out_w, taps_h, taps_w};
    return finish_create(op, resize_create(op, shape, w_h_host, i_h_host, w_w_host, i_w_host), out);
}

int dpsx_op_create_mask(const float *mask_dev, int64_t h, int64_t w, dpsx_op **out)
{
    return dpsx_op_create_mask_n(mask_dev, 1, h, w, out);
}

int dpsx_op_create_mask_n(const float *mask_dev, int64_t mask_n, int64_t h, int64_t w, dpsx_op **out)
{
    if (!mask_dev || !out || mask_n < 1 || mask_n > (1 << 24) || h < 1 || w < 1) return DPSX_EINVAL;
    dpsx_op *op = new_op(OP_MASK);
    if (!op) return DPSX_ENOMEM;
    op->mask = MaskOp{mask_dev, mask_n, h, w};
    return finish_create(op, DPSX_OK, out);
}

int dpsx_op_create_identity(dpsx_op **out)
{
    if (!out) return DPSX_EINVAL;
    dpsx_op *op = new_op(OP_IDENT);
    if (!op) return DPSX_ENOMEM;
    return finish_create(op, DPSX_OK, out);
}

int dpsx_op_create_phase(int64_t h, int64_t pad, int64_t max_planes, dpsx_op **out)
{
    if (!out || h < 1 || pad < 0 || max_planes < 1 || (h + 2 * pad) % 2 != 0) return DPSX_EINVAL;
    dpsx_op *op = new_op(OP_PHASE);
    if (!op) return DPSX_ENOMEM;
    return finish_create(op, phase_create(op, PhaseOp{h, pad, max_planes}), out);
}

void dpsx_op_destroy(dpsx_op *op)
{
    if (!op) return;
    if (op->d_counters) (void)hipFree(op->d_counters);
    if (op->blur) blur_destroy(op);
    if (op->resize) resize_destroy(op);
    if (op->phase) phase_destroy(op);
    delete op;
}

int dpsx_op_kind(const dpsx_op *op) { return op ? op->kind : DPSX_EINVAL; }

int dpsx_op_out_shape(const dpsx_op *op, int64_t h, int64_t w, int64_t *out_h, int64_t *out_w)
{
    if (!op || !out_h || !out_w) return DPSX_EINVAL;
    switch (op->kind) {
    case OP_RESIZE:
        if (h != op->resize->in_h || w != op->resize->in_w) return DPSX_EINVAL;
        *out_h = op->resize->out_h; *out_w = op->resize->out_w;
        return DPSX_OK;
    case OP_PHASE:
        if (h != op->phase->h || w != op->phase->h) return DPSX_EINVAL;
        *out_h = *out_w = op->phase->h + 2 * op->phase->pad;
        return DPSX_OK;
    case OP_MASK:
        if (h != op->mask.h || w != op->mask.w) return DPSX_EINVAL;
        [[fallthrough]];
    default:
        *out_h = h; *out_w = w;
        return DPSX_OK;
    }
}

// partial sums-of-squares slots per particle for the fused paths
static int64_t parts_per_particle(const dpsx_op *op, int64_t c, int64_t h, int64_t w)
{
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS: return blur_parts_per_particle(op, c, h, w);
    case OP_RESIZE: return resize_parts_per_particle(op, c);
    case OP_MASK:
    case OP_IDENT: return (c * h * w + 1023) / 1024;
    case OP_PHASE: return phase_parts_per_particle(op, c);
    }
    return 1;
}

// The two slot-count rules: how many partial sums per particle a launch leaves for its finisher to re-sum.  The generic
// residual pass (elementwise.hip: residual_partials) takes its chunk count from the caller, and it is kResidualSlots
// wherever this file chooses it; every workspace holds at least that many slots per particle.
constexpr int kResidualSlots = 64;
// the fused step: the forward half's partials, re-summed by the in-launch norm, finalize_norm or the backward prologue
static int step_parts(const dpsx_op *op, int64_t c, int64_t h, int64_t w)
{
    return op->kind == OP_IDENT ? kResidualSlots : (int)parts_per_particle(op, c, h, w);
}
// scoring: inpainting, the identity and phase retrieval score through the generic residual pass
static int score_parts(const dpsx_op *op, int64_t c, int64_t h, int64_t w)
{
    if (op->kind == OP_IDENT || op->kind == OP_MASK || op->kind == OP_PHASE) return kResidualSlots;
    return (int)parts_per_particle(op, c, h, w);
}

static int64_t meas_elems(const dpsx_op *op, int64_t c, int64_t h, int64_t w)
{
    int64_t oh = h, ow = w;
    if (dpsx_op_out_shape(op, h, w, &oh, &ow) != DPSX_OK) return -1;
    return c * oh * ow;
}

// THE workspace layout of an operator: [partials | the kind's own part].  Blur: the adjoint's padded-domain scratch.
// Phase, identity, mask (the ops with unfused routes): scratch A (measurement-sized), scratch B (image-sized), then
// whatever remains -- phase's transform buffer.  Resize: nothing.
struct Ws {
    float *partials;
    float *meas;   // measurement-sized scratch (only for unfused ops)
    float *img;    // image-sized scratch (only for unfused ops)
    void *priv;
    int64_t priv_bytes;
};

// carves `base` of ws_bytes (nullable: sizes only) and returns the bytes needed, or a negative DPSX_E* code
static int64_t op_carve(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w, void *base, int64_t ws_bytes, Ws *o)
{
    const int64_t m = meas_elems(op, c, h, w);
    if (m < 0) return DPSX_EINVAL;
    Carver cv(base);
    Ws k{};
    k.partials = cv.take<float>(n * std::max<int64_t>(parts_per_particle(op, c, h, w), kResidualSlots));
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS:
        k.priv_bytes = blur_adjoint_scratch_bytes(op, n * c, h, w);
        k.priv = cv.take<char>(k.priv_bytes);
        break;
    case OP_PHASE:
    case OP_IDENT:
    case OP_MASK:
        k.meas = cv.take<float>(n * m);
        k.img = cv.take<float>(n * c * h * w);
        k.priv_bytes = ws_bytes - cv.bytes();
        k.priv = cv.take<char>(op->kind == OP_PHASE ? phase_workspace_bytes(op, n * c) : 0);
        break;
    }
    if (o) *o = k;
    return cv.bytes();
}

int64_t dpsx_op_workspace_bytes(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w)
{
    if (!op || n < 0 || c < 1 || h < 1 || w < 1) return DPSX_EINVAL;
    return op_carve(op, n, c, h, w, nullptr, 0, nullptr);
}

// the launch path's form: the caller checked the geometry (check_geom)
static int carve(const dpsx_op *op, void *ws, int64_t ws_bytes, int64_t n, int64_t c, int64_t h, int64_t w, Ws &o)
{
    return workspace_check(ws, ws_bytes, op_carve(op, n, c, h, w, ws, ws_bytes, &o));
}

// a table of `rows` entries serves n particles when rows divides n (common.h: meas_row); rows == n == 0 stays valid
static bool rows_ok(int64_t rows, int64_t n) { return rows == 1 || rows == n || (rows > 1 && n % rows == 0); }

static int check_geom(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w)
{
    if (!op || n < 0 || c < 1 || h < 1 || w < 1) return DPSX_EINVAL;
    if (op->kind == OP_MASK && !rows_ok(op->mask.rows, n)) return DPSX_EINVAL;
    if (n * c > (1 << 24)) return DPSX_EUNSUPPORTED;
    int64_t oh, ow;
    return dpsx_op_out_shape(op, h, w, &oh, &ow);
}

int dpsx_op_forward_f32(dpsx_op *op, const float *x, float *y, int64_t n, int64_t c, int64_t h, int64_t w,
                        void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (!x || !y) return DPSX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS: return blur_forward(op, x, y, n * c, h, w, s);
    case OP_RESIZE: return resize_forward(op, x, y, n * c, s);
    case OP_MASK: return mask_mul(x, op->mask.mask, y, n * c, h * w, s, c, row_div(op->mask.rows, n));
    case OP_IDENT:
        DPSX_HIP_TRY(hipMemcpyAsync(y, x, (size_t)(n * c * h * w) * 4, hipMemcpyDeviceToDevice, s));
        return DPSX_OK;
    case OP_PHASE: {
        Ws ws;
        if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
        return phase_forward(op, x, y, nullptr, n * c, ws.priv, ws.priv_bytes, s);
    }
    }
    return DPSX_EUNSUPPORTED;
}

int dpsx_op_adjoint_f32(dpsx_op *op, const float *u, const float *x, float *g, int64_t n, int64_t c, int64_t h,
                        int64_t w, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (!u || !g) return DPSX_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS: {
        Ws ws;
        if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
        return blur_adjoint(op, u, g, n * c, h, w, static_cast<float *>(ws.priv), ws.priv_bytes, s);
    }
    case OP_RESIZE: return resize_adjoint(op, u, g, n * c, s);
    case OP_MASK: return mask_mul(u, op->mask.mask, g, n * c, h * w, s, c, row_div(op->mask.rows, n));
    case OP_IDENT:
        DPSX_HIP_TRY(hipMemcpyAsync(g, u, (size_t)(n * c * h * w) * 4, hipMemcpyDeviceToDevice, s));
        return DPSX_OK;
    case OP_PHASE: {
        if (!x) return DPSX_EINVAL;
        Ws ws;
        if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
        return phase_adjoint(op, u, x, g, n * c, ws.priv, ws.priv_bytes, s);
    }
    }
    return DPSX_EUNSUPPORTED;
}

// ------------------------------------------------------------------ residual norm
int dpsx_residual_norm_f32(const float *y, int64_t y_n, const float *ax, float *r, float *norm, int64_t n,
                           int64_t m, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!y || !ax || !norm || n < 0 || m < 0 || !rows_ok(y_n, n)) return DPSX_EINVAL;
    if (n == 0) return DPSX_OK;
    const int parts = (int)std::min<int64_t>(256, std::max<int64_t>(1, (m + 4095) / 4096));
    if (!workspace || workspace_bytes < n * parts * 4) return DPSX_EWORKSPACE;
    float *partials = static_cast<float *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    int rc = residual_partials(y, y_n, ax, r, partials, n, m, parts, s);
    if (rc != DPSX_OK) return rc;
    return finalize_norm(partials, parts, norm, n, s);
}

int dpsx_norm_bwd_f32(const float *r, const float *norm, const float *g_norm, int power, float *g_ax, int64_t n,
                      int64_t m, void *stream)
{
    if (!r || !norm || !g_norm || !g_ax || n < 0 || m < 0 || (power != 1 && power != 2)) return DPSX_EINVAL;
    return norm_bwd(r, norm, g_norm, power, g_ax, n, m, (hipStream_t)stream);
}

// ------------------------------------------------------------------ fused DPS step
int64_t dpsx_step_resid_bytes(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w)
{
    if (!op) return DPSX_EINVAL;
    const int64_t m = meas_elems(op, c, h, w);
    if (m < 0) return DPSX_EINVAL;
    switch (op->kind) {
    case OP_MASK: return 256;                         // residual is recomputed from x0_hat
    case OP_PHASE: return phase_step_resid_bytes(op, n * c);   // padded real image + Hermitian half spectrum
    default: return align256(n * m * 4);
    }
}

// the fused inpainting step has the 16-byte form only (common.h: vec_ok): whole float4 units per plane, so that a unit
// has one mask row, as well as per particle; ptrs: the launch's buffers beside the mask
static bool mask_fused_ok(const dpsx_op *op, int64_t c, int64_t h, int64_t w,
                          std::initializer_list<const void *> ptrs)
{
    return (h * w) % 4 == 0 && aligned16(op->mask.mask) && vec_ok(c * h * w, ptrs);
}

int dpsx_step_draws_in_kernel(const dpsx_op *op, int64_t c, int64_t h, int64_t w)
{
    if (!op || c < 1 || h < 1 || w < 1) return 0;
    switch (op->kind) {
    case OP_IDENT: return 1;
    case OP_MASK: return (h * w) % 4 == 0 && (c * h * w) % 4 == 0;
    case OP_SEP:
    case OP_TAPS: return blur_step_draws_in_kernel(op, h, w) ? 1 : 0;
    case OP_RESIZE: return h == op->resize->in_h && w == op->resize->in_w && resize_step_draws_in_kernel(op) ? 1 : 0;
    default: return 0;       // phase retrieval: fill + pointer form
    }
}

// rng != NULL: the noise is drawn inside the launch (noise is then NULL).  Routes without an in-kernel draw decline
// before anything is launched.
static int step_fwd_impl(dpsx_op *op, const float *x_t, const float *model_out, const float *noise, const dpsx_rng *rng,
                         const float *y, int64_t y_n, float *x0_hat, float *sample, uint8_t *inside, void *resid,
                         float *norm, int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                         void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    RngK rk{};
    if (rng) {
        if ((rc = to_rngk(rng, n, rk)) != DPSX_OK) return rc;
        if (!dpsx_step_draws_in_kernel(op, c, h, w)) return DPSX_EUNSUPPORTED;
    }
    if (!x_t || !model_out || !y || !sample || !inside || !resid || !coefs_host) return DPSX_EINVAL;
    // x0_hat is an optional OUTPUT where the launch consumes it on the fly (blur, resize): the `ps` loop reads it nowhere
    // after this call (the backward half works from the clamp gate), so a caller that does not need the image saves its
    // store (blur, resize, the hand-written spectral phase step); inpainting's backward half, the identity and the
    // library-FFT phase paths read it back and need it
    if (!x0_hat && op && op->kind != OP_SEP && op->kind != OP_TAPS && op->kind != OP_RESIZE &&
        !(op->kind == OP_PHASE && phase_is_spectral(op)))
        return DPSX_EINVAL;
    if ((coefs_host->add_noise & 1) && !noise && !rng) return DPSX_EINVAL;
    if (!rows_ok(y_n, n)) return DPSX_EINVAL;
    if (n == 0) return DPSX_OK;
    Ws ws;
    if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Coefs k = to_coefs(coefs_host);
    const int64_t chw = c * h * w;
    StepFwdArgs a{x_t, model_out, noise, y, y_n, x0_hat, sample, inside, static_cast<float *>(resid),
                  ws.partials, n, c, h, w, k};
    a.y_div = row_div(y_n, n);
    a.mask_div = row_div(op->mask.rows, n);
    a.use_rng = rng != nullptr;
    a.rng = rk;
    const int parts = step_parts(op, c, h, w);
    // norm != NULL: the launch itself finishes the per-particle reduction (each particle's last block re-sums its
    // partials in the order of k_finalize_norm -- bit-identical, no extra launch; common.h: NormTail)
    bool tail_done = false;
    if (norm && op->d_counters && n <= kTailMaxParticles && op->kind != OP_PHASE) {
        a.tail.counters = op->d_counters;
        a.tail.partials = ws.partials;
        a.tail.parts = parts;
        a.tail.out = norm;
        tail_done = true;
    }
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS: rc = blur_step_fwd(op, a, s); break;
    case OP_RESIZE: rc = resize_step_fwd(op, a, s); break;
    case OP_MASK:
        // shapes that are not a multiple of 4 have no fused form: the Python front end asks first (OpHandle.fuses_step in
        // kernels.py mirrors mask_fused_ok) and GaussianDiffusion._fusion_plan then runs the step per op under autograd --
        // S1, dpsx_op_forward_f32, dpsx_residual_norm_f32 and their VJPs; a caller that launches anyway gets the refusal
        if (!mask_fused_ok(op, c, h, w, {x_t, model_out, noise, y, x0_hat, sample}) ||
            !aligned4(inside))
            return DPSX_EUNSUPPORTED;
        rc = mask_step_fwd(op, a, parts, s);
        break;
    case OP_IDENT:
        rc = posterior_fwd(x_t, model_out, noise, a.use_rng, rk, x0_hat, sample, inside, n, chw, k, s);
        if (rc != DPSX_OK) return rc;
        rc = residual_partials(y, y_n, x0_hat, static_cast<float *>(resid), ws.partials, n, chw, parts, s, 0, nullptr, 0, 1,
                               a.tail);
        break;
    case OP_PHASE:
        // resid is the transforms' own buffer here (padded image + half spectrum, complex words): 16 bytes like a workspace
        if (!aligned16(resid)) return DPSX_EUNSUPPORTED;
        rc = phase_step_fwd(op, a, static_cast<float *>(resid), s);      // S1 + staging + R2C + residual / cotangent
        break;
    default: return DPSX_EUNSUPPORTED;
    }
    if (rc != DPSX_OK) {
        // a launch that failed part-way may leave arrival counters non-zero: clear them behind whatever did run, so that
        // the handle's next in-launch reduction does not start from a stale count
        if (tail_done)
            (void)hipMemsetAsync(op->d_counters, 0, kNormCounterBytes, s);
        return rc;
    }
    // norm == NULL: the partial sums stay in `workspace` and dpsx_step_bwd_f32 finalises them in its prologue
    return (norm && !tail_done) ? finalize_norm(ws.partials, parts, norm, n, s) : DPSX_OK;
}

int dpsx_step_fwd_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise, const float *y,
                      int64_t y_n, float *x0_hat, float *sample, uint8_t *inside, void *resid, float *norm,
                      int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host, void *workspace,
                      int64_t workspace_bytes, void *stream)
{
    return step_fwd_impl(op, x_t, model_out, noise, nullptr, y, y_n, x0_hat, sample, inside, resid, norm, n, c, h, w,
                         coefs_host, workspace, workspace_bytes, stream);
}

int dpsx_step_fwd_rng_f32(dpsx_op *op, const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                          const float *y, int64_t y_n, float *x0_hat, float *sample, uint8_t *inside, void *resid,
                          float *norm, int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                          void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!rng_host) return DPSX_EINVAL;
    return step_fwd_impl(op, x_t, model_out, nullptr, rng_host, y, y_n, x0_hat, sample, inside, resid, norm, n, c, h, w,
                         coefs_host, workspace, workspace_bytes, stream);
}

int dpsx_step_bwd_f32(dpsx_op *op, const void *resid, const float *norm, float *norm_out, const uint8_t *inside,
                      const float *x0_hat, const float *y, int64_t y_n, float scale, int power,
                      float *g_model_out, int64_t n, int64_t c, int64_t h, int64_t w,
                      const dpsx_coefs *coefs_host, void *workspace, int64_t workspace_bytes, void *stream)
{
    return dpsx_step_bwd_extra_f32(op, resid, norm, norm_out, inside, x0_hat, y, y_n, scale, power, nullptr,
                                   g_model_out, n, c, h, w, coefs_host, workspace, workspace_bytes, stream);
}

int dpsx_step_bwd_extra_f32(dpsx_op *op, const void *resid, const float *norm, float *norm_out,
                            const uint8_t *inside, const float *x0_hat, const float *y, int64_t y_n, float scale,
                            int power, const float *g_x0_extra, float *g_model_out, int64_t n, int64_t c, int64_t h,
                            int64_t w, const dpsx_coefs *coefs_host, void *workspace, int64_t workspace_bytes,
                            void *stream)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (!resid || !inside || !g_model_out || !coefs_host || (power != 1 && power != 2)) return DPSX_EINVAL;
    if (!norm && !norm_out) return DPSX_EINVAL;
    if (y && !rows_ok(y_n, n)) return DPSX_EINVAL;
    if (n == 0) return DPSX_OK;
    Ws ws;
    if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Coefs k = to_coefs(coefs_host);
    const int64_t chw = c * h * w;
    const int parts = step_parts(op, c, h, w);
    if (op->kind == OP_PHASE && !aligned16(resid)) return DPSX_EUNSUPPORTED;       // as in the forward half
    if (op->kind == OP_IDENT || op->kind == OP_PHASE) {
        // (the hand-written spectral phase step finalises the norm in its backward launch's prologue)
        if (!norm && !(op->kind == OP_PHASE && phase_norm_in_bwd(op))) {     // no fused prologue: finalise with the small kernel
            if ((rc = finalize_norm(ws.partials, parts, norm_out, n, s)) != DPSX_OK) return rc;
            norm = norm_out;
        }
    }
    StepBwdArgs b{static_cast<const float *>(resid), norm, ws.partials, parts, norm_out, inside, x0_hat, y, y_n,
                  scale, power, g_model_out, n, c, h, w, k, g_x0_extra};
    b.y_div = row_div(y_n, n);
    b.mask_div = row_div(op->mask.rows, n);
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS: return blur_step_bwd(op, b, static_cast<float *>(ws.priv), ws.priv_bytes, s);
    case OP_RESIZE: return resize_step_bwd(op, b, s);
    case OP_MASK:
        if (!x0_hat || !y || !rows_ok(y_n, n)) return DPSX_EINVAL;
        if (!mask_fused_ok(op, c, h, w, {x0_hat, y, g_model_out, g_x0_extra}) || !aligned4(inside))
            return DPSX_EUNSUPPORTED;
        return mask_step_bwd(op, b, s);
    case OP_IDENT:
        return clamp_scale_to_eps(static_cast<const float *>(resid), norm, inside, scale, power, g_model_out, n,
                                  chw, k, s, g_x0_extra);
    case OP_PHASE:
        if (phase_vec4_ok(op) && vec_ok(h, {g_model_out, g_x0_extra}) && aligned4(inside))   // (h % 4 == 0: phase_vec4_ok)
            return phase_step_bwd_fused(op, const_cast<float *>(static_cast<const float *>(resid)), b, s);
        if (phase_is_spectral(op)) return DPSX_EUNSUPPORTED;     // its buffers have no unaligned form
        rc = phase_step_bwd(op, const_cast<float *>(static_cast<const float *>(resid)), ws.img, n * c, s);
        if (rc != DPSX_OK) return rc;
        return clamp_scale_to_eps(ws.img, norm, inside, scale, power, g_model_out, n, chw, k, s, g_x0_extra);
    }
    return DPSX_EUNSUPPORTED;
}

int dpsx_step_update_f32(const float *sample, const float *g_model_out, const float *g_unet, float *x_next,
                         int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream)
{
    if (!sample || !g_model_out || !x_next || !coefs_host || n < 0 || chw < 0) return DPSX_EINVAL;
    if (coefs_host->b == 0.0f) return DPSX_EINVAL;
    return step_update(sample, g_model_out, g_unet, x_next, n, chw, to_coefs(coefs_host), (hipStream_t)stream);
}

// ------------------------------------------------------------------ particle weights (smc.hip)
int dpsx_corr_slots(int64_t chw) { return chw < 0 ? DPSX_EINVAL : cg_slots(chw); }

// what the entry points in K3's place share: the argument checks and the launch form of the noise counters
static int update_place_args(const float *sample, const float *g_model_out, const float *model_out, const float *noise,
                             const dpsx_rng *rng_host, const float *x_next, int64_t n, int64_t chw,
                             const dpsx_coefs *coefs_host, RngK &r)
{
    if (!sample || !g_model_out || !x_next || !coefs_host || n < 0 || chw < 0) return DPSX_EINVAL;
    if ((noise != nullptr) == (rng_host != nullptr)) return DPSX_EINVAL;         // exactly one noise source, whatever the step
    if (coefs_host->b == 0.0f) return DPSX_EINVAL;
    const int mode = coefs_host->add_noise;
    if ((mode & 1) && (mode & 2) && !(coefs_host->min_log > 0.0f)) return DPSX_EINVAL;      // eta = 0: sd = 0, no density, no sphere
    if ((mode & 1) && !(mode & 2) && !model_out) return DPSX_EINVAL;                       // sd comes from its variance half
    r = RngK{};
    if (rng_host) {
        int rc = to_rngk(rng_host, n, r);
        if (rc != DPSX_OK) return rc;
    }
    return n > 65535 ? DPSX_EUNSUPPORTED : DPSX_OK;                // particles are the grid's y dimension
}

int dpsx_step_update_corr_f32(const float *sample, const float *g_model_out, const float *g_unet, const float *model_out,
                              const float *noise, const dpsx_rng *rng_host, float *x_next, float *corr_partials, int64_t n,
                              int64_t chw, const dpsx_coefs *coefs_host, void *stream)
{
    if (!corr_partials) return DPSX_EINVAL;
    RngK r;
    const int rc = update_place_args(sample, g_model_out, model_out, noise, rng_host, x_next, n, chw, coefs_host, r);
    if (rc != DPSX_OK) return rc;
    return step_update_corr(sample, g_model_out, g_unet, model_out, noise, rng_host != nullptr, r, x_next, corr_partials, n,
                            chw, to_coefs(coefs_host), (hipStream_t)stream);
}

int dpsx_smc_accum_f32(float *E, float *d_prev, const float *d_cur, const float *corr_partials, int slots,
                       const uint8_t *reset, int64_t segments, int64_t n, float twist_scale, int power,
                       float proposal_weight, void *stream)
{
    if (!E || !d_prev || !d_cur || n < 0 || segments < 1 || n % segments) return DPSX_EINVAL;
    if (power != 1 && power != 2) return DPSX_EINVAL;
    if (corr_partials && slots < 1) return DPSX_EINVAL;
    if (!std::isfinite(twist_scale) || !std::isfinite(proposal_weight)) return DPSX_EINVAL;
    if (n > 65535) return DPSX_EUNSUPPORTED;
    return smc_accum(E, d_prev, d_cur, corr_partials, slots, reset, segments, n, twist_scale, power, proposal_weight,
                     (hipStream_t)stream);
}

// ------------------------------------------------------------------ spherical-Gaussian guidance (dsg.hip)
int dpsx_step_update_dsg_f32(const float *sample, const float *g_model_out, const float *g_unet, const float *model_out,
                             const float *noise, const dpsx_rng *rng_host, float guidance_rate, float *x_next, float *stats,
                             int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream)
{
    if (!stats || !(guidance_rate >= 0.0f && guidance_rate <= 1.0f)) return DPSX_EINVAL;    // NaN included
    RngK r;
    const int rc = update_place_args(sample, g_model_out, model_out, noise, rng_host, x_next, n, chw, coefs_host, r);
    if (rc != DPSX_OK) return rc;
    return step_update_dsg(sample, g_model_out, g_unet, model_out, noise, rng_host != nullptr, r, guidance_rate, x_next,
                           stats, n, chw, to_coefs(coefs_host), (hipStream_t)stream);
}

// ------------------------------------------------------------------ the multistep update (dpmpp.hip)
int dpsx_step_update_ms_f32(const float *sample, const float *g_model_out, const float *g_unet, const float *x0_cur,
                            const float *x0_prev, float c, float *x_next, int64_t n, int64_t chw,
                            const dpsx_coefs *coefs_host, void *stream)
{
    if (!sample || !g_model_out || !x_next || !coefs_host || n < 0 || chw < 1) return DPSX_EINVAL;
    if (coefs_host->b == 0.0f || !std::isfinite(c)) return DPSX_EINVAL;
    if (c != 0.0f && (!x0_cur || !x0_prev)) return DPSX_EINVAL;
    if (n > 65535) return DPSX_EUNSUPPORTED;                       // particles are the grid's y dimension
    return step_update_ms(sample, g_model_out, g_unet, x0_cur, x0_prev, c, x_next, n, chw, to_coefs(coefs_host),
                          (hipStream_t)stream);
}

// ------------------------------------------------------------------ image metrics (metrics.hip)
int64_t dpsx_metrics_workspace_bytes(int64_t n, int64_t m, int64_t c, int64_t h, int64_t w)
{
    if (n < 0 || m < 1 || n % m) return DPSX_EINVAL;
    if (c < 1 || h < 1 || w < 1) return DPSX_EINVAL;
    if (n > 65535 || !metrics_shape_ok(c, h, w)) return DPSX_EUNSUPPORTED;
    return metrics_workspace_bytes(n, m, c, h, w);
}

int dpsx_image_metrics_f32(const float *x, const float *label, int64_t m, float data_range, float *mse, float *psnr,
                           float *ssim, int64_t n, int64_t c, int64_t h, int64_t w, void *workspace,
                           int64_t workspace_bytes, void *stream)
{
    if (!x || !label || !workspace || (!mse && !psnr && !ssim)) return DPSX_EINVAL;
    if (n < 0 || m < 1 || n % m || c < 1 || h < 1 || w < 1) return DPSX_EINVAL;
    if (!(data_range >= 0.0f) || !std::isfinite(data_range)) return DPSX_EINVAL;           // NaN included
    if (ssim && (h < 11 || w < 11)) return DPSX_EINVAL;
    if (n > 65535 || !metrics_shape_ok(c, h, w)) return DPSX_EUNSUPPORTED;
    const int rc = workspace_check(workspace, workspace_bytes, metrics_workspace_bytes(n, m, c, h, w));
    if (rc != DPSX_OK) return rc;
    return image_metrics(x, label, m, data_range, mse, psnr, ssim, n, c, h, w, workspace, (hipStream_t)stream);
}

// ------------------------------------------------------------------ particle repulsion (repulse.hip)
// The entries over an image-major particle set (from here to the principal components) check in this order: their pointers
// and arguments -- a null workspace is one: DPSX_EINVAL --, the set's shape (common.h: particle_set_shape; the size query
// applies it and workspace_check passes its refusal on), the workspace.  An empty set is valid for the repulsion entries only.
int64_t dpsx_repulse_workspace_bytes(int64_t n, int64_t chw, int64_t segments)
{
    const int rc = particle_set_shape(n, chw, segments, kRepulseMaxK, true);
    return rc != DPSX_OK ? rc : repulse_workspace_bytes(n, chw, segments);
}

int dpsx_pairwise_sqdist_f32(const float *x, float *d2, float *info, int64_t n, int64_t chw, int64_t segments,
                             void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!x || !d2 || !workspace) return DPSX_EINVAL;
    const int rc = workspace_check(workspace, workspace_bytes, dpsx_repulse_workspace_bytes(n, chw, segments));
    if (rc != DPSX_OK) return rc;
    return repulse(false, 0.0f, 0.0f, x, nullptr, d2, nullptr, info, nullptr, n, chw, segments, workspace,
                   (hipStream_t)stream);
}

int dpsx_repulse_f32(float c, float bandwidth, const float *x, float *out, float *d2, float *w, float *info,
                     uint8_t *applied, int64_t n, int64_t chw, int64_t segments, void *workspace, int64_t workspace_bytes,
                     void *stream)
{
    if (!x || !out || !workspace) return DPSX_EINVAL;
    if (!(c >= 0.0f) || !std::isfinite(c) || !(bandwidth >= 0.0f) || !std::isfinite(bandwidth)) return DPSX_EINVAL;
    const int64_t need = dpsx_repulse_workspace_bytes(n, chw, segments);
    if (need < 0) return (int)need;
    const char *xb = reinterpret_cast<const char *>(x), *ob = reinterpret_cast<const char *>(out);
    const int64_t bytes = n * chw * (int64_t)sizeof(float);
    if (xb < ob + bytes && ob < xb + bytes) return DPSX_EINVAL;       // every particle reads all K: out must not overlap x
    const int rc = workspace_check(workspace, workspace_bytes, need);
    if (rc != DPSX_OK) return rc;
    return repulse(true, c, bandwidth, x, out, d2, w, info, applied, n, chw, segments, workspace, (hipStream_t)stream);
}

// ------------------------------------------------------------------ ensemble statistics (ensemble.hip)
int64_t dpsx_ensemble_workspace_bytes(int64_t n, int64_t d, int64_t images)
{
    const int rc = particle_set_shape(n, d, images, kEnsMaxK, false);
    return rc != DPSX_OK ? rc : ensemble_workspace_bytes(n, d, images);
}

int dpsx_ensemble_ex_f32(const float *x, const float *y, const float *neg_log_w, int64_t count0, float *mean, float *var,
                         float *mean_lo, float *var_lo, float *curve, float *info, int64_t n, int64_t d, int64_t images,
                         void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!x || !mean || !var || !info || !workspace || !mean_lo != !var_lo) return DPSX_EINVAL;
    if (count0 < 0 || (neg_log_w && count0 > 0) || (curve && !y)) return DPSX_EINVAL;
    const int rc = workspace_check(workspace, workspace_bytes, dpsx_ensemble_workspace_bytes(n, d, images));
    if (rc != DPSX_OK) return rc;
    return ensemble(x, y, neg_log_w, count0, mean, var, mean_lo, var_lo, curve, info, n, d, images, workspace,
                    (hipStream_t)stream);
}

int dpsx_ensemble_f32(const float *x, const float *y, const float *neg_log_w, int64_t count0, float *mean, float *var,
                      float *curve, float *info, int64_t n, int64_t d, int64_t images, void *workspace,
                      int64_t workspace_bytes, void *stream)
{
    return dpsx_ensemble_ex_f32(x, y, neg_log_w, count0, mean, var, nullptr, nullptr, curve, info, n, d, images, workspace,
                                workspace_bytes, stream);
}

// ------------------------------------------------------------------ order statistics (quantile.hip)
int64_t dpsx_quantiles_workspace_bytes(int64_t n, int64_t d, int64_t images)
{
    const int rc = particle_set_shape(n, d, images, kQuantMaxK, false);
    return rc != DPSX_OK ? rc : quantiles_workspace_bytes(n, d, images);
}

int dpsx_quantiles_f32(const float *x, const float *y, const double *probs, int64_t q, float *quant, int32_t *hist,
                       float *info, int64_t n, int64_t d, int64_t images, void *workspace, int64_t workspace_bytes,
                       void *stream)
{
    if (!x || !quant || !info || !workspace || !probs || (hist && !y)) return DPSX_EINVAL;
    if (q < 1 || q > kQuantMaxQ) return DPSX_EINVAL;
    for (int64_t i = 0; i < q; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) return DPSX_EINVAL;       // NaN fails both
    const int rc = workspace_check(workspace, workspace_bytes, dpsx_quantiles_workspace_bytes(n, d, images));
    if (rc != DPSX_OK) return rc;
    return quantiles(x, y, probs, q, quant, hist, info, n, d, images, workspace, (hipStream_t)stream);
}

// ------------------------------------------------------------------ principal components (pca.hip)
int64_t dpsx_pca_workspace_bytes(int64_t n, int64_t d, int64_t images)
{
    const int rc = particle_set_shape(n, d, images, kPcaMaxK, false);
    return rc != DPSX_OK ? rc : pca_workspace_bytes(n, d, images);
}

int dpsx_pca_f32(const float *x, int64_t q, float *dirs, float *evals, float *coords, float *info, float *d2, int64_t n,
                 int64_t d, int64_t images, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!x || !dirs || !evals || !coords || !info || !workspace) return DPSX_EINVAL;
    if (q < 1 || q > kPcaMaxQ) return DPSX_EINVAL;
    const int rc = workspace_check(workspace, workspace_bytes, dpsx_pca_workspace_bytes(n, d, images));
    if (rc != DPSX_OK) return rc;
    return pca(x, q, dirs, evals, coords, info, d2, n, d, images, workspace, (hipStream_t)stream);
}

int dpsx_update_f32(const float *sample, const float *g_a, const float *g_b, float *out, int64_t count,
                    void *stream)
{
    if (!sample || !g_a || !out || count < 0) return DPSX_EINVAL;
    return plain_update(sample, g_a, g_b, out, count, (hipStream_t)stream);
}

// ------------------------------------------------------------------ CG data-consistency step
// workspace: [the operator's own workspace | residual-norm partials | rs (x2), pp, tt partials | per-particle scalars |
//             t, r_y (measurement-sized) | r, p, s, d (image-sized)]
struct CgWs {
    void *op_ws;
    int64_t op_bytes;
    float *norm_part, *rs[2], *pp, *tt, *scal, *t, *ry, *r, *p, *s, *d;
};

// carves `base` (nullable: sizes only) and returns the bytes needed, or a negative DPSX_E* code
static int64_t cg_carve(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w, void *base, CgWs *o)
{
    const int64_t op_bytes = dpsx_op_workspace_bytes(op, n, c, h, w), m = meas_elems(op, c, h, w);
    if (op_bytes < 0 || m < 0) return DPSX_EINVAL;
    Carver cv(base);
    CgWs k{};
    k.op_ws = cv.take<char>(op_bytes);
    k.op_bytes = op_bytes;
    for (float **q : {&k.norm_part, &k.rs[0], &k.rs[1], &k.pp, &k.tt}) *q = cv.take<float>(n * 256);
    k.scal = cv.take<float>(n * 4);
    k.t = cv.take<float>(n * m);
    k.ry = cv.take<float>(n * m);
    for (float **q : {&k.r, &k.p, &k.s, &k.d}) *q = cv.take<float>(n * c * h * w);
    if (o) *o = k;
    return cv.bytes();
}

int64_t dpsx_cg_workspace_bytes(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (op->kind == OP_PHASE) return DPSX_EUNSUPPORTED;
    return cg_carve(op, n, c, h, w, nullptr, nullptr);
}

// the refusals both CG entries share, in dpsx_cg_step_f32's order; ptrs: the entry's own pointers are all there
static int cg_check(const dpsx_op *op, bool ptrs, int64_t y_n, float rho, int iters, int64_t n, int64_t c, int64_t h, int64_t w)
{
    const int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (op->kind == OP_PHASE) return DPSX_EUNSUPPORTED;          // no adjoint independent of the point: not a linear solve
    if (!ptrs) return DPSX_EINVAL;
    if (iters < 0 || iters > kCgMaxIters || !(rho >= 0.0f) || !std::isfinite(rho) || !rows_ok(y_n, n)) return DPSX_EINVAL;
    return n > 65535 ? DPSX_EUNSUPPORTED : DPSX_OK;               // particles are the grid's y dimension
}

// How a CG chain ends.  g_mo == NULL: dpsx_cg_step_f32's x_next = sample + kappa d (cg_final); else dpsx_cg_pullback_f32's
// g_mo[:, :e] = inside ? gain d : +0 (cg_pullback).  Everything before the last launch is one chain.
struct CgEnd {
    const float *sample;
    float *x_next;
    float kappa;
    const uint8_t *inside;
    float *g_mo;
    float gain;
};

// the chain of launches of both entries (arguments checked by the caller, n > 0)
static int cg_chain(dpsx_op *op, const float *x0_hat, const float *y, int64_t y_n, float rho, int iters, const CgEnd &end,
                    float *dist, float *d_out, int64_t n, int64_t c, int64_t h, int64_t w, void *workspace,
                    int64_t workspace_bytes, void *stream)
{
    CgWs k;
    int rc = workspace_check(workspace, workspace_bytes, cg_carve(op, n, c, h, w, workspace, &k));
    if (rc != DPSX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t e = c * h * w, m = meas_elems(op, c, h, w);
    // r_y = y - A x0_hat, dist = ||r_y||_2 (the residual-norm path), r = A^T r_y
    if ((rc = dpsx_op_forward_f32(op, x0_hat, k.t, n, c, h, w, k.op_ws, k.op_bytes, stream)) != DPSX_OK) return rc;
    if ((rc = dpsx_residual_norm_f32(y, y_n, k.t, k.ry, dist, n, m, k.norm_part, n * 256 * 4, stream)) != DPSX_OK) return rc;
    if ((rc = dpsx_op_adjoint_f32(op, k.ry, nullptr, k.r, n, c, h, w, k.op_ws, k.op_bytes, stream)) != DPSX_OK) return rc;
    if (iters == 0) {
        if (end.g_mo)                                             // d = 0: the eps half of every particle's row, zeroed
            DPSX_HIP_TRY(hipMemset2DAsync(end.g_mo, (size_t)(2 * e) * 4, 0, (size_t)e * 4, (size_t)n, s));
        else if (end.x_next != end.sample)
            DPSX_HIP_TRY(hipMemcpyAsync(end.x_next, end.sample, (size_t)(n * e) * 4, hipMemcpyDeviceToDevice, s));
        if (d_out) DPSX_HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)(n * e) * 4, s));
        return DPSX_OK;
    }
    if ((rc = cg_init(k.r, k.p, k.rs[0], n, e, s)) != DPSX_OK) return rc;
    float *d = d_out ? d_out : k.d;
    for (int it = 0; it < iters; ++it) {
        const float *rs_old = k.rs[it & 1], *pp = it == 0 ? k.rs[0] : k.pp;       // p = r before the first iteration
        float *rs_new = k.rs[(it + 1) & 1];
        if ((rc = dpsx_op_forward_f32(op, k.p, k.t, n, c, h, w, k.op_ws, k.op_bytes, stream)) != DPSX_OK) return rc;
        if ((rc = dpsx_op_adjoint_f32(op, k.t, nullptr, k.s, n, c, h, w, k.op_ws, k.op_bytes, stream)) != DPSX_OK) return rc;
        if ((rc = cg_sumsq(k.t, k.tt, n, m, s)) != DPSX_OK) return rc;
        if (it == iters - 1) {
            if (end.g_mo)
                return cg_pullback(d, k.p, end.inside, end.g_mo, d_out, rs_old, k.tt, pp, k.scal, rho, end.gain, it == 0, n,
                                   e, m, s);
            return cg_final(end.sample, d, k.p, end.x_next, d_out, rs_old, k.tt, pp, k.scal, rho, end.kappa, it == 0, n, e,
                            m, s);
        }
        if ((rc = cg_update(d, k.p, k.r, k.s, rs_old, k.tt, pp, rs_new, k.scal, rho, it == 0, n, e, m, s)) != DPSX_OK) return rc;
        if ((rc = cg_pupdate(k.r, k.p, rs_old, rs_new, k.pp, k.scal, n, e, s)) != DPSX_OK) return rc;
    }
    return DPSX_OK;
}

int dpsx_cg_step_f32(dpsx_op *op, const float *x0_hat, const float *sample, const float *y, int64_t y_n, float rho,
                     int iters, const dpsx_coefs *coefs_host, float *x_next, float *dist, float *d_out, int64_t n,
                     int64_t c, int64_t h, int64_t w, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int rc = cg_check(op, x0_hat && sample && y && coefs_host && x_next && dist, y_n, rho, iters, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    // the slope of the sampler's `sample` in x0_hat (fp32, in this order): DDPM c1; DDIM c1 - c2 / b
    float kappa = coefs_host->c1;
    if (coefs_host->add_noise & 2) {
        if (coefs_host->b == 0.0f) return DPSX_EINVAL;
        const float q = coefs_host->c2 / coefs_host->b;
        kappa = coefs_host->c1 - q;
    }
    if (n == 0) return DPSX_OK;
    return cg_chain(op, x0_hat, y, y_n, rho, iters, CgEnd{sample, x_next, kappa, nullptr, nullptr, 0.0f}, dist, d_out, n, c, h,
                    w, workspace, workspace_bytes, stream);
}

int dpsx_cg_pullback_f32(dpsx_op *op, const float *x0_hat, const uint8_t *inside, const float *y, int64_t y_n, float rho,
                         int iters, float gain, float *g_model_out, float *dist, float *d_out, int64_t n, int64_t c,
                         int64_t h, int64_t w, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int rc = cg_check(op, x0_hat && inside && y && g_model_out && dist, y_n, rho, iters, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (!std::isfinite(gain)) return DPSX_EINVAL;
    if (n == 0) return DPSX_OK;
    return cg_chain(op, x0_hat, y, y_n, rho, iters, CgEnd{nullptr, nullptr, 0.0f, inside, g_model_out, gain}, dist, d_out, n,
                    c, h, w, workspace, workspace_bytes, stream);
}

// ------------------------------------------------------------------ best-of-N
// Residual partials per block (one launch; two for the operators that materialise A x first), then one small launch
// that finishes costs[p] and, when asked, the combine with the previous costs and the argmin over all particles.
// the scoring launch of one contiguous range of particles (partial sums only; finalize_select finishes them)
static int score_launch(dpsx_op *op, const Ws &ws, const float *x, const float *y, int64_t y_n, int l1, int parts,
                        int64_t n, int64_t c, int64_t h, int64_t w, hipStream_t s)
{
    const int64_t chw = c * h * w;
    int rc;
    switch (op->kind) {
    case OP_SEP:
    case OP_TAPS: return blur_score(op, x, y, y_n, ws.partials, n, c, h, w, l1, s);
    case OP_RESIZE: return resize_score(op, x, y, y_n, ws.partials, n, c, l1, s);
    case OP_IDENT: return residual_partials(y, y_n, x, nullptr, ws.partials, n, chw, parts, s, l1);
    case OP_MASK:      // y - mask * x in the reduction itself (one launch, no scratch)
        return residual_partials(y, y_n, x, nullptr, ws.partials, n, chw, parts, s, l1, op->mask.mask, h * w, op->mask.rows);
    case OP_PHASE: {
        // A x into scratch, then the generic residual reduction
        const int64_t m = meas_elems(op, c, h, w);
        float *ax = ws.meas;
        rc = phase_forward(op, x, ax, nullptr, n * c, ws.priv, ws.priv_bytes, s);
        if (rc != DPSX_OK) return rc;
        return residual_partials(y, y_n, ax, nullptr, ws.partials, n, m, parts, s, l1);
    }
    default: return DPSX_EUNSUPPORTED;
    }
}

static CostArgs cost_args(const Ws &ws, int parts, int l1, const float *prev, int potential, float *raw_out, float *costs,
                          int64_t *best_idx, float *best_val, int64_t n, int64_t chw)
{
    // the reduction is finished by one small follow-up launch (finalize_select), not inside the scoring launch: see
    // the measurement at k_finalize_select
    CostArgs fin{};
    fin.partials = ws.partials;
    fin.parts = parts;
    fin.mode = l1 ? COST_L1SQ : COST_L2;
    fin.l1_scale = (float)(1.0 / (double)chw);
    fin.prev = prev;
    fin.potential = potential;
    fin.raw_out = raw_out;
    fin.out = costs;
    fin.best_idx = best_idx;
    fin.best_val = best_val;
    fin.n = (int)n;
    return fin;
}

static int score_impl(dpsx_op *op, const float *x, const float *y, int64_t y_n, int l1, const float *prev,
                      int potential, float *raw_out, float *costs, int64_t *best_idx, float *best_val, int64_t n,
                      int64_t c, int64_t h, int64_t w, void *workspace, int64_t workspace_bytes, void *stream)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (!x || !y || !costs || !rows_ok(y_n, n)) return DPSX_EINVAL;
    if (n == 0) return best_idx ? DPSX_EINVAL : DPSX_OK;
    Ws ws;
    if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int parts = score_parts(op, c, h, w);
    if ((rc = score_launch(op, ws, x, y, y_n, l1, parts, n, c, h, w, s)) != DPSX_OK) return rc;
    return finalize_select(cost_args(ws, parts, l1, prev, potential, raw_out, costs, best_idx, best_val, n, c * h * w), 1, s);
}

// ------------------------------------------------------------------ the search_ddpm step
// The one argument check of the search step.  segments == 0: unsegmented (y rows as everywhere else); segments >= 1: a
// multi-image batch of `segments` images x n / segments particles, y holds one row (broadcast) or one per image.
static int search_seg_args(const dpsx_op *op, const float *x_t, const float *model_out, const void *noise, const float *y,
                           int64_t y_n, const float *sample, const float *costs, const int64_t *best_idx_dev,
                           const float *x_next, int64_t segments, bool one_state, int64_t n, int64_t c, int64_t h,
                           int64_t w, const dpsx_coefs *coefs_host)
{
    int rc = check_geom(op, n, c, h, w);
    if (rc != DPSX_OK) return rc;
    if (!x_t || !model_out || !y || !sample || !costs || !best_idx_dev || !coefs_host) return DPSX_EINVAL;
    if ((coefs_host->add_noise & 1) && !noise) return DPSX_EINVAL;
    if (n == 0 || segments < 0) return DPSX_EINVAL;
    if (segments ? n % segments != 0 || (y_n != 1 && y_n != segments) : !rows_ok(y_n, n)) return DPSX_EINVAL;
    // dpsx_search_step_f32 alone accepts x_next == x_t (the replication runs after S1 has read every state)
    if (x_next == sample || (x_next == x_t && (segments || one_state))) return DPSX_EINVAL;
    return DPSX_OK;
}

// All six exported search steps.  noise / rng: the source of S1's noise (rng != NULL: drawn inside S1's launch, noise is
// then NULL).  segments: 0 = one particle set; M >= 1 = M images of n / M particles, the select runs per image and
// best_idx_dev / best_val_dev are [M].  one_state: x_t / model_out hold ONE state per image instead of one per particle.
// beam >= 1 (the beam step, with one_state): x_t / model_out hold `states` states, n / states consecutive proposals each,
// and the select keeps the first `beam` particles of every image: best_idx_dev / best_val_dev and x_next are [M beam].
static int search_step_impl(dpsx_op *op, const float *x_t, const float *model_out, const float *noise, const dpsx_rng *rng,
                            const float *y, int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev,
                            float *best_val_dev, float *x_next, int64_t segments, bool one_state, int64_t n, int64_t c,
                            int64_t h, int64_t w, const dpsx_coefs *coefs_host, void *workspace, int64_t workspace_bytes,
                            void *stream, int64_t states = 0, int64_t beam = 0)
{
    int rc = search_seg_args(op, x_t, model_out, rng ? (const void *)rng : (const void *)noise, y, y_n, sample, costs,
                             best_idx_dev, x_next, segments, one_state, n, c, h, w, coefs_host);
    if (rc != DPSX_OK) return rc;
    if (beam) {
        if (segments < 1 || states < 1 || n % states != 0 || states % segments != 0 || beam < 1 || beam > n / segments)
            return DPSX_EINVAL;
        if (n / segments > kTopbMaxK || segments > (1 << 24)) return DPSX_EUNSUPPORTED;
    }
    RngK rk{};
    if (rng && (rc = to_rngk(rng, n, rk)) != DPSX_OK) return rc;
    // S1 (no x0_hat store) -> scoring launch -> one launch for costs + select -> the winner's replication.
    // Measured and dropped (N = 64, Gaussian, 89.7 us for this sequence): S1 fused into the separable scoring kernel (the
    // proposal's halo needs all four input streams: 72 us for the fused launch against 37 + 30 for the two); costs +
    // select + replication in one launch (92.5 us per step); the particles in 2 / 3 / 4 chunks with the (latency-bound)
    // scoring of chunk k on a second stream beside the (bandwidth-bound) S1 of chunk k + 1, forked and joined by events:
    // 94.8 / 100.8 / 113.6 us -- the cross-stream dependencies cost more than the overlap returns.
    // one_state: after a select every particle of SearchDDPM is a copy of the winner (img[best_path.repeat(n_paths)],
    // :633), so the loop's state is ONE particle per image: S1 reads that state and its model output once for all its
    // proposals (proposal p reads state p / (n / images); the per-particle noise makes them differ), the scoring launch
    // and the select are the n-particle ones, and each winner is copied out once instead of n / images times: 3P of
    // traffic per particle-step (noise in, proposal out, proposal scored) instead of the 8P of the replicated form --
    // and one model evaluation per step instead of n for the caller.
    Ws ws;
    if ((rc = carve(op, workspace, workspace_bytes, n, c, h, w, ws)) != DPSX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t chw = c * h * w;
    const int64_t images = std::max<int64_t>(segments, 1);
    const int parts = score_parts(op, c, h, w);
    rc = posterior_fwd(x_t, model_out, noise, rng != nullptr, rk, nullptr, sample, nullptr, n, chw, to_coefs(coefs_host), s,
                       one_state, beam ? states : images);
    if (rc != DPSX_OK) return rc;
    if ((rc = score_launch(op, ws, sample, y, y_n, 0, parts, n, c, h, w, s)) != DPSX_OK) return rc;
    const CostArgs fin = cost_args(ws, parts, 0, nullptr, POT_NONE, nullptr, costs, best_idx_dev, best_val_dev, n, chw);
    if (beam) {       // costs + the top-`beam` select per image: one launch; the winners' copies: one more (DESIGN.md "beam search")
        rc = finalize_topb(fin, (int)images, (int)beam, s);
        if (rc != DPSX_OK || !x_next) return rc;
        return gather_f32(sample, best_idx_dev, x_next, images * beam, n, chw, s);
    }
    static const bool unfused = getenv("DPSX_SEARCH_ONE_UNFUSED") != nullptr;       // A/B switch for tools/kbench_search.py
    if (one_state && !unfused && x_next && vec_ok(chw, {sample, x_next}))
        return finalize_select_copy(fin, (int)images, sample, x_next, chw, s);   // costs + select + the winners' copies: one launch
    rc = finalize_select(fin, (int)images, s);
    if (rc != DPSX_OK || !x_next) return rc;
    if (one_state) return gather_f32(sample, best_idx_dev, x_next, images, n, chw, s);
    return replicate_seg_f32(sample, best_idx_dev, x_next, n, n / images, n, chw, s);
}

int dpsx_search_step_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise, const float *y,
                         int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev, float *best_val_dev,
                         float *x_next, int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                         void *workspace, int64_t workspace_bytes, void *stream)
{
    return search_step_impl(op, x_t, model_out, noise, nullptr, y, y_n, sample, costs, best_idx_dev, best_val_dev, x_next,
                            0, false, n, c, h, w, coefs_host, workspace, workspace_bytes, stream);
}

int dpsx_search_step_one_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise, const float *y,
                             int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev, float *best_val_dev,
                             float *x_next, int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                             void *workspace, int64_t workspace_bytes, void *stream)
{
    return search_step_impl(op, x_t, model_out, noise, nullptr, y, y_n, sample, costs, best_idx_dev, best_val_dev, x_next,
                            0, true, n, c, h, w, coefs_host, workspace, workspace_bytes, stream);
}

// multi-image forms (segments of n / segments particles): a segment count below 1 is refused here, 0 being the
// unsegmented step of the shared body
int dpsx_search_step_seg_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise, const float *y,
                             int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev, float *best_val_dev,
                             float *x_next, int64_t segments, int64_t n, int64_t c, int64_t h, int64_t w,
                             const dpsx_coefs *coefs_host, void *workspace, int64_t workspace_bytes, void *stream)
{
    return search_step_impl(op, x_t, model_out, noise, nullptr, y, y_n, sample, costs, best_idx_dev, best_val_dev, x_next,
                            segments < 1 ? -1 : segments, false, n, c, h, w, coefs_host, workspace, workspace_bytes, stream);
}

int dpsx_search_step_seg_rng_f32(dpsx_op *op, const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                                 const float *y, int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev,
                                 float *best_val_dev, float *x_next, int64_t segments, int64_t n, int64_t c, int64_t h,
                                 int64_t w, const dpsx_coefs *coefs_host, void *workspace, int64_t workspace_bytes,
                                 void *stream)
{
    if (!rng_host) return DPSX_EINVAL;
    return search_step_impl(op, x_t, model_out, nullptr, rng_host, y, y_n, sample, costs, best_idx_dev, best_val_dev,
                            x_next, segments < 1 ? -1 : segments, false, n, c, h, w, coefs_host, workspace,
                            workspace_bytes, stream);
}

int dpsx_search_step_one_seg_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                                 const float *y, int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev,
                                 float *best_val_dev, float *x_next, int64_t segments, int64_t n, int64_t c, int64_t h,
                                 int64_t w, const dpsx_coefs *coefs_host, void *workspace, int64_t workspace_bytes,
                                 void *stream)
{
    return search_step_impl(op, x_t, model_out, noise, nullptr, y, y_n, sample, costs, best_idx_dev, best_val_dev, x_next,
                            segments < 1 ? -1 : segments, true, n, c, h, w, coefs_host, workspace, workspace_bytes, stream);
}

int dpsx_search_step_one_seg_rng_f32(dpsx_op *op, const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                                     const float *y, int64_t y_n, float *sample, float *costs, int64_t *best_idx_dev,
                                     float *best_val_dev, float *x_next, int64_t segments, int64_t n, int64_t c,
                                     int64_t h, int64_t w, const dpsx_coefs *coefs_host, void *workspace,
                                     int64_t workspace_bytes, void *stream)
{
    if (!rng_host) return DPSX_EINVAL;
    return search_step_impl(op, x_t, model_out, nullptr, rng_host, y, y_n, sample, costs, best_idx_dev, best_val_dev,
                            x_next, segments < 1 ? -1 : segments, true, n, c, h, w, coefs_host, workspace, workspace_bytes,
                            stream);
}

int dpsx_search_step_beam_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                              const dpsx_rng *rng_host, const float *y, int64_t y_n, float *sample, float *costs,
                              int64_t *best_idx_dev, float *best_val_dev, float *x_next, int64_t segments, int64_t states,
                              int64_t beam, int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                              void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!coefs_host || ((coefs_host->add_noise & 1) && (noise != nullptr) == (rng_host != nullptr))) return DPSX_EINVAL;
    if (segments < 1 || beam < 1) return DPSX_EINVAL;
    return search_step_impl(op, x_t, model_out, rng_host ? nullptr : noise, rng_host, y, y_n, sample, costs, best_idx_dev,
                            best_val_dev, x_next, segments, true, n, c, h, w, coefs_host, workspace, workspace_bytes, stream,
                            states, beam);
}

int dpsx_score_f32(dpsx_op *op, const float *x, const float *y, int64_t y_n, float *costs, int64_t n, int64_t c,
                   int64_t h, int64_t w, void *workspace, int64_t workspace_bytes, void *stream)
{
    return score_impl(op, x, y, y_n, 0, nullptr, POT_NONE, nullptr, costs, nullptr, nullptr, n, c, h, w, workspace,
                      workspace_bytes, stream);
}

int dpsx_score_argmin_f32(dpsx_op *op, const float *x, const float *y, int64_t y_n, float *costs,
                          int64_t *best_idx_dev, float *best_val_dev, int64_t n, int64_t c, int64_t h, int64_t w,
                          void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!best_idx_dev) return DPSX_EINVAL;
    return score_impl(op, x, y, y_n, 0, nullptr, POT_NONE, nullptr, costs, best_idx_dev, best_val_dev, n, c, h, w,
                      workspace, workspace_bytes, stream);
}

int dpsx_resample_cost_f32(dpsx_op *op, const float *x, const float *y, int64_t y_n, const float *prev_costs,
                           int potential, float *curr_costs, float *net_costs, int64_t n, int64_t c, int64_t h,
                           int64_t w, void *workspace, int64_t workspace_bytes, void *stream)
{
    if (potential < DPSX_POT_MEAN || potential > DPSX_POT_CURR) return DPSX_EINVAL;
    return score_impl(op, x, y, y_n, 1, prev_costs, potential, curr_costs, net_costs, nullptr, nullptr, n, c, h, w,
                      workspace, workspace_bytes, stream);
}

int dpsx_argmin_f32(const float *v, int64_t n, int64_t *idx_out_dev, float *val_out_dev, void *stream)
{
    if (!v || !idx_out_dev || n < 1) return DPSX_EINVAL;
    return argmin_seg_f32(v, 1, n, idx_out_dev, val_out_dev, (hipStream_t)stream);
}

int dpsx_argmin_seg_f32(const float *v, int64_t segments, int64_t k, int64_t *idx_out_dev, float *val_out_dev,
                        void *stream)
{
    if (!v || !idx_out_dev || segments < 1 || segments > (1 << 24) || k < 1) return DPSX_EINVAL;
    return argmin_seg_f32(v, segments, k, idx_out_dev, val_out_dev, (hipStream_t)stream);
}

int dpsx_topk_seg_f32(const float *v, int64_t segments, int64_t k, int64_t b, int64_t *idx_out_dev, float *val_out_dev,
                      void *stream)
{
    if (!v || !idx_out_dev || segments < 1 || k < 1 || b < 1 || b > k) return DPSX_EINVAL;
    if (k > kTopbMaxK || segments > (1 << 24)) return DPSX_EUNSUPPORTED;
    return topk_seg_f32(v, segments, k, b, idx_out_dev, val_out_dev, (hipStream_t)stream);
}

int dpsx_gather_f32(const float *src, const int64_t *ids_dev, float *dst, int64_t n_out, int64_t n_src,
                    int64_t chw, void *stream)
{
    if (n_out < 0 || chw < 0) return DPSX_EINVAL;
    if (n_out == 0 || chw == 0) return DPSX_OK;
    if (!src || !ids_dev || !dst || n_src < 1 || src == dst) return DPSX_EINVAL;
    return gather_f32(src, ids_dev, dst, n_out, n_src, chw, (hipStream_t)stream);
}

int dpsx_replicate_f32(const float *src, const int64_t *idx_dev, float *dst, int64_t n_out, int64_t n_src,
                       int64_t chw, void *stream)
{
    if (n_out < 0 || chw < 0) return DPSX_EINVAL;
    if (n_out == 0 || chw == 0) return DPSX_OK;
    if (!src || !idx_dev || !dst || n_src < 1 || src == dst) return DPSX_EINVAL;
    return replicate_seg_f32(src, idx_dev, dst, n_out, n_out, n_src, chw, (hipStream_t)stream);     // one id for all rows
}

// The four resampling entry points: !fused is the draw alone (src .. chw unused), opts == nullptr the plain form.  The checks
// run in a fixed order (a call that is wrong in several ways keeps its code): the draw's arguments, the fused form's
// gathers, then the scheme and the trigger.
static int resample_entry(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale, bool fused,
                          const float *src, float *dst, float *d_out, int64_t *ids, int32_t *q_out, int64_t n, int64_t chw,
                          const ResampleOpts *opts, void *stream)
{
    if (!d || !u || !ids || segments < 1 || k < 1 || !(inv_scale >= 0.0f) || inv_scale > 3.402823466e38f)
        return DPSX_EINVAL;
    if (k > kResampleMaxK || segments > (1 << 24)) return DPSX_EUNSUPPORTED;       // the CDF of a segment lives in 8 k bytes of LDS
    if (fused) {
        if (!src || !dst || !d_out || n != segments * k || chw < 1) return DPSX_EINVAL;
        // the gather reads whole particles of src while other blocks write dst: no overlap of the two ranges, and the
        // distances are read by every block while one of them writes d_out
        const char *sb = reinterpret_cast<const char *>(src), *db = reinterpret_cast<const char *>(dst);
        const int64_t bytes = n * chw * (int64_t)sizeof(float);
        if (sb < db + bytes && db < sb + bytes) return DPSX_EINVAL;
        if (d_out < d + n && d < d_out + n) return DPSX_EINVAL;
        if (n > 65535) return DPSX_EUNSUPPORTED;                              // one grid row per destination particle
    }
    if (opts && !(opts->scheme >= DPSX_RESAMPLE_MULTINOMIAL && opts->scheme <= DPSX_RESAMPLE_SYSTEMATIC &&
                  opts->ess_q16 >= 0 && opts->ess_q16 <= 65536))
        return DPSX_EINVAL;
    if (!fused) return resample_draw_seg(d, u, segments, k, inv_scale, ids, q_out, opts, (hipStream_t)stream);
    return resample_seg(d, u, segments, k, inv_scale, src, dst, d_out, ids, q_out, chw, opts, (hipStream_t)stream);
}

int dpsx_resample_draw_seg_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                               int64_t *ids_out, int32_t *q_out, void *stream)
{
    return resample_entry(d, u, segments, k, inv_scale, false, nullptr, nullptr, nullptr, ids_out, q_out, 0, 0, nullptr, stream);
}

int dpsx_resample_seg_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                          const float *src, float *dst, float *d_out, int64_t *ids_out, int32_t *q_out,
                          int64_t n, int64_t chw, void *stream)
{
    return resample_entry(d, u, segments, k, inv_scale, true, src, dst, d_out, ids_out, q_out, n, chw, nullptr, stream);
}

int dpsx_resample_draw_seg_ex_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                                  int64_t *ids_out, int32_t *q_out, int scheme, int32_t ess_q16,
                                  uint8_t *resampled_out, float *ess_out, void *stream)
{
    const ResampleOpts opts{scheme, ess_q16, resampled_out, ess_out};
    return resample_entry(d, u, segments, k, inv_scale, false, nullptr, nullptr, nullptr, ids_out, q_out, 0, 0, &opts, stream);
}

int dpsx_resample_seg_ex_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                             const float *src, float *dst, float *d_out, int64_t *ids_out, int32_t *q_out,
                             int64_t n, int64_t chw, int scheme, int32_t ess_q16, uint8_t *resampled_out,
                             float *ess_out, void *stream)
{
    const ResampleOpts opts{scheme, ess_q16, resampled_out, ess_out};
    return resample_entry(d, u, segments, k, inv_scale, true, src, dst, d_out, ids_out, q_out, n, chw, &opts, stream);
}

int dpsx_pack_champion_f32(const float *particles, const float *costs, const int64_t *best_idx_dev,
                           const float *best_val_dev, float *out, int64_t n, int64_t chw, void *stream)
{
    if (!particles || !out || n < 1 || chw < 4 || chw % 4 != 0) return DPSX_EINVAL;
    if (!best_idx_dev && !costs) return DPSX_EINVAL;
    if (best_idx_dev && !best_val_dev && !costs) return DPSX_EINVAL;
    if (!aligned16(particles) || !aligned16(out)) return DPSX_EUNSUPPORTED;
    return pack_champion(particles, costs, best_idx_dev, best_val_dev, out, n, chw, (hipStream_t)stream);
}

int dpsx_select_champion_f32(const float *table, int64_t world, int64_t chw, float *dst, int64_t n_out,
                             int64_t *win_rank_dev, int64_t *win_local_dev, void *stream)
{
    if (!table || !dst || world < 1 || world > (1 << 20) || chw < 4 || chw % 4 != 0 || n_out < 1) return DPSX_EINVAL;
    if (!aligned16(table) || !aligned16(dst)) return DPSX_EUNSUPPORTED;
    return select_champion(table, (int)world, chw, dst, n_out, win_rank_dev, win_local_dev, (hipStream_t)stream);
}

}  // extern "C"
#pragma GCC visibility pop
