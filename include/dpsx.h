/* dpsx -- C ABI of the MI355X (gfx950) DPS test-time-compute hot path.
 *
 * Drop-in boundary for vishnutez/dps-ttc.  The reference is pure Python and has
 * no FFI of its own; each entry point below names the reference function
 * (file:line under /root/reference) whose device work it replaces, and
 * INTEGRATION.md shows the ctypes binding a maintainer adds on the reference
 * side.  Conventions:
 *   - every pointer is a DEVICE pointer to contiguous fp32 (NCHW) unless the
 *     name ends in _host; the caller owns all buffers;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*),
 *     does no allocation and no host sync (graph-capturable);
 *   - a dpsx_op serves ONE stream at a time: its workspace (caller-provided, sized by
 *     dpsx_op_workspace_bytes) carries the per-tile partial sums from dpsx_step_fwd_f32 to
 *     dpsx_step_bwd_f32, and its arrival counters belong to the launch in flight.  Calls on
 *     one op must be stream-ordered; concurrency is across ops (one op + workspace per
 *     stream -- kernels.ParticleGroups does exactly that).  Calls that take no op are
 *     re-entrant;
 *   - return value: DPSX_OK or a negative DPSX_E* code; nothing throws/exits;
 *   - `n` = particles, `c` = channels, `h`,`w` = image size, chw = c*h*w;
 *   - a measurement `y` is [y_n, ...] with y_n dividing n: particle p reads row p / (n / y_n).  y_n = 1
 *     broadcasts one measurement, y_n = n gives one per particle, and y_n = M serves a multi-image batch of
 *     M images x n / M particles in image-major order (particles [m K, (m + 1) K) belong to image m).
 *
 * Buffer placement.  An fp32 (or int32) buffer needs 4-byte alignment, an int64 buffer 8, the byte gate `inside` and the
 * other uint8 buffers none; a workspace needs 16.  Every launcher runs its 16-byte (float4) form where the size allows it
 * and every buffer of the call is 16-byte aligned (`inside`: 4), else a scalar form: results agree within the bounds
 * stated per entry point -- bit for bit where the entry says so or computes each output element on its own (S1, the
 * normals, the updates' x_next, gather / replicate, selects and resampling ids); a sum whose lanes own float4 units adds
 * its terms in another order than the scalar form -- and no call writes outside the buffers as sized here, whichever form
 * runs.  The exceptions, each returned before anything is launched or written:
 *   - DPSX_EWORKSPACE: a workspace off the 16-byte grid or shorter than its query, from every call that uses one
 *     (dpsx_op_forward_f32 uses it for phase retrieval only, dpsx_op_adjoint_f32 for the blurs and phase retrieval; the
 *     other operators ignore the two arguments there).  A NULL workspace is the same code from the operator, CG and
 *     residual-norm entries and DPSX_EINVAL from the analysis entries, as each of them states.
 *     dpsx_residual_norm_f32 has no query: its workspace holds min(256, max(1, ceil(m / 4096))) fp32 partial sums per
 *     particle (n * 256 * 4 bytes always suffice) and needs 4-byte alignment only.
 *   - DPSX_EUNSUPPORTED from the fused step of an inpainting operator (16-byte form only): dpsx_step_fwd_f32 / _rng with
 *     x_t, model_out, noise, y, x0_hat or sample off the 16-byte grid or `inside` off the 4-byte grid; dpsx_step_bwd_f32 /
 *     _extra with x0_hat, y, g_model_out, g_x0_extra or `inside` so.
 *   - DPSX_EUNSUPPORTED from the fused step of a phase-retrieval operator: `resid` off the 16-byte grid (it is the
 *     transforms' own buffer: complex words); at the hand-written 384-point geometry also x_t, model_out, noise, x0_hat,
 *     sample (forward) or g_model_out, g_x0_extra (backward) off the 16-byte grid, or `inside` off the 4-byte grid.
 *   - DPSX_EUNSUPPORTED from dpsx_step_fwd_rng_f32 of a blur or resize operator with a buffer off the grid: the draw
 *     inside the launch exists in the 16-byte form (see dpsx_step_draws_in_kernel); the caller fills a noise buffer.
 *   - DPSX_EUNSUPPORTED from dpsx_pack_champion_f32 (particles, out) and dpsx_select_champion_f32 (table, dst).
 * The size queries (dpsx_op_workspace_bytes, dpsx_step_resid_bytes, dpsx_cg_workspace_bytes, dpsx_*_workspace_bytes)
 * know no pointer: a workspace of the queried size serves every placement of the other buffers.
 */
#ifndef DPSX_H
#define DPSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPSX_ABI_VERSION 3

enum {
    DPSX_OK = 0,
    DPSX_EINVAL = -1,     /* null pointer / bad size / bad enum */
    DPSX_EUNSUPPORTED = -2,
    DPSX_ELAUNCH = -3,    /* HIP reported a launch/runtime error */
    DPSX_ENOMEM = -4,
    DPSX_EWORKSPACE = -5  /* caller workspace too small or off the 16-byte grid */
};

int dpsx_abi_version(void);
const char *dpsx_strerror(int code);
/* last HIP error string seen by this thread (for DPSX_ELAUNCH / DPSX_ENOMEM) */
const char *dpsx_last_hip_error(void);

/* ---- per-step scalars -----------------------------------------------------
 * The six fp32 table entries one DDPM step reads, replacing eight
 * extract_and_expand() H2D copies per step (gaussian_diffusion.py:769-773,
 * posterior_mean_variance.py:116-117, 121-122, 235-236). */
typedef struct dpsx_coefs {
    float a;        /* sqrt_recip_alphas_cumprod[t]    posterior_mean_variance.py:121 */
    float b;        /* sqrt_recipm1_alphas_cumprod[t]  :122 */
    float c1;       /* posterior_mean_coef1[t]         :116 */
    float c2;       /* posterior_mean_coef2[t]         :117 */
    float min_log;  /* posterior_log_variance_clipped[t]  :235 */
    float max_log;  /* log(betas[t])                   :236 */
    int32_t add_noise; /* bit 0: t != 0 (add the noise term)  gaussian_diffusion.py:473, :503
                        * bit 1: DDIM step instead of DDPM (DDIM.p_sample, gaussian_diffusion.py:481-509); the
                        *        record then carries c1 = sqrt(alphas_cumprod_prev[t]),
                        *        c2 = sqrt(1 - alphas_cumprod_prev[t] - sigma^2), min_log = sigma (eta-scaled, :487-491),
                        *        max_log unused; a, b as above (also predict_eps_from_x_start, :506-509).
                        *        The variance channels of model_out are then not read. */
} dpsx_coefs;

/* ---- S1: p_mean_variance + DDPM.p_sample ----------------------------------
 * gaussian_diffusion.py:308-330, 466-476; posterior_mean_variance.py:96-129
 * (epsilon), :40-45 (clip), :211-242 (learned_range).
 * model_out is [n, 2c, h, w] (eps | v).  x0_hat, sample: [n, c, h, w].
 * inside (optional, may be NULL): uint8 [n*chw], 1 where the pre-clamp value
 * lies in [-1, 1] (the set on which torch's clamp passes gradient). */
int dpsx_posterior_fwd_f32(const float *x_t, const float *model_out, const float *noise,
                           float *x0_hat, float *sample, uint8_t *inside,
                           int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream);

/* VJP of the above, as torch.autograd.grad walks it (condition_methods.py:48,185).
 * g_x0 / g_sample may be NULL (zero cotangent).  g_model_out is [n, 2c, h, w]. */
int dpsx_posterior_bwd_f32(const float *g_x0, const float *g_sample, const float *x_t,
                           const float *model_out, const float *noise,
                           float *g_x, float *g_model_out,
                           int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream);

/* ---- measurement operators A (measurements.py) ---------------------------- */
typedef struct dpsx_op dpsx_op; /* opaque; owns only its constant tables */

/* DPSX_BLUR_AUTO: a kernel K that is rank 1 takes the separable path.  With col = K[:, pj] and
 * row = K[pi, :] / K[pi, pj] through the tap of largest magnitude (pi, pj), both rounded to fp32,
 * K counts as rank 1 when   sum |col[i] row[j] - K[i][j]| <= 1e-6 * sum |K[i][j]|   (evaluated in
 * double): the separable operator then differs from the given one by at most 1e-6 max|x| per
 * output pixel, relative to an operator of gain sum |K|.  Every other kernel, and every kernel
 * under DPSX_BLUR_FORCE_TAPS, runs as the list of its non-zero taps. */
enum { DPSX_BLUR_AUTO = 0, DPSX_BLUR_FORCE_TAPS = 1 };

/* GaussialBlurOperator / MotionBlurOperator: ReflectionPad2d(ks/2) + depthwise
 * cross-correlation, same ks x ks kernel on every channel
 * (measurements.py:93-149, util/img_utils.py:268-308).  kernel_host: ks*ks fp32,
 * row-major, HOST memory.  Rank-1 kernels take the separable LDS path unless
 * mode == DPSX_BLUR_FORCE_TAPS. */
int dpsx_op_create_blur(const float *kernel_host, int ks, int mode, dpsx_op **out);

/* SuperResolutionOperator -> Resizer (measurements.py:76-91, util/resizer.py:55-74).
 * w_*_host [taps_*, out_*] fp32 and i_*_host [taps_*, out_*] int64 are
 * Resizer.weights / Resizer.field_of_view for the H and W axes. */
int dpsx_op_create_resize(int64_t in_h, int64_t in_w,
                          const float *w_h_host, const int64_t *i_h_host, int64_t taps_h, int64_t out_h,
                          const float *w_w_host, const int64_t *i_w_host, int64_t taps_w, int64_t out_w,
                          dpsx_op **out);

/* InpaintingOperator (measurements.py:151-168): mask_dev is a DEVICE pointer to
 * h*w fp32 ([1,1,h,w], broadcast over n and c); borrowed, must outlive the op. */
int dpsx_op_create_mask(const float *mask_dev, int64_t h, int64_t w, dpsx_op **out);
/* The same with one mask per image (sample_condition_batched_data.py:131-190 draws a mask per image):
 * mask_dev is [mask_n, h, w] and particle p of n uses mask p / (n / mask_n).  Calls with an n that mask_n
 * does not divide return DPSX_EINVAL. */
int dpsx_op_create_mask_n(const float *mask_dev, int64_t mask_n, int64_t h, int64_t w, dpsx_op **out);

/* DenoiseOperator (measurements.py:57-73): identity. */
int dpsx_op_create_identity(dpsx_op **out);

/* PhaseRetrievalOperator (measurements.py:179-189 -> util/img_utils.py:26-30 ->
 * util/fastmri_utils.py:67-89): zero-pad by `pad`, centred orthonormal 2-D FFT,
 * modulus.  Square images of side h; plans are built for up to max_planes = n*c. */
int dpsx_op_create_phase(int64_t h, int64_t pad, int64_t max_planes, dpsx_op **out);

void dpsx_op_destroy(dpsx_op *op);
/* measurement shape for an [*, *, h, w] input */
int dpsx_op_out_shape(const dpsx_op *op, int64_t h, int64_t w, int64_t *out_h, int64_t *out_w);
/* 0 generic taps, 1 separable, 2 resize, 3 mask, 4 identity, 5 phase */
int dpsx_op_kind(const dpsx_op *op);
/* bytes of scratch the op-level and step-level calls below need for n particles */
int64_t dpsx_op_workspace_bytes(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w);

/* operator.forward(data)  (measurements.py:84,108,142,158,186) */
int dpsx_op_forward_f32(dpsx_op *op, const float *x, float *y,
                        int64_t n, int64_t c, int64_t h, int64_t w,
                        void *workspace, int64_t workspace_bytes, void *stream);
/* exact VJP of operator.forward (what autograd computes for condition_methods.py:48,185).
 * Linear ops ignore x; phase retrieval differentiates at x (re-runs the forward FFT). */
int dpsx_op_adjoint_f32(dpsx_op *op, const float *u, const float *x, float *g,
                        int64_t n, int64_t c, int64_t h, int64_t w,
                        void *workspace, int64_t workspace_bytes, void *stream);

/* ---- residual norm (condition_methods.py:37-39, 179-181; gaussian_diffusion.py:627-630)
 * r = y - ax (y has y_n rows, y_n dividing n); norm[p] = ||r_p||_2.  Deterministic
 * two-pass reduction (no float atomics).  r may be NULL. */
int dpsx_residual_norm_f32(const float *y, int64_t y_n, const float *ax, float *r, float *norm,
                           int64_t n, int64_t m, void *workspace, int64_t workspace_bytes, void *stream);
/* cotangent on ax of sum_p g_norm[p] * norm_p^power, power in {1, 2}; 0 where norm == 0 */
int dpsx_norm_bwd_f32(const float *r, const float *norm, const float *g_norm, int power,
                      float *g_ax, int64_t n, int64_t m, void *stream);

/* ---- fused DPS step (gaussian_diffusion.py:207-257 + condition_methods.py:33-60,
 *      94-106, 145-187, 198-212), three launches per step:
 *  fwd : S1 + A(x0_hat) + residual + norm   -> x0_hat, sample, inside, resid, norm
 *  bwd : cotangent of scale*norm^power back through A and the clamp to the UNet
 *        output: g_model_out[:, :c] = -b * g_pre,  g_model_out[:, c:] untouched
 *        (the caller zeroes that half once), where g_pre = dLoss/d(pre-clamp x0)
 *  upd : x_{t-1} = sample - (a * g_pre + g_unet)   with a*g_pre = (-a/b) * g_eps
 * `resid` is an op-defined scratch of dpsx_step_resid_bytes() bytes that carries
 * the residual (or, for phase retrieval, the complex cotangent) from fwd to bwd. */
int64_t dpsx_step_resid_bytes(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w);

/* norm != NULL: the launch finishes the per-particle norms itself (each particle's last block re-sums the partials
 * in a fixed order: deterministic, no extra launch).  norm == NULL: they are finalised by dpsx_step_bwd_f32's
 * prologue from the partial sums left in `workspace` (see there).
 * x0_hat == NULL (blur and resize operators, phase retrieval at the hand-written 384-point geometry): pred_xstart is consumed inside the launch -- A(x0_hat), the clamp gate --
 * and not written out; the `ps` step reads it nowhere afterwards (posterior_mean_variance.py:96-129 returns it to
 * condition_methods.py:33-60, which uses it for the norm only).  The other operators read it back and require it.
 * DPSX_EUNSUPPORTED (here and from dpsx_step_bwd_f32, before anything is launched): an inpainting op whose H * W is not
 * a multiple of 4, or whose buffers are not 16-byte aligned -- that step exists in its float4 form only.  The caller runs
 * such a step from the per-op calls instead (dpsx_posterior_fwd_f32, dpsx_op_forward_f32, dpsx_residual_norm_f32 and
 * their VJPs); the Python front end decides this from the shape before its loop starts (OpHandle.fuses_step). */
int dpsx_step_fwd_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                      const float *y, int64_t y_n,
                      float *x0_hat, float *sample, uint8_t *inside, void *resid, float *norm,
                      int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* norm: the norms dpsx_step_fwd_f32 produced, or NULL when that call was given norm == NULL: the partial sums
 * it left in `workspace` (same buffer, untouched in between) are then finalised in this launch's prologue --
 * saving a launch per step -- and written to norm_out (required in that case, optional otherwise). */
int dpsx_step_bwd_f32(dpsx_op *op, const void *resid, const float *norm, float *norm_out, const uint8_t *inside,
                      const float *x0_hat, const float *y, int64_t y_n,
                      float scale, int power, float *g_model_out,
                      int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                      void *workspace, int64_t workspace_bytes, void *stream);

/* The same launch with one more cotangent on x0_hat: g_x0_extra [n, c, h, w] (NULL = none) is added to
 * coef * A^T r before the clamp gate and the -b scaling.  It carries the gradient of any further loss term that
 * depends on x0_hat only -- the semantic-guidance term of PosteriorSamplingSemanticGuid.measurement_semantic_guidance
 * (condition_methods.py:155-187: sem_guid_scale_t * ||emb(x0_hat) - emb_ref||^p, its VJP taken by the caller
 * through the pluggable embedder) -- so that configuration also runs on the three fused launches. */
int dpsx_step_bwd_extra_f32(dpsx_op *op, const void *resid, const float *norm, float *norm_out,
                            const uint8_t *inside, const float *x0_hat, const float *y, int64_t y_n,
                            float scale, int power, const float *g_x0_extra, float *g_model_out,
                            int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                            void *workspace, int64_t workspace_bytes, void *stream);

int dpsx_step_update_f32(const float *sample, const float *g_model_out, const float *g_unet,
                         float *x_next, int64_t n, int64_t chw, const dpsx_coefs *coefs_host,
                         void *stream);

/* plain x_{t-1} = sample - (g_a + g_b)   (g_b may be NULL)  gaussian_diffusion.py:255 */
int dpsx_update_f32(const float *sample, const float *g_a, const float *g_b, float *out,
                    int64_t count, void *stream);

/* ---- Jacobian-free conditioning: a fixed number of conjugate-gradient iterations per particle on the data-consistency
 * system (A^T A + rho I)(x0_hat + d) = A^T y + rho x0_hat, from d = 0, followed by the sampler's own step with x0_hat
 * replaced by x0_hat + d.  Linear operators only (kinds 0-4); needs A and A^T, no derivative of the model.
 *   r_y = y - A x0_hat ;  dist[p] = ||r_y||_2            (the quantity dpsx_residual_norm_f32 reports, same bits)
 *   r = A^T r_y ;  p = r ;  rs = ||r||^2
 *   repeat iters times:
 *       t = A p ;  s = A^T t
 *       pq = ||t||^2 + rho ||p||^2                       (= p^T (A^T A + rho I) p, never negative)
 *       alpha = pq > 0 ? rs / pq : 0
 *       d += alpha p ;  r -= alpha (s + rho p)
 *       rs' = ||r||^2 ;  beta = rs > 0 ? rs' / rs : 0 ;  rs = rs'
 *       p = r + beta p
 *   x_next = sample + kappa d                            (x0_hat + d is not clamped)
 * kappa is the slope of the sampler's `sample` in x0_hat, evaluated in fp32 on the host: c1 for a DDPM record,
 * c1 - c2 / b for a DDIM record (bit 1 of add_noise: eps is re-derived from x0_hat, the variance does not depend on it).
 * Every ||.||^2 is one particle's sum: fp32 per-block partials in a fixed order, whose count depends on the particle size
 * only, added in double by the launch that consumes them; alpha and beta are formed in double and rounded to fp32 once.
 * A non-finite sum gives that particle the alpha / beta IEEE arithmetic yields and touches no other particle.  The last
 * iteration updates neither r nor p.  iters = 0 copies sample to x_next (and zeroes d_out) and still reports dist.
 * One linear chain of launches on `stream`: no allocation, no host read, no branch on data (graph-capturable).
 * sample, x_next: [n, c, h, w], x_next may be sample.  dist: [n].  d_out (nullable): [n, c, h, w] receives d.
 * DPSX_EUNSUPPORTED: phase retrieval, n > 65535.  DPSX_EINVAL: iters < 0 or > 64, rho negative or not finite, y_n not
 * dividing n, a DDIM record with b = 0, a null pointer.  All of them return before anything is launched. */
int64_t dpsx_cg_workspace_bytes(const dpsx_op *op, int64_t n, int64_t c, int64_t h, int64_t w);
int dpsx_cg_step_f32(dpsx_op *op, const float *x0_hat, const float *sample, const float *y, int64_t y_n,
                     float rho, int iters, const dpsx_coefs *coefs_host,
                     float *x_next, float *dist /* [n] */, float *d_out /* [n,c,h,w], may be NULL */,
                     int64_t n, int64_t c, int64_t h, int64_t w,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* ---- pseudoinverse guidance (PiGDM; Song, Vahdat, Mardani, Kautz 2023) on the CG solve: the measurement's noise-aware,
 * preconditioned residual pulled back through the model.  By the push-through identity, with rho_t = sigma_y^2 / r_t^2 and
 * r_t^2 = 1 - abar_t (the paper's unit-variance prior),
 *     r_t^2 A^T (r_t^2 A A^T + sigma_y^2 I)^-1 (y - A x0_hat)  =  (A^T A + rho_t I)^-1 A^T (y - A x0_hat)  =  d,
 * the vector dpsx_cg_step_f32 iterates on.  Per step, with the step's dpsx_coefs record and the sampler's float64 tables:
 *     d       = iters CG iterations from d = 0                      (dpsx_cg_step_f32's recurrence and launches, unchanged)
 *     rho_t   = sigma_y^2 / (1 - abar_t)                            (sigma_y = 0 for a clean measurement; no floor)
 *     x_next  = sample + weight w_t J^T d ,   J = d x0_hat / d x_t = gate (a I - b d eps / d x_t)
 *     w_t     = kappa a                  weighting "score" (kappa: dpsx_cg_step_f32's slope, c1 or c1 - c2 / b)
 *     w_t     = sqrt(abar_prev) / a      weighting "paper" (the paper's update with eps kept: "score" times abar_t on the
 *                                        x0_hat term only)
 * "score" is the step that is consistent with eps' = eps - sqrt(1 - abar_t) grad log p(y | x_t): x0_hat is shifted by
 * a J^T d and eps is re-derived from it, hence kappa; its error against the exact posterior of a Gaussian prior shrinks at
 * first order in the step count, while "paper" has a per-step weight that does not shrink with the step.
 * The caller forms rho = rho_t and gain = weight w_t b in float64 and rounds each to fp32 once.  This entry runs the chain
 * of dpsx_cg_step_f32 with one other last launch: per element, with D = d + alpha p of the last iteration (two fp32
 * roundings: the bits dpsx_cg_step_f32 leaves in d_out),
 *     g_model_out[p, e] = inside[p, e] ? gain * D : +0.0f           e < c h w: the eps half of [n, 2c, h, w]
 * one fp32 multiply.  The variance half of g_model_out is not touched (the caller zeroes it once, as for
 * dpsx_step_bwd_f32).  dpsx_step_update_f32 on it and on the model's VJP of it then gives
 *     sample - ((-a / b) g_eps + g_unet)  =  sample + weight w_t J^T d.
 * inside: dpsx_posterior_fwd_f32's clamp gate, uint8 [n, c, h, w].  dist, d_out, workspace (dpsx_cg_workspace_bytes), y_n:
 * as for dpsx_cg_step_f32, same bits.  iters = 0 zeroes the eps half (and d_out) and still reports dist.  No atomics; one
 * linear chain of launches on `stream`: no allocation, no host read, no branch on data (graph-capturable).
 * The last launch takes the 16-byte form where c h w is a multiple of 4, g_model_out and d_out are 16-byte aligned and
 * inside is 4-byte aligned, else the scalar form: same bits.
 * DPSX_EUNSUPPORTED: phase retrieval, n > 65535.  DPSX_EINVAL: iters < 0 or > 64, rho negative or not finite, gain not
 * finite, y_n not dividing n, a null pointer.  All of them return before anything is launched or written. */
int dpsx_cg_pullback_f32(dpsx_op *op, const float *x0_hat, const uint8_t *inside, const float *y, int64_t y_n,
                         float rho, int iters, float gain,
                         float *g_model_out /* [n,2c,h,w] */, float *dist /* [n] */,
                         float *d_out /* [n,c,h,w], may be NULL */,
                         int64_t n, int64_t c, int64_t h, int64_t w,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* ---- best-of-N scoring / select (gaussian_diffusion.py:626-633, 687-698;
 *      best_of_n_simple.py:32-40) */
/* costs[p] = ||y - A(x_p)||_2 without materialising the residual */
int dpsx_score_f32(dpsx_op *op, const float *x, const float *y, int64_t y_n, float *costs,
                   int64_t n, int64_t c, int64_t h, int64_t w,
                   void *workspace, int64_t workspace_bytes, void *stream);
/* The same scoring with the select fused in (gaussian_diffusion.py:626-631): costs[p] as above, *best_idx_dev =
 * argmin_p costs[p] (torch.argmin: first minimum, NaN counts as the minimum) and, if best_val_dev != NULL, its cost
 * -- the per-particle reduction and the select share one small follow-up launch. */
int dpsx_score_argmin_f32(dpsx_op *op, const float *x, const float *y, int64_t y_n, float *costs,
                          int64_t *best_idx_dev, float *best_val_dev,
                          int64_t n, int64_t c, int64_t h, int64_t w,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* One step of SearchDDPM.p_sample_loop (gaussian_diffusion.py:618-633): S1 (p_sample: `sample` out; x0_hat is not
 * needed by this loop), costs[p] = ||y - A(sample_p)||_2, best = argmin (torch.argmin order) and, if x_next != NULL,
 * x_next[p] = sample[best] for every p (img[best_path.repeat(n_paths)]).  Four launches: S1, the scoring launch, one
 * small launch that finishes the costs and selects, the replication.  x_next == NULL: up to the select only (multi-GPU callers
 * exchange the champions first). */
int dpsx_search_step_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                         const float *y, int64_t y_n, float *sample, float *costs,
                         int64_t *best_idx_dev, float *best_val_dev, float *x_next,
                         int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* The same step with the loop's state held as ONE particle (gaussian_diffusion.py:618-633): after a select every particle
 * is a copy of the winner (img[best_path.repeat(n_paths)], :633), so x_t is [1, c, h, w] and model_out [1, 2c, h, w] -- one
 * model evaluation per step for the caller -- while noise, sample and costs stay per particle ([n, ...]).  x_next (nullable)
 * receives the winner ONCE, [1, c, h, w].  Results are those of dpsx_search_step_f32 on n copies of the state, bit for bit. */
int dpsx_search_step_one_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                             const float *y, int64_t y_n, float *sample, float *costs,
                             int64_t *best_idx_dev, float *best_val_dev, float *x_next,
                             int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                             void *workspace, int64_t workspace_bytes, void *stream);

/* Multi-image forms of the two steps above: the n particles are `segments` images of n / segments particles each
 * (image-major), y_n is 1 or `segments`, and the select runs per image: best_idx_dev / best_val_dev are [segments] and
 * receive each image's winner as a global particle index (m * K + local), torch.argmin order within the image.
 *   _seg:     x_next[p] = sample[best[p / K]] (each image's winner replicated over its own particles);
 *   _one_seg: x_t [segments, c, h, w] and model_out [segments, 2c, h, w] hold one state per image (proposal p reads
 *             state p / K) and x_next [segments, c, h, w] receives each image's winner once.
 * With segments = 1 they equal dpsx_search_step_f32 / dpsx_search_step_one_f32 bit for bit. */
int dpsx_search_step_seg_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                             const float *y, int64_t y_n, float *sample, float *costs,
                             int64_t *best_idx_dev, float *best_val_dev, float *x_next, int64_t segments,
                             int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                             void *workspace, int64_t workspace_bytes, void *stream);
int dpsx_search_step_one_seg_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                                 const float *y, int64_t y_n, float *sample, float *costs,
                                 int64_t *best_idx_dev, float *best_val_dev, float *x_next, int64_t segments,
                                 int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                                 void *workspace, int64_t workspace_bytes, void *stream);

/* SearchDDPM.resample_update's cost update (gaussian_diffusion.py:556-585):
 *   curr[p] = ||y - A(x_p)||_1^2 / (c*h*w)                                         (:557-563)
 *   net[p]  = curr + prev (MEAN) | min(curr, prev) (MIN, NaN propagates as torch.min) | curr - prev (DIFF) | curr (CURR)
 * prev_costs == NULL (first call, :566-579) gives net = curr for every potential.  curr_costs may be NULL. */
enum { DPSX_POT_MEAN = 1, DPSX_POT_MIN = 2, DPSX_POT_DIFF = 3, DPSX_POT_CURR = 4 };
int dpsx_resample_cost_f32(dpsx_op *op, const float *x, const float *y, int64_t y_n, const float *prev_costs,
                           int potential, float *curr_costs, float *net_costs,
                           int64_t n, int64_t c, int64_t h, int64_t w,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* torch.argmin semantics: first minimum wins, NaN counts as the minimum (gaussian_diffusion.py:631).
 * val_out_dev (optional, may be NULL) receives v[argmin] -- `costs[best_path]` of :632 without a host index. */
int dpsx_argmin_f32(const float *v, int64_t n, int64_t *idx_out_dev, float *val_out_dev, void *stream);
/* The same per segment: v is [segments, k]; idx_out_dev[m] = m * k + the torch.argmin of v[m] (a global index),
 * val_out_dev[m] (nullable) its value -- the per-image best-of-N of a multi-image batch (best_of_n_simple.py:32-40). */
int dpsx_argmin_seg_f32(const float *v, int64_t segments, int64_t k, int64_t *idx_out_dev, float *val_out_dev,
                        void *stream);
/* The first b entries of every segment under the same order, in that order: NaN before every number (among NaNs the lower
 * index first), then the lower value, equal values (-0.0 == +0.0) by the lower index.  v is [segments, k];
 * idx_out_dev[m * b + r] is the global index of segment m's rank r, val_out_dev[m * b + r] (nullable) its value.  b = 1
 * is dpsx_argmin_seg_f32.  A rank is a count of the entries before it, so the result does not depend on how the launch
 * splits the work.  1 <= b <= k (DPSX_EINVAL); k <= 4096 (DPSX_EUNSUPPORTED above). */
int dpsx_topk_seg_f32(const float *v, int64_t segments, int64_t k, int64_t b, int64_t *idx_out_dev, float *val_out_dev,
                      void *stream);
/* dst[p] = src[ids[p]]   (ids: device int64 [n_out]; an id outside [0, n_src) fills dst[p] with NaN) */
int dpsx_gather_f32(const float *src, const int64_t *ids_dev, float *dst,
                    int64_t n_out, int64_t n_src, int64_t chw, void *stream);
/* dst[p] = src[*idx_dev] for all p  (img[best.repeat(n)], gaussian_diffusion.py:633) */
int dpsx_replicate_f32(const float *src, const int64_t *idx_dev, float *dst,
                       int64_t n_out, int64_t n_src, int64_t chw, void *stream);

/* ---- resampling draw: a pure function of (distances, uniforms), per segment of k particles (one image of a multi-image
 * batch; segments = 1: the whole set).  d, u: [segments * k] fp32, u[j] in [0, 1) is the caller's uniform of output slot j
 * (the library owns no RNG state); inv_scale finite and >= 0.  For each segment:
 *   1. a NaN / infinite distance gets weight 0; d_min = the minimum over the finite ones
 *   2. w_i = expf(-(d_i - d_min) * inv_scale)                       (fp32; the best particle has weight 1)
 *   3. q_i = (uint32) rintf(w_i * 2^24)                             (integer weights in [0, 2^24])
 *   4. all q_i equal (k = 1 and "no finite distance" included): the segment's ids are the identity
 *   5. else cdf_i = q_0 + ... + q_i in 64-bit integers, total = cdf_{k-1},
 *      ui = clamp((uint32)(u * 2^24), 0, 2^24 - 1) (NaN counts as 0), target = (total * ui) >> 24,
 *      slot j takes the smallest i with cdf_i > target.
 * Ids are global particle indices (segment * k + i), always inside their own segment; a particle with q_i = 0 is never
 * drawn.  The sums are integer sums, so the ids do not depend on how the launch splits the work: a segmented call and
 * one call per segment fed u[m k .. (m + 1) k) agree bit for bit.  k <= 4096 (DPSX_EUNSUPPORTED above).
 *   draw:     ids_out [n] int64, q_out [n] int32 (nullable: the integer weights).
 *   resample: the same draw fused with the gathers, one launch: dst[p] = src[ids[p]] ([n, chw] fp32), d_out[p] = d[ids[p]].
 *             n = segments * k <= 65535; src / dst and d / d_out must not overlap (DPSX_EINVAL). */
int dpsx_resample_draw_seg_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                               int64_t *ids_out, int32_t *q_out, void *stream);
int dpsx_resample_seg_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                          const float *src, float *dst, float *d_out, int64_t *ids_out, int32_t *q_out,
                          int64_t n, int64_t chw, void *stream);

/* ---- resampling schemes and the ESS trigger: the two entry points above with a scheme, a per-segment trigger and two
 * per-segment diagnostics.  Steps 1-3 are the draw's; with T = sum q_i, cdf_i = q_0 + ... + q_i, S2 = sum q_i^2 (exact
 * integers: T <= 2^36, S2 < 2^60 at k = 4096):
 *   trigger   ess_q16 in [0, 65536] is tau * 65536 rounded to nearest.  A segment resamples iff
 *             T^2 * 65536 < ess_q16 * k * S2   (both sides up to 2^88, compared in 128 bits), i.e. iff its effective
 *             sample size (sum w)^2 / sum w^2 is below tau * k; a segment that does not gets the identity.  By
 *             Cauchy-Schwarz T^2 <= k S2 with equality iff all q_i are equal, so ess_q16 = 65536 is exactly step 4's
 *             flat rule ("always, as above"; the all-zero segment gives 0 < 0), and ess_q16 = 0 means never.
 *   position  of slot j (the local index inside its segment), ui as in step 5:
 *             DPSX_RESAMPLE_MULTINOMIAL  target_j = (T * ui_j) >> 24                         (step 5)
 *             DPSX_RESAMPLE_STRATIFIED   target_j = ((T * (j * 2^24 + ui_j)) >> 24) / k      (product in 128 bits)
 *             DPSX_RESAMPLE_SYSTEMATIC   the same with ui_0, the uniform of the segment's first slot, for every j; the
 *                                        other k - 1 uniforms are ignored (the caller still supplies k of them, so its
 *                                        RNG stream position does not depend on the scheme)
 *             slot j takes the smallest i with cdf_i > target_j, clamped to [0, k - 1].
 * target_j < T always: a particle with q_i = 0 is never drawn and ids stay inside their segment whatever d and u hold.
 * With L_i = floor(k q_i / T) and n_i the number of slots that drew particle i: systematic L_i <= n_i <= L_i + 1,
 * stratified max(0, L_i - 1) <= n_i <= L_i + 2; both give ids that are non-decreasing in j.  The best particle of a
 * segment has q_i = 2^24 >= T / k, so the systematic scheme never loses it.
 *   resampled_out [segments] uint8 (nullable): 1 where the segment resampled, exactly the trigger above.
 *   ess_out       [segments] fp32  (nullable): (double) T * (double) T / (double) S2 rounded to fp32; 0 when S2 = 0.
 * Everything is integer arithmetic from q on, so these ids too are a property of the segment and not of the launch.
 * Refusals as above; an unknown scheme or ess_q16 outside [0, 65536] is DPSX_EINVAL.  With scheme 0 and ess_q16 = 65536
 * every output equals the entry points above. */
enum { DPSX_RESAMPLE_MULTINOMIAL = 0, DPSX_RESAMPLE_STRATIFIED = 1, DPSX_RESAMPLE_SYSTEMATIC = 2 };
int dpsx_resample_draw_seg_ex_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                                  int64_t *ids_out, int32_t *q_out, int scheme, int32_t ess_q16,
                                  uint8_t *resampled_out, float *ess_out, void *stream);
int dpsx_resample_seg_ex_f32(const float *d, const float *u, int64_t segments, int64_t k, float inv_scale,
                             const float *src, float *dst, float *d_out, int64_t *ids_out, int32_t *q_out,
                             int64_t n, int64_t chw, int scheme, int32_t ess_q16, uint8_t *resampled_out,
                             float *ess_out, void *stream);

/* ---- counter-based normals: the step noise as a pure function of (seed, step, tag, particle id, element), so a path's
 * noise does not depend on the batch, the particle groups, the images per batch or the ranks it is computed with.
 * Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), one call per float4 unit:
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (unit = element offset inside the particle / 4, particle id, step, tag)    tag 0: step noise, 1: x_start
 *   particle id of batch row p = particle_base + (per_image > 0 ? p % per_image : p); it must fit 32 bits (DPSX_EINVAL)
 *   words r0..r3 -> u1 = ((r >> 8) + 1) 2^-24 in (0, 1], u2 = (r >> 8) 2^-24 in [0, 1); rad = sqrt(-2 ln u1);
 *   (r0, r1) -> elements 0, 1 = (rad cos 2 pi u2, rad sin 2 pi u2), (r2, r3) -> elements 2, 3.   |z| <= 5.77, always finite.
 * Element e of a particle takes word e % 4 of unit e / 4 (chw need not be a multiple of 4).  The same distribution as
 * torch.randn, not the same stream.  One device function computes it everywhere: the fill below and the in-kernel draws
 * of the _rng entry points agree bit for bit.  The record is read on the host when the call is enqueued: a captured
 * graph replays the counters it was captured with. */
typedef struct dpsx_rng { uint64_t seed; uint32_t step; uint32_t tag; int64_t particle_base; int64_t per_image; } dpsx_rng;

/* out [n, chw] normals; bits_out (nullable) uint32 [n, 4 * ceil(chw / 4)]: the Philox words of every unit */
int dpsx_randn_f32(float *out, uint32_t *bits_out, int64_t n, int64_t chw, const dpsx_rng *rng_host, void *stream);

/* dpsx_posterior_fwd_f32 with the noise drawn inside the launch (no noise tensor is written or read) */
int dpsx_posterior_fwd_rng_f32(const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                               float *x0_hat, float *sample, uint8_t *inside,
                               int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream);

/* dpsx_step_fwd_f32 without the noise pointer.  DPSX_EUNSUPPORTED, before anything is launched: this operator / shape
 * has no in-kernel draw; the caller fills a noise buffer with dpsx_randn_f32 and calls dpsx_step_fwd_f32 -- the same bits.
 * dpsx_step_draws_in_kernel: 1 where the _rng call draws in its launch for 16-byte aligned buffers (both blur kernels
 * on whole 64 x 64 tiles, the row-streaming resize kernel, inpainting with H * W a multiple of 4, the identity), 0 where
 * it declines (the blur kernels' general loaders, the staged-rows resize kernel, phase retrieval). */
int dpsx_step_draws_in_kernel(const dpsx_op *op, int64_t c, int64_t h, int64_t w);
int dpsx_step_fwd_rng_f32(dpsx_op *op, const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                          const float *y, int64_t y_n,
                          float *x0_hat, float *sample, uint8_t *inside, void *resid, float *norm,
                          int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                          void *workspace, int64_t workspace_bytes, void *stream);

/* dpsx_search_step_seg_f32 / dpsx_search_step_one_seg_f32 with S1's noise drawn inside its launch (segments = 1: the
 * unsegmented steps) */
int dpsx_search_step_seg_rng_f32(dpsx_op *op, const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                                 const float *y, int64_t y_n, float *sample, float *costs,
                                 int64_t *best_idx_dev, float *best_val_dev, float *x_next, int64_t segments,
                                 int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                                 void *workspace, int64_t workspace_bytes, void *stream);
int dpsx_search_step_one_seg_rng_f32(dpsx_op *op, const float *x_t, const float *model_out, const dpsx_rng *rng_host,
                                     const float *y, int64_t y_n, float *sample, float *costs,
                                     int64_t *best_idx_dev, float *best_val_dev, float *x_next, int64_t segments,
                                     int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                                     void *workspace, int64_t workspace_bytes, void *stream);

/* The beam step: the search step that keeps the `beam` best proposals of every image instead of one.
 * x_t [states, c, h, w], model_out [states, 2c, h, w]: proposal p of n reads state p / (n / states); n % states == 0 and
 * states % segments == 0 (image m owns the states [m states / segments, ...) and the particles [m n / segments, ...)).
 * states == n is a loop's first step (n distinct particles, one proposal each), states == segments * beam every later one.
 * noise [n, c, h, w] or rng_host: exactly one of them when the step adds noise.  y_n is 1 or segments.
 * S1 -> the scoring launch -> costs + the per-image top-`beam` select (the order of dpsx_topk_seg_f32) -> the winners'
 * gather: best_idx_dev / best_val_dev (nullable) are [segments * beam] (global particle indices, rank-major inside an
 * image), x_next (nullable) [segments * beam, c, h, w] with x_next[m * beam + r] = sample[best_idx_dev[m * beam + r]].
 * x_next must not be x_t or sample.  beam = 1 with states = segments is dpsx_search_step_one_seg_f32 / _rng bit for bit.
 * 1 <= beam <= n / segments (DPSX_EINVAL); n / segments <= 4096 (DPSX_EUNSUPPORTED above). */
int dpsx_search_step_beam_f32(dpsx_op *op, const float *x_t, const float *model_out, const float *noise,
                              const dpsx_rng *rng_host, const float *y, int64_t y_n, float *sample, float *costs,
                              int64_t *best_idx_dev, float *best_val_dev, float *x_next, int64_t segments, int64_t states,
                              int64_t beam, int64_t n, int64_t c, int64_t h, int64_t w, const dpsx_coefs *coefs_host,
                              void *workspace, int64_t workspace_bytes, void *stream);

/* ---- particle weights for sequential Monte Carlo over the guided step (twisted SMC: Wu et al. 2023, "Practical and
 * asymptotically exact conditional sampling in diffusion models"; proposal_weight = 0 leaves the Feynman-Kac "difference"
 * potential).  K1 built sample = mean_u + sd z (z the step noise; sd per element: exp(0.5 logvar(v)) for a DDPM record,
 * sigma for a DDIM record) and K3 forms x_next = sample - s, s = (-a/b) g_eps + g_unet.  The guided proposal is
 * N(mean_u - s, sd^2), the model's own transition N(mean_u, sd^2), so
 *   corr = log p_u(x_next) - log q(x_next) = sum_e q_e (z_e - q_e / 2),   q_e = s_e / sd_e
 * and corr = 0 by definition on a step that adds no noise (bit 0 of add_noise clear: the proposal is deterministic).
 * Each particle carries its NEGATIVE log-weight E (the sign the resampling draw takes as its d, with inv_scale = 1):
 *   E      <- E + twist_scale (d_cur^p - d_prev^p) - proposal_weight corr        p in {1, 2}, d_cur = ||y - A(x0_hat)||
 *   d_prev <- d_cur                                                             (d_prev starts at 0: the twist at x_T)
 * A segment that resampled restarts from E = 0 (`reset`); the increment still missing arrives at the next step through the
 * gathered d_prev.
 *
 * dpsx_step_update_corr_f32: dpsx_step_update_f32 (x_next has its bits: the same expression, the same roundings) plus
 * the correction's partial sums, one launch.  model_out [n, 2c, h, w] (its variance half gives sd; not read for a DDIM
 * record); the noise is `noise` [n, chw] or the counters of rng_host (tag 0 and the particle-id rule of the _rng entry
 * points: the same bits as the pointer form fed dpsx_randn_f32) -- exactly one of the two, whatever the step.  Per element
 * q = s / sd and q (z - 0.5 q), one rounding per operation; sd comes from the device functions S1 uses.
 * corr_partials [n, slots], slots = dpsx_corr_slots of chw: grid (slots, n), one fp32 partial per block in a fixed tree;
 * the slot count depends on the particle size only, so a particle's partials do not depend on the batch it runs in; no
 * atomics.  On a step without noise the partials are written as 0 and model_out / noise are not read.
 * DPSX_EINVAL: a null pointer, both or neither of noise / rng_host, b = 0, a DDIM record with sigma <= 0 and bit 0 set, a
 * bad rng record; DPSX_EUNSUPPORTED: n > 65535.  All of them return before anything is launched.
 *
 * dpsx_smc_accum_f32: the recurrence above, one wave per particle.  corr (corr_partials == NULL: no correction term) is
 * the particle's `slots` partials added in double in a fixed order; base = reset[segment of p] ? 0 : E[p] (reset
 * [segments] uint8, nullable; the n particles are `segments` images of n / segments each, image-major); the sum is formed
 * in double from the fp32 inputs and rounded to fp32 once; d_prev[p] = d_cur[p].  A non-finite input reaches its own
 * particle's E only (the draw gives a NaN or infinite d weight 0).
 * DPSX_EINVAL: a null E / d_prev / d_cur, power not 1 or 2, segments < 1 or not dividing n, slots < 1 with partials given,
 * a non-finite twist_scale or proposal_weight; DPSX_EUNSUPPORTED: n > 65535.  Nothing is launched then.
 * Both calls are one launch on `stream`: no allocation, no host read (graph-capturable). */
int dpsx_corr_slots(int64_t chw);       /* partial slots per particle: ceil(chw / 1024), at least 1, at most 256 */
int dpsx_step_update_corr_f32(const float *sample, const float *g_model_out, const float *g_unet /* nullable */,
                              const float *model_out, const float *noise, const dpsx_rng *rng_host,
                              float *x_next, float *corr_partials, int64_t n, int64_t chw,
                              const dpsx_coefs *coefs_host, void *stream);
int dpsx_smc_accum_f32(float *E, float *d_prev, const float *d_cur, const float *corr_partials, int slots,
                       const uint8_t *reset, int64_t segments, int64_t n,
                       float twist_scale, int power, float proposal_weight, void *stream);

/* ---- spherical-Gaussian guidance (DSG: Yang et al. 2024, "Guidance with Spherical Gaussian Constraint for Conditional
 * Diffusion"; not in the reference): K3's place -- the update of gaussian_diffusion.py:255 -- without a step size.  K1 built
 * sample = mean + n, n = sd z (sd and z as in "particle weights" above), and s = (-a/b) g_eps + g_unet is the gradient K3
 * would subtract (dpsx_step_update_f32's expression and roundings).  Only the direction of s is used: x_next is put on the
 * sphere of radius r = ||sd|| around the mean, at m = n + g (d* - n) scaled back to the sphere, d* = -r s / ||s|| the
 * steepest-descent point and g = guidance_rate in [0, 1].  Per particle, S = sum s^2, Nn = sum n^2, C = sum s n, R = sum sd^2:
 *   r = sqrt(R) ;  mm = (1 - g)^2 Nn + g^2 R - 2 g (1 - g) r C / sqrt(S)                  (= ||m||^2)
 *   alpha = r (1 - g) / sqrt(mm) ;  beta = r^2 g / (sqrt(mm) sqrt(S))
 *   x_next = sample + (alpha - 1) n - beta s                                              (= mean + r m / ||m||)
 * Two launches on `stream`, grid (slots, n) with slots = dpsx_corr_slots(chw): the first leaves the four sums as fp32
 * per-block partials in stats [n, slots, 4] (order S, Nn, C, R; a fixed tree, no atomics, a slot count that depends on
 * the particle size only); in the second every block adds its particle's partials in double in a fixed order, forms alpha
 * and beta in double, rounds each to fp32 once and writes its range of x_next.  Every per-element operation is one fp32
 * rounding; the exact expression is the header of csrc/dsg.hip.  g = 0 is the unconditional sample renormalised to r.
 * A step without noise (bit 0 of add_noise clear: r = 0), a particle with S not > 0 (a zero gradient) or mm not > 0, NaN
 * sums included: x_next = sample bit for bit.  A step without noise writes stats as zeros and reads neither model_out,
 * noise nor the gradients.  A non-finite input reaches its own particle only.  x_next must not overlap an input.
 * The noise is `noise` [n, chw] or the counters of rng_host exactly as dpsx_step_update_corr_f32 draws them -- exactly one
 * of the two, whatever the step.
 * DPSX_EINVAL: a null pointer, both or neither of noise / rng_host, b = 0, guidance_rate outside [0, 1] or not finite, a
 * DDIM record with sigma <= 0 and bit 0 set, a bad rng record; DPSX_EUNSUPPORTED: n > 65535.  All of them return before
 * anything is launched.  No allocation, no host read (graph-capturable). */
int dpsx_step_update_dsg_f32(const float *sample, const float *g_model_out, const float *g_unet /* nullable */,
                             const float *model_out, const float *noise, const dpsx_rng *rng_host,
                             float guidance_rate, float *x_next, float *stats /* [n, slots, 4] */,
                             int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream);

/* ---- the multistep update of DPM-Solver++(2M) (Lu et al. 2022, "DPM-Solver++: Fast Solver for Guided Sampling of
 * Diffusion Probabilistic Models"; not in the reference): K3's place on a DDIM step of second order.  The first-order
 * DPM-Solver++ step is the DDIM record K1 already runs (eta = 0: the ODE form, eta = 1: the SDE form), so the 2M step is
 * dpsx_step_update_f32 plus one term in the difference of this step's and the previous step's x0_hat, with a host scalar
 * c (the sampler's table: c_i = sqrt(abar_{i-1}) (1 - e^{-h_i}) / (2 r_i) for eta = 0, (1 - e^{-2 h_i}) for eta = 1).
 * Per element, every operation one fp32 rounding:
 *   s      = (-a/b) g_eps + g_unet                        (dpsx_step_update_f32's expression; g_unet NULL: + 0.0f)
 *   u      = sample - s
 *   x_next = c == 0 ? u : u + c (x0_cur - x0_prev)
 * x0_cur, x0_prev [n, chw].  c == 0 (the step without history, the step onto the clean image): neither history pointer is
 * read, both may be NULL, and x_next has dpsx_step_update_f32's bits, -0.0 and NaN payloads included (the call runs that
 * entry point's launch).  Nothing crosses
 * particles or elements: a non-finite input reaches its own element of x_next only.  x_next must not overlap an input.
 * The float4 form runs where chw % 4 == 0 and every buffer the call reads or writes is 16-byte aligned (the histories
 * count only when c != 0), else the scalar form of the same body: the same bits.  With c != 0 sample, the gradients and
 * x0_prev are read for the last time of their step (non-temporal loads); x0_cur is the next step's x0_prev.
 * Bytes per particle of P = 4 chw: 5 P read (3 P at c = 0) and 1 P written, against dpsx_step_update_f32's 3 P + 1 P.
 * DPSX_EINVAL: a null sample / g_model_out / x_next / coefs_host, b = 0, c not finite, c != 0 with a null history pointer,
 * n < 0 or chw < 1; DPSX_EUNSUPPORTED: n > 65535.  All of them return before anything is launched.
 * One launch on `stream`: no partials, no atomics, no allocation, no host read (graph-capturable). */
int dpsx_step_update_ms_f32(const float *sample, const float *g_model_out, const float *g_unet /* nullable */,
                            const float *x0_cur, const float *x0_prev, float c,
                            float *x_next, int64_t n, int64_t chw, const dpsx_coefs *coefs_host, void *stream);

/* ---- per-particle reconstruction metrics against the label, on the device: what compute_metrics.py:77-90 (PSNR with
 * torchmetrics' default range) and the per-path loop feeding best_of_n_simple.py:20-40 compute on the host, plus SSIM
 * (Wang et al. 2004, the convention skimage and torchmetrics share).  Evaluation only: nothing here steers a sampler.
 *   x [n, c, h, w] particles, label [m, c, h, w], m | n, image-major: particle p belongs to image p / (n / m).
 *   L_m    = data_range if data_range > 0, else max(label_m) - min(label_m) (one fp32 subtraction; NaN propagates as
 *            torch's max / min do)
 *   mse_p  = mean over c h w of (x - label)^2 ;  psnr_p = 10 log10(L^2 / mse_p), evaluated as written in IEEE arithmetic:
 *            mse = 0 gives +inf, L = 0 gives -inf or NaN
 *   ssim_p = mean of s over the c (h - 10) (w - 10) positions at which the 11 x 11 window lies inside the image (no
 *            padding); window g_k ~ exp(-(k - 5)^2 / (2 1.5^2)), k = 0 .. 10, normalised to sum 1 (taps formed in double on
 *            the host), separable; per position and channel, with E[.] the windowed mean:
 *              mux = E[x], muy = E[y], vx = E[x^2] - mux^2, vy = E[y^2] - muy^2, cxy = E[xy] - mux muy   (biased, weighted)
 *              C1 = (0.01 L)^2, C2 = (0.03 L)^2
 *              s = (2 mux muy + C1) (2 cxy + C2) / ((mux^2 + muy^2 + C1) (vx + vy + C2))
 * One linear chain of at most three launches on `stream`: the label range (only when data_range is 0 and psnr or ssim is
 * asked for), the partial sums, the finisher.  With ssim the partial-sum launch runs one 32 x 32 tile of window positions
 * of one plane per block (the five windowed moments in fp32, every tap an fmaf in tap order, horizontal then vertical);
 * without it, a float4 stream over the particle (a scalar one when c h w is no multiple of 4 or a pointer is unaligned).
 * Every block leaves one fp32 partial (each lane adds serially, then a fixed tree); the squared-error partials of the two
 * forms are the same launch geometry and code, so mse and psnr of a call with ssim equal those of a call without, bit for
 * bit.  The finisher (one wave per particle) adds a particle's partials in double in a fixed order, forms mse, psnr and
 * ssim in double and rounds each to fp32 once.  No atomics, no fence, no allocation, no host read (graph-capturable).
 * Slot counts and the tile grid depend on (c, h, w) only: a particle's three numbers depend on its own pixels, its label
 * row, the shape and data_range -- not on n, m or its position in the batch.  A NaN in a particle reaches that particle's
 * numbers only; a NaN in a label reaches the particles of its image only.
 * mse, psnr, ssim: [n] each, each nullable, not all three.  The workspace (dpsx_metrics_workspace_bytes; it holds the
 * partial sums) serves one stream at a time.
 * DPSX_EINVAL: a null x, label or workspace; all three outputs null; m < 1 or m not dividing n; a size < 1; data_range
 * negative or not finite; ssim requested with h < 11 or w < 11.  DPSX_EUNSUPPORTED: n > 65535 (or c h w >= 2^31).
 * DPSX_EWORKSPACE: a short workspace.  All of them return before anything is launched. */
int64_t dpsx_metrics_workspace_bytes(int64_t n, int64_t m, int64_t c, int64_t h, int64_t w);
int dpsx_image_metrics_f32(const float *x, const float *label, int64_t m, float data_range,
                           float *mse, float *psnr, float *ssim,
                           int64_t n, int64_t c, int64_t h, int64_t w,
                           void *workspace, int64_t workspace_bytes, void *stream);

/* ---- particle repulsion: after the sampler's step, every particle of an image is pushed away from the image's other
 * particles by an RBF-kernel-weighted sum of differences (Corso et al. 2023, particle guidance, the fixed-potential form in
 * x_t space).  No model gradient: a pure function of the image's K states.  Its first half, the K x K squared-distance
 * matrix of an image, is also the diversity / collapse diagnostic of a particle set.  tests/repulse_ref.py restates the
 * definition in float64.
 *   x [n, chw] particles, image-major: M = segments images of K = n / M particles each, D = chw.  Everything below is per
 *   image and uses the image's own particles only.
 *   d2[i][j] = sum_e (x_i[e] - x_j[e])^2 in the difference form: one fp32 subtraction per element, the square accumulated
 *              with one fma.  Each pair is computed once (i < j) and mirrored: the matrix is symmetric bit for bit, its
 *              diagonal is +0.0, and two particles with equal bits have distance exactly 0.  The sum: per block (one tile
 *              pair of 8 x 8 particles and one contiguous element range) every lane adds its elements in index order, then a
 *              fixed tree; the slot count is a function of (D, K) only; the finisher adds a pair's slots in double in index
 *              order and rounds to fp32 once.
 *   mean     = sum_{i<j} d2[i][j] / (K (K - 1) / 2) in double over the fp32 entries, in a fixed order that depends on K only
 *              (thread t of 1024 adds the pairs at matrix entries t, t + 1024, ... in index order; then a fixed tree);
 *              min = the smallest off-diagonal entry (a NaN entry gives NaN).  K = 1: mean = 0, min = +inf.
 *   h        = bandwidth D if bandwidth > 0 (bandwidth is then a mean squared per-element difference), else
 *              mean / ln(K + 1): SVGD's heuristic with the mean in the median's place -- at the typical distance a weight
 *              is 1 / (K + 1).  In double.
 *   w[i][j]  = exp(-d2[i][j] / h) for i != j, formed in double and rounded to fp32 once; w[i][i] = 0.
 *   gain     = 2 c / h (double, rounded to fp32 once); c >= 0 is the caller's strength for this step.
 *   out_i[e] = fma(gain, S_i[e], x_i[e]),  S_i[e] = sum_j w[i][j] (x_i[e] - x_j[e]): j = 0 .. K - 1 in index order, each
 *              term one fp32 subtraction and one fma into the sum.  The push is repulsive (K = 2: out_0 - out_1 =
 *              (x_0 - x_1) (1 + 2 gain w01)) and, w being symmetric, keeps the image's mean.
 *   The flag: an image is stepped (applied = 1) iff K > 1, mean is finite, h > 0, h is finite and gain is finite in fp32.
 *   Otherwise it is COPIED, no arithmetic (-0.0 and NaN bits survive), its flag is 0, its w is all 0 and its gain is
 *   reported as 0: this covers K = 1, all particles equal, and any NaN / Inf in the image, decided per image inside the
 *   launches with no host read.  A non-finite value reaches its own image only.  All weights underflowing to 0 gives
 *   out = x.
 *   info [M, 4] = (h, gain, mean, min) per image; applied [M] the flag.
 * Three launches on `stream`: the pair partials (lanes across elements, float4 units where chw % 4 == 0 and x / out are
 * 16-byte aligned, else the scalar instantiation of the same body), the finisher (one block per image) and the apply.
 * No atomics, no fence, no allocation, no host read (graph-capturable).  An image's numbers do not depend on M or on its
 * place in the batch.  dpsx_pairwise_sqdist_f32 runs the first launch and the distance half of the second: d2 [M, K, K]
 * and info (nullable; h is the mean heuristic's, gain is 0).  dpsx_repulse_f32 runs all three; out [n, chw] must not
 * overlap x (every particle reads all K); d2 [M, K, K], w [M, K, K], info and applied are nullable outputs.  The workspace
 * (dpsx_repulse_workspace_bytes) serves one stream at a time.
 * DPSX_EINVAL: a null x, out (d2 for the distances) or workspace; chw < 1, segments < 1, n not divisible by segments;
 * c or bandwidth negative or not finite; out overlapping x.  DPSX_EUNSUPPORTED: K > 512 (more than 65535 images,
 * chw >= 2^31).  DPSX_EWORKSPACE: a short workspace.  All of them return before anything is launched. */
int64_t dpsx_repulse_workspace_bytes(int64_t n, int64_t chw, int64_t segments);
int dpsx_pairwise_sqdist_f32(const float *x, float *d2, float *info /* nullable */, int64_t n, int64_t chw,
                             int64_t segments, void *workspace, int64_t workspace_bytes, void *stream);
int dpsx_repulse_f32(float c, float bandwidth, const float *x, float *out, float *d2, float *w, float *info,
                     uint8_t *applied, int64_t n, int64_t chw, int64_t segments,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* ---- ensemble statistics: what an image's K particles say together -- the posterior mean (the MMSE estimate), the
 * per-pixel variance (the uncertainty map), the mean-of-n curve against the label (the companion of the best-of-n curve)
 * and one record per image.  Evaluation only: nothing here steers a sampler.  tests/ensemble_ref.py restates the
 * definition in float64.
 *   x [n, d] particles, image-major: M = images images of K = n / M particles each, d = c h w.  y [M, d] the label
 *   (nullable).  E [n] negative log-weights with SMC's sign convention (nullable: w_i = 1).  A prior (count0 > 0, with
 *   mean [M, d] and var [M, d] holding mean0 and var0 on entry) stands for count0 earlier particles of the same images.
 *   Everything below is per image and uses the image's own particles only.
 *   weights  with E: a non-finite E_i gives w_i = 0; E_min over the finite entries; w_i = exp(-(E_i - E_min)), the
 *            difference one fp32 subtraction, the exponential in double; W = sum w in double in index order; the
 *            normalised weight w_i / W is rounded to fp32 once.  ESS = W^2 / sum w^2 in double, rounded once.  An image
 *            with no finite E_i takes the uniform form below (ESS = K).  Without E, ESS = T.
 *   sums     per element e, particles in index order: c = mean0[e] with a prior, else the image's first particle's x[e];
 *            S1 = sum w (x - c), S2 = sum w (x - c)^2 in double (x - c formed in double; each term of S2 one fma).
 *   uniform  T = count0 + K:  mean = c + S1 / T;  M2 = var0 count0 + S2 - S1^2 / T;  var = max(M2 / T, 0)
 *   weighted (normalised fp32 weights):  mean = c + S1;  var = max(S2 - S1^2, 0)
 *            mean and var are each rounded to fp32 once.  The variance is the biased one; NaN passes through the max; an
 *            image of equal particles has var = +0.0 exactly.
 *   curve    only with y.  For n = 1 .. K: pm_n = c + (sum_{i <= n} (x_i - c)) r_n with r_n = 1 / (count0 + n) rounded to
 *            double once (with a prior c is mean0, so the prior adds 0 to the sum); curve[m][n - 1] = mean over e of
 *            (pm_n - y)^2, each squared error formed in double and rounded to fp32.  Always the uniform prefix in path
 *            order, whatever E is.  Column K holds the same error for the final (possibly weighted) mean, taken before
 *            its rounding to fp32.  The sum over e: a lane adds its elements serially in fp32, then a fixed tree per block;
 *            the finisher adds an image's cg_slots(d) block partials in double in a fixed order, divides by d and rounds
 *            once.
 *   info [M, 4] = (ESS, mean over e of the fp32 var, column K of the curve or NaN without y, T).
 * K <= 4096.  At most three launches on `stream`: the weights (only with E; one block per image), the stream over the
 * particles (grid (cg_slots(d), M); float4 units where d % 4 == 0 and x, y, mean, var are 16-byte aligned, else the scalar
 * instantiation of the same body; mean and var are the same bits in both forms) and the finisher.  No atomics, no fence,
 * no allocation, no host read (graph-capturable).  Slot counts depend on d only: an image's numbers depend on neither M
 * nor its place in the batch.  A NaN or Inf in a particle reaches its own elements of its own image's mean and var, and
 * the curve entries of its image from that particle on; nothing else changes a bit.  x is not written.
 *   low parts (dpsx_ensemble_ex_f32 only; mean_lo, var_lo [M, d], both or neither).  A prior is fp32, and mean0's rounding
 *            alone (2^-25 |mean0|) can exceed what a merged number may be off by -- where two groups' means nearly cancel,
 *            or the variance is tiny against the mean.  On return mean_lo = mean - fp32(mean) and var_lo = var - fp32(var),
 *            each rounded to fp32 (0 where the fp32 value is not finite).  With a prior they are read first, as ml and vl
 *            of the prior: its particles then count as count0 ml in S1 (and in the curve's prefix) and as
 *            count0 (var0 + vl + ml^2) in place of var0 count0.  Zero low parts, or dpsx_ensemble_f32, give the fp32 triple
 *            alone, exactly as stated above.  They are arguments like the others: a call's results depend on its
 *            arguments only.
 * mean, var [M, d] (in/out with a prior); curve [M, K + 1] nullable (null without y); info [M, 4].  The workspace
 * (dpsx_ensemble_workspace_bytes: the partial sums and the weights; nothing in it outlives the call) serves one stream
 * at a time.
 * DPSX_EINVAL: a null x, mean, var, info or workspace; one of mean_lo / var_lo without the other; n < 1, d < 1, images < 1, n not divisible by images; count0 < 0;
 * E together with a prior (two calls share no reference level for their weights); curve without y.
 * DPSX_EUNSUPPORTED: K > 4096 (more than 65535 images, d >= 2^31).  DPSX_EWORKSPACE: a short workspace.  All of them
 * return before anything is launched. */
int64_t dpsx_ensemble_workspace_bytes(int64_t n, int64_t d, int64_t images);
int dpsx_ensemble_f32(const float *x, const float *y /* nullable */, const float *neg_log_weights /* nullable */,
                      int64_t count0, float *mean, float *var, float *curve /* nullable */, float *info,
                      int64_t n, int64_t d, int64_t images, void *workspace, int64_t workspace_bytes, void *stream);
int dpsx_ensemble_ex_f32(const float *x, const float *y /* nullable */, const float *neg_log_weights /* nullable */,
                         int64_t count0, float *mean, float *var, float *mean_lo /* nullable */,
                         float *var_lo /* nullable */, float *curve /* nullable */, float *info,
                         int64_t n, int64_t d, int64_t images, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- order statistics: what an image's K particles say per element without assuming a shape -- quantiles (the median,
 * a credible band), the rank histogram of the label among the particles (the Talagrand diagram) and the CRPS, all from
 * one per-element sort across the particles.  Evaluation only: nothing here steers a sampler.  tests/quantile_ref.py
 * restates the definition in float64.
 *   x [n, d] particles, image-major: M = images images of K = n / M particles each.  y [M, d] the label (nullable).
 *   probs [q]: a HOST array of doubles, read before the first launch (the call stays graph-capturable); 1 <= q <= 8,
 *   each in [0, 1].  Everything below is per image and per element e and uses that image's own K values only.
 *   order    the non-NaN values of an element are ordered by IEEE comparison with -0.0 before +0.0: signed comparison of
 *            s ^ ((s >> 31) & 0x7fffffff) on the bit pattern s.  A total order: the sorted sequence
 *            x_(0) <= ... <= x_(K-1) is determined bit for bit.
 *   quant [M, q, d]: h = probs[i] (K - 1) in double, lo = floor(h), f = h - lo, both formed on the host, once;
 *            a = x_(lo), b = x_(min(lo + 1, K - 1)).  f == 0 or a == b: the output is a, its bits kept.  Otherwise
 *            (float)(a + f (b - a)): the subtraction, the product and the sum one rounding in double each, no fma; the
 *            result is rounded to fp32 once.  +-Inf behave as IEEE gives them; an interpolation that is NaN (-Inf
 *            against +Inf) is the canonical quiet NaN 0x7fc00000.  If any of the element's K values is NaN, all q
 *            outputs of the element are 0x7fc00000.
 *   hist [M, K + 2] int32, only with y (nullable): rank_e = #{j : x_j[e] < y[e]}, strict IEEE comparison, 0 .. K; an
 *            element whose label or any of whose particles is NaN goes to bin K + 1.  The bins of an image sum to d.
 *            Exact: integer counts per block, added per column by the finisher.
 *   info [M, 4] = (mean CRPS, mean of quant[q - 1] - quant[0] (one fp32 subtraction) over the elements where it is
 *            finite, number of invalid elements, K).  The first is NaN and the third 0 without y.  Per element, in
 *            double, i 0-based over the sorted values, both sums in sorted order:
 *                crps_e = (sum_i |x_(i) - y|) / K - (sum_i (2 i - K + 1) x_(i)) / K^2
 *            rounded to fp32 once.  Invalid elements (bin K + 1) contribute 0 and are left out of the divisor.  The sum
 *            over e: a lane adds its elements serially in fp32, then a fixed tree per block, one partial per block; the
 *            finisher adds an image's partials in double in a fixed order and divides once.  The width likewise.
 * K <= 512.  K <= 64 sorts in registers (a fixed network on K padded to a power of two), 64 < K <= 512 in LDS.  Two
 * launches on `stream`: the element pass (a lane owns an element; the block count per image is a function of (d, K) only)
 * and the finisher.  No global atomics, no fence, no allocation, no host read, no memset (graph-capturable; results
 * depend on the arguments only).  An image's numbers depend neither on M nor on its place in the batch, bit for bit.  A
 * NaN reaches its own element of its own image only.  x is not written and may have any 4-byte alignment.  The workspace
 * (dpsx_quantiles_workspace_bytes: the per-block partials; nothing in it outlives the call) serves one stream at a time.
 * DPSX_EINVAL: a null x, quant, info, workspace or probs; q outside 1 .. 8; a prob outside [0, 1] or NaN; hist without y;
 * n < 1, d < 1, images < 1, n not divisible by images.  DPSX_EUNSUPPORTED: K > 512 (more than 65535 images, d >= 2^31).
 * DPSX_EWORKSPACE: a short workspace.  All of them return before anything is launched. */
int64_t dpsx_quantiles_workspace_bytes(int64_t n, int64_t d, int64_t images);
int dpsx_quantiles_f32(const float *x, const float *y /* nullable */, const double *probs /* host */, int64_t q,
                       float *quant /* [M, q, d] */, int32_t *hist /* nullable, [M, K + 2] */, float *info /* [M, 4] */,
                       int64_t n, int64_t d, int64_t images, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- principal components: in which directions an image's K particles vary together -- the top q eigenvectors of their
 * sample covariance (shown as mean +- 2 sigma_j u_j), the variance along each and every particle's score along it.  With
 * K << d this is a K x K problem: the eigenpairs of the centred Gram matrix, projected back to image space.  Evaluation
 * only: nothing here steers a sampler.  tests/pca_ref.py restates the definition in float64.
 *   x [n, d] particles, image-major: M = images images of K = n / M particles each; 1 <= q <= 8 components.  Everything
 *   below is per image and uses the image's own particles only.
 *   d2       [K, K], exactly what dpsx_pairwise_sqdist_f32 defines: the same two launches, the same bits.
 *   G        the centred Gram matrix, G_ij = (x_i - mean) . (x_j - mean) = -1/2 (d2_ij - r_i - r_j + t) with
 *            r_i = (sum_j d2_ij) / K and t = (sum_i r_i) / K, both in double over the fp32 entries in index order;
 *            G_ij = (float)(-0.5 (((d2_ij - r_lo) - r_hi) + t)) with lo = min(i, j), hi = max(i, j), every operation one
 *            rounding in double: symmetric bit for bit.  trace = sum_i G_ii in double over the fp32 entries in index order
 *            (= sum_i |x_i - mean|^2).
 *   eigenpairs  G = V L V^T by the cyclic Jacobi method in fp32, the rotations of a sweep in a fixed (round-robin) order
 *            that depends on K only.  A rotation is skipped where |g_pq| <= 2^-24 sqrt(|g_pp g_qq|).  After every sweep:
 *            off = the sum of the squared off-diagonal entries, total = that of all entries, in double in a fixed order;
 *            the sweeps end when off <= K 2^-46 total (an off-diagonal norm of sqrt(K) 2^-23 |G|_F: above the rounding
 *            floor of the rotations, which sits near sqrt(K) 2^-26) or after 24 sweeps.  l_i = the diagonal; the order is
 *            descending, the lower index first among equal values.
 *   null     component j is null if j >= K or l_j <= K 2^-23 l_0 (the product formed in fp32, K 2^-23 first) or
 *            l_j <= 0: below the resolution of an fp32 Jacobi method on a K x K matrix, negative round-off included.
 *            A null component has evals = +0.0 and all-zero dirs and coords.
 *   centring every non-null v_j among the first q is centred and renormalised: v_ij <- (v_ij - m_j) / |v_j - m_j| with m_j
 *            the mean of its entries, in double in index order, each entry rounded to fp32 once.  An eigenvector of a
 *            non-zero eigenvalue of G is orthogonal to the constant vector; the part along it that fp32 rounding leaves
 *            (about 2^-23 l_0 / l_j) would enter dirs multiplied by (mean - x_0) / sqrt(l_j).  The eigenvalue reported
 *            for it is the Rayleigh quotient of the unit vector, l_j <- (float)(l_j / |v_j - m_j|^2) (the accumulated
 *            rotations leave |v_j| within about 1e-5 of 1 at K = 128, and the diagonal is v_j^T G v_j of that v_j); the
 *            order, the null rule and rank use the diagonal as the sweeps left it.
 *   sign     in every non-null v_j the entry of largest magnitude is then positive (the lowest index wins ties).
 *   evals [M, q] = l_j (0 for a null component).  coords [M, K, q]: c_ij = sqrt(l_j) v_ij (one fp32 square root, one product): the score of
 *            particle i along component j.
 *   dirs [M, q, d]: u_j[e] = S_j[e] (1 / l_j), S_j[e] = sum_i c_ij (x_i[e] - x_0[e]): i = 0 .. K - 1 in index order, each
 *            term one fp32 subtraction and one fp32 fma into the sum; 1 / l_j one fp32 division, the product one rounding.
 *            (The scores of a component sum to zero, so any common offset drops out; x_0 keeps the differences small.)
 *            Unit norm and mutually orthogonal up to rounding.
 *   info [M, 4] = (trace, rank, sweeps, K): rank = the number of non-null eigenvalues among all K; sweeps = the sweeps
 *            performed.  The variance along component j is l_j / K (the biased one, as dpsx_ensemble_f32's: trace / K is the
 *            sum over the elements of its var), its share of the total l_j / trace.
 *   degenerate images, decided inside the launches with no host read.  K = 1, or t exactly 0 (all particles equal): every
 *            output is +0.0, rank 0, no rotation is performed.  t not finite (a NaN or Inf anywhere in the image): evals,
 *            dirs, coords and info[0] are the canonical quiet NaN 0x7fc00000, rank is -1, sweeps 0; the flag reaches that
 *            image only.  24 sweeps without convergence: rank is -2, the other outputs are what the last sweep left.
 * K <= 128: G and V live in the 160 KiB of LDS of one compute unit (two fp32 matrices of 128 x 129 words); more particles
 * need a blocked or global-memory solver.  Four launches on `stream`: the two distance launches, the eigensolver (one
 * workgroup per image, instantiated for K <= 32 / 64 / 128) and the projection (lanes across elements, float4 units where
 * d % 4 == 0 and x / dirs are 16-byte aligned, else the scalar instantiation of the same body).  No atomics, no fence, no
 * allocation, no host read, no memset (graph-capturable).  An image's numbers depend neither on M nor on its place in the
 * batch, bit for bit.  x is not written.  d2 [M, K, K] is a nullable output.  The workspace (dpsx_pca_workspace_bytes:
 * the distance launches' partials and d2; nothing in it outlives the call) serves one stream at a time.
 * DPSX_EINVAL: a null x, dirs, evals, coords, info or workspace; q outside 1 .. 8; n < 1, d < 1, images < 1, n not
 * divisible by images.  DPSX_EUNSUPPORTED: K > 128, more than 65535 images, d >= 2^31.  DPSX_EWORKSPACE: a short workspace.
 * All of them return before anything is launched. */
int64_t dpsx_pca_workspace_bytes(int64_t n, int64_t d, int64_t images);
int dpsx_pca_f32(const float *x, int64_t q, float *dirs /* [M, q, d] */, float *evals /* [M, q] */,
                 float *coords /* [M, K, q] */, float *info /* [M, 4] */, float *d2 /* nullable, [M, K, K] */,
                 int64_t n, int64_t d, int64_t images, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- the device half of the multi-GPU champion exchange (best-of-N across ranks: gaussian_diffusion.py:626-633 and
 * best_of_n_simple.py:32-40 over a sharded particle set).  The collective itself stays with the caller's communicator
 * (RCCL through torch.distributed); these two launches replace the seven small device ops around it -- argmin, copy,
 * concatenation, two strided copies, argmin, replication -- whose launch gaps and host calls cost more than the collective.
 *   pack:   out[0 .. chw) = particles[best], out[chw .. chw+4) = (cost, (float)best, 0, 0): the record one all-gather
 *           carries (the header sits BEHIND the image so that the image stays 16-byte aligned).  best_idx_dev == NULL:
 *           the torch.argmin-order select over costs runs in this launch; else costs may be NULL if best_val_dev is given.
 *   select: table is the gathered [world][chw + 4]; the winner is the torch.argmin-order minimum of table[r][chw]
 *           (lowest rank wins ties, NaN counts as the minimum); dst[p] = its image for p < n_out; win_rank_dev /
 *           win_local_dev (nullable) receive the winning rank and its local particle index. */
int dpsx_pack_champion_f32(const float *particles, const float *costs, const int64_t *best_idx_dev,
                           const float *best_val_dev, float *out, int64_t n, int64_t chw, void *stream);
int dpsx_select_champion_f32(const float *table, int64_t world, int64_t chw, float *dst, int64_t n_out,
                             int64_t *win_rank_dev, int64_t *win_local_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DPSX_H */
