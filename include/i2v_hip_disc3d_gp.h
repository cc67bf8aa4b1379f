/* libi2v_hip.so -- the temporal discriminator's gradient penalty (loss.py:35-43) WITH its gradient at the parameters, the w_GP term of
 * loss.py:94-109 (csrc/i2v_res3d_gp.h, csrc/i2v_disc3d.hip).
 *
 * A seventh header, with a table of its own (i2v_native.DISC3D_GP_SYMBOLS); the handle is i2v_hip_disc3d.h's.  Same conventions: plain
 * device pointers, calls only enqueue on `stream`, 0 = ok and I2V_E_* otherwise, i2v_last_error() for the message; every buffer is the
 * caller's, and an entry writes nothing outside the bytes it is given.
 *
 * No general double backward.  With P = mean_b pred_b, g = grad_x P and L_GP = (1 / n) sum_b |g_b|^2, the gradient of L_GP at the
 * parameters is the gradient of the directional derivative of P along v = (2 / n) g, v held constant: one tangent forward with
 * x-dot = v on the primal's ReLU masks, argmaxes, statistics and normalised weights, then one reverse pass over the pair (primal,
 * tangent) seeded at the tangent of P.  u and v of the spectral norm are constants, sigma depends on weight_orig as in the existing
 * projection.  Exact fp32 on the matrix cores, no atomics, fixed summation orders: two runs give the same bits. */
#ifndef I2V_HIP_DISC3D_GP_H
#define I2V_HIP_DISC3D_GP_H

#include "i2v_hip_disc3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kinds of i2v_disc3d_gp_saved_layout: the tangent maps, all fp32 */
#define I2V_DISC3D_GP_CONV_OUT 0 /* the tangent of a conv's output */
#define I2V_DISC3D_GP_ACT 1      /* the tangent behind the GroupNorm (and the residual add and the primal's ReLU mask) */
#define I2V_DISC3D_GP_POOL_OUT 2 /* the tangent of the max pool's output */
#define I2V_DISC3D_GP_INPUT 3    /* the tangent clip (2 scale / n) g, [n][t][h][w][4] = (r, g, b, 0) */

/* The tangent's saved region and the workspace of i2v_disc3d_gp_backward; 0 for a shape that is refused. */
size_t i2v_disc3d_gp_saved_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w);
size_t i2v_disc3d_gp_workspace_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w);
/* Where the tangent maps lie in `gp_saved` after i2v_disc3d_gp_backward, as i2v_disc3d_saved_layout describes `saved` (kinds
 * I2V_DISC3D_GP_*; conv -1 for the pool's map and the input).  Arrays of 64.  A host function. */
int i2v_disc3d_gp_saved_layout(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w, int32_t* count, int32_t* kind, int32_t* conv,
                               int32_t* dims, int64_t* offset);
/* From the `saved` of a forward with I2V_DISC3D_SAVE on the real clips, without a host synchronisation: g = the gradient of mean(pred)
 * at the clips (seed 1 / n), *l_gp = (1 / n) sum_b |g_b|^2 (one double on the device; the bits of i2v_disc3d_backward +
 * i2v_disc3d_sumsq), the tangent forward with x-dot = (2 scale / n) g into `gp_saved`, the reverse pass over the pair, and
 * scale * dL_GP / dparameter into every bound gradient tensor, written or (accumulate) added.  layer.3.1.bn2.bias has no penalty
 * gradient: zero is written (added).  No gradient at the clips is formed.  `saved` is read only. */
int i2v_disc3d_gp_backward(i2v_disc3d* d, const void* saved, size_t saved_bytes, int32_t n, int32_t t, int32_t h, int32_t w, float scale,
                           void* gp_saved, size_t gp_saved_bytes, double* l_gp, int32_t accumulate, void* workspace, size_t workspace_bytes,
                           void* stream);
/* The same with the scale scale * *scale_dev, *scale_dev one float on the device (an upstream gradient that must not reach the host). */
int i2v_disc3d_gp_backward_dev(i2v_disc3d* d, const void* saved, size_t saved_bytes, int32_t n, int32_t t, int32_t h, int32_t w, float scale,
                               const float* scale_dev, void* gp_saved, size_t gp_saved_bytes, double* l_gp, int32_t accumulate, void* workspace,
                               size_t workspace_bytes, void* stream);

/* ---- one kernel group at a time, from raw DEVICE tensors, for the tests.  Maps channels-last [n][positions][c], c % 16 == 0.  Per
 * (sample, group) of m elements: xh = (x - mean) rstd, M(a) = mean(a), C(a) = mean(xh a), Pi(a) = a - M(a) - xh C(a). ---- */
size_t i2v_disc3d_gp_groupnorm_workspace_bytes(int32_t n, int32_t c);
/* GroupNorm's tangent: x, stats of the primal (i2v_disc3d_groupnorm_unit), xd the tangent input -> tstats [n][16][2] float64 =
 * (M(xd), C(xd)) and out = weight rstd Pi(xd) (+ resd) (times [mask > 0] when mask, the primal's activated output, is given). */
int i2v_disc3d_gp_groupnorm_tangent_unit(const float* x, const float* xd, const double* stats, const float* resd, const float* mask,
                                         const float* weight, int32_t n, int64_t positions, int32_t c, float* out, double* tstats, void* workspace,
                                         size_t workspace_bytes, void* stream);
/* The reverse of (GroupNorm, its tangent): g, gd the adjoints at the primal and at the tangent output (both times [mask > 0] when mask
 * is given), p = weight gd, q = weight g -> dxd = rstd Pi(p), dx = rstd Pi(q) - rstd^2 [xh mean(p Pi(xd)) + C(xd) Pi(p) + C(p) Pi(xd)],
 * dweight = sum g xh + sum gd rstd Pi(xd), dbias = sum g (both or neither; written or added). */
int i2v_disc3d_gp_groupnorm_dual_backward_unit(const float* g, const float* gd, const float* mask, const float* x, const float* xd,
                                               const double* stats, const double* tstats, const float* weight, int32_t n, int64_t positions,
                                               int32_t c, float* dx, float* dxd, float* dweight, float* dbias, int32_t accumulate, void* workspace,
                                               size_t workspace_bytes, void* stream);
/* The max pool's tangent: out [n][t][ho][wo][c] = xd [n][t][h][w][c] at the primal's argmax (I2V_DISC3D_POOL_ARGMAX). */
int i2v_disc3d_gp_maxpool_tangent_unit(const float* xd, const int32_t* argmax, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, float* out,
                                       void* stream);
/* The head's tangent and its reverse: xd [n][16][c], weight [c] -> pdot [n] = weight . avg(xd_b); with s the seed scale,
 * dweight [c] = (s / n) sum_b avg(xd_b), dxd [n][16][c] = s weight / (16 n), dx [n][16][c] = 0. */
int i2v_disc3d_gp_head_dual_unit(const float* xd, const float* weight, float s, int32_t n, int32_t c, float* pdot, float* dx, float* dxd,
                                 float* dweight, void* stream);

#ifdef __cplusplus
}
#endif
#endif
