/* libi2v_hip.so -- the TRAINING path of one GeneratorBlock of the stage-1 decoder (stage1_VAE/modules/decoder.py:7-52 with the Spade, ADAIN and
 * Norm3D of normalization_layer.py): a forward that saves what the backward needs, and the backward to x, to the latent and to every
 * parameter of the block (csrc/i2v_gblock_train.hip).  The inference path stays i2v_gblock_* of i2v_hip.h.
 *
 * A fifth header with a table of its own (i2v_native.GBLOCK_TRAIN_SYMBOLS).  Conventions of i2v_hip_enc3d_train.h: plain device pointers, calls
 * only enqueue on `stream`, 0 = ok and I2V_E_* otherwise, i2v_last_error() for the message; exact fp32 on the matrix cores, no atomics,
 * every sum has a fixed order and two runs give the same bits.  The two 3x3x3 convs, Spade's three 2-D convs, the affine GroupNorm and the
 * power iteration run on the kernels of the 3-D ResNet training trunk (csrc/i2v_res3d_trunk.h).  The surface is the reference's
 * [B][C][T][H][W]; inside, activations are channels-last [B][T][H][W][C]. */
#ifndef I2V_HIP_GBLOCK_TRAIN_H
#define I2V_HIP_GBLOCK_TRAIN_H

#include "i2v_hip_disc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_gblock_train i2v_gblock_train;

#define I2V_GBLOCK_TRAIN_SAVE 1  /* keep in `saved` what i2v_gblock_train_backward needs */
#define I2V_GBLOCK_TRAIN_TRAIN 2 /* .train(): one power iteration per spectral-normed conv, in place on weight_u / weight_v */

/* modes of i2v_gblock_train_modnorm_backward_unit */
#define I2V_GBLOCK_TRAIN_SPADE 0
#define I2V_GBLOCK_TRAIN_ADAIN 1

/* I2V_E_INVALID before a device is looked for: n_in or n_out not a multiple of 16 in [16, 1024], z_dim < 1.  spectral_norm 0: the
 * same code with sigma = 1 and the keys conv_*.weight instead of conv_*.weight_orig / weight_u / weight_v. */
int i2v_gblock_train_create(int32_t n_in, int32_t n_out, int32_t z_dim, int32_t spectral_norm, i2v_gblock_train** out);
void i2v_gblock_train_destroy(i2v_gblock_train* g);
/* params[i].data: DEVICE pointer of the tensor with state_dict key params[i].name -- conv_{0,1}.{weight_orig,weight_u,weight_v,bias},
 * conv_s.{weight_orig,weight_u,weight_v} and norm_s.bn.{weight,bias} where n_in != n_out, norm_0.{conv,conv_gamma,conv_beta}.{weight,bias},
 * norm_1.linear.{weight,bias}.  Read in place by every call; nothing is copied or packed on the host. */
int i2v_gblock_train_bind(i2v_gblock_train* g, const i2v_tensor* params, int32_t n);
/* The gradient tensors of the parameters under the same keys (DEVICE pointers); grads NULL with n = 0: none bound. */
int i2v_gblock_train_bind_grads(i2v_gblock_train* g, const i2v_tensor* grads, int32_t n);
/* 0 for a shape that is refused. */
size_t i2v_gblock_train_saved_bytes(const i2v_gblock_train* g, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t img_h, int32_t img_w);
size_t i2v_gblock_train_workspace_bytes(const i2v_gblock_train* g, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t img_h, int32_t img_w);
/* GeneratorBlock.forward: x [batch][n_in][t][h][w], z [batch][z_dim], img [batch][3][img_h][img_w] -> out [batch][n_out][t][h][w].
 * flags: I2V_GBLOCK_TRAIN_SAVE (then `saved` takes the activations, the statistics, the operand layouts of the weights and this call's
 * sigma, u and v; else it may be NULL), I2V_GBLOCK_TRAIN_TRAIN. */
int i2v_gblock_train_forward(i2v_gblock_train* g, const float* x, const float* z, const float* img, int32_t batch, int32_t t, int32_t h, int32_t w,
                             int32_t img_h, int32_t img_w, int32_t flags, float* out, void* saved, size_t saved_bytes, void* workspace,
                             size_t workspace_bytes, void* stream);
/* Backward of the forward that filled `saved`: g_out [batch][n_out][t][h][w] -> dx [batch][n_in][t][h][w] and dz [batch][z_dim] (each NULL:
 * not wanted) and, with param_grads, the gradient of every bound parameter, written or (accumulate) added; without param_grads no
 * weight-gradient kernel is launched.  No gradient is formed at the start frame.  Nothing wanted at all: I2V_E_INVALID. */
int i2v_gblock_train_backward(i2v_gblock_train* g, const float* g_out, const float* z, const void* saved, size_t saved_bytes, int32_t batch, int32_t t,
                              int32_t h, int32_t w, int32_t img_h, int32_t img_w, float* dx, float* dz, int32_t param_grads, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream);

/* ---- the new kernel families one at a time, from raw DEVICE tensors, for the tests.  Maps are channels-last, c a multiple of 16. ---- */
/* enough for every unit below on `rows` rows (the positions of all `batch` samples) of at most `c` channels on either side */
size_t i2v_gblock_train_unit_workspace_bytes(int32_t batch, int64_t rows, int32_t c);
/* The backward of a normalisation under a modulation and a LeakyReLU(0.2).  g, act (the activated output: its sign is the decision) and
 * x [batch][t][h][w][c].  I2V_GBLOCK_TRAIN_SPADE: GroupNorm(16) without affine under (1 + mod), mod [batch][h][w][c]; dgamma and dbeta
 * [batch][h][w][c] are the sums over t.  I2V_GBLOCK_TRAIN_ADAIN: the instance norm under mod[.][0 .. c), mod [batch][2 c]; dgamma
 * [batch][2 c] receives (d gamma | d beta) and dbeta is not used.  dx (+ add, of dx's shape), dgamma and dbeta: NULL is not wanted. */
int i2v_gblock_train_modnorm_backward_unit(int32_t mode, const float* g, const float* act, const float* x, const float* mod, int32_t batch, int32_t t,
                                           int32_t h, int32_t w, int32_t c, const float* add, float* dx, float* dgamma, float* dbeta,
                                           void* workspace, size_t workspace_bytes, void* stream);
/* out [m][n] = a [m][k] . w [n][k]^T (+ add [m][n]): the 1x1x1 conv and, with the transposed weight, its input gradient. */
int i2v_gblock_train_pointwise_unit(const float* a, const float* w, const float* add, int64_t m, int32_t k, int32_t n, float* out, void* stream);
/* dw [cout][cin] = sum over the rows of g [m][cout] x [m][cin], in slices added in slice order; with sigma (and u [cout], v [cin]) the
 * spectral-norm projection (dw - <dw, w / sigma> u v^T) / sigma against w = weight_orig. */
int i2v_gblock_train_pointwise_wgrad_unit(const float* g, const float* x, const float* w, const float* u, const float* v, const float* sigma,
                                          int64_t m, int32_t cout, int32_t cin, int32_t accumulate, float* dw, void* workspace,
                                          size_t workspace_bytes, void* stream);
/* db [c] = the sum of g [m][c] over the rows in float64, rounded once. */
int i2v_gblock_train_bias_grad_unit(const float* g, int64_t m, int32_t c, int32_t accumulate, float* db, void* workspace, size_t workspace_bytes,
                                    void* stream);
/* ADAIN's Linear backwards: d_lin [batch][j], z [batch][k], w [j][k] -> dw [j][k], db [j], dz [batch][k] (each NULL: not wanted). */
int i2v_gblock_train_linear_backward_unit(const float* d_lin, const float* z, const float* w, int32_t batch, int32_t j, int32_t k, int32_t accumulate,
                                          float* dw, float* db, float* dz, void* stream);
/* A 3x3 2-D conv (stride 1, pad 1) on the trunk's kernels: x [batch][h][w][cinp] (cinp = 4 for cin 3), w [cout][cin][3][3], g
 * [batch][h][w][cout] -> y (the conv of x, without bias), dx [batch][h][w][cin] (cin a multiple of 16) and dw; each NULL: not wanted. */
int i2v_gblock_train_conv2d_unit(const float* x, const float* w, const float* g, int32_t batch, int32_t h, int32_t w_, int32_t cin, int32_t cout,
                                 float* y, float* dx, float* dw, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
