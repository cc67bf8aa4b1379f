/* libi2v_hip.so -- the TRAINING path of the motion encoder of stage 1: resnet3D.Encoder (stage1_VAE/modules/resnet3D.py:138-219), a 3-D
 * ResNet-18 with GroupNorm(16), a (3, 7, 7) stem of stride (2, 2, 2) and the posterior head (conv_mu, conv_var, the reparameterisation,
 * the KL term of loss.py:10-12), forward and backward (csrc/i2v_encoder_train.hip).  The inference path stays i2v_encoder3d_* of i2v_hip.h.
 *
 * A fourth header with a table of its own (i2v_native.ENC3D_TRAIN_SYMBOLS).  Conventions of i2v_hip_disc3d.h: plain device pointers, calls
 * only enqueue on `stream`, 0 = ok and I2V_E_* otherwise, i2v_last_error() for the message; exact fp32 on the matrix cores, no atomics,
 * every sum has a fixed order and two runs give the same bits.  The trunk's kernels are those of the temporal discriminator
 * (csrc/i2v_res3d_trunk.h).  Activations are channels-last [N][T][H][W][C]; the clips come and their gradient leaves as [N][3][T][H][W]. */
#ifndef I2V_HIP_ENC3D_TRAIN_H
#define I2V_HIP_ENC3D_TRAIN_H

#include "i2v_hip_disc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_enc3d_train i2v_enc3d_train;

typedef struct {
    int32_t z_dim;         /* width of mu and logvar, any positive integer */
    int32_t channels[5];   /* stem width and the four layer widths, each a multiple of 16 */
    int32_t stride_s[4];   /* spatial stride of block 0 of each layer, 1 or 2 */
    int32_t stride_t[4];   /* temporal stride of block 0 of each layer, 1 or 2 */
    int32_t use_max_pool;  /* refused, as by i2v_encoder3d_create */
} i2v_enc3d_train_cfg;

#define I2V_ENC3D_TRAIN_SAVE 1 /* keep in `saved` what i2v_enc3d_train_backward needs */

/* kinds of i2v_enc3d_train_saved_layout */
#define I2V_ENC3D_TRAIN_CONV_OUT 0 /* a conv's output, before its GroupNorm: fp32 */
#define I2V_ENC3D_TRAIN_ACT 1      /* behind the GroupNorm (and the residual add and ReLU where the network has them): fp32 */

/* I2V_E_INVALID before anything else happens: z_dim < 1, a width that is not a positive multiple of 16, a stride outside {1, 2},
 * use_max_pool, or a layer with stride_t 2, stride_s 1 and equal widths (it has no downsample branch for its half-rate residual: the
 * branch exists iff stride_s != 1 or the widths differ, resnet3D.py:184). */
int i2v_enc3d_train_create(const i2v_enc3d_train_cfg* cfg, i2v_enc3d_train** out);
void i2v_enc3d_train_destroy(i2v_enc3d_train* e);
/* params[i].data: DEVICE pointer of the tensor with state_dict key params[i].name -- conv1.weight, norm1.{weight,bias},
 * layer.L.i.conv{1,2}.weight, layer.L.i.bn{1,2}.{weight,bias}, layer.L.0.downsample.{0.weight,1.weight,1.bias},
 * conv_mu.{weight,bias}, conv_var.{weight,bias}.  Read in place by every call; nothing is copied or packed on the host. */
int i2v_enc3d_train_bind(i2v_enc3d_train* e, const i2v_tensor* params, int32_t n);
/* The gradient tensors of the parameters under the same keys (DEVICE pointers); grads NULL with n = 0: none bound. */
int i2v_enc3d_train_bind_grads(i2v_enc3d_train* e, const i2v_tensor* grads, int32_t n);
/* shape[0 .. 3] = (t, h, w, c) of the trunk's last map for clips of t frames of h x w.  I2V_E_INVALID, with the map in the message,
 * unless it is [1, 4, 4] (conv_mu and conv_var are 4 x 4 convolutions of one frame). */
int i2v_enc3d_train_out_shape(const i2v_enc3d_train* e, int32_t t, int32_t h, int32_t w, int32_t* shape);
/* 0 for a shape that is refused. */
size_t i2v_enc3d_train_saved_bytes(const i2v_enc3d_train* e, int32_t n, int32_t t, int32_t h, int32_t w);
size_t i2v_enc3d_train_workspace_bytes(const i2v_enc3d_train* e, int32_t n, int32_t t, int32_t h, int32_t w);
/* Where the maps of a forward with I2V_ENC3D_TRAIN_SAVE lie, for the tests: entry e < *count is the map of kind[e] of conv conv[e]
 * (order: stem; per layer block 0 conv1, conv2, downsample if any, block 1 conv1, conv2), dims[4 e ..] = (t, h, w, c),
 * [n][t][h][w][c] at byte offset[e] of `saved`.  Arrays of 64.  A host function. */
int i2v_enc3d_train_saved_layout(const i2v_enc3d_train* e, int32_t n, int32_t t, int32_t h, int32_t w, int32_t* count, int32_t* kind,
                                 int32_t* conv, int32_t* dims, int64_t* offset);
/* Encoder.forward behind the transpose: x [n][3][t][h][w] -> mu, logvar [n][z] and, with eps [n][z] (NULL: none), sample =
 * eps * exp(0.5 logvar) + mu (NULL without eps).  With I2V_ENC3D_TRAIN_SAVE, `saved` takes the maps, the GroupNorm statistics, the
 * operand layouts of the weights, eps, mu and logvar; else it may be NULL. */
int i2v_enc3d_train_forward(i2v_enc3d_train* e, const float* x, const float* eps, int32_t n, int32_t t, int32_t h, int32_t w, int32_t flags,
                            float* sample, float* mu, float* logvar, void* saved, size_t saved_bytes, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Backward of the forward that filled `saved`: d_sample, d_mu, d_logvar [n][z] (NULL: zero; d_sample needs a forward with eps) and
 * kl_scale, which adds kl_scale * d KL / d (mu, logvar) with KL = -0.5 mean_n sum_j (1 + lv - mu^2 - e^lv): mu / n and
 * (e^lv - 1) / (2 n) -> d_x [n][3][t][h][w] (NULL: not wanted) and, with param_grads, the gradient of every bound parameter, written
 * or (accumulate) added.  The GroupNorm weights and conv_mu / conv_var are read from the bound parameters when the backward runs.
 * Without d_x and param_grads, or with neither an upstream gradient nor kl_scale: I2V_E_INVALID. */
int i2v_enc3d_train_backward(i2v_enc3d_train* e, const float* d_sample, const float* d_mu, const float* d_logvar, float kl_scale,
                             const void* saved, size_t saved_bytes, int32_t n, int32_t t, int32_t h, int32_t w, float* d_x,
                             int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* d_mu = scale * mu / n, d_logvar = scale * (e^logvar - 1) / (2 n) over [n][z], formed in float64 and rounded once: the gradient of
 * `scale * KL` on its own, for the autograd form of loss.KL. */
int i2v_enc3d_kl_backward(const float* mu, const float* logvar, int32_t n, int32_t z, float scale, float* d_mu, float* d_logvar, void* stream);

/* ---- the posterior head's kernels one at a time, from raw DEVICE tensors, for the tests.  emb [n][16][c] channels-last (the [1, 4, 4]
 * map), weights [z][c][4][4] and biases [z] in the reference's layout; c a multiple of 16, n and z any positive integers. ---- */
size_t i2v_enc3d_head_workspace_bytes(int32_t n, int32_t c, int32_t z);
/* mu, logvar [n][z] (one GEMM [n x 16 c] . [16 c x 2 z] in c / 16 slices of K, added in slice order, plus the bias) and, with eps,
 * sample. */
int i2v_enc3d_head_forward_unit(const float* emb, const float* w_mu, const float* b_mu, const float* w_var, const float* b_var, const float* eps,
                                int32_t n, int32_t c, int32_t z, float* sample, float* mu, float* logvar, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The head's backward from emb, the weights, the forward's mu, logvar and eps (NULL with d_sample NULL) and the upstream gradients
 * (each NULL: zero) with kl_scale as above -> d_emb [n][16][c] and, where dw_mu is given (all four or none), dw_mu, db_mu, dw_var,
 * db_var, written or (accumulate) added. */
int i2v_enc3d_head_backward_unit(const float* emb, const float* w_mu, const float* w_var, const float* mu, const float* logvar, const float* eps,
                                 const float* d_sample, const float* d_mu, const float* d_logvar, float kl_scale, int32_t n, int32_t c,
                                 int32_t z, float* d_emb, float* dw_mu, float* db_mu, float* dw_var, float* db_var, int32_t accumulate,
                                 void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
