/* libi2v_hip.so -- what the TRAINING path of the stage-1 Generator (stage1_VAE/modules/decoder.py:55-120) needs between and around its six
 * GeneratorBlocks (i2v_hip_gblock_train.h, unchanged): `fc` with its backward, the nearest up-sampling with its adjoint, and the image head
 * tanh(conv_img(lrelu_0.2(x))) with its backward (csrc/i2v_gen_train.hip).  The module composes them in Python.
 *
 * A sixth header with a table of its own (i2v_native.GEN_TRAIN_SYMBOLS).  Conventions of i2v_hip_gblock_train.h: plain device pointers, calls
 * only enqueue on `stream`, 0 = ok and I2V_E_* otherwise, i2v_last_error() for the message; exact fp32, no atomics, every sum has a fixed
 * order and two runs give the same bits; writes stay inside the caller's buffers and their prior contents do not matter.  The surface is the
 * reference's [B][C][T][H][W]; the frames leave as [B][T][3][H][W].  The head's three conv passes run on the kernels of the 3-D ResNet
 * training trunk (csrc/i2v_train_conv.h) as the passes of the ADJOINT conv 3 -> nf. */
#ifndef I2V_HIP_GEN_TRAIN_H
#define I2V_HIP_GEN_TRAIN_H

#include "i2v_hip_gblock_train.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_gen_train i2v_gen_train;

#define I2V_GEN_TRAIN_SAVE 1 /* keep in `saved` what i2v_gen_train_head_backward needs */

/* I2V_E_INVALID before a device is looked for: the channel factor nf must be a multiple of 16 with 16 nf <= 1024 (the GeneratorBlocks
 * take channel counts that are multiples of 16), z_dim >= 1. */
int i2v_gen_train_create(int32_t nf, int32_t z_dim, i2v_gen_train** out);
void i2v_gen_train_destroy(i2v_gen_train* g);
/* params[i].data: DEVICE pointer of the tensor with state_dict key params[i].name -- fc.{weight,bias} ([256 nf][z_dim], [256 nf]) and
 * conv_img.{weight,bias} ([3][nf][3][3][3], [3]).  Read in place by every call; nothing is copied or packed on the host. */
int i2v_gen_train_bind(i2v_gen_train* g, const i2v_tensor* params, int32_t n);
/* The gradient tensors of the parameters under the same keys (DEVICE pointers); grads NULL with n = 0: none bound. */
int i2v_gen_train_bind_grads(i2v_gen_train* g, const i2v_tensor* grads, int32_t n);

/* ---- sizes: functions of the shape alone; 0 for a shape that is refused ---- */
/* fc backward from `batch` rows of j outputs over k inputs */
size_t i2v_gen_train_fc_workspace_bytes(int32_t batch, int32_t j, int32_t k);
size_t i2v_gen_train_head_saved_bytes(int32_t nf, int32_t batch, int32_t t, int32_t h, int32_t w);
size_t i2v_gen_train_head_workspace_bytes(int32_t nf, int32_t batch, int32_t t, int32_t h, int32_t w);
/* the slices of j that the fc backward's dz adds in slice order */
int32_t i2v_gen_train_fc_slices(int32_t j);

/* ---- the module's calls, on the bound parameters ---- */
/* out [batch][256 nf] = fc.bias + z [batch][z_dim] . fc.weight^T; [batch][16 nf][1][4][4] is a view of it */
int i2v_gen_train_fc_forward(i2v_gen_train* g, const float* z, int32_t batch, float* out, void* stream);
/* g_out [batch][256 nf] -> dz [batch][z_dim] (NULL: not wanted) and, with param_grads, the gradients of fc.weight and fc.bias, written or
 * (accumulate) added.  Nothing wanted: I2V_E_INVALID. */
int i2v_gen_train_fc_backward(i2v_gen_train* g, const float* g_out, const float* z, int32_t batch, float* dz, int32_t param_grads, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream);
/* x [batch][nf][t][h][w] -> out [batch][t][3][h][w] = tanh(conv_img(lrelu(x))).  flags: I2V_GEN_TRAIN_SAVE (then `saved` takes lrelu(x)
 * channels-last and the frames; else it may be NULL). */
int i2v_gen_train_head_forward(i2v_gen_train* g, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t flags, float* out, void* saved,
                               size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* g_out [batch][t][3][h][w] -> dx [batch][nf][t][h][w] (NULL: not wanted) and, with param_grads, the gradients of conv_img.weight and
 * conv_img.bias; without param_grads no weight-gradient kernel is launched. */
int i2v_gen_train_head_backward(i2v_gen_train* g, const float* g_out, const void* saved, size_t saved_bytes, int32_t batch, int32_t t, int32_t h,
                                int32_t w, float* dx, int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- nearest up-sampling by (ut, us, us), each of ut, us in {1, 2, 4}; `planes` = batch x channels maps of t x h x w (the LOW resolution) ---- */
/* out [planes][ut t][us h][us w]: out[.., T, H, W] = x[.., T / ut, H / us, W / us] */
int i2v_gen_train_upsample_forward(const float* x, int64_t planes, int32_t t, int32_t h, int32_t w, int32_t ut, int32_t us, float* out, void* stream);
/* dx [planes][t][h][w] = the sum of the ut us us gradients of g [planes][ut t][us h][us w] in fp32 in (dt, dh, dw) order */
int i2v_gen_train_upsample_backward(const float* g, int64_t planes, int32_t t, int32_t h, int32_t w, int32_t ut, int32_t us, float* dx, void* stream);

/* ---- the same kernels from raw DEVICE tensors, for the tests ---- */
/* w [j][k], bias [j], z [batch][k] -> out [batch][j] */
int i2v_gen_train_fc_forward_unit(const float* z, const float* w, const float* bias, int32_t batch, int32_t j, int32_t k, float* out, void* stream);
/* g [batch][j] -> dw [j][k], db [j], dz [batch][k] (each NULL: not wanted) */
int i2v_gen_train_fc_backward_unit(const float* g, const float* z, const float* w, int32_t batch, int32_t j, int32_t k, int32_t accumulate, float* dw,
                                   float* db, float* dz, void* workspace, size_t workspace_bytes, void* stream);
/* w [3][nf][3][3][3], bias [3]; saved NULL: nothing kept */
int i2v_gen_train_head_forward_unit(const float* x, const float* w, const float* bias, int32_t nf, int32_t batch, int32_t t, int32_t h, int32_t w_,
                                    float* out, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* dx, dw [3][nf][3][3][3] and db [3]: each NULL is not wanted; dw and db come together */
int i2v_gen_train_head_backward_unit(const float* g, const void* saved, size_t saved_bytes, const float* w, int32_t nf, int32_t batch, int32_t t,
                                     int32_t h, int32_t w_, int32_t accumulate, float* dx, float* dw, float* db, void* workspace,
                                     size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
