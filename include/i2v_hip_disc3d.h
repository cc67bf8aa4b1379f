/* libi2v_hip.so -- the temporal discriminator of stage-1 training: resnet3D.Discriminator (stage1_VAE/modules/resnet3D.py:222-301), a
 * 3-D ResNet-18 with GroupNorm(16) and spectral norm on block 0 of every layer, with its backward pass, the feature-map loss
 * (loss.py:14-21) and the pieces of the step of loss.py:94-109, 127-137 (csrc/i2v_disc3d.hip).
 *
 * A third header next to i2v_hip.h and i2v_hip_disc.h, with a table of its own (i2v_native.DISC3D_SYMBOLS).  Same conventions: plain
 * device pointers, calls only enqueue on `stream`, 0 = ok and I2V_E_* otherwise, i2v_last_error() for the message.
 *
 * Exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32), no atomics: every sum has a fixed order and two runs give the same bits.
 * Activations are channels-last [N][T][H][W][C]; the clips come and their gradient leaves as [N][3][T][H][W]. */
#ifndef I2V_HIP_DISC3D_H
#define I2V_HIP_DISC3D_H

#include "i2v_hip_disc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_disc3d i2v_disc3d;

typedef struct {
    int32_t res_type;      /* 18 (res_type_encoder 'resnet18': two BasicBlocks per layer); anything else is refused */
    int32_t channels[5];   /* stem width and the four layer widths, each a multiple of 16 */
    int32_t stride_s[4];   /* spatial stride of block 0 of each layer, 1 or 2 */
    int32_t stride_t[4];   /* temporal stride of block 0 of each layer, 1 or 2 */
    int32_t use_max_pool;  /* MaxPool3d(3, stride (1, 2, 2), pad 1) behind the stem */
    int32_t spectral_norm; /* conv1 / conv2 of block 0 of each layer are spectral-normed; the downsample convs always are */
} i2v_disc3d_cfg;

#define I2V_DISC3D_ITERATE 1 /* one power iteration per spectral-normed conv first, in place on u and v (training mode) */
#define I2V_DISC3D_SAVE 2    /* keep in `saved` what i2v_disc3d_backward needs */

#define I2V_FMAP_L1 0
#define I2V_FMAP_L2 1

/* kinds of i2v_disc3d_saved_layout */
#define I2V_DISC3D_CONV_OUT 0    /* a conv's output, before its GroupNorm: fp32 */
#define I2V_DISC3D_ACT 1         /* behind the GroupNorm (and the residual add and ReLU where the network has them): fp32 */
#define I2V_DISC3D_POOL_OUT 2    /* the max pool's output: fp32 */
#define I2V_DISC3D_POOL_ARGMAX 3 /* per pooled element the (t * H + h) * W + w of the maximum within its sample's input map: int32 */

/* I2V_E_INVALID before anything else happens: res_type != 18, a width that is not a positive multiple of 16, a stride outside {1, 2}. */
int i2v_disc3d_create(const i2v_disc3d_cfg* cfg, i2v_disc3d** out);
void i2v_disc3d_destroy(i2v_disc3d* d);
/* params[i].data: DEVICE pointer of the tensor with state_dict key params[i].name -- conv1.weight, norm1.{weight,bias},
 * layer.L.0.conv{1,2}.{weight_orig,weight_u,weight_v} (spectral_norm 0: .weight), layer.L.1.conv{1,2}.weight,
 * layer.L.i.bn{1,2}.{weight,bias}, layer.L.0.downsample.0.{weight_orig,weight_u,weight_v}, layer.L.0.downsample.1.{weight,bias},
 * fc.weight.  Read in place and, for u and v, updated in place; nothing is copied or packed on the host. */
int i2v_disc3d_bind(i2v_disc3d* d, const i2v_tensor* params, int32_t n);
/* The gradient tensors of the parameters under the same keys (DEVICE pointers); grads NULL with n = 0: none bound. */
int i2v_disc3d_bind_grads(i2v_disc3d* d, const i2v_tensor* grads, int32_t n);
/* shapes[4 L .. 4 L + 3] = (t, h, w, c) of feature map L for clips of t frames of h x w.  I2V_E_INVALID, with the map in the message,
 * unless the network ends on a [1, 4, 4] map (fc takes exactly channels[4] features). */
int i2v_disc3d_out_shape(const i2v_disc3d* d, int32_t t, int32_t h, int32_t w, int32_t* shapes);
/* 0 for a shape that is refused. */
size_t i2v_disc3d_saved_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w);
size_t i2v_disc3d_workspace_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w);
/* Where the maps of a forward with I2V_DISC3D_SAVE lie, for the tests: entry e < *count is the map of kind[e] (I2V_DISC3D_*) of conv
 * conv[e] (order: stem; per layer block 0 conv1, conv2, downsample if any, block 1 conv1, conv2; -1 for the pool's), dims[4 e ..] =
 * (t, h, w, c), [n][t][h][w][c] at byte offset[e] of `saved`.  Arrays of 64.  A host function. */
int i2v_disc3d_saved_layout(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w, int32_t* count, int32_t* kind, int32_t* conv,
                            int32_t* dims, int64_t* offset);
/* Discriminator.forward behind the transpose (resnet3D.py:287-301): x [n][3][t][h][w] -> pred [n] and, where fmaps and fmaps[L] are
 * given, feature map L [n][t][h][w][c] (channels-last).  flags: I2V_DISC3D_*.  With I2V_DISC3D_SAVE, `saved` takes the maps, the
 * GroupNorm statistics, the pool's argmax, the normalised weights and this call's u, v and sigma; else it may be NULL. */
int i2v_disc3d_forward(i2v_disc3d* d, const float* x, int32_t n, int32_t t, int32_t h, int32_t w, int32_t flags, float* pred, float* const* fmaps,
                       void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the forward that filled `saved`: d_pred [n] (NULL: zero) and d_fmaps[L] (channels-last; d_fmaps or an entry NULL: zero)
 * -> d_x [n][3][t][h][w] (NULL: not wanted) and, with param_grads, the gradient of every bound parameter, written or (accumulate)
 * added.  u, v, sigma and W / sigma are those of that forward; weight_orig (the projection) and the GroupNorm weights are read from the
 * bound parameters when the backward runs.  Without d_x and param_grads, or without any upstream gradient: I2V_E_INVALID. */
int i2v_disc3d_backward(i2v_disc3d* d, const float* d_pred, const float* const* d_fmaps, const void* saved, size_t saved_bytes, int32_t n,
                        int32_t t, int32_t h, int32_t w, float* d_x, int32_t param_grads, int32_t accumulate, void* workspace,
                        size_t workspace_bytes, void* stream);
/* fmap_loss (loss.py:14-21) over n_layers <= 4 pairs of maps of numel[L] elements, float64 sums in a fixed order: out[0] = mean over
 * the layers of mean |a - b| (I2V_FMAP_L2: of mean (a - b)^2), out[1 + L] the layer's own mean.  With d_a, d_a[L] = grad_scale *
 * sign(a - b) / (numel[L] n_layers), sign(0) = 0 (L2: grad_scale * 2 (a - b) / ...).  out: 5 doubles on the device; workspace:
 * i2v_disc3d_fmap_loss_workspace_bytes(). */
size_t i2v_disc3d_fmap_loss_workspace_bytes(void);
int i2v_disc3d_fmap_loss(const float* const* a, const float* const* b, const int64_t* numel, int32_t n_layers, int32_t metric, float grad_scale,
                         double* out, float* const* d_a, void* workspace, size_t workspace_bytes, void* stream);
/* out[i] = sum of x[i][0 .. per)^2 in float64, i < n: the per-sample squared norm of the gradient penalty's value. */
int i2v_disc3d_sumsq(const float* x, int32_t n, int64_t per, double* out, void* stream);
/* The split of the weight gradient's position range, a pure function of the shape: `slices` workgroups per output tile and tap, each
 * over `slice_len` positions (a multiple of 16; the last slice is masked).  taps: 27, or 147 for the stem. */
int i2v_disc3d_wgrad_plan(int32_t cout, int32_t cin, int32_t taps, int64_t positions, int32_t* slices, int32_t* slice_len);

/* ---- one kernel at a time, from raw DEVICE tensors, for the tests.  weight [cout][cin][3][kh][kw] with kh = kw = 3 pad 1, or (stem) 7
 * pad 3; maps channels-last; cin = 3 reads and writes 4-channel maps; cout % 16 == 0, cin == 3 or cin % 16 == 0; strides 1 or 2. ---- */
size_t i2v_disc3d_unit_workspace_bytes(int32_t n, int32_t ti, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem);
int i2v_disc3d_conv_unit(const float* x, const float* weight, int32_t n, int32_t ti, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem,
                         int32_t stride_t, int32_t stride_s, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* g [n][to][ho][wo][cout], times [act > 0] when act is given -> out [n][ti][hi][wi][cin], plus add (times [add_mask > 0] when given)
 * when add is given; cin = 3: out has 4 channels, or with frames_out is [n][3][ti][hi][wi]. */
int i2v_disc3d_dgrad_unit(const float* g, const float* weight, const float* act, const float* add, const float* add_mask, int32_t n, int32_t ti,
                          int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem, int32_t stride_t, int32_t stride_s, float* out,
                          int32_t frames_out, void* workspace, size_t workspace_bytes, void* stream);
/* dweight [cout][cin][3][kh][kw] from g (masked as above) and the conv's input x; with u [cout], v [cin * taps] and sigma [1] the
 * spectral-norm projection (dWn - <dWn, W / sigma> u v^T) / sigma is applied. */
int i2v_disc3d_wgrad_unit(const float* g, const float* act, const float* x, const float* weight, const float* u, const float* v, const float* sigma,
                          int32_t n, int32_t ti, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem, int32_t stride_t,
                          int32_t stride_s, int32_t accumulate, float* dweight, void* workspace, size_t workspace_bytes, void* stream);
/* GroupNorm(16, c, eps 1e-5) over x [n][positions][c]: stats [n][16][2] float64 (mean, 1 / sqrt(var + eps)); out = norm(x) * weight +
 * bias (+ res) (ReLU when asked).  workspace: i2v_disc3d_groupnorm_workspace_bytes(n, c). */
size_t i2v_disc3d_groupnorm_workspace_bytes(int32_t n, int32_t c);
int i2v_disc3d_groupnorm_unit(const float* x, const float* res, const float* weight, const float* bias, int32_t n, int64_t positions, int32_t c,
                              int32_t relu, float* out, double* stats, void* workspace, size_t workspace_bytes, void* stream);
/* g at the norm's (activated) output, times [mask > 0] when mask is given -> dx; dweight, dbias (both or neither), written or added. */
int i2v_disc3d_groupnorm_backward_unit(const float* g, const float* mask, const float* x, const double* stats, const float* weight, int32_t n,
                                       int64_t positions, int32_t c, float* dx, float* dweight, float* dbias, int32_t accumulate, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* MaxPool3d(3, stride (1, 2, 2), pad 1): x [n][t][h][w][c] -> out [n][t][ho][wo][c] and argmax (I2V_DISC3D_POOL_ARGMAX; the first
 * maximum in (t, h, w) scan order). */
int i2v_disc3d_maxpool_unit(const float* x, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, float* out, int32_t* argmax, void* stream);
/* dx[i] = sum of g over the windows whose argmax is i, gathered in (t, h, w) order of the windows. */
int i2v_disc3d_maxpool_backward_unit(const float* g, const int32_t* argmax, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, float* dx,
                                     void* stream);
/* AvgPool3d((1, 4, 4)) + fc: x [n][16][c], weight [c] -> pred [n]; with g [n] also dx [n][16][c] and (when given) dweight [c]. */
int i2v_disc3d_head_unit(const float* x, const float* weight, const float* g, int32_t n, int32_t c, float* pred, float* dx, float* dweight,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
