/* libi2v_hip.so -- the spatial (patch) discriminator of stage-1 training: NLayerDiscriminator, stage1_VAE/modules/patch_disc.py:101-165,
 * with spectral norm in training mode, ActNorm with its data-dependent init, the backward pass and the hinge loss of
 * stage1_VAE/modules/loss.py:24-32, 111-125 (csrc/i2v_patchdisc.hip).
 *
 * A header of its own next to i2v_hip.h: that header's declarations are counted by the tests of the handle layer, and a training
 * component that nothing of the sampling path needs does not belong to its table.  Same conventions: plain device pointers, calls only
 * enqueue on `stream`, 0 = ok and I2V_E_* otherwise, i2v_last_error() for the message.
 *
 * Exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32), no atomics: every sum has a fixed order and two runs give the same bits.
 * Activations are channels-last [N][H][W][C]; the frames come and their gradient leaves as [N][3][H][W]. */
#ifndef I2V_HIP_DISC_H
#define I2V_HIP_DISC_H

#include "i2v_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct i2v_patchdisc i2v_patchdisc;

typedef struct {
    int32_t in_channels;   /* 3 (anything else is refused) */
    int32_t ndf;           /* 64 in every shipped config; a multiple of 16 */
    int32_t n_layers;      /* 3: the net has n_layers + 2 convolutions; 1..6 */
    int32_t use_actnorm;   /* 1; 0 (BatchNorm2d) is refused: not built */
    int32_t spectral_norm; /* 1: every conv is wrapped in torch.nn.utils.spectral_norm; 0: the same code with sigma = 1 */
} i2v_patchdisc_cfg;

#define I2V_PATCHDISC_ITERATE 1      /* one power iteration per conv first, in place on u and v (training mode) */
#define I2V_PATCHDISC_INIT_ACTNORM 2 /* every ActNorm sets loc and scale from its input first (patch_disc.py:28-47) */
#define I2V_PATCHDISC_SAVE 4         /* keep in `saved` what i2v_patchdisc_backward needs */

#define I2V_HINGE_DISC 0
#define I2V_HINGE_GEN 1

/* I2V_E_INVALID before anything else happens: ndf % 16 != 0, in_channels != 3, use_actnorm = 0, n_layers outside 1..6. */
int i2v_patchdisc_create(const i2v_patchdisc_cfg* cfg, i2v_patchdisc** out);
void i2v_patchdisc_destroy(i2v_patchdisc* d);
/* params[i].data: DEVICE pointer of the tensor with state_dict key params[i].name -- main.{i}.{bias, weight_orig, weight_u, weight_v}
 * (without spectral norm: main.{i}.{bias, weight}) and main.{j}.{loc, scale}.  Read and, for u, v, loc and scale, updated in place;
 * nothing is copied or packed on the host. */
int i2v_patchdisc_bind(i2v_patchdisc* d, const i2v_tensor* params, int32_t n);
/* The gradient tensors of bias, weight_orig / weight, loc and scale under the same keys (DEVICE pointers), bound apart from the
 * parameters: a caller with a fresh gradient buffer per backward re-binds these alone.  grads NULL with n = 0: none bound. */
int i2v_patchdisc_bind_grads(i2v_patchdisc* d, const i2v_tensor* grads, int32_t n);
/* [n][3][h][w] -> [n][1][ho][wo]; I2V_E_INVALID when a map shrinks below 1 x 1 (the short side must be >= 3 * 2^n_layers). */
int i2v_patchdisc_out_shape(const i2v_patchdisc* d, int32_t h, int32_t w, int32_t* ho, int32_t* wo);
/* 0 for a shape that is refused. */
size_t i2v_patchdisc_saved_bytes(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w);
size_t i2v_patchdisc_workspace_bytes(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w);
/* Where the activations of a forward with I2V_PATCHDISC_SAVE lie, for the tests: per conv i < *nconv the output map ho[i] x wo[i] x
 * cout[i] and the byte offsets in `saved` of its activation (behind ActNorm and LeakyReLU) and of its pre-ActNorm output, each
 * [n][ho][wo][cout] fp32; -1 where there is none (the last conv; a conv without ActNorm).  Arrays of 8.  A host function. */
int i2v_patchdisc_saved_layout(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w, int32_t* nconv, int32_t* ho, int32_t* wo, int32_t* cout,
                               int64_t* act_offset, int64_t* pre_offset);
/* NLayerDiscriminator.forward (patch_disc.py:163-165).  flags: I2V_PATCHDISC_*.  With I2V_PATCHDISC_SAVE, `saved` takes the
 * activations, the pre-ActNorm conv outputs, the normalised weights and this call's u, v and sigma; else it may be NULL. */
int i2v_patchdisc_forward(i2v_patchdisc* d, const float* x, int32_t n, int32_t h, int32_t w, int32_t flags, float* pred, void* saved,
                          size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* (From `saved` the backward takes the activations, the packed W / sigma and that forward's u, v and sigma.  weight_orig -- for the
 * projection --, loc and scale are read from the bound parameters when the backward runs: a parameter that changes between a forward and
 * its backward, an optimiser step between two saved forwards' backwards for instance, gives an inconsistent gradient without an error.) */
/* Backward of the forward that filled `saved`: d_pred [n][1][ho][wo] -> d_x [n][3][h][w] (NULL: not wanted) and, with param_grads,
 * the gradient of every bound parameter, written or (accumulate) added.  Without either there is nothing to do: I2V_E_INVALID. */
int i2v_patchdisc_backward(i2v_patchdisc* d, const float* d_pred, const void* saved, size_t saved_bytes, int32_t n, int32_t h, int32_t w,
                           float* d_x, int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);
/* hinge_loss (loss.py:24-32) with its gradient, one workgroup, float64 sums in a fixed order.  I2V_HINGE_DISC: out[0] =
 * (mean relu(1 - real) + mean relu(1 + fake)) / 2, out[1] = mean(real), out[2] = mean(fake); d_real = -[real < 1] / (2 numel),
 * d_fake = [fake > -1] / (2 numel).  I2V_HINGE_GEN: out[0] = -mean(fake), out[2] = mean(fake), d_fake = -1 / numel; real, d_real
 * unused.  out: 3 doubles on the device. */
int i2v_patchdisc_hinge(const float* fake, const float* real, int64_t numel, int32_t mode, double* out, float* d_fake, float* d_real,
                        void* stream);
/* The split of the weight gradient's position range, a pure function of the shape: `slices` workgroups per output tile, each over
 * `slice_len` positions (a multiple of 16; the last slice is masked). */
int i2v_patchdisc_wgrad_plan(int32_t cout, int32_t cin, int64_t positions, int32_t* slices, int32_t* slice_len);

/* ---- one kernel at a time, from raw DEVICE tensors, for the tests.  weight [cout][cin][4][4]; maps channels-last; cin = 3 reads
 * and writes 4-channel maps; cout % 16 == 0, cin == 3 or cin % 16 == 0; stride 1 or 2; pad 1. ---- */
/* (cout = 1: the workspace of i2v_patchdisc_head_unit) */
size_t i2v_patchdisc_unit_workspace_bytes(int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout);
/* y = conv(x) + bias -> pre (optional); then scale * (y + loc) when loc is given; then LeakyReLU(0.2) when asked -> out */
int i2v_patchdisc_conv_unit(const float* x, const float* weight, const float* bias, const float* loc, const float* scale, int32_t n, int32_t hi,
                            int32_t wi, int32_t cin, int32_t cout, int32_t stride, int32_t lrelu, float* out, float* pre, void* workspace,
                            size_t workspace_bytes, void* stream);
/* g [n][ho][wo][cout] times (act > 0 ? 1 : 0.2) when act is given, times scale[c] when scale is given -> out [n][hi][wi][cin];
 * cin = 3: out [n][hi][wi][4], or with frames_out [n][3][hi][wi]. */
int i2v_patchdisc_dgrad_unit(const float* g, const float* weight, const float* act, const float* scale, int32_t n, int32_t hi, int32_t wi,
                             int32_t cin, int32_t cout, int32_t stride, float* out, int32_t frames_out, void* workspace,
                             size_t workspace_bytes, void* stream);
/* dweight [cout][cin][4][4] and dbias [cout] from g (masked and scaled as above) and the conv's input x; with u [cout], v [cin * 16]
 * and sigma [1] the spectral-norm projection (dWn - <dWn, W / sigma> u v^T) / sigma is applied. */
int i2v_patchdisc_wgrad_unit(const float* g, const float* act, const float* scale, const float* x, const float* weight, const float* u,
                             const float* v, const float* sigma, int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout,
                             int32_t stride, int32_t accumulate, float* dweight, float* dbias, void* workspace, size_t workspace_bytes,
                             void* stream);
/* The cout = 1 conv (stride 1): out [n][hi-1][wi-1] = conv(x) + bias; with g (same shape) also dx [n][hi][wi][cin], dweight
 * [1][cin][4][4] and dbias [1]. */
int i2v_patchdisc_head_unit(const float* x, const float* weight, const float* bias, const float* g, int32_t n, int32_t hi, int32_t wi,
                            int32_t cin, float* out, float* dx, float* dweight, float* dbias, void* workspace, size_t workspace_bytes,
                            void* stream);
/* weight [rows][cols]; iterate: v <- normalize(W^T u), u <- normalize(W v) in place; sigma [1] = u . (W v). */
int i2v_patchdisc_power_iteration_unit(const float* weight, float* u, float* v, int32_t rows, int32_t cols, int32_t iterate, float* sigma,
                                       void* workspace, size_t workspace_bytes, void* stream);
/* pre [m][c] -> loc [c] = -mean, scale [c] = 1 / (unbiased std + 1e-6), float64 sums */
int i2v_patchdisc_actnorm_init_unit(const float* pre, int64_t m, int32_t c, float* loc, float* scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
