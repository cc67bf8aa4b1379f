/* libi2v_hip.so -- C ABI of the MI355X-native (gfx950) cINN-sampling + VAE-decoder hot path.
 *
 * The reference (CompVis/image2video-synthesis-using-cINNs) is pure PyTorch and has no FFI of
 * its own: the boundary it offers is the Python class surface.  This header is
 * the NEW native boundary underneath that surface; each entry point names the reference
 * method (file:line relative to the reference repo) whose arithmetic it replaces.  The Python
 * mirror of the reference classes (image2video-synthesis-using-cinns_amd/...) calls these via
 * ctypes, see INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.
 *   - "host tensors" (i2v_tensor) are read during *_load only and are not retained.
 *   - all pointers passed to the compute calls are DEVICE pointers owned by the caller (PyTorch
 *     allocates inputs, outputs and the workspace); the library owns only its packed weights.
 *   - compute calls only ENQUEUE on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and never synchronise.  A handle is bound to the device current at create time,
 *     is not re-entrant, and must be used from one stream at a time.
 *   - return value: 0 = ok, negative = error (I2V_E_*); i2v_last_error() gives the message of
 *     the last failure on the calling thread.
 *   - *_load may be called again to replace the weights.  A load that fails (I2V_E_MISSING, a
 *     failed upload, ...) leaves the handle UNLOADED, whatever it held before: part of the
 *     packed weights may already be the new ones, so every call that needs weights returns
 *     I2V_E_STATE until a load succeeds.  This holds for every handle type.
 */
#ifndef I2V_HIP_H
#define I2V_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define I2V_OK 0
#define I2V_E_INVALID (-1)   /* bad argument / unsupported configuration */
#define I2V_E_MISSING (-2)   /* a state_dict key is missing or has the wrong size */
#define I2V_E_HIP (-3)       /* a HIP runtime call failed */
#define I2V_E_WORKSPACE (-4) /* workspace too small */
#define I2V_E_STATE (-5)     /* weights not loaded (never, or the last load failed) */
#define I2V_E_RANGE (-6)     /* an activation left the fp16 range of the split-fp16 operand format (see i2v_dec_status) */

#define I2V_F32 0
#define I2V_I64 1
#define I2V_U8 2

/* One named host tensor of a PyTorch state_dict (contiguous). */
typedef struct {
    const char* name;  /* state_dict key, e.g. "sub_layers.3.coupling.s.0.main.2.weight" */
    const void* data;  /* HOST pointer */
    int64_t numel;
    int32_t dtype;     /* I2V_F32 / I2V_I64 / I2V_U8 */
} i2v_tensor;

const char* i2v_last_error(void);
int i2v_version(void);
/* Number of HIP devices visible; <0 on error.  Used by the Python side to fail loudly. */
int i2v_device_count(void);

/* ------------------------------------------------------------------------------------------
 * cINN flow: ConditionalFlow (stage2_cINN/modules/flow_blocks.py:8-60)
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_flow i2v_flow;

typedef struct {
    int32_t in_channels;   /* 64 (flow_blocks.py:13); the kernels map channel <-> wavefront lane */
    int32_t embedding_dim; /* E (+30 with control), flow_blocks.py:14 */
    int32_t hidden_dim;    /* 512 = z_dim * flow_mid_channels_factor, get_model.py:34 */
    int32_t hidden_depth;  /* 2, flow_blocks.py:16 */
    int32_t n_flows;       /* 20 */
    int32_t control;       /* 1: blocks fl%4 != 0 run in mode 'cond' (flow_blocks.py:24); 2: every block does */
    int32_t activation;    /* 1 = InvLeakyRelu(0.9) (default), 0 = IgnoreLeakyRelu */
    int32_t skip_actnorm;  /* 1: no ActNorm  (used to expose the bare coupling block, :63-105) */
    int32_t skip_shuffle;  /* 1: no Shuffle */
    int32_t use_graph;     /* 1: replay the launch chain from a captured hipGraph */
    int32_t linear_f16;    /* 1: fp16-operand mode of the s- / t-net Linear layers (BASELINE configs[4]: "fp16 MFMA conditioning
                            * GEMM"): weights rounded to fp16 once at load, activations per layer, v_mfma_f32_16x16x16_f16 with fp32
                            * accumulation; bias, LeakyReLU, coupling and log-det stay fp32.  NOT within the 1e-4 fp32 gate (z rel-L2
                            * ~1e-3); 0 (default): exact fp32 matrix cores.  Needs the tile-chain geometry. */
} i2v_flow_cfg;

int i2v_flow_create(const i2v_flow_cfg* cfg, i2v_flow** out);
void i2v_flow_destroy(i2v_flow* f);
/* Packs the 80 MLPs, ActNorm and Shuffle parameters of ConditionalFlow.state_dict() into the
 * streaming layout and uploads them.  Keys: sub_layers.{i}.{norm_layer.{loc,scale},
 * coupling.{s,t}.{0,1}.main.{0,2,4,6}.{weight,bias}, shuffle.{forward,backward}_shuffle_idx}. */
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_flow_load(i2v_flow* f, const i2v_tensor* tensors, int32_t n_tensors);
size_t i2v_flow_workspace_bytes(const i2v_flow* f, int32_t batch);
/* Bytes of parameters streamed per pass (the algorithmic HBM traffic of SURVEY §8d). */
size_t i2v_flow_param_bytes(const i2v_flow* f);
/* Host-only query of what a pass at `batch` launches on a LOADED handle (nothing is launched): chain 0 = the generic vector-ALU
 * chain, 1 = the matrix-core tile chain; for the tile chain kpw = k-blocks per wave (hidden / 128), ns = sample tiles per
 * hidden-layer workgroup (1, 2 or 4) and fold = 1 when the tail travels with the first hidden layer's launch -- the values
 * the launcher itself uses; 0, 0, 0 for the generic chain.  I2V_E_INVALID: null argument or batch <= 0. */
int i2v_flow_plan(const i2v_flow* f, int32_t batch, int32_t* chain, int32_t* kpw, int32_t* ns, int32_t* fold);
/* ConditionalFlow.forward(x, embedding, reverse=False), flow_blocks.py:42-51.
 * x [B,64], embed [B,E] -> zt [B,64], logdet [B]. */
int i2v_flow_forward(i2v_flow* f, const float* x, const float* embed, float* zt, float* logdet,
                     void* workspace, size_t workspace_bytes, int32_t batch, void* stream);
/* ConditionalFlow.forward(x, embedding, reverse=True), flow_blocks.py:53-57. */
int i2v_flow_inverse(i2v_flow* f, const float* residual, const float* embed, float* z,
                     void* workspace, size_t workspace_bytes, int32_t batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * cINN flow, training path (stage2_cINN/main.py:22-46: forward, FlowLoss, loss.backward(), optimizer.step())
 *
 * A second handle next to i2v_flow: it packs nothing.  The parameters are read in place, in their state_dict layout,
 * through DEVICE pointers bound once, so an optimiser step on them is seen by the next forward without a re-load.
 * Exact fp32 matrix cores only; every gradient element has one owner and a fixed summation order (no atomics):
 * the same inputs give the same bits.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_flow_train i2v_flow_train;
/* Same cfg as the inference handle (control 0 / 1 / 2, activation, skip_actnorm, skip_shuffle; use_graph is ignored).
 * Refused with I2V_E_INVALID: linear_f16 = 1, and any geometry outside 64 channels, hidden 128..512 in steps of 128,
 * depth >= 1, embedding <= 128. */
int i2v_flow_train_create(const i2v_flow_cfg* cfg, i2v_flow_train** out);
void i2v_flow_train_destroy(i2v_flow_train* f);
/* params[i].data: DEVICE pointer of the tensor with state_dict key params[i].name (the keys of i2v_flow_load; the
 * Shuffle indices as I2V_I64, bound once and not trained).  grads: one entry per trained tensor under the same key; its
 * `data` is either the device pointer of the gradient tensor, or a BYTE OFFSET into one flat gradient buffer whose base
 * is passed to each backward call (a caller that allocates a fresh flat buffer per backward never re-binds).  Nothing is
 * copied; all pointers / offsets must be 16-byte aligned. */
int i2v_flow_train_bind(i2v_flow_train* f, const i2v_tensor* params, const i2v_tensor* grads, int32_t n);
/* Size of the `saved` buffer of one forward / backward pair: MLP inputs, hidden activations, s / t of every half-step
 * and the backward's pre-activation gradients (about 1 MB per sample at 20 flows, hidden 512, depth 2). */
size_t i2v_flow_train_saved_bytes(const i2v_flow_train* f, int32_t batch);
/* Where each region of `saved` lies, in floats, for tests that check one kernel at a time.  Per half-step st, at
 * st * step_sz: xs [B][64] at 0, cin [B][KP] at o_cin, act [2][depth + 1][B][H] at o_act, out [2][B][32] at o_out, dpre
 * (shaped like act) at o_dpre, dout [2][B][32] at o_dout; then once: xin [n_flows][B][64] at o_xin, gan (same shape) at
 * o_gan, part [B][64] at o_part, dcin [B][KP] at o_dcin.  A host function: no handle, no device call.  I2V_E_INVALID for
 * a geometry i2v_flow_train_create refuses. */
typedef struct {
    int64_t KP, step_sz, o_cin, o_act, o_out, o_dpre, o_dout, o_xin, o_gan, o_part, o_dcin, total;
} i2v_flow_train_layout;
int i2v_flow_train_saved_layout(int32_t hidden, int32_t depth, int32_t embedding_dim, int32_t n_flows, int32_t batch,
                                i2v_flow_train_layout* out);
/* ConditionalFlow.forward(x, embedding), flow_blocks.py:42-51, keeping in `saved` what the backward needs:
 * x [B,64], embed [B,E] -> zt [B,64], logdet [B]. */
int i2v_flow_train_forward(i2v_flow_train* f, const float* x, const float* embed, float* zt, float* logdet, void* saved,
                           size_t saved_bytes, int32_t batch, void* stream);
/* Backward of that forward from the same `saved`: given d_zt [B,64] and d_logdet [B], writes (accumulate = 1: adds to)
 * the gradient of every trained parameter at (char*)grad_base + grads[i].data (grad_base NULL: plain pointers were
 * bound), and d_x [B,64], d_embed [B,E] when non-null.  Linear layers: dX = dY W on the chain, dW = dY^T X and
 * db = sum_b dY behind it; affine coupling flow_blocks.py:88-93 (ds = dy x exp(s) + d_logdet, dt = dy, dx = dy exp(s),
 * conditioner gradient into the kept half and the embedding); ActNorm modules.py:80-89 (d_scale includes
 * sum_b d_logdet[b] / scale); InvLeakyRelu with its reported log-det of 0 (flow_blocks.py:176-182); Shuffle as the
 * inverse gather. */
int i2v_flow_train_backward(i2v_flow_train* f, const float* d_zt, const float* d_logdet, void* saved, size_t saved_bytes,
                            float* d_x, float* d_embed, void* grad_base, int32_t accumulate, int32_t batch, void* stream);

/* One tensor of a fused optimiser step: device pointers, max_exp_avg_sq may be null without amsgrad. */
typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* max_exp_avg_sq;
    int64_t numel;
} i2v_adam_tensor;
/* Elements of one workgroup's chunk in the chunk list below. */
int32_t i2v_adam_chunk(void);
/* torch.optim.Adam.step over a DEVICE table of tensors in one launch (the reference trains with lr 1e-5,
 * betas (0.9, 0.99), weight_decay 0, amsgrad, stage2_cINN/configs): L2 weight_decay added to the gradient, bias
 * corrections from `step` (the count after this step, >= 1), eps outside the square root.  chunks: device array of
 * n_chunks pairs (table index, first element); every tensor is covered by ceil(numel / chunk) pairs. */
int i2v_adam_step(const i2v_adam_tensor* table, const int32_t* chunks, int32_t n_chunks, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int32_t amsgrad, int64_t step, void* stream);

/* ------------------------------------------------------------------------------------------
 * Leaf modules of the flow, individually callable (sub-module classes stay usable)
 * ---------------------------------------------------------------------------------------- */
/* BasicFullyConnectedNet (stage2_cINN/modules/modules.py:9-30): Linear(dim,hidden) -> LeakyReLU(0.01) ->
 * depth x [Linear(hidden,hidden) -> LeakyReLU(0.01)] -> Linear(hidden,out_dim).  Keys main.{0,2,...}.{weight,bias}. */
typedef struct i2v_mlp i2v_mlp;
int i2v_mlp_create(int32_t dim, int32_t hidden_dim, int32_t depth, int32_t out_dim, i2v_mlp** out);
void i2v_mlp_destroy(i2v_mlp* m);
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_mlp_load(i2v_mlp* m, const i2v_tensor* tensors, int32_t n_tensors);
size_t i2v_mlp_workspace_bytes(const i2v_mlp* m, int32_t batch);
/* x [B,dim] -> y [B,out_dim] */
int i2v_mlp_forward(i2v_mlp* m, const float* x, float* y, void* workspace, size_t workspace_bytes, int32_t batch,
                    void* stream);

/* Per-channel elementwise ops on a contiguous [B][C][inner] tensor. */
#define I2V_OP_ACTNORM_FWD 0  /* out = p1[c] * (x + p0[c])        ActNorm.forward, modules.py:80 (p0 = loc, p1 = scale) */
#define I2V_OP_ACTNORM_REV 1  /* out = x / p1[c] - p0[c]          ActNorm.reverse, modules.py:100 */
#define I2V_OP_INVLRELU_FWD 2 /* out = x * (x >= 0 ? 1 : alpha)   InvLeakyRelu.forward, flow_blocks.py:180-181 */
#define I2V_OP_INVLRELU_REV 3 /* out = x / (x >= 0 ? 1 : alpha)   InvLeakyRelu.reverse, flow_blocks.py:185-186 */
#define I2V_OP_GATHER 4       /* out[b,c] = x[b, idx[c]]          Shuffle, flow_blocks.py:152-154 (idx: device int64) */
int i2v_channel_op(int32_t op, const float* x, float* out, int32_t batch, int32_t channels, int32_t inner,
                   const float* p0, const float* p1, const int64_t* idx, float alpha, void* stream);
/* Per-row mean and unbiased std of x [rows][n] (ActNorm.initialize, modules.py:43-63). */
int i2v_row_mean_std(const float* x, int32_t rows, int32_t n, float* mean, float* std, void* stream);
/* out[b] = hw * sum_c log|scale[c]| for b < batch (ActNorm log-det, modules.py:86-88). */
int i2v_actnorm_logdet(const float* scale, int32_t channels, float hw, float* out, int32_t batch, void* stream);

/* Measurement helper (no reference counterpart; used by bench.py only): enqueues an MFMA-only loop -- `workgroups` x 512
 * threads, `iters` k-steps of 12 v_mfma_f32_32x32x16_f16 per wavefront on live pseudo-random register operands, no
 * memory traffic -- and returns the fp16 MFMA FLOPs it executes in *flops.  Timed by the caller with events on `stream`,
 * it gives the matrix-core rate the chip SUSTAINS under power management, next to the data-sheet peak.
 * scratch: device buffer of workgroups * 512 floats. */
int i2v_probe_mfma_f16(int32_t workgroups, int32_t iters, float* scratch, double* flops, void* stream);


/* ------------------------------------------------------------------------------------------
 * Stage-1 decoder: Generator (stage1_VAE/modules/decoder.py:55-120)
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_dec i2v_dec;

typedef struct {
    int32_t channel_factor; /* nf, decoder.py:59 (multiple of 8) */
    int32_t z_dim;          /* 64 */
    int32_t upsample_s[2];  /* decoder.py:66 */
    int32_t upsample_t[2];  /* decoder.py:67 */
    int32_t spectral_norm;  /* decoder.py:64 */
    int32_t mma;            /* 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32); 1 = split-fp16 3-term MFMA; 2 = auto: split-fp16 with a
                             * per-layer fallback to the exact-fp32 kernels behind the range guard -- both weight sets are packed, every
                             * forward synchronises its stream, looks at the operand maxima the writers published, switches the 3x3x3 convs
                             * whose operand left the window the split format holds 1e-4 in (for the life of the handle) and runs the call
                             * again; a checkpoint inside the window runs exactly the launches of mma = 1 (i2v_dec_fallback_layers);
                             * 3 = "fp16": opt-in half precision -- the launches of mma = 1, except that the 3x3x3 block convs on the
                             * Winograd F(4,3) kernel run its one-term form (conv_wino4_f16_kernel: fp16 operands, ONE MFMA per product,
                             * fp32 accumulation) on an operand rounded to fp16 once; not an fp32 emulation: frames within ~1e-3 relative
                             * L2 of the fp32 reference, measured tolerances in INTEGRATION.md §3.  Not combined with auto. */
} i2v_dec_cfg;

int i2v_dec_create(const i2v_dec_cfg* cfg, i2v_dec** out);
void i2v_dec_destroy(i2v_dec* d);
/* Folds W/sigma (signed sigma = u.(W_mat v), torch spectral_norm eval semantics, hook at
 * decoder.py:20-25), re-lays every conv for the implicit-GEMM kernels and uploads.  Keys as in
 * Generator.state_dict(): fc.*, {head_0,g_0..g_4}.{conv_0,conv_1,conv_s}.{weight_orig,weight_u,
 * weight_v,bias} (or .weight when spectral_norm = 0), .norm_0.{conv,conv_gamma,conv_beta}.*,
 * .norm_1.linear.*, .norm_s.bn.*, conv_img.*. */
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_dec_load(i2v_dec* d, const i2v_tensor* tensors, int32_t n_tensors);
/* Output geometry [T, H, W] of one decoder pass (T = 16 for every shipped config). */
int i2v_dec_out_shape(const i2v_dec* d, int32_t* t, int32_t* h, int32_t* w);
size_t i2v_dec_workspace_bytes(const i2v_dec* d, int32_t batch, int32_t img_h, int32_t img_w);
double i2v_dec_flops_per_sample(const i2v_dec* d, int32_t img_h, int32_t img_w);
/* Generator.forward(img, motion), decoder.py:97-120.
 * img [B,3,img_h,img_w] (NCHW, [-1,1]), motion [B,z_dim] -> out [B,T,3,H,W] contiguous. */
int i2v_dec_forward(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, const float* motion,
                    float* out, void* workspace, size_t workspace_bytes, int32_t batch, void* stream);
/* The same with explicit SAMPLE strides (in floats; 0 = dense) for the start frames and the output: img sample b starts at
 * img + b * img_bstride (its [3,img_h,img_w] planes stay contiguous), out sample b at out + b * out_bstride (its [T,3,H,W]
 * block stays contiguous).  This is what the autoregressive loop of Model.forward (get_model.py:68-73) needs to run without
 * torch.cat / .contiguous() copies: pass k decodes straight into frames [16k, 16k+16) of ONE pre-allocated
 * [B, vid_length, 3, H, W] buffer (out = buf + 16k * 3*H*W, out_bstride = vid_length * 3*H*W) and pass k+1 reads its start
 * frames seq[:, -1] from the same buffer (img = buf + (16k + 15) * 3*H*W, img_bstride = vid_length * 3*H*W). */
int i2v_dec_forward_strided(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int64_t img_bstride,
                            const float* motion, float* out, int64_t out_bstride, void* workspace, size_t workspace_bytes,
                            int32_t batch, void* stream);
/* Optional first half of Generator.forward: the SPADE conditioning branches of all six blocks (normalization_layer.py:20-23:
 * F.interpolate(start frame) -> Conv2d(3,128) + lrelu -> conv_gamma | conv_beta).  They depend on the start frame only, not on
 * the motion latent, so a caller can enqueue them on a SIDE stream while the cINN pass that produces the latent runs
 * (get_model.py:59-66), and then call i2v_dec_forward with the SAME img pointer, size, batch and workspace (after making its
 * stream wait for the side stream): that forward skips the branches and reads the prepared gamma | beta maps from the
 * workspace.  One prepare serves AT MOST the next forward call on the handle: every i2v_dec_forward* entry -- matching or not,
 * successful or not (I2V_E_RANGE of the previous call, bad arguments, workspace too small) -- consumes or discards it before
 * anything else.  The identity test is by address: the CONTENTS of img must not change between the prepare and its forward;
 * a caller that refills the buffer in place calls i2v_dec_prepare_cancel (the Python binding does, keyed on the tensor's
 * version counter).  Same kernels, same bits.
 * Since round 5 the branches are enqueued on a side stream the HANDLE owns, ordered behind everything already on `stream` (an event),
 * and the consuming forward waits per level (events): the caller's stream stays free, e.g. for the cINN pass, and needs no stream
 * of its own for this.  (While `stream` captures a graph, with I2V_DEC_OVERLAP=0 or the debug tap on they run inline on `stream`.)
 * A forward WITHOUT prepared maps forks its own branches the same way, underneath its first levels.
 * LIFETIME CONTRACT of a prepare that ran on the side stream: `workspace` and `img` must stay allocated and unmodified until the
 * NEXT i2v_dec_forward* / i2v_dec_prepare / i2v_dec_join call on the handle has been enqueued -- each of them either consumes the
 * prepared maps (waiting per level) or makes its stream wait for the whole side stream before it does anything else, so from then
 * on synchronising THAT stream bounds the lifetime of both buffers again.  A caller that wants to release or reuse them without
 * another forward calls i2v_dec_join(d, stream) and orders the release behind `stream`.  i2v_dec_destroy synchronises the side
 * stream.  Graph capture: a forward captured on `stream` runs everything inline (no side stream, no cross-stream events); a prepare
 * that was forked BEFORE the capture began is dropped by it (join it with i2v_dec_join before capturing). */
int i2v_dec_prepare(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, void* workspace, size_t workspace_bytes,
                    int32_t batch, void* stream);
/* Realizations: F start frames, K samples per frame -- sample f*K + k is realization k of frame f (rows frame-major, the
 * realization index fastest).  img holds the F frames ([F,3,img_h,img_w], frame stride img_bstride: 0 = dense), motion the F*K
 * latents [F*K][z_dim], out receives F*K samples (out_bstride as for i2v_dec_forward_strided).  The result equals
 * i2v_dec_forward_strided on the frames repeated K times (repeat_interleave), bit for bit, in every mode; the SPADE conditioning
 * branches -- they depend on the start frame only -- run once per FRAME, and every SPADE-consuming operand writer reads map row
 * sample / K.  The workspace holds the gamma | beta maps and the SPADE scratch for F frames, everything else for F*K samples:
 * i2v_dec_workspace_bytes_realizations(F, K) <= i2v_dec_workspace_bytes(F*K), equal for K = 1.  K = 1 runs the launches of
 * i2v_dec_forward_strided.  i2v_dec_prepare_realizations is i2v_dec_prepare for such a call (dense frames [F,3,img_h,img_w]); it
 * serves the next forward only when address, F, K, size and workspace all match, under the rules of i2v_dec_prepare above.
 * Debug tap 0 (gamma | beta) returns the F frame maps.  No reference counterpart (the reference repeats the frames). */
size_t i2v_dec_workspace_bytes_realizations(const i2v_dec* d, int32_t frames, int32_t realizations, int32_t img_h, int32_t img_w);
int i2v_dec_forward_realizations(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int64_t img_bstride, int32_t frames,
                                 int32_t realizations, const float* motion, float* out, int64_t out_bstride, void* workspace,
                                 size_t workspace_bytes, void* stream);
int i2v_dec_prepare_realizations(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int32_t frames, int32_t realizations,
                                 void* workspace, size_t workspace_bytes, void* stream);
/* Drops a pending prepare (no-op without one). */
int i2v_dec_prepare_cancel(i2v_dec* d);
/* Makes `stream` wait for everything the handle has enqueued on its own side stream (a forked i2v_dec_prepare that no forward has
 * consumed) and drops the pending prepare: behind this call `stream` bounds the lifetime of the workspace / start frames again.
 * No reference counterpart (the reference has one stream: generate_samples.py:47-54). */
int i2v_dec_join(i2v_dec* d, void* stream);
/* The handle's side work (SPADE conditioning branches, learned shortcuts, i2v_dec_prepare) runs on `side_stream` instead of a stream
 * the handle creates -- typically the stream the caller's cINN prefetch already runs on, so that a job uses main + ONE side stream
 * (+ its collation stream) next to RCCL's: HIP multiplexes streams onto four hardware queues, and streams that share a queue
 * serialise.  `side_stream` stays the caller's (it must outlive the handle or be reset with NULL: the handle then creates its own
 * again).  Same kernels, same events, same bits.  No reference counterpart (the reference has one stream). */
int i2v_dec_set_side_stream(i2v_dec* d, void* side_stream);
/* mma = 2 (auto): which 3x3x3 convs the range guard has switched to the exact-fp32 kernels so far: bit 2 * block + (0: conv_0, 1: conv_1),
 * blocks head_0, g_0 .. g_4; bit 30: the whole handle (an overflow outside the conv operands: SPADE's activation, a shortcut, conv_img).
 * reruns (optional): forwards that were run a second time because a layer had to be switched.  Always 0 / 0 for mma = 0, 1.
 * No reference counterpart (the reference computes in fp32 throughout: decoder.py:99-120). */
int i2v_dec_fallback_layers(i2v_dec* d, int32_t* mask, int32_t* reruns);
/* Roofline instrumentation.  With profiling on, every 3x3x3 Conv3d launch (the dominant kernel) is bracketed by HIP
 * events recorded on the launch stream -- no synchronisation is added to the forward.  After the caller has
 * synchronised, i2v_dec_get_profile resolves the pending pairs and returns the totals since set_profile(d, 1):
 * summed kernel time [ms], summed algorithmic FLOPs (2*M*N*K of the reference's conv per launch), summed matrix-core
 * FLOPs actually issued (3 per product in split-fp16 mode, 18 of 27 taps in temporal-duplication mode) and launches. */
int i2v_dec_set_profile(i2v_dec* d, int32_t on);
int i2v_dec_get_profile(i2v_dec* d, double* conv3_ms, double* conv3_flops, double* conv3_mfma_flops, int64_t* conv3_launches);
/* The same totals per layer: layer = 2 * block + {0: conv_0, 1: conv_1}, block 0..5 = head_0, g_0 .. g_4 (decoder.py:74-79).
 * name receives "<block>.conv_<i>"; kernel: 0 = exact-fp32 MFMA implicit GEMM (direct), 1 = split-fp16 direct, 2 = split-fp16
 * Winograd F(2,3), 3 = split-fp16 Winograd F(4,3), 4 = split-fp16 F(4,3) with the operand generated in the kernel,
 * 5 = exact-fp32 Winograd F(4,3), 6 = one-term fp16 Winograd F(4,3) (mma = 3: one MFMA product per product is counted). */
int i2v_dec_get_layer_profile(i2v_dec* d, int32_t layer, char* name, int32_t name_len, double* ms, double* flops,
                              double* mfma_flops, int64_t* launches, int32_t* kernel);
/* Test hook: during the next forwards copy up to max_floats of one channels-last intermediate of GeneratorBlock
 * `block` (0 = head_0 .. 5 = g_4) into dst (device).  which: 0 = SPADE (1+gamma | beta) [B,H,W,2C], 1 = lrelu(Spade(x)),
 * 2 = conv_0 output, 3 = lrelu(ADAIN(.)), 4 = shortcut (low resolution), 5 = block output.  dst = NULL disables. */
/* Range guard of the split-fp16 ("hl16") operand format (mma = 1): the kernels that produce conv operands raise a sticky
 * device flag when a value is non-finite or exceeds the fp16 range (|x| > 65504 -- a regime no synthetic-weight parity
 * test reaches, but a released checkpoint with a large SPADE (1 + gamma) might).  Nothing synchronises on the fast path:
 * every i2v_dec_forward ends with an async copy of the flag to pinned host memory, and the NEXT i2v_dec_forward (or
 * i2v_gblock_forward) on the handle returns I2V_E_RANGE when it finds it set.  i2v_dec_status synchronises `stream`, reads
 * the flag (bit 0 = overflow seen) and optionally clears it; use mma = 0 (exact fp32 MFMA) for such checkpoints.
 * Bit 1 (value 2) = UNDERFLOW warning: the format has an absolute error floor of ~2^-25 (the lo part is an fp16 subnormal
 * below |x| = 2^-3), so a conv whose whole operand tensor lies below 2^-10 no longer holds the 1e-4 gate (measured table:
 * INTEGRATION.md §3).  The two operand writers of every block (the inputs of conv_0 and conv_1: 12 tensors per forward) publish
 * the largest |activation| they wrote; a non-zero tensor whose maximum is below 2^-10 sets bit 1.  Coverage, as built: the
 * maximum is per operand TENSOR over the whole batch (one normal sample hides an underflowing one in the same call), and SPADE's
 * internal 128-channel operand, the EPI_HL16 conv epilogue and conv_img's input are not watched (they carry bit 0 only).  It is reported by i2v_dec_status only (sticky until reset) and does NOT make the next call fail:
 * the output is finite and merely less precise; mma = 0 is exact there too.
 * mma = 3 ("fp16"): the same status word and the same writers' guard.  Bit 0: a value of a conv operand left the fp16 range (the
 * one-term operand holds exactly the split format's hi parts, so the same values overflow) -- the output is invalid, use mma = 0 or
 * auto.  Bit 1 keeps its trigger (a non-zero operand tensor whose maximum is below 2^-10) and means for this format: the operand
 * reaches towards fp16's subnormal range (below 2^-14), where the one-term values lose relative precision beyond the mode's normal
 * ~2^-12 per value; a warning, as in mma = 1. */
int i2v_dec_status(i2v_dec* d, int32_t* flags, int32_t reset, void* stream);

/* Test hook: during every following forward, copy one intermediate of block `block` (0 = head_0 .. 5 = g_4) into `dst` (device,
 * min(size of the intermediate, max_floats) floats, enqueued on the forward's stream where the data is complete and before its
 * buffer is reused); dst = null switches the hook off.  With a tap set the SPADE branches and the learned shortcut run inline on the
 * caller's stream and the operand-generating F(4,3) kernel (I2V_DEC_GEN) is not used; nothing else changes -- with no tap set, launch
 * order and bits are those of a build without the hook.  Activations are channels-last fp32.  `which`:
 *    0  SPADE's (1 + gamma | beta) maps [F][H][W][2 n_in]
 *    1  the WHOLE operand conv_0's writer wrote, in the format of the kernel the layer runs (i2v_dec_get_layer_profile's code):
 *         fp32 direct             [B][T][H][W][C] fp32
 *         split-fp16 direct       [B][T][H][W][C/8][8 fp16 hi | 8 fp16 lo]   (a temporal-duplication conv_0: T / 2 frames, here and below)
 *         split-fp16 F(2,3) V     [B][T][C/16][4 planes][H][W/2][c 0-7 hi | lo | c 8-15 hi | lo]      2 floats per activation
 *         split-fp16 F(4,3) V     [B][T][C/16][6 planes][H][W/4][c 0-7 hi | lo | c 8-15 hi | lo]      3/2 floats per activation
 *         one-term fp16 F(4,3) V  [B][T][CinPad/32][6][H][W/4][c 0-7 | 16-23 | 8-15 | 24-31], CinPad = C rounded up to 64
 *         exact-fp32 F(4,3) V     [6 planes][B][T][H][W/4][C] fp32                                    3/2 floats per activation
 *    2  conv_0's output (with its bias) [B][T][H][W][n_mid]
 *    3  the whole operand of conv_1, as 1
 *    4  the learned shortcut at the block input's resolution [B][T/ut][H/us][W/us][n_out] (learned blocks only)
 *    5  the block output [B][T][H][W][n_out] (g_4: lrelu(.), fused into conv_1's epilogue)
 *    6  the (sum, sumsq) fp64 pairs [B][n_mid] ADAIN's coefficients are derived from (conv_0's epilogue or the statistics kernel
 *       filled them), copied as bytes: 4 floats per pair, here and in 7 and 8
 *    7  the fp64 pairs [B][n_out] of the block output, ONLY where conv_1's epilogue accumulated them (else nothing is copied)
 *    8  the fp64 pairs [B][n_in] of the block input as this block reads them (the previous block's epilogue or the statistics kernel)
 *    9  the (A, B) float2 table [B][n_in] handed to conv_0's operand writer (SPADE's group norm: norm(x) = x A + B)
 *   10  the (A, B) table [B][n_mid] handed to conv_1's operand writer (ADAIN: gamma norm(x) + beta = x A + B)
 *   11  the (A, B) table [B][n_in] of the learned shortcut's Norm3D (learned blocks only)
 *   12  the block input [B][T/ut][H/us][W/us][n_in]
 *   13  SPADE's branch: the start frames resized to the level (bilinear, align_corners) as 16-channel rows [F][H][W][16], channels 3 .. 15
 *       zero: fp32, or split-fp16 rows [8 fp16 hi | 8 fp16 lo] x 2 where the branch runs split-fp16 kernels (forms 0 .. 2 below)
 *   14  SPADE's branch: lrelu(Conv2d(3, 128)(.)) [F][H][W][128]: fp32 (forms 0, 1, 3) or the split-fp16 direct operand (form 2), as tap 1
 *   15  SPADE's branch, forms 0 and 1 only: the Winograd operand of tap 14, as tap 1 with T = 1 and C = 128 */
#define I2V_DEC_TAP_LAST 15
int i2v_dec_debug_tap(i2v_dec* d, int32_t block, int32_t which, float* dst, size_t max_floats);
/* The form SPADE's branch of `block` took in the last forward / prepare: 0 = split-fp16 F(4,3) gamma | beta conv, 1 = split-fp16 F(2,3),
 * 2 = direct split-fp16 (the activation handed over in the operand format by the first conv's epilogue), 3 = exact fp32; -1 = not run yet. */
int i2v_dec_get_spade_form(i2v_dec* d, int32_t block, int32_t* form);

/* Test hooks: the decoder's units outside the blocks, through the functions the decoder itself calls.  Both pack `weight` / `bias`
 * (host, float32), run on `stream` and synchronise it before they return.
 * i2v_conv_img_unit: conv_img (decoder.py:117-120): x channels-last [b][t][h][w][c] (device) -> tanh(Conv3d(c -> 3, 3x3x3, pad 1)) as frames
 * [b][t][3][h][w], out_bstride floats between samples (0: dense).  weight [3][c][3][3][3], bias [3].  form: -1 = what a split-fp16
 * (mma = 1) decoder of this output geometry runs, 0 = fused matrix-core kernel (c in 16, 32, 48, 64; h % 8 == 0, w % 32 == 0),
 * 1 = transposed 81-column split-fp16 GEMM + gather (c >= 64; the decoder under I2V_DEC_IMG16=1), 2 = vector-ALU kernel, exact fp32
 * (t, h, w % 8 == 0, c % 4 == 0), 3 = the generic implicit-GEMM conv, exact fp32 (t, h, w that tile into its 128-position bricks: powers of two).  A named form whose predicate refuses
 * the geometry returns I2V_E_INVALID.  form_used: the form that ran; tch: output frames per workgroup of form 0 (else 0); range_flag:
 * the split-fp16 forms' overflow flag after the run (all optional).
 * i2v_pointwise_unit: out[m][cout] = act((in[m][cin] * A + B) @ weight^T + bias + res): in / res / out (device), weight [cout][cin] and
 * bias [cout] or null (host), coef = (A, B) float2 table [m / p rows][cin] (device) or null, p = rows per sample.  split16: 1 = the
 * split-fp16 GEMM (the decoder's shortcut in mma = 1), 0 = the exact-fp32 GEMM.  transposed (split16 only, no res / coef): out[cout][m].
 * tile_n: columns of the 128-row tile that ran (128, 64 or 32). */
int i2v_conv_img_unit(const float* x, const float* weight, const float* bias, int32_t b, int32_t t, int32_t h, int32_t w, int32_t c, int32_t form,
                      float* out, int64_t out_bstride, int32_t* form_used, int32_t* tch, int32_t* range_flag, void* stream);
int i2v_pointwise_unit(const float* in, const float* weight, const float* bias, const float* res, const float* coef, float* out, int64_t m,
                       int64_t p, int32_t cin, int32_t cout, int32_t lrelu, int32_t split16, int32_t transposed, int32_t* tile_n,
                       int32_t* range_flag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Decoder sub-modules, individually callable with the reference's [B][C][T][H][W] tensors:
 * GeneratorBlock (decoder.py:7-52), Spade / Norm3D / ADAIN (normalization_layer.py:5-51).
 * T, H, W must be powers of two (>= 1) so the convolutions tile into bricks.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_gblock i2v_gblock;
/* mma: 0 (exact fp32), 1 (split-fp16) or 3 (fp16, see i2v_dec_cfg.mma); a block has no re-run loop, so there is no auto mode.  A learned shortcut (n_in != n_out)
 * needs n_in % 16 == 0: its Norm3D is GroupNorm(16, n_in).  Both return I2V_E_INVALID otherwise. */
int i2v_gblock_create(int32_t n_in, int32_t n_out, int32_t z_dim, int32_t spectral_norm, int32_t mma, i2v_gblock** out);
void i2v_gblock_destroy(i2v_gblock* g);
/* Keys relative to the block: conv_{0,1,s}.*, norm_0.{conv,conv_gamma,conv_beta}.*, norm_1.linear.*, norm_s.bn.*.
 * Groups of keys that are absent are skipped, so a handle can carry a lone Spade / ADAIN / Norm3D. */
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_gblock_load(i2v_gblock* g, const i2v_tensor* tensors, int32_t n_tensors);
size_t i2v_gblock_workspace_bytes(const i2v_gblock* g, int32_t batch, int32_t t, int32_t h, int32_t w);
/* GeneratorBlock.forward(x, cond1 = z, cond2 = img): x [B,n_in,T,H,W] -> out [B,n_out,T,H,W]. */
int i2v_gblock_forward(i2v_gblock* g, const float* x, const float* z, const float* img, int32_t img_h, int32_t img_w,
                       float* out, void* workspace, size_t workspace_bytes, int32_t batch, int32_t t, int32_t h, int32_t w,
                       void* stream);
/* The block's own range guard (see i2v_dec_status): synchronises `stream`, returns the sticky flag word of the split-fp16
 * operand writers of this handle (bit 0 = an operand left the fp16 range) and optionally clears it. */
int i2v_gblock_status(i2v_gblock* g, int32_t* flags, int32_t reset, void* stream);
/* part 0: Spade.forward(x, cond = img [B,3,img_h,img_w]); part 1: ADAIN.forward(x [B,n_mid,...], cond = z [B,z_dim]);
 * part 2: Norm3D.forward(x).  Output has the shape of x. */
int i2v_gblock_norm(i2v_gblock* g, int32_t part, const float* x, const float* cond, int32_t img_h, int32_t img_w, float* out,
                    void* workspace, size_t workspace_bytes, int32_t batch, int32_t t, int32_t h, int32_t w, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conditioning embedder (row N1): ResnetEncoder.encode(x).mode() -- stage2_cINN/AE/modules/AE.py:91-166,
 * distributions.py:41-42.  torchvision-0.8.1 ResNet-50 with InstanceNorm2d (use_batchnorm = 0) or eval-mode
 * BatchNorm2d (1), fc = Conv2d(2048, 2E, 1); returns the posterior mean [B, E].
 * Keys: model.conv1.weight, model.layer{1..4}.{i}.conv{1,2,3}.weight, model.layer{k}.0.downsample.0.weight,
 * (BatchNorm) model.bn1.*, ...bn{1,2,3}.*, ...downsample.1.* {weight,bias,running_mean,running_var},
 * model.fc.sub_layers.0.{weight,bias}.  Image side must be a power of two >= 64.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_embedder i2v_embedder;
int i2v_embedder_create(int32_t z_dim, int32_t use_batchnorm, i2v_embedder** out);
void i2v_embedder_destroy(i2v_embedder* e);
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_embedder_load(i2v_embedder* e, const i2v_tensor* tensors, int32_t n_tensors);
size_t i2v_embedder_workspace_bytes(const i2v_embedder* e, int32_t batch, int32_t h, int32_t w);
/* img [B,3,h,w] in [-1,1] (NCHW) -> embed [B, z_dim] */
int i2v_embedder_forward(i2v_embedder* e, const float* img, int32_t h, int32_t w, float* embed, void* workspace,
                         size_t workspace_bytes, int32_t batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * FVD feature network: the Kinetics-400 I3D -- metrics/PyTorch_FVD/I3D.py (I3D.forward :273-299, Unit3Dpy :48-131,
 * MaxPool3dTFPadding :134-154, Mixed :157-191) with the host preprocessing of metrics/PyTorch_FVD/FVD_logging.py:190-206
 * (bilinear align_corners=True resize to 224 x 224, denorm) fused into its input stage.  rgb only (in_channels = 3).
 * Keys (the reference state_dict as it is): conv3d_1a_7x7.conv3d.weight, ....batch3d.{weight,bias,running_mean,running_var},
 * conv3d_2b_1x1.*, conv3d_2c_3x3.*, mixed_{3b,3c,4b..4f,5b,5c}.branch_0.*, .branch_1.{0,1}.*, .branch_2.{0,1}.*, .branch_3.1.*,
 * conv3d_0c_1x1.conv3d.{weight,bias}; num_batches_tracked is ignored.  Eval-mode BatchNorm3d (eps 1e-3) is folded into a
 * per-channel scale and shift at load.  Exact fp32 matrix cores; there is no reduced-precision mode.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_i3d i2v_i3d;
/* I3D.__init__ (I3D.py:194-271) */
int i2v_i3d_create(int32_t num_classes, int32_t in_channels, i2v_i3d** out);
void i2v_i3d_destroy(i2v_i3d* n);
/* Module.load_state_dict of the reference module (FVD_logging.load_model :208-214) */
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_i3d_load(i2v_i3d* n, const i2v_tensor* tensors, int32_t n_tensors);
size_t i2v_i3d_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t, int32_t h, int32_t w);
/* FVD_logging.preprocess + I3D.forward: frames [B][t][3][h][w] fp32 (the decoder's output layout), denorm != 0: the values are
 * in [-1, 1] and are mapped by (x + 1) / 2 after the resize -> logits [B][num_classes] (out_logits; FVD does not use the
 * softmax).  t >= 9.  Only enqueues on `stream`: no synchronisation, no environment reads. */
int i2v_i3d_forward(i2v_i3d* n, const float* frames, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t denorm, float* logits,
                    void* workspace, size_t workspace_bytes, void* stream);
/* The input stage of i2v_i3d_forward alone (FVD_logging.preprocess :190-206): frames [n_frames][3][h][w] -> channels-last
 * [n_frames][224][224][4] (channel 3 zero), bilinear align_corners=True, (x + 1) / 2 when denorm != 0.  For tests and inspection. */
int i2v_i3d_input_stage(const float* frames, int32_t n_frames, int32_t h, int32_t w, int32_t denorm, float* out, void* stream);
/* Streaming form of FVD_logging.calculate_activation_statistics (:152-174): sum [d] and gram [d][d] (float64, device) +=
 * the n rows of feats [n][d] fp32.  One owner per output element, the rows in order, no atomics: two runs give the same bits. */
int i2v_fvd_stats_update(const float* feats, int32_t n, int32_t d, double* sum, double* gram, void* stream);

/* ------------------------------------------------------------------------------------------
 * DTFVD / diversity feature network: the dynamic-texture I3D -- metrics/DTFVD/ID3.py (length 16) and ID3_32.py (length 32):
 * InceptionI3D.get_representation :351-358, Unit3D :48-119, MaxPool3dSamePadding :12-42, InceptionModule :125-181.  A second
 * variant on the i2v_i3d handle; what differs from the Kinetics network:
 *   keys      Conv3d_1a_7x7.conv3d.weight, .bn.{weight,bias,running_mean,running_var}, Conv3d_2b_1x1.*, Conv3d_2c_3x3.*,
 *             Mixed_{3b,3c,4b..4f,5b,5c}.{b0,b1a,b1b,b2a,b2b,b3b}.*, logits.conv3d.{weight,bias}; num_batches_tracked is ignored
 *   BatchNorm eps 1e-5 (torch's default), folded at load
 *   padding   SAME by the size % stride rule in all three dimensions (compute_pad); equal to the Kinetics rule at 224 x 224
 *   head      AvgPool3d((2, 7, 7)), length 32: ((4, 7, 7)); the metric reads its output, the classifier is never run
 * i2v_i3d_load, i2v_i3d_destroy and i2v_i3d_forward (logits; not used by DTFVD) work on either variant.
 * ---------------------------------------------------------------------------------------- */
/* InceptionI3D.__init__ (ID3.py:224-321, ID3_32.py) as DTFVD_Score.load_model(length) builds it; length 16 or 32 */
int i2v_dti3d_create(int32_t num_classes, int32_t length, i2v_i3d** out);
/* Workspace of i2v_i3d_features for t_out frames per clip; 0 if there is no plan (too few frames for the average pool). */
size_t i2v_i3d_features_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t_out, int32_t h, int32_t w);
/* T' of get_representation for t_out input frames (0: too few; at least 9 frames, length 32: 25) */
int32_t i2v_i3d_feature_steps(const i2v_i3d* n, int32_t t_out);
/* InceptionI3D.get_representation behind the input rule of DTFVD_Score.calculate_FVD (:173-176) / embedding_I3D (:205-206):
 * frames [B][t_in][3][h][w] fp32 are resized to 224 x 224 (bilinear, align_corners=True); frame t of the t_out that enter the
 * network is source frame t % t_in (repeat(1, 3, 1, 1, 1)[:, :16]; t_out <= t_in is plain truncation); (x + 1) / 2 only when
 * denorm != 0 (the DTFVD paths pass 0) -> feats [B][1024][T'], the average pool's output after the two squeeze(3).  Either
 * variant of the handle.  Only enqueues on `stream`. */
int i2v_i3d_features(i2v_i3d* n, const float* frames, int32_t batch, int32_t t_in, int32_t t_out, int32_t h, int32_t w, int32_t denorm,
                     float* feats, void* workspace, size_t workspace_bytes, void* stream);
/* The pair loop of metrics/Diversity/I3D.py compute_DTI3D_diversity (:53-57) on embed [n][r][d] fp32 (instance, realization,
 * feature): acc[0] += sum over the n instances and all ordered pairs i != j of mean_d (e_i - e_j)^2, acc[1] += n r (r - 1).
 * float64, one workgroup, fixed order: two runs give the same bits.  acc[0] / acc[1] is the reference's np.mean(div). */
int i2v_diversity_update(const float* embed, int32_t n, int32_t r, int32_t d, double* acc, void* stream);

/* ------------------------------------------------------------------------------------------
 * I3D sub-modules, individually callable on a LOADED i2v_i3d handle (either variant) at a caller-chosen batch, t, h, w -- for
 * tests and inspection.  Tensors are channels-last fp32 on the device, [B][T][H][W][C].  The padding and shape arithmetic is the
 * code the whole-network walk runs: Kinetics rule (size % stride on time only) or dynamic-texture rule (on every dimension) by
 * the handle's variant.  Bad arguments return I2V_E_INVALID, a short output or workspace I2V_E_WORKSPACE, before any launch.
 * ---------------------------------------------------------------------------------------- */
/* Unit index: stem (7x7x7, stride 2; its input carries 4 channels r, g, b, 0), conv3d_2b_1x1, conv3d_2c_3x3, the six units of
 * Mixed block i in {0 = 3b .. 8 = 5c} as I2V_I3D_UNIT_MIXED + 6 i + j (j: branch_0, branch_1.0, branch_1.1, branch_2.0,
 * branch_2.1, branch_3.1), the classifier conv3d_0c_1x1 / logits (bias, no BatchNorm, no ReLU). */
#define I2V_I3D_UNIT_STEM 0
#define I2V_I3D_UNIT_2B 1
#define I2V_I3D_UNIT_2C 2
#define I2V_I3D_UNIT_MIXED 3
#define I2V_I3D_UNIT_HEAD 57
/* cin: input channels the unit reads (a multiple of 4), cout, out_dims[3] = (To, Ho, Wo) on a [t][h][w] map; each may be NULL. */
int i2v_i3d_unit_shape(const i2v_i3d* n, int32_t unit, int32_t t, int32_t h, int32_t w, int32_t* cin, int32_t* cout, int32_t* out_dims);
/* x [B][t][h][w][in_cs] (channels [0, cin) are read) -> channels [out_off, out_off + cout) of out [B][To][Ho][Wo][out_cs]; the
 * other channels of out are left as they are.  out_floats: the capacity of out. */
int i2v_i3d_unit_forward(i2v_i3d* n, int32_t unit, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t in_cs, float* out,
                         int32_t out_cs, int32_t out_off, size_t out_floats, void* stream);
/* Mixed block (0 = mixed_3b .. 8 = mixed_5c): x [B][t][h][w][cin] -> out [B][t][h][w][Co], the six convs, the 3x3x3 / 1 max pool,
 * the branch temporaries and the four slice stores as the network runs them. */
size_t i2v_i3d_mixed_workspace_bytes(const i2v_i3d* n, int32_t block, int32_t batch, int32_t t, int32_t h, int32_t w);
int i2v_i3d_mixed_forward(i2v_i3d* n, int32_t block, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, float* out, void* workspace,
                          size_t workspace_bytes, void* stream);
/* Max pool (kt, k, k) / (st, s, s) with the variant's SAME zero padding, ceil mode: out_dims[3] = (To, Ho, Wo); x [B][t][h][w][c]
 * (c % 4 == 0) -> out [B][To][Ho][Wo][c].  out_floats: the capacity of out. */
int i2v_i3d_maxpool_shape(const i2v_i3d* n, int32_t kt, int32_t k, int32_t st, int32_t s, int32_t t, int32_t h, int32_t w, int32_t* out_dims);
int i2v_i3d_maxpool_forward(i2v_i3d* n, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t c, int32_t kt, int32_t k, int32_t st,
                            int32_t s, float* out, size_t out_floats, void* stream);
/* Head on x [B][t][7][7][1024] with T' = t - pool_t + 1: the average pool in both layouts (pooled [B][T'][1024], feats
 * [B][1024][T'] as i2v_i3d_features returns it), then the classifier and the time mean -> logits [B][num_classes]. */
size_t i2v_i3d_head_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t);
int i2v_i3d_head_forward(i2v_i3d* n, const float* x, int32_t batch, int32_t t, float* pooled, float* feats, float* logits, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * VGG-16 feature trunk (csrc/i2v_vgg.hip; its layer plan: csrc/i2v_vgg_plan.h), LPIPS and the VGG diversity score (the reductions:
 * csrc/i2v_lpips.hip) -- stage2_cINN/AE/modules/vgg16.py (vgg16.forward
 * :30-42: the `features` trunk of torchvision's configuration D cut into five slices), stage2_cINN/AE/modules/LPIPS.py (LPIPS.forward
 * :38-52, ScalingLayer :55-62, NetLinLayer :65-72) and metrics/Diversity/VGG.py (compute_vgg_diversity :9-47).
 * Thirteen 3x3 convolutions (stride 1, pad 1, bias, ReLU) in exact fp32 on the matrix cores and four MaxPool2d(2, 2); activations
 * are channels-last [N][H][W][C], the 3-channel input is stored as 4 channels (r, g, b, 0).  Single stream: every call only
 * enqueues on `stream` (i2v_vgg_conv_unit excepted) and can be captured into a graph.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_vgg i2v_vgg;
#define I2V_VGG_INPUT_LPIPS 0      /* (x - shift) / scale: ScalingLayer, LPIPS.py:55-62; no resize */
#define I2V_VGG_INPUT_DIVERSITY 1  /* ((x + 1) / 2 - mean) / std with the ImageNet constants, then bilinear: metrics/Diversity/VGG.py:20-21, 29, 36 */
/* vgg16.__init__ (vgg16.py:7-28) */
int i2v_vgg_create(i2v_vgg** out);
void i2v_vgg_destroy(i2v_vgg* v);
/* torchvision keys features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight [Cout][Cin][3][3], bias [Cout]} (other keys, the classifier
 * among them, are ignored) and, optionally, all five lin{0..4}.model.1.weight [1][C][1][1] of LPIPS.py:18-22.  Packed once, here. */
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_vgg_load(i2v_vgg* v, const i2v_tensor* tensors, int32_t n_tensors);
/* Device pointer to the loaded lin{layer} weights [C] (NULL: none loaded, or layer outside 0..4). */
const float* i2v_vgg_lin(const i2v_vgg* v, int32_t layer);
/* Workspace of i2v_vgg_features; 0 when h or w is below 16 (a pool would leave an empty map). */
size_t i2v_vgg_workspace_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w);
/* frames [n][3][hi][wi] fp32 in [-1, 1] -> out [n][ho][wo][4] channels-last (channel 3 zero).  Every source pixel is normalised by
 * `mode`, then sampled bilinearly in the arithmetic of torch's upsample_bilinear2d with `align_corners` (the reference's order:
 * resize(normalize(x))).  I2V_VGG_INPUT_LPIPS needs ho = hi and wo = wi; at equal sizes the sample IS the normalised pixel. */
int i2v_vgg_input_stage(const float* frames, int32_t n, int32_t hi, int32_t wi, int32_t mode, int32_t ho, int32_t wo, int32_t align_corners,
                        float* out, void* stream);
/* vgg16.forward (vgg16.py:30-42): x [batch][h][w][4] -> the five taps, caller-owned and channels-last: relu1_2 [batch][h][w][64],
 * relu2_2 [..][h/2][w/2][128], relu3_3 [..][h/4][w/4][256], relu4_3 [..][h/8][w/8][512], relu5_3 [..][h/16][w/16][512] (floor). */
int i2v_vgg_features(i2v_vgg* v, const float* x, int32_t batch, int32_t h, int32_t w, float* relu1_2, float* relu2_2, float* relu3_3, float* relu4_3,
                     float* relu5_3, void* workspace, size_t workspace_bytes, void* stream);
/* One convolution of the trunk's kind from raw weights [cout][cin][3][3] and bias [cout] (HOST pointers): x [n][h][w][cin] -> out
 * [n][h][w][cout] with bias and ReLU.  cin = 3 reads x as [n][h][w][4]; every other cin is a multiple of 16, cout a multiple of 64;
 * anything else is refused.  Packs per call and synchronises the stream: for the unit tests (nn.Conv2d(3, padding=1) + ReLU). */
int i2v_vgg_conv_unit(const float* x, const float* weight, const float* bias, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, float* out,
                      void* stream);
/* nn.MaxPool2d(kernel_size=2, stride=2), floor mode: x [n][h][w][c] -> out [n][h/2][w/2][c]; c a multiple of 4. */
int i2v_vgg_maxpool2(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream);
/* Bytes of the partial-sum workspace that i2v_lpips_layer needs for n images; i2v_vgg_pairdiff_update needs what n = 1 gives. */
size_t i2v_vgg_reduce_workspace_bytes(int32_t n);
/* One layer of LPIPS.forward (LPIPS.py:44-48; normalize_tensor and spatial_average of vgg16.py:45-52): f0, f1 [n][p][c] fp32
 * channels-last taps, lin [c] (device):  out[i] += mean_p sum_c lin_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 for image i,
 * |.| the norm over c, in float64.  Both maps are read once; two fixed-order stages, no atomics.  c in {64, 128, 256, 512}. */
int i2v_lpips_layer(const float* f0, const float* f1, const float* lin, int32_t n, int32_t p, int32_t c, double* out, void* workspace,
                    size_t workspace_bytes, void* stream);
/* The pair loop of metrics/Diversity/VGG.py:38-43 for one layer of one group: maps [r][d] fp32 (r realizations, 2..16):
 * acc[0] += sum_{i != j} mean_d (f_i - f_j)^2, acc[1] += r (r - 1) -- the convention of i2v_diversity_update -- in float64; every
 * element is read once; two fixed-order stages, no atomics. */
int i2v_vgg_pairdiff_update(const float* maps, int32_t r, int64_t d, double* acc, void* workspace, size_t workspace_bytes, void* stream);

/* ---- LPIPS as a loss: the gradient at the input of the frozen trunk (stage1_VAE/modules/loss.py:139, 147 `self.lpips(seq_orig, seq_gen).mean()`
 * in Backward.forward, back-propagated through the second argument; stage2_cINN/AE/modules/loss.py:38 uses the same module).  VGG-16 and the
 * lin layers carry no gradient (vgg16.py:26-28, LPIPS.py:23-24): only input gradients exist.  Every call below only enqueues on
 * `stream` (the *_unit entry excepted), uses no atomics, and gives a batch row the bits of its single-image run. */
/* Bytes of the saved state of i2v_vgg_features_saved: the eight post-ReLU activations that are not taps (the taps themselves are
 * the other five).  0 when h or w is below 16. */
size_t i2v_vgg_saved_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w);
/* Workspace of i2v_vgg_backward: two gradient maps of relu1_2's size.  0 when h or w is below 16. */
size_t i2v_vgg_backward_workspace_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w);
/* Where the thirteen post-ReLU activations of one i2v_vgg_features_saved pass lie: out[13] in layer order, each [batch][h][w][cout]
 * fp32; tap >= 0: it is that tap (the caller's buffer), else it starts at byte `offset` of `saved`.  A host function: no handle, no
 * device call.  I2V_E_INVALID for a shape i2v_vgg_features_saved refuses. */
typedef struct {
    int32_t h, w, cout, tap;
    int64_t offset;
} i2v_vgg_layer;
int i2v_vgg_saved_layout(int32_t batch, int32_t h, int32_t w, i2v_vgg_layer* out);
/* vgg16.forward (vgg16.py:30-42) as i2v_vgg_features, the same kernels and the same tap bits; the intermediate activations go to
 * `saved` instead of a ping-pong workspace (the ReLU masks of the backward pass; the pool arg-max is read from the taps). */
int i2v_vgg_features_saved(i2v_vgg* v, const float* x, int32_t batch, int32_t h, int32_t w, float* relu1_2, float* relu2_2, float* relu3_3,
                           float* relu4_3, float* relu5_3, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream);
/* Backward of one layer of LPIPS.forward (LPIPS.py:44-52 with normalize_tensor, vgg16.py:46-48): upstream[i] (float64, device) is
 * the weight of image i's output.  grad0 / grad1 [n][p][c] fp32 take the gradient at f0 / f1 (null: not wanted; not both).  The two
 * per-position dot products are float64.  At an all-zero feature vector the result is dn / 1e-10 (finite; torch gives NaN). */
int i2v_lpips_layer_backward(const float* f0, const float* f1, const float* lin, const double* upstream, int32_t n, int32_t p, int32_t c,
                             float* grad0, float* grad1, void* stream);
/* Backward of vgg16.forward (vgg16.py:30-42) at the input: taps[5] the tap buffers of i2v_vgg_features_saved, tap_grads[5] their
 * gradients (same shapes, channels-last; both arrays of device pointers live on the HOST), `saved` its saved state (NULL: refused).
 * frames_out = 0: out [batch][h][w][4], the gradient at x (channel 3 zero).  frames_out = 1: out [batch][3][h][w], the gradient at
 * the frames behind ScalingLayer (LPIPS.py:56-63: divided by scale).  The first backward call of a handle packs the backward
 * weights (59 MB) and must not be captured; later calls can be. */
int i2v_vgg_backward(i2v_vgg* v, const float* const* taps, const float* const* tap_grads, const void* saved, size_t saved_bytes, int32_t batch,
                     int32_t h, int32_t w, float* out, int32_t frames_out, void* workspace, size_t workspace_bytes, void* stream);
/* Input gradient of one convolution of the trunk's kind (nn.Conv2d(cin, cout, 3, padding=1): the torchvision layers of vgg16.py:9-25) from raw weights
 * [cout][cin][3][3] (HOST pointer): g [n][h][w][cout] -> out [n][h][w][cin] = (dgrad + add) * (ymask > 0), add and ymask
 * [n][h][w][cin] optional.  cin a multiple of 64, cout a multiple of 16.  cin = 3 (cout = 64) is the first-layer form: out
 * [n][h][w][4], or with frames_out [n][3][h][w] divided by ScalingLayer's scale; no add, no mask.  Packs per call and synchronises. */
int i2v_vgg_dgrad_unit(const float* g, const float* weight, const float* add, const float* ymask, int32_t n, int32_t h, int32_t w, int32_t cin,
                       int32_t cout, float* out, int32_t frames_out, void* stream);
/* Backward of nn.MaxPool2d(2, 2) (features.4 / 9 / 16 / 23 of vgg16.py:9-25): grad [n][h/2][w/2][c], y [n][h][w][c] the pool's input -> out [n][h][w][c].  The
 * gradient goes to the first maximum of a window in row-major order (torch's rule); everything else, the dropped row / column of an
 * odd map included, is zero.  Then + add [n][h][w][c] (optional) and, with relu_mask, * (y > 0). */
int i2v_vgg_maxpool2_backward(const float* grad, const float* y, const float* add, int32_t relu_mask, int32_t n, int32_t h, int32_t w, int32_t c,
                              float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * FID Inception-v3 trunk (csrc/i2v_inception.hip) -- metrics/FID/inception.py (InceptionV3.forward :129-161, fid_inception_v3
 * :164-186, FIDInceptionA / C / E_1 / E_2 :189-306 and the torchvision blocks InceptionB / D and BasicConv2d they sit on) and the
 * feature half of metrics/FID/FID_Score.py (get_activations :98-158; the statistics run on i2v_fvd_stats_update with d = 2048).
 * 94 BasicConv2d units (Conv2d without bias, BatchNorm2d(eps = 0.001) in eval mode, ReLU) in exact fp32 on the matrix cores: square
 * 1x1 / 3x3 / 5x5 and rectangular 1x7 / 7x1 / 1x3 / 3x1 windows, stride 1 or 2; three 3x3 pools and the global average.  Activations
 * are channels-last [N][H][W][C], the 3-channel input is stored as 4 channels (r, g, b, 0); the branches of a Mixed block store into
 * their channel slice.  Single stream: every call only enqueues on `stream` (i2v_inception_conv_unit excepted) and can be captured
 * into a graph.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_inception i2v_inception;
#define I2V_INCEPTION_POOL_MAX_S2 0  /* nn.MaxPool2d(kernel_size=3, stride=2): no padding, floor mode (inception.py:89, 98; InceptionB / D) */
#define I2V_INCEPTION_POOL_MAX_S1 1  /* F.max_pool2d(x, 3, stride=1, padding=1): the padding never wins (FIDInceptionE_2.forward, inception.py:302) */
#define I2V_INCEPTION_POOL_AVG 2     /* F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False) (inception.py:206, 234, 267) */
#define I2V_INCEPTION_BLOCKS 11      /* Mixed_5b, 5c, 5d, 6a, 6b, 6c, 6d, 6e, 7a, 7b, 7c: the `block` index of i2v_inception_mixed_* */
/* fid_inception_v3 (inception.py:164-186): the graph, without weights */
int i2v_inception_create(i2v_inception** out);
void i2v_inception_destroy(i2v_inception* n);
/* torchvision keys <unit>.conv.weight [Cout][Cin][KH][KW] and <unit>.bn.{weight, bias, running_mean, running_var} [Cout] of every
 * BasicConv2d (Conv2d_1a_3x3 ... Mixed_7c.branch_pool); every other key (num_batches_tracked, fc.*, AuxLogits.*) is ignored.  A
 * missing or mis-shaped entry: I2V_E_MISSING with the key in i2v_last_error.  BatchNorm is folded to (scale, shift) here. */
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_inception_load(i2v_inception* n, const i2v_tensor* tensors, int32_t n_tensors);
/* dims = (H', W', C) of output block 0..3 (inception.py:84-124: 64, 192, 768 channels, 2048 at 1 x 1) for an [h][w] trunk input. */
int i2v_inception_block_shape(const i2v_inception* n, int32_t h, int32_t w, int32_t block, int32_t* dims);
/* Workspace of i2v_inception_features when `last_block` is the last block requested; 0 when h or w is below 75. */
size_t i2v_inception_workspace_bytes(const i2v_inception* n, int32_t batch, int32_t h, int32_t w, int32_t last_block);
/* InceptionV3.forward :144-151: frames [n][3][hi][wi] fp32 -> out channels-last [n][299][299][4] when `resize` (F.interpolate, bilinear,
 * align_corners=False, in the arithmetic of torch's upsample_bilinear2d), else [n][hi][wi][4]; then 2 x - 1 when `normalize`. */
int i2v_inception_input_stage(const float* frames, int32_t n, int32_t hi, int32_t wi, int32_t resize, int32_t normalize, float* out, void* stream);
/* InceptionV3.forward :153-161: x [batch][h][w][4] -> the requested blocks, caller-owned and channels-last (i2v_inception_block_shape);
 * block3 is [batch][2048].  A NULL block is skipped and the walk stops behind the last one requested.  h, w >= 75. */
int i2v_inception_features(i2v_inception* n, const float* x, int32_t batch, int32_t h, int32_t w, float* block0, float* block1, float* block2,
                           float* block3, void* workspace, size_t workspace_bytes, void* stream);
/* One BasicConv2d (torchvision inception.py) from raw HOST weights [cout][cin][kh][kw] and BatchNorm vectors [cout]: channels
 * [in_off, in_off + cin) of x [n][h][w][in_cs] -> channels [out_off, out_off + cout) of out [n][h'][w'][out_cs]; the other channels
 * of out are not touched.  cin = 3 reads 4 stored channels; every other cin is a multiple of 16; kernel extents 1..7, stride 1 or 2,
 * padding below the kernel; anything else is refused.  Packs per call and synchronises the stream: for the unit tests. */
int i2v_inception_conv_unit(const float* x, int32_t n, int32_t h, int32_t w, int32_t in_cs, int32_t in_off, const float* weight, const float* bn_weight,
                            const float* bn_bias, const float* bn_mean, const float* bn_var, int32_t cin, int32_t cout, int32_t kh, int32_t kw,
                            int32_t stride, int32_t pad_h, int32_t pad_w, float* out, int32_t out_cs, int32_t out_off, size_t out_floats, void* stream);
/* One 3x3 pool of `kind` (I2V_INCEPTION_POOL_*): x [n][h][w][c] -> channels [out_off, out_off + c) of out [n][h'][w'][out_cs]; c, out_cs
 * and out_off multiples of 4. */
int i2v_inception_pool(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kind, float* out, int32_t out_cs, int32_t out_off,
                       size_t out_floats, void* stream);
/* nn.AdaptiveAvgPool2d((1, 1)) (inception.py:122): x [n][h][w][c] -> out [n][c]. */
int i2v_inception_global_avg(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream);
/* Mixed block `block` (0 = Mixed_5b ... 10 = Mixed_7c) of a loaded handle on an [h][w] map: its channel counts and output map. */
int i2v_inception_mixed_shape(const i2v_inception* n, int32_t block, int32_t h, int32_t w, int32_t* cin, int32_t* cout, int32_t* out_hw);
size_t i2v_inception_mixed_workspace_bytes(const i2v_inception* n, int32_t block, int32_t batch, int32_t h, int32_t w);
/* FIDInceptionA / InceptionB / FIDInceptionC / InceptionD / FIDInceptionE_1 / E_2 .forward: x [batch][h][w][cin] -> out
 * [batch][h'][w'][cout], torch.cat(outputs, 1) as channel slices. */
int i2v_inception_mixed_forward(i2v_inception* n, int32_t block, const float* x, int32_t batch, int32_t h, int32_t w, float* out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Motion encoder of the transfer path (row N3): Encoder.forward -- stage1_VAE/modules/resnet3D.py:138-219
 * (3D ResNet-18, GroupNorm(16), conv_mu / conv_var).  Model.transfer (get_model.py:87) uses mu.
 * Keys: conv1.weight, norm1.*, layer.{L}.{i}.{conv1,conv2}.weight, .bn{1,2}.*, .downsample.{0.weight,1.*},
 * conv_mu.*, conv_var.*.  Frames must be powers of two >= 64 and reduce to a [1,4,4] map (checked before anything is launched).
 * Channels: multiples of 16 in [16, 1024], the stem at most 80.  A layer with stride_t 2, stride_s 1 and equal widths has no
 * downsample branch for its half-rate residual (resnet3D.py:184; the reference fails in `out += residual`): create refuses it.
 * ---------------------------------------------------------------------------------------- */
typedef struct i2v_encoder3d i2v_encoder3d;
typedef struct {
    int32_t z_dim;        /* 64 */
    int32_t channels[5];  /* e.g. [64,128,256,512,512] */
    int32_t stride_s[4];  /* e.g. [1,2,2,2] */
    int32_t stride_t[4];  /* e.g. [1,2,2,2] */
    int32_t use_max_pool; /* must be 0 (every shipped config) */
} i2v_encoder3d_cfg;
int i2v_encoder3d_create(const i2v_encoder3d_cfg* cfg, i2v_encoder3d** out);
void i2v_encoder3d_destroy(i2v_encoder3d* e);
/* (a failed load leaves the handle unloaded: its next forward returns I2V_E_STATE -- see Conventions) */
int i2v_encoder3d_load(i2v_encoder3d* e, const i2v_tensor* tensors, int32_t n_tensors);
size_t i2v_encoder3d_workspace_bytes(const i2v_encoder3d* e, int32_t batch, int32_t t, int32_t h, int32_t w);
/* x [B,3,t,h,w] -> mu [B,z], logvar [B,z]; sample = eps * exp(0.5 logvar) + mu when sample != NULL (eps [B,z]). */
int i2v_encoder3d_forward(i2v_encoder3d* e, const float* x, int32_t t, int32_t h, int32_t w, const float* eps, float* sample,
                          float* mu, float* logvar, void* workspace, size_t workspace_bytes, int32_t batch, void* stream);

/* ------------------------------------------------------------------------------------------
 * Output stage: decoder frames -> interleaved uint8 on the device (csrc/i2v_frames.hip).  Replaces the host-side tail of every
 * caller: denorm (utils/auxiliaries.py:53-55), the GIF tiling permute + divide-by-own-maximum (utils/auxiliaries.py:15-22) and the
 * uint8 cast that follows them, which the reference and the host path of this package run in numpy on a full fp32 copy.
 * No handle: both calls are stateless, only enqueue on `stream`, never synchronise and can be captured into a graph.
 * ---------------------------------------------------------------------------------------- */
#define I2V_FRAMES_PEAK 0   /* GIF semantics: d = min(max(x*0.5f + 0.5f, 0), 1) (multiply and add rounded separately),
                             * s = (float)(255.0 / (double)d(peak)), u8 = trunc(d * s) */
#define I2V_FRAMES_UNIT 1   /* u8 = trunc(min(max(d * 255.0f + 0.5f, 0), 255)): the rounding of torchvision's save_image */
#define I2V_FRAMES_STRIP 0  /* dst [T, rows, cols, 3]: sample s at pixel row row0 + (s % k) * h, pixel column col0 + (s / k) * w */
#define I2V_FRAMES_CLIPS 1  /* dst [N, T, H, W, 3], dense */

typedef struct {
    int32_t n, t, h, w;        /* x: N samples of [T, 3, H, W] fp32 planes (what i2v_dec_forward* writes) */
    int64_t n_stride;          /* floats between two samples of x; 0 = dense (T*3*H*W).  [F, K, ...] blocks are N = F*K samples */
    int32_t k;                 /* STRIP: grid rows (realizations per start frame); must divide n.  1 = one strip */
    int32_t layout;            /* I2V_FRAMES_STRIP / I2V_FRAMES_CLIPS */
    int64_t dst_row_bytes;     /* STRIP: bytes between two pixel rows of dst (>= 3 * (col0 + n/k * w)) */
    int64_t dst_frame_bytes;   /* STRIP: bytes between two frames of dst (>= (row0 + k*h) * dst_row_bytes) */
    int64_t dst_bytes;         /* size of the dst allocation, checked against the geometry before the launch */
    int32_t row0, col0;        /* STRIP: placement of this block inside dst, in pixels (several batches fill ONE job-wide strip) */
} i2v_frames_cfg;

/* Maximum of all raw values of x into *peak (ONE device float): the maximum that utils/auxiliaries.py:20-21 takes over the
 * de-normalised strip is clamp(*peak * 0.5 + 0.5) because the de-normalisation is monotone.  accumulate = 0 starts from -inf,
 * accumulate != 0 keeps max(*peak, max x): a job converted batch by batch is normalised by one peak.  Uses cfg->n, t, h, w, n_stride. */
int i2v_frames_peak(const float* x, const i2v_frames_cfg* cfg, float* peak, int32_t accumulate, void* stream);
/* x -> interleaved bytes (utils/auxiliaries.py:15-22 + 53-55 and the cast of their callers).  mode I2V_FRAMES_PEAK reads the scale
 * from the device float `peak` that i2v_frames_peak wrote (no host round trip between the two launches); I2V_FRAMES_UNIT takes
 * peak = NULL.  Null pointers, non-positive sizes, k not dividing n, a block that does not fit dst: I2V_E_INVALID before any launch. */
int i2v_frames_to_u8(const float* x, const i2v_frames_cfg* cfg, const float* peak, uint8_t* dst, int32_t mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * Stage-1 validation metrics (csrc/i2v_recon.hip) -- stage1_VAE/modules/loss.py: Backward.eval :183-216 and KL :10-12.  PSNR, SSIM,
 * the L1 error and the KL term of a reconstruction, on frames that stay on the device.  The reference takes psnr and ssim from
 * pytorch_lightning.metrics.functional (1.2.7); this row is pinned to the formulas below, not to that library.
 * Both frame tensors are fp32 [b][t][c][h][w]; `pred_bstride` / `target_bstride` are the floats between two batch entries (0 = dense,
 * t*c*h*w), so the view seq[:, 1:] needs no copy.  An image is one [c][h][w] block, N = b*t of them.  Argument order as the reference
 * calls psnr(seq_orig, seq_gen) / ssim(seq_orig, seq_gen): `pred` is the real clip, `target` the generated one.
 * Stateless; every call only enqueues on `stream`, reads no environment, accumulates in float64 in two fixed-order stages with one
 * owner per output element and plain stores (two runs give the same bits).  Bad arguments: I2V_E_INVALID, a short workspace:
 * I2V_E_WORKSPACE, before any launch.
 * ---------------------------------------------------------------------------------------- */
/* Bytes of the workspace of i2v_recon_range and i2v_recon_stats; 0 for a shape they refuse. */
size_t i2v_recon_workspace_bytes(int32_t b, int32_t t, int32_t c, int32_t h, int32_t w);
/* range[4] (device doubles) = min(pred), max(pred), min(target), max(target): the data_range=None rule of psnr / ssim
 * (loss.py:191, :194 pass none). */
int i2v_recon_range(const float* pred, const float* target, int32_t b, int32_t t, int32_t c, int32_t h, int32_t w, int64_t pred_bstride,
                    int64_t target_bstride, double* range, void* workspace, size_t workspace_bytes, void* stream);
/* One pass over both tensors (loss.py:191 psnr, :194 ssim, :199 the L1 error).  R comes from `range` (what i2v_recon_range wrote,
 * fixed_range = 0) or from the host value fixed_range > 0 (range may then be NULL).
 *   per_image [N][3]  sum |p - t|, sum (p - t)^2, sum of the SSIM map over its valid positions, of image n
 *   scalars [5]       mean |p - t|; MSE; PSNR = (2 ln R - ln MSE) * 10 / ln 10 with R = max(target) - min(target) (only the generated
 *                     frames set it: the 1.2.x rule, kept) or fixed_range; SSIM; the number of SSIM terms N c (h - 10) (w - 10).
 *                     They come from the per_image rows summed in index order.  Identical inputs: PSNR = +inf.
 * SSIM: R = max(max p - min p, max t - min t) or fixed_range, c1 = (0.01 R)^2, c2 = (0.03 R)^2; window = outer product of g / sum g,
 * g_i = exp(-(d_i / 1.5)^2 / 2), d = -5..5, applied per channel to p, t, p^2, t^2, p t (separably, in float64); with mu and
 * sigma.. = E[..] - mu mu from those five, ssim = (2 mu_p mu_t + c1)(2 sigma_pt + c2) / ((mu_p^2 + mu_t^2 + c1)(sigma_p^2 + sigma_t^2 + c2)),
 * averaged over the (h - 10) x (w - 10) positions whose window lies inside the image (what the reflect-pad-and-crop of the library
 * leaves).  h < 11 or w < 11 is refused.  Constant frames (R = 0) give 0 / 0 = NaN as in the reference; nothing synchronises to refuse it. */
int i2v_recon_stats(const float* pred, const float* target, int32_t b, int32_t t, int32_t c, int32_t h, int32_t w, int64_t pred_bstride,
                    int64_t target_bstride, const double* range, double fixed_range, double* per_image, double* scalars,
                    void* workspace, size_t workspace_bytes, void* stream);
/* KL (loss.py:10-12): out[0] (device double) = -0.5 * mean_b sum_d (1 + logvar - mu^2 - exp(logvar)); mu, logvar [b][d] fp32.
 * One workgroup, float64, fixed order. */
int i2v_kl_normal(const float* mu, const float* logvar, int32_t b, int32_t d, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* I2V_HIP_H */
