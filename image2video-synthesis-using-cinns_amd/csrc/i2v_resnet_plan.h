// The two residual networks in front of the cINN as data: the motion encoder (i2v_encoder.hip, 3D ResNet-18, row N3) and the
// conditioning embedder (i2v_embed.hip, ResNet-50, row N1).  A plan is the ordered list of the steps of one forward -- one Step per
// conv, norm (+ residual, + ReLU), pool, copy or head, with its unit, its form, its maps, its strides and the workspace slots it reads
// and writes -- and the floats every slot takes.  enc3d_plan / embedder_plan make every decision of a forward once: the refusals, the
// kernel form of each conv and the packed set it reads, the effective temporal stride, the rotation of the buffers.  The workspace
// queries read a plan; the forwards hand it to launch() (i2v_resnet.h), one loop over the steps.
// The topology tables at the top are what the loaders and the plans both read.
// Plain C++, no HIP include: the carver comes in as a template argument (i2v_handle.h: Carver), and tests/resnet_plan_host_check.cpp
// prints every plan field for tests/test_host_resnet_plan.py, which also checks that no step reads a slot before it is written or
// after it was overwritten.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/i2v_hip.h"

namespace i2v {

// ---------------------------------------------------------------------------------------------------------------- topology

// One residual block.  BasicBlock (encoder): conv1 3x3x3 (ss, st) -> conv2 3x3x3; Bottleneck (embedder): conv1 1x1 -> conv2 3x3 (ss)
// -> conv3 1x1.  The downsample branch is a conv of the block's stride (3x3x3 in the encoder, 1x1 in the embedder) and a norm.
struct ResBlockSpec {
    int layer, index;      // state_dict position
    int cin, width, cout;  // block input, inner width, block output (BasicBlock: width == cout)
    int ss, st;            // spatial / temporal stride of the block
    bool has_down;
};
// Units: indices into a handle's conv table and norm table.  Block k of the encoder owns convs 3k .. 3k+2 (conv1, conv2,
// downsample) and norms 1+3k .. 3+3k (bn1, bn2, downsample.1); block k of the embedder convs 1+4k .. 4+4k (conv1, conv2, conv3,
// downsample) and norms 1+4k .. 4+4k.  Norm 0 is the stem's.
constexpr int ENC_BLOCKS = 8, ENC_HEAD = 24, ENC_NCONV = 25, ENC_NNORM = 25;
constexpr int EMB_BLOCKS = 16, EMB_STEM = 0, EMB_FC = 65, EMB_NCONV = 66, EMB_NNORM = 65;
inline int enc_conv(int k, int j) { return 3 * k + j; }
inline int enc_norm(int k, int j) { return 1 + 3 * k + j; }
inline int emb_conv(int k, int j) { return 1 + 4 * k + j; }
inline int emb_norm(int k, int j) { return 1 + 4 * k + j; }

// resnet18: BasicBlock x [2,2,2,2]; strides on the first block of a layer; a downsample branch where the reference builds one
// (resnet3D.py:180: stride_s != 1 or a change of width)
inline void enc3d_blocks(const i2v_encoder3d_cfg& cfg, ResBlockSpec out[ENC_BLOCKS]) {
    int inplanes = cfg.channels[0];
    for (int L = 0; L < 4; ++L)
        for (int i = 0; i < 2; ++i) {
            const int planes = cfg.channels[L + 1];
            out[2 * L + i] = ResBlockSpec{L, i, inplanes, planes, planes, i == 0 ? cfg.stride_s[L] : 1, i == 0 ? cfg.stride_t[L] : 1,
                                          i == 0 && (cfg.stride_s[L] != 1 || inplanes != planes)};
            inplanes = planes;
        }
}
// A layer that halves the time extent needs a downsample branch for its residual, and resnet3D.py:180 builds one only for a spatial
// stride or a change of width: without it the reference's `out += residual` fails on the time extent.  The first such layer, or -1.
inline int enc3d_halfrate_without_down(const i2v_encoder3d_cfg& cfg) {
    for (int i = 0; i < 4; ++i)
        if (cfg.stride_s[i] == 1 && cfg.stride_t[i] == 2 && cfg.channels[i] == cfg.channels[i + 1]) return i;
    return -1;
}
inline std::string enc3d_prefix(const ResBlockSpec& b) { return "layer." + std::to_string(b.layer) + "." + std::to_string(b.index) + "."; }

// torchvision resnet50 (0.8.1 layout): Bottleneck [3,4,6,3] x widths [64,128,256,512], the stride on the 3x3 conv of the first block
// of layers 2-4, a downsample branch on every first block
inline void embedder_blocks(ResBlockSpec out[EMB_BLOCKS]) {
    const int nblk[4] = {3, 4, 6, 3}, width[4] = {64, 128, 256, 512};
    int inplanes = 64, k = 0;
    for (int L = 0; L < 4; ++L)
        for (int i = 0; i < nblk[L]; ++i) {
            out[k++] = ResBlockSpec{L, i, inplanes, width[L], 4 * width[L], (i == 0 && L > 0) ? 2 : 1, 1, i == 0};
            inplanes = 4 * width[L];
        }
}
inline std::string embedder_prefix(const ResBlockSpec& b) { return "model.layer" + std::to_string(b.layer + 1) + "." + std::to_string(b.index) + "."; }

// ---------------------------------------------------------------------------------------------------------------- forms

// The kernel a conv runs on, fixed at load by its window and strides:
//   RC_F16  stride-1 3x3(x3) conv on the split-fp16 matrix-core kernel (conv16_forward)
//   RC_S2D  3x3x3 conv with spatial stride 2 as a stride-1 2-tap conv16_forward on the space-to-depth copy of its input; packed set 0
//           for its temporal stride, set 1 (temporal stride 2 only) for a single-frame input, where that stride is the identity
//   RC_F32  everything else on the exact-fp32 kernel (conv_forward): 1x1 and 7x7 convs, the embedder's strided 3x3 convs, a 3x3x3 conv
//           with a temporal stride only (run with stride 1 on a single frame)
enum ResForm { RC_F16 = 0, RC_S2D = 1, RC_F32 = 2 };
inline int res_conv_form(int kt, int kh, int ss, int st) {
    if (kh == 3 && ss == 1 && st == 1) return RC_F16;
    if (kt == 3 && ss == 2) return RC_S2D;
    return RC_F32;
}

// ---------------------------------------------------------------------------------------------------------------- steps

struct ResMap { int T, H, W; long pos() const { return (long)T * H * W; } };   // embedder: T = 1

enum ResKind { RS_STEM, RS_RESIZE, RS_S2D, RS_CONV, RS_NORM, RS_MAXPOOL, RS_MEAN, RS_HEAD, RS_REPARAM };
enum ResNormMode { RN_GROUP16, RN_INSTANCE, RN_BATCH };   // GroupNorm(16, affine); InstanceNorm2d; BatchNorm2d folded to constants

// Slots.  RB_IN .. RB_LOGVAR are the caller's tensors (RB_OUT: the embedding); RB_IMG .. RB_POOLED the workspace, in the order it
// is carved.  The split-fp16 operand format takes the bytes of fp32 per element, so the embedder (which has no RB_H slot) places
// such a tensor in an RB_F slot: a step names it in `dst16`, the format is the step's, not the slot's.
enum ResBuf { RB_NONE = -1, RB_IN, RB_OUT, RB_EPS, RB_SAMPLE, RB_MU, RB_LOGVAR,
              RB_IMG, RB_F0, RB_F1, RB_F2, RB_F3, RB_F4, RB_H0, RB_H1, RB_H2, RB_SUMS, RB_COEF, RB_ML, RB_POOLED, RES_NBUF };
constexpr int RES_SLOT_FIRST = RB_IMG, RES_SLOT_LAST = RB_POOLED;

struct ResStep {
    int kind = RS_CONV;
    int unit = -1;                  // conv / head: the conv table; norm: the norm table
    int form = -1, set = 0;         // conv / head: ResForm and the packed set it reads
    int src = RB_NONE, res = RB_NONE, dst = RB_NONE, dst16 = RB_NONE;   // dst: fp32 output; dst16: split-fp16 output
    ResMap in{1, 1, 1}, out{1, 1, 1};
    int cin = 0, C = 0;             // channels of the tensor read (its channel stride) and channels written
    int ss = 1, st = 1;             // spatial stride and EFFECTIVE temporal stride (1 on a single frame)
    bool relu = false;
};

struct ResnetPlan {
    int B = 0, norm = RN_GROUP16;
    std::vector<ResStep> steps;
    size_t floats[RES_NBUF] = {}, off[RES_NBUF] = {}, total = 0;   // per workspace slot; byte offsets and their total
    int status = I2V_OK;
    char error[256] = "";

    ResnetPlan(int batch, int norm_mode, size_t max_steps) : B(batch), norm(norm_mode) { steps.reserve(max_steps); }   // one allocation per plan

    __attribute__((format(printf, 3, 4))) ResnetPlan& fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(error, sizeof error, fmt, ap);
        va_end(ap);
        status = code;
        return *this;
    }
    template <class Carver>
    void carve() {
        Carver c;
        for (int i = RES_SLOT_FIRST; i <= RES_SLOT_LAST; ++i) off[i] = c.take_floats(floats[i]);
        total = c.total();
    }
    void conv(int kind, int unit, int form, int set, int src, int dst, ResMap in, ResMap out, int cin, int C, int ss, int st) {
        ResStep s;
        s.kind = kind; s.unit = unit; s.form = form; s.set = set; s.src = src; s.dst = dst; s.in = in; s.out = out;
        s.cin = cin; s.C = C; s.ss = ss; s.st = st;
        steps.push_back(s);
    }
    // dst / dst16 = act(norm(src) (+ res)) on the map m
    void norm_act(int unit, int src, int res, int dst, int dst16, ResMap m, int C, bool relu) {
        ResStep s;
        s.kind = RS_NORM; s.unit = unit; s.src = src; s.res = res; s.dst = dst; s.dst16 = dst16; s.in = s.out = m;
        s.cin = s.C = C; s.relu = relu;
        steps.push_back(s);
    }
    void other(int kind, int src, int res, int dst, int dst16, ResMap in, ResMap out, int cin, int C, int ss, int st) {
        ResStep s;
        s.kind = kind; s.src = src; s.res = res; s.dst = dst; s.dst16 = dst16; s.in = in; s.out = out; s.cin = cin; s.C = C;
        s.ss = ss; s.st = st;
        steps.push_back(s);
    }
};

inline bool pow2_ge64(int v) { return v >= 64 && (v & (v - 1)) == 0; }

// ---------------------------------------------------------------------------------------------------------------- motion encoder

// x [B][3][t][h][w] -> mu, logvar (and a sample where the caller brings eps).  Four fp32 slots and three split-fp16 slots, each the
// size of the largest activation: F1 / F0 / F3 rotate as block input x, residual y and downsample temporary t2, F2 is the conv
// temporary t1; H0 / H1 rotate as the split copy of the block input x16 and of the block output y16, H2 holds conv2's operand.
// A strided block builds the space-to-depth copy of its input in y16, which is free until the block's last norm writes there.
// The frame count behind the stem is a power of two, so every layer that halves it meets an even count or a single frame: no
// "odd temporal extent" can occur behind the two refusals below.
template <class Carver>
ResnetPlan enc3d_plan(const i2v_encoder3d_cfg& cfg, int B, int t, int h, int w, bool sample = true) {
    ResnetPlan p(B, RN_GROUP16, 60);
    ResBlockSpec blocks[ENC_BLOCKS];
    enc3d_blocks(cfg, blocks);
    ResMap m{(t + 2 - 3) / 2 + 1, h / 2, w / 2};   // stem: kernel (3,7,7), stride 2, pad (1,3,3)
    {   // the sizes depend on the arguments only: a size query answers for a shape the forward refuses too
        ResMap d = m;
        size_t mx = (size_t)d.pos() * cfg.channels[0];
        for (int l = 0; l < 4; ++l) {
            d = ResMap{(d.T + cfg.stride_t[l] - 1) / cfg.stride_t[l], d.H / cfg.stride_s[l], d.W / cfg.stride_s[l]};
            mx = std::max(mx, (size_t)d.pos() * cfg.channels[l + 1]);
        }
        for (int i = RB_F0; i <= RB_F3; ++i) p.floats[i] = (size_t)B * mx;
        for (int i = RB_H0; i <= RB_H2; ++i) p.floats[i] = (size_t)B * mx;
        p.floats[RB_SUMS] = (size_t)B * 1024 * 4;
        p.floats[RB_COEF] = (size_t)B * 1024 * 2;
        p.floats[RB_ML] = (size_t)B * 2 * cfg.z_dim;
        p.template carve<Carver>();
        if (!pow2_ge64(h) || !pow2_ge64(w))
            return p.fail(I2V_E_INVALID, "i2v_encoder3d_forward: frame size %dx%d must be a power of two >= 64", h, w);
        if ((m.T & (m.T - 1)) != 0)
            return p.fail(I2V_E_INVALID, "i2v_encoder3d_forward: %d input frames give %d stem frames (need a power of two)", t, m.T);
        if (!(d.T == 1 && d.H == 4 && d.W == 4))
            return p.fail(I2V_E_INVALID, "i2v_encoder3d_forward: the feature map is [%d,%d,%d], conv_mu/conv_var need [1,4,4]", d.T, d.H, d.W);
    }
    int C = cfg.channels[0];
    p.other(RS_STEM, RB_IN, RB_NONE, RB_F0, RB_NONE, ResMap{t, h, w}, m, 3, C, 2, 2);
    p.norm_act(0, RB_F0, RB_NONE, RB_F1, RB_H0, m, C, true);
    int x = RB_F1, y = RB_F0, t2 = RB_F3, x16 = RB_H0, y16 = RB_H1;
    const int t1 = RB_F2, t16 = RB_H2;
    for (int k = 0; k < ENC_BLOCKS; ++k) {
        const ResBlockSpec& b = blocks[k];
        const int form = res_conv_form(3, 3, b.ss, b.st);
        const int st = m.T == 1 ? 1 : b.st;   // a temporal stride of 2 is the identity on a single frame (pad 1, kernel 3)
        const int set = form == RC_S2D && st != b.st ? 1 : 0;
        const ResMap o{m.T / st, m.H / b.ss, m.W / b.ss};
        if (form == RC_S2D) p.other(RS_S2D, x, RB_NONE, RB_NONE, y16, m, o, C, st * 4 * C, 2, st);
        const int src = form == RC_F16 ? x16 : form == RC_S2D ? y16 : x;
        // out = relu(bn1(conv1(x)))   (only conv2 reads it: split-fp16 copy only)
        p.conv(RS_CONV, enc_conv(k, 0), form, set, src, t1, m, o, C, b.cout, b.ss, st);
        p.norm_act(enc_norm(k, 0), t1, RB_NONE, RB_NONE, t16, o, b.cout, true);
        // out = relu(bn2(conv2(out)) + residual)
        p.conv(RS_CONV, enc_conv(k, 1), RC_F16, 0, t16, t1, o, o, b.cout, b.cout, 1, 1);
        if (b.has_down) {   // 3x3x3 strided conv + GroupNorm (resnet3D.py:181-189): the residual goes to y, the block output to t2
            p.conv(RS_CONV, enc_conv(k, 2), form, set, src, t2, m, o, C, b.cout, b.ss, st);
            p.norm_act(enc_norm(k, 2), t2, RB_NONE, y, RB_NONE, o, b.cout, false);
            p.norm_act(enc_norm(k, 1), t1, y, t2, y16, o, b.cout, true);
            std::swap(x, t2);
        } else {
            p.norm_act(enc_norm(k, 1), t1, x, y, y16, o, b.cout, true);
            std::swap(x, y);
        }
        std::swap(x16, y16);
        m = o; C = b.cout;
    }
    // conv_mu | conv_var: Conv2d(c4, z, 4) on the 4x4 map == one Linear over (h, w, c) of the channels-last map
    p.conv(RS_HEAD, ENC_HEAD, RC_F32, 0, x, RB_ML, ResMap{1, 1, 1}, ResMap{1, 1, 1}, 16 * C, 2 * cfg.z_dim, 1, 1);
    p.other(RS_REPARAM, RB_ML, sample ? RB_EPS : RB_NONE, sample ? RB_SAMPLE : RB_NONE, RB_NONE, ResMap{1, 1, 1}, ResMap{1, 1, 1},
            2 * cfg.z_dim, cfg.z_dim, 1, 1);
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- embedder

// img [B][3][h][w] -> the embedding [B][E] (E: the handle's, only a step's record of the channels fc writes).  Five fp32 slots of the largest activation (B h w 16 floats = B (h/2) (w/2) 64 =
// B (h/4) (w/4) 256): F0 / F1 rotate as block input x and block output y, F2 / F3 are the conv temporaries t1 / t2, F4 holds the
// downsample branch.  Where conv2 runs on the split-fp16 kernel, norm1 writes its operand to t2 as dst16.
template <class Carver>
ResnetPlan embedder_plan(int bn, int B, int h, int w, int E = 0) {
    ResnetPlan p(B, bn ? RN_BATCH : RN_INSTANCE, 112);
    ResBlockSpec blocks[EMB_BLOCKS];
    embedder_blocks(blocks);
    const size_t big = (size_t)B * h * w * 16;
    p.floats[RB_IMG] = big;
    for (int i = RB_F0; i <= RB_F4; ++i) p.floats[i] = big;
    p.floats[RB_SUMS] = (size_t)B * 2048 * 4;
    p.floats[RB_COEF] = (size_t)B * 2048 * 2;
    p.floats[RB_POOLED] = (size_t)B * 2048;
    p.template carve<Carver>();
    if (!pow2_ge64(h) || !pow2_ge64(w))
        return p.fail(I2V_E_INVALID, "i2v_embedder_forward: image size %dx%d must be a power of two >= 64", h, w);
    // stem: NCHW -> channels-last with 3 -> 16 zero-padded channels, conv1 7x7 s2 -> norm -> ReLU -> MaxPool 3x3 s2
    ResMap m{1, h / 2, w / 2};
    p.other(RS_RESIZE, RB_IN, RB_NONE, RB_IMG, RB_NONE, ResMap{1, h, w}, ResMap{1, h, w}, 3, 16, 1, 1);
    p.conv(RS_CONV, EMB_STEM, RC_F32, 0, RB_IMG, RB_F0, ResMap{1, h, w}, m, 16, 64, 2, 1);
    p.norm_act(0, RB_F0, RB_NONE, RB_F1, RB_NONE, m, 64, true);
    p.other(RS_MAXPOOL, RB_F1, RB_NONE, RB_F0, RB_NONE, m, ResMap{1, m.H / 2, m.W / 2}, 64, 64, 2, 1);
    m = ResMap{1, m.H / 2, m.W / 2};
    int x = RB_F0, y = RB_F1, C = 64;
    const int t1 = RB_F2, t2 = RB_F3, idn = RB_F4;
    for (int k = 0; k < EMB_BLOCKS; ++k) {
        const ResBlockSpec& b = blocks[k];
        const int form = res_conv_form(1, 3, b.ss, 1);
        const ResMap o{1, m.H / b.ss, m.W / b.ss};
        p.conv(RS_CONV, emb_conv(k, 0), RC_F32, 0, x, t1, m, m, C, b.width, 1, 1);
        p.norm_act(emb_norm(k, 0), t1, RB_NONE, form == RC_F16 ? RB_NONE : t2, form == RC_F16 ? t2 : RB_NONE, m, b.width, true);
        p.conv(RS_CONV, emb_conv(k, 1), form, 0, t2, t1, m, o, b.width, b.width, b.ss, 1);   // the stride is on THIS conv (torchvision >= 0.3)
        p.norm_act(emb_norm(k, 1), t1, RB_NONE, t2, RB_NONE, o, b.width, true);
        p.conv(RS_CONV, emb_conv(k, 2), RC_F32, 0, t2, t1, o, o, b.width, b.cout, 1, 1);
        int identity = x;
        if (b.has_down) {   // downsample = Conv2d 1x1 stride s (bias-free) -> norm
            p.conv(RS_CONV, emb_conv(k, 3), RC_F32, 0, x, t2, m, o, C, b.cout, b.ss, 1);
            p.norm_act(emb_norm(k, 3), t2, RB_NONE, idn, RB_NONE, o, b.cout, false);
            identity = idn;
        }
        p.norm_act(emb_norm(k, 2), t1, identity, y, RB_NONE, o, b.cout, true);   // out = ReLU(norm(conv3) + identity)
        std::swap(x, y);
        m = o; C = b.cout;
    }
    // AdaptiveAvgPool2d((1,1)) from the fused statistics, then fc (the first E output channels = the mean of the posterior)
    p.other(RS_MEAN, x, RB_NONE, RB_POOLED, RB_NONE, m, ResMap{1, 1, 1}, C, C, 1, 1);
    p.conv(RS_HEAD, EMB_FC, RC_F32, 0, RB_POOLED, RB_OUT, ResMap{1, 1, 1}, ResMap{1, 1, 1}, C, E, 1, 1);
    return p;
}

}  // namespace i2v
