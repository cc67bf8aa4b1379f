// Motion encoder of the transfer path (row N3): Encoder.forward (reference stage1_VAE/modules/resnet3D.py:138-219).
//
// 3D ResNet-18: Conv3d(3, c0, (3,7,7), stride 2, pad (1,3,3)) -> GroupNorm(16) -> ReLU -> 4 layers of 2 BasicBlocks
// (3x3x3 convs, strides (stride_t, stride_s, stride_s) on the first conv and on the 3x3x3 down-sample conv of each layer,
// GroupNorm(16, affine) everywhere) -> squeeze(T = 1) -> conv_mu / conv_var = Conv2d(c4, z, 4) on the 4x4 map.
// Model.transfer (get_model.py:87) keeps the MEAN mu; logvar is returned as well.
//
// This file is the handle: create, the loader (one loop over the topology table of i2v_resnet_plan.h) and the entries.  What a
// forward launches is enc3d_plan's list of steps; the kernels and the loop that runs them are in i2v_resnet.hip.
#include "i2v_handle.h"
#include "i2v_resnet.h"

using namespace i2v;

struct i2v_encoder3d {
    i2v_encoder3d_cfg cfg;
    int device = 0;
    bool loaded = false;
    DevBuf stem_w;
    std::vector<ResConv> convs;   // ENC_NCONV: per block conv1, conv2, downsample; conv_mu | conv_var as one Linear(16*c4 -> 2z)
    std::vector<ResNorm> norms;   // ENC_NNORM: the stem's, per block bn1, bn2, downsample.1
};

namespace {

int load_gn(const StateDict& sd, const std::string& name, int C, ResNorm& g) {
    const float* w = sd.f32(name + ".weight", C);
    const float* b = sd.f32(name + ".bias", C);
    if (!w || !b) return I2V_E_MISSING;
    int rc = g.w.upload(w, (size_t)C * 4);
    if (rc) return rc;
    return g.b.upload(b, (size_t)C * 4);
}

}  // namespace

extern "C" {

int i2v_encoder3d_create(const i2v_encoder3d_cfg* cfg, i2v_encoder3d** out) {
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "i2v_encoder3d_create: null argument");
    for (int i = 0; i < 5; ++i)
        I2V_REQUIRE(cfg->channels[i] >= 16 && cfg->channels[i] % 16 == 0 && cfg->channels[i] <= 1024, I2V_E_INVALID,
                    "i2v_encoder3d_create: channels must be multiples of 16 in [16, 1024]");
    for (int i = 0; i < 4; ++i)
        I2V_REQUIRE((cfg->stride_s[i] == 1 || cfg->stride_s[i] == 2) && (cfg->stride_t[i] == 1 || cfg->stride_t[i] == 2), I2V_E_INVALID,
                    "i2v_encoder3d_create: strides must be 1 or 2");
    I2V_REQUIRE(cfg->z_dim > 0 && !cfg->use_max_pool, I2V_E_INVALID,
                "i2v_encoder3d_create: z_dim > 0 required; use_max_pool is false in every shipped config and is not supported");
    I2V_REQUIRE(147 * 3 * cfg->channels[0] * 4 <= 150 * 1024, I2V_E_INVALID, "i2v_encoder3d_create: stem too wide for LDS");
    const int bad = enc3d_halfrate_without_down(*cfg);   // (the message's arguments are read only where it is refused)
    I2V_REQUIRE(bad < 0, I2V_E_INVALID,
                "i2v_encoder3d_create: layer %d has stride_t 2 with stride_s 1 and equal widths (%d): no downsample branch exists "
                "for its half-rate residual", bad, cfg->channels[bad]);
    return create_handle("i2v_encoder3d_create", out, [&](i2v_encoder3d* e) {
        e->cfg = *cfg;
        const char* zp = nullptr;
        return zero_page(&zp);  // allocated here, not inside a forward
    });
}

void i2v_encoder3d_destroy(i2v_encoder3d* e) { delete e; }

static int encoder3d_pack(i2v_encoder3d* e, const StateDict& sd) {
    const int c0 = e->cfg.channels[0];
    int rc;
    e->convs = std::vector<ResConv>(ENC_NCONV);
    e->norms = std::vector<ResNorm>(ENC_NNORM);
    {   // conv1.weight [c0][3][3][7][7] -> [tap][cin][c0]
        const float* w = sd.f32("conv1.weight", (int64_t)c0 * 3 * 147);
        if (!w) return I2V_E_MISSING;
        std::vector<float> p((size_t)147 * 3 * c0);
        for (int n = 0; n < c0; ++n)
            for (int c = 0; c < 3; ++c)
                for (int tap = 0; tap < 147; ++tap) p[((size_t)tap * 3 + c) * c0 + n] = w[((size_t)n * 3 + c) * 147 + tap];
        if ((rc = e->stem_w.upload(p.data(), p.size() * 4))) return rc;
        if ((rc = load_gn(sd, "norm1", c0, e->norms[0]))) return rc;
    }
    ResBlockSpec blocks[ENC_BLOCKS];
    enc3d_blocks(e->cfg, blocks);
    for (int k = 0; k < ENC_BLOCKS; ++k) {
        const ResBlockSpec& b = blocks[k];
        const std::string p = enc3d_prefix(b);
        const float* w1 = sd.f32(p + "conv1.weight", (int64_t)b.cout * b.cin * 27);
        const float* w2 = sd.f32(p + "conv2.weight", (int64_t)b.cout * b.cout * 27);
        if (!w1 || !w2) return I2V_E_MISSING;
        if ((rc = e->convs[enc_conv(k, 0)].pack(w1, b.cout, b.cin, 3, 3, 3, b.ss, b.st))) return rc;
        if ((rc = e->convs[enc_conv(k, 1)].pack(w2, b.cout, b.cout, 3, 3, 3, 1, 1))) return rc;
        if ((rc = load_gn(sd, p + "bn1", b.cout, e->norms[enc_norm(k, 0)]))) return rc;
        if ((rc = load_gn(sd, p + "bn2", b.cout, e->norms[enc_norm(k, 1)]))) return rc;
        if (!b.has_down) continue;
        const float* wd = sd.f32(p + "downsample.0.weight", (int64_t)b.cout * b.cin * 27);
        if (!wd) return I2V_E_MISSING;
        if ((rc = e->convs[enc_conv(k, 2)].pack(wd, b.cout, b.cin, 3, 3, 3, b.ss, b.st))) return rc;
        if ((rc = load_gn(sd, p + "downsample.1", b.cout, e->norms[enc_norm(k, 2)]))) return rc;
    }
    // conv_mu / conv_var: Conv2d(c4, z, 4, 1, 0) on [B, c4, 4, 4] == Linear over (h, w, c) of the channels-last map
    const int c4 = e->cfg.channels[4], z = e->cfg.z_dim;
    const float* wm = sd.f32("conv_mu.weight", (int64_t)z * c4 * 16);
    const float* bm = sd.f32("conv_mu.bias", z);
    const float* wv = sd.f32("conv_var.weight", (int64_t)z * c4 * 16);
    const float* bv = sd.f32("conv_var.bias", z);
    if (!wm || !bm || !wv || !bv) return I2V_E_MISSING;
    std::vector<float> w((size_t)2 * z * 16 * c4), bias((size_t)2 * z);
    for (int part = 0; part < 2; ++part)
        for (int n = 0; n < z; ++n) {
            const float* src = (part ? wv : wm) + (size_t)n * c4 * 16;
            for (int c = 0; c < c4; ++c)
                for (int hw = 0; hw < 16; ++hw) w[((size_t)(part * z + n) * 16 + hw) * c4 + c] = src[(size_t)c * 16 + hw];
            bias[part * z + n] = (part ? bv : bm)[n];
        }
    return e->convs[ENC_HEAD].pack(w.data(), 2 * z, 16 * c4, 1, 1, 1, 1, 1, bias.data());
}

int i2v_encoder3d_load(i2v_encoder3d* e, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_encoder3d_load", e, tensors, n_tensors, encoder3d_pack);
}

size_t i2v_encoder3d_workspace_bytes(const i2v_encoder3d* e, int32_t batch, int32_t t, int32_t h, int32_t w) {
    if (!e || batch <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    return enc3d_plan<Carver>(e->cfg, batch, t, h, w).total;
}

int i2v_encoder3d_forward(i2v_encoder3d* e, const float* x, int32_t t, int32_t h, int32_t w, const float* eps, float* sample,
                          float* mu, float* logvar, void* workspace, size_t workspace_bytes, int32_t batch, void* stream) {
    I2V_ENTER(sc, e, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_encoder3d_forward");
    I2V_REQUIRE(x && mu && logvar && workspace && batch > 0 && t >= 1, I2V_E_INVALID, "i2v_encoder3d_forward: bad argument");
    I2V_REQUIRE(!sample || eps, I2V_E_INVALID, "i2v_encoder3d_forward: a sample needs eps");
    const ResnetPlan plan = enc3d_plan<Carver>(e->cfg, batch, t, h, w, sample != nullptr);
    if (plan.status) return plan_refusal(plan);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, plan.total, "i2v_encoder3d_forward");
    ResBufs bufs(plan, workspace);
    bufs.caller(RB_IN, x).caller(RB_EPS, eps).caller(RB_SAMPLE, sample).caller(RB_MU, mu).caller(RB_LOGVAR, logvar);
    bufs.stem_w = e->stem_w.as<float>();
    return launch(plan, e->convs, e->norms, bufs, static_cast<hipStream_t>(stream));
}

}  // extern "C"
