// Conditioning embedder: ResnetEncoder.encode(x).mode()  (reference: stage2_cINN/AE/modules/AE.py:91-166,
// distributions.py:6-42; row N1 of the coverage contract -- the step immediately in front of the cINN).
//
// torchvision.models.resnet50 (0.8.1 layout: Bottleneck [3,4,6,3], stride on the 3x3 conv, all convs bias-free) with
// norm_layer = InstanceNorm2d (affine-less, per-sample statistics) or BatchNorm2d (eval: running statistics), AdaptiveAvgPool,
// and `fc` replaced by Conv2d(2048, 2E, 1); .mode() of the diagonal Gaussian = the first E channels (the mean).
// The [-1,1] start frame goes in as is (the ImageNet transform at AE.py:111-114 is never applied).
//
// ~0.34 GFLOP per 64x64 sample: < 0.1 % of the path.  This file is the handle: create, the loader (one loop over the topology
// table of i2v_resnet_plan.h) and the entries.  What a forward launches is embedder_plan's list of steps; the kernels and the loop
// that runs them are in i2v_resnet.hip.
#include <cmath>

#include "i2v_handle.h"
#include "i2v_resnet.h"

using namespace i2v;

struct i2v_embedder {
    int E = 0, bn = 0;
    int device = 0;
    bool loaded = false;
    std::vector<ResConv> convs;   // EMB_NCONV: the 7x7 stem, per block conv1, conv2, conv3, downsample; fc
    std::vector<ResNorm> norms;   // EMB_NNORM: BatchNorm constants folded to (A,B) per channel; empty for InstanceNorm
    // One handle = (normally) one workspace: forwards on a handle are serialised.  A call that arrives on another stream than the
    // previous one (LatentPrefetcher's side stream next to the main stream) first waits for the previous forward (event recorded
    // behind every forward), like i2v_flow: a direct call on the main stream cannot race a ticket outstanding on the side stream.
    StreamOrder order;   // (capture-aware: see i2v_common.h)
};

namespace {

// BatchNorm2d in eval mode folded to (A,B) pairs; InstanceNorm has nothing to load
int load_norm(const i2v_embedder* e, const StateDict& sd, const std::string& name, int C, ResNorm& out) {
    if (!e->bn) return I2V_OK;
    const float* w = sd.f32(name + ".weight", C);
    const float* b = sd.f32(name + ".bias", C);
    const float* m = sd.f32(name + ".running_mean", C);
    const float* v = sd.f32(name + ".running_var", C);
    if (!w || !b || !m || !v) return I2V_E_MISSING;
    std::vector<float> ab((size_t)C * 2);
    for (int c = 0; c < C; ++c) {  // F.batch_norm eval: (x - mean) / sqrt(var + eps) * w + b, eps = 1e-5
        const double a = (double)w[c] / std::sqrt((double)v[c] + 1e-5);
        ab[2 * c] = (float)a;
        ab[2 * c + 1] = (float)((double)b[c] - (double)m[c] * a);
    }
    return out.w.upload(ab.data(), ab.size() * 4);
}

}  // namespace

extern "C" {

int i2v_embedder_create(int32_t z_dim, int32_t use_batchnorm, i2v_embedder** out) {
    I2V_REQUIRE(out && z_dim > 0, I2V_E_INVALID, "i2v_embedder_create: bad argument");
    return create_handle("i2v_embedder_create", out, [&](i2v_embedder* e) {
        e->E = z_dim;
        e->bn = use_batchnorm ? 1 : 0;
        const char* zp = nullptr;
        return zero_page(&zp);  // allocated here, not inside a forward
    });
}

void i2v_embedder_destroy(i2v_embedder* e) { delete e; }

static int embedder_pack(i2v_embedder* e, const StateDict& sd) {
    int rc;
    e->convs = std::vector<ResConv>(EMB_NCONV);
    e->norms = std::vector<ResNorm>(EMB_NNORM);
    const float* w = sd.f32("model.conv1.weight", 64 * 3 * 49);
    if (!w) return I2V_E_MISSING;
    if ((rc = e->convs[EMB_STEM].pack(w, 64, 3, 1, 7, 7, 2, 1))) return rc;
    if ((rc = load_norm(e, sd, "model.bn1", 64, e->norms[0]))) return rc;
    ResBlockSpec blocks[EMB_BLOCKS];
    embedder_blocks(blocks);
    for (int k = 0; k < EMB_BLOCKS; ++k) {
        const ResBlockSpec& b = blocks[k];
        const std::string p = embedder_prefix(b);
        const float* w1 = sd.f32(p + "conv1.weight", (int64_t)b.width * b.cin);
        const float* w2 = sd.f32(p + "conv2.weight", (int64_t)b.width * b.width * 9);
        const float* w3 = sd.f32(p + "conv3.weight", (int64_t)b.cout * b.width);
        if (!w1 || !w2 || !w3) return I2V_E_MISSING;
        if ((rc = e->convs[emb_conv(k, 0)].pack(w1, b.width, b.cin, 1, 1, 1, 1, 1))) return rc;
        if ((rc = e->convs[emb_conv(k, 1)].pack(w2, b.width, b.width, 1, 3, 3, b.ss, 1))) return rc;
        if ((rc = e->convs[emb_conv(k, 2)].pack(w3, b.cout, b.width, 1, 1, 1, 1, 1))) return rc;
        if ((rc = load_norm(e, sd, p + "bn1", b.width, e->norms[emb_norm(k, 0)]))) return rc;
        if ((rc = load_norm(e, sd, p + "bn2", b.width, e->norms[emb_norm(k, 1)]))) return rc;
        if ((rc = load_norm(e, sd, p + "bn3", b.cout, e->norms[emb_norm(k, 2)]))) return rc;
        if (!b.has_down) continue;
        const float* wdn = sd.f32(p + "downsample.0.weight", (int64_t)b.cout * b.cin);
        if (!wdn) return I2V_E_MISSING;
        if ((rc = e->convs[emb_conv(k, 3)].pack(wdn, b.cout, b.cin, 1, 1, 1, b.ss, 1))) return rc;
        if ((rc = load_norm(e, sd, p + "downsample.1", b.cout, e->norms[emb_norm(k, 3)]))) return rc;
    }
    // fc = Conv2d(2048, 2E, kernel = 1) (AE.py:121-124); .mode() keeps the mean = output channels [0, E)
    const float* fw = sd.f32("model.fc.sub_layers.0.weight", (int64_t)2 * e->E * 2048);
    const float* fb = sd.f32("model.fc.sub_layers.0.bias", (int64_t)2 * e->E);
    if (!fw || !fb) return I2V_E_MISSING;
    return e->convs[EMB_FC].pack(fw, e->E, 2048, 1, 1, 1, 1, 1, fb);
}

int i2v_embedder_load(i2v_embedder* e, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_embedder_load", e, tensors, n_tensors, embedder_pack);
}

size_t i2v_embedder_workspace_bytes(const i2v_embedder* e, int32_t batch, int32_t h, int32_t w) {
    if (!e || batch <= 0 || h <= 0 || w <= 0) return 0;
    return embedder_plan<Carver>(e->bn, batch, h, w, e->E).total;
}

int i2v_embedder_forward(i2v_embedder* e, const float* img, int32_t h, int32_t w, float* embed, void* workspace,
                         size_t workspace_bytes, int32_t batch, void* stream) {
    I2V_ENTER(sc, e, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_embedder_forward");
    I2V_REQUIRE(img && embed && workspace && batch > 0, I2V_E_INVALID, "i2v_embedder_forward: null argument");
    const ResnetPlan plan = embedder_plan<Carver>(e->bn, batch, h, w, e->E);
    if (plan.status) return plan_refusal(plan);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, plan.total, "i2v_embedder_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(e->order, st)) return rco;
    ResBufs bufs(plan, workspace);
    bufs.caller(RB_IN, img).caller(RB_OUT, embed);
    return launch(plan, e->convs, e->norms, bufs, st);
}

}  // extern "C"
