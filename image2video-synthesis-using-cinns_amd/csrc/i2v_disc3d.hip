// The temporal discriminator of stage-1 training: resnet3D.Discriminator (stage1_VAE/modules/resnet3D.py:222-301) forward and backward,
// spectral norm in training mode on block 0 of every layer, GroupNorm(16), the max pool, the head, the feature-map loss (loss.py:14-21).
// The C ABI is include/i2v_hip_disc3d.h.  Conventions of i2v_patchdisc.hip: exact fp32 on v_mfma_f32_16x16x4_f32; every sum has one owner
// and a fixed order, so two runs give the same bits.
// The trunk's conv, dgrad, wgrad, finish and pack kernels (__builtin_amdgcn_mfma_f32_16x16x4f32), their launchers and plan helpers are the
// Trunk3d family of i2v_train_conv.h, shared with the patch discriminator; GroupNorm and the pool are in i2v_res3d_trunk.h; the plan of
// the convs and blocks, the binding, the layout of `saved` and of the workspace, the spectral-norm bookkeeping and the forward and
// backward walks are in i2v_res3d_net.h.  The last two are shared with the motion encoder's training path (i2v_encoder_train.hip).
// Here: the head, the feature-map loss, the unit entries and the C entries.  The gradient penalty's gradient (include/i2v_hip_disc3d_gp.h)
// is the pair of walks of i2v_res3d_gp.h; its entries are at the end of this file.
//   * Activations are channels-last [N][T][H][W][C]; the clip is stored with 4 channels (r, g, b, 0).
//   * A forward packs W (/ sigma where the conv is spectral-normed) of every conv once, on the device, into wf [tap][cout][cin] and
//     wd [tap][cin][cout].  With I2V_DISC3D_SAVE they live in `saved` with that call's u, v and sigma.
//   * conv forward: implicit GEMM, 128 or 64 positions x BN channels per workgroup, K over (tap, channel) in chunks of 16 double-buffered
//     in LDS; windows (3, 3, 3) pad 1 and (3, 7, 7) pad (1, 3, 3); the last chunk of the stem (147 taps x 4 channels) is masked.
//   * dgrad: the same GEMM as a gather over input positions.  Along an axis of stride 2 a coordinate receives the taps of its parity
//     (window 3: one tap for an even coordinate, two for an odd one; window 7: three and four), so the positions are processed in
//     stride_t x stride_s x stride_s parity classes (blockIdx.y), each with its own tap list: no structural zero is multiplied.
//   * wgrad: per tap a [cout] x [cin] GEMM over the positions, cut into slices by wgrad_plan; the four waves of a workgroup take a
//     quarter of a slice each and are summed in wave order; tc_finish_a adds the slices in slice order, tc_finish_dot forms <dWn, W> once,
//     tc_finish_b applies the projection.
//   * GroupNorm: float64 statistics per (sample, group) from slices added in slice order; one apply pass; the backward's per-channel sums
//     likewise, then the two per-(sample, group) sums, then dx.
#include "i2v_handle.h"
#include "i2v_power_iter.h"
#include "i2v_res3d_trunk.h"
#include "i2v_res3d_net.h"
#include "i2v_res3d_gp.h"
#include "../../include/i2v_hip_disc3d.h"
#include "../../include/i2v_hip_disc3d_gp.h"

namespace i2v {
namespace {

constexpr int D3_FMAP_BLOCKS = 64;

// ------------------------------------------------------------------------------------------------------------------ head
// AvgPool3d((1, 4, 4)) over the [1, 4, 4] map, then fc: one workgroup per sample
__global__ __launch_bounds__(256) void d3_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ pred, int C) {
    __shared__ double red[256];
    const int n = blockIdx.x;
    double acc = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int p = 0; p < 16; ++p) s += x[((long)n * 16 + p) * C + c];
        acc += (double)(s * 0.0625f) * (double)w[c];
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) pred[n] = (float)acc;
}

// thread = channel: dx [n][16][c] = g[n] w[c] / 16; dweight[c] = sum over n (in order) of g[n] * pooled[n][c]
__global__ __launch_bounds__(256) void d3_head_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ dx, float* __restrict__ dw, int N, int C, int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float wc = w[c] * 0.0625f;
    double acc = 0.0;
    for (int n = 0; n < N; ++n) {
        float s = 0.f;
        for (int p = 0; p < 16; ++p) {
            s += x[((long)n * 16 + p) * C + c];
            if (dx) dx[((long)n * 16 + p) * C + c] = g[n] * wc;
        }
        acc += (double)g[n] * (double)(s * 0.0625f);
    }
    if (dw) dw[c] = accumulate ? dw[c] + (float)acc : (float)acc;
}

// ------------------------------------------------------------------------------------------------------------------ feature-map loss
__global__ __launch_bounds__(256) void d3_fmap_partial_kernel(const float* __restrict__ x, const float* __restrict__ y, long n, int metric, float coef,
                                                              float* __restrict__ dx, double* __restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) {
        const float d = x[i] - y[i];
        if (metric == I2V_FMAP_L1) {
            s += (double)fabsf(d);
            if (dx) dx[i] = d > 0.f ? coef : d < 0.f ? -coef : 0.f;
        } else {
            s += (double)d * (double)d;
            if (dx) dx[i] = 2.f * d * coef;
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

struct D3FmapFinal { long numel[4]; int nblk[4]; int nl; };
__global__ void d3_fmap_final_kernel(D3FmapFinal f, const double* __restrict__ partial, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int l = 0; l < f.nl; ++l) {
        double s = 0.0;
        for (int b = 0; b < f.nblk[l]; ++b) s += partial[l * D3_FMAP_BLOCKS + b];
        out[1 + l] = s / (double)f.numel[l];
        total += out[1 + l];
    }
    for (int l = f.nl; l < 4; ++l) out[1 + l] = 0.0;
    out[0] = total / (double)f.nl;
}

__global__ __launch_bounds__(256) void d3_sumsq_kernel(const float* __restrict__ x, long per, double* __restrict__ out) {
    __shared__ double red[256];
    const float* s = x + blockIdx.x * per;
    double q = 0.0;
    for (long i = threadIdx.x; i < per; i += 256) q += (double)s[i] * (double)s[i];
    q = block_sum(q, red);
    if (threadIdx.x == 0) out[blockIdx.x] = q;
}

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_disc3d {
    int device = 0;
    bool loaded = false;   // parameters bound
    bool have_grads = false;
    R3Trunk trunk;
    float *fc = nullptr, *gfc = nullptr;
};

namespace {

R3Layout d3_layout(const i2v_disc3d* d, int n, int t, int h, int w) { return r3_layout(d->trunk, n, t, h, w, R3Extra{"fc takes", {0, 0, 0}, 0}); }

int check_unit(const char* what, int n, int ti, int hi, int wi, int cin, int cout, int stem, int st, int ss) {
    I2V_REQUIRE(n > 0 && ti >= 1 && hi >= 1 && wi >= 1 && (st == 1 || st == 2) && (ss == 1 || ss == 2), I2V_E_INVALID,
                "%s: n %d, map %d x %d x %d, strides %d, %d", what, n, ti, hi, wi, st, ss);
    I2V_REQUIRE((stem ? cin == 3 : (cin > 0 && cin % 16 == 0)) && cout > 0 && cout % 16 == 0, I2V_E_INVALID,
                "%s: cin %d (a multiple of 16; the stem: 3), cout %d (a multiple of 16)", what, cin, cout);
    return I2V_OK;
}

// workspace of the unit entries
struct D3UnitWs { size_t wf, wd, part, dwn, dotp, total; };
D3UnitWs unit_ws(int n, int ti, int hi, int wi, int cin, int cout, int stem) {
    const TcConv c = make_conv(cin, cout, stem, 1, 1, 0);
    const TcGeo m = make_geo(n, ti, hi, wi, c);   // stride 1 has the most positions
    Carver k;
    D3UnitWs y{};
    y.wf = k.take_floats((size_t)ntap_of(c) * cout * c.cinp);
    y.wd = k.take_floats(pack_elems(c));
    y.part = k.take_floats(wgrad_part_floats(c, std::max<long>(m.mo, 1)) * 2);   // (a strided conv has fewer positions but may plan other slices)
    y.dwn = k.take_floats((size_t)cout * cin * ntap_of(c));
    y.dotp = k.take_bytes((finish_blocks(c) + 1) * 8);
    y.total = k.total();
    return y;
}

int pack_unit(const TcConv& c, const float* weight, float* wf, float* wd, hipStream_t st) {
    TcPackArgs p{};
    p.nconv = 1; p.total = (long)pack_elems(c);
    p.c[0] = TcPackConv{weight, nullptr, wf, wd, c.cout, c.cin, c.cinp, c.cind, ntap_of(c), 0};
    return launch_pack<Trunk3d>(p, st);
}

}  // namespace

extern "C" {

int i2v_disc3d_create(const i2v_disc3d_cfg* cfg, i2v_disc3d** out) {
    const char* what = "i2v_disc3d_create";
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(cfg->res_type == 18, I2V_E_INVALID, "%s: res type %d (only resnet18 is built)", what, cfg->res_type);
    for (int i = 0; i < 5; ++i)
        I2V_REQUIRE(cfg->channels[i] > 0 && cfg->channels[i] % 16 == 0, I2V_E_INVALID, "%s: channels[%d] = %d is not a positive multiple of 16", what, i,
                    cfg->channels[i]);
    for (int i = 0; i < 4; ++i)
        I2V_REQUIRE((cfg->stride_s[i] == 1 || cfg->stride_s[i] == 2) && (cfg->stride_t[i] == 1 || cfg->stride_t[i] == 2), I2V_E_INVALID,
                    "%s: layer %d has strides (t %d, s %d) outside {1, 2}", what, i, cfg->stride_t[i], cfg->stride_s[i]);
    const i2v_disc3d_cfg c = *cfg;
    return create_handle(what, out, [c](i2v_disc3d* d) {
        r3_build(d->trunk, c.channels, c.stride_s, c.stride_t, R3Rules{1, 2, c.spectral_norm ? 1 : 0, 1, c.use_max_pool ? 1 : 0, true});
        return I2V_OK;
    });
}

void i2v_disc3d_destroy(i2v_disc3d* d) { delete d; }

int i2v_disc3d_bind(i2v_disc3d* d, const i2v_tensor* params, int32_t n) {
    I2V_REQUIRE(d && params && n > 0, I2V_E_INVALID, "i2v_disc3d_bind: null argument");
    d->loaded = false;
    const StateDict sd(params, n);
    if (int rc = r3_bind(d->trunk, sd)) return rc;
    if (!bound_ptr(sd, "fc.weight", d->trunk.L[d->trunk.last()].cout, &d->fc)) return I2V_E_MISSING;
    d->loaded = true;
    return I2V_OK;
}

int i2v_disc3d_bind_grads(i2v_disc3d* d, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(d && (grads ? n > 0 : n == 0), I2V_E_INVALID, "i2v_disc3d_bind_grads: null handle, or a count without tensors");
    d->have_grads = false;
    if (!grads) return I2V_OK;
    const StateDict gd(grads, n);
    if (int rc = r3_bind_grads(d->trunk, gd)) return rc;
    if (!bound_ptr(gd, "fc.weight", d->trunk.L[d->trunk.last()].cout, &d->gfc)) return I2V_E_MISSING;
    d->have_grads = true;
    return I2V_OK;
}

int i2v_disc3d_out_shape(const i2v_disc3d* d, int32_t t, int32_t h, int32_t w, int32_t* shapes) {
    I2V_REQUIRE(d && shapes, I2V_E_INVALID, "i2v_disc3d_out_shape: null argument");
    const R3Layout y = d3_layout(d, 1, t, h, w);
    if (!y.ok) return r3_refuse("i2v_disc3d_out_shape", y);
    for (int l = 0; l < 4; ++l) {
        const int i = d->trunk.B[2 * l + 1].c2;
        shapes[4 * l] = y.geo[i].to; shapes[4 * l + 1] = y.geo[i].ho; shapes[4 * l + 2] = y.geo[i].wo; shapes[4 * l + 3] = d->trunk.L[i].cout;
    }
    return I2V_OK;
}

size_t i2v_disc3d_saved_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w) { return d ? d3_layout(d, n, t, h, w).saved_total : 0; }
size_t i2v_disc3d_workspace_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w) { return d ? d3_layout(d, n, t, h, w).ws_total : 0; }

int i2v_disc3d_saved_layout(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w, int32_t* count, int32_t* kind, int32_t* conv,
                            int32_t* dims, int64_t* offset) {
    I2V_REQUIRE(d && count && kind && conv && dims && offset, I2V_E_INVALID, "i2v_disc3d_saved_layout: null argument");
    const R3Layout y = d3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse("i2v_disc3d_saved_layout", y);
    R3Table tab{kind, conv, dims, offset};
    tab.put_convs(d->trunk, y, I2V_DISC3D_CONV_OUT, I2V_DISC3D_ACT);
    if (d->trunk.pool) {
        tab.put(I2V_DISC3D_POOL_OUT, -1, y.pt, y.pho, y.pwo, d->trunk.L[0].cout, y.pout);
        tab.put(I2V_DISC3D_POOL_ARGMAX, -1, y.pt, y.pho, y.pwo, d->trunk.L[0].cout, y.parg);
    }
    *count = tab.count;
    return I2V_OK;
}

int i2v_disc3d_forward(i2v_disc3d* d, const float* x, int32_t n, int32_t t, int32_t h, int32_t w, int32_t flags, float* pred, float* const* fmaps,
                       void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_forward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(x && pred && workspace, I2V_E_INVALID, "%s: null argument", what);
    const R3Layout y = d3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse(what, y);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    const bool save = flags & I2V_DISC3D_SAVE;
    if (save) {
        I2V_REQUIRE(saved, I2V_E_INVALID, "%s: I2V_DISC3D_SAVE without a saved buffer", what);
        I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = save ? saved : Carver::at<char>(workspace, y.fwd);
    if (int rc = r3_forward(d->trunk, y, x, flags & I2V_DISC3D_ITERATE, fmaps, sv, workspace, st)) return rc;
    const int last = d->trunk.last();
    hipLaunchKernelGGL(d3_head_fwd_kernel, dim3(n), dim3(256), 0, st, Carver::at(sv, y.act[last]), d->fc, pred, d->trunk.L[last].cout);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_disc3d_backward(i2v_disc3d* d, const float* d_pred, const float* const* d_fmaps, const void* saved, size_t saved_bytes, int32_t n, int32_t t,
                        int32_t h, int32_t w, float* d_x, int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes,
                        void* stream) {
    const char* what = "i2v_disc3d_backward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(saved && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(d_x || param_grads, I2V_E_INVALID, "%s: neither the input gradient nor the parameter gradients are asked for", what);
    bool any = d_pred != nullptr;
    for (int l = 0; l < 4 && d_fmaps; ++l) any = any || d_fmaps[l];
    I2V_REQUIRE(any, I2V_E_INVALID, "%s: no upstream gradient (d_pred and every d_fmaps entry are null)", what);
    I2V_REQUIRE(!param_grads || d->have_grads, I2V_E_STATE, "%s: no gradient tensors are bound", what);
    const R3Layout y = d3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse(what, y);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = const_cast<void*>(saved);
    const bool acc = accumulate != 0, pg = param_grads != 0;

    // the head: the gradient at the last activation -> gbuf[0]
    const int last = d->trunk.last(), C = d->trunk.L[last].cout;
    float* G = Carver::at(workspace, y.gbuf[0]);
    if (d_pred) {
        hipLaunchKernelGGL(d3_head_bwd_kernel, dim3((C + 255) / 256), dim3(256), 0, st, Carver::at(sv, y.act[last]), d->fc, d_pred, G,
                           pg ? d->gfc : nullptr, n, C, acc ? 1 : 0);
        I2V_LAUNCHED();
    } else {
        I2V_HIP_CHECK(hipMemsetAsync(G, 0, (size_t)n * 16 * C * 4, st));
        if (pg && !acc) I2V_HIP_CHECK(hipMemsetAsync(d->gfc, 0, (size_t)C * 4, st));
    }
    return r3_backward(d->trunk, y, d_fmaps, sv, d_x, pg, acc, workspace, st);
}

size_t i2v_disc3d_fmap_loss_workspace_bytes(void) { return (size_t)4 * D3_FMAP_BLOCKS * 8; }

int i2v_disc3d_fmap_loss(const float* const* a, const float* const* b, const int64_t* numel, int32_t n_layers, int32_t metric, float grad_scale, double* out,
                         float* const* d_a, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_fmap_loss";
    I2V_REQUIRE(a && b && numel && out && workspace && n_layers >= 1 && n_layers <= 4 && (metric == I2V_FMAP_L1 || metric == I2V_FMAP_L2), I2V_E_INVALID,
                "%s: null argument, %d layers or metric %d", what, n_layers, metric);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, i2v_disc3d_fmap_loss_workspace_bytes(), what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    D3FmapFinal f{};
    f.nl = n_layers;
    for (int l = 0; l < n_layers; ++l) {
        I2V_REQUIRE(a[l] && b[l] && numel[l] > 0, I2V_E_INVALID, "%s: layer %d is null or empty", what, l);
        f.numel[l] = numel[l];
        f.nblk[l] = (int)std::min<long>((numel[l] + 255) / 256, D3_FMAP_BLOCKS);
        const float coef = (float)((double)grad_scale / ((double)numel[l] * n_layers));
        hipLaunchKernelGGL(d3_fmap_partial_kernel, dim3(f.nblk[l]), dim3(256), 0, st, a[l], b[l], (long)numel[l], metric, coef, d_a ? d_a[l] : nullptr,
                           Carver::at<double>(workspace, 0) + l * D3_FMAP_BLOCKS);
        I2V_LAUNCHED();
    }
    hipLaunchKernelGGL(d3_fmap_final_kernel, dim3(1), dim3(64), 0, st, f, Carver::at<double>(workspace, 0), out);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_disc3d_sumsq(const float* x, int32_t n, int64_t per, double* out, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && per > 0, I2V_E_INVALID, "i2v_disc3d_sumsq: null argument, %d rows of %lld", n, (long long)per);
    hipLaunchKernelGGL(d3_sumsq_kernel, dim3(n), dim3(256), 0, static_cast<hipStream_t>(stream), x, (long)per, out);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_disc3d_wgrad_plan(int32_t cout, int32_t cin, int32_t taps, int64_t positions, int32_t* slices, int32_t* slice_len) {
    I2V_REQUIRE(slices && slice_len && positions > 0 && cout > 0 && cout % 16 == 0 && (cin == 3 || (cin > 0 && cin % 16 == 0)) && (taps == 27 || taps == 147),
                I2V_E_INVALID, "i2v_disc3d_wgrad_plan: cout %d, cin %d, %d taps, %lld positions", cout, cin, taps, (long long)positions);
    wgrad_plan(cout, cin, taps, positions, slices, slice_len);
    return I2V_OK;
}

size_t i2v_disc3d_unit_workspace_bytes(int32_t n, int32_t ti, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem) {
    if (n <= 0 || ti < 1 || hi < 1 || wi < 1 || cin <= 0 || cout <= 0) return 0;
    return unit_ws(n, ti, hi, wi, cin, cout, stem).total;
}

int i2v_disc3d_conv_unit(const float* x, const float* weight, int32_t n, int32_t ti, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem,
                         int32_t stride_t, int32_t stride_s, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_conv_unit";
    if (int rc = check_unit(what, n, ti, hi, wi, cin, cout, stem, stride_t, stride_s)) return rc;
    I2V_REQUIRE(x && weight && out && workspace, I2V_E_INVALID, "%s: null argument", what);
    const D3UnitWs k = unit_ws(n, ti, hi, wi, cin, cout, stem);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TcConv c = make_conv(cin, cout, stem, stride_t, stride_s, 0);
    if (int rc = pack_unit(c, weight, Carver::at(workspace, k.wf), Carver::at(workspace, k.wd), st)) return rc;
    return launch_conv<Trunk3d>(c, x, Carver::at(workspace, k.wf), out, make_geo(n, ti, hi, wi, c), st);
}

int i2v_disc3d_dgrad_unit(const float* g, const float* weight, const float* act, const float* add, const float* add_mask, int32_t n, int32_t ti, int32_t hi,
                          int32_t wi, int32_t cin, int32_t cout, int32_t stem, int32_t stride_t, int32_t stride_s, float* out, int32_t frames_out,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_dgrad_unit";
    if (int rc = check_unit(what, n, ti, hi, wi, cin, cout, stem, stride_t, stride_s)) return rc;
    I2V_REQUIRE(g && weight && out && workspace && (!frames_out || (cin == 3 && !add)) && (add || !add_mask), I2V_E_INVALID,
                "%s: null argument, frames_out with cin %d or with add, or add_mask without add", what, cin);
    const D3UnitWs k = unit_ws(n, ti, hi, wi, cin, cout, stem);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TcConv c = make_conv(cin, cout, stem, stride_t, stride_s, 0);
    if (int rc = pack_unit(c, weight, Carver::at(workspace, k.wf), Carver::at(workspace, k.wd), st)) return rc;
    return launch_dgrad<Trunk3d>(c, g, act, nullptr, Carver::at(workspace, k.wd), add, add_mask, out, frames_out != 0, n, make_geo(n, ti, hi, wi, c), st);
}

int i2v_disc3d_wgrad_unit(const float* g, const float* act, const float* x, const float* weight, const float* u, const float* v, const float* sigma,
                          int32_t n, int32_t ti, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stem, int32_t stride_t, int32_t stride_s,
                          int32_t accumulate, float* dweight, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_wgrad_unit";
    if (int rc = check_unit(what, n, ti, hi, wi, cin, cout, stem, stride_t, stride_s)) return rc;
    I2V_REQUIRE(g && x && weight && dweight && workspace && !u == !v && !u == !sigma, I2V_E_INVALID, "%s: null argument", what);
    const D3UnitWs k = unit_ws(n, ti, hi, wi, cin, cout, stem);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    const TcConv c = make_conv(cin, cout, stem, stride_t, stride_s, 0);
    return launch_wgrad<Trunk3d>(c, g, act, nullptr, x, weight, u, v, sigma, Carver::at(workspace, k.part), Carver::at(workspace, k.dwn),
                        Carver::at<double>(workspace, k.dotp), dweight, accumulate != 0, make_geo(n, ti, hi, wi, c), static_cast<hipStream_t>(stream));
}

size_t i2v_disc3d_groupnorm_workspace_bytes(int32_t n, int32_t c) { return n > 0 && c > 0 ? gn_ws(n, c).total : 0; }

int i2v_disc3d_groupnorm_unit(const float* x, const float* res, const float* weight, const float* bias, int32_t n, int64_t positions, int32_t c,
                              int32_t relu, float* out, double* stats, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_groupnorm_unit";
    I2V_REQUIRE(x && weight && bias && out && stats && workspace && n > 0 && positions > 0 && c > 0 && c % 16 == 0, I2V_E_INVALID,
                "%s: null argument, n %d, %lld positions or %d channels", what, n, (long long)positions, c);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, gn_ws(n, c).total, what);
    return launch_gn(x, res, weight, bias, n, positions, c, relu != 0, out, stats, workspace, static_cast<hipStream_t>(stream));
}

int i2v_disc3d_groupnorm_backward_unit(const float* g, const float* mask, const float* x, const double* stats, const float* weight, int32_t n,
                                       int64_t positions, int32_t c, float* dx, float* dweight, float* dbias, int32_t accumulate, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_groupnorm_backward_unit";
    I2V_REQUIRE(g && x && stats && weight && dx && workspace && !dweight == !dbias && n > 0 && positions > 0 && c > 0 && c % 16 == 0, I2V_E_INVALID,
                "%s: null argument, n %d, %lld positions or %d channels", what, n, (long long)positions, c);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, gn_ws(n, c).total, what);
    return launch_gn_bwd(g, mask, x, stats, weight, n, positions, c, dx, dweight, dbias, accumulate != 0, workspace, static_cast<hipStream_t>(stream));
}

int i2v_disc3d_maxpool_unit(const float* x, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, float* out, int32_t* argmax, void* stream) {
    I2V_REQUIRE(x && out && argmax && n > 0 && t > 0 && h > 0 && w > 0 && c > 0, I2V_E_INVALID, "i2v_disc3d_maxpool_unit: null argument or an empty map");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const long total = (long)n * t * ho * wo * c;
    hipLaunchKernelGGL(d3_maxpool_kernel, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, argmax, total, t, h, w, ho, wo, c);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_disc3d_maxpool_backward_unit(const float* g, const int32_t* argmax, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, float* dx, void* stream) {
    I2V_REQUIRE(g && argmax && dx && n > 0 && t > 0 && h > 0 && w > 0 && c > 0, I2V_E_INVALID, "i2v_disc3d_maxpool_backward_unit: null argument or an empty map");
    const int ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    const long total = (long)n * t * h * w * c;
    hipLaunchKernelGGL(d3_maxpool_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, static_cast<hipStream_t>(stream), g, argmax, dx, total, t, h, w, ho, wo, c);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_disc3d_head_unit(const float* x, const float* weight, const float* g, int32_t n, int32_t c, float* pred, float* dx, float* dweight, void* stream) {
    I2V_REQUIRE(x && weight && pred && n > 0 && c > 0 && (g ? dx != nullptr : !dx && !dweight), I2V_E_INVALID, "i2v_disc3d_head_unit: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(d3_head_fwd_kernel, dim3(n), dim3(256), 0, st, x, weight, pred, c);
    I2V_LAUNCHED();
    if (!g) return I2V_OK;
    hipLaunchKernelGGL(d3_head_bwd_kernel, dim3((c + 255) / 256), dim3(256), 0, st, x, weight, g, dx, dweight, n, c, 0);
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------ gradient penalty
namespace {

int gp_backward(const char* what, i2v_disc3d* d, const void* saved, size_t saved_bytes, int n, int t, int h, int w, float scale, const float* scale_dev,
                void* gp_saved, size_t gp_saved_bytes, double* l_gp, int accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(saved && gp_saved && l_gp && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(d->have_grads, I2V_E_STATE, "%s: no gradient tensors are bound", what);
    const R3Layout y = d3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse(what, y);
    const R3GpLayout p = r3_gp_layout(d->trunk, y);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    I2V_REQUIRE_WORKSPACE(gp_saved_bytes, p.saved_total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = const_cast<void*>(saved);
    const bool acc = accumulate != 0;
    const int last = d->trunk.last(), C = d->trunk.L[last].cout;

    // g = the gradient of mean(pred) at the clips, and the penalty's value
    float* seed = Carver::at(workspace, p.seed);
    float* dxf = Carver::at(workspace, p.dxf);
    double* sq = Carver::at<double>(workspace, p.sq);
    hipLaunchKernelGGL(d3g_seed_kernel, dim3((n + 255) / 256), dim3(256), 0, st, seed, n);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3_head_bwd_kernel, dim3((C + 255) / 256), dim3(256), 0, st, Carver::at(sv, y.act[last]), d->fc, seed,
                       Carver::at(workspace, y.gbuf[0]), static_cast<float*>(nullptr), n, C, 0);
    I2V_LAUNCHED();
    if (int rc = r3_backward(d->trunk, y, nullptr, sv, dxf, false, false, workspace, st)) return rc;
    const long thw = y.geo[0].mi / n;
    hipLaunchKernelGGL(d3_sumsq_kernel, dim3(n), dim3(256), 0, st, dxf, 3 * thw, sq);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3g_lgp_kernel, dim3(1), dim3(64), 0, st, sq, n, l_gp);
    I2V_LAUNCHED();

    // the tangent forward along (2 scale / n) g
    hipLaunchKernelGGL(d3g_tangent_input_kernel, dim3(grid_for(y.geo[0].mi)), dim3(256), 0, st, dxf, Carver::at(gp_saved, p.x4), y.geo[0].mi, thw, scale,
                       scale_dev, n);
    I2V_LAUNCHED();
    if (int rc = r3_tangent_forward(d->trunk, y, p, sv, gp_saved, workspace, st)) return rc;

    // the head: Pdot = (1 / n) sum_b fc . avg(a'_b) is the quantity differentiated; its adjoint is 1
    hipLaunchKernelGGL(d3g_head_dual_kernel, dim3((C + 255) / 256), dim3(256), 0, st, Carver::at(gp_saved, p.act[last]), d->fc, 1.f,
                       Carver::at(workspace, y.gbuf[0]), Carver::at(workspace, p.gbuf[0]), d->gfc, n, C, acc ? 1 : 0);
    I2V_LAUNCHED();
    return r3_dual_backward(d->trunk, y, p, sv, gp_saved, acc, workspace, st);
}

}  // namespace

extern "C" {

size_t i2v_disc3d_gp_saved_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w) {
    if (!d) return 0;
    const R3Layout y = d3_layout(d, n, t, h, w);
    return y.ok ? r3_gp_layout(d->trunk, y).saved_total : 0;
}

size_t i2v_disc3d_gp_workspace_bytes(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w) {
    if (!d) return 0;
    const R3Layout y = d3_layout(d, n, t, h, w);
    return y.ok ? r3_gp_layout(d->trunk, y).ws_total : 0;
}

int i2v_disc3d_gp_saved_layout(const i2v_disc3d* d, int32_t n, int32_t t, int32_t h, int32_t w, int32_t* count, int32_t* kind, int32_t* conv,
                               int32_t* dims, int64_t* offset) {
    I2V_REQUIRE(d && count && kind && conv && dims && offset, I2V_E_INVALID, "i2v_disc3d_gp_saved_layout: null argument");
    const R3Layout y = d3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse("i2v_disc3d_gp_saved_layout", y);
    const R3GpLayout p = r3_gp_layout(d->trunk, y);
    R3Table tab{kind, conv, dims, offset};
    for (int i = 0; i < d->trunk.nconv; ++i) {
        tab.put(I2V_DISC3D_GP_CONV_OUT, i, y.geo[i].to, y.geo[i].ho, y.geo[i].wo, d->trunk.L[i].cout, p.pre[i]);
        tab.put(I2V_DISC3D_GP_ACT, i, y.geo[i].to, y.geo[i].ho, y.geo[i].wo, d->trunk.L[i].cout, p.act[i]);
    }
    if (d->trunk.pool) tab.put(I2V_DISC3D_GP_POOL_OUT, -1, y.pt, y.pho, y.pwo, d->trunk.L[0].cout, p.pout);
    tab.put(I2V_DISC3D_GP_INPUT, -1, y.geo[0].ti, y.geo[0].hi, y.geo[0].wi, 4, p.x4);
    *count = tab.count;
    return I2V_OK;
}

int i2v_disc3d_gp_backward(i2v_disc3d* d, const void* saved, size_t saved_bytes, int32_t n, int32_t t, int32_t h, int32_t w, float scale,
                           void* gp_saved, size_t gp_saved_bytes, double* l_gp, int32_t accumulate, void* workspace, size_t workspace_bytes,
                           void* stream) {
    return gp_backward("i2v_disc3d_gp_backward", d, saved, saved_bytes, n, t, h, w, scale, nullptr, gp_saved, gp_saved_bytes, l_gp, accumulate, workspace,
                       workspace_bytes, stream);
}

int i2v_disc3d_gp_backward_dev(i2v_disc3d* d, const void* saved, size_t saved_bytes, int32_t n, int32_t t, int32_t h, int32_t w, float scale,
                               const float* scale_dev, void* gp_saved, size_t gp_saved_bytes, double* l_gp, int32_t accumulate, void* workspace,
                               size_t workspace_bytes, void* stream) {
    I2V_REQUIRE(scale_dev, I2V_E_INVALID, "i2v_disc3d_gp_backward_dev: null argument");
    return gp_backward("i2v_disc3d_gp_backward_dev", d, saved, saved_bytes, n, t, h, w, scale, scale_dev, gp_saved, gp_saved_bytes, l_gp, accumulate,
                       workspace, workspace_bytes, stream);
}

size_t i2v_disc3d_gp_groupnorm_workspace_bytes(int32_t n, int32_t c) { return n > 0 && c > 0 ? gp_gn_ws(n, c).total : 0; }

int i2v_disc3d_gp_groupnorm_tangent_unit(const float* x, const float* xd, const double* stats, const float* resd, const float* mask,
                                         const float* weight, int32_t n, int64_t positions, int32_t c, float* out, double* tstats, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_gp_groupnorm_tangent_unit";
    I2V_REQUIRE(x && xd && stats && weight && out && tstats && workspace && n > 0 && positions > 0 && c > 0 && c % 16 == 0, I2V_E_INVALID,
                "%s: null argument, n %d, %lld positions or %d channels", what, n, (long long)positions, c);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, gp_gn_ws(n, c).total, what);
    return launch_gn_tangent(x, xd, stats, resd, mask, weight, n, positions, c, out, tstats, workspace, static_cast<hipStream_t>(stream));
}

int i2v_disc3d_gp_groupnorm_dual_backward_unit(const float* g, const float* gd, const float* mask, const float* x, const float* xd,
                                               const double* stats, const double* tstats, const float* weight, int32_t n, int64_t positions,
                                               int32_t c, float* dx, float* dxd, float* dweight, float* dbias, int32_t accumulate, void* workspace,
                                               size_t workspace_bytes, void* stream) {
    const char* what = "i2v_disc3d_gp_groupnorm_dual_backward_unit";
    I2V_REQUIRE(g && gd && x && xd && stats && tstats && weight && dx && dxd && workspace && !dweight == !dbias && n > 0 && positions > 0 && c > 0 &&
                    c % 16 == 0,
                I2V_E_INVALID, "%s: null argument, n %d, %lld positions or %d channels", what, n, (long long)positions, c);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, gp_gn_ws(n, c).total, what);
    return launch_gn_dual_bwd(g, gd, mask, x, xd, stats, tstats, weight, n, positions, c, dx, dxd, dweight, dbias, accumulate != 0, workspace,
                              static_cast<hipStream_t>(stream));
}

int i2v_disc3d_gp_maxpool_tangent_unit(const float* xd, const int32_t* argmax, int32_t n, int32_t t, int32_t h, int32_t w, int32_t c, float* out,
                                       void* stream) {
    I2V_REQUIRE(xd && argmax && out && n > 0 && t > 0 && h > 0 && w > 0 && c > 0, I2V_E_INVALID,
                "i2v_disc3d_gp_maxpool_tangent_unit: null argument or an empty map");
    const long ho = (h - 1) / 2 + 1, wo = (w - 1) / 2 + 1;
    return launch_maxpool_tangent(xd, argmax, out, n, (long)t * ho * wo, (long)t * h * w, c, static_cast<hipStream_t>(stream));
}

int i2v_disc3d_gp_head_dual_unit(const float* xd, const float* weight, float s, int32_t n, int32_t c, float* pdot, float* dx, float* dxd,
                                 float* dweight, void* stream) {
    I2V_REQUIRE(xd && weight && pdot && dx && dxd && n > 0 && c > 0, I2V_E_INVALID, "i2v_disc3d_gp_head_dual_unit: null argument");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(d3_head_fwd_kernel, dim3(n), dim3(256), 0, st, xd, weight, pdot, c);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3g_head_dual_kernel, dim3((c + 255) / 256), dim3(256), 0, st, xd, weight, s, dx, dxd, dweight, n, c, 0);
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // extern "C"
