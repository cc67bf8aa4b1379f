// FID Inception-v3 trunk (torchvision's Inception3 graph with the pytorch-fid patches) up to the final average pool.
//
// Replaces metrics/FID/inception.py (InceptionV3.forward, fid_inception_v3, FIDInceptionA / C / E_1 / E_2 and the torchvision blocks
// InceptionB / D, BasicConv2d underneath) and the feature half of metrics/FID/FID_Score.py (get_activations); the statistics run on
// i2v_fvd_stats_update (i2v_i3d.hip) with D = 2048.
//
// Convolutions: flat_conv_kernel<NT, false> (i2v_flatconv.h), the 2-D unit, for 1x1, 3x3, 5x5, 1x7, 7x1, 1x3 and 3x1 windows at stride
// 1 or 2 with symmetric padding; BasicConv2d's eval-mode BatchNorm2d(eps = 0.001) folded to (scale, shift) at load, ReLU.
//
// Pools (channels-last, 4 channels per thread, taps in (dh, dw) order):
//   (a) MaxPool2d(3, stride 2): no padding, floor mode;
//   (b) max_pool2d(3, stride 1, padding 1): a tap outside the map never wins (-inf, NOT the zeros of the I3D pools);
//   (c) avg_pool2d(3, stride 1, padding 1, count_include_pad=False): the divisor is the number of taps inside the map;
//   (d) AdaptiveAvgPool2d((1, 1)): [N][H][W][C] -> [N][C].
#include <algorithm>
#include <cmath>

#include "i2v_flatconv.h"
#include "i2v_handle.h"
#include "i2v_trunk_plan.h"

namespace i2v {
namespace {

// InceptionV3.forward :144-151 fused with the layout change: frames [N][3][Hi][Wi] -> channels-last [N][Ho][Wo][4] (channel 3 zero),
// bilinear with align_corners=False in the arithmetic of torch's upsample_bilinear2d (Ho = Hi and Wo = Wi: weights (1, 0), the sample
// is the pixel itself), then 2 x - 1 when `normalize`.
__global__ __launch_bounds__(256) void inc_input_kernel(const float* __restrict__ frames, float* __restrict__ out, long N, int Hi, int Wi, int Ho,
                                                        int Wo, int normalize) {
    const long total = N * Ho * Wo;
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;   // area_pixel_compute_scale
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i % Wo), h = (int)((i / Wo) % Ho);
        const long n = i / ((long)Wo * Ho);
        // area_pixel_compute_source_index: max(scale * (dst + 0.5) - 0.5, 0)
        const float fh = fmaxf(sh * (h + 0.5f) - 0.5f, 0.f), fw = fmaxf(sw * (w + 0.5f) - 0.5f, 0.f);
        const int h0 = min((int)fh, Hi - 1), w0 = min((int)fw, Wi - 1);
        const int h1 = h0 + (h0 < Hi - 1 ? 1 : 0), w1 = w0 + (w0 < Wi - 1 ? 1 : 0);
        const float lh1 = fminf(fmaxf(fh - h0, 0.f), 1.f), lh0 = 1.f - lh1, lw1 = fminf(fmaxf(fw - w0, 0.f), 1.f), lw0 = 1.f - lw1;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = frames + (n * 3 + c) * (long)Hi * Wi;
            v[c] = lh0 * (lw0 * pl[(long)h0 * Wi + w0] + lw1 * pl[(long)h0 * Wi + w1]) + lh1 * (lw0 * pl[(long)h1 * Wi + w0] + lw1 * pl[(long)h1 * Wi + w1]);
            if (normalize) v[c] = 2.0f * v[c] - 1.0f;
        }
        *reinterpret_cast<float4*>(out + i * 4) = make_float4(v[0], v[1], v[2], 0.f);
    }
}

struct IncPoolArgs {
    const float* in; float* out;   // [N][Hi][Wi][C] -> channels [outOff, outOff + C) of [N][Ho][Wo][outCS]
    long N;
    int Hi, Wi, Ho, Wo, C, stride, pad, avg, outCS, outOff;
};
// 3 x 3 window; a tap outside the map takes no part: not in the maximum, not in the sum, not in the divisor
__global__ __launch_bounds__(256) void inc_pool_kernel(IncPoolArgs a) {
    const int C4 = a.C >> 2;
    const long total = a.N * a.Ho * a.Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % a.Wo);
        const int ho = (int)((p / a.Wo) % a.Ho);
        const long n = p / ((long)a.Wo * a.Ho);
        float4 m = a.avg ? make_float4(0.f, 0.f, 0.f, 0.f) : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        int cnt = 0;
        for (int dh = 0; dh < 3; ++dh) {
            const int h = ho * a.stride - a.pad + dh;
            if ((unsigned)h >= (unsigned)a.Hi) continue;
            for (int dw = 0; dw < 3; ++dw) {
                const int w = wo * a.stride - a.pad + dw;
                if ((unsigned)w >= (unsigned)a.Wi) continue;
                const float4 v = *reinterpret_cast<const float4*>(a.in + ((n * a.Hi + h) * a.Wi + w) * a.C + 4 * c4);
                if (a.avg) { m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w; }
                else { m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w); }
                ++cnt;
            }
        }
        if (a.avg) { const float d = (float)cnt; m.x /= d; m.y /= d; m.z /= d; m.w /= d; }
        *reinterpret_cast<float4*>(a.out + p * a.outCS + a.outOff + 4 * c4) = m;
    }
}

// AdaptiveAvgPool2d((1, 1)): [N][P][C] -> [N][C], the positions in order
__global__ __launch_bounds__(256) void inc_global_avg_kernel(const float* __restrict__ in, float* __restrict__ out, long N, int P, int C) {
    const long total = N * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const float* p = in + (i / C) * P * C + i % C;
        float s = 0.f;
        for (int j = 0; j < P; ++j) s += p[(long)j * C];
        out[i] = s / (float)P;
    }
}

const char* conv_shape_error(const ConvSpec& c) {
    if (!(c.cin == 3 || (c.cin > 0 && c.cin % 16 == 0))) return "input channels must be 3 (stored as r, g, b, 0) or a multiple of 16";
    if (c.cout <= 0) return "no output channels";
    if (c.kh < 1 || c.kh > 7 || c.kw < 1 || c.kw > 7) return "kernel extents must be 1 to 7";
    if (c.s != 1 && c.s != 2) return "stride must be 1 or 2";
    if (c.ph < 0 || c.ph >= c.kh || c.pw < 0 || c.pw >= c.kw) return "padding must be smaller than the kernel";
    return nullptr;
}

// One BasicConv2d: [Cout][Cin][KH][KW] packed as a 2-D flat conv unit, its BatchNorm2d(eps=0.001) in eval mode folded to (scale, shift)
struct Unit : FlatConv {
    const ConvSpec* spec = nullptr;
    int load(const StateDict& sd) {
        return FlatConv::load(sd, spec->name + ".conv.weight", spec->cin, spec->cout, 0, spec->kh, spec->kw, spec->name + ".bn", 1e-3);
    }
};

constexpr long INC_MAX_FLOATS = 1L << 40;

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_inception {
    int device = 0;
    bool loaded = false;
    Unit stem[N_STEM];
    std::vector<Unit> units[N_MIXED];   // the convs of inception_graph().blocks
    StreamOrder order;
};

namespace {

int conv_launch(const Unit& u, int B, const Step& s, const float* in, float* out, hipStream_t st) {
    const FlatConvMaps g{B, 1, s.in.H, s.in.W, 1, s.out.H, s.out.W, 1, s.s[1], s.s[2], 0, s.p[1], s.p[2]};
    return flat_conv_launch<false>(("inception conv " + u.spec->name).c_str(), u, in, s.inCS, s.inOff, out, s.outCS, s.outOff, g, true, st);
}

int pool_launch(int B, const Step& s, const float* in, float* out, hipStream_t st) {
    I2V_REQUIRE(s.C > 0 && s.C % 4 == 0 && s.outCS % 4 == 0 && s.outOff % 4 == 0 && s.outOff >= 0 && s.outOff + s.C <= s.outCS, I2V_E_INVALID,
                "inception pool: %d channels -> [%d, +%d) of %d (multiples of 4 are needed)", s.C, s.outOff, s.C, s.outCS);
    const IncPoolArgs a{in, out, B, s.in.H, s.in.W, s.out.H, s.out.W, s.C, s.s[1], s.p[1], s.pool == I2V_INCEPTION_POOL_AVG ? 1 : 0, s.outCS, s.outOff};
    hipLaunchKernelGGL(inc_pool_kernel, dim3(grid_for((long)B * s.out.pos() * (s.C / 4))), dim3(256), 0, st, a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

// The launches of a plan (i2v_trunk_plan.h), in order
int launch(const i2v_inception* n, const TrunkPlan& p, const TrunkBufs& buf, hipStream_t st) {
    for (const Step& s : p.steps) {
        const float* in = buf.p[s.src];
        float* out = buf.p[s.dst];
        switch (s.kind) {
        case STEP_CONV:
            if (int rc = conv_launch(s.block < 0 ? n->stem[s.unit] : n->units[s.block][s.unit], p.B, s, in, out, st)) return rc;
            break;
        case STEP_INC_POOL:
            if (int rc = pool_launch(p.B, s, in, out, st)) return rc;
            break;
        case STEP_GLOBAL_AVG:
            hipLaunchKernelGGL(inc_global_avg_kernel, dim3(grid_for((long)p.B * s.C)), dim3(256), 0, st, in, out, (long)p.B, (int)s.in.pos(), s.C);
            I2V_HIP_CHECK(hipGetLastError());
            break;
        default:
            I2V_REQUIRE(false, I2V_E_INVALID, "inception: step kind %d", s.kind);
        }
    }
    return I2V_OK;
}

// plan of the Mixed entries: the caller's tensor in BUF_IN, its output in BUF_OUT, the workspace carved into T0 and T1
TrunkPlan mixed_plan(int block, int B, Map3 d) {
    TrunkPlan p(B);
    if (inc_mixed(p, block, BUF_IN, d, BUF_OUT, BUF_NONE)) p.carve<Carver>();
    return p;
}

}  // namespace

extern "C" {

// the units of fid_inception_v3's graph, without weights
static int bind_graph(i2v_inception* n) {
    const InceptionGraph& g = inception_graph();
    for (int j = 0; j < N_STEM; ++j) n->stem[j].spec = &g.stem[j];
    for (int i = 0; i < N_MIXED; ++i) {
        n->units[i].resize(g.blocks[i].convs.size());
        for (size_t j = 0; j < n->units[i].size(); ++j) {
            n->units[i][j].spec = &g.blocks[i].convs[j];
            if (const char* why = conv_shape_error(g.blocks[i].convs[j])) {
                set_error("i2v_inception_create: %s: %s", g.blocks[i].convs[j].name.c_str(), why);
                return I2V_E_INVALID;
            }
        }
    }
    return I2V_OK;
}

int i2v_inception_create(i2v_inception** out) { return create_handle("i2v_inception_create", out, bind_graph); }

void i2v_inception_destroy(i2v_inception* n) { delete n; }

static int inception_pack(i2v_inception* n, const StateDict& sd) {
    for (Unit& u : n->stem)
        if (int rc = u.load(sd)) return rc;
    for (auto& us : n->units)
        for (Unit& u : us)
            if (int rc = u.load(sd)) return rc;
    return I2V_OK;
}

int i2v_inception_load(i2v_inception* n, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_inception_load", n, tensors, n_tensors, inception_pack);
}

int i2v_inception_block_shape(const i2v_inception* n, int32_t h, int32_t w, int32_t block, int32_t* dims) {
    I2V_REQUIRE(n && dims && block >= 0 && block <= 3, I2V_E_INVALID, "i2v_inception_block_shape: bad argument");
    I2V_REQUIRE(inc_dims_ok(h, w), I2V_E_INVALID, "i2v_inception_block_shape: a %d x %d input is too small (at least %d x %d is needed)", h, w, INC_MIN,
                INC_MIN);
    const TrunkPlan p = inception_plan<Carver>(1, h, w, block, 0);
    if (p.status) return plan_refusal(p);
    dims[0] = p.block[block].H; dims[1] = p.block[block].W; dims[2] = BLOCK_C[block];
    return I2V_OK;
}

size_t i2v_inception_workspace_bytes(const i2v_inception* n, int32_t batch, int32_t h, int32_t w, int32_t last_block) {
    if (!n || batch <= 0 || !inc_dims_ok(h, w) || last_block < 0 || last_block > 3) return 0;
    const TrunkPlan p = inception_plan<Carver>(batch, h, w, last_block, 0);
    return p.status ? (plan_refusal(p), 0) : p.total;
}

int i2v_inception_input_stage(const float* frames, int32_t n, int32_t hi, int32_t wi, int32_t resize, int32_t normalize, float* out, void* stream) {
    I2V_REQUIRE(frames && out && n > 0 && hi > 0 && wi > 0, I2V_E_INVALID, "i2v_inception_input_stage: bad argument");
    const int ho = resize ? INC_SIDE : hi, wo = resize ? INC_SIDE : wi;
    I2V_REQUIRE((long)n * 3 * hi * wi < INC_MAX_FLOATS && (long)n * 4 * ho * wo < INC_MAX_FLOATS, I2V_E_INVALID,
                "i2v_inception_input_stage: %d frames is too large", n);
    hipLaunchKernelGGL(inc_input_kernel, dim3(grid_for((long)n * ho * wo)), dim3(256), 0, static_cast<hipStream_t>(stream), frames, out, (long)n, hi, wi,
                       ho, wo, normalize ? 1 : 0);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_inception_features(i2v_inception* n, const float* x, int32_t batch, int32_t h, int32_t w, float* block0, float* block1, float* block2,
                           float* block3, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_inception_features");
    I2V_REQUIRE(x && workspace && batch > 0, I2V_E_INVALID, "i2v_inception_features: bad argument");
    TrunkBufs buf(x, nullptr);
    buf.p[INC_TAP0] = block0; buf.p[INC_TAP1] = block1; buf.p[INC_TAP2] = block2; buf.p[INC_TAP3] = block3;
    int last = -1;
    unsigned taps = 0;
    for (int k = 0; k < 4; ++k)
        if (buf.p[INC_TAP0 + k]) { last = k; taps |= 1u << k; }
    I2V_REQUIRE(last >= 0, I2V_E_INVALID, "i2v_inception_features: no block requested");
    I2V_REQUIRE(inc_dims_ok(h, w), I2V_E_INVALID,
                "i2v_inception_features: a %d x %d input is too small: at least %d x %d is needed (the map in front of the final pool would be empty)", h,
                w, INC_MIN, INC_MIN);
    I2V_REQUIRE((long)batch * h * w * 32 < INC_MAX_FLOATS, I2V_E_INVALID, "i2v_inception_features: batch %d x [%d, %d] is too large", batch, h, w);
    const TrunkPlan p = inception_plan<Carver>(batch, h, w, last, taps);
    if (p.status) return plan_refusal(p);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.total, "i2v_inception_features");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    return launch(n, p, buf.carve(p, workspace), st);
}

// ---- sub-modules, individually callable on channels-last tensors (for tests and inspection)

int i2v_inception_conv_unit(const float* x, int32_t n, int32_t h, int32_t w, int32_t in_cs, int32_t in_off, const float* weight, const float* bn_weight,
                            const float* bn_bias, const float* bn_mean, const float* bn_var, int32_t cin, int32_t cout, int32_t kh, int32_t kw,
                            int32_t stride, int32_t pad_h, int32_t pad_w, float* out, int32_t out_cs, int32_t out_off, size_t out_floats, void* stream) {
    I2V_REQUIRE(x && weight && bn_weight && bn_bias && bn_mean && bn_var && out && n > 0 && h > 0 && w > 0, I2V_E_INVALID,
                "i2v_inception_conv_unit: bad argument");
    const ConvSpec spec{"unit", cin, cout, kh, kw, stride, pad_h, pad_w};
    if (const char* why = conv_shape_error(spec)) {
        set_error("i2v_inception_conv_unit: %d -> %d channels, kernel (%d, %d), stride %d, padding (%d, %d): %s", cin, cout, kh, kw, stride, pad_h, pad_w, why);
        return I2V_E_INVALID;
    }
    const Step s = inc_conv_step(spec, -1, 0, BUF_IN, in_cs, in_off, Map3{1, h, w}, BUF_OUT, out_cs, out_off);
    const Map3 o = s.out;
    I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "i2v_inception_conv_unit: a [%d, %d] map is smaller than the (%d, %d) window", h, w, kh, kw);
    I2V_REQUIRE((long)n * h * w * in_cs < TRUNK_SUB_MAX && (long)n * o.pos() * out_cs < TRUNK_SUB_MAX, I2V_E_INVALID,
                "i2v_inception_conv_unit: batch %d x [%d, %d] is too large", n, h, w);
    I2V_REQUIRE(out_cs > 0 && out_floats >= (size_t)n * o.pos() * out_cs, I2V_E_WORKSPACE, "i2v_inception_conv_unit: output of %zu floats < required %zu",
                out_floats, (size_t)n * o.pos() * out_cs);
    Unit u;
    u.spec = &spec;
    FlatConvPacked packed = flatconv_pack(weight, cin, cout, 0, kh, kw);
    flatconv_fold_bn(packed, bn_weight, bn_bias, bn_mean, bn_var, 1e-3);
    if (int rc = u.upload(packed)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = conv_launch(u, n, s, x, out, st)) return rc;
    I2V_HIP_CHECK(hipStreamSynchronize(st));   // the packed weights die with this call
    return I2V_OK;
}

int i2v_inception_pool(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kind, float* out, int32_t out_cs, int32_t out_off,
                       size_t out_floats, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_inception_pool: bad argument");
    I2V_REQUIRE(kind == I2V_INCEPTION_POOL_MAX_S2 || kind == I2V_INCEPTION_POOL_MAX_S1 || kind == I2V_INCEPTION_POOL_AVG, I2V_E_INVALID,
                "i2v_inception_pool: unknown kind %d", kind);
    const Step s = inc_pool_step(kind, BUF_IN, c, Map3{1, h, w}, BUF_OUT, out_cs, out_off);
    const Map3 o = s.out;
    I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "i2v_inception_pool: a [%d, %d] map is smaller than the 3 x 3 window", h, w);
    I2V_REQUIRE(c > 0 && out_cs > 0 && (long)n * h * w * c < TRUNK_SUB_MAX && (long)n * o.pos() * out_cs < TRUNK_SUB_MAX, I2V_E_INVALID,
                "i2v_inception_pool: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    I2V_REQUIRE(out_floats >= (size_t)n * o.pos() * out_cs, I2V_E_WORKSPACE, "i2v_inception_pool: output of %zu floats < required %zu", out_floats,
                (size_t)n * o.pos() * out_cs);
    return pool_launch(n, s, x, out, static_cast<hipStream_t>(stream));
}

int i2v_inception_global_avg(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && h > 0 && w > 0 && c > 0, I2V_E_INVALID, "i2v_inception_global_avg: bad argument");
    I2V_REQUIRE((long)n * h * w * c < TRUNK_SUB_MAX, I2V_E_INVALID, "i2v_inception_global_avg: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    hipLaunchKernelGGL(inc_global_avg_kernel, dim3(grid_for((long)n * c)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, (long)n, h * w, c);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_inception_mixed_shape(const i2v_inception* n, int32_t block, int32_t h, int32_t w, int32_t* cin, int32_t* cout, int32_t* out_hw) {
    I2V_REQUIRE(n && block >= 0 && block < N_MIXED && h > 0 && w > 0, I2V_E_INVALID, "i2v_inception_mixed_shape: block %d on a [%d, %d] map", block, h, w);
    const TrunkPlan p = mixed_plan(block, 1, Map3{1, h, w});
    if (p.status) return plan_refusal(p);
    if (cin) *cin = inception_graph().blocks[block].cin;
    if (cout) *cout = inception_graph().blocks[block].cout;
    if (out_hw) { out_hw[0] = p.out.H; out_hw[1] = p.out.W; }
    return I2V_OK;
}

size_t i2v_inception_mixed_workspace_bytes(const i2v_inception* n, int32_t block, int32_t batch, int32_t h, int32_t w) {
    if (!n || block < 0 || block >= N_MIXED || batch <= 0 || h <= 0 || w <= 0) return 0;
    const TrunkPlan p = mixed_plan(block, batch, Map3{1, h, w});
    return p.status ? (plan_refusal(p), 0) : p.total;
}

int i2v_inception_mixed_forward(i2v_inception* n, int32_t block, const float* x, int32_t batch, int32_t h, int32_t w, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_inception_mixed_forward");
    I2V_REQUIRE(block >= 0 && block < N_MIXED, I2V_E_INVALID, "i2v_inception_mixed_forward: unknown block %d", block);
    I2V_REQUIRE(x && out && workspace && batch > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_inception_mixed_forward: bad argument");
    I2V_REQUIRE((long)batch * h * w * 2048 < TRUNK_SUB_MAX, I2V_E_INVALID, "i2v_inception_mixed_forward: batch %d x [%d, %d] is too large", batch, h, w);
    const TrunkPlan p = mixed_plan(block, batch, Map3{1, h, w});
    if (p.status) return plan_refusal(p);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.total, "i2v_inception_mixed_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    return launch(n, p, TrunkBufs(x, out).carve(p, workspace), st);
}

}  // extern "C"
