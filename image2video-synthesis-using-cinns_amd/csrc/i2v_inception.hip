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

namespace i2v {
namespace {

constexpr int INC_SIDE = 299;
constexpr int INC_MIN = 75;   // the smallest input that leaves a 1 x 1 map in front of the final pool

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

struct Map { int H, W; long pos() const { return (long)H * W; } };

struct ConvSpec { std::string name; int cin, cout, kh, kw, s, ph, pw; };

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
    ConvSpec spec;
    Map out(Map d) const { return Map{(d.H + 2 * spec.ph - spec.kh) / spec.s + 1, (d.W + 2 * spec.pw - spec.kw) / spec.s + 1}; }
    int pack(const float* wsrc, const float* g, const float* b, const float* m, const float* v) {
        FlatConvPacked p = flatconv_pack(wsrc, spec.cin, spec.cout, 0, spec.kh, spec.kw);
        flatconv_fold_bn(p, g, b, m, v, 1e-3);
        return upload(p);
    }
    int load(const StateDict& sd) {
        const float* wsrc = sd.f32(spec.name + ".conv.weight", (int64_t)spec.cout * spec.cin * spec.kh * spec.kw);
        const float* g = sd.f32(spec.name + ".bn.weight", spec.cout);
        const float* b = sd.f32(spec.name + ".bn.bias", spec.cout);
        const float* m = sd.f32(spec.name + ".bn.running_mean", spec.cout);
        const float* v = sd.f32(spec.name + ".bn.running_var", spec.cout);
        if (!wsrc || !g || !b || !m || !v) return I2V_E_MISSING;
        return pack(wsrc, g, b, m, v);
    }
};

// ---- topology: every Mixed block is a short program over the block input X, the block output Y and two temporaries T0, T1
enum { X = 0, T0 = 1, T1 = 2, Y = 3 };
enum { OP_CONV = 0, OP_POOL = 1 };
struct Op { int op, arg, src, dst, off; };   // conv: arg = unit of the block; pool: arg = I2V_INCEPTION_POOL_*; off: channel offset in Y
struct Block { std::string name; int cin = 0, cout = 0; std::vector<ConvSpec> convs; std::vector<Op> ops; };

ConvSpec cs(const std::string& n, int cin, int cout, int kh = 1, int kw = 1, int s = 1, int ph = 0, int pw = 0) {
    return ConvSpec{n, cin, cout, kh, kw, s, ph, pw};
}

// torchvision InceptionA with the FID patch (avg pool without the padding in its divisor); cat: 1x1, 5x5, 3x3dbl, pool
Block block_a(const std::string& n, int cin, int pf) {
    Block b{n, cin, 224 + pf};
    b.convs = {cs(n + ".branch1x1", cin, 64), cs(n + ".branch5x5_1", cin, 48), cs(n + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2),
               cs(n + ".branch3x3dbl_1", cin, 64), cs(n + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), cs(n + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
               cs(n + ".branch_pool", cin, pf)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, Y, 64}, {OP_CONV, 3, X, T0, 0}, {OP_CONV, 4, T0, T1, 0},
             {OP_CONV, 5, T1, Y, 128}, {OP_POOL, I2V_INCEPTION_POOL_AVG, X, T0, 0}, {OP_CONV, 6, T0, Y, 224}};
    return b;
}
// torchvision InceptionB (unpatched); cat: 3x3, 3x3dbl, max pool of the input
Block block_b(const std::string& n, int cin) {
    Block b{n, cin, 480 + cin};
    b.convs = {cs(n + ".branch3x3", cin, 384, 3, 3, 2), cs(n + ".branch3x3dbl_1", cin, 64), cs(n + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1),
               cs(n + ".branch3x3dbl_3", 96, 96, 3, 3, 2)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, T1, 0}, {OP_CONV, 3, T1, Y, 384},
             {OP_POOL, I2V_INCEPTION_POOL_MAX_S2, X, Y, 480}};
    return b;
}
// InceptionC with the FID patch; cat: 1x1, 7x7, 7x7dbl, pool
Block block_c(const std::string& n, int cin, int c7) {
    Block b{n, cin, 768};
    b.convs = {cs(n + ".branch1x1", cin, 192),
               cs(n + ".branch7x7_1", cin, c7), cs(n + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3), cs(n + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0),
               cs(n + ".branch7x7dbl_1", cin, c7), cs(n + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0), cs(n + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3),
               cs(n + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0), cs(n + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3),
               cs(n + ".branch_pool", cin, 192)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, T1, 0}, {OP_CONV, 3, T1, Y, 192},
             {OP_CONV, 4, X, T0, 0}, {OP_CONV, 5, T0, T1, 0}, {OP_CONV, 6, T1, T0, 0}, {OP_CONV, 7, T0, T1, 0}, {OP_CONV, 8, T1, Y, 384},
             {OP_POOL, I2V_INCEPTION_POOL_AVG, X, T0, 0}, {OP_CONV, 9, T0, Y, 576}};
    return b;
}
// torchvision InceptionD (unpatched); cat: 3x3, 7x7x3, max pool of the input
Block block_d(const std::string& n, int cin) {
    Block b{n, cin, 512 + cin};
    b.convs = {cs(n + ".branch3x3_1", cin, 192), cs(n + ".branch3x3_2", 192, 320, 3, 3, 2),
               cs(n + ".branch7x7x3_1", cin, 192), cs(n + ".branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3), cs(n + ".branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0),
               cs(n + ".branch7x7x3_4", 192, 192, 3, 3, 2)};
    b.ops = {{OP_CONV, 0, X, T0, 0}, {OP_CONV, 1, T0, Y, 0}, {OP_CONV, 2, X, T0, 0}, {OP_CONV, 3, T0, T1, 0}, {OP_CONV, 4, T1, T0, 0},
             {OP_CONV, 5, T0, Y, 320}, {OP_POOL, I2V_INCEPTION_POOL_MAX_S2, X, Y, 512}};
    return b;
}
// InceptionE with the FID patches: E_1 (Mixed_7b) the unpadded-divisor avg pool, E_2 (Mixed_7c) a MAX pool; cat: 1x1, 3x3 (2a, 2b),
// 3x3dbl (3a, 3b), pool
Block block_e(const std::string& n, int cin, int pool) {
    Block b{n, cin, 2048};
    b.convs = {cs(n + ".branch1x1", cin, 320),
               cs(n + ".branch3x3_1", cin, 384), cs(n + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), cs(n + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
               cs(n + ".branch3x3dbl_1", cin, 448), cs(n + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
               cs(n + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), cs(n + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
               cs(n + ".branch_pool", cin, 192)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, Y, 320}, {OP_CONV, 3, T0, Y, 704},
             {OP_CONV, 4, X, T0, 0}, {OP_CONV, 5, T0, T1, 0}, {OP_CONV, 6, T1, Y, 1088}, {OP_CONV, 7, T1, Y, 1472},
             {OP_POOL, pool, X, T0, 0}, {OP_CONV, 8, T0, Y, 1856}};
    return b;
}

constexpr int N_STEM = 5, N_MIXED = 11;
constexpr long INC_SUB_MAX = 1L << 31;   // floats per tensor of a sub-module call
constexpr long INC_MAX_FLOATS = 1L << 40;

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_inception {
    int device = 0;
    bool loaded = false;
    Unit stem[N_STEM];
    Block blocks[N_MIXED];
    std::vector<Unit> units[N_MIXED];
    StreamOrder order;
};

namespace {

void pool_geom(int kind, Map d, int* stride, int* pad, Map* o) {
    *stride = kind == I2V_INCEPTION_POOL_MAX_S2 ? 2 : 1;
    *pad = kind == I2V_INCEPTION_POOL_MAX_S2 ? 0 : 1;
    *o = Map{(d.H + 2 * *pad - 3) / *stride + 1, (d.W + 2 * *pad - 3) / *stride + 1};
}

int conv_launch(const Unit& u, int B, const float* in, int inCS, int inOff, Map di, float* out, int outCS, int outOff, hipStream_t st) {
    const Map d = u.out(di);
    I2V_REQUIRE(d.H > 0 && d.W > 0, I2V_E_INVALID, "inception conv %s: a [%d, %d] map is smaller than its window", u.spec.name.c_str(), di.H, di.W);
    const FlatConvMaps g{B, 1, di.H, di.W, 1, d.H, d.W, 1, u.spec.s, u.spec.s, 0, u.spec.ph, u.spec.pw};
    return flat_conv_launch<false>(("inception conv " + u.spec.name).c_str(), u, in, inCS, inOff, out, outCS, outOff, g, true, st);
}

int pool_launch(int kind, int B, const float* in, int C, Map di, float* out, int outCS, int outOff, hipStream_t st) {
    IncPoolArgs a{};
    Map o;
    pool_geom(kind, di, &a.stride, &a.pad, &o);
    I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "inception pool: a [%d, %d] map is smaller than the 3 x 3 window", di.H, di.W);
    I2V_REQUIRE(C > 0 && C % 4 == 0 && outCS % 4 == 0 && outOff % 4 == 0 && outOff >= 0 && outOff + C <= outCS, I2V_E_INVALID,
                "inception pool: %d channels -> [%d, +%d) of %d (multiples of 4 are needed)", C, outOff, C, outCS);
    a.in = in; a.out = out; a.N = B; a.Hi = di.H; a.Wi = di.W; a.Ho = o.H; a.Wo = o.W; a.C = C;
    a.avg = kind == I2V_INCEPTION_POOL_AVG ? 1 : 0; a.outCS = outCS; a.outOff = outOff;
    hipLaunchKernelGGL(inc_pool_kernel, dim3(grid_for((long)B * o.pos() * (C / 4))), dim3(256), 0, st, a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

// One walk of the network serves the block shapes and the workspace size (dry: no buffers, no launches) and the forward.
struct Walk {
    const i2v_inception* net;
    int B;
    bool dry;
    hipStream_t st;
    size_t act_floats = 0, t_floats[2] = {0, 0};   // dry: the largest block-level tensor / the largest use of each temporary
    Map bdim[4] = {};                              // map of every block output reached

    void need(size_t* slot, long floats) { *slot = std::max(*slot, (size_t)floats); }

    // Mixed block i: x [B][d][cin] -> y [B][*dout][cout]
    int mixed(int i, const float* x, Map d, float* y, float* t0, float* t1, Map* dout) {
        const Block& b = net->blocks[i];
        const float* src[4] = {x, t0, t1, nullptr};
        float* dst[4] = {nullptr, t0, t1, y};
        int cs_[4] = {b.cin, 0, 0, b.cout};   // channels of what each buffer holds
        Map dm[4] = {d, d, d, d};
        for (const Op& op : b.ops) {
            Map o;
            int c;
            if (op.op == OP_CONV) {
                const Unit& u = net->units[i][op.arg];
                o = u.out(dm[op.src]);
                c = u.spec.cout;
                I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "inception %s: a [%d, %d] map is too small", u.spec.name.c_str(), d.H, d.W);
                if (!dry)
                    if (int rc = conv_launch(u, B, src[op.src], cs_[op.src], 0, dm[op.src], dst[op.dst], op.dst == Y ? b.cout : c, op.off, st)) return rc;
            } else {
                int s, p;
                pool_geom(op.arg, dm[op.src], &s, &p, &o);
                c = cs_[op.src];
                I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "inception %s: a [%d, %d] map is too small", b.name.c_str(), d.H, d.W);
                if (!dry)
                    if (int rc = pool_launch(op.arg, B, src[op.src], c, dm[op.src], dst[op.dst], op.dst == Y ? b.cout : c, op.off, st)) return rc;
            }
            dm[op.dst] = o;
            if (op.dst != Y) {
                cs_[op.dst] = c;
                need(&t_floats[op.dst - T0], (long)B * o.pos() * c);
            }
        }
        *dout = dm[Y];
        need(&act_floats, (long)B * dout->pos() * b.cout);
        return I2V_OK;
    }

    // x [B][H][W][4] -> the requested blocks; a, b: the ping-pong buffers of block-level tensors (null when dry, as the taps may be)
    int run(const float* x, int H, int W, float* const* taps, int last, float* a, float* b, float* t0, float* t1) {
        int rc;
        Map d{H, W}, o;
        const float* cur = x;
        int C = 4;
        auto other = [&]() { return cur == a ? b : a; };
        auto conv = [&](const Unit& u, float* dst) {
            o = u.out(d);
            if (o.H <= 0 || o.W <= 0) { set_error("inception %s: a [%d, %d] map is too small", u.spec.name.c_str(), d.H, d.W); return (int)I2V_E_INVALID; }
            need(&act_floats, (long)B * o.pos() * u.spec.cout);
            if (!dry)
                if (int r = conv_launch(u, B, cur, C, 0, d, dst, u.spec.cout, 0, st)) return r;
            cur = dst; d = o; C = u.spec.cout;
            return (int)I2V_OK;
        };
        auto pool_a = [&](float* dst) {   // MaxPool2d(kernel_size=3, stride=2) between the stem blocks
            int s, p;
            pool_geom(I2V_INCEPTION_POOL_MAX_S2, d, &s, &p, &o);
            if (o.H <= 0 || o.W <= 0) { set_error("inception: a [%d, %d] map is too small for MaxPool2d(3, 2)", d.H, d.W); return (int)I2V_E_INVALID; }
            need(&act_floats, (long)B * o.pos() * C);
            if (!dry)
                if (int r = pool_launch(I2V_INCEPTION_POOL_MAX_S2, B, cur, C, d, dst, C, 0, st)) return r;
            cur = dst; d = o;
            return (int)I2V_OK;
        };
        const Unit* s = net->stem;
        // block 0: Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3, max pool
        if ((rc = conv(s[0], a)) || (rc = conv(s[1], b)) || (rc = conv(s[2], a)) || (rc = pool_a(taps[0] ? taps[0] : b))) return rc;
        bdim[0] = d;
        if (last == 0) return I2V_OK;
        // block 1: Conv2d_3b_1x1, Conv2d_4a_3x3, max pool
        if ((rc = conv(s[3], other())) || (rc = conv(s[4], other())) || (rc = pool_a(taps[1] ? taps[1] : other()))) return rc;
        bdim[1] = d;
        if (last == 1) return I2V_OK;
        // block 2: Mixed_5b .. Mixed_6e; block 3: Mixed_7a .. Mixed_7c, the global average
        for (int i = 0; i < N_MIXED; ++i) {
            float* y = i == 7 && taps[2] ? taps[2] : other();
            if ((rc = mixed(i, cur, d, y, t0, t1, &o))) return rc;
            cur = y; d = o; C = net->blocks[i].cout;
            if (i == 7) {
                bdim[2] = d;
                if (last == 2) return I2V_OK;
            }
        }
        bdim[3] = Map{1, 1};
        if (dry) return I2V_OK;
        hipLaunchKernelGGL(inc_global_avg_kernel, dim3(grid_for((long)B * C)), dim3(256), 0, st, cur, taps[3], (long)B, (int)d.pos(), C);
        I2V_HIP_CHECK(hipGetLastError());
        return I2V_OK;
    }
};

struct IncWs { size_t a, b, t0, t1, total; };

int inc_ws(const i2v_inception* net, int B, int H, int W, int last, IncWs* L, Map* bdim = nullptr) {
    Walk wk{net, B, true, nullptr};
    float* none[4] = {nullptr, nullptr, nullptr, nullptr};
    if (int rc = wk.run(nullptr, H, W, none, last, nullptr, nullptr, nullptr, nullptr)) return rc;
    if (bdim) std::copy(wk.bdim, wk.bdim + 4, bdim);
    Carver c;
    L->a = c.take_floats(wk.act_floats);
    L->b = c.take_floats(wk.act_floats);
    L->t0 = c.take_floats(wk.t_floats[0]);
    L->t1 = c.take_floats(wk.t_floats[1]);
    L->total = c.total();
    return I2V_OK;
}

const int BLOCK_C[4] = {64, 192, 768, 2048};

bool inc_dims_ok(int h, int w) { return h >= INC_MIN && w >= INC_MIN; }

}  // namespace

extern "C" {

// fid_inception_v3's graph, without weights
static int inception_graph(i2v_inception* n) {
    n->stem[0].spec = cs("Conv2d_1a_3x3", 3, 32, 3, 3, 2);
    n->stem[1].spec = cs("Conv2d_2a_3x3", 32, 32, 3, 3);
    n->stem[2].spec = cs("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
    n->stem[3].spec = cs("Conv2d_3b_1x1", 64, 80);
    n->stem[4].spec = cs("Conv2d_4a_3x3", 80, 192, 3, 3);
    n->blocks[0] = block_a("Mixed_5b", 192, 32);
    n->blocks[1] = block_a("Mixed_5c", 256, 64);
    n->blocks[2] = block_a("Mixed_5d", 288, 64);
    n->blocks[3] = block_b("Mixed_6a", 288);
    n->blocks[4] = block_c("Mixed_6b", 768, 128);
    n->blocks[5] = block_c("Mixed_6c", 768, 160);
    n->blocks[6] = block_c("Mixed_6d", 768, 160);
    n->blocks[7] = block_c("Mixed_6e", 768, 192);
    n->blocks[8] = block_d("Mixed_7a", 768);
    n->blocks[9] = block_e("Mixed_7b", 1280, I2V_INCEPTION_POOL_AVG);
    n->blocks[10] = block_e("Mixed_7c", 2048, I2V_INCEPTION_POOL_MAX_S1);
    for (int i = 0; i < N_MIXED; ++i) {
        n->units[i].resize(n->blocks[i].convs.size());
        for (size_t j = 0; j < n->units[i].size(); ++j) {
            n->units[i][j].spec = n->blocks[i].convs[j];
            if (const char* why = conv_shape_error(n->units[i][j].spec)) {
                set_error("i2v_inception_create: %s: %s", n->units[i][j].spec.name.c_str(), why);
                return I2V_E_INVALID;
            }
        }
    }
    return I2V_OK;
}

int i2v_inception_create(i2v_inception** out) { return create_handle("i2v_inception_create", out, inception_graph); }

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
    IncWs L;
    Map bd[4];
    if (int rc = inc_ws(n, 1, h, w, block, &L, bd)) return rc;
    dims[0] = bd[block].H; dims[1] = bd[block].W; dims[2] = BLOCK_C[block];
    return I2V_OK;
}

size_t i2v_inception_workspace_bytes(const i2v_inception* n, int32_t batch, int32_t h, int32_t w, int32_t last_block) {
    if (!n || batch <= 0 || !inc_dims_ok(h, w) || last_block < 0 || last_block > 3) return 0;
    IncWs L;
    if (inc_ws(n, batch, h, w, last_block, &L)) return 0;
    return L.total;
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
    float* taps[4] = {block0, block1, block2, block3};
    int last = -1;
    for (int k = 0; k < 4; ++k)
        if (taps[k]) last = k;
    I2V_REQUIRE(last >= 0, I2V_E_INVALID, "i2v_inception_features: no block requested");
    I2V_REQUIRE(inc_dims_ok(h, w), I2V_E_INVALID,
                "i2v_inception_features: a %d x %d input is too small: at least %d x %d is needed (the map in front of the final pool would be empty)", h,
                w, INC_MIN, INC_MIN);
    I2V_REQUIRE((long)batch * h * w * 32 < INC_MAX_FLOATS, I2V_E_INVALID, "i2v_inception_features: batch %d x [%d, %d] is too large", batch, h, w);
    IncWs L;
    if (int rc = inc_ws(n, batch, h, w, last, &L)) return rc;
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_inception_features");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    void* const ws = workspace;
    Walk wk{n, batch, false, st};
    return wk.run(x, h, w, taps, last, Carver::at(ws, L.a), Carver::at(ws, L.b), Carver::at(ws, L.t0), Carver::at(ws, L.t1));
}

// ---- sub-modules, individually callable on channels-last tensors (for tests and inspection)

int i2v_inception_conv_unit(const float* x, int32_t n, int32_t h, int32_t w, int32_t in_cs, int32_t in_off, const float* weight, const float* bn_weight,
                            const float* bn_bias, const float* bn_mean, const float* bn_var, int32_t cin, int32_t cout, int32_t kh, int32_t kw,
                            int32_t stride, int32_t pad_h, int32_t pad_w, float* out, int32_t out_cs, int32_t out_off, size_t out_floats, void* stream) {
    I2V_REQUIRE(x && weight && bn_weight && bn_bias && bn_mean && bn_var && out && n > 0 && h > 0 && w > 0, I2V_E_INVALID,
                "i2v_inception_conv_unit: bad argument");
    Unit u;
    u.spec = ConvSpec{"unit", cin, cout, kh, kw, stride, pad_h, pad_w};
    if (const char* why = conv_shape_error(u.spec)) {
        set_error("i2v_inception_conv_unit: %d -> %d channels, kernel (%d, %d), stride %d, padding (%d, %d): %s", cin, cout, kh, kw, stride, pad_h, pad_w, why);
        return I2V_E_INVALID;
    }
    const Map o = u.out(Map{h, w});
    I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "i2v_inception_conv_unit: a [%d, %d] map is smaller than the (%d, %d) window", h, w, kh, kw);
    I2V_REQUIRE((long)n * h * w * in_cs < INC_SUB_MAX && (long)n * o.pos() * out_cs < INC_SUB_MAX, I2V_E_INVALID,
                "i2v_inception_conv_unit: batch %d x [%d, %d] is too large", n, h, w);
    I2V_REQUIRE(out_cs > 0 && out_floats >= (size_t)n * o.pos() * out_cs, I2V_E_WORKSPACE, "i2v_inception_conv_unit: output of %zu floats < required %zu",
                out_floats, (size_t)n * o.pos() * out_cs);
    if (int rc = u.pack(weight, bn_weight, bn_bias, bn_mean, bn_var)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = conv_launch(u, n, x, in_cs, in_off, Map{h, w}, out, out_cs, out_off, st)) return rc;
    I2V_HIP_CHECK(hipStreamSynchronize(st));   // the packed weights die with this call
    return I2V_OK;
}

int i2v_inception_pool(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kind, float* out, int32_t out_cs, int32_t out_off,
                       size_t out_floats, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_inception_pool: bad argument");
    I2V_REQUIRE(kind == I2V_INCEPTION_POOL_MAX_S2 || kind == I2V_INCEPTION_POOL_MAX_S1 || kind == I2V_INCEPTION_POOL_AVG, I2V_E_INVALID,
                "i2v_inception_pool: unknown kind %d", kind);
    int s, p;
    Map o;
    pool_geom(kind, Map{h, w}, &s, &p, &o);
    I2V_REQUIRE(o.H > 0 && o.W > 0, I2V_E_INVALID, "i2v_inception_pool: a [%d, %d] map is smaller than the 3 x 3 window", h, w);
    I2V_REQUIRE(c > 0 && out_cs > 0 && (long)n * h * w * c < INC_SUB_MAX && (long)n * o.pos() * out_cs < INC_SUB_MAX, I2V_E_INVALID,
                "i2v_inception_pool: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    I2V_REQUIRE(out_floats >= (size_t)n * o.pos() * out_cs, I2V_E_WORKSPACE, "i2v_inception_pool: output of %zu floats < required %zu", out_floats,
                (size_t)n * o.pos() * out_cs);
    return pool_launch(kind, n, x, c, Map{h, w}, out, out_cs, out_off, static_cast<hipStream_t>(stream));
}

int i2v_inception_global_avg(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && h > 0 && w > 0 && c > 0, I2V_E_INVALID, "i2v_inception_global_avg: bad argument");
    I2V_REQUIRE((long)n * h * w * c < INC_SUB_MAX, I2V_E_INVALID, "i2v_inception_global_avg: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    hipLaunchKernelGGL(inc_global_avg_kernel, dim3(grid_for((long)n * c)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, (long)n, h * w, c);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_inception_mixed_shape(const i2v_inception* n, int32_t block, int32_t h, int32_t w, int32_t* cin, int32_t* cout, int32_t* out_hw) {
    I2V_REQUIRE(n && block >= 0 && block < N_MIXED && h > 0 && w > 0, I2V_E_INVALID, "i2v_inception_mixed_shape: block %d on a [%d, %d] map", block, h, w);
    Walk wk{n, 1, true, nullptr};
    Map o;
    if (int rc = wk.mixed(block, nullptr, Map{h, w}, nullptr, nullptr, nullptr, &o)) return rc;
    if (cin) *cin = n->blocks[block].cin;
    if (cout) *cout = n->blocks[block].cout;
    if (out_hw) { out_hw[0] = o.H; out_hw[1] = o.W; }
    return I2V_OK;
}

size_t i2v_inception_mixed_workspace_bytes(const i2v_inception* n, int32_t block, int32_t batch, int32_t h, int32_t w) {
    if (!n || block < 0 || block >= N_MIXED || batch <= 0 || h <= 0 || w <= 0) return 0;
    Walk wk{n, batch, true, nullptr};
    Map o;
    if (wk.mixed(block, nullptr, Map{h, w}, nullptr, nullptr, nullptr, &o)) return 0;
    return align_up(wk.t_floats[0] * 4, 256) + align_up(wk.t_floats[1] * 4, 256);
}

int i2v_inception_mixed_forward(i2v_inception* n, int32_t block, const float* x, int32_t batch, int32_t h, int32_t w, float* out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_inception_mixed_forward");
    I2V_REQUIRE(block >= 0 && block < N_MIXED, I2V_E_INVALID, "i2v_inception_mixed_forward: unknown block %d", block);
    I2V_REQUIRE(x && out && workspace && batch > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_inception_mixed_forward: bad argument");
    I2V_REQUIRE((long)batch * h * w * 2048 < INC_SUB_MAX, I2V_E_INVALID, "i2v_inception_mixed_forward: batch %d x [%d, %d] is too large", batch, h, w);
    Walk dry{n, batch, true, nullptr};
    Map o;
    if (int rc = dry.mixed(block, nullptr, Map{h, w}, nullptr, nullptr, nullptr, &o)) return rc;
    const size_t t0b = align_up(dry.t_floats[0] * 4, 256), need = t0b + align_up(dry.t_floats[1] * 4, 256);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, "i2v_inception_mixed_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    Walk wk{n, batch, false, st};
    return wk.mixed(block, x, Map{h, w}, out, Carver::at(workspace, 0), Carver::at(workspace, t0b), &o);
}

}  // extern "C"
