// The implicit-GEMM conv of the evaluation trunks on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32): every conv unit of the
// I3D networks (i2v_i3d.hip, 3-D) and of the Inception-v3 trunk (i2v_inception.hip, 2-D).  Included by both, inside no namespace; the
// kernel has internal linkage in each translation unit, as the one of i2v_conv16w4_kernel.h has.
//   Out[m = (b, to, ho, wo) flattened][n] = act(scale[n] * sum_k In[gather(m, k)] * W[k][n] + shift[n])
// conv_forward (i2v_conv.hip) tiles T, H, W into bricks of 128 positions and pads symmetrically; these networks have 14 x 14, 8 x 8 and
// 7 x 7 maps, asymmetric "TF SAME" padding, rectangular windows and Mixed blocks whose branches write channel slices of one tensor.  So:
//   * positions are flattened over B * To * Ho * Wo, 128 per workgroup, the last tile masked;
//   * K is flattened over (tap = (dt * KH + dh) * KW + dw, channel) in groups of 4 channels: a 16-wide K chunk of a conv on the image
//     (4 channels: r, g, b, 0) holds 4 taps, a chunk of a 1x1 unit 16 channels -- one gather path for every window, no padded K work
//     on the image;
//   * the window, the stride and the padding in front per dimension are arguments; so are the channel stride / offset of the input and
//     of the output (the branches of a Mixed block store straight into their slice: there is no concat kernel);
//   * epilogue: (scale, shift) per output channel -- a folded eval-mode BatchNorm, a bias or the identity (i2v_flatconv_pack.h) --
//     and ReLU when asked for;
//   * TIME = false is the 2-D unit: no time division, tap split, bound check or address term (NOT a 3-D unit with T = 1).
// 4 waves x (32 rows x BN columns) per workgroup, BN = 16 NT in {32, 64, 128} per unit; A and W chunks are double-buffered in LDS (rows
// of 16 floats padded to 20: conflict-free ds_read_b128), the next chunk's global loads are in flight during the MFMAs: one barrier
// per chunk.  Loads are unconditional with clamped addresses.  The K order of an output element depends on neither the batch nor the
// tile it falls in: batch rows equal their single-sample runs bit for bit, and there are no atomics anywhere.
#pragma once
#include "i2v_common.h"
#include "i2v_flatconv_pack.h"

namespace i2v {
namespace {

constexpr int FLATCONV_BM = 128;
constexpr int FLATCONV_LS = 20;    // floats per staged row of 16

struct FlatConvArgs {
    const float* in;     // channels-last [B][Ti][Hi][Wi][inCS], the unit reads channels [inOff, inOff + 4 C4)
    const float* wp;     // [nchunk][CoutPad][16]
    const float2* ss;    // [CoutPad] (scale, shift)
    float* out;          // [M][outCS], the unit writes channels [outOff, outOff + Cout)
    long M;
    int Ti, Hi, Wi, To, Ho, Wo;       // a 2-D unit: Ti = To = 1 (not read)
    int inCS, inOff, C4, G, nchunk;   // C4: groups of 4 input channels, G = taps * C4
    int KH, KW, sT, sH, sW, pT, pH, pW;
    int Cout, CoutPad, outCS, outOff, relu;
};

template <int NT, bool TIME>   // 16-column tiles per wave: BN = 16 NT; TIME: the map has a time dimension
__global__ __launch_bounds__(256) void flat_conv_kernel(FlatConvArgs a) {
    constexpr int BN = 16 * NT;
    constexpr int WLD = (BN * 4 + 255) / 256;
    __shared__ __attribute__((aligned(16))) float a_lds[2][FLATCONV_BM * FLATCONV_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * FLATCONV_LS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int nNt = a.CoutPad / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * FLATCONV_BM;
    const int q = tid & 3;

    // the two staged rows of this thread: output position -> first input coordinate of its window
    int rb[2], rh[2], rw[2];
    [[maybe_unused]] int rt[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < a.M;
        if (!ok) m = 0;
        const int wo = (int)(m % a.Wo); m /= a.Wo;
        const int ho = (int)(m % a.Ho); m /= a.Ho;
        if constexpr (TIME) {
            const int to = (int)(m % a.To); m /= a.To;
            rt[u] = to * a.sT - a.pT;
        }
        rb[u] = ok ? (int)m : -1;
        rh[u] = ho * a.sH - a.pH; rw[u] = wo * a.sW - a.pW;
    }
    [[maybe_unused]] const int khw = a.KH * a.KW;

    static_assert(WLD <= 2, "weight pieces per thread");
    float4 pa0, pa1, pw0, pw1;   // (named, not arrays: arrays written under a branch go to scratch)
    pw1 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const bool gok = g < a.G;
        const int tap = gok ? g / a.C4 : 0;
        const int c = (g - tap * a.C4) * 4;
        int dt = 0, r2 = tap;
        if constexpr (TIME) { dt = tap / khw; r2 = tap - dt * khw; }
        const int dh = r2 / a.KW, dw = r2 - dh * a.KW;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int h = rh[u] + dh, w = rw[u] + dw;
            bool ok = gok && rb[u] >= 0;
            long row = rb[u];
            if constexpr (TIME) {
                const int t = rt[u] + dt;
                ok = ok && (unsigned)t < (unsigned)a.Ti;
                row = row * a.Ti + t;
            }
            ok = ok && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
            const long off = ok ? ((row * a.Hi + h) * a.Wi + w) * a.inCS + a.inOff + c : 0;
            const float4 v = *reinterpret_cast<const float4*>(a.in + off);
            const float4 z = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (u == 0) pa0 = z; else pa1 = z;
        }
        const float* wsrc = a.wp + ((long)ch * a.CoutPad + n0) * 16;
        pw0 = *reinterpret_cast<const float4*>(wsrc + (tid < BN * 4 ? tid : 0) * 4);
        if constexpr (WLD > 1) pw1 = *reinterpret_cast<const float4*>(wsrc + (tid + 256) * 4);
    };
    auto park = [&](int buf) {
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * FLATCONV_LS + 4 * q]) = pa0;
        *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * FLATCONV_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * FLATCONV_LS + 4 * q]) = pw0;
        if constexpr (WLD > 1) *reinterpret_cast<float4*>(&w_lds[buf][((tid + 256) >> 2) * FLATCONV_LS + 4 * q]) = pw1;
    };

    f32x4 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    request(0);
    park(0);
    __syncthreads();
    for (int ch = 0; ch < a.nchunk; ++ch) {
        const int buf = ch & 1;
        request(ch + 1 < a.nchunk ? ch + 1 : ch);
        // MFMA k-slot (lane >> 4) of step s carries K element 4 (lane >> 4) + s of the chunk, for both operands
        float4 av[2], bv[NT];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 32 + 16 * mt + lr) * FLATCONV_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * FLATCONV_LS + 4 * kq]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float as = s == 0 ? av[mt].x : s == 1 ? av[mt].y : s == 2 ? av[mt].z : av[mt].w;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float bs = s == 0 ? bv[nt].x : s == 1 ? bv[nt].y : s == 2 ? bv[nt].z : bv[nt].w;
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs, acc[mt][nt], 0, 0, 0);
                }
            }
        if (ch + 1 < a.nchunk) park(buf ^ 1);
        __syncthreads();
    }

    // C/D layout of the 16x16 MFMA: column = lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = n0 + 16 * nt + lr;
        if (n >= a.Cout) continue;
        const float2 ss = a.ss[n];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wave * 32 + 16 * mt + 4 * kq + r;
                if (m >= a.M) continue;
                float v = fmaf(acc[mt][nt][r], ss.x, ss.y);
                if (a.relu) v = fmaxf(v, 0.f);
                a.out[m * a.outCS + a.outOff + n] = v;
            }
    }
}

// One conv unit on the device: what flatconv_pack and the epilogue functions made, uploaded
struct FlatConv {
    DevBuf w, ss;
    int Cin = 0, Cout = 0, CoutPad = 0, BN = 64, C4 = 0, nchunk = 0;
    int kt = 0, kh = 1, kw = 1;   // kt = 0: a 2-D unit
    int upload(const FlatConvPacked& p) {
        Cin = p.Cin; Cout = p.Cout; CoutPad = p.CoutPad; BN = p.BN; C4 = p.C4; nchunk = p.nchunk; kt = p.kt; kh = p.kh; kw = p.kw;
        if (int rc = w.upload(p.w.data(), p.w.size() * 4)) return rc;
        return ss.upload(p.ss.data(), p.ss.size() * 4);
    }
    // One unit of a state_dict: the weight [cout][cin][kt kh kw] under `wkey` (kt = 0: [cout][cin][kh][kw]) and its epilogue -- the
    // eval-mode BatchNorm under <bn>.weight / .bias / .running_mean / .running_var with `eps` when `bn` is given, else the bias
    // under `bias` when that is given, else the identity -- packed and uploaded
    int load(const StateDict& sd, const std::string& wkey, int cin, int cout, int kt_, int kh_, int kw_, const std::string& bn, double eps,
             const std::string& bias = "") {
        const float* wsrc = sd.f32(wkey, (int64_t)cout * cin * (kt_ > 0 ? kt_ : 1) * kh_ * kw_);
        if (!wsrc) return I2V_E_MISSING;
        FlatConvPacked p = flatconv_pack(wsrc, cin, cout, kt_, kh_, kw_);
        if (!bn.empty()) {
            const float* g = sd.f32(bn + ".weight", cout);
            const float* b = sd.f32(bn + ".bias", cout);
            const float* m = sd.f32(bn + ".running_mean", cout);
            const float* v = sd.f32(bn + ".running_var", cout);
            if (!g || !b || !m || !v) return I2V_E_MISSING;
            flatconv_fold_bn(p, g, b, m, v, eps);
        } else if (!bias.empty()) {
            const float* b = sd.f32(bias, cout);
            if (!b) return I2V_E_MISSING;
            flatconv_bias(p, b);
        }
        return upload(p);
    }
};

// input and output map of one launch with the stride and the padding in FRONT per dimension; a 2-D unit: Ti = To = 1, sT = 1, pT = 0
struct FlatConvMaps { int B, Ti, Hi, Wi, To, Ho, Wo, sT, sH, sW, pT, pH, pW; };

// TIME = whether the unit has a time extent: a network instantiates only its own form of the kernel.  `label` names the network and
// the unit in the error texts
template <bool TIME>
int flat_conv_launch(const char* label, const FlatConv& u, const float* in, int inCS, int inOff, float* out, int outCS, int outOff,
                     const FlatConvMaps& g, bool relu, hipStream_t st) {
    FlatConvArgs a{};
    a.in = in; a.wp = u.w.as<float>(); a.ss = u.ss.as<float2>(); a.out = out;
    a.M = (long)g.B * g.To * g.Ho * g.Wo;
    a.Ti = g.Ti; a.Hi = g.Hi; a.Wi = g.Wi; a.To = g.To; a.Ho = g.Ho; a.Wo = g.Wo;
    a.inCS = inCS; a.inOff = inOff; a.C4 = u.C4; a.G = (u.kt > 0 ? u.kt : 1) * u.kh * u.kw * u.C4; a.nchunk = u.nchunk;
    a.KH = u.kh; a.KW = u.kw; a.sT = g.sT; a.sH = g.sH; a.sW = g.sW; a.pT = g.pT; a.pH = g.pH; a.pW = g.pW;
    a.Cout = u.Cout; a.CoutPad = u.CoutPad; a.outCS = outCS; a.outOff = outOff; a.relu = relu ? 1 : 0;
    I2V_REQUIRE(TIME ? u.kt > 0 : u.kt == 0 && g.Ti == 1 && g.To == 1 && g.sT == 1 && g.pT == 0, I2V_E_INVALID,
                "%s: a %d-D unit launched as a %d-D one", label, u.kt > 0 ? 3 : 2, TIME ? 3 : 2);
    I2V_REQUIRE(inCS % 4 == 0 && inOff % 4 == 0 && inOff >= 0 && inOff + 4 * u.C4 <= inCS && outOff >= 0 && outOff + u.Cout <= outCS, I2V_E_INVALID,
                "%s: channel slice [%d, +%d) of %d -> [%d, +%d) of %d", label, inOff, 4 * u.C4, inCS, outOff, u.Cout, outCS);
    const long nblk = (a.M + FLATCONV_BM - 1) / FLATCONV_BM * (u.CoutPad / u.BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "%s: grid of %ld workgroups", label, nblk);
    if (u.BN == 128) hipLaunchKernelGGL((flat_conv_kernel<8, TIME>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    else if (u.BN == 64) hipLaunchKernelGGL((flat_conv_kernel<4, TIME>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((flat_conv_kernel<2, TIME>), dim3((unsigned)nblk), dim3(256), 0, st, a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // namespace
}  // namespace i2v
