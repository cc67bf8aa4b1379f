// The exact-fp32 training convolution of stage 1, once: the patch discriminator (i2v_patchdisc.hip) and the 3-D ResNet trunk
// (i2v_res3d_trunk.h: temporal discriminator, motion encoder, GeneratorBlock) run these kernels.  v_mfma_f32_16x16x4_f32; every sum has
// one owner and a fixed order.  Included into the anonymous namespace of its users, as i2v_power_iter.h is.
//   * Activations are channels-last [N][T][H][W][C]; a 3-channel input is stored with 4 channels (r, g, b, 0) by tc_input4_kernel.
//   * tc_pack_kernel writes W (/ sigma) of every conv of a network in one launch into the two operand layouts: wf [tap][cout][cin]
//     (forward: K over (tap, channel)) and wd [tap][cin][cout] (input gradient: K over (tap, output channel)).
//   * conv forward: a flat implicit GEMM, 128 or 64 positions x BN channels per workgroup, chunks of 16 K elements double-buffered in LDS.
//   * dgrad: the same GEMM as a gather over input pixels.  A pixel receives only the taps of its parity under the strides, so the pixels
//     are processed in parity classes (blockIdx.y), each with its own taps in the order (jt, jh, jw).
//   * wgrad: per tap a [cout] x [cin] GEMM over the positions, operands straight from global memory.  The position range is cut into
//     slices (wgrad_plan, a pure function of the shape); the four waves of a workgroup take a quarter of a slice each and are summed in
//     LDS in wave order; tc_finish_a adds the slices' partial sums in slice order and forms the blocks of <dWn, W>; tc_finish_dot adds
//     those in block order, once; tc_finish_b applies the spectral-norm projection and writes or accumulates.
// What differs between the two families is chosen at compile time by a family type F, so nothing inside a K loop is read at run time:
// the window (F::Win: tap decoding, strides, the time axis), the gate on the upstream gradient (F::LRELU), the conv epilogue (F::ACTNORM)
// and whether the dgrad store adds (F::ADD).  A 2-D conv is its own window, NOT a 3-D one with T = 1 (the rule of i2v_flatconv.h).  The
// launchers refuse a conv that is not of the family's window and an operand that the family does not read.
// The per-position conditions of the main loops are single expressions in a tried order: how they are written decides whether the
// compiler keeps the loop's branch-free form and the register budget (profiles/train_conv_bits.md).
#pragma once
#include "i2v_handle.h"
#include "i2v_power_iter.h"

namespace i2v {
namespace {

constexpr int TC_MAXCONV = 21;   // convs per pack launch (the trunk: stem + 4 layers x (2 + 1 + 2))
constexpr int TC_LS = 20;        // floats per staged row of 16

struct TcConv { int cin, cinp, cind, cout, kt, kh, kw, st, ss, sn; };   // cinp: channels of the stored input map; cind: columns of the dgrad GEMM
struct TcGeo { int ti, hi, wi, to, ho, wo; long mi, mo; };
int ntap_of(const TcConv& c) { return c.kt * c.kh * c.kw; }

__device__ __forceinline__ float lrelu_slope(float a) { return a > 0.f ? 1.f : 0.2f; }

// ------------------------------------------------------------------------------------------------------------------ the two windows
struct TcTap { int t, h, w; };
// 3 x kh x kw, pad (1, kh / 2, kw / 2), strides (st, ss, ss).  split: tap of an nh x nw plane stack -> (jt, jh, jw), jw fastest.
struct Win3 {
    int h, w, t, s;
    static constexpr bool TIME = true, WHOLE_CHUNKS = false;   // the stem's 147 taps of 4 channels end inside a chunk
    static Win3 of(const TcConv& c) { return Win3{c.kh, c.kw, c.st, c.ss}; }
    static bool fits(const TcConv& c) { return c.kt == 3; }
    __device__ int kh() const { return h; }
    __device__ int kw() const { return w; }
    __device__ int ph() const { return h >> 1; }
    __device__ int pw() const { return w >> 1; }
    __device__ int st() const { return t; }
    __device__ int ss() const { return s; }
    __device__ int div_t(int x) const { return x / t; }
    __device__ int div_s(int x) const { return x / s; }
    __device__ int mod_t(int x) const { return x % t; }
    __device__ int mod_s(int x) const { return x % s; }
    __device__ int mul_t(int x) const { return x * t; }
    __device__ int mul_s(int x) const { return x * s; }
    __device__ static int ntap(int of_the_conv) { return of_the_conv; }
    __device__ TcTap split(int tap, int nh, int nw) const {
        const int jt = tap / (nh * nw), r = tap - jt * nh * nw, jh = r / nw;
        return TcTap{jt, jh, r - jh * nw};
    }
};

// 4 x 4, pad 1, stride 1 or 2, no time axis.  split: nh = nw = 4, or 2 inside a parity class of stride 2.
struct Win2 {
    int s;
    static constexpr bool TIME = false, WHOLE_CHUNKS = true;
    static Win2 of(const TcConv& c) { return Win2{c.ss}; }
    static bool fits(const TcConv& c) { return c.kt == 1 && c.kh == 4 && c.kw == 4 && c.st == 1 && (c.ss == 1 || c.ss == 2); }
    __device__ int kh() const { return 4; }
    __device__ int kw() const { return 4; }
    __device__ int ph() const { return 1; }
    __device__ int pw() const { return 1; }
    __device__ int st() const { return 1; }
    __device__ int ss() const { return s; }
    __device__ int div_t(int x) const { return x; }
    __device__ int div_s(int x) const { return s == 2 ? x >> 1 : x; }
    __device__ int mod_t(int) const { return 0; }
    __device__ int mod_s(int x) const { return s == 2 ? x & 1 : 0; }
    __device__ int mul_t(int x) const { return x; }
    __device__ int mul_s(int x) const { return s == 2 ? x << 1 : x; }
    __device__ static int ntap(int) { return 16; }
    __device__ TcTap split(int tap, int, int nw) const { return TcTap{0, tap >> (nw == 4 ? 2 : 1), tap & (nw - 1)}; }
};

// ACTNORM: the conv epilogue bias -> [pre] -> ActNorm -> LeakyReLU instead of the plain store.  LRELU: the upstream gradient of dgrad and
// wgrad passes the LeakyReLU slope and ActNorm's scale instead of a ReLU mask.  ADD: the dgrad store takes add / add_mask.
struct Trunk3d {
    using Win = Win3;
    static constexpr bool ACTNORM = false, LRELU = false, ADD = true;
    static constexpr const char* NAME = "temporal discriminator";
};
struct Patch2d {
    using Win = Win2;
    static constexpr bool ACTNORM = true, LRELU = true, ADD = false;
    static constexpr const char* NAME = "patch discriminator";
};

template <class F>
__device__ __forceinline__ float gate(float g, float act) {
    if constexpr (F::LRELU) return g * lrelu_slope(act);
    else return act > 0.f ? g : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ input stage
__global__ __launch_bounds__(256) void tc_input4_kernel(const float* __restrict__ x, float* __restrict__ out, long npix, long thw) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < npix; i += gridDim.x * 256L) {
        const long n = i / thw, p = i - n * thw;
        const float* s = x + n * 3 * thw + p;
        *reinterpret_cast<float4*>(out + 4 * i) = make_float4(s[0], s[thw], s[2 * thw], 0.f);
    }
}

// ------------------------------------------------------------------------------------------------------------------ weight packing
struct TcPackConv { const float* w; const float* sigma; float* wf; float* wd; int cout, cin, cinp, cind, ntap; long first; };   // wd may be null
struct TcPackArgs { TcPackConv c[TC_MAXCONV]; int nconv; long total; };

template <class W>   // the tap count is the window's where it is fixed
__global__ __launch_bounds__(256) void tc_pack_kernel(TcPackArgs a) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < a.total; e += gridDim.x * 256L) {
        int ci = 0;
        while (ci + 1 < a.nconv && e >= a.c[ci + 1].first) ++ci;
        const TcPackConv& c = a.c[ci];
        const int ntap = W::ntap(c.ntap);
        long r = e - c.first;                       // ((co * cind) + cip) * ntap + tap
        const int tap = (int)(r % ntap); r /= ntap;
        const int cip = (int)(r % c.cind), co = (int)(r / c.cind);
        float val = 0.f;
        if (cip < c.cin) {
            val = c.w[((long)co * c.cin + cip) * ntap + tap];
            if (c.sigma) val = val / *c.sigma;
        }
        if (cip < c.cinp) c.wf[((long)tap * c.cout + co) * c.cinp + cip] = val;
        if (c.wd) c.wd[((long)tap * c.cind + cip) * c.cout + co] = val;
    }
}

// ------------------------------------------------------------------------------------------------------------------ conv forward
// What the ACTNORM epilogue reads; the plain store carries none of it, so the trunk's kernel arguments are the conv's alone
template <bool ACTNORM>
struct TcEpilogueArgs {
    const float *bias, *loc, *scale;   // loc / scale null: no ActNorm
    float* pre;                        // [M][cout] or null
    int lrelu;
};
template <>
struct TcEpilogueArgs<false> {};

template <class F>
struct TcConvArgs : TcEpilogueArgs<F::ACTNORM> {
    const float* in;     // [N][Ti][Hi][Wi][cinp]
    const float* wf;     // [ntap][cout][cinp]
    float* out;          // [M][cout]; ACTNORM: may be null
    long M;
    int Ti, Hi, Wi, To, Ho, Wo, cinp, C4, nchunk, ntap;
    typename F::Win win;
    int cout;
};

template <class F, int NT, int MR>   // BN = 16 NT columns, BM = 64 MR rows per workgroup
__global__ __launch_bounds__(256) void tc_conv_kernel(TcConvArgs<F> a) {
    using W = typename F::Win;
    constexpr int BN = 16 * NT, BM = 64 * MR;
    __shared__ __attribute__((aligned(16))) float a_lds[2][BM * TC_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * TC_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4, q = tid & 3;
    const int nNt = a.cout / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * BM;
    const W& win = a.win;

    int rb[MR], rt[MR], rh[MR], rw[MR];
#pragma unroll
    for (int u = 0; u < MR; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < a.M;
        if (!ok) m = 0;
        const int wo = (int)(m % a.Wo); m /= a.Wo;
        const int ho = (int)(m % a.Ho); m /= a.Ho;
        const int to = W::TIME ? (int)(m % a.To) : 0;
        if constexpr (W::TIME) m /= a.To;
        rb[u] = ok ? (int)m : -1;
        rt[u] = W::TIME ? to * win.st() - 1 : 0; rh[u] = ho * win.ss() - win.ph(); rw[u] = wo * win.ss() - win.pw();
    }
    float4 pa0, pa1, pw0;
    pa1 = pw0 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const int tap = g / a.C4, c = (g - tap * a.C4) * 4;
        const bool tok = W::WHOLE_CHUNKS || tap < a.ntap;   // the stem's last chunk
        const TcTap d = win.split(tap, win.kh(), win.kw());
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            const int t = rt[u] + d.t, h = rh[u] + d.h, w = rw[u] + d.w;
            // (one expression, in this order: a flag amended per axis costs the loop its branch-free form -- profiles/train_conv_bits.md)
            const bool ok = tok && rb[u] >= 0 && (!W::TIME || (unsigned)t < (unsigned)a.Ti) && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
            const long row = W::TIME ? (long)rb[u] * a.Ti + t : rb[u];
            const long off = ok ? ((row * a.Hi + h) * a.Wi + w) * a.cinp + c : 0;
            const float4 v = *reinterpret_cast<const float4*>(a.in + off);
            const float4 z = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (u == 0) pa0 = z; else pa1 = z;
        }
        if (tid < BN * 4) {
            const float4 v = *reinterpret_cast<const float4*>(a.wf + (tok ? ((long)tap * a.cout + n0 + (tid >> 2)) * a.cinp + c : 0));
            pw0 = tok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto park = [&](int buf) {
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * TC_LS + 4 * q]) = pa0;
        if constexpr (MR == 2) *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * TC_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * TC_LS + 4 * q]) = pw0;
    };

    f32x4 acc[MR][NT];
#pragma unroll
    for (int mt = 0; mt < MR; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    request(0);
    park(0);
    __syncthreads();
    for (int ch = 0; ch < a.nchunk; ++ch) {
        const int buf = ch & 1;
        request(ch + 1 < a.nchunk ? ch + 1 : ch);
        // MFMA k-slot (lane >> 4) of step s carries K element 4 (lane >> 4) + s of the chunk, for both operands
        float4 av[MR], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MR; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 16 * MR + 16 * mt + lr) * TC_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * TC_LS + 4 * kq]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < MR; ++mt) {
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
        float b = 0.f, lc = 0.f, sc = 1.f;
        if constexpr (F::ACTNORM) {
            b = a.bias[n];
            if (a.loc) { lc = a.loc[n]; sc = a.scale[n]; }
        }
#pragma unroll
        for (int mt = 0; mt < MR; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wave * 16 * MR + 16 * mt + 4 * kq + r;
                if (m >= a.M) continue;
                if constexpr (F::ACTNORM) {
                    float y = acc[mt][nt][r] + b;
                    if (a.pre) a.pre[m * a.cout + n] = y;
                    if (a.loc) y = sc * (y + lc);
                    if (a.lrelu) y = y > 0.f ? y : 0.2f * y;
                    if (a.out) a.out[m * a.cout + n] = y;
                } else {
                    a.out[m * a.cout + n] = acc[mt][nt][r];
                }
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------ input gradient
template <class W>
struct TcDgradArgs {
    const float* g;      // [N][To][Ho][Wo][cout], the gradient at the conv's output (LRELU: at the layer's activation)
    const float* act;    // of g's shape or null: the ReLU mask (g counts where act > 0), or the activation whose LeakyReLU slope g passes
    const float* scale;  // LRELU only: ActNorm's scale [cout] or null
    const float* wd;     // [ntap][cind][cout]
    float* out;          // [N][Ti][Hi][Wi][cin]; frames: [N][3][Ti][Hi][Wi]
    const float *add, *add_mask;   // ADD only: of out's shape or null: out = result + add [add_mask > 0]
    int N, Ti, Hi, Wi, To, Ho, Wo, cout, C4o;
    W win;
    int cin, cind, frames;
};   // (a family's pointers lie together: one not read before the epilogue, loaded apart, costs the main loop its staggered LDS waits)

template <class F, int NT, int MR>
__global__ __launch_bounds__(256) void tc_dgrad_kernel(TcDgradArgs<typename F::Win> a) {
    using W = typename F::Win;
    constexpr int BN = 16 * NT, BM = 64 * MR;
    __shared__ __attribute__((aligned(16))) float a_lds[2][BM * TC_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * TC_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4, q = tid & 3;
    const W& win = a.win;
    const int str_t = win.st(), str_s = win.ss();
    // the parity class of this workgroup: (pt, ph, pw), each 0 where its axis has stride 1
    const int cls = blockIdx.y;
    const int pw_ = win.mod_s(cls), ph_ = win.mod_s(win.div_s(cls)), pt_ = W::TIME ? cls / (str_s * str_s) : 0;
    const int Tc = W::TIME ? win.div_t(a.Ti - pt_ + str_t - 1) : 1, Hc = win.div_s(a.Hi - ph_ + str_s - 1), Wc = win.div_s(a.Wi - pw_ + str_s - 1);
    const long Mc = (long)a.N * Tc * Hc * Wc;
    const int nNt = a.cind / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * BM;
    if (m0 >= Mc) return;
    // taps of the class along an axis of window k, pad p, stride s: k_j = kb + s j with kb = (parity + p) % s
    const int padh = win.ph(), padw = win.pw();
    const int ktb = W::TIME ? win.mod_t(pt_ + 1) : 0, khb = win.mod_s(ph_ + padh), kwb = win.mod_s(pw_ + padw);
    const int ntt = W::TIME ? win.div_t(3 - ktb + str_t - 1) : 1, nth = win.div_s(win.kh() - khb + str_s - 1), ntw = win.div_s(win.kw() - kwb + str_s - 1);
    const int nchunk = ntt * nth * ntw * a.C4o / 4;

    int rb[MR], rt[MR], rh[MR], rw[MR];   // batch row (-1: masked), t + 1, h + pad, w + pad
#pragma unroll
    for (int u = 0; u < MR; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < Mc;
        if (!ok) m = 0;
        const int wc = (int)(m % Wc); m /= Wc;
        const int hc = (int)(m % Hc); m /= Hc;
        const int tc = W::TIME ? (int)(m % Tc) : 0;
        if constexpr (W::TIME) m /= Tc;
        rb[u] = ok ? (int)m : -1;
        rt[u] = W::TIME ? win.mul_t(tc) + pt_ + 1 : 0; rh[u] = win.mul_s(hc) + ph_ + padh; rw[u] = win.mul_s(wc) + pw_ + padw;
    }
    float4 pa0, pa1, pw0;
    pa1 = pw0 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const int tj = g / a.C4o, c = (g - tj * a.C4o) * 4;
        const TcTap j = win.split(tj, nth, ntw);
        const int kt = W::TIME ? ktb + win.mul_t(j.t) : 0, kh = khb + win.mul_s(j.h), kw = kwb + win.mul_s(j.w);
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            const int dt = rt[u] - kt, dh = rh[u] - kh, dw = rw[u] - kw;   // multiples of the strides by the choice of the taps
            const int to = win.div_t(dt), ho = win.div_s(dh), wo = win.div_s(dw);
            // (one expression, in this order: the row test in front or behind costs an instantiation 4 VGPRs -- profiles/train_conv_bits.md)
            const bool ok = dt >= 0 && dh >= 0 && dw >= 0 && rb[u] >= 0 && to < (W::TIME ? a.To : 1) && ho < a.Ho && wo < a.Wo;
            const long row = W::TIME ? (long)rb[u] * a.To + to : rb[u];
            const long off = ok ? ((row * a.Ho + ho) * a.Wo + wo) * a.cout + c : 0;
            float4 v = *reinterpret_cast<const float4*>(a.g + off);
            if (a.act) {
                const float4 y = *reinterpret_cast<const float4*>(a.act + off);
                v.x = gate<F>(v.x, y.x); v.y = gate<F>(v.y, y.y); v.z = gate<F>(v.z, y.z); v.w = gate<F>(v.w, y.w);
            }
            if constexpr (F::LRELU) {
                if (a.scale) {
                    const float4 sc = *reinterpret_cast<const float4*>(a.scale + c);
                    v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
                }
            }
            const float4 z = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (u == 0) pa0 = z; else pa1 = z;
        }
        if (tid < BN * 4) pw0 = *reinterpret_cast<const float4*>(a.wd + ((long)((kt * win.kh() + kh) * win.kw() + kw) * a.cind + n0 + (tid >> 2)) * a.cout + c);
    };
    auto park = [&](int buf) {
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * TC_LS + 4 * q]) = pa0;
        if constexpr (MR == 2) *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * TC_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * TC_LS + 4 * q]) = pw0;
    };

    f32x4 acc[MR][NT];
#pragma unroll
    for (int mt = 0; mt < MR; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    request(0);
    park(0);
    __syncthreads();
    for (int ch = 0; ch < nchunk; ++ch) {
        const int buf = ch & 1;
        request(ch + 1 < nchunk ? ch + 1 : ch);
        float4 av[MR], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MR; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 16 * MR + 16 * mt + lr) * TC_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * TC_LS + 4 * kq]);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int mt = 0; mt < MR; ++mt) {
                const float as = s == 0 ? av[mt].x : s == 1 ? av[mt].y : s == 2 ? av[mt].z : av[mt].w;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const float bs = s == 0 ? bv[nt].x : s == 1 ? bv[nt].y : s == 2 ? bv[nt].z : bv[nt].w;
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs, acc[mt][nt], 0, 0, 0);
                }
            }
        if (ch + 1 < nchunk) park(buf ^ 1);
        __syncthreads();
    }

#pragma unroll
    for (int mt = 0; mt < MR; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            long m = m0 + wave * 16 * MR + 16 * mt + 4 * kq + r;
            if (m >= Mc) continue;
            const int wc = (int)(m % Wc); m /= Wc;
            const int hc = (int)(m % Hc); m /= Hc;
            const int tc = W::TIME ? (int)(m % Tc) : 0;
            if constexpr (W::TIME) m /= Tc;
            const int t = win.mul_t(tc) + pt_, h = win.mul_s(hc) + ph_, w = win.mul_s(wc) + pw_;
            const int planes = W::TIME ? a.Ti : 1;   // of one sample and channel
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = n0 + 16 * nt + lr;
                if (a.frames) {
                    if (n < 3) a.out[(((m * 3 + n) * planes + t) * a.Hi + h) * a.Wi + w] = acc[mt][nt][r];
                } else if (n < a.cin) {
                    const long o = (((m * planes + t) * a.Hi + h) * a.Wi + w) * a.cin + n;
                    float v = acc[mt][nt][r];
                    if constexpr (F::ADD) {
                        if (a.add) v += a.add_mask ? (a.add_mask[o] > 0.f ? a.add[o] : 0.f) : a.add[o];
                    }
                    a.out[o] = v;
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
template <class W>
struct TcWgradArgs {
    const float *g, *act, *scale;   // as TcDgradArgs
    const float* x;                 // the conv's input [N][Ti][Hi][Wi][cinp]
    float* part;                    // [slices][ntap][cout][CP]
    long P;                         // positions N To Ho Wo
    int Ti, Hi, Wi, To, Ho, Wo, cinp, cout, CP, slice_len;
    W win;
};

template <class F, int MT, int NT>
__global__ __launch_bounds__(256) void tc_wgrad_kernel(TcWgradArgs<typename F::Win> a) {
    using W = typename F::Win;
    __shared__ float red[3][MT * NT * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const W& win = a.win;
    const int nCi = a.CP / (16 * NT);
    const int co0 = (int)(blockIdx.x / nCi) * 16 * MT, ci0 = (int)(blockIdx.x % nCi) * 16 * NT;
    const int tap = blockIdx.y;
    const TcTap k = win.split(tap, win.kh(), win.kw());
    const int kt = k.t, kh = k.h, kw = k.w;
    const int sl = blockIdx.z, quarter = a.slice_len / 4;
    const long begin = (long)sl * a.slice_len + (long)wave * quarter;
    const long end = begin + quarter < a.P ? begin + quarter : a.P;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // A[i = co][k = position], B[k = position][j = ci]: k-slot (lane >> 4) of a step is position mb + (lane >> 4)
    for (long mb = begin; mb < end; mb += 4) {
        long m = mb + kq;
        const bool ok = m < end;
        if (!ok) m = 0;
        const long mrow = m;
        const int wo = (int)(m % a.Wo); m /= a.Wo;
        const int ho = (int)(m % a.Ho); m /= a.Ho;
        const int h = ho * win.ss() - win.ph() + kh, w = wo * win.ss() - win.pw() + kw;
        bool xok = ok && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
        if constexpr (W::TIME) {
            const int to = (int)(m % a.To); m /= a.To;
            const int t = to * win.st() - 1 + kt;
            xok = xok && (unsigned)t < (unsigned)a.Ti;
            m = m * a.Ti + t;
        }
        const long pix = xok ? (m * a.Hi + h) * a.Wi + w : 0;
        float av[MT], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int co = co0 + 16 * mt + lr;
            float v = a.g[mrow * a.cout + co];
            if (a.act) v = gate<F>(v, a.act[mrow * a.cout + co]);
            if constexpr (F::LRELU) {
                if (a.scale) v *= a.scale[co];
            }
            av[mt] = ok ? v : 0.f;
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int ci = ci0 + 16 * nt + lr;
            const bool cok = xok && ci < a.cinp;
            const float v = a.x[cok ? pix * a.cinp + ci : 0];
            bv[nt] = cok ? v : 0.f;
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
    }

    // the four waves' sums in wave order
    if (wave > 0) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave - 1][((mt * NT + nt) * 4 + r) * 64 + lane] = acc[mt][nt][r];
    }
    __syncthreads();
    if (wave > 0) return;
    float* dst = a.part + ((long)sl * gridDim.y + tap) * a.cout * a.CP;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[mt][nt][r];
                for (int w = 0; w < 3; ++w) v += red[w][((mt * NT + nt) * 4 + r) * 64 + lane];
                dst[(long)(co0 + 16 * mt + 4 * kq + r) * a.CP + ci0 + 16 * nt + lr] = v;
            }
}

struct TcFinishArgs {
    const float* part;   // [S][ntap][cout][CP]
    const float* w;      // weight_orig [cout][cin][ntap]
    const float *u, *v, *sigma;   // this forward's values; sigma null: no projection
    float* dwn;          // [cout][cin][ntap]
    double* dotp;        // [nblk]: the workgroups' sums of dWn * W; tc_finish_dot leaves their total in dotp[0]
    float* grad;
    long E;
    int S, cout, cin, CP, ntap, nblk, accumulate;
};

// dWn = the slices' partial sums in slice order; per workgroup sum of dWn * W in float64
__global__ __launch_bounds__(256) void tc_finish_a_kernel(TcFinishArgs a) {
    __shared__ double red[256];
    const long e = blockIdx.x * 256L + threadIdx.x;
    double d = 0.0;
    if (e < a.E) {
        const int K = a.cin * a.ntap;
        const int co = (int)(e / K), k = (int)(e % K), ci = k / a.ntap, tap = k - ci * a.ntap;
        float sum = 0.f;
        for (int s = 0; s < a.S; ++s) sum += a.part[(((long)s * a.ntap + tap) * a.cout + co) * a.CP + ci];
        a.dwn[e] = sum;
        d = (double)sum * (double)a.w[e];
    }
    d = block_sum(d, red);
    if (threadIdx.x == 0) a.dotp[blockIdx.x] = d;
}

// <dWn, W> = the workgroups' sums in block order, once for the whole tensor (one workgroup).  Every sum has been read before block_sum's
// first barrier, so the total can take the place of dotp[0]
__global__ __launch_bounds__(256) void tc_finish_dot_kernel(TcFinishArgs a) {
    __shared__ double red[256];
    double d = 0.0;
    for (int i = threadIdx.x; i < a.nblk; i += 256) d += a.dotp[i];
    d = block_sum(d, red);
    if (threadIdx.x == 0) a.dotp[0] = d;
}

// dW_orig = (dWn - <dWn, W / sigma> u v^T) / sigma, written or accumulated
__global__ __launch_bounds__(256) void tc_finish_b_kernel(TcFinishArgs a) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= a.E) return;
    float gv = a.dwn[e];
    if (a.sigma) {
        const float sg = *a.sigma;
        const float proj = (float)(a.dotp[0] / (double)sg);
        const int K = a.cin * a.ntap;
        gv = (gv - proj * a.u[e / K] * a.v[e % K]) / sg;
    }
    a.grad[e] = a.accumulate ? a.grad[e] + gv : gv;
}

// =================================================================================================================== host side
int bn_of(int c) { return c % 64 == 0 ? 64 : c % 32 == 0 ? 32 : 16; }
// rows per workgroup of the two GEMM kernels: 128, or 64 where 128 would leave the device's compute units without two workgroups each
// (a function of the shape alone: the same shape always runs the same kernel)
int rows_of(long rows, int column_tiles) { return (rows + 127) / 128 * column_tiles >= 512 ? 128 : 64; }

size_t pack_elems(const TcConv& c) { return (size_t)c.cout * c.cind * ntap_of(c); }

// P positions in at most S slices of a multiple of 16 positions
void cut_slices(long P, long S, int* slices, int* slice_len) {
    const long L = (long)align_up((size_t)((P + S - 1) / S), 16);
    *slice_len = (int)L;
    *slices = (int)((P + L - 1) / L);
}
// the slice plan of the weight gradient: enough workgroups to fill the device, slices of at least 64 positions
void wgrad_plan(int cout, int cin, int ntap, long P, int* slices, int* slice_len) {
    const int CP = (int)align_up(cin == 3 ? 4 : cin, 16);
    const long tiles = (long)ntap * (cout / bn_of(cout)) * (CP / bn_of(CP));
    cut_slices(P, std::min<long>(std::max<long>((1024 + tiles - 1) / tiles, 1), std::max<long>((P + 63) / 64, 1)), slices, slice_len);
}
size_t wgrad_part_floats(const TcConv& c, long P) {
    int S, L;
    wgrad_plan(c.cout, c.cin, ntap_of(c), P, &S, &L);
    return (size_t)S * ntap_of(c) * c.cout * align_up(c.cinp, 16);
}
size_t finish_blocks(const TcConv& c) { return ((size_t)c.cout * c.cin * ntap_of(c) + 255) / 256; }

template <class F>
int launch_pack(const TcPackArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((tc_pack_kernel<typename F::Win>), dim3(grid_for(a.total)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

// ACTNORM only: what the conv epilogue adds to the plain store
struct TcEpilogue { const float *bias = nullptr, *loc = nullptr, *scale = nullptr; float* pre = nullptr; bool lrelu = false; };

template <class F>
int launch_conv(const TcConv& c, const float* in, const float* wf, float* out, const TcGeo& mp, hipStream_t st, const TcEpilogue& e = {}) {
    I2V_REQUIRE(F::Win::fits(c) && F::ACTNORM == (e.bias != nullptr), I2V_E_INVALID, "%s: a conv outside this family's window, or its epilogue", F::NAME);
    TcConvArgs<F> a{};
    a.in = in; a.wf = wf; a.out = out;
    if constexpr (F::ACTNORM) { a.bias = e.bias; a.loc = e.loc; a.scale = e.scale; a.pre = e.pre; a.lrelu = e.lrelu ? 1 : 0; }
    a.M = mp.mo; a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo;
    a.cinp = c.cinp; a.C4 = c.cinp / 4; a.ntap = ntap_of(c); a.nchunk = (a.ntap * a.C4 + 3) / 4; a.cout = c.cout; a.win = F::Win::of(c);
    const int BN = bn_of(c.cout);
    const int BM = rows_of(a.M, c.cout / BN);
    const long nblk = (a.M + BM - 1) / BM * (c.cout / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "%s: conv grid of %ld workgroups", F::NAME, nblk);
    const dim3 grid((unsigned)nblk);
    if (BM == 128) {
        if (BN == 64) hipLaunchKernelGGL((tc_conv_kernel<F, 4, 2>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((tc_conv_kernel<F, 2, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tc_conv_kernel<F, 1, 2>), grid, dim3(256), 0, st, a);
    } else {
        if (BN == 64) hipLaunchKernelGGL((tc_conv_kernel<F, 4, 1>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((tc_conv_kernel<F, 2, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tc_conv_kernel<F, 1, 1>), grid, dim3(256), 0, st, a);
    }
    I2V_LAUNCHED();
    return I2V_OK;
}

// act: the ReLU mask, or (LRELU) the activation whose LeakyReLU slope g passes; scale: LRELU only, ActNorm's scale
template <class F>
int launch_dgrad(const TcConv& c, const float* g, const float* act, const float* scale, const float* wd, const float* add, const float* add_mask,
                 float* out, bool frames, int N, const TcGeo& mp, hipStream_t st) {
    I2V_REQUIRE(F::Win::fits(c) && (F::ADD || (!add && !add_mask)) && (F::LRELU || !scale), I2V_E_INVALID,
                "%s: a conv outside this family's window, or an add or a scale that its dgrad does not take", F::NAME);
    TcDgradArgs<typename F::Win> a{};
    a.g = g; a.act = act; a.scale = scale; a.wd = wd; a.add = add; a.add_mask = add_mask; a.out = out;
    a.N = N; a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo;
    a.cout = c.cout; a.C4o = c.cout / 4; a.win = F::Win::of(c);
    a.cin = c.cin == 3 && !frames ? 4 : c.cin; a.cind = c.cind; a.frames = frames ? 1 : 0;
    const int BN = bn_of(c.cind);
    const int classes = c.st * c.ss * c.ss;
    const long mc = (long)N * ((mp.ti + c.st - 1) / c.st) * ((mp.hi + c.ss - 1) / c.ss) * ((mp.wi + c.ss - 1) / c.ss);   // the largest parity class
    const int BM = rows_of(mc * classes, c.cind / BN);
    const long nblk = (mc + BM - 1) / BM * (c.cind / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "%s: dgrad grid of %ld workgroups", F::NAME, nblk);
    const dim3 grid((unsigned)nblk, classes);
    if (BM == 128) {
        if (BN == 64) hipLaunchKernelGGL((tc_dgrad_kernel<F, 4, 2>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((tc_dgrad_kernel<F, 2, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tc_dgrad_kernel<F, 1, 2>), grid, dim3(256), 0, st, a);
    } else {
        if (BN == 64) hipLaunchKernelGGL((tc_dgrad_kernel<F, 4, 1>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((tc_dgrad_kernel<F, 2, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((tc_dgrad_kernel<F, 1, 1>), grid, dim3(256), 0, st, a);
    }
    I2V_LAUNCHED();
    return I2V_OK;
}

// partial sums [S][ntap][cout][CP] -> dwn -> grad (written or accumulated); with sigma, through the spectral-norm projection
int launch_finish(const float* part, int S, int CP, int cout, int cin, int ntap, const float* w, const float* u, const float* v, const float* sigma,
                  float* dwn, double* dotp, float* grad, bool accumulate, hipStream_t st) {
    TcFinishArgs f{};
    f.part = part; f.w = w; f.u = u; f.v = v; f.sigma = sigma; f.dwn = dwn; f.dotp = dotp; f.grad = grad;
    f.E = (long)cout * cin * ntap; f.S = S; f.cout = cout; f.cin = cin; f.CP = CP; f.ntap = ntap; f.nblk = (int)((f.E + 255) / 256);
    f.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(tc_finish_a_kernel, dim3(f.nblk), dim3(256), 0, st, f);
    I2V_LAUNCHED();
    if (sigma) {
        hipLaunchKernelGGL(tc_finish_dot_kernel, dim3(1), dim3(256), 0, st, f);
        I2V_LAUNCHED();
    }
    hipLaunchKernelGGL(tc_finish_b_kernel, dim3(f.nblk), dim3(256), 0, st, f);
    I2V_LAUNCHED();
    return I2V_OK;
}

template <class F, int MT>
void launch_wgrad_nt(int nt, dim3 grid, hipStream_t st, const TcWgradArgs<typename F::Win>& a) {
    if (nt == 4) hipLaunchKernelGGL((tc_wgrad_kernel<F, MT, 4>), grid, dim3(256), 0, st, a);
    else if (nt == 2) hipLaunchKernelGGL((tc_wgrad_kernel<F, MT, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((tc_wgrad_kernel<F, MT, 1>), grid, dim3(256), 0, st, a);
}

// g gated as in the dgrad
template <class F>
int launch_wgrad(const TcConv& c, const float* g, const float* act, const float* scale, const float* x, const float* w, const float* u, const float* v,
                 const float* sigma, float* part, float* dwn, double* dotp, float* grad, bool accumulate, const TcGeo& mp, hipStream_t st) {
    I2V_REQUIRE(F::Win::fits(c) && (F::LRELU || !scale), I2V_E_INVALID, "%s: a conv outside this family's window, or a scale that its wgrad does not take",
                F::NAME);
    int S, L;
    const int ntap = ntap_of(c);
    wgrad_plan(c.cout, c.cin, ntap, mp.mo, &S, &L);
    TcWgradArgs<typename F::Win> a{};
    a.g = g; a.act = act; a.scale = scale; a.x = x; a.part = part; a.P = mp.mo;
    a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo; a.cinp = c.cinp; a.cout = c.cout; a.CP = (int)align_up(c.cinp, 16);
    a.slice_len = L; a.win = F::Win::of(c);
    const int mt = bn_of(c.cout) / 16, nt = bn_of(a.CP) / 16;
    const dim3 grid((unsigned)((c.cout / (16 * mt)) * (a.CP / (16 * nt))), ntap, (unsigned)S);
    if (mt == 4) launch_wgrad_nt<F, 4>(nt, grid, st, a);
    else if (mt == 2) launch_wgrad_nt<F, 2>(nt, grid, st, a);
    else launch_wgrad_nt<F, 1>(nt, grid, st, a);
    I2V_LAUNCHED();
    return launch_finish(part, S, a.CP, c.cout, c.cin, ntap, w, u, v, sigma, dwn, dotp, grad, accumulate, st);
}

}  // namespace
}  // namespace i2v
