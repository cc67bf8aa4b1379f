// The 3-D ResNet-18 trunk with GroupNorm(16) that the temporal discriminator (i2v_disc3d.hip) and the motion encoder's training path
// (i2v_encoder_train.hip) share: the conv, input-gradient, weight-gradient, finish, GroupNorm and pool kernels, their launchers and the
// plan helpers, moved here unchanged from i2v_disc3d.hip (whose head comment describes them).  The host side of the trunk as a whole --
// plan, binding, layout and the two walks -- is i2v_res3d_net.h.  Included into the anonymous namespace of its users, as
// i2v_power_iter.h is.
#pragma once
#include "i2v_handle.h"
#include "i2v_power_iter.h"

namespace i2v {
namespace {

constexpr int D3_MAXCONV = 21;   // stem + 4 layers x (2 + 1 + 2)
constexpr int D3_LS = 20;        // floats per staged row of 16
constexpr int D3_GROUPS = 16;
constexpr int D3_GN_SLICES = 32;

struct D3Conv { int cin, cinp, cind, cout, kh, kw, st, ss, sn; };   // cinp: channels of the stored input map; cind: columns of the dgrad GEMM
struct D3Geo { int ti, hi, wi, to, ho, wo; long mi, mo; };

// ------------------------------------------------------------------------------------------------------------------ small kernels
__global__ __launch_bounds__(256) void d3_input4_kernel(const float* __restrict__ x, float* __restrict__ out, long npix, long thw) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < npix; i += gridDim.x * 256L) {
        const long n = i / thw, p = i - n * thw;
        const float* s = x + n * 3 * thw + p;
        *reinterpret_cast<float4*>(out + 4 * i) = make_float4(s[0], s[thw], s[2 * thw], 0.f);
    }
}

__global__ __launch_bounds__(256) void d3_add_kernel(float* __restrict__ dst, const float* __restrict__ src, long total) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) dst[i] += src[i];
}

// ------------------------------------------------------------------------------------------------------------------ max pool
// MaxPool3d(3, stride (1, 2, 2), pad 1); the first maximum in (t, h, w) scan order wins
__global__ __launch_bounds__(256) void d3_maxpool_kernel(const float* __restrict__ x, float* __restrict__ out, int* __restrict__ arg, long total, int T,
                                                         int H, int W, int Ho, int Wo, int C) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % C);
        long p = i / C;
        const int wo = (int)(p % Wo); p /= Wo;
        const int ho = (int)(p % Ho); p /= Ho;
        const int to = (int)(p % T); p /= T;
        float best = 0.f;
        int bi = -1;
        for (int dt = -1; dt <= 1; ++dt) {
            const int t = to + dt;
            if ((unsigned)t >= (unsigned)T) continue;
            for (int dh = -1; dh <= 1; ++dh) {
                const int h = 2 * ho + dh;
                if ((unsigned)h >= (unsigned)H) continue;
                for (int dw = -1; dw <= 1; ++dw) {
                    const int w = 2 * wo + dw;
                    if ((unsigned)w >= (unsigned)W) continue;
                    const int idx = (t * H + h) * W + w;
                    const float v = x[(p * (long)T * H * W + idx) * C + c];
                    if (bi < 0 || v > best) { best = v; bi = idx; }
                }
            }
        }
        out[i] = best;
        arg[i] = bi;
    }
}

// a gather: the windows overlap, so an input sums the gradients of the windows that chose it, in the windows' scan order
__global__ __launch_bounds__(256) void d3_maxpool_bwd_kernel(const float* __restrict__ g, const int* __restrict__ arg, float* __restrict__ dx, long total,
                                                             int T, int H, int W, int Ho, int Wo, int C) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % C);
        long p = i / C;
        const int w = (int)(p % W); p /= W;
        const int h = (int)(p % H); p /= H;
        const int t = (int)(p % T); p /= T;
        const int idx = (t * H + h) * W + w;
        const int ho0 = h / 2, ho1 = (h + 1) / 2, wo0 = w / 2, wo1 = (w + 1) / 2;   // 2 o - 1 <= i <= 2 o + 1
        float acc = 0.f;
        for (int to = t - 1; to <= t + 1; ++to) {
            if ((unsigned)to >= (unsigned)T) continue;
            for (int ho = ho0; ho <= ho1 && ho < Ho; ++ho)
                for (int wo = wo0; wo <= wo1 && wo < Wo; ++wo) {
                    const long o = (((p * T + to) * Ho + ho) * Wo + wo) * C + c;
                    if (arg[o] == idx) acc += g[o];
                }
        }
        dx[i] = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------------ weight packing
// W (/ sigma) into the two operand layouts
struct D3PackConv { const float* w; const float* sigma; float* wf; float* wd; int cout, cin, cinp, cind, ntap; long first; };
struct D3PackArgs { D3PackConv c[D3_MAXCONV]; int nconv; long total; };

__global__ __launch_bounds__(256) void d3_pack_kernel(D3PackArgs a) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < a.total; e += gridDim.x * 256L) {
        int ci = 0;
        while (ci + 1 < a.nconv && e >= a.c[ci + 1].first) ++ci;
        const D3PackConv& c = a.c[ci];
        long r = e - c.first;                       // ((co * cind) + cip) * ntap + tap
        const int tap = (int)(r % c.ntap); r /= c.ntap;
        const int cip = (int)(r % c.cind), co = (int)(r / c.cind);
        float val = 0.f;
        if (cip < c.cin) {
            val = c.w[((long)co * c.cin + cip) * c.ntap + tap];
            if (c.sigma) val = val / *c.sigma;
        }
        if (cip < c.cinp) c.wf[((long)tap * c.cout + co) * c.cinp + cip] = val;
        if (c.wd) c.wd[((long)tap * c.cind + cip) * c.cout + co] = val;
    }
}

// ------------------------------------------------------------------------------------------------------------------ conv forward
struct D3ConvArgs {
    const float* in;     // [N][Ti][Hi][Wi][cinp]
    const float* wf;     // [ntap][cout][cinp]
    float* out;          // [M][cout]
    long M;
    int Ti, Hi, Wi, To, Ho, Wo, cinp, C4, nchunk, ntap, kh, kw, st, ss, cout;
};

template <int NT, int MR>   // BN = 16 NT columns, BM = 64 MR rows per workgroup
__global__ __launch_bounds__(256) void d3_conv_kernel(D3ConvArgs a) {
    constexpr int BN = 16 * NT, BM = 64 * MR;
    __shared__ __attribute__((aligned(16))) float a_lds[2][BM * D3_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * D3_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4, q = tid & 3;
    const int nNt = a.cout / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * BM;
    const int khw = a.kh * a.kw, ph = a.kh >> 1, pw = a.kw >> 1;

    int rb[MR], rt[MR], rh[MR], rw[MR];
#pragma unroll
    for (int u = 0; u < MR; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < a.M;
        if (!ok) m = 0;
        const int wo = (int)(m % a.Wo); m /= a.Wo;
        const int ho = (int)(m % a.Ho); m /= a.Ho;
        const int to = (int)(m % a.To); m /= a.To;
        rb[u] = ok ? (int)m : -1;
        rt[u] = to * a.st - 1; rh[u] = ho * a.ss - ph; rw[u] = wo * a.ss - pw;
    }
    float4 pa0, pa1, pw0;
    pa1 = pw0 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const int tap = g / a.C4, c = (g - tap * a.C4) * 4;
        const bool tok = tap < a.ntap;   // the stem's last chunk
        const int dt = tap / khw, rr = tap - dt * khw;
        const int dh = rr / a.kw, dw = rr - dh * a.kw;
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            const int t = rt[u] + dt, h = rh[u] + dh, w = rw[u] + dw;
            const bool ok = tok && rb[u] >= 0 && (unsigned)t < (unsigned)a.Ti && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
            const long off = ok ? ((((long)rb[u] * a.Ti + t) * a.Hi + h) * a.Wi + w) * a.cinp + c : 0;
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
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * D3_LS + 4 * q]) = pa0;
        if constexpr (MR == 2) *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * D3_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * D3_LS + 4 * q]) = pw0;
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
        for (int mt = 0; mt < MR; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 16 * MR + 16 * mt + lr) * D3_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * D3_LS + 4 * kq]);
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
#pragma unroll
        for (int mt = 0; mt < MR; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wave * 16 * MR + 16 * mt + 4 * kq + r;
                if (m < a.M) a.out[m * a.cout + n] = acc[mt][nt][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------------------------ input gradient
struct D3DgradArgs {
    const float* g;      // [N][To][Ho][Wo][cout], the gradient at the conv's output
    const float* act;    // a ReLU mask of g's shape (g counts where act > 0) or null
    const float* wd;     // [ntap][cind][cout]
    const float *add, *add_mask;   // of out's shape or null: out = result + add [add_mask > 0]
    float* out;          // [N][Ti][Hi][Wi][cin]; frames: [N][3][Ti][Hi][Wi]
    int N, Ti, Hi, Wi, To, Ho, Wo, cout, C4o, kh, kw, st, ss, cin, cind, frames;
};

template <int NT, int MR>
__global__ __launch_bounds__(256) void d3_dgrad_kernel(D3DgradArgs a) {
    constexpr int BN = 16 * NT, BM = 64 * MR;
    __shared__ __attribute__((aligned(16))) float a_lds[2][BM * D3_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * D3_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4, q = tid & 3;
    // the parity class of this workgroup: (pt, ph, pw), each 0 where its axis has stride 1
    const int cls = blockIdx.y;
    const int pw_ = cls % a.ss, ph_ = (cls / a.ss) % a.ss, pt_ = cls / (a.ss * a.ss);
    const int Tc = (a.Ti - pt_ + a.st - 1) / a.st, Hc = (a.Hi - ph_ + a.ss - 1) / a.ss, Wc = (a.Wi - pw_ + a.ss - 1) / a.ss;
    const long Mc = (long)a.N * Tc * Hc * Wc;
    const int nNt = a.cind / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * BM;
    if (m0 >= Mc) return;
    // taps of the class along an axis of window k, pad p, stride s: k_j = kb + s j with kb = (parity + p) % s
    const int padh = a.kh >> 1, padw = a.kw >> 1;
    const int ktb = (pt_ + 1) % a.st, khb = (ph_ + padh) % a.ss, kwb = (pw_ + padw) % a.ss;
    const int ntt = (3 - ktb + a.st - 1) / a.st, nth = (a.kh - khb + a.ss - 1) / a.ss, ntw = (a.kw - kwb + a.ss - 1) / a.ss;
    const int nchunk = ntt * nth * ntw * a.C4o / 4;

    int rb[MR], rt[MR], rh[MR], rw[MR];   // batch row (-1: masked), t + 1, h + pad, w + pad
#pragma unroll
    for (int u = 0; u < MR; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < Mc;
        if (!ok) m = 0;
        const int wc = (int)(m % Wc); m /= Wc;
        const int hc = (int)(m % Hc); m /= Hc;
        const int tc = (int)(m % Tc); m /= Tc;
        rb[u] = ok ? (int)m : -1;
        rt[u] = tc * a.st + pt_ + 1; rh[u] = hc * a.ss + ph_ + padh; rw[u] = wc * a.ss + pw_ + padw;
    }
    float4 pa0, pa1, pw0;
    pa1 = pw0 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const int tj = g / a.C4o, c = (g - tj * a.C4o) * 4;
        const int jt = tj / (nth * ntw), jr = tj - jt * nth * ntw, jh = jr / ntw, jw = jr - jh * ntw;
        const int kt = ktb + a.st * jt, kh = khb + a.ss * jh, kw = kwb + a.ss * jw;
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            const int dt = rt[u] - kt, dh = rh[u] - kh, dw = rw[u] - kw;   // multiples of the strides by the choice of the taps
            const int to = dt / a.st, ho = dh / a.ss, wo = dw / a.ss;
            const bool ok = rb[u] >= 0 && dt >= 0 && dh >= 0 && dw >= 0 && to < a.To && ho < a.Ho && wo < a.Wo;
            const long off = ok ? ((((long)rb[u] * a.To + to) * a.Ho + ho) * a.Wo + wo) * a.cout + c : 0;
            float4 v = *reinterpret_cast<const float4*>(a.g + off);
            if (a.act) {
                const float4 y = *reinterpret_cast<const float4*>(a.act + off);
                v.x = y.x > 0.f ? v.x : 0.f; v.y = y.y > 0.f ? v.y : 0.f; v.z = y.z > 0.f ? v.z : 0.f; v.w = y.w > 0.f ? v.w : 0.f;
            }
            const float4 z = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (u == 0) pa0 = z; else pa1 = z;
        }
        if (tid < BN * 4) pw0 = *reinterpret_cast<const float4*>(a.wd + ((long)((kt * a.kh + kh) * a.kw + kw) * a.cind + n0 + (tid >> 2)) * a.cout + c);
    };
    auto park = [&](int buf) {
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * D3_LS + 4 * q]) = pa0;
        if constexpr (MR == 2) *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * D3_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * D3_LS + 4 * q]) = pw0;
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
        for (int mt = 0; mt < MR; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 16 * MR + 16 * mt + lr) * D3_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * D3_LS + 4 * kq]);
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
            const int tc = (int)(m % Tc); m /= Tc;
            const int t = tc * a.st + pt_, h = hc * a.ss + ph_, w = wc * a.ss + pw_;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = n0 + 16 * nt + lr;
                if (a.frames) {
                    if (n < 3) a.out[(((m * 3 + n) * a.Ti + t) * a.Hi + h) * a.Wi + w] = acc[mt][nt][r];
                } else if (n < a.cin) {
                    const long o = (((m * a.Ti + t) * a.Hi + h) * a.Wi + w) * a.cin + n;
                    float v = acc[mt][nt][r];
                    if (a.add) v += a.add_mask ? (a.add_mask[o] > 0.f ? a.add[o] : 0.f) : a.add[o];
                    a.out[o] = v;
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
struct D3WgradArgs {
    const float *g, *act;   // as D3DgradArgs
    const float* x;         // the conv's input [N][Ti][Hi][Wi][cinp]
    float* part;            // [slices][ntap][cout][CP]
    long P;                 // positions N To Ho Wo
    int Ti, Hi, Wi, To, Ho, Wo, cinp, cout, CP, kh, kw, st, ss, slice_len;
};

template <int MT, int NT>
__global__ __launch_bounds__(256) void d3_wgrad_kernel(D3WgradArgs a) {
    __shared__ float red[3][MT * NT * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int nCi = a.CP / (16 * NT);
    const int co0 = (int)(blockIdx.x / nCi) * 16 * MT, ci0 = (int)(blockIdx.x % nCi) * 16 * NT;
    const int tap = blockIdx.y, khw = a.kh * a.kw;
    const int kt = tap / khw, kh = (tap - kt * khw) / a.kw, kw = tap - kt * khw - kh * a.kw;
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
        const int to = (int)(m % a.To); m /= a.To;
        const int t = to * a.st - 1 + kt, h = ho * a.ss - (a.kh >> 1) + kh, w = wo * a.ss - (a.kw >> 1) + kw;
        const bool xok = ok && (unsigned)t < (unsigned)a.Ti && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
        const long pix = xok ? ((m * a.Ti + t) * a.Hi + h) * a.Wi + w : 0;
        float av[MT], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int co = co0 + 16 * mt + lr;
            float v = a.g[mrow * a.cout + co];
            if (a.act) v = a.act[mrow * a.cout + co] > 0.f ? v : 0.f;
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

struct D3FinishArgs {
    const float* part;   // [S][ntap][cout][CP]
    const float* w;      // weight_orig [cout][cin][ntap]
    const float *u, *v, *sigma;   // this forward's values; sigma null: no projection
    float* dwn;          // [cout][cin][ntap]
    double* dotp;        // [nblk + 1]: the workgroups' sums of dWn * W, then their total
    float* grad;
    long E;
    int S, cout, cin, CP, ntap, nblk, accumulate;
};

// dWn = the slices' partial sums in slice order; per workgroup sum of dWn * W in float64
__global__ __launch_bounds__(256) void d3_finish_a_kernel(D3FinishArgs a) {
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

// <dWn, W> = the workgroups' sums in block order, once for the whole tensor: dotp[nblk]
__global__ __launch_bounds__(256) void d3_finish_dot_kernel(D3FinishArgs a) {
    __shared__ double red[256];
    double d = 0.0;
    for (int i = threadIdx.x; i < a.nblk; i += 256) d += a.dotp[i];
    d = block_sum(d, red);
    if (threadIdx.x == 0) a.dotp[a.nblk] = d;
}

// dW_orig = (dWn - <dWn, W / sigma> u v^T) / sigma, written or accumulated
__global__ __launch_bounds__(256) void d3_finish_b_kernel(D3FinishArgs a) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= a.E) return;
    float gv = a.dwn[e];
    if (a.sigma) {
        const float sg = *a.sigma;
        const float proj = (float)(a.dotp[a.nblk] / (double)sg);
        const int K = a.cin * a.ntap;
        gv = (gv - proj * a.u[e / K] * a.v[e % K]) / sg;
    }
    a.grad[e] = a.accumulate ? a.grad[e] + gv : gv;
}

// ------------------------------------------------------------------------------------------------------------------ GroupNorm(16)
struct D3GnArgs {
    const float *x, *res, *weight, *bias;   // forward: x [N][P][C], res of the same shape or null
    const float *g, *mask;                  // backward: g at the output, mask (the activated output; g counts where mask > 0) or null
    float *out, *dweight, *dbias;           // out: the forward's output or the backward's dx
    double *stats;                          // [N][16][2]: mean, 1 / sqrt(var + eps)
    double *partial, *ab, *gs;              // slices' sums; backward: [N][C][2] per-channel sums, [N][16][2] per-group sums
    long P, rows_per;
    int N, C, cpg, R, relu, accumulate;
};

// sum and sum of squares of one (sample, group) over a slice of the positions
__global__ __launch_bounds__(256) void d3_gn_stats_kernel(D3GnArgs a) {
    __shared__ double red[256];
    const int grp = blockIdx.x, n = blockIdx.y, r = blockIdx.z;
    const long p0 = r * a.rows_per, p1 = p0 + a.rows_per < a.P ? p0 + a.rows_per : a.P;
    const long cnt = p1 > p0 ? (p1 - p0) * a.cpg : 0;
    const float* base = a.x + (long)n * a.P * a.C + grp * a.cpg;
    double s = 0.0, q = 0.0;
    for (long i = threadIdx.x; i < cnt; i += 256) {
        const long p = p0 + i / a.cpg;
        const double v = (double)base[p * a.C + (int)(i % a.cpg)];
        s += v; q += v * v;
    }
    s = block_sum(s, red);
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
        double* dst = a.partial + (((long)n * D3_GROUPS + grp) * a.R + r) * 2;
        dst[0] = s; dst[1] = q;
    }
}

__global__ __launch_bounds__(256) void d3_gn_stats_final_kernel(D3GnArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * D3_GROUPS) return;
    double s = 0.0, q = 0.0;
    for (int r = 0; r < a.R; ++r) { s += a.partial[((long)i * a.R + r) * 2]; q += a.partial[((long)i * a.R + r) * 2 + 1]; }
    const double m = (double)a.P * a.cpg, mean = s / m;
    const double var = fmax(q / m - mean * mean, 0.0);
    a.stats[2 * i] = mean;
    a.stats[2 * i + 1] = 1.0 / sqrt(var + 1e-5);
}

__global__ __launch_bounds__(256) void d3_gn_apply_kernel(D3GnArgs a) {
    const long total4 = (long)a.N * a.P * a.C / 4, pc4 = a.P * a.C / 4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += gridDim.x * 256L) {
        const int n = (int)(i / pc4), c = (int)((i * 4) % a.C);
        const float4 xv = *reinterpret_cast<const float4*>(a.x + 4 * i);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        float ys[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double* st = a.stats + ((long)n * D3_GROUPS + (c + j) / a.cpg) * 2;
            ys[j] = fmaf((float)(((double)xs[j] - st[0]) * st[1]), a.weight[c + j], a.bias[c + j]);
        }
        if (a.res) {
            const float4 rv = *reinterpret_cast<const float4*>(a.res + 4 * i);
            ys[0] += rv.x; ys[1] += rv.y; ys[2] += rv.z; ys[3] += rv.w;
        }
        if (a.relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) ys[j] = ys[j] > 0.f ? ys[j] : 0.f;
        }
        *reinterpret_cast<float4*>(a.out + 4 * i) = make_float4(ys[0], ys[1], ys[2], ys[3]);
    }
}

// per (sample, channel) over a slice of the positions: sum of dy and of dy * xhat, dy = g [mask > 0]; 16 channels x 16 rows per workgroup
__global__ __launch_bounds__(256) void d3_gn_bwd_partial_kernel(D3GnArgs a) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), n = blockIdx.y, r = blockIdx.z;
    const long p0 = r * a.rows_per, p1 = p0 + a.rows_per < a.P ? p0 + a.rows_per : a.P;
    const double* st = a.stats + ((long)n * D3_GROUPS + c / a.cpg) * 2;
    const double mean = st[0], rstd = st[1];
    double s1 = 0.0, s2 = 0.0;
    for (long p = p0 + (tid >> 4); p < p1; p += 16) {
        const long o = ((long)n * a.P + p) * a.C + c;
        float dy = a.g[o];
        if (a.mask) dy = a.mask[o] > 0.f ? dy : 0.f;
        s1 += (double)dy;
        s2 += (double)dy * (((double)a.x[o] - mean) * rstd);
    }
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    if (tid >= 16) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < 16; ++j) { t1 += red[0][j * 16 + tid]; t2 += red[1][j * 16 + tid]; }
    double* dst = a.partial + (((long)n * a.R + r) * a.C + c) * 2;
    dst[0] = t1; dst[1] = t2;
}

// one workgroup per sample: the slices in slice order -> ab [n][c]; then per group sum of weight * ab -> gs [n][group]
__global__ __launch_bounds__(256) void d3_gn_bwd_reduce_kernel(D3GnArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < a.C; c += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int r = 0; r < a.R; ++r) {
            const double* src = a.partial + (((long)n * a.R + r) * a.C + c) * 2;
            t1 += src[0]; t2 += src[1];
        }
        a.ab[((long)n * a.C + c) * 2] = t1;
        a.ab[((long)n * a.C + c) * 2 + 1] = t2;
    }
    __syncthreads();
    if (tid < D3_GROUPS) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < a.cpg; ++j) {
            const int c = tid * a.cpg + j;
            const double w = (double)a.weight[c];
            s1 += w * a.ab[((long)n * a.C + c) * 2];
            s2 += w * a.ab[((long)n * a.C + c) * 2 + 1];
        }
        a.gs[((long)n * D3_GROUPS + tid) * 2] = s1;
        a.gs[((long)n * D3_GROUPS + tid) * 2 + 1] = s2;
    }
}

__global__ __launch_bounds__(256) void d3_gn_bwd_param_kernel(D3GnArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    double t1 = 0.0, t2 = 0.0;
    for (int n = 0; n < a.N; ++n) { t1 += a.ab[((long)n * a.C + c) * 2]; t2 += a.ab[((long)n * a.C + c) * 2 + 1]; }
    a.dbias[c] = a.accumulate ? a.dbias[c] + (float)t1 : (float)t1;
    a.dweight[c] = a.accumulate ? a.dweight[c] + (float)t2 : (float)t2;
}

// dx = rstd (dy w - s1 / m - xhat s2 / m)
__global__ __launch_bounds__(256) void d3_gn_bwd_dx_kernel(D3GnArgs a) {
    const long total = (long)a.N * a.P * a.C, pc = a.P * a.C;
    const double inv_m = 1.0 / ((double)a.P * a.cpg);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int n = (int)(i / pc), c = (int)(i % a.C), grp = c / a.cpg;
        const double* st = a.stats + ((long)n * D3_GROUPS + grp) * 2;
        const double* gs = a.gs + ((long)n * D3_GROUPS + grp) * 2;
        float dy = a.g[i];
        if (a.mask) dy = a.mask[i] > 0.f ? dy : 0.f;
        const double xhat = ((double)a.x[i] - st[0]) * st[1];
        a.out[i] = (float)(st[1] * ((double)dy * (double)a.weight[c] - gs[0] * inv_m - xhat * gs[1] * inv_m));
    }
}

// =================================================================================================================== host side
int bn_of(int c) { return c % 64 == 0 ? 64 : c % 32 == 0 ? 32 : 16; }
// rows per workgroup of the two GEMM kernels: 128, or 64 where 128 would leave the device's compute units without two workgroups each
// (a function of the shape alone: the same shape always runs the same kernel)
int rows_of(long rows, int column_tiles) { return (rows + 127) / 128 * column_tiles >= 512 ? 128 : 64; }

int ntap_of(const D3Conv& c) { return 3 * c.kh * c.kw; }

D3Conv make_conv(int cin, int cout, bool stem, int st, int ss, int sn) {
    return D3Conv{cin, cin == 3 ? 4 : cin, cin == 3 ? 16 : cin, cout, stem ? 7 : 3, stem ? 7 : 3, st, ss, sn};
}
int out_extent(int n, int k, int s) { return n + 2 * (k / 2) - k < 0 ? 0 : (n + 2 * (k / 2) - k) / s + 1; }
D3Geo make_geo(int n, int ti, int hi, int wi, const D3Conv& c) {
    D3Geo m{};
    m.ti = ti; m.hi = hi; m.wi = wi;
    m.to = out_extent(ti, 3, c.st); m.ho = out_extent(hi, c.kh, c.ss); m.wo = out_extent(wi, c.kw, c.ss);
    m.mi = (long)n * ti * hi * wi; m.mo = (long)n * m.to * m.ho * m.wo;
    return m;
}
size_t pack_elems(const D3Conv& c) { return (size_t)c.cout * c.cind * ntap_of(c); }

// the slice plan of the weight gradient: enough workgroups to fill the device, slices of at least 64 positions
void d3_wgrad_plan(int cout, int cin, int ntap, long P, int* slices, int* slice_len) {
    const int CP = (int)align_up(cin == 3 ? 4 : cin, 16);
    const long tiles = (long)ntap * (cout / bn_of(cout)) * (CP / bn_of(CP));
    const long S = std::min<long>(std::max<long>((1024 + tiles - 1) / tiles, 1), std::max<long>((P + 63) / 64, 1));
    const long L = (long)align_up((size_t)((P + S - 1) / S), 16);
    *slice_len = (int)L;
    *slices = (int)((P + L - 1) / L);
}

int launch_conv(const D3Conv& c, const float* in, const float* wf, float* out, const D3Geo& mp, hipStream_t st) {
    D3ConvArgs a{};
    a.in = in; a.wf = wf; a.out = out;
    a.M = mp.mo; a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo;
    a.cinp = c.cinp; a.C4 = c.cinp / 4; a.ntap = ntap_of(c); a.nchunk = (a.ntap * a.C4 + 3) / 4; a.kh = c.kh; a.kw = c.kw; a.st = c.st; a.ss = c.ss;
    a.cout = c.cout;
    const int BN = bn_of(c.cout);
    const int BM = rows_of(a.M, c.cout / BN);
    const long nblk = (a.M + BM - 1) / BM * (c.cout / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "temporal discriminator: conv grid of %ld workgroups", nblk);
    const dim3 grid((unsigned)nblk);
    if (BM == 128) {
        if (BN == 64) hipLaunchKernelGGL((d3_conv_kernel<4, 2>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((d3_conv_kernel<2, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((d3_conv_kernel<1, 2>), grid, dim3(256), 0, st, a);
    } else {
        if (BN == 64) hipLaunchKernelGGL((d3_conv_kernel<4, 1>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((d3_conv_kernel<2, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((d3_conv_kernel<1, 1>), grid, dim3(256), 0, st, a);
    }
    PD_LAUNCHED();
    return I2V_OK;
}

int launch_dgrad(const D3Conv& c, const float* g, const float* act, const float* wd, const float* add, const float* add_mask, float* out, bool frames,
                 int N, const D3Geo& mp, hipStream_t st) {
    D3DgradArgs a{};
    a.g = g; a.act = act; a.wd = wd; a.add = add; a.add_mask = add_mask; a.out = out;
    a.N = N; a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo;
    a.cout = c.cout; a.C4o = c.cout / 4; a.kh = c.kh; a.kw = c.kw; a.st = c.st; a.ss = c.ss;
    a.cin = c.cin == 3 && !frames ? 4 : c.cin; a.cind = c.cind; a.frames = frames ? 1 : 0;
    const int BN = bn_of(c.cind);
    const int classes = c.st * c.ss * c.ss;
    const long mc = (long)N * ((mp.ti + c.st - 1) / c.st) * ((mp.hi + c.ss - 1) / c.ss) * ((mp.wi + c.ss - 1) / c.ss);   // the largest parity class
    const int BM = rows_of(mc * classes, c.cind / BN);
    const long nblk = (mc + BM - 1) / BM * (c.cind / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "temporal discriminator: dgrad grid of %ld workgroups", nblk);
    const dim3 grid((unsigned)nblk, classes);
    if (BM == 128) {
        if (BN == 64) hipLaunchKernelGGL((d3_dgrad_kernel<4, 2>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((d3_dgrad_kernel<2, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((d3_dgrad_kernel<1, 2>), grid, dim3(256), 0, st, a);
    } else {
        if (BN == 64) hipLaunchKernelGGL((d3_dgrad_kernel<4, 1>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((d3_dgrad_kernel<2, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((d3_dgrad_kernel<1, 1>), grid, dim3(256), 0, st, a);
    }
    PD_LAUNCHED();
    return I2V_OK;
}

template <int MT>
void launch_wgrad_nt(int nt, dim3 grid, hipStream_t st, const D3WgradArgs& a) {
    if (nt == 4) hipLaunchKernelGGL((d3_wgrad_kernel<MT, 4>), grid, dim3(256), 0, st, a);
    else if (nt == 2) hipLaunchKernelGGL((d3_wgrad_kernel<MT, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((d3_wgrad_kernel<MT, 1>), grid, dim3(256), 0, st, a);
}

size_t wgrad_part_floats(const D3Conv& c, long P) {
    int S, L;
    d3_wgrad_plan(c.cout, c.cin, ntap_of(c), P, &S, &L);
    return (size_t)S * ntap_of(c) * c.cout * align_up(c.cinp, 16);
}
size_t finish_blocks(const D3Conv& c) { return ((size_t)c.cout * c.cin * ntap_of(c) + 255) / 256; }

// partial sums -> dwn -> grad (written or accumulated)
int launch_wgrad(const D3Conv& c, const float* g, const float* act, const float* x, const float* w, const float* u, const float* v, const float* sigma,
                 float* part, float* dwn, double* dotp, float* grad, bool accumulate, const D3Geo& mp, hipStream_t st) {
    int S, L;
    const int ntap = ntap_of(c);
    d3_wgrad_plan(c.cout, c.cin, ntap, mp.mo, &S, &L);
    D3WgradArgs a{};
    a.g = g; a.act = act; a.x = x; a.part = part; a.P = mp.mo;
    a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo; a.cinp = c.cinp; a.cout = c.cout; a.CP = (int)align_up(c.cinp, 16);
    a.kh = c.kh; a.kw = c.kw; a.st = c.st; a.ss = c.ss; a.slice_len = L;
    const int mt = bn_of(c.cout) / 16, nt = bn_of(a.CP) / 16;
    const dim3 grid((unsigned)((c.cout / (16 * mt)) * (a.CP / (16 * nt))), ntap, (unsigned)S);
    if (mt == 4) launch_wgrad_nt<4>(nt, grid, st, a);
    else if (mt == 2) launch_wgrad_nt<2>(nt, grid, st, a);
    else launch_wgrad_nt<1>(nt, grid, st, a);
    PD_LAUNCHED();
    D3FinishArgs f{};
    f.part = part; f.w = w; f.u = u; f.v = v; f.sigma = sigma; f.dwn = dwn; f.dotp = dotp; f.grad = grad;
    f.E = (long)c.cout * c.cin * ntap; f.S = S; f.cout = c.cout; f.cin = c.cin; f.CP = a.CP; f.ntap = ntap; f.nblk = (int)finish_blocks(c);
    f.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(d3_finish_a_kernel, dim3(f.nblk), dim3(256), 0, st, f);
    PD_LAUNCHED();
    if (sigma) {
        hipLaunchKernelGGL(d3_finish_dot_kernel, dim3(1), dim3(256), 0, st, f);
        PD_LAUNCHED();
    }
    hipLaunchKernelGGL(d3_finish_b_kernel, dim3(f.nblk), dim3(256), 0, st, f);
    PD_LAUNCHED();
    return I2V_OK;
}

// GroupNorm scratch: `partial` serves the forward's statistics ([N][16][R][2]) and the backward's channel sums ([N][R][C][2])
struct D3GnWs { size_t partial, ab, gs, total; };
D3GnWs gn_ws(int n, int c) {
    Carver k;
    D3GnWs y{};
    y.partial = k.take_bytes((size_t)n * D3_GN_SLICES * std::max(c, D3_GROUPS) * 2 * 8);
    y.ab = k.take_bytes((size_t)n * c * 2 * 8);
    y.gs = k.take_bytes((size_t)n * D3_GROUPS * 2 * 8);
    y.total = k.total();
    return y;
}
int gn_slices(long P, int per_row) { return (int)std::min<long>(std::max<long>(P * per_row / 4096, 1), D3_GN_SLICES); }

int launch_gn(const float* x, const float* res, const float* weight, const float* bias, int N, long P, int C, bool relu, float* out, double* stats,
              void* ws, hipStream_t st) {
    const D3GnWs k = gn_ws(N, C);
    D3GnArgs a{};
    a.x = x; a.res = res; a.weight = weight; a.bias = bias; a.out = out; a.stats = stats; a.partial = Carver::at<double>(ws, k.partial);
    a.P = P; a.N = N; a.C = C; a.cpg = C / D3_GROUPS; a.R = gn_slices(P, a.cpg); a.rows_per = (P + a.R - 1) / a.R; a.relu = relu ? 1 : 0;
    hipLaunchKernelGGL(d3_gn_stats_kernel, dim3(D3_GROUPS, N, a.R), dim3(256), 0, st, a);
    PD_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_stats_final_kernel, dim3((N * D3_GROUPS + 255) / 256), dim3(256), 0, st, a);
    PD_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_apply_kernel, dim3(grid_for((long)N * P * C / 4)), dim3(256), 0, st, a);
    PD_LAUNCHED();
    return I2V_OK;
}

int launch_gn_bwd(const float* g, const float* mask, const float* x, const double* stats, const float* weight, int N, long P, int C, float* dx,
                  float* dweight, float* dbias, bool accumulate, void* ws, hipStream_t st) {
    const D3GnWs k = gn_ws(N, C);
    D3GnArgs a{};
    a.g = g; a.mask = mask; a.x = x; a.stats = const_cast<double*>(stats); a.weight = weight; a.out = dx; a.dweight = dweight; a.dbias = dbias;
    a.partial = Carver::at<double>(ws, k.partial); a.ab = Carver::at<double>(ws, k.ab); a.gs = Carver::at<double>(ws, k.gs);
    a.P = P; a.N = N; a.C = C; a.cpg = C / D3_GROUPS; a.R = gn_slices(P, 16); a.rows_per = (P + a.R - 1) / a.R; a.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(d3_gn_bwd_partial_kernel, dim3(C / 16, N, a.R), dim3(256), 0, st, a);
    PD_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_bwd_reduce_kernel, dim3(N), dim3(256), 0, st, a);
    PD_LAUNCHED();
    if (dweight) {
        hipLaunchKernelGGL(d3_gn_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, st, a);
        PD_LAUNCHED();
    }
    hipLaunchKernelGGL(d3_gn_bwd_dx_kernel, dim3(grid_for((long)N * P * C)), dim3(256), 0, st, a);
    PD_LAUNCHED();
    return I2V_OK;
}

}  // namespace
}  // namespace i2v
