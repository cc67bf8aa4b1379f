// The spatial (patch) discriminator of stage-1 training: NLayerDiscriminator (stage1_VAE/modules/patch_disc.py:101-165) forward and
// backward, spectral norm in training mode, ActNorm with its data init, and the hinge loss (stage1_VAE/modules/loss.py:24-32).  The
// C ABI is include/i2v_hip_disc.h.  Exact fp32 on v_mfma_f32_16x16x4_f32; every sum has one owner and a fixed order.
//   * Activations are channels-last [N][H][W][C]; the frames are stored with 4 channels (r, g, b, 0) as the VGG and Inception input
//     stages store them.
//   * A forward packs W / sigma of every conv once, on the device, into the two operand layouts: wf [tap][cout][cin] (forward: K over
//     (tap, channel)) and wd [tap][cin][cout] (input gradient: K over (tap, output channel)).  With I2V_PATCHDISC_SAVE they live in
//     `saved` together with that call's u, v and sigma: a backward uses those values of ITS forward.  weight_orig (the projection),
//     loc and scale are read from the bound parameters at backward time: they must not change between a forward and its backward.
//   * conv forward: the flat implicit GEMM of i2v_flatconv.h (128 or 64 positions x BN channels per workgroup, chunks of 16 K elements
//     double-buffered in LDS) with the window fixed at 4 x 4 pad 1 and the epilogue bias -> [pre] -> ActNorm -> LeakyReLU.
//   * dgrad: the same GEMM as a gather over input pixels.  At stride 2 a pixel receives the 2 x 2 taps of its parity, so the pixels
//     are processed in four parity classes (blockIdx.y), each with its own taps: K = 4 cout.  The upstream gradient passes through
//     the LeakyReLU mask and ActNorm's scale while it is loaded.
//   * wgrad: per tap a [cout] x [cin] GEMM over the positions, operands straight from global memory.  The position range is cut into
//     slices (pd_wgrad_plan, a pure function of the shape); the four waves of a workgroup take a quarter of a slice each and are
//     summed in LDS in wave order; the slices' partial sums are added in slice order by pd_finish_a, which also forms the blocks
//     of <dWn, W>; pd_finish_b adds those in block order, applies the spectral-norm projection and writes or accumulates.
//   * the cout = 1 head is a dot product per position (one wave), with thread-per-element gradient forms.
#include "i2v_handle.h"
#include "i2v_power_iter.h"
#include "../../include/i2v_hip_disc.h"

namespace i2v {
namespace {

constexpr int PD_LS = 20;   // floats per staged row of 16

struct PdConv { int cin, cinp, cind, cout, stride, actnorm, lrelu, key; };   // cinp: channels of the stored input map; cind: columns of the dgrad GEMM
struct PdMap { int hi, wi, ho, wo; long mi, mo; };

__device__ __forceinline__ float lrelu_slope(float a) { return a > 0.f ? 1.f : 0.2f; }

// ------------------------------------------------------------------------------------------------------------------ input stage
__global__ __launch_bounds__(256) void pd_input4_kernel(const float* __restrict__ x, float* __restrict__ out, long npix, long hw) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < npix; i += gridDim.x * 256L) {
        const long n = i / hw, p = i - n * hw;
        const float* s = x + n * 3 * hw + p;
        *reinterpret_cast<float4*>(out + 4 * i) = make_float4(s[0], s[hw], s[2 * hw], 0.f);
    }
}

// ------------------------------------------------------------------------------------------------------------------ spectral norm
// (the power iteration: i2v_power_iter.h)  W / sigma into the two operand layouts
struct PdPackConv { const float* w; const float* sigma; float* wf; float* wd; int cout, cin, cinp, cind; long first; };
struct PdPackArgs { PdPackConv c[PD_MAXCONV]; int nconv; long total; };

__global__ __launch_bounds__(256) void pd_pack_kernel(PdPackArgs a) {
    for (long e = blockIdx.x * 256L + threadIdx.x; e < a.total; e += gridDim.x * 256L) {
        int ci = 0;
        while (ci + 1 < a.nconv && e >= a.c[ci + 1].first) ++ci;
        const PdPackConv& c = a.c[ci];
        long r = e - c.first;                       // ((co * cind) + cip) * 16 + tap
        const int tap = (int)(r & 15); r >>= 4;
        const int cip = (int)(r % c.cind), co = (int)(r / c.cind);
        float val = 0.f;
        if (cip < c.cin) {
            val = c.w[((long)co * c.cin + cip) * 16 + tap];
            if (c.sigma) val = val / *c.sigma;
        }
        if (cip < c.cinp) c.wf[((long)tap * c.cout + co) * c.cinp + cip] = val;
        if (c.wd) c.wd[((long)tap * c.cind + cip) * c.cout + co] = val;
    }
}

// ------------------------------------------------------------------------------------------------------------------ conv forward
struct PdConvArgs {
    const float* in;     // [N][Hi][Wi][cinp]
    const float* wf;     // [16][cout][cinp]
    const float *bias, *loc, *scale;   // loc / scale null: no ActNorm
    float *out, *pre;    // [M][cout]; either may be null
    long M;
    int Hi, Wi, Ho, Wo, cinp, C4, nchunk, stride, cout, lrelu;
};

template <int NT, int MR>   // BN = 16 NT columns, BM = 64 MR rows per workgroup
__global__ __launch_bounds__(256) void pd_conv_kernel(PdConvArgs a) {
    constexpr int BN = 16 * NT, BM = 64 * MR;
    __shared__ __attribute__((aligned(16))) float a_lds[2][BM * PD_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * PD_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4, q = tid & 3;
    const int nNt = a.cout / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * BM;

    int rb[MR], rh[MR], rw[MR];
#pragma unroll
    for (int u = 0; u < MR; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < a.M;
        if (!ok) m = 0;
        const int wo = (int)(m % a.Wo); m /= a.Wo;
        const int ho = (int)(m % a.Ho); m /= a.Ho;
        rb[u] = ok ? (int)m : -1;
        rh[u] = ho * a.stride - 1; rw[u] = wo * a.stride - 1;
    }
    float4 pa0, pa1, pw0;
    pa1 = pw0 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const int tap = g / a.C4, c = (g - tap * a.C4) * 4;
        const int dh = tap >> 2, dw = tap & 3;
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            const int h = rh[u] + dh, w = rw[u] + dw;
            const bool ok = rb[u] >= 0 && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
            const long off = ok ? (((long)rb[u] * a.Hi + h) * a.Wi + w) * a.cinp + c : 0;
            const float4 v = *reinterpret_cast<const float4*>(a.in + off);
            const float4 z = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (u == 0) pa0 = z; else pa1 = z;
        }
        if (tid < BN * 4) pw0 = *reinterpret_cast<const float4*>(a.wf + ((long)tap * a.cout + n0 + (tid >> 2)) * a.cinp + c);
    };
    auto park = [&](int buf) {
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * PD_LS + 4 * q]) = pa0;
        if constexpr (MR == 2) *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * PD_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * PD_LS + 4 * q]) = pw0;
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
        for (int mt = 0; mt < MR; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 16 * MR + 16 * mt + lr) * PD_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * PD_LS + 4 * kq]);
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
        const float b = a.bias[n];
        const float lc = a.loc ? a.loc[n] : 0.f, sc = a.loc ? a.scale[n] : 1.f;
#pragma unroll
        for (int mt = 0; mt < MR; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + wave * 16 * MR + 16 * mt + 4 * kq + r;
                if (m >= a.M) continue;
                float y = acc[mt][nt][r] + b;
                if (a.pre) a.pre[m * a.cout + n] = y;
                if (a.loc) y = sc * (y + lc);
                if (a.lrelu) y = y > 0.f ? y : 0.2f * y;
                if (a.out) a.out[m * a.cout + n] = y;
            }
    }
}

// h = LeakyReLU(scale * (pre + loc)): the forward that initialises ActNorm computes the conv first and applies the norm afterwards
__global__ __launch_bounds__(256) void pd_actnorm_apply_kernel(const float* __restrict__ pre, const float* __restrict__ loc, const float* __restrict__ scale,
                                                               float* __restrict__ out, long total, int C) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % C);
        const float y = scale[c] * (pre[i] + loc[c]);
        out[i] = y > 0.f ? y : 0.2f * y;
    }
}

// per channel over the M rows of x [M][C]: loc = -mean, scale = 1 / (unbiased std + 1e-6); float64, two passes, fixed order
__global__ __launch_bounds__(256) void pd_actnorm_init_kernel(const float* __restrict__ x, long M, int C, float* __restrict__ loc, float* __restrict__ scale) {
    __shared__ double red[256];
    __shared__ double meanv[4];
    const int CG = C >= 4 ? 4 : 1, tid = threadIdx.x;
    const int c = blockIdx.x * CG + tid % CG, rstep = 256 / CG;
    double s = 0.0;
    for (long r = tid / CG; r < M; r += rstep) s += (double)x[r * C + c];
    red[tid] = s;
    __syncthreads();
    if (tid < CG) {
        double t = 0.0;
        for (int j = 0; j < rstep; ++j) t += red[j * CG + tid];
        meanv[tid] = t / (double)M;
    }
    __syncthreads();
    const double mean = meanv[tid % CG];
    double qd = 0.0;
    for (long r = tid / CG; r < M; r += rstep) {
        const double d = (double)x[r * C + c] - mean;
        qd += d * d;
    }
    red[tid] = qd;
    __syncthreads();
    if (tid < CG) {
        double t = 0.0;
        for (int j = 0; j < rstep; ++j) t += red[j * CG + tid];
        loc[c] = (float)(-mean);
        scale[c] = (float)(1.0 / (sqrt(t / (double)(M - 1)) + 1e-6));
    }
}

// ------------------------------------------------------------------------------------------------------------------ input gradient
struct PdDgradArgs {
    const float* g;      // [N][Ho][Wo][cout], the gradient at the layer's activation
    const float* act;    // the activation itself (the LeakyReLU mask) or null
    const float* scale;  // ActNorm's scale [cout] or null
    const float* wd;     // [16][cind][cout]
    float* out;          // [N][Hi][Wi][cin]; frames: [N][3][Hi][Wi]
    int N, Hi, Wi, Ho, Wo, cout, C4o, stride, cin, cind, frames;
};

template <int NT, int MR>
__global__ __launch_bounds__(256) void pd_dgrad_kernel(PdDgradArgs a) {
    constexpr int BN = 16 * NT, BM = 64 * MR;
    __shared__ __attribute__((aligned(16))) float a_lds[2][BM * PD_LS];
    __shared__ __attribute__((aligned(16))) float w_lds[2][BN * PD_LS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4, q = tid & 3;
    // the pixels of one parity class (stride 2) or all of them (stride 1)
    const int s2 = a.stride == 2;
    const int ph = s2 ? (int)(blockIdx.y >> 1) : 0, pw = s2 ? (int)(blockIdx.y & 1) : 0;
    const int Hc = s2 ? (a.Hi + 1 - ph) / 2 : a.Hi, Wc = s2 ? (a.Wi + 1 - pw) / 2 : a.Wi;
    const long Mc = (long)a.N * Hc * Wc;
    const int nNt = a.cind / BN;
    const int n0 = (int)(blockIdx.x % nNt) * BN;
    const long m0 = (long)(blockIdx.x / nNt) * BM;
    if (m0 >= Mc) return;
    const int khb = s2 ? (ph + 1) & 1 : 0, kwb = s2 ? (pw + 1) & 1 : 0;
    const int ntap = s2 ? 4 : 16;
    const int nchunk = ntap * a.C4o / 4;

    int rb[MR], rh[MR], rw[MR];   // batch row (-1: masked), h + 1, w + 1
#pragma unroll
    for (int u = 0; u < MR; ++u) {
        long m = m0 + (tid >> 2) + 64 * u;
        const bool ok = m < Mc;
        if (!ok) m = 0;
        const int wc = (int)(m % Wc); m /= Wc;
        const int hc = (int)(m % Hc); m /= Hc;
        rb[u] = ok ? (int)m : -1;
        rh[u] = (s2 ? 2 * hc + ph : hc) + 1; rw[u] = (s2 ? 2 * wc + pw : wc) + 1;
    }
    float4 pa0, pa1, pw0;
    pa1 = pw0 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int ch) {
        const int g = ch * 4 + q;
        const int tj = g / a.C4o, c = (g - tj * a.C4o) * 4;
        const int kh = s2 ? khb + 2 * (tj >> 1) : tj >> 2, kw = s2 ? kwb + 2 * (tj & 1) : tj & 3;
#pragma unroll
        for (int u = 0; u < MR; ++u) {
            const int th = rh[u] - kh, tw = rw[u] - kw;   // even at stride 2 by the choice of the taps
            const int ho = s2 ? th >> 1 : th, wo = s2 ? tw >> 1 : tw;
            const bool ok = rb[u] >= 0 && th >= 0 && tw >= 0 && ho < a.Ho && wo < a.Wo;
            const long off = ok ? (((long)rb[u] * a.Ho + ho) * a.Wo + wo) * a.cout + c : 0;
            float4 v = *reinterpret_cast<const float4*>(a.g + off);
            if (a.act) {
                const float4 y = *reinterpret_cast<const float4*>(a.act + off);
                v.x *= lrelu_slope(y.x); v.y *= lrelu_slope(y.y); v.z *= lrelu_slope(y.z); v.w *= lrelu_slope(y.w);
            }
            if (a.scale) {
                const float4 sc = *reinterpret_cast<const float4*>(a.scale + c);
                v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w;
            }
            const float4 z = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            if (u == 0) pa0 = z; else pa1 = z;
        }
        if (tid < BN * 4) pw0 = *reinterpret_cast<const float4*>(a.wd + ((long)(kh * 4 + kw) * a.cind + n0 + (tid >> 2)) * a.cout + c);
    };
    auto park = [&](int buf) {
        *reinterpret_cast<float4*>(&a_lds[buf][(tid >> 2) * PD_LS + 4 * q]) = pa0;
        if constexpr (MR == 2) *reinterpret_cast<float4*>(&a_lds[buf][((tid >> 2) + 64) * PD_LS + 4 * q]) = pa1;
        if (tid < BN * 4) *reinterpret_cast<float4*>(&w_lds[buf][(tid >> 2) * PD_LS + 4 * q]) = pw0;
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
        for (int mt = 0; mt < MR; ++mt) av[mt] = *reinterpret_cast<const float4*>(&a_lds[buf][(wave * 16 * MR + 16 * mt + lr) * PD_LS + 4 * kq]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(&w_lds[buf][(16 * nt + lr) * PD_LS + 4 * kq]);
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
            const int h = s2 ? 2 * hc + ph : hc, w = s2 ? 2 * wc + pw : wc;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const int n = n0 + 16 * nt + lr;
                if (a.frames) {
                    if (n < 3) a.out[((m * 3 + n) * a.Hi + h) * a.Wi + w] = acc[mt][nt][r];
                } else if (n < a.cin) {
                    a.out[((m * a.Hi + h) * a.Wi + w) * a.cin + n] = acc[mt][nt][r];
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
struct PdWgradArgs {
    const float *g, *act, *scale;   // as PdDgradArgs
    const float* x;                 // the conv's input [N][Hi][Wi][cinp]
    float* part;                    // [slices][16][cout][CP]
    long P;                         // positions N Ho Wo
    int Hi, Wi, Ho, Wo, cinp, cout, CP, stride, slice_len;
};

template <int MT, int NT>
__global__ __launch_bounds__(256) void pd_wgrad_kernel(PdWgradArgs a) {
    __shared__ float red[3][MT * NT * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int nCi = a.CP / (16 * NT);
    const int co0 = (int)(blockIdx.x / nCi) * 16 * MT, ci0 = (int)(blockIdx.x % nCi) * 16 * NT;
    const int tap = blockIdx.y, kh = tap >> 2, kw = tap & 3;
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
        const int h = ho * a.stride - 1 + kh, w = wo * a.stride - 1 + kw;
        const bool xok = ok && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi;
        const long pix = xok ? (m * a.Hi + h) * a.Wi + w : 0;
        float av[MT], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int co = co0 + 16 * mt + lr;
            float v = a.g[mrow * a.cout + co];
            if (a.act) v *= lrelu_slope(a.act[mrow * a.cout + co]);
            if (a.scale) v *= a.scale[co];
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
    float* dst = a.part + ((long)sl * 16 + tap) * a.cout * a.CP;
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

struct PdFinishArgs {
    const float* part;   // [S][16][cout][CP]
    const float* w;      // weight_orig [cout][cin][16]
    const float *u, *v, *sigma;   // this forward's values; sigma null: no projection
    float* dwn;          // [cout][cin][16]
    double* dotp;        // [nblk]
    float* grad;
    long E;
    int S, cout, cin, CP, nblk, accumulate;
};

// dWn = the slices' partial sums in slice order; per workgroup sum of dWn * W in float64
__global__ __launch_bounds__(256) void pd_finish_a_kernel(PdFinishArgs a) {
    __shared__ double red[256];
    const long e = blockIdx.x * 256L + threadIdx.x;
    double d = 0.0;
    if (e < a.E) {
        const int K = a.cin * 16;
        const int co = (int)(e / K), k = (int)(e % K), ci = k >> 4, tap = k & 15;
        float sum = 0.f;
        for (int s = 0; s < a.S; ++s) sum += a.part[(((long)s * 16 + tap) * a.cout + co) * a.CP + ci];
        a.dwn[e] = sum;
        d = (double)sum * (double)a.w[e];
    }
    d = block_sum(d, red);
    if (threadIdx.x == 0) a.dotp[blockIdx.x] = d;
}

// dW_orig = (dWn - <dWn, W / sigma> u v^T) / sigma, written or accumulated
__global__ __launch_bounds__(256) void pd_finish_b_kernel(PdFinishArgs a) {
    __shared__ double red[256];
    float proj = 0.f, sg = 1.f;
    if (a.sigma) {
        double d = 0.0;
        for (int i = threadIdx.x; i < a.nblk; i += 256) d += a.dotp[i];
        d = block_sum(d, red);
        sg = *a.sigma;
        proj = (float)(d / (double)sg);
    }
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= a.E) return;
    float gv = a.dwn[e];
    if (a.sigma) {
        const int K = a.cin * 16;
        gv = (gv - proj * a.u[e / K] * a.v[e % K]) / sg;
    }
    a.grad[e] = a.accumulate ? a.grad[e] + gv : gv;
}

// per channel over the M rows: dh = g * mask; dbias = scale * sum dh, d_loc = scale * sum dh, d_scale = sum dh * (pre + loc); float64.
// Two stages: a workgroup sums a row slice of 16 channels (C = 1: of the one) into `partial` [R][C][2]; the second adds the slices in order
struct PdChanArgs {
    const float *g, *act, *pre, *loc, *scale;   // act null: no mask; pre / loc / scale null: no ActNorm
    float *dbias, *dloc, *dscale;
    double* partial;
    long M, rows_per;
    int C, R, accumulate;
};

__global__ __launch_bounds__(256) void pd_chan_partial_kernel(PdChanArgs a) {
    __shared__ double red[2][256];
    const int CW = a.C >= 16 ? 16 : 1, tid = threadIdx.x;
    const int c = blockIdx.x * CW + tid % CW, rstep = 256 / CW;
    const long r0 = blockIdx.y * a.rows_per, r1 = r0 + a.rows_per < a.M ? r0 + a.rows_per : a.M;
    const float lc = a.loc ? a.loc[c] : 0.f;
    double s1 = 0.0, s2 = 0.0;
    for (long r = r0 + tid / CW; r < r1; r += rstep) {
        float dh = a.g[r * a.C + c];
        if (a.act) dh *= lrelu_slope(a.act[r * a.C + c]);
        s1 += (double)dh;
        if (a.pre) s2 += (double)dh * (double)(a.pre[r * a.C + c] + lc);
    }
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    if (tid >= CW) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < rstep; ++j) { t1 += red[0][j * CW + tid]; t2 += red[1][j * CW + tid]; }
    a.partial[((long)blockIdx.y * a.C + c) * 2] = t1;
    a.partial[((long)blockIdx.y * a.C + c) * 2 + 1] = t2;
}

__global__ __launch_bounds__(256) void pd_chan_final_kernel(PdChanArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < a.R; ++j) { t1 += a.partial[((long)j * a.C + c) * 2]; t2 += a.partial[((long)j * a.C + c) * 2 + 1]; }
    const double sc = a.scale ? (double)a.scale[c] : 1.0;
    const float db = (float)(sc * t1);
    a.dbias[c] = a.accumulate ? a.dbias[c] + db : db;
    if (a.pre) {
        a.dloc[c] = a.accumulate ? a.dloc[c] + db : db;
        a.dscale[c] = a.accumulate ? a.dscale[c] + (float)t2 : (float)t2;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the cout = 1 head
// one wave per output position: 16 taps x cin products, lanes over channels, fixed shuffle tree
__global__ __launch_bounds__(256) void pd_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wf, const float* __restrict__ bias,
                                                          float* __restrict__ out, long M, int Hi, int Wi, int cin) {
    const int lane = threadIdx.x & 63;
    const long m = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (m >= M) return;
    const int Ho = Hi - 1, Wo = Wi - 1;
    const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
    const long n = m / ((long)Wo * Ho);
    float acc = 0.f;
    for (int tap = 0; tap < 16; ++tap) {
        const int h = ho - 1 + (tap >> 2), w = wo - 1 + (tap & 3);
        if ((unsigned)h >= (unsigned)Hi || (unsigned)w >= (unsigned)Wi) continue;
        const float* xs = x + ((n * Hi + h) * Wi + w) * cin;
        const float* ws = wf + (long)tap * cin;
        for (int c = 4 * lane; c < cin; c += 256) {
            const float4 xv = *reinterpret_cast<const float4*>(xs + c), wv = *reinterpret_cast<const float4*>(ws + c);
            acc = fmaf(xv.x, wv.x, acc); acc = fmaf(xv.y, wv.y, acc); acc = fmaf(xv.z, wv.z, acc); acc = fmaf(xv.w, wv.w, acc);
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[m] = acc + bias[0];
}

__global__ __launch_bounds__(256) void pd_head_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ wf, float* __restrict__ out, long total,
                                                            int Hi, int Wi, int cin) {
    const int Ho = Hi - 1, Wo = Wi - 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % cin);
        long p = i / cin;
        const int w = (int)(p % Wi); p /= Wi;
        const int h = (int)(p % Hi); p /= Hi;
        float acc = 0.f;
        for (int tap = 0; tap < 16; ++tap) {
            const int ho = h + 1 - (tap >> 2), wo = w + 1 - (tap & 3);
            if ((unsigned)ho >= (unsigned)Ho || (unsigned)wo >= (unsigned)Wo) continue;
            acc = fmaf(g[(p * Ho + ho) * Wo + wo], wf[(long)tap * cin + c], acc);
        }
        out[i] = acc;
    }
}

// part [slices][16][cin]: thread = channel, blockIdx.y = tap, blockIdx.z = slice
__global__ __launch_bounds__(256) void pd_head_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ part, long P,
                                                            int Hi, int Wi, int cin, int slice_len) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cin) return;
    const int Ho = Hi - 1, Wo = Wi - 1, tap = blockIdx.y;
    const long begin = (long)blockIdx.z * slice_len, end = begin + slice_len < P ? begin + slice_len : P;
    float acc = 0.f;
    for (long m = begin; m < end; ++m) {
        const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
        const long n = m / ((long)Wo * Ho);
        const int h = ho - 1 + (tap >> 2), w = wo - 1 + (tap & 3);
        if ((unsigned)h >= (unsigned)Hi || (unsigned)w >= (unsigned)Wi) continue;
        acc = fmaf(g[m], x[((n * Hi + h) * Wi + w) * cin + c], acc);
    }
    part[((long)blockIdx.z * 16 + tap) * cin + c] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ hinge loss
__global__ __launch_bounds__(256) void pd_hinge_kernel(const float* __restrict__ fake, const float* __restrict__ real, long n, int mode, double* __restrict__ out,
                                                       float* __restrict__ d_fake, float* __restrict__ d_real) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double lf = 0.0, lr = 0.0, mf = 0.0, mr = 0.0;
    const float gd = (float)(0.5 / (double)n), gg = (float)(-1.0 / (double)n);
    for (long i = tid; i < n; i += 256) {
        const float f = fake[i];
        mf += (double)f;
        if (mode == I2V_HINGE_GEN) {
            if (d_fake) d_fake[i] = gg;
            continue;
        }
        const float r = real[i];
        mr += (double)r;
        const double hf = 1.0 + (double)f, hr = 1.0 - (double)r;   // exact: the hinge sits where the float64 reference has it
        if (hf > 0.0) lf += hf;
        if (hr > 0.0) lr += hr;
        if (d_fake) d_fake[i] = hf > 0.0 ? gd : 0.f;
        if (d_real) d_real[i] = hr > 0.0 ? -gd : 0.f;
    }
    lf = block_sum(lf, red); lr = block_sum(lr, red); mf = block_sum(mf, red); mr = block_sum(mr, red);
    if (tid == 0) {
        const double dn = (double)n;
        out[0] = mode == I2V_HINGE_GEN ? -mf / dn : (lr / dn + lf / dn) / 2.0;
        out[1] = mr / dn;
        out[2] = mf / dn;
    }
}

// =================================================================================================================== host side

int bn_of(int c) { return c % 64 == 0 ? 64 : c % 32 == 0 ? 32 : 16; }
// rows per workgroup of the two GEMM kernels: 128, or 64 where 128 would leave the device's compute units without two workgroups each
// (a function of the shape alone: the same shape always runs the same kernel)
int rows_of(long rows, int column_tiles) { return (rows + 127) / 128 * column_tiles >= 512 ? 128 : 64; }

// the slice plan of the weight gradient: enough workgroups to fill the device, slices of at least 64 positions
void pd_wgrad_plan(int cout, int cin, long P, int* slices, int* slice_len) {
    long S;
    if (cout == 1) {
        S = std::min<long>(std::max<long>((P + 63) / 64, 1), 128);
    } else {
        const int CP = (int)align_up(cin == 3 ? 4 : cin, 16);
        const long tiles = 16L * (cout / bn_of(cout)) * (CP / bn_of(CP));
        S = std::min<long>(std::max<long>((1024 + tiles - 1) / tiles, 1), std::max<long>((P + 63) / 64, 1));
    }
    const long L = (long)align_up((size_t)((P + S - 1) / S), 16);
    *slice_len = (int)L;
    *slices = (int)((P + L - 1) / L);
}

int launch_conv(const PdConv& c, const float* in, const float* wf, const float* bias, const float* loc, const float* scale, float* out, float* pre,
                int N, const PdMap& mp, bool lrelu, hipStream_t st) {
    PdConvArgs a{};
    a.in = in; a.wf = wf; a.bias = bias; a.loc = loc; a.scale = scale; a.out = out; a.pre = pre;
    a.M = mp.mo; a.Hi = mp.hi; a.Wi = mp.wi; a.Ho = mp.ho; a.Wo = mp.wo;
    a.cinp = c.cinp; a.C4 = c.cinp / 4; a.nchunk = 4 * a.C4; a.stride = c.stride; a.cout = c.cout; a.lrelu = lrelu ? 1 : 0;
    const int BN = bn_of(c.cout);
    const int BM = rows_of(a.M, c.cout / BN);
    const long nblk = (a.M + BM - 1) / BM * (c.cout / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "patch discriminator: conv grid of %ld workgroups", nblk);
    const dim3 grid((unsigned)nblk);
    if (BM == 128) {
        if (BN == 64) hipLaunchKernelGGL((pd_conv_kernel<4, 2>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((pd_conv_kernel<2, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((pd_conv_kernel<1, 2>), grid, dim3(256), 0, st, a);
    } else {
        if (BN == 64) hipLaunchKernelGGL((pd_conv_kernel<4, 1>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((pd_conv_kernel<2, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((pd_conv_kernel<1, 1>), grid, dim3(256), 0, st, a);
    }
    PD_LAUNCHED();
    return I2V_OK;
}

int launch_dgrad(const PdConv& c, const float* g, const float* act, const float* scale, const float* wd, float* out, bool frames, int N, const PdMap& mp,
                 hipStream_t st) {
    PdDgradArgs a{};
    a.g = g; a.act = act; a.scale = scale; a.wd = wd; a.out = out;
    a.N = N; a.Hi = mp.hi; a.Wi = mp.wi; a.Ho = mp.ho; a.Wo = mp.wo;
    a.cout = c.cout; a.C4o = c.cout / 4; a.stride = c.stride; a.cin = c.cin == 3 && !frames ? 4 : c.cin; a.cind = c.cind; a.frames = frames ? 1 : 0;
    const int BN = bn_of(c.cind);
    const long mc = c.stride == 2 ? (long)N * ((mp.hi + 1) / 2) * ((mp.wi + 1) / 2) : mp.mi;   // the largest parity class
    const int BM = rows_of(mc * (c.stride == 2 ? 4 : 1), c.cind / BN);
    const long nblk = (mc + BM - 1) / BM * (c.cind / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "patch discriminator: dgrad grid of %ld workgroups", nblk);
    const dim3 grid((unsigned)nblk, c.stride == 2 ? 4 : 1);
    if (BM == 128) {
        if (BN == 64) hipLaunchKernelGGL((pd_dgrad_kernel<4, 2>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((pd_dgrad_kernel<2, 2>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((pd_dgrad_kernel<1, 2>), grid, dim3(256), 0, st, a);
    } else {
        if (BN == 64) hipLaunchKernelGGL((pd_dgrad_kernel<4, 1>), grid, dim3(256), 0, st, a);
        else if (BN == 32) hipLaunchKernelGGL((pd_dgrad_kernel<2, 1>), grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL((pd_dgrad_kernel<1, 1>), grid, dim3(256), 0, st, a);
    }
    PD_LAUNCHED();
    return I2V_OK;
}

template <int MT>
void launch_wgrad_nt(int nt, dim3 grid, hipStream_t st, const PdWgradArgs& a) {
    if (nt == 4) hipLaunchKernelGGL((pd_wgrad_kernel<MT, 4>), grid, dim3(256), 0, st, a);
    else if (nt == 2) hipLaunchKernelGGL((pd_wgrad_kernel<MT, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pd_wgrad_kernel<MT, 1>), grid, dim3(256), 0, st, a);
}

size_t wgrad_part_floats(const PdConv& c, long P) {
    int S, L;
    pd_wgrad_plan(c.cout, c.cin, P, &S, &L);
    return (size_t)S * 16 * c.cout * (c.cout == 1 ? c.cin : align_up(c.cinp, 16));
}
size_t finish_blocks(const PdConv& c) { return ((size_t)c.cout * c.cin * 16 + 255) / 256; }

// partial sums -> dwn -> grad (written or accumulated): g masked and scaled as in the dgrad
int launch_wgrad(const PdConv& c, const float* g, const float* act, const float* scale, const float* x, const float* w, const float* u, const float* v,
                 const float* sigma, float* part, float* dwn, double* dotp, float* grad, bool accumulate, const PdMap& mp, hipStream_t st) {
    int S, L;
    pd_wgrad_plan(c.cout, c.cin, mp.mo, &S, &L);
    PdFinishArgs f{};
    if (c.cout == 1) {
        hipLaunchKernelGGL(pd_head_wgrad_kernel, dim3((c.cin + 255) / 256, 16, S), dim3(256), 0, st, g, x, part, mp.mo, mp.hi, mp.wi, c.cin, L);
        f.CP = c.cin;
    } else {
        PdWgradArgs a{};
        a.g = g; a.act = act; a.scale = scale; a.x = x; a.part = part; a.P = mp.mo;
        a.Hi = mp.hi; a.Wi = mp.wi; a.Ho = mp.ho; a.Wo = mp.wo; a.cinp = c.cinp; a.cout = c.cout; a.CP = (int)align_up(c.cinp, 16);
        a.stride = c.stride; a.slice_len = L;
        const int mt = bn_of(c.cout) / 16, nt = bn_of(a.CP) / 16;
        const dim3 grid((unsigned)((c.cout / (16 * mt)) * (a.CP / (16 * nt))), 16, (unsigned)S);
        if (mt == 4) launch_wgrad_nt<4>(nt, grid, st, a);
        else if (mt == 2) launch_wgrad_nt<2>(nt, grid, st, a);
        else launch_wgrad_nt<1>(nt, grid, st, a);
        f.CP = a.CP;
    }
    PD_LAUNCHED();
    f.part = part; f.w = w; f.u = u; f.v = v; f.sigma = sigma; f.dwn = dwn; f.dotp = dotp; f.grad = grad;
    f.E = (long)c.cout * c.cin * 16; f.S = S; f.cout = c.cout; f.cin = c.cin; f.nblk = (int)finish_blocks(c); f.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(pd_finish_a_kernel, dim3(f.nblk), dim3(256), 0, st, f);
    PD_LAUNCHED();
    hipLaunchKernelGGL(pd_finish_b_kernel, dim3(f.nblk), dim3(256), 0, st, f);
    PD_LAUNCHED();
    return I2V_OK;
}

constexpr int PD_CHAN_SLICES = 64;
size_t chan_partial_bytes(int C) { return (size_t)PD_CHAN_SLICES * C * 2 * 8; }

int launch_chan_grads(const float* g, const float* act, const float* pre, const float* loc, const float* scale, float* dbias, float* dloc, float* dscale,
                      double* partial, long M, int C, bool accumulate, hipStream_t st) {
    const int R = (int)std::min<long>(std::max<long>((M + 1023) / 1024, 1), PD_CHAN_SLICES);
    PdChanArgs a{g, act, pre, loc, scale, dbias, dloc, dscale, partial, M, (M + R - 1) / R, C, R, accumulate ? 1 : 0};
    hipLaunchKernelGGL(pd_chan_partial_kernel, dim3(C >= 16 ? C / 16 : C, R), dim3(256), 0, st, a);
    PD_LAUNCHED();
    hipLaunchKernelGGL(pd_chan_final_kernel, dim3((C + 255) / 256), dim3(256), 0, st, a);
    PD_LAUNCHED();
    return I2V_OK;
}

int launch_pack(const PdPackArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(pd_pack_kernel, dim3(grid_for(a.total)), dim3(256), 0, st, a);
    PD_LAUNCHED();
    return I2V_OK;
}

PdConv make_conv(int cin, int cout, int stride, int actnorm, int lrelu, int key) {
    return PdConv{cin, cin == 3 ? 4 : cin, cin == 3 ? 16 : cin, cout, stride, actnorm, lrelu, key};
}
PdMap make_map(int n, int hi, int wi, int stride) {
    PdMap m{};
    m.hi = hi; m.wi = wi; m.ho = (hi + 2 - 4) / stride + 1; m.wo = (wi + 2 - 4) / stride + 1;
    if (hi < 2) m.ho = 0;
    if (wi < 2) m.wo = 0;
    m.mi = (long)n * hi * wi; m.mo = (long)n * m.ho * m.wo;
    return m;
}
size_t pack_elems(const PdConv& c) { return (size_t)c.cout * c.cind * 16; }

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_patchdisc {
    int device = 0;
    bool loaded = false;   // parameters bound
    bool have_grads = false;
    int nconv = 0, sn = 1;
    PdConv L[PD_MAXCONV];
    float *w[PD_MAXCONV] = {}, *b[PD_MAXCONV] = {}, *u[PD_MAXCONV] = {}, *v[PD_MAXCONV] = {}, *loc[PD_MAXCONV] = {}, *scale[PD_MAXCONV] = {};
    float *gw[PD_MAXCONV] = {}, *gb[PD_MAXCONV] = {}, *gloc[PD_MAXCONV] = {}, *gscale[PD_MAXCONV] = {};
};

namespace {

// Where everything lies for one input shape: `saved` (offsets from its base) and the workspace
struct PdLayout {
    bool ok = false;
    PdMap map[PD_MAXCONV];
    size_t x4 = 0, act[PD_MAXCONV] = {}, pre[PD_MAXCONV] = {}, wf[PD_MAXCONV] = {}, wd[PD_MAXCONV] = {}, sigma[PD_MAXCONV] = {}, us[PD_MAXCONV] = {},
           vs[PD_MAXCONV] = {}, saved_total = 0;
    size_t pi_t[PD_MAXCONV] = {}, pi_s[PD_MAXCONV] = {}, fwd = 0, ga = 0, gb = 0, part = 0, dwn = 0, dotp = 0, chan = 0, ws_total = 0;
};

PdLayout pd_layout(const i2v_patchdisc* d, int n, int h, int w) {
    PdLayout y;
    if (n <= 0 || h <= 0 || w <= 0) return y;
    int hi = h, wi = w;
    for (int i = 0; i < d->nconv; ++i) {
        y.map[i] = make_map(n, hi, wi, d->L[i].stride);
        if (y.map[i].ho < 1 || y.map[i].wo < 1) return y;
        hi = y.map[i].ho; wi = y.map[i].wo;
    }
    Carver s;
    y.x4 = s.take_floats((size_t)y.map[0].mi * 4);
    size_t gmax = 0, pmax = 0, emax = 0, bmax = 0, cmax = 0;
    for (int i = 0; i < d->nconv; ++i) {
        const PdConv& c = d->L[i];
        if (i + 1 < d->nconv) {
            y.act[i] = s.take_floats((size_t)y.map[i].mo * c.cout);
            y.pre[i] = s.take_floats(c.actnorm ? (size_t)y.map[i].mo * c.cout : 0);
            gmax = std::max(gmax, (size_t)y.map[i].mo * c.cout);
        }
        y.wf[i] = s.take_floats((size_t)16 * c.cout * c.cinp);
        y.wd[i] = s.take_floats(c.cout == 1 ? 0 : pack_elems(c));
        y.sigma[i] = s.take_floats(1);
        y.us[i] = s.take_floats(c.cout);
        y.vs[i] = s.take_floats((size_t)c.cin * 16);
        pmax = std::max(pmax, wgrad_part_floats(c, y.map[i].mo));
        emax = std::max(emax, (size_t)c.cout * c.cin * 16);
        bmax = std::max(bmax, finish_blocks(c));
        cmax = std::max(cmax, chan_partial_bytes(c.cout));
    }
    y.saved_total = s.total();
    Carver k;
    for (int i = 0; i < d->nconv; ++i) {
        y.pi_t[i] = k.take_bytes((size_t)d->L[i].cin * 16 * 8);
        y.pi_s[i] = k.take_bytes((size_t)d->L[i].cout * 8);
    }
    y.fwd = k.take_bytes(y.saved_total);
    y.ga = k.take_floats(gmax);
    y.gb = k.take_floats(gmax);
    y.part = k.take_floats(pmax);
    y.dwn = k.take_floats(emax);
    y.dotp = k.take_bytes(bmax * 8);
    y.chan = k.take_bytes(cmax);
    y.ws_total = k.total();
    y.ok = true;
    return y;
}

int check_unit(const char* what, int n, int hi, int wi, int cin, int cout, int stride) {
    I2V_REQUIRE(n > 0 && hi >= 2 && wi >= 2 && (stride == 1 || stride == 2), I2V_E_INVALID, "%s: n %d, map %d x %d, stride %d", what, n, hi, wi, stride);
    I2V_REQUIRE((cin == 3 || (cin > 0 && cin % 16 == 0)) && cout > 0 && cout % 16 == 0, I2V_E_INVALID,
                "%s: cin %d (3 or a multiple of 16), cout %d (a multiple of 16)", what, cin, cout);
    const PdMap m = make_map(n, hi, wi, stride);
    I2V_REQUIRE(m.ho >= 1 && m.wo >= 1, I2V_E_INVALID, "%s: a %d x %d map leaves no output", what, hi, wi);
    return I2V_OK;
}

// workspace of the unit entries: wf, wd, part, dwn, dotp, the power iteration's t and s
struct PdUnitWs { size_t wf, wd, part, dwn, dotp, chan, t, s, sig, total; };
PdUnitWs unit_ws(int n, int hi, int wi, int cin, int cout) {
    const PdConv c = make_conv(cin, cout, 1, 0, 0, 0);
    const PdMap m = make_map(n, hi, wi, 1);   // stride 1 has the most positions
    Carver k;
    PdUnitWs y{};
    y.wf = k.take_floats((size_t)16 * cout * c.cinp);
    y.wd = k.take_floats(pack_elems(c));
    y.part = k.take_floats(wgrad_part_floats(c, std::max<long>(m.mo, 1)) + wgrad_part_floats(make_conv(cin, cout, 2, 0, 0, 0), std::max<long>(m.mo, 1)));
    y.dwn = k.take_floats((size_t)cout * cin * 16);
    y.dotp = k.take_bytes(finish_blocks(c) * 8);
    y.chan = k.take_bytes(chan_partial_bytes(cout));
    y.t = k.take_bytes((size_t)cin * 16 * 8);
    y.s = k.take_bytes((size_t)cout * 8);
    y.sig = k.take_floats(1);
    y.total = k.total();
    return y;
}

// workspace of the head unit, from the cout = 1 conv's own plan
PdUnitWs head_ws(int n, int hi, int wi, int cin) {
    const PdConv c = make_conv(cin, 1, 1, 0, 0, 0);
    Carver k;
    PdUnitWs y{};
    y.wf = k.take_floats((size_t)16 * cin);
    y.part = k.take_floats(wgrad_part_floats(c, std::max<long>(make_map(n, hi, wi, 1).mo, 1)));
    y.dwn = k.take_floats((size_t)cin * 16);
    y.dotp = k.take_bytes(finish_blocks(c) * 8);
    y.chan = k.take_bytes(chan_partial_bytes(1));
    y.total = k.total();
    return y;
}

int pack_unit(const PdConv& c, const float* weight, float* wf, float* wd, hipStream_t st) {
    PdPackArgs p{};
    p.nconv = 1; p.total = (long)pack_elems(c);
    p.c[0] = PdPackConv{weight, nullptr, wf, wd, c.cout, c.cin, c.cinp, c.cind, 0};
    return launch_pack(p, st);
}

}  // namespace

extern "C" {

int i2v_patchdisc_create(const i2v_patchdisc_cfg* cfg, i2v_patchdisc** out) {
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "i2v_patchdisc_create: null argument");
    I2V_REQUIRE(cfg->use_actnorm, I2V_E_INVALID, "i2v_patchdisc_create: use_actnorm = 0 (BatchNorm2d) is not built");
    I2V_REQUIRE(cfg->in_channels == 3, I2V_E_INVALID, "i2v_patchdisc_create: in_channels %d (only 3 is built)", cfg->in_channels);
    I2V_REQUIRE(cfg->ndf > 0 && cfg->ndf % 16 == 0, I2V_E_INVALID, "i2v_patchdisc_create: ndf %d is not a multiple of 16", cfg->ndf);
    I2V_REQUIRE(cfg->n_layers >= 1 && cfg->n_layers <= PD_MAXCONV - 2, I2V_E_INVALID, "i2v_patchdisc_create: n_layers %d outside 1..%d", cfg->n_layers,
                PD_MAXCONV - 2);
    const i2v_patchdisc_cfg c = *cfg;
    return create_handle("i2v_patchdisc_create", out, [c](i2v_patchdisc* d) {
        d->sn = c.spectral_norm ? 1 : 0;
        int k = 0, mult = 1;
        d->L[k++] = make_conv(3, c.ndf, 2, 0, 1, 0);
        for (int n = 1; n <= c.n_layers; ++n) {
            const int prev = mult;
            mult = std::min(1 << n, 8);
            d->L[k++] = make_conv(c.ndf * prev, c.ndf * mult, n < c.n_layers ? 2 : 1, 1, 1, 2 + 3 * (n - 1));
        }
        d->L[k++] = make_conv(c.ndf * mult, 1, 1, 0, 0, 2 + 3 * c.n_layers);
        d->nconv = k;
        return I2V_OK;
    });
}

void i2v_patchdisc_destroy(i2v_patchdisc* d) { delete d; }

// the device pointer under `key`, or null with the error set
static bool bound_ptr(const StateDict& s, const std::string& key, int64_t numel, float** out) {
    const float* p = s.f32(key, numel);
    *out = const_cast<float*>(p);
    return p != nullptr;
}

int i2v_patchdisc_bind(i2v_patchdisc* d, const i2v_tensor* params, int32_t n) {
    I2V_REQUIRE(d && params && n > 0, I2V_E_INVALID, "i2v_patchdisc_bind: null argument");
    d->loaded = false;
    const StateDict sd(params, n);
    for (int i = 0; i < d->nconv; ++i) {
        const PdConv& c = d->L[i];
        const std::string m = "main." + std::to_string(c.key);
        if (!bound_ptr(sd, m + (d->sn ? ".weight_orig" : ".weight"), (int64_t)c.cout * c.cin * 16, &d->w[i]) || !bound_ptr(sd, m + ".bias", c.cout, &d->b[i]))
            return I2V_E_MISSING;
        if (d->sn && (!bound_ptr(sd, m + ".weight_u", c.cout, &d->u[i]) || !bound_ptr(sd, m + ".weight_v", (int64_t)c.cin * 16, &d->v[i]))) return I2V_E_MISSING;
        if (c.actnorm) {
            const std::string a = "main." + std::to_string(c.key + 1);
            if (!bound_ptr(sd, a + ".loc", c.cout, &d->loc[i]) || !bound_ptr(sd, a + ".scale", c.cout, &d->scale[i])) return I2V_E_MISSING;
        }
    }
    d->loaded = true;
    return I2V_OK;
}

int i2v_patchdisc_bind_grads(i2v_patchdisc* d, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(d && (grads ? n > 0 : n == 0), I2V_E_INVALID, "i2v_patchdisc_bind_grads: null handle, or a count without tensors");
    d->have_grads = false;
    if (!grads) return I2V_OK;
    const StateDict gd(grads, n);
    for (int i = 0; i < d->nconv; ++i) {
        const PdConv& c = d->L[i];
        const std::string m = "main." + std::to_string(c.key);
        if (!bound_ptr(gd, m + (d->sn ? ".weight_orig" : ".weight"), (int64_t)c.cout * c.cin * 16, &d->gw[i]) || !bound_ptr(gd, m + ".bias", c.cout, &d->gb[i]))
            return I2V_E_MISSING;
        if (c.actnorm) {
            const std::string a = "main." + std::to_string(c.key + 1);
            if (!bound_ptr(gd, a + ".loc", c.cout, &d->gloc[i]) || !bound_ptr(gd, a + ".scale", c.cout, &d->gscale[i])) return I2V_E_MISSING;
        }
    }
    d->have_grads = true;
    return I2V_OK;
}

int i2v_patchdisc_out_shape(const i2v_patchdisc* d, int32_t h, int32_t w, int32_t* ho, int32_t* wo) {
    I2V_REQUIRE(d && ho && wo, I2V_E_INVALID, "i2v_patchdisc_out_shape: null argument");
    const PdLayout y = pd_layout(d, 1, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "i2v_patchdisc_out_shape: a %d x %d input shrinks below a 1 x 1 output", h, w);
    *ho = y.map[d->nconv - 1].ho; *wo = y.map[d->nconv - 1].wo;
    return I2V_OK;
}

size_t i2v_patchdisc_saved_bytes(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w) { return d ? pd_layout(d, n, h, w).saved_total : 0; }
size_t i2v_patchdisc_workspace_bytes(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w) { return d ? pd_layout(d, n, h, w).ws_total : 0; }

int i2v_patchdisc_saved_layout(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w, int32_t* nconv, int32_t* ho, int32_t* wo, int32_t* cout,
                               int64_t* act_offset, int64_t* pre_offset) {
    I2V_REQUIRE(d && nconv && ho && wo && cout && act_offset && pre_offset, I2V_E_INVALID, "i2v_patchdisc_saved_layout: null argument");
    const PdLayout y = pd_layout(d, n, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "i2v_patchdisc_saved_layout: a %d x %d input (batch %d) shrinks below a 1 x 1 output", h, w, n);
    *nconv = d->nconv;
    for (int i = 0; i < d->nconv; ++i) {
        ho[i] = y.map[i].ho; wo[i] = y.map[i].wo; cout[i] = d->L[i].cout;
        act_offset[i] = i + 1 < d->nconv ? (int64_t)y.act[i] : -1;
        pre_offset[i] = i + 1 < d->nconv && d->L[i].actnorm ? (int64_t)y.pre[i] : -1;
    }
    return I2V_OK;
}

int i2v_patchdisc_forward(i2v_patchdisc* d, const float* x, int32_t n, int32_t h, int32_t w, int32_t flags, float* pred, void* saved, size_t saved_bytes,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_forward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(x && pred && workspace, I2V_E_INVALID, "%s: null argument", what);
    const PdLayout y = pd_layout(d, n, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: a %d x %d input (batch %d) shrinks below a 1 x 1 output", what, h, w, n);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    const bool save = flags & I2V_PATCHDISC_SAVE, init = flags & I2V_PATCHDISC_INIT_ACTNORM;
    if (save) {
        I2V_REQUIRE(saved, I2V_E_INVALID, "%s: I2V_PATCHDISC_SAVE without a saved buffer", what);
        I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = save ? saved : Carver::at<char>(workspace, y.fwd);
    const int nc = d->nconv;

    float* x4 = Carver::at(sv, y.x4);
    hipLaunchKernelGGL(pd_input4_kernel, dim3(grid_for(y.map[0].mi)), dim3(256), 0, st, x, x4, y.map[0].mi, (long)h * w);
    PD_LAUNCHED();

    PdPackArgs pk{};
    pk.nconv = nc;
    if (d->sn) {
        PdPiArgs pi{};
        pi.nconv = nc; pi.iterate = flags & I2V_PATCHDISC_ITERATE ? 1 : 0;
        for (int i = 0; i < nc; ++i) {
            const PdConv& c = d->L[i];
            pi.c[i] = PdPiConv{d->w[i], d->u[i], d->v[i], Carver::at(sv, y.sigma[i]), Carver::at(sv, y.us[i]), Carver::at(sv, y.vs[i]),
                               Carver::at<double>(workspace, y.pi_t[i]), Carver::at<double>(workspace, y.pi_s[i]), c.cout, c.cin * 16, pi.btotal, pi.rtotal};
            pi.btotal += (c.cin * 16 + 63) / 64; pi.rtotal += c.cout;
        }
        if (int rc = launch_power_iteration(pi, st)) return rc;
    }
    for (int i = 0; i < nc; ++i) {
        const PdConv& c = d->L[i];
        pk.c[i] = PdPackConv{d->w[i], d->sn ? Carver::at(sv, y.sigma[i]) : nullptr, Carver::at(sv, y.wf[i]), c.cout == 1 ? nullptr : Carver::at(sv, y.wd[i]),
                             c.cout, c.cin, c.cinp, c.cind, pk.total};
        pk.total += (long)pack_elems(c);
    }
    if (int rc = launch_pack(pk, st)) return rc;

    const float* in = x4;
    for (int i = 0; i + 1 < nc; ++i) {
        const PdConv& c = d->L[i];
        float* act = Carver::at(sv, y.act[i]);
        float* pre = c.actnorm && (save || init) ? Carver::at(sv, y.pre[i]) : nullptr;
        if (c.actnorm && init) {
            if (int rc = launch_conv(c, in, Carver::at(sv, y.wf[i]), d->b[i], nullptr, nullptr, nullptr, pre, n, y.map[i], false, st)) return rc;
            hipLaunchKernelGGL(pd_actnorm_init_kernel, dim3(c.cout / 4), dim3(256), 0, st, pre, y.map[i].mo, c.cout, d->loc[i], d->scale[i]);
            PD_LAUNCHED();
            const long total = y.map[i].mo * c.cout;
            hipLaunchKernelGGL(pd_actnorm_apply_kernel, dim3(grid_for(total)), dim3(256), 0, st, pre, d->loc[i], d->scale[i], act, total, c.cout);
            PD_LAUNCHED();
        } else if (int rc = launch_conv(c, in, Carver::at(sv, y.wf[i]), d->b[i], c.actnorm ? d->loc[i] : nullptr, c.actnorm ? d->scale[i] : nullptr, act,
                                        pre, n, y.map[i], c.lrelu, st)) {
            return rc;
        }
        in = act;
    }
    const PdMap& hm = y.map[nc - 1];
    hipLaunchKernelGGL(pd_head_fwd_kernel, dim3((unsigned)((hm.mo + 3) / 4)), dim3(256), 0, st, in, Carver::at(sv, y.wf[nc - 1]), d->b[nc - 1], pred, hm.mo,
                       hm.hi, hm.wi, d->L[nc - 1].cin);
    PD_LAUNCHED();
    return I2V_OK;
}

int i2v_patchdisc_backward(i2v_patchdisc* d, const float* d_pred, const void* saved, size_t saved_bytes, int32_t n, int32_t h, int32_t w, float* d_x,
                           int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_backward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(d_pred && saved && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(d_x || param_grads, I2V_E_INVALID, "%s: neither the input gradient nor the parameter gradients are asked for", what);
    I2V_REQUIRE(!param_grads || d->have_grads, I2V_E_STATE, "%s: no gradient tensors are bound", what);
    const PdLayout y = pd_layout(d, n, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: a %d x %d input (batch %d) shrinks below a 1 x 1 output", what, h, w, n);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = const_cast<void*>(saved);
    const int nc = d->nconv;
    const bool acc = accumulate != 0;
    float* part = Carver::at(workspace, y.part);
    float* dwn = Carver::at(workspace, y.dwn);
    double* dotp = Carver::at<double>(workspace, y.dotp);
    double* chan = Carver::at<double>(workspace, y.chan);
    float* ga = Carver::at(workspace, y.ga);
    float* gb = Carver::at(workspace, y.gb);
    auto snap = [&](int i, const float** u, const float** v, const float** sg) {
        *u = d->sn ? Carver::at(sv, y.us[i]) : nullptr; *v = d->sn ? Carver::at(sv, y.vs[i]) : nullptr; *sg = d->sn ? Carver::at(sv, y.sigma[i]) : nullptr;
    };
    const float *us, *vs, *sg;

    // the head
    {
        const int i = nc - 1;
        const PdConv& c = d->L[i];
        const float* xin = Carver::at(sv, y.act[i - 1]);
        if (param_grads) {
            if (int rc = launch_chan_grads(d_pred, nullptr, nullptr, nullptr, nullptr, d->gb[i], nullptr, nullptr, chan, y.map[i].mo, 1, acc, st)) return rc;
            snap(i, &us, &vs, &sg);
            if (int rc = launch_wgrad(c, d_pred, nullptr, nullptr, xin, d->w[i], us, vs, sg, part, dwn, dotp, d->gw[i], acc, y.map[i], st)) return rc;
        }
        const long total = y.map[i].mi * c.cin;
        hipLaunchKernelGGL(pd_head_dgrad_kernel, dim3(grid_for(total)), dim3(256), 0, st, d_pred, Carver::at(sv, y.wf[i]), ga, total, y.map[i].hi, y.map[i].wi,
                           c.cin);
        PD_LAUNCHED();
    }
    for (int i = nc - 2; i >= 0; --i) {
        const PdConv& c = d->L[i];
        const float* act = Carver::at(sv, y.act[i]);
        const float* scale = c.actnorm ? d->scale[i] : nullptr;
        const float* xin = i == 0 ? Carver::at(sv, y.x4) : Carver::at(sv, y.act[i - 1]);
        if (param_grads) {
            if (int rc = launch_chan_grads(ga, act, c.actnorm ? Carver::at(sv, y.pre[i]) : nullptr, c.actnorm ? d->loc[i] : nullptr, scale, d->gb[i],
                                           d->gloc[i], d->gscale[i], chan, y.map[i].mo, c.cout, acc, st))
                return rc;
            snap(i, &us, &vs, &sg);
            if (int rc = launch_wgrad(c, ga, act, scale, xin, d->w[i], us, vs, sg, part, dwn, dotp, d->gw[i], acc, y.map[i], st)) return rc;
        }
        if (i == 0 && !d_x) break;
        if (int rc = launch_dgrad(c, ga, act, scale, Carver::at(sv, y.wd[i]), i == 0 ? d_x : gb, i == 0, n, y.map[i], st)) return rc;
        std::swap(ga, gb);
    }
    return I2V_OK;
}

int i2v_patchdisc_hinge(const float* fake, const float* real, int64_t numel, int32_t mode, double* out, float* d_fake, float* d_real, void* stream) {
    I2V_REQUIRE(fake && out && numel > 0 && (mode == I2V_HINGE_GEN || (mode == I2V_HINGE_DISC && real)), I2V_E_INVALID,
                "i2v_patchdisc_hinge: null argument, numel %lld or mode %d", (long long)numel, mode);
    hipLaunchKernelGGL(pd_hinge_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), fake, real, (long)numel, mode, out, d_fake, d_real);
    PD_LAUNCHED();
    return I2V_OK;
}

int i2v_patchdisc_wgrad_plan(int32_t cout, int32_t cin, int64_t positions, int32_t* slices, int32_t* slice_len) {
    I2V_REQUIRE(slices && slice_len && positions > 0 && (cout == 1 || (cout > 0 && cout % 16 == 0)) && (cin == 3 || (cin > 0 && cin % 16 == 0)), I2V_E_INVALID,
                "i2v_patchdisc_wgrad_plan: cout %d, cin %d, %lld positions", cout, cin, (long long)positions);
    pd_wgrad_plan(cout, cin, positions, slices, slice_len);
    return I2V_OK;
}

size_t i2v_patchdisc_unit_workspace_bytes(int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout) {
    if (n <= 0 || hi < 2 || wi < 2 || cin <= 0 || cout <= 0) return 0;
    return cout == 1 ? head_ws(n, hi, wi, cin).total : unit_ws(n, hi, wi, cin, cout).total;
}

int i2v_patchdisc_conv_unit(const float* x, const float* weight, const float* bias, const float* loc, const float* scale, int32_t n, int32_t hi, int32_t wi,
                            int32_t cin, int32_t cout, int32_t stride, int32_t lrelu, float* out, float* pre, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const char* what = "i2v_patchdisc_conv_unit";
    if (int rc = check_unit(what, n, hi, wi, cin, cout, stride)) return rc;
    I2V_REQUIRE(x && weight && bias && (out || pre) && workspace && !loc == !scale, I2V_E_INVALID, "%s: null argument", what);
    const PdUnitWs k = unit_ws(n, hi, wi, cin, cout);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdConv c = make_conv(cin, cout, stride, loc != nullptr, lrelu, 0);
    if (int rc = pack_unit(c, weight, Carver::at(workspace, k.wf), nullptr, st)) return rc;
    return launch_conv(c, x, Carver::at(workspace, k.wf), bias, loc, scale, out, pre, n, make_map(n, hi, wi, stride), lrelu != 0, st);
}

int i2v_patchdisc_dgrad_unit(const float* g, const float* weight, const float* act, const float* scale, int32_t n, int32_t hi, int32_t wi, int32_t cin,
                             int32_t cout, int32_t stride, float* out, int32_t frames_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_dgrad_unit";
    if (int rc = check_unit(what, n, hi, wi, cin, cout, stride)) return rc;
    I2V_REQUIRE(g && weight && out && workspace && (!frames_out || cin == 3), I2V_E_INVALID, "%s: null argument, or frames_out with cin %d", what, cin);
    const PdUnitWs k = unit_ws(n, hi, wi, cin, cout);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdConv c = make_conv(cin, cout, stride, 0, 0, 0);
    if (int rc = pack_unit(c, weight, Carver::at(workspace, k.wf), Carver::at(workspace, k.wd), st)) return rc;
    return launch_dgrad(c, g, act, scale, Carver::at(workspace, k.wd), out, frames_out != 0, n, make_map(n, hi, wi, stride), st);
}

int i2v_patchdisc_wgrad_unit(const float* g, const float* act, const float* scale, const float* x, const float* weight, const float* u, const float* v,
                             const float* sigma, int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stride, int32_t accumulate,
                             float* dweight, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_wgrad_unit";
    if (int rc = check_unit(what, n, hi, wi, cin, cout, stride)) return rc;
    I2V_REQUIRE(g && x && weight && dweight && dbias && workspace && !u == !v && !u == !sigma, I2V_E_INVALID, "%s: null argument", what);
    const PdUnitWs k = unit_ws(n, hi, wi, cin, cout);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdConv c = make_conv(cin, cout, stride, 0, 0, 0);
    const PdMap mp = make_map(n, hi, wi, stride);
    if (int rc = launch_chan_grads(g, act, nullptr, nullptr, scale, dbias, nullptr, nullptr, Carver::at<double>(workspace, k.chan), mp.mo, cout, accumulate != 0, st)) return rc;
    return launch_wgrad(c, g, act, scale, x, weight, u, v, sigma, Carver::at(workspace, k.part), Carver::at(workspace, k.dwn),
                        Carver::at<double>(workspace, k.dotp), dweight, accumulate != 0, mp, st);
}

int i2v_patchdisc_head_unit(const float* x, const float* weight, const float* bias, const float* g, int32_t n, int32_t hi, int32_t wi, int32_t cin,
                            float* out, float* dx, float* dweight, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_head_unit";
    I2V_REQUIRE(n > 0 && hi >= 2 && wi >= 2 && cin > 0 && cin % 16 == 0, I2V_E_INVALID, "%s: n %d, map %d x %d, cin %d", what, n, hi, wi, cin);
    I2V_REQUIRE(x && weight && bias && out && workspace && (!g || (dx && dweight && dbias)), I2V_E_INVALID, "%s: null argument", what);
    const PdUnitWs k = head_ws(n, hi, wi, cin);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdConv c = make_conv(cin, 1, 1, 0, 0, 0);
    const PdMap mp = make_map(n, hi, wi, 1);
    float* wf = Carver::at(workspace, k.wf);
    if (int rc = pack_unit(c, weight, wf, nullptr, st)) return rc;
    hipLaunchKernelGGL(pd_head_fwd_kernel, dim3((unsigned)((mp.mo + 3) / 4)), dim3(256), 0, st, x, wf, bias, out, mp.mo, hi, wi, cin);
    PD_LAUNCHED();
    if (!g) return I2V_OK;
    if (int rc = launch_chan_grads(g, nullptr, nullptr, nullptr, nullptr, dbias, nullptr, nullptr, Carver::at<double>(workspace, k.chan), mp.mo, 1, false, st)) return rc;
    if (int rc = launch_wgrad(c, g, nullptr, nullptr, x, weight, nullptr, nullptr, nullptr, Carver::at(workspace, k.part), Carver::at(workspace, k.dwn),
                              Carver::at<double>(workspace, k.dotp), dweight, false, mp, st))
        return rc;
    const long total = mp.mi * cin;
    hipLaunchKernelGGL(pd_head_dgrad_kernel, dim3(grid_for(total)), dim3(256), 0, st, g, wf, dx, total, hi, wi, cin);
    PD_LAUNCHED();
    return I2V_OK;
}

int i2v_patchdisc_power_iteration_unit(const float* weight, float* u, float* v, int32_t rows, int32_t cols, int32_t iterate, float* sigma, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_power_iteration_unit";
    I2V_REQUIRE(weight && u && v && sigma && workspace && rows > 0 && cols > 0, I2V_E_INVALID, "%s: null argument or %d x %d", what, rows, cols);
    Carver k;
    const size_t ot = k.take_bytes((size_t)cols * 8), os = k.take_bytes((size_t)rows * 8);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total(), what);
    PdPiArgs pi{};
    pi.nconv = 1; pi.iterate = iterate ? 1 : 0; pi.btotal = (cols + 63) / 64; pi.rtotal = rows;
    pi.c[0] = PdPiConv{weight, u, v, sigma, nullptr, nullptr, Carver::at<double>(workspace, ot), Carver::at<double>(workspace, os), rows, cols, 0, 0};
    return launch_power_iteration(pi, static_cast<hipStream_t>(stream));
}

int i2v_patchdisc_actnorm_init_unit(const float* pre, int64_t m, int32_t c, float* loc, float* scale, void* stream) {
    I2V_REQUIRE(pre && loc && scale && m > 1 && c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_patchdisc_actnorm_init_unit: null argument, %lld rows or %d channels",
                (long long)m, c);
    hipLaunchKernelGGL(pd_actnorm_init_kernel, dim3(c / 4), dim3(256), 0, static_cast<hipStream_t>(stream), pre, (long)m, c, loc, scale);
    PD_LAUNCHED();
    return I2V_OK;
}

}  // extern "C"
