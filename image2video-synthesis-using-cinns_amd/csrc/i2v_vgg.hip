// VGG-16 `features` trunk (torchvision configuration D), the LPIPS layer reduction and the pair reduction of the VGG diversity score.
//
// Replaces stage2_cINN/AE/modules/vgg16.py (vgg16.forward: the five slices up to relu1_2, relu2_2, relu3_3, relu4_3, relu5_3),
// stage2_cINN/AE/modules/LPIPS.py (ScalingLayer, normalize_tensor, the lin layers, spatial_average) and the host path of
// metrics/Diversity/VGG.py (kornia Normalize + Resize, the pair loop with one .cpu().item() per term).
//
// Convolution: 3x3, stride 1, pad 1, bias, ReLU, channels-last [N][H][W][C], exact fp32 on v_mfma_f32_16x16x4_f32.
//   A workgroup owns an 8 x 16 tile of output positions (M = 128; wave w the tile rows 2w and 2w + 1, one 16-row MFMA tile per
//   tile row) and BN = 64 output channels.  Per chunk of CC input channels it stages the 10 x 18 halo of the tile in LDS ONCE; the
//   A operand of tap (dh, dw) is that same image read at pixel offset dh * 18 + dw -- nine taps, one staged image, no per-tap
//   gather from global memory (what flat_conv_kernel does).  The chunk's weights [9][64][CC] are staged next to it.
//   CC = 16: pixel rows of 16 floats padded to 20 (conflict-free ds_read_b128 as in i2v_flatconv.h), A and W double-buffered, the
//   next chunk's global loads in flight under the MFMAs, one barrier per chunk; 2 x (14400 + 46080) + 16 = 120976 bytes of LDS (the 16: one spare float4 for idle staging slots).
//   CC = 4: the first layer, stored (r, g, b, 0): one chunk, K = 36, no padded taps; rows of 4 floats, one float per lane and tap.
//   Loads are unconditional with clamped addresses; the halo outside the map is zero.  The K order of an output element is
//   (chunk, tap, channel): it depends on neither batch nor tile, so batch rows equal their single-image runs bit for bit.  No atomics.
//
// The reductions (lpips_layer, pairdiff) accumulate in float64 in two fixed-order stages: per-workgroup partial sums, then one
// workgroup that adds them in index order.  The grid is a function of the shapes alone: two runs give the same bits.
//
// LPIPS as a loss (stage1_VAE/modules/loss.py: w_percep * LPIPS(seq_orig, seq_gen).mean()): the input gradient of the frozen trunk and of
// the LPIPS head, see "backward (input gradient)" below.
#include <algorithm>
#include <type_traits>

#include "i2v_handle.h"

namespace i2v {
namespace {

// f(0), f(1), ..., f(N - 1) with the index a compile-time constant: register arrays stay registers
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

constexpr int VGG_TH = 8, VGG_TW = 16;          // output tile
constexpr int VGG_HW = VGG_TW + 2;              // halo width (18), halo height 10
constexpr int VGG_HPIX = (VGG_TH + 2) * VGG_HW;  // 180 halo pixels
constexpr int VGG_BN = 64;

constexpr int vgg_ls(int cc) { return cc == 16 ? 20 : cc; }   // floats per staged row of CC
constexpr int vgg_lds_bytes(int cc) { return 2 * (VGG_HPIX + 9 * VGG_BN) * vgg_ls(cc) * 4 + 16; }   // + one float4 that takes the stores of idle staging slots

struct VggConvArgs {
    const float* in;     // [N][H][W][Cin]  (Cin = nchunk * CC)
    const float* wp;     // [nchunk][9][Cout][CC]
    const float* bias;   // [Cout]
    float* out;          // [N][H][W][Cout]
    int H, W, Cin, Cout, nchunk, tilesH, tilesW;
    const float* add;    // VGG_EPI_DGRAD: [N][H][W][Cout] added to the sum, or null
    const float* ymask;  // VGG_EPI_DGRAD: [N][H][W][Cout], the result is kept where it is > 0, or null
};

// Epilogue of vgg_conv_kernel.  FWD: relu(acc + bias), the trunk's forward.  DGRAD: the input gradient of a forward conv run as a
// conv over the output gradient with re-packed weights (dgrad_repack_kernel): no bias, out = (acc + add) * (ymask > 0), both optional.
constexpr int VGG_EPI_FWD = 0, VGG_EPI_DGRAD = 1;

template <int CC, int EPI = VGG_EPI_FWD>
__attribute__((amdgpu_waves_per_eu(1, 2)))   // CC = 16 holds 120960 bytes of LDS: one workgroup per CU, so the registers of two waves per SIMD are free to use
__global__ __launch_bounds__(256) void vgg_conv_kernel(VggConvArgs a) {
    constexpr int LS = vgg_ls(CC);
    constexpr int V = CC / 4;                   // float4 per pixel row = floats per lane and k-slot
    constexpr int A_V4 = VGG_HPIX * V, W_V4 = 9 * VGG_BN * V;
    constexpr int NA = (A_V4 + 255) / 256, NW = (W_V4 + 255) / 256;
    constexpr int A_FLOATS = VGG_HPIX * LS, W_FLOATS = 9 * VGG_BN * LS;
    extern __shared__ __attribute__((aligned(16))) float vgg_lds[];
    float* const a_lds = vgg_lds;                    // [2][A_FLOATS]
    float* const w_lds = vgg_lds + 2 * A_FLOATS;     // [2][W_FLOATS]
    constexpr int DUMP = 2 * W_FLOATS;               // (relative to w_lds; relative to a_lds: 2 A_FLOATS + DUMP) never read

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int nNt = a.Cout / VGG_BN;
    int blk = (int)blockIdx.x;
    const int n0 = (blk % nNt) * VGG_BN; blk /= nNt;
    const int w0 = (blk % a.tilesW) * VGG_TW; blk /= a.tilesW;
    const int h0 = (blk % a.tilesH) * VGG_TH;
    const int img = blk / a.tilesH;

    // the staged pieces of this thread, fixed over the chunks: halo pixel -> input offset (0 and a zero value outside the map)
    long aoff[NA]; bool aok[NA]; int adst[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int idx = tid + 256 * j;
        const int p = idx / V, q = idx - p * V;
        const int hr = p / VGG_HW, hc = p - hr * VGG_HW;
        const int h = h0 - 1 + hr, w = w0 - 1 + hc;
        aok[j] = idx < A_V4 && (unsigned)h < (unsigned)a.H && (unsigned)w < (unsigned)a.W;
        aoff[j] = aok[j] ? (((long)img * a.H + h) * a.W + w) * a.Cin + 4 * q : 0;
        adst[j] = idx < A_V4 ? p * LS + 4 * q : -1;   // -1: an idle slot (the last piece of some threads)
    }
    long woff[NW]; int wdst[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int idx = tid + 256 * j;
        const bool ok = idx < W_V4;
        const int tap = ok ? idx / (VGG_BN * V) : 0, rem = ok ? idx - tap * (VGG_BN * V) : 0;
        woff[j] = ((long)tap * a.Cout + n0) * CC + 4 * rem;
        wdst[j] = ok ? (tap * VGG_BN + rem / V) * LS + 4 * (rem % V) : -1;
    }

    f32x4 pa[NA], pw[NW];   // (native vectors: arrays of the float4 struct do not leave scratch)
    auto request = [&](int ch) {
        static_for<0, NA>([&](auto J) {
            constexpr int j = decltype(J)::value;
            const f32x4 v = *reinterpret_cast<const f32x4*>(a.in + (aok[j] ? aoff[j] + ch * CC : 0));
            pa[j] = aok[j] ? v : f32x4{0.f, 0.f, 0.f, 0.f};
        });
        const float* wsrc = a.wp + (long)ch * 9 * a.Cout * CC;
        static_for<0, NW>([&](auto J) {
            constexpr int j = decltype(J)::value;
            pw[j] = *reinterpret_cast<const f32x4*>(wsrc + woff[j]);
        });
    };
    auto park = [&](int buf) {
        static_for<0, NA>([&](auto J) {
            constexpr int j = decltype(J)::value;
            *reinterpret_cast<f32x4*>(&a_lds[adst[j] >= 0 ? buf * A_FLOATS + adst[j] : 2 * A_FLOATS + DUMP]) = pa[j];
        });
        static_for<0, NW>([&](auto J) {
            constexpr int j = decltype(J)::value;
            *reinterpret_cast<f32x4*>(&w_lds[wdst[j] >= 0 ? buf * W_FLOATS + wdst[j] : DUMP]) = pw[j];
        });
    };

    f32x4 acc[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    request(0);
    park(0);
    __syncthreads();
    for (int ch = 0; ch < a.nchunk; ++ch) {
        const int buf = ch & 1;
        request(ch + 1 < a.nchunk ? ch + 1 : ch);
        const float* al = a_lds + buf * A_FLOATS + V * kq;
        const float* wl = w_lds + buf * W_FLOATS + V * kq;
        // MFMA k-slot (lane >> 4) of step s carries channel V (lane >> 4) + s of the chunk, for both operands
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dh = tap / 3, dw = tap - 3 * dh;
            float av[2][V], bv[4][V];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const float* p = al + ((2 * wave + mt + dh) * VGG_HW + lr + dw) * LS;
                if constexpr (V == 4) {
                    const float4 t = *reinterpret_cast<const float4*>(p);
                    av[mt][0] = t.x; av[mt][1] = t.y; av[mt][2] = t.z; av[mt][3] = t.w;
                } else {
                    av[mt][0] = *p;
                }
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const float* p = wl + (tap * VGG_BN + 16 * nt + lr) * LS;
                if constexpr (V == 4) {
                    const float4 t = *reinterpret_cast<const float4*>(p);
                    bv[nt][0] = t.x; bv[nt][1] = t.y; bv[nt][2] = t.z; bv[nt][3] = t.w;
                } else {
                    bv[nt][0] = *p;
                }
            }
#pragma unroll
            for (int s = 0; s < V; ++s)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][s], bv[nt][s], acc[mt][nt], 0, 0, 0);
        }
        if (ch + 1 < a.nchunk) park(buf ^ 1);
        __syncthreads();
    }

    // C/D layout of the 16x16 MFMA: column = lane & 15 (output channel), rows 4 (lane >> 4) + r (tile column)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + 16 * nt + lr;
        float b = 0.f;
        if constexpr (EPI == VGG_EPI_FWD) b = a.bias[n];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int ho = h0 + 2 * wave + mt;
            if (ho >= a.H) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int wo = w0 + 4 * kq + r;
                if (wo >= a.W) continue;
                const long o = (((long)img * a.H + ho) * a.W + wo) * a.Cout + n;
                if constexpr (EPI == VGG_EPI_FWD) {
                    a.out[o] = fmaxf(acc[mt][nt][r] + b, 0.f);
                } else {
                    float v = acc[mt][nt][r];
                    if (a.add) v += a.add[o];
                    if (a.ymask) v = a.ymask[o] > 0.f ? v : 0.f;
                    a.out[o] = v;
                }
            }
        }
    }
}

// MaxPool2d(2, 2), floor mode, channels-last: [N][H][W][C] -> [N][H / 2][W / 2][C]; an odd last row / column is dropped
__global__ __launch_bounds__(256) void vgg_maxpool2_kernel(const float* __restrict__ in, float* __restrict__ out, long N, int H, int W, int C) {
    const int C4 = C >> 2, Ho = H >> 1, Wo = W >> 1;
    const long total = N * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % Wo); p /= Wo;
        const int ho = (int)(p % Ho);
        const long n = p / Ho;
        const float* s = in + (((n * H + 2 * ho) * W + 2 * wo) * C) + 4 * c4;
        const float4 v00 = *reinterpret_cast<const float4*>(s), v01 = *reinterpret_cast<const float4*>(s + C);
        const float4 v10 = *reinterpret_cast<const float4*>(s + (long)W * C), v11 = *reinterpret_cast<const float4*>(s + (long)W * C + C);
        float4 m;
        m.x = fmaxf(fmaxf(v00.x, v01.x), fmaxf(v10.x, v11.x));
        m.y = fmaxf(fmaxf(v00.y, v01.y), fmaxf(v10.y, v11.y));
        m.z = fmaxf(fmaxf(v00.z, v01.z), fmaxf(v10.z, v11.z));
        m.w = fmaxf(fmaxf(v00.w, v01.w), fmaxf(v10.w, v11.w));
        *reinterpret_cast<float4*>(out + i * 4) = m;
    }
}

// Input stage: frames [N][3][Hi][Wi] in [-1, 1] -> channels-last [N][Ho][Wo][4] (channel 3 zero).  Every source pixel is normalised
// first, then the four neighbours are blended in the arithmetic of torch's upsample_bilinear2d (the reference's order:
// resize(normalize(x))).  Ho = Hi and Wo = Wi give weights (1, 0): the sample is the normalised pixel itself, exactly.
//   I2V_VGG_INPUT_LPIPS:      (x - shift) / scale, LPIPS.py ScalingLayer
//   I2V_VGG_INPUT_DIVERSITY:  ((x + 1) / 2 - mean) / std, metrics/Diversity/VGG.py:29 + kornia Normalize with the ImageNet constants
__global__ __launch_bounds__(256) void vgg_input_kernel(const float* __restrict__ frames, float* __restrict__ out, long N, int Hi, int Wi, int Ho,
                                                        int Wo, int mode, int align_corners) {
    const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const long total = N * Ho * Wo;
    // area_pixel_compute_scale
    const float sh = align_corners ? (Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f) : (float)Hi / (float)Ho;
    const float sw = align_corners ? (Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f) : (float)Wi / (float)Wo;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i % Wo), h = (int)((i / Wo) % Ho);
        const long n = i / ((long)Wo * Ho);
        // area_pixel_compute_source_index: align_corners scale * dst, else max(scale * (dst + 0.5) - 0.5, 0)
        const float fh = align_corners ? sh * h : fmaxf(sh * (h + 0.5f) - 0.5f, 0.f);
        const float fw = align_corners ? sw * w : fmaxf(sw * (w + 0.5f) - 0.5f, 0.f);
        const int h0 = min((int)fh, Hi - 1), w0 = min((int)fw, Wi - 1);
        const int h1 = h0 + (h0 < Hi - 1 ? 1 : 0), w1 = w0 + (w0 < Wi - 1 ? 1 : 0);
        const float lh1 = fminf(fmaxf(fh - h0, 0.f), 1.f), lh0 = 1.f - lh1, lw1 = fminf(fmaxf(fw - w0, 0.f), 1.f), lw0 = 1.f - lw1;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = frames + (n * 3 + c) * (long)Hi * Wi;
            float s[4] = {pl[(long)h0 * Wi + w0], pl[(long)h0 * Wi + w1], pl[(long)h1 * Wi + w0], pl[(long)h1 * Wi + w1]};
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = mode == I2V_VGG_INPUT_LPIPS ? (s[k] - shift[c]) / scale[c] : ((s[k] + 1.0f) / 2.0f - mean[c]) / stdv[c];
            v[c] = lh0 * (lw0 * s[0] + lw1 * s[1]) + lh1 * (lw0 * s[2] + lw1 * s[3]);
        }
        *reinterpret_cast<float4*>(out + i * 4) = make_float4(v[0], v[1], v[2], 0.f);
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {   // fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

constexpr int LPIPS_G = 64;     // partial sums per image
constexpr int PAIR_G = 1024;    // partial sums of the pair reduction
constexpr int PAIR_RMAX = 16;

// LPIPS.forward :44-48 for one layer: f0, f1 [N][P][C] fp32, lin [C].  One wave per position: the C = 64 KC channels of both maps go into
// registers once, the two norms and sum_c w_c (f0 / (|f0| + 1e-10) - f1 / (|f1| + 1e-10))^2 are formed in float64.  Workgroup (n, g) sums
// the positions 4 g + wave, + 4 G, ... of image n in order -> partial[n][g].
template <int KC>
__global__ __launch_bounds__(256) void lpips_partial_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ lin,
                                                            int P, int G, double* __restrict__ partial) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x / G, g = blockIdx.x % G;
    constexpr int C = 64 * KC;
    float w[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) w[k] = lin[lane + 64 * k];
    double s = 0.0;
    for (int p = 4 * g + wave; p < P; p += 4 * G) {
        const float* a = f0 + ((long)n * P + p) * C;
        const float* b = f1 + ((long)n * P + p) * C;
        float x[KC], y[KC];
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            x[k] = a[lane + 64 * k]; y[k] = b[lane + 64 * k];
            sx += (double)x[k] * (double)x[k]; sy += (double)y[k] * (double)y[k];
        }
        const double ix = 1.0 / (sqrt(wave_sum_f64(sx)) + 1e-10), iy = 1.0 / (sqrt(wave_sum_f64(sy)) + 1e-10);
        double d = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const double v = (double)x[k] * ix - (double)y[k] * iy;
            d += (double)w[k] * v * v;
        }
        s += wave_sum_f64(d);
    }
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) partial[(long)n * G + g] = ((red[0] + red[1]) + red[2]) + red[3];
}
// out[n] += (sum_g partial[n][g]) / P: spatial_average
__global__ __launch_bounds__(256) void lpips_final_kernel(const double* __restrict__ partial, int N, int P, int G, double* __restrict__ out) {
    for (int n = threadIdx.x; n < N; n += 256) {
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += partial[(long)n * G + g];
        out[n] += s / (double)P;
    }
}

// metrics/Diversity/VGG.py:38-43 for one group of R feature maps f [R][D]: every element is read once, the R values of index d sit in
// registers and all pairs i < j are formed from them in float64.  Workgroup g sums d = 256 g + tid, + 256 G, ... in order -> partial[g].
__global__ __launch_bounds__(256) void pairdiff_partial_kernel(const float* __restrict__ f, int R, long D, int G, double* __restrict__ partial) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long d = (long)blockIdx.x * 256 + tid; d < D; d += (long)G * 256) {
        float v[PAIR_RMAX];
#pragma unroll
        for (int i = 0; i < PAIR_RMAX; ++i) v[i] = i < R ? f[i * D + d] : 0.f;
#pragma unroll
        for (int i = 0; i < PAIR_RMAX; ++i)
#pragma unroll
            for (int j = i + 1; j < PAIR_RMAX; ++j)
                if (j < R) {
                    const double t = (double)v[i] - (double)v[j];
                    s += t * t;
                }
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = red[0];
}
// acc[0] += 2 (sum_g partial[g]) / D (each unordered pair counts twice: the square is symmetric; .mean() over the map), acc[1] += R (R - 1)
__global__ __launch_bounds__(256) void pairdiff_final_kernel(const double* __restrict__ partial, int G, int R, long D, double* __restrict__ acc) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int g = tid; g < G; g += 256) s += partial[g];
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        acc[0] += 2.0 * red[0] / (double)D;
        acc[1] += (double)R * (R - 1);
    }
}

// ------------------------------------------------------------------------------------------------------------ backward (input gradient)
// The trunk is frozen: only the gradient at the input is formed.  The input gradient of a 3x3 / stride 1 / pad 1 convolution is the same
// convolution over the output gradient with the kernel transposed (Cin <-> Cout) and the taps flipped, so twelve of the thirteen backward
// convolutions are vgg_conv_kernel<16, VGG_EPI_DGRAD> on weights re-packed once per handle (dgrad_repack_kernel).  The first layer
// (64 -> 3) has its own narrow kernel.  Everything else is one fused memory-bound pass per pool (vgg_maxpool2_bwd_kernel: routing, the
// tap gradient that enters there, the ReLU mask), one pass per LPIPS layer (lpips_bwd_kernel) and one masked copy of the relu5_3 gradient.

// forward-packed [nchunk_in][9][Cout][16] -> dgrad-packed [Cout / 16][9 flipped][Cin][16]: element (co, ci, tap) of the forward weight
// sits at tap 8 - tap, "output" channel ci, "input" channel co of the backward convolution
__global__ __launch_bounds__(256) void dgrad_repack_kernel(const float* __restrict__ fwd, float* __restrict__ bwd, int Cin, int Cout) {
    const long total = (long)Cin * Cout * 9;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int cl = (int)(i & 15);
        long r = i >> 4;
        const int ci = (int)(r % Cin); r /= Cin;
        const int tap = (int)(r % 9);
        const int co = (int)(r / 9) * 16 + cl;
        bwd[i] = fwd[(((long)(ci >> 4) * 9 + (8 - tap)) * Cout + co) * 16 + (ci & 15)];
    }
}

// Input gradient of the first layer (3 -> 64 forward): g [N][H][W][64] -> the gradient at the three input channels, K = 9 x 64 = 576 per
// output.  One thread per pixel; the weights [9][64][4] (the FORWARD packing of the CC = 4 layer, read at tap 8 - tap) sit in LDS and every
// lane reads the same address (a broadcast).  The K order is (tap, channel): it depends on neither batch nor grid.
//   nchw = 0: out [N][H][W][4] (channel 3 zero), the gradient at the channels-last input of i2v_vgg_features
//   nchw = 1: out [N][3][H][W], divided by ScalingLayer's scale: the gradient at the frames (the inverse of vgg_input_kernel in LPIPS mode)
__global__ __launch_bounds__(256) void vgg_dgrad_first_kernel(const float* __restrict__ g, const float* __restrict__ wp, float* __restrict__ out,
                                                              long N, int H, int W, int nchw) {
    __shared__ __attribute__((aligned(16))) float wl[9 * 64 * 4];
    for (int i = threadIdx.x; i < 9 * 64; i += 256) *reinterpret_cast<float4*>(&wl[4 * i]) = *reinterpret_cast<const float4*>(wp + 4 * i);
    __syncthreads();
    const float scale[3] = {.458f, .448f, .450f};
    const long total = N * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i % W), h = (int)((i / W) % H);
        const long n = i / ((long)W * H);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 1   // (fully unrolled, the 144 loads of a pixel are hoisted together: 255 VGPRs and scratch)
        for (int tap = 0; tap < 9; ++tap) {
            const int hh = h + tap / 3 - 1, ww = w + tap % 3 - 1;
            if ((unsigned)hh >= (unsigned)H || (unsigned)ww >= (unsigned)W) continue;
            const float* gp = g + ((n * H + hh) * W + ww) * 64;
            const float* wt = wl + (8 - tap) * 256;
#pragma unroll 4
            for (int q = 0; q < 16; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(gp + 4 * q);
                const float gv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 wv = *reinterpret_cast<const float4*>(wt + 4 * (4 * q + k));
                    a0 = fmaf(gv[k], wv.x, a0); a1 = fmaf(gv[k], wv.y, a1); a2 = fmaf(gv[k], wv.z, a2);
                }
            }
        }
        if (nchw) {
            const long plane = (long)H * W, o = n * 3 * plane + (long)h * W + w;
            out[o] = a0 / scale[0]; out[o + plane] = a1 / scale[1]; out[o + 2 * plane] = a2 / scale[2];
        } else {
            *reinterpret_cast<float4*>(out + i * 4) = make_float4(a0, a1, a2, 0.f);
        }
    }
}

// MaxPool2d(2, 2) backward, channels-last, one float4 of one 2 x 2 window per lane: gp [N][H / 2][W / 2][C] (the pooled gradient), y
// [N][H][W][C] (the saved pool input) -> out [N][H][W][C].  The pooled gradient goes to the FIRST maximum of the window in row-major
// order (a later value wins only when it is greater: torch's rule), the other three positions get zero, and so do the dropped last row
// and column of an odd map (the window grid is ceil(H / 2) x ceil(W / 2); an incomplete window routes nothing).  Fused behind the routing:
// + add (the tap gradient that enters at this activation; null: none), then x (y > 0) when relu_mask (y is a post-ReLU activation).
__global__ __launch_bounds__(256) void vgg_maxpool2_bwd_kernel(const float* __restrict__ gp, const float* __restrict__ y, const float* __restrict__ add,
                                                               float* __restrict__ out, long N, int H, int W, int C, int relu_mask) {
    const int C4 = C >> 2, Ho = H >> 1, Wo = W >> 1, Hc = (H + 1) >> 1, Wc = (W + 1) >> 1;
    const long total = N * Hc * Wc * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % Wc); p /= Wc;
        const int ho = (int)(p % Hc);
        const long n = p / Hc;
        const bool full = ho < Ho && wo < Wo;
        const bool ok[4] = {true, 2 * wo + 1 < W, 2 * ho + 1 < H, 2 * wo + 1 < W && 2 * ho + 1 < H};
        long off[4];
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            off[k] = ((n * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1)) * C + 4 * c4;
            v[k] = ok[k] ? *reinterpret_cast<const f32x4*>(y + off[k]) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        f32x4 gv = {0.f, 0.f, 0.f, 0.f};
        if (full) gv = *reinterpret_cast<const f32x4*>(gp + (((n * Ho + ho) * Wo + wo) * C) + 4 * c4);
        int arg[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float best = v[0][e];
            int bi = 0;
#pragma unroll
            for (int k = 1; k < 4; ++k)
                if (v[k][e] > best) { best = v[k][e]; bi = k; }
            arg[e] = full ? bi : -1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!ok[k]) continue;
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = arg[e] == k ? gv[e] : 0.f;
            if (add) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(add + off[k]);
                o += t;
            }
            if (relu_mask) {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = v[k][e] > 0.f ? o[e] : 0.f;
            }
            *reinterpret_cast<f32x4*>(out + off[k]) = o;
        }
    }
}

// out = g x (y > 0): the relu5_3 tap gradient enters the chain behind no pool, so its ReLU mask has no kernel to ride on.  The map is
// the smallest of the trunk ([N][H / 16][W / 16][512]: 1 / 32 of relu1_2's bytes).
__global__ __launch_bounds__(256) void vgg_relu_mask_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ out, long total4) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + 4 * i), yv = *reinterpret_cast<const f32x4*>(y + 4 * i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = yv[e] > 0.f ? gv[e] : 0.f;
        *reinterpret_cast<f32x4*>(out + 4 * i) = o;
    }
}

// Backward of lpips_partial_kernel for one layer: with s = |f| over c, n = f / (s + eps), d = n0 - n1 and out[i] = sum_p sum_c lin d^2 / P,
// an upstream weight u[i] gives dn0 = 2 u[i] / P lin d (dn1 = -dn0) and df = dn / (s + eps) - f (f . dn) / (s (s + eps)^2).  One wave per
// position as in the forward: both feature vectors go into registers once, |f|^2 and f . dn are float64 wave sums, the result is rounded
// to fp32 once.  s = 0 (an all-zero feature vector): the second term is dropped, df = dn / eps (torch's sqrt backward gives NaN there).
// g0 / g1 null: that side's gradient is not written.  No reduction across positions: nothing to order.
template <int KC>
__global__ __launch_bounds__(256) void lpips_bwd_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ lin,
                                                        const double* __restrict__ u, int P, long NP, float* __restrict__ g0, float* __restrict__ g1) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int C = 64 * KC;
    constexpr double eps = 1e-10;
    float w[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) w[k] = lin[lane + 64 * k];
    for (long q = (long)blockIdx.x * 4 + wave; q < NP; q += (long)gridDim.x * 4) {
        const double coef = 2.0 * u[q / P] / (double)P;
        float x[KC], y[KC];
        double sx = 0.0, sy = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            x[k] = f0[q * C + lane + 64 * k]; y[k] = f1[q * C + lane + 64 * k];
            sx += (double)x[k] * (double)x[k]; sy += (double)y[k] * (double)y[k];
        }
        const double s0 = sqrt(wave_sum_f64(sx)), s1 = sqrt(wave_sum_f64(sy));
        const double i0 = 1.0 / (s0 + eps), i1 = 1.0 / (s1 + eps);
        double dn[KC], dx = 0.0, dy = 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            dn[k] = coef * (double)w[k] * ((double)x[k] * i0 - (double)y[k] * i1);
            dx += (double)x[k] * dn[k]; dy += (double)y[k] * dn[k];
        }
        dx = wave_sum_f64(dx); dy = wave_sum_f64(dy);
        const double r0 = s0 > 0.0 ? dx * i0 * i0 / s0 : 0.0, r1 = s1 > 0.0 ? dy * i1 * i1 / s1 : 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (g0) g0[q * C + lane + 64 * k] = (float)(dn[k] * i0 - (double)x[k] * r0);
            if (g1) g1[q * C + lane + 64 * k] = (float)(-(dn[k] * i1 - (double)y[k] * r1));
        }
    }
}

// torchvision vgg16().features: index of every conv, its widths, and whether a tap / a pool follows its ReLU
struct LayerSpec { int idx, cin, cout, tap, pool; };
const LayerSpec VGG_LAYERS[13] = {
    {0, 3, 64, -1, 0},    {2, 64, 64, 0, 1},                             // slice1: relu1_2, then MaxPool (features.4, head of slice2)
    {5, 64, 128, -1, 0},  {7, 128, 128, 1, 1},                           // relu2_2
    {10, 128, 256, -1, 0}, {12, 256, 256, -1, 0}, {14, 256, 256, 2, 1},  // relu3_3
    {17, 256, 512, -1, 0}, {19, 512, 512, -1, 0}, {21, 512, 512, 3, 1},  // relu4_3
    {24, 512, 512, -1, 0}, {26, 512, 512, -1, 0}, {28, 512, 512, 4, 0}}; // relu5_3 (features.30, the last pool, is not part of slice5)
const int VGG_TAP_C[5] = {64, 128, 256, 512, 512};

struct Conv {
    DevBuf w, bias;
    int Cin = 0, CinS = 0, Cout = 0, CC = 16, nchunk = 0;   // CinS: stored input channels (3 -> 4)
    int pack(const float* wsrc, const float* bsrc, int cin, int cout);
};

const char* dgrad_shape_error(int cin, int cout) {
    if (cin == 3) return cout == 64 ? nullptr : "the first-layer form (3 input channels) has 64 output channels";
    if (!(cin > 0 && cin % VGG_BN == 0)) return "forward input channels must be 3 or a multiple of 64 (the backward kernel's output tile)";
    if (!(cout > 0 && cout % 16 == 0)) return "forward output channels must be a multiple of 16 (the backward kernel's chunk)";
    return nullptr;
}

// [Cout][Cin][3][3] -> [Cout / 16][9 flipped][Cin][16]: what dgrad_repack_kernel makes of the forward packing, from raw weights
std::vector<float> pack_dgrad_host(const float* wsrc, int cin, int cout) {
    std::vector<float> p((size_t)cin * cout * 9);
    for (int n = 0; n < cout; ++n)
        for (int c = 0; c < cin; ++c)
            for (int tap = 0; tap < 9; ++tap) p[(((size_t)(n / 16) * 9 + (8 - tap)) * cin + c) * 16 + n % 16] = wsrc[((size_t)n * cin + c) * 9 + tap];
    return p;
}

const char* conv_shape_error(int cin, int cout) {
    if (!(cin == 3 || (cin > 0 && cin % 16 == 0))) return "input channels must be 3 (stored as r, g, b, 0) or a multiple of 16";
    if (!(cout > 0 && cout % VGG_BN == 0)) return "output channels must be a multiple of 64";
    return nullptr;
}

// [Cout][Cin][3][3] -> [nchunk][9][Cout][CC]
int Conv::pack(const float* wsrc, const float* bsrc, int cin, int cout) {
    Cin = cin; Cout = cout;
    CC = cin == 3 ? 4 : 16;
    CinS = cin == 3 ? 4 : cin;
    nchunk = CinS / CC;
    std::vector<float> p((size_t)nchunk * 9 * cout * CC, 0.f);
    for (int n = 0; n < cout; ++n)
        for (int c = 0; c < cin; ++c)
            for (int tap = 0; tap < 9; ++tap) p[(((size_t)(c / CC) * 9 + tap) * cout + n) * CC + c % CC] = wsrc[((size_t)n * cin + c) * 9 + tap];
    return upload_packed(w, bias, p.data(), p.size() * 4, bsrc, cout);
}

int conv_launch(const Conv& c, const float* in, float* out, int N, int H, int W, hipStream_t st) {
    VggConvArgs a{};
    a.in = in; a.wp = c.w.as<float>(); a.bias = c.bias.as<float>(); a.out = out;
    a.H = H; a.W = W; a.Cin = c.CinS; a.Cout = c.Cout; a.nchunk = c.nchunk;
    a.tilesH = (H + VGG_TH - 1) / VGG_TH; a.tilesW = (W + VGG_TW - 1) / VGG_TW;
    const long nblk = (long)N * a.tilesH * a.tilesW * (c.Cout / VGG_BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "vgg conv: grid of %ld workgroups", nblk);
    if (c.CC == 16) {
        static bool done[I2V_MAX_DEV];
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&vgg_conv_kernel<16>), vgg_lds_bytes(16), done)) return rc;
        hipLaunchKernelGGL(vgg_conv_kernel<16>, dim3((unsigned)nblk), dim3(256), vgg_lds_bytes(16), st, a);
    } else {
        hipLaunchKernelGGL(vgg_conv_kernel<4>, dim3((unsigned)nblk), dim3(256), vgg_lds_bytes(4), st, a);
    }
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

// Input gradient of a forward conv cin -> cout: g [N][H][W][cout] -> out [N][H][W][cin] on the forward kernel with the DGRAD epilogue
int dgrad_launch(const float* wb, int cin, int cout, const float* g, float* out, const float* add, const float* ymask, int N, int H, int W,
                 hipStream_t st) {
    VggConvArgs a{};
    a.in = g; a.wp = wb; a.bias = nullptr; a.out = out; a.add = add; a.ymask = ymask;
    a.H = H; a.W = W; a.Cin = cout; a.Cout = cin; a.nchunk = cout / 16;
    a.tilesH = (H + VGG_TH - 1) / VGG_TH; a.tilesW = (W + VGG_TW - 1) / VGG_TW;
    const long nblk = (long)N * a.tilesH * a.tilesW * (cin / VGG_BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "vgg dgrad: grid of %ld workgroups", nblk);
    static bool done[I2V_MAX_DEV];
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&vgg_conv_kernel<16, VGG_EPI_DGRAD>), vgg_lds_bytes(16), done)) return rc;
    hipLaunchKernelGGL((vgg_conv_kernel<16, VGG_EPI_DGRAD>), dim3((unsigned)nblk), dim3(256), vgg_lds_bytes(16), st, a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int dgrad_first_launch(const float* w0, const float* g, float* out, int N, int H, int W, int nchw, hipStream_t st) {
    hipLaunchKernelGGL(vgg_dgrad_first_kernel, dim3(grid_for((long)N * H * W)), dim3(256), 0, st, g, w0, out, (long)N, H, W, nchw);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int pool_bwd_launch(const float* gp, const float* y, const float* add, float* out, int N, int H, int W, int C, int relu_mask, hipStream_t st) {
    hipLaunchKernelGGL(vgg_maxpool2_bwd_kernel, dim3(grid_for((long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 4))), dim3(256), 0, st, gp, y, add, out,
                       (long)N, H, W, C, relu_mask);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int pool_launch(const float* in, float* out, int N, int H, int W, int C, hipStream_t st) {
    hipLaunchKernelGGL(vgg_maxpool2_kernel, dim3(grid_for((long)N * (H / 2) * (W / 2) * (C / 4))), dim3(256), 0, st, in, out, (long)N, H, W, C);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

constexpr long VGG_MAX_FLOATS = 1L << 40;

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_vgg {
    int device = 0;
    bool loaded = false, have_lin = false;
    Conv conv[13];
    DevBuf lin[5];
    DevBuf dgrad_w[13];        // [1..12]: the backward packing, made on the first backward call (inference never pays for it)
    bool dgrad_ready = false;
};

namespace {

// Buffer plan of the trunk: a conv that feeds a tap writes the caller's tap buffer; every other conv writes workspace buffer a, or b
// when it reads a; a pool always writes a (its source is a tap buffer).  vgg_ws_floats sizes a and b by the same rule.
void vgg_ws_floats(int N, int H, int W, size_t* a_floats, size_t* b_floats) {
    size_t af = 0, bf = 0;
    int h = H, w = W;
    bool cur_is_a = false;
    for (int l = 0; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        const size_t of = (size_t)N * h * w * s.cout;
        if (s.tap < 0) {
            if (cur_is_a) bf = std::max(bf, of); else af = std::max(af, of);
            cur_is_a = !cur_is_a;
        } else {
            cur_is_a = false;
        }
        if (s.pool) {
            h /= 2; w /= 2;
            af = std::max(af, (size_t)N * h * w * s.cout);
            cur_is_a = true;
        }
    }
    *a_floats = af; *b_floats = bf;
}

// Saved state of the backward pass: the eight post-ReLU activations that are not taps, in layer order, each 256-byte aligned (the
// five taps stay with the caller).  off[l]: byte offset of layer l (taps: unused); returns the total.
size_t vgg_saved_offsets(int N, int H, int W, size_t* off) {
    size_t total = 0;
    int h = H, w = W;
    for (int l = 0; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        off[l] = total;
        if (s.tap < 0) total += align_up((size_t)N * h * w * s.cout * 4, 256);
        if (s.pool) { h /= 2; w /= 2; }
    }
    return total;
}

// x: channels-last input [N][H][W][4]; a, b: the workspace buffers; saved (or null): where the non-tap activations are kept instead
int vgg_run(const i2v_vgg* v, const float* x, int N, int H, int W, float* const* taps, float* a, float* b, char* saved, hipStream_t st) {
    const float* cur = x;
    int h = H, w = W;
    size_t off[13];
    vgg_saved_offsets(N, H, W, off);
    for (int l = 0; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        float* dst = s.tap >= 0 ? taps[s.tap] : saved ? reinterpret_cast<float*>(saved + off[l]) : cur == a ? b : a;
        if (int rc = conv_launch(v->conv[l], cur, dst, N, h, w, st)) return rc;
        cur = dst;
        if (s.pool) {
            if (int rc = pool_launch(cur, a, N, h, w, s.cout, st)) return rc;
            cur = a;
            h /= 2; w /= 2;
        }
    }
    return I2V_OK;
}

// The backward packing of layers 1..12 (14.7 M floats, 59 MB), made from the forward packing on the device by the first backward call
// of a handle.  That call allocates; every later one only enqueues.  (Layer 0 needs none: vgg_dgrad_first_kernel reads the forward
// packing at the flipped tap.)
int ensure_dgrad(i2v_vgg* v, hipStream_t st) {
    if (v->dgrad_ready) return I2V_OK;
    I2V_REQUIRE(!stream_is_capturing(st), I2V_E_STATE,
                "i2v_vgg_backward: the first backward call of a handle packs the backward weights and cannot be captured; run it once eagerly");
    for (int l = 1; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        DevBuf& d = v->dgrad_w[l];
        d.release();
        const size_t bytes = (size_t)s.cin * s.cout * 9 * 4;
        I2V_HIP_CHECK(hipMalloc(&d.p, bytes));
        d.bytes = bytes;
        hipLaunchKernelGGL(dgrad_repack_kernel, dim3(grid_for((long)s.cin * s.cout * 9)), dim3(256), 0, st, v->conv[l].w.as<float>(), d.as<float>(), s.cin,
                           s.cout);
        I2V_HIP_CHECK(hipGetLastError());
    }
    v->dgrad_ready = true;
    return I2V_OK;
}

bool vgg_dims_ok(int h, int w) { return (h >> 4) > 0 && (w >> 4) > 0; }

}  // namespace

extern "C" {

int i2v_vgg_create(i2v_vgg** out) {
    return create_handle("i2v_vgg_create", out, [](i2v_vgg*) { return I2V_OK; });
}

void i2v_vgg_destroy(i2v_vgg* v) { delete v; }

static int vgg_pack(i2v_vgg* v, const StateDict& sd) {
    v->have_lin = false;
    v->dgrad_ready = false;
    for (int l = 0; l < 13; ++l) v->dgrad_w[l].release();
    for (int l = 0; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        const std::string key = "features." + std::to_string(s.idx);
        const float* w = sd.f32(key + ".weight", (int64_t)s.cout * s.cin * 9);
        const float* b = sd.f32(key + ".bias", s.cout);
        if (!w || !b) return I2V_E_MISSING;
        if (int rc = v->conv[l].pack(w, b, s.cin, s.cout)) return rc;
    }
    if (sd.has("lin0.model.1.weight")) {
        for (int k = 0; k < 5; ++k) {
            const float* w = sd.f32("lin" + std::to_string(k) + ".model.1.weight", VGG_TAP_C[k]);
            if (!w) return I2V_E_MISSING;
            if (int rc = v->lin[k].upload(w, (size_t)VGG_TAP_C[k] * 4)) return rc;
        }
        v->have_lin = true;
    }
    return I2V_OK;
}

int i2v_vgg_load(i2v_vgg* v, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_vgg_load", v, tensors, n_tensors, vgg_pack);
}

const float* i2v_vgg_lin(const i2v_vgg* v, int32_t layer) {
    if (!v || !v->have_lin || layer < 0 || layer >= 5) return nullptr;
    return v->lin[layer].as<float>();
}

size_t i2v_vgg_workspace_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w) {
    if (!v || batch <= 0 || !vgg_dims_ok(h, w)) return 0;
    size_t af, bf;
    vgg_ws_floats(batch, h, w, &af, &bf);
    return align_up(af * 4, 256) + align_up(bf * 4, 256);
}

int i2v_vgg_input_stage(const float* frames, int32_t n, int32_t hi, int32_t wi, int32_t mode, int32_t ho, int32_t wo, int32_t align_corners,
                        float* out, void* stream) {
    I2V_REQUIRE(frames && out && n > 0 && hi > 0 && wi > 0 && ho > 0 && wo > 0, I2V_E_INVALID, "i2v_vgg_input_stage: bad argument");
    I2V_REQUIRE(mode == I2V_VGG_INPUT_LPIPS || mode == I2V_VGG_INPUT_DIVERSITY, I2V_E_INVALID, "i2v_vgg_input_stage: unknown mode %d", mode);
    I2V_REQUIRE(mode != I2V_VGG_INPUT_LPIPS || (ho == hi && wo == wi), I2V_E_INVALID,
                "i2v_vgg_input_stage: the LPIPS mode does not resize (%d x %d -> %d x %d)", hi, wi, ho, wo);
    I2V_REQUIRE((long)n * 3 * hi * wi < VGG_MAX_FLOATS && (long)n * 4 * ho * wo < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_input_stage: %d frames is too large", n);
    hipLaunchKernelGGL(vgg_input_kernel, dim3(grid_for((long)n * ho * wo)), dim3(256), 0, static_cast<hipStream_t>(stream), frames, out, (long)n, hi, wi,
                       ho, wo, mode, align_corners ? 1 : 0);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_vgg_features(i2v_vgg* v, const float* x, int32_t batch, int32_t h, int32_t w, float* relu1_2, float* relu2_2, float* relu3_3, float* relu4_3,
                     float* relu5_3, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, v, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_vgg_features");
    I2V_REQUIRE(x && relu1_2 && relu2_2 && relu3_3 && relu4_3 && relu5_3 && workspace && batch > 0, I2V_E_INVALID, "i2v_vgg_features: bad argument");
    I2V_REQUIRE(vgg_dims_ok(h, w), I2V_E_INVALID, "i2v_vgg_features: a %d x %d input leaves an empty map after four pools (at least 16 x 16 is needed)", h, w);
    I2V_REQUIRE((long)batch * h * w * 64 < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_features: batch %d x [%d, %d] is too large", batch, h, w);
    size_t af, bf;
    vgg_ws_floats(batch, h, w, &af, &bf);
    const size_t need = align_up(af * 4, 256) + align_up(bf * 4, 256);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, "i2v_vgg_features");
    float* a = static_cast<float*>(workspace);
    float* b = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_up(af * 4, 256));
    float* taps[5] = {relu1_2, relu2_2, relu3_3, relu4_3, relu5_3};
    return vgg_run(v, x, batch, h, w, taps, a, b, nullptr, static_cast<hipStream_t>(stream));
}

size_t i2v_vgg_saved_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w) {
    if (!v || batch <= 0 || !vgg_dims_ok(h, w)) return 0;
    size_t off[13];
    return vgg_saved_offsets(batch, h, w, off);
}

size_t i2v_vgg_backward_workspace_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w) {
    if (!v || batch <= 0 || !vgg_dims_ok(h, w)) return 0;
    return 2 * align_up((size_t)batch * h * w * 64 * 4, 256);   // two gradient maps of the largest size (relu1_x)
}

int i2v_vgg_features_saved(i2v_vgg* v, const float* x, int32_t batch, int32_t h, int32_t w, float* relu1_2, float* relu2_2, float* relu3_3,
                           float* relu4_3, float* relu5_3, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, v, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_vgg_features_saved");
    I2V_REQUIRE(x && relu1_2 && relu2_2 && relu3_3 && relu4_3 && relu5_3 && saved && workspace && batch > 0, I2V_E_INVALID,
                "i2v_vgg_features_saved: bad argument");
    I2V_REQUIRE(vgg_dims_ok(h, w), I2V_E_INVALID,
                "i2v_vgg_features_saved: a %d x %d input leaves an empty map after four pools (at least 16 x 16 is needed)", h, w);
    I2V_REQUIRE((long)batch * h * w * 64 < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_features_saved: batch %d x [%d, %d] is too large", batch, h, w);
    size_t af, bf, off[13];
    vgg_ws_floats(batch, h, w, &af, &bf);
    const size_t need = align_up(af * 4, 256) + align_up(bf * 4, 256), need_saved = vgg_saved_offsets(batch, h, w, off);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, "i2v_vgg_features_saved");
    I2V_REQUIRE(saved_bytes >= need_saved, I2V_E_WORKSPACE, "i2v_vgg_features_saved: saved state %zu < required %zu", saved_bytes, need_saved);
    float* a = static_cast<float*>(workspace);
    float* b = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_up(af * 4, 256));
    float* taps[5] = {relu1_2, relu2_2, relu3_3, relu4_3, relu5_3};
    return vgg_run(v, x, batch, h, w, taps, a, b, static_cast<char*>(saved), static_cast<hipStream_t>(stream));
}

int i2v_vgg_backward(i2v_vgg* v, const float* const* taps, const float* const* tap_grads, const void* saved, size_t saved_bytes, int32_t batch,
                     int32_t h, int32_t w, float* out, int32_t frames_out, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, v, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_vgg_backward");
    I2V_REQUIRE(saved, I2V_E_STATE, "i2v_vgg_backward: no saved state (run i2v_vgg_features_saved first: i2v_vgg_features keeps only the taps)");
    I2V_REQUIRE(taps && tap_grads && out && workspace && batch > 0, I2V_E_INVALID, "i2v_vgg_backward: bad argument");
    for (int k = 0; k < 5; ++k) I2V_REQUIRE(taps[k] && tap_grads[k], I2V_E_INVALID, "i2v_vgg_backward: tap %d or its gradient is null", k);
    I2V_REQUIRE(vgg_dims_ok(h, w), I2V_E_INVALID, "i2v_vgg_backward: a %d x %d input leaves an empty map after four pools (at least 16 x 16 is needed)",
                h, w);
    I2V_REQUIRE((long)batch * h * w * 64 < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_backward: batch %d x [%d, %d] is too large", batch, h, w);
    size_t off[13];
    const size_t need_saved = vgg_saved_offsets(batch, h, w, off), half = align_up((size_t)batch * h * w * 64 * 4, 256);
    I2V_REQUIRE(saved_bytes >= need_saved, I2V_E_WORKSPACE, "i2v_vgg_backward: saved state %zu < required %zu", saved_bytes, need_saved);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, 2 * half, "i2v_vgg_backward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ensure_dgrad(v, st)) return rc;

    int hl[13], wl[13];
    const float* y[13];
    for (int l = 0, hh = h, ww = w; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        hl[l] = hh; wl[l] = ww;
        y[l] = s.tap >= 0 ? taps[s.tap] : reinterpret_cast<const float*>(static_cast<const char*>(saved) + off[l]);
        if (s.pool) { hh /= 2; ww /= 2; }
    }
    float* const A = static_cast<float*>(workspace);
    float* const B = reinterpret_cast<float*>(static_cast<char*>(workspace) + half);
    // cur: the gradient at the pre-activation of layer l, [batch][hl][wl][cout_l]
    float* cur = A;
    const long top4 = (long)batch * hl[12] * wl[12] * (512 / 4);
    hipLaunchKernelGGL(vgg_relu_mask_kernel, dim3(grid_for(top4)), dim3(256), 0, st, tap_grads[4], y[12], cur, top4);
    I2V_HIP_CHECK(hipGetLastError());
    for (int l = 12; l >= 1; --l) {
        const LayerSpec& s = VGG_LAYERS[l];
        const LayerSpec& prev = VGG_LAYERS[l - 1];
        float* other = cur == A ? B : A;
        const float* wb = v->dgrad_w[l].as<float>();
        if (prev.pool) {   // the pooled gradient, then routing + the tap gradient that enters at y[l - 1] + its ReLU mask in one pass
            if (int rc = dgrad_launch(wb, s.cin, s.cout, cur, other, nullptr, nullptr, batch, hl[l], wl[l], st)) return rc;
            if (int rc = pool_bwd_launch(other, y[l - 1], tap_grads[prev.tap], cur, batch, hl[l - 1], wl[l - 1], prev.cout, 1, st)) return rc;
        } else {
            if (int rc = dgrad_launch(wb, s.cin, s.cout, cur, other, nullptr, y[l - 1], batch, hl[l], wl[l], st)) return rc;
            cur = other;
        }
    }
    return dgrad_first_launch(v->conv[0].w.as<float>(), cur, out, batch, h, w, frames_out ? 1 : 0, st);
}

int i2v_vgg_dgrad_unit(const float* g, const float* weight, const float* add, const float* ymask, int32_t n, int32_t h, int32_t w, int32_t cin,
                       int32_t cout, float* out, int32_t frames_out, void* stream) {
    I2V_REQUIRE(g && weight && out && n > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_vgg_dgrad_unit: bad argument");
    if (const char* why = dgrad_shape_error(cin, cout)) {
        set_error("i2v_vgg_dgrad_unit: %d -> %d channels: %s", cin, cout, why);
        return I2V_E_INVALID;
    }
    I2V_REQUIRE(cin != 3 || (!add && !ymask), I2V_E_INVALID, "i2v_vgg_dgrad_unit: the first-layer form takes neither an addend nor a mask");
    I2V_REQUIRE(cin == 3 || !frames_out, I2V_E_INVALID, "i2v_vgg_dgrad_unit: only the first-layer form writes frames");
    I2V_REQUIRE((long)n * h * w * std::max(cin, cout) < (1L << 31), I2V_E_INVALID, "i2v_vgg_dgrad_unit: batch %d x [%d, %d] is too large", n, h, w);
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf wb;
    if (cin == 3) {
        Conv c;
        std::vector<float> zero(cout, 0.f);
        if (int rc = c.pack(weight, zero.data(), cin, cout)) return rc;
        if (int rc = dgrad_first_launch(c.w.as<float>(), g, out, n, h, w, frames_out ? 1 : 0, st)) return rc;
        I2V_HIP_CHECK(hipStreamSynchronize(st));   // the packed weights die with this call
        return I2V_OK;
    }
    const std::vector<float> p = pack_dgrad_host(weight, cin, cout);
    if (int rc = wb.upload(p.data(), p.size() * 4)) return rc;
    if (int rc = dgrad_launch(wb.as<float>(), cin, cout, g, out, add, ymask, n, h, w, st)) return rc;
    I2V_HIP_CHECK(hipStreamSynchronize(st));
    return I2V_OK;
}

int i2v_vgg_maxpool2_backward(const float* grad, const float* y, const float* add, int32_t relu_mask, int32_t n, int32_t h, int32_t w, int32_t c,
                              float* out, void* stream) {
    I2V_REQUIRE(grad && y && out && n > 0 && h >= 2 && w >= 2, I2V_E_INVALID,
                "i2v_vgg_maxpool2_backward: bad argument (a map of at least 2 x 2 is needed)");
    I2V_REQUIRE(c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_vgg_maxpool2_backward: %d channels (a multiple of 4 is needed)", c);
    I2V_REQUIRE((long)n * h * w * c < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_maxpool2_backward: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    return pool_bwd_launch(grad, y, add, out, n, h, w, c, relu_mask ? 1 : 0, static_cast<hipStream_t>(stream));
}

int i2v_lpips_layer_backward(const float* f0, const float* f1, const float* lin, const double* upstream, int32_t n, int32_t p, int32_t c,
                             float* grad0, float* grad1, void* stream) {
    I2V_REQUIRE(f0 && f1 && lin && upstream && n > 0 && p > 0, I2V_E_INVALID, "i2v_lpips_layer_backward: bad argument");
    I2V_REQUIRE(grad0 || grad1, I2V_E_INVALID, "i2v_lpips_layer_backward: no gradient requested (grad0 and grad1 are both null)");
    I2V_REQUIRE(c == 64 || c == 128 || c == 256 || c == 512, I2V_E_INVALID,
                "i2v_lpips_layer_backward: %d channels (64, 128, 256 or 512: the VGG-16 taps)", c);
    I2V_REQUIRE((long)n * p * c < VGG_MAX_FLOATS && n <= (1 << 20), I2V_E_INVALID, "i2v_lpips_layer_backward: %d maps of %d positions is too large", n, p);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long np = (long)n * p;
    const dim3 grid((unsigned)std::min<long>((np + 3) / 4, 1L << 20));
    if (c == 64) hipLaunchKernelGGL(lpips_bwd_kernel<1>, grid, dim3(256), 0, st, f0, f1, lin, upstream, p, np, grad0, grad1);
    else if (c == 128) hipLaunchKernelGGL(lpips_bwd_kernel<2>, grid, dim3(256), 0, st, f0, f1, lin, upstream, p, np, grad0, grad1);
    else if (c == 256) hipLaunchKernelGGL(lpips_bwd_kernel<4>, grid, dim3(256), 0, st, f0, f1, lin, upstream, p, np, grad0, grad1);
    else hipLaunchKernelGGL(lpips_bwd_kernel<8>, grid, dim3(256), 0, st, f0, f1, lin, upstream, p, np, grad0, grad1);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_vgg_conv_unit(const float* x, const float* weight, const float* bias, int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, float* out,
                      void* stream) {
    I2V_REQUIRE(x && weight && bias && out && n > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_vgg_conv_unit: bad argument");
    if (const char* why = conv_shape_error(cin, cout)) {
        set_error("i2v_vgg_conv_unit: %d -> %d channels: %s", cin, cout, why);
        return I2V_E_INVALID;
    }
    I2V_REQUIRE((long)n * h * w * std::max(cin, cout) < (1L << 31), I2V_E_INVALID, "i2v_vgg_conv_unit: batch %d x [%d, %d] is too large", n, h, w);
    Conv c;
    if (int rc = c.pack(weight, bias, cin, cout)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = conv_launch(c, x, out, n, h, w, st)) return rc;
    I2V_HIP_CHECK(hipStreamSynchronize(st));   // the packed weights die with this call
    return I2V_OK;
}

int i2v_vgg_maxpool2(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && h >= 2 && w >= 2, I2V_E_INVALID, "i2v_vgg_maxpool2: bad argument (a map of at least 2 x 2 is needed)");
    I2V_REQUIRE(c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_vgg_maxpool2: %d channels (a multiple of 4 is needed)", c);
    I2V_REQUIRE((long)n * h * w * c < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_maxpool2: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    return pool_launch(x, out, n, h, w, c, static_cast<hipStream_t>(stream));
}

size_t i2v_vgg_reduce_workspace_bytes(int32_t n) { return n > 0 ? (size_t)std::max(n * LPIPS_G, PAIR_G) * sizeof(double) : 0; }

int i2v_lpips_layer(const float* f0, const float* f1, const float* lin, int32_t n, int32_t p, int32_t c, double* out, void* workspace,
                    size_t workspace_bytes, void* stream) {
    I2V_REQUIRE(f0 && f1 && lin && out && workspace && n > 0 && p > 0, I2V_E_INVALID, "i2v_lpips_layer: bad argument");
    I2V_REQUIRE(c == 64 || c == 128 || c == 256 || c == 512, I2V_E_INVALID, "i2v_lpips_layer: %d channels (64, 128, 256 or 512: the VGG-16 taps)", c);
    I2V_REQUIRE((long)n * p * c < VGG_MAX_FLOATS && n <= (1 << 20), I2V_E_INVALID, "i2v_lpips_layer: %d maps of %d positions is too large", n, p);
    const int G = std::min((p + 3) / 4, LPIPS_G);
    I2V_REQUIRE(workspace_bytes >= (size_t)n * G * sizeof(double), I2V_E_WORKSPACE, "i2v_lpips_layer: workspace %zu < required %zu", workspace_bytes,
                (size_t)n * G * sizeof(double));
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    const dim3 grid((unsigned)(n * G));
    if (c == 64) hipLaunchKernelGGL(lpips_partial_kernel<1>, grid, dim3(256), 0, st, f0, f1, lin, p, G, partial);
    else if (c == 128) hipLaunchKernelGGL(lpips_partial_kernel<2>, grid, dim3(256), 0, st, f0, f1, lin, p, G, partial);
    else if (c == 256) hipLaunchKernelGGL(lpips_partial_kernel<4>, grid, dim3(256), 0, st, f0, f1, lin, p, G, partial);
    else hipLaunchKernelGGL(lpips_partial_kernel<8>, grid, dim3(256), 0, st, f0, f1, lin, p, G, partial);
    I2V_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(lpips_final_kernel, dim3(1), dim3(256), 0, st, partial, n, p, G, out);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_vgg_pairdiff_update(const float* maps, int32_t r, int64_t d, double* acc, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_REQUIRE(maps && acc && workspace && d > 0, I2V_E_INVALID, "i2v_vgg_pairdiff_update: bad argument");
    I2V_REQUIRE(r >= 2 && r <= PAIR_RMAX, I2V_E_INVALID, "i2v_vgg_pairdiff_update: %d maps (2 to %d: a pair needs two, the kernel holds %d in registers)", r,
                PAIR_RMAX, PAIR_RMAX);
    I2V_REQUIRE((long)r * d < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_pairdiff_update: %d maps of %lld elements is too large", r, (long long)d);
    const int G = (int)std::min<long>((d + 255) / 256, PAIR_G);
    I2V_REQUIRE(workspace_bytes >= (size_t)G * sizeof(double), I2V_E_WORKSPACE, "i2v_vgg_pairdiff_update: workspace %zu < required %zu", workspace_bytes,
                (size_t)G * sizeof(double));
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(pairdiff_partial_kernel, dim3((unsigned)G), dim3(256), 0, st, maps, r, (long)d, G, partial);
    I2V_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pairdiff_final_kernel, dim3(1), dim3(256), 0, st, partial, G, r, (long)d, acc);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // extern "C"
