// VGG-16 `features` trunk (torchvision configuration D): the handle, its weights, the forward and the input gradient.  The layer
// table and the one walk over it (maps, buffers, sizes) are i2v_vgg_plan.h; the float64 reductions that consume the taps (the LPIPS
// layer term and its backward, the pair reduction of the VGG diversity score) are i2v_lpips.hip.
//
// Replaces stage2_cINN/AE/modules/vgg16.py (vgg16.forward: the five slices up to relu1_2, relu2_2, relu3_3, relu4_3, relu5_3),
// ScalingLayer of stage2_cINN/AE/modules/LPIPS.py and kornia Normalize + Resize of metrics/Diversity/VGG.py (the input stage).
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
// LPIPS as a loss (stage1_VAE/modules/loss.py: w_percep * LPIPS(seq_orig, seq_gen).mean()): the input gradient of the frozen trunk, see
// "backward (input gradient)" below (that of the LPIPS head: i2v_lpips.hip).
#include <algorithm>
#include <type_traits>

#include "i2v_handle.h"
#include "i2v_vgg_plan.h"

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

// ------------------------------------------------------------------------------------------------------------ backward (input gradient)
// The trunk is frozen: only the gradient at the input is formed.  The input gradient of a 3x3 / stride 1 / pad 1 convolution is the same
// convolution over the output gradient with the kernel transposed (Cin <-> Cout) and the taps flipped, so twelve of the thirteen backward
// convolutions are vgg_conv_kernel<16, VGG_EPI_DGRAD> on weights re-packed once per handle (dgrad_repack_kernel).  The first layer
// (64 -> 3) has its own narrow kernel.  Everything else is one fused memory-bound pass per pool (vgg_maxpool2_bwd_kernel: routing, the
// tap gradient that enters there, the ReLU mask), one pass per LPIPS layer (lpips_bwd_kernel, i2v_lpips.hip) and one masked copy of the relu5_3 gradient.

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

// The one launch of vgg_conv_kernel<CC, EPI>: a (all but the tile counts filled in) over N maps.  CC = 16 needs more LDS than a
// kernel gets by default: raised once per instantiation and device.
template <int CC, int EPI>
int conv_launch(VggConvArgs a, int N, const char* what, hipStream_t st) {
    a.tilesH = (a.H + VGG_TH - 1) / VGG_TH; a.tilesW = (a.W + VGG_TW - 1) / VGG_TW;
    const long nblk = (long)N * a.tilesH * a.tilesW * (a.Cout / VGG_BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "%s: grid of %ld workgroups", what, nblk);
    if constexpr (CC == 16) {
        static bool done[I2V_MAX_DEV];
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&vgg_conv_kernel<CC, EPI>), vgg_lds_bytes(CC), done)) return rc;
    }
    hipLaunchKernelGGL((vgg_conv_kernel<CC, EPI>), dim3((unsigned)nblk), dim3(256), vgg_lds_bytes(CC), st, a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int conv_fwd(const Conv& c, const float* in, float* out, int N, int H, int W, hipStream_t st) {
    VggConvArgs a{};
    a.in = in; a.wp = c.w.as<float>(); a.bias = c.bias.as<float>(); a.out = out;
    a.H = H; a.W = W; a.Cin = c.CinS; a.Cout = c.Cout; a.nchunk = c.nchunk;
    return c.CC == 16 ? conv_launch<16, VGG_EPI_FWD>(a, N, "vgg conv", st) : conv_launch<4, VGG_EPI_FWD>(a, N, "vgg conv", st);
}

// Input gradient of a forward conv cin -> cout: g [N][H][W][cout] -> out [N][H][W][cin] on the forward kernel with the DGRAD epilogue
int conv_dgrad(const float* wb, int cin, int cout, const float* g, float* out, const float* add, const float* ymask, int N, int H, int W,
               hipStream_t st) {
    VggConvArgs a{};
    a.in = g; a.wp = wb; a.bias = nullptr; a.out = out; a.add = add; a.ymask = ymask;
    a.H = H; a.W = W; a.Cin = cout; a.Cout = cin; a.nchunk = cout / 16;
    return conv_launch<16, VGG_EPI_DGRAD>(a, N, "vgg dgrad", st);
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

// what every entry that runs the trunk asks of its shape (behind its own "bad argument" check, which covers batch > 0)
int vgg_shape_check(const char* what, int batch, int h, int w) {
    I2V_REQUIRE(vgg_dims_ok(h, w), I2V_E_INVALID, "%s: a %d x %d input leaves an empty map after four pools (at least 16 x 16 is needed)", what, h, w);
    I2V_REQUIRE((long)batch * h * w * 64 < VGG_MAX_FLOATS, I2V_E_INVALID, "%s: batch %d x [%d, %d] is too large", what, batch, h, w);
    return I2V_OK;
}

// i2v_vgg_features (saved_wanted false: saved is not looked at) and i2v_vgg_features_saved.  x: channels-last input
// [batch][h][w][4]; saved: where the non-tap activations are kept instead of the workspace slots
int vgg_features(const char* what, i2v_vgg* v, const float* x, int batch, int h, int w, float* const (&taps)[5], bool saved_wanted, void* saved,
                 size_t saved_bytes, void* workspace, size_t workspace_bytes, hipStream_t st) {
    I2V_ENTER(sc, v, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, what);
    I2V_REQUIRE(x && taps[0] && taps[1] && taps[2] && taps[3] && taps[4] && (saved || !saved_wanted) && workspace && batch > 0, I2V_E_INVALID,
                "%s: bad argument", what);
    if (int rc = vgg_shape_check(what, batch, h, w)) return rc;
    const VggPlan p = vgg_plan<Carver>(batch, h, w);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.ws_bytes, what);
    I2V_REQUIRE(!saved_wanted || saved_bytes >= p.saved_bytes, I2V_E_WORKSPACE, "%s: saved state %zu < required %zu", what, saved_bytes, p.saved_bytes);
    const float* cur = x;
    for (int l = 0; l < 13; ++l) {
        const VggLayerPlan& L = p.layer[l];
        auto at = [&](VggBuf b) {
            return b == VGG_BUF_TAP ? taps[L.tap] : b == VGG_BUF_SAVED ? Carver::at(saved, L.saved_off) : Carver::at(workspace, b == VGG_BUF_A ? p.ws_a : p.ws_b);
        };
        float* const out = at(L.dst(saved_wanted));
        if (int rc = conv_fwd(v->conv[l], cur, out, batch, L.h, L.w, st)) return rc;
        cur = out;
        if (L.pool) {
            if (int rc = pool_launch(out, at(L.pool_dst), batch, L.h, L.w, L.cout, st)) return rc;
            cur = at(L.pool_dst);
        }
    }
    return I2V_OK;
}

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
    return v ? vgg_plan<Carver>(batch, h, w).ws_bytes : 0;   // (a shape the entries refuse has an empty plan)
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
    return vgg_features("i2v_vgg_features", v, x, batch, h, w, {relu1_2, relu2_2, relu3_3, relu4_3, relu5_3}, false, nullptr, 0, workspace,
                        workspace_bytes, static_cast<hipStream_t>(stream));
}

size_t i2v_vgg_saved_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w) {
    return v ? vgg_plan<Carver>(batch, h, w).saved_bytes : 0;
}

size_t i2v_vgg_backward_workspace_bytes(const i2v_vgg* v, int32_t batch, int32_t h, int32_t w) {
    return v ? vgg_plan<Carver>(batch, h, w).bwd_bytes : 0;
}

int i2v_vgg_saved_layout(int32_t batch, int32_t h, int32_t w, i2v_vgg_layer* out) {
    I2V_REQUIRE(out && batch > 0, I2V_E_INVALID, "i2v_vgg_saved_layout: bad argument");
    if (int rc = vgg_shape_check("i2v_vgg_saved_layout", batch, h, w)) return rc;
    const VggPlan p = vgg_plan<Carver>(batch, h, w);
    for (int l = 0; l < 13; ++l) out[l] = {p.layer[l].h, p.layer[l].w, p.layer[l].cout, p.layer[l].tap, (int64_t)p.layer[l].saved_off};
    return I2V_OK;
}

int i2v_vgg_features_saved(i2v_vgg* v, const float* x, int32_t batch, int32_t h, int32_t w, float* relu1_2, float* relu2_2, float* relu3_3,
                           float* relu4_3, float* relu5_3, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return vgg_features("i2v_vgg_features_saved", v, x, batch, h, w, {relu1_2, relu2_2, relu3_3, relu4_3, relu5_3}, true, saved, saved_bytes,
                        workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

int i2v_vgg_backward(i2v_vgg* v, const float* const* taps, const float* const* tap_grads, const void* saved, size_t saved_bytes, int32_t batch,
                     int32_t h, int32_t w, float* out, int32_t frames_out, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, v, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_vgg_backward");
    I2V_REQUIRE(saved, I2V_E_STATE, "i2v_vgg_backward: no saved state (run i2v_vgg_features_saved first: i2v_vgg_features keeps only the taps)");
    I2V_REQUIRE(taps && tap_grads && out && workspace && batch > 0, I2V_E_INVALID, "i2v_vgg_backward: bad argument");
    for (int k = 0; k < 5; ++k) I2V_REQUIRE(taps[k] && tap_grads[k], I2V_E_INVALID, "i2v_vgg_backward: tap %d or its gradient is null", k);
    if (int rc = vgg_shape_check("i2v_vgg_backward", batch, h, w)) return rc;
    const VggPlan p = vgg_plan<Carver>(batch, h, w);
    I2V_REQUIRE(saved_bytes >= p.saved_bytes, I2V_E_WORKSPACE, "i2v_vgg_backward: saved state %zu < required %zu", saved_bytes, p.saved_bytes);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.bwd_bytes, "i2v_vgg_backward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = ensure_dgrad(v, st)) return rc;

    // y(l): the post-ReLU activation of layer l, where the forward left it
    auto y = [&](int l) {
        const VggLayerPlan& L = p.layer[l];
        return L.tap >= 0 ? taps[L.tap] : Carver::at<const float>(const_cast<void*>(saved), L.saved_off);
    };
    float* const A = Carver::at(workspace, p.bwd_a);
    float* const B = Carver::at(workspace, p.bwd_b);
    // cur: the gradient at the pre-activation of layer l, [batch][h_l][w_l][cout_l]
    float* cur = A;
    const long top4 = (long)batch * p.layer[12].h * p.layer[12].w * (512 / 4);
    hipLaunchKernelGGL(vgg_relu_mask_kernel, dim3(grid_for(top4)), dim3(256), 0, st, tap_grads[4], y(12), cur, top4);
    I2V_HIP_CHECK(hipGetLastError());
    for (int l = 12; l >= 1; --l) {
        const VggLayerPlan& s = p.layer[l];
        const VggLayerPlan& prev = p.layer[l - 1];
        float* other = cur == A ? B : A;
        // inside a slice the ReLU mask of y(l - 1) rides on the dgrad conv; in front of a pool the pool's backward applies it
        if (int rc = conv_dgrad(v->dgrad_w[l].as<float>(), s.cin, s.cout, cur, other, nullptr, prev.pool ? nullptr : y(l - 1), batch, s.h, s.w, st)) return rc;
        if (prev.pool) {   // the pooled gradient is in `other`: routing + the tap gradient that enters at y(l - 1) + its ReLU mask in one pass
            if (int rc = pool_bwd_launch(other, y(l - 1), tap_grads[prev.tap], cur, batch, prev.h, prev.w, prev.cout, 1, st)) return rc;
        } else {
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
    Conv c;      // the first-layer form reads the forward packing,
    DevBuf wb;   // every other one the backward packing
    if (cin == 3) {
        std::vector<float> zero(cout, 0.f);
        if (int rc = c.pack(weight, zero.data(), cin, cout)) return rc;
        if (int rc = dgrad_first_launch(c.w.as<float>(), g, out, n, h, w, frames_out ? 1 : 0, st)) return rc;
    } else {
        const std::vector<float> p = pack_dgrad_host(weight, cin, cout);
        if (int rc = wb.upload(p.data(), p.size() * 4)) return rc;
        if (int rc = conv_dgrad(wb.as<float>(), cin, cout, g, out, add, ymask, n, h, w, st)) return rc;
    }
    I2V_HIP_CHECK(hipStreamSynchronize(st));   // the packed weights die with this call
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
    if (int rc = conv_fwd(c, x, out, n, h, w, st)) return rc;
    I2V_HIP_CHECK(hipStreamSynchronize(st));   // the packed weights die with this call
    return I2V_OK;
}

int i2v_vgg_maxpool2(const float* x, int32_t n, int32_t h, int32_t w, int32_t c, float* out, void* stream) {
    I2V_REQUIRE(x && out && n > 0 && h >= 2 && w >= 2, I2V_E_INVALID, "i2v_vgg_maxpool2: bad argument (a map of at least 2 x 2 is needed)");
    I2V_REQUIRE(c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_vgg_maxpool2: %d channels (a multiple of 4 is needed)", c);
    I2V_REQUIRE((long)n * h * w * c < VGG_MAX_FLOATS, I2V_E_INVALID, "i2v_vgg_maxpool2: batch %d x [%d, %d] x %d is too large", n, h, w, c);
    return pool_launch(x, out, n, h, w, c, static_cast<hipStream_t>(stream));
}

}  // extern "C"
