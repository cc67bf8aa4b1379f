// Device-side output stage: decoder frames (fp32, planar, [N, T, 3, H, W] in [-1, 1]) -> interleaved uint8 strips, grids and clips.
// Own implementation of the reference's GIF tiling and de-normalisation (utils/auxiliaries.py:15-22, 53-55) and of the rounding of
// torchvision's save_image, as device kernels: the host path pulls fp32 frames through pageable memory and permutes them in numpy.
//
//   frames_peak_kernel    max over all raw values into ONE device float (optionally accumulated into the value already there).
//                         clamp(x * 0.5 + 0.5, 0, 1) is monotone non-decreasing and so is each of its two roundings, hence the peak
//                         of the de-normalised strip is the de-normalised peak of x: reduce raw values, transform once.
//   frames_to_u8_kernel   three planes in, interleaved bytes out, placed inside a larger strip / grid or written as dense clips.
//
// Both modes are fixed by arithmetic, not by a tolerance: the multiply and the add of the de-normalisation are rounded separately
// (torch runs two kernels' worth of roundings; contraction to an FMA would change the last bit), which is why this file switches
// floating-point contraction off.
#include "i2v_common.h"

#pragma clang fp contract(off)

namespace i2v {

constexpr int FR_THREADS = 256;
constexpr int FR_PEAK_UNROLL = 4;   // float4 loads in flight per lane of the peak kernel

// Maximum into a float cell with integer atomics: the bit patterns of the non-negative floats order like signed integers, those of
// the negative ones in reverse like unsigned integers, so one atomic max or min per value serves both signs (the cell starts a job
// at -inf, which loses against everything under both orders).  Order-independent: any reduction tree gives the same bits.
__device__ __forceinline__ void peak_atomic_max(float* cell, float v) {
    if (!(__float_as_uint(v) & 0x80000000u)) atomicMax(reinterpret_cast<int*>(cell), __float_as_int(v));
    else atomicMin(reinterpret_cast<unsigned*>(cell), __float_as_uint(v));
}

__global__ void frames_peak_init_kernel(float* __restrict__ cell) { *cell = -INFINITY; }

// grid (chunks of one sample, samples folded into y); per-lane maximum -> wave (cross-lane) -> workgroup (LDS) -> ONE vector atomic.
template <bool VEC>
__global__ __launch_bounds__(FR_THREADS) void frames_peak_kernel(const float* __restrict__ x, long long per_sample, long long n_stride,
                                                                 int n, float* __restrict__ cell) {
    float m = -INFINITY;
    for (int s = blockIdx.y; s < n; s += gridDim.y) {
        const float* xs = x + (long long)s * n_stride;
        if constexpr (VEC) {
            const long long quads = per_sample >> 2;
            const float4* x4 = reinterpret_cast<const float4*>(xs);
            long long i = ((long long)blockIdx.x * FR_PEAK_UNROLL) * FR_THREADS + threadIdx.x;
#pragma unroll
            for (int u = 0; u < FR_PEAK_UNROLL; ++u, i += FR_THREADS)
                if (i < quads) {
                    const float4 v = x4[i];
                    m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
                }
        } else {
            long long i = ((long long)blockIdx.x * FR_PEAK_UNROLL) * FR_THREADS + threadIdx.x;
#pragma unroll
            for (int u = 0; u < FR_PEAK_UNROLL; ++u, i += FR_THREADS)
                if (i < per_sample) m = fmaxf(m, xs[i]);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    __shared__ float part[FR_THREADS / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < FR_THREADS / 64; ++w) m = fmaxf(m, part[w]);
        peak_atomic_max(cell, m);
    }
}

struct FrArgs {
    const float* x;
    const float* peak;          // the job's maximum of i2v_frames_peak (PEAK mode), else nullptr
    unsigned char* dst;
    long long n_stride;         // floats between samples
    long long sample_bytes;     // clips: bytes between samples of dst; strip: W * 3 (bytes between the columns of two samples)
    long long frame_bytes;      // bytes between frames of dst
    long long row_bytes;        // bytes between pixel rows of dst
    long long origin;           // byte offset of this block's first pixel inside a frame of dst
    int t, h, w, k;             // frames, rows, pixels per row; grid rows (sample s -> grid row s % k, column s / k)
    int nt;                     // n * t
    int clips;                  // 1: dst [N, T, H, W, 3]
};

__device__ __forceinline__ float fr_denorm(float v) { return fminf(fmaxf(v * 0.5f + 0.5f, 0.0f), 1.0f); }

// PEAK: trunc(d * s), s = (float)(255.0 / (double)d_peak).  UNIT: trunc(min(max(d * 255 + 0.5, 0), 255)).  The conversion saturates
// and maps NaN to 0, so non-finite frames (out of contract, as on the host) produce some byte and never a fault.
template <bool PEAK>
__device__ __forceinline__ unsigned fr_quant(float v, float s) {
    const float d = fr_denorm(v);
    if constexpr (PEAK) return (unsigned)(d * s) & 0xffu;
    return (unsigned)fminf(fmaxf(d * 255.0f + 0.5f, 0.0f), 255.0f);
}

// grid (chunks of one frame, frames of all samples folded into y).  VEC: W % 4 == 0 and every address 16-byte (loads) / 4-byte
// (stores) aligned -- a lane loads one float4 per plane (four pixels) and stores their 12 bytes as three dwords, a wave 768 contiguous
// bytes per row segment.  Otherwise a lane handles one pixel with scalar loads and byte stores (any W >= 1, any placement).
template <bool PEAK, bool VEC>
__global__ __launch_bounds__(FR_THREADS) void frames_to_u8_kernel(FrArgs a) {
    float s = 0.0f;
    if constexpr (PEAK) s = (float)(255.0 / (double)fr_denorm(*a.peak));
    const int per_row = VEC ? (a.w >> 2) : a.w;
    const int items = a.h * per_row;
    const long long plane = (long long)a.h * a.w;
    for (int f = blockIdx.y; f < a.nt; f += gridDim.y) {
        const int smp = f / a.t, t = f - smp * a.t;
        const float* src = a.x + (long long)smp * a.n_stride + (long long)t * 3 * plane;
        unsigned char* out = a.dst + (long long)t * a.frame_bytes + a.origin +
                             (a.clips ? (long long)smp * a.sample_bytes
                                      : (long long)(smp % a.k) * a.h * a.row_bytes + (long long)(smp / a.k) * a.sample_bytes);
        for (int i = blockIdx.x * FR_THREADS + threadIdx.x; i < items; i += gridDim.x * FR_THREADS) {
            const int row = i / per_row, col = i - row * per_row;
            if constexpr (VEC) {
                const long long o = (long long)row * a.w + 4 * col;
                const float4 r = *reinterpret_cast<const float4*>(src + o);
                const float4 g = *reinterpret_cast<const float4*>(src + plane + o);
                const float4 b = *reinterpret_cast<const float4*>(src + 2 * plane + o);
                const unsigned r0 = fr_quant<PEAK>(r.x, s), r1 = fr_quant<PEAK>(r.y, s), r2 = fr_quant<PEAK>(r.z, s), r3 = fr_quant<PEAK>(r.w, s);
                const unsigned g0 = fr_quant<PEAK>(g.x, s), g1 = fr_quant<PEAK>(g.y, s), g2 = fr_quant<PEAK>(g.z, s), g3 = fr_quant<PEAK>(g.w, s);
                const unsigned b0 = fr_quant<PEAK>(b.x, s), b1 = fr_quant<PEAK>(b.y, s), b2 = fr_quant<PEAK>(b.z, s), b3 = fr_quant<PEAK>(b.w, s);
                struct alignas(4) U3 { unsigned a, b, c; };
                U3 v;
                v.a = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
                v.b = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
                v.c = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
                *reinterpret_cast<U3*>(out + (long long)row * a.row_bytes + 12 * col) = v;
            } else {
                const long long o = (long long)row * a.w + col;
                unsigned char* p = out + (long long)row * a.row_bytes + 3 * col;
                p[0] = (unsigned char)fr_quant<PEAK>(src[o], s);
                p[1] = (unsigned char)fr_quant<PEAK>(src[plane + o], s);
                p[2] = (unsigned char)fr_quant<PEAK>(src[2 * plane + o], s);
            }
        }
    }
}

static bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// Checks shared by both entry points; `per_sample` and the effective sample stride come back.
static int frames_geometry(const char* what, const float* x, const i2v_frames_cfg* c, long long* per_sample, long long* n_stride) {
    I2V_REQUIRE(x && c, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(c->n > 0 && c->t > 0 && c->h > 0 && c->w > 0, I2V_E_INVALID, "%s: n, t, h, w must be positive (got %d, %d, %d, %d)", what,
                c->n, c->t, c->h, c->w);
    const long long per = (long long)c->t * 3 * c->h * c->w;
    I2V_REQUIRE((long long)c->n * c->t < (1ll << 31) && per < (1ll << 40), I2V_E_INVALID, "%s: geometry too large", what);
    I2V_REQUIRE(c->n_stride == 0 || c->n_stride >= per, I2V_E_INVALID,
                "%s: n_stride %lld is smaller than one sample (%lld floats)", what, (long long)c->n_stride, per);
    *per_sample = per;
    *n_stride = c->n_stride ? c->n_stride : per;
    return I2V_OK;
}

}  // namespace i2v

using namespace i2v;

extern "C" {

int i2v_frames_peak(const float* x, const i2v_frames_cfg* cfg, float* peak, int32_t accumulate, void* stream) {
    long long per = 0, ns = 0;
    if (int rc = frames_geometry("i2v_frames_peak", x, cfg, &per, &ns)) return rc;
    I2V_REQUIRE(peak, I2V_E_INVALID, "i2v_frames_peak: null peak");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!accumulate) frames_peak_init_kernel<<<1, 1, 0, st>>>(peak);
    const bool vec = per % 4 == 0 && ns % 4 == 0 && aligned(x, 16);
    const long long units = vec ? per / 4 : per, per_block = (long long)FR_THREADS * FR_PEAK_UNROLL;
    // about a thousand workgroups, each looping over samples: every workgroup ends in one atomic on the same cell, and a few thousand
    // of them cost more than the reduction itself (measured: 42 us at 3072 workgroups for 50 MB)
    const long long gx = (units + per_block - 1) / per_block, gy = gx >= 1024 ? 1 : 1024 / gx;
    const dim3 grid((unsigned)gx, (unsigned)(cfg->n < gy ? cfg->n : gy));
    if (vec) frames_peak_kernel<true><<<grid, FR_THREADS, 0, st>>>(x, per, ns, cfg->n, peak);
    else frames_peak_kernel<false><<<grid, FR_THREADS, 0, st>>>(x, per, ns, cfg->n, peak);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_frames_to_u8(const float* x, const i2v_frames_cfg* cfg, const float* peak, uint8_t* dst, int32_t mode, void* stream) {
    long long per = 0, ns = 0;
    if (int rc = frames_geometry("i2v_frames_to_u8", x, cfg, &per, &ns)) return rc;
    I2V_REQUIRE(dst, I2V_E_INVALID, "i2v_frames_to_u8: null dst");
    I2V_REQUIRE(mode == I2V_FRAMES_PEAK || mode == I2V_FRAMES_UNIT, I2V_E_INVALID, "i2v_frames_to_u8: mode %d", mode);
    I2V_REQUIRE((mode == I2V_FRAMES_PEAK) == (peak != nullptr), I2V_E_INVALID,
                "i2v_frames_to_u8: PEAK mode needs the peak of i2v_frames_peak, UNIT mode takes NULL");
    I2V_REQUIRE(cfg->layout == I2V_FRAMES_STRIP || cfg->layout == I2V_FRAMES_CLIPS, I2V_E_INVALID, "i2v_frames_to_u8: layout %d", cfg->layout);
    FrArgs a{};
    a.x = x; a.peak = peak; a.dst = dst;
    a.n_stride = ns; a.t = cfg->t; a.h = cfg->h; a.w = cfg->w; a.nt = cfg->n * cfg->t;
    const long long row = (long long)cfg->w * 3;
    if (cfg->layout == I2V_FRAMES_CLIPS) {
        I2V_REQUIRE(cfg->k == 1 && cfg->row0 == 0 && cfg->col0 == 0, I2V_E_INVALID, "i2v_frames_to_u8: the clip layout has no grid placement (k = 1, row0 = col0 = 0)");
        a.clips = 1; a.k = 1;
        a.row_bytes = row; a.frame_bytes = row * cfg->h; a.sample_bytes = a.frame_bytes * cfg->t; a.origin = 0;
        I2V_REQUIRE(cfg->dst_bytes >= a.sample_bytes * cfg->n, I2V_E_INVALID, "i2v_frames_to_u8: dst holds %lld bytes, %d clips need %lld",
                    (long long)cfg->dst_bytes, cfg->n, a.sample_bytes * cfg->n);
    } else {
        I2V_REQUIRE(cfg->k >= 1 && cfg->n % cfg->k == 0, I2V_E_INVALID, "i2v_frames_to_u8: k = %d does not divide n = %d", cfg->k, cfg->n);
        I2V_REQUIRE(cfg->row0 >= 0 && cfg->col0 >= 0 && cfg->dst_row_bytes > 0 && cfg->dst_frame_bytes > 0, I2V_E_INVALID,
                    "i2v_frames_to_u8: negative placement or non-positive dst strides");
        const long long cols = cfg->n / cfg->k;
        I2V_REQUIRE(((long long)cfg->col0 + cols * cfg->w) * 3 <= cfg->dst_row_bytes, I2V_E_INVALID,
                    "i2v_frames_to_u8: the column block [%d, %lld) pixels does not fit dst_row_bytes = %lld", cfg->col0,
                    (long long)cfg->col0 + cols * cfg->w, (long long)cfg->dst_row_bytes);
        I2V_REQUIRE(((long long)cfg->row0 + (long long)cfg->k * cfg->h) * cfg->dst_row_bytes <= cfg->dst_frame_bytes, I2V_E_INVALID,
                    "i2v_frames_to_u8: rows [%d, %lld) do not fit dst_frame_bytes = %lld", cfg->row0,
                    (long long)cfg->row0 + (long long)cfg->k * cfg->h, (long long)cfg->dst_frame_bytes);
        I2V_REQUIRE(cfg->dst_bytes >= cfg->dst_frame_bytes * cfg->t, I2V_E_INVALID, "i2v_frames_to_u8: dst holds %lld bytes, %d frames need %lld",
                    (long long)cfg->dst_bytes, cfg->t, (long long)cfg->dst_frame_bytes * cfg->t);
        a.clips = 0; a.k = cfg->k;
        a.row_bytes = cfg->dst_row_bytes; a.frame_bytes = cfg->dst_frame_bytes; a.sample_bytes = row;
        a.origin = (long long)cfg->row0 * cfg->dst_row_bytes + (long long)cfg->col0 * 3;
    }
    const bool vec = cfg->w % 4 == 0 && ns % 4 == 0 && aligned(x, 16) && aligned(dst, 4) && a.row_bytes % 4 == 0 && a.frame_bytes % 4 == 0 &&
                     a.origin % 4 == 0;   // (W % 4 == 0 makes W * 3, the sample and the plane strides multiples of 4 too)
    const long long items = (long long)cfg->h * (vec ? cfg->w / 4 : cfg->w);
    const dim3 grid((unsigned)((items + FR_THREADS - 1) / FR_THREADS < 64 ? (items + FR_THREADS - 1) / FR_THREADS : 64),
                    (unsigned)(a.nt < 32768 ? a.nt : 32768));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool pk = mode == I2V_FRAMES_PEAK;
    if (pk && vec) frames_to_u8_kernel<true, true><<<grid, FR_THREADS, 0, st>>>(a);
    else if (pk) frames_to_u8_kernel<true, false><<<grid, FR_THREADS, 0, st>>>(a);
    else if (vec) frames_to_u8_kernel<false, true><<<grid, FR_THREADS, 0, st>>>(a);
    else frames_to_u8_kernel<false, false><<<grid, FR_THREADS, 0, st>>>(a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // extern "C"
