// The float64 reductions behind the VGG-16 trunk (i2v_vgg.hip), forward and backward: the LPIPS layer term and the pair reduction of
// the VGG diversity score.  No handle, no weights of their own: every entry takes device pointers (the lin weights come from
// i2v_vgg_lin) and only enqueues.
//
// Replaces stage2_cINN/AE/modules/LPIPS.py (normalize_tensor, the lin layers, spatial_average) and the pair loop of
// metrics/Diversity/VGG.py (one .cpu().item() per term).
//
// The reductions (lpips_layer, pairdiff) accumulate in float64 in two fixed-order stages: per-workgroup partial sums, then one
// workgroup that adds them in index order.  The grid is a function of the shapes alone: two runs give the same bits.
#include <algorithm>

#include "i2v_common.h"
#include "i2v_vgg_plan.h"

namespace i2v {
namespace {

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

bool lpips_channels_ok(int c) { return c == 64 || c == 128 || c == 256 || c == 512; }

// the instantiation kernel<KC> of one of the two LPIPS kernels for c = 64 KC channels (c: lpips_channels_ok)
#define LPIPS_KC(c, kernel) ((c) == 64 ? kernel<1> : (c) == 128 ? kernel<2> : (c) == 256 ? kernel<4> : kernel<8>)

}  // namespace
}  // namespace i2v

using namespace i2v;

extern "C" {

int i2v_lpips_layer_backward(const float* f0, const float* f1, const float* lin, const double* upstream, int32_t n, int32_t p, int32_t c,
                             float* grad0, float* grad1, void* stream) {
    I2V_REQUIRE(f0 && f1 && lin && upstream && n > 0 && p > 0, I2V_E_INVALID, "i2v_lpips_layer_backward: bad argument");
    I2V_REQUIRE(grad0 || grad1, I2V_E_INVALID, "i2v_lpips_layer_backward: no gradient requested (grad0 and grad1 are both null)");
    I2V_REQUIRE(lpips_channels_ok(c), I2V_E_INVALID, "i2v_lpips_layer_backward: %d channels (64, 128, 256 or 512: the VGG-16 taps)", c);
    I2V_REQUIRE((long)n * p * c < VGG_MAX_FLOATS && n <= (1 << 20), I2V_E_INVALID, "i2v_lpips_layer_backward: %d maps of %d positions is too large", n, p);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long np = (long)n * p;
    const dim3 grid((unsigned)std::min<long>((np + 3) / 4, 1L << 20));
    hipLaunchKernelGGL(LPIPS_KC(c, lpips_bwd_kernel), grid, dim3(256), 0, st, f0, f1, lin, upstream, p, np, grad0, grad1);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

size_t i2v_vgg_reduce_workspace_bytes(int32_t n) { return n > 0 ? (size_t)std::max(n * LPIPS_G, PAIR_G) * sizeof(double) : 0; }

int i2v_lpips_layer(const float* f0, const float* f1, const float* lin, int32_t n, int32_t p, int32_t c, double* out, void* workspace,
                    size_t workspace_bytes, void* stream) {
    I2V_REQUIRE(f0 && f1 && lin && out && workspace && n > 0 && p > 0, I2V_E_INVALID, "i2v_lpips_layer: bad argument");
    I2V_REQUIRE(lpips_channels_ok(c), I2V_E_INVALID, "i2v_lpips_layer: %d channels (64, 128, 256 or 512: the VGG-16 taps)", c);
    I2V_REQUIRE((long)n * p * c < VGG_MAX_FLOATS && n <= (1 << 20), I2V_E_INVALID, "i2v_lpips_layer: %d maps of %d positions is too large", n, p);
    const int G = std::min((p + 3) / 4, LPIPS_G);
    I2V_REQUIRE(workspace_bytes >= (size_t)n * G * sizeof(double), I2V_E_WORKSPACE, "i2v_lpips_layer: workspace %zu < required %zu", workspace_bytes,
                (size_t)n * G * sizeof(double));
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    const dim3 grid((unsigned)(n * G));
    hipLaunchKernelGGL(LPIPS_KC(c, lpips_partial_kernel), grid, dim3(256), 0, st, f0, f1, lin, p, G, partial);
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
