// Reconstruction metrics of the stage-1 validation pass -- stage1_VAE/modules/loss.py Backward.eval :183-216 (psnr :191, ssim :194,
// the L1 error :199, KL :10-12 / :202) -- on frames that stay on the device.
//
// The reference takes psnr and ssim from pytorch_lightning.metrics.functional (1.2.7); the formulas are restated in
// include/i2v_hip.h and DESIGN §12.4.  Everything here accumulates in float64: fp32 pixels and their pairwise products are exact in
// float64, so neither the window sums nor E[x^2] - mu^2 carry fp32 cancellation.
//
//   range   recon_range_partial_kernel (one workgroup per slice of an image) -> recon_range_final_kernel (one workgroup)
//   stats   recon_tile_kernel: one workgroup per 32 x 32 tile of one channel plane; halo of p and t in LDS as fp32, the separable
//           11-tap filter rows first (five float64 row sums per halo row and column, in LDS), then columns, the SSIM quotient per
//           position, and the |p - t|, (p - t)^2 terms of the pixels the tile owns -> partial[image][channel][tile][3]
//           recon_final_kernel: per image the partials in index order -> per_image[N][3]; the rows in index order -> five scalars
//   kl      kl_normal_kernel: one workgroup
// Every reduction has one owner per output element and a fixed order, every store is a plain vector store: two runs give the same bits.
#include <cmath>

#include "i2v_common.h"

using namespace i2v;

namespace {

constexpr int RECON_WIN = 11;            // window of the Gaussian filter
constexpr int RECON_HALO = RECON_WIN - 1;
constexpr int RECON_TW = 32;             // tile width: one lane group of a ds_read_b32 / ds_read_b64 reads one tile row, conflict-free
constexpr int RECON_TH = 32;             // tile height: 7-8 % ahead of 16 rows at (64, 16, 3, 64, 64) and (32, 16, 3, 128, 128) (profiles/recon_tile_ab.md)
constexpr int RECON_RANGE_GMAX = 16;     // slices per image of the range pass
constexpr int RECON_RANGE_SLICE = 2048;  // elements per slice before the slices start to stride
constexpr long RECON_MAX_FLOATS = 1L << 40;

struct ReconGeom {
    const float* p;
    const float* t;
    long pbs, tbs;   // batch strides in floats
    int T, C, H, W;
    int tiles_y, tiles_x;
};

struct ReconWindow {
    double w[RECON_WIN];
};

__device__ __forceinline__ double wave_sum_f64(double v) {   // fixed butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over the 256 threads of a workgroup in a fixed order (wave butterfly, then the four waves in order); valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ long image_base(long bs, int T, long chw, int n) { return (long)(n / T) * bs + (long)(n % T) * chw; }

// ---------------------------------------------------------------------------------------------------------------- range

__global__ __launch_bounds__(256) void recon_range_partial_kernel(ReconGeom g, int GI, double* __restrict__ partial) {
    __shared__ float red[4][4];
    const int tid = threadIdx.x, n = blockIdx.x / GI, s = blockIdx.x % GI;
    const long chw = (long)g.C * g.H * g.W;
    const float* p = g.p + image_base(g.pbs, g.T, chw, n);
    const float* t = g.t + image_base(g.tbs, g.T, chw, n);
    float v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (long e = (long)s * 256 + tid; e < chw; e += (long)GI * 256) {
        const float a = p[e], b = t[e];
        v[0] = fminf(v[0], a); v[1] = fmaxf(v[1], a);
        v[2] = fminf(v[2], b); v[3] = fmaxf(v[3], b);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        v[0] = fminf(v[0], __shfl_xor(v[0], off, 64)); v[1] = fmaxf(v[1], __shfl_xor(v[1], off, 64));
        v[2] = fminf(v[2], __shfl_xor(v[2], off, 64)); v[3] = fmaxf(v[3], __shfl_xor(v[3], off, 64));
    }
    if ((tid & 63) == 0)
        for (int k = 0; k < 4; ++k) red[tid >> 6][k] = v[k];
    __syncthreads();
    if (tid < 4) {
        float r = red[0][tid];
        for (int w = 1; w < 4; ++w) r = (tid & 1) ? fmaxf(r, red[w][tid]) : fminf(r, red[w][tid]);
        partial[(long)blockIdx.x * 4 + tid] = (double)r;
    }
}

__global__ __launch_bounds__(256) void recon_range_final_kernel(const double* __restrict__ partial, long G, double* __restrict__ range) {
    __shared__ double red[256][4];
    const int tid = threadIdx.x;
    double v[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
    for (long i = tid; i < G; i += 256) {
        v[0] = fmin(v[0], partial[i * 4 + 0]); v[1] = fmax(v[1], partial[i * 4 + 1]);
        v[2] = fmin(v[2], partial[i * 4 + 2]); v[3] = fmax(v[3], partial[i * 4 + 3]);
    }
    for (int k = 0; k < 4; ++k) red[tid][k] = v[k];
    __syncthreads();
    if (tid < 4) {
        double r = red[0][tid];
        for (int i = 1; i < 256; ++i) r = (tid & 1) ? fmax(r, red[i][tid]) : fmin(r, red[i][tid]);
        range[tid] = r;
    }
}

// ---------------------------------------------------------------------------------------------------------------- stats

// The SSIM quotient of one position from the five window means.  Contraction is off: with it the compiler is free to fuse
// 2 (mp mt) + c1 and mp^2 + mt^2 + c1 differently, and identical inputs would no longer give exactly 1.
__device__ __forceinline__ double ssim_term(double mp, double mt, double epp, double ett, double ept, double c1, double c2) {
#pragma clang fp contract(off)
    const double mpp = mp * mp, mtt = mt * mt, mpt = mp * mt;
    const double spp = epp - mpp, stt = ett - mtt, spt = ept - mpt;
    const double upper = 2.0 * spt + c2, lower = spp + stt + c2;
    return ((2.0 * mpt + c1) * upper) / ((mpp + mtt + c1) * lower);
}

// LDS: hp, ht [TH + 10][TW + 10] fp32 (a halo row pair is 336 bytes: the float64 part behind them stays 16-byte aligned), then
// rs [5][TH + 10][TW] float64 and the four doubles of the workgroup sum
constexpr size_t RECON_HALO_BYTES = (size_t)2 * (RECON_TH + RECON_HALO) * (RECON_TW + RECON_HALO) * sizeof(float);
constexpr size_t RECON_LDS_BYTES = RECON_HALO_BYTES + (size_t)5 * (RECON_TH + RECON_HALO) * RECON_TW * sizeof(double) + 4 * sizeof(double);
static_assert(RECON_HALO_BYTES % 16 == 0, "float64 part of the LDS is misaligned");
static_assert(RECON_LDS_BYTES <= 160 * 1024, "tile does not fit the LDS");

__global__ __launch_bounds__(256) void recon_tile_kernel(ReconGeom g, ReconWindow win, const double* __restrict__ range, double fixed_range,
                                                         double* __restrict__ partial) {
    constexpr int TH = RECON_TH, TW = RECON_TW, HR = TH + RECON_HALO, HC = TW + RECON_HALO;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float* hp = reinterpret_cast<float*>(lds_raw);
    float* ht = hp + HR * HC;
    double* rs = reinterpret_cast<double*>(lds_raw + RECON_HALO_BYTES);
    double* red = rs + 5 * HR * TW;
    const int tid = threadIdx.x;
    const int tiles = g.tiles_y * g.tiles_x;
    const int tile = blockIdx.x % tiles, plane = blockIdx.x / tiles;   // plane = n * C + c
    const int n = plane / g.C, c = plane % g.C;
    const int y0 = (tile / g.tiles_x) * TH, x0 = (tile % g.tiles_x) * TW;
    const long hw = (long)g.H * g.W, chw = hw * g.C;
    const float* p = g.p + image_base(g.pbs, g.T, chw, n) + c * hw;
    const float* t = g.t + image_base(g.tbs, g.T, chw, n) + c * hw;

    double R = fixed_range;
    if (!(fixed_range > 0.0)) R = fmax(range[1] - range[0], range[3] - range[2]);
    const double k1 = 0.01 * R, k2 = 0.03 * R;
    const double c1 = k1 * k1, c2 = k2 * k2;

    // halo: rows y0 .. y0 + TH + 10, columns x0 .. x0 + TW + 10, zero outside the image (only masked positions read those)
    for (int i = tid; i < HR * HC; i += 256) {
        const int r = i / HC, q = i % HC;
        const int y = y0 + r, x = x0 + q;
        const bool in = y < g.H && x < g.W;
        hp[i] = in ? p[(long)y * g.W + x] : 0.f;
        ht[i] = in ? t[(long)y * g.W + x] : 0.f;
    }
    __syncthreads();

    // the pixels this tile owns: |p - t| and (p - t)^2
    double l1 = 0.0, sq = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / 256; ++k) {
        const int i = (tid + 256 * k) / TW, j = (tid + 256 * k) % TW;
        if (y0 + i < g.H && x0 + j < g.W) {
            const double d = (double)hp[i * HC + j] - (double)ht[i * HC + j];
            l1 += fabs(d);
            sq += d * d;
        }
    }

    // rows: rs[k][r][j] = sum_d w[d] x_k[r][j + d] for the halo rows inside the image and the columns whose window is
    const int vw = g.W - RECON_HALO - x0;   // valid output columns of this tile (may be <= 0)
    const int vh = g.H - RECON_HALO - y0;   // valid output rows
    for (int idx = tid; idx < HR * TW; idx += 256) {
        const int r = idx / TW, j = idx % TW;
        if (y0 + r < g.H && j < vw && vh > 0) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
            for (int d = 0; d < RECON_WIN; ++d) {
                const double a = (double)hp[r * HC + j + d], b = (double)ht[r * HC + j + d];
                a0 = fma(win.w[d], a, a0);
                a1 = fma(win.w[d], b, a1);
                a2 = fma(win.w[d], a * a, a2);
                a3 = fma(win.w[d], b * b, a3);
                a4 = fma(win.w[d], a * b, a4);
            }
            rs[(0 * HR + r) * TW + j] = a0;
            rs[(1 * HR + r) * TW + j] = a1;
            rs[(2 * HR + r) * TW + j] = a2;
            rs[(3 * HR + r) * TW + j] = a3;
            rs[(4 * HR + r) * TW + j] = a4;
        }
    }
    __syncthreads();

    // columns and the quotient
    double ss = 0.0;
#pragma unroll
    for (int k = 0; k < TH * TW / 256; ++k) {
        const int i = (tid + 256 * k) / TW, j = (tid + 256 * k) % TW;
        if (i < vh && j < vw) {
            double m[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) {
                double a = 0.0;
#pragma unroll
                for (int d = 0; d < RECON_WIN; ++d) a = fma(win.w[d], rs[(q * HR + i + d) * TW + j], a);
                m[q] = a;
            }
            ss += ssim_term(m[0], m[1], m[2], m[3], m[4], c1, c2);
        }
    }

    l1 = block_sum_f64(l1, red);
    sq = block_sum_f64(sq, red);
    ss = block_sum_f64(ss, red);
    if (tid == 0) {
        double* o = partial + (long)blockIdx.x * 3;
        o[0] = l1; o[1] = sq; o[2] = ss;
    }
}

// per image the C * tiles partial rows in index order -> per_image[n][3]; then the image rows in index order -> scalars[5]
__global__ __launch_bounds__(256) void recon_final_kernel(const double* __restrict__ partial, int N, int per, double pixels, double terms,
                                                          const double* __restrict__ range, double fixed_range, double* __restrict__ per_image,
                                                          double* __restrict__ scalars) {
    __shared__ double rows[256][3];
    __shared__ double tot[3];
    const int tid = threadIdx.x;
    double acc = 0.0;   // threads 0..2: the running total of column tid
    for (int base = 0; base < N; base += 256) {
        const int n = base + tid;
        if (n < N) {
            double s[3] = {0.0, 0.0, 0.0};
            const double* q = partial + (long)n * per * 3;
            for (int i = 0; i < per; ++i) {
                s[0] += q[i * 3 + 0]; s[1] += q[i * 3 + 1]; s[2] += q[i * 3 + 2];
            }
            for (int k = 0; k < 3; ++k) {
                per_image[(long)n * 3 + k] = s[k];
                rows[tid][k] = s[k];
            }
        }
        __syncthreads();
        if (tid < 3) {
            const int m = min(256, N - base);
            for (int i = 0; i < m; ++i) acc += rows[i][tid];
        }
        __syncthreads();
    }
    if (tid < 3) tot[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        const double R = fixed_range > 0.0 ? fixed_range : range[3] - range[2];   // psnr: the range of `target` alone
        const double mse = tot[1] / pixels;
        scalars[0] = tot[0] / pixels;
        scalars[1] = mse;
        scalars[2] = (2.0 * log(R) - log(mse)) * (10.0 / log(10.0));
        scalars[3] = tot[2] / terms;
        scalars[4] = terms;
    }
}

// ---------------------------------------------------------------------------------------------------------------- KL

__global__ __launch_bounds__(256) void kl_normal_kernel(const float* __restrict__ mu, const float* __restrict__ logvar, long n, int b,
                                                        double* __restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) {
        const double m = (double)mu[i], lv = (double)logvar[i];
        s += ((1.0 + lv) - m * m) - exp(lv);
    }
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) out[0] = -0.5 * (s / (double)b);
}

struct ReconPlan {
    ReconGeom g;
    int n;            // images
    long range_g;     // range partials: n * gi rows of 4 doubles
    int gi;
    long tiles;       // partial rows: n * c * tiles_y * tiles_x
    size_t off_tiles; // byte offset of the tile partials
    size_t bytes;
};

// 0 on success
int recon_plan(int32_t b, int32_t t, int32_t c, int32_t h, int32_t w, ReconPlan& pl) {
    if (b <= 0 || t <= 0 || c <= 0 || h <= 0 || w <= 0) return -1;
    const long chw = (long)c * h * w;
    if ((long)b * t > (1L << 24) || chw > (1L << 31) - 1 || (long)b * t * chw >= RECON_MAX_FLOATS) return -1;
    pl.n = b * t;
    pl.g.T = t; pl.g.C = c; pl.g.H = h; pl.g.W = w;
    pl.g.tiles_y = (h + RECON_TH - 1) / RECON_TH;
    pl.g.tiles_x = (w + RECON_TW - 1) / RECON_TW;
    pl.gi = (int)std::min<long>((chw + RECON_RANGE_SLICE - 1) / RECON_RANGE_SLICE, RECON_RANGE_GMAX);
    pl.range_g = (long)pl.n * pl.gi;
    pl.tiles = (long)pl.n * c * pl.g.tiles_y * pl.g.tiles_x;
    if (pl.tiles >= (1L << 31) - 1 || pl.range_g >= (1L << 31) - 1) return -1;
    pl.off_tiles = align_up((size_t)pl.n * RECON_RANGE_GMAX * 4 * sizeof(double), 256);
    pl.bytes = pl.off_tiles + (size_t)pl.tiles * 3 * sizeof(double);
    return 0;
}

int recon_tile_launch(const ReconPlan& pl, const ReconWindow& win, const double* range, double fixed_range, double* partial, hipStream_t st) {
    static bool done[I2V_MAX_DEV];   // 66 KiB of LDS: above the 64 KiB a kernel gets without asking
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(&recon_tile_kernel), (int)RECON_LDS_BYTES, done)) return rc;
    hipLaunchKernelGGL(recon_tile_kernel, dim3((unsigned)pl.tiles), dim3(256), RECON_LDS_BYTES, st, pl.g, win, range, fixed_range, partial);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

// g_i = exp(-(d_i / 1.5)^2 / 2), d = -5 .. 5, normalised by its sum
ReconWindow recon_window() {
    ReconWindow win;
    double sum = 0.0;
    for (int i = 0; i < RECON_WIN; ++i) {
        const double d = ((double)i - 5.0) / 1.5;
        win.w[i] = std::exp(-(d * d) / 2.0);
        sum += win.w[i];
    }
    for (int i = 0; i < RECON_WIN; ++i) win.w[i] /= sum;
    return win;
}

int recon_strides(const char* who, long chw, int32_t t, int64_t pred_bstride, int64_t target_bstride, ReconGeom& g) {
    const long dense = (long)t * chw;
    g.pbs = pred_bstride == 0 ? dense : pred_bstride;
    g.tbs = target_bstride == 0 ? dense : target_bstride;
    I2V_REQUIRE(g.pbs >= dense && g.tbs >= dense, I2V_E_INVALID, "%s: a batch stride below t * c * h * w = %ld floats (0 means dense)", who, dense);
    return I2V_OK;
}

}  // namespace

extern "C" {

size_t i2v_recon_workspace_bytes(int32_t b, int32_t t, int32_t c, int32_t h, int32_t w) {
    ReconPlan pl;
    return recon_plan(b, t, c, h, w, pl) ? 0 : pl.bytes;
}

int i2v_recon_range(const float* pred, const float* target, int32_t b, int32_t t, int32_t c, int32_t h, int32_t w, int64_t pred_bstride,
                    int64_t target_bstride, double* range, void* workspace, size_t workspace_bytes, void* stream) {
    ReconPlan pl;
    I2V_REQUIRE(pred && target && range && workspace, I2V_E_INVALID, "i2v_recon_range: null argument");
    I2V_REQUIRE(recon_plan(b, t, c, h, w, pl) == 0, I2V_E_INVALID, "i2v_recon_range: bad shape [%d][%d][%d][%d][%d]", b, t, c, h, w);
    if (int rc = recon_strides("i2v_recon_range", (long)c * h * w, t, pred_bstride, target_bstride, pl.g)) return rc;
    I2V_REQUIRE(workspace_bytes >= pl.bytes, I2V_E_WORKSPACE, "i2v_recon_range: workspace %zu < required %zu", workspace_bytes, pl.bytes);
    pl.g.p = pred; pl.g.t = target;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = static_cast<double*>(workspace);
    hipLaunchKernelGGL(recon_range_partial_kernel, dim3((unsigned)pl.range_g), dim3(256), 0, st, pl.g, pl.gi, partial);
    I2V_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(recon_range_final_kernel, dim3(1), dim3(256), 0, st, partial, pl.range_g, range);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_recon_stats(const float* pred, const float* target, int32_t b, int32_t t, int32_t c, int32_t h, int32_t w, int64_t pred_bstride,
                    int64_t target_bstride, const double* range, double fixed_range, double* per_image, double* scalars,
                    void* workspace, size_t workspace_bytes, void* stream) {
    ReconPlan pl;
    I2V_REQUIRE(pred && target && per_image && scalars && workspace, I2V_E_INVALID, "i2v_recon_stats: null argument");
    I2V_REQUIRE(fixed_range > 0.0 || (range && fixed_range == 0.0), I2V_E_INVALID,
                "i2v_recon_stats: needs the range buffer of i2v_recon_range or a fixed_range > 0 (got %g)", fixed_range);
    I2V_REQUIRE(recon_plan(b, t, c, h, w, pl) == 0, I2V_E_INVALID, "i2v_recon_stats: bad shape [%d][%d][%d][%d][%d]", b, t, c, h, w);
    I2V_REQUIRE(h >= RECON_WIN && w >= RECON_WIN, I2V_E_INVALID, "i2v_recon_stats: %d x %d frames are smaller than the 11 x 11 SSIM window", h, w);
    if (int rc = recon_strides("i2v_recon_stats", (long)c * h * w, t, pred_bstride, target_bstride, pl.g)) return rc;
    I2V_REQUIRE(workspace_bytes >= pl.bytes, I2V_E_WORKSPACE, "i2v_recon_stats: workspace %zu < required %zu", workspace_bytes, pl.bytes);
    pl.g.p = pred; pl.g.t = target;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* partial = reinterpret_cast<double*>(static_cast<char*>(workspace) + pl.off_tiles);
    const ReconWindow win = recon_window();
    if (int rc = recon_tile_launch(pl, win, range, fixed_range, partial, st)) return rc;
    const double pixels = (double)pl.n * c * h * w, terms = (double)pl.n * c * (h - RECON_HALO) * (w - RECON_HALO);
    hipLaunchKernelGGL(recon_final_kernel, dim3(1), dim3(256), 0, st, partial, pl.n, c * pl.g.tiles_y * pl.g.tiles_x, pixels, terms, range, fixed_range,
                       per_image, scalars);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_kl_normal(const float* mu, const float* logvar, int32_t b, int32_t d, double* out, void* stream) {
    I2V_REQUIRE(mu && logvar && out && b > 0 && d > 0, I2V_E_INVALID, "i2v_kl_normal: bad argument");
    hipLaunchKernelGGL(kl_normal_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), mu, logvar, (long)b * d, b, out);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // extern "C"
