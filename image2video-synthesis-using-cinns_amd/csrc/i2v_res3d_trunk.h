// The 3-D ResNet-18 trunk with GroupNorm(16) that the temporal discriminator (i2v_disc3d.hip) and the motion encoder's training path
// (i2v_encoder_train.hip) share.  Its convolutions are the Trunk3d family of i2v_train_conv.h (conv, input gradient, weight gradient,
// finish, packing, the launchers and the plan helpers); what is the trunk's own lies here: the residual add, the max pool, GroupNorm and
// the windows of its convs (i2v_disc3d.hip's head comment describes them).  The host side of the trunk as a whole -- plan, binding,
// layout and the two walks -- is i2v_res3d_net.h.  Included into the anonymous namespace of its users, as i2v_power_iter.h is.
#pragma once
#include "i2v_handle.h"
#include "i2v_train_conv.h"

namespace i2v {
namespace {

constexpr int D3_MAXCONV = 21;   // stem + 4 layers x (2 + 1 + 2)
static_assert(D3_MAXCONV <= TC_MAXCONV, "one pack launch takes every conv of the trunk");
constexpr int D3_GROUPS = 16;
constexpr int D3_GN_SLICES = 32;

// ------------------------------------------------------------------------------------------------------------------ small kernels
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
TcConv make_conv(int cin, int cout, bool stem, int st, int ss, int sn) {
    return TcConv{cin, cin == 3 ? 4 : cin, cin == 3 ? 16 : cin, cout, 3, stem ? 7 : 3, stem ? 7 : 3, st, ss, sn};
}
int out_extent(int n, int k, int s) { return n + 2 * (k / 2) - k < 0 ? 0 : (n + 2 * (k / 2) - k) / s + 1; }
TcGeo make_geo(int n, int ti, int hi, int wi, const TcConv& c) {
    TcGeo m{};
    m.ti = ti; m.hi = hi; m.wi = wi;
    m.to = out_extent(ti, c.kt, c.st); m.ho = out_extent(hi, c.kh, c.ss); m.wo = out_extent(wi, c.kw, c.ss);
    m.mi = (long)n * ti * hi * wi; m.mo = (long)n * m.to * m.ho * m.wo;
    return m;
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
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_stats_final_kernel, dim3((N * D3_GROUPS + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_apply_kernel, dim3(grid_for((long)N * P * C / 4)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
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
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_bwd_reduce_kernel, dim3(N), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    if (dweight) {
        hipLaunchKernelGGL(d3_gn_bwd_param_kernel, dim3((C + 255) / 256), dim3(256), 0, st, a);
        I2V_LAUNCHED();
    }
    hipLaunchKernelGGL(d3_gn_bwd_dx_kernel, dim3(grid_for((long)N * P * C)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // namespace
}  // namespace i2v
