// The training path of one GeneratorBlock of the stage-1 decoder (stage1_VAE/modules/decoder.py:7-52): a forward that saves what the
// backward needs and the backward to x, to the latent and to every parameter, with the parameters read in place.
// The C ABI is include/i2v_hip_gblock_train.h.  Exact fp32 on v_mfma_f32_16x16x4_f32; no atomics, every sum has one owner and a fixed order.
//   * On the kernels of the 3-D ResNet training trunk (i2v_res3d_trunk.h, unchanged): conv_0 and conv_1 (conv, input gradient, sliced
//     weight gradient with the spectral-norm finish), the affine GroupNorm(16) of the learned shortcut, the power iteration, and Spade's
//     three 2-D convs: a 3x3 conv on [B][H][W] is the trunk's conv with a (3, 1, 3) window on the map [T' = H][H' = 1][W' = W] -- its
//     nine taps in torch's order, no tap that reads only padding, the 2-D weight read in place.
//   * Here: the backward of a normalisation under a modulation and a LeakyReLU (gt_nb_*: Spade and ADAIN), the 1x1x1 conv_s as plain
//     GEMMs (gt_gemm_kernel forwards and for the input gradient, gt_wgrad1_kernel sliced over the positions and finished by the trunk's
//     finish kernels), the bias gradients, ADAIN's Linear, the bilinear resize and the pointwise kernels between them.
#include "i2v_handle.h"
#include "i2v_res3d_trunk.h"
#include "../../include/i2v_hip_gblock_train.h"

#include <cstdint>

namespace i2v {
namespace {

constexpr int GT_SLICES = 32;   // most slices of a float64 partial pass

// [B][R][S] -> [B][S][R] through LDS, both sides coalesced (to_cl: [B][C][P] -> [B][P][C])
__global__ __launch_bounds__(256) void gt_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int S) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 32, s0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* ip = in + (long)b * R * S;
    float* op = out + (long)b * R * S;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && s0 + tx < S) tile[i][tx] = ip[(long)(r0 + i) * S + s0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (s0 + i < S && r0 + tx < R) op[(long)(s0 + i) * R + r0 + tx] = tile[tx][i];
}

// F.interpolate(img, (H, W), mode = 'bilinear', align_corners = True): img [B][3][ih][iw] -> out [B][H][W][4] (channel 3 is zero);
// formed in float64 and rounded once
__global__ __launch_bounds__(256) void gt_resize_kernel(const float* __restrict__ img, float* __restrict__ out, long total, int ih, int iw, int H, int W) {
    const double sh = H > 1 ? (double)(ih - 1) / (double)(H - 1) : 0.0, sw = W > 1 ? (double)(iw - 1) / (double)(W - 1) : 0.0;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int w = (int)(i % W), h = (int)((i / W) % H);
        const long b = i / ((long)W * H);
        const double fh = sh * h, fw = sw * w;
        int h0 = (int)fh, w0 = (int)fw;
        h0 = h0 > ih - 1 ? ih - 1 : h0; w0 = w0 > iw - 1 ? iw - 1 : w0;
        const int h1 = h0 + 1 < ih ? h0 + 1 : ih - 1, w1 = w0 + 1 < iw ? w0 + 1 : iw - 1;
        const double lh = fh - h0, lw = fw - w0;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* p = img + (b * 3 + c) * (long)ih * iw;
            const double top = (1.0 - lw) * (double)p[(long)h0 * iw + w0] + lw * (double)p[(long)h0 * iw + w1];
            const double bot = (1.0 - lw) * (double)p[(long)h1 * iw + w0] + lw * (double)p[(long)h1 * iw + w1];
            v[c] = (float)((1.0 - lh) * top + lh * bot);
        }
        *reinterpret_cast<float4*>(out + 4 * i) = make_float4(v[0], v[1], v[2], 0.f);
    }
}

// y [m][C] += bias [C], then LeakyReLU(0.2) where `act`
__global__ __launch_bounds__(256) void gt_bias_act_kernel(float* __restrict__ y, const float* __restrict__ bias, long total4, int C, int act) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += gridDim.x * 256L) {
        const int c = (int)((i * 4) % C);
        float4 v = *reinterpret_cast<float4*>(y + 4 * i);
        const float4 b = *reinterpret_cast<const float4*>(bias + c);
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
        if (act) {
            v.x = v.x > 0.f ? v.x : 0.2f * v.x; v.y = v.y > 0.f ? v.y : 0.2f * v.y;
            v.z = v.z > 0.f ? v.z : 0.2f * v.z; v.w = v.w > 0.f ? v.w : 0.2f * v.w;
        }
        *reinterpret_cast<float4*>(y + 4 * i) = v;
    }
}

// g *= (act > 0 ? 1 : 0.2): torch's leaky_relu_backward, the slope at exactly 0 is 0.2
__global__ __launch_bounds__(256) void gt_lrelu_bwd_kernel(float* __restrict__ g, const float* __restrict__ act, long total4) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += gridDim.x * 256L) {
        float4 v = *reinterpret_cast<float4*>(g + 4 * i);
        const float4 a = *reinterpret_cast<const float4*>(act + 4 * i);
        v.x = a.x > 0.f ? v.x : 0.2f * v.x; v.y = a.y > 0.f ? v.y : 0.2f * v.y;
        v.z = a.z > 0.f ? v.z : 0.2f * v.z; v.w = a.w > 0.f ? v.w : 0.2f * v.w;
        *reinterpret_cast<float4*>(g + 4 * i) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ modulated norms
// x [B][P][C]; stats [B][G][2] (mean, 1 / sqrt(var + eps)) of G groups of cpg channels (the instance norm: G = C).
// Spade: out = lrelu(xhat (1 + gamma) + beta), gamma and beta [B][HW][C]; ADAIN: out = lrelu(lin[c] xhat + lin[C + c]), lin [B][2 C].
struct GtModArgs {
    const float *x, *gamma, *beta, *lin;
    const double* stats;
    float* out;
    long P, HW;
    int B, C, cpg, G, adain;
};

__global__ __launch_bounds__(256) void gt_modulate_kernel(GtModArgs a) {
    const long pc4 = a.P * a.C / 4, total4 = (long)a.B * pc4;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += gridDim.x * 256L) {
        const long n = i / pc4;
        const int c = (int)((i * 4) % a.C);
        const long p = (i - n * pc4) * 4 / a.C, hw = p % a.HW;
        const float4 xv = *reinterpret_cast<const float4*>(a.x + 4 * i);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
        float4 mv, bv;
        if (a.adain) {
            mv = *reinterpret_cast<const float4*>(a.lin + n * 2 * a.C + c);
            bv = *reinterpret_cast<const float4*>(a.lin + n * 2 * a.C + a.C + c);
        } else {
            mv = *reinterpret_cast<const float4*>(a.gamma + (n * a.HW + hw) * a.C + c);
            bv = *reinterpret_cast<const float4*>(a.beta + (n * a.HW + hw) * a.C + c);
            mv.x += 1.f; mv.y += 1.f; mv.z += 1.f; mv.w += 1.f;
        }
        const float ms[4] = {mv.x, mv.y, mv.z, mv.w}, bs[4] = {bv.x, bv.y, bv.z, bv.w};
        float ys[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double* st = a.stats + (n * a.G + (c + j) / a.cpg) * 2;
            const float hv = fmaf((float)(((double)xs[j] - st[0]) * st[1]), ms[j], bs[j]);
            ys[j] = hv > 0.f ? hv : 0.2f * hv;
        }
        *reinterpret_cast<float4*>(a.out + 4 * i) = make_float4(ys[0], ys[1], ys[2], ys[3]);
    }
}

// the instance norm's statistics: per (sample, channel) sum and sum of squares over a slice of the positions, 16 channels x 16 rows per
// workgroup, the rows added in row order
struct GtStatArgs {
    const float* x;
    double *partial, *stats;   // [B][R][C][2]; [B][C][2]
    long P, rows_per;
    int B, C, R;
};

__global__ __launch_bounds__(256) void gt_in_stats_partial_kernel(GtStatArgs a) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), n = blockIdx.y, r = blockIdx.z;
    const long p0 = r * a.rows_per, p1 = p0 + a.rows_per < a.P ? p0 + a.rows_per : a.P;
    double s = 0.0, q = 0.0;
    for (long p = p0 + (tid >> 4); p < p1; p += 16) {
        const double v = (double)a.x[((long)n * a.P + p) * a.C + c];
        s += v; q += v * v;
    }
    red[0][tid] = s; red[1][tid] = q;
    __syncthreads();
    if (tid >= 16) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < 16; ++j) { t1 += red[0][j * 16 + tid]; t2 += red[1][j * 16 + tid]; }
    double* dst = a.partial + (((long)n * a.R + r) * a.C + c) * 2;
    dst[0] = t1; dst[1] = t2;
}

__global__ __launch_bounds__(256) void gt_in_stats_final_kernel(GtStatArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.B * a.C) return;
    const int n = i / a.C, c = i - n * a.C;
    double s = 0.0, q = 0.0;
    for (int r = 0; r < a.R; ++r) {
        const double* src = a.partial + (((long)n * a.R + r) * a.C + c) * 2;
        s += src[0]; q += src[1];
    }
    const double mean = s / (double)a.P, var = fmax(q / (double)a.P - mean * mean, 0.0);
    a.stats[2 * i] = mean;
    a.stats[2 * i + 1] = 1.0 / sqrt(var + 1e-5);
}

// The backward.  ga = g (act > 0 ? 1 : 0.2) in fp32 (torch's leaky_relu_backward), everything behind it in float64.
struct GtNbArgs {
    const float *g, *act, *x;
    const float* mod;      // Spade: gamma [B][HW][C]; ADAIN: lin [B][2 C]
    const double* stats;   // [B][G][2]
    const float* add;      // of dx's shape or null
    float *dx, *dgamma, *dbeta;   // Spade: the maps [B][HW][C]; ADAIN: dgamma = d_lin [B][2 C]
    double *partial, *ab, *gs;    // [B][R][C][2]; [B][C][2]; [B][G][2]
    long P, HW, rows_per;
    int B, T, C, cpg, G, R, adain;
};

// per (sample, channel) over a slice of the rows: Spade -- a row is one (h, w), all t of it summed here into the dgamma / dbeta maps,
// and the slice's sums of ga (1 + gamma) and ga (1 + gamma) xhat; ADAIN -- a row is a position, the sums of ga and ga xhat
__global__ __launch_bounds__(256) void gt_nb_partial_kernel(GtNbArgs a) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), n = blockIdx.y, r = blockIdx.z;
    const long rows = a.adain ? a.P : a.HW;
    const long r0 = r * a.rows_per, r1 = r0 + a.rows_per < rows ? r0 + a.rows_per : rows;
    const int tcount = a.adain ? 1 : a.T;
    const double* st = a.stats + ((long)n * a.G + c / a.cpg) * 2;
    const double mean = st[0], rstd = st[1];
    double s1 = 0.0, s2 = 0.0;
    for (long row = r0 + (tid >> 4); row < r1; row += 16) {
        double db = 0.0, dg = 0.0;
        for (int t = 0; t < tcount; ++t) {
            const long o = ((long)n * a.P + (a.adain ? row : t * a.HW + row)) * a.C + c;
            const float gv = a.g[o];
            const float ga = a.act[o] > 0.f ? gv : 0.2f * gv;
            db += (double)ga;
            dg += (double)ga * (((double)a.x[o] - mean) * rstd);
        }
        double m = 1.0;
        if (!a.adain) {
            const long mo = ((long)n * a.HW + row) * a.C + c;
            m = 1.0 + (double)a.mod[mo];
            if (a.dgamma) { a.dgamma[mo] = (float)dg; a.dbeta[mo] = (float)db; }
        }
        s1 += m * db; s2 += m * dg;
    }
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    if (tid >= 16) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < 16; ++j) { t1 += red[0][j * 16 + tid]; t2 += red[1][j * 16 + tid]; }
    double* dst = a.partial + (((long)n * a.R + r) * a.C + c) * 2;
    dst[0] = t1; dst[1] = t2;
}

// one workgroup per sample: the slices in slice order -> ab [n][c]; Spade: the groups' sums over their channels -> gs [n][group];
// ADAIN: (d gamma | d beta) = (ab[1] | ab[0]) -> d_lin, and gs [n][c] = gamma ab
__global__ __launch_bounds__(256) void gt_nb_reduce_kernel(GtNbArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < a.C; c += 256) {
        double t1 = 0.0, t2 = 0.0;
        for (int r = 0; r < a.R; ++r) {
            const double* src = a.partial + (((long)n * a.R + r) * a.C + c) * 2;
            t1 += src[0]; t2 += src[1];
        }
        a.ab[((long)n * a.C + c) * 2] = t1;
        a.ab[((long)n * a.C + c) * 2 + 1] = t2;
        if (a.adain) {
            const double gz = (double)a.mod[(long)n * 2 * a.C + c];
            a.gs[((long)n * a.C + c) * 2] = gz * t1;
            a.gs[((long)n * a.C + c) * 2 + 1] = gz * t2;
            if (a.dgamma) {
                a.dgamma[(long)n * 2 * a.C + c] = (float)t2;
                a.dgamma[(long)n * 2 * a.C + a.C + c] = (float)t1;
            }
        }
    }
    __syncthreads();
    if (!a.adain && tid < a.G) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < a.cpg; ++j) {
            const int c = tid * a.cpg + j;
            s1 += a.ab[((long)n * a.C + c) * 2];
            s2 += a.ab[((long)n * a.C + c) * 2 + 1];
        }
        a.gs[((long)n * a.G + tid) * 2] = s1;
        a.gs[((long)n * a.G + tid) * 2 + 1] = s2;
    }
}

// dx = rstd (ga m - s1 / M - xhat s2 / M) (+ add), M = P cpg
__global__ __launch_bounds__(256) void gt_nb_apply_kernel(GtNbArgs a) {
    const long pc4 = a.P * a.C / 4, total4 = (long)a.B * pc4;
    const double inv_m = 1.0 / ((double)a.P * a.cpg);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total4; i += gridDim.x * 256L) {
        const long n = i / pc4;
        const int c = (int)((i * 4) % a.C);
        const long p = (i - n * pc4) * 4 / a.C, hw = p % a.HW;
        const float4 gv = *reinterpret_cast<const float4*>(a.g + 4 * i);
        const float4 av = *reinterpret_cast<const float4*>(a.act + 4 * i);
        const float4 xv = *reinterpret_cast<const float4*>(a.x + 4 * i);
        const float4 mv = *reinterpret_cast<const float4*>(a.mod + (a.adain ? n * 2 * a.C + c : (n * a.HW + hw) * a.C + c));
        float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.add) dv = *reinterpret_cast<const float4*>(a.add + 4 * i);
        const float gs_[4] = {gv.x, gv.y, gv.z, gv.w}, as_[4] = {av.x, av.y, av.z, av.w}, xs[4] = {xv.x, xv.y, xv.z, xv.w};
        const float ms[4] = {mv.x, mv.y, mv.z, mv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
        float ys[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long grp = n * a.G + (c + j) / a.cpg;
            const double* st = a.stats + grp * 2;
            const double* gs = a.gs + grp * 2;
            const float ga = as_[j] > 0.f ? gs_[j] : 0.2f * gs_[j];
            const double m = a.adain ? (double)ms[j] : 1.0 + (double)ms[j];
            const double xhat = ((double)xs[j] - st[0]) * st[1];
            ys[j] = (float)(st[1] * ((double)ga * m - gs[0] * inv_m - xhat * gs[1] * inv_m)) + ds[j];
        }
        *reinterpret_cast<float4*>(a.dx + 4 * i) = make_float4(ys[0], ys[1], ys[2], ys[3]);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the 1x1x1 conv
// out [M][N] = A [M][K] . Bt [N][K]^T (+ add).  A workgroup owns 64 rows x 16 NT columns, a wave 16 rows; both operands come straight
// from memory as float4 along K: the MFMA k-slot (lane >> 4) of step s carries K element 4 (lane >> 4) + s of the chunk of 16.
struct GtGemmArgs {
    const float *a, *bt, *add;
    float* out;
    long M;
    int K, N;
};

template <int NT>
__global__ __launch_bounds__(256) void gt_gemm_kernel(GtGemmArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int nNt = a.N / (16 * NT);
    const int n0 = (int)(blockIdx.x % nNt) * 16 * NT;
    const long m0 = (long)(blockIdx.x / nNt) * 64 + wave * 16;
    const long row = m0 + lr;
    const bool rok = row < a.M;
    const float* ap = a.a + (rok ? row : 0) * a.K + 4 * kq;
    const float* bp = a.bt + (long)(n0 + lr) * a.K + 4 * kq;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < a.K; k += 16) {
        float4 av = *reinterpret_cast<const float4*>(ap + k);
        if (!rok) av = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 bv[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(bp + (long)16 * nt * a.K + k);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float as = s == 0 ? av.x : s == 1 ? av.y : s == 2 ? av.z : av.w;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float bs = s == 0 ? bv[nt].x : s == 1 ? bv[nt].y : s == 2 ? bv[nt].z : bv[nt].w;
                acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(as, bs, acc[nt], 0, 0, 0);
            }
        }
    }
    // C/D layout of the 16x16 MFMA: column = lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long m = m0 + 4 * kq + r;
            if (m >= a.M) continue;
            const long o = m * a.N + n0 + 16 * nt + lr;
            float v = acc[nt][r];
            if (a.add) v += a.add[o];
            a.out[o] = v;
        }
}

// part [S][cout][cin]: slice sl of the positions, a 16 x 16 tile per workgroup, a quarter of the slice per wave, the waves added in wave
// order.  A[i = co][k = position], B[k = position][j = ci]: k-slot (lane >> 4) of a step is position mb + (lane >> 4).
struct GtWg1Args {
    const float *g, *x;
    float* part;
    long P;
    int cout, cin, slice_len;
};

__global__ __launch_bounds__(256) void gt_wgrad1_kernel(GtWg1Args a) {
    __shared__ float red[3][4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int nCi = a.cin / 16;
    const int co0 = (int)(blockIdx.x / nCi) * 16, ci0 = (int)(blockIdx.x % nCi) * 16;
    const int sl = blockIdx.y, quarter = a.slice_len / 4;
    const long begin = (long)sl * a.slice_len + (long)wave * quarter;
    const long end = begin + quarter < a.P ? begin + quarter : a.P;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (long mb = begin; mb < end; mb += 4) {
        long m = mb + kq;
        const bool ok = m < end;
        if (!ok) m = 0;
        const float gv = a.g[m * a.cout + co0 + lr], xv = a.x[m * a.cin + ci0 + lr];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ok ? gv : 0.f, ok ? xv : 0.f, acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave > 0) return;
    float* dst = a.part + (long)sl * a.cout * a.cin;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = acc[r];
        for (int w = 0; w < 3; ++w) v += red[w][r * 64 + lane];
        dst[(long)(co0 + 4 * kq + r) * a.cin + ci0 + lr] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ bias, Linear
struct GtBgArgs {
    const float* g;    // [M][C]
    double* partial;   // [R][C]
    float* db;
    long M, rows_per;
    int C, R, accumulate;
};

__global__ __launch_bounds__(256) void gt_bias_partial_kernel(GtBgArgs a) {
    __shared__ double red[256];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), r = blockIdx.y;
    const long p0 = r * a.rows_per, p1 = p0 + a.rows_per < a.M ? p0 + a.rows_per : a.M;
    double s = 0.0;
    for (long p = p0 + (tid >> 4); p < p1; p += 16) s += (double)a.g[p * a.C + c];
    red[tid] = s;
    __syncthreads();
    if (tid >= 16) return;
    double t = 0.0;
    for (int j = 0; j < 16; ++j) t += red[j * 16 + tid];
    a.partial[(long)r * a.C + c] = t;
}

__global__ __launch_bounds__(256) void gt_bias_final_kernel(GtBgArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    double t = 0.0;
    for (int r = 0; r < a.R; ++r) t += a.partial[(long)r * a.C + c];
    a.db[c] = a.accumulate ? a.db[c] + (float)t : (float)t;
}

// lin [B][J] = z [B][K] . w [J][K]^T + bias, each element a float64 sum in k order, rounded once
__global__ __launch_bounds__(256) void gt_linear_fwd_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ lin, int B, int J, int K) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * J) return;
    const int b = i / J, j = i - b * J;
    double acc = (double)bias[j];
    for (int k = 0; k < K; ++k) acc += (double)w[(long)j * K + k] * (double)z[(long)b * K + k];
    lin[i] = (float)acc;
}

// dw [J][K] = d_lin^T z, db [J] = sum_b d_lin, dz [B][K] = d_lin w: one thread per element, float64 sums in a fixed order
__global__ __launch_bounds__(256) void gt_linear_bwd_kernel(const float* __restrict__ d_lin, const float* __restrict__ z, const float* __restrict__ w,
                                                            float* dw, float* db, float* dz, int B, int J, int K, int accumulate) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    const long nw = (long)J * K;
    if (i < nw) {
        if (!dw) return;
        const int j = (int)(i / K), k = (int)(i % K);
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += (double)d_lin[(long)b * J + j] * (double)z[(long)b * K + k];
        dw[i] = accumulate ? dw[i] + (float)acc : (float)acc;
    } else if (i < nw + J) {
        if (!db) return;
        const int j = (int)(i - nw);
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += (double)d_lin[(long)b * J + j];
        db[j] = accumulate ? db[j] + (float)acc : (float)acc;
    } else if (i < nw + J + (long)B * K) {
        if (!dz) return;
        const long e = i - nw - J;
        const int b = (int)(e / K), k = (int)(e % K);
        double acc = 0.0;
        for (int j = 0; j < J; ++j) acc += (double)d_lin[(long)b * J + j] * (double)w[(long)j * K + k];
        dz[e] = (float)acc;
    }
}

// =================================================================================================================== host side
int slices_of(long rows) { return (int)std::min<long>(std::max<long>(rows / 64, 1), GT_SLICES); }

int launch_transpose(const float* in, float* out, int B, int R, long S, hipStream_t st) {
    I2V_REQUIRE(B <= 65535 && (R + 31) / 32 <= 65535, I2V_E_INVALID, "generator block: transpose grid (%d, %d)", B, (R + 31) / 32);
    hipLaunchKernelGGL(gt_transpose_kernel, dim3((unsigned)((S + 31) / 32), (R + 31) / 32, B), dim3(256), 0, st, in, out, R, (int)S);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_bias_act(float* y, const float* bias, long rows, int C, bool act, hipStream_t st) {
    hipLaunchKernelGGL(gt_bias_act_kernel, dim3(grid_for(rows * C / 4)), dim3(256), 0, st, y, bias, rows * C / 4, C, act ? 1 : 0);
    I2V_LAUNCHED();
    return I2V_OK;
}

// GroupNorm(16) statistics alone (the trunk's two statistics kernels): stats [N][16][2]
int launch_gn_stats(const float* x, int N, long P, int C, double* stats, void* ws, hipStream_t st) {
    const D3GnWs k = gn_ws(N, C);
    D3GnArgs a{};
    a.x = x; a.stats = stats; a.partial = Carver::at<double>(ws, k.partial);
    a.P = P; a.N = N; a.C = C; a.cpg = C / D3_GROUPS; a.R = gn_slices(P, a.cpg); a.rows_per = (P + a.R - 1) / a.R;
    hipLaunchKernelGGL(d3_gn_stats_kernel, dim3(D3_GROUPS, N, a.R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3_gn_stats_final_kernel, dim3((N * D3_GROUPS + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

// scratch of the float64 partial passes: `partial` [B][GT_SLICES][C][2], ab [B][C][2], gs [B][C][2]
struct GtNormWs { size_t partial, ab, gs, total; };
GtNormWs norm_ws(int B, int C) {
    Carver k;
    GtNormWs y{};
    y.partial = k.take_bytes((size_t)B * GT_SLICES * C * 2 * 8);
    y.ab = k.take_bytes((size_t)B * C * 2 * 8);
    y.gs = k.take_bytes((size_t)B * C * 2 * 8);
    y.total = k.total();
    return y;
}

int launch_in_stats(const float* x, int B, long P, int C, double* stats, void* ws, hipStream_t st) {
    I2V_REQUIRE(B <= 65535, I2V_E_INVALID, "generator block: batch %d", B);
    const GtNormWs k = norm_ws(B, C);
    GtStatArgs a{};
    a.x = x; a.partial = Carver::at<double>(ws, k.partial); a.stats = stats;
    a.P = P; a.B = B; a.C = C; a.R = slices_of(P); a.rows_per = (P + a.R - 1) / a.R;
    hipLaunchKernelGGL(gt_in_stats_partial_kernel, dim3(C / 16, B, a.R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(gt_in_stats_final_kernel, dim3((B * C + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_modulate(const float* x, const double* stats, const float* gamma, const float* beta, const float* lin, int B, long P, long HW, int C,
                    bool adain, float* out, hipStream_t st) {
    GtModArgs a{};
    a.x = x; a.gamma = gamma; a.beta = beta; a.lin = lin; a.stats = stats; a.out = out;
    a.P = P; a.HW = HW; a.B = B; a.C = C; a.adain = adain ? 1 : 0; a.G = adain ? C : D3_GROUPS; a.cpg = C / a.G;
    hipLaunchKernelGGL(gt_modulate_kernel, dim3(grid_for((long)B * P * C / 4)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

// the partial and the reduce pass always run (they produce dgamma / dbeta and the sums); the apply pass where dx is wanted
int launch_modnorm_bwd(bool adain, const float* g, const float* act, const float* x, const double* stats, const float* mod, int B, int T, long HW,
                       int C, const float* add, float* dx, float* dgamma, float* dbeta, void* ws, hipStream_t st) {
    I2V_REQUIRE(B <= 65535, I2V_E_INVALID, "generator block: batch %d", B);
    const GtNormWs k = norm_ws(B, C);
    GtNbArgs a{};
    a.g = g; a.act = act; a.x = x; a.mod = mod; a.stats = stats; a.add = add; a.dx = dx; a.dgamma = dgamma; a.dbeta = dbeta;
    a.partial = Carver::at<double>(ws, k.partial); a.ab = Carver::at<double>(ws, k.ab); a.gs = Carver::at<double>(ws, k.gs);
    a.P = (long)T * HW; a.HW = HW; a.B = B; a.T = T; a.C = C; a.adain = adain ? 1 : 0; a.G = adain ? C : D3_GROUPS; a.cpg = C / a.G;
    const long rows = adain ? a.P : HW;
    a.R = slices_of(rows); a.rows_per = (rows + a.R - 1) / a.R;
    hipLaunchKernelGGL(gt_nb_partial_kernel, dim3(C / 16, B, a.R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(gt_nb_reduce_kernel, dim3(B), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    if (dx) {
        hipLaunchKernelGGL(gt_nb_apply_kernel, dim3(grid_for((long)B * a.P * C / 4)), dim3(256), 0, st, a);
        I2V_LAUNCHED();
    }
    return I2V_OK;
}

int launch_gemm(const float* A, const float* Bt, const float* add, long M, int K, int N, float* out, hipStream_t st) {
    GtGemmArgs a{A, Bt, add, out, M, K, N};
    const int BN = bn_of(N);
    const long nblk = (M + 63) / 64 * (N / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 31), I2V_E_INVALID, "generator block: 1x1x1 conv grid of %ld workgroups", nblk);
    const dim3 grid((unsigned)nblk);
    if (BN == 64) hipLaunchKernelGGL((gt_gemm_kernel<4>), grid, dim3(256), 0, st, a);
    else if (BN == 32) hipLaunchKernelGGL((gt_gemm_kernel<2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gt_gemm_kernel<1>), grid, dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

// the slice plan of the 1x1x1 weight gradient: enough workgroups to fill the device, slices of at least 64 positions
void wgrad1_plan(int cout, int cin, long P, int* slices, int* slice_len) {
    const long tiles = (long)(cout / 16) * (cin / 16);
    const long S = std::min<long>(std::max<long>((1024 + tiles - 1) / tiles, 1), std::max<long>((P + 63) / 64, 1));
    const long L = (long)align_up((size_t)((P + S - 1) / S), 16);
    *slice_len = (int)L;
    *slices = (int)((P + L - 1) / L);
}
size_t wgrad1_part_floats(int cout, int cin, long P) {
    int S, L;
    wgrad1_plan(cout, cin, P, &S, &L);
    return (size_t)S * cout * cin;
}

int launch_wgrad1(const float* g, const float* x, const float* w, const float* u, const float* v, const float* sigma, long P, int cout, int cin,
                  float* part, float* dwn, double* dotp, float* grad, bool accumulate, hipStream_t st) {
    int S, L;
    wgrad1_plan(cout, cin, P, &S, &L);
    I2V_REQUIRE(S <= 65535, I2V_E_INVALID, "generator block: %d weight-gradient slices", S);
    GtWg1Args a{g, x, part, P, cout, cin, L};
    hipLaunchKernelGGL(gt_wgrad1_kernel, dim3((unsigned)((cout / 16) * (cin / 16)), (unsigned)S), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return launch_finish(part, S, cin, cout, cin, 1, w, u, v, sigma, dwn, dotp, grad, accumulate, st);
}

int launch_bias_grad(const float* g, long M, int C, float* db, bool accumulate, double* partial, hipStream_t st) {
    GtBgArgs a{};
    a.g = g; a.partial = partial; a.db = db; a.M = M; a.C = C; a.R = slices_of(M); a.rows_per = (M + a.R - 1) / a.R; a.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(gt_bias_partial_kernel, dim3(C / 16, a.R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(gt_bias_final_kernel, dim3((C + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_linear_bwd(const float* d_lin, const float* z, const float* w, int B, int J, int K, float* dw, float* db, float* dz, bool accumulate,
                      hipStream_t st) {
    const long total = (long)J * K + J + (long)B * K;
    hipLaunchKernelGGL(gt_linear_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_lin, z, w, dw, db, dz, B, J, K, accumulate ? 1 : 0);
    I2V_LAUNCHED();
    return I2V_OK;
}

// a 3x3 2-D conv as the trunk's conv: window (3, 1, 3) over [T' = H][H' = 1][W' = W]
TcConv conv2d_of(int cin, int cout) { return TcConv{cin, cin == 3 ? 4 : cin, cin == 3 ? 16 : cin, cout, 3, 1, 3, 1, 1, 0}; }
TcConv conv3d_of(int cin, int cout, int sn) { return TcConv{cin, cin, cin, cout, 3, 3, 3, 1, 1, sn}; }

bool bound_ptr_(const StateDict& s, const std::string& key, int64_t numel, float** out) {
    const float* p = s.f32(key, numel);
    *out = const_cast<float*>(p);
    return p != nullptr;
}

}  // namespace
}  // namespace i2v

using namespace i2v;

// conv indices
enum { GC_0, GC_1, GC_SP, GC_G, GC_B, GC_S, GC_N };

struct i2v_gblock_train {
    int device = 0;
    bool loaded = false, have_grads = false;
    int n_in = 0, n_out = 0, n_mid = 0, z_dim = 0;
    bool sn = false, learned = false;
    TcConv L[GC_N];   // GC_S: the 1x1x1 conv, described with one tap (cout, cin, sn only)
    float *w[GC_N] = {}, *b[GC_N] = {}, *u[GC_N] = {}, *v[GC_N] = {}, *nsw = nullptr, *nsb = nullptr, *lw = nullptr, *lb = nullptr;
    float *gw[GC_N] = {}, *gb[GC_N] = {}, *gnsw = nullptr, *gnsb = nullptr, *glw = nullptr, *glb = nullptr;
};

namespace {

const char* const GC_KEY[GC_N] = {"conv_0", "conv_1", "norm_0.conv", "norm_0.conv_gamma", "norm_0.conv_beta", "conv_s"};

int ntap_gc(const i2v_gblock_train* g, int i) { return i == GC_S ? 1 : ntap_of(g->L[i]); }
bool has_gc(const i2v_gblock_train* g, int i) { return i != GC_S || g->learned; }

struct GtLayout {
    bool ok = false;
    int B = 0, T = 0, H = 0, W = 0, ih = 0, iw = 0;
    long P = 0, HW = 0;
    TcGeo geo[GC_N];
    // saved
    size_t x_cl = 0, img4 = 0, y1 = 0, gamma = 0, beta = 0, a0 = 0, y0 = 0, lin = 0, a1 = 0, xn = 0, stats0 = 0, stats1 = 0, stats_s = 0;
    size_t wf[GC_N] = {}, wd[GC_N] = {}, sigma[GC_N] = {}, us[GC_N] = {}, vs[GC_N] = {}, saved_total = 0;
    // workspace
    size_t pi_t[GC_N] = {}, pi_s[GC_N] = {}, fwd = 0, buf[6] = {}, dlin = 0, part = 0, dwn = 0, dotp = 0, norm = 0, gn = 0, ws_total = 0;
};

GtLayout gt_layout(const i2v_gblock_train* g, int B, int T, int H, int W, int ih, int iw) {
    GtLayout y;
    if (!g || B <= 0 || T <= 0 || H <= 0 || W <= 0 || ih <= 0 || iw <= 0) return y;
    const long P = (long)T * H * W, HW = (long)H * W;
    if ((long)B * P * 1024 >= (1L << 40)) return y;
    y.B = B; y.T = T; y.H = H; y.W = W; y.ih = ih; y.iw = iw; y.P = P; y.HW = HW;
    y.geo[GC_0] = make_geo(B, T, H, W, g->L[GC_0]);
    y.geo[GC_1] = make_geo(B, T, H, W, g->L[GC_1]);
    for (int i = GC_SP; i <= GC_B; ++i) y.geo[i] = make_geo(B, H, 1, W, g->L[i]);
    const size_t BP = (size_t)B * P, BHW = (size_t)B * HW;
    const int cmax = std::max(std::max(g->n_in, g->n_out), 128);
    Carver s;
    y.x_cl = s.take_floats(BP * g->n_in);
    y.img4 = s.take_floats(BHW * 4);
    y.y1 = s.take_floats(BHW * 128);
    y.gamma = s.take_floats(BHW * g->n_in);
    y.beta = s.take_floats(BHW * g->n_in);
    y.a0 = s.take_floats(BP * g->n_in);
    y.y0 = s.take_floats(BP * g->n_mid);
    y.lin = s.take_floats((size_t)B * 2 * g->n_mid);
    y.a1 = s.take_floats(BP * g->n_mid);
    y.xn = s.take_floats(g->learned ? BP * g->n_in : 0);
    y.stats0 = s.take_bytes((size_t)B * D3_GROUPS * 2 * 8);
    y.stats1 = s.take_bytes((size_t)B * g->n_mid * 2 * 8);
    y.stats_s = s.take_bytes(g->learned ? (size_t)B * D3_GROUPS * 2 * 8 : 0);
    size_t pmax = 0, emax = 0;
    for (int i = 0; i < GC_N; ++i) {
        if (!has_gc(g, i)) continue;
        const TcConv& c = g->L[i];
        const int ntap = ntap_gc(g, i);
        y.wf[i] = s.take_floats((size_t)ntap * c.cout * c.cinp);
        y.wd[i] = s.take_floats(i == GC_SP ? 0 : (size_t)ntap * c.cind * c.cout);
        y.sigma[i] = s.take_floats(c.sn ? 1 : 0);
        y.us[i] = s.take_floats(c.sn ? c.cout : 0);
        y.vs[i] = s.take_floats(c.sn ? (size_t)c.cin * ntap : 0);
        pmax = std::max(pmax, i == GC_S ? wgrad1_part_floats(c.cout, c.cin, (long)BP) : wgrad_part_floats(c, y.geo[i].mo));
        emax = std::max(emax, (size_t)c.cout * c.cin * ntap);
    }
    y.saved_total = s.total();
    Carver k;
    for (int i = 0; i < GC_N; ++i) {
        const bool sn = has_gc(g, i) && g->L[i].sn;
        y.pi_t[i] = k.take_bytes(sn ? (size_t)g->L[i].cin * ntap_gc(g, i) * 8 : 0);
        y.pi_s[i] = k.take_bytes(sn ? (size_t)g->L[i].cout * 8 : 0);
    }
    y.fwd = k.take_bytes(y.saved_total);
    for (int i = 0; i < 6; ++i) y.buf[i] = k.take_floats(BP * cmax);
    y.dlin = k.take_floats((size_t)B * 2 * g->n_mid);
    y.part = k.take_floats(pmax);
    y.dwn = k.take_floats(emax);
    y.dotp = k.take_bytes(((emax + 255) / 256 + 1) * 8);
    y.norm = k.take_bytes(norm_ws(B, cmax).total);
    y.gn = k.take_bytes(gn_ws(B, cmax).total);
    y.ws_total = k.total();
    y.ok = true;
    return y;
}

bool bind_keys(const i2v_gblock_train* g, const StateDict& sd, bool grads, float** w, float** b, float** u, float** v, float** nsw, float** nsb,
               float** lw, float** lb) {
    for (int i = 0; i < GC_N; ++i) {
        if (!has_gc(g, i)) continue;
        const TcConv& c = g->L[i];
        const std::string key = GC_KEY[i];
        const int64_t wn = (int64_t)c.cout * c.cin * ntap_gc(g, i);
        if (!bound_ptr_(sd, key + (c.sn ? ".weight_orig" : ".weight"), wn, &w[i])) return false;
        if (i != GC_S && !bound_ptr_(sd, key + ".bias", c.cout, &b[i])) return false;
        if (!grads && c.sn && (!bound_ptr_(sd, key + ".weight_u", c.cout, &u[i]) || !bound_ptr_(sd, key + ".weight_v", wn / c.cout, &v[i]))) return false;
    }
    if (g->learned && (!bound_ptr_(sd, "norm_s.bn.weight", g->n_in, nsw) || !bound_ptr_(sd, "norm_s.bn.bias", g->n_in, nsb))) return false;
    return bound_ptr_(sd, "norm_1.linear.weight", (int64_t)2 * g->n_mid * g->z_dim, lw) && bound_ptr_(sd, "norm_1.linear.bias", (int64_t)2 * g->n_mid, lb);
}

}  // namespace

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// spectral norm of the wrapped convs (sigma, and this call's u and v, into `sv`), then W (/ sigma) into the operand layouts
int gt_prepare_weights(const i2v_gblock_train* g, const GtLayout& y, bool iterate, void* sv, void* ws, hipStream_t st) {
    PdPiArgs pi{};
    pi.iterate = iterate ? 1 : 0;
    TcPackArgs pk{};
    for (int i = 0; i < GC_N; ++i) {
        if (!has_gc(g, i)) continue;
        const TcConv& c = g->L[i];
        const int ntap = ntap_gc(g, i);
        if (c.sn) {
            const int cols = c.cin * ntap;
            pi.c[pi.nconv++] = PdPiConv{g->w[i], g->u[i], g->v[i], Carver::at(sv, y.sigma[i]), Carver::at(sv, y.us[i]), Carver::at(sv, y.vs[i]),
                                        Carver::at<double>(ws, y.pi_t[i]), Carver::at<double>(ws, y.pi_s[i]), c.cout, cols, pi.btotal, pi.rtotal};
            pi.btotal += (cols + 63) / 64; pi.rtotal += c.cout;
        }
        pk.c[pk.nconv++] = TcPackConv{g->w[i], c.sn ? Carver::at(sv, y.sigma[i]) : nullptr, Carver::at(sv, y.wf[i]),
                                      i == GC_SP ? nullptr : Carver::at(sv, y.wd[i]), c.cout, c.cin, c.cinp, c.cind, ntap, pk.total};
        pk.total += (long)c.cout * c.cind * ntap;
    }
    if (pi.nconv > 0)
        if (int rc = launch_power_iteration(pi, st)) return rc;
    return launch_pack<Trunk3d>(pk, st);
}

}  // namespace

extern "C" {

int i2v_gblock_train_create(int32_t n_in, int32_t n_out, int32_t z_dim, int32_t spectral_norm, i2v_gblock_train** out) {
    const char* what = "i2v_gblock_train_create";
    I2V_REQUIRE(out, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(n_in >= 16 && n_in <= 1024 && n_in % 16 == 0 && n_out >= 16 && n_out <= 1024 && n_out % 16 == 0, I2V_E_INVALID,
                "%s: channel counts (%d -> %d) must be multiples of 16 in [16, 1024]", what, n_in, n_out);
    I2V_REQUIRE(z_dim >= 1, I2V_E_INVALID, "%s: z_dim %d is not positive", what, z_dim);
    return create_handle(what, out, [&](i2v_gblock_train* g) {
        g->n_in = n_in; g->n_out = n_out; g->n_mid = std::min(n_in, n_out); g->z_dim = z_dim;
        g->sn = spectral_norm != 0; g->learned = n_in != n_out;
        g->L[GC_0] = conv3d_of(n_in, g->n_mid, g->sn);
        g->L[GC_1] = conv3d_of(g->n_mid, n_out, g->sn);
        g->L[GC_SP] = conv2d_of(3, 128);
        g->L[GC_G] = conv2d_of(128, n_in);
        g->L[GC_B] = conv2d_of(128, n_in);
        g->L[GC_S] = TcConv{n_in, n_in, n_in, n_out, 1, 1, 1, 1, 1, g->sn};
        return I2V_OK;
    });
}

void i2v_gblock_train_destroy(i2v_gblock_train* g) { delete g; }

int i2v_gblock_train_bind(i2v_gblock_train* g, const i2v_tensor* params, int32_t n) {
    I2V_REQUIRE(g && params && n > 0, I2V_E_INVALID, "i2v_gblock_train_bind: null argument");
    g->loaded = false;
    const StateDict sd(params, n);
    if (!bind_keys(g, sd, false, g->w, g->b, g->u, g->v, &g->nsw, &g->nsb, &g->lw, &g->lb)) return I2V_E_MISSING;
    for (int i = 0; i < GC_N; ++i)
        I2V_REQUIRE(aligned16(g->w[i]) && aligned16(g->b[i]), I2V_E_INVALID, "i2v_gblock_train_bind: %s weight and bias must be 16-byte aligned", GC_KEY[i]);
    g->loaded = true;
    return I2V_OK;
}

int i2v_gblock_train_bind_grads(i2v_gblock_train* g, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(g && (grads ? n > 0 : n == 0), I2V_E_INVALID, "i2v_gblock_train_bind_grads: null handle, or a count without tensors");
    g->have_grads = false;
    if (!grads) return I2V_OK;
    const StateDict gd(grads, n);
    float *u[GC_N], *v[GC_N];
    if (!bind_keys(g, gd, true, g->gw, g->gb, u, v, &g->gnsw, &g->gnsb, &g->glw, &g->glb)) return I2V_E_MISSING;
    g->have_grads = true;
    return I2V_OK;
}

size_t i2v_gblock_train_saved_bytes(const i2v_gblock_train* g, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t img_h, int32_t img_w) {
    return gt_layout(g, batch, t, h, w, img_h, img_w).saved_total;
}
size_t i2v_gblock_train_workspace_bytes(const i2v_gblock_train* g, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t img_h, int32_t img_w) {
    return gt_layout(g, batch, t, h, w, img_h, img_w).ws_total;
}

int i2v_gblock_train_forward(i2v_gblock_train* g, const float* x, const float* z, const float* img, int32_t batch, int32_t t, int32_t h, int32_t w,
                             int32_t img_h, int32_t img_w, int32_t flags, float* out, void* saved, size_t saved_bytes, void* workspace,
                             size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gblock_train_forward";
    I2V_ENTER(sc, g, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(x && z && img && out && workspace, I2V_E_INVALID, "%s: null argument", what);
    const GtLayout y = gt_layout(g, batch, t, h, w, img_h, img_w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: batch %d, map %d x %d x %d, start frame %d x %d", what, batch, t, h, w, img_h, img_w);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    const bool save = flags & I2V_GBLOCK_TRAIN_SAVE;
    if (save) {
        I2V_REQUIRE(saved, I2V_E_INVALID, "%s: I2V_GBLOCK_TRAIN_SAVE without a saved buffer", what);
        I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* const ws = workspace;
    void* sv = save ? saved : Carver::at<char>(ws, y.fwd);
    const int B = batch, Cin = g->n_in, Cm = g->n_mid, Co = g->n_out;
    const long P = y.P, HW = y.HW, BP = B * P, BHW = B * HW;
    float *x_cl = Carver::at(sv, y.x_cl), *img4 = Carver::at(sv, y.img4), *y1 = Carver::at(sv, y.y1), *gamma = Carver::at(sv, y.gamma),
          *beta = Carver::at(sv, y.beta), *a0 = Carver::at(sv, y.a0), *y0 = Carver::at(sv, y.y0), *lin = Carver::at(sv, y.lin), *a1 = Carver::at(sv, y.a1);
    double *stats0 = Carver::at<double>(sv, y.stats0), *stats1 = Carver::at<double>(sv, y.stats1);
    float *dx1 = Carver::at(ws, y.buf[0]), *out_cl = Carver::at(ws, y.buf[1]);
    void* nws = Carver::at<char>(ws, y.norm);
    void* gnws = Carver::at<char>(ws, y.gn);
    int rc;
    if ((rc = launch_transpose(x, x_cl, B, Cin, P, st))) return rc;
    if ((rc = gt_prepare_weights(g, y, flags & I2V_GBLOCK_TRAIN_TRAIN, sv, ws, st))) return rc;
    // Spade's branch on the resized start frame
    hipLaunchKernelGGL(gt_resize_kernel, dim3(grid_for(BHW)), dim3(256), 0, st, img, img4, BHW, img_h, img_w, h, w);
    I2V_LAUNCHED();
    if ((rc = launch_conv<Trunk3d>(g->L[GC_SP], img4, Carver::at(sv, y.wf[GC_SP]), y1, y.geo[GC_SP], st))) return rc;
    if ((rc = launch_bias_act(y1, g->b[GC_SP], BHW, 128, true, st))) return rc;
    if ((rc = launch_conv<Trunk3d>(g->L[GC_G], y1, Carver::at(sv, y.wf[GC_G]), gamma, y.geo[GC_G], st))) return rc;
    if ((rc = launch_bias_act(gamma, g->b[GC_G], BHW, Cin, false, st))) return rc;
    if ((rc = launch_conv<Trunk3d>(g->L[GC_B], y1, Carver::at(sv, y.wf[GC_B]), beta, y.geo[GC_B], st))) return rc;
    if ((rc = launch_bias_act(beta, g->b[GC_B], BHW, Cin, false, st))) return rc;
    // a0 = lrelu(Spade(x)), y0 = conv_0(a0)
    if ((rc = launch_gn_stats(x_cl, B, P, Cin, stats0, gnws, st))) return rc;
    if ((rc = launch_modulate(x_cl, stats0, gamma, beta, nullptr, B, P, HW, Cin, false, a0, st))) return rc;
    if ((rc = launch_conv<Trunk3d>(g->L[GC_0], a0, Carver::at(sv, y.wf[GC_0]), y0, y.geo[GC_0], st))) return rc;
    if ((rc = launch_bias_act(y0, g->b[GC_0], BP, Cm, false, st))) return rc;
    // a1 = lrelu(ADAIN(y0, z)), dx1 = conv_1(a1)
    if ((rc = launch_in_stats(y0, B, P, Cm, stats1, nws, st))) return rc;
    hipLaunchKernelGGL(gt_linear_fwd_kernel, dim3((B * 2 * Cm + 255) / 256), dim3(256), 0, st, z, g->lw, g->lb, lin, B, 2 * Cm, g->z_dim);
    I2V_LAUNCHED();
    if ((rc = launch_modulate(y0, stats1, nullptr, nullptr, lin, B, P, HW, Cm, true, a1, st))) return rc;
    if ((rc = launch_conv<Trunk3d>(g->L[GC_1], a1, Carver::at(sv, y.wf[GC_1]), dx1, y.geo[GC_1], st))) return rc;
    if ((rc = launch_bias_act(dx1, g->b[GC_1], BP, Co, false, st))) return rc;
    // the shortcut and the sum
    if (g->learned) {
        float* xn = Carver::at(sv, y.xn);
        if ((rc = launch_gn(x_cl, nullptr, g->nsw, g->nsb, B, P, Cin, false, xn, Carver::at<double>(sv, y.stats_s), gnws, st))) return rc;
        if ((rc = launch_gemm(xn, Carver::at(sv, y.wf[GC_S]), dx1, BP, Cin, Co, out_cl, st))) return rc;
    } else {
        hipLaunchKernelGGL(d3_add_kernel, dim3(grid_for(BP * Co)), dim3(256), 0, st, dx1, x_cl, BP * Co);
        I2V_LAUNCHED();
        out_cl = dx1;
    }
    return launch_transpose(out_cl, out, B, (int)P, Co, st);
}

int i2v_gblock_train_backward(i2v_gblock_train* g, const float* g_out, const float* z, const void* saved, size_t saved_bytes, int32_t batch, int32_t t,
                              int32_t h, int32_t w, int32_t img_h, int32_t img_w, float* dx, float* dz, int32_t param_grads, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gblock_train_backward";
    I2V_ENTER(sc, g, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(g_out && z && saved && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(dx || dz || param_grads, I2V_E_INVALID, "%s: neither dx, dz nor the parameter gradients are wanted", what);
    I2V_REQUIRE(!param_grads || g->have_grads, I2V_E_STATE, "%s: param_grads without bound gradient tensors", what);
    const GtLayout y = gt_layout(g, batch, t, h, w, img_h, img_w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: batch %d, map %d x %d x %d, start frame %d x %d", what, batch, t, h, w, img_h, img_w);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* const ws = workspace;
    void* sv = const_cast<void*>(saved);
    const bool pg = param_grads != 0, acc = accumulate != 0;
    const int B = batch, Cin = g->n_in, Cm = g->n_mid, Co = g->n_out;
    const long P = y.P, HW = y.HW, BP = B * P, BHW = B * HW;
    const float *x_cl = Carver::at(sv, y.x_cl), *img4 = Carver::at(sv, y.img4), *y1 = Carver::at(sv, y.y1), *gamma = Carver::at(sv, y.gamma),
                *a0 = Carver::at(sv, y.a0), *y0 = Carver::at(sv, y.y0), *lin = Carver::at(sv, y.lin), *a1 = Carver::at(sv, y.a1);
    const double *stats0 = Carver::at<double>(sv, y.stats0), *stats1 = Carver::at<double>(sv, y.stats1);
    float *G = Carver::at(ws, y.buf[0]), *D1 = Carver::at(ws, y.buf[1]), *D2 = Carver::at(ws, y.buf[2]), *D3 = Carver::at(ws, y.buf[3]),
          *E1 = Carver::at(ws, y.buf[4]), *E2 = Carver::at(ws, y.buf[5]);
    float *d_lin = Carver::at(ws, y.dlin), *part = Carver::at(ws, y.part), *dwn = Carver::at(ws, y.dwn);
    double* dotp = Carver::at<double>(ws, y.dotp);
    void* nws = Carver::at<char>(ws, y.norm);
    void* gnws = Carver::at<char>(ws, y.gn);
    double* bpart = Carver::at<double>(nws, 0);
    auto wgrad = [&](int i, const float* gy, const float* xin) -> int {
        const TcConv& c = g->L[i];
        return launch_wgrad<Trunk3d>(c, gy, nullptr, nullptr, xin, g->w[i], c.sn ? Carver::at(sv, y.us[i]) : nullptr, c.sn ? Carver::at(sv, y.vs[i]) : nullptr,
                            c.sn ? Carver::at(sv, y.sigma[i]) : nullptr, part, dwn, dotp, g->gw[i], acc, y.geo[i], st);
    };
    auto dgrad = [&](int i, const float* gy, const float* add, float* dst) -> int {
        return launch_dgrad<Trunk3d>(g->L[i], gy, nullptr, nullptr, Carver::at(sv, y.wd[i]), add, nullptr, dst, false, B, y.geo[i], st);
    };
    int rc;
    if ((rc = launch_transpose(g_out, G, B, Co, P, st))) return rc;
    // conv_1
    if (pg) {
        if ((rc = launch_bias_grad(G, BP, Co, g->gb[GC_1], acc, bpart, st))) return rc;
        if ((rc = wgrad(GC_1, G, a1))) return rc;
    }
    if ((rc = dgrad(GC_1, G, nullptr, D1))) return rc;
    // ADAIN under the LeakyReLU, and its Linear
    const bool below = dx || pg;   // anything wanted below ADAIN
    if ((rc = launch_modnorm_bwd(true, D1, a1, y0, stats1, lin, B, t, HW, Cm, nullptr, below ? D2 : nullptr, d_lin, nullptr, nws, st))) return rc;
    if (pg || dz)
        if ((rc = launch_linear_bwd(d_lin, z, g->lw, B, 2 * Cm, g->z_dim, pg ? g->glw : nullptr, pg ? g->glb : nullptr, dz, acc, st))) return rc;
    if (!below) return I2V_OK;
    // conv_0
    if (pg) {
        if ((rc = launch_bias_grad(D2, BP, Cm, g->gb[GC_0], acc, bpart, st))) return rc;
        if ((rc = wgrad(GC_0, D2, a0))) return rc;
    }
    if ((rc = dgrad(GC_0, D2, nullptr, D3))) return rc;
    // the shortcut: D1 takes its gradient at x
    const float* short_dx = G;
    if (g->learned) {
        if ((rc = launch_gemm(G, Carver::at(sv, y.wd[GC_S]), nullptr, BP, Co, Cin, E1, st))) return rc;
        if (pg) {
            const TcConv& c = g->L[GC_S];
            if ((rc = launch_wgrad1(G, Carver::at(sv, y.xn), g->w[GC_S], c.sn ? Carver::at(sv, y.us[GC_S]) : nullptr,
                                    c.sn ? Carver::at(sv, y.vs[GC_S]) : nullptr, c.sn ? Carver::at(sv, y.sigma[GC_S]) : nullptr, BP, Co, Cin, part, dwn,
                                    dotp, g->gw[GC_S], acc, st)))
                return rc;
        }
        if ((rc = launch_gn_bwd(E1, nullptr, x_cl, Carver::at<double>(sv, y.stats_s), g->nsw, B, P, Cin, D1, pg ? g->gnsw : nullptr,
                                pg ? g->gnsb : nullptr, acc, gnws, st)))
            return rc;
        short_dx = D1;
    }
    // Spade under the LeakyReLU: dx = dx_spade + dx_shortcut, and the maps dgamma (E1) and dbeta (E2)
    if ((rc = launch_modnorm_bwd(false, D3, a0, x_cl, stats0, gamma, B, t, HW, Cin, short_dx, dx ? D2 : nullptr, pg ? E1 : nullptr, pg ? E2 : nullptr,
                                 nws, st)))
        return rc;
    if (dx)
        if ((rc = launch_transpose(D2, dx, B, (int)P, Cin, st))) return rc;
    if (!pg) return I2V_OK;
    // Spade's branch: conv_gamma and conv_beta, the LeakyReLU, conv
    if ((rc = launch_bias_grad(E1, BHW, Cin, g->gb[GC_G], acc, bpart, st))) return rc;
    if ((rc = launch_bias_grad(E2, BHW, Cin, g->gb[GC_B], acc, bpart, st))) return rc;
    if ((rc = wgrad(GC_G, E1, y1))) return rc;
    if ((rc = wgrad(GC_B, E2, y1))) return rc;
    if ((rc = dgrad(GC_G, E1, nullptr, D3))) return rc;
    if ((rc = dgrad(GC_B, E2, D3, G))) return rc;
    hipLaunchKernelGGL(gt_lrelu_bwd_kernel, dim3(grid_for(BHW * 128 / 4)), dim3(256), 0, st, G, y1, BHW * 128 / 4);
    I2V_LAUNCHED();
    if ((rc = launch_bias_grad(G, BHW, 128, g->gb[GC_SP], acc, bpart, st))) return rc;
    return wgrad(GC_SP, G, img4);
}

// ---------------------------------------------------------------------------------------------------------------- unit entries
size_t i2v_gblock_train_unit_workspace_bytes(int32_t batch, int64_t rows, int32_t c) {
    if (batch <= 0 || rows <= 0 || c <= 0 || c % 16) return 0;
    const TcConv cc = conv2d_of(c, c), c3 = conv2d_of(3, c);
    const size_t E = (size_t)c * c * 9;
    Carver k;
    k.take_bytes(norm_ws(batch, c).total);
    k.take_bytes((size_t)batch * c * 2 * 8);
    k.take_bytes(gn_ws(batch, c).total);
    k.take_floats(2 * E);
    k.take_floats(std::max(wgrad1_part_floats(c, c, rows), std::max(wgrad_part_floats(cc, rows), wgrad_part_floats(c3, rows))));
    k.take_floats(E);
    k.take_bytes(((E + 255) / 256 + 1) * 8);
    return k.total();
}

int i2v_gblock_train_modnorm_backward_unit(int32_t mode, const float* g, const float* act, const float* x, const float* mod, int32_t batch, int32_t t,
                                           int32_t h, int32_t w, int32_t c, const float* add, float* dx, float* dgamma, float* dbeta,
                                           void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gblock_train_modnorm_backward_unit";
    I2V_REQUIRE(g && act && x && mod && workspace && batch > 0 && batch <= 65535 && t > 0 && h > 0 && w > 0 && c > 0 && c % 16 == 0 &&
                    (mode == I2V_GBLOCK_TRAIN_SPADE || mode == I2V_GBLOCK_TRAIN_ADAIN),
                I2V_E_INVALID, "%s: bad argument", what);
    I2V_REQUIRE(mode == I2V_GBLOCK_TRAIN_ADAIN || !dgamma == !dbeta, I2V_E_INVALID, "%s: dgamma and dbeta come together", what);
    const bool adain = mode == I2V_GBLOCK_TRAIN_ADAIN;
    const long HW = (long)h * w, P = t * HW;
    Carver k;
    const size_t o_norm = k.take_bytes(norm_ws(batch, c).total), o_stats = k.take_bytes((size_t)batch * c * 2 * 8), o_gn = k.take_bytes(gn_ws(batch, c).total);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total(), what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* stats = Carver::at<double>(workspace, o_stats);
    void* nws = Carver::at<char>(workspace, o_norm);
    int rc;
    if (adain) rc = launch_in_stats(x, batch, P, c, stats, nws, st);
    else rc = launch_gn_stats(x, batch, P, c, stats, Carver::at<char>(workspace, o_gn), st);
    if (rc) return rc;
    return launch_modnorm_bwd(adain, g, act, x, stats, mod, batch, t, HW, c, add, dx, dgamma, dbeta, nws, st);
}

int i2v_gblock_train_pointwise_unit(const float* a, const float* w, const float* add, int64_t m, int32_t k, int32_t n, float* out, void* stream) {
    I2V_REQUIRE(a && w && out && m > 0 && k > 0 && n > 0 && k % 16 == 0 && n % 16 == 0 && aligned16(a) && aligned16(w), I2V_E_INVALID,
                "i2v_gblock_train_pointwise_unit: bad argument (k and n multiples of 16, 16-byte aligned operands)");
    return launch_gemm(a, w, add, m, k, n, out, static_cast<hipStream_t>(stream));
}

int i2v_gblock_train_pointwise_wgrad_unit(const float* g, const float* x, const float* w, const float* u, const float* v, const float* sigma,
                                          int64_t m, int32_t cout, int32_t cin, int32_t accumulate, float* dw, void* workspace,
                                          size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gblock_train_pointwise_wgrad_unit";
    I2V_REQUIRE(g && x && w && dw && workspace && m > 0 && cout > 0 && cin > 0 && cout % 16 == 0 && cin % 16 == 0 && (!sigma || (u && v)), I2V_E_INVALID,
                "%s: bad argument", what);
    const size_t E = (size_t)cout * cin;
    Carver k;
    const size_t o_part = k.take_floats(wgrad1_part_floats(cout, cin, m)), o_dwn = k.take_floats(E), o_dot = k.take_bytes(((E + 255) / 256 + 1) * 8);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total(), what);
    return launch_wgrad1(g, x, w, u, v, sigma, m, cout, cin, Carver::at(workspace, o_part), Carver::at(workspace, o_dwn),
                         Carver::at<double>(workspace, o_dot), dw, accumulate != 0, static_cast<hipStream_t>(stream));
}

int i2v_gblock_train_bias_grad_unit(const float* g, int64_t m, int32_t c, int32_t accumulate, float* db, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const char* what = "i2v_gblock_train_bias_grad_unit";
    I2V_REQUIRE(g && db && workspace && m > 0 && c > 0 && c % 16 == 0, I2V_E_INVALID, "%s: bad argument", what);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, (size_t)GT_SLICES * c * 8, what);
    return launch_bias_grad(g, m, c, db, accumulate != 0, static_cast<double*>(workspace), static_cast<hipStream_t>(stream));
}

int i2v_gblock_train_linear_backward_unit(const float* d_lin, const float* z, const float* w, int32_t batch, int32_t j, int32_t k, int32_t accumulate,
                                          float* dw, float* db, float* dz, void* stream) {
    I2V_REQUIRE(d_lin && z && w && batch > 0 && j > 0 && k > 0 && (dw || db || dz), I2V_E_INVALID, "i2v_gblock_train_linear_backward_unit: bad argument");
    return launch_linear_bwd(d_lin, z, w, batch, j, k, dw, db, dz, accumulate != 0, static_cast<hipStream_t>(stream));
}

int i2v_gblock_train_conv2d_unit(const float* x, const float* w, const float* g, int32_t batch, int32_t h, int32_t w_, int32_t cin, int32_t cout,
                                 float* y, float* dx, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gblock_train_conv2d_unit";
    I2V_REQUIRE(x && w && workspace && batch > 0 && h > 0 && w_ > 0 && cout > 0 && cout % 16 == 0 && (cin == 3 || (cin > 0 && cin % 16 == 0)) &&
                    (y || dx || dw) && (g || !(dx || dw)) && !(dx && cin == 3),
                I2V_E_INVALID, "%s: bad argument", what);
    const TcConv c = conv2d_of(cin, cout);
    const TcGeo geo = make_geo(batch, h, 1, w_, c);
    const size_t E = (size_t)cout * cin * 9;
    Carver k;
    const size_t o_wf = k.take_floats((size_t)9 * cout * c.cinp), o_wd = k.take_floats((size_t)9 * c.cind * cout),
                 o_part = k.take_floats(wgrad_part_floats(c, geo.mo)), o_dwn = k.take_floats(E), o_dot = k.take_bytes(((E + 255) / 256 + 1) * 8);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total(), what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    TcPackArgs pk{};
    pk.nconv = 1;
    pk.c[0] = TcPackConv{w, nullptr, Carver::at(workspace, o_wf), Carver::at(workspace, o_wd), cout, cin, c.cinp, c.cind, 9, 0};
    pk.total = (long)cout * c.cind * 9;
    int rc = launch_pack<Trunk3d>(pk, st);
    if (rc) return rc;
    if (y && (rc = launch_conv<Trunk3d>(c, x, Carver::at(workspace, o_wf), y, geo, st))) return rc;
    if (dx && (rc = launch_dgrad<Trunk3d>(c, g, nullptr, nullptr, Carver::at(workspace, o_wd), nullptr, nullptr, dx, false, batch, geo, st))) return rc;
    if (dw && (rc = launch_wgrad<Trunk3d>(c, g, nullptr, nullptr, x, w, nullptr, nullptr, nullptr, Carver::at(workspace, o_part), Carver::at(workspace, o_dwn),
                                 Carver::at<double>(workspace, o_dot), dw, false, geo, st)))
        return rc;
    return I2V_OK;
}

}  // extern "C"
