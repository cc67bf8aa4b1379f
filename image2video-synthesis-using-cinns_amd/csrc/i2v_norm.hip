// Normalisation helpers shared by the decoder, the embedder and the motion encoder (declared in i2v_conv.h):
//   stats_forward    per-(b,c) sum / sum of squares of a channels-last tensor (fp64 accumulation)
//   coef_forward     the statistics folded with the affine / ADAIN parameters into one (A, B) pair per (b,c)
//   resize_forward   bilinear resize of the start frames into the conv kernels' 16-channel rows
//   norm_act_forward act(x * A + B (+ residual)) in fp32 and / or the split-fp16 operand format
#include <algorithm>

#include "i2v_conv.h"

namespace i2v {

// ------------------------------------------------------------------------------------------------ statistics
// x [B][P][C] -> sums[b][c] = (sum, sumsq) in fp64.  grid (chunks, B), block 256 = R rows x C4 float4 columns.
// Channel counts above 1024 are covered by blockIdx.z slices of 1024 channels (Ctot = row stride, C = slice width).
__global__ __launch_bounds__(256) void stats_kernel(const float* __restrict__ x, double* __restrict__ sums, int P, int C,
                                                    int rows_per_block, int Ctot) {
    __shared__ double red[256][8];
    x += (long)blockIdx.z * 1024;
    sums += (long)blockIdx.z * 2048;
    const int C4 = C >> 2;
    const int tid = threadIdx.x;
    const int R = 256 / C4;            // rows handled concurrently (C4 <= 256)
    const int col = tid % C4, r = tid / C4;
    const int b = blockIdx.y;
    const int p0 = blockIdx.x * rows_per_block;
    const int p1 = min(P, p0 + rows_per_block);
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (r < R) {
        const float* base = x + (long)b * P * Ctot + 4 * col;
        for (int p = p0 + r; p < p1; p += R) {
            const float4 v = *reinterpret_cast<const float4*>(base + (long)p * Ctot);
            s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
            q[0] += (double)v.x * v.x; q[1] += (double)v.y * v.y; q[2] += (double)v.z * v.z; q[3] += (double)v.w * v.w;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[tid][j] = s[j]; red[tid][4 + j] = q[j]; }
    __syncthreads();
    if (r == 0) {
        for (int rr = 1; rr < R; ++rr) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { s[j] += red[rr * C4 + col][j]; q[j] += red[rr * C4 + col][4 + j]; }
        }
        double* dst = sums + ((long)b * Ctot + 4 * col) * 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            atomicAdd(dst + 2 * j, s[j]);
            atomicAdd(dst + 2 * j + 1, q[j]);
        }
    }
}

// (sum, sumsq) -> per-(b,c) affine (A, B) with norm(x)*gamma + beta == x*A + B.
//   groups: number of normalisation groups (C for instance norm); count = elements per channel (T*H*W)
//   gamma/beta sources: zl != null: ADAIN, gamma = zl[b][zoff + c], beta = zl[b][zoff + C + c] (normalization_layer.py:49-50)
//                       gw != null: GroupNorm affine weight/bias per channel (normalization_layer.py:31)
//                       neither: plain normalisation (Spade's GroupNorm(affine=False), :11)
__global__ void coef_kernel(const double* __restrict__ sums, float2* __restrict__ coef, int C, int groups, double count,
                            const float* __restrict__ zl, int zstride, int zoff, const float* __restrict__ gw,
                            const float* __restrict__ gb) {
    // The sample's C (sum, sumsq) pairs are staged in LDS (one memory round trip instead of a chain of dependent ones), the
    // per-GROUP totals are formed once per group (not once per channel of the group), in the same summation order.
    __shared__ double ss[1024], qq[1024], gsum[512], gsq[512];
    const int b = blockIdx.x;
    const int cpg = C / groups;
    const bool staged = C <= 1024;
    if (staged) {
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            const double2 v = *reinterpret_cast<const double2*>(sums + ((long)b * C + c) * 2);
            ss[c] = v.x; qq[c] = v.y;
        }
        __syncthreads();
        if (cpg > 1) {   // (then groups <= 512)
            for (int g = threadIdx.x; g < groups; g += blockDim.x) {
                double s = 0, q = 0;
                for (int j = 0; j < cpg; ++j) { s += ss[g * cpg + j]; q += qq[g * cpg + j]; }
                gsum[g] = s; gsq[g] = q;
            }
            __syncthreads();
        }
    }
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        double s = 0, q = 0;
        if (staged) {
            s = cpg > 1 ? gsum[c / cpg] : ss[c];
            q = cpg > 1 ? gsq[c / cpg] : qq[c];
        } else {
            const int g0 = (c / cpg) * cpg;
            for (int j = 0; j < cpg; ++j) {
                s += sums[((long)b * C + g0 + j) * 2];
                q += sums[((long)b * C + g0 + j) * 2 + 1];
            }
        }
        const double n = count * cpg;
        const double mean = s / n;
        double var = q / n - mean * mean;  // biased variance, as F.group_norm / F.instance_norm
        var = var > 0 ? var : 0;
        const double rstd = 1.0 / sqrt(var + 1e-5);
        double gamma = 1.0, beta = 0.0;
        if (zl) { gamma = zl[(long)b * zstride + zoff + c]; beta = zl[(long)b * zstride + zoff + C + c]; }
        else if (gw) { gamma = gw[c]; beta = gb[c]; }
        coef[(long)b * C + c] = make_float2((float)(gamma * rstd), (float)(beta - gamma * mean * rstd));
    }
}

// F.interpolate(img, size=(h,w), mode='bilinear', align_corners=True) (normalization_layer.py:20), written
// channels-last with the 3 colour channels zero-padded to 16 (the conv kernel's K chunk).
__global__ void resize_kernel(const float* __restrict__ img, float* __restrict__ out, int B, int Hi, int Wi, int Ho, int Wo,
                              int hl16, int* __restrict__ range_flag, long ibs) {   // ibs: floats between the samples of `img`
    bool bad = false;
    const long total = (long)B * Ho * Wo;
    const float sh = Ho > 1 ? (float)(Hi - 1) / (float)(Ho - 1) : 0.f;
    const float sw = Wo > 1 ? (float)(Wi - 1) / (float)(Wo - 1) : 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int w = (int)(i % Wo);
        const int h = (int)((i / Wo) % Ho);
        const int b = (int)(i / ((long)Wo * Ho));
        const float fh = sh * h, fw = sw * w;
        const int h0 = (int)fh, w0 = (int)fw;
        const int h1 = h0 + (h0 < Hi - 1 ? 1 : 0), w1 = w0 + (w0 < Wi - 1 ? 1 : 0);
        const float lh1 = fh - h0, lh0 = 1.f - lh1, lw1 = fw - w0, lw0 = 1.f - lw1;
        float* o = out + i * 16;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = img + (long)b * ibs + (long)c * Hi * Wi;
            v[c] = lh0 * (lw0 * pl[h0 * Wi + w0] + lw1 * pl[h0 * Wi + w1]) +
                   lh1 * (lw0 * pl[h1 * Wi + w0] + lw1 * pl[h1 * Wi + w1]);
        }
#pragma unroll
        for (int c = 0; c < 16; ++c) o[c] = 0.f;
        if (hl16) {  // split-fp16 operand format: per 8 channels 8 x fp16 hi | 8 x fp16 lo (64 bytes per position, as fp32)
            _Float16* oh = reinterpret_cast<_Float16*>(o);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const _Float16 hh = (_Float16)v[c];
                bad |= !(fabsf(v[c]) <= 65504.f);
                oh[c] = hh;
                oh[8 + c] = (_Float16)(v[c] - (float)hh);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[c] = v[c];
        }
    }
    if (bad && range_flag) atomicOr(range_flag, 1);
}

// out = act(x * A + B (+ res)); coef index = b * cstride + c (cstride = C for per-sample norms, 0 for BatchNorm constants).
// out16 (optional, C % 8 == 0): the same values in the split-fp16 operand format of i2v_conv16.hip (per 8 channels: 8 x fp16
// hi | 8 x fp16 lo); out may then be null when only the next convolution reads the result.
__global__ __launch_bounds__(256) void norm_act_kernel(const float* __restrict__ x, const float2* __restrict__ coef, long cstride,
                                                       const float* __restrict__ res, float* __restrict__ out,
                                                       char* __restrict__ out16, long per, int C, int relu) {
    const int C4 = C >> 2;
    const int b = blockIdx.y;
    const float2* cp = coef + (long)b * cstride;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        const long off = (long)b * per * 4 + i * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + off);
        const float4 ab0 = *reinterpret_cast<const float4*>(cp + 4 * c4), ab1 = *reinterpret_cast<const float4*>(cp + 4 * c4 + 2);
        float4 r = make_float4(fmaf(v.x, ab0.x, ab0.y), fmaf(v.y, ab0.z, ab0.w), fmaf(v.z, ab1.x, ab1.y), fmaf(v.w, ab1.z, ab1.w));
        if (res) {
            const float4 q = *reinterpret_cast<const float4*>(res + off);
            r.x += q.x; r.y += q.y; r.z += q.z; r.w += q.w;
        }
        if (relu) { r.x = fmaxf(r.x, 0.f); r.y = fmaxf(r.y, 0.f); r.z = fmaxf(r.z, 0.f); r.w = fmaxf(r.w, 0.f); }
        if (out) *reinterpret_cast<float4*>(out + off) = r;
        if (out16) {
            typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
            const float rr[4] = {r.x, r.y, r.z, r.w};
            half4_t hi, lo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const _Float16 hh = (_Float16)rr[j];
                hi[j] = hh;
                lo[j] = (_Float16)(rr[j] - (float)hh);
            }
            // element index (b, pos, c4): the 8-channel group c4 / 2 occupies 32 bytes, this thread owns half of each 16-byte part
            char* o = out16 + ((long)b * per + (i - c4)) * 16 + (c4 >> 1) * 32 + (c4 & 1) * 8;
            *reinterpret_cast<half4_t*>(o) = hi;
            *reinterpret_cast<half4_t*>(o + 16) = lo;
        }
    }
}

int stats_forward(const float* x, double* sums, int B, long P, int C, hipStream_t st) {
    I2V_REQUIRE(C % 4 == 0 && (C <= 1024 || C % 1024 == 0), I2V_E_INVALID, "stats: unsupported channel count %d", C);
    I2V_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)B * C * 16, st));
    const int Cs = C > 1024 ? 1024 : C, nz = C / Cs;  // channel slices
    const int R = 256 / (Cs / 4);
    long rows = R * 16;                       // at least 16 rows per thread-row
    const long want = (P + 1023) / 1024;      // at most ~1024 chunks per sample
    if (rows < want) rows = (want + R - 1) / R * R;
    const int chunks = (int)((P + rows - 1) / rows);
    hipLaunchKernelGGL(stats_kernel, dim3(chunks, B, nz), dim3(256), 0, st, x, sums, (int)P, Cs, (int)rows, C);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int coef_forward(const double* sums, float* coef, int B, int C, int groups, double count, hipStream_t st, const float* gw,
                 const float* gb, const float* zl, int zstride, int zoff) {
    hipLaunchKernelGGL(coef_kernel, dim3(B), dim3(256), 0, st, sums, reinterpret_cast<float2*>(coef), C, groups, count, zl,
                       zstride, zoff, gw, gb);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int resize_forward(const float* img, float* out, int B, int Hi, int Wi, int Ho, int Wo, hipStream_t st, int hl16, int* flag, long ibs) {
    if (!ibs) ibs = (long)3 * Hi * Wi;
    const long tot = (long)B * Ho * Wo;
    hipLaunchKernelGGL(resize_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 65536)), dim3(256), 0, st, img, out, B, Hi, Wi,
                       Ho, Wo, hl16, flag, ibs);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int norm_act_forward(const float* x, const float* coef, long cstride, const float* res, float* out, int B, long P, int C, bool relu,
                     hipStream_t st, void* out_hl16) {
    I2V_REQUIRE(out || out_hl16, I2V_E_INVALID, "norm_act: no output");
    I2V_REQUIRE(!out_hl16 || C % 8 == 0, I2V_E_INVALID, "norm_act: the split-fp16 output needs C %% 8 == 0 (C = %d)", C);
    const long per = P * (C / 4);
    hipLaunchKernelGGL(norm_act_kernel, dim3((unsigned)std::min<long>((per + 255) / 256, 4096), B), dim3(256), 0, st, x,
                       reinterpret_cast<const float2*>(coef), cstride, res, out, static_cast<char*>(out_hl16), per, C, relu ? 1 : 0);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // namespace i2v
