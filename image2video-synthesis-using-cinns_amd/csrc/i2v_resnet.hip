// The launch side of the two residual networks in front of the cINN (motion encoder, row N3; conditioning embedder, row N1): the
// kernels only they run, the conv description ResConv, and launch(), the loop over the steps of a plan (i2v_resnet_plan.h).
//
// Motion encoder: the 3-channel stem is a direct fp32 convolution on the vector ALU with its whole [3*7*7*3][c0] weight set resident
// in LDS (a 7x7 stride-2 halo brick of 16-channel rows would not fit the MFMA kernel's LDS tile).  The 3x3x3 convs run on the
// split-fp16 matrix-core kernel (i2v_conv16.hip, fp32-class accuracy): the stride-1 ones directly, the strided conv1 / down-sample
// convs as stride-1 2-tap convs on a space-to-depth copy of their input (enc_s2d_hl16_kernel); a temporal stride alone runs on the
// exact-fp32 kernel.  Embedder: the stride-1 3x3 convs on the split-fp16 kernel, every other conv on the exact-fp32 MFMA implicit-GEMM
// kernel (i2v_conv.hip, with spatial stride and the 7x7 stem).  Norm + ReLU (+ residual) is one elementwise pass over channels-last
// activations driven by per-(b,c) (A,B) pairs (i2v_norm.hip); it emits fp32 and / or the split-fp16 operand format.
#include <algorithm>

#include "i2v_resnet.h"

namespace i2v {

// x [B][3][Tin][Hin][Win] (the reference's NCDHW clip) -> out channels-last [B][To][Ho][Wo][C0]; stride 2, pad (1,3,3).
// Weights in LDS as [tap][cin][C0]; one thread = one output position x 16 output channels.
__global__ __launch_bounds__(256) void enc_stem_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                       float* __restrict__ out, int B, int Tin, int Hin, int Win, int To, int Ho,
                                                       int Wo, int C0) {
    extern __shared__ __attribute__((aligned(16))) float wl[];  // [147*3][C0]
    const int nw = 147 * 3 * C0;
    for (int i = threadIdx.x; i < nw; i += 256) wl[i] = wp[i];
    __syncthreads();
    const int ngrp = C0 / 16;
    const long npos = (long)B * To * Ho * Wo;
    const long total = (npos + 63) / 64 * 64 * ngrp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int pos_in_blk = (int)(i % 64);  // 64 consecutive positions x ngrp groups: lanes of a wave share the group
        long blk = i / 64;
        const int g = (int)(blk % ngrp);
        const long p = (blk / ngrp) * 64 + pos_in_blk;
        if (p >= npos) continue;
        long q = p;
        const int wo = (int)(q % Wo); q /= Wo;
        const int ho = (int)(q % Ho); q /= Ho;
        const int to = (int)(q % To);
        const int b = (int)(q / To);
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        for (int dt = 0; dt < 3; ++dt) {
            const int t = 2 * to + dt - 1;
            if ((unsigned)t >= (unsigned)Tin) continue;
            for (int dh = 0; dh < 7; ++dh) {
                const int h = 2 * ho + dh - 3;
                if ((unsigned)h >= (unsigned)Hin) continue;
                for (int dw = 0; dw < 7; ++dw) {
                    const int w = 2 * wo + dw - 3;
                    if ((unsigned)w >= (unsigned)Win) continue;
                    const int tap = (dt * 7 + dh) * 7 + dw;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float v = x[((((long)b * 3 + c) * Tin + t) * Hin + h) * Win + w];
                        const float4* wr = reinterpret_cast<const float4*>(wl + ((tap * 3 + c) * C0 + 16 * g));
#pragma unroll
                        for (int j4 = 0; j4 < 4; ++j4) {
                            const float4 w4 = wr[j4];
                            acc[4 * j4] = fmaf(v, w4.x, acc[4 * j4]);
                            acc[4 * j4 + 1] = fmaf(v, w4.y, acc[4 * j4 + 1]);
                            acc[4 * j4 + 2] = fmaf(v, w4.z, acc[4 * j4 + 2]);
                            acc[4 * j4 + 3] = fmaf(v, w4.w, acc[4 * j4 + 3]);
                        }
                    }
                }
            }
        }
        float4* o = reinterpret_cast<float4*>(out + p * C0 + 16 * g);
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) o[j4] = make_float4(acc[4 * j4], acc[4 * j4 + 1], acc[4 * j4 + 2], acc[4 * j4 + 3]);
    }
}

// Space-to-depth for the strided 3x3x3 convs: a stride-2 conv with pad 1 reads x[2o + d - 1], d = 0..2, i.e. the ODD
// phase at shifts (-1, 0) and the EVEN phase at shift 0.  With X'[o][phase p][c] = x[2o + p][c] it becomes a STRIDE-1 conv
// with a 2-tap kernel (offsets -1, 0; the even phase's -1 tap is zero) over P x C channels -- which runs on the split-fp16
// matrix-core kernel (27 of its 8 x 8 = 64 tap-phase products are non-zero; still 4x faster than the strided fp32 path).
// in: fp32 channels-last [B][T][H][W][C]; out: hl16 [B][T/st][H/2][W/2][P*C], P = st*4, phase index (pt*2 + ph)*2 + pw.
__global__ __launch_bounds__(256) void enc_s2d_hl16_kernel(const float* __restrict__ x, char* __restrict__ out, int B, int T, int H,
                                                           int W, int C, int st) {
    typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
    const int C8 = C >> 3, To = T / st, Ho = H / 2, Wo = W / 2, P = st * 4;
    const long total = (long)B * To * Ho * Wo * P * C8;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c8 = (int)(i % C8);
        long q = i / C8;
        const int p = (int)(q % P); q /= P;
        const int wo = (int)(q % Wo); q /= Wo;
        const int ho = (int)(q % Ho); q /= Ho;
        const int to = (int)(q % To);
        const int b = (int)(q / To);
        const int pw = p & 1, ph = (p >> 1) & 1, pt = p >> 2;
        const float* src = x + ((((long)b * T + to * st + pt) * H + 2 * ho + ph) * W + 2 * wo + pw) * C + 8 * c8;
        const float4 v0 = *reinterpret_cast<const float4*>(src), v1 = *reinterpret_cast<const float4*>(src + 4);
        const float r[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
        half8_t hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const _Float16 hh = (_Float16)r[j];
            hi[j] = hh;
            lo[j] = (_Float16)(r[j] - (float)hh);
        }
        char* o = out + i * 32;  // flat (b, to, ho, wo, p, c8) order == channels-last with channel index p*C + 8*c8
        *reinterpret_cast<half8_t*>(o) = hi;
        *reinterpret_cast<half8_t*>(o + 16) = lo;
    }
}

// eps*std + mu with std = exp(0.5 logvar)  (Encoder.reparameterize, resnet3D.py:199-203); ml = [B][2z] = (mu | logvar)
__global__ void reparam_kernel(const float* __restrict__ ml, const float* __restrict__ eps, float* __restrict__ sample,
                               float* __restrict__ mu, float* __restrict__ logvar, int B, int z) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < B * z; i += gridDim.x * blockDim.x) {
        const int b = i / z, j = i % z;
        const float m = ml[(long)b * 2 * z + j], lv = ml[(long)b * 2 * z + z + j];
        mu[i] = m;
        logvar[i] = lv;
        if (sample) sample[i] = fmaf(eps[i], expf(0.5f * lv), m);
    }
}

// MaxPool2d(kernel 3, stride 2, padding 1) on channels-last [B][H][W][C] -> [B][H/2][W/2][C]
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W,
                                                         int C) {
    const int C4 = C >> 2, Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % Wo); p /= Wo;
        const int ho = (int)(p % Ho);
        const int b = (int)(p / Ho);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int dh = -1; dh <= 1; ++dh)
            for (int dw = -1; dw <= 1; ++dw) {
                const int h = 2 * ho + dh, w = 2 * wo + dw;
                if ((unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W) {
                    const float4 v = *reinterpret_cast<const float4*>(x + (((long)b * H + h) * W + w) * C + 4 * c4);
                    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
                }
            }
        *reinterpret_cast<float4*>(out + i * 4) = m;
    }
}

// AdaptiveAvgPool2d((1,1)) from the fused statistics: mean[b][c] = sum / P
__global__ void mean_from_sums_kernel(const double* __restrict__ sums, float* __restrict__ out, long n, double inv_count) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = (float)(sums[2 * i] * inv_count);
}

namespace {

// weights [N][C][3][3][3] of a stride-(st,2,2) conv -> [N][P*C][kt][2][2] of the equivalent stride-1 conv on the
// space-to-depth input (see enc_s2d_hl16_kernel): per strided dim, tap shift -1 <- (odd phase, w[0]); shift 0 <- (even
// phase, w[1]) and (odd phase, w[2]).  A dim with stride 1 keeps its three taps.
int pack_s2d(const float* w, int N, int C, int st, Conv16Weights& out) {
    const int P = st * 4, kt = st == 2 ? 2 : 3;
    std::vector<float> w2((size_t)N * P * C * kt * 4, 0.f);
    auto src_tap = [](int phase, int shift) { return phase == 0 ? (shift == 1 ? 1 : -1) : (shift == 0 ? 0 : 2); };  // shift idx 0: -1, 1: 0
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < C; ++c)
            for (int pt = 0; pt < st; ++pt)
                for (int ph = 0; ph < 2; ++ph)
                    for (int pw = 0; pw < 2; ++pw)
                        for (int it = 0; it < kt; ++it)
                            for (int ih = 0; ih < 2; ++ih)
                                for (int iw = 0; iw < 2; ++iw) {
                                    const int dt = st == 2 ? src_tap(pt, it) : it, dh = src_tap(ph, ih), dw = src_tap(pw, iw);
                                    if (dt < 0 || dh < 0 || dw < 0) continue;
                                    const int p = (pt * 2 + ph) * 2 + pw;
                                    w2[(((size_t)n * P * C + (size_t)p * C + c) * kt + it) * 4 + ih * 2 + iw] =
                                        w[((size_t)n * C + c) * 27 + (dt * 3 + dh) * 3 + dw];
                                }
    return out.pack(w2.data(), nullptr, N, P * C, kt, 2, 2, 1.0);
}

}  // namespace

int ResConv::pack(const float* w, int cout, int cin, int kt, int kh, int kw, int ss, int st, const float* bias) {
    form = res_conv_form(kt, kh, ss, st);
    if (form == RC_F16) return w16[0].pack(w, bias, cout, cin, kt, kh, kw, 1.0);
    if (form == RC_F32) return w32.pack(w, bias, cout, cin, kt, kh, kw, 1.0);
    if (int rc = pack_s2d(w, cout, cin, st, w16[0])) return rc;
    return st == 2 ? pack_s2d(w, cout, cin, 1, w16[1]) : I2V_OK;
}

int ResConv::run(const ResStep& s, const ResBufs& b, int B, hipStream_t st) const {
    if (form == RC_F32)
        return conv_forward(w32, b.at(s.src), s.cin, b.at(s.dst), nullptr, 1, 1, B, s.out.T, s.out.H, s.out.W, EPI_NONE, st, nullptr, s.ss, s.st);
    return conv16_forward(w16[s.set], b.at<void>(s.src), b.at(s.dst), nullptr, 1, 1, B, s.out.T, s.out.H, s.out.W, EPI_NONE, st);
}

int launch(const ResnetPlan& plan, const std::vector<ResConv>& convs, const std::vector<ResNorm>& norms, const ResBufs& b, hipStream_t st) {
    const int B = plan.B;
    double* sums = b.at<double>(RB_SUMS);
    float* coef = b.at(RB_COEF);
    int rc;
    for (const ResStep& s : plan.steps) {
        const long P = s.out.pos();
        switch (s.kind) {
        case RS_STEM: {
            static bool attr[I2V_MAX_DEV] = {};
            if ((rc = ensure_dynamic_lds(reinterpret_cast<const void*>(enc_stem_kernel), 160 * 1024, attr))) return rc;
            hipLaunchKernelGGL(enc_stem_kernel, dim3(1024), dim3(256), (size_t)147 * 3 * s.C * 4, st, b.at(s.src), b.stem_w, b.at(s.dst), B,
                               s.in.T, s.in.H, s.in.W, s.out.T, s.out.H, s.out.W, s.C);
            I2V_HIP_CHECK(hipGetLastError());
            break;
        }
        case RS_RESIZE:   // NCHW -> channels-last, 3 -> 16 zero-padded
            if ((rc = resize_forward(b.at(s.src), b.at(s.dst), B, s.in.H, s.in.W, s.out.H, s.out.W, st))) return rc;
            break;
        case RS_S2D: {
            const long tot = (long)B * P * (s.st * 4) * (s.cin / 8);
            hipLaunchKernelGGL(enc_s2d_hl16_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 16384)), dim3(256), 0, st, b.at(s.src),
                               b.at<char>(s.dst16), B, s.in.T, s.in.H, s.in.W, s.cin, s.st);
            I2V_HIP_CHECK(hipGetLastError());
            break;
        }
        case RS_CONV:
        case RS_HEAD:
            if ((rc = convs[s.unit].run(s, b, B, st))) return rc;
            break;
        case RS_NORM: {
            const ResNorm& n = norms[s.unit];
            const float* ab = coef;
            long cstride = s.C;
            if (plan.norm == RN_BATCH) {   // constants folded at load
                ab = n.w.as<float>();
                cstride = 0;
            } else {   // statistics of this sample: GroupNorm(16, affine), or InstanceNorm2d(affine=False) per channel
                if ((rc = stats_forward(b.at(s.src), sums, B, P, s.C, st))) return rc;
                if ((rc = coef_forward(sums, coef, B, s.C, plan.norm == RN_GROUP16 ? 16 : s.C, (double)P, st, n.w.as<float>(), n.b.as<float>())))
                    return rc;
            }
            if ((rc = norm_act_forward(b.at(s.src), ab, cstride, b.at(s.res), b.at(s.dst), B, P, s.C, s.relu, st, b.at<void>(s.dst16)))) return rc;
            break;
        }
        case RS_MAXPOOL: {
            const long tot = (long)B * P * (s.C / 4);
            hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)std::min<long>((tot + 255) / 256, 65536)), dim3(256), 0, st, b.at(s.src),
                               b.at(s.dst), B, s.in.H, s.in.W, s.C);
            I2V_HIP_CHECK(hipGetLastError());
            break;
        }
        case RS_MEAN:
            if ((rc = stats_forward(b.at(s.src), sums, B, s.in.pos(), s.C, st))) return rc;
            hipLaunchKernelGGL(mean_from_sums_kernel, dim3((unsigned)(((long)B * s.C + 255) / 256)), dim3(256), 0, st, sums, b.at(s.dst),
                               (long)B * s.C, 1.0 / ((double)s.in.H * s.in.W));
            I2V_HIP_CHECK(hipGetLastError());
            break;
        case RS_REPARAM:
            hipLaunchKernelGGL(reparam_kernel, dim3((B * s.C + 255) / 256), dim3(256), 0, st, b.at(s.src), b.at(RB_EPS), b.at(RB_SAMPLE),
                               b.at(RB_MU), b.at(RB_LOGVAR), B, s.C);
            I2V_HIP_CHECK(hipGetLastError());
            break;
        }
    }
    return I2V_OK;
}

}  // namespace i2v
