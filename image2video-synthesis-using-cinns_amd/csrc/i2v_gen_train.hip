// What the training path of the stage-1 Generator (stage1_VAE/modules/decoder.py:55-120) needs between and around its six GeneratorBlocks
// (i2v_gblock_train.hip, unchanged): fc with its backward, the nearest up-sampling with its adjoint, and the image head
// tanh(conv_img(lrelu(x))) with its backward.  The C ABI is include/i2v_hip_gen_train.h.  Exact fp32; no atomics, every sum has one owner
// and a fixed order.
//   * fc: K = z_dim is tiny and J = 256 nf large.  Forward, dW and db are one thread per element with a float64 sum in index order; dz
//     reduces over J in slices of GN_FC_SLICE rows (a workgroup per slice and sample), the slices' float64 partials added in slice order.
//   * up-sampling: memory bound; 16-byte accesses along W where the row length allows, a scalar form otherwise.  The adjoint is a gather:
//     one owner per low-resolution element, the box in (dt, dh, dw) order.
//   * the head: conv_img is 3 <- nf, and the trunk's kernels (i2v_train_conv.h) take channel counts that are multiples of 16 on the output
//     side only.  So the three passes run as the passes of the ADJOINT conv c' (3 -> nf, the trunk's stem family: a 3-channel map stored with
//     4 channels) with w'[c][o][tap] = W[o][c][26 - tap]: conv_img's forward is c''s input gradient in its `frames` form, conv_img's input
//     gradient is c''s forward on the 4-channel gy, conv_img's weight gradient is c''s with lrelu(x) in the role of the upstream gradient.
//     Here: the two operand layouts of w' straight from W (every call: the parameters are read in place), the LeakyReLU + layout at the
//     entry, bias + tanh + the [B][T][3][H][W] store, gy with the bias partials, the slope + layout at the exit, dW' back into dW.
#include "i2v_handle.h"
#include "i2v_res3d_trunk.h"
#include "../../include/i2v_hip_gen_train.h"

#include <cstdint>

namespace i2v {
namespace {

constexpr int GN_FC_SLICE = 256;    // rows of fc.weight per slice of dz
constexpr int GN_GY_ROWS = 1024;    // positions per workgroup of the gy kernel: one bias partial each

// ------------------------------------------------------------------------------------------------------------------ fc
// out [B][J] = bias + z [B][K] . w [J][K]^T, each element a float64 sum in k order, rounded once
__global__ __launch_bounds__(256) void gn_fc_fwd_kernel(const float* __restrict__ z, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ out, int B, int J, int K) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)B * J) return;
    const int b = (int)(i / J), j = (int)(i - (long)b * J);
    double acc = (double)bias[j];
    for (int k = 0; k < K; ++k) acc += (double)z[(long)b * K + k] * (double)w[(long)j * K + k];
    out[i] = (float)acc;
}

// dw [J][K] = sum_b g z, db [J] = sum_b g: one thread per element, float64 over the samples in order
__global__ __launch_bounds__(256) void gn_fc_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ z, float* dw, float* db, int B, int J,
                                                          int K, int accumulate) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    const long nw = (long)J * K;
    if (i < nw) {
        const int j = (int)(i / K), k = (int)(i - (long)j * K);
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += (double)g[(long)b * J + j] * (double)z[(long)b * K + k];
        dw[i] = accumulate ? dw[i] + (float)acc : (float)acc;
    } else if (i < nw + J) {
        const int j = (int)(i - nw);
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += (double)g[(long)b * J + j];
        db[j] = accumulate ? db[j] + (float)acc : (float)acc;
    }
}

// partial [B][S][K]: slice s = rows [s GN_FC_SLICE, ...) of sample b.  16 columns x 16 row groups per pass over the columns; a row group
// adds its rows in row order, the groups are added in group order.
__global__ __launch_bounds__(256) void gn_fc_dz_partial_kernel(const float* __restrict__ g, const float* __restrict__ w, double* __restrict__ partial,
                                                               int J, int K) {
    __shared__ double red[256];
    const int tid = threadIdx.x, kk = tid & 15, rg = tid >> 4;
    const int s = blockIdx.x, b = blockIdx.y, S = gridDim.x;
    const int j0 = s * GN_FC_SLICE, j1 = j0 + GN_FC_SLICE < J ? j0 + GN_FC_SLICE : J;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int k = k0 + kk;
        double acc = 0.0;
        if (k < K)
            for (int j = j0 + rg; j < j1; j += 16) acc += (double)g[(long)b * J + j] * (double)w[(long)j * K + k];
        red[tid] = acc;
        __syncthreads();
        if (tid < 16 && k < K) {
            double t = 0.0;
            for (int r = 0; r < 16; ++r) t += red[r * 16 + tid];
            partial[((long)b * S + s) * K + k] = t;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void gn_fc_dz_final_kernel(const double* __restrict__ partial, float* __restrict__ dz, int B, int S, int K) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * K) return;
    const int b = i / K, k = i - b * K;
    double t = 0.0;
    for (int s = 0; s < S; ++s) t += partial[((long)b * S + s) * K + k];
    dz[i] = (float)t;
}

// ------------------------------------------------------------------------------------------------------------------ up-sampling
struct GnUpArgs {
    const float* in;
    float* out;
    long total;          // threads' items
    int T, H, W;         // the LOW resolution
    int ut, us;
};

// one output element per item
__global__ __launch_bounds__(256) void gn_up_fwd_kernel(GnUpArgs a) {
    const int Wo = a.W * a.us, Ho = a.H * a.us, To = a.T * a.ut;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += gridDim.x * 256L) {
        long r = i;
        const int wo = (int)(r % Wo); r /= Wo;
        const int ho = (int)(r % Ho); r /= Ho;
        const int to = (int)(r % To); r /= To;
        a.out[i] = a.in[((r * a.T + to / a.ut) * a.H + ho / a.us) * a.W + wo / a.us];
    }
}

// four output elements along W per item: one 16-byte store (W us a multiple of 4, 16-byte aligned maps)
template <int US>
__global__ __launch_bounds__(256) void gn_up_fwd4_kernel(GnUpArgs a) {
    const int Wq = a.W * US / 4, Ho = a.H * US, To = a.T * a.ut;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += gridDim.x * 256L) {
        long r = i;
        const int q = (int)(r % Wq); r /= Wq;
        const int ho = (int)(r % Ho); r /= Ho;
        const int to = (int)(r % To); r /= To;
        const float* src = a.in + ((r * a.T + to / a.ut) * a.H + ho / US) * a.W;
        float4 v;
        if constexpr (US == 1) {
            v = *reinterpret_cast<const float4*>(src + 4 * q);
        } else if constexpr (US == 2) {
            const float2 s = *reinterpret_cast<const float2*>(src + 2 * q);
            v = make_float4(s.x, s.x, s.y, s.y);
        } else {
            const float s = src[q];
            v = make_float4(s, s, s, s);
        }
        *reinterpret_cast<float4*>(a.out + 4 * i) = v;
    }
}

// the adjoint, one low-resolution element per item: the box in (dt, dh, dw) order in fp32
__global__ __launch_bounds__(256) void gn_up_bwd_kernel(GnUpArgs a) {
    const int Wo = a.W * a.us, Ho = a.H * a.us, To = a.T * a.ut;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += gridDim.x * 256L) {
        long r = i;
        const int w = (int)(r % a.W); r /= a.W;
        const int h = (int)(r % a.H); r /= a.H;
        const int t = (int)(r % a.T); r /= a.T;
        float acc = 0.f;
        for (int dt = 0; dt < a.ut; ++dt)
            for (int dh = 0; dh < a.us; ++dh) {
                const float* src = a.in + ((r * To + t * a.ut + dt) * Ho + h * a.us + dh) * Wo + (long)w * a.us;
                for (int dw = 0; dw < a.us; ++dw) acc += src[dw];
            }
        a.out[i] = acc;
    }
}

// 4 / US low-resolution elements along W per item: every row of the box is one 16-byte load (W a multiple of 4 / US, 16-byte aligned maps)
template <int US>
__global__ __launch_bounds__(256) void gn_up_bwd4_kernel(GnUpArgs a) {
    constexpr int V = 4 / US;
    const int Wv = a.W / V, Wo = a.W * US, Ho = a.H * US, To = a.T * a.ut;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < a.total; i += gridDim.x * 256L) {
        long r = i;
        const int q = (int)(r % Wv); r /= Wv;
        const int h = (int)(r % a.H); r /= a.H;
        const int t = (int)(r % a.T); r /= a.T;
        float acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = 0.f;
        for (int dt = 0; dt < a.ut; ++dt)
#pragma unroll
            for (int dh = 0; dh < US; ++dh) {
                const float4 v = *reinterpret_cast<const float4*>(a.in + ((r * To + t * a.ut + dt) * Ho + h * US + dh) * Wo + 4 * q);
                if constexpr (US == 1) { acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w; }
                else if constexpr (US == 2) { acc[0] += v.x; acc[0] += v.y; acc[1] += v.z; acc[1] += v.w; }
                else { acc[0] += v.x; acc[0] += v.y; acc[0] += v.z; acc[0] += v.w; }
            }
        float* dst = a.out + V * i;
        if constexpr (US == 1) *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        else if constexpr (US == 2) *reinterpret_cast<float2*>(dst) = make_float2(acc[0], acc[1]);
        else dst[0] = acc[0];
    }
}

// ------------------------------------------------------------------------------------------------------------------ the head
// W [3][nf][27] -> the operand layouts of the adjoint conv w'[c][o][tap] = W[o][c][26 - tap]: wd [27][16][nf] (its input gradient =
// conv_img's forward; rows 3 .. 15 are zero) and wf [27][nf][4] (its forward = conv_img's input gradient; column 3 is zero)
__global__ __launch_bounds__(256) void gn_head_pack_kernel(const float* __restrict__ w, float* __restrict__ wd, float* __restrict__ wf, int nf) {
    const long total = 27L * 16 * nf;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += gridDim.x * 256L) {
        const int c = (int)(e % nf), o = (int)((e / nf) % 16), tap = (int)(e / (16L * nf));
        const float v = o < 3 ? w[((long)o * nf + c) * 27 + 26 - tap] : 0.f;
        wd[e] = v;
        if (o < 4) wf[((long)tap * nf + c) * 4 + o] = v;
    }
}

// [B][R][S] -> [B][S][R] through LDS, both sides coalesced.  MODE 0: out = lrelu(in) (the entry: [B][C][P] -> [B][P][C]);
// MODE 1: out = in * slope(act), act of in's shape (the exit: [B][P][C] -> [B][C][P]; at exactly 0 the slope is 0.2)
template <int MODE>
__global__ __launch_bounds__(256) void gn_transpose_kernel(const float* __restrict__ in, const float* __restrict__ act, float* __restrict__ out, int R,
                                                           int S) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 32, s0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long base = (long)b * R * S;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && s0 + tx < S) {
            const long o = base + (long)(r0 + i) * S + s0 + tx;
            float v = in[o];
            if constexpr (MODE == 0) v = v > 0.f ? v : 0.2f * v;
            else v = act[o] > 0.f ? v : 0.2f * v;
            tile[i][tx] = v;
        }
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (s0 + i < S && r0 + tx < R) out[base + (long)(s0 + i) * R + r0 + tx] = tile[tx][i];
}

// pre [B][3][T][HW] (the conv without bias) -> y [B][T][3][HW] = tanh(pre + bias), formed in float64 and rounded once; into `out` and,
// where kept, into `keep`.  VEC: four elements along HW per item.
template <bool VEC>
__global__ __launch_bounds__(256) void gn_head_out_kernel(const float* __restrict__ pre, const float* __restrict__ bias, float* __restrict__ out,
                                                          float* __restrict__ keep, long total, int T, long HW) {
    constexpr int V = VEC ? 4 : 1;
    const long HWv = HW / V;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        long r = i;
        const long p = (r % HWv) * V; r /= HWv;
        const int o = (int)(r % 3); r /= 3;
        const int t = (int)(r % T); r /= T;
        const float* src = pre + ((r * 3 + o) * T + t) * HW + p;
        const double bv = (double)bias[o];
        if constexpr (VEC) {
            const float4 v = *reinterpret_cast<const float4*>(src);
            const float4 y = make_float4((float)tanh((double)v.x + bv), (float)tanh((double)v.y + bv), (float)tanh((double)v.z + bv),
                                         (float)tanh((double)v.w + bv));
            *reinterpret_cast<float4*>(out + 4 * i) = y;
            if (keep) *reinterpret_cast<float4*>(keep + 4 * i) = y;
        } else {
            const float y = (float)tanh((double)src[0] + bv);
            out[i] = y;
            if (keep) keep[i] = y;
        }
    }
}

// g, y [B][T][3][HW] -> gy4 [B][T][HW][4] = (g (1 - y y) in fp32, as torch forms it; 0), and per workgroup (GN_GY_ROWS positions) the
// float64 sums of its three channels -> partial [workgroup][4]
__global__ __launch_bounds__(256) void gn_head_gy_kernel(const float* __restrict__ g, const float* __restrict__ y, float* __restrict__ gy4,
                                                         double* __restrict__ partial, long rows, long HW) {
    __shared__ double red[256];
    const long r0 = (long)blockIdx.x * GN_GY_ROWS;
    double s[3] = {0.0, 0.0, 0.0};
    for (int u = 0; u < GN_GY_ROWS / 256; ++u) {
        const long row = r0 + u * 256 + threadIdx.x;      // (b t) HW + p
        if (row >= rows) break;
        const long bt = row / HW, p = row - bt * HW;
        float v[3];
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const long idx = (bt * 3 + o) * HW + p;
            const float yv = y[idx];
            v[o] = __fmul_rn(g[idx], __fsub_rn(1.f, __fmul_rn(yv, yv)));   // three roundings, never contracted
            s[o] += (double)v[o];
        }
        *reinterpret_cast<float4*>(gy4 + 4 * row) = make_float4(v[0], v[1], v[2], 0.f);
    }
    if (!partial) return;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const double t = block_sum(s[o], red);
        if (threadIdx.x == 0) partial[(long)blockIdx.x * 4 + o] = t;
    }
}

// db [3] = the workgroups' partial sums: a thread's share in index order, the threads by block_sum's tree; rounded once
__global__ __launch_bounds__(256) void gn_head_bias_final_kernel(const double* __restrict__ partial, float* db, long nblk, int accumulate) {
    __shared__ double red[256];
    for (int o = 0; o < 3; ++o) {
        double s = 0.0;
        for (long i = threadIdx.x; i < nblk; i += 256) s += partial[i * 4 + o];
        s = block_sum(s, red);
        if (threadIdx.x == 0) db[o] = accumulate ? db[o] + (float)s : (float)s;
    }
}

// dW [3][nf][27] (+)= dW' [nf][3][27] with the taps flipped back
__global__ __launch_bounds__(256) void gn_head_dw_kernel(const float* __restrict__ dwp, float* dw, int nf, int accumulate) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 81 * nf) return;
    const int tap = e % 27, c = (e / 27) % nf, o = e / (27 * nf);
    const float v = dwp[((long)c * 3 + o) * 27 + 26 - tap];
    dw[e] = accumulate ? dw[e] + v : v;
}

// =================================================================================================================== host side
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool factor_ok(int f) { return f == 1 || f == 2 || f == 4; }
int fc_slices(int J) { return (J + GN_FC_SLICE - 1) / GN_FC_SLICE; }

int launch_fc_fwd(const float* z, const float* w, const float* bias, int B, int J, int K, float* out, hipStream_t st) {
    const long nblk = ((long)B * J + 255) / 256;
    I2V_REQUIRE(nblk < (1L << 31), I2V_E_INVALID, "generator fc: grid of %ld workgroups", nblk);
    hipLaunchKernelGGL(gn_fc_fwd_kernel, dim3((unsigned)nblk), dim3(256), 0, st, z, w, bias, out, B, J, K);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_fc_bwd(const float* g, const float* z, const float* w, int B, int J, int K, float* dw, float* db, float* dz, bool accumulate, void* ws,
                  hipStream_t st) {
    if (dw) {
        const long nblk = ((long)J * K + J + 255) / 256;
        I2V_REQUIRE(nblk < (1L << 31), I2V_E_INVALID, "generator fc: weight-gradient grid of %ld workgroups", nblk);
        hipLaunchKernelGGL(gn_fc_wgrad_kernel, dim3((unsigned)nblk), dim3(256), 0, st, g, z, dw, db, B, J, K, accumulate ? 1 : 0);
        I2V_LAUNCHED();
    }
    if (dz) {
        const int S = fc_slices(J);
        I2V_REQUIRE(B <= 65535, I2V_E_INVALID, "generator fc: batch %d", B);
        double* partial = static_cast<double*>(ws);
        hipLaunchKernelGGL(gn_fc_dz_partial_kernel, dim3(S, B), dim3(256), 0, st, g, w, partial, J, K);
        I2V_LAUNCHED();
        hipLaunchKernelGGL(gn_fc_dz_final_kernel, dim3((B * K + 255) / 256), dim3(256), 0, st, partial, dz, B, S, K);
        I2V_LAUNCHED();
    }
    return I2V_OK;
}

size_t fc_ws_bytes(int B, int J, int K) {
    if (B <= 0 || B > 65535 || J <= 0 || K <= 0 || (long)B * J >= (1L << 31) || (long)J * K >= (1L << 31)) return 0;
    return align_up((size_t)B * fc_slices(J) * K * 8, 256);
}

TcConv head_conv(int nf) { return TcConv{3, 4, 16, nf, 3, 3, 3, 1, 1, 0}; }   // the adjoint conv 3 -> nf

struct GnHeadLayout {
    bool ok = false;
    long P = 0, HW = 0, BP = 0, gy_blocks = 0;
    TcGeo geo{};
    size_t a_cl = 0, y = 0, saved_total = 0;                                                      // saved
    size_t wd = 0, wf = 0, pre = 0, gy4 = 0, dxa = 0, part = 0, dwn = 0, dotp = 0, bpart = 0, a_tmp = 0, ws_total = 0;   // workspace
};

GnHeadLayout head_layout(int nf, int B, int T, int H, int W) {
    GnHeadLayout y;
    if (nf < 16 || nf > 1024 || nf % 16 || B <= 0 || B > 65535 || T <= 0 || H <= 0 || W <= 0) return y;
    const long P = (long)T * H * W, BP = B * P;
    if (BP * nf >= (1L << 31) || (P + 31) / 32 > 65535) return y;   // (the transposes' grid.y)
    y.P = P; y.HW = (long)H * W; y.BP = BP; y.gy_blocks = (BP + GN_GY_ROWS - 1) / GN_GY_ROWS;
    const TcConv c = head_conv(nf);
    y.geo = make_geo(B, T, H, W, c);
    Carver s;
    y.a_cl = s.take_floats((size_t)BP * nf);
    y.y = s.take_floats((size_t)BP * 3);
    y.saved_total = s.total();
    const size_t E = (size_t)nf * 81;
    Carver k;
    y.wd = k.take_floats((size_t)27 * 16 * nf);
    y.wf = k.take_floats((size_t)27 * nf * 4);
    y.pre = k.take_floats((size_t)BP * 3);
    y.gy4 = k.take_floats((size_t)BP * 4);
    y.dxa = k.take_floats((size_t)BP * nf);
    y.part = k.take_floats(wgrad_part_floats(c, y.geo.mo));
    y.dwn = k.take_floats(E);
    y.dotp = k.take_bytes(((E + 255) / 256 + 1) * 8);
    y.bpart = k.take_bytes((size_t)y.gy_blocks * 4 * 8);
    y.a_tmp = k.take_floats((size_t)BP * nf);   // lrelu(x) of a forward that keeps nothing
    y.ws_total = k.total();
    y.ok = true;
    return y;
}

template <int MODE>
int launch_gn_transpose(const float* in, const float* act, float* out, int B, long R, long S, hipStream_t st) {
    const long gy = (R + 31) / 32, gx = (S + 31) / 32;
    I2V_REQUIRE(B <= 65535 && gy <= 65535 && gx < (1L << 31), I2V_E_INVALID, "generator head: transpose grid (%ld, %ld, %d)", gx, gy, B);
    hipLaunchKernelGGL((gn_transpose_kernel<MODE>), dim3((unsigned)gx, (unsigned)gy, B), dim3(256), 0, st, in, act, out, (int)R, (int)S);
    I2V_LAUNCHED();
    return I2V_OK;
}

int head_forward(const float* x, const float* w, const float* bias, int nf, int B, int T, int H, int W, float* out, void* saved, size_t saved_bytes,
                 void* ws, size_t ws_bytes, hipStream_t st, const char* what) {
    const GnHeadLayout y = head_layout(nf, B, T, H, W);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: nf %d (a multiple of 16 in [16, 1024]), batch %d, map %d x %d x %d", what, nf, B, T, H, W);
    I2V_REQUIRE_WORKSPACE(ws_bytes, y.ws_total, what);
    if (saved) I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    I2V_REQUIRE(aligned16(w) && aligned16(out) && aligned16(ws) && aligned16(saved), I2V_E_INVALID, "%s: buffers must be 16-byte aligned", what);
    const TcConv c = head_conv(nf);
    float* a_cl = saved ? Carver::at(saved, y.a_cl) : Carver::at(ws, y.a_tmp);
    float* keep = saved ? Carver::at(saved, y.y) : nullptr;
    float *wd = Carver::at(ws, y.wd), *wf = Carver::at(ws, y.wf), *pre = Carver::at(ws, y.pre);
    int rc;
    if ((rc = launch_gn_transpose<0>(x, nullptr, a_cl, B, nf, y.P, st))) return rc;
    hipLaunchKernelGGL(gn_head_pack_kernel, dim3(grid_for(27L * 16 * nf)), dim3(256), 0, st, w, wd, wf, nf);
    I2V_LAUNCHED();
    if ((rc = launch_dgrad<Trunk3d>(c, a_cl, nullptr, nullptr, wd, nullptr, nullptr, pre, true, B, y.geo, st))) return rc;
    const long total = y.BP * 3;
    if (y.HW % 4 == 0) hipLaunchKernelGGL((gn_head_out_kernel<true>), dim3(grid_for(total / 4)), dim3(256), 0, st, pre, bias, out, keep, total / 4, T, y.HW);
    else hipLaunchKernelGGL((gn_head_out_kernel<false>), dim3(grid_for(total)), dim3(256), 0, st, pre, bias, out, keep, total, T, y.HW);
    I2V_LAUNCHED();
    return I2V_OK;
}

int head_backward(const float* g, const void* saved, size_t saved_bytes, const float* w, int nf, int B, int T, int H, int W, bool accumulate, float* dx,
                  float* dw, float* db, void* ws, size_t ws_bytes, hipStream_t st, const char* what) {
    const GnHeadLayout y = head_layout(nf, B, T, H, W);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: nf %d (a multiple of 16 in [16, 1024]), batch %d, map %d x %d x %d", what, nf, B, T, H, W);
    I2V_REQUIRE(dx || dw, I2V_E_INVALID, "%s: neither dx nor the parameter gradients are wanted", what);
    I2V_REQUIRE(!dw == !db, I2V_E_INVALID, "%s: dw and db come together", what);
    I2V_REQUIRE_WORKSPACE(ws_bytes, y.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    I2V_REQUIRE(aligned16(w) && aligned16(ws) && aligned16(saved), I2V_E_INVALID, "%s: buffers must be 16-byte aligned", what);
    I2V_REQUIRE(y.gy_blocks < (1L << 31), I2V_E_INVALID, "%s: gy grid of %ld workgroups", what, y.gy_blocks);
    const TcConv c = head_conv(nf);
    void* sv = const_cast<void*>(saved);
    const float *a_cl = Carver::at(sv, y.a_cl), *yk = Carver::at(sv, y.y);
    float *wd = Carver::at(ws, y.wd), *wf = Carver::at(ws, y.wf), *gy4 = Carver::at(ws, y.gy4), *dxa = Carver::at(ws, y.dxa);
    double* bpart = Carver::at<double>(ws, y.bpart);
    int rc;
    hipLaunchKernelGGL(gn_head_gy_kernel, dim3((unsigned)y.gy_blocks), dim3(256), 0, st, g, yk, gy4, dw ? bpart : nullptr, y.BP, y.HW);
    I2V_LAUNCHED();
    if (dw) {
        hipLaunchKernelGGL(gn_head_bias_final_kernel, dim3(1), dim3(256), 0, st, bpart, db, y.gy_blocks, accumulate ? 1 : 0);
        I2V_LAUNCHED();
        // dW'[c][o][tap] = sum over the positions of lrelu(x)[c] gy[o]: the adjoint conv's weight gradient with lrelu(x) as its upstream
        // gradient (W only stands in as the operand of the finish pass's inner product, which nobody reads without a sigma)
        float* dwn = Carver::at(ws, y.dwn);
        if ((rc = launch_wgrad<Trunk3d>(c, a_cl, nullptr, nullptr, gy4, w, nullptr, nullptr, nullptr, Carver::at(ws, y.part), dwn,
                                        Carver::at<double>(ws, y.dotp), dwn, false, y.geo, st)))
            return rc;
        hipLaunchKernelGGL(gn_head_dw_kernel, dim3((81 * nf + 255) / 256), dim3(256), 0, st, dwn, dw, nf, accumulate ? 1 : 0);
        I2V_LAUNCHED();
    }
    if (dx) {
        hipLaunchKernelGGL(gn_head_pack_kernel, dim3(grid_for(27L * 16 * nf)), dim3(256), 0, st, w, wd, wf, nf);
        I2V_LAUNCHED();
        if ((rc = launch_conv<Trunk3d>(c, gy4, wf, dxa, y.geo, st))) return rc;
        if ((rc = launch_gn_transpose<1>(dxa, a_cl, dx, B, y.P, nf, st))) return rc;
    }
    return I2V_OK;
}

int upsample(bool backward, const float* in, long planes, int T, int H, int W, int ut, int us, float* out, hipStream_t st, const char* what) {
    I2V_REQUIRE(in && out && planes > 0 && T > 0 && H > 0 && W > 0, I2V_E_INVALID, "%s: null argument or an empty map", what);
    I2V_REQUIRE(factor_ok(ut) && factor_ok(us), I2V_E_INVALID, "%s: factors (%d, %d, %d): each of ut, us must be 1, 2 or 4", what, ut, us, us);
    const long lo = planes * T * H * W, hi = lo * ut * us * us;
    I2V_REQUIRE(hi / ((long)ut * us * us) == lo && hi < (1L << 40), I2V_E_INVALID, "%s: %ld planes of %d x %d x %d by (%d, %d, %d)", what, planes, T, H, W,
                ut, us, us);
    GnUpArgs a{in, out, 0, T, H, W, ut, us};
    const bool al = aligned16(in) && aligned16(out);
    if (!backward) {
        if (al && (W * us) % 4 == 0) {
            a.total = hi / 4;
            const dim3 grid(grid_for(a.total));
            if (us == 1) hipLaunchKernelGGL((gn_up_fwd4_kernel<1>), grid, dim3(256), 0, st, a);
            else if (us == 2) hipLaunchKernelGGL((gn_up_fwd4_kernel<2>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((gn_up_fwd4_kernel<4>), grid, dim3(256), 0, st, a);
        } else {
            a.total = hi;
            hipLaunchKernelGGL(gn_up_fwd_kernel, dim3(grid_for(a.total)), dim3(256), 0, st, a);
        }
    } else {
        const int V = 4 / us;
        if (al && W % V == 0) {
            a.total = lo / V;
            const dim3 grid(grid_for(a.total));
            if (us == 1) hipLaunchKernelGGL((gn_up_bwd4_kernel<1>), grid, dim3(256), 0, st, a);
            else if (us == 2) hipLaunchKernelGGL((gn_up_bwd4_kernel<2>), grid, dim3(256), 0, st, a);
            else hipLaunchKernelGGL((gn_up_bwd4_kernel<4>), grid, dim3(256), 0, st, a);
        } else {
            a.total = lo;
            hipLaunchKernelGGL(gn_up_bwd_kernel, dim3(grid_for(a.total)), dim3(256), 0, st, a);
        }
    }
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_gen_train {
    int device = 0;
    bool loaded = false, have_grads = false;
    int nf = 0, z_dim = 0;
    float *fw = nullptr, *fb = nullptr, *cw = nullptr, *cb = nullptr;
    float *gfw = nullptr, *gfb = nullptr, *gcw = nullptr, *gcb = nullptr;
};

namespace {

bool gen_bind_keys(const i2v_gen_train* g, const StateDict& sd, float** fw, float** fb, float** cw, float** cb) {
    const int64_t J = (int64_t)256 * g->nf;
    const float* p[4] = {sd.f32("fc.weight", J * g->z_dim), nullptr, nullptr, nullptr};
    if (!p[0] || !(p[1] = sd.f32("fc.bias", J)) || !(p[2] = sd.f32("conv_img.weight", (int64_t)81 * g->nf)) || !(p[3] = sd.f32("conv_img.bias", 3)))
        return false;
    *fw = const_cast<float*>(p[0]); *fb = const_cast<float*>(p[1]); *cw = const_cast<float*>(p[2]); *cb = const_cast<float*>(p[3]);
    return true;
}

}  // namespace

extern "C" {

int i2v_gen_train_create(int32_t nf, int32_t z_dim, i2v_gen_train** out) {
    const char* what = "i2v_gen_train_create";
    I2V_REQUIRE(out, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(nf >= 16 && nf % 16 == 0 && 16 * nf <= 1024, I2V_E_INVALID,
                "%s: channel_factor %d must be a multiple of 16 with 16 nf <= 1024 (the GeneratorBlocks take channel counts that are multiples of 16)", what,
                nf);
    I2V_REQUIRE(z_dim >= 1, I2V_E_INVALID, "%s: z_dim %d is not positive", what, z_dim);
    return create_handle(what, out, [&](i2v_gen_train* g) {
        g->nf = nf; g->z_dim = z_dim;
        return I2V_OK;
    });
}

void i2v_gen_train_destroy(i2v_gen_train* g) { delete g; }

int i2v_gen_train_bind(i2v_gen_train* g, const i2v_tensor* params, int32_t n) {
    I2V_REQUIRE(g && params && n > 0, I2V_E_INVALID, "i2v_gen_train_bind: null argument");
    g->loaded = false;
    const StateDict sd(params, n);
    if (!gen_bind_keys(g, sd, &g->fw, &g->fb, &g->cw, &g->cb)) return I2V_E_MISSING;
    I2V_REQUIRE(aligned16(g->cw), I2V_E_INVALID, "i2v_gen_train_bind: conv_img.weight must be 16-byte aligned");
    g->loaded = true;
    return I2V_OK;
}

int i2v_gen_train_bind_grads(i2v_gen_train* g, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(g && (grads ? n > 0 : n == 0), I2V_E_INVALID, "i2v_gen_train_bind_grads: null handle, or a count without tensors");
    g->have_grads = false;
    if (!grads) return I2V_OK;
    const StateDict gd(grads, n);
    if (!gen_bind_keys(g, gd, &g->gfw, &g->gfb, &g->gcw, &g->gcb)) return I2V_E_MISSING;
    g->have_grads = true;
    return I2V_OK;
}

size_t i2v_gen_train_fc_workspace_bytes(int32_t batch, int32_t j, int32_t k) { return fc_ws_bytes(batch, j, k); }
size_t i2v_gen_train_head_saved_bytes(int32_t nf, int32_t batch, int32_t t, int32_t h, int32_t w) { return head_layout(nf, batch, t, h, w).saved_total; }
size_t i2v_gen_train_head_workspace_bytes(int32_t nf, int32_t batch, int32_t t, int32_t h, int32_t w) { return head_layout(nf, batch, t, h, w).ws_total; }
int32_t i2v_gen_train_fc_slices(int32_t j) { return j > 0 ? fc_slices(j) : 0; }

int i2v_gen_train_fc_forward(i2v_gen_train* g, const float* z, int32_t batch, float* out, void* stream) {
    const char* what = "i2v_gen_train_fc_forward";
    I2V_ENTER(sc, g, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(z && out && fc_ws_bytes(batch, 256 * g->nf, g->z_dim), I2V_E_INVALID, "%s: null argument, or batch %d", what, batch);
    return launch_fc_fwd(z, g->fw, g->fb, batch, 256 * g->nf, g->z_dim, out, static_cast<hipStream_t>(stream));
}

int i2v_gen_train_fc_backward(i2v_gen_train* g, const float* g_out, const float* z, int32_t batch, float* dz, int32_t param_grads, int32_t accumulate,
                              void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gen_train_fc_backward";
    I2V_ENTER(sc, g, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(g_out && z && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(dz || param_grads, I2V_E_INVALID, "%s: neither dz nor the parameter gradients are wanted", what);
    I2V_REQUIRE(!param_grads || g->have_grads, I2V_E_STATE, "%s: param_grads without bound gradient tensors", what);
    const size_t need = fc_ws_bytes(batch, 256 * g->nf, g->z_dim);
    I2V_REQUIRE(need, I2V_E_INVALID, "%s: batch %d", what, batch);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, what);
    return launch_fc_bwd(g_out, z, g->fw, batch, 256 * g->nf, g->z_dim, param_grads ? g->gfw : nullptr, param_grads ? g->gfb : nullptr, dz, accumulate != 0,
                         workspace, static_cast<hipStream_t>(stream));
}

int i2v_gen_train_head_forward(i2v_gen_train* g, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t flags, float* out, void* saved,
                               size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gen_train_head_forward";
    I2V_ENTER(sc, g, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(x && out && workspace, I2V_E_INVALID, "%s: null argument", what);
    const bool save = flags & I2V_GEN_TRAIN_SAVE;
    I2V_REQUIRE(!save || saved, I2V_E_INVALID, "%s: I2V_GEN_TRAIN_SAVE without a saved buffer", what);
    return head_forward(x, g->cw, g->cb, g->nf, batch, t, h, w, out, save ? saved : nullptr, saved_bytes, workspace, workspace_bytes,
                        static_cast<hipStream_t>(stream), what);
}

int i2v_gen_train_head_backward(i2v_gen_train* g, const float* g_out, const void* saved, size_t saved_bytes, int32_t batch, int32_t t, int32_t h,
                                int32_t w, float* dx, int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gen_train_head_backward";
    I2V_ENTER(sc, g, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(g_out && saved && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(!param_grads || g->have_grads, I2V_E_STATE, "%s: param_grads without bound gradient tensors", what);
    return head_backward(g_out, saved, saved_bytes, g->cw, g->nf, batch, t, h, w, accumulate != 0, dx, param_grads ? g->gcw : nullptr,
                         param_grads ? g->gcb : nullptr, workspace, workspace_bytes, static_cast<hipStream_t>(stream), what);
}

int i2v_gen_train_upsample_forward(const float* x, int64_t planes, int32_t t, int32_t h, int32_t w, int32_t ut, int32_t us, float* out, void* stream) {
    return upsample(false, x, planes, t, h, w, ut, us, out, static_cast<hipStream_t>(stream), "i2v_gen_train_upsample_forward");
}

int i2v_gen_train_upsample_backward(const float* g, int64_t planes, int32_t t, int32_t h, int32_t w, int32_t ut, int32_t us, float* dx, void* stream) {
    return upsample(true, g, planes, t, h, w, ut, us, dx, static_cast<hipStream_t>(stream), "i2v_gen_train_upsample_backward");
}

int i2v_gen_train_fc_forward_unit(const float* z, const float* w, const float* bias, int32_t batch, int32_t j, int32_t k, float* out, void* stream) {
    I2V_REQUIRE(z && w && bias && out && fc_ws_bytes(batch, j, k), I2V_E_INVALID, "i2v_gen_train_fc_forward_unit: bad argument");
    return launch_fc_fwd(z, w, bias, batch, j, k, out, static_cast<hipStream_t>(stream));
}

int i2v_gen_train_fc_backward_unit(const float* g, const float* z, const float* w, int32_t batch, int32_t j, int32_t k, int32_t accumulate, float* dw,
                                   float* db, float* dz, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gen_train_fc_backward_unit";
    const size_t need = fc_ws_bytes(batch, j, k);
    I2V_REQUIRE(g && z && w && workspace && need && (dw || dz) && !dw == !db, I2V_E_INVALID, "%s: bad argument (dw and db come together)", what);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, what);
    return launch_fc_bwd(g, z, w, batch, j, k, dw, db, dz, accumulate != 0, workspace, static_cast<hipStream_t>(stream));
}

int i2v_gen_train_head_forward_unit(const float* x, const float* w, const float* bias, int32_t nf, int32_t batch, int32_t t, int32_t h, int32_t w_,
                                    float* out, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gen_train_head_forward_unit";
    I2V_REQUIRE(x && w && bias && out && workspace, I2V_E_INVALID, "%s: null argument", what);
    return head_forward(x, w, bias, nf, batch, t, h, w_, out, saved, saved_bytes, workspace, workspace_bytes, static_cast<hipStream_t>(stream), what);
}

int i2v_gen_train_head_backward_unit(const float* g, const void* saved, size_t saved_bytes, const float* w, int32_t nf, int32_t batch, int32_t t,
                                     int32_t h, int32_t w_, int32_t accumulate, float* dx, float* dw, float* db, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const char* what = "i2v_gen_train_head_backward_unit";
    I2V_REQUIRE(g && saved && w && workspace, I2V_E_INVALID, "%s: null argument", what);
    return head_backward(g, saved, saved_bytes, w, nf, batch, t, h, w_, accumulate != 0, dx, dw, db, workspace, workspace_bytes,
                         static_cast<hipStream_t>(stream), what);
}

}  // extern "C"
