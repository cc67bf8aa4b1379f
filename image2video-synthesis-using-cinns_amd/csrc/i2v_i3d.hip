// Kinetics-400 I3D (the FVD feature network) and the FVD statistics accumulator.
//
// Replaces metrics/PyTorch_FVD/I3D.py (I3D.forward, Unit3Dpy, MaxPool3dTFPadding, Mixed) and the host path in front of it,
// metrics/PyTorch_FVD/FVD_logging.py:177-203 (preprocess: every frame to the host, a CPU bilinear resize, batches of 20 back).
// Frames stay on the device: the decoder's [B][T][3][H][W] output is resized (bilinear, align_corners=True) to 224 x 224 and
// de-normalised in one kernel that writes the channels-last stem input.
//
// Convolutions: flat_conv_kernel<NT, true> (i2v_flatconv.h) for every unit: cubic windows, stride 1 or 2, the asymmetric "TF SAME"
// padding as padding in front, eval-mode BatchNorm3d folded to (scale, shift) at load and ReLU; the head conv has a bias and no ReLU.
//
// Max pools pad with ZEROS that take part in the maximum (ConstantPad3d(.., 0) in front of MaxPool3d(ceil_mode=True)).
//
// Second variant on the same handle: the dynamic-texture I3D of metrics/DTFVD/ID3.py (length 16) and ID3_32.py (length 32), the DTFVD
// and diversity feature network.  Same topology, same kernels; its own state_dict keys (Conv3d_1a_7x7.bn, Mixed_3b.b1a, logits),
// BatchNorm eps 1e-5, SAME padding by the size % stride rule in all three dimensions (compute_pad; F.pad zeros in front of a
// floor-mode MaxPool3d -- on a SAME-padded extent floor and ceil agree), AvgPool3d((2, 7, 7)) or ((4, 7, 7)).  The metric reads
// get_representation, the average pool's output as [B][1024][T']: i2v_i3d_features stops there, no classifier, no time mean.
// The input stage maps output frame t to source frame t % T_in (calculate_FVD's repeat x 3 then [:16]).
// i2v_diversity_update: the pair loop of metrics/Diversity/I3D.py in float64, one workgroup, fixed order.
#include <algorithm>
#include <cmath>

#include "i2v_flatconv.h"
#include "i2v_handle.h"

namespace i2v {
namespace {

constexpr int I3D_SIDE = 224;

// FVD_logging.preprocess fused with the layout change: frames [N = B T][3][Hi][Wi] -> channels-last [N][224][224][4] (channel 3
// zero), bilinear with align_corners=True in the arithmetic of torch's upsample_bilinear2d, then (x + 1) / 2 when `denorm`.
// Time mapping: output frame t of clip b (N = B Tout) reads source frame b Tin + t % Tin -- DTFVD_Score.calculate_FVD's
// repeat(1, 3, 1, 1, 1)[:, :16]; Tout <= Tin is plain truncation, Tin = Tout = 1 a flat list of N frames.
__global__ __launch_bounds__(256) void i3d_input_kernel(const float* __restrict__ frames, float* __restrict__ out, long N, int Tin, int Tout,
                                                        int Hi, int Wi, int denorm) {
    const long total = N * I3D_SIDE * I3D_SIDE;
    const float sh = (float)(Hi - 1) / (float)(I3D_SIDE - 1), sw = (float)(Wi - 1) / (float)(I3D_SIDE - 1);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int w = (int)(i % I3D_SIDE), h = (int)((i / I3D_SIDE) % I3D_SIDE);
        const long no = i / (I3D_SIDE * I3D_SIDE);
        const long n = no / Tout * Tin + (int)(no % Tout) % Tin;
        const float fh = sh * h, fw = sw * w;
        const int h0 = (int)fh, w0 = (int)fw;
        const int h1 = h0 + (h0 < Hi - 1 ? 1 : 0), w1 = w0 + (w0 < Wi - 1 ? 1 : 0);
        const float lh1 = fh - h0, lh0 = 1.f - lh1, lw1 = fw - w0, lw0 = 1.f - lw1;
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* pl = frames + (n * 3 + c) * (long)Hi * Wi;
            v[c] = lh0 * (lw0 * pl[h0 * Wi + w0] + lw1 * pl[h0 * Wi + w1]) + lh1 * (lw0 * pl[h1 * Wi + w0] + lw1 * pl[h1 * Wi + w1]);
            if (denorm) v[c] = (v[c] + 1.0f) / 2.0f;
        }
        *reinterpret_cast<float4*>(out + i * 4) = make_float4(v[0], v[1], v[2], 0.f);
    }
}

// MaxPool3dTFPadding: ConstantPad3d((p0, p1) per dimension, 0) then MaxPool3d(kernel, stride, ceil_mode=True).  A window position
// inside the padded extent but outside the tensor contributes 0; one beyond the padded extent (ceil_mode) contributes nothing.
struct I3dPoolArgs {
    const float* in; float* out;
    int B, Ti, Hi, Wi, To, Ho, Wo, C;
    int kT, kH, kW, sT, sH, sW, pT, pH, pW;   // p*: padding in FRONT
    int eT, eH, eW;                           // padded extents (front + size + back)
};
__global__ __launch_bounds__(256) void i3d_maxpool_kernel(I3dPoolArgs a) {
    const int C4 = a.C >> 2;
    const long total = (long)a.B * a.To * a.Ho * a.Wo * C4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        long p = i / C4;
        const int wo = (int)(p % a.Wo); p /= a.Wo;
        const int ho = (int)(p % a.Ho); p /= a.Ho;
        const int to = (int)(p % a.To);
        const int b = (int)(p / a.To);
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        for (int dt = 0; dt < a.kT; ++dt) {
            const int ut = to * a.sT + dt;
            if (ut >= a.eT) continue;
            for (int dh = 0; dh < a.kH; ++dh) {
                const int uh = ho * a.sH + dh;
                if (uh >= a.eH) continue;
                for (int dw = 0; dw < a.kW; ++dw) {
                    const int uw = wo * a.sW + dw;
                    if (uw >= a.eW) continue;
                    const int t = ut - a.pT, h = uh - a.pH, w = uw - a.pW;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if ((unsigned)t < (unsigned)a.Ti && (unsigned)h < (unsigned)a.Hi && (unsigned)w < (unsigned)a.Wi)
                        v = *reinterpret_cast<const float4*>(a.in + ((((long)b * a.Ti + t) * a.Hi + h) * a.Wi + w) * a.C + 4 * c4);
                    m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
                }
            }
        }
        *reinterpret_cast<float4*>(a.out + i * 4) = m;
    }
}

// AvgPool3d((kT, 7, 7), stride 1) on [B][T][7][7][C] -> [B][T - kT + 1][C], or with `chw` [B][C][T - kT + 1] (get_representation's
// layout after its two squeeze(3)); fixed summation order
__global__ __launch_bounds__(256) void i3d_avgpool_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int T, int C, int kT,
                                                          int chw) {
    const int To = T - kT + 1, n = 49 * kT;
    const long total = (long)B * To * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int t = (int)((i / C) % To);
        const int b = (int)(i / ((long)C * To));
        const float* p = in + (((long)b * T + t) * 49) * C + c;
        float s = 0.f;
        for (int j = 0; j < n; ++j) s += p[(long)j * C];
        out[chw ? ((long)b * C + c) * To + t : i] = s / (float)n;
    }
}

// out.mean(2): logits[b][n] = mean over the remaining time steps of x[b][t][n]
__global__ __launch_bounds__(256) void i3d_time_mean_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int T, int N) {
    const long total = (long)B * N;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i % N);
        const int b = (int)(i / N);
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += x[((long)b * T + t) * N + n];
        out[i] = s / (float)T;
    }
}

// sum[j] += sum_b f[b][j], gram[i][j] += sum_b f[b][i] f[b][j] in float64: one owner per output element, the batch in order
__global__ __launch_bounds__(256) void fvd_stats_kernel(const float* __restrict__ f, int n, int D, double* __restrict__ sum,
                                                        double* __restrict__ gram) {
    const long total = (long)D * D + D;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        if (i < (long)D * D) {
            const int r = (int)(i / D), c = (int)(i % D);
            double s = gram[i];
            for (int b = 0; b < n; ++b) s += (double)f[(long)b * D + r] * (double)f[(long)b * D + c];
            gram[i] = s;
        } else {
            const int c = (int)(i - (long)D * D);
            double s = sum[c];
            for (int b = 0; b < n; ++b) s += (double)f[(long)b * D + c];
            sum[c] = s;
        }
    }
}

// The pair loop of metrics/Diversity/I3D.py:53-57 on embed [N][R][D]: acc[0] += sum_n sum_{i != j} mean_d (e_ni - e_nj)^2, acc[1] += the
// number N R (R - 1) of (instance, ordered pair) terms.  ONE workgroup owns the result: thread x sums its columns d = x, x + 256, ... over
// the instances and the pairs i < j in order (each counted twice: the square is symmetric), in float64 as the reference's float64 array
// does; then a fixed tree over the 256 partial sums.  Two runs give the same bits.
__global__ __launch_bounds__(256) void diversity_kernel(const float* __restrict__ e, int N, int R, int D, double* __restrict__ acc) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int n = 0; n < N; ++n) {
        const float* en = e + (long)n * R * D;
        for (int i = 0; i < R; ++i)
            for (int j = i + 1; j < R; ++j)
                for (int d = tid; d < D; d += 256) {
                    const double v = (double)en[(long)i * D + d] - (double)en[(long)j * D + d];
                    s += v * v;
                }
    }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        acc[0] += 2.0 * red[0] / (double)D;
        acc[1] += (double)N * R * (R - 1);
    }
}

// "TF SAME" padding of one dimension (get_padding_shape): `mod` = input size % stride for the TIME dimension of a strided unit
// (Kinetics), for every dimension of a strided unit (dynamic-texture variant: Unit3D.compute_pad, MaxPool3dSamePadding.compute_pad)
void same_pad(int k, int s, int mod, int* front, int* back) {
    const int along = std::max(mod ? k - mod : k - s, 0);
    *front = along / 2;
    *back = along - along / 2;
}
// MaxPool3d(ceil_mode=True, padding 0) on an extent e
int pool_out(int e, int k, int s) {
    int o = (e - k + s - 1) / s + 1;
    if ((o - 1) * s >= e) --o;
    return o;
}

// One conv unit (Unit3Dpy / ID3.Unit3D) of the state_dict: [cout][cin][k][k][k] under <name>.conv3d.weight, and its epilogue: the eval-mode
// BatchNorm3d under <name>.<bnkey> (eps 1e-3 under "batch3d", 1e-5 under "bn"), else the conv bias, else nothing
struct Unit : FlatConv {
    int pack(const StateDict& sd, const std::string& name, int cin, int cout, int k, bool bn, bool bias, const char* bnkey = "batch3d",
             double eps = 1e-3) {
        const float* wsrc = sd.f32(name + ".conv3d.weight", (int64_t)cout * cin * k * k * k);
        if (!wsrc) return I2V_E_MISSING;
        FlatConvPacked p = flatconv_pack(wsrc, cin, cout, k, k, k);
        if (bn) {
            const std::string bk = name + "." + bnkey;
            const float* g = sd.f32(bk + ".weight", cout);
            const float* b = sd.f32(bk + ".bias", cout);
            const float* m = sd.f32(bk + ".running_mean", cout);
            const float* v = sd.f32(bk + ".running_var", cout);
            if (!g || !b || !m || !v) return I2V_E_MISSING;
            flatconv_fold_bn(p, g, b, m, v, eps);
        } else if (bias) {
            const float* b = sd.f32(name + ".conv3d.bias", cout);
            if (!b) return I2V_E_MISSING;
            flatconv_bias(p, b);
        }
        return upload(p);
    }
};

struct MixedSpec { const char* name; int cin; int o[6]; };
const MixedSpec MIXED[9] = {
    {"mixed_3b", 192, {64, 96, 128, 16, 32, 32}},   {"mixed_3c", 256, {128, 128, 192, 32, 96, 64}},
    {"mixed_4b", 480, {192, 96, 208, 16, 48, 64}},  {"mixed_4c", 512, {160, 112, 224, 24, 64, 64}},
    {"mixed_4d", 512, {128, 128, 256, 24, 64, 64}}, {"mixed_4e", 512, {112, 144, 288, 32, 64, 64}},
    {"mixed_4f", 528, {256, 160, 320, 32, 128, 128}}, {"mixed_5b", 832, {256, 160, 320, 32, 128, 128}},
    {"mixed_5c", 832, {384, 192, 384, 48, 128, 128}}};

struct Dims { int T, H, W; long pos() const { return (long)T * H * W; } };

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_i3d {
    int num_classes = 0, in_channels = 3, device = 0;
    int dt = 0;       // 0: Kinetics-400 network (metrics/PyTorch_FVD/I3D.py); 16 / 32: dynamic-texture network of that length (metrics/DTFVD)
    int pool_t = 2;   // time extent of the average pool: (2, 7, 7), ID3_32: (4, 7, 7)
    bool loaded = false;
    Unit stem, c2b, c2c, head;
    Unit mixed[9][6];   // branch_0, branch_1.0, branch_1.1, branch_2.0, branch_2.1, branch_3.1
    StreamOrder order;
};

namespace {

// SAME padding in front and output dims of a conv unit with kernel (k, k, k) and stride (s, s, s) on a [T][H][W] map: the size % stride
// rule on time only (Kinetics), on every dimension (dynamic-texture variant)
void unit_geom(const i2v_i3d* net, int k, int s, Dims d, int* pT, int* pH, int* pW, Dims* o) {
    int bT, bH, bW;
    same_pad(k, s, s > 1 ? d.T % s : 0, pT, &bT);
    same_pad(k, s, net->dt && s > 1 ? d.H % s : 0, pH, &bH);
    same_pad(k, s, net->dt && s > 1 ? d.W % s : 0, pW, &bW);
    *o = Dims{(d.T + *pT + bT - k) / s + 1, (d.H + *pH + bH - k) / s + 1, (d.W + *pW + bW - k) / s + 1};
}

// One walk of the network serves the workspace size (dry: no buffers, no launches) and the forward.
struct Walk {
    const i2v_i3d* net;
    int B;
    bool dry;
    hipStream_t st;
    size_t act_floats = 0, tmp_floats = 0;   // dry: the largest block-level tensor / branch temporary

    int conv(const Unit& u, const float* in, int inCS, int inOff, Dims di, float* out, int outCS, int outOff, Dims dout, int sT, int s,
             int pT, int pS, bool relu, int pW = -1) {
        if (dry) return I2V_OK;
        const FlatConvMaps g{B, di.T, di.H, di.W, dout.T, dout.H, dout.W, sT, s, s, pT, pS, pW < 0 ? pS : pW};
        return flat_conv_launch<true>("i3d conv", u, in, inCS, inOff, out, outCS, outOff, g, relu, st);
    }

    // One conv unit at stride (s, s, s) with its own SAME padding (unit_geom); returns the output dims
    int unit(const Unit& u, int s, const float* in, int inCS, int inOff, Dims di, float* out, int outCS, int outOff, bool relu, Dims* dout) {
        int pT, pH, pW;
        unit_geom(net, u.kt, s, di, &pT, &pH, &pW, dout);
        return conv(u, in, inCS, inOff, di, out, outCS, outOff, *dout, s, s, pT, pH, relu, pW);
    }

    // MaxPool3dTFPadding(kernel (kT, k, k), stride (sT, s, s)); returns the output dims
    int pool(const float* in, float* out, int C, Dims di, int kT, int k, int sT, int s, Dims* dout) {
        I3dPoolArgs a{};
        int bT, bH, bW;
        same_pad(kT, sT, sT > 1 ? di.T % sT : 0, &a.pT, &bT);
        same_pad(k, s, net->dt && s > 1 ? di.H % s : 0, &a.pH, &bH);
        same_pad(k, s, net->dt && s > 1 ? di.W % s : 0, &a.pW, &bW);
        a.eT = a.pT + di.T + bT; a.eH = a.pH + di.H + bH; a.eW = a.pW + di.W + bW;
        dout->T = pool_out(a.eT, kT, sT); dout->H = pool_out(a.eH, k, s); dout->W = pool_out(a.eW, k, s);
        if (dry) return I2V_OK;
        a.in = in; a.out = out; a.B = B; a.Ti = di.T; a.Hi = di.H; a.Wi = di.W; a.To = dout->T; a.Ho = dout->H; a.Wo = dout->W; a.C = C;
        a.kT = kT; a.kH = k; a.kW = k; a.sT = sT; a.sH = s; a.sW = s;
        hipLaunchKernelGGL(i3d_maxpool_kernel, dim3(grid_for((long)B * dout->pos() * (C / 4))), dim3(256), 0, st, a);
        I2V_HIP_CHECK(hipGetLastError());
        return I2V_OK;
    }

    void need(size_t* slot, long floats) { *slot = std::max(*slot, (size_t)floats); }

    static int mixed_out(int i) { return MIXED[i].o[0] + MIXED[i].o[2] + MIXED[i].o[4] + MIXED[i].o[5]; }

    // Mixed block i: x [B][d][cin] -> y [B][d][Co]; tmp holds one branch temporary at a time
    int mixed(int i, const float* x, Dims d, float* y, float* tmp) {
        int rc;
        const MixedSpec& s = MIXED[i];
        const Unit* u = net->mixed[i];
        const int C = s.cin, Co = mixed_out(i);
        need(&act_floats, (long)B * d.pos() * Co);
        need(&tmp_floats, (long)B * d.pos() * std::max(std::max(s.o[1], s.o[3]), C));
        // the branches store into their channel slice of y (torch.cat((out_0, out_1, out_2, out_3), 1))
        if ((rc = conv(u[0], x, C, 0, d, y, Co, 0, d, 1, 1, 0, 0, true))) return rc;
        if ((rc = conv(u[1], x, C, 0, d, tmp, s.o[1], 0, d, 1, 1, 0, 0, true))) return rc;
        if ((rc = conv(u[2], tmp, s.o[1], 0, d, y, Co, s.o[0], d, 1, 1, 1, 1, true))) return rc;
        if ((rc = conv(u[3], x, C, 0, d, tmp, s.o[3], 0, d, 1, 1, 0, 0, true))) return rc;
        if ((rc = conv(u[4], tmp, s.o[3], 0, d, y, Co, s.o[0] + s.o[2], d, 1, 1, 1, 1, true))) return rc;
        Dims po;
        if ((rc = pool(x, tmp, C, d, 3, 3, 1, 1, &po))) return rc;
        return conv(u[5], tmp, C, 0, d, y, Co, s.o[0] + s.o[2] + s.o[4], d, 1, 1, 0, 0, true);
    }

    // AvgPool3d((pool_t, 7, 7)) on x [B][T][7][7][1024] -> pooled [B][T'][1024], conv3d_0c_1x1 -> cls [B][T'][classes], time mean -> logits;
    // with `features` only the pool, stored as [B][1024][T'] into logits
    int head(const float* x, int T, float* pooled, float* cls, float* logits, bool features) {
        const int kT = net->pool_t;
        hipLaunchKernelGGL(i3d_avgpool_kernel, dim3(grid_for((long)B * (T - kT + 1) * 1024)), dim3(256), 0, st, x, features ? logits : pooled, B,
                           T, 1024, kT, features ? 1 : 0);
        I2V_HIP_CHECK(hipGetLastError());
        if (features) return I2V_OK;
        const Dims dh{T - kT + 1, 1, 1};
        if (int rc = conv(net->head, pooled, 1024, 0, dh, cls, net->num_classes, 0, dh, 1, 1, 0, 0, false)) return rc;   // conv3d_0c_1x1
        hipLaunchKernelGGL(i3d_time_mean_kernel, dim3(grid_for((long)B * net->num_classes)), dim3(256), 0, st, cls, logits, B, dh.T,
                           net->num_classes);
        I2V_HIP_CHECK(hipGetLastError());
        return I2V_OK;
    }

    // frames -> logits, or with `features` -> the average pool's output [B][1024][T'] in `logits` (no classifier, no time mean).
    // T frames enter the network, frame t read from source frame t % Tin.  inp / x / y / tmp / pooled / cls: workspace buffers (null when dry)
    int run(const float* frames, int Tin, int T, int H, int W, int denorm, float* inp, float* x, float* y, float* tmp, float* pooled, float* cls,
            float* logits, int* t_head, bool features = false) {
        int rc;
        Dims d{T, I3D_SIDE, I3D_SIDE};
        if (!dry) {
            hipLaunchKernelGGL(i3d_input_kernel, dim3(grid_for((long)B * T * I3D_SIDE * I3D_SIDE)), dim3(256), 0, st, frames, inp, (long)B * T, Tin, T,
                               H, W, denorm);
            I2V_HIP_CHECK(hipGetLastError());
        }
        // conv3d_1a_7x7: stride 2, SAME = (2, 3) per dimension, (3, 3) in time for an odd T (and, by the dynamic-texture variant's rule, in
        // an odd spatial dimension: none at 224)
        Dims o;
        if ((rc = unit(net->stem, 2, inp, 4, 0, d, x, 64, 0, true, &o))) return rc;
        need(&act_floats, (long)B * o.pos() * 64);
        d = o;
        if ((rc = pool(x, y, 64, d, 1, 3, 1, 2, &o))) return rc;                              // maxPool3d_2a_3x3
        d = o;
        if ((rc = conv(net->c2b, y, 64, 0, d, x, 64, 0, d, 1, 1, 0, 0, true))) return rc;      // conv3d_2b_1x1
        need(&act_floats, (long)B * d.pos() * 192);
        if ((rc = conv(net->c2c, x, 64, 0, d, y, 192, 0, d, 1, 1, 1, 1, true))) return rc;     // conv3d_2c_3x3
        if ((rc = pool(y, x, 192, d, 1, 3, 1, 2, &o))) return rc;                             // maxPool3d_3a_3x3
        d = o;
        int C = 192;
        for (int i = 0; i < 9; ++i) {
            if ((rc = mixed(i, x, d, y, tmp))) return rc;
            std::swap(x, y);
            C = mixed_out(i);
            if (i == 1) { if ((rc = pool(x, y, C, d, 3, 3, 2, 2, &o))) return rc; d = o; std::swap(x, y); }   // maxPool3d_4a_3x3
            if (i == 6) { if ((rc = pool(x, y, C, d, 2, 2, 2, 2, &o))) return rc; d = o; std::swap(x, y); }   // maxPool3d_5a_2x2
        }
        const int kT = net->pool_t;
        I2V_REQUIRE(d.H == 7 && d.W == 7 && d.T >= kT, I2V_E_INVALID,
                    "i3d: %d frames leave a [%d, %d, %d] map in front of AvgPool3d((%d, 7, 7)); at least %d frames are needed", T, d.T, d.H, d.W, kT,
                    8 * (kT - 1) + 1);
        *t_head = d.T - kT + 1;
        if (dry) return I2V_OK;
        return head(x, d.T, pooled, cls, logits, features);
    }
};

struct I3dWs { size_t inp, x, y, tmp, pooled, cls, total; };

int i3d_ws(const i2v_i3d* net, int B, int T, int H, int W, I3dWs* L, bool features = false, int* t_head = nullptr) {
    Walk wk{net, B, true, nullptr};
    int th = 0;
    if (int rc = wk.run(nullptr, T, T, H, W, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &th, features)) return rc;
    if (t_head) *t_head = th;
    Carver c;
    L->inp = c.take_floats((size_t)B * T * I3D_SIDE * I3D_SIDE * 4);
    L->x = c.take_floats(wk.act_floats);
    L->y = c.take_floats(wk.act_floats);
    L->tmp = c.take_floats(wk.tmp_floats);
    L->pooled = c.take_floats(features ? 0 : (size_t)B * th * 1024);
    L->cls = c.take_floats(features ? 0 : (size_t)B * th * net->num_classes);
    L->total = c.total();
    return I2V_OK;
}

}  // namespace

extern "C" {

int i2v_i3d_create(int32_t num_classes, int32_t in_channels, i2v_i3d** out) {
    I2V_REQUIRE(out && num_classes > 0, I2V_E_INVALID, "i2v_i3d_create: bad argument");
    I2V_REQUIRE(in_channels == 3, I2V_E_INVALID, "i2v_i3d_create: only the rgb network (3 input channels) is built, got %d", in_channels);
    return create_handle("i2v_i3d_create", out, [&](i2v_i3d* n) {
        n->num_classes = num_classes;
        n->in_channels = in_channels;
        return I2V_OK;
    });
}

int i2v_dti3d_create(int32_t num_classes, int32_t length, i2v_i3d** out) {
    I2V_REQUIRE(length == 16 || length == 32, I2V_E_INVALID, "i2v_dti3d_create: the dynamic-texture I3D exists for length 16 and 32, got %d", length);
    if (int rc = i2v_i3d_create(num_classes, 3, out)) return rc;
    (*out)->dt = length;
    (*out)->pool_t = length == 32 ? 4 : 2;
    return I2V_OK;
}

void i2v_i3d_destroy(i2v_i3d* n) { delete n; }

static int i3d_pack(i2v_i3d* n, const StateDict& sd) {
    int rc;
    if (n->dt) {   // ID3.InceptionI3D: Conv3d_* / Mixed_*.{b0,b1a,b1b,b2a,b2b,b3b} / logits, BatchNorm3d under "bn" with eps 1e-5
        static const char* const BR[6] = {".b0", ".b1a", ".b1b", ".b2a", ".b2b", ".b3b"};
        if ((rc = n->stem.pack(sd, "Conv3d_1a_7x7", n->in_channels, 64, 7, true, false, "bn", 1e-5))) return rc;
        if ((rc = n->c2b.pack(sd, "Conv3d_2b_1x1", 64, 64, 1, true, false, "bn", 1e-5))) return rc;
        if ((rc = n->c2c.pack(sd, "Conv3d_2c_3x3", 64, 192, 3, true, false, "bn", 1e-5))) return rc;
        for (int i = 0; i < 9; ++i) {
            const MixedSpec& s = MIXED[i];
            std::string p = s.name;
            p[0] = 'M';
            const int cin[6] = {s.cin, s.cin, s.o[1], s.cin, s.o[3], s.cin};
            for (int j = 0; j < 6; ++j)
                if ((rc = n->mixed[i][j].pack(sd, p + BR[j], cin[j], s.o[j], j == 2 || j == 4 ? 3 : 1, true, false, "bn", 1e-5))) return rc;
        }
        return n->head.pack(sd, "logits", 1024, n->num_classes, 1, false, true);   // (i2v_i3d_features never launches it)
    }
    if ((rc = n->stem.pack(sd, "conv3d_1a_7x7", n->in_channels, 64, 7, true, false))) return rc;
    if ((rc = n->c2b.pack(sd, "conv3d_2b_1x1", 64, 64, 1, true, false))) return rc;
    if ((rc = n->c2c.pack(sd, "conv3d_2c_3x3", 64, 192, 3, true, false))) return rc;
    for (int i = 0; i < 9; ++i) {
        const MixedSpec& s = MIXED[i];
        const std::string p = std::string(s.name) + ".";
        Unit* u = n->mixed[i];
        if ((rc = u[0].pack(sd, p + "branch_0", s.cin, s.o[0], 1, true, false))) return rc;
        if ((rc = u[1].pack(sd, p + "branch_1.0", s.cin, s.o[1], 1, true, false))) return rc;
        if ((rc = u[2].pack(sd, p + "branch_1.1", s.o[1], s.o[2], 3, true, false))) return rc;
        if ((rc = u[3].pack(sd, p + "branch_2.0", s.cin, s.o[3], 1, true, false))) return rc;
        if ((rc = u[4].pack(sd, p + "branch_2.1", s.o[3], s.o[4], 3, true, false))) return rc;
        if ((rc = u[5].pack(sd, p + "branch_3.1", s.cin, s.o[5], 1, true, false))) return rc;
    }
    return n->head.pack(sd, "conv3d_0c_1x1", 1024, n->num_classes, 1, false, true);
}

int i2v_i3d_load(i2v_i3d* n, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_i3d_load", n, tensors, n_tensors, i3d_pack);
}

size_t i2v_i3d_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t, int32_t h, int32_t w) {
    if (!n || batch <= 0 || t <= 0 || h < 2 || w < 2) return 0;
    I3dWs L;
    if (i3d_ws(n, batch, t, h, w, &L)) return 0;
    return L.total;
}

int i2v_i3d_forward(i2v_i3d* n, const float* frames, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t denorm, float* logits,
                    void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_i3d_forward");
    I2V_REQUIRE(frames && logits && workspace && batch > 0 && t > 0 && h >= 2 && w >= 2, I2V_E_INVALID, "i2v_i3d_forward: bad argument");
    I2V_REQUIRE((long)batch * t * I3D_SIDE * I3D_SIDE * 64 < (1L << 40), I2V_E_INVALID, "i2v_i3d_forward: batch %d x %d frames is too large", batch, t);
    I3dWs L;
    if (int rc = i3d_ws(n, batch, t, h, w, &L)) return rc;
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_i3d_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    void* const ws = workspace;
    Walk wk{n, batch, false, st};
    int th = 0;
    return wk.run(frames, t, t, h, w, denorm ? 1 : 0, Carver::at(ws, L.inp), Carver::at(ws, L.x), Carver::at(ws, L.y), Carver::at(ws, L.tmp),
                  Carver::at(ws, L.pooled), Carver::at(ws, L.cls), logits, &th);
}

size_t i2v_i3d_features_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t_out, int32_t h, int32_t w) {
    if (!n || batch <= 0 || t_out <= 0 || h < 2 || w < 2) return 0;
    I3dWs L;
    if (i3d_ws(n, batch, t_out, h, w, &L, true)) return 0;
    return L.total;
}

int32_t i2v_i3d_feature_steps(const i2v_i3d* n, int32_t t_out) {
    if (!n || t_out <= 0) return 0;
    I3dWs L;
    int th = 0;
    if (i3d_ws(n, 1, t_out, I3D_SIDE, I3D_SIDE, &L, true, &th)) return 0;
    return th;
}

int i2v_i3d_features(i2v_i3d* n, const float* frames, int32_t batch, int32_t t_in, int32_t t_out, int32_t h, int32_t w, int32_t denorm,
                     float* feats, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_i3d_features");
    I2V_REQUIRE(frames && feats && workspace && batch > 0 && t_in > 0 && t_out > 0 && h >= 2 && w >= 2, I2V_E_INVALID,
                "i2v_i3d_features: bad argument");
    I2V_REQUIRE((long)batch * t_out * I3D_SIDE * I3D_SIDE * 64 < (1L << 40) && (long)batch * t_in * 3 * h * w < (1L << 40), I2V_E_INVALID,
                "i2v_i3d_features: batch %d x %d frames is too large", batch, t_out);
    I3dWs L;
    if (int rc = i3d_ws(n, batch, t_out, h, w, &L, true)) return rc;
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_i3d_features");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    void* const ws = workspace;
    Walk wk{n, batch, false, st};
    int th = 0;
    return wk.run(frames, t_in, t_out, h, w, denorm ? 1 : 0, Carver::at(ws, L.inp), Carver::at(ws, L.x), Carver::at(ws, L.y), Carver::at(ws, L.tmp),
                  nullptr, nullptr, feats, &th, true);
}

// ---- sub-modules of a loaded handle, individually callable on channels-last tensors (for tests and inspection)

namespace {
// unit index -> the unit and its stride; null for an unknown index
const Unit* i3d_unit(const i2v_i3d* n, int unit, int* stride) {
    *stride = unit == I2V_I3D_UNIT_STEM ? 2 : 1;
    if (unit == I2V_I3D_UNIT_STEM) return &n->stem;
    if (unit == I2V_I3D_UNIT_2B) return &n->c2b;
    if (unit == I2V_I3D_UNIT_2C) return &n->c2c;
    if (unit == I2V_I3D_UNIT_HEAD) return &n->head;
    if (unit >= I2V_I3D_UNIT_MIXED && unit < I2V_I3D_UNIT_MIXED + 54) return &n->mixed[(unit - I2V_I3D_UNIT_MIXED) / 6][(unit - I2V_I3D_UNIT_MIXED) % 6];
    return nullptr;
}
constexpr long I3D_SUB_MAX = 1L << 31;   // floats per tensor of a sub-module call
}  // namespace

int i2v_i3d_unit_shape(const i2v_i3d* n, int32_t unit, int32_t t, int32_t h, int32_t w, int32_t* cin, int32_t* cout, int32_t* out_dims) {
    I2V_REQUIRE(n, I2V_E_INVALID, "i2v_i3d_unit_shape: null handle");
    I2V_REQUIRE(n->loaded, I2V_E_STATE, "i2v_i3d_unit_shape: weights not loaded");
    int s;
    const Unit* u = i3d_unit(n, unit, &s);
    I2V_REQUIRE(u && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_unit_shape: unit %d on a [%d, %d, %d] map", unit, t, h, w);
    int pT, pH, pW;
    Dims o;
    unit_geom(n, u->kt, s, Dims{t, h, w}, &pT, &pH, &pW, &o);
    if (cin) *cin = 4 * u->C4;
    if (cout) *cout = u->Cout;
    if (out_dims) { out_dims[0] = o.T; out_dims[1] = o.H; out_dims[2] = o.W; }
    return I2V_OK;
}

int i2v_i3d_unit_forward(i2v_i3d* n, int32_t unit, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t in_cs, float* out,
                         int32_t out_cs, int32_t out_off, size_t out_floats, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_i3d_unit_forward");
    int s;
    const Unit* u = i3d_unit(n, unit, &s);
    I2V_REQUIRE(u, I2V_E_INVALID, "i2v_i3d_unit_forward: unknown unit %d", unit);
    I2V_REQUIRE(x && out && batch > 0 && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_unit_forward: bad argument");
    I2V_REQUIRE(in_cs > 0 && in_cs % 4 == 0 && in_cs >= 4 * u->C4 && out_cs > 0 && out_off >= 0 && out_off + u->Cout <= out_cs, I2V_E_INVALID,
                "i2v_i3d_unit_forward: channels [0, %d) of %d -> [%d, +%d) of %d do not fit", 4 * u->C4, in_cs, out_off, u->Cout, out_cs);
    int pT, pH, pW;
    Dims o;
    unit_geom(n, u->kt, s, Dims{t, h, w}, &pT, &pH, &pW, &o);
    I2V_REQUIRE((long)batch * t * h * w * in_cs < I3D_SUB_MAX && (long)batch * o.pos() * out_cs < I3D_SUB_MAX, I2V_E_INVALID,
                "i2v_i3d_unit_forward: batch %d x [%d, %d, %d] is too large", batch, t, h, w);
    I2V_REQUIRE(out_floats >= (size_t)batch * o.pos() * out_cs, I2V_E_WORKSPACE, "i2v_i3d_unit_forward: output of %zu floats < required %zu",
                out_floats, (size_t)batch * o.pos() * out_cs);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    Walk wk{n, batch, false, st};
    return wk.unit(*u, s, x, in_cs, 0, Dims{t, h, w}, out, out_cs, out_off, unit != I2V_I3D_UNIT_HEAD, &o);
}

size_t i2v_i3d_mixed_workspace_bytes(const i2v_i3d* n, int32_t block, int32_t batch, int32_t t, int32_t h, int32_t w) {
    if (!n || block < 0 || block >= 9 || batch <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    Walk wk{n, batch, true, nullptr};
    if (wk.mixed(block, nullptr, Dims{t, h, w}, nullptr, nullptr)) return 0;
    return align_up(wk.tmp_floats * 4, 256);
}

int i2v_i3d_mixed_forward(i2v_i3d* n, int32_t block, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, float* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_i3d_mixed_forward");
    I2V_REQUIRE(block >= 0 && block < 9, I2V_E_INVALID, "i2v_i3d_mixed_forward: unknown block %d", block);
    I2V_REQUIRE(x && out && workspace && batch > 0 && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_mixed_forward: bad argument");
    I2V_REQUIRE((long)batch * t * h * w * 1024 < I3D_SUB_MAX, I2V_E_INVALID, "i2v_i3d_mixed_forward: batch %d x [%d, %d, %d] is too large", batch, t, h,
                w);
    const size_t need = i2v_i3d_mixed_workspace_bytes(n, block, batch, t, h, w);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, "i2v_i3d_mixed_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    Walk wk{n, batch, false, st};
    return wk.mixed(block, x, Dims{t, h, w}, out, static_cast<float*>(workspace));
}

int i2v_i3d_maxpool_shape(const i2v_i3d* n, int32_t kt, int32_t k, int32_t st, int32_t s, int32_t t, int32_t h, int32_t w, int32_t* out_dims) {
    I2V_REQUIRE(n && out_dims && kt > 0 && k > 0 && st > 0 && s > 0 && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_maxpool_shape: bad argument");
    Walk wk{n, 1, true, nullptr};
    Dims o;
    if (int rc = wk.pool(nullptr, nullptr, 4, Dims{t, h, w}, kt, k, st, s, &o)) return rc;
    out_dims[0] = o.T; out_dims[1] = o.H; out_dims[2] = o.W;
    return I2V_OK;
}

int i2v_i3d_maxpool_forward(i2v_i3d* n, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t c, int32_t kt, int32_t k, int32_t st,
                            int32_t s, float* out, size_t out_floats, void* stream) {
    I2V_ENTER(sc, n, 0, "i2v_i3d_maxpool_forward");
    I2V_REQUIRE(x && out && batch > 0 && t > 0 && h > 0 && w > 0 && kt > 0 && k > 0 && st > 0 && s > 0, I2V_E_INVALID,
                "i2v_i3d_maxpool_forward: bad argument");
    I2V_REQUIRE(c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_i3d_maxpool_forward: %d channels (a multiple of 4 is needed)", c);
    int od[3];
    if (int rc = i2v_i3d_maxpool_shape(n, kt, k, st, s, t, h, w, od)) return rc;
    I2V_REQUIRE(od[0] > 0 && od[1] > 0 && od[2] > 0 && (long)batch * t * h * w * c < I3D_SUB_MAX && (long)batch * od[0] * od[1] * od[2] * c < I3D_SUB_MAX,
                I2V_E_INVALID, "i2v_i3d_maxpool_forward: batch %d x [%d, %d, %d] x %d", batch, t, h, w, c);
    const size_t need = (size_t)batch * od[0] * od[1] * od[2] * c;
    I2V_REQUIRE(out_floats >= need, I2V_E_WORKSPACE, "i2v_i3d_maxpool_forward: output of %zu floats < required %zu", out_floats, need);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, hs)) return rco;
    Walk wk{n, batch, false, hs};
    Dims o;
    return wk.pool(x, out, c, Dims{t, h, w}, kt, k, st, s, &o);
}

size_t i2v_i3d_head_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t) {
    if (!n || batch <= 0 || t < n->pool_t) return 0;
    return align_up((size_t)batch * (t - n->pool_t + 1) * n->num_classes * 4, 256);
}

int i2v_i3d_head_forward(i2v_i3d* n, const float* x, int32_t batch, int32_t t, float* pooled, float* feats, float* logits, void* workspace,
                         size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_i3d_head_forward");
    I2V_REQUIRE(x && pooled && feats && logits && workspace && batch > 0, I2V_E_INVALID, "i2v_i3d_head_forward: bad argument");
    I2V_REQUIRE(t >= n->pool_t && (long)batch * t * 49 * 1024 < I3D_SUB_MAX, I2V_E_INVALID,
                "i2v_i3d_head_forward: %d time steps in front of AvgPool3d((%d, 7, 7)), batch %d", t, n->pool_t, batch);
    const size_t need = i2v_i3d_head_workspace_bytes(n, batch, t);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, need, "i2v_i3d_head_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    Walk wk{n, batch, false, st};
    if (int rc = wk.head(x, t, nullptr, nullptr, feats, true)) return rc;
    return wk.head(x, t, pooled, static_cast<float*>(workspace), logits, false);
}

int i2v_i3d_input_stage(const float* frames, int32_t n_frames, int32_t h, int32_t w, int32_t denorm, float* out, void* stream) {
    I2V_REQUIRE(frames && out && n_frames > 0 && h >= 2 && w >= 2, I2V_E_INVALID, "i2v_i3d_input_stage: bad argument");
    hipLaunchKernelGGL(i3d_input_kernel, dim3(grid_for((long)n_frames * I3D_SIDE * I3D_SIDE)), dim3(256), 0, static_cast<hipStream_t>(stream), frames,
                       out, (long)n_frames, 1, 1, h, w, denorm ? 1 : 0);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_fvd_stats_update(const float* feats, int32_t n, int32_t d, double* sum, double* gram, void* stream) {
    I2V_REQUIRE(feats && sum && gram && n > 0 && d > 0, I2V_E_INVALID, "i2v_fvd_stats_update: bad argument");
    hipLaunchKernelGGL(fvd_stats_kernel, dim3(grid_for((long)d * d + d)), dim3(256), 0, static_cast<hipStream_t>(stream), feats, n, d, sum, gram);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_diversity_update(const float* embed, int32_t n, int32_t r, int32_t d, double* acc, void* stream) {
    I2V_REQUIRE(embed && acc && n > 0 && r > 0 && d > 0, I2V_E_INVALID, "i2v_diversity_update: bad argument");
    hipLaunchKernelGGL(diversity_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), embed, n, r, d, acc);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // extern "C"
