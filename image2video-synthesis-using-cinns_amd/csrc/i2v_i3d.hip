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
#include "i2v_trunk_plan.h"

namespace i2v {
namespace {

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

// One conv unit (Unit3Dpy / ID3.Unit3D) of the state_dict: [cout][cin][k][k][k] under <name>.conv3d.weight, and its epilogue: the eval-mode
// BatchNorm3d under <name>.<bnkey> (eps 1e-3 under "batch3d", 1e-5 under "bn"), or without a bnkey the conv bias
struct Unit : FlatConv {
    int pack(const StateDict& sd, const std::string& name, int cin, int cout, int k, const char* bnkey, double eps) {
        return load(sd, name + ".conv3d.weight", cin, cout, k, k, k, bnkey ? name + "." + bnkey : "", eps, name + ".conv3d.bias");
    }
};

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_i3d {
    I3dVariant v{0, 2, 0};   // Kinetics-400 network (metrics/PyTorch_FVD/I3D.py) with AvgPool3d((2, 7, 7)); i2v_dti3d_create: metrics/DTFVD
    int in_channels = 3, device = 0;
    bool loaded = false;
    Unit units[I2V_I3D_UNIT_HEAD + 1];   // by I2V_I3D_UNIT_*
    StreamOrder order;
};

namespace {

// The launches of a plan (i2v_trunk_plan.h), in order
int launch(const i2v_i3d* n, const TrunkPlan& p, const TrunkBufs& buf, int denorm, hipStream_t st) {
    const int B = p.B;
    for (const Step& s : p.steps) {
        const float* in = buf.p[s.src];
        float* out = buf.p[s.dst];
        switch (s.kind) {
        case STEP_INPUT:
            hipLaunchKernelGGL(i3d_input_kernel, dim3(grid_for((long)B * s.out.T * I3D_SIDE * I3D_SIDE)), dim3(256), 0, st, in, out, (long)B * s.out.T,
                               s.in.T, s.out.T, s.in.H, s.in.W, denorm);
            break;
        case STEP_CONV: {
            const FlatConvMaps g{B, s.in.T, s.in.H, s.in.W, s.out.T, s.out.H, s.out.W, s.s[0], s.s[1], s.s[2], s.p[0], s.p[1], s.p[2]};
            if (int rc = flat_conv_launch<true>("i3d conv", n->units[s.unit], in, s.inCS, s.inOff, out, s.outCS, s.outOff, g, s.relu, st)) return rc;
            continue;
        }
        case STEP_I3D_POOL: {
            const I3dPoolArgs a{in, out, B, s.in.T, s.in.H, s.in.W, s.out.T, s.out.H, s.out.W, s.C, s.k[0], s.k[1], s.k[2], s.s[0], s.s[1], s.s[2],
                                s.p[0], s.p[1], s.p[2], s.e[0], s.e[1], s.e[2]};
            hipLaunchKernelGGL(i3d_maxpool_kernel, dim3(grid_for((long)B * s.out.pos() * (s.C / 4))), dim3(256), 0, st, a);
            break;
        }
        case STEP_AVGPOOL:
            hipLaunchKernelGGL(i3d_avgpool_kernel, dim3(grid_for((long)B * s.out.T * s.C)), dim3(256), 0, st, in, out, B, s.in.T, s.C, s.k[0],
                               s.chw ? 1 : 0);
            break;
        case STEP_TIME_MEAN:
            hipLaunchKernelGGL(i3d_time_mean_kernel, dim3(grid_for((long)B * s.C)), dim3(256), 0, st, in, out, B, s.in.T, s.C);
            break;
        default:
            I2V_REQUIRE(false, I2V_E_INVALID, "i3d: step kind %d", s.kind);
        }
        I2V_HIP_CHECK(hipGetLastError());
    }
    return I2V_OK;
}

// plans of the sub-module entries: the caller's tensor in BUF_IN, its output in BUF_OUT
TrunkPlan unit_plan(const i2v_i3d* n, int unit, int B, Map3 d, int in_cs, int out_cs, int out_off) {
    TrunkPlan p(B);
    i3d_unit(p, n->v, unit, BUF_IN, in_cs, d, BUF_OUT, out_cs, out_off, unit != I2V_I3D_UNIT_HEAD);
    return p;
}
TrunkPlan mixed_plan(const i2v_i3d* n, int block, int B, Map3 d) {
    TrunkPlan p(B);
    i3d_mixed(p, n->v, block, BUF_IN, d, BUF_OUT);
    p.carve<Carver>();
    return p;
}
TrunkPlan pool_plan(const i2v_i3d* n, int B, int C, Map3 d, int kt, int k, int st, int s) {
    TrunkPlan p(B);
    i3d_pool(p, n->v, BUF_IN, BUF_OUT, C, d, kt, k, st, s);
    return p;
}
TrunkPlan head_plan(const i2v_i3d* n, int B, int T, bool features) {
    TrunkPlan p(B);
    i3d_head(p, n->v, BUF_IN, T, features);
    return p;
}

size_t trunk_bytes(const i2v_i3d* n, int batch, int t, int h, int w, bool features) {
    if (!n || batch <= 0 || t <= 0 || h < 2 || w < 2) return 0;
    const TrunkPlan p = i3d_plan<Carver>(n->v, batch, t, t, h, w, features);
    return p.status ? (plan_refusal(p), 0) : p.total;   // a refused shape answers 0 and leaves its message
}

// i2v_i3d_forward (t_in = t_out, logits) and i2v_i3d_features
int trunk_forward(const char* what, bool features, i2v_i3d* n, const float* frames, int batch, int t_in, int t_out, int h, int w, int denorm,
                  float* out, void* workspace, size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, what);
    I2V_REQUIRE(frames && out && workspace && batch > 0 && t_in > 0 && t_out > 0 && h >= 2 && w >= 2, I2V_E_INVALID, "%s: bad argument", what);
    I2V_REQUIRE((long)batch * t_out * I3D_SIDE * I3D_SIDE * 64 < (1L << 40) && (!features || (long)batch * t_in * 3 * h * w < (1L << 40)),
                I2V_E_INVALID, "%s: batch %d x %d frames is too large", what, batch, t_out);
    const TrunkPlan p = i3d_plan<Carver>(n->v, batch, t_in, t_out, h, w, features);
    if (p.status) return plan_refusal(p);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    return launch(n, p, TrunkBufs(frames, out).carve(p, workspace), denorm ? 1 : 0, st);
}

}  // namespace

extern "C" {

int i2v_i3d_create(int32_t num_classes, int32_t in_channels, i2v_i3d** out) {
    I2V_REQUIRE(out && num_classes > 0, I2V_E_INVALID, "i2v_i3d_create: bad argument");
    I2V_REQUIRE(in_channels == 3, I2V_E_INVALID, "i2v_i3d_create: only the rgb network (3 input channels) is built, got %d", in_channels);
    return create_handle("i2v_i3d_create", out, [&](i2v_i3d* n) {
        n->v.num_classes = num_classes;
        n->in_channels = in_channels;
        return I2V_OK;
    });
}

int i2v_dti3d_create(int32_t num_classes, int32_t length, i2v_i3d** out) {
    I2V_REQUIRE(length == 16 || length == 32, I2V_E_INVALID, "i2v_dti3d_create: the dynamic-texture I3D exists for length 16 and 32, got %d", length);
    if (int rc = i2v_i3d_create(num_classes, 3, out)) return rc;
    (*out)->v.dt = length;
    (*out)->v.pool_t = length == 32 ? 4 : 2;   // ID3_32: AvgPool3d((4, 7, 7))
    return I2V_OK;
}

void i2v_i3d_destroy(i2v_i3d* n) { delete n; }

// Kinetics: conv3d_* / mixed_*.branch_* / conv3d_0c_1x1, BatchNorm3d under "batch3d" with eps 1e-3; ID3.InceptionI3D: Conv3d_* /
// Mixed_*.{b0,b1a,b1b,b2a,b2b,b3b} / logits, BatchNorm3d under "bn" with eps 1e-5.  The head has a bias and no norm
// (i2v_i3d_features never launches it).
static int i3d_pack(i2v_i3d* n, const StateDict& sd) {
    static const char* const BR[2][6] = {{".branch_0", ".branch_1.0", ".branch_1.1", ".branch_2.0", ".branch_2.1", ".branch_3.1"},
                                         {".b0", ".b1a", ".b1b", ".b2a", ".b2b", ".b3b"}};
    const bool dt = n->v.dt != 0;
    for (int unit = 0; unit <= I2V_I3D_UNIT_HEAD; ++unit) {
        I3dUnitSpec u;
        i3d_unit_spec(n->v, unit, &u);
        const bool head = unit == I2V_I3D_UNIT_HEAD;
        std::string name = unit == I2V_I3D_UNIT_STEM ? "conv3d_1a_7x7" : unit == I2V_I3D_UNIT_2B ? "conv3d_2b_1x1" : unit == I2V_I3D_UNIT_2C ? "conv3d_2c_3x3"
                           : head ? (dt ? "logits" : "conv3d_0c_1x1")
                                  : std::string(MIXED[(unit - I2V_I3D_UNIT_MIXED) / 6].name) + BR[dt][(unit - I2V_I3D_UNIT_MIXED) % 6];
        if (dt && !head) name[0] = (char)(name[0] - 'a' + 'A');
        if (int rc = n->units[unit].pack(sd, name, u.cin, u.cout, u.k, head ? nullptr : dt ? "bn" : "batch3d", dt ? 1e-5 : 1e-3)) return rc;
    }
    return I2V_OK;
}

int i2v_i3d_load(i2v_i3d* n, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_i3d_load", n, tensors, n_tensors, i3d_pack);
}

size_t i2v_i3d_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t, int32_t h, int32_t w) { return trunk_bytes(n, batch, t, h, w, false); }

int i2v_i3d_forward(i2v_i3d* n, const float* frames, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t denorm, float* logits,
                    void* workspace, size_t workspace_bytes, void* stream) {
    return trunk_forward("i2v_i3d_forward", false, n, frames, batch, t, t, h, w, denorm, logits, workspace, workspace_bytes, stream);
}

size_t i2v_i3d_features_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t_out, int32_t h, int32_t w) {
    return trunk_bytes(n, batch, t_out, h, w, true);
}

int32_t i2v_i3d_feature_steps(const i2v_i3d* n, int32_t t_out) {
    if (!n || t_out <= 0) return 0;
    const TrunkPlan p = i3d_plan<Carver>(n->v, 1, t_out, t_out, I3D_SIDE, I3D_SIDE, true);
    return p.status ? (plan_refusal(p), 0) : p.t_head;
}

int i2v_i3d_features(i2v_i3d* n, const float* frames, int32_t batch, int32_t t_in, int32_t t_out, int32_t h, int32_t w, int32_t denorm,
                     float* feats, void* workspace, size_t workspace_bytes, void* stream) {
    return trunk_forward("i2v_i3d_features", true, n, frames, batch, t_in, t_out, h, w, denorm, feats, workspace, workspace_bytes, stream);
}

// ---- sub-modules of a loaded handle, individually callable on channels-last tensors (for tests and inspection)

int i2v_i3d_unit_shape(const i2v_i3d* n, int32_t unit, int32_t t, int32_t h, int32_t w, int32_t* cin, int32_t* cout, int32_t* out_dims) {
    I2V_REQUIRE(n, I2V_E_INVALID, "i2v_i3d_unit_shape: null handle");
    I2V_REQUIRE(n->loaded, I2V_E_STATE, "i2v_i3d_unit_shape: weights not loaded");
    const bool known = unit >= 0 && unit <= I2V_I3D_UNIT_HEAD;
    I2V_REQUIRE(known && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_unit_shape: unit %d on a [%d, %d, %d] map", unit, t, h, w);
    const Map3 o = unit_plan(n, unit, 1, Map3{t, h, w}, 0, 0, 0).out;
    if (cin) *cin = 4 * n->units[unit].C4;
    if (cout) *cout = n->units[unit].Cout;
    if (out_dims) { out_dims[0] = o.T; out_dims[1] = o.H; out_dims[2] = o.W; }
    return I2V_OK;
}

int i2v_i3d_unit_forward(i2v_i3d* n, int32_t unit, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t in_cs, float* out,
                         int32_t out_cs, int32_t out_off, size_t out_floats, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_i3d_unit_forward");
    I2V_REQUIRE(unit >= 0 && unit <= I2V_I3D_UNIT_HEAD, I2V_E_INVALID, "i2v_i3d_unit_forward: unknown unit %d", unit);
    const Unit* u = &n->units[unit];
    I2V_REQUIRE(x && out && batch > 0 && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_unit_forward: bad argument");
    I2V_REQUIRE(in_cs > 0 && in_cs % 4 == 0 && in_cs >= 4 * u->C4 && out_cs > 0 && out_off >= 0 && out_off + u->Cout <= out_cs, I2V_E_INVALID,
                "i2v_i3d_unit_forward: channels [0, %d) of %d -> [%d, +%d) of %d do not fit", 4 * u->C4, in_cs, out_off, u->Cout, out_cs);
    const TrunkPlan p = unit_plan(n, unit, batch, Map3{t, h, w}, in_cs, out_cs, out_off);
    const Map3 o = p.out;
    I2V_REQUIRE((long)batch * t * h * w * in_cs < TRUNK_SUB_MAX && (long)batch * o.pos() * out_cs < TRUNK_SUB_MAX, I2V_E_INVALID,
                "i2v_i3d_unit_forward: batch %d x [%d, %d, %d] is too large", batch, t, h, w);
    I2V_REQUIRE(out_floats >= (size_t)batch * o.pos() * out_cs, I2V_E_WORKSPACE, "i2v_i3d_unit_forward: output of %zu floats < required %zu",
                out_floats, (size_t)batch * o.pos() * out_cs);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    return launch(n, p, TrunkBufs(x, out), 0, st);
}

size_t i2v_i3d_mixed_workspace_bytes(const i2v_i3d* n, int32_t block, int32_t batch, int32_t t, int32_t h, int32_t w) {
    if (!n || block < 0 || block >= 9 || batch <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    return mixed_plan(n, block, batch, Map3{t, h, w}).total;
}

int i2v_i3d_mixed_forward(i2v_i3d* n, int32_t block, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, float* out, void* workspace,
                          size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_i3d_mixed_forward");
    I2V_REQUIRE(block >= 0 && block < 9, I2V_E_INVALID, "i2v_i3d_mixed_forward: unknown block %d", block);
    I2V_REQUIRE(x && out && workspace && batch > 0 && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_mixed_forward: bad argument");
    I2V_REQUIRE((long)batch * t * h * w * 1024 < TRUNK_SUB_MAX, I2V_E_INVALID, "i2v_i3d_mixed_forward: batch %d x [%d, %d, %d] is too large", batch, t, h,
                w);
    const TrunkPlan p = mixed_plan(n, block, batch, Map3{t, h, w});
    I2V_REQUIRE_WORKSPACE(workspace_bytes, p.total, "i2v_i3d_mixed_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    return launch(n, p, TrunkBufs(x, out).carve(p, workspace), 0, st);
}

int i2v_i3d_maxpool_shape(const i2v_i3d* n, int32_t kt, int32_t k, int32_t st, int32_t s, int32_t t, int32_t h, int32_t w, int32_t* out_dims) {
    I2V_REQUIRE(n && out_dims && kt > 0 && k > 0 && st > 0 && s > 0 && t > 0 && h > 0 && w > 0, I2V_E_INVALID, "i2v_i3d_maxpool_shape: bad argument");
    const Map3 o = pool_plan(n, 1, 4, Map3{t, h, w}, kt, k, st, s).out;
    out_dims[0] = o.T; out_dims[1] = o.H; out_dims[2] = o.W;
    return I2V_OK;
}

int i2v_i3d_maxpool_forward(i2v_i3d* n, const float* x, int32_t batch, int32_t t, int32_t h, int32_t w, int32_t c, int32_t kt, int32_t k, int32_t st,
                            int32_t s, float* out, size_t out_floats, void* stream) {
    I2V_ENTER(sc, n, 0, "i2v_i3d_maxpool_forward");
    I2V_REQUIRE(x && out && batch > 0 && t > 0 && h > 0 && w > 0 && kt > 0 && k > 0 && st > 0 && s > 0, I2V_E_INVALID,
                "i2v_i3d_maxpool_forward: bad argument");
    I2V_REQUIRE(c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_i3d_maxpool_forward: %d channels (a multiple of 4 is needed)", c);
    const TrunkPlan p = pool_plan(n, batch, c, Map3{t, h, w}, kt, k, st, s);
    const Map3 o = p.out;
    I2V_REQUIRE(o.T > 0 && o.H > 0 && o.W > 0 && (long)batch * t * h * w * c < TRUNK_SUB_MAX && (long)batch * o.pos() * c < TRUNK_SUB_MAX,
                I2V_E_INVALID, "i2v_i3d_maxpool_forward: batch %d x [%d, %d, %d] x %d", batch, t, h, w, c);
    const size_t need = (size_t)batch * o.pos() * c;
    I2V_REQUIRE(out_floats >= need, I2V_E_WORKSPACE, "i2v_i3d_maxpool_forward: output of %zu floats < required %zu", out_floats, need);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, hs)) return rco;
    return launch(n, p, TrunkBufs(x, out), 0, hs);
}

// the head's workspace is its I3D_CLS slot; the caller brings I3D_POOLED
size_t i2v_i3d_head_workspace_bytes(const i2v_i3d* n, int32_t batch, int32_t t) {
    if (!n || batch <= 0 || t < n->v.pool_t) return 0;
    return align_up(head_plan(n, batch, t, false).floats[I3D_CLS] * 4, 256);
}

int i2v_i3d_head_forward(i2v_i3d* n, const float* x, int32_t batch, int32_t t, float* pooled, float* feats, float* logits, void* workspace,
                         size_t workspace_bytes, void* stream) {
    I2V_ENTER(sc, n, Entry::NEEDS_WEIGHTS, "i2v_i3d_head_forward");
    I2V_REQUIRE(x && pooled && feats && logits && workspace && batch > 0, I2V_E_INVALID, "i2v_i3d_head_forward: bad argument");
    I2V_REQUIRE(t >= n->v.pool_t && (long)batch * t * 49 * 1024 < TRUNK_SUB_MAX, I2V_E_INVALID,
                "i2v_i3d_head_forward: %d time steps in front of AvgPool3d((%d, 7, 7)), batch %d", t, n->v.pool_t, batch);
    const TrunkPlan p = head_plan(n, batch, t, false);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, align_up(p.floats[I3D_CLS] * 4, 256), "i2v_i3d_head_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(n->order, st)) return rco;
    if (int rc = launch(n, head_plan(n, batch, t, true), TrunkBufs(x, feats), 0, st)) return rc;
    TrunkBufs buf(x, logits);
    buf.p[I3D_POOLED] = pooled;
    buf.p[I3D_CLS] = static_cast<float*>(workspace);
    return launch(n, p, buf, 0, st);
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
