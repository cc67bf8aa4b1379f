// The training path of the motion encoder of stage 1: resnet3D.Encoder (stage1_VAE/modules/resnet3D.py:138-219) forward and backward with
// the parameters read in place -- the 3-D ResNet-18 trunk with GroupNorm(16) that it shares with the temporal discriminator (kernels and
// launchers: i2v_res3d_trunk.h; plan, binding, layout and the two walks: i2v_res3d_net.h), and, here, the posterior head: conv_mu,
// conv_var, the reparameterisation and the KL gradient (loss.py:10-12).
// The C ABI is include/i2v_hip_enc3d_train.h.  Exact fp32 on v_mfma_f32_16x16x4_f32; every sum has one owner and a fixed order.
//   * The trunk differs from the discriminator's in its stem (stride (2, 2, 2)), in the downsample rule (no stride_t term,
//     resnet3D.py:184), and in having neither spectral norm nor a pool.  Its last activation is [N][16][C] (the [1, 4, 4] map).
//   * Head forward: one GEMM [n x 16 C] . [16 C x 2 z], mu and logvar together.  K = (position p, channel c) is cut into C / 16 slices of
//     16 channels, one workgroup per (slice, 16 columns, 16 rows), a wave per 4 channels; the waves are summed in wave order, the
//     slices by e3_head_finish_kernel in slice order, which adds the bias and forms the sample (float64, rounded once).  The weights
//     stay [z][C][4][4]: column j of channel c is 16 contiguous floats, which a lane reads as one float4 (positions 4 q .. 4 q + 3).
//   * Head backward: e3_fold_kernel forms g = (d_mu + d_sample + kl mu / n | d_logvar + d_sample eps e^{lv / 2} / 2 + kl (e^lv - 1) / 2n)
//     [n][2 z]; the input gradient is a sum over the 2 z columns (a workgroup owns 4 channels, its waves every fourth column, summed in
//     wave order); the weight gradient a sum over the n samples, each element written once; the bias gradient a float64 sum over n.
#include "i2v_handle.h"
#include "i2v_res3d_trunk.h"
#include "i2v_res3d_net.h"
#include "../../include/i2v_hip_enc3d_train.h"

#include <cstdint>

namespace i2v {
namespace {

constexpr int E3_JCHUNK = 128;   // columns of g staged in LDS at a time by the head's input gradient

struct E3HeadArgs {
    const float *emb, *w_mu, *w_var, *b_mu, *b_var, *eps;   // emb [n][16][C]; weights [z][C][16]
    const float *g;                                         // backward: [n][2 z]
    float *part;                                            // [S][NR][NC], S = C / 16 slices
    float *sample, *mu, *logvar;
    float *d_emb, *dw_mu, *db_mu, *dw_var, *db_var;
    int n, C, z, NR, NC, accumulate;
};

// grid (C / 16, NC / 16, NR / 16); the k-slot (lane >> 4) of step (u, s) carries position 4 (lane >> 4) + s of channel c0 + u
__global__ __launch_bounds__(256) void e3_head_fwd_kernel(E3HeadArgs a) {
    __shared__ float red[3][4 * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 15, kq = lane >> 4;
    const int j = blockIdx.y * 16 + lr, row = blockIdx.z * 16 + lr;
    const bool jok = j < 2 * a.z, rok = row < a.n;
    const float* wj = !jok ? a.w_mu : j < a.z ? a.w_mu + (long)j * a.C * 16 : a.w_var + (long)(j - a.z) * a.C * 16;
    const int c0 = blockIdx.x * 16 + wave * 4;
    float4 bv[4];
    float av[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float4 v = *reinterpret_cast<const float4*>(wj + (long)(c0 + u) * 16 + 4 * kq);
        bv[u] = jok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float e = a.emb[rok ? ((long)row * 16 + 4 * kq + s) * a.C + c0 + u : 0];
            av[u][s] = rok ? e : 0.f;
        }
    }
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float bs = s == 0 ? bv[u].x : s == 1 ? bv[u].y : s == 2 ? bv[u].z : bv[u].w;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u][s], bs, acc, 0, 0, 0);
        }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave > 0) return;
    // C/D layout: column = lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = acc[r];
        for (int w = 0; w < 3; ++w) v += red[w][r * 64 + lane];
        a.part[((long)blockIdx.x * a.NR + blockIdx.z * 16 + 4 * kq + r) * a.NC + blockIdx.y * 16 + lr] = v;
    }
}

// the slices in slice order, the bias, and sample = eps e^{lv / 2} + mu in float64, rounded once
__global__ __launch_bounds__(256) void e3_head_finish_kernel(E3HeadArgs a) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= (long)a.n * a.z) return;
    const int i = (int)(e / a.z), j = (int)(e % a.z), S = a.C / 16;
    float m = 0.f, l = 0.f;
    for (int s = 0; s < S; ++s) {
        m += a.part[((long)s * a.NR + i) * a.NC + j];
        l += a.part[((long)s * a.NR + i) * a.NC + a.z + j];
    }
    m += a.b_mu[j];
    l += a.b_var[j];
    a.mu[e] = m;
    a.logvar[e] = l;
    if (a.sample) a.sample[e] = (float)((double)a.eps[e] * exp(0.5 * (double)l) + (double)m);
}

struct E3FoldArgs {
    const float *mu, *logvar, *eps, *d_sample, *d_mu, *d_logvar;
    float *g_mu, *g_lv;   // row stride ld
    int n, z, ld;
    float kl_scale;
};

// the gradients at mu and logvar: upstream, the sample's share and the KL term, in float64, rounded once
__global__ __launch_bounds__(256) void e3_fold_kernel(E3FoldArgs a) {
    const long e = blockIdx.x * 256L + threadIdx.x;
    if (e >= (long)a.n * a.z) return;
    const int i = (int)(e / a.z), j = (int)(e % a.z);
    const double m = (double)a.mu[e], l = (double)a.logvar[e];
    double gm = a.d_mu ? (double)a.d_mu[e] : 0.0, gl = a.d_logvar ? (double)a.d_logvar[e] : 0.0;
    if (a.d_sample) {
        const double ds = (double)a.d_sample[e];
        gm += ds;
        gl += ds * (double)a.eps[e] * 0.5 * exp(0.5 * l);
    }
    if (a.kl_scale != 0.f) {
        gm += (double)a.kl_scale * m / (double)a.n;
        gl += (double)a.kl_scale * (exp(l) - 1.0) / (2.0 * (double)a.n);
    }
    a.g_mu[(long)i * a.ld + j] = (float)gm;
    a.g_lv[(long)i * a.ld + j] = (float)gl;
}

// d_emb [i][p][c] = sum over the 2 z columns of g[i][j] w[j][c][p]: grid (C / 4, row tiles of 16); lane = (channel, position), wave w
// takes the columns j = w (mod 4) in rising order
__global__ __launch_bounds__(256) void e3_head_dgrad_kernel(E3HeadArgs a) {
    __shared__ float g_lds[16][E3_JCHUNK];
    __shared__ float red[3][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = blockIdx.x * 4 + (lane >> 4), p = lane & 15, i0 = blockIdx.y * 16, z2 = 2 * a.z;
    float acc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int jb = 0; jb < z2; jb += E3_JCHUNK) {
        __syncthreads();
        for (int e = tid; e < 16 * E3_JCHUNK; e += 256) {
            const int r = e / E3_JCHUNK, jj = e % E3_JCHUNK;
            const bool ok = i0 + r < a.n && jb + jj < z2;
            g_lds[r][jj] = ok ? a.g[(long)(i0 + r) * z2 + jb + jj] : 0.f;
        }
        __syncthreads();
        const int jend = z2 - jb < E3_JCHUNK ? z2 - jb : E3_JCHUNK;
        for (int jj = wave; jj < jend; jj += 4) {
            const int j = jb + jj;
            const float* wj = j < a.z ? a.w_mu + (long)j * a.C * 16 : a.w_var + (long)(j - a.z) * a.C * 16;
            const float wv = wj[(long)c * 16 + p];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = fmaf(g_lds[r][jj], wv, acc[r]);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if (i0 + r >= a.n) continue;
        float v = acc[r];
        for (int w = 0; w < 3; ++w) v += red[w][r][lane];
        a.d_emb[((long)(i0 + r) * 16 + p) * a.C + c] = v;
    }
}

// dW [j][c][p] = sum over the samples (in order) of g[i][j] emb[i][p][c]: one thread per weight
__global__ __launch_bounds__(256) void e3_head_wgrad_kernel(E3HeadArgs a) {
    const long per = (long)a.C * 16, total = 2L * a.z * per;
    for (long e = blockIdx.x * 256L + threadIdx.x; e < total; e += gridDim.x * 256L) {
        const int j = (int)(e / per);
        const int r = (int)(e % per), c = r >> 4, p = r & 15;
        float acc = 0.f;
        for (int i = 0; i < a.n; ++i) acc = fmaf(a.g[(long)i * 2 * a.z + j], a.emb[((long)i * 16 + p) * a.C + c], acc);
        float* dst = j < a.z ? a.dw_mu + e : a.dw_var + (e - (long)a.z * per);
        *dst = a.accumulate ? *dst + acc : acc;
    }
}

__global__ __launch_bounds__(256) void e3_head_bias_kernel(E3HeadArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 2 * a.z) return;
    double s = 0.0;
    for (int i = 0; i < a.n; ++i) s += (double)a.g[(long)i * 2 * a.z + j];
    float* dst = j < a.z ? a.db_mu + j : a.db_var + (j - a.z);
    *dst = a.accumulate ? *dst + (float)s : (float)s;
}

// the largest static LDS footprint of the head's kernels against the 64 KiB a workgroup may take without asking
static_assert(sizeof(float) * (16 * E3_JCHUNK + 3 * 16 * 64) <= 64 * 1024, "e3_head_dgrad_kernel: LDS");

// =================================================================================================================== host side
struct E3HeadWs { size_t part, g, total; int NR, NC; };
E3HeadWs head_ws(int n, int c, int z) {
    E3HeadWs y{};
    y.NR = (int)align_up(n, 16); y.NC = (int)align_up(2 * (size_t)z, 16);
    Carver k;
    y.part = k.take_floats((size_t)(c / 16) * y.NR * y.NC);
    y.g = k.take_floats((size_t)n * 2 * z);
    y.total = k.total();
    return y;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int launch_head_fwd(E3HeadArgs a, void* ws, hipStream_t st) {
    const E3HeadWs k = head_ws(a.n, a.C, a.z);
    a.part = Carver::at(ws, k.part); a.NR = k.NR; a.NC = k.NC;
    hipLaunchKernelGGL(e3_head_fwd_kernel, dim3(a.C / 16, k.NC / 16, k.NR / 16), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(e3_head_finish_kernel, dim3(grid_for((long)a.n * a.z)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_fold(const E3FoldArgs& f, hipStream_t st) {
    hipLaunchKernelGGL(e3_fold_kernel, dim3(grid_for((long)f.n * f.z)), dim3(256), 0, st, f);
    I2V_LAUNCHED();
    return I2V_OK;
}

// fold -> g; the input gradient; with a.dw_mu the four parameter gradients
int launch_head_bwd(E3HeadArgs a, E3FoldArgs f, void* ws, hipStream_t st) {
    const E3HeadWs k = head_ws(a.n, a.C, a.z);
    float* g = Carver::at(ws, k.g);
    f.g_mu = g; f.g_lv = g + a.z; f.ld = 2 * a.z; f.n = a.n; f.z = a.z;
    if (int rc = launch_fold(f, st)) return rc;
    a.g = g;
    hipLaunchKernelGGL(e3_head_dgrad_kernel, dim3(a.C / 4, k.NR / 16), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    if (!a.dw_mu) return I2V_OK;
    hipLaunchKernelGGL(e3_head_wgrad_kernel, dim3(grid_for(2L * a.z * a.C * 16)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(e3_head_bias_kernel, dim3((2 * a.z + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_enc3d_train {
    int device = 0;
    bool loaded = false;   // parameters bound
    bool have_grads = false;
    int z = 0;
    R3Trunk trunk;
    float *wmu = nullptr, *bmu = nullptr, *wvar = nullptr, *bvar = nullptr;
    float *gwmu = nullptr, *gbmu = nullptr, *gwvar = nullptr, *gbvar = nullptr;
};

namespace {

// behind the trunk's entries: eps, mu and logvar in `saved` (y.tail[0 .. 2]), the head's scratch in the workspace (y.ws_tail)
R3Layout e3_layout(const i2v_enc3d_train* d, int n, int t, int h, int w) {
    R3Extra x{"conv_mu and conv_var take", {0, 0, 0}, 0};
    if (n > 0) {
        x.saved[0] = x.saved[1] = x.saved[2] = (size_t)n * d->z * 4;
        x.ws = head_ws(n, d->trunk.L[d->trunk.last()].cout, d->z).total;
    }
    return r3_layout(d->trunk, n, t, h, w, x);
}

// the four head tensors of a state dict or of a gradient dict
bool bind_head(const i2v_enc3d_train* d, const StateDict& s, float** wmu, float** bmu, float** wvar, float** bvar) {
    const int64_t hw = (int64_t)d->z * d->trunk.L[d->trunk.last()].cout * 16;
    return bound_ptr(s, "conv_mu.weight", hw, wmu) && bound_ptr(s, "conv_mu.bias", d->z, bmu) && bound_ptr(s, "conv_var.weight", hw, wvar) &&
           bound_ptr(s, "conv_var.bias", d->z, bvar);
}

int check_head_unit(const char* what, int n, int c, int z) {
    I2V_REQUIRE(n > 0 && z > 0 && c > 0 && c % 16 == 0, I2V_E_INVALID, "%s: n %d, %d channels (a multiple of 16), z %d", what, n, c, z);
    return I2V_OK;
}

}  // namespace

extern "C" {

int i2v_enc3d_train_create(const i2v_enc3d_train_cfg* cfg, i2v_enc3d_train** out) {
    const char* what = "i2v_enc3d_train_create";
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(cfg->z_dim > 0, I2V_E_INVALID, "%s: z_dim %d is not positive", what, cfg->z_dim);
    I2V_REQUIRE(!cfg->use_max_pool, I2V_E_INVALID, "%s: use_max_pool is false in every shipped config and is not supported", what);
    for (int i = 0; i < 5; ++i)
        I2V_REQUIRE(cfg->channels[i] > 0 && cfg->channels[i] % 16 == 0, I2V_E_INVALID, "%s: channels[%d] = %d is not a positive multiple of 16", what, i,
                    cfg->channels[i]);
    for (int i = 0; i < 4; ++i)
        I2V_REQUIRE((cfg->stride_s[i] == 1 || cfg->stride_s[i] == 2) && (cfg->stride_t[i] == 1 || cfg->stride_t[i] == 2), I2V_E_INVALID,
                    "%s: layer %d has strides (t %d, s %d) outside {1, 2}", what, i, cfg->stride_t[i], cfg->stride_s[i]);
    for (int i = 0; i < 4; ++i)
        I2V_REQUIRE(!(cfg->stride_t[i] == 2 && cfg->stride_s[i] == 1 && cfg->channels[i] == cfg->channels[i + 1]), I2V_E_INVALID,
                    "%s: layer %d has stride_t 2 with stride_s 1 and equal widths (%d): no downsample branch exists for its half-rate residual", what, i,
                    cfg->channels[i]);
    const i2v_enc3d_train_cfg c = *cfg;
    return create_handle(what, out, [c](i2v_enc3d_train* d) {
        d->z = c.z_dim;
        r3_build(d->trunk, c.channels, c.stride_s, c.stride_t, R3Rules{2, 2, 0, 0, 0, false});
        return I2V_OK;
    });
}

void i2v_enc3d_train_destroy(i2v_enc3d_train* e) { delete e; }

int i2v_enc3d_train_bind(i2v_enc3d_train* d, const i2v_tensor* params, int32_t n) {
    I2V_REQUIRE(d && params && n > 0, I2V_E_INVALID, "i2v_enc3d_train_bind: null argument");
    d->loaded = false;
    const StateDict sd(params, n);
    if (int rc = r3_bind(d->trunk, sd)) return rc;
    if (!bind_head(d, sd, &d->wmu, &d->bmu, &d->wvar, &d->bvar)) return I2V_E_MISSING;
    I2V_REQUIRE(aligned16(d->wmu) && aligned16(d->wvar), I2V_E_INVALID, "i2v_enc3d_train_bind: conv_mu.weight and conv_var.weight must be 16-byte aligned");
    d->loaded = true;
    return I2V_OK;
}

int i2v_enc3d_train_bind_grads(i2v_enc3d_train* d, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(d && (grads ? n > 0 : n == 0), I2V_E_INVALID, "i2v_enc3d_train_bind_grads: null handle, or a count without tensors");
    d->have_grads = false;
    if (!grads) return I2V_OK;
    const StateDict gd(grads, n);
    if (int rc = r3_bind_grads(d->trunk, gd)) return rc;
    if (!bind_head(d, gd, &d->gwmu, &d->gbmu, &d->gwvar, &d->gbvar)) return I2V_E_MISSING;
    d->have_grads = true;
    return I2V_OK;
}

int i2v_enc3d_train_out_shape(const i2v_enc3d_train* d, int32_t t, int32_t h, int32_t w, int32_t* shape) {
    I2V_REQUIRE(d && shape, I2V_E_INVALID, "i2v_enc3d_train_out_shape: null argument");
    const R3Layout y = e3_layout(d, 1, t, h, w);
    if (!y.ok) return r3_refuse("i2v_enc3d_train_out_shape", y);
    const int last = d->trunk.last();
    shape[0] = y.geo[last].to; shape[1] = y.geo[last].ho; shape[2] = y.geo[last].wo; shape[3] = d->trunk.L[last].cout;
    return I2V_OK;
}

size_t i2v_enc3d_train_saved_bytes(const i2v_enc3d_train* d, int32_t n, int32_t t, int32_t h, int32_t w) {
    return d ? e3_layout(d, n, t, h, w).saved_total : 0;
}
size_t i2v_enc3d_train_workspace_bytes(const i2v_enc3d_train* d, int32_t n, int32_t t, int32_t h, int32_t w) {
    return d ? e3_layout(d, n, t, h, w).ws_total : 0;
}

int i2v_enc3d_train_saved_layout(const i2v_enc3d_train* d, int32_t n, int32_t t, int32_t h, int32_t w, int32_t* count, int32_t* kind, int32_t* conv,
                                 int32_t* dims, int64_t* offset) {
    I2V_REQUIRE(d && count && kind && conv && dims && offset, I2V_E_INVALID, "i2v_enc3d_train_saved_layout: null argument");
    const R3Layout y = e3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse("i2v_enc3d_train_saved_layout", y);
    R3Table tab{kind, conv, dims, offset};
    tab.put_convs(d->trunk, y, I2V_ENC3D_TRAIN_CONV_OUT, I2V_ENC3D_TRAIN_ACT);
    *count = tab.count;
    return I2V_OK;
}

int i2v_enc3d_train_forward(i2v_enc3d_train* d, const float* x, const float* eps, int32_t n, int32_t t, int32_t h, int32_t w, int32_t flags,
                            float* sample, float* mu, float* logvar, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const char* what = "i2v_enc3d_train_forward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(x && mu && logvar && workspace && !eps == !sample, I2V_E_INVALID, "%s: null argument, or eps without sample (or the reverse)", what);
    const R3Layout y = e3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse(what, y);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    const bool save = flags & I2V_ENC3D_TRAIN_SAVE;
    if (save) {
        I2V_REQUIRE(saved, I2V_E_INVALID, "%s: I2V_ENC3D_TRAIN_SAVE without a saved buffer", what);
        I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = save ? saved : Carver::at<char>(workspace, y.fwd);
    if (int rc = r3_forward(d->trunk, y, x, false, nullptr, sv, workspace, st)) return rc;
    const int last = d->trunk.last();
    float* seps = Carver::at(sv, y.tail[0]);
    float* smu = Carver::at(sv, y.tail[1]);
    float* slv = Carver::at(sv, y.tail[2]);
    E3HeadArgs a{};
    a.emb = Carver::at(sv, y.act[last]); a.w_mu = d->wmu; a.w_var = d->wvar; a.b_mu = d->bmu; a.b_var = d->bvar; a.eps = eps;
    a.sample = sample; a.mu = smu; a.logvar = slv; a.n = n; a.C = d->trunk.L[last].cout; a.z = d->z;
    if (int rc = launch_head_fwd(a, Carver::at<char>(workspace, y.ws_tail), st)) return rc;
    const size_t zb = (size_t)n * d->z * 4;
    I2V_HIP_CHECK(hipMemcpyAsync(mu, smu, zb, hipMemcpyDeviceToDevice, st));
    I2V_HIP_CHECK(hipMemcpyAsync(logvar, slv, zb, hipMemcpyDeviceToDevice, st));
    if (eps) I2V_HIP_CHECK(hipMemcpyAsync(seps, eps, zb, hipMemcpyDeviceToDevice, st));
    else I2V_HIP_CHECK(hipMemsetAsync(seps, 0, zb, st));
    return I2V_OK;
}

int i2v_enc3d_train_backward(i2v_enc3d_train* d, const float* d_sample, const float* d_mu, const float* d_logvar, float kl_scale, const void* saved,
                             size_t saved_bytes, int32_t n, int32_t t, int32_t h, int32_t w, float* d_x, int32_t param_grads, int32_t accumulate,
                             void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_enc3d_train_backward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(saved && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(d_x || param_grads, I2V_E_INVALID, "%s: neither the input gradient nor the parameter gradients are asked for", what);
    I2V_REQUIRE(d_sample || d_mu || d_logvar || kl_scale != 0.f, I2V_E_INVALID,
                "%s: no upstream gradient (d_sample, d_mu and d_logvar are null and kl_scale is 0)", what);
    I2V_REQUIRE(!param_grads || d->have_grads, I2V_E_STATE, "%s: no gradient tensors are bound", what);
    const R3Layout y = e3_layout(d, n, t, h, w);
    if (!y.ok) return r3_refuse(what, y);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = const_cast<void*>(saved);
    const bool acc = accumulate != 0, pg = param_grads != 0;

    // the head: the gradient at the last activation -> gbuf[0]
    const int last = d->trunk.last();
    E3HeadArgs a{};
    a.emb = Carver::at(sv, y.act[last]); a.w_mu = d->wmu; a.w_var = d->wvar; a.n = n; a.C = d->trunk.L[last].cout; a.z = d->z;
    a.d_emb = Carver::at(workspace, y.gbuf[0]);
    if (pg) { a.dw_mu = d->gwmu; a.db_mu = d->gbmu; a.dw_var = d->gwvar; a.db_var = d->gbvar; }
    a.accumulate = acc ? 1 : 0;
    E3FoldArgs f{};
    f.eps = Carver::at(sv, y.tail[0]); f.mu = Carver::at(sv, y.tail[1]); f.logvar = Carver::at(sv, y.tail[2]);
    f.d_sample = d_sample; f.d_mu = d_mu; f.d_logvar = d_logvar; f.kl_scale = kl_scale;
    if (int rc = launch_head_bwd(a, f, Carver::at<char>(workspace, y.ws_tail), st)) return rc;
    return r3_backward(d->trunk, y, nullptr, sv, d_x, pg, acc, workspace, st);
}

int i2v_enc3d_kl_backward(const float* mu, const float* logvar, int32_t n, int32_t z, float scale, float* d_mu, float* d_logvar, void* stream) {
    I2V_REQUIRE(mu && logvar && d_mu && d_logvar && n > 0 && z > 0, I2V_E_INVALID, "i2v_enc3d_kl_backward: null argument, n %d or z %d", n, z);
    E3FoldArgs f{};
    f.mu = mu; f.logvar = logvar; f.kl_scale = scale; f.g_mu = d_mu; f.g_lv = d_logvar; f.ld = z; f.n = n; f.z = z;
    return launch_fold(f, static_cast<hipStream_t>(stream));
}

size_t i2v_enc3d_head_workspace_bytes(int32_t n, int32_t c, int32_t z) { return n > 0 && c > 0 && c % 16 == 0 && z > 0 ? head_ws(n, c, z).total : 0; }

int i2v_enc3d_head_forward_unit(const float* emb, const float* w_mu, const float* b_mu, const float* w_var, const float* b_var, const float* eps,
                                int32_t n, int32_t c, int32_t z, float* sample, float* mu, float* logvar, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const char* what = "i2v_enc3d_head_forward_unit";
    if (int rc = check_head_unit(what, n, c, z)) return rc;
    I2V_REQUIRE(emb && w_mu && b_mu && w_var && b_var && mu && logvar && workspace && !eps == !sample && aligned16(w_mu) && aligned16(w_var), I2V_E_INVALID,
                "%s: null argument, eps without sample (or the reverse), or a weight that is not 16-byte aligned", what);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, head_ws(n, c, z).total, what);
    E3HeadArgs a{};
    a.emb = emb; a.w_mu = w_mu; a.w_var = w_var; a.b_mu = b_mu; a.b_var = b_var; a.eps = eps; a.sample = sample; a.mu = mu; a.logvar = logvar;
    a.n = n; a.C = c; a.z = z;
    return launch_head_fwd(a, workspace, static_cast<hipStream_t>(stream));
}

int i2v_enc3d_head_backward_unit(const float* emb, const float* w_mu, const float* w_var, const float* mu, const float* logvar, const float* eps,
                                 const float* d_sample, const float* d_mu, const float* d_logvar, float kl_scale, int32_t n, int32_t c, int32_t z,
                                 float* d_emb, float* dw_mu, float* db_mu, float* dw_var, float* db_var, int32_t accumulate, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const char* what = "i2v_enc3d_head_backward_unit";
    if (int rc = check_head_unit(what, n, c, z)) return rc;
    I2V_REQUIRE(emb && w_mu && w_var && mu && logvar && d_emb && workspace && (!d_sample || eps), I2V_E_INVALID,
                "%s: null argument, or d_sample without eps", what);
    I2V_REQUIRE(!dw_mu == !db_mu && !dw_mu == !dw_var && !dw_mu == !db_var, I2V_E_INVALID, "%s: the four parameter gradients come together or not at all",
                what);
    I2V_REQUIRE(d_sample || d_mu || d_logvar || kl_scale != 0.f, I2V_E_INVALID, "%s: no upstream gradient and kl_scale 0", what);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, head_ws(n, c, z).total, what);
    E3HeadArgs a{};
    a.emb = emb; a.w_mu = w_mu; a.w_var = w_var; a.n = n; a.C = c; a.z = z; a.d_emb = d_emb;
    a.dw_mu = dw_mu; a.db_mu = db_mu; a.dw_var = dw_var; a.db_var = db_var; a.accumulate = accumulate ? 1 : 0;
    E3FoldArgs f{};
    f.mu = mu; f.logvar = logvar; f.eps = eps; f.d_sample = d_sample; f.d_mu = d_mu; f.d_logvar = d_logvar; f.kl_scale = kl_scale;
    return launch_head_bwd(a, f, workspace, static_cast<hipStream_t>(stream));
}

}  // extern "C"
