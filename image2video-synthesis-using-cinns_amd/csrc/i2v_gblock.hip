// Stand-alone GeneratorBlock / Spade / ADAIN / Norm3D (reference tensors [B][C][T][H][W] in and out): one block of the decoder
// (i2v_dec_block.h) behind a handle of its own, for the sub-module entry points of stage1_VAE/modules.
#include <algorithm>

#include "i2v_dec_block.h"

namespace i2v {

// Layout conversion for the stand-alone sub-module entry points: the reference surface is [B][C][T][H][W] ("NCDHW"),
// the kernels work channels-last.  32x32 tiles through LDS, both sides coalesced.  to_cl: in [B][C][P] -> out [B][P][C].
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int C, int P,
                                                        int to_cl) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int R = to_cl ? C : P, S = to_cl ? P : C;  // input is [R][S] per sample, output [S][R]
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

}  // namespace i2v

using namespace i2v;

struct i2v_gblock {
    BlockCtx ctx;
    int& device = ctx.device;
    bool loaded = false;   // a load has succeeded; which groups of keys it carried: has_*
    Block b;
    ConvWeights zlin;  // this block's ADAIN Linear(z_dim, 2*n_mid)
    int z_dim = 0;
    bool spectral_norm = false;
    bool has_convs = false, has_spade = false, has_adain = false, has_norm_s = false;
};

namespace {

struct GbWs { size_t x_cl, out_cl, a, dx, xs_in, xs_low, y0, y1, gb, zl, sums1, sums2, coef, total; };

GbWs gb_ws(const i2v_gblock* g, int B, int T, int H, int W) {
    const Block& b = g->b;
    const size_t P = (size_t)T * H * W, cm = std::max(b.n_in, std::max(b.n_mid, b.n_out));
    GbWs L;
    Carver c;
    L.x_cl = c.take_floats(B * P * cm); L.out_cl = c.take_floats(B * P * cm); L.a = c.take_floats(B * P * cm * 2); L.dx = c.take_floats(B * P * b.n_mid);
    L.xs_in = c.take_floats(B * P * b.n_in); L.xs_low = c.take_floats(B * P * b.n_out);
    L.y0 = c.take_floats((size_t)B * H * W * 16); L.y1 = c.take_floats((size_t)B * H * W * 128); L.gb = c.take_floats((size_t)B * H * W * 2 * b.n_in);
    L.zl = c.take_floats((size_t)B * 2 * b.n_mid);
    L.sums1 = c.take_floats((size_t)B * cm * 4); L.sums2 = c.take_floats((size_t)B * cm * 4); L.coef = c.take_floats((size_t)B * cm * 2);
    L.total = c.total();
    return L;
}

int run_transpose(const float* in, float* out, int B, int C, long P, bool to_cl, hipStream_t st) {
    const int R = to_cl ? C : (int)P, S = to_cl ? (int)P : C;
    hipLaunchKernelGGL(transpose_kernel, dim3((S + 31) / 32, (R + 31) / 32, B), dim3(256), 0, st, in, out, C, (int)P, to_cl ? 1 : 0);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // namespace

extern "C" {

int i2v_gblock_create(int32_t n_in, int32_t n_out, int32_t z_dim, int32_t spectral_norm, int32_t mma, i2v_gblock** out) {
    I2V_REQUIRE(out && n_in > 0 && n_out > 0 && n_in % 8 == 0 && n_out % 8 == 0 && n_in <= 1024 && n_out <= 1024, I2V_E_INVALID,
                "i2v_gblock_create: channel counts must be multiples of 8 in [8, 1024]");
    I2V_REQUIRE(z_dim > 0 && z_dim % 4 == 0 && (mma == 0 || mma == 1 || mma == 3), I2V_E_INVALID, "i2v_gblock_create: bad z_dim / mma (0 fp32, 1 split-fp16, 3 fp16)");
    // the learned shortcut's Norm3D is GroupNorm(16, n_in) (normalization_layer.py:31), which needs n_in % 16 == 0
    I2V_REQUIRE(n_in == n_out || n_in % 16 == 0, I2V_E_INVALID,
                "i2v_gblock_create: a learned shortcut needs n_in %% 16 == 0 (GroupNorm(16, n_in)), got n_in %d", n_in);
    return create_handle("i2v_gblock_create", out, [&](i2v_gblock* g) {
        g->ctx.mma = mma;
        g->spectral_norm = spectral_norm != 0;
        read_switches(&g->ctx, false);
        if (int rc = init_status(&g->ctx)) return rc;
        g->z_dim = z_dim;
        Block& b = g->b;
        b.name = "";
        b.n_in = n_in; b.n_out = n_out; b.n_mid = std::min(n_in, n_out);
        b.learned = n_in != n_out;
        int grp = 16;
        while (n_in % grp) --grp;
        b.groups_spade = grp;
        b.zoff = 0;
        init_convs(b, false);
        return I2V_OK;
    });
}

void i2v_gblock_destroy(i2v_gblock* g) { delete g; }

static int gblock_pack(i2v_gblock* g, const StateDict& sd) {
    Block& b = g->b;
    const bool sn = g->spectral_norm, f16 = g->ctx.has16(), one = g->ctx.one16();
    int rc;
    g->has_convs = g->has_spade = g->has_adain = g->has_norm_s = false;
    if (sd.has(sn ? "conv_0.weight_orig" : "conv_0.weight")) {
        // the geometry is only known at the call: next to the direct kernel, pack the Winograd variants where the channel counts allow
        // them at a nominal 16 x 64 x 64 -- F(2,3), and F(4,3) (used where the call's geometry gives a sample >= 32 workgroups;
        // I2V_DEC_WINO4=2: always; mma = 3: its one-term form instead)
        const Level probe{16, 64, 64, 1, 1};
        for (int i = 0; i < 2; ++i) {
            Conv3& c = b.conv[i];
            unsigned variants = bit(K_F32);
            if (f16) variants = bit(K_F16) | (conv3_wants(&g->ctx, c, probe, K_F23) ? bit(K_F23) : 0) |
                                (conv3_wants(&g->ctx, c, probe, K_F43) ? bit(one ? K_F43_ONE : K_F43) : 0);
            if ((rc = pack_conv3(sd, i ? "conv_1" : "conv_0", sn, c, variants))) return rc;
        }
        if (b.learned && (rc = sn_pack(sd, "conv_s", sn, b.n_out, b.n_in, 1, false, b.convs))) return rc;
        if (b.learned && f16 && g->ctx.pw16 && (rc = sn_pack(sd, "conv_s", sn, b.n_out, b.n_in, 1, false, b.convs16))) return rc;
        g->has_convs = true;
    }
    if (sd.has("norm_s.bn.weight")) {
        const float* gw = sd.f32("norm_s.bn.weight", b.n_in);
        const float* gb = sd.f32("norm_s.bn.bias", b.n_in);
        if (!gw || !gb) return I2V_E_MISSING;
        if ((rc = b.gn_w.upload(gw, (size_t)b.n_in * 4))) return rc;
        if ((rc = b.gn_b.upload(gb, (size_t)b.n_in * 4))) return rc;
        g->has_norm_s = true;
    }
    if (sd.has("norm_0.conv.weight")) {
        if ((rc = pack_spade(sd, "", b, f16, !f16, false, false))) return rc;
        g->has_spade = true;
    }
    if (sd.has("norm_1.linear.weight")) {
        const float* lw = sd.f32("norm_1.linear.weight", (int64_t)2 * b.n_mid * g->z_dim);
        const float* lb = sd.f32("norm_1.linear.bias", (int64_t)2 * b.n_mid);
        if (!lw || !lb) return I2V_E_MISSING;
        if ((rc = g->zlin.pack(lw, lb, 2 * b.n_mid, g->z_dim, 1, 1, 1, 1.0))) return rc;
        g->has_adain = true;
    }
    I2V_REQUIRE(g->has_convs || g->has_spade || g->has_adain || g->has_norm_s, I2V_E_MISSING,
                "i2v_gblock_load: no GeneratorBlock / Spade / ADAIN / Norm3D keys found");
    return I2V_OK;
}

int i2v_gblock_load(i2v_gblock* g, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_gblock_load", g, tensors, n_tensors, gblock_pack);
}

size_t i2v_gblock_workspace_bytes(const i2v_gblock* g, int32_t batch, int32_t t, int32_t h, int32_t w) {
    if (!g || batch <= 0 || t <= 0 || h <= 0 || w <= 0) return 0;
    return gb_ws(g, batch, t, h, w).total;
}

int i2v_gblock_forward(i2v_gblock* g, const float* x, const float* z, const float* img, int32_t img_h, int32_t img_w, float* out,
                       void* workspace, size_t workspace_bytes, int32_t batch, int32_t t, int32_t h, int32_t w, void* stream) {
    Entry sc;
    if (int rc0 = check_entry(sc, g, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_gblock_forward")) return rc0;
    I2V_REQUIRE(g->has_convs && g->has_spade && g->has_adain && (!g->b.learned || g->has_norm_s), I2V_E_STATE,
                "i2v_gblock_forward: block weights not (fully) loaded");
    I2V_REQUIRE(x && z && img && out && workspace && batch > 0, I2V_E_INVALID, "i2v_gblock_forward: null argument");
    const GbWs L = gb_ws(g, batch, t, h, w);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_gblock_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* const ws = workspace;
    float *x_cl = Carver::at(ws, L.x_cl), *out_cl = Carver::at(ws, L.out_cl), *zl = Carver::at(ws, L.zl);
    const long P = (long)t * h * w;
    Block& b = g->b;
    int rc;
    if ((rc = run_transpose(x, x_cl, batch, b.n_in, P, true, st))) return rc;
    if ((rc = conv_forward(g->zlin, z, g->z_dim, zl, nullptr, 1, 1, batch, 1, 1, 1, EPI_NONE, st))) return rc;
    BlockBufs bufs{Carver::at(ws, L.a), Carver::at(ws, L.dx), Carver::at(ws, L.xs_in), Carver::at(ws, L.xs_low), Carver::at(ws, L.y0),
                   Carver::at(ws, L.y1), Carver::at(ws, L.gb), Carver::at(ws, L.coef), Carver::at<double>(ws, L.sums1),
                   Carver::at<double>(ws, L.sums2)};
    bool ready = false;
    const Level l{t, h, w, 1, 1};
    if ((rc = block_forward(&g->ctx, 0, b, l, x_cl, out_cl, img, img_h, img_w, 0, zl, 2 * b.n_mid, batch, bufs, ready, false, st)))
        return rc;
    if ((rc = run_transpose(out_cl, out, batch, b.n_out, P, false, st))) return rc;
    if (g->ctx.has16()) {
        if ((rc = status_finish(g->ctx.status_dev, st))) return rc;
        I2V_HIP_CHECK(hipMemcpyAsync(g->ctx.status_host, g->ctx.status_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    return I2V_OK;
}

int i2v_gblock_status(i2v_gblock* g, int32_t* flags, int32_t reset, void* stream) {
    I2V_REQUIRE(g && flags, I2V_E_INVALID, "i2v_gblock_status: null argument");
    return g->ctx.status(flags, reset, static_cast<hipStream_t>(stream), "i2v_gblock_status");
}

int i2v_gblock_norm(i2v_gblock* g, int32_t part, const float* x, const float* cond, int32_t img_h, int32_t img_w, float* out,
                    void* workspace, size_t workspace_bytes, int32_t batch, int32_t t, int32_t h, int32_t w, void* stream) {
    Entry sc;
    if (int rc0 = check_entry(sc, g, Entry::NEEDS_WEIGHTS, "i2v_gblock_norm")) return rc0;
    I2V_REQUIRE(x && out && workspace && batch > 0 && part >= 0 && part <= 2, I2V_E_INVALID, "i2v_gblock_norm: bad argument");
    const GbWs L = gb_ws(g, batch, t, h, w);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_gblock_norm");
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* const ws = workspace;
    const long P = (long)t * h * w;
    Block& b = g->b;
    const int B = batch;
    double* sums = Carver::at<double>(ws, L.sums1);
    float *x_cl = Carver::at(ws, L.x_cl), *a = Carver::at(ws, L.a), *coef = Carver::at(ws, L.coef), *zl = Carver::at(ws, L.zl), *gb = Carver::at(ws, L.gb);
    int rc;
    const int C = part == 1 ? b.n_mid : b.n_in;
    if ((rc = run_transpose(x, x_cl, B, C, P, true, st))) return rc;
    if ((rc = stats_forward(x_cl, sums, B, P, C, st))) return rc;
    if (part == 0) {        // Spade.forward(x, img), normalization_layer.py:18-24
        I2V_REQUIRE(g->has_spade && cond, I2V_E_STATE, "i2v_gblock_norm: Spade weights not loaded / no start frame");
        if ((rc = coef_forward(sums, coef, B, C, b.groups_spade, (double)P, st))) return rc;
        if ((rc = spade_branch(&g->ctx, b, Level{t, h, w, 1, 1}, cond, img_h, img_w, 0, B, Carver::at(ws, L.y0), Carver::at(ws, L.y1), nullptr, gb, st))) return rc;
        if ((rc = run_modulate(x_cl, coef, gb, a, B, t, h, w, C, 1, 1, 0, st))) return rc;
    } else if (part == 1) { // ADAIN.forward(x, z), normalization_layer.py:47-51
        I2V_REQUIRE(g->has_adain && cond, I2V_E_STATE, "i2v_gblock_norm: ADAIN weights not loaded / no latent");
        if ((rc = conv_forward(g->zlin, cond, g->z_dim, zl, nullptr, 1, 1, B, 1, 1, 1, EPI_NONE, st))) return rc;
        if ((rc = coef_forward(sums, coef, B, C, C, (double)P, st, nullptr, nullptr, zl, 2 * b.n_mid, 0))) return rc;
        if ((rc = run_modulate(x_cl, coef, nullptr, a, B, t, h, w, C, 1, 1, 0, st))) return rc;
    } else {                // Norm3D.forward(x), normalization_layer.py:33-35
        I2V_REQUIRE(C % 16 == 0, I2V_E_INVALID, "i2v_gblock_norm: Norm3D is GroupNorm(16, C), needs C %% 16 == 0, got %d", C);
        I2V_REQUIRE(g->has_norm_s, I2V_E_STATE, "i2v_gblock_norm: Norm3D weights not loaded");
        if ((rc = coef_forward(sums, coef, B, C, 16, (double)P, st, b.gn_w.as<float>(), b.gn_b.as<float>()))) return rc;
        if ((rc = run_modulate(x_cl, coef, nullptr, a, B, t, h, w, C, 1, 1, 0, st))) return rc;
    }
    return run_transpose(a, out, B, C, P, false, st);
}

}  // extern "C"
