// Stage-1 VAE decoder on gfx950: Generator.forward (reference: stage1_VAE/modules/decoder.py:97-120).
//
// All activations live channels-last ([B][T][H][W][C] fp32) in the caller's workspace.  Per GeneratorBlock
// (decoder.py:33-52) the launch sequence is
//   stats(x)                       per-(b,c) sum / sum-of-squares (fp64 accumulation, coalesced float4 rows)
//   coef                           GroupNorm / InstanceNorm statistics folded with the ADAIN / affine parameters
//                                  into one (A, B) pair per (b,c): norm(x)*g + beta == x*A + B
//   resize + conv2d + conv2d       SPADE branch on the start frame (normalization_layer.py:20-23); gamma and beta
//                                  come out of ONE 128 -> 2C implicit-GEMM conv, "+1" folded into the gamma bias
//   modulate                       a0 = lrelu((x_up*A+B)*gamma' + beta): nearest upsample folded into the read index,
//                                  gamma/beta broadcast over T instead of repeat_interleave'd (:22-23)
//   conv3d 3x3x3 (MFMA)            dx = conv_0(a0)
//   stats + coef + modulate        a1 = lrelu(ADAIN(dx, z))
//   [coef + modulate + conv 1x1x1] learned shortcut, evaluated at the LOW resolution (1x1x1 conv and GroupNorm
//                                  statistics commute with nearest upsampling)
//   conv3d 3x3x3 (MFMA)            out = conv_1(a1) + shortcut (residual read through the upsample index map)
// Spectral norm (W / sigma, signed sigma) is folded once at load time (decoder.py:20-25 recomputes it per call).
#include <algorithm>
#include <cmath>

#include "i2v_dec_block.h"

using namespace i2v;

namespace {

// What i2v_dec_prepare left behind: the SPADE maps of the start frames `img` (B samples, K realizations per frame, h x w, bstride
// floats apart) are in gbs[] of the workspace `ws`; forked: they are being computed on the handle's side stream, SideStream::ev_lvl[k]
// mark them complete.  img == null: nothing is prepared.
// A prepare serves at most the NEXT forward on the handle, and it never survives an error return: every forward drops it on entry,
// before it has checked anything (range error of the previous call, bad argument, workspace too small) -- a later call's start frames
// can sit at the same address (caching allocators, buffers refilled in place).  (A forked prepare that is dropped keeps
// SideStream::unjoined: the next forward / prepare / i2v_dec_join joins it.)
struct Prepared {
    const float* img = nullptr;
    int B = 0, K = 1, h = 0, w = 0;
    long bstride = 0;
    const void* ws = nullptr;
    bool forked = false;
    bool matches(const float* img_, int B_, int K_, int h_, int w_, long bstride_, const void* ws_) const {
        return img == img_ && B == B_ && K == K_ && h == h_ && w == w_ && ws == ws_ && bstride == bstride_;
    }
    void drop() { img = nullptr; }
};

// In-call overlap (round 5): the SPADE conditioning branches of all six blocks depend on the start frames only, so a forward
// that finds no prepared maps runs them on the handle's own side stream (forked from the caller's stream by an event) while the
// caller's stream computes fc / ADAIN linears / head_0 / g_0 ... -- the early levels' launches leave most of the chip idle
// (4x4 .. 16x16 maps), the branches of the late levels fill it.  Every block waits for its level's event; same kernels, same
// bits.  env I2V_DEC_OVERLAP=0: the branches run inline on the caller's stream (round 4).
struct SideStream {
    hipStream_t stream = nullptr;
    bool owned = true;   // false: `stream` is a caller's stream (i2v_dec_set_side_stream), e.g. the one its cINN prefetch runs on
    hipEvent_t ev_fork = nullptr, ev_lvl[6] = {};
    // ... and the learned shortcut of a block (Norm3D + 1x1x1 conv at the low resolution: an HBM-bound GEMM that only conv_1 needs)
    // runs there too, underneath the block's modulate / conv_0 chain: ev_x[k] = block input and its statistics complete (caller's
    // stream), ev_s[k] = shortcut complete (side stream)
    hipEvent_t ev_x[6] = {}, ev_s[6] = {};
    // A forked prepare (or an in-call fork that failed half-way) leaves work on the side stream that nothing on a caller's stream has
    // waited for yet: `unjoined`.  Whoever DROPS such a prepare (i2v_dec_prepare_cancel followed by a forward, a forward with other
    // start frames / another workspace, i2v_dec_join, the destructor) joins the side stream first, so that the lifetime of the
    // caller-owned workspace and start frames is bounded by the caller's stream again (round-5 advisor finding).
    bool unjoined = false;
    // the stream and the events, created at the first fork
    int open() {
        if (!stream) {
            I2V_HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            owned = true;
        }
        if (!ev_fork) {
            I2V_HIP_CHECK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
            for (auto& e : ev_lvl) I2V_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            for (auto& e : ev_x) I2V_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            for (auto& e : ev_s) I2V_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        return I2V_OK;
    }
    // `st` waits for everything enqueued on the side stream so far (a fresh record of ev_fork on the side stream: covers the SPADE
    // branches of every level AND the shortcut GEMMs).  Not while `st` captures: an event recorded outside a capture cannot be waited
    // on inside it; the flag then stays set for the next eager call.
    int join(hipStream_t st) {
        if (!stream || !ev_fork) { unjoined = false; return I2V_OK; }
        if (stream_is_capturing(st)) return I2V_OK;
        I2V_HIP_CHECK(hipEventRecord(ev_fork, stream));
        I2V_HIP_CHECK(hipStreamWaitEvent(st, ev_fork, 0));
        unjoined = false;
        return I2V_OK;
    }
    SideStream() = default;
    SideStream(const SideStream&) = delete;
    SideStream& operator=(const SideStream&) = delete;
    ~SideStream() {
        if (stream) (void)hipStreamSynchronize(stream);   // nothing of this handle may still write the caller's workspace once it is gone
        for (auto& e : ev_x)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_s)
            if (e) (void)hipEventDestroy(e);
        if (stream && owned) (void)hipStreamDestroy(stream);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        for (auto& e : ev_lvl)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace

struct i2v_dec {
    i2v_dec_cfg cfg;
    bool loaded = false;
    int nf = 0;
    // mode, switches, status words, tap, profile: what the block code reads.  mma = auto (2): both weight sets are packed; every forward
    // ends with a stream synchronisation and a look at the operand maxima the writers published -- a 3x3x3 conv whose operand tensor left
    // the window the split format holds 1e-4 in (max |activation| below 2^-10 or above 6400) is switched to the exact-fp32 kernels
    // (Winograd F(4,3) on the fp32 matrix cores where the shape allows, i2v_wino32.hip) for the rest of the handle's life and the forward
    // is run again; an overflow no slot explains (SPADE's own activation, the shortcut GEMM, conv_img) switches the whole handle.
    // In-range checkpoints run exactly the mma = 1 launches.
    BlockCtx ctx;
    int& device = ctx.device;
    Block blk[6];
    Level lvl[6];
    ConvWeights fc, zlin;
    ConvImgSet conv_img;        // every packed form of conv_img (i2v_convimg.hip)
    int Nz = 0;
    int auto_reruns = 0;        // mma = auto: forwards that had to be run again (reporting)
    double prof_conv3_ms = 0, prof_conv3_flops = 0, prof_conv3_exec = 0;   // totals of the resolved profile events
    long prof_conv3_launches = 0;
    Prepared prep;
    // One handle = one workspace, one set of side-stream events: forwards / prepares on a handle are serialised.  A call that arrives
    // on another stream than the previous one first waits for the previous call (event recorded behind every call), like i2v_flow.
    StreamOrder order;   // (capture-aware: i2v_common.h)
    SideStream side;     // (declared last: its destructor waits for the side stream before anything else of the handle goes)
};

namespace {

struct DecWs {
    size_t xA, xB, a, dx, xs_in, xs_low, y0, y1, gb, zl, sums1, sums2, sums3, coef, splitk, splitk_floats, y1v, total;
    size_t gbs[6], py0, py1, py1v;   // i2v_dec_prepare: one gamma|beta buffer per level and its own SPADE scratch
    size_t m6 = 0;                   // exact-fp32 Winograd: the six partial outputs M_x of one conv
    size_t coef_s = 0;
    bool has_y1v = false;
};

// B samples; their SPADE maps and scratch (y0, y1, y1v, gb, gbs, py*) are sized for Fg start frames (realizations: Fg = B / K; 0: B)
DecWs dec_ws(const i2v_dec* d, int B, int Fg = 0) {
    if (Fg <= 0) Fg = B;
    size_t mx_x = (size_t)16 * d->blk[0].n_in, mx_a = 0, mx_dx = 0, mx_xsin = 0, mx_xslow = 0, mx_y = 0, mx_gb = 0, mx_yv = 0, mx_m6 = 0;
    int cmax = 0;
    for (int k = 0; k < 6; ++k) {
        const Block& b = d->blk[k];
        const Level& l = d->lvl[k];
        const size_t P = (size_t)l.T * l.H * l.W, Pl = P / ((size_t)l.ut * l.us * l.us);
        mx_x = std::max(mx_x, P * b.n_out);
        for (const Conv3& c : b.conv) {
            // conv operands: hl16 (4 B per element), or the Winograd operand V (4 values per output pair: 8 B per element)
            mx_a = std::max(mx_a, P * c.cin * (conv3_split_kernel(&d->ctx, c, l) != K_F16 ? 2 : 1));
            // exact-fp32 Winograd: V = 6 planes per 4 positions (1.5 x the activation), M = 6 planes per 4 outputs
            if (conv3_wants(&d->ctx, c, l, K_F32_WINO)) { mx_a = std::max(mx_a, P * c.cin * 3 / 2); mx_m6 = std::max(mx_m6, P * c.cout * 3 / 2); }
        }
        mx_dx = std::max(mx_dx, P * b.n_mid);
        if (b.learned) { mx_xsin = std::max(mx_xsin, Pl * b.n_in); mx_xslow = std::max(mx_xslow, Pl * b.n_out); }
        mx_y = std::max(mx_y, (size_t)l.H * l.W);
        if (spade_wino_wanted(&d->ctx, b, l)) mx_yv = std::max(mx_yv, (size_t)l.H * l.W);   // only levels whose gamma|beta conv runs a Winograd kernel
        mx_gb = std::max(mx_gb, (size_t)l.H * l.W * 2 * b.n_in);
        cmax = std::max(cmax, std::max(b.n_in, b.n_mid));
    }
    if (d->ctx.has16() && d->ctx.img16 == 1 && conv_img_gemm_supported(d->nf)) mx_a = std::max(mx_a, (size_t)d->lvl[5].T * d->lvl[5].H * d->lvl[5].W * 81);  // conv_img's Y
    DecWs L;
    Carver c;
    L.xA = c.take_floats(B * mx_x); L.xB = c.take_floats(B * mx_x);
    L.a = c.take_floats(B * mx_a); L.dx = c.take_floats(B * mx_dx);
    L.xs_in = c.take_floats(B * mx_xsin); L.xs_low = c.take_floats(B * mx_xslow);
    L.y0 = c.take_floats(Fg * mx_y * 16); L.y1 = c.take_floats(Fg * mx_y * 128); L.gb = c.take_floats(Fg * mx_gb);
    L.y1v = c.take_floats(Fg * mx_yv * 256);  // Winograd operand V of SPADE's 128-channel activation (8 bytes per activation)
    L.has_y1v = mx_yv > 0;
    L.zl = c.take_floats((size_t)B * d->Nz);
    L.sums1 = c.take_floats((size_t)B * cmax * 4); L.sums2 = c.take_floats((size_t)B * cmax * 4);  // doubles: 2 per channel
    L.sums3 = c.take_floats((size_t)B * cmax * 4);   // block output statistics (sums1 / sums3 alternate as a block's input / output statistics)
    L.coef = c.take_floats((size_t)B * cmax * 2);
    L.coef_s = c.take_floats((size_t)B * cmax * 2);   // the shortcut's Norm3D coefficients when it runs on the side stream
    {   // split-K scratch of the direct conv kernel (the tiny feature maps of head_0 / g_0): its partial copies of the output
        size_t mx = 0;
        for (int k = 0; k < 6; ++k) {
            const long P = (long)d->lvl[k].T * d->lvl[k].H * d->lvl[k].W;
            const int f = std::max(conv16_splitk_factor(P, (d->blk[k].n_in + 31) / 32), conv16_splitk_factor(P, (d->blk[k].n_mid + 31) / 32));
            if (f > 1) mx = std::max(mx, (size_t)f * P * std::max(d->blk[k].n_mid, d->blk[k].n_out));
        }
        L.splitk_floats = (size_t)B * mx;
        L.splitk = c.take_floats(L.splitk_floats);
    }
    for (int k = 0; k < 6; ++k) L.gbs[k] = c.take_floats((size_t)Fg * d->lvl[k].H * d->lvl[k].W * 2 * d->blk[k].n_in);
    L.py0 = c.take_floats(Fg * mx_y * 16); L.py1 = c.take_floats(Fg * mx_y * 128); L.py1v = c.take_floats(Fg * mx_yv * 256);
    L.m6 = c.take_floats(B * mx_m6);   // exact-fp32 Winograd: the six partial outputs M_x
    L.total = c.total();
    return L;
}

}  // namespace

extern "C" {

int i2v_dec_create(const i2v_dec_cfg* cfg, i2v_dec** out) {
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "i2v_dec_create: null argument");
    I2V_REQUIRE(cfg->channel_factor > 0 && cfg->channel_factor % 8 == 0, I2V_E_INVALID,
                "i2v_dec_create: channel_factor must be a multiple of 8 (Norm3D uses 16 groups), got %d", cfg->channel_factor);
    I2V_REQUIRE(cfg->channel_factor * 16 <= 1024, I2V_E_INVALID, "i2v_dec_create: channel_factor %d too large", cfg->channel_factor);
    I2V_REQUIRE(cfg->z_dim > 0 && cfg->z_dim % 4 == 0, I2V_E_INVALID, "i2v_dec_create: z_dim must be a multiple of 4");
    for (int i = 0; i < 2; ++i) {
        const int s = cfg->upsample_s[i], t = cfg->upsample_t[i];
        I2V_REQUIRE((s == 1 || s == 2 || s == 4) && (t == 1 || t == 2 || t == 4), I2V_E_INVALID,
                    "i2v_dec_create: upsample factors must be 1, 2 or 4");
    }
    I2V_REQUIRE(cfg->mma >= 0 && cfg->mma <= 3, I2V_E_INVALID, "i2v_dec_create: unknown mma mode %d (0 fp32, 1 split-fp16, 2 auto, 3 fp16)", cfg->mma);
    return create_handle("i2v_dec_create", out, [&](i2v_dec* d) {
        d->cfg = *cfg;
        d->ctx.mma = cfg->mma;
        read_switches(&d->ctx, true);
        if (int rc = init_status(&d->ctx)) return rc;
        const int nf = d->nf = cfg->channel_factor;
        const char* names[6] = {"head_0", "g_0", "g_1", "g_2", "g_3", "g_4"};
        const int cin[6] = {16, 16, 16, 8, 4, 2}, cout[6] = {16, 16, 8, 4, 2, 1};
        int T = 1, S = 4, zoff = 0;
        for (int k = 0; k < 6; ++k) {
            Block& b = d->blk[k];
            b.name = names[k];
            b.n_in = cin[k] * nf; b.n_out = cout[k] * nf; b.n_mid = std::min(b.n_in, b.n_out);
            b.learned = b.n_in != b.n_out;
            int g = 16;
            while (b.n_in % g) --g;  // normalization_layer.py:9-10
            b.groups_spade = g;
            b.zoff = zoff;
            zoff += 2 * b.n_mid;
            int ut = 1, us = 1;
            if (k >= 1 && k <= 3) { ut = 2; us = 2; }                                  // decoder.py:102-108
            if (k == 4) { ut = cfg->upsample_t[0]; us = cfg->upsample_s[0]; }          // :111
            if (k == 5) { ut = cfg->upsample_t[1]; us = cfg->upsample_s[1]; }          // :114
            T *= ut; S *= us;
            d->lvl[k] = Level{T, S, S, ut, us};
            init_convs(b, ut == 2);
        }
        d->Nz = zoff;
        return I2V_OK;
    });
}

void i2v_dec_destroy(i2v_dec* d) { delete d; }

static int dec_pack(i2v_dec* d, const StateDict& sd) {
    const int nf = d->nf, zd = d->cfg.z_dim;
    const bool sn = d->cfg.spectral_norm != 0;
    int rc;
    {   // fc: Linear(z_dim, 4*4*16nf) (decoder.py:72); rows permuted so the output is channels-last [h][w][c]
        const int C = 16 * nf;
        const float* w = sd.f32("fc.weight", (int64_t)16 * C * zd);
        const float* b = sd.f32("fc.bias", (int64_t)16 * C);
        if (!w || !b) return I2V_E_MISSING;
        std::vector<float> wp((size_t)16 * C * zd), bp((size_t)16 * C);
        for (int c = 0; c < C; ++c)
            for (int hw = 0; hw < 16; ++hw) {
                std::memcpy(&wp[((size_t)hw * C + c) * zd], w + ((size_t)c * 16 + hw) * zd, (size_t)zd * 4);
                bp[(size_t)hw * C + c] = b[(size_t)c * 16 + hw];
            }
        if ((rc = d->fc.pack(wp.data(), bp.data(), 16 * C, zd, 1, 1, 1, 1.0))) return rc;
    }
    std::vector<float> zw((size_t)d->Nz * zd), zb((size_t)d->Nz);
    for (int k = 0; k < 6; ++k) {
        Block& b = d->blk[k];
        const std::string p = b.name + ".";
        for (int i = 0; i < 2; ++i) {
            // split-fp16: the one kernel the layer's shape selects (mma = 3: F(4,3) in its one-term form); exact fp32: the direct kernel
            // and, from the 8x8 level on, Winograd F(4,3) on the fp32 matrix cores (half the MFMA work of the 27-tap kernel).
            // (mma = auto packs both sets)
            Conv3& c = b.conv[i];
            unsigned variants = 0;
            if (d->ctx.has16()) {
                const Conv3Kernel s = conv3_split_kernel(&d->ctx, c, d->lvl[k]);
                variants |= bit(s == K_F43 && d->ctx.one16() ? K_F43_ONE : s);
            }
            if (d->ctx.has32()) variants |= bit(K_F32) | (conv3_wants(&d->ctx, c, d->lvl[k], K_F32_WINO) ? bit(K_F32_WINO) : 0);
            if ((rc = pack_conv3(sd, p + (i ? "conv_1" : "conv_0"), sn, c, variants))) return rc;
        }
        if (b.learned) {
            if ((rc = sn_pack(sd, p + "conv_s", sn, b.n_out, b.n_in, 1, false, b.convs))) return rc;
            if (d->ctx.has16() && d->ctx.pw16 && (rc = sn_pack(sd, p + "conv_s", sn, b.n_out, b.n_in, 1, false, b.convs16))) return rc;
            const float* gw = sd.f32(p + "norm_s.bn.weight", b.n_in);
            const float* gb = sd.f32(p + "norm_s.bn.bias", b.n_in);
            if (!gw || !gb) return I2V_E_MISSING;
            if ((rc = b.gn_w.upload(gw, (size_t)b.n_in * 4))) return rc;
            if ((rc = b.gn_b.upload(gb, (size_t)b.n_in * 4))) return rc;
        }
        if ((rc = pack_spade(sd, p, b, d->ctx.has16(), d->ctx.has32(), spade_w4_wanted(&d->ctx, b, d->lvl[k]), spade_wino_wanted(&d->ctx, b, d->lvl[k])))) return rc;
        // ADAIN linear rows into the shared z-GEMM
        const float* lw = sd.f32(p + "norm_1.linear.weight", (int64_t)2 * b.n_mid * zd);
        const float* lb = sd.f32(p + "norm_1.linear.bias", (int64_t)2 * b.n_mid);
        if (!lw || !lb) return I2V_E_MISSING;
        std::memcpy(&zw[(size_t)b.zoff * zd], lw, (size_t)2 * b.n_mid * zd * 4);
        std::memcpy(&zb[b.zoff], lb, (size_t)2 * b.n_mid * 4);
    }
    if ((rc = d->zlin.pack(zw.data(), zb.data(), d->Nz, zd, 1, 1, 1, 1.0))) return rc;
    {
        const float* w = sd.f32("conv_img.weight", (int64_t)3 * nf * 27);
        const float* b = sd.f32("conv_img.bias", 3);
        if (!w || !b) return I2V_E_MISSING;
        if ((rc = d->conv_img.pack(w, b, nf, d->lvl[5].T, d->lvl[5].H, d->lvl[5].W, d->ctx.has16(), d->ctx.img16))) return rc;
    }
    return I2V_OK;
}

int i2v_dec_load(i2v_dec* d, const i2v_tensor* tensors, int32_t n_tensors) {
    return load_handle("i2v_dec_load", d, tensors, n_tensors, dec_pack);
}

int i2v_dec_out_shape(const i2v_dec* d, int32_t* t, int32_t* h, int32_t* w) {
    I2V_REQUIRE(d && t && h && w, I2V_E_INVALID, "i2v_dec_out_shape: null argument");
    *t = d->lvl[5].T; *h = d->lvl[5].H; *w = d->lvl[5].W;
    return I2V_OK;
}

size_t i2v_dec_workspace_bytes(const i2v_dec* d, int32_t batch, int32_t img_h, int32_t img_w) {
    (void)img_h; (void)img_w;
    if (!d || batch <= 0) return 0;
    return dec_ws(d, batch).total;
}

size_t i2v_dec_workspace_bytes_realizations(const i2v_dec* d, int32_t frames, int32_t realizations, int32_t img_h, int32_t img_w) {
    (void)img_h; (void)img_w;
    if (!d || frames <= 0 || realizations <= 0 || (int64_t)frames * realizations > INT32_MAX) return 0;
    return dec_ws(d, frames * realizations, frames).total;
}

double i2v_dec_flops_per_sample(const i2v_dec* d, int32_t img_h, int32_t img_w) {
    (void)img_h; (void)img_w;
    if (!d) return 0.0;
    double f = 2.0 * d->cfg.z_dim * (16.0 * 16 * d->nf + d->Nz);
    for (int k = 0; k < 6; ++k) {
        const Block& b = d->blk[k];
        const Level& l = d->lvl[k];
        const double P = (double)l.T * l.H * l.W, HW = (double)l.H * l.W;
        f += 2.0 * P * 27.0 * ((double)b.n_in * b.n_mid + (double)b.n_mid * b.n_out);
        if (b.learned) f += 2.0 * P * (double)b.n_in * b.n_out;  // counted at output resolution, as the reference runs it
        f += 2.0 * HW * 9.0 * (3.0 * 128 + 128.0 * 2 * b.n_in);
    }
    const Level& l = d->lvl[5];
    f += 2.0 * l.T * l.H * l.W * 27.0 * d->nf * 3;
    return f;
}

int i2v_dec_set_profile(i2v_dec* d, int32_t on) {
    I2V_REQUIRE(d, I2V_E_INVALID, "i2v_dec_set_profile: null");
    d->ctx.profile = on;
    d->prof_conv3_ms = d->prof_conv3_flops = d->prof_conv3_exec = 0;
    d->prof_conv3_launches = 0;
    for (auto& pl : d->ctx.prof_layers) pl = BlockCtx::ProfLayer{};
    return I2V_OK;
}

int i2v_dec_debug_tap(i2v_dec* d, int32_t block, int32_t which, float* dst, size_t max_floats) {
    I2V_REQUIRE(d, I2V_E_INVALID, "i2v_dec_debug_tap: null");
    I2V_REQUIRE(!dst || (block >= 0 && block < 6 && which >= 0 && which <= I2V_DEC_TAP_LAST), I2V_E_INVALID,
                "i2v_dec_debug_tap: block %d / tap %d (blocks 0..5, taps 0..%d)", block, which, I2V_DEC_TAP_LAST);
    d->ctx.tap_block = block; d->ctx.tap_which = which; d->ctx.tap_dst = dst; d->ctx.tap_max = max_floats;
    return I2V_OK;
}

int i2v_dec_get_profile(i2v_dec* d, double* conv3_ms, double* conv3_flops, double* conv3_mfma_flops, int64_t* conv3_launches) {
    I2V_REQUIRE(d, I2V_E_INVALID, "i2v_dec_get_profile: null");
    for (auto& ev : d->ctx.prof_events) {
        I2V_HIP_CHECK(hipEventSynchronize(ev.e1));
        float ms = 0;
        I2V_HIP_CHECK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
        d->prof_conv3_ms += ms;
        d->prof_conv3_flops += ev.flops;
        d->prof_conv3_exec += ev.exec_flops;
        d->prof_conv3_launches += 1;
        if (ev.layer >= 0 && ev.layer < 12) {
            auto& pl = d->ctx.prof_layers[ev.layer];
            pl.ms += ms; pl.flops += ev.flops; pl.exec_flops += ev.exec_flops; pl.launches += 1;
        }
        (void)hipEventDestroy(ev.e0);
        (void)hipEventDestroy(ev.e1);
    }
    d->ctx.prof_events.clear();
    if (conv3_ms) *conv3_ms = d->prof_conv3_ms;
    if (conv3_flops) *conv3_flops = d->prof_conv3_flops;
    if (conv3_mfma_flops) *conv3_mfma_flops = d->prof_conv3_exec;
    if (conv3_launches) *conv3_launches = d->prof_conv3_launches;
    return I2V_OK;
}

int i2v_dec_get_layer_profile(i2v_dec* d, int32_t layer, char* name, int32_t name_len, double* ms, double* flops,
                              double* mfma_flops, int64_t* launches, int32_t* kernel) {
    I2V_REQUIRE(d && layer >= 0 && layer < 12, I2V_E_INVALID, "i2v_dec_get_layer_profile: layer index %d", layer);
    if (int rc = i2v_dec_get_profile(d, nullptr, nullptr, nullptr, nullptr)) return rc;  // resolves pending event pairs
    const auto& pl = d->ctx.prof_layers[layer];
    if (name && name_len > 0) snprintf(name, (size_t)name_len, "%s.conv_%d", d->blk[layer / 2].name.c_str(), layer & 1);
    if (ms) *ms = pl.ms;
    if (flops) *flops = pl.flops;
    if (mfma_flops) *mfma_flops = pl.exec_flops;
    if (launches) *launches = pl.launches;
    if (kernel) *kernel = pl.kernel;
    return I2V_OK;
}

int i2v_dec_get_spade_form(i2v_dec* d, int32_t block, int32_t* form) {
    I2V_REQUIRE(d && form && block >= 0 && block < 6, I2V_E_INVALID, "i2v_dec_get_spade_form: block %d (0..5)", block);
    *form = d->blk[block].spade_form;
    return I2V_OK;
}

}  // extern "C"

// The SPADE conditioning branches of all six blocks on the handle's side stream, forked from `st` by an event (everything the
// caller enqueued on `st` before -- the start frames, an earlier forward on this workspace -- is complete before the side stream
// touches the workspace); one event per level for the consumer.  *done = false: not possible here (graph capture on `st`, debug tap
// active, overlap switched off) -- the caller runs the branches inline.
static int fork_spade(i2v_dec* d, const DecWs& L, void* ws, const float* img, int img_h, int img_w, long ibs, int B, hipStream_t st, bool* done) {
    *done = false;
    if (!d->ctx.overlap || d->ctx.tap_dst) return I2V_OK;
    if (stream_is_capturing(st)) return I2V_OK;
    SideStream& sd = d->side;
    if (sd.stream && sd.stream == st) return I2V_OK;   // the caller runs this call ON the shared side stream: nothing to fork to
    if (int rco = sd.open()) return rco;
    float* const y1v = L.has_y1v ? Carver::at(ws, L.y1v) : nullptr;
    float* const py1v = L.has_y1v ? Carver::at(ws, L.py1v) : nullptr;
    I2V_HIP_CHECK(hipEventRecord(sd.ev_fork, st));
    I2V_HIP_CHECK(hipStreamWaitEvent(sd.stream, sd.ev_fork, 0));
    int rc = I2V_OK;
    // A SHARED side stream (i2v_dec_set_side_stream: the caller's cINN prefetch runs on it) typically has the NEXT batch's cINN pass
    // queued in front of these branches: the two tiny first levels (4x4, 8x8 maps: the maps head_0 and g_0 wait for) then run inline on
    // the caller's stream -- with their own scratch -- so that the main chain does not stall behind that pass; the branches of the
    // later levels have the first two blocks' time to get through.  (Own side stream: everything on it, as before.)
    const int k0 = sd.owned ? 0 : 2;
    for (int k = 0; k < k0 && !rc; ++k) {
        rc = spade_branch(&d->ctx, d->blk[k], d->lvl[k], img, img_h, img_w, ibs, B, Carver::at(ws, L.y0), Carver::at(ws, L.y1), y1v, Carver::at(ws, L.gbs[k]), st, k);
        if (!rc && hipEventRecord(sd.ev_lvl[k], st) != hipSuccess) rc = I2V_E_HIP;
    }
    for (int k = k0; k < 6 && !rc; ++k) {
        rc = spade_branch(&d->ctx, d->blk[k], d->lvl[k], img, img_h, img_w, ibs, B, Carver::at(ws, L.py0), Carver::at(ws, L.py1), py1v, Carver::at(ws, L.gbs[k]), sd.stream, k);
        if (!rc && hipEventRecord(sd.ev_lvl[k], sd.stream) != hipSuccess) rc = I2V_E_HIP;
    }
    // (an error must not leave the caller's stream ahead of work this call put on the side stream)
    if (rc) { (void)hipStreamSynchronize(sd.stream); return rc; }
    sd.unjoined = true;
    *done = true;
    return I2V_OK;
}

extern "C" {

int i2v_dec_forward(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, const float* motion, float* out,
                    void* workspace, size_t workspace_bytes, int32_t batch, void* stream) {
    return i2v_dec_forward_strided(d, img, img_h, img_w, 0, motion, out, 0, workspace, workspace_bytes, batch, stream);
}

}  // extern "C"

// batch = samples; K = realizations per start frame: img holds batch / K frames, sample s decodes frame s / K (K = 1: the plain forward)
static int dec_forward_once(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int64_t img_bstride, const float* motion, float* out,
                            int64_t out_bstride, void* workspace, size_t workspace_bytes, int32_t batch, int K, void* stream) {
    Prepared prep;   // dropped before anything is checked: Prepared's rule
    if (d) { prep = d->prep; d->prep.drop(); }
    Entry sc;   // (declared before Join: the end of the call is recorded after the join)
    if (int rc0 = check_entry(sc, d, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_dec_forward")) return rc0;
    I2V_REQUIRE(img && motion && out && workspace && batch > 0 && img_h > 0 && img_w > 0, I2V_E_INVALID,
                "i2v_dec_forward: null argument or bad size");
    const int B = batch;
    I2V_REQUIRE(K >= 1 && B % K == 0, I2V_E_INVALID, "i2v_dec_forward: %d samples are not a multiple of %d realizations", B, K);
    const int Fr = B / K;   // start frames
    {
        const Level& lo = d->lvl[5];
        const int64_t img_dense = (int64_t)3 * img_h * img_w, out_dense = (int64_t)lo.T * 3 * lo.H * lo.W;
        I2V_REQUIRE((img_bstride == 0 || img_bstride >= img_dense) && (out_bstride == 0 || out_bstride >= out_dense), I2V_E_INVALID,
                    "i2v_dec_forward_strided: sample strides %lld / %lld below the dense %lld / %lld", (long long)img_bstride,
                    (long long)out_bstride, (long long)img_dense, (long long)out_dense);
        if (img_bstride == 0) img_bstride = img_dense;
        if (out_bstride == 0) out_bstride = out_dense;
    }
    const DecWs L = dec_ws(d, B, Fr);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_dec_forward");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(d->order, st)) return rco;
    void* const ws = workspace;
    float *xA = Carver::at(ws, L.xA), *xB = Carver::at(ws, L.xB), *a = Carver::at(ws, L.a), *dx = Carver::at(ws, L.dx);
    float *xs_in = Carver::at(ws, L.xs_in), *xs_low = Carver::at(ws, L.xs_low), *y0 = Carver::at(ws, L.y0), *y1 = Carver::at(ws, L.y1);
    float *gb = Carver::at(ws, L.gb), *zl = Carver::at(ws, L.zl), *coef = Carver::at(ws, L.coef);
    double* sums1 = Carver::at<double>(ws, L.sums1);
    double* sums2 = Carver::at<double>(ws, L.sums2);
    int rc;
    // x = fc(motion).reshape(B, 16nf, 1, 4, 4) (decoder.py:99) -- written channels-last [B][1][4][4][16nf]
    if ((rc = conv_forward(d->fc, motion, d->cfg.z_dim, xA, nullptr, 1, 1, B, 1, 1, 1, EPI_NONE, st))) return rc;
    // all six ADAIN Linear(z_dim, 2C) in one GEMM (they depend only on z)
    if ((rc = conv_forward(d->zlin, motion, d->cfg.z_dim, zl, nullptr, 1, 1, B, 1, 1, 1, EPI_NONE, st))) return rc;
    float* x = xA;
    float* xn = xB;
    bool x_stats_ready = false;
    double* sums3 = Carver::at<double>(ws, L.sums3);
    // SPADE branches computed ahead by i2v_dec_prepare for exactly these start frames (same pointer, batch, size, workspace)?
    bool prepared = prep.matches(img, B, K, img_h, img_w, img_bstride, workspace);
    // Prepared on the side stream (i2v_dec_prepare), or not prepared at all: then compute the maps on the handle's side stream now,
    // underneath the first levels (see SideStream).  Either way every block waits for its level's event.
    // While `st` captures a graph the per-level events of a prepare forked BEFORE the capture cannot be waited on (they were recorded
    // outside it): the prepared maps are dropped and the branches run inline, inside the capture (fork_spade refuses to fork there).
    if (prepared && prep.forked && stream_is_capturing(st)) prepared = false;
    bool forked = prepared && prep.forked;
    // A forked prepare this call does NOT consume (other frames / batch / workspace, cancelled, capture): its side-stream work still
    // writes gbs / py0 / py1 of the workspace it was given -- join it before anything of this call touches a workspace.
    if (!forked && d->side.unjoined)
        if (int rcj = d->side.join(st)) return rcj;
    if (!prepared) {
        if (int rcf = fork_spade(d, L, ws, img, img_h, img_w, img_bstride, Fr, st, &forked)) return rcf;
        prepared = forked;
    }
    struct Join {   // an error return below must not leave the caller's stream ahead of the side stream's work on its buffers
        SideStream* side; hipStream_t st; bool on;   // (branches of every level and the shortcut GEMMs: join covers both)
        ~Join() { if (on) (void)side->join(st); }
    } join{&d->side, st, forked};
    for (int k = 0; k < 6; ++k) {
        const Block& b = d->blk[k];
        const Level& l = d->lvl[k];
        double* s_in = (k & 1) ? sums3 : sums1;
        double* s_out = (k & 1) ? sums1 : sums3;
        // Sub-batches (I2V_DEC_SUB = samples per sub-batch, levels whose one sample already fills the chip): the block's launch
        // sequence runs once per sub-batch, so that what one launch writes (dx, the V operands: ~100 MB per sample at the last
        // two levels) is still in the 256 MB Infinity Cache when the next launch reads it.  Every op is per sample: same bits.
        int nsub = B;
        if (d->ctx.sub > 0 && k >= 4 && (long)l.T * l.H * l.W >= 65536) nsub = std::min(B, d->ctx.sub);
        const long Pl = (long)(l.T / l.ut) * (l.H / l.us) * (l.W / l.us), P = (long)l.T * l.H * l.W;
        bool ready_out = x_stats_ready;
        if (forked) {   // this level's gamma | beta maps are complete
            I2V_HIP_CHECK(hipStreamWaitEvent(st, d->side.ev_lvl[k], 0));
            if (k == 5) d->side.unjoined = false;   // every branch has been waited for (a shortcut enqueued below keeps join.on)
        }
        for (int s0 = 0; s0 < B; s0 += nsub) {
            const int n = std::min(nsub, B - s0);
            const int f0 = s0 / K;   // the sub-batch's first start frame (K = 1: s0)
            BlockBufs bufs{a, dx, xs_in, xs_low, y0, y1, gb, coef, s_in + (size_t)s0 * b.n_in * 2, sums2, s_out + (size_t)s0 * b.n_out * 2,
                           Carver::at(ws, L.splitk), L.splitk_floats, L.has_y1v ? Carver::at(ws, L.y1v) : nullptr,
                           prepared ? Carver::at(ws, L.gbs[k]) + (size_t)f0 * l.H * l.W * 2 * b.n_in : nullptr,
                           d->ctx.has32() && d->ctx.wino32 ? Carver::at(ws, L.m6) : nullptr,
                           forked && nsub == B && d->ctx.overlap >= 1 && !d->ctx.no_side_shortcut ? d->side.stream : nullptr, Carver::at(ws, L.coef_s),
                           d->side.ev_x[k], d->side.ev_s[k], GbRows{K, s0 % K}};
            bool ready = x_stats_ready;
            if ((rc = block_forward(&d->ctx, k, d->blk[k], l, x + (size_t)s0 * Pl * b.n_in, xn + (size_t)s0 * P * b.n_out,
                                    img + (size_t)f0 * (size_t)img_bstride, img_h, img_w, img_bstride, zl + (size_t)s0 * d->Nz, d->Nz, n, bufs, ready, k == 5, st)))
                return rc;
            ready_out = ready;
        }
        x_stats_ready = ready_out;
        std::swap(x, xn);
    }
    join.on = false;   // every level's maps and every shortcut have been waited for by their consumers
    {
        const Level& l = d->lvl[5];
        rc = conv_img_run(d->conv_img, conv_img_form(d->conv_img, d->ctx.aux16(), l.T, l.H, l.W), x, out, a, B, l.T, l.H, l.W, st, d->ctx.status_dev,
                          out_bstride);
        if (rc) return rc;
    }
    if (d->ctx.has16()) {
        if ((rc = status_finish(d->ctx.status_dev, st))) return rc;
        I2V_HIP_CHECK(hipMemcpyAsync(d->ctx.status_host, d->ctx.status_dev, I2V_STATUS_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    return I2V_OK;
}

// mma = auto: after a forward has been synchronised, turn what the range guard saw into per-layer decisions.  Returns true when a
// layer (or the whole handle) was switched to the exact-fp32 kernels, i.e. the forward has to be run again.
static bool auto_decide(i2v_dec* d) {
    const int* h = d->ctx.status_host;
    bool changed = false;
    for (int layer = 0; layer < 12; ++layer) {
        const int bits = h[I2V_STATUS_SNAP + 1 + layer];
        if (!bits || d->ctx.fp32_layer[layer]) continue;
        float m;
        std::memcpy(&m, &bits, 4);
        if (!(m >= I2V_UNDERFLOW_MAX && m <= I2V_OVERFLOW_MAX)) { d->ctx.fp32_layer[layer] = true; changed = true; }
    }
    if ((h[0] & 1) && !changed && !d->ctx.fp32_all) { d->ctx.fp32_all = true; changed = true; }   // an overflow no operand slot explains
    return changed;
}

// one forward; mma = auto: re-run (the same call, shared start frames included) until the range guard is satisfied
static int dec_forward(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int64_t img_bstride, const float* motion, float* out,
                       int64_t out_bstride, void* workspace, size_t workspace_bytes, int32_t batch, int K, void* stream) {
    int rc = dec_forward_once(d, img, img_h, img_w, img_bstride, motion, out, out_bstride, workspace, workspace_bytes, batch, K, stream);
    if (rc || !d || d->ctx.mma != 2) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (stream_is_capturing(st)) return rc;   // (a captured forward runs the layer choices made so far; it cannot look at its own flags)
    for (int round = 0; round < 14; ++round) {
        I2V_HIP_CHECK(hipStreamSynchronize(st));
        if (!auto_decide(d)) {
            // what is left in the flag word has been handled (bit 1 -- underflow -- by the per-layer switch; bit 0 cannot remain)
            if (*d->ctx.status_host & 2) { I2V_HIP_CHECK(hipMemsetAsync(d->ctx.status_dev, 0, sizeof(int), st)); *d->ctx.status_host &= ~2; }
            return I2V_OK;
        }
        I2V_HIP_CHECK(hipMemsetAsync(d->ctx.status_dev, 0, sizeof(int), st));
        *d->ctx.status_host = 0;
        d->auto_reruns += 1;
        if ((rc = dec_forward_once(d, img, img_h, img_w, img_bstride, motion, out, out_bstride, workspace, workspace_bytes, batch, K, stream))) return rc;
    }
    I2V_REQUIRE(false, I2V_E_RANGE, "i2v_dec_forward (mma = auto): the range guard still fires with every layer on the exact-fp32 kernels");
}

extern "C" {

int i2v_dec_forward_strided(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int64_t img_bstride, const float* motion, float* out,
                            int64_t out_bstride, void* workspace, size_t workspace_bytes, int32_t batch, void* stream) {
    return dec_forward(d, img, img_h, img_w, img_bstride, motion, out, out_bstride, workspace, workspace_bytes, batch, 1, stream);
}

int i2v_dec_forward_realizations(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int64_t img_bstride, int32_t frames,
                                 int32_t realizations, const float* motion, float* out, int64_t out_bstride, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!(frames > 0 && realizations > 0 && (int64_t)frames * realizations <= INT32_MAX)) {
        if (d) d->prep.drop();   // (Prepared's rule)
        I2V_REQUIRE(false, I2V_E_INVALID, "i2v_dec_forward_realizations: %d frames x %d realizations", frames, realizations);
    }
    return dec_forward(d, img, img_h, img_w, img_bstride, motion, out, out_bstride, workspace, workspace_bytes, frames * realizations,
                       realizations, stream);
}

int i2v_dec_fallback_layers(i2v_dec* d, int32_t* mask, int32_t* reruns) {
    I2V_REQUIRE(d && mask, I2V_E_INVALID, "i2v_dec_fallback_layers: null argument");
    int m = 0;
    for (int layer = 0; layer < 12; ++layer)
        if (d->ctx.fp32_layer[layer] || d->ctx.fp32_all) m |= 1 << layer;
    if (d->ctx.fp32_all) m |= 1 << 30;
    *mask = m;
    if (reruns) *reruns = d->auto_reruns;
    return I2V_OK;
}

}  // extern "C"

// batch = samples of the forward this prepares, K = realizations per start frame: the branches run for the batch / K frames of img
static int dec_prepare(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, void* workspace, size_t workspace_bytes, int32_t batch,
                       int K, void* stream) {
    Entry sc;
    if (int rc0 = check_entry(sc, d, Entry::NEEDS_WEIGHTS | Entry::NULL_IS_UNLOADED, "i2v_dec_prepare")) return rc0;
    I2V_REQUIRE(img && workspace && batch > 0 && img_h > 0 && img_w > 0, I2V_E_INVALID, "i2v_dec_prepare: null argument or bad size");
    I2V_REQUIRE(K >= 1 && batch % K == 0, I2V_E_INVALID, "i2v_dec_prepare: %d samples are not a multiple of %d realizations", batch, K);
    const int B = batch, Fr = batch / K;
    const DecWs L = dec_ws(d, B, Fr);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, L.total, "i2v_dec_prepare");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rco = sc.serialise(d->order, st)) return rco;
    void* const ws = workspace;
    // an earlier forked prepare that was never consumed may have been given ANOTHER workspace (or start frames the caller has
    // released since): `st` joins it before this prepare replaces it
    if (d->side.unjoined && (d->prep.img == nullptr || d->prep.ws != workspace))
        if (int rcj = d->side.join(st)) return rcj;
    d->prep.drop();
    // on the handle's side stream where possible (ordered behind everything already on `st`): the caller's stream stays free for
    // whatever it can do meanwhile, and the consuming forward waits per level; else inline on `st`
    bool forked = false;
    if (int rc = fork_spade(d, L, ws, img, img_h, img_w, 0, Fr, st, &forked)) return rc;
    if (!forked)
        for (int k = 0; k < 6; ++k)
            if (int rc = spade_branch(&d->ctx, d->blk[k], d->lvl[k], img, img_h, img_w, 0, Fr, Carver::at(ws, L.py0), Carver::at(ws, L.py1), L.has_y1v ? Carver::at(ws, L.py1v) : nullptr,
                                      Carver::at(ws, L.gbs[k]), st, k))
                return rc;
    d->prep = Prepared{img, B, K, img_h, img_w, (long)3 * img_h * img_w, workspace, forked};
    return I2V_OK;
}

extern "C" {

int i2v_dec_prepare(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, void* workspace, size_t workspace_bytes, int32_t batch,
                    void* stream) {
    return dec_prepare(d, img, img_h, img_w, workspace, workspace_bytes, batch, 1, stream);
}

int i2v_dec_prepare_realizations(i2v_dec* d, const float* img, int32_t img_h, int32_t img_w, int32_t frames, int32_t realizations,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    I2V_REQUIRE(frames > 0 && realizations > 0 && (int64_t)frames * realizations <= INT32_MAX, I2V_E_INVALID,
                "i2v_dec_prepare_realizations: %d frames x %d realizations", frames, realizations);
    return dec_prepare(d, img, img_h, img_w, workspace, workspace_bytes, frames * realizations, realizations, stream);
}

int i2v_dec_prepare_cancel(i2v_dec* d) {
    I2V_REQUIRE(d, I2V_E_INVALID, "i2v_dec_prepare_cancel: null handle");
    d->prep.drop();
    return I2V_OK;
}

int i2v_dec_set_side_stream(i2v_dec* d, void* side_stream) {
    I2V_ENTER(sc, d, 0, "i2v_dec_set_side_stream");
    hipStream_t ns = static_cast<hipStream_t>(side_stream);
    SideStream& sd = d->side;
    if (sd.stream && sd.stream == ns && !sd.owned) return I2V_OK;
    // whatever the old side stream still carries for this handle completes first (rare: a host wait at configuration time)
    if (sd.stream) {
        I2V_HIP_CHECK(hipStreamSynchronize(sd.stream));
        if (sd.owned) (void)hipStreamDestroy(sd.stream);
    }
    sd.unjoined = false;
    d->prep.drop();
    sd.stream = ns;               // null: the handle creates its own stream again at the next fork
    sd.owned = ns == nullptr;
    return I2V_OK;
}

int i2v_dec_join(i2v_dec* d, void* stream) {
    I2V_ENTER(sc, d, 0, "i2v_dec_join");
    hipStream_t st = static_cast<hipStream_t>(stream);
    I2V_REQUIRE(!stream_is_capturing(st), I2V_E_STATE, "i2v_dec_join: the stream is capturing a graph (join before the capture begins)");
    d->prep.drop();
    return d->side.join(st);
}

int i2v_dec_status(i2v_dec* d, int32_t* flags, int32_t reset, void* stream) {
    I2V_REQUIRE(d && flags, I2V_E_INVALID, "i2v_dec_status: null argument");
    return d->ctx.status(flags, reset, static_cast<hipStream_t>(stream), "i2v_dec_status");
}

}  // extern "C"
