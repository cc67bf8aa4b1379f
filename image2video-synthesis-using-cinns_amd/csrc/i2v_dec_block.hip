// One GeneratorBlock on channels-last tensors and the load-time code of its weights (see i2v_dec_block.h).
#include <algorithm>
#include <cmath>

#include "i2v_dec_block.h"

namespace i2v {

// F(4,3): its bricks hold 512 output positions x 64 or 32 channels (the launcher picks 32-channel workgroups when 64-channel ones
// would not fill the chip; both give the same bits) -- wherever one SAMPLE gives >= 16 workgroups of 32 channels, i.e. from the
// 16x16 level on (round 3 stopped at 32x32: g_1 ran F(2,3); measured at B = 64: g_1.conv_0 1.94 -> 1.49 ms, conv_1 1.47 -> 1.13,
// at B = 8 equal).  WHETHER a layer runs F(4,3) depends on the layer only; the workgroup width (64 or 32 channels) is chosen by the
// launcher from batch x bricks against the CU count -- it changes the schedule, not the accumulation order of any output, so
// shards reproduce the full batch bit for bit (test_f43_tile_width_switch_across_batches crosses the threshold).
static bool w4_fills(const Level& l, int cout) { return (long)l.T * l.H * l.W / 512 * std::max(cout / 32, 1) >= 16; }

// Wanted by shape: would a conv of (cin, cout, tdup) at this level run kernel `kn` (K_F43, K_F23 or K_F32_WINO) under the handle's
// switches?  (A tdup conv reads the half-rate tensor through pair kernels: T / 2 frames, 2 temporal taps.)
bool conv3_wants(const BlockCtx* d, const Conv3& c, const Level& l, Conv3Kernel kn) {
    const int T = c.tdup ? l.T / 2 : l.T, KT = c.tdup ? 2 : 3;
    switch (kn) {
    case K_F43: return d->has16() && d->wino && d->wino4 && (d->wino4 == 2 || w4_fills(l, c.cout)) && wino4_supported(c.cout, c.cin, T, l.H, l.W, KT);
    case K_F23: return d->has16() && d->wino && wino16_supported(c.cout, c.cin, T, l.H, l.W, KT);
    case K_F32_WINO: return d->has32() && d->wino32 && wino4f32_supported(c.cout, c.cin, l.T, l.H, l.W);
    default: return false;
    }
}
// ... and the split-fp16 kernel it would run: layers whose shape allows it run on a Winograd kernel (F(4,3) before F(2,3): 1.5x / 2x
// fewer MFMAs), the rest on the direct one
Conv3Kernel conv3_split_kernel(const BlockCtx* d, const Conv3& c, const Level& l) {
    return conv3_wants(d, c, l, K_F43) ? K_F43 : conv3_wants(d, c, l, K_F23) ? K_F23 : K_F16;
}

// SPADE's gamma|beta Conv2d(128, 2C, 3) on a Winograd kernel (F(4,3) 1x3x3 variant, else F(2,3)): the predicate of
// i2v_dec_load's packing and of the y1v workspace
bool spade_w4_wanted(const BlockCtx* d, const Block& b, const Level& l) {
    return d->has16() && d->wino && d->spw && d->wino4 && (2 * b.n_in) % 64 == 0 && wino4_supported(2 * b.n_in, 128, 1, l.H, l.W, 1);
}
bool spade_wino_wanted(const BlockCtx* d, const Block& b, const Level& l) {
    return spade_w4_wanted(d, b, l) || (d->has16() && d->wino && d->spw && wino16_supported(2 * b.n_in, 128, 1, l.H, l.W, 1));
}

// Brackets one 3x3x3 conv launch with HIP events on the launch stream WITHOUT synchronising; the pairs are
// resolved later by i2v_dec_get_profile (after the caller has synchronised the stream).
namespace {
struct ProfScope {
    BlockCtx* d;
    hipStream_t st;
    hipEvent_t e0 = nullptr;
    double flops, exec_flops;
    ProfScope(BlockCtx* d_, hipStream_t st_, double flops_, double exec_) : d(d_), st(st_), flops(flops_), exec_flops(exec_) {
        if (d->profile) { (void)hipEventCreate(&e0); (void)hipEventRecord(e0, st); }
    }
    ~ProfScope() {
        if (d->profile) {
            hipEvent_t e1 = nullptr;
            (void)hipEventCreate(&e1);
            (void)hipEventRecord(e1, st);
            d->prof_events.push_back({e0, e1, flops, exec_flops, d->prof_cur_layer});
            if (d->prof_cur_layer >= 0 && d->prof_cur_layer < 12) d->prof_layers[d->prof_cur_layer].kernel = d->prof_cur_kernel;
        }
    }
};
}  // namespace

// SPADE's conditioning branch of one block (normalization_layer.py:20-23): resize(start frame) -> Conv2d(3, 128) + lrelu ->
// fused gamma | beta Conv2d(128, 2C) ("+1" folded into the gamma bias) -> gb [B][H][W][2C].  Depends on the start frame only.
int spade_branch(BlockCtx* d, Block& b, const Level& l, const float* img, int img_h, int img_w, long ibs, int B, float* y0, float* y1,
                 float* y1v, float* gb, hipStream_t st, int k) {
    int rc;
    // debug taps 13 .. 15 of block k (k < 0: a stand-alone block, no taps): the branch's intermediates in the form they are stored in
    auto tap = [&](int which, const void* src, size_t count) -> int {
        if (k >= 0 && d->tap_dst && d->tap_block == k && d->tap_which == which)
            I2V_HIP_CHECK(hipMemcpyAsync(d->tap_dst, src, std::min(count, d->tap_max) * 4, hipMemcpyDeviceToDevice, st));
        return I2V_OK;
    };
    const size_t HW = (size_t)B * l.H * l.W;
    if ((rc = resize_forward(img, y0, B, img_h, img_w, l.H, l.W, st, d->aux16() ? 1 : 0, d->status_dev, ibs))) return rc;
    if ((rc = tap(13, y0, HW * 16))) return rc;
    if (d->aux16() && b.sp_gb_w4.w.p && y1v) {
        b.spade_form = SPADE_F43;
        if ((rc = conv16_forward(b.sp_conv16, y0, y1, nullptr, 1, 1, B, 1, l.H, l.W, EPI_LRELU, st))) return rc;
        if ((rc = tap(14, y1, HW * 128))) return rc;
        if ((rc = run_modulate_wino4(y1, nullptr, nullptr, y1v, B, 1, l.H, l.W, 128, 1, 1, 0, st, false, d->status_dev))) return rc;
        if ((rc = tap(15, y1v, HW * 128 * 3 / 2))) return rc;
        if ((rc = wino4_forward(b.sp_gb_w4, y1v, gb, nullptr, 1, 1, B, 1, l.H, l.W, EPI_NONE, st, nullptr))) return rc;
    } else if (d->aux16() && b.sp_gb_w.w.p && y1v) {
        // gamma | beta conv on the Winograd kernel: the 128-channel activation goes through fp32 once more (the operand
        // writer needs the w-neighbours of every position, which the producing conv's epilogue does not hold)
        b.spade_form = SPADE_F23;
        if ((rc = conv16_forward(b.sp_conv16, y0, y1, nullptr, 1, 1, B, 1, l.H, l.W, EPI_LRELU, st))) return rc;
        if ((rc = tap(14, y1, HW * 128))) return rc;
        if ((rc = run_modulate_wino(y1, nullptr, nullptr, y1v, B, 1, l.H, l.W, 128, 1, 1, 0, st, d->status_dev))) return rc;
        if ((rc = tap(15, y1v, HW * 128 * 2))) return rc;
        if ((rc = wino16_forward(b.sp_gb_w, y1v, gb, nullptr, 1, 1, B, 1, l.H, l.W, EPI_NONE, st, nullptr))) return rc;
    } else if (d->aux16()) {
        b.spade_form = SPADE_DIRECT16;
        if ((rc = conv16_forward(b.sp_conv16, y0, y1, nullptr, 1, 1, B, 1, l.H, l.W, EPI_LRELU | EPI_HL16, st, nullptr, d->status_dev)))
            return rc;
        if ((rc = tap(14, y1, HW * 128))) return rc;
        if ((rc = conv16_forward(b.sp_gb16, y1, gb, nullptr, 1, 1, B, 1, l.H, l.W, EPI_NONE, st))) return rc;
    } else {
        b.spade_form = SPADE_F32;
        if ((rc = conv_forward(b.sp_conv, y0, 16, y1, nullptr, 1, 1, B, 1, l.H, l.W, EPI_LRELU, st))) return rc;
        if ((rc = tap(14, y1, HW * 128))) return rc;
        if ((rc = conv_forward(b.sp_gb, y1, 128, gb, nullptr, 1, 1, B, 1, l.H, l.W, EPI_NONE, st))) return rc;
    }
    return I2V_OK;
}

// What a block conv is applied to: lrelu((x A + B) gamma' + beta) read through the nearest up-sampling map (ut, us).  x = the fp32 tensor
// before the modulation, coef = the per-(b, c) (A, B) pairs, gb = SPADE's maps (conv_0) or null (conv_1, behind ADAIN).
struct Conv3In { const float* x; const float* coef; const float* gb; int ut, us; GbRows rows; };

// The kernel conv `layer` (= 2 * block + (0: conv_0, 1: conv_1)) runs in THIS call: wanted by shape, packed, and the layer on the
// split-fp16 path (mma = 0: none is; mma = auto: not the layers the range guard switched, BlockCtx::fp32_layer).  m6: the exact-fp32
// Winograd scratch (null: the direct fp32 kernel is used).
static Conv3Kernel conv3_choose(const BlockCtx* d, const Conv3& c, const Level& l, int layer, const Conv3In& in, const float* m6) {
    if (!d->layer16(layer)) return m6 && c.wf.u[0].w.p && conv3_wants(d, c, l, K_F32_WINO) ? K_F32_WINO : K_F32;
    if (c.w43.w.p && conv3_wants(d, c, l, K_F43)) {
        if (c.w43.one) return K_F43_ONE;
        // thin F(4,3) layers: the operand is generated by the conv kernel's producer waves (no writer launch, no V tensor).
        // I2V_DEC_GEN = 1: conv_0 and conv_1 of the thin level, 2: conv_1 only.  conv_0 reads SPADE's maps through a x2 spatial
        // up-sampling, conv_1 (ADAIN) through none; neither through a temporal one, and the debug tap wants the V tensor.
        const bool first = !(layer & 1);
        const bool gen = (first ? d->gen == 1 : d->gen != 0) && !c.tdup && in.ut == 1 && in.us == (first ? 2 : 1) && !d->tap_dst &&
                         wino4g_supported(c.cout, c.cin, l.T, l.H, l.W, in.us);
        return gen ? K_F43_GEN : K_F43;
    }
    if (c.w23.w.p && conv3_wants(d, c, l, K_F23)) return K_F23;
    return K_F16;
}

// Launches the operand writer kernel `kn` reads (K_F43_GEN: none) into `a`; *tap_floats = what it wrote, for the debug tap (0: nothing to
// tap).  A tdup conv's operand is kept at the half temporal rate (its frames 2i and 2i+1 coincide) -- while the layer is on the
// split-fp16 path: a layer that `auto` switched to fp32 reads through the real ut.
// Range guard: the operand tensor of layer i publishes its maximum in slot 1 + i.
static int conv3_write_operand(BlockCtx* d, const Conv3& c, Conv3Kernel kn, const Level& l, int layer, const Conv3In& in, float* a, int B,
                        hipStream_t st, size_t* tap_floats) {
    const bool tdup = c.tdup && is_split(kn);
    const int T = tdup ? l.T / 2 : l.T, ut = tdup ? 1 : in.ut;
    int* flag = d->status_dev;
    int* umax = is_split(kn) && flag ? flag + 1 + layer : nullptr;
    const size_t pos = (size_t)B * T * l.H * l.W;
    // the whole operand, in floats: 4 bytes per activation in the direct formats (fp32, or fp16 hi | lo), 4 planes per 2 positions in
    // F(2,3)'s V, 6 per 4 in F(4,3)'s (split and exact fp32), 6 per 4 of 2 bytes over CinPad channels in the one-term V
    *tap_floats = kn == K_F43_GEN ? 0 : kn == K_F43_ONE ? pos * c.w43.CinPad * 3 / 4 : kn == K_F23 ? pos * c.cin * 2 :
                  kn == K_F43 || kn == K_F32_WINO ? pos * c.cin * 3 / 2 : pos * c.cin;
    switch (kn) {
    case K_F43_GEN: return I2V_OK;
    case K_F32_WINO: return modulate_wino4_f32(in.x, in.coef, in.gb, a, B, T, l.H, l.W, c.cin, ut, in.us, 1, st, in.rows);
    case K_F43_ONE:
    case K_F43: return run_modulate_wino4(in.x, in.coef, in.gb, a, B, T, l.H, l.W, c.cin, ut, in.us, 1, st, kn == K_F43_ONE, flag, umax, in.rows);
    case K_F23: return run_modulate_wino(in.x, in.coef, in.gb, a, B, T, l.H, l.W, c.cin, ut, in.us, 1, st, flag, umax, in.rows);
    default: return run_modulate(in.x, in.coef, in.gb, a, B, T, l.H, l.W, c.cin, ut, in.us, 1, st, kn == K_F16, flag, umax, in.rows);
    }
}

// Runs the conv on kernel `kn`: a = the operand conv3_write_operand wrote (K_F43_GEN: generated in the kernel from `in`, with the
// writer's range guard); stats = where the epilogue accumulates the output's statistics (null: not fused; never on the fp32 kernels).
static int conv3_run(BlockCtx* d, const Conv3& c, Conv3Kernel kn, const Level& l, int layer, const Conv3In& in, const float* a, float* out,
              const float* res, int rt, int rs, int B, int epi, double* stats, const BlockBufs& w, hipStream_t st) {
    if (stats) I2V_HIP_CHECK(hipMemsetAsync(stats, 0, (size_t)B * c.cout * 16, st));
    // algorithmic FLOPs of the reference's 3x3x3 conv, and the matrix-core FLOPs actually issued: 3 fp16 MFMAs per product on the
    // split-fp16 kernels, one on the one-term kernel; F(2,3): 4 Winograd products per 2 outputs x 3 kw taps (x 2/3), F(4,3): 6 per
    // 4 outputs (x 1/2); 18 instead of 27 taps in temporal-duplication mode (the generating kernel never is)
    const double fl = 2.0 * B * l.T * l.H * l.W * (double)c.cin * c.cout * 27.0, td = c.tdup ? 18.0 / 27.0 : 1.0;
    // (the split and one-term F(4,3) kernels: minus the units its edge form skips -- temporal taps that read only zero padding)
    const double exec = kn == K_F32 ? fl : kn == K_F32_WINO ? 0.5 * fl : kn == K_F16 ? 3.0 * fl * td : kn == K_F23 ? 3.0 * fl * (2.0 / 3.0) * td :
                        kn == K_F43 ? 3.0 * fl * 0.5 * td * (d->profile ? wino4_issued_share(c.w43, B, l.T, l.H, l.W) : 1.0) :
                        kn == K_F43_ONE ? fl * 0.5 * td * (d->profile ? wino4_issued_share(c.w43, B, l.T, l.H, l.W) : 1.0) : 3.0 * fl * 0.5;
    d->prof_cur_layer = layer;
    d->prof_cur_kernel = kn;
    ProfScope ps(d, st, fl, exec);
    int* flag = d->status_dev;
    switch (kn) {
    case K_F32: return conv_forward(c.f32, a, c.cin, out, res, rt, rs, B, l.T, l.H, l.W, epi, st);
    case K_F32_WINO: return wino4f32_forward(c.wf, a, w.m6, out, res, rt, rs, B, l.T, l.H, l.W, epi, st);
    case K_F16: return conv16_forward(c.d16, a, out, res, rt, rs, B, l.T, l.H, l.W, epi, st, stats, nullptr, w.splitk, w.splitk_floats);
    case K_F23: return wino16_forward(c.w23, a, out, res, rt, rs, B, l.T, l.H, l.W, epi, st, stats);
    case K_F43:
    case K_F43_ONE: return wino4_forward(c.w43, a, out, res, rt, rs, B, l.T, l.H, l.W, epi, st, stats);
    case K_F43_GEN: return wino4g_forward(c.w43, in.x, in.coef, in.gb, in.us, out, res, rt, rs, B, l.T, l.H, l.W, epi, st, stats, flag,
                                          flag ? flag + 1 + layer : nullptr, in.rows);
    }
    return I2V_E_INVALID;
}

// One GeneratorBlock (decoder.py:33-52) on channels-last tensors: x [B][T/ut][H/us][W/us][n_in] -> xn [B][T][H][W][n_out].
// `last`: the block output only feeds conv_img(leaky_relu(.)) (decoder.py:117), so the activation is fused here.
int block_forward(BlockCtx* d, int k, Block& b, const Level& l, const float* x, float* xn, const float* img, int img_h, int img_w, long ibs,
                  const float* zl, int zstride, int B, const BlockBufs& w, bool& x_stats_ready, bool last, hipStream_t st) {
    float *a = w.a, *dx = w.dx, *xs_in = w.xs_in, *xs_low = w.xs_low, *y0 = w.y0, *y1 = w.y1, *gb = w.gb, *coef = w.coef;
    double *sums1 = w.sums1, *sums2 = w.sums2;
    double* sums_out = w.sums_out ? w.sums_out : w.sums1;
    int rc;
    // (count in floats; an fp64 pair table is copied as bytes: 4 floats per pair.  The copy is enqueued where the data is complete
    //  and before the next launch that rewrites the buffer: coef is rewritten three times per block, sums1 by conv_1)
    auto tap = [&](int k_, int which, const void* src, size_t count, hipStream_t ts) -> int {
        if (d->tap_dst && d->tap_block == k_ && d->tap_which == which)
            I2V_HIP_CHECK(hipMemcpyAsync(d->tap_dst, src, std::min(count, d->tap_max) * 4, hipMemcpyDeviceToDevice, ts));
        return I2V_OK;
    };
    const int Tl = l.T / l.ut, Hl = l.H / l.us, Wl = l.W / l.us;
    const long Pl = (long)Tl * Hl * Wl, P = (long)l.T * l.H * l.W;
    // GroupNorm statistics of the (virtually upsampled) block input == statistics of the low-res tensor; they are
    // already in sums1 when the previous block's conv_1 accumulated them in its epilogue
    if (!x_stats_ready && (rc = stats_forward(x, sums1, B, Pl, b.n_in, st))) return rc;
    if ((rc = tap(k, 12, x, (size_t)B * Pl * b.n_in, st)) || (rc = tap(k, 8, sums1, (size_t)B * b.n_in * 4, st))) return rc;
    if ((rc = coef_forward(sums1, coef, B, b.n_in, b.groups_spade, (double)Pl, st))) return rc;
    if ((rc = tap(k, 9, coef, (size_t)B * b.n_in * 2, st))) return rc;
    // The learned shortcut depends on the block input and its statistics only: on the side stream it runs underneath the
    // modulate / conv_0 / modulate chain below (an HBM-bound GEMM next to matrix-core-bound convs); conv_1 waits for it.
    const bool side_shortcut = b.learned && w.side && w.coef_s;
    if (side_shortcut) {
        I2V_HIP_CHECK(hipEventRecord(w.ev_x, st));
        I2V_HIP_CHECK(hipStreamWaitEvent(w.side, w.ev_x, 0));
        int rs_ = coef_forward(sums1, w.coef_s, B, b.n_in, 16, (double)Pl, w.side, b.gn_w.as<float>(), b.gn_b.as<float>());
        if (!rs_) rs_ = tap(k, 11, w.coef_s, (size_t)B * b.n_in * 2, w.side);
        if (!rs_) {
            if (d->aux16() && b.convs16.w.p) rs_ = pointwise16_forward(b.convs16, x, xs_low, nullptr, (long)B * Pl, Pl, EPI_NONE, w.side, w.coef_s, d->status_dev);
            else rs_ = conv_forward(b.convs, x, b.n_in, xs_low, nullptr, 1, 1, B, Tl, Hl, Wl, EPI_NONE, w.side, w.coef_s);
        }
        if (!rs_ && hipEventRecord(w.ev_s, w.side) != hipSuccess) rs_ = I2V_E_HIP;
        if (rs_) { (void)hipStreamSynchronize(w.side); return rs_; }
    }
    // SPADE branch (normalization_layer.py:20-23): depends on the start frame only -- either computed here, or already there
    // (w.gb_ready: i2v_dec_prepare ran it, typically on a side stream underneath the cINN pass)
    // (realizations: the B samples of this launch span Bg start frames -- the branch runs once per frame)
    const GbRows rows = w.rows;
    const int Bg = rows.shared() ? (rows.r0 + B - 1) / rows.k + 1 : B;
    if (w.gb_ready) gb = const_cast<float*>(w.gb_ready);
    else if ((rc = spade_branch(d, b, l, img, img_h, img_w, ibs, Bg, y0, y1, w.y1v, gb, st, k))) return rc;
    if ((rc = tap(k, 0, gb, (size_t)Bg * l.H * l.W * 2 * b.n_in, st))) return rc;
    // per conv: the kernel it runs in this call, its operand writer, the conv
    const Conv3 &c0 = b.conv[0], &c1 = b.conv[1];
    const Conv3In in0{x, coef, gb, l.ut, l.us, rows}, in1{dx, coef, nullptr, 1, 1, {}};
    const Conv3Kernel k0 = conv3_choose(d, c0, l, 2 * k, in0, w.m6), k1 = conv3_choose(d, c1, l, 2 * k + 1, in1, w.m6);
    size_t tap_floats = 0;
    if ((rc = conv3_write_operand(d, c0, k0, l, 2 * k, in0, a, B, st, &tap_floats))) return rc;
    if (tap_floats && (rc = tap(k, 1, a, tap_floats, st))) return rc;
    // (statistics fused into the epilogue: split-fp16 kernels only; a tdup conv_0 is launched on the half-rate geometry)
    const bool fuse = is_split(k0) && conv16_can_fuse_stats(c0.tdup ? l.T / 2 : l.T, l.H, l.W);
    if ((rc = conv3_run(d, c0, k0, l, 2 * k, in0, a, dx, nullptr, 1, 1, B, EPI_NONE, fuse ? sums2 : nullptr, w, st))) return rc;
    if ((rc = tap(k, 2, dx, (size_t)B * P * b.n_mid, st))) return rc;
    // ADAIN (normalization_layer.py:47-51) + leaky_relu
    if (!fuse && (rc = stats_forward(dx, sums2, B, P, b.n_mid, st))) return rc;
    if ((rc = tap(k, 6, sums2, (size_t)B * b.n_mid * 4, st))) return rc;
    if ((rc = coef_forward(sums2, coef, B, b.n_mid, b.n_mid, (double)P, st, nullptr, nullptr, zl, zstride, b.zoff))) return rc;
    if ((rc = tap(k, 10, coef, (size_t)B * b.n_mid * 2, st))) return rc;
    if ((rc = conv3_write_operand(d, c1, k1, l, 2 * k + 1, in1, a, B, st, &tap_floats))) return rc;
    if (tap_floats && (rc = tap(k, 3, a, tap_floats, st))) return rc;
    // shortcut (decoder.py:44-49) at low resolution
    const float* res = x;
    if (b.learned && !side_shortcut) {
        if ((rc = coef_forward(sums1, coef, B, b.n_in, 16, (double)Pl, st, b.gn_w.as<float>(), b.gn_b.as<float>()))) return rc;
        if ((rc = tap(k, 11, coef, (size_t)B * b.n_in * 2, st))) return rc;
        // Norm3D folded into the 1x1x1 conv's loads (no padding taps -> exact): no normalised copy of x is written
        (void)xs_in;
        if (d->aux16() && b.convs16.w.p) rc = pointwise16_forward(b.convs16, x, xs_low, nullptr, (long)B * Pl, Pl, EPI_NONE, st, coef, d->status_dev);
        else rc = conv_forward(b.convs, x, b.n_in, xs_low, nullptr, 1, 1, B, Tl, Hl, Wl, EPI_NONE, st, coef);
        if (rc) return rc;
        res = xs_low;
        if ((rc = tap(k, 4, xs_low, (size_t)B * Pl * b.n_out, st))) return rc;
    } else if (b.learned) {
        res = xs_low;
        I2V_HIP_CHECK(hipStreamWaitEvent(st, w.ev_s, 0));   // enqueued on the side stream at the top of the block
    }
    // g_4's output only feeds conv_img(leaky_relu(x)) (decoder.py:117): fuse the activation here
    // (the shortcut's coefficients were derived from sums1 above, so conv_1 may now overwrite sums1 with the
    // statistics of the block OUTPUT = the next block's input)
    const bool fuse_out = is_split(k1) && conv16_can_fuse_stats(l.T, l.H, l.W) && !last;
    if ((rc = conv3_run(d, c1, k1, l, 2 * k + 1, in1, a, xn, res, l.ut, l.us, B, last ? EPI_LRELU : EPI_NONE, fuse_out ? sums_out : nullptr, w, st)))
        return rc;
    x_stats_ready = fuse_out;
    if (fuse_out && (rc = tap(k, 7, sums_out, (size_t)B * b.n_out * 4, st))) return rc;
    if ((rc = tap(k, 5, xn, (size_t)B * P * b.n_out, st))) return rc;
    return I2V_OK;
}

// sigma = u . (W_mat v), W_mat = weight_orig.reshape(Cout, -1); signed, no abs (torch spectral_norm, eval mode)
static int sn_scale(const StateDict& sd, const std::string& name, bool spectral, int cout, int64_t kk, const float** w_out,
             double* scale_out) {
    if (!spectral) {
        *w_out = sd.f32(name + ".weight", (int64_t)cout * kk);
        *scale_out = 1.0;
        return *w_out ? I2V_OK : I2V_E_MISSING;
    }
    const float* w = sd.f32(name + ".weight_orig", (int64_t)cout * kk);
    const float* u = sd.f32(name + ".weight_u", cout);
    const float* v = sd.f32(name + ".weight_v", kk);
    if (!w || !u || !v) return I2V_E_MISSING;
    double sigma = 0.0;
    for (int n = 0; n < cout; ++n) {
        double r = 0.0;
        const float* row = w + (size_t)n * kk;
        for (int64_t j = 0; j < kk; ++j) r += (double)row[j] * v[j];
        sigma += r * u[n];
    }
    I2V_REQUIRE(sigma != 0.0 && std::isfinite(sigma), I2V_E_INVALID, "spectral norm sigma of %s is %g", name.c_str(), sigma);
    *w_out = w;
    *scale_out = 1.0 / sigma;
    return I2V_OK;
}

template <class WT>
int sn_pack(const StateDict& sd, const std::string& name, bool spectral, int cout, int cin, int k, bool has_bias,
            WT& out) {
    const float* bias = nullptr;
    if (has_bias) { bias = sd.f32(name + ".bias", cout); if (!bias) return I2V_E_MISSING; }
    const float* w = nullptr;
    double scale = 1.0;
    int rc = sn_scale(sd, name, spectral, cout, (int64_t)cin * k * k * k, &w, &scale);
    if (rc) return rc;
    return out.pack(w, bias, cout, cin, k, k, k, scale);
}
template int sn_pack(const StateDict&, const std::string&, bool, int, int, int, bool, ConvWeights&);
template int sn_pack(const StateDict&, const std::string&, bool, int, int, int, bool, Conv16Weights&);

// Packs the kernel variants `variants` (bits of Conv3Kernel; K_F43_GEN reads K_F43's weights) of one block conv from the state dict
int pack_conv3(const StateDict& sd, const std::string& name, bool spectral, Conv3& c, unsigned variants) {
    const float* bias = sd.f32(name + ".bias", c.cout);
    if (!bias) return I2V_E_MISSING;
    const float* w = nullptr;
    double scale = 1.0;
    int rc = sn_scale(sd, name, spectral, c.cout, (int64_t)c.cin * 27, &w, &scale);
    if (rc) return rc;
    const int co = c.cout, ci = c.cin;
    if ((variants & bit(K_F32)) && (rc = c.f32.pack(w, bias, co, ci, 3, 3, 3, scale))) return rc;
    if ((variants & bit(K_F32_WINO)) && (rc = c.wf.pack(w, bias, co, ci, scale))) return rc;
    // (tdup: packed for the half-rate input, Conv16Weights::pack_tdup)
    if ((variants & bit(K_F16)) && (rc = c.tdup ? c.d16.pack_tdup(w, bias, co, ci, scale) : c.d16.pack(w, bias, co, ci, 3, 3, 3, scale))) return rc;
    if ((variants & bit(K_F23)) && (rc = c.tdup ? c.w23.pack_tdup(w, bias, co, ci, scale) : c.w23.pack(w, bias, co, ci, 3, scale))) return rc;
    const bool one = variants & bit(K_F43_ONE);   // (packed instead of K_F43, never next to it)
    if ((variants & (bit(K_F43) | bit(K_F43_ONE))) && (rc = c.tdup ? c.w43.pack_tdup(w, bias, co, ci, scale, one) : c.w43.pack(w, bias, co, ci, scale, 3, one))) return rc;
    return I2V_OK;
}

// Spade (keys p + "norm_0.*"): Conv2d(3,128,3) then conv_gamma | conv_beta fused as one Conv2d(128, 2C, 3), the latter packed for the
// kernels the caller names: gb16 / gb32 the direct split-fp16 / fp32 ones, gb_w4 -- else gb_w -- the F(4,3) / F(2,3) Winograd ones
int pack_spade(const StateDict& sd, const std::string& p, Block& b, bool gb16, bool gb32, bool gb_w4, bool gb_w) {
    int rc;
    const float* w1 = sd.f32(p + "norm_0.conv.weight", 128 * 3 * 9);
    const float* b1 = sd.f32(p + "norm_0.conv.bias", 128);
    const float* wg = sd.f32(p + "norm_0.conv_gamma.weight", (int64_t)b.n_in * 128 * 9);
    const float* bg = sd.f32(p + "norm_0.conv_gamma.bias", b.n_in);
    const float* wb = sd.f32(p + "norm_0.conv_beta.weight", (int64_t)b.n_in * 128 * 9);
    const float* bb = sd.f32(p + "norm_0.conv_beta.bias", b.n_in);
    if (!w1 || !b1 || !wg || !bg || !wb || !bb) return I2V_E_MISSING;
    if ((rc = b.sp_conv.pack(w1, b1, 128, 3, 1, 3, 3, 1.0))) return rc;
    {   // the same conv for the split-fp16 path: input channels padded 3 -> 16 (the resize kernel's row)
        std::vector<float> w16((size_t)128 * 16 * 9, 0.f);
        for (int n = 0; n < 128; ++n)
            for (int c = 0; c < 3; ++c)
                for (int t = 0; t < 9; ++t) w16[((size_t)n * 16 + c) * 9 + t] = w1[((size_t)n * 3 + c) * 9 + t];
        if ((rc = b.sp_conv16.pack(w16.data(), b1, 128, 16, 1, 3, 3, 1.0))) return rc;
    }
    std::vector<float> wgb((size_t)2 * b.n_in * 128 * 9), bgb((size_t)2 * b.n_in);
    std::memcpy(wgb.data(), wg, (size_t)b.n_in * 128 * 9 * 4);
    std::memcpy(wgb.data() + (size_t)b.n_in * 128 * 9, wb, (size_t)b.n_in * 128 * 9 * 4);
    for (int c = 0; c < b.n_in; ++c) { bgb[c] = bg[c] + 1.0f; bgb[b.n_in + c] = bb[c]; }  // normalized*(1+gamma)+beta
    if (gb16 && (rc = b.sp_gb16.pack(wgb.data(), bgb.data(), 2 * b.n_in, 128, 1, 3, 3, 1.0))) return rc;
    if (gb32 && (rc = b.sp_gb.pack(wgb.data(), bgb.data(), 2 * b.n_in, 128, 1, 3, 3, 1.0))) return rc;
    if (gb_w4) return b.sp_gb_w4.pack(wgb.data(), bgb.data(), 2 * b.n_in, 128, 1.0, 1);
    if (gb_w) return b.sp_gb_w.pack(wgb.data(), bgb.data(), 2 * b.n_in, 128, 1, 1.0);
    return I2V_OK;
}

// The environment switches of a handle.  A stand-alone block (i2v_gblock; whole = false) reads the three that choose among its conv
// kernels and keeps the defaults of the rest.
void read_switches(BlockCtx* d, bool whole) {
    if (const char* e = std::getenv("I2V_DEC_WINO")) d->wino = std::atoi(e) != 0;
    if (const char* e = std::getenv("I2V_DEC_WINO4")) d->wino4 = std::atoi(e);
    if (const char* e = std::getenv("I2V_DEC_PW16")) d->pw16 = std::atoi(e) != 0;
    if (!whole) return;
    if (const char* e = std::getenv("I2V_DEC_IMG16")) d->img16 = std::atoi(e);
    if (const char* e = std::getenv("I2V_DEC_SPW")) d->spw = std::atoi(e) != 0;
    if (const char* e = std::getenv("I2V_DEC_WINO32")) d->wino32 = std::atoi(e) != 0;
    if (const char* e = std::getenv("I2V_DEC_GEN")) d->gen = std::atoi(e);   // 1: conv_0 and conv_1 of the thin level, 2: conv_1 only
    if (const char* e = std::getenv("I2V_DEC_OVERLAP")) { d->overlap = std::atoi(e) != 0; d->no_side_shortcut = std::atoi(e) == 2; }
    if (const char* e = std::getenv("I2V_DEC_SUB")) d->sub = std::max(0, std::atoi(e));
}

// the channel counts of a block's two convs; tdup: the block sits behind a x2 temporal up-sampling (Conv3::tdup)
void init_convs(Block& b, bool tdup) {
    b.conv[0].cin = b.n_in; b.conv[0].cout = b.conv[1].cin = b.n_mid; b.conv[1].cout = b.n_out;
    b.conv[0].tdup = tdup;
}

// the sticky range flag (device word and pinned host mirror); create_handle has bound the device
int init_status(BlockCtx* d) {
    { const char* zp = nullptr; if (int rcz = zero_page(&zp)) return rcz; }  // the conv kernels' zero page: allocated here, not inside a forward
    I2V_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d->status_dev), I2V_STATUS_WORDS * sizeof(int)));   // [0] flags, [1..] underflow maxima
    I2V_HIP_CHECK(hipMemset(d->status_dev, 0, I2V_STATUS_WORDS * sizeof(int)));
    I2V_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&d->status_host), I2V_STATUS_WORDS * sizeof(int), hipHostMallocDefault));   // [0] flags, [32 + i] the last forward's maxima
    std::memset(d->status_host, 0, I2V_STATUS_WORDS * sizeof(int));
    return I2V_OK;
}

// behind Entry::check in every call that enqueues work (check_entry): no overflow reported by an earlier call
int check_range(const BlockCtx* d, const char* what) {
    I2V_REQUIRE(!(*static_cast<volatile const int*>(d->status_host) & 1), I2V_E_RANGE,
                "%s: an earlier call on this handle produced activations outside the fp16 range of the split-fp16 operand "
                "format (|x| > 65504 or non-finite); its output is invalid.  Use the exact-fp32 mode (mma = 0 / I2V_DEC_MMA=0) "
                "for this checkpoint, or clear the flag with i2v_dec_status(reset = 1)", what);
    return I2V_OK;
}

int BlockCtx::status(int32_t* flags, int32_t reset, hipStream_t st, const char* what) {
    I2V_REQUIRE_DEVICE(device, what);
    I2V_HIP_CHECK(hipMemcpyAsync(status_host, status_dev, sizeof(int), hipMemcpyDeviceToHost, st));
    I2V_HIP_CHECK(hipStreamSynchronize(st));
    *flags = *status_host;
    if (reset) {
        I2V_HIP_CHECK(hipMemsetAsync(status_dev, 0, sizeof(int), st));
        I2V_HIP_CHECK(hipStreamSynchronize(st));
        *status_host = 0;
    }
    return I2V_OK;
}

}  // namespace i2v
