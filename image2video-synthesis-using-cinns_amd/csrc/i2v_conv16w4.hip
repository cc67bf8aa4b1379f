// 3x3x3 Conv3d with a Winograd F(4,3) transform along W on the gfx950 fp16 matrix cores (split-fp16 operands).
//
// F(2,3) (i2v_conv16w.hip) multiplies 4 transformed planes per 2 outputs; F(4,3) multiplies 6 per 4: 0.75x the MFMAs and a
// V operand of 12 instead of 16 bytes per activation.  Per tile of four output positions (w = 4j .. 4j+3) and (kt, kh) tap
//     d_k = a[t+kt-1][h+kh-1][4j-1+k], k = 0..5 (zero padded)
//     V0 = 4 d0 - 5 d2 + d4        V1 = -4 d1 - 4 d2 + d3 + d4     V2 = 4 d1 - 4 d2 - d3 + d4
//     V3 = -2 d1 - d2 + 2 d3 + d4  V4 = 2 d1 - d2 - 2 d3 + d4      V5 = 4 d1 - 5 d3 + d5
//     U0 = g0/4   U1 = -(g0+g1+g2)/6   U2 = -(g0-g1+g2)/6   U3 = g0/24 + g1/12 + g2/6   U4 = g0/24 - g1/12 + g2/6   U5 = g2
//     M_x = sum over (kt, kh, c) of V_x U_x
//     y0 = M0+M1+M2+M3+M4   y1 = M1-M2+2M3-2M4   y2 = M1+M2+4M3+4M4   y3 = M1-M2+8M3-8M4+M5
// V = B^T d is written once by the producer (modulate_wino4_kernel, fp32 then split into fp16 hi / lo) as
// [B][T][C/16][6][H][W/4][16 channels = 64 B]; U = G g is computed in fp64 at load time.
//
// What shapes the kernel: 160 KB of LDS and the weight (B-operand) traffic.  A wave must multiply ONE weight fragment with
// 128 tiles (4 MFMA row blocks) -- at 64 tiles the weight stream from L2 doubles per MFMA, which is what holds the
// 32-channel variant of the F(2,3) kernel at 60 % of the 64-channel one -- and the double-buffered halo brick of SIX planes
// of 128 tiles would need 184 KB.  So the six planes are multiplied in TWO passes over the K loop with the accumulators of
// both passes kept in registers:
//   pass A  planes 0..3: exactly the loop of the F(2,3) kernel (wave = (plane, 32-channel half), 4 row blocks, 64
//           accumulator registers, nine-slot weight ring, V brick of 4 planes double-buffered by LDS-DMA);
//   pass B  planes 4, 5: wave = (plane, 32-channel half, tile half), 2 row blocks, 32 more accumulator registers, V brick of
//           2 planes (this third of the MFMAs sees the doubled weight stream);
//   epilogue: per 32-channel half the six partial GEMMs of a tile meet in LDS (98 KB), y = A^T M in fp32, then bias,
//           residual, optional lrelu, fused per-(b,c) statistics, stores of four positions per tile.
// Workgroup = 512 threads, 128 tiles = 512 output positions (TT x TH x 16 brick) x 64 output channels.
// Schedule (round 3, from per-tap and per-workgroup timing: -DW4_TAPTIME / -DW4_TIMELINE builds of tools/conv16w_check): an
// in-order wave that issues its MFMAs back to back sits blocked on the matrix pipe, and whatever it issues outside the MFMA
// block is time the pipe idles unless the partner wave of the SIMD happens to have an MFMA ready.  So everything a tap has to
// issue for the NEXT taps -- per row block the LDS address arithmetic and the two ds_read_b128 of the next tap's A operands,
// then the weight request of tap U + R - 1 (scalar base + the lane's 16 bytes: no vector address arithmetic) -- sits one small
// piece per 32-cycle gap between the tap's MFMAs; wave priority falls with the tap index inside a chunk, so that whichever of
// the two waves of a SIMD is behind gets the pipe; pass A requests pass B's first brick behind its own last chunk (no V
// round trip between the passes).  MFMA pipe busy 0.53 -> 0.62 at 1.71 -> 1.63 GHz (the chip is power-limited: DESIGN.md).
// Loads are asm statements with hand-counted waits exactly as in i2v_conv16w.hip; every pass waits for ALL of its prologue
// requests before the loop (the loop's counts assume the steady state).  tools/check_asm_waits.py replays both compiled loops
// of every instantiation, checks that each is entered with nothing in flight and that no asm load reads a freshly
// VALU-written SGPR.
// Temporal edge units: the 512-thread 3x3x3 and pair launches whose MFMA row blocks lie inside one frame (TT = 4 / TH = 8, TT = 2 /
// TH = 16 -- every such launch of the shipped configs) run conv_wino4e_f16x3_kernel (i2v_conv16w4e.hip, plan form W4_EDGE): the same
// template with the (kt, row block) units that read only the clip's temporal zero padding left out of the tap loops at compile time
// (w4_unit_dead, i2v_conv16w4_edge.h).  Same bits.  The instantiations of this file remain the kernels of every other case -- the 2-D
// convs, the 256-thread thin layers -- and, in the measurement build, the A/B and bit reference of the edge kernel (I2V_W4_TSKIP=0).
#include "i2v_conv16w4_dev.h"

namespace i2v {

// ---- host side ------------------------------------------------------------------------------------------------------

static_assert(WINO_F43.kc == W4_KC && WINO_F43_ONE.kc == 2 * W4_KC, "the packer's chunks are the kernels'");

// one: the one-term form (cin % 32 like the split form's chunk pairs -- its packer pads to 64 --, no 1x3x3 variant)
bool wino4_supported(int cout, int cin, int T, int H, int W, int KT, bool one) {
    if (cout % 32 || cin % (2 * W4_KC) || (KT != 3 && KT != 2 && (KT != 1 || one))) return false;
    int TT, TH;
    return wino4_tiling(T, H, W, KT, &TT, &TH);
}

static int wino4_store(Wino4Weights& o, const PackedHalfs& p, const float* bias_src, int cout, int cin, int kt, bool tdup, bool one) {
    o.Cin = cin; o.Cout = cout; o.KT = kt; o.tdup = tdup; o.one = one;
    o.CinPad = p.CinPad; o.CoutPad = p.CoutPad; o.nchunk = p.nchunk; o.wexp = p.wexp; o.set_bytes = p.set_bytes;
    return upload_packed(o.w, o.bias, p.halfs.data(), p.bytes(), bias_src, cout);
}

int Wino4Weights::pack(const float* w_src, const float* bias_src, int cout, int cin, double scale, int kt, bool one_) {
    I2V_REQUIRE(kt == 3 || (kt == 1 && !one_), I2V_E_INVALID, "%s: temporal kernel size %d", one_ ? "wino4h" : "wino4", kt);
    return wino4_store(*this, wino_pack(one_ ? WINO_F43_ONE : WINO_F43, w_src, cout, cin, scale, kt, false), bias_src, cout, cin, kt, false, one_);
}

int Wino4Weights::pack_tdup(const float* w_src, const float* bias_src, int cout, int cin, double scale, bool one_) {
    return wino4_store(*this, wino_pack(one_ ? WINO_F43_ONE : WINO_F43, w_src, cout, cin, scale, 3, true), bias_src, cout, cin, 2, true, one_);
}

// Measurement switches of this kernel.  The PRODUCTION library (no -DI2V_MEASURE) reads no environment variable on a launch path;
// the structure switches -- forced tile widths / workgroup sizes (I2V_W4_BN, I2V_W4_NTH), the brick -> XCD order (I2V_W4_ORDER), the
// full tap loops instead of the edge form (I2V_W4_TSKIP) and the launch trace (I2V_W4_TRACE) -- exist in the measurement build only
// (make measure -> lib/libi2v_hip_measure.so, loaded through I2V_LIB_PATH; tools/conv16w_check* are built with the flag too), where
// they are read per launch so that tests and A/B runs can flip them inside one process.  They choose among the kernels that ship.
// The one-term form has no structure switches: it always runs the defaults (but for I2V_W4_TSKIP and the trace).
static W4Switches w4_switches() {
    W4Switches w{};
#ifdef I2V_MEASURE
    if (const char* e = getenv("I2V_W4_BN")) w.bn = atoi(e);
    if (const char* e = getenv("I2V_W4_ORDER")) w.order = atoi(e);
    if (const char* e = getenv("I2V_W4_NTH")) w.nth = atoi(e);
    w.trace = getenv("I2V_W4_TRACE") != nullptr;
    if (const char* e = getenv("I2V_W4_TSKIP")) w.tskip = atoi(e);   // 0: the full tap loops on every brick (A/B and bit reference of i2v_conv16w4e.hip)
#endif
    return w;
}

// (the one-term form has no structure switches: of the measurement build's it takes the edge form's A/B switch and the launch trace only)
static W4Switches w4_plan_switches(const Wino4Weights& wts) {
    const W4Switches sw = w4_switches();
    if (!wts.one) return sw;
    W4Switches d{};
    d.tskip = sw.tskip; d.trace = sw.trace;
    return d;
}

// The launch plan of every F(4,3) kernel.  Neither the tile width, the brick shape nor the workgroup size enters the accumulation order
// of an output: the choices below change the speed, never the bits.
int wino4_plan(W4Plan* p, const Wino4Weights& wts, int B, int T, int H, int W, bool has_res, int rt, int rs, int epi, bool has_stats, int cus,
               const W4Switches& sw, bool gen) {
    const char* nm = gen ? "wino4g" : wts.one ? "wino4h" : "wino4";
    const int KT = wts.KT;
    I2V_REQUIRE((epi & ~EPI_LRELU) == 0, I2V_E_INVALID, "%s: unsupported epilogue %d", nm, epi);
    *p = W4Plan{};
    W4Args& a = p->a;
    a.B = B; a.H = H; a.W = W; a.J = W / 4; a.Cin = wts.Cin; a.Cout = wts.Cout; a.CoutPad = wts.CoutPad; a.nchunk = wts.nchunk;
    a.tdup = wts.tdup ? 1 : 0;
    a.wset_stride = wts.set_bytes;
    if (wts.tdup) {  // T is the OUTPUT frame count; the half-rate input has T / 2 frames
        I2V_REQUIRE(T % 2 == 0 && !has_res, I2V_E_INVALID, "%s: temporal-duplication mode needs an even frame count and no residual", nm);
        T /= 2;
    }
    a.T = T;
    I2V_REQUIRE(wino4_supported(wts.Cout, wts.Cin, T, H, W, KT, wts.one), I2V_E_INVALID, "%s: unsupported shape [%d,%d,%d] %d -> %d (kt = %d)", nm,
                T, H, W, wts.Cin, wts.Cout, KT);
    a.rt = has_res ? rt : 1; a.rs = has_res ? rs : 1; a.epi = epi;
    I2V_REQUIRE((a.rt == 1 || a.rt == 2 || a.rt == 4) && (a.rs == 1 || a.rs == 2 || a.rs == 4), I2V_E_INVALID,
                "%s: residual up-sampling factors %d / %d (1, 2 or 4)", nm, a.rt, a.rs);
    a.rt_shift = a.rt >> 1 == 2 ? 2 : a.rt >> 1; a.rs_shift = a.rs >> 1 == 2 ? 2 : a.rs >> 1;
    a.oscale = (float)std::ldexp(1.0, -wts.wexp);
    int TT = 1, TH = 1;
    (void)wino4_tiling(T, H, W, KT, &TT, &TH);
    int BN = a.CoutPad % 64 == 0 && !gen ? 64 : 32;  // output channels per workgroup
#ifdef W4_TAPTIME   // (the per-tap timing build carries the 512-thread kernels only)
    const bool thin_ok = false;
#else
    const bool thin_ok = !gen;
#endif
    // 64-channel workgroups that would leave CUs idle (16x16 maps at small batches) become twice as many 32-channel ones
    if (BN == 64 && KT != 1 && (long)B * (T / TT) * (H / TH) * (a.J / 4) * (a.CoutPad / 64) * (wts.tdup ? 2 : 1) < cus) BN = 32;
    if (sw.bn == 32 && KT != 1) BN = 32;
    if (sw.bn == 64 && a.CoutPad % 64 == 0 && !gen) BN = 64;
    p->form = gen ? W4_GEN : wts.one ? W4_ONE : W4_SPLIT;
    // 32-channel layers: two 256-thread workgroups of 64 tiles per CU instead of one 512-thread workgroup of 128 (W4Geo).
    // Default: only the layers that HAVE 32 output channels (g_4 of the 128 x 128 configs: +3 % on 32 -> 32, +-0 on 64 -> 32,
    // profiles/r05_c_*); 64-channel layers narrowed for a small grid keep the 512-thread geometry (-2 % at B = 8 with 256).
    // I2V_W4_NTH=256 forces the 256-thread geometry wherever the brick fits, 512 forbids it (round 4's geometry, for A/B runs).
    bool thin = false;
    if (thin_ok && (p->form == W4_SPLIT || p->form == W4_ONE) && BN == 32 && KT != 1 && sw.nth != 512 && (a.CoutPad % 64 != 0 || sw.nth == 256))
        thin = wino4_tiling(T, H, W, KT, &TT, &TH, W4Geo<256>::TILES, W4Geo<256>::ROWS_A, W4Geo<256>::ROWS_B);
    I2V_REQUIRE(BN == 64 || KT != 1, I2V_E_INVALID, "%s: the 1x3x3 variant exists for 64-channel tiles only", nm);
    a.TT = TT; a.TH = TH; a.TJ = 4; a.nbT = T / TT; a.nbH = H / TH; a.nbJ = a.J / 4;
    a.th_shift = 0;
    while ((1 << a.th_shift) < TH) ++a.th_shift;
    I2V_REQUIRE((1 << a.th_shift) == TH, I2V_E_INVALID, "%s: brick height %d is not a power of two", nm, TH);
    a.hh_magic = ((1 << 20) + TH + 1) / (TH + 2);
    I2V_REQUIRE(!has_stats || (long)TT * TH * 4 <= (long)T * H * a.J, I2V_E_INVALID, "%s: fused statistics need bricks inside one sample", nm);
    a.order = sw.order;
    const long nblk = (long)B * a.nbT * a.nbH * a.nbJ * (a.CoutPad / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 30), I2V_E_INVALID, "%s: grid of %ld workgroups", nm, nblk);
    // the kernel's index tables (gpos: V rows, tpos / tres: output and residual positions) are 32-bit
    if (!gen) {   // (the generating kernel reads no V tensor)
        I2V_REQUIRE((long)T * a.nchunk * 6 * H * a.J * 64 < (1L << 31), I2V_E_INVALID, "%s: the V operand of one sample ([%d,%d,%d] x %d chunks) exceeds the 2 GB a buffer descriptor offset can address", nm, T, H, W, a.nchunk);
        I2V_REQUIRE((long)B * T * a.nchunk * 6 * H * a.J < (1L << 31), I2V_E_INVALID,
                    "%s: batch %d too large for the 32-bit row indices of this kernel ([%d,%d,%d] x %d chunks)", nm, B, T, H, W, a.nchunk);
    }
    I2V_REQUIRE((long)B * (wts.tdup ? 2 * T : T) * H * W < (1L << 31), I2V_E_INVALID,
                "%s: batch %d too large for the 32-bit row indices of this kernel ([%d,%d,%d] x %d chunks)", nm, B, T, H, W, a.nchunk);
    a.nvirt = (int)(a.tdup ? 2 * nblk : nblk);   // workgroups = bricks x channel tiles x frame parities
    p->NT = 3 * KT; p->BN = BN; p->NTH = thin ? 256 : 512;
    p->grid = (unsigned)a.nvirt;
    a.tofs = 2 * W4_ROWS_A * 64;   // two V regions (pass B and the epilogue's exchange buffer reuse them), the index tables behind
    p->lds_bytes = (size_t)a.tofs + (size_t)W4_TABLE_BYTES;
    if (thin) {   // two workgroups per CU: 2 V regions of 576 rows + one table set = 79 616 bytes
        a.tofs = 2 * W4Geo<256>::ROWS_A * 64;
        p->lds_bytes = (size_t)a.tofs + (size_t)w4_table_bytes<256>();
    } else if (p->form == W4_GEN) {   // 12 waves; no V row tables (tpos / tres only)
        p->NTH = W4G_THREADS;
        p->lds_bytes = (size_t)a.tofs + 5 * W4Geo<512>::TILES * 4;
    }
    // Temporal edge units (i2v_conv16w4e.hip): the 512-thread kernels whose row blocks lie inside one frame
    // -- geometry only: 3-D taps, the TT = 4 / TH = 8 and TT = 2 / TH = 16 bricks its masks are compiled for (TT = 1 / TH = 32, odd clips:
    // no shipped config).  Every such launch has edge bricks (nbT x TT = T).
    p->issued = 1.0;
    if ((p->form == W4_SPLIT || p->form == W4_ONE) && sw.tskip && p->NTH == 512 && KT >= 2 && TH * 4 >= 32 && (TT == 4 || TT == 2)) {
        p->form = p->form == W4_ONE ? W4_EDGE_ONE : W4_EDGE;
        long dead, units;
        w4_dead_units(a.T, TT, a.th_shift, KT, a.tdup, &dead, &units);
        p->issued = 1.0 - (double)dead / (double)units;
    }
#ifdef W4_TAPTIME
    if (p->form == W4_SPLIT || p->form == W4_EDGE || p->form == W4_EDGE_ONE) p->lds_bytes = 160 * 1024;   // + the per-tap timing slots
#endif
    return I2V_OK;
}

// -DW4_HOST_ONLY (tests/wino_host_check.hip: the packers' bytes and the plans) and the host-side self-test below link this file
// without the other two translation units and instantiate no kernel
#if !defined(W4_HOST_ONLY) && !defined(W4_DECODE_SELFTEST)
template <int NT, int BN, int NTH>
static int launch_wino4_(const W4Plan& p, hipStream_t st) {
    auto kern = conv_wino4_f16x3_kernel<NT, BN, NTH>;
    static bool attr_set[I2V_MAX_DEV] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_set)) return rc;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(NTH), p.lds_bytes, st, p.a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

static int wino4_launch(const W4Plan& p, hipStream_t st) {
    if (p.form == W4_EDGE || p.form == W4_EDGE_ONE) return wino4e_launch(p, st);
    if (p.form == W4_ONE) return wino4h_launch(p, st);
    // (the order of the cases is the order in which the kernels are instantiated and emitted: keep it, the code object stays the same)
#define W4_CASE(NT, BN, NTH) case w4_key(NT, BN, NTH): return launch_wino4_<NT, BN, NTH>(p, st);
    switch (w4_key(p.NT, p.BN, p.NTH)) {
        W4_CASE(9, 64, 512) W4_CASE(6, 64, 512) W4_CASE(3, 64, 512)   // (3 taps: one time slice, SPADE's 2-D convs)
#ifndef W4_TAPTIME
        W4_CASE(9, 32, 256) W4_CASE(6, 32, 256)
#endif
        W4_CASE(9, 32, 512) W4_CASE(6, 32, 512)
    }
#undef W4_CASE
    set_error("wino4: no kernel <%d taps, %d channels, %d threads> in this build", p.NT, p.BN, p.NTH);
    return I2V_E_INVALID;
}

int wino4_forward(const Wino4Weights& wts, const void* v16, float* out, const float* res, int rt, int rs, int B, int T, int H,
                  int W, int epi, hipStream_t st, double* stats) {
    I2V_REQUIRE(wts.w.p, I2V_E_STATE, "%s: weights not packed", wts.one ? "wino4h" : "wino4");
    const W4Switches sw = w4_plan_switches(wts);      // (defaults unless built with -DI2V_MEASURE)
    W4Plan p;
    if (int rc = wino4_plan(&p, wts, B, T, H, W, res != nullptr, rt, rs, epi, stats != nullptr, device_cus(), sw)) return rc;
    W4Args& a = p.a;
    a.in = static_cast<const char*>(v16); a.wp = wts.w.as<char>(); a.bias = wts.bias.as<float>(); a.res = res; a.out = out;
    a.stats = stats;
    if (sw.trace) {
        fprintf(stderr, "wino4: B %d T %d H %d W %d Cin %d Cout %d pad %d KT %d tdup %d TT %d TH %d res %p rt %d rs %d stats %p epi %d nvirt %d form %d\n", B, a.T, H, W,
                a.Cin, a.Cout, a.CoutPad, wts.KT, a.tdup, a.TT, a.TH, (const void*)res, a.rt, a.rs, (void*)stats, epi, a.nvirt, (int)p.form);
        (void)hipDeviceSynchronize();
    }
    return wino4_launch(p, st);
}

// share of the full tap loops' matrix-core work a launch of this layer issues (the layer profile's issued-MFMA FLOPs): < 1 where the
// plan picks the edge form
double wino4_issued_share(const Wino4Weights& wts, int B, int T, int H, int W) {
    const W4Switches sw = w4_plan_switches(wts);
    W4Plan p;
    if (wino4_plan(&p, wts, B, T, H, W, false, 1, 1, EPI_NONE, false, device_cus(), sw)) return 1.0;
    return p.issued;
}
#endif

#if defined(W4_TIMELINE) || defined(W4_TAPTIME)   // instrumented builds: the edge kernel shares this unit's device-side buffers
}  // namespace i2v
#define W4E_IN_MAIN
#include "i2v_conv16w4e.hip"
namespace i2v {
#endif

#ifdef W4_TAPTIME
void w4_taptime_report() {
    std::vector<unsigned long long> h(2 * 8 * 18 * 2);
    (void)hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(w4_tt), h.size() * 8);
    for (int p = 0; p < 2; ++p) {
        printf("   pass %c: mean ticks (10 ns) from the start of tap slot U-1 to the start of tap slot U, per wave\n", p ? 'B' : 'A');
        for (int w = 0; w < 8; ++w) {
            printf("      wave %d:", w);
            for (int u = 0; u < 18; ++u) {
                const unsigned long long t = h[((p * 8 + w) * 18 + u) * 2], c = h[((p * 8 + w) * 18 + u) * 2 + 1];
                printf(" %5.1f", c ? (double)t / (double)c : 0.0);
            }
            printf("\n");
        }
    }
}
#endif

#ifdef W4_TIMELINE
void w4_timeline_report(unsigned nwg) {
    if (nwg > 8192) nwg = 8192;
    std::vector<unsigned long long> h(8192 * 16);
    (void)hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(w4_tl), h.size() * 8);
    const char* nm[6] = {"tables + first V brick", "pass A loop", "hand-over to pass B", "pass B loop", "epilogue half 0", "epilogue half 1"};
    double sum[6] = {}, sub[5] = {}, tot = 0;
    unsigned long long lo = ~0ull, hi = 0;
    unsigned cnt = 0;
    for (unsigned w = 0; w < nwg; ++w) {
        unsigned long long t[16];
        for (int i = 0; i < 16; ++i) t[i] = h[w * 16 + i];
        if (!t[6]) t[6] = t[5];   // 32-channel workgroups have ONE epilogue half: stamp 6 is never written (it used to wrap to 1.8e17)
        if (!t[0] || !t[7] || t[7] < t[0]) continue;   // workgroup not stamped
        ++cnt;
        for (int i = 0; i < 6; ++i) sum[i] += (double)(t[i + 1] - t[i]);
        sub[0] += (double)(t[8] - t[4]); sub[1] += (double)(t[9] - t[8]); sub[2] += (double)(t[10] - t[9]); sub[3] += (double)(t[5] - t[10]);
        tot += (double)(t[7] - t[0]);
        lo = std::min(lo, t[0]); hi = std::max(hi, t[7]);
        sub[4] += (double)(t[7] - t[6]);
    }
    if (!cnt) { printf("   F(4,3) timeline: no stamped workgroups\n"); return; }
    const unsigned nall = cnt;
    nwg = cnt;   // (means over the stamped workgroups)
    printf("   F(4,3) timeline over %u workgroups (us, 100 MHz clock): total %.2f per workgroup; kernel span %.1f = %.2f per workgroup slot of 256 CUs\n",
           nwg, tot / nwg / 100.0, (double)(hi - lo) / 100.0, (double)(hi - lo) / 100.0 / (nall / 256.0));
    for (int i = 0; i < 6; ++i) printf("      %-24s %7.2f\n", nm[i], sum[i] / nwg / 100.0);
    printf("      epilogue half 0 = residual requests + first barrier %.2f | accumulators -> LDS + barrier %.2f | transform, bias, residual, stores issued %.2f | statistics (per-wave part) %.2f; cross-wave sums + atomics of both halves %.2f\n",
           sub[0] / nwg / 100.0, sub[1] / nwg / 100.0, sub[2] / nwg / 100.0, sub[3] / nwg / 100.0, sub[4] / nwg / 100.0);
}
#endif

#ifdef W4_DECODE_SELFTEST
// Host-side self-test of the virtual-workgroup -> (brick, channel tile, frame parity) map (tests/test_host_cpu.py compiles this
// file with -DW4_DECODE_SELFTEST for the host only): for every order and a sweep of geometries the map must be a bijection onto
// {samples} x {t bricks} x {h bricks} x {w bricks} x {channel tiles} x {parities}.
template <int BN>
static long w4_decode_check(int B, int nbT, int nbH, int nbJ, int coutpad, int tdup, int order) {
    W4Args a{};
    a.B = B; a.nbT = nbT; a.nbH = nbH; a.nbJ = nbJ; a.CoutPad = coutpad; a.tdup = tdup; a.order = order; a.TT = 4; a.TH = 8;
    const int nNt = coutpad / BN, npar = tdup ? 2 : 1;
    a.nvirt = B * nbT * nbH * nbJ * nNt * npar;
    std::vector<char> seen((size_t)a.nvirt, 0);
    long bad = 0;
    for (int v = 0; v < a.nvirt; ++v) {
        const W4Brick k = w4_decode<BN>(a, v);
        const int bt = k.t0 / a.TT, bh = k.h0 / a.TH, bj = k.j0 / 4;
        if (k.par < 0 || k.par >= npar || k.ntile < 0 || k.ntile >= nNt || k.b0 < 0 || k.b0 >= B || bt < 0 || bt >= nbT || bh < 0 || bh >= nbH ||
            bj < 0 || bj >= nbJ) { ++bad; continue; }
        const size_t id = (((((size_t)k.b0 * nbT + bt) * nbH + bh) * nbJ + bj) * nNt + k.ntile) * npar + k.par;
        if (seen[id]) ++bad;
        seen[id] = 1;
    }
    return bad;
}
}  // namespace i2v
int main() {
    long bad = 0, cases = 0;
    for (int order = 0; order < 3; ++order)
        for (int B : {1, 2, 3, 8, 13, 64})
            for (int nbT : {1, 2, 4})
                for (int nbH : {1, 2, 8, 16})
                    for (int nbJ : {1, 2, 4, 8})
                        for (int tdup = 0; tdup < 2; ++tdup)
                            for (int cp : {32, 64, 128, 512}) {
                                bad += i2v::w4_decode_check<32>(B, nbT, nbH, nbJ, cp, tdup, order);
                                if (cp % 64 == 0) bad += i2v::w4_decode_check<64>(B, nbT, nbH, nbJ, cp, tdup, order);
                                ++cases;
                            }
    printf("w4_decode self-test: %ld geometries, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
#else
}  // namespace i2v
#endif