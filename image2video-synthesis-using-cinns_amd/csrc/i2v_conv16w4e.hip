// The split-fp16 Winograd F(4,3) 3x3x3 / 2x3x3 kernel (i2v_conv16w4.hip) that does not multiply the clip's temporal zero padding.
//
// Every 3x3x3 conv pads one frame at each end of the clip, and the decoder's clips are short (2 .. 16 frames per launch).  With the
// 512-thread brick (TT x TH x 16 positions, TH * 4 >= 32) a 32-tile MFMA row block lies inside ONE frame, so in a brick at the clip's
// edge the three (kt, kh) taps of the outermost kt feed that frame's row blocks from the zero page: all 3 x 3 MFMAs per chunk of such a
// (kt, row block) "unit" add +0 to the accumulators.  w4_unit_dead (i2v_conv16w4_dev.h) is the rule; w4_pass<..., DEAD> leaves the dead
// units' MFMAs and operand reads out at COMPILE time, so every tap loop stays one basic block with the loads, waits and barriers of
// the full loop.  Same kernel template (i2v_conv16w4_kernel.h, W4K_EDGE): a brick's waves pick, once per pass and wave-uniformly, the
// loop compiled for their own row blocks' mask --
//     front  kt = 0 on the row blocks of the brick's first frame       (t0 = 0; pair kernels: the even output frames' parity only)
//     back   kt = KT - 1 on the row blocks of its last frame           (t0 + TT = T; pair kernels: the odd parity only)
//     both   one brick holds the whole clip (T == TT, 3x3x3 only; pass A of the 64-channel kernel, whose waves hold all four row blocks)
// and the full loop everywhere else.  ETT (template parameter) = the brick's frame count the masks are derived for: 4 (TH = 8: a row
// block is a frame) or 2 (TH = 16: two row blocks per frame; pair kernels only -- the two-frame input of g_1.conv_0).  The products left out are exact zeros (zero-page
// rows x finite weights) and the order of the remaining accumulation is untouched: the outputs are bit-identical to
// conv_wino4_f16x3_kernel's, which stays the kernel of every other case and, in the measurement build, the A/B reference
// (I2V_W4_TSKIP=0).  The one-term fp16 form (conv_wino4e_f16_kernel, mma = "fp16") comes through W4K_ONE with the same masks: it leaves
// out two MFMAs per product of a dead unit instead of three, and the layer profile's issued-MFMA count of both forms shrinks alike.
// Share of the tap loops' MFMAs not issued (w4_dead_units): T = 2 pairs 25 %, T = 4 16.7 % (3x3x3) / 12.5 % (pairs), T = 8 8.3 % / 6.25 %,
// T = 16 4.2 % / 3.1 %.
// Instrumented builds (-DW4_TIMELINE / -DW4_TAPTIME, tools/conv16w_check): their device-side buffers live in i2v_conv16w4.hip, which
// then includes this file (W4E_IN_MAIN) instead of linking it.
#if defined(W4E_IN_MAIN) || !(defined(W4_TIMELINE) || defined(W4_TAPTIME))
#ifndef W4E_IN_MAIN
#define W4_NO_INSTRUMENT
#endif
#include "i2v_conv16w4_dev.h"

namespace i2v {

#define W4K_NAME conv_wino4e_f16x3_kernel
#define W4K_ONE false
#define W4K_EDGE
#include "i2v_conv16w4_kernel.h"

// the one-term fp16 form (i2v_conv16w4h.hip, mma = "fp16") comes with the template: two MFMAs per product instead of three, the same units
#define W4K_NAME conv_wino4e_f16_kernel
#define W4K_ONE true
#define W4K_EDGE
#include "i2v_conv16w4_kernel.h"

template <int NT, int BN, int ETT, bool ONE>
static int launch_wino4e(const W4Plan& p, hipStream_t st) {
    auto kern = ONE ? conv_wino4e_f16_kernel<NT, BN, 512, ETT> : conv_wino4e_f16x3_kernel<NT, BN, 512, ETT>;
    static bool attr_set[I2V_MAX_DEV] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_set)) return rc;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(512), p.lds_bytes, st, p.a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

// The plan is wino4_plan's (forms W4_EDGE / W4_EDGE_ONE: 512 threads, TT = 4 / TH = 8 or TT = 2 / TH = 16).
int wino4e_launch(const W4Plan& p, hipStream_t st) {
#define W4_CASE(NT, BN, ETT)                                                                                         \
    case w4_key(NT, BN, 512) * 8 + ETT:                                                                              \
        return p.form == W4_EDGE_ONE ? launch_wino4e<NT, BN, ETT, true>(p, st) : launch_wino4e<NT, BN, ETT, false>(p, st);
    if (p.NTH == 512 && p.a.TT * p.a.TH == 32) switch (w4_key(p.NT, p.BN, 512) * 8 + p.a.TT) {
        W4_CASE(9, 64, 4) W4_CASE(6, 64, 4) W4_CASE(9, 32, 4) W4_CASE(6, 32, 4)
        W4_CASE(6, 64, 2) W4_CASE(6, 32, 2)   // (a 3x3x3 halo brick of 2 x 16 rows does not fit the V buffers: wino4_tiling)
    }
#undef W4_CASE
    set_error("wino4e: no kernel <%d taps, %d channels, %d threads, %d x %d brick>", p.NT, p.BN, p.NTH, p.a.TT, p.a.TH);
    return I2V_E_INVALID;
}

}  // namespace i2v
#endif
