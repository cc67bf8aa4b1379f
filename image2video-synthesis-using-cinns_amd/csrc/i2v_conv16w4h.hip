// 3x3x3 Conv3d with a Winograd F(4,3) transform along W on the gfx950 fp16 matrix cores, ONE-TERM fp16 operands (mma = 3, "fp16").
//
// The split-fp16 kernel (i2v_conv16w4.hip) emulates fp32: every product is hx hw + hx lw + lx hw, three MFMAs.  This one multiplies the
// fp16 values themselves -- V rounded to fp16 by its writer (modulate_wino4h_kernel), U = G g rounded to fp16 by the packer, fp32
// accumulation -- one MFMA per product, a third of the split kernel's matrix-core work per input channel and half its V bytes.
// Layout: the 64-byte V row of the split format holds the values of 32 channels instead of hi | lo of 16,
//     V: [B][T][CinPad/32][6][H][W/4][32 channels: pieces c0-7 | c16-23 | c8-15 | c24-31]
//     U: [parity][tap][chunk of 32][6][CoutPad/32][k-step 0 = channels 0..15 | k-step 1 = channels 16..31][64 lanes][16 B]
// so that every row still feeds a lane two 16-byte A operands (now the two k-steps of the row's 32 channels) and every weight
// fragment still has two halves: the brick geometry, the LDS-DMA requests, the weight ring and its hand-counted waits are those of the
// split kernel, the tap issues 2 WM MFMAs instead of 3 WM (w4_pass<..., ONE = true>), and the chunk loop runs over half as many chunks.
// CinPad = Cin rounded up to 64 (the loop takes chunks in pairs): the 32-channel input of g_4.conv_1 at nf = 32 is padded with zero
// channels by the writer and zero weights by the packer (WINO_F43_ONE, i2v_wino_pack.h).
// The epilogue is the split kernel's: A^T M in fp32, 2^-wexp, bias, residual through the up-sampling map, optional lrelu, fused fp64
// statistics.  Same kernel template (i2v_conv16w4_kernel.h), no structure switches.
// Host side: Wino4Weights packed with one = true, wino4_forward (i2v_conv16w4.hip) plans the launch; this file exports the launch only.
#define W4_NO_INSTRUMENT
#include "i2v_conv16w4_dev.h"

namespace i2v {

#define W4K_NAME conv_wino4_f16_kernel
#define W4K_ONE true
#include "i2v_conv16w4_kernel.h"

template <int NT, int BN, int NTH>
static int launch_wino4h(const W4Plan& p, hipStream_t st) {
    auto kern = conv_wino4_f16_kernel<NT, BN, NTH>;
    static bool attr_set[I2V_MAX_DEV] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_set)) return rc;
    hipLaunchKernelGGL(kern, dim3(p.grid), dim3(NTH), p.lds_bytes, st, p.a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

// The plan is wino4_plan's (i2v_conv16w4.hip): the geometry of the split kernel, with default switches.
int wino4h_launch(const W4Plan& p, hipStream_t st) {
#define W4_CASE(NT, BN, NTH) case w4_key(NT, BN, NTH): return launch_wino4h<NT, BN, NTH>(p, st);
    switch (w4_key(p.NT, p.BN, p.NTH)) {
        W4_CASE(9, 32, 256) W4_CASE(6, 32, 256) W4_CASE(9, 64, 512) W4_CASE(6, 64, 512) W4_CASE(9, 32, 512) W4_CASE(6, 32, 512)
    }
#undef W4_CASE
    set_error("wino4h: no kernel <%d taps, %d channels, %d threads>", p.NT, p.BN, p.NTH);
    return I2V_E_INVALID;
}

}  // namespace i2v
