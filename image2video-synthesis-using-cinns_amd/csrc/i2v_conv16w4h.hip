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
// channels by the writer and zero weights by the packer.
// The epilogue is the split kernel's: A^T M in fp32, 2^-wexp, bias, residual through the up-sampling map, optional lrelu, fused fp64
// statistics.  Same kernel template (i2v_conv16w4_kernel.h), one-brick-per-workgroup form only, no measurement switches.
#define W4_NO_INSTRUMENT
#include "i2v_conv16w4_dev.h"

namespace i2v {

#define W4K_NAME conv_wino4_f16_kernel
#define W4K_ONE true
#include "i2v_conv16w4_kernel.h"

// w3: [nset][Cout][Cin][NT][3] (fp64, already scaled); packs U = G g per (kt, kh), rounded to fp16 once (the hi part of the split packer)
static int wino4h_pack_sets(Wino4hWeights& o, const std::vector<double>& w3, int nset, int cout, int cin, int kt) {
    o.Cin = cin; o.Cout = cout; o.KT = kt;
    o.CinPad = (cin + 63) / 64 * 64;
    o.CoutPad = (cout + 31) / 32 * 32;
    o.nchunk = o.CinPad / 32;
    const int NT = kt * 3;
    std::vector<double> u((size_t)nset * cout * cin * NT * 6);
    double wmax = 0.0;
    for (size_t i = 0; i < (size_t)nset * cout * cin * NT; ++i) {
        const double g0 = w3[i * 3], g1 = w3[i * 3 + 1], g2 = w3[i * 3 + 2];
        double* d = &u[i * 6];
        d[0] = g0 / 4.0;
        d[1] = -(g0 + g1 + g2) / 6.0;
        d[2] = -(g0 - g1 + g2) / 6.0;
        d[3] = g0 / 24.0 + g1 / 12.0 + g2 / 6.0;
        d[4] = g0 / 24.0 - g1 / 12.0 + g2 / 6.0;
        d[5] = g2;
        for (int x = 0; x < 6; ++x) wmax = std::max(wmax, std::fabs(d[x]));
    }
    o.wexp = 0;   // the split packer's prescale: the largest |U| lands at 2^14
    if (wmax > 0.0 && std::isfinite(wmax)) o.wexp = std::max(-40, std::min(40, (int)std::floor(std::log2(16384.0 / wmax))));
    const double pre = std::ldexp(1.0, o.wexp);
    const size_t set_halfs = (size_t)NT * o.nchunk * 6 * o.CoutPad * 32;
    std::vector<_Float16> p((size_t)nset * set_halfs, (_Float16)0.f);
    for (int s = 0; s < nset; ++s)
        for (int n = 0; n < cout; ++n)
            for (int c = 0; c < cin; ++c)
                for (int tap = 0; tap < NT; ++tap)
                    for (int x = 0; x < 6; ++x) {
                        const float v = (float)(u[((((size_t)s * cout + n) * cin + c) * NT + tap) * 6 + x] * pre);
                        // fragment-major: [tap][chunk][x][32-channel block][k-step][lane = kg * 32 + n % 32][8 halfs]
                        const int chunk = c / 32, cc = c % 32, ks = cc >> 4, kgq = (cc >> 3) & 1, j = cc & 7;
                        _Float16* blk = &p[s * set_halfs + ((((size_t)tap * o.nchunk + chunk) * 6 + x) * (o.CoutPad / 32) + n / 32) * 1024];
                        blk[ks * 512 + (kgq * 32 + n % 32) * 8 + j] = (_Float16)v;
                    }
    o.set_bytes = (long)set_halfs * 2;
    return o.w.upload(p.data(), p.size() * 2);
}

bool wino4h_supported(int cout, int cin, int T, int H, int W, int KT) {
    if (cout % 32 || cin % 32 || (KT != 3 && KT != 2)) return false;
    int TT, TH;
    return wino4_tiling(T, H, W, KT, &TT, &TH);
}

int Wino4hWeights::pack(const float* w_src, const float* bias_src, int cout, int cin, double scale) {
    tdup = false;
    std::vector<double> w3((size_t)cout * cin * 27);
    for (size_t i = 0; i < w3.size(); ++i) w3[i] = (double)w_src[i] * scale;
    int rc = wino4h_pack_sets(*this, w3, 1, cout, cin, 3);
    if (rc) return rc;
    if (bias_src) return bias.upload(bias_src, (size_t)cout * 4);
    bias.release();
    return I2V_OK;
}

int Wino4hWeights::pack_tdup(const float* w_src, const float* bias_src, int cout, int cin, double scale) {
    // parity 0 = (W[0], W[1]+W[2]), parity 1 = (W[0]+W[1], W[2]) along time (as Wino4Weights::pack_tdup)
    std::vector<double> w3((size_t)2 * cout * cin * 18);
    for (int par = 0; par < 2; ++par)
        for (size_t nc = 0; nc < (size_t)cout * cin; ++nc)
            for (int hw = 0; hw < 9; ++hw) {
                const double w0 = w_src[nc * 27 + hw], w1 = w_src[nc * 27 + 9 + hw], w2 = w_src[nc * 27 + 18 + hw];
                double* dst = &w3[((size_t)par * cout * cin + nc) * 18];
                dst[hw] = (par == 0 ? w0 : w0 + w1) * scale;
                dst[9 + hw] = (par == 0 ? w1 + w2 : w2) * scale;
            }
    tdup = true;
    int rc = wino4h_pack_sets(*this, w3, 2, cout, cin, 2);
    if (rc) return rc;
    if (bias_src) return bias.upload(bias_src, (size_t)cout * 4);
    bias.release();
    return I2V_OK;
}

template <int NT, int BN, int NTH>
static int launch_wino4h(const W4Args& a, size_t lds, hipStream_t st) {
    auto kern = conv_wino4_f16_kernel<NT, BN, 0, NTH>;
    static bool attr_set[I2V_MAX_DEV] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), 160 * 1024, attr_set)) return rc;
    hipLaunchKernelGGL(kern, dim3((unsigned)a.nvirt), dim3(NTH), lds, st, a);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

static int device_cus_h() {
    static int cus[I2V_MAX_DEV] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= I2V_MAX_DEV) return 256;
    if (!cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return cus[dev];
}

// The launch geometry is the production geometry of wino4_forward: 64-channel workgroups (32 where 64 would leave CUs idle), and the
// 256-thread 32-channel form for layers that have 32 output channels.
int wino4h_forward(const Wino4hWeights& wts, const void* v16, float* out, const float* res, int rt, int rs, int B, int T, int H, int W,
                   int epi, hipStream_t st, double* stats) {
    I2V_REQUIRE(wts.w.p, I2V_E_STATE, "wino4h: weights not packed");
    I2V_REQUIRE((epi & ~EPI_LRELU) == 0, I2V_E_INVALID, "wino4h: unsupported epilogue %d", epi);
    W4Args a{};
    if (int rc0 = zero_page(&a.zeros)) return rc0;
    a.in = static_cast<const char*>(v16); a.wp = wts.w.as<char>(); a.bias = wts.bias.as<float>(); a.res = res; a.out = out;
    a.stats = stats;
    a.B = B; a.H = H; a.W = W; a.J = W / 4; a.Cin = wts.Cin; a.Cout = wts.Cout; a.CoutPad = wts.CoutPad; a.nchunk = wts.nchunk;
    a.tdup = wts.tdup ? 1 : 0;
    a.wset_stride = wts.set_bytes;
    if (wts.tdup) {  // T is the OUTPUT frame count; the half-rate input has T / 2 frames
        I2V_REQUIRE(T % 2 == 0 && !res, I2V_E_INVALID, "wino4h: temporal-duplication mode needs an even frame count and no residual");
        T /= 2;
    }
    a.T = T;
    I2V_REQUIRE(wino4h_supported(wts.Cout, wts.Cin, T, H, W, wts.KT), I2V_E_INVALID, "wino4h: unsupported shape [%d,%d,%d] %d -> %d (kt = %d)",
                T, H, W, wts.Cin, wts.Cout, wts.KT);
    a.rt = res ? rt : 1; a.rs = res ? rs : 1; a.epi = epi;
    I2V_REQUIRE((a.rt == 1 || a.rt == 2 || a.rt == 4) && (a.rs == 1 || a.rs == 2 || a.rs == 4), I2V_E_INVALID,
                "wino4h: residual up-sampling factors %d / %d (1, 2 or 4)", a.rt, a.rs);
    a.rt_shift = a.rt >> 1 == 2 ? 2 : a.rt >> 1; a.rs_shift = a.rs >> 1 == 2 ? 2 : a.rs >> 1;
    a.oscale = (float)std::ldexp(1.0, -wts.wexp);
    int TT = 1, TH = 1;
    (void)wino4_tiling(T, H, W, wts.KT, &TT, &TH);
    int BN = a.CoutPad % 64 == 0 ? 64 : 32;
    if (BN == 64 && (long)B * (T / TT) * (H / TH) * (a.J / 4) * (a.CoutPad / 64) * (wts.tdup ? 2 : 1) < device_cus_h()) BN = 32;
    bool thin = false;
    {
        int TT2 = 1, TH2 = 1;
        if (BN == 32 && a.CoutPad % 64 != 0 &&
            wino4_tiling(T, H, W, wts.KT, &TT2, &TH2, W4Geo<256>::TILES, W4Geo<256>::ROWS_A, W4Geo<256>::ROWS_B)) {
            thin = true; TT = TT2; TH = TH2;
        }
    }
    a.TT = TT; a.TH = TH; a.TJ = 4; a.nbT = T / TT; a.nbH = H / TH; a.nbJ = a.J / 4;
    a.th_shift = 0;
    while ((1 << a.th_shift) < TH) ++a.th_shift;
    I2V_REQUIRE((1 << a.th_shift) == TH, I2V_E_INVALID, "wino4h: brick height %d is not a power of two", TH);
    a.hh_magic = ((1 << 20) + TH + 1) / (TH + 2);
    I2V_REQUIRE(!stats || (long)TT * TH * 4 <= (long)T * H * a.J, I2V_E_INVALID, "wino4h: fused statistics need bricks inside one sample");
    a.order = W4_DEFAULT_ORDER;
    const long nblk = (long)B * a.nbT * a.nbH * a.nbJ * (a.CoutPad / BN);
    I2V_REQUIRE(nblk > 0 && nblk < (1L << 30), I2V_E_INVALID, "wino4h: grid of %ld workgroups", nblk);
    I2V_REQUIRE((long)T * a.nchunk * 6 * H * a.J * 64 < (1L << 31), I2V_E_INVALID, "wino4h: the V operand of one sample ([%d,%d,%d] x %d chunks) exceeds the 2 GB a buffer descriptor offset can address", T, H, W, a.nchunk);
    I2V_REQUIRE((long)B * T * a.nchunk * 6 * H * a.J < (1L << 31) && (long)B * (wts.tdup ? 2 * T : T) * H * W < (1L << 31), I2V_E_INVALID,
                "wino4h: batch %d too large for the 32-bit row indices of this kernel ([%d,%d,%d] x %d chunks)", B, T, H, W, a.nchunk);
    a.nvirt = (int)(a.tdup ? 2 * nblk : nblk);
    if (thin) {   // two 256-thread workgroups per CU: 2 V regions of 576 rows + one table set
        a.tofs = 2 * W4Geo<256>::ROWS_A * 64;
        const size_t lds = (size_t)a.tofs + (size_t)w4_table_bytes<256>();
        return wts.KT == 3 ? launch_wino4h<9, 32, 256>(a, lds, st) : launch_wino4h<6, 32, 256>(a, lds, st);
    }
    a.tofs = 2 * W4_ROWS_A * 64;
    const size_t lds = (size_t)a.tofs + (size_t)W4_TABLE_BYTES;
    if (BN == 64) return wts.KT == 3 ? launch_wino4h<9, 64, 512>(a, lds, st) : launch_wino4h<6, 64, 512>(a, lds, st);
    return wts.KT == 3 ? launch_wino4h<9, 32, 512>(a, lds, st) : launch_wino4h<6, 32, 512>(a, lds, st);
}

}  // namespace i2v
