// The F(4,3) kernel template (see i2v_conv16w4_dev.h and i2v_conv16w4.hip for the design).  No include guard: included once per kernel
// name, inside namespace i2v, behind i2v_conv16w4_dev.h --
//   W4K_NAME conv_wino4_f16x3_kernel, W4K_ONE false  split-fp16 operands, three MFMAs per product (i2v_conv16w4_dev.h)
//   W4K_NAME conv_wino4_f16_kernel,   W4K_ONE true   one-term fp16 operands, one MFMA per product (i2v_conv16w4h.hip, mma = 3)
// The two differ in their tap loops only (w4_pass<..., ONE>).  A kernel template rather than a device function both kernels call:
// wrapping the body changes the register allocation of the split kernel's loops, and this way its code stays what it was.
//   W4K_NAME conv_wino4e_f16x3_kernel, W4K_ONE false, W4K_EDGE  the split kernel that skips temporal edge units (i2v_conv16w4e.hip)
//   W4K_NAME conv_wino4e_f16_kernel,   W4K_ONE true,  W4K_EDGE  its one-term form (same file)
// W4K_EDGE adds a fourth template parameter, the brick's frame count TT (4 or 2: what the compiled dead masks are derived from), and makes
// each wave pick the instantiation of each pass's tap loop whose dead mask is that of its own row blocks in this brick (w4_dead_mask);
// a mask no loop was compiled for runs the full loop.  Without it the kernel body is what it was.
#ifdef W4K_EDGE
template <int NT, int BN, int NTH, int ETT>
#else
template <int NT, int BN, int NTH>
#endif
__global__ __launch_bounds__(NTH, 2) void W4K_NAME(W4Args a) {
#ifdef W4K_EDGE
    constexpr bool EDGE = true;
    static_assert(NTH == 512 && NT >= 6 && (ETT == 4 || ETT == 2), "the edge form: one 512-thread workgroup per brick, 3-D taps");
#else
    constexpr bool EDGE = false;
    constexpr int ETT = 4;
#endif
    constexpr bool ONE = W4K_ONE;
    static_assert(NTH == 512 || (NTH == 256 && BN == 32), "the 256-thread geometry exists for 32-channel workgroups");
    using Geo = W4Geo<NTH>;
    constexpr int NW = NTH / 64;
    constexpr int WMA = BN == 64 ? 4 : 2, WMB = BN == 64 ? 2 : 1;
    constexpr int KT = NT / 3;
    constexpr int ETH_SHIFT = ETT == 4 ? 3 : 4, ETDUP = KT == 2 ? 1 : 0;   // (EDGE) the brick the compiled masks stand for: TH = 32 / TT rows
    (void)ETH_SHIFT; (void)ETDUP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int HH = a.TH + 2;
    const int plane = (a.TT + KT - 1) * HH * 4;
    const int nblk = a.CoutPad >> 5;

    const W4Brick bk = w4_decode<BN>(a, (int)blockIdx.x);
    const int w4_tlv_ = (int)blockIdx.x;   // (timeline builds index their stamps by the workgroup)
    W4_STAMP(0)
    int* gposA = reinterpret_cast<int*>(smem + a.tofs);
    w4_tables<KT, NTH>(a, bk, gposA, tid);
    const int lane = tid & 63;
    const int kg = lane >> 5, l31 = lane & 31;
    int* gposB = gposA + Geo::ROWS_A;
    const int* tpos = gposB + Geo::ROWS_A;
    const int* tres = tpos + Geo::TILES;
    const int n0 = bk.ntile * BN, b0 = bk.b0;
    const char* wbase = a.wp + (long)bk.par * a.wset_stride;   // wave-uniform; the lane's 16 bytes are added by the load
    // descriptor of this brick's sample of V: base + b0 * bytes per sample, num_records = bytes per sample (< 2^31, checked by the launcher)
    const long vsample = (long)a.T * a.nchunk * 6 * a.H * a.J * 64;
    const __amdgpu_buffer_rsrc_t vrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.in) + (long)b0 * vsample, 0, (int)vsample, 0x00020000);
    // V buffers (LDS rows): pass A's two buffers are the two 64 KB regions; pass B's two smaller ones live in the first
    const int rA0 = 0, rA1 = Geo::ROWS_A;
    const int rB0 = rA0, rB1 = rA0 + Geo::ROWS_B;

    // ---- pass A: planes 0..3, wave = (plane, 32-channel half), all 128 tiles   [BN = 32: (plane, tile half)]
    const int xa = wave & 3, nha = BN == 64 ? wave >> 2 : 0, mha = BN == 64 ? 0 : (wave >> 2) * 64;
    f32x16 accA[WMA];
    {
        int arow[WMA];
#pragma unroll
        for (int wm = 0; wm < WMA; ++wm) {
            int m = mha + wm * 32 + w4_row_tile<NTH>(l31);
            const int ij = m & 3; m >>= 2;
            const int ih = m & (a.TH - 1); m >>= a.th_shift;
            arow[wm] = xa * plane + (m * HH + ih) * 4 + ij;
#pragma unroll
            for (int r = 0; r < 16; ++r) accA[wm][r] = 0.f;
        }
#define W4K_PASS_A(M)                                                                                                                          \
        w4_pass<NT, WMA, Geo::VA0, Geo::VA1, NTH, false>(a, smem, gposA, gposB, accA, arow, wbase + ((long)xa * nblk + (n0 >> 5) + nha) * 2048, HH, tid, \
                                         lane, wave, rA0, rA1, w4_tlv_, vrsrc, std::bool_constant<ONE>{}, std::integral_constant<unsigned, (M)>{});
        if constexpr (!EDGE) {
        w4_pass<NT, WMA, Geo::VA0, Geo::VA1, NTH, false>(a, smem, gposA, gposB, accA, arow, wbase + ((long)xa * nblk + (n0 >> 5) + nha) * 2048, HH, tid,
                                         lane, wave, rA0, rA1, w4_tlv_, vrsrc, std::bool_constant<ONE>{});
        } else {
            // the wave's own dead mask in this brick (wave-uniform), and the loops compiled for this geometry: front, back, both ends
            constexpr unsigned MF = w4_dead_mask<WMA>(3 * ETT, ETH_SHIFT, KT, ETDUP, 0, 0, 0);
            constexpr unsigned MB = w4_dead_mask<WMA>(3 * ETT, ETH_SHIFT, KT, ETDUP, 2 * ETT, ETDUP, 4 - WMA);
            constexpr unsigned MFB = w4_dead_mask<WMA>(ETT, ETH_SHIFT, KT, ETDUP, 0, 0, 0);
            const unsigned mk = w4_dead_mask<WMA>(a.T, a.th_shift, KT, a.tdup, bk.t0, bk.par, mha >> 5);
            if (mk == MF) W4K_PASS_A(MF)
            else if (mk == MB) W4K_PASS_A(MB)
            else if (MFB != MF && MFB != MB && mk == MFB) W4K_PASS_A(MFB)
            else W4K_PASS_A(0u)
        }
#undef W4K_PASS_A
    }
    W4_STAMP(2)
    // ---- pass B: planes 4, 5, wave = (plane, 32-channel half, tile half)   [BN = 32: (plane, tile quarter)]
    const int xb = wave & 1, nhb = BN == 64 ? (wave >> 1) & 1 : 0, mhb = BN == 64 ? (wave >> 2) * 64 : (wave >> 1) * 32;
    f32x16 accB[WMB];
    {
        int arow[WMB];
#pragma unroll
        for (int wm = 0; wm < WMB; ++wm) {
            int m = mhb + wm * 32 + w4_row_tile<NTH>(l31);
            const int ij = m & 3; m >>= 2;
            const int ih = m & (a.TH - 1); m >>= a.th_shift;
            arow[wm] = xb * plane + (m * HH + ih) * 4 + ij;
#pragma unroll
            for (int r = 0; r < 16; ++r) accB[wm][r] = 0.f;
        }
        // (chunk 0 of this brick was requested by pass A behind its last chunk and published by its last barrier; pass B's
        //  own request behind ITS last chunk re-reads its chunk 0 harmlessly)
        if constexpr (!EDGE) {
        w4_pass<NT, WMB, Geo::VB0, Geo::VB1, NTH, true>(a, smem, gposB, gposB, accB, arow, wbase + ((long)(4 + xb) * nblk + (n0 >> 5) + nhb) * 2048, HH, tid,
                                        lane, wave, rB0, rB1, w4_tlv_, vrsrc, std::bool_constant<ONE>{});
        } else {
            // (a wave of this pass holds two or one of the brick's row blocks: its mask depends on its tile half / quarter too; every
            //  variant runs the same barriers)
#define W4K_PASS_B(M)                                                                                                                          \
            w4_pass<NT, WMB, Geo::VB0, Geo::VB1, NTH, true>(a, smem, gposB, gposB, accB, arow, wbase + ((long)(4 + xb) * nblk + (n0 >> 5) + nhb) * 2048, HH, tid, \
                                        lane, wave, rB0, rB1, w4_tlv_, vrsrc, std::bool_constant<ONE>{}, std::integral_constant<unsigned, (M)>{});
            constexpr unsigned MF = w4_dead_mask<WMB>(3 * ETT, ETH_SHIFT, KT, ETDUP, 0, 0, 0);
            constexpr unsigned MB = w4_dead_mask<WMB>(3 * ETT, ETH_SHIFT, KT, ETDUP, 2 * ETT, ETDUP, 4 - WMB);
            const unsigned mk = w4_dead_mask<WMB>(a.T, a.th_shift, KT, a.tdup, bk.t0, bk.par, mhb >> 5);
            if (mk == MF) W4K_PASS_B(MF)
            else if (mk == MB) W4K_PASS_B(MB)
            else W4K_PASS_B(0u)
#undef W4K_PASS_B
        }
    }
    W4_STAMP(4)

    // ---- epilogue: E = [6 planes][tiles][32 channels] fp32.  A wave's ds_write_b32 stores the rows m (lanes 0..31) and m + 4
    // (lanes 32..63) of an accumulator register: 512 bytes apart = the same 32 banks.  Tile m is therefore kept in row
    // m ^ ((m >> 2) & 1), which puts the two halves of the wave on the two halves of the banks.
    // One 32-channel half at a time, all of the brick's tiles (98 KB over both V regions).
    constexpr int NQ = 8, TPI = NTH / NQ;         // a thread owns four channels of one tile per iteration
    constexpr int ET = Geo::TILES;                // tiles in E
    constexpr int NIT = ET / TPI;
    float* E = reinterpret_cast<float*>(smem);
    double* S = reinterpret_cast<double*>(reinterpret_cast<char*>(E) + 6 * ET * 32 * 4);   // [2 halves][NW waves][32 channels][2] behind E
    const int n4 = tid % NQ;
    const int e3 = kg * 96, e5 = kg * 160;   // row offsets (in floats) of the wave's upper lanes, see the E writes
    const int e8 = kg * 256;                 // (256-thread kernels: the upper lanes' tile quad is 2 tile quads = 8 rows away, see w4_escatter)
#pragma unroll 1
    for (int half = 0; half < BN / 32; ++half) {
        const int n = n0 + half * 32 + 4 * n4;
        const bool ncol = n < a.Cout;
        double ssum[4] = {0, 0, 0, 0}, ssq[4] = {0, 0, 0, 0};
        float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.bias && ncol) bias = *reinterpret_cast<const float4*>(a.bias + n);
        const float bv[4] = {bias.x, bias.y, bias.z, bias.w};
        // residual rows first, all of them, so that their latency hides behind the LDS exchange
        f32x4 rres[NIT][4];
#pragma unroll
        for (int it = 0; it < NIT; ++it)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                rres[it][c] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.res && ncol)
                    rres[it][c] = *reinterpret_cast<const f32x4*>(a.res + (long)tres[4 * (tid / NQ + TPI * it) + c] * a.Cout + n);
            }
        __syncthreads();   // the V bricks / the previous E are no longer read
        if (half == 0) W4_STAMP(8)
        if (nha == half) {
#pragma unroll
            for (int wm = 0; wm < WMA; ++wm) {
                const int m0 = mha + wm * 32;    // first tile of this row block (wave-uniform)
                // (the row block lies inside E: always true, but the compiler does not know it, and without the branch it pairs the
                //  stores differently and allocates the 64-channel edge kernels' registers anew -- profiles/f43_retire_forms.md)
                if (m0 >= 0 && m0 < ET)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (NTH == 256) E[w4_escatter(xa * ET + m0, r) * 32 + l31 + (w4_escatter_up(r) ? e8 : -e8)] = accA[wm][r];
                    else {
                        // tile m = c + 4 kg sits in row m ^ ((m >> 2) & 1) = c + (r odd ? 3 : 5) kg: two base addresses + immediates
                        const int c = m0 + (r & 3) + 8 * (r >> 2);
                        E[(xa * ET + c) * 32 + l31 + ((r & 1) ? e3 : e5)] = accA[wm][r];
                    }
                }
            }
        }
        if (nhb == half) {
#pragma unroll
            for (int wm = 0; wm < WMB; ++wm) {
                const int m0 = mhb + wm * 32;
                if (m0 >= 0 && m0 < ET)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if constexpr (NTH == 256) E[w4_escatter((4 + xb) * ET + m0, r) * 32 + l31 + (w4_escatter_up(r) ? e8 : -e8)] = accB[wm][r];
                    else {
                        const int c = m0 + (r & 3) + 8 * (r >> 2);
                        E[((4 + xb) * ET + c) * 32 + l31 + ((r & 1) ? e3 : e5)] = accB[wm][r];
                    }
                }
            }
        }
        __syncthreads();
        if (half == 0) W4_STAMP(9)
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int tile = tid / NQ + TPI * it;
            float mx[6][4];
#pragma unroll
            for (int x = 0; x < 6; ++x) {
                const float4 vv = *reinterpret_cast<const float4*>(E + (x * ET + (tile ^ ((tile >> 2) & 1))) * 32 + 4 * n4);
                mx[x][0] = vv.x; mx[x][1] = vv.y; mx[x][2] = vv.z; mx[x][3] = vv.w;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float s12 = mx[1][j] + mx[2][j], d12 = mx[1][j] - mx[2][j];
                const float s34 = mx[3][j] + mx[4][j], d34 = mx[3][j] - mx[4][j];
                const float y[4] = {mx[0][j] + s12 + s34, fmaf(2.f, d34, d12), fmaf(4.f, s34, s12), fmaf(8.f, d34, d12) + mx[5][j]};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float vv = fmaf(y[c], a.oscale, bv[j]) + rres[it][c][j];
                    if (ncol) {
                        ssum[j] += (double)vv;
                        ssq[j] = fma((double)vv, (double)vv, ssq[j]);
                    }
                    if (a.epi & EPI_LRELU) vv = vv >= 0.f ? vv : 0.2f * vv;
                    rres[it][c][j] = vv;
                }
            }
        }
        if (ncol) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const long p = tpos[tid / NQ + TPI * it];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
#ifdef W4_OUT_NT
                    __builtin_nontemporal_store(rres[it][c], reinterpret_cast<f32x4*>(a.out + (p + c) * a.Cout + n));
#else
                    *reinterpret_cast<f32x4*>(a.out + (p + c) * a.Cout + n) = rres[it][c];
#endif
                }
            }
        }
        if (half == 0) W4_STAMP(10)
        if (a.stats) {
            // lanes of a wave that share (lane % NQ) hold the same four channels -> wavefront shuffles; the eight waves'
            // partials meet in LDS (behind E) and one wave per channel half issues its 2 x 32 fp64 atomics
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if constexpr (NQ <= 8) { ssum[j] = wave_xor_add_f64<8>(ssum[j]); ssq[j] = wave_xor_add_f64<8>(ssq[j]); }
                ssum[j] = wave_xor_add_f64<16>(ssum[j]); ssq[j] = wave_xor_add_f64<16>(ssq[j]);
                ssum[j] = wave_xor_add_f64<32>(ssum[j]); ssq[j] = wave_xor_add_f64<32>(ssq[j]);
            }
            // (each half has its own 4 KB of S: the cross-wave sums and the atomics of both halves wait until after the loop,
            //  one barrier and two waves instead of a barrier and a serial section of wave 0 per half)
            double* Sh = S + half * (NW * 32 * 2);
            if (lane < NQ) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    Sh[(wave * 32 + 4 * lane + j) * 2] = ssum[j];
                    Sh[(wave * 32 + 4 * lane + j) * 2 + 1] = ssq[j];
                }
            }
        }
        W4_STAMP(5 + half)
    }
    if (a.stats) {
        __syncthreads();
        if (wave < BN / 32 && lane < 32 && n0 + wave * 32 + lane < a.Cout) {   // wave h sums channel half h
            const double* Sh = S + wave * (NW * 32 * 2);
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                s0 += Sh[(w * 32 + lane) * 2];
                s1 += Sh[(w * 32 + lane) * 2 + 1];
            }
            double* dst = a.stats + ((long)b0 * a.Cout + n0 + wave * 32 + lane) * 2;
            atomicAdd(dst, s0);
            atomicAdd(dst + 1, s1);
        }
    }
    W4_STAMP(7)
}
#undef W4K_NAME
#undef W4K_ONE
#undef W4K_EDGE
