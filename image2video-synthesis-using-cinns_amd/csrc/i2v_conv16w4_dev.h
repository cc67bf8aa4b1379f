// Device side of the Winograd F(4,3) split-fp16 convolution (see i2v_conv16w4.hip for the design): argument blocks, the tap-loop
// pass (w4_pass), the brick decode, the index tables and the kernel template -- shared by i2v_conv16w4.hip (the kernels that read
// the operand V a producer launch wrote), i2v_conv16w4h.hip (their one-term fp16 form) and i2v_conv16w4g.hip (the kernel that
// generates it in its own producer waves); at the end the host-side launch plan (wino4_plan) all three are launched from.
// A translation unit that defines W4_NO_INSTRUMENT before including this file gets no measurement hooks (timeline stamps,
// per-tap timing): their device-side buffers live in i2v_conv16w4.hip only.
#pragma once
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <vector>

#include "i2v_conv.h"
#include "i2v_conv16w4_edge.h"

#ifdef W4_NO_INSTRUMENT
#undef W4_TIMELINE
#undef W4_TAPTIME
#endif

namespace i2v {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifdef W4_TIMELINE   // measurement builds (tools/conv16w_check): per-workgroup phase stamps, 100 MHz wall clock
__device__ unsigned long long w4_tl[8192 * 16];
#define W4_STAMP(i) { if (tid == 0 && w4_tlv_ < 8192) w4_tl[w4_tlv_ * 16 + (i)] = wall_clock64(); }   // w4_tlv_: the workgroup
#else
#define W4_STAMP(i) {}
#endif
#ifdef W4_ABLATE_AL   // measurement builds only (wrong results): the lo halves of the A operands are not read from LDS
#define W4_ABL_AL(x, y) y
#else
#define W4_ABL_AL(x, y) x
#endif
#ifdef W4_ABLATE_BL   // measurement builds only (wrong results): the lo weight fragment is loaded from the hi fragment's lines
#define W4_ABL_BL(x, y) y
#else
#define W4_ABL_BL(x, y) x
#endif
#ifdef W4_TAPTIME   // measurement builds: time between the starts of consecutive taps, per wave and tap slot (s_memtime, 100 MHz)
__device__ unsigned long long w4_tt[2 * 8 * 18 * 2];   // [pass][wave][tap slot]{ticks, count}
#define W4_TT(U)                                                                                                     \
    {                                                                                                                \
        const unsigned long long now_ = __builtin_readcyclecounter();                                                \
        if (lane == 0) { tt_lds[(U)] += (unsigned)(now_ - tt_prev); tt_cnt[(U)] += 1; }                              \
        tt_prev = now_;                                                                                              \
    }
#else
#define W4_TT(U)
#endif
constexpr int W4_DEFAULT_ORDER = 2;   // brick -> XCD order (kernel comment); I2V_W4_ORDER overrides for A/B runs
// Cache-policy experiments (measurement builds, tools/build_measurement_libs.sh nt): -DW4_V_NT marks the V stream (LDS-DMA loads)
// non-temporal so that it does not turn the weight fragments out of the 4 MB L2; -DW4_OUT_NT stores the output non-temporally.
#ifdef W4_V_NT
#define W4_V_POLICY " nt"
#else
#define W4_V_POLICY ""
#endif
constexpr int W4_TILES = 128;   // tiles (of four output positions) per workgroup of the 512-thread kernels
constexpr int W4_KC = 16;       // input channels per K chunk
constexpr int W4_ROWS_A = 1024; // staged V rows per buffer, pass A (4 planes); pass B stages 512 (2 planes)  [512-thread kernels]

// Workgroup geometry.  NTH = 512: the kernel as described above (8 waves, 128 tiles, one workgroup per CU: 138 KB of LDS).
// NTH = 256 (round 5, 32-channel layers only): 4 waves, 64 tiles (4 frames x 4 rows x 16 positions), TWO workgroups per CU (2 x 78 KB).
// A 32-channel workgroup of the 512-thread kernel is two independent 64-tile halves that share nothing but the V brick (pass A:
// wave = (plane, tile half) with two row blocks per weight fragment; pass B: (plane, tile quarter) with one): splitting it into two
// workgroups keeps every wave's loop exactly as it was -- same fragments per MFMA, same accumulation order, same bits -- and lets
// the CU run one workgroup's tables / first brick / hand-over / epilogue (10 of 22 us per 128 tiles on the 64 -> 32 layer at 128 x 128,
// matrix pipe idle) underneath the other one's tap loops, which one workgroup per CU cannot do.  The halo brick of 64 tiles has
// 4 x 144 rows per chunk (36 KB) instead of 4 x 240: 1.2 x the V bytes through L2 per tile.
// A workgroup load instruction (global_load_lds_dwordx4, one per thread) stages NTH / 4 rows of 64 bytes; a chunk's brick is
// requested in two half-requests of V0 and V1 such instructions.
template <int NTH> struct W4Geo;
template <> struct W4Geo<512> { static constexpr int TILES = 128, ROWS_A = 1024, ROWS_B = 512, VA0 = 4, VA1 = 4, VB0 = 2, VB1 = 2; };
template <> struct W4Geo<256> { static constexpr int TILES = 64, ROWS_A = 576, ROWS_B = 320, VA0 = 5, VA1 = 4, VB0 = 3, VB1 = 2; };
template <int NTH> constexpr int w4_table_bytes() { return (2 * W4Geo<NTH>::ROWS_A + 5 * W4Geo<NTH>::TILES) * 4; }
// Which tile of its 32-tile row block an MFMA row (= A-operand lane l31) holds.  512-thread kernels: tile = row (32 consecutive
// tiles = 32 consecutive V rows, which the XOR key (row >> 2) & 3 spreads over the 16-byte slots without conflicts for the four
// 16-lane groups {0-3,12-15,20-27} {4-11,16-19,28-31} ... of ds_read_b128).  The 64-tile brick is 4 frames x 4 rows x 4 tiles: a row
// block is two 16-row runs 24 rows apart (keys k .. k+3 and k+2 .. k+5), and with tile = row both lane groups would read two
// pairs of rows with equal keys (2-way conflicts: 41 % conflict cycles when round 3 tried this brick).  So the eight lane quads
// take the tile quads 0 2 3 1 6 4 5 7: group {0,3,5,6} -> tile quads {0,1,4,5} = keys {k,k+1,k+2,k+3}, group {1,2,4,7} -> {2,3,6,7} =
// keys {k+2,k+3,k,k+1}.  Only the row -> tile labels move (arow here, the accumulator scatter in the epilogue): no loop changes,
// and no output's accumulation order either.
// The accumulator scatter that goes with it (256-thread kernels).  Register r of lane (l31, kg) is MFMA row (r & 3) + 8 (r >> 2) + 4 kg =
// lane quad j = 2 (r >> 2) + kg, i.e. tile quad tq = {0 2 3 1 6 4 5 7}[j], tile 4 tq + (r & 3), kept in E row tile ^ (tq & 1):
//   r >> 2 = 0: tq = 0 | 2 -> row (r & 3)           + 8 kg        r >> 2 = 1: tq = 3 | 1 -> row 12 + ((r & 3) ^ 1) - 8 kg
//   r >> 2 = 2: tq = 6 | 4 -> row 24 + (r & 3)      - 8 kg        r >> 2 = 3: tq = 5 | 7 -> row 20 + ((r & 3) ^ 1) + 8 kg
// w4_escatter: the row for kg = 0 (compile-time in r); w4_escatter_up: whether the upper lanes sit 8 rows above (else below).
__device__ __forceinline__ constexpr int w4_escatter(int base, int r) {
    return base + ((r >> 2) == 0 ? 0 : (r >> 2) == 1 ? 12 : (r >> 2) == 2 ? 24 : 20) + ((r & 3) ^ ((r >> 2) & 1));
}
__device__ __forceinline__ constexpr bool w4_escatter_up(int r) { return (r >> 2) == 0 || (r >> 2) == 3; }
template <int NTH> __device__ __forceinline__ int w4_row_tile(int l31) {
    if constexpr (NTH == 256) return 4 * ((0x75461320u >> (4 * (l31 >> 2))) & 7) + (l31 & 3);
    else return l31;
}

struct W4Args {
    const char* in;     // V: hl16 [B][T][Cin/16][6][H][J][64 B], J = W / 4
    const char* wp;     // U: [parity][tap][chunk][6][CoutPad/32][hi | lo][64 lanes][16 B]
    const float* bias;
    const float* res;
    float* out;         // fp32 channels-last [B][To][H][W][Cout]
    double* stats;
    int B, T, H, W, J, Cin, Cout, CoutPad, nchunk;   // T = frames of the INPUT tensor
    int tdup;
    long wset_stride;
    int TT, TH, TJ, nbT, nbH, nbJ;
    int th_shift, rt_shift, rs_shift, hh_magic;   // TH, rt, rs are powers of two; hh_magic = ceil(2^20 / (TH + 2)): n / HH == n * hh_magic >> 20 for n * HH < 2^20
    int rt, rs, epi;
    float oscale;
    int tofs;           // LDS byte offset of the index tables
    int order;          // brick -> XCD order (see w4_decode): 0 round-robin over the flat brick index, 1 / 2 one w-column per XCD
    int nvirt;          // virtual workgroups = bricks x channel tiles x frame parities = the grid
};

// Wave priority inside a chunk.  The two waves of a SIMD share the matrix pipe, arbitrated by priority, then age: at equal
// priority the older wave (0..3) runs its taps at full speed, the younger one gets the leftover slots, falls ~4 taps behind per
// chunk, finishes the chunk alone at half the pipe rate while the older one waits ~2000 cycles at the chunk barrier
// (per-tap timing, -DW4_TAPTIME).  A priority that FALLS with the tap index hands the pipe to whichever wave is behind.
#ifndef W4_PRIO
#define W4_PRIO 1
#endif
constexpr int w4_prio(int t, int NT) {
    return NT == 3 ? 3 - t : (t < 6 ? 3 - t / 2 : 0);   // 9 taps: 3 3 2 2 1 1 0 0 0
}
constexpr int w4_count(int t, int R, int NT, int h) {
    int n = 0;
    for (int k = 0; k < R; ++k) n += ((t - k - h) % NT + NT) % NT == 0;
    return n;
}

// One pass of the K loop over NPL = VH planes... (VH = 16-byte V pieces per thread and half-request: 4 -> 1024 staged rows =
// four planes, 2 -> 512 rows = two planes).  WM = MFMA row blocks of this wave.  arow[wm]: LDS row of the lane's tile (tap
// (0,0)) inside the pass's brick; gpos: V row (chunk 0, inside the sample) of every staged row, W4_PAD_ROW = zero padding; wfrag: this wave's
// weight fragments (tap 0, chunk 0).
// gposN / PRE: hand-over between the passes.  The request a chunk issues for "the next chunk" is a harmless repeat behind the
// LAST chunk; pass A instead requests chunk 0 of pass B's brick there (table gposN: its rows in front, padding behind), into the
// buffer pass B reads first, so that pass B (PRE = true) starts without a V round trip.
// rb0 / rb1: the LDS rows at which the pass's two V buffers start.
// The V requests go through a raw buffer descriptor of the brick's SAMPLE (`vrsrc`: base = the sample's V tensor, num_records = its
// bytes < 2^31): the table holds the row index inside the sample (padding rows: W4_PAD_ROW = 2^25, i.e. byte offset 2^31, out of range
// under any reading of the range check, and an out-of-range lane of `buffer_load ... lds` writes ZEROS into LDS:
// tools/bufload_lds_test), the lane's offset is ONE v_lshl_or_b32, the chunk goes into the scalar offset -- 5 instead of the 13
// instructions per load of a 64-bit address in front of the first MFMAs of taps 0 / 1, where
// profiles/r05_n_f43_inloop_idle_analysis.md finds most of the tap loops' idle cycles.
constexpr int W4_PAD_ROW = 1 << 25;
// ONE (i2v_conv16w4h.hip, mma = 3): the one-term fp16 form.  A 64-byte V row then holds the fp16 values of 32 channels, pieces
// [c0-7 | c16-23 | c8-15 | c24-31], so the two operands a lane reads per row block ("ah" / "al" below) are the k-steps of channels
// 0..15 and 16..31, and the weight fragment's halves are those two k-steps instead of hi | lo: a tap issues 2 WM MFMAs (ah bh, al bl)
// instead of 3 WM over twice the channels -- one third per input channel.  Same loads in the same order, same wait counts.
// DEAD (i2v_conv16w4e.hip): compile-time mask over (kt, own row block), bit kt * WM + wm, of the units that read zero padding only
// (w4_unit_dead).  A dead unit's MFMAs are not emitted, nor its operand's two ds_read_b128 and their address piece; every other piece
// keeps its slot -- the weight requests, every V request, every wait, both barriers, the priorities -- so the in-order VMEM stream and
// the hand-counted waits are those of DEAD = 0, and so are the bits: the products left out are exact zeros.
template <int NT, int WM, int VH0, int VH1, int NTH, bool PRE, bool ONE = false, unsigned DEAD = 0>
__device__ __forceinline__ void w4_pass(const W4Args& a, char* smem, const int* gpos, const int* gposN, f32x16 (&acc)[WM],
                                        int (&arow)[WM], const char* wfrag, int HH, int tid, int lane, int wave, int rb0, int rb1,
                                        int w4_tlv_, __amdgpu_buffer_rsrc_t vrsrc,
                                        std::bool_constant<ONE> = {}, std::integral_constant<unsigned, DEAD> = {}) {
    constexpr int RPL = NTH / 4;          // V rows staged by one load instruction of the workgroup (4 threads per 64-byte row)
    // GEN (VH0 = VH1 = 0): this pass requests no V at all -- the producer waves of conv_wino4g_f16x3_kernel generate every chunk's
    // brick into the buffer the chunk barrier publishes (same buffers, same barriers); the wait counts then hold only weight loads
    constexpr bool GEN = VH0 == 0 && VH1 == 0;
    const int kg = lane >> 5;
    char* v_lds = smem;
    const long cstride = (long)a.CoutPad * 384;          // bytes per (tap, chunk): 6 planes x CoutPad x 64
    const long wtap_stride = (long)a.nchunk * cstride;
    const unsigned lds0 = (unsigned)(unsigned long)(__attribute__((address_space(3))) char*)smem;
    const unsigned vdst = __builtin_amdgcn_readfirstlane(lds0 + wave * 1024);
    const unsigned voff0 = __builtin_amdgcn_readfirstlane(rb0 * 64), voff1 = __builtin_amdgcn_readfirstlane(rb1 * 64);   // byte offsets of the two V buffers
    const int* gq = gpos + (tid >> 2);
    const int* gqn = gposN + (tid >> 2);
    const unsigned vpiece32 = (unsigned)(((tid & 3) ^ ((tid >> 4) & 3)) * 16);   // the thread's 16-byte piece of a V row (XOR swizzle)
    const unsigned vchunk32 = (unsigned)__builtin_amdgcn_readfirstlane(6 * a.H * a.J * 64);   // bytes between the K chunks of one frame
    const unsigned wofs = lane * 16;                     // the lane's piece of a weight fragment (the rest of the address is scalar)
    {   // the fragment base goes into the loads' scalar address operand: make its uniformity explicit
        const unsigned long w_ = (unsigned long)wfrag;
        const unsigned lo_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w_);          // (the builtin returns int:
        const unsigned hi_ = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(w_ >> 32));  //  no sign extension)
        wfrag = reinterpret_cast<const char*>((unsigned long)lo_ | ((unsigned long)hi_ << 32));
    }
#define W4_BLDS(off_, soff_, dst_)                                                                                   \
    {                                                                                                                \
        unsigned keep_;                                                                                              \
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %4 offen lds" W4_V_POLICY "\n\ts_mov_b32 m0, %0" \
                     : "=&s"(keep_) : "v"(off_), "s"(vrsrc), "s"(dst_), "s"(soff_) : "memory");                      \
    }
#define W4_REQUEST_V(ch_, VB, HF)                                                                                    \
    if constexpr (!GEN) {                                                                                            \
        const bool nx_ = (ch_) >= a.nchunk;              /* behind the last chunk: the hand-over table, chunk 0 */    \
        const int* gt_ = nx_ ? gqn : gq;                                                                             \
        constexpr int nv_ = (HF) ? VH1 : VH0, v0_ = (HF) ? VH0 : 0;   /* this half-request's load instructions */     \
        int gp_[nv_];                                                                                                \
        _Pragma("unroll") for (int u = 0; u < nv_; ++u) gp_[u] = gt_[RPL * (v0_ + u)];                               \
        const unsigned so_ = (unsigned)(nx_ ? 0 : (ch_)) * vchunk32;                                                 \
        _Pragma("unroll") for (int u = 0; u < nv_; ++u) {                                                            \
            const unsigned o_ = ((unsigned)gp_[u] << 6) | vpiece32;                                                  \
            W4_BLDS(o_, so_, vdst + ((VB) ? voff1 : voff0) + (unsigned)((v0_ + u) * (NTH * 16)))                      \
        }                                                                                                            \
    }
    struct AOps { half8 ah[WM], al[WM]; };
    struct BOps { half8 bh, bl; };
    AOps a0, a1;
    int adn[WM];
    constexpr int R = NT == 9 ? 9 : 6;
    // tap at whose start the second half of the next chunk's V brick is requested (the first half: tap 0).  A 3-tap chunk
    // (SPADE's 2-D convs) requests both at tap 0: the brick then has two taps instead of one to arrive before the chunk barrier.
    constexpr int VT1 = NT == 3 ? 0 : 1;
    BOps bq0, bq1, bq2, bq3, bq4, bq5, bq6, bq7, bq8;
    /* LDS address of one row block of the A operands, and its two ds_read_b128 */
#define W4_ADDR_A(TAP, VB, wm)                                                                                       \
    {                                                                                                                \
        const int r_ = arow[wm] + (((TAP) / 3) * HH + ((TAP) % 3)) * 4 + ((VB) ? rb1 : rb0);                       \
        adn[wm] = (r_ << 6) + (((kg << 1) ^ ((r_ >> 2) & 3)) << 4);                                                  \
    }
#define W4_READ_A(o, wm)                                                                                             \
    {                                                                                                                \
        (o).ah[wm] = *reinterpret_cast<const half8*>(v_lds + adn[wm]);                                               \
        W4_ABL_AL((o).al[wm] = *reinterpret_cast<const half8*>(v_lds + (adn[wm] ^ 16)), (o).al[wm] = (o).ah[wm]);    \
    }
    /* (DEAD = 0 folds in the front end: the kernels without a mask are compiled from exactly the code they were) */
#define W4_IS_DEAD(TAP, wm) (DEAD != 0u && (((DEAD) >> (((TAP) / 3) * WM + (wm))) & 1u))
#define W4_LOAD_A(o, TAP, VB)                                                                                        \
    {                                                                                                                \
        _Pragma("unroll") for (int wm = 0; wm < WM; ++wm) {                                                          \
            if (!W4_IS_DEAD(TAP, wm)) {                                                                              \
                W4_ADDR_A(TAP, VB, wm)                                                                               \
                W4_READ_A(o, wm)                                                                                     \
            }                                                                                                        \
        }                                                                                                            \
    }
    /* weight fragments of one tap: scalar base + the lane's 16 bytes */                                            \
#define W4_REQUEST_B(q, TAP, CH)                                                                                     \
    {                                                                                                                \
        const int c_ = (CH) < a.nchunk ? (CH) : a.nchunk - 1;                                                        \
        const char* p_ = wfrag + (long)(TAP) * wtap_stride + (long)c_ * cstride;                                     \
        asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"((q).bh) : "v"(wofs), "s"(p_));                         \
        W4_ABL_BL(asm volatile("global_load_dwordx4 %0, %1, %2 offset:1024" : "=&v"((q).bl) : "v"(wofs), "s"(p_)),   \
                  asm volatile("global_load_dwordx4 %0, %1, %2" : "=&v"((q).bl) : "v"(wofs), "s"(p_)));              \
    }
#define W4_WAIT_B(q, N) asm volatile("s_waitcnt vmcnt(%2)" : "+v"((q).bh), "+v"((q).bl) : "n"(N));
#define W4_WAIT_VM(N) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
    // The 3 WM MFMAs of a tap with everything else this wave has to issue for the NEXT taps in the 32-cycle shadows between
    // them, one small piece per gap: an in-order wave that issues its MFMAs back to back sits blocked on the pipe, and whatever
    // it issues outside the MFMA block is time the pipe idles unless the partner wave happens to have an MFMA ready (per-tap
    // timing: a wave running alone reached 54 % of the pipe, the pair 66-76 %).  Pieces: per row block the LDS address
    // arithmetic and the two ds_read_b128 of the next tap's A operands, then the weight request of tap U + R - 1.
    // MFMAs per row block and tap, and the gap behind which the weight request goes (ONE: behind the last A-operand read)
    constexpr int NTERM = ONE ? 2 : 3, IREQ = ONE ? 2 * WM - 1 : 2 * WM;
#define W4_MFMA_SPREAD(o, q, TAPC, onxt, TAPN, VBN, QREQ, TAPR, CHR)                                                       \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < NTERM * WM; ++i) {                                                     \
            const int wm_ = i % WM, term_ = i / WM;                                                                  \
            if (W4_IS_DEAD(TAPC, wm_)) {                                                                             \
            } else if constexpr (ONE)                                                                                \
                acc[wm_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term_ ? (o).al[wm_] : (o).ah[wm_],                 \
                                                                  term_ ? (q).bl : (q).bh, acc[wm_], 0, 0, 0);       \
            else                                                                                                     \
                acc[wm_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(term_ == 2 ? (o).al[wm_] : (o).ah[wm_],            \
                                                                  term_ == 1 ? (q).bl : (q).bh, acc[wm_], 0, 0, 0);  \
            __builtin_amdgcn_sched_barrier(0);                                                                       \
            if (WM >= 2) {                                                                                           \
                if (i < 2 * WM && (i & 1) == 0 && !W4_IS_DEAD(TAPN, i / 2)) W4_ADDR_A(TAPN, VBN, i / 2)              \
                if (i < 2 * WM && (i & 1) == 1 && !W4_IS_DEAD(TAPN, i / 2)) W4_READ_A(onxt, i / 2)                   \
                if (i == IREQ) W4_REQUEST_B(QREQ, TAPR, CHR)                                   \
            } else {                                                                                                 \
                if (i == 0 && !W4_IS_DEAD(TAPN, 0)) W4_ADDR_A(TAPN, VBN, 0)                                          \
                if (i == 1 && !W4_IS_DEAD(TAPN, 0)) W4_READ_A(onxt, 0)                                               \
                if (i == IREQ) W4_REQUEST_B(QREQ, TAPR, CHR)                                   \
            }                                                                                                        \
            __builtin_amdgcn_sched_barrier(0);                                                                       \
        }                                                                                                            \
    }

    // prologue: the first R-1 weight requests do not need the index tables; everything requested here has landed before the
    // loop starts (the wait counts inside the loop assume the steady state and would under-wait in the first taps otherwise)
    W4_REQUEST_B(bq0, 0 % NT, 0 / NT)
    W4_REQUEST_B(bq1, 1 % NT, 1 / NT)
    W4_REQUEST_B(bq2, 2 % NT, 2 / NT)
    W4_REQUEST_B(bq3, 3 % NT, 3 / NT)
    W4_REQUEST_B(bq4, 4 % NT, 4 / NT)
    if constexpr (R == 9) {
        W4_REQUEST_B(bq5, 5 % NT, 5 / NT)
        W4_REQUEST_B(bq6, 6 % NT, 6 / NT)
        W4_REQUEST_B(bq7, 7 % NT, 7 / NT)
    }
    if constexpr (!PRE && !GEN) {
        __syncthreads();  // tables written
        W4_REQUEST_V(0, 0, 0)
        W4_REQUEST_V(0, 0, 1)
    }
    if constexpr (R == 9) {
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(bq0.bh), "+v"(bq0.bl), "+v"(bq1.bh), "+v"(bq1.bl), "+v"(bq2.bh), "+v"(bq2.bl), "+v"(bq3.bh),
                       "+v"(bq3.bl), "+v"(bq4.bh), "+v"(bq4.bl), "+v"(bq5.bh), "+v"(bq5.bl), "+v"(bq6.bh), "+v"(bq6.bl),
                       "+v"(bq7.bh), "+v"(bq7.bl)
                     :
                     : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(bq0.bh), "+v"(bq0.bl), "+v"(bq1.bh), "+v"(bq1.bl), "+v"(bq2.bh), "+v"(bq2.bl), "+v"(bq3.bh),
                       "+v"(bq3.bl), "+v"(bq4.bh), "+v"(bq4.bl)
                     :
                     : "memory");
    }
    __syncthreads();
    W4_STAMP(PRE ? 3 : 1)
    W4_LOAD_A(a0, 0, 0)
#ifdef W4_TAPTIME
    unsigned* tt_lds = reinterpret_cast<unsigned*>(smem + 150 * 1024) + ((PRE ? 8 : 0) + wave) * 36;
    unsigned* tt_cnt = tt_lds + 18;
    if (lane < 36) tt_lds[lane] = 0;
    unsigned long long tt_prev = __builtin_readcyclecounter();
#endif

    // Tap U of a chunk pair.  Program order of a tap: [V half-request of the next chunk (taps 0, 1)] [chunk barrier (last tap)]
    // [wait for this tap's weights] [MFMAs, between them: next tap's A operands, then the weight request of tap U + R - 1].
    // Younger than the weight request of tap U (issued in the middle of tap U - R + 1): the weight requests of taps
    // U-R+2 .. U-1 (2 (R-2) loads) and the V half-requests (VH loads each) of every chunk's taps 0 and 1 among taps
    // U-R+2 .. U.  At a chunk's last tap the next chunk's brick must have landed: younger than its second half-request (start
    // of tap VT1) are the weight requests of taps VT1 .. NT-2.
#define W4_TAP(U, ACUR, ANXT, BCUR, BREQ)                                                                            \
    {                                                                                                                \
        constexpr int cp_ = (U) / NT, t_ = (U) % NT;                                                                 \
        constexpr int un_ = (U) + R - 1, cn_ = un_ / NT, tn_ = un_ % NT;                                             \
        constexpr int nb_ = 2 * (R - 2) + VH0 * w4_count(t_, R - 1, NT, 0) + VH1 * w4_count(t_, R - 1, NT, VT1);  \
        W4_TT(U)                                                                                                     \
        if constexpr (W4_PRIO && (t_ == 0 || w4_prio(t_, NT) != w4_prio(t_ - 1, NT)))                                \
            __builtin_amdgcn_s_setprio(w4_prio(t_, NT));                                                             \
        if constexpr (WM >= 2) asm volatile("" : "+v"(arow[0]), "+v"(arow[1]), "+v"(arow[WM - 2]), "+v"(arow[WM - 1])); \
        else asm volatile("" : "+v"(arow[0]));                                                                       \
        if constexpr (t_ == 0)                                                                                       \
            W4_REQUEST_V(ch + cp_ + 1, 1 - cp_, 0)                                                                   \
        if constexpr (t_ == VT1)                                                                                     \
            W4_REQUEST_V(ch + cp_ + 1, 1 - cp_, 1)                                                                   \
        if constexpr (t_ == NT - 1) {                                                                                \
            W4_WAIT_VM(2 * (NT - 1 - VT1))                                                                           \
            __syncthreads();                                                                                         \
        }                                                                                                            \
        W4_WAIT_B(BCUR, nb_)                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                           \
        if constexpr (t_ < NT - 1) W4_MFMA_SPREAD(ACUR, BCUR, t_, ANXT, t_ + 1, cp_, BREQ, tn_, ch + cn_)            \
        else W4_MFMA_SPREAD(ACUR, BCUR, t_, ANXT, 0, 1 - cp_, BREQ, tn_, ch + cn_)                                   \
    }
#define W4_TAP6(U0)                                                                                                  \
    {                                                                                                                \
        W4_TAP((U0) + 0, a0, a1, bq0, bq5)                                                                           \
        W4_TAP((U0) + 1, a1, a0, bq1, bq0)                                                                           \
        W4_TAP((U0) + 2, a0, a1, bq2, bq1)                                                                           \
        W4_TAP((U0) + 3, a1, a0, bq3, bq2)                                                                           \
        W4_TAP((U0) + 4, a0, a1, bq4, bq3)                                                                           \
        W4_TAP((U0) + 5, a1, a0, bq5, bq4)                                                                           \
    }
#define W4_TAP18R9()                                                                                                 \
    {                                                                                                                \
        W4_TAP(0, a0, a1, bq0, bq8)                                                                                  \
        W4_TAP(1, a1, a0, bq1, bq0)                                                                                  \
        W4_TAP(2, a0, a1, bq2, bq1)                                                                                  \
        W4_TAP(3, a1, a0, bq3, bq2)                                                                                  \
        W4_TAP(4, a0, a1, bq4, bq3)                                                                                  \
        W4_TAP(5, a1, a0, bq5, bq4)                                                                                  \
        W4_TAP(6, a0, a1, bq6, bq5)                                                                                  \
        W4_TAP(7, a1, a0, bq7, bq6)                                                                                  \
        W4_TAP(8, a0, a1, bq8, bq7)                                                                                  \
        W4_TAP(9, a1, a0, bq0, bq8)                                                                                  \
        W4_TAP(10, a0, a1, bq1, bq0)                                                                                 \
        W4_TAP(11, a1, a0, bq2, bq1)                                                                                 \
        W4_TAP(12, a0, a1, bq3, bq2)                                                                                 \
        W4_TAP(13, a1, a0, bq4, bq3)                                                                                 \
        W4_TAP(14, a0, a1, bq5, bq4)                                                                                 \
        W4_TAP(15, a1, a0, bq6, bq5)                                                                                 \
        W4_TAP(16, a0, a1, bq7, bq6)                                                                                 \
        W4_TAP(17, a1, a0, bq8, bq7)                                                                                 \
    }
    for (int ch = 0; ch < a.nchunk; ch += 2) {
        if constexpr (R == 9) {
            W4_TAP18R9()
        } else {
            W4_TAP6(0)
            if constexpr (NT >= 6) W4_TAP6(6)
        }
    }
    if constexpr (W4_PRIO) __builtin_amdgcn_s_setprio(0);
    // the stream's harmless last requests (LDS-DMA included) must land before LDS and the ring's registers are reused
    if constexpr (R == 9) {
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(bq0.bh), "+v"(bq0.bl), "+v"(bq1.bh), "+v"(bq1.bl), "+v"(bq2.bh), "+v"(bq2.bl), "+v"(bq3.bh),
                       "+v"(bq3.bl), "+v"(bq4.bh), "+v"(bq4.bl), "+v"(bq5.bh), "+v"(bq5.bl), "+v"(bq6.bh), "+v"(bq6.bl),
                       "+v"(bq7.bh), "+v"(bq7.bl), "+v"(bq8.bh), "+v"(bq8.bl)
                     :
                     : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)"
                     : "+v"(bq0.bh), "+v"(bq0.bl), "+v"(bq1.bh), "+v"(bq1.bl), "+v"(bq2.bh), "+v"(bq2.bl), "+v"(bq3.bh),
                       "+v"(bq3.bl), "+v"(bq4.bh), "+v"(bq4.bl), "+v"(bq5.bh), "+v"(bq5.bl)
                     :
                     : "memory");
    }
#ifdef W4_TAPTIME
    if (lane < 18) {
        atomicAdd(&w4_tt[(((PRE ? 8 : 0) + wave) * 18 + lane) * 2], (unsigned long long)tt_lds[lane]);
        atomicAdd(&w4_tt[(((PRE ? 8 : 0) + wave) * 18 + lane) * 2 + 1], (unsigned long long)tt_cnt[lane]);
    }
#endif
#undef W4_BLDS
#undef W4_REQUEST_V
#undef W4_LOAD_A
#undef W4_ADDR_A
#undef W4_READ_A
#undef W4_IS_DEAD
#undef W4_MFMA_SPREAD
#undef W4_REQUEST_B
#undef W4_WAIT_B
#undef W4_WAIT_VM
#undef W4_TAP
#undef W4_TAP6
#undef W4_TAP18R9
}

// Workgroup -> (brick, channel tile, frame parity).  All workgroups that read the same V brick (channel tiles, frame
// parities) take consecutive slots of ONE XCD (workgroup i runs on XCD i % 8).  Which bricks an XCD gets decides what its 4 MB L2
// can share between them (every brick re-reads a t-halo of 2 / TT and an h-halo of 2 / TH of its rows):
//   order 0  XCD x owns the flat brick indices x, x + 8, ... (bj fastest, then bh): one w-column and every SECOND bh -- the
//            h-neighbours of a brick always sit on another XCD;
//   order 1  XCD x owns whole (sample, w-column) columns x, x + 8, ...; inside a column bh runs fastest, then bt: the ~16
//            bricks an XCD has in flight form a contiguous (t, h) slab whose inner halos are shared through its L2;
//   order 2  the same with bt fastest.
struct W4Brick { int par, ntile, b0, t0, h0, j0; };

template <int BN>
__host__ __device__ __forceinline__ W4Brick w4_decode(const W4Args& a, int v) {
    const int nNt = a.CoutPad / BN;
    const int npar = a.tdup ? 2 : 1;
    const int per_brick = nNt * npar;
    const int nbrick = a.nvirt / per_brick;
    int par, ntile, b0, bt, bh, bj;
    if ((nbrick & 7) == 0) {
        const int xcd = v & 7, slot = v >> 3;
        const int sub = slot % per_brick, q = slot / per_brick;   // q: this XCD's q-th brick
        par = a.tdup ? sub & 1 : 0;
        ntile = a.tdup ? sub >> 1 : sub;
        const int ncol = a.B * a.nbJ;
        if (a.order && (ncol & 7) == 0) {
            const int bpc = a.nbT * a.nbH;
            const int colq = q / bpc, r = q - colq * bpc;
            const int col = colq * 8 + xcd;
            b0 = col / a.nbJ; bj = col - b0 * a.nbJ;
            if (a.order == 1) { bt = r / a.nbH; bh = r - bt * a.nbH; }
            else { bh = r / a.nbT; bt = r - bh * a.nbT; }
        } else {
            int brick = q * 8 + xcd;
            bj = brick % a.nbJ; brick /= a.nbJ;
            bh = brick % a.nbH; brick /= a.nbH;
            bt = brick % a.nbT; b0 = brick / a.nbT;
        }
    } else {
        par = a.tdup ? (int)(v >= (a.nvirt >> 1)) : 0;
        int brick = a.tdup ? v % (a.nvirt >> 1) : v;
        ntile = brick % nNt; brick /= nNt;
        bj = brick % a.nbJ; brick /= a.nbJ;
        bh = brick % a.nbH; brick /= a.nbH;
        bt = brick % a.nbT; b0 = brick / a.nbT;
    }
    return W4Brick{par, ntile, b0, bt * a.TT, bh * a.TH, bj * 4};
}

// index tables of one brick: gposA [1024] (planes 0..3), gposB [1024] (planes 4, 5 in rows 0..511, padding behind),
// tpos [128] (output position of a tile's first column), tres [128][4] (residual rows of the tile's four columns).
// gpos: V rows relative to the brick's sample, W4_PAD_ROW for zero padding (the buffer-descriptor requests of w4_pass)
template <int KT, int NTH>
__device__ __forceinline__ void w4_tables(const W4Args& a, const W4Brick& k, int* gposA, int tid) {
    constexpr int ROWS_A = W4Geo<NTH>::ROWS_A, TILES = W4Geo<NTH>::TILES;
    int* gposB = gposA + ROWS_A;
    int* tpos = gposB + ROWS_A;
    int* tres = tpos + TILES;
    const int pt = a.tdup ? 1 - k.par : KT / 2;
    const int HT = a.TT + KT - 1, HH = a.TH + 2;
    const int plane = HT * HH * 4;        // (TJ = 4 tiles along w in every brick of this kernel)
    if (tid < TILES) {
        int m = tid;
        const int ij = m & 3; m >>= 2;       // (no integer divisions in the index tables: they cost a workgroup ~1.5 us)
        const int ih = m & (a.TH - 1); m >>= a.th_shift;
        const int t = k.t0 + m, h = k.h0 + ih, w = 4 * (k.j0 + ij);
        const int To = a.tdup ? 2 * a.T : a.T, to = a.tdup ? 2 * t + k.par : t;
        tpos[tid] = ((k.b0 * To + to) * a.H + h) * a.W + w;
        const int rbase = ((k.b0 * (To >> a.rt_shift) + (to >> a.rt_shift)) * (a.H >> a.rs_shift) + (h >> a.rs_shift)) * (a.W >> a.rs_shift);
#pragma unroll
        for (int c = 0; c < 4; ++c) tres[4 * tid + c] = rbase + ((w + c) >> a.rs_shift);
    }
    for (int r = tid; r < 2 * ROWS_A; r += NTH) {
        const bool pb = r >= ROWS_A;                    // row of pass B's brick
        const int rr = pb ? r - ROWS_A : r;
        const int x = (rr >= plane) + (rr >= 2 * plane) + (rr >= 3 * plane) + (rr >= 4 * plane);   // (>= 4: not a row of the brick)
        int q = rr - x * plane;
        const int ij = q & 3; q >>= 2;
        const int qh = (int)(((unsigned)q * (unsigned)a.hh_magic) >> 20);   // q / HH
        const int ih = q - qh * HH; q = qh;
        const int t = k.t0 + q - pt, h = k.h0 + ih - 1, j = k.j0 + ij;
        const bool ok = x < (pb ? 2 : 4) && (unsigned)t < (unsigned)a.T && (unsigned)h < (unsigned)a.H;
        const int xg = pb ? 4 + x : x;
        (pb ? gposB : gposA)[rr] = ok ? (((t * a.nchunk * 6 + xg) * a.H + h) * a.J + j) : W4_PAD_ROW;   // chunk 0; 64-byte rows
    }
}

constexpr int W4_TABLE_BYTES = w4_table_bytes<512>();   // the index tables of the 512-thread kernels

// NT: (kt, kh) taps: 9 = 3x3x3, 6 = temporal-duplication pair kernels (2x3x3), 3 = one time slice (1x3x3: Conv2d).
// BN: output channels per workgroup.  64: as described above.  32 (layers with 32 output channels): pass A wave = (plane,
// tile half) with 2 row blocks, pass B wave = (plane, tile quarter) with 1 row block.
// NTH: threads per workgroup (W4Geo): 512, or 256 = the 32-channel kernel as two workgroups per CU.
#define W4K_NAME conv_wino4_f16x3_kernel
#define W4K_ONE false
#include "i2v_conv16w4_kernel.h"


// brick of `tiles` (128: 512-thread kernels, 64: 256-thread kernels) = TT frames x TH rows x 4 tiles (16 output positions); rows_a /
// rows_b: V rows one buffer of pass A / pass B can stage
inline bool wino4_tiling(int T, int H, int W, int KT, int* TT_, int* TH_, int tiles = W4_TILES, int rows_a = W4_ROWS_A, int rows_b = W4_ROWS_A / 2 - 16) {
    if (T < 1 || (T < 2 && KT != 1) || W % 16 || H < 8) return false;
    int TT = 1;
    while (TT < 4 && T % (TT * 2) == 0) TT *= 2;
    const int TH = tiles / (TT * 4);
    if (TH < 4 || TH > H || H % TH || TH * 4 % 16) return false;       // (16 consecutive tiles = 16 consecutive V rows: conflict-free ds_read_b128)
    if (4 * (TT + KT - 1) * (TH + 2) * 4 > rows_a) return false;       // pass A's halo brick
    if (2 * (TT + KT - 1) * (TH + 2) * 4 > rows_b) return false;       // pass B's (the 512-thread kernels' buffer keeps 16 rows free)
    *TT_ = TT; *TH_ = TH;
    return true;
}


// ---- the launch plan (i2v_conv16w4.hip): every host-side decision about a launch of one of the F(4,3) kernels, made once
// Measurement switches (see w4_switches in i2v_conv16w4.hip: the production library always runs the defaults)
struct W4Switches { int bn = 0, order = W4_DEFAULT_ORDER, nth = 0, trace = 0, tskip = 1; };
// Which kernel runs the plan: the split / one-term kernels (i2v_conv16w4.hip / i2v_conv16w4h.hip), the operand-generating kernel
// (i2v_conv16w4g.hip), the split and one-term kernels that skip temporal edge units (i2v_conv16w4e.hip)
// (the values are what the launch trace prints and tests/f43_tskip_worker.py reads: they stay what they were)
enum W4Form : int { W4_SPLIT = 0, W4_ONE = 1, W4_GEN = 6, W4_EDGE = 7, W4_EDGE_ONE = 8 };
struct W4Plan {
    W4Args a;             // everything but the pointers in / wp / bias / res / out / stats, which the caller sets
    int NT, BN, NTH;      // the kernel instantiation: (kt, kh) taps, channels and threads per workgroup
    W4Form form;
    unsigned grid;
    size_t lds_bytes;
    double issued;        // share of the full tap loops' MFMAs this launch issues (< 1: form W4_EDGE, see w4_dead_units)
};
// T = OUTPUT frames.  cus: compute units of the device.  gen: the plan of the operand-generating kernel (fixed 4 x 8 brick, 32
// channels per workgroup, no V tensor: wino4g_forward has checked its own preconditions).  Returns an error code and sets the error.
int wino4_plan(W4Plan* p, const Wino4Weights& wts, int B, int T, int H, int W, bool has_res, int rt, int rs, int epi, bool has_stats, int cus,
               const W4Switches& sw, bool gen = false);
// what the other two translation units export: the launch of a plan on their kernels
int wino4h_launch(const W4Plan& p, hipStream_t st);          // form W4_ONE
int wino4e_launch(const W4Plan& p, hipStream_t st);          // forms W4_EDGE / W4_EDGE_ONE
// key of the one switch over instantiations each translation unit has
constexpr int w4_key(int NT, int BN, int NTH) { return (NT * 128 + BN) * 1024 + NTH; }
constexpr int W4G_THREADS = 768;   // the 12-wave workgroup of i2v_conv16w4g.hip

}  // namespace i2v
