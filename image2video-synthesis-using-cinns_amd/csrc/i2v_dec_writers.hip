// Operand writers of the decoder's block convs and the range guard of the split-fp16 formats (see i2v_dec_writers.h).
#include <algorithm>
#include <type_traits>

#include "i2v_dec_writers.h"

namespace i2v {

// out[b][t][h][w][c] = act( (x[b][t/ut][h/us][w/us][c] * A + B) * gamma'[b][h][w][c] + beta[b][h][w][c] )
//   gb: [B][H][W][2C] (gamma' = 1 + gamma in [0,C), beta in [C,2C)) or null.
// One thread = one (h, w) position x 8 channels (consecutive threads = consecutive channel groups), looping over the
// frames: the per-(sample, channel) coefficients and the SPADE gamma/beta of the position -- neither depends on t -- are
// loaded once and reused for all T frames, the source row once per `ut` frames; per frame 32 B are stored.
// blockIdx.y = sample, all per-sample index math in 32 bits.  HL16: write the split-fp16 operand format of
// i2v_conv16.hip (8 x fp16 hi | 8 x fp16 lo per 8 channels, lo = x - hi) instead of fp32.
// SH (every SPADE-consuming writer below has it): gk consecutive samples share one start frame (i2v_dec_forward_realizations), sample b
// reads the map row (gr0 + b) / gk of gb, gr0 = the realization index of the launch's first sample.  SH = false: row b.
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void publish_umax(int* slot, float m) {
    if (!slot) return;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) {
        const int bits = __float_as_int(m);   // m >= 0: the integer order of the bit patterns is the float order
        if (bits > *reinterpret_cast<volatile int*>(slot)) atomicMax(slot, bits);
    }
}

__global__ void status_finish_kernel(int* __restrict__ status) {
    int f = 0;
    for (int i = 1; i < I2V_STATUS_SNAP; ++i) {
        const int v = status[i];
        if (v != 0 && __int_as_float(v) < I2V_UNDERFLOW_MAX) f = 2;
        status[I2V_STATUS_SNAP + i] = v;   // kept for the host (mma = auto decides per layer from these)
        status[i] = 0;
    }
    if (f) atomicOr(status, f);
}

template <bool HL16, bool SH = false>
__global__ __launch_bounds__(256) void modulate_kernel(const float* __restrict__ x, const float2* __restrict__ coef,
                                                       const float* __restrict__ gb, float* __restrict__ out, int T, int H,
                                                       int W, int C, int ut, int us, int lrelu, int* __restrict__ range_flag,
                                                       int* __restrict__ umax, int gk = 1, int gr0 = 0) {
    const int C8 = C >> 3;
    const int b = blockIdx.y;
    const int per = H * W * C8;  // threads per sample
    bool bad = false;  // HL16: a value left the fp16 range of the hi part (sticky flag, see i2v_dec_status)
    float vmax = 0.f;  // HL16: largest |activation| written (underflow guard)
    const int Hl = H / us, Wl = W / us, Tl = T / ut;
    const float2* cp0 = coef + (long)b * C;
    const float* xb = x + (long)b * Tl * Hl * Wl * C;
    const float* gbb = gb ? gb + (long)(SH ? (gr0 + b) / gk : b) * H * W * 2 * C : nullptr;
    char* ob = reinterpret_cast<char*>(out) + (long)b * T * per * 32;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
        const int c8 = i % C8;
        int p = i / C8;
        const int w = p % W;
        const int h = p / W;
        float ca[8], cb[8];  // norm(x) == x * ca + cb
        {
            const float4* cp = reinterpret_cast<const float4*>(cp0 + 8 * c8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 ab = cp[j];
                ca[2 * j] = ab.x; cb[2 * j] = ab.y; ca[2 * j + 1] = ab.z; cb[2 * j + 1] = ab.w;
            }
        }
        if (gbb) {  // fold SPADE's gamma / beta into the affine: (x ca + cb) ga + be
            const float* g = gbb + ((long)h * W + w) * (2 * C) + 8 * c8;
            const float4 g0 = *reinterpret_cast<const float4*>(g), g1 = *reinterpret_cast<const float4*>(g + 4);
            const float4 e0 = *reinterpret_cast<const float4*>(g + C), e1 = *reinterpret_cast<const float4*>(g + C + 4);
            const float ga[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float be[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) { cb[j] = fmaf(cb[j], ga[j], be[j]); ca[j] = ca[j] * ga[j]; }
        }
        const float* xp0 = xb + ((long)(h / us) * Wl + w / us) * C + 8 * c8;
        const long xstride = (long)Hl * Wl * C;
        float r0[8];
        for (int t = 0; t < T; ++t) {
            if (t % ut == 0) {
                const float* xp = xp0 + (long)(t / ut) * xstride;
                const float4 v0 = *reinterpret_cast<const float4*>(xp), v1 = *reinterpret_cast<const float4*>(xp + 4);
                r0[0] = v0.x; r0[1] = v0.y; r0[2] = v0.z; r0[3] = v0.w; r0[4] = v1.x; r0[5] = v1.y; r0[6] = v1.z; r0[7] = v1.w;
            }
            float r[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                r[j] = fmaf(r0[j], ca[j], cb[j]);
                if (lrelu) r[j] = r[j] >= 0.f ? r[j] : 0.2f * r[j];
            }
            char* o = ob + ((long)t * per + i) * 32;
            if (HL16) {
                half8_t hi, lo;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const _Float16 hh = (_Float16)r[j];
                    bad |= !(fabsf(r[j]) <= 65504.f);
                    vmax = fmaxf(vmax, fabsf(r[j]));
                    hi[j] = hh;
                    lo[j] = (_Float16)(r[j] - (float)hh);
                }
                *reinterpret_cast<half8_t*>(o) = hi;
                *reinterpret_cast<half8_t*>(o + 16) = lo;
            } else {
                *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
                *reinterpret_cast<float4*>(o + 16) = make_float4(r[4], r[5], r[6], r[7]);
            }
        }
    }
    if (HL16 && bad && range_flag) atomicOr(range_flag, 1);
    if (HL16) publish_umax(umax, vmax);
}

// The same modulation, written as the Winograd-transformed operand V = B^T d of i2v_conv16w.hip:
//   V[b][t][c/16][x][h][j][c%16]  (hl16: per 8 channels 8 x fp16 hi | 8 x fp16 lo),  j = output pair (w = 2j, 2j+1),
//   V0 = d0 - d2, V1 = d1 + d2, V2 = d2 - d1, V3 = d1 - d3,  d_k = act(...)[t][h][2j-1+k]  (0 outside the row).
// One thread = one (h, j, 8-channel group), looping over the frames like modulate_kernel.  It evaluates only its OWN two
// positions (d1, d2); d0 and d3 are the neighbouring pairs' d2 / d1 and arrive by lane shuffle: thread order = channel
// group within a 32-channel (128-byte) input line fastest, then j, so lane l +- 4 holds pair j +- 1 of the same channels.
// Only the first / last pair of a 16-pair wave segment evaluates its outer neighbour itself.  (Evaluating all four
// positions per thread read every input twice: 9.1 GB instead of 5.5 GB per BAIR step.)
struct ModPos {   // affine of one position: act(x * a + b), and its source row
    float a[8], b[8];
    const float* xp;
};

__device__ __forceinline__ void mod_pos_init(ModPos& m, const float* ca, const float* cb, const float* xb, const float* gbb, int h, int w,
                                             int W, int C, int c8, int us, int Wl) {
    m.xp = xb + ((long)(h / us) * Wl + w / us) * C + 8 * c8;
    if (gbb) {  // fold SPADE's gamma' / beta of the position into the affine: (x ca + cb) ga + be
        const float* g = gbb + ((long)h * W + w) * (2 * C) + 8 * c8;
        const float4 g0 = *reinterpret_cast<const float4*>(g), g1 = *reinterpret_cast<const float4*>(g + 4);
        const float4 e0 = *reinterpret_cast<const float4*>(g + C), e1 = *reinterpret_cast<const float4*>(g + C + 4);
        const float ga[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        const float be[8] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) { m.b[c] = fmaf(cb[c], ga[c], be[c]); m.a[c] = ca[c] * ga[c]; }
    } else {
#pragma unroll
        for (int c = 0; c < 8; ++c) { m.a[c] = ca[c]; m.b[c] = cb[c]; }
    }
}

__device__ __forceinline__ void mod_pos_eval(const ModPos& m, long toff, int lrelu, float* d, float& vmax) {
    const float* p = m.xp + toff;
    const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + 4);
    const float r0[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float r = fmaf(r0[c], m.a[c], m.b[c]);
        d[c] = (lrelu && r < 0.f) ? 0.2f * r : r;
        vmax = fmaxf(vmax, fabsf(d[c]));
    }
}

template <bool SH = false>
__global__ __launch_bounds__(256) void modulate_wino_kernel(const float* __restrict__ x, const float2* __restrict__ coef,
                                                            const float* __restrict__ gb, char* __restrict__ out, int T, int H,
                                                            int W, int C, int ut, int us, int lrelu, int* __restrict__ range_flag,
                                                            int* __restrict__ umax, int gk = 1, int gr0 = 0) {
    bool bad = false;
    float vmax = 0.f;
    const int C8 = C >> 3, J = W >> 1;
    const int b = blockIdx.y;
    // Thread = (h, chunk, j, piece p): piece p of a 64-byte V row is [hi | lo] (p & 1) of the 8 channels c8 = 2 chunk + (p >> 1).
    // The hi and the lo lane of a channel group compute the same values (the x loads coalesce; the kernel is HBM-bound),
    // so that every store instruction of a wave writes 16 whole rows = 1 KB contiguous.
    const int per = H * J * C8 * 2;  // threads per sample (a multiple of 64: whole waves stay active for the shuffles)
    const int Hl = H / us, Wl = W / us, Tl = T / ut;
    const float2* cp0 = coef ? coef + (long)b * C : nullptr;   // null: identity (the kernel then only formats the operand)
    const float* xb = x + (long)b * Tl * Hl * Wl * C;
    const float* gbb = gb ? gb + (long)(SH ? (gr0 + b) / gk : b) * H * W * 2 * C : nullptr;
    const int nchunk = C >> 4;
    const long xstride = (long)Hl * Wl * C;
    const int lane = threadIdx.x & 63, jj = lane >> 2;   // jj: position of the pair inside the wave's 16-pair segment
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
        // i = ((h * nchunk + chunk) * J + j) * 4 + p
        const int p = i & 3;
        int q = i >> 2;
        const int j = q % J; q /= J;
        const int chunk = q % nchunk;
        const int h = q / nchunk;
        const int c8 = chunk * 2 + (p >> 1);
        const bool is_lo = p & 1;
        float ca[8], cb[8];
        if (cp0) {
            const float4* cp = reinterpret_cast<const float4*>(cp0 + 8 * c8);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 ab = cp[k];
                ca[2 * k] = ab.x; cb[2 * k] = ab.y; ca[2 * k + 1] = ab.z; cb[2 * k + 1] = ab.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) { ca[k] = 1.f; cb[k] = 0.f; }
        }
        // own positions w = 2j, 2j + 1; the outer neighbours 2j - 1 / 2j + 2 come from lane -+ 4 unless this pair opens /
        // closes the wave's segment (then they are evaluated here) or the row (then they are 0: the conv's zero padding)
        ModPos m1, m2, me;
        mod_pos_init(m1, ca, cb, xb, gbb, h, 2 * j, W, C, c8, us, Wl);
        mod_pos_init(m2, ca, cb, xb, gbb, h, 2 * j + 1, W, C, c8, us, Wl);
        const bool left_row = j == 0, right_row = j == J - 1;
        const bool left_own = !left_row && jj == 0, right_own = !right_row && jj == 15;
        if (left_own || right_own)   // (an edge pair is never both: J >= 4 keeps jj == 0 and jj == 15 apart unless J >= 16)
            mod_pos_init(me, ca, cb, xb, gbb, h, left_own ? 2 * j - 1 : 2 * j + 2, W, C, c8, us, Wl);
        const bool both_own = left_own && right_own;   // impossible (jj is 0 or 15), kept for clarity
        (void)both_own;
        float d0[8], d1[8], d2[8], d3[8], de[8];
        // V row of (t, chunk, x, h, j): 64 bytes; this thread owns its 16-byte piece p
        char* ob = out + ((((long)b * T * nchunk + chunk) * 4 * H + h) * J + j) * 64 + p * 16;
        const long ostride_x = (long)H * J * 64, ostride_t = (long)nchunk * 4 * ostride_x;
        for (int t = 0; t < T; ++t) {
            if (t % ut == 0) {
                const long toff = (long)(t / ut) * xstride;
                mod_pos_eval(m1, toff, lrelu, d1, vmax);
                mod_pos_eval(m2, toff, lrelu, d2, vmax);
                if (left_own || right_own) mod_pos_eval(me, toff, lrelu, de, vmax);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float up = __shfl_up(d2[c], 4), dn = __shfl_down(d1[c], 4);
                    d0[c] = left_row ? 0.f : (left_own ? de[c] : up);
                    d3[c] = right_row ? 0.f : (right_own ? de[c] : dn);
                }
            }
            char* o = ob + (long)t * ostride_t;
#pragma unroll
            for (int xq = 0; xq < 4; ++xq) {
                half8_t piece;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float v = xq == 0 ? d0[c] - d2[c] : xq == 1 ? d1[c] + d2[c] : xq == 2 ? d2[c] - d1[c] : d1[c] - d3[c];
                    const _Float16 hh = (_Float16)v;
                    bad |= !(fabsf(v) <= 65504.f);
                    piece[c] = is_lo ? (_Float16)(v - (float)hh) : hh;
                }
                *reinterpret_cast<half8_t*>(o + xq * ostride_x) = piece;
            }
        }
    }
    if (bad && range_flag) atomicOr(range_flag, 1);
    publish_umax(umax, vmax);
}

// The operand of the F(4,3) kernel (i2v_conv16w4.hip): V[b][t][c/16][x][h][j][c%16], x = 0..5, j = tile of four output
// positions (w = 4j .. 4j+3), d_k = act(...)[t][h][4j-1+k]:
//   V0 = 4 d0 - 5 d2 + d4   V1 = -4 d1 - 4 d2 + d3 + d4   V2 = 4 d1 - 4 d2 - d3 + d4
//   V3 = -2 d1 - d2 + 2 d3 + d4   V4 = 2 d1 - d2 - 2 d3 + d4   V5 = 4 d1 - 5 d3 + d5
// Same thread mapping as modulate_wino_kernel: one thread = one 16-byte piece of the V rows of one (h, tile) column; it
// evaluates its OWN four positions (d1..d4), gets d0 / d5 from the neighbouring tiles by lane shuffle and loops over the frames.
// Thread = (h, chunk, tile j, q): the FOUR channels 4q .. 4q+3 of the chunk, hi AND lo parts.  (Round 3 gave a lane 8 channels of
// the hi OR the lo part: every value was loaded, evaluated and kept twice -- 215 VGPRs and scratch; now every element is loaded and
// evaluated once.)  Per plane the thread holds two 8-byte half-pieces: hi at byte (q >> 1) * 32 + (q & 1) * 8 of the 64-byte row, lo
// 16 bytes behind.  They leave as ONE 16-byte piece after an exchange with the other lane of the pair: see MOD4_FORM below.
// GB: SPADE's gamma' / beta are present -- every position then has its own affine (a, b)[4], kept in registers over the frame loop;
// without them (the ADAIN operand of conv_1, SPADE's own activation) all positions share the sample's (ca, cb).
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

template <bool GB>
struct ModPos4 {
    float a[GB ? 4 : 1], b[GB ? 4 : 1];
    const float* xp;
};

template <bool GB>
__device__ __forceinline__ void mod_pos4_init(ModPos4<GB>& m, const float* ca, const float* cb, const float* xb, const float* gbb, int h, int w,
                                              int W, int C, int c4, int us, int Wl) {
    m.xp = xb + ((long)(h / us) * Wl + w / us) * C + 4 * c4;
    if constexpr (GB) {  // fold SPADE's gamma' / beta of the position into the affine: (x ca + cb) ga + be
        const float* g = gbb + ((long)h * W + w) * (2 * C) + 4 * c4;
        const float4 g0 = *reinterpret_cast<const float4*>(g), e0 = *reinterpret_cast<const float4*>(g + C);
        const float ga[4] = {g0.x, g0.y, g0.z, g0.w};
        const float be[4] = {e0.x, e0.y, e0.z, e0.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) { m.b[c] = fmaf(cb[c], ga[c], be[c]); m.a[c] = ca[c] * ga[c]; }
    }
}

// the position's four channels of the frame at `toff`, as they lie in memory
template <bool GB>
__device__ __forceinline__ float4 mod_pos4_load(const ModPos4<GB>& m, long toff) {
#ifdef MOD_NT   // measurement build: the writer's reads and writes are pure streams
    typedef float f4v_ __attribute__((ext_vector_type(4)));
    const f4v_ v0 = __builtin_nontemporal_load(reinterpret_cast<const f4v_*>(m.xp + toff));
    return make_float4(v0.x, v0.y, v0.z, v0.w);
#else
    return *reinterpret_cast<const float4*>(m.xp + toff);
#endif
}

template <bool GB>
__device__ __forceinline__ void mod_pos4_eval(const ModPos4<GB>& m, const float* ca, const float* cb, const float4 v0, int lrelu, float* d,
                                              float& vmax) {
    const float r0[4] = {v0.x, v0.y, v0.z, v0.w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float r = GB ? fmaf(r0[c], m.a[c], m.b[c]) : fmaf(r0[c], ca[c], cb[c]);
        d[c] = (lrelu && r < 0.f) ? 0.2f * r : r;
        vmax = fmaxf(vmax, fabsf(d[c]));
    }
}

// Plane XQ of B^T d for the thread's four channels: hi = (half)v, lo = (half)(v - (float)hi); bad: |v| > 65504 or not finite.
template <int XQ>
__device__ __forceinline__ void mod4_plane(const float* d0, const float* d1, const float* d2, const float* d3, const float* d4,
                                           const float* d5, half4_t& ph, half4_t& pl, bool& bad) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v;
        if (XQ == 0) v = fmaf(4.f, d0[c], fmaf(-5.f, d2[c], d4[c]));
        else if (XQ == 1) v = fmaf(-4.f, d1[c] + d2[c], d3[c] + d4[c]);
        else if (XQ == 2) v = fmaf(4.f, d1[c] - d2[c], d4[c] - d3[c]);
        else if (XQ == 3) v = fmaf(2.f, d3[c] - d1[c], d4[c] - d2[c]);
        else if (XQ == 4) v = fmaf(2.f, d1[c] - d3[c], d4[c] - d2[c]);
        else v = fmaf(4.f, d1[c], fmaf(-5.f, d3[c], d5[c]));
        // v is rounded to fp32 first, as a value of its own: without this the compiler may merge the last fmaf and the conversion into
        // one v_fma_mixlo_f16, which rounds once -- another hi part in rare cases (the lo part's difference is exact either way)
        asm("" : "+v"(v));
        const _Float16 hh = (_Float16)v;
        bad |= !(fabsf(v) <= 65504.f);
        ph[c] = hh;
        pl[c] = (_Float16)(v - (float)hh);
    }
}

// The 8 bytes `mine` of the other lane of the pair (lanes 2k, 2k + 1): DPP quad_perm [1, 0, 3, 2], no LDS.
__device__ __forceinline__ uint2 mod4_pair_swap(uint2 mine) {
    return make_uint2((unsigned)__builtin_amdgcn_update_dpp(0, (int)mine.x, 0xB1, 0xF, 0xF, false),
                      (unsigned)__builtin_amdgcn_update_dpp(0, (int)mine.y, 0xB1, 0xF, 0xF, false));
}

__device__ __forceinline__ uint2 mod4_bits(half4_t p) { return __builtin_bit_cast(uint2, p); }

// Stores of the writer, FORM bit 0.
//   0: every lane stores its own 8-byte half-pieces (two per plane in the split form): a wave instruction covers 1 KB with 8-byte
//      pieces and 8-byte holes.  The form up to round 6.
//   1: the two lanes of a pair first exchange 8 bytes, then every lane stores one whole 16-byte piece.  Split form: lane q4 stores
//      piece q4 of the 64-byte row (q4 even: its hi part + the neighbour's, odd: the neighbour's lo part + its own); a wave
//      instruction writes 1 KB contiguous, 6 instead of 12 stores per lane and frame.  One-term form: the even lane stores the
//      pair's piece of the planes 0, 2, 4, the odd lane that of the planes 1, 3, 5; 3 instead of 6 stores.
// Frame loop, FORM bit 1.
//   1: the float4 loads of the next input frame are requested before the transform and the stores of the current one.
// The bytes of V do not depend on FORM.  The production library holds form 1.  The measurement build holds 0, 1 and 3
// (I2V_MOD4_FORM); 3 measured no gain beyond its own noise on the 128 x 128 configs: profiles/writer_stores_ab.md.
#ifndef MOD4_FORM
#define MOD4_FORM 1
#endif

// A 16-byte piece to global memory (MOD_NT, a measurement build: non-temporal, like the 8-byte stores of form 0 there)
__device__ __forceinline__ void mod4_store16(char* p, uint4 v) {
#ifdef MOD_NT
    typedef unsigned u4v_ __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(u4v_{v.x, v.y, v.z, v.w}, reinterpret_cast<u4v_*>(p));
#else
    *reinterpret_cast<uint4*>(p) = v;
#endif
}

// ONE (mma = 3, the one-term operand of conv_wino4_f16_kernel, i2v_conv16w4h.hip): the same values, rounded to fp16 once -- exactly the
// hi parts the split writer stores -- into [B][T][CinPad/32][6][H][J][32 channels = 64 B], pieces c0-7 | c16-23 | c8-15 | c24-31 of the
// 32-channel chunk.  The thread mapping stays that of 16-channel chunks: chunk16 = 2 chunk32 + e writes the 8-byte half-piece
// (q >> 1) * 32 + e * 16 + (q & 1) * 8 of its row.  C is then CinPad: the chunks at and above the tensor's own channels (Cx) hold zeros.
// The range guard is the split writer's: bit 0 for |V| > 65504 or non-finite values, the maximum |activation| into the layer's slot.
template <bool GB, bool ONE = false, bool SH = false, int FORM = MOD4_FORM>
__attribute__((amdgpu_waves_per_eu(GB ? 3 : 4)))   // registers for 12 (SPADE maps held per position) / 16 waves per CU in every form
__global__ __launch_bounds__(256) void modulate_wino4_kernel(const float* __restrict__ x, const float2* __restrict__ coef,
                                                             const float* __restrict__ gb, char* __restrict__ out, int T, int H,
                                                             int W, int C, int ut, int us, int lrelu, int* __restrict__ range_flag,
                                                             int* __restrict__ umax, int Cx = 0, int gk = 1, int gr0 = 0) {
    constexpr bool ST16 = FORM & 1, AHEAD = FORM & 2;
    bool bad = false;
    float vmax = 0.f;
    if constexpr (!ONE) Cx = C;
    const int C4 = C >> 2, J = W >> 2;
    const int b = blockIdx.y;
    const int per = H * J * C4;        // threads per sample (a multiple of 64: whole waves stay active for the shuffles)
    const int Hl = H / us, Wl = W / us, Tl = T / ut;
    const float2* cp0 = coef ? coef + (long)b * Cx : nullptr;
    const float* xb = x + (long)b * Tl * Hl * Wl * Cx;
    const float* gbb = GB ? gb + (long)(SH ? (gr0 + b) / gk : b) * H * W * 2 * Cx : nullptr;
    const int nchunk = C >> 4;
    const long xstride = (long)Hl * Wl * Cx;
    const int lane = threadIdx.x & 63, jj = lane >> 2;   // jj: position of the tile inside the wave's 16-tile segment
    for (int i = blockIdx.x * 256 + threadIdx.x; i < per; i += gridDim.x * 256) {
        // i = ((h * nchunk + chunk) * J + j) * 4 + q
        // (workgroup = four chunks of one row.  Four rows of one chunk -- 4-8 KB contiguous writes per plane and frame instead of
        //  1-2 KB -- measured the same: profiles/r04_h_operand_writer_order.txt)
        const int q4 = i & 3;
        int q = i >> 2;
        const int j = q % J; q /= J;
        const int chunk = q % nchunk;
        const int h = q / nchunk;
        const int c4 = chunk * 4 + q4;
        // (ONE: the padding channels at and above Cx are zeros.  Their threads evaluate channel group 0 of the position -- values a
        //  live thread evaluates too, so the range guard sees nothing new -- and store zeros.)
        const bool live = !ONE || 4 * c4 < Cx;
        const int c4x = ONE && !live ? 0 : c4;
        float ca[4], cb[4];
        if (cp0) {
            const float4* cp = reinterpret_cast<const float4*>(cp0 + 4 * c4x);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float4 ab = cp[k];
                ca[2 * k] = ab.x; cb[2 * k] = ab.y; ca[2 * k + 1] = ab.z; cb[2 * k + 1] = ab.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { ca[k] = 1.f; cb[k] = 0.f; }
        }
        ModPos4<GB> m1, m2, m3, m4, me;
        mod_pos4_init<GB>(m1, ca, cb, xb, gbb, h, 4 * j, W, Cx, c4x, us, Wl);
        mod_pos4_init<GB>(m2, ca, cb, xb, gbb, h, 4 * j + 1, W, Cx, c4x, us, Wl);
        mod_pos4_init<GB>(m3, ca, cb, xb, gbb, h, 4 * j + 2, W, Cx, c4x, us, Wl);
        mod_pos4_init<GB>(m4, ca, cb, xb, gbb, h, 4 * j + 3, W, Cx, c4x, us, Wl);
        // own positions w = 4j .. 4j+3; the outer neighbours 4j - 1 / 4j + 4 come from lane -+ 4 unless this tile opens / closes the
        // wave's segment (then they are evaluated here) or the row (then they are 0: the conv's zero padding)
        const bool left_row = j == 0, right_row = j == J - 1;
        const bool left_own = !left_row && jj == 0, right_own = !right_row && jj == 15;
        me = m1;
        if (left_own || right_own) mod_pos4_init<GB>(me, ca, cb, xb, gbb, h, left_own ? 4 * j - 1 : 4 * j + 4, W, Cx, c4x, us, Wl);
        float d0[4], d1[4], d2[4], d3[4], d4[4], d5[4], de[4];
        // V row of (t, chunk, plane, h, j): 64 bytes [hi c0-7 | lo c0-7 | hi c8-15 | lo c8-15]; this thread's channels 4 q4 .. 4 q4 + 3
        const int nrow = ONE ? nchunk >> 1 : nchunk, crow = ONE ? chunk >> 1 : chunk;   // chunks of the V rows
        const bool odd = q4 & 1;
        const int piece = !ST16 ? (q4 >> 1) * 32 + (q4 & 1) * 8 + (ONE ? (chunk & 1) * 16 : 0)
                                : ONE ? (q4 >> 1) * 32 + (chunk & 1) * 16 : q4 * 16;
        const long ostride_x = (long)H * J * 64, ostride_t = (long)nrow * 6 * ostride_x;
        char* ob = out + ((((long)b * T * nrow + crow) * 6 * H + h) * J + j) * 64 + piece + (ST16 && ONE && odd ? ostride_x : 0);
        const bool edge = left_own || right_own;
        float4 r1, r2, r3, r4, re;
        auto request = [&](long toff) {   // the float4 loads of one input frame
            r1 = mod_pos4_load<GB>(m1, toff); r2 = mod_pos4_load<GB>(m2, toff); r3 = mod_pos4_load<GB>(m3, toff); r4 = mod_pos4_load<GB>(m4, toff);
            if (edge) re = mod_pos4_load<GB>(me, toff);
        };
        if constexpr (AHEAD) request(0);
        for (int t = 0; t < T; ++t) {
            if (t % ut == 0) {
                const long toff = (long)(t / ut) * xstride;
                if constexpr (!AHEAD) request(toff);
                mod_pos4_eval<GB>(m1, ca, cb, r1, lrelu, d1, vmax);
                mod_pos4_eval<GB>(m2, ca, cb, r2, lrelu, d2, vmax);
                mod_pos4_eval<GB>(m3, ca, cb, r3, lrelu, d3, vmax);
                mod_pos4_eval<GB>(m4, ca, cb, r4, lrelu, d4, vmax);
                if (edge) mod_pos4_eval<GB>(me, ca, cb, re, lrelu, de, vmax);
                // the next input frame's requests go out in front of this frame's transform and stores, and stay in flight under them
                if constexpr (AHEAD) if (t + ut < T) request(toff + xstride);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float up = __shfl_up(d4[c], 4), dn = __shfl_down(d1[c], 4);
                    d0[c] = left_row ? 0.f : (left_own ? de[c] : up);
                    d5[c] = right_row ? 0.f : (right_own ? de[c] : dn);
                }
            }
            char* o = ob + (long)t * ostride_t;
            auto planes = [&](auto k) {   // the planes 2k and 2k + 1
                constexpr int X0 = 2 * decltype(k)::value, X1 = X0 + 1;
                half4_t ph0, pl0, ph1, pl1;
                mod4_plane<X0>(d0, d1, d2, d3, d4, d5, ph0, pl0, bad);
                mod4_plane<X1>(d0, d1, d2, d3, d4, d5, ph1, pl1, bad);
                if constexpr (ONE) {
                    if (!live) ph0 = ph1 = half4_t{0, 0, 0, 0};
                    if constexpr (ST16) {   // even lane: plane 2k = its four channels + the odd lane's; odd lane: plane 2k + 1 (ob holds the + 1)
                        const uint2 h0 = mod4_bits(ph0), h1 = mod4_bits(ph1);
                        const uint2 got = mod4_pair_swap(odd ? h0 : h1);
                        mod4_store16(o + X0 * ostride_x, odd ? make_uint4(got.x, got.y, h1.x, h1.y) : make_uint4(h0.x, h0.y, got.x, got.y));
                    } else {
                        *reinterpret_cast<half4_t*>(o + X0 * ostride_x) = ph0;
                        *reinterpret_cast<half4_t*>(o + X1 * ostride_x) = ph1;
                    }
                } else if constexpr (ST16) {   // even lane: hi c0-7 (c8-15) = its hi part + the odd lane's; odd lane: lo = the even lane's + its own
                    const uint2 h0 = mod4_bits(ph0), l0 = mod4_bits(pl0), h1 = mod4_bits(ph1), l1 = mod4_bits(pl1);
                    const uint2 g0 = mod4_pair_swap(odd ? h0 : l0), g1 = mod4_pair_swap(odd ? h1 : l1);
                    mod4_store16(o + X0 * ostride_x, odd ? make_uint4(g0.x, g0.y, l0.x, l0.y) : make_uint4(h0.x, h0.y, g0.x, g0.y));
                    mod4_store16(o + X1 * ostride_x, odd ? make_uint4(g1.x, g1.y, l1.x, l1.y) : make_uint4(h1.x, h1.y, g1.x, g1.y));
                } else {
#ifdef MOD_NT
                    __builtin_nontemporal_store(ph0, reinterpret_cast<half4_t*>(o + X0 * ostride_x));
                    __builtin_nontemporal_store(pl0, reinterpret_cast<half4_t*>(o + X0 * ostride_x + 16));
                    __builtin_nontemporal_store(ph1, reinterpret_cast<half4_t*>(o + X1 * ostride_x));
                    __builtin_nontemporal_store(pl1, reinterpret_cast<half4_t*>(o + X1 * ostride_x + 16));
#else
                    *reinterpret_cast<half4_t*>(o + X0 * ostride_x) = ph0;
                    *reinterpret_cast<half4_t*>(o + X0 * ostride_x + 16) = pl0;
                    *reinterpret_cast<half4_t*>(o + X1 * ostride_x) = ph1;
                    *reinterpret_cast<half4_t*>(o + X1 * ostride_x + 16) = pl1;
#endif
                }
            };
            planes(std::integral_constant<int, 0>{});
            planes(std::integral_constant<int, 1>{});
            planes(std::integral_constant<int, 2>{});
        }
    }
    if (bad && range_flag) atomicOr(range_flag, 1);
    publish_umax(umax, vmax);
}

int run_modulate(const float* x, const float* coef, const float* gb, float* out, int B, int T, int H, int W, int C, int ut,
                 int us, int lrelu, hipStream_t st, bool hl16, int* range_flag, int* umax, GbRows rows) {
    I2V_REQUIRE(C % 8 == 0, I2V_E_INVALID, "modulate: channels %d not a multiple of 8", C);
    const long per = (long)H * W * (C / 8);  // threads per sample (each loops over the T frames)
    I2V_REQUIRE(per * T < (1L << 31), I2V_E_INVALID, "modulate: tensor too large");
    const unsigned gx = (unsigned)std::min<long>((per + 255) / 256, 8192);
    if (gb && rows.shared() && hl16)
        hipLaunchKernelGGL((modulate_kernel<true, true>), dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb, out,
                           T, H, W, C, ut, us, lrelu, range_flag, umax, rows.k, rows.r0);
    else if (gb && rows.shared())
        hipLaunchKernelGGL((modulate_kernel<false, true>), dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb, out,
                           T, H, W, C, ut, us, lrelu, range_flag, umax, rows.k, rows.r0);
    else if (hl16)
        hipLaunchKernelGGL(modulate_kernel<true>, dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb, out,
                           T, H, W, C, ut, us, lrelu, range_flag, umax);
    else
        hipLaunchKernelGGL(modulate_kernel<false>, dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb, out,
                           T, H, W, C, ut, us, lrelu, range_flag, umax);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

#ifdef I2V_MEASURE
static int mod4_last_form = -1;   // the FORM the last writer launch ran: lets a test see that I2V_MOD4_FORM reached the launch
extern "C" int i2v_measure_mod4_last_form() { return mod4_last_form; }
#endif

// the F(4,3) operand.  one: the one-term operand (mma = 3) -- C channels of x, written as CinPad = C rounded up to 64 (the kernel's
// chunks come in pairs)
int run_modulate_wino4(const float* x, const float* coef, const float* gb, float* out, int B, int T, int H, int W, int C, int ut,
                       int us, int lrelu, hipStream_t st, bool one, int* range_flag, int* umax, GbRows rows) {
    const char* what = one ? "one-term F(4,3)" : "F(4,3)";
    I2V_REQUIRE(C % 32 == 0 && W % 4 == 0, I2V_E_INVALID, "modulate (%s operand): channels %d / width %d", what, C, W);
    const int Cp = one ? (C + 63) / 64 * 64 : C;
    const long per = (long)H * (W / 4) * (Cp / 4);   // one thread per (h, tile, 4 channels)
    I2V_REQUIRE(per % 64 == 0, I2V_E_INVALID, "modulate (%s operand): %ld threads per sample (need whole wavefronts)", what, per);
    I2V_REQUIRE(per * T * 6 < (1L << 31), I2V_E_INVALID, "modulate: tensor too large");
    const unsigned gx = (unsigned)std::min<long>((per + 255) / 256, 8192);
    const bool sh = gb && rows.shared();
    // (the trailing C is the tensor's own channel count Cx of the one-term form; the split form sets Cx = C itself)
    auto launch = [&](auto* kernel) {
        hipLaunchKernelGGL(kernel, dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb, reinterpret_cast<char*>(out),
                           T, H, W, Cp, ut, us, lrelu, range_flag, umax, C, rows.k, rows.r0);
    };
#ifdef I2V_MEASURE   // (measurement build only: the production library reads no environment variable on a launch path)
    mod4_last_form = MOD4_FORM;
    if (const char* e = getenv("I2V_MOD4_FORM")) {   // bit 0: 16-byte stores, bit 1: frame-ahead loads; 0 is the writer up to round 6
        auto pick = [&](auto form) {
            constexpr int F = decltype(form)::value;
            if (!one && sh) launch(modulate_wino4_kernel<true, false, true, F>);
            else if (!one && gb) launch(modulate_wino4_kernel<true, false, false, F>);
            else if (!one) launch(modulate_wino4_kernel<false, false, false, F>);
            else if (sh) launch(modulate_wino4_kernel<true, true, true, F>);
            else if (gb) launch(modulate_wino4_kernel<true, true, false, F>);
            else launch(modulate_wino4_kernel<false, true, false, F>);
        };
        mod4_last_form = atoi(e) == 0 ? 0 : atoi(e) == 1 ? 1 : 3;
        switch (atoi(e)) {   // (2, loads ahead of 8-byte stores, is not built: 16 waves per CU leave it no registers)
        case 0: pick(std::integral_constant<int, 0>{}); break;
        case 1: pick(std::integral_constant<int, 1>{}); break;
        default: pick(std::integral_constant<int, 3>{}); break;
        }
        I2V_HIP_CHECK(hipGetLastError());
        return I2V_OK;
    }
#endif
    if (!one && sh) launch(modulate_wino4_kernel<true, false, true>);
    else if (!one && gb) launch(modulate_wino4_kernel<true>);
    else if (!one) launch(modulate_wino4_kernel<false>);
    else if (sh) launch(modulate_wino4_kernel<true, true, true>);
    else if (gb) launch(modulate_wino4_kernel<true, true>);
    else launch(modulate_wino4_kernel<false, true>);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int run_modulate_wino(const float* x, const float* coef, const float* gb, float* out, int B, int T, int H, int W, int C, int ut,
                      int us, int lrelu, hipStream_t st, int* range_flag, int* umax, GbRows rows) {
    I2V_REQUIRE(C % 32 == 0 && W % 2 == 0, I2V_E_INVALID, "modulate (Winograd operand): channels %d / width %d", C, W);
    const long per = (long)H * (W / 2) * (C / 8) * 2;
    I2V_REQUIRE(per % 64 == 0, I2V_E_INVALID, "modulate (Winograd operand): %ld threads per sample (need whole wavefronts)", per);
    I2V_REQUIRE(per * T * 4 < (1L << 31), I2V_E_INVALID, "modulate: tensor too large");
    const unsigned gx = (unsigned)std::min<long>((per + 255) / 256, 8192);
    if (gb && rows.shared())
        hipLaunchKernelGGL(modulate_wino_kernel<true>, dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb,
                           reinterpret_cast<char*>(out), T, H, W, C, ut, us, lrelu, range_flag, umax, rows.k, rows.r0);
    else
        hipLaunchKernelGGL(modulate_wino_kernel<false>, dim3(gx, B), dim3(256), 0, st, x, reinterpret_cast<const float2*>(coef), gb,
                           reinterpret_cast<char*>(out), T, H, W, C, ut, us, lrelu, range_flag, umax);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int status_finish(int* status, hipStream_t st) {
    hipLaunchKernelGGL(status_finish_kernel, dim3(1), dim3(1), 0, st, status);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

}  // namespace i2v
