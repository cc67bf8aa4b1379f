// Host-side weight packing of the fp16 conv kernels: the power-of-two prescale, the temporal-duplication pair sums, the Winograd
// transforms U = G g and the fragment-major layouts of the F(2,3) / F(4,3) kernels, the rows of the direct split-fp16 kernel.
// Plain C++ (no HIP call, no device memory): the .hip files upload what these functions return (upload_packed, i2v_common.h), and a
// host program can digest the bytes (tests/wino_host_check.hip).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace i2v {

// Weights are stored multiplied by 2^wexp (undone in the epilogue): the largest |w| lands in [2^13, 2^14), so every lo part of a
// non-negligible weight is a normal fp16 number (full 2^-22 split precision) and hi stays far from the fp16 overflow threshold.
inline int prescale_exp(double wmax) {
    if (!(wmax > 0.0) || !std::isfinite(wmax)) return 0;
    return std::max(-40, std::min(40, (int)std::floor(std::log2(16384.0 / wmax))));
}

// A 3x3x3 conv whose input is a x2 nearest up-sampling in time of a half-rate tensor (frames 2i and 2i+1 identical) is a pair of
// 2-tap temporal kernels on that tensor: parity 0 = (W[0], W[1]+W[2]), parity 1 = (W[0]+W[1], W[2]).
// w_src [Cout][Cin][3][3][3] -> unscaled fp64 sums [2][Cout][Cin][2][3][3]
inline std::vector<double> tdup_pair_sums(const float* w_src, int cout, int cin) {
    std::vector<double> s((size_t)2 * cout * cin * 18);
    for (int par = 0; par < 2; ++par)
        for (size_t nc = 0; nc < (size_t)cout * cin; ++nc)
            for (int hw = 0; hw < 9; ++hw) {
                const double w0 = w_src[nc * 27 + hw], w1 = w_src[nc * 27 + 9 + hw], w2 = w_src[nc * 27 + 18 + hw];
                double* dst = &s[((size_t)par * cout * cin + nc) * 18];
                dst[hw] = par == 0 ? w0 : w0 + w1;
                dst[9 + hw] = par == 0 ? w1 + w2 : w2;
            }
    return s;
}

// ---- Winograd along W: U = G g of the three kw taps g.  (Functions, not coefficient tables: the packed bits depend on these
// expressions' order of operations.)
inline void wino_g23(const double* g, double* u) {
    u[0] = g[0]; u[1] = 0.5 * (g[0] + g[1] + g[2]); u[2] = 0.5 * (g[0] - g[1] + g[2]); u[3] = g[2];
}
inline void wino_g43(const double* g, double* u) {
    u[0] = g[0] / 4.0;
    u[1] = -(g[0] + g[1] + g[2]) / 6.0;
    u[2] = -(g[0] - g[1] + g[2]) / 6.0;
    u[3] = g[0] / 24.0 + g[1] / 12.0 + g[2] / 6.0;
    u[4] = g[0] / 24.0 - g[1] / 12.0 + g[2] / 6.0;
    u[5] = g[2];
}

// The fragment-major layout of a Winograd kernel's U: [parity set][tap (kt, kh)][chunk of kc channels][plane][CoutPad / 32] blocks of
// 1 KB = 2 halves x [lane = kg * 32 + n % 32][8 halfs].
//   split (kc = 16):    half 0 = fp16 hi, half 1 = fp16 lo of channels 8 kg .. 8 kg + 7 of the chunk
//   one-term (kc = 32): half = k-step (channels 0..15 | 16..31 of the chunk), the value rounded to fp16 once; Cin is padded with
//                       zero weights to a multiple of 64 (the kernel's loop takes chunks in pairs)
struct WinoLayout {
    int planes;                                  // 4: F(2,3), 6: F(4,3)
    void (*G)(const double* g, double* u);
    int kc;                                      // input channels per chunk
    bool split;
};
constexpr WinoLayout WINO_F23{4, wino_g23, 16, true}, WINO_F43{6, wino_g43, 16, true}, WINO_F43_ONE{6, wino_g43, 32, false};

struct PackedHalfs {
    std::vector<_Float16> halfs;   // every parity set
    int CoutPad = 0, CinPad = 0, nchunk = 0, wexp = 0;
    long set_bytes = 0;            // bytes of one parity set
    size_t bytes() const { return halfs.size() * 2; }
};

// w3: [nset][Cout][Cin][NT = kt * 3][3] in fp64, already scaled
inline PackedHalfs wino_pack_sets(const WinoLayout& L, const std::vector<double>& w3, int nset, int cout, int cin, int kt) {
    PackedHalfs o;
    o.CinPad = L.split ? cin : (cin + 63) / 64 * 64;
    o.CoutPad = (cout + 31) / 32 * 32;
    o.nchunk = o.CinPad / L.kc;
    const int NT = kt * 3, P = L.planes;
    std::vector<double> u((size_t)nset * cout * cin * NT * P);
    double wmax = 0.0;
    for (size_t i = 0; i < (size_t)nset * cout * cin * NT; ++i) {
        L.G(&w3[i * 3], &u[i * P]);
        for (int x = 0; x < P; ++x) wmax = std::max(wmax, std::fabs(u[i * P + x]));
    }
    o.wexp = prescale_exp(wmax);
    const double pre = std::ldexp(1.0, o.wexp);
    const size_t set_halfs = (size_t)NT * o.nchunk * P * o.CoutPad * 32;
    o.halfs.assign((size_t)nset * set_halfs, (_Float16)0.f);
    for (int s = 0; s < nset; ++s)
        for (int n = 0; n < cout; ++n)
            for (int c = 0; c < cin; ++c)
                for (int tap = 0; tap < NT; ++tap)
                    for (int x = 0; x < P; ++x) {
                        const float v = (float)(u[((((size_t)s * cout + n) * cin + c) * NT + tap) * P + x] * pre);
                        const _Float16 hi = (_Float16)v;
                        const int chunk = c / L.kc, cc = c % L.kc;
                        _Float16* blk = &o.halfs[s * set_halfs + ((((size_t)tap * o.nchunk + chunk) * P + x) * (o.CoutPad / 32) + n / 32) * 1024];
                        const int at = (cc >> 4) * 512 + ((((cc >> 3) & 1) * 32 + n % 32) * 8) + (cc & 7);
                        blk[at] = hi;
                        if (L.split) blk[at + 512] = (_Float16)(v - (float)hi);
                    }
    o.set_bytes = (long)set_halfs * 2;
    return o;
}

// w_src: torch layout [Cout][Cin][kt][3][3]; tdup: from a 3x3x3 kernel, the two parity sets of its 2x3x3 pair kernels (KT = 2)
inline PackedHalfs wino_pack(const WinoLayout& L, const float* w_src, int cout, int cin, double scale, int kt, bool tdup) {
    std::vector<double> w3;
    if (tdup) {
        w3 = tdup_pair_sums(w_src, cout, cin);
        for (double& v : w3) v *= scale;
    } else {
        w3.resize((size_t)cout * cin * kt * 9);
        for (size_t i = 0; i < w3.size(); ++i) w3[i] = (double)w_src[i] * scale;
    }
    return wino_pack_sets(L, w3, tdup ? 2 : 1, cout, cin, tdup ? 2 : kt);
}

// The six fp32 plane kernels U_x [Cout][Cin][3 (kt)][3 (kh)] of the exact-fp32 F(4,3) path (fp64 -> fp32 once)
inline std::vector<float> wino43_planes_f32(const float* w_src, int cout, int cin, double scale) {
    const size_t plane = (size_t)cout * cin * 9;
    std::vector<float> u(6 * plane);
    for (size_t i = 0; i < plane; ++i) {
        const double g[3] = {(double)w_src[i * 3] * scale, (double)w_src[i * 3 + 1] * scale, (double)w_src[i * 3 + 2] * scale};
        double d[6];
        wino_g43(g, d);
        for (int x = 0; x < 6; ++x) u[x * plane + i] = (float)d[x];
    }
    return u;
}

// ---- the direct split-fp16 kernel (i2v_conv16.hip): [set][tap + one all-zero tap][chunk of 32][CoutPad][4 groups x (8 hi | 8 lo)]
constexpr int CONV16_KC = 32;
// w: [nset][Cout][Cin][ntaps] in fp64, NOT yet scaled (every value is multiplied by scale, then by the prescale)
inline PackedHalfs conv16_pack_sets(const std::vector<double>& w, int nset, int cout, int cin, int ntaps, double scale) {
    PackedHalfs o;
    o.CinPad = cin;
    o.CoutPad = (cout + 31) / 32 * 32;
    if (o.CoutPad > 64 && o.CoutPad % 128) o.CoutPad = (o.CoutPad + 127) / 128 * 128;
    o.nchunk = (cin + CONV16_KC - 1) / CONV16_KC;
    double wmax = 0.0;
    for (double v : w) wmax = std::max(wmax, std::fabs(v * scale));
    o.wexp = prescale_exp(wmax);
    const double pre = std::ldexp(1.0, o.wexp);
    const size_t set_halfs = (size_t)(ntaps + 1) * o.nchunk * o.CoutPad * 64;
    o.halfs.assign((size_t)nset * set_halfs, (_Float16)0.f);
    for (int s = 0; s < nset; ++s)
        for (int n = 0; n < cout; ++n)
            for (int c = 0; c < cin; ++c)
                for (int tap = 0; tap < ntaps; ++tap) {
                    const float v = (float)(w[(((size_t)s * cout + n) * cin + c) * ntaps + tap] * scale * pre);
                    const _Float16 hi = (_Float16)v;
                    const int chunk = c / CONV16_KC, g = (c % CONV16_KC) / 8, j = c % 8;
                    _Float16* row = &o.halfs[s * set_halfs + (((size_t)tap * o.nchunk + chunk) * o.CoutPad + n) * 64];
                    row[g * 16 + j] = hi;
                    row[g * 16 + 8 + j] = (_Float16)(v - (float)hi);
                }
    o.set_bytes = (long)set_halfs * 2;
    return o;
}

}  // namespace i2v
