// Host-side packing of the flat implicit-GEMM conv (i2v_flatconv.h): the column-tile rule, the [Cout][Cin][taps] -> [nchunk][CoutPad][16]
// weight layout and the three epilogue forms as (scale, shift) pairs.
// Plain C++ (no HIP call, no device memory): the .hip files upload what these functions return (FlatConv::upload), and a host program
// can digest the bytes (tests/flatconv_host_check.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace i2v {

// column tile of a unit: the one of 128, 64, 32 that pads Cout least, the wider on a tie
inline int flatconv_tile(int cout) {
    int best = 128;
    for (int bn : {64, 32})
        if ((cout + bn - 1) / bn * bn < (cout + best - 1) / best * best) best = bn;
    return best;
}

struct FlatConvPacked {
    std::vector<float> w;    // [nchunk][CoutPad][16], K = tap * CinP + c in chunks of 16, zero where K or Cout is padded
    std::vector<float> ss;   // [CoutPad] (scale, shift), (0, 0) behind Cout
    int Cin = 0, Cout = 0, CoutPad = 0, BN = 64, C4 = 0, nchunk = 0;   // C4: groups of 4 input channels (CinP / 4)
    int kt = 0, kh = 1, kw = 1;                                        // the window; kt = 0: a 2-D unit (no time extent)
};

// wsrc [Cout][Cin][taps], taps = kt kh kw in (dt, dh, dw) order (kh kw for kt = 0); the epilogue is the identity (1, 0) until one of
// the functions below sets it
inline FlatConvPacked flatconv_pack(const float* wsrc, int cin, int cout, int kt, int kh, int kw) {
    FlatConvPacked p;
    p.Cin = cin; p.Cout = cout; p.kt = kt; p.kh = kh; p.kw = kw;
    const int taps = (kt > 0 ? kt : 1) * kh * kw;
    p.BN = flatconv_tile(cout);
    p.CoutPad = (cout + p.BN - 1) / p.BN * p.BN;
    const int CinP = (cin + 3) / 4 * 4;
    p.C4 = CinP / 4;
    p.nchunk = (int)(((long)taps * CinP + 15) / 16);
    p.w.assign((size_t)p.nchunk * p.CoutPad * 16, 0.f);
    for (int n = 0; n < cout; ++n)
        for (int c = 0; c < cin; ++c)
            for (int tap = 0; tap < taps; ++tap) {
                const long kk = (long)tap * CinP + c;
                p.w[((size_t)(kk / 16) * p.CoutPad + n) * 16 + kk % 16] = wsrc[((size_t)n * cin + c) * taps + tap];
            }
    p.ss.assign((size_t)p.CoutPad * 2, 0.f);
    for (int n = 0; n < cout; ++n) p.ss[2 * n] = 1.f;
    return p;
}

// eval-mode BatchNorm, (x - mean) / sqrt(var + eps) * weight + bias, folded in double; eps = 1e-3 in the Kinetics I3D (Unit3Dpy:
// tf_style_eps) and in Inception's BasicConv2d, torch's default 1e-5 in the dynamic-texture I3D (ID3.Unit3D)
inline void flatconv_fold_bn(FlatConvPacked& p, const float* g, const float* b, const float* m, const float* v, double eps) {
    for (int n = 0; n < p.Cout; ++n) {
        const double a = (double)g[n] / std::sqrt((double)v[n] + eps);
        p.ss[2 * n] = (float)a;
        p.ss[2 * n + 1] = (float)((double)b[n] - (double)m[n] * a);
    }
}

// a conv bias and no norm: (1, bias)
inline void flatconv_bias(FlatConvPacked& p, const float* bias) {
    for (int n = 0; n < p.Cout; ++n) { p.ss[2 * n] = 1.f; p.ss[2 * n + 1] = bias[n]; }
}

}  // namespace i2v
