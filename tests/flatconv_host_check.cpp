// Host-only check program of the flat conv's packing (csrc/i2v_flatconv_pack.h, the only header it includes).  tests/test_host_flatconv.py
// compiles it as plain C++17 and compares its output with tests/golden/flatconv_pack_digests.json:
//   pack <case> <FNV-1a-64 over the packed weights, the (scale, shift) pairs and Cin, Cout, CoutPad, BN, C4, nchunk>
//   tile <cout> <column tile>                                                  for every cout up to 2048
// The digests were recorded BEFORE the two networks shared this header: a throwaway copy of this program in which pack_case() held the
// bodies of the two Unit::pack functions of that commit (csrc/i2v_i3d.hip for the cubic windows and all four epilogue forms,
// csrc/i2v_inception.hip for the 2-D windows with BatchNorm eps 1e-3; their upload calls replaced by a copy into the vectors) printed
// them for the same cases.  A 1x1x1 and a 1x1 window with the same epilogue are the one case both bodies have: they gave equal digests.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "i2v_flatconv_pack.h"

using namespace i2v;

static uint64_t g_lcg = 1;
static float lcg_unit() {   // [-1, 1)
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(g_lcg >> 40) / 8388608.0 - 1.0);
}
// fill: 0 LCG, 1 all zero, 2 LCG with one 1e20 entry
static std::vector<float> weights(size_t n, int fill, uint64_t seed) {
    g_lcg = seed;
    std::vector<float> w(n);
    for (float& v : w) v = fill == 1 ? 0.f : lcg_unit();
    if (fill == 2) w[n / 3] = 1e20f;
    return w;
}

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    }
    void num(long v) { const int64_t x = v; bytes(&x, 8); }
};

enum { EPI_BN = 0, EPI_BIAS = 1, EPI_IDENTITY = 2 };

// one unit through the packer; g, b, m, v: the BatchNorm tensors (b also serves as the conv bias)
static FlatConvPacked pack_case(const float* w, int cin, int cout, int kt, int kh, int kw, int epi, double eps, const float* g, const float* b,
                                const float* m, const float* v) {
    FlatConvPacked p = flatconv_pack(w, cin, cout, kt, kh, kw);
    if (epi == EPI_BN) flatconv_fold_bn(p, g, b, m, v, eps);
    else if (epi == EPI_BIAS) flatconv_bias(p, b);
    return p;
}

static void run_case(int cin, int cout, int kt, int kh, int kw, int epi, double eps, int fill) {
    const int taps = (kt > 0 ? kt : 1) * kh * kw;
    const uint64_t seed = 1234 + (uint64_t)cout * 131 + cin * 7 + taps;
    const std::vector<float> w = weights((size_t)cout * cin * taps, fill, seed);
    const std::vector<float> g = weights(cout, fill, seed + 1), b = weights(cout, fill, seed + 2), m = weights(cout, fill, seed + 3);
    std::vector<float> v = weights(cout, fill, seed + 4);
    for (float& x : v) x = 1.f + 0.5f * x;   // a variance: [0.5, 1.5), 1 when all zero, one 5e19 entry
    const FlatConvPacked p = pack_case(w.data(), cin, cout, kt, kh, kw, epi, eps, g.data(), b.data(), m.data(), v.data());
    Fnv f;
    f.bytes(p.w.data(), p.w.size() * 4);
    f.bytes(p.ss.data(), p.ss.size() * 4);
    for (long x : {(long)p.Cin, (long)p.Cout, (long)p.CoutPad, (long)p.BN, (long)p.C4, (long)p.nchunk, (long)p.w.size(), (long)p.ss.size()}) f.num(x);
    char win[32];
    if (kt > 0) snprintf(win, sizeof win, "k%dx%dx%d", kt, kh, kw);
    else snprintf(win, sizeof win, "k%dx%d", kh, kw);
    printf("pack %s_c%d_o%d_%s%s %016llx\n", win, cin, cout, epi == EPI_BN ? (eps == 1e-3 ? "bn1e-3" : "bn1e-5") : epi == EPI_BIAS ? "bias" : "identity",
           fill == 0 ? "" : fill == 1 ? "_zero" : "_1e20", (unsigned long long)f.h);
}

int main() {
    const int CIN[] = {3, 16, 24, 48, 80};        // 24 and 80: the last K chunk is ragged
    const int COUT[] = {32, 48, 112, 192, 400};   // 48 and 112: ragged against every column tile; 400: the head
    const int WIN2[][2] = {{1, 1}, {3, 3}, {5, 5}, {1, 7}, {7, 1}, {1, 3}, {3, 1}};
    for (int fill = 0; fill < 3; ++fill)
        for (int cout : COUT) {
            for (int cin : CIN) {
                for (int k : {1, 3, 7}) {
                    if (k == 7 && cin != 3) continue;   // the stem
                    run_case(cin, cout, k, k, k, EPI_BN, 1e-3, fill);
                    run_case(cin, cout, k, k, k, EPI_BN, 1e-5, fill);
                    run_case(cin, cout, k, k, k, EPI_BIAS, 0.0, fill);
                    run_case(cin, cout, k, k, k, EPI_IDENTITY, 0.0, fill);
                }
                for (const auto& k : WIN2) run_case(cin, cout, 0, k[0], k[1], EPI_BN, 1e-3, fill);
            }
        }
    for (int cout = 1; cout <= 2048; ++cout) printf("tile %d %d\n", cout, flatconv_tile(cout));
    return 0;
}
