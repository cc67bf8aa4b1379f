// Host-only check program of the conv kernels' host code (tests/test_host_wino_pack.py compiles it with csrc/i2v_conv16w4.hip
// -DW4_HOST_ONLY and csrc/i2v_common.hip, and compares
// its output with tests/golden/wino_pack_digests.json, which the same cases gave on the packers and forwards BEFORE they were
// folded into csrc/i2v_wino_pack.h and wino4_plan):
//   pack <case> <FNV-1a-64 over the packed bytes and the metadata>     every weight packer, weights from a small LCG
//   plan <layer> <the W4Args block and the kernel instantiation>       every F(4,3) layer of two decoders, 256 CUs, default switches
// No HIP call is made: the packers are plain C++ and the plan is a pure function.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "i2v_conv16w4_dev.h"

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

static void emit(const std::string& name, const Fnv& f) { printf("pack %s %016llx\n", name.c_str(), (unsigned long long)f.h); }

static const char* fill_name(int fill) { return fill == 0 ? "" : fill == 1 ? "_zero" : "_1e20"; }
static std::string scale_name(double s) { return s == 1.0 ? "s1" : "sneg"; }

// layout: 0 split F(2,3), 1 split F(4,3), 2 one-term F(4,3)
static void wino_case(int layout, int cout, int cin, int kt, bool tdup, double scale, int fill) {
    const WinoLayout& L = layout == 0 ? WINO_F23 : layout == 1 ? WINO_F43 : WINO_F43_ONE;
    const std::vector<float> w = weights((size_t)cout * cin * (tdup ? 27 : kt * 9), fill, 77 + cout * 131 + cin);
    const PackedHalfs p = wino_pack(L, w.data(), cout, cin, scale, kt, tdup);
    Fnv f;
    f.bytes(p.halfs.data(), p.bytes());
    for (long v : {(long)cout, (long)cin, (long)(tdup ? 2 : kt), (long)tdup, (long)p.CoutPad, (long)p.CinPad, (long)p.nchunk, (long)p.wexp, p.set_bytes}) f.num(v);
    char nm[128];
    snprintf(nm, sizeof nm, "%s_%dx%d_%s_%s%s", layout == 0 ? "f23" : layout == 1 ? "f43" : "f43one", cout, cin, tdup ? "tdup" : kt == 3 ? "kt3" : "kt1",
             scale_name(scale).c_str(), fill_name(fill));
    emit(nm, f);
}

static void conv16_case(int cout, int cin, int kt, int kh, int kw, bool tdup, double scale, int fill) {
    const std::vector<float> w = weights((size_t)cout * cin * (tdup ? 27 : kt * kh * kw), fill, 99 + cout * 131 + cin);
    std::vector<double> w2;
    if (tdup) {
        w2 = tdup_pair_sums(w.data(), cout, cin);
        for (double& v : w2) v = (double)(float)v;
    } else {
        w2.assign(w.begin(), w.end());
    }
    const PackedHalfs p = conv16_pack_sets(w2, tdup ? 2 : 1, cout, cin, tdup ? 18 : kt * kh * kw, scale);
    Fnv f;
    f.bytes(p.halfs.data(), p.bytes());
    for (long v : {(long)cout, (long)cin, (long)(tdup ? 2 : kt), (long)(tdup ? 3 : kh), (long)(tdup ? 3 : kw), (long)tdup, (long)p.CoutPad, (long)p.nchunk, (long)p.wexp,
                   tdup ? p.set_bytes : 0L}) f.num(v);
    char nm[128];
    snprintf(nm, sizeof nm, "c16_%dx%d_%s_%s%s", cout, cin, tdup ? "tdup" : kt == 3 ? "k333" : kh == 3 ? "k133" : "k111", scale_name(scale).c_str(), fill_name(fill));
    emit(nm, f);
}

static void wino32_case(int cout, int cin, double scale) {
    const std::vector<float> w = weights((size_t)cout * cin * 27, 0, 55 + cout * 131 + cin);
    const std::vector<float> u = wino43_planes_f32(w.data(), cout, cin, scale);   // [6][Cout][Cin][kt][kh]
    Fnv f;
    f.bytes(u.data(), u.size() * 4);
    char nm[128];
    snprintf(nm, sizeof nm, "f43f32_%dx%d_%s", cout, cin, scale_name(scale).c_str());
    emit(nm, f);
}

// ---- launch plans
static void plan_case(const char* dec, const char* layer, bool one, int cout, int cin, int kt, bool tdup, int B, int T, int H, int W, bool has_res, int rt, int rs,
                      int epi, bool has_stats) {
    Wino4Weights wts;   // the metadata the packers would leave (their formulas are covered by the pack digests); nothing is uploaded
    wts.Cin = cin; wts.Cout = cout; wts.KT = tdup ? 2 : kt; wts.tdup = tdup; wts.one = one;
    wts.CinPad = one ? (cin + 63) / 64 * 64 : cin;
    wts.CoutPad = (cout + 31) / 32 * 32;
    wts.nchunk = one ? wts.CinPad / 32 : cin / 16;
    wts.wexp = 3;
    wts.set_bytes = (long)wts.KT * 3 * wts.nchunk * 6 * wts.CoutPad * 32 * 2;
    printf("plan %s_%s_%s_B%d ", dec, layer, one ? "one" : "split", B);
    W4Plan p;
    if (wino4_plan(&p, wts, B, T, H, W, has_res, rt, rs, epi, has_stats, 256, W4Switches{})) { printf("error\n"); return; }
    const W4Args& a = p.a;
    unsigned ob;
    std::memcpy(&ob, &a.oscale, 4);
    // (skew=0: a field of the persistent kernels, retired since; the recorded plans keep its place)
    printf("B=%d T=%d H=%d W=%d J=%d Cin=%d Cout=%d CoutPad=%d nchunk=%d tdup=%d wset_stride=%ld TT=%d TH=%d TJ=%d nbT=%d nbH=%d nbJ=%d th_shift=%d rt_shift=%d "
           "rs_shift=%d hh_magic=%d rt=%d rs=%d epi=%d oscale=%08x tofs=%d order=%d skew=0 nvirt=%d NT=%d BN=%d NTH=%d grid=%u lds=%zu\n",
           a.B, a.T, a.H, a.W, a.J, a.Cin, a.Cout, a.CoutPad, a.nchunk, a.tdup, a.wset_stride, a.TT, a.TH, a.TJ, a.nbT, a.nbH, a.nbJ, a.th_shift, a.rt_shift,
           a.rs_shift, a.hh_magic, a.rt, a.rs, a.epi, ob, a.tofs, a.order, a.nvirt, p.NT, p.BN, p.NTH, p.grid, p.lds_bytes);
}

// blocks g_1 .. g_4 of a decoder: channels (16, 8, 4, 2) nf -> (8, 4, 2, 1) nf; g_1 .. g_3 up-sample x2 in time and space (conv_0 is a
// temporal-duplication pair), g_4 by (ut4, us4)
static void decoder_plans(const char* dec, int nf, int ut4, int us4) {
    int T = 2, S = 8;
    for (int k = 1; k <= 4; ++k) {
        const int ut = k < 4 ? 2 : ut4, us = k < 4 ? 2 : us4;
        T *= ut; S *= us;
        const int n_in = (32 >> k) * nf, n_out = n_in / 2;
        char layer[3][32];
        snprintf(layer[0], 32, "g%d_conv0", k); snprintf(layer[1], 32, "g%d_conv1", k); snprintf(layer[2], 32, "g%d_spade", k);
        for (int B : {1, 8, 32, 64}) {
            for (int one = 0; one < 2; ++one) {
                plan_case(dec, layer[0], one, n_out, n_in, 3, ut == 2, B, T, S, S, false, 1, 1, EPI_NONE, true);
                plan_case(dec, layer[1], one, n_out, n_out, 3, false, B, T, S, S, true, ut, us, EPI_LRELU, true);
            }
            plan_case(dec, layer[2], false, 2 * n_in, 128, 1, false, B, 1, S, S, false, 1, 1, EPI_NONE, false);   // SPADE's gamma | beta Conv2d
        }
    }
}

int main() {
    const std::pair<int, int> wino_shapes[] = {{32, 32}, {64, 32}, {32, 64}, {96, 64}, {128, 128}};
    for (int layout = 0; layout < 3; ++layout) {
        for (auto [cout, cin] : wino_shapes)
            for (double scale : {1.0, -0.37}) {
                wino_case(layout, cout, cin, 3, false, scale, 0);
                if (layout != 2) wino_case(layout, cout, cin, 1, false, scale, 0);   // (the one-term form has no 1x3x3 variant)
                wino_case(layout, cout, cin, 3, true, scale, 0);
            }
        wino_case(layout, 32, 32, 3, false, 1.0, 1);
        wino_case(layout, 32, 32, 3, false, 1.0, 2);
        wino_case(layout, 32, 32, 3, true, -0.37, 2);
    }
    const std::pair<int, int> c16_shapes[] = {{40, 24}, {72, 32}, {128, 128}};
    for (auto [cout, cin] : c16_shapes)
        for (double scale : {1.0, -0.37}) {
            conv16_case(cout, cin, 3, 3, 3, false, scale, 0);
            conv16_case(cout, cin, 1, 3, 3, false, scale, 0);
            conv16_case(cout, cin, 1, 1, 1, false, scale, 0);
            conv16_case(cout, cin, 3, 3, 3, true, scale, 0);
        }
    conv16_case(40, 24, 3, 3, 3, false, 1.0, 1);
    conv16_case(40, 24, 3, 3, 3, false, 1.0, 2);
    conv16_case(40, 24, 3, 3, 3, true, -0.37, 2);
    for (double scale : {1.0, -0.37}) { wino32_case(32, 32, scale); wino32_case(64, 32, scale); }
    decoder_plans("bair64_nf64", 64, 1, 1);     // 64 x 64, T = 16
    decoder_plans("hw128_nf32", 32, 1, 2);      // 128 x 128, T = 16
    return 0;
}
