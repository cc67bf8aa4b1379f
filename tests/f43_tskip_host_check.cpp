// Host-only self-test of the temporal edge rule of the F(4,3) kernels (csrc/i2v_conv16w4_edge.h, the only header it includes).
// tests/test_host_f43_tskip.py compiles it as plain C++17 (also with -fsanitize=address,undefined) and reads its last line.
//
// For T in {2, 4, 6, 8, 12, 16, 32} input frames, KT = 2 (temporal-duplication pairs, both parities) and 3, TH in {4, 8, 16, 32} rows per
// brick frame (TT = 32 / TH frames per brick of 128 tiles, where that is a whole number of frames: TH = 4 has eight half-size frames and
// a row block spanning two) and EVERY t-brick of the launch, at the top, an inner and the bottom h-brick of the map:
//   mask    w4_unit_dead == the brute force: enumerate every staged V row a (kt, row block) unit reads -- 32 tiles x 3 kh taps, row =
//           arow + (kt HH + kh) 4 as in w4_pass -- decode it as w4_tables does (frame, row, tile column of the halo brick) and apply its
//           `ok` flag; the unit is dead iff ALL its rows are padding;
//   count   per launch (T a multiple of TT) the dead units equal the closed form: 2 x (row blocks per frame) where a row block lies in
//           one frame (3x3x3: the front and the back frame; pairs: one end per parity), none where it spans two;
//   masks   w4_dead_mask packs the same bits per wave (WM = 4, 2, 1).
// Negative controls, each of which the comparison must flag: pt off by one, the parities swapped, and a rule that declares a unit dead
// by its first frame where the row block spans two.
#include <cstdio>
#include <vector>

#include "i2v_conv16w4_edge.h"

using namespace i2v;

typedef bool (*Rule)(int T, int th_shift, int KT, int tdup, int t0, int par, int kt, int rb);

static bool rule_pt_off(int T, int s, int KT, int tdup, int t0, int par, int kt, int rb) { return w4_unit_dead(T, s, KT, tdup, t0, par, kt - 1, rb); }
static bool rule_par_swapped(int T, int s, int KT, int tdup, int t0, int par, int kt, int rb) { return w4_unit_dead(T, s, KT, tdup, t0, tdup ? 1 - par : par, kt, rb); }
static bool rule_spanning(int T, int s, int KT, int tdup, int t0, int par, int kt, int rb) {
    const int pt = tdup ? 1 - par : KT / 2;
    const int t = t0 + ((rb * 32) >> (s + 2)) + kt - pt;   // (no guard: the FIRST frame of the row block decides)
    return t < 0 || t >= T;
}

// the `ok` flag of w4_tables for staged row r of plane 0 of the brick (t0, h0) -- T x H map, halo brick of (TT + KT - 1) x (TH + 2) x 4 rows
static bool row_ok(int r, int T, int H, int TH, int KT, int tdup, int t0, int h0, int par) {
    const int pt = tdup ? 1 - par : KT / 2;
    const int HH = TH + 2;
    int q = r >> 2;
    const int qh = q / HH, ih = q - qh * HH;
    const int t = t0 + qh - pt, h = h0 + ih - 1;
    return t >= 0 && t < T && h >= 0 && h < H;
}

static bool brute_dead(int T, int H, int TH, int th_shift, int KT, int tdup, int t0, int h0, int par, int kt, int rb, std::vector<int>* frames) {
    const int HH = TH + 2;
    bool any_ok = false;
    for (int l = 0; l < 32; ++l) {
        int m = rb * 32 + l;                       // tile of the brick (512-thread kernels: tile = MFMA row)
        const int ij = m & 3; m >>= 2;
        const int ih = m & (TH - 1); m >>= th_shift;
        if (frames) frames->push_back(m);
        const int arow = (m * HH + ih) * 4 + ij;   // LDS row of the tile at tap (0, 0)
        for (int kh = 0; kh < 3; ++kh) any_ok |= row_ok(arow + (kt * HH + kh) * 4, T, H, TH, KT, tdup, t0, h0, par);
    }
    return !any_ok;
}

struct Tally { long units = 0, mismatches = 0, count_bad = 0, launches = 0, dead = 0, spanning_dead = 0; };

static Tally sweep(Rule rule, bool own) {
    Tally y;
    const int Ts[] = {2, 4, 6, 8, 12, 16, 32}, THs[] = {4, 8, 16, 32};
    for (int T : Ts)
        for (int KT = 2; KT <= 3; ++KT)
            for (int TH : THs) {
                const int tdup = KT == 2;
                int th_shift = 0;
                while ((1 << th_shift) < TH) ++th_shift;
                const int fpb = 128 / (TH * 4);                // frames a brick of 128 tiles covers
                const int TT = fpb;
                const int H = 2 * TH + TH;                     // three h-bricks: top, inner, bottom
                long dead_launch = 0;
                for (int par = 0; par < (tdup ? 2 : 1); ++par)
                    for (int t0 = 0; t0 < T; t0 += TT)
                        for (int kt = 0; kt < KT; ++kt)
                            for (int rb = 0; rb < 4; ++rb) {
                                const bool got = rule(T, th_shift, KT, tdup, t0, par, kt, rb);
                                for (int h0 = 0; h0 < H; h0 += TH) {
                                    std::vector<int> fr;
                                    const bool want = brute_dead(T, H, TH, th_shift, KT, tdup, t0, h0, par, kt, rb, &fr);
                                    ++y.units;
                                    // (where a row block spans two frames the rule is defined as "nothing dead": it may only err on
                                    //  the safe side there, e.g. for the frames of a brick behind the end of a short clip)
                                    if (TH * 4 >= 32 ? got != want : got && !want) ++y.mismatches;
                                    if (got && fr.front() != fr.back()) ++y.spanning_dead;
                                }
                                dead_launch += got;
                                y.dead += got;
                            }
                if (T % TT == 0) {
                    ++y.launches;
                    const long closed = TH * 4 >= 32 ? 2 * (TH * 4 / 32) : 0;
                    if (dead_launch != closed) ++y.count_bad;
                    if (own) {   // the plan's count and the per-wave masks are the same rule
                        long d, u;
                        w4_dead_units(T, TT, th_shift, KT, tdup, &d, &u);
                        if (d != dead_launch || u != (long)(tdup ? 2 : 1) * (T / TT) * KT * 4) ++y.count_bad;
                        for (int par = 0; par < (tdup ? 2 : 1); ++par)
                            for (int t0 = 0; t0 < T; t0 += TT) {
                                unsigned m4 = w4_dead_mask<4>(T, th_shift, KT, tdup, t0, par, 0), m2 = 0, m1 = 0;
                                for (int kt = 0; kt < KT; ++kt)
                                    for (int rb = 0; rb < 4; ++rb) {
                                        m2 |= ((w4_dead_mask<2>(T, th_shift, KT, tdup, t0, par, rb & ~1) >> (kt * 2 + (rb & 1))) & 1u) << (kt * 4 + rb);
                                        m1 |= ((w4_dead_mask<1>(T, th_shift, KT, tdup, t0, par, rb) >> kt) & 1u) << (kt * 4 + rb);
                                        if (((m4 >> (kt * 4 + rb)) & 1u) != (unsigned)w4_unit_dead(T, th_shift, KT, tdup, t0, par, kt, rb)) ++y.mismatches;
                                    }
                                if (m2 != m4 || m1 != m4) ++y.mismatches;
                            }
                    }
                }
            }
    return y;
}

int main() {
    const Tally ok = sweep(w4_unit_dead, true);
    const Tally c1 = sweep(rule_pt_off, false), c2 = sweep(rule_par_swapped, false), c3 = sweep(rule_spanning, false);
    // the compiled masks of the kernel's two geometries (what i2v_conv16w4_kernel.h derives at compile time)
    static_assert(w4_dead_mask<4>(12, 3, 3, 0, 0, 0, 0) == 0x001u && w4_dead_mask<4>(12, 3, 3, 0, 8, 0, 0) == 0x800u &&
                      w4_dead_mask<4>(4, 3, 3, 0, 0, 0, 0) == 0x801u, "TT = 4, 3x3x3: front, back, both");
    static_assert(w4_dead_mask<4>(6, 4, 2, 1, 0, 0, 0) == 0x03u && w4_dead_mask<4>(6, 4, 2, 1, 4, 1, 0) == 0xC0u &&
                      w4_dead_mask<4>(6, 4, 2, 1, 0, 1, 0) == 0u && w4_dead_mask<4>(6, 4, 2, 1, 4, 0, 0) == 0u, "TT = 2, pairs: one end per parity");
    const bool controls = c1.mismatches > 0 && c2.mismatches > 0 && c3.mismatches > 0 && c3.spanning_dead > 0;
    const bool good = ok.mismatches == 0 && ok.count_bad == 0 && ok.spanning_dead == 0 && ok.dead > 0 && controls;
    printf("f43 tskip self-test: %ld units in %ld launches, %ld dead, %ld mismatches, %ld bad counts, %ld dead units spanning frames; "
           "controls flagged %ld / %ld / %ld (%ld spanning): %s\n",
           ok.units, ok.launches, ok.dead, ok.mismatches, ok.count_bad, ok.spanning_dead, c1.mismatches, c2.mismatches, c3.mismatches,
           c3.spanning_dead, good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
