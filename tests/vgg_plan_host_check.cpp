// Host check of the VGG-16 layer plan (csrc/i2v_vgg_plan.h: vgg_plan) against the rules the trunk's entries carried one by one before
// they shared it, written out here independently: the slot-sizing loop (a flag that says whether the input lies in slot a), the
// saved-offset loop, the forward's choice of a destination by comparing pointers, the h /= 2; w /= 2 bookkeeping of each, and
// 2 * align_up(N * H * W * 64 * 4, 256) for the backward workspace.  tests/test_host_vgg.py compiles it for the host (also with
// -fsanitize=address,undefined) and reads its last line.  `--perturb` swaps slots a and b of one layer of every plan before the
// comparison: the check has to count mismatches then.  No device code, no HIP call.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "i2v_handle.h"
#include "i2v_vgg_plan.h"

namespace {

// (output channels, tap or -1, pool behind it) of the thirteen convolutions, typed in again
const int COUT[13] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int CIN[13] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int TAP[13] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};
const int POOL[13] = {0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0};

size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// "addresses": the workspace, the saved buffer and the five tap buffers lie far apart
const uint64_t WS = 1ull << 44, SAVED = 2ull << 44, TAPS = 3ull << 44;
uint64_t tap_addr(int k) { return TAPS + ((uint64_t)k << 40); }

uint64_t plan_addr(const i2v::VggPlan& p, const i2v::VggLayerPlan& L, i2v::VggBuf b) {
    return b == i2v::VGG_BUF_TAP ? tap_addr(L.tap) : b == i2v::VGG_BUF_SAVED ? SAVED + L.saved_off : WS + (b == i2v::VGG_BUF_A ? p.ws_a : p.ws_b);
}

}  // namespace

int main(int argc, char** argv) {
    const bool perturb = argc > 1 && !std::strcmp(argv[1], "--perturb");
    const int NS[4] = {1, 2, 3, 7}, HW[10] = {16, 17, 24, 29, 31, 32, 35, 40, 64, 224};
    long shapes = 0, checks = 0, bad = 0;
    auto expect = [&](uint64_t got, uint64_t want) { ++checks; if (got != want) ++bad; };
    for (int N : NS)
        for (int H : HW)
            for (int W : HW) {
                i2v::VggPlan p = i2v::vgg_plan<i2v::Carver>(N, H, W);
                if (perturb) {
                    i2v::VggBuf& d = p.layer[5].ws_dst;
                    d = d == i2v::VGG_BUF_A ? i2v::VGG_BUF_B : i2v::VGG_BUF_A;
                }
                ++shapes;

                // the slot-sizing loop
                size_t af = 0, bf = 0;
                {
                    int h = H, w = W;
                    bool cur_is_a = false;
                    for (int l = 0; l < 13; ++l) {
                        const size_t of = (size_t)N * h * w * COUT[l];
                        if (TAP[l] < 0) {
                            if (cur_is_a) bf = of > bf ? of : bf; else af = of > af ? of : af;
                            cur_is_a = !cur_is_a;
                        } else {
                            cur_is_a = false;
                        }
                        if (POOL[l]) {
                            h /= 2; w /= 2;
                            const size_t pf = (size_t)N * h * w * COUT[l];
                            af = pf > af ? pf : af;
                            cur_is_a = true;
                        }
                    }
                }
                const size_t a_off = 0, b_off = up256(af * 4);
                expect(p.ws_a, a_off);
                expect(p.ws_b, b_off);
                expect(p.ws_bytes, up256(af * 4) + up256(bf * 4));

                // the saved-offset loop
                size_t off[13], saved_total = 0;
                {
                    int h = H, w = W;
                    for (int l = 0; l < 13; ++l) {
                        off[l] = saved_total;
                        if (TAP[l] < 0) saved_total += up256((size_t)N * h * w * COUT[l] * 4);
                        if (POOL[l]) { h /= 2; w /= 2; }
                    }
                }
                expect(p.saved_bytes, saved_total);
                for (int l = 0; l < 13; ++l) expect(p.layer[l].saved_off, off[l]);

                // the backward workspace
                const size_t half = up256((size_t)N * H * W * 64 * 4);
                expect(p.bwd_a, 0);
                expect(p.bwd_b, half);
                expect(p.bwd_bytes, 2 * half);

                // the forward, with and without saved state: the destination of every conv and pool by the pointer comparison
                for (int keep = 0; keep < 2; ++keep) {
                    const uint64_t a = WS + a_off, b = WS + b_off, saved = keep ? SAVED : 0;
                    uint64_t cur = 5ull << 44;   // x: none of the buffers
                    int h = H, w = W;
                    for (int l = 0; l < 13; ++l) {
                        const i2v::VggLayerPlan& L = p.layer[l];
                        const uint64_t dst = TAP[l] >= 0 ? tap_addr(TAP[l]) : saved ? saved + off[l] : cur == a ? b : a;
                        expect((uint64_t)L.h, (uint64_t)h);
                        expect((uint64_t)L.w, (uint64_t)w);
                        expect((uint64_t)L.cin, (uint64_t)CIN[l]);
                        expect((uint64_t)L.cout, (uint64_t)COUT[l]);
                        expect((uint64_t)(int64_t)L.tap, (uint64_t)(int64_t)TAP[l]);
                        expect(L.pool, POOL[l] != 0);
                        expect(plan_addr(p, L, L.dst(keep != 0)), dst);
                        cur = dst;
                        if (POOL[l]) {
                            expect(plan_addr(p, L, L.pool_dst), a);
                            cur = a;
                            h /= 2; w /= 2;
                        }
                    }
                }
            }
    std::printf("%ld shapes, %ld checks, %ld mismatches: %s\n", shapes, checks, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
