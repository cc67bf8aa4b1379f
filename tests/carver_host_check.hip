// Host check of the workspace carver (csrc/i2v_handle.h: Carver) against the formula every handle's layout function used to carry as a
// lambda of its own, written out here: o = align_up(o + bytes, 256) after every slot.  tests/test_host_abi.py compiles it for the host
// (also with -fsanitize=address,undefined) and reads its last line.  No device code, no HIP call.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "i2v_handle.h"

int main() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    long lists = 0, slots = 0, zero_slots = 0, bad = 0;
    for (int it = 0; it < 4000; ++it) {
        const int n = 1 + (int)(next() % 24);
        i2v::Carver c;
        size_t o = 0;   // the old lambdas' running offset
        for (int i = 0; i < n; ++i) {
            // sizes around the alignment, tiny, zero, and up to a few GiB (the decoder's largest slots); floats or bytes
            const uint64_t kind = next() % 8;
            size_t units = kind == 0 ? 0 : kind == 1 ? (size_t)(next() % 3) : kind == 2 ? (size_t)(62 + next() % 5) : kind == 3 ? (size_t)(254 + next() % 5)
                         : kind == 4 ? (size_t)(next() % 100000) : kind == 5 ? ((size_t)1 << (next() % 31)) : (size_t)(next() % ((size_t)3 << 30));
            const bool as_floats = next() & 1;
            const size_t bytes = as_floats ? units * 4 : units;
            const size_t want = o;
            o = (o + bytes + 255) / 256 * 256;
            const size_t got = as_floats ? c.take_floats(units) : c.take_bytes(units);
            if (got != want || c.total() != o || got % 256 != 0) ++bad;
            ++slots;
            if (!bytes) ++zero_slots;
        }
        ++lists;
    }
    // at<T>: base + offset, typed
    alignas(256) static char base[1024];
    if (i2v::Carver::at(base, 256) != reinterpret_cast<float*>(base + 256)) ++bad;
    if (i2v::Carver::at<double>(base, 512) != reinterpret_cast<double*>(base + 512)) ++bad;
    if (i2v::Carver::at<char>(base, 0) != base) ++bad;
    std::printf("%ld lists, %ld slots, %ld zero-sized, %ld mismatches: %s\n", lists, slots, zero_slots, bad, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
