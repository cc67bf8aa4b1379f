// Host check of the launch plans of the two metric trunks (csrc/i2v_trunk_plan.h): prints, case by case, every step of the plan with
// all its fields -- kind, unit, buffers (as offsets into the workspace, or the caller's), maps, window, stride, padding in front,
// padded extents of an I3D pool, channel strides and offsets, channels, relu, the grid and the column tile of the launch -- and every
// size, offset and refusal, then one FNV-1a-64 digest over the case's lines.  tests/test_host_trunk_plan.py compiles it for the host
// (also with -fsanitize=address,undefined), compares the digests with tests/golden/trunk_plan_parent.json -- the same lines printed
// from the launches of the code before the plans existed -- and the steps of a few cases with the shapes the torch modules produce.
// `--perturb` changes one field of one step of every plan (the front pad of a strided I3D unit, else the channel offset of a
// concatenation) before it is printed: the digests have to differ then.  No device code, no HIP call.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "i2v_handle.h"
#include "i2v_trunk_plan.h"

// ---- shared: the printed record, the case list ------------------------------------------------------------------------------
struct Rec {
    const char* kind = "";
    int unit = -1, blk = -1, pool = -1;
    std::string src, dst;
    int in[3] = {1, 1, 1}, out[3] = {1, 1, 1}, k[3] = {1, 1, 1}, s[3] = {1, 1, 1}, p[3] = {0, 0, 0}, e[3] = {0, 0, 0};
    int ics = 0, ioff = 0, ocs = 0, ooff = 0, C = 0, relu = 0, chw = 0;
    long grid = 0;
    int nt = 0;   // conv: 16-column tiles per wave
};
struct Out {
    std::string id, text;
    long cases = 0;
    void begin(const std::string& i) { id = i; text.clear(); }
    __attribute__((format(printf, 2, 3))) void line(const char* fmt, ...) {
        char b[640];
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(b, sizeof b, fmt, ap);
        va_end(ap);
        text += b;
        text += '\n';
    }
    void step(const Rec& r) {
        line("  %s u=%d blk=%d pool=%d %s->%s in=%d,%d,%d out=%d,%d,%d k=%d,%d,%d s=%d,%d,%d p=%d,%d,%d e=%d,%d,%d cs=%d+%d->%d+%d C=%d relu=%d chw=%d grid=%ld nt=%d",
             r.kind, r.unit, r.blk, r.pool, r.src.c_str(), r.dst.c_str(), r.in[0], r.in[1], r.in[2], r.out[0], r.out[1], r.out[2], r.k[0], r.k[1],
             r.k[2], r.s[0], r.s[1], r.s[2], r.p[0], r.p[1], r.p[2], r.e[0], r.e[1], r.e[2], r.ics, r.ioff, r.ocs, r.ooff, r.C, r.relu, r.chw, r.grid, r.nt);
    }
    void end() {
        uint64_t h = 1469598103934665603ull;
        long n = 0;
        for (unsigned char c : text) { h = (h ^ c) * 1099511628211ull; n += c == '\n'; }
        std::printf("case %s\n%sdigest %s %016llx lines %ld\n", id.c_str(), text.c_str(), id.c_str(), (unsigned long long)h, n);
        ++cases;
    }
};
struct Variant { const char* name; int dt, pool_t, classes; };
const Variant VARIANTS[3] = {{"kin", 0, 2, 400}, {"dt16", 16, 2, 18}, {"dt32", 32, 4, 18}};
std::string fmt_id(const char* fmt, ...) {
    char b[200];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    return b;
}

// Every case, on a backend that prints it: the whole trunks, then the sub-module entries at the shapes of tests/i3d_units_common.py
// and tests/fid_common.py
template <class Backend>
void all_cases(Backend& be) {
    const int TS[8] = {8, 9, 10, 16, 17, 24, 25, 32};   // 8 (Kinetics, length 16) and 24 (length 32) are refused, as every T below them
    for (const Variant& v : VARIANTS)
        for (int features = 0; features < 2; ++features)
            for (int B : {1, 3})
                for (int T : TS) be.i3d_trunk(v, features != 0, B, features ? (T < 9 ? T : 9) : T, T, 24, 40);
    const int SIDES[6] = {75, 76, 80, 99, 128, 299};
    for (int H : SIDES)
        for (int W : SIDES) be.inc_trunk(1, H, W, 3, 0xF);
    const int HW[5][2] = {{75, 80}, {99, 76}, {128, 299}, {299, 299}, {74, 74}};   // the last: refused
    for (const auto& hw : HW)
        for (int last = 0; last < 4; ++last)
            for (int B : {1, 3})
                for (unsigned taps : {0u, 0xFu, 4u}) be.inc_trunk(B, hw[0], hw[1], last, taps);
    const int REST[4] = {2, 3, 6, 5}, LADDER[4][4] = {{1, 2, 5, 5}, {1, 2, 8, 8}, {2, 1, 5, 13}, {3, 3, 7, 6}};
    const int STEM[3][4] = {{2, 9, 12, 9}, {2, 8, 12, 9}, {2, 2, 7, 16}}, HEAD[2][4] = {{2, 1, 1, 1}, {2, 3, 1, 1}};
    for (int vi = 0; vi < 2; ++vi) {
        const Variant& v = VARIANTS[vi];
        for (int unit = 0; unit <= 57; ++unit) be.i3d_unit(v, unit, REST);
        for (int unit : {3 + 6 * 2 + 1, 1, 3 + 6 * 1 + 0})
            for (const auto& sh : LADDER) be.i3d_unit(v, unit, sh);
        for (const auto& sh : STEM) be.i3d_unit(v, 0, sh);
        for (const auto& sh : HEAD) be.i3d_unit(v, 57, sh);
        const int MSH[2][4] = {{2, 3, 5, 4}, {1, 1, 7, 7}};
        for (int block = 0; block < 9; ++block)
            for (const auto& sh : MSH) be.i3d_mixed(v, block, sh);
        const int POOLS[9][9] = {{1, 3, 3, 1, 2, 2, 1, 7, 10}, {1, 3, 3, 1, 2, 2, 1, 8, 14}, {3, 3, 3, 2, 2, 2, 4, 6, 7}, {3, 3, 3, 2, 2, 2, 5, 6, 7},
                                 {2, 2, 2, 2, 2, 2, 3, 14, 5}, {2, 2, 2, 2, 2, 2, 4, 14, 5}, {3, 3, 3, 1, 1, 1, 1, 5, 6}, {3, 3, 3, 1, 1, 1, 2, 5, 6},
                                 {3, 3, 3, 1, 1, 1, 3, 5, 6}};
        for (const auto& q : POOLS)
            for (int C : {64, 528}) be.i3d_pool(v, 2, C, q[0], q[1], q[3], q[4], q[6], q[7], q[8]);
    }
    for (int T : {2, 3, 5}) { be.i3d_head(VARIANTS[0], 3, T); be.i3d_head(VARIANTS[1], 3, T); }
    for (int T : {4, 6}) be.i3d_head(VARIANTS[2], 3, T);
    const int IMAP[11][2] = {{5, 6}, {5, 6}, {5, 6}, {7, 9}, {5, 6}, {5, 6}, {5, 6}, {5, 6}, {7, 9}, {3, 4}, {3, 4}};
    for (int block = 0; block < 11; ++block) {
        be.inc_mixed(block, 2, IMAP[block][0], IMAP[block][1]);
        be.inc_mixed(block, 1, 1, 1);   // blocks B and D refuse a [1, 1] map
    }
}
// ---- end shared -------------------------------------------------------------------------------------------------------------

namespace {

using namespace i2v;

bool g_perturb = false;

// column tile of a conv (the one of 128, 64, 32 that pads Cout least, the wider on a tie) and grid rules, typed in again
long conv_grid(long M, int cout, int* nt) {
    int best = 128;
    for (int bn : {64, 32})
        if ((cout + bn - 1) / bn * bn < (cout + best - 1) / best * best) best = bn;
    *nt = best / 16;
    return (M + 127) / 128 * ((cout + best - 1) / best);
}
long flat_grid(long total) { return total + 255 < (256L << 20) ? (total + 255) / 256 : 1L << 20; }

const char* const KIND[7] = {"input", "conv", "i3dpool", "incpool", "avgpool", "globalavg", "timemean"};

struct PlanBackend {
    Out out;
    const char* names[TRUNK_NBUF] = {};   // a case's own names of buffers the caller brings

    std::string buf(const TrunkPlan& p, int id) {
        if (names[id]) return names[id];
        if (id == BUF_IN) return "in";
        if (id == BUF_OUT) return "out";
        if (id >= INC_TAP0) return fmt_id("tap%d", id - INC_TAP0);
        return fmt_id("ws+%zu", p.off[id]);
    }
    // one field of one step: the front pad of the first strided I3D unit, else the channel offset of the first concatenation slice
    void perturb(TrunkPlan& p) {
        for (Step& s : p.steps)
            if (s.kind == STEP_CONV && s.block < 0 && s.s[0] > 1) { ++s.p[1]; return; }
        for (Step& s : p.steps)
            if (s.outOff > 0) { s.outOff += 4; return; }
    }
    void steps(TrunkPlan& p) {
        if (g_perturb) perturb(p);
        for (const Step& s : p.steps) {
            Rec r;
            r.kind = KIND[s.kind]; r.unit = s.unit; r.blk = s.block; r.pool = s.pool;
            r.src = buf(p, s.src); r.dst = buf(p, s.dst);
            const int in[3] = {s.in.T, s.in.H, s.in.W}, o[3] = {s.out.T, s.out.H, s.out.W};
            for (int d = 0; d < 3; ++d) {
                r.in[d] = in[d]; r.out[d] = o[d]; r.k[d] = s.k[d]; r.s[d] = s.s[d]; r.p[d] = s.p[d];
                r.e[d] = s.kind == STEP_I3D_POOL ? s.e[d] : 0;
            }
            if (s.kind == STEP_GLOBAL_AVG) { r.in[1] = 1; r.in[2] = (int)s.in.pos(); }   // the kernel takes the positions flattened
            r.ics = s.inCS; r.ioff = s.inOff; r.ocs = s.outCS; r.ooff = s.outOff; r.C = s.C; r.relu = s.relu; r.chw = s.chw;
            const long B = p.B;
            switch (s.kind) {
            case STEP_INPUT: r.grid = flat_grid(B * s.out.pos()); break;
            case STEP_CONV: r.grid = conv_grid(B * s.out.pos(), s.C, &r.nt); break;
            case STEP_I3D_POOL: case STEP_INC_POOL: r.grid = flat_grid(B * s.out.pos() * (s.C / 4)); break;
            case STEP_AVGPOOL: r.grid = flat_grid(B * s.out.T * s.C); break;
            default: r.grid = flat_grid(B * s.C);
            }
            out.step(r);
        }
    }
    bool refused(const TrunkPlan& p) {
        if (p.status) out.line("refused code=%d msg=%s", p.status, p.error);
        return p.status != 0;
    }

    void i3d_trunk(const Variant& v, bool features, int B, int Tin, int T, int H, int W) {
        out.begin(fmt_id("i3d/%s/%s/B%d/T%d", v.name, features ? "features" : "logits", B, T));
        TrunkPlan p = i3d_plan<Carver>(I3dVariant{v.dt, v.pool_t, v.classes}, B, Tin, T, H, W, features);
        const bool bad = refused(p);
        out.line("bytes=%zu t_head=%d", bad ? (size_t)0 : p.total, bad ? 0 : p.t_head);
        if (!bad) {
            out.line("off inp=%zu x=%zu y=%zu tmp=%zu pooled=%zu cls=%zu", p.off[I3D_INP], p.off[I3D_X], p.off[I3D_Y], p.off[I3D_TMP], p.off[I3D_POOLED],
                     p.off[I3D_CLS]);
            steps(p);
        }
        out.end();
    }
    void inc_trunk(int B, int H, int W, int last, unsigned taps) {
        out.begin(fmt_id("inception/%dx%d/last%d/B%d/taps%x", H, W, last, B, taps));
        TrunkPlan p = inception_plan<Carver>(B, H, W, last, taps);
        const bool bad = refused(p);
        out.line("dims_ok=%d bytes=%zu", inc_dims_ok(H, W) ? 1 : 0, bad ? (size_t)0 : p.total);
        if (!bad) {
            out.line("off a=%zu b=%zu t0=%zu t1=%zu", p.off[INC_A], p.off[INC_B], p.off[INC_T0], p.off[INC_T1]);
            for (int k = 0; k <= last; ++k) out.line("block%d=%d,%d,%d", k, p.block[k].H, p.block[k].W, BLOCK_C[k]);
            steps(p);
        }
        out.end();
    }
    void i3d_unit(const Variant& v, int unit, const int* sh) {
        out.begin(fmt_id("i3d_unit/%s/u%d/%dx%dx%dx%d", v.name, unit, sh[0], sh[1], sh[2], sh[3]));
        const I3dVariant iv{v.dt, v.pool_t, v.classes};
        I3dUnitSpec u;
        i3d_unit_spec(iv, unit, &u);
        TrunkPlan p(sh[0]);
        i2v::i3d_unit(p, iv, unit, BUF_IN, (u.cin + 3) / 4 * 4, Map3{sh[1], sh[2], sh[3]}, BUF_OUT, u.cout + 20, 12, unit != I2V_I3D_UNIT_HEAD);
        out.line("shape cin=%d cout=%d out=%d,%d,%d", (u.cin + 3) / 4 * 4, u.cout, p.out.T, p.out.H, p.out.W);
        steps(p);
        out.end();
    }
    void i3d_mixed(const Variant& v, int block, const int* sh) {
        out.begin(fmt_id("i3d_mixed/%s/b%d/%dx%dx%dx%d", v.name, block, sh[0], sh[1], sh[2], sh[3]));
        TrunkPlan p(sh[0]);
        i2v::i3d_mixed(p, I3dVariant{v.dt, v.pool_t, v.classes}, block, BUF_IN, Map3{sh[1], sh[2], sh[3]}, BUF_OUT);
        p.carve<Carver>();
        out.line("bytes=%zu", p.total);
        steps(p);
        out.end();
    }
    void i3d_pool(const Variant& v, int B, int C, int kT, int k, int sT, int s, int T, int H, int W) {
        out.begin(fmt_id("i3d_pool/%s/k%d%ds%d%d/%dx%dx%d/c%d", v.name, kT, k, sT, s, T, H, W, C));
        TrunkPlan p(B);
        i2v::i3d_pool(p, I3dVariant{v.dt, v.pool_t, v.classes}, BUF_IN, BUF_OUT, C, Map3{T, H, W}, kT, k, sT, s);
        out.line("shape out=%d,%d,%d", p.out.T, p.out.H, p.out.W);
        steps(p);
        out.end();
    }
    void i3d_head(const Variant& v, int B, int T) {
        out.begin(fmt_id("i3d_head/%s/B%d/T%d", v.name, B, T));
        const I3dVariant iv{v.dt, v.pool_t, v.classes};
        names[I3D_POOLED] = "pooled"; names[I3D_CLS] = "ws+0";   // the entry takes `pooled` from the caller, its workspace is the cls slot
        for (int features = 1; features >= 0; --features) {
            TrunkPlan p(B);
            i2v::i3d_head(p, iv, BUF_IN, T, features != 0);
            if (!features) out.line("bytes=%zu", (p.floats[I3D_CLS] * 4 + 255) / 256 * 256);
            names[BUF_OUT] = features ? "feats" : "logits";
            steps(p);
        }
        names[I3D_POOLED] = names[I3D_CLS] = names[BUF_OUT] = nullptr;
        out.end();
    }
    void inc_mixed(int block, int B, int H, int W) {
        out.begin(fmt_id("inc_mixed/b%d/B%d/%dx%d", block, B, H, W));
        TrunkPlan p(B);
        if (i2v::inc_mixed(p, block, BUF_IN, Map3{1, H, W}, BUF_OUT, BUF_NONE)) p.carve<Carver>();
        if (!refused(p)) {
            const Block& b = inception_graph().blocks[block];
            out.line("shape cin=%d cout=%d out=%d,%d bytes=%zu", b.cin, b.cout, p.out.H, p.out.W, p.total);
            steps(p);
        }
        out.end();
    }
};

}  // namespace

int main(int argc, char** argv) {
    g_perturb = argc > 1 && !std::strcmp(argv[1], "--perturb");
    PlanBackend be;
    all_cases(be);
    std::printf("%ld cases\n", be.out.cases);
    return 0;
}
