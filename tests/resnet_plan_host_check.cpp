// Host check of the launch plans of the motion encoder and the conditioning embedder (csrc/i2v_resnet_plan.h): prints, case by case,
// the workspace total, every slot offset, a refusal's code and text, and every step of the plan with all its fields -- kind, unit, form
// and packed set, buffers (as offsets into the workspace, or the caller's names), maps, channels, strides, ReLU, the grid of the
// networks' own kernels -- then one FNV-1a-64 digest over the case's lines.  tests/test_host_resnet_plan.py compiles it for the host
// (also with -fsanitize=address,undefined), compares the digests with tests/golden/resnet_plan_parent.json -- the same lines printed
// from the launches of the code before the plans existed -- walks the steps for slot liveness and compares the conv steps with the
// float64 oracles' convs.  `--perturb` changes one field of one step of every plan (the source slot of the first downsample conv, else
// the stride of the first strided step) before it is printed: the digests have to differ then.  Behind the cases it prints what the
// create-time rule of the encoder answers for every stride combination.  No device code, no HIP call.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "i2v_handle.h"
#include "i2v_resnet_plan.h"

// ---- shared: the printed record, the case list ------------------------------------------------------------------------------
struct Rec {
    const char* kind = "";
    int unit = -1;
    const char* form = "-";
    int set = 0;
    std::string src = "-", res = "-", dst = "-", dst16 = "-";
    int in[3] = {1, 1, 1}, out[3] = {1, 1, 1};
    int cin = 0, C = 0, ss = 1, st = 1, relu = 0;
    long grid = 0;   // the networks' own kernels only
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
        line("  %s u=%d form=%s set=%d %s+%s->%s|%s in=%d,%d,%d out=%d,%d,%d cin=%d C=%d s=%d,%d relu=%d grid=%ld", r.kind, r.unit, r.form, r.set,
             r.src.c_str(), r.res.c_str(), r.dst.c_str(), r.dst16.c_str(), r.in[0], r.in[1], r.in[2], r.out[0], r.out[1], r.out[2], r.cin, r.C, r.ss,
             r.st, r.relu, r.grid);
    }
    void end() {
        uint64_t h = 1469598103934665603ull;
        long n = 0;
        for (unsigned char c : text) { h = (h ^ c) * 1099511628211ull; n += c == '\n'; }
        std::printf("case %s\n%sdigest %s %016llx lines %ld\n", id.c_str(), text.c_str(), id.c_str(), (unsigned long long)h, n);
        ++cases;
    }
};
std::string fmt_id(const char* fmt, ...) {
    char b[200];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    return b;
}
long grid_cap(long total, long cap) { return (total + 255) / 256 < cap ? (total + 255) / 256 : cap; }

// name, channels, stride_s, stride_t: the eleven configurations of tests/encoder_cfgs.py, the two golden fixtures enc3d_bair /
// enc3d_land, and the two configurations of bench.py's encoder_latency
struct EncCfg { const char* name; int ch[5], ss[4], st[4]; };
const EncCfg ENC_CFGS[15] = {
    {"dtdb", {64, 64, 128, 256, 512}, {2, 2, 2, 2}, {1, 2, 2, 2}},      {"nodown_l0", {64, 64, 32, 48, 80}, {1, 2, 2, 2}, {1, 2, 2, 2}},
    {"t8", {64, 32, 32, 48, 64}, {1, 2, 2, 2}, {1, 2, 2, 2}},           {"t7_128", {64, 32, 32, 48, 64}, {2, 2, 2, 2}, {1, 2, 2, 2}},
    {"t3", {64, 32, 32, 48, 64}, {1, 2, 2, 2}, {1, 2, 2, 2}},           {"st2_ss1", {64, 32, 32, 48, 64}, {1, 2, 2, 2}, {2, 2, 2, 1}},
    {"st2_ss1_t1", {64, 32, 48, 64, 64}, {2, 2, 1, 2}, {2, 2, 2, 2}},   {"st1122", {64, 32, 48, 64, 32}, {2, 2, 2, 1}, {1, 1, 2, 2}},
    {"wide1024", {64, 64, 128, 512, 1024}, {1, 2, 2, 2}, {1, 2, 2, 2}}, {"c0_16", {16, 16, 32, 48, 80}, {1, 2, 2, 2}, {1, 2, 2, 2}},
    {"c0_80", {80, 48, 48, 64, 64}, {1, 2, 2, 2}, {1, 2, 2, 2}},
    {"enc3d_bair", {64, 128, 256, 512, 512}, {1, 2, 2, 2}, {1, 2, 2, 2}}, {"enc3d_land", {64, 128, 128, 256, 512}, {2, 2, 2, 2}, {1, 2, 2, 2}},
    {"bench_bair", {64, 128, 256, 512, 512}, {1, 2, 2, 2}, {1, 2, 2, 2}}, {"bench_land", {64, 128, 128, 256, 512}, {2, 2, 2, 2}, {1, 2, 2, 2}}};
constexpr int Z_DIM = 64;

// Every case, on a backend that prints it.  Encoder: every configuration x B 1, 3 x 1 .. 33 frames x 32 (refused), 64, 128, 256 and
// 64x128 frames; a sample (and eps) is asked for with B = 1 only.  Embedder: both norms x B 1, 2, 3, 5, 64 x h, w in 32 (refused),
// 64, 96 (refused), 128, 256.
template <class Backend>
void all_cases(Backend& be) {
    const int HW[5][2] = {{32, 32}, {64, 64}, {128, 128}, {256, 256}, {64, 128}};
    for (const EncCfg& c : ENC_CFGS)
        for (int B : {1, 3})
            for (int t = 1; t <= 33; ++t)
                for (const auto& hw : HW) be.encoder(c, B, t, hw[0], hw[1], B == 1);
    const int SIDES[5] = {32, 64, 96, 128, 256};
    for (int bn = 0; bn < 2; ++bn)
        for (int B : {1, 2, 3, 5, 64})
            for (int h : SIDES)
                for (int w : SIDES) be.embedder(bn, B, h, w);
}
// ---- end shared -------------------------------------------------------------------------------------------------------------

namespace {

using namespace i2v;

bool g_perturb = false;

const char* const KIND[9] = {"stem", "resize", "s2d", "conv", "norm", "maxpool", "mean", "head", "reparam"};
const char* const FORM[3] = {"f16", "s2d", "f32"};
const char* const NORM[3] = {"group16", "instance", "batch"};

struct PlanBackend {
    Out out;

    static std::string buf(const ResnetPlan& p, int id) {
        static const char* const CALLER[6] = {"in", "out", "eps", "sample", "mu", "logvar"};
        if (id < 0) return "-";
        if (id < RES_SLOT_FIRST) return CALLER[id];
        return fmt_id("ws+%zu", p.off[id]);
    }
    // one field of one step: the source slot of the first downsample conv, else the stride of the first strided step
    static void perturb(ResnetPlan& p) {
        const bool enc = p.norm == RN_GROUP16;
        for (ResStep& s : p.steps)
            if (s.kind == RS_CONV && (enc ? s.unit % 3 == 2 : s.unit > 0 && (s.unit - 1) % 4 == 3)) { s.src = s.src == RB_F0 ? RB_F1 : RB_F0; return; }
        for (ResStep& s : p.steps)
            if (s.ss > 1 || s.st > 1) { ++s.ss; return; }
    }
    void plan(ResnetPlan& p) {
        if (p.status) { out.line("refused code=%d msg=%s", p.status, p.error); return; }
        if (g_perturb) perturb(p);
        out.line("norm=%s", NORM[p.norm]);
        const long B = p.B;
        for (const ResStep& s : p.steps) {
            Rec r;
            r.kind = KIND[s.kind];
            r.unit = s.kind == RS_NORM && p.norm == RN_INSTANCE ? -1 : s.unit;   // InstanceNorm has no parameters: no unit is read
            if (s.form >= 0) r.form = FORM[s.form];
            r.set = s.set;
            r.src = buf(p, s.src); r.res = buf(p, s.res); r.dst = buf(p, s.dst); r.dst16 = buf(p, s.dst16);
            const int in[3] = {s.in.T, s.in.H, s.in.W}, o[3] = {s.out.T, s.out.H, s.out.W};
            for (int d = 0; d < 3; ++d) { r.in[d] = in[d]; r.out[d] = o[d]; }
            r.cin = s.cin; r.C = s.C; r.ss = s.ss; r.st = s.st; r.relu = s.relu;
            switch (s.kind) {   // the grids of the networks' own kernels, typed in again
            case RS_STEM: r.grid = 1024; break;
            case RS_S2D: r.grid = grid_cap(B * s.out.pos() * (s.st * 4) * (s.cin / 8), 16384); break;
            case RS_MAXPOOL: r.grid = grid_cap(B * s.out.pos() * (s.C / 4), 65536); break;
            case RS_MEAN: case RS_REPARAM: r.grid = (B * s.C + 255) / 256; break;
            default: break;
            }
            out.step(r);
        }
    }
    void encoder(const EncCfg& c, int B, int t, int h, int w, bool sample) {
        out.begin(fmt_id("enc/%s/B%d/t%d/%dx%d", c.name, B, t, h, w));
        i2v_encoder3d_cfg cfg{};
        cfg.z_dim = Z_DIM;
        for (int i = 0; i < 5; ++i) cfg.channels[i] = c.ch[i];
        for (int i = 0; i < 4; ++i) { cfg.stride_s[i] = c.ss[i]; cfg.stride_t[i] = c.st[i]; }
        ResnetPlan p = enc3d_plan<Carver>(cfg, B, t, h, w, sample);
        out.line("bytes=%zu", p.total);
        out.line("off f=%zu,%zu,%zu,%zu h=%zu,%zu,%zu sums=%zu coef=%zu ml=%zu", p.off[RB_F0], p.off[RB_F1], p.off[RB_F2], p.off[RB_F3], p.off[RB_H0],
                 p.off[RB_H1], p.off[RB_H2], p.off[RB_SUMS], p.off[RB_COEF], p.off[RB_ML]);
        plan(p);
        out.end();
    }
    void embedder(int bn, int B, int h, int w) {
        out.begin(fmt_id("emb/%s/B%d/%dx%d", bn ? "bn" : "in", B, h, w));
        ResnetPlan p = embedder_plan<Carver>(bn, B, h, w, Z_DIM);
        out.line("bytes=%zu", p.total);
        out.line("off img=%zu f=%zu,%zu,%zu,%zu,%zu sums=%zu coef=%zu pooled=%zu", p.off[RB_IMG], p.off[RB_F0], p.off[RB_F1], p.off[RB_F2], p.off[RB_F3],
                 p.off[RB_F4], p.off[RB_SUMS], p.off[RB_COEF], p.off[RB_POOLED]);
        plan(p);
        out.end();
    }
};

}  // namespace

int main(int argc, char** argv) {
    g_perturb = argc > 1 && !std::strcmp(argv[1], "--perturb");
    PlanBackend be;
    all_cases(be);
    std::printf("%ld cases\n", be.out.cases);
    // the create-time rule: every stride combination at equal and at changing widths
    for (int eq = 0; eq < 2; ++eq)
        for (int m = 0; m < 256; ++m) {
            i2v_encoder3d_cfg cfg{};
            for (int i = 0; i < 5; ++i) cfg.channels[i] = eq ? 64 : 32 + 16 * i;
            for (int i = 0; i < 4; ++i) { cfg.stride_s[i] = 1 + (m >> i & 1); cfg.stride_t[i] = 1 + (m >> (4 + i) & 1); }
            std::printf("create %s ss=%d,%d,%d,%d st=%d,%d,%d,%d layer=%d\n", eq ? "equal" : "changing", cfg.stride_s[0], cfg.stride_s[1], cfg.stride_s[2],
                        cfg.stride_s[3], cfg.stride_t[0], cfg.stride_t[1], cfg.stride_t[2], cfg.stride_t[3], i2v::enc3d_halfrate_without_down(cfg));
        }
    return 0;
}
