// The two metric trunks as data: the I3D networks (i2v_i3d.hip) and the FID Inception-v3 (i2v_inception.hip).  A plan is the list
// of launches of one call -- one Step per launch, with its maps, window, padding, channel slices and buffer ids -- and the floats
// every workspace slot takes.  i3d_plan / inception_plan build a whole trunk out of the same small builders the sub-module entries
// call (one conv unit, one max pool, one Mixed block, the I3D head), so the padding rules, the ceil-mode extents, the output maps,
// the concatenation offsets, the slot sizes and the ping-pong of the block-level buffers exist once.  The size and shape queries
// read a plan; the forwards hand it to their file's launch(), a loop over the steps.
// Plain C++, no HIP include: the carver comes in as a template argument (i2v_handle.h: Carver), and tests/trunk_plan_host_check.cpp
// prints every plan field for tests/test_host_trunk_plan.py.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/i2v_hip.h"

namespace i2v {

constexpr long TRUNK_SUB_MAX = 1L << 31;   // floats per tensor of a sub-module call

struct Map3 { int T, H, W; long pos() const { return (long)T * H * W; } };   // Inception: T = 1

enum StepKind { STEP_INPUT, STEP_CONV, STEP_I3D_POOL, STEP_INC_POOL, STEP_AVGPOOL, STEP_GLOBAL_AVG, STEP_TIME_MEAN };

// BUF_IN / BUF_OUT: the caller's input and output (logits, feats, the output of a sub-module call); I3D_* and INC_A .. INC_T1: the
// workspace slots, in the order they are carved; INC_TAP0 .. 3: the caller's block outputs
enum TrunkBuf { BUF_NONE = -1, BUF_IN, BUF_OUT, I3D_INP, I3D_X, I3D_Y, I3D_TMP, I3D_POOLED, I3D_CLS, INC_A, INC_B, INC_T0, INC_T1,
                INC_TAP0, INC_TAP1, INC_TAP2, INC_TAP3, TRUNK_NBUF };
constexpr int SLOT_FIRST = I3D_INP, SLOT_LAST = INC_T1;

struct Step {
    int kind = STEP_CONV;
    int block = -1, unit = -1;   // conv: I3D the I2V_I3D_UNIT_* index; Inception the Mixed block (-1: stem) and the conv of it
    int pool = -1;               // STEP_INC_POOL: I2V_INCEPTION_POOL_*
    int src = BUF_NONE, dst = BUF_NONE;
    Map3 in{1, 1, 1}, out{1, 1, 1};
    int k[3] = {1, 1, 1}, s[3] = {1, 1, 1}, p[3] = {0, 0, 0};   // window, stride, padding in FRONT per (T, H, W)
    int e[3] = {0, 0, 0};                                      // STEP_I3D_POOL: the padded extents (front + size + back)
    int inCS = 0, inOff = 0, outCS = 0, outOff = 0;            // channel stride and offset of the source and of the destination
    int C = 0;                                                 // channels written
    bool relu = false;
    bool chw = false;            // STEP_AVGPOOL: stored as [B][C][T'] (get_representation), else [B][T'][C]
};

struct TrunkPlan {
    int B = 0;
    std::vector<Step> steps;
    size_t floats[TRUNK_NBUF] = {}, off[TRUNK_NBUF] = {}, total = 0;   // per workspace slot; byte offsets and their total (carve)
    int t_head = 0;      // I3D: time steps behind the average pool
    Map3 block[4] = {};  // Inception: the map of every block output reached
    Map3 out{0, 0, 0};   // the map the last builder left
    int status = I2V_OK;
    char error[256] = "";

    explicit TrunkPlan(int batch, size_t max_steps = 16) : B(batch) { steps.reserve(max_steps); }   // one allocation per plan

    // The slot-sizing rule: a slot holds the largest tensor a step writes to it (its whole channel stride).  `slot` differs from
    // the destination where a caller's tap stands in for a ping-pong buffer: the size is counted as if it did not.
    void emit(const Step& s, int slot) {
        steps.push_back(s);
        if (slot >= SLOT_FIRST && slot <= SLOT_LAST) floats[slot] = std::max(floats[slot], (size_t)B * s.out.pos() * s.outCS);
        out = s.out;
    }
    void emit(const Step& s) { emit(s, s.dst); }
    __attribute__((format(printf, 2, 3))) bool fail(const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        std::vsnprintf(error, sizeof error, fmt, ap);
        va_end(ap);
        status = I2V_E_INVALID;
        return false;
    }
    // the two ping-pong slots of a trunk are interchangeable: both take the larger size
    void pair(int a, int b) { floats[a] = floats[b] = std::max(floats[a], floats[b]); }
    template <class Carver>
    void carve() {
        Carver c;
        for (int i = SLOT_FIRST; i <= SLOT_LAST; ++i) off[i] = c.take_floats(floats[i]);
        total = c.total();
    }
};

// The pointer behind every buffer id of a call: the caller's input and output, the workspace slots at the plan's offsets
struct TrunkBufs {
    float* p[TRUNK_NBUF] = {};
    TrunkBufs(const float* in, float* out) { p[BUF_IN] = const_cast<float*>(in); p[BUF_OUT] = out; }
    TrunkBufs& carve(const TrunkPlan& plan, void* ws) {
        for (int i = SLOT_FIRST; i <= SLOT_LAST; ++i) p[i] = reinterpret_cast<float*>(static_cast<char*>(ws) + plan.off[i]);
        return *this;
    }
};

// ---------------------------------------------------------------------------------------------------------------- I3D

constexpr int I3D_SIDE = 224;

struct I3dVariant {
    int dt;        // 0: Kinetics-400 network; 16 / 32: dynamic-texture network of that length
    int pool_t;    // time extent of the average pool
    int num_classes;
};

struct MixedSpec { const char* name; int cin; int o[6]; };   // o: branch_0, branch_1.0, branch_1.1, branch_2.0, branch_2.1, branch_3.1
const MixedSpec MIXED[9] = {
    {"mixed_3b", 192, {64, 96, 128, 16, 32, 32}},   {"mixed_3c", 256, {128, 128, 192, 32, 96, 64}},
    {"mixed_4b", 480, {192, 96, 208, 16, 48, 64}},  {"mixed_4c", 512, {160, 112, 224, 24, 64, 64}},
    {"mixed_4d", 512, {128, 128, 256, 24, 64, 64}}, {"mixed_4e", 512, {112, 144, 288, 32, 64, 64}},
    {"mixed_4f", 528, {256, 160, 320, 32, 128, 128}}, {"mixed_5b", 832, {256, 160, 320, 32, 128, 128}},
    {"mixed_5c", 832, {384, 192, 384, 48, 128, 128}}};
inline int i3d_mixed_out(int i) { return MIXED[i].o[0] + MIXED[i].o[2] + MIXED[i].o[4] + MIXED[i].o[5]; }

// (cin, cout, cubic kernel, stride) of unit index `unit` (I2V_I3D_UNIT_*); false for an unknown index
struct I3dUnitSpec { int cin, cout, k, s; };
inline bool i3d_unit_spec(const I3dVariant& v, int unit, I3dUnitSpec* u) {
    if (unit == I2V_I3D_UNIT_STEM) *u = {3, 64, 7, 2};
    else if (unit == I2V_I3D_UNIT_2B) *u = {64, 64, 1, 1};
    else if (unit == I2V_I3D_UNIT_2C) *u = {64, 192, 3, 1};
    else if (unit == I2V_I3D_UNIT_HEAD) *u = {1024, v.num_classes, 1, 1};
    else if (unit >= I2V_I3D_UNIT_MIXED && unit < I2V_I3D_UNIT_MIXED + 54) {
        const MixedSpec& m = MIXED[(unit - I2V_I3D_UNIT_MIXED) / 6];
        const int j = (unit - I2V_I3D_UNIT_MIXED) % 6;
        const int cin[6] = {m.cin, m.cin, m.o[1], m.cin, m.o[3], m.cin};
        *u = {cin[j], m.o[j], j == 2 || j == 4 ? 3 : 1, 1};
    } else return false;
    return true;
}

// "TF SAME" padding (get_padding_shape; Unit3D.compute_pad, MaxPool3dSamePadding.compute_pad) of a window s.k at stride s.s on the
// map s.in: k - stride zeros per dimension, or k - size % stride where that is not 0 -- a rule the Kinetics modules apply to the
// TIME dimension of a strided layer only, the dynamic-texture ones to every dimension; the smaller half in front.  Fills s.p and s.e.
inline void i3d_same_pad(const I3dVariant& v, Step& s) {
    const int size[3] = {s.in.T, s.in.H, s.in.W};
    for (int d = 0; d < 3; ++d) {
        const int mod = (d == 0 || v.dt) && s.s[d] > 1 ? size[d] % s.s[d] : 0;
        const int along = std::max(mod ? s.k[d] - mod : s.k[d] - s.s[d], 0);
        s.p[d] = along / 2;
        s.e[d] = size[d] + along;
    }
}
// MaxPool3d(ceil_mode=True, padding 0) on an extent e
inline int i3d_pool_out(int e, int k, int s) {
    int o = (e - k + s - 1) / s + 1;
    if ((o - 1) * s >= e) --o;
    return o;
}

// One conv unit with its own SAME padding: channels [0, cin) of src (stride inCS) -> [outOff, +cout) of dst (stride outCS)
inline bool i3d_unit(TrunkPlan& p, const I3dVariant& v, int unit, int src, int inCS, Map3 in, int dst, int outCS, int outOff, bool relu) {
    I3dUnitSpec u;
    if (!i3d_unit_spec(v, unit, &u)) return p.fail("i3d: unknown unit %d", unit);
    Step s;
    s.kind = STEP_CONV; s.unit = unit; s.src = src; s.dst = dst; s.in = in;
    for (int d = 0; d < 3; ++d) { s.k[d] = u.k; s.s[d] = u.s; }
    i3d_same_pad(v, s);
    s.out = Map3{(s.e[0] - u.k) / u.s + 1, (s.e[1] - u.k) / u.s + 1, (s.e[2] - u.k) / u.s + 1};
    s.inCS = inCS; s.outCS = outCS; s.outOff = outOff; s.C = u.cout; s.relu = relu;
    p.emit(s);
    return true;
}

// MaxPool3dTFPadding(kernel (kT, k, k), stride (sT, s, s)) on C channels: zeros in front and behind that take part in the maximum
inline bool i3d_pool(TrunkPlan& p, const I3dVariant& v, int src, int dst, int C, Map3 in, int kT, int k, int sT, int s_) {
    Step s;
    s.kind = STEP_I3D_POOL; s.src = src; s.dst = dst; s.in = in;
    s.k[0] = kT; s.k[1] = s.k[2] = k; s.s[0] = sT; s.s[1] = s.s[2] = s_;
    i3d_same_pad(v, s);
    s.out = Map3{i3d_pool_out(s.e[0], kT, sT), i3d_pool_out(s.e[1], k, s_), i3d_pool_out(s.e[2], k, s_)};
    s.inCS = s.outCS = s.C = C;
    p.emit(s);
    return true;
}

// Mixed block i: src [B][d][cin] -> dst [B][d][Co]; the branches store into their channel slice of dst (torch.cat((out_0, out_1,
// out_2, out_3), 1)), I3D_TMP holds one branch temporary at a time
inline bool i3d_mixed(TrunkPlan& p, const I3dVariant& v, int i, int src, Map3 d, int dst) {
    const MixedSpec& m = MIXED[i];
    const int u = I2V_I3D_UNIT_MIXED + 6 * i, C = m.cin, Co = i3d_mixed_out(i);
    return i3d_unit(p, v, u + 0, src, C, d, dst, Co, 0, true) &&
           i3d_unit(p, v, u + 1, src, C, d, I3D_TMP, m.o[1], 0, true) &&
           i3d_unit(p, v, u + 2, I3D_TMP, m.o[1], d, dst, Co, m.o[0], true) &&
           i3d_unit(p, v, u + 3, src, C, d, I3D_TMP, m.o[3], 0, true) &&
           i3d_unit(p, v, u + 4, I3D_TMP, m.o[3], d, dst, Co, m.o[0] + m.o[2], true) &&
           i3d_pool(p, v, src, I3D_TMP, C, d, 3, 3, 1, 1) &&
           i3d_unit(p, v, u + 5, I3D_TMP, C, d, dst, Co, m.o[0] + m.o[2] + m.o[4], true);
}

// AvgPool3d((pool_t, 7, 7)) on src [B][T][7][7][1024] -> I3D_POOLED [B][T'][1024], conv3d_0c_1x1 -> I3D_CLS [B][T'][classes], time
// mean -> BUF_OUT; with `features` only the pool, stored as [B][1024][T'] into BUF_OUT
inline bool i3d_head(TrunkPlan& p, const I3dVariant& v, int src, int T, bool features) {
    Step a;
    a.kind = STEP_AVGPOOL; a.src = src; a.dst = features ? BUF_OUT : I3D_POOLED;
    a.in = Map3{T, 7, 7}; a.out = Map3{T - v.pool_t + 1, 1, 1};
    a.k[0] = v.pool_t; a.k[1] = a.k[2] = 7;
    a.inCS = a.outCS = a.C = 1024; a.chw = features;
    p.emit(a);
    p.t_head = a.out.T;
    if (features) return true;
    if (!i3d_unit(p, v, I2V_I3D_UNIT_HEAD, I3D_POOLED, 1024, a.out, I3D_CLS, v.num_classes, 0, false)) return false;
    Step m;
    m.kind = STEP_TIME_MEAN; m.src = I3D_CLS; m.dst = BUF_OUT; m.in = a.out;
    m.inCS = m.outCS = m.C = v.num_classes;
    p.emit(m);
    return true;
}

// frames [B][Tin][3][H][W] -> logits, or with `features` -> the average pool's output [B][1024][T'].  T frames enter the network,
// frame t read from source frame t % Tin
template <class Carver>
TrunkPlan i3d_plan(const I3dVariant& v, int B, int Tin, int T, int H, int W, bool features) {
    TrunkPlan p(B, 76);
    Step in;
    in.kind = STEP_INPUT; in.src = BUF_IN; in.dst = I3D_INP;
    in.in = Map3{Tin, H, W}; in.out = Map3{T, I3D_SIDE, I3D_SIDE};
    in.inCS = 3; in.outCS = in.C = 4;
    p.emit(in);
    int x = I3D_X, y = I3D_Y;
    // conv3d_1a_7x7, maxPool3d_2a_3x3, conv3d_2b_1x1, conv3d_2c_3x3, maxPool3d_3a_3x3
    bool ok = i3d_unit(p, v, I2V_I3D_UNIT_STEM, I3D_INP, 4, p.out, x, 64, 0, true) && i3d_pool(p, v, x, y, 64, p.out, 1, 3, 1, 2) &&
              i3d_unit(p, v, I2V_I3D_UNIT_2B, y, 64, p.out, x, 64, 0, true) && i3d_unit(p, v, I2V_I3D_UNIT_2C, x, 64, p.out, y, 192, 0, true) &&
              i3d_pool(p, v, y, x, 192, p.out, 1, 3, 1, 2);
    for (int i = 0; ok && i < 9; ++i) {
        ok = i3d_mixed(p, v, i, x, p.out, y);
        std::swap(x, y);
        if (ok && i == 1) { ok = i3d_pool(p, v, x, y, i3d_mixed_out(i), p.out, 3, 3, 2, 2); std::swap(x, y); }   // maxPool3d_4a_3x3
        if (ok && i == 6) { ok = i3d_pool(p, v, x, y, i3d_mixed_out(i), p.out, 2, 2, 2, 2); std::swap(x, y); }   // maxPool3d_5a_2x2
    }
    if (!ok) return p;
    const Map3 d = p.out;
    if (!(d.H == 7 && d.W == 7 && d.T >= v.pool_t)) {
        p.fail("i3d: %d frames leave a [%d, %d, %d] map in front of AvgPool3d((%d, 7, 7)); at least %d frames are needed", T, d.T, d.H, d.W,
               v.pool_t, 8 * (v.pool_t - 1) + 1);
        return p;
    }
    if (!i3d_head(p, v, x, d.T, features)) return p;
    p.pair(I3D_X, I3D_Y);
    p.template carve<Carver>();
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- Inception-v3

constexpr int INC_SIDE = 299;
constexpr int INC_MIN = 75;   // the smallest input that leaves a 1 x 1 map in front of the final pool
constexpr int N_STEM = 5, N_MIXED = 11;
const int BLOCK_C[4] = {64, 192, 768, 2048};

struct ConvSpec { std::string name; int cin, cout, kh, kw, s, ph, pw; };

// every Mixed block is a short program over the block input X, the block output Y and two temporaries T0, T1
enum { X = 0, T0 = 1, T1 = 2, Y = 3 };
enum { OP_CONV = 0, OP_POOL = 1 };
struct Op { int op, arg, src, dst, off; };   // conv: arg = unit of the block; pool: arg = I2V_INCEPTION_POOL_*; off: channel offset in Y
struct Block { std::string name; int cin = 0, cout = 0; std::vector<ConvSpec> convs; std::vector<Op> ops; };

inline ConvSpec cs(const std::string& n, int cin, int cout, int kh = 1, int kw = 1, int s = 1, int ph = 0, int pw = 0) {
    return ConvSpec{n, cin, cout, kh, kw, s, ph, pw};
}

// torchvision InceptionA with the FID patch (avg pool without the padding in its divisor); cat: 1x1, 5x5, 3x3dbl, pool
inline Block block_a(const std::string& n, int cin, int pf) {
    Block b{n, cin, 224 + pf};
    b.convs = {cs(n + ".branch1x1", cin, 64), cs(n + ".branch5x5_1", cin, 48), cs(n + ".branch5x5_2", 48, 64, 5, 5, 1, 2, 2),
               cs(n + ".branch3x3dbl_1", cin, 64), cs(n + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1), cs(n + ".branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1),
               cs(n + ".branch_pool", cin, pf)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, Y, 64}, {OP_CONV, 3, X, T0, 0}, {OP_CONV, 4, T0, T1, 0},
             {OP_CONV, 5, T1, Y, 128}, {OP_POOL, I2V_INCEPTION_POOL_AVG, X, T0, 0}, {OP_CONV, 6, T0, Y, 224}};
    return b;
}
// torchvision InceptionB (unpatched); cat: 3x3, 3x3dbl, max pool of the input
inline Block block_b(const std::string& n, int cin) {
    Block b{n, cin, 480 + cin};
    b.convs = {cs(n + ".branch3x3", cin, 384, 3, 3, 2), cs(n + ".branch3x3dbl_1", cin, 64), cs(n + ".branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1),
               cs(n + ".branch3x3dbl_3", 96, 96, 3, 3, 2)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, T1, 0}, {OP_CONV, 3, T1, Y, 384},
             {OP_POOL, I2V_INCEPTION_POOL_MAX_S2, X, Y, 480}};
    return b;
}
// InceptionC with the FID patch; cat: 1x1, 7x7, 7x7dbl, pool
inline Block block_c(const std::string& n, int cin, int c7) {
    Block b{n, cin, 768};
    b.convs = {cs(n + ".branch1x1", cin, 192),
               cs(n + ".branch7x7_1", cin, c7), cs(n + ".branch7x7_2", c7, c7, 1, 7, 1, 0, 3), cs(n + ".branch7x7_3", c7, 192, 7, 1, 1, 3, 0),
               cs(n + ".branch7x7dbl_1", cin, c7), cs(n + ".branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0), cs(n + ".branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3),
               cs(n + ".branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0), cs(n + ".branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3),
               cs(n + ".branch_pool", cin, 192)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, T1, 0}, {OP_CONV, 3, T1, Y, 192},
             {OP_CONV, 4, X, T0, 0}, {OP_CONV, 5, T0, T1, 0}, {OP_CONV, 6, T1, T0, 0}, {OP_CONV, 7, T0, T1, 0}, {OP_CONV, 8, T1, Y, 384},
             {OP_POOL, I2V_INCEPTION_POOL_AVG, X, T0, 0}, {OP_CONV, 9, T0, Y, 576}};
    return b;
}
// torchvision InceptionD (unpatched); cat: 3x3, 7x7x3, max pool of the input
inline Block block_d(const std::string& n, int cin) {
    Block b{n, cin, 512 + cin};
    b.convs = {cs(n + ".branch3x3_1", cin, 192), cs(n + ".branch3x3_2", 192, 320, 3, 3, 2),
               cs(n + ".branch7x7x3_1", cin, 192), cs(n + ".branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3), cs(n + ".branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0),
               cs(n + ".branch7x7x3_4", 192, 192, 3, 3, 2)};
    b.ops = {{OP_CONV, 0, X, T0, 0}, {OP_CONV, 1, T0, Y, 0}, {OP_CONV, 2, X, T0, 0}, {OP_CONV, 3, T0, T1, 0}, {OP_CONV, 4, T1, T0, 0},
             {OP_CONV, 5, T0, Y, 320}, {OP_POOL, I2V_INCEPTION_POOL_MAX_S2, X, Y, 512}};
    return b;
}
// InceptionE with the FID patches: E_1 (Mixed_7b) the unpadded-divisor avg pool, E_2 (Mixed_7c) a MAX pool; cat: 1x1, 3x3 (2a, 2b),
// 3x3dbl (3a, 3b), pool
inline Block block_e(const std::string& n, int cin, int pool) {
    Block b{n, cin, 2048};
    b.convs = {cs(n + ".branch1x1", cin, 320),
               cs(n + ".branch3x3_1", cin, 384), cs(n + ".branch3x3_2a", 384, 384, 1, 3, 1, 0, 1), cs(n + ".branch3x3_2b", 384, 384, 3, 1, 1, 1, 0),
               cs(n + ".branch3x3dbl_1", cin, 448), cs(n + ".branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1),
               cs(n + ".branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1), cs(n + ".branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0),
               cs(n + ".branch_pool", cin, 192)};
    b.ops = {{OP_CONV, 0, X, Y, 0}, {OP_CONV, 1, X, T0, 0}, {OP_CONV, 2, T0, Y, 320}, {OP_CONV, 3, T0, Y, 704},
             {OP_CONV, 4, X, T0, 0}, {OP_CONV, 5, T0, T1, 0}, {OP_CONV, 6, T1, Y, 1088}, {OP_CONV, 7, T1, Y, 1472},
             {OP_POOL, pool, X, T0, 0}, {OP_CONV, 8, T0, Y, 1856}};
    return b;
}

// fid_inception_v3's graph.  The stem is a program too: its convs in order, a MaxPool2d(3, 2) behind Conv2d_2b_3x3 (the end of
// block 0) and behind Conv2d_4a_3x3 (the end of block 1)
struct InceptionGraph {
    ConvSpec stem[N_STEM];
    int stem_pool_behind[2] = {2, 4};
    Block blocks[N_MIXED];
};
inline const InceptionGraph& inception_graph() {
    static const InceptionGraph g = [] {
        InceptionGraph g;
        g.stem[0] = cs("Conv2d_1a_3x3", 3, 32, 3, 3, 2);
        g.stem[1] = cs("Conv2d_2a_3x3", 32, 32, 3, 3);
        g.stem[2] = cs("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
        g.stem[3] = cs("Conv2d_3b_1x1", 64, 80);
        g.stem[4] = cs("Conv2d_4a_3x3", 80, 192, 3, 3);
        g.blocks[0] = block_a("Mixed_5b", 192, 32);
        g.blocks[1] = block_a("Mixed_5c", 256, 64);
        g.blocks[2] = block_a("Mixed_5d", 288, 64);
        g.blocks[3] = block_b("Mixed_6a", 288);
        g.blocks[4] = block_c("Mixed_6b", 768, 128);
        g.blocks[5] = block_c("Mixed_6c", 768, 160);
        g.blocks[6] = block_c("Mixed_6d", 768, 160);
        g.blocks[7] = block_c("Mixed_6e", 768, 192);
        g.blocks[8] = block_d("Mixed_7a", 768);
        g.blocks[9] = block_e("Mixed_7b", 1280, I2V_INCEPTION_POOL_AVG);
        g.blocks[10] = block_e("Mixed_7c", 2048, I2V_INCEPTION_POOL_MAX_S1);
        return g;
    }();
    return g;
}

inline bool inc_dims_ok(int h, int w) { return h >= INC_MIN && w >= INC_MIN; }

// One BasicConv2d on the map `in`: floor-mode output with symmetric padding.  The map may come out empty: the callers refuse it in
// their own words
inline Step inc_conv_step(const ConvSpec& c, int block, int unit, int src, int inCS, int inOff, Map3 in, int dst, int outCS, int outOff) {
    Step s;
    s.kind = STEP_CONV; s.block = block; s.unit = unit; s.src = src; s.dst = dst; s.in = in;
    s.k[1] = c.kh; s.k[2] = c.kw; s.s[1] = s.s[2] = c.s; s.p[1] = c.ph; s.p[2] = c.pw;
    s.out = Map3{1, (in.H + 2 * c.ph - c.kh) / c.s + 1, (in.W + 2 * c.pw - c.kw) / c.s + 1};
    s.inCS = inCS; s.inOff = inOff; s.outCS = outCS; s.outOff = outOff; s.C = c.cout; s.relu = true;
    return s;
}
// One 3 x 3 pool of `kind` on C channels: MaxPool2d(3, 2) without padding, the two stride-1 pools with padding 1; floor mode
inline Step inc_pool_step(int kind, int src, int C, Map3 in, int dst, int outCS, int outOff) {
    Step s;
    s.kind = STEP_INC_POOL; s.pool = kind; s.src = src; s.dst = dst; s.in = in;
    const int stride = kind == I2V_INCEPTION_POOL_MAX_S2 ? 2 : 1, pad = kind == I2V_INCEPTION_POOL_MAX_S2 ? 0 : 1;
    s.k[1] = s.k[2] = 3; s.s[1] = s.s[2] = stride; s.p[1] = s.p[2] = pad;
    s.out = Map3{1, (in.H + 2 * pad - 3) / stride + 1, (in.W + 2 * pad - 3) / stride + 1};
    s.inCS = C; s.outCS = outCS; s.outOff = outOff; s.C = C;
    return s;
}
inline bool empty(Map3 m) { return m.H <= 0 || m.W <= 0; }

// Mixed block i: src [B][d][cin] -> dst [B][out][cout], the slot `slot` sized for it
inline bool inc_mixed(TrunkPlan& p, int i, int src, Map3 d, int dst, int slot) {
    const Block& b = inception_graph().blocks[i];
    const int buf[4] = {src, INC_T0, INC_T1, dst};
    int ch[4] = {b.cin, 0, 0, b.cout};   // channels of what each buffer holds
    Map3 dm[4] = {d, d, d, d};
    for (const Op& op : b.ops) {
        const int c = op.op == OP_CONV ? b.convs[op.arg].cout : ch[op.src];
        const int outCS = op.dst == Y ? b.cout : c;
        const Step s = op.op == OP_CONV ? inc_conv_step(b.convs[op.arg], i, op.arg, buf[op.src], ch[op.src], 0, dm[op.src], buf[op.dst], outCS, op.off)
                                        : inc_pool_step(op.arg, buf[op.src], c, dm[op.src], buf[op.dst], outCS, op.off);
        if (empty(s.out))
            return p.fail("inception %s: a [%d, %d] map is too small", (op.op == OP_CONV ? b.convs[op.arg].name : b.name).c_str(), d.H, d.W);
        p.emit(s, op.dst == Y ? slot : s.dst);
        dm[op.dst] = s.out;
        if (op.dst != Y) ch[op.dst] = c;
    }
    p.out = dm[Y];
    return true;
}

// x [B][H][W][4] -> blocks 0 .. last; tap k set in `taps`: block k goes to the caller's INC_TAP0 + k instead of a ping-pong slot
// (the slot sizes do not depend on it).  Block 3, the global average, always goes to its tap.
template <class Carver>
TrunkPlan inception_plan(int B, int H, int W, int last, unsigned taps) {
    TrunkPlan p(B, 112);
    const InceptionGraph& g = inception_graph();
    int cur = BUF_IN, C = 4;
    p.out = Map3{1, H, W};
    auto other = [&] { return cur == INC_A ? INC_B : INC_A; };
    auto finish = [&]() -> TrunkPlan& { p.pair(INC_A, INC_B); p.template carve<Carver>(); return p; };
    // blocks 0 and 1: Conv2d_1a_3x3, Conv2d_2a_3x3, Conv2d_2b_3x3, max pool; Conv2d_3b_1x1, Conv2d_4a_3x3, max pool
    for (int j = 0, blk = 0; j < N_STEM; ++j) {
        const Map3 d = p.out;
        const Step s = inc_conv_step(g.stem[j], -1, j, cur, C, 0, d, other(), g.stem[j].cout, 0);
        if (empty(s.out)) { p.fail("inception %s: a [%d, %d] map is too small", g.stem[j].name.c_str(), d.H, d.W); return p; }
        p.emit(s);
        cur = s.dst; C = s.C;
        if (j != g.stem_pool_behind[blk]) continue;
        const int slot = other();
        const Step q = inc_pool_step(I2V_INCEPTION_POOL_MAX_S2, cur, C, s.out, (taps >> blk & 1) ? INC_TAP0 + blk : slot, C, 0);
        if (empty(q.out)) { p.fail("inception: a [%d, %d] map is too small for MaxPool2d(3, 2)", s.out.H, s.out.W); return p; }
        p.emit(q, slot);
        cur = q.dst;
        p.block[blk] = q.out;
        if (last == blk++) return finish();
    }
    // block 2: Mixed_5b .. Mixed_6e; block 3: Mixed_7a .. Mixed_7c, the global average
    for (int i = 0; i < N_MIXED; ++i) {
        const int slot = other(), y = i == 7 && (taps >> 2 & 1) ? INC_TAP2 : slot;
        if (!inc_mixed(p, i, cur, p.out, y, slot)) return p;
        cur = y; C = g.blocks[i].cout;
        if (i == 7) {
            p.block[2] = p.out;
            if (last == 2) return finish();
        }
    }
    Step a;
    a.kind = STEP_GLOBAL_AVG; a.src = cur; a.dst = INC_TAP3; a.in = p.out; a.out = Map3{1, 1, 1};
    a.inCS = a.outCS = a.C = C;
    p.emit(a);
    p.block[3] = a.out;
    return finish();
}

}  // namespace i2v
