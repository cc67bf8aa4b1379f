// VGG-16 `features` trunk: the layer table and the one walk over it.  vgg_plan(N, H, W) gives every layer's map, where its output
// and the output of a pool behind it go, and the sizes and offsets of the three buffers the trunk's entries take (the forward
// workspace, the saved state of the backward pass, the backward workspace).  The size queries, the forward with and without
// saved state, the backward's geometry and i2v_vgg_saved_layout all read it (i2v_vgg.hip).
// Plain C++, no HIP include: the carver comes in as a template argument (i2v_handle.h: Carver), and
// tests/vgg_plan_host_check.cpp pins the plan to the rules the entries used to spell out one by one.
#pragma once
#include <algorithm>
#include <cstddef>

namespace i2v {

// torchvision vgg16().features: index of every conv, its widths, and whether a tap / a pool follows its ReLU
struct LayerSpec { int idx, cin, cout, tap, pool; };
const LayerSpec VGG_LAYERS[13] = {
    {0, 3, 64, -1, 0},    {2, 64, 64, 0, 1},                             // slice1: relu1_2, then MaxPool (features.4, head of slice2)
    {5, 64, 128, -1, 0},  {7, 128, 128, 1, 1},                           // relu2_2
    {10, 128, 256, -1, 0}, {12, 256, 256, -1, 0}, {14, 256, 256, 2, 1},  // relu3_3
    {17, 256, 512, -1, 0}, {19, 512, 512, -1, 0}, {21, 512, 512, 3, 1},  // relu4_3
    {24, 512, 512, -1, 0}, {26, 512, 512, -1, 0}, {28, 512, 512, 4, 0}}; // relu5_3 (features.30, the last pool, is not part of slice5)
const int VGG_TAP_C[5] = {64, 128, 256, 512, 512};

// four pools: a side below 16 leaves an empty map
inline bool vgg_dims_ok(int h, int w) { return (h >> 4) > 0 && (w >> 4) > 0; }
constexpr long VGG_MAX_FLOATS = 1L << 40;   // what the entries accept as one tensor

enum VggBuf { VGG_BUF_TAP, VGG_BUF_A, VGG_BUF_B, VGG_BUF_SAVED };   // the caller's tap, workspace slot a / b, the saved buffer

struct VggLayerPlan {
    int h, w, cin, cout;   // the map the conv runs on (a pool behind it halves it, floor mode, for the next layer)
    int tap;               // the tap its output is, or -1
    bool pool;
    VggBuf ws_dst;         // where the output goes when no state is saved: the tap, or slot a / b
    size_t saved_off;      // byte offset in the saved buffer (a tap has no room there: the offset of the next layer that has)
    VggBuf pool_dst;       // where the pool behind it writes
    // where the output goes: a conv that feeds a tap writes the caller's tap buffer; every other conv writes the saved buffer when
    // state is kept, else the workspace slot
    VggBuf dst(bool saved) const { return tap >= 0 ? VGG_BUF_TAP : saved ? VGG_BUF_SAVED : ws_dst; }
};

struct VggPlan {
    VggLayerPlan layer[13];
    size_t ws_a = 0, ws_b = 0, ws_bytes = 0;      // forward workspace: byte offsets of the slots, total
    size_t saved_bytes = 0;
    size_t bwd_a = 0, bwd_b = 0, bwd_bytes = 0;   // backward workspace: two gradient maps of the largest size (relu1_x)
};

// Buffer rule of the trunk: a conv that does not feed a tap writes workspace slot a, or b when it reads a; a pool always writes a
// (its source is a tap buffer).  Saved state: the eight post-ReLU activations that are not taps, in layer order, each slot carved
// (the five taps stay with the caller).
template <class Carver>
VggPlan vgg_plan(int N, int H, int W) {
    VggPlan p{};
    if (N <= 0 || !vgg_dims_ok(H, W)) return p;   // nothing to run: every total is 0, what the size queries answer
    size_t floats[4] = {};                        // per VggBuf: the largest map it takes (the two workspace slots are sized by it)
    Carver saved;
    int h = H, w = W;
    VggBuf in = VGG_BUF_TAP;   // where the layer's input lies (the caller's x is no workspace slot either)
    for (int l = 0; l < 13; ++l) {
        const LayerSpec& s = VGG_LAYERS[l];
        VggLayerPlan& L = p.layer[l];
        const size_t of = (size_t)N * h * w * s.cout;
        L.h = h; L.w = w; L.cin = s.cin; L.cout = s.cout; L.tap = s.tap; L.pool = s.pool != 0;
        L.ws_dst = in = s.tap >= 0 ? VGG_BUF_TAP : in == VGG_BUF_A ? VGG_BUF_B : VGG_BUF_A;
        L.saved_off = s.tap >= 0 ? saved.total() : saved.take_floats(of);
        floats[in] = std::max(floats[in], of);
        L.pool_dst = VGG_BUF_A;
        if (s.pool) {
            h /= 2; w /= 2;
            in = L.pool_dst;
            floats[in] = std::max(floats[in], (size_t)N * h * w * s.cout);
        }
    }
    Carver ws, bwd;
    p.ws_a = ws.take_floats(floats[VGG_BUF_A]); p.ws_b = ws.take_floats(floats[VGG_BUF_B]); p.ws_bytes = ws.total();
    p.saved_bytes = saved.total();
    const size_t g = (size_t)N * H * W * VGG_LAYERS[0].cout;
    p.bwd_a = bwd.take_floats(g); p.bwd_b = bwd.take_floats(g); p.bwd_bytes = bwd.total();
    return p;
}

}  // namespace i2v
