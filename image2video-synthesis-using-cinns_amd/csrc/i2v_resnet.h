// What the motion encoder and the conditioning embedder run a plan (i2v_resnet_plan.h) with: one conv description whose kernel form
// is fixed at load, the norm parameters, the pointer behind every slot of a call, and the launch loop (i2v_resnet.hip).
#pragma once
#include "i2v_conv.h"
#include "i2v_resnet_plan.h"

namespace i2v {

// The pointer behind every slot id of a call: the caller's tensors, the workspace slots at the plan's offsets
struct ResBufs {
    void* p[RES_NBUF] = {};
    const float* stem_w = nullptr;   // RS_STEM: the encoder's stem weights [tap][cin][c0]
    ResBufs(const ResnetPlan& plan, void* ws) {
        for (int i = RES_SLOT_FIRST; i <= RES_SLOT_LAST; ++i) p[i] = static_cast<char*>(ws) + plan.off[i];
    }
    ResBufs& caller(int id, const void* ptr) { p[id] = const_cast<void*>(ptr); return *this; }
    template <class T = float>
    T* at(int id) const { return id < 0 ? nullptr : static_cast<T*>(p[id]); }
};

// One conv of a residual network.  pack() chooses the form (res_conv_form) and packs what that form reads; run() is the one call
// site of conv16_forward / conv_forward for both networks.
struct ResConv {
    int form = RC_F32;
    Conv16Weights w16[2];   // RC_F16: [0]; RC_S2D: [0] for the conv's own temporal stride, [1] the single-frame set (stride_t 2 only)
    ConvWeights w32;        // RC_F32
    // w: torch layout [cout][cin][kt][kh][kw]; ss, st: spatial / temporal stride
    int pack(const float* w, int cout, int cin, int kt, int kh, int kw, int ss, int st, const float* bias = nullptr);
    int run(const ResStep& s, const ResBufs& b, int B, hipStream_t st) const;
};

// Norm parameters of one unit.  Encoder: GroupNorm weight / bias.  Embedder: BatchNorm folded to (A,B) pairs per channel in `w`, or
// nothing (InstanceNorm).
struct ResNorm { DevBuf w, b; };

// Runs the steps of a plan in order on `st`
int launch(const ResnetPlan& plan, const std::vector<ResConv>& convs, const std::vector<ResNorm>& norms, const ResBufs& b, hipStream_t st);

}  // namespace i2v
