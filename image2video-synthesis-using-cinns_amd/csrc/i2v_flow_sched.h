// cINN flow: what a pass does BETWEEN two coupling half-steps, and how the reference names the parameters -- the one copy of
// the host logic that every launch chain (i2v_flow.hip, i2v_flow_tile.hip; any future one) and the loaders consume.
// Plain C++, no HIP include: tests/flow_sched_check.cpp compiles it for the host and pins it to the reference's op order.
#pragma once
#include <string>
#include <vector>

namespace i2v {

// block `fl` is a mode-'cond' block: the first layers of its s- / t-nets see only the embedding (flow_blocks.py:24 with
// i2v_flow_cfg.control = 1; 2 = every block, the stand-alone coupling / flow-block modules in mode 'cond')
inline bool flow_block_cond(int control, int fl) { return control == 2 || (control == 1 && fl % 4 != 0); }

// state_dict key, without ".weight" / ".bias", of Linear `layer` (0 .. depth + 1; BasicFullyConnectedNet.main holds the Linear
// layers at the even indices, modules.py:14-24) of net 0 = s / 1 = t of half-step i of block fl
inline std::string flow_linear_key(int fl, int net, int i, int layer) {
    return "sub_layers." + std::to_string(fl) + ".coupling." + (net ? "t." : "s.") + std::to_string(i) + ".main." + std::to_string(2 * layer);
}

// One launch boundary of a pass: the coupling of half-step `step` (= 2 fl + i; -1: none, the link in front of the first
// half-step), then the elementwise ops up to the next half-step -- forward in the order Shuffle shuf_block, ActNorm an_block,
// InvLeakyRelu, half swap; reverse InvLeakyRelu^-1, ActNorm^-1 an_block, Shuffle^-1 shuf_block, half swap (block indices, -1:
// none) -- then the first Linear of half-step next_step (-1: none, the last link).
struct FlowLink {
    int step, shuf_block, an_block, next_step;
    bool lrelu, swap;
};

// The S + 1 = 2 n_flows + 1 links of a pass in launch order.  A block is ActNorm -> activation -> coupling -> Shuffle
// (flow_blocks.py:118-129), reversed Shuffle^-1 -> coupling^-1 -> activation^-1 -> ActNorm^-1 (:131-136); the coupling is
// half-step 0, cat(chunk[::-1]), half-step 1 (:84-92), reversed half-step 1, cat(chunk[::-1]), half-step 0 (:98-104).
inline std::vector<FlowLink> flow_schedule(int n_flows, bool reverse, bool use_an, bool use_act, bool use_shuf) {
    const int nf = n_flows, S = 2 * nf;
    // forward visits (fl, i) = (0,0),(0,1),(1,0)...; reverse visits (nf-1,1),(nf-1,0),(nf-2,1)...
    auto step_of = [&](int it) { return reverse ? S - 1 - it : it; };
    std::vector<FlowLink> links;
    // in front of the first half-step: ActNorm 0 + activation (:121-124) / Shuffle^-1 of the last block (:132)
    if (!reverse) links.push_back({-1, -1, use_an ? 0 : -1, step_of(0), use_act, false});
    else links.push_back({-1, use_shuf ? nf - 1 : -1, -1, step_of(0), false, false});
    for (int it = 0; it < S; ++it) {
        const int step = step_of(it), fl = step / 2, i = step % 2;
        FlowLink k{step, -1, -1, it + 1 < S ? step_of(it + 1) : -1, false, false};
        if (!reverse) {
            if (i == 0) k.swap = true;  // before half-step 1: cat(chunk[::-1]), flow_blocks.py:86-87
            else {                      // block boundary: Shuffle fl (:127), then ActNorm + activation of block fl + 1 (:121-124)
                if (use_shuf) k.shuf_block = fl;
                if (fl + 1 < nf) { if (use_an) k.an_block = fl + 1; k.lrelu = use_act; }
            }
        } else {
            if (i == 1) k.swap = true;  // before half-step 0 (flow_blocks.py:99-100)
            else {                      // block boundary: activation^-1, ActNorm^-1 of block fl (:134-135), Shuffle^-1 of block fl - 1 (:132)
                k.lrelu = use_act;
                if (use_an) k.an_block = fl;
                if (fl - 1 >= 0 && use_shuf) k.shuf_block = fl - 1;
            }
        }
        links.push_back(k);
    }
    return links;
}

}  // namespace i2v
