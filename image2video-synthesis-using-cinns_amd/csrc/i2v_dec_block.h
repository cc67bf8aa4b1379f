// One GeneratorBlock of the stage-1 decoder (decoder.py:33-52; launch sequence: i2v_dec.hip) and what both of its users -- the decoder
// handle (i2v_dec.hip: six blocks) and the stand-alone block handle (i2v_gblock.hip: one) -- share: the weights of a block, the
// per-handle context the block code reads, the packers, and the status words of the range guard.
#pragma once
#include <string>
#include <vector>

#include "i2v_dec_writers.h"
#include "i2v_handle.h"

namespace i2v {

// The kernel a 3x3x3 block conv runs.  The values are the codes i2v_dec_get_layer_profile reports.
enum Conv3Kernel : int { K_F32 = 0, K_F16 = 1, K_F23 = 2, K_F43 = 3, K_F43_GEN = 4, K_F32_WINO = 5, K_F43_ONE = 6 };
constexpr unsigned bit(Conv3Kernel k) { return 1u << k; }
constexpr bool is_split(Conv3Kernel k) { return k != K_F32 && k != K_F32_WINO; }   // reads a split-fp16 (or one-term fp16) operand

// One 3x3x3 block conv (conv_0 or conv_1) and the weights of every kernel variant packed for it
struct Conv3 {
    int cin = 0, cout = 0;
    // conv_0 behind a x2 temporal up-sampling.  SPADE's output is identical for frames 2i and 2i+1 (gamma/beta do not depend on t):
    // the split-fp16 variants run on the half-rate tensor with two pre-summed 2-tap temporal kernels (-1/3 of the MACs)
    bool tdup = false;
    ConvWeights f32;          // exact fp32, direct 27-tap kernel
    Wino4F32Weights wf;       // exact fp32, Winograd F(4,3) on the fp32 matrix cores (i2v_wino32.hip), next to f32
    Conv16Weights d16;        // split-fp16, direct kernel
    Wino16Weights w23;        // split-fp16, Winograd F(2,3) (packed where the shape allows)
    Wino4Weights w43;         // Winograd F(4,3) (i2v_conv16w4.hip), packed INSTEAD of the F(2,3) one: split-fp16, or (w43.one) the
                              // one-term fp16 form of mma = 3
};

struct Block {
    std::string name;
    int n_in = 0, n_out = 0, n_mid = 0;
    bool learned = false;
    int groups_spade = 16;
    Conv3 conv[2];              // conv_0: n_in -> n_mid, conv_1: n_mid -> n_out
    ConvWeights convs, sp_conv, sp_gb;
    Conv16Weights sp_conv16;  // SPADE's Conv2d(3, 128, 3) with the 3 input channels zero-padded to 8 (split-fp16 mode)
    Conv16Weights sp_gb16;      // split-fp16 variant (cfg.mma == 1)
    Conv16Weights convs16;      // the learned shortcut's 1x1x1 conv on split-fp16 operands (pointwise16_forward)
    Wino16Weights sp_gb_w;      // SPADE's fused gamma|beta Conv2d(128, 2C, 3) on the Winograd kernel (1x3x3 variant)
    Wino4Weights sp_gb_w4;      // ... on the F(4,3) kernel (packed INSTEAD where the shape allows: W % 16 == 0, H % 32 == 0)
    DevBuf gn_w, gn_b;
    int spade_form = -1;        // SpadeForm of the last spade_branch call (-1: none yet)
    int zoff = 0;  // offset of this block's ADAIN (gamma|beta) in the z-GEMM output
};

// The form SPADE's branch takes (spade_branch): the codes i2v_dec_get_spade_form reports
enum SpadeForm : int { SPADE_F43 = 0, SPADE_F23 = 1, SPADE_DIRECT16 = 2, SPADE_F32 = 3 };

struct Level { int T, H, W, ut, us; };  // resolution a block runs at and the upsample factors in front of it

// What the block code reads of the handle it runs for: the matrix-core mode, the environment switches, the status words of the range
// guard, the debug tap and the profile of the 3x3x3 launches.
struct BlockCtx {
    // Matrix-core mode (i2v_dec_cfg.mma): 0 exact fp32, 1 split-fp16, 2 AUTO = split-fp16 with a per-layer fallback behind the range
    // guard (i2v_dec.hip: dec_forward), 3 ("fp16") = the launches of mma = 1, except that the 3x3x3 block convs on the F(4,3) kernel run
    // its one-term form (conv_wino4_f16_kernel: fp16 operands, one MFMA per product) on the one-term operand (modulate_wino4_kernel<GB, true>)
    int mma = 0;
    bool fp32_layer[12] = {};   // mma = auto: layer = 2 * block + (0: conv_0, 1: conv_1) was switched to the exact-fp32 kernels
    bool fp32_all = false;
    bool has16() const { return mma != 0; }                           // split-fp16 weights are packed
    bool has32() const { return mma == 0 || mma == 2; }               // exact-fp32 weights are packed
    bool one16() const { return mma == 3; }                           // the F(4,3) block convs run one-term fp16
    bool aux16() const { return has16() && !fp32_all; }               // SPADE branch, shortcut GEMM, conv_img, resize on the split-fp16 path
    bool layer16(int layer) const { return aux16() && !fp32_layer[layer]; }
    // environment switches (read_switches)
    int wino = 1;  // 1: 3x3x3 convs whose shape allows it use the Winograd kernel (env I2V_DEC_WINO=0 disables)
    int wino4 = 1; // 1: F(4,3) Winograd kernel where the shape allows and one sample gives >= 32 workgroups (env I2V_DEC_WINO4=0: F(2,3); 2: wherever the shape allows)
    int spw = 1;   // 1: SPADE's gamma|beta conv uses the Winograd kernel where the shape allows (env I2V_DEC_SPW=0: direct kernel)
    int gen = 0;   // 1: the thin F(4,3) layers of the 128 x 128 configs (g_4: 32 output channels at 16 x 128 x 128) generate their operand in the
                   // conv kernel's own producer waves instead of reading a V tensor an operand-writer launch wrote (i2v_conv16w4g.hip; same
                   // bits).  env I2V_DEC_GEN.  Measured in profiles/r06_*_thin_fused_*.
    int wino32 = 1;  // exact-fp32 mode (mma = 0): 1 = 3x3x3 convs from the 8x8 level on run Winograd F(4,3) on the fp32 matrix cores (env I2V_DEC_WINO32=0: direct kernel)
    int pw16 = 1;  // 1: split-fp16 mode runs the shortcut convs on split-fp16 operands too (env I2V_DEC_PW16=0: exact-fp32 MFMA)
    int img16 = 2;  // split-fp16 mode: 2 fused matrix-core kernel (i2v_convimg.hip), 1 round 2's 81-plane GEMM + gather at nf >= 64, 0 vector-ALU kernel (env I2V_DEC_IMG16)
    int sub = 0;   // samples per sub-batch of the last two levels (env I2V_DEC_SUB; 0: the whole batch per launch)
    int overlap = 1;            // env I2V_DEC_OVERLAP=0: no side stream (i2v_dec.hip: SideStream)
    int no_side_shortcut = 0;   // env I2V_DEC_OVERLAP=2: branches on the side stream, shortcuts inline (A/B of the two halves)
    int device = 0;             // the device the packed weights live on (the handle's `device` is a reference to it)
    int* status_dev = nullptr;  // sticky range flag of the hl16 producers (device) ...
    int* status_host = nullptr; // ... and its pinned host mirror, refreshed asynchronously at the end of every forward
    // debug tap: copy one intermediate (channels-last) of one block out of the workspace during forward
    int tap_block = -1, tap_which = -1;
    float* tap_dst = nullptr;
    size_t tap_max = 0;
    // profile: event pairs around the 3x3x3 launches (ProfScope), resolved by i2v_dec_get_profile
    int profile = 0;
    struct ProfEv { hipEvent_t e0, e1; double flops, exec_flops; int layer; };
    std::vector<ProfEv> prof_events;
    // per-layer totals of the profiled 3x3x3 launches: layer = 2 * block + (0: conv_0, 1: conv_1)
    struct ProfLayer { double ms = 0, flops = 0, exec_flops = 0; long launches = 0; int kernel = 0; long grid = 0; };
    ProfLayer prof_layers[12];
    int prof_cur_layer = 0, prof_cur_kernel = 0;

    BlockCtx() = default;
    BlockCtx(const BlockCtx&) = delete;
    BlockCtx& operator=(const BlockCtx&) = delete;
    ~BlockCtx() {
        if (status_dev) (void)hipFree(status_dev);
        if (status_host) (void)hipHostFree(status_host);
    }
    // i2v_dec_status / i2v_gblock_status: the flag word once everything on `st` has run, optionally cleared
    int status(int32_t* flags, int32_t reset, hipStream_t st, const char* what);
};

struct BlockBufs {
    float *a, *dx, *xs_in, *xs_low, *y0, *y1, *gb, *coef;
    double *sums1, *sums2;        // sums1: statistics of the block INPUT (filled by the previous block's conv_1 epilogue or by run_stats)
    double* sums_out = nullptr;   // where conv_1's epilogue accumulates the statistics of the block OUTPUT (null: into sums1)
    float* splitk = nullptr;      // split-K scratch of conv16_forward (optional)
    size_t splitk_floats = 0;
    float* y1v = nullptr;         // Winograd operand of SPADE's 128-channel activation (2 x the size of y1; optional)
    const float* gb_ready = nullptr;   // this block's gamma | beta, already computed by i2v_dec_prepare
    float* m6 = nullptr;          // exact-fp32 Winograd scratch (six partial outputs); null: the direct kernel is used
    hipStream_t side = nullptr;   // the learned shortcut runs on this stream, with coef_s and the two events:
    float* coef_s = nullptr;
    hipEvent_t ev_x = nullptr, ev_s = nullptr;   // block input and its statistics complete (caller's stream) / shortcut complete (side stream)
    GbRows rows;                  // realizations: rows.k samples share a start frame; img / gb / gb_ready then hold the launch's FRAMES
};

// Would a conv of (cin, cout, tdup) at this level run kernel `kn` (K_F43, K_F23 or K_F32_WINO) under the handle's switches, the
// split-fp16 kernel it would run, and the same question for SPADE's gamma|beta conv: the predicates of packing and of the workspace
bool conv3_wants(const BlockCtx* d, const Conv3& c, const Level& l, Conv3Kernel kn);
Conv3Kernel conv3_split_kernel(const BlockCtx* d, const Conv3& c, const Level& l);
bool spade_w4_wanted(const BlockCtx* d, const Block& b, const Level& l);
bool spade_wino_wanted(const BlockCtx* d, const Block& b, const Level& l);

// ibs: floats between the samples of `img` (0: dense [B][3][H][W]); k: the decoder block whose debug taps 13 .. 15 the branch serves
// (-1: none).  Records the form it took in b.spade_form (i2v_dec_get_spade_form).
int spade_branch(BlockCtx* d, Block& b, const Level& l, const float* img, int img_h, int img_w, long ibs, int B, float* y0, float* y1,
                 float* y1v, float* gb, hipStream_t st, int k = -1);
int block_forward(BlockCtx* d, int k, Block& b, const Level& l, const float* x, float* xn, const float* img, int img_h, int img_w, long ibs,
                  const float* zl, int zstride, int B, const BlockBufs& w, bool& x_stats_ready, bool last, hipStream_t st);

// load time: spectral norm folded (W / sigma), then the packers of the kernels' weight formats
template <class WT>
int sn_pack(const StateDict& sd, const std::string& name, bool spectral, int cout, int cin, int k, bool has_bias, WT& out);
int pack_conv3(const StateDict& sd, const std::string& name, bool spectral, Conv3& c, unsigned variants);
int pack_spade(const StateDict& sd, const std::string& p, Block& b, bool gb16, bool gb32, bool gb_w4, bool gb_w);

// creation time
void read_switches(BlockCtx* d, bool whole);
void init_convs(Block& b, bool tdup);
int init_status(BlockCtx* d);
int check_range(const BlockCtx* d, const char* what);
// the entry scope of a decoder / block call that enqueues work: Entry::check (handle, device, weights), then the sticky range flag
template <class H>
int check_entry(Entry& sc, const H* h, unsigned flags, const char* what) {
    if (int rc = sc.check(h, flags, what)) return rc;
    return check_range(&h->ctx, what);
}

}  // namespace i2v
