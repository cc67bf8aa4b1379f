// The decoder's operand writers and range guard (i2v_dec_writers.hip): the kernels that turn a block conv's input
// lrelu((x A + B) gamma' + beta) into the operand format of the conv kernel that reads it, and the status words they publish into.
#pragma once
#include "i2v_conv.h"

namespace i2v {

// Underflow side of the range guard.  The lo part of a split-fp16 operand is an fp16 subnormal for |x| < 2^-3, i.e. the format
// has an ABSOLUTE error floor of ~2^-25: a conv whose whole operand tensor sits below ~2^-11 loses the 1e-4 gate (measured:
// INTEGRATION.md §3) although nothing overflows.  Every operand writer therefore publishes the largest |activation| it wrote
// (before the Winograd transform) into its own slot (float bits, atomicMax); status_finish_kernel turns "non-zero tensor whose
// maximum is below I2V_UNDERFLOW_MAX" into status bit 1 (value 2) at the end of the forward.
constexpr float I2V_UNDERFLOW_MAX = 0x1p-10f;
constexpr float I2V_OVERFLOW_MAX = 6400.f;   // |V| <= 10 max|d| (F(4,3): 4 + 5 + 1): below this no transformed value can leave the fp16 range
constexpr int I2V_STATUS_WORDS = 64;   // [0] flag word, [1 .. 31] per-writer maxima of the running forward, [32 + i] the last forward's (snapshot)
constexpr int I2V_STATUS_SNAP = 32;

// The operand of conv `kernel family`: run_modulate the direct kernels' (fp32, or hl16 = the split-fp16 rows of i2v_conv16.hip),
// run_modulate_wino the F(2,3) one, run_modulate_wino4 the F(4,3) one (one: its one-term fp16 form).  x [B][T/ut][H/us][W/us][C] fp32,
// coef = per-(b,c) (A, B) pairs or null, gb = SPADE's maps or null; range_flag = status word [0], umax = the layer's slot.
int run_modulate(const float* x, const float* coef, const float* gb, float* out, int B, int T, int H, int W, int C, int ut,
                 int us, int lrelu, hipStream_t st, bool hl16 = false, int* range_flag = nullptr, int* umax = nullptr, GbRows rows = {});
int run_modulate_wino(const float* x, const float* coef, const float* gb, float* out, int B, int T, int H, int W, int C, int ut,
                      int us, int lrelu, hipStream_t st, int* range_flag, int* umax = nullptr, GbRows rows = {});
int run_modulate_wino4(const float* x, const float* coef, const float* gb, float* out, int B, int T, int H, int W, int C, int ut,
                       int us, int lrelu, hipStream_t st, bool one, int* range_flag, int* umax = nullptr, GbRows rows = {});
// status_finish_kernel at the end of a forward: the writers' maxima become status bit 1 and the snapshot words
int status_finish(int* status, hipStream_t st);

}  // namespace i2v
