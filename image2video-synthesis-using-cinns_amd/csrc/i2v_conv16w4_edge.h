// The temporal edge rule of the Winograd F(4,3) kernels (i2v_conv16w4e.hip): which (kt, MFMA row block) units of a brick read nothing but
// the clip's temporal zero padding.  Plain C++ (no HIP header) so that the host self-test (tests/f43_tskip_host_check.cpp) compiles it
// alone, with any compiler and under the host sanitizers; i2v_conv16w4_dev.h includes it for everything else.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define W4_HD __host__ __device__
#else
#define W4_HD
#endif

namespace i2v {

// Temporal edge units.  Every 3x3x3 conv pads one frame at each end of the clip, and a brick at the clip's edge stages that frame from
// the zero page.  A "unit" is one (kt, MFMA row block of 32 tiles) of a brick: where a row block lies inside ONE frame (TH * 4 >= 32
// tiles per brick row of frames) the unit whose frame reads input frame t0 + m + kt - pt outside [0, T) multiplies zeros only -- all
// three (kt, kh) taps of it, in every chunk.  The rule, once, for the device (conv_wino4e_f16x3_kernel picks its tap loops by it), the
// plan (the issued-MFMA count) and the host self-test (tests/f43_tskip_host_check.cpp: against the `ok` flag of w4_tables, row by row).
// T: frames of the INPUT tensor; (t0, par): the brick (W4Brick); rb: row block over the brick's 128 tiles, tile -> frame =
// tile >> (th_shift + 2); pt as in w4_tables.
W4_HD constexpr bool w4_unit_dead(int T, int th_shift, int KT, int tdup, int t0, int par, int kt, int rb) {
    if ((4 << th_shift) < 32) return false;            // the row block spans two frames or more: nothing is dead
    const int pt = tdup ? 1 - par : KT / 2;
    const int m = (rb * 32) >> (th_shift + 2);         // the one frame of the brick this row block lies in
    const int t = t0 + m + kt - pt;
    return t < 0 || t >= T;
}
// dead mask of the WM row blocks rb0 .. rb0 + WM - 1 (what one wave of a pass holds): bit kt * WM + wm
template <int WM>
W4_HD constexpr unsigned w4_dead_mask(int T, int th_shift, int KT, int tdup, int t0, int par, int rb0) {
    unsigned m = 0;
    for (int kt = 0; kt < KT; ++kt)
        for (int wm = 0; wm < WM; ++wm) m |= (w4_unit_dead(T, th_shift, KT, tdup, t0, par, kt, rb0 + wm) ? 1u : 0u) << (kt * WM + wm);
    return m;
}
// dead units of a whole launch, over its t-bricks and frame parities (x the bricks per frame slab and the channel tiles: the same for
// all), and its units = taps / 3 x 4 row blocks per brick: the share of the tap loops' MFMAs that the edge kernel does not issue
inline void w4_dead_units(int T, int TT, int th_shift, int KT, int tdup, long* dead, long* units) {
    *dead = 0; *units = 0;
    for (int par = 0; par < (tdup ? 2 : 1); ++par)
        for (int t0 = 0; t0 < T; t0 += TT)
            for (int kt = 0; kt < KT; ++kt)
                for (int rb = 0; rb < 4; ++rb) { *dead += w4_unit_dead(T, th_shift, KT, tdup, t0, par, kt, rb); *units += 1; }
}

}  // namespace i2v
