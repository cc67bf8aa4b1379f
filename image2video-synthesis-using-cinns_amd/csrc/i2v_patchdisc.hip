// The spatial (patch) discriminator of stage-1 training: NLayerDiscriminator (stage1_VAE/modules/patch_disc.py:101-165) forward and
// backward, spectral norm in training mode, ActNorm with its data init, and the hinge loss (stage1_VAE/modules/loss.py:24-32).  The
// C ABI is include/i2v_hip_disc.h.  Exact fp32 on v_mfma_f32_16x16x4_f32; every sum has one owner and a fixed order.
//   * Activations are channels-last [N][H][W][C]; the frames are stored with 4 channels (r, g, b, 0) as the VGG and Inception input
//     stages store them.
//   * A forward packs W / sigma of every conv once, on the device, into the two operand layouts: wf [tap][cout][cin] (forward: K over
//     (tap, channel)) and wd [tap][cin][cout] (input gradient: K over (tap, output channel)).  With I2V_PATCHDISC_SAVE they live in
//     `saved` together with that call's u, v and sigma: a backward uses those values of ITS forward.  weight_orig (the projection),
//     loc and scale are read from the bound parameters at backward time: they must not change between a forward and its backward.
//   The kernels of the next three points are the Patch2d family of i2v_train_conv.h, shared with the 3-D ResNet trunk; here are ActNorm,
//   the channel gradients, the cout = 1 head, the hinge, the layout and the C entries.
//   * conv forward: the flat implicit GEMM of i2v_flatconv.h (128 or 64 positions x BN channels per workgroup, chunks of 16 K elements
//     double-buffered in LDS) with the window fixed at 4 x 4 pad 1 and the epilogue bias -> [pre] -> ActNorm -> LeakyReLU.
//   * dgrad: the same GEMM as a gather over input pixels.  At stride 2 a pixel receives the 2 x 2 taps of its parity, so the pixels
//     are processed in four parity classes (blockIdx.y), each with its own taps: K = 4 cout.  The upstream gradient passes through
//     the LeakyReLU mask and ActNorm's scale while it is loaded.
//   * wgrad: per tap a [cout] x [cin] GEMM over the positions, operands straight from global memory.  The position range is cut into
//     slices (wgrad_plan, a pure function of the shape); the four waves of a workgroup take a quarter of a slice each and are
//     summed in LDS in wave order; the slices' partial sums are added in slice order by tc_finish_a, which also forms the blocks
//     of <dWn, W>; tc_finish_dot adds those in block order; tc_finish_b applies the spectral-norm projection and writes or accumulates.
//   * the cout = 1 head is a dot product per position (one wave), with thread-per-element gradient forms.
#include "i2v_handle.h"
#include "i2v_train_conv.h"
#include "../../include/i2v_hip_disc.h"

namespace i2v {
namespace {

static_assert(PD_MAXCONV <= TC_MAXCONV, "one pack launch takes every conv of the network");
struct PdLayer : TcConv { int actnorm, lrelu, key; };   // a conv of the network, its ActNorm and LeakyReLU, its index in `main`

// h = LeakyReLU(scale * (pre + loc)): the forward that initialises ActNorm computes the conv first and applies the norm afterwards
__global__ __launch_bounds__(256) void pd_actnorm_apply_kernel(const float* __restrict__ pre, const float* __restrict__ loc, const float* __restrict__ scale,
                                                               float* __restrict__ out, long total, int C) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % C);
        const float y = scale[c] * (pre[i] + loc[c]);
        out[i] = y > 0.f ? y : 0.2f * y;
    }
}

// per channel over the M rows of x [M][C]: loc = -mean, scale = 1 / (unbiased std + 1e-6); float64, two passes, fixed order
__global__ __launch_bounds__(256) void pd_actnorm_init_kernel(const float* __restrict__ x, long M, int C, float* __restrict__ loc, float* __restrict__ scale) {
    __shared__ double red[256];
    __shared__ double meanv[4];
    const int CG = C >= 4 ? 4 : 1, tid = threadIdx.x;
    const int c = blockIdx.x * CG + tid % CG, rstep = 256 / CG;
    double s = 0.0;
    for (long r = tid / CG; r < M; r += rstep) s += (double)x[r * C + c];
    red[tid] = s;
    __syncthreads();
    if (tid < CG) {
        double t = 0.0;
        for (int j = 0; j < rstep; ++j) t += red[j * CG + tid];
        meanv[tid] = t / (double)M;
    }
    __syncthreads();
    const double mean = meanv[tid % CG];
    double qd = 0.0;
    for (long r = tid / CG; r < M; r += rstep) {
        const double d = (double)x[r * C + c] - mean;
        qd += d * d;
    }
    red[tid] = qd;
    __syncthreads();
    if (tid < CG) {
        double t = 0.0;
        for (int j = 0; j < rstep; ++j) t += red[j * CG + tid];
        loc[c] = (float)(-mean);
        scale[c] = (float)(1.0 / (sqrt(t / (double)(M - 1)) + 1e-6));
    }
}

// per channel over the M rows: dh = g * mask; dbias = scale * sum dh, d_loc = scale * sum dh, d_scale = sum dh * (pre + loc); float64.
// Two stages: a workgroup sums a row slice of 16 channels (C = 1: of the one) into `partial` [R][C][2]; the second adds the slices in order
struct PdChanArgs {
    const float *g, *act, *pre, *loc, *scale;   // act null: no mask; pre / loc / scale null: no ActNorm
    float *dbias, *dloc, *dscale;
    double* partial;
    long M, rows_per;
    int C, R, accumulate;
};

__global__ __launch_bounds__(256) void pd_chan_partial_kernel(PdChanArgs a) {
    __shared__ double red[2][256];
    const int CW = a.C >= 16 ? 16 : 1, tid = threadIdx.x;
    const int c = blockIdx.x * CW + tid % CW, rstep = 256 / CW;
    const long r0 = blockIdx.y * a.rows_per, r1 = r0 + a.rows_per < a.M ? r0 + a.rows_per : a.M;
    const float lc = a.loc ? a.loc[c] : 0.f;
    double s1 = 0.0, s2 = 0.0;
    for (long r = r0 + tid / CW; r < r1; r += rstep) {
        float dh = a.g[r * a.C + c];
        if (a.act) dh *= lrelu_slope(a.act[r * a.C + c]);
        s1 += (double)dh;
        if (a.pre) s2 += (double)dh * (double)(a.pre[r * a.C + c] + lc);
    }
    red[0][tid] = s1; red[1][tid] = s2;
    __syncthreads();
    if (tid >= CW) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < rstep; ++j) { t1 += red[0][j * CW + tid]; t2 += red[1][j * CW + tid]; }
    a.partial[((long)blockIdx.y * a.C + c) * 2] = t1;
    a.partial[((long)blockIdx.y * a.C + c) * 2 + 1] = t2;
}

__global__ __launch_bounds__(256) void pd_chan_final_kernel(PdChanArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    double t1 = 0.0, t2 = 0.0;
    for (int j = 0; j < a.R; ++j) { t1 += a.partial[((long)j * a.C + c) * 2]; t2 += a.partial[((long)j * a.C + c) * 2 + 1]; }
    const double sc = a.scale ? (double)a.scale[c] : 1.0;
    const float db = (float)(sc * t1);
    a.dbias[c] = a.accumulate ? a.dbias[c] + db : db;
    if (a.pre) {
        a.dloc[c] = a.accumulate ? a.dloc[c] + db : db;
        a.dscale[c] = a.accumulate ? a.dscale[c] + (float)t2 : (float)t2;
    }
}

// ------------------------------------------------------------------------------------------------------------------ the cout = 1 head
// one wave per output position: 16 taps x cin products, lanes over channels, fixed shuffle tree
__global__ __launch_bounds__(256) void pd_head_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wf, const float* __restrict__ bias,
                                                          float* __restrict__ out, long M, int Hi, int Wi, int cin) {
    const int lane = threadIdx.x & 63;
    const long m = blockIdx.x * 4L + (threadIdx.x >> 6);
    if (m >= M) return;
    const int Ho = Hi - 1, Wo = Wi - 1;
    const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
    const long n = m / ((long)Wo * Ho);
    float acc = 0.f;
    for (int tap = 0; tap < 16; ++tap) {
        const int h = ho - 1 + (tap >> 2), w = wo - 1 + (tap & 3);
        if ((unsigned)h >= (unsigned)Hi || (unsigned)w >= (unsigned)Wi) continue;
        const float* xs = x + ((n * Hi + h) * Wi + w) * cin;
        const float* ws = wf + (long)tap * cin;
        for (int c = 4 * lane; c < cin; c += 256) {
            const float4 xv = *reinterpret_cast<const float4*>(xs + c), wv = *reinterpret_cast<const float4*>(ws + c);
            acc = fmaf(xv.x, wv.x, acc); acc = fmaf(xv.y, wv.y, acc); acc = fmaf(xv.z, wv.z, acc); acc = fmaf(xv.w, wv.w, acc);
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) out[m] = acc + bias[0];
}

__global__ __launch_bounds__(256) void pd_head_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ wf, float* __restrict__ out, long total,
                                                            int Hi, int Wi, int cin) {
    const int Ho = Hi - 1, Wo = Wi - 1;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % cin);
        long p = i / cin;
        const int w = (int)(p % Wi); p /= Wi;
        const int h = (int)(p % Hi); p /= Hi;
        float acc = 0.f;
        for (int tap = 0; tap < 16; ++tap) {
            const int ho = h + 1 - (tap >> 2), wo = w + 1 - (tap & 3);
            if ((unsigned)ho >= (unsigned)Ho || (unsigned)wo >= (unsigned)Wo) continue;
            acc = fmaf(g[(p * Ho + ho) * Wo + wo], wf[(long)tap * cin + c], acc);
        }
        out[i] = acc;
    }
}

// part [slices][16][cin]: thread = channel, blockIdx.y = tap, blockIdx.z = slice
__global__ __launch_bounds__(256) void pd_head_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ part, long P,
                                                            int Hi, int Wi, int cin, int slice_len) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cin) return;
    const int Ho = Hi - 1, Wo = Wi - 1, tap = blockIdx.y;
    const long begin = (long)blockIdx.z * slice_len, end = begin + slice_len < P ? begin + slice_len : P;
    float acc = 0.f;
    for (long m = begin; m < end; ++m) {
        const int wo = (int)(m % Wo), ho = (int)((m / Wo) % Ho);
        const long n = m / ((long)Wo * Ho);
        const int h = ho - 1 + (tap >> 2), w = wo - 1 + (tap & 3);
        if ((unsigned)h >= (unsigned)Hi || (unsigned)w >= (unsigned)Wi) continue;
        acc = fmaf(g[m], x[((n * Hi + h) * Wi + w) * cin + c], acc);
    }
    part[((long)blockIdx.z * 16 + tap) * cin + c] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ hinge loss
__global__ __launch_bounds__(256) void pd_hinge_kernel(const float* __restrict__ fake, const float* __restrict__ real, long n, int mode, double* __restrict__ out,
                                                       float* __restrict__ d_fake, float* __restrict__ d_real) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double lf = 0.0, lr = 0.0, mf = 0.0, mr = 0.0;
    const float gd = (float)(0.5 / (double)n), gg = (float)(-1.0 / (double)n);
    for (long i = tid; i < n; i += 256) {
        const float f = fake[i];
        mf += (double)f;
        if (mode == I2V_HINGE_GEN) {
            if (d_fake) d_fake[i] = gg;
            continue;
        }
        const float r = real[i];
        mr += (double)r;
        const double hf = 1.0 + (double)f, hr = 1.0 - (double)r;   // exact: the hinge sits where the float64 reference has it
        if (hf > 0.0) lf += hf;
        if (hr > 0.0) lr += hr;
        if (d_fake) d_fake[i] = hf > 0.0 ? gd : 0.f;
        if (d_real) d_real[i] = hr > 0.0 ? -gd : 0.f;
    }
    lf = block_sum(lf, red); lr = block_sum(lr, red); mf = block_sum(mf, red); mr = block_sum(mr, red);
    if (tid == 0) {
        const double dn = (double)n;
        out[0] = mode == I2V_HINGE_GEN ? -mf / dn : (lr / dn + lf / dn) / 2.0;
        out[1] = mr / dn;
        out[2] = mf / dn;
    }
}

// =================================================================================================================== host side

constexpr int PD_CHAN_SLICES = 64;
size_t chan_partial_bytes(int C) { return (size_t)PD_CHAN_SLICES * C * 2 * 8; }

int launch_chan_grads(const float* g, const float* act, const float* pre, const float* loc, const float* scale, float* dbias, float* dloc, float* dscale,
                      double* partial, long M, int C, bool accumulate, hipStream_t st) {
    const int R = (int)std::min<long>(std::max<long>((M + 1023) / 1024, 1), PD_CHAN_SLICES);
    PdChanArgs a{g, act, pre, loc, scale, dbias, dloc, dscale, partial, M, (M + R - 1) / R, C, R, accumulate ? 1 : 0};
    hipLaunchKernelGGL(pd_chan_partial_kernel, dim3(C >= 16 ? C / 16 : C, R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(pd_chan_final_kernel, dim3((C + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

// the head's branch of the weight gradient's slice plan, its partial sums [slices][16][cin] and its launch
void head_wgrad_plan(long P, int* slices, int* slice_len) { cut_slices(P, std::min<long>(std::max<long>((P + 63) / 64, 1), 128), slices, slice_len); }
size_t part_floats(const TcConv& c, long P) {
    if (c.cout > 1) return wgrad_part_floats(c, P);
    int S, L;
    head_wgrad_plan(P, &S, &L);
    return (size_t)S * 16 * c.cin;
}
int launch_head_wgrad(const TcConv& c, const float* g, const float* x, const float* w, const float* u, const float* v, const float* sigma, float* part,
                      float* dwn, double* dotp, float* grad, bool accumulate, const TcGeo& mp, hipStream_t st) {
    int S, L;
    head_wgrad_plan(mp.mo, &S, &L);
    hipLaunchKernelGGL(pd_head_wgrad_kernel, dim3((c.cin + 255) / 256, 16, S), dim3(256), 0, st, g, x, part, mp.mo, mp.hi, mp.wi, c.cin, L);
    I2V_LAUNCHED();
    return launch_finish(part, S, c.cin, 1, c.cin, 16, w, u, v, sigma, dwn, dotp, grad, accumulate, st);
}

// the window of Win2: 4 x 4, pad 1, no time axis (sn: set by the network; a unit entry is told by its u, v, sigma arguments)
PdLayer make_conv(int cin, int cout, int stride, int actnorm, int lrelu, int key) {
    return PdLayer{TcConv{cin, cin == 3 ? 4 : cin, cin == 3 ? 16 : cin, cout, 1, 4, 4, 1, stride, 0}, actnorm, lrelu, key};
}
TcGeo make_map(int n, int hi, int wi, int stride) {
    TcGeo m{};
    m.ti = m.to = 1;
    m.hi = hi; m.wi = wi; m.ho = (hi + 2 - 4) / stride + 1; m.wo = (wi + 2 - 4) / stride + 1;
    if (hi < 2) m.ho = 0;
    if (wi < 2) m.wo = 0;
    m.mi = (long)n * hi * wi; m.mo = (long)n * m.ho * m.wo;
    return m;
}

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_patchdisc {
    int device = 0;
    bool loaded = false;   // parameters bound
    bool have_grads = false;
    int nconv = 0, sn = 1;
    PdLayer L[PD_MAXCONV];
    float *w[PD_MAXCONV] = {}, *b[PD_MAXCONV] = {}, *u[PD_MAXCONV] = {}, *v[PD_MAXCONV] = {}, *loc[PD_MAXCONV] = {}, *scale[PD_MAXCONV] = {};
    float *gw[PD_MAXCONV] = {}, *gb[PD_MAXCONV] = {}, *gloc[PD_MAXCONV] = {}, *gscale[PD_MAXCONV] = {};
};

namespace {

// Where everything lies for one input shape: `saved` (offsets from its base) and the workspace
struct PdLayout {
    bool ok = false;
    TcGeo map[PD_MAXCONV];
    size_t x4 = 0, act[PD_MAXCONV] = {}, pre[PD_MAXCONV] = {}, wf[PD_MAXCONV] = {}, wd[PD_MAXCONV] = {}, sigma[PD_MAXCONV] = {}, us[PD_MAXCONV] = {},
           vs[PD_MAXCONV] = {}, saved_total = 0;
    size_t pi_t[PD_MAXCONV] = {}, pi_s[PD_MAXCONV] = {}, fwd = 0, ga = 0, gb = 0, part = 0, dwn = 0, dotp = 0, chan = 0, ws_total = 0;
};

PdLayout pd_layout(const i2v_patchdisc* d, int n, int h, int w) {
    PdLayout y;
    if (n <= 0 || h <= 0 || w <= 0) return y;
    int hi = h, wi = w;
    for (int i = 0; i < d->nconv; ++i) {
        y.map[i] = make_map(n, hi, wi, d->L[i].ss);
        if (y.map[i].ho < 1 || y.map[i].wo < 1) return y;
        hi = y.map[i].ho; wi = y.map[i].wo;
    }
    Carver s;
    y.x4 = s.take_floats((size_t)y.map[0].mi * 4);
    size_t gmax = 0, pmax = 0, emax = 0, bmax = 0, cmax = 0;
    for (int i = 0; i < d->nconv; ++i) {
        const PdLayer& c = d->L[i];
        if (i + 1 < d->nconv) {
            y.act[i] = s.take_floats((size_t)y.map[i].mo * c.cout);
            y.pre[i] = s.take_floats(c.actnorm ? (size_t)y.map[i].mo * c.cout : 0);
            gmax = std::max(gmax, (size_t)y.map[i].mo * c.cout);
        }
        y.wf[i] = s.take_floats((size_t)16 * c.cout * c.cinp);
        y.wd[i] = s.take_floats(c.cout == 1 ? 0 : pack_elems(c));
        y.sigma[i] = s.take_floats(1);
        y.us[i] = s.take_floats(c.cout);
        y.vs[i] = s.take_floats((size_t)c.cin * 16);
        pmax = std::max(pmax, part_floats(c, y.map[i].mo));
        emax = std::max(emax, (size_t)c.cout * c.cin * 16);
        bmax = std::max(bmax, finish_blocks(c));
        cmax = std::max(cmax, chan_partial_bytes(c.cout));
    }
    y.saved_total = s.total();
    Carver k;
    for (int i = 0; i < d->nconv; ++i) {
        y.pi_t[i] = k.take_bytes((size_t)d->L[i].cin * 16 * 8);
        y.pi_s[i] = k.take_bytes((size_t)d->L[i].cout * 8);
    }
    y.fwd = k.take_bytes(y.saved_total);
    y.ga = k.take_floats(gmax);
    y.gb = k.take_floats(gmax);
    y.part = k.take_floats(pmax);
    y.dwn = k.take_floats(emax);
    y.dotp = k.take_bytes(bmax * 8);
    y.chan = k.take_bytes(cmax);
    y.ws_total = k.total();
    y.ok = true;
    return y;
}

int check_unit(const char* what, int n, int hi, int wi, int cin, int cout, int stride) {
    I2V_REQUIRE(n > 0 && hi >= 2 && wi >= 2 && (stride == 1 || stride == 2), I2V_E_INVALID, "%s: n %d, map %d x %d, stride %d", what, n, hi, wi, stride);
    I2V_REQUIRE((cin == 3 || (cin > 0 && cin % 16 == 0)) && cout > 0 && cout % 16 == 0, I2V_E_INVALID,
                "%s: cin %d (3 or a multiple of 16), cout %d (a multiple of 16)", what, cin, cout);
    const TcGeo m = make_map(n, hi, wi, stride);
    I2V_REQUIRE(m.ho >= 1 && m.wo >= 1, I2V_E_INVALID, "%s: a %d x %d map leaves no output", what, hi, wi);
    return I2V_OK;
}

// workspace of the unit entries: wf, wd, part, dwn, dotp, the power iteration's t and s
struct PdUnitWs { size_t wf, wd, part, dwn, dotp, chan, t, s, sig, total; };
PdUnitWs unit_ws(int n, int hi, int wi, int cin, int cout) {
    const PdLayer c = make_conv(cin, cout, 1, 0, 0, 0);
    const TcGeo m = make_map(n, hi, wi, 1);   // stride 1 has the most positions
    Carver k;
    PdUnitWs y{};
    y.wf = k.take_floats((size_t)16 * cout * c.cinp);
    y.wd = k.take_floats(pack_elems(c));
    y.part = k.take_floats(part_floats(c, std::max<long>(m.mo, 1)) + part_floats(make_conv(cin, cout, 2, 0, 0, 0), std::max<long>(m.mo, 1)));
    y.dwn = k.take_floats((size_t)cout * cin * 16);
    y.dotp = k.take_bytes(finish_blocks(c) * 8);
    y.chan = k.take_bytes(chan_partial_bytes(cout));
    y.t = k.take_bytes((size_t)cin * 16 * 8);
    y.s = k.take_bytes((size_t)cout * 8);
    y.sig = k.take_floats(1);
    y.total = k.total();
    return y;
}

// workspace of the head unit, from the cout = 1 conv's own plan
PdUnitWs head_ws(int n, int hi, int wi, int cin) {
    const PdLayer c = make_conv(cin, 1, 1, 0, 0, 0);
    Carver k;
    PdUnitWs y{};
    y.wf = k.take_floats((size_t)16 * cin);
    y.part = k.take_floats(part_floats(c, std::max<long>(make_map(n, hi, wi, 1).mo, 1)));
    y.dwn = k.take_floats((size_t)cin * 16);
    y.dotp = k.take_bytes(finish_blocks(c) * 8);
    y.chan = k.take_bytes(chan_partial_bytes(1));
    y.total = k.total();
    return y;
}

int pack_unit(const PdLayer& c, const float* weight, float* wf, float* wd, hipStream_t st) {
    TcPackArgs p{};
    p.nconv = 1; p.total = (long)pack_elems(c);
    p.c[0] = TcPackConv{weight, nullptr, wf, wd, c.cout, c.cin, c.cinp, c.cind, 16, 0};
    return launch_pack<Patch2d>(p, st);
}

}  // namespace

extern "C" {

int i2v_patchdisc_create(const i2v_patchdisc_cfg* cfg, i2v_patchdisc** out) {
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "i2v_patchdisc_create: null argument");
    I2V_REQUIRE(cfg->use_actnorm, I2V_E_INVALID, "i2v_patchdisc_create: use_actnorm = 0 (BatchNorm2d) is not built");
    I2V_REQUIRE(cfg->in_channels == 3, I2V_E_INVALID, "i2v_patchdisc_create: in_channels %d (only 3 is built)", cfg->in_channels);
    I2V_REQUIRE(cfg->ndf > 0 && cfg->ndf % 16 == 0, I2V_E_INVALID, "i2v_patchdisc_create: ndf %d is not a multiple of 16", cfg->ndf);
    I2V_REQUIRE(cfg->n_layers >= 1 && cfg->n_layers <= PD_MAXCONV - 2, I2V_E_INVALID, "i2v_patchdisc_create: n_layers %d outside 1..%d", cfg->n_layers,
                PD_MAXCONV - 2);
    const i2v_patchdisc_cfg c = *cfg;
    return create_handle("i2v_patchdisc_create", out, [c](i2v_patchdisc* d) {
        d->sn = c.spectral_norm ? 1 : 0;
        int k = 0, mult = 1;
        d->L[k++] = make_conv(3, c.ndf, 2, 0, 1, 0);
        for (int n = 1; n <= c.n_layers; ++n) {
            const int prev = mult;
            mult = std::min(1 << n, 8);
            d->L[k++] = make_conv(c.ndf * prev, c.ndf * mult, n < c.n_layers ? 2 : 1, 1, 1, 2 + 3 * (n - 1));
        }
        d->L[k++] = make_conv(c.ndf * mult, 1, 1, 0, 0, 2 + 3 * c.n_layers);
        d->nconv = k;
        for (int i = 0; i < k; ++i) d->L[i].sn = d->sn;
        return I2V_OK;
    });
}

void i2v_patchdisc_destroy(i2v_patchdisc* d) { delete d; }

// the device pointer under `key`, or null with the error set
static bool bound_ptr(const StateDict& s, const std::string& key, int64_t numel, float** out) {
    const float* p = s.f32(key, numel);
    *out = const_cast<float*>(p);
    return p != nullptr;
}

int i2v_patchdisc_bind(i2v_patchdisc* d, const i2v_tensor* params, int32_t n) {
    I2V_REQUIRE(d && params && n > 0, I2V_E_INVALID, "i2v_patchdisc_bind: null argument");
    d->loaded = false;
    const StateDict sd(params, n);
    for (int i = 0; i < d->nconv; ++i) {
        const PdLayer& c = d->L[i];
        const std::string m = "main." + std::to_string(c.key);
        if (!bound_ptr(sd, m + (d->sn ? ".weight_orig" : ".weight"), (int64_t)c.cout * c.cin * 16, &d->w[i]) || !bound_ptr(sd, m + ".bias", c.cout, &d->b[i]))
            return I2V_E_MISSING;
        if (d->sn && (!bound_ptr(sd, m + ".weight_u", c.cout, &d->u[i]) || !bound_ptr(sd, m + ".weight_v", (int64_t)c.cin * 16, &d->v[i]))) return I2V_E_MISSING;
        if (c.actnorm) {
            const std::string a = "main." + std::to_string(c.key + 1);
            if (!bound_ptr(sd, a + ".loc", c.cout, &d->loc[i]) || !bound_ptr(sd, a + ".scale", c.cout, &d->scale[i])) return I2V_E_MISSING;
        }
    }
    d->loaded = true;
    return I2V_OK;
}

int i2v_patchdisc_bind_grads(i2v_patchdisc* d, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(d && (grads ? n > 0 : n == 0), I2V_E_INVALID, "i2v_patchdisc_bind_grads: null handle, or a count without tensors");
    d->have_grads = false;
    if (!grads) return I2V_OK;
    const StateDict gd(grads, n);
    for (int i = 0; i < d->nconv; ++i) {
        const PdLayer& c = d->L[i];
        const std::string m = "main." + std::to_string(c.key);
        if (!bound_ptr(gd, m + (d->sn ? ".weight_orig" : ".weight"), (int64_t)c.cout * c.cin * 16, &d->gw[i]) || !bound_ptr(gd, m + ".bias", c.cout, &d->gb[i]))
            return I2V_E_MISSING;
        if (c.actnorm) {
            const std::string a = "main." + std::to_string(c.key + 1);
            if (!bound_ptr(gd, a + ".loc", c.cout, &d->gloc[i]) || !bound_ptr(gd, a + ".scale", c.cout, &d->gscale[i])) return I2V_E_MISSING;
        }
    }
    d->have_grads = true;
    return I2V_OK;
}

int i2v_patchdisc_out_shape(const i2v_patchdisc* d, int32_t h, int32_t w, int32_t* ho, int32_t* wo) {
    I2V_REQUIRE(d && ho && wo, I2V_E_INVALID, "i2v_patchdisc_out_shape: null argument");
    const PdLayout y = pd_layout(d, 1, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "i2v_patchdisc_out_shape: a %d x %d input shrinks below a 1 x 1 output", h, w);
    *ho = y.map[d->nconv - 1].ho; *wo = y.map[d->nconv - 1].wo;
    return I2V_OK;
}

size_t i2v_patchdisc_saved_bytes(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w) { return d ? pd_layout(d, n, h, w).saved_total : 0; }
size_t i2v_patchdisc_workspace_bytes(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w) { return d ? pd_layout(d, n, h, w).ws_total : 0; }

int i2v_patchdisc_saved_layout(const i2v_patchdisc* d, int32_t n, int32_t h, int32_t w, int32_t* nconv, int32_t* ho, int32_t* wo, int32_t* cout,
                               int64_t* act_offset, int64_t* pre_offset) {
    I2V_REQUIRE(d && nconv && ho && wo && cout && act_offset && pre_offset, I2V_E_INVALID, "i2v_patchdisc_saved_layout: null argument");
    const PdLayout y = pd_layout(d, n, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "i2v_patchdisc_saved_layout: a %d x %d input (batch %d) shrinks below a 1 x 1 output", h, w, n);
    *nconv = d->nconv;
    for (int i = 0; i < d->nconv; ++i) {
        ho[i] = y.map[i].ho; wo[i] = y.map[i].wo; cout[i] = d->L[i].cout;
        act_offset[i] = i + 1 < d->nconv ? (int64_t)y.act[i] : -1;
        pre_offset[i] = i + 1 < d->nconv && d->L[i].actnorm ? (int64_t)y.pre[i] : -1;
    }
    return I2V_OK;
}

int i2v_patchdisc_forward(i2v_patchdisc* d, const float* x, int32_t n, int32_t h, int32_t w, int32_t flags, float* pred, void* saved, size_t saved_bytes,
                          void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_forward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(x && pred && workspace, I2V_E_INVALID, "%s: null argument", what);
    const PdLayout y = pd_layout(d, n, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: a %d x %d input (batch %d) shrinks below a 1 x 1 output", what, h, w, n);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    const bool save = flags & I2V_PATCHDISC_SAVE, init = flags & I2V_PATCHDISC_INIT_ACTNORM;
    if (save) {
        I2V_REQUIRE(saved, I2V_E_INVALID, "%s: I2V_PATCHDISC_SAVE without a saved buffer", what);
        I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = save ? saved : Carver::at<char>(workspace, y.fwd);
    const int nc = d->nconv;

    float* x4 = Carver::at(sv, y.x4);
    hipLaunchKernelGGL(tc_input4_kernel, dim3(grid_for(y.map[0].mi)), dim3(256), 0, st, x, x4, y.map[0].mi, (long)h * w);
    I2V_LAUNCHED();

    TcPackArgs pk{};
    pk.nconv = nc;
    if (d->sn) {
        PdPiArgs pi{};
        pi.nconv = nc; pi.iterate = flags & I2V_PATCHDISC_ITERATE ? 1 : 0;
        for (int i = 0; i < nc; ++i) {
            const PdLayer& c = d->L[i];
            pi.c[i] = PdPiConv{d->w[i], d->u[i], d->v[i], Carver::at(sv, y.sigma[i]), Carver::at(sv, y.us[i]), Carver::at(sv, y.vs[i]),
                               Carver::at<double>(workspace, y.pi_t[i]), Carver::at<double>(workspace, y.pi_s[i]), c.cout, c.cin * 16, pi.btotal, pi.rtotal};
            pi.btotal += (c.cin * 16 + 63) / 64; pi.rtotal += c.cout;
        }
        if (int rc = launch_power_iteration(pi, st)) return rc;
    }
    for (int i = 0; i < nc; ++i) {
        const PdLayer& c = d->L[i];
        pk.c[i] = TcPackConv{d->w[i], d->sn ? Carver::at(sv, y.sigma[i]) : nullptr, Carver::at(sv, y.wf[i]), c.cout == 1 ? nullptr : Carver::at(sv, y.wd[i]),
                             c.cout, c.cin, c.cinp, c.cind, 16, pk.total};
        pk.total += (long)pack_elems(c);
    }
    if (int rc = launch_pack<Patch2d>(pk, st)) return rc;

    const float* in = x4;
    for (int i = 0; i + 1 < nc; ++i) {
        const PdLayer& c = d->L[i];
        float* act = Carver::at(sv, y.act[i]);
        float* pre = c.actnorm && (save || init) ? Carver::at(sv, y.pre[i]) : nullptr;
        if (c.actnorm && init) {
            if (int rc = launch_conv<Patch2d>(c, in, Carver::at(sv, y.wf[i]), nullptr, y.map[i], st, {d->b[i], nullptr, nullptr, pre, false})) return rc;
            hipLaunchKernelGGL(pd_actnorm_init_kernel, dim3(c.cout / 4), dim3(256), 0, st, pre, y.map[i].mo, c.cout, d->loc[i], d->scale[i]);
            I2V_LAUNCHED();
            const long total = y.map[i].mo * c.cout;
            hipLaunchKernelGGL(pd_actnorm_apply_kernel, dim3(grid_for(total)), dim3(256), 0, st, pre, d->loc[i], d->scale[i], act, total, c.cout);
            I2V_LAUNCHED();
        } else if (int rc = launch_conv<Patch2d>(c, in, Carver::at(sv, y.wf[i]), act, y.map[i], st,
                                                 {d->b[i], c.actnorm ? d->loc[i] : nullptr, c.actnorm ? d->scale[i] : nullptr, pre, c.lrelu != 0})) {
            return rc;
        }
        in = act;
    }
    const TcGeo& hm = y.map[nc - 1];
    hipLaunchKernelGGL(pd_head_fwd_kernel, dim3((unsigned)((hm.mo + 3) / 4)), dim3(256), 0, st, in, Carver::at(sv, y.wf[nc - 1]), d->b[nc - 1], pred, hm.mo,
                       hm.hi, hm.wi, d->L[nc - 1].cin);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_patchdisc_backward(i2v_patchdisc* d, const float* d_pred, const void* saved, size_t saved_bytes, int32_t n, int32_t h, int32_t w, float* d_x,
                           int32_t param_grads, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_backward";
    I2V_ENTER(sc, d, Entry::NEEDS_WEIGHTS, what);
    I2V_REQUIRE(d_pred && saved && workspace, I2V_E_INVALID, "%s: null argument", what);
    I2V_REQUIRE(d_x || param_grads, I2V_E_INVALID, "%s: neither the input gradient nor the parameter gradients are asked for", what);
    I2V_REQUIRE(!param_grads || d->have_grads, I2V_E_STATE, "%s: no gradient tensors are bound", what);
    const PdLayout y = pd_layout(d, n, h, w);
    I2V_REQUIRE(y.ok, I2V_E_INVALID, "%s: a %d x %d input (batch %d) shrinks below a 1 x 1 output", what, h, w, n);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, y.ws_total, what);
    I2V_REQUIRE_WORKSPACE(saved_bytes, y.saved_total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* sv = const_cast<void*>(saved);
    const int nc = d->nconv;
    const bool acc = accumulate != 0;
    float* part = Carver::at(workspace, y.part);
    float* dwn = Carver::at(workspace, y.dwn);
    double* dotp = Carver::at<double>(workspace, y.dotp);
    double* chan = Carver::at<double>(workspace, y.chan);
    float* ga = Carver::at(workspace, y.ga);
    float* gb = Carver::at(workspace, y.gb);
    auto snap = [&](int i, const float** u, const float** v, const float** sg) {
        *u = d->sn ? Carver::at(sv, y.us[i]) : nullptr; *v = d->sn ? Carver::at(sv, y.vs[i]) : nullptr; *sg = d->sn ? Carver::at(sv, y.sigma[i]) : nullptr;
    };
    const float *us, *vs, *sg;

    // the head
    {
        const int i = nc - 1;
        const PdLayer& c = d->L[i];
        const float* xin = Carver::at(sv, y.act[i - 1]);
        if (param_grads) {
            if (int rc = launch_chan_grads(d_pred, nullptr, nullptr, nullptr, nullptr, d->gb[i], nullptr, nullptr, chan, y.map[i].mo, 1, acc, st)) return rc;
            snap(i, &us, &vs, &sg);
            if (int rc = launch_head_wgrad(c, d_pred, xin, d->w[i], us, vs, sg, part, dwn, dotp, d->gw[i], acc, y.map[i], st)) return rc;
        }
        const long total = y.map[i].mi * c.cin;
        hipLaunchKernelGGL(pd_head_dgrad_kernel, dim3(grid_for(total)), dim3(256), 0, st, d_pred, Carver::at(sv, y.wf[i]), ga, total, y.map[i].hi, y.map[i].wi,
                           c.cin);
        I2V_LAUNCHED();
    }
    for (int i = nc - 2; i >= 0; --i) {
        const PdLayer& c = d->L[i];
        const float* act = Carver::at(sv, y.act[i]);
        const float* scale = c.actnorm ? d->scale[i] : nullptr;
        const float* xin = i == 0 ? Carver::at(sv, y.x4) : Carver::at(sv, y.act[i - 1]);
        if (param_grads) {
            if (int rc = launch_chan_grads(ga, act, c.actnorm ? Carver::at(sv, y.pre[i]) : nullptr, c.actnorm ? d->loc[i] : nullptr, scale, d->gb[i],
                                           d->gloc[i], d->gscale[i], chan, y.map[i].mo, c.cout, acc, st))
                return rc;
            snap(i, &us, &vs, &sg);
            if (int rc = launch_wgrad<Patch2d>(c, ga, act, scale, xin, d->w[i], us, vs, sg, part, dwn, dotp, d->gw[i], acc, y.map[i], st)) return rc;
        }
        if (i == 0 && !d_x) break;
        if (int rc = launch_dgrad<Patch2d>(c, ga, act, scale, Carver::at(sv, y.wd[i]), nullptr, nullptr, i == 0 ? d_x : gb, i == 0, n, y.map[i], st))
            return rc;
        std::swap(ga, gb);
    }
    return I2V_OK;
}

int i2v_patchdisc_hinge(const float* fake, const float* real, int64_t numel, int32_t mode, double* out, float* d_fake, float* d_real, void* stream) {
    I2V_REQUIRE(fake && out && numel > 0 && (mode == I2V_HINGE_GEN || (mode == I2V_HINGE_DISC && real)), I2V_E_INVALID,
                "i2v_patchdisc_hinge: null argument, numel %lld or mode %d", (long long)numel, mode);
    hipLaunchKernelGGL(pd_hinge_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), fake, real, (long)numel, mode, out, d_fake, d_real);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_patchdisc_wgrad_plan(int32_t cout, int32_t cin, int64_t positions, int32_t* slices, int32_t* slice_len) {
    I2V_REQUIRE(slices && slice_len && positions > 0 && (cout == 1 || (cout > 0 && cout % 16 == 0)) && (cin == 3 || (cin > 0 && cin % 16 == 0)), I2V_E_INVALID,
                "i2v_patchdisc_wgrad_plan: cout %d, cin %d, %lld positions", cout, cin, (long long)positions);
    if (cout == 1) head_wgrad_plan(positions, slices, slice_len);
    else wgrad_plan(cout, cin, 16, positions, slices, slice_len);
    return I2V_OK;
}

size_t i2v_patchdisc_unit_workspace_bytes(int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout) {
    if (n <= 0 || hi < 2 || wi < 2 || cin <= 0 || cout <= 0) return 0;
    return cout == 1 ? head_ws(n, hi, wi, cin).total : unit_ws(n, hi, wi, cin, cout).total;
}

int i2v_patchdisc_conv_unit(const float* x, const float* weight, const float* bias, const float* loc, const float* scale, int32_t n, int32_t hi, int32_t wi,
                            int32_t cin, int32_t cout, int32_t stride, int32_t lrelu, float* out, float* pre, void* workspace, size_t workspace_bytes,
                            void* stream) {
    const char* what = "i2v_patchdisc_conv_unit";
    if (int rc = check_unit(what, n, hi, wi, cin, cout, stride)) return rc;
    I2V_REQUIRE(x && weight && bias && (out || pre) && workspace && !loc == !scale, I2V_E_INVALID, "%s: null argument", what);
    const PdUnitWs k = unit_ws(n, hi, wi, cin, cout);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdLayer c = make_conv(cin, cout, stride, loc != nullptr, lrelu, 0);
    if (int rc = pack_unit(c, weight, Carver::at(workspace, k.wf), nullptr, st)) return rc;
    return launch_conv<Patch2d>(c, x, Carver::at(workspace, k.wf), out, make_map(n, hi, wi, stride), st, {bias, loc, scale, pre, lrelu != 0});
}

int i2v_patchdisc_dgrad_unit(const float* g, const float* weight, const float* act, const float* scale, int32_t n, int32_t hi, int32_t wi, int32_t cin,
                             int32_t cout, int32_t stride, float* out, int32_t frames_out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_dgrad_unit";
    if (int rc = check_unit(what, n, hi, wi, cin, cout, stride)) return rc;
    I2V_REQUIRE(g && weight && out && workspace && (!frames_out || cin == 3), I2V_E_INVALID, "%s: null argument, or frames_out with cin %d", what, cin);
    const PdUnitWs k = unit_ws(n, hi, wi, cin, cout);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdLayer c = make_conv(cin, cout, stride, 0, 0, 0);
    if (int rc = pack_unit(c, weight, Carver::at(workspace, k.wf), Carver::at(workspace, k.wd), st)) return rc;
    return launch_dgrad<Patch2d>(c, g, act, scale, Carver::at(workspace, k.wd), nullptr, nullptr, out, frames_out != 0, n, make_map(n, hi, wi, stride), st);
}

int i2v_patchdisc_wgrad_unit(const float* g, const float* act, const float* scale, const float* x, const float* weight, const float* u, const float* v,
                             const float* sigma, int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t stride, int32_t accumulate,
                             float* dweight, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_wgrad_unit";
    if (int rc = check_unit(what, n, hi, wi, cin, cout, stride)) return rc;
    I2V_REQUIRE(g && x && weight && dweight && dbias && workspace && !u == !v && !u == !sigma, I2V_E_INVALID, "%s: null argument", what);
    const PdUnitWs k = unit_ws(n, hi, wi, cin, cout);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdLayer c = make_conv(cin, cout, stride, 0, 0, 0);
    const TcGeo mp = make_map(n, hi, wi, stride);
    if (int rc = launch_chan_grads(g, act, nullptr, nullptr, scale, dbias, nullptr, nullptr, Carver::at<double>(workspace, k.chan), mp.mo, cout, accumulate != 0, st)) return rc;
    return launch_wgrad<Patch2d>(c, g, act, scale, x, weight, u, v, sigma, Carver::at(workspace, k.part), Carver::at(workspace, k.dwn),
                                 Carver::at<double>(workspace, k.dotp), dweight, accumulate != 0, mp, st);
}

int i2v_patchdisc_head_unit(const float* x, const float* weight, const float* bias, const float* g, int32_t n, int32_t hi, int32_t wi, int32_t cin,
                            float* out, float* dx, float* dweight, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_head_unit";
    I2V_REQUIRE(n > 0 && hi >= 2 && wi >= 2 && cin > 0 && cin % 16 == 0, I2V_E_INVALID, "%s: n %d, map %d x %d, cin %d", what, n, hi, wi, cin);
    I2V_REQUIRE(x && weight && bias && out && workspace && (!g || (dx && dweight && dbias)), I2V_E_INVALID, "%s: null argument", what);
    const PdUnitWs k = head_ws(n, hi, wi, cin);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total, what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PdLayer c = make_conv(cin, 1, 1, 0, 0, 0);
    const TcGeo mp = make_map(n, hi, wi, 1);
    float* wf = Carver::at(workspace, k.wf);
    if (int rc = pack_unit(c, weight, wf, nullptr, st)) return rc;
    hipLaunchKernelGGL(pd_head_fwd_kernel, dim3((unsigned)((mp.mo + 3) / 4)), dim3(256), 0, st, x, wf, bias, out, mp.mo, hi, wi, cin);
    I2V_LAUNCHED();
    if (!g) return I2V_OK;
    if (int rc = launch_chan_grads(g, nullptr, nullptr, nullptr, nullptr, dbias, nullptr, nullptr, Carver::at<double>(workspace, k.chan), mp.mo, 1, false, st)) return rc;
    if (int rc = launch_head_wgrad(c, g, x, weight, nullptr, nullptr, nullptr, Carver::at(workspace, k.part), Carver::at(workspace, k.dwn),
                                   Carver::at<double>(workspace, k.dotp), dweight, false, mp, st))
        return rc;
    const long total = mp.mi * cin;
    hipLaunchKernelGGL(pd_head_dgrad_kernel, dim3(grid_for(total)), dim3(256), 0, st, g, wf, dx, total, hi, wi, cin);
    I2V_LAUNCHED();
    return I2V_OK;
}

int i2v_patchdisc_power_iteration_unit(const float* weight, float* u, float* v, int32_t rows, int32_t cols, int32_t iterate, float* sigma, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    const char* what = "i2v_patchdisc_power_iteration_unit";
    I2V_REQUIRE(weight && u && v && sigma && workspace && rows > 0 && cols > 0, I2V_E_INVALID, "%s: null argument or %d x %d", what, rows, cols);
    Carver k;
    const size_t ot = k.take_bytes((size_t)cols * 8), os = k.take_bytes((size_t)rows * 8);
    I2V_REQUIRE_WORKSPACE(workspace_bytes, k.total(), what);
    PdPiArgs pi{};
    pi.nconv = 1; pi.iterate = iterate ? 1 : 0; pi.btotal = (cols + 63) / 64; pi.rtotal = rows;
    pi.c[0] = PdPiConv{weight, u, v, sigma, nullptr, nullptr, Carver::at<double>(workspace, ot), Carver::at<double>(workspace, os), rows, cols, 0, 0};
    return launch_power_iteration(pi, static_cast<hipStream_t>(stream));
}

int i2v_patchdisc_actnorm_init_unit(const float* pre, int64_t m, int32_t c, float* loc, float* scale, void* stream) {
    I2V_REQUIRE(pre && loc && scale && m > 1 && c > 0 && c % 4 == 0, I2V_E_INVALID, "i2v_patchdisc_actnorm_init_unit: null argument, %lld rows or %d channels",
                (long long)m, c);
    hipLaunchKernelGGL(pd_actnorm_init_kernel, dim3(c / 4), dim3(256), 0, static_cast<hipStream_t>(stream), pre, (long)m, c, loc, scale);
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // extern "C"
