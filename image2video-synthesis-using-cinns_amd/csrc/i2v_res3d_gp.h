// The gradient of the gradient penalty on the 3-D ResNet training trunk, without a general double backward.  With P = mean_b pred_b,
// g = grad_x P and L_GP = (1 / n) sum_b |g_b|^2, the gradient of L_GP at the parameters is that of the directional derivative of P along
// v = (2 / n) g (held constant): one TANGENT forward (x-dot = v through the network, on the primal's masks, argmaxes and statistics) and
// one ordinary reverse pass over the pair (primal, tangent), seeded at the tangent of P alone.  The convs are linear, so the tangent
// forward, the two input gradients and the two weight gradients of a conv are the existing Trunk3d launchers; ReLU, the pool and the
// residual add take the primal's decisions for both members.  What is new lies here: GroupNorm's tangent and its dual backward, the
// pool's tangent gather, the head's dual, and the two walks.  Per (sample, group) of m elements, with xh = (x - mu) r, M(a) = mean(a),
// C(a) = mean(xh a), Pi(a) = a - M(a) - xh C(a), p = w yb', q = w yb (yb, yb': the adjoints of the primal and of the tangent output):
//   tangent   xh' = r Pi(x'), y' = w xh'
//   xb'       = r Pi(p)
//   xb        = r Pi(q) - r^2 [xh mean(p Pi(x')) + C(x') Pi(p) + C(p) Pi(x')]
//   wb        = sum yb xh + sum yb' xh',   bb = sum yb
// Sums are float64 over position slices in slice order, every element is rounded once: two runs give the same bits.
// Included into the anonymous namespace of its user behind i2v_res3d_net.h; the motion encoder's path does not include it.
#pragma once
#include "i2v_res3d_net.h"

namespace i2v {
namespace {

struct D3GpGnArgs {
    const float *x, *xd;          // the primal and the tangent input of the norm [N][P][C]
    const float *resd, *mask;     // tangent forward: the residual's tangent or null; the ReLU mask (the primal's activated output) or null
    const float *g, *gd;          // backward: the adjoints at the primal and at the tangent output, both counted where mask > 0
    const float* weight;
    float *out, *outd;            // tangent forward: out; backward: the adjoints at x (out) and at xd (outd)
    float *dweight, *dbias;
    const double* stats;          // [N][16][2]: mean, rstd of the primal
    double* tstats;               // [N][16][2]: M(xd), C(xd)
    double *partial, *ab, *gs;    // slices' sums; [N][C][5] per-channel sums; [N][16][5] per-group sums
    long P, rows_per;
    int N, C, cpg, R, accumulate;
};

// sum of xd and of xh xd of one (sample, group) over a slice of the positions
__global__ __launch_bounds__(256) void d3g_gn_tan_stats_kernel(D3GpGnArgs a) {
    __shared__ double red[256];
    const int grp = blockIdx.x, n = blockIdx.y, r = blockIdx.z;
    const long p0 = r * a.rows_per, p1 = p0 + a.rows_per < a.P ? p0 + a.rows_per : a.P;
    const long cnt = p1 > p0 ? (p1 - p0) * a.cpg : 0;
    const long base = (long)n * a.P * a.C + grp * a.cpg;
    const double* st = a.stats + ((long)n * D3_GROUPS + grp) * 2;
    const double mean = st[0], rstd = st[1];
    double s = 0.0, q = 0.0;
    for (long i = threadIdx.x; i < cnt; i += 256) {
        const long o = base + (p0 + i / a.cpg) * a.C + (int)(i % a.cpg);
        const double v = (double)a.xd[o];
        s += v; q += v * (((double)a.x[o] - mean) * rstd);
    }
    s = block_sum(s, red);
    q = block_sum(q, red);
    if (threadIdx.x == 0) {
        double* dst = a.partial + (((long)n * D3_GROUPS + grp) * a.R + r) * 2;
        dst[0] = s; dst[1] = q;
    }
}

__global__ __launch_bounds__(256) void d3g_gn_tan_final_kernel(D3GpGnArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * D3_GROUPS) return;
    double s = 0.0, q = 0.0;
    for (int r = 0; r < a.R; ++r) { s += a.partial[((long)i * a.R + r) * 2]; q += a.partial[((long)i * a.R + r) * 2 + 1]; }
    const double m = (double)a.P * a.cpg;
    a.tstats[2 * i] = s / m;
    a.tstats[2 * i + 1] = q / m;
}

// y' = w r Pi(x') (+ res') (where mask > 0)
__global__ __launch_bounds__(256) void d3g_gn_tan_apply_kernel(D3GpGnArgs a) {
    const long total = (long)a.N * a.P * a.C, pc = a.P * a.C;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int n = (int)(i / pc), c = (int)(i % a.C), grp = c / a.cpg;
        const double* st = a.stats + ((long)n * D3_GROUPS + grp) * 2;
        const double* ts = a.tstats + ((long)n * D3_GROUPS + grp) * 2;
        const double xhat = ((double)a.x[i] - st[0]) * st[1];
        float y = (float)(st[1] * ((double)a.xd[i] - ts[0] - xhat * ts[1])) * a.weight[c];
        if (a.resd) y += a.resd[i];
        if (a.mask) y = a.mask[i] > 0.f ? y : 0.f;
        a.out[i] = y;
    }
}

// per (sample, channel) over a slice of the positions: sums of yb, yb xh, yb', yb' xh, yb' x'; 16 channels x 16 rows per workgroup
__global__ __launch_bounds__(256) void d3g_gn_dual_partial_kernel(D3GpGnArgs a) {
    __shared__ double red[5][256];
    const int tid = threadIdx.x, c = blockIdx.x * 16 + (tid & 15), n = blockIdx.y, r = blockIdx.z;
    const long p0 = r * a.rows_per, p1 = p0 + a.rows_per < a.P ? p0 + a.rows_per : a.P;
    const double* st = a.stats + ((long)n * D3_GROUPS + c / a.cpg) * 2;
    const double mean = st[0], rstd = st[1];
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (long p = p0 + (tid >> 4); p < p1; p += 16) {
        const long o = ((long)n * a.P + p) * a.C + c;
        float dy = a.g[o], dyd = a.gd[o];
        if (a.mask) {
            const bool on = a.mask[o] > 0.f;
            dy = on ? dy : 0.f; dyd = on ? dyd : 0.f;
        }
        const double xhat = ((double)a.x[o] - mean) * rstd;
        s[0] += (double)dy;
        s[1] += (double)dy * xhat;
        s[2] += (double)dyd;
        s[3] += (double)dyd * xhat;
        s[4] += (double)dyd * (double)a.xd[o];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][tid] = s[k];
    __syncthreads();
    if (tid >= 16) return;
    double* dst = a.partial + (((long)n * a.R + r) * a.C + c) * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        double t = 0.0;
        for (int j = 0; j < 16; ++j) t += red[k][j * 16 + tid];
        dst[k] = t;
    }
}

// one workgroup per sample: the slices in slice order -> ab [n][c][5]; then per group the sums of weight * ab -> gs [n][group][5]
__global__ __launch_bounds__(256) void d3g_gn_dual_reduce_kernel(D3GpGnArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < a.C; c += 256) {
        double t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int r = 0; r < a.R; ++r) {
            const double* src = a.partial + (((long)n * a.R + r) * a.C + c) * 5;
#pragma unroll
            for (int k = 0; k < 5; ++k) t[k] += src[k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) a.ab[((long)n * a.C + c) * 5 + k] = t[k];
    }
    __syncthreads();
    if (tid < D3_GROUPS) {
        double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < a.cpg; ++j) {
            const int c = tid * a.cpg + j;
            const double w = (double)a.weight[c];
#pragma unroll
            for (int k = 0; k < 5; ++k) s[k] += w * a.ab[((long)n * a.C + c) * 5 + k];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) a.gs[((long)n * D3_GROUPS + tid) * 5 + k] = s[k];
    }
}

// bb = sum yb; wb = sum yb xh + sum_n r (sum yb' x' - M(x') sum yb' - C(x') sum yb' xh), the samples in order
__global__ __launch_bounds__(256) void d3g_gn_dual_param_kernel(D3GpGnArgs a) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= a.C) return;
    const int grp = c / a.cpg;
    double t1 = 0.0, t2 = 0.0;
    for (int n = 0; n < a.N; ++n) {
        const double* ab = a.ab + ((long)n * a.C + c) * 5;
        const double* ts = a.tstats + ((long)n * D3_GROUPS + grp) * 2;
        const double rstd = a.stats[((long)n * D3_GROUPS + grp) * 2 + 1];
        t1 += ab[0];
        t2 += ab[1] + rstd * (ab[4] - ts[0] * ab[2] - ts[1] * ab[3]);
    }
    a.dbias[c] = a.accumulate ? a.dbias[c] + (float)t1 : (float)t1;
    a.dweight[c] = a.accumulate ? a.dweight[c] + (float)t2 : (float)t2;
}

__global__ __launch_bounds__(256) void d3g_gn_dual_dx_kernel(D3GpGnArgs a) {
    const long total = (long)a.N * a.P * a.C, pc = a.P * a.C;
    const double inv_m = 1.0 / ((double)a.P * a.cpg);
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int n = (int)(i / pc), c = (int)(i % a.C), grp = c / a.cpg;
        const double* st = a.stats + ((long)n * D3_GROUPS + grp) * 2;
        const double* ts = a.tstats + ((long)n * D3_GROUPS + grp) * 2;
        const double* gs = a.gs + ((long)n * D3_GROUPS + grp) * 5;
        float dy = a.g[i], dyd = a.gd[i];
        if (a.mask) {
            const bool on = a.mask[i] > 0.f;
            dy = on ? dy : 0.f; dyd = on ? dyd : 0.f;
        }
        const double w = (double)a.weight[c], r = st[1];
        const double xhat = ((double)a.x[i] - st[0]) * r;
        const double Mq = gs[0] * inv_m, Cq = gs[1] * inv_m, Mp = gs[2] * inv_m, Cp = gs[3] * inv_m;
        const double K = gs[4] * inv_m - ts[0] * Mp - ts[1] * Cp;   // mean(p Pi(x'))
        const double pix = (double)a.xd[i] - ts[0] - xhat * ts[1];
        const double pip = (double)dyd * w - Mp - xhat * Cp;
        const double piq = (double)dy * w - Mq - xhat * Cq;
        a.outd[i] = (float)(r * pip);
        a.out[i] = (float)(r * piq - r * r * (xhat * K + ts[1] * pip + Cp * pix));
    }
}

// the tangent of the max pool: the tangent input at the primal's argmax
__global__ __launch_bounds__(256) void d3g_maxpool_tan_kernel(const float* __restrict__ xd, const int* __restrict__ arg, float* __restrict__ out, long total,
                                                              long per_out, long per_in, int C) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += gridDim.x * 256L) {
        const int c = (int)(i % C);
        const long n = i / (per_out * C);
        out[i] = xd[(n * per_in + arg[i]) * C + c];
    }
}

// thread = channel.  With Pdot = (s / n) sum_b w . avg(a'_b): dweight[c] = (s / n) sum_b avg(a'_b)[c] (the samples in order), the adjoint at
// the tangent activation s w[c] / (16 n), the adjoint at the primal activation zero
__global__ __launch_bounds__(256) void d3g_head_dual_kernel(const float* __restrict__ xd, const float* __restrict__ w, float s, float* __restrict__ dx,
                                                            float* __restrict__ dxd, float* __restrict__ dw, int N, int C, int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float seed = s / (float)N;
    const float gc = seed * (w[c] * 0.0625f);
    double acc = 0.0;
    for (int n = 0; n < N; ++n) {
        float t = 0.f;
        for (int p = 0; p < 16; ++p) {
            const long o = ((long)n * 16 + p) * C + c;
            t += xd[o];
            dx[o] = 0.f;
            dxd[o] = gc;
        }
        acc += (double)seed * (double)(t * 0.0625f);
    }
    if (dw) dw[c] = accumulate ? dw[c] + (float)acc : (float)acc;
}

__global__ void d3g_seed_kernel(float* __restrict__ seed, int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) seed[i] = (float)(1.0 / (double)N);
}

// L_GP = the mean of the samples' squared norms, added in sample order
__global__ void d3g_lgp_kernel(const double* __restrict__ sq, int N, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += sq[n];
    *out = s / (double)N;
}

// g [N][3][T][H][W] -> the tangent clip (2 scale / N) g as [N][T][H][W][4] (r, g, b, 0); scale = scale_host (* *scale_dev)
__global__ __launch_bounds__(256) void d3g_tangent_input_kernel(const float* __restrict__ g, float* __restrict__ out, long npix, long thw, float scale_host,
                                                                const float* __restrict__ scale_dev, int N) {
    const float coef = 2.f * (scale_dev ? scale_host * *scale_dev : scale_host) / (float)N;
    for (long i = blockIdx.x * 256L + threadIdx.x; i < npix; i += gridDim.x * 256L) {
        const long n = i / thw, p = i - n * thw;
        const float* s = g + n * 3 * thw + p;
        *reinterpret_cast<float4*>(out + 4 * i) = make_float4(coef * s[0], coef * s[thw], coef * s[2 * thw], 0.f);
    }
}

// =================================================================================================================== host side
// GroupNorm scratch of the pair: `partial` serves the tangent's statistics ([N][16][R][2]) and the dual backward's channel sums ([N][R][C][5])
struct D3GpGnWs { size_t partial, ab, gs, total; };
D3GpGnWs gp_gn_ws(int n, int c) {
    Carver k;
    D3GpGnWs y{};
    y.partial = k.take_bytes((size_t)n * D3_GN_SLICES * std::max(c, D3_GROUPS) * 5 * 8);
    y.ab = k.take_bytes((size_t)n * c * 5 * 8);
    y.gs = k.take_bytes((size_t)n * D3_GROUPS * 5 * 8);
    y.total = k.total();
    return y;
}

int launch_gn_tangent(const float* x, const float* xd, const double* stats, const float* resd, const float* mask, const float* weight, int N, long P,
                      int C, float* out, double* tstats, void* ws, hipStream_t st) {
    const D3GpGnWs k = gp_gn_ws(N, C);
    D3GpGnArgs a{};
    a.x = x; a.xd = xd; a.stats = stats; a.resd = resd; a.mask = mask; a.weight = weight; a.out = out; a.tstats = tstats;
    a.partial = Carver::at<double>(ws, k.partial);
    a.P = P; a.N = N; a.C = C; a.cpg = C / D3_GROUPS; a.R = gn_slices(P, a.cpg); a.rows_per = (P + a.R - 1) / a.R;
    hipLaunchKernelGGL(d3g_gn_tan_stats_kernel, dim3(D3_GROUPS, N, a.R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3g_gn_tan_final_kernel, dim3((N * D3_GROUPS + 255) / 256), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3g_gn_tan_apply_kernel, dim3(grid_for((long)N * P * C)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_gn_dual_bwd(const float* g, const float* gd, const float* mask, const float* x, const float* xd, const double* stats, const double* tstats,
                       const float* weight, int N, long P, int C, float* dx, float* dxd, float* dweight, float* dbias, bool accumulate, void* ws,
                       hipStream_t st) {
    const D3GpGnWs k = gp_gn_ws(N, C);
    D3GpGnArgs a{};
    a.g = g; a.gd = gd; a.mask = mask; a.x = x; a.xd = xd; a.stats = stats; a.tstats = const_cast<double*>(tstats); a.weight = weight;
    a.out = dx; a.outd = dxd; a.dweight = dweight; a.dbias = dbias;
    a.partial = Carver::at<double>(ws, k.partial); a.ab = Carver::at<double>(ws, k.ab); a.gs = Carver::at<double>(ws, k.gs);
    a.P = P; a.N = N; a.C = C; a.cpg = C / D3_GROUPS; a.R = gn_slices(P, 16); a.rows_per = (P + a.R - 1) / a.R; a.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(d3g_gn_dual_partial_kernel, dim3(C / 16, N, a.R), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(d3g_gn_dual_reduce_kernel, dim3(N), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    if (dweight) {
        hipLaunchKernelGGL(d3g_gn_dual_param_kernel, dim3((C + 255) / 256), dim3(256), 0, st, a);
        I2V_LAUNCHED();
    }
    hipLaunchKernelGGL(d3g_gn_dual_dx_kernel, dim3(grid_for((long)N * P * C)), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

int launch_maxpool_tangent(const float* xd, const int* arg, float* out, int N, long per_out, long per_in, int C, hipStream_t st) {
    const long total = (long)N * per_out * C;
    hipLaunchKernelGGL(d3g_maxpool_tan_kernel, dim3(grid_for(total)), dim3(256), 0, st, xd, arg, out, total, per_out, per_in, C);
    I2V_LAUNCHED();
    return I2V_OK;
}

// The weight gradient of a conv from both members: dWn = wgrad(g0, x0) + wgrad(g1, x1).  The existing wgrad kernel runs once per member
// into its own set of slices; the existing finish adds the 2 S slices in slice order and applies the spectral projection ONCE to the sum
// (it is linear in dWn), so the gradient is written or accumulated in one step.  `part`: two sets of wgrad_part_floats.
template <class F>
int launch_wgrad_pair(const TcConv& c, const float* g0, const float* x0, const float* g1, const float* x1, const float* w, const float* u, const float* v,
                      const float* sigma, float* part, float* dwn, double* dotp, float* grad, bool accumulate, const TcGeo& mp, hipStream_t st) {
    I2V_REQUIRE(F::Win::fits(c), I2V_E_INVALID, "%s: a conv outside this family's window", F::NAME);
    int S, L;
    const int ntap = ntap_of(c);
    wgrad_plan(c.cout, c.cin, ntap, mp.mo, &S, &L);
    TcWgradArgs<typename F::Win> a{};
    a.P = mp.mo;
    a.Ti = mp.ti; a.Hi = mp.hi; a.Wi = mp.wi; a.To = mp.to; a.Ho = mp.ho; a.Wo = mp.wo; a.cinp = c.cinp; a.cout = c.cout; a.CP = (int)align_up(c.cinp, 16);
    a.slice_len = L; a.win = F::Win::of(c);
    const int mt = bn_of(c.cout) / 16, nt = bn_of(a.CP) / 16;
    const dim3 grid((unsigned)((c.cout / (16 * mt)) * (a.CP / (16 * nt))), ntap, (unsigned)S);
    const size_t set = (size_t)S * ntap * c.cout * a.CP;
    for (int m = 0; m < 2; ++m) {
        a.g = m ? g1 : g0; a.x = m ? x1 : x0; a.part = part + m * set;
        if (mt == 4) launch_wgrad_nt<F, 4>(nt, grid, st, a);
        else if (mt == 2) launch_wgrad_nt<F, 2>(nt, grid, st, a);
        else launch_wgrad_nt<F, 1>(nt, grid, st, a);
        I2V_LAUNCHED();
    }
    return launch_finish(part, 2 * S, a.CP, c.cout, c.cin, ntap, w, u, v, sigma, dwn, dotp, grad, accumulate, st);
}

// Where the tangent's maps lie in `gp_saved` (offsets from its base) and what the penalty adds behind the trunk's workspace
struct R3GpLayout {
    size_t x4 = 0, pre[D3_MAXCONV] = {}, act[D3_MAXCONV] = {}, tstats[D3_MAXCONV] = {}, pout = 0, saved_total = 0;
    size_t dxf = 0, seed = 0, sq = 0, part = 0, gbuf[4] = {}, dc[2] = {}, gn = 0, ws_total = 0;
};

R3GpLayout r3_gp_layout(const R3Trunk& d, const R3Layout& y) {
    R3GpLayout g;
    Carver s;
    g.x4 = s.take_floats((size_t)y.geo[0].mi * 4);
    size_t cmax = 0;
    for (int i = 0; i < d.nconv; ++i) {
        const size_t elems = (size_t)y.geo[i].mo * d.L[i].cout;
        g.pre[i] = s.take_floats(elems);
        g.act[i] = s.take_floats(elems);
        g.tstats[i] = s.take_bytes((size_t)y.n * D3_GROUPS * 2 * 8);
        cmax = std::max(cmax, (size_t)d.L[i].cout);
    }
    if (d.pool) g.pout = s.take_floats((size_t)y.pool_out * d.L[0].cout);
    g.saved_total = s.total();
    // the workspace: the trunk's own (the clips' gradient runs r3_backward in it; the primal member of the pair uses its buffers), then
    // the clips' gradient, the seeds, the tangent member's buffers and the pair's GroupNorm scratch
    const size_t gbytes = y.gbuf[1] - y.gbuf[0];
    Carver k;
    k.take_bytes(y.ws_total);
    g.dxf = k.take_floats((size_t)y.geo[0].mi * 3);
    g.seed = k.take_floats((size_t)y.n);
    g.sq = k.take_bytes((size_t)y.n * 8);
    g.part = k.take_bytes(2 * (y.dwn - y.part));   // the wgrad slices of both members
    for (int i = 0; i < 4; ++i) g.gbuf[i] = k.take_bytes(gbytes);
    for (int i = 0; i < 2; ++i) g.dc[i] = k.take_bytes(gbytes);
    g.gn = k.take_bytes(gp_gn_ws(y.n, (int)cmax).total);
    g.ws_total = k.total();
    return g;
}

// The tangent forward: xd4 (the tangent clip, at p.x4 of `gsv`) through the network on the decisions, statistics and packed weights of
// `sv`; every tangent map is left in `gsv`
int r3_tangent_forward(const R3Trunk& d, const R3Layout& y, const R3GpLayout& p, const void* sv_, void* gsv, void* workspace, hipStream_t st) {
    void* sv = const_cast<void*>(sv_);
    void* gnws = Carver::at<char>(workspace, p.gn);
    const int n = y.n;
    auto conv_gn = [&](int i, const float* ind, const float* resd, bool relu) -> int {
        const TcConv& c = d.L[i];
        float* pred = Carver::at(gsv, p.pre[i]);
        if (int rc = launch_conv<Trunk3d>(c, ind, Carver::at(sv, y.wf[i]), pred, y.geo[i], st)) return rc;
        return launch_gn_tangent(Carver::at(sv, y.pre[i]), pred, Carver::at<double>(sv, y.stats[i]), resd, relu ? Carver::at(sv, y.act[i]) : nullptr, d.nw[i],
                                 n, y.geo[i].mo / n, c.cout, Carver::at(gsv, p.act[i]), Carver::at<double>(gsv, p.tstats[i]), gnws, st);
    };
    if (int rc = conv_gn(0, Carver::at(gsv, p.x4), nullptr, true)) return rc;
    if (d.pool)
        if (int rc = launch_maxpool_tangent(Carver::at(gsv, p.act[0]), Carver::at<int>(sv, y.parg), Carver::at(gsv, p.pout), n, y.pool_out / n, y.pool_in / n,
                                            d.L[0].cout, st))
            return rc;
    for (int b = 0; b < 8; ++b) {
        const R3Block& k = d.B[b];
        const float* ind = k.in < 0 ? Carver::at(gsv, p.pout) : Carver::at(gsv, p.act[k.in]);
        if (int rc = conv_gn(k.c1, ind, nullptr, true)) return rc;
        const float* resd = ind;
        if (k.cd >= 0) {
            if (int rc = conv_gn(k.cd, ind, nullptr, false)) return rc;
            resd = Carver::at(gsv, p.act[k.cd]);
        }
        if (int rc = conv_gn(k.c2, Carver::at(gsv, p.act[k.c1]), resd, true)) return rc;
    }
    return I2V_OK;
}

// The reverse pass over the pair.  The caller's head has written the adjoints at the last activation (primal: gbuf[0] of the trunk's
// workspace; tangent: p.gbuf[0]).  The parameter gradients go to the bound tensors, written or (`acc`) added, each in one step: a conv's
// two weight gradients are summed before the spectral projection.  No gradient at the clips.
int r3_dual_backward(const R3Trunk& d, const R3Layout& y, const R3GpLayout& p, const void* sv_, const void* gsv_, bool acc, void* workspace, hipStream_t st) {
    void* sv = const_cast<void*>(sv_);
    void* gsv = const_cast<void*>(gsv_);
    const int n = y.n;
    float* part = Carver::at(workspace, p.part);
    float* dwn = Carver::at(workspace, y.dwn);
    double* dotp = Carver::at<double>(workspace, y.dotp);
    void* gnws = Carver::at<char>(workspace, p.gn);
    // [0]: the primal member, [1]: the tangent member
    float* G[2] = {Carver::at(workspace, y.gbuf[0]), Carver::at(workspace, p.gbuf[0])};
    float* Gn[2] = {Carver::at(workspace, y.gbuf[1]), Carver::at(workspace, p.gbuf[1])};
    float* H1[2] = {Carver::at(workspace, y.gbuf[2]), Carver::at(workspace, p.gbuf[2])};
    float* X2[2] = {Carver::at(workspace, y.gbuf[3]), Carver::at(workspace, p.gbuf[3])};
    float* DC[2] = {Carver::at(workspace, y.dc[0]), Carver::at(workspace, p.dc[0])};
    float* DC2[2] = {Carver::at(workspace, y.dc[1]), Carver::at(workspace, p.dc[1])};

    // GroupNorm of conv i backwards for the pair: g (masked by `mask`) -> dc; then the conv's weight gradient from both members
    auto norm_conv_bwd = [&](int i, float* const* g, const float* mask, const float* xin, const float* xind, float* const* dc) -> int {
        const TcConv& c = d.L[i];
        if (int rc = launch_gn_dual_bwd(g[0], g[1], mask, Carver::at(sv, y.pre[i]), Carver::at(gsv, p.pre[i]), Carver::at<double>(sv, y.stats[i]),
                                        Carver::at<double>(gsv, p.tstats[i]), d.nw[i], n, y.geo[i].mo / n, c.cout, dc[0], dc[1], d.gnw[i], d.gnb[i], acc,
                                        gnws, st))
            return rc;
        const float* us = c.sn ? Carver::at(sv, y.us[i]) : nullptr;
        const float* vs = c.sn ? Carver::at(sv, y.vs[i]) : nullptr;
        const float* sg = c.sn ? Carver::at(sv, y.sigma[i]) : nullptr;
        return launch_wgrad_pair<Trunk3d>(c, dc[0], xin, dc[1], xind, d.w[i], us, vs, sg, part, dwn, dotp, d.gw[i], acc, y.geo[i], st);
    };
    auto dgrad2 = [&](int i, float* const* dc, float* const* add, const float* add_mask, float* const* out) -> int {
        for (int m = 0; m < 2; ++m)
            if (int rc = launch_dgrad<Trunk3d>(d.L[i], dc[m], nullptr, nullptr, Carver::at(sv, y.wd[i]), add ? add[m] : nullptr, add ? add_mask : nullptr,
                                               out[m], false, n, y.geo[i], st))
                return rc;
        return I2V_OK;
    };
    for (int b = 7; b >= 0; --b) {
        const R3Block& k = d.B[b];
        const float* out = Carver::at(sv, y.act[k.c2]);
        const float* xin = k.in < 0 ? Carver::at(sv, y.pout) : Carver::at(sv, y.act[k.in]);
        const float* xind = k.in < 0 ? Carver::at(gsv, p.pout) : Carver::at(gsv, p.act[k.in]);
        const float* h1 = Carver::at(sv, y.act[k.c1]);
        const float* h1d = Carver::at(gsv, p.act[k.c1]);
        if (int rc = norm_conv_bwd(k.c2, G, out, h1, h1d, DC)) return rc;
        if (int rc = dgrad2(k.c2, DC, nullptr, nullptr, H1)) return rc;
        if (int rc = norm_conv_bwd(k.c1, H1, h1, xin, xind, DC)) return rc;
        if (k.cd >= 0) {
            if (int rc = norm_conv_bwd(k.cd, G, out, xin, xind, DC2)) return rc;
            if (int rc = dgrad2(k.cd, DC2, nullptr, nullptr, X2)) return rc;
            if (int rc = dgrad2(k.c1, DC, X2, nullptr, Gn)) return rc;
        } else if (int rc = dgrad2(k.c1, DC, G, out, Gn)) {
            return rc;
        }
        std::swap(G[0], Gn[0]); std::swap(G[1], Gn[1]);
    }
    if (d.pool) {
        const long total = y.pool_in * d.L[0].cout;
        for (int m = 0; m < 2; ++m) {
            hipLaunchKernelGGL(d3_maxpool_bwd_kernel, dim3(grid_for(total)), dim3(256), 0, st, G[m], Carver::at<int>(sv, y.parg), Gn[m], total, y.pt, y.ph,
                               y.pw, y.pho, y.pwo, d.L[0].cout);
            I2V_LAUNCHED();
        }
        std::swap(G[0], Gn[0]); std::swap(G[1], Gn[1]);
    }
    return norm_conv_bwd(0, G, Carver::at(sv, y.act[0]), Carver::at(sv, y.x4), Carver::at(gsv, p.x4), DC);
}

}  // namespace
}  // namespace i2v
