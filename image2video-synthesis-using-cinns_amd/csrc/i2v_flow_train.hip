// Training path of the cINN flow (i2v_flow_train_*, i2v_adam_step): forward with saved activations, backward, fused Adam.
//
// Unlike the inference handle (i2v_flow.hip / i2v_flow_tile.hip), which packs the parameters on the host into streaming
// layouts once, this path reads the parameters WHERE THE nn.Parameters LIVE, in their state_dict layout (torch [out][in]),
// through device pointers bound once: an optimiser step is seen by the next forward with no re-load.
//
// Every Linear of forward and backward is a tile of v_mfma_f32_16x16x4_f32 (exact fp32): D[m][n] = sum_r A[m][r] B[r][n] with
// n = the sample on the lane.  Three products per layer:
//   forward   Y[b][o]  = sum_k X[b][k]  W[o][k]     m = o, r = k   (chain_gemm<0>)
//   dX        dX[b][k] = sum_o dY[b][o] W[o][k]     m = k, r = o   (chain_gemm<1>; W read column-wise, coalesced over m)
//   dW        dW[o][k] = sum_b dY[b][o] X[b][k]     m = o, n = k, r = b   (dw_gemm; one owner per output tile, plain stores)
// Only forward and dX sit on the dependent chain; dW / db / ActNorm gradients are computed from the kept dY buffers by three
// batched launches over ALL half-steps behind the chain.  No atomics anywhere: every gradient element has one owner and a
// fixed summation order, so two runs give the same bits.
#include <cmath>

#include "i2v_flow_tile.h"
#include "i2v_handle.h"

namespace i2v {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Layout of the `saved` buffer, in floats.  Per half-step st: xs [B][64] (the state entering the half-step, halves already
// swapped: [:32] feeds the nets and is kept, [32:] is transformed), cin [B][KP] (conditioner input, KP = Kin rounded up to 4),
// act [2 nets][depth + 1][B][H] (post-LeakyReLU outputs), out [2][B][32] (s, t), and the backward's dpre (same shape as act:
// gradients of the pre-activations) and dout.  Then per block: xin (block input) and gan (gradient at the ActNorm output);
// then part [B][64] (gradient of the half-step input without the conditioner term) and dcin [B][KP].
struct TrainLayout {
    int B, H, depth, E, KP, S, nfl;
    size_t BH, o_cin, o_act, o_out, o_dpre, o_dout, step_sz, o_xin, o_gan, o_part, o_dcin, total;
    __host__ __device__ size_t xs(int st) const { return (size_t)st * step_sz; }
    __host__ __device__ size_t cin(int st) const { return (size_t)st * step_sz + o_cin; }
    __host__ __device__ size_t act(int st, int net, int l) const { return (size_t)st * step_sz + o_act + (size_t)(net * (depth + 1) + l) * BH; }
    __host__ __device__ size_t out(int st, int net) const { return (size_t)st * step_sz + o_out + (size_t)net * B * 32; }
    __host__ __device__ size_t dpre(int st, int net, int l) const { return (size_t)st * step_sz + o_dpre + (size_t)(net * (depth + 1) + l) * BH; }
    __host__ __device__ size_t dout(int st, int net) const { return (size_t)st * step_sz + o_dout + (size_t)net * B * 32; }
    __host__ __device__ size_t xin(int fl) const { return o_xin + (size_t)fl * B * 64; }
    __host__ __device__ size_t gan(int fl) const { return o_gan + (size_t)fl * B * 64; }
};

TrainLayout make_layout(int B, int H, int depth, int E, int nfl) {
    TrainLayout L;
    L.B = B; L.H = H; L.depth = depth; L.E = E; L.nfl = nfl; L.S = 2 * nfl;
    L.KP = (32 + E + 3) / 4 * 4;
    L.BH = (size_t)B * H;
    L.o_cin = (size_t)B * 64;
    L.o_act = L.o_cin + (size_t)B * L.KP;
    L.o_out = L.o_act + 2 * (size_t)(depth + 1) * L.BH;
    L.o_dpre = L.o_out + 2 * (size_t)B * 32;
    L.o_dout = L.o_dpre + 2 * (size_t)(depth + 1) * L.BH;
    L.step_sz = L.o_dout + 2 * (size_t)B * 32;
    L.o_xin = (size_t)L.S * L.step_sz;
    L.o_gan = L.o_xin + (size_t)nfl * B * 64;
    L.o_part = L.o_gan + (size_t)nfl * B * 64;
    L.o_dcin = L.o_part + (size_t)B * 64;
    L.total = L.o_dcin + (size_t)B * L.KP;
    return L;   // every offset is a multiple of 4 floats (64, KP, H and 32 are): 16-byte vector accesses stay aligned
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- the two products on the dependent chain ------------------------------------------------------------------------------
struct ChainArgs {
    const float* W[2];      // per net (blockIdx.z), or per reduction segment (nseg = 2)
    const float* X[2];      // B operand: [B][ldx], the reduction index contiguous
    const float* bias[2];   // MODE 0
    const float* mask[2];   // MODE 1: saved post-activation of the layer whose pre-activation gradient is formed (null: none)
    float* Y[2];            // [B][ldy]
    int M;                  // rows of D: output features (MODE 0) / input features (MODE 1)
    int R;                  // reduction length: input features (MODE 0) / output features (MODE 1)
    int ldw, ldx, ldy, B;
    int nseg;               // 2: both nets are two segments of ONE reduction into Y[0] (dX of the first layer)
    int lrelu;
};

// One workgroup = 16 rows of D x up to 64 samples; its four waves split the reduction, add their partial tiles through LDS in
// a fixed order, and each wave finishes one 16-sample tile.  The weight fragment of a wave is used against all four sample
// tiles.  MODE 0: A[m][r] = W[m * ldw + r]; MODE 1: A[m][r] = W[r * ldw + m].  VEC: the r-contiguous operands are read as
// 16-byte vectors (R % 16 == 0, strides % 4 == 0); otherwise element-wise with bounds (first layer at E = 94: K = 126).
// The k index inside a 16-chunk is permuted (MFMA step j of lane quarter q takes r = 16 c + 4 q + j) for both operands alike.
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void chain_gemm(const ChainArgs a) {
    __shared__ f32x4 red[4][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = lane >> 4, l16 = lane & 15;
    const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 64;
    const int nt = min(4, (a.B - n0 + 15) / 16);
    const int chunks = (a.R + 15) / 16, cpw = (chunks + 3) / 4;
    const int c0 = w * cpw, c1 = min(chunks, c0 + cpw);
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int m = m0 + l16;
    for (int seg = 0; seg < a.nseg; ++seg) {
        const int sn = a.nseg == 2 ? seg : (int)blockIdx.z;
        const float* __restrict__ W = a.W[sn];
        const float* __restrict__ X = a.X[sn];
#pragma unroll 2
        for (int c = c0; c < c1; ++c) {
            const int r = c * 16 + 4 * q;
            float av[4];
            if (MODE == 0) {
                if (VEC) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(W + (size_t)m * a.ldw + r);
                    av[0] = v[0]; av[1] = v[1]; av[2] = v[2]; av[3] = v[3];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) av[j] = (m < a.M && r + j < a.R) ? W[(size_t)m * a.ldw + r + j] : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) av[j] = (m < a.M && r + j < a.R) ? W[(size_t)(r + j) * a.ldw + m] : 0.f;
            }
            f32x4 bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int n = n0 + 16 * t + l16;
                bv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (t < nt && n < a.B) {
                    if (VEC) {
                        bv[t] = *reinterpret_cast<const f32x4*>(X + (size_t)n * a.ldx + r);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) bv[t][j] = (r + j < a.R) ? X[(size_t)n * a.ldx + r + j] : 0.f;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[t][j], acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) red[w][t][lane] = acc[t];
    __syncthreads();
    if (w >= nt) return;
    f32x4 v = red[0][w][lane];
    v += red[1][w][lane];
    v += red[2][w][lane];
    v += red[3][w][lane];
    const int n = n0 + 16 * w + l16;
    const int mr = m0 + 4 * q;   // this lane holds rows mr .. mr + 3 of sample n
    if (n >= a.B) return;
    const int on = a.nseg == 2 ? 0 : (int)blockIdx.z;
    if (MODE == 0) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias[on] + mr);
        v += b;
        if (a.lrelu) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.f ? v[i] : v[i] * 0.01f;
        }
        *reinterpret_cast<f32x4*>(a.Y[on] + (size_t)n * a.ldy + mr) = v;
    } else {
        if (mr + 3 >= a.ldy) return;   // rows past M hold zeros and fall into the padding of the row, or are dropped here
        if (a.mask[on]) {
            const f32x4 mk = *reinterpret_cast<const f32x4*>(a.mask[on] + (size_t)n * a.ldy + mr);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = mk[i] > 0.f ? v[i] : v[i] * 0.01f;
        }
        *reinterpret_cast<f32x4*>(a.Y[on] + (size_t)n * a.ldy + mr) = v;
    }
}

// ---- weight and bias gradients, batched over every half-step ------------------------------------------------------------------
struct DwEntry {
    long long gW, gb;   // byte offsets of the gradient tensors from the gradient base
    int st, net, layer, M, K;
    int pad;
};

// grid (ceil(M / 64), ceil(K / 64), entries): wave w of a workgroup owns rows 16 (4 x + w) .. + 15 and 64 columns of dW and sums
// over the whole batch; db falls out of one more MFMA against a B operand of ones (the wave of column block 0 stores it).
__global__ __launch_bounds__(256) void dw_gemm(const DwEntry* __restrict__ tab, int ent0, const TrainLayout L, const float* __restrict__ saved,
                                               char* gbase, int accumulate) {
    const DwEntry e = tab[ent0 + blockIdx.z];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = lane >> 4, l16 = lane & 15;
    const int m0 = (blockIdx.x * 4 + w) * 16, i0 = blockIdx.y * 64;
    if (m0 >= e.M || i0 >= e.K) return;
    const float* dY; const float* X; int ldd, ldx;
    if (e.layer == 0) { dY = saved + L.dpre(e.st, e.net, 0); ldd = L.H; X = saved + L.cin(e.st); ldx = L.KP; }
    else if (e.layer <= L.depth) { dY = saved + L.dpre(e.st, e.net, e.layer); ldd = L.H; X = saved + L.act(e.st, e.net, e.layer - 1); ldx = L.H; }
    else { dY = saved + L.dout(e.st, e.net); ldd = 32; X = saved + L.act(e.st, e.net, L.depth); ldx = L.H; }
    f32x4 acc[4], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nt = min(4, (e.K - i0 + 15) / 16);
#pragma unroll 2
    for (int r0 = 0; r0 < L.B; r0 += 4) {
        const int r = r0 + q;
        const float av = r < L.B ? dY[(size_t)r * ldd + m0 + l16] : 0.f;
        float bv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = i0 + 16 * t + l16;
            bv[t] = (r < L.B && n < e.K) ? X[(size_t)r * ldx + n] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (t < nt) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t], 0, 0, 0);
        accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accb, 0, 0, 0);
    }
    float* gW = reinterpret_cast<float*>(gbase + e.gW);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = m0 + 4 * q + i;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = i0 + 16 * t + l16;
            if (t < nt && n < e.K) {
                float* p = gW + (size_t)m * e.K + n;
                *p = accumulate ? *p + acc[t][i] : acc[t][i];
            }
        }
    }
    if (blockIdx.y == 0 && l16 == 0) {
        float* gb = reinterpret_cast<float*>(gbase + e.gb);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float* p = gb + m0 + 4 * q + i;
            *p = accumulate ? *p + accb[i] : accb[i];
        }
    }
}

// ---- ActNorm gradients (modules.py:80-89): d_loc = sum_b g scale, d_scale = sum_b g (x + loc) + sum_b d_logdet[b] / scale ------
struct AnEntry {
    const float* loc; const float* scale;
    long long gloc, gscale;
};
__global__ __launch_bounds__(64) void actnorm_grad(const AnEntry* __restrict__ tab, const TrainLayout L, const float* __restrict__ saved,
                                                   const float* __restrict__ dld, char* gbase, int accumulate) {
    const AnEntry e = tab[blockIdx.x];
    const int c = threadIdx.x;
    const float* g = saved + L.gan(blockIdx.x);
    const float* x = saved + L.xin(blockIdx.x);
    const float sc = e.scale[c], lc = e.loc[c];
    float s1 = 0.f, s2 = 0.f, sd = 0.f;
    for (int b = 0; b < L.B; ++b) {
        const float gv = g[(size_t)b * 64 + c];
        s1 += gv;
        s2 += gv * (x[(size_t)b * 64 + c] + lc);
        sd += dld[b];
    }
    float* gl = reinterpret_cast<float*>(gbase + e.gloc) + c;
    float* gs = reinterpret_cast<float*>(gbase + e.gscale) + c;
    const float dl = s1 * sc, ds = s2 + sd / sc;
    *gl = accumulate ? *gl + dl : dl;
    *gs = accumulate ? *gs + ds : ds;
}

// ---- element-wise links of the chain: one wave per sample, channel on the lane ----------------------------------------------
struct FwdArgs {
    TrainLayout L;
    float* saved;
    const float* x; const float* embed;
    float* zt; float* logdet;
    const float* loc_next; const float* scale_next;   // ActNorm of the block that starts at step st + 1 (null: none)
    const long long* shuf;                            // forward_shuffle_idx of the block that ends at step st (null: none)
    int st;                                           // half-step whose s / t have just been computed; -1: the entry
    int cond_next;                                    // step st + 1 conditions on the embedding only (mode 'cond')
    int use_act;
};

// coupling of step st (flow_blocks.py:88-93), then either the half swap or Shuffle -> ActNorm -> InvLeakyRelu of the next block,
// and the conditioner input of step st + 1
__global__ __launch_bounds__(256) void fwd_link(const FwdArgs a) {
    const TrainLayout& L = a.L;
    const int c = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;
    const int st = a.st;
    float y, ld = 0.f;
    if (st < 0) {
        y = a.x[(size_t)b * 64 + c];
    } else {
        y = a.saved[L.xs(st) + (size_t)b * 64 + c];
        float s = 0.f;
        if (c >= 32) {
            s = a.saved[L.out(st, 0) + (size_t)b * 32 + c - 32];
            y = y * expf(s) + a.saved[L.out(st, 1) + (size_t)b * 32 + c - 32];
        }
        ld = wave_sum(s);
    }
    if (st >= 0 && !(st & 1)) {
        y = __shfl(y, c ^ 32);   // the second coupling of the block works on the swapped halves
    } else {
        if (st >= 0 && a.shuf) y = __shfl(y, (int)a.shuf[c]);
        if (st == L.S - 1) {
            a.zt[(size_t)b * 64 + c] = y;
            if (c == 0) a.logdet[b] += ld;
            return;
        }
        a.saved[L.xin((st + 1) / 2) + (size_t)b * 64 + c] = y;
        if (a.loc_next) {
            const float sc = a.scale_next[c];
            y = sc * (y + a.loc_next[c]);
            ld += wave_sum(logf(fabsf(sc)));
        }
        if (a.use_act) y = y >= 0.f ? y : y * 0.9f;   // InvLeakyRelu.forward; its log-det is reported as 0 (quirk Q2)
    }
    a.saved[L.xs(st + 1) + (size_t)b * 64 + c] = y;
    float* cin = a.saved + L.cin(st + 1) + (size_t)b * L.KP;
    const int off = a.cond_next ? 0 : 32;
    if (!a.cond_next && c < 32) cin[c] = y;
    for (int e = c; off + e < L.KP; e += 64) cin[off + e] = e < L.E ? a.embed[(size_t)b * L.E + e] : 0.f;
    if (c == 0) a.logdet[b] = (st < 0 ? 0.f : a.logdet[b]) + ld;
}

struct BwdArgs {
    TrainLayout L;
    float* saved;
    const float* d_zt; const float* d_logdet;
    float* d_x; float* d_embed;
    const float* scale;      // ActNorm scale of the block that starts at step st + 1 (null: none / not a block start)
    const long long* bshuf;  // backward_shuffle_idx of the block that ends at step st (null: none)
    int st;                  // half-step whose coupling backward is started; -1: the exit
    int cond1;               // mode of step st + 1
    int first;               // st == S - 1: the gradient comes from d_zt
    int use_act;
};

// finishes the backward of step st + 1 (conditioner gradient into the kept half and into d_embed, un-swap or
// InvLeakyRelu / ActNorm / Shuffle backward), then starts step st: ds = dy x exp(s) + d_logdet, dt = dy, dx = dy exp(s)
__global__ __launch_bounds__(256) void bwd_link(const BwdArgs a) {
    const TrainLayout& L = a.L;
    const int c = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;
    const int st = a.st;
    float dy;
    if (a.first) {
        dy = a.d_zt[(size_t)b * 64 + (a.bshuf ? (int)a.bshuf[c] : c)];
    } else {
        const int t1 = st + 1;
        float gx = a.saved[L.o_part + (size_t)b * 64 + c];
        const float* dcin = a.saved + L.o_dcin + (size_t)b * L.KP;
        if (!a.cond1 && c < 32) gx += dcin[c];
        if (a.d_embed) {
            const int off = a.cond1 ? 0 : 32;
            for (int e = c; e < L.E; e += 64) {
                float* p = a.d_embed + (size_t)b * L.E + e;
                *p = (t1 == L.S - 1) ? dcin[off + e] : *p + dcin[off + e];
            }
        }
        if (t1 & 1) {
            dy = __shfl(gx, c ^ 32);
        } else {
            const int fl = t1 >> 1;
            if (a.use_act) gx *= a.saved[L.xs(t1) + (size_t)b * 64 + c] >= 0.f ? 1.f : 0.9f;
            a.saved[L.gan(fl) + (size_t)b * 64 + c] = gx;
            if (a.scale) gx *= a.scale[c];
            if (fl == 0) {
                if (a.d_x) a.d_x[(size_t)b * 64 + c] = gx;
                return;
            }
            dy = a.bshuf ? __shfl(gx, (int)a.bshuf[c]) : gx;
        }
    }
    float p = dy;
    if (c >= 32) {
        const size_t o = (size_t)b * 32 + c - 32;
        const float es = expf(a.saved[L.out(st, 0) + o]);
        a.saved[L.dout(st, 0) + o] = dy * a.saved[L.xs(st) + (size_t)b * 64 + c] * es + a.d_logdet[b];
        a.saved[L.dout(st, 1) + o] = dy;
        p = dy * es;
    }
    a.saved[L.o_part + (size_t)b * 64 + c] = p;
}

// ---- Adam over a table of tensors (torch.optim.Adam, single-tensor formulas) --------------------------------------------------
constexpr int ADAM_CHUNK = 2048;   // elements per workgroup: 256 threads x 2 x 4

struct AdamScalars {
    float step_size, beta1, beta2, eps, wd, bc2_sqrt;
    int amsgrad;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float& vm, const AdamScalars& s) {
    if (s.wd != 0.f) g += s.wd * p;
    m += (g - m) * (1.f - s.beta1);
    v = v * s.beta2 + (1.f - s.beta2) * g * g;
    float d;
    if (s.amsgrad) { vm = fmaxf(vm, v); d = sqrtf(vm) / s.bc2_sqrt + s.eps; }
    else d = sqrtf(v) / s.bc2_sqrt + s.eps;
    p -= s.step_size * (m / d);
}

__global__ __launch_bounds__(256) void adam_kernel(const i2v_adam_tensor* __restrict__ tab, const int* __restrict__ chunks, const AdamScalars s) {
    const int ti = chunks[2 * blockIdx.x];
    const long long start = chunks[2 * blockIdx.x + 1];
    const i2v_adam_tensor t = tab[ti];
    const bool al = ((((size_t)t.param) | ((size_t)t.grad) | ((size_t)t.exp_avg) | ((size_t)t.exp_avg_sq) | ((size_t)t.max_exp_avg_sq)) & 15) == 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const long long i = start + (long long)(k * 256 + threadIdx.x) * 4;
        if (i >= t.numel) continue;
        if (al && i + 3 < t.numel) {
            f32x4 p = *reinterpret_cast<f32x4*>(t.param + i);
            const f32x4 g = *reinterpret_cast<const f32x4*>(t.grad + i);
            f32x4 m = *reinterpret_cast<f32x4*>(t.exp_avg + i);
            f32x4 v = *reinterpret_cast<f32x4*>(t.exp_avg_sq + i);
            f32x4 vm = f32x4{0.f, 0.f, 0.f, 0.f};
            if (s.amsgrad) vm = *reinterpret_cast<f32x4*>(t.max_exp_avg_sq + i);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = p[j], mj = m[j], vj = v[j], vmj = vm[j];
                adam_one(pj, g[j], mj, vj, vmj, s);
                p[j] = pj; m[j] = mj; v[j] = vj; vm[j] = vmj;
            }
            *reinterpret_cast<f32x4*>(t.param + i) = p;
            *reinterpret_cast<f32x4*>(t.exp_avg + i) = m;
            *reinterpret_cast<f32x4*>(t.exp_avg_sq + i) = v;
            if (s.amsgrad) *reinterpret_cast<f32x4*>(t.max_exp_avg_sq + i) = vm;
        } else {
            for (int j = 0; j < 4 && i + j < t.numel; ++j) {
                float vm = s.amsgrad ? t.max_exp_avg_sq[i + j] : 0.f;
                adam_one(t.param[i + j], t.grad[i + j], t.exp_avg[i + j], t.exp_avg_sq[i + j], vm, s);
                if (s.amsgrad) t.max_exp_avg_sq[i + j] = vm;
            }
        }
    }
}

}  // namespace
}  // namespace i2v

using namespace i2v;

struct i2v_flow_train {
    i2v_flow_cfg cfg{};
    int device = 0;
    int S = 0, H = 0, depth = 0, E = 0, nfl = 0;
    std::vector<int> step_cond;                       // [S]
    struct Lin { const float* W; const float* b; };
    std::vector<Lin> lin;                             // [S][2][depth + 2]
    std::vector<AnEntry> an;                          // [nfl]
    std::vector<const long long*> shuf_f, shuf_b;     // [nfl]
    DevBuf dw_tab, an_tab;
    int n_l0 = 0, n_mid = 0, n_l3 = 0;                // entries of dw_tab, in this order
    bool bound = false;
    StreamOrder order;
    const Lin& L(int st, int net, int l) const { return lin[((size_t)st * 2 + net) * (depth + 2) + l]; }
    int kin(int st) const { return step_cond[st] ? E : 32 + E; }
};

extern "C" size_t i2v_flow_train_saved_bytes(const i2v_flow_train* f, int32_t batch);

static int train_call_checks(const i2v_flow_train* f, const void* saved, size_t saved_bytes, int batch, const char* what) {
    I2V_REQUIRE(f, I2V_E_INVALID, "%s: null handle", what);
    I2V_REQUIRE(f->bound, I2V_E_STATE, "%s: no parameters bound (call i2v_flow_train_bind first)", what);
    I2V_REQUIRE(batch >= 1, I2V_E_INVALID, "%s: batch %d", what, batch);
    I2V_REQUIRE(saved && (reinterpret_cast<size_t>(saved) & 15) == 0, I2V_E_INVALID, "%s: `saved` is null or not 16-byte aligned", what);
    I2V_REQUIRE(saved_bytes >= i2v_flow_train_saved_bytes(f, batch), I2V_E_WORKSPACE, "%s: `saved` holds %zu bytes, batch %d needs %zu", what,
                saved_bytes, batch, i2v_flow_train_saved_bytes(f, batch));
    return I2V_OK;
}

template <int MODE>
static void launch_chain(const ChainArgs& a, bool vec, int nets, hipStream_t st) {
    // MODE 1 covers every row of Y up to ldy, not only the M rows of W: the rows between hold zeros (dcin in 'cond' mode, where
    // KP - M >= 32, would otherwise keep whatever `saved` held there)
    const dim3 grid(((MODE == 1 ? a.ldy : a.M) + 15) / 16, (a.B + 63) / 64, nets);
    if (vec) hipLaunchKernelGGL((chain_gemm<MODE, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((chain_gemm<MODE, false>), grid, dim3(256), 0, st, a);
}

extern "C" {

int i2v_flow_train_create(const i2v_flow_cfg* cfg, i2v_flow_train** out) {
    I2V_REQUIRE(cfg && out, I2V_E_INVALID, "i2v_flow_train_create: null argument");
    I2V_REQUIRE(cfg->linear_f16 == 0, I2V_E_INVALID,
                "i2v_flow_train_create: linear_f16 = 1 is an inference mode; the training path is exact fp32 only");
    I2V_REQUIRE(cfg->n_flows >= 1 && cfg->control >= 0 && cfg->control <= 2 && (cfg->activation == 0 || cfg->activation == 1),
                I2V_E_INVALID, "i2v_flow_train_create: n_flows %d / control %d / activation %d out of range", cfg->n_flows, cfg->control,
                cfg->activation);
    I2V_REQUIRE(flow_tile_geometry_ok(cfg->in_channels, cfg->hidden_dim, cfg->hidden_depth, cfg->embedding_dim), I2V_E_INVALID,
                "i2v_flow_train_create: unsupported geometry (in_channels %d, hidden_dim %d, hidden_depth %d, embedding_dim %d): the "
                "training path covers 64 channels, hidden 128..512 in steps of 128, depth >= 1, embedding <= 128",
                cfg->in_channels, cfg->hidden_dim, cfg->hidden_depth, cfg->embedding_dim);
    auto* f = new i2v_flow_train();
    f->cfg = *cfg;
    I2V_HIP_CHECK(hipGetDevice(&f->device));
    f->nfl = cfg->n_flows; f->S = 2 * cfg->n_flows; f->H = cfg->hidden_dim; f->depth = cfg->hidden_depth; f->E = cfg->embedding_dim;
    f->step_cond.resize(f->S);
    for (int st = 0; st < f->S; ++st) f->step_cond[st] = flow_block_cond(cfg->control, st / 2);
    *out = f;
    return I2V_OK;
}

void i2v_flow_train_destroy(i2v_flow_train* f) { delete f; }

size_t i2v_flow_train_saved_bytes(const i2v_flow_train* f, int32_t batch) {
    if (!f || batch < 1) return 0;
    return make_layout(batch, f->H, f->depth, f->E, f->nfl).total * sizeof(float);
}

int i2v_flow_train_saved_layout(int32_t hidden, int32_t depth, int32_t embedding_dim, int32_t n_flows, int32_t batch,
                                i2v_flow_train_layout* out) {
    I2V_REQUIRE(out, I2V_E_INVALID, "i2v_flow_train_saved_layout: null argument");
    I2V_REQUIRE(n_flows >= 1 && batch >= 1, I2V_E_INVALID, "i2v_flow_train_saved_layout: n_flows %d / batch %d", n_flows, batch);
    I2V_REQUIRE(flow_tile_geometry_ok(64, hidden, depth, embedding_dim), I2V_E_INVALID,
                "i2v_flow_train_saved_layout: unsupported geometry (hidden_dim %d, hidden_depth %d, embedding_dim %d)", hidden, depth,
                embedding_dim);
    const TrainLayout L = make_layout(batch, hidden, depth, embedding_dim, n_flows);
    out->KP = L.KP; out->step_sz = (int64_t)L.step_sz;
    out->o_cin = (int64_t)L.o_cin; out->o_act = (int64_t)L.o_act; out->o_out = (int64_t)L.o_out; out->o_dpre = (int64_t)L.o_dpre;
    out->o_dout = (int64_t)L.o_dout; out->o_xin = (int64_t)L.o_xin; out->o_gan = (int64_t)L.o_gan; out->o_part = (int64_t)L.o_part;
    out->o_dcin = (int64_t)L.o_dcin; out->total = (int64_t)L.total;
    return I2V_OK;
}

int i2v_flow_train_bind(i2v_flow_train* f, const i2v_tensor* params, const i2v_tensor* grads, int32_t n) {
    I2V_REQUIRE(f && params && grads && n > 0, I2V_E_INVALID, "i2v_flow_train_bind: null argument");
    I2V_REQUIRE_DEVICE(f->device, "i2v_flow_train_bind");
    f->bound = false;
    StateDict P(params, n), G(grads, n);
    const int H = f->H, depth = f->depth, nl = depth + 2;
    auto aligned = [](const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; };
    // the gradient "pointer" may be a byte offset into a flat buffer (see i2v_flow_train_backward): 0 is a valid value, so the
    // lookup goes through the map directly
    auto grad_of = [&](const std::string& key, int64_t numel, long long* off) -> int {
        auto it = G.map.find(key);
        I2V_REQUIRE(it != G.map.end() && it->second->dtype == I2V_F32 && it->second->numel == numel, I2V_E_MISSING,
                    "i2v_flow_train_bind: gradient tensor '%s' missing or not %lld float32 elements", key.c_str(), (long long)numel);
        I2V_REQUIRE(aligned(it->second->data), I2V_E_INVALID, "i2v_flow_train_bind: gradient of '%s' is not 16-byte aligned", key.c_str());
        *off = (long long)reinterpret_cast<size_t>(it->second->data);
        return I2V_OK;
    };
    f->lin.assign((size_t)f->S * 2 * nl, {});
    std::vector<DwEntry> tabs[3];
    for (int st = 0; st < f->S; ++st) {
        const int fl = st / 2, i = st & 1, kin = f->kin(st);
        for (int net = 0; net < 2; ++net) {
            for (int l = 0; l < nl; ++l) {
                const int M = l == nl - 1 ? 32 : H, K = l == 0 ? kin : H;
                const std::string base = flow_linear_key(fl, net, i, l);
                const float* W = P.f32(base + ".weight", (int64_t)M * K);
                if (!W) return I2V_E_MISSING;
                const float* b = P.f32(base + ".bias", M);
                if (!b) return I2V_E_MISSING;
                I2V_REQUIRE(aligned(W) && aligned(b), I2V_E_INVALID, "i2v_flow_train_bind: '%s' is not 16-byte aligned", base.c_str());
                f->lin[((size_t)st * 2 + net) * nl + l] = {W, b};
                DwEntry e{};
                int rc = grad_of(base + ".weight", (int64_t)M * K, &e.gW);
                if (rc) return rc;
                rc = grad_of(base + ".bias", M, &e.gb);
                if (rc) return rc;
                e.st = st; e.net = net; e.layer = l; e.M = M; e.K = K;
                tabs[l == 0 ? 0 : (l == nl - 1 ? 2 : 1)].push_back(e);
            }
        }
    }
    f->an.assign(f->nfl, {});
    f->shuf_f.assign(f->nfl, nullptr);
    f->shuf_b.assign(f->nfl, nullptr);
    for (int fl = 0; fl < f->nfl; ++fl) {
        const std::string pre = "sub_layers." + std::to_string(fl) + ".";
        if (!f->cfg.skip_actnorm) {
            AnEntry& e = f->an[fl];
            e.loc = P.f32(pre + "norm_layer.loc", 64);
            if (!e.loc) return I2V_E_MISSING;
            e.scale = P.f32(pre + "norm_layer.scale", 64);
            if (!e.scale) return I2V_E_MISSING;
            int rc = grad_of(pre + "norm_layer.loc", 64, &e.gloc);
            if (rc) return rc;
            rc = grad_of(pre + "norm_layer.scale", 64, &e.gscale);
            if (rc) return rc;
        }
        if (!f->cfg.skip_shuffle) {
            const int64_t* sf = P.i64(pre + "shuffle.forward_shuffle_idx", 64);
            if (!sf) return I2V_E_MISSING;
            const int64_t* sb = P.i64(pre + "shuffle.backward_shuffle_idx", 64);
            if (!sb) return I2V_E_MISSING;
            f->shuf_f[fl] = reinterpret_cast<const long long*>(sf);
            f->shuf_b[fl] = reinterpret_cast<const long long*>(sb);
        }
    }
    std::vector<DwEntry> all;
    for (auto& t : tabs) all.insert(all.end(), t.begin(), t.end());
    f->n_l0 = (int)tabs[0].size(); f->n_mid = (int)tabs[1].size(); f->n_l3 = (int)tabs[2].size();
    int rc = f->dw_tab.upload(all.data(), all.size() * sizeof(DwEntry));
    if (rc) return rc;
    rc = f->an_tab.upload(f->an.data(), f->an.size() * sizeof(AnEntry));
    if (rc) return rc;
    f->bound = true;
    return I2V_OK;
}

int i2v_flow_train_forward(i2v_flow_train* f, const float* x, const float* embed, float* zt, float* logdet, void* saved,
                           size_t saved_bytes, int32_t batch, void* stream) {
    int rc = train_call_checks(f, saved, saved_bytes, batch, "i2v_flow_train_forward");
    if (rc) return rc;
    I2V_REQUIRE(x && embed && zt && logdet, I2V_E_INVALID, "i2v_flow_train_forward: null tensor");
    I2V_REQUIRE_DEVICE(f->device, "i2v_flow_train_forward");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Entry sc;
    if ((rc = sc.serialise(f->order, s))) return rc;
    const TrainLayout L = make_layout(batch, f->H, f->depth, f->E, f->nfl);
    float* sv = static_cast<float*>(saved);
    const int H = f->H, depth = f->depth, B = batch;
    const dim3 lgrid((B + 3) / 4);
    for (int st = -1; st < f->S; ++st) {
        if (st >= 0) {
            const int kin = f->kin(st);
            for (int l = 0; l < depth + 2; ++l) {
                ChainArgs a{};
                for (int net = 0; net < 2; ++net) {
                    a.W[net] = f->L(st, net, l).W;
                    a.bias[net] = f->L(st, net, l).b;
                    a.X[net] = l == 0 ? sv + L.cin(st) : sv + L.act(st, net, l - 1);
                    a.Y[net] = l == depth + 1 ? sv + L.out(st, net) : sv + L.act(st, net, l);
                }
                a.M = l == depth + 1 ? 32 : H;
                a.R = l == 0 ? kin : H;
                a.ldw = a.R;
                a.ldx = l == 0 ? L.KP : H;
                a.ldy = a.M;
                a.B = B; a.nseg = 1; a.lrelu = l <= depth;
                launch_chain<0>(a, a.R % 16 == 0, 2, s);
            }
        }
        FwdArgs a{};
        a.L = L; a.saved = sv; a.x = x; a.embed = embed; a.zt = zt; a.logdet = logdet; a.st = st;
        a.use_act = f->cfg.activation;
        const bool block_end = st < 0 || (st & 1);
        if (st >= 0 && (st & 1)) a.shuf = f->shuf_f[st / 2];
        if (block_end && st + 1 < f->S && !f->cfg.skip_actnorm) {
            a.loc_next = f->an[(st + 1) / 2].loc;
            a.scale_next = f->an[(st + 1) / 2].scale;
        }
        a.cond_next = st + 1 < f->S ? f->step_cond[st + 1] : 0;
        hipLaunchKernelGGL(fwd_link, lgrid, dim3(256), 0, s, a);
    }
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_flow_train_backward(i2v_flow_train* f, const float* d_zt, const float* d_logdet, void* saved, size_t saved_bytes, float* d_x,
                            float* d_embed, void* grad_base, int32_t accumulate, int32_t batch, void* stream) {
    int rc = train_call_checks(f, saved, saved_bytes, batch, "i2v_flow_train_backward");
    if (rc) return rc;
    I2V_REQUIRE(d_zt && d_logdet, I2V_E_INVALID, "i2v_flow_train_backward: null output gradient");
    I2V_REQUIRE((reinterpret_cast<size_t>(grad_base) & 15) == 0, I2V_E_INVALID, "i2v_flow_train_backward: grad_base is not 16-byte aligned");
    I2V_REQUIRE_DEVICE(f->device, "i2v_flow_train_backward");
    hipStream_t s = static_cast<hipStream_t>(stream);
    Entry sc;
    if ((rc = sc.serialise(f->order, s))) return rc;
    const TrainLayout L = make_layout(batch, f->H, f->depth, f->E, f->nfl);
    float* sv = static_cast<float*>(saved);
    char* gbase = static_cast<char*>(grad_base);
    const int H = f->H, depth = f->depth, B = batch;
    const dim3 lgrid((B + 3) / 4);
    for (int st = f->S - 1; st >= -1; --st) {
        // link: finishes step st + 1, starts step st
        BwdArgs a{};
        a.L = L; a.saved = sv; a.d_zt = d_zt; a.d_logdet = d_logdet; a.d_x = d_x; a.d_embed = d_embed; a.st = st;
        a.first = st == f->S - 1;
        a.use_act = f->cfg.activation;
        a.cond1 = st + 1 < f->S ? f->step_cond[st + 1] : 0;
        if (!a.first && !((st + 1) & 1) && !f->cfg.skip_actnorm) a.scale = f->an[(st + 1) / 2].scale;
        if (st >= 0 && (st & 1)) a.bshuf = f->shuf_b[st / 2];
        hipLaunchKernelGGL(bwd_link, lgrid, dim3(256), 0, s, a);
        if (st < 0) break;
        // dX through the s- and t-net of step st, last layer first
        for (int l = depth + 1; l >= 1; --l) {
            ChainArgs g{};
            for (int net = 0; net < 2; ++net) {
                g.W[net] = f->L(st, net, l).W;
                g.X[net] = l == depth + 1 ? sv + L.dout(st, net) : sv + L.dpre(st, net, l);
                g.Y[net] = sv + L.dpre(st, net, l - 1);
                g.mask[net] = sv + L.act(st, net, l - 1);
            }
            g.M = H; g.R = l == depth + 1 ? 32 : H; g.ldw = H; g.ldx = g.R; g.ldy = H; g.B = B; g.nseg = 1;
            launch_chain<1>(g, true, 2, s);
        }
        ChainArgs g{};
        for (int net = 0; net < 2; ++net) {
            g.W[net] = f->L(st, net, 0).W;
            g.X[net] = sv + L.dpre(st, net, 0);
        }
        g.Y[0] = sv + L.o_dcin;
        g.M = f->kin(st); g.R = H; g.ldw = g.M; g.ldx = H; g.ldy = L.KP; g.B = B; g.nseg = 2;
        launch_chain<1>(g, true, 1, s);
    }
    // off the chain: every weight / bias gradient from the kept dY buffers, one owner per output tile
    const DwEntry* tab = f->dw_tab.as<DwEntry>();
    const int kmax = 32 + f->E;
    hipLaunchKernelGGL(dw_gemm, dim3((H + 63) / 64, (kmax + 63) / 64, f->n_l0), dim3(256), 0, s, tab, 0, L, sv, gbase, accumulate);
    hipLaunchKernelGGL(dw_gemm, dim3((H + 63) / 64, (H + 63) / 64, f->n_mid), dim3(256), 0, s, tab, f->n_l0, L, sv, gbase, accumulate);
    hipLaunchKernelGGL(dw_gemm, dim3(1, (H + 63) / 64, f->n_l3), dim3(256), 0, s, tab, f->n_l0 + f->n_mid, L, sv, gbase, accumulate);
    if (!f->cfg.skip_actnorm)
        hipLaunchKernelGGL(actnorm_grad, dim3(f->nfl), dim3(64), 0, s, f->an_tab.as<AnEntry>(), L, sv, d_logdet, gbase, accumulate);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int i2v_adam_step(const i2v_adam_tensor* table, const int32_t* chunks, int32_t n_chunks, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t amsgrad, int64_t step, void* stream) {
    I2V_REQUIRE(table && chunks && n_chunks > 0, I2V_E_INVALID, "i2v_adam_step: null table or no chunks");
    I2V_REQUIRE(step >= 1, I2V_E_INVALID, "i2v_adam_step: step %lld (the count AFTER this step, >= 1)", (long long)step);
    AdamScalars s{};
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step), bc2 = 1.0 - std::pow((double)beta2, (double)step);
    s.step_size = (float)((double)lr / bc1);
    s.bc2_sqrt = (float)std::sqrt(bc2);
    s.beta1 = beta1; s.beta2 = beta2; s.eps = eps; s.wd = weight_decay; s.amsgrad = amsgrad;
    hipLaunchKernelGGL(adam_kernel, dim3(n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), table, chunks, s);
    I2V_HIP_CHECK(hipGetLastError());
    return I2V_OK;
}

int32_t i2v_adam_chunk(void) { return ADAM_CHUNK; }

}  // extern "C"
