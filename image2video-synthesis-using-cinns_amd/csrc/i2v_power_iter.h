// Spectral norm's power iteration (torch.nn.utils.spectral_norm, one iteration) over the convs of one network, in three launches; shared
// by the two discriminators (i2v_patchdisc.hip, i2v_disc3d.hip).  Float64 sums with one owner and a fixed order.  Included into the
// anonymous namespace of its users.
#pragma once
#include "i2v_handle.h"

namespace i2v {
namespace {

constexpr int PD_MAXCONV = 8;   // convs per launch; a network with more calls launch_power_iteration once per group

// sum of `v` over the 256 threads of the workgroup in a fixed tree; every thread gets the result.  `red`: 256 doubles.
__device__ __forceinline__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

struct PdPiConv {
    const float* w;   // [rows][cols]
    float *u, *v;     // in place
    float *sigma, *usnap, *vsnap;   // this call's values (usnap / vsnap may be null)
    double *t, *s;    // W^T u [cols], W v [rows]
    int rows, cols, bfirst, rfirst;   // bfirst: first workgroup of pd_pi_wtu_kernel (64 columns each); rfirst: first row
};
struct PdPiArgs { PdPiConv c[PD_MAXCONV]; int nconv, btotal, rtotal, iterate; };

// t = W^T u: a workgroup owns 64 columns, its four waves a quarter of the rows each, summed in wave order
__global__ __launch_bounds__(256) void pd_pi_wtu_kernel(PdPiArgs a) {
    __shared__ double red[3][64];
    const int bid = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ci = 0;
    while (ci + 1 < a.nconv && bid >= a.c[ci + 1].bfirst) ++ci;
    const PdPiConv& c = a.c[ci];
    const int k = (bid - c.bfirst) * 64 + lane;
    const int rq = (c.rows + 3) / 4, r0 = wave * rq, r1 = r0 + rq < c.rows ? r0 + rq : c.rows;
    double acc = 0.0;
    if (k < c.cols)
        for (int r = r0; r < r1; ++r) acc += (double)c.w[(long)r * c.cols + k] * (double)c.u[r];
    if (wave > 0) red[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && k < c.cols) c.t[k] = ((acc + red[0][lane]) + red[1][lane]) + red[2][lane];
}

__global__ __launch_bounds__(256) void pd_pi_wv_kernel(PdPiArgs a) {
    __shared__ double red[256];
    const int bid = blockIdx.x, tid = threadIdx.x;
    int ci = 0;
    while (ci + 1 < a.nconv && bid >= a.c[ci + 1].rfirst) ++ci;
    const PdPiConv& c = a.c[ci];
    const int r = bid - c.rfirst;
    double inv = 1.0;
    if (a.iterate) {
        double q = 0.0;
        for (int k = tid; k < c.cols; k += 256) q += c.t[k] * c.t[k];
        inv = 1.0 / fmax(sqrt(block_sum(q, red)), 1e-12);
    }
    double acc = 0.0;
    for (int k = tid; k < c.cols; k += 256) {
        const float vk = a.iterate ? (float)(c.t[k] * inv) : c.v[k];
        if (r == 0) {
            if (a.iterate) c.v[k] = vk;
            if (c.vsnap) c.vsnap[k] = vk;
        }
        acc += (double)c.w[(long)r * c.cols + k] * (double)vk;
    }
    const double s = block_sum(acc, red);
    if (tid == 0) c.s[r] = s;
}

__global__ __launch_bounds__(256) void pd_pi_sigma_kernel(PdPiArgs a) {
    __shared__ double red[256];
    const PdPiConv& c = a.c[blockIdx.x];
    const int tid = threadIdx.x;
    double inv = 1.0;
    if (a.iterate) {
        double q = 0.0;
        for (int r = tid; r < c.rows; r += 256) q += c.s[r] * c.s[r];
        inv = 1.0 / fmax(sqrt(block_sum(q, red)), 1e-12);
    }
    double acc = 0.0;
    for (int r = tid; r < c.rows; r += 256) {
        const float ur = a.iterate ? (float)(c.s[r] * inv) : c.u[r];
        if (a.iterate) c.u[r] = ur;
        if (c.usnap) c.usnap[r] = ur;
        acc += (double)ur * c.s[r];
    }
    const double sg = block_sum(acc, red);
    if (tid == 0) *c.sigma = (float)sg;
}

#define I2V_LAUNCHED() I2V_HIP_CHECK(hipGetLastError())

// the three launches of the spectral norm over the convs of `a` (all of them in one go)
int launch_power_iteration(const PdPiArgs& a, hipStream_t st) {
    if (a.iterate) {
        hipLaunchKernelGGL(pd_pi_wtu_kernel, dim3(a.btotal), dim3(256), 0, st, a);
        I2V_LAUNCHED();
    }
    hipLaunchKernelGGL(pd_pi_wv_kernel, dim3(a.rtotal), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    hipLaunchKernelGGL(pd_pi_sigma_kernel, dim3(a.nconv), dim3(256), 0, st, a);
    I2V_LAUNCHED();
    return I2V_OK;
}

}  // namespace
}  // namespace i2v
