// Row-wise kernels of the training paths, shared by tcl_train.hip, cawn_train.hip and tgat_train.hip: residual + dropout + LayerNorm and
// its backward (one wave per row), the site-2 dropout of the hidden rows and the hidden gradient's mask, and the time encoder's fp64
// two-stage gradient sums.  Dropout masks come from train::Drop (dropout.h) and are redrawn, never stored.
#pragma once
#include "colsum.h"
#include "common.h"
#include "dropout.h"
#include "mfma_tile.h"

namespace dygnn {
namespace train {

constexpr float kLnEps = 1e-5f;

// TCL's rows are [2 B sides][S] with the sides [src ; dst]; the dropout generator counts side s as pair sequence 2 p + side
__device__ __forceinline__ int64_t pair_seq(int64_t s, int64_t B) { return s < B ? 2 * s : 2 * (s - B) + 1; }

// The dropout generator's row of token row r.  B = 0: r itself.  B > 0 (TCL): row (s, i) draws as row (pair_seq(s, B), i).
struct RowMap {
    int S;
    int64_t B;
    __device__ __forceinline__ uint64_t row(int64_t r) const {
        if (B == 0) return (uint64_t)r;
        const int64_t s = r / S;
        return (uint64_t)(pair_seq(s, B) * S + (r - s * S));
    }
};

// ---- residual + dropout + LayerNorm, one wave per row, NV columns per lane (d <= 64 NV; the iterations beyond d add nothing, so the bits do
// not depend on NV): pre = res + t * mask(site, map.row(r) d + c); y = LN(pre) ---------------------------------------------------------------
template <int NV>
static __global__ __launch_bounds__(256) void k_res_ln(const float* __restrict__ t, const float* __restrict__ res, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int64_t R, int d, RowMap map, Drop dr, uint32_t site,
                                                         float* __restrict__ pre, float* __restrict__ mean_o, float* __restrict__ rstd_o, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const uint64_t e0 = map.row(r) * d;
    const uint32_t skey = dr.site_key(site);
    float x[NV];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        x[u] = 0.f;
        if (f < d) {
            const uint64_t idx = e0 + f;
            x[u] = res[r * d + f] + t[r * d + f] * dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
            pre[r * d + f] = x[u];
            sum += x[u];
        }
    }
    const float mean = wave_sum(sum) / (float)d;
    float var = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + 64 * u < d) { const float c = x[u] - mean; var = fmaf(c, c, var); }
    const float rstd = 1.0f / sqrtf(wave_sum(var) / (float)d + kLnEps);
    if (lane == 0) { mean_o[r] = mean; rstd_o[r] = rstd; }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        if (f < d) y[r * d + f] = fmaf((x[u] - mean) * rstd, gamma[f], beta[f]);
    }
}

// LayerNorm backward, one wave per row: g = dy gamma, dpre = rstd (g - mean(g) - xhat mean(g xhat)).  dpre reaches the residual (dres) and,
// through the redrawn mask, the dropped-out term (dt); dyx = dy xhat feeds the gamma gradient.
template <int NV>
static __global__ __launch_bounds__(256) void k_res_ln_bwd(const float* __restrict__ dy, const float* __restrict__ pre, const float* __restrict__ mean_in,
                                                             const float* __restrict__ rstd_in, const float* __restrict__ gamma, int64_t R, int d, RowMap map,
                                                             Drop dr, uint32_t site, float* __restrict__ dres, float* __restrict__ dt,
                                                             float* __restrict__ dyx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const uint64_t e0 = map.row(r) * d;
    const uint32_t skey = dr.site_key(site);
    const float mean = mean_in[r], rstd = rstd_in[r];
    float xh[NV], g[NV];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        xh[u] = g[u] = 0.f;
        if (f < d) {
            xh[u] = (pre[r * d + f] - mean) * rstd;
            const float v = dy[r * d + f];
            g[u] = v * gamma[f];
            dyx[r * d + f] = v * xh[u];
            sg += g[u];
            sgx = fmaf(g[u], xh[u], sgx);
        }
    }
    sg = wave_sum(sg) / (float)d;
    sgx = wave_sum(sgx) / (float)d;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        if (f < d) {
            const uint64_t idx = e0 + f;
            const float v = rstd * (g[u] - sg - xh[u] * sgx);
            dres[r * d + f] = v;
            dt[r * d + f] = v * dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
        }
    }
}

// site 2: hid [count / W][W] *= mask(site, map.row(r) W + c), one thread per element
static __global__ void k_row_drop(float* __restrict__ hid, int64_t count, int W, RowMap map, Drop dr, uint32_t site) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    uint64_t idx = (uint64_t)e;
    if (map.B) {
        const int64_t r = e / W;
        idx = map.row(r) * W + (uint64_t)(e - r * W);
    }
    hid[e] *= dr.mask(site, idx);
}
// the hidden gradient through dropout and ReLU: the stored rows are positive exactly where the ReLU was open AND the element was kept
static __global__ void k_hid_bwd(float* __restrict__ g, const float* __restrict__ hid, int64_t count, float keep_scale) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) g[e] = hid[e] > 0.f ? g[e] * keep_scale : 0.f;
}

// Time encoder gradients: dw = sum_r -sin(pre) dt g, db = sum_r -sin(pre) g with the forward's pre = fma(dt, w, b), as fixed-order column sums
// (colsum.h's two stages: 32 rows per workgroup, then the partials in block order).  dt reaches 10^6 and the terms cancel, so the terms and
// both stages are fp64 (the reference's autograd sums this product in fp64 too: its time encoder input is a double).
// part: [blocks][2][Ft] doubles.
static __global__ __launch_bounds__(256) void k_time_part(const float* __restrict__ g, const float* __restrict__ DT, const float* __restrict__ tw,
                                                            const float* __restrict__ tb, int64_t R, int Ft, double* __restrict__ part) {
    const int64_t r0 = (int64_t)blockIdx.x * tgt::kColRows, r1 = r0 + tgt::kColRows < R ? r0 + tgt::kColRows : R;
    for (int f = threadIdx.x; f < Ft; f += blockDim.x) {
        const float w = tw[f], b = tb[f];
        double sw = 0.0, sb = 0.0;
        for (int64_t r = r0; r < r1; ++r) {
            const float dt = DT[r];
            const double t = (double)(-sinf(fmaf(dt, w, b))) * (double)g[r * Ft + f];
            sb += t;
            sw += t * (double)dt;
        }
        part[((size_t)blockIdx.x * 2) * Ft + f] = sw;
        part[((size_t)blockIdx.x * 2 + 1) * Ft + f] = sb;
    }
}
static __global__ __launch_bounds__(256) void k_time_fin(const double* __restrict__ part, int nblk, int Ft, float* __restrict__ gw, float* __restrict__ gb) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= Ft) return;
    double sw = 0.0, sb = 0.0;
    for (int b = 0; b < nblk; ++b) {
        sw += part[((size_t)b * 2) * Ft + f];
        sb += part[((size_t)b * 2 + 1) * Ft + f];
    }
    gw[f] += (float)sw;
    gb[f] += (float)sb;
}
// gw[f] += sum_r -sin(pre) dt g, gb[f] += sum_r -sin(pre) g over the R rows of g [R][Ft];  part: ceil(R / kColRows) * 2 * Ft doubles
static int time_grad(hipStream_t s, const float* g, const float* DT, const float* tw, const float* tb, int64_t R, int Ft, double* part, float* gw, float* gb) {
    const int nblk = (int)ceil_div(R, tgt::kColRows);
    hipLaunchKernelGGL(k_time_part, dim3((unsigned)nblk), dim3(256), 0, s, g, DT, tw, tb, R, Ft, part);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_time_fin, dim3((unsigned)ceil_div(Ft, 256)), dim3(256), 0, s, part, nblk, Ft, gw, gb);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace train
}  // namespace dygnn
