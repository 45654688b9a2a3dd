// What DyGFormer's two product-by-product paths (dygformer_generic.hip, inference; dygformer_train.hip, unfused training) compute alike, written
// once: a pair's windows and co-occurrence counts, the time and co-occurrence patch values, and the LayerNorm row.  The fused kernel
// builds its windows in a layout of its own (fused3_forward.h).
#pragma once
#include "common.h"

namespace dygnn {
namespace rows {

struct Csr { const int32_t* nbr; const int32_t* eid; const double* ts; int64_t num_nodes; };

// The windows of pair b in LDS, positions [0, Ss) = source side, [Ss, Ss + Sd) = destination side, left aligned, position 0 of a side = the
// queried node (pad_sequences, DyGFormer.py:228-245), and each position's appearance counts on the two sides (count_nodes_appearances,
// :337-393; the padding node counts as 0).  A query id outside [0, num_nodes) is the padding node (never a fault).  hist_len / end_pos:
// window_lengths_device's, queries [src of the B pairs | dst].  The whole workgroup calls; the arrays are complete when it returns.
__device__ __forceinline__ void fill_windows(const Csr& g, const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const double* __restrict__ times,
                                             const int32_t* __restrict__ hist_len, const int64_t* __restrict__ end_pos, int64_t B, int64_t b, int Ss, int Sd,
                                             int L, int32_t* ids, int32_t* eids, float* dts, int32_t* c0, int32_t* c1) {
    const int S = Ss + Sd;
    const double t = times[b];
    for (int p = threadIdx.x; p < S; p += blockDim.x) {
        const bool is_dst = p >= Ss;
        const int j = is_dst ? p - Ss : p;
        const int64_t q = is_dst ? B + b : b;
        const int32_t len = hist_len[q];
        const int32_t m = len < L - 1 ? len : L - 1;
        int32_t id = 0, e = 0;
        float tn = 0.f;
        if (j == 0) {
            const int64_t qid = is_dst ? dst[b] : src[b];
            id = qid < 0 || qid >= g.num_nodes ? 0 : (int32_t)qid;
            tn = (float)t;
        } else if (j <= m) {
            const int64_t pos = end_pos[q] - m + (j - 1);
            id = g.nbr[pos]; e = g.eid[pos]; tn = (float)g.ts[pos];
        }
        ids[p] = id; eids[p] = e;
        dts[p] = (float)(t - (double)tn);                       // DyGFormer.py:263: f64 - f32 -> f64 -> .float()
    }
    __syncthreads();
    for (int p = threadIdx.x; p < S; p += blockDim.x) {
        const int32_t v = ids[p];
        int32_t cs = 0, cdn = 0;
        for (int q = 0; q < Ss; ++q) cs += (ids[q] == v);
        for (int q = Ss; q < S; ++q) cdn += (ids[q] == v);
        if (v == 0) { cs = 0; cdn = 0; }
        c0[p] = cs; c1[p] = cdn;
    }
    __syncthreads();
}

// time feature f of a position: cos(w dt + b), zero at the padding node (modules.py:37, DyGFormer.py:263-266)
__device__ __forceinline__ float time_feature(int32_t id, float dt, const float* __restrict__ tw, const float* __restrict__ tb, int f) {
    return id == 0 ? 0.f : cosf(fmaf(dt, tw[f], tb[f]));
}
// co-occurrence feature f of a position with counts (c0, c1): lut[c0] + lut[c1] (DyGFormer.py:409-411)
__device__ __forceinline__ float cooc_feature(const float* __restrict__ lut, int C, int32_t c0, int32_t c1, int f) {
    return lut[(size_t)c0 * C + f] + lut[(size_t)c1 * C + f];
}

// y = LayerNorm(x) of one row of D columns by one wave (eps 1e-5, biased variance, plain multiply-add form; DyGFormer.py:438-439)
__device__ __forceinline__ void layernorm_row(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta, int D, int lane,
                                              float* __restrict__ y, float& mean, float& rstd) {
    float s = 0.f;
    for (int k = lane; k < D; k += kWave) s += x[k];
    mean = wave_sum(s) / (float)D;
    float v = 0.f;
    for (int k = lane; k < D; k += kWave) { const float d = x[k] - mean; v = fmaf(d, d, v); }
    rstd = 1.0f / sqrtf(wave_sum(v) / (float)D + 1e-5f);
    for (int k = lane; k < D; k += kWave) y[k] = (x[k] - mean) * rstd * gamma[k] + beta[k];
}

}  // namespace rows
}  // namespace dygnn
