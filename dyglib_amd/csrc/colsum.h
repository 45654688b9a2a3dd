// Column sums in a fixed order, shared by tgat_train.hip and tcl_train.hip: out[c] += sum_r A[r][c].  Stage 1: one workgroup per 32 rows ->
// part[blk][c]; stage 2: the partials in block order.  (Deterministic: the time encoder's, the LayerNorm's and the bias gradients that go
// through here are the same bits run to run.)
#pragma once
#include "common.h"

namespace dygnn {
namespace tgt {

constexpr int kColRows = 32;
static __global__ __launch_bounds__(256) void k_tt_colsum_part(const float* __restrict__ A, int lda, int64_t rows, int cols, float* __restrict__ part) {
    const int64_t r0 = (int64_t)blockIdx.x * kColRows, r1 = r0 + kColRows < rows ? r0 + kColRows : rows;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        float s = 0.f;
        for (int64_t r = r0; r < r1; ++r) s += A[r * lda + c];
        part[(size_t)blockIdx.x * cols + c] = s;
    }
}
static __global__ __launch_bounds__(256) void k_tt_colsum_fin(const float* __restrict__ part, int nblk, int cols, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * cols + c];
    out[c] += s;
}

// part: ceil(rows / kColRows) * cols floats of scratch
static int colsum(hipStream_t s, const float* A, int lda, int64_t rows, int cols, float* part, float* out) {
    if (rows <= 0) return DYGNN_OK;
    const int nblk = (int)ceil_div(rows, kColRows);
    hipLaunchKernelGGL(k_tt_colsum_part, dim3((unsigned)nblk), dim3(256), 0, s, A, lda, rows, cols, part);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tt_colsum_fin, dim3((unsigned)ceil_div(cols, 256)), dim3(256), 0, s, part, nblk, cols, out);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace tgt
}  // namespace dygnn
