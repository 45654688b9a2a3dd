// Column sums in a fixed order, shared by every *_train.hip: out[c] += sum_r A[r][c].  Stage 1: one workgroup per 32 rows -> part[blk][c];
// stage 2: the partials in block order, with one thread per column (tgt::colsum, tgat_train.hip) or one wave per column (train::colsum,
// the other backbones); the two add the partials in different orders, so their bits differ.  (Deterministic: the time encoder's, the
// LayerNorm's and the bias gradients that go through here are the same bits run to run.)
#pragma once
#include "common.h"
#include "mfma_tile.h"

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

namespace train {

// Stage 2 with one WAVE per column: lane l adds the partials of blocks l, l + 64, ... in order, then the lanes meet in wave_sum's fixed
// butterfly (the same bits run to run).  tgt::k_tt_colsum_fin walks the partials with one thread per column: 57 us per call at TCL's 263
// row blocks, 76 calls per step.  Where the sum goes is the Out argument's business, so a caller passes no more than it needs:
//   ColOut   out[c] += s, and out2[c] += s if given (b_hh beside b_ih: the same sum);
//   ColSegs  column c belongs to the first segment whose end exceeds it and is ADDED to that tensor.
struct ColOut {
    float *out, *out2;
    __device__ __forceinline__ void add(int c, float s) const {
        if (out2) {                                                  // both loads before either store: the two tensors never overlap
            const float a = out[c], b = out2[c];
            out[c] = a + s;
            out2[c] = b + s;
        } else out[c] += s;
    }
};
struct ColSegs {
    float* out[6];
    int end[6];
    __device__ __forceinline__ void add(int c, float s) const {
        int k = 0;
        while (c >= end[k]) ++k;
        out[k][c - (k ? end[k - 1] : 0)] += s;
    }
};
template <class Out>
static __global__ __launch_bounds__(256) void k_colsum_fin(const float* __restrict__ part, int nblk, int cols, Out out) {
    const int lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= cols) return;                                           // wave-uniform
    float s = 0.f;
    for (int b = lane; b < nblk; b += 64) s += part[(size_t)b * cols + c];
    s = wave_sum(s);
    if (lane == 0) out.add(c, s);
}
// out (ColOut or ColSegs) += the column sums of A [rows][cols];  part: ceil(rows / kColRows) * cols floats of scratch
template <class Out>
static int colsum_launch(hipStream_t s, const float* A, int lda, int64_t rows, int cols, float* part, const Out& out) {
    if (rows <= 0) return DYGNN_OK;
    const int nblk = (int)ceil_div(rows, tgt::kColRows);
    hipLaunchKernelGGL(tgt::k_tt_colsum_part, dim3((unsigned)nblk), dim3(256), 0, s, A, lda, rows, cols, part);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_colsum_fin<Out>, dim3((unsigned)ceil_div(cols, 4)), dim3(256), 0, s, part, nblk, cols, out);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
// one tensor: out[c] += sum_r A[r][c], and out2[c] if given (a gradient struct's pointers are const: it is the weight struct)
static int colsum(hipStream_t s, const float* A, int lda, int64_t rows, int cols, float* part, const float* out, float* out2 = nullptr) {
    return colsum_launch(s, A, lda, rows, cols, part, ColOut{const_cast<float*>(out), out2});
}
static int colsum(hipStream_t s, const float* A, int lda, int64_t rows, int cols, float* part, const ColSegs& sg) {
    return colsum_launch(s, A, lda, rows, cols, part, sg);
}

}  // namespace train
}  // namespace dygnn
