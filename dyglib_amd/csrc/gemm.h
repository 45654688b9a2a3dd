// General fp32-MFMA GEMM of the library (defined in dygformer_train.hip; include/dygnn.h states the same contract for dygnn_mm):
//   C = [relu] (alpha * op(A) . op(B) (+ bias[n]) (+ beta * C)), op(A)[m][k] = tA ? A[k*lda + m] : A[m*lda + k], op(B)[k][n] = tB ? B[n*ldb + k] : B[k*ldb + n]
// Large-K products (batch == 1, K >= 2048, no relu) are split over workgroups and summed with atomics into C: zeroed first (beta == 0, unless
// c_is_zero says it already is) or added onto the old C (beta == 1); any other beta on a split product is refused.
// `batch` products in one launch: batch index z = zb * H + zh adds zb*sXb + zh*sXh floats to the three base pointers.
// Refused with DYGNN_E_UNSUPPORTED before anything is launched: a split product with beta outside {0, 1}; colsum_out with !tA or batch > 1;
// a_rows with tA; a_rows on a call that does not take the LDS-DMA kernel.
#pragma once
#include "common.h"

namespace dygnn {
namespace train {
int mm(hipStream_t s, const float* A, int lda, bool tA, const float* B, int ldb, bool tB, float* C, int ldc, int M, int N, int K,
       const float* bias = nullptr, float alpha = 1.f, float beta = 0.f, int batch = 1, int H = 1, int64_t sAb = 0, int64_t sAh = 0,
       int64_t sBb = 0, int64_t sBh = 0, int64_t sCb = 0, int64_t sCh = 0, bool relu = false, bool c_is_zero = false,
       float* colsum_out = nullptr,       // tA and batch == 1 only (else refused): colsum_out[m] += sum_k op(A)[m][k] (accumulates: zero it first)
       const int32_t* m_dev = nullptr,    // device-side count of live rows (<= M): row tiles beyond it are skipped on the device
       bool a_kpad = false,               // A [M][lda] has zeros behind its K columns up to a multiple of 4 (K itself need not be one)
       const int32_t* a_rows = nullptr);  // !tA only (else refused): row m of the product's A is A[a_rows[m]] (device table; the product gathers its rows: no staging copy)
// What mm() does with a set of arguments, decided on the host from sizes, strides and pointer alignment alone (no pointer is followed, nothing
// is launched).  mm() runs exactly this plan; dygnn_mm_path reports it.
enum { kMmSmall = 0, kMmBig = 1, kMmDma = 2 };      // k_mm, k_mm_big, k_mm_dma
struct MmPlan {
    int kernel;            // kMmSmall / kMmBig / kMmDma
    int ksplit, kchunk;    // K parts (1 = not split) of kchunk columns each
    int f4_epilogue;       // k_mm_dma leaves through LDS as float4 rows (aligned C, one part, beta == 0)
    int colsum_route;      // 0 none, 1 rides along in the 64-row-tile kernel, 2 the stand-alone reduction
    int vecA, vecB, vecC;  // operand / result rows may move as aligned float4
};
// DYGNN_OK and *out, or the code mm() returns for these arguments (message in dygnn_last_error); an empty product plans nothing and is DYGNN_OK
int mm_plan(const float* A, int lda, bool tA, const float* B, int ldb, bool tB, const float* C, int ldc, int M, int N, int K, float beta, int batch, int64_t sAb,
            int64_t sAh, int64_t sBb, int64_t sBh, int64_t sCb, int64_t sCh, bool relu, bool has_colsum, bool a_kpad, bool has_rows, MmPlan* out);
// Whether mm(s, A, lda, false, B, ldb, true, C, ldc, M, N, K, ...) takes the LDS-DMA kernel, the only one that accepts a row table `a_rows`
// (C's alignment is not a precondition).  DYGNN_MM_DMA=0 (read per call) makes it false.  Asks mm_plan.
bool mm_gathers_rows(const float* A, int lda, const float* B, int ldb, int M, int N, int K);
// Weight-gradient-shaped products in one grouped split-K launch (k_dw_grouped): C_p[m][n] += sum_k A_p[k][m] * B_p[k][n] for every problem p, all
// over the same K rows; colsum_p[m] += sum_k A_p[k][m] where given.  C and colsum ACCUMULATE (atomics): zero them first.  A, B 16-byte aligned,
// lda, ldb, N multiples of 4; M a multiple of 4 or lda >= round_up(M, 4).  Anything else is refused before the launch.
struct DwPair { const float* A; int lda, M; const float* B; int ldb, N; float* C; int ldc; float* colsum; };
int dw_grouped(hipStream_t s, int K, const DwPair* pairs, int npairs);
}  // namespace train
}  // namespace dygnn
