// General fp32-MFMA GEMM of the library (defined in gemm.hip, with its C entry points; include/dygnn.h states the same contract for dygnn_mm):
//   C = [relu] (alpha * op(A) . op(B) (+ bias[n]) (+ beta * C)), op(A)[m][k] = tA ? A[k*lda + m] : A[m*lda + k], op(B)[k][n] = tB ? B[n*ldb + k] : B[k*ldb + n]
// Large-K products (batch == 1, K >= 2048, no relu) are split over workgroups and summed with atomics into C: zeroed first (beta == 0, unless
// c_is_zero says it already is) or added onto the old C (beta == 1); any other beta on a split product is refused.
// `batch` products in one launch: batch index z = zb * H + zh adds zb*sXb + zh*sXh floats to the three base pointers.
// Refused with DYGNN_E_UNSUPPORTED before anything is launched: a split product with beta outside {0, 1}; colsum with !tA or batch > 1;
// rows with tA; rows on a call that does not take the LDS-DMA kernel.
#pragma once
#include "common.h"

namespace dygnn {
namespace train {
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
// What a product deviates in from the plain C = op(A) . op(B): a call names exactly that, e.g. MmOpt().bias(b).relu(), MmOpt().beta(1.f),
// MmOpt().batched(B * H, H).strideA(sAb, sAh).strideB(sBb, sBh).strideC(sCb, sCh), MmOpt().live_rows(nl).rows(table).
class MmOpt {
public:
    MmOpt& bias(const float* b) { bias_ = b; return *this; }
    MmOpt& alpha(float a) { alpha_ = a; return *this; }
    MmOpt& beta(float b) { beta_ = b; return *this; }
    MmOpt& relu(bool on = true) { relu_ = on; return *this; }
    MmOpt& batched(int batch, int H) { batch_ = batch; H_ = H; return *this; }      // z = zb * H + zh, zb < batch / H
    MmOpt& strideA(int64_t b, int64_t h) { sAb_ = b; sAh_ = h; return *this; }      // floats added to A per zb, per zh
    MmOpt& strideB(int64_t b, int64_t h) { sBb_ = b; sBh_ = h; return *this; }
    MmOpt& strideC(int64_t b, int64_t h) { sCb_ = b; sCh_ = h; return *this; }
    MmOpt& c_is_zero(bool on = true) { c_is_zero_ = on; return *this; }             // a split product with beta == 0 need not zero C first
    MmOpt& colsum(float* out) { colsum_out_ = out; return *this; }                  // tA and batch == 1 only (else refused): out[m] += sum_k op(A)[m][k] (accumulates: zero it first)
    MmOpt& live_rows(const int32_t* m_dev) { m_dev_ = m_dev; return *this; }        // device-side count of live rows (<= M): row tiles beyond it are skipped on the device
    MmOpt& a_kpad(bool on = true) { a_kpad_ = on; return *this; }                   // A [M][lda] has zeros behind its K columns up to a multiple of 4 (K itself need not be one)
    MmOpt& rows(const int32_t* a_rows) { a_rows_ = a_rows; return *this; }          // !tA only (else refused): row m of the product's A is A[a_rows[m]] (device table; the product gathers its rows: no staging copy)

private:
    const float* bias_ = nullptr;
    float alpha_ = 1.f, beta_ = 0.f;
    bool relu_ = false;
    int batch_ = 1, H_ = 1;
    int64_t sAb_ = 0, sAh_ = 0, sBb_ = 0, sBh_ = 0, sCb_ = 0, sCh_ = 0;
    bool c_is_zero_ = false;
    float* colsum_out_ = nullptr;
    const int32_t* m_dev_ = nullptr;
    bool a_kpad_ = false;
    const int32_t* a_rows_ = nullptr;
    friend int mm(hipStream_t, const float*, int, bool, const float*, int, bool, float*, int, int, int, int, const MmOpt&);
    friend int mm_plan(const float*, int, bool, const float*, int, bool, const float*, int, int, int, int, const MmOpt&, MmPlan*);
};
int mm(hipStream_t s, const float* A, int lda, bool tA, const float* B, int ldb, bool tB, float* C, int ldc, int M, int N, int K, const MmOpt& o = {});
// DYGNN_OK and *out, or the code mm() returns for these arguments (message in dygnn_last_error); an empty product plans nothing and is DYGNN_OK
int mm_plan(const float* A, int lda, bool tA, const float* B, int ldb, bool tB, const float* C, int ldc, int M, int N, int K, const MmOpt& o, MmPlan* out);
// Whether mm(s, A, lda, false, B, ldb, true, C, ldc, M, N, K, ...) takes the LDS-DMA kernel, the only one that accepts a row table
// (C's alignment is not a precondition).  DYGNN_MM_DMA=0 (read per call) makes it false.  Asks mm_plan.
bool mm_gathers_rows(const float* A, int lda, const float* B, int ldb, int M, int N, int K);
// out[n] += sum_m A[m][n] with one float atomic per column and 256-row chunk: always accumulates (zero `out` first), and the order of the
// additions is not fixed (colsum.h has the fixed-order column sum)
int colsum_atomic(hipStream_t s, const float* A, int lda, int64_t M, int N, float* out);
// Weight-gradient-shaped products in one grouped split-K launch (k_dw_grouped): C_p[m][n] += sum_k A_p[k][m] * B_p[k][n] for every problem p, all
// over the same K rows; colsum_p[m] += sum_k A_p[k][m] where given.  C and colsum ACCUMULATE (atomics): zero them first.  A, B 16-byte aligned,
// lda, ldb, N multiples of 4; M a multiple of 4 or lda >= round_up(M, 4).  Anything else is refused before the launch.
struct DwPair { const float* A; int lda, M; const float* B; int ldb, N; float* C; int ldc; float* colsum; };
int dw_grouped(hipStream_t s, int K, const DwPair* pairs, int npairs);
// The list of problems behind dw_grouped, for a caller that collects them over a whole pass and wants to know which ones were taken
// (dygnn_dygformer_backward sends a projection that try_add declines through mm instead).
struct DwProblem { const float* A; const float* B; float* C; float* colsum; int lda, ldb, ldc, M, N, ncw; };
constexpr int kDwMaxProblems = 4 * DYGNN_MAX_LAYERS + 4, kDwMaxItems = 32 * DYGNN_MAX_LAYERS + 16;
static_assert(kDwMaxProblems <= (1 << 20), "item code: problem index above bit 12");
struct DwArgs {
    DwProblem prob[kDwMaxProblems];
    unsigned int item[kDwMaxItems];        // problem << 12 | m-group << 6 | n-chunk (up to kDwMaxProblems = 36 problems: a 16-bit code held 16)
    int nitems, K, kchunk;
};
struct DwList {
    DwArgs args{};
    int nprob = 0;
    bool ok = true;
    void add(const float* A, int lda, int M, const float* B, int ldb, int N, float* C, int ldc, float* colsum) {
        if (!try_add(A, lda, M, B, ldb, N, C, ldc, colsum)) ok = false;
    }
    // M need not be a multiple of 4 when A's rows are padded to one (lda >= round_up(M, 4)): the float4 that holds the last columns then stays
    // inside the row, and outputs beyond M are never written
    bool try_add(const float* A, int lda, int M, const float* B, int ldb, int N, float* C, int ldc, float* colsum) {
        const bool aligned = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 && lda % 4 == 0 && ldb % 4 == 0 &&
                             (M % 4 == 0 || lda >= ((M + 3) & ~3)) && N % 4 == 0;
        const int nch = (N + 207) / 208, ncw = (((N + nch - 1) / nch) + 3) & ~3;
        const int mg = (M + 127) / 128;
        if (!aligned || nprob >= kDwMaxProblems || mg > 64 || nch > 64 || args.nitems + mg * nch > kDwMaxItems) return false;
        args.prob[nprob] = DwProblem{A, B, C, colsum, lda, ldb, ldc, M, N, ncw};
        for (int x = 0; x < mg; ++x)
            for (int y = 0; y < nch; ++y) args.item[args.nitems++] = (unsigned)nprob << 12 | (unsigned)x << 6 | (unsigned)y;
        ++nprob;
        return true;
    }
    int launch(hipStream_t s, int K);      // gemm.hip: it names the kernel
};
}  // namespace train
}  // namespace dygnn
