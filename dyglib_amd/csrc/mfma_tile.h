// fp32 MFMA tile product of a four-wave workgroup, shared by graphmixer.hip and tcl.hip.  gfx950 only.
//
// v_mfma_f32_16x16x4_f32 in the transposed form of k_gemm_nt (tgat.hip): the weight rows are the A operand, so lane (c, g) of a tile ends up
// with out[m0 + c][n0 + 4g .. 4g + 3], one float4.  Both operands are K-contiguous: lane (c, g) reads the float4 at [row c][k0 + 4g] of each and
// feeds its four components to four MFMAs (the k order inside a block of 16 is permuted the same way on both sides).
#pragma once
#include "common.h"

namespace dygnn {
namespace tile {

using f4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f4 z4() { return f4{0.f, 0.f, 0.f, 0.f}; }
constexpr int kThreads = 256, kWaves = 4;

__host__ __device__ inline int round16(int x) { return (x + 15) & ~15; }

// acc[t][mt] += W[n0(t) + ., 0:Kdim] . A[16 mt + ., 0:Kdim]^T for the calling wave's column tiles n0(t) = 16 (wave + 4 t), t < NT.
// A: LDS rows of stride lda, zero beyond Kdim up to round16(Kdim).  W: global [N][ldw] (16-byte aligned rows), read at columns wk0 + k.
template <int NT, int MT>
__device__ __forceinline__ void wave_product(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw, int wk0, int N, int Kdim,
                                             int wave, int lane, f4 (&acc)[NT][MT]) {
    const int c = lane & 15, g = lane >> 4;
    for (int k0 = 0; k0 < Kdim; k0 += 16) {
        const int k = k0 + 4 * g;
        f4 a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f4*>(A + (size_t)(16 * mt + c) * lda + k);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n0 = 16 * (wave + kWaves * t);
            if (n0 >= N) continue;                                   // wave-uniform
            const int n = n0 + c;
            const f4 w = (n < N && k < Kdim) ? *reinterpret_cast<const f4*>(W + (size_t)n * ldw + wk0 + k) : z4();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[t][mt] = mfma4(w.x, a[mt].x, acc[t][mt]);
                acc[t][mt] = mfma4(w.y, a[mt].y, acc[t][mt]);
                acc[t][mt] = mfma4(w.z, a[mt].z, acc[t][mt]);
                acc[t][mt] = mfma4(w.w, a[mt].w, acc[t][mt]);
            }
        }
    }
}

// raise a kernel's dynamic LDS limit when it needs more than the default 64 KiB
template <typename Kern>
static int lds_limit(Kern kernel, size_t bytes) {
    if (bytes > 64 * 1024) DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return DYGNN_OK;
}

}  // namespace tile
}  // namespace dygnn
