// The exact (erf) GELU of nn.GELU() / F.gelu and its derivative, as every product-by-product path evaluates them: graphmixer.hip,
// graphmixer_train.hip, dygformer_train.hip and dygformer_generic.hip's k_gemm<GELU>.  The fused DyGFormer kernels have forms of their own
// with other bits (fused3_device.h's erf_as, gelu_table.h).
#pragma once
#include <hip/hip_runtime.h>

namespace dygnn {

__device__ __forceinline__ float gelu_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// d gelu(x) / dx = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_exact_grad(float x) {
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * (0.39894228040143267794f * expf(-0.5f * x * x));
}

}  // namespace dygnn
