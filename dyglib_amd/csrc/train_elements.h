// Element kernels of the training paths whose dense activations number their dropout elements by offset, shared by dygformer_train.hip
// (DyGFormer.py:456-460) and graphmixer_train.hip (the channel half): GELU and dropout, dropout and residual, and their gradients, one
// thread per element.  Dropout masks come from train::Drop (dropout.h) and are redrawn, never stored.  The kernels are static like
// train_rows.h's, which every source that includes them compiles a copy of: hence a header of their own, included where they are launched.
#pragma once
#include "dropout.h"
#include "gelu_exact.h"

namespace dygnn {
namespace train {

// out = gelu(pre) * mask
static __global__ void k_gelu_drop(const float* __restrict__ pre, int64_t count, Drop dr, uint32_t site, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) out[e] = gelu_exact(pre[e]) * dr.mask(site, (uint64_t)e);
}
// g = g * mask * gelu'(pre), in place
static __global__ void k_gelu_drop_bwd(float* __restrict__ g, const float* __restrict__ pre, int64_t count, Drop dr, uint32_t site) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) g[e] = g[e] * dr.mask(site, (uint64_t)e) * gelu_exact_grad(pre[e]);
}
// out = x + y * mask
static __global__ void k_drop_add(const float* __restrict__ x, const float* __restrict__ y, int64_t count, Drop dr, uint32_t site, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) out[e] = x[e] + y[e] * dr.mask(site, (uint64_t)e);
}
// out = g * mask
static __global__ void k_drop_bwd(const float* __restrict__ g, int64_t count, Drop dr, uint32_t site, float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) out[e] = g[e] * dr.mask(site, (uint64_t)e);
}

}  // namespace train
}  // namespace dygnn
