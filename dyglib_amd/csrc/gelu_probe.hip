// Test-only export of the two GELU forms of the fused DyGFormer forward (fused3_device.h): the table form of the inference kernels — the table
// staged into LDS by the kernels' routine at the kernels' offset, read by the kernels' device function — and the erf form of the training
// kernels (tests/test_gelu_table_gpu.py compares both with float64).  No backbone calls this.
#include <vector>

#include "fused3_device.h"

namespace dygnn {
namespace {

constexpr int kProbeThreads = 512;      // eight waves, as the kernels that split the table's 32 pieces four to a wave
constexpr int kProbeLdsBytes = (v3::kLdsGelu + v3::kGeluTabFloats) * 4;

template <int FORM>
__global__ void __launch_bounds__(kProbeThreads) k_gelu_probe(const float* __restrict__ in, int64_t n, const float* __restrict__ gtab, float* __restrict__ out) {
    using namespace v3;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if constexpr (FORM == 0) {
        const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        stage_gelu_table(gtab + lane * 4, kLdsGelu, wave, kProbeThreads / 64);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    for (int64_t i = (int64_t)blockIdx.x * kProbeThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kProbeThreads) {
        if constexpr (FORM == 0) out[i] = gelu_table(in[i], lds + kLdsGelu);
        else out[i] = gelu_erf(in[i]);
    }
}

}  // namespace
}  // namespace dygnn

extern "C" int dygnn_gelu_table_host(float* out) {
    using namespace dygnn;
    DYGNN_REQUIRE(out, "gelu_table_host: null array");
    v3::gelu_table_fill(out);
    return DYGNN_OK;
}

extern "C" int dygnn_gelu_probe(const float* in, float* out, int64_t n, int32_t form, dygnn_stream_t stream) {
    using namespace dygnn;
    DYGNN_REQUIRE(form == 0 || form == 1, "gelu_probe: form %d is not 0 (table) or 1 (erf)", (int)form);
    DYGNN_REQUIRE(n >= 0 && n <= (int64_t(1) << 31), "gelu_probe: n out of range");
    if (n == 0) return DYGNN_OK;
    DYGNN_REQUIRE(in && out, "gelu_probe: null array");
    hipStream_t s = as_stream(stream);
    const int64_t want = ceil_div(n, kProbeThreads);
    const unsigned grid = (unsigned)(want < 1024 ? want : 1024);
    if (form == 1) {
        k_gelu_probe<1><<<dim3(grid), dim3(kProbeThreads), 0, s>>>(in, n, nullptr, out);
        DYGNN_LAUNCH_CHECK();
        DYGNN_HIP(hipStreamSynchronize(s));
        return DYGNN_OK;
    }
    std::vector<float> tab(v3::kGeluTabFloats);
    v3::gelu_table_fill(tab.data());
    float* dtab = nullptr;
    DYGNN_HIP(hipMalloc(&dtab, tab.size() * sizeof(float)));
    int rc = DYGNN_OK;
    if (hipMemcpy(dtab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_gelu_probe<0>), hipFuncAttributeMaxDynamicSharedMemorySize, kProbeLdsBytes) != hipSuccess) {
        set_error("gelu_probe: table upload failed");
        rc = DYGNN_E_HIP;
    } else {
        k_gelu_probe<0><<<dim3(grid), dim3(kProbeThreads), kProbeLdsBytes, s>>>(in, n, dtab, out);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) { set_error("gelu_probe: launch failed"); rc = DYGNN_E_HIP; }
    }
    (void)hipFree(dtab);
    return rc;
}
