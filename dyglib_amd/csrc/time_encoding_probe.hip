// Test-only export of the cosine forms of time_encoding.h: one thread per element, float32 in, float32 out, one kernel instance per form so
// that every form is compiled as a caller of its own (tests/test_time_encoding_gpu.py compares them with float64).  No backbone calls this.
#include "time_encoding.h"

namespace dygnn {
namespace {

template <int FORM>
__global__ void __launch_bounds__(256) k_timeenc_probe(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float r;
    if constexpr (FORM == 0) r = timeenc::cos_fast(x[i]);
    else if constexpr (FORM == 1) {      // the pair (x[2j], x[2j + 1]) that holds element i; an odd n's last element is paired with 0
        const int64_t j = i & ~int64_t(1);
        const timeenc::f2 c = timeenc::cos_fast2(timeenc::f2{x[j], j + 1 < n ? x[j + 1] : 0.0f});
        r = (i & 1) ? c.y : c.x;
    } else if constexpr (FORM == 2) r = timeenc::cos_time(x[i]);
    else if constexpr (FORM == 3) r = timeenc::cos_time_select(x[i]);
    else if constexpr (FORM == 4) r = timeenc::sin_fast(x[i]);
    else r = timeenc::sin_time(x[i]);
    out[i] = r;
}

template <int FORM>
void launch(const float* x, int64_t n, float* out, hipStream_t s) {
    k_timeenc_probe<FORM><<<dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s>>>(x, n, out);
}

}  // namespace
}  // namespace dygnn

extern "C" int dygnn_timeenc_probe(int32_t form, const float* x, int64_t n, float* out, dygnn_stream_t stream) {
    using namespace dygnn;
    DYGNN_REQUIRE(form >= 0 && form <= 5, "timeenc_probe: form %d is not one of 0..5", (int)form);
    DYGNN_REQUIRE(n >= 0 && n <= (int64_t(1) << 31), "timeenc_probe: n out of range");
    if (n == 0) return DYGNN_OK;
    DYGNN_REQUIRE(x && out, "timeenc_probe: null array");
    hipStream_t s = as_stream(stream);
    switch (form) {
        case 0: launch<0>(x, n, out, s); break;
        case 1: launch<1>(x, n, out, s); break;
        case 2: launch<2>(x, n, out, s); break;
        case 3: launch<3>(x, n, out, s); break;
        case 4: launch<4>(x, n, out, s); break;
        default: launch<5>(x, n, out, s); break;
    }
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
