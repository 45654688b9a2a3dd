// Shared helpers for libdygnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/dygnn.h"

namespace dygnn {

void set_error(const char* fmt, ...);

inline hipStream_t as_stream(dygnn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

constexpr int kWave = 64;   // CDNA4 wavefront

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Carving a workspace into consecutive blocks: take(bytes) = the byte offset of the next block, every block 256-byte aligned; o = the total
struct Carve {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t r = o; o += (bytes + 255) & ~size_t(255); return r; }
};

// Sum / maximum over the 64 lanes of a wave, in every lane: the xor butterfly 32, 16, .. 1, so the order of the additions (and with it the
// bits) is fixed.  T = float, double or unsigned long long.  All 64 lanes must call.
__device__ __forceinline__ float larger(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double larger(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ unsigned long long larger(unsigned long long a, unsigned long long b) { return b > a ? b : a; }
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = larger(v, __shfl_xor(v, o, kWave));
    return v;
}

// First index p in [lo, hi) with ts[p] >= t, or hi (np.searchsorted side='left' on an ascending CSR row).  A 64-ary search: every step the
// wave probes 64 evenly spaced timestamps and one ballot+popcount picks the sub-range.  All 64 lanes must call (uniform lo/hi/t).
__device__ __forceinline__ int64_t wave_lower_bound(const double* __restrict__ ts, int64_t lo, int64_t hi, double t, int lane) {
    while (hi - lo > kWave) {
        const int64_t step = (hi - lo + kWave - 1) / kWave;
        const int64_t p = lo + (int64_t)lane * step;
        const bool pred = (p < hi) && (ts[p] < t);
        const int c = __popcll(__ballot(pred));      // rows ascend => pred is true exactly for lanes < c
        if (c == 0) return lo;
        const int64_t nlo = lo + (int64_t)(c - 1) * step + 1;
        const int64_t nhi = lo + (int64_t)c * step;
        hi = nhi < hi ? nhi : hi;
        lo = nlo;
    }
    const int64_t p = lo + lane;
    const bool pred = (p < hi) && (ts[p] < t);
    return lo + __popcll(__ballot(pred));
}

}  // namespace dygnn

#define DYGNN_REQUIRE(cond, ...)                                  \
    do {                                                          \
        if (!(cond)) {                                            \
            dygnn::set_error(__VA_ARGS__);                        \
            return DYGNN_E_INVALID;                               \
        }                                                         \
    } while (0)

#define DYGNN_HIP(expr)                                                                        \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            dygnn::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return DYGNN_E_HIP;                                                                \
        }                                                                                      \
    } while (0)

#define DYGNN_LAUNCH_CHECK() DYGNN_HIP(hipGetLastError())
