// The FFN's GELU of the fused DyGFormer inference kernels as a table: gelu(v) = v Phi(v), Phi by linear interpolation in kGeluCells cells
// over [-6, 6], one (Phi(x_i), Phi(x_{i+1}) - Phi(x_i)) float pair per cell, 32 KB, read from LDS (fused3_device.h: gelu_table).  The point is
// the pipe, not the polynomial: on gfx950 a VALU instruction takes matrix-pipe time and an LDS read does not, and the table
// form has no transcendental.  This header is the host side and compiles without HIP (tools/gelu_table_check.cpp runs it under sanitizers).
#pragma once
#include <cmath>
#include <cstdint>

namespace dygnn {
namespace v3 {

constexpr int kGeluCells = 4096;                 // 2048 cells: max |gelu - exact| 1.41e-6, 4096: 4.8e-7, 8192: 4.7e-7 (A&S 7.1.26 form: 4.7e-7)
constexpr int kGeluTabFloats = 2 * kGeluCells;
constexpr float kGeluLo = -6.0f;
constexpr float kGeluInvH = kGeluCells / 12.0f;  // cells per unit of v
constexpr float kGeluMid = kGeluCells / 2.0f;    // cell coordinate of v = 0
constexpr float kGeluTMax = 4095.999755859375f;  // the largest float below kGeluCells: the cell coordinate is clamped to [0, kGeluTMax]
static_assert(kGeluCells == 4096, "kGeluTMax is written for 4096 cells");

// out[2 i] = Phi(x_i), out[2 i + 1] = Phi(x_{i+1}) - Phi(x_i), x_i = -6 + 12 i / kGeluCells.  Phi in float64 (std::erf), every knot rounded to
// fp32 once; the step is the difference of the two ROUNDED knots — exact in fp32 (neighbours differ by < 2^-9 and are multiples of one
// ulp) — so the interpolant is continuous across cell edges.  Cell 0's base is exactly 0: Phi = 0 at and below -6, so a hidden activation of
// -1e30 gives -0 and not -1e21.  The knots from 5.42 on round to exactly 1.0f: Phi = 1 at and above +6.
inline void gelu_table_fill(float* out) {
    auto knot = [](int i) -> float {
        if (i <= 0) return 0.0f;
        const double x = -6.0 + 12.0 * (double)i / (double)kGeluCells;
        return (float)(0.5 * (1.0 + std::erf(x * 0.70710678118654752440)));
    };
    float lo = knot(0);
    for (int i = 0; i < kGeluCells; ++i) {
        const float hi = knot(i + 1);
        out[2 * i] = lo;
        out[2 * i + 1] = hi - lo;
        lo = hi;
    }
}

}  // namespace v3
}  // namespace dygnn
