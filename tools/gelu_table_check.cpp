// Stand-alone host check of gelu_table_fill (csrc/gelu_table.h), for AddressSanitizer / UndefinedBehaviorSanitizer builds: no HIP, no GPU.
//     clang++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I dyglib_amd/csrc tools/gelu_table_check.cpp -o gelu_table_check
// Fills a heap buffer of exactly the table's size (a write past either end is a sanitizer report), checks the properties the kernels lean
// on, and evaluates the table form on the host by the device function's arithmetic at the arguments where an index could leave the table.
// Exit status 0 and one line "gelu_table_check ok ..." on success (tests/test_gelu_table_cpu.py builds and runs it).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "gelu_table.h"

using namespace dygnn::v3;

// gelu_table of fused3_device.h on the host: fma, clamp (a NaN takes the lower bound), truncation, fraction, fma, product
static float gelu_table_host(float v, const std::vector<float>& tab) {
    float t = std::fmaf(v, kGeluInvH, kGeluMid);
    t = !(t > 0.0f) ? 0.0f : (t > kGeluTMax ? kGeluTMax : t);
    const int i = (int)t;
    const float f = t - (float)i;
    return v * std::fmaf(f, tab.at(2 * i + 1), tab.at(2 * i));
}

int main() {
    std::vector<float> tab(kGeluTabFloats);
    gelu_table_fill(tab.data());
    int bad = 0;
    auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAILED: %s\n", what); ++bad; } };
    expect(tab[0] == 0.0f && !std::signbit(tab[0]), "cell 0 starts at exactly +0");
    expect(tab[2 * (kGeluCells - 1)] + tab[2 * (kGeluCells - 1) + 1] == 1.0f, "the last cell ends at exactly 1");
    for (int i = 0; i < kGeluCells; ++i) {
        expect(tab[2 * i + 1] >= 0.0f, "steps are not negative");
        if (i + 1 < kGeluCells) expect(tab[2 * i] + tab[2 * i + 1] == tab[2 * i + 2], "a cell ends where the next one starts");
    }
    const float inf = std::numeric_limits<float>::infinity();
    expect(gelu_table_host(1e30f, tab) == 1e30f, "gelu(1e30) = 1e30");
    const float m = gelu_table_host(-1e30f, tab);
    expect(m == 0.0f && std::signbit(m), "gelu(-1e30) = -0");
    expect(gelu_table_host(inf, tab) == inf, "gelu(inf) = inf");
    expect(std::isnan(gelu_table_host(-inf, tab)), "gelu(-inf) is NaN, as 0.5 v (1 + erf) gives");
    expect(std::isnan(gelu_table_host(std::numeric_limits<float>::quiet_NaN(), tab)), "gelu(NaN) is NaN");
    expect(gelu_table_host(6.0f, tab) == 6.0f && gelu_table_host(std::nextafter(6.0f, 7.0f), tab) == std::nextafter(6.0f, 7.0f), "Phi = 1 at and above +6");
    expect(gelu_table_host(-6.0f, tab) == 0.0f && gelu_table_host(std::nextafter(-6.0f, -7.0f), tab) == 0.0f, "Phi = 0 at and below -6");
    double worst = 0.0;
    for (int k = -80000; k <= 80000; ++k) {
        const float v = (float)k * 1e-4f;
        const double ex = 0.5 * (double)v * (1.0 + std::erf((double)v * 0.70710678118654752440));
        const double e = std::fabs((double)gelu_table_host(v, tab) - ex);
        if (e > worst) worst = e;
    }
    expect(worst < 6e-7, "max |gelu - exact| on [-8, 8] in steps of 1e-4 stays below 6e-7");
    if (bad) return 1;
    std::printf("gelu_table_check ok: %d cells, max |gelu - exact| %.3e\n", kGeluCells, worst);
    return 0;
}
