// cos (and, for the backward, sin) of the time encoder's argument w * dt + b, shared by every backbone.  gfx950 only.
//
// The argument reaches 2.7e6 rad, where libm's cosf takes its slow Payne-Hanek path; here x / (2 pi) is formed as a two-float product
// (kInvHi + kInvLo = 1 / (2 pi) to 2^-52), its fractional part u in [0, 0.5] is folded to [0, 0.25] and cos(2 pi u) evaluated by an even
// degree-12 minimax polynomial (|err| <= 6e-8 on the folded range); beyond 3e7 the product's rounding error would exceed 1e-7 turns and
// libm is called instead (tests/test_dygformer_gpu.py::test_large_timestamps_take_the_libm_cosine_path).
// Every form below is exported alone by time_encoding_probe.hip and held to these figures by tests/test_time_encoding_gpu.py (|err| <= 7.5e-7
// = 2 pi 1e-7 + 6e-8 + 2^-24 against float64; observed 3.6e-7 for cos, 5.0e-7 for sin, whose quarter-turn shift rounds once more); every
// backbone runs with arguments in (2.7e6, 3e7] and beyond 3e7 in tests/test_large_timestamps_gpu.py.
//
// There are TWO guarded cosines on purpose, same values, different code around the rare libm call:
//   * cos_time: an early return into the out-of-line cos_libm.  libm's slow path needs scratch; kept behind a call it costs the caller
//     nothing but the call's clobbers, and callers place it where nothing live has to be spilled around it (tgat_attn.h, phase A).
//     Every backbone except the fused DyGFormer kernels uses this form.
//   * cos_time_select: fast and libm value chosen by a select, cosf inlined.  The fused DyGFormer kernels reach it only from a branch of
//     their own that tests four arguments at once (fused3_forward.h: t_finish) and keep this form.
// sin_time (the time encoder's gradient, dygformer_train.hip: k_time_bwd) guards with an early return into sinf.
//
// NOT here, deliberately: sites that call cosf / sinf directly.  They compute other bits than the forms below and stay as they are:
//   * the dt = 0 encodings (cosf(b)) in tgat.hip, tgat_chain.hip and tgat_train.hip;
//   * the message rows in tgn.hip and memory_rnn.hip;
//   * dygformer_generic.hip;
//   * k_embed_inputs in dygformer_train.hip;
//   * train_rows.h: k_time_part;
//   * the backward of tgat_train.hip (sinf).
#pragma once
#include "common.h"

namespace dygnn {
namespace timeenc {

constexpr float kInvHi = 0.15915493667125702f, kInvLo = 6.4206382432985265e-09f;      // 1 / (2 pi), two floats
constexpr float kFastMax = 3.0e7f;                                                     // |x| beyond which the guarded forms call libm
// cos(2 pi v) = 1 + kC2 z + kC4 z^2 + ... + kC12 z^6, z = v^2, v in [0, 0.25]
constexpr float kC12 = 7.903536371318467f, kC10 = -26.42625678337438f, kC8 = 60.24464137187666f, kC6 = -85.45681720669373f, kC4 = 64.93939402266829f,
                kC2 = -19.739208802178716f;

// x / (2 pi) minus the nearest integer, in [-0.5, 0.5] (a rounding error's width beyond): the turns fraction
__device__ __forceinline__ float turns_fraction(float x) {
    const float p = x * kInvHi;
    const float e = fmaf(x, kInvHi, -p);
    const float q = fmaf(x, kInvLo, e);
    return (p - rintf(p)) + q;
}
// cos(2 pi u) for u in [0, 0.5]: folded to [0, 0.25], the polynomial, the sign
__device__ __forceinline__ float cos_folded(float u) {
    const bool flip = u > 0.25f;
    const float v = flip ? 0.5f - u : u;
    const float z = v * v;
    float r = fmaf(kC12, z, kC10);
    r = fmaf(r, z, kC8);
    r = fmaf(r, z, kC6);
    r = fmaf(r, z, kC4);
    r = fmaf(r, z, kC2);
    r = fmaf(r, z, 1.0f);
    return flip ? -r : r;
}
__device__ __forceinline__ float cos_fast(float x) {      // |x| <= kFastMax (branch-free; the guarded forms check)
    float u = fabsf(turns_fraction(x));
    u = u > 0.5f ? 1.0f - u : u;
    return cos_folded(u);
}
__device__ __forceinline__ float sin_fast(float x) {      // |x| <= kFastMax: sin(2 pi t) = cos(2 pi (t - 1/4)), the same reduction a quarter turn on
    float t = turns_fraction(x) - 0.25f;
    t -= rintf(t);
    return cos_folded(fabsf(t));
}
// cos_fast on two arguments at once, written on 2-vectors so that hipcc emits packed fp32 instructions (v_pk_mul / v_pk_fma /
// v_pk_add_f32: two results in ~1.6 issue slots, tools/coissue_ubench.hip; VALU instructions take matrix-pipe time in the fused kernel)
using f2 = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 cos_fast2(f2 x) {
    const f2 INV_HI = {kInvHi, kInvHi}, INV_LO = {kInvLo, kInvLo};
    const f2 p = x * INV_HI;
    const f2 e = pk_fma(x, INV_HI, -p);
    const f2 q = pk_fma(x, INV_LO, e);
    const f2 rp = {rintf(p.x), rintf(p.y)};
    const f2 t = (p - rp) + q;
    f2 u = {fabsf(t.x), fabsf(t.y)};
    const f2 one_u = f2{1.0f, 1.0f} - u;
    u = f2{u.x > 0.5f ? one_u.x : u.x, u.y > 0.5f ? one_u.y : u.y};
    const bool fx = u.x > 0.25f, fy = u.y > 0.25f;
    const f2 half_u = f2{0.5f, 0.5f} - u;
    const f2 v = {fx ? half_u.x : u.x, fy ? half_u.y : u.y};
    const f2 z = v * v;
    auto c2 = [](float c) { return f2{c, c}; };
    f2 r = pk_fma(c2(kC12), z, c2(kC10));
    r = pk_fma(r, z, c2(kC8));
    r = pk_fma(r, z, c2(kC6));
    r = pk_fma(r, z, c2(kC4));
    r = pk_fma(r, z, c2(kC2));
    r = pk_fma(r, z, c2(1.0f));
    return f2{fx ? -r.x : r.x, fy ? -r.y : r.y};
}

// the guarded forms (see the top of the file)
__device__ __attribute__((noinline)) float cos_libm(float x) { return cosf(x); }
__device__ __forceinline__ float cos_time(float x) {
    if (!(fabsf(x) <= kFastMax)) return cos_libm(x);
    return cos_fast(x);
}
__device__ __forceinline__ float cos_time_select(float x) { return fabsf(x) <= kFastMax ? cos_fast(x) : cosf(x); }
__device__ __forceinline__ float sin_time(float x) {
    if (!(fabsf(x) <= kFastMax)) return sinf(x);
    return sin_fast(x);
}

}  // namespace timeenc
}  // namespace dygnn
