// Fused DyGFormer forward for gfx950, "token-owner" layout (models/DyGFormer.py:68-194 end to end).
//
// One workgroup = 8 wave64 = 128 tokens: two (src,dst,t) pairs of <= 64 tokens (TPW = 4 token tiles per pair) or one
// pair of <= 128 tokens (TPW = 8; BASELINE config 4, L=512 / P=8).  Wave w owns 16 tokens x ALL 200 channels:
//   * the residual stream X^T (13 accumulator tiles = 52 VGPRs) never leaves the wave's registers;
//   * LayerNorm is wave-local (register sums + two cross-lane adds) and its output IS the MFMA B operand of the
//     QKV / FFN products — no LDS round trip, no partial-sum exchange between waves, no K-split;
//   * Q^T, softmax(S)^T, O^T and gelu(H)^T feed the next product straight from accumulators (same layout trick
//     an accumulator tile is the B operand of the product that sums over its rows).
// Only K and V of ONE head at a time live in LDS ([128 tokens][100], 2 x 51.2 KB); heads run back to back.
//
// LDS map (float offsets into the one dynamic array, 160 KB):
//   kLdsK     0 .. 12799      K of one head [128][100]     | prologue: window arrays, projection slab | pooled layer: gpool [8][2][800]
//   kLdsV 12800 .. 25599      V of one head [128][100]     | prologue: the same                       | epilogue: pool [8][2][208], mean, mean_g
//     kLdsGelu 16128 .. 24319   inference, FFN phases only: the GELU table [4096][2] (gelu_table.h), staged by LDS-DMA once per FFN phase over
//                               V rows 33 .. 115 (dead from the last out-projection of a layer to the next layer's first K/V stores); it lies
//                               behind pool and over mean / mean_g, which are written after the FFN loop and its barrier
//   25600 .. 25615            slack (tile 6 of the last K/V row reads 12 floats past it)
//   kLdsRing 25616 .. 38927   weight ring, 52 fragments of 1 KiB
//   kLdsMisc 38928 ..         FFN hidden bias [2][800], time-encoder w | b
//
// Weights: all 8 waves consume the SAME fragments in the SAME order, so the whole model is ONE linear stream of
// 1-KiB MFMA-A fragments per kernel, brought on chip once per workgroup by LDS-DMA (global_load_lds, no VGPRs)
// into a 52-fragment LDS ring and read with ds_read_b128.  (Measured in tools/v3_ubench.hip: weight fragments
// loaded global->VGPR per wave hold the MFMA pipe at 66 %, LDS-DMA staged at 85 %, registers only 90 %.)
// The ring protocol: stages of 13 fragments; after the step that finishes a stage every wave waits for its own
// DMAs, passes one barrier, and issues its share of the stage four ahead.  Steps never straddle the ring end
// (the packer inserts pad fragments with the same rule the consumer applies).
//
// This header holds what the forward kernel (fused3_forward.h) and the backward kernels (dygformer_fused3_bwd.hip) share: the constants,
// the MFMA / LDS-DMA primitives, the weight stream and the products that more than one kernel runs.
#pragma once
#include "dygformer_layout.h"
#include "fused3_plan.h"
#include "gelu_table.h"
#include "time_encoding.h"

// The K = 200 products (QKV, FFN W1) spend 2 instead of 4 MFMAs on their last k-chunk (192..207: only 8 real k: mma_group2 / kpack), the
// head-dim contractions (Q K^T, out-projection) 1 instead of 4 on theirs (96..111: only 4 real k: mma_group1 / kpack4); the packer lays the
// A fragments of those chunks out to match (FragDesc.kmode).
// Measured and NOT kept (round 2, profiles/r02_fused3_ab.md): a software-pipelined FFN (stream order W1(p+1) before W2(p), GELU of step p
// issued inside the W1(p+1) block — in chunks between MFMA groups, or whole before / after the block's MFMAs with the two waves of a SIMD at
// opposite ends): 1.3-1.6 % SLOWER in every arrangement, the two waves of a SIMD already run the block one after the other (the older or
// prioritised wave takes nearly every matrix-pipe slot), so one GELU of the two is hidden as it is; a static s_setprio 1 for waves 4-7: +-0.2 %;
// stage barriers every 13 instead of 26 fragments in the FFN with the next group's fragments read before the barrier: slower (twice the barriers).
// Measured and NOT kept (round 3, tools/ab_fused3.py, 32 steps per launch; the build-time arms are gone, DESIGN §4.3 names the last commit that had
// them): the FFN's W1 blocks (or W1 and W2 blocks) starting on fragments read across the stage barrier in front of them: -0.3 % (-2.7 %: 16 more
// live VGPRs spill).

namespace dygnn {
namespace v3 {

using f4 = __attribute__((ext_vector_type(4))) float;
using i4 = __attribute__((ext_vector_type(4))) int;

constexpr int kD = 200, kDP = 208, kNT = 13, kKC = 13, kHD = 100, kHid = 800, kC = 50;
constexpr int kFrag = 256;            // floats per 16x16 fragment
constexpr int kPoolRow = kHid + kDP;  // deferred pooled epilogue: one (pair, side) row = 800 means of gelu(h) | 208 means of the residual
constexpr int kRing = 52;             // LDS ring, fragments
// kStage = 26 (two stages of 26 fragments: half the stage barriers) measured +1.25 % at L = 64, +0.8 % at L = 512 (round 3, tools/ab_fused3.py) and
// NOT kept: with two stages the fragments a step reads ahead ACROSS the barrier that ends a stage belong to a stage whose DMAs that very
// barrier publishes (with four stages the barrier one stage earlier did) — a read-ahead that is legal only with three stages in flight;
// re-reading after the barrier costs what the halved barriers save.
constexpr int kStage = 13;            // DMA / barrier granularity, fragments: the ring holds kRing / kStage stages
constexpr int kNStage = kRing / kStage;
static_assert(kStage * kNStage == kRing && kNStage >= 2, "the ring is a whole number (>= 2) of stages");
constexpr int kTokWG = 128;           // tokens per workgroup
constexpr int kKV = 100;              // K/V row stride (floats): 4*25 -> conflict-free b128 row reads and b32 column reads
constexpr int kLdsK = 0;
constexpr int kLdsV = kTokWG * kKV;                 // 12800
constexpr int kLdsRing = 2 * kTokWG * kKV + 16;     // 16 floats of slack: tile 6 of the last row reads 12 floats past it
constexpr int kLdsMisc = kLdsRing + kRing * kFrag;  // 38928 floats = 155,712 B
constexpr int kMiscB1 = 0;            // [2][800]: FFN hidden bias, double-buffered by layer parity (no barrier needed:
                                      // dozens of stream barriers lie between a buffer's write and its reads / reuse)
constexpr int kMiscFloats = 2 * kHid;               // 1600
constexpr int kLdsBytes = 160 * 1024;
static_assert((kLdsMisc + kMiscFloats) * 4 <= kLdsBytes, "LDS budget");
constexpr int kScratchFloats = 2 * kTokWG * kKV;    // prologue window arrays live in the K/V region

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
template <int N>
__device__ __forceinline__ void mma_group(f4* acc, const f4* a, const f4 b) {
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].x, b.x, acc[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].y, b.y, acc[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].z, b.z, acc[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].w, b.w, acc[u]);
}
// last k-chunk of a K = 200 product: k = 192..199 packed into TWO MFMAs (b0: k = 192 + {0,4,1,5}[g], b1: k = 192 + {2,6,3,7}[g]);
// the A fragments of that chunk are packed to match (FragDesc.kmode 1)
template <int N>
__device__ __forceinline__ void mma_group2(f4* acc, const f4* a, const float b0, const float b1) {
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].x, b0, acc[u]);
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].y, b1, acc[u]);
}
// v = rows 192 + 4g + r of an accumulator-layout tile (g >= 2: zero padding).  v_permlane32_swap moves lanes 0..31 of the second
// operand into lanes 32..63 of the first: (x, y) -> lanes g = 0,1,2,3 hold rows 192, 196, 193, 197; (z, w) -> 194, 198, 195, 199
__device__ __forceinline__ void kpack(const f4 v, float& b0, float& b1) {
    // (scalars first: __builtin_bit_cast applied to a vector ELEMENT expression reads element 0 whatever the element — hipcc, ROCm 7.2)
    const float vx = v.x, vy = v.y, vz = v.z, vw = v.w;
    const auto r0 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, vx), __builtin_bit_cast(unsigned, vy), false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, vz), __builtin_bit_cast(unsigned, vw), false, false);
    b0 = __builtin_bit_cast(float, r0[0]);
    b1 = __builtin_bit_cast(float, r1[0]);
}
// v = rows 96 + 4 g + r of a head-dim tile: only rows 96 .. 99 (lane group 0) are real (head dim 100).  Returns the B operand of ONE
// MFMA that carries all four: lane group g holds row 96 + g (permlane16_swap: 16-lane rows 1, 3 of the first operand <-> rows 0, 2 of the
// second; then permlane32_swap as in kpack).  The A fragments of that k-chunk are packed to match (FragDesc.kmode 2: k = 96 + g).
__device__ __forceinline__ float kpack4(const f4 v) {
    const float vx = v.x, vy = v.y, vz = v.z, vw = v.w;
    const auto t1 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, vx), __builtin_bit_cast(unsigned, vy), false, false);
    const auto t2 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, vz), __builtin_bit_cast(unsigned, vw), false, false);
    const auto r = __builtin_amdgcn_permlane32_swap(t1[0], t2[0], false, false);
    return __builtin_bit_cast(float, r[0]);
}
template <int N>
__device__ __forceinline__ void mma_group1(f4* acc, const f4* a, const float b0) {
#pragma unroll
    for (int u = 0; u < N; ++u) acc[u] = mfma(a[u].x, b0, acc[u]);
}
__device__ __forceinline__ f4 ldg4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ f4 lds4(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ f4 zero4() { return f4{0.f, 0.f, 0.f, 0.f}; }
// One LDS-DMA piece: 64 lanes x 16 B from per-lane global addresses to LDS [dst, dst + 1 KiB), no VGPR destination.
// Written as inline asm on purpose.  With the builtin (__builtin_amdgcn_global_load_lds) hipcc (ROCm 7.2) knows an LDS-DMA is in flight
// and from then on waits `s_waitcnt lgkmcnt(0)` — not a counted lgkmcnt(N) — before the MFMAs that consume ds_read results: every other
// MFMA group of every weight loop then stalls for the LDS round trip of the fragments it has just PREFETCHED for the next group (this
// kernel keeps a DMA in flight all the time).  The asm form is invisible to that bookkeeping; the protocol needs nothing from it: every
// wave drains its own DMAs with an explicit `s_waitcnt vmcnt(0)` in front of the stage barrier (WStream::advance).
// The destination is given as a FLOAT OFFSET into the kernel's one dynamic LDS array (which starts at __builtin_amdgcn_groupstaticsize():
// the kernel has no static LDS), not as a pointer: an addrspacecast of a generic pointer in this position trips an instruction verifier error.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // "clobber list contains reserved registers: m0", once per inlined copy: m0 IS written here
__device__ __forceinline__ void dma_frag(const float* gsrc_lane, int lds_float_off_uniform) {
    const unsigned m0v = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_groupstaticsize() + 4u * (unsigned)lds_float_off_uniform);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc_lane), "s"(m0v) : "memory", "m0");
}
#pragma clang diagnostic pop

// sum over the 16 lanes of a DPP row (= the 16 tokens of a tile, lane & 15), result in every lane: four VALU adds with
// DPP operands (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror) instead of four LDS bpermutes
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_sum16(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}
// An empty asm keeps a value scalar where hipcc would pair it with a neighbour into a v_pk_* instruction (gelu_table_finish)
__device__ __forceinline__ float keep_scalar(float v) { asm("" : "+v"(v)); return v; }
// The per-side pooling sums (pool_sides, and gelu(h) in the pooled layer) as a REDUCE-SCATTER: eight values per lane (two accumulator tiles,
// or one tile of either side) are summed over the 16 tokens of the row, and every partial sum is computed once instead of in all sixteen
// lanes.  Lane bits 3 and 2 are folded by v_add_f32_dpp with a bank mask — the enabled banks take value + rotated value, the disabled
// ones keep what the register held, so one instruction per input register halves the registers: 8 -> 4 (row_ror:8: banks 0, 1 keep the
// first tile, banks 2, 3 the second), 4 -> 2 (row_ror:12 / row_ror:4: even banks keep registers 0, 1, odd banks registers 2, 3; lane c
// reads lane c - n mod 16).  Bits 1 and 0 are two quad_perm adds on the two registers that remain.  16 VALU instructions for eight
// sums, where eight row_sum16 take 32.  Afterwards every lane of bank b = (lane & 15) >> 2 holds in result j the sum of input
// pool_sum_input(j, b) (fused3_plan.h); one lane per bank stores its two adjacent words.
// Every value takes the same tree whatever register or bank it ends in — ((c + c^8) + (c^4 + c^12)) per lane, then the quad's lanes ^1, ^2
// — and a float add commutes, so a row's bits depend on its sixteen tokens alone.
// Inline asm: __builtin_amdgcn_update_dpp with a bank mask comes out as a move and an add.  The hazard "VALU write of a VGPR, then a DPP
// read of it: 2 wait states" is the asm's own business (hipcc does not look inside): the leading s_nop covers the inputs, the instruction
// order and the two s_nop 0 cover the chain, and nothing after the last add reads with DPP.  The outputs are early-clobber: an input
// must not share a register with one of them, equal value or not.
__device__ __forceinline__ timeenc::f2 row_sums8(const f4 a, const f4 b) {
    float v0 = a.x, v1 = a.y, v2 = a.z, v3 = a.w;
    const float v4 = b.x, v5 = b.y, v6 = b.z, v7 = b.w;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %2, %2, %2 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %3, %3, %3 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %4, %4 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %1, %5, %5 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %2, %6, %6 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %3, %7, %7 row_ror:8 row_mask:0xf bank_mask:0xc\n\t"
        "v_add_f32_dpp %0, %0, %0 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %1, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "v_add_f32_dpp %1, %3, %3 row_ror:4 row_mask:0xf bank_mask:0xa\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 0\n\t"
        "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %1, %1, %1 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf"
        : "+&v"(v0), "+&v"(v1), "+&v"(v2), "+&v"(v3)
        : "v"(v4), "v"(v5), "v"(v6), "v"(v7));
    return timeenc::f2{v0, v1};
}

// The time encoder's cosine is time_encoding.h; the fused kernels take the select form of its guard.
using timeenc::f2;
using timeenc::pk_fma;
// erf for the exact GELU: Abramowitz & Stegun 7.1.26 (|err| <= 1.5e-7), branch-free.
__device__ __forceinline__ float erf_as(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = __expf(-ax * ax);
    return copysignf(fmaf(-p * t, e, 1.0f), x);
}
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erf_as(v * 0.70710678118654752440f)); }

// ---- the inference kernels' GELU: v Phi(v), Phi interpolated in the LDS table of gelu_table.h.  Seven VALU instructions and one
// ds_read_b64 per element (fma, v_med3, v_cvt_i32, v_fract, v_lshl_add, fma, mul), no transcendental; the training kernels keep gelu_erf,
// whose derivative the backward takes from hpre.  v <= -6 reads cell 0 at fraction 0: Phi = 0 and the result is -0 (or NaN for -inf, as
// 0.5 v (1 + erf) gives); v >= 6 reads the last cell, whose knots are 1.0f; a NaN clamps or converts to a cell inside the table and
// leaves through the final product.
constexpr int kLdsGelu = kLdsV + 8 * 2 * kDP;       // behind pool_sides' [8 waves][2 sides][208] in the V region, which is dead during every FFN phase
static_assert(kLdsGelu + kGeluTabFloats <= kLdsRing, "the GELU table ends inside the V region");
static_assert((kLdsGelu * 4) % 16 == 0 && kGeluTabFloats % kFrag == 0, "the table is staged in whole, 16-byte aligned LDS-DMA pieces");
static_assert(kLdsGelu * 4 < 65536, "the table's base fits the offset field of ds_read_b64");
// In two halves, so that a caller with several elements issues all their reads before it consumes the first (gelu_table_n): cell -> the
// cell's (base, step) read is issued, the position inside the cell comes back in `frac`; finish -> v Phi.
__device__ __forceinline__ f2 gelu_table_cell(float v, const float* tab, float& frac) {
    float t = fmaf(v, kGeluInvH, kGeluMid);
    t = __builtin_amdgcn_fmed3f(t, 0.0f, kGeluTMax);
    const int i = (int)t;
    frac = __builtin_amdgcn_fractf(t);
    return *reinterpret_cast<const f2*>(tab + 2 * i);
}
// (the empty asm keeps Phi scalar: paired into v_pk_fma_f32 / v_pk_mul_f32 the two halves of every ds_read_b64 result are first moved into
//  pairs of their own — three v_mov_b32 per two elements, five instructions where the scalar form has four)
__device__ __forceinline__ float gelu_table_finish(float v, float frac, const f2 e) { return v * keep_scalar(fmaf(frac, e.y, e.x)); }
template <int N>
__device__ __forceinline__ void gelu_table_n(float (&v)[N], const float* tab) {
    f2 e[N];
    float fr[N];
#pragma unroll
    for (int k = 0; k < N; ++k) e[k] = gelu_table_cell(v[k], tab, fr[k]);
    __builtin_amdgcn_sched_barrier(0);           // N reads in flight, one LDS round trip (left alone hipcc consumes them two by two)
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = gelu_table_finish(v[k], fr[k], e[k]);
}
__device__ __forceinline__ float gelu_table(float v, const float* tab) {
    float w[1] = {v};
    gelu_table_n<1>(w, tab);
    return w[0];
}
// The table into LDS at float offset lds_off: kGeluTabFloats / kFrag = 32 pieces of 1 KiB split over the workgroup's nw waves.  The caller
// waits for its own pieces (s_waitcnt vmcnt(0)) and passes a barrier before anyone reads the table.
// gtab_lane = table + lane * 4 (per lane).
__device__ __forceinline__ void stage_gelu_table(const float* gtab_lane, int lds_off, int wave, int nw) {
    for (int j = wave; j < kGeluTabFloats / kFrag; j += nw) dma_frag(gtab_lane + j * kFrag, lds_off + j * kFrag);
}

// load / LDS-DMA source for rows that do not exist (static: one copy per translation unit, the build has no relocatable device code)
[[maybe_unused]] static __device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};

// ---- the shared weight stream ---------------------------------------------------------------------------------
struct WStream {
    const float* gsrc;    // stream base + lane*4 (per lane)
    int ring;             // LDS ring: float offset into the dynamic LDS array (wave-uniform)
    int wave, nstages;
    int nw;               // waves of the workgroup (8; 4 in the one-pair-per-workgroup kernels for small batches): they split a stage's 13 fragments
    int pos;              // ring slot of the next fragment
    int instage;          // fragments consumed of the current stage
    int issued;           // stages whose DMA this wave has issued
    __device__ __forceinline__ void issue(int s) {
        if (s < nstages) {
            const float* srcp = gsrc + (size_t)s * (kStage * kFrag);
            const int dst = ring + (s % kNStage) * (kStage * kFrag);
#pragma unroll
            for (int u = 0; u < (kStage + 3) / 4; ++u) {      // nw >= 4 waves split the stage's fragments
                const int f = wave + u * nw;
                if (f < kStage) dma_frag(srcp + f * kFrag, dst + f * kFrag);
            }
        }
    }
    __device__ __forceinline__ void open(const float* stream, int ring_, int lane, int wave_, int nstages_, int nw_ = 8) {
        gsrc = stream + lane * 4; ring = ring_; wave = wave_; nstages = nstages_; nw = nw_;
        pos = 0; instage = 0; issued = kNStage;
#pragma unroll
        for (int s = 0; s < kNStage; ++s) issue(s);
    }
    // n fragments consumed (or skipped).  Crossing a stage boundary: wait for own DMAs, barrier (every wave is done with
    // the finished stage, every stage issued before is now visible), then refill the freed ring quarter.
    // younger_stores (training forward): this wave has issued exactly that many global stores since its last DMA issue.  vmcnt retires in
    // issue order, so waiting until only those are outstanding proves the (older) DMAs landed without exposing the stores' latency.
    __device__ __forceinline__ void advance(int n, int younger_stores = 0) {
        pos += n;
        if (pos >= kRing) pos -= kRing;
        instage += n;
        if (instage >= kStage) {
            if (younger_stores == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (younger_stores == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's LDS-DMA has landed before anyone passes the barrier
            __syncthreads();
            do { instage -= kStage; issue(issued); ++issued; } while (instage >= kStage);
        }
    }
    __device__ __forceinline__ void fit(int n) { if (pos + n > kRing) advance(kRing - pos); }
    __device__ __forceinline__ void align26() {
        if (pos != 0 && pos != 26) advance(pos < 26 ? 26 - pos : kRing - pos);
    }
    // ring slot of the step after one of n fragments that starts at `pos` (same rule as advance + fit)
    __device__ __forceinline__ int next_pos(int n, int n_next) const {
        int p = pos + n;
        if (p >= kRing) p -= kRing;
        if (p + n_next > kRing) p = 0;
        return p;
    }
};

// Diagnostic build (-DDYGNN_STAMPS): every wave accumulates s_memtime ticks per phase category and the last four
// workgroups of the grid store them: taps.phase_cycles[wg][wave][cat]; cat 31 = total.
#ifdef DYGNN_STAMPS
#define TDECL unsigned long long tacc_[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long tk_ = __builtin_amdgcn_s_memtime(); const unsigned long long tk0_ = tk_
#define TACC(i) do { __builtin_amdgcn_sched_barrier(0); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); tacc_[i] += t_ - tk_; tk_ = t_; __builtin_amdgcn_sched_barrier(0); } while (0)
#define TSTORE()                                                                                   \
    do {                                                                                           \
        if (a.stamps != nullptr && lane == 0 && blockIdx.x + 4 >= gridDim.x) {                     \
            unsigned long long* o_ = a.stamps + ((size_t)(blockIdx.x + 4 - gridDim.x) * 8 + wave) * 32;   \
            for (int i_ = 0; i_ < 24; ++i_) o_[i_] = tacc_[i_];                                    \
            o_[31] = tk_ - tk0_;                                                                   \
        }                                                                                          \
    } while (0)
#else
#define TDECL do { } while (0)
#define TACC(i) do { } while (0)
#define TSTORE() do { } while (0)
#endif
enum { T_WIN = 0, T_PROJ, T_LN, T_QKV, T_QKVBAR, T_ATTN, T_OPROJ, T_FFN, T_POOL, T_MISC, T_POOL1, T_POOL2, T_PNODE, T_PTIME, T_PEDGE, T_PCOOC,
       T_F_W1 = 16, T_F_GELU, T_F_ADV1, T_F_W2, T_F_ADV2,              // FFN sub-phases
       T_E_MEAN = 21, T_E_W2 };      // pooled epilogue: the mean / mean_g columns, the W2 product; T_POOL keeps the output layer alone

// LayerNorm of the register-resident X^T (two-pass, biased variance, eps 1e-5); gamma/beta from LDS
__device__ __forceinline__ void layernorm(f4 (&xn)[kNT], const f4 (&x)[kNT], const float* gamma, const float* beta, int g, float& mean_o, float& rstd_o) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kNT; ++i) s += (x[i].x + x[i].y) + (x[i].z + x[i].w);     // rows 200..207 are exact zeros
    s += __shfl_xor(s, 16, 64);
    s += __shfl_xor(s, 32, 64);
    const float mean = s * (1.0f / kD);
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        if (i < 12 || g < 2) {            // rows 200..207 (tile 12, g >= 2) are padding
            const float d0 = x[i].x - mean, d1 = x[i].y - mean, d2 = x[i].z - mean, d3 = x[i].w - mean;
            v += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
        }
    }
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    const float rstd = 1.0f / sqrtf(v * (1.0f / kD) + 1e-5f);
    mean_o = mean; rstd_o = rstd;
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const f4 gm = lds4(gamma + 16 * i + 4 * g), bt = lds4(beta + 16 * i + 4 * g);   // zero beyond 200
        xn[i].x = (x[i].x - mean) * rstd * gm.x + bt.x;
        xn[i].y = (x[i].y - mean) * rstd * gm.y + bt.y;
        xn[i].z = (x[i].z - mean) * rstd * gm.z + bt.z;
        xn[i].w = (x[i].w - mean) * rstd * gm.w + bt.w;
    }
}

// acc[NT] += W(NT tiles of one head's q, k or v) . xn : 13 stream steps of NT fragments [k-chunk][tile], each multiplied
// as sub-groups of 4 and NT - 4 tiles whose fragments are read one sub-group ahead (8 fragments live instead of 14)
// skip > 0 (layer 0 of the inference kernels with constant input channels, fused3_plan.h): the first `skip` (3 or 6) k-chunks multiply rows of
// LN(x) that depend on the token through (mean, rstd) alone.  Their fragments are stepped over in place — the same fit / advance sequence, no
// LDS reads, no MFMAs: the stream, the packer's padding rule and the stage barriers stay as they are — and ONE MFMA per tile adds their sum
// at the end: A operand cst[64 u + lane] (cst wave-uniform; this lane's element of tile u: A | G | Bt | 0 by lane group), B operand ck
// (rs | -mean rs | 1 | 0 by lane group).  The order of a row's sum is bias, chunks skip .. 12, the rank-3 term, in every instance.  The
// operands are plain global loads issued at the group's head; hipcc waits for them (vmcnt) in front of the rank-3 MFMAs, by which time
// several stage crossings have drained them.
// Measured and NOT kept (profiles/const_qkv_ab.md): the operands loaded by inline asm (no wait of hipcc's in front of their use) together with
// a counted vmcnt(N) instead of vmcnt(0) at the stage crossings of the skipped chunks (N = the loads issued since the crossing before):
// slower than this form (-0.8 % against the parent where this form has -1.6 %).  The skip length as a template argument, with instances of their
// own for layer 0: 28 spilled VGPRs in the eight-wave kernels.  (The scalar test per unrolled chunk of this form is not free: a call WITHOUT
// constant channels runs 0.6 % slower than before the test was there; with them the kernel is 1.4 - 1.6 % faster.)
template <int NT>
__device__ __forceinline__ void qkv_group(f4 (&acc)[NT], const f4 (&xn)[kNT], const float xk0, const float xk1, WStream& ws, const float* ringl, bool active,
                                          const int skip = 0, const float* cst = nullptr, const int lane = 0, const float ck = 0.f) {
    constexpr int N2 = NT - 4;
    f4 fs[2][4];
    float ca[NT];
    ws.fit(NT);
    if (active) {
        if (skip == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) fs[0][u] = lds4(ringl + (ws.pos + u) * kFrag);
        } else {
#pragma unroll
            for (int u = 0; u < NT; ++u) ca[u] = cst[64 * u + lane];
        }
    }
#pragma unroll
    for (int kc = 0; kc < kKC; ++kc) {
        if (active && (kc >= kQkvSkipMax || kc >= skip)) {
#pragma unroll
            for (int u = 0; u < N2; ++u) fs[1][u] = lds4(ringl + (ws.pos + 4 + u) * kFrag);
            __builtin_amdgcn_sched_barrier(0);
            if (kc == kKC - 1) mma_group2<4>(&acc[0], fs[0], xk0, xk1); else mma_group<4>(&acc[0], fs[0], xn[kc]);
            __builtin_amdgcn_sched_barrier(0);
            if (kc + 1 < kKC) {
                const int p1 = ws.next_pos(NT, NT);
#pragma unroll
                for (int u = 0; u < 4; ++u) fs[0][u] = lds4(ringl + (p1 + u) * kFrag);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (kc == kKC - 1) mma_group2<N2>(&acc[4], fs[1], xk0, xk1); else mma_group<N2>(&acc[4], fs[1], xn[kc]);
            __builtin_amdgcn_sched_barrier(0);
        }
        ws.advance(NT);
        if (kc + 1 < kKC) ws.fit(NT);
        if (kc < kQkvSkipMax && active && kc + 1 == skip) {      // the first chunk that runs reads its own first sub-group (nobody read ahead for it)
#pragma unroll
            for (int u = 0; u < 4; ++u) fs[0][u] = lds4(ringl + (ws.pos + u) * kFrag);
        }
    }
    if (active && skip > 0) {
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[u] = mfma(ca[u], ck, acc[u]);
    }
}

// ---- FFN blocks: one block = the 26 fragments of one product of one step, at ring position 0 or 26.
// First product: h[2] (two 16-wide hidden tiles) = b1 + W1 . LN(x); 13 k-chunks of two fragments [k-chunk][tile] read one chunk ahead.
__device__ __forceinline__ void ffn_w1(f4 (&h)[2], const f4 (&xn)[kNT], const float xk0, const float xk1, const float* abuf, const float* b1p, const int g) {
    if (b1p != nullptr) { h[0] = lds4(b1p + 4 * g); h[1] = lds4(b1p + 16 + 4 * g); }
    else { h[0] = zero4(); h[1] = zero4(); }
    f4 sa[2][2];
    sa[0][0] = lds4(abuf); sa[0][1] = lds4(abuf + kFrag);
#pragma unroll
    for (int kc = 0; kc < kKC; ++kc) {
        const int cur = kc & 1;
        if (kc + 1 < kKC) {
            sa[cur ^ 1][0] = lds4(abuf + (size_t)(2 * (kc + 1)) * kFrag);
            sa[cur ^ 1][1] = lds4(abuf + (size_t)(2 * (kc + 1) + 1) * kFrag);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (kc == kKC - 1) mma_group2<2>(h, sa[cur], xk0, xk1); else mma_group<2>(h, sa[cur], xn[kc]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// Second product: acc (13 model-dim tiles) += W2[:, the two hidden tiles] . h; fragments [tile u][n-tile i] in sub-groups (4,3,3,3)
// read one sub-group ahead
__device__ __forceinline__ void ffn_w2(f4 (&acc)[kNT], const f4 (&h)[2], const float* bbuf) {
    f4 fs[2][4];
#pragma unroll
    for (int v = 0; v < 4; ++v) fs[0][v] = lds4(bbuf + (size_t)v * kFrag);
#pragma unroll
    for (int gi = 0; gi < 8; ++gi) {
        const int u = gi >> 2, q = gi & 3;
        const int i0 = q == 0 ? 0 : 4 + 3 * (q - 1), n = q == 0 ? 4 : 3;
        if (gi + 1 < 8) {
            const int u2 = (gi + 1) >> 2, q2 = (gi + 1) & 3;
            const int j0 = q2 == 0 ? 0 : 4 + 3 * (q2 - 1), n2 = q2 == 0 ? 4 : 3;
#pragma unroll
            for (int v = 0; v < 4; ++v) if (v < n2) fs[(gi + 1) & 1][v] = lds4(bbuf + (size_t)(u2 * 13 + j0 + v) * kFrag);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (n == 4) mma_group<4>(&acc[i0], fs[gi & 1], h[u]); else mma_group<3>(&acc[i0], fs[gi & 1], h[u]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- the attention-shaped products (the forward's S^T, O^T and out-projection; the attention backward runs each of them several times)
template <int TPW>
__device__ __forceinline__ void s_like(f4 (&sa)[TPW], const float* base, const f4 (&q)[7], int c, int g) {       // sa[kt] += rows(16 kt ..)(base) . q   (forward: S^T = K Q^T)
    const float q6 = kpack4(q[6]);       // rows 96 .. 99 of q for the one-MFMA last d-chunk; row tiles of `base` in chunks of 4
#pragma unroll
    for (int kh = 0; kh < TPW / 4; ++kh) {
        const float* kbase = base + (64 * kh + c) * kKV + 4 * g;
        f4 kf[2][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) kf[0][kt] = lds4(kbase + 16 * kt * kKV);
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            if (j + 1 < 6) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) kf[(j + 1) & 1][kt] = lds4(kbase + 16 * kt * kKV + 16 * (j + 1));
            } else if (j + 1 == 6) {     // d = 96 .. 99 in ONE MFMA: lane group g reads base[row][96 + g] (kbase points at column 4 g)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) kf[0][kt].x = kbase[16 * kt * kKV + 96 - 3 * g];
            }
            __builtin_amdgcn_sched_barrier(0);
            if (j == 6) mma_group1<4>(&sa[4 * kh], kf[0], q6); else mma_group<4>(&sa[4 * kh], kf[j & 1], q[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}
// the first N <= 4 row tiles only (the packed forward: a pair of N token tiles); every sa[kt] is the chain s_like runs for it
template <int N>
__device__ __forceinline__ void s_like_n(f4 (&sa)[4], const float* base, const f4 (&q)[7], int c, int g) {
    static_assert(N >= 1 && N <= 4, "one chunk of row tiles");
    const float q6 = kpack4(q[6]);
    const float* kbase = base + c * kKV + 4 * g;
    f4 kf[2][N];
#pragma unroll
    for (int kt = 0; kt < N; ++kt) kf[0][kt] = lds4(kbase + 16 * kt * kKV);
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        if (j + 1 < 6) {
#pragma unroll
            for (int kt = 0; kt < N; ++kt) kf[(j + 1) & 1][kt] = lds4(kbase + 16 * kt * kKV + 16 * (j + 1));
        } else if (j + 1 == 6) {
#pragma unroll
            for (int kt = 0; kt < N; ++kt) kf[0][kt].x = kbase[16 * kt * kKV + 96 - 3 * g];
        }
        __builtin_amdgcn_sched_barrier(0);
        if (j == 6) mma_group1<N>(&sa[0], kf[0], q6); else mma_group<N>(&sa[0], kf[j & 1], q[j]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
template <int TPW>
__device__ __forceinline__ void pv_like(f4 (&oa)[7], const float* base, const f4 (&p)[TPW], int c, int g) {     // oa += rows(base)^T . p   (forward: O^T = V^T P^T)
    // the rows as the A operand: sub-steps (row tile kt, d-tiles 0..3 | 4..6), read one sub-step ahead (8 fragments live, not 14)
    auto load_v = [&](f4 (&va)[4], int kt, int j0, int n) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < n) {
                const float* vp = base + (16 * kt + 4 * g) * kKV + 16 * (j0 + j) + c;
                va[j].x = vp[0]; va[j].y = vp[kKV]; va[j].z = vp[2 * kKV]; va[j].w = vp[3 * kKV];
            }
        }
    };
    f4 va[2][4];
    load_v(va[0], 0, 0, 4);
#pragma unroll
    for (int st = 0; st < 2 * TPW; ++st) {
        const int kt = st >> 1, half = st & 1;
        if (st + 1 < 2 * TPW) load_v(va[(st + 1) & 1], (st + 1) >> 1, ((st + 1) & 1) ? 4 : 0, ((st + 1) & 1) ? 3 : 4);
        __builtin_amdgcn_sched_barrier(0);
        if (half == 0) mma_group<4>(&oa[0], va[st & 1], p[kt]); else mma_group<3>(&oa[4], va[st & 1], p[kt]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// acc (13 model-dim tiles) += W^T(7 d-chunks x 13 tiles, from the ring) . t (7 head-dim tiles)   (forward: the out-projection)
// 7 steps (d-chunk j) of 13 fragments (n-tile i), sub-groups (4,3,3,3) read one ahead; the last d-chunk (rows 96 .. 99 of t) is one MFMA
__device__ __forceinline__ void proj_t(f4 (&acc)[kNT], const f4 (&t)[7], WStream& ws, const float* ringl, bool active) {
    ws.fit(13);
    f4 fs[2][4];
    float t6 = 0.f;
    if (active) {
#pragma unroll
        for (int v = 0; v < 4; ++v) fs[0][v] = lds4(ringl + (ws.pos + v) * kFrag);
        t6 = kpack4(t[6]);
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const int pcur = ws.pos;
        const int pnext = ws.next_pos(13, 13);
        if (active) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int gi = 4 * j + q;
                const int i0 = q == 0 ? 0 : 4 + 3 * (q - 1), n = q == 0 ? 4 : 3;
                if (q + 1 < 4) {
                    const int j0 = 4 + 3 * q;
#pragma unroll
                    for (int v = 0; v < 3; ++v) fs[(gi + 1) & 1][v] = lds4(ringl + (pcur + j0 + v) * kFrag);
                } else if (j + 1 < 7) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) fs[(gi + 1) & 1][v] = lds4(ringl + (pnext + v) * kFrag);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (j == 6) { if (n == 4) mma_group1<4>(&acc[i0], fs[gi & 1], t6); else mma_group1<3>(&acc[i0], fs[gi & 1], t6); }
                else if (n == 4) mma_group<4>(&acc[i0], fs[gi & 1], t[j]); else mma_group<3>(&acc[i0], fs[gi & 1], t[j]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        ws.advance(13);
        if (j + 1 < 7) ws.fit(13);
    }
}
}  // namespace v3
}  // namespace dygnn
