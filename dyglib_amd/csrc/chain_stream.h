// The weight stream of the row-block chain kernels (tgat_chain.hip, memory_rnn.hip): device-side pieces shared by every kernel that runs
// Out[R][N] = Act[R][K] . W^T with the activations in LDS and the packed weight fragments (tgat_chain.h) streamed into the A operand of
// `v_mfma_f32_4x4x1_16b_f32`.  gfx950 only.  The fragment layout and the order of operations of a row are described in tgat_chain.hip.
#pragma once
#include <cstdlib>
#include "common.h"

namespace dygnn {
namespace chain {

using f4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, c, 0, 0, 0); }

constexpr int kWaves = 8;
constexpr int kThreads = kWaves * 64;
__host__ __device__ inline int r16(int K) { return (K + 15) & ~15; }
__host__ __device__ inline int pad_ld(int K) {           // smallest row stride >= K with stride % 32 == 16: the four rows of an operand read fall on distinct banks
    const int l = r16(K);
    return (l & 16) ? l : l + 16;
}

// ---- the weight stream of a wave ------------------------------------------------------------------------------------------------
// A stage gives wave w the tiles t = w, w + 8, ... < T.  Their fragments form ONE sequence of steps (tile by tile, chunk by chunk) that
// runs through a ring of U float4 registers filled U steps ahead -- across tile boundaries, so the stream only drains at the end of a
// stage.  Steady state is branch-free but for the tile epilogue (refills are always issued; beyond the stream they re-read the wave's
// first tile), so the compiler counts the loads in flight (s_waitcnt vmcnt(U-1)) instead of draining them.  The LDS operands of step
// s+1 are read before the MFMAs of step s.
// AF: act(t) = LDS base of the activation operand of tile t.  Ep(t, acc): the finished tile -- every lane holds the sums of
// Out[4m + j][16t + 4ng .. +3] in acc[m]; the ks == 0 lanes store.
#ifndef DYGNN_CHAIN_U
#define DYGNN_CHAIN_U 4      // ring depth: the chains run at the rate a CU streams fragments through its vector L1 (~35 B/clk measured), 4 .. 16 deep gave the same time per step; 4 is the least code
#endif
constexpr int U = DYGNN_CHAIN_U;

struct IdTile { __device__ __forceinline__ int operator()(int t) const { return t; } };
// TM: local tile index -> tile index in the packed stage (a workgroup that owns a slice of a stage's tiles).
// start() issues the first U fragment loads -- they depend on nothing the kernel computes, so a stage's ring is started BEFORE the
// previous stage runs (its loads are then older than that stage's refills and have landed when it ends); run() consumes.
template <class TM>
struct WStream {
    const f4* pk;
    int T, nch, wave, lane, pt, pch, adv;
    const f4* pp;
    TM tmap;
    f4 ring[U];
    __device__ __forceinline__ WStream(const f4* pk_, int T_, int nch_, int wave_, int lane_, TM tm) : pk(pk_), T(T_), nch(nch_), wave(wave_), lane(lane_), pt(wave_), pch(0), tmap(tm) {
        adv = wave < T ? 64 : 0;
        pp = wave < T ? pk + (size_t)tmap(wave) * nch * 64 + lane : pk;
#pragma unroll
        for (int u = 0; u < U; ++u) fetch(ring[u]);
    }
    // Behind the wave's last fragment every lane re-reads ONE address (a single 16-byte request): the refill stays unconditional -- the
    // compiler keeps counting the loads in flight -- without fetching a junk KiB per step (U junk fragments per stage and wave were 10-70 %
    // of these short streams' traffic).
    __device__ __forceinline__ void fetch(f4& dst) {
        dst = *pp;
        pp += adv;
        if (++pch == nch) {
            pch = 0; pt += kWaves;
            if (pt < T) pp = pk + (size_t)tmap(pt) * nch * 64 + lane;
            else { pp = pk; adv = 0; }
        }
    }
    template <int MT, class AF, class Ep>
    __device__ __forceinline__ void run(int lda, AF actf, Ep ep) {
        if (wave >= T) return;
        const int j = lane & 3, ks = (lane >> 2) & 3;
        const int S = ((T - wave + kWaves - 1) / kWaves) * nch;
        const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
        int ct = wave, cch = 0;                                           // consume cursor
        const float* ab = actf(ct) + j * lda + 4 * ks;
        f4 acc[MT], bn[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) { acc[m] = zero; bn[m] = *reinterpret_cast<const f4*>(ab + m * 4 * lda); }
        auto step = [&](f4& slot, bool refill) {
            const f4 w = slot;
            f4 b[MT];
#pragma unroll
            for (int m = 0; m < MT; ++m) b[m] = bn[m];
            const bool tile_end = cch + 1 == nch;
            const int nt = tile_end ? ct + kWaves : ct, nc = tile_end ? 0 : cch + 1;
            const float* nab = tile_end ? actf(nt < T ? nt : ct) + j * lda + 4 * ks : ab;
#pragma unroll
            for (int m = 0; m < MT; ++m) bn[m] = *reinterpret_cast<const f4*>(nab + m * 4 * lda + 16 * nc);      // (behind the last step: a valid, unused read)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma4(w.x, b[m].x, acc[m]);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma4(w.y, b[m].y, acc[m]);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma4(w.z, b[m].z, acc[m]);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = mfma4(w.w, b[m].w, acc[m]);
            if (refill) fetch(slot);
            if (tile_end) {
                f4 r[MT];
#pragma unroll
                for (int m = 0; m < MT; ++m) {          // k-slices 0 + 1, 2 + 3, then the pairs: fixed order
                    f4 v = acc[m];                      // rotations inside the row of 16 lanes (DPP row_ror 4, then 8): no LDS
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x = v[e];
                        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x124, 0xf, 0xf, false));
                        x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x128, 0xf, 0xf, false));
                        v[e] = x;
                    }
                    r[m] = v;
                    acc[m] = zero;
                }
                ep(ct, r);
            }
            ct = nt; cch = nc; ab = nab;
        };
        int s0 = 0;
        for (; s0 + U <= S; s0 += U) {
#pragma unroll
            for (int u = 0; u < U; ++u) step(ring[u], true);
        }
#pragma unroll
        for (int u = 0; u < U - 1; ++u)
            if (s0 + u < S) step(ring[u], false);
    }
};
template <class TM>
__device__ __forceinline__ WStream<TM> wstream(const f4* pk, int T, int nch, int wave, int lane, TM tm) { return WStream<TM>(pk, T, nch, wave, lane, tm); }
__device__ __forceinline__ WStream<IdTile> wstream(const f4* pk, int T, int nch, int wave, int lane) { return WStream<IdTile>(pk, T, nch, wave, lane, IdTile()); }

// ---- host side: launch shapes -------------------------------------------------------------------------------------------------------
constexpr size_t kLdsMax = 160 * 1024;

template <class K>
static int set_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return DYGNN_OK;
}
// Rows per workgroup = 4 MT.  Small levels take few rows so that they still spread over the chip (the weights are re-streamed from L2 by
// every workgroup: 4 rows at 800 rows = 200 workgroups); large levels take 32 rows (every weight fragment feeds 32 MFMAs).  A row's
// bits do not depend on the choice.
static int pick_mt(int64_t n) { return n <= 2048 ? 1 : n <= 8192 ? 2 : 4; }
static int env_mt(const char* name, int mt) {          // DYGNN_CHAIN_MT / DYGNN_GRU_MT / DYGNN_RNN_MT = 1 | 2 | 4 | 8: tuning override (read per call)
    const char* e = getenv(name);
    if (e && (e[0] == '1' || e[0] == '2' || e[0] == '4' || e[0] == '8') && e[1] == 0) return e[0] - '0';
    return mt;
}
static int env_slices(const char* name, int dflt) {    // DYGNN_GRU_SLICES / DYGNN_RNN_SLICES = 1 .. 6: tuning override (read per call)
    const char* e = getenv(name);
    return (e && e[0] >= '1' && e[0] <= '6' && e[1] == 0) ? e[0] - '0' : dflt;
}

}  // namespace chain
}  // namespace dygnn
