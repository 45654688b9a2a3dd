// Token compaction and pair packing of the fused DyGFormer inference kernels: the arithmetic that the kernels, the plan kernel
// (dygformer_pack_plan.hip) and the host (tests) share.  Everything here is integer arithmetic on the window lengths of a call.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define DYGNN_HD __host__ __device__
#else
#define DYGNN_HD
#endif

namespace dygnn {
namespace v3 {

// A patch that holds padding positions only has a constant encoder input (node row 0, edge row 0, zeroed time features, lut[0] + lut[0]),
// so all such tokens of a pair are one token computed once.  Per side: R = patches with a real position (the target node and the
// min(len, L - 1) neighbours in front of it), m = T_side - R all-padding patches.  Compact order: R_s source tokens, R_d destination
// tokens, then one padding token if m_s + m_d > 0.
struct PairTokens { int Rs, Rd, ms, md, Tc; };
DYGNN_HD inline PairTokens pair_tokens(int len_s, int len_d, int L, int P, int T_s, int T_d) {
    PairTokens r;
    const int ws = (len_s < L - 1 ? len_s : L - 1) + 1, wd = (len_d < L - 1 ? len_d : L - 1) + 1;
    r.Rs = (ws + P - 1) / P; r.Rd = (wd + P - 1) / P;
    if (r.Rs > T_s) r.Rs = T_s;          // (a call's padded length covers every window of the call: never taken)
    if (r.Rd > T_d) r.Rd = T_d;
    r.ms = T_s - r.Rs; r.md = T_d - r.Rd;
    r.Tc = r.Rs + r.Rd + (r.ms + r.md > 0 ? 1 : 0);
    return r;
}

// what a kernel keeps of it (wave-uniform): tokens and source tokens of the compact order, those of the padded call, the padding token
struct TokOrder { int T, Ts, Tf, Tsf, padtok; };

// ---- the packing plan.  Pairs of 1 .. 4 token tiles (16 tokens = one wave) are laid into workgroups of 8 waves by fixed patterns,
// pairs taken in the order of their rank within their class (class = tiles):
//   A  4+4                          floor(n4 / 2) workgroups
//   B  3+3 (+2 | +1+1 | +1 | -)     floor(n3 / 2) workgroups; the first c332 take a 2, the next ones two 1s while there are any
//   C  2+2+2+2                      the remaining 2s
//   D  1 x 8                        the remaining 1s
//   E  what is left over (at most one 4, one 3, three 2s, seven 1s), first-fit in that order
// Every workgroup but the last of E holds at least two pairs, so the plan never needs more than ceil(B / 2) workgroups.
// The plan as the kernel reads it: int32 [ceil(B / 2) workgroups][8 waves] = the pair of every wave, -1 for a wave without one.  A pair's
// waves are consecutive, so a wave finds its pair's first wave and tile count among the eight entries of its workgroup; a workgroup
// beyond the plan's count holds -1 eight times.
struct PlanSlot { int32_t wg, fw; };
struct PackPlan {
    int32_t n[5];                        // n[k] = pairs of k tiles
    int32_t baseB, c332, use1, baseC, wgC, baseD, wgD, baseE, used;
    int32_t lo[5];                       // leftover pairs of each class (the last ranks of the class)
    uint8_t lo_wg[5][8], lo_fw[5][8];    // ... their workgroup (relative to baseE) and first wave
};
DYGNN_HD inline PackPlan make_pack_plan(int64_t n1, int64_t n2, int64_t n3, int64_t n4) {
    PackPlan p{};
    p.n[1] = (int32_t)n1; p.n[2] = (int32_t)n2; p.n[3] = (int32_t)n3; p.n[4] = (int32_t)n4;
    const int32_t wgA = p.n[4] / 2, wgB = p.n[3] / 2;
    p.baseB = wgA;
    p.c332 = wgB < p.n[2] ? wgB : p.n[2];
    const int32_t room1 = 2 * (wgB - p.c332);
    p.use1 = room1 < p.n[1] ? room1 : p.n[1];
    p.baseC = p.baseB + wgB;
    const int32_t n2r = p.n[2] - p.c332, n1r = p.n[1] - p.use1;
    p.wgC = n2r / 4;
    p.baseD = p.baseC + p.wgC;
    p.wgD = n1r / 8;
    p.baseE = p.baseD + p.wgD;
    p.lo[4] = p.n[4] & 1; p.lo[3] = p.n[3] & 1; p.lo[2] = n2r % 4; p.lo[1] = n1r % 8;
    int fill[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bins = 0;
    for (int k = 4; k >= 1; --k)
        for (int i = 0; i < p.lo[k]; ++i) {
            int w = 0;
            while (w < bins && fill[w] + k > 8) ++w;
            if (w == bins) ++bins;
            p.lo_wg[k][i] = (uint8_t)w; p.lo_fw[k][i] = (uint8_t)fill[w];
            fill[w] += k;
        }
    p.used = p.baseE + bins;
    return p;
}
// workgroup and first wave of the pair with rank `rank` among the pairs of `k` tiles
DYGNN_HD inline PlanSlot plan_slot(const PackPlan& p, int k, int32_t rank) {
    int32_t full, r;
    if (k == 4) {
        full = 2 * (p.n[4] / 2);
        if (rank < full) return {rank / 2, 4 * (rank & 1)};
    } else if (k == 3) {
        full = 2 * (p.n[3] / 2);
        if (rank < full) return {p.baseB + rank / 2, 3 * (rank & 1)};
    } else if (k == 2) {
        if (rank < p.c332) return {p.baseB + rank, 6};
        r = rank - p.c332;
        if (r < 4 * p.wgC) return {p.baseC + r / 4, 2 * (r & 3)};
        full = p.c332 + 4 * p.wgC;
    } else {
        if (rank < p.use1) return {p.baseB + p.c332 + rank / 2, 6 + (rank & 1)};
        r = rank - p.use1;
        if (r < 8 * p.wgD) return {p.baseD + r / 8, r & 7};
        full = p.use1 + 8 * p.wgD;
    }
    const int i = rank - full;
    return {p.baseE + p.lo_wg[k][i], p.lo_fw[k][i]};
}

// ---- constant input channels of layer 0 (DESIGN §4.3 "Constant input channels").  A channel whose table is flagged all zero leaves its
// rows of the encoder input at the projection bias b for every token, so the first K0 rows of LN0(x0) depend on the token through its
// LayerNorm mean mu and reciprocal standard deviation rs alone:  LN(x0)[k] = rs . gamma_k b_k - mu rs . gamma_k + beta_k  (k < K0), and
//     sum_{k < K0} W[n][k] LN(x0)[k] = rs A[n] + (-mu rs) G[n] + Bt[n],   A = sum W gamma b,  G = sum W gamma,  Bt = sum W beta
// — a K = 3 product, one MFMA per output tile in place of the K0 / 16 k-chunks (K0 = 48: node table zero; 96: node and edge).
// A layer's Q/K/V product has 38 output tiles in stream order: per head the q group's 7 (the seventh = the combined tile of rows 96 .. 99 of
// q | k | v: FragDesc kmode 8), then 6 of k, then 6 of v.
constexpr int kQkvTiles = 38;
constexpr int kQkvSkipMax = 6;           // k-chunks the rank-3 term can stand for: 3 (K0 = 48) or 6 (K0 = 96)
// in_proj row (0 .. 599: q | k | v blocks of 200, head h at 100 h) of row c (0 .. 15) of output tile `tile`; -1: the row is padding
DYGNN_HD inline int qkv_tile_row(int tile, int c) {
    const int h = tile / 19, t = tile % 19;
    if (t == 6) return (c >> 2) < 3 ? 200 * (c >> 2) + 100 * h + 96 + (c & 3) : -1;
    const int part = t < 6 ? 0 : (t - 7) / 6 + 1, j = t < 6 ? t : (t - 7) % 6;
    return 200 * part + 100 * h + 16 * j + c;
}
// element `lane` (c = lane & 15: the tile's row, g = lane >> 4: the k column) of the rank-3 term's MFMA A operand of `tile`: A | G | Bt | 0 of
// the row.  in_proj: [600][200] of layer 0; gamma, beta: norm_layers.0; bias: the projection biases in model-dim order (>= K0 floats).  Every
// sum is one float64 chain over k ascending, rounded to fp32 once.
DYGNN_HD inline float qkv0_const(const float* in_proj, const float* gamma, const float* beta, const float* bias, int K0, int tile, int lane) {
    const int row = qkv_tile_row(tile, lane & 15), g = lane >> 4;
    if (row < 0 || g == 3) return 0.f;
    const float* wr = in_proj + (size_t)row * 200;
    double s = 0.0;
    for (int k = 0; k < K0; ++k) {
        const double m = g == 0 ? (double)gamma[k] * (double)bias[k] : g == 1 ? (double)gamma[k] : (double)beta[k];
        s += (double)wr[k] * m;
    }
    return (float)s;
}

// ---- the per-side token sums of the pooled layer (row_sums8, fused3_device.h): where the reduce-scatter leaves its sums.  Its eight inputs per
// lane are two register tiles, input k = 4 u + r = row 4 g + r of tile u in lane group g = lane >> 4; the 16 lanes of a group are the
// row's 16 tokens, in four banks of four lanes.  Afterwards every lane of bank `bank` holds in result j (0, 1) the token sum of input
DYGNN_HD inline int pool_sum_input(int j, int bank) { return 4 * (bank >> 1) + 2 * (bank & 1) + j; }
// The first lane of every bank stores its two results as one pair of words.  Inside a block of two consecutive tiles [2][16] rows (gpool's
// 32 hidden units of a step, pool's tiles 2 i and 2 i + 1) the pair begins at row pool_sum_row(lane) of tile pool_sum_tile(lane); where the
// two input tiles are one tile's source and destination form (pool's tile 12), pool_sum_tile is the side.
DYGNN_HD inline bool pool_sum_stores(int lane) { return (lane & 3) == 0; }
DYGNN_HD inline int pool_sum_tile(int lane) { return (lane >> 3) & 1; }
DYGNN_HD inline int pool_sum_row(int lane) { return 4 * (lane >> 4) + ((lane >> 1) & 2); }

}  // namespace v3
}  // namespace dygnn
