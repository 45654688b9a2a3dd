// The packing plan of a packed fused DyGFormer launch (fused3_plan.h; consumer: k_dygformer_fused3_packed in fused3_forward.h).
// One workgroup: every thread takes a contiguous run of pairs, counts its pairs of 1 .. 4 token tiles, an exclusive scan over the threads
// gives every pair its rank within its class, and the closed-form plan turns (class, rank) into a (workgroup, first wave) slot.  Ranks
// follow the pair order, so the plan is a function of the call alone.  Runs on the launch's stream behind window_lengths_device; the
// host never reads it.
#include "dygformer_layout.h"
#include "fused3_plan.h"

namespace dygnn {
namespace v3 {

constexpr int kPlanThreads = 1024;

__device__ __forceinline__ int pair_tile_count(const int32_t* hist_len, const CallDims* cd, int64_t b, int64_t B, int64_t G, int L, int P) {
    const CallDims d = cd[b / G];
    const PairTokens t = pair_tokens(hist_len[b], hist_len[B + b], L, P, d.T_s, d.T_d);
    const int nt = (t.Tc + 15) / 16;
    return nt < 1 ? 1 : nt > 4 ? 4 : nt;         // (pairs of <= 64 tokens: the host launches nothing else here)
}

__global__ __launch_bounds__(kPlanThreads) void k_pack_plan(const int32_t* hist_len, const CallDims* cd, int64_t B, int64_t G, int L, int P, int32_t* plan,
                                                            int32_t max_wg) {
    __shared__ int32_t cnt[2][4][kPlanThreads];
    __shared__ PackPlan pp;
    const int t = threadIdx.x;
    const int64_t chunk = (B + kPlanThreads - 1) / kPlanThreads;
    const int64_t b0 = t * chunk, b1 = b0 + chunk < B ? b0 + chunk : B;
    int32_t mine[4] = {0, 0, 0, 0};
    for (int64_t b = b0; b < b1; ++b) ++mine[pair_tile_count(hist_len, cd, b, B, G, L, P) - 1];
    for (int k = 0; k < 4; ++k) cnt[0][k][t] = mine[k];
    __syncthreads();
    int cur = 0;
    for (int off = 1; off < kPlanThreads; off <<= 1) {       // inclusive scan over the threads, all four classes at once
        for (int k = 0; k < 4; ++k) cnt[cur ^ 1][k][t] = cnt[cur][k][t] + (t >= off ? cnt[cur][k][t - off] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (t == 0) {
        pp = make_pack_plan(cnt[cur][0][kPlanThreads - 1], cnt[cur][1][kPlanThreads - 1], cnt[cur][2][kPlanThreads - 1], cnt[cur][3][kPlanThreads - 1]);
    }
    __syncthreads();
    const bool fits = pp.used <= max_wg;                     // (never more than ceil(B / 2): fused3_plan.h)
    int32_t* ent = plan;
    for (int64_t i = t; i < (int64_t)max_wg * 8; i += kPlanThreads) ent[i] = -1;      // a wave without a pair; a workgroup beyond the plan: eight of them
    __syncthreads();
    int32_t rank[4];
    for (int k = 0; k < 4; ++k) rank[k] = cnt[cur][k][t] - mine[k];
    for (int64_t b = b0; b < b1 && fits; ++b) {
        const int nt = pair_tile_count(hist_len, cd, b, B, G, L, P);
        const PlanSlot sl = plan_slot(pp, nt, rank[nt - 1]++);
        for (int w = 0; w < nt; ++w) ent[(int64_t)sl.wg * 8 + sl.fw + w] = (int32_t)b;
    }
}

}  // namespace v3

int pack_plan_device(const Dims& d, int64_t B, int64_t G, char* ws, const WorkspaceLayout& wl, hipStream_t s) {
    using namespace v3;
    hipLaunchKernelGGL(k_pack_plan, dim3(1), dim3(kPlanThreads), 0, s, reinterpret_cast<const int32_t*>(ws + wl.hist_len),
                       reinterpret_cast<const CallDims*>(ws + wl.dims), B, G, d.L, d.P, reinterpret_cast<int32_t*>(ws + wl.dims + plan_offset(B, G)),
                       (int32_t)((B + 1) / 2));
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace dygnn

// The plan of given tile counts, computed on the host by the kernel's own arithmetic (tests): wg[i], fw[i] = slot of pair i.
// Returns the number of workgroups used, or -1 for a tile count outside 1 .. 4.
extern "C" int64_t dygnn_dygformer_pack_plan_host(const int32_t* tiles, int64_t n, int32_t* wg, int32_t* fw) {
    using namespace dygnn::v3;
    int64_t cnt[5] = {0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        if (tiles[i] < 1 || tiles[i] > 4) return -1;
        ++cnt[tiles[i]];
    }
    const PackPlan pp = make_pack_plan(cnt[1], cnt[2], cnt[3], cnt[4]);
    int32_t rank[5] = {0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; ++i) {
        const PlanSlot sl = plan_slot(pp, tiles[i], rank[tiles[i]]++);
        wg[i] = sl.wg; fw[i] = sl.fw;
    }
    return pp.used;
}
// tokens of a pair in the compact order (tests): out = {R_s, R_d, m_s, m_d, Tc}
extern "C" void dygnn_dygformer_pair_tokens_host(int32_t len_s, int32_t len_d, int32_t L, int32_t P, int32_t T_s, int32_t T_d, int32_t* out) {
    const dygnn::v3::PairTokens t = dygnn::v3::pair_tokens(len_s, len_d, L, P, T_s, T_d);
    out[0] = t.Rs; out[1] = t.Rd; out[2] = t.ms; out[3] = t.md; out[4] = t.Tc;
}
// where the pooled layer's reduce-scatter leaves its sums (tests): out = {1 if the lane stores, tile, first row, input of result 0, of result 1}
extern "C" void dygnn_dygformer_pool_sum_slot_host(int32_t lane, int32_t* out) {
    using namespace dygnn::v3;
    const int bank = (lane & 15) >> 2;
    out[0] = pool_sum_stores(lane) ? 1 : 0; out[1] = pool_sum_tile(lane); out[2] = pool_sum_row(lane);
    out[3] = pool_sum_input(0, bank); out[4] = pool_sum_input(1, bank);
}
