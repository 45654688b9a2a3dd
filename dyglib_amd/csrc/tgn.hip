// TGN and DyRep inference: ONE memory-update step (memory_update) inside ONE memory-attention stage (memory_attention) over the stages of
// tgat_stages.h; the two differ in the cell and in what a call returns and commits.
#include "memory_rnn.h"
#include "tgn.h"

namespace dygnn {

// TGN on PRE-SAMPLED levels (random sampling strategies): what k_tgat_expand's `tt` does while it writes level 0 — every level-0 slot names
// itself owner of its node (slot code: level-1 entry q, neighbour column j, or k for the entry itself), the two list counters are zeroed
__global__ void k_tgn_touch_levels(const int32_t* __restrict__ ids0, int64_t n1, int k, TgnTouch tt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2) tt.counts[i] = 0;
    if (i >= n1 * (k + 1)) return;
    const int32_t node = ids0[i];
    if (node < 0 || node >= tt.N) return;
    if (i < n1) tt.owner[node] = (int32_t)(i * (k + 1) + k);
    else { const int64_t q = (i - n1) / k; tt.owner[node] = (int32_t)(q * (k + 1) + (i - n1 - q * k)); }
}

// ================================================================================================
// TGN (BASELINE config 5; reference models/MemoryModel.py): memory bank + last-message aggregation + GRU update +
// the same temporal graph attention over (memory + raw) node features.
// State (owned by the caller, one per model): memory M [N][Fn], last-update time U [N] (float32), and ONE pending raw
// message per node (msg [N][2Fn+Ft+Fe], its float64 time, a flag): the reference keeps a Python list per node
// (MemoryModel.py:389-407) but its aggregator only ever reads the last element (:284-291), and lists are cleared
// whole (:400-407), so the last message is the entire observable state.
// ================================================================================================
// End of a positive call, one launch: for every batch node (a) persist the updated memory if it had a pending message and (b) store its
// new raw message (MemoryModel.py:142-161, :223-241, :425-459).  Messages are stored source role first, then destination role, and only a
// node's LAST stored message is ever read (:284-291): entry e = role * B + i (role 0 = source); the last entry of a node does the work
// for that node, the others exit.  "Had a pending message" is read from the call's pendf (written by the list pass), not from
// has_msg, which this kernel rewrites; the other endpoint's updated memory is Mnew when it was pending, M when not (nobody writes it then),
// so no workgroup reads what another one writes.
__global__ __launch_bounds__(256) void k_tgn_commit(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const double* __restrict__ times,
                                                      const int64_t* __restrict__ eids, int64_t B, const float* __restrict__ Mnew, const int32_t* __restrict__ pendf,
                                                      float* __restrict__ M, float* __restrict__ U, const float* __restrict__ edge_feat,
                                                      const float* __restrict__ tw, const float* __restrict__ tb, int Fn, int Fe, int Ft, float* __restrict__ msg,
                                                      double* __restrict__ msg_t, int32_t* __restrict__ has_msg, int64_t N) {
    const int64_t e = blockIdx.x;
    const bool role = e >= B;
    const int64_t i = role ? e - B : e;
    const int64_t node = role ? dst[i] : src[i];
    const int64_t o = role ? src[i] : dst[i];
    if (node < 0 || node >= N || o < 0 || o >= N) return;      // never index the state tables out of range (the host API raises IndexError for such ids)
    int later = 0;
    for (int64_t e2 = e + 1 + threadIdx.x; e2 < 2 * B; e2 += blockDim.x) {
        const int64_t i2 = e2 >= B ? e2 - B : e2;
        const int64_t n2 = e2 >= B ? dst[i2] : src[i2], o2 = e2 >= B ? src[i2] : dst[i2];
        later |= (n2 == node && o2 >= 0 && o2 < N) ? 1 : 0;
    }
    if (__syncthreads_or(later)) return;
    const bool pend = pendf[node] != 0, pend_o = pendf[o] != 0;
    const float* mn = pend ? Mnew + node * Fn : M + node * Fn;      // the node's updated memory (MemoryModel.py:142-145 persists exactly this)
    const float* mo = pend_o ? Mnew + o * Fn : M + o * Fn;
    const float u = pend ? (float)msg_t[node] : U[node];            // last-update time after the persist (:447-459)
    const int D = 2 * Fn + Ft + Fe;
    const float dt = (float)times[i] - u;                           // float32 - float32 (MemoryModel.py:232-233)
    float* m = msg + node * D;
    for (int f = threadIdx.x; f < D; f += blockDim.x) {
        float v;
        if (f < Fn) v = mn[f];
        else if (f < 2 * Fn) v = mo[f - Fn];
        else if (f < 2 * Fn + Ft) v = cosf(fmaf(dt, tw[f - 2 * Fn], tb[f - 2 * Fn]));
        else v = edge_feat[(size_t)eids[i] * Fe + (f - 2 * Fn - Ft)];
        m[f] = v;
        if (pend && f < Fn) M[node * Fn + f] = v;                   // persist
    }
    __syncthreads();                                                // msg_t[node] was read above by every thread
    if (threadIdx.x == 0) {
        if (pend) U[node] = u;
        msg_t[node] = times[i];
        has_msg[node] = 1;
    }
}

int tgn_touch_levels(hipStream_t s, const int32_t* ids0, int64_t n1, int k, const TgnTouch& touch) {
    hipLaunchKernelGGL(k_tgn_touch_levels, dim3((unsigned)ceil_div(n1 * (k + 1), 256)), dim3(256), 0, s, ids0, n1, k, touch);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

int tgn_commit(hipStream_t s, const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t n_pos, const float* Mnew,
               const int32_t* pendf, const dygnn_tgn_state* st, const float* edge_feat, const float* tw, const float* tb, int Fn, int Fe, int Ft) {
    hipLaunchKernelGGL(k_tgn_commit, dim3((unsigned)(2 * n_pos)), dim3(256), 0, s, src, dst, times, edge_ids, n_pos, Mnew, pendf, st->memory, st->last_update, edge_feat,
                       tw, tb, Fn, Fe, Ft, st->msg, st->msg_time, st->has_msg, st->num_nodes);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

// ---- the nodes a call reads (TGN) --------------------------------------------------------------------------------------------
// The reference updates the memory of every node with a pending message on every call (get_updated_memories over range(num_nodes),
// MemoryModel.py:108-109) although a call only reads the rows of its level-0 set (roots and sampled neighbours).  Here the cell runs
// over exactly those: every level-0 slot names itself owner of its node (k_tgat_expand); the winning slot lists the node (the list blocks
// of chain::pack's launch): with a pending message for the cell's row-block kernel (tgat_chain.hip, memory_rnn.hip: gathers the listed rows,
// runs the gate products and scatters the new memory and feat0 = memory + raw), without one for the plain feat0 = memory + raw rows
// (MemoryModel.py:609) of the same launch.  Rows of a product do not depend on which other rows are in it, so every row read later is
// bit-identical to the all-nodes update.  That launch also packs the weights of the L layers, and of a GRU, into operand fragments (tgat_chain.h).
int tgn::memory_update(hipStream_t s, const dygnn_tgat_config& cfg, int L, const dygnn_tgat_weights* w, const Cell& cell, const TgatLevel0& l0, const Scratch& m,
                       const dygnn_tgn_state* st, const float* node_feat) {
    const int64_t N = st->num_nodes;
    const int Fn = cfg.node_feat_dim, Fe = cfg.edge_feat_dim, Ft = cfg.time_feat_dim, Dkv = Fn + Fe + Ft, Dm = 2 * Fn + Ft + Fe;
    const int gru_Dm = cell.gru ? Dm : 0;
    const chain::PackPlan pp = chain::plan_pack(L, Fn, Ft, Dkv, cfg.num_heads, gru_Dm);
    const chain::ListArgs la{l0.ids0, l0.live, m.owner, st->has_msg, m.pendf, m.count, m.list, m.count2, m.list2, l0.n1, N, cfg.num_neighbors};
    if (int rc = chain::pack(s, pp, L, Fn, Ft, Dkv, cfg.num_heads, w, cell.gru, gru_Dm, l0.pack, &la)) return rc;
    const int64_t ub = N < l0.n0 ? N : l0.n0;                  // the list cannot be longer than the level-0 set
    const chain::GruArgs ga{m.list, m.count, m.list2, m.count2, st->msg, st->memory, node_feat, cell.gru ? l0.pack : cell.pk, cell.gru ? pp.ih : cell.off_ih,
                            cell.gru ? pp.hh : cell.off_hh, cell.b_ih, cell.b_hh, m.Mnew, m.feat0, ub, Dm, Fn};
    return cell.run(s, ga);
}

struct TgnPlan { tgn::ScratchPlan mem; size_t tgat, total; };
static TgnPlan make_tgn_plan(const dygnn_tgat_config& c, int64_t N, int64_t B) {
    TgnPlan p{};
    Carve ws;
    p.mem = tgn::carve_scratch(ws, N, c.node_feat_dim, true);
    p.tgat = ws.take(tgat_plan_bytes(c, B));
    p.total = ws.o;
    return p;
}

// The memory-attention stage on the block `ws` of a TgnPlan for roots.B pairs: the levels of the roots (they depend on the graph only; sampled
// here, or the caller's pre-sampled `levels`: `uniform` / `time_interval_aware`, the caller replayed the sampler's RandomState,
// MemoryModel.py:626-629), whose level-0 set is what the call reads; the memory-update step over it; then the temporal graph attention
// over (memory + raw) features (GraphAttentionEmbedding, MemoryModel.py:548-664) into out_src / out_dst.  `who` prefixes the messages.
static int memory_attention(hipStream_t s, const char* who, const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const tgn::Cell& cell,
                            const dygnn_csr* csr, const dygnn_tgat_levels* levels, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st,
                            const TgatRoots& roots, const TgnPlan& p, char* ws, float* out_src, float* out_dst) {
    const tgn::Scratch m = tgn::scratch_at(ws, p.mem);
    if (int rc = check_tgat_args(cfg, w, csr, levels, m.feat0, edge_feat, roots, out_src, out_dst, ws + p.tgat, p.total - p.tgat)) return rc;
    DYGNN_REQUIRE(chain::fits(cfg->node_feat_dim, cfg->time_feat_dim, cfg->node_feat_dim + cfg->edge_feat_dim + cfg->time_feat_dim, cfg->num_heads),
                  "%s: feature dims do not fit the row-block kernels", who);
    const TgatStages c = tgat_stages(*cfg, roots.B, ws + p.tgat, s, levels != nullptr);
    const TgnTouch touch{m.owner, m.count, st->num_nodes};
    if (int rc = tgat_levels(c, csr, roots, levels, &touch)) return rc;
    if (int rc = tgn::memory_update(s, *cfg, cfg->num_layers, w, cell, tgat_level0(c), m, st, node_feat)) return rc;
    return tgat_layers(c, w, m.feat0, edge_feat, out_src, out_dst, true);
}

// The first n_pos pairs of the batch are positive edges (they update the state), the rest only read it.
static int tgn_forward_impl(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_gru_weights* gru, const dygnn_csr* csr,
                            const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st, const int64_t* src, const int64_t* dst,
                            const double* times, const int64_t* edge_ids, int64_t batch, int64_t n_pos, float* out_src,
                            float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream, const dygnn_tgat_levels* levels = nullptr) {
    const bool edges_are_positive = n_pos > 0;
    if (int rc = check_tgat(cfg)) return rc;
    DYGNN_REQUIRE(n_pos >= 0 && n_pos <= batch, "tgn: n_positive must be in [0, batch]");
    if (int rc = check_cell(gru, "tgn", "GRU weights")) return rc;
    if (int rc = check_state(st, "tgn")) return rc;
    DYGNN_REQUIRE(batch >= 0 && node_feat && edge_feat && workspace, "tgn: bad arguments");
    DYGNN_REQUIRE(!edges_are_positive || edge_ids != nullptr, "tgn: edge_ids required for positive edges");   // MemoryModel.py:140
    if (batch == 0) return DYGNN_OK;
    const TgnPlan p = make_tgn_plan(*cfg, st->num_nodes, batch);
    if (workspace_bytes < p.total) { set_error("tgn: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total); return DYGNN_E_WORKSPACE; }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    const tgn::Cell cell{gru, nullptr, 0, 0, gru->bias_ih, gru->bias_hh, chain::launch_gru};
    if (int rc = memory_attention(s, "tgn", cfg, w, cell, csr, levels, node_feat, edge_feat, st, TgatRoots{src, dst, times, batch, false}, p, ws, out_src, out_dst))
        return rc;
    if (!edges_are_positive) return DYGNN_OK;
    // persist the updated memories of the batch nodes and store their new raw messages (MemoryModel.py:142-161)
    const tgn::Scratch m = tgn::scratch_at(ws, p.mem);
    return tgn_commit(s, src, dst, times, edge_ids, n_pos, m.Mnew, m.pendf, st, edge_feat, w->time_w, w->time_b, cfg->node_feat_dim, cfg->edge_feat_dim,
                      cfg->time_feat_dim);
}

// ================================================================================================
// DyRep (reference models/MemoryModel.py with model_name == 'DyRep'): TGN's modules with nn.RNNCell in place of nn.GRUCell, and two twists
// on the data flow (:163-166, :225-227): a call RETURNS the updated memories of its roots, and in a positive call the attention embedding
// of the other endpoint of a pair takes the place of its memory in the new raw message.  So only the positive pairs need the attention:
//   1. chain::pack_rnn + k_rnn_rows (memory_rnn.hip) over all roots [src ; dst] of the batch, without the time projection: the returned
//      rows -- gathered from updated memory BEFORE the commit, which runs last -- and the per-root scratch of the commit.  A negative call
//      (n_positive = 0) ends here: its attention would be thrown away (the reference still computes it).
//   2. TGN's memory-attention stage on the first n_positive pairs: levels (sampled here, or the caller's), owner slots, list pass + layer
//      packing, k_rnn_list (the cell over the listed level-0 nodes, row count on the device) -> feat0 = updated memory + raw, the layers as
//      chains -> attention rows [2 n_positive][Fn] in the workspace.
//   3. chain::memory_commit with those rows as the "other endpoint" part of the messages.
// ================================================================================================
struct DyrepPlan { size_t tgn, rpk, upd, lu, pend, att, total; };
static DyrepPlan make_dyrep_plan(const dygnn_tgat_config& c, int64_t N, int64_t B) {
    DyrepPlan p{};
    Carve ws;
    const int Fn = c.node_feat_dim, Dm = 2 * Fn + c.time_feat_dim + c.edge_feat_dim;
    p.tgn = ws.take(make_tgn_plan(c, N, B).total);                  // room for every n_positive <= B
    p.rpk = ws.take(chain::pack_bytes(chain::plan_pack_rnn(Fn, Dm)));
    p.upd = ws.take((size_t)2 * B * Fn * sizeof(float));
    p.lu = ws.take((size_t)2 * B * sizeof(float));
    p.pend = ws.take((size_t)2 * B * sizeof(int32_t));
    p.att = ws.take((size_t)2 * B * Fn * sizeof(float));
    p.total = ws.o;
    return p;
}

static int dyrep_forward_impl(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_rnn_weights* rnn, const dygnn_csr* csr,
                              const dygnn_tgat_levels* levels, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st,
                              const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t batch, int64_t n_pos,
                              float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = check_tgat(cfg)) return rc;
    if (int rc = chain::check_rnn_dims("dyrep", cfg->node_feat_dim, cfg->edge_feat_dim, cfg->time_feat_dim)) return rc;
    DYGNN_REQUIRE(n_pos >= 0 && n_pos <= batch, "dyrep: n_positive must be in [0, batch]");
    if (int rc = check_cell(rnn, "dyrep", "RNN weights")) return rc;
    if (int rc = check_state(st, "dyrep")) return rc;
    DYGNN_REQUIRE(batch >= 0 && node_feat && edge_feat && workspace && w && w->time_w && w->time_b, "dyrep: bad arguments");
    DYGNN_REQUIRE(batch == 0 || (src && dst && times && out_src && out_dst), "dyrep: null pointer");
    DYGNN_REQUIRE(n_pos == 0 || edge_ids != nullptr, "dyrep: edge_ids required for positive edges");   // MemoryModel.py:140
    DYGNN_REQUIRE(batch == 0 || out_dst == out_src + (size_t)batch * cfg->node_feat_dim, "dyrep: out_dst must follow out_src (one [2, batch, dim] block)");
    if (batch == 0) return DYGNN_OK;
    const int64_t N = st->num_nodes;
    const int Fn = cfg->node_feat_dim, Fe = cfg->edge_feat_dim, Ft = cfg->time_feat_dim, Dm = 2 * Fn + Ft + Fe;
    const DyrepPlan p = make_dyrep_plan(*cfg, N, batch);
    if (workspace_bytes < p.total) { set_error("dyrep: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total); return DYGNN_E_WORKSPACE; }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    float* rpk = reinterpret_cast<float*>(ws + p.rpk);
    float* upd = reinterpret_cast<float*>(ws + p.upd);
    float* lu = reinterpret_cast<float*>(ws + p.lu);
    int32_t* pend = reinterpret_cast<int32_t*>(ws + p.pend);
    float* att_src = reinterpret_cast<float*>(ws + p.att);
    float* att_dst = att_src + (size_t)n_pos * Fn;
    // 1. the returned rows: the updated memories of the roots, before anything is committed
    const chain::RnnPackPlan rp = chain::plan_pack_rnn(Fn, Dm);
    if (int rc = chain::pack_rnn(s, rp, Fn, Dm, rnn, rpk)) return rc;
    chain::RnnRowArgs ra{src, dst, times, batch, N, st->msg, st->memory, st->last_update, st->msg_time, st->has_msg, rpk, rp.ih, rp.hh,
                         rnn->bias_ih, rnn->bias_hh, nullptr, nullptr, {0.f, 0.f}, {1.f, 1.f}, out_src, upd, lu, pend, Dm, Fn};
    if (int rc = chain::launch_rnn_rows(s, ra)) return rc;
    if (n_pos == 0) return DYGNN_OK;
    // 2. the attention embeddings of the positive pairs, over updated memory + raw features (TGN's stage with the RNN cell)
    const tgn::Cell cell{nullptr, rpk, rp.ih, rp.hh, rnn->bias_ih, rnn->bias_hh, chain::launch_rnn_list};
    if (int rc = memory_attention(s, "dyrep", cfg, w, cell, csr, levels, node_feat, edge_feat, st, TgatRoots{src, dst, times, n_pos, false},
                                  make_tgn_plan(*cfg, N, n_pos), ws + p.tgn, att_src, att_dst)) return rc;
    // 3. persist and store: the other endpoint's part of a message is its attention row (MemoryModel.py:225-227)
    return chain::memory_commit(s, src, dst, times, edge_ids, n_pos, batch, upd, lu, pend, att_src, att_dst, st, edge_feat, w->time_w, w->time_b, Fn, Fe, Ft);
}

}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_tgn_workspace_bytes(const dygnn_tgat_config* cfg, int64_t num_nodes, int64_t batch) {
    if (check_tgat(cfg) != DYGNN_OK || batch < 0 || num_nodes < 1) return 0;
    return make_tgn_plan(*cfg, num_nodes, batch).total;
}

extern "C" int dygnn_tgn_forward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_gru_weights* gru, const dygnn_csr* csr,
                                 const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st, const int64_t* src, const int64_t* dst,
                                 const double* times, const int64_t* edge_ids, int64_t batch, int32_t edges_are_positive, float* out_src,
                                 float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    return tgn_forward_impl(cfg, w, gru, csr, node_feat, edge_feat, st, src, dst, times, edge_ids, batch, edges_are_positive ? batch : 0, out_src, out_dst,
                            workspace, workspace_bytes, stream);
}

// dygnn_tgn_forward_step on PRE-SAMPLED levels: the reference accepts any sampling strategy for TGN (MemoryModel.py:626-629); `uniform` and
// `time_interval_aware` draw from the sampler's numpy RandomState, which the host mirror replays in the reference's order (one call on
// [src ; dst], MemoryModel.py:104-131) and hands over as level arrays in dygnn_tgat_forward_levels' layout.  src / dst / times are still read:
// by the commit of a positive call (messages, last-update times).
extern "C" int dygnn_tgn_forward_levels(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_gru_weights* gru,
                                        const dygnn_tgat_levels* levels, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st,
                                        const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t batch,
                                        int64_t n_positive, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    DYGNN_REQUIRE(levels != nullptr, "tgn_forward_levels: levels is NULL");
    DYGNN_REQUIRE(n_positive == 0 || (src && dst && times), "tgn_forward_levels: a positive call needs src / dst / times");
    return tgn_forward_impl(cfg, w, gru, nullptr, node_feat, edge_feat, st, src, dst, times, edge_ids, batch, n_positive, out_src, out_dst, workspace,
                            workspace_bytes, stream, levels);
}

extern "C" int dygnn_tgn_forward_step(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_gru_weights* gru, const dygnn_csr* csr,
                                      const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st, const int64_t* src, const int64_t* dst,
                                      const double* times, const int64_t* edge_ids, int64_t batch, int64_t n_positive, float* out_src,
                                      float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    return tgn_forward_impl(cfg, w, gru, csr, node_feat, edge_feat, st, src, dst, times, edge_ids, batch, n_positive, out_src, out_dst, workspace,
                            workspace_bytes, stream);
}

extern "C" size_t dygnn_dyrep_workspace_bytes(const dygnn_tgat_config* cfg, int64_t num_nodes, int64_t batch) {
    if (check_tgat(cfg) != DYGNN_OK || batch < 0 || num_nodes < 1) return 0;
    if (chain::check_rnn_dims("dyrep", cfg->node_feat_dim, cfg->edge_feat_dim, cfg->time_feat_dim) != DYGNN_OK) return 0;
    return make_dyrep_plan(*cfg, num_nodes, batch).total;
}

extern "C" int dygnn_dyrep_forward_step(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_rnn_weights* rnn, const dygnn_csr* csr,
                                        const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st, const int64_t* src, const int64_t* dst,
                                        const double* times, const int64_t* edge_ids, int64_t batch, int64_t n_positive, float* out_src,
                                        float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    return dyrep_forward_impl(cfg, w, rnn, csr, nullptr, node_feat, edge_feat, st, src, dst, times, edge_ids, batch, n_positive, out_src, out_dst, workspace,
                              workspace_bytes, stream);
}

// dygnn_dyrep_forward_step on PRE-SAMPLED levels of the first n_positive pairs (dygnn_tgn_forward_levels' layout with batch = n_positive;
// not read when n_positive = 0)
extern "C" int dygnn_dyrep_forward_levels(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_rnn_weights* rnn,
                                          const dygnn_tgat_levels* levels, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st,
                                          const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t batch,
                                          int64_t n_positive, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    DYGNN_REQUIRE(n_positive <= 0 || levels != nullptr, "dyrep_forward_levels: levels is NULL");
    return dyrep_forward_impl(cfg, w, rnn, nullptr, levels, node_feat, edge_feat, st, src, dst, times, edge_ids, batch, n_positive, out_src, out_dst, workspace,
                              workspace_bytes, stream);
}
