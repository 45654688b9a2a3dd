// TGN training (SURVEY.md §8f-1 for BASELINE config 5): models/MemoryModel.py:87-168 in TRAIN mode and the backward pass of one call, so that
// train_link_prediction.py:186-207, :242-264 (negative call, positive call, MergeLayer + BCE, loss.backward(), Adam, detach_memory_bank) runs
// on the HIP path.
//
// What a call's loss differentiates:
//   * the updated memories, GRUCell(last message, stored memory) of the nodes with a pending message.  Message and stored memory are constants
//     (MemoryModel.py:374-387 detaches them; :461-487 reads the memory through .data), so this step gives a gradient to the four GRUCell
//     tensors only;
//   * TGAT's layers over feat0 = updated memory + raw features (:598, :662): the training stages of tgat_train.hip, whose backward pass here
//     also sums the gradient of the level-0 rows per node id (tgt::Feat0Grad, float atomics), for the nodes with a pending message;
//   * nothing else: the state commit of a positive call feeds no loss of this batch and the next batch starts from detached state.
// Forward: levels -> owner slots / node lists / GRU (the INFERENCE kernels: chain::pack's list pass, k_tgn_gru_chain) -> copy of the listed
// nodes' message and memory rows into the workspace -> train-mode layers on feat0 -> k_tgn_commit for the positive pairs.  The committed
// memories are the inference kernel's, so the memory bank after a training call equals the one after the inference call bit for bit.
// Backward: layers (d feat0 rows by atomics) -> gate pre-activations recomputed from the saved rows (two GEMMs) -> gate derivatives (one
// kernel) -> dW_ih, dW_hh, db_ih, db_hh (one grouped split-K launch).  It reads nothing of dygnn_tgn_state: a positive call has overwritten
// the memory, message and flag of its batch nodes by then, and the negative call's backward runs after the positive call's commit.
#include "common.h"
#include "gemm.h"
#include "tgat_chain.h"
#include "tgat_train.h"
#include "tgn.h"

namespace dygnn {
namespace tgn {

// meta words of a call (device): the two list lengths of the list pass
enum { kCount = 0, kCount2 = 1 };

// Rows r < count of the pending list: pos[node] = r and the node's message and stored memory rows are copied (the commit overwrites them
// before the backward pass runs); rows beyond: zeros (they enter the weight-gradient products as K rows).  Rows r < count2 of the other list:
// pos[node] = -1.  One workgroup per row.
__global__ __launch_bounds__(256) void k_tgn_save(const int32_t* __restrict__ list, const int32_t* __restrict__ list2, const int32_t* __restrict__ meta,
                                                    const float* __restrict__ msg, const float* __restrict__ M, int Dm, int Fn, int32_t N, int64_t rows,
                                                    int32_t* __restrict__ pos, float* __restrict__ msgs, float* __restrict__ hold) {
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int32_t node = r < meta[kCount] ? list[r] : -1;
    const bool live = node >= 0 && node < N;
    if (live && threadIdx.x == 0) pos[node] = (int32_t)r;
    if (r < meta[kCount2] && threadIdx.x == 1) {
        const int32_t other = list2[r];
        if (other >= 0 && other < N) pos[other] = -1;
    }
    for (int f = threadIdx.x; f < Dm; f += blockDim.x) msgs[r * Dm + f] = live ? msg[(size_t)node * Dm + f] : 0.f;
    for (int f = threadIdx.x; f < Fn; f += blockDim.x) hold[r * Fn + f] = live ? M[(size_t)node * Fn + f] : 0.f;
}

// nn.GRUCell backward of the listed rows, gate order r | z | n: with gi = W_ih x + b_ih, gh = W_hh h + b_hh [rows][3F],
//   r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h
// and dh' the gradient of the updated memory row:
//   dn = dh' (1 - z) (1 - n^2) ; dz = dh' (h - n) z (1 - z) ; dr = dn gh_n r (1 - r)
//   dgi = [dr | dz | dn], dgh = [dr | dz | dn r], written over gi / gh.  x and h are constants: no dx, no dh.
// Rows beyond the list: zeros.  One thread per (row, memory dim).
__global__ __launch_bounds__(256) void k_tgn_gru_bwd(const int32_t* __restrict__ meta, const float* __restrict__ dh, const float* __restrict__ hold, int F,
                                                       int64_t rows, float* __restrict__ gi, float* __restrict__ gh) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * F) return;
    const int64_t row = e / F;
    const int f = (int)(e - row * F);
    float* a = gi + row * 3 * F;
    float* b = gh + row * 3 * F;
    float dr = 0.f, dz = 0.f, dn = 0.f, dnr = 0.f;
    if (row < meta[kCount]) {
        const float r = 1.0f / (1.0f + expf(-(a[f] + b[f])));
        const float z = 1.0f / (1.0f + expf(-(a[F + f] + b[F + f])));
        const float hn = b[2 * F + f];
        const float n = tanhf(fmaf(r, hn, a[2 * F + f]));
        const float g = dh[e];
        dn = g * (1.0f - z) * (1.0f - n * n);
        dz = g * (hold[e] - n) * z * (1.0f - z);
        dr = dn * hn * r * (1.0f - r);
        dnr = dn * r;
    }
    a[f] = dr; a[F + f] = dz; a[2 * F + f] = dn;
    b[f] = dr; b[F + f] = dz; b[2 * F + f] = dnr;
}

// The layers' block, the meta words, the saved rows and the GRU backward's buffers (`rows` = min(N, the level-0 set's size) bounds the pending
// list) and pos [N]; then what only the forward call uses: the per-node scratch (its two counters are the meta words) and the GRU's fragments.
struct Plan {
    int Fn, Dm;
    int64_t rows;
    size_t tgat, meta, msgs, hold, dfeat, gi, gh, pos;
    ScratchPlan mem;
    size_t pack, total;
};

static Plan make_plan(const dygnn_tgat_config& c, int64_t N, int64_t B) {
    Plan p{};
    p.Fn = c.node_feat_dim;
    p.Dm = 2 * c.node_feat_dim + c.time_feat_dim + c.edge_feat_dim;
    int64_t n0 = 2 * B;
    for (int l = 0; l < c.num_layers; ++l) n0 *= 1 + c.num_neighbors;
    p.rows = N < n0 ? N : n0;
    Carve ws;
    p.tgat = ws.take(tgt::train_plan_bytes(c, B));
    p.meta = ws.take(4 * sizeof(int32_t));
    p.msgs = ws.take((size_t)p.rows * p.Dm * sizeof(float));
    p.hold = ws.take((size_t)p.rows * p.Fn * sizeof(float));
    p.dfeat = ws.take((size_t)p.rows * p.Fn * sizeof(float));
    p.gi = ws.take((size_t)p.rows * 3 * p.Fn * sizeof(float));
    p.gh = ws.take((size_t)p.rows * 3 * p.Fn * sizeof(float));
    p.pos = ws.take((size_t)N * sizeof(int32_t));
    p.mem = carve_scratch(ws, N, p.Fn, false);
    p.mem.count = p.meta + kCount * sizeof(int32_t);
    p.pack = ws.take(chain::pack_bytes(chain::plan_pack(0, c.node_feat_dim, c.time_feat_dim, c.node_feat_dim + c.edge_feat_dim + c.time_feat_dim, c.num_heads, p.Dm)));
    p.total = ws.o;
    return p;
}

// the configurations dygnn_tgn_forward_step and dygnn_tgat_train_forward both take
static int check_cfg(const dygnn_tgat_config* cfg) {
    if (int rc = check_tgat(cfg)) return rc;
    if (!chain::fits(cfg->node_feat_dim, cfg->time_feat_dim, cfg->node_feat_dim + cfg->edge_feat_dim + cfg->time_feat_dim, cfg->num_heads)) {
        set_error("tgn: feature dims do not fit the row-block kernels");
        return DYGNN_E_UNSUPPORTED;
    }
    return DYGNN_OK;
}

}  // namespace tgn
}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_tgn_train_workspace_bytes(const dygnn_tgat_config* cfg, int64_t num_nodes, int64_t batch) {
    if (tgn::check_cfg(cfg) != DYGNN_OK || batch < 1 || num_nodes < 1 || num_nodes > INT32_MAX) return 0;
    return tgn::make_plan(*cfg, num_nodes, batch).total;
}

extern "C" int dygnn_tgn_train_forward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_gru_weights* gru, const dygnn_csr* csr,
                                       const dygnn_tgat_levels* levels, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* st,
                                       const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t batch,
                                       int64_t n_pos, float dropout_p, uint64_t seed, float* out_src, float* out_dst, void* workspace,
                                       size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = tgn::check_cfg(cfg)) return rc;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && node_feat && edge_feat, "tgn_train_forward: null pointer");
    DYGNN_REQUIRE(batch > 0 && out_src && out_dst && workspace, "tgn_train_forward: bad arguments");
    DYGNN_REQUIRE(n_pos >= 0 && n_pos <= batch, "tgn_train_forward: n_positive must be in [0, batch]");
    if (int rc = check_cell(gru, "tgn_train_forward", "GRU weights")) return rc;
    if (int rc = check_state(st, "tgn_train_forward", INT32_MAX)) return rc;
    DYGNN_REQUIRE(n_pos == 0 || edge_ids != nullptr, "tgn_train_forward: edge_ids required for positive edges");      // MemoryModel.py:140
    DYGNN_REQUIRE(levels ? (n_pos == 0 || (src && dst && times)) : (csr && csr->indptr && csr->num_nodes >= 1 && src && dst && times),
                  "tgn_train_forward: need csr + src / dst / times (with levels: for a positive call)");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "tgn_train_forward: dropout must be in [0, 1)");
    const int64_t N = st->num_nodes;
    const tgn::Plan p = tgn::make_plan(*cfg, N, batch);
    if (workspace_bytes < p.total) { set_error("tgn_train_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total); return DYGNN_E_WORKSPACE; }
    if (int rc = check_layer_weights(w, cfg->num_layers, "tgn_train_forward: null layer weights")) return rc;
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    const int Fn = cfg->node_feat_dim, Fe = cfg->edge_feat_dim, Ft = cfg->time_feat_dim;
    int32_t* meta = I32(p.meta);
    const tgn::Scratch m = tgn::scratch_at(ws, p.mem);
    // 0. the levels of this call; every slot of their level-0 set names itself owner of its node
    if (int rc = tgt::train_levels(s, *cfg, csr, levels, src, dst, times, batch, ws + p.tgat, "tgn_train_forward")) return rc;
    const tgt::TrainLevel0 l0 = tgt::train_level0(*cfg, batch, ws + p.tgat);
    if (int rc = tgn_touch_levels(s, l0.ids0, l0.n1, cfg->num_neighbors, TgnTouch{m.owner, meta, N})) return rc;
    // 1. the inference path's memory-update step, no layers packed (the training levels are not de-duplicated: no live count): Mnew (what a
    //    positive call commits) and feat0 = updated memory + raw for the call's nodes
    const tgn::Cell cell{gru, nullptr, 0, 0, gru->bias_ih, gru->bias_hh, chain::launch_gru};
    if (int rc = tgn::memory_update(s, *cfg, 0, w, cell, TgatLevel0{l0.ids0, nullptr, l0.n0, l0.n1, F32(p.pack)}, m, st, node_feat)) return rc;
    // 2. what the GRU backward needs of the state, before the commit below (or a later call's) overwrites it
    hipLaunchKernelGGL(tgn::k_tgn_save, dim3((unsigned)p.rows), dim3(256), 0, s, m.list, m.list2, meta, st->msg, st->memory, p.Dm, Fn, (int32_t)N, p.rows,
                       I32(p.pos), F32(p.msgs), F32(p.hold));
    DYGNN_LAUNCH_CHECK();
    // 3. the train-mode layers over feat0 (GraphAttentionEmbedding, MemoryModel.py:548-664)
    if (int rc = tgt::train_forward(s, *cfg, w, m.feat0, edge_feat, batch, dropout_p, seed, out_src, out_dst, ws + p.tgat)) return rc;
    if (n_pos == 0) return DYGNN_OK;
    // 4. persist the updated memories of the positive pairs' nodes and store their new raw messages (MemoryModel.py:142-161)
    return tgn_commit(s, src, dst, times, edge_ids, n_pos, m.Mnew, m.pendf, st, edge_feat, w->time_w, w->time_b, Fn, Fe, Ft);
}

extern "C" int dygnn_tgn_backward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_gru_weights* gru, const dygnn_tgat_weights* grads,
                                  const dygnn_gru_grads* gg, const float* grad_out_src, const float* grad_out_dst, int64_t num_nodes, int64_t batch,
                                  float dropout_p, uint64_t seed, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = tgn::check_cfg(cfg)) return rc;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && grads && grads->time_w && grads->time_b && grad_out_src && grad_out_dst && workspace && batch > 0,
                  "tgn_backward: bad arguments");
    if (int rc = check_cell(gru, "tgn_backward", "GRU weights")) return rc;
    if (int rc = check_cell(gg, "tgn_backward", "GRU gradient buffer")) return rc;
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "tgn_backward: dropout must be in [0, 1)");
    DYGNN_REQUIRE(num_nodes >= 1 && num_nodes <= INT32_MAX, "tgn_backward: bad num_nodes");
    const tgn::Plan p = tgn::make_plan(*cfg, num_nodes, batch);
    if (workspace_bytes < p.total) { set_error("tgn_backward: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total); return DYGNN_E_WORKSPACE; }
    if (int rc = check_layer_weights(w, cfg->num_layers, "tgn_backward: null layer weights")) return rc;
    if (int rc = check_layer_weights(grads, cfg->num_layers, "tgn_backward: null gradient buffer")) return rc;
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int32_t* meta = reinterpret_cast<const int32_t*>(ws + p.meta);
    const int F = p.Fn, Dm = p.Dm, rows = (int)p.rows;
    // 1. the layers; d feat0 rows of the nodes with a pending message, summed over every place that read them
    DYGNN_HIP(hipMemsetAsync(F32(p.dfeat), 0, (size_t)p.rows * F * sizeof(float), s));
    const tgt::Feat0Grad fg{F32(p.dfeat), reinterpret_cast<const int32_t*>(ws + p.pos), num_nodes};
    if (int rc = tgt::train_backward(s, *cfg, w, grads, grad_out_src, grad_out_dst, batch, dropout_p, seed, ws + p.tgat, &fg)) return rc;
    // 2. GRU cell: gate pre-activations of the listed rows again (the saved message / memory rows, the current weights), their derivatives,
    //    then the four parameter gradients.  d(updated memory) = d feat0 (feat0 = memory + raw).
    if (int rc = train::mm(s, F32(p.msgs), Dm, false, gru->weight_ih, Dm, true, F32(p.gi), 3 * F, rows, 3 * F, Dm,
                           train::MmOpt().bias(gru->bias_ih).live_rows(meta + tgn::kCount))) return rc;
    if (int rc = train::mm(s, F32(p.hold), F, false, gru->weight_hh, F, true, F32(p.gh), 3 * F, rows, 3 * F, F,
                           train::MmOpt().bias(gru->bias_hh).live_rows(meta + tgn::kCount))) return rc;
    hipLaunchKernelGGL(tgn::k_tgn_gru_bwd, dim3((unsigned)ceil_div(p.rows * F, 256)), dim3(256), 0, s, meta, F32(p.dfeat), F32(p.hold), F, p.rows, F32(p.gi), F32(p.gh));
    DYGNN_LAUNCH_CHECK();
    const train::DwPair pairs[2] = {{F32(p.gi), 3 * F, 3 * F, F32(p.msgs), Dm, Dm, gg->weight_ih, Dm, gg->bias_ih},
                                    {F32(p.gh), 3 * F, 3 * F, F32(p.hold), F, F, gg->weight_hh, F, gg->bias_hh}};
    return train::dw_grouped(s, rows, pairs, 2);
}
