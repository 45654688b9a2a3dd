// What the memory models (TGN, DyRep, JODIE; tgn.hip, tgn_train.hip, memory_rnn.hip) share: the argument checks of cell and state, TGN's owner
// slots of a level-0 set, the per-node scratch of a call, the memory-update step over the listed level-0 nodes and the commit of a positive call.
#pragma once
#include "common.h"
#include "tgat_chain.h"
#include "tgat_stages.h"

namespace dygnn {

// dygnn_gru_weights / dygnn_rnn_weights / dygnn_gru_grads: "<who>: null <what>"
template <class W>
int check_cell(const W* c, const char* who, const char* what) {
    DYGNN_REQUIRE(c && c->weight_ih && c->weight_hh && c->bias_ih && c->bias_hh, "%s: null %s", who, what);
    return DYGNN_OK;
}
inline int check_state(const dygnn_tgn_state* st, const char* who, int64_t max_nodes = INT64_MAX) {
    DYGNN_REQUIRE(st && st->memory && st->last_update && st->msg && st->msg_time && st->has_msg && st->num_nodes >= 1 && st->num_nodes <= max_nodes,
                  "%s: bad state", who);
    return DYGNN_OK;
}

// TGN's owner slots of level 0 (tgat.hip: k_tgat_expand; tgn.hip: k_tgn_touch_levels)
struct TgnTouch {
    int32_t* owner;                // [N]; entries of nodes outside this call's level-0 set are stale and never read
    int32_t* counts;               // the two list lengths, zeroed here for the list pass of the next launch
    int64_t N;
};

// TGN on levels that are already in place (ids0 = [n1 entries | n1 * k neighbours]): every level-0 slot names itself owner of its node and the
// two list counters are zeroed, as expand_levels' `touch` does while it samples (the inference path on pre-sampled levels; the training path)
int tgn_touch_levels(hipStream_t s, const int32_t* ids0, int64_t n1, int k, const TgnTouch& touch);
// End of a positive TGN call (k_tgn_commit): persist the updated memories Mnew of the first n_pos pairs' nodes where pendf says they had a
// pending message, and store their new raw messages.  ONE implementation for inference and training: the state a call leaves is the same bits.
int tgn_commit(hipStream_t s, const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t n_pos, const float* Mnew,
               const int32_t* pendf, const dygnn_tgn_state* st, const float* edge_feat, const float* tw, const float* tb, int Fn, int Fe, int Ft);

namespace tgn {

// The per-node scratch of a call: updated memory and feat0 = memory + raw [N][Fn]; the level-0 slot that speaks for a node and whether the node
// had a pending message [N]; the nodes with (list) and without (list2) a pending message [N] and the two list lengths (adjacent words)
struct Scratch {
    float *Mnew, *feat0;
    int32_t *owner, *pendf, *count, *count2, *list, *list2;
};
struct ScratchPlan { size_t Mnew, feat0, owner, pendf, count, list, list2; };      // byte offsets
// own_counts = false: the caller keeps the two counters elsewhere and sets `count` itself
inline ScratchPlan carve_scratch(Carve& c, int64_t N, int Fn, bool own_counts) {
    ScratchPlan p{};
    p.Mnew = c.take((size_t)N * Fn * sizeof(float));
    p.feat0 = c.take((size_t)N * Fn * sizeof(float));
    p.owner = c.take((size_t)N * sizeof(int32_t));
    p.pendf = c.take((size_t)N * sizeof(int32_t));
    if (own_counts) p.count = c.take(2 * sizeof(int32_t));
    p.list = c.take((size_t)N * sizeof(int32_t));
    p.list2 = c.take((size_t)N * sizeof(int32_t));
    return p;
}
inline Scratch scratch_at(void* workspace, const ScratchPlan& p) {
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    return Scratch{F32(p.Mnew), F32(p.feat0), I32(p.owner), I32(p.pendf), I32(p.count), I32(p.count) + 1, I32(p.list), I32(p.list2)};
}

// The memory cell of a model.  nn.GRUCell (TGN): `gru` given, its weights are packed inside chain::pack's launch, behind the layers', and
// pk / off_ih / off_hh are filled in by memory_update.  nn.RNNCell (DyRep): packed beforehand by chain::pack_rnn into pk.
struct Cell {
    const dygnn_gru_weights* gru;
    const float* pk;               // packed fragments
    uint32_t off_ih, off_hh;
    const float *b_ih, *b_hh;
    int (*run)(hipStream_t, const chain::GruArgs&);      // the list kernel: chain::launch_gru or chain::launch_rnn_list
};

// The memory-update step of a call whose level-0 set is in place and whose owner slots are named (tgn.hip): the list pass, in the launch that
// packs the weights of L layers (training: 0) and of a GRU, then the cell over the listed nodes: m.Mnew and m.feat0 of every node the call reads.
int memory_update(hipStream_t s, const dygnn_tgat_config& cfg, int L, const dygnn_tgat_weights* w, const Cell& cell, const TgatLevel0& l0, const Scratch& m,
                  const dygnn_tgn_state* st, const float* node_feat);

}  // namespace tgn
}  // namespace dygnn
