// nn.RNNCell memory update of the JODIE / DyRep arms of the reference MemoryModel (memory_rnn.hip): the one-gate siblings of the GRU
// row-block kernel (tgat_chain.h), in two forms -- one row per ROOT of a call (JODIE's rows; DyRep's returned rows) and one row per
// LISTED node with the row count read on the device (DyRep's updated memories under the attention, TGN's list pass: the cell of
// tgn::memory_update, tgn.h) -- and the commit of the positive pairs from the per-root scratch.  DyRep's entry points: tgn.hip.
#pragma once
#include "tgat_chain.h"

namespace dygnn {
namespace chain {

// whether a four-row block of these dims fits the LDS; otherwise DYGNN_E_UNSUPPORTED with the value in the message (`who` prefixes it)
int check_rnn_dims(const char* who, int Fn, int Fe, int Ft);

struct RnnRowArgs {
    const int64_t *src, *dst;      // [B] each: row r < B is src[r], row B + i is dst[i]
    const double* times;           // [B]
    int64_t B, N;
    const float *msg, *M, *U;      // state: pending message [N][Dm], memory [N][Fn], last update [N]
    const double* msg_t;
    const int32_t* has_msg;
    const float* pk;               // pack_rnn's fragments
    uint32_t off_ih, off_hh;
    const float *b_ih, *b_hh;
    const float *proj_w, *proj_b;  // JODIE's time projection, embedding_module.linear_layer; NULL (DyRep): the row is the updated memory itself
    float mean[2], stdv[2];        // [0] source rows, [1] destination rows
    float* out;                    // [2B][Fn] embeddings
    float* upd;                    // [2B][Fn] updated memory of the row's node
    float* lu;                     // [2B]     its last-update time after the update
    int32_t* pend;                 // [2B]     whether it had a pending message
    int Dm, Fn;
};
int launch_rnn_rows(hipStream_t s, const RnnRowArgs& a);

// The list form: GruArgs' meaning (row r = node list[r], r < *count <= max_rows, Mnew / feat0 scattered, list2's plain rows in the same
// launch) with nn.RNNCell in place of nn.GRUCell; a.pk = pack_rnn's fragments.
int launch_rnn_list(hipStream_t s, const GruArgs& a);

// End of a positive call: persists updated memories / last-update times of the first n_pos pairs' nodes and stores their new raw messages, from
// the per-root scratch of launch_rnn_rows (rows i and B + i).  other_src / other_dst [n_pos][Fn] (DyRep; NULL for JODIE): the "other
// endpoint" part of a source's message is other_dst[i], of a destination's other_src[i], instead of the other endpoint's updated memory.
int memory_commit(hipStream_t s, const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t n_pos, int64_t B,
                  const float* upd, const float* lu, const int32_t* pend, const float* other_src, const float* other_dst, const dygnn_tgn_state* st,
                  const float* edge_feat, const float* tw, const float* tb, int Fn, int Fe, int Ft);

}  // namespace chain
}  // namespace dygnn
