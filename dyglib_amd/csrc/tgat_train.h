// The training stages of the TGAT layer stack (tgat_train.hip), shared by TGAT training and TGN training (tgn_train.hip): the level sets of
// a call, the train-mode forward over them and its backward pass, all on ONE workspace block of train_plan_bytes() bytes.
#pragma once
#include "common.h"

namespace dygnn {
namespace tgt {

// TGN only: where the gradient of the level-0 feature rows goes.  TGAT's level 0 is the constant node feature table; TGN's is
// feat0 = updated memory + raw features (MemoryModel.py:598), read as layer-1 query rows, as layer-1 key / value rows and as the second
// input of every layer's MergeLayer (:662), the same node from many places: its gradient is the SUM over all occurrences of the node id.
// Only nodes with a pending message pass the gradient on (to the GRU cell; memory and raw features are constants), so only their rows are
// kept: d [rows][Fn], row pos[node] (-1: the node has no pending message), summed with float atomics (zeroed by the caller).
struct Feat0Grad {
    float* d;
    const int32_t* pos;             // [N]: valid for every node of the call's level-0 set
    int64_t N;
};

size_t train_plan_bytes(const dygnn_tgat_config& cfg, int64_t batch);
// the call's level-0 ids [n1 entries | n1 * k neighbours] inside its workspace (n0 = n1 (1 + k))
struct TrainLevel0 { const int32_t* ids0; int64_t n0, n1; };
TrainLevel0 train_level0(const dygnn_tgat_config& cfg, int64_t batch, void* workspace);
// Levels: sampled here (`recent`, levels == NULL) or copied from the caller's host-replayed draws.  `what` prefixes the error messages.
int train_levels(hipStream_t s, const dygnn_tgat_config& cfg, const dygnn_csr* csr, const dygnn_tgat_levels* levels, const int64_t* src, const int64_t* dst,
                 const double* times, int64_t batch, void* workspace, const char* what);
// The layers over the levels built by train_levels.  node_feat = the level-0 feature table (TGN: feat0); it and edge_feat are read again
// by train_backward.
int train_forward(hipStream_t s, const dygnn_tgat_config& cfg, const dygnn_tgat_weights* w, const float* node_feat, const float* edge_feat, int64_t batch,
                  float dropout_p, uint64_t seed, float* out_src, float* out_dst, void* workspace);
// feat0 == NULL: level 0 is constant (TGAT)
int train_backward(hipStream_t s, const dygnn_tgat_config& cfg, const dygnn_tgat_weights* w, const dygnn_tgat_weights* grads, const float* grad_out_src,
                   const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed, void* workspace, const Feat0Grad* feat0);

}  // namespace tgt
}  // namespace dygnn
