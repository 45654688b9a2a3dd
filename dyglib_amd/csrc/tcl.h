// What the TCL training path (tcl_train.hip) shares with the inference forward (tcl.hip): the configuration check and the encoder input.
#pragma once
#include "common.h"

namespace dygnn {
namespace tcl {

// DYGNN_OK, or why the configuration is refused (message in dygnn_last_error)
int check_tcl(const dygnn_tcl_config* c);
// k_tcl_encode over N sides: X0 [N][S][d] = proj_node(node rows) + proj_edge(edge rows) + proj_time(cos(dt w + b)) + depth embedding
int encode(hipStream_t s, const dygnn_tcl_config& c, const dygnn_tcl_weights& w, const float* node_feat, const float* edge_feat, const int64_t* side_root,
           const double* side_time, const int64_t* nbr_id, const int64_t* nbr_eid, const float* nbr_t, int64_t N, float* X0);

}  // namespace tcl
}  // namespace dygnn
