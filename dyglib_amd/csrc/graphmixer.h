// What the GraphMixer training path (graphmixer_train.hip) shares with the inference forward (graphmixer.hip): the constants, the CSR view
// and history search, the configuration check and the launches of the two kernels both paths run as they are.
#pragma once
#include "common.h"

namespace dygnn {
namespace gm {

constexpr int kMaxTokens = 32;
constexpr float kLnEps = 1e-5f;

struct Csr {
    const int64_t* indptr;
    const int32_t* nbr;
    const int32_t* eid;
    const double* ts;
    int64_t num_nodes;
};

// the strictly-earlier prefix [lo, end) of the root's CSR row; an id outside the graph has the empty row 0 (as query_row, sampler.hip)
__device__ __forceinline__ void history(const Csr& g, int64_t node, double t, int lane, int64_t& lo, int64_t& end) {
    if (node < 0 || node >= g.num_nodes) node = 0;
    lo = g.indptr[node];
    end = wave_lower_bound(g.ts, lo, g.indptr[node + 1], t, lane);
}

// DYGNN_OK, or why the configuration is refused (message in dygnn_last_error)
int check_graphmixer(const dygnn_graphmixer_config* c);
// k_gm_node over n roots: term [n][Fn], the node encoder's windowed row mean BEFORE node_feat[v] is added
int node_term(hipStream_t s, const Csr& g, const float* node_feat, const int64_t* nodes, const double* times, int64_t n, int Fn, int G, float* term);
// k_gm_proj over n roots: X [n K][C] = projection_layer([edge row | cos(w dt + b)]) of the K sampled tokens
int project(hipStream_t s, const Csr& g, const float* edge_feat, const int64_t* nodes, const double* times, int64_t n, const dygnn_graphmixer_weights& w,
            int K, int C, int Ft, float* X);

}  // namespace gm
}  // namespace dygnn
