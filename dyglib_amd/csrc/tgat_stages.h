// The inference stages of the TGAT layer stack (tgat.hip), shared by TGAT inference and the memory models on top of it (tgn.hip): the argument
// checks, the level sets of a call and the layers over them, all on ONE workspace block of tgat_plan_bytes() bytes.  The inference sibling of
// tgat_train.h.
#pragma once
#include "common.h"
#include "tgat_levels.h"

namespace dygnn {

size_t tgat_plan_bytes(const dygnn_tgat_config& cfg, int64_t batch);

// The argument checks of a TGAT / TGN inference call.  `levels` given: the caller's pre-sampled levels (copy_levels checks them), csr and the
// roots are not read.
int check_tgat_args(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_csr* csr, const dygnn_tgat_levels* levels, const float* node_feat,
                    const float* edge_feat, const TgatRoots& r, const float* out_src, const float* out_dst, const void* workspace, size_t workspace_bytes);

// What the level stage and the layer stage of one call share
struct TgatStages {
    const dygnn_tgat_config& cfg;
    int64_t B;
    char* ws;             // the call's workspace block
    hipStream_t s;
    bool dedup;           // level 1 is computed on its distinct entries: decided once per library call, by tgat_stages()
};
TgatStages tgat_stages(const dygnn_tgat_config& cfg, int64_t batch, void* workspace, hipStream_t s, bool presampled);

// Level stage: the level arrays of the call in its workspace, sampled from the graph (`recent`) or copied from the caller's `levels`.
// touch (TGN): every level-0 slot names itself owner of its node.
int tgat_levels(const TgatStages& c, const dygnn_csr* csr, const TgatRoots& roots, const dygnn_tgat_levels* levels, const TgnTouch* touch);

// What a memory model reads of the levels: the level-0 ids [n1 entries | n1 * k neighbours] (n0 = n1 (1 + k)); the device-side count of the
// level-1 entries in use when level 1 is de-duplicated, else NULL; the call's block of packed weight fragments (tgat_chain.h)
struct TgatLevel0 {
    const int32_t* ids0;
    const int32_t* live;
    int64_t n0, n1;
    float* pack;
};
TgatLevel0 tgat_level0(const TgatStages& c);

// Layer stage: layers 1..L, bottom-up, on the levels in the workspace, into out_src / out_dst.  packed (TGN): the caller has packed the layer
// weights into the workspace's row-block fragments, and the layers run as chains.
int tgat_layers(const TgatStages& c, const dygnn_tgat_weights* w, const float* node_feat, const float* edge_feat, float* out_src, float* out_dst, bool packed);

}  // namespace dygnn
