// Host glue shared by the TGAT inference (tgat.hip) and training (tgat_train.hip) paths: argument checks and the level sets of a call.
// (The inference stages built on it: tgat_stages.h; what TGN adds to a level-0 set: tgn.h.)
// Level L = the 2B roots [src ; dst]; level l-1 = [level l ; its k neighbours (row-major n[l] x k)]; for l >= 1 the neighbours' edge ids and
// time deltas (eid / dt [n[l]][k]) belong to level l.
#pragma once
#include "common.h"

namespace dygnn {

// Where a call's level arrays live (in its workspace)
struct LevelBufs {
    int32_t* ids[DYGNN_MAX_LAYERS + 1];
    double* times[DYGNN_MAX_LAYERS + 1];
    int32_t* eid[DYGNN_MAX_LAYERS + 1];
    float* dt[DYGNN_MAX_LAYERS + 1];
};

// The top level, read straight from the caller's arrays: B pairs [src ; dst] at times[B], or (per_root) every root with its own time
struct TgatRoots {
    const int64_t* src;
    const int64_t* dst;
    const double* times;
    int64_t B;
    bool per_root;
};

struct DedupBufs;      // tgat.hip: de-duplication of level 1 (inference)
struct TgnTouch;       // tgn.h: TGN's owner slots of level 0

int check_tgat(const dygnn_tgat_config* c);
// every pointer of w->layers[0..L-1]; the message is "<what> (layer l)"
int check_layer_weights(const dygnn_tgat_weights* w, int L, const char* what);
// Caller-drawn levels (random sampling strategies), copied where the sampling would have written them: ids[0..id_levels-1] and
// nbr_eid / nbr_dt[1..L].  Every required array is checked before the first copy.
int copy_levels(hipStream_t s, const dygnn_tgat_levels* lv, int L, int k, const int64_t* n, int id_levels, const LevelBufs& to, const char* what);
// The `recent` levels, sampled top-down with k_tgat_expand.  Level L is never written: to.ids[L] / to.times[L] are passed to the kernel
// as they are (it reads the roots instead).  dd: level 1 is expanded from its distinct entries; touch: TGN's owner slots of level 0.
int expand_levels(hipStream_t s, const dygnn_csr* csr, const TgatRoots& roots, int L, int k, const LevelBufs& to, const DedupBufs* dd = nullptr,
                  const TgnTouch* touch = nullptr);

}  // namespace dygnn
