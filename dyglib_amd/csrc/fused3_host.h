// Host-side interface of the fused DyGFormer path: the layout of its section of the packed buffer and the prototype of every entry point
// that another translation unit calls.  dygformer_layout.h includes this header, so the types below are only forward-declared here.
#pragma once
#include <cstdlib>

#include "common.h"

namespace dygnn {

struct Dims;
struct PackedLayout;
struct WorkspaceLayout;
namespace train { struct Drop; struct TrainOut; }

namespace v3 {

struct PackLayout3 {       // float offsets relative to PackedLayout.fused3
    size_t bias_x;
    size_t stream; int64_t nfrag; int nstages;     // ring stream: nfrag fragments, padded to whole stages (+ one of slack)
    size_t aux; int64_t naux;                      // output-layer fragments
    size_t proj; int64_t nproj;                    // projection fragments
    int scr_floats, slab_chunks;                   // LDS split of the K/V region during the prologue
    int np, slab_in_ring;                          // pairs per workgroup (0: shape unsupported); slab placed in the weight ring
    int tab_off, tab_slots, tab_bits;              // co-occurrence table (long windows): LDS word offset, slots per pair
    int scr_floats8, slab_chunks8;                 // the same split with the window arrays of EIGHT pairs (the packed kernel); 0: they do not fit
    size_t bwd[DYGNN_MAX_LAYERS]; int bwd_nstages;  // per layer: the backward stream of its FFN block (training only)
    size_t bwa[DYGNN_MAX_LAYERS]; int bwa_nstages; int64_t bwa_frags;      // ... and of its attention block
    size_t stream_p; int64_t nfrag_p; int nstages_p;       // ring stream of the pooled inference kernels (build_stream, pooled)
    size_t w2;                                     // ... and their last layer's W2 fragments (build_w2)
    size_t qkv0c;                                  // layer 0's constant-channel operands (fused3_plan.h: qkv0_const): [K0 = 48 | 96][38 tiles][64 lanes]
    size_t gelu;                                   // the GELU table of the inference kernels (gelu_table.h): [4096][2], independent of the weights
    size_t desc;           // FragDesc table (device copy), 8-byte aligned
    size_t total;
};

PackLayout3 make_layout3(const Dims& d);       // dygformer_fused3_pack.hip
bool supported(const Dims& d);
int proj_slots(int nchunk);                    // k-chunk slots a projection channel occupies in the stored fragment sequence

}  // namespace v3

// calls of at most this many pairs run one pair per four-wave workgroup (see k_dygformer_fused3): one round on the 256 CUs
constexpr int64_t kSmallBatchPairs = 256;
inline bool small_off() { static const bool off = [] { const char* e = getenv("DYGNN_SMALL_BATCH_KERNELS"); return e && e[0] == '0'; }(); return off; }

// Untapped inference launches of at least this many workgroups end with the token means and leave the last W2 product and the output
// layer to k_pooled_tail (one more launch); smaller ones keep the in-kernel epilogue.  DESIGN §4.3 has the timings behind the figure.
constexpr int64_t kPooledTailMinWorkgroups = 2000;
// DYGNN_POOLED_TAIL = 1 / 0 puts every / no untapped inference launch on the tail path (tests, A/B runs); anything else: the size rule.
// Read on every call.
inline bool pooled_tail_wanted(int64_t workgroups) {
    const char* e = getenv("DYGNN_POOLED_TAIL");
    if (e && (e[0] == '0' || e[0] == '1') && e[1] == '\0') return e[0] == '1';
    return workgroups >= kPooledTailMinWorkgroups;
}

// Untapped launches of pairs of <= 64 tokens that defer their tail run the PACKED kernel: pairs of 1 .. 4 token tiles laid eight tiles to
// a workgroup by the plan kernel (dygformer_pack_plan.hip, fused3_plan.h).  DYGNN_PACK_PAIRS = 0 / 1: never / on every eligible shape (1 also
// defers the tail); anything else: wherever the tail is deferred.  Read on every call.  Returns -1 (unset), 0 or 1.
inline int pack_pairs_env() {
    const char* e = getenv("DYGNN_PACK_PAIRS");
    return (e && (e[0] == '0' || e[0] == '1') && e[1] == '\0') ? e[0] - '0' : -1;
}
// dygformer_pack_plan.hip: the plan of a launch, written to the workspace by one small kernel on stream s
int pack_plan_device(const Dims& d, int64_t B, int64_t G, char* ws, const WorkspaceLayout& wl, hipStream_t s);

// Projected feature tables (dygformer_proj_tables.hip): one (table row, patch slot) segment = the channel's four x tiles, kProjRow floats
constexpr int kProjRow = 64;
// DYGNN_PROJ_TABLES = 0: a forward call ignores the projected tables it is handed (the MFMA path; tests, A/B runs).  Read on every call.
inline bool proj_tables_off() { const char* e = getenv("DYGNN_PROJ_TABLES"); return e && e[0] == '0' && e[1] == '\0'; }

// DYGNN_CONST_QKV = 0 / 1: no / every dygnn_dygformer_forward_projected call carries DYGNN_TABLE_CONST_QKV; anything else: the caller's bit.
// Read on every call.  Returns -1 (unset), 0 or 1.
inline int const_qkv_env() {
    const char* e = getenv("DYGNN_CONST_QKV");
    return (e && (e[0] == '0' || e[0] == '1') && e[1] == '\0') ? e[0] - '0' : -1;
}

// dygformer_generic.hip
int window_lengths_device(const Dims& d, const dygnn_csr* csr, const int64_t* src, const int64_t* dst, const double* times,
                          int64_t B, int64_t G, char* ws, const WorkspaceLayout& wl, hipStream_t s);
// the co-occurrence table lut [rows][C], row c = W1 relu(W0 c + b0) + b1 (DyGFormer.py:332-335); hid (may be NULL) [rows][C] = the hidden
// rows relu(W0 c + b0), which the training backward reads
int cooc_table_device(const dygnn_dygformer_weights* w, int rows, int C, float* lut, float* hid, hipStream_t s);
// dygformer_fused3_pack.hip
bool fused3_supported(const Dims& d);
size_t fused3_packed_floats(const Dims& d);
int pack_fused3(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, float* packed, hipStream_t s, bool reuse_desc, bool training);
// dygformer_fused3.hip
int forward_fused3(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, const float* packed,
                   const dygnn_csr* csr, const float* node_feat, const float* edge_feat, const int64_t* src,
                   const int64_t* dst, const double* times, int64_t B, int64_t G, int64_t pair_stride, float* out_src, float* out_dst, char* ws,
                   const WorkspaceLayout& wl, const dygnn_dygformer_taps* taps, uint32_t table_flags, const float* node_proj, const float* edge_proj,
                   hipStream_t s);
// dygformer_pooled_tail.hip: rows [R][1008] (R = 2 B, row 2 * pair + side) -> out_src / out_dst [B][Fn]
int pooled_tail(const float* rows, int64_t R, const float* w2frag, const float* b2, const float* outfrag, const float* outb, int Fn,
                float* out_src, float* out_dst, hipStream_t s);
// dygformer_fused3_train.hip
int forward_fused3_train(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, const float* packed, const dygnn_csr* csr,
                         const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times, int64_t B,
                         const float* lut, float* out_src, float* out_dst, char* ws, const WorkspaceLayout& wl, const train::TrainOut& tr, hipStream_t s);
// dygformer_fused3_bwd.hip
int ffn_backward_fused3(const Dims& d, const PackedLayout& pl, const float* packed, int l, int64_t M, float* dX, const float* hpre, const float* x1,
                        const float* m1, const float* r1, float* dF2, float* dH, float* dgamma, float* dbeta, const train::Drop& dr, hipStream_t s);
int attn_backward_fused3(const Dims& d, const PackedLayout& pl, const float* packed, int l, int64_t B, int T, float* dX, const float* X, const float* m0,
                         const float* r0, const float* qkv, const float* P, const float* Pd, float* dAo, float* dQKV, float* dgamma, float* dbeta,
                         const train::Drop& dr, hipStream_t s);

}  // namespace dygnn
