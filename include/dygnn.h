/*
 * dygnn.h — C ABI of libdygnn_hip.so: MI355X (gfx950) kernels for DyGLib's
 * temporal-neighbour-aggregation hot path.
 *
 * The reference (webster-781/DyGLib) is pure Python and has no FFI: its boundary for this
 * path is the duck-typed Python interface of utils/utils.py:71-302 (NeighborSampler) and
 * models/DyGFormer.py:11-317 (DyGFormer).  This header is what a binding for that path
 * binds; every entry point cites the reference code it replaces.  INTEGRATION.md shows the
 * ctypes stub and the two-line change to train_link_prediction.py.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / HIP types in the signatures (dygnn_stream_t is a
 *     hipStream_t passed as void*; NULL = the null stream);
 *   - every pointer is a DEVICE pointer unless the parameter name ends in _host;
 *   - no allocation and no host synchronisation inside any *device* entry point: callers pass
 *     workspaces sized by the *_bytes() helpers, so calls can be captured in a hipGraph;
 *   - return value: 0 = ok, <0 = error (DYGNN_E_*); dygnn_last_error() returns a message for
 *     the calling thread.  Invalid arguments map to the reference's AssertionError sites,
 *     e.g. k <= 0 (utils/utils.py:157) or max_input_sequence_length <= 1 (DyGFormer.py:209).
 */
#ifndef DYGNN_H
#define DYGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYGNN_OK            0
#define DYGNN_E_INVALID    -1   /* bad argument (reference: AssertionError / ValueError)   */
#define DYGNN_E_HIP        -2   /* HIP runtime error (launch failure, bad pointer ...)     */
#define DYGNN_E_UNSUPPORTED -3  /* shape outside what the kernels were built for           */
#define DYGNN_E_WORKSPACE  -4   /* caller workspace too small                              */

#define DYGNN_MAX_LAYERS 8

typedef void* dygnn_stream_t;   /* hipStream_t */

const char* dygnn_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int dygnn_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Temporal CSR: the time-sorted adjacency of NeighborSampler.__init__ (utils/utils.py:73-110)
 * built from an interaction list by get_neighbor_sampler (utils/utils.py:283-302).
 * Row r = node id r; row 0 = padding node, empty.  Inside a row entries ascend in time, ties
 * in edge-list order (stable sort, utils/utils.py:98-100).  Undirected: each interaction is
 * stored under both endpoints (utils/utils.py:298-300), src entry first.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_csr {
    int64_t        num_nodes;    /* rows = max node id + 1                                  */
    int64_t        num_entries;  /* 2 * number of interactions                              */
    const int64_t* indptr;       /* [num_nodes + 1]                                         */
    const int32_t* nbr;          /* [num_entries] neighbour node id                         */
    const int32_t* eid;          /* [num_entries] edge id                                   */
    const double*  ts;           /* [num_entries] interaction time (float64, as stored)     */
} dygnn_csr;

/* Host-side builder (C++, no GPU needed).  Inputs: the four parallel arrays of `Data`
 * (utils/DataLoader.py:46-64).  Outputs: caller-allocated host arrays of the sizes above with
 * num_nodes = max(src,dst)+1.  Replaces utils/utils.py:283-302 + :96-103. */
int dygnn_csr_build_host(int64_t num_edges, const int64_t* src_host, const int64_t* dst_host,
                         const int64_t* eid_host, const double* ts_host, int64_t num_nodes,
                         int64_t* indptr_host, int32_t* nbr_host, int32_t* eid_out_host, double* ts_out_host);

/* `uniform` neighbour sampling, host side (utils/utils.py:176-199): row r draws k positions in [0, hist_len[r]) exactly
 * as `RandomState.choice(a=hist_len[r], size=k)` of numpy's legacy MT19937 generator does (masked rejection on 32-bit outputs; rows with
 * hist_len <= 1 consume nothing and get zeros).  key[624] / *pos are the generator's state, taken from and written back to the sampler's
 * numpy RandomState by the caller, so the stream stays numpy's.  Host pointers; no GPU work. */
int dygnn_mt19937_choice_rows_host(uint32_t* key_host, int32_t* pos_host, const int32_t* hist_len_host, int64_t n, int32_t k,
                                   int32_t* sampled_host);

/* find_neighbors_before for n queries (utils/utils.py:130-147): hist_len[q] = i =
 * searchsorted(times[node], t, side='left') and end_pos[q] = indptr[node] + i (absolute CSR
 * index one past the last strictly-earlier interaction).  Either output may be NULL. */
int dygnn_find_neighbors_before(const dygnn_csr* csr_host, const int64_t* nodes, const double* times, int64_t n,
                                int32_t* hist_len, int64_t* end_pos, dygnn_stream_t stream);

/* get_historical_neighbors, strategy 'recent' (utils/utils.py:149-214, branch :200-209):
 * most recent k strictly-earlier interactions, RIGHT-aligned, zero-filled at the front.
 * Outputs [n,k]: int64 ids, int64 edge ids, float32 times (dtypes of utils/utils.py:161-167). */
int dygnn_sample_recent(const dygnn_csr* csr_host, const int64_t* nodes, const double* times, int64_t n, int32_t k,
                        int64_t* out_nbr, int64_t* out_eid, float* out_ts, dygnn_stream_t stream);

/* get_historical_neighbors, strategies 'uniform' / 'time_interval_aware' (utils/utils.py:176-199): the draws come
 * from the host (numpy RandomState replay, so they are bit-identical to the reference's), this entry point gathers
 * them: sel [n,k] int32 holds, per query, the positions INSIDE the node's time-sorted row (0 = oldest interaction) in
 * final output order, or -1 for "no neighbour" (rows of nodes without history stay zero, utils/utils.py:161-167).
 * Outputs [n,k]: int64 ids, int64 edge ids, float32 times. */
int dygnn_gather_selected(const dygnn_csr* csr_host, const int64_t* nodes, const int32_t* sel, int64_t n, int32_t k,
                          int64_t* out_nbr, int64_t* out_eid, float* out_ts, dygnn_stream_t stream);

/* DyGFormer window, phase 1 (get_all_first_hop_neighbors utils/utils.py:254-273 + the length
 * scan of pad_sequences models/DyGFormer.py:210-220): per query hist_len / end_pos as above and
 * *max_window = max_q min(hist_len[q], L-1) (device int32, overwritten).  The padded length is
 * S = roundup(*max_window + 1, patch_size) (models/DyGFormer.py:223-226). */
int dygnn_window_lengths(const dygnn_csr* csr_host, const int64_t* nodes, const double* times, int64_t n,
                         int32_t max_input_sequence_length, int32_t* hist_len, int64_t* end_pos,
                         int32_t* max_window, dygnn_stream_t stream);

/* DyGFormer window, phase 2 (pad_sequences models/DyGFormer.py:228-245): [n,S] LEFT-aligned
 * rows: col 0 = (node, edge 0, float32(t)); cols 1..m = the most recent m = min(hist_len, L-1)
 * interactions oldest->newest; zeros after.  int64 / int64 / float32 as :230-232. */
int dygnn_window_fill(const dygnn_csr* csr_host, const int64_t* nodes, const double* times, int64_t n,
                      int32_t max_input_sequence_length, int32_t S, const int32_t* hist_len, const int64_t* end_pos,
                      int64_t* out_ids, int64_t* out_eids, float* out_ts, dygnn_stream_t stream);

/* NeighborCooccurrenceEncoder.count_nodes_appearances (models/DyGFormer.py:337-393):
 * src_ids [n,S_s], dst_ids [n,S_d] int64 -> cnt_src [n,S_s,2], cnt_dst [n,S_d,2] float32 holding
 * [count in src row, count in dst row]; positions with id 0 give [0,0]. */
int dygnn_cooccurrence(const int64_t* src_ids, const int64_t* dst_ids, int64_t n, int32_t S_s, int32_t S_d,
                       float* cnt_src, float* cnt_dst, dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DyGFormer.compute_src_dst_node_temporal_embeddings (models/DyGFormer.py:68-194), eval mode.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_dygformer_config {
    int32_t node_feat_dim;              /* F_n (172)                         DyGFormer.py:36 */
    int32_t edge_feat_dim;              /* F_e (172)                         DyGFormer.py:37 */
    int32_t time_feat_dim;              /* F_t (100)                         DyGFormer.py:38 */
    int32_t channel_embedding_dim;      /* C (50); model dim D = 4C          DyGFormer.py:39 */
    int32_t patch_size;                 /* P                                 DyGFormer.py:40 */
    int32_t num_layers;                 /* <= DYGNN_MAX_LAYERS               DyGFormer.py:41 */
    int32_t num_heads;                  /* H, D % H == 0                     DyGFormer.py:42 */
    int32_t max_input_sequence_length;  /* L                                 DyGFormer.py:44 */
} dygnn_dygformer_config;

/* Raw parameter pointers in PyTorch layout (row-major [out,in]); names = state_dict keys
 * (SURVEY.md Appendix A). */
typedef struct dygnn_encoder_layer_weights {
    const float *in_proj_weight, *in_proj_bias;      /* [3D,D],[3D]  multi_head_attention     */
    const float *out_proj_weight, *out_proj_bias;    /* [D,D],[D]                             */
    const float *ffn0_weight, *ffn0_bias;            /* [4D,D],[4D]  linear_layers.0          */
    const float *ffn1_weight, *ffn1_bias;            /* [D,4D],[D]   linear_layers.1          */
    const float *norm0_weight, *norm0_bias;          /* [D]          norm_layers.0            */
    const float *norm1_weight, *norm1_bias;          /* [D]          norm_layers.1            */
} dygnn_encoder_layer_weights;

typedef struct dygnn_dygformer_weights {
    const float *time_w, *time_b;                    /* [F_t,1],[F_t] time_encoder.w          */
    const float *cooc_w0, *cooc_b0;                  /* [C,1],[C]    ..encode_layer.0         */
    const float *cooc_w1, *cooc_b1;                  /* [C,C],[C]    ..encode_layer.2         */
    const float *proj_node_w, *proj_node_b;          /* [C,P*F_n],[C]                         */
    const float *proj_edge_w, *proj_edge_b;          /* [C,P*F_e],[C]                         */
    const float *proj_time_w, *proj_time_b;          /* [C,P*F_t],[C]                         */
    const float *proj_cooc_w, *proj_cooc_b;          /* [C,P*C],[C]                           */
    dygnn_encoder_layer_weights layers[DYGNN_MAX_LAYERS];
    const float *output_w, *output_b;                /* [F_n,D],[F_n] output_layer            */
} dygnn_dygformer_weights;

/* Optional stage taps for parity tests (any member may be NULL).  Row-major, token stride
 * T_max = 2*ceil(L/P):  encoder_input / layer_out[l] are [B, T_max, D]. */
typedef struct dygnn_dygformer_taps {
    int32_t* seq_lens;                               /* [2]: S_src, S_dst of group 0          */
    float*   encoder_input;
    float*   layer_out[DYGNN_MAX_LAYERS];
    uint64_t* phase_cycles;                          /* diagnostic builds (-DDYGNN_STAMPS) only:
                                                        [4 workgroups][8 waves][32] s_memtime stamps */
    void*    ev_kernel_start;                        /* hipEvent_t (or NULL): recorded on `stream` immediately before / after the  */
    void*    ev_kernel_stop;                         /* launch of the dominant kernel of the call (the fused forward), so a caller  */
                                                     /* can time THAT kernel, not the call (bench.py's roofline line)               */
} dygnn_dygformer_taps;

/* Kernel-ready copy of the weights (transposed / MFMA-fragment order, co-occurrence LUT).
 * Re-pack after every optimizer step; packing is one cheap launch sequence. */
size_t dygnn_dygformer_packed_bytes(const dygnn_dygformer_config* cfg_host);
int dygnn_dygformer_pack(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                         void* packed, size_t packed_bytes, dygnn_stream_t stream);
/* The weights changed IN PLACE (an optimizer step: same device addresses as at the last dygnn_dygformer_pack into `packed`):
 * refresh the copy with kernel launches only — no host work, no synchronisation (train_link_prediction.py:257 runs once per step).
 * fused_only != 0 refreshes just what the training entry points read (the fragment streams: two launches); the co-occurrence table and
 * the transposed copies of the inference paths are then stale until a call with fused_only = 0. */
int dygnn_dygformer_repack(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                           void* packed, size_t packed_bytes, int32_t fused_only, dygnn_stream_t stream);

size_t dygnn_dygformer_workspace_bytes(const dygnn_dygformer_config* cfg_host, int64_t batch);
/* the same for one implementation choice (`impl` of dygnn_dygformer_forward): the fused kernels need only the per-query search
 * results, the generic path also its activation buffers; dygnn_dygformer_workspace_bytes is the size that serves every impl */
size_t dygnn_dygformer_workspace_bytes_for(const dygnn_dygformer_config* cfg_host, int64_t batch, int32_t impl);

/* Host arithmetic of the fused inference kernels' token compaction and pair packing (tests; no GPU).  pair_tokens: a pair of a call
 * padded to T_s + T_d tokens whose windows hold len_s / len_d neighbours -> out = {R_s, R_d, m_s, m_d, Tc}: real tokens and all-padding
 * tokens per side, tokens computed (real ones + one padding token).  pack_plan: pairs of tiles[i] (1 .. 4) token tiles laid eight tiles
 * to a workgroup by the plan kernel's own arithmetic -> wg[i], first_wave[i]; returns the workgroups used, -1 on a bad tile count. */
void dygnn_dygformer_pair_tokens_host(int32_t len_s, int32_t len_d, int32_t L, int32_t P, int32_t T_s, int32_t T_d, int32_t* out);
int64_t dygnn_dygformer_pack_plan_host(const int32_t* tiles, int64_t n, int32_t* wg, int32_t* first_wave);
/* ... and of layer 0's constant input channels (DYGNN_TABLE_CONST_QKV below).  qkv_tile_row: the in_proj row (0 .. 599) that row c (0 .. 15)
 * of output tile `tile` (0 .. 37, stream order: per head 7 q tiles — the seventh combines rows 96 .. 99 of q | k | v — 6 k tiles, 6 v tiles)
 * holds; -1: padding, -2: bad arguments.  qkv0_const: out[38][64] = the rank-3 term's MFMA A operands for the prefix k0 = 48 or 96 — lane
 * (c = lane & 15, g = lane >> 4) of a tile holds A | G | Bt | 0 (g = 0 .. 3) of its row, float64 sums rounded once; in_proj_weight [600][200],
 * gamma / beta = norm_layers.0 [200], bias = the node then the edge projection bias (>= k0 floats).  All host pointers. */
int32_t dygnn_dygformer_qkv_tile_row_host(int32_t tile, int32_t c);
int dygnn_dygformer_qkv0_const_host(const float* in_proj_weight, const float* gamma, const float* beta, const float* bias, int32_t k0, float* out);
/* ... and of the pooled layer's per-side token sums.  The kernels sum eight values per lane (input k = 4 u + r: row 4 (lane >> 4) + r of
 * register tile u) over the 16 lanes of a lane group by a reduce-scatter; pool_sum_slot: out = {1 if `lane` (0 .. 63) stores, the tile u and
 * the first row (0 .. 15) of the two adjacent words it stores, the inputs whose sums its two results hold}. */
void dygnn_dygformer_pool_sum_slot_host(int32_t lane, int32_t* out);

/* One launch sequence for `batch` (src,dst,t) pairs.  group_size = G splits the pairs into consecutive
 * groups of G that are padded independently (each group has its own S_src/S_dst, models/DyGFormer.py:219-226):
 * the result of every group is bit-identical to a separate reference call on that group, so several
 * reference calls (e.g. the positive and the negative call of a step, evaluate_models_utils.py:126-136, or
 * several evaluation batches) run as ONE grid that keeps all 256 CUs busy.  G = 0 or G >= batch: one group.
 * pair_stride (caller-side fusion): 0, or batch / 2 when the batch is [positive calls ; negative calls] of the same
 * edges — pair i + pair_stride has the source and time of pair i (train_link_prediction.py:165-166, evaluate_models_utils.py:62-63).
 * The fused kernel then puts both pairs of an edge in one workgroup and gathers / projects the shared source side once; every row
 * is still bit-identical to the separate reference calls, and pairs whose (src, t) differ simply take the plain path.
 * impl: 0 = auto (the fused MFMA kernel when the shape is supported, else generic),
 *       1 = generic multi-kernel path (any shape),
 *       3 = fused kernel, token-owner layout (<= 128 tokens per pair; error if unsupported);
 *       2 (the first fused kernel, superseded) was removed in ABI 11 and is an error.
 * Node ids: the reference trusts them (an out-of-range id is an IndexError from numpy).  The host mirror raises
 * that IndexError for numpy inputs and validates the tables once per sampler (every CSR neighbour id < rows of node_feat,
 * every CSR edge id < rows of edge_feat); the kernels themselves never fault on a bad QUERY id: ids outside
 * [0, csr.num_nodes) are treated as the padding node 0 (empty history, zero feature row). */
int dygnn_dygformer_forward(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                            const void* packed, const dygnn_csr* csr_host,
                            const float* node_feat, const float* edge_feat,
                            const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                            int64_t group_size, int64_t pair_stride, float* out_src, float* out_dst,
                            void* workspace, size_t workspace_bytes,
                            const dygnn_dygformer_taps* taps_host, int32_t impl, dygnn_stream_t stream);

/* dygnn_dygformer_forward with a promise about the feature tables.  table_flags is a bit set:
 *   DYGNN_TABLE_NODE_ZERO  every element of node_feat is 0.0 (what the reference's preprocessing writes for every dataset,
 *                          preprocess_data/preprocess_data.py:108)
 *   DYGNN_TABLE_EDGE_ZERO  every element of edge_feat is 0.0
 * The fused inference kernel then leaves the channel out of the patch projection: no gathers, no MFMAs and no weight traffic for it;
 * its token rows are the channel's projection bias.  For finite projection weights the result has the bits of the unflagged call,
 * because adding w * 0 to the bias changes nothing — with one exception: a bias element of -0.0 stays -0.0 here, where the
 * unflagged call turns it into +0.0 (-0.0 + 0.0).  Non-finite weights give NaN unflagged (inf * 0) and the bias here.
 * The flags are the CALLER'S PROMISE and are not checked: a flag set for a table that holds a non-zero element gives WRONG RESULTS
 * (the table is ignored).  Establish them once per table (it is a constructor argument of the model) and again when it changes.
 * Every fused inference shape honours the flags, the long-window one whose projection slab borrows the weight ring included.  The
 * generic path (impl = 1, or an unsupported shape under impl = 0) and the training entry points ignore them.  Any other bit is an
 * error.  table_flags = 0 is dygnn_dygformer_forward. */
#define DYGNN_TABLE_NODE_ZERO 1u
#define DYGNN_TABLE_EDGE_ZERO 2u
int dygnn_dygformer_forward_tables(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                                   const void* packed, const dygnn_csr* csr_host,
                                   const float* node_feat, const float* edge_feat,
                                   const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                                   int64_t group_size, int64_t pair_stride, float* out_src, float* out_dst,
                                   void* workspace, size_t workspace_bytes,
                                   const dygnn_dygformer_taps* taps_host, int32_t impl, dygnn_stream_t stream, uint32_t table_flags);

/* Projected feature tables.  The patch projection of the node and of the edge channel is linear in the table rows it gathers, and
 * neither the table nor (in an evaluation pass) the weights change between calls: dygnn_dygformer_project_table computes
 *     projected[row][p][0 .. 63] = proj_w[:, p F .. (p + 1) F) . table[row]        (p < patch_size; F = the channel's feature dim)
 * once — each element one fmaf chain over the F features; the 64 floats are the four 16-row tiles of the model dimension that the
 * channel touches, zero outside its 50 rows — and the fused inference kernel then adds patch_size gathered rows per token instead of
 * running the product: x = ((bias + projected[row_0][0]) + projected[row_1][1]) + ...  The sum is split per slot, so the channel's rows
 * differ from the unprojected call's in the last bits; they do not depend on kernel shape, batch size, group_size or pair_stride.
 *   dygnn_dygformer_projected_bytes   size of one projected table of `rows` rows (host only; 0: bad config, rows <= 0, or a shape the
 *                                     fused kernel does not support) = rows * patch_size * 64 * sizeof(float)
 *   dygnn_dygformer_project_table     channel 0 = node features (proj_node_w), 1 = edge features (proj_edge_w); one launch on `stream`.
 *                                     `projected` is device memory, 16-byte aligned.  Run it again whenever the weights or the table change.
 *   dygnn_dygformer_forward_projected dygnn_dygformer_forward_tables plus
 *       DYGNN_TABLE_NODE_PROJ  node_proj is the projected node table        DYGNN_TABLE_EDGE_PROJ  edge_proj is the projected edge table
 *     A pointer whose bit is not set is ignored; a set bit with a NULL pointer is an error.  A channel flagged all zero ignores its
 *     projected table.  The flags are the caller's promise, as above: a stale projected table gives wrong results.  The environment
 *     variable DYGNN_PROJ_TABLES=0 (read on every call) makes the call ignore both, which is dygnn_dygformer_forward_tables; so do the
 *     generic path and the training entry points.  Without projected bits the call IS dygnn_dygformer_forward_tables, bit for bit.
 *       DYGNN_TABLE_CONST_QKV  (this entry point only; dygnn_dygformer_forward_tables rejects it)  With DYGNN_TABLE_NODE_ZERO the first 50
 *     rows of every token's encoder input are the node projection bias, so the first 48 rows of layer 0's LayerNorm output depend on the
 *     token through its mean and reciprocal standard deviation alone: layer 0's Q/K/V products leave out those 3 k-chunks and add
 *     rs A + (-mean rs) G + Bt instead, one MFMA per output tile, with A, G, Bt summed once per weights version (dygnn_dygformer_pack, and
 *     dygnn_dygformer_repack with fused_only = 0).  With DYGNN_TABLE_EDGE_ZERO as well the prefix is 96 rows = 6 k-chunks.  The rule is the
 *     constant PREFIX: without DYGNN_TABLE_NODE_ZERO the bit changes nothing, and a projected table is not constant.  The sums are taken
 *     in another order, so q, k, v of layer 0 differ from the call without the bit in the last bits (1e-6 of values up to 3); they do not
 *     depend on kernel shape, batch size, group_size, pair_stride or taps.  DYGNN_CONST_QKV=0 / 1 (read on every call) clears / sets
 *     the bit whatever the caller passed; DYGNN_PROJ_TABLES does not touch it.  The generic path ignores it. */
#define DYGNN_TABLE_NODE_PROJ 4u
#define DYGNN_TABLE_EDGE_PROJ 8u
#define DYGNN_TABLE_CONST_QKV 32u      /* (16u stays an unknown bit) */
size_t dygnn_dygformer_projected_bytes(const dygnn_dygformer_config* cfg_host, int64_t rows);
int dygnn_dygformer_project_table(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host, int32_t channel,
                                  const float* table, int64_t rows, void* projected, size_t projected_bytes, dygnn_stream_t stream);
int dygnn_dygformer_forward_projected(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                                      const void* packed, const dygnn_csr* csr_host,
                                      const float* node_feat, const float* edge_feat,
                                      const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                                      int64_t group_size, int64_t pair_stride, float* out_src, float* out_dst,
                                      void* workspace, size_t workspace_bytes,
                                      const dygnn_dygformer_taps* taps_host, int32_t impl, dygnn_stream_t stream, uint32_t table_flags,
                                      const float* node_proj, const float* edge_proj);

/* ------------------------------------------------------------------------------------------
 * TGAT.compute_src_dst_node_temporal_embeddings (models/TGAT.py:48-136), eval mode, `recent`
 * sampling: L temporal-attention layers (MultiHeadAttention models/modules.py:99-206, mask =
 * neighbour id == 0 -> -1e10, post-LayerNorm) each followed by MergeLayer([out | raw node feat])
 * (models/TGAT.py:134).  Hop-(l+1) queries use the float32 neighbour times (models/TGAT.py:107-110).
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_tgat_config {
    int32_t node_feat_dim, edge_feat_dim, time_feat_dim;   /* 172, 172, 100; each a multiple of 4   */
    int32_t num_layers;                                    /* 1..3                  models/TGAT.py:28 */
    int32_t num_heads;                                     /* (F_n+F_t) % H == 0    modules.py:120   */
    int32_t num_neighbors;                                 /* k <= 64               models/TGAT.py:49 */
} dygnn_tgat_config;

typedef struct dygnn_tgat_layer_weights {                  /* state_dict keys, PyTorch [out,in] layout */
    const float *query_w;                                  /* temporal_conv_layers.l.query_projection.weight [Dq,Dq]  */
    const float *key_w, *value_w;                          /* ...key_projection / value_projection.weight    [Dq,Dkv] */
    const float *ln_w, *ln_b;                              /* ...layer_norm.{weight,bias}                     [Dq]     */
    const float *res_w, *res_b;                            /* ...residual_fc.{weight,bias}              [Dq,Dq],[Dq]   */
    const float *fc1_w, *fc1_b;                            /* merge_layers.l.fc1                 [F_n,Dq+F_n],[F_n]    */
    const float *fc2_w, *fc2_b;                            /* merge_layers.l.fc2                 [F_n,F_n],[F_n]       */
} dygnn_tgat_layer_weights;

typedef struct dygnn_tgat_weights {
    const float *time_w, *time_b;                          /* time_encoder.w                                           */
    dygnn_tgat_layer_weights layers[DYGNN_MAX_LAYERS];
} dygnn_tgat_weights;

size_t dygnn_tgat_workspace_bytes(const dygnn_tgat_config* cfg_host, int64_t batch);
int dygnn_tgat_forward(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_csr* csr_host,
                       const float* node_feat, const float* edge_feat,
                       const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                       float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* The same forward for a LIST of (node, time) roots: out [n_roots][node_feat_dim] = TGAT.compute_node_temporal_embeddings(ids, times,
 * num_layers) (models/TGAT.py:66-136), every root with its own time (`recent` sampling).  n_roots must be even; workspace as for
 * dygnn_tgat_forward with batch = n_roots / 2.  The evaluation step of evaluate_models_utils.py:126-136 needs the embeddings of
 * [sources ; destinations ; negative destinations] at the batch times: its negative call repeats the sources of its positive call
 * (:62-63), so one call on 3 B roots replaces two calls on 2 B roots each. */
int dygnn_tgat_forward_roots(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_csr* csr_host,
                             const float* node_feat, const float* edge_feat, const int64_t* ids, const double* times, int64_t n_roots,
                             float* out, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* The same forward on PRE-SAMPLED neighbours, for the random strategies (uniform / time_interval_aware, e.g. the reference's
 * best TGAT configuration on Reddit, utils/load_configs.py:83-84): the draws must come from the sampler's numpy RandomState
 * in the reference's recursion order (models/TGAT.py:92-110), so the host builds the level sets and this entry point runs
 * everything else.  Level L = the 2*batch query nodes [src ; dst]; level l-1 = [level-l entries ; their k sampled neighbours
 * (row-major)].  For l = 1..L: nbr_eid[l] / nbr_dt[l] are [n_l, k] (edge id; float32(t_entry - float32(t_neighbour)),
 * models/TGAT.py:116-119); ids[l] for l = 0..L are the node ids of the level entries (int32).  All device pointers. */
typedef struct dygnn_tgat_levels {
    const int32_t* ids[DYGNN_MAX_LAYERS + 1];
    const int32_t* nbr_eid[DYGNN_MAX_LAYERS + 1];          /* [0] unused */
    const float* nbr_dt[DYGNN_MAX_LAYERS + 1];             /* [0] unused */
} dygnn_tgat_levels;
int dygnn_tgat_forward_levels(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_tgat_levels* levels_host,
                              const float* node_feat, const float* edge_feat, int64_t batch,
                              float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* Diagnostic (synchronises `stream`): how many (node, time) entries the LAST dygnn_tgat_forward call on `workspace` (same cfg / batch)
 * had over its computed levels (*total = sum of the level sizes n_1 .. n_L, what the reference computes, models/TGAT.py:92-110) and how
 * many the library computed (*computed): with `recent` sampling a two-layer model computes every distinct entry of level 1 once. */
int dygnn_tgat_level_entries(const dygnn_tgat_config* cfg_host, int64_t batch, const void* workspace, int64_t* total_host, int64_t* computed_host,
                             dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * TGN: MemoryModel.compute_src_dst_node_temporal_embeddings with model_name == 'TGN'
 * (models/MemoryModel.py:87-168): GRU memory update from the last pending raw message of every node
 * (MessageAggregator :267-300, GRUMemoryUpdater :490-501 = nn.GRUCell(2F_n+F_t+F_e, F_n)), temporal graph
 * attention over (memory + raw) node features (GraphAttentionEmbedding :548-664, same layer as TGAT), and —
 * for positive edges — memory persistence + new raw messages (:142-161, :212-251).
 * State lives in caller-owned device buffers and is MUTATED by positive calls; batches must be issued in
 * chronological order on one stream (the reference's strict batch-sequential semantics).
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_gru_weights {          /* memory_updater.memory_updater.{weight_ih,weight_hh,bias_ih,bias_hh}           */
    const float *weight_ih, *weight_hh;     /* [3F_n, 2F_n+F_t+F_e], [3F_n, F_n]   (gate order r | z | n, nn.GRUCell)         */
    const float *bias_ih, *bias_hh;         /* [3F_n], [3F_n]                                                                  */
} dygnn_gru_weights;

typedef struct dygnn_tgn_state {
    int64_t  num_nodes;                     /* rows of node_raw_features (max node id + 1)                                     */
    float*   memory;                        /* [N, F_n]  memory_bank.node_memories                                             */
    float*   last_update;                   /* [N]       memory_bank.node_last_updated_times (float32)                         */
    float*   msg;                           /* [N, 2F_n+F_t+F_e]  last pending raw message per node                            */
    double*  msg_time;                      /* [N]       its interaction time                                                  */
    int32_t* has_msg;                       /* [N]       1 while a message is pending (list non-empty, MemoryModel.py:284)     */
} dygnn_tgn_state;

size_t dygnn_tgn_workspace_bytes(const dygnn_tgat_config* cfg_host, int64_t num_nodes, int64_t batch);
int dygnn_tgn_forward(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_gru_weights* gru_host,
                      const dygnn_csr* csr_host, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* state_host,
                      const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids /* NULL if !positive */,
                      int64_t batch, int32_t edges_are_positive, float* out_src, float* out_dst,
                      void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* One evaluation / training step in ONE call (caller-side fusion): the reference issues the negative call and then the
 * positive call of a batch (evaluate_models_utils.py:85-107); both read the same state -- only the positive call writes it, at its end --
 * so the batch may hold both: the first n_positive pairs are the positive edges (they persist memories and leave new raw messages,
 * edge_ids [n_positive]), the remaining batch - n_positive pairs only read.  Rows and the state left behind are bit-identical to
 * dygnn_tgn_forward(negatives, edges_are_positive = 0) followed by dygnn_tgn_forward(positives, 1); the GRU update and every
 * kernel launch happen once instead of twice.  n_positive = batch / 0 reproduces the two modes of dygnn_tgn_forward. */
int dygnn_tgn_forward_step(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_gru_weights* gru_host,
                           const dygnn_csr* csr_host, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* state_host,
                           const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids /* [n_positive] */,
                           int64_t batch, int64_t n_positive, float* out_src, float* out_dst,
                           void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* dygnn_tgn_forward_step on PRE-SAMPLED neighbour levels: the reference's TGN accepts any sample_neighbor_strategy
 * (models/MemoryModel.py:626-629 calls the sampler it was given; utils/utils.py:176-199 for 'uniform' / 'time_interval_aware', whose
 * draws consume the sampler's numpy RandomState in call order).  The host mirror replays those draws in the reference's order — ONE
 * get_historical_neighbors call on [src ; dst] per layer of the recursion, MemoryModel.py:104-131, :596-640 — and hands the levels over
 * in dygnn_tgat_levels' layout (batch = pairs; level L = [src ; dst]).  src / dst / times / edge_ids are read by the commit of a positive
 * call only (n_positive > 0).  Same workspace size as dygnn_tgn_forward. */
int dygnn_tgn_forward_levels(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_gru_weights* gru_host,
                             const dygnn_tgat_levels* levels_host, const float* node_feat, const float* edge_feat,
                             const dygnn_tgn_state* state_host, const int64_t* src, const int64_t* dst, const double* times,
                             const int64_t* edge_ids /* [n_positive] */, int64_t batch, int64_t n_positive, float* out_src, float* out_dst,
                             void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * JODIE: MemoryModel.compute_src_dst_node_temporal_embeddings with model_name == 'JODIE' (models/MemoryModel.py:87-168, :519-545):
 * nn.RNNCell memory update from the last pending raw message (RNNMemoryUpdater :504-515: h' = tanh(W_ih m + b_ih + W_hh h + b_hh)) and
 * the time-projection embedding  emb = updated_memory * (1 + linear_layer(delta)),  delta = (float32(t) - updated_last_update - mean) / std
 * in float32, the source pair of shift constants for source rows and the destination pair for destination rows (:111-124).  No
 * neighbours, no sampler.  State, message layout and the commit of the positive pairs are TGN's (dygnn_tgn_state).
 * A call reads only its roots: rows [src ; dst] of the batch, every row computed on its own (duplicates repeat the same bits), so the
 * workspace does not depend on the number of nodes.  n_positive as in dygnn_tgn_forward_step: the first n_positive pairs persist their
 * updated memories / last-update times and leave new raw messages (edge_ids [n_positive]); batch = a positive call, 0 = a negative call.
 * Rows and state are bit-identical to the negative call followed by the positive call.  At most three launches (weight packing, the
 * row kernel, the commit); inference only.
 * Dimensions: node_feat_dim (= memory dim), time_feat_dim, edge_feat_dim multiples of 4 whose four-row block fits the LDS; others
 * DYGNN_E_UNSUPPORTED, the message names the value.  cfg->num_layers / num_heads / num_neighbors are not read.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_rnn_weights {          /* memory_updater.memory_updater.{weight_ih,weight_hh,bias_ih,bias_hh} of nn.RNNCell: one gate */
    const float *weight_ih, *weight_hh;     /* [F_n, 2F_n+F_t+F_e], [F_n, F_n]                                                  */
    const float *bias_ih, *bias_hh;         /* [F_n], [F_n]                                                                     */
} dygnn_rnn_weights;

size_t dygnn_jodie_workspace_bytes(const dygnn_tgat_config* cfg_host, int64_t num_nodes /* not used: the size depends on batch only */, int64_t batch);
int dygnn_jodie_forward_step(const dygnn_tgat_config* cfg_host, const float* time_w, const float* time_b, const dygnn_rnn_weights* rnn_host,
                             const float* proj_w /* embedding_module.linear_layer.weight [F_n, 1] */, const float* proj_b /* [F_n] */,
                             double src_mean_time_shift, double src_std_time_shift, double dst_mean_time_shift, double dst_std_time_shift,
                             const float* edge_feat, const dygnn_tgn_state* state_host, const int64_t* src, const int64_t* dst, const double* times,
                             const int64_t* edge_ids /* [n_positive] */, int64_t batch, int64_t n_positive, float* out_src, float* out_dst,
                             void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * DyRep: MemoryModel.compute_src_dst_node_temporal_embeddings with model_name == 'DyRep' (models/MemoryModel.py:73-83, :125-132, :163-166,
 * :225-227): TGN's modules with the RNN cell (dygnn_rnn_weights).  A call returns the UPDATED MEMORIES of its roots (the cell output for a
 * node with a pending message, the stored memory otherwise); the temporal attention runs for the first n_positive pairs only, where the
 * attention embedding of the other endpoint of pair i replaces its memory in the new raw message.  n_positive = 0 (a negative call) runs no
 * attention at all.  n_positive, state, chronological order, workspace and argument checks as for dygnn_tgn_forward_step; out_dst must
 * follow out_src (one [2, batch, F_n] block).  dygnn_dyrep_forward_levels: the levels are those of the first n_positive pairs
 * (dygnn_tgn_forward_levels' layout with batch = n_positive; not read when n_positive = 0).  Inference only.
 * ---------------------------------------------------------------------------------------- */
size_t dygnn_dyrep_workspace_bytes(const dygnn_tgat_config* cfg_host, int64_t num_nodes, int64_t batch);
int dygnn_dyrep_forward_step(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_rnn_weights* rnn_host,
                             const dygnn_csr* csr_host, const float* node_feat, const float* edge_feat, const dygnn_tgn_state* state_host,
                             const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids /* [n_positive] */,
                             int64_t batch, int64_t n_positive, float* out_src, float* out_dst,
                             void* workspace, size_t workspace_bytes, dygnn_stream_t stream);
int dygnn_dyrep_forward_levels(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_rnn_weights* rnn_host,
                               const dygnn_tgat_levels* levels_host, const float* node_feat, const float* edge_feat,
                               const dygnn_tgn_state* state_host, const int64_t* src, const int64_t* dst, const double* times,
                               const int64_t* edge_ids /* [n_positive] */, int64_t batch, int64_t n_positive, float* out_src, float* out_dst,
                               void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* ---- training: train_link_prediction.py:229-257 on the HIP path ------------------------------------
 * dygnn_dygformer_train_forward = models/DyGFormer.py:68-194 in TRAIN mode: dropout (probability dropout_p) on the attention
 * probabilities, the attention output and the FFN (models/DyGFormer.py:429-431, :456-460), masks drawn from a counter-based
 * generator keyed by `seed` (statistically, not bitwise, the reference's torch masks; dropout_p = 0 reproduces the eval
 * forward).  It keeps every activation the backward pass needs in `workspace` (size from
 * dygnn_dygformer_train_workspace_bytes; must stay untouched until dygnn_dygformer_backward of the same call returns) and
 * writes this call's padded lengths (S_src, S_dst) to seq_lens_host[2] (one host synchronisation of `stream`) — unless the caller
 * passes them in (both > 0, e.g. obtained with dygnn_window_lengths on a side stream), in which case the call stays asynchronous.
 * `packed` (may be NULL) = the kernel-ready copy of the CURRENT weights (dygnn_dygformer_pack / dygnn_dygformer_repack): with it, and a
 * shape the fused kernel takes, the forward is ONE kernel (the inference kernel plus dropout and the activation stores); without it the
 * product-by-product path runs.  Same results within fp32 rounding, same workspace contents for dygnn_dygformer_backward.
 * dygnn_dygformer_backward: `grads` has the layout of dygnn_dygformer_weights but its pointers are WRITABLE device buffers
 * of the parameter shapes that MUST BE ZERO on entry (the reductions accumulate into them); on return each holds
 * d(sum(out_src*grad_out_src) + sum(out_dst*grad_out_dst))/dparam.
 * The feature tables receive no gradient (constants in the reference, models/DyGFormer.py:28-29).
 * `packed` (may be NULL): the buffer the forward was given; with it the FFN blocks run backward as one fused kernel per layer. */
size_t dygnn_dygformer_train_workspace_bytes(const dygnn_dygformer_config* cfg_host, int64_t batch);
int dygnn_dygformer_train_forward(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                                  const dygnn_csr* csr_host, const float* node_feat, const float* edge_feat,
                                  const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                                  float dropout_p, uint64_t seed, float* out_src, float* out_dst,
                                  void* workspace, size_t workspace_bytes, int32_t* seq_lens_host, const void* packed,
                                  dygnn_stream_t stream);
int dygnn_dygformer_backward(const dygnn_dygformer_config* cfg_host, const dygnn_dygformer_weights* w_host,
                             const dygnn_dygformer_weights* grads_host, const float* grad_out_src, const float* grad_out_dst,
                             int64_t batch, float dropout_p, uint64_t seed, const int32_t* seq_lens_host,
                             void* workspace, size_t workspace_bytes, const void* packed, dygnn_stream_t stream);

/* TGAT training (models/TGAT.py:48-136 in TRAIN mode, trained by train_link_prediction.py:170-185, :242-257).
 * dygnn_tgat_train_forward: the forward of dygnn_tgat_forward (`levels` == NULL: `recent` sampling on csr from src / dst / times) or of
 * dygnn_tgat_forward_levels (`levels` given: host-replayed random draws; csr / src / dst / times may be NULL), with dropout (probability
 * dropout_p) on the attention probabilities and on the residual_fc output (models/modules.py:187, :196), masks drawn from a counter-based
 * generator keyed by `seed` (dropout_p = 0 reproduces the eval forward).  Every level entry is computed as its own row (the reference's
 * recursion, no de-duplication).  `workspace` (size from dygnn_tgat_train_workspace_bytes) holds every activation the backward pass reads
 * and belongs to ONE call: it, node_feat and edge_feat must stay untouched until dygnn_tgat_backward of the same call returns.
 * dygnn_tgat_backward: `grads` has the layout of dygnn_tgat_weights, its pointers are WRITABLE device buffers of the parameter shapes that
 * MUST BE ZERO on entry (the reductions accumulate into them); on return each holds
 * d(sum(out_src*grad_out_src) + sum(out_dst*grad_out_dst))/dparam.  The feature tables receive no gradient (constants in the reference,
 * models/TGAT.py:26-27).  Configurations: those dygnn_tgat_forward takes with node_feat_dim + edge_feat_dim + time_feat_dim <= 1024
 * (else DYGNN_E_UNSUPPORTED). */
size_t dygnn_tgat_train_workspace_bytes(const dygnn_tgat_config* cfg_host, int64_t batch);
int dygnn_tgat_train_forward(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_csr* csr_host,
                             const dygnn_tgat_levels* levels_host, const float* node_feat, const float* edge_feat,
                             const int64_t* src, const int64_t* dst, const double* times, int64_t batch, float dropout_p, uint64_t seed,
                             float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);
int dygnn_tgat_backward(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_tgat_weights* grads_host,
                        const float* grad_out_src, const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed,
                        void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* TGN training (models/MemoryModel.py:87-168 in TRAIN mode, trained by train_link_prediction.py:186-207, :242-264).
 * dygnn_tgn_train_forward: the forward of dygnn_tgn_forward_step (`levels` == NULL: `recent` sampling on csr) or of dygnn_tgn_forward_levels
 * (`levels` given: host-replayed random draws), its layers in train mode as dygnn_tgat_train_forward runs them (dropout on the attention
 * probabilities and on the residual_fc output, masks keyed by `seed`, every level entry its own row) over feat0 = updated memory + raw
 * features.  The first n_positive pairs are positive edges: their nodes' updated memories are persisted and their new raw messages stored by
 * the code of the inference call, so the state a call leaves is bit-identical to the one dygnn_tgn_forward_step leaves, whatever dropout_p is.
 * `workspace` (size from dygnn_tgn_train_workspace_bytes; 0 for configurations the call refuses) belongs to ONE call and holds everything the
 * backward pass reads, including copies of the pending messages and stored memories the GRU consumed: dygnn_tgn_backward reads nothing of
 * `state`, which a positive call (this one or a later one) has overwritten by then.  edge_feat must stay untouched until it returns.
 * dygnn_tgn_backward (num_nodes = state->num_nodes of the forward call): `grads` as for dygnn_tgat_backward, `gru_grads` the four GRUCell
 * tensors; all WRITABLE device buffers of the parameter shapes that MUST BE ZERO on entry.  On return each holds
 * d(sum(out_src*grad_out_src) + sum(out_dst*grad_out_dst))/dparam: the layers and the time encoder through the attention, the GRUCell through
 * the updated memories of the nodes that had a pending message (their message and stored memory are constants, MemoryModel.py:374-387,
 * :461-487).  The gradient of a node's feat0 row is the sum over every place the call read it, accumulated with float atomics: parameter
 * gradients are not bit-reproducible run to run; the forward outputs and the committed state are.  Nothing flows through the state commit
 * or from call to call.  Configurations: those dygnn_tgn_forward_step and dygnn_tgat_train_forward both take. */
typedef struct dygnn_gru_grads {            /* layout of dygnn_gru_weights, writable                                           */
    float *weight_ih, *weight_hh;
    float *bias_ih, *bias_hh;
} dygnn_gru_grads;
size_t dygnn_tgn_train_workspace_bytes(const dygnn_tgat_config* cfg_host, int64_t num_nodes, int64_t batch);
int dygnn_tgn_train_forward(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_gru_weights* gru_host,
                            const dygnn_csr* csr_host, const dygnn_tgat_levels* levels_host /* NULL: recent */, const float* node_feat,
                            const float* edge_feat, const dygnn_tgn_state* state_host, const int64_t* src, const int64_t* dst,
                            const double* times, const int64_t* edge_ids /* [n_positive] */, int64_t batch, int64_t n_positive,
                            float dropout_p, uint64_t seed, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes,
                            dygnn_stream_t stream);
int dygnn_tgn_backward(const dygnn_tgat_config* cfg_host, const dygnn_tgat_weights* w_host, const dygnn_gru_weights* gru_host,
                       const dygnn_tgat_weights* grads_host, const dygnn_gru_grads* gru_grads_host, const float* grad_out_src,
                       const float* grad_out_dst, int64_t num_nodes, int64_t batch, float dropout_p, uint64_t seed,
                       void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* Caller-side link predictor, fused: sigmoid(MergeLayer(a,b)) with
 * MergeLayer = fc2(relu(fc1(cat(a,b)))) (models/modules.py:57-68; evaluate_models_utils.py:140-141).
 * a,b [n,dim]; fc1 [hidden, 2*dim]; fc2 [1,hidden]; out [n]. */
int dygnn_merge_layer_sigmoid(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden,
                              const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                              float* out, dygnn_stream_t stream);
/* Which forward kernel dygnn_merge_layer_sigmoid / dygnn_merge_layer_logits run for these sizes (host only, nothing is launched):
 * 0 = one workgroup per row, 1 = 4 rows per workgroup, 2 = 16 rows per workgroup, 3 = one wave per 16 rows on the matrix cores;
 * < 0 = the sizes are refused (DYGNN_E_INVALID, message in dygnn_last_error).  The forward takes any dim and hidden whose single row
 * (2 dim + 4 floats) fits 64 KB of LDS, at every n. */
int32_t dygnn_merge_layer_forward_path(int64_t n, int32_t dim, int32_t hidden);
/* The same head for the TRAINING step (train_link_prediction.py:241-257): the logits z = MergeLayer(a, b) [n] (output_dim 1) and their
 * backward pass.  grad_logits = dL/dz [n]; grad_a, grad_b [n,dim] are written; the four parameter gradients are ACCUMULATED into buffers the
 * caller has zeroed; `workspace` = n * hidden floats, 16-byte aligned like a and b.  dim and hidden multiples of 4, hidden <= 192. */
int dygnn_merge_layer_logits(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden,
                             const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                             float* out, dygnn_stream_t stream);
int dygnn_merge_layer_backward(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden,
                               const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* grad_logits,
                               float* grad_a, float* grad_b, float* grad_fc1_w, float* grad_fc1_b, float* grad_fc2_w, float* grad_fc2_b,
                               float* workspace, dygnn_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * GraphMixer.compute_node_temporal_embeddings (models/GraphMixer.py:70-150), eval mode, `recent` sampling, fp32.  Per root (v, t):
 *   link encoder: the K = num_tokens most recent interactions before t (dygnn_sample_recent's layout: right-aligned, zero padded) as tokens
 *     [edge_feat[eid] | cos(w dt + b)] (time features ZERO on padded slots, edge row edge_feat[0]), projection_layer, num_layers MLP-Mixer
 *     blocks (token LayerNorm + FFN K -> token_hidden_dim -> K over the token axis, channel LayerNorm + FFN C -> channel_hidden_dim -> C,
 *     exact GELU, residuals), mean over the K tokens;
 *   node encoder: m = min(history length, time_gap) most recent neighbours: (1 / time_gap) (1 / m) sum node_feat[nbr] (+ node_feat[v]);
 *     m = 0: node_feat[0] / time_gap (the reference's softmax over an all-masked row is uniform).  The neighbour rows are read straight from
 *     the CSR row: no [n, time_gap] array exists, and the workspace does not depend on time_gap;
 *   output_layer on [link part | node part].
 * One call serves any list of roots ([src ; dst], [src ; dst ; neg_dst], ...); a root's row does not depend on the other roots.
 * Configurations: feature dims multiples of 4, each <= 256; 2 <= num_tokens <= 32; 1 <= token_hidden_dim <= 16; channel_hidden_dim a
 * multiple of 16, <= 1024; 1 <= num_layers <= DYGNN_MAX_LAYERS; time_gap >= 1.  Others: DYGNN_E_UNSUPPORTED.  num_neighbors <= 0,
 * time_gap <= 0 and num_neighbors != num_tokens are DYGNN_E_INVALID.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_graphmixer_config {
    int32_t node_feat_dim, edge_feat_dim, time_feat_dim;   /* F_n, C = num_channels, F_t                                        */
    int32_t num_tokens;                                    /* K: the length of the token LayerNorm / FFN                        */
    int32_t num_layers;
    int32_t token_hidden_dim;                              /* int(token_dim_expansion_factor * num_tokens)                      */
    int32_t channel_hidden_dim;                            /* int(channel_dim_expansion_factor * C)                             */
    int32_t num_neighbors;                                 /* of the call; must equal num_tokens                                */
    int32_t time_gap;                                      /* G of the call                                                     */
    int32_t num_node_rows;                                 /* rows of node_feat (root ids outside read row 0); 0: csr num_nodes */
} dygnn_graphmixer_config;

typedef struct dygnn_mixer_layer_weights {                 /* mlp_mixers.l.*, PyTorch [out,in] layout                           */
    const float *token_norm_w, *token_norm_b;              /* token_norm.{weight,bias}                          [K]             */
    const float *token_fc0_w, *token_fc0_b;                /* token_feedforward.ffn.0          [token_hidden,K],[token_hidden]  */
    const float *token_fc1_w, *token_fc1_b;                /* token_feedforward.ffn.3          [K,token_hidden],[K]             */
    const float *channel_norm_w, *channel_norm_b;          /* channel_norm.{weight,bias}                        [C]             */
    const float *channel_fc0_w, *channel_fc0_b;            /* channel_feedforward.ffn.0    [channel_hidden,C],[channel_hidden]  */
    const float *channel_fc1_w, *channel_fc1_b;            /* channel_feedforward.ffn.3    [C,channel_hidden],[C]               */
} dygnn_mixer_layer_weights;

typedef struct dygnn_graphmixer_weights {
    const float *time_w, *time_b;                          /* time_encoder.w.{weight,bias}                   [F_t,1],[F_t]      */
    const float *proj_w, *proj_b;                          /* projection_layer                             [C,C+F_t],[C]        */
    dygnn_mixer_layer_weights layers[DYGNN_MAX_LAYERS];
    const float *output_w, *output_b;                      /* output_layer                              [F_n,C+F_n],[F_n]       */
} dygnn_graphmixer_weights;

/* Optional intermediates of the first min(rows, n) roots (device buffers, each nullable) */
typedef struct dygnn_graphmixer_taps {
    int64_t rows;
    float* projection;                                     /* [rows, K, C] projection_layer output                              */
    float* layer_out[DYGNN_MAX_LAYERS];                    /* [rows, K, C] output of Mixer block l                              */
    float* token_mean;                                     /* [rows, C]                                                         */
    float* node_term;                                      /* [rows, F_n] node-encoder term BEFORE node_feat[v] is added        */
} dygnn_graphmixer_taps;

/* DYGNN_OK, or why dygnn_graphmixer_workspace_bytes returned 0 (message in dygnn_last_error) */
int dygnn_graphmixer_check(const dygnn_graphmixer_config* cfg_host);
/* n_roots * (K * C + F_n) floats (+ alignment): the token activations and the node-encoder term.  0 = the configuration is refused. */
size_t dygnn_graphmixer_workspace_bytes(const dygnn_graphmixer_config* cfg_host, int64_t n_roots);
int dygnn_graphmixer_forward(const dygnn_graphmixer_config* cfg_host, const dygnn_graphmixer_weights* w_host, const dygnn_csr* csr_host,
                             const float* node_feat, const float* edge_feat, const int64_t* nodes, const double* times, int64_t n,
                             float* out /* [n, F_n] */, const dygnn_graphmixer_taps* taps_host /* or NULL */,
                             void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* GraphMixer training (dyglib_amd/csrc/graphmixer_train.hip): the train-mode forward of one compute_node_temporal_embeddings call on n roots
 * (a training call: [src ; dst]) and its backward pass; `recent` sampling.  Dropout (p in [0, 1)) after the GELU and on the output of the
 * token and of the channel FFN of every block, masks from the counter-based generator of dropout.h: site = 4 layer + s, q = the root's
 * index in the call, elements numbered as the reference's dense activations: s = 0 token hidden [n, C, Kh]: (q C + ch) Kh + i; s = 1 token
 * FFN output [n, C, K]: (q C + ch) K + j; s = 2 channel hidden [n, K, H]: (q K + j) H + h; s = 3 channel FFN output [n, K, C]:
 * (q K + j) C + c.  dropout_p = 0 is the inference forward within fp32 rounding.  The workspace belongs to ONE forward / backward pair: it
 * keeps the gathered token rows and every activation the backward pass reads (nothing in it has a time_gap dimension; the caller's
 * arrays and tables are not read again).  Arguments are checked as dygnn_graphmixer_forward checks them.
 * workspace_bytes: 0 = the configuration or n_roots is refused (message in dygnn_last_error).  n == 0: DYGNN_OK, nothing launched. */
size_t dygnn_graphmixer_train_workspace_bytes(const dygnn_graphmixer_config* cfg_host, int64_t n_roots);
int dygnn_graphmixer_train_forward(const dygnn_graphmixer_config* cfg_host, const dygnn_graphmixer_weights* w_host, const dygnn_csr* csr_host,
                                   const float* node_feat, const float* edge_feat, const int64_t* nodes, const double* times, int64_t n,
                                   float dropout_p, uint64_t seed, float* out /* [n, F_n] */, void* workspace, size_t workspace_bytes,
                                   dygnn_stream_t stream);
/* grads: a dygnn_graphmixer_weights of gradient buffers (same shapes as the weights), ZEROED by the caller: every tensor is accumulated
 * into; its time_w / time_b may be NULL and are never written (the time encoder is frozen).  The four matrices projection_layer, output_layer
 * and channel fc0 / fc1 are summed with float atomics (not bit-reproducible run to run); every bias, both LayerNorms and the token FFN's
 * matrices are fixed-order sums (the same bits run to run). */
int dygnn_graphmixer_backward(const dygnn_graphmixer_config* cfg_host, const dygnn_graphmixer_weights* w_host,
                              const dygnn_graphmixer_weights* grads_host, const float* grad_out /* [n, F_n] */, int64_t n, float dropout_p,
                              uint64_t seed, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);


/* ------------------------------------------------------------------------------------------
 * TCL.compute_src_dst_node_temporal_embeddings (models/TCL.py:56-154, TransformerEncoder models/modules.py:209-266), eval mode, fp32.
 * The call works on SIDES and PAIRS.  A side is one root (v, t) with its K sampled neighbours, as get_historical_neighbors returns them
 * (any strategy: sampling is not part of the call).  Its sequence has S = K + 1 positions: position 0 is the root itself (edge id 0,
 * time t), positions 1..K the neighbours.  Encoder input of a position:
 *     node_proj(node_feat[id]) + edge_proj(edge_feat[eid]) + time_proj(cos(w float32(t - t_nbr) + b)) + depth_embedding[position]
 * (a padded slot, id 0, reads node_feat[0], edge_feat[0] and dt = t - 0).  A pair names two sides a, b.  Every layer applies the SAME
 * transformer block four times: self-attention on a, on b, then a over b's self-attended sequence and b over a's (both read the
 * self-attended sequences).  Every attention masks the keys whose node id is 0.  Block: nn.MultiheadAttention (scale 1 / sqrt(d / heads)),
 * LayerNorm(x + attn), Linear d -> 4d, ReLU, Linear 4d -> d, LayerNorm(residual).  out_a / out_b = output_layer(position 0) after the last
 * layer.  A side named by several pairs has its encoder input and its first self-attention computed once.  A pair's rows do not depend on
 * the other pairs of the call.  A sequence without any valid key (root id 0 and no neighbour) attends to nothing: its attention term is
 * zero (the reference returns NaN there).
 * Configurations: 1 <= num_neighbors <= 63; d = node_feat_dim, edge_feat_dim, time_feat_dim multiples of 4, each <= 256; 1 <= num_heads <= 8
 * dividing d; 1 <= num_layers <= DYGNN_MAX_LAYERS.  Others: DYGNN_E_UNSUPPORTED.  num_neighbors <= 0: DYGNN_E_INVALID.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_tcl_config {
    int32_t node_feat_dim, edge_feat_dim, time_feat_dim;   /* d = F_n, F_e, F_t                                                 */
    int32_t num_neighbors;                                 /* K of the call; the depth embedding has K + 1 rows                 */
    int32_t num_layers, num_heads;
    int32_t num_node_rows, num_edge_rows;                  /* rows of node_feat / edge_feat: ids outside read row 0             */
} dygnn_tcl_config;

typedef struct dygnn_tcl_layer_weights {                   /* transformers.l.*, PyTorch [out,in] layout                         */
    const float *in_proj_w, *in_proj_b;                    /* multi_head_attention.in_proj_{weight,bias}        [3d,d],[3d]     */
    const float *out_proj_w, *out_proj_b;                  /* multi_head_attention.out_proj                     [d,d],[d]       */
    const float *fc0_w, *fc0_b;                            /* linear_layers.0                                   [4d,d],[4d]     */
    const float *fc1_w, *fc1_b;                            /* linear_layers.1                                   [d,4d],[d]      */
    const float *norm0_w, *norm0_b;                        /* norm_layers.0                                     [d]             */
    const float *norm1_w, *norm1_b;                        /* norm_layers.1                                     [d]             */
} dygnn_tcl_layer_weights;

typedef struct dygnn_tcl_weights {
    const float *time_w, *time_b;                          /* time_encoder.w.{weight,bias}                   [F_t,1],[F_t]      */
    const float *depth_w;                                  /* depth_embedding.weight                         [K+1,d]            */
    const float *proj_node_w, *proj_node_b;                /* projection_layer.node                          [d,d],[d]          */
    const float *proj_edge_w, *proj_edge_b;                /* projection_layer.edge                          [d,F_e],[d]        */
    const float *proj_time_w, *proj_time_b;                /* projection_layer.time                          [d,F_t],[d]        */
    dygnn_tcl_layer_weights layers[DYGNN_MAX_LAYERS];
    const float *output_w, *output_b;                      /* output_layer                                   [d,d],[d]          */
} dygnn_tcl_weights;

/* Optional intermediates of the first min(rows, n_pairs) pairs (device buffers, each nullable); index 1 of the second axis is side a / b.
 * Values at padded positions are unspecified. */
typedef struct dygnn_tcl_taps {
    int64_t rows;
    float* encoder_input;                                  /* [rows, 2, S, d]                                                   */
    float* layer_out[DYGNN_MAX_LAYERS];                    /* [rows, 2, S, d] the two cross-attention outputs of layer l        */
} dygnn_tcl_taps;

/* DYGNN_OK, or why dygnn_tcl_workspace_bytes returned 0 (message in dygnn_last_error) */
int dygnn_tcl_check(const dygnn_tcl_config* cfg_host);
/* Activations of the sides and of the 2 n_pairs sequences of the pairs, their Q / K / V and attention output, and the pair index.
 * 0 = the configuration is refused. */
size_t dygnn_tcl_workspace_bytes(const dygnn_tcl_config* cfg_host, int64_t n_sides, int64_t n_pairs);
/* side_* / nbr_* are device arrays; pair_a / pair_b are HOST arrays (checked against [0, n_sides) before any launch and copied). */
int dygnn_tcl_forward(const dygnn_tcl_config* cfg_host, const dygnn_tcl_weights* w_host, const float* node_feat, const float* edge_feat,
                      const int64_t* side_root /* [n_sides] */, const double* side_time /* [n_sides] */,
                      const int64_t* nbr_id /* [n_sides, K] */, const int64_t* nbr_eid /* [n_sides, K] */, const float* nbr_t /* [n_sides, K] */,
                      int64_t n_sides, const int32_t* pair_a_host /* [n_pairs] */, const int32_t* pair_b_host /* [n_pairs] */, int64_t n_pairs,
                      float* out_a /* [n_pairs, d] */, float* out_b /* [n_pairs, d] */, const dygnn_tcl_taps* taps_host /* or NULL */,
                      void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* TCL training (dyglib_amd/csrc/tcl_train.hip): the train-mode forward of one compute_src_dst_node_temporal_embeddings call and its backward
 * pass.  The call's 2 batch sides are [src ; dst] and pair p is (side p, side batch + p): no index vector, no stream synchronisation.
 * Dropout (p in [0, 1)) on the attention probabilities, the attention block's output, relu(fc0) and the fc1 output of every block, masks
 * from the counter-based generator of dropout.h: site = 8 layer + 4 stage + {0, 1, 2, 3} (stage 0 = self, 1 = cross), sequence index
 * q = 2 p + side, element ((q H + h) S + i) S + j (site 0), (q S + i) d + c (sites 1, 3), (q S + i) 4d + c (site 2).  dropout_p = 0 is the
 * inference forward within fp32 rounding.  The workspace belongs to ONE forward / backward pair: it keeps the sampled sides and every
 * activation the backward pass reads; node_feat / edge_feat must stay alive until the backward has run (it regathers their rows).
 * workspace_bytes: 0 = the configuration or the batch is refused (message in dygnn_last_error).  batch == 0: DYGNN_OK, nothing launched. */
size_t dygnn_tcl_train_workspace_bytes(const dygnn_tcl_config* cfg_host, int64_t batch);
int dygnn_tcl_train_forward(const dygnn_tcl_config* cfg_host, const dygnn_tcl_weights* w_host, const float* node_feat, const float* edge_feat,
                            const int64_t* side_root /* [2 batch] */, const double* side_time /* [2 batch] */,
                            const int64_t* nbr_id /* [2 batch, K] */, const int64_t* nbr_eid /* [2 batch, K] */, const float* nbr_t /* [2 batch, K] */,
                            int64_t batch, float dropout_p, uint64_t seed, float* out_src /* [batch, d] */, float* out_dst /* [batch, d] */,
                            void* workspace, size_t workspace_bytes, dygnn_stream_t stream);
/* grads: a dygnn_tcl_weights of gradient buffers (same shapes as the weights), ZEROED by the caller: every tensor is accumulated into.
 * Weight matrices are summed with float atomics (not bit-reproducible run to run); biases, LayerNorm, depth and time-encoder gradients
 * are fixed-order column sums. */
int dygnn_tcl_backward(const dygnn_tcl_config* cfg_host, const dygnn_tcl_weights* w_host, const dygnn_tcl_weights* grads_host,
                       const float* grad_out_src /* [batch, d] */, const float* grad_out_dst /* [batch, d] */, int64_t batch, float dropout_p,
                       uint64_t seed, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CAWN.compute_src_dst_node_temporal_embeddings (models/CAWN.py:48-396), eval mode, fp32 (dyglib_amd/csrc/cawn.hip).
 * The call works on SIDES and PAIRS, on PRE-SAMPLED hop arrays (any strategy: sampling is not part of the call).  A side is one target
 * (v, t) with the arrays get_multi_hop_neighbors returns for it: hop h = 1..W holds k^h (node id, edge id, float32 time).  Walk j of the
 * M = k^W walks of a side is [target, hop1[j / k^(W-1)], ..., hopW[j]]; position 0 carries edge id 0 and time t; the valid length is the
 * number of non-zero ids (zeros are a suffix).  A pair names two sides a, b.  Per pair, every node id of the two trees gets the counts
 * [2][W + 1] (row 0: appearances in a's tree, row 1: in b's, column = hop, each appearance 1 / k^hop; the entry of id 0 is zero) and the
 * position feature sum_rows MLP(W + 1 -> P -> P, ReLU).  Input of a walk position: [node_feat[id] | cos(w float32(t - t_pos) + b) |
 * edge_feat[eid] | position feature].  Two BiLSTMs (input D = F_n + F_e + F_t + P, hidden D / 2 per direction; input P, hidden P / 2) give
 * their output at the last valid position; their concatenation goes through projection_layers[0] (-> attention_dim = D / 2 rounded up to a
 * multiple of the heads), one TransformerEncoder block over the M walks of a side (no mask), the mean over the walks and
 * projection_layers[1] (-> F_n).  A pair's rows do not depend on the other pairs of the call; a side named by several pairs is encoded
 * once per pair (its position features depend on the partner).
 * Configurations: walk_length 1 or 2; k^W <= 128; F_n, F_e, F_t multiples of 4, P even, each <= 256; attention_dim a multiple of 4, <= 512, and
 * attention_dim / heads <= 64.  Others: DYGNN_E_UNSUPPORTED, the message names the value.  num_neighbors or walk_length <= 0: DYGNN_E_INVALID.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_cawn_config {
    int32_t node_feat_dim, edge_feat_dim, time_feat_dim, position_feat_dim;   /* F_n, F_e, F_t, P                                */
    int32_t walk_length, num_neighbors, num_walk_heads;                       /* W, k, heads                                     */
    int32_t num_node_rows, num_edge_rows;                  /* rows of node_feat / edge_feat: ids outside read row 0             */
} dygnn_cawn_config;

typedef struct dygnn_cawn_lstm_weights {                   /* one direction of an nn.LSTM with hidden size H, gates i, f, g, o  */
    const float *w_ih, *w_hh;                              /* weight_ih_l0 [4H,in], weight_hh_l0 [4H,H]                         */
    const float *b_ih, *b_hh;                              /* bias_ih_l0 [4H], bias_hh_l0 [4H]                                  */
} dygnn_cawn_lstm_weights;

typedef struct dygnn_cawn_weights {                        /* the order of the reference's state_dict                           */
    const float *time_w, *time_b;                          /* time_encoder.w.{weight,bias}                      [F_t,1],[F_t]   */
    const float *pos_w0, *pos_b0;                          /* position_encoder.position_encode_layer.0          [P,W+1],[P]     */
    const float *pos_w1, *pos_b1;                          /* position_encoder.position_encode_layer.2          [P,P],[P]       */
    dygnn_cawn_lstm_weights feature[2];                    /* walk_encoder.feature_encoder.bilstm_encoder: forward, reverse     */
    dygnn_cawn_lstm_weights position[2];                   /* walk_encoder.position_encoder.bilstm_encoder: forward, reverse    */
    dygnn_tcl_layer_weights attn;                          /* walk_encoder.transformer_encoder.*, d = attention_dim             */
    const float *proj0_w, *proj0_b;                        /* walk_encoder.projection_layers.0    [attention_dim, D + P]        */
    const float *proj1_w, *proj1_b;                        /* walk_encoder.projection_layers.1    [F_n, attention_dim]          */
} dygnn_cawn_weights;

typedef struct dygnn_cawn_hops {                           /* device arrays [n_sides, k^h], index h - 1; hop 2 NULL when W = 1   */
    const int64_t* id[2];
    const int64_t* eid[2];
    const float* t[2];
} dygnn_cawn_hops;

/* Optional intermediates of the first min(rows, n_pairs) pairs (device buffers, each nullable); index 1 of the second axis is side a / b. */
typedef struct dygnn_cawn_taps {
    int64_t rows;
    int64_t* walk_ids;                                     /* [rows, 2, M, W+1]                                                 */
    float* counts;                                         /* [rows, 2, M, W+1, 2, W+1] the counts of every walk position       */
    float* feature_out;                                    /* [rows, 2, M, D]   feature encoder output (D even)                 */
    float* position_out;                                   /* [rows, 2, M, P]   position encoder output                         */
    float* attn_in;                                        /* [rows, 2, M, attention_dim] projection_layers[0] output           */
    float* attn_out;                                       /* [rows, 2, M, attention_dim] transformer output                    */
} dygnn_cawn_taps;

/* DYGNN_OK, or why dygnn_cawn_workspace_bytes returned 0 (message in dygnn_last_error) */
int dygnn_cawn_check(const dygnn_cawn_config* cfg_host);
/* Per pair: the position tables; per sequence (2 n_pairs): the LSTM states, the encoder outputs of the M walks, the transformer's
 * activations.  0 = the configuration is refused. */
size_t dygnn_cawn_workspace_bytes(const dygnn_cawn_config* cfg_host, int64_t n_sides, int64_t n_pairs);
/* side_* and the hop arrays are device arrays; pair_a / pair_b are HOST arrays (checked against [0, n_sides) before any launch and copied). */
int dygnn_cawn_forward(const dygnn_cawn_config* cfg_host, const dygnn_cawn_weights* w_host, const float* node_feat, const float* edge_feat,
                       const int64_t* side_root /* [n_sides] */, const double* side_time /* [n_sides] */, const dygnn_cawn_hops* hops_host,
                       int64_t n_sides, const int32_t* pair_a_host /* [n_pairs] */, const int32_t* pair_b_host /* [n_pairs] */, int64_t n_pairs,
                       float* out_a /* [n_pairs, F_n] */, float* out_b /* [n_pairs, F_n] */, const dygnn_cawn_taps* taps_host /* or NULL */,
                       void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* CAWN training (dyglib_amd/csrc/cawn_train.hip): the train-mode forward of one compute_src_dst_node_temporal_embeddings call and its
 * backward pass.  The call's 2 batch sides are [src ; dst] (side_root, side_time and the hop arrays [2 batch, k^h]) and pair p is
 * (side p, side batch + p): no index vector, no stream synchronisation.  Dropout (p in [0, 1)) on the attention probabilities, the
 * attention block's output, relu(fc0) and the fc1 output of the walk encoder's transformer block, masks from the counter-based generator of
 * dropout.h: sites 0 .. 3, sequence index q = 2 p + side, element ((q H + h) M + i) M + j (site 0), (q M + i) A + c (sites 1, 3),
 * (q M + i) 4A + c (site 2), A = attention_dim.  dropout_p = 0 is the inference forward within fp32 rounding.  The workspace belongs to
 * ONE forward / backward pair: it keeps the gathered input rows and every activation the backward pass reads (the feature tables and the
 * hop arrays are not read again).  Configurations: those of dygnn_cawn_check with at most 64 walks (k^W <= 64; more: DYGNN_E_UNSUPPORTED,
 * the message names the value).  workspace_bytes: 0 = the configuration or the batch is refused (message in dygnn_last_error).
 * batch == 0: DYGNN_OK, nothing launched. */
size_t dygnn_cawn_train_workspace_bytes(const dygnn_cawn_config* cfg_host, int64_t batch);
int dygnn_cawn_train_forward(const dygnn_cawn_config* cfg_host, const dygnn_cawn_weights* w_host, const float* node_feat, const float* edge_feat,
                             const int64_t* side_root /* [2 batch] */, const double* side_time /* [2 batch] */,
                             const dygnn_cawn_hops* hops_host /* [2 batch, k^h] */, int64_t batch, float dropout_p, uint64_t seed,
                             float* out_src /* [batch, F_n] */, float* out_dst /* [batch, F_n] */, void* workspace, size_t workspace_bytes,
                             dygnn_stream_t stream);
/* grads: a dygnn_cawn_weights of gradient buffers (same shapes as the weights), ZEROED by the caller: every tensor is accumulated into
 * (feature[1].w_hh and position[1].w_hh, the reverse direction's hidden weights, are left at zero: that is their gradient).  Weight
 * matrices are summed with float atomics (not bit-reproducible run to run); biases (b_ih and b_hh get the same sum), LayerNorm,
 * time-encoder gradients and the position-feature scatter are fixed-order sums. */
int dygnn_cawn_backward(const dygnn_cawn_config* cfg_host, const dygnn_cawn_weights* w_host, const dygnn_cawn_weights* grads_host,
                        const float* grad_out_src /* [batch, F_n] */, const float* grad_out_dst /* [batch, F_n] */, int64_t batch, float dropout_p,
                        uint64_t seed, void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* Evaluation metrics on the device, replacing the scikit-learn host round trip of
 * get_link_prediction_metrics / get_node_classification_metrics (utils/metrics.py:5-34; called per batch at
 * evaluate_models_utils.py:139-150 and per evaluation at :245-249).  predicts / labels: [n_groups, group_size] float32
 * (labels 0.0 / 1.0, as the reference builds them with ones_like / zeros_like); one group = one call of the reference
 * function.  Outputs (device, each nullable): average_precision [n_groups] (average_precision_score), roc_auc [n_groups]
 * (roc_auc_score; NaN where it would raise), bce_loss [n_groups] (torch.nn.BCELoss, mean; evaluate_models_utils.py:145),
 * status [n_groups] int32 (1 = only one class present: roc_auc_score raises ValueError there, and so does the wrapper).
 * Rank counts are exact; sums are float64 in a fixed order (reproducible); agreement with scikit-learn <= 1e-12. */
size_t dygnn_link_metrics_workspace_bytes(int64_t group_size, int64_t n_groups);
int dygnn_link_metrics(const float* predicts, const float* labels, int64_t group_size, int64_t n_groups,
                       double* average_precision, double* roc_auc, double* bce_loss, int32_t* status,
                       void* workspace, size_t workspace_bytes, dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * EdgeBank (models/EdgeBank.py:7-121; evaluated at evaluate_models_utils.py:303-350): a directed edge (src, dst) scores 1.0 if its pair is
 * in memory and 0.0 otherwise.  The history is a persistent hash table on the device that grows by position ranges of one edge list
 * (src / dst int64, times float64, device arrays; position = index in them), so an evaluation inserts each edge once instead of
 * rebuilding a set per batch.  Layout, hash and the argument for run-to-run bit-identical state: dyglib_amd/csrc/edgebank.hip.
 *
 * The caller owns the table: `buffer` is device memory of dygnn_edgebank_table_bytes(max_edges) bytes (0 = max_edges refused: negative or
 * above 2^30), `num_edges` is written by reset / insert / evaluate and read by the checks (H against the edges inserted), all on the host.
 * Ids must lie in [0, 2^31): the caller checks (the Python layer raises ValueError); the kernels skip other ids and set bit 0 of the int32
 * word at byte 32 of the buffer (bit 1: table overfilled, bit 2: an inserted key was not found again; both impossible within max_edges).
 *
 * memory mode 0 unlimited_memory: the pair occurs in the history.  1 repeat_threshold_memory: count(pair) >= H / D in float64, D = distinct
 * pairs.  2 time_window_memory: max time of the pair >= start, with window mode 0 fixed_proportion: start = start_time, which the caller
 * computes (np.quantile(times[:H], 1 - proportion), EdgeBank.py:52), or 1 repeat_interval: start = max(times) - S / D computed on the device,
 * S = sum over pairs with n > 1 occurrences of (t[last position] - t[first position]) / (n - 1) (EdgeBank.py:56-68, the mean of consecutive
 * differences telescoped).  The window mode is looked at in memory mode 2 only.  Mode 2 on an empty history is refused (the reference's
 * max() of an empty sequence raises ValueError).
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_edgebank {
    void*   buffer;         /* device, dygnn_edgebank_table_bytes(max_edges) bytes              */
    size_t  buffer_bytes;
    int64_t max_edges;      /* the most edges the table will ever hold                          */
    int64_t num_edges;      /* edges inserted so far = the history length H the table answers for */
} dygnn_edgebank;

size_t dygnn_edgebank_table_bytes(int64_t max_edges);
/* Home slot of a pair in a table for max_edges (host; UINT64_MAX for refused arguments): what tests use to build colliding keys. */
uint64_t dygnn_edgebank_home_slot(int64_t src, int64_t dst, int64_t max_edges);
/* Empties the table (two memsets on `stream`). */
int dygnn_edgebank_reset(dygnn_edgebank* table_host, dygnn_stream_t stream);
/* Inserts positions [first, last) of the edge arrays; first must equal table_host->num_edges (the table holds a prefix). */
int dygnn_edgebank_insert(dygnn_edgebank* table_host, const int64_t* src, const int64_t* dst, const double* times, int64_t first,
                          int64_t last, dygnn_stream_t stream);
/* out[i] = score of (q_src[i], q_dst[i]) against the H = table_host->num_edges edges inserted (another H is refused).  `times` = the edge
 * list's times, needed by repeat_interval only.  Never inserts. */
int dygnn_edgebank_query(const dygnn_edgebank* table_host, const double* times, int32_t mode, int32_t window_mode, int64_t H,
                         double start_time, const int64_t* q_src, const int64_t* q_dst, int64_t n, float* out, dygnn_stream_t stream);
/* A whole evaluation with no host synchronisation: for batch b, insert the edges up to hist_len_host[b] (non-decreasing, starting at or above
 * table_host->num_edges), then score its queries q_src / q_dst [n_batches, queries_per_batch] into out (same shape) with
 * start_times[b] (device, [n_batches]; fixed_proportion only, else may be NULL). */
int dygnn_edgebank_evaluate(dygnn_edgebank* table_host, const int64_t* src, const int64_t* dst, const double* times,
                            const int64_t* hist_len_host, const double* start_times, const int64_t* q_src, const int64_t* q_dst,
                            int64_t n_batches, int64_t queries_per_batch, int32_t mode, int32_t window_mode, float* out,
                            dygnn_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The general fp32 GEMM every backbone's products go through, and the grouped weight-gradient product of the fused trainers, as entry
 * points of their own (what tests/test_gemm_gpu.py drives; the backbones call the same functions inside the library).
 *
 *   C = [relu] (alpha * op(A) . op(B) + bias[n] + beta * C)      per batch z = zb * H + zh, which adds zb * sXb + zh * sXh floats to A, B, C
 *   op(A)[m][k] = tA ? A[k * lda + m] : A[m * lda + k],  op(B)[k][n] = tB ? B[n * ldb + k] : B[k * ldb + n]
 *
 * C is OVERWRITTEN (beta = 0: its old contents are not read, NaN included) or scaled and added to (beta != 0).  Exactly M x N elements per
 * batch are written: nothing between N and ldc, nothing outside the batches.  bias (or NULL) is added once, before relu.
 * Products with batch == 1, K >= 2048 and no relu are split over K and meet in float atomics: C is zeroed first (beta = 0; skipped when
 * c_is_zero says the caller did it), or the parts add onto it (beta = 1).  A split product takes beta 0 or 1 only.
 * colsum_out (or NULL; tA and batch == 1 only): colsum_out[m] += sum_k op(A)[m][k], ACCUMULATED onto what the buffer holds.
 * m_dev (or NULL): device int32 count of live rows, 0 <= *m_dev <= M.  Rows below it are computed.  64-row tiles wholly at or beyond it are
 *   not touched by the kernels, except that a split product with beta = 0 and !c_is_zero has zeroed all M rows.  Rows of the tile that holds
 *   the count, at or beyond it, are unspecified (written from operand rows [count, M), which must be readable).
 * a_kpad: !tA and !tB only; A's rows hold zeros from column K to the next multiple of 4 (lda at least that), which lets a K that is no multiple
 *   of 4 take the LDS-DMA kernel.
 * a_rows (or NULL; !tA only): device int32 table, row m of op(A) is A[a_rows[m]].  Only the LDS-DMA kernel gathers: a call that cannot take it
 *   (see below) is refused.  With m_dev, entries at and beyond the count are not read.
 * No alignment is required for a correct result; alignment picks the kernel (dygnn_mm_path):
 *   0  M < 48 or N < 48: the 64 x 64 scalar-load kernel
 *   2  the LDS-DMA kernel: A, B 16-byte aligned, lda, ldb and the A / B batch strides multiples of 4, K % 4 == 0 (or a_kpad), M % 4 == 0 with tA,
 *      N % 4 == 0 with !tB, and the environment variable DYGNN_MM_DMA (read per call) not "0".  Its float4 epilogue needs C 16-byte aligned,
 *      ldc and the C strides multiples of 4, beta = 0 and no split.
 *   1  everything else.
 * Refused with DYGNN_E_UNSUPPORTED before anything is launched or zeroed: a split product with beta outside {0, 1}; colsum_out with !tA or
 * batch > 1; a_rows with tA; a_rows on a call that is not path 2.  NULL A, B or C, negative sizes, H < 1: DYGNN_E_INVALID.
 * ---------------------------------------------------------------------------------------- */
typedef struct dygnn_mm_args {
    const float*   A;
    const float*   B;
    float*         C;
    const float*   bias;
    float*         colsum_out;
    const int32_t* m_dev;
    const int32_t* a_rows;
    int64_t sAb, sAh, sBb, sBh, sCb, sCh;
    int32_t lda, ldb, ldc;
    int32_t M, N, K;
    int32_t batch, H;
    float   alpha, beta;
    int32_t tA, tB, relu, c_is_zero, a_kpad;
} dygnn_mm_args;

int dygnn_mm(const dygnn_mm_args* a, dygnn_stream_t stream);
/* Which kernel dygnn_mm runs for these arguments: 0, 1 or 2 as above, or the (negative) code dygnn_mm would return.  Host only: nothing is
 * launched and no pointer is followed (their alignment is what counts).  An empty product (M, N or batch 0) launches nothing and reports 0.
 * dygnn_mm_plan also reports the number of K parts (1 = not split) and whether the float4 epilogue is taken (either may be NULL). */
int32_t dygnn_mm_path(const dygnn_mm_args* a);
int32_t dygnn_mm_plan(const dygnn_mm_args* a, int32_t* ksplit, int32_t* float4_epilogue);
/* 1 when a !tA, tB product of these operands takes the LDS-DMA kernel, the only one that accepts a_rows (what the backbones ask before they
 * choose between a row table and a staging copy); the same decision as dygnn_mm_path. */
int32_t dygnn_mm_gathers_rows(const float* A, int32_t lda, const float* B, int32_t ldb, int32_t M, int32_t N, int32_t K);

/* Weight-gradient-shaped products in one grouped split-K launch: C_p[m][n] += sum_k A_p[k][m] * B_p[k][n] for every problem p, all over the
 * same K rows; colsum_p[m] += sum_k A_p[k][m] where colsum is not NULL.  C and colsum ACCUMULATE (float atomics): zero them first.
 * Preconditions, else DYGNN_E_UNSUPPORTED with nothing launched: A and B 16-byte aligned; lda, ldb and N multiples of 4; M a multiple of 4 or
 * lda >= M rounded up to one; at most 4 * DYGNN_MAX_LAYERS + 4 problems.  C, ldc and colsum need no alignment; only M x N elements are touched. */
typedef struct dygnn_dw_pair {
    const float* A; int32_t lda, M;
    const float* B; int32_t ldb, N;
    float* C; int32_t ldc;
    float* colsum;
} dygnn_dw_pair;

int dygnn_dw_grouped(int32_t K, const dygnn_dw_pair* pairs, int32_t npairs, dygnn_stream_t stream);

/* Test-only: the cosine forms of the time encoder (csrc/time_encoding.h) on n device floats, one thread per element: out[i] = f(x[i]).
 * form: 0 cos_fast, 1 cos_fast2 on the consecutive pairs (x[2j], x[2j + 1]) (an odd n's last element is paired with 0), 2 cos_time,
 * 3 cos_time_select, 4 sin_fast, 5 sin_time.  Forms 0, 1 and 4 are unguarded: their result is unspecified for |x| > 3e7.
 * Another form, negative n or n > 2^31, a NULL array with n > 0: DYGNN_E_INVALID.  No backbone calls it. */
int dygnn_timeenc_probe(int32_t form, const float* x, int64_t n, float* out, dygnn_stream_t stream);

/* Test-only: the GELU of the fused DyGFormer forward on n device floats: out[i] = gelu(in[i]).  form 0: the table form of the inference
 * kernels — the probe stages the table (csrc/gelu_table.h) into LDS by the kernels' routine, at the kernels' offset, and runs their device
 * function; form 1: the erf form (Abramowitz & Stegun 7.1.26) of the training kernels.  The call returns after the work is done.
 * Another form, negative n or n > 2^31, a NULL array with n > 0: DYGNN_E_INVALID.  No backbone calls it.
 * gelu_table_host: the table as the packed buffer holds it, out[4096][2] = (Phi(x_i), Phi(x_{i+1}) - Phi(x_i)), x_i = -6 + 12 i / 4096 (host). */
int dygnn_gelu_probe(const float* in, float* out, int64_t n, int32_t form, dygnn_stream_t stream);
int dygnn_gelu_table_host(float* out);

#ifdef __cplusplus
}
#endif
#endif /* DYGNN_H */
