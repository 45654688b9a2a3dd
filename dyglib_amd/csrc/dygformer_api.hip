// C-ABI entry points for the DyGFormer forward path: sizes, pack / repack, forward (the link-predictor head's are in merge_layer.hip, the general GEMM's in gemm.hip).
#include "dygformer_layout.h"
#include "fused3_plan.h"

namespace dygnn {
// dygformer_generic.hip
int pack_generic(const Dims&, const PackedLayout&, const dygnn_dygformer_weights*, float* packed, hipStream_t);
int forward_generic(const Dims&, const PackedLayout&, const dygnn_dygformer_weights*, const float* packed, const dygnn_csr*,
                    const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times,
                    int64_t B, int64_t G, int64_t pair_stride, float* out_src, float* out_dst, char* ws, const WorkspaceLayout&,
                    const dygnn_dygformer_taps*, hipStream_t);

static int check_weights(const Dims& d, const dygnn_dygformer_weights* w) {
    DYGNN_REQUIRE(w != nullptr, "weights is NULL");
    const void* p[] = {w->time_w, w->time_b, w->cooc_w0, w->cooc_b0, w->cooc_w1, w->cooc_b1, w->proj_node_w, w->proj_node_b,
                       w->proj_edge_w, w->proj_edge_b, w->proj_time_w, w->proj_time_b, w->proj_cooc_w, w->proj_cooc_b,
                       w->output_w, w->output_b};
    for (const void* q : p) DYGNN_REQUIRE(q != nullptr, "weights: null parameter pointer");
    for (int l = 0; l < d.NL; ++l) {
        const dygnn_encoder_layer_weights& L = w->layers[l];
        const void* r[] = {L.in_proj_weight, L.in_proj_bias, L.out_proj_weight, L.out_proj_bias, L.ffn0_weight, L.ffn0_bias,
                           L.ffn1_weight, L.ffn1_bias, L.norm0_weight, L.norm0_bias, L.norm1_weight, L.norm1_bias};
        for (const void* q : r) DYGNN_REQUIRE(q != nullptr, "weights: null parameter pointer in layer %d", l);
    }
    return DYGNN_OK;
}


}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_dygformer_packed_bytes(const dygnn_dygformer_config* cfg) {
    if (check_config(cfg) != DYGNN_OK) return 0;
    const Dims d = make_dims(*cfg);
    return make_packed_layout(d).total * sizeof(float);
}

extern "C" size_t dygnn_dygformer_workspace_bytes(const dygnn_dygformer_config* cfg, int64_t batch) {
    if (check_config(cfg) != DYGNN_OK || batch < 0) return 0;
    const Dims d = make_dims(*cfg);
    return make_workspace_layout(d, batch).total;
}

// impl as in dygnn_dygformer_forward.  The fused kernels keep every activation on chip: they only need the per-query search results
// (a few bytes per pair); the generic path also needs its HBM activation buffers (~29 KB per token).
extern "C" size_t dygnn_dygformer_workspace_bytes_for(const dygnn_dygformer_config* cfg, int64_t batch, int32_t impl) {
    if (check_config(cfg) != DYGNN_OK || batch < 0 || !(impl == 0 || impl == 1 || impl == 3)) return 0;
    const Dims d = make_dims(*cfg);
    const WorkspaceLayout wl = make_workspace_layout(d, batch);
    const bool generic = impl == 1 || !fused3_supported(d);
    return generic ? wl.total : wl.X;
}

static int pack_impl(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, void* packed, size_t packed_bytes, dygnn_stream_t stream, bool reuse_desc,
                     bool fused_only = false) {
    if (int rc = check_config(cfg)) return rc;
    const Dims d = make_dims(*cfg);
    if (int rc = check_weights(d, w)) return rc;
    const PackedLayout pl = make_packed_layout(d);
    DYGNN_REQUIRE(packed != nullptr, "pack: packed buffer is NULL");
    if (packed_bytes < pl.total * sizeof(float)) {
        set_error("pack: buffer too small (%zu < %zu bytes)", packed_bytes, pl.total * sizeof(float));
        return DYGNN_E_WORKSPACE;
    }
    if (!(fused_only && fused3_supported(d)))
        if (int rc = pack_generic(d, pl, w, static_cast<float*>(packed), as_stream(stream))) return rc;
    if (fused3_supported(d))
        if (int rc = pack_fused3(d, pl, w, static_cast<float*>(packed), as_stream(stream), reuse_desc, fused_only)) return rc;
    return DYGNN_OK;
}

extern "C" int dygnn_dygformer_pack(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, void* packed,
                                    size_t packed_bytes, dygnn_stream_t stream) {
    return pack_impl(cfg, w, packed, packed_bytes, stream, false);
}

extern "C" int dygnn_dygformer_repack(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, void* packed,
                                      size_t packed_bytes, int32_t fused_only, dygnn_stream_t stream) {
    return pack_impl(cfg, w, packed, packed_bytes, stream, true, fused_only != 0);
}

static int forward_impl(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, const void* packed, const dygnn_csr* csr,
                        const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                        int64_t group_size, int64_t pair_stride, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes,
                        const dygnn_dygformer_taps* taps, int32_t impl, dygnn_stream_t stream, uint32_t table_flags, const float* node_proj,
                        const float* edge_proj) {
    if (int rc = check_config(cfg)) return rc;
    const Dims d = make_dims(*cfg);
    if (int rc = check_weights(d, w)) return rc;
    DYGNN_REQUIRE(csr && csr->indptr && csr->num_nodes >= 1, "forward: bad csr");
    DYGNN_REQUIRE(batch >= 0, "forward: negative batch");
    DYGNN_REQUIRE(group_size >= 0, "forward: negative group_size");
    if (group_size == 0 || group_size > batch) group_size = batch;      // one group = the reference's single call
    DYGNN_REQUIRE(pair_stride == 0 || (2 * pair_stride == batch && pair_stride % group_size == 0),
                  "forward: pair_stride must be 0 or batch / 2, a whole number of groups (pairs i and i + pair_stride = the positive and negative call of one edge)");
    DYGNN_REQUIRE(packed && node_feat && edge_feat, "forward: null table / packed pointer");
    DYGNN_REQUIRE(batch == 0 || (src && dst && times && out_src && out_dst && workspace), "forward: null pointer");
    DYGNN_REQUIRE(impl == 0 || impl == 1 || impl == 3, "forward: impl must be 0 (auto), 1 (generic) or 3 (fused, token-owner layout)");
    if (batch == 0) return DYGNN_OK;
    const WorkspaceLayout wl = make_workspace_layout(d, batch);
    const size_t need = dygnn_dygformer_workspace_bytes_for(cfg, batch, impl);
    if (workspace_bytes < need) {
        set_error("forward: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
        return DYGNN_E_WORKSPACE;
    }
    const PackedLayout pl = make_packed_layout(d);
    const bool can_fuse3 = fused3_supported(d);
    if (impl == 3 && !can_fuse3) {
        set_error("forward: token-owner fused kernel does not support this shape (D=%d H=%d tokens<=%d)", d.D, d.H, d.Tmax);
        return DYGNN_E_UNSUPPORTED;
    }
    if (impl == 3 || (impl == 0 && can_fuse3))
        return forward_fused3(d, pl, w, static_cast<const float*>(packed), csr, node_feat, edge_feat, src, dst, times, batch, group_size, pair_stride, out_src,
                              out_dst, static_cast<char*>(workspace), wl, taps, table_flags, node_proj, edge_proj, as_stream(stream));
    // the generic path multiplies the tables as they are: the flags promise nothing it uses
    return forward_generic(d, pl, w, static_cast<const float*>(packed), csr, node_feat, edge_feat, src, dst, times, batch, group_size, pair_stride, out_src,
                           out_dst, static_cast<char*>(workspace), wl, taps, as_stream(stream));
}

extern "C" int dygnn_dygformer_forward_tables(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, const void* packed,
                                              const dygnn_csr* csr, const float* node_feat, const float* edge_feat, const int64_t* src,
                                              const int64_t* dst, const double* times, int64_t batch, int64_t group_size, int64_t pair_stride,
                                              float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, const dygnn_dygformer_taps* taps,
                                              int32_t impl, dygnn_stream_t stream, uint32_t table_flags) {
    if (int rc = check_config(cfg)) return rc;
    DYGNN_REQUIRE((table_flags & ~(uint32_t)(DYGNN_TABLE_NODE_ZERO | DYGNN_TABLE_EDGE_ZERO)) == 0, "forward: unknown table_flags bit");
    return forward_impl(cfg, w, packed, csr, node_feat, edge_feat, src, dst, times, batch, group_size, pair_stride, out_src, out_dst, workspace,
                        workspace_bytes, taps, impl, stream, table_flags, nullptr, nullptr);
}

// The projected tables are the caller's (dygnn_dygformer_project_table): a channel whose bit is set takes the row-addition path of the
// fused inference kernels.  DYGNN_PROJ_TABLES=0 ignores them (the MFMA path), as the generic path does.
extern "C" int dygnn_dygformer_forward_projected(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, const void* packed,
                                                 const dygnn_csr* csr, const float* node_feat, const float* edge_feat, const int64_t* src,
                                                 const int64_t* dst, const double* times, int64_t batch, int64_t group_size, int64_t pair_stride,
                                                 float* out_src, float* out_dst, void* workspace, size_t workspace_bytes,
                                                 const dygnn_dygformer_taps* taps, int32_t impl, dygnn_stream_t stream, uint32_t table_flags,
                                                 const float* node_proj, const float* edge_proj) {
    if (int rc = check_config(cfg)) return rc;
    DYGNN_REQUIRE((table_flags & ~(uint32_t)(DYGNN_TABLE_NODE_ZERO | DYGNN_TABLE_EDGE_ZERO | DYGNN_TABLE_NODE_PROJ | DYGNN_TABLE_EDGE_PROJ | DYGNN_TABLE_CONST_QKV)) == 0,
                  "forward: unknown table_flags bit");
    DYGNN_REQUIRE(!(table_flags & DYGNN_TABLE_NODE_PROJ) || node_proj != nullptr, "forward: table_flags names a projected node table, node_proj is NULL");
    DYGNN_REQUIRE(!(table_flags & DYGNN_TABLE_EDGE_PROJ) || edge_proj != nullptr, "forward: table_flags names a projected edge table, edge_proj is NULL");
    DYGNN_REQUIRE(((reinterpret_cast<uintptr_t>(node_proj) | reinterpret_cast<uintptr_t>(edge_proj)) & 15) == 0, "forward: projected tables must be 16-byte aligned");
    const bool off = proj_tables_off();
    // DYGNN_CONST_QKV = 0 / 1 overrides the caller's bit (DYGNN_PROJ_TABLES has no say in it)
    const int cq = const_qkv_env();
    const uint32_t const_qkv = cq < 0 ? (table_flags & DYGNN_TABLE_CONST_QKV) : cq ? DYGNN_TABLE_CONST_QKV : 0u;
    return forward_impl(cfg, w, packed, csr, node_feat, edge_feat, src, dst, times, batch, group_size, pair_stride, out_src, out_dst, workspace,
                        workspace_bytes, taps, impl, stream, (table_flags & (uint32_t)(DYGNN_TABLE_NODE_ZERO | DYGNN_TABLE_EDGE_ZERO)) | const_qkv,
                        !off && (table_flags & DYGNN_TABLE_NODE_PROJ) ? node_proj : nullptr, !off && (table_flags & DYGNN_TABLE_EDGE_PROJ) ? edge_proj : nullptr);
}

extern "C" int dygnn_dygformer_forward(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, const void* packed,
                                       const dygnn_csr* csr, const float* node_feat, const float* edge_feat, const int64_t* src,
                                       const int64_t* dst, const double* times, int64_t batch, int64_t group_size, int64_t pair_stride,
                                       float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, const dygnn_dygformer_taps* taps,
                                       int32_t impl, dygnn_stream_t stream) {
    return dygnn_dygformer_forward_tables(cfg, w, packed, csr, node_feat, edge_feat, src, dst, times, batch, group_size, pair_stride, out_src, out_dst,
                                          workspace, workspace_bytes, taps, impl, stream, 0);
}

// host mirrors of the constant-channel arithmetic (fused3_plan.h; tests, no GPU)
extern "C" int32_t dygnn_dygformer_qkv_tile_row_host(int32_t tile, int32_t c) {
    if (tile < 0 || tile >= v3::kQkvTiles || c < 0 || c >= 16) return -2;
    return v3::qkv_tile_row(tile, c);
}
extern "C" int dygnn_dygformer_qkv0_const_host(const float* in_proj_weight, const float* gamma, const float* beta, const float* bias, int32_t k0, float* out) {
    DYGNN_REQUIRE(in_proj_weight && gamma && beta && bias && out, "qkv0_const: null pointer");
    DYGNN_REQUIRE(k0 == 48 || k0 == 96, "qkv0_const: k0 must be 48 or 96");
    for (int i = 0; i < v3::kQkvTiles * 64; ++i) out[i] = v3::qkv0_const(in_proj_weight, gamma, beta, bias, k0, i / 64, i % 64);
    return DYGNN_OK;
}
