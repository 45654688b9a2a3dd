// Fused DyGFormer forward, inference: the host dispatch of k_dygformer_fused3 and its nine inference instances (kernel and design:
// fused3_forward.h, fused3_device.h; training instances: dygformer_fused3_train.hip; backward: dygformer_fused3_bwd.hip; weight
// packing: dygformer_fused3_pack.hip).
#include "fused3_forward.h"

namespace dygnn {

namespace v3 {
// the packed form (fused3_body, PK): untapped launches of pairs of <= 64 tokens that defer their tail.  A kernel name of its own: the
// template list of k_dygformer_fused3 is what the resource tests match.
__global__ __launch_bounds__(512, 2) void k_dygformer_fused3_packed(const Args a) {
    fused3_body<4, false, 8, 3, true>(a);
}
}  // namespace v3

// table_flags (dygnn_dygformer_forward_tables): the stored fragment sequence is [node | time | edge | cooc], every channel in whole
// groups of four slots (build_proj).  A channel whose table is all zero leaves the walk: its chunk count becomes 0 and the prologue's
// DMA steps over its stored fragments.
static void drop_zero_channels(v3::Args& a, uint32_t table_flags) {
    using namespace v3;
    const int node_frags = 4 * proj_slots(a.nchunk[0]), time_frags = 4 * proj_slots(a.nchunk[2]), edge_frags = 4 * proj_slots(a.nchunk[1]);
    if (table_flags & DYGNN_TABLE_NODE_ZERO) { a.proj_skip0 = node_frags; a.proj_frags -= node_frags; a.nchunk[0] = 0; }
    a.proj_cut = (a.nchunk[0] ? node_frags : 0) + time_frags;
    if (table_flags & DYGNN_TABLE_EDGE_ZERO) { a.proj_skip1 = edge_frags; a.proj_frags -= edge_frags; a.nchunk[1] = 0; }
}

int forward_fused3(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, const float* packed,
                   const dygnn_csr* csr, const float* node_feat, const float* edge_feat, const int64_t* src,
                   const int64_t* dst, const double* times, int64_t B, int64_t G, int64_t pair_stride, float* out_src, float* out_dst, char* ws,
                   const WorkspaceLayout& wl, const dygnn_dygformer_taps* taps, uint32_t table_flags, const float* node_proj, const float* edge_proj,
                   hipStream_t s) {
    using namespace v3;
    if (!supported(d)) { set_error("fused kernel: unsupported shape"); return DYGNN_E_UNSUPPORTED; }
    if (int rc = window_lengths_device(d, csr, src, dst, times, B, G, ws, wl, s)) return rc;
    Args a{};
    PackLayout3 f;
    if (int rc = fused3_args(d, pl, w, packed, csr, node_feat, edge_feat, src, dst, times, B, G, out_src, out_dst, ws, wl, taps, a, f)) return rc;
    // A projected table (dygformer_proj_tables.hip) takes its channel out of the walk exactly as a zero table does; the kernel adds the
    // projected rows instead.  A table flagged all zero needs neither.
    if (table_flags & DYGNN_TABLE_NODE_ZERO) node_proj = nullptr;
    if (table_flags & DYGNN_TABLE_EDGE_ZERO) edge_proj = nullptr;
    drop_zero_channels(a, table_flags | (node_proj ? DYGNN_TABLE_NODE_ZERO : 0u) | (edge_proj ? DYGNN_TABLE_EDGE_ZERO : 0u));
    a.pt_node = node_proj; a.pt_edge = edge_proj;
    // DYGNN_TABLE_CONST_QKV: the rows of the encoder input that stay at the projection bias are a PREFIX of the model dimension only while the
    // node table is flagged zero (rows 0 .. 49), and the edge table too for the longer one (rows 0 .. 99); a projected table is not constant
    if (table_flags & DYGNN_TABLE_CONST_QKV) {
        a.qkv0_skip = !(table_flags & DYGNN_TABLE_NODE_ZERO) ? 0 : (table_flags & DYGNN_TABLE_EDGE_ZERO) ? 6 : 3;
        a.qkv0c = packed + pl.fused3 + f.qkv0c + (a.qkv0_skip == 6 ? kQkvTiles * 64 : 0);
    }
    if (taps && taps->seq_lens) DYGNN_HIP(hipMemcpyAsync(taps->seq_lens, ws + wl.dims + 2 * sizeof(int32_t), 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (taps && taps->ev_kernel_start) DYGNN_HIP(hipEventRecord(static_cast<hipEvent_t>(taps->ev_kernel_start), s));
    a.pair_stride = (f.np == 2 && pair_stride > 0) ? pair_stride : 0;      // one pair per workgroup (128 tokens): nothing to share inside a workgroup
    // Inference runs the pooled last layer.  A call that taps the last layer's per-token output gets it from the full stream (PL = 2); its
    // embeddings are the pooled ones bit for bit.  Every other call streams the pooled form: PL = 1, or from kPooledTailMinWorkgroups
    // workgroups on PL = 3 followed by k_pooled_tail, which gives the same bits (dygformer_pooled_tail.hip).
    const bool tap_last = taps && taps->layer_out[d.NL - 1] != nullptr;
    if (!tap_last) { a.stream = packed + pl.fused3 + f.stream_p; a.nstages = f.nstages_p; }
    // The packed form (fused3_plan.h): untapped launches of pairs of <= 64 tokens.  By default wherever the tail is deferred; DYGNN_PACK_PAIRS = 1
    // puts every such launch on it, a small one included (and defers its tail), 0 none.
    bool untapped = !tap_last && !(taps && (taps->encoder_input || taps->phase_cycles));
    for (int l = 0; l < d.NL; ++l) untapped = untapped && !(taps && taps->layer_out[l]);
    const int pk_env = pack_pairs_env();
    const size_t plan_off = plan_offset(B, G);       // 0: the workspace has no room for this call's plan (dygformer_layout.h)
    const bool pack_ok = untapped && f.np == 2 && f.scr_floats8 > 0 && B <= INT32_MAX && plan_off > 0 && pk_env != 0;
    const bool small = f.np == 2 && a.pair_stride == 0 && B <= kSmallBatchPairs && !small_off() && !(pack_ok && pk_env == 1);      // a small call: one pair per four-wave workgroup
    const unsigned grid = small || f.np != 2 ? (unsigned)B : (unsigned)(a.pair_stride ? a.pair_stride : (B + 1) / 2);
    auto launch = [&](auto kern, unsigned threads) -> int {
        // per device and cheap: set on every call (a process may drive several GPUs, or call from several threads)
        DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), kLdsBytes, s, a);
        return DYGNN_OK;
    };
    // (the size rule looks at the UNPACKED workgroup count: a launch keeps its form whatever the plan makes of it)
    const bool tail = !tap_last && (pooled_tail_wanted(grid) || (pack_ok && pk_env == 1));
    const bool pack_it = pack_ok && !small && tail;
    int rc;
    if (pack_it) {
        // the plan is part of the launch: inside the timed pair of events, on the same stream, no host synchronisation.  The grid stays the
        // unpacked one (the plan never needs more); workgroups beyond the plan's count return at once.
        if (int rcp = pack_plan_device(d, B, G, ws, wl, s)) return rcp;
        a.plan = reinterpret_cast<const int32_t*>(ws + wl.dims + plan_off);
        a.pair_stride = 0; a.scr_floats = f.scr_floats8; a.slab_chunks = f.slab_chunks8; a.tab_off = 0; a.tab_slots = 0; a.tab_bits = 0;
        rc = launch(k_dygformer_fused3_packed, 512);
    } else if (tail) rc = small ? launch(k_dygformer_fused3<4, false, 4, 3>, 256) : f.np == 2 ? launch(k_dygformer_fused3<4, false, 8, 3>, 512) : launch(k_dygformer_fused3<8, false, 8, 3>, 512);
    else if (small) rc = tap_last ? launch(k_dygformer_fused3<4, false, 4, 2>, 256) : launch(k_dygformer_fused3<4, false, 4, 1>, 256);
    else if (f.np == 2) rc = tap_last ? launch(k_dygformer_fused3<4, false, 8, 2>, 512) : launch(k_dygformer_fused3<4, false, 8, 1>, 512);
    else rc = tap_last ? launch(k_dygformer_fused3<8, false, 8, 2>, 512) : launch(k_dygformer_fused3<8, false, 8, 1>, 512);
    if (rc) return rc;
    DYGNN_LAUNCH_CHECK();
    if (tail)
        if (int rc2 = pooled_tail(a.pooled_rows, 2 * B, a.w2frag, a.b2_last, a.outfrag, a.outb, a.Fn, out_src, out_dst, s)) return rc2;
    if (taps && taps->ev_kernel_stop) DYGNN_HIP(hipEventRecord(static_cast<hipEvent_t>(taps->ev_kernel_stop), s));
    return DYGNN_OK;
}

}  // namespace dygnn
