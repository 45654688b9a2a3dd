// The launch sequence of one TransformerEncoder block (models/modules.py:209-266) on the training paths, forward and backward, shared by
// tcl_train.hip (2 L blocks per call) and cawn_train.hip (one).  The attention kernels are the caller's (key mask and cross-attention in
// TCL, M walks without a mask in CAWN): two callables launch them.  Dense products go through train::mm, the block's four weight
// gradients through ONE train::dw_grouped launch, LayerNorm and bias gradients through fixed-order column sums (train::colsum).
//
// Dropout sites of a block, counted from its site base: 0 attention probabilities (the caller's kernels), 1 attention block output,
// 2 relu(fc0), 3 fc1 output; element (map.row(r) d + c), site 2 (map.row(r) 4d + c).
#pragma once
#include "colsum.h"
#include "common.h"
#include "dropout.h"
#include "gemm.h"
#include "train_rows.h"

namespace dygnn {
namespace train {

// R token rows of width d.  Saved by the forward, read by the backward: q | k | v [R][3d] with bias (q unscaled), the attention output O
// [R][d], the two pre-LayerNorm sums with mean and rstd, LayerNorm 0's output, the post-ReLU post-dropout hidden rows [R][4d], the block
// output.  (The softmax is the attention kernels' own.)
struct BlockBufs {
    float *qkv, *O, *pre0, *mean0, *rstd0, *y0, *hid, *pre1, *mean1, *rstd1, *out;
    float* tmp;                                                  // forward scratch [R][d]
    float *gA, *gB, *gC, *gD, *gE, *gF, *dhid, *dqkv, *part;     // backward scratch: six [R][d], [R][4d], [R][3d], the column sums' partials
};

// X [R][d] -> v.out.  attn(): v.qkv -> v.O (site `site`).  NV: columns per lane of the row kernels, d <= 64 NV.
template <int NV, class Attn>
static int encoder_block_forward(hipStream_t s, int d, int64_t R, const float* X, const dygnn_tcl_layer_weights& m, const Drop& dr, float dropout_p,
                                 uint32_t site, const RowMap& map, const BlockBufs& v, Attn attn) {
    const unsigned row_blocks = (unsigned)ceil_div(R, 4);
    const int Ri = (int)R;
    if (int rc = mm(s, X, d, false, m.in_proj_w, d, true, v.qkv, 3 * d, Ri, 3 * d, d, MmOpt().bias(m.in_proj_b))) return rc;
    if (int rc = attn()) return rc;
    if (int rc = mm(s, v.O, d, false, m.out_proj_w, d, true, v.tmp, d, Ri, d, d, MmOpt().bias(m.out_proj_b))) return rc;
    hipLaunchKernelGGL(k_res_ln<NV>, dim3(row_blocks), dim3(256), 0, s, v.tmp, X, m.norm0_w, m.norm0_b, R, d, map, dr, site + 1, v.pre0, v.mean0, v.rstd0,
                       v.y0);
    DYGNN_LAUNCH_CHECK();
    if (int rc = mm(s, v.y0, d, false, m.fc0_w, d, true, v.hid, 4 * d, Ri, 4 * d, d, MmOpt().bias(m.fc0_b).relu())) return rc;
    if (dropout_p > 0.f) {
        hipLaunchKernelGGL(k_row_drop, dim3((unsigned)ceil_div(R * 4 * d, 256)), dim3(256), 0, s, v.hid, R * 4 * d, 4 * d, map, dr, site + 2);
        DYGNN_LAUNCH_CHECK();
    }
    if (int rc = mm(s, v.hid, 4 * d, false, m.fc1_w, 4 * d, true, v.tmp, d, Ri, d, 4 * d, MmOpt().bias(m.fc1_b))) return rc;
    hipLaunchKernelGGL(k_res_ln<NV>, dim3(row_blocks), dim3(256), 0, s, v.tmp, v.y0, m.norm1_w, m.norm1_b, R, d, map, dr, site + 3, v.pre1, v.mean1, v.rstd1,
                       v.out);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

// v.gA = d (block output) on entry, d X on exit; the gradients of the block's 12 tensors are ADDED to g's.  attn_bwd(): v.gF = d O -> v.dqkv.
template <int NV, class AttnBwd>
static int encoder_block_backward(hipStream_t s, int d, int64_t R, const float* X, const dygnn_tcl_layer_weights& m, const dygnn_tcl_layer_weights& g,
                                  const Drop& dr, uint32_t site, const RowMap& map, const BlockBufs& v, AttnBwd attn_bwd) {
    const unsigned row_blocks = (unsigned)ceil_div(R, 4);
    const int Ri = (int)R;
    auto W = [](const float* p) { return const_cast<float*>(p); };      // a gradient struct is the weight struct: const pointers to writable buffers
    auto cs = [&](const float* A, int cols, const float* out) { return colsum(s, A, cols, R, cols, v.part, out); };
    // LayerNorm 1, fc1 dropout: gA = d out -> gB = d y0 (residual part), gC = d (fc1 output)
    hipLaunchKernelGGL(k_res_ln_bwd<NV>, dim3(row_blocks), dim3(256), 0, s, v.gA, v.pre1, v.mean1, v.rstd1, m.norm1_w, R, d, map, dr, site + 3, v.gB, v.gC,
                       v.gD);
    DYGNN_LAUNCH_CHECK();
    if (int rc = cs(v.gD, d, g.norm1_w)) return rc;
    if (int rc = cs(v.gA, d, g.norm1_b)) return rc;
    if (int rc = cs(v.gC, d, g.fc1_b)) return rc;
    // fc1^T, ReLU and site-2 mask, fc0^T
    if (int rc = mm(s, v.gC, d, false, m.fc1_w, 4 * d, false, v.dhid, 4 * d, Ri, 4 * d, d)) return rc;
    hipLaunchKernelGGL(k_hid_bwd, dim3((unsigned)ceil_div(R * 4 * d, 256)), dim3(256), 0, s, v.dhid, v.hid, R * 4 * d, dr.scale);
    DYGNN_LAUNCH_CHECK();
    if (int rc = cs(v.dhid, 4 * d, g.fc0_b)) return rc;
    if (int rc = mm(s, v.dhid, 4 * d, false, m.fc0_w, d, false, v.gB, d, Ri, d, 4 * d, MmOpt().beta(1.f))) return rc;
    // LayerNorm 0, attention block dropout: gB = d y0 -> gA = d X (residual part), gE = d (out_proj output)
    hipLaunchKernelGGL(k_res_ln_bwd<NV>, dim3(row_blocks), dim3(256), 0, s, v.gB, v.pre0, v.mean0, v.rstd0, m.norm0_w, R, d, map, dr, site + 1, v.gA, v.gE,
                       v.gD);
    DYGNN_LAUNCH_CHECK();
    if (int rc = cs(v.gD, d, g.norm0_w)) return rc;
    if (int rc = cs(v.gB, d, g.norm0_b)) return rc;
    if (int rc = cs(v.gE, d, g.out_proj_b)) return rc;
    // out_proj^T, attention, in_proj^T
    if (int rc = mm(s, v.gE, d, false, m.out_proj_w, d, false, v.gF, d, Ri, d, d)) return rc;
    if (int rc = attn_bwd()) return rc;
    if (int rc = cs(v.dqkv, 3 * d, g.in_proj_b)) return rc;
    if (int rc = mm(s, v.dqkv, 3 * d, false, m.in_proj_w, d, false, v.gA, d, Ri, d, 3 * d, MmOpt().beta(1.f))) return rc;
    // the block's weight gradients, grouped split-K over its R rows
    const DwPair pairs[4] = {{v.dqkv, 3 * d, 3 * d, X, d, d, W(g.in_proj_w), d, nullptr},
                             {v.gE, d, d, v.O, d, d, W(g.out_proj_w), d, nullptr},
                             {v.dhid, 4 * d, 4 * d, v.y0, d, d, W(g.fc0_w), d, nullptr},
                             {v.gC, d, d, v.hid, 4 * d, 4 * d, W(g.fc1_w), 4 * d, nullptr}};
    return dw_grouped(s, Ri, pairs, 4);
}

}  // namespace train
}  // namespace dygnn
