// Fused DyGFormer forward, training: the host dispatch of the three k_dygformer_fused3<.., TR = true> instances (kernel: fused3_forward.h).
#include <cstdlib>

#include "fused3_forward.h"

namespace dygnn {

// Training forward through the fused kernel (dygformer_train.hip calls this when the shape is supported): one group of B pairs whose
// window lengths (hist_len / end_pos / dims at the head of `ws`, layout `wl`) the caller has already computed; `lut` = the co-occurrence
// table of the CURRENT weights; `packed` holds the fragment stream of the current weights (dygnn_dygformer_pack / _repack).
int forward_fused3_train(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, const float* packed, const dygnn_csr* csr,
                         const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times, int64_t B,
                         const float* lut, float* out_src, float* out_dst, char* ws, const WorkspaceLayout& wl, const train::TrainOut& tr, hipStream_t s) {
    using namespace v3;
    if (!supported(d)) { set_error("fused training forward: unsupported shape"); return DYGNN_E_UNSUPPORTED; }
    Args a{};
    PackLayout3 f;
    if (int rc = fused3_args(d, pl, w, packed, csr, node_feat, edge_feat, src, dst, times, B, B, out_src, out_dst, ws, wl, nullptr, a, f)) return rc;
    a.lut = lut;
    a.tr = tr;
    a.pair_stride = 0;
#ifdef DYGNN_STAMPS
    if (const char* sp = getenv("DYGNN_STAMPS_PTR")) a.stamps = reinterpret_cast<unsigned long long*>(strtoull(sp, nullptr, 0));   // diagnostic build: [4][8][32] device words
#endif
    DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_dygformer_fused3<4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_dygformer_fused3<8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    if (f.np == 2 && B <= kSmallBatchPairs && !small_off()) {
        DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_dygformer_fused3<4, true, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        hipLaunchKernelGGL((k_dygformer_fused3<4, true, 4>), dim3((unsigned)B), dim3(256), kLdsBytes, s, a);
    } else if (f.np == 2) hipLaunchKernelGGL((k_dygformer_fused3<4, true>), dim3((unsigned)((B + 1) / 2)), dim3(512), kLdsBytes, s, a);
    else hipLaunchKernelGGL((k_dygformer_fused3<8, true>), dim3((unsigned)B), dim3(512), kLdsBytes, s, a);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace dygnn
