// Projected feature tables of the fused DyGFormer inference forward.
//
// The patch projection of a gathered channel (node or edge features) is linear in the table rows it gathers:
//     x0[channel rows](token) = b + sum_{p < P} W[:, p F .. (p + 1) F) . table[row(token, p)]          (DyGFormer.py:148-157, :259-261)
// The table does not change between calls and neither do the weights of an evaluation pass, so W[:, slot p] . table[row] is computed
// here once per (row, slot) and weights version, and the kernel adds P gathered rows per token instead of running the product.
//
// Layout [rows][P][kProjRow = 64]: one (row, slot) segment is the four x tiles the channel touches — model rows 16 t0 .. 16 t0 + 63 with
// t0 = (50 ch) / 16 — zero outside the channel's 50 rows, so lane (c, g) of a token-owner wave reads its accumulator registers as the
// float4s at 16 v + 4 g, v = 0 .. 3.  Every element is one fmaf chain over f = 0 .. F - 1 starting from 0.  Row 0 (the padding row) is a
// row like any other.
#include "dygformer_layout.h"
#include "fused3_device.h"

namespace dygnn {

constexpr int kProjRowsPerBlock = 16;      // 4 waves x 4 rows: a lane's weight value serves four table rows

// thread (j, q): element j of the segments of rows r0 + 4 q .. + 3, slot blockIdx.y
__global__ __launch_bounds__(256) void k_project_table(const float* __restrict__ w, const float* __restrict__ table, int64_t rows, int F, int P, int ch,
                                                        float* __restrict__ out) {
    using namespace v3;
    const int j = threadIdx.x & 63, q = threadIdx.x >> 6, p = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * kProjRowsPerBlock + 4 * q;
    const int k = 16 * ((kC * ch) / 16) + j - kC * ch;            // the channel's output row behind element j
    const bool live = k >= 0 && k < kC;
    const float* wr = w + (size_t)(live ? k : 0) * P * F + (size_t)p * F;
    const float* tr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) tr[i] = table + (size_t)(r0 + i < rows ? r0 + i : 0) * F;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int f = 0; f < F; ++f) {
        const float wv = wr[f];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = fmaf(wv, tr[i][f], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (r0 + i < rows) out[((size_t)(r0 + i) * P + p) * kProjRow + j] = live ? acc[i] : 0.f;
}

}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_dygformer_projected_bytes(const dygnn_dygformer_config* cfg, int64_t rows) {
    if (check_config(cfg) != DYGNN_OK || rows <= 0) return 0;
    const Dims d = make_dims(*cfg);
    if (!fused3_supported(d)) return 0;
    return (size_t)rows * (size_t)d.P * kProjRow * sizeof(float);
}

extern "C" int dygnn_dygformer_project_table(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, int32_t channel, const float* table,
                                             int64_t rows, void* projected, size_t projected_bytes, dygnn_stream_t stream) {
    if (int rc = check_config(cfg)) return rc;
    DYGNN_REQUIRE(channel == 0 || channel == 1, "project_table: channel must be 0 (node features) or 1 (edge features)");
    DYGNN_REQUIRE(w != nullptr && w->proj_node_w != nullptr && w->proj_edge_w != nullptr, "project_table: null projection weights");
    DYGNN_REQUIRE(table != nullptr && projected != nullptr && rows > 0, "project_table: null table / output pointer or no rows");
    DYGNN_REQUIRE((reinterpret_cast<uintptr_t>(projected) & 15) == 0, "project_table: the output must be 16-byte aligned");
    const Dims d = make_dims(*cfg);
    const size_t need = dygnn_dygformer_projected_bytes(cfg, rows);
    if (need == 0) { set_error("project_table: the fused kernel does not support this shape"); return DYGNN_E_UNSUPPORTED; }
    if (projected_bytes < need) { set_error("project_table: buffer too small (%zu < %zu bytes)", projected_bytes, need); return DYGNN_E_WORKSPACE; }
    const dim3 grid((unsigned)((rows + kProjRowsPerBlock - 1) / kProjRowsPerBlock), (unsigned)d.P);
    hipLaunchKernelGGL(k_project_table, grid, dim3(256), 0, as_stream(stream), channel == 0 ? w->proj_node_w : w->proj_edge_w, table, rows,
                       channel == 0 ? d.Fn : d.Fe, d.P, (int)channel, static_cast<float*>(projected));
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
