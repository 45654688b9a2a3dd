// GraphMixer training (models/GraphMixer.py:70-150, MLPMixer :200-244, FeedForwardNet :163-191): the forward of graphmixer.hip in TRAIN mode
// and its hand-written backward pass, so that train_link_prediction.py's two calls, MergeLayer + BCE, loss.backward() and Adam run on the
// HIP path.
//
// Layout.  A call works on n roots (for a training call [src ; dst], n = 2 B), K tokens each, token rows r = q K + j (R = n K rows), C
// channels, Kh = token hidden width, H = channel hidden width.  A root's rows never depend on the other roots of the call.  The time
// encoder is frozen and the node encoder has no parameters, so nothing that walks a [n, time_gap] window has a backward pass: the node
// term is computed once (k_gm_node) and only enters output_layer's weight gradient.
//
// Saved (workspace, read by the backward pass): the gathered token rows [R][C + Ft] (the B operand of the projection's weight gradient;
// the padded slots' rules stay in k_gmt_rows), output_layer's input [n][C + Fn], and per block the block input X [R][C], the residual after
// the token half X1 [R][C], the channel LayerNorm output [R][C] with its mean and rstd [R], the channel hidden rows before GELU [R][H] and
// after GELU and dropout [R][H].  The token half's intermediates (K and Kh values per column) are recomputed by its backward kernel with
// the forward's instruction sequence, hence the forward's mean and rstd.  Both LayerNorms keep the mean-refinement pass of graphmixer.hip.
//
// Dropout.  Masks are never stored: forward and backward redraw them from train::Drop (dropout.h).  site = 4 layer + s, q = the root's
// index in the call; the elements are numbered as the reference's dense activations:
//   s = 0 token hidden after GELU   [n, C, Kh]: (q C + ch) Kh + i       s = 2 channel hidden after GELU [n, K, H]: (q K + j) H + h
//   s = 1 token FFN output          [n, C, K]:  (q C + ch) K + j        s = 3 channel FFN output        [n, K, C]: (q K + j) C + c
// p = 0 has thresh = 0: every mask is 1 and the forward is the eval forward.
//
// Kernels:  k_gm_node / k_gm_proj                as they are (graphmixer.h)
//           k_gmt_rows                           the gathered token rows
//           k_gmt_token_fwd / k_gmt_token_bwd    token half, one root per workgroup and one thread per channel; the backward reduces its
//                                                2 K Kh + Kh + 3 K parameter gradients over the C threads in LDS in a fixed order and writes
//                                                one partial row per root
//           k_gmt_ln_fwd / k_gmt_ln_bwd          channel LayerNorm, one wave per row
//           train::k_gelu_drop / k_gelu_drop_bwd GELU and the site-2 mask; the mask times the exact GELU derivative   (train_elements.h: the dense
//           train::k_drop_add / k_drop_bwd       site-3 mask and residual; the mask on the gradient                   activations are numbered by offset)
//           k_gmt_cat / k_gmt_bcast              token mean | node part; the mean's gradient / K to the K rows
//           train::k_colsum_fin (colsum.h)       stage 2 of the fixed-order column sums, shared with the other backbones; into up to six tensors
// Dense products (channel fc0, fc1, their transposes, output_layer) go through train::mm (fp32 MFMA, gemm.h), a block's two channel weight
// gradients through ONE train::dw_grouped launch (float atomics), every vector gradient and the token half's matrices through fixed-order
// two-stage column sums (colsum.h's first stage): those are the same bits run to run.
#include "colsum.h"
#include "common.h"
#include "gemm.h"
#include "graphmixer.h"
#include "mfma_tile.h"
#include "time_encoding.h"
#include "train_elements.h"

namespace dygnn {
namespace gmt {

using timeenc::cos_time;
using gm::Csr;
using gm::history;
using gm::kLnEps;
using gm::kMaxTokens;
using train::colsum;

constexpr int NV = 4;                 // columns per lane of a row: C <= 256

// ---- the gathered token rows (k_gm_proj's sampling and padded-slot rules): TOK [R][C + Ft] ----------------------------------------------------
__global__ __launch_bounds__(256) void k_gmt_rows(Csr g, const float* __restrict__ edge_feat, const int64_t* __restrict__ nodes,
                                                    const double* __restrict__ times, const float* __restrict__ tw, const float* __restrict__ tb, int K, int C,
                                                    int Ft, float* __restrict__ TOK) {
    __shared__ int32_t s_eid[kMaxTokens];
    __shared__ float s_dt[kMaxTokens];
    const int lane = threadIdx.x & 63;
    const int64_t q = blockIdx.x;
    const int W = C + Ft;
    const double t = times[q];
    int64_t lo, end;
    history(g, nodes[q], t, lane, lo, end);
    const int64_t len = end - lo;
    const int m = (int)(len < K ? len : K), pad = K - m;
    if (threadIdx.x < kMaxTokens) {
        const int j = threadIdx.x;
        int32_t e = 0;
        float dt = 0.f;
        if (j >= pad && j < K) {
            const int64_t p = end - m + (j - pad);
            e = g.eid[p];
            dt = (float)(t - (double)(float)g.ts[p]);                  // f64 - f32 -> f64 -> .float(), as k_gm_proj
        }
        s_eid[j] = e; s_dt[j] = dt;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < K * W; i += 256) {
        const int j = i / W, f = i - j * W;
        float v = 0.f;
        if (f < C) v = edge_feat[(size_t)s_eid[j] * C + f];            // a padded slot reads edge row 0
        else if (j >= pad) v = cos_time(fmaf(s_dt[j], tw[f - C], tb[f - C]));      // time features of a padded slot are zero
        TOK[((size_t)q * K + j) * W + f] = v;
    }
}

// ---- Mixer block, token half: k_gm_token with the site-0 / site-1 masks, out of place (the block input is saved) --------------------------------
// LDS: T [K][C] (x, then the normalised column), Hd [Kh][C].
__global__ __launch_bounds__(256) void k_gmt_token_fwd(const float* __restrict__ Xin, float* __restrict__ Xout, const float* __restrict__ ln_w,
                                                         const float* __restrict__ ln_b, const float* __restrict__ W0, const float* __restrict__ b0,
                                                         const float* __restrict__ W1, const float* __restrict__ b1, int K, int Kh, int C, train::Drop dr,
                                                         uint32_t site) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* T = smem;
    float* Hd = smem + K * C;
    const int64_t q = blockIdx.x;
    const float* x = Xin + (size_t)q * K * C;
    float* y = Xout + (size_t)q * K * C;
    for (int i = threadIdx.x; i < K * C; i += 256) T[i] = x[i];
    __syncthreads();
    for (int ch = threadIdx.x; ch < C; ch += 256) {
        float s = 0.f;
        for (int j = 0; j < K; ++j) s += T[j * C + ch];
        float mean = s / (float)K;
        s = 0.f;
        for (int j = 0; j < K; ++j) s += T[j * C + ch] - mean;          // refinement pass, as k_gm_token
        mean += s / (float)K;
        float v = 0.f;
        for (int j = 0; j < K; ++j) { const float d = T[j * C + ch] - mean; v = fmaf(d, d, v); }
        const float rstd = 1.0f / sqrtf(v / (float)K + kLnEps);
        const uint64_t col = (uint64_t)q * C + ch;
        for (int j = 0; j < K; ++j) {
            const float xv = T[j * C + ch];
            y[(size_t)j * C + ch] = xv;                                  // the residual; the FFN output is added below
            T[j * C + ch] = fmaf((xv - mean) * rstd, ln_w[j], ln_b[j]);
        }
        for (int i = 0; i < Kh; ++i) {
            float a = b0[i];
            for (int j = 0; j < K; ++j) a = fmaf(W0[i * K + j], T[j * C + ch], a);
            Hd[i * C + ch] = gelu_exact(a) * dr.mask(site, col * Kh + i);
        }
        for (int j = 0; j < K; ++j) {
            float a = b1[j];
            for (int i = 0; i < Kh; ++i) a = fmaf(W1[j * Kh + i], Hd[i * C + ch], a);
            y[(size_t)j * C + ch] += a * dr.mask(site + 1, col * K + j);
        }
    }
}

// Token half backward of root q = blockIdx.x, thread = channel.  In: the block input Xin, dX1 (gradient of the half's output).  Out: dX1 is
// overwritten IN PLACE with the gradient of the block input (the residual's gradient included); part[q][P] receives the root's parameter
// gradients, P = 2 K Kh + Kh + 3 K in the order fc0 weight [Kh][K], fc0 bias, fc1 weight [K][Kh], fc1 bias, LayerNorm weight, LayerNorm bias.
// LDS (row stride ld = C | 1: the reduction's threads walk different rows at the same channel): XH [K] xhat, Y [K] LayerNorm output,
// DO [K] masked output gradient, later the LayerNorm output's gradient, HD [Kh] hidden after GELU and mask, DA [Kh] pre-GELU gradient.
__global__ __launch_bounds__(256) void k_gmt_token_bwd(const float* __restrict__ Xin, float* __restrict__ dX, const float* __restrict__ ln_w,
                                                         const float* __restrict__ ln_b, const float* __restrict__ W0, const float* __restrict__ b0,
                                                         const float* __restrict__ W1, int K, int Kh, int C, train::Drop dr, uint32_t site,
                                                         float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ld = C | 1;
    float* XH = smem;
    float* Y = XH + K * ld;
    float* DO = Y + K * ld;
    float* HD = DO + K * ld;
    float* DA = HD + Kh * ld;
    const int64_t q = blockIdx.x;
    const int ch = threadIdx.x;
    const bool on = ch < C;
    const float* x = Xin + (size_t)q * K * C + ch;
    float* dx = dX + (size_t)q * K * C + ch;
    const uint64_t col = (uint64_t)q * C + ch;
    float rstd = 0.f;
    if (on) {
        // the forward's LayerNorm, instruction for instruction: the same mean and rstd
        float s = 0.f;
        for (int j = 0; j < K; ++j) { const float v = x[(size_t)j * C]; XH[j * ld + ch] = v; s += v; }
        float mean = s / (float)K;
        s = 0.f;
        for (int j = 0; j < K; ++j) s += XH[j * ld + ch] - mean;
        mean += s / (float)K;
        float v = 0.f;
        for (int j = 0; j < K; ++j) { const float d = XH[j * ld + ch] - mean; v = fmaf(d, d, v); }
        rstd = 1.0f / sqrtf(v / (float)K + kLnEps);
        for (int j = 0; j < K; ++j) {
            const float xh = (XH[j * ld + ch] - mean) * rstd;
            XH[j * ld + ch] = xh;
            Y[j * ld + ch] = fmaf(xh, ln_w[j], ln_b[j]);
            DO[j * ld + ch] = dx[(size_t)j * C] * dr.mask(site + 1, col * K + j);
        }
        for (int i = 0; i < Kh; ++i) {
            float a = b0[i];
            for (int j = 0; j < K; ++j) a = fmaf(W0[i * K + j], Y[j * ld + ch], a);
            const float m0 = dr.mask(site, col * Kh + i);
            HD[i * ld + ch] = gelu_exact(a) * m0;
            float dh = 0.f;
            for (int j = 0; j < K; ++j) dh = fmaf(W1[j * Kh + i], DO[j * ld + ch], dh);
            DA[i * ld + ch] = dh * m0 * gelu_exact_grad(a);
        }
    }
    __syncthreads();
    // parameter gradients of the two Linear layers: sums over the channels in ascending order
    float* out = part + (size_t)q * (2 * K * Kh + Kh + 3 * K);
    const int oB0 = Kh * K, oW1 = oB0 + Kh, oB1 = oW1 + K * Kh, oG = oB1 + K;
    for (int o = threadIdx.x; o < oG; o += 256) {
        float s = 0.f;
        if (o < oB0) {                                                   // fc0 weight [i][j] = sum DA[i] Y[j]
            const float *a = DA + (o / K) * ld, *b = Y + (o % K) * ld;
            for (int c = 0; c < C; ++c) s = fmaf(a[c], b[c], s);
        } else if (o < oW1) {
            const float* a = DA + (o - oB0) * ld;
            for (int c = 0; c < C; ++c) s += a[c];
        } else if (o < oB1) {                                            // fc1 weight [j][i] = sum DO[j] HD[i]
            const float *a = DO + ((o - oW1) / Kh) * ld, *b = HD + ((o - oW1) % Kh) * ld;
            for (int c = 0; c < C; ++c) s = fmaf(a[c], b[c], s);
        } else {
            const float* a = DO + (o - oB1) * ld;
            for (int c = 0; c < C; ++c) s += a[c];
        }
        out[o] = s;
    }
    __syncthreads();                                                     // DO has been read: it now takes the LayerNorm output's gradient
    if (on) {
        float sg = 0.f, sgx = 0.f;
        for (int j = 0; j < K; ++j) {
            float dy = 0.f;
            for (int i = 0; i < Kh; ++i) dy = fmaf(W0[i * K + j], DA[i * ld + ch], dy);
            DO[j * ld + ch] = dy;
            const float gj = dy * ln_w[j];
            sg += gj;
            sgx = fmaf(gj, XH[j * ld + ch], sgx);
        }
        // mean(g) with a refinement pass: on a column of identical tokens rstd = 316 multiplies whatever rounding error the mean carries
        float mg = sg / (float)K;
        float s = 0.f;
        for (int j = 0; j < K; ++j) s += DO[j * ld + ch] * ln_w[j] - mg;
        mg += s / (float)K;
        const float mgx = sgx / (float)K;
        for (int j = 0; j < K; ++j) {
            const float gj = DO[j * ld + ch] * ln_w[j];
            dx[(size_t)j * C] += rstd * ((gj - mg) - XH[j * ld + ch] * mgx);
        }
    }
    __syncthreads();
    for (int o = threadIdx.x; o < 2 * K; o += 256) {                    // LayerNorm weight [j] = sum dy xhat, bias [j] = sum dy
        const int j = o < K ? o : o - K;
        const float *a = DO + j * ld, *b = XH + j * ld;
        float s = 0.f;
        if (o < K) for (int c = 0; c < C; ++c) s = fmaf(a[c], b[c], s);
        else for (int c = 0; c < C; ++c) s += a[c];
        out[oG + o] = s;
    }
}

// ---- channel LayerNorm, one wave per row (k_gm_ffn's, with the refinement pass): Y = LN(X1), mean and rstd saved ------------------------------
__global__ __launch_bounds__(256) void k_gmt_ln_fwd(const float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta, int64_t R,
                                                      int C, float* __restrict__ Y, float* __restrict__ mean_o, float* __restrict__ rstd_o) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    float x[NV];
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        x[u] = f < C ? X[r * C + f] : 0.f;
        if (f < C) s += x[u];
    }
    float mean = wave_sum(s) / (float)C;
    s = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + 64 * u < C) s += x[u] - mean;
    mean += wave_sum(s) / (float)C;
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + 64 * u < C) { const float d = x[u] - mean; v = fmaf(d, d, v); }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)C + kLnEps);
    if (lane == 0) { mean_o[r] = mean; rstd_o[r] = rstd; }
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        if (f < C) Y[r * C + f] = fmaf((x[u] - mean) * rstd, gamma[f], beta[f]);
    }
}

// LayerNorm backward, one wave per row, with the forward's mean and rstd: g = dy gamma, dx = dres + rstd (g - mean(g) - xhat mean(g xhat));
// dyx = dy xhat feeds the gamma gradient.  mean(g) takes a refinement pass like the forward's mean.
__global__ __launch_bounds__(256) void k_gmt_ln_bwd(const float* __restrict__ dy, const float* __restrict__ X, const float* __restrict__ mean_in,
                                                      const float* __restrict__ rstd_in, const float* __restrict__ gamma, const float* __restrict__ dres,
                                                      int64_t R, int C, float* __restrict__ dx, float* __restrict__ dyx) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float mean = mean_in[r], rstd = rstd_in[r];
    float xh[NV], g[NV];
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        xh[u] = g[u] = 0.f;
        if (f < C) {
            xh[u] = (X[r * C + f] - mean) * rstd;
            const float v = dy[r * C + f];
            g[u] = v * gamma[f];
            dyx[r * C + f] = v * xh[u];
            sg += g[u];
            sgx = fmaf(g[u], xh[u], sgx);
        }
    }
    float mg = wave_sum(sg) / (float)C;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + 64 * u < C) s += g[u] - mg;
    mg += wave_sum(s) / (float)C;
    const float mgx = wave_sum(sgx) / (float)C;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        if (f < C) dx[r * C + f] = dres[r * C + f] + rstd * ((g[u] - mg) - xh[u] * mgx);
    }
}

// Z [n][C + Fn] = [mean over the K tokens | node term + node_feat[v]] (k_gm_out's operand rows, the same sums)
__global__ void k_gmt_cat(const float* __restrict__ X, const float* __restrict__ term, const float* __restrict__ node_feat, const int64_t* __restrict__ nodes,
                          int64_t n, int64_t node_rows, int K, int C, int Fn, float* __restrict__ Z) {
    const int W = C + Fn;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * W) return;
    const int64_t q = e / W;
    const int f = (int)(e - q * W);
    float v;
    if (f < C) {
        const float* x = X + (size_t)q * K * C + f;
        float s = 0.f;
        for (int j = 0; j < K; ++j) s += x[(size_t)j * C];
        v = s / (float)K;
    } else {
        int64_t node = nodes[q];
        if (node < 0 || node >= node_rows) node = 0;
        v = term[(size_t)q * Fn + (f - C)] + node_feat[(size_t)node * Fn + (f - C)];
    }
    Z[e] = v;
}
// the token mean's gradient to its K rows: g [R][C] = dmean [n][C] / K
__global__ void k_gmt_bcast(const float* __restrict__ dmean, float* __restrict__ g, int64_t count, int K, int C) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= count) return;
    const int64_t r = e / C;
    g[e] = dmean[(r / K) * C + (e - r * C)] / (float)K;
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------------
struct Layer { size_t x1, y, mean, rstd, hpre, hact; };
struct Plan {
    int K, Kh, C, Ft, Fn, H, L, P;
    int64_t n, R;
    size_t term, tok, z;
    size_t x[DYGNN_MAX_LAYERS + 1];                        // x[l] = input of block l; x[L] = the last block's output
    Layer layer[DYGNN_MAX_LAYERS];
    size_t tmp;                                            // forward scratch [R][C]
    size_t dmean, gA, gB, gC, gD, gE, dhid, tpart, part;   // backward scratch
    size_t total;
};

static Plan make_plan(const dygnn_graphmixer_config& c, int64_t n) {
    Plan p{};
    p.K = c.num_tokens; p.Kh = c.token_hidden_dim; p.C = c.edge_feat_dim; p.Ft = c.time_feat_dim; p.Fn = c.node_feat_dim; p.H = c.channel_hidden_dim;
    p.L = c.num_layers; p.P = 2 * p.K * p.Kh + p.Kh + 3 * p.K;
    p.n = n; p.R = n * p.K;
    const size_t N = (size_t)n, R = (size_t)p.R, C = (size_t)p.C, H = (size_t)p.H;
    size_t o = 0;
    auto take = [&](size_t words) { size_t r = o; o += (words * 4 + 255) & ~size_t(255); return r; };      // 4-byte elements
    p.term = take(N * p.Fn); p.tok = take(R * (C + p.Ft)); p.z = take(N * (C + p.Fn));
    for (int l = 0; l <= p.L; ++l) p.x[l] = take(R * C);
    for (int l = 0; l < p.L; ++l) {
        Layer& v = p.layer[l];
        v.x1 = take(R * C); v.y = take(R * C); v.mean = take(R); v.rstd = take(R); v.hpre = take(R * H); v.hact = take(R * H);
    }
    p.tmp = take(R * C);
    p.dmean = take(N * C); p.gA = take(R * C); p.gB = take(R * C); p.gC = take(R * C); p.gD = take(R * C); p.gE = take(R * C); p.dhid = take(R * H);
    p.tpart = take(N * p.P);
    const size_t row_part = (size_t)ceil_div(p.R, tgt::kColRows) * (H > C ? H : C), root_cols = (size_t)(p.P > p.Fn ? p.P : p.Fn);
    const size_t root_part = (size_t)ceil_div(n, tgt::kColRows) * root_cols;
    p.part = take(row_part > root_part ? row_part : root_part);
    p.total = o;
    return p;
}

static int check_weights(const dygnn_graphmixer_weights* w, int L, bool time_encoder, const char* what) {
    DYGNN_REQUIRE(w && (!time_encoder || (w->time_w && w->time_b)) && w->proj_w && w->proj_b && w->output_w && w->output_b, "graphmixer: %s", what);
    for (int l = 0; l < L; ++l) {
        const dygnn_mixer_layer_weights& m = w->layers[l];
        DYGNN_REQUIRE(m.token_norm_w && m.token_norm_b && m.token_fc0_w && m.token_fc0_b && m.token_fc1_w && m.token_fc1_b && m.channel_norm_w &&
                      m.channel_norm_b && m.channel_fc0_w && m.channel_fc0_b && m.channel_fc1_w && m.channel_fc1_b,
                      "graphmixer: %s (layer %d)", what, l);
    }
    return DYGNN_OK;
}

// R = n K rows are counted in int by the products; element offsets are 64-bit everywhere
constexpr int64_t kMaxRoots = INT32_MAX / kMaxTokens;
static unsigned blocks(int64_t count) { return (unsigned)ceil_div(count, 256); }

}  // namespace gmt
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::gmt;

extern "C" size_t dygnn_graphmixer_train_workspace_bytes(const dygnn_graphmixer_config* cfg, int64_t n_roots) {
    if (gm::check_graphmixer(cfg) != DYGNN_OK) return 0;
    if (n_roots < 0 || n_roots > kMaxRoots) { set_error("graphmixer: n_roots must be in [0, %lld]", (long long)kMaxRoots); return 0; }
    return make_plan(*cfg, n_roots > 0 ? n_roots : 1).total;
}

extern "C" int dygnn_graphmixer_train_forward(const dygnn_graphmixer_config* cfg, const dygnn_graphmixer_weights* w, const dygnn_csr* csr,
                                              const float* node_feat, const float* edge_feat, const int64_t* nodes, const double* times, int64_t n,
                                              float dropout_p, uint64_t seed, float* out, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = gm::check_graphmixer(cfg)) return rc;
    if (int rc = check_weights(w, cfg->num_layers, true, "null weights")) return rc;
    DYGNN_REQUIRE(csr && csr->indptr && csr->num_nodes >= 1 && (csr->num_entries == 0 || (csr->nbr && csr->eid && csr->ts)), "graphmixer: bad csr");
    DYGNN_REQUIRE(n >= 0 && n <= kMaxRoots && node_feat && edge_feat, "graphmixer: bad arguments");
    if (n == 0) return DYGNN_OK;
    DYGNN_REQUIRE(nodes && times && out && workspace, "graphmixer: null pointer");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "graphmixer: dropout must be in [0, 1)");
    const Plan p = make_plan(*cfg, n);
    if (workspace_bytes < p.total) {
        set_error("graphmixer: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int K = p.K, Kh = p.Kh, C = p.C, Ft = p.Ft, Fn = p.Fn, H = p.H, R = (int)p.R;
    const int64_t node_rows = cfg->num_node_rows > 0 ? cfg->num_node_rows : csr->num_nodes;
    const Csr g{csr->indptr, csr->nbr, csr->eid, csr->ts, csr->num_nodes};
    const train::Drop dr = train::make_drop(dropout_p, seed);

    if (int rc = gm::node_term(s, g, node_feat, nodes, times, n, Fn, cfg->time_gap, F32(p.term))) return rc;
    if (int rc = gm::project(s, g, edge_feat, nodes, times, n, *w, K, C, Ft, F32(p.x[0]))) return rc;
    hipLaunchKernelGGL(k_gmt_rows, dim3((unsigned)n), dim3(256), 0, s, g, edge_feat, nodes, times, w->time_w, w->time_b, K, C, Ft, F32(p.tok));
    DYGNN_LAUNCH_CHECK();
    const size_t lds_tok = (size_t)(K + Kh) * C * sizeof(float);
    if (int rc = tile::lds_limit(k_gmt_token_fwd, lds_tok)) return rc;
    for (int l = 0; l < p.L; ++l) {
        const dygnn_mixer_layer_weights& m = w->layers[l];
        const Layer& v = p.layer[l];
        const uint32_t site = 4u * (uint32_t)l;
        hipLaunchKernelGGL(k_gmt_token_fwd, dim3((unsigned)n), dim3(256), lds_tok, s, F32(p.x[l]), F32(v.x1), m.token_norm_w, m.token_norm_b, m.token_fc0_w,
                           m.token_fc0_b, m.token_fc1_w, m.token_fc1_b, K, Kh, C, dr, site);
        DYGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_gmt_ln_fwd, dim3((unsigned)ceil_div(p.R, 4)), dim3(256), 0, s, F32(v.x1), m.channel_norm_w, m.channel_norm_b, p.R, C, F32(v.y),
                           F32(v.mean), F32(v.rstd));
        DYGNN_LAUNCH_CHECK();
        if (int rc = train::mm(s, F32(v.y), C, false, m.channel_fc0_w, C, true, F32(v.hpre), H, R, H, C, train::MmOpt().bias(m.channel_fc0_b))) return rc;
        hipLaunchKernelGGL(train::k_gelu_drop, dim3(blocks(p.R * H)), dim3(256), 0, s, F32(v.hpre), p.R * H, dr, site + 2, F32(v.hact));
        DYGNN_LAUNCH_CHECK();
        if (int rc = train::mm(s, F32(v.hact), H, false, m.channel_fc1_w, H, true, F32(p.tmp), C, R, C, H, train::MmOpt().bias(m.channel_fc1_b))) return rc;
        hipLaunchKernelGGL(train::k_drop_add, dim3(blocks(p.R * C)), dim3(256), 0, s, F32(v.x1), F32(p.tmp), p.R * C, dr, site + 3, F32(p.x[l + 1]));
        DYGNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_gmt_cat, dim3(blocks(n * (C + Fn))), dim3(256), 0, s, F32(p.x[p.L]), F32(p.term), node_feat, nodes, n, node_rows, K, C, Fn, F32(p.z));
    DYGNN_LAUNCH_CHECK();
    return train::mm(s, F32(p.z), C + Fn, false, w->output_w, C + Fn, true, out, Fn, (int)n, Fn, C + Fn, train::MmOpt().bias(w->output_b));
}

extern "C" int dygnn_graphmixer_backward(const dygnn_graphmixer_config* cfg, const dygnn_graphmixer_weights* w, const dygnn_graphmixer_weights* grads,
                                         const float* grad_out, int64_t n, float dropout_p, uint64_t seed, void* workspace, size_t workspace_bytes,
                                         dygnn_stream_t stream) {
    if (int rc = gm::check_graphmixer(cfg)) return rc;
    if (int rc = check_weights(w, cfg->num_layers, true, "null weights")) return rc;
    if (int rc = check_weights(grads, cfg->num_layers, false, "null gradient buffer")) return rc;
    DYGNN_REQUIRE(n >= 0 && n <= kMaxRoots, "graphmixer: bad arguments");
    if (n == 0) return DYGNN_OK;
    DYGNN_REQUIRE(grad_out && workspace, "graphmixer: null pointer");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "graphmixer: dropout must be in [0, 1)");
    const Plan p = make_plan(*cfg, n);
    if (workspace_bytes < p.total) {
        set_error("graphmixer: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto G = [](const float* g) { return const_cast<float*>(g); };
    const int K = p.K, Kh = p.Kh, C = p.C, Ft = p.Ft, Fn = p.Fn, H = p.H, R = (int)p.R, P = p.P;
    const train::Drop dr = train::make_drop(dropout_p, seed);
    float *dmean = F32(p.dmean), *gA = F32(p.gA), *gB = F32(p.gB), *gC = F32(p.gC), *gD = F32(p.gD), *gE = F32(p.gE), *dhid = F32(p.dhid),
          *tpart = F32(p.tpart), *part = F32(p.part);
    auto cs = [&](const float* A, int cols, const float* out) { return colsum(s, A, cols, p.R, cols, part, out); };

    // output_layer: its input's first C columns are the token mean, whose gradient goes to the K rows as 1 / K
    if (int rc = train::mm(s, grad_out, Fn, false, w->output_w, C + Fn, false, dmean, C, (int)n, C, Fn)) return rc;
    {
        const train::DwPair pair{grad_out, Fn, Fn, F32(p.z), C + Fn, C + Fn, G(grads->output_w), C + Fn, nullptr};
        if (int rc = train::dw_grouped(s, (int)n, &pair, 1)) return rc;
        if (int rc = colsum(s, grad_out, Fn, n, Fn, part, grads->output_b)) return rc;
    }
    hipLaunchKernelGGL(k_gmt_bcast, dim3(blocks(p.R * C)), dim3(256), 0, s, dmean, gA, p.R * C, K, C);
    DYGNN_LAUNCH_CHECK();
    const size_t lds_tok = (size_t)(3 * K + 2 * Kh) * (C | 1) * sizeof(float);
    if (int rc = tile::lds_limit(k_gmt_token_bwd, lds_tok)) return rc;
    for (int l = p.L - 1; l >= 0; --l) {                                 // gA = the gradient of block l's output
        const dygnn_mixer_layer_weights& m = w->layers[l];
        const dygnn_mixer_layer_weights& g = grads->layers[l];
        const Layer& v = p.layer[l];
        const uint32_t site = 4u * (uint32_t)l;
        // channel half: site-3 mask, fc1^T, site-2 mask and GELU', fc0^T, LayerNorm
        hipLaunchKernelGGL(train::k_drop_bwd, dim3(blocks(p.R * C)), dim3(256), 0, s, gA, p.R * C, dr, site + 3, gC);
        DYGNN_LAUNCH_CHECK();
        if (int rc = cs(gC, C, g.channel_fc1_b)) return rc;
        if (int rc = train::mm(s, gC, C, false, m.channel_fc1_w, H, false, dhid, H, R, H, C)) return rc;
        hipLaunchKernelGGL(train::k_gelu_drop_bwd, dim3(blocks(p.R * H)), dim3(256), 0, s, dhid, F32(v.hpre), p.R * H, dr, site + 2);
        DYGNN_LAUNCH_CHECK();
        if (int rc = cs(dhid, H, g.channel_fc0_b)) return rc;
        if (int rc = train::mm(s, dhid, H, false, m.channel_fc0_w, C, false, gB, C, R, C, H)) return rc;
        hipLaunchKernelGGL(k_gmt_ln_bwd, dim3((unsigned)ceil_div(p.R, 4)), dim3(256), 0, s, gB, F32(v.x1), F32(v.mean), F32(v.rstd), m.channel_norm_w, gA, p.R, C,
                           gD, gE);
        DYGNN_LAUNCH_CHECK();
        if (int rc = cs(gE, C, g.channel_norm_w)) return rc;
        if (int rc = cs(gB, C, g.channel_norm_b)) return rc;
        const train::DwPair pairs[2] = {{dhid, H, H, F32(v.y), C, C, G(g.channel_fc0_w), C, nullptr},
                                        {gC, C, C, F32(v.hact), H, H, G(g.channel_fc1_w), H, nullptr}};
        if (int rc = train::dw_grouped(s, R, pairs, 2)) return rc;
        // token half: gD = the gradient of the half's output -> of the block's input, in place
        hipLaunchKernelGGL(k_gmt_token_bwd, dim3((unsigned)n), dim3(256), lds_tok, s, F32(p.x[l]), gD, m.token_norm_w, m.token_norm_b, m.token_fc0_w,
                           m.token_fc0_b, m.token_fc1_w, K, Kh, C, dr, site, tpart);
        DYGNN_LAUNCH_CHECK();
        train::ColSegs sg{};
        const int sizes[6] = {Kh * K, Kh, K * Kh, K, K, K};
        float* outs[6] = {G(g.token_fc0_w), G(g.token_fc0_b), G(g.token_fc1_w), G(g.token_fc1_b), G(g.token_norm_w), G(g.token_norm_b)};
        for (int k = 0, e = 0; k < 6; ++k) { e += sizes[k]; sg.out[k] = outs[k]; sg.end[k] = e; }
        if (int rc = colsum(s, tpart, P, n, P, part, sg)) return rc;
        float* t = gA; gA = gD; gD = t;
    }
    // projection_layer: gA = the gradient of its output
    if (int rc = cs(gA, C, grads->proj_b)) return rc;
    const train::DwPair pair{gA, C, C, F32(p.tok), C + Ft, C + Ft, G(grads->proj_w), C + Ft, nullptr};
    return train::dw_grouped(s, R, &pair, 1);
}
