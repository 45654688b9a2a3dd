// GraphMixer inference forward (models/GraphMixer.py:70-150, MLPMixer :200-244), fp32, gfx950.  Five kernels per call:
//   k_gm_node   one root per workgroup: history search, then the windowed row sum of the node encoder straight off the CSR row
//   k_gm_proj   one root per workgroup: sample K, gather edge rows, time-encode, projection_layer (fp32 MFMA)        -> X [n K, C]
//   k_gm_token  one root per workgroup, per Mixer block: token LayerNorm + token FFN + residual over the [K, C] tile  -> X in place
//   k_gm_ffn    64 token rows per workgroup, per Mixer block: channel LayerNorm + C -> 4C -> C FFN + residual; the hidden rows live in LDS,
//               64 columns at a time, and never reach memory                                                          -> X in place
//   k_gm_out    16 roots per workgroup: token mean, [mean | node term + node_feat[v]], output_layer                    -> out [n, Fn]
// The workspace is X and the node term: n (K C + Fn) floats.  Nothing has a time_gap dimension.
//
// Products use the fp32 MFMA tile product of mfma_tile.h.
#include "common.h"
#include "gelu_exact.h"
#include "graphmixer.h"
#include "mfma_tile.h"
#include "time_encoding.h"

namespace dygnn {
namespace gm {

using timeenc::cos_time;
using tile::f4;
using tile::kThreads;
using tile::kWaves;
using tile::lds_limit;
using tile::mfma4;
using tile::round16;
using tile::wave_product;
using tile::z4;

constexpr int kFfnRows = 64;      // token rows per workgroup of k_gm_ffn
constexpr int kFfnChunk = 64;     // hidden columns in LDS at a time
constexpr int kOutRoots = 16;

// ---- node encoder (models/GraphMixer.py:117-141) ---------------------------------------------------------------------------------------------
// One root per workgroup, so a hub root (m = time_gap rows) holds up nobody: short roots retire and their slots are refilled.  The four waves
// take the rows j = 4 wave + u (mod 16), u < 4: four 16-byte-per-lane row loads in flight per wave, lanes across the row (Fn / 4 <= 64 lanes).
// Sums are fp32 in a fixed order (16 partial sums per root, ascending j in each, then a fixed tree): deterministic.
__global__ __launch_bounds__(kThreads) void k_gm_node(Csr g, const float* __restrict__ node_feat, const int64_t* __restrict__ nodes,
                                                        const double* __restrict__ times, int Fn, int G, float* __restrict__ term) {
    __shared__ f4 part[kWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    int64_t lo, end;
    history(g, nodes[q], times[q], lane, lo, end);
    const int64_t len = end - lo;
    const int m = (int)(len < G ? len : G);
    const int64_t first = end - m;
    const bool on = lane < (Fn >> 2);
    const float* col = node_feat + 4 * lane;
    f4 acc[4] = {z4(), z4(), z4(), z4()};                               // one partial sum per row in flight: 16 per root, each over <= m / 16 rows
    for (int j = 4 * wave; j < m; j += 4 * kWaves) {
        f4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            r[u] = z4();
            if (j + u < m) {                                          // wave-uniform
                const int32_t nb = g.nbr[first + j + u];
                if (on) r[u] = *reinterpret_cast<const f4*>(col + (size_t)nb * Fn);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] += r[u];
    }
    part[wave][lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    __syncthreads();
    if (wave == 0 && on) {
        f4 s;
        if (m == 0) s = *reinterpret_cast<const f4*>(col);         // all slots masked: uniform softmax over time_gap copies of row 0
        else s = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
        const float d = (float)(m == 0 ? 1 : m), Gf = (float)G;
        s = f4{s.x / d / Gf, s.y / d / Gf, s.z / d / Gf, s.w / d / Gf};
        *reinterpret_cast<f4*>(term + (size_t)q * Fn + 4 * lane) = s;
    }
}

// ---- link encoder: tokens and projection (models/GraphMixer.py:86-104) -----------------------------------------------------------------------
// LDS: the root's token rows [32][lda], lda = round16(C + Ft) + 4 (rows K..31 and the columns beyond C + Ft are zero)
__global__ __launch_bounds__(kThreads) void k_gm_proj(Csr g, const float* __restrict__ edge_feat, const int64_t* __restrict__ nodes,
                                                        const double* __restrict__ times, const float* __restrict__ tw, const float* __restrict__ tb,
                                                        const float* __restrict__ W, const float* __restrict__ bias, int K, int C, int Ft,
                                                        float* __restrict__ X) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int32_t s_eid[kMaxTokens];
    __shared__ float s_dt[kMaxTokens];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    const int Kdim = C + Ft, Kp = round16(Kdim), lda = Kp + 4;
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
            dt = (float)(t - (double)(float)g.ts[p]);                  // f64 - f32 -> f64 -> .float(), as k_tgat_expand
        }
        s_eid[j] = e; s_dt[j] = dt;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kMaxTokens * Kp; i += kThreads) {
        const int j = i / Kp, f = i - j * Kp;
        float v = 0.f;
        if (j < K) {
            if (f < C) v = edge_feat[(size_t)s_eid[j] * C + f];        // a padded slot reads edge row 0
            else if (f < Kdim && j >= pad) v = cos_time(fmaf(s_dt[j], tw[f - C], tb[f - C]));      // time features of a padded slot are zero
        }
        smem[j * lda + f] = v;
    }
    __syncthreads();
    f4 acc[4][2];
#pragma unroll
    for (int t_ = 0; t_ < 4; ++t_) { acc[t_][0] = z4(); acc[t_][1] = z4(); }
    wave_product<4, 2>(smem, lda, W, Kdim, 0, C, Kdim, wave, lane, acc);
    const int c = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
    for (int t_ = 0; t_ < 4; ++t_) {
        const int n = 16 * (wave + kWaves * t_) + g4;
        if (n >= C) continue;
        const f4 b = *reinterpret_cast<const f4*>(bias + n);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int j = 16 * mt + c;
            if (j < K) *reinterpret_cast<f4*>(X + ((size_t)q * K + j) * C + n) = acc[t_][mt] + b;
        }
    }
}

// ---- Mixer block, token half (models/GraphMixer.py:228-234) ------------------------------------------------------------------------------------
// One thread per channel: everything it touches is its own column of the LDS tiles, so the kernel has one barrier (after the tile load).
// LDS: T [K][C] (x, then the normalised column), Hd [Kh][C].
__global__ __launch_bounds__(kThreads) void k_gm_token(float* __restrict__ X, const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                         const float* __restrict__ W0, const float* __restrict__ b0, const float* __restrict__ W1,
                                                         const float* __restrict__ b1, int K, int Kh, int C) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* T = smem;
    float* Hd = smem + K * C;
    float* x = X + (size_t)blockIdx.x * K * C;
    for (int i = threadIdx.x; i < (K * C) >> 2; i += kThreads) reinterpret_cast<f4*>(T)[i] = reinterpret_cast<const f4*>(x)[i];
    __syncthreads();
    for (int ch = threadIdx.x; ch < C; ch += kThreads) {
        // the mean with one refinement pass: a root with no (or one) neighbour has K (nearly) identical tokens, the variance is ~0 and
        // 1 / sqrt(var + eps) = 316 multiplies whatever rounding error the mean carries; refined, identical tokens give exactly zero deviations
        float s = 0.f;
        for (int j = 0; j < K; ++j) s += T[j * C + ch];
        float mean = s / (float)K;
        s = 0.f;
        for (int j = 0; j < K; ++j) s += T[j * C + ch] - mean;
        mean += s / (float)K;
        float v = 0.f;
        for (int j = 0; j < K; ++j) { const float d = T[j * C + ch] - mean; v = fmaf(d, d, v); }
        const float rstd = 1.0f / sqrtf(v / (float)K + kLnEps);
        for (int j = 0; j < K; ++j) T[j * C + ch] = fmaf((T[j * C + ch] - mean) * rstd, ln_w[j], ln_b[j]);
        for (int i = 0; i < Kh; ++i) {
            float a = b0[i];
            for (int j = 0; j < K; ++j) a = fmaf(W0[i * K + j], T[j * C + ch], a);
            Hd[i * C + ch] = gelu_exact(a);
        }
        for (int j = 0; j < K; ++j) {
            float a = b1[j];
            for (int i = 0; i < Kh; ++i) a = fmaf(W1[j * Kh + i], Hd[i * C + ch], a);
            x[(size_t)j * C + ch] += a;                              // residual on the block's input
        }
    }
}

// ---- Mixer block, channel half (models/GraphMixer.py:236-242) ----------------------------------------------------------------------------------
// LDS: A [64][lda] the rows' LayerNorm output (lda = round16(C) + 4, zero beyond C), Hc [64][ldh] one chunk of GELU'd hidden columns.
// Per chunk: stage 1, wave w computes hidden columns 16 w .. 16 w + 15 of the chunk for all 64 rows (K = C); barrier; stage 2, every wave adds the
// chunk's contribution to its output tiles (columns 16 (w + 4 t), 64 accumulator registers per lane); barrier.  The block's weights are read
// once per workgroup, straight from L2.
__global__ __launch_bounds__(kThreads) void k_gm_ffn(float* __restrict__ X, int64_t R, const float* __restrict__ ln_w, const float* __restrict__ ln_b,
                                                       const float* __restrict__ W0, const float* __restrict__ b0, const float* __restrict__ W1,
                                                       const float* __restrict__ b1, int C, int Hdim) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Cp = round16(C), lda = Cp + 4, ldh = kFfnChunk + 4;
    float* A = smem;
    float* Hc = smem + kFfnRows * lda;
    const int64_t r0 = (int64_t)blockIdx.x * kFfnRows;
    const int C4 = C >> 2, lda4 = lda >> 2;
    for (int i = threadIdx.x; i < kFfnRows * lda4; i += kThreads) {
        const int r = i / lda4, c4 = i - r * lda4;
        f4 v = z4();
        if (c4 < C4 && r0 + r < R) v = *reinterpret_cast<const f4*>(X + (size_t)(r0 + r) * C + 4 * c4);
        *reinterpret_cast<f4*>(A + r * lda + 4 * c4) = v;
    }
    __syncthreads();
    for (int r = wave; r < kFfnRows; r += kWaves) {                   // channel LayerNorm in place, one wave per row
        float* row = A + r * lda;
        float s = 0.f;
        for (int f = lane; f < C; f += 64) s += row[f];
        float mean = wave_sum(s) / (float)C;
        s = 0.f;
        for (int f = lane; f < C; f += 64) s += row[f] - mean;            // refinement pass, as in k_gm_token
        mean += wave_sum(s) / (float)C;
        float v = 0.f;
        for (int f = lane; f < C; f += 64) { const float d = row[f] - mean; v = fmaf(d, d, v); }
        const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)C + kLnEps);
        for (int f = lane; f < C; f += 64) row[f] = fmaf((row[f] - mean) * rstd, ln_w[f], ln_b[f]);
    }
    __syncthreads();
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    f4 out[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) out[t][mt] = z4();
    for (int h0 = 0; h0 < Hdim; h0 += kFfnChunk) {
        const int hn = Hdim - h0 < kFfnChunk ? Hdim - h0 : kFfnChunk;      // live hidden columns of this chunk (a multiple of 16)
        f4 hid[1][4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) hid[0][mt] = z4();
        wave_product<1, 4>(A, lda, W0 + (size_t)h0 * C, C, 0, hn, C, wave, lane, hid);
        {
            const int hcol = 16 * wave + g4;                           // column inside the chunk
            f4 b = z4();
            if (hcol < hn) b = *reinterpret_cast<const f4*>(b0 + h0 + hcol);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                f4 v = z4();
                if (hcol < hn) {
                    const f4 z = hid[0][mt] + b;
                    v = f4{gelu_exact(z.x), gelu_exact(z.y), gelu_exact(z.z), gelu_exact(z.w)};
                }
                *reinterpret_cast<f4*>(Hc + (16 * mt + c) * ldh + hcol) = v;      // dead columns are zero: stage 2 runs over the whole chunk
            }
        }
        __syncthreads();
        wave_product<4, 4>(Hc, ldh, W1, Hdim, h0, C, hn, wave, lane, out);
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = 16 * (wave + kWaves * t) + g4;
        if (n >= C) continue;
        const f4 b = *reinterpret_cast<const f4*>(b1 + n);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int64_t r = r0 + 16 * mt + c;
            if (r >= R) continue;
            f4* p = reinterpret_cast<f4*>(X + (size_t)r * C + n);
            *p = (out[t][mt] + b) + *p;                               // residual on the channel half's input
        }
    }
}

// ---- token mean, node part, output_layer (models/GraphMixer.py:106-148) ------------------------------------------------------------------------
// LDS: [16][lda] rows [mean over the K tokens | node term + node_feat[v]], lda = round16(C + Fn) + 4
__global__ __launch_bounds__(kThreads) void k_gm_out(const float* __restrict__ X, const float* __restrict__ term, const float* __restrict__ node_feat,
                                                       const int64_t* __restrict__ nodes, int64_t n, int64_t node_rows, const float* __restrict__ W,
                                                       const float* __restrict__ bias, int K, int C, int Fn, float* __restrict__ out,
                                                       float* __restrict__ tap_mean, int64_t tap_rows) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Kdim = C + Fn, Kp = round16(Kdim), lda = Kp + 4;
    const int64_t q0 = (int64_t)blockIdx.x * kOutRoots;
    for (int i = threadIdx.x; i < kOutRoots * Kp; i += kThreads) {
        const int r = i / Kp, f = i - r * Kp;
        const int64_t q = q0 + r;
        float v = 0.f;
        if (q < n && f < C) {
            const float* x = X + (size_t)q * K * C + f;
            float s = 0.f;
            for (int j = 0; j < K; ++j) s += x[(size_t)j * C];
            v = s / (float)K;
            if (tap_mean && q < tap_rows) tap_mean[(size_t)q * C + f] = v;
        } else if (q < n && f < Kdim) {
            int64_t node = nodes[q];
            if (node < 0 || node >= node_rows) node = 0;
            v = term[(size_t)q * Fn + (f - C)] + node_feat[(size_t)node * Fn + (f - C)];
        }
        smem[r * lda + f] = v;
    }
    __syncthreads();
    f4 acc[4][1];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t][0] = z4();
    wave_product<4, 1>(smem, lda, W, Kdim, 0, Fn, Kdim, wave, lane, acc);
    const int c = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int nn = 16 * (wave + kWaves * t) + g4;
        if (nn >= Fn || q0 + c >= n) continue;
        *reinterpret_cast<f4*>(out + (size_t)(q0 + c) * Fn + nn) = acc[t][0] + *reinterpret_cast<const f4*>(bias + nn);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
#define GM_SUPPORTED(cond, ...)                                   \
    do {                                                          \
        if (!(cond)) {                                            \
            set_error(__VA_ARGS__);                               \
            return DYGNN_E_UNSUPPORTED;                           \
        }                                                         \
    } while (0)

int check_graphmixer(const dygnn_graphmixer_config* c) {
    DYGNN_REQUIRE(c != nullptr, "graphmixer: config is NULL");
    // utils/utils.py:157, for the link encoder's and the node encoder's sampler call
    DYGNN_REQUIRE(c->num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!");
    DYGNN_REQUIRE(c->time_gap > 0, "graphmixer: time_gap must be greater than 0 (Number of sampled neighbors for each node should be greater than 0!)");
    // the token LayerNorm / FFN have num_tokens entries: any other num_neighbors is a shape error in the reference (models/GraphMixer.py:229)
    DYGNN_REQUIRE(c->num_neighbors == c->num_tokens, "graphmixer: num_neighbors (%d) must equal num_tokens (%d)", c->num_neighbors, c->num_tokens);
    DYGNN_REQUIRE(c->node_feat_dim > 0 && c->edge_feat_dim > 0 && c->time_feat_dim > 0, "graphmixer: feature dims must be positive");
    DYGNN_REQUIRE(c->num_layers >= 1 && c->num_node_rows >= 0, "graphmixer: num_layers must be at least 1, num_node_rows non-negative");
    GM_SUPPORTED(c->num_layers <= DYGNN_MAX_LAYERS, "graphmixer: num_layers %d > %d not supported", c->num_layers, DYGNN_MAX_LAYERS);
    GM_SUPPORTED(c->num_tokens >= 2 && c->num_tokens <= kMaxTokens,
                 "graphmixer: num_tokens %d not supported (2..%d; one token has a zero-width token FFN)", c->num_tokens, kMaxTokens);
    GM_SUPPORTED(c->token_hidden_dim >= 1 && c->token_hidden_dim <= kMaxTokens / 2 && c->token_hidden_dim <= c->num_tokens,
                 "graphmixer: token_hidden_dim %d not supported (1..%d, at most num_tokens)", c->token_hidden_dim, kMaxTokens / 2);
    GM_SUPPORTED(c->node_feat_dim % 4 == 0 && c->edge_feat_dim % 4 == 0 && c->time_feat_dim % 4 == 0, "graphmixer: feature dims must be multiples of 4");
    GM_SUPPORTED(c->node_feat_dim <= 256 && c->edge_feat_dim <= 256 && c->time_feat_dim <= 256, "graphmixer: feature dims > 256 not supported");
    GM_SUPPORTED(c->channel_hidden_dim >= 16 && c->channel_hidden_dim % 16 == 0 && c->channel_hidden_dim <= 1024,
                 "graphmixer: channel_hidden_dim %d not supported (a multiple of 16, at most 1024)", c->channel_hidden_dim);
    return DYGNN_OK;
}

int node_term(hipStream_t s, const Csr& g, const float* node_feat, const int64_t* nodes, const double* times, int64_t n, int Fn, int G, float* term) {
    hipLaunchKernelGGL(k_gm_node, dim3((unsigned)n), dim3(kThreads), 0, s, g, node_feat, nodes, times, Fn, G, term);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

int project(hipStream_t s, const Csr& g, const float* edge_feat, const int64_t* nodes, const double* times, int64_t n, const dygnn_graphmixer_weights& w,
            int K, int C, int Ft, float* X) {
    const size_t lds_proj = (size_t)kMaxTokens * (round16(C + Ft) + 4) * sizeof(float);
    if (int rc = lds_limit(k_gm_proj, lds_proj)) return rc;
    hipLaunchKernelGGL(k_gm_proj, dim3((unsigned)n), dim3(kThreads), lds_proj, s, g, edge_feat, nodes, times, w.time_w, w.time_b, w.proj_w, w.proj_b, K, C, Ft, X);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Plan {
    size_t x, term, total;       // byte offsets: X [n K C], the node term [n Fn]
};
static Plan make_plan(const dygnn_graphmixer_config& c, int64_t n) {
    Plan p;
    p.x = 0;
    p.term = align256((size_t)n * c.num_tokens * c.edge_feat_dim * sizeof(float));
    p.total = p.term + align256((size_t)n * c.node_feat_dim * sizeof(float));
    return p;
}

}  // namespace gm
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::gm;

extern "C" int dygnn_graphmixer_check(const dygnn_graphmixer_config* cfg) { return check_graphmixer(cfg); }

extern "C" size_t dygnn_graphmixer_workspace_bytes(const dygnn_graphmixer_config* cfg, int64_t n_roots) {
    if (check_graphmixer(cfg) != DYGNN_OK) return 0;
    if (n_roots < 0) { set_error("graphmixer: n_roots must be non-negative"); return 0; }
    return make_plan(*cfg, n_roots > 0 ? n_roots : 1).total;
}

extern "C" int dygnn_graphmixer_forward(const dygnn_graphmixer_config* cfg, const dygnn_graphmixer_weights* w, const dygnn_csr* csr,
                                        const float* node_feat, const float* edge_feat, const int64_t* nodes, const double* times, int64_t n,
                                        float* out, const dygnn_graphmixer_taps* taps, void* workspace, size_t workspace_bytes,
                                        dygnn_stream_t stream) {
    if (int rc = check_graphmixer(cfg)) return rc;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && w->proj_w && w->proj_b && w->output_w && w->output_b, "graphmixer: null weights");
    for (int l = 0; l < cfg->num_layers; ++l) {
        const dygnn_mixer_layer_weights& m = w->layers[l];
        DYGNN_REQUIRE(m.token_norm_w && m.token_norm_b && m.token_fc0_w && m.token_fc0_b && m.token_fc1_w && m.token_fc1_b && m.channel_norm_w &&
                      m.channel_norm_b && m.channel_fc0_w && m.channel_fc0_b && m.channel_fc1_w && m.channel_fc1_b,
                      "graphmixer: null layer weights (layer %d)", l);
    }
    DYGNN_REQUIRE(csr && csr->indptr && csr->num_nodes >= 1 && (csr->num_entries == 0 || (csr->nbr && csr->eid && csr->ts)), "graphmixer: bad csr");
    DYGNN_REQUIRE(n >= 0 && n <= INT32_MAX && node_feat && edge_feat, "graphmixer: bad arguments");
    if (n == 0) return DYGNN_OK;
    DYGNN_REQUIRE(nodes && times && out && workspace, "graphmixer: null pointer");
    const Plan p = make_plan(*cfg, n);
    if (workspace_bytes < p.total) {
        set_error("graphmixer: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    const int Fn = cfg->node_feat_dim, C = cfg->edge_feat_dim, Ft = cfg->time_feat_dim, K = cfg->num_tokens, Kh = cfg->token_hidden_dim;
    const int Hdim = cfg->channel_hidden_dim, G = cfg->time_gap;
    const int64_t node_rows = cfg->num_node_rows > 0 ? cfg->num_node_rows : csr->num_nodes;
    hipStream_t s = as_stream(stream);
    float* X = reinterpret_cast<float*>(static_cast<char*>(workspace) + p.x);
    float* term = reinterpret_cast<float*>(static_cast<char*>(workspace) + p.term);
    const Csr g{csr->indptr, csr->nbr, csr->eid, csr->ts, csr->num_nodes};
    const int64_t tap_rows = taps ? (taps->rows < n ? taps->rows : n) : 0;
    const size_t tap_bytes = (size_t)(tap_rows > 0 ? tap_rows : 0) * K * C * sizeof(float);

    if (int rc = node_term(s, g, node_feat, nodes, times, n, Fn, G, term)) return rc;
    if (int rc = project(s, g, edge_feat, nodes, times, n, *w, K, C, Ft, X)) return rc;
    if (tap_bytes && taps->projection) DYGNN_HIP(hipMemcpyAsync(taps->projection, X, tap_bytes, hipMemcpyDeviceToDevice, s));
    const size_t lds_tok = (size_t)(K + Kh) * C * sizeof(float);
    const size_t lds_ffn = (size_t)kFfnRows * ((round16(C) + 4) + (kFfnChunk + 4)) * sizeof(float);
    if (int rc = lds_limit(k_gm_token, lds_tok)) return rc;
    if (int rc = lds_limit(k_gm_ffn, lds_ffn)) return rc;
    const int64_t R = n * K;
    for (int l = 0; l < cfg->num_layers; ++l) {
        const dygnn_mixer_layer_weights& m = w->layers[l];
        hipLaunchKernelGGL(k_gm_token, dim3((unsigned)n), dim3(kThreads), lds_tok, s, X, m.token_norm_w, m.token_norm_b, m.token_fc0_w, m.token_fc0_b,
                           m.token_fc1_w, m.token_fc1_b, K, Kh, C);
        DYGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_gm_ffn, dim3((unsigned)ceil_div(R, kFfnRows)), dim3(kThreads), lds_ffn, s, X, R, m.channel_norm_w, m.channel_norm_b,
                           m.channel_fc0_w, m.channel_fc0_b, m.channel_fc1_w, m.channel_fc1_b, C, Hdim);
        DYGNN_LAUNCH_CHECK();
        if (tap_bytes && taps->layer_out[l]) DYGNN_HIP(hipMemcpyAsync(taps->layer_out[l], X, tap_bytes, hipMemcpyDeviceToDevice, s));
    }
    const size_t lds_out = (size_t)kOutRoots * (round16(C + Fn) + 4) * sizeof(float);
    hipLaunchKernelGGL(k_gm_out, dim3((unsigned)ceil_div(n, kOutRoots)), dim3(kThreads), lds_out, s, X, term, node_feat, nodes, n, node_rows, w->output_w,
                       w->output_b, K, C, Fn, out, tap_rows > 0 ? taps->token_mean : nullptr, tap_rows);
    DYGNN_LAUNCH_CHECK();
    if (tap_rows > 0 && taps->node_term)
        DYGNN_HIP(hipMemcpyAsync(taps->node_term, term, (size_t)tap_rows * Fn * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DYGNN_OK;
}
