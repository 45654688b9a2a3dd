// TCL inference forward (models/TCL.py:56-154, TransformerEncoder models/modules.py:209-266), fp32, gfx950.
//
// A call works on n_sides sides (root + K sampled neighbours, S = K + 1 positions) and P pairs of sides.  Sequences are stored as [S][d] row
// blocks; "rows" below are token rows across sequences.  Kernels:
//   k_tcl_encode  one side per workgroup: gather node / edge rows, time-encode, the three projections (fp32 MFMA) + depth embedding -> X0
//   k_tcl_qkv     64 token rows per workgroup, grid.y = {Q, K, V}: rows x in_proj (fp32 MFMA)                                       -> Q, K, V planes
//   k_tcl_attn    one (query sequence, key sequence) per workgroup, head by head: scores over <= 64 head columns at a time from LDS,
//                 masked softmax in LDS, weighted value sum                                                                          -> O
//   k_encoder_post<4, 4> (encoder_block.h, shared with cawn.hip)  64 token rows per workgroup: out_proj + residual, LayerNorm, d -> 4d (ReLU)
//                 -> d with the hidden rows in LDS 64 columns at a time, residual, LayerNorm (all products fp32 MFMA)              -> next X
//   k_tcl_out     16 rows per workgroup: output_layer on position 0 of every pair sequence                                          -> out_a, out_b
// A layer is two stages (self, cross) of qkv + attn + post.  The first self stage runs on the sides (a side shared by several pairs is
// computed once), and so does the Q / K / V product of the first cross stage; from there on everything runs on the 2 P sequences of the
// pairs (sequence 2 p is side a of pair p, 2 p + 1 side b).  The last cross stage computes only query position 0 (one row per sequence)
// unless taps are asked for.  No [n, S, S] array exists outside LDS.
#include <vector>

#include "common.h"
#include "encoder_block.h"
#include "mfma_tile.h"
#include "tcl.h"
#include "time_encoding.h"

namespace dygnn {
namespace tcl {

using timeenc::cos_time;
using encoder::k_encoder_post;
using encoder::load_rows;
using tile::f4;
using tile::kThreads;
using tile::kWaves;
using tile::lds_limit;
using tile::round16;
using tile::wave_product;
using tile::z4;

constexpr int kMaxSeq = 64;       // S = K + 1 <= 64: one row of scores per lane set, four row tiles
constexpr int kRows = 64;         // token rows per workgroup of k_tcl_qkv / k_encoder_post<4, 4>
constexpr int kOutRows = 16;
constexpr int kHeadChunk = 64;    // head columns of Q and K in LDS at a time

// ---- encoder input (models/TCL.py:84-128, :156-177) ---------------------------------------------------------------------------------------------
// LDS: A [16 MT][lda], lda = round16(max(Fn, Fe, Ft)) + 4, filled three times (node rows, edge rows, time encodings): the three products
// accumulate in the same registers.  Rows >= S and columns beyond the part's width are zero.
template <int MT>
__global__ __launch_bounds__(kThreads) void k_tcl_encode(const float* __restrict__ node_feat, const float* __restrict__ edge_feat,
                                                           const int64_t* __restrict__ side_root, const double* __restrict__ side_time,
                                                           const int64_t* __restrict__ nbr_id, const int64_t* __restrict__ nbr_eid,
                                                           const float* __restrict__ nbr_t, dygnn_tcl_weights w, int K, int Fn, int Fe, int Ft,
                                                           int64_t node_rows, int64_t edge_rows, float* __restrict__ X0) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ int64_t s_id[kMaxSeq], s_eid[kMaxSeq];
    __shared__ float s_dt[kMaxSeq];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    const int S = K + 1;
    int mx = Fn > Fe ? Fn : Fe;
    mx = mx > Ft ? mx : Ft;
    const int lda = round16(mx) + 4;
    if (threadIdx.x < kMaxSeq) {
        const int j = threadIdx.x;
        int64_t id = 0, e = 0;
        float dt = 0.f;
        if (j == 0) id = side_root[q];                               // the root: edge id 0, dt = t - t
        else if (j < S) {
            const double t = side_time[q];
            id = nbr_id[q * K + j - 1];
            e = nbr_eid[q * K + j - 1];
            dt = (float)(t - (double)nbr_t[q * K + j - 1]);             // f64 - f32 -> f64 -> .float()
        }
        s_id[j] = (id < 0 || id >= node_rows) ? 0 : id;
        s_eid[j] = (e < 0 || e >= edge_rows) ? 0 : e;
        s_dt[j] = dt;
    }
    f4 acc[4][MT];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = z4();
    for (int part = 0; part < 3; ++part) {
        const int dim = part == 0 ? Fn : part == 1 ? Fe : Ft, Kp = round16(dim);
        __syncthreads();                                             // s_* written / the previous product has read A
        for (int i = threadIdx.x; i < 16 * MT * Kp; i += kThreads) {
            const int j = i / Kp, f = i - j * Kp;
            float v = 0.f;
            if (j < S && f < dim) {
                if (part == 0) v = node_feat[(size_t)s_id[j] * Fn + f];
                else if (part == 1) v = edge_feat[(size_t)s_eid[j] * Fe + f];
                else v = cos_time(fmaf(s_dt[j], w.time_w[f], w.time_b[f]));
            }
            smem[j * lda + f] = v;
        }
        __syncthreads();
        const float* W = part == 0 ? w.proj_node_w : part == 1 ? w.proj_edge_w : w.proj_time_w;
        wave_product<4, MT>(smem, lda, W, dim, 0, Fn, dim, wave, lane, acc);
    }
    const int c = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = 16 * (wave + kWaves * t) + g4;
        if (n >= Fn) continue;
        const f4 b = (*reinterpret_cast<const f4*>(w.proj_node_b + n) + *reinterpret_cast<const f4*>(w.proj_edge_b + n)) +
                     *reinterpret_cast<const f4*>(w.proj_time_b + n);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int j = 16 * mt + c;
            if (j < S) *reinterpret_cast<f4*>(X0 + ((size_t)q * S + j) * Fn + n) = (acc[t][mt] + b) + *reinterpret_cast<const f4*>(w.depth_w + (size_t)j * Fn + n);
        }
    }
}

// ---- in_proj: Q, K, V of R token rows ---------------------------------------------------------------------------------------------------------------
// blockIdx.y picks the plane: QKV + y R d = X in_proj_weight[y d : (y + 1) d]^T + in_proj_bias[y d : (y + 1) d].  LDS: A [64][round16(d) + 4].
__global__ __launch_bounds__(kThreads) void k_tcl_qkv(const float* __restrict__ X, int64_t R, const float* __restrict__ W, const float* __restrict__ bias,
                                                        int d, float* __restrict__ QKV) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lda = round16(d) + 4, y = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    load_rows(smem, lda, kRows, X, r0, R, d);
    __syncthreads();
    f4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[t][mt] = z4();
    wave_product<4, 4>(smem, lda, W + (size_t)y * d * d, d, 0, d, d, wave, lane, acc);
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    float* out = QKV + (size_t)y * R * d;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = 16 * (wave + kWaves * t) + g4;
        if (n >= d) continue;
        const f4 b = *reinterpret_cast<const f4*>(bias + (size_t)y * d + n);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int64_t r = r0 + 16 * mt + c;
            if (r < R) *reinterpret_cast<f4*>(out + (size_t)r * d + n) = acc[t][mt] + b;
        }
    }
}

// ---- attention of one query sequence over one key sequence (nn.MultiheadAttention, key_padding_mask = (id == 0)) -------------------------------
// Workgroup i: queries are the first nq positions of sequence q_seq[i] (i when NULL), keys / values sequence kv_seq[i] (i ^ kv_xor when NULL),
// both in the planes Q / K / V [.][S][d]; the key mask is the id row of side mask_side[i] (i when NULL).  Per head: thread (row = e-th row of
// the wave's 16, key = lane) accumulates its score over chunks of <= 64 head columns staged in LDS (stride 65: the lanes of a wave read one Q
// element and 64 keys on 64 banks), the wave that owns a row does its softmax, then thread (row, column) sums the values, read coalesced.
// O is [n][nq][d].  LDS: Qc, Kc [64][65], P [64][65].
__global__ __launch_bounds__(kThreads) void k_tcl_attn(const float* __restrict__ Q, const float* __restrict__ Kp, const float* __restrict__ V,
                                                         const int32_t* __restrict__ q_seq, const int32_t* __restrict__ kv_seq, int kv_xor,
                                                         const int32_t* __restrict__ mask_side, const int64_t* __restrict__ side_root,
                                                         const int64_t* __restrict__ nbr_id, int K, int nq, int d, int H, float scale,
                                                         float* __restrict__ O) {
    constexpr int LD = kHeadChunk + 1;
    __shared__ float Qc[kMaxSeq * LD], Kc[kMaxSeq * LD], Pm[kMaxSeq * LD];
    __shared__ int s_valid[kMaxSeq];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = K + 1, dh = d / H;
    const int64_t i = blockIdx.x;
    const int64_t qs = q_seq ? q_seq[i] : i, ks = kv_seq ? kv_seq[i] : (i ^ kv_xor), ms = mask_side ? mask_side[i] : i;
    if (threadIdx.x < kMaxSeq) {
        const int j = threadIdx.x;
        s_valid[j] = j < S && (j == 0 ? side_root[ms] : nbr_id[ms * K + j - 1]) != 0;
    }
    const float* q = Q + (size_t)qs * S * d;
    const float* k = Kp + (size_t)ks * S * d;
    const float* v = V + (size_t)ks * S * d;
    float* o = O + (size_t)i * nq * d;
    for (int h = 0; h < H; ++h) {
        float sc[16];                                                // scores of rows wave + 4 e, key = lane
#pragma unroll
        for (int e = 0; e < 16; ++e) sc[e] = 0.f;
        for (int c0 = 0; c0 < dh; c0 += kHeadChunk) {
            const int cn = dh - c0 < kHeadChunk ? dh - c0 : kHeadChunk;
            __syncthreads();                                         // the previous chunk / head has been read
            for (int x = threadIdx.x; x < kMaxSeq * cn; x += kThreads) {
                const int r = x / cn, cc = x - r * cn;
                Qc[r * LD + cc] = r < nq ? q[(size_t)r * d + h * dh + c0 + cc] : 0.f;
                Kc[r * LD + cc] = r < S ? k[(size_t)r * d + h * dh + c0 + cc] : 0.f;
            }
            __syncthreads();
            for (int cc = 0; cc < cn; ++cc) {
                const float kk = Kc[lane * LD + cc];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int r = wave + kWaves * e;
                    if (r < nq) sc[e] = fmaf(Qc[r * LD + cc], kk, sc[e]);      // wave-uniform
                }
            }
        }
        const bool on = s_valid[lane] != 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int r = wave + kWaves * e;
            if (r >= nq) continue;
            const float s = on ? sc[e] * scale : -INFINITY;
            const float m = wave_max(s);
            const float ex = on ? expf(s - m) : 0.f;
            const float sum = wave_sum(ex);
            Pm[r * LD + lane] = sum > 0.f ? ex / sum : 0.f;         // no valid key: the sequence attends to nothing
        }
        __syncthreads();
        for (int x = threadIdx.x; x < nq * dh; x += kThreads) {
            const int r = x / dh, cc = x - r * dh;
            float a = 0.f;
            for (int j = 0; j < S; ++j) a = fmaf(Pm[r * LD + j], v[(size_t)j * d + h * dh + cc], a);
            o[(size_t)r * d + h * dh + cc] = a;
        }
    }
}

// ---- output_layer on position 0 of the 2 P pair sequences (models/TCL.py:150-152) ------------------------------------------------------------------
// Z [2 P][nq][d]; sequence 2 p -> out_a[p], 2 p + 1 -> out_b[p].  LDS: [16][round16(d) + 4]
__global__ __launch_bounds__(kThreads) void k_tcl_out(const float* __restrict__ Z, int64_t n, int nq, const float* __restrict__ W,
                                                        const float* __restrict__ bias, int d, float* __restrict__ out_a, float* __restrict__ out_b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Kp = round16(d), lda = Kp + 4;
    const int64_t q0 = (int64_t)blockIdx.x * kOutRows;
    for (int i = threadIdx.x; i < kOutRows * Kp; i += kThreads) {
        const int r = i / Kp, f = i - r * Kp;
        smem[r * lda + f] = (q0 + r < n && f < d) ? Z[(size_t)(q0 + r) * nq * d + f] : 0.f;
    }
    __syncthreads();
    f4 acc[4][1];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t][0] = z4();
    wave_product<4, 1>(smem, lda, W, d, 0, d, d, wave, lane, acc);
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    const int64_t q = q0 + c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int nn = 16 * (wave + kWaves * t) + g4;
        if (nn >= d || q >= n) continue;
        float* o = ((q & 1) ? out_b : out_a) + (size_t)(q >> 1) * d + nn;
        *reinterpret_cast<f4*>(o) = acc[t][0] + *reinterpret_cast<const f4*>(bias + nn);
    }
}

// taps: sequence seq[i] (i when NULL) of X [.][S][d] -> dst [n][S][d]
__global__ void k_tcl_tap(const float* __restrict__ X, const int32_t* __restrict__ seq, int64_t sd4, f4* __restrict__ dst) {
    const int64_t i = blockIdx.x;
    const f4* src = reinterpret_cast<const f4*>(X) + (size_t)(seq ? seq[i] : i) * sd4;
    for (int64_t x = threadIdx.x; x < sd4; x += blockDim.x) dst[i * sd4 + x] = src[x];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
#define TCL_SUPPORTED(cond, ...)                                  \
    do {                                                          \
        if (!(cond)) {                                            \
            set_error(__VA_ARGS__);                               \
            return DYGNN_E_UNSUPPORTED;                           \
        }                                                         \
    } while (0)

int check_tcl(const dygnn_tcl_config* c) {
    DYGNN_REQUIRE(c != nullptr, "tcl: config is NULL");
    DYGNN_REQUIRE(c->num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!");      // utils/utils.py:157
    DYGNN_REQUIRE(c->node_feat_dim > 0 && c->edge_feat_dim > 0 && c->time_feat_dim > 0, "tcl: feature dims must be positive");
    DYGNN_REQUIRE(c->num_layers >= 1 && c->num_heads >= 1, "tcl: num_layers and num_heads must be at least 1");
    DYGNN_REQUIRE(c->num_node_rows >= 1 && c->num_edge_rows >= 1, "tcl: num_node_rows and num_edge_rows must be at least 1");
    TCL_SUPPORTED(c->num_neighbors <= kMaxSeq - 1, "tcl: num_neighbors %d not supported (1..%d)", c->num_neighbors, kMaxSeq - 1);
    TCL_SUPPORTED(c->node_feat_dim % 4 == 0 && c->edge_feat_dim % 4 == 0 && c->time_feat_dim % 4 == 0,
                  "tcl: node_feat_dim, edge_feat_dim and time_feat_dim must be multiples of 4 (%d, %d, %d)", c->node_feat_dim, c->edge_feat_dim,
                  c->time_feat_dim);
    TCL_SUPPORTED(c->node_feat_dim <= 256, "tcl: node_feat_dim %d > 256 not supported", c->node_feat_dim);
    TCL_SUPPORTED(c->edge_feat_dim <= 256, "tcl: edge_feat_dim %d > 256 not supported", c->edge_feat_dim);
    TCL_SUPPORTED(c->time_feat_dim <= 256, "tcl: time_feat_dim %d > 256 not supported", c->time_feat_dim);
    TCL_SUPPORTED(c->num_heads <= 8, "tcl: num_heads %d > 8 not supported", c->num_heads);
    TCL_SUPPORTED(c->node_feat_dim % c->num_heads == 0, "tcl: num_heads %d does not divide node_feat_dim %d", c->num_heads, c->node_feat_dim);
    TCL_SUPPORTED(c->num_layers <= DYGNN_MAX_LAYERS, "tcl: num_layers %d > %d not supported", c->num_layers, DYGNN_MAX_LAYERS);
    return DYGNN_OK;
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Plan {
    size_t x0, y1, qkv, o, z, y, idx, total;      // byte offsets
};
// sides: X0, Y1 [N S d]; Q / K / V planes [3][M S d] and O [M S d] with M = max(N, 2 P); pair sequences: Z, Y [2 P S d]; index [2][2 P] int32
static Plan make_plan(const dygnn_tcl_config& c, int64_t N, int64_t P) {
    const size_t seq = (size_t)(c.num_neighbors + 1) * c.node_feat_dim * sizeof(float);
    const size_t I = 2 * (size_t)P, M = (size_t)N > I ? (size_t)N : I;
    Plan p;
    p.x0 = 0;
    p.y1 = p.x0 + align256((size_t)N * seq);
    p.qkv = p.y1 + align256((size_t)N * seq);
    p.o = p.qkv + align256(3 * M * seq);
    p.z = p.o + align256(M * seq);
    p.y = p.z + align256(I * seq);
    p.idx = p.y + align256(I * seq);
    p.total = p.idx + align256(2 * I * sizeof(int32_t));
    return p;
}

template <int MT>
static int launch_encode(const dygnn_tcl_config& c, const dygnn_tcl_weights& w, const float* node_feat, const float* edge_feat, const int64_t* side_root,
                         const double* side_time, const int64_t* nbr_id, const int64_t* nbr_eid, const float* nbr_t, int64_t N, float* X0, hipStream_t s) {
    int mx = c.node_feat_dim > c.edge_feat_dim ? c.node_feat_dim : c.edge_feat_dim;
    mx = mx > c.time_feat_dim ? mx : c.time_feat_dim;
    const size_t lds = (size_t)16 * MT * (round16(mx) + 4) * sizeof(float);
    if (int rc = lds_limit(k_tcl_encode<MT>, lds)) return rc;
    hipLaunchKernelGGL(k_tcl_encode<MT>, dim3((unsigned)N), dim3(kThreads), lds, s, node_feat, edge_feat, side_root, side_time, nbr_id, nbr_eid, nbr_t, w,
                       c.num_neighbors, c.node_feat_dim, c.edge_feat_dim, c.time_feat_dim, (int64_t)c.num_node_rows, (int64_t)c.num_edge_rows, X0);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

int encode(hipStream_t s, const dygnn_tcl_config& c, const dygnn_tcl_weights& w, const float* node_feat, const float* edge_feat, const int64_t* side_root,
           const double* side_time, const int64_t* nbr_id, const int64_t* nbr_eid, const float* nbr_t, int64_t N, float* X0) {
    const int MT = (c.num_neighbors + 1 + 15) / 16;
    return MT == 1 ? launch_encode<1>(c, w, node_feat, edge_feat, side_root, side_time, nbr_id, nbr_eid, nbr_t, N, X0, s)
         : MT == 2 ? launch_encode<2>(c, w, node_feat, edge_feat, side_root, side_time, nbr_id, nbr_eid, nbr_t, N, X0, s)
         : MT == 3 ? launch_encode<3>(c, w, node_feat, edge_feat, side_root, side_time, nbr_id, nbr_eid, nbr_t, N, X0, s)
                   : launch_encode<4>(c, w, node_feat, edge_feat, side_root, side_time, nbr_id, nbr_eid, nbr_t, N, X0, s);
}

}  // namespace tcl
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::tcl;

extern "C" int dygnn_tcl_check(const dygnn_tcl_config* cfg) { return check_tcl(cfg); }

extern "C" size_t dygnn_tcl_workspace_bytes(const dygnn_tcl_config* cfg, int64_t n_sides, int64_t n_pairs) {
    if (check_tcl(cfg) != DYGNN_OK) return 0;
    if (n_sides < 0 || n_pairs < 0 || n_sides > INT32_MAX || n_pairs > INT32_MAX / 2) {
        set_error("tcl: n_sides and n_pairs must be non-negative (at most 2^31 - 1 sides, 2^30 - 1 pairs)");
        return 0;
    }
    return make_plan(*cfg, n_sides > 0 ? n_sides : 1, n_pairs > 0 ? n_pairs : 1).total;
}

extern "C" int dygnn_tcl_forward(const dygnn_tcl_config* cfg, const dygnn_tcl_weights* w, const float* node_feat, const float* edge_feat,
                                 const int64_t* side_root, const double* side_time, const int64_t* nbr_id, const int64_t* nbr_eid, const float* nbr_t,
                                 int64_t n_sides, const int32_t* pair_a, const int32_t* pair_b, int64_t n_pairs, float* out_a, float* out_b,
                                 const dygnn_tcl_taps* taps, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = check_tcl(cfg)) return rc;
    DYGNN_REQUIRE(n_sides >= 0 && n_sides <= INT32_MAX && n_pairs >= 0 && n_pairs <= INT32_MAX / 2, "tcl: bad n_sides / n_pairs");
    if (n_pairs == 0) return DYGNN_OK;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && w->depth_w && w->proj_node_w && w->proj_node_b && w->proj_edge_w && w->proj_edge_b && w->proj_time_w &&
                  w->proj_time_b && w->output_w && w->output_b, "tcl: null weights");
    for (int l = 0; l < cfg->num_layers; ++l) {
        const dygnn_tcl_layer_weights& m = w->layers[l];
        DYGNN_REQUIRE(m.in_proj_w && m.in_proj_b && m.out_proj_w && m.out_proj_b && m.fc0_w && m.fc0_b && m.fc1_w && m.fc1_b && m.norm0_w && m.norm0_b &&
                      m.norm1_w && m.norm1_b, "tcl: null layer weights (layer %d)", l);
    }
    DYGNN_REQUIRE(node_feat && edge_feat && side_root && side_time && nbr_id && nbr_eid && nbr_t && pair_a && pair_b && out_a && out_b && workspace,
                  "tcl: null pointer");
    const int64_t N = n_sides, P = n_pairs, I = 2 * P;
    for (int64_t p = 0; p < P; ++p)
        DYGNN_REQUIRE(pair_a[p] >= 0 && pair_a[p] < N && pair_b[p] >= 0 && pair_b[p] < N, "tcl: pair %lld names a side outside [0, %lld)", (long long)p,
                      (long long)N);
    const Plan pl = make_plan(*cfg, N, P);
    if (workspace_bytes < pl.total) {
        set_error("tcl: workspace too small (%zu < %zu bytes)", workspace_bytes, pl.total);
        return DYGNN_E_WORKSPACE;
    }
    const int K = cfg->num_neighbors, S = K + 1, d = cfg->node_feat_dim, H = cfg->num_heads, L = cfg->num_layers;
    const float scale = 1.0f / sqrtf((float)(d / H));
    hipStream_t s = as_stream(stream);
    char* base = static_cast<char*>(workspace);
    float* X0 = reinterpret_cast<float*>(base + pl.x0);
    float* Y1 = reinterpret_cast<float*>(base + pl.y1);
    float* QKV = reinterpret_cast<float*>(base + pl.qkv);
    float* O = reinterpret_cast<float*>(base + pl.o);
    float* Z = reinterpret_cast<float*>(base + pl.z);
    float* Y = reinterpret_cast<float*>(base + pl.y);
    int32_t* own = reinterpret_cast<int32_t*>(base + pl.idx);      // side of pair sequence i: (a_p, b_p) interleaved
    int32_t* other = own + I;                                       // side of its partner: (b_p, a_p)
    {
        std::vector<int32_t> idx((size_t)2 * I);
        for (int64_t p = 0; p < P; ++p) {
            idx[2 * p] = pair_a[p]; idx[2 * p + 1] = pair_b[p];
            idx[I + 2 * p] = pair_b[p]; idx[I + 2 * p + 1] = pair_a[p];
        }
        DYGNN_HIP(hipMemcpyAsync(own, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        DYGNN_HIP(hipStreamSynchronize(s));                          // idx is about to go out of scope
    }
    const int64_t tap_rows = taps ? (taps->rows < P ? taps->rows : P) : 0;
    const bool tapping = tap_rows > 0;
    const int64_t sd4 = (int64_t)S * d / 4;

    int rc = encode(s, *cfg, *w, node_feat, edge_feat, side_root, side_time, nbr_id, nbr_eid, nbr_t, N, X0);
    if (rc) return rc;
    if (tapping && taps->encoder_input) {
        hipLaunchKernelGGL(k_tcl_tap, dim3((unsigned)(2 * tap_rows)), dim3(kThreads), 0, s, X0, own, sd4, reinterpret_cast<f4*>(taps->encoder_input));
        DYGNN_LAUNCH_CHECK();
    }
    const size_t lds_rows = (size_t)kRows * (round16(d) + 4) * sizeof(float);
    const size_t lds_post = encoder::post_lds_bytes(4, d);
    const size_t lds_out = (size_t)kOutRows * (round16(d) + 4) * sizeof(float);
    if ((rc = lds_limit(k_tcl_qkv, lds_rows))) return rc;
    if ((rc = lds_limit(k_encoder_post<4, 4>, lds_post))) return rc;

    // one stage: Q / K / V of the n_in input sequences, attention of n_at (query, key) sequence pairs, the rest of the block on their rows
    auto stage = [&](const dygnn_tcl_layer_weights& m, const float* Xin, int64_t n_in, int64_t n_at, const int32_t* q_seq, const int32_t* kv_seq,
                     int kv_xor, const int32_t* mask_side, int nq, float* Xout) -> int {
        const int64_t Rin = n_in * S, R = n_at * nq;
        hipLaunchKernelGGL(k_tcl_qkv, dim3((unsigned)ceil_div(Rin, kRows), 3), dim3(kThreads), lds_rows, s, Xin, Rin, m.in_proj_w, m.in_proj_b, d, QKV);
        DYGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_tcl_attn, dim3((unsigned)n_at), dim3(kThreads), 0, s, QKV, QKV + (size_t)Rin * d, QKV + 2 * (size_t)Rin * d, q_seq, kv_seq,
                           kv_xor, mask_side, side_root, nbr_id, K, nq, d, H, scale, O);
        DYGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_encoder_post<4, 4>), dim3((unsigned)ceil_div(R, kRows)), dim3(kThreads), lds_post, s, O, R, Xin, encoder::ResMap{q_seq, nq, S}, m, d,
                           Xout);
        DYGNN_LAUNCH_CHECK();
        return DYGNN_OK;
    };
    int nq_last = S;
    for (int l = 0; l < L; ++l) {
        const dygnn_tcl_layer_weights& m = w->layers[l];
        const int nq = (l == L - 1 && !tapping) ? 1 : S;          // only position 0 is read after the last layer
        if (l == 0) {
            if ((rc = stage(m, X0, N, N, nullptr, nullptr, 0, nullptr, S, Y1))) return rc;
            if ((rc = stage(m, Y1, N, I, own, other, 0, other, nq, Z))) return rc;
        } else {
            if ((rc = stage(m, Z, I, I, nullptr, nullptr, 0, own, S, Y))) return rc;
            if ((rc = stage(m, Y, I, I, nullptr, nullptr, 1, other, nq, Z))) return rc;
        }
        nq_last = nq;
        if (tapping && taps->layer_out[l])
            DYGNN_HIP(hipMemcpyAsync(taps->layer_out[l], Z, (size_t)tap_rows * 2 * S * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(k_tcl_out, dim3((unsigned)ceil_div(I, kOutRows)), dim3(kThreads), lds_out, s, Z, I, nq_last, w->output_w, w->output_b, d, out_a,
                       out_b);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
