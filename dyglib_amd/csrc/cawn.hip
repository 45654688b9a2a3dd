// CAWN inference forward (models/CAWN.py:48-396, TransformerEncoder models/modules.py:209-266), fp32, gfx950.
//
// A call works on n_sides sides (a target (v, t) with its sampled hop arrays [k], [k^2]) and P pairs of sides.  Pair p makes two SEQUENCES,
// 2 p (side a) and 2 p + 1 (side b); a sequence is the M = k^W walks of its side, encoded with the position features of ITS pair, so a side
// named by several pairs is encoded once per pair.  The tree of a side has T = 1 + k (+ k^2) positions e: 0 the target, 1 .. k hop 1,
// 1 + k .. hop 2; walk j visits e = 0, 1 + j / k^(W-1), 1 + k + j.  No [n][M][W + 1] array exists outside the taps.  Kernels:
//   k_cawn_pos    one pair per workgroup: LDS hash table node id -> appearance counts [2][W + 1] over both trees, the unique ids compacted in
//                 tree order, the position MLP (fp32 MFMA) once per unique id   -> PF [P][2 T][Pd], the counts CT, and every tree position's
//                 row in them, pidx [P][2][T]
//   k_cawn_lstm   64 rows x 64 hidden units (all four gates) per workgroup: gathers the input rows [node | cos | edge | position feature]
//                 128 columns at a time into LDS, x W_ih^T and (steps >= 1) h_prev W_hh^T as fp32 MFMAs into the same accumulators, then the cell.
//                 Launched per row set: step 0 once per SEQUENCE (the walks of a sequence share position 0), step h once per hop-h tree node
//                 (a padded node carries its parent's state on), and the reverse direction as ONE cell from the zero state on each walk's
//                 last valid position (that is the reverse LSTM's output there).  The last forward step and the reverse cell write the
//                 encoder output [rows][2 H] directly.
//   k_cawn_proj   64 walk rows per workgroup: [feature encoder out | position encoder out] x projection_layers[0]     -> X, and in_proj -> Q, K, V
//   k_cawn_attn / k_encoder_post<NT, MT> (encoder_block.h, shared with tcl.hip)   the rest of the TransformerEncoder over the M walks of a
//                 sequence, no mask: attention with M <= 128 keys and one head of Q, K, V in LDS at stride 65; the block tail with the width
//                 taken past 256 columns (<4, 4>, <5, 2>, <8, 2>: NT column tiles per wave, 16 MT rows per workgroup), identity residual map -> Y
//   k_cawn_out    4 sequences per workgroup: mean over the walks, projection_layers[1]                                  -> out_a, out_b
// The K axis of every product that gathers its rows goes through LDS 128 columns at a time, so four workgroups share a CU.
#include <vector>

#include "common.h"
#include "encoder_block.h"
#include "mfma_tile.h"
#include "time_encoding.h"

namespace dygnn {
namespace cawn {

using timeenc::cos_time;
using encoder::k_encoder_post;
using tile::f4;
using tile::kThreads;
using tile::kWaves;
using tile::lds_limit;
using tile::mfma4;
using tile::round16;
using tile::wave_product;
using tile::z4;

constexpr int kMaxWalks = 128;      // M = k^W: two keys per lane in k_cawn_attn
constexpr int kMaxTree = 136;       // T <= 1 + 128 (W = 1) or 1 + 11 + 121 (W = 2)
constexpr int kSlots = 1024;        // hash slots of a pair: <= 2 T = 272 keys
constexpr int kRows = 64;
constexpr int kMaxHead = 64;        // attention_dim / heads: one output column per lane
constexpr int kKChunk = 128;        // input columns of k_cawn_lstm / k_cawn_proj in LDS at a time: 33 KiB tiles, four workgroups per CU
constexpr int kOutSeqs = 4;         // sequences per workgroup of k_cawn_out (rows 4 .. 15 of its MFMA tile are zero)
constexpr unsigned long long kEmpty = ~0ull;

struct Tree {                       // the hop arrays of all sides, as the sampler returns them (hop 2 NULL when W = 1)
    const int64_t *id1, *id2, *eid1, *eid2;
    const float *t1, *t2;
};

struct Dims {
    int Fn, Fe, Ft, Pd, W, k, M, T, D, Hf, Hp, A, heads;
};

static Dims dims_of(const dygnn_cawn_config& c) {
    Dims d;
    d.Fn = c.node_feat_dim, d.Fe = c.edge_feat_dim, d.Ft = c.time_feat_dim, d.Pd = c.position_feat_dim;
    d.W = c.walk_length, d.k = c.num_neighbors, d.heads = c.num_walk_heads;
    d.M = d.W == 1 ? d.k : d.k * d.k;
    d.T = 1 + d.k + (d.W == 2 ? d.k * d.k : 0);
    d.D = d.Fn + d.Fe + d.Ft + d.Pd;
    d.Hf = d.D / 2, d.Hp = d.Pd / 2;
    d.A = d.D / 2;                                                  // models/CAWN.py:307-313
    if (d.A % d.heads != 0) d.A += d.heads - d.A % d.heads;
    return d;
}

__device__ __forceinline__ int64_t tree_id(const Tree& tr, const int64_t* __restrict__ side_root, int64_t s, int e, int k, int M) {
    const int64_t id = e == 0 ? side_root[s] : e <= k ? tr.id1[s * k + e - 1] : tr.id2[s * M + e - 1 - k];
    return id < 0 ? 0 : id;
}

__device__ __forceinline__ f4 load_w4(const float* __restrict__ p, int k, int Kdim, bool aligned) {
    if (aligned) return k < Kdim ? *reinterpret_cast<const f4*>(p + k) : z4();
    f4 w = z4();
    if (k < Kdim) w.x = p[k];
    if (k + 1 < Kdim) w.y = p[k + 1];
    if (k + 2 < Kdim) w.z = p[k + 2];
    if (k + 3 < Kdim) w.w = p[k + 3];
    return w;
}

// tile::wave_product for weight rows that need not be 16-byte aligned (ldw or Kdim no multiple of 4: position_feat_dim = 2 mod 4)
template <int NT, int MT>
__device__ __forceinline__ void wave_product_any(const float* __restrict__ A, int lda, const float* __restrict__ Wm, int ldw, int N, int Kdim, bool aligned,
                                                 int wave, int lane, f4 (&acc)[NT][MT]) {
    const int c = lane & 15, g = lane >> 4;
    for (int k0 = 0; k0 < Kdim; k0 += 16) {
        const int k = k0 + 4 * g;
        f4 a[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a[mt] = *reinterpret_cast<const f4*>(A + (size_t)(16 * mt + c) * lda + k);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n0 = 16 * (wave + kWaves * t);
            if (n0 >= N) continue;                                   // wave-uniform
            const int n = n0 + c;
            const f4 w = n < N ? load_w4(Wm + (size_t)n * ldw, k, Kdim, aligned) : z4();
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[t][mt] = mfma4(w.x, a[mt].x, acc[t][mt]);
                acc[t][mt] = mfma4(w.y, a[mt].y, acc[t][mt]);
                acc[t][mt] = mfma4(w.z, a[mt].z, acc[t][mt]);
                acc[t][mt] = mfma4(w.w, a[mt].w, acc[t][mt]);
            }
        }
    }
}

// ---- position counts and position features of a pair (models/CAWN.py:197-289) -------------------------------------------------------------------
// Dynamic LDS: keys [kSlots] u64 | counts [kSlots][2][3] int | first tree position [kSlots] | compact index [kSlots] | slot of every tree
// position [2 T] | slot of every unique id [2 T] | count values [2 T][2][3] float | MLP tile [64][round16(Pd) + 4].
// Counts are integers; the value is count / k^hop (the reference adds 1 / k^hop in float32: within k^hop 2^-24 of it).
static size_t pos_lds_bytes(int Pd) {
    return (size_t)kSlots * 8 + (size_t)kSlots * 6 * 4 + (size_t)kSlots * 4 * 2 + (size_t)2 * kMaxTree * 4 * 2 + (size_t)2 * kMaxTree * 6 * 4 +
           (size_t)kRows * (round16(Pd) + 4) * 4;
}

__global__ __launch_bounds__(kThreads) void k_cawn_pos(const int64_t* __restrict__ side_root, Tree tr, const int32_t* __restrict__ own,
                                                         const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, int k, int W, int M, int T, int Pd, int32_t* __restrict__ pidx,
                                                         float* __restrict__ CT, float* __restrict__ PF) {
    extern __shared__ __attribute__((aligned(16))) unsigned char raw[];
    unsigned long long* s_key = reinterpret_cast<unsigned long long*>(raw);
    int* s_cnt = reinterpret_cast<int*>(s_key + kSlots);
    int* s_rep = s_cnt + kSlots * 6;
    int* s_u = s_rep + kSlots;
    int* s_slot = s_u + kSlots;
    int* s_ulist = s_slot + 2 * kMaxTree;
    float* s_cv = reinterpret_cast<float*>(s_ulist + 2 * kMaxTree);
    float* A = s_cv + 2 * kMaxTree * 6;
    __shared__ int s_U;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = blockIdx.x;
    const int T2 = 2 * T, W1 = W + 1;
    for (int i = threadIdx.x; i < kSlots; i += kThreads) {
        s_key[i] = kEmpty;
        s_rep[i] = T2;
#pragma unroll
        for (int x = 0; x < 6; ++x) s_cnt[i * 6 + x] = 0;
    }
    __syncthreads();
    for (int e2 = threadIdx.x; e2 < T2; e2 += kThreads) {
        const int sel = e2 >= T, e = e2 - sel * T;
        const unsigned long long id = (unsigned long long)tree_id(tr, side_root, own[2 * p + sel], e, k, M);
        const int hop = e == 0 ? 0 : e <= k ? 1 : 2;
        int slot = (int)((id * 0x9E3779B97F4A7C15ull) >> 54);         // 10 bits
        for (;;) {                                                      // <= 272 keys in 1024 slots: a free slot exists
            const unsigned long long prev = atomicCAS(&s_key[slot], kEmpty, id);
            if (prev == kEmpty || prev == id) break;
            slot = (slot + 1) & (kSlots - 1);
        }
        atomicAdd(&s_cnt[slot * 6 + sel * 3 + hop], 1);
        atomicMin(&s_rep[slot], e2);
        s_slot[e2] = slot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                             // unique ids in the order of their first tree position
        int U = 0;
        for (int e2 = 0; e2 < T2; ++e2) {
            const int slot = s_slot[e2];
            if (s_rep[slot] == e2) {
                s_u[slot] = U;
                s_ulist[U++] = slot;
            }
        }
        s_U = U;
    }
    __syncthreads();
    const int U = s_U;
    for (int e2 = threadIdx.x; e2 < T2; e2 += kThreads) pidx[p * T2 + e2] = s_u[s_slot[e2]];
    for (int i = threadIdx.x; i < U * 6; i += kThreads) {
        const int u = i / 6, x = i - u * 6, hop = x % 3;
        const int slot = s_ulist[u];
        const float n = hop == 0 ? 1.f : hop == 1 ? (float)k : (float)(k * k);
        const float v = s_key[slot] == 0ull ? 0.f : (float)s_cnt[slot * 6 + x] / n;      // the padded node's entry is set to zero (:255)
        s_cv[i] = v;
        if (hop < W1) CT[((size_t)p * T2 + u) * 2 * W1 + (x / 3) * W1 + hop] = v;
    }
    const int Kp = round16(Pd), lda = Kp + 4;
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    for (int u0 = 0; u0 < U; u0 += kRows) {
        f4 acc[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) acc[t][mt] = z4();
        for (int sel = 0; sel < 2; ++sel) {
            __syncthreads();                                            // s_cv written / the previous product has read A
            for (int i = threadIdx.x; i < kRows * Kp; i += kThreads) {
                const int r = i / Kp, f = i - r * Kp;
                float v = 0.f;
                if (u0 + r < U && f < Pd) {
                    v = b0[f];
                    for (int h = 0; h < W1; ++h) v = fmaf(s_cv[(u0 + r) * 6 + sel * 3 + h], w0[f * W1 + h], v);
                    v = fmaxf(v, 0.f);
                }
                A[r * lda + f] = v;
            }
            __syncthreads();
            wave_product_any<4, 4>(A, lda, w1, Pd, Pd, Pd, (Pd & 3) == 0, wave, lane, acc);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int n = 16 * (wave + kWaves * t) + g4;
            if (n >= Pd) continue;
            const f4 b = load_w4(b1, n, Pd, (Pd & 3) == 0);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int u = u0 + 16 * mt + c;
                if (u >= U) continue;
                float* dst = PF + ((size_t)p * T2 + u) * Pd + n;
                const f4 v = (acc[t][mt] + b) + b;                   // both rows carry the bias
                if ((Pd & 3) == 0) *reinterpret_cast<f4*>(dst) = v;
                else {                                               // rows of 2 mod 4 floats: 8-byte aligned, the last quad holds two
                    dst[0] = v.x, dst[1] = v.y;
                    if (n + 2 < Pd) dst[2] = v.z, dst[3] = v.w;
                }
            }
        }
    }
}

// taps: walk ids [rows][2][M][W + 1] and their counts [rows][2][M][W + 1][2][W + 1]
__global__ void k_cawn_tap_walks(const int64_t* __restrict__ side_root, Tree tr, const int32_t* __restrict__ own, const int32_t* __restrict__ pidx,
                                 const float* __restrict__ CT, int k, int W, int M, int T, int64_t n, int64_t* __restrict__ ids,
                                 float* __restrict__ counts) {
    const int W1 = W + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int pos = (int)(i % W1);
        const int j = (int)((i / W1) % M);
        const int64_t q = i / W1 / M;
        const int e = pos == 0 ? 0 : (pos == 1 ? 1 + (W == 1 ? j : j / k) : 1 + k + j);
        const int64_t p = q >> 1;
        if (ids) ids[i] = tree_id(tr, side_root, own[q], e, k, M);
        if (counts) {
            const float* src = CT + ((size_t)p * 2 * T + pidx[p * 2 * T + (q & 1) * T + e]) * 2 * W1;
            for (int x = 0; x < 2 * W1; ++x) counts[i * 2 * W1 + x] = src[x];
        }
    }
}

// ---- one LSTM step of a row set (models/CAWN.py:358-396) -----------------------------------------------------------------------------------------
struct LstmArgs {
    const float *node_feat, *edge_feat;
    const int64_t* side_root;
    const double* side_time;
    Tree tr;
    const int32_t *own, *pidx;
    const float *PF, *time_w, *time_b;
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    const float *h_prev, *c_prev;      // [rows / k][H] (mode 1), NULL = the zero state
    float* h_out;                      // row r at h_out + r ld_out + col_out
    float* c_out;                      // [rows][H] or NULL
    int64_t rows, node_rows, edge_rows;
    int ld_out, col_out;
    int mode;                          // 0: position 0 of every sequence; 1: the nodes of hop `hop`; 2: the last valid position of every walk
    int hop, n_hop;                    // mode 1: n_hop = k^hop nodes per sequence
    int pos_only;                      // the position encoder: the input row is the position feature alone
    int Fn, Fe, Ft, Pd, k, W, M, T, H;
};

// acc[gate][mt] += W[gate H + u0 + 16 wave + ., wk0 : wk0 + Kdim] . A[16 mt + ., 0 : Kdim]^T: the wave's 16 hidden units in all four gates.
// A: LDS rows of stride lda, zero beyond Kdim up to round16(Kdim).  aligned: ldw, wk0 and Kdim are multiples of 4.
__device__ __forceinline__ void gate_product(const float* __restrict__ A, int lda, const float* __restrict__ Wm, int ldw, int wk0, int H, int u0, int Kdim,
                                             bool aligned, int wave, int lane, f4 (&acc)[4][4]) {
    const int c = lane & 15, g = lane >> 4;
    if (u0 + 16 * wave >= H) return;                                 // wave-uniform
    const int u = u0 + 16 * wave + c;
    for (int k0 = 0; k0 < Kdim; k0 += 16) {
        const int kk = k0 + 4 * g;
        f4 a[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) a[mt] = *reinterpret_cast<const f4*>(A + (size_t)(16 * mt + c) * lda + kk);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const f4 w = u < H ? load_w4(Wm + ((size_t)t * H + u) * ldw + wk0, kk, Kdim, aligned) : z4();
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                acc[t][mt] = mfma4(w.x, a[mt].x, acc[t][mt]);
                acc[t][mt] = mfma4(w.y, a[mt].y, acc[t][mt]);
                acc[t][mt] = mfma4(w.z, a[mt].z, acc[t][mt]);
                acc[t][mt] = mfma4(w.w, a[mt].w, acc[t][mt]);
            }
        }
    }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// grid (row tiles of 64, unit tiles of 64).  LDS: A [64][kKChunk + 4], the K axis kKChunk columns at a time
__global__ __launch_bounds__(kThreads) void k_cawn_lstm(LstmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float A[];
    __shared__ int64_t s_id[kRows], s_eid[kRows], s_par[kRows];
    __shared__ const float* s_pf[kRows];
    __shared__ float s_dt[kRows];
    __shared__ int s_valid[kRows], s_live[kRows];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    const int u0 = blockIdx.y * kRows;
    const int H = a.H, k = a.k, M = a.M, T = a.T;
    int valid = 0;
    if (threadIdx.x < kRows) {
        const int64_t r = r0 + threadIdx.x;
        int live = 0;
        int64_t id = 0, eid = 0, par = 0;
        float dt = 0.f;
        const float* pf = nullptr;
        if (r < a.rows) {
            live = 1;
            int64_t q;
            int e;
            if (a.mode == 0) {
                q = r, e = 0;
            } else if (a.mode == 1) {
                q = r / a.n_hop;
                e = (a.hop == 1 ? 1 : 1 + k) + (int)(r - q * a.n_hop);
                par = r / k;
            } else {
                q = r / M;
                const int j = (int)(r - q * M);
                const int64_t s = a.own[q];
                if (a.W == 1) e = a.tr.id1[s * k + j] != 0 ? 1 + j : 0;
                else e = a.tr.id2[s * M + j] != 0 ? 1 + k + j : a.tr.id1[s * k + j / k] != 0 ? 1 + j / k : 0;
            }
            const int64_t s = a.own[q];
            id = tree_id(a.tr, a.side_root, s, e, k, M);
            valid = a.mode != 1 || id != 0;
            if (e > 0) {
                eid = e <= k ? a.tr.eid1[s * k + e - 1] : a.tr.eid2[s * M + e - 1 - k];
                const float tn = e <= k ? a.tr.t1[s * k + e - 1] : a.tr.t2[s * M + e - 1 - k];
                dt = (float)(a.side_time[s] - (double)tn);              // f64 - f32 -> f64 -> .float()
            }
            const int64_t p = q >> 1;
            pf = a.PF + ((size_t)p * 2 * T + a.pidx[p * 2 * T + (q & 1) * T + e]) * a.Pd;
        }
        s_id[threadIdx.x] = id >= a.node_rows ? 0 : id;
        s_eid[threadIdx.x] = (eid < 0 || eid >= a.edge_rows) ? 0 : eid;
        s_par[threadIdx.x] = par;
        s_pf[threadIdx.x] = pf;
        s_dt[threadIdx.x] = dt;
        s_valid[threadIdx.x] = valid;
        s_live[threadIdx.x] = live;
    }
    const int any = __syncthreads_or(valid);                         // a tile of padded nodes only carries the state on
    f4 acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[t][mt] = z4();
    constexpr int lda = kKChunk + 4;
    if (any) {
        const int ldx = a.pos_only ? a.Pd : a.Fn + a.Ft + a.Fe + a.Pd;
        // segments of the product's K axis: models/CAWN.py:342 [node | time | edge | position], then the parent's hidden state
        for (int seg = a.pos_only ? 3 : 0; seg < (a.h_prev ? 5 : 4); ++seg) {
            const int dim = seg == 0 ? a.Fn : seg == 1 ? a.Ft : seg == 2 ? a.Fe : seg == 3 ? a.Pd : H;
            const int off = (a.pos_only || seg == 0 || seg == 4) ? 0 : seg == 1 ? a.Fn : seg == 2 ? a.Fn + a.Ft : a.Fn + a.Ft + a.Fe;
            for (int c0 = 0; c0 < dim; c0 += kKChunk) {
                const int cn = dim - c0 < kKChunk ? dim - c0 : kKChunk, Kp = round16(cn), K4 = Kp >> 2;
                __syncthreads();                                     // the previous product has read A
                if (seg < 4) {
                    for (int i = threadIdx.x; i < kRows * K4; i += kThreads) {
                        const int j = i / K4, f = 4 * (i - j * K4), col = c0 + f;
                        f4 v = z4();
                        if (s_valid[j] && f < cn) {
                            if (seg == 0) v = *reinterpret_cast<const f4*>(a.node_feat + (size_t)s_id[j] * a.Fn + col);
                            else if (seg == 2) v = *reinterpret_cast<const f4*>(a.edge_feat + (size_t)s_eid[j] * a.Fe + col);
                            else if (seg == 3) v = load_w4(s_pf[j], col, a.Pd, (a.Pd & 3) == 0);
                            else {
                                const float dt = s_dt[j];
                                v.x = cos_time(fmaf(dt, a.time_w[col], a.time_b[col]));
                                v.y = cos_time(fmaf(dt, a.time_w[col + 1], a.time_b[col + 1]));
                                v.z = cos_time(fmaf(dt, a.time_w[col + 2], a.time_b[col + 2]));
                                v.w = cos_time(fmaf(dt, a.time_w[col + 3], a.time_b[col + 3]));
                            }
                        }
                        *reinterpret_cast<f4*>(A + j * lda + f) = v;
                    }
                } else {
                    for (int i = threadIdx.x; i < kRows * Kp; i += kThreads) {
                        const int j = i / Kp, f = i - j * Kp;
                        A[j * lda + f] = (s_valid[j] && f < cn) ? a.h_prev[(size_t)s_par[j] * H + c0 + f] : 0.f;
                    }
                }
                __syncthreads();
                if (seg < 4) gate_product(A, lda, a.w_ih, ldx, off + c0, H, u0, cn, (ldx & 3) == 0, wave, lane, acc);
                else gate_product(A, lda, a.w_hh, H, c0, H, u0, cn, (H & 3) == 0, wave, lane, acc);
            }
        }
    }
    const int c = lane & 15, ub = u0 + 16 * wave + 4 * (lane >> 4);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const int j = 16 * mt + c;
        if (!s_live[j]) continue;
        const int64_t r = r0 + j;
        const bool on = s_valid[j] != 0;
        const size_t par = (size_t)s_par[j] * H;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int u = ub + v;
            if (u >= H) continue;
            const float cp = a.c_prev ? a.c_prev[par + u] : 0.f;
            float h, cn;
            if (on) {
                const float gi = acc[0][mt][v] + (a.b_ih[u] + a.b_hh[u]);
                const float gf = acc[1][mt][v] + (a.b_ih[H + u] + a.b_hh[H + u]);
                const float gg = acc[2][mt][v] + (a.b_ih[2 * H + u] + a.b_hh[2 * H + u]);
                const float go = acc[3][mt][v] + (a.b_ih[3 * H + u] + a.b_hh[3 * H + u]);
                cn = fmaf(sigmoidf_(gf), cp, sigmoidf_(gi) * tanhf(gg));
                h = sigmoidf_(go) * tanhf(cn);
            } else {                                                 // a padded node: the walk ended before it
                cn = cp;
                h = a.h_prev[par + u];
            }
            a.h_out[(size_t)r * a.ld_out + a.col_out + u] = h;
            if (a.c_out) a.c_out[(size_t)r * H + u] = cn;
        }
    }
}

// ---- projection_layers[0] on [feature encoder output | position encoder output] (models/CAWN.py:348-350) ------------------------------------------
// and, with EP = NULL and grid.y = 3, in_proj: plane y = X in_proj_weight[y d : (y + 1) d]^T + in_proj_bias[y d : (y + 1) d] -> out + y R d.
// LDS: A [64][kKChunk + 4], the input columns kKChunk at a time
template <int NT>
__global__ __launch_bounds__(kThreads) void k_cawn_proj(const float* __restrict__ EF, int wf, const float* __restrict__ EP, int wp, int64_t R,
                                                          const float* __restrict__ Wm, const float* __restrict__ bias, int d, float* __restrict__ X) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lda = kKChunk + 4, Kt = wf + wp, y = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * kRows;
    Wm += (size_t)y * d * Kt, bias += (size_t)y * d, X += (size_t)y * R * d;
    f4 acc[NT][4];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) acc[t][mt] = z4();
    for (int kc = 0; kc < Kt; kc += kKChunk) {
        const int kn = Kt - kc < kKChunk ? Kt - kc : kKChunk, Kp = round16(kn);
        __syncthreads();
        for (int i = threadIdx.x; i < kRows * Kp; i += kThreads) {
            const int r = i / Kp, f = i - r * Kp, col = kc + f;
            float v = 0.f;
            if (r0 + r < R && f < kn) v = col < wf ? EF[(size_t)(r0 + r) * wf + col] : EP[(size_t)(r0 + r) * wp + col - wf];
            smem[r * lda + f] = v;
        }
        __syncthreads();
        wave_product<NT, 4>(smem, lda, Wm, Kt, kc, d, kn, wave, lane, acc);
    }
    const int c = lane & 15, g4 = 4 * (lane >> 4);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = 16 * (wave + kWaves * t) + g4;
        if (n >= d) continue;
        const f4 b = *reinterpret_cast<const f4*>(bias + n);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            const int64_t r = r0 + 16 * mt + c;
            if (r < R) *reinterpret_cast<f4*>(X + (size_t)r * d + n) = acc[t][mt] + b;
        }
    }
}

// ---- self-attention over the M walks of one sequence, no mask (models/CAWN.py:352) ----------------------------------------------------------------------
// Head by head: Q, K, V of the head in LDS at stride 65; wave w owns the query rows w, w + 4, ...; lane l scores the keys l and l + 64, the
// wave does the softmax, then lane l sums head column l over the keys (the probabilities broadcast lane by lane).  LDS: 3 [M][65].
__global__ __launch_bounds__(kThreads) void k_cawn_attn(const float* __restrict__ Q, const float* __restrict__ Kp, const float* __restrict__ V, int M, int d,
                                                          int Hn, float scale, float* __restrict__ O) {
    constexpr int LD = kMaxHead + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ks = Qs + M * LD;
    float* Vs = Ks + M * LD;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dh = d / Hn;
    const size_t base = (size_t)blockIdx.x * M * d;
    const bool on0 = lane < M, on1 = lane + 64 < M;
    for (int h = 0; h < Hn; ++h) {
        __syncthreads();                                             // the previous head has been read
        for (int x = threadIdx.x; x < M * dh; x += kThreads) {
            const int r = x / dh, cc = x - r * dh;
            const size_t g = base + (size_t)r * d + h * dh + cc;
            Qs[r * LD + cc] = Q[g];
            Ks[r * LD + cc] = Kp[g];
            Vs[r * LD + cc] = V[g];
        }
        __syncthreads();
        for (int r = wave; r < M; r += kWaves) {
            float s0 = 0.f, s1 = 0.f;
            const float* k0 = Ks + (on0 ? lane : 0) * LD;
            const float* k1 = Ks + (on1 ? lane + 64 : 0) * LD;
            if (M > 64) {
#pragma unroll 4
                for (int cc = 0; cc < dh; ++cc) {
                    const float qv = Qs[r * LD + cc];
                    s0 = fmaf(qv, k0[cc], s0);
                    s1 = fmaf(qv, k1[cc], s1);
                }
            } else {
#pragma unroll 8
                for (int cc = 0; cc < dh; ++cc) s0 = fmaf(Qs[r * LD + cc], k0[cc], s0);
            }
            s0 = on0 ? s0 * scale : -INFINITY;
            s1 = on1 ? s1 * scale : -INFINITY;
            const float m = wave_max(fmaxf(s0, s1));
            const float e0 = on0 ? expf(s0 - m) : 0.f, e1 = on1 ? expf(s1 - m) : 0.f;
            const float sum = wave_sum(e0 + e1);
            const float p0 = e0 / sum, p1 = e1 / sum;
            const int col = lane < dh ? lane : 0;
            float o = 0.f;
            const int n0 = M < 64 ? M : 64;
            for (int j = 0; j < n0; ++j) o = fmaf(__shfl(p0, j), Vs[j * LD + col], o);
            for (int j = 64; j < M; ++j) o = fmaf(__shfl(p1, j - 64), Vs[j * LD + col], o);
            if (lane < dh) O[base + (size_t)r * d + h * dh + lane] = o;
        }
    }
}

// ---- mean over the walks, projection_layers[1] (models/CAWN.py:352-354) ------------------------------------------------------------------------------
// Y [n][M][d]; sequence 2 p -> out_a[p], 2 p + 1 -> out_b[p].  kOutSeqs sequences per workgroup.  LDS: [16][round16(d) + 4]
__global__ __launch_bounds__(kThreads) void k_cawn_out(const float* __restrict__ Y, int64_t n, int M, const float* __restrict__ Wm,
                                                         const float* __restrict__ bias, int d, int Fn, float* __restrict__ out_a, float* __restrict__ out_b) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Kp = round16(d), lda = Kp + 4;
    const int64_t q0 = (int64_t)blockIdx.x * kOutSeqs;
    for (int i = threadIdx.x; i < 16 * Kp; i += kThreads) {
        const int r = i / Kp, f = i - r * Kp;
        float v = 0.f;
        if (r < kOutSeqs && q0 + r < n && f < d) {
            const float* y = Y + (size_t)(q0 + r) * M * d + f;
            for (int j = 0; j < M; ++j) v += y[(size_t)j * d];
            v /= (float)M;
        }
        smem[r * lda + f] = v;
    }
    __syncthreads();
    f4 acc[4][1];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t][0] = z4();
    wave_product<4, 1>(smem, lda, Wm, d, 0, Fn, d, wave, lane, acc);
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    const int64_t q = q0 + c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int nn = 16 * (wave + kWaves * t) + g4;
        if (nn >= Fn || c >= kOutSeqs || q >= n) continue;
        float* o = ((q & 1) ? out_b : out_a) + (size_t)(q >> 1) * Fn + nn;
        *reinterpret_cast<f4*>(o) = acc[t][0] + *reinterpret_cast<const f4*>(bias + nn);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
#define CAWN_SUPPORTED(cond, ...)                                 \
    do {                                                          \
        if (!(cond)) {                                            \
            set_error(__VA_ARGS__);                               \
            return DYGNN_E_UNSUPPORTED;                           \
        }                                                         \
    } while (0)

static int check_cawn(const dygnn_cawn_config* c) {
    DYGNN_REQUIRE(c != nullptr, "cawn: config is NULL");
    DYGNN_REQUIRE(c->num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!");      // utils/utils.py:157
    DYGNN_REQUIRE(c->walk_length > 0, "Number of sampled hops should be greater than 0!");                            // utils/utils.py:228
    DYGNN_REQUIRE(c->node_feat_dim > 0 && c->edge_feat_dim > 0 && c->time_feat_dim > 0 && c->position_feat_dim > 0, "cawn: feature dims must be positive");
    DYGNN_REQUIRE(c->num_walk_heads >= 1, "cawn: num_walk_heads must be at least 1");
    DYGNN_REQUIRE(c->num_node_rows >= 1 && c->num_edge_rows >= 1, "cawn: num_node_rows and num_edge_rows must be at least 1");
    CAWN_SUPPORTED(c->walk_length <= 2, "cawn: walk_length %d not supported (1..2)", c->walk_length);
    const long long M = c->walk_length == 1 ? c->num_neighbors : (long long)c->num_neighbors * c->num_neighbors;
    CAWN_SUPPORTED(M <= kMaxWalks, "cawn: %lld walks (num_neighbors %d ** walk_length %d) > %d not supported", M, c->num_neighbors, c->walk_length, kMaxWalks);
    CAWN_SUPPORTED(c->node_feat_dim % 4 == 0 && c->edge_feat_dim % 4 == 0 && c->time_feat_dim % 4 == 0,
                   "cawn: node_feat_dim, edge_feat_dim and time_feat_dim must be multiples of 4 (%d, %d, %d)", c->node_feat_dim, c->edge_feat_dim,
                   c->time_feat_dim);
    CAWN_SUPPORTED(c->position_feat_dim % 2 == 0, "cawn: position_feat_dim %d is odd (and so is the walk input dim): not supported", c->position_feat_dim);
    CAWN_SUPPORTED(c->node_feat_dim <= 256, "cawn: node_feat_dim %d > 256 not supported", c->node_feat_dim);
    CAWN_SUPPORTED(c->edge_feat_dim <= 256, "cawn: edge_feat_dim %d > 256 not supported", c->edge_feat_dim);
    CAWN_SUPPORTED(c->time_feat_dim <= 256, "cawn: time_feat_dim %d > 256 not supported", c->time_feat_dim);
    CAWN_SUPPORTED(c->position_feat_dim <= 256, "cawn: position_feat_dim %d > 256 not supported", c->position_feat_dim);
    const Dims d = dims_of(*c);
    CAWN_SUPPORTED(d.A % 4 == 0, "cawn: attention_dim %d (input dim %d // 2 rounded up to num_walk_heads %d) is not a multiple of 4", d.A, d.D, d.heads);
    CAWN_SUPPORTED(d.A <= 512, "cawn: attention_dim %d (input dim %d // 2 rounded up to num_walk_heads %d) > 512 not supported", d.A, d.D, d.heads);
    CAWN_SUPPORTED(d.A / d.heads <= kMaxHead, "cawn: head size %d (attention_dim %d / num_walk_heads %d) > %d not supported", d.A / d.heads, d.A, d.heads,
                   kMaxHead);
    return DYGNN_OK;
}

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
struct Plan {
    size_t own, pidx, ct, pf, h0[2], c0[2], h1[2], c1[2], enc[2], x, qkv, o, y, total;      // byte offsets; [0] feature, [1] position encoder
};
static Plan make_plan(const Dims& d, int64_t P) {
    const size_t I = 2 * (size_t)P, R = I * d.M, f = sizeof(float);
    Plan p;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    p.own = take(I * sizeof(int32_t));
    p.pidx = take((size_t)P * 2 * d.T * sizeof(int32_t));
    p.ct = take((size_t)P * 2 * d.T * 2 * (d.W + 1) * f);
    p.pf = take((size_t)P * 2 * d.T * d.Pd * f);
    for (int e = 0; e < 2; ++e) {
        const size_t H = e == 0 ? d.Hf : d.Hp;
        p.h0[e] = take(I * H * f);
        p.c0[e] = take(I * H * f);
        p.h1[e] = take(d.W == 2 ? I * d.k * H * f : 0);
        p.c1[e] = take(d.W == 2 ? I * d.k * H * f : 0);
        p.enc[e] = take(R * 2 * H * f);
    }
    p.x = take(R * d.A * f);
    p.qkv = take(3 * R * d.A * f);
    p.o = take(R * d.A * f);
    p.y = take(R * d.A * f);
    p.total = at;
    return p;
}

static int launch_lstm(hipStream_t s, const LstmArgs& a) {
    const size_t lds = (size_t)kRows * (kKChunk + 4) * sizeof(float);
    if (int rc = lds_limit(k_cawn_lstm, lds)) return rc;
    hipLaunchKernelGGL(k_cawn_lstm, dim3((unsigned)ceil_div(a.rows, kRows), (unsigned)ceil_div(a.H, kRows)), dim3(kThreads), lds, s, a);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

template <int NT, int MT>
static int transformer(hipStream_t s, const Dims& d, const dygnn_cawn_weights& w, const float* EF, const float* EP, int64_t R, float* X, float* QKV, float* O,
                       float* Y) {
    const int A = d.A;
    const size_t lds_proj = (size_t)kRows * (kKChunk + 4) * sizeof(float);
    const size_t lds_post = encoder::post_lds_bytes(MT, A);
    const size_t lds_attn = (size_t)3 * d.M * (kMaxHead + 1) * sizeof(float);
    int rc;
    if ((rc = lds_limit(k_cawn_proj<NT>, lds_proj))) return rc;
    if ((rc = lds_limit(k_encoder_post<NT, MT>, lds_post))) return rc;
    if ((rc = lds_limit(k_cawn_attn, lds_attn))) return rc;
    const unsigned tiles = (unsigned)ceil_div(R, kRows);
    hipLaunchKernelGGL(k_cawn_proj<NT>, dim3(tiles), dim3(kThreads), lds_proj, s, EF, 2 * d.Hf, EP, 2 * d.Hp, R, w.proj0_w, w.proj0_b, A, X);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cawn_proj<NT>, dim3(tiles, 3), dim3(kThreads), lds_proj, s, X, A, (const float*)nullptr, 0, R, w.attn.in_proj_w, w.attn.in_proj_b, A, QKV);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cawn_attn, dim3((unsigned)(R / d.M)), dim3(kThreads), lds_attn, s, QKV, QKV + (size_t)R * A, QKV + 2 * (size_t)R * A, d.M, A, d.heads,
                       1.0f / sqrtf((float)(A / d.heads)), O);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL((k_encoder_post<NT, MT>), dim3((unsigned)ceil_div(R, 16 * MT)), dim3(kThreads), lds_post, s, O, R, X, encoder::ResMap{nullptr, d.M, d.M}, w.attn, A,
                       Y);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace cawn
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::cawn;

extern "C" int dygnn_cawn_check(const dygnn_cawn_config* cfg) { return check_cawn(cfg); }

extern "C" size_t dygnn_cawn_workspace_bytes(const dygnn_cawn_config* cfg, int64_t n_sides, int64_t n_pairs) {
    if (check_cawn(cfg) != DYGNN_OK) return 0;
    if (n_sides < 0 || n_pairs < 0 || n_sides > INT32_MAX || n_pairs > (1 << 20)) {
        set_error("cawn: n_sides and n_pairs must be non-negative (at most 2^31 - 1 sides, 2^20 pairs)");
        return 0;
    }
    return make_plan(dims_of(*cfg), n_pairs > 0 ? n_pairs : 1).total;
}

extern "C" int dygnn_cawn_forward(const dygnn_cawn_config* cfg, const dygnn_cawn_weights* w, const float* node_feat, const float* edge_feat,
                                  const int64_t* side_root, const double* side_time, const dygnn_cawn_hops* hops, int64_t n_sides, const int32_t* pair_a,
                                  const int32_t* pair_b, int64_t n_pairs, float* out_a, float* out_b, const dygnn_cawn_taps* taps, void* workspace,
                                  size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = check_cawn(cfg)) return rc;
    DYGNN_REQUIRE(n_sides >= 0 && n_sides <= INT32_MAX && n_pairs >= 0 && n_pairs <= (1 << 20), "cawn: bad n_sides / n_pairs");
    if (n_pairs == 0) return DYGNN_OK;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && w->pos_w0 && w->pos_b0 && w->pos_w1 && w->pos_b1 && w->proj0_w && w->proj0_b && w->proj1_w && w->proj1_b,
                  "cawn: null weights");
    for (int e = 0; e < 2; ++e)
        for (int dir = 0; dir < 2; ++dir) {
            const dygnn_cawn_lstm_weights& m = e == 0 ? w->feature[dir] : w->position[dir];
            DYGNN_REQUIRE(m.w_ih && m.w_hh && m.b_ih && m.b_hh, "cawn: null LSTM weights (%s encoder, direction %d)", e == 0 ? "feature" : "position", dir);
        }
    {
        const dygnn_tcl_layer_weights& m = w->attn;
        DYGNN_REQUIRE(m.in_proj_w && m.in_proj_b && m.out_proj_w && m.out_proj_b && m.fc0_w && m.fc0_b && m.fc1_w && m.fc1_b && m.norm0_w && m.norm0_b &&
                      m.norm1_w && m.norm1_b, "cawn: null transformer weights");
    }
    const Dims d = dims_of(*cfg);
    DYGNN_REQUIRE(node_feat && edge_feat && side_root && side_time && hops && hops->id[0] && hops->eid[0] && hops->t[0] && pair_a && pair_b && out_a && out_b &&
                  workspace, "cawn: null pointer");
    DYGNN_REQUIRE(d.W == 1 || (hops->id[1] && hops->eid[1] && hops->t[1]), "cawn: null pointer (hop 2 arrays)");
    const int64_t N = n_sides, P = n_pairs, I = 2 * P, R = I * d.M;
    for (int64_t p = 0; p < P; ++p)
        DYGNN_REQUIRE(pair_a[p] >= 0 && pair_a[p] < N && pair_b[p] >= 0 && pair_b[p] < N, "cawn: pair %lld names a side outside [0, %lld)", (long long)p,
                      (long long)N);
    const Plan pl = make_plan(d, P);
    if (workspace_bytes < pl.total) {
        set_error("cawn: workspace too small (%zu < %zu bytes)", workspace_bytes, pl.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* base = static_cast<char*>(workspace);
    auto fp = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    int32_t* own = reinterpret_cast<int32_t*>(base + pl.own);       // side of sequence i: (a_p, b_p) interleaved
    int32_t* pidx = reinterpret_cast<int32_t*>(base + pl.pidx);
    {
        std::vector<int32_t> idx((size_t)I);
        for (int64_t p = 0; p < P; ++p) idx[2 * p] = pair_a[p], idx[2 * p + 1] = pair_b[p];
        DYGNN_HIP(hipMemcpyAsync(own, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
        DYGNN_HIP(hipStreamSynchronize(s));                          // idx is about to go out of scope
    }
    const Tree tr{hops->id[0], hops->id[1], hops->eid[0], hops->eid[1], hops->t[0], hops->t[1]};
    int rc;
    const size_t lds_pos = pos_lds_bytes(d.Pd);
    if ((rc = lds_limit(k_cawn_pos, lds_pos))) return rc;
    hipLaunchKernelGGL(k_cawn_pos, dim3((unsigned)P), dim3(kThreads), lds_pos, s, side_root, tr, own, w->pos_w0, w->pos_b0, w->pos_w1, w->pos_b1, d.k, d.W, d.M,
                       d.T, d.Pd, pidx, fp(pl.ct), fp(pl.pf));
    DYGNN_LAUNCH_CHECK();
    const int64_t tap_rows = taps ? (taps->rows < P ? taps->rows : P) : 0;
    const int64_t tap_walks = 2 * tap_rows * d.M;
    if (tap_rows > 0 && (taps->walk_ids || taps->counts)) {
        const int64_t n = tap_walks * (d.W + 1);
        hipLaunchKernelGGL(k_cawn_tap_walks, dim3((unsigned)ceil_div(n, kThreads)), dim3(kThreads), 0, s, side_root, tr, own, pidx, fp(pl.ct), d.k, d.W, d.M, d.T,
                           n, taps->walk_ids, taps->counts);
        DYGNN_LAUNCH_CHECK();
    }
    for (int e = 0; e < 2; ++e) {
        const dygnn_cawn_lstm_weights* m = e == 0 ? w->feature : w->position;
        const int H = e == 0 ? d.Hf : d.Hp;
        LstmArgs a{};
        a.node_feat = node_feat, a.edge_feat = edge_feat, a.side_root = side_root, a.side_time = side_time, a.tr = tr, a.own = own, a.pidx = pidx;
        a.PF = fp(pl.pf), a.time_w = w->time_w, a.time_b = w->time_b;
        a.node_rows = cfg->num_node_rows, a.edge_rows = cfg->num_edge_rows;
        a.pos_only = e, a.Fn = d.Fn, a.Fe = d.Fe, a.Ft = d.Ft, a.Pd = d.Pd, a.k = d.k, a.W = d.W, a.M = d.M, a.T = d.T, a.H = H;
        a.w_ih = m[0].w_ih, a.w_hh = m[0].w_hh, a.b_ih = m[0].b_ih, a.b_hh = m[0].b_hh;
        // step 0: once per sequence, from the zero state
        a.mode = 0, a.rows = I, a.h_prev = a.c_prev = nullptr, a.h_out = fp(pl.h0[e]), a.ld_out = H, a.col_out = 0, a.c_out = fp(pl.c0[e]);
        if ((rc = launch_lstm(s, a))) return rc;
        // steps 1 .. W: once per tree node of the hop; the last one writes the forward half of the encoder output
        for (int hop = 1; hop <= d.W; ++hop) {
            const bool last = hop == d.W;
            a.mode = 1, a.hop = hop, a.n_hop = hop == 1 ? d.k : d.M, a.rows = I * a.n_hop;
            a.h_prev = hop == 1 ? fp(pl.h0[e]) : fp(pl.h1[e]), a.c_prev = hop == 1 ? fp(pl.c0[e]) : fp(pl.c1[e]);
            a.h_out = last ? fp(pl.enc[e]) : fp(pl.h1[e]), a.ld_out = last ? 2 * H : H, a.c_out = last ? nullptr : fp(pl.c1[e]);
            if ((rc = launch_lstm(s, a))) return rc;
        }
        // the reverse direction's output at the last valid position: its first step
        a.w_ih = m[1].w_ih, a.w_hh = m[1].w_hh, a.b_ih = m[1].b_ih, a.b_hh = m[1].b_hh;
        a.mode = 2, a.rows = R, a.h_prev = a.c_prev = nullptr, a.h_out = fp(pl.enc[e]), a.ld_out = 2 * H, a.col_out = H, a.c_out = nullptr;
        if ((rc = launch_lstm(s, a))) return rc;
    }
    float *X = fp(pl.x), *Y = fp(pl.y);
    rc = d.A <= 256 ? transformer<4, 4>(s, d, *w, fp(pl.enc[0]), fp(pl.enc[1]), R, X, fp(pl.qkv), fp(pl.o), Y)
       : d.A <= 320 ? transformer<5, 2>(s, d, *w, fp(pl.enc[0]), fp(pl.enc[1]), R, X, fp(pl.qkv), fp(pl.o), Y)
                    : transformer<8, 2>(s, d, *w, fp(pl.enc[0]), fp(pl.enc[1]), R, X, fp(pl.qkv), fp(pl.o), Y);
    if (rc) return rc;
    const size_t lds_out = (size_t)16 * (round16(d.A) + 4) * sizeof(float);
    hipLaunchKernelGGL(k_cawn_out, dim3((unsigned)ceil_div(I, kOutSeqs)), dim3(kThreads), lds_out, s, Y, I, d.M, w->proj1_w, w->proj1_b, d.A, d.Fn, out_a, out_b);
    DYGNN_LAUNCH_CHECK();
    if (tap_rows > 0) {
        const size_t n = (size_t)tap_walks * sizeof(float);
        if (taps->feature_out) DYGNN_HIP(hipMemcpyAsync(taps->feature_out, fp(pl.enc[0]), n * 2 * d.Hf, hipMemcpyDeviceToDevice, s));
        if (taps->position_out) DYGNN_HIP(hipMemcpyAsync(taps->position_out, fp(pl.enc[1]), n * 2 * d.Hp, hipMemcpyDeviceToDevice, s));
        if (taps->attn_in) DYGNN_HIP(hipMemcpyAsync(taps->attn_in, X, n * d.A, hipMemcpyDeviceToDevice, s));
        if (taps->attn_out) DYGNN_HIP(hipMemcpyAsync(taps->attn_out, Y, n * d.A, hipMemcpyDeviceToDevice, s));
    }
    return DYGNN_OK;
}
