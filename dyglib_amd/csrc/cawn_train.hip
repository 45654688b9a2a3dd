// CAWN training (models/CAWN.py:48-396, TransformerEncoder models/modules.py:209-266): the forward of cawn.hip in TRAIN mode and its hand-written
// backward pass, so that train_link_prediction.py's two calls, MergeLayer + BCE, loss.backward() and Adam run on the HIP path.
//
// Layout.  A call works on 2 B sides [src ; dst]; pair p is (side p, side B + p) and makes the sequences q = 2 p (source) and 2 p + 1
// (destination), so the side of sequence q is (q & 1) B + (q >> 1): computed where it is needed, no index vector, no host synchronisation.
// Tree nodes are stored LEVEL-MAJOR: level lv (0 the target, 1 hop 1, 2 hop 2) has n_lv = k^lv nodes per sequence and the rows
// base_lv + q n_lv + j, base = (0, I, I (1 + k)), I = 2 B sequences, NT = I T rows in all.  The parent of row r of level lv is row r / k of
// level lv - 1, so the rows of a level and of its parents are both contiguous: every product of the BiLSTMs is a plain dense product
// (train::mm, fp32 MFMA) over a level, and the hidden-state products run over the PARENTS (k times fewer rows):
//     forward   gates(level lv)  = X W_ih^T + b_ih  (all NT rows at once)  +  (h_parent W_hh^T)[r / k]  + b_hh
//     backward  dh_parent        = (sum over the k children of dG) W_hh,      dW_hh += (sum over the children of dG)^T h_parent
// Both exact rewrites of cawn.hip are kept (position 0 once per sequence: it IS level 0; the reverse direction as one cell from the zero state,
// here computed once per tree node and read by every walk whose last valid position it is), and the backward adds a third: node and edge
// features are constants, so only the F_t time columns and the P position columns of dx = dG W_ih are computed.
//
// Saved per call (workspace, read by the backward pass): the gathered input rows X [NT][D] (RESTAGED in HBM: they are the B operand of
// dW_ih += dG^T X, read by the general product with no gather of its own, and the forward's W_ih product reads the same rows), valid flag
// and dt per tree node, pidx / counts / summed MLP hidden rows / PF per pair; per LSTM cell the four gate ACTIVATIONS [NT][4H] (stored, not
// recomputed: the backward overwrites them in place with the gate gradients, which then feed four products) and c, h [NT][H], for the forward
// direction and (gates only) the reverse cell of both encoders; the encoder outputs [R][D + P]; the block's activations as tcl_train.hip
// saves them (X0, q | k | v, the softmax before dropout, O, both pre-LayerNorm sums with mean and rstd, LayerNorm 0's output, the
// post-ReLU post-dropout hidden rows).
//
// Dropout.  Masks are never stored: forward and backward redraw them from train::Drop (dropout.h).  Sites 0 .. 3 of the one block:
//   site 0 (attention probabilities) element ((q H + h) M + i) M + j;  sites 1 (attention block output), 3 (fc1 output) element
//   (q M + i) A + c;  site 2 (relu(fc0)) element (q M + i) 4A + c.
//
// Kernels (k_cawnt_*): tree (ids, dt, valid per node), pos (counts and unique ids of a pair by all-pairs comparison in LDS: <= 146 ids),
// poshid / mlp_bwd (the position MLP's first layer and its backward), gather (X rows), cell / cell_bwd / rev_bwd / child_sum (the LSTM cell,
// elementwise on the product outputs), encout, attn_fwd / attn_bwd (one (sequence, head) per workgroup, M <= 64), mean / bcast, pos_scatter
// (the position-feature gradients of a pair summed per unique id in FIXED tree order by the row's one owner: no atomics).  Shared with
// tcl_train.hip: the block's launch sequence (train::encoder_block_forward / _backward, encoder_block_train.h; identity row map, site base 0)
// and its row kernels (train_rows.h: train::k_res_ln<8> / k_res_ln_bwd<8> for widths up to 512, k_row_drop / k_hid_bwd, k_time_part /
// k_time_fin, the fp64 two-stage sums), and the column sums' wave-per-column second stage (train::colsum, colsum.h; its second output gives
// b_hh the sum of b_ih).  Dense products go through train::mm, weight gradients
// through train::dw_grouped where its alignment rules hold and train::mm (transposed A, accumulating) where they do not (position_feat_dim
// = 2 mod 4); bias, LayerNorm and time-encoder gradients are fixed-order column sums; b_ih and b_hh receive the same sum.
#include "colsum.h"
#include "common.h"
#include "dropout.h"
#include "encoder_block_train.h"
#include "gemm.h"
#include "mfma_tile.h"
#include "time_encoding.h"

namespace dygnn {
namespace cawnt {

using timeenc::cos_time;
using train::colsum;

constexpr int kMaxWalks = 64;       // M = k^W: one key per lane in the attention kernels
constexpr int kMaxTree2 = 2 * (1 + 8 + 64);      // tree positions of a pair
constexpr int kMaxHead = 64;
constexpr int kLdh = kMaxHead + 1;
constexpr int kNV = 8;              // columns per lane of a row (train_rows.h): attention_dim <= 512

struct Dims {
    int Fn, Fe, Ft, Pd, W, k, M, T, D, Hf, Hp, A, heads, E;
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
    d.E = 2 * d.Hf + 2 * d.Hp;
    return d;
}

// the level-major row layout of the tree nodes
struct Lay {
    int k, W, M, T;
    int64_t I;
    __host__ __device__ int n(int lv) const { return lv == 0 ? 1 : lv == 1 ? k : k * k; }
    __host__ __device__ int off(int lv) const { return lv == 0 ? 0 : lv == 1 ? 1 : 1 + k; }
    __host__ __device__ int64_t base(int lv) const { return lv == 0 ? 0 : lv == 1 ? I : I * (1 + k); }
    __host__ __device__ int64_t rows() const { return I * T; }
    __device__ int64_t row(int64_t q, int e) const {
        const int lv = e == 0 ? 0 : e <= k ? 1 : 2;
        return base(lv) + q * n(lv) + (e - off(lv));
    }
    __device__ void unrow(int64_t g, int64_t& q, int& e) const {
        const int lv = g < base(1) ? 0 : (W == 1 || g < base(2)) ? 1 : 2;
        const int64_t r = g - base(lv);
        q = r / n(lv);
        e = off(lv) + (int)(r - q * n(lv));
    }
    // the row whose reverse cell walk j of sequence q reads: its last valid position (cawn.hip, mode 2)
    __device__ int64_t pick(const int32_t* __restrict__ valid, int64_t q, int j) const {
        if (W == 2) {
            const int64_t g2 = base(2) + q * M + j;
            if (valid[g2]) return g2;
            const int64_t g1 = base(1) + q * k + j / k;
            return valid[g1] ? g1 : q;
        }
        const int64_t g1 = base(1) + q * k + j;
        return valid[g1] ? g1 : q;
    }
};

struct Tree {
    const int64_t *root, *id1, *id2, *eid1, *eid2;
    const double* time;
    const float *t1, *t2;
};

// ---- tree nodes: raw id (position counts), clamped feature rows, dt, valid --------------------------------------------------------------------
__global__ void k_cawnt_tree(Tree tr, Lay L, int64_t B, int64_t node_rows, int64_t edge_rows, int64_t* __restrict__ rawid, int32_t* __restrict__ nid,
                             int32_t* __restrict__ eidc, float* __restrict__ dtv, int32_t* __restrict__ valid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.rows()) return;
    const int64_t q = i / L.T;
    const int e = (int)(i - q * L.T), k = L.k, M = L.M;
    const int64_t s = (q & 1) * B + (q >> 1);
    int64_t id = e == 0 ? tr.root[s] : e <= k ? tr.id1[s * k + e - 1] : tr.id2[s * M + e - 1 - k];
    if (id < 0) id = 0;
    int64_t eid = 0;
    float dt = 0.f;
    if (e > 0) {
        eid = e <= k ? tr.eid1[s * k + e - 1] : tr.eid2[s * M + e - 1 - k];
        const float tn = e <= k ? tr.t1[s * k + e - 1] : tr.t2[s * M + e - 1 - k];
        dt = (float)(tr.time[s] - (double)tn);                          // f64 - f32 -> f64 -> .float()
    }
    const int64_t g = L.row(q, e);
    rawid[g] = id;
    nid[g] = (int32_t)(id >= node_rows ? 0 : id);
    eidc[g] = (int32_t)((eid < 0 || eid >= edge_rows) ? 0 : eid);
    dtv[g] = dt;
    valid[g] = e == 0 || id != 0;
}

// ---- position counts of a pair (models/CAWN.py:197-289): one workgroup per pair, one thread per tree position of the two trees -----------------
// The unique ids are numbered in the order of their first tree position (as k_cawn_pos does); CT [P][2 T][2][3] = count / k^hop, zero for
// id 0 and (by the caller's fill) for the rows beyond the pair's unique ids.
__global__ __launch_bounds__(256) void k_cawnt_pos(const int64_t* __restrict__ rawid, Lay L, int32_t* __restrict__ pidx, float* __restrict__ CT) {
    __shared__ int64_t s_id[kMaxTree2];
    __shared__ int s_rep[kMaxTree2], s_u[kMaxTree2];
    const int64_t p = blockIdx.x;
    const int T = L.T, T2 = 2 * T, e2 = threadIdx.x, k = L.k;
    if (e2 < T2) {
        const int sel = e2 >= T;
        s_id[e2] = rawid[L.row(2 * p + sel, e2 - sel * T)];
    }
    __syncthreads();
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    int64_t id = 0;
    if (e2 < T2) {
        id = s_id[e2];
        int rep = e2;
        for (int x = 0; x < T2; ++x) {
            if (s_id[x] != id) continue;
            if (x < rep) rep = x;
            const int sx = x >= T, ex = x - sx * T;
            ++cnt[sx * 3 + (ex == 0 ? 0 : ex <= k ? 1 : 2)];
        }
        s_rep[e2] = rep;
    }
    __syncthreads();
    if (e2 < T2 && s_rep[e2] == e2) {
        int u = 0;
        for (int x = 0; x < e2; ++x) u += s_rep[x] == x;
        s_u[e2] = u;
        float* ct = CT + ((size_t)p * T2 + u) * 6;
#pragma unroll
        for (int x = 0; x < 6; ++x) {
            const int hop = x % 3;
            const float n = hop == 0 ? 1.f : hop == 1 ? (float)k : (float)(k * k);
            ct[x] = id == 0 ? 0.f : (float)cnt[x] / n;                  // the padded node's entry is set to zero (:255)
        }
    }
    __syncthreads();
    if (e2 < T2) pidx[p * T2 + e2] = s_u[s_rep[e2]];
}

// HS[r][f] = relu(b0 + W0 ct[r][0]) + relu(b0 + W0 ct[r][1]): both count rows go through the same MLP and their outputs add
__global__ void k_cawnt_poshid(const float* __restrict__ CT, const float* __restrict__ w0, const float* __restrict__ b0, int64_t rows, int Pd, int W1,
                               float* __restrict__ HS) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * Pd) return;
    const int64_t r = i / Pd;
    const int f = (int)(i - r * Pd);
    float s = 0.f;
    for (int sel = 0; sel < 2; ++sel) {
        float v = b0[f];
        for (int h = 0; h < W1; ++h) v = fmaf(CT[r * 6 + sel * 3 + h], w0[f * W1 + h], v);
        s += fmaxf(v, 0.f);
    }
    HS[i] = s;
}
// DP[2 r + sel][f] = dHS[r][f] where the first layer's pre-activation of count row sel is positive
__global__ void k_cawnt_mlp_bwd(const float* __restrict__ CT, const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ dHS,
                                int64_t rows, int Pd, int W1, float* __restrict__ DP) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * Pd) return;
    const int64_t r = i / Pd;
    const int f = (int)(i - r * Pd);
    const float g = dHS[i];
    for (int sel = 0; sel < 2; ++sel) {
        float v = b0[f];
        for (int h = 0; h < W1; ++h) v = fmaf(CT[r * 6 + sel * 3 + h], w0[f * W1 + h], v);
        DP[(2 * r + sel) * Pd + f] = v > 0.f ? g : 0.f;
    }
}
__global__ void k_cawnt_scale(const float* __restrict__ x, int n, float a, float* __restrict__ y) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = a * x[i];
}

// ---- the input row of every tree node (models/CAWN.py:342): [node | cos(dt w + b) | edge | position feature], zero for a padded node -------------
__global__ void k_cawnt_gather(const float* __restrict__ node_feat, const float* __restrict__ edge_feat, const int32_t* __restrict__ nid,
                               const int32_t* __restrict__ eidc, const float* __restrict__ dtv, const int32_t* __restrict__ valid,
                               const int32_t* __restrict__ pidx, const float* __restrict__ PF, const float* __restrict__ tw, const float* __restrict__ tb,
                               Lay L, int Fn, int Ft, int Fe, int Pd, float* __restrict__ X) {
    const int D = Fn + Ft + Fe + Pd;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.rows() * D) return;
    const int64_t g = i / D;
    const int col = (int)(i - g * D);
    float v = 0.f;
    if (valid[g]) {
        if (col < Fn) v = node_feat[(size_t)nid[g] * Fn + col];
        else if (col < Fn + Ft) v = cos_time(fmaf(dtv[g], tw[col - Fn], tb[col - Fn]));
        else if (col < Fn + Ft + Fe) v = edge_feat[(size_t)eidc[g] * Fe + col - Fn - Ft];
        else {
            int64_t q;
            int e;
            L.unrow(g, q, e);
            const int64_t p = q >> 1;
            v = PF[((size_t)p * 2 * L.T + pidx[p * 2 * L.T + (q & 1) * L.T + e]) * Pd + col - Fn - Ft - Fe];
        }
    }
    X[i] = v;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- the LSTM cell of the rows r < rows of one level: G [.][4H] holds X W_ih^T + b_ih on entry and the gate activations i, f, g, o on exit;
// HH [rows / k][4H] = h_parent W_hh^T (NULL: the zero state).  A padded node carries its parent's state on.  rev: the reverse cell (always from
// the zero state; never read at a padded node).
__global__ void k_cawnt_cell(float* __restrict__ G, const float* __restrict__ HH, const float* __restrict__ b_hh, const int32_t* __restrict__ valid,
                             int64_t base, int64_t base_par, int64_t rows, int k, int H, float* __restrict__ hbuf, float* __restrict__ cbuf) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * H) return;
    const int64_t r = i / H, g = base + r, rp = r / k, par = base_par + rp;
    const int u = (int)(i - r * H);
    float* gt = G + (size_t)g * 4 * H;
    float pre[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        pre[t] = gt[t * H + u] + b_hh[t * H + u];
        if (HH) pre[t] += HH[(size_t)rp * 4 * H + t * H + u];
    }
    const float gi = sigmoidf_(pre[0]), gf = sigmoidf_(pre[1]), gg = tanhf(pre[2]), go = sigmoidf_(pre[3]);
    const float cp = HH ? cbuf[(size_t)par * H + u] : 0.f;
    float cn = fmaf(gf, cp, gi * gg);
    float h = go * tanhf(cn);
    if (HH && !valid[g]) {                                           // the walk ended before this node
        cn = cp;
        h = hbuf[(size_t)par * H + u];
    }
    gt[u] = gi, gt[H + u] = gf, gt[2 * H + u] = gg, gt[3 * H + u] = go;
    hbuf[(size_t)g * H + u] = h;
    if (cbuf) cbuf[(size_t)g * H + u] = cn;
}

// encoder outputs of walk row r = q M + j: [forward h of its hop-W node | reverse h of its last valid node] of both encoders -> EO [R][E]
__global__ void k_cawnt_encout(const float* __restrict__ hF, const float* __restrict__ rF, const float* __restrict__ hP, const float* __restrict__ rP,
                               const int32_t* __restrict__ valid, Lay L, int Hf, int Hp, float* __restrict__ EO) {
    const int E = 2 * Hf + 2 * Hp;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.I * L.M * E) return;
    const int64_t r = i / E, q = r / L.M;
    const int col = (int)(i - r * E), j = (int)(r - q * L.M);
    const int64_t top = L.base(L.W) + r;
    float v;
    if (col < Hf) v = hF[(size_t)top * Hf + col];
    else if (col < 2 * Hf) v = rF[(size_t)L.pick(valid, q, j) * Hf + col - Hf];
    else if (col < 2 * Hf + Hp) v = hP[(size_t)top * Hp + col - 2 * Hf];
    else v = rP[(size_t)L.pick(valid, q, j) * Hp + col - 2 * Hf - Hp];
    EO[i] = v;
}

// ---- attention forward of (sequence q, head h), no key mask: saves the softmax P, multiplies the site-0 mask in, writes O ------------------------
// qkv rows [q | k | v] of stride 3 d.  Wave w owns the query rows w, w + 4, ...; lane l scores key l.  Dynamic LDS: Q, K, V [M][65].
__global__ __launch_bounds__(256) void k_cawnt_attn_fwd(const float* __restrict__ qkv, int M, int d, int Hn, float scale, train::Drop dr,
                                                          float* __restrict__ P, float* __restrict__ O) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ks = Qs + M * kLdh;
    float* Vs = Ks + M * kLdh;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dh = d / Hn, ld = 3 * d, h = blockIdx.y;
    const int64_t q = blockIdx.x;
    const float* src = qkv + (size_t)q * M * ld + h * dh;
    for (int x = threadIdx.x; x < M * dh; x += 256) {
        const int r = x / dh, cc = x - r * dh;
        Qs[r * kLdh + cc] = src[(size_t)r * ld + cc];
        Ks[r * kLdh + cc] = src[(size_t)r * ld + d + cc];
        Vs[r * kLdh + cc] = src[(size_t)r * ld + 2 * d + cc];
    }
    __syncthreads();
    const bool on = lane < M;
    const uint32_t skey = dr.site_key(0);
    for (int r = wave; r < M; r += 4) {
        float s = 0.f;
        const float* kr = Ks + (on ? lane : 0) * kLdh;
        for (int cc = 0; cc < dh; ++cc) s = fmaf(Qs[r * kLdh + cc], kr[cc], s);
        s = on ? s * scale : -INFINITY;
        const float m = wave_max(s);
        const float ex = on ? expf(s - m) : 0.f;
        const float p = ex / wave_sum(ex);
        float pd = 0.f;
        if (on) {
            const uint64_t idx = (((uint64_t)q * Hn + h) * M + r) * M + lane;
            P[idx] = p;
            pd = p * dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
        }
        const int col = lane < dh ? lane : 0;
        float o = 0.f;
        for (int j = 0; j < M; ++j) o = fmaf(__shfl(pd, j), Vs[j * kLdh + col], o);
        if (lane < dh) O[((size_t)q * M + r) * d + h * dh + lane] = o;
    }
}

// ---- attention backward of (sequence q, head h) ------------------------------------------------------------------------------------------------
// Pass A, wave per query row i, lane = key j: dP = dO_i . V_j, times the redrawn site-0 mask; dS = scale P (dP - sum_j P dP); dS and P mask
// go to LDS; dQ_i = sum_j dS_ij K_j (lane = head column).  Pass B, wave per key row j, lane = head column: dK_j = sum_i dS_ij Q_i,
// dV_j = sum_i (P mask)_ij dO_i.  One producer per row of dqkv.  Dynamic LDS: Q, K, V, dO [M][65], dS, Pm [M][M + 1].
__global__ __launch_bounds__(256) void k_cawnt_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dO, int M, int d,
                                                          int Hn, float scale, train::Drop dr, float* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ks = Qs + M * kLdh;
    float* Vs = Ks + M * kLdh;
    float* Gs = Vs + M * kLdh;
    const int ldp = M + 1;
    float* dS = Gs + M * kLdh;
    float* Pm = dS + M * ldp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int dh = d / Hn, ld = 3 * d, h = blockIdx.y;
    const int64_t q = blockIdx.x;
    const float* src = qkv + (size_t)q * M * ld + h * dh;
    const float* go = dO + (size_t)q * M * d + h * dh;
    float* dst = dqkv + (size_t)q * M * ld + h * dh;
    for (int x = threadIdx.x; x < M * dh; x += 256) {
        const int r = x / dh, cc = x - r * dh;
        Qs[r * kLdh + cc] = src[(size_t)r * ld + cc];
        Ks[r * kLdh + cc] = src[(size_t)r * ld + d + cc];
        Vs[r * kLdh + cc] = src[(size_t)r * ld + 2 * d + cc];
        Gs[r * kLdh + cc] = go[(size_t)r * d + cc];
    }
    __syncthreads();
    const bool on = lane < M;
    const uint32_t skey = dr.site_key(0);
    const int col = lane < dh ? lane : 0;
    for (int i = wave; i < M; i += 4) {
        float dp = 0.f, p = 0.f, m = 0.f;
        if (on) {
            for (int cc = 0; cc < dh; ++cc) dp = fmaf(Gs[i * kLdh + cc], Vs[lane * kLdh + cc], dp);
            const uint64_t idx = (((uint64_t)q * Hn + h) * M + i) * M + lane;
            p = P[idx];
            m = dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
            dp *= m;
        }
        const float t = wave_sum(p * dp);
        const float ds = scale * (p * (dp - t));
        if (on) {
            dS[i * ldp + lane] = ds;
            Pm[i * ldp + lane] = p * m;
        }
        float a = 0.f;
        for (int j = 0; j < M; ++j) a = fmaf(__shfl(ds, j), Ks[j * kLdh + col], a);
        if (lane < dh) dst[(size_t)i * ld + lane] = a;
    }
    __syncthreads();
    for (int j = wave; j < M; j += 4) {
        float dk = 0.f, dv = 0.f;
        for (int i = 0; i < M; ++i) {
            dk = fmaf(dS[i * ldp + j], Qs[i * kLdh + col], dk);
            dv = fmaf(Pm[i * ldp + j], Gs[i * kLdh + col], dv);
        }
        if (lane < dh) {
            dst[(size_t)j * ld + d + lane] = dk;
            dst[(size_t)j * ld + 2 * d + lane] = dv;
        }
    }
}

// YM[q][c] = mean over the M walks of Y[q M + j][c]
__global__ void k_cawnt_mean(const float* __restrict__ Y, int64_t I, int M, int d, float* __restrict__ YM) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I * d) return;
    const int64_t q = i / d;
    const int c = (int)(i - q * d);
    float v = 0.f;
    for (int j = 0; j < M; ++j) v += Y[((size_t)q * M + j) * d + c];
    YM[i] = v / (float)M;
}
// dY[q M + j][c] = dYM[q][c] / M
__global__ void k_cawnt_bcast(const float* __restrict__ dYM, int64_t R, int M, int d, float* __restrict__ dY) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * d) return;
    const int64_t r = i / d;
    dY[i] = dYM[(r / M) * d + (i - r * d)] / (float)M;
}

// ---- the reverse cell's backward, all tree rows: the gradient of row g is the sum over the walks that read it (gathered by the row) -------------
// G [NT][4H] holds the activations on entry and the gate gradients on exit (the f gate's is zero: c_prev = 0).
__global__ void k_cawnt_rev_bwd(float* __restrict__ G, const float* __restrict__ dEO, int E, int col0, const int32_t* __restrict__ valid, Lay L, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.rows() * H) return;
    const int64_t g = i / H;
    const int u = (int)(i - g * H);
    int64_t q;
    int e;
    L.unrow(g, q, e);
    const int lv = e == 0 ? 0 : e <= L.k ? 1 : 2;
    const int span = L.M / L.n(lv), j0 = (e - L.off(lv)) * span;
    float dh = 0.f;
    if (valid[g])
        for (int j = j0; j < j0 + span; ++j)
            if (L.pick(valid, q, j) == g) dh += dEO[((size_t)q * L.M + j) * E + col0 + u];
    float* gt = G + (size_t)g * 4 * H;
    const float gi = gt[u], gg = gt[2 * H + u], go = gt[3 * H + u];
    const float tc = tanhf(gi * gg);
    const float dct = dh * go * (1.f - tc * tc);
    gt[u] = dct * gg * gi * (1.f - gi);
    gt[H + u] = 0.f;
    gt[2 * H + u] = dct * gi * (1.f - gg * gg);
    gt[3 * H + u] = dh * tc * go * (1.f - go);
}

// ---- the forward direction's cell backward on the rows of one level ----------------------------------------------------------------------------
// (dh, dc) of row r: at the top level the walk's output gradient dEO[r][col0 + u] (dc = 0); below, DHP[r] = (sum over the children of dG) W_hh
// plus what the padded children pass on unchanged (CH, CC of the level below).  G: activations in, gate gradients out (zero for a padded
// node); CH / CC [NT][H]: what this row hands to its parent outside the product (a padded node: (dh, dc); a valid one: (0, dc f)).
__global__ void k_cawnt_cell_bwd(float* __restrict__ G, const float* __restrict__ cbuf, const int32_t* __restrict__ valid, const float* __restrict__ dEO,
                                 int E, int col0, const float* __restrict__ DHP, float* __restrict__ CH, float* __restrict__ CC, int64_t base,
                                 int64_t base_par, int64_t base_child, int64_t rows, int k, int H, int top, int has_par) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * H) return;
    const int64_t r = i / H, g = base + r;
    const int u = (int)(i - r * H);
    float dh, dc = 0.f;
    if (top) dh = dEO[(size_t)r * E + col0 + u];
    else {
        dh = DHP[(size_t)r * H + u];
        for (int ch = 0; ch < k; ++ch) {
            const size_t c = (size_t)(base_child + r * k + ch) * H + u;
            dh += CH[c];
            dc += CC[c];
        }
    }
    float* gt = G + (size_t)g * 4 * H;
    float ph = dh, pc = dc;
    float di = 0.f, df = 0.f, dg = 0.f, dO = 0.f;
    if (!has_par || valid[g]) {
        const float gi = gt[u], gf = gt[H + u], gg = gt[2 * H + u], go = gt[3 * H + u];
        const float cp = has_par ? cbuf[(size_t)(base_par + r / k) * H + u] : 0.f;
        const float tc = tanhf(cbuf[(size_t)g * H + u]);
        const float dct = dc + dh * go * (1.f - tc * tc);
        dO = dh * tc * go * (1.f - go);
        di = dct * gg * gi * (1.f - gi);
        dg = dct * gi * (1.f - gg * gg);
        df = dct * cp * gf * (1.f - gf);
        ph = 0.f;
        pc = dct * gf;
    }
    gt[u] = di, gt[H + u] = df, gt[2 * H + u] = dg, gt[3 * H + u] = dO;
    if (has_par) {
        CH[(size_t)g * H + u] = ph;
        CC[(size_t)g * H + u] = pc;
    }
}
// SG[a][x] = sum over the k children of parent a of G[child][x] (x < 4H), in child order
__global__ void k_cawnt_child_sum(const float* __restrict__ G, int64_t base_child, int64_t parents, int k, int H4, float* __restrict__ SG) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= parents * H4) return;
    const int64_t a = i / H4;
    const int x = (int)(i - a * H4);
    float s = 0.f;
    for (int ch = 0; ch < k; ++ch) s += G[(size_t)(base_child + a * k + ch) * H4 + x];
    SG[i] = s;
}

// ---- position features: dPF[p][u] = sum, in tree order, of dXP over the tree positions of pair p whose unique id is u ------------------------------
// One workgroup per pair; every (u, column) has one owner thread that walks the 2 T positions in order: exact to rounding, the same bits run
// to run, no atomics.
__global__ __launch_bounds__(256) void k_cawnt_pos_scatter(const float* __restrict__ dXP, const int32_t* __restrict__ pidx, Lay L, int Pd,
                                                             float* __restrict__ dPF) {
    __shared__ int s_u[kMaxTree2];
    __shared__ int64_t s_row[kMaxTree2];
    const int64_t p = blockIdx.x;
    const int T = L.T, T2 = 2 * T;
    if (threadIdx.x < T2) {
        const int e2 = threadIdx.x, sel = e2 >= T;
        s_u[e2] = pidx[p * T2 + e2];
        s_row[e2] = L.row(2 * p + sel, e2 - sel * T);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < T2 * Pd; x += 256) {
        const int u = x / Pd, f = x - u * Pd;
        float a = 0.f;
        for (int e2 = 0; e2 < T2; ++e2)
            if (s_u[e2] == u) a += dXP[(size_t)s_row[e2] * Pd + f];
        dPF[((size_t)p * T2 + u) * Pd + f] = a;
    }
}

// C[m][n] += sum_k A[k][m] B[k][n]: the grouped split-K kernel where its alignment rules hold, the general product otherwise
static int wgrad(hipStream_t s, int K, const float* A, int lda, int M, const float* B, int ldb, int N, float* C, int ldc) {
    const bool aligned = ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) == 0 && lda % 4 == 0 && ldb % 4 == 0 && M % 4 == 0 &&
                         N % 4 == 0 && (M + 127) / 128 <= 64 && (N + 207) / 208 <= 64 && ((M + 127) / 128) * ((N + 207) / 208) <= 128;
    if (aligned) {
        const train::DwPair pr{A, lda, M, B, ldb, N, C, ldc, nullptr};
        return train::dw_grouped(s, K, &pr, 1);
    }
    return train::mm(s, A, lda, true, B, ldb, false, C, ldc, M, N, K, train::MmOpt().beta(1.f));
}

// ---- workspace ------------------------------------------------------------------------------------------------------------------------------
struct Enc { size_t G, GR, h, c, hr; };
struct Plan {
    Dims d;
    int64_t B, I, R, NT, PR;                                        // PR = P 2 T rows of the position tables
    size_t rawid, nid, eidc, dtv, valid, pidx, ct, hs, pf, b1x2, x;
    Enc enc[2];
    size_t hh, eo, x0, qkv, P, O, tmp, pre0, mean0, rstd0, y0, hid, pre1, mean1, rstd1, y, ym;      // forward
    size_t gA, gB, gC, gD, gE, gF, dhid, dqkv, part, deo, dym, ch, cc, sg, dhp, dxt, dxp, tpart, dpf, dhs, dp;      // backward scratch
    size_t total;
};
static Plan make_plan(const dygnn_cawn_config& c, int64_t B) {
    Plan p{};
    const Dims d = dims_of(c);
    p.d = d, p.B = B, p.I = 2 * B, p.R = p.I * d.M, p.NT = p.I * d.T, p.PR = B * 2 * d.T;
    const size_t I = (size_t)p.I, R = (size_t)p.R, NT = (size_t)p.NT, PR = (size_t)p.PR, A = (size_t)d.A;
    const size_t parents = I * (size_t)(d.W == 1 ? 1 : d.k);         // the largest parent level
    size_t o = 0;
    auto take = [&](size_t words) { size_t r = o; o += (words * 4 + 255) & ~size_t(255); return r; };      // 4-byte elements
    p.rawid = take(2 * NT), p.nid = take(NT), p.eidc = take(NT), p.dtv = take(NT), p.valid = take(NT);
    p.pidx = take(PR), p.ct = take(PR * 6), p.hs = take(PR * d.Pd), p.pf = take(PR * d.Pd), p.b1x2 = take(d.Pd);
    p.x = take(NT * d.D);
    for (int e = 0; e < 2; ++e) {
        const size_t H = e == 0 ? d.Hf : d.Hp;
        p.enc[e].G = take(NT * 4 * H), p.enc[e].GR = take(NT * 4 * H), p.enc[e].h = take(NT * H), p.enc[e].c = take(NT * H), p.enc[e].hr = take(NT * H);
    }
    p.hh = take(parents * 4 * d.Hf);
    p.eo = take(R * d.E), p.x0 = take(R * A), p.qkv = take(3 * R * A), p.P = take(I * d.heads * d.M * d.M), p.O = take(R * A), p.tmp = take(R * A);
    p.pre0 = take(R * A), p.mean0 = take(R), p.rstd0 = take(R), p.y0 = take(R * A), p.hid = take(4 * R * A);
    p.pre1 = take(R * A), p.mean1 = take(R), p.rstd1 = take(R), p.y = take(R * A), p.ym = take(I * A);
    p.gA = take(R * A), p.gB = take(R * A), p.gC = take(R * A), p.gD = take(R * A), p.gE = take(R * A), p.gF = take(R * A);
    p.dhid = take(4 * R * A), p.dqkv = take(3 * R * A);
    const size_t prow = (size_t)ceil_div((int64_t)(NT > 2 * PR ? NT : 2 * PR), tgt::kColRows);      // NT >= R: the rows of every column sum
    const size_t pcol = 4 * (A > (size_t)d.Hf ? A : (size_t)d.Hf);
    p.part = take(prow * pcol);
    p.deo = take(R * d.E), p.dym = take(I * A), p.ch = take(NT * d.Hf), p.cc = take(NT * d.Hf), p.sg = take(parents * 4 * d.Hf), p.dhp = take(parents * d.Hf);
    p.dxt = take(NT * d.Ft), p.dxp = take(NT * d.Pd), p.tpart = take((size_t)ceil_div(p.NT, tgt::kColRows) * 4 * d.Ft);
    p.dpf = take(PR * d.Pd), p.dhs = take(PR * d.Pd), p.dp = take(2 * PR * d.Pd);
    p.total = o;
    return p;
}

// the buffers of the one transformer block (encoder_block_train.h)
static train::BlockBufs bufs(const Plan& p, char* ws) {
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    return {F32(p.qkv), F32(p.O), F32(p.pre0), F32(p.mean0), F32(p.rstd0), F32(p.y0), F32(p.hid), F32(p.pre1), F32(p.mean1), F32(p.rstd1), F32(p.y),
            F32(p.tmp), F32(p.gA), F32(p.gB), F32(p.gC), F32(p.gD), F32(p.gE), F32(p.gF), F32(p.dhid), F32(p.dqkv), F32(p.part)};
}

static int check_lstm(const dygnn_cawn_lstm_weights* m, const char* what) {
    for (int dir = 0; dir < 2; ++dir) DYGNN_REQUIRE(m[dir].w_ih && m[dir].w_hh && m[dir].b_ih && m[dir].b_hh, "%s (an LSTM tensor, direction %d)", what, dir);
    return DYGNN_OK;
}
static int check_weights(const dygnn_cawn_weights* w, const char* what) {
    DYGNN_REQUIRE(w && w->time_w && w->time_b && w->pos_w0 && w->pos_b0 && w->pos_w1 && w->pos_b1 && w->proj0_w && w->proj0_b && w->proj1_w && w->proj1_b,
                  "%s", what);
    if (int rc = check_lstm(w->feature, what)) return rc;
    if (int rc = check_lstm(w->position, what)) return rc;
    const dygnn_tcl_layer_weights& m = w->attn;
    DYGNN_REQUIRE(m.in_proj_w && m.in_proj_b && m.out_proj_w && m.out_proj_b && m.fc0_w && m.fc0_b && m.fc1_w && m.fc1_b && m.norm0_w && m.norm0_b &&
                  m.norm1_w && m.norm1_b, "%s (a transformer tensor)", what);
    return DYGNN_OK;
}

// dygnn_cawn_check, then what the training path refuses beyond it
static int check_batch(const dygnn_cawn_config* cfg, int64_t batch, const char* what) {
    if (int rc = dygnn_cawn_check(cfg)) return rc;
    const Dims d = dims_of(*cfg);
    if (d.M > kMaxWalks) {
        set_error("%s: %d walks (num_neighbors %d ** walk_length %d) > %d not supported by the training path (the attention backward holds one key per lane)",
                  what, d.M, d.k, d.W, kMaxWalks);
        return DYGNN_E_UNSUPPORTED;
    }
    // every row count (NT = 2 batch T rows, their 4 H columns indexed with 64 bits) stays inside int for the products
    const int64_t lim = (INT32_MAX / 4) / d.T;
    DYGNN_REQUIRE(batch >= 0 && batch <= lim, "%s: batch must be in [0, %lld]", what, (long long)lim);
    return DYGNN_OK;
}

static unsigned blocks(int64_t n) { return (unsigned)ceil_div(n, 256); }

}  // namespace cawnt
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::cawnt;

extern "C" size_t dygnn_cawn_train_workspace_bytes(const dygnn_cawn_config* cfg, int64_t batch) {
    if (check_batch(cfg, batch, "cawn_train_workspace_bytes") != DYGNN_OK) return 0;
    return make_plan(*cfg, batch > 0 ? batch : 1).total;
}

extern "C" int dygnn_cawn_train_forward(const dygnn_cawn_config* cfg, const dygnn_cawn_weights* w, const float* node_feat, const float* edge_feat,
                                        const int64_t* side_root, const double* side_time, const dygnn_cawn_hops* hops, int64_t batch, float dropout_p,
                                        uint64_t seed, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = check_batch(cfg, batch, "cawn_train_forward")) return rc;
    if (batch == 0) return DYGNN_OK;
    if (int rc = check_weights(w, "cawn_train_forward: null weights")) return rc;
    DYGNN_REQUIRE(node_feat && edge_feat && side_root && side_time && hops && hops->id[0] && hops->eid[0] && hops->t[0] && out_src && out_dst && workspace,
                  "cawn_train_forward: null pointer");
    DYGNN_REQUIRE(cfg->walk_length == 1 || (hops->id[1] && hops->eid[1] && hops->t[1]), "cawn_train_forward: null pointer (hop 2 arrays)");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "cawn_train_forward: dropout must be in [0, 1)");
    const Plan p = make_plan(*cfg, batch);
    if (workspace_bytes < p.total) {
        set_error("cawn_train_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    const Dims& d = p.d;
    const Lay L{d.k, d.W, d.M, d.T, p.I};
    const int A = d.A, R = (int)p.R, NT = (int)p.NT, PR = (int)p.PR, W1 = d.W + 1;
    const Tree tr{side_root, hops->id[0], hops->id[1], hops->eid[0], hops->eid[1], side_time, hops->t[0], hops->t[1]};
    int64_t* rawid = reinterpret_cast<int64_t*>(ws + p.rawid);
    int32_t *valid = I32(p.valid), *pidx = I32(p.pidx);
    hipLaunchKernelGGL(k_cawnt_tree, dim3(blocks(p.NT)), dim3(256), 0, s, tr, L, batch, (int64_t)cfg->num_node_rows, (int64_t)cfg->num_edge_rows, rawid,
                       I32(p.nid), I32(p.eidc), F32(p.dtv), valid);
    DYGNN_LAUNCH_CHECK();
    // position features: counts, the MLP once per unique id of a pair
    DYGNN_HIP(hipMemsetAsync(F32(p.ct), 0, (size_t)PR * 6 * sizeof(float), s));
    hipLaunchKernelGGL(k_cawnt_pos, dim3((unsigned)batch), dim3(256), 0, s, rawid, L, pidx, F32(p.ct));
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cawnt_poshid, dim3(blocks((int64_t)PR * d.Pd)), dim3(256), 0, s, F32(p.ct), w->pos_w0, w->pos_b0, (int64_t)PR, d.Pd, W1, F32(p.hs));
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_cawnt_scale, dim3(blocks(d.Pd)), dim3(256), 0, s, w->pos_b1, d.Pd, 2.f, F32(p.b1x2));      // both rows carry the bias
    DYGNN_LAUNCH_CHECK();
    if (int rc = train::mm(s, F32(p.hs), d.Pd, false, w->pos_w1, d.Pd, true, F32(p.pf), d.Pd, PR, d.Pd, d.Pd, train::MmOpt().bias(F32(p.b1x2)))) return rc;
    hipLaunchKernelGGL(k_cawnt_gather, dim3(blocks(p.NT * d.D)), dim3(256), 0, s, node_feat, edge_feat, I32(p.nid), I32(p.eidc), F32(p.dtv), valid, pidx,
                       F32(p.pf), w->time_w, w->time_b, L, d.Fn, d.Ft, d.Fe, d.Pd, F32(p.x));
    DYGNN_LAUNCH_CHECK();
    // the two BiLSTMs on the tree
    for (int e = 0; e < 2; ++e) {
        const dygnn_cawn_lstm_weights* m = e == 0 ? w->feature : w->position;
        const int H = e == 0 ? d.Hf : d.Hp, in = e == 0 ? d.D : d.Pd;
        const float* Xin = F32(p.x) + (e == 0 ? 0 : d.D - d.Pd);
        float *G = F32(p.enc[e].G), *GR = F32(p.enc[e].GR), *hb = F32(p.enc[e].h), *cb = F32(p.enc[e].c);
        if (int rc = train::mm(s, Xin, d.D, false, m[0].w_ih, in, true, G, 4 * H, NT, 4 * H, in, train::MmOpt().bias(m[0].b_ih))) return rc;
        for (int lv = 0; lv <= d.W; ++lv) {
            const int64_t rows = p.I * L.n(lv);
            const float* HH = nullptr;
            if (lv > 0) {
                if (int rc = train::mm(s, hb + (size_t)L.base(lv - 1) * H, H, false, m[0].w_hh, H, true, F32(p.hh), 4 * H, (int)(p.I * L.n(lv - 1)), 4 * H, H))
                    return rc;
                HH = F32(p.hh);
            }
            hipLaunchKernelGGL(k_cawnt_cell, dim3(blocks(rows * H)), dim3(256), 0, s, G, HH, m[0].b_hh, valid, L.base(lv), lv > 0 ? L.base(lv - 1) : 0, rows,
                               d.k, H, hb, cb);
            DYGNN_LAUNCH_CHECK();
        }
        if (int rc = train::mm(s, Xin, d.D, false, m[1].w_ih, in, true, GR, 4 * H, NT, 4 * H, in, train::MmOpt().bias(m[1].b_ih))) return rc;
        hipLaunchKernelGGL(k_cawnt_cell, dim3(blocks(p.NT * H)), dim3(256), 0, s, GR, (const float*)nullptr, m[1].b_hh, valid, (int64_t)0, (int64_t)0, p.NT,
                           d.k, H, F32(p.enc[e].hr), (float*)nullptr);
        DYGNN_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_cawnt_encout, dim3(blocks(p.R * d.E)), dim3(256), 0, s, F32(p.enc[0].h), F32(p.enc[0].hr), F32(p.enc[1].h), F32(p.enc[1].hr), valid, L,
                       d.Hf, d.Hp, F32(p.eo));
    DYGNN_LAUNCH_CHECK();
    // projection_layers[0], the transformer block over the M walks of a sequence (sites 0 .. 3, every row draws as itself)
    const train::Drop dr = train::make_drop(dropout_p, seed);
    const float scale = 1.0f / sqrtf((float)(A / d.heads));
    if (int rc = train::mm(s, F32(p.eo), d.E, false, w->proj0_w, d.E, true, F32(p.x0), A, R, A, d.E, train::MmOpt().bias(w->proj0_b))) return rc;
    const train::BlockBufs v = bufs(p, ws);
    auto attn = [&]() -> int {
        const size_t lds_fwd = (size_t)3 * d.M * kLdh * sizeof(float);
        DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_cawnt_attn_fwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_fwd));
        hipLaunchKernelGGL(k_cawnt_attn_fwd, dim3((unsigned)p.I, (unsigned)d.heads), dim3(256), lds_fwd, s, v.qkv, d.M, A, d.heads, scale, dr, F32(p.P), v.O);
        DYGNN_LAUNCH_CHECK();
        return DYGNN_OK;
    };
    if (int rc = train::encoder_block_forward<kNV>(s, A, p.R, F32(p.x0), w->attn, dr, dropout_p, 0u, train::RowMap{d.M, 0}, v, attn)) return rc;
    // mean over the walks, projection_layers[1]: sequence 2 p -> out_src[p], 2 p + 1 -> out_dst[p] (rows of stride 2 A)
    hipLaunchKernelGGL(k_cawnt_mean, dim3(blocks(p.I * A)), dim3(256), 0, s, F32(p.y), p.I, d.M, A, F32(p.ym));
    DYGNN_LAUNCH_CHECK();
    if (int rc = train::mm(s, F32(p.ym), 2 * A, false, w->proj1_w, A, true, out_src, d.Fn, (int)batch, d.Fn, A, train::MmOpt().bias(w->proj1_b))) return rc;
    return train::mm(s, F32(p.ym) + A, 2 * A, false, w->proj1_w, A, true, out_dst, d.Fn, (int)batch, d.Fn, A, train::MmOpt().bias(w->proj1_b));
}

extern "C" int dygnn_cawn_backward(const dygnn_cawn_config* cfg, const dygnn_cawn_weights* w, const dygnn_cawn_weights* grads, const float* grad_out_src,
                                   const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed, void* workspace, size_t workspace_bytes,
                                   dygnn_stream_t stream) {
    if (int rc = check_batch(cfg, batch, "cawn_backward")) return rc;
    if (batch == 0) return DYGNN_OK;
    if (int rc = check_weights(w, "cawn_backward: null weights")) return rc;
    if (int rc = check_weights(grads, "cawn_backward: null gradient buffer")) return rc;
    DYGNN_REQUIRE(grad_out_src && grad_out_dst && workspace, "cawn_backward: null pointer");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "cawn_backward: dropout must be in [0, 1)");
    const Plan p = make_plan(*cfg, batch);
    if (workspace_bytes < p.total) {
        set_error("cawn_backward: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto G = [](const float* g) { return const_cast<float*>(g); };
    const Dims& d = p.d;
    const Lay L{d.k, d.W, d.M, d.T, p.I};
    const int A = d.A, R = (int)p.R, NT = (int)p.NT, PR = (int)p.PR, W1 = d.W + 1, B = (int)batch;
    const int32_t* valid = reinterpret_cast<const int32_t*>(ws + p.valid);
    const int32_t* pidx = reinterpret_cast<const int32_t*>(ws + p.pidx);
    const train::Drop dr = train::make_drop(dropout_p, seed);
    const float scale = 1.0f / sqrtf((float)(A / d.heads));
    float *gA = F32(p.gA), *part = F32(p.part);
    auto cs = [&](const float* Am, int cols, const float* out) { return colsum(s, Am, cols, p.R, cols, part, out); };

    // 1. projection_layers[1] and the mean over the walks
    float* dym = F32(p.dym);
    if (int rc = train::mm(s, grad_out_src, d.Fn, false, w->proj1_w, A, false, dym, 2 * A, B, A, d.Fn)) return rc;
    if (int rc = train::mm(s, grad_out_dst, d.Fn, false, w->proj1_w, A, false, dym + A, 2 * A, B, A, d.Fn)) return rc;
    if (int rc = train::mm(s, grad_out_src, d.Fn, true, F32(p.ym), 2 * A, false, G(grads->proj1_w), A, d.Fn, A, B, train::MmOpt().beta(1.f))) return rc;
    if (int rc = train::mm(s, grad_out_dst, d.Fn, true, F32(p.ym) + A, 2 * A, false, G(grads->proj1_w), A, d.Fn, A, B, train::MmOpt().beta(1.f))) return rc;
    if (int rc = colsum(s, grad_out_src, d.Fn, batch, d.Fn, part, G(grads->proj1_b))) return rc;
    if (int rc = colsum(s, grad_out_dst, d.Fn, batch, d.Fn, part, G(grads->proj1_b))) return rc;
    hipLaunchKernelGGL(k_cawnt_bcast, dim3(blocks(p.R * A)), dim3(256), 0, s, dym, p.R, d.M, A, gA);
    DYGNN_LAUNCH_CHECK();

    // 2. the transformer block
    {
        const train::BlockBufs v = bufs(p, ws);
        auto attn_bwd = [&]() -> int {
            const size_t lds_bwd = ((size_t)4 * d.M * kLdh + (size_t)2 * d.M * (d.M + 1)) * sizeof(float);
            DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_cawnt_attn_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bwd));
            hipLaunchKernelGGL(k_cawnt_attn_bwd, dim3((unsigned)p.I, (unsigned)d.heads), dim3(256), lds_bwd, s, v.qkv, F32(p.P), v.gF, d.M, A, d.heads, scale, dr,
                               v.dqkv);
            DYGNN_LAUNCH_CHECK();
            return DYGNN_OK;
        };
        if (int rc = train::encoder_block_backward<kNV>(s, A, p.R, F32(p.x0), w->attn, grads->attn, dr, 0u, train::RowMap{d.M, 0}, v, attn_bwd)) return rc;
    }

    // 3. projection_layers[0]: gA = d X0 -> d [feature forward | feature reverse | position forward | position reverse]
    float* deo = F32(p.deo);
    if (int rc = cs(gA, A, grads->proj0_b)) return rc;
    if (int rc = train::mm(s, gA, A, false, w->proj0_w, d.E, false, deo, d.E, R, d.E, A)) return rc;
    if (int rc = wgrad(s, R, gA, A, A, F32(p.eo), d.E, d.E, G(grads->proj0_w), d.E)) return rc;

    // 4. the BiLSTMs on the tree
    float *dxt = F32(p.dxt), *dxp = F32(p.dxp), *CH = F32(p.ch), *CC = F32(p.cc), *SG = F32(p.sg), *DHP = F32(p.dhp);
    bool dxp_set = false;
    for (int e = 0; e < 2; ++e) {
        const dygnn_cawn_lstm_weights* m = e == 0 ? w->feature : w->position;
        const dygnn_cawn_lstm_weights* g = e == 0 ? grads->feature : grads->position;
        const int H = e == 0 ? d.Hf : d.Hp, in = e == 0 ? d.D : d.Pd;
        const int col_fwd = e == 0 ? 0 : 2 * d.Hf, col_rev = col_fwd + H, pcol = in - d.Pd;      // the position columns of this encoder's input
        const float* Xin = F32(p.x) + (e == 0 ? 0 : d.D - d.Pd);
        float *Gf = F32(p.enc[e].G), *GR = F32(p.enc[e].GR), *hb = F32(p.enc[e].h), *cb = F32(p.enc[e].c);
        // the reverse cell: dW_ih, both biases, dx; weight_hh_l0_reverse keeps the caller's zeros
        hipLaunchKernelGGL(k_cawnt_rev_bwd, dim3(blocks(p.NT * H)), dim3(256), 0, s, GR, deo, d.E, col_rev, valid, L, H);
        DYGNN_LAUNCH_CHECK();
        // the forward direction, hop W down to step 0
        for (int lv = d.W; lv >= 0; --lv) {
            const int64_t rows = p.I * L.n(lv);
            hipLaunchKernelGGL(k_cawnt_cell_bwd, dim3(blocks(rows * H)), dim3(256), 0, s, Gf, cb, valid, deo, d.E, col_fwd, DHP, CH, CC, L.base(lv),
                               lv > 0 ? L.base(lv - 1) : 0, lv < d.W ? L.base(lv + 1) : 0, rows, d.k, H, lv == d.W ? 1 : 0, lv > 0 ? 1 : 0);
            DYGNN_LAUNCH_CHECK();
            if (lv == 0) break;
            const int64_t parents = p.I * L.n(lv - 1);
            hipLaunchKernelGGL(k_cawnt_child_sum, dim3(blocks(parents * 4 * H)), dim3(256), 0, s, Gf, L.base(lv), parents, d.k, 4 * H, SG);
            DYGNN_LAUNCH_CHECK();
            if (int rc = train::mm(s, SG, 4 * H, false, m[0].w_hh, H, false, DHP, H, (int)parents, H, 4 * H)) return rc;
            if (int rc = wgrad(s, (int)parents, SG, 4 * H, 4 * H, hb + (size_t)L.base(lv - 1) * H, H, H, G(g[0].w_hh), H)) return rc;
        }
        for (int dir = 0; dir < 2; ++dir) {
            const float* dG = dir == 0 ? Gf : GR;
            if (int rc = wgrad(s, NT, dG, 4 * H, 4 * H, Xin, d.D, in, G(g[dir].w_ih), in)) return rc;
            if (int rc = colsum(s, dG, 4 * H, p.NT, 4 * H, part, G(g[dir].b_ih), G(g[dir].b_hh))) return rc;
            // dx: node and edge features are constants, only the time and the position columns are computed
            if (e == 0)
                if (int rc = train::mm(s, dG, 4 * H, false, m[dir].w_ih + d.Fn, in, false, dxt, d.Ft, NT, d.Ft, 4 * H, train::MmOpt().beta(dir == 0 ? 0.f : 1.f))) return rc;
            if (int rc = train::mm(s, dG, 4 * H, false, m[dir].w_ih + pcol, in, false, dxp, d.Pd, NT, d.Pd, 4 * H, train::MmOpt().beta(dxp_set ? 1.f : 0.f))) return rc;
            dxp_set = true;
        }
    }

    // 5. the time encoder
    {
        double* tpart = reinterpret_cast<double*>(ws + p.tpart);
        if (int rc = train::time_grad(s, dxt, F32(p.dtv), w->time_w, w->time_b, p.NT, d.Ft, tpart, G(grads->time_w), G(grads->time_b))) return rc;
    }

    // 6. position features: the scatter onto the unique ids of a pair, then the MLP once per unique id
    float *dpf = F32(p.dpf), *dhs = F32(p.dhs), *dp = F32(p.dp);
    hipLaunchKernelGGL(k_cawnt_pos_scatter, dim3((unsigned)batch), dim3(256), 0, s, dxp, pidx, L, d.Pd, dpf);
    DYGNN_LAUNCH_CHECK();
    if (int rc = colsum(s, dpf, d.Pd, PR, d.Pd, part, G(grads->pos_b1))) return rc;            // both rows carry the bias: twice the sum
    if (int rc = colsum(s, dpf, d.Pd, PR, d.Pd, part, G(grads->pos_b1))) return rc;
    if (int rc = wgrad(s, PR, dpf, d.Pd, d.Pd, F32(p.hs), d.Pd, d.Pd, G(grads->pos_w1), d.Pd)) return rc;
    if (int rc = train::mm(s, dpf, d.Pd, false, w->pos_w1, d.Pd, false, dhs, d.Pd, PR, d.Pd, d.Pd)) return rc;
    hipLaunchKernelGGL(k_cawnt_mlp_bwd, dim3(blocks((int64_t)PR * d.Pd)), dim3(256), 0, s, F32(p.ct), w->pos_w0, w->pos_b0, dhs, (int64_t)PR, d.Pd, W1, dp);
    DYGNN_LAUNCH_CHECK();
    if (int rc = colsum(s, dp, d.Pd, 2 * (int64_t)PR, d.Pd, part, G(grads->pos_b0))) return rc;
    return train::mm(s, dp, d.Pd, true, F32(p.ct), 3, false, G(grads->pos_w0), W1, d.Pd, W1, 2 * PR, train::MmOpt().beta(1.f));
}
