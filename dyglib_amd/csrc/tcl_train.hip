// TCL training (models/TCL.py:56-154, TransformerEncoder models/modules.py:209-266): the forward of tcl.hip in TRAIN mode and its hand-written
// backward pass, so that train_link_prediction.py's two calls, MergeLayer + BCE, loss.backward() and Adam run on the HIP path.
//
// Layout.  A call works on n = 2 B sides [src ; dst], S = K + 1 positions each, token rows r = side * S + position (R = n S rows).  Pair p is
// (side p, side B + p): the partner of side s is s +- B, so there is no index vector, no host synchronisation, and every side's gradient
// has exactly ONE producer (no scatter-add of activation gradients).  A layer is two stages (0 = self, 1 = cross) over all n sides at once;
// the layer's 12 tensors collect gradient from both stages (four uses in the reference's terms: self a, self b, a <- b, b <- a).
//
// Saved per stage (workspace, read by the backward pass): the block input X [R][d] (the previous stage's output), q | k | v [R][3d] with bias
// (q unscaled), the softmax BEFORE dropout P [n][H][S][S] (the only [n, S, S] array outside LDS), the attention output O [R][d], the two
// pre-LayerNorm sums with mean and rstd, LayerNorm 0's output, and the post-ReLU, post-dropout hidden rows [R][4d] (STORED, not recomputed:
// they are the B operand of fc1's weight gradient, and their sign is the ReLU-and-dropout mask).  The sampled ids, edge ids and times are
// copied into the workspace; feature rows are regathered by the encoder's backward, not stored.  The last cross stage computes all S
// positions (a padded or unread position costs time, never correctness); its backward starts from a gradient at position 0 only.
//
// Dropout.  Masks are never stored: forward and backward redraw them from train::Drop (dropout.h).  Indexing, independent of which kernel
// draws:  site = 8 layer + 4 stage + {0: attention probabilities, 1: attention block output, 2: relu(fc0), 3: fc1 output};
//   the sequence index is the pair-sequence index q = 2 p + side (side 0 = source), also in the layer-0 self stage;
//   site 0 element ((q H + h) S + i) S + j;  sites 1, 3 element (q S + i) d + c;  site 2 element (q S + i) 4d + c;  i = position in the full
//   S-row layout.
//
// Kernels:  k_tclt_attn_fwd / k_tclt_attn_bwd  one (query sequence, head) per workgroup, tiles in LDS as in k_tcl_attn; the backward's four
//                                              products (dO V^T, dS K, dS^T Q, (P mask)^T dO) are fp32 MFMA on LDS tiles;
//           k_tclt_enc_rows                     the encoder's gathered operand rows;
//           shared (train_rows.h): train::k_res_ln<4> / k_res_ln_bwd<4>  residual + dropout + LayerNorm and its backward, one wave per row;
//                                  train::k_row_drop / k_hid_bwd         site-2 dropout and the ReLU-and-dropout mask of the hidden gradient;
//                                  train::k_time_part / k_time_fin       the time encoder's gradients, fixed-order fp64 column sums.
// A stage's launch sequence, forward and backward, is train::encoder_block_forward / _backward (encoder_block_train.h, shared with
// cawn_train.hip) with the row map {S, B} (side s draws as pair sequence 2 p + side) and the site base 8 layer + 4 stage.
// Dense products (in_proj, out_proj, fc0, fc1, their transposes, output_layer) go through train::mm (fp32 MFMA, gemm.h), the weight gradients
// of a stage through ONE train::dw_grouped launch, LayerNorm, bias and depth gradients through fixed-order two-stage column sums (train::colsum, colsum.h: one wave per column in the second stage).  Padded query positions are reachable only as masked keys (P = 0 exactly), so their gradient is exactly zero by construction.
#include "colsum.h"
#include "common.h"
#include "dropout.h"
#include "encoder_block_train.h"
#include "gemm.h"
#include "mfma_tile.h"
#include "tcl.h"
#include "time_encoding.h"

namespace dygnn {
namespace tclt {

using timeenc::cos_time;
using tile::f4;
using tile::mfma4;
using tile::round16;
using tile::z4;
using train::colsum;
using train::pair_seq;      // the dropout generator's sequence index of side s (train_rows.h)

constexpr int kMaxSeq = 64;
constexpr int kHeadChunk = 64;
constexpr int NV = 4;                 // columns per lane of a row (train_rows.h): d <= 256


// ---- attention forward of (query sequence s, head h) -------------------------------------------------------------------------------------
// k_tcl_attn on the interleaved q | k | v rows (stride 3d), one head per workgroup; keys / values and the key mask come from sequence s
// (self) or its partner (cross).  Saves the softmax P, multiplies the site-0 mask in, writes O.  LDS: Qc, Kc, Pm [64][65].
__global__ __launch_bounds__(256) void k_tclt_attn_fwd(const float* __restrict__ qkv, int64_t B, int cross, const int64_t* __restrict__ side_root,
                                                         const int64_t* __restrict__ nbr_id, int K, int d, int H, float scale, train::Drop dr, uint32_t site,
                                                         float* __restrict__ P, float* __restrict__ O) {
    constexpr int LD = kHeadChunk + 1;
    __shared__ float Qc[kMaxSeq * LD], Kc[kMaxSeq * LD], Pm[kMaxSeq * LD];
    __shared__ int s_valid[kMaxSeq];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = K + 1, dh = d / H, ld = 3 * d, h = blockIdx.y;
    const int64_t s = blockIdx.x, ks = cross ? (s < B ? s + B : s - B) : s, qi = pair_seq(s, B);
    if (threadIdx.x < kMaxSeq) {
        const int j = threadIdx.x;
        s_valid[j] = j < S && (j == 0 ? side_root[ks] : nbr_id[ks * K + j - 1]) != 0;
    }
    const float* q = qkv + (size_t)s * S * ld + h * dh;
    const float* k = qkv + (size_t)ks * S * ld + d + h * dh;
    const float* v = k + d;
    float sc[16];                                                    // scores of rows wave + 4 e, key = lane
#pragma unroll
    for (int e = 0; e < 16; ++e) sc[e] = 0.f;
    for (int c0 = 0; c0 < dh; c0 += kHeadChunk) {
        const int cn = dh - c0 < kHeadChunk ? dh - c0 : kHeadChunk;
        __syncthreads();                                             // s_valid written / the previous chunk has been read
        for (int x = threadIdx.x; x < kMaxSeq * cn; x += 256) {
            const int r = x / cn, cc = x - r * cn;
            Qc[r * LD + cc] = r < S ? q[(size_t)r * ld + c0 + cc] : 0.f;
            Kc[r * LD + cc] = r < S ? k[(size_t)r * ld + c0 + cc] : 0.f;
        }
        __syncthreads();
        for (int cc = 0; cc < cn; ++cc) {
            const float kk = Kc[lane * LD + cc];
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = wave + 4 * e;
                if (r < S) sc[e] = fmaf(Qc[r * LD + cc], kk, sc[e]);      // wave-uniform
            }
        }
    }
    const bool on = s_valid[lane] != 0;
    const uint32_t skey = dr.site_key(site);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = wave + 4 * e;
        if (r >= S) continue;
        const float sv = on ? sc[e] * scale : -INFINITY;
        const float m = wave_max(sv);
        const float ex = on ? expf(sv - m) : 0.f;
        const float sum = wave_sum(ex);
        const float p = sum > 0.f ? ex / sum : 0.f;
        float pd = 0.f;
        if (lane < S) {
            P[(((size_t)s * H + h) * S + r) * S + lane] = p;
            const uint64_t idx = (((uint64_t)qi * H + h) * S + r) * S + lane;
            pd = p * dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
        }
        Pm[r * LD + lane] = pd;
    }
    __syncthreads();
    float* o = O + (size_t)s * S * d + h * dh;
    for (int x = threadIdx.x; x < S * dh; x += 256) {
        const int r = x / dh, cc = x - r * dh;
        float a = 0.f;
        for (int j = 0; j < S; ++j) a = fmaf(Pm[r * LD + j], v[(size_t)j * ld + cc], a);
        o[(size_t)r * d + cc] = a;
    }
}

// One 16 x 16 tile of a product of two LDS operands of row stride kLd: acc += sum_k T(m0 + c, k) U(n0 + c, k) over k < Kp (a multiple of 16; both
// operands hold zeros, not stale bits, beyond their live part).  Lane (c, g) ends with out[m0 + c][n0 + 4 g .. 4 g + 3], as in tile::wave_product
// (U feeds the MFMA's A operand).  An operand stored k-contiguous ([row][k]) is read as one float4 per lane; one stored transposed ([k][row])
// as four floats, lanes (c, g) on banks c + 16 g: conflict-free either way.
constexpr int kLd = 68;
template <bool TT, bool UT>
__device__ __forceinline__ f4 lds_tile(const float* __restrict__ T, const float* __restrict__ U, int m0, int n0, int Kp, int lane, f4 acc) {
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    for (int k0 = 0; k0 < Kp; k0 += 16) {
        const int k = k0 + g4;
        f4 t, u;
        if (TT) t = f4{T[k * kLd + m0 + c], T[(k + 1) * kLd + m0 + c], T[(k + 2) * kLd + m0 + c], T[(k + 3) * kLd + m0 + c]};
        else t = *reinterpret_cast<const f4*>(T + (m0 + c) * kLd + k);
        if (UT) u = f4{U[k * kLd + n0 + c], U[(k + 1) * kLd + n0 + c], U[(k + 2) * kLd + n0 + c], U[(k + 3) * kLd + n0 + c]};
        else u = *reinterpret_cast<const f4*>(U + (n0 + c) * kLd + k);
        acc = mfma4(u.x, t.x, acc);
        acc = mfma4(u.y, t.y, acc);
        acc = mfma4(u.z, t.z, acc);
        acc = mfma4(u.w, t.w, acc);
    }
    return acc;
}
// rows 0 .. S-1, columns c0 .. c0 + cn - 1 of X (row stride ldx) into the LDS tile [64][kLd], zeros elsewhere in its [64][64] part
__device__ __forceinline__ void load_chunk(float* __restrict__ A, const float* __restrict__ X, int ldx, int S, int c0, int cn) {
    for (int x = threadIdx.x; x < kMaxSeq * kHeadChunk; x += 256) {
        const int r = x >> 6, cc = x & 63;
        A[r * kLd + cc] = (r < S && cc < cn) ? X[(size_t)r * ldx + c0 + cc] : 0.f;
    }
}
// a wave's tiles of an [Sp][np] product: out rows < S and columns < cn go to dst[row * ldd + col]
template <bool TT, bool UT>
__device__ __forceinline__ void product_out(const float* __restrict__ T, const float* __restrict__ U, int Sp, int np, int Kp, int S, int cn,
                                            float* __restrict__ dst, int ldd, int wave, int lane) {
    const int c = lane & 15, g4 = 4 * (lane >> 4), nts = np >> 4, tiles = (Sp >> 4) * nts;
    for (int tl = wave; tl < tiles; tl += 4) {
        const int mt = tl / nts, nt = tl - mt * nts;
        const f4 acc = lds_tile<TT, UT>(T, U, 16 * mt, 16 * nt, Kp, lane, z4());
        const int row = 16 * mt + c, col = 16 * nt + g4;
        if (row >= S) continue;
        float* o = dst + (size_t)row * ldd + col;
        if (col < cn) o[0] = acc.x;
        if (col + 1 < cn) o[1] = acc.y;
        if (col + 2 < cn) o[2] = acc.z;
        if (col + 3 < cn) o[3] = acc.w;
    }
}

// ---- attention backward of (query sequence s, head h), products as fp32 MFMA on LDS tiles ----------------------------------------------------
// dPd = dO V^T (accumulated over chunks of <= 64 head columns); dP = dPd * mask (site 0 redrawn); dS = scale P (dP - sum_j P dP) (a masked
// key has P = 0: dS = 0); then per chunk dQ = dS K -> the q columns of sequence s, dK = dS^T Q and dV = (P mask)^T dO -> the k / v columns of
// the KEY sequence (s or its partner: one producer per row).  LDS: three [64][68] tiles: dS, P mask, and the chunk in flight (phase 1: dO and
// V chunks in the first two).
__global__ __launch_bounds__(256) void k_tclt_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ P, const float* __restrict__ dO, int64_t B,
                                                         int cross, int K, int d, int H, float scale, train::Drop dr, uint32_t site,
                                                         float* __restrict__ dqkv) {
    __shared__ __attribute__((aligned(16))) float T0[kMaxSeq * kLd], T1[kMaxSeq * kLd], T2[kMaxSeq * kLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = K + 1, Sp = round16(S), dh = d / H, ld = 3 * d, h = blockIdx.y;
    const int64_t s = blockIdx.x, ks = cross ? (s < B ? s + B : s - B) : s, qi = pair_seq(s, B);
    const float* q = qkv + (size_t)s * S * ld + h * dh;
    const float* k = qkv + (size_t)ks * S * ld + d + h * dh;
    const float* v = k + d;
    const float* go = dO + (size_t)s * S * d + h * dh;
    const int c = lane & 15, g4 = 4 * (lane >> 4), mts = Sp >> 4;
    f4 acc[4];                                                       // dPd tiles wave + 4 e of the [mts][mts] grid
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = z4();
    for (int c0 = 0; c0 < dh; c0 += kHeadChunk) {
        const int cn = dh - c0 < kHeadChunk ? dh - c0 : kHeadChunk;
        __syncthreads();                                             // the previous chunk has been read
        load_chunk(T0, go, d, S, c0, cn);
        load_chunk(T1, v, ld, S, c0, cn);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int tl = wave + 4 * e;
            if (tl < mts * mts) acc[e] = lds_tile<false, false>(T0, T1, 16 * (tl / mts), 16 * (tl % mts), round16(cn), lane, acc[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int tl = wave + 4 * e;
        if (tl < mts * mts) *reinterpret_cast<f4*>(T2 + (16 * (tl / mts) + c) * kLd + 16 * (tl % mts) + g4) = acc[e];
    }
    __syncthreads();                                                 // dPd is in T2; the chunks in T0 / T1 have been read
    const uint32_t skey = dr.site_key(site);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int r = wave + 4 * e;
        float ds = 0.f, pd = 0.f;
        if (r < S) {                                                 // wave-uniform
            float p = 0.f, m = 0.f, dp = 0.f;
            if (lane < S) {
                p = P[(((size_t)s * H + h) * S + r) * S + lane];
                const uint64_t idx = (((uint64_t)qi * H + h) * S + r) * S + lane;
                m = dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
                dp = T2[r * kLd + lane] * m;
            }
            const float t = wave_sum(p * dp);
            ds = scale * (p * (dp - t));
            pd = p * m;
        }
        T0[r * kLd + lane] = ds;                                     // zeros beyond S in both directions: the products run over Sp
        T1[r * kLd + lane] = pd;
    }
    float* dq = dqkv + (size_t)s * S * ld + h * dh;
    float* dk = dqkv + (size_t)ks * S * ld + d + h * dh;
    for (int c0 = 0; c0 < dh; c0 += kHeadChunk) {
        const int cn = dh - c0 < kHeadChunk ? dh - c0 : kHeadChunk, np = round16(cn);
        __syncthreads();                                             // dS / P mask written, T2 (dPd or the previous chunk) has been read
        load_chunk(T2, k, ld, S, c0, cn);
        __syncthreads();
        product_out<false, true>(T0, T2, Sp, np, Sp, S, cn, dq + c0, ld, wave, lane);            // dQ[i][c] = sum_j dS[i][j] K[j][c]
        __syncthreads();
        load_chunk(T2, q, ld, S, c0, cn);
        __syncthreads();
        product_out<true, true>(T0, T2, Sp, np, Sp, S, cn, dk + c0, ld, wave, lane);             // dK[j][c] = sum_i dS[i][j] Q[i][c]
        __syncthreads();
        load_chunk(T2, go, d, S, c0, cn);
        __syncthreads();
        product_out<true, true>(T1, T2, Sp, np, Sp, S, cn, dk + d + c0, ld, wave, lane);         // dV[j][c] = sum_i (P mask)[i][j] dO[i][c]
    }
}

// ---- encoder backward operands: the rows the three projections read, regathered (k_tcl_encode's clamps and dt) -------------------------------
// One side per workgroup: NF [R][Fn], EF [R][Fe], TF [R][Ft] = cos(fma(dt, w, b)), DT [R].  The feature tables are the forward's, whose
// pointers wait in the workspace (the backward entry point does not take them).
__global__ void k_tclt_tabs(const float** tabs, const float* node_feat, const float* edge_feat) { tabs[0] = node_feat; tabs[1] = edge_feat; }
__global__ __launch_bounds__(256) void k_tclt_enc_rows(const float* const* __restrict__ tabs, const int64_t* __restrict__ side_root, const double* __restrict__ side_time,
                                                         const int64_t* __restrict__ nbr_id, const int64_t* __restrict__ nbr_eid,
                                                         const float* __restrict__ nbr_t, const float* __restrict__ tw, const float* __restrict__ tb, int K,
                                                         int Fn, int Fe, int Ft, int64_t node_rows, int64_t edge_rows, float* __restrict__ NF,
                                                         float* __restrict__ EF, float* __restrict__ TF, float* __restrict__ DT) {
    __shared__ int64_t s_id[kMaxSeq], s_eid[kMaxSeq];
    __shared__ float s_dt[kMaxSeq];
    const float* __restrict__ node_feat = tabs[0];
    const float* __restrict__ edge_feat = tabs[1];
    const int64_t q = blockIdx.x;
    const int S = K + 1;
    if (threadIdx.x < S) {
        const int j = threadIdx.x;
        int64_t id = 0, e = 0;
        float dt = 0.f;
        if (j == 0) id = side_root[q];
        else {
            const double t = side_time[q];
            id = nbr_id[q * K + j - 1];
            e = nbr_eid[q * K + j - 1];
            dt = (float)(t - (double)nbr_t[q * K + j - 1]);
        }
        s_id[j] = (id < 0 || id >= node_rows) ? 0 : id;
        s_eid[j] = (e < 0 || e >= edge_rows) ? 0 : e;
        s_dt[j] = dt;
        DT[q * S + j] = dt;
    }
    __syncthreads();
    const int W = Fn + Fe + Ft;
    for (int x = threadIdx.x; x < S * W; x += 256) {
        const int j = x / W, f = x - j * W;
        const size_t r = (size_t)q * S + j;
        if (f < Fn) NF[r * Fn + f] = node_feat[(size_t)s_id[j] * Fn + f];
        else if (f < Fn + Fe) EF[r * Fe + f - Fn] = edge_feat[(size_t)s_eid[j] * Fe + f - Fn];
        else {
            const int c = f - Fn - Fe;
            TF[r * Ft + c] = cos_time(fmaf(s_dt[j], tw[c], tb[c]));
        }
    }
}
// ---- workspace ------------------------------------------------------------------------------------------------------------------------------
struct Stage { size_t qkv, P, O, pre0, mean0, rstd0, y0, hid, pre1, mean1, rstd1, out; };
struct Plan {
    int K, S, d, Fe, Ft, H, L;
    int64_t n, R;
    size_t root, time, nid, neid, nt;                      // the call's sides (copied: the caller's arrays need not outlive the forward)
    size_t tabs;                                           // the forward's feature table pointers
    size_t x0;
    Stage st[2 * DYGNN_MAX_LAYERS];
    size_t tmp;                                            // forward scratch [R][d]
    size_t gA, gB, gC, gD, gE, gF, dhid, dqkv, part;       // backward scratch
    size_t nf, ef, tf, dtv, dtf, tpart;                    // encoder backward
    size_t total;
};

static Plan make_plan(const dygnn_tcl_config& c, int64_t B) {
    Plan p{};
    p.K = c.num_neighbors; p.S = p.K + 1; p.d = c.node_feat_dim; p.Fe = c.edge_feat_dim; p.Ft = c.time_feat_dim; p.H = c.num_heads; p.L = c.num_layers;
    p.n = 2 * B; p.R = p.n * p.S;
    const size_t n = (size_t)p.n, R = (size_t)p.R, d = (size_t)p.d;
    size_t o = 0;
    auto take = [&](size_t words) { size_t r = o; o += (words * 4 + 255) & ~size_t(255); return r; };      // 4-byte elements
    p.root = take(2 * n); p.time = take(2 * n); p.nid = take(2 * n * p.K); p.neid = take(2 * n * p.K); p.nt = take(n * p.K);
    p.tabs = take(4);
    p.x0 = take(R * d);
    for (int t = 0; t < 2 * p.L; ++t) {
        Stage& s = p.st[t];
        s.qkv = take(3 * R * d); s.P = take(n * p.H * p.S * p.S); s.O = take(R * d);
        s.pre0 = take(R * d); s.mean0 = take(R); s.rstd0 = take(R); s.y0 = take(R * d);
        s.hid = take(4 * R * d);
        s.pre1 = take(R * d); s.mean1 = take(R); s.rstd1 = take(R); s.out = take(R * d);
    }
    p.tmp = take(R * d);
    p.gA = take(R * d); p.gB = take(R * d); p.gC = take(R * d); p.gD = take(R * d); p.gE = take(R * d); p.gF = take(R * d);
    p.dhid = take(4 * R * d); p.dqkv = take(3 * R * d);
    int mx = 4 * p.d > p.Ft ? 4 * p.d : p.Ft;
    const size_t part_rows = (size_t)ceil_div(p.R, tgt::kColRows) * mx, part_depth = (size_t)ceil_div(p.n, tgt::kColRows) * p.S * d;
    p.part = take(part_rows > part_depth ? part_rows : part_depth);
    p.nf = take(R * d); p.ef = take(R * p.Fe); p.tf = take(R * p.Ft); p.dtv = take(R); p.dtf = take(R * p.Ft);
    p.tpart = take((size_t)ceil_div(p.R, tgt::kColRows) * 4 * p.Ft);      // [blocks][2][Ft] doubles
    p.total = o;
    return p;
}

// the block buffers of stage t (encoder_block_train.h)
static train::BlockBufs bufs(const Plan& p, char* ws, int t) {
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const Stage& v = p.st[t];
    return {F32(v.qkv), F32(v.O), F32(v.pre0), F32(v.mean0), F32(v.rstd0), F32(v.y0), F32(v.hid), F32(v.pre1), F32(v.mean1), F32(v.rstd1), F32(v.out),
            F32(p.tmp), F32(p.gA), F32(p.gB), F32(p.gC), F32(p.gD), F32(p.gE), F32(p.gF), F32(p.dhid), F32(p.dqkv), F32(p.part)};
}

static int check_weights(const dygnn_tcl_weights* w, int L, const char* what) {
    DYGNN_REQUIRE(w && w->time_w && w->time_b && w->depth_w && w->proj_node_w && w->proj_node_b && w->proj_edge_w && w->proj_edge_b && w->proj_time_w &&
                  w->proj_time_b && w->output_w && w->output_b, "%s", what);
    for (int l = 0; l < L; ++l) {
        const dygnn_tcl_layer_weights& m = w->layers[l];
        DYGNN_REQUIRE(m.in_proj_w && m.in_proj_b && m.out_proj_w && m.out_proj_b && m.fc0_w && m.fc0_b && m.fc1_w && m.fc1_b && m.norm0_w && m.norm0_b &&
                      m.norm1_w && m.norm1_b, "%s (layer %d)", what, l);
    }
    return DYGNN_OK;
}

static int check_batch(const dygnn_tcl_config* cfg, int64_t batch, const char* what) {
    if (int rc = tcl::check_tcl(cfg)) return rc;
    // R (1 + 4 d) elements are indexed with 64 bits everywhere; the bound keeps n and R inside int for the products' row counts
    DYGNN_REQUIRE(batch >= 0 && batch <= (INT32_MAX / 2) / (cfg->num_neighbors + 1), "%s: batch must be in [0, %d]", what,
                  (INT32_MAX / 2) / (cfg->num_neighbors + 1));
    return DYGNN_OK;
}

}  // namespace tclt
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::tclt;

extern "C" size_t dygnn_tcl_train_workspace_bytes(const dygnn_tcl_config* cfg, int64_t batch) {
    if (check_batch(cfg, batch, "tcl_train_workspace_bytes") != DYGNN_OK) return 0;
    return make_plan(*cfg, batch > 0 ? batch : 1).total;
}

extern "C" int dygnn_tcl_train_forward(const dygnn_tcl_config* cfg, const dygnn_tcl_weights* w, const float* node_feat, const float* edge_feat,
                                       const int64_t* side_root, const double* side_time, const int64_t* nbr_id, const int64_t* nbr_eid, const float* nbr_t,
                                       int64_t batch, float dropout_p, uint64_t seed, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes,
                                       dygnn_stream_t stream) {
    if (int rc = check_batch(cfg, batch, "tcl_train_forward")) return rc;
    if (batch == 0) return DYGNN_OK;
    if (int rc = check_weights(w, cfg->num_layers, "tcl_train_forward: null weights")) return rc;
    DYGNN_REQUIRE(node_feat && edge_feat && side_root && side_time && nbr_id && nbr_eid && nbr_t && out_src && out_dst && workspace,
                  "tcl_train_forward: null pointer");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "tcl_train_forward: dropout must be in [0, 1)");
    const Plan p = make_plan(*cfg, batch);
    if (workspace_bytes < p.total) {
        set_error("tcl_train_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int K = p.K, S = p.S, d = p.d, H = p.H;
    const int64_t n = p.n, B = batch;
    int64_t* root = reinterpret_cast<int64_t*>(ws + p.root);
    double* tms = reinterpret_cast<double*>(ws + p.time);
    int64_t* nid = reinterpret_cast<int64_t*>(ws + p.nid);
    int64_t* neid = reinterpret_cast<int64_t*>(ws + p.neid);
    float* nt = F32(p.nt);
    DYGNN_HIP(hipMemcpyAsync(root, side_root, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(tms, side_time, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(nid, nbr_id, (size_t)n * K * 8, hipMemcpyDeviceToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(neid, nbr_eid, (size_t)n * K * 8, hipMemcpyDeviceToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(nt, nbr_t, (size_t)n * K * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_tclt_tabs, dim3(1), dim3(1), 0, s, reinterpret_cast<const float**>(ws + p.tabs), node_feat, edge_feat);
    DYGNN_LAUNCH_CHECK();
    if (int rc = tcl::encode(s, *cfg, *w, node_feat, edge_feat, root, tms, nid, neid, nt, n, F32(p.x0))) return rc;
    const train::Drop dr = train::make_drop(dropout_p, seed);
    const float scale = 1.0f / sqrtf((float)(d / H));
    const float* X = F32(p.x0);
    for (int t = 0; t < 2 * p.L; ++t) {
        const train::BlockBufs v = bufs(p, ws, t);
        const uint32_t site = 8u * (uint32_t)(t / 2) + 4u * (uint32_t)(t & 1);
        float* P = F32(p.st[t].P);
        auto attn = [&]() -> int {
            hipLaunchKernelGGL(k_tclt_attn_fwd, dim3((unsigned)n, (unsigned)H), dim3(256), 0, s, v.qkv, B, t & 1, root, nid, K, d, H, scale, dr, site, P, v.O);
            DYGNN_LAUNCH_CHECK();
            return DYGNN_OK;
        };
        if (int rc = train::encoder_block_forward<NV>(s, d, p.R, X, w->layers[t / 2], dr, dropout_p, site, train::RowMap{S, B}, v, attn)) return rc;
        X = v.out;
    }
    // output_layer on position 0 of every sequence: rows of stride S d
    if (int rc = train::mm(s, X, S * d, false, w->output_w, d, true, out_src, d, (int)B, d, d, train::MmOpt().bias(w->output_b))) return rc;
    return train::mm(s, X + (size_t)B * S * d, S * d, false, w->output_w, d, true, out_dst, d, (int)B, d, d, train::MmOpt().bias(w->output_b));
}

extern "C" int dygnn_tcl_backward(const dygnn_tcl_config* cfg, const dygnn_tcl_weights* w, const dygnn_tcl_weights* grads, const float* grad_out_src,
                                  const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed, void* workspace, size_t workspace_bytes,
                                  dygnn_stream_t stream) {
    if (int rc = check_batch(cfg, batch, "tcl_backward")) return rc;
    if (batch == 0) return DYGNN_OK;
    if (int rc = check_weights(w, cfg->num_layers, "tcl_backward: null weights")) return rc;
    if (int rc = check_weights(grads, cfg->num_layers, "tcl_backward: null gradient buffer")) return rc;
    DYGNN_REQUIRE(grad_out_src && grad_out_dst && workspace, "tcl_backward: null pointer");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "tcl_backward: dropout must be in [0, 1)");
    const Plan p = make_plan(*cfg, batch);
    if (workspace_bytes < p.total) {
        set_error("tcl_backward: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total);
        return DYGNN_E_WORKSPACE;
    }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto G = [](const float* g) { return const_cast<float*>(g); };
    const int K = p.K, S = p.S, d = p.d, H = p.H, R = (int)p.R, Fe = p.Fe, Ft = p.Ft;
    const int64_t n = p.n, B = batch;
    const train::Drop dr = train::make_drop(dropout_p, seed);
    const float scale = 1.0f / sqrtf((float)(d / H));
    float *gA = F32(p.gA), *part = F32(p.part);
    auto cs = [&](const float* A, int cols, const float* out) { return colsum(s, A, cols, p.R, cols, part, out); };

    // output_layer: the gradient enters at position 0 of every sequence, every other row starts at zero
    const float* Z = F32(p.st[2 * p.L - 1].out);
    DYGNN_HIP(hipMemsetAsync(gA, 0, (size_t)p.R * d * sizeof(float), s));
    if (int rc = train::mm(s, grad_out_src, d, false, w->output_w, d, false, gA, S * d, (int)B, d, d)) return rc;
    if (int rc = train::mm(s, grad_out_dst, d, false, w->output_w, d, false, gA + (size_t)B * S * d, S * d, (int)B, d, d)) return rc;
    {
        const train::DwPair pairs[2] = {{grad_out_src, d, d, Z, S * d, d, G(grads->output_w), d, nullptr},
                                        {grad_out_dst, d, d, Z + (size_t)B * S * d, S * d, d, G(grads->output_w), d, nullptr}};
        if (int rc = train::dw_grouped(s, (int)B, pairs, 2)) return rc;
        if (int rc = colsum(s, grad_out_src, d, B, d, part, G(grads->output_b))) return rc;
        if (int rc = colsum(s, grad_out_dst, d, B, d, part, G(grads->output_b))) return rc;
    }
    for (int t = 2 * p.L - 1; t >= 0; --t) {
        const train::BlockBufs v = bufs(p, ws, t);
        const float* X = t == 0 ? F32(p.x0) : F32(p.st[t - 1].out);
        const uint32_t site = 8u * (uint32_t)(t / 2) + 4u * (uint32_t)(t & 1);
        const float* P = F32(p.st[t].P);
        auto attn_bwd = [&]() -> int {
            hipLaunchKernelGGL(k_tclt_attn_bwd, dim3((unsigned)n, (unsigned)H), dim3(256), 0, s, v.qkv, P, v.gF, B, t & 1, K, d, H, scale, dr, site, v.dqkv);
            DYGNN_LAUNCH_CHECK();
            return DYGNN_OK;
        };
        // both stages of a layer add into the same 12 tensors
        if (int rc = train::encoder_block_backward<NV>(s, d, p.R, X, w->layers[t / 2], grads->layers[t / 2], dr, site, train::RowMap{S, B}, v, attn_bwd))
            return rc;
    }
    // encoder: gA = d X0.  Biases and the depth embedding are column sums of it; the projections' operand rows are regathered
    float *NF = F32(p.nf), *EF = F32(p.ef), *TF = F32(p.tf), *DT = F32(p.dtv), *dtf = F32(p.dtf);
    double* tpart = reinterpret_cast<double*>(ws + p.tpart);
    if (int rc = cs(gA, d, grads->proj_node_b)) return rc;
    if (int rc = cs(gA, d, grads->proj_edge_b)) return rc;
    if (int rc = cs(gA, d, grads->proj_time_b)) return rc;
    if (int rc = colsum(s, gA, S * d, n, S * d, part, G(grads->depth_w))) return rc;
    hipLaunchKernelGGL(k_tclt_enc_rows, dim3((unsigned)n), dim3(256), 0, s, reinterpret_cast<const float* const*>(ws + p.tabs),
                       reinterpret_cast<const int64_t*>(ws + p.root), reinterpret_cast<const double*>(ws + p.time),
                       reinterpret_cast<const int64_t*>(ws + p.nid), reinterpret_cast<const int64_t*>(ws + p.neid), F32(p.nt), w->time_w, w->time_b, K, d, Fe,
                       Ft, (int64_t)cfg->num_node_rows, (int64_t)cfg->num_edge_rows, NF, EF, TF, DT);
    DYGNN_LAUNCH_CHECK();
    if (int rc = train::mm(s, gA, d, false, w->proj_time_w, Ft, false, dtf, Ft, R, Ft, d)) return rc;
    if (int rc = train::time_grad(s, dtf, DT, w->time_w, w->time_b, p.R, Ft, tpart, G(grads->time_w), G(grads->time_b))) return rc;
    const train::DwPair pairs[3] = {{gA, d, d, NF, d, d, G(grads->proj_node_w), d, nullptr},
                                    {gA, d, d, EF, Fe, Fe, G(grads->proj_edge_w), Fe, nullptr},
                                    {gA, d, d, TF, Ft, Ft, G(grads->proj_time_w), Ft, nullptr}};
    return train::dw_grouped(s, R, pairs, 3);
}
