// Training path of the DyGFormer hot path: a forward that keeps what the backward pass needs and the
// backward pass itself, so train_link_prediction.py:229-257 (forward, loss.backward(), optimizer.step()) runs on hand-written
// HIP kernels.  models/DyGFormer.py:68-194 and :418-461 in train mode: dropout on the attention probabilities
// (nn.MultiheadAttention(dropout=...), :429), on the attention output and on the FFN (:456-460).
//
// Design: activations live in HBM (dense [B*T][.] rows, T = tokens per pair of THIS call), every product goes through the
// library's general fp32-MFMA GEMM (train::mm, gemm.hip: any transposition, strided batches for the per-(pair, head) attention products), the
// rest is row-wise / element-wise kernels.  Dropout masks are not stored: both passes draw them from a counter-based hash of
// (seed, site, element).  Gradients are produced for every parameter; the feature tables get none (the reference keeps
// them as constants, models/DyGFormer.py:28-29).
// This is the first, unfused version (correctness + a working training loop); inference uses dygformer_fused3.hip; the fused training
// kernels this file dispatches to are in dygformer_fused3_train.hip (forward) and dygformer_fused3_bwd.hip (backward).
#include <cstdlib>
#include "dygformer_layout.h"
#include "dygformer_rows.h"
#include "gemm.h"
#include "time_encoding.h"
#include "train_elements.h"

namespace dygnn {

namespace train {

using f4 = __attribute__((ext_vector_type(4))) float;

// ---- LayerNorm rows (eps 1e-5, biased variance; models/DyGFormer.py:438-439) ---------------------------------------
__global__ __launch_bounds__(256) void k_ln_fwd(const float* __restrict__ X, const float* __restrict__ gamma, const float* __restrict__ beta, int64_t M,
                                                  int D, float* __restrict__ Y, float* __restrict__ mean_o, float* __restrict__ rstd_o) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float mean, rstd;
    rows::layernorm_row(X + row * D, gamma, beta, D, lane, Y + row * D, mean, rstd);
    if (lane == 0) { mean_o[row] = mean; rstd_o[row] = rstd; }
}
// dX[row] += LN'(dY) ; dgamma += sum dY*xhat ; dbeta += sum dY.  A lane owns columns lane, lane+64, ...: its partial sums over the
// 16 rows of its wave stay in registers, the four waves meet in LDS, one global atomic per column and workgroup.  D <= 256.
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ mean_i,
                                                  const float* __restrict__ rstd_i, const float* __restrict__ gamma, int64_t M, int D,
                                                  float* __restrict__ dX, float* __restrict__ dgamma, float* __restrict__ dbeta) {
    extern __shared__ float part[];            // [4 waves][2][D]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pg[4] = {0.f, 0.f, 0.f, 0.f}, pb[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int RB = 4;                      // rows of one wave in flight together: their loads and reductions overlap
    for (int rr = 0; rr < 16; rr += RB) {      // 64 rows per workgroup, 16 per wave
        float xh[RB][4], dy[RB][4], s1[RB], s2[RB], rstd[RB];
        int64_t row[RB];
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            row[u] = (int64_t)blockIdx.x * 64 + (rr + u) * 4 + wave;
            const bool on = row[u] < M;
            const float mean = on ? mean_i[row[u]] : 0.f;
            rstd[u] = on ? rstd_i[row[u]] : 0.f;
            s1[u] = 0.f; s2[u] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = lane + 64 * q;
                xh[u][q] = 0.f; dy[u][q] = 0.f;
                if (on && k < D) {
                    xh[u][q] = (X[row[u] * D + k] - mean) * rstd[u]; dy[u][q] = dY[row[u] * D + k];
                    const float gy = dy[u][q] * gamma[k];
                    s1[u] += gy; s2[u] = fmaf(gy, xh[u][q], s2[u]);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < RB; ++u) { s1[u] += __shfl_xor(s1[u], o, 64); s2[u] += __shfl_xor(s2[u], o, 64); }
#pragma unroll
        for (int u = 0; u < RB; ++u) {
            if (row[u] >= M) continue;
            const float m1 = s1[u] / (float)D, m2 = s2[u] / (float)D;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = lane + 64 * q;
                if (k < D) {
                    dX[row[u] * D + k] += rstd[u] * (dy[u][q] * gamma[k] - m1 - xh[u][q] * m2);
                    pg[q] = fmaf(dy[u][q], xh[u][q], pg[q]); pb[q] += dy[u][q];
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int k = lane + 64 * q;
        if (k < D) { part[(wave * 2 + 0) * D + k] = pg[q]; part[(wave * 2 + 1) * D + k] = pb[q]; }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 2 * D; k += 256) {
        const int which = k / D, col = k % D;
        const float t = (part[(0 * 2 + which) * D + col] + part[(1 * 2 + which) * D + col]) + (part[(2 * 2 + which) * D + col] + part[(3 * 2 + which) * D + col]);
        atomicAdd(which ? &dbeta[col] : &dgamma[col], t);
    }
}

// ---- softmax over the keys of one (pair, head, query) row + dropout on the probabilities ---------------------------
__global__ __launch_bounds__(256) void k_softmax_fwd(const float* __restrict__ S, int64_t rows, int T, Drop dr, uint32_t site,
                                                       float* __restrict__ P, float* __restrict__ Pd) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = S + row * T;
    float mx = -INFINITY;
    for (int j = lane; j < T; j += 64) mx = fmaxf(mx, s[j]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int j = lane; j < T; j += 64) sum += expf(s[j] - mx);
    const float inv = 1.0f / wave_sum(sum);
    for (int j = lane; j < T; j += 64) {
        const float pv = expf(s[j] - mx) * inv;
        P[row * T + j] = pv;
        Pd[row * T + j] = pv * dr.mask(site, (uint64_t)row * T + j);
    }
}
// dS = P o (dP - sum_j dP_j P_j), dP = dPd * mask      (in place: dPd -> dS)
__global__ __launch_bounds__(256) void k_softmax_bwd(float* __restrict__ dPd, const float* __restrict__ P, int64_t rows, int T, Drop dr, uint32_t site) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    float dot = 0.f;
    for (int j = lane; j < T; j += 64) dot = fmaf(dPd[row * T + j] * dr.mask(site, (uint64_t)row * T + j), P[row * T + j], dot);
    dot = wave_sum(dot);
    for (int j = lane; j < T; j += 64) {
        const float dp = dPd[row * T + j] * dr.mask(site, (uint64_t)row * T + j);
        dPd[row * T + j] = P[row * T + j] * (dp - dot);
    }
}

// ---- embedding inputs: windows, co-occurrence counts, patch matrices -----------------------------------------------------
struct EmbedArgs {
    const int64_t* indptr; const int32_t* nbr; const int32_t* eid; const double* ts;
    const int64_t *src, *dst; const double* times; const int32_t* hist_len; const int64_t* end_pos;
    const float *node_feat, *edge_feat, *time_w, *time_b, *lut;
    int64_t B; int Ss, Sd, Ts, T, P, L, Fn, Fe, Ft, C;
    int32_t *ids, *c0, *c1; float* dts;          // meta [B][S]
    float *Pn, *Pe, *Pt, *Pc;                    // patch matrices [B*T][P*F]
    int64_t num_nodes;                           // rows of the CSR: query ids outside [0, num_nodes) are the padding node
};
__global__ __launch_bounds__(256) void k_embed_inputs(const EmbedArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = a.Ss + a.Sd;
    int32_t* ids = reinterpret_cast<int32_t*>(smem);
    int32_t* eids = ids + S;
    float* dts = reinterpret_cast<float*>(eids + S);
    int32_t* c0 = reinterpret_cast<int32_t*>(dts + S);
    int32_t* c1 = c0 + S;
    const int64_t b = blockIdx.x;
    rows::fill_windows(rows::Csr{a.nbr, a.eid, a.ts, a.num_nodes}, a.src, a.dst, a.times, a.hist_len, a.end_pos, a.B, b, a.Ss, a.Sd, a.L, ids, eids, dts, c0, c1);
    if (blockIdx.y == 0)                                    // the meta arrays the backward pass reads
        for (int p = threadIdx.x; p < S; p += 256) { a.ids[b * S + p] = ids[p]; a.dts[b * S + p] = dts[p]; a.c0[b * S + p] = c0[p]; a.c1[b * S + p] = c1[p]; }
    // the patch matrices: the workgroups (b, 0 .. gridDim.y-1) of a pair share its tokens (each rebuilt the 128-position window
    // above, which is cheap); node / edge rows move as float4 where a table row is whole float4s (F % 4 == 0: every address is then 16-byte
    // aligned and no float4 crosses a row), element by element otherwise
    const int tok0 = (int)((int64_t)a.T * blockIdx.y / gridDim.y), ntok = (int)((int64_t)a.T * (blockIdx.y + 1) / gridDim.y) - tok0;
    const int Kn = a.P * a.Fn, Ke = a.P * a.Fe, Kt = a.P * a.Ft, Kc = a.P * a.C;
    const int Kn4 = (a.Fn & 3) ? 0 : Kn >> 2, Ke4 = (a.Fe & 3) ? 0 : Ke >> 2, KV = Kn4 + Ke4, KS = Kt + Kc;
    const int Kn1 = (a.Fn & 3) ? Kn : 0, K1 = Kn1 + ((a.Fe & 3) ? Ke : 0);
    for (int idx = threadIdx.x; idx < ntok * K1; idx += 256) {
        const int tok = tok0 + idx / K1;
        int k = idx % K1;
        const int p0 = tok < a.Ts ? tok * a.P : a.Ss + (tok - a.Ts) * a.P;
        const int64_t row = b * a.T + tok;
        if (k < Kn1) { a.Pn[row * Kn + k] = a.node_feat[(size_t)ids[p0 + k / a.Fn] * a.Fn + k % a.Fn]; continue; }
        k -= Kn1;
        a.Pe[row * Ke + k] = a.edge_feat[(size_t)eids[p0 + k / a.Fe] * a.Fe + k % a.Fe];
    }
    for (int idx = threadIdx.x; idx < ntok * KV; idx += 256) {
        const int tok = tok0 + idx / KV, k4 = idx % KV;
        const int p0 = tok < a.Ts ? tok * a.P : a.Ss + (tok - a.Ts) * a.P;
        const int64_t row = b * a.T + tok;
        if (k4 < Kn4) {
            const int k = 4 * k4, pp = p0 + k / a.Fn;
            *reinterpret_cast<f4*>(a.Pn + row * Kn + k) = *reinterpret_cast<const f4*>(a.node_feat + (size_t)ids[pp] * a.Fn + k % a.Fn);
        } else {
            const int k = 4 * (k4 - Kn4), pp = p0 + k / a.Fe;
            *reinterpret_cast<f4*>(a.Pe + row * Ke + k) = *reinterpret_cast<const f4*>(a.edge_feat + (size_t)eids[pp] * a.Fe + k % a.Fe);
        }
    }
    for (int idx = threadIdx.x; idx < ntok * KS; idx += 256) {
        const int tok = tok0 + idx / KS;
        int k = idx % KS;
        const int p0 = tok < a.Ts ? tok * a.P : a.Ss + (tok - a.Ts) * a.P;
        const int64_t row = b * a.T + tok;
        if (k < Kt) {
            const int pp = p0 + k / a.Ft, f = k % a.Ft;
            a.Pt[row * Kt + k] = rows::time_feature(ids[pp], dts[pp], a.time_w, a.time_b, f);
            continue;
        }
        k -= Kt;
        { const int pp = p0 + k / a.C, f = k % a.C; a.Pc[row * Kc + k] = rows::cooc_feature(a.lut, a.C, c0[pp], c1[pp], f); }
    }
}
// time-encoder gradients from dPt [M][P*Ft]: pre = w dt + b, d cos = -sin(pre).  One workgroup per pair, thread = column k = pp * Ft + f of
// the pair's rows (coalesced), its sums over the T tokens in registers; the P columns of a feature meet in LDS, one atomic per feature.
__global__ __launch_bounds__(256) void k_time_bwd(const float* __restrict__ dPt, const int32_t* __restrict__ ids, const float* __restrict__ dts,
                                                    const float* __restrict__ tw, const float* __restrict__ tb, int64_t B, int Ss, int Sd, int Ts, int T,
                                                    int P, int Ft, float* __restrict__ dw, float* __restrict__ db) {
    extern __shared__ float part[];            // [2][Ft]
    for (int k = threadIdx.x; k < 2 * Ft; k += 256) part[k] = 0.f;
    __syncthreads();
    const int S = Ss + Sd, Kt = P * Ft;
    const int64_t b = blockIdx.x;
    for (int k = threadIdx.x; k < Kt; k += 256) {
        const int pp = k / Ft, f = k - pp * Ft;
        const float w = tw[f], bb = tb[f];
        float gw = 0.f, gb = 0.f;
        for (int tok = 0; tok < T; ++tok) {
            const int pos = (tok < Ts ? tok * P : Ss + (tok - Ts) * P) + pp;
            if (ids[b * S + pos] == 0) continue;
            const float dt = dts[b * S + pos];
            const float gsin = -timeenc::sin_time(fmaf(dt, w, bb)) * dPt[(b * T + tok) * Kt + k];
            gw = fmaf(gsin, dt, gw); gb += gsin;
        }
        atomicAdd(&part[f], gw);
        atomicAdd(&part[Ft + f], gb);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < Ft; k += 256) { atomicAdd(&dw[k], part[k]); atomicAdd(&db[k], part[Ft + k]); }
}
// dlut[count][j] += dPc over both count channels (feature = lut[c0] + lut[c1], DyGFormer.py:409-411).
// One workgroup handles kPairsPerWg pairs.  Thread (grp, j) owns column j of its own LDS copy [grp][count < 16][C] and walks
// every 5th (token, position) of the pair, so the hot counts (0, 1, 2, ...) are summed without atomics; the five copies are
// then folded into the global table with one atomic per (count, column) and workgroup.  Counts >= 16 go straight to global.
constexpr int kCoocRows = 16, kCoocGroups = 5, kPairsPerWg = 1;      // one pair per workgroup: the walk is a chain of load latencies, so what pays is more workgroups
__global__ __launch_bounds__(256) void k_cooc_bwd(const float* __restrict__ dPc, const int32_t* __restrict__ c0, const int32_t* __restrict__ c1, int64_t B,
                                                    int Ss, int Sd, int Ts, int T, int P, int C, float* __restrict__ dlut) {
    extern __shared__ float acc[];             // [5][16][C]
    const int S = Ss + Sd, Kc = P * C;
    for (int i = threadIdx.x; i < kCoocGroups * kCoocRows * C; i += 256) acc[i] = 0.f;
    __syncthreads();
    const int grp = threadIdx.x / C, j = threadIdx.x % C;
    if (grp < kCoocGroups) {
        float* mine = acc + (size_t)grp * kCoocRows * C;
        for (int64_t b = (int64_t)blockIdx.x * kPairsPerWg; b < B && b < (int64_t)(blockIdx.x + 1) * kPairsPerWg; ++b) {
            for (int q = grp; q < T * P; q += kCoocGroups) {          // q = token * P + position inside the patch
                const int tok = q / P, pin = q - tok * P;
                const int pp = (tok < Ts ? tok * P : Ss + (tok - Ts) * P) + pin;
                const float gv = dPc[(b * T + tok) * Kc + pin * C + j];
                const int32_t a0 = c0[b * S + pp], a1 = c1[b * S + pp];
                if (a0 < kCoocRows) mine[a0 * C + j] += gv; else atomicAdd(&dlut[(size_t)a0 * C + j], gv);
                if (a1 < kCoocRows) mine[a1 * C + j] += gv; else atomicAdd(&dlut[(size_t)a1 * C + j], gv);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kCoocRows * C; i += 256) {
        float t = 0.f;
#pragma unroll
        for (int gq = 0; gq < kCoocGroups; ++gq) t += acc[(size_t)gq * kCoocRows * C + i];
        if (t != 0.f) atomicAdd(&dlut[i], t);
    }
}
// gradients of the co-occurrence MLP from dlut: dh[c][k] = (hid[c][k] > 0) sum_j w1[j][k] dlut[c][j]  (one workgroup per count)
__global__ void k_lut_bwd_hidden(const float* __restrict__ dlut, const float* __restrict__ hid, const float* __restrict__ w1, int C, float* __restrict__ dh) {
    const int c = blockIdx.x;
    for (int k = threadIdx.x; k < C; k += blockDim.x) {
        float v = 0.f;
        if (hid[c * C + k] > 0.f)
            for (int j = 0; j < C; ++j) v = fmaf(w1[j * C + k], dlut[c * C + j], v);
        dh[c * C + k] = v;
    }
}
// dw1[j][k] = sum_c dlut[c][j] hid[c][k] ; db1[j] = sum_c dlut[c][j] ; dw0[k] = sum_c dh[c][k] * c ; db0[k] = sum_c dh[c][k]
// (three [rows][C] tables, rows <= 2 Smax + 1: staged in LDS once per workgroup, the sums then run from LDS instead of as chains of global loads)
constexpr int kLutChunk = 128;                 // table rows staged per pass
__global__ __launch_bounds__(256) void k_lut_bwd(const float* __restrict__ dlut, const float* __restrict__ hid, const float* __restrict__ dh, int rows, int C,
                                                   float* __restrict__ dw0, float* __restrict__ db0, float* __restrict__ dw1, float* __restrict__ db1) {
    extern __shared__ float lsm[];             // dlut | hid | dh, each [kLutChunk][C]
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int nmax = kLutChunk * C;
    const float *sl = lsm, *sh = lsm + nmax, *sd = lsm + 2 * nmax;
    float acc = 0.f, acc2 = 0.f;
    for (int r0 = 0; r0 < rows; r0 += kLutChunk) {
        const int nr = rows - r0 < kLutChunk ? rows - r0 : kLutChunk, n = nr * C;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += 256) { lsm[i] = dlut[r0 * C + i]; lsm[nmax + i] = hid[r0 * C + i]; lsm[2 * nmax + i] = dh[r0 * C + i]; }
        __syncthreads();
        if (idx < C * C) {
            const int j = idx / C, k = idx % C;
            for (int c = 0; c < nr; ++c) acc = fmaf(sl[c * C + j], sh[c * C + k], acc);
        } else if (idx < C * C + C) {
            const int j = idx - C * C;
            for (int c = 0; c < nr; ++c) acc += sl[c * C + j];
        } else if (idx < C * C + 2 * C) {
            const int k = idx - C * C - C;
            for (int c = 0; c < nr; ++c) { const float v = sd[c * C + k]; acc = fmaf(v, (float)(r0 + c), acc); acc2 += v; }
        }
    }
    if (idx < C * C) dw1[idx] = acc;
    else if (idx < C * C + C) db1[idx - C * C] = acc;
    else if (idx < C * C + 2 * C) { dw0[idx - C * C - C] = acc; db0[idx - C * C - C] = acc2; }
}

// pooled[side][b][:] = mean over the side's tokens (DyGFormer.py:181-187)
__global__ __launch_bounds__(256) void k_pool_fwd(const float* __restrict__ X, int64_t B, int Ts, int T, int D, float* __restrict__ pooled) {
    const int64_t b = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * D; i += 256) {
        const int side = i / D, n = i % D;
        const int t0 = side ? Ts : 0, t1 = side ? T : Ts;
        float s = 0.f;
        for (int t = t0; t < t1; ++t) s += X[(b * T + t) * D + n];
        pooled[((int64_t)side * B + b) * D + n] = s / (float)(t1 - t0);
    }
}
__global__ void k_pool_bwd(const float* __restrict__ dpooled, int64_t B, int Ts, int T, int D, float* __restrict__ dX) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * T * D) return;
    const int n = (int)(i % D);
    const int64_t row = i / D, b = row / T;
    const int t = (int)(row % T);
    const int side = t >= Ts;
    dX[i] = dpooled[((int64_t)side * B + b) * D + n] / (float)(side ? T - Ts : Ts);
}

// dX0 [M][4 C] -> four channel blocks [4][M][Cp], Cp = round_up(C, 4), zeros behind C: every block is then a 16-byte-aligned operand of the
// grouped weight-gradient launch (projection weights) and of the LDS-DMA GEMM (time / co-occurrence encoder inputs)
__global__ void k_split_channels(const float* __restrict__ dX, int64_t M, int C, int Cp, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 4 * M * Cp) return;
    const int j = (int)(i % Cp);
    const int64_t row = (i / Cp) % M;
    const int ch = (int)(i / ((int64_t)Cp * M));
    out[i] = j < C ? dX[row * (4 * C) + ch * C + j] : 0.f;
}

// ---- workspace -----------------------------------------------------------------------------------------------------------
struct Plan {
    WorkspaceLayout wl;       // prefix compatible with window_lengths_device (dims, hist_len, end_pos)
    size_t ids, dts, c0, c1, lut, hid, Pn, Pe, Pt, Pc, X[DYGNN_MAX_LAYERS + 1];
    struct L { size_t xn0, m0, r0, qkv, S, P, Pd, oa, ao, x1, xn1, m1, r1, hpre, hact, f2, dF2, dH, dAo, dQKV; } layer[DYGNN_MAX_LAYERS];
    size_t pooled, out, dX, dA, dB, dXc, dpool, dPt, dPc, dlut, total;
};
static Plan make_plan(const Dims& d, int64_t B) {
    Plan p{};
    p.wl = make_workspace_layout(d, B);
    size_t o = (p.wl.end_pos + (size_t)2 * B * sizeof(int64_t) + 255) & ~size_t(255);
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~size_t(255); return r; };
    const size_t S = 2 * (size_t)d.Smax, M = (size_t)B * d.Tmax, F = sizeof(float);
    p.ids = take(B * S * 4); p.dts = take(B * S * 4); p.c0 = take(B * S * 4); p.c1 = take(B * S * 4);
    p.lut = take((size_t)(S + 1) * d.C * F); p.hid = take((size_t)(S + 1) * d.C * F);
    p.Pn = take(M * d.P * d.Fn * F); p.Pe = take(M * d.P * d.Fe * F); p.Pt = take(M * d.P * d.Ft * F); p.Pc = take(M * d.P * d.C * F);
    for (int l = 0; l <= d.NL; ++l) p.X[l] = take(M * d.D * F);
    for (int l = 0; l < d.NL; ++l) {
        auto& L = p.layer[l];
        L.xn0 = take(M * d.D * F); L.m0 = take(M * F); L.r0 = take(M * F); L.qkv = take(M * 3 * d.D * F);
        L.S = take((size_t)B * d.H * d.Tmax * d.Tmax * F); L.P = take((size_t)B * d.H * d.Tmax * d.Tmax * F); L.Pd = take((size_t)B * d.H * d.Tmax * d.Tmax * F);
        L.oa = take(M * d.D * F); L.ao = take(M * d.D * F); L.x1 = take(M * d.D * F); L.xn1 = take(M * d.D * F); L.m1 = take(M * F); L.r1 = take(M * F);
        L.hpre = take(M * 4 * d.D * F); L.hact = take(M * 4 * d.D * F); L.f2 = take(M * d.D * F);
    }
    p.pooled = take((size_t)2 * B * d.D * F); p.out = take((size_t)2 * B * d.Fn * F);
    p.dX = take(M * d.D * F); p.dA = take(M * d.D * F); p.dB = take(M * d.D * F); p.dXc = take(4 * M * ((d.C + 3) & ~3) * F);
    // operands of the weight gradients stay alive until the ONE grouped launch at the end of the backward pass (k_dw_grouped): per layer
    for (int l = 0; l < d.NL; ++l) {
        auto& L = p.layer[l];
        L.dF2 = take(M * d.D * F); L.dH = take(M * 4 * d.D * F); L.dAo = take(M * d.D * F); L.dQKV = take(M * 3 * d.D * F);
    }
    // dPc [M][P C] = B S rows of C; the backward pass reuses it for dh [S + 1][C], which is one row more when B = 1
    p.dpool = take((size_t)2 * B * d.D * F); p.dPt = take(M * d.P * d.Ft * F); p.dPc = take((M * d.P > S + 1 ? M * d.P : S + 1) * d.C * F); p.dlut = take((size_t)(S + 1) * d.C * F);
    p.total = o;
    return p;
}

static int supported(const Dims& d) {
    if (d.C <= 0 || d.H <= 0 || d.D % d.H != 0) { set_error("train: bad dims"); return DYGNN_E_INVALID; }
    if (d.D > 256) { set_error("train: model dim > 256 not supported"); return DYGNN_E_UNSUPPORTED; }
    if (d.C * kCoocGroups > 256) { set_error("train: channel_embedding_dim > 51 not supported"); return DYGNN_E_UNSUPPORTED; }
    if ((size_t)5 * 2 * d.Smax * 4 > 60 * 1024) { set_error("train: max_input_sequence_length too large for the embedding kernel"); return DYGNN_E_UNSUPPORTED; }
    return DYGNN_OK;
}

#define EW(kernel, n, ...)                                                                                          \
    do {                                                                                                            \
        hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div((int64_t)(n), 256)), dim3(256), 0, s, __VA_ARGS__);      \
        DYGNN_LAUNCH_CHECK();                                                                                       \
    } while (0)

// ---- one call -----------------------------------------------------------------------------------------------------------
// What both entry points derive from their arguments: the sizes, the plan and the typed view of the workspace.
struct Call {
    Dims d;
    Plan p;
    char* ws;
    hipStream_t s;
    Drop dr;
    int64_t B, M;                  // pairs; token rows M = B * T
    int Ss, Sd, S, Ts, T;          // this call's padded lengths (set_lengths)
    float scale;                   // 1 / sqrt(head dim)
    float* F32(size_t off) const { return reinterpret_cast<float*>(ws + off); }
    int32_t* I32(size_t off) const { return reinterpret_cast<int32_t*>(ws + off); }
    void set_lengths(int ss, int sd) { Ss = ss; Sd = sd; S = ss + sd; Ts = ss / d.P; T = S / d.P; M = B * T; }
};
// config -> Dims, or why this path refuses it
static int train_dims(const dygnn_dygformer_config* cfg, Dims& d) {
    if (int rc = check_config(cfg)) return rc;
    d = make_dims(*cfg);
    return supported(d);
}
static int make_call(const Dims& d, int64_t batch, float dropout_p, uint64_t seed, void* workspace, size_t workspace_bytes, dygnn_stream_t stream,
                     const char* who, Call& c) {
    c.d = d;
    c.p = make_plan(d, batch);
    if (workspace_bytes < c.p.total) { set_error("%s: workspace too small (%zu < %zu bytes)", who, workspace_bytes, c.p.total); return DYGNN_E_WORKSPACE; }
    c.ws = static_cast<char*>(workspace);
    c.s = as_stream(stream);
    c.dr = make_drop(dropout_p, seed);
    c.B = batch;
    c.scale = (float)sqrt(1.0 / (double)d.hd);
    return DYGNN_OK;
}

// Which blocks of this call run as fused kernels (dygformer_fused3_train.hip, dygformer_fused3_bwd.hip).  `packed` = the kernel-ready copy of the
// CURRENT weights (dygnn_dygformer_pack / dygnn_dygformer_repack; it holds the backward fragment streams too).  NULL, DYGNN_TRAIN_UNFUSED (read on
// every call) or a shape the fused kernels do not take: the product-by-product path.
struct Path { bool forward, ffn_bwd, attn_bwd; };
static Path choose_path(const Call& c, const void* packed) {
    const uint64_t M = (uint64_t)c.M, BH = (uint64_t)c.B * c.d.H, T = (uint64_t)c.T;
    Path p;
    p.ffn_bwd = packed != nullptr && fused3_supported(c.d) && M * 4 * c.d.D < (1ull << 32) && !getenv("DYGNN_TRAIN_UNFUSED");
    p.forward = p.ffn_bwd && BH * T * T < (1ull << 32);
    p.attn_bwd = p.ffn_bwd && c.T <= 128 && c.d.H == 2;
    return p;
}

// ---- forward ------------------------------------------------------------------------------------------------------------
// the co-occurrence table of this step's weights, then the windows' meta arrays and the four patch matrices (both paths)
static int embed_inputs(const Call& c, const dygnn_dygformer_weights* w, const dygnn_csr* csr, const float* node_feat, const float* edge_feat,
                        const int64_t* src, const int64_t* dst, const double* times) {
    const Dims& d = c.d;
    const Plan& p = c.p;
    hipStream_t s = c.s;
    if (int rc = cooc_table_device(w, c.S + 1, d.C, c.F32(p.lut), c.F32(p.hid), s)) return rc;
    EmbedArgs ea{csr->indptr, csr->nbr, csr->eid, csr->ts, src, dst, times, reinterpret_cast<const int32_t*>(c.ws + p.wl.hist_len),
                 reinterpret_cast<const int64_t*>(c.ws + p.wl.end_pos), node_feat, edge_feat, w->time_w, w->time_b, c.F32(p.lut), c.B, c.Ss, c.Sd, c.Ts, c.T, d.P,
                 d.L, d.Fn, d.Fe, d.Ft, d.C, c.I32(p.ids), c.I32(p.c0), c.I32(p.c1), c.F32(p.dts), c.F32(p.Pn), c.F32(p.Pe), c.F32(p.Pt), c.F32(p.Pc), csr->num_nodes};
    hipLaunchKernelGGL(k_embed_inputs, dim3((unsigned)c.B, (unsigned)(c.T >= 8 ? 8 : 1)), dim3(256), (size_t)5 * c.S * 4, s, ea);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
// The fused forward (dygformer_fused3_train.hip, TR = true): one kernel from the windows to the embeddings that also writes every activation
// the backward pass reads into this Plan's buffers.
static int forward_fused(const Call& c, const dygnn_dygformer_weights* w, const void* packed, const dygnn_csr* csr, const float* node_feat,
                         const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times, float* out_src, float* out_dst) {
    const Plan& p = c.p;
    TrainOut tr{};
    for (int l = 0; l <= c.d.NL; ++l) tr.X[l] = c.F32(p.X[l]);
    for (int l = 0; l < c.d.NL; ++l) {
        const auto& L = p.layer[l];
        tr.layer[l] = TrainOut::L{c.F32(L.xn0), c.F32(L.m0), c.F32(L.r0), c.F32(L.qkv), c.F32(L.P), c.F32(L.Pd), c.F32(L.oa), c.F32(L.x1), c.F32(L.xn1),
                                  c.F32(L.m1), c.F32(L.r1), c.F32(L.hpre), c.F32(L.hact)};
    }
    tr.pooled = c.F32(p.pooled);
    tr.dr = c.dr;
    return forward_fused3_train(c.d, make_packed_layout(c.d), w, static_cast<const float*>(packed), csr, node_feat, edge_feat, src, dst, times, c.B,
                                c.F32(p.lut), out_src, out_dst, c.ws, p.wl, tr, c.s);
}
// encoder layer l, product by product (DyGFormer.py:418-461): X[l] -> X[l + 1], every intermediate kept
static int layer_forward_unfused(const Call& c, const dygnn_encoder_layer_weights& Lw, int l) {
    const auto& L = c.p.layer[l];
    hipStream_t s = c.s;
    const int64_t B = c.B, M = c.M;
    const int D = c.d.D, H = c.d.H, hd = c.d.hd, T = c.T;
    const Drop& dr = c.dr;
    auto F32 = [&](size_t off) { return c.F32(off); };
    const float* Xin = F32(c.p.X[l]);
    hipLaunchKernelGGL(k_ln_fwd, dim3((unsigned)ceil_div(M, 4)), dim3(256), 0, s, Xin, Lw.norm0_weight, Lw.norm0_bias, M, D, F32(L.xn0), F32(L.m0), F32(L.r0));
    DYGNN_LAUNCH_CHECK();
    if (int rc = mm(s, F32(L.xn0), D, false, Lw.in_proj_weight, D, true, F32(L.qkv), 3 * D, (int)M, 3 * D, D, MmOpt().bias(Lw.in_proj_bias))) return rc;
    // S_bh = scale * Q_bh K_bh^T ; batch z = b*H + h
    if (int rc = mm(s, F32(L.qkv), 3 * D, false, F32(L.qkv) + D, 3 * D, true, F32(L.S), T, T, T, hd,
                    MmOpt().alpha(c.scale).batched((int)(B * H), H).strideA((int64_t)T * 3 * D, hd).strideB((int64_t)T * 3 * D, hd).strideC((int64_t)H * T * T, (int64_t)T * T))) return rc;
    hipLaunchKernelGGL(k_softmax_fwd, dim3((unsigned)ceil_div(B * H * T, 4)), dim3(256), 0, s, F32(L.S), B * H * T, T, dr, (uint32_t)(4 * l + 0), F32(L.P), F32(L.Pd));
    DYGNN_LAUNCH_CHECK();
    // Oa_bh = Pd_bh V_bh
    if (int rc = mm(s, F32(L.Pd), T, false, F32(L.qkv) + 2 * D, 3 * D, false, F32(L.oa), D, T, hd, T,
                    MmOpt().batched((int)(B * H), H).strideA((int64_t)H * T * T, (int64_t)T * T).strideB((int64_t)T * 3 * D, hd).strideC((int64_t)T * D, hd))) return rc;
    if (int rc = mm(s, F32(L.oa), D, false, Lw.out_proj_weight, D, true, F32(L.ao), D, (int)M, D, D, MmOpt().bias(Lw.out_proj_bias))) return rc;
    EW(k_drop_add, M * D, Xin, F32(L.ao), M * D, dr, (uint32_t)(4 * l + 1), F32(L.x1));                                             // DyGFormer.py:456
    hipLaunchKernelGGL(k_ln_fwd, dim3((unsigned)ceil_div(M, 4)), dim3(256), 0, s, F32(L.x1), Lw.norm1_weight, Lw.norm1_bias, M, D, F32(L.xn1), F32(L.m1), F32(L.r1));
    DYGNN_LAUNCH_CHECK();
    if (int rc = mm(s, F32(L.xn1), D, false, Lw.ffn0_weight, D, true, F32(L.hpre), 4 * D, (int)M, 4 * D, D, MmOpt().bias(Lw.ffn0_bias))) return rc;
    EW(k_gelu_drop, M * 4 * D, F32(L.hpre), M * 4 * D, dr, (uint32_t)(4 * l + 2), F32(L.hact));                                     // :458
    if (int rc = mm(s, F32(L.hact), 4 * D, false, Lw.ffn1_weight, 4 * D, true, F32(L.f2), D, (int)M, D, 4 * D, MmOpt().bias(Lw.ffn1_bias))) return rc;
    EW(k_drop_add, M * D, F32(L.x1), F32(L.f2), M * D, dr, (uint32_t)(4 * l + 3), F32(c.p.X[l + 1]));                               // :460
    return DYGNN_OK;
}
// the whole forward, product by product: patch projections, the encoder layers, per-side token means, output layer
static int forward_unfused(const Call& c, const dygnn_dygformer_weights* w, float* out_src, float* out_dst) {
    const Dims& d = c.d;
    const Plan& p = c.p;
    hipStream_t s = c.s;
    const int64_t B = c.B, M = c.M;
    const int D = d.D, C = d.C;
    // projections (DyGFormer.py:148-157): X0[:, 50ch : 50ch+50] = P_ch . W_ch^T + b_ch
    const float* PW[4] = {w->proj_node_w, w->proj_edge_w, w->proj_time_w, w->proj_cooc_w};
    const float* PB[4] = {w->proj_node_b, w->proj_edge_b, w->proj_time_b, w->proj_cooc_b};
    const size_t PM[4] = {p.Pn, p.Pe, p.Pt, p.Pc};
    const int PK[4] = {d.P * d.Fn, d.P * d.Fe, d.P * d.Ft, d.P * C};
    for (int ch = 0; ch < 4; ++ch)
        if (int rc = mm(s, c.F32(PM[ch]), PK[ch], false, PW[ch], PK[ch], true, c.F32(p.X[0]) + ch * C, D, (int)M, C, PK[ch], MmOpt().bias(PB[ch]))) return rc;
    for (int l = 0; l < d.NL; ++l)
        if (int rc = layer_forward_unfused(c, w->layers[l], l)) return rc;
    hipLaunchKernelGGL(k_pool_fwd, dim3((unsigned)B), dim3(256), 0, s, c.F32(p.X[d.NL]), B, c.Ts, c.T, D, c.F32(p.pooled));
    DYGNN_LAUNCH_CHECK();
    if (int rc = mm(s, c.F32(p.pooled), D, false, w->output_w, D, true, out_src, d.Fn, (int)B, d.Fn, D, MmOpt().bias(w->output_b))) return rc;
    return mm(s, c.F32(p.pooled) + B * D, D, false, w->output_w, D, true, out_dst, d.Fn, (int)B, d.Fn, D, MmOpt().bias(w->output_b));
}

// ---- backward -----------------------------------------------------------------------------------------------------------
// the grads struct reuses the weights layout; its buffers are written
static float* G(const float* q) { return const_cast<float*>(q); }

// Layer l's four weight gradients take their operands from these buffers in the ONE grouped launch at the end of the pass
struct LayerGrads { float *dF2, *dH, *dAo, *dQKV; };       // [M][D], [M][4D], [M][D], [M][3D]

// X_{l+1} = X1 + drop(F2), F2 = Hact W2^T + b2, product by product: dF2, dHpre written for the grouped launch, dX <- dX1 in place
static int ffn_backward_unfused(const Call& c, const dygnn_encoder_layer_weights& Lw, const dygnn_encoder_layer_weights& Lg, int l, float* dX, const LayerGrads& g) {
    const auto& L = c.p.layer[l];
    hipStream_t s = c.s;
    const int64_t M = c.M;
    const int D = c.d.D;
    float* dBf = c.F32(c.p.dB);     // [M][D] scratch
    EW(k_drop_bwd, M * D, dX, M * D, c.dr, (uint32_t)(4 * l + 3), g.dF2);                                                     // dF2
    if (int rc = mm(s, g.dF2, D, false, Lw.ffn1_weight, 4 * D, false, g.dH, 4 * D, (int)M, 4 * D, D)) return rc;               // dHact
    EW(k_gelu_drop_bwd, M * 4 * D, g.dH, c.F32(L.hpre), M * 4 * D, c.dr, (uint32_t)(4 * l + 2));                              // dHpre
    if (int rc = mm(s, g.dH, 4 * D, false, Lw.ffn0_weight, D, false, dBf, D, (int)M, D, 4 * D)) return rc;                     // dxn1
    hipLaunchKernelGGL(k_ln_bwd, dim3((unsigned)ceil_div(M, 64)), dim3(256), 8 * D * sizeof(float), s, dBf, c.F32(L.x1), c.F32(L.m1), c.F32(L.r1), Lw.norm1_weight, M, D,
                       dX, G(Lg.norm1_weight), G(Lg.norm1_bias));                                                             // dX is now dX1
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
// X1 = Xin + drop(Ao), Ao = Oa Wo^T + bo ; Oa_bh = Pd_bh V_bh ; S_bh = scale Q_bh K_bh^T ; [Q | K | V] = LN0(Xin) Win^T + bin, product by product:
// dAo, dQKV written for the grouped launch, dX <- dX_l in place
static int attn_backward_unfused(const Call& c, const dygnn_encoder_layer_weights& Lw, const dygnn_encoder_layer_weights& Lg, int l, float* dX, const LayerGrads& g) {
    const auto& L = c.p.layer[l];
    hipStream_t s = c.s;
    const int64_t B = c.B, M = c.M;
    const int D = c.d.D, H = c.d.H, hd = c.d.hd, T = c.T;
    auto F32 = [&](size_t off) { return c.F32(off); };
    float *dA = F32(c.p.dA), *dBf = F32(c.p.dB);      // [M][D] scratch
    float* dQKV = g.dQKV;
    EW(k_drop_bwd, M * D, dX, M * D, c.dr, (uint32_t)(4 * l + 1), g.dAo);                                                     // dAo
    if (int rc = mm(s, g.dAo, D, false, Lw.out_proj_weight, D, false, dBf, D, (int)M, D, D)) return rc;                        // dOa
    // dV_bh = Pd^T dOa_bh
    if (int rc = mm(s, F32(L.Pd), T, true, dBf, D, false, dQKV + 2 * D, 3 * D, T, hd, T,
                    MmOpt().batched((int)(B * H), H).strideA((int64_t)H * T * T, (int64_t)T * T).strideB((int64_t)T * D, hd).strideC((int64_t)T * 3 * D, hd))) return rc;
    // dPd_bh = dOa_bh V_bh^T  (into the S buffer)
    if (int rc = mm(s, dBf, D, false, F32(L.qkv) + 2 * D, 3 * D, true, F32(L.S), T, T, T, hd,
                    MmOpt().batched((int)(B * H), H).strideA((int64_t)T * D, hd).strideB((int64_t)T * 3 * D, hd).strideC((int64_t)H * T * T, (int64_t)T * T))) return rc;
    hipLaunchKernelGGL(k_softmax_bwd, dim3((unsigned)ceil_div(B * H * T, 4)), dim3(256), 0, s, F32(L.S), F32(L.P), B * H * T, T, c.dr, (uint32_t)(4 * l + 0));
    DYGNN_LAUNCH_CHECK();
    // dQ_bh = scale dS K_bh ; dK_bh = scale dS^T Q_bh
    if (int rc = mm(s, F32(L.S), T, false, F32(L.qkv) + D, 3 * D, false, dQKV, 3 * D, T, hd, T,
                    MmOpt().alpha(c.scale).batched((int)(B * H), H).strideA((int64_t)H * T * T, (int64_t)T * T).strideB((int64_t)T * 3 * D, hd).strideC((int64_t)T * 3 * D, hd))) return rc;
    if (int rc = mm(s, F32(L.S), T, true, F32(L.qkv), 3 * D, false, dQKV + D, 3 * D, T, hd, T,
                    MmOpt().alpha(c.scale).batched((int)(B * H), H).strideA((int64_t)H * T * T, (int64_t)T * T).strideB((int64_t)T * 3 * D, hd).strideC((int64_t)T * 3 * D, hd))) return rc;
    if (int rc = mm(s, dQKV, 3 * D, false, Lw.in_proj_weight, D, false, dA, D, (int)M, D, 3 * D)) return rc;                   // dxn0
    hipLaunchKernelGGL(k_ln_bwd, dim3((unsigned)ceil_div(M, 64)), dim3(256), 8 * D * sizeof(float), s, dA, F32(c.p.X[l]), F32(L.m0), F32(L.r0), Lw.norm0_weight, M, D,
                       dX, G(Lg.norm0_weight), G(Lg.norm0_bias));                                                             // dX is now dX_l
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
// From dX = dX0 down to the parameters below the encoder: the grouped weight-gradient launch (`dw` holds the layers' problems already), the
// projections, the time encoder and the co-occurrence encoder.
static int inputs_backward(const Call& c, const dygnn_dygformer_weights* w, const dygnn_dygformer_weights* grads, float* dX, DwList& dw) {
    const Dims& d = c.d;
    const Plan& p = c.p;
    hipStream_t s = c.s;
    const int64_t B = c.B, M = c.M;
    const int D = d.D, C = d.C, S = c.S;
    auto F32 = [&](size_t off) { return c.F32(off); };
    // projections: X0[:, ch] = P_ch W_ch^T + b_ch.  dX0 is split into channel blocks (aligned operands); the four projection weight gradients
    // join the grouped launch where their shapes allow, the rest takes the general path
    const float* PW[4] = {w->proj_node_w, w->proj_edge_w, w->proj_time_w, w->proj_cooc_w};
    float* GW[4] = {G(grads->proj_node_w), G(grads->proj_edge_w), G(grads->proj_time_w), G(grads->proj_cooc_w)};
    float* GB[4] = {G(grads->proj_node_b), G(grads->proj_edge_b), G(grads->proj_time_b), G(grads->proj_cooc_b)};
    const size_t PM[4] = {p.Pn, p.Pe, p.Pt, p.Pc};
    const int PK[4] = {d.P * d.Fn, d.P * d.Fe, d.P * d.Ft, d.P * C};
    const int Cp = (C + 3) & ~3;
    float* dXc = F32(p.dXc);
    EW(k_split_channels, 4 * M * Cp, dX, M, C, Cp, dXc);
    bool grouped[4];
    for (int ch = 0; ch < 4; ++ch) grouped[ch] = dw.try_add(dXc + (size_t)ch * M * Cp, Cp, C, F32(PM[ch]), PK[ch], PK[ch], GW[ch], PK[ch], GB[ch]);
    // every weight gradient of the encoder layers and projections (and its bias gradient) in one grouped split-K launch
    if (!dw.ok) { set_error("backward: weight-gradient operands are not 16-byte aligned / too many problems"); return DYGNN_E_UNSUPPORTED; }
    if (int rc = dw.launch(s, (int)M)) return rc;
    for (int ch = 0; ch < 4; ++ch) {
        if (grouped[ch]) continue;
        if (int rc = mm(s, dX + ch * C, D, true, F32(PM[ch]), PK[ch], false, GW[ch], PK[ch], C, PK[ch], (int)M, MmOpt().c_is_zero().colsum(GB[ch]))) return rc;     // dW_ch [C][K]
    }
    // time encoder
    if (int rc = mm(s, dXc + (size_t)2 * M * Cp, Cp, false, PW[2], PK[2], false, F32(p.dPt), PK[2], (int)M, PK[2], C, MmOpt().a_kpad())) return rc;
    hipLaunchKernelGGL(k_time_bwd, dim3((unsigned)B), dim3(256), 2 * d.Ft * sizeof(float), s, F32(p.dPt), c.I32(p.ids), F32(p.dts), w->time_w, w->time_b, B, c.Ss, c.Sd,
                       c.Ts, c.T, d.P, d.Ft, G(grads->time_w), G(grads->time_b));
    DYGNN_LAUNCH_CHECK();
    // co-occurrence encoder
    if (int rc = mm(s, dXc + (size_t)3 * M * Cp, Cp, false, PW[3], PK[3], false, F32(p.dPc), PK[3], (int)M, PK[3], C, MmOpt().a_kpad())) return rc;
    DYGNN_HIP(hipMemsetAsync(F32(p.dlut), 0, (size_t)(S + 1) * C * sizeof(float), s));
    hipLaunchKernelGGL(k_cooc_bwd, dim3((unsigned)ceil_div(B, kPairsPerWg)), dim3(256), (size_t)kCoocGroups * kCoocRows * C * sizeof(float), s, F32(p.dPc),
                       c.I32(p.c0), c.I32(p.c1), B, c.Ss, c.Sd, c.Ts, c.T, d.P, C, F32(p.dlut));
    DYGNN_LAUNCH_CHECK();
    float* dh = F32(p.dPc);        // dPc is dead now: reuse its head for dh [S+1][C]
    hipLaunchKernelGGL(k_lut_bwd_hidden, dim3((unsigned)(S + 1)), dim3(64), 0, s, F32(p.dlut), F32(p.hid), w->cooc_w1, C, dh);
    DYGNN_LAUNCH_CHECK();
    DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lut_bwd), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(k_lut_bwd, dim3((unsigned)ceil_div(C * C + 2 * C, 256)), dim3(256), (size_t)3 * kLutChunk * C * sizeof(float), s, F32(p.dlut), F32(p.hid), dh, S + 1, C, G(grads->cooc_w0),
                       G(grads->cooc_b0), G(grads->cooc_w1), G(grads->cooc_b1));
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace train
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::train;

extern "C" size_t dygnn_dygformer_train_workspace_bytes(const dygnn_dygformer_config* cfg, int64_t batch) {
    if (check_config(cfg) != DYGNN_OK || batch < 0) return 0;
    const Dims d = make_dims(*cfg);
    if (supported(d) != DYGNN_OK) return 0;
    return make_plan(d, batch).total;
}

extern "C" int dygnn_dygformer_train_forward(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, const dygnn_csr* csr,
                                             const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst,
                                             const double* times, int64_t batch, float dropout_p, uint64_t seed, float* out_src, float* out_dst,
                                             void* workspace, size_t workspace_bytes, int32_t* seq_lens_host, const void* packed, dygnn_stream_t stream) {
    Dims d;
    if (int rc = train_dims(cfg, d)) return rc;
    DYGNN_REQUIRE(w && csr && csr->indptr && node_feat && edge_feat, "train_forward: null pointer");
    DYGNN_REQUIRE(batch > 0 && src && dst && times && out_src && out_dst && workspace && seq_lens_host, "train_forward: bad arguments");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "train_forward: dropout must be in [0, 1)");
    Call c;
    if (int rc = make_call(d, batch, dropout_p, seed, workspace, workspace_bytes, stream, "train_forward", c)) return rc;
    if (int rc = window_lengths_device(d, csr, src, dst, times, c.B, c.B, c.ws, c.p.wl, c.s)) return rc;
    // the padded lengths size every product below.  seq_lens_host = {0, 0}: read them back here (one host synchronisation of this
    // stream); non-zero: the caller already knows them (e.g. from dygnn_window_lengths on a side stream) and the call stays asynchronous
    if (seq_lens_host[0] <= 0 || seq_lens_host[1] <= 0) {
        CallDims cd;
        DYGNN_HIP(hipMemcpyAsync(&cd, c.ws + c.p.wl.dims, sizeof(CallDims), hipMemcpyDeviceToHost, c.s));
        DYGNN_HIP(hipStreamSynchronize(c.s));
        seq_lens_host[0] = cd.S_s; seq_lens_host[1] = cd.S_d;
    }
    const int Ss = seq_lens_host[0], Sd = seq_lens_host[1];
    DYGNN_REQUIRE(Ss % d.P == 0 && Sd % d.P == 0 && Ss <= d.Smax && Sd <= d.Smax, "train_forward: bad sequence lengths");
    c.set_lengths(Ss, Sd);
    if (int rc = embed_inputs(c, w, csr, node_feat, edge_feat, src, dst, times)) return rc;
    if (choose_path(c, packed).forward) return forward_fused(c, w, packed, csr, node_feat, edge_feat, src, dst, times, out_src, out_dst);
    return forward_unfused(c, w, out_src, out_dst);
}

extern "C" int dygnn_dygformer_backward(const dygnn_dygformer_config* cfg, const dygnn_dygformer_weights* w, const dygnn_dygformer_weights* grads,
                                        const float* grad_out_src, const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed,
                                        const int32_t* seq_lens_host, void* workspace, size_t workspace_bytes, const void* packed, dygnn_stream_t stream) {
    Dims d;
    if (int rc = train_dims(cfg, d)) return rc;
    DYGNN_REQUIRE(w && grads && grad_out_src && grad_out_dst && workspace && seq_lens_host && batch > 0, "backward: bad arguments");
    Call c;
    if (int rc = make_call(d, batch, dropout_p, seed, workspace, workspace_bytes, stream, "backward", c)) return rc;
    const int Ss = seq_lens_host[0], Sd = seq_lens_host[1];
    DYGNN_REQUIRE(Ss > 0 && Sd > 0 && Ss % d.P == 0 && Sd % d.P == 0 && Ss + Sd <= 2 * d.Smax, "backward: bad sequence lengths");
    c.set_lengths(Ss, Sd);
    const Path path = choose_path(c, packed);
    const Plan& p = c.p;
    hipStream_t s = c.s;
    const int64_t B = c.B, M = c.M;
    const int D = d.D, Fn = d.Fn;
    // output layer: out = pooled W^T + b over both sides
    if (int rc = mm(s, grad_out_src, Fn, true, c.F32(p.pooled), D, false, G(grads->output_w), D, Fn, D, (int)B)) return rc;
    if (int rc = mm(s, grad_out_dst, Fn, true, c.F32(p.pooled) + B * D, D, false, G(grads->output_w), D, Fn, D, (int)B, MmOpt().beta(1.f))) return rc;
    if (int rc = colsum_atomic(s, grad_out_src, Fn, B, Fn, G(grads->output_b))) return rc;
    if (int rc = colsum_atomic(s, grad_out_dst, Fn, B, Fn, G(grads->output_b))) return rc;
    if (int rc = mm(s, grad_out_src, Fn, false, w->output_w, D, false, c.F32(p.dpool), D, (int)B, D, Fn)) return rc;
    if (int rc = mm(s, grad_out_dst, Fn, false, w->output_w, D, false, c.F32(p.dpool) + B * D, D, (int)B, D, Fn)) return rc;
    float* dX = c.F32(p.dX);
    EW(k_pool_bwd, M * D, c.F32(p.dpool), B, c.Ts, c.T, D, dX);
    DwList dw;
    const PackedLayout pl = make_packed_layout(d);
    const float* pk = static_cast<const float*>(packed);
    for (int l = d.NL - 1; l >= 0; --l) {
        const dygnn_encoder_layer_weights& Lw = w->layers[l];
        const dygnn_encoder_layer_weights& Lg = grads->layers[l];
        const auto& L = p.layer[l];
        const LayerGrads g{c.F32(L.dF2), c.F32(L.dH), c.F32(L.dAo), c.F32(L.dQKV)};
        dw.add(g.dF2, D, D, c.F32(L.hact), 4 * D, 4 * D, G(Lg.ffn1_weight), 4 * D, G(Lg.ffn1_bias));                             // dW2 [D][4D], db2
        dw.add(g.dH, 4 * D, 4 * D, c.F32(L.xn1), D, D, G(Lg.ffn0_weight), D, G(Lg.ffn0_bias));                                   // dW1 [4D][D], db1
        if (int rc = path.ffn_bwd ? ffn_backward_fused3(d, pl, pk, l, M, dX, c.F32(L.hpre), c.F32(L.x1), c.F32(L.m1), c.F32(L.r1), g.dF2, g.dH, G(Lg.norm1_weight),
                                                        G(Lg.norm1_bias), c.dr, s)
                                  : ffn_backward_unfused(c, Lw, Lg, l, dX, g)) return rc;
        dw.add(g.dAo, D, D, c.F32(L.oa), D, D, G(Lg.out_proj_weight), D, G(Lg.out_proj_bias));                                   // dWo [D][D], dbo
        dw.add(g.dQKV, 3 * D, 3 * D, c.F32(L.xn0), D, D, G(Lg.in_proj_weight), D, G(Lg.in_proj_bias));                            // dWin [3D][D], dbin
        if (int rc = path.attn_bwd ? attn_backward_fused3(d, pl, pk, l, B, c.T, dX, c.F32(p.X[l]), c.F32(L.m0), c.F32(L.r0), c.F32(L.qkv), c.F32(L.P), c.F32(L.Pd), g.dAo,
                                                          g.dQKV, G(Lg.norm0_weight), G(Lg.norm0_bias), c.dr, s)
                                   : attn_backward_unfused(c, Lw, Lg, l, dX, g)) return rc;
    }
    return inputs_backward(c, w, grads, dX, dw);
}
