// TGAT training (SURVEY.md §8f-1 for BASELINE config 3): the forward of tgat.hip in TRAIN mode and its hand-written backward pass, so that
// train_link_prediction.py:170-185, :242-257 (two calls, MergeLayer + BCE, loss.backward(), Adam) runs on the HIP path.
//
// Differences from the inference forward (tgat.hip: its level and layer stages, tgat_levels / tgat_layers, tgat_stages.h):
//   * no de-duplication of level 1 and no row-block chains: every level entry is its own row, as in the reference recursion
//     (models/TGAT.py:92-110), so each occurrence draws its own dropout mask and each level-(l-1) row has exactly ONE consumer
//     (level l-1 = [level-l self rows ; their neighbour rows]).  The backward pass therefore WRITES the lower level's row gradients:
//     no scatter-add, no atomics on activations.
//   * dropout (models/modules.py:187, :196) on the attention probabilities and on the residual_fc output, masks from train::Drop
//     (dropout.h) keyed by (seed, site = 2 * layer + {0: probabilities, 1: residual_fc output}, dense element index); never stored, the
//     backward pass redraws them.  dropout_p = 0 reproduces the eval forward within fp32 rounding.
//   * every activation the backward pass reads stays in the call's workspace (TrainPlan).
// K and V stay un-materialised: the attention kernels gather the k neighbour input rows x_ij = [h_lower | edge | cos(w dt + b)]
// on the fly and work with W_k,h^T q_ih; the products go through the library's GEMMs (gemm.h), the weight gradients through one grouped
// split-K launch per layer (train::dw_grouped).  The LayerNorm backward with the residual_fc dropout is the shared train::k_res_ln_bwd<5>
// (train_rows.h, with tcl_train.hip and cawn_train.hip; identity row map); the column sums keep colsum.h's one-thread-per-column second
// stage (tgt::colsum), whose summation order the wave-per-column train::colsum does not have.
#include "colsum.h"
#include "common.h"
#include "dropout.h"
#include "gemm.h"
#include "time_encoding.h"
#include "tgat_levels.h"
#include "tgat_train.h"
#include "train_rows.h"

namespace dygnn {
namespace tgt {

using f4 = __attribute__((ext_vector_type(4))) float;
constexpr int NC = 4;                 // float4 columns per lane of an input row: Dkv <= 4 * 64 * 4 = 1024

// TGN: the gradient row of a level-0 node, or NULL where the node passes no gradient on (no pending message; id 0, the padding, never has one)
__device__ __forceinline__ float* feat0_row(const Feat0Grad& fg, int32_t node, int Fn) {
    if (!fg.d || node < 0 || node >= fg.N) return nullptr;
    const int32_t r = fg.pos[node];
    return r < 0 ? nullptr : fg.d + (size_t)r * Fn;
}
__device__ __forceinline__ float dot4(const f4 a, const f4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// The attention's input rows of layer l: x_ir = [h_lower(n + r) | edge(eid[r]) | cos(fma(dt[r], w, b))], r = i * k + j (models/modules.py:157)
struct XRows {
    const float *h_lower, *node_feat, *edge_feat;      // h_lower = level l-1 embeddings, NULL for layer 1 (raw rows through ids_lower)
    const int32_t *ids_lower, *eid;
    const float *dt, *tw, *tb;
    int64_t n;
    int k, Fn, Fe, Ft, Dkv;
    __device__ __forceinline__ f4 get(int64_t r, int c4) const {
        const int kk = 4 * c4;
        if (kk < Fn) {
            const float* hp = h_lower ? h_lower + (n + r) * Fn : node_feat + (size_t)ids_lower[n + r] * Fn;
            return *reinterpret_cast<const f4*>(hp + kk);
        }
        if (kk < Fn + Fe) return *reinterpret_cast<const f4*>(edge_feat + (size_t)eid[r] * Fe + (kk - Fn));
        const int f = kk - Fn - Fe;
        const float d = dt[r];
        return f4{timeenc::cos_time(fmaf(d, tw[f], tb[f])), timeenc::cos_time(fmaf(d, tw[f + 1], tb[f + 1])), timeenc::cos_time(fmaf(d, tw[f + 2], tb[f + 2])),
                  timeenc::cos_time(fmaf(d, tw[f + 3], tb[f + 3]))};
    }
    __device__ __forceinline__ void fetch(int64_t r, int lane, f4 (&xs)[NC]) const {
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int c4 = lane + 64 * u;
            xs[u] = c4 < (Dkv >> 2) ? get(r, c4) : f4{0.f, 0.f, 0.f, 0.f};
        }
    }
};

// q_in = [h(self) | cos(b)] (models/TGAT.py:84, models/modules.py:150-152), one wave per row
__global__ __launch_bounds__(256) void k_tt_qin(const float* __restrict__ h_lower, const float* __restrict__ node_feat, const int32_t* __restrict__ ids_lower,
                                                  const float* __restrict__ tw, const float* __restrict__ tb, int64_t n, int Fn, int Ft, float* __restrict__ q_in) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const float* hs = h_lower ? h_lower + i * Fn : node_feat + (size_t)ids_lower[i] * Fn;
    float* o = q_in + i * (Fn + Ft);
    for (int f = lane; f < Fn; f += 64) o[f] = hs[f];
    for (int f = lane; f < Ft; f += 64) o[Fn + f] = cosf(fmaf(0.0f, tw[f], tb[f]));
}

// Attention of row i over its k neighbours, train mode (one wave per row, every head): scores from qk = W_k,h^T q_ih (modules.py:172-173),
// mask id 0 -> -1e10 (:176-184), softmax -> P (saved, before dropout), z_ih = sum_j drop(p_ijh) x_ij (:187, :190 with W_v,h applied later).
// LDS: scores [H][k], dropped probabilities [H][k].
__global__ __launch_bounds__(64) void k_tt_attn_fwd(const XRows X, const float* __restrict__ qk, int H, float scale, train::Drop dr, uint32_t site,
                                                      float* __restrict__ P, float* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int k = X.k, Dkv = X.Dkv, D4 = Dkv >> 2;
    float* sc = lds;
    float* pd = lds + H * k;
    for (int j = 0; j < k; ++j) {
        f4 xs[NC];
        X.fetch(i * k + j, lane, xs);
        const bool masked = X.ids_lower[X.n + i * k + j] == 0;
        for (int h = 0; h < H; ++h) {
            const f4* qh = reinterpret_cast<const f4*>(qk + ((size_t)i * H + h) * Dkv);
            float a = 0.f;
#pragma unroll
            for (int u = 0; u < NC; ++u)
                if (lane + 64 * u < D4) a += dot4(qh[lane + 64 * u], xs[u]);
            a = wave_sum(a);
            if (lane == 0) sc[h * k + j] = masked ? -1e10f : a * scale;
        }
    }
    __syncthreads();
    const uint32_t skey = dr.site_key(site);
    for (int h = lane; h < H; h += 64) {
        float mx = -INFINITY;
        for (int j = 0; j < k; ++j) mx = fmaxf(mx, sc[h * k + j]);
        float sum = 0.f;
        for (int j = 0; j < k; ++j) { const float e = expf(sc[h * k + j] - mx); sc[h * k + j] = e; sum += e; }
        const float inv = 1.0f / sum;
        for (int j = 0; j < k; ++j) {
            const uint64_t idx = ((uint64_t)i * H + h) * k + j;
            const float p = sc[h * k + j] * inv;
            P[idx] = p;
            pd[h * k + j] = p * dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
        }
    }
    __syncthreads();
    for (int h = 0; h < H; ++h) {
        f4 acc[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < k; ++j) {
            f4 xs[NC];
            X.fetch(i * k + j, lane, xs);
            const float p = pd[h * k + j];
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                acc[u].x = fmaf(p, xs[u].x, acc[u].x); acc[u].y = fmaf(p, xs[u].y, acc[u].y);
                acc[u].z = fmaf(p, xs[u].z, acc[u].z); acc[u].w = fmaf(p, xs[u].w, acc[u].w);
            }
        }
        f4* zo = reinterpret_cast<f4*>(z + ((size_t)i * H + h) * Dkv);
#pragma unroll
        for (int u = 0; u < NC; ++u)
            if (lane + 64 * u < D4) zo[lane + 64 * u] = acc[u];
    }
}

// pre = drop(fc) + q_in, its LayerNorm into the first Dq columns of the MergeLayer input [y | raw] (models/modules.py:196-199, models/TGAT.py:134);
// pre and its mean / rstd are kept for the backward pass.  One wave per row, Dq <= 272 (five elements per lane).
__global__ __launch_bounds__(256) void k_tt_post(const float* __restrict__ fc, const float* __restrict__ q_in, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ node_feat, const int32_t* __restrict__ ids_lower,
                                                   int64_t n, int Dq, int Fn, train::Drop dr, uint32_t site, float* __restrict__ pre,
                                                   float* __restrict__ mean_out, float* __restrict__ rstd_out, float* __restrict__ merge_in) {
    constexpr int NV = 5;
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const uint32_t skey = dr.site_key(site);
    float x[NV];
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        x[u] = 0.f;
        if (f < Dq) {
            const uint64_t idx = (uint64_t)i * Dq + f;
            x[u] = fc[idx] * dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32)) + q_in[idx];
            pre[idx] = x[u];
            s += x[u];
        }
    }
    s = wave_sum(s);
    const float mean = s / (float)Dq;
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + 64 * u < Dq) { const float d = x[u] - mean; v = fmaf(d, d, v); }
    v = wave_sum(v);
    const float rstd = 1.0f / sqrtf(v / (float)Dq + 1e-5f);
    if (lane == 0) { mean_out[i] = mean; rstd_out[i] = rstd; }
    float* o = merge_in + i * (Dq + Fn);
    const float* raw = node_feat + (size_t)ids_lower[i] * Fn;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + 64 * u;
        if (f < Dq) o[f] = (x[u] - mean) * rstd * gamma[f] + beta[f];
        if (f < Fn) o[Dq + f] = raw[f];
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------------
__global__ void k_tt_relu_bwd(float* __restrict__ g, const float* __restrict__ act, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count && !(act[e] > 0.f)) g[e] = 0.f;
}

// Attention backward of row i (one wave per row, every head).  With dz_ih = W_v,h^T datt_ih:
//   dp~_ijh = dz_ih . x_ij ; dp = dp~ * mask (dropout of :187) ; ds_ijh = p (dp - sum_j p dp), zero where the slot is masked (the -1e10 fill
//   cuts the score off; the probability of a masked slot is still used, so padded slots do get dx) ;
//   d(W_k,h^T q_ih) = scale sum_j ds_ijh x_ij ;  dx_ij = sum_h p~_ijh dz_ih + scale ds_ijh (W_k,h^T q_ih).
// dx's h_lower columns are the gradient of the neighbour's level-(l-1) row (its only consumer: written, not added; TGN's level 0: added to
// the node's row of fg, one float atomic per element, skipped for nodes without a pending message); its time columns give
// the time encoder's per-row partial sums (tdw, tdb [n][Ft]: -sin(pre) dt g, -sin(pre) g with the forward's pre = fma(dt, w, b)); the edge
// columns are dropped (constants).  LDS: scale * ds [H][k], p~ [H][k].
__global__ __launch_bounds__(64) void k_tt_attn_bwd(XRows X, const float* const* __restrict__ tabs, const float* __restrict__ qk, const float* __restrict__ P, const float* __restrict__ dz,
                                                      int H, float scale, train::Drop dr, uint32_t site, float* __restrict__ dqk, float* __restrict__ dh_lower,
                                                      float* __restrict__ tdw, float* __restrict__ tdb, const Feat0Grad fg) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int k = X.k, Dkv = X.Dkv, D4 = Dkv >> 2, Fn = X.Fn, Fe = X.Fe, Ft = X.Ft;
    X.node_feat = tabs[0];       // the feature tables of the forward call (the backward's signature does not carry them)
    X.edge_feat = tabs[1];
    float* a = lds;              // dp~, then scale * ds
    float* b = lds + H * k;      // p~
    for (int j = 0; j < k; ++j) {
        f4 xs[NC];
        X.fetch(i * k + j, lane, xs);
        for (int h = 0; h < H; ++h) {
            const f4* dzh = reinterpret_cast<const f4*>(dz + ((size_t)i * H + h) * Dkv);
            float s = 0.f;
#pragma unroll
            for (int u = 0; u < NC; ++u)
                if (lane + 64 * u < D4) s += dot4(dzh[lane + 64 * u], xs[u]);
            s = wave_sum(s);
            if (lane == 0) a[h * k + j] = s;
        }
    }
    __syncthreads();
    const uint32_t skey = dr.site_key(site);
    for (int h = lane; h < H; h += 64) {
        float sum = 0.f;
        for (int j = 0; j < k; ++j) {
            const uint64_t idx = ((uint64_t)i * H + h) * k + j;
            const float m = dr.mask32(skey, (uint32_t)idx + 0x27d4eb2fU * (uint32_t)(idx >> 32));
            const float p = P[idx];
            const float dp = a[h * k + j] * m;
            a[h * k + j] = dp;
            b[h * k + j] = p * m;
            sum = fmaf(p, dp, sum);
        }
        for (int j = 0; j < k; ++j) {
            const float p = P[((uint64_t)i * H + h) * k + j];
            const bool masked = X.ids_lower[X.n + i * k + j] == 0;
            a[h * k + j] = masked ? 0.f : scale * (p * (a[h * k + j] - sum));
        }
    }
    __syncthreads();
    // d(W_k,h^T q_ih) = sum_j (scale ds_ijh) x_ij
    for (int h = 0; h < H; ++h) {
        f4 acc[NC];
#pragma unroll
        for (int u = 0; u < NC; ++u) acc[u] = f4{0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < k; ++j) {
            f4 xs[NC];
            X.fetch(i * k + j, lane, xs);
            const float w = a[h * k + j];
#pragma unroll
            for (int u = 0; u < NC; ++u) {
                acc[u].x = fmaf(w, xs[u].x, acc[u].x); acc[u].y = fmaf(w, xs[u].y, acc[u].y);
                acc[u].z = fmaf(w, xs[u].z, acc[u].z); acc[u].w = fmaf(w, xs[u].w, acc[u].w);
            }
        }
        f4* o = reinterpret_cast<f4*>(dqk + ((size_t)i * H + h) * Dkv);
#pragma unroll
        for (int u = 0; u < NC; ++u)
            if (lane + 64 * u < D4) o[lane + 64 * u] = acc[u];
    }
    // dx_ij, column by column of the lane
    f4 gw[NC], gb[NC];
#pragma unroll
    for (int u = 0; u < NC; ++u) gw[u] = gb[u] = f4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
        const int64_t r = i * k + j;
        const float d = X.dt[r];
        float* frow = dh_lower ? nullptr : feat0_row(fg, X.ids_lower[X.n + r], Fn);      // wave-uniform
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int c4 = lane + 64 * u, kk = 4 * c4;
            if (c4 >= D4 || (kk >= Fn && kk < Fn + Fe) || (kk < Fn && !dh_lower && !frow)) continue;
            f4 g = f4{0.f, 0.f, 0.f, 0.f};
            for (int h = 0; h < H; ++h) {
                const f4 zv = reinterpret_cast<const f4*>(dz + ((size_t)i * H + h) * Dkv)[c4];
                const f4 qv = reinterpret_cast<const f4*>(qk + ((size_t)i * H + h) * Dkv)[c4];
                const float pt = b[h * k + j], ds = a[h * k + j];
                g.x = fmaf(pt, zv.x, fmaf(ds, qv.x, g.x)); g.y = fmaf(pt, zv.y, fmaf(ds, qv.y, g.y));
                g.z = fmaf(pt, zv.z, fmaf(ds, qv.z, g.z)); g.w = fmaf(pt, zv.w, fmaf(ds, qv.w, g.w));
            }
            if (kk < Fn) {
                if (dh_lower) *reinterpret_cast<f4*>(dh_lower + (X.n + r) * Fn + kk) = g;
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) atomicAdd(frow + kk + e, g[e]);
                }
            } else {
                const int f = kk - Fn - Fe;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float sn = sinf(fmaf(d, X.tw[f + e], X.tb[f + e]));
                    gb[u][e] = fmaf(-sn, g[e], gb[u][e]);
                    gw[u][e] = fmaf(-sn * d, g[e], gw[u][e]);
                }
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NC; ++u) {
        const int c4 = lane + 64 * u, kk = 4 * c4;
        if (c4 < D4 && kk >= Fn + Fe) {
            const int f = kk - Fn - Fe;
            *reinterpret_cast<f4*>(tdw + i * Ft + f) = gw[u];
            *reinterpret_cast<f4*>(tdb + i * Ft + f) = gb[u];
        }
    }
}

// The query input's gradient dqin = [dh(self) | d cos(b)]: the h part is the self row's gradient at level l-1 (rows 0..n-1, its only
// consumer; TGN's level 0: added to the node's row of fg), the time part adds -sin(b) g to the time encoder's bias partial sums (dt = 0: no
// weight term).  One thread per element.
__global__ void k_tt_qin_bwd(const float* __restrict__ dqin, int64_t n, int Fn, int Ft, const float* __restrict__ tw, const float* __restrict__ tb,
                             float* __restrict__ dh_lower, float* __restrict__ tdb, const int32_t* __restrict__ ids_lower, const Feat0Grad fg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int Dq = Fn + Ft;
    if (e >= n * Dq) return;
    const int64_t i = e / Dq;
    const int f = (int)(e - i * Dq);
    if (f < Fn) {
        if (dh_lower) dh_lower[i * Fn + f] = dqin[e];
        else if (float* frow = feat0_row(fg, ids_lower[i], Fn)) atomicAdd(frow + f, dqin[e]);
    } else {
        const int t = f - Fn;
        tdb[i * Ft + t] = fmaf(-sinf(fmaf(0.0f, tw[t], tb[t])), dqin[e], tdb[i * Ft + t]);
    }
}

// TGN: rows g [n][Fn] (the MergeLayer's gradient with respect to its second input, feat0[ids[i]]) added to the nodes' rows of fg.
// One thread per element.
__global__ void k_tt_feat0_rows(const float* __restrict__ g, const int32_t* __restrict__ ids, int64_t n, int Fn, const Feat0Grad fg) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * Fn) return;
    const int64_t i = e / Fn;
    if (float* frow = feat0_row(fg, ids[i], Fn)) atomicAdd(frow + (e - i * Fn), g[e]);
}

__global__ void k_tt_tabs(const float** tabs, const float* node_feat, const float* edge_feat) { tabs[0] = node_feat; tabs[1] = edge_feat; }

// ---- workspace --------------------------------------------------------------------------------------------------------------------------
struct TrainPlan {
    int L, k, Fn, Fe, Ft, H, hd, Dq, Dkv;
    int64_t n[DYGNN_MAX_LAYERS + 1];       // n[L] = 2B, n[l-1] = n[l] (1 + k)
    size_t ids[DYGNN_MAX_LAYERS + 1], tms[DYGNN_MAX_LAYERS + 1], eid[DYGNN_MAX_LAYERS + 1], dt[DYGNN_MAX_LAYERS + 1];
    struct Lv { size_t qin, q, qk, P, z, att, pre, mean, rstd, merge, hid, h; } lv[DYGNN_MAX_LAYERS + 1];       // per computed level 1..L
    size_t tabs;                                                                                                // the forward's feature table pointers
    size_t fc;                                                                                                  // forward scratch
    size_t dh0, dh1, dhid, dy, dyx, dfc, dqin, datt, dz, dqk, dq, tdw, tdb, part;                               // backward scratch
    size_t total;
};

static TrainPlan make_plan(const dygnn_tgat_config& c, int64_t B) {
    TrainPlan p{};
    p.L = c.num_layers; p.k = c.num_neighbors; p.Fn = c.node_feat_dim; p.Fe = c.edge_feat_dim; p.Ft = c.time_feat_dim; p.H = c.num_heads;
    p.Dq = p.Fn + p.Ft; p.Dkv = p.Fn + p.Fe + p.Ft; p.hd = p.Dq / p.H;
    p.n[p.L] = 2 * B;
    for (int l = p.L; l >= 1; --l) p.n[l - 1] = p.n[l] * (1 + p.k);
    size_t o = 0;
    auto take = [&](size_t floats) { size_t r = o; o += (floats * 4 + 255) & ~size_t(255); return r; };      // 4-byte elements
    for (int l = 0; l <= p.L; ++l) {
        p.ids[l] = take(p.n[l]);
        p.tms[l] = take(2 * p.n[l]);
        if (l == 0) continue;
        const size_t n = p.n[l];
        p.eid[l] = take(n * p.k);
        p.dt[l] = take(n * p.k);
        TrainPlan::Lv& v = p.lv[l];
        v.qin = take(n * p.Dq); v.q = take(n * p.Dq); v.qk = take(n * p.H * p.Dkv); v.P = take(n * p.H * p.k); v.z = take(n * p.H * p.Dkv);
        v.att = take(n * p.Dq); v.pre = take(n * p.Dq); v.mean = take(n); v.rstd = take(n); v.merge = take(n * (p.Dq + p.Fn));
        v.hid = take(n * p.Fn); v.h = take(n * p.Fn);
    }
    const size_t nm = p.n[1];                 // the largest computed level
    p.tabs = take(4);
    p.fc = take(nm * p.Dq);
    p.dh0 = take(nm * p.Fn); p.dh1 = take(nm * p.Fn);
    p.dhid = take(nm * p.Fn); p.dy = take(nm * p.Dq); p.dyx = take(nm * p.Dq); p.dfc = take(nm * p.Dq); p.dqin = take(nm * p.Dq);
    p.datt = take(nm * p.Dq); p.dz = take(nm * p.H * p.Dkv); p.dqk = take(nm * p.H * p.Dkv); p.dq = take(nm * p.Dq);
    p.tdw = take(nm * p.Ft); p.tdb = take(nm * p.Ft);
    p.part = take((size_t)ceil_div((int64_t)nm, kColRows) * p.Dq);
    p.total = o;
    return p;
}

static int check_train(const dygnn_tgat_config* cfg) {
    static_assert(4 * 64 * NC == 1024, "check_tgat bounds Dkv by the columns a lane holds");
    return check_tgat(cfg);
}

size_t train_plan_bytes(const dygnn_tgat_config& cfg, int64_t batch) { return make_plan(cfg, batch).total; }

TrainLevel0 train_level0(const dygnn_tgat_config& cfg, int64_t batch, void* workspace) {
    const TrainPlan p = make_plan(cfg, batch);
    return TrainLevel0{reinterpret_cast<const int32_t*>(static_cast<char*>(workspace) + p.ids[0]), p.n[0], p.n[1]};
}

int train_levels(hipStream_t s, const dygnn_tgat_config& cfg, const dygnn_csr* csr, const dygnn_tgat_levels* levels, const int64_t* src, const int64_t* dst,
                 const double* times, int64_t batch, void* workspace, const char* what) {
    const TrainPlan p = make_plan(cfg, batch);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    // levels: sampled here (`recent`) or copied from the caller's host-replayed draws (random strategies, as dygnn_tgat_forward_levels); both
    // write ids[0..L-1] (level L is read from src / dst)
    LevelBufs to{};
    for (int l = 0; l < p.L; ++l) { to.ids[l] = I32(p.ids[l]); to.times[l] = reinterpret_cast<double*>(ws + p.tms[l]); }
    for (int l = 1; l <= p.L; ++l) { to.eid[l] = I32(p.eid[l]); to.dt[l] = F32(p.dt[l]); }
    return levels ? copy_levels(s, levels, p.L, p.k, p.n, p.L, to, what) : expand_levels(s, csr, TgatRoots{src, dst, times, batch, false}, p.L, p.k, to);
}

int train_forward(hipStream_t s, const dygnn_tgat_config& cfg, const dygnn_tgat_weights* w, const float* node_feat, const float* edge_feat, int64_t batch,
                  float dropout_p, uint64_t seed, float* out_src, float* out_dst, void* workspace) {
    const TrainPlan p = make_plan(cfg, batch);
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    hipLaunchKernelGGL(k_tt_tabs, dim3(1), dim3(1), 0, s, reinterpret_cast<const float**>(ws + p.tabs), node_feat, edge_feat);
    DYGNN_LAUNCH_CHECK();
    const train::Drop dr = train::make_drop(dropout_p, seed);
    const float scale = (float)pow((double)p.hd, -0.5);
    const size_t attn_lds = (size_t)2 * p.H * p.k * sizeof(float);
    for (int l = 1; l <= p.L; ++l) {
        const dygnn_tgat_layer_weights& Lw = w->layers[l - 1];
        const TrainPlan::Lv& v = p.lv[l];
        const int64_t n = p.n[l];
        const float* h_lower = l >= 2 ? F32(p.lv[l - 1].h) : nullptr;
        const int32_t* ids_lower = I32(p.ids[l - 1]);
        hipLaunchKernelGGL(k_tt_qin, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, h_lower, node_feat, ids_lower, w->time_w, w->time_b, n, p.Fn, p.Ft, F32(v.qin));
        DYGNN_LAUNCH_CHECK();
        if (int rc = train::mm(s, F32(v.qin), p.Dq, false, Lw.query_w, p.Dq, true, F32(v.q), p.Dq, (int)n, p.Dq, p.Dq)) return rc;
        // qk[i][h] = W_k,h^T q_ih, per head [n][hd] x [hd][Dkv]
        if (int rc = train::mm(s, F32(v.q), p.Dq, false, Lw.key_w, p.Dkv, false, F32(v.qk), p.H * p.Dkv, (int)n, p.Dkv, p.hd,
                               train::MmOpt().batched(p.H, p.H).strideA(0, p.hd).strideB(0, (int64_t)p.hd * p.Dkv).strideC(0, p.Dkv))) return rc;
        const XRows X{h_lower, node_feat, edge_feat, ids_lower, I32(p.eid[l]), F32(p.dt[l]), w->time_w, w->time_b, n, p.k, p.Fn, p.Fe, p.Ft, p.Dkv};
        hipLaunchKernelGGL(k_tt_attn_fwd, dim3((unsigned)n), dim3(64), attn_lds, s, X, F32(v.qk), p.H, scale, dr, (uint32_t)(2 * (l - 1)), F32(v.P), F32(v.z));
        DYGNN_LAUNCH_CHECK();
        // att[i][h*hd ..] = W_v,h z_ih
        if (int rc = train::mm(s, F32(v.z), p.H * p.Dkv, false, Lw.value_w, p.Dkv, true, F32(v.att), p.Dq, (int)n, p.hd, p.Dkv,
                               train::MmOpt().batched(p.H, p.H).strideA(0, p.Dkv).strideB(0, (int64_t)p.hd * p.Dkv).strideC(0, p.hd))) return rc;
        if (int rc = train::mm(s, F32(v.att), p.Dq, false, Lw.res_w, p.Dq, true, F32(p.fc), p.Dq, (int)n, p.Dq, p.Dq, train::MmOpt().bias(Lw.res_b))) return rc;
        hipLaunchKernelGGL(k_tt_post, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, F32(p.fc), F32(v.qin), Lw.ln_w, Lw.ln_b, node_feat, ids_lower, n, p.Dq, p.Fn,
                           dr, (uint32_t)(2 * (l - 1) + 1), F32(v.pre), F32(v.mean), F32(v.rstd), F32(v.merge));
        DYGNN_LAUNCH_CHECK();
        if (int rc = train::mm(s, F32(v.merge), p.Dq + p.Fn, false, Lw.fc1_w, p.Dq + p.Fn, true, F32(v.hid), p.Fn, (int)n, p.Fn, p.Dq + p.Fn,
                               train::MmOpt().bias(Lw.fc1_b).relu())) return rc;
        if (int rc = train::mm(s, F32(v.hid), p.Fn, false, Lw.fc2_w, p.Fn, true, F32(v.h), p.Fn, (int)n, p.Fn, p.Fn, train::MmOpt().bias(Lw.fc2_b))) return rc;
    }
    const size_t half = (size_t)batch * p.Fn * sizeof(float);
    DYGNN_HIP(hipMemcpyAsync(out_src, F32(p.lv[p.L].h), half, hipMemcpyDeviceToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(out_dst, reinterpret_cast<char*>(F32(p.lv[p.L].h)) + half, half, hipMemcpyDeviceToDevice, s));
    return DYGNN_OK;
}

int train_backward(hipStream_t s, const dygnn_tgat_config& cfg, const dygnn_tgat_weights* w, const dygnn_tgat_weights* grads, const float* grad_out_src,
                   const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed, void* workspace, const Feat0Grad* feat0) {
    const TrainPlan p = make_plan(cfg, batch);
    const Feat0Grad fg = feat0 ? *feat0 : Feat0Grad{nullptr, nullptr, 0};
    char* ws = static_cast<char*>(workspace);
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(ws + off); };
    auto W = [](const float* g) { return const_cast<float*>(g); };
    const train::Drop dr = train::make_drop(dropout_p, seed);
    const float scale = (float)pow((double)p.hd, -0.5);
    const size_t attn_lds = (size_t)2 * p.H * p.k * sizeof(float);
    const int Dq = p.Dq, Fn = p.Fn, Ft = p.Ft, Dkv = p.Dkv, H = p.H, hd = p.hd;
    float* dh = F32(p.dh0);          // gradient of the level being processed (level l), written by the level above
    float* dh_low = F32(p.dh1);      // gradient of level l-1
    const size_t half = (size_t)batch * Fn * sizeof(float);
    DYGNN_HIP(hipMemcpyAsync(dh, grad_out_src, half, hipMemcpyDeviceToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(reinterpret_cast<char*>(dh) + half, grad_out_dst, half, hipMemcpyDeviceToDevice, s));
    for (int l = p.L; l >= 1; --l) {
        const dygnn_tgat_layer_weights& Lw = w->layers[l - 1];
        const dygnn_tgat_layer_weights& G = grads->layers[l - 1];
        const TrainPlan::Lv& v = p.lv[l];
        const int64_t n = p.n[l];
        const int ni = (int)n;
        const float* h_lower = l >= 2 ? F32(p.lv[l - 1].h) : nullptr;
        float* dlow = l >= 2 ? dh_low : nullptr;         // level 0: TGAT's raw features get no gradient, TGN's feat0 rows are summed per node (fg)
        const int32_t* ids_lower = I32(p.ids[l - 1]);
        const uint32_t site_p = (uint32_t)(2 * (l - 1)), site_o = site_p + 1;
        // 1. MergeLayer: fc2 -> ReLU -> fc1 (the second half of the merge input: TGAT's raw features get no gradient; TGN's feat0[ids[i]] does, at
        //    every layer -- through p.datt, which step 3 writes only later)
        if (int rc = train::mm(s, dh, Fn, false, Lw.fc2_w, Fn, false, F32(p.dhid), Fn, ni, Fn, Fn)) return rc;
        hipLaunchKernelGGL(k_tt_relu_bwd, dim3((unsigned)ceil_div(n * Fn, 256)), dim3(256), 0, s, F32(p.dhid), F32(v.hid), n * Fn);
        DYGNN_LAUNCH_CHECK();
        if (int rc = train::mm(s, F32(p.dhid), Fn, false, Lw.fc1_w, Dq + Fn, false, F32(p.dy), Dq, ni, Dq, Fn)) return rc;
        if (fg.d) {
            if (int rc = train::mm(s, F32(p.dhid), Fn, false, Lw.fc1_w + Dq, Dq + Fn, false, F32(p.datt), Fn, ni, Fn, Fn)) return rc;
            hipLaunchKernelGGL(k_tt_feat0_rows, dim3((unsigned)ceil_div(n * Fn, 256)), dim3(256), 0, s, F32(p.datt), ids_lower, n, Fn, fg);
            DYGNN_LAUNCH_CHECK();
        }
        // 2. LayerNorm + residual + residual_fc dropout (train_rows.h, Dq <= 272: five columns per lane): dpre reaches the residual q_in (dqin)
        //    and, through the dropout mask, the residual_fc output (dfc); dyx = dy xhat feeds the gamma gradient
        hipLaunchKernelGGL(train::k_res_ln_bwd<5>, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, F32(p.dy), F32(v.pre), F32(v.mean), F32(v.rstd), Lw.ln_w, n, Dq,
                           train::RowMap{0, 0}, dr, site_o, F32(p.dqin), F32(p.dfc), F32(p.dyx));
        DYGNN_LAUNCH_CHECK();
        if (int rc = colsum(s, F32(p.dyx), Dq, n, Dq, F32(p.part), W(G.ln_w))) return rc;
        if (int rc = colsum(s, F32(p.dy), Dq, n, Dq, F32(p.part), W(G.ln_b))) return rc;
        // 3. residual_fc, then W_v per head: dz_ih = W_v,h^T datt_ih
        if (int rc = train::mm(s, F32(p.dfc), Dq, false, Lw.res_w, Dq, false, F32(p.datt), Dq, ni, Dq, Dq)) return rc;
        if (int rc = train::mm(s, F32(p.datt), Dq, false, Lw.value_w, Dkv, false, F32(p.dz), H * Dkv, ni, Dkv, hd,
                               train::MmOpt().batched(H, H).strideA(0, hd).strideB(0, (int64_t)hd * Dkv).strideC(0, Dkv))) return rc;
        // 4. attention
        const XRows X{h_lower, nullptr, nullptr, ids_lower, I32(p.eid[l]), F32(p.dt[l]), w->time_w, w->time_b, n, p.k, Fn, p.Fe, Ft, Dkv};
        hipLaunchKernelGGL(k_tt_attn_bwd, dim3((unsigned)n), dim3(64), attn_lds, s, X, reinterpret_cast<const float* const*>(ws + p.tabs), F32(v.qk), F32(v.P),
                           F32(p.dz), H, scale, dr, site_p, F32(p.dqk), dlow, F32(p.tdw), F32(p.tdb), fg);
        DYGNN_LAUNCH_CHECK();
        // 5. W_k, W_q: dq_ih = W_k,h d(W_k,h^T q_ih); dqin += dq W_q
        if (int rc = train::mm(s, F32(p.dqk), H * Dkv, false, Lw.key_w, Dkv, true, F32(p.dq), Dq, ni, hd, Dkv,
                               train::MmOpt().batched(H, H).strideA(0, Dkv).strideB(0, (int64_t)hd * Dkv).strideC(0, hd))) return rc;
        if (int rc = train::mm(s, F32(p.dq), Dq, false, Lw.query_w, Dq, false, F32(p.dqin), Dq, ni, Dq, Dq, train::MmOpt().beta(1.f))) return rc;
        hipLaunchKernelGGL(k_tt_qin_bwd, dim3((unsigned)ceil_div(n * Dq, 256)), dim3(256), 0, s, F32(p.dqin), n, Fn, Ft, w->time_w, w->time_b, dlow, F32(p.tdb), ids_lower, fg);
        DYGNN_LAUNCH_CHECK();
        // 7. time encoder (shared by all layers and the query's cos(b)): per-row partials -> fixed-order column sums
        if (int rc = colsum(s, F32(p.tdw), Ft, n, Ft, F32(p.part), W(grads->time_w))) return rc;
        if (int rc = colsum(s, F32(p.tdb), Ft, n, Ft, F32(p.part), W(grads->time_b))) return rc;
        // 6. the layer's weight gradients, grouped split-K over its n rows
        train::DwPair pairs[4 + 2 * 68];
        int np = 0;
        pairs[np++] = {dh, Fn, Fn, F32(v.hid), Fn, Fn, W(G.fc2_w), Fn, W(G.fc2_b)};
        pairs[np++] = {F32(p.dhid), Fn, Fn, F32(v.merge), Dq + Fn, Dq + Fn, W(G.fc1_w), Dq + Fn, W(G.fc1_b)};
        pairs[np++] = {F32(p.dfc), Dq, Dq, F32(v.att), Dq, Dq, W(G.res_w), Dq, W(G.res_b)};
        pairs[np++] = {F32(p.dq), Dq, Dq, F32(v.qin), Dq, Dq, W(G.query_w), Dq, nullptr};
        for (int h = 0; h < H; ++h) {
            pairs[np++] = {F32(p.datt) + h * hd, Dq, hd, F32(v.z) + (size_t)h * Dkv, H * Dkv, Dkv, W(G.value_w) + (size_t)h * hd * Dkv, Dkv, nullptr};
            pairs[np++] = {F32(v.q) + h * hd, Dq, hd, F32(p.dqk) + (size_t)h * Dkv, H * Dkv, Dkv, W(G.key_w) + (size_t)h * hd * Dkv, Dkv, nullptr};
        }
        for (int b0 = 0; b0 < np; b0 += 16)
            if (int rc = train::dw_grouped(s, ni, pairs + b0, np - b0 < 16 ? np - b0 : 16)) return rc;
        float* t = dh; dh = dh_low; dh_low = t;
    }
    return DYGNN_OK;
}

}  // namespace tgt
}  // namespace dygnn

using namespace dygnn;
using namespace dygnn::tgt;

extern "C" size_t dygnn_tgat_train_workspace_bytes(const dygnn_tgat_config* cfg, int64_t batch) {
    if (check_train(cfg) != DYGNN_OK || batch < 1) return 0;
    return make_plan(*cfg, batch).total;
}

extern "C" int dygnn_tgat_train_forward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_csr* csr, const dygnn_tgat_levels* levels,
                                        const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times,
                                        int64_t batch, float dropout_p, uint64_t seed, float* out_src, float* out_dst, void* workspace,
                                        size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = check_train(cfg)) return rc;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && node_feat && edge_feat, "tgat_train_forward: null pointer");
    DYGNN_REQUIRE(batch > 0 && out_src && out_dst && workspace, "tgat_train_forward: bad arguments");
    DYGNN_REQUIRE(levels || (csr && csr->indptr && csr->num_nodes >= 1 && src && dst && times), "tgat_train_forward: need levels or csr + src / dst / times");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "tgat_train_forward: dropout must be in [0, 1)");
    const size_t need = train_plan_bytes(*cfg, batch);
    if (workspace_bytes < need) { set_error("tgat_train_forward: workspace too small (%zu < %zu bytes)", workspace_bytes, need); return DYGNN_E_WORKSPACE; }
    if (int rc = check_layer_weights(w, cfg->num_layers, "tgat_train_forward: null layer weights")) return rc;
    hipStream_t s = as_stream(stream);
    if (int rc = train_levels(s, *cfg, csr, levels, src, dst, times, batch, workspace, "tgat_train_forward")) return rc;
    return train_forward(s, *cfg, w, node_feat, edge_feat, batch, dropout_p, seed, out_src, out_dst, workspace);
}

extern "C" int dygnn_tgat_backward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_tgat_weights* grads, const float* grad_out_src,
                                   const float* grad_out_dst, int64_t batch, float dropout_p, uint64_t seed, void* workspace, size_t workspace_bytes,
                                   dygnn_stream_t stream) {
    if (int rc = check_train(cfg)) return rc;
    DYGNN_REQUIRE(w && w->time_w && w->time_b && grads && grads->time_w && grads->time_b && grad_out_src && grad_out_dst && workspace && batch > 0,
                  "tgat_backward: bad arguments");
    DYGNN_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "tgat_backward: dropout must be in [0, 1)");
    const size_t need = train_plan_bytes(*cfg, batch);
    if (workspace_bytes < need) { set_error("tgat_backward: workspace too small (%zu < %zu bytes)", workspace_bytes, need); return DYGNN_E_WORKSPACE; }
    if (int rc = check_layer_weights(w, cfg->num_layers, "tgat_backward: null layer weights")) return rc;
    if (int rc = check_layer_weights(grads, cfg->num_layers, "tgat_backward: null gradient buffer")) return rc;
    return train_backward(as_stream(stream), *cfg, w, grads, grad_out_src, grad_out_dst, batch, dropout_p, seed, workspace, nullptr);
}
