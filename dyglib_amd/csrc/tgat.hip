// TGAT forward (BASELINE config 3; reference models/TGAT.py:48-136 + MultiHeadAttention models/modules.py:99-206 +
// MergeLayer models/modules.py:42-68), eval mode.
//
// The reference recurses per node set: layer-l embeddings of a set need layer-(l-1) embeddings of the set itself and of
// its k most recent neighbours.  Here the recursion is unrolled top-down into level sets (level L = the 2B query nodes,
// level l-1 = [level-l nodes ; their k neighbours]; neighbour times are the float32 values the sampler returns,
// models/TGAT.py:107-110) and evaluated bottom-up, one batched pass per layer:
//   sample_recent -> query projection -> W_k^T q per head -> attention over the k neighbours' INPUT rows (gathered on the
//   fly; K and V are never materialised, see k_tgat_attn_lin) -> W_v z per head -> residual_fc + residual + LayerNorm ->
//   MergeLayer.  All products go through the library's general fp32-MFMA GEMM (gemm.h).
#include <cstdlib>
#include "common.h"
#include "gemm.h"
#include "tgat_chain.h"
#include "tgat_attn.h"
#include "tgat_stages.h"
#include "tgn.h"

namespace dygnn {

using f4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f4 tmfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// level expansion: for the n nodes of a level (ids/times), sample the k most recent neighbours (utils/utils.py:200-209)
// and append them to the next-lower level: lower = [this level ; neighbours (row-major n x k)].
// nbr ids / edge ids int32, times float64 holding float32-rounded values (models/TGAT.py:107-110).
// TGN (MemoryModel.py:108-109, :609): the level-0 set of a call is what it reads.  Every level-0 slot (entry q, position j) stores
// owner[id] = slot -- plain stores, some slot of a node wins; chain::pack's list blocks (tgat_chain.h: ListArgs) let the winner list its
// node.  (Flags claimed with returning atomics cost 25 us per step here: 8,800 device-scope atomics on a 28-KB array.)
// (struct TgnTouch: tgn.h)
// `src` given: this is the top level [src ; dst] read straight from the caller's int64 / float64 arrays (B pairs)
__global__ __launch_bounds__(256) void k_tgat_expand(const int64_t* __restrict__ indptr, const int32_t* __restrict__ cnbr,
                                                       const int32_t* __restrict__ ceid, const double* __restrict__ cts, int64_t num_nodes,
                                                       const int32_t* __restrict__ ids, const double* __restrict__ times, int64_t n, int k,
                                                       int32_t* __restrict__ lower_ids, double* __restrict__ lower_times,
                                                       int32_t* __restrict__ nbr_eid, float* __restrict__ nbr_dt, const int32_t* __restrict__ n_live,
                                                       const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const double* __restrict__ tq,
                                                       int64_t B, const TgnTouch tt, int per_root) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tt.owner && blockIdx.x == 0 && threadIdx.x < 2) tt.counts[threadIdx.x] = 0;
    if (q >= n || (n_live && q >= *n_live)) return;      // n = layout size of the level, *n_live = entries in use (de-duplicated level)
    int64_t node = src ? (q < B ? src[q] : dst[q - B]) : (int64_t)ids[q];
    if (node < 0 || node >= num_nodes) node = 0;
    const double t = src ? tq[(per_root || q < B) ? q : q - B] : times[q];
    const int64_t lo = indptr[node], hi = indptr[node + 1];
    const int64_t i = wave_lower_bound(cts, lo, hi, t, lane);
    const int64_t len = i - lo;
    const int m = (int)(len < k ? len : k), pad = k - m;
    if (lane == 0) {
        lower_ids[q] = (int32_t)node; lower_times[q] = t;
        if (tt.owner && node < tt.N) tt.owner[node] = (int32_t)(q * (k + 1) + k);
    }
    for (int j = lane; j < k; j += kWave) {
        int32_t nb = 0, e = 0;
        float tn = 0.f;
        if (j >= pad) {
            const int64_t p = i - m + (j - pad);
            nb = cnbr[p]; e = ceid[p]; tn = (float)cts[p];              // float32 on store, utils/utils.py:167
        }
        lower_ids[n + q * k + j] = nb;
        lower_times[n + q * k + j] = (double)tn;                        // hop-(l+1) queries use the float32 time
        nbr_eid[q * k + j] = e;
        nbr_dt[q * k + j] = (float)(t - (double)tn);                    // models/TGAT.py:116-119: f64 - f32 -> f64 -> .float()
        if (tt.owner && nb >= 0 && nb < tt.N) tt.owner[nb] = (int32_t)(q * (k + 1) + j);
    }
}

// the query-input rows alone, [n][Fn+Ft] = [h(self) | cos(b)]: one wave per row, four rows per workgroup, float4 copies (its predecessor, one
// 256-thread workgroup per 1.1-KB row, ran a 119 k-row level at 1.3 TB/s: 163 us) (models/modules.py:150-157)
__global__ __launch_bounds__(256) void k_tgat_qrows(const float* __restrict__ h_lower, const float* __restrict__ node_feat, const int32_t* __restrict__ lower_ids,
                                                      const float* __restrict__ tw, const float* __restrict__ tb, int64_t n, int Fn, int Ft,
                                                      float* __restrict__ q_in, const int32_t* __restrict__ n_live, const int32_t* __restrict__ lower_map) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n || (n_live && i >= *n_live)) return;
    const float* hsrc = h_lower ? h_lower + (lower_map ? (int64_t)lower_map[i] : i) * Fn : node_feat + (size_t)lower_ids[i] * Fn;
    float* o = q_in + i * (Fn + Ft);
    for (int x = lane; x < (Fn >> 2); x += kWave) *reinterpret_cast<f4*>(o + 4 * x) = *reinterpret_cast<const f4*>(hsrc + 4 * x);
    for (int f = lane; f < Ft; f += kWave) o[Fn + f] = cosf(fmaf(0.0f, tw[f], tb[f]));      // the encoding of dt = 0 (models/TGAT.py:84)
}

using timeenc::cos_time;

// C[M][N] = act(A[M][K] . W[N][K]^T + bias): fp32 MFMA, operands straight from global memory (both are K-contiguous, so
// lane (c,g) of a 16x16x4 fragment reads the float4 at [row c][k0 + 4g]); a wave computes a 64 x 64 block (4x4 tiles).
// Transposed product: accumulator tile = C^T[n = 4g+r][m = c]  ->  float4 store at C[m][n0 + 4g].
template <bool RELU>
__global__ __launch_bounds__(256) void k_gemm_nt(const float* __restrict__ A, const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ C, int64_t M, int N, int K, int ldc, int ldw = 0) {
    if (ldw == 0) ldw = K;                   // row stride of W (a product over the first K columns of wider rows passes it)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
    const int n0 = blockIdx.y * 64;
    if (m0 >= M) return;
    f4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int kk = k0 + 4 * g;
        f4 a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 16 * i + c;
            a[i] = (n < N && kk < K) ? *reinterpret_cast<const f4*>(W + (size_t)n * ldw + kk) : f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = m0 + 16 * j + c;
            b[j] = (m < M && kk < K) ? *reinterpret_cast<const f4*>(A + (size_t)m * K + kk) : f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[i][j] = tmfma(a[i].x, b[j].x, acc[i][j]);
                acc[i][j] = tmfma(a[i].y, b[j].y, acc[i][j]);
                acc[i][j] = tmfma(a[i].z, b[j].z, acc[i][j]);
                acc[i][j] = tmfma(a[i].w, b[j].w, acc[i][j]);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + 16 * i + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t m = m0 + 16 * j + c;
            if (m >= M) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (n + r < N) {
                    float v = acc[i][j][r] + (bias ? bias[n + r] : 0.f);
                    if (RELU) v = fmaxf(v, 0.f);
                    C[(size_t)m * ldc + n + r] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Attention over the k neighbours WITHOUT materialising K and V.  The key / value projections are bias-free linear maps
// (models/modules.py:126-128), so
//     score_ijh = q_ih . (W_k,h x_ij) = (W_k,h^T q_ih) . x_ij          and          o_ih = sum_j p_ijh (W_v,h x_ij) = W_v,h (sum_j p_ijh x_ij)
// with x_ij = [h(nbr) | edge | cos(w dt + b)] the neighbour's input row: the two [n*k, 444] x [444, 272] products (81 GFLOP per
// layer-1 pass at Reddit size) become two [n, 136] x [136, 444] products per head (4 GFLOP) around this kernel, which is
// bound by gathering the input rows twice.  One wave per node; lanes sweep a row as float4, NCOL per lane (Dkv/4 <= 64 NCOL columns).
// qk [n][H][Dkv] = W_k,h^T q_ih ; z [n][H][Dkv] = sum_j p_ijh x_ij.
// ------------------------------------------------------------------------------------------------
// KCACHE > 0: the k <= KCACHE input rows stay in registers between the score pass and the weighted sum (one gather).  NCOL = 2: Dkv <= 512,
// NCOL = 4: Dkv <= 1024 (check_tgat's bound, the training path's).
template <int KCACHE, int NCOL>
__global__ __launch_bounds__(256) void k_tgat_attn_lin(const float* __restrict__ qk, const float* __restrict__ h_lower, const float* __restrict__ node_feat,
                                                         const float* __restrict__ edge_feat, const int32_t* __restrict__ lower_ids,
                                                         const int32_t* __restrict__ nbr_eid, const float* __restrict__ nbr_dt, const float* __restrict__ tw,
                                                         const float* __restrict__ tb, int64_t n, int k, int Fn, int Fe, int Ft, int H, float scale,
                                                         float* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * 4 + wave;
    if (i >= n) return;
    float* pw = reinterpret_cast<float*>(smem) + wave * H * k;       // [H][k] scores -> probabilities
    const int Dkv = Fn + Fe + Ft, D4 = Dkv >> 2;
    bool vc[NCOL];                                                   // float4 column lane + 64 c of the row exists
#pragma unroll
    for (int c = 0; c < NCOL; ++c) vc[c] = lane + 64 * c < D4;
    auto fetch = [&](int64_t r, int x) -> f4 {                       // float4 column x of the input row of neighbour entry r
        const int kk = 4 * x;
        if (kk < Fn) {
            const int64_t le = n + r;
            const float* hp = h_lower ? h_lower + le * Fn : node_feat + (size_t)lower_ids[le] * Fn;
            return *reinterpret_cast<const f4*>(hp + kk);
        }
        if (kk < Fn + Fe) return *reinterpret_cast<const f4*>(edge_feat + (size_t)nbr_eid[r] * Fe + (kk - Fn));
        const int f = kk - Fn - Fe;
        const float dt = nbr_dt[r];
        const f4 w = *reinterpret_cast<const f4*>(tw + f), b = *reinterpret_cast<const f4*>(tb + f);
        return f4{cos_time(fmaf(dt, w.x, b.x)), cos_time(fmaf(dt, w.y, b.y)), cos_time(fmaf(dt, w.z, b.z)), cos_time(fmaf(dt, w.w, b.w))};
    };
    auto dot4 = [](const f4 a, const f4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); };
    const f4 zero = f4{0.f, 0.f, 0.f, 0.f};
    f4 xs[KCACHE > 0 ? KCACHE : 1][NCOL];
    if (KCACHE > 0) {
        // all k rows are requested back to back (one memory latency for the whole neighbourhood), then every (row, head)
        // score is reduced: 2*k independent butterfly chains that pipeline instead of one chain per loop iteration
        // Branch-free gathers: which table a lane reads (node / edge / none) depends only on its column, so every lane
        // issues exactly one unconditional float4 load per row and pass (lanes of the time columns and beyond read row 0 of
        // the edge table and discard it); the row indices are wave-uniform scalars.  The cosines are filled in afterwards.
        const float* ntab = h_lower ? h_lower : node_feat;
        const float* bp[NCOL]; size_t st[NCOL]; int cls[NCOL];
#pragma unroll
        for (int ps = 0; ps < NCOL; ++ps) {
            const int kk = 4 * (lane + 64 * ps);
            cls[ps] = kk < Fn ? 0 : kk < Fn + Fe ? 1 : kk < Dkv ? 2 : 3;
            bp[ps] = cls[ps] == 0 ? ntab + kk : cls[ps] == 1 ? edge_feat + (kk - Fn) : edge_feat;
            st[ps] = cls[ps] == 0 ? (size_t)Fn : cls[ps] == 1 ? (size_t)Fe : 0;
        }
#pragma unroll
        for (int j = 0; j < KCACHE; ++j) {
            const int64_t r = i * k + (j < k ? j : 0);
            const int64_t nrow = h_lower ? n + r : (int64_t)lower_ids[n + r];
            const int64_t erow = nbr_eid[r];
#pragma unroll
            for (int ps = 0; ps < NCOL; ++ps) xs[j][ps] = *reinterpret_cast<const f4*>(bp[ps] + (cls[ps] == 0 ? nrow : erow) * st[ps]);
        }
        // time encoding: computed in a ROLLED loop into LDS (the cosine code exists once; unrolled over 20 rows it alone was
        // 100 KB of straight-line code, more than the instruction cache, executed once per wave), then read back per row
        float* tf = reinterpret_cast<float*>(smem) + 4 * H * k + (size_t)wave * KCACHE * Ft;          // [KCACHE][Ft]
#pragma unroll
        for (int ps = 0; ps < NCOL; ++ps) {
            if (cls[ps] == 2) {
                const int f = 4 * (lane + 64 * ps) - Fn - Fe;
                const f4 w = *reinterpret_cast<const f4*>(tw + f), b = *reinterpret_cast<const f4*>(tb + f);
#pragma unroll 1
                for (int j = 0; j < k; ++j) {
                    const float dt = nbr_dt[i * k + j];
                    *reinterpret_cast<f4*>(tf + j * Ft + f) = f4{cos_time(fmaf(dt, w.x, b.x)), cos_time(fmaf(dt, w.y, b.y)), cos_time(fmaf(dt, w.z, b.z)),
                                                                cos_time(fmaf(dt, w.w, b.w))};
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int ps = 0; ps < NCOL; ++ps) {
            if (cls[ps] == 2) {
                const int f = 4 * (lane + 64 * ps) - Fn - Fe;
#pragma unroll
                for (int j = 0; j < KCACHE; ++j) xs[j][ps] = *reinterpret_cast<const f4*>(tf + (j < k ? j : 0) * Ft + f);
            } else if (cls[ps] == 3) {
#pragma unroll
                for (int j = 0; j < KCACHE; ++j) xs[j][ps] = zero;
            }
        }
#pragma unroll
        for (int j = 0; j < KCACHE; ++j)
            if (j >= k)
#pragma unroll
                for (int ps = 0; ps < NCOL; ++ps) xs[j][ps] = zero;
        for (int h = 0; h < H; ++h) {
            const f4* qh = reinterpret_cast<const f4*>(qk + ((size_t)i * H + h) * Dkv);
            f4 qv[NCOL];
#pragma unroll
            for (int c = 0; c < NCOL; ++c) qv[c] = vc[c] ? qh[lane + 64 * c] : zero;
            float sc[KCACHE > 0 ? KCACHE : 1];
#pragma unroll
            for (int j = 0; j < KCACHE; ++j) {
                sc[j] = dot4(qv[0], xs[j][0]);
#pragma unroll
                for (int c = 1; c < NCOL; ++c) sc[j] += dot4(qv[c], xs[j][c]);
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1)
#pragma unroll
                for (int j = 0; j < KCACHE; ++j) sc[j] += __shfl_xor(sc[j], o, 64);
#pragma unroll
            for (int j = 0; j < KCACHE; ++j)
                if (lane == j && j < k) pw[h * k + j] = lower_ids[n + i * k + j] == 0 ? -1e10f : sc[j] * scale;      // modules.py:173, :176-184
        }
    }
#pragma unroll
    for (int j = 0; j < (KCACHE > 0 ? 0 : 1 << 30); ++j) {
        if (j >= k) break;
        const int64_t r = i * k + j;
        f4 xv[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; ++c) xv[c] = vc[c] ? fetch(r, lane + 64 * c) : zero;
        for (int h = 0; h < H; ++h) {
            const f4* qh = reinterpret_cast<const f4*>(qk + ((size_t)i * H + h) * Dkv);
            float sc = vc[0] ? dot4(qh[lane], xv[0]) : 0.f;
#pragma unroll
            for (int c = 1; c < NCOL; ++c) sc += vc[c] ? dot4(qh[lane + 64 * c], xv[c]) : 0.f;
            sc = wave_sum(sc);
            if (lane == 0) {
                sc *= scale;                                              // modules.py:173
                if (lower_ids[n + r] == 0) sc = -1e10f;                   // modules.py:176-184
                pw[h * k + j] = sc;
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int hh = lane; hh < H; hh += kWave) {                       // H may exceed the wave (up to 68 heads of 4 at Dq = 272)
        float mx = -INFINITY;
        for (int j = 0; j < k; ++j) mx = fmaxf(mx, pw[hh * k + j]);
        float sum = 0.f;
        for (int j = 0; j < k; ++j) { const float e = expf(pw[hh * k + j] - mx); pw[hh * k + j] = e; sum += e; }
        const float inv = 1.0f / sum;
        for (int j = 0; j < k; ++j) pw[hh * k + j] *= inv;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int h = 0; h < H; ++h) {
        f4 za[NCOL];
#pragma unroll
        for (int c = 0; c < NCOL; ++c) za[c] = zero;
#pragma unroll
        for (int j = 0; j < (KCACHE > 0 ? KCACHE : 1 << 30); ++j) {
            if (j >= k) break;
            const int64_t r = i * k + j;
            const float p = pw[h * k + j];
#pragma unroll
            for (int c = 0; c < NCOL; ++c) {
                if (KCACHE == 0 && !vc[c]) continue;
                const f4 xv = KCACHE > 0 ? xs[j][c] : fetch(r, lane + 64 * c);
                za[c].x = fmaf(p, xv.x, za[c].x); za[c].y = fmaf(p, xv.y, za[c].y); za[c].z = fmaf(p, xv.z, za[c].z); za[c].w = fmaf(p, xv.w, za[c].w);
            }
        }
        f4* zo = reinterpret_cast<f4*>(z + ((size_t)i * H + h) * Dkv);
#pragma unroll
        for (int c = 0; c < NCOL; ++c)
            if (vc[c]) zo[lane + 64 * c] = za[c];
    }
}

// The same attention with TWO waves per node (k <= KC, H <= 2, Dkv <= 512; tgat_attn.h: attn::pair_node).  Workgroup = 2 nodes.
template <int KC, bool FULL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_tgat_attn_pair(const float* __restrict__ qk, const float* __restrict__ h_lower, const float* __restrict__ node_feat,
                                                          const float* __restrict__ edge_feat, const int32_t* __restrict__ lower_ids,
                                                          const int32_t* __restrict__ nbr_eid, const float* __restrict__ nbr_dt, const float* __restrict__ tw,
                                                          const float* __restrict__ tb, int64_t n, int k, int Fn, int Fe, int Ft, int H, float scale,
                                                          float* __restrict__ z, const int32_t* __restrict__ n_live, const int32_t* __restrict__ lower_map) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int64_t i = (int64_t)blockIdx.x * 2 + (wave >> 1);
    const int64_t nl = n_live ? (int64_t)*n_live : n;      // entries in use (a de-duplicated level keeps the layout size n)
    if ((int64_t)blockIdx.x * 2 >= nl) return;              // whole workgroup beyond the live entries
    const bool live = i < nl;
    if (!live) i = nl - 1;                                  // keeps the barrier uniform; nothing is written
    const int Dkv = Fn + Fe + Ft;
    attn::pair_node<KC, FULL>(qk, h_lower, node_feat, edge_feat, lower_ids, nbr_eid, nbr_dt, tw, tb, n, k, Fn, Fe, Ft, H, scale, lower_map, i, live, false, wave, 4, lane,
                        reinterpret_cast<float*>(smem), z + (size_t)i * H * Dkv, Dkv);
}

// The query input of a node is [h(node) | timeenc(0)] (models/TGAT.py:84, models/modules.py:150-157) and timeenc(0) = cos(b) is the SAME vector
// for every row: q = W_q [h | cos(b)] = W_q[:, :Fn] h + W_q[:, Fn:] cos(b).  The second term is a constant of the call (cq, the bias of the
// product over the Fn feature columns, which gathers its rows itself: no [n][Fn + Ft] query-input matrix is written or read), and the
// residual branch of the layer (models/modules.py:196-199) rebuilds [h | cos(b)] from the feature row and ct = cos(b).
__global__ void k_tgat_const_q(const float* __restrict__ Wq, const float* __restrict__ tw, const float* __restrict__ tb, int Dq, int Fn, int Ft,
                               float* __restrict__ cq, float* __restrict__ ct) {
    // one wave per output row (4 per workgroup): lanes stride over the Ft time columns (coalesced), partial sums meet by shuffles in a fixed order
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0) for (int f = threadIdx.x; f < Ft; f += blockDim.x) ct[f] = cosf(fmaf(0.0f, tw[f], tb[f]));
    if (j >= Dq) return;
    float a = 0.f;
    for (int f = lane; f < Ft; f += 64) a = fmaf(Wq[(size_t)j * Dq + Fn + f], cosf(fmaf(0.0f, tw[f], tb[f])), a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if (lane == 0) cq[j] = a;
}

// y = LayerNorm(fc_out + residual) (models/modules.py:196-199), written into the first Dq columns of the MergeLayer input
// row [Dq + Fn]; the raw node features fill the rest (models/TGAT.py:134, models/modules.py:64).  residual = [h(node) | cos(b)]: h from the
// layer below (h_lower, through the row map of a de-duplicated level) or, for layer 1, the raw feature row itself
__global__ __launch_bounds__(256) void k_tgat_post(const float* __restrict__ fc_out, const float* __restrict__ h_lower, const int32_t* __restrict__ lower_map,
                                                     const float* __restrict__ ct, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ node_feat,
                                                     const int32_t* __restrict__ lower_ids, int64_t n, int Dq, int Fn, float* __restrict__ merge_in,
                                                     const int32_t* __restrict__ n_live) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n || (n_live && i >= *n_live)) return;
    // the row lives in registers (Dq <= 272: five elements per lane) between the three passes; a lane adds its elements in the order of the
    // three-loop form this replaces, so the bits are the same
    constexpr int NV = 5;
    float x[NV];
    const float* raw = node_feat + (size_t)lower_ids[i] * Fn;
    const float* hrow = h_lower ? h_lower + (lower_map ? (int64_t)lower_map[i] : i) * Fn : raw;
    float rv[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + kWave * u;
        rv[u] = f < Fn ? raw[f] : 0.f;
        const float res = f < Fn ? (h_lower ? hrow[f] : rv[u]) : (f < Dq ? ct[f - Fn] : 0.f);
        x[u] = f < Dq ? fc_out[i * Dq + f] + res : 0.f;
    }
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + kWave * u < Dq) s += x[u];
    const float mean = wave_sum(s) / (float)Dq;
    float v = 0.f;
#pragma unroll
    for (int u = 0; u < NV; ++u)
        if (lane + kWave * u < Dq) { const float d = x[u] - mean; v = fmaf(d, d, v); }
    const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)Dq + 1e-5f);
    float* o = merge_in + i * (Dq + Fn);
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int f = lane + kWave * u;
        if (f < Dq) o[f] = (x[u] - mean) * rstd * gamma[f] + beta[f];
        if (f < Fn) o[Dq + f] = rv[u];
    }
}

// ---- de-duplication of a level (recent sampling only) --------------------------------------------------------------------
// Entries of a level are (node, time) queries.  With `recent` sampling an entry's embedding is a function of that pair alone, and
// the level below the roots repeats itself: consecutive interactions of a node share 19 of their 20 most recent neighbours, and
// both endpoints of an edge list it (at Reddit shape, 16 steps per call: 128,000 queries, 46,000 distinct).  Distinct entries
// are found with an open-addressing table keyed by (node, time bits): the first thread to claim a slot is the representative,
// every other entry with an equal key maps to it.  Which duplicate wins is a race, but all of them would compute the same row,
// so results do not depend on it.  canon[i] = representative entry; the representatives are then numbered (cidx) and copied
// into the compact level (cids, ctimes); map[i] = compact index of entry i.
__device__ __forceinline__ uint32_t dedup_hash(int32_t id, double t) {
    uint64_t z = (uint64_t)__double_as_longlong(t) ^ ((uint64_t)(uint32_t)id * 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(z ^ (z >> 31));
}
__global__ void k_dedup_insert(const int32_t* __restrict__ ids, const double* __restrict__ times, int64_t n, int32_t* __restrict__ slots, uint32_t cap_mask,
                               int32_t* __restrict__ canon) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t id = ids[i];
    const double t = times[i];
    uint32_t h = dedup_hash(id, t) & cap_mask;
    for (;;) {
        // look before claiming: a level repeats its popular (node, time) entries hundreds of times, and a compare-and-swap per duplicate on the
        // representative's slot serialises them (~8 ns each); a slot never changes once claimed, so a plain read of a claimed slot is final
        int32_t prev = __atomic_load_n(&slots[h], __ATOMIC_RELAXED);
        if (prev == -1) prev = atomicCAS(&slots[h], -1, (int32_t)i);
        if (prev == -1) { canon[i] = (int32_t)i; return; }
        if (ids[prev] == id && __double_as_longlong(times[prev]) == __double_as_longlong(t)) { canon[i] = prev; return; }
        h = (h + 1) & cap_mask;
    }
}
__global__ void k_dedup_number(const int32_t* __restrict__ ids, const double* __restrict__ times, const int32_t* __restrict__ canon, int64_t n,
                               int32_t* __restrict__ count, int32_t* __restrict__ cidx, int32_t* __restrict__ cids, double* __restrict__ ctimes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool rep = i < n && canon[i] == (int32_t)i;
    // ONE atomic per 1024-thread workgroup reserves the compact indices of its representatives: lanes count inside their wave (ballot), waves
    // inside the workgroup (LDS).  Same-address device atomics cost ~8 ns each here: one per representative was 54 us for 10^5 of them, one
    // per wave still 51 us.
    __shared__ int32_t s_cnt, s_base;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t m = __ballot(rep);
    int32_t off = 0;
    if (lane == 0 && m) off = atomicAdd(&s_cnt, __popcll(m));
    off = __shfl(off, 0, 64);
    __syncthreads();
    if (threadIdx.x == 0) s_base = s_cnt ? atomicAdd(count, s_cnt) : 0;
    __syncthreads();
    if (!rep) return;
    const int32_t c = s_base + off + __popcll(m & ((1ull << lane) - 1));
    cidx[i] = c;
    cids[c] = ids[i];
    ctimes[c] = times[i];
}
__global__ void k_dedup_map(const int32_t* __restrict__ canon, const int32_t* __restrict__ cidx, int64_t n, int32_t* __restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) map[i] = cidx[canon[i]];
}

__global__ void k_split_out(const float* __restrict__ h, int64_t B, int Fn, float* __restrict__ out_src, float* __restrict__ out_dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * B * Fn) return;
    const int64_t r = i / Fn;
    (r < B ? out_src : out_dst)[(r < B ? r : r - B) * Fn + i % Fn] = h[i];
}

struct TgatPlan {
    int L, k, Fn, Fe, Ft, H, hd, Dq, Dkv;
    int64_t n[DYGNN_MAX_LAYERS + 1];       // level sizes: n[L] = 2B, n[l-1] = n[l] * (1 + k)
    // byte offsets
    size_t ids[DYGNN_MAX_LAYERS + 1], times[DYGNN_MAX_LAYERS + 1], eid[DYGNN_MAX_LAYERS + 1], dt[DYGNN_MAX_LAYERS + 1], h[DYGNN_MAX_LAYERS + 1];
    size_t q_in, q, att, fc, merge_in, hid, qk, z, pack, cq, total;
    // de-duplication of level L-1 (two-layer models, recent sampling): hash slots, representative / compact index / map per entry, compact level
    size_t dd_slots, dd_canon, dd_cidx, dd_map, dd_count, dd_ids, dd_times;
    uint32_t dd_cap;
};

static TgatPlan make_tgat_plan(const dygnn_tgat_config& c, int64_t B) {
    TgatPlan p{};
    p.L = c.num_layers; p.k = c.num_neighbors; p.Fn = c.node_feat_dim; p.Fe = c.edge_feat_dim; p.Ft = c.time_feat_dim; p.H = c.num_heads;
    p.Dq = p.Fn + p.Ft; p.Dkv = p.Fn + p.Fe + p.Ft; p.hd = p.H > 0 ? p.Dq / p.H : 0;
    p.n[p.L] = 2 * B;
    for (int l = p.L; l >= 1; --l) p.n[l - 1] = p.n[l] * (1 + p.k);
    Carve ws;
    for (int l = 0; l <= p.L; ++l) {
        p.ids[l] = ws.take(p.n[l] * sizeof(int32_t));
        p.times[l] = ws.take(p.n[l] * sizeof(double));
        p.h[l] = l >= 1 ? ws.take((size_t)p.n[l] * p.Fn * sizeof(float)) : 0;
        p.eid[l] = l >= 1 ? ws.take((size_t)p.n[l] * p.k * sizeof(int32_t)) : 0;
        p.dt[l] = l >= 1 ? ws.take((size_t)p.n[l] * p.k * sizeof(float)) : 0;
    }
    const int64_t nmax = p.L >= 1 ? p.n[1] : 0;                        // the largest computed level
    p.q_in = ws.take((size_t)nmax * p.Dq * sizeof(float));
    p.qk = ws.take((size_t)nmax * p.H * p.Dkv * sizeof(float));
    p.z = ws.take((size_t)nmax * p.H * p.Dkv * sizeof(float));
    p.q = ws.take((size_t)nmax * p.Dq * sizeof(float));
    p.att = ws.take((size_t)nmax * p.Dq * sizeof(float));
    p.fc = ws.take((size_t)nmax * p.Dq * sizeof(float));
    p.merge_in = ws.take((size_t)nmax * (p.Dq + p.Fn) * sizeof(float));
    p.hid = ws.take((size_t)nmax * p.Fn * sizeof(float));
    p.cq = ws.take((size_t)(p.L > 0 ? p.L : 1) * (p.Dq + p.Ft) * sizeof(float));      // per layer: the query's constant term [Dq] | cos(b) [Ft]
    if (p.L == 2) {
        p.dd_cap = 1024;
        while ((int64_t)p.dd_cap < 2 * p.n[1]) p.dd_cap <<= 1;
        p.dd_slots = ws.take((size_t)p.dd_cap * sizeof(int32_t));
        p.dd_canon = ws.take((size_t)p.n[1] * sizeof(int32_t));
        p.dd_cidx = ws.take((size_t)p.n[1] * sizeof(int32_t));
        p.dd_map = ws.take((size_t)p.n[1] * sizeof(int32_t));
        p.dd_count = ws.take(sizeof(int32_t));
        p.dd_ids = ws.take((size_t)p.n[1] * sizeof(int32_t));
        p.dd_times = ws.take((size_t)p.n[1] * sizeof(double));
    }
    // packed weight fragments of the row-block chains (tgat_chain.h), with room for the GRU of a TGN call
    p.pack = ws.take(chain::pack_bytes(chain::plan_pack(p.L, p.Fn, p.Ft, p.Dkv, p.H > 0 ? p.H : 1, 2 * p.Fn + p.Ft + p.Fe)));
    p.total = ws.o;
    return p;
}

int check_tgat(const dygnn_tgat_config* c) {      // (also the training path's check, tgat_train.hip)
    DYGNN_REQUIRE(c != nullptr, "tgat: config is NULL");
    DYGNN_REQUIRE(c->node_feat_dim > 0 && c->edge_feat_dim > 0 && c->time_feat_dim > 0, "tgat: feature dims must be positive");
    DYGNN_REQUIRE(c->node_feat_dim % 4 == 0 && c->edge_feat_dim % 4 == 0 && c->time_feat_dim % 4 == 0, "tgat: feature dims must be multiples of 4");
    DYGNN_REQUIRE(c->num_layers >= 1 && c->num_layers <= 3, "tgat: num_layers must be in [1,3]");
    // models/modules.py:120
    DYGNN_REQUIRE(c->num_heads >= 1 && (c->node_feat_dim + c->time_feat_dim) % c->num_heads == 0,
                  "The sum of node_feat_dim and time_feat_dim should be divided by num_heads!");
    // utils/utils.py:157
    DYGNN_REQUIRE(c->num_neighbors > 0, "Number of sampled neighbors for each node should be greater than 0!");
    DYGNN_REQUIRE(c->num_neighbors <= 64, "tgat: num_neighbors > 64 not supported");
    DYGNN_REQUIRE(c->node_feat_dim + c->time_feat_dim <= 16 * 17, "tgat: node_feat_dim + time_feat_dim > 272 not supported");
    DYGNN_REQUIRE(((c->node_feat_dim + c->time_feat_dim) / c->num_heads) % 4 == 0, "tgat: head dim must be a multiple of 4");
    // the attention kernels hold an input row [h | edge | time] as at most four float4 columns per lane (k_tgat_attn_lin, tgat_train.hip: NC)
    DYGNN_REQUIRE((int64_t)c->node_feat_dim + c->edge_feat_dim + c->time_feat_dim <= 1024, "tgat: node_feat_dim + edge_feat_dim + time_feat_dim > 1024 not supported");
    return DYGNN_OK;
}

int check_layer_weights(const dygnn_tgat_weights* w, int L, const char* what) {
    for (int l = 0; l < L; ++l) {
        const dygnn_tgat_layer_weights& Lw = w->layers[l];
        DYGNN_REQUIRE(Lw.query_w && Lw.key_w && Lw.value_w && Lw.ln_w && Lw.ln_b && Lw.res_w && Lw.res_b && Lw.fc1_w && Lw.fc1_b && Lw.fc2_w && Lw.fc2_b,
                      "%s (layer %d)", what, l);
    }
    return DYGNN_OK;
}

int copy_levels(hipStream_t s, const dygnn_tgat_levels* lv, int L, int k, const int64_t* n, int id_levels, const LevelBufs& to, const char* what) {
    for (int l = 0; l <= L; ++l)
        DYGNN_REQUIRE((l >= id_levels || lv->ids[l]) && (l == 0 || (lv->nbr_eid[l] && lv->nbr_dt[l])), "%s: null level array (level %d)", what, l);
    for (int l = 0; l <= L; ++l) {
        if (l < id_levels) DYGNN_HIP(hipMemcpyAsync(to.ids[l], lv->ids[l], (size_t)n[l] * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        if (l >= 1) {
            DYGNN_HIP(hipMemcpyAsync(to.eid[l], lv->nbr_eid[l], (size_t)n[l] * k * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
            DYGNN_HIP(hipMemcpyAsync(to.dt[l], lv->nbr_dt[l], (size_t)n[l] * k * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    return DYGNN_OK;
}

// the de-duplication of level 1 (see k_dedup_insert): hash slots, representative / compact index / map per entry, the compact level
struct DedupBufs {
    int32_t *slots, *canon, *cidx, *map, *count, *ids;
    double* times;
    uint32_t cap;
};

int expand_levels(hipStream_t s, const dygnn_csr* csr, const TgatRoots& r, int L, int k, const LevelBufs& to, const DedupBufs* dd, const TgnTouch* touch) {
    int64_t n = 2 * r.B;
    for (int l = L; l >= 1; --l, n *= 1 + k) {
        const bool top = l == L;
        const bool d1 = dd && l == 1;             // level 1 is expanded from its distinct entries only
        hipLaunchKernelGGL(k_tgat_expand, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, csr->indptr, csr->nbr, csr->eid, csr->ts, csr->num_nodes,
                           d1 ? dd->ids : to.ids[l], d1 ? dd->times : to.times[l], n, k, to.ids[l - 1], to.times[l - 1], to.eid[l], to.dt[l],
                           d1 ? dd->count : (const int32_t*)nullptr, top ? r.src : nullptr, top ? r.dst : nullptr, top ? r.times : nullptr, r.B,
                           touch && l == 1 ? *touch : TgnTouch{}, r.per_root ? 1 : 0);
        DYGNN_LAUNCH_CHECK();
        if (dd && l == 2) {                       // level 1 is complete: find its distinct (node, time) entries
            const int64_t n1 = n * (1 + k);
            DYGNN_HIP(hipMemsetAsync(dd->slots, 0xFF, (size_t)dd->cap * sizeof(int32_t), s));
            DYGNN_HIP(hipMemsetAsync(dd->count, 0, sizeof(int32_t), s));
            hipLaunchKernelGGL(k_dedup_insert, dim3((unsigned)ceil_div(n1, 256)), dim3(256), 0, s, to.ids[1], to.times[1], n1, dd->slots, dd->cap - 1, dd->canon);
            DYGNN_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_dedup_number, dim3((unsigned)ceil_div(n1, 1024)), dim3(1024), 0, s, to.ids[1], to.times[1], dd->canon, n1, dd->count, dd->cidx,
                               dd->ids, dd->times);
            DYGNN_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_dedup_map, dim3((unsigned)ceil_div(n1, 256)), dim3(256), 0, s, dd->canon, dd->cidx, n1, dd->map);
            DYGNN_LAUNCH_CHECK();
        }
    }
    return DYGNN_OK;
}

template <bool RELU>
static int gemm_nt(const float* A, const float* W, const float* bias, float* C, int64_t M, int N, int K, int ldc, hipStream_t s, const int32_t* m_dev = nullptr) {
    if (M == 0) return DYGNN_OK;
    if (M >= 48 || m_dev) return train::mm(s, A, K, false, W, K, true, C, ldc, (int)M, N, K, train::MmOpt().bias(bias).relu(RELU).live_rows(m_dev));      // the LDS-tiled general GEMM
    hipLaunchKernelGGL((k_gemm_nt<RELU>), dim3((unsigned)ceil_div(M, 256), (unsigned)ceil_div(N, 64)), dim3(256), 0, s, A, W, bias, C, M, N, K, ldc);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_tgat_workspace_bytes(const dygnn_tgat_config* cfg, int64_t batch) {
    if (check_tgat(cfg) != DYGNN_OK || batch < 0) return 0;
    return make_tgat_plan(*cfg, batch).total;
}

namespace dygnn {
size_t tgat_plan_bytes(const dygnn_tgat_config& cfg, int64_t batch) { return make_tgat_plan(cfg, batch).total; }

// Distinct entries of level 1 are computed once (see k_dedup_insert): only when the library samples itself (`recent` is a function of
// (node, time); pre-sampled random levels draw independently per entry) and the pair attention kernel, which knows the row map, applies.
// Decided once per library call, by its entry point.
static bool tgat_dedup_active(const dygnn_tgat_config& c, bool presampled) {
    const char* dd_env = getenv("DYGNN_TGAT_DEDUP");                 // "0" switches it off (read per call: the A/B switch of tests/test_tgat.py)
    const bool dedup_on = !(dd_env && dd_env[0] == '0');
    return dedup_on && !presampled && c.num_layers == 2 && c.num_neighbors <= 20 && c.num_heads <= 2 &&
           c.node_feat_dim + c.edge_feat_dim + c.time_feat_dim <= 512;
}
TgatStages tgat_stages(const dygnn_tgat_config& cfg, int64_t batch, void* workspace, hipStream_t s, bool presampled) {
    return TgatStages{cfg, batch, static_cast<char*>(workspace), s, tgat_dedup_active(cfg, presampled)};
}

int check_tgat_args(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_csr* csr, const dygnn_tgat_levels* levels, const float* node_feat,
                    const float* edge_feat, const TgatRoots& r, const float* out_src, const float* out_dst, const void* workspace, size_t workspace_bytes) {
    if (int rc = check_tgat(cfg)) return rc;
    DYGNN_REQUIRE(w && w->time_w && w->time_b, "tgat: null weights");
    DYGNN_REQUIRE(levels || (csr && csr->indptr && csr->num_nodes >= 1), "tgat: bad csr");
    DYGNN_REQUIRE(r.B >= 0 && node_feat && edge_feat, "tgat: bad arguments");
    if (r.B == 0) return DYGNN_OK;
    DYGNN_REQUIRE((levels || (r.src && r.dst && r.times)) && out_src && out_dst && workspace, "tgat: null pointer");
    const size_t need = make_tgat_plan(*cfg, r.B).total;
    if (workspace_bytes < need) {
        set_error("tgat: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
        return DYGNN_E_WORKSPACE;
    }
    return check_layer_weights(w, cfg->num_layers, "tgat: null layer weights");
}

TgatLevel0 tgat_level0(const TgatStages& c) {
    const TgatPlan p = make_tgat_plan(c.cfg, c.B);
    return TgatLevel0{reinterpret_cast<const int32_t*>(c.ws + p.ids[0]), c.dedup ? reinterpret_cast<const int32_t*>(c.ws + p.dd_count) : nullptr, p.n[0], p.n[1],
                      reinterpret_cast<float*>(c.ws + p.pack)};
}

int tgat_levels(const TgatStages& c, const dygnn_csr* csr, const TgatRoots& roots, const dygnn_tgat_levels* levels, const TgnTouch* touch) {
    const TgatPlan p = make_tgat_plan(c.cfg, c.B);
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(c.ws + off); };
    auto F64 = [&](size_t off) { return reinterpret_cast<double*>(c.ws + off); };
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(c.ws + off); };
    LevelBufs to{};
    for (int l = 0; l <= p.L; ++l) {
        to.ids[l] = I32(p.ids[l]); to.times[l] = F64(p.times[l]);
        if (l >= 1) { to.eid[l] = I32(p.eid[l]); to.dt[l] = F32(p.dt[l]); }
    }
    if (!levels) {
        const DedupBufs dd{I32(p.dd_slots), I32(p.dd_canon), I32(p.dd_cidx), I32(p.dd_map), I32(p.dd_count), I32(p.dd_ids), F64(p.dd_times), p.dd_cap};
        return expand_levels(c.s, csr, roots, p.L, p.k, to, c.dedup ? &dd : nullptr, touch);
    }
    // pre-sampled levels (random strategies): copied where the sampling kernels would have written them
    if (int rc = copy_levels(c.s, levels, p.L, p.k, p.n, p.L + 1, to, "tgat")) return rc;
    if (touch) {
        if (int rc = tgn_touch_levels(c.s, to.ids[0], p.n[1], p.k, *touch)) return rc;
    }
    return DYGNN_OK;
}

// The one-wave-per-node attention (k_tgat_attn_lin) for what the two-wave kernel does not take: more than 20 neighbours (row slots in LDS),
// more than two heads (k <= 20: rows in registers), Dkv > 512 (four float4 columns per lane; rows re-gathered).  Its LDS ([4][H][k] scores,
// plus [4][20][Ft] time encodings with rows in registers) exceeds the default 64 KiB for many heads or time features (H = 68 at k = 64:
// 68 KiB; H = 4, Ft = 268: 85 KiB); check_tgat's bounds keep it under 160 KiB.
template <int KC, int NCOL>
static int launch_attn_lin_t(hipStream_t s, const TgatPlan& p, size_t lds, const float* qk, const float* h_lower, const float* node_feat,
                             const float* edge_feat, const int32_t* ids, const int32_t* eid, const float* dt, const float* tw, const float* tb, int64_t n,
                             float scale, float* z) {
    if (lds > 64 * 1024) DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tgat_attn_lin<KC, NCOL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((k_tgat_attn_lin<KC, NCOL>), dim3((unsigned)ceil_div(n, 4)), dim3(256), lds, s, qk, h_lower, node_feat, edge_feat, ids, eid, dt, tw, tb, n,
                       p.k, p.Fn, p.Fe, p.Ft, p.H, scale, z);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
static int launch_attn_lin(hipStream_t s, const TgatPlan& p, const float* qk, const float* h_lower, const float* node_feat, const float* edge_feat,
                           const int32_t* ids, const int32_t* eid, const float* dt, const float* tw, const float* tb, int64_t n, float scale, float* z) {
    const size_t lds = (size_t)4 * p.H * p.k * sizeof(float);
    if (p.Dkv > 4 * 64 * 2) return launch_attn_lin_t<0, 4>(s, p, lds, qk, h_lower, node_feat, edge_feat, ids, eid, dt, tw, tb, n, scale, z);
    if (p.k <= 20)
        return launch_attn_lin_t<20, 2>(s, p, lds + (size_t)4 * 20 * p.Ft * sizeof(float), qk, h_lower, node_feat, edge_feat, ids, eid, dt, tw, tb, n, scale, z);
    return launch_attn_lin_t<0, 2>(s, p, lds, qk, h_lower, node_feat, edge_feat, ids, eid, dt, tw, tb, n, scale, z);
}

int tgat_layers(const TgatStages& c, const dygnn_tgat_weights* w, const float* node_feat, const float* edge_feat, float* out_src, float* out_dst, bool packed) {
    const TgatPlan p = make_tgat_plan(c.cfg, c.B);
    const hipStream_t s = c.s;
    const bool dedup = c.dedup;
    const int64_t B = p.n[p.L] / 2;
    auto I32 = [&](size_t off) { return reinterpret_cast<int32_t*>(c.ws + off); };
    auto F32 = [&](size_t off) { return reinterpret_cast<float*>(c.ws + off); };
    // bottom-up: layer l turns level-(l-1) embeddings (raw features for l = 1) into level-l embeddings
    const float scale = (float)pow((double)p.hd, -0.5);
    // Two forms of a layer.  Row-block chains (tgat_chain.hip; three launches, intermediates in LDS): every workgroup streams the layer's
    // 2 MB of weights through its own CU, which pays when a level has few rows -- TGN calls (one step of a few hundred roots; they come
    // with their weights packed).  Product by product through the general GEMM: TGAT's levels of 10^4..10^5 rows.  The choice depends on
    // the caller, never on the batch, so a row keeps its bits at every batch size; DYGNN_TGAT_CHAIN=0/1 forces one (A/B switch, read per call).
    const char* ch_env = getenv("DYGNN_TGAT_CHAIN");
    // chain_from: the first layer that runs as chains.  TGN: all (1).  TGAT: none (L + 1); DYGNN_TGAT_CHAIN=1: all, =2: the top layer only (the
    // roots: a few hundred rows per evaluation step) -- by layer, never by batch size.
    const bool fits = chain::fits(p.Fn, p.Ft, p.Dkv, p.H);
    int chain_from = packed ? 1 : p.L + 1;
    if (ch_env && ch_env[0] >= '0' && ch_env[0] <= '2') chain_from = ch_env[0] == '0' ? p.L + 1 : ch_env[0] == '1' ? 1 : p.L;
    if (!fits) chain_from = p.L + 1;
    const chain::PackPlan pp = chain::plan_pack(p.L, p.Fn, p.Ft, p.Dkv, p.H, 2 * p.Fn + p.Ft + p.Fe);
    if (chain_from <= p.L && !packed)
        if (int rc = chain::pack(s, pp, p.L, p.Fn, p.Ft, p.Dkv, p.H, w, nullptr, 0, F32(p.pack))) return rc;
    for (int l = 1; l <= p.L; ++l) {
        const bool chain = l >= chain_from;
        const dygnn_tgat_layer_weights& Lw = w->layers[l - 1];
        const int64_t n = p.n[l];
        const float* h_lower = l >= 2 ? F32(p.h[l - 1]) : nullptr;
        const int32_t* nl = dedup && l == 1 ? I32(p.dd_count) : nullptr;       // layer 1 runs over the distinct level-1 entries (count on the device)
        const int32_t* lmap = dedup && l == 2 ? I32(p.dd_map) : nullptr;       // layer 2 finds an entry's layer-1 row through the map
        // the top level is [src rows ; dst rows]: when the caller's two outputs are one [2B, Fn] block it is written in place
        const bool direct = l == p.L && out_dst == out_src + (size_t)B * p.Fn;
        float* h_out = direct ? out_src : F32(p.h[l]);
        float* cq = F32(p.cq) + (size_t)(l - 1) * (p.Dq + p.Ft);
        float* ct = cq + p.Dq;
        if (chain) {
            // q_in -> q -> W_k^T q inside one workgroup per 16 / 32 rows (tgat_chain.hip): intermediates stay in LDS
            chain::PreArgs pa{h_lower, node_feat, I32(p.ids[l - 1]), lmap, nl, w->time_w, w->time_b, F32(p.pack), pp.layer[l - 1].q, pp.layer[l - 1].k, F32(p.qk), n,
                              p.Fn, p.Ft, p.Dkv, p.H};
            if (int rc = chain::launch_pre(s, pa)) return rc;
        } else {
        // q = W_q[:, :Fn] h + cq (see k_tgat_const_q): the product gathers the feature rows itself
        hipLaunchKernelGGL(k_tgat_const_q, dim3((unsigned)ceil_div(p.Dq, 4)), dim3(256), 0, s, Lw.query_w, w->time_w, w->time_b, p.Dq, p.Fn, p.Ft, cq, ct);
        DYGNN_LAUNCH_CHECK();
        const float* qa = h_lower ? h_lower : node_feat;
        if (n >= 48 && train::mm_gathers_rows(qa, p.Fn, Lw.query_w, p.Dq, (int)n, p.Dq, p.Fn)) {
            if (int rc = train::mm(s, qa, p.Fn, false, Lw.query_w, p.Dq, true, F32(p.q), p.Dq, (int)n, p.Dq, p.Fn,
                                   train::MmOpt().bias(cq).live_rows(nl).rows(h_lower ? lmap : I32(p.ids[l - 1])))) return rc;
        } else {      // a handful of rows, or a product the row-gathering kernel cannot take (Dq < 48, DYGNN_MM_DMA=0, unaligned feature table): the
                      // feature rows are staged ([n][Fn], Ft = 0: no time columns), then the small-M kernel
            hipLaunchKernelGGL(k_tgat_qrows, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, h_lower, node_feat, I32(p.ids[l - 1]), w->time_w, w->time_b, n, p.Fn, 0,
                               F32(p.q_in), nl, lmap);
            DYGNN_LAUNCH_CHECK();
            hipLaunchKernelGGL((k_gemm_nt<false>), dim3((unsigned)ceil_div(n, 256), (unsigned)ceil_div(p.Dq, 64)), dim3(256), 0, s, F32(p.q_in), Lw.query_w, cq, F32(p.q), n,
                               p.Dq, p.Fn, p.Dq, p.Dq);
            DYGNN_LAUNCH_CHECK();
        }
        // qk[i][h] = W_k,h^T q_ih : per head [n][hd] x [hd][Dkv] (rows h*hd .. of key_w), one batched launch over the heads
        if (int rc = train::mm(s, F32(p.q), p.Dq, false, Lw.key_w, p.Dkv, false, F32(p.qk), p.H * p.Dkv, (int)n, p.Dkv, p.hd,
                               train::MmOpt().batched(p.H, p.H).strideA(0, p.hd).strideB(0, (int64_t)p.hd * p.Dkv).strideC(0, p.Dkv).live_rows(nl))) return rc;
        }
        const bool attn_in_post = chain && chain::post_fuses_attention(n, p.Fn, p.Ft, p.Dkv, p.H, p.k);      // the chain's last kernel runs it on its own rows
        if (attn_in_post) {
        } else if (p.k <= 20 && p.H <= 2 && p.Dkv <= 512) {
            const int TW = 4 * ((p.Ft / 4 + 1) / 2);
            // KC = the row slots a lane keeps in registers: 10 for k <= 10 (TGN's configuration; half the gathers of the 20-slot form, whose
            // idle slots re-read row 0), 20 otherwise.  Idle slots contribute exact zeros, so a row's bits do not depend on KC.
            const int KC = p.k <= 10 ? 10 : 20;
            const size_t lds2 = ((size_t)8 * p.H * KC + (size_t)4 * KC * TW) * sizeof(float);
            // (k == KC: the instantiation without idle row slots; the bits of a row are the same)
#define DYGNN_ATTN_LAUNCH(KC_, FULL_)                                                                                                                           \
    hipLaunchKernelGGL((k_tgat_attn_pair<KC_, FULL_>), dim3((unsigned)ceil_div(n, 2)), dim3(256), lds2, s, F32(p.qk), h_lower, node_feat, edge_feat, I32(p.ids[l - 1]), \
                       I32(p.eid[l]), F32(p.dt[l]), w->time_w, w->time_b, n, p.k, p.Fn, p.Fe, p.Ft, p.H, scale, F32(p.z), nl, lmap)
            if (KC == 10) { if (p.k == 10) DYGNN_ATTN_LAUNCH(10, true); else DYGNN_ATTN_LAUNCH(10, false); }
            else { if (p.k == 20) DYGNN_ATTN_LAUNCH(20, true); else DYGNN_ATTN_LAUNCH(20, false); }
#undef DYGNN_ATTN_LAUNCH
        } else if (int rc = launch_attn_lin(s, p, F32(p.qk), h_lower, node_feat, edge_feat, I32(p.ids[l - 1]), I32(p.eid[l]), F32(p.dt[l]), w->time_w, w->time_b, n,
                                            scale, F32(p.z))) return rc;
        DYGNN_LAUNCH_CHECK();
        if (chain) {
            // W_v z -> residual_fc + q_in -> LayerNorm -> MergeLayer, one workgroup per 16 / 32 rows
            const chain::LayerPack& y = pp.layer[l - 1];
            chain::PostArgs po{F32(p.z), h_lower, node_feat, I32(p.ids[l - 1]), lmap, nl, w->time_w, w->time_b, F32(p.pack), y.v, y.r, y.f1, y.f2, Lw.res_b, Lw.ln_w,
                               Lw.ln_b, Lw.fc1_b, Lw.fc2_b, h_out, n, p.Fn, p.Ft, p.Dkv, p.H, nullptr,
                               attn_in_post ? F32(p.qk) : nullptr, edge_feat, I32(p.eid[l]), F32(p.dt[l]), p.k, p.Fe, scale};
#ifdef DYGNN_STAMPS      // diagnostic build only (tools/chain_stamps.py, DYGNN_LIB_VARIANT=stamps): the product library never takes a device address from the environment
            if (const char* st_env = getenv("DYGNN_CHAIN_STAMPS")) po.stamps = reinterpret_cast<unsigned long long*>(strtoull(st_env, nullptr, 0));
#endif
            if (int rc = chain::launch_post(s, po)) return rc;
            if (direct) return DYGNN_OK;
            continue;
        }
        // att[i][h*hd ..] = W_v,h z_ih : per head [n][Dkv] x [Dkv][hd]
        if (int rc = train::mm(s, F32(p.z), p.H * p.Dkv, false, Lw.value_w, p.Dkv, true, F32(p.att), p.Dq, (int)n, p.hd, p.Dkv,
                               train::MmOpt().batched(p.H, p.H).strideA(0, p.Dkv).strideB(0, (int64_t)p.hd * p.Dkv).strideC(0, p.hd).live_rows(nl))) return rc;
        if (int rc = gemm_nt<false>(F32(p.att), Lw.res_w, Lw.res_b, F32(p.fc), n, p.Dq, p.Dq, p.Dq, s, nl)) return rc;
        hipLaunchKernelGGL(k_tgat_post, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, s, F32(p.fc), h_lower, lmap, ct, Lw.ln_w, Lw.ln_b, node_feat, I32(p.ids[l - 1]),
                           n, p.Dq, p.Fn, F32(p.merge_in), nl);
        DYGNN_LAUNCH_CHECK();
        if (int rc = gemm_nt<true>(F32(p.merge_in), Lw.fc1_w, Lw.fc1_b, F32(p.hid), n, p.Fn, p.Dq + p.Fn, p.Fn, s, nl)) return rc;
        if (int rc = gemm_nt<false>(F32(p.hid), Lw.fc2_w, Lw.fc2_b, h_out, n, p.Fn, p.Fn, p.Fn, s, nl)) return rc;
        if (direct) return DYGNN_OK;
    }
    hipLaunchKernelGGL(k_split_out, dim3((unsigned)ceil_div(2 * B * p.Fn, 256)), dim3(256), 0, s, F32(p.h[p.L]), B, p.Fn, out_src, out_dst);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

// dygnn_tgat_forward, _forward_roots and _forward_levels
static int tgat_forward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_csr* csr, const dygnn_tgat_levels* levels,
                        const float* node_feat, const float* edge_feat, const TgatRoots& roots, float* out_src, float* out_dst, void* workspace,
                        size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = check_tgat_args(cfg, w, csr, levels, node_feat, edge_feat, roots, out_src, out_dst, workspace, workspace_bytes)) return rc;
    if (roots.B == 0) return DYGNN_OK;
    const TgatStages c = tgat_stages(*cfg, roots.B, workspace, as_stream(stream), levels != nullptr);
    if (int rc = tgat_levels(c, csr, roots, levels, nullptr)) return rc;
    return tgat_layers(c, w, node_feat, edge_feat, out_src, out_dst, false);
}

}  // namespace dygnn

extern "C" int dygnn_tgat_forward_levels(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_tgat_levels* levels, const float* node_feat,
                                         const float* edge_feat, int64_t batch, float* out_src, float* out_dst, void* workspace, size_t workspace_bytes,
                                         dygnn_stream_t stream) {
    DYGNN_REQUIRE(levels != nullptr, "tgat_forward_levels: levels is NULL");
    return tgat_forward(cfg, w, nullptr, levels, node_feat, edge_feat, TgatRoots{nullptr, nullptr, nullptr, batch, false}, out_src, out_dst, workspace,
                        workspace_bytes, stream);
}

extern "C" int dygnn_tgat_level_entries(const dygnn_tgat_config* cfg, int64_t batch, const void* workspace, int64_t* total, int64_t* computed,
                                        dygnn_stream_t stream) {
    if (int rc = check_tgat(cfg)) return rc;
    DYGNN_REQUIRE(batch > 0 && workspace && total && computed, "tgat_level_entries: bad arguments");
    const TgatPlan p = make_tgat_plan(*cfg, batch);
    *total = 0;
    for (int l = 1; l <= p.L; ++l) *total += p.n[l];
    *computed = *total;
    if (p.L == 2) {
        int32_t u = 0;
        DYGNN_HIP(hipMemcpyAsync(&u, static_cast<const char*>(workspace) + p.dd_count, sizeof(u), hipMemcpyDeviceToHost, as_stream(stream)));
        DYGNN_HIP(hipStreamSynchronize(as_stream(stream)));
        if (u > 0 && u <= p.n[1]) *computed = p.n[2] + u;
    }
    return DYGNN_OK;
}

extern "C" int dygnn_tgat_forward(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_csr* csr, const float* node_feat,
                                  const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times, int64_t batch,
                                  float* out_src, float* out_dst, void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    return tgat_forward(cfg, w, csr, nullptr, node_feat, edge_feat, TgatRoots{src, dst, times, batch, false}, out_src, out_dst, workspace, workspace_bytes,
                        stream);
}

// Embeddings of a LIST of (node, time) roots [n_roots] (n_roots even: the roots are the level [first half ; second half] of n_roots / 2
// "pairs", every root with its own time).  An evaluation step's positive and negative call share their source rows: the caller hands
// [sources ; destinations ; negative destinations] over once instead of [sources ; destinations] + [sources ; negatives].
extern "C" int dygnn_tgat_forward_roots(const dygnn_tgat_config* cfg, const dygnn_tgat_weights* w, const dygnn_csr* csr, const float* node_feat,
                                        const float* edge_feat, const int64_t* ids, const double* times, int64_t n_roots, float* out,
                                        void* workspace, size_t workspace_bytes, dygnn_stream_t stream) {
    DYGNN_REQUIRE(n_roots >= 0 && n_roots % 2 == 0, "tgat_forward_roots: n_roots must be even (pad with a repeated root)");
    DYGNN_REQUIRE(n_roots == 0 || (ids && times && out && cfg), "tgat_forward_roots: null pointer");
    const int64_t b = n_roots / 2;
    return tgat_forward(cfg, w, csr, nullptr, node_feat, edge_feat, TgatRoots{ids, ids + b, times, b, true}, out, out + (size_t)b * (cfg ? cfg->node_feat_dim : 0),
                        workspace, workspace_bytes, stream);
}
