// The link-predictor head every backbone evaluates and trains through: MergeLayer, sigmoid(fc2(relu(fc1(cat(a, b))))) (models/modules.py:57-68).
// Four forward kernels, chosen by the number of rows and the sizes (dygnn_merge_layer_forward_path), one backward kernel, and their C-ABI entry points.
#include "common.h"
#include "gemm.h"

namespace dygnn {

// The head's ReLU: a NaN pre-activation stays NaN as in torch.relu (fmaxf(x, 0) would turn a diverged model's NaN embeddings into
// sigmoid(fc2.bias), a normal-looking score).  Forward kernels only.  IEEE 754-2019 maximum is one v_maximum3_f32 on gfx950; the select
// form is a compare and a v_cndmask.
__device__ __forceinline__ float relu_nan(float x) {
#if __has_builtin(__builtin_elementwise_maximum)
    return __builtin_elementwise_maximum(x, 0.f);
#else
    return x < 0.f ? 0.f : x;
#endif
}

// sigmoid(fc2(relu(fc1(cat(a,b)))))   models/modules.py:57-68 + evaluate_models_utils.py:140-141
__global__ __launch_bounds__(256) void k_merge_sigmoid(const float* __restrict__ a, const float* __restrict__ b, int dim, int hidden,
                                                         const float* __restrict__ w1, const float* __restrict__ b1,
                                                         const float* __restrict__ w2, const float* __restrict__ b2,
                                                         float* __restrict__ out, int sig) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* x = reinterpret_cast<float*>(smem);          // [2*dim]
    float* red = x + 2 * dim;                           // [4]
    const int64_t r = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * dim; i += blockDim.x) x[i] = i < dim ? a[r * dim + i] : b[r * dim + (i - dim)];
    __syncthreads();
    float part = 0.f;
    for (int j = threadIdx.x; j < hidden; j += blockDim.x) {
        float acc = 0.f;
        const float* wr = w1 + (size_t)j * 2 * dim;
        for (int k = 0; k < 2 * dim; ++k) acc = fmaf(x[k], wr[k], acc);
        part = fmaf(relu_nan(acc + b1[j]), w2[j], part);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        float z = b2[0];
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) z += red[wv];
        out[r] = sig ? 1.0f / (1.0f + expf(-z)) : z;
    }
}

// The same head on the matrix cores: one wave = 16 rows.  Transposed product H^T[n][m] = sum_k W1[n][k] cat(a,b)[m][k]
// (A operand = fc1 rows, B operand = the row's features, both K-contiguous float4 reads), four hidden tiles at a time;
// relu, the fc2 dot product and the sigmoid are applied to the accumulators.  Needs dim % 4 == 0.
using mf4 = __attribute__((ext_vector_type(4))) float;
__global__ __launch_bounds__(256) void k_merge_sigmoid_mfma(const float* __restrict__ a, const float* __restrict__ b, int64_t n_rows, int dim,
                                                              int hidden, const float* __restrict__ w1, const float* __restrict__ b1,
                                                              const float* __restrict__ w2, const float* __restrict__ b2,
                                                              float* __restrict__ out, int sig) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * 16;
    if (m0 >= n_rows) return;
    const int64_t m = m0 + c;
    const bool mv = m < n_rows;
    const int K = 2 * dim;
    float z = 0.f;
    for (int n0 = 0; n0 < hidden; n0 += 64) {
        mf4 acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = mf4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < K; k0 += 16) {
            const int kk = k0 + 4 * g;
            mf4 bf = mf4{0.f, 0.f, 0.f, 0.f};
            if (mv && kk < K) bf = kk < dim ? *reinterpret_cast<const mf4*>(a + m * dim + kk) : *reinterpret_cast<const mf4*>(b + m * dim + (kk - dim));
            mf4 af[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n0 + 16 * i + c;
                af[i] = (n < hidden && kk < K) ? *reinterpret_cast<const mf4*>(w1 + (size_t)n * K + kk) : mf4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][t], bf[t], acc[i], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 16 * i + 4 * g + r;
                if (n < hidden) z = fmaf(relu_nan(acc[i][r] + b1[n]), w2[n], z);
            }
    }
    z += __shfl_xor(z, 16, 64);
    z += __shfl_xor(z, 32, 64);
    if (g == 0 && mv) out[m] = sig ? 1.0f / (1.0f + expf(-(z + b2[0]))) : z + b2[0];
}


// The same head for a few hundred rows (one evaluation step: 400 .. 800).  FOUR rows per workgroup and one wave per 16-wide tile of hidden
// units (hidden = 172: 11 waves), on `v_mfma_f32_4x4x1_16b_f32` used as 4 groups of hidden units x 4 slices of k against the four rows
// (tgat_chain.hip has the long form of this): lane L = 16 ng + 4 ks + i holds fc1[16 wave + 4 ng + i][16 chunk + 4 ks ..] -- the 16 lanes of a
// quarter-wave read 4 rows x 64 contiguous bytes (the 16x16x4 form: 16 rows x 16 bytes, four times the L1 lookups per byte) -- and
// multiplies it with cat(a, b)[row j][16 chunk + 4 ks ..] out of LDS.  400 rows = 100 workgroups; a wave's stream is 22 steps.
// (The previous form, 16 rows per workgroup with 4 waves over the hidden units, took 16 us for 400 rows on 25 workgroups: every wave's
// float4 operand loads touched 16 rows, and 4 or 8 k-steps in flight made no difference.)
template <int MT>      // 4 MT rows per workgroup: 4 for an evaluation step's few hundred rows, 16 for thousands (the fc1 stream is shared by more rows)
__global__ __launch_bounds__(1024) void k_merge_sigmoid_rows4(const float* __restrict__ a, const float* __restrict__ b, int64_t n_rows, int dim,
                                                               int hidden, const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, const float* __restrict__ b2,
                                                               float* __restrict__ out, int sig, int ldx) {
    extern __shared__ __attribute__((aligned(16))) float mlds[];
    constexpr int R = 4 * MT;
    float* x = mlds;                      // [R][ldx] cat(a, b) rows, zero-padded to the 16-k chunk
    float* zp = x + R * ldx;              // [waves][R] per-tile parts of the fc2 dot product
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int j = lane & 3, ks = (lane >> 2) & 3, ng = lane >> 4;
    const int K = 2 * dim, nch = (K + 15) >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    const int n_lane = 16 * wave + 4 * ng + j;
    const bool rowok = n_lane < hidden;
    // a lane whose k-slice lies beyond a short row (K = 8: ks = 2, 3) multiplies zeros; its loads stay at the start of its row, inside fc1
    const float* wp = w1 + (size_t)(rowok ? n_lane : 0) * K + (4 * ks < K ? 4 * ks : 0);
    constexpr int PF = 4;
    mf4 ring[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) ring[u] = *reinterpret_cast<const mf4*>(wp + ((16 * u + 4 * ks < K) ? 16 * u : 0));
    for (int rr = wave; rr < R; rr += nwaves) {
        const int64_t m = r0 + rr;
        for (int f = lane; f < ldx; f += 64) x[rr * ldx + f] = (m < n_rows && f < K) ? (f < dim ? a[m * dim + f] : b[m * dim + (f - dim)]) : 0.f;
    }
    __syncthreads();
    mf4 acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = mf4{0.f, 0.f, 0.f, 0.f};
    const float* xb = x + j * ldx + 4 * ks;
    for (int c0 = 0; c0 < nch; c0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int ch = c0 + u;
            if (ch < nch) {
                const bool kok = 16 * ch + 4 * ks < K;
                const mf4 w = (rowok && kok) ? ring[u] : mf4{0.f, 0.f, 0.f, 0.f};
                const int nx = ch + PF;
                ring[u] = *reinterpret_cast<const mf4*>(wp + ((nx < nch && 16 * nx + 4 * ks < K) ? 16 * nx : 0));
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const mf4 xv = *reinterpret_cast<const mf4*>(xb + m * 4 * ldx + 16 * ch);
                    acc[m] = __builtin_amdgcn_mfma_f32_4x4x1f32(w.x, xv.x, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_4x4x1f32(w.y, xv.y, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_4x4x1f32(w.z, xv.z, acc[m], 0, 0, 0);
                    acc[m] = __builtin_amdgcn_mfma_f32_4x4x1f32(w.w, xv.w, acc[m], 0, 0, 0);
                }
            }
        }
    }
    // k-slices 0 + 1, 2 + 3, then the pairs; then relu(h + b1) . w2 over the lane's four hidden units, the four groups, the tiles
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            acc[m][e] += __shfl_xor(acc[m][e], 4, 64);
            acc[m][e] += __shfl_xor(acc[m][e], 8, 64);
        }
        float z = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = 16 * wave + 4 * ng + e;
            if (n < hidden) z = fmaf(relu_nan(acc[m][e] + b1[n]), w2[n], z);
        }
        z += __shfl_xor(z, 16, 64);
        z += __shfl_xor(z, 32, 64);
        if (lane < 4) zp[wave * R + 4 * m + lane] = z;      // ng = 0, ks = 0, row 4 m + lane
    }
    __syncthreads();
    if (threadIdx.x < R && r0 + threadIdx.x < n_rows) {
        float t = 0.f;
        for (int w = 0; w < nwaves; ++w) t += zp[w * R + threadIdx.x];
        t += b2[0];
        out[r0 + threadIdx.x] = sig ? 1.0f / (1.0f + expf(-t)) : t;
    }
}

// Backward of the link predictor z = fc2(relu(fc1(cat(a, b)))) for the training step (train_link_prediction.py:241-257; models/modules.py:57-68):
// given g = dL/dz [n] it produces da, db [n][dim] and ACCUMULATES the four parameter gradients (buffers zeroed by the caller).
// k_merge_bwd_rows, one workgroup = 16 rows (the forward kernel above with a different ending):
//   * hidden pre-activations on the matrix cores, 16 rows per workgroup (wave w: kBwdTiles = three 16-wide hidden tiles from 48 w);
//   * dh = g w2 [pre > 0] leaves as rows [n][hidden] (the operand of the weight-gradient product below) and, transposed, into LDS; dfc2_w from the
//     accumulators (DPP row sums, one atomic per hidden unit and workgroup), dfc2_b likewise;
//   * dcat = dh fc1 on the matrix cores: out^T[k][row] = sum_j fc1[j][k] dh^T[j][row].  One float4 of an fc1 row (4 consecutive k) per lane feeds FOUR
//     MFMAs whose output rows are k = 4 c + t: the 16 lanes of a group cover 64 consecutive k, each lane ends up with 16 consecutive k per lane group;
// dfc1 = dh^T [a | b] (+ dfc1_b = column sums of dh) is a weight-gradient-shaped product: train::dw_grouped (k_dw_grouped), two problems.
// (Two earlier FMA-only versions — one atomic per dfc1 element, then two atomics-free kernels — took 80-90 us per call: chains of load and atomic
// latencies on 25 workgroups.)
constexpr int kBwdWaves = 4, kBwdTiles = 3;                           // waves of a workgroup, 16-wide hidden tiles per wave
constexpr int kBwdWaveHidden = 16 * kBwdTiles;                        // 48 hidden units per wave
constexpr int kBwdMaxHidden = kBwdWaves * kBwdWaveHidden;             // 192: what one workgroup's dh^T holds (modules.py checks the same number)
__global__ __launch_bounds__(64 * kBwdWaves) void k_merge_bwd_rows(const float* __restrict__ a, const float* __restrict__ b, int64_t n_rows, int dim, int hidden,
                                                         const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ gz, float* __restrict__ dh, int ldh, float* __restrict__ da,
                                                         float* __restrict__ db, float* __restrict__ dw2, float* __restrict__ db2) {
    __shared__ float dhs[kBwdMaxHidden][17];             // dh^T [hidden][row] (+1: the transposed reads below hit 16 different banks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 15, g = lane >> 4;
    const int64_t m = (int64_t)blockIdx.x * 16 + c;
    const bool mv = m < n_rows;
    const int K = 2 * dim, nsteps = (K + 15) >> 4;
    constexpr int PF = 4;
    const int n0 = kBwdWaveHidden * wave;
    auto load_b = [&](int st) -> mf4 {
        const int kk = 16 * st + 4 * g;
        if (!(mv && kk < K)) return mf4{0.f, 0.f, 0.f, 0.f};
        return kk < dim ? *reinterpret_cast<const mf4*>(a + m * dim + kk) : *reinterpret_cast<const mf4*>(b + m * dim + (kk - dim));
    };
    auto load_a = [&](int st, int i) -> mf4 {
        const int kk = 16 * st + 4 * g, n = n0 + 16 * i + c;
        return (n < hidden && kk < K) ? *reinterpret_cast<const mf4*>(w1 + (size_t)n * K + kk) : mf4{0.f, 0.f, 0.f, 0.f};
    };
    mf4 acc[kBwdTiles] = {mf4{0.f, 0.f, 0.f, 0.f}, mf4{0.f, 0.f, 0.f, 0.f}, mf4{0.f, 0.f, 0.f, 0.f}};
    {
        mf4 bq[PF], aq[PF][kBwdTiles];
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            bq[u] = load_b(u);
#pragma unroll
            for (int i = 0; i < kBwdTiles; ++i) aq[u][i] = load_a(u, i);
        }
        for (int st0 = 0; st0 < nsteps; st0 += PF) {
#pragma unroll
            for (int u = 0; u < PF; ++u) {
                if (st0 + u < nsteps) {
                    const mf4 bf = bq[u];
                    mf4 af[kBwdTiles];
#pragma unroll
                    for (int i = 0; i < kBwdTiles; ++i) af[i] = aq[u][i];
                    bq[u] = load_b(st0 + u + PF);
#pragma unroll
                    for (int i = 0; i < kBwdTiles; ++i) aq[u][i] = load_a(st0 + u + PF, i);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int i = 0; i < kBwdTiles; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][t], bf[t], acc[i], 0, 0, 0);
                }
            }
        }
    }
    // dh, dfc2_w, dfc2_b from the accumulators (rows = hidden units n0 + 16 i + 4 g + r, columns = the 16 rows of the workgroup)
    const float gm = mv ? gz[m] : 0.f;
#pragma unroll
    for (int i = 0; i < kBwdTiles; ++i) {
        mf4 d, hr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + 16 * i + 4 * g + r;
            const float pre = n < hidden ? acc[i][r] + b1[n] : 0.f;
            d[r] = (n < hidden && pre > 0.f) ? gm * w2[n] : 0.f;
            hr[r] = fmaxf(pre, 0.f) * gm;
            dhs[n][c] = d[r];
        }
        const int nb = n0 + 16 * i + 4 * g;
        if (mv && nb < hidden) *reinterpret_cast<mf4*>(dh + m * ldh + nb) = d;          // hidden % 4 == 0: a float4 never straddles the end
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = hr[r];                    // sum over the 16 rows (lanes of one group)
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
            if (c == 0 && nb + r < hidden) atomicAdd(dw2 + nb + r, v);
        }
    }
    if (wave == 0) {
        float v = g == 0 ? gm : 0.f;
        v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64);
        if (lane == 0) atomicAdd(db2, v);
    }
    __syncthreads();
    // dcat: sets of 64 consecutive input features k, dealt to the waves; per k-step of 4 hidden units one float4 of fc1 per lane and four MFMAs
    const int nset = (K + 63) >> 6, hsteps = (hidden + 3) >> 2;
    for (int set = wave; set < nset; set += kBwdWaves) {
        const int kbase = 64 * set, kl = kbase + 4 * c;            // this lane's four features
        mf4 o[4] = {mf4{0.f, 0.f, 0.f, 0.f}, mf4{0.f, 0.f, 0.f, 0.f}, mf4{0.f, 0.f, 0.f, 0.f}, mf4{0.f, 0.f, 0.f, 0.f}};
        auto load_w = [&](int hs) -> mf4 {
            const int j = 4 * hs + g;
            return (j < hidden && kl < K) ? *reinterpret_cast<const mf4*>(w1 + (size_t)j * K + kl) : mf4{0.f, 0.f, 0.f, 0.f};
        };
        constexpr int WQ = 8;
        mf4 wq[WQ];
#pragma unroll
        for (int u = 0; u < WQ; ++u) wq[u] = load_w(u);
        for (int hs0 = 0; hs0 < hsteps; hs0 += WQ) {
#pragma unroll
            for (int u = 0; u < WQ; ++u) {
                if (hs0 + u < hsteps) {
                    const mf4 wv = wq[u];
                    wq[u] = load_w(hs0 + u + WQ);
                    const int j = 4 * (hs0 + u) + g;
                    const float bv = j < hidden ? dhs[j][c] : 0.f;      // B[k = hidden unit j][n = row c]
#pragma unroll
                    for (int t = 0; t < 4; ++t) o[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[t], bv, o[t], 0, 0, 0);
                }
            }
        }
        // o[t][r] = dcat[row c][k = kbase + 4 (4 g + r) + t]: 16 consecutive features per lane
        if (mv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = kbase + 16 * g + 4 * r;
                if (k < K) {
                    const mf4 v = mf4{o[0][r], o[1][r], o[2][r], o[3][r]};
                    if (k < dim) *reinterpret_cast<mf4*>(da + m * dim + k) = v; else *reinterpret_cast<mf4*>(db + m * dim + (k - dim)) = v;
                }
            }
        }
    }
}

}  // namespace dygnn

using namespace dygnn;

// Which forward kernel a call takes (the values are what dygnn_merge_layer_forward_path returns).  The row-block forms stage R rows of cat(a, b)
// in LDS: the widest one that fits is taken, a size that fits none falls through to M (no LDS) and G (one row), so every (dim, hidden) whose
// single row G can stage (2 dim + 4 floats within 64 KB) is answered at every n.  (M also takes longer rows, from 2048 rows on.)
enum MergePath : int32_t {
    kPathG = 0,       // k_merge_sigmoid: one workgroup per row
    kPathR1 = 1,      // k_merge_sigmoid_rows4<1>: 4 rows per workgroup
    kPathR4 = 2,      // k_merge_sigmoid_rows4<4>: 16 rows per workgroup
    kPathM = 3,       // k_merge_sigmoid_mfma: one wave per 16 rows
};
static int64_t merge_ldx(int64_t dim) { const int64_t k16 = (2 * dim + 15) & ~(int64_t)15; return (k16 & 16) ? k16 : k16 + 16; }      // row stride % 32 == 16: the four rows on distinct banks
static size_t merge_rows_lds(int R, int64_t dim, int64_t hidden) { return ((size_t)R * (size_t)merge_ldx(dim) + (size_t)R * (size_t)((hidden + 15) / 16)) * sizeof(float); }
constexpr size_t kMergeLdsMax = 64 * 1024;

extern "C" int32_t dygnn_merge_layer_forward_path(int64_t n, int32_t dim, int32_t hidden) {
    DYGNN_REQUIRE(n >= 0 && dim > 0 && hidden > 0, "merge_layer: bad sizes");
    DYGNN_REQUIRE(dim <= (INT32_MAX - 16) / 2, "merge_layer: dim too large");      // the kernels index a row's 2 dim features, rounded up to 16, in int
    const bool vec = dim % 4 == 0;
    if (vec && hidden <= 256 && n >= 64) {      // an evaluation step's worth of rows (4 per workgroup) or thousands of them (16 per workgroup)
        if (n >= 2048 && merge_rows_lds(16, dim, hidden) <= kMergeLdsMax) return kPathR4;
        if (merge_rows_lds(4, dim, hidden) <= kMergeLdsMax) return kPathR1;
    }
    if (vec && n >= 2048) return kPathM;             // hidden > 256, or rows too long to stage: the wave-per-16-rows form
    DYGNN_REQUIRE((size_t)(2 * (int64_t)dim + 4) * sizeof(float) <= kMergeLdsMax, "merge_layer: dim too large");
    return kPathG;
}

static int merge_forward(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                         const float* fc2_b, float* out, int sig, dygnn_stream_t stream) {
    DYGNN_REQUIRE(n >= 0 && dim > 0 && hidden > 0, "merge_layer: bad sizes");
    DYGNN_REQUIRE(n == 0 || (a && b && fc1_w && fc1_b && fc2_w && fc2_b && out), "merge_layer: null pointer");
    if (n == 0) return DYGNN_OK;
    const int path = dygnn_merge_layer_forward_path(n, dim, hidden);
    if (path < 0) return path;
    const int tiles = (hidden + 15) / 16, ldx = (int)merge_ldx(dim);
    switch (path) {
    case kPathR4:
        hipLaunchKernelGGL(k_merge_sigmoid_rows4<4>, dim3((unsigned)ceil_div(n, 16)), dim3(64 * tiles),
                           merge_rows_lds(16, dim, hidden), as_stream(stream), a, b, n, dim, hidden, fc1_w, fc1_b, fc2_w, fc2_b, out, sig, ldx);
        break;
    case kPathR1:
        hipLaunchKernelGGL(k_merge_sigmoid_rows4<1>, dim3((unsigned)ceil_div(n, 4)), dim3(64 * tiles),
                           merge_rows_lds(4, dim, hidden), as_stream(stream), a, b, n, dim, hidden, fc1_w, fc1_b, fc2_w, fc2_b, out, sig, ldx);
        break;
    case kPathM:
        hipLaunchKernelGGL(k_merge_sigmoid_mfma, dim3((unsigned)ceil_div(n, 64)), dim3(256), 0, as_stream(stream), a, b, n, dim, hidden,
                           fc1_w, fc1_b, fc2_w, fc2_b, out, sig);
        break;
    case kPathG:
        hipLaunchKernelGGL(k_merge_sigmoid, dim3((unsigned)n), dim3(256), (size_t)(2 * dim + 4) * sizeof(float), as_stream(stream), a, b, dim, hidden, fc1_w,
                           fc1_b, fc2_w, fc2_b, out, sig);
    }
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

extern "C" int dygnn_merge_layer_sigmoid(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden,
                                         const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                                         float* out, dygnn_stream_t stream) {
    return merge_forward(a, b, n, dim, hidden, fc1_w, fc1_b, fc2_w, fc2_b, out, 1, stream);
}

extern "C" int dygnn_merge_layer_logits(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden,
                                        const float* fc1_w, const float* fc1_b, const float* fc2_w, const float* fc2_b,
                                        float* out, dygnn_stream_t stream) {
    return merge_forward(a, b, n, dim, hidden, fc1_w, fc1_b, fc2_w, fc2_b, out, 0, stream);
}

extern "C" int dygnn_merge_layer_backward(const float* a, const float* b, int64_t n, int32_t dim, int32_t hidden, const float* fc1_w, const float* fc1_b,
                                          const float* fc2_w, const float* grad_logits, float* grad_a, float* grad_b, float* grad_fc1_w, float* grad_fc1_b,
                                          float* grad_fc2_w, float* grad_fc2_b, float* workspace, dygnn_stream_t stream) {
    DYGNN_REQUIRE(n >= 0 && dim > 0 && hidden > 0 && dim % 4 == 0 && hidden % 4 == 0 && hidden <= kBwdMaxHidden, "merge_layer_backward: dim and hidden must be multiples of 4, hidden <= %d", kBwdMaxHidden);
    DYGNN_REQUIRE(a && b && fc1_w && fc1_b && fc2_w && grad_logits && grad_a && grad_b && grad_fc1_w && grad_fc1_b && grad_fc2_w && grad_fc2_b && workspace,
                  "merge_layer_backward: null pointer");
    DYGNN_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0,
                  "merge_layer_backward: a, b and the workspace must be 16-byte aligned");
    if (n == 0) return DYGNN_OK;
    hipLaunchKernelGGL(k_merge_bwd_rows, dim3((unsigned)ceil_div(n, (int64_t)16)), dim3(64 * kBwdWaves), 0, as_stream(stream), a, b, n, dim, hidden, fc1_w, fc1_b, fc2_w, grad_logits,
                       workspace, hidden, grad_a, grad_b, grad_fc2_w, grad_fc2_b);
    DYGNN_LAUNCH_CHECK();
    const train::DwPair pairs[2] = {{workspace, hidden, hidden, a, dim, dim, grad_fc1_w, 2 * dim, grad_fc1_b},
                                    {workspace, hidden, hidden, b, dim, dim, grad_fc1_w + dim, 2 * dim, nullptr}};
    return train::dw_grouped(as_stream(stream), (int)n, pairs, 2);
}
