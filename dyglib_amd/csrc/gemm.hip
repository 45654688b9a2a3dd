// The library's general fp32-MFMA GEMM (gemm.h): train::mm and its three kernels, the dispatch mm_plan, the grouped weight-gradient product
// dw_grouped, the atomic column sum, and the C entry points dygnn_mm* / dygnn_dw_grouped.  Every backbone's dense products come here.
#include <cstdlib>
#include <vector>
#include "gemm.h"

namespace dygnn {

namespace train {

using f4 = __attribute__((ext_vector_type(4))) float;

// ------------------------------------------------------------------------------------------------
// C = alpha * op(A) . op(B) (+ bias[n]) (+ beta * C), batched: z = zb * H + zh selects A + zb*sAb + zh*sAh etc.
//   op(A)[m][k] = transA ? A[k*lda + m] : A[m*lda + k] ;  op(B)[k][n] = transB ? B[n*ldb + k] : B[k*ldb + n]
// 64x64 tile per workgroup (4 waves x 16 rows x 64 columns), K in steps of 16 through LDS, v_mfma_f32_16x16x4_f32.
// ------------------------------------------------------------------------------------------------
struct MM {
    const float* A; const float* B; float* C; const float* bias;
    int M, N, K, lda, ldb, ldc, transA, transB;
    float alpha, beta;
    int H; int64_t sAb, sAh, sBb, sBh, sCb, sCh;
    int relu;               // epilogue max(v, 0) (not combined with split-K)
    int ksplit, kchunk;     // split-K: blockIdx.z = batch * ksplit + part; part sums k in [part*kchunk, +kchunk) and adds atomically
    float* colsum;          // transA products only: colsum[m] += sum_k op(A)[m][k] (the bias gradient next to a weight gradient), or null
    const int32_t* m_dev;   // optional device-side row count (<= M): workgroups whose rows all lie beyond it exit at once
    int vecC;               // C rows may be written as aligned float4 (pointer, ldc and batch strides multiples of 4 floats)
    const int32_t* a_rows;  // optional (k-contiguous A, LDS-DMA kernel only): row m of op(A) is A[a_rows[m]] — the product gathers its rows itself
};

__global__ __launch_bounds__(256) void k_mm(const MM p) {
    __shared__ float As[16][64 + 16];      // row stride 80 = 16 mod 64 banks: the four k-rows a wave reads at once do not collide
    __shared__ float Bs[16][64 + 16];
    const int z = blockIdx.z / p.ksplit, ks = blockIdx.z % p.ksplit, zb = z / p.H, zh = z % p.H;
    const float* A = p.A + zb * p.sAb + zh * p.sAh;
    const float* Bm = p.B + zb * p.sBb + zh * p.sBh;
    float* C = p.C + zb * p.sCb + zh * p.sCh;
    const int m0 = blockIdx.x * 64, n0 = blockIdx.y * 64;
    if (p.m_dev && m0 >= *p.m_dev) return;
    const int kbeg = ks * p.kchunk, kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    f4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = f4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int idx = tid + 256 * e;
            int m, k;
            if (p.transA) { m = idx & 63; k = idx >> 6; } else { m = idx >> 4; k = idx & 15; }
            float v = 0.f;
            if (m0 + m < p.M && k0 + k < kend) v = p.transA ? A[(size_t)(k0 + k) * p.lda + m0 + m] : A[(size_t)(m0 + m) * p.lda + k0 + k];
            As[k][m] = v;
            int n, kb;
            if (p.transB) { n = idx >> 4; kb = idx & 15; } else { n = idx & 63; kb = idx >> 6; }
            float w = 0.f;
            if (n0 + n < p.N && k0 + kb < kend) w = p.transB ? Bm[(size_t)(n0 + n) * p.ldb + k0 + kb] : Bm[(size_t)(k0 + kb) * p.ldb + n0 + n];
            Bs[kb][n] = w;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const float a = As[4 * kk + g][16 * wave + c];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[4 * kk + g][16 * nt + c], acc[nt], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + 16 * nt + c;
        if (n >= p.N) continue;
        const float bv = (p.bias && ks == 0) ? p.bias[n] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * wave + 4 * g + r;
            if (m >= p.M) continue;
            float v = p.alpha * acc[nt][r] + bv;
            if (p.ksplit > 1) { atomicAdd(&C[(size_t)m * p.ldc + n], v); continue; }
            if (p.beta != 0.f) v += p.beta * C[(size_t)m * p.ldc + n];
            if (p.relu) v = fmaxf(v, 0.f);
            C[(size_t)m * p.ldc + n] = v;
        }
    }
}

// The large products: (32*WM) x (32*WN) tile per workgroup (instantiated as 64 x 64 only), 4 waves as 2 x 2, each wave WM x WN accumulator tiles; operands go
// through LDS in k-major layout ([16 k][tile + 4]) with float4 global loads when pointers / leading dimensions allow
// (vecA / vecB), so one k-step of 16 costs a wave 8 or 6 LDS reads per 16 or 8 MFMAs instead of k_mm's 5 per 4.
template <int WN, int WM>
__global__ __launch_bounds__(256) void k_mm_big(const MM p, const int vecA, const int vecB) {
    constexpr int BM = 32 * WM, BN = 32 * WN, NB = BN / 64, NA = BM / 64;      // tile BM x BN; wave = WM x WN accumulator tiles
    __shared__ float As[2][16][BM + 16];      // double buffered: the global loads of k-step t+1 fly while step t multiplies
    __shared__ float Bs[2][16][BN + 16];
    const int z = blockIdx.z / p.ksplit, ks = blockIdx.z % p.ksplit, zb = z / p.H, zh = z % p.H;
    const float* A = p.A + zb * p.sAb + zh * p.sAh;
    const float* Bm = p.B + zb * p.sBb + zh * p.sBh;
    float* C = p.C + zb * p.sCb + zh * p.sCh;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (p.m_dev && m0 >= *p.m_dev) return;        // uniform over the workgroup, before any barrier
    const int kbeg = ks * p.kchunk, kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = wave >> 1, wx = wave & 1;
    const int c = lane & 15, g = lane >> 4;
    f4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    auto ldA = [&](int m, int k) -> float {      // op(A)[m][k], zero outside
        if (m >= p.M || k >= kend) return 0.f;
        return p.transA ? A[(size_t)k * p.lda + m] : A[(size_t)m * p.lda + k];
    };
    auto ldB = [&](int k, int n) -> float {
        if (n >= p.N || k >= kend) return 0.f;
        return p.transB ? Bm[(size_t)n * p.ldb + k] : Bm[(size_t)k * p.ldb + n];
    };
    f4 ra[NA], rb[NB];
    auto fetch = [&](int k0) {                    // this thread's share of the tiles of k-step k0 -> registers
        if (p.transA) {                           // stored [K][M]: m contiguous; thread -> (k, 4 consecutive m)
#pragma unroll
            for (int e = 0; e < NA; ++e) {
                const int k = (tid / (BM / 4)) + (1024 / BM) * e, m = (tid % (BM / 4)) * 4;
                if (vecA && m0 + m + 3 < p.M && k0 + k < kend) ra[e] = *reinterpret_cast<const f4*>(A + (size_t)(k0 + k) * p.lda + m0 + m);
                else ra[e] = f4{ldA(m0 + m, k0 + k), ldA(m0 + m + 1, k0 + k), ldA(m0 + m + 2, k0 + k), ldA(m0 + m + 3, k0 + k)};
            }
        } else {                                  // stored [M][K]: k contiguous; thread -> (m, 4 consecutive k)
#pragma unroll
            for (int e = 0; e < NA; ++e) {
                const int m = (tid >> 2) + 64 * e, k = (tid & 3) * 4;
                if (vecA && m0 + m < p.M && k0 + k + 3 < kend) ra[e] = *reinterpret_cast<const f4*>(A + (size_t)(m0 + m) * p.lda + k0 + k);
                else ra[e] = f4{ldA(m0 + m, k0 + k), ldA(m0 + m, k0 + k + 1), ldA(m0 + m, k0 + k + 2), ldA(m0 + m, k0 + k + 3)};
            }
        }
        if (!p.transB) {                          // stored [K][N]: n contiguous
#pragma unroll
            for (int e = 0; e < NB; ++e) {
                const int k = (tid / (BN / 4)) + (1024 / BN) * e, n = (tid % (BN / 4)) * 4;
                if (vecB && n0 + n + 3 < p.N && k0 + k < kend) rb[e] = *reinterpret_cast<const f4*>(Bm + (size_t)(k0 + k) * p.ldb + n0 + n);
                else rb[e] = f4{ldB(k0 + k, n0 + n), ldB(k0 + k, n0 + n + 1), ldB(k0 + k, n0 + n + 2), ldB(k0 + k, n0 + n + 3)};
            }
        } else {                                  // stored [N][K]: k contiguous
#pragma unroll
            for (int e = 0; e < NB; ++e) {
                const int n = (tid >> 2) + 64 * e, k = (tid & 3) * 4;
                if (vecB && n0 + n < p.N && k0 + k + 3 < kend) rb[e] = *reinterpret_cast<const f4*>(Bm + (size_t)(n0 + n) * p.ldb + k0 + k);
                else rb[e] = f4{ldB(k0 + k, n0 + n), ldB(k0 + k + 1, n0 + n), ldB(k0 + k + 2, n0 + n), ldB(k0 + k + 3, n0 + n)};
            }
        }
    };
    auto stash = [&](int buf) {                   // registers -> LDS tile `buf` (k-major)
        // LDS column of element (k, m) = (m + 16 * (k / 4)) mod BM: the four k-groups a wave writes at once (rows k, k+4, k+8,
        // k+12 of the same m) would otherwise share their banks (row stride = 16 mod 64 -> 4 rows = 0 mod 64): 4-way conflicts
        if (p.transA) {
#pragma unroll
            for (int e = 0; e < NA; ++e) {
                const int k = (tid / (BM / 4)) + (1024 / BM) * e, m = (tid % (BM / 4)) * 4;
                *reinterpret_cast<f4*>(&As[buf][k][(m + 16 * (k >> 2)) & (BM - 1)]) = ra[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < NA; ++e) {
                const int m = (tid >> 2) + 64 * e, k = (tid & 3) * 4, mr = (m + 16 * (k >> 2)) & (BM - 1);
                As[buf][k][mr] = ra[e].x; As[buf][k + 1][mr] = ra[e].y; As[buf][k + 2][mr] = ra[e].z; As[buf][k + 3][mr] = ra[e].w;
            }
        }
        if (!p.transB) {
#pragma unroll
            for (int e = 0; e < NB; ++e) {
                const int k = (tid / (BN / 4)) + (1024 / BN) * e, n = (tid % (BN / 4)) * 4;
                *reinterpret_cast<f4*>(&Bs[buf][k][(n + 16 * (k >> 2)) & (BN - 1)]) = rb[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < NB; ++e) {
                const int n = (tid >> 2) + 64 * e, k = (tid & 3) * 4, nr = (n + 16 * (k >> 2)) & (BN - 1);
                Bs[buf][k][nr] = rb[e].x; Bs[buf][k + 1][nr] = rb[e].y; Bs[buf][k + 2][nr] = rb[e].z; Bs[buf][k + 3][nr] = rb[e].w;
            }
        }
    };
    fetch(kbeg);
    stash(0);
    __syncthreads();
    int buf = 0;
    static_assert(BM == 64, "the column-sum side product assumes 64-row tiles (wave w sums k rows 4w .. 4w+3 of column `lane`)");
    const bool want_colsum = p.colsum != nullptr && blockIdx.y == 0;
    float csum = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += 16) {
        const bool more = k0 + 16 < kend;
        if (more) fetch(k0 + 16);
        if (want_colsum) {                        // rows beyond kend / M were stored as zeros
            const int col = (lane + 16 * wave) & (BM - 1);
            csum += (As[buf][4 * wave][col] + As[buf][4 * wave + 1][col]) + (As[buf][4 * wave + 2][col] + As[buf][4 * wave + 3][col]);
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float a[WM], b[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) a[i] = As[buf][4 * kk + g][(16 * WM * wy + 16 * i + c + 16 * kk) & (BM - 1)];
#pragma unroll
            for (int j = 0; j < WN; ++j) b[j] = Bs[buf][4 * kk + g][(16 * WN * wx + 16 * j + c + 16 * kk) & (BN - 1)];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) stash(buf ^ 1);                 // the other buffer was last read one iteration ago, before the barrier below
        __syncthreads();
        buf ^= 1;
    }
    if (want_colsum && m0 + lane < p.M) atomicAdd(&p.colsum[m0 + lane], csum);
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int n = n0 + 16 * WN * wx + 16 * j + c;
        if (n >= p.N) continue;
        const float bv = (p.bias && ks == 0) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * WM * wy + 16 * i + 4 * g + r;
                if (m >= p.M) continue;
                float v = p.alpha * acc[i][j][r] + bv;
                if (p.ksplit > 1) { atomicAdd(&C[(size_t)m * p.ldc + n], v); continue; }
                if (p.beta != 0.f) v += p.beta * C[(size_t)m * p.ldc + n];
                if (p.relu) v = fmaxf(v, 0.f);
                C[(size_t)m * p.ldc + n] = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// The same 64 x 64 tile product with both operands fed by LDS-DMA (global_load_lds: no VGPR round trip) into a ring of NS
// stages of one 16-wide k-step each: NS - 1 steps of loads are in flight per workgroup instead of one, which is what the
// latency-bound k-loop of k_mm_big lacks (its second register stage cost occupancy instead).  One barrier per k-step.
// Tile of an operand in a stage: four 1-KiB blocks of 16 rows x 16 k, block w written by wave w with one DMA instruction
// (lane L lands at byte 16 L of the block).  Lane -> element mapping per orientation, chosen so that the MFMA operand
// reads are conflict-free in the PERMUTED k order (MFMA step r takes k = 4 g + r from both operands):
//   k-contiguous operand ([row][k] in memory): lane L loads the float4 (row = L & 15, k = 4 (L >> 4) ..+3)
//       -> lane (c, g) reads the granule at float 4 (16 g + c) with one ds_read_b128
//   row-contiguous operand ([k][row] in memory): lane L loads (k = 4 ((L >> 2) & 3) + (L >> 4), rows 4 (L & 3) ..+3)
//       -> element (row c, k = 4 g + r) sits at float 4 (16 r + 4 g + (c >> 2)) + (c & 3)     (banks 16 g + c per half-wave)
// Rows / k beyond the matrix load from a 16-byte page of zeros (DMA cannot zero-fill), so tails need no special path as long
// as a float4 never straddles a bound (K % 4 == 0, and M % 4 == 0 / N % 4 == 0 for a row-contiguous A / B: checked by mm()).
// ------------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(16))) float g_zero_page[4] = {0.f, 0.f, 0.f, 0.f};

template <int KA, int KB, int WM, int WN, int NS>      // KA / KB = 1: the operand is k-contiguous in memory (A: !transA, B: transB); tile 32 WM x 32 WN
__global__ __launch_bounds__(256) void k_mm_dma(const MM p) {
    constexpr int BM = 32 * WM, BN = 32 * WN, STAGE = 16 * (BM + BN);      // floats per stage: A tile then B tile
    constexpr int LOADS = (WM + WN) / 2;                                    // DMA instructions per wave and stage
    __shared__ __attribute__((aligned(16))) float ring[NS * STAGE];
    const int z = blockIdx.z / p.ksplit, ks = blockIdx.z % p.ksplit, zb = z / p.H, zh = z % p.H;
    const float* A = p.A + zb * p.sAb + zh * p.sAh;
    const float* Bm = p.B + zb * p.sBb + zh * p.sBh;
    float* C = p.C + zb * p.sCb + zh * p.sCh;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    if (p.m_dev && m0 >= *p.m_dev) return;
    const int kbeg = ks * p.kchunk, kend = kbeg + p.kchunk < p.K ? kbeg + p.kchunk : p.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wy = wave >> 1, wx = wave & 1, c = lane & 15, g = lane >> 4;
    f4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    // this lane's source coordinates inside a 16-row block (wave w loads blocks w, w + 4, ...)
    const int rA = KA ? (lane & 15) : 4 * (lane & 3), kA = KA ? 4 * (lane >> 4) : 4 * ((lane >> 2) & 3) + (lane >> 4);
    const int rB = KB ? (lane & 15) : 4 * (lane & 3), kB = KB ? 4 * (lane >> 4) : 4 * ((lane >> 2) & 3) + (lane >> 4);
    const int nsteps = (kend - kbeg + 15) >> 4;
    // rows of op(A) this lane loads (k-contiguous A): with a row table the product gathers them (rows beyond the live count read zeros: the
    // table's entries there are not written)
    int64_t arow[WM / 2];
#pragma unroll
    for (int u = 0; u < WM / 2; ++u) {
        const int r = m0 + 16 * (wave + 4 * u) + rA;
        const int mlim = (p.a_rows && p.m_dev) ? (*p.m_dev < p.M ? *p.m_dev : p.M) : p.M;
        arow[u] = r < mlim ? ((KA && p.a_rows) ? (int64_t)p.a_rows[r] : (int64_t)r) : -1;
    }
    auto issue = [&](int t) {                 // k-step t -> ring slot t % NS (beyond the last step: zeros, which keeps vmcnt uniform)
        const int k0 = kbeg + 16 * t;
        float* slot = ring + (t % NS) * STAGE;
#pragma unroll
        for (int u = 0; u < WM / 2; ++u) {
            const int blk = wave + 4 * u, r = m0 + 16 * blk + rA;
            const float* src = (t < nsteps && arow[u] >= 0 && k0 + kA < kend) ? (KA ? A + (size_t)arow[u] * p.lda + k0 + kA : A + (size_t)(k0 + kA) * p.lda + r) : g_zero_page;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)(slot + 256 * blk), 16, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < WN / 2; ++u) {
            const int blk = wave + 4 * u, r = n0 + 16 * blk + rB;
            const float* src = (t < nsteps && r < p.N && k0 + kB < kend) ? (KB ? Bm + (size_t)r * p.ldb + k0 + kB : Bm + (size_t)(k0 + kB) * p.ldb + r) : g_zero_page;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)(slot + 16 * BM + 256 * blk), 16, 0, 0);
        }
    };
    const bool want_colsum = p.colsum != nullptr && blockIdx.y == 0;      // only with a row-contiguous A (weight gradients), 64-row tiles
    float csum = 0.f;
#pragma unroll
    for (int t = 0; t < NS - 1; ++t) issue(t);
    for (int t = 0; t < nsteps; ++t) {
        // this wave's loads of step t have landed; then a BARE barrier (everybody's have, and everybody is done with step t - 1):
        // __syncthreads() would add a fence = s_waitcnt vmcnt(0), i.e. wait for the whole ring and undo the pipelining
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(LOADS * (NS - 2)) : "memory");
        issue(t + NS - 1);                                                      // into the slot step t - 1 used
        const float* as = ring + (t % NS) * STAGE;
        const float* bs = as + 16 * BM;
        if (!KA && WM == 2 && want_colsum) {  // element (row = lane, k) of the A tile: block lane >> 4, row c; this wave sums k = 4 wave .. +3
            const float* q = as + 256 * g + 4 * (16 * wave + (c >> 2)) + (c & 3);
            csum += (q[0] + q[16]) + (q[32] + q[48]);
        }
        // Permuted k order: MFMA step r multiplies k = 4 g + r of both operands.  A k-contiguous operand then needs ONE conflict-free
        // ds_read_b128 per tile (lane (c, g) takes the whole granule of row c; ds_read_b32 of that layout would be 2-way conflicted,
        // its banks being (a/4) mod 32 per half-wave); a row-contiguous operand reads element (row c, k = 4 g + r) at float
        // 4 (16 r + 4 g + (c >> 2)) + (c & 3): banks 16 g + c inside a half-wave, conflict-free.
        float a[WM][4], b[WN][4];
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            if constexpr (KA) {
                const f4 v = *reinterpret_cast<const f4*>(as + 256 * (WM * wy + i) + 4 * (16 * g + c));
                a[i][0] = v.x; a[i][1] = v.y; a[i][2] = v.z; a[i][3] = v.w;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) a[i][r] = as[256 * (WM * wy + i) + 4 * (16 * r + 4 * g + (c >> 2)) + (c & 3)];
            }
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            if constexpr (KB) {
                const f4 v = *reinterpret_cast<const f4*>(bs + 256 * (WN * wx + j) + 4 * (16 * g + c));
                b[j][0] = v.x; b[j][1] = v.y; b[j][2] = v.z; b[j][3] = v.w;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) b[j][r] = bs[256 * (WN * wx + j) + 4 * (16 * r + 4 * g + (c >> 2)) + (c & 3)];
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][r], b[j][r], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the trailing zero-page loads must not outlive the workgroup's LDS
    if (WM == 2 && want_colsum && m0 + lane < p.M) atomicAdd(&p.colsum[m0 + lane], csum);
    if (WM == 2 && WN == 2 && p.vecC && p.ksplit == 1 && p.beta == 0.f) {
        // coalesced epilogue: the tile goes through LDS (the ring is free now) and leaves as float4 rows -- 16 lanes write one 256-byte
        // row segment, 4 store instructions per wave instead of 16 scalar ones that each touch four rows
        asm volatile("s_barrier" ::: "memory");                   // every wave is done reading the ring
        constexpr int LD = 64 + 4;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nl = 32 * wx + 16 * j + c;
            const float bv = (p.bias && n0 + nl < p.N) ? p.bias[n0 + nl] : 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = p.alpha * acc[i][j][r] + bv;
                    if (p.relu) v = fmaxf(v, 0.f);
                    ring[(32 * wy + 16 * i + 4 * g + r) * LD + nl] = v;
                }
        }
        __syncthreads();
        const int col = 4 * (tid & 15);
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int row = 16 * ps + (tid >> 4), m = m0 + row, n = n0 + col;
            if (m >= p.M || n >= p.N) continue;
            const f4 v = *reinterpret_cast<const f4*>(ring + row * LD + col);
            float* dst = C + (size_t)m * p.ldc + n;
            if (n + 3 < p.N) *reinterpret_cast<f4*>(dst) = v;
            else {
                dst[0] = v.x;
                if (n + 1 < p.N) dst[1] = v.y;
                if (n + 2 < p.N) dst[2] = v.z;
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int n = n0 + 16 * WN * wx + 16 * j + c;
        if (n >= p.N) continue;
        const float bv = (p.bias && ks == 0) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + 16 * WM * wy + 16 * i + 4 * g + r;
                if (m >= p.M) continue;
                float v = p.alpha * acc[i][j][r] + bv;
                if (p.ksplit > 1) { atomicAdd(&C[(size_t)m * p.ldc + n], v); continue; }
                if (p.beta != 0.f) v += p.beta * C[(size_t)m * p.ldc + n];
                if (p.relu) v = fmaxf(v, 0.f);
                C[(size_t)m * p.ldc + n] = v;
            }
    }
}

template <int WM, int WN, int NS>
static void launch_mm_dma(hipStream_t s, const MM& p, bool tA, bool tB, int batch) {
    const dim3 grid((unsigned)ceil_div(p.M, 32 * WM), (unsigned)ceil_div(p.N, 32 * WN), (unsigned)batch);
    if (!tA && tB) hipLaunchKernelGGL((k_mm_dma<1, 1, WM, WN, NS>), grid, dim3(256), 0, s, p);
    else if (!tA && !tB) hipLaunchKernelGGL((k_mm_dma<1, 0, WM, WN, NS>), grid, dim3(256), 0, s, p);
    else if (tA && !tB) hipLaunchKernelGGL((k_mm_dma<0, 0, WM, WN, NS>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_mm_dma<0, 1, WM, WN, NS>), grid, dim3(256), 0, s, p);
}

// The whole dispatch of mm(), host only: which kernel, how many K parts, which epilogue, where the column sums are made -- or the refusal.
// mm() launches what this returns and dygnn_mm_path reports it, so the two cannot disagree.
int mm_plan(const float* A, int lda, bool tA, const float* B, int ldb, bool tB, const float* C, int ldc, int M, int N, int K, const MmOpt& o, MmPlan* out) {
    const bool has_colsum = o.colsum_out_ != nullptr, has_rows = o.a_rows_ != nullptr;
    MmPlan pl{};
    pl.ksplit = 1;
    pl.kchunk = K;
    if (M <= 0 || N <= 0 || o.batch_ <= 0) { *out = pl; return DYGNN_OK; }
    if (has_colsum && !tA) { set_error("mm: column sums need a transposed A (op(A)[m][k] = A[k * lda + m])"); return DYGNN_E_UNSUPPORTED; }
    if (has_colsum && o.batch_ != 1) { set_error("mm: column sums need batch == 1"); return DYGNN_E_UNSUPPORTED; }
    if (has_rows && tA) { set_error("mm: a row table needs a k-contiguous A (!tA)"); return DYGNN_E_UNSUPPORTED; }
    // weight gradients: small output, K = all rows of the call -> split K over workgroups, partial sums meet by atomicAdd
    if (o.batch_ == 1 && K >= 2048 && !o.relu_) {
        if (o.beta_ != 0.f && o.beta_ != 1.f) { set_error("mm: a product split over K (K >= 2048) takes beta 0 or 1"); return DYGNN_E_UNSUPPORTED; }
        pl.kchunk = 256;
        pl.ksplit = (K + pl.kchunk - 1) / pl.kchunk;
    }
    pl.vecC = ((reinterpret_cast<uintptr_t>(C) & 15) == 0 && ldc % 4 == 0 && o.sCb_ % 4 == 0 && o.sCh_ % 4 == 0) ? 1 : 0;
    pl.vecA = ((reinterpret_cast<uintptr_t>(A) & 15) == 0 && lda % 4 == 0 && o.sAb_ % 4 == 0 && o.sAh_ % 4 == 0) ? 1 : 0;
    pl.vecB = ((reinterpret_cast<uintptr_t>(B) & 15) == 0 && ldb % 4 == 0 && o.sBb_ % 4 == 0 && o.sBh_ % 4 == 0) ? 1 : 0;
    if (M >= 48 && N >= 48) {
        // Tile choice, measured on the TGAT / TGN / training shapes (M = 50 .. 270,000, N = 136 .. 800, K = 136 .. 25,600 split):
        //  * 64-row tiles always: the k-loop is latency-bound (one global -> LDS hop per 16-wide k-step), so what pays is more resident
        //    workgroups per CU, not more MFMAs per LDS read; 128-row tiles were slower at every size (TGAT -7 %, training -5 %);
        //  * 64-column tiles always: ceil(N / 128) * 128 >= ceil(N / 64) * 64, so 128-column tiles never pad less.
        // both operands by LDS-DMA when no float4 can straddle a bound (see k_mm_dma)
        const char* dma_env = getenv("DYGNN_MM_DMA");
        // (Measured and not kept, round 2: the 32 x 208-per-wave register tile of k_dw_grouped applied to the tall activation x weight products
        //  of TGAT — M ~ 10^5, N and K of 136 .. 444: 26 MFMAs per 15 LDS operand reads — ran them in the SAME time as these 64 x 64 tiles
        //  (16.5 vs 16.1 ms over a profile): with K this short a workgroup lives for 9 .. 28 k-steps and its ring fill and tile write-out,
        //  not the k-loop's MFMA density, set the pace.)
        // a_kpad: A is k-contiguous with rows padded to a multiple of 4 floats (zeros behind K): its last float4 stays inside the row
        const bool kok = K % 4 == 0 || (o.a_kpad_ && !tA && !tB && lda >= ((K + 3) & ~3));
        if (pl.vecA && pl.vecB && kok && (!tA || M % 4 == 0) && (tB || N % 4 == 0) && !(dma_env && dma_env[0] == '0')) {
            pl.kernel = kMmDma;
            pl.f4_epilogue = (pl.vecC && pl.ksplit == 1 && o.beta_ == 0.f) ? 1 : 0;       // the condition k_mm_dma tests on the device
        } else {
            if (has_rows) { set_error("mm: a row table needs the LDS-DMA kernel (aligned k-contiguous operands, K %% 4 == 0)"); return DYGNN_E_UNSUPPORTED; }
            pl.kernel = kMmBig;
        }
        pl.colsum_route = has_colsum ? 1 : 0;      // rides along inside the 64-row-tile kernels
    } else {
        if (has_rows) { set_error("mm: a row table needs at least 48 rows and columns"); return DYGNN_E_UNSUPPORTED; }
        pl.kernel = kMmSmall;
        pl.colsum_route = has_colsum ? 2 : 0;      // the stand-alone reduction
    }
    *out = pl;
    return DYGNN_OK;
}

bool mm_gathers_rows(const float* A, int lda, const float* B, int ldb, int M, int N, int K) {
    MmPlan pl;
    return mm_plan(A, lda, false, B, ldb, true, nullptr, 0, M, N, K, MmOpt(), &pl) == DYGNN_OK && pl.kernel == kMmDma;
}

int mm(hipStream_t s, const float* A, int lda, bool tA, const float* B, int ldb, bool tB, float* C, int ldc, int M, int N, int K, const MmOpt& o) {
    if (M <= 0 || N <= 0 || o.batch_ <= 0) return DYGNN_OK;
    MmPlan pl;
    if (int rc = mm_plan(A, lda, tA, B, ldb, tB, C, ldc, M, N, K, o, &pl)) return rc;
    MM p{A, B, C, o.bias_, M, N, K, lda, ldb, ldc, tA ? 1 : 0, tB ? 1 : 0, o.alpha_, o.beta_, o.H_, o.sAb_, o.sAh_, o.sBb_, o.sBh_, o.sCb_, o.sCh_, o.relu_ ? 1 : 0, pl.ksplit,
         pl.kchunk, nullptr, o.m_dev_, pl.vecC, o.a_rows_};
    if (pl.colsum_route == 1) p.colsum = o.colsum_out_;
    else if (pl.colsum_route == 2) { if (int rc = colsum_atomic(s, A, lda, K, M, o.colsum_out_)) return rc; }
    // split: the parts add onto a zeroed C (beta = 0) or onto the old one (beta = 1); the kernels do not read p.beta when ksplit > 1
    if (pl.ksplit > 1 && o.beta_ == 0.f && !o.c_is_zero_) DYGNN_HIP(hipMemset2DAsync(C, (size_t)ldc * sizeof(float), 0, (size_t)N * sizeof(float), (size_t)M, s));
    const int batch = o.batch_ * pl.ksplit;
    const dim3 grid((unsigned)ceil_div(M, 64), (unsigned)ceil_div(N, 64), (unsigned)batch);
    // measured: 64 x 64 tiles with a 4-stage ring; 3 stages tie, 6 / 8 stages and 128 x 128 tiles (3 stages) lose occupancy and are slower
    if (pl.kernel == kMmDma) launch_mm_dma<2, 2, 4>(s, p, tA, tB, batch);
    else if (pl.kernel == kMmBig) hipLaunchKernelGGL((k_mm_big<2, 2>), grid, dim3(256), 0, s, p, pl.vecA, pl.vecB);
    else hipLaunchKernelGGL(k_mm, grid, dim3(256), 0, s, p);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}


// ------------------------------------------------------------------------------------------------
// Weight gradients, all of them in ONE launch: C_p[m][n] += sum_k A_p[k][m] * B_p[k][n] for a list of problems p that share K (= all
// token rows of the call).  Both operands are k-major ([token][feature] activations / activation gradients), the outputs are small
// (<= 800 x 200) and K is long, so the work is cut as (problem, 128-row group of m, n-chunk of <= 208 columns, K-split) and every
// workgroup runs its whole K-range with 26 accumulator tiles per wave (32 rows x 208 columns): 26 MFMAs per 15 LDS operand reads,
// against 4 per 4 in the general kernel, and the partial tiles meet by float atomics ONCE per (workgroup, tile) — with all problems of
// both layers in one grid a K-split of ~11 fills the chip, where the general path split every product 100 ways (400 MB of atomics
// per step at the chip-wide 1.3 TB/s atomic rate).  Operands arrive by LDS-DMA in the row-contiguous block layout of k_mm_dma
// (conflict-free ds_read_b32 in the permuted k order); A blocks are private to their wave, the 13 B blocks are shared.  The column
// sums of A (the bias gradient that belongs to the weight gradient) fall out of the A operand registers.  The finished tiles leave
// through a wave-private LDS image so that every atomic wave-instruction adds 256 contiguous bytes (MI355X_MICROARCH.md, global float
// atomics: 64 lanes in 64 rows run 17x slower).
// ------------------------------------------------------------------------------------------------
constexpr int kDwNS = 3, kDwStage = 22 * 256, kDwLdsBytes = kDwNS * kDwStage * 4;      // DwProblem, DwArgs, kDwMaxProblems / kDwMaxItems: gemm.h
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // the m0 clobber is reported once per inlined copy
__device__ __forceinline__ void dw_dma(const float* gsrc_lane, int lds_float_off_uniform) {      // see v3::dma_frag (fused3_device.h)
    const unsigned m0v = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_groupstaticsize() + 4u * (unsigned)lds_float_off_uniform);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc_lane), "s"(m0v) : "memory", "m0");
}
#pragma clang diagnostic pop
__global__ __launch_bounds__(256, 2) void k_dw_grouped(const DwArgs a) {
    extern __shared__ __attribute__((aligned(16))) float dw_lds[];
    const int it = blockIdx.x % a.nitems, ks = blockIdx.x / a.nitems;
    const unsigned code = a.item[it];
    const DwProblem& P = a.prob[code >> 12];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int m0 = 128 * (int)((code >> 6) & 63) + 32 * wave, n0 = P.ncw * (int)(code & 63);
    const int ncols = P.N - n0 < P.ncw ? P.N - n0 : P.ncw;
    const bool act = m0 < P.M;
    const int kbeg = ks * a.kchunk, kend = kbeg + a.kchunk < a.K ? kbeg + a.kchunk : a.K;
    const int nst = (kend - kbeg + 15) >> 4;
    // this lane's piece of a 16 x 16 block: k = kL, rows / columns 4 (lane & 3) .. +3.  Rows / columns outside the matrix read the zero
    // page with stride 0, so the per-step address update is one add and nothing is loaded from the argument block inside the loop
    const int kL = 4 * ((lane >> 2) & 3) + (lane >> 4), rL = 4 * (lane & 3);
    const int lda = P.lda, ldb = P.ldb;
    const float* pa[2]; const float* pb[4];
    size_t sa[2], sb[4];
    int lb[4];                                           // LDS block of this wave's B loads (21 = dummy)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + 16 * i + rL;
        const bool ok = row < P.M;
        pa[i] = ok ? P.A + (size_t)(kbeg + kL) * lda + row : g_zero_page;
        sa[i] = ok ? (size_t)16 * lda : 0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int j = wave + 4 * u;                      // blocks 0 .. 12; u = 3 exists for wave 0 only
        const int col = 16 * j + rL;
        const bool ok = j < 13 && col < ncols;
        lb[u] = j < 13 ? 8 + j : 21;
        pb[u] = ok ? P.B + (size_t)(kbeg + kL) * ldb + n0 + col : g_zero_page;
        sb[u] = ok ? (size_t)16 * ldb : 0;
    }
    const int nfull = (kend - kbeg) >> 4;                // steps whose 16 k all exist
    int slot = 0;                                        // ring slot of the next issue, floats
    auto issue = [&](int t) {                            // k-step t -> next ring slot; six DMAs per wave whatever t (uniform vmcnt)
        if (t < nfull) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { dw_dma(pa[i], slot + 256 * (2 * wave + i)); pa[i] += sa[i]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) { dw_dma(pb[u], slot + 256 * lb[u]); pb[u] += sb[u]; }
        } else {                                         // the K tail of the last split, and the two issues beyond the end: zeros
            const bool kin = t < nst && kbeg + 16 * t + kL < kend;
#pragma unroll
            for (int i = 0; i < 2; ++i) dw_dma(kin ? pa[i] : g_zero_page, slot + 256 * (2 * wave + i));
#pragma unroll
            for (int u = 0; u < 4; ++u) dw_dma(kin ? pb[u] : g_zero_page, slot + 256 * lb[u]);
        }
        slot = slot == (kDwNS - 1) * kDwStage ? 0 : slot + kDwStage;
    };
    f4 acc[2][13];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 13; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
    float csum[2] = {0.f, 0.f};
    issue(0);
    issue(1);
    const int roff = 4 * (4 * g + (c >> 2)) + (c & 3);   // element (row c, k = 4 g + r) of a block sits at float 64 r + roff
    int rslot = 0;                                       // ring slot of the step being multiplied
    for (int t = 0; t < nst; ++t) {
        asm volatile("s_waitcnt vmcnt(6)\n\ts_barrier" ::: "memory");      // this wave's step-t loads have landed; everybody is done with step t - 1
        issue(t + 2);
        if (act) {
            const float* as = dw_lds + rslot + 512 * wave + roff;
            const float* bs = dw_lds + rslot + 2048 + roff;
            float av[2][2], bv[2][13];
            av[0][0] = as[0]; av[0][1] = as[256];
#pragma unroll
            for (int j = 0; j < 13; ++j) bv[0][j] = bs[256 * j];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r + 1 < 4) {
                    av[(r + 1) & 1][0] = as[64 * (r + 1)]; av[(r + 1) & 1][1] = as[256 + 64 * (r + 1)];
#pragma unroll
                    for (int j = 0; j < 13; ++j) bv[(r + 1) & 1][j] = bs[256 * j + 64 * (r + 1)];
                }
                __builtin_amdgcn_sched_barrier(0);
                csum[0] += av[r & 1][0]; csum[1] += av[r & 1][1];
#pragma unroll
                for (int j = 0; j < 13; ++j) {
                    acc[0][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r & 1][0], bv[r & 1][j], acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r & 1][1], bv[r & 1][j], acc[1][j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        rslot = rslot == (kDwNS - 1) * kDwStage ? 0 : rslot + kDwStage;
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");          // the trailing zero-page loads have landed, the ring is free
    if (!act) return;
    if (P.colsum != nullptr && n0 == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float v = csum[i];
            v += __shfl_xor(v, 16, 64);
            v += __shfl_xor(v, 32, 64);
            const int m = m0 + 16 * i + c;
            if (g == 0 && m < P.M) atomicAdd(P.colsum + m, v);
        }
    }
    float* img = dw_lds + wave * (16 * 208);             // wave-private [16][ncols]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int j = 0; j < 13; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * j + c < ncols) img[(4 * g + r) * ncols + 16 * j + c] = acc[i][j][r];
        int row = 0, n = lane;
        for (int f = lane; f < 16 * ncols; f += 64, n += 64) {
            while (n >= ncols) { n -= ncols; ++row; }
            const int m = m0 + 16 * i + row;
            if (m < P.M) atomicAdd(P.C + (size_t)m * P.ldc + n0 + n, img[f]);
        }
    }
}

int DwList::launch(hipStream_t s, int K) {
    if (nprob == 0 || K <= 0) return DYGNN_OK;
    // K-split: about two workgroups per CU over the whole grid, K-ranges of whole 16-wide steps
    int ksplit = 512 / args.nitems;
    if (ksplit < 1) ksplit = 1;
    int kchunk = (((K + ksplit - 1) / ksplit) + 15) & ~15;
    if (kchunk < 32) kchunk = 32;            // (a short K — the link predictor's 200 rows — is still worth splitting: each 16-wide step is a DMA round trip)
    ksplit = (K + kchunk - 1) / kchunk;
    args.K = K; args.kchunk = kchunk;
    DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_dw_grouped), hipFuncAttributeMaxDynamicSharedMemorySize, kDwLdsBytes));
    hipLaunchKernelGGL(k_dw_grouped, dim3((unsigned)(args.nitems * ksplit)), dim3(256), kDwLdsBytes, s, args);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

int dw_grouped(hipStream_t s, int K, const DwPair* pairs, int npairs) {
    DwList dw;
    for (int i = 0; i < npairs; ++i) dw.add(pairs[i].A, pairs[i].lda, pairs[i].M, pairs[i].B, pairs[i].ldb, pairs[i].N, pairs[i].C, pairs[i].ldc, pairs[i].colsum);
    if (!dw.ok) { set_error("dw_grouped: operands are not 16-byte aligned / too many problems"); return DYGNN_E_UNSUPPORTED; }
    return dw.launch(s, K);
}

// out[n] += sum_m A[m][n]   (bias gradients): workgroup = 64 columns x a chunk of 256 rows, one atomic per column and workgroup
__global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ A, int lda, int64_t M, int N, float* __restrict__ out) {
    __shared__ float red[4][64];
    const int n = blockIdx.x * 64 + (threadIdx.x & 63), r0 = threadIdx.x >> 6;
    const int64_t mlo = (int64_t)blockIdx.y * 256, mhi = mlo + 256 < M ? mlo + 256 : M;
    float s = 0.f;
    if (n < N)
        for (int64_t m = mlo + r0; m < mhi; m += 4) s += A[m * lda + n];
    red[r0][threadIdx.x & 63] = s;
    __syncthreads();
    if (r0 == 0 && n < N) atomicAdd(&out[n], (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]));
}
int colsum_atomic(hipStream_t s, const float* A, int lda, int64_t M, int N, float* out) {      // always accumulates: gradient buffers arrive zeroed (dygnn_dygformer_backward contract)
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)ceil_div(N, 64), (unsigned)ceil_div(M, 256)), dim3(256), 0, s, A, lda, M, N, out);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace train
}  // namespace dygnn

using namespace dygnn;

// ---- the C entry points (tests/test_gemm_gpu.py) ------------------------------------------------------------------------------------------
static_assert(sizeof(dygnn_mm_args) == 168 && sizeof(dygnn_dw_pair) == 56, "the ctypes structures of _capi.py assume these layouts");
static int mm_args_check(const dygnn_mm_args* a) {
    DYGNN_REQUIRE(a != nullptr, "mm: null arguments");
    DYGNN_REQUIRE(a->M >= 0 && a->N >= 0 && a->K >= 0 && a->batch >= 0 && a->H >= 1, "mm: negative size");
    DYGNN_REQUIRE(a->A && a->B && a->C, "mm: null pointer");
    DYGNN_REQUIRE(a->lda >= (a->tA ? a->M : a->K) && a->ldb >= (a->tB ? a->K : a->N) && a->ldc >= a->N, "mm: a leading dimension is shorter than its row");
    return DYGNN_OK;
}
static train::MmOpt mm_args_opt(const dygnn_mm_args* a) {
    return train::MmOpt().bias(a->bias).alpha(a->alpha).beta(a->beta).relu(a->relu != 0).batched(a->batch, a->H).strideA(a->sAb, a->sAh).strideB(a->sBb, a->sBh)
        .strideC(a->sCb, a->sCh).c_is_zero(a->c_is_zero != 0).colsum(a->colsum_out).live_rows(a->m_dev).a_kpad(a->a_kpad != 0).rows(a->a_rows);
}

extern "C" int32_t dygnn_mm_plan(const dygnn_mm_args* a, int32_t* ksplit, int32_t* float4_epilogue) {
    if (int rc = mm_args_check(a)) return rc;
    train::MmPlan pl;
    if (int rc = train::mm_plan(a->A, a->lda, a->tA != 0, a->B, a->ldb, a->tB != 0, a->C, a->ldc, a->M, a->N, a->K, mm_args_opt(a), &pl)) return rc;
    if (ksplit) *ksplit = pl.ksplit;
    if (float4_epilogue) *float4_epilogue = pl.f4_epilogue;
    return pl.kernel;
}

extern "C" int32_t dygnn_mm_path(const dygnn_mm_args* a) { return dygnn_mm_plan(a, nullptr, nullptr); }

extern "C" int32_t dygnn_mm_gathers_rows(const float* A, int32_t lda, const float* B, int32_t ldb, int32_t M, int32_t N, int32_t K) {
    return train::mm_gathers_rows(A, lda, B, ldb, M, N, K) ? 1 : 0;
}

extern "C" int dygnn_mm(const dygnn_mm_args* a, dygnn_stream_t stream) {
    if (int rc = mm_args_check(a)) return rc;
    return train::mm(as_stream(stream), a->A, a->lda, a->tA != 0, a->B, a->ldb, a->tB != 0, a->C, a->ldc, a->M, a->N, a->K, mm_args_opt(a));
}

extern "C" int dygnn_dw_grouped(int32_t K, const dygnn_dw_pair* pairs, int32_t npairs, dygnn_stream_t stream) {
    DYGNN_REQUIRE(K >= 0 && npairs >= 0 && (npairs == 0 || pairs != nullptr), "dw_grouped: bad sizes");
    for (int32_t i = 0; i < npairs; ++i) {
        const dygnn_dw_pair& q = pairs[i];
        DYGNN_REQUIRE(q.A && q.B && q.C, "dw_grouped: null pointer");
        DYGNN_REQUIRE(q.M >= 0 && q.N >= 0 && q.lda >= q.M && q.ldb >= q.N && q.ldc >= q.N, "dw_grouped: negative size, or a leading dimension shorter than its row");
    }
    std::vector<train::DwPair> list;
    list.reserve((size_t)npairs);
    for (int32_t i = 0; i < npairs; ++i) list.push_back(train::DwPair{pairs[i].A, pairs[i].lda, pairs[i].M, pairs[i].B, pairs[i].ldb, pairs[i].N, pairs[i].C, pairs[i].ldc, pairs[i].colsum});
    return train::dw_grouped(as_stream(stream), K, list.data(), npairs);
}
