// Backward kernels of the fused DyGFormer training path, k_ffn_bwd and k_attn_bwd, and their launchers.  They run on the device primitives
// and the weight-stream protocol of the forward (fused3_device.h) over backward streams cut from the same tensors (dygformer_fused3_pack.hip).
#include <cstdlib>

#include "dropout.h"
#include "fused3_device.h"
#include "fused3_host.h"

namespace dygnn {
namespace v3 {

// ================================================================================================
// Backward of one encoder layer's FFN block (DyGFormer.py:457-460 reversed), token-owner like the forward: a workgroup = 8 waves = 128
// dense token rows, wave w owns 16 rows x all 200 channels.  In: dX = d loss / d x_{l+1} [M][200].  Per 32-unit hidden step p the two
// activation-gradient products run register to register from the layer's BACKWARD stream (W2^T then W1^T fragments of the same ring):
//     dhact^T = W2[:, step]^T . dF2^T,   dhpre = dhact o mask2 o gelu'(hpre),   dxn1^T += W1[step, :]^T . dhpre^T
// with dF2 = dX o mask3; then LayerNorm-1 backward against the stored statistics, dX <- dX + LN1'(dxn1) in place, and the LN weight /
// bias gradients (row sums by DPP, the eight waves meet in LDS, one atomic per channel and workgroup).  dF2 and dhpre are written as dense
// rows for the grouped weight-gradient launch (k_dw_grouped, gemm.hip), which also sums the bias gradients.
struct FfnBwdArgs {
    const float* stream; int nstages;
    int64_t M;
    float* dX;                                   // [M][200] in: d x_{l+1}; out: d x1
    const float *hpre, *x1, *m1, *r1;            // forward activations (dense rows)
    float *dF2, *dH;                             // [M][200], [M][800]
    float *dgamma, *dbeta;                       // LN1 (accumulated)
    train::Drop dr; uint32_t site_act, site_out;
    unsigned long long* stamps;                  // diagnostic build only
};
__device__ __forceinline__ float gelu_grad(float v) {                       // d/dv [v Phi(v)] = Phi(v) + v phi(v)
    const float cdf = 0.5f * (1.0f + erf_as(v * 0.70710678118654752440f));
    return fmaf(v * 0.39894228040143267794f, __expf(-0.5f * v * v), cdf);
}
template <int NW>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void k_ffn_bwd(const FfnBwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * (16 * NW) + 16 * wave, row = row0 + c;
    const bool active = row0 < a.M, valid = row < a.M;
    TDECL;
    WStream ws;
    ws.open(a.stream, kLdsRing, lane, wave, a.nstages, NW);
    const float* ringl = lds + kLdsRing + lane * 4;
    // dF2^T = (dX o mask3)^T: the B operand of every W2^T product of the layer
    f4 d2[kNT];
    {
        const uint32_t sk = a.dr.site_key(a.site_out), e0 = (uint32_t)row * kD + 4 * g;
        const float* src = a.dX + row * kD + 4 * g;
        float* dst = a.dF2 + row * kD + 4 * g;
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            const bool on = valid && (i < 12 || g < 2);
            f4 v = on ? ldg4(src + 16 * i) : zero4();
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] *= a.dr.mask32(sk, e0 + 16 * i + r);
            if (on) *reinterpret_cast<f4*>(dst + 16 * i) = v;
            d2[i] = v;
        }
    }
    float dk0 = 0.f, dk1 = 0.f;
    kpack(d2[kKC - 1], dk0, dk1);
    f4 dxn[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) dxn[i] = zero4();
    const uint32_t sk2 = a.dr.site_key(a.site_act);
    const float* hrow = a.hpre + row * kHid + 4 * g;
    float* dhrow = a.dH + row * kHid + 4 * g;
    f4 hp[2];
    hp[0] = valid ? ldg4(hrow) : zero4();
    hp[1] = valid ? ldg4(hrow + 16) : zero4();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the first ring stages have landed
    __syncthreads();
    TACC(0);
#pragma unroll 1
    for (int p = 0; p < 25; ++p) {
        f4 dh[2];
        f4 hn[2];
        if (active) {
            // the next step's hidden pre-activations fly through this step (issued first: the two dhpre stores below are then the two
            // youngest vector-memory operations at the stage barrier)
            const bool more = valid && p + 1 < 25;
            hn[0] = more ? ldg4(hrow + 32 * (p + 1)) : zero4();
            hn[1] = more ? ldg4(hrow + 32 * (p + 1) + 16) : zero4();
            ffn_w1(dh, d2, dk0, dk1, ringl + ws.pos * kFrag, nullptr, g);
            TACC(1);
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    dh[u][r] *= a.dr.mask32(sk2, (uint32_t)row * kHid + 32 * p + 16 * u + 4 * g + r) * gelu_grad(hp[u][r]);
            // take the prefetched rows NOW, before the stores below are issued: vmcnt retires in order and the compiler does not see the ring's
            // DMAs, so a wait for these loads placed behind the stores would also sit out the stores' whole round trip
            hp[0] = hn[0]; hp[1] = hn[1];
            asm volatile("" : "+v"(hp[0]), "+v"(hp[1]));
        }
        TACC(2);
        ws.advance(26);
        TACC(3);
        // the dhpre rows leave AFTER the stage barrier's DMA issue: at the next barrier they are the two youngest operations and stay in flight
        // (vmcnt(2) proves the older DMAs landed), and they have both blocks of the next step to retire before a full drain
        if (valid) { *reinterpret_cast<f4*>(dhrow + 32 * p) = dh[0]; *reinterpret_cast<f4*>(dhrow + 32 * p + 16) = dh[1]; }
        if (active) ffn_w2(dxn, dh, ringl + ws.pos * kFrag);
        TACC(4);
        ws.advance(26, active ? 2 : 0);
        TACC(5);
    }
    // LayerNorm-1 backward (x1 rows and their statistics from the forward): dx1 = dX + rstd (gy - mean(gy) - xhat mean(gy xhat)), gy = dxn gamma
    ws.fit(1);
    const float* gam = lds + kLdsRing + ws.pos * kFrag + 4 * g;
    float* red = lds;                            // [8 waves][2][208] partial sums of dgamma / dbeta (the K/V region is unused here)
    {
        const float mean = valid ? a.m1[row] : 0.f, rstd = valid ? a.r1[row] : 0.f;
        const float* xr = a.x1 + row * kD + 4 * g;
        f4 xh[kNT];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            const bool on = valid && (i < 12 || g < 2);
            const f4 xv = on ? ldg4(xr + 16 * i) : zero4();
            const f4 gm = lds4(gam + 16 * i);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                xh[i][r] = on ? (xv[r] - mean) * rstd : 0.f;
                const float gy = dxn[i][r] * gm[r];
                s1 += gy; s2 = fmaf(gy, xh[i][r], s2);
            }
        }
        s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
        const float m1v = s1 * (1.0f / kD), m2v = s2 * (1.0f / kD);
        float* dxr = a.dX + row * kD + 4 * g;
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            const bool on = valid && (i < 12 || g < 2);
            const f4 gm = lds4(gam + 16 * i);
            f4 pg, pb;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pg[r] = row_sum16(dxn[i][r] * xh[i][r]);
                pb[r] = row_sum16(dxn[i][r]);
            }
            if (c == 0) {
                *reinterpret_cast<f4*>(red + (wave * 2 + 0) * kDP + 16 * i + 4 * g) = pg;
                *reinterpret_cast<f4*>(red + (wave * 2 + 1) * kDP + 16 * i + 4 * g) = pb;
            }
            if (on) {
                f4 v = ldg4(dxr + 16 * i);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += rstd * (dxn[i][r] * gm[r] - m1v - xh[i][r] * m2v);
                *reinterpret_cast<f4*>(dxr + 16 * i) = v;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // no LDS-DMA of this workgroup is left in flight
    __syncthreads();
    TACC(6);
    for (int i = tid; i < 2 * kDP; i += 64 * NW) {
        const int which = i / kDP, n = i % kDP;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += red[(w * 2 + which) * kDP + n];
        if (n < kD) atomicAdd((which ? a.dbeta : a.dgamma) + n, t);
    }
    TACC(7);
    TSTORE();
}

// the 13 register tiles of a token-owner wave from dense row `row` of a [M][200] buffer (rows 16 i + 4 g + r of token c)
__device__ __forceinline__ void load_rows(f4 (&x)[kNT], const float* base, int64_t row, int g, bool valid) {
#pragma unroll
    for (int i = 0; i < kNT; ++i) x[i] = (valid && (i < 12 || g < 2)) ? ldg4(base + row * kD + 4 * g + 16 * i) : zero4();
}
// LayerNorm backward of a token-owner wave against stored statistics (shared by the two backward kernels): dX rows += rstd (gy - mean(gy) -
// xhat mean(gy xhat)), gy = dxn gamma; the workgroup's sums of dxn xhat / dxn over its tokens go to `red` [8 waves][2][208]
__device__ __forceinline__ void ln_backward(const f4 (&dxn)[kNT], const float* xrows, const float* mean_p, const float* rstd_p, const float* gam, float* dXrows,
                                            int64_t row, bool valid, float* red, int wave, int c, int g) {
    const float mean = valid ? mean_p[row] : 0.f, rstd = valid ? rstd_p[row] : 0.f;
    const float* xr = xrows + row * kD + 4 * g;
    f4 xh[kNT];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const bool on = valid && (i < 12 || g < 2);
        const f4 xv = on ? ldg4(xr + 16 * i) : zero4();
        const f4 gm = lds4(gam + 16 * i);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            xh[i][r] = on ? (xv[r] - mean) * rstd : 0.f;
            const float gy = dxn[i][r] * gm[r];
            s1 += gy; s2 = fmaf(gy, xh[i][r], s2);
        }
    }
    s1 += __shfl_xor(s1, 16, 64); s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64); s2 += __shfl_xor(s2, 32, 64);
    const float m1v = s1 * (1.0f / kD), m2v = s2 * (1.0f / kD);
    float* dxr = dXrows + row * kD + 4 * g;
    f4 dxv[kNT];                                 // the incoming gradient rows: all loads in flight before the tile-by-tile pass
#pragma unroll
    for (int i = 0; i < kNT; ++i) dxv[i] = (valid && (i < 12 || g < 2)) ? ldg4(dxr + 16 * i) : zero4();
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const bool on = valid && (i < 12 || g < 2);
        const f4 gm = lds4(gam + 16 * i);
        f4 pg, pb;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pg[r] = row_sum16(dxn[i][r] * xh[i][r]);
            pb[r] = row_sum16(dxn[i][r]);
        }
        if (c == 0) {
            *reinterpret_cast<f4*>(red + (wave * 2 + 0) * kDP + 16 * i + 4 * g) = pg;
            *reinterpret_cast<f4*>(red + (wave * 2 + 1) * kDP + 16 * i + 4 * g) = pb;
        }
        if (on) {
            f4 v = dxv[i];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] += rstd * (dxn[i][r] * gm[r] - m1v - xh[i][r] * m2v);
            *reinterpret_cast<f4*>(dxr + 16 * i) = v;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// ================================================================================================
// Backward of one encoder layer's attention block (DyGFormer.py:440-456 reversed; nn.MultiheadAttention with dropout on the probabilities),
// token-owner like the forward: a workgroup = 8 waves = NP pairs x TPW token tiles, wave = 16 tokens x all channels.
// In: dX = d loss / d x1 [M][200] (after k_ffn_bwd).  dAo = dX o mask1 is written as rows (the out-projection's weight-gradient operand) and,
// per head h, streamed through the layer's backward ring:
//     dOa^T = Wo[:, h]^T . dAo^T                                                                    (same shape as a Q/K/V product)
//     phase A, this wave's tokens as QUERIES (K, V of the pair in LDS):  dPd^T = V . dOa^T,  dS^T = P^T o (dPd^T o mask0 - D),  dQ^T = K^T . dS^T
//     phase B, this wave's tokens as KEYS (Q, dOa of the pair in LDS over K, V):  dPd = dOa . V^T,  dS = P o (dPd o mask0 - D),
//              dV^T = dOa^T . Pd,  dK^T = Q^T . dS            — tiles [query rows][own key columns] are again MFMA B operands, so the sums over
//              the pair's queries need no cross-wave exchange beyond D (one float per query, through LDS); P and Pd are re-read from the
//              forward's [B H][T][T] buffers in either orientation
//     dxn0^T += Wq[h]^T . dQ^T + Wv[h]^T . dV^T + Wk[h]^T . dK^T                                     (same shape as the out-projection)
// then LayerNorm-0 backward, dX <- dX + LN0'(dxn0) in place = d loss / d x_l.  dQ | dK | dV leave as rows [M][600] for the grouped
// weight-gradient launch.  scale = 1/sqrt(head dim) multiplies dS once (it serves both dQ and dK: S = scale q.k).
struct AttnBwdArgs {
    const float* stream; int nstages;
    int64_t B; int T;
    float* dX;                                   // [M][200] in: d x1; out: d x_l
    const float *X, *m0, *r0;                    // layer input rows and LN0 statistics
    const float *qkv, *P, *Pd;                   // forward activations
    float *dAo, *dQKV;                           // [M][200], [M][600]
    float *dgamma, *dbeta;                       // LN0 (accumulated)
    train::Drop dr; uint32_t site_p, site_ao;
    float qscale;
    unsigned long long* stamps;                  // diagnostic build only
};
template <int TPW, int NW = 8>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void k_attn_bwd(const AttnBwdArgs a) {
    constexpr int NP = NW / TPW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pi = wave / TPW, tt = wave % TPW;
    const int c = lane & 15, g = lane >> 4;
    const int64_t b = (int64_t)blockIdx.x * NP + pi;
    const int T = a.T;
    const bool pair_ok = b < a.B;
    const bool active = pair_ok && 16 * tt < T, valid = pair_ok && 16 * tt + c < T;
    const int tok = 16 * tt + c;
    const int64_t row = b * T + tok;
    const int tokbase = pi * (16 * TPW);
    TDECL;
    WStream ws;
    ws.open(a.stream, kLdsRing, lane, wave, a.nstages, NW);
    const float* ringl = lds + kLdsRing + lane * 4;
    float* Kb = lds + kLdsK;
    float* Vb = lds + kLdsV;
    float* Dq = lds + kLdsMisc;                  // [128] D of every query of the workgroup
    for (int i = tid; i < kLdsRing / 4; i += 64 * NW) reinterpret_cast<f4*>(lds)[i] = zero4();      // rows of absent tokens are MFMA operands: finite
    for (int i = tid; i < kTokWG; i += 64 * NW) Dq[i] = 0.f;
    // dAo = dX o mask1 (DyGFormer.py:456), as rows: the operand of the out-projection's weight gradient and of the dOa products below
    {
        const uint32_t sk = a.dr.site_key(a.site_ao), e0 = (uint32_t)row * kD + 4 * g;
        const float* src = a.dX + row * kD + 4 * g;
        float* dst = a.dAo + row * kD + 4 * g;
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            if (valid && (i < 12 || g < 2)) {
                f4 v = ldg4(src + 16 * i);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] *= a.dr.mask32(sk, e0 + 16 * i + r);
                *reinterpret_cast<f4*>(dst + 16 * i) = v;
            }
        }
    }
    f4 dxn[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) dxn[i] = zero4();
    const uint32_t skp = a.dr.site_key(a.site_p);
    const bool vec = (T & 3) == 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the first ring stages have landed (and this lane's dAo row is written)
    __syncthreads();
    TACC(0);
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {
        const float* qrow = a.qkv + row * (3 * kD) + kHD * h + 4 * g;
        float* drow = a.dQKV + row * (3 * kD) + kHD * h + 4 * g;
        const int64_t pbase = (b * 2 + h) * (int64_t)T * T;
        // ---- K and V rows of the pair go to LDS by DMA (no registers) and this wave's Q rows (needed in phase B) into registers NOW: they land
        // while the Wo^T product runs.  (Every wave passed stream barriers since the previous head's last reads of the K/V region.)
        {
            constexpr int NCH = 16 * TPW * kKV * 4 / 1024;             // 1-KiB pieces of a pair's K (or V) block: rows are contiguous in LDS
            for (int q = tt; q < NCH; q += TPW) {
                const int o = 1024 * q + 16 * lane, r = o / (4 * kKV), cb = (o - r * 4 * kKV) >> 2;
                const bool on = pair_ok && r < T;
                const float* src = a.qkv + (b * T + r) * (3 * kD) + kHD * h + cb;
                dma_frag(on ? src + kD : g_zero16, kLdsK + tokbase * kKV + 256 * q);
                dma_frag(on ? src + 2 * kD : g_zero16, kLdsV + tokbase * kKV + 256 * q);
            }
        }
        f4 qrows[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) qrows[j] = (valid && (j < 6 || g == 0)) ? ldg4(qrow + 16 * j) : zero4();
        // ---- dOa^T = Wo[:, h]^T . dAo^T
        f4 doa[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) doa[j] = zero4();
        {
            f4 dA[kNT];
            load_rows(dA, a.dAo, row, g, valid);
            float k0 = 0.f, k1 = 0.f;
            kpack(dA[kKC - 1], k0, k1);
            qkv_group(doa, dA, k0, k1, ws, ringl, active);
        }
        TACC(1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of K and V have landed
        __syncthreads();
        TACC(2);
        // ---- phase A: this wave's tokens as queries
        f4 dq[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) dq[j] = zero4();
        if (active) {
            f4 ds[TPW], pt[TPW];
#pragma unroll
            for (int kt = 0; kt < TPW; ++kt) ds[kt] = zero4();
            s_like<TPW>(ds, Vb + tokbase * kKV, doa, c, g);                    // dPd^T[key][query]
            const float* Pq = a.P + pbase + (int64_t)tok * T;
            float D = 0.f;
#pragma unroll
            for (int kt = 0; kt < TPW; ++kt) {
                const int key0 = 16 * kt + 4 * g;
                if (vec) pt[kt] = (valid && key0 < T) ? ldg4(Pq + key0) : zero4();
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pt[kt][r] = (valid && key0 + r < T) ? Pq[key0 + r] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ds[kt][r] *= a.dr.mask32(skp, (uint32_t)(pbase + (int64_t)tok * T) + key0 + r);       // dP = dPd o mask0
                    D = fmaf(ds[kt][r], pt[kt][r], D);
                }
            }
            D += __shfl_xor(D, 16, 64);
            D += __shfl_xor(D, 32, 64);
#pragma unroll
            for (int kt = 0; kt < TPW; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) ds[kt][r] = pt[kt][r] * (ds[kt][r] - D) * a.qscale;
            if (g == 0) Dq[tokbase + tok] = D;
            pv_like<TPW>(dq, Kb + tokbase * kKV, ds, c, g);                    // dQ^T = K^T . dS^T (scaled)
        }
        f4 vt[7];                                    // this wave's V^T tiles for phase B, from its own rows while they are still in LDS
#pragma unroll
        for (int j = 0; j < 7; ++j) vt[j] = (active && (j < 6 || g == 0)) ? lds4(Vb + (tokbase + tok) * kKV + 4 * g + 16 * j) : zero4();
        TACC(3);
        __syncthreads();                             // every wave is done with K and V
        // ---- Q (unscaled, from the registers loaded above) and dOa rows over K and V; this wave's own V rows (its tokens as keys) were read
        // back from LDS before the barrier: the exchange touches no global memory
        if (active) {
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < 6 || g == 0) {
                    *reinterpret_cast<f4*>(Kb + (tokbase + tok) * kKV + 4 * g + 16 * j) = qrows[j];
                    *reinterpret_cast<f4*>(Vb + (tokbase + tok) * kKV + 4 * g + 16 * j) = doa[j];
                }
        }
        __syncthreads();
        TACC(4);
        // dxn0 += Wq[h]^T . dQ^T while the exchange settles (stream order: Wo^T, Wq^T, Wv^T, Wk^T)
        proj_t(dxn, dq, ws, ringl, active);
        // the row stores of dQ (and of dV, dK below) come AFTER the loads that follow their computation: a load behind a store waits for the
        // store's round trip (in-order vmcnt)
        if (valid) {
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < 6 || g == 0) *reinterpret_cast<f4*>(drow + 16 * j) = dq[j];
        }
        TACC(5);
        // ---- phase B: this wave's tokens as keys; tiles [query rows 16 qt + 4 g + r][own key column c]
        f4 dv[7], dk[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) { dv[j] = zero4(); dk[j] = zero4(); }
        {
            f4 ds2[TPW], pd2[TPW];
#pragma unroll
            for (int qt = 0; qt < TPW; ++qt) { ds2[qt] = zero4(); pd2[qt] = zero4(); }
            if (active) {
                s_like<TPW>(ds2, Vb + tokbase * kKV, vt, c, g);                // dPd[query][key] = dOa[query] . V[key]
#pragma unroll
                for (int qt = 0; qt < TPW; ++qt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int q = 16 * qt + 4 * g + r;
                        const bool on = valid && q < T;
                        const int64_t off = pbase + (int64_t)q * T + tok;
                        const float pv = on ? a.P[off] : 0.f;
                        pd2[qt][r] = on ? a.Pd[off] : 0.f;
                        const float dp = ds2[qt][r] * a.dr.mask32(skp, (uint32_t)off);
                        ds2[qt][r] = pv * (dp - Dq[tokbase + q]) * a.qscale;
                    }
                pv_like<TPW>(dv, Vb + tokbase * kKV, pd2, c, g);               // dV^T = dOa^T . Pd
            }
            TACC(6);
            proj_t(dxn, dv, ws, ringl, active);
            TACC(7);
            if (active) pv_like<TPW>(dk, Kb + tokbase * kKV, ds2, c, g);       // dK^T = Q^T . dS (scaled)
        }
        TACC(8);
        proj_t(dxn, dk, ws, ringl, active);
        if (valid) {
#pragma unroll
            for (int j = 0; j < 7; ++j)
                if (j < 6 || g == 0) { *reinterpret_cast<f4*>(drow + 2 * kD + 16 * j) = dv[j]; *reinterpret_cast<f4*>(drow + kD + 16 * j) = dk[j]; }
        }
        TACC(9);
    }
    // ---- LayerNorm-0 backward
    ws.fit(1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                 // every wave is done with the K/V region: it now holds the dgamma / dbeta partial sums
    ln_backward(dxn, a.X, a.m0, a.r0, lds + kLdsRing + ws.pos * kFrag + 4 * g, a.dX, row, valid, lds, wave, c, g);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int i = tid; i < 2 * kDP; i += 64 * NW) {
        const int which = i / kDP, n = i % kDP;
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += lds[(w * 2 + which) * kDP + n];
        if (n < kD) atomicAdd((which ? a.dbeta : a.dgamma) + n, t);
    }
    TACC(10);
    TSTORE();
}

}  // namespace v3

// FFN block of layer l, backward (k_ffn_bwd); the caller's buffers are the dense rows of dygformer_train.hip's Plan
int ffn_backward_fused3(const Dims& d, const PackedLayout& pl, const float* packed, int l, int64_t M, float* dX, const float* hpre, const float* x1,
                        const float* m1, const float* r1, float* dF2, float* dH, float* dgamma, float* dbeta, const train::Drop& dr, hipStream_t s) {
    using namespace v3;
    if (!supported(d)) { set_error("fused FFN backward: unsupported shape"); return DYGNN_E_UNSUPPORTED; }
    const PackLayout3 f = make_layout3(d);
    FfnBwdArgs a{};
    a.stream = packed + pl.fused3 + f.bwd[l]; a.nstages = f.bwd_nstages;
    a.M = M; a.dX = dX; a.hpre = hpre; a.x1 = x1; a.m1 = m1; a.r1 = r1; a.dF2 = dF2; a.dH = dH; a.dgamma = dgamma; a.dbeta = dbeta;
    a.dr = dr; a.site_act = (uint32_t)(4 * l + 2); a.site_out = (uint32_t)(4 * l + 3);
#ifdef DYGNN_STAMPS
    if (const char* sp = getenv("DYGNN_STAMPS_FFN")) a.stamps = reinterpret_cast<unsigned long long*>(strtoull(sp, nullptr, 0));
#endif
    if (M <= (int64_t)kSmallBatchPairs * 64 && !small_off()) {
        DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ffn_bwd<4>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        hipLaunchKernelGGL(k_ffn_bwd<4>, dim3((unsigned)ceil_div(M, (int64_t)64)), dim3(256), kLdsBytes, s, a);
    } else {
        DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ffn_bwd<8>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        hipLaunchKernelGGL(k_ffn_bwd<8>, dim3((unsigned)ceil_div(M, (int64_t)kTokWG)), dim3(512), kLdsBytes, s, a);
    }
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

// Attention block of layer l, backward (k_attn_bwd); B pairs of T tokens each (one group: the training path's dense layout)
int attn_backward_fused3(const Dims& d, const PackedLayout& pl, const float* packed, int l, int64_t B, int T, float* dX, const float* X, const float* m0,
                         const float* r0, const float* qkv, const float* P, const float* Pd, float* dAo, float* dQKV, float* dgamma, float* dbeta,
                         const train::Drop& dr, hipStream_t s) {
    using namespace v3;
    if (!supported(d) || T > 128) { set_error("fused attention backward: unsupported shape"); return DYGNN_E_UNSUPPORTED; }
    const PackLayout3 f = make_layout3(d);
    AttnBwdArgs a{};
    a.stream = packed + pl.fused3 + f.bwa[l]; a.nstages = f.bwa_nstages;
    a.B = B; a.T = T; a.dX = dX; a.X = X; a.m0 = m0; a.r0 = r0; a.qkv = qkv; a.P = P; a.Pd = Pd; a.dAo = dAo; a.dQKV = dQKV; a.dgamma = dgamma; a.dbeta = dbeta;
    a.dr = dr; a.site_p = (uint32_t)(4 * l + 0); a.site_ao = (uint32_t)(4 * l + 1);
    a.qscale = (float)sqrt(1.0 / (double)d.hd);
#ifdef DYGNN_STAMPS
    if (const char* sp = getenv("DYGNN_STAMPS_ATTN")) a.stamps = reinterpret_cast<unsigned long long*>(strtoull(sp, nullptr, 0));
#endif
    DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_bwd<4>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_bwd<8>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
    if (T <= 64 && B <= kSmallBatchPairs && !small_off()) {
        DYGNN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_attn_bwd<4, 4>), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes));
        hipLaunchKernelGGL((k_attn_bwd<4, 4>), dim3((unsigned)B), dim3(256), kLdsBytes, s, a);
    } else if (T <= 64) hipLaunchKernelGGL(k_attn_bwd<4>, dim3((unsigned)((B + 1) / 2)), dim3(512), kLdsBytes, s, a);
    else hipLaunchKernelGGL(k_attn_bwd<8>, dim3((unsigned)B), dim3(512), kLdsBytes, s, a);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace dygnn
