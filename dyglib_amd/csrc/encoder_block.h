// The tail of a TransformerEncoder block (models/modules.py:257-264) at inference, shared by tcl.hip and cawn.hip: out_proj + residual,
// LayerNorm, d -> 4d (ReLU) -> d, residual, LayerNorm, all products fp32 MFMA (mfma_tile.h).  gfx950 only.
#pragma once
#include "common.h"
#include "mfma_tile.h"

namespace dygnn {
namespace encoder {

using tile::f4;
using tile::kThreads;
using tile::kWaves;
using tile::round16;
using tile::wave_product;
using tile::z4;

constexpr int kFfnChunk = 64;     // hidden columns in LDS at a time
constexpr float kLnEps = 1e-5f;

// Where the residual of token row r lives in Xres [.][S][d]: r is query position r % nq of attention output sequence r / nq, its residual
// that position of sequence seq[r / nq] (r / nq when NULL).  {NULL, S, S} is the identity: row r of Xres [R][d].
struct ResMap {
    const int32_t* seq;
    int nq, S;
};

// the rows r0 .. r0 + rows - 1 of X [R][d] into the LDS tile A [rows][lda], zero beyond d and beyond R
__device__ __forceinline__ void load_rows(float* A, int lda, int rows, const float* __restrict__ X, int64_t r0, int64_t R, int d) {
    const int d4 = d >> 2, lda4 = lda >> 2;
    for (int i = threadIdx.x; i < rows * lda4; i += kThreads) {
        const int r = i / lda4, c4 = i - r * lda4;
        f4 v = z4();
        if (c4 < d4 && r0 + r < R) v = *reinterpret_cast<const f4*>(X + (size_t)(r0 + r) * d + 4 * c4);
        *reinterpret_cast<f4*>(A + r * lda + 4 * c4) = v;
    }
}

// LayerNorm of the rows of the LDS tile A in place, one wave per row
__device__ __forceinline__ void norm_rows(float* A, int lda, int rows, int d, const float* __restrict__ ln_w, const float* __restrict__ ln_b, int wave, int lane) {
    for (int r = wave; r < rows; r += kWaves) {
        float* row = A + r * lda;
        float s = 0.f;
        for (int f = lane; f < d; f += 64) s += row[f];
        const float mean = wave_sum(s) / (float)d;
        float v = 0.f;
        for (int f = lane; f < d; f += 64) { const float x = row[f] - mean; v = fmaf(x, x, v); }
        const float rstd = 1.0f / sqrtf(wave_sum(v) / (float)d + kLnEps);
        for (int f = lane; f < d; f += 64) row[f] = fmaf((row[f] - mean) * rstd, ln_w[f], ln_b[f]);
    }
}

// ---- the rest of the block for R token rows, 16 MT of them per workgroup, NT column tiles per wave (d <= 64 NT) ---------------------------------
// out_proj + bias + residual (ResMap) -> LayerNorm 0 -> A; linear 0, ReLU, linear 1 as in k_gm_ffn (graphmixer.hip): per chunk of 64 hidden
// columns, wave w computes 16 of them for all rows into Hc, then every wave adds the chunk to its output tiles; + bias + A -> LayerNorm 1
// -> out [R][d].  MT = 2 past 256 columns: 50 KiB of LDS instead of 100, three workgroups per CU instead of one.
// LDS: A [16 MT][round16(d) + 4], Hc [16 MT][68] (post_lds_bytes).
template <int NT, int MT>
static __global__ __launch_bounds__(kThreads) void k_encoder_post(const float* __restrict__ O, int64_t R, const float* __restrict__ Xres, ResMap map,
                                                                    dygnn_tcl_layer_weights w, int d, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lda = round16(d) + 4, ldh = kFfnChunk + 4, Hdim = 4 * d;
    float* A = smem;
    constexpr int rows = 16 * MT;
    float* Hc = smem + rows * lda;
    const int64_t r0 = (int64_t)blockIdx.x * rows;
    const int c = lane & 15, g4 = 4 * (lane >> 4);
    load_rows(A, lda, rows, O, r0, R, d);
    __syncthreads();
    f4 acc[NT][MT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = z4();
    wave_product<NT, MT>(A, lda, w.out_proj_w, d, 0, d, d, wave, lane, acc);
    __syncthreads();                                                 // every wave has read the attention rows
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int64_t r = r0 + 16 * mt + c;
        const float* res = nullptr;
        if (r < R) {
            const int64_t seq = r / map.nq;
            res = Xres + ((size_t)(map.seq ? map.seq[seq] : seq) * map.S + (r - seq * map.nq)) * d;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = 16 * (wave + kWaves * t) + g4;
            if (n >= d) continue;
            f4 v = z4();
            if (res) v = (acc[t][mt] + *reinterpret_cast<const f4*>(w.out_proj_b + n)) + *reinterpret_cast<const f4*>(res + n);
            *reinterpret_cast<f4*>(A + (16 * mt + c) * lda + n) = v;
        }
    }
    __syncthreads();
    norm_rows(A, lda, rows, d, w.norm0_w, w.norm0_b, wave, lane);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[t][mt] = z4();
    for (int h0 = 0; h0 < Hdim; h0 += kFfnChunk) {
        const int hn = Hdim - h0 < kFfnChunk ? Hdim - h0 : kFfnChunk;      // live hidden columns of this chunk (a multiple of 16)
        f4 hid[1][MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) hid[0][mt] = z4();
        wave_product<1, MT>(A, lda, w.fc0_w + (size_t)h0 * d, d, 0, hn, d, wave, lane, hid);
        {
            const int hcol = 16 * wave + g4;                           // column inside the chunk
            f4 b = z4();
            if (hcol < hn) b = *reinterpret_cast<const f4*>(w.fc0_b + h0 + hcol);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                f4 v = z4();
                if (hcol < hn) {
                    const f4 z = hid[0][mt] + b;
                    v = f4{fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
                }
                *reinterpret_cast<f4*>(Hc + (16 * mt + c) * ldh + hcol) = v;      // dead columns are zero: stage 2 runs over the whole chunk
            }
        }
        __syncthreads();
        wave_product<NT, MT>(Hc, ldh, w.fc1_w, Hdim, h0, d, hn, wave, lane, acc);
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = 16 * (wave + kWaves * t) + g4;
        if (n >= d) continue;
        const f4 b = *reinterpret_cast<const f4*>(w.fc1_b + n);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            f4* p = reinterpret_cast<f4*>(A + (16 * mt + c) * lda + n);      // this lane's own elements: no other lane reads them before the barrier
            *p = (acc[t][mt] + b) + *p;
        }
    }
    __syncthreads();
    norm_rows(A, lda, rows, d, w.norm1_w, w.norm1_b, wave, lane);
    __syncthreads();
    const int d4 = d >> 2;
    for (int i = threadIdx.x; i < rows * d4; i += kThreads) {
        const int r = i / d4, c4 = i - r * d4;
        if (r0 + r < R) *reinterpret_cast<f4*>(out + (size_t)(r0 + r) * d + 4 * c4) = *reinterpret_cast<const f4*>(A + r * lda + 4 * c4);
    }
}

inline size_t post_lds_bytes(int MT, int d) { return (size_t)16 * MT * (round16(d) + 4 + kFfnChunk + 4) * sizeof(float); }

}  // namespace encoder
}  // namespace dygnn
