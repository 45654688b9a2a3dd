// k_pooled_tail: the epilogue of the pooled DyGFormer inference kernels, once per launch instead of once per workgroup.
//
// k_dygformer_fused3<.., PL = 3> ends with the per-side token means of every (pair, side) as one dense row of the workspace:
// [800 means of gelu(h) | 208 means of the residual], row 2 * pair + side.  This kernel finishes them (DyGFormer.py:181-192, :457-460):
//     mean += W2 . mean_g + b2 ;   out = output_layer(mean)
// The in-kernel epilogue (fused3_forward.h) multiplies W2 by the 2 or 4 columns of its own workgroup: 12 or 14 of the MFMA's 16 columns
// are zeros, and every workgroup reads all 650 W2 fragments from global memory.  Here a wave owns 16 rows as the 16 B-operand columns,
// and the 8 waves of a workgroup (128 rows) share each fragment through LDS.
//
// The sums are those of the in-kernel epilogue chain for chain, so both forms give the same bits: per model-dim tile acc0 starts at b2 and
// takes the even k-chunks, acc1 the odd ones, a fragment's four MFMAs run .x .y .z .w, then mean += acc0 + acc1; the output layer likewise
// (acc0 starts at the bias).  A column of an MFMA does not depend on its neighbours, so which rows share a wave does not matter.
// The k-chunk loop is outermost with all 13 tiles' accumulators live (2 x 13 tiles = 104 VGPRs): between two MFMAs of one chain lie
// twelve of other chains, and a wave reads its rows once.  The 13 fragments of a k-chunk are one stage of the LDS ring (kStage, kNStage of
// fused3_device.h), brought in by LDS-DMA from w2frag as it is packed ([tile][chunk]).  The finished means are in accumulator layout,
// which is the B operand of the output layer: it runs from registers, two output tiles at a time.
#include "fused3_device.h"
#include "fused3_host.h"

namespace dygnn {
namespace v3 {

constexpr int kTailWaves = 8, kTailRows = 16 * kTailWaves;
constexpr int kW2Chunks = kHid / 16;          // 50 k-chunks of W2
static_assert(kStage == kNT && kW2Chunks % 2 == 0 && kKC % 2 == 1, "a ring stage is one k-chunk of all 13 tiles; the chunk loops are unrolled by parity");

struct TailArgs {
    const float* rows;            // [R][kPoolRow]
    const float* w2frag;          // [13 tiles][50 k-chunks] fragments
    const float* b2;              // [200]
    const float* outfrag;         // [ceil(Fn / 16) tiles][13 k-chunks] fragments
    const float* outb;            // [Fn]
    float *out_src, *out_dst;     // [R / 2][Fn]: row r belongs to pair r / 2, side r % 2
    int64_t R;
    int Fn;
};

__global__ __launch_bounds__(64 * kTailWaves, 2) void k_pooled_tail(const TailArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];      // the ring alone
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const int64_t r = (int64_t)blockIdx.x * kTailRows + 16 * wave + c;
    const bool row_ok = r < a.R;                                      // rows beyond the last: zero operands (row 0 is read instead), no store
    const float* rowp = a.rows + (row_ok ? r : 0) * kPoolRow + 4 * g;
    const float* w2l = a.w2frag + lane * 4;
    const float* ringl = lds + lane * 4;
    // k-chunk kc -> ring stage kc % kNStage: fragment (tile f, chunk kc) of the [tile][chunk] array, the 8 waves split the 13 tiles
    auto issue = [&](int kc) {
        if (kc < kW2Chunks) {
#pragma unroll
            for (int f = wave; f < kNT; f += kTailWaves) dma_frag(w2l + ((size_t)f * kW2Chunks + kc) * kFrag, ((kc % kNStage) * kStage + f) * kFrag);
        }
    };
#pragma unroll
    for (int s = 0; s < kNStage - 1; ++s) issue(s);

    f4 acc0[kNT], acc1[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const int n0 = 16 * i + 4 * g;
        acc0[i] = n0 < kD ? ldg4(a.b2 + n0) : zero4();
        acc1[i] = zero4();
    }
    f4 bm = ldg4(rowp);
    // One chunk: every wave's DMAs have landed and every wave is done with the chunk before (one barrier says both), so the stage that chunk
    // occupied takes the chunk kNStage - 1 ahead; the rows' next four values are requested before the MFMAs of these.
    // The empty asm pins this chunk's row values in front of those requests: hipcc does not see the wait above and places its own wait
    // for them at their first use — behind the new requests it would wait for those too (the DMA just issued included).
    auto chunk = [&](int kc, f4 (&acc)[kNT]) {
        __builtin_amdgcn_sched_barrier(0);          // the chunk before keeps its MFMAs in front of this wait (they touch no memory: nothing else holds them)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f4 b = row_ok ? bm : zero4();
        asm volatile("" : "+v"(b) : : "memory");
        issue(kc + kNStage - 1);
        if (kc + 1 < kW2Chunks) bm = ldg4(rowp + 16 * (kc + 1));
        __builtin_amdgcn_sched_barrier(0);          // ... and stay there: the scheduler otherwise sinks the load below the MFMAs
        f4 fr[kNT];
#pragma unroll
        for (int i = 0; i < kNT; ++i) fr[i] = lds4(ringl + ((kc % kNStage) * kStage + i) * kFrag);
        mma_group<kNT>(acc, fr, b);
    };
#pragma unroll 1
    for (int kc = 0; kc < kW2Chunks; kc += 2) {
        chunk(kc, acc0);
        chunk(kc + 1, acc1);
    }

    f4 mean[kKC];           // [208 model dims][16 rows] in accumulator layout: lane (c, g) holds dims 16 i + 4 g .. + 3 of row c
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const f4 res = ldg4(rowp + kHid + 16 * i);
        mean[i] = res + (acc0[i] + acc1[i]);
    }

    // output layer: out^T[j][row] = sum_k W[j][k] mean[row][k] + b[j], fragments straight from global memory (every wave needs all of them:
    // 8 waves read the same lines).  Two output tiles per step: their chains alternate, and 26 fragment loads are in flight at once.
    const int ntile = (a.Fn + 15) >> 4;
    const float* ol = a.outfrag + lane * 4;
    float* orow = ((r & 1) ? a.out_dst : a.out_src) + (r >> 1) * a.Fn;
#pragma unroll 1
    for (int jt = 0; jt < ntile; jt += 2) {
        const int jt1 = jt + 1 < ntile ? jt + 1 : jt;             // odd tile count: the last step computes its tile twice and stores it once
        f4 fa[kKC], fb[kKC];
#pragma unroll
        for (int kc = 0; kc < kKC; ++kc) {
            fa[kc] = ldg4(ol + ((size_t)jt * kKC + kc) * kFrag);
            fb[kc] = ldg4(ol + ((size_t)jt1 * kKC + kc) * kFrag);
        }
        const int ja = 16 * jt + 4 * g, jb = 16 * jt1 + 4 * g;
        f4 a0 = ja < a.Fn ? ldg4(a.outb + ja) : zero4(), a1 = zero4();
        f4 b0 = jb < a.Fn ? ldg4(a.outb + jb) : zero4(), b1 = zero4();
#pragma unroll
        for (int kc = 0; kc < kKC; ++kc) {
            const f4 m = mean[kc];
            if (kc & 1) {
                a1 = mfma(fa[kc].x, m.x, a1); b1 = mfma(fb[kc].x, m.x, b1); a1 = mfma(fa[kc].y, m.y, a1); b1 = mfma(fb[kc].y, m.y, b1);
                a1 = mfma(fa[kc].z, m.z, a1); b1 = mfma(fb[kc].z, m.z, b1); a1 = mfma(fa[kc].w, m.w, a1); b1 = mfma(fb[kc].w, m.w, b1);
            } else {
                a0 = mfma(fa[kc].x, m.x, a0); b0 = mfma(fb[kc].x, m.x, b0); a0 = mfma(fa[kc].y, m.y, a0); b0 = mfma(fb[kc].y, m.y, b0);
                a0 = mfma(fa[kc].z, m.z, a0); b0 = mfma(fb[kc].z, m.z, b0); a0 = mfma(fa[kc].w, m.w, a0); b0 = mfma(fb[kc].w, m.w, b0);
            }
        }
        if (row_ok && ja < a.Fn) *reinterpret_cast<f4*>(orow + ja) = a0 + a1;
        if (row_ok && jt1 != jt && jb < a.Fn) *reinterpret_cast<f4*>(orow + jb) = b0 + b1;
    }
}

}  // namespace v3

int pooled_tail(const float* rows, int64_t R, const float* w2frag, const float* b2, const float* outfrag, const float* outb, int Fn,
                float* out_src, float* out_dst, hipStream_t s) {
    using namespace v3;
    TailArgs a{rows, w2frag, b2, outfrag, outb, out_src, out_dst, R, Fn};
    hipLaunchKernelGGL(k_pooled_tail, dim3((unsigned)((R + kTailRows - 1) / kTailRows)), dim3(64 * kTailWaves), kRing * kFrag * sizeof(float), s, a);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace dygnn
