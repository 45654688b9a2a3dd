// The fused DyGFormer forward kernel k_dygformer_fused3 (design: fused3_device.h) and the host code that fills its arguments.  Included by
// dygformer_fused3.hip (the inference instances) and dygformer_fused3_train.hip (the training instances).
#pragma once
#include <type_traits>

#include "dropout.h"
#include "fused3_device.h"
#include "fused3_host.h"
#include "fused3_plan.h"

namespace dygnn {
namespace v3 {

struct LayerP {
    const float* b1;      // [800]; every other per-layer vector travels in the weight stream
};

struct Args {
    const int64_t* indptr; const int32_t* nbr; const int32_t* eid; const double* ts;
    const int64_t *src, *dst; const double* times;
    const int32_t* hist_len; const int64_t* end_pos; const CallDims* cd;
    const float *node_feat, *edge_feat, *time_w, *time_b, *lut;
    const float* stream; int nstages;
    const float* projw;           // projection fragments in step order [node | time | edge | cooc chunks][4 tiles]
    int proj_frags;               // projection fragments this launch walks (the whole sequence, less the channels of all-zero tables)
    int proj_skip0, proj_cut, proj_skip1;   // zero-table channels: walked fragment i is stored fragment i + proj_skip0 (+ proj_skip1 from i = proj_cut on)
    int slab_chunks;              // k-chunk slots per LDS HALF (a multiple of 4; two halves)
    int scr_floats;               // LDS floats reserved for the window arrays (the slab follows)
    int slab_in_ring;             // long windows (e.g. L = 2048): the slab borrows the weight ring, whose stream then opens after the prologue
    int tab_off, tab_slots, tab_bits;   // co-occurrence table per pair (LDS word offset, slots = 2^bits; 0: counts by scanning the rows)
    const float* bias_x;          // [208] projection biases in model-dim order
    const float* outfrag;         // output layer as fragments [ceil(Fn/16) tiles][13 k-chunks]
    const float* w2frag;          // pooled last layer (PL != 0): its W2 as fragments [13 n-tiles][50 k-chunks]
    const float* b2_last;         // ... and its second FFN bias [200]
    LayerP layer[DYGNN_MAX_LAYERS];
    const float *outT, *outb;     // output layer: transposed [200][Fn], bias [Fn]
    float *out_src, *out_dst;
    const int32_t* plan;          // packed form: the pair of every wave, [workgroup][8] (fused3_plan.h; workspace)
    float* pooled_rows;           // deferred epilogue (PL = 3): [2 B][kPoolRow] token means, row 2 * pair + side (workspace)
    float* tap_enc; float* tap_layer[DYGNN_MAX_LAYERS];
    unsigned long long* stamps;
    int64_t B, G, num_nodes;
    int64_t pair_stride;          // > 0 (two pairs per workgroup only): workgroup w holds pairs w and w + pair_stride — the positive and the
                                  // negative call of one edge: where their (src, t) agree the src side is projected once
    int Fn, Fe, Ft, P, L, NL, Tmax;
    int nchunk[4];
    const float *pt_node, *pt_edge;   // inference only: the channel's table already projected per (row, patch slot), [rows][P][kProjRow] (dygformer_proj_tables.hip);
                                  // its chunks have left the walk like a zero table's (nchunk = 0) and the token owner adds P rows instead.  nullptr: the MFMA path
    const float* qkv0c;           // inference only: layer 0's constant-channel operands of the prefix length in use, [38 tiles][64 lanes] (fused3_plan.h)
    int qkv0_skip;                // ... and the k-chunks of layer 0's Q/K/V products they stand for: 0 (none), 3 or 6
    const float* gelu_tab;        // inference only: the GELU table [4096][2] (gelu_table.h), staged into LDS once per FFN phase
    float qscale;
    train::TrainOut tr;           // training forward only (k_dygformer_fused3<.., true>): the dense activations the backward pass reads
};

// DyGFormer.py:458.  TAB (every inference instance): Phi from the LDS table at `tab` (fused3_device.h: gelu_table); the training instances keep
// the erf form, whose derivative their backward takes from hpre
template <bool TAB>
__device__ __forceinline__ void gelu_tiles(f4 (&t)[2], const float* tab) {
    if constexpr (TAB) {
        float v[8] = {t[0].x, t[0].y, t[0].z, t[0].w, t[1].x, t[1].y, t[1].z, t[1].w};
        gelu_table_n<8>(v, tab);
        t[0] = f4{v[0], v[1], v[2], v[3]}; t[1] = f4{v[4], v[5], v[6], v[7]};
    } else {
#pragma unroll
        for (int u = 0; u < 2; ++u) { t[u].x = gelu_erf(t[u].x); t[u].y = gelu_erf(t[u].y); t[u].z = gelu_erf(t[u].z); t[u].w = gelu_erf(t[u].w); }
    }
}
template <int TPW>
__device__ __forceinline__ void tap_store(const f4 (&x)[kNT], float* base, int64_t b, int Tmax, const TokOrder& o, int tt, int c, int g) {
    if (base == nullptr) return;
    const int tok = 16 * tt + c;
    if (tok >= o.T) return;
    auto put = [&](int row) {
#pragma unroll
        for (int i = 0; i < kNT; ++i) {
            const int n = 16 * i + 4 * g;
            if (n < kD) *reinterpret_cast<f4*>(base + ((size_t)b * Tmax + row) * kD + n) = x[i];
        }
    };
    // rows of the padded [B][Tmax] layout: source token k -> k, destination token k -> Tsf + k, the padding token -> every padding row
    if (tok != o.padtok) put(tok < o.Ts ? tok : o.Tsf + (tok - o.Ts));
    else {
        for (int row = o.Ts; row < o.Tsf; ++row) put(row);
        for (int row = o.Tsf + (o.padtok - o.Ts); row < o.Tf; ++row) put(row);
    }
}

// training forward: the 13 register tiles of a token-owner wave (rows 16 i + 4 g + r of token c) as dense row `row` of a [M][200] buffer
__device__ __forceinline__ void store_rows(float* base, int64_t row, const f4 (&x)[kNT], int g, bool valid) {
    if (!valid) return;
    float* p = base + row * kD + 4 * g;
#pragma unroll
    for (int i = 0; i < kNT; ++i)
        if (i < 12 || g < 2) *reinterpret_cast<f4*>(p + 16 * i) = x[i];
}
// x = xin + dropout(y + bias) (DyGFormer.py:456, :460), xin re-read from its dense rows, x also written to `out` (or not: nullptr).  Element
// (row, n = 16 i + 4 g + r) draws mask(site, row * 200 + n) (indices < 2^32: checked by the host).  One tile at a time — load, hash, add,
// store — so that no more than a tile's worth of temporaries is alive beside the two register sets.
__device__ __forceinline__ void residual_dropped(f4 (&x)[kNT], const float* xin, float* out, const f4 (&y)[kNT], const float* bias_lds, const train::Drop& dr,
                                                 uint32_t site, int64_t row, int g, bool valid) {
    const uint32_t sk = dr.site_key(site), e0 = (uint32_t)row * kD + 4 * g;
    const float* src = xin + row * kD + 4 * g;
    float* dst = out ? out + row * kD + 4 * g : nullptr;
    // (all thirteen row loads in flight first would expose one latency instead of thirteen, but next to the two live register sets it spills:
    //  measured 10 % slower)
    constexpr int RQ = 1;                                    // row tiles in flight ahead of the one being finished
    f4 rq[RQ];
#pragma unroll
    for (int u = 0; u < RQ; ++u) rq[u] = (valid && (u < 12 || g < 2)) ? ldg4(src + 16 * u) : zero4();
#pragma unroll
    for (int i = 0; i < kNT; ++i) {
        const bool on = valid && (i < 12 || g < 2);          // rows 200 .. 207 do not exist
        f4 v = rq[i % RQ];
        if (i + RQ < kNT) rq[i % RQ] = (valid && (i + RQ < 12 || g < 2)) ? ldg4(src + 16 * (i + RQ)) : zero4();
        const f4 bv = lds4(bias_lds + 16 * i);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += (y[i][r] + bv[r]) * dr.mask32(sk, e0 + 16 * i + r);      // rows >= 200: y and the bias are zero
        if (on && dst) *reinterpret_cast<f4*>(dst + 16 * i) = v;
        x[i] = v;
        __builtin_amdgcn_sched_barrier(0);
    }
}

// per-side sums over the 16 tokens of this wave's tile of the 13 register tiles: pool[wave][side][208].  row_sums8 takes the tiles two by
// two per side, and tile 12 as the pair (source form, destination form); the first lane of every bank stores its two words (fused3_plan.h)
// wsrc / wdst: how often this lane's token counts on either side (0, 1, or the padding token's multiplicity; x * 1 is x)
__device__ __forceinline__ void pool_sides(const f4 (&x)[kNT], float* pool, int wave, int lane, float wsrc, float wdst) {
    const bool st = pool_sum_stores(lane);
    float* ps = pool + wave * 2 * kDP + pool_sum_row(lane);
    float* pt = ps + 16 * pool_sum_tile(lane);
#pragma unroll
    for (int i = 0; i + 1 < kNT; i += 2) {
        const f2 zs = row_sums8(wsrc != 0.f ? x[i] * wsrc : zero4(), wsrc != 0.f ? x[i + 1] * wsrc : zero4());
        const f2 zd = row_sums8(wdst != 0.f ? x[i] * wdst : zero4(), wdst != 0.f ? x[i + 1] * wdst : zero4());
        if (st) {
            *reinterpret_cast<f2*>(pt + 16 * i) = zs;
            *reinterpret_cast<f2*>(pt + kDP + 16 * i) = zd;
        }
    }
    static_assert(kNT % 2 == 1, "the last tile is left over: its two sides are one block");
    const f2 z = row_sums8(wsrc != 0.f ? x[kNT - 1] * wsrc : zero4(), wdst != 0.f ? x[kNT - 1] * wdst : zero4());
    if (st) *reinterpret_cast<f2*>(ps + kDP * pool_sum_tile(lane) + 16 * (kNT - 1)) = z;
}
// pooled last layer: where its sums live in the K/V region (dead from the last out-projection on)
constexpr int kLdsGPool = 0;                        // [8 waves][2 sides][800] per-wave sums of gelu(h) over the wave's tokens = the K region
constexpr int kLdsPool = kLdsV;                     // [8 waves][2 sides][208] per-wave sums of the residual
constexpr int kLdsMean = kLdsPool + 8 * 2 * kDP;    // [4 columns][208] per-side token means, column = 2 * pair + side
constexpr int kLdsMeanG = kLdsMean + 4 * kDP;       // [4 columns][800] per-side token means of gelu(h)
static_assert(8 * 2 * kHid <= kLdsV && kLdsMeanG + 4 * kHid <= kLdsRing, "the pooled sums fit the K/V region");
// the GELU table (fused3_device.h) during the pooled layer's FFN loop: gpool (K region) and pool end in front of it; mean and mean_g, which it
// lies over, are written after the loop and the barrier behind it
static_assert(kLdsGPool + 8 * 2 * kHid <= kLdsGelu && kLdsPool + 8 * 2 * kDP <= kLdsGelu && kLdsMean >= kLdsGelu, "the GELU table and the pooled sums");

// ================================================================================================
// TR = false: inference.  TR = true: the training forward — dropout at the reference's four sites per layer and every
// activation the backward pass reads written to HBM as dense rows (a.tr); the residual stream is re-read from those rows after the
// attention and the FFN block instead of being kept in registers next to the separate accumulators the dropout needs.
// NW = waves per workgroup: 8 (two pairs of <= 64 tokens, or one of <= 128), or 4 = ONE pair of <= 64 tokens per workgroup, for calls of at most 256
// pairs (the reference's own 200-pair call: 100 eight-wave workgroups would leave 156 CUs idle and run two waves per SIMD on the rest; 200
// four-wave workgroups give every wave a matrix pipe of its own)
// PL (inference only): the LAST layer's second FFN product is taken after the per-side token mean instead of per token — nothing after
// that layer is non-linear, so  mean_tok(x_L) = mean_tok(x1) + W2 . mean_tok(gelu(h)) + b2  (DyGFormer.py:181-192, :457-460):
//   1  the product path: the last layer's FFN steps run W1 and GELU only and leave per-wave, per-side sums of gelu(h) in the K region; the
//      stream (its own: the last layer carries W1 blocks only) ends there, and the epilogue multiplies the 4 (pair, side) means by W2
//   2  a call whose taps ask for the last layer's per-token output: the same sums and the same epilogue — the embeddings are those of
//      PL = 1 bit for bit — and, for the tap alone, the per-token W2 product from the full stream
//   3  the deferred form of 1 for large launches: the kernel ends with the token means, written as dense rows (Args.pooled_rows) instead of
//      LDS columns; k_pooled_tail (dygformer_pooled_tail.hip) runs the W2 product and the output layer once per launch, same chains
// PK (inference, deferred tail only): the PACKED form.  A workgroup's eight waves hold up to eight pairs of 1 .. 4 token tiles each, as the
// plan kernel (dygformer_pack_plan.hip) laid them out: every wave reads its (pair, first wave, tiles) from Args.plan.  The arithmetic per
// pair is that of the unpacked kernels, chain for chain: a pair's bits do not depend on the form that computed it.
template <int TPW, bool TR, int NW, int PL, bool PK>
__device__ __forceinline__ void fused3_body(const Args& a) {
    static_assert(!(TR && PL != 0), "the training forward keeps the per-token form: its backward reads the per-token activations");
    static_assert(!PK || (TPW == 4 && NW == 8 && PL == 3 && !TR), "the packed form: eight waves, pairs of <= 64 tokens, deferred tail");
    constexpr int NP = PK ? 8 : NW / TPW;        // pairs per workgroup (packed: at most)
    constexpr int NTHR = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, g = lane >> 4;
    const bool paired = !PK && NP == 2 && a.pair_stride > 0;
    int pi, tt, nwv, PT;                         // pair slot, token tile, waves of this pair, threads of this pair
    int64_t b;
    bool pair_ok;
    if constexpr (PK) {
        // the eight entries of this workgroup (fused3_plan.h): this wave's pair, its first wave = the first entry that names it, its tiles = how many do
        const int32_t* e = a.plan + (size_t)blockIdx.x * 8;
        int pr = -1, any = -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int id = __builtin_amdgcn_readfirstlane(e[j]);
            pr = j == wave ? id : pr;
            any = id >= 0 ? id : any;
        }
        if (any < 0) return;                     // the grid is the unpacked one: a workgroup beyond the plan's count
        int first = 8, cnt = 0;
#pragma unroll
        for (int j = 7; j >= 0; --j) {
            const bool same = __builtin_amdgcn_readfirstlane(e[j]) == pr;
            first = same ? j : first;
            cnt += same ? 1 : 0;
        }
        pair_ok = pr >= 0;
        b = pair_ok ? pr : 0;
        pi = pair_ok ? first : wave;             // the pair's first wave names its slot
        nwv = pair_ok ? cnt : 1;
        tt = wave - pi;
        PT = 64 * nwv;
    } else {
        pi = wave / TPW; tt = wave % TPW; nwv = TPW; PT = 64 * NW / NP;
        b = paired ? (int64_t)blockIdx.x + pi * a.pair_stride : (int64_t)blockIdx.x * NP + pi;
        pair_ok = paired ? blockIdx.x < a.pair_stride && b < a.B : b < a.B;
    }
    const int wave0 = PK ? pi : pi * TPW;        // this pair's first wave
    const int ptid = tid - 64 * wave0;

    TDECL;
    CallDims cd{};
    if (pair_ok) cd = a.cd[b / a.G];
    const int Ss = cd.S_s, Sd = cd.S_d, Tsf = cd.T_s, Tf = cd.T;
    // Inference computes every DISTINCT token once.  A patch made of padding positions only has a constant encoder input, so all such
    // tokens of a pair stay identical through every layer: the pair runs its real source tokens, its real destination tokens and ONE
    // padding token (order: source, destination, padding), whose softmax weight as a key and whose share of the per-side means count
    // it m_s + m_d and m_s / m_d times.  Ts, T: source tokens and tokens of the compact order; Tsf, Tf: of the padded call (divisors, taps).
    int Ts = Tsf, T = Tf, ms = 0, md = 0;
    if constexpr (!TR) {
        if (pair_ok) {
            const PairTokens pk = pair_tokens(a.hist_len[b], a.hist_len[a.B + b], a.L, a.P, Tsf, Tf - Tsf);
            Ts = pk.Rs; T = pk.Tc; ms = pk.ms; md = pk.md;
        }
    }
    const int padtok = ms + md > 0 ? T - 1 : -1; // the padding token (compact order), or none
    const int SsA = (Ss + 3) & ~3, SdA = (Sd + 3) & ~3, SA = SsA + SdA;
    const bool active = pair_ok && 16 * tt < T;  // wave-uniform: this token tile holds tokens
    const int tokbase = 16 * wave0;              // this pair's first K/V row
    const TokOrder ord{T, Ts, Tf, Tsf, padtok};
    const float padw = (float)(ms + md);
    // how often token `tok` of the compact order counts in the source / destination mean
    auto side_weights = [&](int tok, float& wsrc, float& wdst) {
        const bool pad = tok == padtok;
        wsrc = pad ? (float)ms : tok < Ts ? 1.f : 0.f;
        wdst = pad ? (float)md : (tok >= Ts && tok < T) ? 1.f : 0.f;
    };
    // f4 (caller-side fusion, train_link_prediction.py:166 / evaluate_models_utils.py:62-63): the second pair of the workgroup is the
    // NEGATIVE call of the first pair's edge when it has the same source, the same time and the same padded source length.  Its token
    // tiles that hold source tokens only then take the node / edge / time rows of the residual stream from the first pair's same tile
    // instead of gathering and projecting them again (rows of one channel receive non-zero terms from that channel only, so the bits are
    // those of a separate call); the co-occurrence rows and the destination side are its own.  Anything else: the plain path.
    bool src_shared = false;
    if (!PK && NP == 2) {
        if (paired && pi == 1 && pair_ok) {
            const int64_t b0 = blockIdx.x;
            const CallDims cd0 = a.cd[b0 / a.G];
            // (inference: Ts counts the REAL source tokens; an equal window length and an equal padded length make both pairs' compact source sides equal)
            src_shared = a.src[b0] == a.src[b] && __double_as_longlong(a.times[b0]) == __double_as_longlong(a.times[b]) && cd0.S_s == Ss &&
                         (TR || a.hist_len[b0] == a.hist_len[b]) && 16 * (tt + 1) <= Ts;
        }
        src_shared = __builtin_amdgcn_readfirstlane((int)src_shared) != 0;
    }
    const bool donor = !PK && NP == 2 && paired && pi == 0 && 16 * (tt + 1) <= Ts;     // first-pair tiles a shared tile may copy from (checked by the taker)

    // ---- weights start moving at once: the first four stages of the layer stream into the ring, the first two halves of
    // projection fragments into the K/V region behind the window arrays (all of it lands during the window phase)
    WStream ws;
    if (!a.slab_in_ring) ws.open(a.stream, kLdsRing, lane, wave, a.nstages, NW);
    const float* ringl = lds + kLdsRing + lane * 4;
    // projection fragments: two LDS halves of `slab_chunks` k-chunk slots each (4 fragments per slot), refilled by LDS-DMA one half
    // ahead of the consumer (half q of the slot sequence lives in buffer q & 1)
    const int slab_off = a.slab_in_ring ? kLdsRing : a.scr_floats;
    const float* slabl = lds + slab_off + lane * 4;
    const int hc = a.slab_chunks;
    const int half_frags = 4 * hc;
    auto load_half = [&](int q) {
        const int f0 = q * half_frags;
        const int n = a.proj_frags - f0 < half_frags ? a.proj_frags - f0 : half_frags;      // <= 0 beyond the last half
        // a channel whose table is all zero (Args.proj_skip*) is not part of the walked sequence: its stored fragments are stepped over here
        for (int f = wave; f < n; f += NW) {
            const int sf = f0 + f + a.proj_skip0 + (f0 + f >= a.proj_cut ? a.proj_skip1 : 0);
            dma_frag(a.projw + (size_t)sf * kFrag + lane * 4, slab_off + ((q & 1) * half_frags + f) * kFrag);
        }
    };
    load_half(0);
    load_half(1);
    float* tws = lds + kLdsMisc + kMiscFloats;      // time-encoder w | b
    for (int i = tid; i < 2 * a.Ft; i += NTHR) tws[i] = i < a.Ft ? a.time_w[i] : a.time_b[i - a.Ft];

    // ---- windows (pad_sequences, DyGFormer.py:228-245): per-pair arrays in the (still unused) K/V region.
    // src positions at [0, Ss), dst positions at [SsA, SsA + Sd); alignment gaps hold id -1 (matches nothing).
    int32_t* ids = reinterpret_cast<int32_t*>(lds) + pi * (a.scr_floats / NP);
    int32_t* eids = ids + SA;
    float* dts = reinterpret_cast<float*>(eids + SA);
    int32_t* c0 = reinterpret_cast<int32_t*>(dts + SA);
    int32_t* c1 = c0 + SA;
    if (pair_ok) {
        const double tq = a.times[b];
        for (int p = ptid; p < SA; p += PT) {
            const bool is_dst = p >= SsA;
            const int j = is_dst ? p - SsA : p;
            int32_t id = -1, e = 0;
            float dt = 0.f;
            if (j < (is_dst ? Sd : Ss)) {
                const int64_t q = is_dst ? a.B + b : b;
                const int32_t len = a.hist_len[q];
                const int32_t m = len < a.L - 1 ? len : a.L - 1;
                float tn = 0.f;
                id = 0;
                if (j == 0) {
                    const int64_t qid = is_dst ? a.dst[b] : a.src[b];
                    id = qid < 0 || qid >= a.num_nodes ? 0 : (int32_t)qid;      // a bad query id is the padding node, as in sampler.hip (never a fault)
                    tn = (float)tq;
                } else if (j <= m) {
                    const int64_t pos = a.end_pos[q] - m + (j - 1);
                    id = a.nbr[pos]; e = a.eid[pos]; tn = (float)a.ts[pos];
                }
                dt = (float)(tq - (double)tn);                      // DyGFormer.py:263
            }
            ids[p] = id; eids[p] = e; dts[p] = dt;
        }
    }
    // long windows: an open-addressing table [keys | counts] per pair behind the projection halves (a.tab_slots > 0), cleared here
    int32_t* tkeys = reinterpret_cast<int32_t*>(lds) + a.tab_off + pi * 2 * a.tab_slots;
    int32_t* tcnts = tkeys + a.tab_slots;
    for (int i = ptid; i < a.tab_slots; i += PT) { tkeys[i] = -2; tcnts[i] = 0; }
    __syncthreads();
    // ---- co-occurrence counts (DyGFormer.py:337-393)
    if (a.tab_slots > 0) {
        // Windows of hundreds of positions (L = 512: 1,024 positions per pair, a million comparisons by the scan below = 5 % of the kernel):
        // every position inserts its id into the table (linear probing; the slot's count word holds the source-side count in its low
        // half, the destination-side count in its high half), one barrier, every position reads its id's slot.  Exact integers.
        const uint32_t mask = (uint32_t)a.tab_slots - 1;
        const int shift = 32 - a.tab_bits;
        if (pair_ok) {
            for (int p = ptid; p < SA; p += PT) {
                const int32_t v = ids[p];
                if (v <= 0) continue;
                uint32_t sl = ((uint32_t)v * 2654435761u) >> shift;
                for (int it = 0; it < a.tab_slots; ++it, sl = (sl + 1) & mask) {
                    const int32_t old = atomicCAS(&tkeys[sl], -2, v);
                    if (old == -2 || old == v) { atomicAdd(&tcnts[sl], p >= SsA ? 0x10000 : 1); break; }
                }
            }
        }
        __syncthreads();
        if (pair_ok) {
            for (int p = ptid; p < SA; p += PT) {
                const int32_t v = ids[p];
                int32_t cs = 0, cdn = 0;
                if (v > 0) {
                    uint32_t sl = ((uint32_t)v * 2654435761u) >> shift;
                    for (int it = 0; it < a.tab_slots && tkeys[sl] != v; ++it) sl = (sl + 1) & mask;
                    const int32_t w = tcnts[sl];
                    cs = w & 0xffff; cdn = w >> 16;
                }
                c0[p] = cs; c1[p] = cdn;
            }
        }
    } else if (pair_ok) {
        // one thread per position, 4 ids per broadcast LDS read
        for (int p = ptid; p < SA; p += PT) {
            const int32_t v = ids[p];
            int32_t cs = 0, cdn = 0;
            for (int q = 0; q < SsA; q += 4) {
                const i4 w = *reinterpret_cast<const i4*>(ids + q);
                cs += (w.x == v) + (w.y == v) + (w.z == v) + (w.w == v);
            }
            for (int q = SsA; q < SA; q += 4) {
                const i4 w = *reinterpret_cast<const i4*>(ids + q);
                cdn += (w.x == v) + (w.y == v) + (w.z == v) + (w.w == v);
            }
            if (v <= 0) { cs = 0; cdn = 0; }       // padding node 0 (DyGFormer.py:389-391) and alignment gaps
            c0[p] = cs; c1[p] = cdn;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's share of the first two projection halves and of the first ring stages has landed
    __syncthreads();

    TACC(T_WIN);
    // ---- resident residual stream X^T: 13 tiles (rows 16i+4g+r) x token c of tile tt
    f4 x[kNT];
#pragma unroll
    for (int i = 0; i < kNT; ++i) x[i] = ldg4(a.bias_x + 16 * i + 4 * g);

    // ---- patch projection (DyGFormer.py:148-157): channel ch writes model rows 50ch..50ch+49 = tiles (50ch)/16 .. +3.
    // One step = one 16-wide k-chunk x 4 tiles; the fragments of `slab_chunks` steps sit in an LDS half (loaded by LDS-DMA one half
    // ahead, all waves use the same ones), so inside a half nothing synchronises and the B operand — gathered straight from the feature
    // tables, (pp, f) = (patch position, feature) of this lane's k advanced incrementally — runs four chunks ahead.  Channel order
    // node, time, edge, cooc: the edge gathers are issued before the time channel computes its cosines.
    {
        const int tok = 16 * tt + c;
        const bool tv = tok < T;
        // the padding token reads the first all-padding patch of the pair: on the source side if it has one (m_s > 0), else on the destination side,
        // where it follows the last real destination token as in the padded order
        const int pos0 = tv ? (tok < Ts ? tok * a.P : (tok == padtok && ms > 0) ? Ts * a.P : SsA + (tok - Ts) * a.P) : 0;
        const int P = a.P;
        // Round 3: the whole phase is written WITHOUT branches around loads.  hipcc counts the loads in flight (s_waitcnt vmcnt / lgkmcnt (N))
        // only while every path through the code issues the same loads: with the earlier form — gathers skipped for absent rows, the
        // fragments of a step read "if fresh", cursor rows re-read on a wrap — every step waited `vmcnt(1)` for a gather issued one step
        // before (queue depth 8 on paper) and `lgkmcnt(3)` for the fragment reads of the NEXT step just issued: the matrix pipe ran at 50 %
        // (profiles/r03_lastfm_phase.txt).  Now absent rows are read from a zero word, cursors advance by selects with the next position's
        // row read one step ahead, and the step count of every loop body is a template parameter.
        constexpr int GS = 4;              // steps per group = gathered operands in flight per lane
        static_assert(GS == 4, "the counted wait below is written as vmcnt(4)");
        using std::integral_constant;
        // ---- slot walk.  The channels' k-chunks occupy consecutive slots of the fragment sequence, every channel padded to whole groups
        // of GS slots (build_proj); a half holds hc (a multiple of GS) slots, so a group never straddles a half.
        int pj_half = 0, pj_slot = 0, pj_next = 2, pj_young = 0;      // pj_young: gathers this wave issued since its last LDS-DMA
        auto frag_ptr = [&]() -> const float* { return slabl + (size_t)((pj_half * hc + pj_slot) * 4) * kFrag; };
        // A group is done (its last fragment read is issued).  At the end of a half: this wave's DMAs of the NEXT half have landed — they are
        // older than its last GS gathers, vmcnt retires in issue order, so `vmcnt(GS)` proves it without waiting for the gathers in flight —
        // its own reads of the finished half are complete, one barrier, and the finished half's buffer is refilled two halves ahead.
        auto end_group = [&](bool counted) {
            pj_slot += GS;
            if (pj_slot == hc) {
                if (counted && pj_young >= GS) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_waitcnt(0xc07f);          // lgkmcnt(0)
                __syncthreads();
                load_half(pj_next++);
                pj_young = 0; pj_half ^= 1; pj_slot = 0;
            }
        };
        auto run_idle = [&](int n) { for (int i = 0; i < (n + GS - 1) / GS; ++i) end_group(false); };     // a wave without work in this channel keeps the barriers
        // fragments of one step: 4 tiles
        auto read_frags = [&](f4 (&dst)[4], const float* fr) {
#pragma unroll
            for (int v = 0; v < 4; ++v) dst[v] = lds4(fr + v * kFrag);
        };
        // fragment reads of step u of an NS-step group: the next step's, or — on the last step of a full group, after the half protocol —
        // the first step's of the NEXT group into fa[0] (a channel's last group reads ahead in vain: the next channel starts FRESH)
        auto frags_ahead = [&](auto NSc, int u, const float* fr, f4 (&fa)[2][4], bool counted) {
            constexpr int NS = decltype(NSc)::value;
            if (u + 1 < NS) read_frags(fa[(u + 1) & 1], fr + (size_t)(u + 1) * 4 * kFrag);
            else {
                end_group(counted);
                if (NS == GS) read_frags(fa[0], frag_ptr());
            }
        };

        // ---- gathered channels (node, edge features): (pp, f) = patch position and feature of this lane's k, row = the table row of that
        // position, rown = the row of position pp + 1 (read from LDS one step ahead, every step: no branch)
        struct Cursor { int pp, f, row, rown; };
        auto row_at = [&](const int32_t* idx, int pp) -> int {
            const int32_t r = idx[pos0 + (pp < P ? pp : P - 1)];
            return (tv && pp < P) ? (r < 0 ? 0 : r) : -1;
        };
        auto cur_init = [&](Cursor& cu, const int32_t* idx) { cu.pp = 0; cu.f = 4 * g; cu.row = row_at(idx, 0); cu.rown = row_at(idx, 1); };
        auto gather = [&](const float* table, int F, Cursor& cu, const int32_t* idx) -> f4 {
            // DyGFormer.py:259-261; an absent position reads the zero word.  The select is arithmetic on the address (a ?: on the pointers
            // comes back as a branch around the address computation, which would end the scheduling region of the step)
            const uintptr_t pz = reinterpret_cast<uintptr_t>(g_zero16);
            const uintptr_t pt = reinterpret_cast<uintptr_t>(table + (size_t)(cu.row >= 0 ? cu.row : 0) * F + cu.f);
            const f4 v = ldg4(reinterpret_cast<const float*>(pz + ((pt - pz) & (cu.row >= 0 ? ~uintptr_t(0) : uintptr_t(0)))));
            ++pj_young;
            cu.f += 16;
            const bool wrap = cu.f >= F;
            cu.f = wrap ? cu.f - F : cu.f;
            cu.pp += wrap ? 1 : 0;
            cu.row = wrap ? cu.rown : cu.row;
            cu.rown = row_at(idx, cu.pp + 1);
            return v;
        };
        auto prefill = [&](f4 (&bq)[GS], Cursor& cu, const float* table, const int32_t* idx, int F) {
            cur_init(cu, idx);
#pragma unroll
            for (int u = 0; u < GS; ++u) bq[u] = gather(table, F, cu, idx);
        };
        auto g_group = [&](auto L0c, auto NSc, auto FRESHc, f4 (&fa)[2][4], f4 (&bq)[GS], Cursor& cu, const float* table, const int32_t* idx, int F) {
            constexpr int L0 = decltype(L0c)::value, NS = decltype(NSc)::value;
            const float* fr = frag_ptr();
            if (decltype(FRESHc)::value) read_frags(fa[0], fr);
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const f4 bcur = bq[u];
                bq[u] = gather(table, F, cu, idx);             // chunk + GS (zeros beyond the patch)
                frags_ahead(NSc, u, fr, fa, true);
                // operand loads of later steps stay issued ABOVE this step's MFMAs.  (Measured and not kept: the gather and the cursor arithmetic
                // scheduled into the shadow of the step's own MFMAs by sched_group_barrier, as the time channel does with its cosines —
                // node / edge channel 126 k -> 138 k cycles per 86 chunks at L = 512: the address arithmetic is short enough for the SIMD's
                // other wave to cover, and spreading it stretches the wave's MFMA block.)
                __builtin_amdgcn_sched_barrier(0);
                mma_group<4>(&x[L0], fa[u & 1], bcur);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto run_gathered = [&](auto L0c, f4 (&bq)[GS], Cursor& cu, int n, const float* table, const int32_t* idx, int F) {
            f4 fa[2][4];
            const int ng = n / GS, rem = n % GS;
            if (ng > 0) {
                g_group(L0c, integral_constant<int, GS>{}, std::true_type{}, fa, bq, cu, table, idx, F);
                for (int i = 1; i < ng; ++i) g_group(L0c, integral_constant<int, GS>{}, std::false_type{}, fa, bq, cu, table, idx, F);
            }
            if (rem == 1) g_group(L0c, integral_constant<int, 1>{}, std::true_type{}, fa, bq, cu, table, idx, F);
            else if (rem == 2) g_group(L0c, integral_constant<int, 2>{}, std::true_type{}, fa, bq, cu, table, idx, F);
            else if (rem == 3) g_group(L0c, integral_constant<int, 3>{}, std::true_type{}, fa, bq, cu, table, idx, F);
        };

        // ---- time encoding (modules.py:27-39, DyGFormer.py:263-266): the cursor runs one chunk ahead of the MFMAs; (valid, dt) of the next patch
        // position and the next chunk's w / b are read one step ahead like the gather rows.  What the channel costs beyond its MFMAs is the
        // instruction count of the cosines: on this chip a VALU instruction does not issue in the shadow of an fp32 MFMA — not of the same wave,
        // not of the SIMD's other wave (tools/coissue_ubench.hip: 16 MFMAs + 64 v_fma_f32 take the SUM of their times, 1 or 2 waves per SIMD) —
        // so interleaving them (sched_group_barrier) bought nothing; the cosines are evaluated two at a time on packed fp32 instructions
        struct TCur { int pp, f; float dt; bool ok; int32_t idn; float dn; f4 w, bb; };      // idn, dn: id and dt of position pp + 1 as read from LDS; w, bb: encoder weights / biases of features f .. f+3
        auto tpos_at = [&](int pp, float& dt, bool& ok) {
            const int q = pos0 + (pp < P ? pp : P - 1);
            const int32_t id = ids[q];
            const float d = dts[q];
            ok = tv && pp < P && id > 0;                                                             // DyGFormer.py:266
            dt = ok ? d : 0.f;
        };
        // the reads of the next position are issued here and USED by the next call: nothing in a step waits for an LDS read of its own
        auto t_advance = [&](TCur& tc) {
            tc.f += 16;
            const bool wrap = tc.f >= a.Ft;
            tc.f = wrap ? tc.f - a.Ft : tc.f;
            const bool okn = tv && tc.pp + 1 < P && tc.idn > 0;
            tc.dt = wrap ? (okn ? tc.dn : 0.f) : tc.dt;
            tc.ok = wrap ? okn : tc.ok;
            tc.pp += wrap ? 1 : 0;
            const int q = pos0 + (tc.pp + 1 < P ? tc.pp + 1 : P - 1);
            tc.idn = ids[q];
            tc.dn = dts[q];
            tc.w = lds4(tws + tc.f);
            tc.bb = lds4(tws + a.Ft + tc.f);
        };
        auto t_finish = [&](const bool ok, const f4 arg, f4 cs) -> f4 {      // rare: an argument beyond the fast cosine's range takes libm's
            if (!(fabsf(arg.x) <= 3.0e7f && fabsf(arg.y) <= 3.0e7f && fabsf(arg.z) <= 3.0e7f && fabsf(arg.w) <= 3.0e7f)) {
                cs.x = timeenc::cos_time_select(arg.x); cs.y = timeenc::cos_time_select(arg.y); cs.z = timeenc::cos_time_select(arg.z); cs.w = timeenc::cos_time_select(arg.w);
            }
            return ok ? cs : zero4();
        };
        auto t_group = [&](auto L0c, auto NSc, auto FRESHc, f4 (&fa)[2][4], f4& bnx, TCur& tc) {
            constexpr int L0 = decltype(L0c)::value, NS = decltype(NSc)::value;
            const float* fr = frag_ptr();
            if (decltype(FRESHc)::value) read_frags(fa[0], fr);
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const f4 bcur = bnx;
                const f4 w = tc.w, bb = tc.bb;                  // of the next chunk (read during the previous step)
                frags_ahead(NSc, u, fr, fa, false);
                __builtin_amdgcn_sched_barrier(0);
                const f2 dt2 = {tc.dt, tc.dt};
                const f2 a01 = pk_fma(dt2, f2{w.x, w.y}, f2{bb.x, bb.y}), a23 = pk_fma(dt2, f2{w.z, w.w}, f2{bb.z, bb.w});
                const f2 c01 = timeenc::cos_fast2(a01), c23 = timeenc::cos_fast2(a23);
                const f4 arg = {a01.x, a01.y, a23.x, a23.y}, cs = {c01.x, c01.y, c23.x, c23.y};
                const bool okc = tc.ok;
                t_advance(tc);                                 // the cursor arithmetic and the next position's (valid, dt) reads: same region
                mma_group<4>(&x[L0], fa[u & 1], bcur);
                __builtin_amdgcn_sched_barrier(0);
                bnx = t_finish(okc, arg, cs);
            }
        };
        auto run_time = [&](auto L0c, int n) {
            f4 fa[2][4];
            TCur tc{0, 4 * g, 0.f, false, 0, 0.f, zero4(), zero4()};
            tpos_at(0, tc.dt, tc.ok);
            { const int q = pos0 + (1 < P ? 1 : P - 1); tc.idn = ids[q]; tc.dn = dts[q]; }
            f4 bnx;
            {   // chunk 0 (not overlapped)
                const f4 w = lds4(tws + tc.f), bb = lds4(tws + a.Ft + tc.f);
                f4 arg;
                arg.x = fmaf(tc.dt, w.x, bb.x); arg.y = fmaf(tc.dt, w.y, bb.y); arg.z = fmaf(tc.dt, w.z, bb.z); arg.w = fmaf(tc.dt, w.w, bb.w);
                f4 cs;
                cs.x = timeenc::cos_fast(arg.x); cs.y = timeenc::cos_fast(arg.y); cs.z = timeenc::cos_fast(arg.z); cs.w = timeenc::cos_fast(arg.w);
                bnx = t_finish(tc.ok, arg, cs);
                t_advance(tc);
            }
            const int ng = n / GS, rem = n % GS;
            if (ng > 0) {
                t_group(L0c, integral_constant<int, GS>{}, std::true_type{}, fa, bnx, tc);
                for (int i = 1; i < ng; ++i) t_group(L0c, integral_constant<int, GS>{}, std::false_type{}, fa, bnx, tc);
            }
            if (rem == 1) t_group(L0c, integral_constant<int, 1>{}, std::true_type{}, fa, bnx, tc);
            else if (rem == 2) t_group(L0c, integral_constant<int, 2>{}, std::true_type{}, fa, bnx, tc);
            else if (rem == 3) t_group(L0c, integral_constant<int, 3>{}, std::true_type{}, fa, bnx, tc);
        };

        // ---- co-occurrence features (DyGFormer.py:395-415): k = 50*pp + j is not 4-aligned per position, so every element finds its own
        // (pp, j); k/50 by multiply-shift (exact for k < 12000).  The two LUT rows' values of a chunk are loaded two steps ahead (L2 round trips).
        struct CQ { f4 u, v; };
        int kco = 4 * g;
        auto cooc_issue = [&]() -> CQ {
            CQ r;
#pragma unroll
            for (int t = 0; t < 4; t += 2) {             // k and 50 are even: the pair (k, k + 1) lies inside one position, its LUT address is 8-byte aligned
                const int k = kco + t;
                const int pp = (k * 1311) >> 16;
                const bool ok = tv && pp < P;
                const int q = pos0 + (pp < P ? pp : P - 1);
                const int j = k - pp * kC;
                const uintptr_t pz = reinterpret_cast<uintptr_t>(g_zero16), m = ok ? ~uintptr_t(0) : uintptr_t(0);
                const uintptr_t p0 = reinterpret_cast<uintptr_t>(a.lut + (size_t)c0[q] * kC + j), p1 = reinterpret_cast<uintptr_t>(a.lut + (size_t)c1[q] * kC + j);
                const f2 v0 = *reinterpret_cast<const f2*>(pz + ((p0 - pz) & m));                   // DyGFormer.py:409-411
                const f2 v1 = *reinterpret_cast<const f2*>(pz + ((p1 - pz) & m));
                r.u[t] = v0.x; r.u[t + 1] = v0.y; r.v[t] = v1.x; r.v[t + 1] = v1.y;
            }
            kco += 16;
            return r;
        };
        auto c_group = [&](auto L0c, auto NSc, auto FRESHc, f4 (&fa)[2][4], CQ (&cq)[2]) {
            constexpr int L0 = decltype(L0c)::value, NS = decltype(NSc)::value;
            const float* fr = frag_ptr();
            if (decltype(FRESHc)::value) read_frags(fa[0], fr);
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                const f4 bcur = cq[u & 1].u + cq[u & 1].v;
                cq[u & 1] = cooc_issue();                       // chunk + 2
                frags_ahead(NSc, u, fr, fa, false);
                __builtin_amdgcn_sched_barrier(0);
                mma_group<4>(&x[L0], fa[u & 1], bcur);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto run_cooc = [&](auto L0c, int n) {
            f4 fa[2][4];
            CQ cq[2];
            cq[0] = cooc_issue();
            cq[1] = cooc_issue();
            const int ng = n / GS, rem = n % GS;
            if (ng > 0) {
                c_group(L0c, integral_constant<int, GS>{}, std::true_type{}, fa, cq);
                for (int i = 1; i < ng; ++i) c_group(L0c, integral_constant<int, GS>{}, std::false_type{}, fa, cq);
            }
            if (rem == 1) c_group(L0c, integral_constant<int, 1>{}, std::true_type{}, fa, cq);
            else if (rem == 2) c_group(L0c, integral_constant<int, 2>{}, std::true_type{}, fa, cq);
            else if (rem == 3) c_group(L0c, integral_constant<int, 3>{}, std::true_type{}, fa, cq);
        };

        // ---- projected tables (Args.pt_node / pt_edge): W[:, slot p] . table[row] was computed once per (row, slot) when the weights were
        // packed, so the channel is P row additions per token: x = ((bias + PT[row_0][0]) + PT[row_1][1]) + ..., one fixed chain per element in
        // every instance.  A (row, slot) segment holds the channel's four x tiles (zero outside its 50 rows): lane (c, g) reads its accumulator
        // registers as four float4s.  Absent positions read the zero word, by the address select of gather().
        auto pt_load = [&](f4 (&q)[4], const float* pt, const int32_t* idx, int p) {
            const int pc = p < P ? p : P - 1;
            const int32_t r = idx[pos0 + pc];
            const uintptr_t pz = reinterpret_cast<uintptr_t>(g_zero16), m = (tv && p < P) ? ~uintptr_t(0) : uintptr_t(0);
            const uintptr_t pr = reinterpret_cast<uintptr_t>(pt + ((size_t)(r < 0 ? 0 : r) * P + pc) * kProjRow + 4 * g);
#pragma unroll
            for (int v = 0; v < 4; ++v) q[v] = ldg4(reinterpret_cast<const float*>(pz + ((pr + 64 * v - pz) & m)));
        };
        auto pt_add = [&](auto L0c, const f4 (&q)[4]) {
            constexpr int L0 = decltype(L0c)::value;
#pragma unroll
            for (int v = 0; v < 4; ++v) x[L0 + v] = x[L0 + v] + q[v];
        };

        // Channel order node, time, edge, cooc: the edge gathers are issued before the time channel computes its cosines.  A wave whose
        // tile is empty, or a source tile shared with the first pair (f4), only keeps the barriers of the channel.  A gathered channel
        // whose table the caller declared all zero has nchunk = 0 (and no slots in the walked sequence): no gathers, no MFMAs, no
        // barriers — its rows of x keep the projection bias they started from, which is what adding w . 0 leaves of them.
        const bool work = active && !src_shared;
        const bool work_n = work && a.nchunk[0] > 0, work_e = work && a.nchunk[1] > 0;
        f4 bq[GS];
        Cursor cu;
        if (work_n) prefill(bq, cu, a.node_feat, ids, a.Fn);
        TACC(T_PROJ);
        if (work_n) run_gathered(integral_constant<int, 0>{}, bq, cu, a.nchunk[0], a.node_feat, ids, a.Fn); else run_idle(a.nchunk[0]);
        // projected channels: the edge rows of the first two slots are in flight while the time channel runs, like the gathers they replace;
        // a projected node table (rare: the reference's node tables are zero) adds its rows here
        f4 pq[2][4];
        bool proj_e = false;
        if constexpr (!TR) {
            if (work && a.pt_node != nullptr) {
                for (int p = 0; p < P; ++p) { pt_load(pq[0], a.pt_node, ids, p); pt_add(integral_constant<int, 0>{}, pq[0]); }
            }
            proj_e = work && a.pt_edge != nullptr;
            if (proj_e) { pt_load(pq[0], a.pt_edge, eids, 0); pt_load(pq[1], a.pt_edge, eids, 1); }
        }
        if (work_e) prefill(bq, cu, a.edge_feat, eids, a.Fe);          // in flight while the time channel runs
        TACC(T_PNODE);
        if (work) run_time(integral_constant<int, 6>{}, a.nchunk[2]); else run_idle(a.nchunk[2]);
        TACC(T_PTIME);
        if (work_e) run_gathered(integral_constant<int, 3>{}, bq, cu, a.nchunk[1], a.edge_feat, eids, a.Fe); else run_idle(a.nchunk[1]);
        if constexpr (!TR) {
            if (proj_e) {
                for (int p = 0; p < P; p += 2) {       // slots 0 and 1 were loaded above; patches of more slots load the next two after these
                    pt_add(integral_constant<int, 3>{}, pq[0]);
                    if (p + 1 < P) pt_add(integral_constant<int, 3>{}, pq[1]);
                    if (p + 2 < P) { pt_load(pq[0], a.pt_edge, eids, p + 2); pt_load(pq[1], a.pt_edge, eids, p + 3); }
                }
            }
        }
        TACC(T_PEDGE);
        if (active) run_cooc(integral_constant<int, 9>{}, a.nchunk[3]); else run_idle(a.nchunk[3]);
        TACC(T_PCOOC);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // gathers issued past the end of a channel
    }
    TACC(T_PROJ);
    __syncthreads();     // everyone is done with the window arrays and the slab
    if (NP == 2 && paired) {
        // f4: source tiles of the second pair take rows 0 .. 149 (node, edge, time channels: tiles 0 .. 8 whole, tile 9 rows 144 .. 149) of the
        // first pair's same tile through the (now free) K/V region; [donor tile tt][x tile i][lane] float4
        f4* xch = reinterpret_cast<f4*>(lds);
        if (donor) {
#pragma unroll
            for (int i = 0; i < 10; ++i) xch[(tt * 10 + i) * 64 + lane] = x[i];
        }
        __syncthreads();
        if (src_shared) {
#pragma unroll
            for (int i = 0; i < 9; ++i) x[i] = xch[(tt * 10 + i) * 64 + lane];
            const f4 v = xch[(tt * 10 + 9) * 64 + lane];       // tile 9 = rows 144 + 4 g + r: time channel up to row 149
            if (g == 0) x[9] = v;
            else if (g == 1) { x[9].x = v.x; x[9].y = v.y; }
        }
        __syncthreads();
    }
    // K, V and the slack behind them: rows of absent tokens are read as MFMA operands and must be finite
    for (int i = tid; i < kLdsRing / 4; i += NTHR) reinterpret_cast<f4*>(lds)[i] = zero4();
    tap_store<TPW>(x, a.tap_enc, b, a.Tmax, ord, tt, c, g);

    float* Kb = lds + kLdsK;
    float* Vb = lds + kLdsV;
    float* misc = lds + kLdsMisc;
    const int64_t trow = b * T + 16 * tt + c;                  // training: this lane's dense activation row
    const bool tokv = pair_ok && 16 * tt + c < T;

    if (a.slab_in_ring) {        // the ring was the projection slab until now: start the layer stream (one exposed DMA latency).  Outside the
        ws.open(a.stream, kLdsRing, lane, wave, a.nstages, NW);  // layer loop: inside it the compiler kept the eight DMA addresses live (spilled)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    for (int l = 0; l < a.NL; ++l) {
        const LayerP& W = a.layer[l];
        TACC(T_MISC);
        float* b1s = misc + kMiscB1 + (l & 1) * kHid;
        int tl = tid;
        // (PL: tid + NTHR and the 64-bit form of lane * 4 below are formed where they are used, not kept — spilled — through the layers;
        //  with both, <4, false, 8, 1> needs 243 VGPRs and no scratch, <8, false, 8, 1> spills the 2 VGPRs of the per-token form)
        if constexpr (PL != 0) asm volatile("" : "+v"(tl));
        for (int i = tl; i < kHid; i += NTHR) b1s[i] = W.b1[i];
        if (l == 0) __syncthreads();     // the re-zeroing of K/V above is complete before the first K/V rows are written

        f4 xn[kNT];
        float ln_mean = 0.f, ln_rstd = 0.f;
        if constexpr (TR) { if (l == 0) store_rows(a.tr.X[0], trow, x, g, tokv); }      // X[l + 1] leaves with the FFN's residual add
        ws.fit(2);                       // LN0 gamma, beta: two vector fragments
        if (active) layernorm(xn, x, lds + kLdsRing + ws.pos * kFrag, lds + kLdsRing + (ws.pos + 1) * kFrag, g, ln_mean, ln_rstd);
        ws.advance(2);
        f4 ao[kNT];                      // training: the out-projection sum of both heads (dropout applies to the finished sum); unused otherwise
        if constexpr (TR) {
            store_rows(a.tr.layer[l].xn0, trow, xn, g, tokv);
            if (tokv && g == 0) { a.tr.layer[l].m0[trow] = ln_mean; a.tr.layer[l].r0[trow] = ln_rstd; }
#pragma unroll
            for (int i = 0; i < kNT; ++i) ao[i] = zero4();
        }
        auto& xo = [&]() -> f4 (&)[kNT] { if constexpr (TR) return ao; else return x; }();      // where the out-projection accumulates
        float xk0 = 0.f, xk1 = 0.f;      // LN(x) rows 192..199 as the two packed B operands of the last k-chunk
        kpack(xn[kKC - 1], xk0, xk1);
        // layer 0 with constant input channels: the k-chunks the rank-3 term stands for and its per-token operand (qkv_group)
        int skip0 = 0;
        float ck0 = 0.f;
        if constexpr (!TR) {
            if (l == 0 && a.qkv0_skip > 0) {
                skip0 = a.qkv0_skip;
                ck0 = g == 0 ? ln_rstd : g == 1 ? -ln_mean * ln_rstd : g == 2 ? 1.0f : 0.f;
            }
        }
        TACC(T_LN);

#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            // ================= Q, K, V of head h =================
            f4 qa[7];
            {
                ws.fit(1);               // bias fragment: rows 100h .. 100h+99 of the q bias; elements 100 .. 107: the k and v bias of rows 96 .. 99
                const float* bq = lds + kLdsRing + ws.pos * kFrag + 4 * g;
#pragma unroll
                for (int j = 0; j < 7; ++j) qa[j] = lds4(bq + 16 * j);
                ws.advance(1);
                qkv_group(qa, xn, xk0, xk1, ws, ringl, active, skip0, a.qkv0c + 64 * (19 * h), lane, ck0);
                // Tile 6 is the COMBINED tile of the head (FragDesc kmode 8): lane group 0 holds rows 96 .. 99 of Q^T, group 1 those of K^T, group 2
                // those of V^T (the K and V parts below run 6 tiles instead of 7: 9.5 % of the layer's QKV MFMAs).  Every wave passed a stream
                // barrier since its last read of the previous head's K / V (the out-projection and this group lie in between): their rows
                // can be written.
                if (active && (g == 1 || g == 2)) *reinterpret_cast<f4*>((g == 2 ? Vb : Kb) + (tokbase + 16 * tt + c) * kKV + 96) = qa[6];
                if constexpr (TR) {
                    if (tokv && (g == 1 || g == 2)) *reinterpret_cast<f4*>(a.tr.layer[l].qkv + trow * (3 * kD) + g * kD + kHD * h + 96) = qa[6];
                }
                if (g != 0) qa[6] = zero4();          // rows 100 .. 111 of Q^T do not exist
                if constexpr (TR) {
                    if (tokv) {
                        float* qp = a.tr.layer[l].qkv + trow * (3 * kD) + kHD * h + 4 * g;
#pragma unroll
                        for (int j = 0; j < 7; ++j)
                            if (j < 6 || g == 0) *reinterpret_cast<f4*>(qp + 16 * j) = qa[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < 7; ++j) qa[j] = qa[j] * a.qscale;
            }
#pragma unroll 1
            for (int kv = 0; kv < 2; ++kv) {
                f4 acc[6];               // rows 0 .. 95 of K^T / V^T (rows 96 .. 99 came out of the combined tile above)
                ws.fit(1);
                const float* bk = lds + kLdsRing + ws.pos * kFrag + 4 * g;
#pragma unroll
                for (int j = 0; j < 6; ++j) acc[j] = lds4(bk + 16 * j);
                ws.advance(1);
                qkv_group(acc, xn, xk0, xk1, ws, ringl, active, skip0, a.qkv0c + 64 * (19 * h + 7 + 6 * kv), lane, ck0);
                if (active) {
                    float* row = (kv ? Vb : Kb) + (tokbase + 16 * tt + c) * kKV + 4 * g;
#pragma unroll
                    for (int j = 0; j < 6; ++j) *reinterpret_cast<f4*>(row + 16 * j) = acc[j];
                }
                if constexpr (TR) {
                    if (tokv) {
                        float* kp = a.tr.layer[l].qkv + trow * (3 * kD) + (kv + 1) * kD + kHD * h + 4 * g;
#pragma unroll
                        for (int j = 0; j < 6; ++j) *reinterpret_cast<f4*>(kp + 16 * j) = acc[j];
                    }
                }
            }
            TACC(T_QKV);
            __syncthreads();
            TACC(T_QKVBAR);

            // ================= attention of head h for this wave's 16 queries =================
            f4 oa[7];
#pragma unroll
            for (int j = 0; j < 7; ++j) oa[j] = zero4();
            if (active) {
                f4 sa[TPW];
#pragma unroll
                for (int kt = 0; kt < TPW; ++kt) sa[kt] = zero4();
                // S^T[key][query] = sum_d K[key][d] * Q^T[d][query].  The packed form leaves out key tiles its pair does not have, by halves: a
                // pair of one or two tiles runs two, any other four (a form of its own per tile count — four copies of both products — spills
                // 28 VGPRs; this one needs no scratch).  The rows of a tile the pair does not have belong to its neighbours in the workgroup, or
                // lie up to 16 rows past the region in what follows it (V, the weight ring: filled since the prologue); they are finite, the
                // scores are masked below, and P V adds weight zero times a finite row: the bits are those of the unpacked kernels.
                if constexpr (PK) {
                    if (nwv <= 2) s_like_n<2>(sa, Kb + tokbase * kKV, qa, c, g);
                    else s_like_n<4>(sa, Kb + tokbase * kKV, qa, c, g);
                } else s_like<TPW>(sa, Kb + tokbase * kKV, qa, c, g);
                // softmax over keys (rows 16kt + 4g + r); keys >= T do not exist
                float mx = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < TPW; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int key = 16 * kt + 4 * g + r;
                        if (key >= T) sa[kt][r] = -INFINITY;
                        mx = fmaxf(mx, sa[kt][r]);
                    }
                mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
                mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
                float sum = 0.f;
                // The padding key stands for m_s + m_d identical keys: its weight counts that often in the row sum and in P V (times 1 is exact:
                // every other key, and a pair without padding, is untouched).  Key 16 kt + 4 g + r is the padding token where kt is its tile
                // (a scalar) and r == dq.  dq is made opaque per head: left to itself hipcc forms the 4 TPW factors once, outside the layer
                // loop, and keeps them in registers through the whole kernel (16 VGPRs: the 128-token kernels spill).
                int dq = (padtok & 15) - 4 * g;
                if constexpr (!TR) asm volatile("" : "+v"(dq));
#pragma unroll
                for (int kt = 0; kt < TPW; ++kt) {
                    const float wk = (!TR && (padtok >> 4) == kt) ? padw : 1.0f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        sa[kt][r] = __expf(sa[kt][r] - mx);
                        if constexpr (!TR) sa[kt][r] *= (dq == r) ? wk : 1.0f;
                        sum += sa[kt][r];
                    }
                }
                sum += __shfl_xor(sum, 16, 64);
                sum += __shfl_xor(sum, 32, 64);
                const float inv = 1.0f / sum;
#pragma unroll
                for (int kt = 0; kt < TPW; ++kt) sa[kt] *= inv;
                if constexpr (TR) {
                    // probabilities of query 16 tt + c over keys 16 kt + 4 g + r: row (b H + h) T + query of the [B H][T][T] buffers; the
                    // dropout of nn.MultiheadAttention acts on them (mask index = offset in that buffer)
                    const int64_t prow = ((b * 2 + h) * (int64_t)T + 16 * tt + c) * T;
                    const uint32_t sk = a.tr.dr.site_key((uint32_t)(4 * l + 0));
                    float* const Pp = a.tr.layer[l].P + prow;
                    float* const Pdp = a.tr.layer[l].Pd + prow;
                    const bool vec = (T & 3) == 0;           // rows of T floats: float4 stores need T % 4 == 0 (wave-uniform)
#pragma unroll
                    for (int kt = 0; kt < TPW; ++kt) {
                        const int key0 = 16 * kt + 4 * g;
                        const f4 pv = sa[kt];
#pragma unroll
                        for (int r = 0; r < 4; ++r) sa[kt][r] *= a.tr.dr.mask32(sk, (uint32_t)prow + key0 + r);
                        if (vec) {
                            if (tokv && key0 < T) { *reinterpret_cast<f4*>(Pp + key0) = pv; *reinterpret_cast<f4*>(Pdp + key0) = sa[kt]; }
                        } else {
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                if (tokv && key0 + r < T) { Pp[key0 + r] = pv[r]; Pdp[key0 + r] = sa[kt][r]; }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                // O^T[d][query] = sum_key V[key][d] * P^T[key][query]  (rows >= 100 are junk x zero weight columns)
                if constexpr (PK) {
                    if (nwv <= 2) pv_like<2>(oa, Vb + tokbase * kKV, reinterpret_cast<const f4 (&)[2]>(sa), c, g);
                    else pv_like<4>(oa, Vb + tokbase * kKV, sa, c, g);
                } else pv_like<TPW>(oa, Vb + tokbase * kKV, sa, c, g);
            }
            if constexpr (TR) {
                if (tokv) {
                    float* op = a.tr.layer[l].oa + trow * kD + kHD * h + 4 * g;
#pragma unroll
                    for (int j = 0; j < 7; ++j)
                        if (j < 6 || g == 0) *reinterpret_cast<f4*>(op + 16 * j) = oa[j];
                }
            }
            TACC(T_ATTN);
            // ================= out-projection, accumulated straight into the residual: x^T += Wo[:, head h] . O^T =================
            proj_t(xo, oa, ws, ringl, active);
            TACC(T_OPROJ);
        }
        if constexpr (!TR) {
            // The GELU table into the V region (kLdsGelu), by every wave, with or without tokens.  Every wave is past the stage barriers of head
            // 1's out-projection, and its last read of V (the P V product of head 1) lies in front of the first of them: V is dead.  The DMA
            // lands behind the bias add and LN1; the wait and the barrier in front of the FFN loop publish it.  After the loop nothing has
            // to be waited for: the next layer's first K/V stores follow its Q product — seven stage barriers after any wave's last GELU —
            // and the epilogue's columns over the table (kLdsMean, kLdsMeanG) are written behind the barrier that follows the loop.
            int gl4 = lane * 4;
            asm volatile("" : "+v"(gl4));      // (the per-lane source address is formed here, not kept — spilled — through the layers)
            stage_gelu_table(a.gelu_tab + gl4, kLdsGelu, wave, NW);
        }
        // out-projection bias (one vector fragment)
        ws.fit(1);
        {
            const float* bo = lds + kLdsRing + ws.pos * kFrag + 4 * g;
            if constexpr (TR) {          // x1 = x + dropout(Wo O + bo), DyGFormer.py:456; x re-read from the rows stored at the layer's start
                residual_dropped(x, a.tr.X[l], a.tr.layer[l].x1, ao, bo, a.tr.dr, (uint32_t)(4 * l + 1), trow, g, tokv);
            } else {
#pragma unroll
                for (int i = 0; i < kNT; ++i) x[i] = x[i] + lds4(bo + 16 * i);
            }
        }
        ws.advance(1);

        TACC(T_OPROJ);
        // ================= LN1 + FFN: 25 steps of two hidden tiles; W1 fragments [k-chunk][tile], W2 [tile][n-tile] =================
        ws.fit(2);
        if (active) layernorm(xn, x, lds + kLdsRing + ws.pos * kFrag, lds + kLdsRing + (ws.pos + 1) * kFrag, g, ln_mean, ln_rstd);
        ws.advance(2);
        kpack(xn[kKC - 1], xk0, xk1);
        auto& f2 = xo;                   // where the second FFN product accumulates
        if constexpr (TR) {
            store_rows(a.tr.layer[l].xn1, trow, xn, g, tokv);
            if (tokv && g == 0) { a.tr.layer[l].m1[trow] = ln_mean; a.tr.layer[l].r1[trow] = ln_rstd; }
#pragma unroll
            for (int i = 0; i < kNT; ++i) ao[i] = zero4();
        }
        const uint32_t sk2 = TR ? a.tr.dr.site_key((uint32_t)(4 * l + 2)) : 0u;
        TACC(T_LN);
        ws.align26();
        if constexpr (!TR) {
            // ffn_w1 consumes its 26 fragments without a crossing and align26 crosses a stage only where the position asks for it: the table's
            // own wait and barrier
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
        const bool last = PL != 0 && l == a.NL - 1;      // the pooled layer
        const int ptok = 16 * tt + c;
        if (last) {
            // Every wave has passed the stage barriers of the last out-projection: K and V are dead.  The residual's per-side sums are
            // taken here (x1: what the per-token form adds the FFN output to).
            float wsrc, wdst;
            int ptk = ptok;
            if constexpr (!TR) asm volatile("" : "+v"(ptk));      // (the weights are formed here, not kept through the layers)
            side_weights(ptk, wsrc, wdst);
            pool_sides(x, lds + kLdsPool, wave, lane, wsrc, wdst);
        }
        // wave-uniform: the tile holds tokens of both sides, or the padding token (which counts on both)
        const bool straddle = (16 * tt < Ts && Ts < 16 * (tt + 1)) || (16 * tt <= padtok && padtok < 16 * (tt + 1));
        const bool dst_tile = 16 * tt >= Ts;
        // sums of gelu(h) over the tile's tokens of either side (row_sums8 on the step's two hidden tiles, as pool_sides); a tile of one side
        // sums once: the other side's sum of zeros is zero, so the bits do not depend on which form ran
        const bool g_pad = ptok == padtok;
        const bool g_src = ptok < Ts || (g_pad && ms > 0), g_dst = (ptok >= Ts && ptok < T && !g_pad) || (g_pad && md > 0);
        const float msf = (float)ms, mdf = (float)md;
        auto gelu_sums = [&](const f4 (&h)[2], int p) {
            // (the store address is formed here from the lane, like the weights below, so that it is not live through the FFN loop)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            float* gp = lds + kLdsGPool + wave * 2 * kHid + 32 * p + 16 * pool_sum_tile(ln) + pool_sum_row(ln);
            timeenc::f2 zs, zd;
            if (straddle) {
                // (the weights are formed here from lane masks and scalars: kept in two VGPRs through the FFN loop they spill)
                float one = 1.0f;
                asm volatile("" : "+v"(one));
                const float wsrc = g_pad ? msf : one, wdst = g_pad ? mdf : one;
                zs = row_sums8(g_src ? h[0] * wsrc : zero4(), g_src ? h[1] * wsrc : zero4());
                zd = row_sums8(g_dst ? h[0] * wdst : zero4(), g_dst ? h[1] * wdst : zero4());
            } else {
                const timeenc::f2 z = row_sums8(ptok < T ? h[0] : zero4(), ptok < T ? h[1] : zero4());
                const timeenc::f2 none{0.f, 0.f};
                zs = dst_tile ? none : z;
                zd = dst_tile ? z : none;
            }
            if (pool_sum_stores(ln)) { *reinterpret_cast<timeenc::f2*>(gp) = zs; *reinterpret_cast<timeenc::f2*>(gp + kHid) = zd; }
        };
        // W1(p) | W2(p) per step; W2 accumulates straight into the residual registers (no separate FFN accumulator: 52 VGPRs fewer)
#pragma unroll 1
        for (int p = 0; p < 25; ++p) {
            f4 h[2];
            if (active) {
                ffn_w1(h, xn, xk0, xk1, ringl + ws.pos * kFrag, b1s + 32 * p, g);
                TACC(T_F_W1);
                if constexpr (TR) {
                    if (tokv) {
                        float* hp = a.tr.layer[l].hpre + trow * kHid + 32 * p + 4 * g;
                        *reinterpret_cast<f4*>(hp) = h[0]; *reinterpret_cast<f4*>(hp + 16) = h[1];
                    }
                }
                gelu_tiles<!TR>(h, lds + kLdsGelu);
                if constexpr (TR) {      // dropout on the activation (DyGFormer.py:458): element (row, hidden unit n) draws mask(site, row * 800 + n)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int r = 0; r < 4; ++r) h[u][r] *= a.tr.dr.mask32(sk2, (uint32_t)trow * kHid + 32 * p + 16 * u + 4 * g + r);
                    if (tokv) {
                        float* hp = a.tr.layer[l].hact + trow * kHid + 32 * p + 4 * g;
                        *reinterpret_cast<f4*>(hp) = h[0]; *reinterpret_cast<f4*>(hp + 16) = h[1];
                    }
                }
                if (last) gelu_sums(h, p);
                TACC(T_F_GELU);
            }
            ws.advance(26, (TR && active) ? 4 : 0);      // training: the four hpre / hact stores of this step stay in flight through the W2 block
            TACC(T_F_ADV1);
            if ((PL == 1 || PL == 3) && last) continue;       // the pooled stream: this layer's blocks are W1 only
            if (active) ffn_w2(f2, h, ringl + ws.pos * kFrag);
            TACC(T_F_W2);
            ws.advance(26);
            TACC(T_F_ADV2);
        }
        if (!((PL == 1 || PL == 3) && last)) {
        ws.fit(1);
        {
            const float* b2 = lds + kLdsRing + ws.pos * kFrag + 4 * g;
            if constexpr (TR) {          // x_{l+1} = x1 + dropout(W2 h + b2), DyGFormer.py:460; x1 re-read from its rows (not kept through the FFN)
                residual_dropped(x, a.tr.layer[l].x1, a.tr.X[l + 1], f2, b2, a.tr.dr, (uint32_t)(4 * l + 3), trow, g, tokv);
            } else {
#pragma unroll
                for (int i = 0; i < kNT; ++i) x[i] = x[i] + lds4(b2 + 16 * i);
            }
        }
        ws.advance(1);
        TACC(T_FFN);
        tap_store<TPW>(x, a.tap_layer[l], b, a.Tmax, ord, tt, c, g);
        }
    }

    TACC(T_MISC);
    // ================= per-side mean over tokens + output layer (DyGFormer.py:181-192) =================
    __syncthreads();        // K/V are dead: reuse as scratch (PL: every wave's sums of the last layer are written)
    {
        float* pool = lds + kLdsPool;            // [wave][side][208]
        const int tok = 16 * tt + c;
        int lane4 = lane * 4;
        if constexpr (PL != 0) asm volatile("" : "+v"(lane4));
        if constexpr (PL == 0) {
            float wsrc, wdst;
            side_weights(tok, wsrc, wdst);
            pool_sides(x, pool, wave, lane, wsrc, wdst);
            TACC(T_POOL1);
            __syncthreads();
        }
        TACC(T_POOL2);
        // mean[col][208], col = 2*pair + side (4 columns of the 16-wide B operand are used; the rest multiply zeros)
        float* mean = lds + kLdsMean;
        const int Tse = Tsf, Td = Tf - Tsf;      // the means are over the tokens of the padded call
        const int npw = PK ? nwv : TPW;          // waves of this pair
        for (int i = ptid; i < 2 * kDP; i += PT) {
            const int side = i / kDP, n = i % kDP;
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < npw; ++w) s += pool[((wave0 + w) * 2 + side) * kDP + n];
            const float mv = n < kD ? s / (float)(side ? Td : Tse) : 0.f;
            if constexpr (PL == 3) { if (pair_ok) a.pooled_rows[(2 * b + side) * kPoolRow + kHid + n] = mv; }
            else mean[pi * 2 * kDP + i] = mv;
            if constexpr (TR) { if (pair_ok && n < kD) a.tr.pooled[((int64_t)side * a.B + b) * kD + n] = mv; }
        }
        if constexpr (PL != 0) {
            // mean_g[col][800]: the per-wave sums in the pair-local wave order, then the scale by 1 / T_side, then the product
            const float* gpool = lds + kLdsGPool;
            float* meang = lds + kLdsMeanG;
            for (int i = ptid; i < 2 * kHid; i += PT) {
                const int side = i / kHid, n = i % kHid;
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < npw; ++w) if (16 * w < T) s += gpool[((wave0 + w) * 2 + side) * kHid + n];      // a wave without tokens wrote nothing
                const float mg = s / (float)(side ? Td : Tse);
                if constexpr (PL == 3) { if (pair_ok) a.pooled_rows[(2 * b + side) * kPoolRow + n] = mg; }
                else meang[pi * 2 * kHid + i] = mg;
            }
            if constexpr (PL == 3) { TACC(T_E_MEAN); TSTORE(); return; }      // k_pooled_tail takes it from here
            __syncthreads();
            TACC(T_E_MEAN);
            // mean[col] += W2 . mean_g[col] + b2 on the matrix cores: wave w owns model-dim tiles w, w + NW, ...; 50 k-chunks whose fragments
            // (used by this wave only) come straight from global memory ten at a time, one group ahead.  One tile's sum is one fixed chain
            // (even chunks in acc0, odd in acc1), whichever wave of whichever kernel shape runs it.
            constexpr int GK = 10, NG = kHid / 16 / GK;
            for (int it = wave; it < kNT; it += NW) {
                const float* fp = a.w2frag + (size_t)it * (kHid / 16) * kFrag + lane4;
                f4 fa[2][GK];
#pragma unroll
                for (int u = 0; u < GK; ++u) fa[0][u] = ldg4(fp + (size_t)u * kFrag);
                const int n0 = 16 * it + 4 * g;
                f4 acc0 = n0 < kD ? ldg4(a.b2_last + n0) : zero4(), acc1 = zero4();
#pragma unroll
                for (int gk = 0; gk < NG; ++gk) {
                    if (gk + 1 < NG) {
#pragma unroll
                        for (int u = 0; u < GK; ++u) fa[(gk + 1) & 1][u] = ldg4(fp + (size_t)((gk + 1) * GK + u) * kFrag);
                    }
#pragma unroll
                    for (int u = 0; u < GK; ++u) {
                        const f4 fr = fa[gk & 1][u];
                        const f4 bm = c < 2 * NP ? lds4(meang + c * kHid + 16 * (gk * GK + u) + 4 * g) : zero4();
                        if (u & 1) { acc1 = mfma(fr.x, bm.x, acc1); acc1 = mfma(fr.y, bm.y, acc1); acc1 = mfma(fr.z, bm.z, acc1); acc1 = mfma(fr.w, bm.w, acc1); }
                        else { acc0 = mfma(fr.x, bm.x, acc0); acc0 = mfma(fr.y, bm.y, acc0); acc0 = mfma(fr.z, bm.z, acc0); acc0 = mfma(fr.w, bm.w, acc0); }
                    }
                }
                if (c < 2 * NP) {        // this lane alone owns rows n0 .. n0 + 3 of column c (written before this barrier, read after the next)
                    f4* mp = reinterpret_cast<f4*>(mean + c * kDP + n0);
                    *mp = *mp + (acc0 + acc1);
                }
            }
        }
        __syncthreads();
        if constexpr (PL != 0) TACC(T_E_W2);
        // output layer on the matrix cores: out^T[j][col] = sum_k W[j][k] mean[col][k] + b[j]; wave w owns output tiles w, w+8, ...
        // (each fragment is used by one wave only, so they come straight from global memory, all 13 of a tile in flight)
        const int ntile = (a.Fn + 15) >> 4;
        for (int jt = wave; jt < ntile; jt += NW) {
            f4 fa[kKC];
#pragma unroll
            for (int kc = 0; kc < kKC; ++kc) fa[kc] = ldg4(a.outfrag + ((size_t)jt * kKC + kc) * kFrag + lane4);
            const int j0 = 16 * jt + 4 * g;
            f4 acc0 = j0 < a.Fn ? ldg4(a.outb + j0) : zero4(), acc1 = zero4();
#pragma unroll
            for (int kc = 0; kc < kKC; ++kc) {
                const f4 bm = c < 2 * NP ? lds4(mean + c * kDP + 16 * kc + 4 * g) : zero4();
                if (kc & 1) { acc1 = mfma(fa[kc].x, bm.x, acc1); acc1 = mfma(fa[kc].y, bm.y, acc1); acc1 = mfma(fa[kc].z, bm.z, acc1); acc1 = mfma(fa[kc].w, bm.w, acc1); }
                else { acc0 = mfma(fa[kc].x, bm.x, acc0); acc0 = mfma(fa[kc].y, bm.y, acc0); acc0 = mfma(fa[kc].z, bm.z, acc0); acc0 = mfma(fa[kc].w, bm.w, acc0); }
            }
            const int64_t bo_ = paired ? (int64_t)blockIdx.x + (c >> 1) * a.pair_stride : (int64_t)blockIdx.x * NP + (c >> 1);
            if (c < 2 * NP && bo_ < a.B && j0 < a.Fn)
                *reinterpret_cast<f4*>(((c & 1) ? a.out_dst : a.out_src) + bo_ * a.Fn + j0) = acc0 + acc1;
        }
    }
    TACC(T_POOL);
    TSTORE();
}

template <int TPW, bool TR, int NW = 8, int PL = 0>
__global__ __launch_bounds__(64 * NW, NW == 8 ? 2 : 1) void k_dygformer_fused3(const Args a) {
    fused3_body<TPW, TR, NW, PL, false>(a);
}

}  // namespace v3

inline int fused3_args(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, const float* packed, const dygnn_csr* csr,
                       const float* node_feat, const float* edge_feat, const int64_t* src, const int64_t* dst, const double* times, int64_t B, int64_t G,
                       float* out_src, float* out_dst, char* ws, const WorkspaceLayout& wl, const dygnn_dygformer_taps* taps, v3::Args& a, v3::PackLayout3& f) {
    using namespace v3;
    f = make_layout3(d);
    const float* base = packed + pl.fused3;
    a.indptr = csr->indptr; a.nbr = csr->nbr; a.eid = csr->eid; a.ts = csr->ts;
    a.src = src; a.dst = dst; a.times = times;
    a.hist_len = reinterpret_cast<const int32_t*>(ws + wl.hist_len);
    a.end_pos = reinterpret_cast<const int64_t*>(ws + wl.end_pos);
    a.cd = reinterpret_cast<const CallDims*>(ws + wl.dims);
    a.node_feat = node_feat; a.edge_feat = edge_feat; a.time_w = w->time_w; a.time_b = w->time_b; a.lut = packed + pl.lut;
    a.stream = base + f.stream; a.nstages = f.nstages;
    a.bias_x = base + f.bias_x;
    for (int l = 0; l < d.NL; ++l) {
        a.layer[l].b1 = w->layers[l].ffn0_bias;
        a.tap_layer[l] = taps ? taps->layer_out[l] : nullptr;
    }
    a.outfrag = base + f.aux;
    a.w2frag = base + f.w2; a.b2_last = w->layers[d.NL - 1].ffn1_bias;
    a.gelu_tab = base + f.gelu;
    a.projw = base + f.proj; a.proj_frags = (int)f.nproj; a.slab_chunks = f.slab_chunks; a.scr_floats = f.scr_floats;
    a.slab_in_ring = f.slab_in_ring;
    a.tab_off = f.tab_off; a.tab_slots = f.tab_slots; a.tab_bits = f.tab_bits;
    a.outT = packed + pl.outputT; a.outb = w->output_b;
    a.out_src = out_src; a.out_dst = out_dst;
    a.pooled_rows = reinterpret_cast<float*>(ws + wl.pooled);
    a.tap_enc = taps ? taps->encoder_input : nullptr;
    a.stamps = taps ? reinterpret_cast<unsigned long long*>(taps->phase_cycles) : nullptr;
    a.B = B; a.G = G; a.num_nodes = csr->num_nodes; a.Fn = d.Fn; a.Fe = d.Fe; a.Ft = d.Ft; a.P = d.P; a.L = d.L; a.NL = d.NL; a.Tmax = d.Tmax;
    const int K[4] = {d.P * d.Fn, d.P * d.Fe, d.P * d.Ft, d.P * d.C};
    for (int ch = 0; ch < 4; ++ch) a.nchunk[ch] = (K[ch] + 15) / 16;
    a.proj_skip0 = 0; a.proj_skip1 = 0; a.proj_cut = 0;
    a.qscale = (float)sqrt(1.0 / (double)d.hd);
    return DYGNN_OK;
}

}  // namespace dygnn
