// Weight packing of the fused DyGFormer path: every kernel of it reads its weights as one linear stream of 1-KiB MFMA-A fragments in
// consumption order (fused3_device.h: WStream).
#include <vector>

#include "fused3_device.h"
#include "fused3_host.h"
#include "fused3_plan.h"

namespace dygnn {
namespace v3 {

// ================================================================================================
// packing: the stream is described on the host as a list of fragment descriptors in consumption order (with the pad
// fragments the ring rule asks for), uploaded, and materialised by one kernel.
// ================================================================================================
struct FragDesc {
    const float* src;     // nullptr = pad fragment (zeros)
    int ld;               // matrix fragment: row stride; -1: vector fragment, element e = src[c0 + e] for e < rmax
    int r0, rmax;         // element (c,g,t): row = r0 + c, valid iff 0 <= row < rmax
    int c0, cmax;         //                  col = c0 + 4g + t, valid iff col < cmax
    int kmode;            // 1: last chunk of a K = 200 product, 8 real k in two MFMAs: t < 2: col = c0 + {0,4,1,5}[g] + 2t, t >= 2: zero (mma_group2)
                          // 2: last chunk of a head-dim (100) contraction, 4 real k in one MFMA: t = 0: col = c0 + g, t >= 1: zero (mma_group1)
                          // +4: transposed source, element (row, col) = src[col * ld + row] (the backward stream: W^T fragments of the same tensors)
                          // +8: the COMBINED last head-dim tile of a head's q | k | v (src = in_proj base, r0 = 100 h + 96): rows 4 G .. 4 G + 3 of the tile
                          //     are rows r0 .. r0 + 3 of row block G (q, k, v at G = 0, 1, 2: row = r0 + 200 G + (c & 3)), G = 3 is padding.  The three
                          //     parts' tiles 6 hold 4 real rows each (head dim 100 = 6 tiles + 4): one MFMA tile carries all twelve.
                          //     Vector fragment (+8): elements 100 .. 107 = src[c0 + 200 + 96 ..], src[c0 + 400 + 96 ..] (the k and v bias of those rows)
};
__device__ __forceinline__ float frag_element(const FragDesc& d, int e) {       // e = 4 * lane + t of the fragment
    if (d.src == nullptr) return 0.f;
    const int t = e & 3, lane = (e >> 2) & 63;
    const int c = lane & 15, g = lane >> 4;
    if (d.ld < 0) {
        if (e < d.rmax) return d.src[d.c0 + e];
        if ((d.kmode & 8) && e >= 100 && e < 108) return d.src[d.c0 + kD * ((e - 100) / 4 + 1) + 96 + ((e - 100) & 3)];
        return 0.f;
    }
    int row = d.r0 + c;
    bool rok = row >= 0 && row < d.rmax;
    if (d.kmode & 8) { row = d.r0 + kD * (c >> 2) + (c & 3); rok = (c >> 2) < 3; }
    int col = d.c0 + 4 * g + t;
    if ((d.kmode & 3) == 1) col = t < 2 ? d.c0 + (g & 1) * 4 + (g >> 1) + 2 * t : d.cmax;
    if ((d.kmode & 3) == 2) col = t == 0 ? d.c0 + g : d.cmax;
    if (!rok || col >= d.cmax) return 0.f;
    return (d.kmode & 4) ? d.src[(size_t)col * d.ld + row] : d.src[(size_t)row * d.ld + col];
}

__global__ void k_pack_stream(const FragDesc* __restrict__ desc, int64_t nfrag, float* __restrict__ dst) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nfrag * kFrag) return;
    dst[idx] = frag_element(desc[idx >> 8], (int)(idx & 255));
}

// every fragment stream of the packed buffer in ONE launch (the in-place refresh after an optimizer step): the descriptor table is one
// array, `r` maps its ranges to their destinations
struct PackRanges { int n; int64_t start[6 + 2 * DYGNN_MAX_LAYERS]; float* dst[5 + 2 * DYGNN_MAX_LAYERS]; };
__global__ void k_pack_ranges(const FragDesc* __restrict__ desc, const PackRanges r) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t f = idx >> 8;
    if (f >= r.start[r.n]) return;
    int q = 0;
    while (q + 1 < r.n && f >= r.start[q + 1]) ++q;
    r.dst[q][(f - r.start[q]) * kFrag + (idx & 255)] = frag_element(desc[f], (int)(idx & 255));
}
// the four projection biases in model-dim order [208]
__global__ void k_pack_bias4(const float* __restrict__ b0, const float* __restrict__ b1, const float* __restrict__ b2, const float* __restrict__ b3, float* __restrict__ dst) {
    const int i = threadIdx.x;
    if (i >= kDP) return;
    const int ch = i / kC, j = i % kC;
    dst[i] = i < kD ? (ch == 0 ? b0 : ch == 1 ? b1 : ch == 2 ? b2 : b3)[j] : 0.f;
}

__global__ void k_pack_vec3(const float* __restrict__ src, int n_valid, int src_off, float* __restrict__ dst, int dst_off, int n_total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_total) return;
    dst[dst_off + i] = i < n_valid ? src[src_off + i] : 0.f;
}

// layer 0's constant-channel operands, both prefix lengths: dst[p][tile][lane], K0 = 48 (p = 0) and 96 (p = 1); `bias` = the packed bias_x
__global__ void k_pack_qkv0_const(const float* __restrict__ in_proj, const float* __restrict__ gamma, const float* __restrict__ beta,
                                  const float* __restrict__ bias, float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * kQkvTiles * 64) return;
    const int p = i / (kQkvTiles * 64), r = i % (kQkvTiles * 64);
    dst[i] = qkv0_const(in_proj, gamma, beta, bias, 48 * (p + 1), r / 64, r % 64);
}

// host mirror of WStream's position rule
struct StreamBuilder {
    std::vector<FragDesc> frags;
    int pos = 0;
    void pad(int n) { for (int i = 0; i < n; ++i) frags.push_back(FragDesc{nullptr, 0, 0, 0, 0, 0, 0}); pos = (pos + n) % kRing; }
    void fit(int n) { if (pos + n > kRing) pad(kRing - pos); }
    void align26() { if (pos != 0 && pos != 26) pad(pos < 26 ? 26 - pos : kRing - pos); }
    void put(const float* src, int ld, int r0, int rmax, int c0, int cmax, int kmode = 0) { frags.push_back(FragDesc{src, ld, r0, rmax, c0, cmax, kmode}); pos = (pos + 1) % kRing; }
    void put_vec(const float* src, int off, int n) { put(src, -1, 0, n, off, 0); }     // floats [0, n) of the fragment = src[off ..]
};

// pooled: the stream of k_dygformer_fused3<.., PL = 1> — the last layer's FFN carries its W1 blocks only and ends with the last of them (that
// layer's W2 and b2 are read by the epilogue: build_w2)
static void build_stream(const Dims& d, const dygnn_dygformer_weights* w, StreamBuilder& sb, int (&nchunk)[4], bool pooled = false) {
    const int K[4] = {d.P * d.Fn, d.P * d.Fe, d.P * d.Ft, d.P * d.C};
    for (int ch = 0; ch < 4; ++ch) nchunk[ch] = (K[ch] + 15) / 16;
    for (int l = 0; l < d.NL; ++l) {
        const dygnn_encoder_layer_weights& L = w->layers[l];
        sb.fit(2);
        sb.put_vec(L.norm0_weight, 0, kD);
        sb.put_vec(L.norm0_bias, 0, kD);
        for (int h = 0; h < 2; ++h) {
            for (int part = 0; part < 3; ++part) {           // q, k, v row blocks of in_proj
                // q: 7 tiles, the seventh = the COMBINED tile (rows 96 .. 99 of q, k and v: FragDesc kmode 8); k, v: tiles 0 .. 5
                const int nt = part == 0 ? 7 : 6;
                sb.fit(1);
                if (part == 0) sb.frags.push_back(FragDesc{L.in_proj_bias, -1, 0, kHD, kHD * h, 0, 8}), sb.pos = (sb.pos + 1) % kRing;
                else sb.put_vec(L.in_proj_bias, part * kD + kHD * h, kHD);      // head rows of the bias (elements 0 .. 95 are read)
                sb.fit(nt);
                for (int kc = 0; kc < kKC; ++kc) {
                    const int ks = kc == kKC - 1 ? 1 : 0;
                    for (int j = 0; j < 6; ++j)
                        sb.put(L.in_proj_weight ? L.in_proj_weight + (size_t)part * kD * kD : nullptr, kD, kHD * h + 16 * j, kHD * (h + 1), 16 * kc, kD, ks);
                    if (part == 0) sb.put(L.in_proj_weight, kD, kHD * h + 96, 3 * kD, 16 * kc, kD, ks | 8);
                    if (kc + 1 < kKC) sb.fit(nt);
                }
            }
            sb.fit(13);
            for (int j = 0; j < 7; ++j) {                    // out-projection: [d-chunk j][n-tile i], columns of head h
                for (int i = 0; i < kNT; ++i) sb.put(L.out_proj_weight, kD, 16 * i, kD, kHD * h + 16 * j, kHD * (h + 1), j == 6 ? 2 : 0);
                if (j + 1 < 7) sb.fit(13);
            }
        }
        sb.fit(1);
        sb.put_vec(L.out_proj_bias, 0, kD);
        sb.fit(2);
        sb.put_vec(L.norm1_weight, 0, kD);
        sb.put_vec(L.norm1_bias, 0, kD);
        sb.align26();
        auto put_w1 = [&](int p) {
            for (int kc = 0; kc < kKC; ++kc)
                for (int u = 0; u < 2; ++u) sb.put(L.ffn0_weight, kD, 16 * (2 * p + u), kHid, 16 * kc, kD, kc == kKC - 1);
        };
        auto put_w2 = [&](int p) {
            for (int u = 0; u < 2; ++u)
                for (int i = 0; i < kNT; ++i) sb.put(L.ffn1_weight, kHid, 16 * i, kD, 16 * (2 * p + u), kHid);
        };
        if (pooled && l == d.NL - 1) {
            for (int p = 0; p < 25; ++p) { put_w1(p); }
            break;
        }
        for (int p = 0; p < 25; ++p) { put_w1(p); put_w2(p); }
        sb.fit(1);
        sb.put_vec(L.ffn1_bias, 0, kD);
    }
}

// backward stream of layer l's FFN block (k_ffn_bwd): per hidden step p the W2^T block [k-chunk over channels][hidden tile u] and the
// W1^T block [hidden chunk u][channel tile i] — the transposes of the forward's two blocks, cut from the same tensors — then LN1's gamma
static void build_bwd_ffn(const dygnn_encoder_layer_weights& L, StreamBuilder& sb) {
    for (int p = 0; p < 25; ++p) {
        for (int kc = 0; kc < kKC; ++kc)
            for (int u = 0; u < 2; ++u) sb.put(L.ffn1_weight, kHid, 16 * (2 * p + u), kHid, 16 * kc, kD, (kc == kKC - 1 ? 1 : 0) | 4);
        for (int u = 0; u < 2; ++u)
            for (int i = 0; i < kNT; ++i) sb.put(L.ffn0_weight, kD, 16 * i, kD, 16 * (2 * p + u), kHid, 4);
    }
    sb.fit(1);
    sb.put_vec(L.norm1_weight, 0, kD);
}
constexpr int64_t kBwdFfnFrags = 25 * 52 + 1;
// backward stream of layer l's attention block (k_attn_bwd): per head Wo[:, h]^T in the shape of a Q/K/V product ([channel chunk][7 head-dim
// tiles]), then Wq[h]^T, Wv[h]^T, Wk[h]^T in the shape of the out-projection ([head-dim chunk][13 channel tiles]); then LN0's gamma
static void build_bwd_attn(const dygnn_encoder_layer_weights& L, StreamBuilder& sb) {
    for (int h = 0; h < 2; ++h) {
        sb.fit(7);
        for (int kc = 0; kc < kKC; ++kc) {
            for (int j = 0; j < 7; ++j)
                sb.put(L.out_proj_weight, kD, kHD * h + 16 * j, kHD * (h + 1), 16 * kc, kD, (kc == kKC - 1 ? 1 : 0) | 4);
            if (kc + 1 < kKC) sb.fit(7);
        }
        const int order[3] = {0, 2, 1};              // q, v, k
        for (int o = 0; o < 3; ++o) {
            const float* Wp = L.in_proj_weight ? L.in_proj_weight + (size_t)order[o] * kD * kD : nullptr;
            sb.fit(13);
            for (int j = 0; j < 7; ++j) {
                for (int i = 0; i < kNT; ++i) sb.put(Wp, kD, 16 * i, kD, kHD * h + 16 * j, kHD * (h + 1), (j == 6 ? 2 : 0) | 4);
                if (j + 1 < 7) sb.fit(13);
            }
        }
    }
    sb.fit(1);
    sb.put_vec(L.norm0_weight, 0, kD);
}
static int64_t bwd_attn_frags() {
    static float dummy;
    dygnn_encoder_layer_weights lw{};
    lw.in_proj_weight = lw.out_proj_weight = lw.norm0_weight = &dummy;
    StreamBuilder sb;
    build_bwd_attn(lw, sb);
    return (int64_t)sb.frags.size();
}

// projection fragments in step order (channels node, time, edge, cooc; 4 tiles per k-chunk slot), staged through two LDS halves
int proj_slots(int nchunk) { return (nchunk + 3) / 4 * 4; }
static void build_proj(const Dims& d, const dygnn_dygformer_weights* w, StreamBuilder& sb) {
    const float* pw[4] = {w->proj_node_w, w->proj_edge_w, w->proj_time_w, w->proj_cooc_w};
    const int K[4] = {d.P * d.Fn, d.P * d.Fe, d.P * d.Ft, d.P * d.C};
    const int order[4] = {0, 2, 1, 3};
    for (int o = 0; o < 4; ++o) {
        const int ch = order[o], t0 = (kC * ch) / 16;
        const int n = (K[ch] + 15) / 16;
        for (int kc = 0; kc < n; ++kc)
            for (int u = 0; u < 4; ++u) sb.put(pw[ch], K[ch], 16 * (t0 + u) - kC * ch, kC, 16 * kc, K[ch]);
        sb.pad(4 * (proj_slots(n) - n));           // every channel occupies whole groups of four slots (the kernel's loop bodies are groups)
    }
}

// fragments that do not travel through the ring (read by one wave each): the output layer [tile][k-chunk]
static void build_aux(const Dims& d, const dygnn_dygformer_weights* w, StreamBuilder& sb) {
    const int ntile = (d.Fn + 15) / 16;
    for (int jt = 0; jt < ntile; ++jt)
        for (int kc = 0; kc < kKC; ++kc) sb.put(w->output_w, kD, 16 * jt, d.Fn, 16 * kc, kD);
}

// the last layer's W2 for the pooled epilogue, laid out like the output layer: [13 n-tiles][50 k-chunks], each fragment read by one wave
constexpr int64_t kW2Frags = (int64_t)kNT * (kHid / 16);
static void build_w2(const Dims& d, const dygnn_dygformer_weights* w, StreamBuilder& sb) {
    for (int i = 0; i < kNT; ++i)
        for (int kc = 0; kc < kHid / 16; ++kc) sb.put(w->layers[d.NL - 1].ffn1_weight, kHid, 16 * i, kD, 16 * kc, kHid);
}

static int64_t stream_frags(const Dims& d, bool pooled) {
    // fragment count of build_stream without touching weights: run the builder with null sources
    dygnn_dygformer_weights w{};
    static float dummy;
    w.proj_node_w = w.proj_edge_w = w.proj_time_w = w.proj_cooc_w = &dummy;
    dygnn_encoder_layer_weights lw{};
    lw.in_proj_weight = lw.out_proj_weight = lw.ffn0_weight = lw.ffn1_weight = &dummy;
    lw.in_proj_bias = lw.out_proj_bias = lw.ffn1_bias = lw.norm0_weight = lw.norm0_bias = lw.norm1_weight = lw.norm1_bias = &dummy;
    for (int l = 0; l < d.NL; ++l) w.layers[l] = lw;
    StreamBuilder sb;
    int nchunk[4];
    build_stream(d, &w, sb, nchunk, pooled);
    return (int64_t)sb.frags.size();
}
// the same counts without running the builder on every forward call (make_layout3 is on the call path): they depend on the number of
// layers alone, so both forms of every depth are counted once per process
static int64_t stream_frags_cached(const Dims& d, bool pooled) {
    struct Table { int64_t n[2][DYGNN_MAX_LAYERS + 1]; };
    static const Table t = [] {
        Table r{};
        for (int nl = 1; nl <= DYGNN_MAX_LAYERS; ++nl) {
            Dims dd{};
            dd.NL = nl;
            r.n[0][nl] = stream_frags(dd, false);
            r.n[1][nl] = stream_frags(dd, true);
        }
        return r;
    }();
    return (d.NL >= 1 && d.NL <= DYGNN_MAX_LAYERS) ? t.n[pooled ? 1 : 0][d.NL] : stream_frags(d, pooled);
}

PackLayout3 make_layout3(const Dims& d) {
    PackLayout3 f;
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += (n + 63) & ~size_t(63); return r; };
    f.bias_x = take(kDP);
    f.nfrag = stream_frags_cached(d, false);
    f.nstages = (int)((f.nfrag + kStage - 1) / kStage);
    f.stream = take((size_t)(f.nstages + 1) * kStage * kFrag);
    f.naux = (int64_t)((d.Fn + 15) / 16) * kKC;
    f.aux = take((size_t)f.naux * kFrag);
    const int K[4] = {d.P * d.Fn, d.P * d.Fe, d.P * d.Ft, d.P * d.C};
    f.nproj = 0;
    for (int ch = 0; ch < 4; ++ch) f.nproj += 4 * (int64_t)proj_slots((K[ch] + 15) / 16);
    f.proj = take((size_t)f.nproj * kFrag);
    f.bwd_nstages = (int)((kBwdFfnFrags + kStage - 1) / kStage);
    for (int l = 0; l < d.NL; ++l) f.bwd[l] = take((size_t)(f.bwd_nstages + 1) * kStage * kFrag);
    f.bwa_frags = bwd_attn_frags();
    f.bwa_nstages = (int)((f.bwa_frags + kStage - 1) / kStage);
    for (int l = 0; l < d.NL; ++l) f.bwa[l] = take((size_t)(f.bwa_nstages + 1) * kStage * kFrag);
    f.nfrag_p = stream_frags_cached(d, true);
    f.nstages_p = (int)((f.nfrag_p + kStage - 1) / kStage);
    f.stream_p = take((size_t)(f.nstages_p + 1) * kStage * kFrag);
    f.w2 = take((size_t)kW2Frags * kFrag);
    f.qkv0c = take((size_t)2 * kQkvTiles * 64);
    f.gelu = take((size_t)kGeluTabFloats);
    f.desc = take(((size_t)(f.nfrag + f.naux + f.nproj + d.NL * (kBwdFfnFrags + f.bwa_frags) + f.nfrag_p + kW2Frags) * sizeof(FragDesc) + 3) / 4);
    // prologue LDS split: pairs per workgroup, window arrays (5 x 2 sides x Smax ints per pair), projection slab
    const int per_pair = 5 * 2 * ((d.Smax + 3) & ~3);
    f.np = 0; f.slab_in_ring = 0; f.scr_floats = 0; f.slab_chunks = 0; f.tab_off = 0; f.tab_slots = 0; f.tab_bits = 0;
    f.scr_floats8 = 0; f.slab_chunks8 = 0;
    if (d.Tmax <= 64 && 2 * per_pair + 8 * 4 * kFrag <= kScratchFloats) f.np = 2;
    else if (d.Tmax <= 128 && per_pair + 8 * 4 * kFrag <= kScratchFloats) f.np = 1;
    else if (d.Tmax <= 128 && per_pair <= kScratchFloats) { f.np = 1; f.slab_in_ring = 1; }
    if (f.np) {
        f.scr_floats = f.np * per_pair;
        // two halves of slab_chunks slots each, whole groups of four slots
        f.slab_chunks = (f.slab_in_ring ? kRing / 4 : (kScratchFloats - f.scr_floats) / (4 * kFrag)) / 8 * 4;
        // what the window arrays and the two halves leave of the K/V region: a co-occurrence table of >= 2 x positions slots per pair, for
        // windows long enough that two barriers cost less than the all-pairs scan
        f.tab_off = f.scr_floats + (f.slab_in_ring ? 0 : 2 * f.slab_chunks * 4 * kFrag);
        const int positions = 2 * ((d.Smax + 3) & ~3), words = (kScratchFloats - f.tab_off) / f.np;
        int bits = 0;
        while ((2 << (bits + 1)) <= words) ++bits;          // slots = 2^bits, two words per slot
        if (positions >= 512 && (1 << bits) >= 2 * positions) { f.tab_slots = 1 << bits; f.tab_bits = bits; }
        // the packed kernel: up to eight pairs per workgroup, counts by the scan (short windows only), the slab behind eight sets of arrays
        if (f.np == 2 && positions < 512 && 8 * per_pair + 8 * 4 * kFrag <= kScratchFloats) {
            f.scr_floats8 = 8 * per_pair;
            f.slab_chunks8 = (kScratchFloats - f.scr_floats8) / (4 * kFrag) / 8 * 4;
        }
    }
    f.total = o;
    return f;
}

bool supported(const Dims& d) {
    if (!(d.C == kC && d.H == 2 && d.Fn % 4 == 0 && d.Fe % 4 == 0 && d.Ft % 4 == 0 && d.Fn >= 16 && d.Fe >= 16 && d.Ft >= 16 &&
          d.Fn <= 512 && d.NL <= DYGNN_MAX_LAYERS && d.Tmax <= 128 && (kLdsMisc + kMiscFloats + 2 * d.Ft) * 4 <= kLdsBytes)) return false;
    // k/50 multiply-shift range; the window arrays must fit the K/V region (make_layout3 decides how)
    if (!(d.P * kC < 12000)) return false;
    const int per_pair = 5 * 2 * ((d.Smax + 3) & ~3);
    return per_pair <= kScratchFloats;
}

size_t packed_floats(const Dims& d) { return supported(d) ? make_layout3(d).total : 0; }

static int pack_vec(const float* src, int n_valid, int src_off, float* dst, int dst_off, int n_total, hipStream_t s) {
    hipLaunchKernelGGL(k_pack_vec3, dim3((n_total + 255) / 256), dim3(256), 0, s, src, n_valid, src_off, dst, dst_off, n_total);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

// reuse_desc: the weights changed IN PLACE since the last full pack into this buffer (same addresses): the fragment descriptor table that
// pack left in the buffer is still right, so only the gather kernels run — no host work, no synchronisation (one optimizer step = one repack)
int pack(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, float* packed, hipStream_t s, bool reuse_desc, bool training) {
    const PackLayout3 f = make_layout3(d);
    float* base = packed + pl.fused3;
    if (!reuse_desc) DYGNN_HIP(hipMemsetAsync(base, 0, f.total * sizeof(float), s));
    hipLaunchKernelGGL(k_pack_bias4, dim3(1), dim3(256), 0, s, w->proj_node_b, w->proj_edge_b, w->proj_time_b, w->proj_cooc_b, base + f.bias_x);
    DYGNN_LAUNCH_CHECK();
    // inference only (a training repack leaves them stale, like the other inference sections, until the next full refresh)
    if (!training) {
        const dygnn_encoder_layer_weights& L0 = w->layers[0];
        hipLaunchKernelGGL(k_pack_qkv0_const, dim3((2 * kQkvTiles * 64 + 255) / 256), dim3(256), 0, s, L0.in_proj_weight, L0.norm0_weight, L0.norm0_bias,
                           base + f.bias_x, base + f.qkv0c);
        DYGNN_LAUNCH_CHECK();
    }
    if (reuse_desc) {
        // table order (as laid down by the full pack below): stream | aux | proj | NL x FFN backward | NL x attention backward | pooled stream | W2
        PackRanges r{};
        int64_t o = 0;
        auto range = [&](int64_t nfr, float* dst) { r.start[r.n] = o; r.dst[r.n] = dst; ++r.n; o += nfr; };
        range(f.nfrag, base + f.stream); range(f.naux, base + f.aux); range(f.nproj, base + f.proj);
        for (int l = 0; l < d.NL; ++l) range(kBwdFfnFrags, base + f.bwd[l]);
        for (int l = 0; l < d.NL; ++l) range(f.bwa_frags, base + f.bwa[l]);
        range(f.nfrag_p, base + f.stream_p); range(kW2Frags, base + f.w2);
        r.start[r.n] = o;
        hipLaunchKernelGGL(k_pack_ranges, dim3((unsigned)ceil_div(o * kFrag, 256)), dim3(256), 0, s, reinterpret_cast<const FragDesc*>(base + f.desc), r);
        DYGNN_LAUNCH_CHECK();
        return DYGNN_OK;
    }
    // the GELU table does not depend on the weights: written here, behind the memset of a full pack, and left alone by every repack that
    // reuses the descriptors.  (One host copy per process: the asynchronous copy may read it after this call has returned.)
    static const std::vector<float> gelu_tab = [] { std::vector<float> t(kGeluTabFloats); gelu_table_fill(t.data()); return t; }();
    DYGNN_HIP(hipMemcpyAsync(base + f.gelu, gelu_tab.data(), kGeluTabFloats * sizeof(float), hipMemcpyHostToDevice, s));
    StreamBuilder sb;
    int nchunk[4];
    build_stream(d, w, sb, nchunk);
    if ((int64_t)sb.frags.size() != f.nfrag) { set_error("pack: stream builder mismatch"); return DYGNN_E_INVALID; }
    StreamBuilder aux;
    build_aux(d, w, aux);
    if ((int64_t)aux.frags.size() != f.naux) { set_error("pack: aux builder mismatch"); return DYGNN_E_INVALID; }
    FragDesc* ddesc = reinterpret_cast<FragDesc*>(base + f.desc);
    DYGNN_HIP(hipMemcpyAsync(ddesc, sb.frags.data(), sb.frags.size() * sizeof(FragDesc), hipMemcpyHostToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(ddesc + f.nfrag, aux.frags.data(), aux.frags.size() * sizeof(FragDesc), hipMemcpyHostToDevice, s));
    StreamBuilder pj;
    build_proj(d, w, pj);
    if ((int64_t)pj.frags.size() != f.nproj) { set_error("pack: projection builder mismatch"); return DYGNN_E_INVALID; }
    DYGNN_HIP(hipMemcpyAsync(ddesc + f.nfrag + f.naux, pj.frags.data(), pj.frags.size() * sizeof(FragDesc), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(f.nproj * kFrag, 256)), dim3(256), 0, s, ddesc + f.nfrag + f.naux, f.nproj,
                       base + f.proj);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(f.nfrag * kFrag, 256)), dim3(256), 0, s, ddesc, f.nfrag, base + f.stream);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(f.naux * kFrag, 256)), dim3(256), 0, s, ddesc + f.nfrag, f.naux, base + f.aux);
    DYGNN_LAUNCH_CHECK();
    std::vector<FragDesc> bw;
    for (int l = 0; l < d.NL; ++l) {
        StreamBuilder sbb;
        build_bwd_ffn(w->layers[l], sbb);
        if ((int64_t)sbb.frags.size() != kBwdFfnFrags) { set_error("pack: backward stream builder mismatch"); return DYGNN_E_INVALID; }
        bw.insert(bw.end(), sbb.frags.begin(), sbb.frags.end());
    }
    for (int l = 0; l < d.NL; ++l) {
        StreamBuilder sba;
        build_bwd_attn(w->layers[l], sba);
        if ((int64_t)sba.frags.size() != f.bwa_frags) { set_error("pack: attention backward stream builder mismatch"); return DYGNN_E_INVALID; }
        bw.insert(bw.end(), sba.frags.begin(), sba.frags.end());
    }
    FragDesc* bdesc = ddesc + f.nfrag + f.naux + f.nproj;
    DYGNN_HIP(hipMemcpyAsync(bdesc, bw.data(), bw.size() * sizeof(FragDesc), hipMemcpyHostToDevice, s));
    for (int l = 0; l < d.NL; ++l) {
        hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(kBwdFfnFrags * kFrag, 256)), dim3(256), 0, s, bdesc + l * kBwdFfnFrags, kBwdFfnFrags, base + f.bwd[l]);
        DYGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(f.bwa_frags * kFrag, 256)), dim3(256), 0, s, bdesc + d.NL * kBwdFfnFrags + l * f.bwa_frags, f.bwa_frags,
                           base + f.bwa[l]);
        DYGNN_LAUNCH_CHECK();
    }
    StreamBuilder sp;
    build_stream(d, w, sp, nchunk, true);
    if ((int64_t)sp.frags.size() != f.nfrag_p) { set_error("pack: pooled stream builder mismatch"); return DYGNN_E_INVALID; }
    StreamBuilder sw;
    build_w2(d, w, sw);
    FragDesc* pdesc = bdesc + (int64_t)d.NL * (kBwdFfnFrags + f.bwa_frags);
    DYGNN_HIP(hipMemcpyAsync(pdesc, sp.frags.data(), sp.frags.size() * sizeof(FragDesc), hipMemcpyHostToDevice, s));
    DYGNN_HIP(hipMemcpyAsync(pdesc + f.nfrag_p, sw.frags.data(), sw.frags.size() * sizeof(FragDesc), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(f.nfrag_p * kFrag, 256)), dim3(256), 0, s, pdesc, f.nfrag_p, base + f.stream_p);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_pack_stream, dim3((unsigned)ceil_div(kW2Frags * kFrag, 256)), dim3(256), 0, s, pdesc + f.nfrag_p, kW2Frags, base + f.w2);
    DYGNN_LAUNCH_CHECK();
    DYGNN_HIP(hipStreamSynchronize(s));     // the descriptor tables are copied from this call's host vectors
    return DYGNN_OK;
}

}  // namespace v3

bool fused3_supported(const Dims& d) { return v3::supported(d); }
size_t fused3_packed_floats(const Dims& d) { return v3::packed_floats(d); }
int pack_fused3(const Dims& d, const PackedLayout& pl, const dygnn_dygformer_weights* w, float* packed, hipStream_t s, bool reuse_desc, bool training) {
    return v3::pack(d, pl, w, packed, s, reuse_desc, training);
}

}  // namespace dygnn
