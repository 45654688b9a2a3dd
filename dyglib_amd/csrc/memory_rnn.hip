// JODIE (reference models/MemoryModel.py with model_name == 'JODIE'): nn.RNNCell memory update + time-projection embedding.  gfx950 only.
//
// A step is at most three launches:
//   1. chain::pack_rnn     the two RNNCell matrices into MFMA operand fragments (tgat_chain.h: the call takes raw state_dict pointers)
//   2. k_rnn_rows          one row per root [src ; dst]: gathers the root's pending message and stored memory into LDS, runs both products
//                          on the fragment streams of the chain kernels (chain_stream.h), tanh, then the epilogue: rows without a pending
//                          message take the stored memory and last-update time, the others the cell output and the message's time; the
//                          embedding mem * (1 + w * delta + b) goes to the caller, (updated memory, last update, pending flag) to the
//                          per-row scratch of the commit
//   3. k_jodie_commit      positive pairs only: persists the updated memories / last-update times and stores the new raw messages, from
//                          the per-row scratch alone
// DyRep (tgn.hip: dyrep_forward_impl) uses the same row kernel without the projection for the rows it returns, k_rnn_list (the cell over
// TGN's node lists, row count on the device) under its attention, and the same commit with the attention rows as the other endpoint's part.
// The reference updates all num_nodes memories on every call (MemoryModel.py:108-109) and reads the roots' rows; here a root row is
// computed where it is read, once per occurrence: a row's value is a fixed sequence of operations on its own message and memory (the
// chain kernels' property), so duplicates carry the same bits and nothing of size [num_nodes] is allocated or touched.
#include "memory_rnn.h"
#include "tgn.h"
#include "chain_stream.h"

namespace dygnn {
namespace chain {

constexpr int kRnnSlices = 2;

// ---- what the two forms of the cell share ---------------------------------------------------------------------------------------------------
// The rows of a block into LDS: wave w owns rows w, w + 8, ...; all its rows' float4 pieces are in flight together.  take_msg[r]: the node's
// pending message row (else zeros); valid[r]: its stored memory row (else zeros).
template <int MT>
struct RnnBlock {
    static constexpr int R = 4 * MT, RW = (R + kWaves - 1) / kWaves;
    __device__ static __forceinline__ void gather(const float* __restrict__ msg, const float* __restrict__ M, const int64_t (&node)[RW], const bool (&take_msg)[RW],
                                                  const bool (&valid)[RW], int Dm, int Fn, int ldm, int ldh, float* am, float* ah, int wave, int lane) {
        for (int x = lane; x < (ldm >> 2); x += 64) {
            f4 v[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) v[r] = (take_msg[r] && 4 * x < Dm) ? *reinterpret_cast<const f4*>(msg + node[r] * Dm + 4 * x) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RW; ++r)
                if (wave + kWaves * r < R) *reinterpret_cast<f4*>(am + (wave + kWaves * r) * ldm + 4 * x) = v[r];
        }
        for (int x = lane; x < (ldh >> 2); x += 64) {
            f4 v[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) v[r] = (valid[r] && 4 * x < Fn) ? *reinterpret_cast<const f4*>(M + node[r] * Fn + 4 * x) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r = 0; r < RW; ++r)
                if (wave + kWaves * r < R) *reinterpret_cast<f4*>(ah + (wave + kWaves * r) * ldh + 4 * x) = v[r];
        }
    }
    // gi = W_ih m and gh = W_hh h for the slice's tiles (si: the W_ih stream, started before the gather); ends with the barrier behind them
    template <class S, class TM>
    __device__ static __forceinline__ void products(S& si, const f4* pk, uint32_t off_hh, int nft, int Fn, TM tmap, const float* am, const float* ah, float* gi,
                                                    float* gh, int ldm, int ldh, int ldg, int wave, int lane) {
        const int j = lane & 3, ks = (lane >> 2) & 3, ng = lane >> 4;
        auto sh = wstream(pk + (size_t)off_hh * 64, nft, (Fn + 15) >> 4, kWaves - 1 - wave, lane, tmap);      // waves in reverse: evens the odd tile out
        si.template run<MT>(ldm, [&](int) { return am; }, [&](int t, const f4 (&acc)[MT]) {
            if (ks == 0) {
#pragma unroll
                for (int m = 0; m < MT; ++m) *reinterpret_cast<f4*>(gi + (4 * m + j) * ldg + 16 * t + 4 * ng) = acc[m];
            }
        });
        sh.template run<MT>(ldh, [&](int) { return ah; }, [&](int t, const f4 (&acc)[MT]) {
            if (ks == 0) {
#pragma unroll
                for (int m = 0; m < MT; ++m) *reinterpret_cast<f4*>(gh + (4 * m + j) * ldg + 16 * t + 4 * ng) = acc[m];
            }
        });
        __syncthreads();
    }
    // nn.RNNCell's output element: tanh((W_ih m + b_ih) + (W_hh h + b_hh)), one expression for both forms (a node's bits are the same in either)
    __device__ static __forceinline__ float cell(float gi, float gh, float b_ih, float b_hh) { return tanhf((gi + b_ih) + (gh + b_hh)); }
};

// grid = (row blocks, slices): slice s of a row block owns the memory dims f in [16 ft0, 16 ft1), so the slices share nothing but the
// gathered rows and a row block's weight stream is split over the slices' CUs.  A block none of whose rows has a pending message skips
// both products (their result would not be read).
template <int MT>
__global__ __launch_bounds__(kThreads) void k_rnn_rows(const RnnRowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int R = 4 * MT;
    const int64_t B = a.B;
    const int Dm = a.Dm, Fn = a.Fn;
    const int ntf = (Fn + 15) >> 4, per = (ntf + (int)gridDim.y - 1) / (int)gridDim.y;
    const int ft0 = blockIdx.y * per, ft1 = ft0 + per < ntf ? ft0 + per : ntf, nft = ft1 - ft0;
    if (nft <= 0) return;
    const int ldm = pad_ld(Dm), ldh = pad_ld(Fn), ldg = per * 16;
    float* am = lds;                  // [R][ldm] pending message rows (zero: none)
    float* ah = am + R * ldm;         // [R][ldh] stored memory rows
    float* gi = ah + R * ldh;         // [R][ldg] W_ih m, columns of the slice
    float* gh = gi + R * ldg;         // [R][ldg] W_hh h
    __shared__ int64_t s_node[R];     // -1: a row that is not computed (an id outside the tables: the host API raises IndexError for those)
    __shared__ int32_t s_pend[R];
    const f4* pk = reinterpret_cast<const f4*>(a.pk);
    auto tmap = [=](int t) { return ft0 + t; };
    const int f_lo = 16 * ft0, f_hi = 16 * ft1 < Fn ? 16 * ft1 : Fn, fw = f_hi - f_lo;
    const int64_t r0 = (int64_t)blockIdx.x * R;
    auto si = wstream(pk + (size_t)a.off_ih * 64, nft, (Dm + 15) >> 4, wave, lane, tmap);
    int any = 0;
    {   // the rows: a wave's node ids and flags first, then float4 row pieces of all its rows in flight together
        constexpr int RW = (R + kWaves - 1) / kWaves;
        int64_t node[RW]; bool valid[RW], pend[RW];
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const int rr = wave + kWaves * r;
            const int64_t row = r0 + rr, i = row < B ? row : row - B;
            int64_t id = -1;
            if (rr < R && row < 2 * B) id = row < B ? a.src[i] : a.dst[i];
            valid[r] = id >= 0 && id < a.N;
            node[r] = valid[r] ? id : 0;
            pend[r] = valid[r] && a.has_msg[node[r]] != 0;
            any |= pend[r] ? 1 : 0;
            if (rr < R && lane == 0) { s_node[rr] = valid[r] ? id : -1; s_pend[rr] = pend[r] ? 1 : 0; }
        }
        RnnBlock<MT>::gather(a.msg, a.M, node, pend, valid, Dm, Fn, ldm, ldh, am, ah, wave, lane);
    }
    any = __syncthreads_or(any);      // (also the barrier behind the gathers)
    if (any) RnnBlock<MT>::products(si, pk, a.off_hh, nft, Fn, tmap, am, ah, gi, gh, ldm, ldh, ldg, wave, lane);
    // nn.RNNCell: tanh((W_ih m + b_ih) + (W_hh h + b_hh)) for a row with a pending message, the stored memory otherwise
    // (MemoryModel.py:461-487); then JODIE's projection (:111-124, :543), every operation in float32 and in the reference's order
    for (int idx = threadIdx.x; idx < R * fw; idx += kThreads) {
        const int rr = idx / fw, fl = idx - rr * fw, f = f_lo + fl;
        const int64_t row = r0 + rr;
        if (row >= 2 * B) continue;
        const int64_t node = s_node[rr];
        const int64_t i = row < B ? row : row - B;
        float* o = a.out + row * Fn + f;
        if (node < 0) { *o = 0.f; a.upd[row * Fn + f] = 0.f; if (fl == 0 && blockIdx.y == 0) { a.lu[row] = 0.f; a.pend[row] = 0; } continue; }
        const bool pend = s_pend[rr] != 0;
        float m = ah[rr * ldh + f];
        if (pend) m = RnnBlock<MT>::cell(gi[rr * ldg + fl], gh[rr * ldg + fl], a.b_ih[f], a.b_hh[f]);
        const float u = pend ? (float)a.msg_t[node] : a.U[node];
        float e = m;                                                       // DyRep returns the updated memory itself (MemoryModel.py:163-166)
        if (a.proj_w) {
            const int role = row < B ? 0 : 1;
            const float delta = (((float)a.times[i] - u) - a.mean[role]) / a.stdv[role];
            e = m * (1.0f + fmaf(delta, a.proj_w[f], a.proj_b[f]));      // nn.Linear(1, Fn): one multiply-add, as the time encoder's
        }
        *o = e;
        a.upd[row * Fn + f] = m;
        if (fl == 0 && blockIdx.y == 0) { a.lu[row] = u; a.pend[row] = pend ? 1 : 0; }
    }
}

// End of a positive call, one launch, the form of k_tgn_commit (tgn.hip): entry e = role * n_pos + i (role 0 = source); messages are stored
// source role first, then destination role, and only a node's LAST stored message is ever read (MemoryModel.py:284-291), so the last entry
// of a node does the work for that node and the others exit.  Everything read here is the row kernel's per-row scratch (rows i and B + i
// of the pair) and the call's inputs: no workgroup reads a state row that another one writes.
__global__ __launch_bounds__(256) void k_jodie_commit(const int64_t* __restrict__ src, const int64_t* __restrict__ dst, const double* __restrict__ times,
                                                        const int64_t* __restrict__ eids, int64_t n_pos, int64_t B, const float* __restrict__ upd,
                                                        const float* __restrict__ lu, const int32_t* __restrict__ pendr,
                                                        const float* __restrict__ other_src, const float* __restrict__ other_dst, float* __restrict__ M,
                                                        float* __restrict__ U, const float* __restrict__ edge_feat, const float* __restrict__ tw,
                                                        const float* __restrict__ tb, int Fn, int Fe, int Ft, float* __restrict__ msg,
                                                        double* __restrict__ msg_t, int32_t* __restrict__ has_msg, int64_t N) {
    const int64_t e = blockIdx.x;
    const bool role = e >= n_pos;
    const int64_t i = role ? e - n_pos : e;
    const int64_t node = role ? dst[i] : src[i];
    const int64_t o = role ? src[i] : dst[i];
    if (node < 0 || node >= N || o < 0 || o >= N) return;      // never index the state tables out of range (the host API raises IndexError for such ids)
    int later = 0;
    for (int64_t e2 = e + 1 + threadIdx.x; e2 < 2 * n_pos; e2 += blockDim.x) {
        const int64_t i2 = e2 >= n_pos ? e2 - n_pos : e2;
        const int64_t n2 = e2 >= n_pos ? dst[i2] : src[i2], o2 = e2 >= n_pos ? src[i2] : dst[i2];
        later |= (n2 == node && o2 >= 0 && o2 < N) ? 1 : 0;
    }
    if (__syncthreads_or(later)) return;
    const int64_t row = role ? B + i : i, orow = role ? i : B + i;
    const bool pend = pendr[row] != 0;
    const float* mn = upd + row * Fn;                                // the node's updated memory (MemoryModel.py:142-145 persists exactly this)
    // the other endpoint's updated memory (:229, read after the persist); DyRep: its attention embedding, row i of this pair (:225-227)
    const float* mo = other_src ? (role ? other_src : other_dst) + i * Fn : upd + orow * Fn;
    const float u = lu[row];                                         // last-update time after the persist (:447-459)
    const int D = 2 * Fn + Ft + Fe;
    const float dt = (float)times[i] - u;                            // float32 - float32 (MemoryModel.py:232-233)
    float* m = msg + node * D;
    for (int f = threadIdx.x; f < D; f += blockDim.x) {
        float v;
        if (f < Fn) v = mn[f];
        else if (f < 2 * Fn) v = mo[f - Fn];
        else if (f < 2 * Fn + Ft) v = cosf(fmaf(dt, tw[f - 2 * Fn], tb[f - 2 * Fn]));
        else v = edge_feat[(size_t)eids[i] * Fe + (f - 2 * Fn - Ft)];
        m[f] = v;
        if (pend && f < Fn) M[node * Fn + f] = v;                    // persist
    }
    if (threadIdx.x == 0) {
        if (pend) U[node] = u;
        msg_t[node] = times[i];
        has_msg[node] = 1;
    }
}

// The list form (DyRep: the updated memories the attention reads, over TGN's node lists): k_tgn_gru_chain (tgat_chain.hip) with one gate.
// grid = (row-block workgroups + kRnnPlainBlocks, slices); row r = node list[r], r < *count read on the device; the workgroups behind the row
// blocks (slice 0 only) write feat0 = memory + raw for the nodes of list2 (no pending message).  A row's bits are those of k_rnn_rows for
// the same node: the same streams, the same epilogue expression.
constexpr int kRnnPlainBlocks = 64;
template <int MT>
__global__ __launch_bounds__(kThreads) void k_rnn_list(const GruArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int R = 4 * MT;
    const int64_t cnt = *a.count;
    const int64_t nblk = (cnt + R - 1) / R;
    const int64_t nrow = (int64_t)gridDim.x - kRnnPlainBlocks;
    const int Dm = a.Dm, Fn = a.Fn;
    if ((int64_t)blockIdx.x >= (nblk < nrow ? nblk : nrow)) {
        if (blockIdx.y != 0) return;
        const int64_t first = nblk < nrow ? nblk : nrow;
        const int64_t cnt2 = *a.count2, nb = (int64_t)gridDim.x - first, F4 = Fn >> 2;
        for (int64_t r = ((int64_t)blockIdx.x - first) * kWaves + wave; r < cnt2; r += nb * kWaves) {
            const int64_t node = a.list2[r];
            for (int x = lane; x < F4; x += 64) {
                const f4 m = *reinterpret_cast<const f4*>(a.M + node * Fn + 4 * x), w = *reinterpret_cast<const f4*>(a.raw + node * Fn + 4 * x);
                *reinterpret_cast<f4*>(a.feat0 + node * Fn + 4 * x) = f4{m.x + w.x, m.y + w.y, m.z + w.z, m.w + w.w};      // MemoryModel.py:609
            }
        }
        return;
    }
    const int ntf = (Fn + 15) >> 4, per = (ntf + (int)gridDim.y - 1) / (int)gridDim.y;
    const int ft0 = blockIdx.y * per, ft1 = ft0 + per < ntf ? ft0 + per : ntf, nft = ft1 - ft0;
    if (nft <= 0) return;
    const int ldm = pad_ld(Dm), ldh = pad_ld(Fn), ldg = per * 16;
    float* am = lds;
    float* ah = am + R * ldm;
    float* gi = ah + R * ldh;
    float* gh = gi + R * ldg;
    const f4* pk = reinterpret_cast<const f4*>(a.pk);
    auto tmap = [=](int t) { return ft0 + t; };
    const int f_lo = 16 * ft0, f_hi = 16 * ft1 < Fn ? 16 * ft1 : Fn, fw = f_hi - f_lo;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += nrow) {      // (one round unless the list is longer than the grid's row blocks)
        const int64_t r0 = blk * R;
        auto si = wstream(pk + (size_t)a.off_ih * 64, nft, (Dm + 15) >> 4, wave, lane, tmap);
        {
            constexpr int RW = (R + kWaves - 1) / kWaves;
            int64_t node[RW]; bool valid[RW];
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                const int rr = wave + kWaves * r;
                valid[r] = rr < R && r0 + rr < cnt;
                node[r] = valid[r] ? a.list[r0 + rr] : 0;
            }
            RnnBlock<MT>::gather(a.msg, a.M, node, valid, valid, Dm, Fn, ldm, ldh, am, ah, wave, lane);
        }
        __syncthreads();
        RnnBlock<MT>::products(si, pk, a.off_hh, nft, Fn, tmap, am, ah, gi, gh, ldm, ldh, ldg, wave, lane);
        for (int idx = threadIdx.x; idx < R * fw; idx += kThreads) {
            const int rr = idx / fw, fl = idx - rr * fw, f = f_lo + fl;
            if (r0 + rr >= cnt) continue;
            const int64_t node = a.list[r0 + rr];
            const float hn = RnnBlock<MT>::cell(gi[rr * ldg + fl], gh[rr * ldg + fl], a.b_ih[f], a.b_hh[f]);
            a.Mnew[node * Fn + f] = hn;
            a.feat0[node * Fn + f] = hn + a.raw[node * Fn + f];
        }
        __syncthreads();
    }
}

static int rnn_slices() { return env_slices("DYGNN_RNN_SLICES", kRnnSlices); }
static size_t rnn_lds(int Dm, int Fn, int MT) {      // dynamic bytes; rnn_lds_total adds k_rnn_rows' static per-row arrays (16 bytes per row): what kLdsMax bounds
    const int per = ((Fn + 15) / 16 + rnn_slices() - 1) / rnn_slices();
    return (size_t)4 * MT * (pad_ld(Dm) + pad_ld(Fn) + 2 * per * 16) * sizeof(float);
}
static size_t rnn_lds_total(int Dm, int Fn, int MT) { return rnn_lds(Dm, Fn, MT) + (size_t)4 * MT * 16; }

template <int MT>
static int launch_rnn_rows_mt(hipStream_t s, const RnnRowArgs& a) {
    const size_t bytes = rnn_lds(a.Dm, a.Fn, MT);
    if (int rc = set_lds(k_rnn_rows<MT>, bytes)) return rc;
    hipLaunchKernelGGL(k_rnn_rows<MT>, dim3((unsigned)ceil_div(2 * a.B, 4 * MT), rnn_slices()), dim3(kThreads), bytes, s, a);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
// rows per workgroup 4 MT (DYGNN_RNN_MT) and slices (DYGNN_RNN_SLICES) as for the GRU kernel: a row's bits do not depend on either
int launch_rnn_rows(hipStream_t s, const RnnRowArgs& a) {
    if (a.B == 0) return DYGNN_OK;
    int MT = env_mt("DYGNN_RNN_MT", pick_mt(2 * a.B));
    if (MT > 4) MT = 4;
    while (MT > 1 && rnn_lds_total(a.Dm, a.Fn, MT) > kLdsMax) MT >>= 1;
    return MT == 4 ? launch_rnn_rows_mt<4>(s, a) : MT == 2 ? launch_rnn_rows_mt<2>(s, a) : launch_rnn_rows_mt<1>(s, a);
}

template <int MT>
static int launch_rnn_list_mt(hipStream_t s, const GruArgs& a) {
    const size_t bytes = rnn_lds(a.Dm, a.Fn, MT);
    if (int rc = set_lds(k_rnn_list<MT>, bytes)) return rc;
    const int64_t blocks = ceil_div(a.max_rows, 4 * MT);      // the list length is only known on the device: a bounded grid walks it
    hipLaunchKernelGGL(k_rnn_list<MT>, dim3((unsigned)(blocks < 192 ? blocks : 192) + kRnnPlainBlocks, rnn_slices()), dim3(kThreads), bytes, s, a);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}
int launch_rnn_list(hipStream_t s, const GruArgs& a) {
    if (a.max_rows == 0) return DYGNN_OK;
    int MT = env_mt("DYGNN_RNN_MT", pick_mt(a.max_rows / 8));      // the list is a fraction of the level-0 set
    if (MT > 4) MT = 4;
    while (MT > 1 && rnn_lds_total(a.Dm, a.Fn, MT) > kLdsMax) MT >>= 1;
    return MT == 4 ? launch_rnn_list_mt<4>(s, a) : MT == 2 ? launch_rnn_list_mt<2>(s, a) : launch_rnn_list_mt<1>(s, a);
}

int memory_commit(hipStream_t s, const int64_t* src, const int64_t* dst, const double* times, const int64_t* edge_ids, int64_t n_pos, int64_t B,
                  const float* upd, const float* lu, const int32_t* pend, const float* other_src, const float* other_dst, const dygnn_tgn_state* st,
                  const float* edge_feat, const float* tw, const float* tb, int Fn, int Fe, int Ft) {
    if (n_pos == 0) return DYGNN_OK;
    hipLaunchKernelGGL(k_jodie_commit, dim3((unsigned)(2 * n_pos)), dim3(256), 0, s, src, dst, times, edge_ids, n_pos, B, upd, lu, pend, other_src, other_dst,
                       st->memory, st->last_update, edge_feat, tw, tb, Fn, Fe, Ft, st->msg, st->msg_time, st->has_msg, st->num_nodes);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

struct JodiePlan { size_t pack, upd, lu, pend, total; };
static JodiePlan make_jodie_plan(int Fn, int Dm, int64_t B) {
    JodiePlan p{};
    Carve ws;
    p.pack = ws.take(pack_bytes(plan_pack_rnn(Fn, Dm)));
    p.upd = ws.take((size_t)2 * B * Fn * sizeof(float));
    p.lu = ws.take((size_t)2 * B * sizeof(float));
    p.pend = ws.take((size_t)2 * B * sizeof(int32_t));
    p.total = ws.o;
    return p;
}

int check_rnn_dims(const char* who, int Fn, int Fe, int Ft) {
    if (Fn % 4) { set_error("%s: node_feat_dim = %d is not a multiple of 4 (the row-block kernel reads float4 rows)", who, Fn); return DYGNN_E_UNSUPPORTED; }
    if (Fe % 4) { set_error("%s: edge_feat_dim = %d is not a multiple of 4 (the row-block kernel reads float4 rows)", who, Fe); return DYGNN_E_UNSUPPORTED; }
    if (Ft % 4) { set_error("%s: time_feat_dim = %d is not a multiple of 4 (the row-block kernel reads float4 rows)", who, Ft); return DYGNN_E_UNSUPPORTED; }
    // a four-row block with ONE slice (the most LDS any slice count takes), its static per-row arrays included
    if (Fn > 4096 || Fe > 4096 || Ft > 4096 || (size_t)4 * (pad_ld(2 * Fn + Ft + Fe) + pad_ld(Fn) + 2 * r16(Fn)) * sizeof(float) + 64 > kLdsMax) {
        set_error("%s: message dim 2 * %d + %d + %d = %d: a four-row block does not fit the LDS", who, Fn, Ft, Fe, 2 * Fn + Ft + Fe);
        return DYGNN_E_UNSUPPORTED;
    }
    return DYGNN_OK;
}

static int check_jodie(const dygnn_tgat_config* c) {
    DYGNN_REQUIRE(c != nullptr, "jodie: config is NULL");
    DYGNN_REQUIRE(c->node_feat_dim > 0 && c->edge_feat_dim > 0 && c->time_feat_dim > 0, "jodie: feature dims must be positive");
    return check_rnn_dims("jodie", c->node_feat_dim, c->edge_feat_dim, c->time_feat_dim);
}

}  // namespace chain
}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_jodie_workspace_bytes(const dygnn_tgat_config* cfg, int64_t num_nodes, int64_t batch) {
    if (chain::check_jodie(cfg) != DYGNN_OK) return 0;
    if (batch < 0 || num_nodes < 1) { set_error("jodie: batch must be >= 0 and num_nodes >= 1"); return 0; }
    return chain::make_jodie_plan(cfg->node_feat_dim, 2 * cfg->node_feat_dim + cfg->time_feat_dim + cfg->edge_feat_dim, batch).total;
}

extern "C" int dygnn_jodie_forward_step(const dygnn_tgat_config* cfg, const float* time_w, const float* time_b, const dygnn_rnn_weights* rnn,
                                        const float* proj_w, const float* proj_b, double src_mean, double src_std, double dst_mean, double dst_std,
                                        const float* edge_feat, const dygnn_tgn_state* st, const int64_t* src, const int64_t* dst, const double* times,
                                        const int64_t* edge_ids, int64_t batch, int64_t n_pos, float* out_src, float* out_dst, void* workspace,
                                        size_t workspace_bytes, dygnn_stream_t stream) {
    if (int rc = chain::check_jodie(cfg)) return rc;
    DYGNN_REQUIRE(n_pos >= 0 && n_pos <= batch, "jodie: n_positive must be in [0, batch]");
    DYGNN_REQUIRE(time_w && time_b && proj_w && proj_b, "jodie: null weights");
    if (int rc = check_cell(rnn, "jodie", "RNN weights")) return rc;
    if (int rc = check_state(st, "jodie")) return rc;
    DYGNN_REQUIRE(batch >= 0 && edge_feat && workspace, "jodie: bad arguments");
    DYGNN_REQUIRE(batch == 0 || (src && dst && times && out_src && out_dst), "jodie: null pointer");
    DYGNN_REQUIRE(n_pos == 0 || edge_ids != nullptr, "jodie: edge_ids required for positive edges");   // MemoryModel.py:140
    DYGNN_REQUIRE(batch == 0 || out_dst == out_src + (size_t)batch * cfg->node_feat_dim, "jodie: out_dst must follow out_src (one [2, batch, dim] block)");
    if (batch == 0) return DYGNN_OK;
    const int Fn = cfg->node_feat_dim, Fe = cfg->edge_feat_dim, Ft = cfg->time_feat_dim, Dm = 2 * Fn + Ft + Fe;
    const chain::JodiePlan p = chain::make_jodie_plan(Fn, Dm, batch);
    if (workspace_bytes < p.total) { set_error("jodie: workspace too small (%zu < %zu bytes)", workspace_bytes, p.total); return DYGNN_E_WORKSPACE; }
    hipStream_t s = as_stream(stream);
    char* ws = static_cast<char*>(workspace);
    float* pk = reinterpret_cast<float*>(ws + p.pack);
    float* upd = reinterpret_cast<float*>(ws + p.upd);
    float* lu = reinterpret_cast<float*>(ws + p.lu);
    int32_t* pend = reinterpret_cast<int32_t*>(ws + p.pend);
    const chain::RnnPackPlan pp = chain::plan_pack_rnn(Fn, Dm);
    if (int rc = chain::pack_rnn(s, pp, Fn, Dm, rnn, pk)) return rc;
    chain::RnnRowArgs ra{src, dst, times, batch, st->num_nodes, st->msg, st->memory, st->last_update, st->msg_time, st->has_msg, pk, pp.ih, pp.hh,
                         rnn->bias_ih, rnn->bias_hh, proj_w, proj_b, {(float)src_mean, (float)dst_mean}, {(float)src_std, (float)dst_std}, out_src, upd, lu, pend, Dm, Fn};
    if (int rc = chain::launch_rnn_rows(s, ra)) return rc;
    if (n_pos == 0) return DYGNN_OK;
    // the commit of the positive pairs (MemoryModel.py:142-161): after the rows were written, so the rows of a step do not see it
    return chain::memory_commit(s, src, dst, times, edge_ids, n_pos, batch, upd, lu, pend, nullptr, nullptr, st, edge_feat, time_w, time_b, Fn, Fe, Ft);
}
