// EdgeBank (reference models/EdgeBank.py:7-121): the non-parametric link-prediction baseline.  An edge (src, dst), DIRECTED, scores 1.0 when
// its pair is "in memory" and 0.0 otherwise; the three memory modes differ in which pairs of the history count.  The reference rebuilds a
// Python set / dict over the whole history for every batch (evaluate_models_utils.py:329-341); here the history lives in a persistent
// open-addressing hash table in HBM that a batch only adds its new edges to.
//
// Table = one caller-owned buffer (dygnn_edgebank_table_bytes), capacity C = the power of two >= max(2 * max_edges, 8):
//   [0, 64)            Header: distinct pairs D, image of the largest time, the window record (S, start), error flags
//   [64, 2112)         kStatBlocks float64 partial sums of the window statistic
//   count     u32[C]   occurrences of the pair                          atomicAdd
//   last_pos  u32[C]   largest history position of the pair             atomicMax
//   max_time  u64[C]   image of the pair's largest time                 atomicMax
//   keys      u64[C]   (src << 32) | dst, ~0 = empty                    atomicCAS
//   first_pos u32[C]   smallest history position of the pair            atomicMin
// (the first three arrays start as zero bytes, the last two as 0xff bytes: reset is two memsets).
//
// Hash: home slot = mix(key) & (C - 1) with MurmurHash3's 64-bit finaliser
//   mix(k): k ^= k >> 33; k *= 0xff51afd7ed558ccd; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53; k ^= k >> 33
// and linear probing (slot + 1) & (C - 1): probes wrap at the table's end and stop at an empty slot.
//
// Reproducible state.  Plain concurrent linear probing gives colliding keys whichever slots the race hands them.  Here one insert call is two
// kernels.  k_claim places the keys the table does not hold yet, as ordered linear probing (Amble & Knuth 1974): a carried key that meets a
// smaller key PLACED BY THE SAME CALL swaps with it (64-bit CAS) and carries the smaller one on; keys of earlier calls (count != 0; the counts
// are not written during k_claim) never move.  Every key then sits at the first slot from its home that holds neither an earlier call's key
// nor a larger key of this call, a property exactly one layout has, so the layout is a function of (layout before, set of new keys), not of
// the schedule.  All slots between a carried key's home and the thread's position are occupied, so a thread takes at most C / 2 + 1 steps.
// k_update then finds each edge's slot (keys are stable now) and applies its record updates, all of them commutative integer atomics.
// Nothing is a floating-point atomic; the window statistic is summed slot by slot in a fixed order.  Table bytes and scores are therefore
// bit-identical from run to run.
//
// Guards: an id outside [0, 2^31) is never hashed or stored (insert: flag kFlagBadId; query: score 0), a probe loop ends after C steps
// (kFlagFull / kFlagLost), positions index `times` only below the inserted length.  The flags are word 8 (int32) of the buffer.
#include "common.h"

namespace dygnn {
namespace {

constexpr int kBlock = 256;
constexpr int kStatBlocks = 256;
constexpr unsigned long long kEmpty = ~0ull;
constexpr size_t kHeaderBytes = 64, kPartialBytes = kStatBlocks * sizeof(double);
constexpr int64_t kMaxEdges = 1ll << 30;                 // positions are u32 and C = 2 * max_edges <= 2^31
constexpr unsigned kFlagBadId = 1, kFlagFull = 2, kFlagLost = 4;

struct Header {
    unsigned long long distinct;        // D
    unsigned long long end_image;       // image of max(times)
    double S;                           // repeat_interval: sum over repeated pairs of their mean interval
    double start;                       // repeat_interval: end - S / D
    unsigned int flags;
    unsigned int pad;
    unsigned long long reserved[3];
};
static_assert(sizeof(Header) == kHeaderBytes, "Header is 64 bytes");

struct Table {
    Header* hdr;
    double* partial;
    unsigned int* count;
    unsigned int* last_pos;
    unsigned long long* max_time;
    unsigned long long* keys;
    unsigned int* first_pos;
    unsigned long long mask;            // C - 1
};

inline int64_t capacity_for(int64_t max_edges) {
    int64_t c = 8;
    while (c < 2 * max_edges) c <<= 1;
    return c;
}
inline size_t zero_bytes(int64_t c) { return kHeaderBytes + kPartialBytes + (size_t)c * 16; }
inline size_t table_bytes(int64_t c) { return zero_bytes(c) + (size_t)c * 12; }

inline Table view(void* buffer, int64_t c) {
    char* p = static_cast<char*>(buffer);
    Table t;
    t.hdr = reinterpret_cast<Header*>(p);
    t.partial = reinterpret_cast<double*>(p + kHeaderBytes);
    p += kHeaderBytes + kPartialBytes;
    t.count = reinterpret_cast<unsigned int*>(p);
    t.last_pos = reinterpret_cast<unsigned int*>(p + (size_t)c * 4);
    t.max_time = reinterpret_cast<unsigned long long*>(p + (size_t)c * 8);
    t.keys = reinterpret_cast<unsigned long long*>(p + (size_t)c * 16);
    t.first_pos = reinterpret_cast<unsigned int*>(p + (size_t)c * 24);
    t.mask = (unsigned long long)c - 1;
    return t;
}

__host__ __device__ inline unsigned long long mix(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// order-preserving image of a double: a < b  <=>  image(a) < image(b) as unsigned (NaNs aside); every image is > 0, the reset value
__device__ inline unsigned long long time_image(double t) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(t);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double image_time(unsigned long long m) {
    return __longlong_as_double((long long)((m >> 63) ? (m & 0x7fffffffffffffffull) : ~m));
}

__device__ inline bool valid_id(int64_t v) { return v >= 0 && v < (1ll << 31); }

__device__ inline unsigned long long load_key(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Phase 1 of an insert: place the keys of positions [first, last) that the table does not hold yet (see the file comment).
__global__ __launch_bounds__(kBlock) void k_claim(Table t, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                  const double* __restrict__ times, int64_t first, int64_t last) {
    const int64_t p = first + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = p < last;
    unsigned long long placed = 0, tmax = 0;
    if (live) {
        const int64_t s = src[p], d = dst[p];
        if (!valid_id(s) || !valid_id(d)) {
            atomicOr(&t.hdr->flags, kFlagBadId);
        } else {
            tmax = time_image(times[p]);
            unsigned long long key = ((unsigned long long)s << 32) | (unsigned long long)d;
            unsigned long long slot = mix(key) & t.mask;
            unsigned long long steps = 0;
            for (;;) {
                unsigned long long cur = load_key(&t.keys[slot]);
                if (cur == key) break;
                if (cur == kEmpty) {
                    cur = atomicCAS(&t.keys[slot], kEmpty, key);
                    if (cur == kEmpty) {
                        placed = 1;
                        break;
                    }
                    if (cur == key) break;
                }
                // cur is another key.  One of this call (count still 0) that is smaller gives way.  A failed swap looks at the slot again: the
                // slot's key only ever grows, at most once per new key, so the retries end.
                if (cur < key && __hip_atomic_load(&t.count[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
                    if (atomicCAS(&t.keys[slot], cur, key) != cur) continue;
                    key = cur;
                }
                slot = (slot + 1) & t.mask;
                if (++steps > t.mask) {            // never with C >= 2 * edges; ends the walk on a table the caller overfilled
                    atomicOr(&t.hdr->flags, kFlagFull);
                    break;
                }
            }
        }
    }
    placed = wave_sum(placed);
    tmax = wave_max(tmax);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        if (placed) atomicAdd(&t.hdr->distinct, placed);
        if (tmax) atomicMax(&t.hdr->end_image, tmax);
    }
}

// slot of `key`, or -1: probes from the home slot, stops at an empty slot or after C steps
__device__ inline long long find_slot(const Table& t, unsigned long long key) {
    unsigned long long slot = mix(key) & t.mask;
    for (unsigned long long steps = 0; steps <= t.mask; ++steps) {
        const unsigned long long cur = t.keys[slot];
        if (cur == key) return (long long)slot;
        if (cur == kEmpty) return -1;
        slot = (slot + 1) & t.mask;
    }
    return -1;
}

// Phase 2 of an insert: the record updates of positions [first, last); every one commutes with every other.
__global__ __launch_bounds__(kBlock) void k_update(Table t, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                   const double* __restrict__ times, int64_t first, int64_t last) {
    const int64_t p = first + (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= last) return;
    const int64_t s = src[p], d = dst[p];
    if (!valid_id(s) || !valid_id(d)) return;
    const long long slot = find_slot(t, ((unsigned long long)s << 32) | (unsigned long long)d);
    if (slot < 0) {
        atomicOr(&t.hdr->flags, kFlagLost);
        return;
    }
    atomicAdd(&t.count[slot], 1u);
    atomicMin(&t.first_pos[slot], (unsigned int)p);
    atomicMax(&t.last_pos[slot], (unsigned int)p);
    atomicMax(&t.max_time[slot], time_image(times[p]));
}

// Window statistic, stage 1 (EdgeBank.py:56-64): S = sum over pairs with n > 1 occurrences of the mean of their consecutive time differences
// in history order = (t[last_pos] - t[first_pos]) / (n - 1).  Block b owns slots [b * chunk, (b + 1) * chunk); fixed order throughout.
__global__ __launch_bounds__(kBlock) void k_window_partial(Table t, const double* __restrict__ times, int64_t H, unsigned long long chunk) {
    __shared__ double red[kBlock / kWave];
    const unsigned long long lo = (unsigned long long)blockIdx.x * chunk;
    unsigned long long hi = lo + chunk;
    if (hi > t.mask + 1) hi = t.mask + 1;
    double acc = 0.0;
    for (unsigned long long slot = lo + threadIdx.x; slot < hi; slot += kBlock) {
        const unsigned int n = t.count[slot];
        if (n > 1) {
            const unsigned int a = t.first_pos[slot], b = t.last_pos[slot];
            if ((int64_t)a < H && (int64_t)b < H) acc += (times[b] - times[a]) / (double)(n - 1);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int k = 0; k < kBlock / kWave; ++k) sum += red[k];
        t.partial[blockIdx.x] = sum;
    }
}

// stage 2: S, and start = end - S / D (EdgeBank.py:66-68), into the header
__global__ __launch_bounds__(kWave) void k_window_final(Table t, int nblocks) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kWave) acc += t.partial[b];
    acc = wave_sum(acc);
    if (threadIdx.x == 0) {
        const double average = acc / (double)t.hdr->distinct;
        t.hdr->S = acc;
        t.hdr->start = image_time(t.hdr->end_image) - average;
    }
}

// One thread per query edge; reads only.  mode 0 unlimited, 1 repeat threshold, 2 time window (start: start_ptr[0] if given, else the
// header's for window_mode 1, else start_scalar).
__global__ __launch_bounds__(kBlock) void k_query(Table t, int mode, int window_mode, int64_t H, double start_scalar,
                                                  const double* __restrict__ start_ptr, const int64_t* __restrict__ q_src,
                                                  const int64_t* __restrict__ q_dst, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t s = q_src[i], d = q_dst[i];
    bool in_memory = false;
    if (valid_id(s) && valid_id(d)) {
        const long long slot = find_slot(t, ((unsigned long long)s << 32) | (unsigned long long)d);
        if (slot >= 0) {
            if (mode == 0) {
                in_memory = true;
            } else if (mode == 1) {               // EdgeBank.py:88-90: count >= mean count = H / D, in float64
                in_memory = (double)t.count[slot] >= (double)H / (double)t.hdr->distinct;
            } else {                              // EdgeBank.py:72: some occurrence has start <= t (<= end always holds)
                const double start = window_mode == 1 ? t.hdr->start : (start_ptr ? start_ptr[0] : start_scalar);
                in_memory = image_time(t.max_time[slot]) >= start;
            }
        }
    }
    out[i] = in_memory ? 1.f : 0.f;
}

int check_table(const dygnn_edgebank* tb, const char* who) {
    DYGNN_REQUIRE(tb, "%s: null table", who);
    DYGNN_REQUIRE(tb->buffer, "%s: null table buffer", who);
    DYGNN_REQUIRE(tb->max_edges >= 0 && tb->max_edges <= kMaxEdges, "%s: max_edges %lld outside [0, 2^30]", who, (long long)tb->max_edges);
    if (tb->buffer_bytes < table_bytes(capacity_for(tb->max_edges))) {
        set_error("%s: table buffer too small (%zu bytes for max_edges %lld)", who, tb->buffer_bytes, (long long)tb->max_edges);
        return DYGNN_E_WORKSPACE;
    }
    DYGNN_REQUIRE(tb->num_edges >= 0 && tb->num_edges <= tb->max_edges, "%s: num_edges %lld outside [0, max_edges]", who,
                  (long long)tb->num_edges);
    return DYGNN_OK;
}

int check_modes(int32_t mode, int32_t window_mode, const char* who) {
    DYGNN_REQUIRE(mode >= 0 && mode <= 2, "%s: memory mode %d is not 0 (unlimited), 1 (repeat threshold) or 2 (time window)", who, mode);
    DYGNN_REQUIRE(mode != 2 || window_mode == 0 || window_mode == 1, "%s: time window mode %d is not 0 (fixed proportion) or 1 (repeat interval)",
                  who, window_mode);
    return DYGNN_OK;
}

int launch_insert(dygnn_edgebank* tb, const int64_t* src, const int64_t* dst, const double* times, int64_t last, hipStream_t stream) {
    const int64_t first = tb->num_edges;
    if (last == first) return DYGNN_OK;
    const Table t = view(tb->buffer, capacity_for(tb->max_edges));
    const unsigned grid = (unsigned)ceil_div(last - first, kBlock);
    hipLaunchKernelGGL(k_claim, dim3(grid), dim3(kBlock), 0, stream, t, src, dst, times, first, last);
    DYGNN_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_update, dim3(grid), dim3(kBlock), 0, stream, t, src, dst, times, first, last);
    DYGNN_LAUNCH_CHECK();
    tb->num_edges = last;
    return DYGNN_OK;
}

int launch_query(const dygnn_edgebank* tb, const double* times, int32_t mode, int32_t window_mode, double start_scalar, const double* start_ptr,
                 const int64_t* q_src, const int64_t* q_dst, int64_t n, float* out, hipStream_t stream) {
    const int64_t c = capacity_for(tb->max_edges);
    const Table t = view(tb->buffer, c);
    if (mode == 2 && window_mode == 1) {
        const int nblocks = (int)(ceil_div(c, kBlock) < kStatBlocks ? ceil_div(c, kBlock) : kStatBlocks);
        const unsigned long long chunk = (unsigned long long)ceil_div(c, nblocks);
        hipLaunchKernelGGL(k_window_partial, dim3((unsigned)nblocks), dim3(kBlock), 0, stream, t, times, tb->num_edges, chunk);
        DYGNN_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_window_final, dim3(1), dim3(kWave), 0, stream, t, nblocks);
        DYGNN_LAUNCH_CHECK();
    }
    if (n == 0) return DYGNN_OK;
    hipLaunchKernelGGL(k_query, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, stream, t, (int)mode, (int)window_mode, tb->num_edges,
                       start_scalar, start_ptr, q_src, q_dst, n, out);
    DYGNN_LAUNCH_CHECK();
    return DYGNN_OK;
}

}  // namespace
}  // namespace dygnn

using namespace dygnn;

extern "C" size_t dygnn_edgebank_table_bytes(int64_t max_edges) {
    if (max_edges < 0 || max_edges > kMaxEdges) return 0;
    return table_bytes(capacity_for(max_edges));
}

extern "C" uint64_t dygnn_edgebank_home_slot(int64_t src, int64_t dst, int64_t max_edges) {
    if (max_edges < 0 || max_edges > kMaxEdges || src < 0 || src >= (1ll << 31) || dst < 0 || dst >= (1ll << 31)) return UINT64_MAX;
    return mix(((uint64_t)src << 32) | (uint64_t)dst) & ((uint64_t)capacity_for(max_edges) - 1);
}

extern "C" int dygnn_edgebank_reset(dygnn_edgebank* table_host, dygnn_stream_t stream) {
    if (int rc = check_table(table_host, "edgebank_reset")) return rc;
    const int64_t c = capacity_for(table_host->max_edges);
    char* p = static_cast<char*>(table_host->buffer);
    DYGNN_HIP(hipMemsetAsync(p, 0, zero_bytes(c), as_stream(stream)));
    DYGNN_HIP(hipMemsetAsync(p + zero_bytes(c), 0xff, (size_t)c * 12, as_stream(stream)));
    table_host->num_edges = 0;
    return DYGNN_OK;
}

extern "C" int dygnn_edgebank_insert(dygnn_edgebank* table_host, const int64_t* src, const int64_t* dst, const double* times, int64_t first,
                                     int64_t last, dygnn_stream_t stream) {
    if (int rc = check_table(table_host, "edgebank_insert")) return rc;
    DYGNN_REQUIRE(first == table_host->num_edges, "edgebank_insert: first (%lld) must be the number of edges inserted so far (%lld)",
                  (long long)first, (long long)table_host->num_edges);
    DYGNN_REQUIRE(last >= first, "edgebank_insert: last (%lld) < first (%lld)", (long long)last, (long long)first);
    DYGNN_REQUIRE(last <= table_host->max_edges, "edgebank_insert: last (%lld) exceeds max_edges (%lld)", (long long)last,
                  (long long)table_host->max_edges);
    if (last == first) return DYGNN_OK;
    DYGNN_REQUIRE(src && dst && times, "edgebank_insert: null pointer");
    return launch_insert(table_host, src, dst, times, last, as_stream(stream));
}

extern "C" int dygnn_edgebank_query(const dygnn_edgebank* table_host, const double* times, int32_t mode, int32_t window_mode, int64_t H,
                                    double start_time, const int64_t* q_src, const int64_t* q_dst, int64_t n, float* out,
                                    dygnn_stream_t stream) {
    if (int rc = check_table(table_host, "edgebank_query")) return rc;
    if (int rc = check_modes(mode, window_mode, "edgebank_query")) return rc;
    DYGNN_REQUIRE(H >= 0 && H <= table_host->num_edges, "edgebank_query: H (%lld) exceeds the %lld edges inserted", (long long)H,
                  (long long)table_host->num_edges);
    DYGNN_REQUIRE(H == table_host->num_edges, "edgebank_query: H (%lld) is not the %lld edges inserted: the table answers for all of them",
                  (long long)H, (long long)table_host->num_edges);
    DYGNN_REQUIRE(mode != 2 || H > 0, "edgebank_query: time window memory needs a history (max() arg is an empty sequence)");
    DYGNN_REQUIRE(n >= 0, "edgebank_query: negative query count %lld", (long long)n);
    DYGNN_REQUIRE(n == 0 || (q_src && q_dst && out), "edgebank_query: null pointer");
    DYGNN_REQUIRE(!(mode == 2 && window_mode == 1) || times, "edgebank_query: repeat_interval needs the history times");
    return launch_query(table_host, times, mode, window_mode, start_time, nullptr, q_src, q_dst, n, out, as_stream(stream));
}

extern "C" int dygnn_edgebank_evaluate(dygnn_edgebank* table_host, const int64_t* src, const int64_t* dst, const double* times,
                                       const int64_t* hist_len_host, const double* start_times, const int64_t* q_src, const int64_t* q_dst,
                                       int64_t n_batches, int64_t queries_per_batch, int32_t mode, int32_t window_mode, float* out,
                                       dygnn_stream_t stream) {
    if (int rc = check_table(table_host, "edgebank_evaluate")) return rc;
    if (int rc = check_modes(mode, window_mode, "edgebank_evaluate")) return rc;
    DYGNN_REQUIRE(n_batches >= 0 && queries_per_batch >= 0, "edgebank_evaluate: negative size");
    if (n_batches == 0) return DYGNN_OK;
    DYGNN_REQUIRE(hist_len_host && src && dst && times, "edgebank_evaluate: null pointer");
    DYGNN_REQUIRE(queries_per_batch == 0 || (q_src && q_dst && out), "edgebank_evaluate: null pointer");
    DYGNN_REQUIRE(!(mode == 2 && window_mode == 0) || start_times, "edgebank_evaluate: fixed_proportion needs the batches' start times");
    int64_t prev = table_host->num_edges;
    for (int64_t b = 0; b < n_batches; ++b) {
        const int64_t H = hist_len_host[b];
        DYGNN_REQUIRE(H >= prev, "edgebank_evaluate: history length of batch %lld (%lld) is below the %lld edges already inserted", (long long)b,
                      (long long)H, (long long)prev);
        DYGNN_REQUIRE(H <= table_host->max_edges, "edgebank_evaluate: history length of batch %lld (%lld) exceeds max_edges (%lld)", (long long)b,
                      (long long)H, (long long)table_host->max_edges);
        DYGNN_REQUIRE(mode != 2 || H > 0, "edgebank_evaluate: time window memory needs a history (max() arg is an empty sequence)");
        prev = H;
    }
    for (int64_t b = 0; b < n_batches; ++b) {
        if (int rc = launch_insert(table_host, src, dst, times, hist_len_host[b], as_stream(stream))) return rc;
        const int64_t o = b * queries_per_batch;
        if (int rc = launch_query(table_host, times, mode, window_mode, 0.0, start_times ? start_times + b : nullptr, q_src + o, q_dst + o,
                                  queries_per_batch, out + o, as_stream(stream)))
            return rc;
    }
    return DYGNN_OK;
}
