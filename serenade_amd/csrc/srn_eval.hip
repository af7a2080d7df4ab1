// Offline evaluation on the GPU (include/serenade_hip.h, "offline evaluation"): the reference's evaluation loop (src/bin/evaluator.rs:46-76,
// src/objective.rs:8-52) over a test set resident in HBM.  A trial runs in chunks of queries; per chunk
//   eval_expand_kernel   the chunk's prefixes (CSR) straight from the resident test sessions, windowed to the trial's max_items_in_session
//   device_predict_device  the same launch sequence srn_predict_batch_device takes (the rows are the same bytes)
//   eval_metrics_kernel  one wave per query: the per-query terms of src/metrics/*.rs, and the recommended items' coverage bits
//   eval_group_kernel    partial sums per group of 256 GLOBAL query indices (chunks are multiples of 256, so a group never straddles two)
// The host adds the groups' partial sums in group order: a trial's sums do not depend on the chunk size or on the other trials of the call.
//
// Trials under the serving rules (SRN_FLAG_EVAL_HANDLER, SRN_FLAG_EXCLUDE_SESSION, SRN_FLAG_EXCLUDE_SEEN) expand a chunk in three steps instead:
// once repeated clicks collapse, a query's place in the CSR is no closed form of its state.
//   eval_serve_count_kernel   per query: |query(t)| and |list| packed into one 64-bit word, from a walk back from e_t under the handler's rule
//   rocprim::exclusive_scan   both offsets in one scan (the halves cannot carry into each other: a chunk's items and list ids are both below 2^32)
//   eval_serve_write_kernel   the same walk: items_flat / q_off, the exclusion CSR x_flat / x_off, (session, state)
// and predict with a RowRule over the lists, as srn_predict_batch_device_excl does: wide rows in the workspace's scratch, the filter and the fill kernel behind the
// launch sequence.  Nothing waits on the host between chunks: the buffers are sized from the capacities.  The metric, group and popcount kernels are the same.
#include <hip/hip_runtime.h>

#include <cstring>   // rocprim's texture iterator calls the host memset
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <unordered_map>
#include <vector>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_device.h"
#include "srn_hipsync.h"
#include "srn_events.h"
#include "srn_visitor_table.h"  // align256
#include "srn_segments.h"

// the terms must be the bits the host formulas give: no fused multiply-adds
#pragma clang fp contract(off)

namespace srn {

static constexpr uint32_t kGroup = 256;          // queries per partial sum
static constexpr uint32_t kTerms = 8;            // per query: mrr, hit, ndcg, intersection, precision, recall, popularity, (unused)
static constexpr uint32_t kSums = 6;             // per group: mrr, hit, ndcg, precision, recall, popularity
static constexpr uint32_t kDefaultChunk = 1u << 20;
static constexpr uint32_t kMaxChunk = 1u << 24;  // chunk items < 2^24 * SRN_MAX_SESSION_LEN < 2^32: q_off stays 32-bit
static constexpr uint32_t kMetricWaves = 4;

struct EvalDevice {
    int device = 0;
    uint64_t* items = nullptr; uint64_t* sess_off = nullptr;   // the test sessions
    double* freq = nullptr;                                     // [n_items] training count of each dense item of the index
    double* ndcg_w = nullptr;                                   // [SRN_MAX_HOW_MANY] w_i, then [SRN_MAX_HOW_MANY + 1] prefix sums of w (ndcg.rs:13-27)
    // grow-only workspace
    char* scan = nullptr; size_t scan_bytes = 0;               // per-session query / item offsets of one window
    char* chunk = nullptr; size_t chunk_bytes = 0;             // a chunk's prefixes, q_off, (session, state), rows, terms
    char* part = nullptr; size_t part_bytes = 0;               // per-group partial sums of every trial of a call
    char* cover = nullptr; size_t cover_bytes = 0;             // coverage bitmaps + popcounts + the error word
    char* boot = nullptr; size_t boot_bytes = 0;               // srn_evaluate_bootstrap: every trial's replicate totals, then one replicate tile's group partials
    char* seg = nullptr; size_t seg_bytes = 0;                 // srn_evaluate_segments: the regions of seg_buffers (srn_segments.h)
    std::vector<hipEvent_t> ev;
    std::vector<hipEvent_t> seg_ev;                             // three per chunk around the segment kernels
    double ms_seg = 0.0, ms_seg_boot = 0.0;                     // ... and what they measured in the last srn_evaluate_segments call (srn_debug_eval_segment_ms)
};

uint64_t eval_n_queries(const srn_eval_set* set) {
    uint64_t n = 0;
    for (size_t s = 0; s + 1 < set->sess_off.size(); ++s) { const uint64_t l = set->sess_off[s + 1] - set->sess_off[s]; if (l > 1) n += l - 1; }
    return n;
}

// items of the prefixes of states 1..n at window W: sum_{t=1}^{n} min(t, W)
__host__ __device__ inline uint64_t prefix_items(uint64_t n, uint64_t W) { return n <= W ? n * (n + 1) / 2 : W * (W + 1) / 2 + (n - W) * W; }

__global__ void __launch_bounds__(256) eval_expand_kernel(const uint64_t* __restrict__ items, const uint64_t* __restrict__ sess_off,
                                                          const uint64_t* __restrict__ sess_q, const uint64_t* __restrict__ sess_i, uint32_t n_sessions,
                                                          uint64_t q0, uint32_t nq, uint32_t W, uint64_t item_base,
                                                          uint64_t* __restrict__ out_items, uint32_t* __restrict__ out_qoff, uint2* __restrict__ out_ss) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint64_t g = q0 + i;
    uint32_t lo = 0, hi = n_sessions;   // the session s with sess_q[s] <= g < sess_q[s + 1] (sessions without queries have sess_q[s] == sess_q[s + 1])
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (sess_q[mid] <= g) lo = mid; else hi = mid; }
    const uint32_t s = lo;
    const uint64_t state = g - sess_q[s] + 1;
    const uint64_t start = state > W ? state - W : 0, len = state - start;
    const uint64_t at = sess_i[s] + prefix_items(state - 1, W) - item_base;
    const uint64_t* src = items + sess_off[s] + start;
    for (uint64_t j = 0; j < len; ++j) out_items[at + j] = src[j];
    out_qoff[i] = (uint32_t)at;
    if (i == nq - 1) out_qoff[nq] = (uint32_t)(at + len);
    out_ss[i] = make_uint2(s, (uint32_t)state);
}

// ---- expansion under the serving rules ----
struct ServeArgs {
    const uint64_t* items; const uint64_t* sess_off; const uint64_t* sess_q; uint32_t n_sessions;
    uint64_t q0; uint32_t nq;
    uint32_t W, cap;          // the session window; the exclusion lists' capacity (eval_excl_capacity: H' with SRN_FLAG_EXCLUDE_SEEN, W with SRN_FLAG_EXCLUDE_SESSION alone, else 0)
    uint32_t handler;         // SRN_FLAG_EVAL_HANDLER: a click equal to the one before it is no click
    uint64_t* packed;         // [nq + 1] count kernel: list length << 32 | query length; then, scanned in `offs`, the two offsets
    const uint64_t* offs;
    uint64_t* out_items; uint32_t* out_qoff; uint64_t* x_flat; uint32_t* x_off; uint2* out_ss;
};

// global query g -> its session and state (sessions without queries have sess_q[s] == sess_q[s + 1])
__device__ __forceinline__ void serve_locate(const ServeArgs& a, uint64_t g, uint32_t& s, uint32_t& state) {
    uint32_t lo = 0, hi = a.n_sessions;
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (a.sess_q[mid] <= g) lo = mid; else hi = mid; }
    s = lo; state = (uint32_t)(g - a.sess_q[lo] + 1);
}

// c(t) from its most recent item backwards, at most `want` items: f(r, id) for the r-th of them; returns how many there were.  ev = the session's events, t >= 1.
// One thread per query: neighbouring lanes hold neighbouring states of one session, so step r of the walk reads neighbouring addresses across the wave.
template <typename F> __device__ __forceinline__ uint32_t serve_walk(const uint64_t* __restrict__ ev, uint32_t t, bool handler, uint32_t want, F&& f) {
    uint32_t r = 0;
    if (!handler) {
        const uint32_t n = min(t, want);
        for (; r < n; ++r) f(r, ev[t - 1 - r]);
        return n;
    }
    uint64_t cur = ev[t - 1];
    for (uint32_t j = t; j >= 1 && r < want; --j) {   // e_j = ev[j - 1] stays unless it repeats e_{j-1}
        const uint64_t prev = j >= 2 ? ev[j - 2] : 0ull;
        if (j == 1 || cur != prev) { f(r, cur); ++r; }
        cur = prev;
    }
    return r;
}

__global__ void __launch_bounds__(256) eval_serve_count_kernel(ServeArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.nq) return;
    if (i == a.nq) { a.packed[i] = 0ull; return; }
    uint32_t s, t; serve_locate(a, a.q0 + i, s, t);
    const uint32_t want = max(a.W, a.cap);
    const uint32_t c = a.handler ? serve_walk(a.items + a.sess_off[s], t, true, want, [](uint32_t, uint64_t) {}) : min(t, want);
    a.packed[i] = ((uint64_t)min(c, a.cap) << 32) | min(c, a.W);
}

__global__ void __launch_bounds__(256) eval_serve_write_kernel(ServeArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > a.nq) return;
    const uint64_t o = a.offs[i];
    const uint32_t qo = (uint32_t)o, xo = (uint32_t)(o >> 32);
    a.out_qoff[i] = qo; a.x_off[i] = xo;
    if (i == a.nq) return;
    const uint64_t o1 = a.offs[i + 1];
    const uint32_t len = (uint32_t)o1 - qo, xlen = (uint32_t)(o1 >> 32) - xo;
    uint32_t s, t; serve_locate(a, a.q0 + i, s, t);
    uint64_t* __restrict__ qi = a.out_items + qo; uint64_t* __restrict__ xi = a.x_flat + xo;
    serve_walk(a.items + a.sess_off[s], t, a.handler != 0u, max(len, xlen), [&](uint32_t r, uint64_t id) {   // oldest first, as the handler's session is
        if (r < len) qi[len - 1u - r] = id;
        if (r < xlen) xi[xlen - 1u - r] = id;
    });
    a.out_ss[i] = make_uint2(s, t);
}

struct MetricArgs {
    const uint64_t* items; const uint64_t* sess_off;
    const uint2* ss; const uint64_t* ids; const uint32_t* counts;
    const double* freq; const double* w; const double* wsum; double max_freq;
    IdSlot const* id_table; uint32_t id_mask;
    uint32_t nq, how_many, length;
    double* terms; uint32_t* cover; uint32_t* err;
};

// one wave per query: rank positions across the lanes (64 per round), each lane scans the suffix for its item
__global__ void __launch_bounds__(64 * kMetricWaves) eval_metrics_kernel(MetricArgs a) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * kMetricWaves + (threadIdx.x >> 6);
    if (q >= a.nq) return;   // (wave-uniform)
    const uint32_t cnt = a.counts[q];
    double* t = a.terms + (size_t)q * kTerms;
    if (cnt == 0xFFFFFFFFu) {   // a query predict could not serve: the call fails
        if (lane == 0) { atomicOr(a.err, 1u); for (uint32_t j = 0; j < kTerms; ++j) t[j] = 0.0; }
        return;
    }
    const uint2 ss = a.ss[q];
    const uint64_t* sfx = a.items + a.sess_off[ss.x] + ss.y;
    const uint32_t slen = (uint32_t)(a.sess_off[ss.x + 1] - a.sess_off[ss.x] - ss.y);   // >= 1
    const uint64_t next0 = sfx[0];
    const uint32_t n_top = min(cnt, a.length);
    const uint64_t* row = a.ids + (size_t)q * a.how_many;
    int first = -1; uint32_t inter = 0; double num = 0.0, pop = 0.0;
    for (uint32_t base = 0; base < n_top; base += 64) {
        const uint32_t p = base + lane;
        bool found = false, hit = false; double pv = 0.0;
        if (p < n_top) {
            const uint64_t id = row[p];
            hit = id == next0;
            for (uint32_t j = 0; j < slen && !found; ++j) found = sfx[j] == id;
            uint32_t h = (uint32_t)dev_mix64(id) & a.id_mask, dense = kNone;   // the index's dictionary: recommended ids are always index items
            for (;;) { const IdSlot sl = a.id_table[h]; if (sl.idx == kNone) break; if (sl.key == id) { dense = sl.idx; break; } h = (h + 1) & a.id_mask; }
            if (dense != kNone) {
                pv = a.freq[dense] / a.max_freq;
                // popular items are recommended by most queries: an atomic only while the bit is still clear (one hot word would serialise them all)
                uint32_t* word = a.cover + (dense >> 5); const uint32_t bit = 1u << (dense & 31);
                if ((__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) == 0u) atomicOr(word, bit);
            }
        }
        const uint64_t fm = __ballot(found), hm = __ballot(hit);
        if (first < 0 && hm) first = (int)(base + __ffsll((long long)hm) - 1);
        inter += (uint32_t)__popcll(fm);
        // in rank order, one term at a time (the host restatements add in that order)
        const uint32_t n_here = min(64u, n_top - base);
        for (uint32_t l = 0; l < n_here; ++l) {
            pop += __shfl(pv, (int)l);
            if ((fm >> l) & 1ull) num += a.w[base + l];
        }
    }
    if (lane == 0) {
        t[0] = first >= 0 ? 1.0 / (double)(first + 1) : 0.0;                  // mrr.rs:24-33
        t[1] = first >= 0 ? 1.0 : 0.0;                                          // hitrate.rs:24-33
        t[2] = num / a.wsum[min(slen, a.length)];                               // ndcg.rs:42-56 (the ideal list: the first min(|suffix|, length) next items, all relevant)
        t[3] = (double)inter;
        t[4] = (double)inter / (double)a.length;                                // precision.rs:31-43
        t[5] = (double)inter / (double)slen;                                    // recall.rs:31-44 (duplicates counted)
        t[6] = n_top ? pop / (double)n_top : 0.0;                               // popularity.rs:41-58
        t[7] = 0.0;
    }
}

// one wave per group of 256 queries: four queries per lane in order, then a fixed butterfly
__global__ void __launch_bounds__(64) eval_group_kernel(const double* __restrict__ terms, uint32_t nq, double* __restrict__ part) {
    const uint32_t lane = threadIdx.x, q0 = blockIdx.x * kGroup;
    double s[kSums] = {0, 0, 0, 0, 0, 0};
    for (uint32_t r = 0; r < kGroup / 64; ++r) {
        const uint32_t q = q0 + lane * (kGroup / 64) + r;
        if (q < nq) {
            const double* t = terms + (size_t)q * kTerms;
            s[0] += t[0]; s[1] += t[1]; s[2] += t[2]; s[3] += t[4]; s[4] += t[5]; s[5] += t[6];
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kSums; ++j)
        for (int off = 32; off >= 1; off >>= 1) s[j] += __shfl_xor(s[j], off);
    if (lane == 0)
#pragma unroll
        for (uint32_t j = 0; j < kSums; ++j) part[(size_t)blockIdx.x * kSums + j] = s[j];
}

__global__ void __launch_bounds__(256) eval_popcount_kernel(const uint32_t* __restrict__ bits, uint32_t words, unsigned long long* __restrict__ out) {
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < words; i += gridDim.x * blockDim.x) c += __popc(bits[i]);
    for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

namespace {
template <typename T> int upload_new(T** p, const T* src, size_t n) {
    HIP_TRY(hipMalloc((void**)p, std::max<size_t>(n * sizeof(T), 16)));
    if (n) HIP_TRY(hipMemcpy(*p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return SRN_OK;
}
// ndcg.rs:13-27 on the host (std::log2), so that the device terms are the host formulas' bits
std::vector<double> ndcg_weights() {
    std::vector<double> w(2 * SRN_MAX_HOW_MANY + 1, 0.0);
    for (uint32_t i = 0; i < SRN_MAX_HOW_MANY; ++i) w[i] = i == 0 ? 1.0 : 1.0 / std::log2((double)i + 1.0);
    for (uint32_t n = 1; n <= SRN_MAX_HOW_MANY; ++n) w[SRN_MAX_HOW_MANY + n] = w[SRN_MAX_HOW_MANY + n - 1] + w[n - 1];
    return w;
}
}  // namespace

void eval_set_free(srn_eval_set* set) {
    if (!set) return;
    if (EvalDevice* e = set->dev) {
        (void)hipSetDevice(e->device);
        for (void* p : {(void*)e->items, (void*)e->sess_off, (void*)e->freq, (void*)e->ndcg_w, (void*)e->scan, (void*)e->chunk, (void*)e->part, (void*)e->cover, (void*)e->boot, (void*)e->seg})
            if (p) (void)hipFree(p);
        for (hipEvent_t x : e->ev) (void)hipEventDestroy(x);
        for (hipEvent_t x : e->seg_ev) (void)hipEventDestroy(x);
        delete e;
    }
    delete set;
}

int eval_set_create(const srn_index* idx, const uint64_t* items_flat, const uint64_t* sess_off, size_t n_sessions,
                    const uint64_t* train_ids, const uint64_t* train_counts, size_t n_train, srn_eval_set** out) {
    const FlatIndex& ix = idx->flat;
    srn_eval_set* set = new srn_eval_set();
    struct Guard { srn_eval_set*& s; ~Guard() { if (s) eval_set_free(s); } } guard{set};
    set->idx = idx;
    set->sess_off.assign(sess_off, sess_off + n_sessions + 1);
    for (size_t s = 0; s < n_sessions; ++s) set->max_session_len = std::max<uint64_t>(set->max_session_len, sess_off[s + 1] - sess_off[s]);
    // training counts -> per dense item of the index; Coverage's denominator counts every distinct training item, in the index or not
    std::unordered_map<uint64_t, uint64_t> merged; merged.reserve(n_train * 2 + 1);
    for (size_t i = 0; i < n_train; ++i) merged[train_ids[i]] += train_counts[i];
    std::vector<double> freq(ix.n_items, 0.0); uint64_t max_freq = 0;
    for (const auto& kv : merged) {
        max_freq = std::max(max_freq, kv.second);
        const uint32_t d = ix.lookup(kv.first);
        if (d != kNone) freq[d] = (double)kv.second;
    }
    set->max_freq = max_freq ? (double)max_freq : 1.0;
    set->unique_training_items = merged.size();
    const std::vector<double> w = ndcg_weights();
    EvalDevice* e = new EvalDevice(); set->dev = e; e->device = idx->device;
    HIP_TRY(hipSetDevice(e->device));
    int rc;
    if ((rc = upload_new(&e->items, items_flat, sess_off[n_sessions]))) return rc;
    if ((rc = upload_new(&e->sess_off, sess_off, n_sessions + 1))) return rc;
    if ((rc = upload_new(&e->freq, freq.data(), freq.size()))) return rc;
    if ((rc = upload_new(&e->ndcg_w, w.data(), w.size()))) return rc;
    *out = set; set = nullptr;
    return SRN_OK;
}

// src/io.rs:13-59: "SessionId ItemId Time" after a header line, time rounded half away from zero; sessions in ascending SessionId, each one's
// events ordered by time (a stable sort: equal times keep file order)
static int read_tsv_rows(const char* path, std::vector<std::pair<uint32_t, std::pair<long long, uint64_t>>>& rows) {
    FILE* f = fopen(path, "r");
    if (!f) return fail(SRN_EIO, std::string("cannot open ") + path);
    char line[4096];
    bool header = true;
    while (fgets(line, sizeof line, f)) {
        if (header) { header = false; continue; }
        char* p = line; char* end = nullptr;
        const unsigned long long s = strtoull(p, &end, 10); if (end == p) continue; p = end;
        const unsigned long long it = strtoull(p, &end, 10); if (end == p) continue; p = end;
        const double t = strtod(p, &end); if (end == p) continue;
        rows.push_back({(uint32_t)s, {std::llround(t), (uint64_t)it}});
    }
    fclose(f);
    return SRN_OK;
}

int eval_set_from_tsv(const srn_index* idx, const char* test_path, const char* train_path, srn_eval_set** out) {
    std::vector<std::pair<uint32_t, std::pair<long long, uint64_t>>> test, train;
    int rc = read_tsv_rows(test_path, test); if (rc) return rc;
    rc = read_tsv_rows(train_path, train); if (rc) return rc;
    std::map<uint32_t, std::vector<std::pair<long long, uint64_t>>> by_session;
    for (const auto& r : test) by_session[r.first].push_back(r.second);
    std::vector<uint64_t> items, off{0};
    for (auto& kv : by_session) {
        std::stable_sort(kv.second.begin(), kv.second.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (const auto& e : kv.second) items.push_back(e.second);
        off.push_back(items.size());
    }
    std::unordered_map<uint64_t, uint64_t> counts;
    for (const auto& r : train) ++counts[r.second.second];
    std::vector<uint64_t> ids, cnt;
    for (const auto& kv : counts) { ids.push_back(kv.first); cnt.push_back(kv.second); }
    return eval_set_create(idx, items.data(), off.data(), off.size() - 1, ids.data(), cnt.data(), ids.size(), out);
}

// ---- the same set from rows in memory, grouped and counted on the device (srn_eval_set_from_events) ----
// Test rows: two stable LSD radix sorts that carry the row index, by rounded time and then by session id, leave the rows in (session, time, input order); the items
// gathered in that order are the set's items, and a scan of the session heads gives the offsets.  Training items: one open-addressing table on the full ids
// (srn_events.h) counts the occurrences; a pass over its slots takes the distinct count and the largest count over ALL ids, as eval_set_create does, and writes the
// count of every id the index knows to its dense item.  The counts are integers below 2^32: the doubles are exact whatever order the atomics arrived in.
namespace {
constexpr int kEvTPB = 256;
constexpr unsigned kEvReduceBlocks = 1024;
inline dim3 ev_grid(uint64_t n, unsigned cap = 1u << 16) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + kEvTPB - 1) / kEvTPB, cap))); }
inline int ev_bits(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return std::max(b, 1); }

__global__ void ev_time_keys(const void* times, bool i64, uint64_t n, uint64_t* key, uint32_t* idx) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) { key[j] = event_time(times, i64, j); idx[j] = (uint32_t)j; }
}
__global__ void ev_gather(const uint64_t* src, const uint32_t* idx, uint64_t n, uint64_t* out) {
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) out[j] = src[idx[j]];
}
__global__ void ev_max(const uint64_t* a, uint64_t n, unsigned long long* out) {   // one atomic per wave of a small grid
    unsigned long long m = 0;
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x) m = max(m, (unsigned long long)a[j]);
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}
__global__ void ev_heads(const uint64_t* sess_sorted, uint64_t n, uint32_t* head) {   // head[n] = 0 (the scan's total)
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * blockDim.x)
        head[j] = j < n && (j == 0 || sess_sorted[j] != sess_sorted[j - 1]) ? 1u : 0u;
}
__global__ void ev_offsets(const uint32_t* head, const uint32_t* sid, uint64_t n, uint64_t* off) {   // sid = exclusive scan of head; sid[n] = number of sessions
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j <= n; j += (uint64_t)gridDim.x * blockDim.x)
        if (j == n || head[j]) off[sid[j]] = j;
}
__global__ void __launch_bounds__(kEvTPB) ev_count(const uint64_t* ids, uint64_t n, KeyTable T, uint32_t* cnt, unsigned long long* full) {
    __shared__ CombTable comb;   // the item column is Zipf: equal ids of a block are combined before they reach global memory
    comb_init(comb);
    for (uint64_t base = blockIdx.x * (uint64_t)kCombTile; base < n; base += (uint64_t)gridDim.x * kCombTile) {   // whole blocks stay in the loop together
        for (uint32_t q = 0; q < kCombTile / kEvTPB; ++q) {
            const uint64_t j = base + q * kEvTPB + threadIdx.x;
            if (j >= n) break;
            bool fresh;
            const uint32_t s = key_table_insert(T, ids[j], &fresh);
            if (s == kNone) { atomicAdd(full, 1ull); continue; }
            comb_add(comb, cnt, s);
        }
        comb_flush(comb, cnt);
    }
}
// out2: distinct ids, largest count
__global__ void ev_freq(KeyTable T, const uint32_t* cnt, const IdSlot* id_table, uint32_t id_mask, double* freq, unsigned long long* out2) {
    unsigned long long distinct = 0, mx = 0;
    for (uint64_t e = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; e <= (uint64_t)T.mask + 1; e += (uint64_t)gridDim.x * blockDim.x) {
        const bool own = e == (uint64_t)T.mask + 1;   // the slot of the id ~0
        const unsigned long long key = own ? kEmptyKey : T.keys[e];
        if (own ? T.keys[e] != 0 : key == kEmptyKey) continue;
        const uint32_t c = cnt[e];
        ++distinct; mx = max(mx, (unsigned long long)c);
        if (!id_table) continue;
        for (uint32_t h = (uint32_t)dev_mix64(key) & id_mask;; h = (h + 1) & id_mask) {   // FlatIndex::lookup
            const IdSlot s = id_table[h];
            if (s.idx == kNone) break;
            if (s.key == key) { freq[s.idx] = (double)c; break; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { distinct += __shfl_xor(distinct, o); mx = max(mx, __shfl_xor(mx, o)); }
    if ((threadIdx.x & 63) == 0 && distinct) { atomicAdd(&out2[0], distinct); atomicMax(&out2[1], mx); }
}
}  // namespace

int eval_set_from_events(const srn_index* idx, const uint64_t* test_sess, const uint64_t* test_item, const void* test_times, size_t n_test,
                         const uint64_t* train_item, size_t n_train, unsigned flags, void* stream, srn_eval_set** out) {
    const FlatIndex& ix = idx->flat;
    const bool on_device = flags & SRN_EVENTS_DEVICE, i64 = flags & SRN_EVENTS_TIME_I64;
    if (on_device) {
        int rc = SRN_OK;
        if (n_test && ((rc = check_device_rows(test_sess, idx->device, "test_session_ids")) || (rc = check_device_rows(test_item, idx->device, "test_item_ids")) ||
                       (rc = check_device_rows(test_times, idx->device, "test_times")))) return rc;
        if (n_train && (rc = check_device_rows(train_item, idx->device, "train_item_ids"))) return rc;
    }
    HIP_TRY(hipSetDevice(idx->device));
    hipStream_t st = (hipStream_t)stream;
    srn_eval_set* set = new srn_eval_set();
    struct Guard { srn_eval_set*& s; ~Guard() { if (s) eval_set_free(s); } } guard{set};
    set->idx = idx;
    EvalDevice* e = new EvalDevice(); set->dev = e; e->device = idx->device;
    DevBuf u_s, u_i, u_t, u_tr;
    if (!on_device) {
        if (n_test) {
            HIP_TRY(u_s.alloc(n_test * 8)); HIP_TRY(u_i.alloc(n_test * 8)); HIP_TRY(u_t.alloc(n_test * 8));
            HIP_TRY(hipMemcpyAsync(u_s.p, test_sess, n_test * 8, hipMemcpyHostToDevice, st)); HIP_TRY(hipMemcpyAsync(u_i.p, test_item, n_test * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(u_t.p, test_times, n_test * 8, hipMemcpyHostToDevice, st));
            test_sess = u_s.as<uint64_t>(); test_item = u_i.as<uint64_t>(); test_times = u_t.p;
        }
        if (n_train) {
            HIP_TRY(u_tr.alloc(n_train * 8));
            HIP_TRY(hipMemcpyAsync(u_tr.p, train_item, n_train * 8, hipMemcpyHostToDevice, st));
            train_item = u_tr.as<uint64_t>();
        }
    }
    // the test sessions
    const uint64_t n = n_test;
    HIP_TRY(hipMalloc((void**)&e->items, std::max<size_t>(n * 8, 16)));
    uint64_t n_sessions = 0;
    if (n) {
        DevBuf keyA, keyB, idxA, idxB, mx, head, sid, tmp;
        HIP_TRY(keyA.alloc(n * 8)); HIP_TRY(keyB.alloc(n * 8)); HIP_TRY(idxA.alloc(n * 4)); HIP_TRY(idxB.alloc(n * 4)); HIP_TRY(mx.alloc(16));
        HIP_TRY(head.alloc((n + 1) * 4)); HIP_TRY(sid.alloc((n + 1) * 4));
        HIP_TRY(hipMemsetAsync(mx.p, 0, 16, st));
        hipLaunchKernelGGL(ev_time_keys, ev_grid(n), dim3(kEvTPB), 0, st, test_times, i64, n, keyA.as<uint64_t>(), idxA.as<uint32_t>());
        hipLaunchKernelGGL(ev_max, ev_grid(n, kEvReduceBlocks), dim3(kEvTPB), 0, st, keyA.as<uint64_t>(), n, mx.as<unsigned long long>());
        hipLaunchKernelGGL(ev_max, ev_grid(n, kEvReduceBlocks), dim3(kEvTPB), 0, st, test_sess, n, mx.as<unsigned long long>() + 1);
        unsigned long long maxes[2];
        HIP_TRY(hipMemcpyAsync(maxes, mx.p, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        size_t tb = 0, t1 = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, keyA.as<uint64_t>(), keyB.as<uint64_t>(), idxA.as<uint32_t>(), idxB.as<uint32_t>(), n, 0, 64, st)); tb = t1;
        HIP_TRY(rocprim::exclusive_scan(nullptr, t1, head.as<uint32_t>(), sid.as<uint32_t>(), 0u, n + 1, rocprim::plus<uint32_t>(), st)); tb = std::max(tb, t1);
        HIP_TRY(tmp.alloc(tb));
        t1 = tb; HIP_TRY(rocprim::radix_sort_pairs(tmp.p, t1, keyA.as<uint64_t>(), keyB.as<uint64_t>(), idxA.as<uint32_t>(), idxB.as<uint32_t>(), n, 0, ev_bits(maxes[0]), st));
        hipLaunchKernelGGL(ev_gather, ev_grid(n), dim3(kEvTPB), 0, st, test_sess, idxB.as<uint32_t>(), n, keyA.as<uint64_t>());
        t1 = tb; HIP_TRY(rocprim::radix_sort_pairs(tmp.p, t1, keyA.as<uint64_t>(), keyB.as<uint64_t>(), idxB.as<uint32_t>(), idxA.as<uint32_t>(), n, 0, ev_bits(maxes[1]), st));
        // keyB = the session ids in set order, idxA = the rows' input indices
        hipLaunchKernelGGL(ev_gather, ev_grid(n), dim3(kEvTPB), 0, st, test_item, idxA.as<uint32_t>(), n, e->items);
        hipLaunchKernelGGL(ev_heads, ev_grid(n + 1), dim3(kEvTPB), 0, st, keyB.as<uint64_t>(), n, head.as<uint32_t>());
        t1 = tb; HIP_TRY(rocprim::exclusive_scan(tmp.p, t1, head.as<uint32_t>(), sid.as<uint32_t>(), 0u, n + 1, rocprim::plus<uint32_t>(), st));
        uint32_t ns32 = 0;
        HIP_TRY(hipMemcpyAsync(&ns32, sid.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        n_sessions = ns32;
        HIP_TRY(hipMalloc((void**)&e->sess_off, (n_sessions + 1) * 8));
        hipLaunchKernelGGL(ev_offsets, ev_grid(n + 1), dim3(kEvTPB), 0, st, head.as<uint32_t>(), sid.as<uint32_t>(), n, e->sess_off);
        HIP_TRY(hipGetLastError());
        set->sess_off.resize(n_sessions + 1);
        HIP_TRY(hipMemcpyAsync(set->sess_off.data(), e->sess_off, (n_sessions + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else {
        set->sess_off.assign(1, 0);
        HIP_TRY(hipMalloc((void**)&e->sess_off, 16));
        HIP_TRY(hipMemsetAsync(e->sess_off, 0, 16, st));
    }
    for (uint64_t s = 0; s < n_sessions; ++s) set->max_session_len = std::max<uint64_t>(set->max_session_len, set->sess_off[s + 1] - set->sess_off[s]);
    // the training counts
    HIP_TRY(hipMalloc((void**)&e->freq, std::max<size_t>(ix.n_items * 8, 16)));
    HIP_TRY(hipMemsetAsync(e->freq, 0, std::max<size_t>(ix.n_items * 8, 16), st));
    unsigned long long h3[3] = {0, 0, 0};   // distinct ids, largest count, inserts the table refused
    if (n_train) {
        const uint32_t slots = key_table_slots(n_train);
        DevBuf keys, cnt, out3;
        HIP_TRY(keys.alloc(((uint64_t)slots + 1) * 8)); HIP_TRY(cnt.alloc(((uint64_t)slots + 1) * 4)); HIP_TRY(out3.alloc(24));
        HIP_TRY(hipMemsetAsync(keys.p, 0xFF, ((uint64_t)slots + 1) * 8, st)); HIP_TRY(hipMemsetAsync(cnt.p, 0, ((uint64_t)slots + 1) * 4, st)); HIP_TRY(hipMemsetAsync(out3.p, 0, 24, st));
        const KeyTable T{keys.as<unsigned long long>(), slots - 1, split_hash_bits()};
        hipLaunchKernelGGL(ev_count, dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_train + kCombTile - 1) / kCombTile, 2048))), dim3(kEvTPB), 0, st, train_item, (uint64_t)n_train, T, cnt.as<uint32_t>(), out3.as<unsigned long long>() + 2);
        hipLaunchKernelGGL(ev_freq, ev_grid((uint64_t)slots + 1, kEvReduceBlocks), dim3(kEvTPB), 0, st, T, cnt.as<uint32_t>(), ix.id_table.empty() ? nullptr : idx->dev->di.id_table,
                           idx->dev->di.id_mask, e->freq, out3.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h3, out3.p, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h3[2]) return fail(SRN_ERANGE, "more distinct training items than the counting table's 2^31 slots");
    }
    set->max_freq = h3[1] ? (double)h3[1] : 1.0;
    set->unique_training_items = h3[0];
    const std::vector<double> w = ndcg_weights();
    int rc;
    if ((rc = upload_new(&e->ndcg_w, w.data(), w.size()))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    *out = set; set = nullptr;
    return SRN_OK;
}

static uint32_t chunk_queries(const srn_eval_trial_t& t) {
    // (the rows predict writes are how_many + the lists' capacity wide; a trial that excludes nothing has capacity 0)
    uint32_t c = t.max_chunk_queries ? t.max_chunk_queries : std::min<uint32_t>(kDefaultChunk, (1u << 26) / (t.how_many + eval_excl_capacity(t)));
    // 32-bit offsets: a chunk's items (<= W per query) and list ids (<= the capacity) both stay below 2^32 (kMaxChunk alone keeps them there while SRN_MAX_SESSION_LEN < 256)
    const uint32_t per_query = std::max(t.max_items_in_session, eval_excl_capacity(t));
    c = std::min<uint64_t>(std::min(c, kMaxChunk), 0xFFFFFFFFull / per_query) / kGroup * kGroup;
    return std::max(c, kGroup);
}

int eval_run(srn_eval_set* set, const srn_eval_trial_t* trials, size_t n_trials, srn_eval_result_t* out, void* user_stream, double* terms_out, size_t cap,
             const srn_bootstrap_t* boot, double* rep, const srn_segments_t* seg, srn_eval_segment_t* seg_out, double* seg_rep) {
    EvalDevice* e = set->dev; const srn_index* idx = set->idx; const FlatIndex& ix = idx->flat;
    HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)user_stream;
    const size_t n_s = set->sess_off.size() - 1;
    const uint64_t nq_all = eval_n_queries(set);
    const uint64_t n_groups = (nq_all + kGroup - 1) / kGroup;
    const uint32_t bitmap_words = (uint32_t)((ix.n_items + 31) / 32 + 1);
    if (terms_out && cap < nq_all) return fail(SRN_ERANGE, "per-query terms: no room for every query of the trial");
    // device buffers for the whole call
    int rc;
    const size_t cover_stride = align256((size_t)bitmap_words * 4);
    if ((rc = ensure(&e->cover, &e->cover_bytes, n_trials * cover_stride + align256(n_trials * 8) + 256))) return rc;
    uint32_t* err = (uint32_t*)(e->cover + n_trials * cover_stride + align256(n_trials * 8));
    unsigned long long* covered = (unsigned long long*)(e->cover + n_trials * cover_stride);
    HIP_TRY(hipMemsetAsync(e->cover, 0, e->cover_bytes, st));
    if ((rc = ensure(&e->part, &e->part_bytes, std::max<size_t>(n_trials * n_groups * kSums * 8, 256)))) return rc;
    size_t max_chunk = 0, n_events = 0;
    for (size_t t = 0; t < n_trials; ++t) { const uint64_t c = std::min<uint64_t>(chunk_queries(trials[t]), nq_all); max_chunk = std::max<size_t>(max_chunk, c);
                                            n_events += 4 * ((nq_all + chunk_queries(trials[t]) - 1) / chunk_queries(trials[t])); }
    while (e->ev.size() < n_events) { hipEvent_t x; HIP_TRY(hipEventCreate(&x)); e->ev.push_back(x); }
    // the bootstrap's totals [trial][replicate][sum], zeroed here and copied back with the sums, and behind them the scratch of the largest chunk
    const size_t boot_totals = boot ? align256(n_trials * (size_t)boot->replicates * SRN_BOOTSTRAP_SUMS * 8) : 0;
    if (boot) {
        if ((rc = ensure(&e->boot, &e->boot_bytes, boot_totals + boot_scratch_bytes(max_chunk, boot->replicates)))) return rc;
        HIP_TRY(hipMemsetAsync(e->boot, 0, boot_totals, st));
    }
    // the segmentation: labels up, totals zeroed; the ids of a chunk and the partials of its groups are rewritten chunk by chunk
    const uint32_t S = seg ? seg->segments : 0, seg_B = seg && boot ? boot->replicates : 0;
    SegBuffers sb; SegSet seg_set{}; SegRule seg_rule{};
    size_t seg_ev_at = 0;
    if (seg) {
        sb = seg_buffers(n_s, max_chunk, n_trials, S, seg_B);
        if ((rc = ensure(&e->seg, &e->seg_bytes, sb.bytes))) return rc;
        size_t n_seg_events = 0;
        for (size_t t = 0; t < n_trials; ++t) n_seg_events += 3 * ((nq_all + chunk_queries(trials[t]) - 1) / chunk_queries(trials[t]));
        while (e->seg_ev.size() < n_seg_events) { hipEvent_t x; HIP_TRY(hipEventCreate(&x)); e->seg_ev.push_back(x); }
        seg_set = SegSet{e->items, e->sess_off, e->freq, idx->dev->di.id_table, idx->dev->di.id_mask};
        seg_rule.mode = seg->mode; seg_rule.S = S; seg_rule.labels = (const uint16_t*)(e->seg + sb.labels);
        for (uint32_t j = 0; j + 1 < S && seg->bounds && seg->mode != SRN_SEG_STATE && seg->mode != SRN_SEG_LABEL; ++j) seg_rule.bounds[j] = seg->bounds[j];
        if (seg->mode == SRN_SEG_LABEL && n_s) HIP_TRY(hipMemcpyAsync(e->seg + sb.labels, seg->labels, n_s * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(e->seg + sb.totals, 0, n_trials * S * kSegSums * 8, st));
        if (seg_B) HIP_TRY(hipMemsetAsync(e->seg + sb.boot_totals, 0, n_trials * S * (size_t)seg_B * kSegSums * 8, st));
    }
    if ((rc = ensure(&e->scan, &e->scan_bytes, 2 * (n_s + 1) * 8))) return rc;
    std::vector<uint64_t> scan(2 * (n_s + 1));
    uint32_t scan_W = 0;
    size_t ev_at = 0;
    std::vector<std::pair<size_t, size_t>> trial_events(n_trials);
    for (size_t ti = 0; ti < n_trials; ++ti) {
        const srn_eval_trial_t& tr = trials[ti];
        const uint32_t W = tr.max_items_in_session;
        trial_events[ti].first = ev_at;
        if (nq_all == 0) { trial_events[ti].second = ev_at; continue; }
        if (W != scan_W) {   // per-session query and item offsets of this window (one scan per distinct window in a row of trials)
            uint64_t q = 0, it = 0;
            for (size_t s = 0; s < n_s; ++s) {
                scan[s] = q; scan[n_s + 1 + s] = it;
                const uint64_t l = set->sess_off[s + 1] - set->sess_off[s];
                if (l > 1) { q += l - 1; it += prefix_items(l - 1, W); }
            }
            scan[n_s] = q; scan[2 * n_s + 1] = it;
            HIP_TRY(hipMemcpyAsync(e->scan, scan.data(), scan.size() * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));   // (the host vector is rewritten by the next window)
            scan_W = W;
        }
        const uint64_t* sess_q = (const uint64_t*)e->scan; const uint64_t* sess_i = sess_q + n_s + 1;
        const uint32_t max_len = (uint32_t)std::min<uint64_t>(W, set->max_session_len - 1);
        const uint32_t chunk = chunk_queries(tr);
        const uint32_t cq = (uint32_t)std::min<uint64_t>(chunk, nq_all);
        // the serving rules: the trial's chunks take the count / scan / write expansion and predict with the lists (a trial without these flags enqueues what it always did)
        const bool serving = (tr.flags & (SRN_FLAG_EVAL_HANDLER | SRN_FLAG_EXCLUDE_SESSION | SRN_FLAG_EXCLUDE_SEEN)) != 0u;
        const uint32_t cap = eval_excl_capacity(tr);
        const uint32_t max_x = (uint32_t)std::min<uint64_t>(cap, set->max_session_len - 1);   // a list is never longer than its query's state
        size_t scan_tmp = 0;
        if (serving)   // rocPRIM's temporary storage, for a full chunk and for the last one
            for (const uint64_t n : {(uint64_t)cq + 1, nq_all % chunk + 1}) {
                size_t t1 = 0;
                HIP_TRY(rocprim::exclusive_scan(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr, 0ull, (size_t)n, rocprim::plus<uint64_t>(), st));
                scan_tmp = std::max(scan_tmp, t1);
            }
        // chunk buffers: items | q_off | (session, state) | ids | scores | counts | terms, and under the serving rules | list ids | x_off | packed lengths | packed offsets | scan storage
        // (the serving rules' regions are empty, not absent, without them: the plain call is handed the same pointers as ever)
        const size_t q1 = (size_t)cq + 1, sv = serving ? 1 : 0;
        Bump cbump;
        const auto r_items = cbump.of<uint64_t>((size_t)cq * max_len); const auto r_qoff = cbump.of<uint32_t>(q1); const auto r_ss = cbump.of<uint2>(cq);
        const auto r_ids = cbump.of<uint64_t>((size_t)cq * tr.how_many); const auto r_sc = cbump.of<double>((size_t)cq * tr.how_many); const auto r_cnt = cbump.of<uint32_t>(cq);
        const auto r_terms = cbump.of<double>((size_t)cq * kTerms);
        const auto r_x = cbump.of<uint64_t>(sv * cq * max_x); const auto r_xoff = cbump.of<uint32_t>(sv * q1); const auto r_pk = cbump.of<uint64_t>(sv * q1), r_po = cbump.of<uint64_t>(sv * q1);
        const auto r_tmp = cbump.of<char>(scan_tmp);
        if (cbump.bytes > e->chunk_bytes) { HIP_TRY(hipStreamSynchronize(st)); if ((rc = ensure(&e->chunk, &e->chunk_bytes, cbump.bytes))) return rc; }
        char* cb = e->chunk;
        uint64_t* d_items = r_items.at(cb); uint32_t* d_qoff = r_qoff.at(cb); uint2* d_ss = r_ss.at(cb);
        uint64_t* d_ids = r_ids.at(cb); double* d_sc = r_sc.at(cb); uint32_t* d_cnt = r_cnt.at(cb); double* d_terms = r_terms.at(cb);
        uint64_t* d_x = r_x.at(cb); uint32_t* d_xoff = r_xoff.at(cb);
        double* part = (double*)e->part + ti * n_groups * kSums;
        uint32_t* bitmap = (uint32_t*)(e->cover + ti * cover_stride);
        for (uint64_t q0 = 0; q0 < nq_all; q0 += chunk) {
            const uint32_t nq = (uint32_t)std::min<uint64_t>(chunk, nq_all - q0);
            hipEvent_t* ev = &e->ev[ev_at]; ev_at += 4;
            HIP_TRY(hipEventRecord(ev[0], st));
            // item offset of query q0: its session's start + the prefixes before it
            if (serving) {
                ServeArgs sa{};
                sa.items = e->items; sa.sess_off = e->sess_off; sa.sess_q = sess_q; sa.n_sessions = (uint32_t)n_s; sa.q0 = q0; sa.nq = nq;
                sa.W = W; sa.cap = cap; sa.handler = (tr.flags & SRN_FLAG_EVAL_HANDLER) ? 1u : 0u;
                sa.packed = r_pk.at(cb); sa.offs = r_po.at(cb);
                sa.out_items = d_items; sa.out_qoff = d_qoff; sa.x_flat = d_x; sa.x_off = d_xoff; sa.out_ss = d_ss;
                eval_serve_count_kernel<<<(nq + 1 + 255) / 256, 256, 0, st>>>(sa);
                HIP_TRY(hipGetLastError());
                size_t t1 = scan_tmp;
                HIP_TRY(rocprim::exclusive_scan(r_tmp.at(cb), t1, sa.packed, r_po.at(cb), 0ull, (size_t)nq + 1, rocprim::plus<uint64_t>(), st));
                eval_serve_write_kernel<<<(nq + 1 + 255) / 256, 256, 0, st>>>(sa);
                HIP_TRY(hipGetLastError());
            } else {
                uint64_t item_base;
                { const size_t s = (size_t)(std::upper_bound(scan.begin(), scan.begin() + n_s + 1, q0) - scan.begin()) - 1;
                  item_base = scan[n_s + 1 + s] + prefix_items(q0 - scan[s], W); }
                eval_expand_kernel<<<(nq + 255) / 256, 256, 0, st>>>(e->items, e->sess_off, sess_q, sess_i, (uint32_t)n_s, q0, nq, W, item_base, d_items, d_qoff, d_ss);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(ev[1], st));
            // (a grid of trials is no serving traffic: the index's result cache is bypassed)
            const LaunchParams p = launch_params(nq, tr.k, tr.m, tr.how_many, (tr.flags & SRN_FLAG_BUSINESS_LOGIC) | kFlagNoResultCache, max_len, d_items, d_qoff, d_ids, d_sc, d_cnt);
            // the lists are the exclusion CSR of srn_predict_batch_device_excl, their capacity `cap` (0: the trial excludes nothing, the plain call); SRN_FLAG_FILL: the metric
            // kernel scores the filled rows -- the fill kernel runs behind the launch sequence, inside the call
            RowRule rule; rule.x_flat = d_x; rule.x_off = d_xoff; rule.max_excl = cap; rule.fill = (tr.flags & SRN_FLAG_FILL) != 0u;
            if ((rc = device_predict_device(idx->dev, ix, p, st, rule))) return rc;
            HIP_TRY(hipSetDevice(e->device));
            HIP_TRY(hipEventRecord(ev[2], st));
            MetricArgs a{};
            a.items = e->items; a.sess_off = e->sess_off; a.ss = d_ss; a.ids = d_ids; a.counts = d_cnt;
            a.freq = e->freq; a.w = e->ndcg_w; a.wsum = e->ndcg_w + SRN_MAX_HOW_MANY; a.max_freq = set->max_freq;
            a.id_table = idx->dev->di.id_table; a.id_mask = idx->dev->di.id_mask;
            a.nq = nq; a.how_many = tr.how_many; a.length = tr.length; a.terms = d_terms; a.cover = bitmap; a.err = err;
            eval_metrics_kernel<<<(nq + kMetricWaves - 1) / kMetricWaves, 64 * kMetricWaves, 0, st>>>(a);
            HIP_TRY(hipGetLastError());
            eval_group_kernel<<<(nq + kGroup - 1) / kGroup, 64, 0, st>>>(d_terms, nq, part + (q0 / kGroup) * kSums);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev[3], st));
            if (boot && (rc = boot_chunk(d_terms, d_ss, nq, *boot, (double*)(e->boot + boot_totals),
                                         (double*)e->boot + ti * (size_t)boot->replicates * SRN_BOOTSTRAP_SUMS, st))) return rc;
            if (seg) {
                hipEvent_t* sev = &e->seg_ev[seg_ev_at]; seg_ev_at += 3;
                uint16_t* d_seg_ids = (uint16_t*)(e->seg + sb.ids);
                HIP_TRY(hipEventRecord(sev[0], st));
                if ((rc = seg_ids(seg_set, seg_rule, d_ss, nq, d_seg_ids, st))) return rc;
                if ((rc = seg_chunk(d_terms, d_seg_ids, nq, S, (double*)(e->seg + sb.part), (double*)(e->seg + sb.totals) + ti * S * kSegSums, st))) return rc;
                HIP_TRY(hipEventRecord(sev[1], st));
                if (seg_B && (rc = seg_boot_chunk(d_terms, d_ss, d_seg_ids, nq, S, *boot, (double*)(e->seg + sb.boot_part),
                                                  (double*)(e->seg + sb.boot_totals) + ti * S * (size_t)seg_B * kSegSums, st))) return rc;
                HIP_TRY(hipEventRecord(sev[2], st));
            }
            if (terms_out) {   // (test aid) the chunk's terms, 7 per query
                std::vector<double> h((size_t)nq * kTerms);
                HIP_TRY(hipMemcpyAsync(h.data(), d_terms, h.size() * 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                for (uint32_t q = 0; q < nq; ++q) std::copy(h.begin() + (size_t)q * kTerms, h.begin() + (size_t)q * kTerms + 7, terms_out + (q0 + q) * 7);
            }
        }
        eval_popcount_kernel<<<std::min<uint32_t>((bitmap_words + 255) / 256, 1024), 256, 0, st>>>(bitmap, bitmap_words, covered + ti);
        HIP_TRY(hipGetLastError());
        trial_events[ti].second = ev_at;
    }
    // results: the groups' partial sums in group order
    std::vector<double> part(std::max<size_t>(n_trials * n_groups * kSums, 1));
    std::vector<unsigned long long> cov(std::max<size_t>(n_trials, 1)); uint32_t h_err = 0;
    if (n_trials * n_groups) HIP_TRY(hipMemcpyAsync(part.data(), e->part, n_trials * n_groups * kSums * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(cov.data(), covered, n_trials * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
    if (boot) HIP_TRY(hipMemcpyAsync(rep, e->boot, n_trials * (size_t)boot->replicates * SRN_BOOTSTRAP_SUMS * 8, hipMemcpyDeviceToHost, st));
    std::vector<double> seg_tot(seg ? n_trials * S * kSegSums : 0);
    if (seg) {
        HIP_TRY(hipMemcpyAsync(seg_tot.data(), e->seg + sb.totals, seg_tot.size() * 8, hipMemcpyDeviceToHost, st));
        if (seg_B) HIP_TRY(hipMemcpyAsync(seg_rep, e->seg + sb.boot_totals, n_trials * S * (size_t)seg_B * kSegSums * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (h_err) return fail(SRN_ERANGE, "a query exceeded the kernel's table limits");
    if (seg) {
        for (size_t i = 0; i < n_trials * S; ++i) {   // (the counts are integers far below 2^53: exact as doubles)
            const double* v = &seg_tot[i * kSegSums];
            seg_out[i] = srn_eval_segment_t{(uint64_t)v[0], v[1], v[2], v[3], v[4], v[5], v[6]};
        }
        e->ms_seg = e->ms_seg_boot = 0.0;
        for (size_t k = 0; k < seg_ev_at; k += 3) {
            float a = 0, b = 0;
            HIP_TRY(hipEventElapsedTime(&a, e->seg_ev[k], e->seg_ev[k + 1]));
            HIP_TRY(hipEventElapsedTime(&b, e->seg_ev[k + 1], e->seg_ev[k + 2]));
            e->ms_seg += (double)a; e->ms_seg_boot += (double)b;
        }
    }
    for (size_t ti = 0; ti < n_trials; ++ti) {
        srn_eval_result_t& r = out[ti];
        r = srn_eval_result_t{};
        double s[kSums] = {0, 0, 0, 0, 0, 0};
        for (uint64_t g = 0; g < n_groups; ++g)
            for (uint32_t j = 0; j < kSums; ++j) s[j] += part[(ti * n_groups + g) * kSums + j];
        r.n_evaluations = nq_all;
        r.sum_mrr = s[0]; r.sum_hit_rate = s[1]; r.sum_ndcg = s[2]; r.sum_precision = s[3]; r.sum_recall = s[4]; r.sum_popularity = s[5];
        const double n = (double)nq_all;
        auto avg = [&](double v) { return nq_all ? v / n : 0.0; };
        r.mrr = avg(s[0]); r.hit_rate = avg(s[1]); r.ndcg = avg(s[2]); r.precision = avg(s[3]); r.recall = avg(s[4]); r.popularity = avg(s[5]);
        const double f = 2.0 * (r.precision * r.recall) / (r.precision + r.recall);
        r.f1score = std::isnan(f) ? 0.0 : f;                                               // f1score.rs:27-36
        r.covered_items = cov[ti]; r.unique_training_items = set->unique_training_items;
        r.coverage = set->unique_training_items ? (double)cov[ti] / (double)set->unique_training_items : 0.0;
        for (size_t k = trial_events[ti].first; k < trial_events[ti].second; k += 4) {
            float a = 0, b = 0, c = 0;
            HIP_TRY(hipEventElapsedTime(&a, e->ev[k], e->ev[k + 1]));
            HIP_TRY(hipEventElapsedTime(&b, e->ev[k + 1], e->ev[k + 2]));
            HIP_TRY(hipEventElapsedTime(&c, e->ev[k + 2], e->ev[k + 3]));
            r.ms_eval += (double)a + (double)c; r.ms_predict += (double)b;
        }
    }
    return SRN_OK;
}

// srn_eval_segment_ids: the (session, state) pairs of every query from the host's offsets, the id kernel over them, the ids back
int eval_segment_ids(srn_eval_set* set, const srn_segments_t* seg, uint16_t* out) {
    EvalDevice* e = set->dev; const srn_index* idx = set->idx;
    HIP_TRY(hipSetDevice(e->device));
    const size_t n_s = set->sess_off.size() - 1;
    const uint64_t nq = eval_n_queries(set);
    if (nq == 0) return SRN_OK;
    if (nq > 0xFFFFFFFFull) return fail(SRN_ERANGE, "more than 2^32 - 1 queries");
    std::vector<uint2> ss; ss.reserve(nq);
    for (size_t s = 0; s < n_s; ++s)
        for (uint64_t t = 1; t + set->sess_off[s] < set->sess_off[s + 1]; ++t) ss.push_back(make_uint2((uint32_t)s, (uint32_t)t));
    DevBuf d_ss, d_ids, d_labels;
    HIP_TRY(d_ss.alloc(nq * sizeof(uint2))); HIP_TRY(d_ids.alloc(nq * sizeof(uint16_t)));
    HIP_TRY(hipMemcpy(d_ss.p, ss.data(), nq * sizeof(uint2), hipMemcpyHostToDevice));
    SegRule rule{}; rule.mode = seg->mode; rule.S = seg->segments;
    if (seg->mode == SRN_SEG_LABEL) {
        HIP_TRY(d_labels.alloc(n_s * sizeof(uint16_t)));
        if (n_s) HIP_TRY(hipMemcpy(d_labels.p, seg->labels, n_s * sizeof(uint16_t), hipMemcpyHostToDevice));
        rule.labels = d_labels.as<uint16_t>();
    } else if (seg->mode != SRN_SEG_STATE) {
        for (uint32_t j = 0; j + 1 < seg->segments; ++j) rule.bounds[j] = seg->bounds[j];
    }
    const SegSet ss_set{e->items, e->sess_off, e->freq, idx->dev->di.id_table, idx->dev->di.id_mask};
    int rc = seg_ids(ss_set, rule, d_ss.p, (uint32_t)nq, d_ids.as<uint16_t>(), nullptr); if (rc) return rc;
    HIP_TRY(hipMemcpy(out, d_ids.p, nq * sizeof(uint16_t), hipMemcpyDeviceToHost));
    return SRN_OK;
}

void eval_segment_ms(const srn_eval_set* set, double* ms_segments, double* ms_segment_bootstrap) {
    if (ms_segments) *ms_segments = set->dev->ms_seg;
    if (ms_segment_bootstrap) *ms_segment_bootstrap = set->dev->ms_seg_boot;
}

}  // namespace srn
