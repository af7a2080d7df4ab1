// =====================================================================================
// The device result cache of an index: predict_next is a pure function of the index, the call's parameters and the query's item sequence, so a served row
// may be kept in HBM and copied to a later call's query with the same sequence -- opt-in (srn_index_result_cache_enable), bound to ONE (k, m, how_many, business flag),
// used by the batch launch sequence exactly where its fast path is (srn_runtime.hip: make_plan).
//
//   the table   n_buckets buckets of RC_WAYS entries.  An entry: use stamp (0 = empty, else the number of the last call that stored or hit it) | length | count |
//               max_len raw 64-bit ids | how_many ids | how_many scores -- arrays of their own, entry e = bucket * RC_WAYS + way.
//   vmis_rcache_lookup_kernel   behind the grouping of equal queries, ahead of the sort of the order keys; one wave per query, over representatives only.  Lane l compares
//               item l % max_len of way l / max_len: the FULL key, (length, ids in order) -- hash equality alone never hits.  On a hit lane j copies entry j of the row,
//               the count word gets the real count (no finish kernel looks at the row), the order key becomes 0xFFFF << 32 | q (behind every query that is served: the
//               fast kernel's ordered loop ends before them, FastParams::order_dups) and the entry's stamp becomes this call's number.
//   vmis_rcache_insert_kernel   last of the launch sequence: every cacheable representative that missed and was served (count != 0xFFFFFFFF; 0 is a row) stores key and
//               row in an empty way, else in the way with the oldest stamp.  The way is CLAIMED with an agent-scope atomicCAS on its stamp (old -> this call's number);
//               a loser looks at the stamp it got back and tries the next oldest; it gives up only when no way older than this call is left.
//
// Visibility.  The per-XCD L2s are not coherent and nothing here publishes an entry to another workgroup inside a kernel: entries are written by the insert kernel and read
// by the lookup kernel of a LATER launch.  Inside the insert kernel only the stamps are shared, only through atomics (a stale look costs one failed CAS, which returns the
// word's real value).  Kernels of calls on different streams are chained in enqueue order by the cache's one event: wait, enqueue, record, under the cache's host mutex.
// Two equal sequences that miss in one call (no merging below SRN_ORDER_MIN) or in two overlapping calls land in two ways: harmless -- both hold the same row, the lookup
// takes the first, the other ages out.
// =====================================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "srn_runtime.h"
#include "srn_device.h"
#include "srn_hipsync.h"   // (last: hipFree / hipDeviceSynchronize make the resident latency-path workgroups leave first)

namespace srn {

namespace {
static constexpr uint32_t RC_QPW = 8;   // queries per wave: a wave's counters reach the device words once

__device__ __forceinline__ uint32_t rc_bucket(const ResultCacheView& c, const uint64_t* __restrict__ it, uint32_t L) {
    uint64_t h = dev_mix64(0xD6E8FEB86659FD93ull + L);
    for (uint32_t i = 0; i < L; ++i) h = dev_mix64(h ^ it[i]) + 0x9E3779B97F4A7C15ull;   // (chained: the order of the items counts)
    return ((uint32_t)(h >> 32) & c.hash_mask) % c.n_buckets;
}
// the way of `bucket` that holds (L, it[0..L)), or -1; wave-uniform
__device__ __forceinline__ int rc_find(const ResultCacheView& c, uint32_t bucket, const uint64_t* __restrict__ it, uint32_t L, uint32_t lane) {
    const uint32_t ML = c.max_len, j = lane / ML, i = lane - j * ML;
    bool bad = false;
    if (lane < RC_WAYS * ML) {
        const size_t e = (size_t)bucket * RC_WAYS + j;
        if (i == 0u) bad = c.len[e] != L;
        if (i < L) bad = bad || c.keys[e * ML + i] != it[i];
    }
    const unsigned long long b = __ballot(bad), grp = (1ull << ML) - 1ull;
    for (uint32_t w = 0; w < RC_WAYS; ++w) if (((b >> (w * ML)) & grp) == 0ull) return (int)w;
    return -1;
}
__device__ __forceinline__ bool rc_cacheable(const ResultCacheView& c, uint32_t L, uint32_t call_max_len) { return L >= 1u && L <= c.max_len && L <= call_max_len; }
}  // namespace

__global__ __launch_bounds__(256) void vmis_rcache_lookup_kernel(ResultCacheView c, const uint64_t* __restrict__ items_flat, const uint32_t* __restrict__ q_off, uint32_t nq, uint32_t call_max_len,
                                                                 const uint32_t* __restrict__ rep, unsigned long long* okeys, uint64_t* out_ids, double* out_scores, uint32_t* out_counts,
                                                                 uint32_t now, const uint32_t* n_dup, uint32_t* n_skip) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t q_first = (uint64_t)wave * RC_QPW;
    const uint32_t hm = c.how_many;
    uint32_t looked = 0u, hits = 0u;
    for (uint32_t t = 0; t < RC_QPW && q_first + t < nq; ++t) {
        const uint32_t q = (uint32_t)q_first + t;
        if (rep != nullptr && rep[q] != q) continue;   // (a merged query: its key is 0xFFFF already, its row comes from the representative's at the end)
        const uint32_t qb = q_off[q], L = q_off[q + 1] - qb;
        int way = -1; uint32_t bucket = 0u;
        if (rc_cacheable(c, L, call_max_len)) { ++looked; bucket = rc_bucket(c, items_flat + qb, L); way = rc_find(c, bucket, items_flat + qb, L, lane); }
        if (way < 0) {   // served by the kernels: in front of the merged queries and the hits
            if (lane == 0u && (okeys[q] >> 32) >= 0xFFFFull) okeys[q] = (0xFFFEull << 32) | q;
            continue;
        }
        ++hits;
        const size_t e = (size_t)bucket * RC_WAYS + (uint32_t)way;
        const uint32_t cnt = c.count[e], n = min(cnt, hm);
        for (uint32_t j = lane; j < n; j += 64u) { out_ids[(size_t)q * hm + j] = c.ids[e * hm + j]; out_scores[(size_t)q * hm + j] = c.scores[e * hm + j]; }
        if (lane == 0u) {
            out_counts[q] = cnt; okeys[q] = (0xFFFFull << 32) | q;
            __hip_atomic_store(&c.stamp[e], now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (lane == 0u) {
        if (looked) atomicAdd(&c.counters[RC_LOOKUPS], (unsigned long long)looked);
        if (hits) { atomicAdd(&c.counters[RC_HITS], (unsigned long long)hits); atomicAdd(n_skip, hits); }
        if (wave == 0u && n_dup != nullptr) atomicAdd(n_skip, *n_dup);   // (final: the grouping pass is over)
    }
}

__global__ __launch_bounds__(256) void vmis_rcache_insert_kernel(ResultCacheView c, const uint64_t* __restrict__ items_flat, const uint32_t* __restrict__ q_off, uint32_t nq, uint32_t call_max_len,
                                                                 const uint32_t* __restrict__ rep, const unsigned long long* __restrict__ okeys, const uint64_t* __restrict__ out_ids,
                                                                 const double* __restrict__ out_scores, const uint32_t* __restrict__ out_counts, uint32_t now) {
    const uint32_t lane = threadIdx.x & 63u, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t q_first = (uint64_t)wave * RC_QPW;
    const uint32_t hm = c.how_many, ML = c.max_len;
    uint32_t stored = 0u, evicted = 0u;
    for (uint32_t t = 0; t < RC_QPW && q_first + t < nq; ++t) {
        const uint32_t q = (uint32_t)q_first + t;
        if (rep != nullptr && rep[q] != q) continue;
        const uint32_t qb = q_off[q], L = q_off[q + 1] - qb;
        if (!rc_cacheable(c, L, call_max_len) || (okeys[q] >> 32) == 0xFFFFull) continue;   // (0xFFFF on a representative: the lookup kernel's hit)
        const uint32_t cnt = out_counts[q];
        if (cnt == 0xFFFFFFFFu) continue;   // not served: nothing to keep
        const uint32_t bucket = rc_bucket(c, items_flat + qb, L);
        uint32_t* const stamps = c.stamp + (size_t)bucket * RC_WAYS;
        uint32_t st = lane < RC_WAYS ? __hip_atomic_load(&stamps[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0xFFFFFFFFu;
        int way = -1; uint32_t old = 0u;
        for (uint32_t round = 0; round <= RC_WAYS && way < 0; ++round) {
            // the oldest way among those older than this call (an empty way's stamp is 0: the oldest of all)
            unsigned long long best = lane < RC_WAYS && st < now ? ((unsigned long long)st << 8) | lane : ~0ull;
            for (int d = 1; d < (int)RC_WAYS; d <<= 1) { const unsigned long long o = __shfl_xor(best, d); best = o < best ? o : best; }
            best = __shfl(best, 0);
            if (best == ~0ull) break;
            const uint32_t w = (uint32_t)(best & 0xFFull), seen = (uint32_t)(best >> 8);
            uint32_t got = 0u;
            if (lane == w) { got = atomicCAS(&stamps[w], seen, now); st = got == seen ? now : got; }
            got = __shfl(got, (int)w);
            if (got == seen) { way = (int)w; old = seen; }
        }
        if (way < 0) continue;
        ++stored; evicted += old != 0u ? 1u : 0u;
        const size_t e = (size_t)bucket * RC_WAYS + (uint32_t)way;
        if (lane < ML) c.keys[e * ML + lane] = lane < L ? items_flat[qb + lane] : 0ull;
        if (lane == 0u) { c.len[e] = L; c.count[e] = cnt; }
        const uint32_t n = min(cnt, hm);
        for (uint32_t j = lane; j < n; j += 64u) { c.ids[e * hm + j] = out_ids[(size_t)q * hm + j]; c.scores[e * hm + j] = out_scores[(size_t)q * hm + j]; }
    }
    if (lane == 0u) {
        if (stored) atomicAdd(&c.counters[RC_INSERTS], (unsigned long long)stored);
        if (evicted) atomicAdd(&c.counters[RC_EVICTIONS], (unsigned long long)evicted);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------------
ResultCache::~ResultCache() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();   // (device-pointer calls return with their kernels in flight)
    if (ev) (void)hipEventDestroy(ev);
    if (own) (void)hipStreamDestroy(own);
    if (mem) (void)hipFree(mem);
}

static std::shared_ptr<ResultCache> rcache_of(DeviceState* d) { std::lock_guard<std::mutex> lk(d->mu); return d->rcache; }
std::shared_ptr<ResultCache> device_result_cache(DeviceState* d) { return d ? rcache_of(d) : nullptr; }

int device_result_cache_enable(DeviceState* d, uint64_t rows, uint32_t max_len, uint32_t k, uint32_t m, uint32_t how_many, uint32_t flags) {
    if (rows == 0) return fail(SRN_EINVAL, "result cache: rows must be > 0");
    if (max_len < 1u || max_len > RC_MAX_LEN) return fail(SRN_ERANGE, "result cache: max_len must be 1..8");
    if (rows > (1ull << 28)) return fail(SRN_ERANGE, "result cache: more than 2^28 rows");
    if (rcache_of(d)) return fail(SRN_ESTATE, "result cache: already enabled on this index (srn_index_result_cache_disable first)");
    HIP_TRY(hipSetDevice(d->device));
    auto rc = std::make_shared<ResultCache>();
    rc->device = d->device; rc->k = k; rc->m = m; rc->how_many = how_many; rc->flags = flags & SRN_FLAG_BUSINESS_LOGIC;
    ResultCacheView& v = rc->view;
    v.n_buckets = (uint32_t)((rows + RC_WAYS - 1) / RC_WAYS); v.max_len = max_len; v.how_many = how_many;
    v.hash_mask = 0xFFFFFFFFu;
    const size_t R = (size_t)v.n_buckets * RC_WAYS;
    Bump b;
    const auto r_cnt = b.take<unsigned long long>(RC_COUNTERS * 8); const auto r_stamp = b.take<uint32_t>(R * 4), r_len = b.take<uint32_t>(R * 4), r_count = b.take<uint32_t>(R * 4);
    const auto r_keys = b.take<uint64_t>(R * max_len * 8), r_ids = b.take<uint64_t>(R * how_many * 8); const auto r_sc = b.take<double>(R * how_many * 8);
    const size_t off = b.bytes;
    // (everything the cache will ever need is allocated HERE: hipMalloc synchronises the device, the calls allocate nothing for it)
    if (hipMalloc((void**)&rc->mem, off) != hipSuccess) { (void)hipGetLastError(); rc->mem = nullptr; return fail(SRN_ENOMEM, "result cache: hipMalloc failed"); }
    rc->bytes = off; rc->stamp_bytes = r_count.off - r_stamp.off;   // (stamps and lengths are adjacent: one memset empties the table)
    v.counters = r_cnt.at(rc->mem); v.stamp = r_stamp.at(rc->mem); v.len = r_len.at(rc->mem); v.count = r_count.at(rc->mem);
    v.keys = r_keys.at(rc->mem); v.ids = r_ids.at(rc->mem); v.scores = r_sc.at(rc->mem);
    HIP_TRY(hipEventCreateWithFlags(&rc->ev, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&rc->own, hipStreamNonBlocking));
    HIP_TRY(hipMemsetAsync(rc->mem, 0, off, rc->own));
    HIP_TRY(hipStreamSynchronize(rc->own));
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->rcache) return fail(SRN_ESTATE, "result cache: already enabled on this index (srn_index_result_cache_disable first)");
    d->rcache = rc;
    return SRN_OK;
}
int device_result_cache_disable(DeviceState* d) {
    std::shared_ptr<ResultCache> rc;
    { std::lock_guard<std::mutex> lk(d->mu); rc.swap(d->rcache); }
    return SRN_OK;   // (freed when the last call that holds it has returned: ~ResultCache waits for the device)
}
// empties the table: behind every cache kernel enqueued so far, ahead of every later one (the cache's event chain)
static int rcache_clear_locked(ResultCache* rc) {
    HIP_TRY(hipStreamWaitEvent(rc->own, rc->ev, 0));
    HIP_TRY(hipMemsetAsync(rc->view.stamp, 0, rc->stamp_bytes, rc->own));
    HIP_TRY(hipEventRecord(rc->ev, rc->own));
    HIP_TRY(hipStreamSynchronize(rc->own));
    rc->seq = 0;
    return SRN_OK;
}
int device_result_cache_clear(DeviceState* d) {
    auto rc = rcache_of(d);
    if (!rc) return fail(SRN_ESTATE, "result cache: not enabled");
    HIP_TRY(hipSetDevice(d->device));
    std::lock_guard<std::mutex> lk(rc->mu);
    const int r = rcache_clear_locked(rc.get());
    if (r == SRN_OK) rc->clears.fetch_add(1, std::memory_order_relaxed);
    return r;
}
int device_result_cache_clear_if_enabled(DeviceState* d) { return rcache_of(d) ? device_result_cache_clear(d) : SRN_OK; }
void device_result_cache_bypassed(DeviceState* d) {
    if (auto rc = rcache_of(d)) rc->bypassed.fetch_add(1, std::memory_order_relaxed);
}
int device_result_cache_stats(DeviceState* d, srn_result_cache_stats_t* out) {
    auto rc = rcache_of(d);
    if (!rc) return fail(SRN_ESTATE, "result cache: not enabled");
    HIP_TRY(hipSetDevice(d->device));
    unsigned long long w[RC_COUNTERS] = {};
    { std::lock_guard<std::mutex> lk(rc->mu);
      HIP_TRY(hipStreamWaitEvent(rc->own, rc->ev, 0));   // (behind the last cache kernel of any stream)
      HIP_TRY(hipMemcpyAsync(w, rc->view.counters, sizeof(w), hipMemcpyDeviceToHost, rc->own));
      HIP_TRY(hipStreamSynchronize(rc->own)); }
    memset(out, 0, sizeof(*out));
    out->rows = (uint64_t)rc->view.n_buckets * RC_WAYS; out->ways = RC_WAYS; out->bytes = rc->bytes; out->max_len = rc->view.max_len;
    out->k = rc->k; out->m = rc->m; out->how_many = rc->how_many; out->flags = rc->flags;
    out->lookups = w[RC_LOOKUPS]; out->hits = w[RC_HITS]; out->inserts = w[RC_INSERTS]; out->evictions = w[RC_EVICTIONS];
    out->bypassed_calls = rc->bypassed.load(std::memory_order_relaxed); out->clears = rc->clears.load(std::memory_order_relaxed);
    return SRN_OK;
}

// (hash_bits: SRN_CACHE_HASH_BITS as the call's plan read it -- an entry stored under another cut is simply not found)
static ResultCacheView rc_view(const ResultCache* rc, int hash_bits) { ResultCacheView v = rc->view; v.hash_mask = hash_bits >= 1 && hash_bits < 32 ? (1u << hash_bits) - 1u : 0xFFFFFFFFu; return v; }
static uint32_t rc_grid(uint32_t nq) { return (uint32_t)(((uint64_t)nq + 4u * RC_QPW - 1u) / (4u * RC_QPW)); }   // (256 threads: four waves of RC_QPW queries)
int rcache_enqueue_lookup(ResultCache* rc, hipStream_t st, const LaunchParams& p, const uint32_t* rep, unsigned long long* okeys, const uint32_t* n_dup, uint32_t* n_skip, int hash_bits, uint32_t* now_out) {
    HIP_TRY(hipMemsetAsync(n_skip, 0, 4, st));
    std::lock_guard<std::mutex> lk(rc->mu);
    if (rc->seq >= 0xFFFFFFF0u) { int r = rcache_clear_locked(rc); if (r) return r; }   // (the stamps are 32-bit call numbers: start over)
    const uint32_t now = ++rc->seq; *now_out = now;
    HIP_TRY(hipStreamWaitEvent(st, rc->ev, 0));
    hipLaunchKernelGGL(vmis_rcache_lookup_kernel, dim3(rc_grid(p.nq)), dim3(256), 0, st, rc_view(rc, hash_bits), p.items_flat, p.q_off, p.nq, p.max_len, rep, okeys, p.out_ids, p.out_scores, p.out_counts, now, n_dup, n_skip);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(rc->ev, st));
    return SRN_OK;
}
int rcache_enqueue_insert(ResultCache* rc, hipStream_t st, const LaunchParams& p, const uint32_t* rep, const unsigned long long* okeys, int hash_bits, uint32_t now) {
    std::lock_guard<std::mutex> lk(rc->mu);
    HIP_TRY(hipStreamWaitEvent(st, rc->ev, 0));
    hipLaunchKernelGGL(vmis_rcache_insert_kernel, dim3(rc_grid(p.nq)), dim3(256), 0, st, rc_view(rc, hash_bits), p.items_flat, p.q_off, p.nq, p.max_len, rep, okeys, (const uint64_t*)p.out_ids, (const double*)p.out_scores,
                       (const uint32_t*)p.out_counts, now);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(rc->ev, st));
    return SRN_OK;
}

}  // namespace srn
