// Trending items: which items the live sessions of a device store hold most often (include/serenade_hip.h, srn_device_sessions_top_items).
//
// count(id) = the number of in-range entries whose window holds id at least once; the ranking is count descending, id ascending.  Everything is exact integer work on
// the store's stream, under the store's mutex, behind its previous call; nothing in the store is written.
//   trend_windows<false>   per slot: the number of DISTINCT ids of its window if the entry is in range, else 0
//   exclusive scan         a slot's place in the dense array; the last word, read back, is the exact number of ids T
//   trend_windows<true>    every in-range entry's distinct ids, each at its first position, to its place
//   radix sort of the ids, run-length encode: (id ascending, count); the number of runs R is read back
//   radix sort of the runs by count, descending and stable: id stays ascending among equal counts
//   trend_cut              min_count, the first `cap` entries, and `ranked`
// A slot is read as sess_export_scatter reads it: as 16-byte elements (0 = the key, 1 = epoch | len | state, 2.. = item pairs) by 8 adjacent lanes for 128-byte slots and
// 16 for larger ones, lane e of the group reading element e, e + lanes, ... so a wave reads whole slots side by side.  An id is the first of its window iff no earlier
// position holds it: the group hands every pair of every earlier round to all its lanes by shuffle, so the comparison loops over the window, whatever its length.
//
// Scratch, allocated for the call and released: 12 * (slots + 1) bytes for the counts and places; then two u64 buffers of T, a u32 buffer of T, a u32 buffer of R and
// rocPRIM's temporaries (double-buffered sorts: no copy of the keys in them) -- 20 T + 4 R bytes and little more.  A store of 4 M sessions of 16 items: T = 64 M, about
// 1.3 GB for a moment.  T above 2^31 is refused (rocPRIM's run-length encode counts in 32 bits).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include <rocprim/rocprim.hpp>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_sessions_dev.h"   // the store's handle over srn_visitor_table.h: Table, SlotHead, align256, grid_for
#include "srn_hipsync.h"

namespace srn {

namespace {
constexpr uint32_t kTPB = kTableTPB;   // (grid_for)
constexpr const char* kWho = "srn_device_sessions_top_items";

struct TrendArgs {
    Table t;
    uint64_t now, ttl, since;
    uint32_t lanes_shift;    // 2^lanes_shift adjacent lanes read one slot, 16 bytes each per round
    uint32_t n_el;           // 16-byte elements of a slot that can hold a window: 2 + ceil(items_cap / 2)
    uint32_t* cnt;           // [n_slots + 1] count pass: distinct ids of the slot's window (0: not in range; cnt[n_slots] = 0)
    const uint64_t* pos;     // [n_slots + 1] emit pass: exclusive scan of cnt
    uint64_t* ids;           // [T] emit pass: the dense array
};

// No lane leaves early and every loop bound is the same across the wave: the shuffles and ballots below need all 64 lanes.
template <bool kEmit>
__global__ void __launch_bounds__(kTPB) trend_windows(TrendArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    const uint64_t slot = tid >> a.lanes_shift;
    const uint32_t lanes = 1u << a.lanes_shift, lane = (uint32_t)tid & (lanes - 1);
    const uint32_t gbase = (threadIdx.x & 63u) & ~(lanes - 1);   // the group's first lane in the wave
    uint32_t len = 0;                                            // 0: not in range -- no position is ever read
    const ulonglong2* el = nullptr;
    if (slot <= a.t.mask) {
        const SlotHead* s = slot_at(a.t, (uint32_t)slot);
        el = (const ulonglong2*)s;
        const uint64_t ep = s->epoch;
        if (s->state != kEmpty && !idle_or_old(a.now, ep, a.ttl) && ep >= a.since) len = s->len;
    }
    uint64_t base = 0;
    if (kEmit && len) base = a.pos[slot];
    const uint32_t rounds = (a.n_el + lanes - 1) >> a.lanes_shift;
    uint32_t total = 0;   // distinct ids of the rounds so far: the same in every lane of the group
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint32_t e = lane + (r << a.lanes_shift);
        const uint32_t j = 2 * (e - 2);                          // my pair's positions are j and j + 1 (e >= 2)
        const bool hx = e >= 2 && j < len, hy = e >= 2 && j + 1 < len;
        ulonglong2 v = make_ulonglong2(0, 0);
        if (hx) v = el[e];                                       // (j < len <= items_cap: the pair lies inside the slot)
        bool fx = hx, fy = hy && v.y != v.x;                     // first of the window so far
        for (uint32_t r2 = 0; r2 <= r; ++r2) {
            ulonglong2 w = v;
            if (r2 != r) {
                const uint32_t e2 = lane + (r2 << a.lanes_shift);
                w = make_ulonglong2(0, 0);
                if (e2 >= 2 && 2 * (e2 - 2) < len) w = el[e2];
            }
            for (uint32_t sl = 0; sl < lanes; ++sl) {
                const uint32_t es = sl + (r2 << a.lanes_shift);  // the element lane sl of the group holds in round r2
                if (es < 2) continue;
                if (es >= a.n_el) break;
                const uint64_t ox = __shfl(w.x, (int)(gbase + sl)), oy = __shfl(w.y, (int)(gbase + sl));
                const uint32_t px = 2 * (es - 2), py = px + 1;   // px is even like j, py odd: p < j + 1 is p < j for every position of ANOTHER pair
                if (px < len && px < j) { fx = fx && ox != v.x; fy = fy && ox != v.y; }
                if (py < len && py < j) { fx = fx && oy != v.x; fy = fy && oy != v.y; }
            }
        }
        const uint32_t gmask = (1u << lanes) - 1u;               // lanes <= 16
        const uint32_t gx = (uint32_t)(__ballot(fx) >> gbase) & gmask, gy = (uint32_t)(__ballot(fy) >> gbase) & gmask;
        if (kEmit) {   // in position order: the pairs of the lanes below, then x before y
            const uint32_t below = (1u << lane) - 1u;
            const uint64_t at = base + total + __popc(gx & below) + __popc(gy & below);
            if (fx) a.ids[at] = v.x;
            if (fy) a.ids[at + (fx ? 1u : 0u)] = v.y;
        }
        total += __popc(gx) + __popc(gy);
    }
    if (!kEmit && lane == 0 && slot <= (uint64_t)a.t.mask + 1u) a.cnt[slot] = total;
}

// The runs are sorted by count descending: the ranked ids are a prefix.  *ranked = its length; the first `take` entries of it are written.
__global__ void __launch_bounds__(kTPB) trend_cut(const uint32_t* __restrict__ cnt, const uint64_t* __restrict__ ids, uint32_t n_runs, uint32_t min_count, uint32_t take,
                                                  uint64_t* __restrict__ out_ids, uint32_t* __restrict__ out_cnt, uint64_t* __restrict__ ranked) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    if (i >= n_runs) return;
    const uint32_t c = cnt[i];
    const bool in = c >= min_count;
    if (i == 0 && !in) *ranked = 0;
    if (in && (i + 1 == n_runs || cnt[i + 1] < min_count)) *ranked = (uint64_t)i + 1;
    if (in && i < take) { out_ids[i] = ids[i]; out_cnt[i] = c; }
}

}  // namespace

int dsess_device_of(const srn_device_sessions* s) { return s->device; }

int dsess_top_items(srn_device_sessions* s, uint64_t now_secs, uint64_t since_secs, uint32_t min_count, size_t cap, uint64_t* out_ids, uint32_t* out_counts, size_t* out_n) {
    if (!s) return fail(SRN_EINVAL, std::string(kWho) + ": null store");
    if (!out_n) return fail(SRN_EINVAL, std::string(kWho) + ": null out_n");
    if (cap && !out_ids && !out_counts) return fail(SRN_EINVAL, std::string(kWho) + ": cap > 0 with no output array");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    if (min_count == 0) min_count = 1;
    std::lock_guard<std::mutex> g(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamWaitEvent(s->own, s->last, 0));
    hipStream_t st = s->own;
    *out_n = 0;
    int rc;
    // 1. distinct ids per slot, their places, the total
    const size_t n1 = (size_t)s->n_slots + 1;
    size_t tmp_scan = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_scan, (uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n1, rocprim::plus<uint64_t>(), st));
    Bump b1;
    const auto cnt_at = b1.of<uint32_t>(n1); const auto pos_at = b1.of<uint64_t>(n1); const auto scan_at = b1.of<char>(tmp_scan);
    StageBuf per_slot; if ((rc = per_slot.alloc(b1.bytes, kWho, "the scratch"))) return rc;
    TrendArgs a{};
    a.t = s->tab(); a.now = now; a.ttl = s->ttl; a.since = since_secs;
    a.lanes_shift = s->stride == 128 ? 3 : 4;
    a.n_el = 2 + (uint32_t)((s->items_cap + 1) / 2);
    a.cnt = cnt_at.at(per_slot.p); a.pos = pos_at.at(per_slot.p);
    const dim3 gw = grid_for(n1 << a.lanes_shift);
    trend_windows<false><<<gw, kTPB, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::exclusive_scan(scan_at.at(per_slot.p), tmp_scan, a.cnt, pos_at.at(per_slot.p), (uint64_t)0, n1, rocprim::plus<uint64_t>(), st));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, a.pos + s->n_slots, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (total == 0) return SRN_OK;
    if (total > (1ull << 31)) return fail(SRN_ERANGE, std::string(kWho) + ": more than 2^31 window entries in range");
    // 2. the dense array, sorted; 3. its runs
    const unsigned int T = (unsigned int)total;
    rocprim::double_buffer<uint64_t> ids((uint64_t*)nullptr, (uint64_t*)nullptr);
    size_t tmp_sort = 0, tmp_rle = 0;
    HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_sort, ids, T, 0, 64, st));
    HIP_TRY(rocprim::run_length_encode(nullptr, tmp_rle, (const uint64_t*)nullptr, T, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, st));
    const size_t tmp1 = std::max(tmp_sort, tmp_rle);
    Bump b2;   // (words: the number of runs, then the number of ranked ids)
    const auto idA = b2.of<uint64_t>(T), idB = b2.of<uint64_t>(T); const auto run_cnt_at = b2.of<uint32_t>(T); const auto words_at = b2.of<uint64_t>(2); const auto tmp1_at = b2.of<char>(tmp1);
    StageBuf per_id; if ((rc = per_id.alloc(b2.bytes, kWho, "the scratch"))) return rc;
    ids = rocprim::double_buffer<uint64_t>(idA.at(per_id.p), idB.at(per_id.p));
    uint32_t* run_cnt = run_cnt_at.at(per_id.p);
    uint64_t* d_ranked = words_at.at(per_id.p) + 1;
    uint32_t* d_runs = (uint32_t*)(d_ranked - 1);
    a.ids = ids.current();
    trend_windows<true><<<grid_for((size_t)s->n_slots << a.lanes_shift), kTPB, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    size_t t1 = tmp1;
    HIP_TRY(rocprim::radix_sort_keys(tmp1_at.at(per_id.p), t1, ids, T, 0, 64, st));
    t1 = tmp1;
    HIP_TRY(rocprim::run_length_encode(tmp1_at.at(per_id.p), t1, (const uint64_t*)ids.current(), T, ids.alternate(), run_cnt, d_runs, st));
    uint32_t R = 0;
    HIP_TRY(hipMemcpyAsync(&R, d_runs, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (R == 0 || R > T) return fail(SRN_EHIP, std::string(kWho) + ": the run-length encode returned an impossible number of runs");
    // 4. the runs by count, descending and stable (ids: the runs' ids | the buffer the sorted array was in); 5. the cut
    const size_t take = std::min<size_t>(cap, R);
    rocprim::double_buffer<uint32_t> keys(run_cnt, (uint32_t*)nullptr);
    rocprim::double_buffer<uint64_t> vals(ids.alternate(), ids.current());
    size_t tmp2 = 0;
    HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, tmp2, keys, vals, R, 0, 32, st));
    Bump b3;
    const auto keyB_at = b3.of<uint32_t>(R); const auto oid_at = b3.of<uint64_t>(take); const auto ocnt_at = b3.of<uint32_t>(take); const auto tmp2_at = b3.of<char>(tmp2);
    StageBuf per_run; if ((rc = per_run.alloc(b3.bytes, kWho, "the scratch"))) return rc;
    keys = rocprim::double_buffer<uint32_t>(run_cnt, keyB_at.at(per_run.p));
    HIP_TRY(rocprim::radix_sort_pairs_desc(tmp2_at.at(per_run.p), tmp2, keys, vals, R, 0, 32, st));
    uint64_t* d_oid = oid_at.at(per_run.p); uint32_t* d_ocnt = ocnt_at.at(per_run.p);
    trend_cut<<<grid_for(R), kTPB, 0, st>>>(keys.current(), vals.current(), R, min_count, (uint32_t)take, d_oid, d_ocnt, d_ranked);
    HIP_TRY(hipGetLastError());
    uint64_t ranked = 0;
    HIP_TRY(hipMemcpyAsync(&ranked, d_ranked, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t give = std::min<size_t>(take, ranked);
    if (give && out_ids) HIP_TRY(hipMemcpyAsync(out_ids, d_oid, give * 8, hipMemcpyDeviceToHost, st));
    if (give && out_counts) HIP_TRY(hipMemcpyAsync(out_counts, d_ocnt, give * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out_n = (size_t)ranked;
    return SRN_OK;
}

}  // namespace srn
