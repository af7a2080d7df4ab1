// =====================================================================================
// Short rows filled from a fallback ranking: "a row can be short or empty -- append the best sellers".
//
// An index may carry a fallback ranking F of up to SRN_MAX_FALLBACK distinct public item ids (srn_index_set_fallback*): the ids and, per entry, its dense item index
// (0xFFFFFFFF: the index does not know the id) in device memory.  With SRN_FLAG_FILL a batch call runs its launch sequence -- and the exclusion filter, where it has one --
// unchanged, and one kernel behind them, on the same stream and in place on the caller's rows, appends to every row of c < how_many entries the first how_many - c entries
// of F that the call would not have removed from the model's candidates either: not one of the row's c ids, not the session's most recent item r, not in the query's
// exclusion list (for srn_recommend_batch with SRN_FLAG_EXCLUDE_SEEN: the request's window), not in the session with SRN_FLAG_EXCLUDE_SESSION, and, under the business
// rules, passes_business_rules(attr(r), attr(f)).  Filled entries carry the score -infinity; counts[q] = c + filled.
//
//   vmis_fill_kernel      one wave of 64 lanes per query, four queries per workgroup of 256 threads.  The wave reads counts[q] first and leaves when the row is full or
//                         0xFFFFFFFF: on a stream without short rows the kernel is a read of the counts array.  A short row walks F in chunks of 64, one candidate per lane
//                         (one coalesced 512-byte read); what a candidate is compared with -- the row's c ids, the exclusion list, the session's items (with the flag:
//                         all of them; without: r alone) -- is loaded 64 ids per pass, one per lane, and broadcast lane by lane (two v_readlane on a wave-uniform index).
//                         Under the business rules a lane gathers meta[dense idx].attr; r's attribute byte comes from the id table once per query.  The keep mask's
//                         ballot ranks the kept candidates (mbcnt), which are written -- id and -inf -- at c + written + rank while that is below how_many.  The walk ends
//                         when the row is full or F exhausted; lane 0 writes the new count.  Every loop bound (c, the lists' lengths, R) is wave-uniform: the query
//                         number goes through v_readfirstlane, so they live in scalar registers.  No LDS, no scratch memory.
// =====================================================================================
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>

#include "srn_device.h"
#include "srn_runtime.h"

namespace srn {

namespace {
__device__ __forceinline__ uint64_t lane_bcast64(uint64_t v, uint32_t j) {   // lane j's value to every lane; j is wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)j), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)j);
    return ((uint64_t)hi << 32) | lo;
}
// keep &= id is none of base[0 .. n): 64 ids per pass, one per lane, broadcast lane by lane (n wave-uniform)
__device__ __forceinline__ bool none_of(bool keep, uint64_t id, const uint64_t* __restrict__ base, uint32_t n, uint32_t lane) {
    for (uint32_t tb = 0u; tb < n; tb += 64u) {
        const uint32_t nt = min(n - tb, 64u);
        const uint64_t v = lane < nt ? base[tb + lane] : 0ull;
        for (uint32_t j = 0u; j < nt; ++j) { const uint64_t b = lane_bcast64(v, j); keep = keep && id != b; }   // (the broadcast is made by every lane, kept or not)
    }
    return keep;
}
}  // namespace

__global__ __launch_bounds__(256) void vmis_fill_kernel(uint32_t nq, uint64_t* __restrict__ ids, double* __restrict__ scores, uint32_t* __restrict__ counts, uint32_t how_many,
                                                        const uint64_t* __restrict__ fb_ids, const uint32_t* __restrict__ fb_idx, uint32_t R,
                                                        const uint64_t* __restrict__ x_flat, const uint32_t* __restrict__ x_off,
                                                        const uint64_t* __restrict__ items_flat, const uint32_t* __restrict__ q_off, uint32_t whole_session, uint32_t business,
                                                        const ItemMeta* __restrict__ meta, const IdSlot* __restrict__ id_table, uint32_t id_mask) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));   // (wave-uniform, and known to be)
    if (q >= nq) return;
    const uint32_t c = counts[q];
    if (c >= how_many) return;   // a full row, or 0xFFFFFFFF (not served): not touched
    const uint32_t se = q_off[q + 1], s0 = q_off[q];
    if (se <= s0) return;        // (an empty session is marked 0xFFFFFFFF by the launch sequence: never here)
    const uint32_t sb = whole_session ? s0 : se - 1u, sn = se - sb;   // what of the session a candidate is compared with: all of it, or the most recent item alone
    uint32_t xb = 0u, xn = 0u;
    if (x_flat) { xb = x_off[q]; xn = x_off[q + 1] - xb; }
    uint32_t cur_attr = SRN_ATTR_NONE;
    if (business && id_table) {   // attr(r): None for an item the index does not know
        const uint64_t r = items_flat[se - 1u];
        uint32_t hh = (uint32_t)dev_mix64(r) & id_mask;
        for (;;) { const IdSlot s = id_table[hh]; if (s.idx == kNone) break; if (s.key == r) { cur_attr = meta[s.idx].attr; break; } hh = (hh + 1u) & id_mask; }
    }
    uint64_t* __restrict__ ri = ids + (size_t)q * how_many; double* __restrict__ rs = scores + (size_t)q * how_many;
    const double ninf = -std::numeric_limits<double>::infinity();
    uint32_t at = c;   // entries of the row so far
    for (uint32_t fb = 0u; fb < R && at < how_many; fb += 64u) {
        const uint32_t e = fb + lane;
        bool keep = e < R;
        const uint64_t id = keep ? fb_ids[e] : 0ull;
        if (business) {
            const uint32_t di = keep ? fb_idx[e] : kNone;   // (an id the index does not know has no attributes: dropped)
            uint32_t a = SRN_ATTR_NONE;
            if (di != kNone) a = meta[di].attr;
            keep = keep && business_ok(cur_attr, a);
        }
        keep = none_of(keep, id, items_flat + sb, sn, lane);
        keep = none_of(keep, id, ri, c, lane);   // (the c model entries only: what this wave appends comes from F, whose ids are distinct)
        if (xn) keep = none_of(keep, id, x_flat + xb, xn, lane);
        const unsigned long long mask = __ballot(keep);
        const uint32_t pos = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (keep && pos < how_many) { ri[pos] = id; rs[pos] = ninf; }
        at += (uint32_t)__popcll(mask);
    }
    if (lane == 0u && at != c) counts[q] = min(at, how_many);
}

hipError_t launch_fill(hipStream_t st, const DeviceState* d, uint32_t nq, uint64_t* ids, double* scores, uint32_t* counts, uint32_t how_many, const uint64_t* x_flat, const uint32_t* x_off,
                       const uint64_t* items_flat, const uint32_t* q_off, bool whole_session, bool business) {
    hipLaunchKernelGGL(vmis_fill_kernel, dim3((nq + 3u) / 4u), dim3(256), 0, st, nq, ids, scores, counts, how_many, (const uint64_t*)d->fb_ids, (const uint32_t*)d->fb_idx,
                       d->fb_n.load(std::memory_order_acquire), x_flat, x_off, items_flat, q_off, whole_session ? 1u : 0u, business ? 1u : 0u, d->di.meta, d->di.id_table, d->di.id_mask);
    return hipGetLastError();
}

bool device_has_fallback(const DeviceState* d) { return d && d->fb_n.load(std::memory_order_acquire) != 0u; }

// The ranking's device copy: ids [SRN_MAX_FALLBACK] | dense indices [SRN_MAX_FALLBACK], allocated once (48 KB) and overwritten by a later ranking -- behind whatever
// is in flight on the device, which may still read the old one (like device_update_attr: the caller keeps calls on the index away meanwhile)
int device_set_fallback(DeviceState* d, const FlatIndex& ix, const uint64_t* item_ids, uint32_t n) {
    HIP_TRY(hipSetDevice(d->device));
    if (!d->fb_ids) {
        void* mem = nullptr;
        const size_t bytes = (size_t)SRN_MAX_FALLBACK * 12;
        if (hipMalloc(&mem, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(SRN_ENOMEM, "fallback ranking: hipMalloc failed"); }
        d->allocs.push_back(mem); d->bytes += bytes;
        d->fb_ids = (uint64_t*)mem; d->fb_idx = (uint32_t*)((char*)mem + (size_t)SRN_MAX_FALLBACK * 8);
    }
    std::vector<uint32_t> dense(n);
    for (uint32_t i = 0; i < n; ++i) dense[i] = ix.lookup(item_ids[i]);
    d->fb_n.store(0u, std::memory_order_release);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(d->fb_ids, item_ids, (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d->fb_idx, dense.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    d->fb_n.store(n, std::memory_order_release);
    return SRN_OK;
}
void device_clear_fallback(DeviceState* d) { if (d) d->fb_n.store(0u, std::memory_order_release); }

// measurement aid (srn_debug_fill): the fill kernel alone over the caller's rows, enqueued on `stream`
int device_fill(DeviceState* d, uint32_t nq, uint64_t* ids, double* scores, uint32_t* counts, uint32_t how_many, const uint64_t* x_flat, const uint32_t* x_off,
                const uint64_t* items_flat, const uint32_t* q_off, bool whole_session, bool business, void* stream) {
    HIP_TRY(hipSetDevice(d->device));
    if (nq == 0) return SRN_OK;
    HIP_TRY(launch_fill((hipStream_t)stream, d, nq, ids, scores, counts, how_many, x_flat, x_off, items_flat, q_off, whole_session, business));
    return SRN_OK;
}

}  // namespace srn
