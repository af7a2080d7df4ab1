// What a batch against a table keyed by visitor needs (srn_sessions_dev.hip, srn_feedback.hip, srn_harvest.hip): the run predicates over a batch sorted by visitor,
// the find-or-claim probe of a batch's run heads, the stable sort of 128-bit keys that makes the runs, and what the batch calls of the store and the log open with:
// the sorted front of a request descriptor (VisitorBatch, srn_internal.h), the timed / untimed dispatch and the host stage of the descriptor's arrays.  The table, its
// capacity rule and the scratch's grow rule are srn_visitor_table.h's.  No relocatable device code: every kernel here is a template, every function inline.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include <rocprim/rocprim.hpp>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_device.h"
#include "srn_visitor_table.h"   // the table itself: SlotHead, Table, the slot states, key_hash

namespace srn {

// ---- runs: a batch sorted by (no consent, key_hi, key_lo) holds the consenting requests of one visitor as one contiguous run, in request order ----
// A: a kernel's arguments with order[n] (request index of each sorted position), consent (null: every request consents), key_hi, key_lo and n
template <class A> __device__ __forceinline__ bool consents(const A& a, uint32_t req) { return a.consent == nullptr || a.consent[req] != 0; }
// is `other` a consenting request of the visitor (hi, lo)
template <class A> __device__ __forceinline__ bool same_visitor(const A& a, uint32_t other, uint64_t hi, uint64_t lo) {
    return consents(a, other) && a.key_hi[other] == hi && a.key_lo[other] == lo;
}
// A consenting request of the visitor (hi, lo) at sorted position p: the run's previous request, or kNone where p is the run's head.  The caller loads the key
// before the call and keeps the predecessor it gets: a kernel that goes on to read the predecessor's item or row must not wait for order[p - 1] a second time
template <class A> __device__ __forceinline__ uint32_t run_prev(const A& a, uint32_t p, uint64_t hi, uint64_t lo) {
    if (p == 0) return kNone;
    const uint32_t pr = a.order[p - 1];
    return same_visitor(a, pr, hi, lo) ? pr : kNone;
}
// The consenting request req at sorted position p: is p its run's head / its run's last request.  For the kernels that need the key for nothing else: it is read
// only as far as the comparison gets
template <class A> __device__ __forceinline__ bool same_visitor(const A& a, uint32_t other, uint32_t req) {
    return consents(a, other) && a.key_hi[other] == a.key_hi[req] && a.key_lo[other] == a.key_lo[req];
}
template <class A> __device__ __forceinline__ bool run_head(const A& a, uint32_t p, uint32_t req) { return p == 0 || !same_visitor(a, a.order[p - 1], req); }
template <class A> __device__ __forceinline__ bool run_last(const A& a, uint32_t p, uint32_t req) { return p + 1 >= a.n || !same_visitor(a, a.order[p + 1], req); }

// ---- find-or-claim: one lane per run head of a batch ----
// Both tables' slots begin { key_hi u64 | key_lo u64 | epoch u64 | u32 | state u32 } (SlotHead; table_rebuild asserts it of every owner's slot), so the probe reads
// them as SlotHead.  The claim protocol: CAS empty -> claimed.  Two heads never hold the same key, so a slot claimed during the kernel belongs to another key and the loser
// of a claim probes on: nobody waits for anybody.  A slot in state kFull was complete before the kernel began and its key can be compared.
// -> the slot, and whether it was claimed here (the caller writes the key and its own fields; state stays kClaimed until the call's store kernel) or found kFull (the
// caller reads it); slot kNone: the table is full -- cannot happen under the capacity rule.
struct Claim { uint32_t slot; bool fresh; };
__device__ __forceinline__ Claim find_or_claim(const Table& t, uint64_t hi, uint64_t lo) {
    uint32_t h = key_hash(hi, lo) & t.mask;
    for (uint32_t probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        SlotHead* s = slot_at(t, h);
        uint32_t st = __hip_atomic_load(&s->state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st == kEmpty) {
            st = atomicCAS(&s->state, kEmpty, kClaimed);
            if (st == kEmpty) return Claim{h, true};
        }
        if (st == kFull && s->key_hi == hi && s->key_lo == lo) return Claim{h, false};
    }
    return Claim{kNone, false};
}

// ---- the key sort: stable LSD radix passes over one 64-bit word each, least significant word first; idx ends as the order ----
constexpr uint32_t kKeyTPB = 256;
// a pass's word for entry e: a 64-bit array's, or a one-bit predicate (srn_harvest.hip has one of its own)
struct KeyWord { const uint64_t* src; __device__ __forceinline__ uint64_t operator()(uint32_t e) const { return src[e]; } };
struct KeyNoConsent { const uint8_t* consent; __device__ __forceinline__ uint64_t operator()(uint32_t e) const { return consent[e] ? 0ull : 1ull; } };

__global__ static void __launch_bounds__(kKeyTPB) key_init(const uint64_t* __restrict__ src, uint32_t n, uint64_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const uint32_t i = blockIdx.x * kKeyTPB + threadIdx.x;
    if (i < n) { key[i] = src[i]; idx[i] = i; }
}
// out[i] = word(idx[i]): a pass's keys through the current order (and a timed batch's times through the final one)
template <class W> __global__ void __launch_bounds__(kKeyTPB) key_gather(W word, const uint32_t* __restrict__ idx, uint32_t n, uint64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kKeyTPB + threadIdx.x;
    if (i < n) out[i] = word(idx[i]);
}

// rocPRIM's temporary storage for the passes of n entries (64-bit and 1-bit)
inline int key_sort_tmp_bytes(size_t n, hipStream_t st, size_t* bytes) {
    size_t wide = 0, bit = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, wide, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 64, st));
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, bit, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 1, st));
    *bytes = std::max(wide, bit);
    return SRN_OK;
}
// the caller's scratch: two key buffers and two index buffers of n entries, and tmp_bytes >= key_sort_tmp_bytes(n) at tmp.  order(): the indices behind the last pass
struct KeySort {
    uint64_t* key[2]; uint32_t* idx[2]; char* tmp; size_t tmp_bytes;
    size_t n; hipStream_t st;
    int cur = 0;
    const uint32_t* order() const { return idx[cur]; }
    dim3 grid() const { return dim3((unsigned)((std::max<size_t>(n, 1) + kKeyTPB - 1) / kKeyTPB)); }
    int sort(unsigned begin_bit, unsigned end_bit) {
        size_t t = tmp_bytes;
        HIP_TRY(rocprim::radix_sort_pairs(tmp, t, key[0], key[1], idx[cur], idx[cur ^ 1], n, begin_bit, end_bit, st));
        cur ^= 1;
        return SRN_OK;
    }
    // the first pass: all 64 bits of first[0 .. n)
    int begin(const uint64_t* first) {
        cur = 0;
        key_init<<<grid(), kKeyTPB, 0, st>>>(first, (uint32_t)n, key[0], idx[0]);
        return sort(0, 64);
    }
    // a further pass: bits [begin_bit, end_bit) of word(entry), gathered through the current order
    template <class W> int pass(W word, unsigned begin_bit = 0, unsigned end_bit = 64) {
        key_gather<<<grid(), kKeyTPB, 0, st>>>(word, idx[cur], (uint32_t)n, key[0]);
        return sort(begin_bit, end_bit);
    }
};

// ---- the sorted front: a request descriptor -> the batch sorted by (no consent, key_hi, key_lo) ----
// Two phases, around the owner's scratch growing.  plan() declares the front's regions on the owner's Bump: two key and two index buffers, rocPRIM's temporary storage
// -- the sort's, or scan_bytes for the owner's scans where those need more -- and, for a timed batch, the times in sorted order.  run(base), once the buffer stands,
// enqueues the stable LSD passes: key_lo, key_hi, then (where some request may not consent) the consent bit -- consenting requests first, each visitor's in request
// order -- and the gather of the times through that order.  Then: order, when (null untimed) and tmp / tmp_bytes for the owner's scans.
// (Templates only so that a file which sorts by KeySort alone instantiates none of the front's kernels.)
struct SortedFront {
    Bump::Region<uint64_t> key[2], when_at; Bump::Region<uint32_t> idx[2]; Bump::Region<char> tmp_at;
    const uint32_t* order = nullptr; const uint64_t* when = nullptr; char* tmp = nullptr; size_t tmp_bytes = 0;
    template <class Req> int plan(Bump& b, const Req& r, hipStream_t st, size_t scan_bytes = 0) {
        const int rc = key_sort_tmp_bytes(r.n, st, &tmp_bytes); if (rc) return rc;
        tmp_bytes = std::max(tmp_bytes, scan_bytes);
        for (auto& k : key) k = b.of<uint64_t>(r.n);
        for (auto& i : idx) i = b.of<uint32_t>(r.n);
        tmp_at = b.of<char>(tmp_bytes);
        if (r.times) when_at = b.of<uint64_t>(r.n);
        return SRN_OK;
    }
    template <class Req> int run(char* base, const Req& r, hipStream_t st) {
        tmp = tmp_at.at(base);
        KeySort ks{{key[0].at(base), key[1].at(base)}, {idx[0].at(base), idx[1].at(base)}, tmp, tmp_bytes, r.n, st};
        int rc;
        if ((rc = ks.begin(r.key_lo)) || (rc = ks.pass(KeyWord{r.key_hi})) || (r.consent && (rc = ks.pass(KeyNoConsent{r.consent}, 0, 1)))) return rc;
        order = ks.order();
        if (r.times) {
            key_gather<<<ks.grid(), kKeyTPB, 0, st>>>(KeyWord{r.times}, order, (uint32_t)r.n, when_at.at(base));
            when = when_at.at(base);
        }
        return SRN_OK;
    }
};
// f(std::true_type) for a timed batch, f(std::false_type) for an untimed one: a launch that differs in <kTimed> alone is written once, `decltype(timed)::value` its argument
template <class F> inline auto by_timed(const VisitorBatch& r, F&& f) { if (r.times) return f(std::true_type{}); return f(std::false_type{}); }

// ---- the host stage: a host-pointer call's request arrays on the device ----
// plan() declares the five arrays' copies on the caller's Bump (consent always, times for a timed batch); upload(base, r, st) enqueues the copies of those that are
// given and returns the descriptor of the device side.  The owner stages its own arrays beside them
struct StagedBatch {
    Bump::Region<uint64_t> hi, lo, item, times; Bump::Region<uint8_t> consent;
    void plan(Bump& b, const VisitorBatch& r) {
        hi = b.of<uint64_t>(r.n); lo = b.of<uint64_t>(r.n); item = b.of<uint64_t>(r.n); consent = b.of<uint8_t>(r.n);
        if (r.times) times = b.of<uint64_t>(r.n);
    }
    int upload(char* base, const VisitorBatch& r, hipStream_t st, VisitorBatch* dev) const {
        *dev = VisitorBatch{hi.at(base), lo.at(base), item.at(base), r.consent ? consent.at(base) : nullptr, times.at(base), r.n, r.now_secs};
        const struct { void* to; const void* from; size_t bytes; } copies[] = {
            {hi.at(base), r.key_hi, r.n * 8}, {lo.at(base), r.key_lo, r.n * 8}, {item.at(base), r.item, r.n * 8}, {consent.at(base), r.consent, r.n}, {times.at(base), r.times, r.n * 8}};
        for (const auto& c : copies) if (c.from) HIP_TRY(hipMemcpyAsync(c.to, c.from, c.bytes, hipMemcpyHostToDevice, st));
        return SRN_OK;
    }
};

}  // namespace srn
