// The table keyed by visitor underneath the device session store (srn_sessions_dev.hip) and the click feedback log (srn_feedback.hip), read beside them by
// srn_trending.hip and srn_harvest.hip: the slot's head, the probe, count and rebuild kernels, the host-side core of an owner's handle and the capacity rule, once
// (DESIGN.md 11).  An owner brings its slot, a payload functor, its batch kernels and where its second table comes from: the store keeps a pair and flips, the log
// allocates one inside a sweep.  Also the host code's scratch idiom: regions of one buffer are declared on a Bump (srn_runtime.h) -- element type and count, once,
// where they are named; the total falls out -- and grow_behind is the one rule by which such a buffer grows while the owner's last call may still read it.
// The batch-side pieces (run predicates, find_or_claim, the key sort, the sorted front and the host stage of a visitor batch) are srn_visitors.h's.
// No relocatable device code: every kernel here is a template or static, every function inline.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_device.h"

namespace srn {

// ---- the slot: { key_hi u64 | key_lo u64 | epoch u64 | the owner's u32 | state u32 | the owner's payload }, `stride` bytes apart ----
constexpr uint32_t kSlotHead = 32;             // bytes before the store's items
constexpr uint32_t kEmpty = 0, kFull = 1, kClaimed = 2;
struct SlotHead { uint64_t key_hi, key_lo, epoch; uint32_t len, state; };   // (len: the store's name for the owner's word)
static_assert(sizeof(SlotHead) == kSlotHead, "slot header");
// An owner's slot is probed, counted and rebuilt as SlotHead: it must begin with the same key, epoch and state
template <class S> constexpr bool begins_as_slot_head() {
    return sizeof(S) >= sizeof(SlotHead) && offsetof(S, key_hi) == offsetof(SlotHead, key_hi) && offsetof(S, key_lo) == offsetof(SlotHead, key_lo) &&
           offsetof(S, epoch) == offsetof(SlotHead, epoch) && offsetof(S, state) == offsetof(SlotHead, state);
}

struct Table { char* base; uint32_t mask, stride; };
__device__ __forceinline__ SlotHead* slot_at(const Table& t, uint32_t s) { return (SlotHead*)(t.base + (size_t)s * t.stride); }
__host__ __device__ __forceinline__ bool idle_or_old(uint64_t now, uint64_t epoch, uint64_t limit) { return now > epoch && now - epoch > limit; }
__device__ __forceinline__ uint32_t key_hash(uint64_t hi, uint64_t lo) { return (uint32_t)dev_mix64(lo ^ dev_mix64(hi)); }
inline uint64_t wall_secs() { return (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::system_clock::now().time_since_epoch()).count(); }

// ---- small helpers of the host code around these tables ----
constexpr uint32_t kTableTPB = 256;
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }
inline dim3 grid_for(size_t n) { return dim3((unsigned)((std::max<size_t>(n, 1) + kTableTPB - 1) / kTableTPB)); }   // one lane per entry, blocks of kTableTPB
struct StageBuf {   // a blocking call's own device memory (not DevBuf: that is the loader's, srn_events.h)
    char* p = nullptr;
    ~StageBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes, const char* who, const char* what = "the staging copies") {
        if (hipMalloc((void**)&p, bytes ? bytes : 256) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return fail(SRN_ENOMEM, std::string(who) + ": no device memory for " + what); }
        return SRN_OK;
    }
};
// The grow rule of a scratch buffer that the owner's calls share: the call recorded in `last` may still read it, so wait for that call before the buffer is freed and
// reallocated.  A buffer that is large enough costs nothing
inline int grow_behind(hipEvent_t last, char** buf, size_t* bytes, size_t need) {
    if (need > *bytes) HIP_TRY(hipEventSynchronize(last));
    return ensure(buf, bytes, need);
}

// ---- kernels ----
// the slot that holds the key, or kNone (one lane, from the host: no claim is running)
__device__ __forceinline__ uint32_t probe_key(const Table& t, uint64_t hi, uint64_t lo) {
    uint32_t h = key_hash(hi, lo) & t.mask;
    for (uint32_t probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        const SlotHead* s = slot_at(t, h);
        if (s->state == kEmpty) return kNone;
        if (s->key_hi == hi && s->key_lo == lo) return h;
    }
    return kNone;
}
// counters[0] = occupied slots, [1] = entries a sweep at `now` keeps
__global__ static void __launch_bounds__(kTableTPB) table_count(Table t, uint64_t now, uint64_t ttl, unsigned long long* counters) {
    const uint32_t i = blockIdx.x * kTableTPB + threadIdx.x;
    bool occ = false, live = false;
    if (i <= t.mask) { const SlotHead* s = slot_at(t, i); occ = s->state != kEmpty; live = occ && !idle_or_old(now, s->epoch, ttl); }
    const unsigned long long mo = __ballot(occ), ml = __ballot(live);
    if ((threadIdx.x & 63) == 0) { if (mo) atomicAdd(&counters[0], (unsigned long long)__popcll(mo)); if (ml) atomicAdd(&counters[1], (unsigned long long)__popcll(ml)); }
}
// Slot, the owner's payload functor: Head, its slot struct; copy(const Head* s, Head* d), the owner's word and payload of an entry a rebuild keeps; read(const Head* s,
// uint64_t* out), one entry for the host -- out[0] = its count, out[2..] as the owner likes (out[1] is the epoch).
// The entries a sweep keeps, into the cleared table `to` (every key once: a taken slot is another key's)
template <class Slot>
__global__ void __launch_bounds__(kTableTPB) table_rebuild(Table from, Table to, uint64_t now, uint64_t ttl, Slot slot) {
    static_assert(begins_as_slot_head<typename Slot::Head>(), "table_rebuild, table_count, probe_key and find_or_claim read a slot as SlotHead");
    const uint32_t i = blockIdx.x * kTableTPB + threadIdx.x;
    if (i > from.mask) return;
    const SlotHead* s = slot_at(from, i);
    if (s->state == kEmpty || idle_or_old(now, s->epoch, ttl)) return;
    uint32_t h = key_hash(s->key_hi, s->key_lo) & to.mask;
    for (uint32_t probes = 0; probes <= to.mask; ++probes, h = (h + 1) & to.mask) {
        SlotHead* d = slot_at(to, h);
        if (atomicCAS(&d->state, kEmpty, kFull) != kEmpty) continue;
        d->key_hi = s->key_hi; d->key_lo = s->key_lo; d->epoch = s->epoch;
        slot.copy((const typename Slot::Head*)s, (typename Slot::Head*)d);
        return;
    }
}
// one key, from the host: out[0] = ~0 for an unknown key, else slot.read's words around out[1] = the epoch
template <class Slot>
__global__ void table_get_one(Table t, uint64_t hi, uint64_t lo, Slot slot, uint64_t* out) {
    static_assert(begins_as_slot_head<typename Slot::Head>(), "probe_key reads a slot as SlotHead");
    out[0] = ~0ull;
    const uint32_t h = probe_key(t, hi, lo);
    if (h == kNone) return;
    const SlotHead* s = slot_at(t, h);
    out[1] = s->epoch;
    slot.read((const typename Slot::Head*)s, out);
}

// ---- the host side: what the handle of every owner begins with ----
struct VisitorTable {
    const char* who = "";                                   // the owner's name in a message: "device session store", "click feedback log"
    int device = 0;
    uint64_t capacity = 0, n_slots = 0, ttl = 0, idle = 0;
    uint32_t stride = 0;
    char* table = nullptr;                                  // the table the calls read and write; how a second one comes and goes is the owner's
    std::mutex mu;                                          // covers the enqueue of a call and everything below
    hipEvent_t last = nullptr;                              // end of the most recent call, whatever stream it ran on
    hipStream_t own = nullptr;                              // get / sweep / count and the host-pointer entry points
    uint64_t bound = 0, sweeps = 0, refused = 0;            // bound: upper bound of the occupied slots
    char* small = nullptr;                                  // err word | counters | one entry in / out
    char* ws = nullptr; size_t ws_bytes = 0;                // per-batch scratch, grows with the largest n seen (grow_behind)
    Table tab() const { return Table{table, (uint32_t)(n_slots - 1), stride}; }
    uint32_t* err() const { return (uint32_t*)small; }
    unsigned long long* counters() const { return (unsigned long long*)(small + 64); }
    uint64_t* one() const { return (uint64_t*)(small + 128); }
};

inline uint64_t slots_for(uint64_t capacity) { uint64_t n = 2; while (n < 2 * capacity) n <<= 1; return n; }   // load <= 0.5
inline uint32_t stride_for(uint32_t head_bytes, uint64_t words) { return (uint32_t)((head_bytes + 8 * words + 127) / 128 * 128); }

// create, the shared half: the checks (`fn`: the entry point's name), the clocks with srn_session_store_create's defaults, the shape, the stream, the event and the
// cleared `small` block with room for one entry of one_words.  The owner then allocates its tables, clears the first on `own` and synchronises
inline int table_create(VisitorTable* c, const char* fn, const char* who, int device, size_t capacity, uint64_t ttl_secs, uint64_t idle_secs, uint32_t head_bytes,
                        uint64_t words, size_t one_words) {
    if (capacity == 0) return fail(SRN_EINVAL, std::string(fn) + ": capacity must be > 0");
    if (capacity > (1ull << 30)) return fail(SRN_ERANGE, std::string(fn) + ": capacity above 2^30 entries");
    c->who = who; c->capacity = capacity; c->ttl = ttl_secs ? ttl_secs : 30 * 60; c->idle = idle_secs ? idle_secs : 20 * 60;
    if (c->ttl < c->idle) return fail(SRN_EINVAL, std::string(fn) + ": ttl_secs below idle_secs (a swept entry could still have been read)");
    int n_dev = 0;
    if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return fail(SRN_ENODEV, std::string(fn) + ": no such GPU");
    HIP_TRY(hipSetDevice(device));
    c->device = device; c->n_slots = slots_for(capacity); c->stride = stride_for(head_bytes, words);
    HIP_TRY(hipMalloc((void**)&c->small, 128 + 8 * one_words));
    HIP_TRY(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->last, hipEventDisableTiming));
    HIP_TRY(hipMemsetAsync(c->small, 0, 128, c->own));
    return SRN_OK;
}
// free, the shared half: behind the last call and the own stream's work, then the table and `small`
inline void table_release(VisitorTable* c) {
    if (!c->small) return;   // (a create that failed in its checks: nothing was allocated and the caller's current device stays)
    (void)hipSetDevice(c->device);
    if (c->last) { (void)hipEventSynchronize(c->last); (void)hipEventDestroy(c->last); }
    if (c->own) { (void)hipStreamSynchronize(c->own); (void)hipStreamDestroy(c->own); }
    if (c->table) (void)hipFree(c->table);
    if (c->small) (void)hipFree(c->small);
    if (c->ws) (void)hipFree(c->ws);
}

// behind everything enqueued on the owner so far, on its own stream (mu held)
inline int own_after_last(VisitorTable* c) { HIP_TRY(hipSetDevice(c->device)); HIP_TRY(hipStreamWaitEvent(c->own, c->last, 0)); return SRN_OK; }

inline int count(VisitorTable* c, uint64_t now, uint64_t* occupied, uint64_t* live) {   // blocks (own stream, mu held)
    HIP_TRY(hipMemsetAsync(c->counters(), 0, 16, c->own));
    table_count<<<grid_for(c->n_slots), kTableTPB, 0, c->own>>>(c->tab(), now, c->ttl, c->counters());
    HIP_TRY(hipGetLastError());
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, c->counters(), 16, hipMemcpyDeviceToHost, c->own));
    HIP_TRY(hipStreamSynchronize(c->own));
    *occupied = v[0]; *live = v[1];
    return SRN_OK;
}
// clears `to` and enqueues the rebuild of the current table into it (own stream, mu held)
template <class Slot> inline hipError_t rebuild_into(VisitorTable* c, const Table& to, uint64_t now, Slot slot) {
    const hipError_t e = hipMemsetAsync(to.base, 0, ((size_t)to.mask + 1) * to.stride, c->own);
    if (e != hipSuccess) return e;
    table_rebuild<<<grid_for(c->n_slots), kTableTPB, 0, c->own>>>(c->tab(), to, now, c->ttl, slot);
    return hipGetLastError();
}
// a batch that found the table full left a word behind: the capacity rule was violated (blocks)
inline int check_err(VisitorTable* c) {
    uint32_t err = 0;
    HIP_TRY(hipMemcpy(&err, c->err(), 4, hipMemcpyDeviceToHost));
    if (err) return fail(SRN_ESTATE, std::string(c->who) + ": a batch found the table full (the capacity rule was violated)");
    return SRN_OK;
}

// The capacity rule (mu held): room for n more keys, or SRN_ENOMEM with the table as it was.  Only when the host's bound does not fit does anything wait for the device:
// the exact counts replace the bound, and entries older than the TTL are dropped (a rebuild) if that makes the room; if not even that would, the owner may grow.
//   rebuild(now)       the owner's sweep into its second table, enqueued on `own`; the rule waits for it before the bound drops to the live count
//   grow(need, now)    the owner's growth to a capacity of at least `need`: SRN_OK (it grew), SRN_ENOMEM (it cannot or may not: the call is refused), anything else is returned
template <class Rebuild, class Grow>
inline int make_room(VisitorTable* c, uint64_t n, uint64_t now, Rebuild rebuild, Grow grow) {
    if (c->bound + n <= c->capacity) return SRN_OK;
    int rc = own_after_last(c); if (rc) return rc;
    uint64_t occupied = 0, live = 0;
    if ((rc = count(c, now, &occupied, &live))) return rc;
    c->bound = occupied;
    if (occupied + n <= c->capacity) return SRN_OK;
    if (live + n > c->capacity) {
        if ((rc = grow(live + n, now)) != SRN_ENOMEM) return rc;
        ++c->refused;
        return fail(SRN_ENOMEM, std::string(c->who) + ": the batch does not fit the capacity (live entries + batch > capacity)");
    }
    if ((rc = rebuild(now))) return rc;
    HIP_TRY(hipStreamSynchronize(c->own));
    c->bound = live;
    return SRN_OK;
}
inline int never_grows(uint64_t, uint64_t) { return SRN_ENOMEM; }

// an explicit sweep (mu held): the rebuild, then the exact count of what it left
template <class Rebuild>
inline int sweep(VisitorTable* c, uint64_t now, Rebuild rebuild, uint64_t* n_live) {
    int rc = own_after_last(c); if (rc) return rc;
    if ((rc = rebuild(now))) return rc;
    uint64_t occupied = 0, live = 0;
    if ((rc = count(c, now, &occupied, &live))) return rc;
    c->bound = occupied;
    if (n_live) *n_live = occupied;
    return check_err(c);
}

// One key's entry for the host (mu held; blocks): h = n_words words of slot.read.  *found: the key is stored and not idle at `now`
template <class Slot>
inline int read_one(VisitorTable* c, uint64_t hi, uint64_t lo, uint64_t now, Slot slot, size_t n_words, std::vector<uint64_t>* h, bool* found) {
    int rc = own_after_last(c); if (rc) return rc;
    table_get_one<<<1, 1, 0, c->own>>>(c->tab(), hi, lo, slot, c->one());
    HIP_TRY(hipGetLastError());
    h->assign(n_words, 0);
    HIP_TRY(hipMemcpyAsync(h->data(), c->one(), n_words * 8, hipMemcpyDeviceToHost, c->own));
    HIP_TRY(hipStreamSynchronize(c->own));
    *found = (*h)[0] != ~0ull && !idle_or_old(now, (*h)[1], c->idle);
    return SRN_OK;
}

}  // namespace srn
