// Session harvest (include/serenade_hip.h, "session harvest"): a device-resident log that receives every session at the moment the device session store
// forgets it, and turns the log into training events in the form srn_sessions_from_events reads.
//
// The log: dense arrays in the store's export form, allocated at creation, and a few u64 device words
//   key_hi[capacity] | key_lo[capacity] | epoch[capacity] | len u32[capacity] | items[capacity * items_cap]      words: cursor | lost | skipped_short | from_return | from_rebuild | cleared
//
// An append, on the stream of the call that forgets the sessions, nothing read back (harvest_append; the hooks are in srn_sessions_dev.hip):
//   flag            one u64 per position -- a sorted request position for a return after idle, a slot for a rebuild: kHvStore for a forgotten session of >= min_len items,
//                   kHvSkip for a shorter one, 0 otherwise; the two counts ride in the two halves of one word
//   scan            rocPRIM exclusive scan: a stored session's place behind the cursor in the low half, and the call's two totals in the last word
//   hv_scatter      reads the cursor as its base and copies the slots, adjacent lanes reading the 16-byte elements of one slot (sess_export_scatter's form); places at or
//                   beyond the capacity are not written
//   hv_advance      one lane: cursor and counters, plain stores, ordered by the stream
// No atomic cursor: the append order is the position order, so which sessions a full log loses does not depend on how the lanes were scheduled.
// A timed batch appends a second time in the same shape, from the call's CSR instead of slots: the sessions that ended inside the call
// (harvest_append_csr, hv_scatter_csr).
//
// Reading: the stored sessions are presented sorted by (epoch, key_hi, key_lo) -- stable LSD rocPRIM radix passes over key_lo, key_hi, epoch and a last one-bit pass
// that puts the places beyond the cursor behind the stored ones (the sort's size is the host's upper bound of the cursor, exact after a read-back; the cursor itself
// is only known to the device) -- so the same set of sessions gives the same bytes however the requests were cut into calls and wherever the sweeps fell.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include <rocprim/rocprim.hpp>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_sessions_dev.h"   // the store's and the harvest's handles over srn_visitor_table.h: Table, SlotHead, align256, grid_for
#include "srn_visitors.h"       // the key sort
#include "srn_hipsync.h"

namespace srn {

namespace {
constexpr uint32_t kTPB = kTableTPB;   // (grid_for)

// flag[i] for slot i of a table a rebuild at `now` reads: what the rebuild leaves out (occupied and older than the TTL); flag[n_slots] = 0
__global__ void __launch_bounds__(kTPB) hv_dropped_flag(Table t, uint64_t now, uint64_t ttl, uint32_t min_len, uint64_t* __restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    if (i > (uint64_t)t.mask + 1u) return;
    uint64_t f = 0;
    if (i <= t.mask) {
        const SlotHead* s = slot_at(t, (uint32_t)i);
        if (s->state != kEmpty && idle_or_old(now, s->epoch, ttl)) f = s->len >= min_len ? kHvStore : kHvSkip;
    }
    flag[i] = f;
}

struct AppendArgs {
    Table t; const uint32_t* slot_of;   // position -> slot (null: the position is the slot)
    const uint64_t* flag; const uint64_t* pos; uint64_t n;
    const uint64_t* words; uint64_t capacity, items_cap;
    uint64_t* key_hi; uint64_t* key_lo; uint64_t* epoch; uint32_t* len; uint64_t* items;
    uint32_t lanes_shift;               // 2^lanes_shift adjacent lanes read one slot, 16 bytes each per round
};
// Slot -> log entry cursor + place.  A slot is 16-byte elements: 0 = the key, 1 = epoch | len | state, 2.. = item pairs; items from `len` on are written as zero.
__global__ void __launch_bounds__(kTPB) hv_scatter(AppendArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    const uint64_t i = tid >> a.lanes_shift;
    const uint32_t lanes = 1u << a.lanes_shift, lane = (uint32_t)tid & (lanes - 1);
    if (i >= a.n || a.flag[i] != kHvStore) return;
    const uint64_t d = a.words[kHvCursor] + (uint32_t)a.pos[i];
    if (d >= a.capacity) return;   // the log is full: counted by hv_advance
    const uint32_t slot = a.slot_of ? a.slot_of[i] : (uint32_t)i;
    if (slot > a.t.mask) return;
    const SlotHead* s = slot_at(a.t, slot);
    const uint32_t len = (uint32_t)min((uint64_t)s->len, a.items_cap);   // (a stored session is never longer than the store's items_cap <= the log's)
    const ulonglong2* el = (const ulonglong2*)s;
    const uint64_t n_el = 2 + (a.items_cap + 1) / 2;
    for (uint64_t e = lane; e < n_el; e += lanes) {
        if (e == 0) { const ulonglong2 v = el[0]; a.key_hi[d] = v.x; a.key_lo[d] = v.y; }
        else if (e == 1) { a.epoch[d] = s->epoch; a.len[d] = len; }
        else {
            const uint64_t j = 2 * (e - 2);
            ulonglong2 v = make_ulonglong2(0, 0);
            if (j < len) { v = el[e]; if (j + 1 >= len) v.y = 0; }   // (j < len <= the store's items_cap: the pair lies inside the slot, whose size is a multiple of 128)
            uint64_t* dst = a.items + d * a.items_cap + j;
            dst[0] = v.x; if (j + 1 < a.items_cap) dst[1] = v.y;
        }
    }
}
// A timed batch ends sessions inside the call: flagged sorted position p ends the session of position p - 1, which no slot ever held.  Its source is
// the call's CSR: the key of request order[p] (the run's), the predecessor's time t[p - 1] and the predecessor's window items_flat[q_off[pr] .. q_off[pr + 1]).
struct CsrAppendArgs {
    const uint32_t* order; const uint64_t* src_hi; const uint64_t* src_lo; const uint64_t* t; const uint64_t* items_flat; const uint32_t* q_off;
    const uint64_t* flag; const uint64_t* pos; uint64_t n;
    const uint64_t* words; uint64_t capacity, items_cap;
    uint64_t* key_hi; uint64_t* key_lo; uint64_t* epoch; uint32_t* len; uint64_t* items;
};
// 8 adjacent lanes write one entry: lane l the items l, l + 8, ... (zero from `len` on), the first lane the head words
__global__ void __launch_bounds__(kTPB) hv_scatter_csr(CsrAppendArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    const uint64_t p = tid >> 3;
    const uint32_t lane = (uint32_t)tid & 7u;
    if (p == 0 || p >= a.n || a.flag[p] != kHvStore) return;
    const uint64_t d = a.words[kHvCursor] + (uint32_t)a.pos[p];
    if (d >= a.capacity) return;   // the log is full: counted by hv_advance
    const uint32_t req = a.order[p], pr = a.order[p - 1];
    const uint32_t off = a.q_off[pr];
    const uint32_t len = (uint32_t)min((uint64_t)(a.q_off[pr + 1] - off), a.items_cap);   // (a window is never longer than the store's items_cap <= the log's)
    if (lane == 0) { a.key_hi[d] = a.src_hi[req]; a.key_lo[d] = a.src_lo[req]; a.epoch[d] = a.t[p - 1]; a.len[d] = len; }
    uint64_t* dst = a.items + d * a.items_cap;
    for (uint64_t j = lane; j < a.items_cap; j += 8) dst[j] = j < len ? a.items_flat[off + j] : 0;
}
// total = the scan's last word: stored candidates in the low half, short ones in the high half
__global__ void hv_advance(uint64_t* words, const uint64_t* total, uint64_t capacity, uint32_t which) {
    const uint64_t fit = (uint32_t)*total, small = *total >> 32, base = words[kHvCursor];
    const uint64_t stored = min(fit, capacity - base);
    words[kHvCursor] = base + stored;
    words[kHvLost] += fit - stored;
    words[kHvShort] += small;
    words[which] += fit + small;
}
__global__ void hv_clear(uint64_t* words) { words[kHvCleared] += words[kHvCursor]; words[kHvCursor] = 0; }
__global__ void __launch_bounds__(kTPB) hv_sum_len(const uint32_t* __restrict__ len, const uint64_t* __restrict__ words, uint64_t capacity, unsigned long long* out) {
    const uint64_t i = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    unsigned long long v = i < min(words[kHvCursor], capacity) ? len[i] : 0;
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

// ---- the canonical order ----
// the key sort's last, one-bit word: is place e at or beyond the cursor
struct KeyBeyond { const uint64_t* words; __device__ __forceinline__ uint64_t operator()(uint32_t e) const { return e >= words[kHvCursor] ? 1ull : 0ull; } };

struct ReadArgs {
    const uint64_t* key_hi; const uint64_t* key_lo; const uint64_t* epoch; const uint32_t* len; const uint64_t* items; const uint64_t* words;
    const uint32_t* order;   // [n] log entry of each canonical position
    uint64_t n, items_cap;
};
__device__ __forceinline__ uint64_t hv_held(const ReadArgs& a) { return min(a.words[kHvCursor], a.n); }

__global__ void __launch_bounds__(kTPB) hv_export_heads(ReadArgs a, uint64_t cap, uint64_t* key_hi, uint64_t* key_lo, uint64_t* epoch, uint32_t* len, uint64_t* d_n) {
    const uint64_t r = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    if (r == 0) *d_n = a.words[kHvCursor];
    if (r >= min(hv_held(a), cap)) return;
    const uint32_t src = a.order[r];
    key_hi[r] = a.key_hi[src]; key_lo[r] = a.key_lo[src]; epoch[r] = a.epoch[src]; len[r] = a.len[src];
}
__global__ void __launch_bounds__(kTPB) hv_export_items(ReadArgs a, uint64_t cap, uint64_t* items, uint64_t items_stride) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    const uint64_t r = tid / items_stride, j = tid % items_stride;
    if (r >= min(hv_held(a), cap)) return;
    const uint32_t src = a.order[r];
    items[r * items_stride + j] = j < a.len[src] ? a.items[(uint64_t)src * a.items_cap + j] : 0;   // (len <= items_cap)
}
// lens[r] = the length of canonical session r (0 beyond the stored ones); lens[n] = 0, so that the exclusive scan's last word is the number of rows
__global__ void __launch_bounds__(kTPB) hv_event_lens(ReadArgs a, uint64_t* __restrict__ lens) {
    const uint64_t r = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    if (r > a.n) return;
    lens[r] = r < hv_held(a) ? a.len[a.order[r]] : 0;
}
__global__ void __launch_bounds__(kTPB) hv_events(ReadArgs a, const uint64_t* __restrict__ off, uint64_t id_base, uint64_t cap_rows,
                                                  uint64_t* session_ids, uint64_t* item_ids, int64_t* times, uint64_t* d_rows) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    if (tid == 0) *d_rows = off[a.n];
    const uint64_t r = tid / a.items_cap, j = tid % a.items_cap;
    if (r >= hv_held(a)) return;
    const uint32_t src = a.order[r];
    if (j >= a.len[src]) return;
    const uint64_t row = off[r] + j;
    if (row >= cap_rows) return;
    session_ids[row] = id_base + r; item_ids[row] = a.items[(uint64_t)src * a.items_cap + j]; times[row] = (int64_t)a.epoch[src];
}

// the harvest's mutex, then its store's: every harvest call runs behind the store's previous call, on the store's own stream where it blocks.  Detached: its own pair
struct Enter {
    std::unique_lock<std::mutex> hl, sl;
    hipStream_t own = nullptr; hipEvent_t last = nullptr;
    explicit Enter(srn_harvest* h) : hl(h->mu) {
        if (h->store) { sl = std::unique_lock<std::mutex>(h->store->mu); own = h->store->own; last = h->store->last; }
        else { own = h->own; last = h->last; }
    }
};

struct SortScratch { const uint32_t* order; uint64_t* lens; uint64_t* off; char* tmp; size_t tmp_bytes; };
// the canonical order of the log's first n places on `st` (which already waits for `last`): sc->order
int canonical_order(srn_harvest* h, size_t n, hipEvent_t last, hipStream_t st, SortScratch* sc) {
    size_t tmp = 0, t1 = 0;
    int rc = key_sort_tmp_bytes(n, st, &tmp); if (rc) return rc;
    HIP_TRY(rocprim::exclusive_scan(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr, 0ull, n + 1, rocprim::plus<uint64_t>(), st)); tmp = std::max(tmp, t1);
    Bump b;   // (the key buffers n + 1 wide, as the events' lengths and offsets: a sort by four words over the log's own arrays, so KeySort directly, not the batch's front)
    const auto keyA = b.of<uint64_t>(n + 1), keyB = b.of<uint64_t>(n + 1), lens = b.of<uint64_t>(n + 1), off = b.of<uint64_t>(n + 1);
    const auto idxA = b.of<uint32_t>(n), idxB = b.of<uint32_t>(n); const auto tmp_at = b.of<char>(tmp);
    if ((rc = grow_behind(last, &h->xs, &h->xs_bytes, b.bytes))) return rc;
    char* const xs = h->xs;
    sc->lens = lens.at(xs); sc->off = off.at(xs); sc->tmp = tmp_at.at(xs); sc->tmp_bytes = tmp;
    KeySort ks{{keyA.at(xs), keyB.at(xs)}, {idxA.at(xs), idxB.at(xs)}, sc->tmp, tmp, n, st};
    if ((rc = ks.begin(h->key_lo)) || (rc = ks.pass(KeyWord{h->key_hi})) || (rc = ks.pass(KeyWord{h->epoch})) || (rc = ks.pass(KeyBeyond{h->words}, 0, 1))) return rc;
    HIP_TRY(hipGetLastError());
    sc->order = ks.order();
    return SRN_OK;
}
ReadArgs read_args(const srn_harvest* h, const uint32_t* order, size_t n) {
    return ReadArgs{h->key_hi, h->key_lo, h->epoch, h->len, h->items, h->words, order, n, h->items_cap};
}
// sort + gather on `st`, which already waits for `last`: the first min(stored, cap) sessions of the first n places, *d_n = stored
int export_enqueue(srn_harvest* h, size_t n, size_t cap, uint64_t* d_hi, uint64_t* d_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items, size_t items_stride,
                   uint64_t* d_n, hipEvent_t last, hipStream_t st) {
    SortScratch sc{};
    int rc = canonical_order(h, n, last, st, &sc); if (rc) return rc;
    const ReadArgs a = read_args(h, sc.order, n);
    hv_export_heads<<<grid_for(n), kTPB, 0, st>>>(a, cap, d_hi, d_lo, d_epoch, d_len, d_n);
    if (items_stride && cap) hv_export_items<<<grid_for(std::min(n, cap) * items_stride), kTPB, 0, st>>>(a, cap, d_items, items_stride);
    HIP_TRY(hipGetLastError());
    return SRN_OK;
}
// the device words on the host, with the stored sessions' items summed into words[kHvItems]; blocks (own stream, behind `last`)
int read_words(srn_harvest* h, hipEvent_t last, hipStream_t own, uint64_t* out) {
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamWaitEvent(own, last, 0));
    HIP_TRY(hipMemsetAsync(h->words + kHvItems, 0, 8, own));
    hv_sum_len<<<grid_for(h->capacity), kTPB, 0, own>>>(h->len, h->words, h->capacity, (unsigned long long*)(h->words + kHvItems));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, h->words, kHvWords * 8, hipMemcpyDeviceToHost, own));
    HIP_TRY(hipStreamSynchronize(own));
    h->bound = std::min<uint64_t>(h->capacity, out[kHvCursor]);   // (exact: both mutexes are held, nothing is appended meanwhile)
    return SRN_OK;
}
// the places a device-stream read sorts: the host's bound of the cursor, which a stats / export read-back makes exact -- not the capacity, however few sessions are stored
size_t sort_places(const srn_harvest* h) { return (size_t)std::max<uint64_t>(h->bound, 1); }
}  // namespace

// ---- the append, for the store's hooks (the store's mutex held; `st` is the stream of the call that forgets the sessions) ----
int harvest_scratch_bytes(size_t n, size_t* bytes) {
    size_t tmp = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, (uint64_t*)nullptr, (uint64_t*)nullptr, 0ull, n + 1, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
    *bytes = 2 * align256((n + 1) * 8) + align256(tmp);
    return SRN_OK;
}
int harvest_append(srn_harvest* h, const Table& t, const uint32_t* slot_of, size_t n, char* scratch, bool from_return, hipStream_t st) {
    const size_t w = align256((n + 1) * 8);
    uint64_t* flag = (uint64_t*)scratch; uint64_t* pos = (uint64_t*)(scratch + w);
    size_t tmp = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, flag, pos, 0ull, n + 1, rocprim::plus<uint64_t>(), st));
    HIP_TRY(rocprim::exclusive_scan(scratch + 2 * w, tmp, flag, pos, 0ull, n + 1, rocprim::plus<uint64_t>(), st));
    AppendArgs a{};
    a.t = t; a.slot_of = slot_of; a.flag = flag; a.pos = pos; a.n = n; a.words = h->words; a.capacity = h->capacity; a.items_cap = h->items_cap;
    a.key_hi = h->key_hi; a.key_lo = h->key_lo; a.epoch = h->epoch; a.len = h->len; a.items = h->items;
    a.lanes_shift = t.stride == 128 ? 3 : 4;
    hv_scatter<<<grid_for(n << a.lanes_shift), kTPB, 0, st>>>(a);
    hv_advance<<<1, 1, 0, st>>>(h->words, pos + n, h->capacity, from_return ? kHvReturn : kHvRebuild);
    HIP_TRY(hipGetLastError());
    h->bound = std::min<uint64_t>(h->capacity, h->bound + n);
    return SRN_OK;
}
int harvest_append_csr(srn_harvest* h, const uint32_t* order, const uint64_t* src_hi, const uint64_t* src_lo, const uint64_t* t, const uint64_t* items_flat,
                       const uint32_t* q_off, size_t n, char* scratch, hipStream_t st) {
    const size_t w = align256((n + 1) * 8);
    uint64_t* flag = (uint64_t*)scratch; uint64_t* pos = (uint64_t*)(scratch + w);
    size_t tmp = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, flag, pos, 0ull, n + 1, rocprim::plus<uint64_t>(), st));
    HIP_TRY(rocprim::exclusive_scan(scratch + 2 * w, tmp, flag, pos, 0ull, n + 1, rocprim::plus<uint64_t>(), st));
    CsrAppendArgs a{};
    a.order = order; a.src_hi = src_hi; a.src_lo = src_lo; a.t = t; a.items_flat = items_flat; a.q_off = q_off;
    a.flag = flag; a.pos = pos; a.n = n; a.words = h->words; a.capacity = h->capacity; a.items_cap = h->items_cap;
    a.key_hi = h->key_hi; a.key_lo = h->key_lo; a.epoch = h->epoch; a.len = h->len; a.items = h->items;
    hv_scatter_csr<<<grid_for(n << 3), kTPB, 0, st>>>(a);
    hv_advance<<<1, 1, 0, st>>>(h->words, pos + n, h->capacity, kHvReturn);
    HIP_TRY(hipGetLastError());
    h->bound = std::min<uint64_t>(h->capacity, h->bound + n);
    return SRN_OK;
}
int harvest_dropped(srn_harvest* h, const Table& from, uint64_t now, uint64_t ttl, char* scratch, hipStream_t st) {
    const size_t n = (size_t)from.mask + 1;
    hv_dropped_flag<<<grid_for(n + 1), kTPB, 0, st>>>(from, now, ttl, h->min_len, (uint64_t*)scratch);
    HIP_TRY(hipGetLastError());
    return harvest_append(h, from, nullptr, n, scratch, false, st);
}

// ---- the object ----
static void harvest_release(srn_harvest* h) {
    (void)hipSetDevice(h->device);
    if (h->last) { (void)hipEventSynchronize(h->last); (void)hipEventDestroy(h->last); }
    if (h->own) { (void)hipStreamSynchronize(h->own); (void)hipStreamDestroy(h->own); }
    for (void* p : {(void*)h->key_hi, (void*)h->key_lo, (void*)h->epoch, (void*)h->len, (void*)h->items, (void*)h->words, (void*)h->xs}) if (p) (void)hipFree(p);
    delete h;
}

int harvest_create(int device, size_t capacity, size_t items_cap, uint32_t min_len, srn_harvest** out) {
    if (!out) return fail(SRN_EINVAL, "srn_harvest_create: null output");
    *out = nullptr;
    if (capacity == 0) return fail(SRN_EINVAL, "srn_harvest_create: capacity must be > 0");
    if (capacity > (1ull << 30)) return fail(SRN_ERANGE, "srn_harvest_create: capacity above 2^30 sessions");
    if (items_cap == 0) return fail(SRN_EINVAL, "srn_harvest_create: items_cap must be > 0");
    if (items_cap > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "srn_harvest_create: items_cap above SRN_MAX_SESSION_LEN");
    int n_dev = 0;
    if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return fail(SRN_ENODEV, "srn_harvest_create: no such GPU");
    HIP_TRY(hipSetDevice(device));
    srn_harvest* h = new srn_harvest();
    struct Guard { srn_harvest*& h; ~Guard() { if (h) harvest_release(h); } } guard{h};
    h->device = device; h->capacity = capacity; h->items_cap = items_cap; h->min_len = min_len ? min_len : 1;
    const size_t sizes[5] = {capacity * 8, capacity * 8, capacity * 8, capacity * 4, capacity * items_cap * 8};
    void** arrays[5] = {(void**)&h->key_hi, (void**)&h->key_lo, (void**)&h->epoch, (void**)&h->len, (void**)&h->items};
    for (int i = 0; i < 5; ++i)
        if (hipMalloc(arrays[i], sizes[i]) != hipSuccess) { (void)hipGetLastError(); return fail(SRN_ENOMEM, "srn_harvest_create: no device memory for the log"); }
    HIP_TRY(hipMalloc((void**)&h->words, kHvWords * 8));
    HIP_TRY(hipStreamCreateWithFlags(&h->own, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->last, hipEventDisableTiming));
    for (int i = 0; i < 5; ++i) HIP_TRY(hipMemsetAsync(*arrays[i], 0, sizes[i], h->own));
    HIP_TRY(hipMemsetAsync(h->words, 0, kHvWords * 8, h->own));
    HIP_TRY(hipStreamSynchronize(h->own));
    *out = h; h = nullptr;
    return SRN_OK;
}

int harvest_free(srn_harvest* h) {
    if (!h) return SRN_OK;
    {
        std::lock_guard<std::mutex> g(h->mu);
        if (h->store) return fail(SRN_ESTATE, "srn_harvest_free: the harvest is attached to a store (srn_device_sessions_set_harvest(store, NULL) or free the store first)");
    }
    harvest_release(h);
    return SRN_OK;
}

int dsess_set_harvest(srn_device_sessions* s, srn_harvest* h) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_set_harvest: null store");
    if (!h) {   // detach: the harvest's next call must not overtake the store's last one
        srn_harvest* cur = nullptr;
        { std::lock_guard<std::mutex> g(s->mu); cur = s->harvest; }
        if (!cur) return SRN_OK;
        std::lock_guard<std::mutex> gh(cur->mu);
        std::lock_guard<std::mutex> gs(s->mu);
        if (s->harvest != cur) return SRN_OK;
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipEventSynchronize(s->last));
        s->harvest = nullptr; cur->store = nullptr;
        return SRN_OK;
    }
    std::lock_guard<std::mutex> gh(h->mu);
    std::lock_guard<std::mutex> gs(s->mu);
    if (h->store) return fail(SRN_ESTATE, "srn_device_sessions_set_harvest: the harvest is already attached to a store");
    if (s->harvest) return fail(SRN_ESTATE, "srn_device_sessions_set_harvest: the store already has a harvest");
    if (h->device != s->device) return fail(SRN_EINVAL, "srn_device_sessions_set_harvest: the harvest and the store are on different devices");
    if (h->items_cap < s->items_cap) return fail(SRN_ERANGE, "srn_device_sessions_set_harvest: the harvest's items_cap is below the store's");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipEventSynchronize(h->last));
    s->harvest = h; h->store = s;
    return SRN_OK;
}

int harvest_stats(srn_harvest* h, srn_harvest_stats_t* out) {
    if (!h || !out) return fail(SRN_EINVAL, "srn_harvest_stats: null argument");
    Enter e(h);
    uint64_t w[kHvWords] = {0};
    int rc = read_words(h, e.last, e.own, w); if (rc) return rc;
    *out = srn_harvest_stats_t{h->capacity, h->items_cap, h->min_len, w[kHvCursor], w[kHvItems], w[kHvLost], w[kHvShort], w[kHvReturn], w[kHvRebuild], w[kHvCleared]};
    return SRN_OK;
}

int harvest_clear(srn_harvest* h) {
    if (!h) return fail(SRN_EINVAL, "srn_harvest_clear: null harvest");
    Enter e(h);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamWaitEvent(e.own, e.last, 0));
    hv_clear<<<1, 1, 0, e.own>>>(h->words);
    HIP_TRY(hipGetLastError());
    h->bound = 0;
    HIP_TRY(hipEventRecord(e.last, e.own));
    return SRN_OK;
}

int harvest_export_device(srn_harvest* h, size_t cap, uint64_t* d_hi, uint64_t* d_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items, size_t items_stride,
                          uint64_t* d_n, void* stream) {
    if (!h || !d_n || (cap && (!d_hi || !d_lo || !d_epoch || !d_len || (items_stride && !d_items)))) return fail(SRN_EINVAL, "srn_harvest_export_device: null argument");
    if (items_stride < h->items_cap) return fail(SRN_ERANGE, "srn_harvest_export_device: items_stride below the longest session the harvest may hold (its items_cap)");
    hipStream_t st = (hipStream_t)stream;
    Enter e(h);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamWaitEvent(st, e.last, 0));
    const int rc = export_enqueue(h, sort_places(h), cap, d_hi, d_lo, d_epoch, d_len, d_items, items_stride, d_n, e.last, st);
    (void)hipEventRecord(e.last, st);
    return rc;
}

int harvest_export_host(srn_harvest* h, size_t cap, uint64_t* hi, uint64_t* lo, uint64_t* epoch, uint32_t* len, uint64_t* items, size_t items_stride, size_t* n) {
    const char* who = "srn_harvest_export";
    if (!h || !n || (cap && (!hi || !lo || !epoch || !len || (items_stride && !items)))) return fail(SRN_EINVAL, std::string(who) + ": null argument");
    Enter e(h);
    uint64_t w[kHvWords] = {0};
    int rc = read_words(h, e.last, e.own, w); if (rc) return rc;
    const size_t held = (size_t)w[kHvCursor];
    *n = held;
    if (items_stride < h->items_cap) return fail(SRN_ERANGE, std::string(who) + ": items_stride below the longest session the harvest may hold (its items_cap)");
    if (held > cap) return fail(SRN_ERANGE, std::string(who) + ": more stored sessions than the arrays hold (*n is their number)");
    if (held == 0) return SRN_OK;
    const Dense d(held, items_stride);
    StageBuf buf; if ((rc = buf.alloc(d.bytes, who))) return rc;
    char* const p = buf.p;
    rc = export_enqueue(h, held, held, d.hi.at(p), d.lo.at(p), d.ep.at(p), d.len.at(p), d.items.at(p), items_stride, d.word.at(p), e.last, e.own);
    hipError_t err = hipSuccess;
    if (rc == SRN_OK) {
        err = hipMemcpyAsync(hi, d.hi.at(p), held * 8, hipMemcpyDeviceToHost, e.own);
        if (err == hipSuccess) err = hipMemcpyAsync(lo, d.lo.at(p), held * 8, hipMemcpyDeviceToHost, e.own);
        if (err == hipSuccess) err = hipMemcpyAsync(epoch, d.ep.at(p), held * 8, hipMemcpyDeviceToHost, e.own);
        if (err == hipSuccess) err = hipMemcpyAsync(len, d.len.at(p), held * 4, hipMemcpyDeviceToHost, e.own);
        if (err == hipSuccess && items_stride) err = hipMemcpyAsync(items, d.items.at(p), held * items_stride * 8, hipMemcpyDeviceToHost, e.own);
    }
    const hipError_t err2 = hipStreamSynchronize(e.own);
    if (rc) return rc;
    if (err != hipSuccess || err2 != hipSuccess) return fail(SRN_EHIP, std::string(who) + ": " + hipGetErrorString(err != hipSuccess ? err : err2));
    return SRN_OK;
}

int harvest_events_device(srn_harvest* h, uint64_t id_base, size_t cap_rows, uint64_t* d_session_ids, uint64_t* d_item_ids, int64_t* d_times, uint64_t* d_rows, void* stream) {
    if (!h || !d_rows || (cap_rows && (!d_session_ids || !d_item_ids || !d_times))) return fail(SRN_EINVAL, "srn_harvest_events_device: null argument");
    hipStream_t st = (hipStream_t)stream;
    Enter e(h);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamWaitEvent(st, e.last, 0));
    auto run = [&]() -> int {
        const size_t n = sort_places(h);
        SortScratch sc{};
        int rc = canonical_order(h, n, e.last, st, &sc); if (rc) return rc;
        const ReadArgs a = read_args(h, sc.order, n);
        hv_event_lens<<<grid_for(n + 1), kTPB, 0, st>>>(a, sc.lens);
        size_t t1 = sc.tmp_bytes;
        HIP_TRY(rocprim::exclusive_scan(sc.tmp, t1, sc.lens, sc.off, 0ull, n + 1, rocprim::plus<uint64_t>(), st));
        hv_events<<<grid_for(n * h->items_cap), kTPB, 0, st>>>(a, sc.off, id_base, cap_rows, d_session_ids, d_item_ids, d_times, d_rows);
        HIP_TRY(hipGetLastError());
        return SRN_OK;
    };
    const int rc = run();
    (void)hipEventRecord(e.last, st);
    return rc;
}

}  // namespace srn
