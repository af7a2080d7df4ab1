// Device-resident evolving-session store and the batched /v1/recommend body (include/serenade_hip.h, "device-resident session store").
//
// srn_recommend (srn_session_store.cpp) is the handler body for ONE request against a host table.  Here the table lives in HBM and one call applies the
// handler's update rule (recommend_resource.rs:39-56, sessions/mod.rs:37-72) to a whole batch of (key, clicked item, consent) triples, exactly as if the
// requests had been served one after the other, and predicts every request's session through device_predict_device -- the launch sequence of srn_predict_batch_device.
//
// The table: power-of-two open addressing, linear probing, load <= 0.5, no tombstones (a sweep rebuilds into the second table).  One slot per visitor:
//   { key_hi u64 | key_lo u64 | epoch u64 | len u32 | state u32 | items u64[items_cap] }   rounded up to a multiple of 128 bytes, 128-byte aligned
// so that a request touches one aligned slot (items_cap <= 12: one 128-byte line).  state: 0 empty, 1 occupied, 2 claimed by the find kernel of the running call.
//
// A batch, all on the caller's stream, nothing read back:
//   sort            request indices, stable, by (no consent, key_hi, key_lo): the requests of one visitor become one contiguous RUN in request order
//   sess_find       one lane per run head: find-or-insert the slot.  Two heads never hold the same key, so a slot in state 2 is never "mine" and the loser
//                   of a claim probes on: nobody waits for anybody.  Reads the stored length under the idle rule
//   scans           the update rule needs no walk: request j of a run appends iff its item differs from its predecessor's (the stored last item for the
//                   head), so "kept" is a flag per request, its prefix count inside the run gives every request's session as a window of
//                   (stored items ++ kept clicks of the run), and the window's length is min(stored + kept so far, limit) (or the stored length where that
//                   already exceeds a since-lowered limit: one item is dropped per append)
//   sess_len        window lengths in ORIGINAL request order + the kept clicks compacted; exclusive scan -> q_off
//   sess_emit       every request copies its window into items_flat: O(window) per request, whatever the run's length
//   sess_store      the last request of a run writes its window -- the final session -- and the epoch back, once
//   device_predict_device  on (items_flat, q_off)
// With a history window (srn_device_sessions_set_history) the store keeps the last H clicks under the same rules -- H takes the limit's place in sess_len and
// sess_store -- and predict reads the last min(window, max_items_in_session) items of each window: sess_len writes that length too, a second scan gives p_off, and
// sess_emit copies the window's suffix into a second buffer.  SRN_FLAG_EXCLUDE_SEEN hands the windows (items_flat, q_off) to the exclusion filter (srn_exclude.hip) as the
// call's exclusion CSR.
//
// The store is the one state of the library that training data cannot rebuild, so whole stores move in bulk, each pass behind `last`:
//   export          live flag per slot, exclusive scan, scatter in slot order into dense arrays (no atomic cursor: an unchanged store exports the same bytes)
//   import          the batch's sort over the entries' keys; one lane per distinct key picks the run's winner (largest epoch, later index on a tie) and claims or
//                   finds its slot; a second kernel writes the winners.  Checked before anything is changed
//   resize / growth table_rebuild into a freshly allocated pair of tables of another capacity or items_cap
//   save / load     the export's arrays behind a 96-byte header with a checksum, written through a rename
// The store forgets a session in two places -- sess_store overwrites the slot of a visitor who returns after idle, and table_rebuild leaves out what is older than the
// TTL (rebuild, resize_locked) -- and an attached session harvest (srn_harvest.hip) is handed the entry at both, before the old bytes go away:
// sess_return_flag + harvest_append between sess_find and sess_store, harvest_dropped behind table_rebuild over the old table.  Without one nothing here differs.
//
// A batch whose requests carry their own clocks (srn_recommend_batch*_at) runs the same sequence with the timed form of sess_find, sess_return_flag
// and sess_store -- one body each, template <bool kTimed>, the untimed instantiation compiled without a trace of the other: a run is cut into SEGMENTS where a request
// finds its predecessor's time idle, headpos marks segment heads, a second max scan keeps the run's head for the slot, and the sessions that end inside the call go to
// the harvest from the call's CSR behind sess_emit.  Without times nothing here differs either.
// The table underneath -- the slot's head, the count and rebuild kernels over a payload functor, the capacity rule (make_room), the sweep's tail, the one-key read-back
// and create's and free's shared halves -- is srn_visitor_table.h's, shared with the click feedback log.  Here: the payload (len, items), the batch kernels, the
// pair of tables and its flip, the harvest hooks, resize and growth, export / import and the file form.
// The sort, the run predicates and the find-or-claim probe are srn_visitors.h's, shared with the feedback log and the harvest; so is what a batch call opens with --
// the sorted front of the call's VisitorBatch (srn_internal.h), the timed / untimed dispatch, the host stage -- over a scratch plan (Bump) and grow_behind.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <unistd.h>

#include <rocprim/rocprim.hpp>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_device.h"
#include "srn_sessions_dev.h"   // the store's handle (shared with srn_trending.hip, srn_harvest.hip) over srn_visitor_table.h: the table, its kernels and the capacity rule
#include "srn_visitors.h"       // the run predicates, find_or_claim, the key sort, the sorted front and the host stage (shared with srn_feedback.hip, srn_harvest.hip)
#include "srn_hipsync.h"

namespace srn {

namespace {
constexpr uint32_t kTPB = kTableTPB;          // (grid_for)

// One struct for the untimed and the timed batch.  Untimed, when, runpos and run_head are null and never read; timed, `now` is not read: a run is cut
// into SEGMENTS wherever a request finds its predecessor's time idle, headpos marks segment heads -- so that run_start becomes the segment start and slen is 0 at a
// break -- and runpos marks run heads only: its inclusive max scan, run_head, is where sess_store<true> and the harvest find the run's slot.
struct BatchArgs {
    Table t;
    const uint64_t* key_hi; const uint64_t* key_lo; const uint64_t* item; const uint8_t* consent;   // the caller's arrays
    const uint32_t* order;   // [n] request index of each sorted position
    uint32_t n, max_items;   // max_items: what predict reads of a window
    uint32_t limit;          // what the store keeps: max_items, or the history window H
    uint64_t now, idle;
    uint32_t* slot_of;       // [n] by sorted position of a run head: its slot (kNone: table full -- cannot happen under the capacity rule)
    uint32_t* slen;          // [n] ... and the stored length the run starts from (0 if idle)
    uint32_t* kept;          // [n + 1] 1 = this request appends
    uint32_t* headpos;       // [n] p for a run head, 0 otherwise; inclusive max scan -> run_start
    uint32_t* kex;           // [n + 1] exclusive sum of kept
    uint32_t* run_start;     // [n]
    uint64_t* compact;       // [n] the kept clicks in sorted order
    uint32_t* qlen;          // [n + 1] by REQUEST index
    uint32_t* q_off;         // [n + 1]
    uint64_t* items_flat;
    uint32_t* plen;          // history window only (null otherwise): [n + 1] by REQUEST index, the length predict reads; p_off its exclusive scan; pflat those suffixes
    uint32_t* p_off;
    uint64_t* pflat;
    uint32_t* err;
    const uint64_t* when;    // timed: [n] times[order[p]], so that a position reads when[p] and when[p - 1] as adjacent words
    uint32_t* runpos;        // timed: [n] p for a run head, 0 otherwise; inclusive max scan -> run_head
    uint32_t* run_head;      // timed: [n]
};

// One lane per sorted position.  A run head finds or claims its slot and reads the stored length under the idle rule, against `now` or (timed) its own time; any
// other request keeps its click iff it differs from its predecessor's, and (timed) starts an empty session where it finds its predecessor's time idle
template <bool kTimed>
__global__ void __launch_bounds__(kTPB) sess_find(BatchArgs a) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p > a.n) return;
    if (p == a.n) { a.kept[p] = 0; return; }
    const uint32_t req = a.order[p];
    if (!consents(a, req)) { a.kept[p] = 0; a.headpos[p] = 0; if constexpr (kTimed) a.runpos[p] = 0; return; }
    const uint64_t hi = a.key_hi[req], lo = a.key_lo[req], item = a.item[req];
    uint64_t now = a.now;
    if constexpr (kTimed) now = a.when[p];
    if (const uint32_t pr = run_prev(a, p, hi, lo); pr != kNone) {
        if constexpr (kTimed) {
            a.runpos[p] = 0;
            if (idle_or_old(now, a.when[p - 1], a.idle)) { a.slen[p] = 0; a.headpos[p] = p; a.kept[p] = 1; return; }   // a break: an empty session, whose first click is kept
        }
        a.headpos[p] = 0; a.kept[p] = item != a.item[pr];
        return;
    }
    const Claim c = find_or_claim(a.t, hi, lo);
    uint32_t stored = 0;
    uint64_t last = 0;
    if (c.slot == kNone) atomicOr(a.err, 1u);
    else {
        SlotHead* s = slot_at(a.t, c.slot);
        if (c.fresh) { s->key_hi = hi; s->key_lo = lo; s->epoch = 0; s->len = 0; }
        else if (const uint32_t len = s->len; len && !idle_or_old(now, s->epoch, a.idle)) { stored = len; last = slot_items(s)[len - 1]; }
    }
    a.slot_of[p] = c.slot; a.slen[p] = stored; a.headpos[p] = p;
    if constexpr (kTimed) a.runpos[p] = p;
    a.kept[p] = stored == 0 || last != item;
}

// the window of a consenting request at sorted position p: `len` items ending `a` kept clicks into the run, over (stored items ++ kept clicks)
__global__ void __launch_bounds__(kTPB) sess_len(BatchArgs a) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p > a.n) return;
    if (p == a.n) { a.qlen[a.n] = 0; if (a.plen) a.plen[a.n] = 0; return; }
    const uint32_t req = a.order[p];
    if (!consents(a, req)) { a.qlen[req] = 1; if (a.plen) a.plen[req] = 1; return; }
    const uint32_t s = a.run_start[p], S = a.slen[s], app = a.kex[p + 1] - a.kex[s];
    const uint32_t wlen = S >= a.limit ? S : min(S + app, a.limit);
    a.qlen[req] = wlen;
    if (a.plen) a.plen[req] = min(wlen, a.max_items);
    if (a.kept[p]) a.compact[a.kex[p]] = a.item[req];
}

__global__ void __launch_bounds__(kTPB) sess_emit(BatchArgs a) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t req = a.order[p];
    uint64_t* dst = a.items_flat + a.q_off[req];
    uint64_t* pdst = a.pflat ? a.pflat + a.p_off[req] : nullptr;
    if (!consents(a, req)) { dst[0] = a.item[req]; if (pdst) pdst[0] = a.item[req]; return; }
    const uint32_t s = a.run_start[p], S = a.slen[s], app = a.kex[p + 1] - a.kex[s], len = a.q_off[req + 1] - a.q_off[req];
    const uint32_t first = S + app - len;
    const uint64_t* stored = S ? slot_items(slot_at(a.t, a.slot_of[s])) : nullptr;
    const uint64_t* clicks = a.compact + a.kex[s];
    for (uint32_t i = 0; i < len; ++i) { const uint32_t at = first + i; dst[i] = at < S ? stored[at] : clicks[at - S]; }
    if (pdst) {   // the window's suffix predict reads
        const uint32_t pl = a.p_off[req + 1] - a.p_off[req], pfirst = S + app - pl;
        for (uint32_t i = 0; i < pl; ++i) { const uint32_t at = pfirst + i; pdst[i] = at < S ? stored[at] : clicks[at - S]; }
    }
}

// the run's last request writes its window -- the final session -- into the run's slot, with `now` or (timed) ITS time, not the largest one
template <bool kTimed>
__global__ void __launch_bounds__(kTPB) sess_store(BatchArgs a) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t req = a.order[p];
    if (!consents(a, req) || !run_last(a, p, req)) return;
    uint32_t head = 0; uint64_t now = a.now;
    if constexpr (kTimed) { head = a.run_head[p]; now = a.when[p]; } else head = a.run_start[p];
    const uint32_t slot = a.slot_of[head];
    if (slot == kNone) return;
    SlotHead* s = slot_at(a.t, slot);
    const uint32_t off = a.q_off[req], len = a.q_off[req + 1] - off;
    uint64_t* it = slot_items(s);
    for (uint32_t i = 0; i < len; ++i) it[i] = a.items_flat[off + i];
    s->len = len; s->epoch = now; s->state = kFull;
}

// Session harvest, return after idle (srn_harvest.hip): flag[p] for sorted position p, behind sess_find and before sess_store.  A run head whose key was found stored
// with len > 0 and idle -- at `now` or (timed) at its own time -- is about to have its slot overwritten: kHvStore (kHvSkip below min_len).  sess_find left such a head
// with slen 0 and the slot untouched (a slot claimed in this call is in state kClaimed with len 0).  flag[n] = 0.
template <bool kTimed>
__global__ void __launch_bounds__(kTPB) sess_return_flag(BatchArgs a, uint32_t min_len, uint64_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p > a.n) return;
    uint64_t f = 0;
    if (p < a.n) {
        const uint32_t req = a.order[p];
        if (consents(a, req) && run_head(a, p, req)) {
            const uint32_t slot = a.slot_of[p];
            if (slot != kNone && a.slen[p] == 0) {
                const SlotHead* s = slot_at(a.t, slot);
                uint64_t now = a.now;
                if constexpr (kTimed) now = a.when[p];
                if (s->state == kFull && s->len > 0 && idle_or_old(now, s->epoch, a.idle)) f = s->len >= min_len ? kHvStore : kHvSkip;
            }
        }
    }
    flag[p] = f;
}
// A timed batch only.  The sessions that end INSIDE the call, behind sess_emit: a break at sorted position p ends the session of position p - 1, whose window is in
// the call's CSR.  flag[p] = kHvStore / kHvSkip by that window's length; flag[n] = 0.  (A break is a segment head that is not a run head.)
__global__ void __launch_bounds__(kTPB) sess_break_flag(BatchArgs a, uint32_t min_len, uint64_t* __restrict__ flag) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p > a.n) return;
    uint64_t f = 0;
    if (p > 0 && p < a.n && a.headpos[p] == p && a.runpos[p] == 0) {
        const uint32_t pr = a.order[p - 1];
        f = a.q_off[pr + 1] - a.q_off[pr] >= min_len ? kHvStore : kHvSkip;
    }
    flag[p] = f;
}

// a NULL store: every request's session is its item
__global__ void __launch_bounds__(kTPB) sess_iota(uint32_t n, uint32_t* q_off) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    if (i <= n) q_off[i] = i;
}

// ---- one key, from the host ----
// the store's payload for the table's rebuild and one-key read-back: out[0] = stored length, out[2..] = items
struct SessSlot {
    using Head = SlotHead;
    __device__ void copy(const SlotHead* s, SlotHead* d) const {
        d->len = s->len;
        for (uint32_t j = 0; j < s->len; ++j) slot_items(d)[j] = slot_items(const_cast<SlotHead*>(s))[j];
    }
    __device__ void read(const SlotHead* s, uint64_t* out) const {
        out[0] = s->len;
        for (uint32_t i = 0; i < s->len; ++i) out[2 + i] = slot_items(const_cast<SlotHead*>(s))[i];
    }
};
// io[0] = n, io[1..] = items in; io[0] <- 1 if the key is new, 0 if it was there, 2 if the table is full
__global__ void sess_put_one(Table t, uint64_t hi, uint64_t lo, uint64_t now, uint64_t* io) {
    const uint32_t n = (uint32_t)io[0];
    uint32_t h = key_hash(hi, lo) & t.mask;
    for (uint32_t probes = 0; probes <= t.mask; ++probes, h = (h + 1) & t.mask) {
        SlotHead* s = slot_at(t, h);
        const bool empty = s->state == kEmpty;
        if (empty || (s->key_hi == hi && s->key_lo == lo)) {
            s->key_hi = hi; s->key_lo = lo; s->epoch = now; s->len = n; s->state = kFull;
            for (uint32_t i = 0; i < n; ++i) slot_items(s)[i] = io[1 + i];
            io[0] = empty ? 1 : 0;
            return;
        }
    }
    io[0] = 2;
}

// ---- bulk export / import / resize ----
// counters[0] = occupied slots, [1] = entries a sweep at `now` keeps, [2] = the longest session among those
__global__ void __launch_bounds__(kTPB) sess_count_max(Table t, uint64_t now, uint64_t ttl, unsigned long long* counters) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    bool occ = false, live = false; uint32_t len = 0;
    if (i <= t.mask) { const SlotHead* s = slot_at(t, i); occ = s->state != kEmpty; live = occ && !idle_or_old(now, s->epoch, ttl); if (live) len = s->len; }
    const unsigned long long mo = __ballot(occ), ml = __ballot(live);
    for (int off = 32; off; off >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, off));
    if ((threadIdx.x & 63) == 0) {
        if (mo) atomicAdd(&counters[0], (unsigned long long)__popcll(mo));
        if (ml) { atomicAdd(&counters[1], (unsigned long long)__popcll(ml)); atomicMax(&counters[2], (unsigned long long)len); }
    }
}
// flag[i] = 1 for an entry a sweep at `now` keeps; flag[n_slots] = 0, so that the exclusive scan's last word is the number of live entries
__global__ void __launch_bounds__(kTPB) sess_live_flag(Table t, uint64_t now, uint64_t ttl, uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    if (i > t.mask + 1u) return;
    uint32_t f = 0;
    if (i <= t.mask) { const SlotHead* s = slot_at(t, i); f = s->state != kEmpty && !idle_or_old(now, s->epoch, ttl); }
    flag[i] = f;
}
struct ExportArgs {
    Table t; const uint32_t* pos;      // [n_slots + 1] exclusive scan of the live flags: a live slot's place among the exported entries
    uint64_t now, ttl, cap, items_stride;
    uint64_t* key_hi; uint64_t* key_lo; uint64_t* epoch; uint32_t* len; uint64_t* items; uint64_t* d_n;
    uint32_t lanes_shift;              // 2^lanes_shift adjacent lanes read one slot, 16 bytes each per round
};
// Slot -> dense arrays.  A slot is 16-byte elements: 0 = the key, 1 = epoch | len | state, 2.. = item pairs; lane e of a slot's group reads element e, e + lanes, ...
// so a wave reads whole slots with adjacent lanes and writes each dense array in runs of adjacent words.  Items from `len` on are written as zero.
__global__ void __launch_bounds__(kTPB) sess_export_scatter(ExportArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    if (tid == 0) *a.d_n = a.pos[a.t.mask + 1u];
    const uint64_t slot = tid >> a.lanes_shift;
    const uint32_t lanes = 1u << a.lanes_shift, lane = (uint32_t)tid & (lanes - 1);
    if (slot > a.t.mask) return;
    const SlotHead* s = slot_at(a.t, (uint32_t)slot);
    const uint64_t ep = s->epoch;
    if (s->state == kEmpty || idle_or_old(a.now, ep, a.ttl)) return;
    const uint64_t d = a.pos[slot];
    if (d >= a.cap) return;
    const uint32_t len = s->len;
    const ulonglong2* el = (const ulonglong2*)s;
    const uint64_t n_el = 2 + (a.items_stride + 1) / 2;
    for (uint64_t e = lane; e < n_el; e += lanes) {
        if (e == 0) { const ulonglong2 v = el[0]; a.key_hi[d] = v.x; a.key_lo[d] = v.y; }
        else if (e == 1) { a.epoch[d] = ep; a.len[d] = len; }
        else {
            const uint64_t j = 2 * (e - 2);
            ulonglong2 v = make_ulonglong2(0, 0);
            if (j < len) { v = el[e]; if (j + 1 >= len) v.y = 0; }   // (j < len <= items_cap: the pair lies inside the slot, whose size is a multiple of 128)
            uint64_t* dst = a.items + d * a.items_stride + j;
            dst[0] = v.x; if (j + 1 < a.items_stride) dst[1] = v.y;
        }
    }
}

struct ImportArgs {
    Table t;
    const uint64_t* key_hi; const uint64_t* key_lo; const uint64_t* epoch; const uint32_t* len; const uint64_t* items; uint64_t items_stride;   // the caller's arrays
    const uint32_t* order;   // [n] entry index of each sorted position
    uint32_t n;
    uint32_t* slot_of;       // [n] by sorted position of a run head: its slot
    uint32_t* win;           // [n] ... and the entry that is written there (kNone: the stored entry is newer, or not a head)
    uint32_t* err;
    static constexpr const uint8_t* consent = nullptr;   // (run_head: every entry takes part)
};
__global__ void __launch_bounds__(kTPB) sess_import_maxlen(const uint32_t* __restrict__ len, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kTPB + threadIdx.x;
    uint32_t v = i < n ? len[i] : 0;
    for (int off = 32; off; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
    if ((threadIdx.x & 63) == 0 && v) atomicMax(out, v);
}
// one lane per distinct key (the head of its run): the run's winner -- largest epoch, the later entry on a tie -- and find-or-insert as sess_find does it.  A slot
// claimed here stays in state 2 until sess_import_write, so every slot in state 1 was complete before this kernel began and its key can be compared
__global__ void __launch_bounds__(kTPB) sess_import_find(ImportArgs a) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t e0 = a.order[p];
    const uint64_t hi = a.key_hi[e0], lo = a.key_lo[e0];
    if (run_prev(a, p, hi, lo) != kNone) { a.slot_of[p] = kNone; a.win[p] = kNone; return; }   // not a head
    uint32_t w = e0; uint64_t we = a.epoch[e0];
    for (uint32_t q = p + 1; q < a.n; ++q) {   // (the sort is stable: a later position of the run is a later entry)
        const uint32_t r = a.order[q];
        if (a.key_hi[r] != hi || a.key_lo[r] != lo) break;
        const uint64_t re = a.epoch[r];
        if (re >= we) { w = r; we = re; }
    }
    const Claim c = find_or_claim(a.t, hi, lo);
    if (c.slot == kNone) { atomicOr(a.err, 1u); w = kNone; }
    else if (!c.fresh && we < slot_at(a.t, c.slot)->epoch) w = kNone;   // the stored entry is newer: it stays
    a.slot_of[p] = c.slot; a.win[p] = w;
}
// 16 adjacent lanes write one winner into its slot, a 16-byte element each per round (the layout of sess_export_scatter)
__global__ void __launch_bounds__(kTPB) sess_import_write(ImportArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    const uint64_t p = tid >> 4; const uint32_t lane = (uint32_t)tid & 15u;
    if (p >= a.n) return;
    const uint32_t w = a.win[p];
    if (w == kNone) return;
    SlotHead* s = slot_at(a.t, a.slot_of[p]);
    const uint32_t len = a.len[w];
    const uint64_t* src = a.items + (uint64_t)w * a.items_stride;
    uint64_t* it = slot_items(s);
    for (uint32_t e = lane; e < 2 + (len + 1) / 2; e += 16) {
        if (e == 0) { s->key_hi = a.key_hi[w]; s->key_lo = a.key_lo[w]; }
        else if (e == 1) { s->epoch = a.epoch[w]; s->len = len; s->state = kFull; }
        else { const uint32_t j = 2 * (e - 2); it[j] = src[j]; if (j + 1 < len) it[j + 1] = src[j + 1]; }
    }
}

}  // namespace

}  // namespace srn

using namespace srn;

namespace srn {

void dsess_free(srn_device_sessions* s) {
    if (!s) return;
    if (s->harvest) { std::lock_guard<std::mutex> g(s->harvest->mu); s->harvest->store = nullptr; s->harvest = nullptr; }   // freeing the store detaches its harvest, before its stream goes
    table_release(s);
    for (hipEvent_t e : s->tev) if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)s->old, (void*)s->stage, (void*)s->xs, (void*)s->hs}) if (p) (void)hipFree(p);
    delete s;
}

int dsess_create(int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions** out) {
    if (!out) return fail(SRN_EINVAL, "srn_device_sessions_create: null output");
    *out = nullptr;
    if (items_cap == 0) return fail(SRN_EINVAL, "srn_device_sessions_create: items_cap must be > 0");
    if (items_cap > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "srn_device_sessions_create: items_cap above SRN_MAX_SESSION_LEN");
    srn_device_sessions* s = new srn_device_sessions();
    struct Guard { srn_device_sessions*& s; ~Guard() { if (s) dsess_free(s); } } guard{s};
    s->items_cap = items_cap;
    const int rc = table_create(s, "srn_device_sessions_create", "device session store", device, capacity, ttl_secs, idle_secs, kSlotHead, items_cap, 2 + SRN_MAX_SESSION_LEN + 1);
    if (rc) return rc;
    const size_t bytes = (size_t)s->n_slots * s->stride;
    for (char** t : {&s->table, &s->old})
        if (hipMalloc((void**)t, bytes) != hipSuccess) { (void)hipGetLastError(); *t = nullptr; return fail(SRN_ENOMEM, "srn_device_sessions_create: no device memory for the table"); }
    for (hipEvent_t& e : s->tev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipMemsetAsync(s->table, 0, bytes, s->own));
    HIP_TRY(hipStreamSynchronize(s->own));
    *out = s; s = nullptr;
    return SRN_OK;
}

namespace {
// room for an attached harvest's append over n table slots (own stream behind `last`, mu held).  A scratch of its own: a rebuild runs inside make_room, below an
// import that already holds pointers into the export / import scratch, which must neither move nor be overwritten here
int harvest_room(srn_device_sessions* s, size_t n) {
    size_t bytes = 0;
    int rc = harvest_scratch_bytes(n, &bytes); if (rc) return rc;
    if (bytes <= s->hs_bytes) return SRN_OK;
    HIP_TRY(hipStreamSynchronize(s->own));   // (only rebuilds use it, on the own stream: wait for the previous one before it is freed)
    return ensure(&s->hs, &s->hs_bytes, bytes);
}

int rebuild(srn_device_sessions* s, uint64_t now) {   // (own stream, mu held)
    const Table from = s->tab(); Table to = from; to.base = s->old;
    if (s->harvest) { const int rc = harvest_room(s, s->n_slots); if (rc) return rc; }
    HIP_TRY(rebuild_into(s, to, now, SessSlot{}));
    if (s->harvest) { const int rc = harvest_dropped(s->harvest, from, now, s->ttl, s->hs, s->own); if (rc) return rc; }   // what the rebuild left out, from the old table (it stays until the next rebuild)
    std::swap(s->table, s->old); ++s->sweeps;
    return SRN_OK;
}
int count_max(srn_device_sessions* s, uint64_t now, uint64_t* occupied, uint64_t* live, uint64_t* longest) {   // blocks (own stream, mu held)
    HIP_TRY(hipMemsetAsync(s->counters(), 0, 24, s->own));
    sess_count_max<<<grid_for(s->n_slots), kTPB, 0, s->own>>>(s->tab(), now, s->ttl, s->counters());
    HIP_TRY(hipGetLastError());
    unsigned long long c[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(c, s->counters(), 24, hipMemcpyDeviceToHost, s->own));
    HIP_TRY(hipStreamSynchronize(s->own));
    *occupied = c[0]; *live = c[1]; *longest = c[2];
    return SRN_OK;
}
// Rebuilds the entries a sweep at `now` keeps into tables of another shape (own stream, mu held, behind `last`; blocks).  Both new tables are allocated before the
// old ones are touched -- peak device memory is the old pair + the new pair -- and every failure leaves the store as it was.
int resize_locked(srn_device_sessions* s, uint64_t capacity, uint64_t items_cap, uint64_t now, const char* who) {
    uint64_t occupied = 0, live = 0, longest = 0;
    if (s->harvest && items_cap > s->harvest->items_cap) return fail(SRN_ERANGE, std::string(who) + ": the new items_cap is above the attached harvest's");
    int rc = count_max(s, now, &occupied, &live, &longest); if (rc) return rc;
    if (live > capacity) return fail(SRN_ENOMEM, std::string(who) + ": more live sessions than the new capacity");
    if (longest > items_cap) return fail(SRN_ERANGE, std::string(who) + ": a stored session is longer than the new items_cap");
    const uint64_t n_slots = slots_for(capacity); const uint32_t stride = stride_for(kSlotHead, items_cap);
    const size_t bytes = (size_t)n_slots * stride;
    if (s->harvest && (rc = harvest_room(s, s->n_slots))) return rc;   // (a refused or failed resize harvests nothing: the append is enqueued behind the rebuild below)
    char* nt[2] = {nullptr, nullptr};
    for (int i = 0; i < 2; ++i)
        if (hipMalloc((void**)&nt[i], bytes) != hipSuccess) {
            (void)hipGetLastError();
            if (nt[0]) (void)hipFree(nt[0]);
            return fail(SRN_ENOMEM, std::string(who) + ": no device memory for the new tables");
        }
    const Table from = s->tab(), to{nt[0], (uint32_t)(n_slots - 1), stride};
    hipError_t e = rebuild_into(s, to, now, SessSlot{});
    if (e == hipSuccess && s->harvest && (rc = harvest_dropped(s->harvest, from, now, s->ttl, s->hs, s->own))) {   // from the old table, before it is freed
        (void)hipStreamSynchronize(s->own); (void)hipFree(nt[0]); (void)hipFree(nt[1]);
        return rc;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s->own);
    if (e != hipSuccess) { (void)hipFree(nt[0]); (void)hipFree(nt[1]); return fail(SRN_EHIP, std::string(who) + ": " + hipGetErrorString(e)); }
    (void)hipFree(s->table); (void)hipFree(s->old);
    s->table = nt[0]; s->old = nt[1];
    s->capacity = capacity; s->items_cap = items_cap; s->n_slots = n_slots; s->stride = stride;
    s->bound = live; s->len_bound = std::max<uint32_t>(1u, std::min<uint32_t>(s->len_bound, (uint32_t)items_cap));
    ++s->resizes;
    return SRN_OK;
}
// opt-in growth: the smallest power-of-two multiple of the capacity that holds `need`, if max_capacity allows it (the capacity rule already waits for the device here)
int grow(srn_device_sessions* s, uint64_t need, uint64_t now) {
    uint64_t grown = s->capacity;
    while (grown < need && grown < s->max_capacity) grown *= 2;
    if (grown < need || grown > s->max_capacity) return SRN_ENOMEM;
    const int rc = resize_locked(s, grown, s->items_cap, now, "device session store (growth)");
    if (rc == SRN_OK) ++s->grows;
    return rc;
}
// the capacity rule (srn_visitor_table.h) with the store's rebuild and growth (mu held)
int room_for(srn_device_sessions* s, uint64_t n, uint64_t now) {
    return make_room(s, n, now, [s](uint64_t at) { return rebuild(s, at); }, [s](uint64_t need, uint64_t at) { return grow(s, need, at); });
}
}  // namespace

int dsess_get(srn_device_sessions* s, uint64_t hi, uint64_t lo, uint64_t now_secs, uint64_t* out_items, size_t cap, size_t* out_n) {
    if (!s || !out_n || (cap && !out_items)) return fail(SRN_EINVAL, "srn_device_sessions_get: null argument");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    *out_n = 0;
    std::vector<uint64_t> h; bool found = false;
    const int rc = read_one(s, hi, lo, now, SessSlot{}, 2 + s->items_cap, &h, &found);
    if (rc || !found) return rc;
    if (h[0] > cap) return fail(SRN_ERANGE, "srn_device_sessions_get: output buffer too small");
    std::memcpy(out_items, h.data() + 2, h[0] * 8);
    *out_n = (size_t)h[0];
    return SRN_OK;
}

int dsess_update(srn_device_sessions* s, uint64_t hi, uint64_t lo, uint64_t now_secs, const uint64_t* items, size_t n) {
    if (!s || (n && !items)) return fail(SRN_EINVAL, "srn_device_sessions_update: null argument");
    if (n > s->items_cap) return fail(SRN_ERANGE, "srn_device_sessions_update: session longer than the store's items_cap");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    int rc = room_for(s, 1, now); if (rc) return rc;
    if ((rc = own_after_last(s))) return rc;
    std::vector<uint64_t> h(1 + n); h[0] = n;
    if (n) std::memcpy(h.data() + 1, items, n * 8);
    HIP_TRY(hipMemcpyAsync(s->one(), h.data(), h.size() * 8, hipMemcpyHostToDevice, s->own));
    sess_put_one<<<1, 1, 0, s->own>>>(s->tab(), hi, lo, now, s->one());
    HIP_TRY(hipGetLastError());
    uint64_t res = 0;
    HIP_TRY(hipMemcpyAsync(&res, s->one(), 8, hipMemcpyDeviceToHost, s->own));
    HIP_TRY(hipStreamSynchronize(s->own));
    if (res == 2) return fail(SRN_ENOMEM, "srn_device_sessions_update: the table is full");
    s->bound += res;
    s->len_bound = std::max<uint32_t>(s->len_bound, (uint32_t)n);
    return SRN_OK;
}

int dsess_sweep(srn_device_sessions* s, uint64_t now_secs, uint64_t* n_live) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_sweep: null store");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    return sweep(s, now, [s](uint64_t at) { return rebuild(s, at); }, n_live);
}

int dsess_stats(srn_device_sessions* s, srn_device_sessions_stats_t* out) {
    if (!s || !out) return fail(SRN_EINVAL, "srn_device_sessions_stats: null argument");
    std::lock_guard<std::mutex> g(s->mu);
    *out = srn_device_sessions_stats_t{s->capacity, s->n_slots, s->items_cap, s->stride, s->bound, s->sweeps, s->refused, s->ttl, s->idle, s->len_bound};
    return SRN_OK;
}

int dsess_set_history(srn_device_sessions* s, size_t history) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_set_history: null store");
    std::lock_guard<std::mutex> g(s->mu);
    if (history > s->items_cap) return fail(SRN_ERANGE, "srn_device_sessions_set_history: history above the store's items_cap");
    s->history = (uint32_t)history;
    return SRN_OK;
}
int dsess_history(srn_device_sessions* s, size_t* out) {
    if (!s || !out) return fail(SRN_EINVAL, "srn_device_sessions_history: null argument");
    std::lock_guard<std::mutex> g(s->mu);
    *out = s->history;
    return SRN_OK;
}

int dsess_timing(srn_device_sessions* s, int enable) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_timing: null store");
    std::lock_guard<std::mutex> g(s->mu);
    s->timing = enable != 0;
    return SRN_OK;
}
int dsess_last_ms(srn_device_sessions* s, double* ms_store, double* ms_predict) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_last_ms: null store");
    std::lock_guard<std::mutex> g(s->mu);
    if (!s->last_timed) return fail(SRN_EINVAL, "srn_device_sessions_last_ms: the last batch was not timed (srn_device_sessions_timing)");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventSynchronize(s->tev[2]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, s->tev[0], s->tev[1]));
    HIP_TRY(hipEventElapsedTime(&b, s->tev[1], s->tev[2]));
    if (ms_store) *ms_store = a;
    if (ms_predict) *ms_predict = b;
    return SRN_OK;
}

int dsess_last_csr(srn_device_sessions* s, const void** d_items, const void** d_qoff, size_t* n, size_t* max_len, uint64_t* h_items, size_t cap, uint32_t* h_qoff) {
    if (!s) return fail(SRN_EINVAL, "null store");
    std::lock_guard<std::mutex> g(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipEventSynchronize(s->last));
    if (d_items) *d_items = s->last_items;
    if (d_qoff) *d_qoff = s->last_qoff;
    if (n) *n = s->last_n;
    if (max_len) *max_len = s->last_hint;
    if (h_qoff && s->last_n) {
        HIP_TRY(hipMemcpy(h_qoff, s->last_qoff, (s->last_n + 1) * 4, hipMemcpyDeviceToHost));
        const size_t total = h_qoff[s->last_n];
        if (h_items) {
            if (total > cap) return fail(SRN_ERANGE, "no room for the emitted sessions");
            HIP_TRY(hipMemcpy(h_items, s->last_items, total * 8, hipMemcpyDeviceToHost));
        }
    }
    return SRN_OK;
}

// a NULL store (no request consents): the sessions are the items themselves.  Not the serving path: it allocates and blocks.
static int recommend_no_store(const srn_index* idx, const uint64_t* d_item, const uint8_t* d_consent, size_t n, LaunchParams p, hipStream_t st, bool fill) {
    if (!d_consent) return fail(SRN_EINVAL, "srn_recommend_batch: user consent needs a session store");
    HIP_TRY(hipSetDevice(idx->device));
    std::vector<uint8_t> c(n);
    HIP_TRY(hipMemcpyAsync(c.data(), d_consent, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (std::any_of(c.begin(), c.end(), [](uint8_t x) { return x != 0; })) return fail(SRN_EINVAL, "srn_recommend_batch: user consent needs a session store");
    uint32_t* q_off = nullptr;
    HIP_TRY(hipMalloc((void**)&q_off, (n + 1) * 4));
    sess_iota<<<grid_for(n + 1), kTPB, 0, st>>>((uint32_t)n, q_off);
    p.max_len = 1; p.items_flat = d_item; p.q_off = q_off;
    RowRule rule; rule.fill = fill;
    int rc = hipGetLastError() == hipSuccess ? device_predict_device(idx->dev, idx->flat, p, st, rule) : fail(SRN_EHIP, "sess_iota launch failed");
    (void)hipStreamSynchronize(st);
    (void)hipFree(q_off);
    return rc;
}

// The checks every form of the call shares, in the order the entry points have always made them; the C ABI glue has checked predict's own arguments, the buffers
// and n > 0.  host: the host-pointer form can read the consent array, so a call without a store that needs one is refused before anything is staged
static int check_recommend(const srn_device_sessions* s, const VisitorBatch& r, const RecommendCall& c, bool host) {
    if (c.max_items == 0) return fail(SRN_EINVAL, "srn_recommend_batch: max_items_in_session must be > 0");
    if (host && !s && (!r.consent || std::any_of(r.consent, r.consent + r.n, [](uint8_t x) { return x != 0; }))) return fail(SRN_EINVAL, "srn_recommend_batch: user consent needs a session store");
    if (r.n > kMaxBatch) return fail(SRN_ERANGE, "srn_recommend_batch: more than 2^24 requests in one call");
    return SRN_OK;
}

// a call's windows against the store (mu held), and SRN_FLAG_EXCLUDE_SEEN's room behind the longest window the store may hold
static int check_windows(const srn_device_sessions* s, const srn_index* idx, size_t max_items) {
    if (max_items > s->items_cap) return fail(SRN_ERANGE, "srn_recommend_batch: max_items_in_session above the store's items_cap");
    if (s->device != idx->device) return fail(SRN_EINVAL, "srn_recommend_batch: the store and the index are on different devices");
    const uint32_t H = s->history;
    if (H > s->items_cap) return fail(SRN_ERANGE, "srn_recommend_batch: the store's history window is above its items_cap (lowered by a resize): set a smaller history or resize again");
    if (H && max_items > H) return fail(SRN_ERANGE, "srn_recommend_batch: max_items_in_session above the store's history window");
    return SRN_OK;
}
static int check_exclude_seen(size_t how_many, uint32_t hint) {
    return how_many + hint > SRN_MAX_HOW_MANY ? fail(SRN_ERANGE, "srn_recommend_batch: how_many + the store's longest window above SRN_MAX_HOW_MANY (SRN_FLAG_EXCLUDE_SEEN)") : SRN_OK;
}

// The traffic split's front (srn_arms.hip): every arm's checks against the store as its own call would make them, then the capacity rule for all n requests at once --
// the arms' calls, whose sizes sum to n, then pass theirs.  hint grows from arm to arm as the calls will leave it
int dsess_admit(srn_device_sessions* s, const srn_index* const* idx, const RecommendCall* c, size_t n_arms, uint64_t n, uint64_t now) {
    std::lock_guard<std::mutex> g(s->mu);
    uint32_t hint = s->len_bound;
    for (size_t a = 0; a < n_arms; ++a) {
        if (c[a].max_items == 0) return fail(SRN_EINVAL, "srn_recommend_batch: max_items_in_session must be > 0");
        int rc = check_windows(s, idx[a], c[a].max_items); if (rc) return rc;
        hint = std::max<uint32_t>(hint, s->history ? s->history : (uint32_t)c[a].max_items);
        if ((c[a].flags & SRN_FLAG_EXCLUDE_SEEN) && (rc = check_exclude_seen(c[a].how_many, hint))) return rc;
    }
    return room_for(s, n, now);
}

int dsess_recommend_device(const srn_index* idx, srn_device_sessions* s, const VisitorBatch& r, const RecommendCall& c) {
    int rc = check_recommend(s, r, c, false); if (rc) return rc;
    const size_t n = r.n, max_items = c.max_items, how_many = c.how_many;
    hipStream_t st = (hipStream_t)c.stream;
    const bool excl_seen = (c.flags & SRN_FLAG_EXCLUDE_SEEN) != 0u, fill = (c.flags & SRN_FLAG_FILL) != 0u;   // (SRN_FLAG_FILL: srn_fill.hip, behind the call's launch sequence and filter)
    LaunchParams p = launch_params(n, c.k, c.m, how_many, c.flags & ~(unsigned)(SRN_FLAG_EXCLUDE_SEEN | SRN_FLAG_FILL), 0, nullptr, nullptr, c.ids, c.scores, c.counts);   // (the sessions: below)
    if (!s) {   // (every session is its item, which is never in its own row: SRN_FLAG_EXCLUDE_SEEN has nothing to exclude)
        if (max_items > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "srn_recommend_batch: max_items_in_session above SRN_MAX_SESSION_LEN");
        return recommend_no_store(idx, r.item, r.consent, n, p, st, fill);
    }
    const uint64_t now = r.now_secs ? r.now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    if ((rc = check_windows(s, idx, max_items))) return rc;
    const uint32_t H = s->history, limit = H ? H : (uint32_t)max_items;
    const uint32_t hint = std::max<uint32_t>(s->len_bound, limit);          // the longest window the store may hold behind this call
    const uint32_t phint = H ? (uint32_t)max_items : hint;                  // ... and the longest session predict reads
    if (excl_seen && (rc = check_exclude_seen(how_many, hint))) return rc;
    if ((rc = room_for(s, n, now))) return rc;
    HIP_TRY(hipSetDevice(s->device));
    // scratch: the sorted front's (sort keys and indices, rocPRIM's temporary storage -- also the scans' -- and a timed batch's times), then the per-position and
    // per-request words, the kept clicks and the CSR batch; a region under a condition is null where the condition does not hold
    size_t scan = 0, t1 = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n + 1, rocprim::plus<uint32_t>(), st));
    HIP_TRY(rocprim::inclusive_scan(nullptr, t1, (uint32_t*)nullptr, (uint32_t*)nullptr, n, rocprim::maximum<uint32_t>(), st)); scan = std::max(scan, t1);
    srn_harvest* const hv = s->harvest;
    size_t hv_bytes = 0;   // an attached harvest's flags, places and scan storage for the heads that return after idle
    if (hv && (rc = harvest_scratch_bytes(n, &hv_bytes))) return rc;
    Bump b; SortedFront front;
    if ((rc = front.plan(b, r, st, scan))) return rc;
    const auto slot_of = b.of<uint32_t>(n + 1), slen = b.of<uint32_t>(n + 1), kept = b.of<uint32_t>(n + 1), headpos = b.of<uint32_t>(n + 1), kex = b.of<uint32_t>(n + 1),
               run_start = b.of<uint32_t>(n + 1), qlen = b.of<uint32_t>(n + 1), q_off = b.of<uint32_t>(n + 1);
    const auto compact = b.of<uint64_t>(n), items_flat = b.of<uint64_t>(n * (size_t)hint);
    Bump::Region<uint32_t> plen, p_off, runpos, run_head; Bump::Region<uint64_t> pflat, hv_words;
    if (H) { plen = b.of<uint32_t>(n + 1); p_off = b.of<uint32_t>(n + 1); pflat = b.of<uint64_t>(n * (size_t)phint); }
    if (hv) hv_words = b.take<uint64_t>(hv_bytes);
    if (r.times) { runpos = b.of<uint32_t>(n + 1); run_head = b.of<uint32_t>(n + 1); }   // a timed batch: a second max scan for the run's slot
    if ((rc = grow_behind(s->last, &s->ws, &s->ws_bytes, b.bytes))) return rc;
    HIP_TRY(hipStreamWaitEvent(st, s->last, 0));
    const bool timed = s->timing;
    if (timed) HIP_TRY(hipEventRecord(s->tev[0], st));
    char* const ws = s->ws;
    if ((rc = front.run(ws, r, st))) return rc;
    const dim3 gn = grid_for(n), gn1 = grid_for(n + 1);
    BatchArgs a{};
    a.t = s->tab(); a.key_hi = r.key_hi; a.key_lo = r.key_lo; a.item = r.item; a.consent = r.consent; a.order = front.order; a.n = (uint32_t)n; a.max_items = (uint32_t)max_items; a.limit = limit;
    a.plen = plen.at(ws); a.p_off = p_off.at(ws); a.pflat = pflat.at(ws);
    a.now = now; a.idle = s->idle;
    a.slot_of = slot_of.at(ws); a.slen = slen.at(ws); a.kept = kept.at(ws); a.headpos = headpos.at(ws);
    a.kex = kex.at(ws); a.run_start = run_start.at(ws); a.qlen = qlen.at(ws); a.q_off = q_off.at(ws);
    a.compact = compact.at(ws); a.items_flat = items_flat.at(ws); a.err = s->err();
    a.when = front.when; a.runpos = runpos.at(ws); a.run_head = run_head.at(ws);
    uint64_t* const hv_flags = hv_words.at(ws);
    char* const tmp = front.tmp; const size_t tmp_bytes = front.tmp_bytes;
    by_timed(r, [&](auto t) { sess_find<decltype(t)::value><<<gn1, kTPB, 0, st>>>(a); });
    if (hv) {   // the stored sessions the heads found idle, copied before sess_store overwrites their slots
        by_timed(r, [&](auto t) { sess_return_flag<decltype(t)::value><<<gn1, kTPB, 0, st>>>(a, hv->min_len, hv_flags); });
        HIP_TRY(hipGetLastError());
        if ((rc = harvest_append(hv, a.t, a.slot_of, n, (char*)hv_flags, true, st))) return rc;
    }
    t1 = tmp_bytes; HIP_TRY(rocprim::exclusive_scan(tmp, t1, a.kept, a.kex, 0u, n + 1, rocprim::plus<uint32_t>(), st));
    t1 = tmp_bytes; HIP_TRY(rocprim::inclusive_scan(tmp, t1, a.headpos, a.run_start, n, rocprim::maximum<uint32_t>(), st));
    if (r.times) { t1 = tmp_bytes; HIP_TRY(rocprim::inclusive_scan(tmp, t1, a.runpos, a.run_head, n, rocprim::maximum<uint32_t>(), st)); }
    sess_len<<<gn1, kTPB, 0, st>>>(a);   // (run_start is the segment start and slen 0 at a break: sess_len and sess_emit read a timed batch as they read any other)
    t1 = tmp_bytes; HIP_TRY(rocprim::exclusive_scan(tmp, t1, a.qlen, a.q_off, 0u, n + 1, rocprim::plus<uint32_t>(), st));
    if (H) { t1 = tmp_bytes; HIP_TRY(rocprim::exclusive_scan(tmp, t1, a.plen, a.p_off, 0u, n + 1, rocprim::plus<uint32_t>(), st)); }
    sess_emit<<<gn, kTPB, 0, st>>>(a);
    if (r.times && hv) {   // the sessions ended inside the call, from the windows just emitted
        sess_break_flag<<<gn1, kTPB, 0, st>>>(a, hv->min_len, hv_flags);
        HIP_TRY(hipGetLastError());
        if ((rc = harvest_append_csr(hv, a.order, r.key_hi, r.key_lo, a.when, a.items_flat, a.q_off, n, (char*)hv_flags, st))) return rc;
    }
    by_timed(r, [&](auto t) { sess_store<decltype(t)::value><<<gn, kTPB, 0, st>>>(a); });
    HIP_TRY(hipGetLastError());
    // from here on the store has changed: whatever happens below, the next call is ordered behind this one
    s->bound += n;
    s->len_bound = hint;
    p.max_len = phint; p.items_flat = H ? a.pflat : a.items_flat; p.q_off = H ? a.p_off : a.q_off;
    s->last_items = p.items_flat; s->last_qoff = p.q_off; s->last_n = n; s->last_hint = phint;
    if (timed) (void)hipEventRecord(s->tev[1], st);
    RowRule rule; rule.fill = fill;
    if (excl_seen) { rule.x_flat = a.items_flat; rule.x_off = a.q_off; rule.max_excl = hint; }   // the windows are the exclusion CSR, the bound of their lengths its capacity: the launch sequence runs at how_many + hint (srn_exclude.hip)
    rc = device_predict_device(idx->dev, idx->flat, p, st, rule);
    (void)hipSetDevice(s->device);
    if (timed) (void)hipEventRecord(s->tev[2], st);
    s->last_timed = timed;
    (void)hipEventRecord(s->last, st);
    return rc;
}

int dsess_recommend_host(const srn_index* idx, srn_device_sessions* s, const VisitorBatch& r, const RecommendCall& c) {
    int rc = check_recommend(s, r, c, true); if (rc) return rc;
    HIP_TRY(hipSetDevice(idx->device));
    // device copies: the store's staging, or (no store) a buffer of this call's own
    const size_t n = r.n, rows = n * c.how_many;
    Bump b; StagedBatch in;
    in.plan(b, r);
    const auto ids = b.of<uint64_t>(rows); const auto scores = b.of<double>(rows); const auto counts = b.of<uint32_t>(n);
    StageBuf own_buf; hipStream_t st = nullptr;
    std::unique_lock<std::mutex> sl;
    if (s) {
        sl = std::unique_lock<std::mutex>(s->stage_mu);
        if (s->device != idx->device) return fail(SRN_EINVAL, "srn_recommend_batch: the store and the index are on different devices");
        if ((rc = ensure(&s->stage, &s->stage_bytes, b.bytes))) return rc;
        st = s->own;
    } else {
        HIP_TRY(hipMalloc((void**)&own_buf.p, b.bytes));
    }
    char* const base = s ? s->stage : own_buf.p;
    VisitorBatch dr; RecommendCall dc = c;
    dc.ids = ids.at(base); dc.scores = scores.at(base); dc.counts = counts.at(base); dc.stream = st;
    if ((rc = in.upload(base, r, st, &dr))) return rc;
    HIP_TRY(hipMemsetAsync(dc.ids, 0, counts.off - ids.off, st));   // (entries beyond a row's count read as zero, as in buffers a caller cleared)
    if ((rc = dsess_recommend_device(idx, s, dr, dc))) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(hipSetDevice(idx->device));
    HIP_TRY(hipMemcpyAsync(c.ids, dc.ids, rows * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.scores, dc.scores, rows * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c.counts, dc.counts, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return check_all_served(c.counts, n);
}

// ---- snapshot: count, bulk export / import, resize, growth, the file form ----
namespace {

// flags, scan, scatter on `st`, which already waits for `last` (mu held)
int export_enqueue(srn_device_sessions* s, uint64_t now, size_t cap, uint64_t* d_hi, uint64_t* d_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items,
                   size_t items_stride, uint64_t* d_n, hipStream_t st) {
    const size_t n1 = (size_t)s->n_slots + 1;
    size_t tmp = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, n1, rocprim::plus<uint32_t>(), st));
    Bump b;
    const auto flag_at = b.of<uint32_t>(n1), pos_at = b.of<uint32_t>(n1); const auto tmp_at = b.of<char>(tmp);
    const int rc = grow_behind(s->last, &s->xs, &s->xs_bytes, b.bytes); if (rc) return rc;
    uint32_t* flag = flag_at.at(s->xs); uint32_t* pos = pos_at.at(s->xs);
    sess_live_flag<<<grid_for(n1), kTPB, 0, st>>>(s->tab(), now, s->ttl, flag);
    HIP_TRY(rocprim::exclusive_scan(tmp_at.at(s->xs), tmp, flag, pos, 0u, n1, rocprim::plus<uint32_t>(), st));
    ExportArgs a{};
    a.t = s->tab(); a.pos = pos; a.now = now; a.ttl = s->ttl; a.cap = cap; a.items_stride = items_stride;
    a.key_hi = d_hi; a.key_lo = d_lo; a.epoch = d_epoch; a.len = d_len; a.items = d_items; a.d_n = d_n;
    a.lanes_shift = s->stride == 128 ? 3 : 4;
    sess_export_scatter<<<grid_for((size_t)s->n_slots << a.lanes_shift), kTPB, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    return SRN_OK;
}

// the blocking export into host arrays (own stream, mu held, behind `last`).  exact_stride: items_stride need only hold the longest live session (save)
int export_host_locked(srn_device_sessions* s, uint64_t now, size_t cap, uint64_t* hi, uint64_t* lo, uint64_t* epoch, uint32_t* len, uint64_t* items,
                       size_t items_stride, size_t* n, bool exact_stride, const char* who) {
    uint64_t occupied = 0, live = 0, longest = 0;
    int rc = count_max(s, now, &occupied, &live, &longest); if (rc) return rc;
    *n = (size_t)live;
    if (items_stride < (exact_stride ? longest : (uint64_t)s->len_bound)) return fail(SRN_ERANGE, std::string(who) + ": items_stride below the longest session the store may hold");
    if (live > cap) return fail(SRN_ERANGE, std::string(who) + ": more live sessions than the arrays hold (*n is their number)");
    if (live == 0) return SRN_OK;
    const Dense d(live, items_stride);
    StageBuf b; if ((rc = b.alloc(d.bytes, who))) return rc;
    rc = export_enqueue(s, now, live, d.hi.at(b.p), d.lo.at(b.p), d.ep.at(b.p), d.len.at(b.p), d.items.at(b.p), items_stride, d.word.at(b.p), s->own);
    if (rc) { (void)hipStreamSynchronize(s->own); return rc; }
    hipError_t e = hipMemcpyAsync(hi, d.hi.at(b.p), live * 8, hipMemcpyDeviceToHost, s->own);
    if (e == hipSuccess) e = hipMemcpyAsync(lo, d.lo.at(b.p), live * 8, hipMemcpyDeviceToHost, s->own);
    if (e == hipSuccess) e = hipMemcpyAsync(epoch, d.ep.at(b.p), live * 8, hipMemcpyDeviceToHost, s->own);
    if (e == hipSuccess) e = hipMemcpyAsync(len, d.len.at(b.p), live * 4, hipMemcpyDeviceToHost, s->own);
    if (e == hipSuccess && items_stride) e = hipMemcpyAsync(items, d.items.at(b.p), live * items_stride * 8, hipMemcpyDeviceToHost, s->own);
    const hipError_t e2 = hipStreamSynchronize(s->own);
    if (e != hipSuccess || e2 != hipSuccess) return fail(SRN_EHIP, std::string(who) + ": " + hipGetErrorString(e != hipSuccess ? e : e2));
    return SRN_OK;
}

// validate (blocks), apply the capacity rule, then sort / find / write on `st` (mu held).  Nothing is changed before every check has passed.
int import_locked(srn_device_sessions* s, const uint64_t* d_hi, const uint64_t* d_lo, const uint64_t* d_epoch, const uint32_t* d_len, const uint64_t* d_items,
                  size_t items_stride, size_t n, hipStream_t st, const char* who) {
    if (n == 0) return SRN_OK;
    if (n > (1ull << 30)) return fail(SRN_ERANGE, std::string(who) + ": more than 2^30 entries in one call");
    // scratch: the longest length's word, the sorted front of the entries' keys (no consent, no times), the heads' slots and the runs' winners
    const VisitorBatch keys{d_hi, d_lo, nullptr, nullptr, nullptr, n, 0};
    Bump b; SortedFront front;
    const auto word_at = b.of<uint32_t>(1);
    int rc = front.plan(b, keys, st); if (rc) return rc;
    const auto slot_of = b.of<uint32_t>(n), win = b.of<uint32_t>(n);
    if ((rc = grow_behind(s->last, &s->xs, &s->xs_bytes, b.bytes))) return rc;
    char* const xs = s->xs;
    uint32_t* const word = word_at.at(xs);
    const uint32_t n32 = (uint32_t)n; const dim3 gn = grid_for(n);
    HIP_TRY(hipStreamWaitEvent(st, s->last, 0));
    HIP_TRY(hipMemsetAsync(word, 0, 4, st));
    sess_import_maxlen<<<gn, kTPB, 0, st>>>(d_len, n32, word);
    HIP_TRY(hipGetLastError());
    uint32_t longest = 0;
    HIP_TRY(hipMemcpyAsync(&longest, word, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (longest > s->items_cap) return fail(SRN_ERANGE, std::string(who) + ": a session is longer than the store's items_cap");
    if (longest > items_stride) return fail(SRN_ERANGE, std::string(who) + ": a session is longer than items_stride");
    // every entry counts as a new key; an import reclaims nothing (now = 1: no entry is older than the TTL), so a refused import leaves every slot where it was
    if ((rc = room_for(s, n, 1))) return rc;
    HIP_TRY(hipSetDevice(s->device));
    if ((rc = front.run(xs, keys, st))) return rc;
    ImportArgs a{};
    a.t = s->tab(); a.key_hi = d_hi; a.key_lo = d_lo; a.epoch = d_epoch; a.len = d_len; a.items = d_items; a.items_stride = items_stride;
    a.order = front.order; a.n = n32; a.slot_of = slot_of.at(xs); a.win = win.at(xs); a.err = s->err();
    sess_import_find<<<gn, kTPB, 0, st>>>(a);
    sess_import_write<<<grid_for(n * 16), kTPB, 0, st>>>(a);
    HIP_TRY(hipGetLastError());
    s->bound += n;
    s->len_bound = std::max<uint32_t>(s->len_bound, longest);
    (void)hipEventRecord(s->last, st);
    HIP_TRY(hipStreamSynchronize(st));
    return SRN_OK;
}

// ---- the file form: a 96-byte little-endian header, then the arrays of the export ----
constexpr char kSnapMagic[8] = {'S', 'R', 'N', 'S', 'E', 'S', 'S', '\0'};
constexpr uint32_t kSnapVersion = 1, kSnapHeader = 96;
struct SnapHeader {
    char magic[8]; uint32_t version, header_bytes;
    uint64_t n, longest, items_stride, capacity, items_cap, ttl, idle, saved_at, payload_bytes, checksum;
};
static_assert(sizeof(SnapHeader) == kSnapHeader, "snapshot header");
struct SnapOffsets { uint64_t hi, lo, ep, len, items, bytes; };
// false: the sizes overflow
bool snap_offsets(uint64_t n, uint64_t stride, SnapOffsets* o) {
    if (n > (1ull << 30) || stride > SRN_MAX_SESSION_LEN) return false;
    o->hi = 0; o->lo = n * 8; o->ep = n * 16; o->len = n * 24; o->items = n * 24 + (n * 4 + 7) / 8 * 8; o->bytes = o->items + n * stride * 8;
    return true;
}
// sum over the payload's 8-byte words w[i] of mix64(w[i] + (i + 1) * 0x9E3779B97F4A7C15), mod 2^64
uint64_t snap_checksum(const char* p, uint64_t bytes) {
    uint64_t sum = 0;
    for (uint64_t i = 0; i < bytes / 8; ++i) { uint64_t w; std::memcpy(&w, p + i * 8, 8); sum += mix64(w + (i + 1) * 0x9E3779B97F4A7C15ull); }
    return sum;
}
// reads and verifies the whole file: anything that is not a complete, consistent snapshot is SRN_EIO, and no offset is used before it has been checked against the size
int snap_read(const char* path, std::vector<char>* buf, SnapHeader* h, SnapOffsets* o) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(SRN_EIO, std::string("cannot open ") + path);
    struct Close { FILE* f; ~Close() { std::fclose(f); } } closer{f};
    if (std::fread(h, 1, kSnapHeader, f) != kSnapHeader) return fail(SRN_EIO, std::string(path) + ": shorter than a session snapshot's header");
    if (std::memcmp(h->magic, kSnapMagic, 8) != 0) return fail(SRN_EIO, std::string(path) + ": not a session snapshot (magic)");
    if (h->version != kSnapVersion) return fail(SRN_EIO, std::string(path) + ": unknown session snapshot version");
    if (h->header_bytes != kSnapHeader || !snap_offsets(h->n, h->items_stride, o) || o->bytes != h->payload_bytes || h->longest > h->items_stride)
        return fail(SRN_EIO, std::string(path) + ": the header's sizes do not add up");
    if (std::fseek(f, 0, SEEK_END) != 0) return fail(SRN_EIO, std::string(path) + ": cannot seek");
    const long size = std::ftell(f);
    if (size < 0 || (uint64_t)size != kSnapHeader + h->payload_bytes) return fail(SRN_EIO, std::string(path) + ": the file's size is not what its header says");
    buf->resize(h->payload_bytes);
    if (std::fseek(f, kSnapHeader, SEEK_SET) != 0 || (h->payload_bytes && std::fread(buf->data(), 1, h->payload_bytes, f) != h->payload_bytes))
        return fail(SRN_EIO, std::string(path) + ": short read");
    if (snap_checksum(buf->data(), h->payload_bytes) != h->checksum) return fail(SRN_EIO, std::string(path) + ": checksum mismatch");
    uint64_t longest = 0;
    for (uint64_t i = 0; i < h->n; ++i) { uint32_t l; std::memcpy(&l, buf->data() + o->len + i * 4, 4); longest = std::max<uint64_t>(longest, l); }
    if (longest != h->longest) return fail(SRN_EIO, std::string(path) + ": a session's length disagrees with the header's longest session");
    return SRN_OK;
}
}  // namespace

int dsess_count(srn_device_sessions* s, uint64_t now_secs, uint64_t* occupied, uint64_t* live) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_count: null store");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    int rc = own_after_last(s); if (rc) return rc;
    uint64_t o = 0, l = 0;
    if ((rc = count(s, now, &o, &l))) return rc;
    if (occupied) *occupied = o;
    if (live) *live = l;
    return SRN_OK;
}

int dsess_export_device(srn_device_sessions* s, uint64_t now_secs, size_t cap, uint64_t* d_hi, uint64_t* d_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items,
                        size_t items_stride, uint64_t* d_n, void* stream) {
    if (!s || !d_n || (cap && (!d_hi || !d_lo || !d_epoch || !d_len || (items_stride && !d_items)))) return fail(SRN_EINVAL, "srn_device_sessions_export_device: null argument");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    hipStream_t st = (hipStream_t)stream;
    std::lock_guard<std::mutex> g(s->mu);
    if (items_stride < s->len_bound) return fail(SRN_ERANGE, "srn_device_sessions_export_device: items_stride below the longest session the store may hold");
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipStreamWaitEvent(st, s->last, 0));
    const int rc = export_enqueue(s, now, cap, d_hi, d_lo, d_epoch, d_len, d_items, items_stride, d_n, st);
    (void)hipEventRecord(s->last, st);
    return rc;
}

int dsess_export_host(srn_device_sessions* s, uint64_t now_secs, size_t cap, uint64_t* hi, uint64_t* lo, uint64_t* epoch, uint32_t* len, uint64_t* items,
                      size_t items_stride, size_t* n) {
    if (!s || !n || (cap && (!hi || !lo || !epoch || !len || (items_stride && !items)))) return fail(SRN_EINVAL, "srn_device_sessions_export: null argument");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    int rc = own_after_last(s); if (rc) return rc;
    return export_host_locked(s, now, cap, hi, lo, epoch, len, items, items_stride, n, false, "srn_device_sessions_export");
}

int dsess_import_device(srn_device_sessions* s, const uint64_t* d_hi, const uint64_t* d_lo, const uint64_t* d_epoch, const uint32_t* d_len, const uint64_t* d_items,
                        size_t items_stride, size_t n, void* stream) {
    if (!s || (n && (!d_hi || !d_lo || !d_epoch || !d_len || (items_stride && !d_items)))) return fail(SRN_EINVAL, "srn_device_sessions_import_device: null argument");
    std::lock_guard<std::mutex> g(s->mu);
    HIP_TRY(hipSetDevice(s->device));
    return import_locked(s, d_hi, d_lo, d_epoch, d_len, d_items, items_stride, n, (hipStream_t)stream, "srn_device_sessions_import_device");
}

int dsess_import_host(srn_device_sessions* s, const uint64_t* hi, const uint64_t* lo, const uint64_t* epoch, const uint32_t* len, const uint64_t* items,
                      size_t items_stride, size_t n) {
    const char* who = "srn_device_sessions_import";
    if (!s || (n && (!hi || !lo || !epoch || !len || (items_stride && !items)))) return fail(SRN_EINVAL, std::string(who) + ": null argument");
    if (n == 0) return SRN_OK;
    if (n > (1ull << 30)) return fail(SRN_ERANGE, std::string(who) + ": more than 2^30 entries in one call");
    if (items_stride > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, std::string(who) + ": items_stride above SRN_MAX_SESSION_LEN");
    std::lock_guard<std::mutex> g(s->mu);
    int rc = own_after_last(s); if (rc) return rc;
    const Dense d(n, items_stride);
    StageBuf b; if ((rc = b.alloc(d.bytes, who))) return rc;
    hipError_t e = hipMemcpyAsync(d.hi.at(b.p), hi, n * 8, hipMemcpyHostToDevice, s->own);
    if (e == hipSuccess) e = hipMemcpyAsync(d.lo.at(b.p), lo, n * 8, hipMemcpyHostToDevice, s->own);
    if (e == hipSuccess) e = hipMemcpyAsync(d.ep.at(b.p), epoch, n * 8, hipMemcpyHostToDevice, s->own);
    if (e == hipSuccess) e = hipMemcpyAsync(d.len.at(b.p), len, n * 4, hipMemcpyHostToDevice, s->own);
    if (e == hipSuccess && items_stride) e = hipMemcpyAsync(d.items.at(b.p), items, n * items_stride * 8, hipMemcpyHostToDevice, s->own);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s->own); return fail(SRN_EHIP, std::string(who) + ": " + hipGetErrorString(e)); }
    rc = import_locked(s, d.hi.at(b.p), d.lo.at(b.p), d.ep.at(b.p), d.len.at(b.p), d.items.at(b.p), items_stride, n, s->own, who);
    (void)hipStreamSynchronize(s->own);
    return rc;
}

int dsess_resize(srn_device_sessions* s, size_t capacity, size_t items_cap, uint64_t now_secs) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_resize: null store");
    if (capacity == 0) return fail(SRN_EINVAL, "srn_device_sessions_resize: capacity must be > 0");
    if (capacity > (1ull << 30)) return fail(SRN_ERANGE, "srn_device_sessions_resize: capacity above 2^30 sessions");
    if (items_cap > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "srn_device_sessions_resize: items_cap above SRN_MAX_SESSION_LEN");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(s->mu);
    int rc = own_after_last(s); if (rc) return rc;
    return resize_locked(s, capacity, items_cap ? items_cap : s->items_cap, now, "srn_device_sessions_resize");
}

int dsess_set_max_capacity(srn_device_sessions* s, size_t max_capacity) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_set_max_capacity: null store");
    if (max_capacity > (1ull << 30)) return fail(SRN_ERANGE, "srn_device_sessions_set_max_capacity: above 2^30 sessions");
    std::lock_guard<std::mutex> g(s->mu);
    s->max_capacity = max_capacity;
    return SRN_OK;
}

int dsess_growth(srn_device_sessions* s, uint64_t* max_capacity, uint64_t* grows, uint64_t* resizes) {
    if (!s) return fail(SRN_EINVAL, "srn_device_sessions_growth: null store");
    std::lock_guard<std::mutex> g(s->mu);
    if (max_capacity) *max_capacity = s->max_capacity;
    if (grows) *grows = s->grows;
    if (resizes) *resizes = s->resizes;
    return SRN_OK;
}

int dsess_file_info(const char* path, srn_device_sessions_file_info_t* out) {
    if (!path || !out) return fail(SRN_EINVAL, "srn_device_sessions_file_info: null argument");
    std::vector<char> buf; SnapHeader h; SnapOffsets o;
    const int rc = snap_read(path, &buf, &h, &o); if (rc) return rc;
    *out = srn_device_sessions_file_info_t{h.version, h.n, h.longest, h.items_stride, h.capacity, h.items_cap, h.ttl, h.idle, h.saved_at, h.payload_bytes};
    return SRN_OK;
}

int dsess_save(srn_device_sessions* s, const char* path, uint64_t now_secs) {
    if (!s || !path) return fail(SRN_EINVAL, "srn_device_sessions_save: null argument");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    SnapHeader h{}; SnapOffsets o{}; std::vector<char> buf;
    {
        std::lock_guard<std::mutex> g(s->mu);
        int rc = own_after_last(s); if (rc) return rc;
        uint64_t occupied = 0, live = 0, longest = 0;
        if ((rc = count_max(s, now, &occupied, &live, &longest))) return rc;
        std::memcpy(h.magic, kSnapMagic, 8);
        h.version = kSnapVersion; h.header_bytes = kSnapHeader; h.n = live; h.longest = longest; h.items_stride = longest;
        h.capacity = s->capacity; h.items_cap = s->items_cap; h.ttl = s->ttl; h.idle = s->idle; h.saved_at = now;
        if (!snap_offsets(h.n, h.items_stride, &o)) return fail(SRN_ERANGE, "srn_device_sessions_save: the store is too large for the file form");
        buf.assign(o.bytes, 0);
        size_t n = 0;
        char* p = buf.data();
        rc = export_host_locked(s, now, live, (uint64_t*)(p + o.hi), (uint64_t*)(p + o.lo), (uint64_t*)(p + o.ep), (uint32_t*)(p + o.len), (uint64_t*)(p + o.items),
                                h.items_stride, &n, true, "srn_device_sessions_save");
        if (rc) return rc;
    }
    h.payload_bytes = o.bytes; h.checksum = snap_checksum(buf.data(), o.bytes);
    // a temporary name in the same directory, then a rename: a crash leaves the previous snapshot
    const std::string tmp = std::string(path) + ".tmp." + std::to_string((unsigned long long)::getpid());
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(SRN_EIO, "srn_device_sessions_save: cannot create " + tmp);
    bool ok = std::fwrite(&h, 1, kSnapHeader, f) == kSnapHeader && (o.bytes == 0 || std::fwrite(buf.data(), 1, o.bytes, f) == o.bytes);
    ok = ok && std::fflush(f) == 0 && ::fsync(::fileno(f)) == 0;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok || std::rename(tmp.c_str(), path) != 0) { std::remove(tmp.c_str()); return fail(SRN_EIO, std::string("srn_device_sessions_save: cannot write ") + path); }
    return SRN_OK;
}

int dsess_load(const char* path, int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions** out) {
    if (!path || !out) return fail(SRN_EINVAL, "srn_device_sessions_load: null argument");
    *out = nullptr;
    std::vector<char> buf; SnapHeader h; SnapOffsets o;
    int rc = snap_read(path, &buf, &h, &o); if (rc) return rc;
    const uint64_t cap = capacity ? capacity : std::max<uint64_t>(std::max<uint64_t>(h.capacity, h.n), 1), ic = items_cap ? items_cap : h.items_cap;
    if (h.n > cap) return fail(SRN_ENOMEM, "srn_device_sessions_load: the snapshot holds more sessions than the capacity");
    if (h.longest > ic) return fail(SRN_ERANGE, "srn_device_sessions_load: the snapshot's longest session exceeds items_cap");
    srn_device_sessions* s = nullptr;
    if ((rc = dsess_create(device, cap, ic, ttl_secs ? ttl_secs : h.ttl, idle_secs ? idle_secs : h.idle, &s))) return rc;
    const char* p = buf.data();
    rc = dsess_import_host(s, (const uint64_t*)(p + o.hi), (const uint64_t*)(p + o.lo), (const uint64_t*)(p + o.ep), (const uint32_t*)(p + o.len), (const uint64_t*)(p + o.items),
                           h.items_stride, h.n);
    if (rc) { dsess_free(s); return rc; }
    *out = s;
    return SRN_OK;
}

}  // namespace srn
