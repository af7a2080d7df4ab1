// The device session store's slot and handle (srn_sessions_dev.hip), shared with the code that reads the table beside it (srn_trending.hip, srn_harvest.hip).
// The table underneath is srn_visitor_table.h's; the store's layout and rules: the head comment of srn_sessions_dev.hip.  Also the staging layout of an export's dense arrays.
#pragma once
#include "srn_visitor_table.h"   // SlotHead, Table, the slot states, VisitorTable

namespace srn {

__device__ __forceinline__ uint64_t* slot_items(SlotHead* h) { return (uint64_t*)((char*)h + kSlotHead); }

// the session harvest's device words (srn_harvest.hip) and the two halves of an append flag
enum : uint32_t { kHvCursor = 0, kHvLost, kHvShort, kHvReturn, kHvRebuild, kHvCleared, kHvItems, kHvWords = 8 };
constexpr uint64_t kHvStore = 1, kHvSkip = 1ull << 32;

// the dense arrays of n entries in one staging buffer -- the export form of the store and of the harvest: key_hi | key_lo | epoch | len | items | a u64 word
struct Dense {
    Bump::Region<uint64_t> hi, lo, ep, items, word; Bump::Region<uint32_t> len; size_t bytes;
    Dense(size_t n, size_t items_stride) {
        Bump b;
        hi = b.of<uint64_t>(n); lo = b.of<uint64_t>(n); ep = b.of<uint64_t>(n); len = b.of<uint32_t>(n); items = b.of<uint64_t>(n * items_stride); word = b.of<uint64_t>(1);
        bytes = b.bytes;
    }
};

}  // namespace srn

struct srn_device_sessions;
// The session harvest (srn_harvest.hip): the log's arrays and words never move, so the store's hooks read them under the store's mutex alone
struct srn_harvest {
    int device = 0;
    uint64_t capacity = 0, items_cap = 0; uint32_t min_len = 1;
    uint64_t* key_hi = nullptr; uint64_t* key_lo = nullptr; uint64_t* epoch = nullptr; uint32_t* len = nullptr; uint64_t* items = nullptr;   // [capacity] ([capacity * items_cap])
    uint64_t* words = nullptr;                              // [kHvWords] cursor and counters
    uint64_t bound = 0;                                     // the host's upper bound of the cursor (+ the positions of every append; exact after a read-back): what export / events sort
    srn_device_sessions* store = nullptr;                   // the store it is attached to (set under both mutexes, the harvest's taken first)
    std::mutex mu;
    hipStream_t own = nullptr; hipEvent_t last = nullptr;   // a detached harvest's calls; attached, the store's pair orders them
    char* xs = nullptr; size_t xs_bytes = 0;                // sort and scan scratch of export / events
};

namespace srn {
// The append, for the store's hooks (store mutex held, `st` the stream of the call that forgets the sessions).  scratch: harvest_scratch_bytes(n) bytes, whose first
// (n + 1) u64 words are the flags -- kHvStore / kHvSkip / 0 per position, the last one 0.  slot_of: position -> slot (null: the position is the slot)
int harvest_scratch_bytes(size_t n, size_t* bytes);
int harvest_append(srn_harvest* h, const Table& t, const uint32_t* slot_of, size_t n, char* scratch, bool from_return, hipStream_t st);
// the sessions a timed batch ends inside the call, from the call's CSR: flagged sorted position p appends (key of request order[p], t[p - 1], the window of
// request order[p - 1]); counted in from_return.  scratch as for harvest_append, the flags by sorted position
int harvest_append_csr(srn_harvest* h, const uint32_t* order, const uint64_t* src_hi, const uint64_t* src_lo, const uint64_t* t, const uint64_t* items_flat,
                       const uint32_t* q_off, size_t n, char* scratch, hipStream_t st);
int harvest_dropped(srn_harvest* h, const Table& from, uint64_t now, uint64_t ttl, char* scratch, hipStream_t st);   // flags what a rebuild of `from` at `now` leaves out, then appends
}  // namespace srn

struct srn_device_sessions : srn::VisitorTable {            // get / update / sweep run on `own`
    uint64_t items_cap = 0;
    char* old = nullptr;                                    // the pair's other table: a sweep rebuilds into it and flips, so it holds the previous contents until the next one
    uint32_t len_bound = 1;                                 // upper bound of the stored session lengths (predict's max_len_hint)
    uint32_t history = 0;                                   // srn_device_sessions_set_history: the window the store keeps (0: max_items_in_session, as the reference)
    char* stage = nullptr; size_t stage_bytes = 0;          // the host-pointer entry point's device copies
    std::mutex stage_mu;
    char* xs = nullptr; size_t xs_bytes = 0;                // export / import scratch (flags and places per slot; sort buffers per entry)
    char* hs = nullptr; size_t hs_bytes = 0;                // an attached harvest's append scratch for rebuilds (flags and places per slot)
    srn_harvest* harvest = nullptr;                         // srn_device_sessions_set_harvest: receives what the store forgets (null: nothing does)
    uint64_t max_capacity = 0, grows = 0, resizes = 0;      // opt-in growth (0 = off) | automatic resizes | all resizes
    // the most recent batch (debug accessors, timing)
    const uint64_t* last_items = nullptr; const uint32_t* last_qoff = nullptr; size_t last_n = 0, last_hint = 0;
    bool timing = false, last_timed = false; hipEvent_t tev[3] = {nullptr, nullptr, nullptr};
};
