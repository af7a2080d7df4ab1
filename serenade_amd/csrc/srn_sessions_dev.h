// The device session store's table and handle (srn_sessions_dev.hip), shared with the code that reads the table beside it (srn_trending.hip, srn_harvest.hip).
// Layout and rules: the head comment of srn_sessions_dev.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <mutex>

namespace srn {

constexpr uint32_t kSlotHead = 32;             // bytes before the items
constexpr uint32_t kEmpty = 0, kFull = 1, kClaimed = 2;

struct SlotHead { uint64_t key_hi, key_lo, epoch; uint32_t len, state; };
static_assert(sizeof(SlotHead) == kSlotHead, "slot header");

struct Table { char* base; uint32_t mask, stride; };
__device__ __forceinline__ SlotHead* slot_at(const Table& t, uint32_t s) { return (SlotHead*)(t.base + (size_t)s * t.stride); }
__device__ __forceinline__ uint64_t* slot_items(SlotHead* h) { return (uint64_t*)((char*)h + kSlotHead); }
__host__ __device__ __forceinline__ bool idle_or_old(uint64_t now, uint64_t epoch, uint64_t limit) { return now > epoch && now - epoch > limit; }

// the session harvest's device words (srn_harvest.hip) and the two halves of an append flag
enum : uint32_t { kHvCursor = 0, kHvLost, kHvShort, kHvReturn, kHvRebuild, kHvCleared, kHvItems, kHvWords = 8 };
constexpr uint64_t kHvStore = 1, kHvSkip = 1ull << 32;

inline uint64_t wall_secs() { return (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::system_clock::now().time_since_epoch()).count(); }

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

struct srn_device_sessions {
    int device = 0;
    uint64_t capacity = 0, n_slots = 0, items_cap = 0, ttl = 0, idle = 0;
    uint32_t stride = 0;
    char* table[2] = {nullptr, nullptr}; int cur = 0;      // a sweep rebuilds into the other one
    std::mutex mu;                                          // covers the enqueue of a call and everything below
    hipEvent_t last = nullptr;                              // end of the most recent call, whatever stream it ran on
    hipStream_t own = nullptr;                              // get / update / sweep and the host-pointer entry point
    uint64_t bound = 0, sweeps = 0, refused = 0;            // bound: upper bound of the occupied slots
    uint32_t len_bound = 1;                                 // upper bound of the stored session lengths (predict's max_len_hint)
    uint32_t history = 0;                                   // srn_device_sessions_set_history: the window the store keeps (0: max_items_in_session, as the reference)
    char* ws = nullptr; size_t ws_bytes = 0;                // per-batch scratch, grows with the largest n seen
    char* stage = nullptr; size_t stage_bytes = 0;          // the host-pointer entry point's device copies
    std::mutex stage_mu;
    char* small = nullptr;                                  // err word | counters | one session in / out
    char* xs = nullptr; size_t xs_bytes = 0;                // export / import scratch (flags and places per slot; sort buffers per entry)
    char* hs = nullptr; size_t hs_bytes = 0;                // an attached harvest's append scratch for rebuilds (flags and places per slot)
    srn_harvest* harvest = nullptr;                         // srn_device_sessions_set_harvest: receives what the store forgets (null: nothing does)
    uint64_t max_capacity = 0, grows = 0, resizes = 0;      // opt-in growth (0 = off) | automatic resizes | all resizes
    // the most recent batch (debug accessors, timing)
    const uint64_t* last_items = nullptr; const uint32_t* last_qoff = nullptr; size_t last_n = 0, last_hint = 0;
    bool timing = false, last_timed = false; hipEvent_t tev[3] = {nullptr, nullptr, nullptr};
    srn::Table tab() const { return srn::Table{table[cur], (uint32_t)(n_slots - 1), stride}; }
    uint32_t* err() const { return (uint32_t*)small; }
    unsigned long long* counters() const { return (unsigned long long*)(small + 64); }
    uint64_t* one() const { return (uint64_t*)(small + 128); }
};
