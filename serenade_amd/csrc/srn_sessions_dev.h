// The device session store's table and handle (srn_sessions_dev.hip), shared with the code that reads the table beside it (srn_trending.hip).
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

inline uint64_t wall_secs() { return (uint64_t)std::chrono::duration_cast<std::chrono::seconds>(std::chrono::system_clock::now().time_since_epoch()).count(); }

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
    uint64_t max_capacity = 0, grows = 0, resizes = 0;      // opt-in growth (0 = off) | automatic resizes | all resizes
    // the most recent batch (debug accessors, timing)
    const uint64_t* last_items = nullptr; const uint32_t* last_qoff = nullptr; size_t last_n = 0, last_hint = 0;
    bool timing = false, last_timed = false; hipEvent_t tev[3] = {nullptr, nullptr, nullptr};
    srn::Table tab() const { return srn::Table{table[cur], (uint32_t)(n_slots - 1), stride}; }
    uint32_t* err() const { return (uint32_t*)small; }
    unsigned long long* counters() const { return (unsigned long long*)(small + 64); }
    uint64_t* one() const { return (uint64_t*)(small + 128); }
};
