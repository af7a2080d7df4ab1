// Click-log rows on the device: what the loader (srn_ingest.hip), the splitter (srn_split.hip) and the evaluation set built from events (srn_eval.hip) share.
//   round_time / event_time   the loader's rounding of a time field, and a row's rounded seconds straight from the caller's f64 or i64 column
//   DevBuf                    a device allocation that frees itself
//   DevSessions / DevFlat     grouped sessions and a built index's arrays while they are still on the device: the seams of srn_index_from_events_device
//   KeyTable                  open addressing on full 64-bit keys: a key's slot index is its dense handle for the rest of a call
//   CombTable                 a block's LDS table that combines equal slots before a count reaches global memory
// Include after srn_hipsync.h (DevBuf frees).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "srn_internal.h"
#include "srn_hipsync.h"

namespace srn {

struct DevBuf {   // RAII device allocation
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { if (p) { (void)hipFree(p); p = nullptr; } return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
    void* release() { void* q = p; p = nullptr; return q; }
    template <typename T> T* as() const { return (T*)p; }
};

// `!(t >= 0)` -> 0, then llround (half away from zero) as u64.  t - trunc(t) is exact for t >= 0.
__host__ __device__ inline uint64_t round_time(double t) {
    if (!(t >= 0)) t = 0;
    if (t >= 9223372036854775808.0) return 0x8000000000000000ull;   // llround's out-of-range value (inputs out of scope: the TSV path hands these to the host)
    double r = trunc(t);
    if (t - r >= 0.5) r += 1.0;
    return (uint64_t)r;
}
// row j's rounded seconds: f64 through round_time, int64 seconds with negative -> 0
__host__ __device__ inline uint64_t event_time(const void* times, bool i64, uint64_t j) {
    if (i64) { const int64_t v = ((const int64_t*)times)[j]; return v < 0 ? 0 : (uint64_t)v; }
    return round_time(((const double*)times)[j]);
}

// SRN_EVENTS_DEVICE arrays must be device memory of `device` (a host pointer, or memory of another GPU, would fault in the first kernel)
inline int check_device_rows(const void* p, int device, const char* what) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return fail(SRN_EINVAL, std::string(what) + " is not device memory"); }
    if (a.type != hipMemoryTypeDevice) return fail(SRN_EINVAL, std::string(what) + " is not device memory");
    if (a.device != device) return fail(SRN_EINVAL, std::string(what) + " is on device " + std::to_string(a.device) + ", not on device " + std::to_string(device));
    return SRN_OK;
}

// rows of a TSV file, parsed on the device (srn_ingest.hip): three device arrays in file order, times rounded; host-parsed lines patched in, skipped lines compacted away
struct TsvRows { DevBuf s, i, t; uint64_t n = 0; };
int tsv_rows_device(const char* path, int device, hipStream_t st, TsvRows& out, srn_load_info_t& li);

// grouped training sessions on the device (group_rows_device_core, srn_ingest.hip): what Sessions holds on the host, before any download
struct DevSessions { DevBuf off, items, ts, session_ids; uint64_t n_sessions = 0, nnz = 0; };
int group_rows_device_core(const uint64_t* sess, const uint64_t* item, const uint64_t* time, size_t n, hipStream_t st, DevSessions& out, srn_load_info_t* info);
// srn_sessions_from_events up to the grouping, nothing downloaded (arguments already checked by the C ABI glue)
int device_sessions_from_events(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, int device, void* stream,
                                DevSessions& out, srn_load_info_t* info);
// sessions_length_quantile_counting on device offsets: a histogram kernel over the lengths 0..4095 (+ a count and a maximum of the longer ones), finished on the host;
// an order statistic in the overflow bin downloads the offsets and counts there
int device_length_quantile(const uint64_t* d_off, uint64_t n_sessions, double q, hipStream_t st, uint64_t* out);

// ---- the index builder's device side (srn_build_gpu.hip) ------------------------------------------
// what build_flat_index_core leaves on the device: the four large arrays of a FlatIndex and its per-item arrays (counts by dense idx feed the idf)
struct DevFlat { DevBuf post_rank, row_off, row_items, rank_to_session, item_id, id_rank, count, post_off; };
// device session arrays -> DevFlat + the scalars of ix (n_kept, nnz_*, n_items, max_row_len ...); nothing but scalars comes back
int build_flat_index_core(const uint64_t* d_off, const uint64_t* d_items, const uint32_t* d_ts, uint64_t n_sessions, uint64_t nnz_in, size_t m_index, size_t max_session_len,
                          double idf_weighting, FlatIndex& ix, DevFlat& out);
// the per-item arrays to the host, then idf (the host's std::log), default attributes and the id table
int build_flat_index_items(const DevFlat& dev, FlatIndex& ix);

// ---- open addressing on the full key -----------------------------------------------------------
// keys[0 .. mask] start as kEmptyKey (memset 0xFF); slot mask + 1 belongs to the key that IS kEmptyKey.  A slot goes from empty to its key once and never changes, so a
// plain look before the compare-and-swap is safe: a stale "empty" only costs the swap.  Keys are compared in full; hash_bits (tests: SRN_SPLIT_HASH_BITS; 0 = all) cuts the
// hash so that unequal keys share probe chains.  Returns the slot, or kNone when the table is full (callers size it at twice the keys, so: never) -- the probe is bounded.
static constexpr uint64_t kEmptyKey = ~0ull;
struct KeyTable { unsigned long long* keys; uint32_t mask; uint32_t hash_bits; };
inline uint32_t key_table_slots(uint64_t n_keys) { uint64_t s = 64; while (s < 2 * n_keys && s < (1ull << 31)) s <<= 1; return (uint32_t)s; }   // (+ 1 for kEmptyKey's own)
__device__ inline uint32_t key_table_home(const KeyTable& t, uint64_t key) {
    uint64_t x = key;   // srn_internal.h mix64
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    uint32_t h = (uint32_t)x;
    if (t.hash_bits && t.hash_bits < 32) h &= (1u << t.hash_bits) - 1u;
    return h & t.mask;
}
// *fresh = this call put the key there
__device__ inline uint32_t key_table_insert(const KeyTable& t, uint64_t key, bool* fresh) {
    *fresh = false;
    if (key == kEmptyKey) {
        if (__hip_atomic_load(&t.keys[t.mask + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return t.mask + 1;   // (its slot holds 0 = seen, any other value = not yet)
        *fresh = atomicExch(&t.keys[t.mask + 1], 0ull) != 0;
        return t.mask + 1;
    }
    uint32_t h = key_table_home(t, key);
    for (uint64_t probe = 0; probe <= t.mask; ++probe, h = (h + 1) & t.mask) {
        unsigned long long cur = __hip_atomic_load(&t.keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmptyKey) { cur = atomicCAS(&t.keys[h], (unsigned long long)kEmptyKey, (unsigned long long)key); if (cur == kEmptyKey) { *fresh = true; return h; } }
        if (cur == key) return h;
    }
    return kNone;
}

// ---- counting into slots when the key column is Zipf ---------------------------------------------
// The most popular item of a large log draws several hundred thousand adds to one address.  A block first combines equal slots in a small LDS table -- one LDS
// compare-and-swap and one LDS add per row, no probing: a row whose entry holds another slot adds straight to global memory -- and then adds each entry once.
// comb_flush is called by the whole block (it synchronises before and after).
static constexpr uint32_t kCombSlots = 1024;         // 8 KiB of LDS
static constexpr uint32_t kCombEmpty = 0xFFFFFFFFu;  // (kNone: never a slot)
static constexpr uint32_t kCombTile = 4096;          // rows per block between two flushes
struct CombTable { uint32_t key[kCombSlots], cnt[kCombSlots]; };
__device__ inline void comb_init(CombTable& c) {
    for (uint32_t e = threadIdx.x; e < kCombSlots; e += blockDim.x) { c.key[e] = kCombEmpty; c.cnt[e] = 0; }
    __syncthreads();
}
__device__ inline void comb_add(CombTable& c, uint32_t* counts, uint32_t slot) {
    const uint32_t h = (slot * 2654435761u) >> 22;   // 10 bits
    const uint32_t old = atomicCAS(&c.key[h], kCombEmpty, slot);
    if (old == kCombEmpty || old == slot) atomicAdd(&c.cnt[h], 1u);
    else atomicAdd(&counts[slot], 1u);
}
__device__ inline void comb_flush(CombTable& c, uint32_t* counts) {
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < kCombSlots; e += blockDim.x)
        if (c.key[e] != kCombEmpty) { atomicAdd(&counts[c.key[e]], c.cnt[e]); c.key[e] = kCombEmpty; c.cnt[e] = 0; }
    __syncthreads();
}

}  // namespace srn
