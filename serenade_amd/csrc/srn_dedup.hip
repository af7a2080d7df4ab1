// =====================================================================================
// Queries of ONE call with the same item sequence have the same output row (predict_next is a pure function of the index, the call's parameters and the sequence --
// DESIGN.md 4.6): the launch sequence serves the smallest query index of every such group and copies its row to the others.  Nothing outlives the call.
//
//   vmis_dedup_group_kernel    one thread per query: a hash table over the batch (u32 slots holding a query index, >= 2 per query, cleared to EMPTY32 by the runtime);
//                              hash of (length, the raw 64-bit ids in order), linear probing, an empty slot is claimed with atomicCAS, an occupied one is COMPARED -- the
//                              full sequences, read from the call's read-only input -- and only an equal one ends the probe: a group is the queries that ended on one slot.
//                              The slot's second word takes the atomicMin of their indices.
//   vmis_dedup_resolve_kernel  rep[q] = that minimum (rep[q] == q: a representative).  A merged query's order key becomes 0xFFFF << 32 | q -- the radix sort behind this
//                              kernel puts it behind every representative, whose keys are clamped to 0xFFFE -- and the merged queries are counted.  Where the launch
//                              sequence has the light form on (srn_light.hip) the prep kernel has clamped the keys to 0xFFFD and given 0xFFFE to the light queries:
//                              the kernel also counts the light REPRESENTATIVES and merged + light, the end of the lean kernel's loop.
//   vmis_dedup_mark_kernel     out_counts[q] = 0 for the merged queries, on the stream the serving kernels run on: the finish kernels act on every row of [0, nq) whose
//                              count word is 0x80000000 / 0x80000001, and a merged row's word is whatever the caller's buffer held.  (Where grouping runs on that stream
//                              itself the resolve kernel writes the word.)
//   vmis_dedup_fill_kernel     last of the launch sequence: the representative's count and the ids and scores inside it, to every merged query.
// =====================================================================================
#include <hip/hip_runtime.h>

#include "srn_device.h"
#include "srn_kernels.h"

namespace srn {

namespace {
__device__ __forceinline__ bool same_sequence(const uint64_t* __restrict__ items_flat, const uint32_t* __restrict__ q_off, uint32_t qb, uint32_t L, uint32_t other) {
    const uint32_t ob = q_off[other];
    if (q_off[other + 1] - ob != L) return false;
    for (uint32_t i = 0; i < L; ++i) if (items_flat[qb + i] != items_flat[ob + i]) return false;
    return true;
}
}  // namespace

__global__ __launch_bounds__(256) void vmis_dedup_group_kernel(const uint64_t* __restrict__ items_flat, const uint32_t* __restrict__ q_off, uint32_t nq, uint32_t* slots, uint32_t* slot_min,
                                                               uint32_t slot_mask, uint32_t hash_mask, uint32_t* slot_of, uint32_t* n_dup, uint32_t* light_cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q == 0u) { *n_dup = 0u; if (light_cnt) { light_cnt[0] = 0u; light_cnt[1] = 0u; } }   // (counted by the resolve kernel, behind this one on the stream)
    if (q >= nq) return;
    const uint32_t qb = q_off[q], L = q_off[q + 1] - qb;
    uint64_t h = dev_mix64(0x9E3779B97F4A7C15ull + L);
    for (uint32_t i = 0; i < L; ++i) h = dev_mix64(h ^ items_flat[qb + i]) + 0x9E3779B97F4A7C15ull;   // (chained: the order of the items counts)
    uint32_t s = ((uint32_t)(h >> 32) & hash_mask) & slot_mask;
    // Slots only ever go from empty to taken, and the table has more slots than the batch has queries: the probe ends.  Two equal sequences end on the same slot -- the
    // later one finds every slot the earlier one passed still taken by something unequal, and then the earlier one's claim (or claims that very slot first).
    for (;;) {
        uint32_t c = __atomic_load_n(&slots[s], __ATOMIC_RELAXED);
        if (c == EMPTY32) { c = atomicCAS(&slots[s], EMPTY32, q); if (c == EMPTY32) c = q; }
        if (c == q || same_sequence(items_flat, q_off, qb, L, c)) break;
        s = (s + 1u) & slot_mask;
    }
    slot_of[q] = s;
    if (q < __atomic_load_n(&slot_min[s], __ATOMIC_RELAXED)) atomicMin(&slot_min[s], q);   // (the look first: a popular sequence's thousands of copies would queue on one word)
}

__global__ __launch_bounds__(256) void vmis_dedup_resolve_kernel(uint32_t nq, const uint32_t* __restrict__ slot_min, uint32_t* rep, unsigned long long* __restrict__ okeys,
                                                                 uint32_t* __restrict__ out_counts, uint32_t* n_dup, uint32_t* light_cnt) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    bool dup = false, light = false;
    if (q < nq) {
        const uint32_t r = slot_min[rep[q]];   // (rep[q] holds the query's slot until here)
        rep[q] = r; dup = r != q;
        if (dup) { okeys[q] = (0xFFFFull << 32) | q; if (out_counts) out_counts[q] = 0u; }
        else {
            const uint32_t key = (uint32_t)(okeys[q] >> 32);
            if (key >= 0xFFFFu) okeys[q] = (0xFFFEull << 32) | q;
            else light = light_cnt != nullptr && key == 0xFFFEu;   // (the light form is on: the prep kernel gave 0xFFFE to the light queries alone; a merged one is not served)
        }
    }
    const unsigned long long b = __ballot(dup);
    if (!light_cnt) { if (b != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(n_dup, (uint32_t)__popcll(b)); return; }
    // the light form is on: three counts -- merged | light representatives | merged + light, where the lean kernel's loop ends -- summed over the workgroup first (every
    // wave adding to three words of one line took the kernel from 0.19 to 0.37 ms per 2^20 queries); [0] and [1] are one 64-bit word
    __shared__ uint32_t part[2];
    if (threadIdx.x < 2u) part[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned long long bl = __ballot(light);
    if ((threadIdx.x & 63u) == 0u) { if (b) atomicAdd(&part[0], (uint32_t)__popcll(b)); if (bl) atomicAdd(&part[1], (uint32_t)__popcll(bl)); }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const uint32_t nd = part[0], nl = part[1];
        if (nd) atomicAdd(n_dup, nd);
        if (nd | nl) atomicAdd(reinterpret_cast<unsigned long long*>(light_cnt), ((unsigned long long)(nd + nl) << 32) | nl);
    }
}

__global__ __launch_bounds__(256) void vmis_dedup_mark_kernel(uint32_t nq, const uint32_t* __restrict__ rep, uint32_t* __restrict__ out_counts) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq && rep[q] != q) out_counts[q] = 0u;
}

static constexpr uint32_t FILL_LANES = 16;   // lanes per query: a row of 21 ids + 21 scores in two rounds
__global__ __launch_bounds__(256) void vmis_dedup_fill_kernel(uint32_t nq, const uint32_t* __restrict__ rep, uint64_t* out_ids, double* out_scores, uint32_t* out_counts, uint32_t how_many,
                                                              const uint32_t* __restrict__ n_dup, uint32_t* __restrict__ host_word) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0u && host_word) *host_word = *n_dup;   // (srn_debug_last_dedup_count)
    const uint64_t q = t / FILL_LANES; const uint32_t sub = (uint32_t)(t % FILL_LANES);
    if (q >= nq) return;
    const uint32_t r = rep[q];
    if (r == q) return;
    // (representatives are never written here, and every kernel that writes their rows is over: a representative left unserved -- 0xFFFFFFFF -- or empty copies as such)
    const uint32_t c = out_counts[r], n = c == 0xFFFFFFFFu ? 0u : min(c, how_many);
    const uint64_t* si = out_ids + (size_t)r * how_many; const double* ss = out_scores + (size_t)r * how_many;
    uint64_t* di = out_ids + (size_t)q * how_many; double* ds = out_scores + (size_t)q * how_many;
    for (uint32_t j = sub; j < n; j += FILL_LANES) { di[j] = si[j]; ds[j] = ss[j]; }
    if (sub == 0u) out_counts[q] = c;
}

// slots / slot_min: dedup_slots(nq) words each, cleared to EMPTY32 by the caller on `st`; rep: nq words; okeys: the prep kernel's keys (already written on `st`);
// out_counts: null where the serving kernels run on another stream (launch_dedup_mark there).  hash_bits: SRN_DEDUP_HASH_BITS (tests; 0 = all of them)
uint32_t dedup_slots(uint32_t nq) { uint32_t s = 1024u; while (s < 0x80000000u && (uint64_t)s < 2ull * nq) s <<= 1; return s; }
hipError_t launch_dedup_group(hipStream_t st, const uint64_t* items_flat, const uint32_t* q_off, uint32_t nq, uint32_t* slots, uint32_t* slot_min, uint32_t n_slots, uint32_t hash_bits,
                              uint32_t* rep, unsigned long long* okeys, uint32_t* out_counts, uint32_t* n_dup, uint32_t* light_cnt) {
    const uint32_t hash_mask = hash_bits >= 1u && hash_bits < 32u ? (1u << hash_bits) - 1u : 0xFFFFFFFFu;
    hipLaunchKernelGGL(vmis_dedup_group_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, items_flat, q_off, nq, slots, slot_min, n_slots - 1u, hash_mask, rep, n_dup, light_cnt);
    hipLaunchKernelGGL(vmis_dedup_resolve_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, nq, (const uint32_t*)slot_min, rep, okeys, out_counts, n_dup, light_cnt);
    return hipGetLastError();
}
hipError_t launch_dedup_mark(hipStream_t st, uint32_t nq, const uint32_t* rep, uint32_t* out_counts) {
    hipLaunchKernelGGL(vmis_dedup_mark_kernel, dim3((nq + 255u) / 256u), dim3(256), 0, st, nq, rep, out_counts);
    return hipGetLastError();
}
hipError_t launch_dedup_fill(hipStream_t st, uint32_t nq, const uint32_t* rep, uint64_t* out_ids, double* out_scores, uint32_t* out_counts, uint32_t how_many, const uint32_t* n_dup, uint32_t* host_word) {
    const uint64_t threads = (uint64_t)nq * FILL_LANES;
    hipLaunchKernelGGL(vmis_dedup_fill_kernel, dim3((uint32_t)((threads + 255u) / 256u)), dim3(256), 0, st, nq, rep, out_ids, out_scores, out_counts, how_many, n_dup, host_word);
    return hipGetLastError();
}

}  // namespace srn
