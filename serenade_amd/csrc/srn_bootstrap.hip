// Session-clustered Poisson bootstrap of a trial's per-query terms (include/serenade_hip.h srn_evaluate_bootstrap), behind eval_metrics_kernel
// on the trial's chunk buffer.  Replicate b weighs every query of test session s with w(seed, b, s) (srn_bootstrap.h) and keeps seven sums: the weights, then the
// weighted mrr, ndcg, hit_rate, popularity, precision, recall.  The summation order is part of the contract: within a group of 256 global query indices (the groups
// of eval_group_kernel) from +0.0 in query order, acc = acc + (double)w * term -- product rounded, then the sum -- and the groups in order onto the running total.
//   boot_group_kernel        one workgroup per (group, 256 replicates): the group's terms and session indices staged in LDS once, every lane -- one replicate --
//                            walks the 256 queries in order (all lanes read the same LDS address: a broadcast).  No cross-lane arithmetic, so the order is the rule's.
//   boot_accumulate_kernel   one thread per (sum, replicate): the chunk's groups in order onto the call's totals.
// Replicates go in tiles of kBootTile: the partials of one tile, [group][sum][replicate], are all the scratch there is -- (chunk / 256) * min(B, 1024) * 7 doubles.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_bootstrap.h"

// the replicate sums must be the bits the NumPy model gives: no fused multiply-adds
#pragma clang fp contract(off)

namespace srn {

static constexpr uint32_t kGroup = 256;       // queries per partial sum (srn_eval.hip kGroup)
static constexpr uint32_t kTerms = 8;         // doubles per query in the chunk's term buffer (srn_eval.hip kTerms)
static constexpr uint32_t kBootTerms = 6;     // of which resampled: mrr, ndcg, hit_rate, popularity, precision, recall
static constexpr uint32_t kBootTile = 1024;   // replicates per pass over a chunk
static_assert(SRN_BOOTSTRAP_SUMS == kBootTerms + 1, "seven sums per replicate: the weights and six terms");

__global__ void __launch_bounds__(kGroup) boot_group_kernel(const double* __restrict__ terms, const uint2* __restrict__ ss, uint32_t nq, uint64_t seed,
                                                            uint32_t b0, uint32_t nb, double* __restrict__ scratch) {
    __shared__ double t_s[kGroup * kBootTerms];
    __shared__ uint32_t s_s[kGroup];
    const uint32_t tid = threadIdx.x, q0 = blockIdx.x * kGroup, n = min(kGroup, nq - q0);
    // the term buffer's columns (mrr, hit, ndcg, intersection, precision, recall, popularity, -) -> the sums' order; 15: not resampled
    for (uint32_t r = 0; r < kTerms; ++r) {
        const uint32_t i = r * kGroup + tid, q = i / kTerms, slot = (0xF354F120u >> (4u * (i % kTerms))) & 15u;
        if (q < n && slot < kBootTerms) t_s[q * kBootTerms + slot] = terms[(size_t)q0 * kTerms + i];
    }
    if (tid < n) s_s[tid] = ss[q0 + tid].x;
    __syncthreads();
    const uint32_t bl = blockIdx.y * kGroup + tid;   // the replicate within the tile
    if (bl >= nb) return;
    const uint64_t key = boot_replicate_key(seed, b0 + bl);
    double acc[SRN_BOOTSTRAP_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t prev = 0xFFFFFFFFu;   // (no session has this index: srn_eval_set_create refuses that many)
    double w = 0.0;
    for (uint32_t q = 0; q < n; ++q) {
        const uint32_t s = __builtin_amdgcn_readfirstlane(s_s[q]);   // every lane is at the same query: the branch is wave-uniform
        if (s != prev) { w = (double)boot_weight(key, s); prev = s; }
        const double* t = t_s + q * kBootTerms;
        acc[0] = acc[0] + w;
#pragma unroll
        for (uint32_t j = 0; j < kBootTerms; ++j) acc[1 + j] = acc[1 + j] + w * t[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < SRN_BOOTSTRAP_SUMS; ++j) scratch[((size_t)blockIdx.x * SRN_BOOTSTRAP_SUMS + j) * nb + bl] = acc[j];
}

__global__ void __launch_bounds__(256) boot_accumulate_kernel(const double* __restrict__ scratch, uint32_t n_groups, uint32_t nb, double* __restrict__ totals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * SRN_BOOTSTRAP_SUMS) return;
    const uint32_t j = i / nb, bl = i % nb;
    double* out = totals + (size_t)bl * SRN_BOOTSTRAP_SUMS + j;
    double tot = *out;
    const double* p = scratch + (size_t)j * nb + bl;
#pragma unroll 8
    for (uint32_t g = 0; g < n_groups; ++g) tot = tot + p[(size_t)g * SRN_BOOTSTRAP_SUMS * nb];
    *out = tot;
}

size_t boot_scratch_bytes(uint64_t chunk_queries, uint32_t replicates) {
    return (size_t)((chunk_queries + kGroup - 1) / kGroup) * std::min(replicates, kBootTile) * SRN_BOOTSTRAP_SUMS * sizeof(double);
}

int boot_chunk(const double* terms, const void* session_state, uint32_t nq, const srn_bootstrap_t& boot, double* scratch, double* totals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_groups = (nq + kGroup - 1) / kGroup;
    for (uint32_t b0 = 0; b0 < boot.replicates; b0 += kBootTile) {
        const uint32_t nb = std::min(kBootTile, boot.replicates - b0);
        boot_group_kernel<<<dim3(n_groups, (nb + kGroup - 1) / kGroup), kGroup, 0, st>>>(terms, (const uint2*)session_state, nq, boot.seed, b0, nb, scratch);
        HIP_TRY(hipGetLastError());
        boot_accumulate_kernel<<<(nb * SRN_BOOTSTRAP_SUMS + 255) / 256, 256, 0, st>>>(scratch, n_groups, nb, totals + (size_t)b0 * SRN_BOOTSTRAP_SUMS);
        HIP_TRY(hipGetLastError());
    }
    return SRN_OK;
}

void boot_weights_host(uint64_t seed, uint32_t replicate, uint64_t first_session, size_t n, uint8_t* out) {
    const uint64_t key = boot_replicate_key(seed, replicate);
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)boot_weight(key, first_session + i);
}

}  // namespace srn
