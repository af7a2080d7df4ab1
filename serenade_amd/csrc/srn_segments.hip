// Trials by segment (include/serenade_hip.h srn_evaluate_segments), behind eval_group_kernel -- and behind boot_chunk where there is a bootstrap -- on the
// trial's chunk buffer.  The order of the additions is 10.2's, restricted to a segment's queries: per group of 256 global query indices from +0.0 in query order,
// acc = acc + term (with a bootstrap acc = acc + (double)w * term, product rounded, then the sum), then the groups in order onto the segment's total.
//   seg_id_kernel              one thread per query: the id from (session, state), the set's items and, for the count modes, the dictionary probe of eval_metrics_kernel
//   seg_group_kernel           one workgroup per group: the group's terms and ids staged in LDS once; lane g of the first wave is segment g and walks the 256 queries in order (a broadcast
//                              read), adding the term where the id is its own and +0.0 elsewhere -- every term is >= +0.0, so that is the same bits.  No cross-lane arithmetic
//   seg_accumulate_kernel      one thread per (sum, segment): the chunk's groups in order onto [segment][7]
//   seg_boot_group_kernel      one workgroup per (group, 256 replicates, 8 segments): lane = replicate, its accumulators [segment][sum] a column of an LDS array
//                              [8][7][256] (112 KB).  All lanes are at the same query, so the row its segment selects is wave-uniform and the access contiguous in the
//                              replicate; a query of another tile is skipped.  One walk serves eight segments where boot_group_kernel per segment would take eight
//   seg_boot_accumulate_kernel one thread per (segment, sum, replicate): a pass's groups in order onto [segment][replicate][7]
// The bootstrap's partials go in passes of kSegBootPass groups, so its scratch is kSegBootPass * 8 * 7 * 256 doubles whatever the chunk, S and B.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_device.h"
#include "srn_visitor_table.h"  // align256
#include "srn_bootstrap.h"
#include "srn_segments.h"

// the sums must be the bits the NumPy model gives: no fused multiply-adds
#pragma clang fp contract(off)

namespace srn {

static constexpr uint32_t kGroup = 256;        // queries per partial sum (srn_eval.hip kGroup)
static constexpr uint32_t kTerms = 8;          // doubles per query in the chunk's term buffer (srn_eval.hip kTerms)
static constexpr uint32_t kSegTerms = 6;       // of which summed: mrr, ndcg, hit_rate, popularity, precision, recall
static constexpr uint32_t kSegTile = 8;        // segments per pass of the bootstrap kernel: 8 * 7 * 256 doubles of LDS
static constexpr uint32_t kSegBootPass = 512;  // groups per pass of the bootstrap kernel
static_assert(SRN_MAX_SEGMENTS <= 64, "lane g of one wave is segment g");
static_assert(kSegSums == kSegTerms + 1, "seven sums per segment: the queries (the weights) and six terms");
// the term buffer's columns (mrr, hit, ndcg, intersection, precision, recall, popularity, -) -> the sums' order; 15: not summed (srn_bootstrap.hip)
static constexpr uint32_t kTermSlots = 0xF354F120u;

struct SegIdArgs { SegSet set; SegRule rule; const uint2* ss; uint32_t nq; uint16_t* ids; };

__global__ void __launch_bounds__(256) seg_id_kernel(SegIdArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.nq) return;
    const uint2 st = a.ss[i];   // (session, state): the raw t under every serving rule
    uint32_t id = 0;
    if (a.rule.mode == SRN_SEG_STATE) id = min(st.y, a.rule.S) - 1u;
    else if (a.rule.mode == SRN_SEG_LABEL) id = a.rule.labels[st.x];
    else {
        // e_t = the session's event t - 1, e_{t+1} = event t (t <= n - 1: both exist)
        const uint64_t x = a.set.items[a.set.sess_off[st.x] + st.y - (a.rule.mode == SRN_SEG_CURRENT_COUNT ? 1u : 0u)];
        uint32_t h = (uint32_t)dev_mix64(x) & a.set.id_mask, dense = kNone;
        while (a.set.id_table) { const IdSlot sl = a.set.id_table[h]; if (sl.idx == kNone) break; if (sl.key == x) { dense = sl.idx; break; } h = (h + 1) & a.set.id_mask; }
        const uint64_t c = dense != kNone ? (uint64_t)a.set.freq[dense] : 0ull;   // (counts are integers below 2^32 held as doubles)
        for (uint32_t j = 0; j + 1 < a.rule.S; ++j) id += a.rule.bounds[j] <= c ? 1u : 0u;
    }
    a.ids[i] = (uint16_t)id;
}

// (four waves stage the group -- eight loads in flight per lane, as in boot_group_kernel -- and the first one walks it: S <= 64)
__global__ void __launch_bounds__(kGroup) seg_group_kernel(const double* __restrict__ terms, const uint16_t* __restrict__ ids, uint32_t nq, uint32_t S,
                                                           double* __restrict__ part) {
    __shared__ double t_s[kGroup * kSegTerms];
    __shared__ uint32_t id_s[kGroup];
    const uint32_t lane = threadIdx.x, q0 = blockIdx.x * kGroup, n = min(kGroup, nq - q0);
#pragma unroll
    for (uint32_t r = 0; r < kTerms; ++r) {
        const uint32_t i = r * kGroup + lane, q = i / kTerms, slot = (kTermSlots >> (4u * (i % kTerms))) & 15u;
        if (q < n && slot < kSegTerms) t_s[q * kSegTerms + slot] = terms[(size_t)q0 * kTerms + i];
    }
    if (lane < n) id_s[lane] = ids[q0 + lane];
    __syncthreads();
    if (lane >= S) return;
    double acc[kSegTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t cnt = 0;
#pragma unroll 4
    for (uint32_t q = 0; q < n; ++q) {
        const bool mine = id_s[q] == lane;
        const double* t = t_s + q * kSegTerms;
        cnt += mine ? 1u : 0u;
#pragma unroll
        for (uint32_t j = 0; j < kSegTerms; ++j) acc[j] = acc[j] + (mine ? t[j] : 0.0);
    }
    double* out = part + (size_t)blockIdx.x * kSegSums * S + lane;
    out[0] = (double)cnt;
#pragma unroll
    for (uint32_t j = 0; j < kSegTerms; ++j) out[(size_t)(1 + j) * S] = acc[j];
}

__global__ void __launch_bounds__(256) seg_accumulate_kernel(const double* __restrict__ part, uint32_t n_groups, uint32_t S, double* __restrict__ totals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * kSegSums) return;
    const uint32_t j = i / S, g = i % S;
    double* out = totals + (size_t)g * kSegSums + j;
    double tot = *out;
    const double* p = part + (size_t)j * S + g;
#pragma unroll 32
    for (uint32_t k = 0; k < n_groups; ++k) tot = tot + p[(size_t)k * kSegSums * S];   // (the loads do not wait for the sum: 32 in flight)
    *out = tot;
}

// groups g_first .. g_first + gridDim.x - 1 of the chunk, replicates b0 .. b0 + nb - 1 (nb <= 256), segments seg0 .. seg0 + ns - 1 (ns <= kSegTile)
__global__ void __launch_bounds__(kGroup) seg_boot_group_kernel(const double* __restrict__ terms, const uint2* __restrict__ ss, const uint16_t* __restrict__ ids, uint32_t nq,
                                                                uint32_t g_first, uint64_t seed, uint32_t b0, uint32_t nb, uint32_t seg0, uint32_t ns,
                                                                double* __restrict__ scratch) {
    __shared__ double acc_s[kSegTile * kSegSums * kGroup];
    __shared__ double t_s[kGroup * kSegTerms];
    __shared__ uint32_t s_s[kGroup];
    __shared__ uint32_t id_s[kGroup];
    const uint32_t tid = threadIdx.x, q0 = (g_first + blockIdx.x) * kGroup, n = min(kGroup, nq - q0);
    for (uint32_t r = 0; r < kTerms; ++r) {
        const uint32_t i = r * kGroup + tid, q = i / kTerms, slot = (kTermSlots >> (4u * (i % kTerms))) & 15u;
        if (q < n && slot < kSegTerms) t_s[q * kSegTerms + slot] = terms[(size_t)q0 * kTerms + i];
    }
    if (tid < n) { s_s[tid] = ss[q0 + tid].x; id_s[tid] = ids[q0 + tid]; }
    const uint32_t rows = ns * kSegSums;
    for (uint32_t r = 0; r < rows; ++r) acc_s[r * kGroup + tid] = 0.0;   // (a lane's own column: only the staged terms need the barrier)
    __syncthreads();
    if (tid >= nb) return;
    const uint64_t key = boot_replicate_key(seed, b0 + tid);
    uint32_t prev = 0xFFFFFFFFu;   // (no session has this index: srn_eval_set_create refuses that many)
    double w = 0.0;
    for (uint32_t q = 0; q < n; ++q) {
        const uint32_t g = __builtin_amdgcn_readfirstlane(id_s[q]) - seg0;   // every lane is at the same query: both branches are wave-uniform
        if (g >= ns) continue;
        const uint32_t s = __builtin_amdgcn_readfirstlane(s_s[q]);
        if (s != prev) { w = (double)boot_weight(key, s); prev = s; }
        const double* t = t_s + q * kSegTerms;
        double* a = acc_s + (size_t)g * kSegSums * kGroup + tid;
        a[0] = a[0] + w;
#pragma unroll
        for (uint32_t j = 0; j < kSegTerms; ++j) a[(1 + j) * kGroup] = a[(1 + j) * kGroup] + w * t[j];
    }
    for (uint32_t r = 0; r < rows; ++r) scratch[((size_t)blockIdx.x * rows + r) * nb + tid] = acc_s[r * kGroup + tid];
}

// totals: the trial's [S][B][7]
__global__ void __launch_bounds__(256) seg_boot_accumulate_kernel(const double* __restrict__ scratch, uint32_t n_groups, uint32_t b0, uint32_t nb, uint32_t B, uint32_t seg0,
                                                                  uint32_t ns, double* __restrict__ totals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, rows = ns * kSegSums;
    if (i >= rows * nb) return;
    const uint32_t r = i / nb, bl = i % nb, g = seg0 + r / kSegSums, j = r % kSegSums;
    double* out = totals + ((size_t)g * B + b0 + bl) * kSegSums + j;
    double tot = *out;
    const double* p = scratch + (size_t)r * nb + bl;
#pragma unroll 8
    for (uint32_t k = 0; k < n_groups; ++k) tot = tot + p[(size_t)k * rows * nb];   // (14 336 threads keep enough loads in flight: 32 per thread measured 5.6x slower)
    *out = tot;
}

SegBuffers seg_buffers(size_t n_sessions, uint64_t max_chunk, size_t n_trials, uint32_t S, uint32_t replicates) {
    SegBuffers b;
    const size_t groups = (size_t)((max_chunk + kGroup - 1) / kGroup);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(std::max<size_t>(bytes, 16)); return o; };
    b.labels = take(n_sessions * sizeof(uint16_t));
    b.ids = take((size_t)max_chunk * sizeof(uint16_t));
    b.totals = take(n_trials * S * kSegSums * sizeof(double));
    b.part = take(groups * kSegSums * S * sizeof(double));
    b.boot_totals = take(n_trials * S * (size_t)replicates * kSegSums * sizeof(double));
    b.boot_part = take(replicates ? std::min<size_t>(groups, kSegBootPass) * std::min(S, kSegTile) * kSegSums * std::min(replicates, kGroup) * sizeof(double) : 0);
    b.bytes = at;
    return b;
}

int seg_ids(const SegSet& set, const SegRule& rule, const void* ss, uint32_t nq, uint16_t* ids, void* stream) {
    if (nq == 0) return SRN_OK;
    SegIdArgs a{set, rule, (const uint2*)ss, nq, ids};
    seg_id_kernel<<<(nq + 255) / 256, 256, 0, (hipStream_t)stream>>>(a);
    HIP_TRY(hipGetLastError());
    return SRN_OK;
}

int seg_chunk(const double* terms, const uint16_t* ids, uint32_t nq, uint32_t S, double* part, double* totals, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_groups = (nq + kGroup - 1) / kGroup;
    if (n_groups == 0) return SRN_OK;
    seg_group_kernel<<<n_groups, kGroup, 0, st>>>(terms, ids, nq, S, part);
    HIP_TRY(hipGetLastError());
    seg_accumulate_kernel<<<(S * kSegSums + 255) / 256, 256, 0, st>>>(part, n_groups, S, totals);
    HIP_TRY(hipGetLastError());
    return SRN_OK;
}

int seg_boot_chunk(const double* terms, const void* ss, const uint16_t* ids, uint32_t nq, uint32_t S, const srn_bootstrap_t& boot, double* part, double* totals,
                   void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_groups = (nq + kGroup - 1) / kGroup, B = boot.replicates;
    for (uint32_t seg0 = 0; seg0 < S; seg0 += kSegTile) {
        const uint32_t ns = std::min(kSegTile, S - seg0);
        for (uint32_t b0 = 0; b0 < B; b0 += kGroup) {
            const uint32_t nb = std::min(kGroup, B - b0);
            for (uint32_t g0 = 0; g0 < n_groups; g0 += kSegBootPass) {   // passes in group order: the running total takes the groups in order
                const uint32_t ng = std::min(kSegBootPass, n_groups - g0);
                seg_boot_group_kernel<<<ng, kGroup, 0, st>>>(terms, (const uint2*)ss, ids, nq, g0, boot.seed, b0, nb, seg0, ns, part);
                HIP_TRY(hipGetLastError());
                seg_boot_accumulate_kernel<<<(ns * kSegSums * nb + 255) / 256, 256, 0, st>>>(part, ng, b0, nb, B, seg0, ns, totals);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return SRN_OK;
}

}  // namespace srn
