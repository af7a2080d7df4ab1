// =====================================================================================
// The LIGHT form: a query with ONE posting run of at most 64 kept entries -- a first click on a tail item -- served by one WAVE, outside the lean
// kernel's 512-thread, 53 KB, thirteen-barrier machine.  The prep kernel admits it (RW_LIGHT in the launch-ready block) and gives it the order key 0xFFFE, so the
// light representatives are one segment of the serving order, in front of the merged queries; the lean kernel's loop ends in front of that segment.
//
// Why the row is the lean form's, byte for byte: one list of kept <= 64 <= k, m entries -- every entry is a neighbour, all with the weight of a one-run set,
// w = (9 - ps) * (L - ps) (the lean form's w10t) -- so an item's sum is w * (rows that hold it), an integer; x = idf_eff * (double)sum and score = x / (10 U) are
// finish_inline's expressions, the ranking is its (score desc, id rank asc).  A row of more than 64 scored items is cut the way the latency path's fused launch cuts
// its big rows (wave_nth_top32 / wave_keep_top); what neither fits goes to the general kernel through slow_list.
//
// Per wave and query: the record's first 32 words in one load | lane l < kept: post_rank[base + l] = the row | the row's 64-byte slot, four 16-byte loads in flight | the
// items into the wave's own exact table in LDS (item_insert, weight 1; longer rows gather row_ext) | the table compacted in place, the current item dropped | finish.
// No workgroup barrier in the loop: the four waves of a workgroup never meet.
// =====================================================================================
#include <hip/hip_runtime.h>

#include "srn_device.h"
#include "srn_kernels.h"

namespace srn {

namespace {
constexpr uint32_t LT_BUCKETS = 251, LT_SLOTS = LT_BUCKETS * 4u, LT_ROUNDS = (LT_SLOTS + 63u) / 64u;   // the exact table: 1 004 slots (sampled maximum of distinct items: 533)
constexpr uint32_t LT_WAVES = 4, LT_PAD = LT_ROUNDS * 64u;                                            // waves per workgroup; table words rounded up to whole rounds
struct alignas(16) LightWave { uint32_t keys[LT_PAD]; int acc[LT_PAD]; uint32_t cidx[64]; uint32_t csum[64]; };
static_assert(sizeof(LightWave) * LT_WAVES <= 40u * 1024u, "four workgroups of the light form per CU");
}  // namespace

__global__ __launch_bounds__(64 * LT_WAVES) void vmis_light_kernel(DeviceIndex ix, LaunchParams p, const unsigned long long* __restrict__ order, const uint32_t* __restrict__ cnt_light,
                                                                  const uint32_t* __restrict__ cnt_end, uint32_t* slow_list, uint32_t* slow_cnt, uint32_t* host_word) {
    __shared__ LightWave lds[LT_WAVES];
    const uint32_t ln = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned long long ltl = (1ull << ln) - 1ull;
    LightWave& T = lds[wv];
    const uint32_t n_light = *cnt_light, seg0 = p.nq - *cnt_end;   // the segment of the order: [nq - merged - light, nq - merged)
    if (host_word && blockIdx.x == 0u && threadIdx.x == 0u) *host_word = n_light;   // (srn_debug_last_light_count)
    const bool business = (p.flags & SRN_FLAG_BUSINESS_LOGIC) != 0u;   // (launch-uniform)
    const uint32_t gw = blockIdx.x * LT_WAVES + wv, n_waves = gridDim.x * LT_WAVES;
    if (gw >= n_light) return;   // (an empty segment: every wave leaves at once)
#pragma unroll
    for (uint32_t t = 0; t < LT_ROUNDS; ++t) { T.keys[t * 64u + ln] = EMPTY32; T.acc[t * 64u + ln] = 0; }
    // ---- the record: PrepHead words 0..31 in one load (U = 0, L = 6, cur_attr = 16, the launch-ready block from word 18).  The NEXT query's order entry is requested at
    // the top of a query and its record behind the row requests: two of a query's dependent round trips are hidden behind the previous query's work
    constexpr uint32_t RW0 = (uint32_t)offsetof(PrepHead, ready) / 4u;
    static_assert(RW0 + RW_BASE + 2u <= 32u, "the first run's descriptor lies in the record's first 32 words");
    auto record = [&](uint32_t qq) -> uint32_t { return reinterpret_cast<const uint32_t*>(p.prep + (size_t)qq * p.prep_stride)[ln & 31u]; };
    uint32_t q_next = (uint32_t)order[seg0 + gw];
    uint32_t rw_next = record(q_next);
    for (uint32_t li = gw; li < n_light; li += n_waves) {
        const uint32_t q = q_next, rwv = rw_next;
        const bool more = li + n_waves < n_light;   // (wave-uniform)
        if (more) q_next = (uint32_t)order[seg0 + li + n_waves];
        auto word = [&](uint32_t w) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)rwv, (int)w); };
        const uint32_t U = word(0), L = word(6), cur_attr = word(16), cur = word(RW0 + RW_CUR), ps = word(RW0 + RW_PS) & 0xFFu, kept = min(word(RW0 + RW_KEPT), 64u);
        const unsigned long long base = ((unsigned long long)word(RW0 + RW_BASE + 1u) << 32) | word(RW0 + RW_BASE);
        const uint32_t wgt = (9u - ps) * (L - ps);
        // ---- the list, the rows
        const bool mine = ln < kept;
        const size_t row = mine ? (size_t)ix.post_rank[base + ln] : (size_t)ix.n_kept;   // (idle lanes: the empty slot behind the last row)
        const RowQuad a = ix.row_slots[4 * row], b = ix.row_slots[4 * row + 1], c = ix.row_slots[4 * row + 2], d = ix.row_slots[4 * row + 3];
        if (more) rw_next = record(q_next);
        const uint32_t len = mine ? a.x : 0u;
        const bool big = len > 15u;   // word 1 = where items 14.. start in row_ext, items 0..13 in words 2..15
        const uint32_t it15[15] = {big ? EMPTY32 : a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
        const uint32_t inl = big ? 14u : len;   // items in the slot: words 1.. (short rows) or 2.. (long rows; it15[0] is masked)
        bool ovf = false;
#pragma unroll
        for (uint32_t j = 0; j < 15u; ++j) {
            const uint32_t it = it15[j];
            if ((big ? j >= 1u && j - 1u < inl : j < inl) && it != EMPTY32 && item_insert(T.keys, T.acc, LT_BUCKETS, it, 1) < 0) ovf = true;
        }
        const uint32_t ext_max = wave_max(big ? len - 14u : 0u);
        for (uint32_t j0 = 0; j0 < ext_max; j0 += 8u) {   // the longer rows' items 14..: eight gathers in flight
            uint32_t e[8];
#pragma unroll
            for (uint32_t u = 0; u < 8u; ++u) e[u] = big && 14u + j0 + u < len ? ix.row_ext[a.y + j0 + u] : EMPTY32;
#pragma unroll
            for (uint32_t u = 0; u < 8u; ++u) if (e[u] != EMPTY32 && item_insert(T.keys, T.acc, LT_BUCKETS, e[u], 1) < 0) ovf = true;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- the table, compacted in place (the write index never passes the read index: a round is read into registers before it is written) and cleared behind
        uint32_t M = 0;   // (wave-uniform) scored items
#pragma unroll
        for (uint32_t t = 0; t < LT_ROUNDS; ++t) {
            const uint32_t i = t * 64u + ln;
            const uint32_t key = T.keys[i]; const int acc = T.acc[i];
            bool keep = key != EMPTY32 && key != cur;
            if (business && keep) keep = business_ok(cur_attr, ix.meta[key].attr);
            const unsigned long long bm = __ballot(keep);
            __builtin_amdgcn_wave_barrier();
            T.keys[i] = EMPTY32; T.acc[i] = 0;
            __builtin_amdgcn_wave_barrier();
            if (keep) { const uint32_t at = M + (uint32_t)__popcll(bm & ltl); T.keys[at] = key; T.acc[at] = acc; }
            M += (uint32_t)__popcll(bm);
            __builtin_amdgcn_wave_barrier();
        }
        bool hand_on = __ballot(ovf) != 0ull;   // (a full table: the general kernel serves the query)
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        uint32_t S = M;
        if (!hand_on && M <= 64u) {
            if (ln < M) e = make_uint4((uint32_t)T.acc[ln] * wgt, 0u, T.keys[ln], 1u);
        } else if (!hand_on) {
            // more than 64 scored items: the keys' top halves, the n-th largest of them, what is down to one step below it
            uint32_t hk[LT_ROUNDS];
#pragma unroll
            for (uint32_t h = 0; h < LT_ROUNDS; h += 8u) {
                uint32_t id8[8]; ItemMeta mm[8];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) { const uint32_t i = (h + u) * 64u + ln; id8[u] = h + u < LT_ROUNDS && i < M ? T.keys[i] : 0u; }
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) mm[u] = ix.meta[id8[u]];   // (all gathers of the half in flight together)
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) {
                    if (h + u >= LT_ROUNDS) continue;
                    const uint32_t i = (h + u) * 64u + ln;
                    const double x = (mm[u].idf > 0.0 ? mm[u].idf : 1.0) * (double)(i < M ? (uint32_t)T.acc[i] * wgt : 0u);
                    hk[h + u] = i < M ? (uint32_t)((unsigned long long)__double_as_longlong(x) >> 32) : 0u;
                }
            }
            S = wave_keep_top(hk, M, wave_nth_top32(hk, p.how_many), ln, ltl, [&](uint32_t at, uint32_t i) { T.cidx[at] = T.keys[i]; T.csum[at] = (uint32_t)T.acc[i] * wgt; });
            __builtin_amdgcn_wave_barrier();
            if (S <= 64u && S >= p.how_many) { if (ln < S) e = make_uint4(T.csum[ln], 0u, T.cidx[ln], 1u); }
            else hand_on = true;
        }
        __builtin_amdgcn_wave_barrier();
        // (the compacted entries sit in the table's first M words: back to empty for the next query)
#pragma unroll
        for (uint32_t t = 0; t < LT_ROUNDS; ++t) if (t * 64u < M) { T.keys[t * 64u + ln] = EMPTY32; T.acc[t * 64u + ln] = 0; }
        if (hand_on) { if (ln == 0u) slow_list[atomicAdd(&slow_cnt[SC_GENERAL], 1u)] = q; continue; }
        finish_inline(ix, S, U, e, ln, q, p.out_ids, p.out_scores, p.out_counts, p.how_many);   // the row and its count: no finish kernel acts on it
    }
}

// A fixed grid (the segment's length is known on the device only): four waves per workgroup, up to four workgroups per CU, a few queries per wave at the headline's ~45 000
hipError_t launch_light(hipStream_t st, uint32_t grid, const DeviceIndex& di, const LaunchParams& p, const unsigned long long* order, const uint32_t* cnt_light, const uint32_t* cnt_end,
                        uint32_t* slow_list, uint32_t* slow_cnt, uint32_t* host_word) {
    hipLaunchKernelGGL(vmis_light_kernel, dim3(grid), dim3(64 * LT_WAVES), 0, st, di, p, order, cnt_light, cnt_end, slow_list, slow_cnt, host_word);
    return hipGetLastError();
}

}  // namespace srn
