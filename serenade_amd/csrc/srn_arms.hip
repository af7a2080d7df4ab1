// Traffic split: one visitor batch served under several arms, sticky per visitor.  No predict kernel is touched: four kernels of integer work stand
// around the calls the library already has.
//   arm_assign    one lane per request: arm[i] by the rule (srn_arms.h), and per block the number of requests of each arm -- 64-bit ballots and popcounts per wave,
//                 a [SRN_MAX_ARMS][4] LDS table across the block's four waves, one store per (arm, block).  No atomics.
//   arm_offsets   one workgroup loops an exclusive scan over block_counts in (arm, block) order: every (arm, block)'s base, and arm_begin[A + 1]
//   arm_gather    rank among the block's earlier requests of the same arm = ballot prefix within the wave + the preceding waves' counts; perm[base + rank] = i and the
//                 request's columns to that position.  Every arm's requests are then contiguous and in request order: a visitor is in one arm, so the visitor's
//                 clicks reach the store and the log in the order they came
//   arm_scatter   the served rows, counts, ranks and arms back to request order, lanes along a row's entries
// Between gather and scatter the host reads arm_begin -- the call's one synchronisation: the arms' calls take their sizes from the host -- and enqueues, per
// non-empty arm, dsess_recommend_device and fb_observe_device on the arm's slice of the gathered columns and of the arm-ordered row buffers.
// Every buffer of the device form is allocated at create; calls on one handle take turns behind `mu`, and `last` orders a call's kernels behind the previous
// call's, whatever stream that ran on (the scratch is shared).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_visitor_table.h"   // wall_secs, grid_for, grow_behind
#include "srn_arms.h"
#include "srn_hipsync.h"   // last: wraps hipFree / hipHostFree / hipDeviceSynchronize

struct srn_traffic_split {
    int device = 0;
    uint32_t n_arms = 0, max_how_many = 0;
    uint64_t seed = 0, max_batch = 0;
    uint64_t thr[SRN_MAX_ARMS] = {};                        // T_a, a < n_arms (info's thresholds)
    uint64_t served[SRN_MAX_ARMS] = {}, calls = 0, shortcut_calls = 0;
    std::mutex mu;                                          // a call from its checks to its last enqueue; set_weights; info
    hipEvent_t last = nullptr;                              // end of the most recent call's use of the scratch
    char* scratch = nullptr; size_t scratch_bytes = 0;      // every region below, allocated at create (A = 1: none)
    srn::Bump::Region<uint8_t> arm, g_consent;
    srn::Bump::Region<uint32_t> perm, b_counts, b_rank, block_counts, block_base, arm_begin;
    srn::Bump::Region<uint64_t> g_hi, g_lo, g_item, g_time, b_ids, b_scores;
    uint32_t* begin_host = nullptr;                         // pinned: arm_begin[SRN_MAX_ARMS + 1]
    std::mutex stage_mu;                                    // the host-pointer form: its stream and its device copies (grow with the largest call)
    hipStream_t own = nullptr; char* stage = nullptr; size_t stage_bytes = 0;
    bool timing = false, last_timed = false; hipEvent_t tev[4] = {nullptr, nullptr, nullptr, nullptr};
};

namespace srn {
namespace {

constexpr uint32_t kArmTPB = 256, kArmWaves = kArmTPB / 64;
constexpr uint32_t kNoArm = 0xFFu;   // a lane behind the batch's end

struct AssignArgs { ArmRule rule; const uint64_t* key_hi; const uint64_t* key_lo; uint32_t n, n_arms, n_blocks; uint8_t* arm; uint32_t* block_counts; };

__global__ void __launch_bounds__(kArmTPB) arm_assign(AssignArgs a) {
    __shared__ uint32_t wave_cnt[SRN_MAX_ARMS][kArmWaves];
    const uint32_t i = blockIdx.x * kArmTPB + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t arm = kNoArm;
    if (i < a.n) { arm = arm_of(a.rule, a.key_hi[i], a.key_lo[i]); a.arm[i] = (uint8_t)arm; }
    for (uint32_t x = 0; x < a.n_arms; ++x) {
        const uint64_t mask = __ballot(arm == x);
        if (lane == 0) wave_cnt[x][wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x < a.n_arms) {
        uint32_t c = 0;
        for (uint32_t w = 0; w < kArmWaves; ++w) c += wave_cnt[threadIdx.x][w];
        a.block_counts[(size_t)threadIdx.x * a.n_blocks + blockIdx.x] = c;
    }
}

// one workgroup: base[e] = the sum of counts[0 .. e), e = arm * n_blocks + block, kArmTPB entries per round with the carry in a register; arm_begin[a] = base[a * n_blocks],
// arm_begin[n_arms] = the total (= n)
__global__ void __launch_bounds__(kArmTPB) arm_offsets(const uint32_t* __restrict__ counts, uint32_t total, uint32_t n_blocks, uint32_t n_arms, uint32_t* __restrict__ base,
                                                       uint32_t* __restrict__ arm_begin) {
    __shared__ uint32_t wave_sum[kArmWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t start = 0; start < total; start += kArmTPB) {
        const uint32_t e = start + threadIdx.x;
        const uint32_t v = e < total ? counts[e] : 0u;
        uint32_t inc = v;
        for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d); if (lane >= d) inc += t; }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < kArmWaves; ++w) { const uint32_t s = wave_sum[w]; before += w < wave ? s : 0u; all += s; }
        if (e < total) {
            const uint32_t excl = carry + before + inc - v;
            base[e] = excl;
            if (e % n_blocks == 0) arm_begin[e / n_blocks] = excl;
        }
        carry += all;
        __syncthreads();   // (wave_sum is written again in the next round)
    }
    if (threadIdx.x == 0) arm_begin[n_arms] = carry;
}

struct GatherArgs {
    const uint64_t* key_hi; const uint64_t* key_lo; const uint64_t* item; const uint64_t* times; const uint8_t* consent;   // times / consent null: not gathered
    const uint8_t* arm; const uint32_t* base; uint32_t n, n_arms, n_blocks;
    uint32_t* perm; uint64_t* g_hi; uint64_t* g_lo; uint64_t* g_item; uint64_t* g_time; uint8_t* g_consent;
};

__global__ void __launch_bounds__(kArmTPB) arm_gather(GatherArgs a) {
    __shared__ uint32_t wave_cnt[SRN_MAX_ARMS][kArmWaves];
    const uint32_t i = blockIdx.x * kArmTPB + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t arm = i < a.n ? a.arm[i] : kNoArm;
    uint32_t rank = 0;
    for (uint32_t x = 0; x < a.n_arms; ++x) {
        const uint64_t mask = __ballot(arm == x);
        if (lane == 0) wave_cnt[x][wave] = (uint32_t)__popcll(mask);
        if (arm == x) rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (i >= a.n || arm >= a.n_arms) return;
    for (uint32_t w = 0; w < wave; ++w) rank += wave_cnt[arm][w];
    const uint32_t pos = a.base[(size_t)arm * a.n_blocks + blockIdx.x] + rank;
    if (pos >= a.n) return;   // (cannot happen: the bases are the scan of this kernel's own counts)
    a.perm[pos] = i;
    a.g_hi[pos] = a.key_hi[i]; a.g_lo[pos] = a.key_lo[i]; a.g_item[pos] = a.item[i];
    if (a.times) a.g_time[pos] = a.times[i];
    if (a.consent) a.g_consent[pos] = a.consent[i];
}

// scores travel as their 64 bits (filled entries score -inf).  out_rank / out_arm null: not written
struct ScatterArgs {
    const uint32_t* perm; const uint8_t* arm; const uint64_t* b_ids; const uint64_t* b_scores; const uint32_t* b_counts; const uint32_t* b_rank;
    uint32_t n, how_many;
    uint64_t* out_ids; uint64_t* out_scores; uint32_t* out_counts; uint8_t* out_arm; uint32_t* out_rank;
};

__global__ void __launch_bounds__(kArmTPB) arm_scatter(ScatterArgs a) {
    const size_t e = (size_t)blockIdx.x * kArmTPB + threadIdx.x;
    if (e >= (size_t)a.n * a.how_many) return;
    const uint32_t p = (uint32_t)(e / a.how_many), j = (uint32_t)(e - (size_t)p * a.how_many);
    const uint32_t dst = a.perm[p], c = a.b_counts[p];
    if (dst >= a.n) return;
    if (j < (c <= a.how_many ? c : 0u)) {   // as the plain call: a row's entries beyond its count are not written (0xFFFFFFFF: not served)
        const size_t o = (size_t)dst * a.how_many + j;
        a.out_ids[o] = a.b_ids[e]; a.out_scores[o] = a.b_scores[e];
    }
    if (j == 0) {
        a.out_counts[dst] = c;
        if (a.out_rank) a.out_rank[dst] = a.b_rank[p];
        if (a.out_arm) a.out_arm[dst] = a.arm[dst];
    }
}

inline uint32_t blocks_of(size_t n) { return (uint32_t)((std::max<size_t>(n, 1) + kArmTPB - 1) / kArmTPB); }

// weights -> the handle's thresholds; the ABI's codes for n_arms and W
int thresholds_of(const uint32_t* weights, size_t n_arms, uint64_t* all, const char* who) {
    if (!weights) return fail(SRN_EINVAL, std::string(who) + ": null weights");
    if (n_arms < 1 || n_arms > SRN_MAX_ARMS) return fail(SRN_ERANGE, std::string(who) + ": n_arms outside 1 .. SRN_MAX_ARMS");
    int why = SRN_OK;
    if (!arm_thresholds(weights, n_arms, all, &why))
        return fail(why, std::string(who) + (why == SRN_EINVAL ? ": the weights sum to 0" : ": the weights sum to 2^32 or more"));
    return SRN_OK;
}

}  // namespace

int split_free(srn_traffic_split* sp) {
    if (!sp) return SRN_OK;
    (void)hipSetDevice(sp->device);
    if (sp->last) { (void)hipEventSynchronize(sp->last); (void)hipEventDestroy(sp->last); }
    if (sp->own) { (void)hipStreamSynchronize(sp->own); (void)hipStreamDestroy(sp->own); }
    for (hipEvent_t e : sp->tev) if (e) (void)hipEventDestroy(e);
    for (void* p : {(void*)sp->scratch, (void*)sp->stage}) if (p) (void)hipFree(p);
    if (sp->begin_host) (void)hipHostFree(sp->begin_host);
    delete sp;
    return SRN_OK;
}

int split_create(int device, const uint32_t* weights, size_t n_arms, uint64_t seed, size_t max_batch, size_t max_how_many, srn_traffic_split** out) {
    const char* who = "srn_traffic_split_create";
    if (!out) return fail(SRN_EINVAL, std::string(who) + ": null output");
    *out = nullptr;
    uint64_t thr[SRN_MAX_ARMS];
    int rc = thresholds_of(weights, n_arms, thr, who); if (rc) return rc;
    if (max_batch == 0 || max_how_many == 0) return fail(SRN_EINVAL, std::string(who) + ": max_batch and max_how_many must be > 0");
    if (max_batch > kMaxBatch) return fail(SRN_ERANGE, std::string(who) + ": max_batch above 2^24 requests");
    if (max_how_many > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, std::string(who) + ": max_how_many above SRN_MAX_HOW_MANY");
    int n_dev = 0;
    if (device < 0 || hipGetDeviceCount(&n_dev) != hipSuccess || device >= n_dev) return fail(SRN_ENODEV, std::string(who) + ": no such GPU");
    HIP_TRY(hipSetDevice(device));
    srn_traffic_split* sp = new srn_traffic_split();
    struct Guard { srn_traffic_split*& sp; ~Guard() { if (sp) split_free(sp); } } guard{sp};
    sp->device = device; sp->n_arms = (uint32_t)n_arms; sp->max_how_many = (uint32_t)max_how_many; sp->seed = seed; sp->max_batch = max_batch;
    std::memcpy(sp->thr, thr, sizeof(thr));
    HIP_TRY(hipEventCreateWithFlags(&sp->last, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&sp->own, hipStreamNonBlocking));
    for (hipEvent_t& e : sp->tev) HIP_TRY(hipEventCreate(&e));
    if (n_arms > 1) {
        const size_t n = max_batch, rows = n * max_how_many, cells = n_arms * (size_t)blocks_of(n);
        Bump b;
        sp->arm = b.of<uint8_t>(n); sp->perm = b.of<uint32_t>(n);
        sp->g_hi = b.of<uint64_t>(n); sp->g_lo = b.of<uint64_t>(n); sp->g_item = b.of<uint64_t>(n); sp->g_time = b.of<uint64_t>(n); sp->g_consent = b.of<uint8_t>(n);
        sp->b_ids = b.of<uint64_t>(rows); sp->b_scores = b.of<uint64_t>(rows); sp->b_counts = b.of<uint32_t>(n); sp->b_rank = b.of<uint32_t>(n);
        sp->block_counts = b.of<uint32_t>(cells); sp->block_base = b.of<uint32_t>(cells); sp->arm_begin = b.of<uint32_t>(SRN_MAX_ARMS + 1);
        if (hipMalloc((void**)&sp->scratch, b.bytes) != hipSuccess) { (void)hipGetLastError(); sp->scratch = nullptr; return fail(SRN_ENOMEM, std::string(who) + ": no device memory for the split's buffers"); }
        sp->scratch_bytes = b.bytes;
        HIP_TRY(hipHostMalloc((void**)&sp->begin_host, (SRN_MAX_ARMS + 1) * sizeof(uint32_t), hipHostMallocDefault));
    }
    *out = sp; sp = nullptr;
    return SRN_OK;
}

int split_info(const srn_traffic_split* csp, srn_traffic_split_info_t* out) {
    if (!csp || !out) return fail(SRN_EINVAL, "srn_traffic_split_info: null argument");
    srn_traffic_split* sp = const_cast<srn_traffic_split*>(csp);
    std::lock_guard<std::mutex> sg(sp->stage_mu);
    std::lock_guard<std::mutex> g(sp->mu);
    *out = srn_traffic_split_info_t{};
    out->n_arms = sp->n_arms; out->max_how_many = sp->max_how_many; out->seed = sp->seed; out->max_batch = sp->max_batch;
    out->device_bytes = sp->scratch_bytes + sp->stage_bytes;
    std::memcpy(out->thresholds, sp->thr, sizeof(sp->thr)); std::memcpy(out->served, sp->served, sizeof(sp->served));
    out->calls = sp->calls; out->shortcut_calls = sp->shortcut_calls;
    return SRN_OK;
}

int split_set_weights(srn_traffic_split* sp, const uint32_t* weights, size_t n_arms) {
    const char* who = "srn_traffic_split_set_weights";
    if (!sp) return fail(SRN_EINVAL, std::string(who) + ": null split");
    uint64_t thr[SRN_MAX_ARMS];
    const int rc = thresholds_of(weights, n_arms, thr, who); if (rc) return rc;
    std::lock_guard<std::mutex> g(sp->mu);
    if (n_arms != sp->n_arms) return fail(SRN_EINVAL, std::string(who) + ": the number of arms is the handle's for good");
    std::memcpy(sp->thr, thr, sizeof(thr));
    return SRN_OK;
}

int split_arms_host(uint64_t seed, const uint32_t* weights, size_t n_arms, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out) {
    const char* who = "srn_traffic_split_arms";
    uint64_t thr[SRN_MAX_ARMS];
    const int rc = thresholds_of(weights, n_arms, thr, who); if (rc) return rc;
    if (n && (!key_hi || !key_lo || !out)) return fail(SRN_EINVAL, std::string(who) + ": null argument");
    const ArmRule rule = arm_rule(seed, thr, n_arms);
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)arm_of(rule, key_hi[i], key_lo[i]);
    return SRN_OK;
}

int split_timing(srn_traffic_split* sp, int enable) {
    if (!sp) return fail(SRN_EINVAL, "srn_traffic_split_timing: null split");
    std::lock_guard<std::mutex> g(sp->mu);
    sp->timing = enable != 0;
    return SRN_OK;
}
int split_last_ms(srn_traffic_split* sp, double* ms_front, double* ms_scatter) {
    if (!sp) return fail(SRN_EINVAL, "srn_traffic_split_last_ms: null split");
    std::lock_guard<std::mutex> g(sp->mu);
    if (!sp->last_timed) return fail(SRN_EINVAL, "srn_traffic_split_last_ms: the last call was not timed (srn_traffic_split_timing) or took the one-arm shortcut");
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipEventSynchronize(sp->tev[3]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, sp->tev[0], sp->tev[1]));
    HIP_TRY(hipEventElapsedTime(&b, sp->tev[2], sp->tev[3]));
    if (ms_front) *ms_front = a;
    if (ms_scatter) *ms_scatter = b;
    return SRN_OK;
}

namespace {

// one arm's calls on the slice [begin, begin + n) of request columns and row buffers: the store's call, then the log's.  *log_rc: the log's refusal (SRN_ENOMEM),
// which does not fail the call; the slice's ranks are then SRN_FEEDBACK_NONE, as for an arm without a log
int serve_arm(const srn_arm_t& arm, srn_device_sessions* store, const VisitorBatch& r, size_t how_many, uint64_t* ids, double* scores, uint32_t* counts, uint32_t* rank,
              int* log_rc, hipStream_t st) {
    const RecommendCall c{arm.max_items_in_session, arm.k, arm.m, how_many, arm.flags, ids, scores, counts, st};
    int rc = dsess_recommend_device(arm.idx, store, r, c); if (rc) return rc;
    *log_rc = SRN_OK;
    bool ranked = false;
    if (arm.feedback) {
        rc = fb_observe_device(arm.feedback, r, ObserveCall{ids, scores, counts, how_many, rank, st});
        if (rc && rc != SRN_ENOMEM) return rc;
        *log_rc = rc; ranked = rc == SRN_OK;
    }
    if (rank && !ranked) HIP_TRY(hipMemsetAsync(rank, 0xFF, r.n * sizeof(uint32_t), st));   // SRN_FEEDBACK_NONE
    return SRN_OK;
}

}  // namespace

// every check of a call that needs neither the store's mutex nor the device (mu held); *nothing: n = 0
static int check_call(srn_traffic_split* sp, const srn_arm_t* arms, size_t n_arms, const srn_device_sessions* store, const VisitorBatch& r, size_t how_many,
                      const SplitOut& o, int (*check_arm)(const srn_arm_t&, size_t), bool* nothing) {
    const std::string who = "srn_recommend_batch_split: ";
    *nothing = false;
    if (n_arms != sp->n_arms) return fail(SRN_EINVAL, who + "n_arms is not the handle's");
    for (size_t a = 0; a < n_arms; ++a) {
        const int rc = check_arm(arms[a], how_many); if (rc) return rc;
        if (arms[a].idx->device != sp->device) return fail(SRN_EINVAL, who + "an arm's index is on another device than the split");
        if (!arms[a].feedback) continue;
        for (size_t b = 0; b < a; ++b) if (arms[b].feedback == arms[a].feedback) return fail(SRN_EINVAL, who + "one feedback log in two arms");
        int log_device = 0; uint64_t row_cap = 0;
        fb_shape(arms[a].feedback, &log_device, &row_cap);
        if (log_device != sp->device) return fail(SRN_EINVAL, who + "an arm's feedback log is on another device than the split");
        if (how_many > row_cap) return fail(SRN_ERANGE, who + "how_many above a feedback log's row_cap");
    }
    if (r.n == 0) { *nothing = true; return SRN_OK; }
    if (!has_request_arrays(r, false) || !o.ids || !o.scores || !o.counts) return fail(SRN_EINVAL, who + "null buffer");
    if (!store) return fail(SRN_EINVAL, who + "a split serves against a session store");
    if (r.n > sp->max_batch) return fail(SRN_ERANGE, who + "more requests than the handle's max_batch");
    if (how_many > sp->max_how_many) return fail(SRN_ERANGE, who + "how_many above the handle's max_how_many");
    return SRN_OK;
}
static int check_handles(const srn_traffic_split* sp, const srn_arm_t* arms, size_t n_arms) {
    if (!sp || !arms) return fail(SRN_EINVAL, "srn_recommend_batch_split: null split or arms");
    if (n_arms < 1 || n_arms > SRN_MAX_ARMS) return fail(SRN_ERANGE, "srn_recommend_batch_split: n_arms outside 1 .. SRN_MAX_ARMS");
    return SRN_OK;
}

int split_recommend_device(srn_traffic_split* sp, const srn_arm_t* arms, size_t n_arms, srn_device_sessions* store, const VisitorBatch& r, size_t how_many,
                           const SplitOut& o, void* stream, int (*check_arm)(const srn_arm_t&, size_t)) {
    const std::string who = "srn_recommend_batch_split: ";
    int rc = check_handles(sp, arms, n_arms); if (rc) return rc;
    std::lock_guard<std::mutex> g(sp->mu);
    bool nothing;
    if ((rc = check_call(sp, arms, n_arms, store, r, how_many, o, check_arm, &nothing))) return rc;
    if (o.feedback_rc) std::fill(o.feedback_rc, o.feedback_rc + n_arms, SRN_OK);
    if (nothing) return SRN_OK;
    const size_t n = r.n;
    hipStream_t st = (hipStream_t)stream;
    VisitorBatch all = r;
    all.now_secs = r.now_secs ? r.now_secs : wall_secs();   // the clock, once: every arm's call and every log receive this value
    int log_rc = SRN_OK;
    if (n_arms == 1) {   // the plain call on the caller's buffers
        HIP_TRY(hipSetDevice(sp->device));
        if ((rc = serve_arm(arms[0], store, all, how_many, o.ids, o.scores, o.counts, o.rank, &log_rc, st))) return rc;
        if (o.arm) HIP_TRY(hipMemsetAsync(o.arm, 0, n, st));
        if (o.feedback_rc) o.feedback_rc[0] = log_rc;
        sp->served[0] += n; ++sp->shortcut_calls; sp->last_timed = false;
        return SRN_OK;
    }
    const srn_index* idx[SRN_MAX_ARMS]; RecommendCall calls[SRN_MAX_ARMS];
    for (size_t a = 0; a < n_arms; ++a) {
        idx[a] = arms[a].idx;
        calls[a] = RecommendCall{arms[a].max_items_in_session, arms[a].k, arms[a].m, how_many, arms[a].flags, nullptr, nullptr, nullptr, nullptr};
    }
    if ((rc = dsess_admit(store, idx, calls, n_arms, n, all.now_secs))) return rc;
    // from here on things are enqueued
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipStreamWaitEvent(st, sp->last, 0));
    char* const ws = sp->scratch;
    const uint32_t n32 = (uint32_t)n, A = (uint32_t)n_arms, n_blocks = blocks_of(n);
    const bool timed = sp->timing;
    if (timed) HIP_TRY(hipEventRecord(sp->tev[0], st));
    AssignArgs aa{arm_rule(sp->seed, sp->thr, n_arms), r.key_hi, r.key_lo, n32, A, n_blocks, sp->arm.at(ws), sp->block_counts.at(ws)};
    arm_assign<<<n_blocks, kArmTPB, 0, st>>>(aa);
    arm_offsets<<<1, kArmTPB, 0, st>>>(sp->block_counts.at(ws), A * n_blocks, n_blocks, A, sp->block_base.at(ws), sp->arm_begin.at(ws));
    GatherArgs ga{r.key_hi, r.key_lo, r.item, r.times, r.consent, sp->arm.at(ws), sp->block_base.at(ws), n32, A, n_blocks,
                  sp->perm.at(ws), sp->g_hi.at(ws), sp->g_lo.at(ws), sp->g_item.at(ws), sp->g_time.at(ws), sp->g_consent.at(ws)};
    arm_gather<<<n_blocks, kArmTPB, 0, st>>>(ga);
    HIP_TRY(hipGetLastError());
    if (timed) HIP_TRY(hipEventRecord(sp->tev[1], st));
    HIP_TRY(hipMemcpyAsync(sp->begin_host, sp->arm_begin.at(ws), (A + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the call's one synchronisation: the arms' calls take n from the host
    uint32_t begin[SRN_MAX_ARMS + 1];
    std::memcpy(begin, sp->begin_host, (A + 1) * sizeof(uint32_t));
    if (begin[0] != 0 || begin[A] != n32 || !std::is_sorted(begin, begin + A + 1)) return fail(SRN_ESTATE, who + "the arms' offsets do not add up to the batch");
    uint64_t* const b_ids = sp->b_ids.at(ws); double* const b_scores = (double*)sp->b_scores.at(ws);
    rc = SRN_OK;
    for (uint32_t a = 0; a < A && rc == SRN_OK; ++a) {
        const size_t at = begin[a], na = begin[a + 1] - begin[a];
        if (na == 0) continue;
        const VisitorBatch sub{sp->g_hi.at(ws) + at, sp->g_lo.at(ws) + at, sp->g_item.at(ws) + at, r.consent ? sp->g_consent.at(ws) + at : nullptr,
                               r.times ? sp->g_time.at(ws) + at : nullptr, na, all.now_secs};
        rc = serve_arm(arms[a], store, sub, how_many, b_ids + at * how_many, b_scores + at * how_many, sp->b_counts.at(ws) + at,
                       o.rank ? sp->b_rank.at(ws) + at : nullptr, &log_rc, st);
        if (rc == SRN_OK) { sp->served[a] += na; if (o.feedback_rc) o.feedback_rc[a] = log_rc; }
    }
    (void)hipSetDevice(sp->device);
    if (rc == SRN_OK) {
        if (timed) (void)hipEventRecord(sp->tev[2], st);
        ScatterArgs sa{sp->perm.at(ws), sp->arm.at(ws), b_ids, sp->b_scores.at(ws), sp->b_counts.at(ws), sp->b_rank.at(ws), n32, (uint32_t)how_many,
                       o.ids, (uint64_t*)o.scores, o.counts, o.arm, o.rank};
        arm_scatter<<<blocks_of(n * how_many), kArmTPB, 0, st>>>(sa);
        if (hipGetLastError() != hipSuccess) rc = fail(SRN_EHIP, who + "the scatter's launch failed");
        if (timed) (void)hipEventRecord(sp->tev[3], st);
        sp->last_timed = timed && rc == SRN_OK;
        ++sp->calls;
    }
    (void)hipEventRecord(sp->last, st);   // whatever happened, the next call's kernels wait for what this one enqueued
    return rc;
}

int split_recommend_host(srn_traffic_split* sp, const srn_arm_t* arms, size_t n_arms, srn_device_sessions* store, const VisitorBatch& r, size_t how_many,
                         const SplitOut& o, int (*check_arm)(const srn_arm_t&, size_t)) {
    int rc = check_handles(sp, arms, n_arms); if (rc) return rc;
    const size_t n = r.n, rows = n * how_many;
    {   // refuse before anything is staged (the device form checks again, under the same mutex as its enqueue)
        std::lock_guard<std::mutex> g(sp->mu);
        bool nothing;
        if ((rc = check_call(sp, arms, n_arms, store, r, how_many, o, check_arm, &nothing))) return rc;
        if (nothing) { if (o.feedback_rc) std::fill(o.feedback_rc, o.feedback_rc + n_arms, SRN_OK); return SRN_OK; }
    }
    std::lock_guard<std::mutex> sg(sp->stage_mu);
    HIP_TRY(hipSetDevice(sp->device));
    Bump b;
    const auto hi = b.of<uint64_t>(n), lo = b.of<uint64_t>(n), item = b.of<uint64_t>(n), times = b.of<uint64_t>(n);
    const auto consent = b.of<uint8_t>(n), arm = b.of<uint8_t>(n);
    const auto ids = b.of<uint64_t>(rows); const auto scores = b.of<double>(rows); const auto counts = b.of<uint32_t>(n), rank = b.of<uint32_t>(n);
    hipStream_t st = sp->own;
    HIP_TRY(hipStreamSynchronize(st));   // (the previous host call blocked until its copies were done; a failed one may have left some behind)
    if ((rc = ensure(&sp->stage, &sp->stage_bytes, b.bytes))) return rc;
    char* const base = sp->stage;
    const struct { void* to; const void* from; size_t bytes; } copies[] = {
        {hi.at(base), r.key_hi, n * 8}, {lo.at(base), r.key_lo, n * 8}, {item.at(base), r.item, n * 8}, {consent.at(base), r.consent, n}, {times.at(base), r.times, n * 8}};
    for (const auto& c : copies) if (c.from) HIP_TRY(hipMemcpyAsync(c.to, c.from, c.bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(ids.at(base), 0, counts.off - ids.off, st));   // (entries beyond a row's count read as zero, as in buffers a caller cleared)
    const VisitorBatch dr{hi.at(base), lo.at(base), item.at(base), r.consent ? consent.at(base) : nullptr, r.times ? times.at(base) : nullptr, n, r.now_secs};
    const SplitOut d{ids.at(base), scores.at(base), counts.at(base), o.arm ? arm.at(base) : nullptr, o.rank ? rank.at(base) : nullptr, o.feedback_rc};
    if ((rc = split_recommend_device(sp, arms, n_arms, store, dr, how_many, d, st, check_arm))) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(hipSetDevice(sp->device));
    HIP_TRY(hipMemcpyAsync(o.ids, d.ids, rows * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(o.scores, d.scores, rows * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(o.counts, d.counts, n * 4, hipMemcpyDeviceToHost, st));
    if (o.arm) HIP_TRY(hipMemcpyAsync(o.arm, d.arm, n, hipMemcpyDeviceToHost, st));
    if (o.rank) HIP_TRY(hipMemcpyAsync(o.rank, d.rank, n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return check_all_served(o.counts, n);
}

}  // namespace srn
