// The latency paths of the device runtime: the one-launch form of srn_predict (a handful of sessions on host pointers, zero-copy) and the PERSISTENT form (resident
// workgroups the host posts sessions to).  What they share with the batch launch sequence of srn_runtime.hip -- geometry, the fast kernel's plan and buffers -- is in srn_runtime.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "srn_runtime.h"
#include "srn_hipsync.h"

namespace srn {

// Latency path: a handful of evolving sessions on host pointers (srn_predict: the reference's call shape, one session per call).
// No copies, no memsets, no events: the queries are written into pinned, device-mapped memory that the kernels read directly, the
// results come back the same way; two launches (prep kernel + general kernel, one workgroup per query) and one stream synchronise.
// Returns 1 if a query needs the global-table pass (the caller then takes the normal path).

// the call's pinned buffer: where its inputs, rows and the general kernel's retry list / count stand (regions of 64 bytes' alignment: at(w->pin) for the host, at(dp) for
// the device), and the buffer as the device sees it
struct TinyPin { Bump::Region<uint64_t> items{}, ids{}; Bump::Region<double> sc{}; Bump::Region<uint32_t> qoff{}, cnt{}, rc{}, rl{}; char* dp = nullptr; };
// grows the pinned buffer, copies the sessions in and points p's inputs and outputs at it
static int tiny_stage(Workspace* w, LaunchParams& p, const uint64_t* h_items, const uint32_t* h_qoff, TinyPin& t) {
    const size_t nitems = h_qoff[p.nq], n_out = (size_t)p.nq * p.how_many;
    Bump b(64);
    t.items = b.take<uint64_t>(nitems * 8); t.qoff = b.take<uint32_t>(((size_t)p.nq + 1) * 4); t.ids = b.take<uint64_t>(n_out * 8); t.sc = b.take<double>(n_out * 8); t.cnt = b.take<uint32_t>((size_t)p.nq * 4);
    t.rc = b.take<uint32_t>(4); t.rl = b.take<uint32_t>((size_t)p.nq * 4 + 4);
    const size_t off = b.bytes;
    if (w->pin_bytes < off) {
        if (w->pin) HIP_TRY(hipHostFree(w->pin));
        w->pin = nullptr; w->pin_bytes = 0;
        const size_t want = std::max<size_t>(off * 2, 256 * 1024);   // (room for a full round of the combiner at once: growing a pinned buffer stalls every lane)
        HIP_TRY(hipHostMalloc((void**)&w->pin, want, hipHostMallocMapped | hipHostMallocCoherent));   // (coherent: the fused launch's caller reads its rows as soon as the kernel's last pinned word says so)
        w->pin_bytes = want;
    }
    char* dp = nullptr; HIP_TRY(hipHostGetDevicePointer((void**)&dp, w->pin, 0));
    t.dp = dp;
    memcpy(t.items.at(w->pin), h_items, nitems * 8); memcpy(t.qoff.at(w->pin), h_qoff, ((size_t)p.nq + 1) * 4);
    *(volatile uint32_t*)t.rc.at(w->pin) = 0;
    p.items_flat = t.items.at(dp); p.q_off = t.qoff.at(dp);
    p.out_ids = t.ids.at(dp); p.out_scores = t.sc.at(dp); p.out_counts = t.cnt.at(dp);
    p.stats = nullptr; p.nb_rank = p.nb_num = p.nb_cnt = nullptr; p.phase_cycles = nullptr;
    return SRN_OK;
}
// the rows, from the pinned buffer to the caller's arrays
static void tiny_unstage(const Workspace* w, const LaunchParams& p, const TinyPin& t, uint64_t* h_ids, double* h_scores, uint32_t* h_counts) {
    const uint64_t* r_ids = t.ids.at(w->pin); const double* r_sc = t.sc.at(w->pin); const uint32_t* r_cnt = t.cnt.at(w->pin);
    for (uint32_t q = 0; q < p.nq; ++q) {
        const uint32_t n = r_cnt[q] == 0xFFFFFFFFu ? 0u : std::min<uint32_t>(r_cnt[q], p.how_many);
        h_counts[q] = r_cnt[q];
        memcpy(h_ids + (size_t)q * p.how_many, r_ids + (size_t)q * p.how_many, (size_t)n * 8);
        memcpy(h_scores + (size_t)q * p.how_many, r_sc + (size_t)q * p.how_many, (size_t)n * 8);
        std::fill(h_ids + (size_t)q * p.how_many + n, h_ids + (size_t)(q + 1) * p.how_many, 0ull);      // the unused tail of each row reads as 0
        std::fill(h_scores + (size_t)q * p.how_many + n, h_scores + (size_t)(q + 1) * p.how_many, 0.0);
    }
}
static int latency_wait(Workspace* w, hipStream_t st, bool blocking_wait) {
    if (blocking_wait) {   // a round several callers share: sleep on an interrupt instead of spinning on the signal (the host's cores belong to the callers)
        if (!w->ev_block) HIP_TRY(hipEventCreateWithFlags(&w->ev_block, hipEventBlockingSync | hipEventDisableTiming));
        HIP_TRY(hipEventRecord(w->ev_block, st));
        HIP_TRY(hipEventSynchronize(w->ev_block));
    } else HIP_TRY(hipStreamSynchronize(st));
    return SRN_OK;
}

// what the latency path's launches share
struct TinyCall {
    DeviceState* d; Workspace* w; const Geometry& geo; const LaunchParams& p; const FastPlan& plan; const Knobs& kn; const TinyPin& pin; hipStream_t st; bool blocking_wait;
    FastParams fp{};
};
// the general kernel, one workgroup per query: over all of the call's queries (fast_list false), or over what the fast sequence handed to it
static int tiny_general(const TinyCall& c, bool fast_list, uint32_t grid) {
    PredictLaunch a; a.masks = c.geo.masks; a.slot64 = c.geo.slot64; a.spill = c.w->spill;
    if (fast_list) { a.qlist = c.w->slow_list; a.qn = c.w->slow_cnt; }
    a.retry_list = c.pin.rl.at(c.pin.dp); a.retry_cnt = c.pin.rc.at(c.pin.dp);
    HIP_TRY(launch_predict(a, dim3(grid), c.geo.lds, c.st, c.d->di, c.p, c.geo.c));
    return SRN_OK;
}
static int tiny_finish_big(const TinyCall& c) {
    const LaunchParams& p = c.p;
    HIP_TRY(launch_finish_big(c.st, c.d->di, c.fp, p.out_ids, p.out_scores, p.out_counts, p.how_many, (uint32_t)std::min<uint64_t>(p.nq, (uint64_t)c.d->n_cu * 16), nullptr, c.w->slow_cnt, c.w->h_retry_dev));
    return SRN_OK;
}
// The kernels behind the fast kernel's first launch.  The fused launch is a whole first phase: the counters it publishes say whether a second one (these kernels, and a second
// wait) is needed at all.  The five-launch form (SRN_TINY_FUSED=0) has no second phase: they go behind the fast kernel with every call.  (Splitting the five launches into two
// phases on counters published by the finish kernel was measured in round 5 and lost at p90 / p99 -- profiles/r05_latency_phases.txt: removed.)
static int tiny_rest(const TinyCall& c) {
    const LaunchParams& p = c.p;
    if (c.plan.mid_tier) HIP_TRY(launch_fast(FastForm::Mid, dim3(p.nq), c.st, c.d->di, p, c.fp, c.kn.debug));
    { int rc = tiny_general(c, true, p.nq); if (rc) return rc; }
    HIP_TRY(launch_finish(c.st, c.d->di, c.fp, p.out_ids, p.out_scores, p.out_counts, p.nq, p.how_many));
    // (it also publishes the call's path counters -- handed over, listed for MID -- in the workspace's pinned words: srn_last_path_counts / srn_debug_last_mid_count after a
    //  latency-path call used to say "all through the general kernel")
    return tiny_finish_big(c);
}
// (SRN_DEBUG: how often a single-session call needs the kernels behind the fused launch, and why)
static void tiny_fused_stats(uint32_t n_slow, uint32_t n_mid, uint32_t n_big) {
    static std::atomic<uint64_t> calls{0}, second{0}, why[3] = {{0}, {0}, {0}};
    const uint64_t c = calls.fetch_add(1) + 1;
    if ((n_slow | n_mid | n_big) != 0u) { second.fetch_add(1); if (n_slow) why[0].fetch_add(1); if (n_mid) why[1].fetch_add(1); if (n_big) why[2].fetch_add(1); }
    if (c % 1000 == 0) fprintf(stderr, "[srn] fused single-session calls: %llu, with a second phase %llu (handed to the general kernel %llu, listed for MID %llu, > 63 entries %llu)\n",
                               (unsigned long long)c, (unsigned long long)second.load(), (unsigned long long)why[0].load(), (unsigned long long)why[1].load(), (unsigned long long)why[2].load());
}
// (round 5) ONE evolving session per call -- srn_predict, the reference's call shape: one launch.  The fast kernel's TINY instantiation writes the prep record itself,
// serves the query and finishes its row from registers; the counters it publishes say whether anything is left for the kernels behind it (SRN_TINY_FUSED=0: five launches).
static int tiny_fused(TinyCall& c, const uint64_t* h_items, const uint32_t* h_qoff) {
    Workspace* w = c.w; const LaunchParams& p = c.p; FastParams& fp = c.fp;
    uint32_t L1 = 0; for (uint32_t q = 0; q < p.nq; ++q) L1 = std::max(L1, h_qoff[q + 1] - h_qoff[q]);   // the call's longest session
    if (w->cnt_dirty) HIP_TRY(hipMemsetAsync(w->slow_cnt, 0, sizeof(SlowCntBlock), c.st));   // (only after a call that left the counters non-zero: the fused launch leaves them at 0 unless it hands work on)
    w->cnt_dirty = true;   // (until this call is known to have ended cleanly with nothing handed on: an error return in between must not leave a stale ticket behind a "clean" flag -- ADVICE r5)
    fp.tiny_len = p.nq == 1 && L1 >= 1u && L1 <= 8u ? L1 : 0u;   // (a single session's items in the kernel arguments where they fit)
    for (uint32_t i = 0; i < fp.tiny_len; ++i) fp.tiny_items[i] = h_items[h_qoff[0] + i];
    uint32_t seq = ++w->tiny_seq; if (seq == 0u) seq = ++w->tiny_seq;
    fp.host_seq = seq; fp.host_words = w->h_retry_dev;
    // (a session of > 4 items goes to the MID form at once -- the lean form would only list it: five lists, numerators beyond 15)
    HIP_TRY(launch_fast(c.plan.mid_tier && L1 > 4u ? FastForm::TinyMid : FastForm::Tiny, dim3(p.nq), c.st, c.d->di, p, fp, c.kn.debug));
    fp.host_words = nullptr; fp.tiny_len = 0;
    const volatile uint32_t* hw = w->h_retry;
    bool seen = false;
    if (!c.blocking_wait && !c.kn.no_tiny_spin) {
        // the kernel's last store is the call's number in a pinned word, behind a system-scope fence: the row is readable as soon as the host sees it -- before the
        // queue's completion signal (end-of-kernel cache write-back, signal, the runtime's poll of it) has made its way.  A bounded spin: a fault shows in the stream's wait
        const auto t0 = std::chrono::steady_clock::now();
        for (uint32_t spin = 0; !seen; ++spin) {
            seen = hw[HW_SEQ] == seq;
            if (!seen) {
                __builtin_ia32_pause();   // (the sibling hyper-thread may be another caller spinning on ITS workspace)
                if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
    }
    if (!seen) { int rc = latency_wait(w, c.st, c.blocking_wait); if (rc) return rc; }
    // the counters are this call's only if the kernel published its number behind them; a fused launch that ended without doing so (it cannot, short of a
    // fault the wait above would have reported) gets the full second phase rather than a guess from stale words
    if (hw[HW_SEQ] != seq) { int rc = tiny_rest(c); return rc ? rc : latency_wait(w, c.st, c.blocking_wait); }
    const uint32_t n_slow = hw[HW_GENERAL], n_mid = hw[HW_MID], n_big = hw[HW_OVER63];
    if (c.kn.debug) tiny_fused_stats(n_slow, n_mid, n_big);
    if ((n_slow | n_mid | n_big) == 0u) { w->cnt_dirty = false; return SRN_OK; }   // (a clean end with nothing handed on: the counters and the workgroup ticket are back at 0)
    // the second phase (handed to the general kernel | listed for MID | queries with > 63 entries)
    int rc = SRN_OK;
    if (n_mid == 0u) {   // (nothing listed for MID: the general kernel over what was handed to it -- it writes its rows itself -- and finish-big for a row the fused launch could not finish, each only if needed)
        if (n_slow) rc = tiny_general(c, true, std::min<uint32_t>(p.nq, n_slow));
        if (!rc && n_big) rc = tiny_finish_big(c);
    }
    else rc = tiny_rest(c);
    return rc ? rc : latency_wait(w, c.st, c.blocking_wait);
}

int device_predict_tiny(DeviceState* d, const FlatIndex& ix, Workspace* w, const Geometry& geo, LaunchParams p, const uint64_t* h_items, const uint32_t* h_qoff,
                        uint64_t* h_ids, double* h_scores, uint32_t* h_counts, bool blocking_wait) {
    TinyPin pin; { int rc = tiny_stage(w, p, h_items, h_qoff, pin); if (rc) return rc; }
    hipStream_t st = w->stream;
    const size_t cap_q = std::max<size_t>(p.nq, (size_t)std::max(1, knobs().tiny_max));   // (sized once for the largest round: hipFree / hipMalloc synchronise the device)
    { int rc = ensure(&w->spill, &w->spill_bytes, cap_q * p.k * geo.slot_bytes); if (rc) return rc; }
    const uint32_t prep_stride = prep_stride_of(p.max_len);
    { int rc = ensure(&w->prep, &w->prep_bytes, cap_q * prep_stride); if (rc) return rc; }
    // The fast kernel's launch sequence on the same zero-copy buffers where it pays (round 4): a batch with a session of > 8 items puts ALL its queries on the general kernel's
    // non-position-set build -- 143 us per call against 52 us on config 3, and one such session in a combined round of srn_predict calls slows the whole round -- while the
    // lean / MID instantiations serve sessions of <= 10 items at the short sessions' cost.  Four more launches (~2 us each on an idle stream), no more synchronisation.
    const Knobs kn = knobs();
    const FastPlan plan = fast_plan(d, ix, p, geo, kn, false);
    const bool tiny_fast = plan.fast && (kn.tiny_fast == 3 || (kn.tiny_fast >= 1 && p.max_len > 8) || (kn.tiny_fast == 2 && p.nq <= (kn.no_tiny_fused ? 32u : (uint32_t)kn.tiny_fused_max)));   // (the crossover measured with tools/tiny_crossover.py: profiles/r04_serving_tiny_fast.txt)
    if (tiny_fast) { int rc = reserve_fast(w, cap_q); if (rc) return rc; }   // (sized once, for the largest round)
    const bool fused = tiny_fast && p.nq <= (uint32_t)kn.tiny_fused_max && !kn.no_tiny_fused;
    if (!fused) { w->cnt_dirty = true; HIP_TRY(launch_prep(st, d->di, p.items_flat, p.q_off, p.nq, p.m, p.max_len, w->prep, prep_stride, plan.nb_fast == 3u, tiny_fast ? w->slow_cnt : nullptr)); }
    p.prep = w->prep; p.prep_stride = prep_stride;
    TinyCall c{d, w, geo, p, plan, kn, pin, st, blocking_wait};
    int rc = SRN_OK;
    if (fused) { c.fp = fast_params(d, w, plan, cap_q, plan.mid_tier ? TIER_MID : 0u); rc = tiny_fused(c, h_items, h_qoff); }   // (no BIG / LONG tier on the latency path)
    else if (tiny_fast) {
        c.fp = fast_params(d, w, plan, cap_q, plan.mid_tier ? TIER_MID : 0u);
        HIP_TRY(launch_fast(FastForm::Lean, dim3(p.nq), st, d->di, p, c.fp, kn.debug));
        rc = tiny_rest(c);
        if (!rc) rc = latency_wait(w, st, blocking_wait);
    } else {
        rc = tiny_general(c, false, p.nq);
        if (!rc) rc = latency_wait(w, st, blocking_wait);
    }
    if (rc) return rc;
    if (*(volatile uint32_t*)pin.rc.at(w->pin) != 0) return 1;   // (rare: tables too small for some query)
    // what the timing / path-count APIs report after this call: its query count, how many of them the fast sequence handed to the general kernel (all of them where the
    // two-launch form ran), not timed (the stream is idle here: nothing of an earlier call is still writing the pinned words)
    ++w->untimed_calls; w->last_nq = p.nq; w->last_retry = 0; w->last_fast = tiny_fast; w->last_mid = tiny_fast && plan.mid_tier; w->last_dedup = false; w->last_light = false; w->last_untimed = true;   // (`calls` indexes the event ring: timed calls only)
    tiny_unstage(w, p, pin, h_ids, h_scores, h_counts);
    return SRN_OK;
}


// =====================================================================================================================================================================
// The PERSISTENT latency path (round 6).  srn_predict on the one-launch form costs 28 us from a C++ host of which ~13 us are the GPU's work: the rest
// is queue submission and completion signalling.  Here a workgroup of vmis_fast_kernel<TINY> stays RESIDENT (one third of one CU) and polls a pinned control block
// (ServeCtl, srn_kernels.h): the host writes the session and then its number, the workgroup serves it -- same code, same rows -- and answers with the number; the host
// spins on its own memory.  Doorbell round trip measured on this platform: 1.6 us (tools/ring_probe.hip).  A session the fused form would hand on (general kernel, MID,
// > 63 entries: 0.3-3 % of config 3's) comes back with status 1 and takes the launch path, as does any call whose k / m / how_many / flags are not the resident ones.
// hipFree / hipDeviceSynchronize would wait for a resident workgroup for ever: every such call of the library goes through srn_hipsync.h, which makes them leave first.
// =====================================================================================================================================================================
struct ServeForm {   // one resident launch: N workgroups of the lean form (sessions of <= 4 items) or of the form for 5..10 items
    DeviceState* d = nullptr; bool mid = false; std::atomic<bool> dead{false}; uint32_t n = 0;
    hipStream_t st = nullptr;
    ServeCtl* ctl = nullptr; ServeCtl* ctl_dev = nullptr;   // [n], pinned
    char* rows = nullptr; char* rows_dev = nullptr; size_t row_bytes = 0;   // [n] x (ids | scores), pinned
    char *prep = nullptr, *fin = nullptr, *big = nullptr; uint32_t *slow_list = nullptr, *slow_cnt = nullptr, *counts = nullptr;
    LaunchParams p{}; FastParams fp{};
    std::unique_ptr<std::atomic<int>[]> busy; std::vector<uint32_t> seq;   // per workgroup: taken by a caller; the last number posted
    std::unique_ptr<std::atomic<uint64_t>[]> lane_served;   // per workgroup: sessions it answered itself (test aid: srn_debug_serve_lane_counts)
    std::mutex mu; bool running = false;   // (mu: starting / parking the launch)
};
struct ServeState {
    std::vector<ServeForm*> forms; uint32_t k = 0, m = 0, how_many = 0, flags = 0, max_items = 0; unsigned long long idle_ticks = 0;
    std::atomic<uint64_t> served{0}, not_served{0}, launches{0};
};
static std::mutex g_serve_mu; static std::vector<ServeForm*> g_serve_forms; static std::atomic<int> g_serve_running{0};

static void lane_lock(ServeForm* f, uint32_t i) { int e = 0; while (!f->busy[i].compare_exchange_weak(e, 1, std::memory_order_acquire)) { e = 0; __builtin_ia32_pause(); } }
static void lane_unlock(ServeForm* f, uint32_t i) { f->busy[i].store(0, std::memory_order_release); }
// (f->mu held, no lane held by this thread) the resident workgroups leave -- after the sessions they are serving
static void form_park(ServeForm* f) {
    if (!f->running) return;
    for (uint32_t i = 0; i < f->n; ++i) lane_lock(f, i);   // (nobody is posting, nothing is in flight)
    int cur = 0; (void)hipGetDevice(&cur);
    if (cur != f->d->device) (void)hipSetDevice(f->d->device);
    for (uint32_t i = 0; i < f->n; ++i) __atomic_store_n(&f->ctl[i].stop, 1u, __ATOMIC_RELEASE);
    (void)hipStreamSynchronize(f->st);
    if (cur != f->d->device) (void)hipSetDevice(cur);
    f->running = false; g_serve_running.fetch_sub(1);
    for (uint32_t i = 0; i < f->n; ++i) lane_unlock(f, i);
}
static std::atomic<int> g_serve_hold{0};   // > 0: some thread is inside a call that waits for the whole device (hipFree ...): no resident launch may start
void serve_hold_begin() { g_serve_hold.fetch_add(1, std::memory_order_acq_rel); serve_quiesce_all(); }
void serve_hold_end() { g_serve_hold.fetch_sub(1, std::memory_order_acq_rel); }
void serve_quiesce_all() {
    if (g_serve_running.load(std::memory_order_acquire) == 0) return;
    std::lock_guard<std::mutex> lk(g_serve_mu);
    for (ServeForm* f : g_serve_forms) { std::lock_guard<std::mutex> fl(f->mu); form_park(f); }
}
// (f->mu held, no lane held by this thread) start the resident launch
static int form_launch(ServeState* s, ServeForm* f) {
    // (a launch that starts now would be parked at once, or worse, waited for by the free in progress: the caller takes the launch path this time.  A hold that begins
    //  right after this look parks what is started here: its quiesce takes f->mu, which the caller of this function holds)
    if (g_serve_hold.load(std::memory_order_acquire) > 0) return SRN_ESTATE;
    if (f->running) {   // (workgroups that left by their idle timeout: the launch is over once all have)
        bool all_gone = true; for (uint32_t i = 0; i < f->n; ++i) all_gone = all_gone && __atomic_load_n(&f->ctl[i].alive, __ATOMIC_ACQUIRE) == 0u;
        if (!all_gone) { form_park(f); } else { HIP_TRY(hipSetDevice(f->d->device)); HIP_TRY(hipStreamSynchronize(f->st)); f->running = false; g_serve_running.fetch_sub(1); }
    }
    for (uint32_t i = 0; i < f->n; ++i) lane_lock(f, i);
    auto unlock_all = [&]() { for (uint32_t i = 0; i < f->n; ++i) lane_unlock(f, i); };
    hipError_t e = hipSetDevice(f->d->device);
    for (uint32_t i = 0; i < f->n && e == hipSuccess; ++i) { ServeCtl& c = f->ctl[i]; c.stop = 0; c.alive = 1; c.idle_ticks = s->idle_ticks; c.seq = f->seq[i]; c.done_seq = f->seq[i]; }   // (a post an earlier launch never answered is not served late)
    std::atomic_thread_fence(std::memory_order_seq_cst);
    if (e == hipSuccess) e = hipMemsetAsync(f->slow_cnt, 0, sizeof(SlowCntBlock), f->st);
    if (e == hipSuccess) e = launch_fast(f->mid ? FastForm::TinyMid : FastForm::Tiny, dim3(f->n), f->st, f->d->di, f->p, f->fp);
    if (e == hipSuccess) { f->running = true; g_serve_running.fetch_add(1); s->launches.fetch_add(1); }
    unlock_all();
    return e == hipSuccess ? SRN_OK : fail(SRN_EHIP, std::string("the persistent latency path: ") + hipGetErrorString(e));
}
static void form_free(ServeForm* f) {
    { std::lock_guard<std::mutex> lk(g_serve_mu); g_serve_forms.erase(std::remove(g_serve_forms.begin(), g_serve_forms.end(), f), g_serve_forms.end()); }
    { std::lock_guard<std::mutex> fl(f->mu); form_park(f); }
    for (void* q : {(void*)f->prep, (void*)f->fin, (void*)f->big, (void*)f->slow_list, (void*)f->slow_cnt, (void*)f->counts}) if (q) (void)hipFree(q);
    if (f->ctl) (void)hipHostFree(f->ctl); if (f->rows) (void)hipHostFree(f->rows);
    if (f->st) (void)hipStreamDestroy(f->st);
    delete f;
}
// srn_index_serve_stop may run while other threads are inside srn_predict: a caller that read the state's pointer a moment ago must still find its memory.  Stop therefore
// RETIRES the state -- its forms are marked dead (no new session is posted, no launch is started again) and parked (every session in flight is answered first) -- and
// only device_release (srn_index_free: nobody may be using the index any more) frees it.
void serve_free_retired(DeviceState* d) {
    std::vector<ServeState*> old;
    { std::lock_guard<std::mutex> lk(d->mu); old.swap(d->serve_retired); }
    for (ServeState* s : old) { for (ServeForm* f : s->forms) form_free(f); delete s; }
}
int device_serve_stop(DeviceState* d) {
    ServeState* s = d->serve.exchange(nullptr);
    if (!s) return SRN_OK;
    HIP_TRY(hipSetDevice(d->device));
    for (ServeForm* f : s->forms) { f->dead.store(true); std::lock_guard<std::mutex> fl(f->mu); form_park(f); }
    { std::lock_guard<std::mutex> lk(d->mu); d->serve_retired.push_back(s); }
    return SRN_OK;
}
int device_serve_start(DeviceState* d, const FlatIndex& ix, uint32_t k, uint32_t m, uint32_t how_many, uint32_t flags, uint32_t lanes, uint32_t max_items, uint32_t idle_ms) {
    int rc = device_serve_stop(d); if (rc) return rc;
    if (lanes == 0) return SRN_OK;
    if (lanes > 256) return fail(SRN_ERANGE, "at most 256 resident workgroups per form");
    HIP_TRY(hipSetDevice(d->device));
    const Knobs kn = knobs();
    ServeState* s = new ServeState(); s->k = k; s->m = m; s->how_many = how_many; s->flags = flags; s->max_items = std::min<uint32_t>(std::max<uint32_t>(max_items, 1), F_MID_LMAX);
    s->idle_ticks = (unsigned long long)std::max<uint32_t>(idle_ms, 1) * 100000ull;   // (wall_clock64: 100 MHz)
    auto undo = [&](int code, const std::string& why) { for (ServeForm* f : s->forms) form_free(f); delete s; return fail(code, why); };   // (never published: nobody else holds it)
    // A resident launch never ends, and HIP multiplexes its streams onto a few hardware queues per priority level: on a queue shared with another stream everything
    // behind the resident kernel would wait for ever.  The resident streams take the LOWEST priority level, which nothing else in this library uses.
    int prio_lo = 0, prio_hi = 0; (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    for (int form = 0; form < (s->max_items > 4 ? 2 : 1); ++form) {
        ServeForm* f = new ServeForm(); f->d = d; f->mid = form == 1; f->n = lanes; s->forms.push_back(f);
        f->busy.reset(new std::atomic<int>[lanes]); for (uint32_t i = 0; i < lanes; ++i) f->busy[i].store(0); f->seq.assign(lanes, 0u);
        f->lane_served.reset(new std::atomic<uint64_t>[lanes]); for (uint32_t i = 0; i < lanes; ++i) f->lane_served[i].store(0);
        { std::lock_guard<std::mutex> lk(g_serve_mu); g_serve_forms.push_back(f); }
        LaunchParams& p = f->p;
        p.nq = lanes; p.k = k; p.m = m; p.how_many = how_many; p.flags = flags; p.max_len = f->mid ? F_MID_LMAX : 8u;
        Geometry geo; if (make_geometry(d, ix, p, 0, geo) != SRN_OK) return undo(SRN_EINVAL, "the persistent latency path: no LDS geometry for these parameters");
        const FastPlan plan = fast_plan(d, ix, p, geo, kn, false);
        if (!plan.fast || (f->mid && !plan.mid_tier)) return undo(SRN_EINVAL, "the persistent latency path serves what the fast kernels serve (k <= 1536, m <= 2560 and <= m_index, how_many <= 64, complete lists)");
        f->row_bytes = ((size_t)how_many * 16 + 63) / 64 * 64;
        if (hipStreamCreateWithPriority(&f->st, hipStreamNonBlocking, prio_lo) != hipSuccess ||
            hipHostMalloc((void**)&f->ctl, sizeof(ServeCtl) * lanes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostMalloc((void**)&f->rows, f->row_bytes * lanes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void**)&f->ctl_dev, f->ctl, 0) != hipSuccess || hipHostGetDevicePointer((void**)&f->rows_dev, f->rows, 0) != hipSuccess)
            return undo(SRN_ENOMEM, "the persistent latency path: pinned control blocks");
        memset(f->ctl, 0, sizeof(ServeCtl) * lanes); memset(f->rows, 0, f->row_bytes * lanes);
        const uint32_t prep_stride = prep_stride_of(p.max_len);
        const uint64_t big_entries = (uint64_t)lanes * 1024 + 4096;
        if (hipMalloc((void**)&f->prep, (size_t)prep_stride * lanes + 256) != hipSuccess || hipMalloc((void**)&f->fin, (size_t)F_FIN_BYTES * lanes + 1024) != hipSuccess ||
            hipMalloc((void**)&f->big, big_entries * 16 + (size_t)lanes * 4 + 64) != hipSuccess || hipMalloc((void**)&f->slow_list, ((size_t)lanes * 4 + 64) * 4) != hipSuccess ||
            hipMalloc((void**)&f->slow_cnt, sizeof(SlowCntBlock)) != hipSuccess || hipMalloc((void**)&f->counts, (size_t)lanes * 4 + 64) != hipSuccess)
            return undo(SRN_ENOMEM, "the persistent latency path: device scratch");
        p.items_flat = nullptr; p.q_off = nullptr;
        // a workgroup's row: ids at rows + q * how_many * 8 ... the kernels address rows as out_ids[q * how_many + rank]: ids of all workgroups, then scores of all
        p.out_ids = (uint64_t*)f->rows_dev; p.out_scores = (double*)(f->rows_dev + (size_t)lanes * how_many * 8); p.out_counts = f->counts;
        if ((size_t)lanes * how_many * 16 > f->row_bytes * lanes) return undo(SRN_EINVAL, "row buffer");
        p.stats = nullptr; p.nb_rank = p.nb_num = p.nb_cnt = nullptr; p.phase_cycles = nullptr; p.prep = f->prep; p.prep_stride = prep_stride;
        f->fp = fast_params(d, FastBuffers{f->slow_list, lanes, f->slow_cnt, f->fin, f->big, big_entries}, plan);   // (the form's own buffers; no tier behind it: what it cannot serve takes the launch path)
        f->fp.serve = f->ctl_dev;
    }
    for (ServeForm* f : s->forms) { std::lock_guard<std::mutex> fl(f->mu); rc = form_launch(s, f); if (rc && rc != SRN_ESTATE) return undo(rc, last_error_string()); }   // (SRN_ESTATE: another thread is freeing device memory right now -- the first call that wants the form starts it)
    d->serve.store(s);
    return SRN_OK;
}
int device_serve_stats(DeviceState* d, uint64_t* served, uint64_t* not_served, uint64_t* launches, uint32_t* lanes) {
    ServeState* s = d->serve.load();
    if (served) *served = s ? s->served.load() : 0; if (not_served) *not_served = s ? s->not_served.load() : 0; if (launches) *launches = s ? s->launches.load() : 0;
    uint32_t n = 0; if (s) for (ServeForm* f : s->forms) n += f->n;
    if (lanes) *lanes = n;
    return SRN_OK;
}
int device_serve_lane_counts(DeviceState* d, uint32_t form, uint64_t* out_served, size_t cap, size_t* out_n) {   // (test aid) per resident workgroup of one form: sessions it answered itself
    ServeState* s = d->serve.load();
    if (!s || form >= s->forms.size()) return fail(SRN_ESTATE, "no such resident form");
    ServeForm* f = s->forms[form];
    if (out_n) *out_n = f->n;
    if (cap < f->n) return fail(SRN_ERANGE, "one counter per resident workgroup of the form");
    for (uint32_t i = 0; i < f->n; ++i) out_served[i] = f->lane_served[i].load(std::memory_order_relaxed);
    return SRN_OK;
}
int device_serve_last_stamps(DeviceState* d, uint32_t* out4) {   // (measurement aid) 100 MHz ticks of the lean form's first workgroup's last session: waited | record written | answered
    ServeState* s = d->serve.load();
    if (!s || s->forms.empty()) return fail(SRN_ESTATE, "nothing resident");
    for (int i = 0; i < 4; ++i) out4[i] = s->forms[0]->ctl[0].stamp[i];
    return SRN_OK;
}
int device_serve_predict(DeviceState* d, const uint64_t* items, uint32_t len, uint32_t k, uint32_t m, uint32_t how_many, uint32_t flags, uint64_t* out_ids, double* out_scores, size_t* out_n) {
    ServeState* s = d->serve.load(std::memory_order_acquire);
    if (!s || k != s->k || m != s->m || how_many != s->how_many || flags != s->flags || len == 0 || len > s->max_items) return 1;
    ServeForm* f = s->forms[len > 4 ? 1 : 0];
    if (f->dead) return 1;
    for (int attempt = 0; attempt < 2; ++attempt) {
        uint32_t li = f->n;
        for (uint32_t i = 0; i < f->n; ++i) { int e = 0; if (f->busy[i].compare_exchange_strong(e, 1, std::memory_order_acquire)) { li = i; break; } }
        if (li == f->n) { s->not_served.fetch_add(1); return 1; }   // (every resident workgroup of that form is taken: the launch path)
        ServeCtl* c = &f->ctl[li];
        if (!f->running || __atomic_load_n(&c->alive, __ATOMIC_ACQUIRE) == 0u) {   // parked (something freed device memory) or gone (idle): start the launch again, then look for a lane again
            lane_unlock(f, li);
            std::lock_guard<std::mutex> fl(f->mu);
            if (f->dead.load()) { s->not_served.fetch_add(1); return 1; }   // (retired by srn_index_serve_stop in the meantime: never started again)
            bool gone = !f->running; for (uint32_t i = 0; i < f->n && !gone; ++i) gone = __atomic_load_n(&f->ctl[i].alive, __ATOMIC_ACQUIRE) == 0u;
            if (gone) { const int lrc = form_launch(s, f); if (lrc != SRN_OK) { if (lrc != SRN_ESTATE) f->dead = true; s->not_served.fetch_add(1); return 1; } }
            continue;
        }
        uint32_t chk = 0; for (uint32_t i = 0; i < std::min<uint32_t>(len, 5u); ++i) chk ^= (uint32_t)items[i] ^ (uint32_t)(items[i] >> 32);
        for (uint32_t i = 5; i < len; ++i) c->more[i - 5] = items[i];
        for (uint32_t i = 0; i < std::min<uint32_t>(len, 5u); ++i) c->items[i] = items[i];
        uint32_t seq = ++f->seq[li]; if (seq == 0u) seq = ++f->seq[li];
        c->len = len; c->check = chk ^ seq ^ len;
        __atomic_store_n(&c->seq, seq, __ATOMIC_RELEASE);
        const auto t0 = std::chrono::steady_clock::now();
        bool seen = false;
        for (uint32_t spin = 0;; ++spin) {
            if (__atomic_load_n(&c->done_seq, __ATOMIC_ACQUIRE) == seq) { seen = true; break; }
            __builtin_ia32_pause();
            if ((spin & 1023u) == 1023u) {
                if (__atomic_load_n(&c->alive, __ATOMIC_ACQUIRE) == 0u) break;   // (it left between our look and our post: its idle timeout)
                if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) { f->dead = true; break; }   // (a fault: the form is not used again)
            }
        }
        int ret = 1;
        if (seen && __atomic_load_n(&c->status, __ATOMIC_RELAXED) == 0u) {
            const uint32_t n = std::min<uint32_t>(__atomic_load_n(&c->count, __ATOMIC_RELAXED), how_many);
            memcpy(out_ids, f->rows + ((size_t)li * how_many) * 8, (size_t)n * 8);
            memcpy(out_scores, f->rows + ((size_t)f->n * how_many + (size_t)li * how_many) * 8, (size_t)n * 8);
            *out_n = n; ret = 0;
        }
        lane_unlock(f, li);
        (ret == 0 ? s->served : s->not_served).fetch_add(1);
        if (ret == 0) f->lane_served[li].fetch_add(1, std::memory_order_relaxed);
        return ret;
    }
    s->not_served.fetch_add(1);
    return 1;
}

}  // namespace srn
