// Click feedback log: the last row served to every visitor, scored against the visitor's next click (include/serenade_hip.h, "click feedback").
//
// The rule, request by request, is serving.feedback_model's; the device gives the same ranks and counters for a whole batch, on the caller's stream, nothing read back.
//
// The table: power-of-two open addressing, linear probing, load <= 0.5, no tombstones, an object of its own beside the session store.  One slot per visitor:
//   { key_hi u64 | key_lo u64 | epoch u64 | count u32 | state u32 | n_model u32 | pad u32 | ids u64[row_cap] }   rounded up to a multiple of 128 bytes, 128-byte aligned
// (row_cap <= 11: one 128-byte line).  state: 0 empty, 1 occupied, 2 claimed by the find kernel of the running call.  One table stands; a sweep allocates the second
// one, rebuilds the entries not older than the TTL into it and frees the first.
//
// A batch:
//   sort       request indices, stable LSD passes by key_lo, key_hi, then the consent bit (the session store's order): the consenting requests of one visitor become
//              one contiguous RUN in request order
//   fb_find    one lane per run head: find-or-insert the slot by the store's claim protocol -- CAS empty -> claimed; two heads never hold the same key, so a claimed slot
//              is never "mine" and the loser of a claim probes on: nobody waits for anybody.  Records the slot and whether the stored entry is new, idle or live
//   max scan   of the heads' positions: every position's run start
//   fb_rank    one lane group (8 lanes for rows of up to 8 ids, else 16) per request.  The prior row of a run head is its slot's, if live; of any other request the row
//              served to the previous request of the run, n_model counted from that row's scores.  Lane l of the group takes positions l, l + lanes, ...; a ballot per
//              round finds the match and counts the finite scores.  No lane leaves before the last ballot and the round count is the same across the wave.  The group's
//              first lane writes out_rank and adds to a histogram in LDS; the workgroup then issues one 64-bit global atomic per non-zero bin.  The grid is capped at
//              2048 workgroups, each taking every 2048th block of positions, so that a call of 2^20 requests ends in at most 2048 atomics per counter word, not 65536
//   fb_store   behind fb_rank: the run's last request writes its row, count, n_model, epoch and state full, once (the same lane groups)
//   fb_boot    only while the bootstrap is enabled (srn_feedback_bootstrap_enable), behind fb_rank and fb_store: one lane per replicate weighs every
//              observed request with w(seed, replicate, visitor) and adds it to the replicate's own observed count and histograms (its comment below)
// Integer work throughout: ranks, counters and the table's entries do not depend on the run or on how the requests are cut into calls.
// A batch whose requests carry their own clocks (srn_feedback_observe*_at) runs the timed form of fb_find, fb_rank and fb_store -- one body each,
// template <bool kTimed> -- behind one gather of the times into sorted order: a run head tests its slot's epoch against its own time; any other request tests its
// predecessor's time -- the epoch the predecessor's row would have been stored with -- and a break is counted as idle_expired; the run's last request stores its own
// time.  The runs are the untimed call's, so one max scan over the run heads still gives the slot.
// The table underneath -- the slot's head, the count and rebuild kernels over a payload functor, the capacity rule (make_room), the sweep's tail, the one-key read-back
// and create's and free's shared halves -- is srn_visitor_table.h's, shared with the session store.  Here: the payload (count, n_model, ids), the batch
// kernels, the single table and the sweep that allocates its successor, the counters, the histograms and the bootstrap's words.
// The sort, the run predicates, the find-or-claim probe and what a batch call opens with (the sorted front of the call's VisitorBatch, the timed / untimed dispatch,
// the host stage) are srn_visitors.h's, shared with the session store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "srn_internal.h"
#include "srn_runtime.h"
#include "srn_device.h"
#include "srn_visitor_table.h"  // the table, its kernels and the capacity rule (shared with srn_sessions_dev.hip)
#include "srn_visitors.h"       // the run predicates, find_or_claim, the key sort, the sorted front and the host stage
#include "srn_bootstrap.h"      // the weight rule and the key's fold
#include "srn_hipsync.h"

struct srn_feedback : srn::VisitorTable {                   // one table stands: a sweep rebuilds into a second one, allocated for it; stats / get / sweep / reset run on `own`
    uint64_t row_cap = 0;
    unsigned long long* ctr = nullptr;                      // the counters: 8 words, hits_model[row_cap + 1], hits_filled[row_cap + 1]
    unsigned long long* boot = nullptr;                     // the bootstrap's replicate words (null: off), word-major [1 + 2 * row_cap][boot_b]: observed_w, then
    uint32_t boot_b = 0; uint64_t boot_seed = 0;            // hits_model_w[1 .. row_cap], then hits_filled_w[1 .. row_cap] -- a flush's lanes add to adjacent words
    size_t boot_words() const { return (size_t)(1 + 2 * row_cap) * boot_b; }
    uint32_t n_bins() const { return 8u + 2u * ((uint32_t)row_cap + 1u); }
};

namespace srn {

namespace {
constexpr uint32_t kTPB = kTableTPB;            // (grid_for)
constexpr uint32_t kRankBlocks = 2048;          // fb_rank's grid at the most (256 CUs x 8 workgroups): each workgroup pays one global atomic per non-zero bin
constexpr uint32_t kFbHead = 40;                // bytes before the ids
struct FbSlot { uint64_t key_hi, key_lo, epoch; uint32_t count, state, n_model, pad; };
static_assert(sizeof(FbSlot) == kFbHead, "slot header");
// bins of the counters: the words of srn_feedback_stats_t in its order, then the two histograms
enum : uint32_t { kRequests = 0, kNoConsent = 1, kFirstSeen = 2, kIdleExpired = 3, kObserved = 4, kHitsModel = 5, kHitsFilled = 6, kStored = 7, kHist = 8 };
enum : uint32_t { kNew = 0, kIdle = 1, kLive = 2 };   // what fb_find saw in a head's slot

__device__ __forceinline__ FbSlot* fb_slot(const Table& t, uint32_t s) { return (FbSlot*)(t.base + (size_t)s * t.stride); }
__device__ __forceinline__ uint64_t* fb_ids(FbSlot* h) { return (uint64_t*)((char*)h + kFbHead); }
__device__ __forceinline__ bool finite_bits(uint64_t b) { return ((b >> 52) & 0x7FFull) != 0x7FFull; }

struct ObsArgs {
    Table t;
    const uint64_t* key_hi; const uint64_t* key_lo; const uint64_t* item; const uint8_t* consent;   // the caller's requests
    const uint64_t* ids; const uint64_t* scores; const uint32_t* counts; uint32_t how_many;         // ... and rows (scores as bit patterns; may be null)
    const uint32_t* order;   // [n] request index of each sorted position
    uint32_t n, row_cap;
    uint32_t lanes_shift;    // 2^lanes_shift adjacent lanes take one request
    uint32_t rounds;         // ceil(row_cap / lanes): the same for every group
    uint64_t now, idle;
    uint32_t* slot_of;       // [n] by sorted position of a run head: its slot (kNone: table full -- cannot happen under the capacity rule)
    uint32_t* status;        // [n] ... and kNew / kIdle / kLive
    uint32_t* headpos;       // [n] p for a run head, 0 otherwise; inclusive max scan -> run_start
    uint32_t* run_start;     // [n]
    uint32_t* out_rank;      // [n] by REQUEST index (may be null)
    unsigned long long* ctr;
    uint32_t* err;
    const uint64_t* when;    // a timed batch: [n] times[order[p]], read in `now`'s place, so that a position reads when[p] and when[p - 1] as adjacent
                             // words.  Null and never read in an untimed one
};
// the row served to request req: its length as it is stored
__device__ __forceinline__ uint32_t served_count(const ObsArgs& a, uint32_t req) { const uint32_t c = a.counts[req]; return c == SRN_FEEDBACK_NONE ? 0u : min(c, a.how_many); }

// one lane per run head: its slot, and whether the stored entry is new, idle -- at `now` or (timed) at the head's own time -- or live
template <bool kTimed>
__global__ void __launch_bounds__(kTPB) fb_find(ObsArgs a) {
    const uint32_t p = blockIdx.x * kTPB + threadIdx.x;
    if (p >= a.n) return;
    const uint32_t req = a.order[p];
    a.headpos[p] = 0;
    if (!consents(a, req)) return;
    const uint64_t hi = a.key_hi[req], lo = a.key_lo[req];
    if (run_prev(a, p, hi, lo) != kNone) return;   // not a head
    const Claim c = find_or_claim(a.t, hi, lo);
    uint32_t status = kNew;
    if (c.slot == kNone) atomicOr(a.err, 1u);
    else {
        FbSlot* s = fb_slot(a.t, c.slot);
        uint64_t now = a.now;
        if constexpr (kTimed) now = a.when[p];
        if (c.fresh) { s->key_hi = hi; s->key_lo = lo; s->epoch = 0; s->count = 0; s->n_model = 0; }
        else status = idle_or_old(now, s->epoch, a.idle) ? kIdle : kLive;
    }
    a.slot_of[p] = c.slot; a.status[p] = status; a.headpos[p] = p;
}

// One lane group per request; timed, a request inside a run first tests its predecessor's time and counts a break as idle_expired.
// No lane leaves early and the round count is the same across the wave: the ballots need all 64 lanes.  Dynamic LDS: one u32 per bin.
template <bool kTimed>
__global__ void __launch_bounds__(kTPB) fb_rank(ObsArgs a) {
    extern __shared__ uint32_t bins[];
    const uint32_t n_bins = kHist + 2u * (a.row_cap + 1u);
    for (uint32_t i = threadIdx.x; i < n_bins; i += kTPB) bins[i] = 0;
    __syncthreads();
    const uint32_t lanes = 1u << a.lanes_shift, lane = threadIdx.x & (lanes - 1);
    const uint32_t gbase = (threadIdx.x & 63u) & ~(lanes - 1);   // the group's first lane in the wave
    const uint32_t gmask = (1u << lanes) - 1u;                   // lanes <= 16
    // the grid is capped (kRankBlocks): a workgroup takes the positions g, g + groups, ... and flushes its histogram once.  Every group makes the same number of trips
    const uint64_t groups = (uint64_t)gridDim.x * (kTPB >> a.lanes_shift);
    const uint32_t trips = (uint32_t)((a.n + groups - 1) / groups);
    for (uint32_t trip = 0; trip < trips; ++trip) {
        const uint64_t p = trip * groups + (uint64_t)blockIdx.x * (kTPB >> a.lanes_shift) + (threadIdx.x >> a.lanes_shift);
        uint32_t kind = kRequests;                                   // (no request: nothing is counted)
        uint32_t req = 0, c = 0, n_model = 0;                        // c = 0: no position is ever read
        const uint64_t* row = nullptr; const uint64_t* sc = nullptr;
        uint64_t item = 0;
        if (p < a.n) {
            req = a.order[p];
            if (!consents(a, req)) kind = kNoConsent;
            else {
                const uint64_t hi = a.key_hi[req], lo = a.key_lo[req];
                item = a.item[req];
                const uint32_t pr = run_prev(a, (uint32_t)p, hi, lo);
                if (pr == kNone) {   // a run head
                    const uint32_t st = a.status[p], slot = a.slot_of[p];
                    kind = st == kLive ? kObserved : st == kIdle ? kIdleExpired : kFirstSeen;
                    if (st == kLive && slot != kNone) { FbSlot* s = fb_slot(a.t, slot); c = min(s->count, a.row_cap); n_model = s->n_model; row = fb_ids(s); }
                } else if (kTimed && idle_or_old(a.when[p], a.when[p - 1], a.idle)) {   // (kTimed is a constant: the untimed form holds no trace of this)
                    kind = kIdleExpired;                             // a break: the predecessor's row is idle by the time of this click
                } else {   // the row served to the previous request of the run
                    kind = kObserved;
                    c = served_count(a, pr); n_model = c;
                    row = a.ids + (size_t)pr * a.how_many;
                    if (a.scores) sc = a.scores + (size_t)pr * a.how_many;
                }
            }
        }
        uint32_t found = 0, fin = 0;                                 // the same in every lane of the group
        for (uint32_t r = 0; r < a.rounds; ++r) {
            const uint32_t i = (r << a.lanes_shift) + lane;
            const bool in = i < c;
            const bool match = in && row[i] == item;
            const bool finite = in && sc && finite_bits(sc[i]);
            const uint32_t mm = (uint32_t)(__ballot(match) >> gbase) & gmask, mf = (uint32_t)(__ballot(finite) >> gbase) & gmask;
            if (!found && mm) found = (r << a.lanes_shift) + (uint32_t)__ffs((int)mm);
            fin += __popc(mf);
        }
        if (sc) n_model = fin;
        if (kind != kRequests && lane == 0) {
            uint32_t rank = SRN_FEEDBACK_NONE;
            atomicAdd(&bins[kRequests], 1u);
            atomicAdd(&bins[kind], 1u);
            if (kind != kNoConsent) atomicAdd(&bins[kStored], 1u);
            if (kind == kObserved) {
                const bool filled = found > n_model;
                rank = found | (filled ? SRN_FEEDBACK_FILLED : 0u);
                if (found) { atomicAdd(&bins[filled ? kHitsFilled : kHitsModel], 1u); atomicAdd(&bins[kHist + (filled ? a.row_cap + 1u : 0u) + found], 1u); }   // found <= c <= row_cap
            }
            if (a.out_rank) a.out_rank[req] = rank;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_bins; i += kTPB) { const uint32_t v = bins[i]; if (v) atomicAdd(&a.ctr[i], (unsigned long long)v); }
}

// the run's last request writes the row it was served, with `now` or (timed) its own time: the same lane groups, lane l the positions l, l + lanes, ...
template <bool kTimed>
__global__ void __launch_bounds__(kTPB) fb_store(ObsArgs a) {
    const uint64_t tid = (uint64_t)blockIdx.x * kTPB + threadIdx.x;
    const uint64_t p = tid >> a.lanes_shift;
    const uint32_t lanes = 1u << a.lanes_shift, lane = (uint32_t)tid & (lanes - 1);
    const uint32_t gbase = (threadIdx.x & 63u) & ~(lanes - 1), gmask = (1u << lanes) - 1u;
    FbSlot* s = nullptr;
    uint32_t c = 0;
    const uint64_t* row = nullptr; const uint64_t* sc = nullptr;
    if (p < a.n) {
        const uint32_t req = a.order[p];
        const bool last = consents(a, req) && run_last(a, (uint32_t)p, req);
        const uint32_t slot = last ? a.slot_of[a.run_start[p]] : kNone;
        if (slot != kNone) {
            s = fb_slot(a.t, slot);
            c = served_count(a, req);                            // <= how_many <= row_cap
            row = a.ids + (size_t)req * a.how_many;
            if (a.scores) sc = a.scores + (size_t)req * a.how_many;
        }
    }
    uint64_t* dst = s ? fb_ids(s) : nullptr;
    uint32_t fin = 0;
    for (uint32_t r = 0; r < a.rounds; ++r) {
        const uint32_t i = (r << a.lanes_shift) + lane;
        const bool in = i < c;
        if (in) dst[i] = row[i];
        const bool finite = in && sc && finite_bits(sc[i]);
        fin += __popc((uint32_t)(__ballot(finite) >> gbase) & gmask);
    }
    if (s && lane == 0) {
        uint64_t now = a.now;
        if constexpr (kTimed) now = a.when[p];
        s->count = c; s->n_model = sc ? fin : c; s->epoch = now; s->state = kFull;
    }
}

// ---- the visitor-clustered bootstrap of the counters, behind fb_rank: replicate b weighs every observed request of a visitor with
// w(seed, b, key) = boot_weight(boot_replicate_key(seed, b), boot_fold(key)) and keeps the weighted observed count and both weighted histograms as exact integers ----
constexpr uint32_t kBootBlocks = 512;           // fb_boot's grid.x at the most: a (word, replicate) takes at most 512 global atomics per call
constexpr uint32_t kBootStage = 128;            // sorted positions staged in LDS at a time
constexpr uint32_t kBootWide = 256, kBootNarrow = 64, kBootWideRows = 31;   // replicates per workgroup: 2 * row_cap columns of u32 per lane plus the stage stay within 64 KiB
uint32_t boot_tile(uint64_t row_cap) { return row_cap <= kBootWideRows ? kBootWide : kBootNarrow; }
size_t boot_lds_bytes(uint64_t row_cap) { return (size_t)2 * row_cap * boot_tile(row_cap) * 4 + (size_t)kBootStage * 12; }
static_assert(2 * kBootWideRows * kBootWide * 4 + kBootStage * 12 <= 65536 && 2 * SRN_FEEDBACK_BOOTSTRAP_MAX_ROW_CAP * kBootNarrow * 4 + kBootStage * 12 <= 65536, "fb_boot's LDS");

struct BootArgs {
    const uint64_t* key_hi; const uint64_t* key_lo;
    const uint32_t* order;   // [n] request index of each sorted position: the observed requests of one visitor are adjacent
    const uint32_t* rank;    // [n] by request index, as fb_rank left it
    uint32_t n, row_cap, replicates;
    uint64_t seed;
    unsigned long long* words;
};
// One lane per replicate, blockDim.x replicates per workgroup (blockIdx.y: the tile).  A workgroup takes every gridDim.x-th stage of kBootStage sorted positions: it
// puts (fold(key), rank) of the stage into LDS, then every lane walks the stage -- all lanes at the same position, the staged words read through readfirstlane, so
// every branch is wave-uniform.  The weight is computed where the folded key changes and never carried from one stage to the next.  A hit goes to the lane's own
// column bins[bin][lane] (no two lanes share a word: plain adds), observed_w stays in a register; one 64-bit global atomic per non-zero (word, replicate) at the end.
// A workgroup's sums stay below 12 * 2^24 (kMaxBatch): u32 is enough.
__global__ void __launch_bounds__(kBootWide) fb_boot(BootArgs a) {
    extern __shared__ __align__(16) uint32_t boot_lds[];
    const uint32_t tile = blockDim.x, lane = threadIdx.x, n_bins = 2u * a.row_cap;
    uint32_t* bins = boot_lds;                                        // [n_bins][tile]
    uint64_t* s_fold = (uint64_t*)(boot_lds + (size_t)n_bins * tile);  // [kBootStage]   (n_bins * tile * 4 is a multiple of 8)
    uint32_t* s_rank = (uint32_t*)(s_fold + kBootStage);              // [kBootStage]
    for (uint32_t i = 0; i < n_bins; ++i) bins[i * tile + lane] = 0;
    const uint32_t b = blockIdx.y * tile + lane;                      // (b >= replicates: the lane walks along and adds nothing to memory)
    const uint64_t key = boot_replicate_key(a.seed, b);
    uint32_t obs = 0;
    const uint32_t n_stages = (a.n + kBootStage - 1) / kBootStage;
    for (uint32_t stage = blockIdx.x; stage < n_stages; stage += gridDim.x) {
        const uint32_t p0 = stage * kBootStage, cnt = min(kBootStage, a.n - p0);
        __syncthreads();                                              // the previous stage has been walked by every wave
        for (uint32_t i = lane; i < cnt; i += tile) {
            const uint32_t req = a.order[p0 + i], r = a.rank[req];
            s_rank[i] = r;
            if (r != SRN_FEEDBACK_NONE) s_fold[i] = boot_fold(a.key_hi[req], a.key_lo[req]);
        }
        __syncthreads();
        uint64_t prev = 0; bool have = false; uint32_t w = 0;         // (have: no folded key is reserved as "none")
        for (uint32_t q = 0; q < cnt; ++q) {
            const uint32_t rk = __builtin_amdgcn_readfirstlane(s_rank[q]);
            if (rk == SRN_FEEDBACK_NONE) continue;                    // not observed: adds nothing
            const uint32_t* fw = (const uint32_t*)(s_fold + q);
            const uint32_t f_lo = __builtin_amdgcn_readfirstlane(fw[0]), f_hi = __builtin_amdgcn_readfirstlane(fw[1]);   // (the builtin gives an int: no sign extension)
            const uint64_t fold = (uint64_t)f_lo | ((uint64_t)f_hi << 32);
            if (!have || fold != prev) { w = boot_weight(key, fold); prev = fold; have = true; }
            obs += w;
            const uint32_t r = rk & ~SRN_FEEDBACK_FILLED;
            if (r != 0 && r <= a.row_cap) bins[(((rk & SRN_FEEDBACK_FILLED) ? a.row_cap : 0u) + r - 1u) * tile + lane] += w;
        }
    }
    if (b >= a.replicates) return;                                    // (behind the last barrier)
    if (obs) atomicAdd(&a.words[b], (unsigned long long)obs);
    for (uint32_t i = 0; i < n_bins; ++i) { const uint32_t v = bins[i * tile + lane]; if (v) atomicAdd(&a.words[(size_t)(1 + i) * a.replicates + b], (unsigned long long)v); }
}

// the log's payload for the table's rebuild and one-key read-back: out[0] = count, out[2] = n_model, out[3..] = ids
struct FbPayload {
    using Head = FbSlot;
    uint32_t row_cap;
    __device__ void copy(const FbSlot* s, FbSlot* d) const {
        const uint32_t c = min(s->count, row_cap);
        d->count = c; d->n_model = s->n_model;
        for (uint32_t j = 0; j < c; ++j) fb_ids(d)[j] = fb_ids(const_cast<FbSlot*>(s))[j];
    }
    __device__ void read(const FbSlot* s, uint64_t* out) const {
        const uint32_t c = min(s->count, row_cap);
        out[0] = c; out[2] = s->n_model;
        for (uint32_t i = 0; i < c; ++i) out[3 + i] = fb_ids(const_cast<FbSlot*>(s))[i];
    }
};

// The entries not older than the TTL into a second table, allocated here; the first one is freed (own stream, mu held, behind `last`; blocks).  A failure leaves the log as it was.
int rebuild(srn_feedback* f, uint64_t now) {
    const size_t bytes = (size_t)f->n_slots * f->stride;
    char* nt = nullptr;
    if (hipMalloc((void**)&nt, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(SRN_ENOMEM, "click feedback log: no device memory for the sweep's second table"); }
    Table to = f->tab(); to.base = nt;
    hipError_t e = rebuild_into(f, to, now, FbPayload{(uint32_t)f->row_cap});
    if (e == hipSuccess) e = hipStreamSynchronize(f->own);
    if (e != hipSuccess) { (void)hipFree(nt); return fail(SRN_EHIP, std::string("click feedback log (sweep): ") + hipGetErrorString(e)); }
    (void)hipFree(f->table);
    f->table = nt; ++f->sweeps;
    return SRN_OK;
}
// the capacity rule (srn_visitor_table.h) with the log's rebuild; the log never grows (mu held)
int room_for(srn_feedback* f, uint64_t n, uint64_t now) { return make_room(f, n, now, [f](uint64_t at) { return rebuild(f, at); }, never_grows); }
}  // namespace

void fb_free(srn_feedback* f) {
    if (!f) return;
    table_release(f);
    for (void* p : {(void*)f->ctr, (void*)f->boot}) if (p) (void)hipFree(p);
    delete f;
}

int fb_create(int device, size_t capacity, size_t row_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_feedback** out) {
    if (!out) return fail(SRN_EINVAL, "srn_feedback_create: null output");
    *out = nullptr;
    if (row_cap == 0) return fail(SRN_EINVAL, "srn_feedback_create: row_cap must be > 0");
    if (row_cap > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "srn_feedback_create: row_cap above SRN_MAX_HOW_MANY");
    srn_feedback* f = new srn_feedback();
    struct Guard { srn_feedback*& f; ~Guard() { if (f) fb_free(f); } } guard{f};
    f->row_cap = row_cap;
    const int rc = table_create(f, "srn_feedback_create", "click feedback log", device, capacity, ttl_secs, idle_secs, kFbHead, row_cap, 3 + SRN_MAX_HOW_MANY);
    if (rc) return rc;
    const size_t bytes = (size_t)f->n_slots * f->stride;
    if (hipMalloc((void**)&f->table, bytes) != hipSuccess) { (void)hipGetLastError(); f->table = nullptr; return fail(SRN_ENOMEM, "srn_feedback_create: no device memory for the table"); }
    HIP_TRY(hipMalloc((void**)&f->ctr, 8 * (size_t)f->n_bins()));
    HIP_TRY(hipMemsetAsync(f->table, 0, bytes, f->own));
    HIP_TRY(hipMemsetAsync(f->ctr, 0, 8 * (size_t)f->n_bins(), f->own));
    HIP_TRY(hipStreamSynchronize(f->own));
    *out = f; f = nullptr;
    return SRN_OK;
}

void fb_shape(const srn_feedback* f, int* device, uint64_t* row_cap) { *device = f->device; *row_cap = f->row_cap; }

// the checks both entry points make, in their order; *done: nothing to do (n == 0)
static int check_observe(const srn_feedback* f, const VisitorBatch& r, const ObserveCall& c, bool* done) {
    *done = false;
    if (!f) return fail(SRN_EINVAL, "srn_feedback_observe: null log");
    if (r.n == 0) { *done = true; return SRN_OK; }
    if (!has_request_arrays(r, false) || !c.ids || !c.counts) return fail(SRN_EINVAL, "srn_feedback_observe: null buffer");
    if (r.n > kMaxBatch) return fail(SRN_ERANGE, "srn_feedback_observe: more than 2^24 requests in one call");
    if (c.how_many == 0) return fail(SRN_EINVAL, "srn_feedback_observe: how_many must be > 0");
    if (c.how_many > f->row_cap) return fail(SRN_ERANGE, "srn_feedback_observe: how_many above the log's row_cap");
    return SRN_OK;
}

int fb_observe_device(srn_feedback* f, const VisitorBatch& r, const ObserveCall& c) {
    bool done;
    int rc = check_observe(f, r, c, &done); if (rc || done) return rc;
    const size_t n = r.n;
    hipStream_t st = (hipStream_t)c.stream;
    const uint64_t now = r.now_secs ? r.now_secs : wall_secs();
    std::lock_guard<std::mutex> g(f->mu);
    if ((rc = room_for(f, n, now))) return rc;
    HIP_TRY(hipSetDevice(f->device));
    // scratch: the sorted front's (sort keys and indices, rocPRIM's temporary storage -- also the scan's -- and a timed batch's times), then the per-position words
    size_t scan = 0;
    HIP_TRY(rocprim::inclusive_scan(nullptr, scan, (uint32_t*)nullptr, (uint32_t*)nullptr, n, rocprim::maximum<uint32_t>(), st));
    Bump b; SortedFront front;
    if ((rc = front.plan(b, r, st, scan))) return rc;
    const auto slot_of = b.of<uint32_t>(n), status = b.of<uint32_t>(n), headpos = b.of<uint32_t>(n), run_start = b.of<uint32_t>(n);
    Bump::Region<uint32_t> rank;
    if (f->boot && !c.out_rank) rank = b.of<uint32_t>(n);   // (the bootstrap reads the ranks; the caller gave no buffer for them)
    if ((rc = grow_behind(f->last, &f->ws, &f->ws_bytes, b.bytes))) return rc;
    HIP_TRY(hipStreamWaitEvent(st, f->last, 0));
    char* const ws = f->ws;
    if ((rc = front.run(ws, r, st))) return rc;
    ObsArgs a{};
    a.t = f->tab(); a.key_hi = r.key_hi; a.key_lo = r.key_lo; a.item = r.item; a.consent = r.consent;
    a.ids = c.ids; a.scores = (const uint64_t*)c.scores; a.counts = c.counts; a.how_many = (uint32_t)c.how_many;
    a.order = front.order; a.n = (uint32_t)n; a.row_cap = (uint32_t)f->row_cap;
    a.lanes_shift = f->row_cap <= 8 ? 3 : 4;
    a.rounds = (uint32_t)((f->row_cap + (1u << a.lanes_shift) - 1) >> a.lanes_shift);
    a.now = now; a.idle = f->idle;
    a.slot_of = slot_of.at(ws); a.status = status.at(ws); a.headpos = headpos.at(ws); a.run_start = run_start.at(ws);
    a.out_rank = c.out_rank ? c.out_rank : rank.at(ws); a.ctr = f->ctr; a.err = f->err();
    a.when = front.when;   // a timed batch: the same sequence behind the front's gather of the times into sorted order
    const dim3 gn = grid_for(n), gg = grid_for(n << a.lanes_shift);   // (n <= 2^24: 2^28 lanes at the most)
    hipError_t scanned = hipSuccess;
    by_timed(r, [&](auto t) {
        constexpr bool kTimed = decltype(t)::value;
        fb_find<kTimed><<<gn, kTPB, 0, st>>>(a);
        size_t t1 = front.tmp_bytes;
        scanned = rocprim::inclusive_scan(front.tmp, t1, a.headpos, a.run_start, n, rocprim::maximum<uint32_t>(), st);
        if (scanned != hipSuccess) return;
        fb_rank<kTimed><<<dim3(std::min<unsigned>(gg.x, kRankBlocks)), kTPB, 4 * (size_t)f->n_bins(), st>>>(a);
        fb_store<kTimed><<<gg, kTPB, 0, st>>>(a);
    });
    HIP_TRY(scanned);
    if (f->boot) {   // the replicate words, from the ranks fb_rank wrote
        const BootArgs ba{r.key_hi, r.key_lo, a.order, a.out_rank, a.n, (uint32_t)f->row_cap, f->boot_b, f->boot_seed, f->boot};
        const uint32_t tile = boot_tile(f->row_cap);
        fb_boot<<<dim3(std::min<unsigned>((a.n + kBootStage - 1) / kBootStage, kBootBlocks), (f->boot_b + tile - 1) / tile), tile, boot_lds_bytes(f->row_cap), st>>>(ba);
    }
    HIP_TRY(hipGetLastError());
    // from here on the log has changed: the next call is ordered behind this one
    f->bound += n;
    HIP_TRY(hipEventRecord(f->last, st));
    return SRN_OK;
}

int fb_observe_host(srn_feedback* f, const VisitorBatch& r, const ObserveCall& c) {
    bool done;
    int rc = check_observe(f, r, c, &done); if (rc || done) return rc;
    HIP_TRY(hipSetDevice(f->device));
    const size_t n = r.n, rows = n * c.how_many;
    Bump b; StagedBatch in;
    in.plan(b, r);
    const auto ids = b.of<uint64_t>(rows); const auto scores = b.of<double>(rows); const auto counts = b.of<uint32_t>(n), rank = b.of<uint32_t>(n);
    StageBuf buf; if ((rc = buf.alloc(b.bytes, "srn_feedback_observe"))) return rc;
    char* const base = buf.p;
    hipStream_t st = nullptr;   // a stream of this call's own: two host callers do not wait for each other's copies
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    auto run = [&]() -> int {
        VisitorBatch dr;
        int rc2 = in.upload(base, r, st, &dr); if (rc2) return rc2;
        HIP_TRY(hipMemcpyAsync(ids.at(base), c.ids, rows * 8, hipMemcpyHostToDevice, st));
        if (c.scores) HIP_TRY(hipMemcpyAsync(scores.at(base), c.scores, rows * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(counts.at(base), c.counts, n * 4, hipMemcpyHostToDevice, st));
        if ((rc2 = fb_observe_device(f, dr, ObserveCall{ids.at(base), c.scores ? scores.at(base) : nullptr, counts.at(base), c.how_many, rank.at(base), st}))) return rc2;
        if (c.out_rank) HIP_TRY(hipMemcpyAsync(c.out_rank, rank.at(base), n * 4, hipMemcpyDeviceToHost, st));
        return SRN_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(st);
    (void)hipStreamDestroy(st);
    if (rc == SRN_OK && e != hipSuccess) return fail(SRN_EHIP, std::string("hipStreamSynchronize(st): ") + hipGetErrorString(e));
    return rc;
}

int fb_stats(srn_feedback* f, srn_feedback_stats_t* out) {
    if (!f || !out) return fail(SRN_EINVAL, "srn_feedback_stats: null argument");
    std::lock_guard<std::mutex> g(f->mu);
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipEventSynchronize(f->last));
    unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(c, f->ctr, sizeof(c), hipMemcpyDeviceToHost));
    *out = srn_feedback_stats_t{f->capacity, f->n_slots, f->row_cap, f->stride, f->bound, f->sweeps, f->refused, f->ttl, f->idle,
                                c[kRequests], c[kNoConsent], c[kFirstSeen], c[kIdleExpired], c[kObserved], c[kHitsModel], c[kHitsFilled], c[kStored]};
    return check_err(f);
}

int fb_histogram(srn_feedback* f, uint64_t* hits_model, uint64_t* hits_filled, size_t cap) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_histogram: null log");
    if (cap < f->row_cap + 1) return fail(SRN_ERANGE, "srn_feedback_histogram: fewer than row_cap + 1 entries per array");
    std::lock_guard<std::mutex> g(f->mu);
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipEventSynchronize(f->last));
    const size_t bins = f->row_cap + 1;
    std::vector<unsigned long long> h(2 * bins);
    HIP_TRY(hipMemcpy(h.data(), f->ctr + kHist, h.size() * 8, hipMemcpyDeviceToHost));
    for (size_t r = 0; r < cap; ++r) {
        if (hits_model) hits_model[r] = r < bins ? h[r] : 0;
        if (hits_filled) hits_filled[r] = r < bins ? h[bins + r] : 0;
    }
    return SRN_OK;
}

int fb_reset_counters(srn_feedback* f) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_reset_counters: null log");
    std::lock_guard<std::mutex> g(f->mu);
    int rc = own_after_last(f); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(f->ctr, 0, 8 * (size_t)f->n_bins(), f->own));
    if (f->boot) HIP_TRY(hipMemsetAsync(f->boot, 0, 8 * f->boot_words(), f->own));
    HIP_TRY(hipStreamSynchronize(f->own));
    return SRN_OK;
}

int fb_boot_enable(srn_feedback* f, uint32_t replicates, uint64_t seed) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_bootstrap_enable: null log");
    if (replicates == 0) return fail(SRN_EINVAL, "srn_feedback_bootstrap_enable: replicates must be > 0");
    if (replicates > SRN_MAX_BOOTSTRAP) return fail(SRN_ERANGE, "srn_feedback_bootstrap_enable: replicates above SRN_MAX_BOOTSTRAP");
    if (f->row_cap > SRN_FEEDBACK_BOOTSTRAP_MAX_ROW_CAP) return fail(SRN_ERANGE, "srn_feedback_bootstrap_enable: the log's row_cap is above 64");
    std::lock_guard<std::mutex> g(f->mu);
    if (f->boot) return fail(SRN_ESTATE, "srn_feedback_bootstrap_enable: the bootstrap is already enabled (disable it first)");
    int rc = own_after_last(f); if (rc) return rc;
    const size_t bytes = 8 * (size_t)(1 + 2 * f->row_cap) * replicates;
    unsigned long long* words = nullptr;
    if (hipMalloc((void**)&words, bytes) != hipSuccess) { (void)hipGetLastError(); return fail(SRN_ENOMEM, "srn_feedback_bootstrap_enable: no device memory for the replicate words"); }
    hipError_t e = hipMemsetAsync(words, 0, bytes, f->own);
    if (e == hipSuccess) e = hipStreamSynchronize(f->own);
    if (e != hipSuccess) { (void)hipFree(words); return fail(SRN_EHIP, std::string("srn_feedback_bootstrap_enable: ") + hipGetErrorString(e)); }
    f->boot = words; f->boot_b = replicates; f->boot_seed = seed;
    return SRN_OK;
}

int fb_boot_disable(srn_feedback* f) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_bootstrap_disable: null log");
    std::lock_guard<std::mutex> g(f->mu);
    if (!f->boot) return SRN_OK;
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipEventSynchronize(f->last));   // (the previous call may still add to the words)
    (void)hipFree(f->boot);
    f->boot = nullptr; f->boot_b = 0; f->boot_seed = 0;
    return SRN_OK;
}

int fb_boot_info(srn_feedback* f, uint32_t* replicates, uint64_t* seed) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_bootstrap_info: null log");
    std::lock_guard<std::mutex> g(f->mu);
    if (replicates) *replicates = f->boot_b;
    if (seed) *seed = f->boot_seed;
    return SRN_OK;
}

int fb_boot_read(srn_feedback* f, uint64_t* observed, uint64_t* hits_model, uint64_t* hits_filled, size_t replicates_cap, size_t rank_cap) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_bootstrap_read: null log");
    std::lock_guard<std::mutex> g(f->mu);
    if (!f->boot) return fail(SRN_ESTATE, "srn_feedback_bootstrap_read: the bootstrap is not enabled");
    if (replicates_cap < f->boot_b) return fail(SRN_ERANGE, "srn_feedback_bootstrap_read: fewer than `replicates` entries per array");
    if (rank_cap < f->row_cap + 1) return fail(SRN_ERANGE, "srn_feedback_bootstrap_read: fewer than row_cap + 1 entries per replicate");
    HIP_TRY(hipSetDevice(f->device));
    HIP_TRY(hipEventSynchronize(f->last));
    std::vector<unsigned long long> h(f->boot_words());
    HIP_TRY(hipMemcpy(h.data(), f->boot, h.size() * 8, hipMemcpyDeviceToHost));
    const size_t B = f->boot_b, R = f->row_cap;
    for (size_t b = 0; b < B; ++b) {
        if (observed) observed[b] = h[b];
        for (size_t r = 0; r < rank_cap; ++r) {   // [0] is unused; entries beyond row_cap are written as 0
            const bool in = r >= 1 && r <= R;
            if (hits_model) hits_model[b * rank_cap + r] = in ? h[r * B + b] : 0;
            if (hits_filled) hits_filled[b * rank_cap + r] = in ? h[(R + r) * B + b] : 0;
        }
    }
    return SRN_OK;
}

void fb_boot_weights_host(uint64_t seed, uint32_t replicate, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out) {
    const uint64_t key = boot_replicate_key(seed, replicate);
    for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)boot_weight(key, boot_fold(key_hi[i], key_lo[i]));
}

int fb_sweep(srn_feedback* f, uint64_t now_secs, uint64_t* n_live) {
    if (!f) return fail(SRN_EINVAL, "srn_feedback_sweep: null log");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(f->mu);
    return sweep(f, now, [f](uint64_t at) { return rebuild(f, at); }, n_live);
}

int fb_get(srn_feedback* f, uint64_t hi, uint64_t lo, uint64_t now_secs, uint64_t* out_ids, size_t cap, uint32_t* out_count, uint32_t* out_n_model, uint64_t* out_epoch) {
    if (!f || !out_count || (cap && !out_ids)) return fail(SRN_EINVAL, "srn_feedback_get: null argument");
    const uint64_t now = now_secs ? now_secs : wall_secs();
    std::lock_guard<std::mutex> g(f->mu);
    *out_count = SRN_FEEDBACK_NONE;
    if (out_n_model) *out_n_model = 0;
    if (out_epoch) *out_epoch = 0;
    std::vector<uint64_t> h; bool found = false;
    const int rc = read_one(f, hi, lo, now, FbPayload{(uint32_t)f->row_cap}, 3 + f->row_cap, &h, &found);
    if (rc || !found) return rc;
    if (h[0] > cap) return fail(SRN_ERANGE, "srn_feedback_get: output buffer too small");
    if (h[0]) std::memcpy(out_ids, h.data() + 3, h[0] * 8);
    *out_count = (uint32_t)h[0];
    if (out_n_model) *out_n_model = (uint32_t)h[2];
    if (out_epoch) *out_epoch = h[1];
    return SRN_OK;
}

}  // namespace srn
