// =====================================================================================
// Device runtime of libserenade_hip.so: index upload (row slots laid out on the device), per-call workspaces (own stream,
// staging buffers, event ring), LDS geometry of a launch, the batch launch sequence (predict_core behind the device_predict_* entries: plan, reserve, enqueue), the item-sharded pipeline's stages,
// timing and debug counters.  The latency paths live in srn_latency.hip, the kernels in srn_kernels.hip and srn_fast.hip.
// =====================================================================================
#include <hip/hip_runtime.h>

#include <chrono>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "srn_runtime.h"
#include "srn_hipsync.h"

namespace srn {

static Knobs g_knobs; static std::once_flag g_knobs_once; static std::mutex g_knobs_mu;
// Each variable is read once: a flag is on when the variable is set at all, a switch holds a number (0 = off), an int is clamped to [lo, hi].
static bool env_flag(const char* name) { return getenv(name) != nullptr; }
static int env_int(const char* name, int unset, int lo = INT_MIN, int hi = INT_MAX) { const char* e = getenv(name); return e ? std::min(hi, std::max(lo, atoi(e))) : unset; }
static void knobs_read() {
    Knobs k;
    k.fast_how_many_max = env_int("SRN_FAST_HOW_MANY_MAX", k.fast_how_many_max, 1, 64);
    k.no_masks = env_flag("SRN_NO_MASKS"); k.no_viol = env_flag("SRN_NO_VIOL"); k.no_merge = env_flag("SRN_NO_MERGE");
    k.no_fast = env_flag("SRN_NO_FAST"); k.no_mid = env_flag("SRN_NO_MID"); k.no_big = env_flag("SRN_NO_BIG"); k.no_long = env_flag("SRN_NO_LONG"); k.debug = env_flag("SRN_DEBUG");
    const int row_slots = env_int("SRN_ROW_SLOTS", -1); k.row_slots16 = row_slots == 16 ? 1 : row_slots == 64 ? 0 : -1;
    k.hot_slots = env_int("SRN_HOT_SLOTS", k.hot_slots, 0);
    k.sketch_slots = env_int("SRN_SKETCH_SLOTS", k.sketch_slots, 0);
    k.lds_budget_kb = env_int("SRN_LDS_BUDGET_KB", k.lds_budget_kb, 0);
    const int grid_mult = env_int("SRN_GRID_MULT", 0, 1); k.grid_mult_set = grid_mult != 0; if (grid_mult) k.grid_mult = grid_mult;
    k.host_chunks = env_int("SRN_HOST_CHUNKS", k.host_chunks, 0);
    k.copy_slices = env_int("SRN_COPY_SLICES", k.copy_slices, 0);
    k.host_trace = env_flag("SRN_HOST_TRACE"); k.timing = env_int("SRN_TIMING", 0) != 0;
    k.tiny_max = env_int("SRN_TINY_MAX", k.tiny_max, 0);
    k.no_tiny_fused = env_int("SRN_TINY_FUSED", 1) == 0;
    k.tiny_fused_max = env_int("SRN_TINY_FUSED_MAX", k.tiny_fused_max, 1, 256);
    k.no_tiny_spin = env_int("SRN_TINY_SPIN", 1) == 0;
    k.tiny_fast = env_int("SRN_TINY_FAST", k.tiny_fast, 0, 3);
    k.lanes = env_int("SRN_PREDICT_LANES", k.lanes, 0);
    k.order_min = env_int("SRN_ORDER_MIN", k.order_min, 0);
    k.light_min = env_int("SRN_LIGHT_MIN", k.light_min, 0);
    k.no_dedup = env_flag("SRN_NO_DEDUP"); k.dedup_hash_bits = env_int("SRN_DEDUP_HASH_BITS", 0, 0, 32);
    k.cache_hash_bits = env_int("SRN_CACHE_HASH_BITS", 0, 0, 32);
    k.no_sback_second = env_flag("SRN_NO_SBACK_SECOND");
    k.no_sback = env_flag("SRN_NO_SBACK");
    const int stream = env_int("SRN_SBACK_STREAM", INT_MIN); k.sback_stream_mode = stream == INT_MIN ? -1 : stream != 0 ? 1 : 0;
    k.no_sback_stream = k.sback_stream_mode == 0;
    if (const char* e = getenv("SRN_XGMI_GBPS")) { const double v = atof(e); if (v > 0.0) k.xgmi_gbps = v; }
    k.sback_min_shards = env_int("SRN_SBACK_MIN_SHARDS", k.sback_min_shards, 2);
    k.fast_runs = env_int("SRN_FAST_RUNS", 0) == 3 ? 3 : 0;   // tests: the fast kernel's 29-bit-rank form (3 lists per query) on a small index
    std::lock_guard<std::mutex> lk(g_knobs_mu); g_knobs = k;
}
Knobs knobs() { std::call_once(g_knobs_once, knobs_read); std::lock_guard<std::mutex> lk(g_knobs_mu); return g_knobs; }
int knob_predict_lanes() { return knobs().lanes; }
size_t knob_tiny_max() { return (size_t)std::max(1, knobs().tiny_max); }
void reload_knobs() { std::call_once(g_knobs_once, knobs_read); knobs_read(); ingest_reload_knobs(); split_reload_knobs(); }

namespace {
template <typename T> const T* upload(DeviceState* d, const std::vector<T>& v, bool& ok, size_t pad = 0, size_t = 0) {   // (hipMalloc is 256-byte aligned)
    void* p = nullptr; const size_t n = std::max<size_t>(v.size() * sizeof(T), 16) + pad;
    if (!ok) return nullptr;
    if (hipMalloc(&p, n) != hipSuccess) { ok = false; set_error("hipMalloc failed for index array"); return nullptr; }
    d->allocs.push_back(p); d->bytes += n;
    if (!v.empty() && hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) { ok = false; set_error("hipMemcpy H2D failed"); }
    return (const T*)p;
}
}  // namespace

DeviceState* device_attach(const FlatIndex& ix, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { set_error("no such HIP device"); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice failed"); return nullptr; }
    DeviceState* d = new DeviceState(); d->device = device; d->timing.store(knobs().timing);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) { d->n_cu = prop.multiProcessorCount; d->lds_per_block_max = (int)prop.sharedMemPerBlock; }
    bool ok = true;
    d->di.id_table = upload(d, ix.id_table, ok); d->di.id_mask = ix.id_mask;
    { std::vector<ItemMeta> meta(ix.n_items); std::vector<uint64_t> id_sorted(ix.n_items);
      for (size_t i = 0; i < ix.n_items; ++i) { meta[i] = ItemMeta{ix.idf[i], ix.id_rank[i], ix.attr[i]}; id_sorted[ix.id_rank[i]] = ix.item_id[i]; }
      d->d_meta = (ItemMeta*)upload(d, meta, ok); d->di.meta = d->d_meta; d->di.id_sorted = upload(d, id_sorted, ok);
      std::vector<ItemMeta> ms(512, ItemMeta{0.0, 0u, 0u});   // the fast kernel's threshold sample: one coalesced read per wave
      for (uint32_t w8 = 0; w8 < 8; ++w8) for (uint32_t l = 0; l < 64; ++l) if (8 * l + w8 < ix.n_items) ms[64 * w8 + l] = meta[8 * l + w8];
      d->fast.meta_sample = upload(d, ms, ok); }
    d->di.post_off = upload(d, ix.post_off, ok); d->di.post_rank = upload(d, ix.post_rank, ok);
    d->di.viol = !ix.lists_complete && ix.viol.size() == ix.n_items && ix.n_shards == 1 ? upload(d, ix.viol, ok) : nullptr;   // (a pre-built index whose lists are not all complete: the prep kernel's per-query test)
    if (ok && !ix.postings_only) {   // rows -> 64-byte slots (+ overflow area) on the device, see DeviceIndex and rows_to_slots_kernel
        // item shards: 16-byte FRAGMENT slots (a shard holds ~1/n_shards of a row's items), DeviceIndex::row_frag
        const int rs16 = knobs().row_slots16;
        const bool frag = rs16 >= 0 ? rs16 == 1 : ix.n_shards > 1;   // (SRN_ROW_SLOTS=16|64 forces a form: experiments)
        const uint64_t inl = frag ? 2 : 14;            // items inline in a slot that also carries an overflow offset
        const size_t slot_bytes = frag ? 16 : 64;
        const size_t n = ix.n_kept, nblocks = (n + 1 + 1023) / 1024;
        std::vector<uint32_t> block_base(nblocks);
        uint64_t ext_total = 16;   // ext[0..15] = EMPTY32: what short rows read
        for (size_t b0 = 0; b0 < nblocks; ++b0) {
            block_base[b0] = (uint32_t)ext_total;
            const size_t hi = std::min(n, (b0 + 1) * 1024);
            for (size_t r = b0 * 1024; r < hi; ++r) { const uint64_t len = ix.row_off[r + 1] - ix.row_off[r]; if (len > inl + 1) ext_total += len - inl; }
            if (ext_total >= 0xFFFFFFF0ull) { set_error("row overflow area exceeds 2^32 items"); device_release(d); return nullptr; }
        }
        void *d_off = nullptr, *d_items = nullptr, *d_base = nullptr, *d_slots = nullptr, *d_ext = nullptr;
        const size_t ext_words = ext_total + 16;   // (4-item loads may run past the last row)
        bool good = hipMalloc(&d_off, (n + 1) * 8) == hipSuccess && hipMalloc(&d_items, std::max<size_t>(ix.row_items.size() * 4, 16)) == hipSuccess &&
                    hipMalloc(&d_base, nblocks * 4) == hipSuccess && hipMalloc(&d_slots, (n + 1) * slot_bytes) == hipSuccess && hipMalloc(&d_ext, ext_words * 4) == hipSuccess;
        good = good && hipMemcpy(d_off, ix.row_off.data(), (n + 1) * 8, hipMemcpyHostToDevice) == hipSuccess &&
               (ix.row_items.empty() || hipMemcpy(d_items, ix.row_items.data(), ix.row_items.size() * 4, hipMemcpyHostToDevice) == hipSuccess) &&
               hipMemcpy(d_base, block_base.data(), nblocks * 4, hipMemcpyHostToDevice) == hipSuccess &&
               hipMemset(d_ext, 0xFF, ext_words * 4) == hipSuccess;
        good = good && (frag ? launch_rows_to_frags : launch_rows_to_slots)(nullptr, (const uint64_t*)d_off, (const uint32_t*)d_items, (uint64_t)n, (const uint32_t*)d_base,
                                                                             (uint32_t*)d_slots, (uint32_t*)d_ext) == hipSuccess &&
               hipDeviceSynchronize() == hipSuccess;
        if (good) {   // the fast kernel's rows: 64-byte slots of 16-bit LDS offsets (+ overflow blocks of 8 items); item shards: 16-byte fragment slots, srn_fast.hip
            std::vector<uint32_t> bb(nblocks); uint64_t blocks = 1;   // (block 0: what a stray read finds)
            for (size_t b0 = 0; b0 < nblocks; ++b0) {
                bb[b0] = (uint32_t)blocks;
                const size_t hi = std::min(n, (b0 + 1) * 1024);
                for (size_t r = b0 * 1024; r < hi; ++r) { const uint64_t len = ix.row_off[r + 1] - ix.row_off[r];
                    if (frag) { if (len > 6) blocks += (len - 4 + 7) / 8; } else if (len > 30) blocks += (len - 28 + 7) / 8; }
            }
            void *d_pk = nullptr, *d_e16 = nullptr;
            bool g2 = blocks < 0xFFFFFFF0ull && hipMalloc(&d_pk, (n + 1) * slot_bytes) == hipSuccess && hipMalloc(&d_e16, (blocks + 2) * 16) == hipSuccess &&
                      hipMemcpy(d_base, bb.data(), nblocks * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_e16, 0, (blocks + 2) * 16) == hipSuccess &&
                      launch_rows_to_packed(nullptr, (const uint64_t*)d_off, (const uint32_t*)d_items, (uint64_t)n, (const uint32_t*)d_base, (uint32_t*)d_pk, (uint32_t*)d_e16, frag) == hipSuccess &&
                      hipDeviceSynchronize() == hipSuccess;
            // The packed rows are OPTIONAL (row_packed == nullptr: every query takes the general kernel): they cost another (n + 1) * slot_bytes of HBM
            // next to row_slots, and an index that fits without them must still attach when they do not.
            if (g2) { d->allocs.push_back(d_pk); d->bytes += (n + 1) * slot_bytes; d->allocs.push_back(d_e16); d->bytes += (blocks + 2) * 16;
                      d->fast.row_packed = (const RowQuad*)d_pk; d->fast.row_ext16 = (const uint32_t*)d_e16; }
            else {
                (void)hipGetLastError();   // (clear the sticky allocation error)
                if (d_pk) hipFree(d_pk); if (d_e16) hipFree(d_e16);
                d->fast.row_packed = nullptr; d->fast.row_ext16 = nullptr;
                if (knobs().debug) fprintf(stderr, "[srn] no room for the fast kernel's packed rows (%zu bytes): general kernel only\n", (size_t)((n + 1) * slot_bytes + (blocks + 2) * 16));
            }
        }
        if (good && frag && ix.n_shards >= (uint32_t)knobs().sback_min_shards) {   // the wave-per-query back end's rows (srn_sback.hip): 8-byte slots + overflow blocks; optional like the packed rows
            std::vector<uint32_t> bb(nblocks); uint64_t blocks = 1, longest = 0;
            for (size_t b0 = 0; b0 < nblocks; ++b0) {
                bb[b0] = (uint32_t)blocks;
                const size_t hi = std::min(n, (b0 + 1) * 1024);
                for (size_t r = b0 * 1024; r < hi; ++r) { const uint64_t len = ix.row_off[r + 1] - ix.row_off[r]; longest = std::max(longest, len); if (len > 4) blocks += (len + 7) / 8; }
            }
            void *d_f8 = nullptr, *d_e8 = nullptr, *d_sm = nullptr;
            std::vector<ItemMeta> sm(256, ItemMeta{0.0, 0u, 0u});
            for (size_t i = 0; i < std::min<size_t>(256, ix.n_items); ++i) sm[i] = ItemMeta{ix.idf[i], ix.id_rank[i], ix.attr[i]};
            const bool g3 = blocks < 0xFFFFFFF0ull && longest < (1ull << 11) &&   // (what a long fragment's slot can say: srn_sback.hip, SB_LONG)
                            hipMalloc(&d_f8, (n + 1) * 8) == hipSuccess && hipMalloc(&d_e8, (blocks + 2) * 16) == hipSuccess &&
                            hipMalloc(&d_sm, 256 * sizeof(ItemMeta)) == hipSuccess && hipMemcpy(d_sm, sm.data(), 256 * sizeof(ItemMeta), hipMemcpyHostToDevice) == hipSuccess &&
                            hipMemcpy(d_base, bb.data(), nblocks * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemset(d_e8, 0, (blocks + 2) * 16) == hipSuccess &&
                            launch_rows_to_frag8(nullptr, (const uint64_t*)d_off, (const uint32_t*)d_items, (uint64_t)n, (const uint32_t*)d_base, (uint2*)d_f8, (uint4*)d_e8) == hipSuccess &&
                            hipDeviceSynchronize() == hipSuccess;
            if (g3) { for (void* q : {d_f8, d_e8, d_sm}) d->allocs.push_back(q);
                      d->bytes += (n + 1) * 8 + (blocks + 2) * 16 + 256 * sizeof(ItemMeta);
                      d->sback.frag8 = (const uint2*)d_f8; d->sback.ext8 = (const uint4*)d_e8; d->sback.sample = (const ItemMeta*)d_sm; }
            else { (void)hipGetLastError(); for (void* q : {d_f8, d_e8, d_sm}) if (q) hipFree(q); d->sback = SBackParams{}; }
        }
        if (d_off) hipFree(d_off); if (d_items) hipFree(d_items); if (d_base) hipFree(d_base);
        if (d_slots) { d->allocs.push_back(d_slots); d->bytes += (n + 1) * slot_bytes; }
        d->di.row_frag = frag ? 1u : 0u;
        if (d_ext) { d->allocs.push_back(d_ext); d->bytes += ext_words * 4; }
        if (!good) { ok = false; set_error("row slot layout on the device failed"); }
        d->di.row_slots = (const RowQuad*)d_slots; d->di.row_ext = (const uint32_t*)d_ext;
    }
    d->di.n_items = (uint32_t)ix.n_items; d->di.n_kept = (uint32_t)ix.n_kept;
    double hi = 1.0, lo = 1.0; bool any = false;   // bounds of idf_eff = (idf > 0 ? idf : 1) for the top-n pre-filter
    for (double v : ix.idf) { const double e = v > 0.0 ? v : 1.0; if (!any) { hi = lo = e; any = true; } else { hi = std::max(hi, e); lo = std::min(lo, e); } }
    d->di.idf_hi = hi; d->di.idf_lo = lo;
    device_refresh_fast_bounds(d, ix);
    if (knobs().debug) fprintf(stderr, "[srn] idf_hi=%g idf_lo=%g n_items=%zu\n", hi, lo, (size_t)ix.n_items);
    if (!ok) { device_release(d); return nullptr; }
    return d;
}

// device_attach for an index whose builder (build_flat_index_core) left post_rank, row_off, row_items and rank_to_session on this device: the same DeviceState, with
// post_rank adopted as the served array, the rows laid out from the device arrays, and row_off / row_items / rank_to_session kept as residue until device_materialize
// brings the host copy up to date.  ix holds the scalars and the per-item arrays.  The four allocations are the attach's from here on, whatever it returns
DeviceState* device_attach_resident(const FlatIndex& ix, int device, const ResidentArrays& a) {
    auto drop = [&] { for (void* p : {a.post_rank, a.row_off, a.row_items, a.rank_to_session}) if (p) hipFree(p); };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) { set_error("no such HIP device"); drop(); return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice failed"); drop(); return nullptr; }
    DeviceState* d = new DeviceState(); d->device = device; d->timing.store(knobs().timing);
    const size_t n = ix.n_kept;
    d->allocs.push_back(a.post_rank); d->bytes += std::max<size_t>(ix.nnz_post * 4, 16);
    d->res_row_off = a.row_off; d->res_row_items = a.row_items; d->res_rank_to_session = a.rank_to_session;
    d->res_bytes = std::max<size_t>((n + 1) * 8, 16) + std::max<size_t>(ix.nnz_rows * 4, 16) + std::max<size_t>(n * 4, 16); d->bytes += d->res_bytes;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) { d->n_cu = prop.multiProcessorCount; d->lds_per_block_max = (int)prop.sharedMemPerBlock; }
    bool ok = true;
    d->di.id_table = upload(d, ix.id_table, ok); d->di.id_mask = ix.id_mask;
    { std::vector<ItemMeta> meta(ix.n_items); std::vector<uint64_t> id_sorted(ix.n_items);
      for (size_t i = 0; i < ix.n_items; ++i) { meta[i] = ItemMeta{ix.idf[i], ix.id_rank[i], ix.attr[i]}; id_sorted[ix.id_rank[i]] = ix.item_id[i]; }
      d->d_meta = (ItemMeta*)upload(d, meta, ok); d->di.meta = d->d_meta; d->di.id_sorted = upload(d, id_sorted, ok);
      std::vector<ItemMeta> ms(512, ItemMeta{0.0, 0u, 0u});   // the fast kernel's threshold sample, as device_attach lays it out
      for (uint32_t w8 = 0; w8 < 8; ++w8) for (uint32_t l = 0; l < 64; ++l) if (8 * l + w8 < ix.n_items) ms[64 * w8 + l] = meta[8 * l + w8];
      d->fast.meta_sample = upload(d, ms, ok); }
    d->di.post_off = upload(d, ix.post_off, ok); d->di.post_rank = (const uint32_t*)a.post_rank;
    d->di.viol = nullptr;   // (a built index: every list complete)
    if (ok) {   // rows -> slots: device_attach's layout, its three host walks over the rows replaced by row_block_bases
        const int rs16 = knobs().row_slots16;
        const bool frag = rs16 == 1;   // (unsharded: fragments only when SRN_ROW_SLOTS=16 forces them)
        const size_t slot_bytes = frag ? 16 : 64;
        const size_t nblocks = (n + 1 + 1023) / 1024;
        const uint64_t* d_off = (const uint64_t*)a.row_off; const uint32_t* d_items = (const uint32_t*)a.row_items;
        void *d_base = nullptr, *d_base_pk = nullptr, *d_slots = nullptr, *d_ext = nullptr;
        uint64_t totals[3] = {0, 0, 0};
        bool good = hipMalloc(&d_base, nblocks * 4) == hipSuccess && hipMalloc(&d_base_pk, nblocks * 4) == hipSuccess &&
                    row_block_bases(d_off, n, frag, (uint32_t*)d_base, (uint32_t*)d_base_pk, totals) == SRN_OK;
        if (good && totals[0] >= 0xFFFFFFF0ull) {
            set_error("row overflow area exceeds 2^32 items"); hipFree(d_base); hipFree(d_base_pk); device_release(d); return nullptr; }
        const size_t ext_words = totals[0] + 16;   // (4-item loads may run past the last row)
        good = good && hipMalloc(&d_slots, (n + 1) * slot_bytes) == hipSuccess && hipMalloc(&d_ext, ext_words * 4) == hipSuccess &&
               hipMemset(d_ext, 0xFF, ext_words * 4) == hipSuccess;
        good = good && (frag ? launch_rows_to_frags : launch_rows_to_slots)(nullptr, d_off, d_items, (uint64_t)n, (const uint32_t*)d_base, (uint32_t*)d_slots, (uint32_t*)d_ext) == hipSuccess &&
               hipDeviceSynchronize() == hipSuccess;
        if (good) {   // the fast kernel's packed rows: optional, as in device_attach
            const uint64_t blocks = totals[1];
            void *d_pk = nullptr, *d_e16 = nullptr;
            bool g2 = blocks < 0xFFFFFFF0ull && hipMalloc(&d_pk, (n + 1) * slot_bytes) == hipSuccess && hipMalloc(&d_e16, (blocks + 2) * 16) == hipSuccess &&
                      hipMemset(d_e16, 0, (blocks + 2) * 16) == hipSuccess &&
                      launch_rows_to_packed(nullptr, d_off, d_items, (uint64_t)n, (const uint32_t*)d_base_pk, (uint32_t*)d_pk, (uint32_t*)d_e16, frag) == hipSuccess &&
                      hipDeviceSynchronize() == hipSuccess;
            if (g2) { d->allocs.push_back(d_pk); d->bytes += (n + 1) * slot_bytes; d->allocs.push_back(d_e16); d->bytes += (blocks + 2) * 16;
                      d->fast.row_packed = (const RowQuad*)d_pk; d->fast.row_ext16 = (const uint32_t*)d_e16; }
            else {
                (void)hipGetLastError();   // (clear the sticky allocation error)
                if (d_pk) hipFree(d_pk); if (d_e16) hipFree(d_e16);
                d->fast.row_packed = nullptr; d->fast.row_ext16 = nullptr;
                if (knobs().debug) fprintf(stderr, "[srn] no room for the fast kernel's packed rows (%zu bytes): general kernel only\n", (size_t)((n + 1) * slot_bytes + (blocks + 2) * 16));
            }
        }
        if (d_base) hipFree(d_base); if (d_base_pk) hipFree(d_base_pk);
        if (d_slots) { d->allocs.push_back(d_slots); d->bytes += (n + 1) * slot_bytes; }
        d->di.row_frag = frag ? 1u : 0u;
        if (d_ext) { d->allocs.push_back(d_ext); d->bytes += ext_words * 4; }
        if (!good) { ok = false; set_error("row slot layout on the device failed"); }
        if (good && totals[2] != ix.max_row_len) { ok = false; set_error("the rows on the device disagree with the index's max_row_len"); }
        d->di.row_slots = (const RowQuad*)d_slots; d->di.row_ext = (const uint32_t*)d_ext;
    }
    d->di.n_items = (uint32_t)ix.n_items; d->di.n_kept = (uint32_t)ix.n_kept;
    double hi = 1.0, lo = 1.0; bool any = false;   // bounds of idf_eff = (idf > 0 ? idf : 1) for the top-n pre-filter
    for (double v : ix.idf) { const double e = v > 0.0 ? v : 1.0; if (!any) { hi = lo = e; any = true; } else { hi = std::max(hi, e); lo = std::min(lo, e); } }
    d->di.idf_hi = hi; d->di.idf_lo = lo;
    device_refresh_fast_bounds(d, ix);
    if (!ok) { device_release(d); return nullptr; }
    return d;
}

// The host copy of a resident index, now: post_rank, row_off, row_items and rank_to_session into ix, then the residue serving does not read is freed (post_rank stays:
// it is the served array).  The caller holds the index's host mutex
int device_materialize(DeviceState* d, FlatIndex& ix) {
    if (!d->res_row_off) return SRN_OK;
    HIP_TRY(hipSetDevice(d->device));
    ix.post_rank.resize(ix.nnz_post); ix.row_off.resize(ix.n_kept + 1); ix.row_items.resize(ix.nnz_rows); ix.rank_to_session.resize(ix.n_kept);
    if (ix.nnz_post) HIP_TRY(hipMemcpy(ix.post_rank.data(), d->di.post_rank, ix.nnz_post * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ix.row_off.data(), d->res_row_off, (ix.n_kept + 1) * 8, hipMemcpyDeviceToHost));
    if (ix.nnz_rows) HIP_TRY(hipMemcpy(ix.row_items.data(), d->res_row_items, ix.nnz_rows * 4, hipMemcpyDeviceToHost));
    if (ix.n_kept) HIP_TRY(hipMemcpy(ix.rank_to_session.data(), d->res_rank_to_session, ix.n_kept * 4, hipMemcpyDeviceToHost));
    for (void* p : {d->res_row_off, d->res_row_items, d->res_rank_to_session}) if (p) hipFree(p);
    d->res_row_off = d->res_row_items = d->res_rank_to_session = nullptr;
    d->bytes -= d->res_bytes; d->res_bytes = 0;
    return SRN_OK;
}
uint64_t device_residue_bytes(const DeviceState* d) { return d ? d->res_bytes : 0; }

// idf bounds of the fast kernel's integer floors: the largest idf_eff of each chunk of 512 direct-mapped items, and of all items
void device_refresh_fast_bounds(DeviceState* d, const FlatIndex& ix) {
    double hi_all = 1.0; bool any = false;
    for (double v : ix.idf) { const double e = v > 0.0 ? v : 1.0; hi_all = any ? std::max(hi_all, e) : e; any = true; }
    for (uint32_t c = 0; c < 8; ++c) {
        double hi = 0.0;
        for (uint64_t i = (uint64_t)c * 512; i < std::min<uint64_t>(ix.n_items, (uint64_t)c * 512 + 512); ++i) hi = std::max(hi, ix.idf[i] > 0.0 ? ix.idf[i] : 1.0);
        d->fast.inv_idf_hot[c] = hi > 0.0 ? 1.0 / hi : 1.0;
    }
    d->fast.inv_idf_hi = 1.0 / hi_all;
    for (uint32_t c = 0; c < SB_H / 256; ++c) {   // the wave-per-query back end's floors: chunks of 256
        double hi = 0.0;
        for (uint64_t i = (uint64_t)c * 256; i < std::min<uint64_t>(ix.n_items, (uint64_t)c * 256 + 256); ++i) hi = std::max(hi, ix.idf[i] > 0.0 ? ix.idf[i] : 1.0);
        d->sback.inv_idf_chunk[c] = hi > 0.0 ? 1.0 / hi : 1.0;
    }
    d->sback.inv_idf_all = 1.0 / hi_all;
}

static void ws_free(Workspace* w) {
    if (!w) return;
    if (w->retry_list) hipFree(w->retry_list);
    if (w->retry_cnt) hipFree(w->retry_cnt);
    if (w->gscratch) hipFree(w->gscratch);
    if (w->spill) hipFree(w->spill);
    if (w->prep) hipFree(w->prep);
    if (w->order) hipFree(w->order);
    if (w->order2) hipFree(w->order2);
    if (w->sb_scr) hipFree(w->sb_scr);
    if (w->slow_list) hipFree(w->slow_list);
    if (w->slow_cnt) hipFree(w->slow_cnt);
    if (w->fin) hipFree(w->fin);
    if (w->big) hipFree(w->big);
    if (w->pin) hipHostFree(w->pin);
    if (w->stage) hipFree(w->stage);
    if (w->wide) hipFree(w->wide);
    if (w->h_retry) hipHostFree(w->h_retry);
    if (w->ev_block) hipEventDestroy(w->ev_block);
    if (w->prep2) hipFree(w->prep2);
    for (int i = 0; i < 2; ++i) { if (w->ev_prep[i]) hipEventDestroy(w->ev_prep[i]); if (w->ev_done[i]) hipEventDestroy(w->ev_done[i]); }
    if (w->ev_fork) hipEventDestroy(w->ev_fork); if (w->ev_join) hipEventDestroy(w->ev_join);
    if (w->side) hipStreamDestroy(w->side);
    for (auto& t : w->ev) for (auto& e : t) if (e) hipEventDestroy(e);
    if (w->stream) hipStreamDestroy(w->stream);
    delete w;
}

void device_release(DeviceState* d) {
    if (!d) return;
    (void)device_serve_stop(d); serve_free_retired(d);
    hipSetDevice(d->device);
    d->rcache.reset();   // (waits for the device)
    hostpipes_free(d);
    for (Workspace* w : d->all_ws) ws_free(w);
    for (void* p : d->allocs) hipFree(p);
    for (void* p : {d->res_row_off, d->res_row_items, d->res_rank_to_session}) if (p) hipFree(p);
    if (d->sb_frag_post) hipFree(d->sb_frag_post);
    delete d;
}

int device_update_attr(DeviceState* d, const FlatIndex& ix) {
    HIP_TRY(hipSetDevice(d->device));
    std::vector<ItemMeta> meta(ix.n_items);
    for (size_t i = 0; i < ix.n_items; ++i) meta[i] = ItemMeta{ix.idf[i], ix.id_rank[i], ix.attr[i]};
    HIP_TRY(hipMemcpy(d->d_meta, meta.data(), meta.size() * sizeof(ItemMeta), hipMemcpyHostToDevice));
    if (d->fast.meta_sample) {   // the fast kernel's copy of the 512 most popular items' records (same order as at attach)
        std::vector<ItemMeta> ms(512, ItemMeta{0.0, 0u, 0u});
        for (uint32_t w8 = 0; w8 < 8; ++w8) for (uint32_t l = 0; l < 64; ++l) if (8 * l + w8 < ix.n_items) ms[64 * w8 + l] = meta[8 * l + w8];
        HIP_TRY(hipMemcpy((void*)d->fast.meta_sample, ms.data(), ms.size() * sizeof(ItemMeta), hipMemcpyHostToDevice));
    }
    if (d->sback.sample) {
        std::vector<ItemMeta> sm(256, ItemMeta{0.0, 0u, 0u});
        for (size_t i = 0; i < std::min<size_t>(256, ix.n_items); ++i) sm[i] = meta[i];
        HIP_TRY(hipMemcpy((void*)d->sback.sample, sm.data(), sm.size() * sizeof(ItemMeta), hipMemcpyHostToDevice));
    }
    return SRN_OK;
}
uint64_t device_bytes(const DeviceState* d) { return d ? d->bytes : 0; }
bool device_has_packed_rows(const DeviceState* d) { return d && d->fast.row_packed != nullptr; }
bool device_sback_streams(const DeviceState* d) { return d && d->sb_frag_post != nullptr; }
bool device_sback_wanted(const DeviceState* d) { return d && d->sback.frag8 != nullptr && !knobs().no_sback_stream && !knobs().no_sback; }
int device_sback_attach_postings(DeviceState* d, DeviceState* post, uint64_t n_postings) {
    if (!d) return SRN_OK;
    HIP_TRY(hipSetDevice(d->device));
    if (d->sb_frag_post && (!post || d->sb_post_for != post->di.post_rank)) {   // (another index's lists, or none: the old copy goes -- after whatever still reads it)
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipFree(d->sb_frag_post)); d->bytes -= d->sb_frag_post_bytes; d->sb_frag_post = nullptr; d->sb_post_for = nullptr; d->sb_frag_post_bytes = 0;
    }
    if (!post || !d->sback.frag8 || d->sb_frag_post || n_postings == 0 || knobs().no_sback_stream || knobs().no_sback) return SRN_OK;
    const uint64_t need = n_postings * 8;
    size_t free_b = 0, total_b = 0; HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (free_b < need + std::max<uint64_t>(total_b / 16, 4ull << 30)) {   // (optional: a sixteenth of the device stays free for the batches' workspaces)
        if (knobs().debug) fprintf(stderr, "[srn] no room for the fragments in posting order (%llu bytes, %zu free): the back end gathers\n", (unsigned long long)need, free_b);
        return SRN_OK;
    }
    void* fp = nullptr;
    if (hipMalloc(&fp, need) != hipSuccess) { (void)hipGetLastError(); return SRN_OK; }
    if (launch_frag_post(nullptr, post->di.post_rank, d->sback.frag8, (uint2*)fp, n_postings) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        const hipError_t e = hipGetLastError(); hipFree(fp); return fail(SRN_EHIP, std::string("fragments in posting order: ") + hipGetErrorString(e));
    }
    d->sb_frag_post = fp; d->sb_post_for = post->di.post_rank; d->sb_frag_post_bytes = need; d->bytes += need;
    return SRN_OK;
}
uint64_t device_sback_launches(const DeviceState* d) { return d ? d->sback_launches.load() : 0; }
int device_count() { int n = 0; return hipGetDeviceCount(&n) == hipSuccess ? n : 0; }

// Host-pointer calls borrow a workspace for the duration of the (synchronous) call.  Device-pointer
// calls return while their work is still in flight, so their scratch stays bound to the user's stream
// (stream order then serialises its reuse).
// A workspace from the pool (host-pointer calls: exclusively the caller's until released) or THE workspace bound to `user_stream` (device-pointer calls).  The latter is
// locked for the duration of the call: its buffers are reused in stream order, which holds only while every call's launches are contiguous in the stream -- two host
// threads on one stream (found by tools/fuzz_concurrency.py with 64 threads on torch's pool of 32 streams: wrong rows, then a GPU memory fault) now take turns.
Workspace* ws_acquire(DeviceState* d, bool bind_to_stream, void* user_stream) {
    std::unique_lock<std::mutex> lk(d->mu);
    if (bind_to_stream) for (auto& sw : d->stream_ws) if (sw.first == user_stream) { Workspace* w = sw.second; lk.unlock(); w->call_mu.lock(); return w; }
    if (!bind_to_stream && !d->free_ws.empty()) { Workspace* w = d->free_ws.back(); d->free_ws.pop_back(); return w; }
    Workspace* w = new Workspace();
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) { delete w; return nullptr; }
    for (auto& t : w->ev) for (auto& e : t) if (hipEventCreate(&e) != hipSuccess) { ws_free(w); return nullptr; }
    if (hipMalloc((void**)&w->retry_cnt, 16) != hipSuccess || hipMalloc((void**)&w->slow_cnt, sizeof(SlowCntBlock)) != hipSuccess || hipHostMalloc((void**)&w->h_retry, sizeof(HostWordBlock), hipHostMallocCoherent) != hipSuccess)   /* (coherent whatever HIP_HOST_COHERENT says: the latency path's caller reads these words while the kernel that writes them is still running) */ { ws_free(w); return nullptr; }
    memset(w->h_retry, 0, sizeof(HostWordBlock));
    if (hipHostGetDevicePointer((void**)&w->h_retry_dev, w->h_retry, 0) != hipSuccess) { ws_free(w); return nullptr; }
    d->all_ws.push_back(w);
    if (bind_to_stream) { d->stream_ws.emplace_back(user_stream, w); w->call_mu.lock(); }   // (nobody else can have found it yet: d->mu is held)
    return w;
}
void ws_release(DeviceState* d, Workspace* w, bool bound) {
    { std::lock_guard<std::mutex> lk(d->mu);
      if (!bound) d->free_ws.push_back(w);
      d->last_ws = w; }
    if (bound) w->call_mu.unlock();
}

int ensure(char** p, size_t* have, size_t need, bool exact) {
    if (*have >= need) return SRN_OK;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *have = 0;
    if (!exact) need = need + need / 4 + 256;
    HIP_TRY(hipMalloc((void**)p, need));
    *have = need; return SRN_OK;
}
int ensure_list(uint32_t** p, size_t* cap, size_t nq, size_t bytes) {
    if (*cap >= nq) return SRN_OK;
    size_t have = 0; *cap = 0;
    const int rc = ensure((char**)p, &have, bytes, true); if (rc) return rc;
    *cap = nq; return SRN_OK;
}

static inline uint32_t round_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }
static inline int bits_host(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }


static inline uint32_t floor_pow2(uint64_t v) { uint32_t p2 = 1; while ((uint64_t)p2 * 2 <= v) p2 <<= 1; return p2; }
static inline uint64_t ceil_pow2(uint64_t v) { uint64_t p2 = 1; while (p2 < v) p2 <<= 1; return p2; }
static inline bool is_prime(uint32_t n) { if (n < 2) return false; for (uint32_t d = 2; (uint64_t)d * d <= n; ++d) if (n % d == 0) return false; return true; }
static inline uint32_t prime_at_most(uint32_t n) { while (n > 2 && !is_prime(n)) --n; return std::max<uint32_t>(n, 2); }
static inline uint32_t prime_at_least(uint64_t n) { uint32_t v = (uint32_t)std::min<uint64_t>(n, 0x3FFFFFFFull); while (!is_prime(v)) ++v; return v; }

// a sketch word sums max(w, 0) * num over ALL elements that share it (<= k rows of <= max_row_len items): can that pass 2^32?
static inline bool sketch_wraps(uint64_t k, uint64_t max_row_len, uint64_t Lmax) { return k * std::max<uint64_t>(1, max_row_len) * 9ull * (Lmax * (Lmax + 1) / 2) >= (1ull << 32); }
// LDS layout + table sizes for one launch (all blocks alike).  min_region_b: extra room the caller needs in region B.
int make_geometry(const DeviceState* d, const FlatIndex& ix, const LaunchParams& p, uint32_t min_region_b, Geometry& g) {
    const Knobs kn = knobs();
    const uint64_t Lmax = p.max_len;
    // position-set slots (no first-match pass over the rows) need <= 8 evolving items and lists complete above x_lo
    g.masks = Lmax <= 8 && p.m <= ix.m_index && ix.lists_complete && !kn.no_masks;
    const int num_bits = g.masks ? (int)Lmax : std::max(1, bits_host(Lmax * (Lmax + 1) / 2));
    const int rank_bits = std::max(1, bits_host(ix.n_kept ? ix.n_kept - 1 : 0));
    g.slot64 = rank_bits + num_bits > 32 || ix.n_kept >= 0xFFFFFFF0ull;
    g.slot_bytes = g.slot64 ? 8 : 4;
    const uint32_t slot_bytes = g.slot_bytes;
    // what the query set could need at most
    const uint64_t m_eff = std::min<uint64_t>(p.m, ix.m_index);
    g.need_sess = std::max<uint64_t>(1, std::min<uint64_t>(Lmax * m_eff, ix.n_kept));
    g.need_item = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)p.k * std::max<uint64_t>(1, ix.max_row_len), ix.n_items));
    KernelCfg& c = g.c;
    c.num_bits = (uint32_t)num_bits;
    c.q_cap = round_up((uint32_t)Lmax + 1, 4);
    c.off_q = MISC_WORDS * 4 + 1024;
    c.off_wave = round_up(c.off_q + c.q_cap * 24 + (c.q_cap + 4) * 4, 16);
    c.off_b = c.off_wave;   // (no per-wave scratch any more)
    const uint32_t region_b = round_up(std::max<uint32_t>(std::max<uint32_t>(p.k * slot_bytes, CAND_CAP * 12), min_region_b), 16);
    c.off_a = c.off_b + region_b;
    const uint32_t lds_max = (uint32_t)std::min(d->lds_per_block_max, 160 * 1024);
    uint32_t budget = 80 * 1024;   // two 512-thread blocks per CU
    if (kn.lds_budget_kb) budget = (uint32_t)kn.lds_budget_kb * 1024;   // experiment knob (occupancy studies)
    if (c.off_a + 32 * 1024 > budget) budget = lds_max;   // long sessions / large k: one block per CU
    if (c.off_a + 8 * 1024 > budget) return fail(SRN_ERANGE, "k / session length too large for the LDS layout");
    const uint32_t a_max = budget - c.off_a;
    c.sess_slots = std::min<uint32_t>(floor_pow2(a_max / slot_bytes), (uint32_t)std::min<uint64_t>(1u << 30, ceil_pow2(g.need_sess * 2)));
    c.sess_slots = std::max<uint32_t>(c.sess_slots, 256);
    // item side of region A: direct-mapped accumulators for the most popular idx, the rest a hash of 4-slot buckets.
    // A direct-mapped word packs (touch count, signed weight sum); if those do not fit 32 bits the hot part is disabled.
    // |10 * linear_score| is 9 at the first position but reaches 89 at position 99 (negative weights beyond position 10, Q3): without
    // position sets a session of >= 20 items can see weights up to min(Lmax, 99) - 10
    const uint64_t w_abs = g.masks ? 9 : std::max<uint64_t>(9, std::min<uint64_t>(Lmax, 99) > 10 ? std::min<uint64_t>(Lmax, 99) - 10 : 0);
    const uint64_t w_max = (uint64_t)p.k * w_abs * (Lmax * (Lmax + 1) / 2) + 1;
    // The exact accumulators (item table, direct-mapped words) are 32-bit integers: |acc(item)| <= k * max over first-match positions q of
    // |10 - q| * num_max(q), where a neighbour whose first match is at position q holds no more recent evolving item: num_max(q) = sum of (L - pos) over
    // pos >= q - 1 = (L - q + 1)(L - q + 2) / 2.  Beyond 2^31 the sums would wrap silently: refuse the call instead (k = 8192 with sessions of ~90+ items).
    {
        uint64_t wn_max = 0;
        for (uint64_t q = 1; q <= std::min<uint64_t>(Lmax, 99); ++q) {
            const uint64_t wq = q <= 10 ? 10 - q : q - 10, nq_ = (Lmax - q + 1) * (Lmax - q + 2) / 2;
            wn_max = std::max(wn_max, wq * nq_);
        }
        if ((uint64_t)p.k * wn_max >= (1ull << 31))
            return fail(SRN_ERANGE, "k * |10 * linear_score| * similarity numerator can exceed the 32-bit item accumulators at this k and session length: lower k or max_items_in_session");
        // a sketch word sums max(w, 0) * num over ALL elements that share it (<= k rows of <= max_row_len items): if even that could wrap, no sketch
        g.sketch_may_wrap = sketch_wraps(p.k, ix.max_row_len, Lmax);
    }
    const int sbits = std::max(2, bits_host(w_max) + 1), cbits = bits_host(p.k);
    // exact words for the 2048 most popular items, 4096 where a query walks many rows (measured with the end-of-round kernel, 2048 -> 4096:
    // config 3 / 4 (k = 1500) +2.6 % / +2.3 %, config 2 (k = 500) -2.6 %: clearing and harvesting the extra words costs more than they save there)
    uint32_t hot = sbits + cbits <= 32 ? (p.k >= 1024 ? 4096u : 2048u) : 0u;
    if (kn.hot_slots >= 0) hot = sbits + cbits <= 32 ? (uint32_t)kn.hot_slots : 0u;   // test knob
    hot = std::min<uint32_t>(std::min<uint32_t>(hot, a_max / 8), round_up((uint32_t)std::min<uint64_t>(ix.n_items, 1u << 20), 4)) / 4 * 4;
    c.hot_slots = hot; c.sum_bits = (uint32_t)sbits;
    // sketch: upper-bound words for all other items (needs the direct-mapped part: its top n give the threshold)
    uint32_t sk = hot && !g.sketch_may_wrap ? 8192u : 0u;
    if (kn.sketch_slots >= 0) sk = hot && !g.sketch_may_wrap && kn.sketch_slots > 0 ? floor_pow2((uint64_t)kn.sketch_slots) : 0u;   // test knob
    while (sk && (uint64_t)sk * 4 * 8 > (uint64_t)(a_max - hot * 4) * 5) sk >>= 1;   // leave >= 3/8 of the room to the exact table
    c.sketch_slots = sk; c.sketch_shift = sk ? 32u - (uint32_t)(bits_host(sk) - 1) : 31u;
    const uint64_t want_buckets = std::max<uint64_t>(61, g.need_item / 2 + 8);          // load <= 0.5 at the worst case
    c.item_buckets = prime_at_most((uint32_t)std::min<uint64_t>((a_max - hot * 4 - sk * 4) / 32, want_buckets));
    c.item_slots = c.item_buckets * 4;
    const uint32_t region_a = std::max<uint32_t>(hot * 4 + sk * 4 + c.item_slots * 8, c.sess_slots * slot_bytes);
    c.region_a_bytes = region_a;
    c.no_merge = kn.no_merge ? 1u : 0u;
    g.lds = (size_t)c.off_a + region_a;
    // tables at least twice the worst case cannot exhaust the probe budget: no retry machinery needed
    g.sess_may_overflow = (uint64_t)c.sess_slots < g.need_sess * 2; g.item_may_overflow = (uint64_t)c.item_slots < g.need_item * 2;
    return SRN_OK;
}

// Does the fast kernel (srn_fast.hip: lean instantiation, then MID over its hand-overs, then the general kernel over what is left) serve this launch?
// What the fast kernel needs of the LAUNCH is the position-set condition (DESIGN.md "Why MASKS is exact": m <= m_index, lists complete) and sketch words that cannot wrap
// at ITS session lengths (<= 10 items: the admission is per query, on the device); the batch's longest session only decides which kernels serve the hand-overs -- up to
// round 3 one session of nine items sent the whole batch to the general kernel.
static uint32_t fast_nb_of(uint64_t n_kept, const Knobs& kn) {   // bits of a fast-kernel slot's list set (0: the index has too many sessions for any)
    const int rank_bits_f = std::max(1, bits_host(n_kept ? n_kept - 1 : 0));
    return kn.fast_runs == 3 && rank_bits_f <= 29 ? 3u : rank_bits_f <= 28 ? 4u : rank_bits_f <= 29 ? 3u : 0u;
}
static uint32_t fast_nb(const FlatIndex& ix, const Knobs& kn) { return fast_nb_of(ix.n_kept, kn); }
FastPlan fast_plan(const DeviceState* d, const FlatIndex& ix, const LaunchParams& p, const Geometry& geo, const Knobs& kn, bool has_ext) {
    FastPlan f;
    // the fast kernel packs (rank, set of <= 4 lists) into 32 bits whatever the general kernel's slots look like: up to 2^28 sessions with 4 lists per query,
    // up to 2^29 with 3 (queries with more go to the MID instantiation / the general kernel)
    f.nb_fast = fast_nb(ix, kn);
    // (round 6) an index whose lists are not ALL complete (a pre-built Avro index: srn_avro.cpp) keeps the fast kernels: the prep kernel marks the queries that an
    // incomplete list can affect (PrepHead::unsafe) and only those go to the general kernel, which then runs its row pass (geo.masks is false for such an index)
    const bool sets_exact = p.m <= ix.m_index && (ix.lists_complete || (d->di.viol != nullptr && !kn.no_viol)) && !kn.no_masks;
    // (a sketch word sums the POSITIVE parts: <= k rows of <= max_row_len items, weight <= 9 * numerator; numerators <= 55 at 10 items, <= 210 at 20)
    const bool fast_sketch_ok = (uint64_t)p.k * std::max<uint64_t>(1, ix.max_row_len) * 9ull * (p.max_len > 10 ? 210ull : 55ull) < (1ull << 32);
    f.mid_tier = !kn.no_mid && !has_ext && d->di.row_frag == 0u && p.max_len >= 5;   // (a query of <= 4 items has <= 4 lists and numerators <= 10: nothing for the MID instantiation)
    f.long_tier = f.mid_tier && !kn.no_long && !kn.no_big && p.max_len > 10;          // (round 5: sessions of 11..20 items -- LONG, a form of MID's BIG layout)
    f.fast = d->fast.row_packed != nullptr && sets_exact && (p.max_len <= 8 ? (geo.masks || !ix.lists_complete) && !geo.sketch_may_wrap : f.mid_tier && fast_sketch_ok) && f.nb_fast != 0 && kn.geometry_default() &&
             !kn.no_fast && p.k <= F_K_MAX && p.m <= F_M_MAX && p.how_many <= (uint32_t)kn.fast_how_many_max && (p.flags & ~(unsigned)SRN_FLAG_BUSINESS_LOGIC) == 0 && p.stats == nullptr && p.nb_rank == nullptr;
    return f;
}

// The serving order of a batch (FastParams::order): room for the keys the prep kernel writes, their sorted copy and the sort's scratch in ONE grow-only buffer; then the sort
// itself, enqueued on the stream the prep kernel ran on.
struct DedupRoom { uint32_t* n_dup = nullptr; uint32_t* rep = nullptr; uint32_t* slots = nullptr; uint32_t* slot_min = nullptr; uint32_t n_slots = 0; };
struct OrderBufs { unsigned long long* keys_in = nullptr; unsigned long long* keys_out = nullptr; void* temp = nullptr; size_t temp_bytes = 0; DedupRoom dd;
                   uint32_t* n_skip = nullptr;   // (a call that uses the result cache) queries at the end of the order that nobody serves: the merged ones + the cache's hits
                   uint32_t* light_cnt = nullptr; };   // (the light form is on) [0] the light representatives of the call, [1] merged + light: where the lean kernel's loop ends (FastParams::order_dups)
static int order_room(char** buf, size_t* have, uint32_t nq, OrderBufs* o, bool dedup = false, bool cache = false, bool light = false) {
    DedupRoom* dd = dedup ? &o->dd : nullptr;
    size_t tb = 0;
    if (sort_order_keys(nullptr, nullptr, nullptr, nq, nullptr, &tb) != hipSuccess) return fail(SRN_EHIP, "rocprim::radix_sort_keys (size query) failed");
    const size_t kb = ((size_t)nq * 8 + 255) / 256 * 256, tbr = (tb + 255) / 256 * 256;
    // (dd: the call merges its equal queries -- the merged count, rep[nq] and the hash table's two arrays belong to the order set, like the keys: a resident call groups on
    //  the side stream while the previous call's kernels still read THEIR count and representatives)
    const size_t rb = ((size_t)nq * 4 + 255) / 256 * 256, n_slots = dd ? dedup_slots(nq) : 0;
    const size_t dd_bytes = dd ? 256 + rb + 2 * n_slots * 4 : 0;
    int rc = ensure(buf, have, 2 * kb + tbr + 256 + dd_bytes + (cache || light ? 256 + 256 : 0)); if (rc) return rc;
    o->keys_in = (unsigned long long*)*buf; o->keys_out = (unsigned long long*)(*buf + kb); o->temp = *buf + 2 * kb; o->temp_bytes = tb;
    if (dd) { char* b = *buf + 2 * kb + tbr + 256; dd->n_dup = (uint32_t*)b; dd->rep = (uint32_t*)(b + 256); dd->slots = (uint32_t*)(b + 256 + rb); dd->slot_min = dd->slots + n_slots; dd->n_slots = (uint32_t)n_slots; }
    if (cache) o->n_skip = (uint32_t*)(*buf + (2 * kb + tbr + 256 + dd_bytes + 255) / 256 * 256);
    if (light) o->light_cnt = (uint32_t*)(*buf + (2 * kb + tbr + 256 + dd_bytes + 255) / 256 * 256);   // (never both: a call that uses the result cache has no light form)
    return SRN_OK;
}

// the workspace's side stream (highest priority: a hardware queue of its own, dispatched ahead of the running call's persistent workgroups) and its events
static int ensure_side(Workspace* w) {
    if (w->side) return SRN_OK;
    int lo = 0, hi = 0; (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIP_TRY(hipStreamCreateWithPriority(&w->side, hipStreamNonBlocking, hi));
    for (int i = 0; i < 2; ++i) { HIP_TRY(hipEventCreateWithFlags(&w->ev_prep[i], hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&w->ev_done[i], hipEventDisableTiming)); }
    HIP_TRY(hipEventCreateWithFlags(&w->ev_fork, hipEventDisableTiming)); HIP_TRY(hipEventCreateWithFlags(&w->ev_join, hipEventDisableTiming));
    return SRN_OK;
}

// ---- the fast sequence's buffers and their wiring (declared in srn_runtime.h: the latency paths use them too) ----
static uint64_t fast_big_entries(size_t cap_q) { return std::min<uint64_t>(0x7FFFFFF0ull, (uint64_t)cap_q * 16 + 4096); }
int reserve_fast(Workspace* w, size_t cap_q) {   // (all allocations of a call happen before its first launch)
    { int rc = ensure_list(&w->slow_list, &w->slow_cap, cap_q, (cap_q * 4 + 64) * 4); if (rc) return rc; }   // (second to fourth part: the MID instantiation's list, its BIG form's, the LONG form's)
    { int rc = ensure(&w->fin, &w->fin_bytes, cap_q * F_FIN_BYTES + 1024); if (rc) return rc; }   // one record per query for vmis_finish_kernel
    return ensure(&w->big, &w->big_bytes, fast_big_entries(cap_q) * 16 + cap_q * 4 + 64);
}
FastBuffers fast_buffers(const Workspace* w, size_t cap_q) { return FastBuffers{w->slow_list, w->slow_cap, w->slow_cnt, w->fin, w->big, fast_big_entries(cap_q)}; }
FastParams fast_params(const DeviceState* d, const FastBuffers& b, const FastPlan& plan, unsigned tiers) {
    FastParams fp = d->fast; fp.slow_list = b.slow_list; fp.slow_cnt = b.slow_cnt; fp.nb = plan.nb_fast; fp.max_runs = plan.nb_fast; fp.fin = b.fin;
    fp.big_arena = b.big; fp.big_list = b.big ? (uint32_t*)(b.big + b.big_entries * 16) : nullptr; fp.big_cap_entries = (uint32_t)b.big_entries;
    fp.big_ticket = b.slow_cnt ? (unsigned long long*)(b.slow_cnt + SC_BIG_TICKET_LO) : nullptr;
    fp.xchg = nullptr; fp.xchg_stride = 0; fp.q_base = 0; fp.order = nullptr;
    fp.mid_list = (tiers & TIER_MID) ? slow_part(b.slow_list, b.slow_cap, SL_MID) : nullptr; fp.mid_cnt = fp.mid_list ? b.slow_cnt + SC_MID : nullptr;
    fp.bigq_list = (tiers & TIER_BIGQ) ? slow_part(b.slow_list, b.slow_cap, SL_BIGQ) : nullptr; fp.bigq_cnt = fp.bigq_list ? b.slow_cnt + SC_BIGQ : nullptr;
    fp.long_list = (tiers & TIER_LONG) ? slow_part(b.slow_list, b.slow_cap, SL_LONG) : nullptr; fp.long_cnt = fp.long_list ? b.slow_cnt + SC_LONG : nullptr;
    return fp;
}

// ---- the batch launch sequence: plan -> reserve -> enqueue ----
// What a predict call (predict_core) will do, computed once from the index, the parameters, the knobs and the call's kind; nothing in it touches the device.
struct LaunchPlan {
    Knobs kn; Geometry geo;
    bool retry = false;                                             // some query's session or item table may not fit LDS: the global-table pass stands behind the launch
    KernelCfg cg{}; uint64_t g_stride = 0; int retry_blocks = 0;    // ... its geometry, a workgroup's arena, its grid
    uint32_t grid = 0, grid_fast = 0, prep_stride = 0;              // the general kernel's grid, the fast kernel's
    FastPlan fast;
    bool resident = false, order_set2 = false;                      // SRN_FLAG_INPUTS_RESIDENT: the front on the side stream; on the second set of order buffers
    bool ordered = false, dedup = false, prep_clears = false;
    bool light = false;                                             // the call's light queries -- one posting run of <= 64 kept entries -- are served by vmis_light_kernel (srn_light.hip), a wave each
    bool cache = false;                                             // the call looks its queries up in the index's result cache and stores what it served (srn_result_cache.hip)
};
// the global-table pass: tables at twice the worst case in a global-memory arena per workgroup (cg: geo.c on entry), as many workgroups as 2 GB hold, at most one per CU
static void global_tables_geometry(const DeviceState* d, const Geometry& geo, KernelCfg& cg, uint64_t& g_stride, int& retry_blocks) {
    cg.sess_slots = (uint32_t)std::min<uint64_t>(1u << 30, std::max<uint64_t>(256, ceil_pow2(geo.need_sess * 2)));
    cg.item_buckets = prime_at_least(geo.need_item / 2 + 64); cg.item_slots = cg.item_buckets * 4;
    g_stride = std::max<uint64_t>((uint64_t)cg.sess_slots * geo.slot_bytes, (uint64_t)cg.hot_slots * 4 + (uint64_t)cg.sketch_slots * 4 + (uint64_t)cg.item_slots * 8);
    g_stride = (g_stride + 255) / 256 * 256;
    retry_blocks = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)d->n_cu, (2ull << 30) / g_stride));
}
static LaunchPlan make_plan(const DeviceState* d, const FlatIndex& ix, const LaunchParams& p, const Geometry& geo, const ExtLists* ext, bool resident, const Workspace* w, const ResultCache* rcache) {
    LaunchPlan pl; pl.kn = knobs(); pl.geo = geo; pl.resident = resident;
    const Knobs& kn = pl.kn; const KernelCfg& c = geo.c;
    pl.retry = geo.sess_may_overflow || geo.item_may_overflow;
    pl.cg = c;
    if (pl.retry) global_tables_geometry(d, geo, pl.cg, pl.g_stride, pl.retry_blocks);
    const uint32_t blocks_per_cu = std::max<uint32_t>(1, (160 * 1024) / (uint32_t)geo.lds);
    // 16 workgroups per resident slot: the hardware hands out workgroups as slots free up, so smaller chunks of queries shorten the
    // tail of a launch (measured on config 3: x1 10.62 ms, x4 10.50, x16 10.35, x32 10.32)
    const uint32_t grid_mult = (uint32_t)kn.grid_mult;
    pl.grid = (uint32_t)std::min<uint64_t>(p.nq, (uint64_t)d->n_cu * std::min<uint32_t>(blocks_per_cu, 2048 / kBlock) * grid_mult);
    pl.prep_stride = prep_stride_of(p.max_len);
    pl.fast = fast_plan(d, ix, p, geo, kn, ext != nullptr);
    // The fast kernel's workgroups walk their queries in a pipeline (the next record is fetched during the current query), so they want ~12 queries each;
    // beyond that, more and smaller workgroups shorten the tail of the launch.  Measured on config 3 (ms per launch at 8 / 16 / 32 / 64 resident sets): 2^20 queries
    // 26.29 / 26.06 / 25.85 / 25.81; 2^18: - / 6.62 / 6.57 / 6.63; 2^16: - / 1.70 / 1.72 / 1.78.
    const uint64_t res_wg = (uint64_t)d->n_cu * F_WG_PER_CU;
    pl.grid_fast = kn.grid_mult_set ? (uint32_t)std::min<uint64_t>(p.nq, res_wg * grid_mult)
                                    : (uint32_t)std::min<uint64_t>(p.nq, std::min<uint64_t>(res_wg * 64, std::max<uint64_t>(res_wg * 16, p.nq / 12)));
    // the serving order: the batch sorted by each query's most popular item (keys from the prep kernel, one radix sort behind it)
    pl.ordered = pl.fast.fast && !ext && kn.order_min > 0 && p.nq >= (uint32_t)kn.order_min;
    // ... and, in that order, only the first of the call's queries with one and the same item sequence (srn_dedup.hip); the others get its row at the end
    pl.dedup = pl.ordered && !kn.no_dedup;
    // The result cache is on exactly where the fast path is, for calls with the parameters its rows were computed with.  Such a call is ordered at every
    // batch size -- the order is what keeps queries away from the serving kernels: a hit sorts behind everything that is served, like a merged query -- and never resident:
    // the hits' rows are written into the caller's buffers at the front of the call, which on the side stream could overtake a previous call that still owns them.
    pl.cache = rcache != nullptr && pl.fast.fast && !ext && p.k == rcache->k && p.m == rcache->m && p.how_many == rcache->how_many && (p.flags & SRN_FLAG_BUSINESS_LOGIC) == rcache->flags;
    if (pl.cache) { pl.ordered = true; pl.resident = false; resident = false; }
    // The light form: K = kept needs k >= 64, finish_inline ranks <= 64 entries; its segment of the order exists in an ordered call only.  SRN_LIGHT_MIN is
    // the A/B switch, and keeps small ordered batches (SRN_ORDER_MIN=1 in the tests) on the lean chain
    pl.light = pl.ordered && pl.fast.fast && !ext && !pl.cache && p.k >= RW_LIGHT_KEPT && p.how_many <= 64u && kn.light_min > 0 && p.nq >= (uint32_t)kn.light_min && d->di.row_frag == 0u;
    // (one order per set of prep records: a resident call's prep kernel and sort run on the side stream while the previous call's kernels still read THEIR order)
    pl.order_set2 = resident && (w->resident_calls & 1u) != 0u;
    // The prep kernel clears the launch sequence's counters where it runs on this stream ahead of everything that uses them (two fill kernels otherwise: 6 us each)
    pl.prep_clears = !ext && !resident;
    return pl;
}

// every buffer of the call (all allocations of a call happen before its first launch; hipMalloc / hipFree synchronise the device)
static int reserve_batch(Workspace* w, const LaunchPlan& pl, const LaunchParams& p, const ExtLists* ext, OrderBufs& ob) {
    if (pl.retry) {
        int rc = ensure_list(&w->retry_list, &w->retry_cap, p.nq, (size_t)p.nq * 4 + 64); if (rc) return rc;
        rc = ensure(&w->gscratch, &w->gscratch_bytes, pl.g_stride * pl.retry_blocks); if (rc) return rc;
    }
    // per-block global copy of the neighbour list (walk B reads it after phase 4a has reused the LDS)
    { int rc = ensure(&w->spill, &w->spill_bytes, (size_t)std::max<uint32_t>(pl.grid, (uint32_t)pl.retry_blocks) * p.k * pl.geo.slot_bytes); if (rc) return rc; }
    if (!ext) { int rc = ensure(&w->prep, &w->prep_bytes, (size_t)p.nq * pl.prep_stride); if (rc) return rc; }
    if (pl.resident) {   // a second set of prep records: call i + 1's prep kernel runs while call i's kernels still read theirs
        int rc = ensure(&w->prep2, &w->prep2_bytes, (size_t)p.nq * pl.prep_stride); if (rc) return rc;
        rc = ensure_side(w); if (rc) return rc;
    }
    if (pl.fast.fast) { int rc = reserve_fast(w, p.nq); if (rc) return rc; }
    if (pl.ordered) return order_room(pl.order_set2 ? &w->order2 : &w->order, pl.order_set2 ? &w->order2_bytes : &w->order_bytes, p.nq, &ob, pl.dedup, pl.cache, pl.light);
    return SRN_OK;
}

// one call between its reserve and its last enqueue
struct BatchCall {
    DeviceState* d; Workspace* w; const LaunchPlan& pl; const ExtLists* ext; hipStream_t st; DeviceIndex di; LaunchParams p; OrderBufs ob;
    hipEvent_t* ev = nullptr; bool timed = false, fork_retry = false;
    bool sback_second = false;   // the item shard's wave-per-query back end ran with the fast kernel's back-end form behind it (its list is the MID tier's: srn_debug_last_mid_count reports it)
    FastParams fp{};
    ResultCache* rcache = nullptr; uint32_t cache_now = 0;   // (pl.cache) the index's result cache, held by predict_core for the length of the call; the call's number in it
};

// host-pointer calls: the staging buffer, p pointed at it, the inputs on their way
static int stage_host_inputs(Workspace* w, hipStream_t st, LaunchParams& p, const HostRows& h) {
    const bool stats = h.stats != nullptr, nb = h.nb_rank != nullptr;
    const size_t n_out = (size_t)p.nq * p.how_many, nitems = h.q_off[p.nq];
    Bump b;
    const auto r_items = b.take<const uint64_t>(nitems * 8); const auto r_qoff = b.take<const uint32_t>(((size_t)p.nq + 1) * 4);
    const auto r_ids = b.take<uint64_t>(n_out * 8); const auto r_sc = b.take<double>(n_out * 8); const auto r_cnt = b.take<uint32_t>((size_t)p.nq * 4);
    const auto r_st = b.take<uint32_t>(stats ? (size_t)p.nq * 32 : 0);
    const auto r_nr = b.take<uint32_t>(nb ? (size_t)p.nq * p.k * 4 : 0), r_nn = b.take<uint32_t>(nb ? (size_t)p.nq * p.k * 4 : 0), r_nc = b.take<uint32_t>(nb ? (size_t)p.nq * 4 : 0);
    int rc = ensure(&w->stage, &w->stage_bytes, b.bytes); if (rc) return rc;
    char* s = w->stage;
    p.items_flat = r_items.at(s); p.q_off = r_qoff.at(s);
    p.out_ids = r_ids.at(s); p.out_scores = r_sc.at(s); p.out_counts = r_cnt.at(s);
    p.stats = stats ? r_st.at(s) : nullptr;
    p.nb_rank = nb ? r_nr.at(s) : nullptr; p.nb_num = nb ? r_nn.at(s) : nullptr;
    p.nb_cnt = nb ? r_nc.at(s) : nullptr;
    HIP_TRY(hipMemsetAsync(p.out_ids, 0, n_out * 8, st));      // unused tail of each row reads as 0
    HIP_TRY(hipMemsetAsync(p.out_scores, 0, n_out * 8, st));
    HIP_TRY(hipMemcpyAsync((void*)p.items_flat, h.items, nitems * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync((void*)p.q_off, h.q_off, ((size_t)p.nq + 1) * 4, hipMemcpyHostToDevice, st));
    return SRN_OK;
}
// ... and the results back, then the wait for them
static int fetch_host_outputs(const BatchCall& c, const HostRows& h) {
    const LaunchParams& p = c.p; hipStream_t st = c.st; const size_t n_out = (size_t)p.nq * p.how_many;
    HIP_TRY(hipMemcpyAsync(h.ids, p.out_ids, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h.scores, p.out_scores, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h.counts, p.out_counts, (size_t)p.nq * 4, hipMemcpyDeviceToHost, st));
    if (h.stats) HIP_TRY(hipMemcpyAsync(h.stats, p.stats, (size_t)p.nq * 32, hipMemcpyDeviceToHost, st));
    if (h.nb_rank) {
        HIP_TRY(hipMemcpyAsync(h.nb_rank, p.nb_rank, (size_t)p.nq * p.k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h.nb_num, p.nb_num, (size_t)p.nq * p.k * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h.nb_cnt, p.nb_cnt, (size_t)p.nq * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return SRN_OK;
}

// The front of the sequence on stream `s` -- the prep kernel into the record set `rec`, the grouping of equal queries, the sort of the order keys.  On the caller's own
// stream (prep_clears) the prep kernel also clears the sequence's counters and the grouping pass writes the merged rows' count words; a resident call runs it on the side stream.
static int enqueue_front(BatchCall& c, hipStream_t s, char* rec) {
    const LaunchParams& p = c.p; const LaunchPlan& pl = c.pl; OrderBufs& ob = c.ob; Workspace* w = c.w;
    // (the light form: the light representatives are counted where their key becomes final -- by the grouping pass's resolve kernel, or, in a call that does not merge, by the prep kernel)
    if (pl.light && !pl.dedup) HIP_TRY(hipMemsetAsync(ob.light_cnt, 0, 8, s));
    HIP_TRY(launch_prep(s, c.di, p.items_flat, p.q_off, p.nq, p.m, p.max_len, rec, pl.prep_stride, pl.fast.nb_fast == 3u, pl.prep_clears && pl.fast.fast ? w->slow_cnt : nullptr,
                        pl.prep_clears && pl.retry ? w->retry_cnt : nullptr, nullptr, 0, ob.keys_in, pl.light, pl.light && !pl.dedup ? ob.light_cnt : nullptr));
    if (pl.dedup) {   // (a resident call: the count word of a merged row is written on the caller's stream -- the previous call's kernels may still be writing these very buffers)
        HIP_TRY(hipMemsetAsync(ob.dd.slots, 0xFF, (size_t)ob.dd.n_slots * 8, s));
        HIP_TRY(launch_dedup_group(s, p.items_flat, p.q_off, p.nq, ob.dd.slots, ob.dd.slot_min, ob.dd.n_slots, (uint32_t)pl.kn.dedup_hash_bits, ob.dd.rep, ob.keys_in, pl.prep_clears ? p.out_counts : nullptr, ob.dd.n_dup, pl.light ? ob.light_cnt : nullptr));
    }
    // the result cache's lookup: over the representatives, behind their grouping and ahead of the sort -- a hit's row is written here, its key moves behind the served queries
    if (pl.cache) { int rc = rcache_enqueue_lookup(c.rcache, s, p, pl.dedup ? ob.dd.rep : nullptr, ob.keys_in, pl.dedup ? ob.dd.n_dup : nullptr, ob.n_skip, pl.kn.cache_hash_bits, &c.cache_now); if (rc) return rc; }
    if (pl.ordered) HIP_TRY(sort_order_keys(s, ob.keys_in, ob.keys_out, p.nq, ob.temp, &ob.temp_bytes));
    c.p.prep = rec; c.p.prep_stride = pl.prep_stride;
    return SRN_OK;
}
// a resident call's front on the side stream: behind the call that used this set of records two calls ago, beside the previous call's kernels
static int enqueue_front_resident(BatchCall& c) {
    Workspace* w = c.w; hipStream_t st = c.st;
    const int par = (int)(w->resident_calls & 1u);
    // (ev_done[set] = the end of the LAST call that read record set `set`, resident or not: a non-resident device-pointer call on this stream reads w->prep too)
    if (!w->rec_used[par] && w->calls > 0) { HIP_TRY(hipEventRecord(w->ev_done[par], st)); w->rec_used[par] = true; }   // (earlier calls of this workspace that left no event: everything enqueued so far)
    if (w->rec_used[par]) HIP_TRY(hipStreamWaitEvent(w->side, w->ev_done[par], 0));
    { int rc = enqueue_front(c, w->side, par ? w->prep2 : w->prep); if (rc) return rc; }
    HIP_TRY(hipEventRecord(w->ev_prep[par], w->side));
    HIP_TRY(hipStreamWaitEvent(st, w->ev_prep[par], 0));
    if (c.pl.dedup) HIP_TRY(launch_dedup_mark(st, c.p.nq, c.ob.dd.rep, c.p.out_counts));
    return SRN_OK;
}
// The shard group's neighbours pipeline, FRONT: find_neighbors alone for the queries [q_lo, nq) of the batch this rank fronts -- the fast kernel's front end against
// the replicated posting lists, neighbour lists into the exchange buffer.  Nothing else of the launch sequence runs (the back end of every rank follows the all-gather).
static int enqueue_shard_front(BatchCall& c) {
    const ExtLists* ext = c.ext; LaunchParams& p = c.p;
    if (ext->q_lo >= p.nq) return SRN_OK;
    p.prep = ext->prep; p.prep_stride = c.pl.prep_stride;
    FastParams fp = fast_params(c.d, FastBuffers{}, c.pl.fast);
    fp.xchg = ext->x.words; fp.xchg_stride = ext->x.stride; fp.q_base = ext->q_lo;
    const uint64_t cnt = p.nq - ext->q_lo, res_wg = (uint64_t)c.d->n_cu * F_WG_PER_CU;
    const uint32_t grid_front = (uint32_t)std::min<uint64_t>(cnt, std::min<uint64_t>(res_wg * 64, std::max<uint64_t>(res_wg * 16, cnt / 12)));
    HIP_TRY(launch_fast(FastForm::Front, dim3(grid_front), c.st, c.di, p, fp, c.pl.kn.debug));
    return SRN_OK;
}
// the item shard's own back end (srn_sback.hip): one wave per query, 12 per CU; a persistent grid of a few waves per resident slot
static int enqueue_shard_back(BatchCall& c) {
    DeviceState* d = c.d; Workspace* w = c.w; const ExtLists* ext = c.ext; const LaunchParams& p = c.p; const Knobs& kn = c.pl.kn; FastParams& fp = c.fp;
    SBackParams sbp = d->sback;
    // the streaming form where the shard holds its fragments in the posting order of the very lists the records were written against (9 waves per CU: 16.8 KB each)
    const bool stream = ext->x.positions;
    if (stream && !(d->sb_frag_post && d->sb_post_for == ext->post_rank)) return fail(SRN_ESTATE, "the batch's neighbours came as posting positions, but this shard does not hold its fragments in posting order");
    const uint64_t slots = (uint64_t)d->n_cu * (stream ? 9 : 12);
    uint32_t grid_b = (uint32_t)std::min<uint64_t>(p.nq, slots * (kn.grid_mult_set ? (uint32_t)kn.grid_mult : stream ? 4 : 16));   // (gather form, round 6: 1 / 2 / 4 / 8 / 16 / 32 waves per slot = 1.295 / 1.247 / 1.191 / 1.148 / 1.115 / 1.114 ms -- the tail of a persistent grid costs more than the first query of a wave, which has no prefetched record)
    if (fp.order) grid_b = std::max<uint32_t>(8u, grid_b / 8u * 8u);
    if (stream) {
        int rc = ensure(&w->sb_scr, &w->sb_scr_bytes, (size_t)grid_b * shard_back_scratch_words() * 4); if (rc) return rc;
        sbp.frag_post = (const uint2*)d->sb_frag_post; sbp.post_rank = ext->post_rank; sbp.scr = (uint32_t*)w->sb_scr;
    }
    const bool second = !kn.no_sback_second && !stream; c.sback_second = second;   // (the streaming form's records are not neighbour slots)  // what outgrows the wave's room: the round-4 back end (eight waves per query) over a list, before the general kernel
    if (second) { fp.mid_list = slow_part(w->slow_list, w->slow_cap, SL_MID); fp.mid_cnt = w->slow_cnt + SC_MID; }
    HIP_TRY(launch_shard_back(dim3(grid_b), c.st, c.di, p, fp, sbp, kn.debug));
    d->sback_launches.fetch_add(1, std::memory_order_relaxed);
    if (second) {
        FastParams fl = fp; fl.order = nullptr;
        HIP_TRY(launch_fast(FastForm::Back, dim3((uint32_t)std::min<uint64_t>(p.nq, (uint64_t)d->n_cu * F_WG_PER_CU * 4)), c.st, c.di, p, fl, kn.debug));
        fp.mid_list = nullptr; fp.mid_cnt = nullptr;
    }
    return SRN_OK;
}
// The fast kernel (srn_fast.hip) serves the common query shape; what it cannot take -- decided per query, on the device -- is queued on slow_list and served by the
// general kernel right behind it.  Here: its lean form (or the shard group's back end), then MID, BIG and LONG over what was listed for them.
static int enqueue_fast_tiers(BatchCall& c) {
    DeviceState* d = c.d; Workspace* w = c.w; const ExtLists* ext = c.ext; const LaunchParams& p = c.p; const LaunchPlan& pl = c.pl; const Knobs& kn = pl.kn; hipStream_t st = c.st;
    w->cnt_dirty = true;   // (the latency path's fused launch wants the counters at 0 and clears them itself after a sequence like this one)
    if (!pl.prep_clears) HIP_TRY(hipMemsetAsync(w->slow_cnt, 0, sizeof(SlowCntBlock), st));
    // (round 5: the BIG form also without a MID tier -- it takes the lean shape's oversized queries of the headline batches; not over an item shard's fragments)
    const bool big_tier = !kn.no_big && !ext && d->di.row_frag == 0u;
    FastParams& fp = c.fp;
    fp = fast_params(d, w, pl.fast, p.nq, (pl.fast.mid_tier ? TIER_MID : 0u) | (big_tier ? TIER_BIGQ : 0u) | (pl.fast.long_tier ? TIER_LONG : 0u));
    const bool back = ext && ext->mode == 2;   // neighbour lists from the exchange buffer (any rank's front end), this shard's rows
    if (back) { fp.xchg = ext->x.words; fp.xchg_stride = ext->x.stride; }
    fp.order = pl.ordered ? c.ob.keys_out : back ? ext->order : nullptr;
    fp.order_dups = pl.cache ? c.ob.n_skip : pl.light ? c.ob.light_cnt + 1 : pl.dedup ? c.ob.dd.n_dup : nullptr;   // (the cache's count: its hits + the merged queries; the light form's: the merged queries + the light ones)
    // the light form, right behind the front and ahead of the lean launch: a fixed grid of waves that stride over the light segment of the order and leave at once when it is empty
    if (pl.light) HIP_TRY(launch_light(st, (uint32_t)std::min<uint64_t>((p.nq + 3u) / 4u, (uint64_t)d->n_cu * 4u), c.di, p, c.ob.keys_out, c.ob.light_cnt, c.ob.light_cnt + 1, fp.slow_list, fp.slow_cnt, w->h_retry_dev + HW_LIGHT));
    const uint32_t grid_fo = fp.order ? std::max<uint32_t>(8u, pl.grid_fast / 8u * 8u) : pl.grid_fast;   // (an ordered launch walks an eighth of the order per XCD: the grid is a multiple of 8)
    if (back && d->sback.frag8 && !kn.no_sback && p.max_len <= 8) { int rc = enqueue_shard_back(c); if (rc) return rc; }
    else HIP_TRY(launch_fast(back ? FastForm::Back : FastForm::Lean, dim3(grid_fo), st, c.di, p, fp, kn.debug));
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[4], st));
    const uint64_t res_wg = (uint64_t)d->n_cu * F_WG_PER_CU;
    // The MID instantiation over what the lean one listed for it (sessions of <= 10 items, <= 8 lists); what it cannot take either joins slow_list.  The list's length
    // is known on the device only: a fixed grid, workgroups beyond the list leave at once.
    if (pl.fast.mid_tier) HIP_TRY(launch_fast(FastForm::Mid, dim3((uint32_t)std::min<uint64_t>(p.nq, res_wg * 8)), st, c.di, p, fp, kn.debug));
    // ... and MID's BIG form (80 KB of LDS, two workgroups per CU) over what MID passed on only for want of merge-buffer room
    if (fp.bigq_list) HIP_TRY(launch_fast(FastForm::Big, dim3((uint32_t)std::min<uint64_t>(p.nq, (uint64_t)d->n_cu * 2 * 4)), st, c.di, p, fp, kn.debug));
    // ... and the LONG form over the sessions of 11..20 items the lean instantiation listed for it
    if (fp.long_list) HIP_TRY(launch_fast(FastForm::Long, dim3((uint32_t)std::min<uint64_t>(p.nq, (uint64_t)d->n_cu * 2 * 4)), st, c.di, p, fp, kn.debug));
    return SRN_OK;
}
// the general kernel: over what the fast sequence handed to it, or over the whole batch
static int enqueue_general(const BatchCall& c) {
    const LaunchPlan& pl = c.pl; Workspace* w = c.w;
    PredictLaunch a; a.masks = pl.geo.masks; a.slot64 = pl.geo.slot64; a.spill = w->spill; a.retry_list = w->retry_list; a.retry_cnt = w->retry_cnt;
    if (pl.fast.fast) { a.qlist = w->slow_list; a.qn = w->slow_cnt; }
    HIP_TRY(launch_predict(a, dim3(pl.grid), pl.geo.lds, c.st, c.di, c.p, pl.geo.c));
    return SRN_OK;
}
// the global-table pass over what the general kernel listed: one workgroup per arena, tables in global memory
static int enqueue_global_pass(const BatchCall& c, hipStream_t s) {
    const LaunchPlan& pl = c.pl; Workspace* w = c.w;
    PredictLaunch a; a.masks = pl.geo.masks; a.slot64 = pl.geo.slot64; a.global_tables = true; a.qlist = w->retry_list; a.qn = w->retry_cnt;
    a.gscratch = w->gscratch; a.gstride = pl.g_stride; a.spill = w->spill;
    HIP_TRY(launch_predict(a, dim3(pl.retry_blocks), pl.geo.c.off_a, s, c.di, c.p, pl.cg));
    return SRN_OK;
}
// the fast sequence behind its tiers: the general kernel, the global-table pass where it is forked, the two finish kernels
static int enqueue_fast_finish(const BatchCall& c) {
    Workspace* w = c.w; const LaunchParams& p = c.p; hipStream_t st = c.st;
    { int rc = enqueue_general(c); if (rc) return rc; }
    if (c.fork_retry) {   // the global-table pass beside the finish kernels (they touch disjoint rows: a finish kernel only completes rows flagged by the fast kernel)
        HIP_TRY(hipEventRecord(w->ev_fork, st)); HIP_TRY(hipStreamWaitEvent(w->side, w->ev_fork, 0));
        { int rc = enqueue_global_pass(c, w->side); if (rc) return rc; }
        HIP_TRY(hipEventRecord(w->ev_join, w->side));
    }
    HIP_TRY(launch_finish(st, c.di, c.fp, p.out_ids, p.out_scores, p.out_counts, p.nq, p.how_many));
    // (it also writes the call's two counters -- global-table queries, handed-over queries; both final once the general kernel is done -- into the pinned words)
    HIP_TRY(launch_finish_big(st, c.di, c.fp, p.out_ids, p.out_scores, p.out_counts, p.how_many, (uint32_t)std::min<uint64_t>(p.nq, (uint64_t)c.d->n_cu * 16),
                              c.pl.retry ? w->retry_cnt : nullptr, w->slow_cnt, w->h_retry_dev));
    return SRN_OK;
}
// behind the kernels that serve: the merged queries' rows, the global-table pass (joined, or in line), the call's events and what the next call and the getters read
static int enqueue_tail(BatchCall& c) {
    Workspace* w = c.w; const LaunchParams& p = c.p; const LaunchPlan& pl = c.pl; hipStream_t st = c.st; const OrderBufs& ob = c.ob;
    const bool fast = pl.fast.fast;
    // the merged queries' rows: behind every kernel that can write a representative's row -- the global-table pass included, where the launch has one
    const bool fill_late = pl.dedup && pl.retry;
    if (pl.dedup && !fill_late) HIP_TRY(launch_dedup_fill(st, p.nq, ob.dd.rep, p.out_ids, p.out_scores, p.out_counts, p.how_many, ob.dd.n_dup, w->h_retry_dev + HW_MERGED));
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[1], st));
    if (c.fork_retry) HIP_TRY(hipStreamWaitEvent(st, w->ev_join, 0));
    else if (pl.retry) {
        { int rc = enqueue_global_pass(c, st); if (rc) return rc; }
        if (!fast) HIP_TRY(hipMemcpyAsync(w->h_retry + HW_GLOBAL, w->retry_cnt, 4, hipMemcpyDeviceToHost, st));   // (fast: vmis_finish_big_kernel wrote both words.  Not fast: last_fast = false says
                                                                                                                //  "all of last_nq" -- no host write into a pinned word that an earlier call may still be writing)
    }
    if (fill_late) HIP_TRY(launch_dedup_fill(st, p.nq, ob.dd.rep, p.out_ids, p.out_scores, p.out_counts, p.how_many, ob.dd.n_dup, w->h_retry_dev + HW_MERGED));
    // the result cache's insert: behind everything that can write a row (the global-table pass included, like fill_late) -- the keys the sort read are still in place
    if (pl.cache) { int rc = rcache_enqueue_insert(c.rcache, st, p, pl.dedup ? ob.dd.rep : nullptr, ob.keys_in, pl.kn.cache_hash_bits, c.cache_now); if (rc) return rc; }
    HIP_TRY(hipEventRecord(c.ev[2], st));
    if (pl.resident) { const int par = (int)(w->resident_calls & 1u); HIP_TRY(hipEventRecord(w->ev_done[par], st)); w->rec_used[par] = true; ++w->resident_calls; }
    else if (!c.ext && w->side) { HIP_TRY(hipEventRecord(w->ev_done[0], st)); w->rec_used[0] = true; }   // (a workspace that has served resident calls: the next one's side-stream prep must not overwrite w->prep under this call's kernels)
    ++w->calls; w->last_retry = pl.retry ? 1 : 0; w->last_nq = p.nq; w->last_fast = fast; w->last_mid = fast && (pl.fast.mid_tier || c.sback_second); w->last_dedup = pl.dedup; w->last_light = pl.light; w->last_untimed = false;
    if (pl.retry) w->h_retry_valid = true;   // (from now on the pinned counter holds a finished call's count -- or is being overwritten by a newer one)
    return SRN_OK;
}
// everything a call enqueues between its inputs and its results
static int enqueue_batch(BatchCall& c, bool on_device) {
    Workspace* w = c.w; const LaunchPlan& pl = c.pl; hipStream_t st = c.st; const bool fast = pl.fast.fast;
    if (pl.retry && !pl.prep_clears) HIP_TRY(hipMemsetAsync(w->retry_cnt, 0, 4, st));
    c.ev = w->ev[w->calls % Workspace::RING];
    // Per-kernel events only when someone asked for kernel times: an event between two kernels idles the stream for ~6 us (three of them: 18 us of a 4 096-query batch's 250)
    c.timed = c.d->timing.load(std::memory_order_relaxed);
    w->ring_timed[w->calls % Workspace::RING] = c.timed;
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[0], st));
    if (c.ext) { c.p.prep = c.ext->prep; c.p.prep_stride = pl.prep_stride; }
    else { int rc = pl.resident ? enqueue_front_resident(c) : enqueue_front(c, st, w->prep); if (rc) return rc; }
    if (c.timed) HIP_TRY(hipEventRecord(c.ev[3], st));
    // The global-table retry pass serves a handful of queries with one workgroup each, ~0.3 ms behind everything else on config 5.  Where earlier
    // calls on this workspace did retry queries (the pinned counter of the last finished call says so: a hint, read without synchronising) it is forked onto the side
    // stream right behind the general kernel and runs beside the finish kernels; where nothing is ever retried (configs 2-4) the two extra events would cost more
    // than the empty pass.
    // (Tried in round 3 and dropped: the general kernel over the handed-over queries + the global-table pass on the side stream, beside the two finish kernels -- 38 + 4 us
    //  against 17 + 10 us at 4 096 queries.  4 096 / 65 536 / 2^20 queries: 0.220 / 1.759 / 25.28 ms forked, 0.215 / 1.759 / 25.25 ms in line.)
    c.fork_retry = fast && pl.retry && on_device && *(volatile uint32_t*)(w->h_retry + HW_GLOBAL) != 0u && w->h_retry_valid;
    if (c.fork_retry) { int rc = ensure_side(w); if (rc) return rc; }
    if (fast) {
        int rc = enqueue_fast_tiers(c); if (rc) return rc;
        rc = enqueue_fast_finish(c); if (rc) return rc;
    } else {
        int rc = enqueue_general(c); if (rc) return rc;
        if (c.timed) HIP_TRY(hipEventRecord(c.ev[4], st));
    }
    return enqueue_tail(c);
}

// What one call is, beyond its LaunchParams: each entry below fills in its own kind and nothing else.  host: a host-pointer call (null: device buffers on `stream`);
// ext: the shard group's pipelines; reserve_only (srn_index_reserve): size the call's workspace, enqueue nothing
struct CallKind { void* stream = nullptr; const HostRows* host = nullptr; const ExtLists* ext = nullptr; const RowRule* rule = nullptr; bool reserve_only = false, blocking_wait = false; };

// every predict call: plan -> reserve -> enqueue, with the row rule's filter and fill kernels behind the launch sequence
static int predict_core(DeviceState* d, const FlatIndex& ix, const LaunchParams& p_in, const CallKind& kind) {
    const HostRows* const host = kind.host; const ExtLists* const ext = kind.ext; const bool on_device = !host, reserve_only = kind.reserve_only;
    void* const user_stream = kind.stream;
    HIP_TRY(hipSetDevice(d->device));
    LaunchParams p = p_in;
    if (p.nq == 0) return SRN_OK;
    const bool fill = kind.rule && kind.rule->fill;
    if (fill && !device_has_fallback(d)) return fail(SRN_ESTATE, "SRN_FLAG_FILL: the index has no fallback ranking (srn_index_set_fallback)");
    // The row rule (srn_exclude.hip): with something to exclude the launch sequence runs at the internal, wide how_many and writes wide rows -- the workspace's scratch; a
    // host-pointer call's staged rows -- and the filter behind it the caller's.  Where the width is the caller's own, nothing can be excluded: the plain call, no scratch,
    // no filter kernel (fill: in place on the rows) -- but a host-pointer call's rows pass through the filter's buffers all the same: the fill kernel works on device rows
    const uint32_t wide = kind.rule ? (uint32_t)wide_how_many(p.how_many, kind.rule->max_excl, kind.rule->session, p.max_len) : p.how_many;
    const bool excl = wide != p.how_many || (host && fill);
    ExclSpec xs{};
    if (excl) {
        const RowRule& r = *kind.rule;
        xs = ExclSpec{r.max_excl ? r.x_flat : nullptr, r.max_excl ? r.x_off : nullptr, r.max_excl, r.session, p.how_many, p.out_ids, p.out_scores, p.out_counts};
        p.how_many = wide; p.out_ids = nullptr; p.out_scores = nullptr; p.out_counts = nullptr;
    }
    // SRN_FLAG_INPUTS_RESIDENT (device-pointer calls): the query buffers are complete in device memory at call time, so the prep kernel of THIS call may run on a side
    // stream while the previous call's kernels still occupy the caller's stream (enqueue_front_resident); the kernels never see the flag
    const bool resident = on_device && !ext && (p.flags & SRN_FLAG_INPUTS_RESIDENT) != 0u;
    p.flags &= ~(unsigned)SRN_FLAG_INPUTS_RESIDENT;
    // the index's result cache, if one is enabled and the caller does not rule it out: this call's own reference (srn_index_result_cache_disable may run beside it)
    const bool no_cache = (p.flags & kFlagNoResultCache) != 0u; p.flags &= ~kFlagNoResultCache;
    const std::shared_ptr<ResultCache> rcache = device_result_cache(d);
    // item-sharded index, lists mode (device_shard_lists_*): the posting lists of ALL shards for this batch arrive in one gathered
    // buffer with the prep records already written against it; everything below runs unchanged on "an index whose postings live there"
    DeviceIndex di = d->di;
    if (ext) di.post_rank = ext->post_rank;
    p.phase_cycles = d->phase_on ? d->d_phase : nullptr;
    Workspace* w = ws_acquire(d, on_device, user_stream);
    if (!w) return fail(SRN_EHIP, "cannot create HIP stream / events");
    struct Rel { DeviceState* d; Workspace* w; bool b; ~Rel() { if (w) ws_release(d, w, b); } } rel{d, w, on_device};
    hipStream_t st = on_device ? (hipStream_t)user_stream : w->stream;
    Geometry geo; { int rc = make_geometry(d, ix, p, 0, geo); if (rc) return rc; }

    if (host && !host->stats && !host->nb_rank && !excl) {
        if (p.nq <= (uint32_t)knobs().tiny_max && !d->phase_on) {
            const int rc = device_predict_tiny(d, ix, w, geo, p, host->items, host->q_off, host->ids, host->scores, host->counts, kind.blocking_wait);
            if (rc != 1) { if (rcache) rcache->bypassed.fetch_add(1, std::memory_order_relaxed); return rc; }   // (1: some query needs the global-table pass -- the paths below have it)
        }
        // everything larger: chunks through pinned staging, uploads / kernels / downloads overlapped (srn_hostpipe.hip); each chunk comes back here as a
        // device-pointer call on one of the pipeline's kernel streams.  (This call's own workspace goes back to the pool first.)
        ws_release(d, w, false); rel.w = nullptr;
        return device_predict_host_pipelined(d, ix, p, host->items, host->q_off, host->ids, host->scores, host->counts);
    }
    // ---- plan -> reserve -> enqueue ----
    if (host) { int rc = stage_host_inputs(w, st, p, *host); if (rc) return rc; }   // (p.stats / p.nb_rank decide the plan)
    if (excl) { int rc = on_device ? exclude_wide_room(w, p.nq, p.how_many, &p.out_ids, &p.out_scores, &p.out_counts) : exclude_host_room(w, st, p.nq, xs); if (rc) return rc; }
    const LaunchPlan pl = make_plan(d, ix, p, geo, ext, resident, w, no_cache ? nullptr : rcache.get());
    BatchCall c{d, w, pl, ext, st, di, p}; c.rcache = rcache.get();
    if (rcache && !pl.cache && !reserve_only) rcache->bypassed.fetch_add(1, std::memory_order_relaxed);
    { int rc = reserve_batch(w, pl, c.p, ext, c.ob); if (rc) return rc; }
    if (reserve_only) return SRN_OK;   // (srn_index_reserve: the workspace is sized, nothing was enqueued)
    if (ext && ext->mode != 0 && !pl.fast.fast) return fail(SRN_EINVAL, "the neighbours pipeline needs the fast kernel's query shape (device_fast_eligible)");
    if (ext && ext->prep_stride != pl.prep_stride) return fail(SRN_EINVAL, "prep record stride mismatch");
    if (ext && ext->mode == 1) return enqueue_shard_front(c);
    { int rc = enqueue_batch(c, on_device); if (rc) return rc; }
    if (excl) HIP_TRY(launch_exclude(st, p.nq, p.out_ids, p.out_scores, p.out_counts, p.how_many, xs.x_flat, xs.x_off, xs.max_excl, xs.session ? p.items_flat : nullptr, p.q_off,
                                     xs.out_ids, xs.out_scores, xs.out_counts, xs.how_many));
    // the fallback ranking (srn_fill.hip): short rows of the call's final rows -- the filter's, or the launch sequence's own -- are filled in place; what the launch sequence
    // merged or cached above are the unfilled rows
    if (fill) HIP_TRY(excl ? launch_fill(st, d, p.nq, xs.out_ids, xs.out_scores, xs.out_counts, xs.how_many, xs.x_flat, xs.x_off, p.items_flat, p.q_off, xs.session, (p.flags & SRN_FLAG_BUSINESS_LOGIC) != 0u)
                           : launch_fill(st, d, p.nq, p.out_ids, p.out_scores, p.out_counts, p.how_many, nullptr, nullptr, p.items_flat, p.q_off, false, (p.flags & SRN_FLAG_BUSINESS_LOGIC) != 0u));
    if (excl && host) return exclude_fetch_host(st, p.nq, xs, host->ids, host->scores, host->counts);
    return host ? fetch_host_outputs(c, *host) : SRN_OK;
}

int device_predict_device(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, void* stream, const RowRule& rule) {
    CallKind kind; kind.stream = stream; kind.rule = &rule;
    return predict_core(d, ix, p, kind);
}
int device_predict_host(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, const HostRows& rows, const RowRule& rule, bool blocking_wait) {
    if ((rows.stats || rows.nb_rank) && (rule.max_excl || rule.session || rule.fill)) return fail(SRN_EINVAL, "exclusion lists, SRN_FLAG_FILL: batch calls without statistics or the neighbour dump only");
    CallKind kind; kind.host = &rows; kind.rule = &rule; kind.blocking_wait = blocking_wait;
    return predict_core(d, ix, p, kind);
}
// the shard group's three pipelines: device buffers, prep records and posting lists from the exchange (ExtLists)
static int predict_ext(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, void* stream, const ExtLists& ext) {
    CallKind kind; kind.stream = stream; kind.ext = &ext;
    return predict_core(d, ix, p, kind);
}

// One stage of the item-sharded pipeline (see ShardIO, ShardCall).  Like the unsharded launch sequence, a stage has a second pass with its tables in global memory for
// the queries whose session or item table does not fit LDS (numerator slots only: with position sets the shard group runs the lists pipeline); a query that fits
// neither pass comes back marked 0xFFFFFFFF.
int device_shard_stage(const ShardCall& c, int stage, const LaunchParams& p_in, const ShardIO& sh) {
    DeviceState* d = c.d; const FlatIndex& ix = *c.ix; void* stream = c.stream;
    HIP_TRY(hipSetDevice(d->device));
    LaunchParams p = p_in;
    if (p.nq == 0) return SRN_OK;
    p.phase_cycles = nullptr;
    Geometry geo;
    const uint32_t sort_room = stage == 2 ? (uint32_t)ceil_pow2(std::max<uint32_t>(p.k, 2)) * 8 : 0;   // stage B sorts the neighbour list in region B
    int rc = make_geometry(d, ix, p, sort_room, geo); if (rc) return rc;
    const uint32_t blocks_per_cu = std::max<uint32_t>(1, (160 * 1024) / (uint32_t)geo.lds);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(p.nq, (uint64_t)d->n_cu * std::min<uint32_t>(blocks_per_cu, 2048 / kBlock) * 4);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (stage < 1 || stage > 3) return fail(SRN_EINVAL, "bad stage");
    const bool retry = !geo.masks && (geo.sess_may_overflow || geo.item_may_overflow);
    Workspace* w = nullptr;
    struct Rel { DeviceState* d; Workspace* w; ~Rel() { if (w) ws_release(d, w, true); } } rel{d, nullptr};
    KernelCfg cg = geo.c; uint64_t g_stride = 0; int retry_blocks = 0;
    if (retry) {
        w = ws_acquire(d, true, stream); rel.w = w;
        if (!w) return fail(SRN_EHIP, "cannot create HIP stream / events");
        rc = ensure_list(&w->retry_list, &w->retry_cap, p.nq, (size_t)p.nq * 4 + 64); if (rc) return rc;
        global_tables_geometry(d, geo, cg, g_stride, retry_blocks);
        rc = ensure(&w->gscratch, &w->gscratch_bytes, g_stride * retry_blocks); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(w->retry_cnt, 0, 4, st));
    }
    PredictLaunch a; a.masks = geo.masks; a.slot64 = geo.slot64; a.stage = stage; a.sh = sh;
    if (w) { a.retry_list = w->retry_list; a.retry_cnt = w->retry_cnt; }
    e = launch_predict(a, dim3(grid), geo.lds, st, d->di, p, geo.c);
    if (e != hipSuccess) return fail(SRN_EHIP, std::string("shard stage launch: ") + hipGetErrorString(e));
    if (retry) {
        PredictLaunch g; g.slot64 = geo.slot64; g.global_tables = true; g.stage = stage; g.sh = sh; g.qlist = w->retry_list; g.qn = w->retry_cnt; g.gscratch = w->gscratch; g.gstride = g_stride;
        e = launch_predict(g, dim3(retry_blocks), geo.c.off_a, st, d->di, p, cg);
        if (e != hipSuccess) return fail(SRN_EHIP, std::string("shard stage launch (global tables): ") + hipGetErrorString(e));
    }
    return SRN_OK;
}
// ---- item-sharded index, lists mode (srn_shard.hip): the steps either side of the exchanges; device buffers, asynchronous on `stream` ----
bool device_shard_lists_supported(DeviceState* d, const FlatIndex& ix, const LaunchParams& p) {
    Geometry g;
    return make_geometry(d, ix, p, 0, g) == SRN_OK && g.masks && (p.flags & ~(unsigned)SRN_FLAG_BUSINESS_LOGIC) == 0 && p.stats == nullptr && p.nb_rank == nullptr;
}
// the batch shape the fast kernel takes (the same test a predict call makes): what the shard group's neighbours pipeline needs on top of lists mode
// (the shard group's choice of pipeline must be the SAME on every rank: `max_row_len_all` = the longest row of the whole index -- a shard's own longest fragment differs from
//  rank to rank and is never longer -- and the packed rows, which device_attach may fail to allocate on ONE rank, are checked where the postings are set, not here)
bool device_fast_eligible(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, uint64_t max_row_len_all) {
    Geometry geo;
    if (make_geometry(d, ix, p, 0, geo) != SRN_OK) return false;
    const Knobs kn = knobs();
    const int rank_bits_f = std::max(1, bits_host(ix.n_kept ? ix.n_kept - 1 : 0));
    const bool wraps = max_row_len_all ? sketch_wraps(p.k, std::max<uint64_t>(max_row_len_all, ix.max_row_len), p.max_len) : geo.sketch_may_wrap;
    return (max_row_len_all != 0 || d->fast.row_packed != nullptr) && geo.masks && !wraps && rank_bits_f <= 29 && kn.geometry_default() && !kn.no_fast && p.k <= F_K_MAX && p.m <= F_M_MAX &&
           p.how_many <= 24 && (p.flags & ~(unsigned)SRN_FLAG_BUSINESS_LOGIC) == 0 && p.stats == nullptr && p.nb_rank == nullptr && p.max_len <= 8;
}
uint32_t device_prep_stride(uint32_t max_len) { return prep_stride_of(max_len); }
int device_shard_lists_head(const ShardCall& c, const LaunchParams& p, void* pos, int* head) {
    HIP_TRY(hipSetDevice(c.d->device));
    if (p.nq == 0) return SRN_OK;
    HIP_TRY(launch_shard_lists_head((hipStream_t)c.stream, c.d->di, p.items_flat, p.q_off, p.nq, p.m, p.max_len, (ShardPos*)pos, head));
    return SRN_OK;
}
int device_shard_lists_count(const ShardCall& c, const LaunchParams& p, const void* pos, const int* head, uint32_t* kept, int* tot) {
    HIP_TRY(hipSetDevice(c.d->device));
    if (p.nq == 0) return SRN_OK;
    HIP_TRY(launch_shard_lists_count((hipStream_t)c.stream, c.d->di, p.q_off, p.nq, p.max_len, (const ShardPos*)pos, head, kept, tot));
    return SRN_OK;
}
int device_shard_lists_copy(const ShardCall& c, const LaunchParams& p, const void* pos, const uint32_t* kept, const long long* off, uint32_t* out) {
    HIP_TRY(hipSetDevice(c.d->device));
    if (p.nq == 0) return SRN_OK;
    HIP_TRY(launch_shard_lists_copy((hipStream_t)c.stream, c.d->di, p.nq, p.max_len, (const ShardPos*)pos, kept, off, out));
    return SRN_OK;
}
int device_shard_lists_predict(const ShardCall& c, const LaunchParams& p, const ShardLists& l, char* records) {
    DeviceState* d = c.d; const FlatIndex& ix = *c.ix;
    HIP_TRY(hipSetDevice(d->device));
    if (p.nq == 0) return SRN_OK;
    if (l.n_shards != ix.n_shards) return fail(SRN_EINVAL, "n_shards differs from the number of shards this index was cut into");
    if (!device_shard_lists_supported(d, ix, p)) return fail(SRN_EINVAL, "lists mode needs position-set slots (sessions of <= 8 items, m <= m_index, complete lists): use the three-stage pipeline");
    const uint32_t stride = device_prep_stride(p.max_len);
    HIP_TRY(launch_shard_prep((hipStream_t)c.stream, p.items_flat, p.q_off, p.nq, p.max_len, l.n_shards, l.kept_g, l.off_g, 0ull, l.head, (const ShardPos*)l.pos_local, records, stride, fast_nb(ix, knobs()) == 3u, l.shard_base, l.direct));
    ExtLists ext{records, stride, l.direct ? d->di.post_rank : l.lists_g};
    return predict_ext(d, ix, p, c.stream, ext);
}

// ---- item-sharded index, neighbours pipeline (round 4): the posting lists are replicated (c.post = the device state of the whole index or of its postings-only view),
// the rows stay sharded.  The record of a query is the same on every rank except for the dense idx of its items (this shard's numbering).
int device_shard_nb_prep(const ShardCall& c, const LaunchParams& p, char* records, char** order_buf, size_t* order_bytes, const unsigned long long** order_out) {
    DeviceState* d = c.d;
    HIP_TRY(hipSetDevice(d->device));
    *order_out = nullptr;
    if (p.nq == 0) return SRN_OK;
    const Knobs kn = knobs();
    const bool ordered = kn.order_min > 0 && p.nq >= (uint32_t)kn.order_min;
    OrderBufs ob;
    if (ordered) { int rc = order_room(order_buf, order_bytes, p.nq, &ob); if (rc) return rc; }
    HIP_TRY(launch_prep((hipStream_t)c.stream, c.post->di, p.items_flat, p.q_off, p.nq, p.m, p.max_len, records, device_prep_stride(p.max_len), fast_nb_of(d->di.n_kept, kn) == 3u /* (the fronting kernel runs on d's index) */, nullptr, nullptr, d->di.id_table, d->di.id_mask, ob.keys_in));
    if (ordered) { HIP_TRY(sort_order_keys((hipStream_t)c.stream, ob.keys_in, ob.keys_out, p.nq, ob.temp, &ob.temp_bytes)); *order_out = ob.keys_out; }
    return SRN_OK;
}
int device_shard_nb_run(const ShardCall& c, const LaunchParams& p, const char* records, ExtLists ext) {
    if (ext.q_lo >= p.nq) return SRN_OK;   // (a front end with no query of its own; an empty batch)
    ext.prep = records; ext.prep_stride = device_prep_stride(p.max_len); ext.post_rank = c.post->di.post_rank;
    return predict_ext(c.d, *c.ix, p, c.stream, ext);
}
// (the streaming form's exchange format, srn_sback.hip)
int device_shard_nb_positions(const ShardCall& c, const LaunchParams& p, const char* records, const ShardXchg& in, const ShardXchg& out, uint32_t q_lo) {
    if (q_lo >= p.nq) return SRN_OK;
    HIP_TRY(hipSetDevice(c.d->device));
    const uint32_t grid = (uint32_t)std::min<uint64_t>(p.nq - q_lo, (uint64_t)c.d->n_cu * 16 * 4);
    HIP_TRY(launch_shard_nb_positions(dim3(grid), (hipStream_t)c.stream, records, device_prep_stride(p.max_len), p.max_len, in.words, in.stride, out.words, out.stride, c.post->di.post_rank, q_lo, p.nq, p.m,
                                      fast_nb(*c.ix, knobs()) == 3u));
    return SRN_OK;
}
// words per query of that format for this batch shape, 0 if the batch (or this build's knobs) has no streaming form: RANK-INVARIANT inputs only
uint32_t device_shard_nb_positions_stride(const LaunchParams& p) {
    const Knobs kn = knobs();
    if (kn.no_sback_stream || kn.no_sback || p.max_len > 8) return 0u;
    return shard_nb_positions_stride(p.k, p.m);
}

int device_slot_bytes(DeviceState* d, const FlatIndex& ix, uint32_t max_len, uint32_t* num_bits) {   // element size of the packed candidate / neighbour buffers
    const LaunchParams p = launch_params(0, 1, 1, 0, 0, max_len); Geometry g;
    if (make_geometry(d, ix, p, 0, g) != SRN_OK) return -1;
    if (num_bits) *num_bits = g.c.num_bits;
    return (int)g.slot_bytes;
}

int device_debug_geometry(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, uint32_t* out24) {   // (host code only: no launch, no hipSetDevice)
    Geometry g;
    const int rc = make_geometry(d, ix, p, 0, g); if (rc) return rc;   // (min_region_b = 0: what predict_core passes)
    const KernelCfg& c = g.c;
    const uint32_t w[24] = {g.masks ? 1u : 0u, g.slot64 ? 1u : 0u, g.slot_bytes, (uint32_t)g.lds, g.sess_may_overflow ? 1u : 0u, g.item_may_overflow ? 1u : 0u, g.sketch_may_wrap ? 1u : 0u,
                            (uint32_t)std::min(d->lds_per_block_max, 160 * 1024),
                            c.sess_slots, c.item_slots, c.item_buckets, c.hot_slots, c.sketch_slots, c.sketch_shift, c.sum_bits, c.num_bits, c.q_cap,
                            c.off_q, c.off_wave, c.off_b, c.off_a, c.region_a_bytes, c.no_merge, 0u};
    static_assert(sizeof(KernelCfg) == 15 * 4, "srn_debug_geometry reports every word of KernelCfg: a new word belongs in the list above");
    for (int i = 0; i < 24; ++i) out24[i] = w[i];
    return SRN_OK;
}

int device_last_kernel_ms(DeviceState* d, double* ms_main, double* ms_retry, uint32_t* retried) {
    HIP_TRY(hipSetDevice(d->device));
    Workspace* w;
    { std::lock_guard<std::mutex> lk(d->mu); w = d->last_ws; }
    if (!w || !(w->calls + w->untimed_calls)) return fail(SRN_EINVAL, "no timed predict call yet");
    if (w->last_untimed) return fail(SRN_EINVAL, "the last call took the latency path (<= 256 sessions on host pointers): it records no events");
    if (!w->ring_timed[(w->calls - 1) % Workspace::RING]) return fail(SRN_EINVAL, "kernel timing is off: srn_kernel_timing(idx, 1) before the calls to be timed");
    hipEvent_t* ev = w->ev[(w->calls - 1) % Workspace::RING];
    HIP_TRY(hipEventSynchronize(ev[2]));
    float a = 0, b = 0;
    HIP_TRY(hipEventElapsedTime(&a, ev[3], ev[1]));   // the predict kernel alone (the prep kernel runs between ev[0] and ev[3])
    HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
    if (ms_main) *ms_main = a;
    if (ms_retry) *ms_retry = b;
    if (retried) *retried = w->last_retry ? w->h_retry[HW_GLOBAL] : 0;
    return SRN_OK;
}

// how the last call's queries were served: by the fast kernel / handed to the general kernel / through the global-table pass
// Sizes the workspace bound to `stream` for device-pointer calls of up to nq queries with these parameters, so that
// srn_predict_batch_device allocates nothing (hipMalloc / hipFree synchronise the device) once traffic starts.
int device_reserve(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, void* stream) {
    CallKind kind; kind.stream = stream; kind.reserve_only = true;
    return predict_core(d, ix, p, kind);
}

int device_last_path_counts(DeviceState* d, uint32_t* nq, uint32_t* general, uint32_t* global_pass) {
    HIP_TRY(hipSetDevice(d->device));
    Workspace* w;
    { std::lock_guard<std::mutex> lk(d->mu); w = d->last_ws; }
    if (!w || !(w->calls + w->untimed_calls)) return fail(SRN_EINVAL, "no predict call yet");
    if (!w->last_untimed) HIP_TRY(hipEventSynchronize(w->ev[(w->calls - 1) % Workspace::RING][2]));   // (the latency path returns with its stream idle)
    if (nq) *nq = w->last_nq;
    if (general) *general = w->last_fast ? w->h_retry[HW_GENERAL] : w->last_nq;
    if (global_pass) *global_pass = w->last_retry ? w->h_retry[HW_GLOBAL] : 0;
    return SRN_OK;
}
int device_debug_prep_records(DeviceState* d, const FlatIndex& ix, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t m, size_t max_len, void* out, size_t cap_bytes, size_t* out_stride) {
    if (!q_off || !out_stride || (nq && !out)) return fail(SRN_EINVAL, "null buffer");
    if (nq > (1u << 24) || m == 0 || m > 0xFFFFFFFFull || max_len == 0 || max_len > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "srn_debug_prep_records: sizes out of range");
    for (size_t q = 0; q < nq; ++q) if (q_off[q + 1] < q_off[q]) return fail(SRN_EINVAL, "srn_debug_prep_records: q_off must not decrease");
    const uint32_t stride = prep_stride_of((uint32_t)max_len);
    *out_stride = stride;
    if (nq == 0) return SRN_OK;
    const size_t n_items = q_off[nq], rec_bytes = nq * (size_t)stride;
    if (n_items && !items_flat) return fail(SRN_EINVAL, "null buffer");
    if (cap_bytes < rec_bytes) return fail(SRN_ERANGE, "srn_debug_prep_records: the output buffer is too small");
    HIP_TRY(hipSetDevice(d->device));
    const size_t items_bytes = (n_items + 1) * 8, off_bytes = ((nq + 1) * 4 + 7) & ~(size_t)7;
    void* mem = nullptr;
    if (hipMalloc(&mem, items_bytes + off_bytes + rec_bytes) != hipSuccess) { (void)hipGetLastError(); return fail(SRN_ENOMEM, "srn_debug_prep_records: hipMalloc failed"); }
    uint64_t* d_items = (uint64_t*)mem; uint32_t* d_off = (uint32_t*)((char*)mem + items_bytes); char* d_rec = (char*)mem + items_bytes + off_bytes;
    hipError_t e = hipMemset(d_rec, 0, rec_bytes);   // (a session of 0 or of > max_len items has no item entries: they read as zeros)
    if (e == hipSuccess && n_items) e = hipMemcpy(d_items, items_flat, n_items * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_off, q_off, (nq + 1) * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_prep(0, d->di, d_items, d_off, (uint32_t)nq, (uint32_t)m, (uint32_t)max_len, d_rec, stride, fast_nb(ix, knobs()) == 3u);
    if (e == hipSuccess) e = hipMemcpy(out, d_rec, rec_bytes, hipMemcpyDeviceToHost);   // (the null stream: the copy waits for the kernel)
    (void)hipFree(mem);
    if (e != hipSuccess) return fail(SRN_EHIP, std::string("srn_debug_prep_records: ") + hipGetErrorString(e));
    return SRN_OK;
}
int device_last_mid_count(DeviceState* d, uint32_t* listed, uint32_t* big_listed) {   // queries the last call's lean fast kernel listed for the MID instantiation (0: no such tier in that call)
    uint32_t nq = 0;
    const int rc = device_last_path_counts(d, &nq, nullptr, nullptr);   // (waits for the call's end)
    if (rc != SRN_OK) return rc;
    Workspace* w;
    { std::lock_guard<std::mutex> lk(d->mu); w = d->last_ws; }
    if (listed) *listed = w->last_fast && w->last_mid ? w->h_retry[HW_MID] : 0u;
    if (big_listed) *big_listed = w->last_fast ? w->h_retry[HW_BIGQ] : 0u;   // (the BIG form also takes the lean shape's oversized queries: no MID tier needed)
    return SRN_OK;
}

int device_last_dedup_count(DeviceState* d, uint32_t* merged) {   // queries of the last call that were not served but got the row of an equal, earlier query of the call (0: the call did not merge)
    const int rc = device_last_path_counts(d, nullptr, nullptr, nullptr);   // (waits for the call's end)
    if (rc != SRN_OK) return rc;
    Workspace* w;
    { std::lock_guard<std::mutex> lk(d->mu); w = d->last_ws; }
    if (merged) *merged = w->last_dedup ? w->h_retry[HW_MERGED] : 0u;
    return SRN_OK;
}

int device_last_light_count(DeviceState* d, uint32_t* light) {   // light representatives of the last call: served by vmis_light_kernel or handed on by it (0: the form was off in that call)
    const int rc = device_last_path_counts(d, nullptr, nullptr, nullptr);   // (waits for the call's end)
    if (rc != SRN_OK) return rc;
    Workspace* w;
    { std::lock_guard<std::mutex> lk(d->mu); w = d->last_ws; }
    if (light) *light = w->last_light ? w->h_retry[HW_LIGHT] : 0u;
    return SRN_OK;
}

int device_kernel_timing(DeviceState* d, int enable) { d->timing.store(enable != 0, std::memory_order_relaxed); return SRN_OK; }

int device_phase_cycles(DeviceState* d, int enable, unsigned long long* out16) {
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipDeviceSynchronize());
    if (!d->d_phase) { HIP_TRY(hipMalloc((void**)&d->d_phase, 16 * 8)); d->allocs.push_back(d->d_phase); HIP_TRY(hipMemset(d->d_phase, 0, 16 * 8)); }
    if (out16) HIP_TRY(hipMemcpy(out16, d->d_phase, 16 * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(d->d_phase, 0, 16 * 8));
    d->phase_on = enable != 0;
    return SRN_OK;
}

// durations of the most recent min(max_n, calls, RING) predict launches of the last-used workspace, oldest first
int device_kernel_times(DeviceState* d, uint32_t max_n, double* ms_main, double* ms_retry, uint32_t* out_n, double* ms_prep, double* ms_fast) {
    HIP_TRY(hipSetDevice(d->device));
    Workspace* w;
    { std::lock_guard<std::mutex> lk(d->mu); w = d->last_ws; }
    *out_n = 0;
    if (!w || !w->calls) return SRN_OK;
    uint64_t n = std::min<uint64_t>(std::min<uint64_t>(max_n, w->calls), Workspace::RING);
    { uint64_t timed = 0; while (timed < n && w->ring_timed[(w->calls - 1 - timed) % Workspace::RING]) ++timed; n = timed; }   // the trailing run of timed calls (srn_kernel_timing)
    if (!n) return SRN_OK;
    HIP_TRY(hipEventSynchronize(w->ev[(w->calls - 1) % Workspace::RING][2]));
    for (uint64_t i = 0; i < n; ++i) {
        hipEvent_t* ev = w->ev[(w->calls - n + i) % Workspace::RING];
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, ev[3], ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
        if (ms_main) ms_main[i] = a;
        if (ms_retry) ms_retry[i] = b;
        if (ms_prep) { float c2 = 0; HIP_TRY(hipEventElapsedTime(&c2, ev[0], ev[3])); ms_prep[i] = c2; }
        if (ms_fast) { float c2 = 0; HIP_TRY(hipEventElapsedTime(&c2, ev[3], ev[4])); ms_fast[i] = c2; }
    }
    *out_n = (uint32_t)n;
    return SRN_OK;
}

}  // namespace srn
