// Internal declarations shared by the host index builder, the C ABI glue and the HIP kernels.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/serenade_hip.h"

namespace srn {

// ---- error plumbing (thread-local message behind srn_last_error) ---------------------------
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
std::string last_error_string();   // this thread's message (copied: a combining round hands its leader's error to every member)

// ---- u64 item id -> dense item index: open addressing, 16-byte slots (one load per probe) ----
struct IdSlot {
    uint64_t key;
    uint32_t idx;  // 0xFFFFFFFF = empty
    uint32_t pad;
};
static constexpr uint32_t kNone = 0xFFFFFFFFu;

static inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33; return x;
}

// ---- training sessions (host) ------------------------------------------------------------
struct Sessions {
    std::vector<uint64_t> off, items;
    std::vector<uint32_t> ts;
    std::vector<uint64_t> session_ids;  // original SessionId column, for diagnostics
};
int sessions_from_tsv(const char* path, Sessions& out);
uint64_t sessions_length_quantile(const uint64_t* off, size_t n, double q);
bool parse_tsv_line(const char* p, const char* end, uint64_t& session, uint64_t& item, uint64_t& time);   // one line of sessions_from_tsv (false: skipped)
// the GPU loader (srn_ingest.hip): the same sessions as sessions_from_tsv; info (may be null) gets the load's counts and stage times
int sessions_from_tsv_gpu(const char* path, int device, Sessions& out, srn_load_info_t* info);
int sessions_from_events(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, int device, void* stream,
                         Sessions& out, srn_load_info_t* info);
uint64_t sessions_length_quantile_counting(const uint64_t* off, size_t n, double q);   // = sessions_length_quantile, by counting the lengths
void ingest_reload_knobs();                                                              // SRN_INGEST_CHUNK_BYTES
// a click log's rows on the device and their split by time (srn_ingest.hip, srn_split.hip); arguments already checked by the C ABI glue
int events_from_tsv_gpu(const char* path, int device, srn_events** out);
void events_free(srn_events* e);
int events_split(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, const srn_split_t& split, int device, void* stream,
                 uint8_t* code, uint32_t* pos, srn_split_info_t* info);
int events_take(const uint8_t* code, const uint32_t* pos, size_t n, uint8_t which, const uint64_t* session_ids, const uint64_t* item_ids, const void* times, unsigned flags,
                uint64_t* out_sessions, uint64_t* out_items, void* out_times, int device, void* stream);
void split_reload_knobs();                                                               // SRN_SPLIT_HASH_BITS, SRN_SPLIT_NO_COMBINE
uint32_t split_hash_bits();

// ---- the flat index (host copy).  Layout and invariants: DESIGN.md "Data layout in HBM" ----
struct FlatIndex {
    uint64_t n_items = 0, n_sessions_total = 0, n_kept = 0, nnz_rows = 0, nnz_post = 0;
    uint64_t m_index = 0, max_session_len = 0, max_row_len = 0;
    double idf_weighting = 1.0;
    bool lists_complete = true;             // every posting list holds ALL sessions of its item that are at least as recent as its last entry (and is complete if
                                            // shorter than m_index): true for every index built here; a pre-built (Avro) index may not satisfy it -- then the
                                            // first-match position comes from the rows (the reference's contains() test), not from posting-list membership
    std::vector<uint32_t> viol;             // [n_items] iff !lists_complete on an index whose loader measured it (srn_avro.cpp): 1 + the most recent rank of a LISTED session whose row holds the
                                            // item but which the item's list does not name (0: none; 0xFFFFFFFF: the list names a session without the item).  A query whose items all have
                                            // viol <= its cut x_lo is exact on the position-set path; the prep kernel flags the others for the general kernel's row pass
    bool postings_only = false;             // the REPLICATED part of an item-sharded index (srn_index_postings_view): dictionary, idf / attributes and posting lists of the whole index,
                                            // no rows -- what every rank of a shard group keeps beside its shard for the neighbours pipeline; answers no predict call itself
    uint32_t shard = 0, n_shards = 1;       // item-sharded index: this shard holds the items with owner(id) == shard
    uint64_t total_pairs = 0;               // (session,item) pairs of ALL kept sessions = idf numerator (== nnz_rows when unsharded)
    std::vector<uint64_t> item_id;          // [n_items]   public id of each dense idx; idx = popularity order (count desc, id asc)
    std::vector<uint32_t> id_rank;          // [n_items]   rank of the public id in ascending order (final tie-break key)
    std::vector<double> idf;                // [n_items]
    std::vector<uint8_t> attr;              // [n_items]   SRN_ATTR_* or SRN_ATTR_NONE
    std::vector<uint64_t> post_off;         // [n_items+1]
    std::vector<uint32_t> post_rank;        // [nnz_post]  recency ranks, strictly descending per item
    std::vector<uint64_t> row_off;          // [n_kept+1]  rows addressed by recency rank
    std::vector<uint32_t> row_items;        // [nnz_rows]  item idx (row order = ascending public id, as handed in)
    std::vector<uint32_t> rank_to_session;  // [n_kept]    reference session index of each rank
    std::vector<IdSlot> id_table;           // power-of-two open addressing table
    uint32_t id_mask = 0;
    uint32_t lookup(uint64_t id) const {
        if (id_table.empty()) return kNone;
        uint32_t h = (uint32_t)mix64(id) & id_mask;
        for (;;) { const IdSlot& s = id_table[h]; if (s.idx == kNone) return kNone; if (s.key == id) return s.idx; h = (h + 1) & id_mask; }
    }
};
int build_flat_index(const srn_sessions_view_t& v, size_t m_index, size_t max_session_len, double idf_weighting,
                     uint32_t shard, uint32_t n_shards, FlatIndex& out);
static inline uint32_t item_owner(uint64_t id, uint32_t n_shards) { return (uint32_t)(mix64(id ^ 0x9E3779B97F4A7C15ull) % n_shards); }
int build_flat_index_gpu(const srn_sessions_view_t& v, size_t m_index, size_t max_session_len, double idf_weighting, int device,
                         FlatIndex& out);   // same result, built with rocPRIM sorts on the GPU (srn_build_gpu.hip)
int build_flat_index_from_avro(const char* base_path, FlatIndex& out);   // <base>/itemindex/*.avro + <base>/sessionindex/*.avro (srn_avro.cpp)
int shard_flat_index(const FlatIndex& full, uint32_t shard, uint32_t n_shards, FlatIndex& out);   // shard `shard` of an unsharded index (same bytes as build_flat_index(..., shard, n_shards))
int check_has_rows(const FlatIndex& ix, const char* what);   // SRN_EINVAL for a postings-only view (srn_index_postings_view): it has no rows to cut, save, shard or serve from
int save_flat_index(const FlatIndex& ix, const char* path);
int load_flat_index(const char* path, FlatIndex& ix);

// ---- device side ---------------------------------------------------------------------------
struct ItemMeta {   // one 16-byte gather per scored item
    double idf;
    uint32_t id_rank;   // rank of the public id (ascending): tie-break key of the final ranking
    uint32_t attr;      // SRN_ATTR_* byte
};
struct alignas(16) RowQuad { uint32_t x, y, z, w; };
struct DeviceIndex {  // pointers into HBM; passed by value to the kernels
    const IdSlot* id_table; uint32_t id_mask;
    const ItemMeta* meta;        // [n_items] by dense idx
    const uint64_t* id_sorted;   // [n_items] public ids ascending (indexed by id_rank)
    const uint64_t* post_off; const uint32_t* post_rank;
    const uint32_t* viol;        // [n_items] or null (every list complete): FlatIndex::viol -- the prep kernel sets PrepHead::unsafe from it
    // Rows in HBM: one 64-byte, 64-byte-aligned slot per session, addressed by recency rank -- ONE line fetch per
    // neighbour and no offset lookup.  word 0 = row length; length <= 15: words 1..15 hold the items; longer rows:
    // word 1 = offset (in items) of items 14.. in row_ext, words 2..15 = items 0..13.
    const RowQuad* row_slots;   // 4 quads per slot
    const uint32_t* row_ext;
    uint32_t n_items, n_kept;
    uint32_t row_frag;       // item shards (n_shards > 1): row_slots holds 16-byte FRAGMENT slots instead -- {len, i0, i1, i2}, or {len, offset in row_ext, i0, i1} with
                             // items 2.. in row_ext when the fragment has > 3 items: a shard sees ~len / n_shards items of a row, so its row memory is 16 B per session, not 64
    double idf_hi, idf_lo;   // max / min over items of (idf > 0 ? idf : 1)
};

struct LaunchParams {
    uint32_t nq, k, m, how_many, flags, max_len;
    const uint64_t* items_flat; const uint32_t* q_off;   // device
    uint64_t* out_ids; double* out_scores; uint32_t* out_counts;   // device
    uint32_t* stats;      // [nq*8] or null
    uint32_t* nb_rank; uint32_t* nb_num; uint32_t* nb_cnt;   // debug neighbour dump or null
    unsigned long long* phase_cycles;                       // [16] per-phase shader cycles (debug) or null
    const char* prep; uint32_t prep_stride;                 // per-query records of the prep kernel (or null: translate in the main kernel)
};

struct Workspace;   // per-call device scratch + events, owned by the index handle's pool
struct DeviceState;  // uploaded arrays + workspace pool

DeviceState* device_attach(const FlatIndex& ix, int device);   // nullptr on failure (error set)
// ... of an index whose builder left its four large arrays on the device (srn_index_from_events_device): post_rank becomes the served array, the rows are laid out from
// row_off / row_items in place, and those two and rank_to_session stay as residue until device_materialize copies all four into ix and frees what serving does not read.
// ix: the scalars and the per-item arrays.  The allocations belong to the attach from the call on, also when it fails
struct ResidentArrays { void* post_rank; void* row_off; void* row_items; void* rank_to_session; };
DeviceState* device_attach_resident(const FlatIndex& ix, int device, const ResidentArrays& a);
int device_materialize(DeviceState* d, FlatIndex& ix);
uint64_t device_residue_bytes(const DeviceState* d);   // bytes of the residue still on the device (part of device_bytes)
// the block_base arrays of launch_rows_to_slots / launch_rows_to_packed from row offsets on the device (srn_build_gpu.hip): totals = {overflow items + 16, overflow blocks + 1, longest row}
int row_block_bases(const uint64_t* d_row_off, uint64_t n_rows, bool frag, uint32_t* d_base_ext, uint32_t* d_base_packed, uint64_t totals[3]);
void device_release(DeviceState* d);
int device_update_attr(DeviceState* d, const FlatIndex& ix);
void device_refresh_fast_bounds(DeviceState* d, const FlatIndex& ix);   // idf bounds of the fast kernel's integer floors (srn_runtime.hip)
void reload_knobs();                                                     // re-read the SRN_* test / experiment knobs from the environment
uint64_t device_bytes(const DeviceState* d);
// item-sharded index, lists mode: prep records (PrepHead + max_len * PrepItem per query) written against a gathered posting buffer
// the neighbours pipeline's exchange buffer as one rank's kernels see it: `stride` words per query; positions: position records (device_shard_nb_positions: the
// streaming back end's format), not neighbour slots
struct ShardXchg { uint32_t* words = nullptr; uint32_t stride = 0; bool positions = false; };
struct ExtLists { const char* prep; uint32_t prep_stride; const uint32_t* post_rank;
                  // the shard group's neighbours pipeline: mode 1 = front end only (neighbour lists of the queries [q_lo, nq) -> x), 2 = back end (neighbour lists <- x)
                  int mode = 0; ShardXchg x; uint32_t q_lo = 0;
                  const unsigned long long* order = nullptr; };   // mode 2: the batch's serving order (device_shard_nb_prep sorted it), or null
// ---- the predict call.  Every entry takes the caller's OWN how_many (and, on device buffers, the caller's own rows) in LaunchParams ----
inline LaunchParams launch_params(size_t nq, size_t k, size_t m, size_t how_many, unsigned flags, size_t max_len, const uint64_t* items_flat = nullptr, const uint32_t* q_off = nullptr,
                                  uint64_t* out_ids = nullptr, double* out_scores = nullptr, uint32_t* out_counts = nullptr) {
    LaunchParams p{};
    p.nq = (uint32_t)nq; p.k = (uint32_t)k; p.m = (uint32_t)m; p.how_many = (uint32_t)how_many; p.flags = flags; p.max_len = (uint32_t)max_len;
    p.items_flat = items_flat; p.q_off = q_off; p.out_ids = out_ids; p.out_scores = out_scores; p.out_counts = out_counts;
    return p;
}
// a host-pointer call's buffers, copied in and out by the call; stats [nq * 8] and the neighbour dump (all three or none) may be null
struct HostRows { const uint64_t* items; const uint32_t* q_off; uint64_t* ids; double* scores; uint32_t* counts;
                  uint32_t* stats = nullptr; uint32_t* nb_rank = nullptr; uint32_t* nb_num = nullptr; uint32_t* nb_cnt = nullptr; };
// What happens to a call's rows behind the launch sequence (srn_exclude.hip, srn_fill.hip).  x_flat / x_off: the exclusion CSR, at most max_excl ids per
// query (null with max_excl 0; device pointers for device_predict_device, host pointers for device_predict_host); session: the items of the query's own session are excluded
// too (SRN_FLAG_EXCLUDE_SESSION); fill (SRN_FLAG_FILL): short rows are then filled in place from the index's fallback ranking (SRN_ESTATE without one).  The callers strip
// these flags from LaunchParams::flags: the kernels never see them.  With something to exclude the launch sequence runs at the internal how_many wide_how_many() into wide
// rows of the call's workspace and the filter kernel behind it writes the caller's; where that width is the caller's how_many nothing can be excluded and the call is the plain one
struct RowRule { const uint64_t* x_flat = nullptr; const uint32_t* x_off = nullptr; uint32_t max_excl = 0; bool session = false; bool fill = false; };
inline size_t wide_how_many(size_t how_many, size_t max_excl, bool session, size_t max_len) { return how_many + max_excl + (session ? max_len - 1 : 0); }
// device buffers, asynchronous on `stream` (SRN_FLAG_INPUTS_RESIDENT and kFlagNoResultCache in p.flags are consumed here)
int device_predict_device(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, void* stream, const RowRule& rule = {});
// host buffers; returns with the rows in place.  Small batches take the latency path (blocking_wait: it sleeps on an interrupt instead of spinning), larger ones the chunked
// pipeline; stats, the neighbour dump and a rule that filters go through one staged workspace (a rule together with stats or the dump: SRN_EINVAL)
int device_predict_host(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, const HostRows& rows, const RowRule& rule = {}, bool blocking_wait = false);
template <typename F> inline int guarded(F f) {   // every extern "C" entry that can throw: never let an exception cross the C boundary
    try { return f(); }
    catch (const std::bad_alloc&) { return fail(SRN_ENOMEM, "out of host memory"); }
    catch (const std::exception& e) { return fail(SRN_EINVAL, std::string("internal error: ") + e.what()); }
    catch (...) { return fail(SRN_EINVAL, "internal error"); }
}
// the unserved-query mark of a call's count words
inline int check_all_served(const uint32_t* counts, size_t nq) {
    for (size_t q = 0; q < nq; ++q) if (counts[q] == 0xFFFFFFFFu) return fail(SRN_ERANGE, "a query exceeded the kernel's table limits");
    return SRN_OK;
}
// measurement aid (srn_debug_exclude_filter): the filter kernel alone over the caller's wide rows, enqueued on `stream`
int device_exclude_filter(DeviceState* d, uint32_t nq, const uint64_t* w_ids, const double* w_scores, const uint32_t* w_counts, uint32_t wide, const uint64_t* x_flat, const uint32_t* x_off,
                          uint32_t max_excl, const uint64_t* items_flat, const uint32_t* q_off, uint64_t* out_ids, double* out_scores, uint32_t* out_counts, uint32_t how_many, void* stream);
// The fallback ranking (srn_fill.hip).  RowRule::fill: behind the launch sequence and the exclusion filter, short rows of the call's final rows are filled in
// place from the ranking (a host-pointer call's rows then always pass through the filter's device buffers)
bool device_has_fallback(const DeviceState* d);
int device_set_fallback(DeviceState* d, const FlatIndex& ix, const uint64_t* item_ids, uint32_t n);   // replaces an earlier ranking; synchronises the device
void device_clear_fallback(DeviceState* d);
// measurement aid (srn_debug_fill): the fill kernel alone over the caller's rows, enqueued on `stream`
int device_fill(DeviceState* d, uint32_t nq, uint64_t* ids, double* scores, uint32_t* counts, uint32_t how_many, const uint64_t* x_flat, const uint32_t* x_off,
                const uint64_t* items_flat, const uint32_t* q_off, bool whole_session, bool business, void* stream);
// test aid (srn_debug_class_counts): the k-cut's wave-wide class counts (wave_class_counts, srn_device.h) alone; host pointers, acc [n_waves * 64], out16 [n_waves * 16]
int device_debug_class_counts(const uint64_t* acc, size_t n_waves, uint32_t* out16, int device);
// test aid (srn_debug_merge_pair): the fast kernel's merge_pair (srn_fast.hip) alone in one workgroup; host pointers, room [12 032 words], pairs [n_pairs * 5]
int device_debug_merge_pair(uint32_t* room, const uint32_t* pairs, size_t n_pairs, int device);
struct ShardIO {
    void* cand; uint32_t* cand_cnt;                                       // A out: [nq * m] packed slots, [nq]
    const void* gathered; const uint32_t* gathered_cnt; uint32_t n_shards;   // B in: [G][nq * gathered_stride], [G][nq]
    uint32_t gathered_stride;                                                // entries per query and shard in `gathered` (0 = m)
    void* nb; uint32_t* nb_cnt; int* minpos;                             // B out / C in: [nq * k], [nq], [nq * (k + 1)]
};

bool device_shard_lists_supported(DeviceState* d, const FlatIndex& ix, const LaunchParams& p);
bool device_fast_eligible(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, uint64_t max_row_len_all = 0);   // max_row_len_all != 0: from rank-invariant inputs only (srn_group.hip)
bool device_has_packed_rows(const DeviceState* d);
// the shard's fragments once more, in the posting order of `post`'s lists (the streaming form of the wave-per-query back end); optional: no room, or not a shard of that
// kernel's geometry -> SRN_OK and the gather form runs.  post == nullptr: drop them.
int device_sback_attach_postings(DeviceState* d, DeviceState* post, uint64_t n_postings);
bool device_sback_streams(const DeviceState* d);
bool device_sback_wanted(const DeviceState* d);   // this shard has the wave-per-query back end's rows and the streaming form is not switched off: set_postings expects the copy
uint64_t device_sback_launches(const DeviceState* d);
// One local shard of a shard group, as every device_shard_* step below takes it (device buffers, asynchronous on `stream`).  post: the replicated postings of the
// neighbours pipeline (the whole index's dictionary + lists), null otherwise
struct ShardCall { DeviceState* d; const FlatIndex* ix; DeviceState* post; void* stream; };
// neighbours pipeline: prep records of ALL queries (lists looked up in `post`, dense idx in this shard's table); order_buf (grow-only, the caller's): the batch's serving
// order is sorted into it, *order_out = where (null: batch too small)
int device_shard_nb_prep(const ShardCall& c, const LaunchParams& p, char* records, char** order_buf, size_t* order_bytes, const unsigned long long** order_out);
// ... then the fast kernel over them: ext.mode 1 = the front end over the queries [ext.q_lo, p.nq) -> ext.x, 2 = the back end over all of them <- ext.x (prep, prep_stride
// and post_rank are filled in here)
int device_shard_nb_run(const ShardCall& c, const LaunchParams& p, const char* records, ExtLists ext);
// the fronting rank's neighbour lists [q_lo, p.nq) of `in` -> position records in `out`
int device_shard_nb_positions(const ShardCall& c, const LaunchParams& p, const char* records, const ShardXchg& in, const ShardXchg& out, uint32_t q_lo);
uint32_t device_shard_nb_positions_stride(const LaunchParams& p);   // 0: no streaming form for this batch shape / these knobs (rank-invariant)
uint32_t device_prep_stride(uint32_t max_len);
int device_shard_lists_head(const ShardCall& c, const LaunchParams& p, void* pos, int* head);
int device_shard_lists_count(const ShardCall& c, const LaunchParams& p, const void* pos, const int* head, uint32_t* kept, int* tot);
int device_shard_lists_copy(const ShardCall& c, const LaunchParams& p, const void* pos, const uint32_t* kept, const long long* off, uint32_t* out);
// what the exchanges of the lists pipeline left for the prep records: [n_shards][nq * max_len] kept counts, [n_shards][nq] offsets, the gathered prefixes with shard g's
// segment at shard_base[g] (device), the global cuts, this shard's positions.  direct: a group of one shard reads its lists in place (lists_g = null)
struct ShardLists { uint32_t n_shards; const uint32_t* kept_g; const long long* off_g; const uint32_t* lists_g; const unsigned long long* shard_base; const int* head; const void* pos_local; bool direct; };
int device_shard_lists_predict(const ShardCall& c, const LaunchParams& p, const ShardLists& l, char* records);
int device_shard_stage(const ShardCall& c, int stage, const LaunchParams& p, const ShardIO& sh);
int device_slot_bytes(DeviceState* d, const FlatIndex& ix, uint32_t max_len, uint32_t* num_bits = nullptr);
int device_debug_geometry(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, uint32_t* out24);   // test aid (srn_debug_geometry): make_geometry's decision for a plain predict launch, as words
// ---- the persistent latency path (round 6): resident workgroups that serve srn_predict's call shape without a launch ----
// lanes: resident workgroups of the lean form (sessions of <= 4 items); max_items >= 5: as many of the MID form (5..10 items) beside them; idle_ms: a resident workgroup
// leaves by itself after that long without a request (it is started again by the next call that wants it)
int device_serve_start(DeviceState* d, const FlatIndex& ix, uint32_t k, uint32_t m, uint32_t how_many, uint32_t flags, uint32_t lanes, uint32_t max_items, uint32_t idle_ms);
int device_serve_stop(DeviceState* d);
// 0: served, *out_n rows written; 1: not served (no free lane, another configuration, a session the fused form hands on): the caller takes the launch path
int device_serve_predict(DeviceState* d, const uint64_t* items, uint32_t len, uint32_t k, uint32_t m, uint32_t how_many, uint32_t flags, uint64_t* out_ids, double* out_scores, size_t* out_n);
int device_serve_last_stamps(DeviceState* d, uint32_t* out4);
int device_serve_lane_counts(DeviceState* d, uint32_t form, uint64_t* out_served, size_t cap, size_t* out_n);
int device_serve_stats(DeviceState* d, uint64_t* served, uint64_t* not_served, uint64_t* launches, uint32_t* lanes);
int device_last_kernel_ms(DeviceState* d, double* ms_main, double* ms_retry, uint32_t* retried);
int device_phase_cycles(DeviceState* d, int enable, unsigned long long* out16);
int device_kernel_timing(DeviceState* d, int enable);
int device_reserve(DeviceState* d, const FlatIndex& ix, const LaunchParams& p, void* stream);
int device_last_path_counts(DeviceState* d, uint32_t* nq, uint32_t* general, uint32_t* global_pass);   // debug profiling aid
// test aid (srn_debug_prep_records): the prep kernel alone over a host batch, its records copied to out [nq * stride]; *out_stride = bytes per record
int device_debug_prep_records(DeviceState* d, const FlatIndex& ix, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t m, size_t max_len, void* out, size_t cap_bytes, size_t* out_stride);
int device_last_mid_count(DeviceState* d, uint32_t* listed, uint32_t* big_listed = nullptr);   // queries the last call's lean fast kernel listed for its MID instantiation
int device_last_light_count(DeviceState* d, uint32_t* light);     // light representatives of the last call (srn_light.hip); 0 where the form was off
int device_last_dedup_count(DeviceState* d, uint32_t* merged);   // queries of the last call merged into an equal, earlier query of the same call (srn_dedup.hip)
// ---- the device result cache (srn_result_cache.hip): served rows kept across calls, used by the batch launch sequence where its fast path is ----
static constexpr unsigned kFlagNoResultCache = 0x80000000u;   // LaunchParams::flags, internal (the predict entries strip it): this call bypasses an enabled cache (srn_evaluate)
int device_result_cache_enable(DeviceState* d, uint64_t rows, uint32_t max_len, uint32_t k, uint32_t m, uint32_t how_many, uint32_t flags);
int device_result_cache_disable(DeviceState* d);
int device_result_cache_clear(DeviceState* d);            // SRN_ESTATE: none enabled
int device_result_cache_clear_if_enabled(DeviceState* d);
int device_result_cache_stats(DeviceState* d, srn_result_cache_stats_t* out);
void device_result_cache_bypassed(DeviceState* d);        // a call that did not use the enabled cache (nothing happens without one)
int device_kernel_times(DeviceState* d, uint32_t max_n, double* ms_main, double* ms_retry, uint32_t* out_n, double* ms_prep = nullptr, double* ms_fast = nullptr);

}  // namespace srn

namespace srn {
// concurrent srn_predict calls on one handle combine into rounds (srn_combine.cpp)
struct Combiner;
Combiner* combiner_create();
void combiner_free(Combiner* c);
void combiner_stats(const Combiner* c, uint64_t* rounds, uint64_t* requests, uint64_t* max_round);
int combiner_predict(Combiner* c, const srn_index* idx, const uint64_t* evolving, size_t len, size_t k, size_t m, size_t how_many, unsigned flags,
                     uint64_t* out_ids, double* out_scores, size_t* out_n, int lanes, size_t round_cap);
int knob_predict_lanes();   // SRN_PREDICT_LANES (0 = no combining: every call runs by itself, as in round 2)
size_t knob_tiny_max();     // SRN_TINY_MAX: largest host batch on the zero-copy latency path = largest round
}  // namespace srn

struct srn_index {
    srn::FlatIndex flat;             // host readers of post_rank, row_off, row_items and rank_to_session go through srn::host_flat(): a resident index fetches them lazily
    srn::DeviceState* dev = nullptr;
    int device = -1;
    srn::Combiner* comb = nullptr;   // created with the device state
    std::vector<uint64_t> fallback;  // the fallback ranking as set (srn_index_set_fallback*; empty: none)
    // reference session index -> recency rank (kNone: not a kept session), built at the first srn_index_items_for_session call (the index is immutable: call_once)
    mutable std::vector<uint32_t> session_to_rank; mutable std::once_flag s2r_once;
    // srn_index_from_events_device: flat holds every scalar and per-item array, the four large arrays are on the device until the first host reader (host_complete = false)
    mutable std::atomic<bool> host_complete{true}; mutable std::mutex host_mu; mutable uint64_t materialisations = 0; mutable double ms_materialize = 0.0;
    srn_index_host_state_t build_state{};   // the build's stage times (the other fields are filled in by srn_index_host_state)
};
namespace srn {
// the index's FlatIndex with all of its arrays on the host: downloads the four large arrays of a resident index once (under host_mu), frees the build residue serving does
// not read.  nullptr: the download failed (error set, SRN_EHIP)
const FlatIndex* host_flat(const srn_index* idx);
int index_from_events_device(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, size_t m_index, double idf_weighting,
                             size_t max_session_len, int device, void* stream, srn_index* idx);   // srn_build_gpu.hip; fills idx->flat, idx->dev, idx->device
}  // namespace srn
struct srn_sessions {
    srn::Sessions s;
    srn_load_info_t info{};   // the GPU loader's counts and stage times (zeros for the host loader)
};
struct srn_events {   // a file's rows on the device (srn_events_from_tsv_gpu): three hipMalloc'ed arrays, released by events_free
    uint64_t* s = nullptr; uint64_t* i = nullptr; uint64_t* t = nullptr;
    size_t n = 0;
    int device = -1;
};

// ---- offline evaluation (srn_eval.hip): test sessions + training-item frequencies bound to one index ----
namespace srn { struct EvalDevice; }
struct srn_eval_set {
    const srn_index* idx = nullptr;
    std::vector<uint64_t> sess_off;      // host copy of the test sessions' offsets (the per-window query / item scans)
    uint64_t max_session_len = 0;
    double max_freq = 1.0;               // largest training count (1 without training items, as a 0 / 0 never arises)
    uint64_t unique_training_items = 0;
    srn::EvalDevice* dev = nullptr;
};
namespace srn {
int eval_set_create(const srn_index* idx, const uint64_t* items_flat, const uint64_t* sess_off, size_t n_sessions,
                    const uint64_t* train_ids, const uint64_t* train_counts, size_t n_train, srn_eval_set** out);
int eval_set_from_tsv(const srn_index* idx, const char* test_path, const char* train_path, srn_eval_set** out);
int eval_set_from_events(const srn_index* idx, const uint64_t* test_session_ids, const uint64_t* test_item_ids, const void* test_times, size_t n_test,
                         const uint64_t* train_item_ids, size_t n_train, unsigned flags, void* stream, srn_eval_set** out);
// trials already checked (srn_capi.cpp).  terms != nullptr: one trial, its per-query terms [n * 7] (cap entries of room)
// boot != nullptr (already checked): every trial's replicate sums too, rep[n_trials][boot->replicates][SRN_BOOTSTRAP_SUMS] on the host
int eval_run(srn_eval_set* set, const srn_eval_trial_t* trials, size_t n_trials, srn_eval_result_t* out, void* stream, double* terms, size_t cap,
             const srn_bootstrap_t* boot = nullptr, double* rep = nullptr,
             const srn_segments_t* seg = nullptr, srn_eval_segment_t* seg_out = nullptr, double* seg_rep = nullptr);
// seg != nullptr (already checked, its n_labels included): every trial's sums by segment too (srn_segments.hip), seg_out[n_trials][segments] and, with boot,
// seg_rep[n_trials][segments][replicates][SRN_BOOTSTRAP_SUMS] on the host
int eval_segment_ids(srn_eval_set* set, const srn_segments_t* seg, uint16_t* out);   // out: room for eval_n_queries(set) ids
void eval_segment_ms(const srn_eval_set* set, double* ms_segments, double* ms_segment_bootstrap);   // device time of the last call's segment kernels
// the bootstrap behind the metrics kernel (srn_bootstrap.hip): one chunk's terms [nq][8] and (session, state) pairs onto a trial's running totals
// [replicates][SRN_BOOTSTRAP_SUMS], through scratch of boot_scratch_bytes(largest chunk, replicates); only enqueues
size_t boot_scratch_bytes(uint64_t chunk_queries, uint32_t replicates);
int boot_chunk(const double* terms, const void* session_state, uint32_t nq, const srn_bootstrap_t& boot, double* scratch, double* totals, void* stream);
void boot_weights_host(uint64_t seed, uint32_t replicate, uint64_t first_session, size_t n, uint8_t* out);
uint64_t eval_n_queries(const srn_eval_set* set);   // queries of any trial: sum over sessions of (len - 1)
// a trial's exclusion lists hold at most this many ids (0: the trial excludes nothing): the history window -- the session window without one -- with
// SRN_FLAG_EXCLUDE_SEEN, the session window with SRN_FLAG_EXCLUDE_SESSION alone.  The launch sequence runs at how_many + this
inline uint32_t eval_excl_capacity(const srn_eval_trial_t& t) {
    if (t.flags & SRN_FLAG_EXCLUDE_SEEN) return t.history ? t.history : t.max_items_in_session;
    return (t.flags & SRN_FLAG_EXCLUDE_SESSION) ? t.max_items_in_session : 0u;
}
void eval_set_free(srn_eval_set* set);
}  // namespace srn

// ---- a visitor batch: what the batch calls of the session store and the click feedback log take (srn_visitors.h sorts and stages it) ----
namespace srn {
// the request side, host or device pointers alike: request i = (key_hi[i], key_lo[i], item[i], consent[i]) at times[i].  consent null: every request consents;
// times null: an untimed batch, every request at now_secs (timed, now_secs is the capacity rule's sweep clock alone: DESIGN.md 11.6)
struct VisitorBatch { const uint64_t* key_hi; const uint64_t* key_lo; const uint64_t* item; const uint8_t* consent; const uint64_t* times; size_t n; uint64_t now_secs; };
inline bool has_request_arrays(const VisitorBatch& r, bool timed) { return r.key_hi && r.key_lo && r.item && (!timed || r.times); }
constexpr uint32_t kMaxBatch = 1u << 24;   // requests in one call (the store's q_off is 32-bit: n * SRN_MAX_SESSION_LEN < 2^32)
// ... and each owner's side: the predict parameters and the rows out; the served rows in and the ranks out (scores and out_rank may be null).  stream: the device entries'
struct RecommendCall { size_t max_items, k, m, how_many; unsigned flags; uint64_t* ids; double* scores; uint32_t* counts; void* stream; };
struct ObserveCall { const uint64_t* ids; const double* scores; const uint32_t* counts; size_t how_many; uint32_t* out_rank; void* stream; };
}  // namespace srn

// ---- device-resident session store (srn_sessions_dev.hip); arguments of the batch calls already checked by the C ABI glue ----
namespace srn {
int dsess_create(int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions** out);
void dsess_free(srn_device_sessions* s);
int dsess_get(srn_device_sessions* s, uint64_t hi, uint64_t lo, uint64_t now_secs, uint64_t* out_items, size_t cap, size_t* out_n);
int dsess_update(srn_device_sessions* s, uint64_t hi, uint64_t lo, uint64_t now_secs, const uint64_t* items, size_t n);
int dsess_sweep(srn_device_sessions* s, uint64_t now_secs, uint64_t* n_live);
int dsess_stats(srn_device_sessions* s, srn_device_sessions_stats_t* out);
int dsess_timing(srn_device_sessions* s, int enable);
int dsess_set_history(srn_device_sessions* s, size_t history);
int dsess_history(srn_device_sessions* s, size_t* out);
int dsess_last_ms(srn_device_sessions* s, double* ms_store, double* ms_predict);
int dsess_last_csr(srn_device_sessions* s, const void** d_items, const void** d_qoff, size_t* n, size_t* max_len, uint64_t* h_items, size_t cap, uint32_t* h_qoff);
int dsess_count(srn_device_sessions* s, uint64_t now_secs, uint64_t* occupied, uint64_t* live);
int dsess_export_device(srn_device_sessions* s, uint64_t now_secs, size_t cap, uint64_t* d_hi, uint64_t* d_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items,
                        size_t items_stride, uint64_t* d_n, void* stream);
int dsess_export_host(srn_device_sessions* s, uint64_t now_secs, size_t cap, uint64_t* hi, uint64_t* lo, uint64_t* epoch, uint32_t* len, uint64_t* items,
                      size_t items_stride, size_t* n);
int dsess_import_device(srn_device_sessions* s, const uint64_t* d_hi, const uint64_t* d_lo, const uint64_t* d_epoch, const uint32_t* d_len, const uint64_t* d_items,
                        size_t items_stride, size_t n, void* stream);
int dsess_import_host(srn_device_sessions* s, const uint64_t* hi, const uint64_t* lo, const uint64_t* epoch, const uint32_t* len, const uint64_t* items,
                      size_t items_stride, size_t n);
int dsess_resize(srn_device_sessions* s, size_t capacity, size_t items_cap, uint64_t now_secs);
int dsess_set_max_capacity(srn_device_sessions* s, size_t max_capacity);
int dsess_growth(srn_device_sessions* s, uint64_t* max_capacity, uint64_t* grows, uint64_t* resizes);
int dsess_save(srn_device_sessions* s, const char* path, uint64_t now_secs);
int dsess_load(const char* path, int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions** out);
int dsess_file_info(const char* path, srn_device_sessions_file_info_t* out);
int dsess_recommend_device(const srn_index* idx, srn_device_sessions* s, const VisitorBatch& r, const RecommendCall& c);
int dsess_recommend_host(const srn_index* idx, srn_device_sessions* s, const VisitorBatch& r, const RecommendCall& c);
// the traffic split's front (srn_arms.hip): the arms' checks against the store, then the capacity rule once for all n requests (now: already read from the clock)
int dsess_admit(srn_device_sessions* s, const srn_index* const* idx, const RecommendCall* c, size_t n_arms, uint64_t n, uint64_t now);
// trending items (srn_trending.hip): the items the store's live sessions hold most often
int dsess_top_items(srn_device_sessions* s, uint64_t now_secs, uint64_t since_secs, uint32_t min_count, size_t cap, uint64_t* out_ids, uint32_t* out_counts, size_t* out_n);
int dsess_device_of(const srn_device_sessions* s);
// session harvest (srn_harvest.hip): every argument check is its own
int harvest_create(int device, size_t capacity, size_t items_cap, uint32_t min_len, srn_harvest** out);
int harvest_free(srn_harvest* h);
int dsess_set_harvest(srn_device_sessions* s, srn_harvest* h);
int harvest_stats(srn_harvest* h, srn_harvest_stats_t* out);
int harvest_clear(srn_harvest* h);
int harvest_export_device(srn_harvest* h, size_t cap, uint64_t* d_hi, uint64_t* d_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items, size_t items_stride,
                          uint64_t* d_n, void* stream);
int harvest_export_host(srn_harvest* h, size_t cap, uint64_t* hi, uint64_t* lo, uint64_t* epoch, uint32_t* len, uint64_t* items, size_t items_stride, size_t* n);
int harvest_events_device(srn_harvest* h, uint64_t id_base, size_t cap_rows, uint64_t* d_session_ids, uint64_t* d_item_ids, int64_t* d_times, uint64_t* d_rows, void* stream);
// click feedback log (srn_feedback.hip): every argument check is its own
int fb_create(int device, size_t capacity, size_t row_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_feedback** out);
void fb_free(srn_feedback* f);
int fb_observe_device(srn_feedback* f, const VisitorBatch& r, const ObserveCall& c);
int fb_observe_host(srn_feedback* f, const VisitorBatch& r, const ObserveCall& c);
void fb_shape(const srn_feedback* f, int* device, uint64_t* row_cap);   // what a caller that feeds several logs checks before it feeds any
int fb_stats(srn_feedback* f, srn_feedback_stats_t* out);
int fb_histogram(srn_feedback* f, uint64_t* hits_model, uint64_t* hits_filled, size_t cap);
int fb_reset_counters(srn_feedback* f);
int fb_sweep(srn_feedback* f, uint64_t now_secs, uint64_t* n_live);
int fb_get(srn_feedback* f, uint64_t hi, uint64_t lo, uint64_t now_secs, uint64_t* out_ids, size_t cap, uint32_t* out_count, uint32_t* out_n_model, uint64_t* out_epoch);
// ... and its visitor-clustered bootstrap
int fb_boot_enable(srn_feedback* f, uint32_t replicates, uint64_t seed);
int fb_boot_disable(srn_feedback* f);
int fb_boot_info(srn_feedback* f, uint32_t* replicates, uint64_t* seed);
int fb_boot_read(srn_feedback* f, uint64_t* observed, uint64_t* hits_model, uint64_t* hits_filled, size_t replicates_cap, size_t rank_cap);
void fb_boot_weights_host(uint64_t seed, uint32_t replicate, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out);
// traffic split (srn_arms.hip): every argument check is its own, but an arm's predict parameters -- check_arm(arm, how_many) is the C ABI glue's
struct SplitOut { uint64_t* ids; double* scores; uint32_t* counts; uint8_t* arm; uint32_t* rank; int* feedback_rc; };   // arm, rank and feedback_rc may be null
int split_create(int device, const uint32_t* weights, size_t n_arms, uint64_t seed, size_t max_batch, size_t max_how_many, srn_traffic_split** out);
int split_free(srn_traffic_split* sp);
int split_info(const srn_traffic_split* sp, srn_traffic_split_info_t* out);
int split_set_weights(srn_traffic_split* sp, const uint32_t* weights, size_t n_arms);
int split_arms_host(uint64_t seed, const uint32_t* weights, size_t n_arms, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out);
int split_timing(srn_traffic_split* sp, int enable);
int split_last_ms(srn_traffic_split* sp, double* ms_front, double* ms_scatter);
int split_recommend_device(srn_traffic_split* sp, const srn_arm_t* arms, size_t n_arms, srn_device_sessions* store, const VisitorBatch& r, size_t how_many,
                           const SplitOut& o, void* stream, int (*check_arm)(const srn_arm_t&, size_t));
int split_recommend_host(srn_traffic_split* sp, const srn_arm_t* arms, size_t n_arms, srn_device_sessions* store, const VisitorBatch& r, size_t how_many,
                         const SplitOut& o, int (*check_arm)(const srn_arm_t&, size_t));
}  // namespace srn
