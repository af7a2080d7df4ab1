// C ABI of libserenade_hip.so (include/serenade_hip.h): argument validation, error codes, handle
// ownership.  No compute happens here -- predict calls go to the HIP kernels or fail.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "srn_internal.h"

namespace srn { const char* last_error_cstr(); int device_count(); }
using namespace srn;

// The one door to post_rank, row_off, row_items and rank_to_session on the host.  An index from srn_index_from_events_device keeps them on the device until the first
// caller comes through here; every other index passes straight through
const FlatIndex* srn::host_flat(const srn_index* idx) {
    if (idx->host_complete.load(std::memory_order_acquire)) return &idx->flat;
    std::lock_guard<std::mutex> lk(idx->host_mu);
    if (!idx->host_complete.load(std::memory_order_relaxed)) {
        const auto t0 = std::chrono::steady_clock::now();
        if (device_materialize(idx->dev, const_cast<FlatIndex&>(idx->flat)) != SRN_OK) return nullptr;
        idx->ms_materialize = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        ++idx->materialisations;
        idx->host_complete.store(true, std::memory_order_release);
    }
    return &idx->flat;
}

namespace {

int check_predict_args(const srn_index_t* idx, size_t k, size_t m, size_t how_many) {
    if (!idx) return fail(SRN_EINVAL, "null index");
    if (!idx->dev) return fail(SRN_ENODEV, "index has no device attached; there is no CPU fallback behind this ABI");
    if (idx->flat.postings_only) return fail(SRN_EINVAL, "a postings-only view holds no rows: it serves a shard group (srn_shard_group_set_postings), not predict calls");
    // the reference panics (peek_mut().unwrap() on an empty heap) when any of these is zero
    if (k == 0 || m == 0 || how_many == 0) return fail(SRN_EINVAL, "k, m and how_many must be > 0");
    if (how_many > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "how_many above SRN_MAX_HOW_MANY");
    if (k > SRN_MAX_K) return fail(SRN_ERANGE, "k above SRN_MAX_K");
    if (m > 0x7FFFFFFFull) return fail(SRN_ERANGE, "m too large");
    return SRN_OK;
}
// an item shard answers only through the three stages: its rows are fragments (DeviceIndex::row_frag) and its lists a subset
static int check_not_a_shard(const srn_index_t* idx) {
    return idx && idx->flat.n_shards > 1 ? fail(SRN_EINVAL, "this index is one item shard of several: predictions go through its shard group (srn_shard_group_predict_batch)") : SRN_OK;
}

// a host batch's sessions: *max_len = the longest, or the first offence
int scan_q_off(const uint32_t* q_off, size_t nq, uint32_t* max_len) {
    uint32_t longest = 0;
    for (size_t q = 0; q < nq; ++q) {
        if (q_off[q + 1] < q_off[q]) return fail(SRN_EINVAL, "q_off not monotone");
        if (q_off[q + 1] == q_off[q]) return fail(SRN_EINVAL, "empty evolving session (the reference panics: src/vmisknn/mod.rs:157)");
        longest = std::max(longest, q_off[q + 1] - q_off[q]);
    }
    if (longest > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "evolving session longer than SRN_MAX_SESSION_LEN");
    *max_len = longest;
    return SRN_OK;
}
// the tail every index constructor shares: attach to the device (device < 0: a host-only index), hand the handle out or drop it
int finish_index(srn_index* ix, int rc, int device, srn_index_t** out) {
    if (rc == SRN_OK && device >= 0) { ix->dev = device_attach(ix->flat, device); ix->device = device; if (!ix->dev) rc = SRN_EHIP; else ix->comb = combiner_create(); }
    if (rc) { delete ix; return rc; }
    *out = ix; return SRN_OK;
}

int predict_host(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t k, size_t m,
                 size_t how_many, unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts,
                 uint32_t* out_stats, uint32_t* out_nb_sessions, uint32_t* out_nb_num, uint32_t* out_nb_counts) {
    int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
    rc = check_not_a_shard(idx); if (rc) return rc;
    if (nq == 0) return SRN_OK;
    if (!items_flat || !q_off || !out_ids || !out_scores || !out_counts) return fail(SRN_EINVAL, "null buffer");
    if (nq > 0x7FFFFFFFull) return fail(SRN_ERANGE, "too many queries in one batch");
    if ((out_nb_sessions != nullptr) != (out_nb_num != nullptr) || (out_nb_sessions != nullptr) != (out_nb_counts != nullptr))
        return fail(SRN_EINVAL, "neighbour debug outputs must be given together");
    uint32_t max_len = 0;
    rc = scan_q_off(q_off, nq, &max_len); if (rc) return rc;
    rc = device_predict_host(idx->dev, idx->flat, launch_params(nq, k, m, how_many, flags, max_len),
                             HostRows{items_flat, q_off, out_ids, out_scores, out_counts, out_stats, out_nb_sessions, out_nb_num, out_nb_counts});
    if (rc) return rc;
    rc = check_all_served(out_counts, nq); if (rc) return rc;
    if (out_nb_sessions) {   // recency rank -> reference session index
        const FlatIndex* hf = host_flat(idx); if (!hf) return SRN_EHIP;
        for (size_t q = 0; q < nq; ++q)
            for (uint32_t j = 0; j < out_nb_counts[q]; ++j) {
                uint32_t& r = out_nb_sessions[q * k + j];
                r = hf->rank_to_session[r];
            }
    }
    return SRN_OK;
}
}  // namespace

extern "C" {

const char* srn_last_error(void) { return last_error_cstr(); }
const char* srn_version(void) { return "serenade_hip 0.1 (gfx950)"; }
int srn_device_count(int* out) { if (!out) return fail(SRN_EINVAL, "null argument"); *out = device_count(); return SRN_OK; }
void srn_limits(srn_limits_t* out) { if (out) *out = srn_limits_t{SRN_MAX_HOW_MANY, SRN_MAX_SESSION_LEN, SRN_MAX_K, 0}; }

int srn_sessions_from_tsv(const char* path, srn_sessions_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        srn_sessions* s = new srn_sessions();
        int rc = sessions_from_tsv(path, s->s);
        if (rc) { delete s; return rc; }
        *out = s; return SRN_OK; });
}
int srn_sessions_view(const srn_sessions_t* s, srn_sessions_view_t* out) {
    if (!s || !out) return fail(SRN_EINVAL, "null argument");
    out->sess_off = s->s.off.data(); out->items = s->s.items.data(); out->max_ts = s->s.ts.data(); out->n_sessions = s->s.ts.size();
    return SRN_OK;
}
int srn_sessions_length_quantile(const srn_sessions_t* s, double q, uint64_t* out) {
    if (!s || !out || !(q >= 0.0 && q <= 1.0)) return fail(SRN_EINVAL, "bad argument");
    return guarded([&]() -> int { *out = sessions_length_quantile(s->s.off.data(), s->s.ts.size(), q); return SRN_OK; });
}
void srn_sessions_free(srn_sessions_t* s) { delete s; }

int srn_sessions_from_tsv_gpu(const char* path, int device, srn_sessions_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        if (device < 0) return fail(SRN_ENODEV, "the GPU loader needs a device");
        srn_sessions* s = new srn_sessions();
        int rc = sessions_from_tsv_gpu(path, device, s->s, &s->info);
        if (rc) { delete s; return rc; }
        *out = s; return SRN_OK; });
}
int srn_sessions_from_events(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, int device, void* stream,
                             srn_sessions_t** out) {
    return guarded([&]() -> int {
        if (!out || (n && (!session_ids || !item_ids || !times))) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        if (flags & ~(SRN_EVENTS_TIME_I64 | SRN_EVENTS_DEVICE)) return fail(SRN_EINVAL, "unknown flags");
        if (device < 0) return fail(SRN_ENODEV, "the GPU loader needs a device");
        srn_sessions* s = new srn_sessions();
        int rc = sessions_from_events(session_ids, item_ids, times, n, flags, device, stream, s->s, &s->info);
        if (rc) { delete s; return rc; }
        *out = s; return SRN_OK; });
}
// ---- a click log's rows on the device and their split by time (srn_ingest.hip, srn_split.hip) ----
int srn_events_from_tsv_gpu(const char* path, int device, srn_events_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        if (device < 0) return fail(SRN_ENODEV, "the GPU loader needs a device");
        return events_from_tsv_gpu(path, device, out); });
}
int srn_events_view(const srn_events_t* e, srn_events_view_t* out) {
    if (!e || !out) return fail(SRN_EINVAL, "null argument");
    *out = srn_events_view_t{e->s, e->i, e->t, e->n, e->device, 0};
    return SRN_OK;
}
void srn_events_free(srn_events_t* e) { events_free(e); }
int srn_events_split(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, const srn_split_t* split, int device,
                     void* stream, uint8_t* code, uint32_t* pos, srn_split_info_t* info) {
    return guarded([&]() -> int {
        if (!session_ids || !item_ids || !times || !split || !code || !pos || !info) return fail(SRN_EINVAL, "null argument");
        if (n == 0) return fail(SRN_EINVAL, "no rows to split");
        if (flags & ~(SRN_EVENTS_TIME_I64 | SRN_EVENTS_DEVICE)) return fail(SRN_EINVAL, "unknown flags");
        if (split->cutoff == 0) return fail(SRN_EINVAL, "cutoff must be > 0");
        if (split->start && split->start >= split->cutoff) return fail(SRN_EINVAL, "start must be below cutoff");
        if (split->end && split->end <= split->cutoff) return fail(SRN_EINVAL, "end must be above cutoff");
        if ((split->flags & ~SRN_SPLIT_TEST_KNOWN_ITEMS) || split->reserved) return fail(SRN_EINVAL, "unknown split flags");
        if (n >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "a split takes < 2^32 - 1 rows per call");
        if (device < 0) return fail(SRN_ENODEV, "the split runs on a GPU");
        return events_split(session_ids, item_ids, times, n, flags, *split, device, stream, code, pos, info); });
}
int srn_events_take(const uint8_t* code, const uint32_t* pos, size_t n, uint8_t which, const uint64_t* session_ids, const uint64_t* item_ids, const void* times,
                    unsigned flags, uint64_t* out_sessions, uint64_t* out_items, void* out_times, int device, void* stream) {
    return guarded([&]() -> int {
        if (!code || !pos || !session_ids || !item_ids || !times || !out_sessions || !out_items || !out_times) return fail(SRN_EINVAL, "null argument");
        if (n == 0) return fail(SRN_EINVAL, "no rows to take from");
        if (flags & ~(SRN_EVENTS_TIME_I64 | SRN_EVENTS_DEVICE)) return fail(SRN_EINVAL, "unknown flags");
        if (which != SRN_SPLIT_TRAIN && which != SRN_SPLIT_TEST) return fail(SRN_EINVAL, "which must be SRN_SPLIT_TRAIN or SRN_SPLIT_TEST");
        if (n >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "a split takes < 2^32 - 1 rows per call");
        if (device < 0) return fail(SRN_ENODEV, "the split runs on a GPU");
        return events_take(code, pos, n, which, session_ids, item_ids, times, flags, out_sessions, out_items, out_times, device, stream); });
}
int srn_sessions_load_info(const srn_sessions_t* s, srn_load_info_t* out) {
    if (!s || !out) return fail(SRN_EINVAL, "null argument");
    *out = s->info;
    return SRN_OK;
}

int srn_index_build(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len, double idf_weighting,
                    int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!sessions || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        srn_index* ix = new srn_index();
        return finish_index(ix, build_flat_index(*sessions, m_index, max_session_len, idf_weighting, 0, 1, ix->flat), device, out); });
}

int srn_index_build_gpu(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len, double idf_weighting,
                        int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!sessions || !out) return fail(SRN_EINVAL, "null argument");
        if (device < 0) return fail(SRN_ENODEV, "the GPU index builder needs a device");
        *out = nullptr;
        srn_index* ix = new srn_index();
        return finish_index(ix, build_flat_index_gpu(*sessions, m_index, max_session_len, idf_weighting, device, ix->flat), device, out); });   // (device >= 0: checked above)
}

int srn_index_from_events_device(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, size_t m_most_recent_sessions,
                                 double idf_weighting, size_t max_session_len, int device, void* stream, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!out || (n && (!session_ids || !item_ids || !times))) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        if (flags & ~(SRN_EVENTS_TIME_I64 | SRN_EVENTS_DEVICE)) return fail(SRN_EINVAL, "unknown flags");
        if (device < 0) return fail(SRN_ENODEV, "the GPU loader and the GPU index builder need a device");
        if (n == 0) return fail(SRN_EINVAL, "no training rows");
        if (n >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "the GPU loader groups < 2^32 rows per call; use the host loader");
        if (m_most_recent_sessions == 0) return fail(SRN_EINVAL, "m_index must be > 0");
        srn_index* ix = new srn_index();
        int rc = index_from_events_device(session_ids, item_ids, times, n, flags, m_most_recent_sessions, idf_weighting, max_session_len, device, stream, ix);
        if (rc) { if (ix->dev) device_release(ix->dev); delete ix; return rc; }
        ix->comb = combiner_create();
        *out = ix; return SRN_OK; });
}
int srn_index_host_state(const srn_index_t* idx, srn_index_host_state_t* out) {
    if (!idx || !out) return fail(SRN_EINVAL, "null argument");
    std::lock_guard<std::mutex> lk(idx->host_mu);
    *out = idx->build_state;
    out->host_complete = idx->host_complete.load() ? 1 : 0; out->reserved = 0;
    out->build_bytes_on_device = device_residue_bytes(idx->dev); out->materialisations = idx->materialisations; out->ms_materialize = idx->ms_materialize;
    return SRN_OK;
}
int srn_index_materialize(srn_index_t* idx) {
    if (!idx) return fail(SRN_EINVAL, "null index");
    return guarded([&]() -> int { return host_flat(idx) ? SRN_OK : SRN_EHIP; });
}

int srn_index_new_from_csv(const char* path, size_t m_most_recent_sessions, double idf_weighting, size_t max_session_len,
                           int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        Sessions s; int rc = sessions_from_tsv(path, s); if (rc) return rc;
        if (max_session_len == 0) max_session_len = sessions_length_quantile(s.off.data(), s.ts.size(), 0.995);
        srn_sessions_view_t v{s.off.data(), s.items.data(), s.ts.data(), s.ts.size()};
        // same bytes either way; the GPU builder covers what fits 32-bit ranks and offsets
        const bool gpu = device >= 0 && s.ts.size() < 0xFFFFFFFFull && s.items.size() < 0xFFFFFFFFull;
        return gpu ? srn_index_build_gpu(&v, m_most_recent_sessions, max_session_len, idf_weighting, device, out)
                   : srn_index_build(&v, m_most_recent_sessions, max_session_len, idf_weighting, device, out); });
}

int srn_index_new_from_csv_gpu(const char* path, size_t m_most_recent_sessions, double idf_weighting, size_t max_session_len,
                               int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        if (device < 0) return fail(SRN_ENODEV, "the GPU loader needs a device");
        Sessions s; int rc = sessions_from_tsv_gpu(path, device, s, nullptr); if (rc) return rc;
        if (max_session_len == 0) max_session_len = sessions_length_quantile_counting(s.off.data(), s.ts.size(), 0.995);
        srn_sessions_view_t v{s.off.data(), s.items.data(), s.ts.data(), s.ts.size()};
        // as srn_index_new_from_csv: the GPU builder where 32-bit ranks and offsets suffice
        const bool gpu = s.ts.size() < 0xFFFFFFFFull && s.items.size() < 0xFFFFFFFFull;
        return gpu ? srn_index_build_gpu(&v, m_most_recent_sessions, max_session_len, idf_weighting, device, out)
                   : srn_index_build(&v, m_most_recent_sessions, max_session_len, idf_weighting, device, out); });
}

int srn_index_new_from_avro(const char* base_path, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!base_path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        srn_index* ix = new srn_index();
        return finish_index(ix, build_flat_index_from_avro(base_path, ix->flat), device, out); });
}

int srn_index_save(const srn_index_t* idx, const char* path) {
    if (!idx || !path) return fail(SRN_EINVAL, "null argument");
    return guarded([&]() -> int {
        int rc = check_has_rows(idx->flat, "srn_index_save"); if (rc) return rc;
        const FlatIndex* hf = host_flat(idx); if (!hf) return SRN_EHIP;
        return save_flat_index(*hf, path); });
}
int srn_index_load(const char* path, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        srn_index* ix = new srn_index();
        return finish_index(ix, load_flat_index(path, ix->flat), device, out); });
}
int srn_index_set_attributes(srn_index_t* idx, const uint64_t* item_ids, const uint8_t* flags, size_t n) {
    if (!idx || (n && (!item_ids || !flags))) return fail(SRN_EINVAL, "null argument");
    return guarded([&]() -> int {
        for (size_t i = 0; i < n; ++i) {
            const uint32_t j = idx->flat.lookup(item_ids[i]);
            if (j == kNone) continue;   // attributes of items outside the index can never be consulted
            idx->flat.attr[j] = flags[i] == SRN_ATTR_NONE ? (uint8_t)SRN_ATTR_NONE : (uint8_t)(flags[i] & 3u);
        }
        if (!idx->dev) return SRN_OK;
        const int rc = device_update_attr(idx->dev, idx->flat);
        if (rc == SRN_OK) (void)device_result_cache_clear_if_enabled(idx->dev);   // (rows under the business rules depend on the flags)
        return rc; });
}
// ---- the fallback ranking (srn_fill.hip) ----
static int check_fallback_index(const srn_index_t* idx) {
    if (!idx) return fail(SRN_EINVAL, "null index");
    if (idx->flat.postings_only) return fail(SRN_EINVAL, "a postings-only view serves a shard group, not predict calls: it takes no fallback ranking");
    return check_not_a_shard(idx);
}
int srn_index_set_fallback(srn_index_t* idx, const uint64_t* item_ids, size_t n) {
    return guarded([&]() -> int {
        int rc = check_fallback_index(idx); if (rc) return rc;
        if (n == 0 || !item_ids) return fail(SRN_EINVAL, "srn_index_set_fallback: an empty ranking (srn_index_clear_fallback removes one)");
        if (n > SRN_MAX_FALLBACK) return fail(SRN_ERANGE, "srn_index_set_fallback: more than SRN_MAX_FALLBACK ids");
        std::vector<uint64_t> sorted(item_ids, item_ids + n);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(SRN_EINVAL, "srn_index_set_fallback: an id occurs twice");
        if (idx->dev) { rc = device_set_fallback(idx->dev, idx->flat, item_ids, (uint32_t)n); if (rc) { idx->fallback.clear(); return rc; } }
        idx->fallback.assign(item_ids, item_ids + n);
        return SRN_OK; });
}
int srn_index_set_fallback_popular(srn_index_t* idx, size_t n) {
    return guarded([&]() -> int {
        int rc = check_fallback_index(idx); if (rc) return rc;
        const size_t take = std::min<size_t>(n, idx->flat.n_items);   // (the dense item index IS the popularity order: count of kept sessions descending, id ascending)
        if (take == 0) return fail(SRN_EINVAL, "srn_index_set_fallback_popular: an empty ranking");
        if (take > SRN_MAX_FALLBACK) return fail(SRN_ERANGE, "srn_index_set_fallback_popular: more than SRN_MAX_FALLBACK ids");
        const std::vector<uint64_t> ids(idx->flat.item_id.begin(), idx->flat.item_id.begin() + take);
        return srn_index_set_fallback(idx, ids.data(), take); });
}
int srn_index_fallback(const srn_index_t* idx, uint64_t* out, size_t cap, size_t* out_n) {
    if (!idx || !out_n) return fail(SRN_EINVAL, "null argument");
    *out_n = idx->fallback.size();
    if (out) std::copy(idx->fallback.begin(), idx->fallback.begin() + std::min(cap, idx->fallback.size()), out);
    return SRN_OK;
}
int srn_index_clear_fallback(srn_index_t* idx) {
    if (!idx) return fail(SRN_EINVAL, "null index");
    device_clear_fallback(idx->dev);
    idx->fallback.clear();
    return SRN_OK;
}
int srn_index_info(const srn_index_t* idx, srn_index_info_t* out) {
    if (!idx || !out) return fail(SRN_EINVAL, "null argument");
    const FlatIndex& f = idx->flat;   // (post_rank is read for a pre-built index alone: never one with a lazy host copy)
    uint64_t incomplete = 0;
    if (!f.lists_complete && f.viol.size() == f.n_items)
        for (uint64_t i = 0; i < f.n_items; ++i) { const uint64_t len = f.post_off[i + 1] - f.post_off[i];
            if (f.viol[i] != 0u && !(len == f.m_index && len != 0 && f.viol[i] <= f.post_rank[f.post_off[i + 1] - 1])) ++incomplete; }
    else if (!f.lists_complete) incomplete = f.n_items;   // (a shard cut from such an index: not measured per item)
    *out = srn_index_info_t{f.n_items, f.n_sessions_total, f.n_kept, f.nnz_rows, f.nnz_post, f.m_index, f.max_session_len,
                            f.max_row_len, device_bytes(idx->dev), idx->dev ? idx->device : -1,
                            f.nnz_rows >= 0xFFFFFFFFull ? 1 : 0, f.idf_weighting, incomplete};
    return SRN_OK;
}
int srn_index_postings(const srn_index_t* idx, uint64_t item_id, uint32_t* out_sessions, size_t cap, int64_t* out_len, double* out_idf) {
    if (!idx || !out_len) return fail(SRN_EINVAL, "null argument");
    const FlatIndex& f = idx->flat;
    const uint32_t j = f.lookup(item_id);
    if (j == kNone) { *out_len = -1; return SRN_OK; }
    const uint64_t o0 = f.post_off[j], o1 = f.post_off[j + 1];
    *out_len = (int64_t)(o1 - o0);
    if (out_idf) *out_idf = f.idf[j];
    if (!out_sessions) return SRN_OK;   // (length and idf are per-item: no host copy of the lists needed)
    return guarded([&]() -> int {
        const FlatIndex* hf = host_flat(idx); if (!hf) return SRN_EHIP;
        for (uint64_t t = o0; t < o1 && t - o0 < cap; ++t) out_sessions[t - o0] = hf->rank_to_session[hf->post_rank[t]];
        return SRN_OK; });
}
// ---- the rest of SimilarityComputationNew (src/vmisknn/similarity_indexed.rs:9-23) at the ABI: with srn_index_postings (+ idf) above, a maintainer can write
// `impl SimilarityComputationNew for HipVMISIndex`, not only swap the free function predict ----
int srn_index_items_for_session(const srn_index_t* idx, uint32_t session, uint64_t* out_items, size_t cap, size_t* out_len) {
    return guarded([&]() -> int {
        if (!idx || !out_len) return fail(SRN_EINVAL, "null argument");
        *out_len = 0;
        int rc = check_has_rows(idx->flat, "srn_index_items_for_session"); if (rc) return rc;
        if (idx->flat.n_shards > 1) return fail(SRN_EINVAL, "an item shard holds row FRAGMENTS (the items it owns): ask the unsharded index");
        if (session >= idx->flat.n_sessions_total) return fail(SRN_EINVAL, "no such session (the reference indexes out of bounds: vmis_index.rs:317-319)");
        const FlatIndex* hf = host_flat(idx); if (!hf) return SRN_EHIP;
        const FlatIndex& f = *hf;
        std::call_once(idx->s2r_once, [&] { idx->session_to_rank.assign(f.n_sessions_total, kNone); for (uint64_t r = 0; r < f.n_kept; ++r) idx->session_to_rank[f.rank_to_session[r]] = (uint32_t)r; });
        const uint32_t r = idx->session_to_rank[session];
        // (the reference keeps the rows of ALL sessions, vmis_index.rs:79, but only sessions of <= max_session_len items enter the posting lists, :452 -- and only those can
        //  ever be neighbours, so only their rows are kept here)
        if (r == kNone) return fail(SRN_ERANGE, "this session is in no posting list (longer than max_session_len, vmis_index.rs:452, or named by no list of a pre-built index): never a neighbour, and its row is not kept");
        const uint64_t o0 = f.row_off[r], o1 = f.row_off[r + 1];
        *out_len = (size_t)(o1 - o0);
        if (out_items) for (uint64_t t = o0; t < o1 && t - o0 < cap; ++t) out_items[t - o0] = f.item_id[f.row_items[t]];   // (row order = ascending public id, as the reference's item_ids_asc)
        return SRN_OK; });
}
int srn_index_session_recency(const srn_index_t* idx, uint32_t* out_rank, size_t cap) {
    return guarded([&]() -> int {
        if (!idx || !out_rank) return fail(SRN_EINVAL, "null argument");
        int rc = check_has_rows(idx->flat, "srn_index_session_recency"); if (rc) return rc;
        if (cap < idx->flat.n_sessions_total) return fail(SRN_EINVAL, "room for n_sessions entries needed");
        const FlatIndex* hf = host_flat(idx); if (!hf) return SRN_EHIP;
        const FlatIndex& f = *hf;
        std::fill(out_rank, out_rank + f.n_sessions_total, kNone);
        for (uint64_t r = 0; r < f.n_kept; ++r) out_rank[f.rank_to_session[r]] = (uint32_t)r;
        return SRN_OK; });
}
int srn_index_find_attributes(const srn_index_t* idx, uint64_t item_id, uint8_t* out_flags) {
    if (!idx || !out_flags) return fail(SRN_EINVAL, "null argument");
    const uint32_t j = idx->flat.lookup(item_id);
    *out_flags = j == kNone ? (uint8_t)SRN_ATTR_NONE : idx->flat.attr[j];   // (None for an unknown item, like HashMap::get, vmis_index.rs:417-419)
    return SRN_OK;
}
// find_neighbors (vmis_index.rs:325-415) by itself: the k neighbours of an evolving session as (reference session index, similarity = numerator / U), canonical
// semantics, best first -- similarity descending, ties: the more recent session first.  The GPU does the work (the general kernel with its
// neighbour dump); not a debug aid: same k / m / session-length limits as srn_predict, re-entrant.
int srn_find_neighbors(const srn_index_t* idx, const uint64_t* evolving, size_t len, size_t k, size_t m, uint32_t* out_sessions, double* out_scores, size_t* out_n) {
    return guarded([&]() -> int {
        if (!out_n) return fail(SRN_EINVAL, "null out_n");
        *out_n = 0;
        if (!evolving || len == 0) return fail(SRN_EINVAL, "empty evolving session");
        if (len > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "evolving session longer than SRN_MAX_SESSION_LEN");
        int rc = check_predict_args(idx, k, m, 1); if (rc) return rc;
        rc = check_not_a_shard(idx); if (rc) return rc;
        if (!out_sessions || !out_scores) return fail(SRN_EINVAL, "null buffer");
        std::vector<uint32_t> nb_rank(k), nb_num(k); uint32_t nb_cnt = 0, cnt = 0, stats[8] = {0};
        uint64_t id1 = 0; double sc1 = 0.0;
        const uint32_t q_off[2] = {0u, (uint32_t)len};
        rc = device_predict_host(idx->dev, idx->flat, launch_params(1, k, m, 1, 0, len), HostRows{evolving, q_off, &id1, &sc1, &cnt, stats, nb_rank.data(), nb_num.data(), &nb_cnt});
        if (rc) return rc;
        if (cnt == 0xFFFFFFFFu) return fail(SRN_ERANGE, "the query exceeded the kernel's table limits");
        size_t U = 0;   // distinct raw ids, known or not (vmis_index.rs:334-352: the decay's denominator)
        for (size_t i = 0; i < len; ++i) { bool first = true; for (size_t j = 0; j < i; ++j) first = first && evolving[j] != evolving[i]; U += first; }
        const FlatIndex* hf = host_flat(idx); if (!hf) return SRN_EHIP;
        std::vector<uint32_t> ord(nb_cnt);
        for (uint32_t i = 0; i < nb_cnt; ++i) ord[i] = i;
        std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return nb_num[a] != nb_num[b] ? nb_num[a] > nb_num[b] : nb_rank[a] > nb_rank[b]; });
        for (uint32_t i = 0; i < nb_cnt; ++i) { out_sessions[i] = hf->rank_to_session[nb_rank[ord[i]]]; out_scores[i] = (double)nb_num[ord[i]] / (double)U; }
        *out_n = nb_cnt;
        return SRN_OK; });
}

void srn_index_free(srn_index_t* idx) {
    if (!idx) return;
    if (idx->dev) (void)device_result_cache_disable(idx->dev);
    device_release(idx->dev);
    if (idx->comb) combiner_free(idx->comb);
    delete idx;
}

int srn_predict(const srn_index_t* idx, const uint64_t* evolving, size_t len, size_t k, size_t m, size_t how_many,
                int enable_business_logic, uint64_t* out_ids, double* out_scores, size_t* out_n) {
    return guarded([&]() -> int {
        if (!out_n) return fail(SRN_EINVAL, "null out_n");
        *out_n = 0;
        if (!evolving || len == 0) return fail(SRN_EINVAL, "empty evolving session (the reference panics: src/vmisknn/mod.rs:157)");
        if (len > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "evolving session longer than SRN_MAX_SESSION_LEN");
        // (round 6) a resident workgroup of the persistent latency path, if the handle has them and this call is what they serve: no launch at all
        if (idx && idx->dev && out_ids && out_scores && len <= 16 && k <= 0xFFFFFFFFull && m <= 0xFFFFFFFFull && how_many <= 0xFFFFFFFFull &&
            device_serve_predict(idx->dev, evolving, (uint32_t)len, (uint32_t)k, (uint32_t)m, (uint32_t)how_many, enable_business_logic ? SRN_FLAG_BUSINESS_LOGIC : 0u, out_ids, out_scores, out_n) == 0) {
            device_result_cache_bypassed(idx->dev);
            return SRN_OK;
        }
        // concurrent calls on one handle share launches (srn_combine.cpp); a lone caller runs its own round of one at once
        const int lanes = knob_predict_lanes();
        if (lanes > 0 && idx && idx->comb) {
            int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
            rc = check_not_a_shard(idx); if (rc) return rc;
            if (!out_ids || !out_scores) return fail(SRN_EINVAL, "null buffer");
            return combiner_predict(idx->comb, idx, evolving, len, k, m, how_many, enable_business_logic ? SRN_FLAG_BUSINESS_LOGIC : 0, out_ids, out_scores, out_n,
                                    lanes, knob_tiny_max());
        }
        const uint32_t q_off[2] = {0, (uint32_t)len}; uint32_t cnt = 0;
        int rc = predict_host(idx, evolving, q_off, 1, k, m, how_many, enable_business_logic ? SRN_FLAG_BUSINESS_LOGIC : 0, out_ids,
                              out_scores, &cnt, nullptr, nullptr, nullptr, nullptr);
        if (rc == SRN_OK) *out_n = cnt;
        return rc; });
}

// ---- the persistent latency path (srn_latency.hip, "serve") ----
int srn_index_serve_start(srn_index_t* idx, size_t k, size_t m, size_t how_many, int enable_business_logic, unsigned lanes, unsigned max_items_in_session, unsigned idle_ms) {
    return guarded([&]() -> int {
        if (!idx) return fail(SRN_EINVAL, "null index");
        if (!idx->dev) return fail(SRN_ENODEV, "index has no device attached");
        int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
        rc = check_not_a_shard(idx); if (rc) return rc;
        return device_serve_start(idx->dev, idx->flat, (uint32_t)k, (uint32_t)m, (uint32_t)how_many, enable_business_logic ? SRN_FLAG_BUSINESS_LOGIC : 0u, lanes, max_items_in_session, idle_ms); });
}
int srn_index_serve_stop(srn_index_t* idx) {
    return guarded([&]() -> int {
        if (!idx) return fail(SRN_EINVAL, "null index");
        return idx->dev ? device_serve_stop(idx->dev) : SRN_OK; });
}
int srn_index_serve_stats(const srn_index_t* idx, uint64_t* out_served, uint64_t* out_not_served, uint64_t* out_launches, uint32_t* out_lanes) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return device_serve_stats(idx->dev, out_served, out_not_served, out_launches, out_lanes);
}

// ---- the device result cache (srn_result_cache.hip) ----
int srn_index_result_cache_enable(srn_index_t* idx, size_t rows, size_t max_len, size_t k, size_t m, size_t how_many, unsigned flags) {
    return guarded([&]() -> int {
        if (!idx) return fail(SRN_EINVAL, "null index");
        if (flags & ~(unsigned)SRN_FLAG_BUSINESS_LOGIC) return fail(SRN_EINVAL, "srn_index_result_cache_enable: unknown flags");
        if (rows == 0) return fail(SRN_EINVAL, "srn_index_result_cache_enable: rows must be > 0");
        if (max_len < 1 || max_len > 8) return fail(SRN_ERANGE, "srn_index_result_cache_enable: max_len must be 1..8");
        int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
        rc = check_not_a_shard(idx); if (rc) return rc;
        return device_result_cache_enable(idx->dev, rows, (uint32_t)max_len, (uint32_t)k, (uint32_t)m, (uint32_t)how_many, flags); });
}
int srn_index_result_cache_disable(srn_index_t* idx) {
    return guarded([&]() -> int {
        if (!idx) return fail(SRN_EINVAL, "null index");
        return idx->dev ? device_result_cache_disable(idx->dev) : SRN_OK; });
}
int srn_index_result_cache_clear(srn_index_t* idx) {
    return guarded([&]() -> int {
        if (!idx) return fail(SRN_EINVAL, "null index");
        if (!idx->dev) return fail(SRN_ENODEV, "index has no device attached");
        return device_result_cache_clear(idx->dev); });
}
int srn_index_result_cache_stats(const srn_index_t* idx, srn_result_cache_stats_t* out) {
    return guarded([&]() -> int {
        if (!idx || !out) return fail(SRN_EINVAL, "null argument");
        if (!idx->dev) return fail(SRN_ENODEV, "index has no device attached");
        return device_result_cache_stats(idx->dev, out); });
}

int srn_predict_stats(const srn_index_t* idx, uint64_t* out_rounds, uint64_t* out_requests, uint64_t* out_max_round) {
    if (!idx || !idx->comb) return fail(SRN_ENODEV, "index has no device attached");
    combiner_stats(idx->comb, out_rounds, out_requests, out_max_round);
    return SRN_OK;
}

int srn_predict_batch(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t k, size_t m,
                      size_t how_many, unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts) {
    return guarded([&]() -> int { return predict_host(idx, items_flat, q_off, nq, k, m, how_many, flags, out_ids, out_scores,
                                                       out_counts, nullptr, nullptr, nullptr, nullptr); });
}

int srn_predict_batch_debug(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t k, size_t m,
                            size_t how_many, unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts,
                            uint32_t* out_stats, uint32_t* out_nb_sessions, uint32_t* out_nb_num, uint32_t* out_nb_counts) {
    return guarded([&]() -> int { return predict_host(idx, items_flat, q_off, nq, k, m, how_many, flags, out_ids, out_scores,
                                                       out_counts, out_stats, out_nb_sessions, out_nb_num, out_nb_counts); });
}

int srn_predict_batch_device(const srn_index_t* idx, const uint64_t* d_items_flat, const uint32_t* d_q_off, size_t nq,
                             size_t max_len_hint, size_t k, size_t m, size_t how_many, unsigned flags, uint64_t* d_out_ids,
                             double* d_out_scores, uint32_t* d_out_counts, void* stream) {
    return guarded([&]() -> int {
        int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
        rc = check_not_a_shard(idx); if (rc) return rc;
        if (nq == 0) return SRN_OK;
        if (!d_items_flat || !d_q_off || !d_out_ids || !d_out_scores || !d_out_counts) return fail(SRN_EINVAL, "null buffer");
        if (nq > 0x7FFFFFFFull) return fail(SRN_ERANGE, "too many queries in one batch");
        if (max_len_hint == 0 || max_len_hint > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "max_len_hint out of range");
        return device_predict_device(idx->dev, idx->flat, launch_params(nq, k, m, how_many, flags, max_len_hint, d_items_flat, d_q_off, d_out_ids, d_out_scores, d_out_counts), stream); });
}

// SRN_FLAG_FILL without a ranking: refused before anything is enqueued
static int check_has_fallback(const srn_index_t* idx) {
    return device_has_fallback(idx->dev) ? SRN_OK : fail(SRN_ESTATE, "SRN_FLAG_FILL: the index has no fallback ranking (srn_index_set_fallback)");
}
// ---- exclusion lists (srn_exclude.hip) ----
// the checks both forms share; *wide = the internal how_many
static int check_excl_args(const srn_index_t* idx, size_t nq, size_t max_len_hint, const void* excl_flat, const void* excl_off, size_t max_excl, size_t k, size_t m, size_t how_many,
                           unsigned flags, size_t* wide) {
    int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
    rc = check_not_a_shard(idx); if (rc) return rc;
    if (flags & ~(unsigned)(SRN_FLAG_BUSINESS_LOGIC | SRN_FLAG_INPUTS_RESIDENT | SRN_FLAG_EXCLUDE_SESSION | SRN_FLAG_FILL)) return fail(SRN_EINVAL, "srn_predict_batch_excl: unknown flags");
    if (nq > 0x7FFFFFFFull) return fail(SRN_ERANGE, "too many queries in one batch");
    if (max_len_hint == 0 || max_len_hint > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "max_len_hint out of range");
    if (max_excl > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "how_many + max_excl above SRN_MAX_HOW_MANY");
    *wide = wide_how_many(how_many, max_excl, (flags & SRN_FLAG_EXCLUDE_SESSION) != 0u, max_len_hint);
    if (*wide > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "how_many + max_excl (+ max_len_hint - 1 with SRN_FLAG_EXCLUDE_SESSION) above SRN_MAX_HOW_MANY");
    if (max_excl > 0 && (!excl_flat || !excl_off)) return fail(SRN_EINVAL, "null exclusion list with max_excl > 0");
    if (flags & SRN_FLAG_FILL) return check_has_fallback(idx);
    return SRN_OK;
}
static RowRule excl_rule(const uint64_t* excl_flat, const uint32_t* excl_off, size_t max_excl, unsigned flags) {
    return RowRule{excl_flat, excl_off, (uint32_t)max_excl, (flags & SRN_FLAG_EXCLUDE_SESSION) != 0u, (flags & SRN_FLAG_FILL) != 0u};
}
int srn_predict_batch_device_excl(const srn_index_t* idx, const uint64_t* d_items_flat, const uint32_t* d_q_off, size_t nq, size_t max_len_hint,
                                  const uint64_t* d_excl_flat, const uint32_t* d_excl_off, size_t max_excl, size_t k, size_t m, size_t how_many, unsigned flags,
                                  uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts, void* stream) {
    return guarded([&]() -> int {
        size_t wide = 0;
        int rc = check_excl_args(idx, nq, max_len_hint, d_excl_flat, d_excl_off, max_excl, k, m, how_many, flags, &wide); if (rc) return rc;
        if (nq == 0) return SRN_OK;
        if (!d_items_flat || !d_q_off || !d_out_ids || !d_out_scores || !d_out_counts) return fail(SRN_EINVAL, "null buffer");
        // (the launch sequence never sees the rule's flags: device_fast_eligible sends any flag but the business rules to the general kernel)
        const LaunchParams p = launch_params(nq, k, m, how_many, flags & ~(unsigned)(SRN_FLAG_EXCLUDE_SESSION | SRN_FLAG_FILL), max_len_hint, d_items_flat, d_q_off, d_out_ids, d_out_scores, d_out_counts);
        return device_predict_device(idx->dev, idx->flat, p, stream, excl_rule(d_excl_flat, d_excl_off, max_excl, flags)); });
}
int srn_predict_batch_excl(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, const uint64_t* excl_flat, const uint32_t* excl_off, size_t max_excl,
                           size_t k, size_t m, size_t how_many, unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts) {
    return guarded([&]() -> int {
        if (nq == 0) { size_t wide = 0; return check_excl_args(idx, 0, 1, excl_flat, excl_off, max_excl, k, m, how_many, flags, &wide); }
        if (!items_flat || !q_off || !out_ids || !out_scores || !out_counts) return fail(SRN_EINVAL, "null buffer");
        if (nq > 0x7FFFFFFFull) return fail(SRN_ERANGE, "too many queries in one batch");
        uint32_t max_len = 0;
        int rc = scan_q_off(q_off, nq, &max_len); if (rc) return rc;
        size_t wide = 0;
        rc = check_excl_args(idx, nq, max_len, excl_flat, excl_off, max_excl, k, m, how_many, flags & ~(unsigned)SRN_FLAG_INPUTS_RESIDENT, &wide); if (rc) return rc;
        if (max_excl) for (size_t q = 0; q < nq; ++q) if (excl_off[q + 1] < excl_off[q]) return fail(SRN_EINVAL, "excl_off not monotone");
        rc = device_predict_host(idx->dev, idx->flat, launch_params(nq, k, m, how_many, flags & (unsigned)SRN_FLAG_BUSINESS_LOGIC, max_len),
                                 HostRows{items_flat, q_off, out_ids, out_scores, out_counts}, excl_rule(excl_flat, excl_off, max_excl, flags));
        if (rc) return rc;
        return wide == how_many ? check_all_served(out_counts, nq) : SRN_OK; });   // (nothing could be excluded: the plain call's contract)
}

int srn_debug_exclude_filter(const srn_index_t* idx, size_t nq, const uint64_t* d_wide_ids, const double* d_wide_scores, const uint32_t* d_wide_counts, size_t wide, const uint64_t* d_excl_flat,
                             const uint32_t* d_excl_off, size_t max_excl, const uint64_t* d_items_flat, const uint32_t* d_q_off, size_t how_many, uint64_t* d_out_ids, double* d_out_scores,
                             uint32_t* d_out_counts, void* stream) {
    return guarded([&]() -> int {
        if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
        if (!d_wide_ids || !d_wide_scores || !d_wide_counts || !d_out_ids || !d_out_scores || !d_out_counts || (d_excl_flat != nullptr) != (d_excl_off != nullptr) || (d_items_flat && !d_q_off))
            return fail(SRN_EINVAL, "null buffer");
        if (nq > 0x7FFFFFFFull || how_many == 0 || wide < how_many || wide > SRN_MAX_HOW_MANY || max_excl > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "srn_debug_exclude_filter: sizes out of range");
        return device_exclude_filter(idx->dev, (uint32_t)nq, d_wide_ids, d_wide_scores, d_wide_counts, (uint32_t)wide, d_excl_flat, d_excl_off, (uint32_t)max_excl, d_items_flat, d_q_off,
                                     d_out_ids, d_out_scores, d_out_counts, (uint32_t)how_many, stream); });
}

int srn_debug_fill(const srn_index_t* idx, size_t nq, uint64_t* d_ids, double* d_scores, uint32_t* d_counts, size_t how_many, const uint64_t* d_excl_flat, const uint32_t* d_excl_off,
                   const uint64_t* d_items_flat, const uint32_t* d_q_off, unsigned flags, void* stream) {
    return guarded([&]() -> int {
        if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
        if (!d_ids || !d_scores || !d_counts || !d_items_flat || !d_q_off || (d_excl_flat != nullptr) != (d_excl_off != nullptr)) return fail(SRN_EINVAL, "null buffer");
        if (nq > 0x7FFFFFFFull || how_many == 0 || how_many > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "srn_debug_fill: sizes out of range");
        int rc = check_has_fallback(idx); if (rc) return rc;
        return device_fill(idx->dev, (uint32_t)nq, d_ids, d_scores, d_counts, (uint32_t)how_many, d_excl_flat, d_excl_off, d_items_flat, d_q_off, (flags & SRN_FLAG_EXCLUDE_SESSION) != 0u,
                           (flags & SRN_FLAG_BUSINESS_LOGIC) != 0u, stream); });
}

int srn_debug_class_counts(const uint64_t* acc, size_t n_waves, uint32_t* out16, int device) {
    return guarded([&]() -> int { return device_debug_class_counts(acc, n_waves, out16, device); });
}

int srn_debug_merge_pair(uint32_t* room, const uint32_t* pairs, size_t n_pairs, int device) {
    return guarded([&]() -> int { return device_debug_merge_pair(room, pairs, n_pairs, device); });
}

int srn_index_reserve(const srn_index_t* idx, size_t nq, size_t max_len_hint, size_t k, size_t m, size_t how_many, unsigned flags, void* stream) {
    return guarded([&]() -> int {
        int rc = check_predict_args(idx, k, m, how_many); if (rc) return rc;
        if (nq == 0 || nq > 0x7FFFFFFFull) return fail(SRN_ERANGE, "nq out of range");
        if (max_len_hint == 0 || max_len_hint > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "max_len_hint out of range");
        return device_reserve(idx->dev, idx->flat, launch_params(nq, k, m, how_many, flags, max_len_hint), stream); });
}

int srn_last_kernel_ms(const srn_index_t* idx, double* out_ms_main, double* out_ms_retry, uint32_t* out_retried) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return guarded([&]() -> int { return device_last_kernel_ms(idx->dev, out_ms_main, out_ms_retry, out_retried); });
}

// ---- item-sharded index (DESIGN.md "Multi-GPU"): one shard per GPU, three kernel stages around three collectives ----
int srn_index_build_shard(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len, double idf_weighting,
                          uint32_t shard, uint32_t n_shards, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!sessions || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        srn_index* ix = new srn_index();
        return finish_index(ix, build_flat_index(*sessions, m_index, max_session_len, idf_weighting, shard, n_shards, ix->flat), device, out); });
}
int srn_index_shard(const srn_index_t* full, uint32_t shard, uint32_t n_shards, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!full || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        { int rc0 = check_has_rows(full->flat, "srn_index_shard"); if (rc0) return rc0; }
        const FlatIndex* hf = host_flat(full); if (!hf) return SRN_EHIP;
        srn_index* ix = new srn_index();
        return finish_index(ix, shard_flat_index(*hf, shard, n_shards, ix->flat), device, out); });
}
// The replicated part of an item-sharded index: the whole index's dictionary, idf / attributes and posting lists WITHOUT its rows (config 5: ~10 GB of the 66.6 GB)
int srn_index_postings_view(const srn_index_t* full, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!full || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        if (full->flat.n_shards != 1) return fail(SRN_EINVAL, "the postings view is cut from an UNSHARDED index");
        { int rc0 = check_has_rows(full->flat, "srn_index_postings_view"); if (rc0) return rc0; }
        if (device < 0) return fail(SRN_ENODEV, "a postings view lives on a device");
        const FlatIndex* hf = host_flat(full); if (!hf) return SRN_EHIP;
        srn_index* ix = new srn_index();
        const FlatIndex& f = *hf; FlatIndex& g = ix->flat;
        g.n_items = f.n_items; g.n_sessions_total = f.n_sessions_total; g.n_kept = f.n_kept; g.nnz_rows = 0; g.nnz_post = f.nnz_post; g.m_index = f.m_index;
        g.max_session_len = f.max_session_len; g.max_row_len = f.max_row_len /* (of the index the lists belong to: the shard group derives its choice of pipeline from it, the same on every rank) */; g.idf_weighting = f.idf_weighting; g.lists_complete = f.lists_complete; g.postings_only = true;
        g.total_pairs = f.total_pairs; g.item_id = f.item_id; g.id_rank = f.id_rank; g.idf = f.idf; g.attr = f.attr; g.post_off = f.post_off; g.post_rank = f.post_rank;
        g.id_table = f.id_table; g.id_mask = f.id_mask; g.rank_to_session = f.rank_to_session;   // (srn_index_postings answers in reference session indices)
        ix->dev = device_attach(ix->flat, device); ix->device = device;
        if (!ix->dev) { delete ix; return SRN_EHIP; }
        *out = ix; return SRN_OK; });
}
int srn_index_build_shard_gpu(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len, double idf_weighting,
                              uint32_t shard, uint32_t n_shards, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!sessions || !out) return fail(SRN_EINVAL, "null argument");
        if (device < 0) return fail(SRN_ENODEV, "the GPU index builder needs a device");
        *out = nullptr;
        FlatIndex full;   // built on the GPU, never attached: only the shard goes to HBM
        int rc = build_flat_index_gpu(*sessions, m_index, max_session_len, idf_weighting, device, full);
        if (rc) return rc;
        srn_index* ix = new srn_index();
        return finish_index(ix, shard_flat_index(full, shard, n_shards, ix->flat), device, out); });   // (device >= 0: checked above)
}
int srn_index_load_shard(const char* path, uint32_t shard, uint32_t n_shards, int device, srn_index_t** out) {
    return guarded([&]() -> int {
        if (!path || !out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        FlatIndex full;
        int rc = load_flat_index(path, full);
        if (rc) return rc;
        srn_index* ix = new srn_index();
        rc = full.n_shards == 1 ? shard_flat_index(full, shard, n_shards, ix->flat)
                                : (full.shard == shard && full.n_shards == n_shards ? (ix->flat = std::move(full), SRN_OK) : fail(SRN_EINVAL, "the file holds another shard"));
        return finish_index(ix, rc, device, out); });
}
int srn_kernel_times(const srn_index_t* idx, uint32_t max_n, double* out_ms_main, double* out_ms_retry, uint32_t* out_n) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    if (!out_n) return fail(SRN_EINVAL, "null argument");
    return guarded([&]() -> int { return device_kernel_times(idx->dev, max_n, out_ms_main, out_ms_retry, out_n); });
}

int srn_kernel_times_detail(const srn_index_t* idx, uint32_t max_n, double* out_ms_prep, double* out_ms_fast, double* out_ms_predict,
                            double* out_ms_retry, uint32_t* out_n) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    if (!out_n) return fail(SRN_EINVAL, "null argument");
    return guarded([&]() -> int { return device_kernel_times(idx->dev, max_n, out_ms_predict, out_ms_retry, out_n, out_ms_prep, out_ms_fast); });
}

int srn_kernel_timing(srn_index_t* idx, int enable) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return device_kernel_timing(idx->dev, enable);
}

int srn_debug_phase_cycles(const srn_index_t* idx, int enable, uint64_t* out16) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return guarded([&]() -> int { return device_phase_cycles(idx->dev, enable, (unsigned long long*)out16); });
}

int srn_last_path_counts(const srn_index_t* idx, uint32_t* out_nq, uint32_t* out_general, uint32_t* out_global_pass) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return guarded([&]() -> int { return device_last_path_counts(idx->dev, out_nq, out_general, out_global_pass); });
}
uint32_t srn_debug_shard_nb_positions_stride(size_t k, size_t m) {
    return device_shard_nb_positions_stride(launch_params(1, k, m, 21, 0, 4));
}
int srn_debug_serve_stamps(const srn_index_t* idx, uint32_t* out4) {
    if (!idx || !idx->dev || !out4) return fail(SRN_EINVAL, "null argument");
    return device_serve_last_stamps(idx->dev, out4);
}
int srn_debug_serve_lane_counts(const srn_index_t* idx, unsigned form, uint64_t* out_served, size_t cap, size_t* out_n) {
    if (!idx || !idx->dev || (!out_served && cap)) return fail(SRN_EINVAL, "null argument");
    return device_serve_lane_counts(idx->dev, form, out_served, cap, out_n);
}
int srn_debug_last_mid_count(const srn_index_t* idx, uint32_t* out_listed) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return guarded([&]() -> int { return device_last_mid_count(idx->dev, out_listed); });
}
int srn_debug_prep_records(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t m, size_t max_len, void* out_records, size_t cap_bytes, size_t* out_stride) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return guarded([&]() -> int { return device_debug_prep_records(idx->dev, idx->flat, items_flat, q_off, nq, m, max_len, out_records, cap_bytes, out_stride); });
}
int srn_debug_geometry(const srn_index_t* idx, size_t k, size_t m, size_t max_len, unsigned flags, uint32_t* out_words) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    if (!out_words) return fail(SRN_EINVAL, "null argument");
    if (k == 0 || k > 0xFFFFFFFFull || m == 0 || m > 0xFFFFFFFFull || max_len == 0 || max_len > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "srn_debug_geometry: sizes out of range");
    return guarded([&]() -> int { return device_debug_geometry(idx->dev, idx->flat, launch_params(1, k, m, 21, flags, max_len), out_words); });   // (the geometry reads neither the batch size nor how_many)
}
int srn_debug_last_dedup_count(const srn_index_t* idx, uint32_t* out_merged) {
    if (!idx || !idx->dev || !out_merged) return fail(SRN_EINVAL, "null argument");
    return guarded([&]() -> int { return device_last_dedup_count(idx->dev, out_merged); });
}
int srn_debug_last_light_count(const srn_index_t* idx, uint32_t* out_light) {
    if (!idx || !idx->dev || !out_light) return fail(SRN_EINVAL, "null argument");
    return guarded([&]() -> int { return device_last_light_count(idx->dev, out_light); });
}
int srn_debug_last_big_count(const srn_index_t* idx, uint32_t* out_listed) {
    if (!idx || !idx->dev) return fail(SRN_ENODEV, "index has no device attached");
    return guarded([&]() -> int { return device_last_mid_count(idx->dev, nullptr, out_listed); });
}

int srn_debug_sback_launches(const srn_index_t* idx, uint64_t* out_launches) {
    if (!idx || !idx->dev || !out_launches) return fail(SRN_EINVAL, "null argument / no device");
    *out_launches = device_sback_launches(idx->dev); return SRN_OK;
}

void srn_debug_reload_knobs(void) { reload_knobs(); }

// ---- offline evaluation (srn_eval.hip) ----
static int check_eval_index(const srn_index_t* idx) {
    if (!idx) return fail(SRN_EINVAL, "null index");
    if (!idx->dev) return fail(SRN_ENODEV, "index has no device attached; evaluation runs on the GPU only");
    if (idx->flat.postings_only) return fail(SRN_EINVAL, "a postings-only view holds no rows");
    return check_not_a_shard(idx);
}

// every trial is checked before anything is launched; the checks that need no index come first
static int check_trials(const srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, const srn_eval_result_t* out) {
    if (n_trials && (!trials || !out)) return fail(SRN_EINVAL, "null argument");
    for (size_t t = 0; t < n_trials; ++t) {
        const srn_eval_trial_t& tr = trials[t];
        if (tr.max_items_in_session == 0) return fail(SRN_EINVAL, "max_items_in_session must be > 0");
        if (tr.max_items_in_session > SRN_MAX_SESSION_LEN) return fail(SRN_ERANGE, "max_items_in_session above SRN_MAX_SESSION_LEN: a prefix could exceed the kernels' session limit");
        if (tr.length == 0) return fail(SRN_EINVAL, "length must be > 0");
        if (tr.length > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "length above SRN_MAX_HOW_MANY");
        if (tr.k == 0 || tr.m == 0 || tr.how_many == 0) return fail(SRN_EINVAL, "k, m and how_many must be > 0");
        if (tr.how_many > SRN_MAX_HOW_MANY) return fail(SRN_ERANGE, "how_many above SRN_MAX_HOW_MANY");
        if (tr.k > SRN_MAX_K) return fail(SRN_ERANGE, "k above SRN_MAX_K");
        if (tr.m > 0x7FFFFFFFu) return fail(SRN_ERANGE, "m too large");
        // the serving rules (srn_eval.hip): the history window mirrors srn_device_sessions_set_history and max_items_in_session <= H; the launch sequence runs at
        // how_many + the exclusion lists' capacity
        if (tr.history != 0 && (tr.history < tr.max_items_in_session || tr.history > SRN_MAX_SESSION_LEN))
            return fail(SRN_ERANGE, "history must be 0 or in max_items_in_session..SRN_MAX_SESSION_LEN");
        if (tr.how_many + eval_excl_capacity(tr) > SRN_MAX_HOW_MANY)
            return fail(SRN_ERANGE, "how_many + the exclusion lists' capacity (history, or max_items_in_session) above SRN_MAX_HOW_MANY");
    }
    if (!set) return fail(SRN_EINVAL, "null evaluation set");
    for (size_t t = 0; t < n_trials; ++t) { int rc = check_predict_args(set->idx, trials[t].k, trials[t].m, trials[t].how_many); if (rc) return rc;
                                            if (trials[t].flags & SRN_FLAG_FILL) { rc = check_has_fallback(set->idx); if (rc) return rc; } }
    return SRN_OK;
}

int srn_eval_set_create(const srn_index_t* idx, const uint64_t* items_flat, const uint64_t* sess_off, size_t n_sessions,
                        const uint64_t* train_item_ids, const uint64_t* train_item_counts, size_t n_train_items, srn_eval_set_t** out) {
    return guarded([&]() -> int {
        if (!out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        int rc = check_eval_index(idx); if (rc) return rc;
        if (!sess_off || (sess_off[n_sessions] && !items_flat) || (n_train_items && (!train_item_ids || !train_item_counts))) return fail(SRN_EINVAL, "null buffer");
        if (sess_off[0] != 0) return fail(SRN_EINVAL, "sess_off must start at 0");
        for (size_t s = 0; s < n_sessions; ++s) if (sess_off[s + 1] < sess_off[s]) return fail(SRN_EINVAL, "sess_off not monotone");
        if (n_sessions >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "too many test sessions");
        return eval_set_create(idx, items_flat, sess_off, n_sessions, train_item_ids, train_item_counts, n_train_items, out); });
}

int srn_eval_set_from_tsv(const srn_index_t* idx, const char* test_path, const char* train_path, srn_eval_set_t** out) {
    return guarded([&]() -> int {
        if (!out || !test_path || !train_path) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        int rc = check_eval_index(idx); if (rc) return rc;
        return eval_set_from_tsv(idx, test_path, train_path, out); });
}

int srn_eval_set_from_events(const srn_index_t* idx, const uint64_t* test_session_ids, const uint64_t* test_item_ids, const void* test_times, size_t n_test,
                             const uint64_t* train_item_ids, size_t n_train, unsigned flags, void* stream, srn_eval_set_t** out) {
    return guarded([&]() -> int {
        if (!out) return fail(SRN_EINVAL, "null argument");
        *out = nullptr;
        int rc = check_eval_index(idx); if (rc) return rc;
        if ((n_test && (!test_session_ids || !test_item_ids || !test_times)) || (n_train && !train_item_ids)) return fail(SRN_EINVAL, "null buffer");
        if (flags & ~(SRN_EVENTS_TIME_I64 | SRN_EVENTS_DEVICE)) return fail(SRN_EINVAL, "unknown flags");
        if (n_test >= 0xFFFFFFFFull || n_train >= 0xFFFFFFFFull) return fail(SRN_ERANGE, "an evaluation set takes < 2^32 - 1 test rows and training rows");
        return eval_set_from_events(idx, test_session_ids, test_item_ids, test_times, n_test, train_item_ids, n_train, flags, stream, out); });
}

int srn_evaluate(srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, srn_eval_result_t* out, void* stream) {
    return guarded([&]() -> int {
        int rc = check_trials(set, trials, n_trials, out); if (rc) return rc;
        if (n_trials == 0) return SRN_OK;
        return eval_run(set, trials, n_trials, out, stream, nullptr, 0); });
}

int srn_evaluate_bootstrap(srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, const srn_bootstrap_t* boot, srn_eval_result_t* out, double* rep,
                           void* stream) {
    return guarded([&]() -> int {
        if (!boot || !rep) return fail(SRN_EINVAL, "null argument");
        if (boot->replicates == 0) return fail(SRN_EINVAL, "replicates must be > 0");
        if (boot->flags != 0) return fail(SRN_EINVAL, "srn_bootstrap_t.flags must be 0");
        if (boot->replicates > SRN_MAX_BOOTSTRAP) return fail(SRN_ERANGE, "replicates above SRN_MAX_BOOTSTRAP");
        int rc = check_trials(set, trials, n_trials, out); if (rc) return rc;
        if (n_trials == 0) return SRN_OK;
        return eval_run(set, trials, n_trials, out, stream, nullptr, 0, boot, rep); });
}

int srn_bootstrap_weights(uint64_t seed, uint32_t replicate, uint64_t first_session, size_t n, uint8_t* out) {
    return guarded([&]() -> int {
        if (n && !out) return fail(SRN_EINVAL, "null argument");
        boot_weights_host(seed, replicate, first_session, n, out);
        return SRN_OK; });
}

// a segmentation on its own: everything but n_labels, which needs the set
static int check_segments(const srn_segments_t* seg) {
    if (!seg) return fail(SRN_EINVAL, "null segmentation");
    if (seg->mode < SRN_SEG_STATE || seg->mode > SRN_SEG_CURRENT_COUNT) return fail(SRN_EINVAL, "unknown segmentation mode");
    if (seg->segments == 0) return fail(SRN_EINVAL, "segments must be > 0");
    if (seg->segments > SRN_MAX_SEGMENTS) return fail(SRN_ERANGE, "segments above SRN_MAX_SEGMENTS");
    if (seg->reserved != 0) return fail(SRN_EINVAL, "srn_segments_t.reserved must be 0");
    if (seg->mode == SRN_SEG_LABEL) {
        if (seg->n_labels && !seg->labels) return fail(SRN_EINVAL, "null labels");
        for (size_t s = 0; s < seg->n_labels; ++s)
            if (seg->labels[s] >= seg->segments) return fail(SRN_EINVAL, "a label is not below segments");
    } else if (seg->mode != SRN_SEG_STATE) {
        if (seg->segments > 1 && !seg->bounds) return fail(SRN_EINVAL, "null bounds");
        for (uint32_t j = 0; j + 2 < seg->segments; ++j)
            if (seg->bounds[j] >= seg->bounds[j + 1]) return fail(SRN_EINVAL, "bounds must be strictly ascending");
    }
    return SRN_OK;
}
static int check_labels_fit(const srn_eval_set_t* set, const srn_segments_t* seg) {
    if (seg->mode == SRN_SEG_LABEL && seg->n_labels != set->sess_off.size() - 1) return fail(SRN_EINVAL, "n_labels must be the set's number of test sessions");
    return SRN_OK;
}

int srn_evaluate_segments(srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, const srn_segments_t* seg, const srn_bootstrap_t* boot,
                          srn_eval_result_t* out, srn_eval_segment_t* seg_out, double* rep, double* seg_rep, void* stream) {
    return guarded([&]() -> int {
        int rc = check_segments(seg); if (rc) return rc;
        if (n_trials && !seg_out) return fail(SRN_EINVAL, "null argument");
        if (boot) {
            if (!rep || !seg_rep) return fail(SRN_EINVAL, "null argument");
            if (boot->replicates == 0) return fail(SRN_EINVAL, "replicates must be > 0");
            if (boot->flags != 0) return fail(SRN_EINVAL, "srn_bootstrap_t.flags must be 0");
            if (boot->replicates > SRN_MAX_BOOTSTRAP) return fail(SRN_ERANGE, "replicates above SRN_MAX_BOOTSTRAP");
            if ((uint64_t)seg->segments * boot->replicates > 16ull * SRN_MAX_BOOTSTRAP) return fail(SRN_ERANGE, "segments * replicates above 16 * SRN_MAX_BOOTSTRAP");
        }
        rc = check_trials(set, trials, n_trials, out); if (rc) return rc;
        rc = check_labels_fit(set, seg); if (rc) return rc;
        if (n_trials == 0) return SRN_OK;
        return eval_run(set, trials, n_trials, out, stream, nullptr, 0, boot, rep, seg, seg_out, seg_rep); });
}

int srn_eval_segment_ids(srn_eval_set_t* set, const srn_segments_t* seg, uint16_t* out, size_t cap, size_t* n_queries) {
    return guarded([&]() -> int {
        int rc = check_segments(seg); if (rc) return rc;
        if (!n_queries) return fail(SRN_EINVAL, "null argument");
        if (!set) return fail(SRN_EINVAL, "null evaluation set");
        rc = check_labels_fit(set, seg); if (rc) return rc;
        *n_queries = (size_t)eval_n_queries(set);
        if (!out) return SRN_OK;
        if (cap < *n_queries) return fail(SRN_ERANGE, "segment ids: no room for every query of the set");
        return eval_segment_ids(set, seg, out); });
}

int srn_debug_eval_segment_ms(srn_eval_set_t* set, double* ms_segments, double* ms_segment_bootstrap) {
    return guarded([&]() -> int {
        if (!set) return fail(SRN_EINVAL, "null evaluation set");
        eval_segment_ms(set, ms_segments, ms_segment_bootstrap);
        return SRN_OK; });
}

int srn_debug_eval_terms(srn_eval_set_t* set, const srn_eval_trial_t* trial, double* out_terms, size_t cap, size_t* out_n, srn_eval_result_t* out) {
    return guarded([&]() -> int {
        if (!trial || !out_n) return fail(SRN_EINVAL, "null argument");
        srn_eval_result_t tmp;
        int rc = check_trials(set, trial, 1, &tmp); if (rc) return rc;
        *out_n = (size_t)eval_n_queries(set);
        if (!out_terms) return SRN_OK;
        rc = eval_run(set, trial, 1, &tmp, nullptr, out_terms, cap); if (rc) return rc;
        if (out) *out = tmp;
        return SRN_OK; });
}

void srn_eval_set_free(srn_eval_set_t* set) { eval_set_free(set); }

// ---- device-resident session store (srn_sessions_dev.hip) ----
int srn_device_sessions_create(int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions_t** out) {
    return guarded([&]() -> int { return dsess_create(device, capacity, items_cap, ttl_secs, idle_secs, out); });
}
void srn_device_sessions_free(srn_device_sessions_t* s) { dsess_free(s); }
int srn_device_sessions_get(srn_device_sessions_t* s, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs, uint64_t* out_items, size_t cap, size_t* out_n) {
    return guarded([&]() -> int { return dsess_get(s, key_hi, key_lo, now_secs, out_items, cap, out_n); });
}
int srn_device_sessions_update(srn_device_sessions_t* s, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs, const uint64_t* items, size_t n) {
    return guarded([&]() -> int { return dsess_update(s, key_hi, key_lo, now_secs, items, n); });
}
int srn_device_sessions_sweep(srn_device_sessions_t* s, uint64_t now_secs, uint64_t* n_live) {
    return guarded([&]() -> int { return dsess_sweep(s, now_secs, n_live); });
}
int srn_device_sessions_stats(srn_device_sessions_t* s, srn_device_sessions_stats_t* out) { return guarded([&]() -> int { return dsess_stats(s, out); }); }
int srn_device_sessions_set_history(srn_device_sessions_t* s, size_t history) { return guarded([&]() -> int { return dsess_set_history(s, history); }); }
int srn_device_sessions_history(srn_device_sessions_t* s, size_t* out_history) { return guarded([&]() -> int { return dsess_history(s, out_history); }); }
int srn_device_sessions_timing(srn_device_sessions_t* s, int enable) { return guarded([&]() -> int { return dsess_timing(s, enable); }); }
int srn_device_sessions_last_ms(srn_device_sessions_t* s, double* out_ms_store, double* out_ms_predict) {
    return guarded([&]() -> int { return dsess_last_ms(s, out_ms_store, out_ms_predict); });
}
int srn_debug_device_sessions_last_batch(srn_device_sessions_t* s, const void** d_items, const void** d_q_off, size_t* out_n, size_t* out_max_len,
                                         uint64_t* h_items, size_t cap, uint32_t* h_q_off) {
    return guarded([&]() -> int { return dsess_last_csr(s, d_items, d_q_off, out_n, out_max_len, h_items, cap, h_q_off); });
}

int srn_device_sessions_count(srn_device_sessions_t* s, uint64_t now_secs, uint64_t* occupied, uint64_t* live) {
    return guarded([&]() -> int { return dsess_count(s, now_secs, occupied, live); });
}
int srn_device_sessions_export_device(srn_device_sessions_t* s, uint64_t now_secs, size_t cap, uint64_t* d_key_hi, uint64_t* d_key_lo, uint64_t* d_epoch, uint32_t* d_len,
                                      uint64_t* d_items, size_t items_stride, uint64_t* d_n, void* stream) {
    return guarded([&]() -> int { return dsess_export_device(s, now_secs, cap, d_key_hi, d_key_lo, d_epoch, d_len, d_items, items_stride, d_n, stream); });
}
int srn_device_sessions_export(srn_device_sessions_t* s, uint64_t now_secs, size_t cap, uint64_t* key_hi, uint64_t* key_lo, uint64_t* epoch, uint32_t* len, uint64_t* items,
                               size_t items_stride, size_t* n) {
    return guarded([&]() -> int { return dsess_export_host(s, now_secs, cap, key_hi, key_lo, epoch, len, items, items_stride, n); });
}
int srn_device_sessions_import_device(srn_device_sessions_t* s, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_epoch, const uint32_t* d_len,
                                      const uint64_t* d_items, size_t items_stride, size_t n, void* stream) {
    return guarded([&]() -> int { return dsess_import_device(s, d_key_hi, d_key_lo, d_epoch, d_len, d_items, items_stride, n, stream); });
}
int srn_device_sessions_import(srn_device_sessions_t* s, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* epoch, const uint32_t* len, const uint64_t* items,
                               size_t items_stride, size_t n) {
    return guarded([&]() -> int { return dsess_import_host(s, key_hi, key_lo, epoch, len, items, items_stride, n); });
}
int srn_device_sessions_resize(srn_device_sessions_t* s, size_t capacity, size_t items_cap, uint64_t now_secs) {
    return guarded([&]() -> int { return dsess_resize(s, capacity, items_cap, now_secs); });
}
int srn_device_sessions_set_max_capacity(srn_device_sessions_t* s, size_t max_capacity) { return guarded([&]() -> int { return dsess_set_max_capacity(s, max_capacity); }); }
int srn_device_sessions_growth(srn_device_sessions_t* s, uint64_t* max_capacity, uint64_t* grows, uint64_t* resizes) {
    return guarded([&]() -> int { return dsess_growth(s, max_capacity, grows, resizes); });
}
int srn_device_sessions_save(srn_device_sessions_t* s, const char* path, uint64_t now_secs) { return guarded([&]() -> int { return dsess_save(s, path, now_secs); }); }
int srn_device_sessions_load(const char* path, int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions_t** out) {
    return guarded([&]() -> int { return dsess_load(path, device, capacity, items_cap, ttl_secs, idle_secs, out); });
}
int srn_device_sessions_file_info(const char* path, srn_device_sessions_file_info_t* out) { return guarded([&]() -> int { return dsess_file_info(path, out); }); }
// ---- trending items (srn_trending.hip) ----
int srn_device_sessions_top_items(srn_device_sessions_t* s, uint64_t now_secs, uint64_t since_secs, uint32_t min_count, size_t cap, uint64_t* out_ids, uint32_t* out_counts,
                                  size_t* out_n) {
    return guarded([&]() -> int { return dsess_top_items(s, now_secs, since_secs, min_count, cap, out_ids, out_counts, out_n); });
}
int srn_index_set_fallback_trending(srn_index_t* idx, srn_device_sessions_t* store, uint64_t now_secs, uint64_t since_secs, uint32_t min_count, size_t n, unsigned flags,
                                    size_t* out_trending) {
    return guarded([&]() -> int {
        const std::string who = "srn_index_set_fallback_trending: ";
        if (!idx || !store) return fail(SRN_EINVAL, who + "null argument");
        if (n == 0) return fail(SRN_EINVAL, who + "an empty ranking");
        if (n > SRN_MAX_FALLBACK) return fail(SRN_ERANGE, who + "more than SRN_MAX_FALLBACK ids");
        if (check_fallback_index(idx)) return fail(SRN_EINVAL, who + last_error_string());
        if (!idx->dev) return fail(SRN_ENODEV, who + "the index has no device attached");
        if (dsess_device_of(store) != idx->device) return fail(SRN_EINVAL, who + "the store and the index are on different devices");
        if (out_trending) *out_trending = 0;
        std::vector<uint64_t> list(n);
        size_t ranked = 0;
        int rc = dsess_top_items(store, now_secs, since_secs, min_count, n, list.data(), nullptr, &ranked); if (rc) return rc;
        const size_t trending = std::min(n, ranked);
        list.resize(trending);
        if ((flags & SRN_TRENDING_POPULAR_TAIL) && trending < n) {   // the popularity order (the dense item index) without what the list already holds
            std::vector<uint64_t> have(list);
            std::sort(have.begin(), have.end());
            for (size_t i = 0; i < idx->flat.n_items && list.size() < n; ++i) {
                const uint64_t id = idx->flat.item_id[i];
                if (!std::binary_search(have.begin(), have.end(), id)) list.push_back(id);
            }
        }
        if (list.empty()) return SRN_OK;   // (the ranking stays as it was)
        rc = srn_index_set_fallback(idx, list.data(), list.size()); if (rc) return rc;
        if (out_trending) *out_trending = trending;
        return SRN_OK; });
}

// Every form of the batch call: the checks in srn_predict_batch_device's order, then the store's entry for device or host pointers.  timed (the _at forms, DESIGN.md
// 11.6): `times` is among the buffers; now_secs is then the capacity rule's sweep clock alone
static int recommend_batch(const srn_index_t* idx, srn_device_sessions_t* store, const VisitorBatch& r, const RecommendCall& c, bool timed, bool host) {
    return guarded([&]() -> int {
        int rc = check_predict_args(idx, c.k, c.m, c.how_many); if (rc) return rc;
        rc = check_not_a_shard(idx); if (rc) return rc;
        if (r.n == 0) return SRN_OK;
        if (!has_request_arrays(r, timed) || !c.ids || !c.scores || !c.counts) return fail(SRN_EINVAL, "null buffer");
        if (c.flags & ~(unsigned)(SRN_FLAG_BUSINESS_LOGIC | SRN_FLAG_EXCLUDE_SEEN | SRN_FLAG_FILL)) return fail(SRN_EINVAL, "srn_recommend_batch: unknown flags");
        if ((c.flags & SRN_FLAG_FILL) && (rc = check_has_fallback(idx))) return rc;   // (before the store changes)
        return host ? dsess_recommend_host(idx, store, r, c) : dsess_recommend_device(idx, store, r, c); });
}
int srn_recommend_batch_device(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids,
                               const uint8_t* d_consent, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m, size_t how_many,
                               unsigned flags, uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts, void* stream) {
    return recommend_batch(idx, store, {d_key_hi, d_key_lo, d_item_ids, d_consent, nullptr, n, now_secs},
                           {max_items_in_session, k, m, how_many, flags, d_out_ids, d_out_scores, d_out_counts, stream}, false, false);
}
int srn_recommend_batch(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids,
                        const uint8_t* consent, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m, size_t how_many,
                        unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts) {
    return recommend_batch(idx, store, {key_hi, key_lo, item_ids, consent, nullptr, n, now_secs},
                           {max_items_in_session, k, m, how_many, flags, out_ids, out_scores, out_counts, nullptr}, false, true);
}
int srn_recommend_batch_device_at(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids,
                                  const uint8_t* d_consent, const uint64_t* d_times, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m,
                                  size_t how_many, unsigned flags, uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts, void* stream) {
    return recommend_batch(idx, store, {d_key_hi, d_key_lo, d_item_ids, d_consent, d_times, n, now_secs},
                           {max_items_in_session, k, m, how_many, flags, d_out_ids, d_out_scores, d_out_counts, stream}, true, false);
}
int srn_recommend_batch_at(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids,
                           const uint8_t* consent, const uint64_t* times, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m, size_t how_many,
                           unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts) {
    return recommend_batch(idx, store, {key_hi, key_lo, item_ids, consent, times, n, now_secs},
                           {max_items_in_session, k, m, how_many, flags, out_ids, out_scores, out_counts, nullptr}, true, true);
}

// ---- session harvest (srn_harvest.hip) ----
int srn_harvest_create(int device, size_t capacity, size_t items_cap, uint32_t min_len, srn_harvest_t** out) {
    return guarded([&]() -> int { return harvest_create(device, capacity, items_cap, min_len, out); });
}
int srn_harvest_free(srn_harvest_t* h) { return guarded([&]() -> int { return harvest_free(h); }); }
int srn_device_sessions_set_harvest(srn_device_sessions_t* s, srn_harvest_t* h) { return guarded([&]() -> int { return dsess_set_harvest(s, h); }); }
int srn_harvest_stats(srn_harvest_t* h, srn_harvest_stats_t* out) { return guarded([&]() -> int { return harvest_stats(h, out); }); }
int srn_harvest_export(srn_harvest_t* h, size_t cap, uint64_t* key_hi, uint64_t* key_lo, uint64_t* epoch, uint32_t* len, uint64_t* items, size_t items_stride, size_t* n) {
    return guarded([&]() -> int { return harvest_export_host(h, cap, key_hi, key_lo, epoch, len, items, items_stride, n); });
}
int srn_harvest_export_device(srn_harvest_t* h, size_t cap, uint64_t* d_key_hi, uint64_t* d_key_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items, size_t items_stride,
                              uint64_t* d_n, void* stream) {
    return guarded([&]() -> int { return harvest_export_device(h, cap, d_key_hi, d_key_lo, d_epoch, d_len, d_items, items_stride, d_n, stream); });
}
int srn_harvest_events_device(srn_harvest_t* h, uint64_t id_base, size_t cap_rows, uint64_t* d_session_ids, uint64_t* d_item_ids, int64_t* d_times, uint64_t* d_rows,
                              void* stream) {
    return guarded([&]() -> int { return harvest_events_device(h, id_base, cap_rows, d_session_ids, d_item_ids, d_times, d_rows, stream); });
}
int srn_harvest_clear(srn_harvest_t* h) { return guarded([&]() -> int { return harvest_clear(h); }); }

// ---- click feedback log (srn_feedback.hip) ----
int srn_feedback_create(int device, size_t capacity, size_t row_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_feedback_t** out) {
    return guarded([&]() -> int { return fb_create(device, capacity, row_cap, ttl_secs, idle_secs, out); });
}
void srn_feedback_free(srn_feedback_t* f) { fb_free(f); }
// every form of the observe call; timed (the _at forms): `times` is among the buffers.  Every other check is the log's own
static int feedback_observe(srn_feedback_t* f, const VisitorBatch& r, const ObserveCall& c, bool timed, bool host) {
    return guarded([&]() -> int {
        if (f && r.n && timed && !r.times) return fail(SRN_EINVAL, "srn_feedback_observe: null buffer");
        return host ? fb_observe_host(f, r, c) : fb_observe_device(f, r, c); });
}
int srn_feedback_observe_device(srn_feedback_t* f, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids, const uint8_t* d_consent, size_t n,
                                uint64_t now_secs, const uint64_t* d_ids, const double* d_scores, const uint32_t* d_counts, size_t how_many, uint32_t* d_out_rank,
                                void* stream) {
    return feedback_observe(f, {d_key_hi, d_key_lo, d_item_ids, d_consent, nullptr, n, now_secs}, {d_ids, d_scores, d_counts, how_many, d_out_rank, stream}, false, false);
}
int srn_feedback_observe(srn_feedback_t* f, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids, const uint8_t* consent, size_t n,
                         uint64_t now_secs, const uint64_t* ids, const double* scores, const uint32_t* counts, size_t how_many, uint32_t* out_rank) {
    return feedback_observe(f, {key_hi, key_lo, item_ids, consent, nullptr, n, now_secs}, {ids, scores, counts, how_many, out_rank, nullptr}, false, true);
}
int srn_feedback_observe_device_at(srn_feedback_t* f, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids, const uint8_t* d_consent,
                                   const uint64_t* d_times, size_t n, uint64_t now_secs, const uint64_t* d_ids, const double* d_scores, const uint32_t* d_counts,
                                   size_t how_many, uint32_t* d_out_rank, void* stream) {
    return feedback_observe(f, {d_key_hi, d_key_lo, d_item_ids, d_consent, d_times, n, now_secs}, {d_ids, d_scores, d_counts, how_many, d_out_rank, stream}, true, false);
}
int srn_feedback_observe_at(srn_feedback_t* f, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids, const uint8_t* consent, const uint64_t* times,
                            size_t n, uint64_t now_secs, const uint64_t* ids, const double* scores, const uint32_t* counts, size_t how_many, uint32_t* out_rank) {
    return feedback_observe(f, {key_hi, key_lo, item_ids, consent, times, n, now_secs}, {ids, scores, counts, how_many, out_rank, nullptr}, true, true);
}
int srn_feedback_stats(srn_feedback_t* f, srn_feedback_stats_t* out) { return guarded([&]() -> int { return fb_stats(f, out); }); }
int srn_feedback_histogram(srn_feedback_t* f, uint64_t* hits_model, uint64_t* hits_filled, size_t cap) {
    return guarded([&]() -> int { return fb_histogram(f, hits_model, hits_filled, cap); });
}
int srn_feedback_reset_counters(srn_feedback_t* f) { return guarded([&]() -> int { return fb_reset_counters(f); }); }
int srn_feedback_sweep(srn_feedback_t* f, uint64_t now_secs, uint64_t* n_live) { return guarded([&]() -> int { return fb_sweep(f, now_secs, n_live); }); }
int srn_feedback_get(srn_feedback_t* f, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs, uint64_t* out_ids, size_t cap, uint32_t* out_count, uint32_t* out_n_model,
                     uint64_t* out_epoch) {
    return guarded([&]() -> int { return fb_get(f, key_hi, key_lo, now_secs, out_ids, cap, out_count, out_n_model, out_epoch); });
}
int srn_feedback_bootstrap_enable(srn_feedback_t* f, uint32_t replicates, uint64_t seed) { return guarded([&]() -> int { return fb_boot_enable(f, replicates, seed); }); }
int srn_feedback_bootstrap_disable(srn_feedback_t* f) { return guarded([&]() -> int { return fb_boot_disable(f); }); }
int srn_feedback_bootstrap_info(srn_feedback_t* f, uint32_t* replicates, uint64_t* seed) { return guarded([&]() -> int { return fb_boot_info(f, replicates, seed); }); }
int srn_feedback_bootstrap_read(srn_feedback_t* f, uint64_t* observed, uint64_t* hits_model, uint64_t* hits_filled, size_t replicates_cap, size_t rank_cap) {
    return guarded([&]() -> int { return fb_boot_read(f, observed, hits_model, hits_filled, replicates_cap, rank_cap); });
}
int srn_feedback_bootstrap_weights(uint64_t seed, uint32_t replicate, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out) {
    return guarded([&]() -> int {
        if (n && (!key_hi || !key_lo || !out)) return fail(SRN_EINVAL, "srn_feedback_bootstrap_weights: null argument");
        fb_boot_weights_host(seed, replicate, key_hi, key_lo, n, out);
        return SRN_OK; });
}

// ---- traffic split (srn_arms.hip) ----
// an arm's predict parameters, as recommend_batch checks a call's
static int check_arm(const srn_arm_t& arm, size_t how_many) {
    int rc = check_predict_args(arm.idx, arm.k, arm.m, how_many); if (rc) return rc;
    if ((rc = check_not_a_shard(arm.idx))) return rc;
    if (arm.flags & ~(unsigned)(SRN_FLAG_BUSINESS_LOGIC | SRN_FLAG_EXCLUDE_SEEN | SRN_FLAG_FILL)) return fail(SRN_EINVAL, "srn_recommend_batch: unknown flags");
    if ((arm.flags & SRN_FLAG_FILL) && (rc = check_has_fallback(arm.idx))) return rc;
    return SRN_OK;
}
int srn_traffic_split_create(int device, const uint32_t* weights, size_t n_arms, uint64_t seed, size_t max_batch, size_t max_how_many, srn_traffic_split_t** out) {
    return guarded([&]() -> int { return split_create(device, weights, n_arms, seed, max_batch, max_how_many, out); });
}
int srn_traffic_split_free(srn_traffic_split_t* split) { return guarded([&]() -> int { return split_free(split); }); }
int srn_traffic_split_info(const srn_traffic_split_t* split, srn_traffic_split_info_t* out) { return guarded([&]() -> int { return split_info(split, out); }); }
int srn_traffic_split_set_weights(srn_traffic_split_t* split, const uint32_t* weights, size_t n_arms) {
    return guarded([&]() -> int { return split_set_weights(split, weights, n_arms); });
}
int srn_traffic_split_arms(uint64_t seed, const uint32_t* weights, size_t n_arms, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out) {
    return guarded([&]() -> int { return split_arms_host(seed, weights, n_arms, key_hi, key_lo, n, out); });
}
int srn_traffic_split_timing(srn_traffic_split_t* split, int enable) { return guarded([&]() -> int { return split_timing(split, enable); }); }
int srn_traffic_split_last_ms(srn_traffic_split_t* split, double* ms_front, double* ms_scatter) {
    return guarded([&]() -> int { return split_last_ms(split, ms_front, ms_scatter); });
}
int srn_recommend_batch_split_device(srn_traffic_split_t* split, const srn_arm_t* arms, size_t n_arms, srn_device_sessions_t* store,
                                     const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids, const uint8_t* d_consent, const uint64_t* d_times,
                                     size_t n, uint64_t now_secs, size_t how_many, uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts,
                                     uint8_t* d_out_arm, uint32_t* d_out_rank, int* feedback_rc, void* stream) {
    return guarded([&]() -> int {
        return split_recommend_device(split, arms, n_arms, store, {d_key_hi, d_key_lo, d_item_ids, d_consent, d_times, n, now_secs}, how_many,
                                      {d_out_ids, d_out_scores, d_out_counts, d_out_arm, d_out_rank, feedback_rc}, stream, check_arm); });
}
int srn_recommend_batch_split(srn_traffic_split_t* split, const srn_arm_t* arms, size_t n_arms, srn_device_sessions_t* store,
                              const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids, const uint8_t* consent, const uint64_t* times,
                              size_t n, uint64_t now_secs, size_t how_many, uint64_t* out_ids, double* out_scores, uint32_t* out_counts,
                              uint8_t* out_arm, uint32_t* out_rank, int* feedback_rc) {
    return guarded([&]() -> int {
        return split_recommend_host(split, arms, n_arms, store, {key_hi, key_lo, item_ids, consent, times, n, now_secs}, how_many,
                                    {out_ids, out_scores, out_counts, out_arm, out_rank, feedback_rc}, check_arm); });
}

}  // extern "C"
