/* =====================================================================================
 * serenade_hip.h -- C ABI of libserenade_hip.so: the MI355X (gfx950) implementation of
 * Serenade's VMIS-kNN `predict_next` hot path.
 *
 * The reference (bolcom/serenade @ 2024-11-08, pure Rust) has no FFI of its own; its boundary for
 * this path is the Rust signature
 *
 *   vmisknn::predict<I: SimilarityComputationNew + Send + Sync>(index: &I,
 *       evolving_session: &[u64], k: usize, m: usize, how_many: usize,
 *       enable_business_logic: bool) -> BinaryHeap<ItemScore>        src/vmisknn/mod.rs:118-125
 *
 * plus the index constructors VMISIndex::new_from_csv (src/vmisknn/vmis_index.rs:38-83) and the
 * trait accessors (src/vmisknn/similarity_indexed.rs:8-24).  The entry points below are what a Rust
 * `extern "C"` block in the reference would bind to swap that path for the GPU one (INTEGRATION.md
 * shows the binding).  Plain pointers and sizes only; every function returns 0 or a negative
 * SRN_E* code and never unwinds across the boundary; srn_last_error() gives a thread-local
 * message for the last failure on the calling thread.
 *
 * There is NO CPU fallback behind this ABI: predict calls on an index without an attached device
 * fail with SRN_ENODEV.
 *
 * Result order: every predict entry point writes results score-descending (ties: ascending item
 * id), i.e. already in the `into_sorted_vec()` order all reference callers use
 * (src/bin/evaluator.rs:67-71, src/endpoints/recommend_resource.rs:58-62).
 * ===================================================================================== */
#ifndef SERENADE_HIP_H
#define SERENADE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRN_OK 0
#define SRN_EINVAL (-1) /* null pointer, empty evolving session (reference panics: mod.rs:157), bad CSR */
#define SRN_ENOMEM (-2)
#define SRN_EHIP (-3)    /* a HIP runtime call failed; see srn_last_error() */
#define SRN_ERANGE (-4)  /* k / m / how_many / session length above the compiled kernel limits */
#define SRN_EIO (-5)
#define SRN_ENODEV (-6)  /* index has no device attached (built with device < 0) or no GPU present */
#define SRN_ESTATE (-7)  /* the handle is unusable since an earlier failure (a shard group after a failed batch): free it */
#define SRN_ETIMEOUT (-8) /* srn_shard_group_wait: the batch did not finish in time */

/* compiled kernel limits (srn_limits() reports the same numbers at run time) */
#define SRN_MAX_HOW_MANY 512
#define SRN_MAX_SESSION_LEN 255
#define SRN_MAX_K 8192

/* attribute flags, one byte per item (ProductAttributes, src/vmisknn/vmis_index.rs:23-26) */
#define SRN_ATTR_ADULT 1u
#define SRN_ATTR_FOR_SALE 2u
#define SRN_ATTR_NONE 0xFFu /* item has no attributes (find_attributes() == None, vmis_index.rs:417-419) */

/* predict flags */
#define SRN_FLAG_BUSINESS_LOGIC 1u /* enable_business_logic = true (mod.rs:162-182) */

typedef struct srn_index srn_index_t;
typedef struct srn_sessions srn_sessions_t;

/* Training sessions in the form prepare_hashmap() consumes (src/vmisknn/vmis_index.rs:422-427):
 * session i owns items[sess_off[i] .. sess_off[i+1]) (ascending, de-duplicated item ids) and
 * max_ts[i]; the session's index i is the reference's dense session id. */
typedef struct {
    const uint64_t* sess_off; /* [n_sessions + 1] */
    const uint64_t* items;    /* [sess_off[n_sessions]] */
    const uint32_t* max_ts;   /* [n_sessions] */
    size_t n_sessions;
} srn_sessions_view_t;

typedef struct {
    uint64_t n_items;          /* distinct items in kept sessions */
    uint64_t n_sessions_total; /* sessions handed to the builder */
    uint64_t n_sessions_kept;  /* sessions with len <= max_session_len (vmis_index.rs:452) */
    uint64_t nnz_rows;         /* (session,item) pairs of kept sessions = idf numerator (vmis_index.rs:509) */
    uint64_t nnz_postings;     /* posting entries after truncation to m_index (vmis_index.rs:504) */
    uint64_t m_index;
    uint64_t max_session_len;
    uint64_t max_row_len;      /* longest kept row */
    uint64_t device_bytes;     /* HBM held by the index (0 if host-only) */
    int32_t device;            /* HIP device ordinal, -1 = host-only */
    int32_t offsets_64bit;     /* row offsets stored as u64 (nnz_rows >= 2^32) */
    double idf_weighting;
    uint64_t incomplete_items; /* (round 6) items of a PRE-BUILT index (srn_index_new_from_avro) whose posting list is not "the most recent sessions that hold the item" under any
                                * tie order the loader could infer: queries such an item can affect are served by the general kernel's row pass (lists as given,
                                * vmis_index.rs:201-228), everything else by the fast kernels.  0 for every index built by this library */
} srn_index_info_t;

typedef struct {
    uint32_t max_how_many, max_session_len, max_k, reserved;
} srn_limits_t;

/* ---- training data ---------------------------------------------------------------------- */

/* TSV "SessionId\tItemId\tTime" -> sessions, with the loader semantics of read_from_file()
 * (src/vmisknn/vmis_index.rs:591-686): stable order inside a session, first-occurrence de-dup then
 * ascending sort, max-timestamp updated on non-duplicate rows only, the final row closes the current
 * session without being added and the last session is dropped. */
int srn_sessions_from_tsv(const char* path, srn_sessions_t** out);
int srn_sessions_view(const srn_sessions_t* s, srn_sessions_view_t* out);
/* exact q-quantile of the session lengths (linear interpolation, rounded): the default stand-in for
 * the reference's t-digest estimate qty_events_p99_5 (vmis_index.rs:689-716, used at :67). */
int srn_sessions_length_quantile(const srn_sessions_t* s, double q, uint64_t* out);
void srn_sessions_free(srn_sessions_t* s);
/* read_from_file (vmis_index.rs:591-686) on the GPU: the same sessions as srn_sessions_from_tsv, bit for bit.  The file is read in
 * chunks and parsed on the device; time fields outside the exact decimal form the device certifies are parsed by the host loader's
 * own code.  < 2^32 rows (SRN_ERANGE above: the host loader remains for those).  device < 0: SRN_ENODEV; a missing file: SRN_EIO. */
int srn_sessions_from_tsv_gpu(const char* path, int device, srn_sessions_t** out);
#define SRN_EVENTS_TIME_I64 1u /* times are int64 seconds (negative -> 0) instead of f64 */
#define SRN_EVENTS_DEVICE 2u   /* the three arrays are device memory on `device` (read on `stream`, never copied to the host) */
/* the same semantics over rows already in memory, in file order; times as f64 (rounded like the file's) or,
 * with SRN_EVENTS_TIME_I64, int64 seconds (negative -> 0); SRN_EVENTS_DEVICE: the three arrays are device memory on `device` */
int srn_sessions_from_events(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n,
                             unsigned flags, int device, void* stream, srn_sessions_t** out);
typedef struct {
    uint64_t lines, rows, skipped, host_parsed; /* lines of the file, rows kept, lines skipped (header, empty, unparsable), lines parsed on the host */
    double ms_read, ms_upload, ms_parse, ms_group, ms_download;
} srn_load_info_t;
int srn_sessions_load_info(const srn_sessions_t* s, srn_load_info_t* out); /* zeros for a host-loaded handle */

/* ---- preparing a click log: its rows on the device, and a split by time (srn_split.hip) ----
 * srn_events_from_tsv_gpu holds what srn_sessions_from_tsv_gpu holds just before it groups: the file's rows in file order as three device arrays, the times as
 * rounded seconds (u64), lines the host re-read patched in, skipped lines gone.  The view's pointers are device memory on `device`, valid until srn_events_free,
 * and are passed on with SRN_EVENTS_DEVICE | SRN_EVENTS_TIME_I64.  A file without a row gives n = 0. */
typedef struct srn_events srn_events_t;
typedef struct {
    const uint64_t* session_ids; const uint64_t* item_ids; const uint64_t* times; /* device memory */
    size_t n;
    int32_t device, reserved;
} srn_events_view_t;
int srn_events_from_tsv_gpu(const char* path, int device, srn_events_t** out);
int srn_events_view(const srn_events_t* e, srn_events_view_t* out);
void srn_events_free(srn_events_t* e);

/* srn_events_split: n rows (session, item, time) in file order, passed exactly as to srn_sessions_from_events (host arrays, or device arrays with SRN_EVENTS_DEVICE;
 * f64 times are rounded like the file's, int64 seconds with SRN_EVENTS_TIME_I64 have negative -> 0; every comparison is on these rounded seconds), get one code each.
 * The rule, in this order -- a later step sees only rows no earlier step dropped:
 *   1. last(s) = the largest time of any row of session s.  Sessions are never cut: the evaluator scores a session's later items against its earlier ones.
 *   2. OUT: every row of a session with last(s) < start, or with end > 0 and last(s) >= end.
 *   3. the other sessions are on the test side if last(s) >= cutoff, else on the train side (a test session's early rows may lie before the cutoff).
 *   4. RARE: a train-side row whose item occurs in fewer than min_item_support train-side ROWS (rows, not distinct sessions).
 *   5. SHORT_TRAIN: the remaining rows of a train session with fewer than min_session_len rows left.  One pass, no fixed point: dropping a short session may leave
 *      an item with fewer than min_item_support rows, and it stays.
 *   6. TRAIN: what is left on the train side.
 *   7. UNKNOWN (with SRN_SPLIT_TEST_KNOWN_ITEMS): a test-side row whose item has no TRAIN row.
 *   8. SHORT_TEST: the remaining rows of a test session with fewer than min_session_len rows left.
 *   9. TEST: the rest.
 * code[n] gets the codes; pos[n] for a TRAIN or TEST row the number of earlier rows with the same code, 0xFFFFFFFF otherwise -- both in memory of the inputs' kind.
 * Exact integer work: the outputs are the same bytes from run to run.  The call waits for `stream` (it returns counts).
 * srn_events_take is the stable compaction of one side: row j with code[j] == which goes to out_*[pos[j]]; times are copied as the 8 bytes given.  Device arrays:
 * only enqueued on `stream`; host arrays: done on return.
 * n = 0, a null buffer, cutoff = 0, start >= cutoff or end <= cutoff (when not 0), unknown flags, which not 1 or 2: SRN_EINVAL; n >= 2^32 - 1: SRN_ERANGE;
 * device < 0: SRN_ENODEV. */
#define SRN_SPLIT_TRAIN 1
#define SRN_SPLIT_TEST 2
#define SRN_SPLIT_OUT 16
#define SRN_SPLIT_RARE 17
#define SRN_SPLIT_SHORT_TRAIN 18
#define SRN_SPLIT_UNKNOWN 19
#define SRN_SPLIT_SHORT_TEST 20
#define SRN_SPLIT_TEST_KNOWN_ITEMS 1u
typedef struct {
    uint64_t cutoff;           /* > 0 */
    uint64_t start, end;       /* 0 = none; else start < cutoff < end */
    uint32_t min_item_support; /* 0 reads as 1 */
    uint32_t min_session_len;  /* 0 reads as 1 */
    uint32_t flags;            /* SRN_SPLIT_TEST_KNOWN_ITEMS */
    uint32_t reserved;         /* 0 */
} srn_split_t;
typedef struct {
    uint64_t train_rows, train_sessions, train_items; /* TRAIN rows, the sessions and the distinct items that have one */
    uint64_t test_rows, test_sessions, test_items;    /* the same for TEST */
    uint64_t dropped_out, dropped_rare, dropped_short_train, dropped_unknown, dropped_short_test; /* rows per drop code */
    uint64_t sessions, items;                         /* distinct in the input */
    uint64_t t_min, t_max;                            /* over all rows, rounded seconds */
} srn_split_info_t;
int srn_events_split(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, const srn_split_t* split, int device,
                     void* stream, uint8_t* code, uint32_t* pos, srn_split_info_t* info);
int srn_events_take(const uint8_t* code, const uint32_t* pos, size_t n, uint8_t which, const uint64_t* session_ids, const uint64_t* item_ids, const void* times,
                    unsigned flags, uint64_t* out_sessions, uint64_t* out_items, void* out_times, int device, void* stream);

/* ---- index ------------------------------------------------------------------------------ */

/* prepare_hashmap() (src/vmisknn/vmis_index.rs:422-528) into the flat HBM layout:
 * sessions longer than max_session_len are left out, posting lists are most-recent-first (ties:
 * larger session index first) and truncated to m_index, idf = ln(pairs / sessions_with_item) *
 * idf_weighting, every item {for_sale, not adult}.  device >= 0 uploads to that GPU; device < 0
 * keeps a host-only index (build / save / inspect; predict then fails with SRN_ENODEV). */
int srn_index_build(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len,
                    double idf_weighting, int device, srn_index_t** out);
/* The same index built on the GPU (rocPRIM radix sorts instead of host loops; < 2^32 sessions and interactions).
 * Bit-identical to srn_index_build(); 582 M interactions take seconds instead of ~45 s on one host core. */
int srn_index_build_gpu(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len,
                        double idf_weighting, int device, srn_index_t** out);
/* srn_sessions_from_events + srn_index_build_gpu in one call, with nothing large on the host in between: n event rows passed exactly as to srn_sessions_from_events
 * (host arrays are uploaded once; SRN_EVENTS_DEVICE arrays are read in place on `stream`) are grouped, built and attached on `device`.  max_session_len = 0: the exact
 * p99.5 of the session lengths, from a histogram kernel.  The index is the one srn_index_build_gpu gives for those sessions, bit for bit -- every predict call, every
 * accessor and srn_index_save see the same bytes -- but its host copy is LAZY: the scalars and the per-item arrays (ids, idf, attributes, posting offsets, the id table)
 * are on the host from the start, while the posting lists, the rows and the rank -> session map stay on the device until a call that reads them on the host asks:
 * srn_index_save, srn_index_postings, srn_index_items_for_session, srn_index_session_recency, srn_find_neighbors and the neighbour dump of srn_predict_batch_debug,
 * srn_index_shard, srn_index_postings_view.  That first call downloads them once (under a mutex; concurrent callers wait) and frees the device copies serving does not
 * read.  Predict, evaluate, recommend, the result cache, the fallback rankings, srn_index_set_attributes, srn_index_info and the evaluation sets never trigger it.
 * Unsharded only.  Errors as the two calls it replaces: a NULL array or out, unknown flags, n = 0, m_most_recent_sessions = 0: SRN_EINVAL; device < 0: SRN_ENODEV;
 * n >= 2^32 - 1: SRN_ERANGE. */
int srn_index_from_events_device(const uint64_t* session_ids, const uint64_t* item_ids, const void* times, size_t n, unsigned flags, size_t m_most_recent_sessions,
                                 double idf_weighting, size_t max_session_len, int device, void* stream, srn_index_t** out);
typedef struct {
    int32_t host_complete;          /* 1: every array of the index is on the host (always, unless srn_index_from_events_device built it and no host reader has asked yet) */
    int32_t reserved;
    uint64_t build_bytes_on_device; /* device bytes held only for the deferred download (part of srn_index_info's device_bytes); 0 once host_complete */
    uint64_t materialisations;      /* downloads of the large arrays so far: 0 or 1 */
    double ms_upload, ms_group, ms_quantile, ms_build, ms_items, ms_attach; /* srn_index_from_events_device's stages: host rows up | times + grouping | the length
                                     * quantile | the builder's sorts and scans | per-item arrays down + idf + id table | row slots and the rest of the attach; else 0 */
    double ms_materialize;          /* the deferred download, once it has happened */
} srn_index_host_state_t;
int srn_index_host_state(const srn_index_t* idx, srn_index_host_state_t* out);
int srn_index_materialize(srn_index_t* idx); /* bring the host copy up to date now; idempotent, SRN_OK on any index */
/* VMISIndex::new_from_csv(path, m_most_recent_sessions, idf_weighting) (vmis_index.rs:38-83);
 * max_session_len = 0 selects the exact p99.5 of the session lengths. */
int srn_index_new_from_csv(const char* path, size_t m_most_recent_sessions, double idf_weighting,
                           size_t max_session_len, int device, srn_index_t** out);
/* VMISIndex::new_from_csv with the GPU loader + GPU builder (falls back to the host builder exactly where srn_index_new_from_csv does) */
int srn_index_new_from_csv_gpu(const char* path, size_t m_most_recent_sessions, double idf_weighting,
                               size_t max_session_len, int device, srn_index_t** out);
/* VMISIndex::new(base_path) (src/vmisknn/vmis_index.rs:85-314): the pre-built production index, two directories of Avro
 * object-container files (codec null or snappy):
 *   <base>/itemindex/[files].avro     {ItemId: long, session_indices_time_ordered: array<int>, idf: double, ForSale, IsAdult: boolean}
 *   <base>/sessionindex/[files].avro  {SessionIndex: int, item_ids_asc: array<long>, Time: int}
 * Posting lists, idf and the product flags are taken from the files as they are (nothing is recomputed); the lists must be
 * what their name says -- each item's most recent sessions -- or the call fails with SRN_EINVAL.  device < 0: host only. */
int srn_index_new_from_avro(const char* base_path, int device, srn_index_t** out);
int srn_index_save(const srn_index_t* idx, const char* path);
int srn_index_load(const char* path, int device, srn_index_t** out);
/* replace ProductAttributes of the given items (the Avro path carries real flags, vmis_index.rs:223-228) */
int srn_index_set_attributes(srn_index_t* idx, const uint64_t* item_ids, const uint8_t* flags, size_t n);
int srn_index_info(const srn_index_t* idx, srn_index_info_t* out);
/* posting list of one item as reference session indices (most recent first) and its idf;
 * *out_len = -1 if the item is unknown.  For index-parity tests and debugging. */
int srn_index_postings(const srn_index_t* idx, uint64_t item_id, uint32_t* out_sessions, size_t cap,
                       int64_t* out_len, double* out_idf);
/* The other accessors of the trait predict() is generic over (SimilarityComputationNew, src/vmisknn/similarity_indexed.rs:9-23) -- with srn_index_postings' idf they
 * are what `impl SimilarityComputationNew for HipVMISIndex` needs:
 *   items_for_session(&u32) -> &[u64]   (vmis_index.rs:317-319)  the row of a session by its reference index, ascending item ids; *out_len = its length (items beyond
 *                                        `cap` are not written).  Rows are kept for the sessions that can be neighbours (len <= max_session_len, vmis_index.rs:452); any
 *                                        other session index: SRN_ERANGE (the reference keeps those rows too, :79, but never reads them on this path)
 *   find_attributes(&u64) -> Option<&ProductAttributes>   (vmis_index.rs:417-419)  *out_flags = SRN_ATTR_* bits, SRN_ATTR_NONE for None (unknown item or no attributes)
 *   find_neighbors(&[u64], k, m) -> BinaryHeap<SessionScore>   (vmis_index.rs:325-415)  the neighbour sessions as (reference session index, similarity = numerator / U),
 *                                        best first (similarity desc, ties: more recent first -- the reference's heap order is unspecified); room for k entries; runs on
 *                                        the GPU, canonical semantics as everywhere */
int srn_index_items_for_session(const srn_index_t* idx, uint32_t session, uint64_t* out_items, size_t cap, size_t* out_len);
int srn_index_find_attributes(const srn_index_t* idx, uint64_t item_id, uint8_t* out_flags);
/* The recency order this index serves with -- the total order behind "most recent" in find_neighbors (session_to_max_time_stamp, vmis_index.rs:33, 358-383, 404-410):
 * out_rank[s] = the recency rank of reference session s (0 = oldest; ascending max timestamp; sessions of EQUAL timestamp, which the reference leaves to its containers,
 * by SessionIndex -- or, for a pre-built Avro index, in the order its producer's list cuts imply), 0xFFFFFFFF for a session that is in no posting list and keeps no row.
 * Room for srn_index_info().n_sessions_total entries.  What a checker needs to state the canonical answer for an index with tied timestamps. */
int srn_index_session_recency(const srn_index_t* idx, uint32_t* out_rank, size_t cap);
int srn_find_neighbors(const srn_index_t* idx, const uint64_t* evolving, size_t len, size_t k, size_t m,
                       uint32_t* out_sessions, double* out_scores, size_t* out_n);
void srn_index_free(srn_index_t* idx);

/* ---- predict ---------------------------------------------------------------------------- */

/* One evolving session (oldest item first, like the reference slice).  out_ids / out_scores have
 * room for how_many entries; *out_n receives the number written.  Unknown items give *out_n = 0
 * with SRN_OK (vmis_index.rs:350); an empty session is SRN_EINVAL (the reference panics). */
int srn_predict(const srn_index_t* idx, const uint64_t* evolving, size_t len, size_t k, size_t m,
                size_t how_many, int enable_business_logic, uint64_t* out_ids, double* out_scores,
                size_t* out_n);
/* ---- the persistent latency path (round 6) ------------------------------------------------------------------------------------------------------------
 * srn_predict is the reference's call shape (one evolving session per call: src/endpoints/recommend_resource.rs:56, src/bin/evaluator.rs:58).  On the one-launch form a
 * call costs ~28 us from a C++ host, of which ~18 us are the GPU's work; the rest is queue submission and completion signalling.  srn_index_serve_start parks `lanes`
 * (<= 256) RESIDENT workgroups on the index's GPU (a CU each, ONE launch on a stream of the lowest priority; with max_items_in_session > 4 a second launch of as many
 * workgroups of the form that serves sessions of 5..10 items; sessions of more items always take the launch path): a call of
 * srn_predict with the same k / m / how_many / business-logic flag then posts its session to a free one through pinned memory and spins on the answer -- no launch.
 * A session the resident form cannot finish (0.3-3 % of config 3's: merged lists beyond its layout, > 63 scored candidates of a small query), a call with other
 * parameters, and a call that finds every resident workgroup taken run exactly as without this: the rows are the same bytes either way.
 *   idle_ms: a resident workgroup leaves by itself after that long without a request (a host that died leaves nothing behind); the next call that wants it starts it again.
 *   Anything in this library that frees device memory or synchronises the device makes the resident workgroups leave first (they come back on demand): allocate and
 *   reserve (srn_index_reserve) BEFORE serving.  APPLICATION code that calls hipFree / hipDeviceSynchronize on this device while workgroups are resident waits until they
 *   leave (idle_ms at most): call srn_index_serve_stop first.
 *   Measured on config 3 (C++ host, profiles/r06_latency_resident_cfg3.json): p50 / p90 22.6 / 27.4 us against 27.8 / 32.7 on the launch path; 16 callers on 16 resident
 *   workgroups 23.7 / 30.0 us and 655 K requests/s against 62.8 / 86.6 us and 246 K.  srn_index_serve_stop may be called while other threads are inside srn_predict.
 * srn_index_serve_stats: sessions answered by a resident workgroup | sent to the launch path | kernel launches so far (1 per form + restarts) | resident workgroups. */
int srn_index_serve_start(srn_index_t* idx, size_t k, size_t m, size_t how_many, int enable_business_logic, unsigned lanes, unsigned max_items_in_session, unsigned idle_ms);
int srn_index_serve_stop(srn_index_t* idx);
int srn_index_serve_stats(const srn_index_t* idx, uint64_t* out_served, uint64_t* out_not_served, uint64_t* out_launches, uint32_t* out_lanes);

/* ---- the device result cache ----------------------------------------------------------------------------------------------------------
 * predict_next is a pure function of the index, the call's parameters and the query's item sequence.  srn_index_result_cache_enable keeps served rows in device memory
 * ACROSS calls: a later query with the same sequence gets the cached row -- the very bytes the kernels wrote -- instead of being computed.  Opt-in; without it nothing
 * changes (same plan, same kernels, same buffers).
 *   rows      entries of the table (rounded up to whole buckets of `ways` entries; 12 + 8 * max_len + 16 * how_many bytes each).  ALL device memory of the cache is
 *             allocated here (hipMalloc synchronises the device: enable before serving); calls allocate nothing for it afterwards.
 *   max_len   1..8: sequences of 1..max_len items are cacheable.  The key is (length, the raw 64-bit ids in order), compared in full on every probe.
 *   k, m, how_many, enable_business_logic   fixed here: the parameters the cached rows are computed with.  They are not part of the key.
 * The cache is used by every call of the batch launch sequence that has these parameters and is on the fast path (m and how_many within the fast kernels, no SRN_NO_FAST):
 * srn_predict_batch_device, srn_predict_batch's chunked path, srn_recommend_batch / _device, the batcher's batches.  Every other call on the index BYPASSES it, computes
 * as without a cache and counts one bypassed_calls: other parameters, host batches of <= SRN_TINY_MAX sessions and srn_predict (the latency paths), the resident serve
 * path, srn_predict_batch_debug, srn_find_neighbors, srn_evaluate.  An item shard has no cache (SRN_EINVAL).
 * A call that uses the cache is served in the sorted order at every batch size, and SRN_FLAG_INPUTS_RESIDENT is ignored for it: the flag is a permission, and the hit
 * rows are written into the caller's output buffers early in the call, which a previous call may still own on the library's side stream.
 * Replacement: an empty entry of the bucket, else the least recently used one (stored or hit by the oldest call); never one stored or hit by the call itself.
 * Returns SRN_EINVAL (rows == 0, a shard), SRN_ERANGE (max_len outside 1..8, the limits of srn_predict's arguments), SRN_ENODEV (no device), SRN_ENOMEM, and SRN_ESTATE
 * when a cache is already enabled.  srn_index_result_cache_disable frees it (SRN_OK without one); _clear empties it; srn_index_set_attributes clears it (rows under the
 * business rules depend on the flags); srn_index_free disables it.  _clear and _stats without a cache: SRN_ESTATE.
 * srn_index_result_cache_stats waits for the cache's kernels enqueued so far.  lookups / hits / inserts / evictions are counted on the device since enable: cacheable
 * queries looked up (one per group of equal queries where the call merges them) | of those, served from the cache | rows stored | of those, over a live entry. */
typedef struct srn_result_cache_stats {
    uint64_t rows, ways, bytes;                       /* entries, entries per bucket, device bytes */
    uint32_t max_len, k, m, how_many, flags, reserved;
    uint64_t lookups, hits, inserts, evictions;
    uint64_t bypassed_calls, clears;                  /* calls on the index that did not use the cache | srn_index_result_cache_clear + srn_index_set_attributes */
} srn_result_cache_stats_t;
int srn_index_result_cache_enable(srn_index_t* idx, size_t rows, size_t max_len, size_t k, size_t m, size_t how_many, unsigned flags);
int srn_index_result_cache_disable(srn_index_t* idx);
int srn_index_result_cache_clear(srn_index_t* idx);
int srn_index_result_cache_stats(const srn_index_t* idx, srn_result_cache_stats_t* out);

/* srn_predict is re-entrant on one handle from any number of host threads, like predict() on the Arc<VMISIndex> the actix workers
 * share (src/bin/serving.rs:62-94).  Concurrent calls with the same (k, m, how_many, business flag) COMBINE into rounds: one batch
 * launch serves every call that arrived while the previous rounds ran (a lone caller runs alone, at once; environment
 * SRN_PREDICT_LANES = rounds in flight side by side, default 4, 0 = never combine).  Counters since the handle was created: */
int srn_predict_stats(const srn_index_t* idx, uint64_t* out_rounds, uint64_t* out_requests, uint64_t* out_max_round);

/* nq sessions in CSR form: session q = items_flat[q_off[q] .. q_off[q+1]).  Host pointers.
 * out_ids / out_scores are [nq * how_many] (row q at q * how_many), out_counts [nq].
 * Up to 256 sessions take the zero-copy latency path (pinned, device-mapped staging, no copies: ONE launch for calls of <= 48 sessions -- a workgroup per session writes
 * its query's record, serves it and finishes its row; the fast kernel's launch sequence for larger calls with a session of > 8 items; prep + general kernel -- two
 * launches -- otherwise); larger batches are cut into
 * chunks whose uploads, kernels and downloads overlap on separate streams, the results landing in the caller's buffers while
 * the next chunks run (srn_hostpipe.hip).  The buffers may be pageable. */
int srn_predict_batch(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq,
                      size_t k, size_t m, size_t how_many, unsigned flags, uint64_t* out_ids,
                      double* out_scores, uint32_t* out_counts);

/* Same with every buffer already resident in the index's device memory, enqueued on `stream`
 * (a hipStream_t; NULL = the null stream) without host synchronisation.  max_len_hint must be
 * >= the longest session in the batch (<= SRN_MAX_SESSION_LEN).  Calls from several host threads on the SAME stream take turns inside the library (each call's
 * launches stay contiguous in the stream: they share the workspace bound to it); different streams run side by side.  A query the kernel cannot serve
 * (empty or over-long session) gets out_counts[q] = 0xFFFFFFFF.  flags: SRN_FLAG_BUSINESS_LOGIC, SRN_FLAG_INPUTS_RESIDENT
 * (the prep kernel of this call then runs beside the previous call's kernels; for back-to-back full batches that was measured as a LOSS -- the prep kernel's
 * 0.44 ms per 2^20 queries disappear but the concurrent random look-ups slow vmis_fast_kernel by 0.7 ms -- it pays where the previous call leaves the GPU idle). */
int srn_predict_batch_device(const srn_index_t* idx, const uint64_t* d_items_flat, const uint32_t* d_q_off,
                             size_t nq, size_t max_len_hint, size_t k, size_t m, size_t how_many,
                             unsigned flags, uint64_t* d_out_ids, double* d_out_scores,
                             uint32_t* d_out_counts, void* stream);

/* ---- exclusion lists -------------------------------------------------------------------------------------------------------------------
 * predict removes ONE item from a row: the session's most recent one (mod.rs:156-160).  srn_predict_batch_device_excl also removes, per query, a caller-given list of ids
 * ("already in the basket", "already on the page") and, with SRN_FLAG_EXCLUDE_SESSION, every item of the query's own session -- and still returns how_many entries where
 * the candidates allow: the rows are those of "remove the ids from ALL candidates, then cut to how_many", bit for bit.  The launch sequence runs unchanged at the INTERNAL
 *     how_many + max_excl + (SRN_FLAG_EXCLUDE_SESSION ? max_len_hint - 1 : 0)        (above SRN_MAX_HOW_MANY: SRN_ERANGE)
 * into wide rows, and one kernel (srn_exclude.hip) drops the listed ids and compacts each row.  The wide rows are scratch of the workspace bound to `stream`:
 * 16 * nq * internal how_many + 4 * nq bytes, grown on first use and kept (2^20 queries, how_many 21, max_excl 16: 620 MB); equal-shaped calls allocate nothing.
 *   d_excl_flat / d_excl_off   the lists as a CSR of u64 ids and nq + 1 u32 offsets; NULL with max_excl = 0 (NULL with max_excl > 0: SRN_EINVAL)
 *   max_excl                   the capacity of one list -- an argument, not read from the data, so that the call never waits for the device.  A query whose list is longer
 *                              gets out_counts[q] = 0xFFFFFFFF, like a query with an empty or over-long session.  Duplicates in a list count toward max_excl and are
 *                              otherwise harmless, as are ids the index does not know.
 * Enqueued on `stream` without host synchronisation, like srn_predict_batch_device; SRN_FLAG_BUSINESS_LOGIC and SRN_FLAG_INPUTS_RESIDENT as there.  With max_excl = 0 and
 * no SRN_FLAG_EXCLUDE_SESSION the call IS srn_predict_batch_device: no scratch, no extra kernel.  Item shards and postings-only views are refused, as for predict.
 * The internal how_many is what the launch sequence sees: it stays on the fast kernels up to SRN_FAST_HOW_MANY_MAX (64), and an enabled result cache is used exactly when
 * its parameters equal the INTERNAL ones -- a server that excludes up to E ids enables it with how_many + E -- and is bypassed (and counted so) otherwise.  Cached and
 * merged rows are the wide, unfiltered ones; the filter runs per query behind them: two equal sessions with different lists get different rows.
 * srn_predict_batch_excl: the same with host pointers (pageable allowed) -- upload, the device form, download; it blocks.  A convenience form: the chunked host pipeline and
 * the latency path of srn_predict_batch are NOT extended to it; a serving host uses the device form. */
#define SRN_FLAG_EXCLUDE_SESSION 4u /* srn_predict_batch*_excl: every item of the query's own session is excluded, not only the most recent one */
int srn_predict_batch_device_excl(const srn_index_t* idx, const uint64_t* d_items_flat, const uint32_t* d_q_off, size_t nq, size_t max_len_hint,
                                  const uint64_t* d_excl_flat, const uint32_t* d_excl_off, size_t max_excl, size_t k, size_t m, size_t how_many, unsigned flags,
                                  uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts, void* stream);
int srn_predict_batch_excl(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, const uint64_t* excl_flat, const uint32_t* excl_off, size_t max_excl,
                           size_t k, size_t m, size_t how_many, unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts);

/* ---- short rows filled from a fallback ranking -------------------------------------------------------------------------------------------
 * A row is short (count < how_many) whenever the neighbours do not yield enough candidates, and empty whenever the clicked item is unknown to the index -- every product
 * listed since the index was built.  An index may carry a FALLBACK RANKING: up to SRN_MAX_FALLBACK distinct public item ids, best first; ids the index does not know are
 * allowed (a list of new products is a legitimate ranking).  With SRN_FLAG_FILL a batch call appends, on the device, on the caller's stream and in place, to every row of
 * c < how_many entries the first how_many - c entries f of the ranking, in ranking order, that
 *   - are none of the row's c ids and not the session's most recent item r,
 *   - are in nothing the call removes from the model's candidates: the query's exclusion list, with SRN_FLAG_EXCLUDE_SESSION every item of the session, with
 *     SRN_FLAG_EXCLUDE_SEEN the request's window,
 *   - and, with SRN_FLAG_BUSINESS_LOGIC, pass passes_business_rules(attr(r), attr(f)) (mod.rs:162-182): f needs attributes (an id unknown to the index is dropped) and must
 *     be for sale; an adult f passes only when r has attributes and is adult.  The attributes are read at call time: a later srn_index_set_attributes is honoured.
 * The c model entries are untouched; filled entries carry the score -infinity (model scores are finite, but zero and negative ones exist: no finite value can say "no model
 * score", and -inf keeps the row score-descending); out_counts[q] = c + filled.  A row with c >= how_many is not touched, a count of 0xFFFFFFFF stays, and where the
 * ranking runs out the row stays short.  Without the flag every call enqueues the same kernels and writes the same bytes as before, ranking or not.
 * SRN_FLAG_FILL is accepted by srn_predict_batch_device_excl, srn_predict_batch_excl, srn_recommend_batch_device, srn_recommend_batch and srn_eval_trial_t.flags; with the
 * flag and no ranking they fail with SRN_ESTATE before anything is enqueued.  srn_predict_batch_device_excl with max_excl = 0, no SRN_FLAG_EXCLUDE_SESSION and
 * SRN_FLAG_FILL is srn_predict_batch_device plus the fill kernel on the caller's buffers: no scratch.  Merged rows and the result cache's rows stay the unfilled ones (the
 * fill runs per query behind them, like the exclusion filter); the cache's parameters and statistics are unaffected, and a new ranking does not clear it.
 *   srn_index_set_fallback          replaces an earlier ranking.  n == 0 or an id that occurs twice: SRN_EINVAL; n > SRN_MAX_FALLBACK: SRN_ERANGE.
 *   srn_index_set_fallback_popular  the first min(n, n_items) items of the index's popularity order: count of kept sessions that hold the item descending, id ascending.
 *   srn_index_fallback              *out_n = the ranking's length (0: none); up to cap ids into out (may be NULL).
 *   srn_index_clear_fallback        no ranking (SRN_OK without one).
 * Item shards and postings-only views are refused, as for predict.  Setting a ranking allocates device memory and waits for the device: set it before serving.  The
 * concurrency rule is that of srn_index_set_attributes, which overwrites the item records with a blocking copy that no stream orders against a kernel in flight: the
 * caller makes sure that NO call on the index is running or enqueued-and-unfinished while the ranking (or the attributes) change -- a call that overlaps one may see the
 * old entries, the new ones, or some of each.  srn_index_free releases the ranking; srn_index_save / srn_index_load do not carry it (the file format is unchanged): set
 * it again after a load. */
#define SRN_FLAG_FILL 16u
#define SRN_MAX_FALLBACK 4096
int srn_index_set_fallback(srn_index_t* idx, const uint64_t* item_ids, size_t n);
int srn_index_set_fallback_popular(srn_index_t* idx, size_t n);
int srn_index_fallback(const srn_index_t* idx, uint64_t* out, size_t cap, size_t* out_n);
int srn_index_clear_fallback(srn_index_t* idx);

/* Debug / measurement variant of srn_predict_batch (host pointers; any of the three extra outputs
 * may be NULL):
 *   out_stats  [nq * 8]  P, C, K, I, D, H, L, status per query -- the per-query terms of the
 *                        algorithmic-bytes formula
 *   out_nb_sessions / out_nb_num [nq * k], out_nb_counts [nq]: the selected neighbour sessions
 *                        (reference session indices, unordered) and their integer similarity
 *                        numerators (similarity = num / distinct evolving items). */
int srn_predict_batch_debug(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq,
                            size_t k, size_t m, size_t how_many, unsigned flags, uint64_t* out_ids,
                            double* out_scores, uint32_t* out_counts, uint32_t* out_stats,
                            uint32_t* out_nb_sessions, uint32_t* out_nb_num, uint32_t* out_nb_counts);

/* Sizes the per-stream workspace of srn_predict_batch_device for calls of up to nq queries with these parameters: after it, such
 * calls on `stream` allocate nothing (hipMalloc / hipFree synchronise the device, so a serving process reserves once at start-up).
 * Without it the workspace grows on demand, the first time a larger batch arrives. */
int srn_index_reserve(const srn_index_t* idx, size_t nq, size_t max_len_hint, size_t k, size_t m, size_t how_many, unsigned flags, void* stream);

/* Kernel timing on (enable != 0) or off, per index; off by default (SRN_TIMING=1 in the environment: on from the start).  When on, every batch call records HIP
 * events between its kernels, which srn_last_kernel_ms / srn_kernel_times* read back; each event idles the launch stream for ~6 us (three per call: 18 us of the
 * 250 us a 4 096-query batch takes), so a serving process leaves it off and a benchmark switches it on around the region it reports kernel times for. */
int srn_kernel_timing(srn_index_t* idx, int enable);

/* Average duration in milliseconds of the predict kernel launches enqueued by the most recent
 * srn_predict_batch* call on this thread, measured with HIP events on the launch stream (blocks
 * until that work has finished); *out_launches = number of kernel launches it covered.  SRN_EINVAL if kernel timing
 * was off for that call (srn_kernel_timing). */
int srn_last_kernel_ms(const srn_index_t* idx, double* out_ms_main, double* out_ms_retry, uint32_t* out_retried);

/* ---- item-sharded index: one shard per GPU ---------------------------------------------------
 * For indices that outgrow one GPU (BASELINE config 5), and for the north star's multi-GPU mode, the index is split by item: shard g holds postings, row
 * fragments and idf of the items with owner(id) == g (a fixed hash of the public id), while session recency ranks stay global.  A shard answers no predict
 * call by itself: a SHARD GROUP (below) drives the shards of all ranks through one batch call.  Results are bit-identical to the unsharded path
 * (tests/test_gpu_shard_group.py, tests/test_gpu_sharded.py).
 * Shard `shard` of n_shards is cut out of an UNSHARDED index -- built by srn_index_build_gpu or read by srn_index_load; the same bytes
 * srn_index_build_shard builds from the sessions, in one O(nnz) pass (an item-sharded deployment builds or loads ONE index and
 * every rank cuts its own shard out of it; the reference loads its production index: src/vmisknn/vmis_index.rs:85-314).
 * srn_index_build_shard_gpu = srn_index_build_gpu + srn_index_shard without ever attaching the full index to the device;
 * srn_index_load_shard reads a saved index (unsharded: cut; already that shard: as is). */
int srn_index_build_shard(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len,
                          double idf_weighting, uint32_t shard, uint32_t n_shards, int device, srn_index_t** out);
int srn_index_shard(const srn_index_t* full, uint32_t shard, uint32_t n_shards, int device, srn_index_t** out);
int srn_index_build_shard_gpu(const srn_sessions_view_t* sessions, size_t m_index, size_t max_session_len, double idf_weighting,
                              uint32_t shard, uint32_t n_shards, int device, srn_index_t** out);
int srn_index_load_shard(const char* path, uint32_t shard, uint32_t n_shards, int device, srn_index_t** out);

/* ---- the shard group: the whole item-sharded batch in ONE call, collectives inside (srn_group.hip) ---------------------------------------
 * What a reference-side host (serving / evaluator, src/endpoints/recommend_resource.rs:56, src/bin/evaluator.rs:58) calls to drive an index
 * sharded over the GPUs of a node: one process (or thread group) per GPU creates its rank of the group around its shard, then every rank calls
 * srn_shard_group_predict_batch with the SAME batch; the call runs the LISTS pipeline -- head kernel, all-reduce(max) of the cuts, count kernel, all-gather of the
 * counts, variable-length exchange of the kept list prefixes, the unsharded kernels over the rank's row fragments, all-gather of the per-shard
 * top-n, merge by (score desc, id asc) -- with RCCL called from inside the library.  Results (identical on every rank, bit-identical to the
 * unsharded index) are written to the caller's device buffers, asynchronously on `stream`; the call itself blocks the host for one short
 * synchronisation on the group's own exchange stream (the per-shard list totals size the exchange).  With SRN_FLAG_INPUTS_RESIDENT a batch's
 * exchange phase overlaps the previous batch's kernels.  Batches the lists pipeline does not serve (sessions of > 8 items,
 * m > m_index, incomplete posting lists) take the three-stage pipeline inside the same call: stage A -> all-gather of the candidates -> stage B ->
 * all-reduce(min) of the first-match positions -> stage C -> all-gather of the per-shard top-n -> merge (no host synchronisation at all).
 *
 *   rank 0:   srn_shard_group_unique_id(id, sizeof id)      -- 256 opaque bytes; hand them to the other ranks (your own control plane)
 *   rank r:   srn_index_load_shard(path, r, world, device_r, &shard);  srn_shard_group_create(shard, id, r, world, &group)
 *   per batch, every rank:   srn_shard_group_predict_batch(group, d_items, d_q_off, nq, ...)
 */
#define SRN_SHARD_GROUP_ID_BYTES 256
#define SRN_FLAG_INPUTS_RESIDENT 2u /* srn_shard_group_predict_batch, srn_predict_batch_device: d_items_flat / d_q_off are complete in device memory at call time (not pending on `stream`):
                                     * the call's first small kernels may then run on a stream of the library's own, beside the previous call's kernels */
typedef struct srn_shard_group srn_shard_group_t;
int srn_shard_group_unique_id(void* out, size_t bytes);
int srn_shard_group_create(const srn_index_t* shard, const void* unique_id, int rank, int world, srn_shard_group_t** out);
/* The same group over the APPLICATION's transport instead of RCCL (MPI, sockets, a test harness): three collectives on device buffers.  Each
 * callback must order itself after the work already enqueued on `stream` and complete (or be enqueued on `stream`) before it returns;
 * channel 0 / 1 = the group's two independent sequences of collectives (exchange stream / caller's stream).  Non-zero return = failure.
 *   all_reduce_max_i32 / all_reduce_min_i32(user, channel, d_buf, count, stream)   element-wise maximum / minimum over the ranks, in place
 *   all_gather(user, channel, d_buf, block_bytes, stream)                   d_buf = world blocks; block `rank` holds this rank's data
 *   all_gather_v(user, channel, d_buf, byte_off[world], byte_cnt[world], stream)    segment r = d_buf[byte_off[r] .. + byte_cnt[r]); this rank's is in place */
typedef struct {
    void* user;
    int (*all_reduce_max_i32)(void* user, int channel, int32_t* d_buf, size_t count, void* stream);
    int (*all_gather)(void* user, int channel, void* d_buf, size_t block_bytes, void* stream);
    int (*all_gather_v)(void* user, int channel, void* d_buf, const uint64_t* byte_off, const uint64_t* byte_cnt, void* stream);
    int (*all_reduce_min_i32)(void* user, int channel, int32_t* d_buf, size_t count, void* stream);   /* may be NULL: the group then serves the lists pipeline only */
} srn_shard_comm_t;
int srn_shard_group_create_with_comm(const srn_index_t* shard, int rank, int world, const srn_shard_comm_t* comm, srn_shard_group_t** out);
/* All shards of the group in THIS process on one device (tests; capacity experiments on one GPU): the collectives degenerate to kernels. */
int srn_shard_group_create_local(const srn_index_t* const* shards, int n_shards, srn_shard_group_t** out);
/* Threads and streams: calls on one group are serialised inside (a mutex for the enqueue; a buffer slot is reused only behind the batch that used it, whatever stream
 * that batch ran on).  Over a multi-rank transport every rank must issue the group's batches in the SAME order, and a rank that alternates between streams must
 * order them itself: collectives on one communicator execute in issue order on every rank.  One stream per group is the simple way. */
int srn_shard_group_predict_batch(srn_shard_group_t* g, const uint64_t* d_items_flat, const uint32_t* d_q_off, size_t nq, size_t max_len_hint,
                                  size_t k, size_t m, size_t how_many, unsigned flags, uint64_t* d_out_ids, double* d_out_scores,
                                  uint32_t* d_out_counts, void* stream);
typedef struct {
    uint64_t n_shards, batches, queries;
    uint64_t bytes_head, bytes_counts, bytes_lists, bytes_results; /* what THIS rank contributed to each exchange, summed over the batches */
    uint64_t bytes_lists_max_rank;                                 /* the fullest rank's list segment, summed over the batches (what a padded all-gather would ship per rank) */
    uint32_t transport;                                            /* 0 in-process, 1 RCCL, 2 application callbacks */
    uint32_t overlapped;                                           /* the exchange phase runs on the group's own stream */
    uint64_t stage_batches, bytes_stage_candidates, bytes_stage_minpos; /* batches that took the three-stage pipeline, and what this rank contributed to its two big exchanges */
    uint64_t neighbour_batches, bytes_neighbours;                      /* batches that took the neighbours pipeline, and the neighbour-list block this rank contributed to its all-gather */
} srn_shard_group_stats_t;
int srn_shard_group_stats(const srn_shard_group_t* g, srn_shard_group_stats_t* out);
/* Overlap of batch i + 1's exchange (the group's own stream and first communicator) with batch i's kernels and result gather (caller's stream, second communicator).
 * on = 0: everything in issue order on the caller's stream, one collective of the group in flight at a time -- the conservative form (two communicators with collectives in
 * flight at once need both collective kernels to become resident on every rank; they do here -- the predict kernels are finite -- but a host that wants no such
 * dependence leaves it off).  Default OFF since round 5 -- the overlapped form has never run on more than one GPU; a host opts in (or SRN_GROUP_OVERLAP=1 in the environment);
 * takes effect from the next batch; every rank must use the same setting for the same batch. */
int srn_shard_group_set_overlap(srn_shard_group_t* g, int on);
/* Failure of a batch.  A srn_shard_group_predict_batch that fails after its first collective was handed to the transport (or for a reason its peers do not share: a HIP
 * error, an allocation) leaves the peers' collectives of that batch without their partner.  The group is then BROKEN on this rank: its RCCL communicators are aborted at
 * once (nothing of this rank keeps a peer's GPU waiting), and every further call on it fails with SRN_ESTATE.  The peers learn of it from their own transport (a callback
 * that returns non-zero breaks their group the same way) or from srn_shard_group_wait: a bounded wait for the group's most recent batch -- SRN_OK when its results are
 * complete, SRN_ETIMEOUT after timeout_ms, which also breaks the group (a collective whose partner died never ends; a plain stream synchronise would hang with it).
 * A broken group is freed without waiting for the device.  Refusals every rank makes alike before anything is issued (SRN_EINVAL / SRN_ERANGE) leave the group usable. */
int srn_shard_group_wait(srn_shard_group_t* g, uint64_t timeout_ms);
/* The NEIGHBOURS pipeline (round 4; SURVEY 8(e)'s replicated-postings variant, with the candidate work divided over the ranks).  The posting lists are the pruned structure
 * (<= m_index entries per item: config 3 111 MB, config 5 ~9 GB) -- every rank keeps ALL of them beside its shard of the rows: `postings` = the unsharded index itself, or
 * its rows-free view (srn_index_postings_view: dictionary, idf / attributes, lists), on the group's device.  Per batch, rank r then runs find_neighbors
 * (vmis_index.rs:325-415: lists, merge, m-cut, k-cut) for the queries [r nq / G, (r + 1) nq / G) ONLY, one all-gather ships the neighbour lists ((k + 1) * 4 bytes per
 * query, fixed-size blocks: no host synchronisation), and every rank scores ALL queries over its own row fragments (mod.rs:126-214) before the usual all-gather of the
 * per-shard top-n and the merge.  Same integers as the unsharded index on every rank: bit-identical results.  Serves what the lists pipeline serves and the fast kernel's
 * shape (k <= 1536, m <= 2560, how_many <= 24, no debug outputs); other batches take the lists / three-stage pipelines as before.  postings = NULL switches it off.
 * Every rank must make the same call; the handle must outlive the group. */
int srn_shard_group_set_postings(srn_shard_group_t* g, const srn_index_t* postings);
int srn_index_postings_view(const srn_index_t* full, int device, srn_index_t** out);
void srn_shard_group_free(srn_shard_group_t* g);

/* The same for the most recent min(max_n, 64) predict calls (oldest first): per-call duration in ms of
 * the main kernel and of the retry pass, from HIP events recorded on the launch stream around each
 * launch.  This is what bench.py reports as the kernel's live-measured launch duration.  Only the trailing run of calls
 * made with kernel timing on (srn_kernel_timing) is reported: *out_n = 0 if the last call was not timed. */
int srn_kernel_times(const srn_index_t* idx, uint32_t max_n, double* out_ms_main, double* out_ms_retry, uint32_t* out_n);

/* The same with the launches of a call told apart: prep kernel | fast kernel alone (vmis_fast_kernel, the dominant kernel;
 * 0 when the call was not eligible for it) | all predict launches (fast kernel + general kernel over the handed-over
 * queries + finish kernel: == out_ms_main of srn_kernel_times) | global-table retry pass.  Any output may be null. */
int srn_kernel_times_detail(const srn_index_t* idx, uint32_t max_n, double* out_ms_prep, double* out_ms_fast, double* out_ms_predict,
                            double* out_ms_retry, uint32_t* out_n);


/* How the queries of the most recent predict call on this handle were served: *out_nq queries in all, *out_general of them by
 * the general kernel (the fast kernel hands over what does not fit its query shape; == nq when the launch was not eligible for
 * the fast kernel at all), *out_global_pass through the global-table retry pass.  Waits for that call to finish. */
int srn_last_path_counts(const srn_index_t* idx, uint32_t* out_nq, uint32_t* out_general, uint32_t* out_global_pass);


/* ---- misc ------------------------------------------------------------------------------- */
/* ---- dynamic batching: the serving-side caller ------------------------------------------------------------------
 * The reference answers every /v1/recommend call with its own vmisknn::predict on an actix worker
 * (src/endpoints/recommend_resource.rs:56-62; workers share one Arc<VMISIndex>, src/bin/serving.rs:62-94).
 * srn_batcher_predict has predict()'s shape -- one evolving session in, <= how_many (id, score) pairs out, blocking --
 * and may be called from any number of threads; a dispatcher thread folds what is waiting (up to max_batch requests, or
 * whatever has arrived max_wait_us after the first one) into ONE srn_predict_batch launch.  k, m, how_many and the
 * business-logic switch are fixed per batcher, like the serving binary's configuration (src/config.rs). */
typedef struct srn_batcher srn_batcher_t;
int srn_batcher_create(const srn_index_t* idx, size_t max_batch, unsigned max_wait_us, size_t k, size_t m, size_t how_many,
                       int enable_business_logic, srn_batcher_t** out);
int srn_batcher_predict(srn_batcher_t* b, const uint64_t* evolving, size_t len, uint64_t* out_ids, double* out_scores, size_t* out_n);
int srn_batcher_stats(srn_batcher_t* b, uint64_t* n_requests, uint64_t* n_batches, uint64_t* max_batch_seen);
int srn_batcher_how_many(const srn_batcher_t* b, size_t* out);   /* the result capacity a caller's buffers need */
void srn_batcher_free(srn_batcher_t* b);   /* serves what is still queued, then stops the dispatcher */

/* ---- evolving-session store + the /v1/recommend handler body --------------------------------------------------------
 * Replaces RocksDBSessionStore (src/sessions/mod.rs:7-77) and the body of v1_recommend
 * (src/endpoints/recommend_resource.rs:20-65) between the web framework and predict.  The store is in memory (a visitor
 * is pinned to one pod by session_id affinity).  This host store does not survive the process; the device-resident store below can
 * be saved to a file and loaded again (srn_device_sessions_save / _load), as the reference's RocksDB survives a restart.  Keys are the reference's: the MD5
 * digest of the session_id string read as a big-endian u128 (recommend_resource.rs:27-28), here as (hi, lo).
 * A session idle for more than idle_secs reads as empty (mod.rs:46-52; 0 = the reference's 20 minutes); entries older than
 * ttl_secs are dropped (RocksDB TTL, src/bin/serving.rs:55-56; 0 = the reference's 30 minutes).  now_secs = 0 means the
 * system clock (seconds since the epoch, mod.rs:74-76); tests pass explicit times. */
typedef struct srn_session_store srn_session_store_t;
int srn_session_key(const char* session_id, size_t len, uint64_t* key_hi, uint64_t* key_lo);
int srn_session_store_create(uint64_t ttl_secs, uint64_t idle_secs, srn_session_store_t** out);
void srn_session_store_free(srn_session_store_t* s);
/* get_session_items (mod.rs:37-57): unknown or idle session -> *out_n = 0 */
int srn_session_store_get(srn_session_store_t* s, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs,
                          uint64_t* out_items, size_t cap, size_t* out_n);
/* update_session_items (mod.rs:59-72) */
int srn_session_store_update(srn_session_store_t* s, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs,
                             const uint64_t* items, size_t n);
/* drops every entry older than ttl_secs now (also done incrementally by updates); *n_live = entries kept */
int srn_session_store_sweep(srn_session_store_t* s, uint64_t now_secs, uint64_t* n_live);
/* v1_recommend's body: with user_consent, session := stored items; append item_id unless it repeats the last one; drop the
 * oldest beyond max_items_in_session; store; without consent the session is [item_id] and the store is untouched.  Then
 * predict through the batcher.  out_ids (and out_scores, may be NULL: the endpoint returns ids only) hold how_many entries. */
int srn_recommend(srn_batcher_t* b, srn_session_store_t* s, const char* session_id, size_t session_id_len, uint64_t item_id,
                  int user_consent, size_t max_items_in_session, uint64_t now_secs, uint64_t* out_ids, double* out_scores,
                  size_t* out_n);

/* ---- device-resident session store + /v1/recommend for a whole batch ----------------------------------------------------
 * The same handler body with the evolving sessions in HBM (srn_sessions_dev.hip): one call takes n (session key, clicked item, consent) triples, applies the update
 * rule above to the store and predicts every request's session, through the launch sequence of srn_predict_batch_device, with no host round trip in between.
 * The result -- rows AND store -- is what n calls of srn_recommend in request order with the same now_secs and max_items_in_session give: a request sees the session as
 * the earlier requests of its key in the batch left it (any multiplicity; keys compared by all 128 bits); without consent the session is [item] and the store is not
 * touched, not even its clock.  A stored session longer than a since-lowered max_items_in_session stays that long (one item is dropped per append), as in the reference.
 *   capacity   live sessions the table holds: a power-of-two open-addressing table of >= 2 * capacity slots, allocated (twice: a sweep rebuilds into the other half,
 *              there are no tombstones) at creation.  The host keeps an upper bound of the occupied slots (+ n per call); a call that would pass `capacity` by that bound
 *              waits for the device, takes the exact count and, if that is what makes room, drops the entries older than ttl_secs; if live sessions + n still exceed
 *              capacity it fails with SRN_ENOMEM and the store is as it was.  Size capacity >= peak live sessions + largest batch; the normal path reads nothing back.
 *   items_cap  items a stored session may have (1..SRN_MAX_SESSION_LEN); max_items_in_session above it: SRN_ERANGE.  A slot is 32 + 8 * items_cap bytes rounded up to 128.
 *   ttl_secs / idle_secs: as srn_session_store_create (0 = 30 / 20 minutes); ttl_secs < idle_secs: SRN_EINVAL (TTL governs reclamation only).
 * Calls on one store from several threads or streams are serialised by the library (a mutex for the enqueue, an event between consecutive calls); different stores run
 * side by side.  Errors are raised before anything is changed: max_items_in_session 0 SRN_EINVAL; predict's own checks as ever; a store on another device than the index
 * SRN_EINVAL; n = 0 SRN_OK. */
typedef struct srn_device_sessions srn_device_sessions_t;
typedef struct {
    uint64_t capacity, slots, items_cap, slot_bytes;
    uint64_t live_bound;        /* the host's upper bound of the occupied slots */
    uint64_t sweeps, refused;   /* rebuilds that dropped expired entries (explicit or automatic) | calls refused with SRN_ENOMEM for capacity */
    uint64_t ttl_secs, idle_secs;
    uint64_t max_stored_len;    /* upper bound of the stored session lengths = the max_len_hint predict is called with */
} srn_device_sessions_stats_t;
int srn_device_sessions_create(int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions_t** out);
void srn_device_sessions_free(srn_device_sessions_t* s);
/* srn_session_store_get / _update / _sweep for the device store, from the host (tests, debugging; one key per call -- whole stores move with srn_device_sessions_export / _import below): they block.
 * update: n above items_cap is SRN_ERANGE.  sweep: *n_live = entries kept. */
int srn_device_sessions_get(srn_device_sessions_t* s, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs, uint64_t* out_items, size_t cap, size_t* out_n);
int srn_device_sessions_update(srn_device_sessions_t* s, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs, const uint64_t* items, size_t n);
int srn_device_sessions_sweep(srn_device_sessions_t* s, uint64_t now_secs, uint64_t* n_live);
int srn_device_sessions_stats(srn_device_sessions_t* s, srn_device_sessions_stats_t* out);
/* The store remembers more than it predicts on.  history = 0 (the default): the store keeps max_items_in_session items, as the reference does -- nothing
 * changes.  history = H in 1..items_cap (above: SRN_ERANGE): a srn_recommend_batch* call on this store keeps a window of the last H clicks -- the same append rule, idle
 * rule and one-item-dropped-per-append rule, with H in the limit's place -- and predicts on the LAST min(window, max_items_in_session) items of it; it needs
 * max_items_in_session <= H (else SRN_ERANGE, before anything changes).  The rows are those of a plain store driven with the same constant max_items_in_session.
 * srn_device_sessions_get / _export / _save see the whole window; the file format does not change and H, a runtime setting, is not saved: a store that was filled with a
 * history window should be given its H again after srn_device_sessions_load (until then the next call would cut the windows to max_items_in_session, an item per append). */
int srn_device_sessions_set_history(srn_device_sessions_t* s, size_t history);
int srn_device_sessions_history(srn_device_sessions_t* s, size_t* out_history);
/* HIP events around the store's kernels and predict's launches of every batch (off by default); last_ms blocks until the most recent batch is done */
int srn_device_sessions_timing(srn_device_sessions_t* s, int enable);
int srn_device_sessions_last_ms(srn_device_sessions_t* s, double* out_ms_store, double* out_ms_predict);
/* ---- snapshot, restore, merge and grow the device store (bulk, on the device) ----
 * Every call takes the store's mutex and is ordered behind the store's previous call, like the calls above.  now_secs = 0: the system clock.
 * The LIVE entries at now_secs are those a sweep at now_secs keeps: occupied and not older than ttl_secs.  The idle rule is a read rule: an entry that is idle but
 * younger than the TTL is live and is exported with its epoch.  now_secs = 1 therefore means "everything". */
/* exact counts, from the device: *occupied slots and *live entries (either may be NULL); blocks */
int srn_device_sessions_count(srn_device_sessions_t* s, uint64_t now_secs, uint64_t* occupied, uint64_t* live);
/* The live entries as dense arrays, in ascending slot order (two exports of an unchanged store give identical bytes):
 *   key_hi[i] | key_lo[i] | epoch[i] (seconds, as stored) | len[i] | items[i * items_stride .. + len[i]), the rest of the row zero
 * items_stride below the store's max_stored_len (srn_device_sessions_stats): SRN_ERANGE.  An empty store and cap = 0 (the arrays may then be NULL) are SRN_OK.
 * _export_device: device buffers on the store's GPU, enqueued on `stream` with no host synchronisation; writes the first min(live, cap) entries and *d_n = live --
 *                 the caller compares.  NULL store or d_n: SRN_EINVAL.
 * _export:        host arrays; blocks.  live > cap: SRN_ERANGE with *n = live and the arrays untouched.  NULL store or n: SRN_EINVAL. */
int srn_device_sessions_export_device(srn_device_sessions_t* s, uint64_t now_secs, size_t cap, uint64_t* d_key_hi, uint64_t* d_key_lo, uint64_t* d_epoch, uint32_t* d_len,
                                      uint64_t* d_items, size_t items_stride, uint64_t* d_n, void* stream);
int srn_device_sessions_export(srn_device_sessions_t* s, uint64_t now_secs, size_t cap, uint64_t* key_hi, uint64_t* key_lo, uint64_t* epoch, uint32_t* len, uint64_t* items,
                               size_t items_stride, size_t* n);
/* Inserts n entries in the arrays' form above, each with its own epoch.  The merge rule: among entries with the same 128-bit key in one call the largest epoch wins
 * (ties: the later index); an entry whose key is stored replaces it iff its epoch is >= the stored one; any other key is inserted.  Both forms block (the checks read
 * a device reduction back) and nothing is changed unless every check passes: a len[i] above the store's items_cap or above items_stride is SRN_ERANGE; the capacity
 * rule of a batch applies with every entry counted as a new key and nothing reclaimed (occupied + n > capacity: SRN_ENOMEM, or growth).  n = 0: SRN_OK. */
int srn_device_sessions_import_device(srn_device_sessions_t* s, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_epoch, const uint32_t* d_len,
                                      const uint64_t* d_items, size_t items_stride, size_t n, void* stream);
int srn_device_sessions_import(srn_device_sessions_t* s, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* epoch, const uint32_t* len, const uint64_t* items,
                               size_t items_stride, size_t n);
/* Rebuilds the live entries at now_secs into tables of another capacity and / or items_cap (0 = keep); what a sweep at now_secs drops is dropped.  More live entries
 * than capacity: SRN_ENOMEM; a live session longer than items_cap (the exact maximum, counted on the device): SRN_ERANGE; no device memory: SRN_ENOMEM -- the
 * store is unchanged and usable in every case.  Both new tables are allocated before the old ones are freed: peak device memory is the old pair + the new pair.  Blocks. */
int srn_device_sessions_resize(srn_device_sessions_t* s, size_t capacity, size_t items_cap, uint64_t now_secs);
/* Opt-in growth.  max_capacity 0 (the default): off.  Otherwise a call that the capacity rule would refuse after its exact count resizes the store to the smallest
 * capacity * 2^j that holds live sessions + n, if that is <= max_capacity, and goes on; beyond it the call is refused with SRN_ENOMEM and counted as ever. */
int srn_device_sessions_set_max_capacity(srn_device_sessions_t* s, size_t max_capacity);
/* *grows: automatic resizes; *resizes: all successful resizes, explicit and automatic (any pointer may be NULL) */
int srn_device_sessions_growth(srn_device_sessions_t* s, uint64_t* max_capacity, uint64_t* grows, uint64_t* resizes);
/* The file form (little-endian; byte by byte in DESIGN.md section 11): a 96-byte header, then the export's arrays.  save writes the live entries at now_secs to a
 * temporary name next to `path` and renames it, so a crash leaves the previous snapshot.  load creates a store on `device` and imports the file: capacity 0 =
 * max(saved capacity, n), items_cap / ttl_secs / idle_secs 0 = the saved values; n above capacity SRN_ENOMEM, the longest session above items_cap SRN_ERANGE.
 * A file that is short, has another magic or version, sizes that do not add up, a length above its stride or a checksum mismatch is SRN_EIO (as srn_index_load).
 * file_info reads and verifies the whole file on the host; it needs no GPU. */
typedef struct {
    uint64_t version, n, longest_session, items_stride;
    uint64_t capacity, items_cap, ttl_secs, idle_secs;   /* of the store that was saved */
    uint64_t saved_at_secs, payload_bytes;
} srn_device_sessions_file_info_t;
int srn_device_sessions_save(srn_device_sessions_t* s, const char* path, uint64_t now_secs);
int srn_device_sessions_load(const char* path, int device, size_t capacity, size_t items_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_device_sessions_t** out);
int srn_device_sessions_file_info(const char* path, srn_device_sessions_file_info_t* out);
/* ---- trending items: what the live sessions hold, counted and ranked on the device (srn_trending.hip) ----
 * The items the live sessions hold most often.  An entry is IN RANGE when it is live at now_secs (occupied and not older than ttl_secs: what a sweep at now_secs keeps;
 * now_secs = 0 the system clock, 1 = everything, as for srn_device_sessions_export) and its epoch >= since_secs (0 = no lower bound).
 * count(id) = the number of in-range entries whose stored window items[0 .. len) contains id AT LEAST once (a window A,B,A counts A once; positions >= len are never read,
 * so the id 0 is an id like any other).  The ranking is count descending, id ascending; ids with count < min_count (0 is read as 1) are left out.
 * Writes the first min(cap, ranked) ids and counts (either array may be NULL) and *out_n = ranked, the number of ids with count >= min_count -- the caller compares.
 * Blocks; takes the store's mutex and is ordered behind the store's previous call like every other store call; changes nothing in the store.
 * Counts are exact integers and the order is total: two calls on an unchanged store return the same bytes.
 * NULL store or out_n: SRN_EINVAL; cap > 0 with both arrays NULL: SRN_EINVAL; an empty store or nothing in range: SRN_OK with *out_n = 0.
 * Scratch is sized from the exact number T of (entry, distinct id) pairs in range, allocated for the call and released: 12 bytes per slot, then 20 T bytes + 4 bytes per
 * distinct id + rocPRIM's temporaries -- a store of 4 M sessions of 16 items needs about 1.3 GB for a moment.  No device memory for it: SRN_ENOMEM, with the store
 * untouched and usable.  T above 2^31: SRN_ERANGE. */
int srn_device_sessions_top_items(srn_device_sessions_t* s, uint64_t now_secs, uint64_t since_secs, uint32_t min_count, size_t cap,
                                  uint64_t* out_ids, uint32_t* out_counts, size_t* out_n);
#define SRN_TRENDING_POPULAR_TAIL 1u
/* Sets the index's fallback ranking from a store's live sessions: the first n entries of srn_device_sessions_top_items(store, now_secs, since_secs,
 * min_count); with SRN_TRENDING_POPULAR_TAIL, when those are fewer than n, followed by the index's popularity order (srn_index_set_fallback_popular's) without the ids
 * already in the list, up to n in all.  *out_trending (may be NULL) = how many entries came from the store.  Ids the index does not know stay in the list.
 * NULL index or store: SRN_EINVAL; n == 0: SRN_EINVAL; n > SRN_MAX_FALLBACK: SRN_ERANGE; item shards and postings-only views refused as for srn_index_set_fallback; an
 * index without a device: SRN_ENODEV; store on another device than the index: SRN_EINVAL (checked in this order, before any device work).  A resulting list of 0 entries
 * leaves the ranking as it was (SRN_OK, *out_trending = 0).  The concurrency rule is srn_index_set_fallback's, unchanged: no call on the index may be in flight. */
int srn_index_set_fallback_trending(srn_index_t* idx, srn_device_sessions_t* store, uint64_t now_secs, uint64_t since_secs, uint32_t min_count, size_t n,
                                    unsigned flags, size_t* out_trending);
/* srn_session_key for n strings: string i = ids_flat[off[i] .. off[i + 1]) */
int srn_session_keys(const char* ids_flat, const uint64_t* off, size_t n, uint64_t* key_hi, uint64_t* key_lo);
/* flags: SRN_FLAG_BUSINESS_LOGIC, SRN_FLAG_FILL (short rows filled from the index's fallback ranking, above), and SRN_FLAG_EXCLUDE_SEEN -- a request's recommendations leave out what its visitor has seen: the request's window as the request
 * sees it (the store's history window, or the session window on a store without one), the earlier requests of its key in the batch included; without consent nothing beyond
 * the item itself.  The windows are the exclusion lists of srn_predict_batch_device_excl, their capacity the store's max_stored_len bound (srn_device_sessions_stats):
 * the launch sequence runs at the internal how_many + max_stored_len (above SRN_MAX_HOW_MANY: SRN_ERANGE, before anything changes), which is also what a result cache must
 * be enabled with to serve such calls. */
#define SRN_FLAG_EXCLUDE_SEEN 8u
/* Every buffer in the index's device memory; enqueued on `stream` (a hipStream_t) without host synchronisation.  d_consent: one byte per request, NULL = every request
 * consents.  out rows / counts as srn_predict_batch_device.  store may be NULL only if no request consents (d_consent == NULL with a NULL store: SRN_EINVAL; otherwise the
 * flags are read back and checked before anything is launched -- that call blocks).  now_secs = 0: the system clock, read once. */
int srn_recommend_batch_device(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids,
                               const uint8_t* d_consent, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m, size_t how_many,
                               unsigned flags, uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts, void* stream);
/* The same with host pointers (pageable allowed); the results are in the caller's buffers on return. */
int srn_recommend_batch(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids,
                        const uint8_t* consent, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m, size_t how_many,
                        unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts);
/* ---- the timed batch: every request its own clock ----
 * srn_recommend_batch_device / srn_recommend_batch with times[i], request i's clock in seconds, after the consent array.  A time is used as given: 0 is a time like any
 * other.  The call leaves the rows, the store and an attached harvest exactly as n one-request untimed calls would, call i with now_secs = times[i], in request order
 * i = 0 .. n-1 -- as long as the capacity rule's automatic sweep does not run.  Times need not be monotone: the rule is still "one after the other".  For a visitor's
 * consenting requests r_0 .. r_m in request order: r_0 tests the stored session against times[r_0]; r_j (j >= 1) starts from an empty session iff
 * times[r_j] > times[r_j-1] and times[r_j] - times[r_j-1] > idle_secs (the predecessor would have stored its own time, whether or not its click was appended) -- its click
 * is then kept even where it repeats the previous one; the last request stores its window with epoch = times[r_m] (the last time, not the largest).  An attached harvest
 * is offered the session every such break ends, once: the visitor's key, epoch = times[r_j-1], the items of r_j-1's window as the store would have held it (the history
 * window H where one is set); min_len, capacity and lost apply as for (R) and the offer counts in from_return.  Append order within one call: the heads' stored sessions
 * in ascending key order, as for the untimed call, then the sessions ended inside the call in ascending key order and, within a key, request order.
 * now_secs is the SWEEP CLOCK: the capacity rule's automatic sweep alone reads it.  Pass a lower bound of times -- what the sweep drops is then older than ttl_secs for
 * every request of the call, which would have found it idle anyway (ttl_secs >= idle_secs), and the sweep only moves a session from (R) to (S) in the harvest's counters.
 * now_secs = 0 reads the system clock, as everywhere in this ABI: that is WRONG for a recorded log, whose sessions it would drop as long expired.
 * NULL times: SRN_EINVAL.  Every check of the untimed call applies unchanged, before anything is launched.  A call without times enqueues exactly what it always has. */
int srn_recommend_batch_device_at(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids,
                                  const uint8_t* d_consent, const uint64_t* d_times, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m,
                                  size_t how_many, unsigned flags, uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts, void* stream);
int srn_recommend_batch_at(const srn_index_t* idx, srn_device_sessions_t* store, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids,
                           const uint8_t* consent, const uint64_t* times, size_t n, uint64_t now_secs, size_t max_items_in_session, size_t k, size_t m, size_t how_many,
                           unsigned flags, uint64_t* out_ids, double* out_scores, uint32_t* out_counts);

/* ---- click feedback: served rows scored against the visitor's next click, on the device (srn_feedback.hip) ----
 * A click feedback log keeps, per visitor, the last row served to it: key (128 bit) -> (ids[0 .. c), n_model, epoch).  It is an object of its own, beside the session
 * store.  srn_feedback_observe* takes a batch of requests and the rows just served to them (the arrays of a srn_recommend_batch* call and its outputs) and gives what
 * handling the requests one after the other, j = 0 .. n-1, with one `now` gives:
 *   no consent                           rank[j] = SRN_FEEDBACK_NONE; nothing is read or stored               (counted as no_consent)
 *   consent, no entry for the key        rank[j] = SRN_FEEDBACK_NONE                                          (first_seen)
 *   consent, the entry fails the idle rule (now > epoch and now - epoch > idle_secs, the session store's test): rank[j] = SRN_FEEDBACK_NONE   (idle_expired)
 *   otherwise the request is OBSERVED:   r = the 1-based position of item_ids[j] among the entry's c ids, 0 if it is not there; rank[j] = r, with SRN_FEEDBACK_FILLED
 *                                        or-ed in when r > n_model; observed += 1 and, for r > 0, hits_model[r] += 1 (r <= n_model) or hits_filled[r] += 1
 *   then, for every consenting request, the row is stored: c = counts[j] (0xFFFFFFFF -- not served -- is stored as 0; a count above how_many is read as how_many),
 *                                        ids = ids[j * how_many .. + c), n_model = the number of those c entries whose score is finite (filled entries score -inf,
 *                                        DESIGN.md 4.9; c without scores), epoch = now                      (stored)
 * An empty stored row makes the next click an observed miss (the evaluator counts an empty row: qty += 1).  Positions >= c of a row are never read, the id 0 is an id
 * like any other, and keys are compared by all 128 bits.  Replaying a test set through srn_recommend_batch* and this call reproduces the Mrr and HitRate terms of
 * srn_evaluate (SRN_FLAG_EVAL_HANDLER, length = how_many) request by request: 1 / r and 1, or 0 and 0.
 * Everything is integer work on the caller's stream with no host round trip; ranks and counters are the same from run to run and for any cut of the requests into calls.
 *   capacity   visitors the log can hold; the table has at least 2 * capacity slots (a power of two, linear probing, no tombstones).  The capacity rule is the session
 *              store's: the host adds n to an upper bound per call; only a call that would pass `capacity` waits for the device, counts, and -- if dropping the
 *              entries older than ttl_secs makes the room -- sweeps; otherwise SRN_ENOMEM with the log as it was.  No growth.
 *   row_cap    ids a stored row may have (1..SRN_MAX_HOW_MANY).  A slot is 40 + 8 * row_cap bytes rounded up to 128.  One table is allocated; a sweep allocates the
 *              second one, rebuilds into it and frees the first.
 *   ttl_secs / idle_secs: as srn_device_sessions_create (0 = 30 / 20 minutes; ttl_secs < idle_secs: SRN_EINVAL).
 * Calls on one log are serialised by the library (a mutex for the enqueue, an event between consecutive calls); the caller puts observe on the stream that produced
 * the rows.  Errors are raised before anything changes: NULL log or arrays SRN_EINVAL; n = 0 SRN_OK; n > 2^24 SRN_ERANGE; how_many 0 SRN_EINVAL, above row_cap SRN_ERANGE;
 * no such GPU SRN_ENODEV. */
#define SRN_FEEDBACK_NONE 0xFFFFFFFFu
#define SRN_FEEDBACK_FILLED 0x80000000u
typedef struct srn_feedback srn_feedback_t;
typedef struct {
    uint64_t capacity, slots, row_cap, slot_bytes;
    uint64_t live_bound;        /* the host's upper bound of the occupied slots */
    uint64_t sweeps, refused;   /* rebuilds that dropped old entries (explicit or automatic) | calls refused with SRN_ENOMEM for capacity */
    uint64_t ttl_secs, idle_secs;
    /* since creation or srn_feedback_reset_counters: requests = no_consent + first_seen + idle_expired + observed; hits_* = the sum of the histogram's bins */
    uint64_t requests, no_consent, first_seen, idle_expired, observed, hits_model, hits_filled;
    uint64_t stored;            /* rows stored: the consenting requests */
} srn_feedback_stats_t;
int srn_feedback_create(int device, size_t capacity, size_t row_cap, uint64_t ttl_secs, uint64_t idle_secs, srn_feedback_t** out);
void srn_feedback_free(srn_feedback_t* f);
/* Device buffers on the log's GPU, enqueued on `stream` (a hipStream_t) without host synchronisation.  d_consent: one byte per request, NULL = every request consents.
 * d_ids[n * how_many] / d_scores (may be NULL) / d_counts[n]: the rows served to the requests, how_many the row stride.  d_out_rank[n] (may be NULL: counters only).
 * now_secs = 0: the system clock, read once. */
int srn_feedback_observe_device(srn_feedback_t* f, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids, const uint8_t* d_consent, size_t n,
                                uint64_t now_secs, const uint64_t* d_ids, const double* d_scores, const uint32_t* d_counts, size_t how_many, uint32_t* d_out_rank,
                                void* stream);
/* The same with host pointers (pageable allowed); blocks. */
int srn_feedback_observe(srn_feedback_t* f, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids, const uint8_t* consent, size_t n,
                         uint64_t now_secs, const uint64_t* ids, const double* scores, const uint32_t* counts, size_t how_many, uint32_t* out_rank);
/* The timed batch: times[i] is request i's clock, and the call gives what n one-request calls give, call i with now_secs = times[i], in request order.
 * The first consenting request of a visitor tests its entry's epoch against its own time; a later one is scored against the row served to its predecessor unless
 * times[r_j] > times[r_j-1] and times[r_j] - times[r_j-1] > idle_secs -- then its rank is SRN_FEEDBACK_NONE and it counts in idle_expired; the entry is stored with the
 * last request's time.  now_secs is the capacity rule's sweep clock alone (a lower bound of times; 0 = the system clock, wrong for a recorded log).  NULL times:
 * SRN_EINVAL; every other check as for the untimed call. */
int srn_feedback_observe_device_at(srn_feedback_t* f, const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids, const uint8_t* d_consent,
                                   const uint64_t* d_times, size_t n, uint64_t now_secs, const uint64_t* d_ids, const double* d_scores, const uint32_t* d_counts,
                                   size_t how_many, uint32_t* d_out_rank, void* stream);
int srn_feedback_observe_at(srn_feedback_t* f, const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids, const uint8_t* consent, const uint64_t* times,
                            size_t n, uint64_t now_secs, const uint64_t* ids, const double* scores, const uint32_t* counts, size_t how_many, uint32_t* out_rank);
/* geometry and counters; waits for the log's kernels.  SRN_ESTATE, with *out filled in, if a batch ever found the table full -- rows were dropped; the capacity
 * rule excludes it (srn_feedback_sweep reports the same) */
int srn_feedback_stats(srn_feedback_t* f, srn_feedback_stats_t* out);
/* hits by rank: hits_model[r] / hits_filled[r] for r = 1 .. row_cap ([0] is unused and 0; either array may be NULL).  cap = entries per array, at least row_cap + 1
 * (below: SRN_ERANGE); entries beyond row_cap are written as 0.  Blocks. */
int srn_feedback_histogram(srn_feedback_t* f, uint64_t* hits_model, uint64_t* hits_filled, size_t cap);
/* every counter, both histograms and (where enabled) the bootstrap's replicate words back to 0, behind the log's previous call; the table is untouched */
int srn_feedback_reset_counters(srn_feedback_t* f);
/* drops the entries older than ttl_secs at now_secs (a rebuild); *n_live (may be NULL) = entries kept.  No device memory for the second table: SRN_ENOMEM, the log as it
 * was.  Blocks. */
int srn_feedback_sweep(srn_feedback_t* f, uint64_t now_secs, uint64_t* n_live);
/* (test aid, blocks) one key's entry as a request at now_secs would read it: *out_count = c and the first c of out_ids (cap < c: SRN_ERANGE), *out_n_model, *out_epoch;
 * *out_count = SRN_FEEDBACK_NONE for a key the log does not hold or whose entry fails the idle rule at now_secs (now_secs = 1: whatever is stored; 0: the clock). */
int srn_feedback_get(srn_feedback_t* f, uint64_t key_hi, uint64_t key_lo, uint64_t now_secs, uint64_t* out_ids, size_t cap, uint32_t* out_count, uint32_t* out_n_model,
                     uint64_t* out_epoch);
/* Visitor-clustered bootstrap of the log's counters.  While it is enabled, replicate b = 0 .. replicates-1 weighs every OBSERVED request of
 * visitor (key_hi, key_lo) with
 *   w(seed, b, key) = boot_weight(boot_replicate_key(seed, b), fold(key)),   fold(key) = mix64(key_hi ^ 0x9E3779B97F4A7C15) ^ key_lo
 * -- the Poisson(1)-cut-at-12 rule of srn_bootstrap_weights with the folded key in the session index's place, from nothing but (seed, b, key): not from `replicates`,
 * the call, the cut of the requests into calls, the rows or the configuration -- and the log keeps, per replicate, 1 + 2 * row_cap exact unsigned 64-bit sums:
 *   observed_w[b] = sum of w over the observed requests;  hits_model_w[b][r] / hits_filled_w[b][r] = sum of w over those whose rank is r on a model / a filled entry
 * Requests that are not observed (rank SRN_FEEDBACK_NONE) add nothing.  Integer sums: the same for any order, run, entry point and cut into calls, and for a timed call
 * what one call per request gives.  Every srn_feedback_observe* call on the log runs one more kernel behind its own on the same stream; with the bootstrap off nothing
 * about a call changes.  srn_feedback_reset_counters zeroes the words, a sweep leaves them, a call refused with SRN_ENOMEM leaves them, srn_feedback_free releases them.
 *   enable   allocates and zeroes the words behind the log's previous call.  replicates 0: SRN_EINVAL; above SRN_MAX_BOOTSTRAP: SRN_ERANGE; a log whose row_cap is above
 *            SRN_FEEDBACK_BOOTSTRAP_MAX_ROW_CAP: SRN_ERANGE; already enabled: SRN_ESTATE
 *   disable  frees them (waits for the log's kernels); SRN_OK when not enabled
 *   info     *replicates / *seed (either may be NULL); 0 / 0 when off
 *   read     blocks.  observed[replicates] and hits_*[replicates][rank_cap], rank_cap >= row_cap + 1, entry [b][0] unused and 0, entries beyond row_cap 0; any array may
 *            be NULL.  replicates_cap below `replicates` or rank_cap below row_cap + 1: SRN_ERANGE; not enabled: SRN_ESTATE
 *   weights  the rule on the host, no GPU needed: out[i] = w(seed, replicate, (key_hi[i], key_lo[i])).  n = 0: SRN_OK; a NULL array with n > 0: SRN_EINVAL */
#define SRN_FEEDBACK_BOOTSTRAP_MAX_ROW_CAP 64
int srn_feedback_bootstrap_enable(srn_feedback_t* f, uint32_t replicates, uint64_t seed);
int srn_feedback_bootstrap_disable(srn_feedback_t* f);
int srn_feedback_bootstrap_info(srn_feedback_t* f, uint32_t* replicates, uint64_t* seed);
int srn_feedback_bootstrap_read(srn_feedback_t* f, uint64_t* observed, uint64_t* hits_model, uint64_t* hits_filled, size_t replicates_cap, size_t rank_cap);
int srn_feedback_bootstrap_weights(uint64_t seed, uint32_t replicate, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out);

/* ---- traffic split: one batch served under several arms, sticky per visitor (srn_arms.hip) ----
 * A split is (seed, weights[0 .. A)), A = 1 .. SRN_MAX_ARMS, weights uint32 (zeros allowed), W = their sum in 1 .. 2^32 - 1.  A visitor's arm is
 *   fold(key)  = mix64(key_hi ^ 0x9E3779B97F4A7C15) ^ key_lo                      (the feedback bootstrap's fold)
 *   u          = mix64( mix64(seed ^ 0x53524E5F41524D53) ^ (fold * 0xD1B54A32D192ED03 + 1) ) >> 32
 *   T_a        = floor(2^32 * (w_0 + .. + w_a) / W),  a = 0 .. A-2            (64-bit: T_a may be 2^32)
 *   arm(key)   = #{ a : T_a <= u }
 * so arm a holds the u in [T_(a-1), T_a), an arm of weight 0 holds nothing, and the arm depends on (seed, weights, key) alone: not on consent, the item, the time,
 * the batch, the cut of the requests into calls or the run.  A request without consent is assigned by its key like any other and served with its arm's parameters.
 * srn_recommend_batch_split_device serves request i with arms[arm(key_i)]: its index, window, k, m and flags (those of srn_recommend_batch*), all arms against the one
 * store, and feeds arm a's requests and rows to arms[a].feedback where that is not NULL.  Rows, store, an attached harvest and every log are left as by one
 * srn_recommend_batch_device[_at] call (and one srn_feedback_observe_device[_at] call) per non-empty arm, arm 0 first, each over its arm's requests in request order
 * with the call's one `now` (now_secs = 0: the system clock, read once for all of them).  A visitor is in one arm, so the visitor's clicks stay in order.
 * The call assigns, counts and gathers the requests by arm on `stream`, then WAITS FOR THE STREAM ONCE (hipStreamSynchronize: the arms' calls need their sizes on
 * the host), then enqueues the arms' calls into arm-ordered row buffers and one kernel that puts the rows back in request order; it returns without waiting again.
 * As in the plain call, entries of a row beyond its count are not written.  d_out_arm[n] (may be NULL) receives the arms, d_out_rank[n] (may be NULL) the logs'
 * ranks -- SRN_FEEDBACK_NONE for the requests of an arm without a log.  A log that refuses its arm's call under its capacity rule does not fail the call: the rows
 * are served, the arm's ranks are SRN_FEEDBACK_NONE and feedback_rc[a] (may be NULL; SRN_OK otherwise) is SRN_ENOMEM.
 * The store's capacity rule is asked once for all n requests before the first arm is served, so SRN_ENOMEM leaves the store as it was.  With A = 1 the call is the
 * plain call on the caller's buffers: no scratch, no kernel of its own, no synchronisation (counted in shortcut_calls, not in calls).
 * create allocates every buffer of the device form -- about max_batch * (46 + 16 * max_how_many) bytes, none for A = 1 -- so calls allocate nothing; the host form
 * stages through a buffer that grows with the largest call, as srn_recommend_batch does.  Calls on one handle take turns (a mutex, and an event between
 * consecutive calls).  The arms' indices may differ but must be on the split's device, as the store and the logs.  The result cache behaves as for any call.
 * Errors, all before anything is enqueued or changed: NULL handle, arms, store, request array or output (ids, scores, counts) SRN_EINVAL; n_arms outside
 * 1 .. SRN_MAX_ARMS SRN_ERANGE, not the handle's SRN_EINVAL; W = 0 SRN_EINVAL, W >= 2^32 SRN_ERANGE; n > max_batch, how_many > max_how_many or above a log's row_cap
 * SRN_ERANGE; one log in two arms, an index or a log on another device SRN_EINVAL; and for every arm the error srn_recommend_batch_device gives for its parameters.
 * n = 0: SRN_OK.  create: max_batch or max_how_many 0 SRN_EINVAL, max_batch above 2^24 or max_how_many above SRN_MAX_HOW_MANY SRN_ERANGE, no such GPU SRN_ENODEV.
 *   set_weights  the ramp: other weights for the same number of arms, from the next call on.  Only the keys whose u lies between an old and a new threshold move.
 *   arms         the rule on the host, no GPU needed: out[i] = arm(key_hi[i], key_lo[i]).  n = 0: SRN_OK; a NULL array with n > 0: SRN_EINVAL.
 *   info         thresholds[a] = T_a for a < n_arms (thresholds[n_arms - 1] = 2^32), 0 behind; served[a] = requests arm a has served; device_bytes: what the
 *                handle holds on the device now. */
#define SRN_MAX_ARMS 16
typedef struct srn_traffic_split srn_traffic_split_t;
typedef struct {
    const srn_index_t* idx;
    srn_feedback_t* feedback;   /* or NULL */
    uint32_t max_items_in_session, k, m, flags;
} srn_arm_t;
typedef struct {
    uint32_t n_arms, max_how_many;
    uint64_t seed, max_batch, device_bytes, thresholds[SRN_MAX_ARMS], served[SRN_MAX_ARMS], calls, shortcut_calls;
} srn_traffic_split_info_t;
int srn_traffic_split_create(int device, const uint32_t* weights, size_t n_arms, uint64_t seed, size_t max_batch, size_t max_how_many, srn_traffic_split_t** out);
int srn_traffic_split_free(srn_traffic_split_t* split);
int srn_traffic_split_info(const srn_traffic_split_t* split, srn_traffic_split_info_t* out);
int srn_traffic_split_set_weights(srn_traffic_split_t* split, const uint32_t* weights, size_t n_arms);
int srn_traffic_split_arms(uint64_t seed, const uint32_t* weights, size_t n_arms, const uint64_t* key_hi, const uint64_t* key_lo, size_t n, uint8_t* out);
/* d_times NULL: an untimed batch; otherwise the timed one (srn_recommend_batch_device_at), now_secs its sweep clock */
int srn_recommend_batch_split_device(srn_traffic_split_t* split, const srn_arm_t* arms, size_t n_arms, srn_device_sessions_t* store,
                                     const uint64_t* d_key_hi, const uint64_t* d_key_lo, const uint64_t* d_item_ids, const uint8_t* d_consent, const uint64_t* d_times,
                                     size_t n, uint64_t now_secs, size_t how_many, uint64_t* d_out_ids, double* d_out_scores, uint32_t* d_out_counts,
                                     uint8_t* d_out_arm, uint32_t* d_out_rank, int* feedback_rc, void* stream);
/* The same with host pointers (pageable allowed): staged, served through the device form on a stream of the handle's, copied back; blocks. */
int srn_recommend_batch_split(srn_traffic_split_t* split, const srn_arm_t* arms, size_t n_arms, srn_device_sessions_t* store,
                              const uint64_t* key_hi, const uint64_t* key_lo, const uint64_t* item_ids, const uint8_t* consent, const uint64_t* times,
                              size_t n, uint64_t now_secs, size_t how_many, uint64_t* out_ids, double* out_scores, uint32_t* out_counts,
                              uint8_t* out_arm, uint32_t* out_rank, int* feedback_rc);
/* (measurement aid) with timing enabled the device form records HIP events around its own kernels; last_ms waits for them: *ms_front = assign + offsets + gather,
 * *ms_scatter = the scatter (either may be NULL).  SRN_EINVAL when the last call was not timed or took the shortcut. */
int srn_traffic_split_timing(srn_traffic_split_t* split, int enable);
int srn_traffic_split_last_ms(srn_traffic_split_t* split, double* ms_front, double* ms_scatter);

/* ---- session harvest: finished sessions logged on the device, and training events from them (srn_harvest.hip) ----
 * A harvest is a device-resident log, attached to one device session store, that receives every session at the moment the store forgets it: each one exactly once,
 * on the stream of the call that forgets it, with nothing read back.  An entry (key, epoch, len, items[0 .. len)) is harvested when, and only when, the store drops
 * it by its own rules:
 *   (R) return after idle   inside srn_recommend_batch*: the first consenting request of a key in the call finds the key stored with len > 0 and idle
 *                           (now > epoch and now - epoch > idle_secs); the stored entry is copied before the call's result overwrites it
 *   (S) a rebuild drops it  the entry is occupied and older than ttl_secs at the rebuild's now: srn_device_sessions_sweep, the capacity rule's automatic sweep,
 *                           srn_device_sessions_resize, growth.  A resize or growth that is refused or fails harvests nothing: store and harvest are as they were
 * NOT harvested: what srn_device_sessions_update replaces; an entry replaced or beaten in srn_device_sessions_import*; the entries of a store that is freed
 * (srn_device_sessions_free); anything srn_device_sessions_load reads; requests without consent, which never touch the store.
 * A harvested session carries the epoch as stored -- the time of its last click -- and exactly the items the slot held: with a history window H the last H clicks,
 * otherwise the last max_items_in_session.  An entry of fewer than min_len items (0 is read as 1) is counted in skipped_short and not stored.  Sessions beyond
 * `capacity` are not stored and counted exactly in `lost`; the serving call and the sweep never fail or wait because the log is full.  The log is appended in a fixed
 * order -- (R): ascending (key_hi, key_lo) within a call; (S): ascending slot -- behind a device cursor, without atomics, so which sessions a full log loses does not
 * depend on scheduling (for (S) it depends on where the keys lie in the table).
 *   capacity   sessions the log holds (1..2^30); items_cap: items per session (1..SRN_MAX_SESSION_LEN).  All storage -- 28 + 8 * items_cap bytes per session -- is
 *              allocated at creation.  capacity or items_cap 0: SRN_EINVAL; above their limits: SRN_ERANGE; no such GPU: SRN_ENODEV; no device memory: SRN_ENOMEM.
 * srn_device_sessions_set_harvest(store, h) attaches, (store, NULL) detaches (SRN_OK also when nothing is attached; it waits for the store's last call).  One harvest
 * is attached to at most one store and a store has at most one harvest: a second attach is SRN_ESTATE; a harvest on another device than the store SRN_EINVAL; a
 * harvest whose items_cap is below the store's SRN_ERANGE, and so is a srn_device_sessions_resize to an items_cap above the attached harvest's (before anything
 * changes).  Freeing the store detaches; srn_harvest_free of an attached harvest is SRN_ESTATE (NULL: SRN_OK).  With no harvest attached every store call does what it
 * did before.  Every harvest call takes the store's mutex and is ordered behind the store's previous call, like the store's own calls; a detached harvest uses a
 * stream and an event of its own. */
typedef struct srn_harvest srn_harvest_t;
typedef struct {
    uint64_t capacity, items_cap, min_len;
    uint64_t stored, stored_items;      /* the sessions the log holds now, and the sum of their lengths = the rows srn_harvest_events_device writes */
    uint64_t lost, skipped_short;       /* offered when the log was full | offered with fewer than min_len items */
    uint64_t from_return, from_rebuild; /* offered by (R) | by (S) */
    uint64_t cleared;                   /* sessions srn_harvest_clear removed: from_return + from_rebuild = stored + cleared + lost + skipped_short */
} srn_harvest_stats_t;
int srn_harvest_create(int device, size_t capacity, size_t items_cap, uint32_t min_len, srn_harvest_t** out);
int srn_harvest_free(srn_harvest_t* h);
int srn_device_sessions_set_harvest(srn_device_sessions_t* s, srn_harvest_t* harvest_or_null);
/* blocks and reads the device words back */
int srn_harvest_stats(srn_harvest_t* h, srn_harvest_stats_t* out);
/* The stored sessions in CANONICAL order -- (epoch, key_hi, key_lo) ascending, a triple that is unique because two sessions of one visitor end more than idle_secs
 * apart -- sorted on the device by stable radix passes, in the arrays of srn_device_sessions_export: the same set of sessions gives the same bytes however the requests
 * were cut into calls and wherever the sweeps fell; the log's internal order is not exposed.  Neither call consumes the log.  items_stride below the harvest's
 * items_cap: SRN_ERANGE.
 * _export_device: device buffers on the harvest's GPU, enqueued on `stream` with no host synchronisation; writes the first min(stored, cap) sessions and *d_n = stored
 *                 -- the caller compares.  NULL harvest or d_n: SRN_EINVAL.
 * _export:        host arrays; blocks.  stored > cap: SRN_ERANGE with *n = stored and the arrays untouched.  NULL harvest or n: SRN_EINVAL. */
int srn_harvest_export(srn_harvest_t* h, size_t cap, uint64_t* key_hi, uint64_t* key_lo, uint64_t* epoch, uint32_t* len, uint64_t* items, size_t items_stride, size_t* n);
int srn_harvest_export_device(srn_harvest_t* h, size_t cap, uint64_t* d_key_hi, uint64_t* d_key_lo, uint64_t* d_epoch, uint32_t* d_len, uint64_t* d_items,
                              size_t items_stride, uint64_t* d_n, void* stream);
/* The stored sessions as the rows srn_sessions_from_events reads with SRN_EVENTS_TIME_I64 | SRN_EVENTS_DEVICE: session i in canonical order gets
 * session_id = id_base + i and one row per stored item, in session order, each with time = its epoch.  Device buffers, enqueued on `stream` with no host
 * synchronisation; writes the first min(rows, cap_rows) rows and *d_rows = rows (= stored_items) -- the caller compares. */
int srn_harvest_events_device(srn_harvest_t* h, uint64_t id_base, size_t cap_rows, uint64_t* d_session_ids, uint64_t* d_item_ids, int64_t* d_times, uint64_t* d_rows,
                              void* stream);
/* Empties the log -- stored and stored_items become 0, the sessions removed are added to `cleared` -- behind the previous call.  lost, skipped_short, from_return and
 * from_rebuild keep running until the harvest is freed. */
int srn_harvest_clear(srn_harvest_t* h);

/* ---- offline evaluation: test sets and hyper-parameter trials ----------------------------------------------------------
 * The reference's evaluation loop (src/bin/evaluator.rs:46-76, src/objective.rs:8-52) on the GPU: every prefix of every test session is
 * predicted and scored against the rest of its session, and the eight metrics of src/metrics/evaluation_reporter.rs come back.  Prefixes,
 * recommendation rows and per-query terms stay in device memory; one srn_evaluate call runs any number of trials on one index.
 *
 * An evaluation set binds test sessions and training-item frequencies to one index (which must have a device: SRN_ENODEV otherwise):
 *   items_flat / sess_off: test session i = items_flat[sess_off[i] .. sess_off[i+1]), each ordered by time as read_test_data_evolving orders it
 *                          (src/io.rs:40-59; equal times keep file order).  A session of one event gives no query (the loop starts at state 1).
 *   train_item_ids / train_item_counts: how often each item occurs in the training data's item column (popularity.rs:20-29).  Repeated ids
 *                          add up; the number of distinct ids is Coverage's denominator (coverage.rs:17-25).
 * The set keeps a pointer to the index: free the set first. */
typedef struct srn_eval_set srn_eval_set_t;
/* Trials under the serving rules.  A test session e_1..e_n gives one query per state t = 1..n-1, scored against the raw e_{t+1}..e_n, with or without
 * these flags.  W = max_items_in_session, H' = history if history > 0, else W.
 *   c(t)      with SRN_FLAG_EVAL_HANDLER e_1..e_t without every e_j (j >= 2) equal to e_{j-1} -- what the /v1/recommend handler's rule "append unless the click repeats
 *             the stored last item, drop the oldest beyond the limit" leaves of the clicks (recommend_resource.rs:39-54); without the flag e_1..e_t
 *   query(t)  the last min(|c(t)|, W) items of c(t); seen(t) the last min(|c(t)|, H') -- the window a device session store with history H holds behind click t
 *   list      SRN_FLAG_EXCLUDE_SESSION: query(t)'s items; SRN_FLAG_EXCLUDE_SEEN (alone or with the former): seen(t); neither: none
 * The scored rows are srn_predict_batch_device_excl's for (query(t), list) -- "remove the ids from all candidates, then cut to how_many" -- filled under that call's rule
 * with SRN_FLAG_FILL.  SRN_FLAG_EVAL_HANDLER | SRN_FLAG_EXCLUDE_SEEN scores the rows srn_recommend_batch serves with SRN_FLAG_EXCLUDE_SEEN to one visitor per test
 * session, clicks in order, on a store with history H at a constant clock.  The launch sequence runs at the internal how_many + capacity (H' with
 * SRN_FLAG_EXCLUDE_SEEN, W with SRN_FLAG_EXCLUDE_SESSION alone); above SRN_MAX_HOW_MANY: SRN_ERANGE.  A trial with none of the three flags is the reference evaluator's. */
#define SRN_FLAG_EVAL_HANDLER 32u
typedef struct {
    uint32_t k, m, how_many;          /* predict's arguments (m <= the index's m_index is the normal case: one index answers every smaller m) */
    uint32_t max_items_in_session;    /* the window: a prefix is its last max_items_in_session items (evaluator.rs:50-55); 1..SRN_MAX_SESSION_LEN */
    uint32_t length;                  /* @N of the metrics (1..SRN_MAX_HOW_MANY); independent of how_many (hyperparameter_search.rs asks for 21, scores @20) */
    uint32_t flags;                   /* SRN_FLAG_BUSINESS_LOGIC, SRN_FLAG_FILL (the filled rows are scored; SRN_ESTATE without a ranking), and the serving rules below:
                                       * SRN_FLAG_EXCLUDE_SESSION, SRN_FLAG_EXCLUDE_SEEN, SRN_FLAG_EVAL_HANDLER */
    uint32_t max_chunk_queries;       /* queries per device round (0 = default); rounded down to a multiple of 256.  Results do not depend on it */
    uint32_t history;                 /* the seen-items window H of SRN_FLAG_EXCLUDE_SEEN (below): 0 = none, or max_items_in_session..SRN_MAX_SESSION_LEN (else SRN_ERANGE).
                                       * Without SRN_FLAG_EXCLUDE_SEEN it changes no row.  (The field was `reserved`, 0: same offset, same meaning of 0) */
} srn_eval_trial_t;
typedef struct {
    uint64_t n_evaluations;           /* qty_evaluations: queries of the trial */
    /* the report line of evaluation_reporter.rs, in its order (F1 of 0 / 0 is 0, f1score.rs:27-36) */
    double mrr, ndcg, hit_rate, popularity, precision, coverage, recall, f1score;
    /* raw sums over the queries (averages = sum / n_evaluations) */
    double sum_mrr, sum_ndcg, sum_hit_rate, sum_popularity, sum_precision, sum_recall;
    uint64_t covered_items, unique_training_items;   /* Coverage = covered_items / unique_training_items */
    double ms_predict, ms_eval;       /* device time (HIP events) of the predict launches and of the expansion + metric + reduction kernels */
} srn_eval_result_t;
int srn_eval_set_create(const srn_index_t* idx, const uint64_t* items_flat, const uint64_t* sess_off, size_t n_sessions,
                        const uint64_t* train_item_ids, const uint64_t* train_item_counts, size_t n_train_items, srn_eval_set_t** out);
/* the same from the reference's TSV files "SessionId ItemId Time" (src/io.rs:13-59): sessions in ascending SessionId, events by rounded time */
int srn_eval_set_from_tsv(const srn_index_t* idx, const char* test_path, const char* train_path, srn_eval_set_t** out);
/* the same from rows in memory, grouped and counted on the index's GPU: n_test test rows passed as to srn_sessions_from_events (the same flags; device arrays must
 * be on the index's GPU and are read on `stream`) and the item column of the n_train training rows.  Test sessions in ascending session id, each one's rows by
 * rounded time, equal times in input order; training counts are occurrences per id.  The set is the one srn_eval_set_from_tsv builds from files holding those rows
 * (session ids below 2^32 and times that are not negative: the file reader keeps 32 bits of a session id and orders negative times, this call keeps 64 and reads
 * them as 0): every report and every bootstrap replicate is the same bits.  Only the session offsets come to the host.  n_test >= 2^32 - 1 or n_train >= 2^32 - 1:
 * SRN_ERANGE; a null buffer with rows, unknown flags: SRN_EINVAL.  n_test = 0 gives a set without queries.  The call waits for `stream`. */
int srn_eval_set_from_events(const srn_index_t* idx, const uint64_t* test_session_ids, const uint64_t* test_item_ids, const void* test_times, size_t n_test,
                             const uint64_t* train_item_ids, size_t n_train, unsigned flags, void* stream, srn_eval_set_t** out);
/* Runs n_trials trials and blocks until they are done; out[t] is trial t's result.  Sums are added in a fixed order (partial sums per
 * group of 256 queries): the same trial gives the same bits from call to call, alone or among others, for any max_chunk_queries.
 * Every trial is checked before anything is launched: predict's argument checks, length 0 (SRN_EINVAL) or above SRN_MAX_HOW_MANY, and a
 * window of 0 (SRN_EINVAL) or above SRN_MAX_SESSION_LEN (SRN_ERANGE: a prefix could exceed the kernels' session limit), a history outside its range and an
 * internal how_many above SRN_MAX_HOW_MANY (both SRN_ERANGE) fail the whole call.
 * stream: a hipStream_t (NULL = the null stream). */
int srn_evaluate(srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, srn_eval_result_t* out, void* stream);
void srn_eval_set_free(srn_eval_set_t* set);

/* ---- bootstrap confidence intervals for trials ------------------------------------------------------------
 * srn_evaluate with a session-clustered Poisson bootstrap next to every trial: replicate b weighs all queries of test session s (its index in the set's order;
 * sessions of one event give no query but keep their index) with
 *   w(seed, b, s) = #{ i : T[i] <= u },  u = mix64( mix64(seed + (b + 1) * 0x9E3779B97F4A7C15) ^ (s * 0xD1B54A32D192ED03 + 1) ) >> 32     (mod 2^64)
 *   T[i] = round(2^32 * P(Poisson(1) <= i)), i = 0..11 -- an integer in 0..12 that depends on (seed, b, s) alone: not on replicates, the trial, the index or the chunk.
 * rep[t][b][0] = sum of the weights over the queries; rep[t][b][1..6] = the weighted sums of mrr, ndcg, hit_rate, popularity, precision, recall (the order of the
 * sum_* fields).  The order of the additions is fixed: per group of 256 consecutive query indices from +0.0 in query order, acc = acc + (double)w * term (product
 * rounded, then the sum), then the groups in order onto the total.  A replicate's seven doubles are the same bits from run to run, for any max_chunk_queries, alone or
 * among other trials and for any replicates > b.  Coverage is not resampled.  Only the rep array comes back beside the results; device memory beyond srn_evaluate's:
 * the totals (n_trials * replicates * 7 doubles) and (chunk / 256) * min(replicates, 1024) * 7 doubles of scratch.
 * out[t] is srn_evaluate's result for the trial, bit for bit (the two ms_* fields aside; the bootstrap kernels are in neither).
 * boot or rep NULL, replicates == 0, flags != 0: SRN_EINVAL; replicates > SRN_MAX_BOOTSTRAP: SRN_ERANGE; then srn_evaluate's own refusals, all before anything is launched. */
#define SRN_MAX_BOOTSTRAP 4096
#define SRN_BOOTSTRAP_SUMS 7
typedef struct { uint64_t seed; uint32_t replicates; uint32_t flags; } srn_bootstrap_t;   /* flags: 0 */
int srn_evaluate_bootstrap(srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, const srn_bootstrap_t* boot,
                           srn_eval_result_t* out, double* rep /* [n_trials][replicates][7], host */, void* stream);
/* host only: the rule -- out[i] = w(seed, replicate, first_session + i), i < n.  NULL out with n > 0: SRN_EINVAL */
int srn_bootstrap_weights(uint64_t seed, uint32_t replicate, uint64_t first_session, size_t n, uint8_t* out);

/* ---- trials by segment ------------------------------------------------------------------------------------
 * srn_evaluate (with boot: srn_evaluate_bootstrap) that also says which queries a figure comes from.  A segmentation maps every query (s, t) of the set -- s the
 * test session's index in the set's order, t = 1..n-1 its state, scored against the raw e_{t+1}..e_n -- to a segment id in 0..segments-1.  The id depends on the set
 * and the segmentation alone, never on the trial: under SRN_FLAG_EVAL_HANDLER it is still the raw t, e_t and e_{t+1}.
 *   SRN_SEG_STATE          min(t, segments) - 1: states 1..segments-1 each their own segment, the last one holds t >= segments
 *   SRN_SEG_LABEL          labels[s]: one uint16 per test session in the set's order, sessions of one event included (n_labels = the set's sessions, else SRN_EINVAL;
 *                          a label >= segments: SRN_EINVAL)
 *   SRN_SEG_TARGET_COUNT   #{ j : bounds[j] <= c(e_{t+1}) } over segments-1 strictly ascending bounds; c(x) is the training count the set holds for x, 0 for an item the
 *                          index's dictionary does not know.  With bounds[0] = 1 segment 0 is "the next item was never trained on"
 *   SRN_SEG_CURRENT_COUNT  the same over c(e_t), the clicked item
 * labels and bounds are host pointers, read during the call.  seg_out[t][g] holds the segment's queries and the six sums of srn_eval_result_t; Coverage is a property
 * of the whole row set and is not segmented.  The order of the additions is 10.2's: per group of 256 consecutive global query indices from +0.0 in query order over the
 * group's queries of the segment, acc = acc + term, then the groups in order onto the segment's total -- a segment's sums do not depend on max_chunk_queries, on the
 * other trials, or on `segments` where its queries do not change.  With boot, seg_rep[t][g][b][0..6] are the seven sums of srn_evaluate_bootstrap over the segment's
 * queries: the same weights w(seed, b, s), so a segment is paired with the total, with every other segment and across trials, calls and indices; the same order rule,
 * acc = acc + (double)w * term.  out[t] and rep are srn_evaluate's and srn_evaluate_bootstrap's, bit for bit (the two ms_* fields aside).
 * Refusals, all before anything is launched: seg NULL, seg_out NULL, an unknown mode, segments == 0, reserved != 0, labels NULL or a label >= segments (SRN_SEG_LABEL),
 * bounds NULL with segments > 1 or not strictly ascending (the count modes), with boot a NULL rep or seg_rep: SRN_EINVAL; segments > SRN_MAX_SEGMENTS, with boot
 * segments * replicates > 16 * SRN_MAX_BOOTSTRAP: SRN_ERANGE; then srn_evaluate_bootstrap's and srn_evaluate's own; then n_labels. */
#define SRN_MAX_SEGMENTS 64
#define SRN_SEG_STATE 1u
#define SRN_SEG_LABEL 2u
#define SRN_SEG_TARGET_COUNT 3u
#define SRN_SEG_CURRENT_COUNT 4u
typedef struct { uint32_t mode, segments; const uint16_t* labels; size_t n_labels; const uint64_t* bounds; uint64_t reserved; } srn_segments_t;   /* reserved: 0 */
typedef struct { uint64_t n_evaluations; double sum_mrr, sum_ndcg, sum_hit_rate, sum_popularity, sum_precision, sum_recall; } srn_eval_segment_t;
int srn_evaluate_segments(srn_eval_set_t* set, const srn_eval_trial_t* trials, size_t n_trials, const srn_segments_t* seg, const srn_bootstrap_t* boot /* or NULL */,
                          srn_eval_result_t* out, srn_eval_segment_t* seg_out /* [n_trials][segments] */,
                          double* rep /* [n_trials][replicates][7], or NULL without boot */, double* seg_rep /* [n_trials][segments][replicates][7] */, void* stream);
/* the ids alone, in query order, to the host: *n_queries = the set's queries; out may be NULL (the count alone), else cap < *n_queries: SRN_ERANGE */
int srn_eval_segment_ids(srn_eval_set_t* set, const srn_segments_t* seg, uint16_t* out, size_t cap, size_t* n_queries);

int srn_device_count(int* out);
void srn_limits(srn_limits_t* out);
const char* srn_last_error(void);
const char* srn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SERENADE_HIP_H */
