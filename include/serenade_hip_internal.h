/* serenade_hip_internal.h -- measurement and test aids exported by libserenade_hip.so that are NOT part of the drop-in boundary.
 *
 * include/serenade_hip.h is what a reference-side binding binds: index construction, predict, the shard group, serving.  The three entry
 * points below exist for this repository's own tools and tests (tools/*.py, tests/test_gpu_parity.py): per-phase shader cycles, the per-rank time split of a
 * shard group, and a re-read of the SRN_* experiment knobs.  A host application has no use for them and must not rely on them.
 */
#ifndef SERENADE_HIP_INTERNAL_H
#define SERENADE_HIP_INTERNAL_H

#include "serenade_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Profiling aid: returns (and clears) 16 counters of shader cycles summed over workgroups, one per
 * kernel phase (DESIGN.md "Kernel phases"), accumulated by predict calls made while enabled; then
 * switches the accounting on (enable != 0) or off.  Not for production use. */
int srn_debug_phase_cycles(const srn_index_t* idx, int enable, uint64_t* out16);

/* Measurement aid (environment variable SRN_GROUP_TIMING=1 when the group is created): milliseconds of local shard 0's own launches in the group's last batch --
 * neighbours pipeline: prep records + front end | back end | top-n merge; lists pipeline: head + count + copy | prep + unsharded launch sequence | top-n merge.
 * The call that recorded them synchronised the stream: measurement runs only (tools/shard_rank_time.py). */
int srn_debug_shard_group_times(const srn_shard_group_t* g, double* out_ms3);

/* Measurement aid: how many queries of the last predict call the lean fast kernel listed for its MID instantiation (sessions of <= 10 items with 5..8 posting lists or
 * similarity numerators above 15: DESIGN.md section 4.1); srn_last_path_counts' `general` counts what reached the general kernel after both.  0 when the call had no such tier. */
int srn_debug_last_mid_count(const srn_index_t* idx, uint32_t* out_listed);
/* Measurement aid: how many queries of the last predict call were not served themselves but received the row of an earlier query of the SAME call with the same item
 * sequence (batches of at least SRN_ORDER_MIN queries on the fast path).  0 when the call did not merge (small batch, SRN_NO_DEDUP, other paths). */
int srn_debug_last_dedup_count(const srn_index_t* idx, uint32_t* out_merged);
/* light representatives of the last call -- distinct queries with one posting run of <= 64 kept entries, served one wave each (or handed to the general kernel) by
 * vmis_light_kernel; 0 where the form was off: a batch below SRN_LIGHT_MIN, a call that uses the result cache, a shard group's call */
int srn_debug_last_light_count(const srn_index_t* idx, uint32_t* out_light);
/* the persistent latency path: 100 MHz ticks of the last session the lean form's first resident workgroup served -- [0] waited for the doorbell, [1] doorbell -> prep record
 * written, [2] doorbell -> answer posted */
int srn_debug_serve_stamps(const srn_index_t* idx, uint32_t* out4);
/* Test aid (tests/test_gpu_persistent_edges.py): per resident workgroup of one form of the persistent latency path (form 0: sessions of <= 4 items, form 1: of 5..10), how
 * many sessions it has answered itself (status 0) since srn_index_serve_start -- counted on the host, where srn_index_serve_stats' `served` is.  *out_n = the form's
 * workgroups (out_n may be NULL); cap < that: SRN_ERANGE, with *out_n set.  SRN_ESTATE: nothing resident, or no such form. */
int srn_debug_serve_lane_counts(const srn_index_t* idx, unsigned form, uint64_t* out_served, size_t cap, size_t* out_n);
/* 32-bit words per query of the streaming back end's exchange record at this (k, m) -- 0: none (knobs, shape); the gather form ships k + 1 words */
uint32_t srn_debug_shard_nb_positions_stride(size_t k, size_t m);
/* ... and how many of those MID listed for its BIG form (80 KB of LDS: merged lists beyond the 53 KB layout's buffers). */
int srn_debug_last_big_count(const srn_index_t* idx, uint32_t* out_listed);

/* Test aid: batches of this item shard that went through the wave-per-query back end of srn_sback.hip (the shard group's neighbours pipeline), since the shard was attached. */
int srn_debug_sback_launches(const srn_index_t* idx, uint64_t* out_launches);

/* Test aid: one trial of srn_evaluate with its per-query terms.  out_terms [n * 7] (query order: sessions in set order, states ascending):
 * mrr, hit, ndcg, intersection size, precision, recall, popularity; *out_n = the trial's query count n (out_terms may be NULL to ask for it;
 * cap < n: SRN_ERANGE).  *out (may be NULL) = what srn_evaluate returns for the trial. */
int srn_debug_eval_terms(srn_eval_set_t* set, const srn_eval_trial_t* trial, double* out_terms, size_t cap, size_t* out_n, srn_eval_result_t* out);

/* Measurement aid (tools/eval_bench.py --segments): device time (HIP events, summed over chunks and trials) of the set's most recent srn_evaluate_segments call's
 * segment kernels -- *ms_segments: the id, group and accumulate kernels; *ms_segment_bootstrap: the segmented bootstrap's (0 without boot).  Neither is in ms_eval.
 * Either output may be NULL. */
int srn_debug_eval_segment_ms(srn_eval_set_t* set, double* ms_segments, double* ms_segment_bootstrap);

/* Test / measurement aid: the sessions the store's most recent srn_recommend_batch* call emitted (request q = items[q_off[q] .. q_off[q + 1])), where predict read them:
 * the device pointers (valid until the next call on the store), the request count and the max_len_hint; with h_q_off ([n + 1]) / h_items (cap entries) also copied to
 * the host.  Any output may be NULL.  Blocks until that call is done. */
int srn_debug_device_sessions_last_batch(srn_device_sessions_t* s, const void** d_items, const void** d_q_off, size_t* out_n, size_t* out_max_len,
                                         uint64_t* h_items, size_t cap, uint32_t* h_q_off);

/* Measurement aid (tools/exclude_bench.py): the exclusion filter kernel of srn_predict_batch_device_excl ALONE, over wide rows the caller holds --
 * d_wide_ids / d_wide_scores [nq * wide], d_wide_counts [nq] -> d_out_* [nq * how_many], [nq]; the exclusion CSR and the session CSR (d_items_flat, d_q_off) may each be
 * NULL.  Enqueued on `stream`. */
int srn_debug_exclude_filter(const srn_index_t* idx, size_t nq, const uint64_t* d_wide_ids, const double* d_wide_scores, const uint32_t* d_wide_counts, size_t wide, const uint64_t* d_excl_flat,
                             const uint32_t* d_excl_off, size_t max_excl, const uint64_t* d_items_flat, const uint32_t* d_q_off, size_t how_many, uint64_t* d_out_ids, double* d_out_scores,
                             uint32_t* d_out_counts, void* stream);

/* Measurement aid (tools/fill_bench.py): the fill kernel of SRN_FLAG_FILL ALONE, in place over rows the caller holds -- d_ids / d_scores
 * [nq * how_many], d_counts [nq]; the sessions' CSR is needed (the most recent item), the exclusion CSR may be NULL.  flags: SRN_FLAG_BUSINESS_LOGIC,
 * SRN_FLAG_EXCLUDE_SESSION.  SRN_ESTATE without a ranking.  Enqueued on `stream`. */
int srn_debug_fill(const srn_index_t* idx, size_t nq, uint64_t* d_ids, double* d_scores, uint32_t* d_counts, size_t how_many, const uint64_t* d_excl_flat, const uint32_t* d_excl_off,
                   const uint64_t* d_items_flat, const uint32_t* d_q_off, unsigned flags, void* stream);

/* Test aid (tests/test_gpu_class_counts.py): the k-cut's wave-wide class counts alone.  acc [n_waves * 64]: per lane sixteen 4-bit fields, field c = the lane's count of
 * class c (<= 15); out16 [n_waves * 16]: per wave the sum over its 64 lanes of every field, as the predict kernels compute it on the matrix unit.
 * HOST pointers; blocks until the result is back. */
int srn_debug_class_counts(const uint64_t* acc, size_t n_waves, uint32_t* out16, int device);

/* Test aid (tests/test_gpu_merge_pair.py): the fast kernel's merge_pair alone.  One 512-thread workgroup copies room [SRN_DEBUG_MERGE_ROOM words: the lean form's merge
 * room] into LDS, merges n_pairs (1 or 2) pairs of adjacent descending runs from the room's lower half into its upper half -- the second pair behind the first with no
 * barrier in between, as level 0 of a four-list query does -- and copies the whole room back.  pairs [n_pairs * 5] = (sa, la, lb, lg, reversed) per pair: the runs
 * in[sa, sa + la) and in[sa + la, sa + la + lb) -> out[sa, sa + la + lb), sa + la + lb < SRN_DEBUG_MERGE_ROOM / 2, by a team of 2^lg threads (6 <= lg <= 9) counted
 * from thread 0 up, or from thread 511 down where reversed != 0.  HOST pointers; blocks until the result is back. */
#define SRN_DEBUG_MERGE_ROOM 12032
int srn_debug_merge_pair(uint32_t* room, const uint32_t* pairs, size_t n_pairs, int device);

/* Test aid (tests/test_gpu_ready_record.py): the prep kernel alone.  Writes the prep records of the batch (request q = items_flat[q_off[q] .. q_off[q + 1]), oldest item
 * first) for neighbourhood cut m and sessions of up to max_len items, as a predict call on this index would, and copies them to out_records: *out_stride bytes per record
 * = an 18-word head, the 16-word launch-ready block the lean fast kernel starts from, then max_len entries of 6 words {idx, len, pre, kept, base (64-bit)}, position 0 =
 * the most recent item.  A session of 0 or of more than max_len items has no item entries (zeros).  cap_bytes < nq * stride: SRN_ERANGE, with
 * *out_stride set.  HOST pointers; blocks until the records are back. */
int srn_debug_prep_records(const srn_index_t* idx, const uint64_t* items_flat, const uint32_t* q_off, size_t nq, size_t m, size_t max_len, void* out_records, size_t cap_bytes,
                           size_t* out_stride);

/* Test aid (tests/test_gpu_general_edges.py): what the runtime decides for ONE launch of the general kernel (vmis_predict_kernel) with these parameters on this index
 * under the current SRN_* knobs -- the LDS layout and table sizes every workgroup of a plain predict call gets (no extra room in region B).  Host code only: nothing is
 * launched.  out_words [SRN_DEBUG_GEOMETRY_WORDS]:
 *   [0] masks (position-set slots)  [1] slot64  [2] bytes per session slot  [3] LDS bytes per workgroup  [4] sess_may_overflow  [5] item_may_overflow  [6] sketch_may_wrap
 *   [7] the device's LDS bytes per workgroup as the layout uses it (an input of the decision, reported so that a restatement can take it)
 *   [8..23] the kernel's configuration words in declaration order: sess_slots, item_slots, item_buckets, hot_slots, sketch_slots, sketch_shift, sum_bits, num_bits, q_cap,
 *           off_q, off_wave, off_b, off_a, region_a_bytes, no_merge, 0
 * The geometry depends on neither the batch size nor how_many, so the call takes neither.  SRN_ENODEV: the index has no device attached; SRN_ERANGE where the
 * runtime refuses the launch (k / session length too large for the layout or the accumulators). */
#define SRN_DEBUG_GEOMETRY_WORDS 24
int srn_debug_geometry(const srn_index_t* idx, size_t k, size_t m, size_t max_len, unsigned flags, uint32_t* out_words);

/* Test / experiment knobs (environment variables SRN_NO_FAST, SRN_NO_MID, SRN_NO_MASKS, SRN_NO_MERGE, SRN_HOT_SLOTS,
 * SRN_SKETCH_SLOTS, SRN_LDS_BUDGET_KB, SRN_GRID_MULT, SRN_DEBUG) force individual kernel code paths.  They are read ONCE,
 * when the library is first used -- never on the launch path; this call re-reads them (the parity tests switch paths
 * between calls).  Not for production use: make sure no predict call is in flight. */
void srn_debug_reload_knobs(void);

#ifdef __cplusplus
}
#endif
#endif
