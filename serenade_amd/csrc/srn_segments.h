// Trials evaluated by segment (include/serenade_hip.h srn_evaluate_segments): what srn_eval.hip hands to srn_segments.hip.
// A segmentation maps every query (s, t) of an evaluation set to an id in 0..S-1 from the set and the rule alone; per (trial, segment) the call keeps the number of
// queries and the six sums of srn_eval_result_t, and with a bootstrap the seven sums of every replicate, under the order rule of 10.2 restricted to the segment.
#pragma once
#include <cstddef>
#include <cstdint>

#include "srn_internal.h"

namespace srn {

static constexpr uint32_t kSegSums = 7;   // per (trial, segment): the queries, then mrr, ndcg, hit_rate, popularity, precision, recall
static_assert(kSegSums == SRN_BOOTSTRAP_SUMS, "a segment's sums are a replicate's: the count in the weights' place");

struct SegSet {   // what the id kernel reads of the set and of its index's dictionary
    const uint64_t* items; const uint64_t* sess_off; const double* freq;
    const IdSlot* id_table; uint32_t id_mask;
};
struct SegRule {   // srn_segments_t on the device: the labels uploaded, the bounds by value
    uint32_t mode, S;
    const uint16_t* labels;
    uint64_t bounds[SRN_MAX_SEGMENTS - 1];
};
// byte offsets of a call's regions in one grow-only buffer (256-aligned): the sessions' labels, a chunk's ids, the totals [trial][segment][7] and the partials of a
// chunk's groups [group][7][segment]; with a bootstrap the replicate totals [trial][segment][replicate][7] and one pass's partials
struct SegBuffers { size_t labels = 0, ids = 0, totals = 0, part = 0, boot_totals = 0, boot_part = 0, bytes = 0; };
SegBuffers seg_buffers(size_t n_sessions, uint64_t max_chunk, size_t n_trials, uint32_t S, uint32_t replicates);

// all three only enqueue.  ss: a chunk's (session, state) pairs; terms: its [nq][8] term buffer
int seg_ids(const SegSet& set, const SegRule& rule, const void* ss, uint32_t nq, uint16_t* ids, void* stream);
int seg_chunk(const double* terms, const uint16_t* ids, uint32_t nq, uint32_t S, double* part, double* totals, void* stream);
int seg_boot_chunk(const double* terms, const void* ss, const uint16_t* ids, uint32_t nq, uint32_t S, const srn_bootstrap_t& boot, double* part, double* totals, void* stream);

}  // namespace srn
