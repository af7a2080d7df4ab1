"""Shared by the segment tests: hand-written sessions for the rule, the trial and the specs the GPU tests run, and the C call with raw arrays."""
import ctypes as C

import numpy as np

from serenade_amd import capi, evaluation

RAW = ("n_evaluations", "mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score", "sum_mrr", "sum_ndcg", "sum_hit_rate",
       "sum_popularity", "sum_precision", "sum_recall", "covered_items", "unique_training_items")   # srn_eval_result_t without ms_predict, ms_eval
SEG_FIELDS = ("n_evaluations", "sum_mrr", "sum_ndcg", "sum_hit_rate", "sum_popularity", "sum_precision", "sum_recall")   # srn_eval_segment_t: segment_model's columns
SEED = 0x5EEDC0FFEE
WINDOWS = (1, 2, 5)

# sessions for the rule by hand: one of a single event between the others, a repeated click, items the counts do not hold (900, 901)
HAND = {3: [10, 11, 12, 13, 14], 5: [20], 8: [11, 11, 900, 10], 9: [901, 12]}
HAND_COUNTS = {10: 1, 11: 10, 12: 100, 13: 9, 14: 99, 20: 5}


def trial_of(window, **kw):
    return dict(dict(k=100, m=500, max_items_in_session=window, how_many=21, length=20), **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_sessions(ordinary, pool, rng, unknown_from=None):
    """{index: events}: the ordinary sessions in order, a session of one event before every third of them, and a long session across every multiple of 256 queries
    (the shape of the bootstrap tests' set).  unknown_from: every seventh event of the long sessions and every eleventh of the ordinary ones becomes an id of its own
    from there upwards -- items no index built from the pool knows."""
    sessions, nq, fresh = {}, 0, [unknown_from]

    def spoil(ev, every):
        ev = [int(x) for x in ev]
        if unknown_from is not None:
            for j in range(every - 1, len(ev), every):
                ev[j] = fresh[0]
                fresh[0] += 1
        return ev
    for n, ev in enumerate(ordinary):
        if n % 3 == 0:
            sessions[len(sessions)] = [int(rng.choice(pool))]
        to_boundary = 256 - nq % 256
        if to_boundary <= 40:
            sessions[len(sessions)] = spoil(rng.choice(pool, size=to_boundary + 25), 7)
            nq += to_boundary + 24
        sessions[len(sessions)] = spoil(ev, 11) if n % 2 else [int(x) for x in ev]
        nq += len(ev) - 1
    return sessions


def segments_struct(spec):
    """-> (capi.Segments, S, what it points into)."""
    seg, _, keep = evaluation._segments(spec)
    return seg, int(seg.segments), keep


def run_segments(es, trials, spec, B=0, seed=SEED):
    """srn_evaluate_segments -> (the results' fields without the milliseconds, seg_out float64[n_trials][S][7] in SEG_FIELDS order, rep[n_trials][B][7] or None,
    seg_rep[n_trials][S][B][7] or None).  The output arrays start as NaN / all ones: what comes back was written."""
    seg, S, keep = segments_struct(spec)
    n = len(trials)
    arr = (capi.EvalTrial * n)(*[evaluation._trial(t) for t in trials])
    res = (capi.EvalResult * n)()
    seg_out = (capi.EvalSegment * (n * S))()
    C.memset(seg_out, 0xFF, C.sizeof(seg_out))
    rep = np.full((n, B, 7), np.nan) if B else None
    seg_rep = np.full((n, S, B, 7), np.nan) if B else None
    boot = capi.Bootstrap(seed, B, 0)
    capi.check(capi.lib().srn_evaluate_segments(es._h, arr, n, C.byref(seg), C.byref(boot) if B else None, res, seg_out, capi.ptr(rep), capi.ptr(seg_rep), None))
    del keep
    out = np.array([[float(getattr(seg_out[i], f)) for f in SEG_FIELDS] for i in range(n * S)]).reshape(n, S, 7)
    return [tuple(getattr(r, f) for f in RAW) for r in res], out, rep, seg_rep
