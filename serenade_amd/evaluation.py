"""Offline evaluation on the GPU: the reference's evaluation loop (src/bin/evaluator.rs:46-76, src/objective.rs:8-52) over the C ABI's
srn_eval_set_* / srn_evaluate.

    es = EvalSet(index, test_sessions, training_items)      # or EvalSet.from_tsv(index, "test.txt", "train.txt")
    evaluate(es, [dict(k=50, m=500, max_items_in_session=2), ...])   # -> one report per trial

A trial is a dict: k, m, max_items_in_session (the window), how_many (default 20), length (the metrics' @N, default 20),
business_logic (default False), fill (default False: with it short rows are filled from the index's fallback ranking before they are scored), max_chunk_queries (default 0: the library's chunk size; results do not depend on it),
and the serving rules, all off by default: handler_sessions (the sessions /v1/recommend builds: a click that repeats the one before it is dropped),
exclude_session (a query's own items are left out of its row), exclude_seen with history (the row leaves out the last `history` items the visitor has seen -- the
session window with history=0; history without exclude_seen changes no row).  handler_sessions + exclude_seen scores the rows recommend_batch(..., exclude_seen=True)
serves; serving_queries() states the queries and lists of such a trial in Python.
A report holds the evaluator's report line under its own names (qty_evaluations, Mrr@20, ..., F1score@20), the raw sums and the
device milliseconds of predict and of the evaluation kernels.
"""
import ctypes as C

import numpy as np

from . import capi
from .vmisknn import CSR

METRICS = ("Mrr", "Ndcg", "HitRate", "Popularity", "Precision", "Coverage", "Recall", "F1score")   # evaluation_reporter.rs order
_FIELDS = ("mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score")
TERMS = ("mrr", "hit", "ndcg", "intersection", "precision", "recall", "popularity")   # srn_debug_eval_terms, per query


def _trial(t):
    out = capi.EvalTrial()
    out.k, out.m = int(t["k"]), int(t["m"])
    out.how_many = int(t.get("how_many", 20))
    out.max_items_in_session = int(t["max_items_in_session"])
    out.length = int(t.get("length", 20))
    out.flags = (capi.FLAG_BUSINESS_LOGIC if t.get("business_logic", False) else 0) | (capi.FLAG_FILL if t.get("fill", False) else 0) | \
                (capi.FLAG_EXCLUDE_SESSION if t.get("exclude_session", False) else 0) | (capi.FLAG_EXCLUDE_SEEN if t.get("exclude_seen", False) else 0) | \
                (capi.FLAG_EVAL_HANDLER if t.get("handler_sessions", False) else 0)
    out.max_chunk_queries = int(t.get("max_chunk_queries", 0))
    out.history = int(t.get("history", 0))
    return out


def serving_queries(test_sessions, max_items_in_session, history=0, handler_sessions=False, exclude_session=False, exclude_seen=False):
    """The queries of a trial under the serving rules, in set order (sessions in order, states ascending) -> [(query, exclusion_list, next_items)]; the closed form of
    DESIGN.md 10, the counterpart of serving.filter_rows / fill_rows.  For state t of a session e_1..e_n: c = e_1..e_t, with handler_sessions without every click
    equal to the one before it; query = the last max_items_in_session items of c; the list is empty without exclude_session / exclude_seen, the query's items with
    exclude_session alone, and with exclude_seen the last `history` items of c (the last max_items_in_session with history=0); next_items = e_{t+1}..e_n, raw.
    It needs no GPU."""
    W, H = int(max_items_in_session), int(history)
    if W < 1 or (H and H < W):
        raise ValueError("max_items_in_session must be > 0 and history 0 or >= max_items_in_session")
    seqs = test_sessions.values() if isinstance(test_sessions, dict) else test_sessions
    out = []
    for ev in seqs:
        ev = list(ev)
        for t in range(1, len(ev)):
            c = [x for j, x in enumerate(ev[:t]) if not (handler_sessions and j and x == ev[j - 1])]
            query = c[-W:]
            lst = c[-(H or W):] if exclude_seen else (list(query) if exclude_session else [])
            out.append((query, lst, ev[t:]))
    return out


def _report(r, length):
    rep = {"qty_evaluations": int(r.n_evaluations)}
    for name, field in zip(METRICS, _FIELDS):
        rep["%s@%d" % (name, length)] = float(getattr(r, field))
    rep["sums"] = {n: float(getattr(r, "sum_" + n)) for n in ("mrr", "ndcg", "hit_rate", "popularity", "precision", "recall")}
    rep["covered_items"], rep["unique_training_items"] = int(r.covered_items), int(r.unique_training_items)
    rep["ms_predict"], rep["ms_eval"] = float(r.ms_predict), float(r.ms_eval)
    return rep


class EvalSet:
    """Test sessions and training-item frequencies resident on the index's GPU (srn_eval_set_t).  The index must outlive the set."""

    def __init__(self, index, test_sessions, training_items, _handle=None):
        self._index = index
        self._h = _handle
        if _handle is not None:
            return
        if isinstance(test_sessions, CSR):
            items = capi.as_u64(test_sessions.items_flat)
            off = capi.as_u64(test_sessions.q_off)
        else:
            seqs = list(test_sessions.values()) if isinstance(test_sessions, dict) else list(test_sessions)
            off = np.zeros(len(seqs) + 1, np.uint64)
            off[1:] = np.cumsum([len(s) for s in seqs])
            items = np.fromiter((x for s in seqs for x in s), dtype=np.uint64, count=int(off[-1]))
        if len(off) < 1 or int(off[0]) != 0 or int(off[-1]) != len(items):
            raise ValueError("test sessions: offsets must start at 0 and end at the number of items")
        ids, counts = np.unique(capi.as_u64(training_items), return_counts=True)
        ids, counts = capi.as_u64(ids), capi.as_u64(counts)
        h = C.c_void_p()
        capi.check(capi.lib().srn_eval_set_create(index._h, capi.ptr(items), capi.ptr(off), len(off) - 1, capi.ptr(ids), capi.ptr(counts), len(ids), C.byref(h)))
        self._h = h

    @classmethod
    def from_tsv(cls, index, test_path, train_path):
        """read_test_data_evolving(test_path) and the item column of train_path (src/io.rs:13-59)."""
        h = C.c_void_p()
        capi.check(capi.lib().srn_eval_set_from_tsv(index._h, str(test_path).encode(), str(train_path).encode(), C.byref(h)))
        return cls(index, None, None, _handle=h)

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:   # (None at interpreter shutdown)
            capi.lib().srn_eval_set_free(self._h)
            self._h = None

    __del__ = close

    def terms(self, trial):
        """Per-query terms of one trial (test aid): (float64[n, 7] in TERMS order, report).  Queries in set order, states ascending."""
        t, n, r = _trial(trial), C.c_size_t(), capi.EvalResult()
        capi.check(capi.lib().srn_debug_eval_terms(self._h, C.byref(t), None, 0, C.byref(n), None))
        out = np.zeros((max(n.value, 1), 7))
        capi.check(capi.lib().srn_debug_eval_terms(self._h, C.byref(t), capi.ptr(out), out.shape[0], C.byref(n), C.byref(r)))
        return out[:n.value], _report(r, t.length)


def evaluate(eval_set, trials, stream=0):
    """One srn_evaluate call over all trials -> list of reports (dicts), in trial order."""
    trials = list(trials)
    arr = (capi.EvalTrial * max(len(trials), 1))(*[_trial(t) for t in trials])
    res = (capi.EvalResult * max(len(trials), 1))()
    capi.check(capi.lib().srn_evaluate(eval_set._h if eval_set is not None else None, arr, len(trials), res, C.c_void_p(stream)))
    return [_report(res[i], arr[i].length) for i in range(len(trials))]
