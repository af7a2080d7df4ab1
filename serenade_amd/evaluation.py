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

Confidence intervals: evaluate(es, trials, bootstrap=B, seed=S) resamples the test sessions B times on the GPU next to every trial
(srn_evaluate_bootstrap) and adds percentile intervals and the replicate sums to each report; compare(report_a, report_b) is the paired comparison of two such
reports.  bootstrap_weights / bootstrap_model state the rule in NumPy: the device's replicate sums are the model's, bit for bit.

Segments: evaluate(es, trials, segments=spec) also says which queries a figure comes from (srn_evaluate_segments).  spec is one of
    dict(by="position", n=8)                              the state t of the query: t = 1 .. n-1 each their own segment, the last one t >= n
    dict(by="labels", labels=array, n=S, names=None)      the caller's label (0 .. S-1) per test session, in the set's order, sessions of one event included
    dict(by="target_count", bounds=[1, 10, 100])          how often the next item e_{t+1} occurs in the training data the set holds (0: the index does not know it)
    dict(by="current_count", bounds=[...])                the same for the clicked item e_t
Each report gains "segments": one dict per segment with "name", "qty_evaluations", the seven metrics @N (no Coverage) and "sums"; with bootstrap= also the
intervals and replicate arrays, paired with the totals: compare(a, b, metric, segment=i).  segment_ids_model / segment_model state the rule in NumPy.
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

    @classmethod
    def from_events(cls, index, test_events, train_item_ids):
        """The set from_tsv builds from files holding these rows, grouped and counted on the index's GPU (srn_eval_set_from_events): test_events =
        (session_ids, item_ids, times) of the test rows in file order, train_item_ids = the item column of the training rows.  NumPy arrays, or torch tensors on
        the index's GPU (read in place on the current stream); times float (rounded like the file's) or integer seconds."""
        from .ingest import _event_args, _is_torch
        device = int(index.info["device"])
        sess, items, times = test_events
        keep, (ps, pi, pt), n, flags, stream = _event_args(sess, items, times, device)
        train_on_gpu = _is_torch(train_item_ids) and train_item_ids.device.type == "cuda"
        if train_on_gpu != bool(flags & capi.EVENTS_DEVICE):
            raise ValueError("test_events and train_item_ids must all be GPU tensors or none of them")
        if train_on_gpu:
            if train_item_ids.device.index != device:
                raise ValueError("train_item_ids is not on device %d" % device)
            train = train_item_ids.contiguous()
            if train.element_size() != 8 or train.dtype.is_floating_point:
                raise TypeError("train_item_ids must be a 64-bit integer tensor")
            ptrain, n_train = train.data_ptr(), train.numel()
        else:
            train = capi.as_u64(train_item_ids.numpy() if _is_torch(train_item_ids) else train_item_ids)
            ptrain, n_train = train.ctypes.data, len(train)
        h = C.c_void_p()
        capi.check(capi.lib().srn_eval_set_from_events(index._h, C.c_void_p(ps), C.c_void_p(pi), C.c_void_p(pt), n, C.c_void_p(ptrain), n_train, flags,
                                                       None if stream is None else C.c_void_p(stream), C.byref(h)))
        del keep, train
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

    def segment_ids(self, spec):
        """The segment id of every query under a segments spec (srn_eval_segment_ids) -> uint16[n], queries in set order, states ascending."""
        seg, _, keep = _segments(spec)
        n = C.c_size_t()
        capi.check(capi.lib().srn_eval_segment_ids(self._h, C.byref(seg), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint16)
        capi.check(capi.lib().srn_eval_segment_ids(self._h, C.byref(seg), capi.ptr(out), out.shape[0], C.byref(n)))
        del keep
        return out[:n.value]


def evaluate(eval_set, trials, stream=0, bootstrap=0, seed=0, ci=0.95, segments=None):
    """One srn_evaluate call over all trials -> list of reports (dicts), in trial order.
    bootstrap=B > 0: srn_evaluate_bootstrap with B replicates of the session-clustered Poisson bootstrap at `seed`.  Each report gains
    "bootstrap": {"replicates", "seed", "ci", "weights": float64[B] (a replicate's sum of weights), "sums": {name: float64[B]} (its weighted sums, the names of
    "sums"), "empty_replicates": replicates of weight 0} and, for every metric but Coverage, "<Name>@N_ci": (lo, hi) -- the percentile interval at level `ci` over
    the replicates of non-zero weight ((0, 0) when there is none).  Reports of one seed and B on one test set are paired: compare().
    segments=spec (the module's docstring): srn_evaluate_segments -- the same reports, each with "segments": [{"name", "qty_evaluations", "<Name>@N" for the seven
    metrics but Coverage (F1score from the segment's own Precision and Recall), "sums"}], and with bootstrap= each segment's "<Name>@N_ci" and "bootstrap" too."""
    trials = list(trials)
    B = int(bootstrap)
    if B < 0 or not 0.0 < float(ci) < 1.0:
        raise ValueError("bootstrap must be >= 0 and ci inside (0, 1)")
    arr = (capi.EvalTrial * max(len(trials), 1))(*[_trial(t) for t in trials])
    res = (capi.EvalResult * max(len(trials), 1))()
    h = eval_set._h if eval_set is not None else None
    if segments is not None:
        seg, names, keep = _segments(segments)
        S, n = int(seg.segments), max(len(trials), 1)
        seg_out = (capi.EvalSegment * (n * max(S, 1)))()
        boot = capi.Bootstrap(int(seed) & _M64, B, 0) if B else None
        rep = np.zeros((n, B, capi.BOOTSTRAP_SUMS)) if B else None
        seg_rep = np.zeros((n, max(S, 1), B, capi.BOOTSTRAP_SUMS)) if B else None
        capi.check(capi.lib().srn_evaluate_segments(h, arr, len(trials), C.byref(seg), C.byref(boot) if B else None, res, seg_out, capi.ptr(rep), capi.ptr(seg_rep),
                                                    C.c_void_p(stream)))
        del keep
        out = []
        for i in range(len(trials)):
            length = arr[i].length
            r = _report(res[i], length)
            if B:
                r = _with_bootstrap(r, rep[i], length, int(boot.seed), float(ci))
            r["segments"] = [_segment_report(names[g], seg_out[i * S + g], length) for g in range(S)]
            if B:
                r["segments"] = [_with_bootstrap(sr, seg_rep[i, g], length, int(boot.seed), float(ci)) for g, sr in enumerate(r["segments"])]
            out.append(r)
        return out
    if B == 0:
        capi.check(capi.lib().srn_evaluate(h, arr, len(trials), res, C.c_void_p(stream)))
        return [_report(res[i], arr[i].length) for i in range(len(trials))]
    boot = capi.Bootstrap(int(seed) & _M64, B, 0)
    rep = np.zeros((max(len(trials), 1), B, capi.BOOTSTRAP_SUMS))
    capi.check(capi.lib().srn_evaluate_bootstrap(h, arr, len(trials), C.byref(boot), res, capi.ptr(rep), C.c_void_p(stream)))
    return [_with_bootstrap(_report(res[i], arr[i].length), rep[i], arr[i].length, int(boot.seed), float(ci)) for i in range(len(trials))]


# ---- the bootstrap: the rule in NumPy, the reports' intervals, paired comparison ----
_M64 = (1 << 64) - 1
# round(2^32 * P(Poisson(1) <= i)), i = 0..11
BOOTSTRAP_THRESHOLDS = (1580030169, 3160060337, 3950075422, 4213413783, 4279248374, 4292415292,
                        4294609778, 4294923276, 4294962463, 4294966817, 4294967253, 4294967292)
BOOTSTRAP_SUMS = ("mrr", "ndcg", "hit_rate", "popularity", "precision", "recall")   # rep[..][1..6]; rep[..][0] is the replicate's sum of weights
_BOOT_TERM_COLUMNS = [TERMS.index(n) for n in ("mrr", "ndcg", "hit", "popularity", "precision", "recall")]
_BOOT_METRICS = (("Mrr", "mrr"), ("Ndcg", "ndcg"), ("HitRate", "hit_rate"), ("Popularity", "popularity"), ("Precision", "precision"), ("Recall", "recall"))
GROUP = 256   # queries per partial sum


def _mix64(x):
    """srn_internal.h mix64 on uint64 arrays (arithmetic mod 2^64)."""
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def bootstrap_weights(seed, B, n_sessions, first_session=0):
    """w(seed, b, s) for b < B and s = first_session .. first_session + n_sessions - 1 -> uint8[B, n_sessions]: the number of thresholds T[i] <= u,
    u = mix64(mix64(seed + (b + 1) * 0x9E3779B97F4A7C15) ^ (s * 0xD1B54A32D192ED03 + 1)) >> 32.  Row b does not depend on B."""
    with np.errstate(over="ignore"):
        b = np.arange(int(B), dtype=np.uint64)
        key = _mix64(np.uint64(int(seed) & _M64) + (b + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15))
        s = np.uint64(int(first_session) & _M64) + np.arange(int(n_sessions), dtype=np.uint64)
        u = _mix64(key[:, None] ^ (s * np.uint64(0xD1B54A32D192ED03) + np.uint64(1))[None, :]) >> np.uint64(32)
    return np.searchsorted(np.array(BOOTSTRAP_THRESHOLDS, np.uint64), u, side="right").astype(np.uint8)


def bootstrap_model(terms, session_of_query, B, seed):
    """The replicate sums of srn_evaluate_bootstrap, bit for bit -> float64[B, 7].  terms: float64[n, 7] in TERMS order (EvalSet.terms), queries in set order;
    session_of_query[q]: the index of q's test session in the set's order (sessions of one event count).  Per group of 256 consecutive queries, from +0.0 in query
    order, acc = acc + w * term (the product rounded, then the sum); then the groups in order onto the total."""
    terms = np.asarray(terms, np.float64).reshape(-1, len(TERMS))
    sess = np.asarray(session_of_query, np.int64).reshape(-1)
    if len(sess) != len(terms):
        raise ValueError("one session index per query")
    total = np.zeros((int(B), 1 + len(BOOTSTRAP_SUMS)))
    if not len(terms):
        return total
    first = int(sess.min())
    w_all = bootstrap_weights(seed, B, int(sess.max()) - first + 1, first).astype(np.float64)
    cols = np.concatenate([np.ones((len(terms), 1)), terms[:, _BOOT_TERM_COLUMNS]], axis=1)
    for g0 in range(0, len(terms), GROUP):
        acc = np.zeros_like(total)
        for q in range(g0, min(g0 + GROUP, len(terms))):
            acc = acc + w_all[:, sess[q] - first, None] * cols[q][None, :]
        total = total + acc
    return total


def session_of_query(test_sessions):
    """For each query of a set in set order, the index of its test session (a session of n events gives n - 1 queries; one of a single event none, but it counts)."""
    seqs = test_sessions.values() if isinstance(test_sessions, dict) else test_sessions
    return np.array([s for s, ev in enumerate(seqs) for _ in range(1, len(ev))], np.int64)


def _f1(p, r):
    with np.errstate(invalid="ignore", divide="ignore"):
        f = 2.0 * (p * r) / (p + r)
    return np.where(np.isnan(f), 0.0, f)   # f1score.rs:27-36


def replicate_values(report, metric="Mrr"):
    """A bootstrapped report's metric per replicate -> (float64[B] -- weighted sum / weight, F1score from the replicate's Precision and Recall means; 0 where the
    weight is 0 --, bool[B]: the replicate's weight is not 0)."""
    boot = report["bootstrap"]
    w = np.asarray(boot["weights"], np.float64)
    ok = w > 0
    mean = lambda name: np.divide(np.asarray(boot["sums"][name], np.float64), w, out=np.zeros_like(w), where=ok)
    if metric == "F1score":
        return np.where(ok, _f1(mean("precision"), mean("recall")), 0.0), ok
    names = dict(_BOOT_METRICS)
    if metric not in names:
        raise ValueError("metric must be one of %s (Coverage is not resampled)" % ", ".join(list(names) + ["F1score"]))
    return mean(names[metric]), ok


def _interval(values, ci):
    if not len(values):
        return (0.0, 0.0)
    lo, hi = np.quantile(values, [(1.0 - ci) / 2.0, 1.0 - (1.0 - ci) / 2.0])
    return (float(lo), float(hi))


def _with_bootstrap(rep, sums, length, seed, ci):
    sums = np.asarray(sums, np.float64)
    rep["bootstrap"] = {"replicates": int(sums.shape[0]), "seed": seed, "ci": ci, "weights": sums[:, 0].copy(),
                        "sums": {n: sums[:, 1 + j].copy() for j, n in enumerate(BOOTSTRAP_SUMS)}, "empty_replicates": int(np.count_nonzero(sums[:, 0] == 0))}
    for name in [m for m, _ in _BOOT_METRICS] + ["F1score"]:
        v, ok = replicate_values(rep, name)
        rep["%s@%d_ci" % (name, length)] = _interval(v[ok], ci)
    return rep


def _point(report, metric):
    keys = [k for k in report if k.startswith(metric + "@") and not k.endswith("_ci")]
    if len(keys) != 1:
        raise ValueError("the report has no single %s@N" % metric)
    return float(report[keys[0]])


def compare(report_a, report_b, metric="Mrr", segment=None):
    """Paired bootstrap comparison of two reports of evaluate(..., bootstrap=B) -> {"delta": a - b of the point estimates, "ci": the percentile interval of the
    replicate-by-replicate differences (at report_a's level), "p_better": the share of replicates where a is above b, "replicates": how many entered}.
    The weights depend on (seed, replicate, the session's place in the test set) alone, so reports pair across evaluate calls and across indices on one test set;
    ValueError when seed, B or qty_evaluations differ.
    segment=i pairs segment i of both reports (evaluate(..., segments=spec, bootstrap=B)); segment=(i, j) pairs a's segment i with b's segment j, None standing for
    the whole report -- (i, None) is a segment against the total.  The weights are the same, so the replicates pair; qty_evaluations must agree only where both
    sides are the same part."""
    if segment is not None:
        sa, sb = segment if isinstance(segment, tuple) else (segment, segment)
        def pick(r, i):
            if i is None:
                return r
            if "segments" not in r:
                raise ValueError("compare(segment=) needs reports of evaluate(..., segments=spec)")
            return r["segments"][int(i)]
        ra, rb = pick(report_a, sa), pick(report_b, sb)
        if sa != sb:   # different parts of the test set: only the resampling has to be the same
            if ra.get("bootstrap") is None or rb.get("bootstrap") is None:
                raise ValueError("compare needs reports of evaluate(..., bootstrap=B)")
            rb = dict(rb, qty_evaluations=ra["qty_evaluations"])
        return compare(ra, rb, metric)
    ba, bb = report_a.get("bootstrap"), report_b.get("bootstrap")
    if ba is None or bb is None:
        raise ValueError("compare needs reports of evaluate(..., bootstrap=B)")
    if ba["seed"] != bb["seed"] or ba["replicates"] != bb["replicates"] or report_a["qty_evaluations"] != report_b["qty_evaluations"]:
        raise ValueError("the reports are not paired: seed, replicates and qty_evaluations must be equal")
    va, oka = replicate_values(report_a, metric)
    vb, okb = replicate_values(report_b, metric)
    ok = oka & okb
    d = (va - vb)[ok]
    return {"delta": _point(report_a, metric) - _point(report_b, metric), "ci": _interval(d, float(ba["ci"])),
            "p_better": float(np.count_nonzero(d > 0)) / len(d) if len(d) else 0.0, "replicates": int(len(d))}


# ---- segments: the spec, the reports, the rule in NumPy ----
_SEG_METRICS = (("Mrr", "sum_mrr"), ("Ndcg", "sum_ndcg"), ("HitRate", "sum_hit_rate"), ("Popularity", "sum_popularity"), ("Precision", "sum_precision"), ("Recall", "sum_recall"))
SEGMENT_MODES = {"position": capi.SEG_STATE, "labels": capi.SEG_LABEL, "target_count": capi.SEG_TARGET_COUNT, "current_count": capi.SEG_CURRENT_COUNT}


def _spec(spec):
    """A segments spec checked and normalised -> (by, S, labels uint16[] or None, bounds uint64[] or None, names)."""
    if not isinstance(spec, dict) or spec.get("by") not in SEGMENT_MODES:
        raise ValueError("segments: a dict with by= one of %s" % ", ".join(SEGMENT_MODES))
    by = spec["by"]
    if by == "position":
        S = int(spec["n"])
        return by, S, None, None, ["t=%d" % t for t in range(1, S)] + ["t>=%d" % S]
    if by == "labels":
        raw = np.asarray(spec["labels"])
        if raw.size and (raw.min() < 0 or raw.max() > 0xFFFF):
            raise ValueError("segments: labels must be in 0..65535")
        labels = np.ascontiguousarray(raw, dtype=np.uint16).reshape(-1)
        S = int(spec["n"])
        names = spec.get("names")
        names = ["label=%d" % g for g in range(S)] if names is None else [str(x) for x in names]
        if len(names) != S:
            raise ValueError("segments: one name per label")
        return by, S, labels, None, names
    raw = [int(b) for b in spec["bounds"]]
    if any(b < 0 or b > _M64 for b in raw):
        raise ValueError("segments: bounds must be unsigned 64-bit counts")
    bounds = np.array(raw, dtype=np.uint64).reshape(-1)
    names = ["count>=0"] if not raw else ["count<%d" % raw[0]] + ["%d<=count<%d" % (a, b) for a, b in zip(raw, raw[1:])] + ["count>=%d" % raw[-1]]
    return by, len(raw) + 1, None, bounds, names


def _segments(spec):
    """-> (capi.Segments, the segments' names, what the struct points into: keep it alive across the call)."""
    by, S, labels, bounds, names = _spec(spec)
    if not 0 <= S <= 0xFFFFFFFF:
        raise ValueError("segments: n out of range")
    seg = capi.Segments(SEGMENT_MODES[by], S, None if labels is None else labels.ctypes.data, 0 if labels is None else len(labels),
                        None if bounds is None or not len(bounds) else bounds.ctypes.data, 0)
    return seg, names, (labels, bounds)


def _segment_report(name, r, length):
    n = int(r.n_evaluations)
    rep = {"name": name, "qty_evaluations": n}
    for metric, field in _SEG_METRICS:
        rep["%s@%d" % (metric, length)] = float(getattr(r, field)) / n if n else 0.0
    rep["F1score@%d" % length] = float(_f1(np.float64(rep["Precision@%d" % length]), np.float64(rep["Recall@%d" % length])))
    rep["sums"] = {field[4:]: float(getattr(r, field)) for _, field in _SEG_METRICS}
    return rep


def segment_ids_model(test_sessions, spec, counts=None):
    """The segment id of every query, in set order (sessions in order, states ascending) -> uint16[n]; the rule of srn_evaluate_segments in Python, without a GPU.
    counts: {item id: training count} of what the set holds -- the count modes read it, an id it does not hold counts 0."""
    by, S, labels, bounds, _ = _spec(spec)
    if S < 1:
        raise ValueError("segments: at least one segment")
    seqs = list(test_sessions.values() if isinstance(test_sessions, dict) else test_sessions)
    if by == "labels" and len(labels) != len(seqs):
        raise ValueError("segments: one label per test session")
    if by == "labels" and len(labels) and int(labels.max()) >= S:
        raise ValueError("segments: a label is not below n")
    if bounds is not None and any(int(a) >= int(b) for a, b in zip(bounds, bounds[1:])):
        raise ValueError("segments: bounds must be strictly ascending")
    counts = {} if counts is None else counts
    out = []
    for s, ev in enumerate(seqs):
        ev = list(ev)
        for t in range(1, len(ev)):
            if by == "position":
                out.append(min(t, S) - 1)
            elif by == "labels":
                out.append(int(labels[s]))
            else:
                c = int(counts.get(int(ev[t] if by == "target_count" else ev[t - 1]), 0))
                out.append(sum(1 for b in bounds if int(b) <= c))
    return np.array(out, np.uint16)


def segment_model(terms, ids, S, session_of_query=None, B=0, seed=0):
    """The sums of srn_evaluate_segments, bit for bit.  terms: float64[n, 7] in TERMS order (EvalSet.terms); ids[q]: the query's segment, below S.
    -> float64[S, 7]: per segment the number of queries, then the sums of mrr, ndcg, hit_rate, popularity, precision, recall -- per group of 256 consecutive queries
    from +0.0 in query order over the group's queries of the segment, acc = acc + term, then the groups in order onto the total.
    B > 0 (with session_of_query, as bootstrap_model takes it): -> (that, float64[S, B, 7]): bootstrap_model's seven sums restricted to each segment's queries, the
    same weights and the same order rule."""
    terms = np.asarray(terms, np.float64).reshape(-1, len(TERMS))
    ids = np.asarray(ids, np.int64).reshape(-1)
    S, B = int(S), int(B)
    if len(ids) != len(terms) or (len(ids) and (ids.min() < 0 or ids.max() >= S)):
        raise ValueError("one segment id below S per query")
    cols = np.concatenate([np.ones((len(terms), 1)), terms[:, _BOOT_TERM_COLUMNS]], axis=1)
    total = np.zeros((S, 1 + len(BOOTSTRAP_SUMS)))
    rep = np.zeros((S, B, 1 + len(BOOTSTRAP_SUMS)))
    if B:
        sess = np.asarray(session_of_query, np.int64).reshape(-1)
        if len(sess) != len(terms):
            raise ValueError("one session index per query")
        first = int(sess.min()) if len(sess) else 0
        w_all = bootstrap_weights(seed, B, int(sess.max()) - first + 1, first).astype(np.float64) if len(sess) else np.zeros((B, 0))
    for g0 in range(0, len(terms), GROUP):
        acc, racc = np.zeros_like(total), np.zeros_like(rep)
        for q in range(g0, min(g0 + GROUP, len(terms))):
            acc[ids[q]] = acc[ids[q]] + cols[q]
            if B:
                racc[ids[q]] = racc[ids[q]] + w_all[:, sess[q] - first, None] * cols[q][None, :]
        total, rep = total + acc, rep + racc
    return (total, rep) if B else total
