"""Evaluation trials under the serving rules (SRN_FLAG_EVAL_HANDLER, SRN_FLAG_EXCLUDE_SESSION, SRN_FLAG_EXCLUDE_SEEN and the history window of
srn_eval_trial_t): per-query terms against host restatements of the reference's metrics over predict_batch rows of evaluation.serving_queries' queries and lists,
and against the rows recommend_batch serves to one visitor per test session."""
import ctypes as C
import math
import os
from collections import Counter

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, evaluation, hpo, serving, synth
from helpers import GOLDEN, flatten

pytestmark = pytest.mark.gpu

K, M, HOW_MANY, LENGTH = 100, 500, 21, 20
NDCG_W = [1.0 if i == 0 else 1.0 / math.log2(i + 1.0) for i in range(capi.MAX_HOW_MANY)]   # ndcg.rs:13-27
RAW = ("n_evaluations", "mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score", "sum_mrr", "sum_ndcg", "sum_hit_rate",
       "sum_popularity", "sum_precision", "sum_recall", "covered_items", "unique_training_items")
UNKNOWN = 7   # an id the index does not know (synthetic item ids start far above it)

FLAG_SETS = {"session": dict(exclude_session=True), "seen": dict(exclude_seen=True), "seen+handler": dict(exclude_seen=True, handler_sessions=True),
             "handler": dict(handler_sessions=True), "seen+handler+fill": dict(exclude_seen=True, handler_sessions=True, fill=True)}


def host_terms(recs, nxt, length, freq, max_freq):
    """One query's terms, added in rank order one at a time (src/metrics/mrr.rs:24-33, hitrate.rs:24-33, ndcg.rs:42-56, precision.rs:31-43, recall.rs:31-44,
    popularity.rs:41-58)."""
    top = [int(x) for x in recs[:length]]
    nxt = [int(x) for x in nxt]
    mrr = hit = 0.0
    if nxt[0] in top:
        mrr, hit = 1.0 / (top.index(nxt[0]) + 1), 1.0
    nset = set(nxt)
    num = 0.0
    for i, x in enumerate(top):
        if x in nset:
            num += NDCG_W[i]
    den = 0.0
    for i in range(min(len(nxt), length)):
        den += NDCG_W[i]
    inter = len(nset & set(top))
    pop = 0.0
    for x in top:
        pop += freq.get(x, 0) / float(max_freq)
    return [mrr, hit, num / den, float(inter), inter / float(length), inter / float(len(nxt)), pop / len(top) if top else 0.0]


def assert_terms(got, rep, rows, counts, nexts, freq):
    """got / rep = EvalSet.terms(trial); rows[q, :counts[q]] the expected recommendations of query q."""
    assert got.shape == (len(nexts), 7)
    max_freq = max(freq.values())
    covered = set()
    for q, nxt in enumerate(nexts):
        recs = rows[q, :counts[q]].tolist()
        want = host_terms(recs, nxt, LENGTH, freq, max_freq)
        assert got[q, :6].tolist() == want[:6], (q, got[q].tolist(), want)
        assert abs(got[q, 6] - want[6]) <= 1e-14, (q, got[q, 6], want[6])
        covered.update(recs[:LENGTH])
    assert rep["covered_items"] == len(covered)
    assert rep["qty_evaluations"] == len(nexts)


def expected_rows(index, qs, excluding, fill):
    flat, off = flatten([q for q, _, _ in qs])
    if not excluding and not fill:
        ids, sc, cnt = sa.predict_batch(index, sa.CSR(flat, off), K, M, HOW_MANY)
    else:
        ids, sc, cnt = sa.predict_batch(index, sa.CSR(flat, off), K, M, HOW_MANY, exclude=[x for _, x, _ in qs] if excluding else None, fill=fill)
    return ids, cnt, sc


def raw(r):
    return tuple(getattr(r, f) for f in RAW)


def evaluate_raw(es, trials):
    arr = (capi.EvalTrial * len(trials))(*[evaluation._trial(t) for t in trials])
    res = (capi.EvalResult * len(trials))()
    capi.check(capi.lib().srn_evaluate(es._h, arr, len(trials), res, None))
    return [raw(r) for r in res]


def trial(W, H=0, **kw):
    return dict(dict(k=K, m=M, max_items_in_session=W, how_many=HOW_MANY, length=LENGTH, history=H), **kw)


def make_sessions(freq, n_items):
    """synth.test_sessions(250) and the hand-made sessions: the index's two most popular items a, b and a third one c in runs of repeats (non-empty rows), one
    session of about 70 items with runs, one with an id the index does not know."""
    (a, _), (b, _), (c, _) = freq.most_common(3)
    sessions = synth.test_sessions(250, n_items, seed=synth.SEED + 11)
    rng = np.random.default_rng(23)
    pool = [x for x, _ in freq.most_common(40)]
    long = []
    while len(long) < 70:
        long += [int(rng.choice(pool))] * int(rng.integers(1, 5))
    assert UNKNOWN not in freq
    hand = [[a, a, a, a], [a, b, b], [a, b, b, a, a, c], [a, a], [b, a, a, a, a, a, c, b], long, [a, UNKNOWN, UNKNOWN, b, a, a]]
    for j, s in enumerate(hand):
        sessions[1_000_000 + j] = s
    return sessions, (a, b, c)


@pytest.fixture(scope="module")
def tiny():
    inter, n_items, _, _, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, M, 34, idfw, device=0)
    freq = Counter(int(x) for x in items)
    sessions, abc = make_sessions(freq, n_items)
    es = evaluation.EvalSet(index, sessions, items)
    plain = {}   # W -> rows of the raw prefixes: computed once, shared by the cases
    yield dict(index=index, sessions=sessions, freq=freq, es=es, items=items, n_items=n_items, abc=abc, plain=plain)
    es.close()


def plain_rows(tiny, W):
    if W not in tiny["plain"]:
        tiny["plain"][W] = expected_rows(tiny["index"], evaluation.serving_queries(tiny["sessions"], W), False, False)
    return tiny["plain"][W]


# Queries (of 960) whose row the rule changes against the plain trial of the same window, counted on the CPU with the oracle (oracle.OracleIndex.predict_batch,
# canonical form, at how_many + the longest list, then serving.filter_rows) when this test was written:
#   (W, H)   session   seen   seen+handler   handler
#   (1, 0)      0        0         0            0     -- a window of one item excludes the item itself, which no row holds, and the query is the last click either way
#   (2, 0)    468      468       513           45
#   (2, 2)    468      468       513           45
#   (2, 8)    468      618       622           45
#   (5, 8)    632      639       639           67
# (all but one of each differ within the first 20 entries, which the metrics read); the plain rows of [a, b] -- state 2 of [a, b, b] -- recommend a.
# 31..94 of the plain rows are shorter than how_many, so SRN_FLAG_FILL has rows to fill.
@pytest.mark.parametrize("flags", list(FLAG_SETS))
@pytest.mark.parametrize("W,H", [(1, 0), (2, 0), (2, 2), (2, 8), (5, 8)])
def test_per_query_terms_match_the_host(tiny, W, H, flags):
    kw = FLAG_SETS[flags]
    index, es = tiny["index"], tiny["es"]
    fill = kw.get("fill", False)
    excluding = kw.get("exclude_session", False) or kw.get("exclude_seen", False)
    qs = evaluation.serving_queries(tiny["sessions"], W, history=H, **{k: v for k, v in kw.items() if k != "fill"})
    if fill:
        index.set_fallback_popular(64)
    try:
        rows, cnt, sc = expected_rows(index, qs, excluding, fill)
        got, rep = es.terms(trial(W, H, **kw))
    finally:
        if fill:
            index.clear_fallback()
    assert_terms(got, rep, rows, cnt, [n for _, _, n in qs], tiny["freq"])
    if W > 1:   # no vacuous pass: the rule changes some query's row against the plain trial
        p_rows, p_cnt, _ = plain_rows(tiny, W)
        changed = sum(1 for q in range(len(qs)) if cnt[q] != p_cnt[q] or rows[q, :cnt[q]].tolist() != p_rows[q, :p_cnt[q]].tolist())
        assert changed >= 1, (W, H, flags)
        plain_terms, _ = es.terms(trial(W))
        assert not np.array_equal(plain_terms, got)
    if fill:   # ... and some row was filled (filled entries score -inf)
        assert any(np.isinf(sc[q, :cnt[q]]).any() for q in range(len(qs)))


def test_a_b_b_is_changed_by_exclusion_and_by_the_handler_rule(tiny):
    a, b, _ = tiny["abc"]
    index = tiny["index"]
    ids, _, cnt = sa.predict_batch(index, [[a, b]], K, M, HOW_MANY)
    assert a in ids[0, :cnt[0]].tolist()   # the plain row of [a, b] recommends a: excluding the session's items changes it
    sessions = {1: [a, b, b], 2: [a, b, b, a]}
    es = evaluation.EvalSet(index, sessions, tiny["items"])
    raw_q = evaluation.serving_queries(sessions, 2, exclude_session=True)
    han_q = evaluation.serving_queries(sessions, 2, exclude_session=True, handler_sessions=True)
    assert raw_q[1][0] == [a, b] and raw_q[4][0] == [b, b] and han_q[4][0] == [a, b]   # (state 3 of [a, b, b, a]: the repeated click is no click for the handler)
    for qs, kw in ((raw_q, dict(exclude_session=True)), (han_q, dict(exclude_session=True, handler_sessions=True))):
        rows, c, _ = expected_rows(index, qs, True, False)
        assert a not in rows[1, :c[1]].tolist()
        got, rep = es.terms(trial(2, **kw))
        assert_terms(got, rep, rows, c, [n for _, _, n in qs], tiny["freq"])
    es.close()


@pytest.mark.parametrize("fill", [False, True])
@pytest.mark.parametrize("W,H", [(2, 0), (2, 8)])
def test_handler_trial_scores_what_recommend_batch_serves(tiny, W, H, fill):
    index, es, sessions = tiny["index"], tiny["es"], tiny["sessions"]
    seqs = list(sessions.values())
    hi = np.concatenate([np.full(len(s), 77, np.uint64) for s in seqs])
    lo = np.concatenate([np.full(len(s), i + 1, np.uint64) for i, s in enumerate(seqs)])
    clicks = np.array([x for s in seqs for x in s], np.uint64)
    last = np.zeros(len(clicks), bool)
    last[np.cumsum([len(s) for s in seqs]) - 1] = True
    store = serving.DeviceSessionStore(index, capacity=4096, items_cap=16, history=H)
    if fill:
        index.set_fallback_popular(64)
    try:
        ids, cnt = serving.recommend_batch(index, store, (hi, lo), clicks, k=K, m=M, how_many=HOW_MANY, max_items_in_session=W, now=1_700_000_000,
                                           exclude_seen=True, fill=fill)
        got, rep = es.terms(trial(W, H, exclude_seen=True, handler_sessions=True, fill=fill))
    finally:
        if fill:
            index.clear_fallback()
        store.close()
    nexts = [s[t:] for s in seqs for t in range(1, len(s))]
    assert_terms(got, rep, ids[~last], cnt[~last], nexts, tiny["freq"])
    # the handler flag acts: some query of the raw mode is another one
    han = evaluation.serving_queries(sessions, W, history=H, handler_sessions=True, exclude_seen=True)
    raw_q = evaluation.serving_queries(sessions, W, history=H, exclude_seen=True)
    assert sum(1 for x, y in zip(han, raw_q) if x[:2] != y[:2]) >= 1
    raw_terms, _ = es.terms(trial(W, H, exclude_seen=True, fill=False))
    assert fill or not np.array_equal(raw_terms, got)


def test_bits_do_not_depend_on_packaging(tiny):
    es = tiny["es"]
    serve = [trial(2, 8, exclude_seen=True, handler_sessions=True), trial(5, 0, exclude_session=True), trial(2, 0, handler_sessions=True)]
    plain = [trial(1), trial(2, how_many=20), trial(5, business_logic=True)]
    alone = [evaluate_raw(es, [t])[0] for t in serve]
    assert alone[0][0] > 2 * 256   # several chunks of 256 queries
    plain_alone = evaluate_raw(es, plain)
    mixed = evaluate_raw(es, [plain[0], serve[0], plain[1], serve[1], serve[2], plain[2]])
    assert [mixed[1], mixed[3], mixed[4]] == alone
    assert [mixed[0], mixed[2], mixed[5]] == plain_alone
    chunked = evaluate_raw(es, [dict(t, max_chunk_queries=256) for t in serve])   # sessions are cut across chunks
    assert chunked == alone
    assert evaluate_raw(es, serve) == alone
    # history without SRN_FLAG_EXCLUDE_SEEN changes nothing
    assert evaluate_raw(es, [trial(2, 8)]) == evaluate_raw(es, [trial(2)])
    assert evaluate_raw(es, [trial(2, 8, handler_sessions=True)])[0] == alone[2]


def test_checks_run_before_any_launch(tiny):
    index, es = tiny["index"], tiny["es"]
    good = trial(5, 8, exclude_seen=True, handler_sessions=True)
    before = evaluate_raw(es, [good])
    index.clear_fallback()
    for bad, code in ([(trial(5, h, exclude_seen=True), capi.SRN_ERANGE) for h in (1, 4)] + [(trial(5, 4), capi.SRN_ERANGE)] +
                      [(trial(5, 8, exclude_seen=True, how_many=capi.MAX_HOW_MANY - 7), capi.SRN_ERANGE),
                       (trial(5, 0, exclude_session=True, how_many=capi.MAX_HOW_MANY - 4), capi.SRN_ERANGE),
                       (trial(5, 8, exclude_seen=True, handler_sessions=True, fill=True), capi.SRN_ESTATE)]):
        for trials in ([bad], [good, bad]):   # ... for every trial of the call
            with pytest.raises(capi.SerenadeError) as e:
                evaluation.evaluate(es, trials)
            assert e.value.code == code, (bad, e.value)
    assert evaluate_raw(es, [trial(5, 8, exclude_seen=True, how_many=capi.MAX_HOW_MANY - 8, length=20)])[0][0] == before[0][0]   # the widest trial that fits
    assert evaluate_raw(es, [good]) == before


def _example(tmp_path):
    g = np.load(os.path.join(GOLDEN, "example_golden.npz"))
    off, items, ts = g["sess_off"].astype(np.int64), g["items"], g["ts"]
    train, test = tmp_path / "train.txt", tmp_path / "test.txt"
    with open(train, "w") as f:
        f.write("SessionId\tItemId\tTime\n")
        for s in range(len(ts)):
            for it in items[off[s]:off[s + 1]]:
                f.write("%d\t%d\t%d.0\n" % (s + 1, it, ts[s]))
        f.write("%d\t1\t1.0\n" % (len(ts) + 1))
    with open(test, "w") as f:
        f.write("SessionId\tItemId\tTime\n")
        for s, it, t in g["test_rows"]:
            f.write("%d\t%d\t%d.0\n" % (s, it, t))
    return str(train), str(test)


def test_search_applies_the_serving_rules_to_every_trial(tmp_path):
    train, test = _example(tmp_path)
    trials = [dict(m=500, k=50, max_items_in_session=2, idf_weighting=1), dict(m=500, k=100, max_items_in_session=1, idf_weighting=1),
              dict(m=100, k=50, max_items_in_session=5, idf_weighting=1)]
    rules = dict(exclude_seen=True, history=8, handler_sessions=True)
    res = hpo.search(train, test, trials, business_logic=True, **rules)
    plain = hpo.search(train, test, trials, business_logic=True)
    assert len(res["records"]) == 3
    index = sa.VMISIndex.new_from_csv(train, 500, 1.0)
    es = evaluation.EvalSet.from_tsv(index, test, train)
    for rec, p, t in zip(res["records"], plain["records"], trials):
        d = dict(k=t["k"], m=t["m"], max_items_in_session=t["max_items_in_session"], business_logic=True, **rules)
        rep = evaluation.evaluate(es, [d])[0]
        assert rep["qty_evaluations"] == 931
        for key in rep:
            if not key.startswith("ms_"):
                assert rec["report"][key] == rep[key], (t, key)
        assert rec["MRR@20"] == rep["Mrr@20"]
        assert rec["report"]["sums"] != p["report"]["sums"]   # the rules reach every trial
    es.close()
    index.close()
