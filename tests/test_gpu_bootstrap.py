"""Bootstrap confidence intervals on the GPU (srn_evaluate_bootstrap) against the rule in NumPy (evaluation.bootstrap_model over the trial's
per-query terms): the replicate sums bit for bit, whatever the chunking, the company of other trials or B; the reports' intervals, compare() and the search."""
import ctypes as C
import os

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, evaluation, hpo, synth
from helpers import GOLDEN

pytestmark = pytest.mark.gpu

RAW = ("n_evaluations", "mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score", "sum_mrr", "sum_ndcg", "sum_hit_rate",
       "sum_popularity", "sum_precision", "sum_recall", "covered_items", "unique_training_items")   # srn_eval_result_t without ms_predict, ms_eval
SEED = 0x5EEDC0FFEE
WINDOWS = (1, 2, 5)


def trial_of(window, **kw):
    return dict(dict(k=100, m=500, max_items_in_session=window, how_many=21, length=20), **kw)


def run(es, trials, B, seed=SEED):
    """srn_evaluate_bootstrap -> (the results' fields without the milliseconds, rep[n_trials][B][7])."""
    arr = (capi.EvalTrial * len(trials))(*[evaluation._trial(t) for t in trials])
    res = (capi.EvalResult * len(trials))()
    rep = np.full((len(trials), B, 7), np.nan)
    boot = capi.Bootstrap(seed, B, 0)
    capi.check(capi.lib().srn_evaluate_bootstrap(es._h, arr, len(trials), C.byref(boot), res, capi.ptr(rep), None))
    return [tuple(getattr(r, f) for f in RAW) for r in res], rep


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_sessions(ordinary, pool, rng):
    """{index: events}: the ordinary sessions in order, a session of one event before every third of them, and a long session across every multiple of 256 queries."""
    sessions, nq = {}, 0
    for n, ev in enumerate(ordinary):
        if n % 3 == 0:
            sessions[len(sessions)] = [int(rng.choice(pool))]
        to_boundary = 256 - nq % 256
        if to_boundary <= 40:
            sessions[len(sessions)] = [int(x) for x in rng.choice(pool, size=to_boundary + 25)]
            nq += to_boundary + 24
        sessions[len(sessions)] = list(ev)
        nq += len(ev) - 1
    return sessions


@pytest.fixture(scope="module")
def tiny():
    inter, n_items, k, m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0)
    index.set_fallback_popular(64)
    # ordinary sessions with sessions of one event between them (no query, but an index of their own), and long ones that straddle the groups of 256 queries
    rng = np.random.default_rng(21)
    pool = np.unique(items)[:3000]
    sessions = make_sessions(synth.test_sessions(330, n_items, seed=synth.SEED + 31).values(), pool, rng)
    sess = evaluation.session_of_query(sessions)
    nq = len(sess)
    assert nq > 3 * 256 and nq % 256 != 0
    assert all(sess[g - 1] == sess[g] for g in range(256, nq, 256)),"a session straddles every boundary between groups"
    assert len(np.unique(sess)) < int(sess.max()) + 1 - 50, "sessions of one event lie between the others"
    es = evaluation.EvalSet(index, sessions, items)
    terms = {w: es.terms(trial_of(w))[0] for w in WINDOWS}   # the references: read once, never written
    for t in terms.values():
        t.setflags(write=False)
    yield dict(index=index, es=es, sessions=sessions, sess=sess, terms=terms, items=items, nq=nq)
    es.close()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 1000])
def test_replicate_sums_are_the_models_bits(tiny, window, B):
    _, rep = run(tiny["es"], [trial_of(window)], B)
    model = evaluation.bootstrap_model(tiny["terms"][window], tiny["sess"], B, SEED)
    assert not np.isnan(rep).any()
    worst = float(np.max(np.abs(rep[0] - model) / np.maximum(np.abs(model), 1e-300)))
    print("window %d, B %d: largest relative difference to the model %.3g over %d queries" % (window, B, worst, tiny["nq"]))
    assert same_bits(rep[0], model)
    assert rep[0, :, 1].max() > 0.0   # (the trial recommends something right: the sums are not trivially equal)


def test_chunking_company_and_repetition_change_no_bit(tiny):
    es, B = tiny["es"], 65
    t = trial_of(2)
    res, rep = run(es, [t], B)
    for chunk in (256, 512):
        res_c, rep_c = run(es, [dict(t, max_chunk_queries=chunk)], B)
        assert res_c == res and same_bits(rep_c, rep), chunk
    others = [trial_of(1, k=50), trial_of(5, business_logic=True), trial_of(2, max_chunk_queries=512, how_many=20)]
    res_4, rep_4 = run(es, others[:2] + [t] + others[2:], B)
    assert res_4[2] == res[0] and same_bits(rep_4[2], rep[0])
    res_again, rep_again = run(es, [t], B)
    assert res_again == res and same_bits(rep_again, rep)
    assert same_bits(rep[0], evaluation.bootstrap_model(tiny["terms"][2], tiny["sess"], B, SEED))
    # another seed is another resampling
    assert not np.array_equal(run(es, [t], B, seed=SEED + 1)[1][:, :, 0], rep[:, :, 0])


def test_a_replicate_does_not_depend_on_b(tiny):
    t = trial_of(5)
    _, small = run(tiny["es"], [t], 65)
    _, large = run(tiny["es"], [t], 1000)
    assert same_bits(small[0], large[0, :65])


def test_point_estimates_are_srn_evaluates(tiny):
    trials = [trial_of(1), trial_of(2, business_logic=True), trial_of(5, max_chunk_queries=256),
              trial_of(2, handler_sessions=True, exclude_seen=True, history=8, fill=True)]
    arr = (capi.EvalTrial * len(trials))(*[evaluation._trial(t) for t in trials])
    plain = (capi.EvalResult * len(trials))()
    capi.check(capi.lib().srn_evaluate(tiny["es"]._h, arr, len(trials), plain, None))
    res, _ = run(tiny["es"], trials, 63)
    assert res == [tuple(getattr(r, f) for f in RAW) for r in plain]
    assert res[0][0] == tiny["nq"] and res[0][1] > 0.0
    # and the Python entry without bootstrap gives today's reports
    reps = evaluation.evaluate(tiny["es"], trials)
    assert all("bootstrap" not in r and not any(k.endswith("_ci") for k in r) for r in reps)
    assert [r["sums"]["mrr"] for r in reps] == [r[9] for r in res]


def test_weights_column_is_the_sets_alone(tiny):
    trials = [trial_of(1), trial_of(5, k=50, how_many=20), trial_of(2, handler_sessions=True), trial_of(2, exclude_seen=True, history=8),
              trial_of(2, exclude_session=True, fill=True), trial_of(2, handler_sessions=True, exclude_seen=True, fill=True)]
    B = 257
    _, rep = run(tiny["es"], trials, B)
    w = evaluation.bootstrap_weights(SEED, B, len(tiny["sessions"])).astype(np.float64)
    want = w[:, tiny["sess"]].sum(axis=1)   # (integers far below 2^53: any order of addition gives them exactly)
    for i in range(len(trials)):
        assert same_bits(rep[i, :, 0], want), trials[i]
        assert np.array_equal(rep[i, :, 0], np.round(rep[i, :, 0]))
    # the serving rules change the rows, so the weighted sums differ while the weights do not
    assert not np.array_equal(rep[0, :, 1], rep[3, :, 1])
    model = evaluation.bootstrap_model(tiny["es"].terms(trials[5])[0], tiny["sess"], B, SEED)
    assert same_bits(rep[5], model)


def test_empty_sets_and_empty_replicates(tiny):
    index = tiny["index"]
    empty = evaluation.EvalSet(index, {}, tiny["items"])
    res, rep = run(empty, [trial_of(2)], 64)
    assert res[0][0] == 0 and same_bits(rep, np.zeros((1, 64, 7)))
    r = evaluation.evaluate(empty, [trial_of(2)], bootstrap=64, seed=SEED)[0]
    assert r["bootstrap"]["empty_replicates"] == 64 and r["Mrr@20_ci"] == (0.0, 0.0) and r["F1score@20_ci"] == (0.0, 0.0)
    known = [int(x) for x in np.unique(tiny["items"])[:2]]
    single = evaluation.EvalSet(index, {0: [known[0]], 1: known}, tiny["items"])   # one query, of the session with index 1
    B = 1000
    w = evaluation.bootstrap_weights(SEED, B, 2)[:, 1]
    res, rep = run(single, [trial_of(2)], B)
    assert res[0][0] == 1
    assert same_bits(rep[0], evaluation.bootstrap_model(single.terms(trial_of(2))[0], [1], B, SEED))
    assert np.array_equal(rep[0, :, 0], w.astype(np.float64))
    assert same_bits(rep[0, w == 0], np.zeros((int(np.count_nonzero(w == 0)), 7)))
    r = evaluation.evaluate(single, [trial_of(2)], bootstrap=B, seed=SEED)[0]
    assert r["bootstrap"]["empty_replicates"] == int(np.count_nonzero(w == 0)) > 300   # P(Poisson(1) = 0) = 0.37
    for s in (empty, single):
        s.close()


def test_intervals_contain_the_point_estimates(tiny):
    r = evaluation.evaluate(tiny["es"], [trial_of(2)], bootstrap=64, seed=SEED)[0]
    boot = r["bootstrap"]
    assert (boot["replicates"], boot["seed"], boot["ci"], boot["empty_replicates"]) == (64, SEED, 0.95, 0)
    assert boot["weights"].shape == (64,) and sorted(boot["sums"]) == sorted(evaluation.BOOTSTRAP_SUMS)
    for name in evaluation.METRICS:
        if name == "Coverage":
            assert "Coverage@20_ci" not in r
            continue
        lo, hi = r[name + "@20_ci"]
        print("%s@20 = %.6f in [%.6f, %.6f]" % (name, r[name + "@20"], lo, hi))
        assert lo <= r[name + "@20"] <= hi, name
        assert lo < hi, name
    narrow = evaluation.evaluate(tiny["es"], [trial_of(2)], bootstrap=64, seed=SEED, ci=0.5)[0]
    assert r["Mrr@20_ci"][0] < narrow["Mrr@20_ci"][0] < narrow["Mrr@20_ci"][1] < r["Mrr@20_ci"][1]


def test_compare_on_the_device(tiny):
    good, bad = trial_of(2), trial_of(2, k=1, m=1)
    a, b = evaluation.evaluate(tiny["es"], [good, bad], bootstrap=256, seed=SEED)
    assert evaluation.compare(a, a) == {"delta": 0.0, "ci": (0.0, 0.0), "p_better": 0.0, "replicates": 256}
    c = evaluation.compare(a, b)
    print("good - bad: delta %.6f, interval [%.6f, %.6f], p_better %.3f" % (c["delta"], c["ci"][0], c["ci"][1], c["p_better"]))
    assert c["delta"] == a["Mrr@20"] - b["Mrr@20"] > 0.0
    assert c["ci"][0] > 0.0 and c["p_better"] > 0.975
    assert c["ci"][0] <= c["delta"] <= c["ci"][1]
    # paired across calls: the same trial from a call of its own
    alone = evaluation.evaluate(tiny["es"], [bad], bootstrap=256, seed=SEED)[0]
    assert evaluation.compare(a, alone) == c
    with pytest.raises(ValueError):
        evaluation.compare(a, evaluation.evaluate(tiny["es"], [bad], bootstrap=256, seed=SEED + 1)[0])


def _example(tmp_path):
    g = np.load(os.path.join(GOLDEN, "example_golden.npz"))
    off, items, ts = g["sess_off"].astype(np.int64), g["items"], g["ts"]
    train, test = tmp_path / "train.txt", tmp_path / "test.txt"
    with open(train, "w") as f:
        f.write("SessionId\tItemId\tTime\n")
        for s in range(len(ts)):
            for it in items[off[s]:off[s + 1]]:
                f.write("%d\t%d\t%d.0\n" % (s + 1, it, ts[s]))
    with open(test, "w") as f:
        f.write("SessionId\tItemId\tTime\n")
        for s, it, t in g["test_rows"]:
            f.write("%d\t%d\t%d.0\n" % (s, it, t))
    return str(train), str(test)


def test_search_pairs_trials_across_indices_and_the_cli_keeps_its_csv(tmp_path, monkeypatch, capsys):
    train, test = _example(tmp_path)
    trials = hpo.exhaustive({"m": [100], "k": [50, 100], "max_items_in_session": [2], "idf_weighting": [1, 2]})
    res = hpo.search(train, test, trials, business_logic=True, bootstrap=64, seed=5)
    assert len(res["records"]) == 4 and {r["idf_weighting"] for r in res["records"]} == {1, 2}
    w0 = res["records"][0]["report"]["bootstrap"]["weights"]
    assert w0.shape == (64,) and w0.min() > 0
    for r in res["records"]:
        assert np.array_equal(r["report"]["bootstrap"]["weights"], w0)
        assert "Mrr@20_ci" in r["report"]
    plain = hpo.search(train, test, trials, business_logic=True)
    assert [r["MRR@20"] for r in plain["records"]] == [r["MRR@20"] for r in res["records"]]
    assert len(hpo.within_noise(res["records"], res["best"])) == 3
    # the CLI: the reference's CSV byte for byte, the intervals elsewhere
    cfg = tmp_path / "example.toml"
    cfg.write_text('[hyperparam]\ntraining_data_path = "train.txt"\ntest_data_path = "test.txt"\nsave_records = true\nout_path = "results.csv"\n'
                   'enable_business_logic = true\n')
    monkeypatch.chdir(tmp_path)
    assert hpo.main([str(cfg), "--random", "4", "--seed", "3"]) == 0
    out_plain = capsys.readouterr().out.splitlines()
    csv_plain = open(tmp_path / "results.csv", "rb").read()
    os.remove(tmp_path / "results.csv")
    assert hpo.main([str(cfg), "--random", "4", "--seed", "3", "--bootstrap", "64", "--ci", "0.9", "--ci-csv", "intervals.csv"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert open(tmp_path / "results.csv", "rb").read() == csv_plain and len(csv_plain.splitlines()) == 5
    assert out[:-1] == out_plain
    assert out[-1].startswith("Bootstrap (64 replicates, seed 3): best Mrr@20 90% interval [") and out[-1].endswith("of 3 other trials within noise of the best")
    lines = open(tmp_path / "intervals.csv").read().splitlines()
    assert lines[0] == "iteration,MRR@20,ci_lo,ci_hi,best_minus_trial,diff_lo,diff_hi,p_best_better" and len(lines) == 5
    for line, rec in zip(lines[1:], csv_plain.decode().splitlines()[1:]):
        f = line.split(",")
        assert f[0] == rec.split(",")[0] and f[1] == rec.split(",")[-1]
        assert float(f[2]) <= float(f[1]) <= float(f[3])
