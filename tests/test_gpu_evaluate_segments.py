"""Trials by segment on the GPU (srn_evaluate_segments): the ids against segment_ids_model, the segment sums and segment replicates against
segment_model over the trial's per-query terms bit for bit, the totals against srn_evaluate / srn_evaluate_bootstrap, a label's segment against an evaluation set
built from that label's sessions alone, and the Python surface: reports, compare(segment=), the search and the backtest."""
import ctypes as C
import os

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, evaluation, hpo, synth
from helpers import GOLDEN

import prepare_cases as pc
from segment_cases import RAW, SEED, WINDOWS, make_sessions, run_segments, same_bits, trial_of

pytestmark = pytest.mark.gpu

UNKNOWN = 10 ** 9   # test items from here upwards are in no training session


@pytest.fixture(scope="module")
def tiny():
    inter, n_items, k, m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0)
    index.set_fallback_popular(64)
    rng = np.random.default_rng(21)
    pool = np.unique(items)[:3000]
    sessions = make_sessions(synth.test_sessions(330, n_items, seed=synth.SEED + 31).values(), pool, rng, unknown_from=UNKNOWN)
    sess = evaluation.session_of_query(sessions)
    nq = len(sess)
    assert nq > 3 * 256 and nq % 256 != 0
    assert all(sess[g - 1] == sess[g] for g in range(256, nq, 256)), "a session straddles every boundary between groups"
    assert len(np.unique(sess)) < int(sess.max()) + 1 - 50, "sessions of one event lie between the others"
    es = evaluation.EvalSet(index, sessions, items)
    # what the set holds: the training count of every test item the index's dictionary knows
    ids, cnt = np.unique(items, return_counts=True)
    train = dict(zip(ids.tolist(), cnt.tolist()))
    test_items = sorted({int(x) for ev in sessions.values() for x in ev})
    counts = {x: train[x] for x in test_items if x in train and index.postings(x)[0] is not None}
    assert any(x >= UNKNOWN for x in test_items) and len(counts) > 100
    terms = {w: es.terms(trial_of(w))[0] for w in WINDOWS}   # the references: read once, never written
    for t in terms.values():
        t.setflags(write=False)
    yield dict(index=index, es=es, sessions=sessions, sess=sess, terms=terms, items=items, nq=nq, counts=counts)
    es.close()


def specs(tiny):
    """The segmentations of the tests, by name.  The count bounds come from the set's own counts: bounds[0] = 1 and one bound equal to an occurring count."""
    n_s = len(tiny["sessions"])
    seqs = list(tiny["sessions"].values())

    def bounds(which):   # over the items that occur in the role: e_{t+1} (which = 1) or e_t (0)
        occurring = sorted({tiny["counts"][ev[t - 1 + which]] for ev in seqs for t in range(1, len(ev)) if ev[t - 1 + which] in tiny["counts"]})
        mid, top = occurring[len(occurring) // 2], occurring[-1]
        assert 1 <= occurring[0] < mid < top and mid > 1
        return [1, mid, top]
    return {
        "one": dict(by="position", n=1),
        "two": dict(by="current_count", bounds=bounds(0)[1:2]),
        "pos8": dict(by="position", n=8),
        "pos64": dict(by="position", n=64),
        "lab64": dict(by="labels", labels=np.arange(n_s) % 61, n=64),          # labels 61..63 have no session
        "lab3": dict(by="labels", labels=(np.arange(n_s) * 7 // 3) % 3, n=3, names=["phone", "tablet", "desktop"]),
        "target": dict(by="target_count", bounds=bounds(1)),
        "current": dict(by="current_count", bounds=bounds(0)),
    }


@pytest.mark.parametrize("name", ["one", "two", "pos8", "pos64", "lab64", "lab3", "target", "current"])
def test_ids_are_the_models(tiny, name):
    spec = specs(tiny)[name]
    got = tiny["es"].segment_ids(spec)
    want = evaluation.segment_ids_model(tiny["sessions"], spec, tiny["counts"])
    assert got.dtype == np.uint16 and got.shape == (tiny["nq"],)
    assert np.array_equal(got, want)
    used = np.bincount(got, minlength=evaluation._spec(spec)[1])
    print("%s: queries per segment %s" % (name, used.tolist()))
    if name in ("target", "current"):
        assert used[0] > 0, "some items are absent from the index: count 0, below bounds[0] = 1"
        assert used.min() > 0, "every band occurs"
        which = 1 if name == "target" else 0
        role = [ev[t - 1 + which] for ev in tiny["sessions"].values() for t in range(1, len(ev))]
        on_the_bound = [q for q, x in enumerate(role) if tiny["counts"].get(x, 0) == spec["bounds"][1]]
        assert on_the_bound and all(got[q] == 2 for q in on_the_bound), "a count equal to a bound falls in the upper band"
    if name == "one":
        assert not got.any()


# (window, segmentation, B): every window with S = 1, 2, 8 and 64, B = 1, 255, 256 and 257 among them; S = 64 also through all eight segment tiles at B > 256
SUM_CASES = [(w, n, b) for w in WINDOWS for n, b in (("one", 257), ("two", 255), ("pos8", 256), ("lab64", 1))] + [(2, "lab64", 257), (5, "pos64", 256)]


@pytest.mark.parametrize("window,name,B", SUM_CASES)
def test_segment_sums_and_replicates_are_the_models_bits(tiny, window, name, B):
    spec = specs(tiny)[name]
    S = evaluation._spec(spec)[1]
    ids = evaluation.segment_ids_model(tiny["sessions"], spec, tiny["counts"])
    _, seg_out, rep, seg_rep = run_segments(tiny["es"], [trial_of(window)], spec, B)
    sums, reps = evaluation.segment_model(tiny["terms"][window], ids, S, tiny["sess"], B=B, seed=SEED)
    assert not np.isnan(seg_rep).any() and not np.isnan(seg_out).any()
    worst = float(np.max(np.abs(seg_rep[0] - reps) / np.maximum(np.abs(reps), 1e-300)))
    print("window %d, %s, B %d: largest relative difference of a replicate sum to the model %.3g" % (window, name, B, worst))
    assert same_bits(seg_out[0], sums)
    assert same_bits(seg_rep[0], reps)
    assert seg_out[0, :, 0].sum() == tiny["nq"] and seg_out[0, :, 1].max() > 0.0
    empty = np.flatnonzero(np.bincount(ids, minlength=S) == 0)
    if name == "lab64":
        assert len(empty) == 3, "segments without queries: the labels no session carries"
    if name == "pos64":
        per_group = np.array([np.bincount(ids[g0:g0 + 256], minlength=S) for g0 in range(0, len(ids), 256)])
        assert np.any((per_group == 0) & (per_group.sum(axis=0) > 0)[None, :]), "a segment that is empty in some group only"
    for g in empty:   # n = 0 and +0.0, every bit
        assert same_bits(seg_out[0, g], np.zeros(7)) and same_bits(seg_rep[0, g], np.zeros((B, 7)))


def test_chunking_and_company_change_no_bit(tiny):
    es, B = tiny["es"], 65
    spec = specs(tiny)["pos8"]
    t = trial_of(2)
    res, seg_out, rep, seg_rep = run_segments(es, [t], spec, B)
    res_c, seg_out_c, rep_c, seg_rep_c = run_segments(es, [dict(t, max_chunk_queries=256)], spec, B)
    assert res_c == res and same_bits(seg_out_c, seg_out) and same_bits(rep_c, rep) and same_bits(seg_rep_c, seg_rep)
    others = [trial_of(1, k=50), trial_of(5, business_logic=True), trial_of(2, max_chunk_queries=512, how_many=20)]
    res_4, seg_out_4, rep_4, seg_rep_4 = run_segments(es, others[:2] + [t] + others[2:], spec, B)
    assert res_4[2] == res[0] and same_bits(seg_out_4[2], seg_out[0]) and same_bits(rep_4[2], rep[0]) and same_bits(seg_rep_4[2], seg_rep[0])
    assert not same_bits(seg_out_4[0], seg_out[0])   # (another trial, other sums)
    # without a bootstrap the segment sums are the same, and a segment's do not depend on S where its queries do not change
    _, plain, none_rep, none_seg_rep = run_segments(es, [t], spec)
    assert none_rep is None and none_seg_rep is None and same_bits(plain, seg_out)
    _, wide, _, wide_rep = run_segments(es, [t], specs(tiny)["pos64"], B)
    assert same_bits(wide[0, :7], seg_out[0, :7]) and same_bits(wide_rep[0, :7], seg_rep[0, :7])


def test_nothing_else_moved(tiny):
    es, B = tiny["es"], 63
    trials = [trial_of(1), trial_of(2, business_logic=True), trial_of(5, max_chunk_queries=256),
              trial_of(2, handler_sessions=True, exclude_seen=True, history=8, fill=True)]
    arr = (capi.EvalTrial * len(trials))(*[evaluation._trial(t) for t in trials])
    plain = (capi.EvalResult * len(trials))()
    capi.check(capi.lib().srn_evaluate(es._h, arr, len(trials), plain, None))
    booted = (capi.EvalResult * len(trials))()
    want_rep = np.full((len(trials), B, 7), np.nan)
    boot = capi.Bootstrap(SEED, B, 0)
    capi.check(capi.lib().srn_evaluate_bootstrap(es._h, arr, len(trials), C.byref(boot), booted, capi.ptr(want_rep), None))
    want = [tuple(getattr(r, f) for f in RAW) for r in plain]
    for name in ("pos8", "lab64", "target"):
        spec = specs(tiny)[name]
        res, seg_out, rep, seg_rep = run_segments(es, trials, spec, B)
        res_plain, seg_plain, _, _ = run_segments(es, trials, spec)
        assert res == want and res_plain == want, name
        assert same_bits(rep, want_rep), name
        assert same_bits(seg_plain, seg_out), name
        for i in range(len(trials)):
            r = plain[i]
            assert seg_out[i, :, 0].sum() == r.n_evaluations == tiny["nq"]
            assert seg_out[i, :, 3].sum() == r.sum_hit_rate                       # 0 or 1 per query: exact in any order
            assert np.array_equal(seg_rep[i, :, :, 0].sum(axis=0), rep[i, :, 0])   # the weights: integers
            for col, field in ((1, "sum_mrr"), (2, "sum_ndcg"), (4, "sum_popularity"), (5, "sum_precision"), (6, "sum_recall")):
                total = getattr(r, field)
                assert abs(seg_out[i, :, col].sum() - total) <= 1e-12 * abs(total), (name, i, field)
                assert np.all(np.abs(seg_rep[i, :, :, col].sum(axis=0) - rep[i, :, col]) <= 1e-12 * np.abs(rep[i, :, col])), (name, i, field)
    # the handler's sessions change the rows, never the ids: the raw t, e_t and e_{t+1}
    assert seg_out[3, :, 0].tolist() == seg_out[0, :, 0].tolist()
    # a wrong number of labels is refused
    with pytest.raises(capi.SerenadeError) as e:
        run_segments(es, trials[:1], dict(by="labels", labels=np.zeros(len(tiny["sessions"]) - 1, np.uint16), n=2))
    assert e.value.code == capi.SRN_EINVAL and "n_labels" in str(e.value)
    with pytest.raises(capi.SerenadeError):
        es.segment_ids(dict(by="labels", labels=np.zeros(len(tiny["sessions"]) + 1, np.uint16), n=2))


SEVEN = ("Mrr", "Ndcg", "HitRate", "Popularity", "Precision", "Recall", "F1score")


@pytest.mark.parametrize("rules", [{}, dict(handler_sessions=True, exclude_seen=True, fill=True)], ids=["plain", "serving_rules"])
def test_a_labels_segment_is_the_evaluation_of_its_sessions_alone(tiny, rules):
    spec = specs(tiny)["lab3"]
    trial = trial_of(2, **rules)
    report = evaluation.evaluate(tiny["es"], [trial], segments=spec)[0]
    seqs = list(tiny["sessions"].values())
    assert sum(s["qty_evaluations"] for s in report["segments"]) == tiny["nq"]
    for g in range(3):
        part = evaluation.EvalSet(tiny["index"], [ev for s, ev in enumerate(seqs) if spec["labels"][s] == g], tiny["items"])
        alone = evaluation.evaluate(part, [trial])[0]
        part.close()
        seg = report["segments"][g]
        assert seg["qty_evaluations"] == alone["qty_evaluations"] > 100
        for name in SEVEN:
            a, b = seg[name + "@20"], alone[name + "@20"]
            print("label %d %s@20: segment %.15g, its sessions alone %.15g" % (g, name, a, b))
            assert abs(a - b) <= 1e-12 * abs(b), (g, name)
        assert seg["Mrr@20"] > 0.0


def test_reports_carry_named_segments_and_compare_pairs_them(tiny):
    es = tiny["es"]
    good, bad = trial_of(2), trial_of(2, k=1, m=1)
    a, b = evaluation.evaluate(es, [good, bad], bootstrap=256, seed=SEED, segments=dict(by="position", n=4))
    assert [s["name"] for s in a["segments"]] == ["t=1", "t=2", "t=3", "t>=4"]
    plain = evaluation.evaluate(es, [good], bootstrap=256, seed=SEED)[0]
    for key in plain:
        if key not in ("ms_predict", "ms_eval", "bootstrap"):
            assert a[key] == plain[key], key
    assert np.array_equal(a["bootstrap"]["weights"], plain["bootstrap"]["weights"]) and "segments" not in plain
    for s in a["segments"]:
        assert s["qty_evaluations"] > 0 and s["bootstrap"]["replicates"] == 256 and s["bootstrap"]["weights"].shape == (256,)
        assert sorted(s["sums"]) == sorted(evaluation.BOOTSTRAP_SUMS) and "Coverage@20" not in s
        for name in SEVEN:
            lo, hi = s[name + "@20_ci"]
            assert lo <= s[name + "@20"] <= hi, (s["name"], name)
        assert s["Mrr@20"] == s["sums"]["mrr"] / s["qty_evaluations"]
        p, r = s["Precision@20"], s["Recall@20"]
        assert s["F1score@20"] == 2.0 * (p * r) / (p + r)
    assert sum(s["qty_evaluations"] for s in a["segments"]) == a["qty_evaluations"]
    # without a bootstrap: the same point estimates, no intervals
    a0 = evaluation.evaluate(es, [good], segments=dict(by="position", n=4))[0]
    assert [(s["name"], s["qty_evaluations"], s["Mrr@20"]) for s in a0["segments"]] == [(s["name"], s["qty_evaluations"], s["Mrr@20"]) for s in a["segments"]]
    assert all("bootstrap" not in s and "Mrr@20_ci" not in s for s in a0["segments"]) and "bootstrap" not in a0
    # compare: a segment of two trials, paired across calls; a segment against the total
    c = evaluation.compare(a, b, "Mrr", segment=0)
    print("t=1, good - bad: delta %.6f, interval [%.6f, %.6f], p_better %.3f" % (c["delta"], c["ci"][0], c["ci"][1], c["p_better"]))
    assert c["delta"] == a["segments"][0]["Mrr@20"] - b["segments"][0]["Mrr@20"] > 0.0 and c["ci"][0] > 0.0 and c["replicates"] == 256
    alone = evaluation.evaluate(es, [bad], bootstrap=256, seed=SEED, segments=dict(by="position", n=4))[0]
    assert evaluation.compare(a, alone, "Mrr", segment=0) == c
    assert evaluation.compare(a, a, "Mrr", segment=1) == {"delta": 0.0, "ci": (0.0, 0.0), "p_better": 0.0, "replicates": 256}
    against_total = evaluation.compare(a, a, "Mrr", segment=(0, None))
    assert against_total["delta"] == a["segments"][0]["Mrr@20"] - a["Mrr@20"] and against_total["replicates"] == 256
    assert against_total["ci"][0] <= against_total["delta"] <= against_total["ci"][1]
    with pytest.raises(ValueError):
        evaluation.compare(a, plain, "Mrr", segment=0)
    with pytest.raises(ValueError):
        evaluation.compare(a, evaluation.evaluate(es, [bad], bootstrap=256, seed=SEED + 1, segments=dict(by="position", n=4))[0], "Mrr", segment=0)
    # an empty set: every segment is empty
    empty = evaluation.EvalSet(tiny["index"], {}, tiny["items"])
    r = evaluation.evaluate(empty, [good], bootstrap=64, seed=SEED, segments=dict(by="target_count", bounds=[1, 10]))[0]
    assert [s["name"] for s in r["segments"]] == ["count<1", "1<=count<10", "count>=10"]
    assert all(s["qty_evaluations"] == 0 and s["Mrr@20"] == 0.0 and s["F1score@20"] == 0.0 and s["Mrr@20_ci"] == (0.0, 0.0) for s in r["segments"])
    assert empty.segment_ids(dict(by="position", n=3)).shape == (0,)
    empty.close()


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


def test_search_carries_segments_and_the_cli_prints_the_best_trials_table(tmp_path, monkeypatch, capsys):
    train, test = _example(tmp_path)
    trials = hpo.exhaustive({"m": [100], "k": [50, 100], "max_items_in_session": [2], "idf_weighting": [1, 2]})
    spec = dict(by="target_count", bounds=[1, 3])
    res = hpo.search(train, test, trials, business_logic=True, segments=spec)
    plain = hpo.search(train, test, trials, business_logic=True)
    assert len(res["records"]) == 4
    assert [r["MRR@20"] for r in plain["records"]] == [r["MRR@20"] for r in res["records"]]
    for r, p in zip(res["records"], plain["records"]):
        segs = r["report"]["segments"]
        assert [s["name"] for s in segs] == ["count<1", "1<=count<3", "count>=3"] and "segments" not in p["report"]
        assert sum(s["qty_evaluations"] for s in segs) == r["report"]["qty_evaluations"] > 0
        assert [s["qty_evaluations"] for s in segs] == [s["qty_evaluations"] for s in res["records"][0]["report"]["segments"]]   # the set's alone
    # the CLI: the CSV and the Best lines as ever, the table behind them
    cfg = tmp_path / "example.toml"
    cfg.write_text('[hyperparam]\ntraining_data_path = "train.txt"\ntest_data_path = "test.txt"\nsave_records = true\nout_path = "results.csv"\n'
                   'enable_business_logic = true\n')
    monkeypatch.chdir(tmp_path)
    assert hpo.main([str(cfg), "--random", "4", "--seed", "3"]) == 0
    out_plain = capsys.readouterr().out.splitlines()
    csv_plain = open(tmp_path / "results.csv", "rb").read()
    os.remove(tmp_path / "results.csv")
    assert hpo.main([str(cfg), "--random", "4", "--seed", "3", "--segments", "position:3"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert open(tmp_path / "results.csv", "rb").read() == csv_plain and len(csv_plain.splitlines()) == 5
    assert out[:len(out_plain)] == out_plain and len(out) == len(out_plain) + 5
    assert out[len(out_plain)] == "Best trial by segment (position):"
    assert [line.split()[0] for line in out[len(out_plain) + 1:]] == ["segment", "t=1", "t=2", "t>=3"]
    assert out[len(out_plain) + 1].split()[2:] == ["Mrr@20", "Ndcg@20", "HitRate@20", "Popularity@20", "Precision@20", "Recall@20", "F1score@20"]


def test_backtest_gives_every_folds_reports_their_segments():
    s, i, t = pc.random_log(41, n=3000, n_sessions=450, n_items=60, f64=True)
    trials = [dict(k=50, m=500, max_items_in_session=2)]
    spec = dict(by="position", n=3)
    got = sa.backtest((s, i, t), trials, 500, 1.0, folds=2, test_span=pc.DAY, min_item_support=3, segments=spec)
    plain = sa.backtest((s, i, t), trials, 500, 1.0, folds=2, test_span=pc.DAY, min_item_support=3)
    assert len(got) == 2
    for f, p in zip(got, plain):
        r = f["reports"][0]
        assert [x["name"] for x in r["segments"]] == ["t=1", "t=2", "t>=3"]
        assert sum(x["qty_evaluations"] for x in r["segments"]) == r["qty_evaluations"] > 50
        assert r["sums"] == p["reports"][0]["sums"] and "segments" not in p["reports"][0]
        assert sum(x["sums"]["hit_rate"] for x in r["segments"]) == r["sums"]["hit_rate"]
    with pytest.raises(ValueError, match="labels"):
        sa.backtest((s, i, t), trials, 500, 1.0, folds=2, test_span=pc.DAY, segments=dict(by="labels", labels=[0, 1], n=2))
