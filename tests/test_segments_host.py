"""Trials by segment: what runs without a GPU -- the ABI's symbols, structs and refusals, the id rule and the sum rule in NumPy on hand-written
sessions, the reports' names, compare(segment=) and the search CLI's option."""
import argparse
import ctypes as C

import numpy as np
import pytest

from serenade_amd import capi, evaluation, hpo, prepare
from segment_cases import HAND, HAND_COUNTS


def _trial(**kw):
    t = dict(k=50, m=500, how_many=20, max_items_in_session=2, length=20)
    t.update(kw)
    return evaluation._trial(t)


def test_segment_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in ("srn_evaluate_segments", "srn_eval_segment_ids", "srn_debug_eval_segment_ms"):
        assert name in capi.SYMBOLS
        assert getattr(L, name).argtypes == capi.SYMBOLS[name][1]
    assert C.sizeof(capi.Segments) == 40 and C.sizeof(capi.EvalSegment) == 56
    assert capi.Segments.labels.offset == 8 and capi.Segments.n_labels.offset == 16 and capi.Segments.bounds.offset == 24 and capi.Segments.reserved.offset == 32
    assert capi.MAX_SEGMENTS == 64
    assert (capi.SEG_STATE, capi.SEG_LABEL, capi.SEG_TARGET_COUNT, capi.SEG_CURRENT_COUNT) == (1, 2, 3, 4)
    assert set(evaluation.SEGMENT_MODES.values()) == {1, 2, 3, 4}


def test_segment_arguments_are_refused_before_the_missing_set_is_reached():
    L = capi.lib()
    r, t = capi.EvalResult(), _trial()
    seg_out = (capi.EvalSegment * 64)()
    rep, seg_rep = np.zeros((4096, 7)), np.zeros((16 * 4096, 7))
    labels = np.array([0, 1, 2, 1], np.uint16)
    bounds = np.array([1, 10, 100], np.uint64)

    def seg_of(mode=capi.SEG_STATE, S=8, labels=None, bounds=None, reserved=0):
        return capi.Segments(mode, S, None if labels is None else labels.ctypes.data, 0 if labels is None else len(labels),
                             None if bounds is None else bounds.ctypes.data, reserved)

    def call(seg, boot=None, trial=t, out=seg_out, rep=rep, seg_rep=seg_rep):
        return L.srn_evaluate_segments(None, C.byref(trial), 1, C.byref(seg) if seg is not None else None, C.byref(boot) if boot is not None else None, C.byref(r),
                                       out, capi.ptr(rep), capi.ptr(seg_rep), None)
    assert call(None) == capi.SRN_EINVAL
    assert call(seg_of(mode=0)) == capi.SRN_EINVAL and b"mode" in L.srn_last_error()
    assert call(seg_of(mode=5)) == capi.SRN_EINVAL and b"mode" in L.srn_last_error()
    assert call(seg_of(S=0)) == capi.SRN_EINVAL and b"segments" in L.srn_last_error()
    assert call(seg_of(S=65)) == capi.SRN_ERANGE and b"SRN_MAX_SEGMENTS" in L.srn_last_error()
    assert call(seg_of(reserved=1)) == capi.SRN_EINVAL and b"reserved" in L.srn_last_error()
    assert call(seg_of(capi.SEG_LABEL, 2, labels=labels)) == capi.SRN_EINVAL and b"label" in L.srn_last_error()   # the label 2 is not below 2
    for mode in (capi.SEG_TARGET_COUNT, capi.SEG_CURRENT_COUNT):
        assert call(seg_of(mode, 4, bounds=np.array([1, 10, 10], np.uint64))) == capi.SRN_EINVAL and b"ascending" in L.srn_last_error()
        assert call(seg_of(mode, 4, bounds=np.array([1, 100, 10], np.uint64))) == capi.SRN_EINVAL and b"ascending" in L.srn_last_error()
        assert call(seg_of(mode, 4)) == capi.SRN_EINVAL and b"bounds" in L.srn_last_error()
    assert call(seg_of(), out=None) == capi.SRN_EINVAL and b"null argument" in L.srn_last_error()
    # with a bootstrap: its own refusals, and the product's limit
    assert call(seg_of(), capi.Bootstrap(0, 64, 0), rep=None) == capi.SRN_EINVAL
    assert call(seg_of(), capi.Bootstrap(0, 64, 0), seg_rep=None) == capi.SRN_EINVAL
    assert call(seg_of(), capi.Bootstrap(0, 0, 0)) == capi.SRN_EINVAL and b"replicates" in L.srn_last_error()
    assert call(seg_of(), capi.Bootstrap(0, 64, 1)) == capi.SRN_EINVAL and b"flags" in L.srn_last_error()
    assert call(seg_of(), capi.Bootstrap(0, capi.MAX_BOOTSTRAP + 1, 0)) == capi.SRN_ERANGE and b"SRN_MAX_BOOTSTRAP" in L.srn_last_error()
    assert call(seg_of(S=17), capi.Bootstrap(0, capi.MAX_BOOTSTRAP, 0)) == capi.SRN_ERANGE and b"segments * replicates" in L.srn_last_error()
    assert call(seg_of(S=64), capi.Bootstrap(0, 1025, 0)) == capi.SRN_ERANGE and b"segments * replicates" in L.srn_last_error()
    # srn_evaluate's own refusals stay, and good calls get as far as the missing set
    assert call(seg_of(), trial=_trial(max_items_in_session=capi.MAX_SESSION_LEN + 1)) == capi.SRN_ERANGE
    assert call(seg_of(), trial=_trial(k=0)) == capi.SRN_EINVAL
    for good in (seg_of(), seg_of(S=1), seg_of(S=64), seg_of(capi.SEG_LABEL, 3, labels=labels), seg_of(capi.SEG_TARGET_COUNT, 4, bounds=bounds),
                 seg_of(capi.SEG_CURRENT_COUNT, 1)):
        assert call(good) == capi.SRN_EINVAL and b"null evaluation set" in L.srn_last_error()
    assert call(seg_of(S=16), capi.Bootstrap(0, capi.MAX_BOOTSTRAP, 0)) == capi.SRN_EINVAL and b"null evaluation set" in L.srn_last_error()
    assert call(seg_of(S=64), capi.Bootstrap(0, 1024, 0)) == capi.SRN_EINVAL and b"null evaluation set" in L.srn_last_error()
    # the ids alone
    n = C.c_size_t()
    assert L.srn_eval_segment_ids(None, C.byref(seg_of(S=0)), None, 0, C.byref(n)) == capi.SRN_EINVAL and b"segments" in L.srn_last_error()
    assert L.srn_eval_segment_ids(None, C.byref(seg_of()), None, 0, None) == capi.SRN_EINVAL and b"null argument" in L.srn_last_error()
    assert L.srn_eval_segment_ids(None, C.byref(seg_of()), None, 0, C.byref(n)) == capi.SRN_EINVAL and b"null evaluation set" in L.srn_last_error()
    assert L.srn_debug_eval_segment_ms(None, None, None) == capi.SRN_EINVAL
    with pytest.raises(capi.SerenadeError) as e:
        evaluation.evaluate(None, [dict(k=50, m=500, max_items_in_session=2)], segments=dict(by="position", n=65))
    assert e.value.code == capi.SRN_ERANGE


def test_ids_by_position_clamp_at_s():
    # HAND's queries in set order: session 3 gives t = 1..4, session 5 none, session 8 t = 1..3, session 9 t = 1
    states = [1, 2, 3, 4, 1, 2, 3, 1]
    for S in (1, 2, 3, 4, 8, 64):
        ids = evaluation.segment_ids_model(HAND, dict(by="position", n=S))
        assert ids.dtype == np.uint16 and ids.tolist() == [min(t, S) - 1 for t in states], S
    assert evaluation.segment_ids_model(HAND, dict(by="position", n=1)).tolist() == [0] * 8
    assert evaluation.segment_ids_model(HAND, dict(by="position", n=3)).tolist() == [0, 1, 2, 2, 0, 1, 2, 0]
    assert evaluation.segment_ids_model(list(HAND.values()), dict(by="position", n=3)).tolist() == [0, 1, 2, 2, 0, 1, 2, 0]


def test_ids_by_label_follow_the_session_index_and_count_single_event_sessions():
    ids = evaluation.segment_ids_model(HAND, dict(by="labels", labels=[2, 1, 0, 2], n=3))
    assert ids.tolist() == [2, 2, 2, 2, 0, 0, 0, 2]   # the label 1 belongs to the session of one event: no query carries it
    with pytest.raises(ValueError):
        evaluation.segment_ids_model(HAND, dict(by="labels", labels=[0, 0, 0], n=3))
    with pytest.raises(ValueError):
        evaluation.segment_ids_model(HAND, dict(by="labels", labels=[0, 0, 0, 3], n=3))


def test_ids_by_count_put_a_count_equal_to_a_bound_in_the_upper_band():
    bounds = [1, 10, 100]
    band = lambda c: sum(1 for b in bounds if b <= c)
    assert [band(c) for c in (0, 1, 9, 10, 99, 100, 10 ** 6)] == [0, 1, 1, 2, 2, 3, 3]
    nxt = [11, 12, 13, 14, 11, 900, 10, 12]          # e_{t+1} of HAND's queries
    cur = [10, 11, 12, 13, 11, 11, 900, 901]         # e_t
    target = evaluation.segment_ids_model(HAND, dict(by="target_count", bounds=bounds), HAND_COUNTS)
    assert target.tolist() == [band(HAND_COUNTS.get(x, 0)) for x in nxt] == [2, 3, 1, 2, 2, 0, 1, 3]
    current = evaluation.segment_ids_model(HAND, dict(by="current_count", bounds=bounds), HAND_COUNTS)
    assert current.tolist() == [band(HAND_COUNTS.get(x, 0)) for x in cur] == [1, 2, 3, 1, 2, 2, 0, 0]
    # an unknown item counts 0: with bounds[0] = 1 it is segment 0, and without counts every query is
    assert evaluation.segment_ids_model(HAND, dict(by="target_count", bounds=bounds)).tolist() == [0] * 8
    # one segment: no bounds, all zeros
    for by in ("target_count", "current_count"):
        assert evaluation.segment_ids_model(HAND, dict(by=by, bounds=[]), HAND_COUNTS).tolist() == [0] * 8
    with pytest.raises(ValueError):
        evaluation.segment_ids_model(HAND, dict(by="target_count", bounds=[1, 1]), HAND_COUNTS)
    with pytest.raises(ValueError):
        evaluation.segment_ids_model(HAND, dict(by="nothing"))


def _random_case(n, S, seed):
    rng = np.random.default_rng(seed)
    terms = rng.random((n, 7))
    terms[:, 1] = rng.integers(0, 2, size=n)     # hit: 0 or 1
    ids = rng.integers(0, S, size=n)
    sess = np.sort(rng.integers(0, n // 4 + 1, size=n)) * 2 + 3
    return terms, ids, sess


def test_segment_model_counts_and_hit_sums_add_up_exactly():
    n = 700
    for S in (2, 8, 64):
        terms, ids, _ = _random_case(n, S, S)
        if S == 8:
            ids[ids == 5] = 4                    # a segment that is empty altogether
            ids[:256][ids[:256] == 3] = 2        # ... and one that is empty in the first group
        sums = evaluation.segment_model(terms, ids, S)
        assert sums.shape == (S, 7)
        assert sums[:, 0].tolist() == np.bincount(ids, minlength=S).tolist() and sums[:, 0].sum() == n
        assert sums[:, 3].sum() == terms[:, 1].sum()            # hit_rate: the terms are 0 or 1
        assert np.array_equal(sums[:, 3], np.bincount(ids, weights=terms[:, 1], minlength=S))
        whole = evaluation.segment_model(terms, np.zeros(n, np.int64), 1)
        assert np.allclose(sums.sum(axis=0), whole[0], rtol=1e-12, atol=0.0)
        if S == 8:
            assert np.array_equal(sums[5].view(np.uint64), np.zeros(7, np.uint64))   # +0.0, every bit


def test_segment_model_states_the_order_rule():
    n, S = 700, 5
    terms, ids, sess = _random_case(n, S, 11)
    sums, rep = evaluation.segment_model(terms, ids, S, sess, B=9, seed=11)
    assert np.array_equal(sums, evaluation.segment_model(terms, ids, S))
    w = evaluation.bootstrap_weights(11, 9, int(sess.max()) + 1).astype(np.float64)
    cols = [0, 2, 1, 6, 4, 5]   # TERMS -> mrr, ndcg, hit_rate, popularity, precision, recall
    for g in (0, 4):
        for b in (None, 0, 8):
            want = [0.0] * 7
            for g0 in range(0, n, 256):
                acc = [0.0] * 7
                for q in range(g0, min(g0 + 256, n)):
                    if ids[q] != g:
                        continue
                    wq = 1.0 if b is None else float(w[b, sess[q]])
                    acc[0] = acc[0] + wq
                    for j, c in enumerate(cols):
                        acc[1 + j] = acc[1 + j] + wq * float(terms[q, c])
                want = [t + a for t, a in zip(want, acc)]
            assert (sums[g] if b is None else rep[g, b]).tolist() == want, (g, b)


def test_one_segment_is_the_bootstrap_rule_with_and_without_weights():
    n = 600
    terms, _, sess = _random_case(n, 1, 5)
    ids = np.zeros(n, np.int64)
    sums, rep = evaluation.segment_model(terms, ids, 1, sess, B=7, seed=3)
    assert np.array_equal(rep[0].view(np.uint64), evaluation.bootstrap_model(terms, sess, 7, 3).view(np.uint64))
    # all weights 1: the rule of 10.2 by hand
    cols = np.concatenate([np.ones((n, 1)), terms[:, [0, 2, 1, 6, 4, 5]]], axis=1)
    total = np.zeros(7)
    for g0 in range(0, n, 256):
        acc = np.zeros(7)
        for q in range(g0, min(g0 + 256, n)):
            acc = acc + 1.0 * cols[q]
        total = total + acc
    assert np.array_equal(sums[0].view(np.uint64), total.view(np.uint64))
    # a segment's replicates do not depend on S where its queries do not change
    wide = np.where(np.arange(n) % 3 == 0, 0, 1 + np.arange(n) % 5)
    narrow = np.where(np.arange(n) % 3 == 0, 0, 1)
    a, ra = evaluation.segment_model(terms, wide, 6, sess, B=4, seed=3)
    b, rb = evaluation.segment_model(terms, narrow, 2, sess, B=4, seed=3)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(ra[0].view(np.uint64), rb[0].view(np.uint64))
    # nothing to add
    assert np.array_equal(evaluation.segment_model(np.zeros((0, 7)), [], 3), np.zeros((3, 7)))
    with pytest.raises(ValueError):
        evaluation.segment_model(terms, np.full(n, 2), 2)


def test_spec_names():
    names = lambda spec: evaluation._spec(spec)[4]
    assert names(dict(by="position", n=4)) == ["t=1", "t=2", "t=3", "t>=4"]
    assert names(dict(by="position", n=1)) == ["t>=1"]
    assert names(dict(by="target_count", bounds=[1, 10, 100])) == ["count<1", "1<=count<10", "10<=count<100", "count>=100"]
    assert names(dict(by="current_count", bounds=[5])) == ["count<5", "count>=5"]
    assert names(dict(by="labels", labels=[0, 1], n=2)) == ["label=0", "label=1"]
    assert names(dict(by="labels", labels=[0, 1], n=2, names=["phone", "desktop"])) == ["phone", "desktop"]
    with pytest.raises(ValueError):
        names(dict(by="labels", labels=[0, 1], n=2, names=["one"]))
    with pytest.raises(ValueError):
        names(dict(by="labels", labels=[0, 70000], n=2))
    seg, nm, keep = evaluation._segments(dict(by="target_count", bounds=[1, 10]))
    assert (seg.mode, seg.segments, seg.n_labels, seg.reserved) == (capi.SEG_TARGET_COUNT, 3, 0, 0) and len(nm) == 3


LEVELS = [(1 - 0.95) / 2, 1 - (1 - 0.95) / 2]   # the percentile interval at ci = 0.95


def _segment_report(mrr_by_replicate, weights, n, seed=3):
    w = np.asarray(weights, np.float64)
    sums = np.zeros((len(w), 7))
    sums[:, 0] = w
    sums[:, 1] = np.asarray(mrr_by_replicate, np.float64) * w
    rep = {"name": "x", "qty_evaluations": n, "Mrr@20": 0.5, "Precision@20": 0.0, "Recall@20": 0.0, "F1score@20": 0.0}
    return evaluation._with_bootstrap(rep, sums, 20, seed, 0.95)


def test_compare_pairs_segments_with_each_other_and_with_the_total():
    w_all, w_seg = [10.0, 8.0, 12.0, 9.0], [4.0, 0.0, 6.0, 3.0]
    a = dict(_segment_report([0.5, 0.25, 0.75, 0.5], w_all, 100), segments=[_segment_report([0.75, 0.0, 0.5, 1.0], w_seg, 40)])
    b = dict(_segment_report([0.25, 0.5, 0.25, 0.5], w_all, 100), segments=[_segment_report([0.25, 0.0, 0.75, 0.5], w_seg, 40)])
    c = evaluation.compare(a, b, "Mrr", segment=0)
    d = np.array([0.5, -0.25, 0.5])   # replicate by replicate, the segment's empty replicate left out
    assert c["replicates"] == 3 and c["p_better"] == 2 / 3
    assert c["ci"] == tuple(np.quantile(d, LEVELS).tolist())
    assert c == evaluation.compare(a["segments"][0], b["segments"][0], "Mrr")
    # a segment against the total of the same report: different query counts, the same weights' replicates
    c = evaluation.compare(a, a, "Mrr", segment=(0, None))
    assert c["replicates"] == 3 and c["ci"] == tuple(np.quantile(np.array([0.25, -0.25, 0.5]), LEVELS).tolist())
    assert evaluation.compare(a, a, "Mrr", segment=(None, 0))["p_better"] == 1 / 3
    assert evaluation.compare(a, b, "Mrr") == evaluation.compare(a, b, "Mrr", segment=None)
    with pytest.raises(ValueError):
        evaluation.compare(a, {"qty_evaluations": 100, "Mrr@20": 0.5}, "Mrr", segment=0)
    with pytest.raises(ValueError):
        evaluation.compare(a, dict(b, segments=[_segment_report([0.5] * 4, w_seg, 40, seed=4)]), "Mrr", segment=0)


def test_cli_parses_the_segments_option_and_backtest_refuses_labels():
    a = hpo.parser().parse_args(["example.toml", "--segments", "position:8"])
    assert a.segments == dict(by="position", n=8)
    a = hpo.parser().parse_args(["example.toml", "--segments", "target_count:1,10,100"])
    assert a.segments == dict(by="target_count", bounds=[1, 10, 100])
    assert hpo.parse_segments("current_count:5") == dict(by="current_count", bounds=[5])
    assert hpo.parser().parse_args(["example.toml"]).segments is None
    for bad in ("labels:3", "position:x", "position", "count:1"):
        with pytest.raises(argparse.ArgumentTypeError):
            hpo.parse_segments(bad)
    report = {"segments": [{"name": "t=1", "qty_evaluations": 3, "Mrr@20": 0.5, "F1score@20": 0.25, "sums": {}},
                           {"name": "t>=2", "qty_evaluations": 0, "Mrr@20": 0.0, "F1score@20": 0.0, "sums": {}}]}
    lines = hpo.segment_table(report)
    assert len(lines) == 3 and lines[0].split() == ["segment", "evaluations", "Mrr@20", "F1score@20"]
    assert lines[1].split() == ["t=1", "3", "0.500000", "0.250000"] and lines[2].split()[:2] == ["t>=2", "0"]
    ev = (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0))
    with pytest.raises(ValueError, match="labels"):
        prepare.backtest(ev, [dict(k=50, m=500, max_items_in_session=2)], 500, 1.0, folds=2, segments=dict(by="labels", labels=[0], n=1))
