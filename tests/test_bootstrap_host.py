"""Bootstrap confidence intervals: what runs without a GPU -- the ABI's symbols and refusals, the weight rule in C against the rule in NumPy,
its thresholds and moments, the model's spread against the analytic standard error, compare() and the search CLI's options."""
import ctypes as C
from decimal import Decimal, getcontext

import numpy as np
import pytest

from serenade_amd import capi, evaluation, hpo


def _trial(**kw):
    t = dict(k=50, m=500, how_many=20, max_items_in_session=2, length=20)
    t.update(kw)
    return evaluation._trial(t)


def test_bootstrap_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in ("srn_evaluate_bootstrap", "srn_bootstrap_weights"):
        assert name in capi.SYMBOLS
        assert getattr(L, name).argtypes == capi.SYMBOLS[name][1]
    assert C.sizeof(capi.Bootstrap) == 16
    assert (capi.MAX_BOOTSTRAP, capi.BOOTSTRAP_SUMS) == (4096, 7)
    assert len(evaluation.BOOTSTRAP_SUMS) + 1 == capi.BOOTSTRAP_SUMS


def test_bootstrap_arguments_are_refused_before_the_missing_set_is_reached():
    L = capi.lib()
    r, t = capi.EvalResult(), _trial()
    rep = np.zeros((capi.MAX_BOOTSTRAP + 1, 7))

    def call(boot, rep_ptr=capi.ptr(rep), trial=t):
        return L.srn_evaluate_bootstrap(None, C.byref(trial), 1, C.byref(boot) if boot is not None else None, C.byref(r), rep_ptr, None)
    assert call(capi.Bootstrap(0, 0, 0)) == capi.SRN_EINVAL
    assert b"replicates" in L.srn_last_error()
    assert call(capi.Bootstrap(0, 64, 1)) == capi.SRN_EINVAL
    assert b"flags" in L.srn_last_error()
    assert call(None) == capi.SRN_EINVAL
    assert call(capi.Bootstrap(0, 64, 0), rep_ptr=None) == capi.SRN_EINVAL
    assert b"null argument" in L.srn_last_error()
    assert call(capi.Bootstrap(0, capi.MAX_BOOTSTRAP + 1, 0)) == capi.SRN_ERANGE
    assert b"SRN_MAX_BOOTSTRAP" in L.srn_last_error()
    # srn_evaluate's own refusals stay, and a good call gets as far as the missing set
    assert call(capi.Bootstrap(0, 64, 0), trial=_trial(max_items_in_session=capi.MAX_SESSION_LEN + 1)) == capi.SRN_ERANGE
    assert call(capi.Bootstrap(0, 64, 0), trial=_trial(k=0)) == capi.SRN_EINVAL
    assert call(capi.Bootstrap(0, capi.MAX_BOOTSTRAP, 0)) == capi.SRN_EINVAL
    assert b"null evaluation set" in L.srn_last_error()
    with pytest.raises(capi.SerenadeError) as e:
        evaluation.evaluate(None, [dict(k=50, m=500, max_items_in_session=2)], bootstrap=capi.MAX_BOOTSTRAP + 1)
    assert e.value.code == capi.SRN_ERANGE
    assert L.srn_bootstrap_weights(0, 0, 0, 4, None) == capi.SRN_EINVAL
    assert L.srn_bootstrap_weights(0, 0, 0, 0, None) == capi.SRN_OK


def test_thresholds_are_the_rounded_poisson_cdf():
    getcontext().prec = 60
    e_inv = 1 / Decimal(1).exp()
    cdf, term, want = Decimal(0), Decimal(1), []
    for i in range(12):
        if i:
            term /= i
        cdf += term * e_inv
        want.append(int((cdf * 2 ** 32).to_integral_value(rounding="ROUND_HALF_EVEN")))
    assert list(evaluation.BOOTSTRAP_THRESHOLDS) == want
    assert want[-1] < 2 ** 32   # (a weight of 12 stays possible: u can exceed the last threshold)


def test_c_weights_equal_the_numpy_rule():
    L = capi.lib()
    for seed in (0, 1, 2 ** 63 + 5):
        for b in (0, 1, 4095):
            model = evaluation.bootstrap_weights(seed, b + 1, 10000)[b]
            out = np.full(10000, 255, np.uint8)
            assert L.srn_bootstrap_weights(seed, b, 0, len(out), capi.ptr(out)) == 0
            assert np.array_equal(out, model), (seed, b)
            part = np.full(1500, 255, np.uint8)   # a first_session offset names the same sessions
            assert L.srn_bootstrap_weights(seed, b, 8500, len(part), capi.ptr(part)) == 0
            assert np.array_equal(part, model[8500:]), (seed, b)
            assert np.array_equal(evaluation.bootstrap_weights(seed, b + 1, 1500, first_session=8500)[b], model[8500:])
    assert int(evaluation.bootstrap_weights(1, 64, 10000).max()) <= 12


def test_a_replicates_weights_do_not_depend_on_b():
    small, large = evaluation.bootstrap_weights(7, 65, 3000), evaluation.bootstrap_weights(7, 1000, 3000)
    assert np.array_equal(small, large[:65])
    assert not np.array_equal(large[0], large[1]) and not np.array_equal(large[0], evaluation.bootstrap_weights(8, 1, 3000)[0])


def test_weight_moments_are_poisson_ones():
    w = evaluation.bootstrap_weights(1, 256, 4000).astype(np.float64)
    # N = 1 024 000 draws of variance 1: 4 sigma / sqrt(N) = 0.004 for the mean; the variance's own error is sqrt(2 / N) * 4 = 0.006 (the cut at 12 moves neither by 1e-8)
    assert abs(w.mean() - 1.0) <= 0.01, w.mean()
    assert abs(w.var() - 1.0) <= 0.01, w.var()


@pytest.mark.parametrize("seed", [0, 1, 7, 12345])
def test_replicate_spread_is_the_analytic_standard_error(seed):
    n, B = 4000, 2000
    terms = np.zeros((n, 7))
    terms[:, 0] = np.random.default_rng(0).choice([0.0, 1.0, 0.5, 1.0 / 3.0, 0.25], size=n)   # an Mrr-like term, one query per session
    rep = evaluation.bootstrap_model(terms, np.arange(n), B, seed)
    assert np.array_equal(rep[:, 0], evaluation.bootstrap_weights(seed, B, n).sum(axis=1, dtype=np.float64))
    assert np.all(rep[:, 2:] == 0.0)
    spread = (rep[:, 1] / rep[:, 0]).std(ddof=1)
    se = terms[:, 0].std(ddof=1) / np.sqrt(n)
    print("seed %d: replicate spread / analytic standard error = %.4f" % (seed, spread / se))
    assert abs(spread / se - 1.0) <= 0.10, (seed, spread, se)


def test_model_adds_in_groups_of_256_and_clusters_by_session():
    rng = np.random.default_rng(3)
    n = 700
    terms = rng.random((n, 7))
    sess = np.sort(rng.integers(0, 90, size=n)) * 2 + 5   # gaps: indices that give no query
    rep = evaluation.bootstrap_model(terms, sess, 9, 11)
    w = evaluation.bootstrap_weights(11, 9, int(sess.max()) + 1).astype(np.float64)
    cols = [0, 2, 1, 6, 4, 5]   # TERMS -> mrr, ndcg, hit_rate, popularity, precision, recall
    for b in (0, 8):
        want = [0.0] * 7
        for g0 in range(0, n, 256):
            acc = [0.0] * 7
            for q in range(g0, min(g0 + 256, n)):
                wq = float(w[b, sess[q]])
                acc[0] = acc[0] + wq
                for j, c in enumerate(cols):
                    acc[1 + j] = acc[1 + j] + wq * float(terms[q, c])
            want = [t + a for t, a in zip(want, acc)]
        assert rep[b].tolist() == want
    assert np.array_equal(evaluation.bootstrap_model(np.zeros((0, 7)), [], 5, 0), np.zeros((5, 7)))
    assert evaluation.session_of_query({4: [1], 9: [1, 2, 3], 2: [5], 7: [5, 6]}).tolist() == [1, 1, 3]


LEVELS = [(1 - 0.95) / 2, 1 - (1 - 0.95) / 2]   # the percentile interval at ci = 0.95


def _report(mrr_by_replicate, weights, seed=3, n=100, ci=0.95, length=20):
    w = np.asarray(weights, np.float64)
    sums = np.zeros((len(w), 7))
    sums[:, 0] = w
    sums[:, 1] = np.asarray(mrr_by_replicate, np.float64) * w
    sums[:, 5], sums[:, 6] = 0.5 * w, 0.25 * w
    ok = w > 0
    rep = {"qty_evaluations": n, "Mrr@%d" % length: float(np.mean(np.asarray(mrr_by_replicate)[ok])) if ok.any() else 0.0, "Precision@%d" % length: 0.5,
           "Recall@%d" % length: 0.25, "F1score@%d" % length: 1.0 / 3.0}
    return evaluation._with_bootstrap(rep, sums, length, seed, ci)


def test_compare_pairs_replicates_and_refuses_unpaired_reports():
    w = [4.0, 2.0, 0.0, 8.0, 5.0]
    a = _report([0.5, 0.25, 0.9, 0.75, 0.5], w)
    b = _report([0.25, 0.5, 0.1, 0.25, 0.5], w)
    assert a["bootstrap"]["empty_replicates"] == 1 and a["bootstrap"]["replicates"] == 5
    c = evaluation.compare(a, b)
    d = np.array([0.25, -0.25, 0.5, 0.0])   # replicate by replicate, the empty one left out
    assert c["replicates"] == 4 and c["p_better"] == 0.5
    assert c["ci"] == tuple(np.quantile(d, LEVELS).tolist())
    assert c["delta"] == a["Mrr@20"] - b["Mrr@20"]
    assert evaluation.compare(b, a)["p_better"] == 0.25
    same = evaluation.compare(a, a)
    assert same == {"delta": 0.0, "ci": (0.0, 0.0), "p_better": 0.0, "replicates": 4}
    # pairing is by replicate, not by value: the same values in another order are another comparison
    shuffled = _report([0.25, 0.5, 0.9, 0.5, 0.75], w)
    assert evaluation.compare(a, shuffled)["ci"] != (0.0, 0.0)
    assert a["Mrr@20_ci"] == tuple(np.quantile([0.5, 0.25, 0.75, 0.5], LEVELS).tolist())
    assert a["F1score@20_ci"] == (2 * 0.125 / 0.75,) * 2 and a["Precision@20_ci"] == (0.5, 0.5)
    assert "Coverage@20_ci" not in a
    for other in (_report([0.5] * 5, w, seed=4), _report([0.5] * 4, w[:4]), _report([0.5] * 5, w, n=101)):
        with pytest.raises(ValueError):
            evaluation.compare(a, other)
    with pytest.raises(ValueError):
        evaluation.compare(a, {"qty_evaluations": 100, "Mrr@20": 0.5})
    with pytest.raises(ValueError):
        evaluation.compare(a, b, metric="Coverage")
    empty = _report([0.0, 0.0], [0.0, 0.0])
    assert empty["Mrr@20_ci"] == (0.0, 0.0) and empty["bootstrap"]["empty_replicates"] == 2
    assert evaluation.compare(empty, empty) == {"delta": 0.0, "ci": (0.0, 0.0), "p_better": 0.0, "replicates": 0}


def test_cli_parses_the_bootstrap_options():
    a = hpo.parser().parse_args(["example.toml", "--bootstrap", "256", "--seed", "9", "--ci", "0.9", "--ci-csv", "intervals.csv"])
    assert (a.bootstrap, a.seed, a.ci, a.ci_csv) == (256, 9, 0.9, "intervals.csv")
    a = hpo.parser().parse_args(["example.toml"])
    assert (a.bootstrap, a.seed, a.ci, a.ci_csv) == (0, 0, 0.95, None)
    with pytest.raises(ValueError):
        evaluation.evaluate(None, [], bootstrap=-1)
    with pytest.raises(ValueError):
        evaluation.evaluate(None, [], bootstrap=8, ci=1.0)
