"""Visitor-clustered bootstrap of the click feedback log (srn_feedback_bootstrap_*, serving.feedback_bootstrap_*): what can be checked without a
GPU -- the symbols and the refusals that come before any device work, the weight rule on the host against its NumPy statement and against the evaluation
bootstrap's, the replicate sums of a stream small enough to write out, the spread the replicates show, and feedback_compare."""
import ctypes as C

import numpy as np
import pytest

from serenade_amd import capi, evaluation
from serenade_amd.serving import (feedback_bootstrap_model, feedback_bootstrap_weights, feedback_compare, feedback_fold, feedback_metrics,
                                  feedback_replicate_values)

NONE, FILLED = capi.FEEDBACK_NONE, capi.FEEDBACK_FILLED
NEW_SYMBOLS = ["srn_feedback_bootstrap_enable", "srn_feedback_bootstrap_disable", "srn_feedback_bootstrap_info", "srn_feedback_bootstrap_read",
               "srn_feedback_bootstrap_weights"]
M64 = 2**64 - 1


def test_new_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1] and fn.restype == capi.SYMBOLS[name][0], name
    assert capi.FEEDBACK_BOOTSTRAP_MAX_ROW_CAP == 64 and capi.MAX_BOOTSTRAP == 4096


def test_null_logs_and_null_arrays_are_refused():
    L = capi.lib()
    B, seed = C.c_uint32(7), C.c_uint64(7)
    assert L.srn_feedback_bootstrap_enable(None, 16, 1) == capi.SRN_EINVAL
    assert b"srn_feedback_bootstrap_enable" in L.srn_last_error()
    assert L.srn_feedback_bootstrap_disable(None) == capi.SRN_EINVAL
    assert L.srn_feedback_bootstrap_info(None, C.byref(B), C.byref(seed)) == capi.SRN_EINVAL and (B.value, seed.value) == (7, 7)
    out = np.full(4, 9, np.uint64)
    assert L.srn_feedback_bootstrap_read(None, capi.ptr(out), None, None, 4, 1) == capi.SRN_EINVAL and (out == 9).all()
    one, w = np.ones(1, np.uint64), np.full(1, 9, np.uint8)
    assert L.srn_feedback_bootstrap_weights(1, 0, None, None, 0, None) == capi.SRN_OK                      # n = 0
    for args in ((None, capi.ptr(one), capi.ptr(w)), (capi.ptr(one), None, capi.ptr(w)), (capi.ptr(one), capi.ptr(one), None)):
        assert L.srn_feedback_bootstrap_weights(1, 0, args[0], args[1], 1, args[2]) == capi.SRN_EINVAL
    assert w[0] == 9


def host_weights(seed, B, hi, lo):
    hi, lo = capi.as_u64(hi), capi.as_u64(lo)
    out = np.full((B, len(hi)), 255, np.uint8)
    for b in range(B):
        row = np.full(len(hi), 255, np.uint8)
        capi.check(capi.lib().srn_feedback_bootstrap_weights(seed, b, capi.ptr(hi), capi.ptr(lo), len(hi), capi.ptr(row)))
        out[b] = row
    return out


def test_the_host_rule_is_the_numpy_rule_bit_for_bit():
    rng = np.random.default_rng(3)
    r = lambda n: rng.integers(0, 2**64, n, dtype=np.uint64)   # noqa: E731
    cases = {"random": (r(500), r(500)),
             "hi only": (r(300), np.full(300, 0x1234_5678_9ABC_DEF0, np.uint64)),
             "lo only": (np.full(300, 0xFEDC_BA98_7654_3210, np.uint64), r(300)),
             "one bit of hi": (np.uint64(1) << np.arange(64, dtype=np.uint64), np.zeros(64, np.uint64)),
             "one bit of lo": (np.zeros(64, np.uint64), np.uint64(1) << np.arange(64, dtype=np.uint64)),
             "key 0": (np.zeros(1, np.uint64), np.zeros(1, np.uint64))}
    for name, (hi, lo) in cases.items():
        for seed in (0, 1, 0xDEADBEEFCAFEF00D):
            got, want = host_weights(seed, 9, hi, lo), feedback_bootstrap_weights(seed, 9, (hi, lo))
            assert got.dtype == want.dtype == np.uint8 and np.array_equal(got, want), (name, seed)
            assert int(got.max()) <= 12
    # row b does not depend on B, and a later replicate is what first_replicate says
    hi, lo = cases["random"]
    assert np.array_equal(feedback_bootstrap_weights(5, 40, (hi, lo))[:9], feedback_bootstrap_weights(5, 9, (hi, lo)))
    assert np.array_equal(feedback_bootstrap_weights(5, 40, (hi, lo))[33:], feedback_bootstrap_weights(5, 7, (hi, lo), first_replicate=33))
    # keys that differ in one half alone fold to different words, and weigh differently somewhere
    for name in ("hi only", "lo only", "one bit of hi", "one bit of lo"):
        hi, lo = cases[name]
        assert len(np.unique(feedback_fold((hi, lo)))) == len(hi), name
        w = feedback_bootstrap_weights(1, 64, (hi, lo))
        assert len(np.unique(w, axis=1).T) > len(hi) // 2, name


def test_keys_with_hi_zero_tie_the_rule_to_the_evaluation_bootstraps():
    """fold((0, s)) = mix64(0x9E37...) ^ s: the log weighs visitor (0, s) as srn_bootstrap_weights weighs session s ^ mix64(0x9E3779B97F4A7C15)"""
    c = int(evaluation._mix64(np.array([0x9E3779B97F4A7C15], np.uint64))[0])
    L = capi.lib()
    for seed, b in ((0, 0), (12345, 3), (M64, 4095)):
        for s0 in (0, 1, 1 << 40, M64 - 200):
            lo = np.arange(s0, s0 + 100, dtype=np.uint64)
            got = np.zeros(100, np.uint8)
            capi.check(L.srn_feedback_bootstrap_weights(seed, b, capi.ptr(np.zeros(100, np.uint64)), capi.ptr(lo), 100, capi.ptr(got)))
            for i in (0, 1, 50, 99):   # (consecutive lo are not consecutive sessions: one call of the evaluation's entry point each)
                one = np.zeros(1, np.uint8)
                capi.check(L.srn_bootstrap_weights(seed, b, (s0 + i) ^ c, 1, capi.ptr(one)))
                assert one[0] == got[i], (seed, b, s0, i)
            want = np.array([evaluation.bootstrap_weights(seed, b + 1, 1, first_session=(s0 + i) ^ c)[b, 0] for i in range(100)], np.uint8)
            assert np.array_equal(got, want)


# ---- the replicate sums ----
A, Bv, Cv = (7, 11), (7, 12), (9, 11)                   # three visitors: two agree in hi, two in lo
W = {A: [2, 1, 0, 0], Bv: [2, 1, 2, 1], Cv: [1, 1, 1, 5]}   # w(seed 5, b = 0..3, visitor)


def hand_stream():
    vis = [A, A, Bv, Cv, A, Cv]
    ranks = np.array([NONE, 2, 0, 3 | FILLED, 2, NONE], np.uint32)   # first seen | model hit at 2 | miss | filled hit at 3 | model hit at 2 | no consent
    return ranks, (np.array([v[0] for v in vis], np.uint64), np.array([v[1] for v in vis], np.uint64))


def test_a_stream_of_six_requests_written_out():
    for v, w in W.items():
        assert host_weights(5, 4, [v[0]], [v[1]])[:, 0].tolist() == w, v
    ranks, keys = hand_stream()
    m = feedback_bootstrap_model(ranks, keys, 4, 5, 3)
    assert m["observed"].dtype == np.uint64 and m["hist_model"].shape == m["hist_filled"].shape == (4, 4)
    assert m["observed"].tolist() == [7, 4, 3, 6]                                        # 2 w_A + w_B + w_C: the miss counts, NONE does not
    assert m["hist_model"].tolist() == [[0, 0, 4, 0], [0, 0, 2, 0], [0, 0, 0, 0], [0, 0, 0, 0]]   # [b][2] = 2 w_A
    assert m["hist_filled"].tolist() == [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 1], [0, 0, 0, 5]]  # [b][3] = w_C: the FILLED bit routes the hit
    # the order of the requests and the cut into calls do not matter; replicate b does not depend on B
    p = np.array([5, 3, 1, 0, 4, 2])
    again = feedback_bootstrap_model(ranks[p], (keys[0][p], keys[1][p]), 4, 5, 3)
    wide = feedback_bootstrap_model(ranks, keys, 7, 5, 3)
    for k in m:
        assert np.array_equal(again[k], m[k]) and np.array_equal(wide[k][:4], m[k]), k
        parts = [feedback_bootstrap_model(ranks[a:b], (keys[0][a:b], keys[1][a:b]), 4, 5, 3)[k] for a, b in ((0, 1), (1, 4), (4, 6))]
        assert np.array_equal(sum(parts), m[k]), k


def test_requests_that_are_not_observed_add_nothing():
    hi, lo = np.arange(1, 51, dtype=np.uint64), np.arange(50, dtype=np.uint64)
    m = feedback_bootstrap_model(np.full(50, NONE, np.uint32), (hi, lo), 8, 1, 5)
    assert not m["observed"].any() and not m["hist_model"].any() and not m["hist_filled"].any()
    m = feedback_bootstrap_model(np.zeros(0, np.uint32), (hi[:0], lo[:0]), 8, 1, 5)
    assert m["observed"].shape == (8,) and not m["observed"].any()
    ranks = np.full(50, NONE, np.uint32)
    ranks[7], ranks[9] = 5, 1 | FILLED
    m = feedback_bootstrap_model(ranks, (hi, lo), 8, 1, 5)
    w = feedback_bootstrap_weights(1, 8, (hi, lo)).astype(np.uint64)
    assert np.array_equal(m["observed"], w[:, 7] + w[:, 9]) and m["observed"].any()
    assert np.array_equal(m["hist_model"][:, 5], w[:, 7]) and int(m["hist_model"].sum()) == int(w[:, 7].sum())
    assert np.array_equal(m["hist_filled"][:, 1], w[:, 9]) and int(m["hist_filled"].sum()) == int(w[:, 9].sum())
    with pytest.raises(ValueError):
        feedback_bootstrap_model(np.array([6], np.uint32), (hi[:1], lo[:1]), 8, 1, 5)   # a rank above row_cap


def test_the_replicates_spread_as_a_proportions_standard_error():
    """One request per visitor, 20 000 visitors, hit probability 0.3: the replicates' hit_rate must spread as sqrt(p (1 - p) / n), to 10 % -- the standard deviation
    estimated from B = 2000 replicates carries a relative error of about 1 / sqrt(2 B) = 1.6 %, and a Poisson(1) weight cut at 12 differs from Poisson(1) by 1e-9.
    (Seed 11 on these keys gives a ratio of 1.002.)"""
    n, p, B = 20_000, 0.3, 2000
    rng = np.random.default_rng(1)
    hi, lo = rng.integers(1, 2**63, n).astype(np.uint64), rng.integers(1, 2**63, n).astype(np.uint64)
    ranks = np.where(rng.random(n) < p, 1, 0).astype(np.uint32)
    m = feedback_bootstrap_model(ranks, (hi, lo), B, 11, 1)
    stats = {"bootstrap": dict(m, replicates=B, seed=11, ci=0.95)}
    v, ok = feedback_replicate_values(stats, "hit_rate")
    assert ok.all() and np.array_equal(v, m["hist_model"][:, 1] / m["observed"])
    want = np.sqrt(p * (1 - p) / n)
    print("std of hit_rate over the replicates %.6f, sqrt(p (1 - p) / n) %.6f, ratio %.4f" % (v.std(), want, v.std() / want))
    assert abs(v.std() / want - 1.0) <= 0.10
    assert abs(v.mean() - ranks.mean()) <= 3 * want / np.sqrt(B) + 1e-4                   # ... around the point estimate
    assert abs(m["observed"].mean() / n - 1.0) <= 3.0 / np.sqrt(n * B) * 3                 # the weights' mean is 1 (variance 1): 9 standard errors


# ---- feedback_compare ----
def stats_of(hist, observed, seed=1, ci=0.5):
    """a stats() dict from histograms [B + 1][R] and observed [B + 1]: the first row is the point estimate's, the others the replicates'"""
    hist, observed = np.asarray(hist, np.uint64), np.asarray(observed, np.uint64)
    zero = np.zeros_like(hist[1:])
    out = dict(feedback_metrics(hist[0], zero[0], int(observed[0])), observed=int(observed[0]))
    out["bootstrap"] = {"replicates": len(hist) - 1, "seed": seed, "ci": ci, "observed": observed[1:], "hist_model": hist[1:], "hist_filled": zero}
    return out


def test_compare_on_a_case_stated_by_hand():
    # ranks 1 and 2 only: mrr = (h1 + h2 / 2) / observed.  point: a 6/8, b 4/8; replicates of a: 4/8, 8/8, 4/8, 6/8; of b: 4/8, 4/8, 6/8, 0 observed
    a = stats_of([[0, 4, 4], [0, 2, 4], [0, 8, 0], [0, 4, 0], [0, 4, 4]], [8, 8, 8, 8, 8])
    b = stats_of([[0, 2, 4], [0, 2, 4], [0, 4, 0], [0, 4, 4], [0, 0, 0]], [8, 8, 8, 8, 0])
    assert (a["mrr"], b["mrr"]) == (0.75, 0.5)
    va, oka = feedback_replicate_values(a, "mrr")
    vb, okb = feedback_replicate_values(b, "mrr")
    assert va.tolist() == [0.5, 1.0, 0.5, 0.75] and oka.all() and vb.tolist() == [0.5, 0.5, 0.75, 0.0] and okb.tolist() == [True, True, True, False]
    c = feedback_compare(a, b)                           # differences 0, 0.5, -0.25 over the three replicates that observed something on both sides
    assert c["delta"] == 0.25 and c["replicates"] == 3 and c["p_better"] == 1 / 3 and c["paired"] is False
    assert c["ci"] == (-0.125, 0.25)                    # the quartiles of (-0.25, 0, 0.5) at ci = 0.5, linear between the order statistics
    h = feedback_compare(a, b, metric="hit_rate")        # hits / observed: a 1 | .75, 1, .5, 1; b .75 | .75, .5, 1, -: differences 0, .5, -.5
    assert h["delta"] == 0.25 and h["ci"] == (-0.25, 0.25) and h["p_better"] == 1 / 3
    assert feedback_compare(a, a)["paired"] is True and feedback_compare(a, a)["ci"] == (0.0, 0.0) and feedback_compare(a, a)["p_better"] == 0.0
    # equal observed arrays pair, whatever the histograms are
    b2 = stats_of([[0, 2, 4], [0, 2, 4], [0, 4, 0], [0, 4, 4], [0, 1, 0]], [8, 8, 8, 8, 8])
    c2 = feedback_compare(a, b2)
    assert c2["paired"] is True and c2["replicates"] == 4
    with pytest.raises(ValueError):
        feedback_compare(a, stats_of([[0, 2, 4]] * 5, [8] * 5, seed=2))
    with pytest.raises(ValueError):
        feedback_compare(a, stats_of([[0, 2, 4]] * 4, [8] * 4))
    with pytest.raises(ValueError):
        feedback_compare(a, {"mrr": 0.5})
    with pytest.raises(ValueError):
        feedback_replicate_values(a, "ndcg")
