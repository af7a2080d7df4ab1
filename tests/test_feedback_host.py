"""Click feedback log (srn_feedback_*, serving.feedback_model): what can be checked without a GPU -- the symbols, the argument checks that come before
any device work, and the rule itself as serving.feedback_model states it."""
import ctypes as C

import numpy as np
import pytest

from serenade_amd import capi
from serenade_amd.serving import feedback_metrics, feedback_model

NONE, FILLED = capi.FEEDBACK_NONE, capi.FEEDBACK_FILLED
NEW_SYMBOLS = ["srn_feedback_create", "srn_feedback_free", "srn_feedback_observe_device", "srn_feedback_observe", "srn_feedback_stats", "srn_feedback_histogram",
               "srn_feedback_reset_counters", "srn_feedback_sweep", "srn_feedback_get"]
COUNTERS = ("requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored")
NOW, IDLE = 1_700_000_000, 1200


def test_new_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1], name
    assert (NONE, FILLED) == (0xFFFFFFFF, 0x80000000)
    assert [n for n, _ in capi.FeedbackStats._fields_][9:] == list(COUNTERS)


def _create(device, capacity, row_cap, ttl, idle, null_out=False):
    h = C.c_void_p()
    return capi.lib().srn_feedback_create(device, capacity, row_cap, ttl, idle, None if null_out else C.byref(h)), h


def test_create_without_a_device_is_enodev():
    rc, h = _create(-1, 100, 21, 0, 0)
    assert rc == capi.SRN_ENODEV and not h.value
    rc, h = _create(10_000, 100, 21, 0, 0)                # no box has that many GPUs
    assert rc == capi.SRN_ENODEV and not h.value


def test_create_refuses_bad_arguments_before_it_looks_for_a_device():
    assert _create(0, 0, 21, 0, 0)[0] == capi.SRN_EINVAL                        # capacity 0
    assert _create(0, 100, 0, 0, 0)[0] == capi.SRN_EINVAL                       # row_cap 0
    assert _create(0, 100, capi.MAX_HOW_MANY + 1, 0, 0)[0] == capi.SRN_ERANGE   # row_cap above SRN_MAX_HOW_MANY
    assert _create(0, 100, 21, 600, 1200)[0] == capi.SRN_EINVAL                 # ttl < idle
    assert _create(0, 100, 21, 600, 0)[0] == capi.SRN_EINVAL                    # ttl below the DEFAULT idle limit of 20 minutes
    assert _create(0, 100, 21, 0, 1801)[0] == capi.SRN_EINVAL                   # the default ttl of 30 minutes below idle
    assert _create(0, 100, 21, 0, 0, null_out=True)[0] == capi.SRN_EINVAL
    assert b"srn_feedback_create" in capi.lib().srn_last_error()


def test_null_handles_are_refused():
    L = capi.lib()
    one, row, cnt, rank = np.ones(1, np.uint64), np.ones(21, np.uint64), np.ones(1, np.uint32), np.zeros(1, np.uint32)
    for n in (1, 0):   # (a NULL log is refused whatever n is)
        assert L.srn_feedback_observe(None, capi.ptr(one), capi.ptr(one), capi.ptr(one), None, n, NOW, capi.ptr(row), None, capi.ptr(cnt), 21, capi.ptr(rank)) == capi.SRN_EINVAL
        assert L.srn_feedback_observe_device(None, capi.ptr(one), capi.ptr(one), capi.ptr(one), None, n, NOW, capi.ptr(row), None, capi.ptr(cnt), 21, capi.ptr(rank),
                                             None) == capi.SRN_EINVAL
    assert rank[0] == 0
    assert L.srn_feedback_stats(None, None) == capi.SRN_EINVAL
    assert L.srn_feedback_histogram(None, None, None, 0) == capi.SRN_EINVAL
    assert L.srn_feedback_reset_counters(None) == capi.SRN_EINVAL
    assert L.srn_feedback_sweep(None, 3, None) == capi.SRN_EINVAL
    c = C.c_uint32()
    assert L.srn_feedback_get(None, 1, 2, 3, None, 0, C.byref(c), None, None) == capi.SRN_EINVAL
    L.srn_feedback_free(None)


class _NeverCalled:
    def __getattr__(self, name):
        raise AssertionError("recommend_batch touched the index (%s) before refusing its inputs" % name)


def test_recommend_batch_refuses_a_row_wider_than_the_log_before_the_library_is_called():
    from serenade_amd.serving import recommend_batch

    class Log:
        row_cap, device = 20, 0
    z = np.zeros(4, np.uint64)
    with pytest.raises(ValueError, match="row_cap"):
        recommend_batch(_NeverCalled(), None, (z, z), z, k=10, m=10, how_many=21, feedback=Log())


# ---- the rule ----
def keys_of(ks):
    return np.array([k >> 64 for k in ks], np.uint64), np.array([k & (2**64 - 1) for k in ks], np.uint64)


def step(state, key, item, row, count=None, consent=True, scores=None, now=NOW, how_many=None):
    """one request: -> its rank"""
    how_many = how_many or max(len(row), 1)
    ids = np.zeros((1, how_many), np.uint64)
    ids[0, :len(row)] = row
    sc = None
    if scores is not None:
        sc = np.zeros((1, how_many))
        sc[0, :len(scores)] = scores
    cnt = np.array([len(row) if count is None else count], np.uint32)
    ranks, ctr = feedback_model(state, keys_of([key]), [item], [consent], ids, cnt, sc, now, IDLE)
    return int(ranks[0]), ctr


def test_hits_misses_and_empty_rows():
    st = {}
    row = [11, 12, 13, 14, 15]
    r, ctr = step(st, 5, 1, row)
    assert r == NONE and ctr["first_seen"] == 1 and ctr["stored"] == 1 and ctr["observed"] == 0
    assert st[5][1] == 5 and st[5][2] == NOW and st[5][0].tolist() == row
    assert step(st, 5, 11, row)[0] == 1                     # rank 1
    r, ctr = step(st, 5, 15, row)
    assert r == 5 and ctr["hist_model"][5] == 1 and ctr["hits_model"] == 1 and ctr["hits_filled"] == 0   # the last rank
    r, ctr = step(st, 5, 99, [15, 16])
    assert r == 0 and ctr["observed"] == 1 and ctr["hits_model"] == 0 and not ctr["hist_model"].any()     # a miss
    assert step(st, 5, 99, [15, 16])[0] == 0                # a repeat of the clicked item: the row served for it leaves it out, so a miss
    assert step(st, 5, 15, [], how_many=3)[0] == 1          # only the LAST row counts: 15 was also in the row before it, at rank 5
    r, ctr = step(st, 5, 7, [1, 2])
    assert r == 0 and ctr["observed"] == 1                  # a row of count 0: an observed miss
    # a row that was not served (count 0xFFFFFFFF) is stored as an empty one: positions >= count are never read
    ids = np.full((1, 4), 7, np.uint64)
    ranks, _ = feedback_model(st, keys_of([5]), [2], None, ids, np.array([NONE], np.uint32), None, NOW, IDLE)
    assert ranks[0] == 2 and len(st[5][0]) == 0 and st[5][1] == 0
    ranks, ctr = feedback_model(st, keys_of([5]), [7], None, ids, np.array([2], np.uint32), None, NOW, IDLE)
    assert ranks[0] == 0 and ctr["observed"] == 1 and st[5][0].tolist() == [7, 7]
    # id 0 is an id like any other
    assert step(st, 9, 1, [3, 0, 4])[0] == NONE and step(st, 9, 0, [3])[0] == 2


def test_filled_entries_are_flagged_beyond_the_model_count():
    st = {}
    row, sc = [1, 2, 3, 4, 5], [0.9, 0.5, 0.1, -np.inf, -np.inf]
    step(st, 1, 100, row, scores=sc)
    assert st[1][1] == 3
    r, ctr = step(st, 1, 3, row, scores=sc)
    assert r == 3 and ctr["hits_model"] == 1 and ctr["hist_model"][3] == 1 and ctr["hits_filled"] == 0     # rank n_model: a model entry
    r, ctr = step(st, 1, 4, row, scores=sc)
    assert r == (4 | FILLED) and ctr["hits_filled"] == 1 and ctr["hist_filled"][4] == 1 and ctr["hits_model"] == 0
    assert step(st, 1, 77, row, scores=sc)[0] == 0          # a miss carries no flag
    step(st, 1, 100, row)                                   # no scores: every entry is a model entry
    assert st[1][1] == 5 and step(st, 1, 5, row)[0] == 5


def test_a_request_without_consent_touches_nothing():
    st = {}
    hi, lo = keys_of([3, 3, 3])
    ids = np.array([[10, 11], [20, 21], [30, 31]], np.uint64)
    ranks, ctr = feedback_model(st, (hi, lo), [1, 20, 11], [1, 0, 1], ids, np.full(3, 2, np.uint32), None, NOW, IDLE)
    assert ranks.tolist() == [NONE, NONE, 2]                # the third request is scored against the FIRST row: the second one was never stored
    assert (ctr["no_consent"], ctr["first_seen"], ctr["observed"], ctr["stored"], ctr["requests"]) == (1, 1, 1, 2, 3)
    assert st[3][0].tolist() == [30, 31]
    ranks, _ = feedback_model({}, (hi, lo), [1, 20, 11], [0, 0, 0], ids, np.full(3, 2, np.uint32), None, NOW, IDLE)
    assert ranks.tolist() == [NONE] * 3


def test_the_idle_rule_is_the_session_stores():
    for gap, want in ((IDLE, 1), (IDLE + 1, NONE), (0, 1)):
        st = {}
        step(st, 8, 1, [5, 6], now=NOW)
        r, ctr = step(st, 8, 5, [7], now=NOW + gap)
        assert r == want and ctr["idle_expired"] == (want == NONE) and ctr["observed"] == (want != NONE), gap
        assert st[8][2] == NOW + gap and st[8][0].tolist() == [7]     # stored either way
    st = {}
    step(st, 8, 1, [5, 6], now=NOW)
    assert step(st, 8, 5, [7], now=NOW - 5000)[0] == 1       # a clock that ran backwards is not idle (now > epoch fails)


def test_keys_are_compared_by_all_128_bits():
    st = {}
    ks = [(1 << 64) | 2, (2 << 64) | 2, (1 << 64) | 3, ((1 << 32) + 1 << 64) | 2]
    for i, k in enumerate(ks):
        assert step(st, k, 1, [100 + i])[0] == NONE
    for i, k in enumerate(ks):
        assert step(st, k, 100 + i, [1])[0] == 1
    assert len(st) == 4


def random_stream(seed, n=2000, n_keys=150, how_many=6):
    rng = np.random.default_rng(seed)
    ks = [int(rng.integers(1, 4)) << 64 | (i % 60 + 1) << 32 | i for i in range(n_keys)]   # distinct; many agree in hi
    pick = rng.integers(0, n_keys, n)
    hi, lo = keys_of([ks[i] for i in pick])
    ids = np.stack([rng.permutation(30)[:how_many] for _ in range(n)]).astype(np.uint64)   # distinct ids per row, from a small pool: many hits
    counts = rng.integers(0, how_many + 1, n).astype(np.uint32)
    counts[rng.random(n) < 0.03] = NONE
    sc = np.sort(rng.random((n, how_many)))[:, ::-1].copy()
    tail = rng.integers(0, how_many + 1, n)
    sc[np.arange(how_many)[None, :] >= tail[:, None]] = -np.inf
    items = rng.integers(0, 30, n).astype(np.uint64)
    consent = (rng.random(n) < 0.85).astype(np.uint8)
    return (hi, lo), items, consent, ids, counts, sc


def add(total, ctr):
    for k, v in ctr.items():
        total[k] = total.get(k, 0) + v
    return total


def test_any_cut_into_calls_gives_what_one_call_gives():
    (hi, lo), items, consent, ids, counts, sc = random_stream(7)
    n = len(items)
    one_state = {}
    want_ranks, want = feedback_model(one_state, (hi, lo), items, consent, ids, counts, sc, NOW, IDLE)
    assert want["observed"] > 1000 and want["hits_model"] > 20 and want["hits_filled"] > 20 and want["no_consent"] > 100 and want["first_seen"] > 50
    rng = np.random.default_rng(8)
    for _ in range(3):
        cuts = [0] + sorted(rng.choice(np.arange(1, n), 40, replace=False).tolist()) + [n]
        state, total, ranks = {}, {}, []
        for a, b in zip(cuts, cuts[1:]):
            r, ctr = feedback_model(state, (hi[a:b], lo[a:b]), items[a:b], consent[a:b], ids[a:b], counts[a:b], sc[a:b], NOW, IDLE)
            ranks.append(r)
            add(total, ctr)
        assert np.array_equal(np.concatenate(ranks), want_ranks)
        for k in want:
            assert np.array_equal(total[k], want[k]), k
        assert state.keys() == one_state.keys()
        for k in state:
            assert np.array_equal(state[k][0], one_state[k][0]) and state[k][1:] == one_state[k][1:]


def test_the_counter_identities_hold():
    (hi, lo), items, consent, ids, counts, sc = random_stream(9)
    ranks, c = feedback_model({}, (hi, lo), items, consent, ids, counts, sc, NOW, IDLE)
    assert c["requests"] == len(items) == c["no_consent"] + c["first_seen"] + c["idle_expired"] + c["observed"]
    assert c["stored"] == c["requests"] - c["no_consent"] == int(consent.astype(bool).sum())
    assert c["hits_model"] == int(c["hist_model"].sum()) and c["hits_filled"] == int(c["hist_filled"].sum())
    assert c["hist_model"][0] == 0 and c["hist_filled"][0] == 0
    seen = ranks != NONE
    assert int(seen.sum()) == c["observed"]
    hit = seen & ((ranks & 0x7FFFFFFF) > 0)
    assert int((hit & (ranks & FILLED == 0)).sum()) == c["hits_model"] and int((hit & (ranks & FILLED != 0)).sum()) == c["hits_filled"]
    m = feedback_metrics(c["hist_model"], c["hist_filled"], c["observed"])
    assert m["hit_rate"] == (c["hits_model"] + c["hits_filled"]) / c["observed"]
    assert abs(m["mrr"] - sum(1.0 / (r & 0x7FFFFFFF) for r in ranks[hit].tolist()) / c["observed"]) < 1e-12
    assert abs(m["mrr_model"] + m["mrr_filled"] - m["mrr"]) < 1e-12 and m["hit_rate_model"] + m["hit_rate_filled"] == pytest.approx(m["hit_rate"], rel=1e-15)
    assert feedback_metrics(np.zeros(3), np.zeros(3), 0)["mrr"] == 0.0


def test_a_refusing_log_becomes_a_warning_and_any_other_error_is_raised():
    from serenade_amd import serving

    class Log:
        last_ranks, last_error = "stale", None

        def __init__(self, code):
            self.code = code

        def observe(self, *a, **kw):
            raise capi.SerenadeError(self.code, "no")
    log = Log(capi.SRN_ENOMEM)
    with pytest.warns(RuntimeWarning, match="feedback"):
        serving._observe_served(log, None, None, None, None, None, None, NOW)
    assert log.last_ranks is None and log.last_error.code == capi.SRN_ENOMEM
    log = Log(capi.SRN_EHIP)
    with pytest.raises(capi.SerenadeError):
        serving._observe_served(log, None, None, None, None, None, None, NOW)
