"""The timed batch and replay() without a GPU: the Python models with times= against the same models called once per time step, the properties of
the seeded stream that tests/test_gpu_replay.py relies on, replay()'s cutting against a stub in place of recommend_batch, and the new entry points in the library."""
import numpy as np
import pytest

from serenade_amd import capi, serving
from serenade_amd.serving import feedback_model, harvest_model, replay, replay_plan

import harvest_cases as hc

NEW_SYMBOLS = ["srn_recommend_batch_device_at", "srn_recommend_batch_at", "srn_feedback_observe_device_at", "srn_feedback_observe_at"]
IDLE, TTL = hc.IDLE, hc.TTL
REPLAY_700_25 = (4, 3)          # (calls, boundaries) of the stream under replay(batch=700, every=25): asserted below, used by tests/test_gpu_replay.py


def test_new_symbols_are_bound_and_exported():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1] and fn.restype == capi.SYMBOLS[name][0], name
        assert len(capi.SYMBOLS[name][1]) == len(capi.SYMBOLS[name[:-3]][1]) + 1, name      # the untimed signature + times
    import serenade_amd as sa
    assert sa.replay is replay


def flat(steps):
    """the steps as one request stream: (hi, lo), items, consent, times -- a step's `now` as the time of each of its requests"""
    cat = lambda name: np.concatenate([s[name] for s in steps])
    times = np.concatenate([np.full(len(s["items"]), s["now"], np.uint64) for s in steps])
    return (cat("hi"), cat("lo")), cat("items"), cat("consent"), times


def breaks(steps, per_call):
    """the stream served `per_call` steps to a call -> (breaks inside runs, those beyond the TTL too, visitors with >= 2 breaks): a consenting request whose visitor's
    previous consenting request OF THE SAME CALL is more than IDLE older"""
    n_breaks, n_ttl, per_visitor = 0, 0, {}
    for c in range(0, len(steps), per_call):
        (hi, lo), _, consent, times = flat(steps[c:c + per_call])
        prev = {}
        for j in range(len(times)):
            if not consent[j]:
                continue
            key, t = (int(hi[j]) << 64) | int(lo[j]), int(times[j])
            if key in prev and t > prev[key] and t - prev[key] > IDLE:
                n_breaks += 1
                n_ttl += t - prev[key] > TTL
                per_visitor[key] = per_visitor.get(key, 0) + 1
            prev[key] = t
    return n_breaks, n_ttl, sum(v >= 2 for v in per_visitor.values())


def test_the_stream_breaks_inside_runs():
    steps = hc.make_stream()
    (hi, lo), items, consent, times = flat(steps)
    assert len(items) == 2000 and int(consent.sum()) == 1723 and len(set(zip(hi.tolist(), lo.tolist()))) == 150
    assert breaks(steps, 40) == (109, 34, 12)
    assert breaks(steps, 20)[0] == 59
    assert breaks(steps, 6)[0] == 0
    assert bool((np.diff(times.astype(np.int64)) >= 0).all())


@pytest.mark.parametrize("limit,min_len", [(2, 2), (6, 1)])
@pytest.mark.parametrize("per_call", [40, 20, 7])
def test_harvest_model_with_times_equals_one_call_per_step(limit, min_len, per_call):
    steps = hc.make_stream()
    kw = dict(limit=limit, idle_secs=IDLE, ttl_secs=TTL, min_len=min_len)
    a, b = {}, {}
    for st in steps:
        harvest_model(a, (st["hi"], st["lo"]), st["items"], st["consent"], st["now"], **kw)
    for c in range(0, len(steps), per_call):
        keys, items, consent, times = flat(steps[c:c + per_call])
        harvest_model(b, keys, items, consent, int(times[0]), times=times, **kw)
    strip = lambda st: {k: v for k, v in st.items() if k != "log"}
    assert strip(a) == strip(b)
    sa_, ca = harvest_model(a, None, None, None, hc.FAR, sweep=True, **kw)
    sb_, cb = harvest_model(b, None, None, None, hc.FAR, sweep=True, **kw)
    assert sa_ == sb_ and len(sa_) > 100
    assert {k: v for k, v in ca.items() if k != "append_order"} == {k: v for k, v in cb.items() if k != "append_order"}
    assert cb["from_return"] + cb["from_rebuild"] == cb["stored"] + cb["lost"] + cb["skipped_short"]


def test_harvest_model_append_order_of_a_timed_call():
    A, B = (3 << 64) | 7, (1 << 64) | 9                                         # B < A
    key = lambda ks: (np.array([k >> 64 for k in ks], np.uint64), np.array([k & hc.U64 for k in ks], np.uint64))
    st = {}
    harvest_model(st, key([A, B]), [1, 2], None, 100, idle_secs=IDLE, ttl_secs=TTL)
    # A returns after idle (its stored session), then breaks twice inside the call; B breaks once: heads by key, then the sessions ended inside by key, request order
    reqs = [(A, 3, 130), (B, 4, 110), (A, 5, 160), (B, 6, 140), (A, 5, 190), (A, 6, 150)]
    _, ctr = harvest_model(st, key([k for k, _, _ in reqs]), [i for _, i, _ in reqs], None, 110, times=[t for _, _, t in reqs], limit=4, idle_secs=IDLE, ttl_secs=TTL)
    assert ctr["append_order"] == [(A, 100, [1]), (B, 110, [2, 4]), (A, 130, [3]), (A, 160, [5])]
    assert st[A] == ([5, 6], 150) and st[B] == ([6], 140)                        # a repeat across a break is kept; the last request's time, not the largest
    assert ctr["from_return"] == 4


@pytest.mark.parametrize("per_call", [40, 20, 7])
def test_feedback_model_with_times_equals_one_call_per_step(per_call):
    steps = hc.make_stream()
    rng = np.random.default_rng(5)
    how_many = 4
    rows = [(rng.integers(0, 40, (len(s["items"]), how_many)).astype(np.uint64) * np.uint64(7919) + np.uint64(10 ** 12),
             rng.integers(0, how_many + 1, len(s["items"])).astype(np.uint32)) for s in steps]
    a, b = {}, {}
    ranks_a, ctr_a = [], None
    total = lambda x, y: y if x is None else {k: x[k] + y[k] for k in x}
    for st, (ids, cnt) in zip(steps, rows):
        r, c = feedback_model(a, (st["hi"], st["lo"]), st["items"], st["consent"], ids, cnt, None, st["now"], idle_secs=IDLE, row_cap=how_many)
        ranks_a.append(r)
        ctr_a = total(ctr_a, c)
    ranks_b, ctr_b = [], None
    for c0 in range(0, len(steps), per_call):
        keys, items, consent, times = flat(steps[c0:c0 + per_call])
        ids = np.concatenate([r[0] for r in rows[c0:c0 + per_call]])
        cnt = np.concatenate([r[1] for r in rows[c0:c0 + per_call]])
        r, c = feedback_model(b, keys, items, consent, ids, cnt, None, 0, idle_secs=IDLE, row_cap=how_many, times=times)
        ranks_b.append(r)
        ctr_b = total(ctr_b, c)
    assert np.array_equal(np.concatenate(ranks_a), np.concatenate(ranks_b))
    for name in ctr_a:
        assert np.array_equal(ctr_a[name], ctr_b[name]), name
    assert ctr_a["idle_expired"] > 0 and ctr_a["hits_model"] > 0
    assert a.keys() == b.keys() and all(np.array_equal(a[k][0], b[k][0]) and a[k][1:] == b[k][1:] for k in a)


# ---- replay()'s cutting ----
def brute_plan(times, batch, every):
    """request by request: a new call where the batch is full or the S-second interval changes"""
    plan, start, boundary = [], 0, None
    for i in range(1, len(times) + 1):
        crossed = every is not None and i < len(times) and times[i] // every != times[i - 1] // every
        if i == len(times) or crossed or i - start == batch:
            plan.append((start, i, boundary))
            start, boundary = i, (int(times[i]) // every * every if crossed else None)
    return plan


def test_replay_plan():
    assert replay_plan([], 4) == [] and replay_plan([5], 4, 10) == [(0, 1, None)]
    t = [3, 3, 9, 10, 10, 11, 19, 20, 45, 45, 46]
    assert replay_plan(t, 100) == [(0, 11, None)]
    assert replay_plan(t, 4) == [(0, 4, None), (4, 8, None), (8, 11, None)]
    assert replay_plan(t, 100, 10) == [(0, 3, None), (3, 7, 10), (7, 8, 20), (8, 11, 40)]     # the gap 20 -> 45 crosses 30 and 40: one cut, at 40
    assert replay_plan(t, 3, 10) == [(0, 3, None), (3, 6, 10), (6, 7, None), (7, 8, 20), (8, 11, 40)]
    _, _, _, times = flat(hc.make_stream())
    for batch, every in ((700, 25), (333, None), (1, 7), (2000, 1), (5000, 1000)):
        plan = replay_plan(times, batch, every)
        assert plan == brute_plan(times.tolist(), batch, every)
        assert plan[0][0] == 0 and plan[-1][1] == len(times) and all(a[1] == b[0] for a, b in zip(plan, plan[1:])) and all(0 < b - a <= batch for a, b, _ in plan)
    with pytest.raises(ValueError):
        replay_plan([1, 2, 1], 10)
    with pytest.raises(ValueError):
        replay_plan([1, 2], 0)


def test_replay_cuts_calls_and_boundaries(monkeypatch):
    (hi, lo), items, consent, times = flat(hc.make_stream())
    log = []

    def stub(index, store, keys, item_ids, consent=None, **kw):
        n = len(item_ids)
        assert len(keys[0]) == len(keys[1]) == len(consent) == len(kw["times"]) == n and n > 0
        assert kw["now"] == int(kw["times"][0]) == int(kw["times"].min())           # the sweep clock: the call's first request, a lower bound
        log.append(("call", int(kw["times"][0]), n, kw["fill"], kw["exclude_seen"], kw["max_items_in_session"]))
        return np.tile(np.asarray(item_ids, np.uint64)[:, None], (1, kw["how_many"])), np.full(n, kw["how_many"], np.uint32)

    monkeypatch.setattr(serving, "recommend_batch", stub)
    out = replay("index", "store", (hi, lo), items, times, consent, k=5, m=5, how_many=3, max_items_in_session=4, batch=700, every=25,
                 on_boundary=lambda t: log.append(("boundary", t)), fill=True, collect=True)
    plan = brute_plan(times.tolist(), 700, 25)
    assert out["requests"] == 2000 and out["calls"] == len(plan) and out["boundaries"] == sum(b is not None for _, _, b in plan)
    assert out["calls"] == 4 and out["boundaries"] == 3                            # ~100 s of log from T0 = 0 mod 25: three multiples of 25 crossed, no stretch above 700 requests
    assert (out["calls"], out["boundaries"]) == REPLAY_700_25
    want = []
    for a, b, boundary in plan:
        if boundary is not None:
            assert boundary % 25 == 0 and times[a - 1] < boundary <= times[a]     # called before the requests at or after t
            want.append(("boundary", boundary))
        want.append(("call", int(times[a]), b - a, True, False, 4))
    assert log == want
    assert np.array_equal(out["ids"][:, 0], items) and out["ids"].shape == (2000, 3) and len(out["counts"]) == 2000 and "ranks" not in out and "feedback" not in out
    # a batch below the stretches' lengths: every stretch is served in several calls, and only its first one follows a boundary
    log.clear()
    out = replay("index", "store", (hi, lo), items, times, consent, k=5, m=5, how_many=3, batch=300, every=25, on_boundary=lambda t: log.append(("boundary", t)))
    assert (out["calls"], out["boundaries"]) == (8, 3) and [e for e in log if e[0] == "boundary"] == [("boundary", hc.T0 + 25 * i) for i in (1, 2, 3)]
    assert [e[2] for e in log if e[0] == "call"] == [300, 266, 300, 162, 300, 278, 300, 94] and set(out) == {"requests", "calls", "boundaries"}
    # unsorted times: refused before any call
    log.clear()
    bad = times.copy()
    bad[[10, 1500]] = bad[[1500, 10]]
    with pytest.raises(ValueError):
        replay("index", "store", (hi, lo), items, bad, consent, k=5, m=5, how_many=3, on_boundary=lambda t: log.append(t))
    assert log == []
