"""Session harvest without a GPU: serving.harvest_model -- the rule of srn_harvest.hip in pure Python -- on hand-written cases, its independence of
how a time step's requests are cut into calls, and the new entry points in the built library."""
import ctypes as C

import numpy as np

from serenade_amd import capi
from serenade_amd.serving import harvest_model

import harvest_cases as hc

NEW_SYMBOLS = ["srn_harvest_create", "srn_harvest_free", "srn_device_sessions_set_harvest", "srn_harvest_stats", "srn_harvest_export", "srn_harvest_export_device",
               "srn_harvest_events_device", "srn_harvest_clear"]
IDLE, TTL = 20, 30
A, B = 7, 9                                 # two visitors (128-bit keys with a high word)
KEY_A, KEY_B = (3 << 64) | A, (1 << 64) | B


def test_new_symbols_are_bound_and_exported():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1] and fn.restype == capi.SYMBOLS[name][0], name
    assert C.sizeof(capi.HarvestStats) == 80
    import serenade_amd as sa
    assert sa.SessionHarvest is not None and sa.refreshed_index is not None and sa.harvest_model is harvest_model


def call(state, reqs, now, **kw):
    """reqs: (key, item, consent) triples"""
    hi = np.array([k >> 64 for k, _, _ in reqs], np.uint64)
    lo = np.array([k & hc.U64 for k, _, _ in reqs], np.uint64)
    kw = dict(dict(idle_secs=IDLE, ttl_secs=TTL), **kw)
    return harvest_model(state, (hi, lo), [i for _, i, _ in reqs], [c for _, _, c in reqs], now, **kw)


def test_the_idle_rule_is_strict():
    st = {}
    call(st, [(KEY_A, 1, 1), (KEY_B, 5, 1)], 100)
    call(st, [(KEY_A, 2, 1), (KEY_B, 6, 1)], 110)
    sess, ctr = call(st, [(KEY_A, 3, 1)], 110 + IDLE, limit=4)                 # exactly idle: the session goes on
    assert sess == [] and ctr["from_return"] == 0 and st[KEY_A] == ([1, 2, 3], 130)
    sess, ctr = call(st, [(KEY_B, 7, 1)], 110 + IDLE + 1, limit=4)             # idle + 1: B's session ended at its last click and B starts again
    assert sess == [(KEY_B, 110, [5, 6])] and ctr["from_return"] == 1 and ctr["stored"] == 1 and ctr["stored_items"] == 2
    assert st[KEY_B] == ([7], 131)
    # the TTL rule at a sweep is as strict, and a sweep without one leaves the store alone
    sess, ctr = harvest_model(st, None, None, None, 130 + TTL, ttl_secs=TTL, sweep=True)
    assert ctr["from_rebuild"] == 0 and KEY_A in st
    sess, ctr = harvest_model(st, None, None, None, 130 + TTL + 1, ttl_secs=TTL, sweep=True)
    assert ctr["from_rebuild"] == 1 and KEY_A not in st and KEY_B in st
    assert sess == [(KEY_B, 110, [5, 6]), (KEY_A, 130, [1, 2, 3])]             # canonical: by epoch, then key
    sess, ctr = harvest_model(st, None, None, None, 131 + TTL + 1, ttl_secs=TTL)
    assert ctr["from_rebuild"] == 1 and KEY_B in st


def test_repeated_click_window_and_min_len():
    st = {}
    call(st, [(KEY_A, 1, 1), (KEY_A, 1, 1), (KEY_A, 2, 1), (KEY_A, 2, 1), (KEY_A, 1, 1)], 100, limit=8)
    assert st[KEY_A] == ([1, 2, 1], 100)                                        # a repeat of the last item is not appended; an earlier item is
    call(st, [(KEY_A, i, 1) for i in (3, 4, 5, 6)], 105, limit=3)               # the limit (max_items_in_session, or H): one item dropped per append
    assert st[KEY_A] == ([4, 5, 6], 105)
    call(st, [(KEY_B, 9, 1), (KEY_B, 9, 1)], 105, limit=3)
    assert st[KEY_B] == ([9], 105)
    sess, ctr = harvest_model(st, None, None, None, 200, ttl_secs=TTL, min_len=2, sweep=True)
    assert sess == [(KEY_A, 105, [4, 5, 6])]                                    # the window as the slot held it; B's one item is below min_len
    assert ctr["skipped_short"] == 1 and ctr["from_rebuild"] == 2 and ctr["stored"] == 1 and ctr["lost"] == 0
    assert ctr["from_return"] + ctr["from_rebuild"] == ctr["stored"] + ctr["lost"] + ctr["skipped_short"]


def test_requests_without_consent_touch_nothing():
    st = {}
    call(st, [(KEY_A, 1, 1), (KEY_A, 2, 0), (KEY_B, 5, 0)], 100, limit=4)
    assert st[KEY_A] == ([1], 100) and KEY_B not in st
    sess, ctr = call(st, [(KEY_A, 3, 0)], 100 + IDLE + 5, limit=4)              # neither a return nor a click: not even the clock moves
    assert sess == [] and ctr["from_return"] == 0 and st[KEY_A] == ([1], 100)
    sess, ctr = call(st, [(KEY_A, 3, 0), (KEY_A, 4, 1)], 100 + IDLE + 6, limit=4)
    assert sess == [(KEY_A, 100, [1])] and st[KEY_A] == ([4], 126)


def test_a_full_log_loses_the_later_sessions_in_key_order():
    st = {}
    call(st, [(KEY_A, 1, 1), (KEY_B, 2, 1)], 100)
    sess, ctr = call(st, [(KEY_A, 3, 1), (KEY_B, 4, 1)], 100 + IDLE + 1, capacity=1)
    assert ctr["append_order"] == [(KEY_B, 100, [2])] and ctr["lost"] == 1 and ctr["stored"] == 1   # KEY_B < KEY_A: the call's returns are appended by key, not by request


def test_the_model_does_not_depend_on_the_cut():
    steps = hc.make_stream()
    for limit, min_len in ((2, 2), (6, 1)):
        one, c1, _ = hc.replay(steps, 1, limit=limit, min_len=min_len)
        three, c3, _ = hc.replay(steps, 3, limit=limit, min_len=min_len)
        assert one == three and len(one) > 100
        assert {k: v for k, v in c1.items() if k != "append_order"} == {k: v for k, v in c3.items() if k != "append_order"}
        assert sorted(c1["append_order"]) == sorted(c3["append_order"])
        assert c1["from_return"] + c1["from_rebuild"] == c1["stored"] + c1["lost"] + c1["skipped_short"]
        assert len({(e, k) for k, e, _ in one}) == len(one)                     # (epoch, key) is unique: two sessions of a visitor end more than idle apart


def test_the_stream_has_every_case_the_replay_test_is_about():
    steps = hc.make_stream()
    assert 1800 <= sum(len(s["items"]) for s in steps) <= 2200
    assert any(len(set(zip(s["hi"].tolist(), s["lo"].tolist()))) < len(s["items"]) for s in steps)
    assert sum(s["sweep"] for s in steps) >= 3 and 0 < sum(int(s["consent"].sum()) for s in steps) < sum(len(s["items"]) for s in steps)
    for limit in (2, 6):
        _, ctr, props = hc.replay(steps, 1, limit=limit, min_len=2)
        assert props["return_at_run_head"] >= 1 and props["by_explicit_sweep"] >= 1 and ctr["skipped_short"] >= 1 and ctr["from_return"] >= 10
        assert 100 < ctr["stored"] <= 256 and ctr["lost"] == 0                  # a log of 256 sessions holds them all
