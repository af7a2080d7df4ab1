"""Evaluation trials under the serving rules: what runs without a GPU -- evaluation.serving_queries against a step-by-step
simulation of the /v1/recommend handler's session rule, the plain trial against the evaluator's prefixes, the trial encoding and the
refusals that need no evaluation set."""
import ctypes as C

import numpy as np
import pytest

from serenade_amd import capi, evaluation
from helpers import evaluator_queries


def handler_simulation(sessions, W, H, exclude_seen):
    """One visitor per test session, clicks in order (recommend_resource.rs:39-54 at a constant limit): append the click unless it repeats the stored last item,
    drop the oldest beyond the limit -- the history window H, or the session window W on a store without one; predict on the last min(len, W) stored items.
    The last click of a session is sent too, but it has no next items and is no query."""
    limit = H if H else W
    out = []
    for ev in sessions.values():
        stored = []
        for t, click in enumerate(ev):
            if not stored or stored[-1] != click:
                stored.append(click)
                if len(stored) > limit:
                    stored.pop(0)
            if t + 1 < len(ev):
                out.append((stored[-min(len(stored), W):], list(stored) if exclude_seen else [], ev[t + 1:]))
    return out


def sessions_with_repeats(seed, W):
    rng = np.random.default_rng(seed)
    s = {}
    for i in range(60):   # random sessions over few items, with injected runs of repeats
        ev = [int(x) for x in rng.integers(1, 12, size=int(rng.integers(1, 30)))]
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(ev)))
            ev[at:at] = [ev[at]] * int(rng.integers(1, 7))
        s[i] = ev
    s[100] = [5]                                          # no query
    s[101] = [5, 5]
    s[102] = [5, 6]
    s[103] = [7] * 9                                      # all equal
    s[104] = [1, 2, 3][:max(1, W - 1)] + [4] * 5 + [5, 6]     # a run that starts inside the window and ends beyond it
    s[105] = list(range(1, W + 1)) + [9, 9, 9] + list(range(20, 20 + W + 1))   # a run that straddles the window's edge as the session moves on
    s[106] = [int(x) for x in rng.integers(1, 4, size=300)]     # longer than any history window, many natural repeats
    return s


@pytest.mark.parametrize("W", [1, 2, 5])
def test_closed_form_equals_the_handler_rule_step_by_step(W):
    sessions = sessions_with_repeats(17 + W, W)
    assert any(len(v) == 1 for v in sessions.values()) and any(len(v) == 2 for v in sessions.values())
    for H in (0, W, 8, 255):
        if H and H < W:
            continue
        for seen in (False, True):
            got = evaluation.serving_queries(sessions, W, history=H, handler_sessions=True, exclude_seen=seen)
            want = handler_simulation(sessions, W, H, seen)
            assert got == want, (W, H, seen)
        # the session's own items: the query's, whatever the history window
        got = evaluation.serving_queries(sessions, W, history=H, handler_sessions=True, exclude_session=True)
        assert got == [(q, q, n) for q, _, n in handler_simulation(sessions, W, H, False)]
        # both flags: the seen window, a superset of the query's items
        both = evaluation.serving_queries(sessions, W, history=H, handler_sessions=True, exclude_session=True, exclude_seen=True)
        assert both == handler_simulation(sessions, W, H, True)
        assert all(set(q) <= set(x) for q, x, _ in both)
    # the handler rule acts on these sessions: some seen window differs from the raw one (and, from a window of 2 on, some query: at 1 both are the last click)
    raw = evaluation.serving_queries(sessions, W, history=8, exclude_seen=True)
    assert [x for _, x, _ in raw] != [x for _, x, _ in handler_simulation(sessions, W, 8, True)]
    assert W == 1 or [q for q, _, _ in raw] != [q for q, _, _ in handler_simulation(sessions, W, 8, True)]


@pytest.mark.parametrize("W", [1, 2, 5])
def test_raw_sessions_keep_repeats_and_window_the_seen_items(W):
    sessions = sessions_with_repeats(3, W)
    for H in (0, W, 8, 255):
        if H and H < W:
            continue
        got = evaluation.serving_queries(sessions, W, history=H, exclude_seen=True)
        want = [(ev[max(0, t - W):t], ev[max(0, t - (H or W)):t], ev[t:]) for ev in sessions.values() for t in range(1, len(ev))]
        assert got == want


@pytest.mark.parametrize("W", [1, 2, 5, 100])
def test_without_flags_the_queries_are_the_evaluators(W):
    sessions = sessions_with_repeats(5, min(W, 5))
    want = evaluator_queries(sessions, W)
    for H in (0, W, 255):   # history alone changes nothing
        got = evaluation.serving_queries(sessions, W, history=H)
        assert [(q, n) for q, _, n in got] == want
        assert all(x == [] for _, x, _ in got)
    assert evaluation.serving_queries(list(sessions.values()), W) == evaluation.serving_queries(sessions, W)
    with pytest.raises(ValueError):
        evaluation.serving_queries(sessions, 5, history=4)


def test_trial_encoding_of_the_serving_keys():
    base = dict(k=50, m=500, max_items_in_session=2)
    t = evaluation._trial(base)
    assert (t.flags, t.history) == (0, 0)
    assert C.sizeof(capi.EvalTrial) == 32 and capi.EvalTrial.history.offset == 28 and capi.EvalTrial.flags.offset == 20
    assert capi.FLAG_EVAL_HANDLER == 32
    for key, flag in (("exclude_session", capi.FLAG_EXCLUDE_SESSION), ("exclude_seen", capi.FLAG_EXCLUDE_SEEN), ("handler_sessions", capi.FLAG_EVAL_HANDLER),
                      ("fill", capi.FLAG_FILL), ("business_logic", capi.FLAG_BUSINESS_LOGIC)):
        assert evaluation._trial(dict(base, **{key: True})).flags == flag
        assert evaluation._trial(dict(base, **{key: False})).flags == 0
    t = evaluation._trial(dict(base, exclude_seen=True, handler_sessions=True, fill=True, history=8, max_chunk_queries=256))
    assert t.flags == capi.FLAG_EXCLUDE_SEEN | capi.FLAG_EVAL_HANDLER | capi.FLAG_FILL
    assert (t.history, t.max_chunk_queries, t.k, t.m, t.how_many, t.max_items_in_session, t.length) == (8, 256, 50, 500, 20, 2, 20)
    assert evaluation._trial(dict(base, history=8)).flags == 0   # history alone sets no flag


def test_history_and_wide_rows_are_checked_before_the_set_is_looked_at():
    L, r = capi.lib(), capi.EvalResult()

    def code(**kw):
        t = evaluation._trial(dict(dict(k=50, m=500, max_items_in_session=4), **kw))
        return L.srn_evaluate(None, C.byref(t), 1, C.byref(r), None)
    good = capi.SRN_EINVAL   # a good trial gets as far as the missing set
    assert code() == good
    for h in (1, 2, 3, capi.MAX_SESSION_LEN + 1):
        assert code(history=h) == capi.SRN_ERANGE
        assert code(history=h, exclude_seen=True) == capi.SRN_ERANGE
    for h in (0, 4, 8, capi.MAX_SESSION_LEN):
        assert code(history=h) == good and code(history=h, exclude_seen=True, handler_sessions=True) == good
    # the internal how_many: how_many + history with exclude_seen (the window without a history), + the window with exclude_session alone
    assert code(how_many=capi.MAX_HOW_MANY - 8, history=8, exclude_seen=True) == good
    assert code(how_many=capi.MAX_HOW_MANY - 7, history=8, exclude_seen=True) == capi.SRN_ERANGE
    assert code(how_many=capi.MAX_HOW_MANY - 7, history=8) == good                      # history without the flag widens nothing
    assert code(how_many=capi.MAX_HOW_MANY - 7, history=8, exclude_session=True) == good    # ... the session window does: 4
    assert code(how_many=capi.MAX_HOW_MANY - 3, exclude_session=True) == capi.SRN_ERANGE
    assert code(how_many=capi.MAX_HOW_MANY - 3, exclude_seen=True) == capi.SRN_ERANGE
    assert code(how_many=capi.MAX_HOW_MANY, handler_sessions=True) == good
    # every trial of a call is checked, not only the first
    ts = (capi.EvalTrial * 2)(evaluation._trial(dict(k=50, m=500, max_items_in_session=4)), evaluation._trial(dict(k=50, m=500, max_items_in_session=4, history=2)))
    rs = (capi.EvalResult * 2)()
    assert L.srn_evaluate(None, ts, 2, rs, None) == capi.SRN_ERANGE


def test_search_refuses_a_history_below_a_trials_window_before_it_reads_anything():
    from serenade_amd import hpo
    trials = [dict(m=100, k=50, max_items_in_session=2, idf_weighting=1), dict(m=100, k=50, max_items_in_session=10, idf_weighting=1)]
    with pytest.raises(ValueError, match="trial 1"):
        hpo.search("no-such-train.txt", "no-such-test.txt", trials, exclude_seen=True, history=8)
