"""The PERSISTENT latency path (srn_index_serve_start: resident workgroups of vmis_fast_kernel<TINY> that poll a pinned control block) on the designed index of
tests/edge_cases.py, one srn_predict call per session.  What only this path runs: the doorbell line (number, length, check word, items 0..4 as 32-bit halves) and the
second line (items 5..12), the prep record a workgroup writes for itself, the state a workgroup keeps in LDS from one session to the next, the answer's status from the
sentinel in out_counts, and the hand-over counters it puts back to 0 by hand.

Parametrised over {distinct, tied timestamps} x {narrow ids, ids through edge_cases.wide_ids: both 32-bit halves non-zero and different}.  lanes = 2,
max_items_in_session = 10, idle_ms = 1 500 unless a test says otherwise; every test calls predict once before serve_start (the launch path's workspace exists) and stops
the resident workgroups in a `finally`.

Per call, everywhere: the row equals the oracle's (ids and order exactly, scores to SCORE_RTOL) AND, bit for bit, the row the fused one-launch form gave for the same
session before anything was resident (the same code: the same bytes); the change of (served, not_served) is what the CPU restatement says (edge_cases.resident_kind --
never read from the counters under test).

THE SERVED PREDICATE, corrected from the code.  The issue behind this file stated it as `route in (lean, mid) and E <= 63`.  The routing half holds (with the resident
forms' own limits: the lean form takes L <= 4, the other one 5..10, neither has a BIG tier: edge_cases.resident_route, which the census compares with the launch
sequence's route).  The row half does not: F_FIN_ENTRIES = 63 bounds the RECORD of a row handed to a finish kernel, but vmis_fast_kernel<TINY> finishes a longer entry
list in place as well when at most 64 of its keys lie at or above one step below the how_many-th largest (srn_fast.hip, `if (S <= 64u && S >= p.how_many)`), and a large
query's thresholds leave far fewer entries than it has scored items.  In the restatement's terms: served iff T <= 64, T = edge_cases.tight_set (which needs the scores'
top 32 bits: idf * acc, an extension of what restate_one's consumers computed so far).  With how_many = 21 every row of the designed index has T <= 24 -- the rows of
E = 64 and 65 items included: they ARE served; with how_many = 64 the edge is live, E = 63 / 64 -> T = 63 / 64 served, E = 65 -> T = 65 not served.

(a) every servable cell (<= 10 items, no q_shift: the selection of test_gpu_edge_cases.py (d)) plus three sessions without a known item, one caller, both shapes of
    E.SHAPES with a serve_stop / serve_start between them (the first request after the restart is served, and served right); `launches` stays at one per form.
(b) (a) in cell order, reversed, and in the designed interleave of edge_cases.serve_orders: per form heaviest, lightest, second heaviest, ... and every call the form
    does not finish with a served one directly behind it.  Rows and counters do not depend on the order.
(c) what the resident form must not touch: 5 items at max_items_in_session = 4 (one form resident), 11 items at 10, another k, m, how_many or business flag: neither
    counter moves, the row is the launch path's.
(d) (a) with how_many = 64 and with the business rules (fill_cases.draw_attrs' bytes) as the resident parameters, at the second shape.
(e) two threads behind a barrier, lanes = 2: the pass of (a) side by side, then per form its heaviest served sessions in a loop that is nothing but the C call (a Python
    thread that waits for the interpreter lock wakes up later than a resident call lasts: only such a loop makes the callers meet).  Every row right, served + not_served
    = the calls made, and per form at least two workgroups have served (srn_debug_serve_lane_counts).  A call that finds both taken takes the launch path: not_served,
    no error.
(f) ids through wide_ids on the BATCH path: one World.call per shape against the mapped oracle rows and bit for bit against SRN_NO_FAST=1, the path counts the
    restatement's -- which test_gpu_edge_cases.py asserts for the narrow world."""
import threading
import time

import numpy as np
import pytest

import edge_cases as E
from edge_world import SCORE_RTOL, World, _same_bytes, _vs_oracle, knobs  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu

LANES, MAX_ITEMS, IDLE_MS = 2, 10, 1500
WORLDS = [("distinct", False), ("distinct", True), ("tied", False), ("tied", True)]


_WORLDS = {}


def _world(variant, wide):
    """One World per (variant, ids) for the whole module (an index of this size is a few MB on the device)."""
    if (variant, wide) not in _WORLDS:
        w = World(variant == "tied", wide_ids=wide)
        w.label = "%s, %s ids" % (variant, "mapped" if wide else "narrow")
        w._serve = {}
        print("%s: %d queries, fixture built in %.1f s" % (w.label, w.nq, w.seconds))
        _WORLDS[(variant, wide)] = w
    return _WORLDS[(variant, wide)]


@pytest.fixture(scope="module", autouse=True)
def _close_worlds():
    yield
    for w in _WORLDS.values():
        w.gix.serve_stop()
        w.gix.close()
    _WORLDS.clear()


@pytest.fixture(scope="module", params=WORLDS, ids=["%s-%s" % (v, "mapped" if w else "narrow") for v, w in WORLDS])
def world(request):
    return _world(*request.param)


@pytest.fixture(scope="module", params=["distinct", "tied"])
def mapped_world(request):
    return _world(request.param, True)


def _predict(world, q, k, m, how_many, business):
    import serenade_amd as sa
    recs = sa.predict(world.gix, q, k, m, how_many, business)
    return np.array([r.id for r in recs], np.uint64), np.array([r.score for r in recs], np.float64)


def _plan(world, shape, how_many=21, business=False):
    """The calls of one pass with everything a check needs, made once per world while NOTHING is resident: the session as the GPU sees it, the oracle's row, the fused
    one-launch form's row for the same session, and what the restatement says the resident form does with it."""
    key = (shape, how_many, business)
    if key not in world._serve:
        world.gix.serve_stop()
        k, m = E.SHAPES[shape]
        ref = world.ref(k, m, how_many, business)
        attrs = E.business_attrs(world.ix) if business else None
        orders, kinds = E.serve_orders(world.tied, shape, how_many, attrs)
        calls = []
        for c, kind in zip(E.serve_calls(world.tied, shape), kinds):
            if c["qi"] is not None:
                n = int(ref["counts"][c["qi"]])
                want = (ref["ids"][c["qi"], :n], ref["scores"][c["qi"], :n])
            else:
                want = world.ref_one(c["q"], k, m, how_many, business)
            q = world.session(c["q"])
            calls.append(dict(name=c["name"], q=q, narrow=c["q"], want=want, fused=_predict(world, q, k, m, how_many, business), kind=kind, L=len(q),
                              general=0 if c["r"]["route"] in ("lean", "mid") else 1))
        world._serve[key] = (calls, orders)
    return world._serve[key]


def _check_row(got, c, what):
    ids, sc = got
    assert ids.tolist() == c["want"][0].tolist(), "%s: ids differ from the oracle\n got  %s\n want %s" % (what, ids.tolist(), c["want"][0].tolist())
    np.testing.assert_allclose(sc, c["want"][1], rtol=SCORE_RTOL, atol=0, err_msg=what)
    assert ids.tolist() == c["fused"][0].tolist() and sc.view(np.uint64).tolist() == c["fused"][1].view(np.uint64).tolist(), "%s: not the bytes of the fused one-launch form" % what


def _one_pass(world, shape, order, how_many=21, business=False):
    """serve_start at the shape's (k, m), every call of `order` by one caller -> {kind: calls}.  The resident workgroups are left running: the caller stops them."""
    gix = world.gix
    k, m = E.SHAPES[shape]
    calls, orders = _plan(world, shape, how_many, business)
    order = orders[order]
    _predict(world, calls[0]["q"], k, m, how_many, business)              # (the launch path's workspace exists before anything is resident)
    gix.serve_start(k, m, how_many, business, lanes=LANES, max_items_in_session=MAX_ITEMS, idle_ms=IDLE_MS)
    assert gix.serve_stats() == (0, 0, 2, 2 * LANES)
    assert calls[order[0]]["kind"] == "served", "the first request after a (re)start is one the resident form finishes itself"
    seen, bad = {}, []
    before = gix.serve_stats()
    t0 = time.time()
    for step, i in enumerate(order):
        c = calls[i]
        what = "%s, (k, m) = (%d, %d), how_many %d%s, step %d: %s (L = %d, %s)" % (world.label, k, m, how_many, ", business rules" if business else "", step, c["name"], c["L"], c["kind"])
        got = _predict(world, c["q"], k, m, how_many, business)
        after = gix.serve_stats()
        delta = (after[0] - before[0], after[1] - before[1])
        before = after
        # (a resident form that has gone -- marked dead after the host's 500 ms, or retired -- counts nothing: nothing more is posted to it)
        assert delta != (0, 0), "%s: neither counter moved: the resident form is gone (stats %s)" % (what, after)
        _check_row(got, c, what)
        if delta != ((1, 0) if c["kind"] == "served" else (0, 1)):
            bad.append("%s: (served, not_served) moved by %s" % (what, delta))
        if c["kind"] != "served" and gix.last_path_counts()[:2] != (1, c["general"]):
            bad.append("%s: the launch path's counts are %s" % (what, gix.last_path_counts()))
        seen[c["kind"]] = seen.get(c["kind"], 0) + 1
    secs = time.time() - t0
    stats = gix.serve_stats()
    print("%s, (k, m) = (%d, %d), how_many %d%s: %d calls in %.3f s, served %d, not served %d %s, launches %d, lanes served lean %s / 5..10 %s" % (
        world.label, k, m, how_many, ", business rules" if business else "", len(order), secs, stats[0], stats[1], {kd: n for kd, n in sorted(seen.items()) if kd != "served"}, stats[2],
        gix.serve_lane_counts(0), gix.serve_lane_counts(1)))
    assert not bad, "%d calls contradict the restatement:\n%s" % (len(bad), "\n".join(bad[:12]))
    assert stats[:2] == (seen.get("served", 0), len(order) - seen.get("served", 0))
    assert stats[2] == 2, "something made the resident workgroups leave during the pass: %d launches" % stats[2]
    assert sum(gix.serve_lane_counts(0)) + sum(gix.serve_lane_counts(1)) == stats[0]
    return seen


@pytest.mark.parametrize("order", ["cells", "reversed", "interleave"])
def test_ab_every_servable_cell_in_three_orders(world, knobs, order):
    knobs()
    try:
        for shape in (0, 1):   # (serve_start stops what is resident: the second shape is a restart with another (k, m))
            seen = _one_pass(world, shape, order)
            assert seen.get("served", 0) >= 120 and seen.get("general", 0) >= 1 and (shape == 0 or seen.get("big", 0) >= 1), seen
    finally:
        world.gix.serve_stop()
    assert world.gix.serve_stats()[3] == 0


def _untouched(world, q_narrow, k, m, how_many, business, what):
    """One call the resident state must not take: neither counter moves, the row is the oracle's."""
    before = world.gix.serve_stats()
    ids, sc = _predict(world, world.session(q_narrow), k, m, how_many, business)
    want = world.ref_one(q_narrow, k, m, how_many, business)
    assert world.gix.serve_stats() == before, "%s: the resident state counted a call that is not its own: %s -> %s" % (what, before, world.gix.serve_stats())
    assert ids.tolist() == want[0].tolist(), what
    np.testing.assert_allclose(sc, want[1], rtol=SCORE_RTOL, atol=0, err_msg=what)


def test_c_what_the_resident_form_must_not_touch(world, knobs):
    knobs()
    gix, ix = world.gix, world.ix
    k, m = E.SHAPES[0]
    calls, _orders = _plan(world, 0)
    one, four, five, six = (next(c["narrow"] for c in calls if c["L"] == L and c["kind"] == "served") for L in (1, 4, 5, 6))
    eleven = next(q for qi, q in enumerate(ix.queries) if len(q) == 11 and not ix.q_shift[qi])
    _predict(world, world.session(one), k, m, 21, False)
    try:
        gix.serve_start(k, m, 21, False, lanes=LANES, max_items_in_session=4, idle_ms=IDLE_MS)
        assert gix.serve_stats() == (0, 0, 1, LANES), "max_items_in_session = 4: the lean form alone is resident"
        _untouched(world, five, k, m, 21, False, "5 items at max_items_in_session = 4")
        ids, _sc = _predict(world, world.session(four), k, m, 21, False)
        assert gix.serve_stats()[:2] == (1, 0) and ids.tolist() == world.ref_one(four, k, m, 21)[0].tolist(), "4 items at max_items_in_session = 4 are the resident form's"
        gix.serve_start(k, m, 21, False, lanes=LANES, max_items_in_session=MAX_ITEMS, idle_ms=IDLE_MS)
        assert gix.serve_stats() == (0, 0, 2, 2 * LANES)
        _untouched(world, eleven, k, m, 21, False, "11 items at max_items_in_session = 10")
        for q, form in ((one, "lean"), (six, "5..10")):
            _untouched(world, q, k - 1, m, 21, False, "another k (%s)" % form)
            _untouched(world, q, k, m - 1, 21, False, "another m (%s)" % form)
            _untouched(world, q, k, m, 20, False, "another how_many (%s)" % form)
            _untouched(world, q, k, m, 21, True, "the business flag (%s)" % form)
        for q in (one, six):   # ... and the resident parameters are still served
            before = gix.serve_stats()
            ids, _sc = _predict(world, world.session(q), k, m, 21, False)
            assert gix.serve_stats()[:2] == (before[0] + 1, before[1]) and ids.tolist() == world.ref_one(q, k, m, 21)[0].tolist()
    finally:
        gix.serve_stop()


@pytest.mark.parametrize("how_many,business", [(64, False), (21, True)], ids=["how_many64", "business"])
def test_d_how_many_64_and_the_business_rules(world, knobs, how_many, business):
    knobs()
    try:
        seen = _one_pass(world, 1, "cells", how_many, business)
        assert seen.get("served", 0) >= 120, seen
        if how_many == 64:   # the edge of the row that wave 0 finishes in place: 64 entries at the cut are served, 65 are not (rows E = 64 / 65)
            assert seen.get("over64", 0) >= 1, seen
    finally:
        world.gix.serve_stop()


def _tight_loop(world, session, k, m, how_many, n_calls):
    """What a caller needs to post one session n_calls times with next to no Python between the calls: -> (run, rows).  run() makes the calls -- srn_predict through
    ctypes on arguments built beforehand, every call into a row of its own -- and returns the return codes; rows() gives [(ids, scores)] afterwards."""
    import ctypes as C
    from serenade_amd import capi
    fn, h = capi.lib().srn_predict, world.gix._h
    ev = capi.as_u64(session)
    ids, sc, n = np.zeros((n_calls, how_many), np.uint64), np.zeros((n_calls, how_many), np.float64), (C.c_size_t * n_calls)()
    args = [(h, capi.ptr(ev), len(ev), k, m, how_many, 0, capi.ptr(ids[j]), capi.ptr(sc[j]), C.cast(C.byref(n, j * C.sizeof(C.c_size_t)), C.POINTER(C.c_size_t))) for j in range(n_calls)]

    keep = (ev, ids, sc, n)   # (the arguments are addresses: what they point to lives as long as run does)

    def run():
        assert keep
        return [fn(*a) for a in args]

    def rows():
        return [(ids[j, :n[j]], sc[j, :n[j]]) for j in range(n_calls)]
    return run, rows


def test_e_two_callers_share_the_lanes(world, knobs):
    """Two threads start behind one barrier.  First the pass of (a) side by side, every row checked as it comes.  A resident call is over in some 15 us and a Python
    thread that waits for the interpreter lock wakes up later than that, so in that pass the two callers seldom meet inside the library; the second part makes them:
    per form, both callers post its three heaviest served sessions (the longest stays in a workgroup) 100 times each in a loop that is nothing but the C call, the rows
    compared afterwards -- repeated (at most five times) while the form's second workgroup has served nothing.  Nothing is timed."""
    knobs()
    gix = world.gix
    shape = 1
    k, m = E.SHAPES[shape]
    calls, orders = _plan(world, shape)
    order = orders["cells"]
    weight = [E.serve_weight(c) for c in E.serve_calls(world.tied, shape)]
    _predict(world, calls[0]["q"], k, m, 21, False)
    errs, made = [], [[0, 0], [0, 0]]   # per caller: calls made, of them calls of the kind `served`

    def pass_of_a(t):
        for step, i in enumerate(order):
            got = _predict(world, calls[i]["q"], k, m, 21, False)
            made[t][0] += 1
            made[t][1] += calls[i]["kind"] == "served"
            _check_row(got, calls[i], "caller %d, step %d: %s" % (t, step, calls[i]["name"]))

    def side_by_side(work):
        barrier = threading.Barrier(2, timeout=20)

        def caller(t):
            try:
                barrier.wait()
                work[t](t)
            except Exception as e:  # noqa: BLE001
                errs.append("caller %d: %r" % (t, e))
        th = [threading.Thread(target=caller, args=(t,)) for t in range(2)]
        t0 = time.time()
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        return time.time() - t0
    try:
        gix.serve_start(k, m, 21, False, lanes=LANES, max_items_in_session=MAX_ITEMS, idle_ms=IDLE_MS)
        secs = side_by_side([pass_of_a, pass_of_a])
        after_pass = [gix.serve_lane_counts(0), gix.serve_lane_counts(1)]
        rounds, n_each = [0, 0], 100
        for form in (0, 1):
            mine = sorted((i for i, c in enumerate(calls) if (c["L"] > 4) == bool(form) and c["kind"] == "served"), key=lambda i: (weight[i], i))[-3:]
            while rounds[form] == 0 or (rounds[form] < 5 and sum(1 for x in gix.serve_lane_counts(form) if x > 0) < 2):
                rounds[form] += 1
                loops = [[_tight_loop(world, calls[i]["q"], k, m, 21, n_each) for i in mine] for _t in range(2)]

                def hammer(t):
                    for run, _rows in loops[t]:
                        rcs = run()
                        made[t][0] += len(rcs)
                        made[t][1] += len(rcs)
                        assert not any(rcs), "srn_predict failed: %s" % sorted(set(rcs))
                side_by_side([hammer, hammer])
                for t in range(2):
                    for i, (_run, rows) in zip(mine, loops[t]):
                        got = rows()
                        assert all(np.array_equal(a, got[0][0]) and np.array_equal(b.view(np.uint64), got[0][1].view(np.uint64)) for a, b in got), "caller %d: %s: the rows of one session differ among its calls" % (t, calls[i]["name"])
                        _check_row(got[0], calls[i], "caller %d, side by side: %s" % (t, calls[i]["name"]))
        lanes = [gix.serve_lane_counts(0), gix.serve_lane_counts(1)]
        served, not_served, launches, _n = gix.serve_stats()
        print("%s: two callers, %d calls each in %.3f s (lanes served after it: lean %s / 5..10 %s), then %s rounds of 3 x %d calls per caller and form: served %d, not served %d, launches %d, "
              "lanes served lean %s / 5..10 %s" % (world.label, len(order), secs, after_pass[0], after_pass[1], rounds, n_each, served, not_served, launches, lanes[0], lanes[1]))
        assert served + not_served == made[0][0] + made[1][0] == 2 * (len(order) + 3 * n_each * sum(rounds))
        assert sum(lanes[0]) + sum(lanes[1]) == served
        assert served <= made[0][1] + made[1][1], "a call the restatement says the resident form cannot finish was counted as served"
        for form, name in zip(lanes, ("lean", "5..10")):
            assert len(form) == LANES and sum(1 for x in form if x > 0) >= 2, "the %s form: only %s of its workgroups served" % (name, form)
    finally:
        gix.serve_stop()


@pytest.mark.parametrize("shape", [0, 1], ids=["k500_m1100", "k1536_m2560"])
def test_f_mapped_ids_on_the_batch_path(mapped_world, knobs, shape):
    world = mapped_world
    k, m = E.SHAPES[shape]
    slow = world.slow(knobs, k, m)
    knobs()
    got = world.call(k, m)
    gix = world.gix
    nq, general, _glob = gix.last_path_counts()
    mid, big, merged = gix.last_mid_count(), gix.last_big_count(), gix.last_dedup_count()
    ref = world.ref(k, m)
    inside = np.arange(21)[None, :] < ref["counts"][:, None].astype(np.int64)
    hi, lo = ref["ids"][inside] >> np.uint64(32), ref["ids"][inside] & np.uint64(0xFFFFFFFF)
    assert (hi != 0).all() and (lo != 0).all() and (hi != lo).all(), "every expected id has two non-zero, different halves"
    _vs_oracle(got, ref, "mapped ids, batch path")
    _vs_oracle(slow, ref, "mapped ids, SRN_NO_FAST=1")
    _same_bytes(got, slow, "mapped ids against SRN_NO_FAST=1")
    routes = [r["route"] for r in E.restate(world.tied, shape)]
    want = (sum(r.startswith("mid") for r in routes), sum(r in ("big", "mid>big") for r in routes), sum(r in ("general", "mid>general", "long>general") for r in routes))
    print("%s (k %d, m %d): %d queries, MID %d, BIG %d, general %d" % (world.label, k, m, nq, mid, big, general))
    assert (nq, merged) == (world.nq, 0) and (mid, big, general) == want, "the mapped ids take other paths than the narrow ones: %s, want %s" % ((mid, big, general), want)
