"""The timed batch on the GPU (srn_recommend_batch*_at, srn_feedback_observe*_at, serving.replay): a call whose requests carry their own clocks leaves
rows, store, harvest and feedback log as the same requests served one after the other do.  The reference arm is the code as it stood before: untimed calls.
The stream is harvest_cases.make_stream()'s, its 40 item ids mapped one to one onto ids the small index knows, so that the rows are not empty."""
import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi
from serenade_amd.serving import ClickFeedback, DeviceSessionStore, SessionHarvest, feedback_model, harvest_model, recommend_batch, replay

import harvest_cases as hc
from helpers import small_dataset
from test_replay_host import REPLAY_700_25, flat

pytestmark = pytest.mark.gpu

K, M, HOW_MANY = 50, 200, 21
IDLE, TTL, T0, FAR = hc.IDLE, hc.TTL, hc.T0, hc.FAR
COUNTERS = ("stored", "stored_items", "lost", "skipped_short", "from_return", "from_rebuild")
CONFIGS = {"limit2": dict(history=0, limit=2, flags={}), "h6_exclude_fill": dict(history=6, limit=6, flags=dict(exclude_seen=True, fill=True))}


@pytest.fixture(scope="module")
def index():
    off, items, ts, ids = small_dataset(33, n_sessions=1500, n_items=200)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 200, 12, 1.0)
    gix.set_fallback_popular(64)
    gix.known_ids = ids
    yield gix
    gix.close()


def export_bytes(e):
    """a store's or harvest's export as bytes, the entries in ascending (epoch, key_hi, key_lo) order: a harvest's export already is; a store's is in slot order, and
    where two colliding keys land is decided by the claim races of sess_find, so two stores driven alike hold the same entries, not always in the same slots"""
    order = np.lexsort((e[0][1], e[0][0], e[1]))
    return b"".join(np.ascontiguousarray(x[order]).tobytes() for x in (e[0][0], e[0][1]) + tuple(e[1:]))


def stream(index):
    """-> (hi, lo), items, consent, times, step edges: the 2000 requests, a step's `now` as the time of each of its requests"""
    steps = hc.make_stream()
    keys, items, consent, times = flat(steps)
    pool = np.arange(40, dtype=np.uint64) * np.uint64(7919) + np.uint64(10 ** 12)
    assert np.isin(items, pool).all()
    items = index.known_ids[:40][np.searchsorted(pool, items)]                    # one to one: what repeats what is unchanged
    edges = np.concatenate([[0], np.cumsum([len(s["items"]) for s in steps])])
    return keys, items, consent, times, edges


def serve(index, cfg, calls, reqs, harvest=dict(capacity=512, min_len=2), sweep_far=True):
    """calls: [(start, stop, now or None)] -- now: an untimed call at that time; None: a timed call with the requests' own times (sweep clock: their minimum).
    -> everything the arms are compared by"""
    (hi, lo), items, consent, times = reqs
    store = DeviceSessionStore(index, capacity=8192, items_cap=8, ttl_secs=TTL, idle_secs=IDLE, history=cfg["history"])
    hv = SessionHarvest(index, items_cap=8, **harvest)
    store.set_harvest(hv)
    fb = ClickFeedback(index, capacity=8192, row_cap=HOW_MANY, ttl_secs=TTL, idle_secs=IDLE)
    rows, ranks = [], []
    for a, b, now in calls:
        sl = slice(a, b)
        kw = dict(now=now) if now is not None else dict(times=times[sl])
        rows.append(recommend_batch(index, store, (hi[sl], lo[sl]), items[sl], None if consent is None else consent[sl], k=K, m=M, how_many=HOW_MANY,
                                    max_items_in_session=2, scores=True, feedback=fb, **cfg["flags"], **kw))
        ranks.append(fb.last_ranks)
    out = dict(ids=np.concatenate([r[0] for r in rows]), counts=np.concatenate([r[1] for r in rows]), scores=np.concatenate([r[2] for r in rows]),
               ranks=np.concatenate(ranks), store=store.export(now=1), store_stats=store.stats, fb_stats=fb.stats(), fb_hist=fb.histogram(), hv_before=hv.stats())
    if sweep_far:
        store.sweep(FAR)
    out["hv"], out["hv_stats"] = hv.export(), hv.stats()
    for o in (store, hv, fb):
        o.close()
    return out


def assert_same(got, ref, what):
    for name in ("ids", "counts", "scores", "ranks"):
        assert got[name].tobytes() == ref[name].tobytes(), (what, name, np.flatnonzero((got[name] != ref[name]).reshape(len(ref[name]), -1).any(axis=1))[:8])
    assert export_bytes(got["store"]) == export_bytes(ref["store"]), (what, "store")
    assert len(got["store"][1]) == len(ref["store"][1])
    assert export_bytes(got["hv"]) == export_bytes(ref["hv"]), (what, "harvest", len(got["hv"][1]), len(ref["hv"][1]))
    for name in ("stored", "stored_items", "skipped_short", "lost"):
        assert got["hv_stats"][name] == ref["hv_stats"][name], (what, name)
    assert got["hv_stats"]["from_return"] + got["hv_stats"]["from_rebuild"] == ref["hv_stats"]["from_return"] + ref["hv_stats"]["from_rebuild"], what
    assert got["fb_stats"] == ref["fb_stats"], (what, got["fb_stats"], ref["fb_stats"])
    assert all(np.array_equal(x, y) for x, y in zip(got["fb_hist"], ref["fb_hist"])), what
    assert got["store_stats"]["sweeps"] == ref["store_stats"]["sweeps"] == 0 and got["fb_stats"]["sweeps"] == 0     # no automatic sweep ran


_STEPPED = {}


def stepped(index, name):
    """arm (a), once per configuration: one untimed call per step"""
    if name not in _STEPPED:
        keys, items, consent, times, edges = stream(index)
        calls = [(int(a), int(b), int(times[a])) for a, b in zip(edges, edges[1:])]
        _STEPPED[name] = serve(index, CONFIGS[name], calls, (keys, items, consent, times))
    return _STEPPED[name]


@pytest.mark.parametrize("arm", ["two_calls_of_20_steps", "one_call", "every_333_requests"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_timed_equals_stepped(index, name, arm):
    cfg = CONFIGS[name]
    keys, items, consent, times, edges = stream(index)
    n = len(items)
    calls = {"two_calls_of_20_steps": [(0, int(edges[20]), None), (int(edges[20]), n, None)], "one_call": [(0, n, None)],
             "every_333_requests": [(a, min(a + 333, n), None) for a in range(0, n, 333)]}[arm]
    ref = stepped(index, name)
    got = serve(index, cfg, calls, (keys, items, consent, times))
    assert_same(got, ref, (name, arm))
    assert int(ref["counts"].max()) > 0 and ref["fb_stats"]["hits_model"] + ref["fb_stats"]["hits_filled"] > 0 and ref["fb_stats"]["idle_expired"] > 0
    # ... and the Python models with times=, cut as the arm is
    state, fstate, model, ranks, ctr = {}, {}, None, [], None
    for a, b, _ in calls:
        sl = slice(a, b)
        model = harvest_model(state, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], int(times[a]), times=times[sl], limit=cfg["limit"], idle_secs=IDLE, ttl_secs=TTL,
                              min_len=2)
        r, c = feedback_model(fstate, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], got["ids"][sl], got["counts"][sl], got["scores"][sl], 0, idle_secs=IDLE,
                              row_cap=HOW_MANY, times=times[sl])
        ranks.append(r)
        ctr = c if ctr is None else {k_: ctr[k_] + c[k_] for k_ in c}
    for name_ in ("from_return", "skipped_short", "stored", "lost"):
        assert got["hv_before"][name_] == model[1][name_], (arm, name_)
    sessions, mctr = harvest_model(state, None, None, None, FAR, sweep=True, ttl_secs=TTL, min_len=2)
    assert export_bytes(got["hv"]) == export_bytes(hc.as_arrays(sessions, 8)) and len(sessions) > 100
    for name_ in COUNTERS:
        assert got["hv_stats"][name_] == mctr[name_], (arm, name_)
    assert np.array_equal(np.concatenate(ranks), got["ranks"])
    for name_ in ("requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored"):
        assert got["fb_stats"][name_] == ctr[name_], (arm, name_)
    assert np.array_equal(got["fb_hist"][0], ctr["hist_model"]) and np.array_equal(got["fb_hist"][1], ctr["hist_filled"])
    if arm == "one_call":
        assert got["hv_before"]["from_return"] == 109                             # the breaks inside runs (tests/test_replay_host.py), all offered by this one call


def one_by_one(index, cfg, reqs):
    times = reqs[3]
    return serve(index, cfg, [(i, i + 1, int(times[i])) for i in range(len(times))], reqs)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_visitor_with_breaks_at_block_edges(index, name):
    """600 consenting requests of one visitor: segments that start on, before and after a 256-lane block edge"""
    n = 600
    gaps = np.ones(n, np.uint64)
    gaps[[255, 256, 257, 511, 512]] = IDLE + 1
    times = np.uint64(T0) + np.cumsum(gaps)
    rng = np.random.default_rng(3)
    items = index.known_ids[rng.integers(0, 12, n)]
    items[[256, 511]] = items[[255, 510]]                                        # a click that repeats the previous one across a break
    reqs = ((np.full(n, 7, np.uint64), np.full(n, 9, np.uint64)), items, None, times)
    cfg = CONFIGS[name]
    ref = one_by_one(index, cfg, reqs)
    got = serve(index, cfg, [(0, n, None)], reqs)
    assert_same(got, ref, name)
    s = got["hv_before"]
    assert s["from_return"] == 5 and s["stored"] + s["skipped_short"] == 5
    assert s["skipped_short"] == 3                                               # the sessions that start at positions 255, 256 and 511 hold one click: below min_len 2
    assert got["fb_stats"]["idle_expired"] == 5 and got["fb_stats"]["first_seen"] == 1
    assert got["store"][1].tolist() == [int(times[-1])] and got["store"][2].tolist() == [cfg["limit"]]


def edge_requests(index):
    """three visitors: non-consenting requests between a visitor's consenting ones, times that decrease within a visitor, a repeat across a break, a visitor known to
    the store from an earlier call"""
    ids = index.known_ids
    A, B, D = (3, 7), (1, 9), (3, 9)
    rows = [  # key, item, consent, time
        (A, ids[0], 1, T0 + 100), (B, ids[1], 1, T0 + 100), (A, ids[2], 0, T0 + 101), (A, ids[0], 1, T0 + 100 + IDLE + 1),   # a break whose predecessor in request order does not consent; a repeat kept
        (B, ids[3], 1, T0 + 90), (B, ids[4], 1, T0 + 95), (B, ids[4], 1, T0 + 95 + IDLE), (B, ids[5], 0, T0 + 500), (B, ids[5], 1, T0 + 70),   # decreasing; exactly idle: no break
        (D, ids[6], 1, T0 + 50), (D, ids[7], 1, T0 + 50 + IDLE), (D, ids[7], 1, T0 + 51 + 2 * IDLE), (A, ids[8], 1, T0 + 60), (D, ids[9], 0, T0 + 1), (D, ids[9], 1, T0 + 52 + 3 * IDLE),
        (A, ids[8], 1, T0 + 61), (A, ids[9], 1, T0 + 300), (A, ids[9], 1, T0 + 300 + TTL + 1)]                            # breaks beyond the TTL
    key = np.array([r[0] for r in rows], np.uint64)
    return (key[:, 0].copy(), key[:, 1].copy()), np.array([r[1] for r in rows], np.uint64), np.array([r[2] for r in rows], np.uint8), np.array([r[3] for r in rows], np.uint64)


def test_interleaved_consent_decreasing_times_and_repeats(index):
    reqs = edge_requests(index)
    n = len(reqs[1])
    for name, cfg in CONFIGS.items():
        ref = one_by_one(index, cfg, reqs)
        for calls in ([(0, n, None)], [(0, 5, None), (5, n, None)], [(i, i + 1, None) for i in range(n)]):       # the last: n = 1, every call
            got = serve(index, cfg, calls, reqs)
            assert_same(got, ref, (name, calls))
        assert ref["hv_stats"]["from_return"] >= 4


def test_a_call_without_consent_and_all_times_equal(index):
    keys, items, consent, times, edges = stream(index)
    cfg = CONFIGS["limit2"]
    T = int(times[edges[20]])
    # the first 20 steps build up a store; then one call of 300 requests whose times are all T against the untimed call at T: rows and store export, bit for bit
    first = [(int(a), int(b), int(times[a])) for a, b in zip(edges[:20], edges[1:21])]
    a, b = int(edges[20]), int(edges[20]) + 300
    same_t = times.copy()
    same_t[a:b] = T
    ref = serve(index, cfg, first + [(a, b, T)], (keys, items, consent, same_t))
    got = serve(index, cfg, first + [(a, b, None)], (keys, items, consent, same_t))
    assert_same(got, ref, "all times equal")
    # no consenting request: nothing is stored, nothing is offered, the rows are the untimed call's
    none = np.zeros(len(items), np.uint8)
    ref = serve(index, cfg, [(0, 300, T)], (keys, items, none, times))
    got = serve(index, cfg, [(0, 300, None)], (keys, items, none, times))
    assert_same(got, ref, "no consent")
    assert len(got["store"][1]) == 0 and got["hv_stats"]["from_return"] == 0 and got["fb_stats"]["no_consent"] == 300 and int(got["counts"].max()) > 0


def test_a_full_log_keeps_the_first_sessions_of_the_append_order(index):
    keys, items, consent, times, _ = stream(index)
    cfg = CONFIGS["limit2"]
    got = serve(index, cfg, [(0, len(items), None)], (keys, items, consent, times), harvest=dict(capacity=8, min_len=1), sweep_far=False)
    state = {}
    sessions, ctr = harvest_model(state, keys, items, consent, int(times[0]), times=times, limit=2, idle_secs=IDLE, ttl_secs=TTL, min_len=1, capacity=8)
    assert ctr["stored"] == 8 and ctr["lost"] > 50 and len(ctr["append_order"]) == 8
    keys_in_order = [k_ for k_, _, _ in ctr["append_order"]]
    assert keys_in_order == sorted(keys_in_order)                                # (one call on an empty store: no head returns, the sessions ended inside by key)
    assert export_bytes(got["hv"]) == export_bytes(hc.as_arrays(sessions, 8))
    s = got["hv_stats"]
    for name in COUNTERS:
        assert s[name] == ctr[name], name
    assert s["from_return"] + s["from_rebuild"] == s["stored"] + s["cleared"] + s["lost"] + s["skipped_short"]


def test_arguments(index):
    L = capi.lib()
    keys, items, consent, times, _ = stream(index)
    cfg = CONFIGS["limit2"]
    store = DeviceSessionStore(index, capacity=1024, items_cap=8, ttl_secs=TTL, idle_secs=IDLE)
    hv = SessionHarvest(index, capacity=64, items_cap=8, min_len=1)
    store.set_harvest(hv)
    fb = ClickFeedback(index, capacity=1024, row_cap=8, ttl_secs=TTL, idle_secs=IDLE)
    n = 100
    sl = slice(0, n)
    ids, cnt, sc = recommend_batch(index, store, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], k=K, m=M, how_many=8, scores=True, feedback=fb, times=times[sl])
    before = (export_bytes(store.export(now=1)), hv.stats(), fb.stats(), fb.histogram()[0].tobytes())
    hi, lo, it, tm = (capi.as_u64(a[sl]) for a in (keys[0], keys[1], items, times))
    con = np.ascontiguousarray(consent[sl])
    out = np.zeros((n, 8), np.uint64), np.zeros((n, 8), np.float64), np.zeros(n, np.uint32)
    p = capi.ptr
    rec = lambda times_p, n_, how_many=8, st=store: L.srn_recommend_batch_at(index._h, st._h, p(hi), p(lo), p(it), p(con), times_p, n_, T0, 2, K, M, how_many, 0,   # noqa: E731
                                                                              p(out[0]), p(out[1]), p(out[2]))
    assert rec(None, n) == capi.SRN_EINVAL
    assert rec(p(tm), 2 ** 24 + 1) == capi.SRN_ERANGE
    assert rec(p(tm), 0) == capi.SRN_OK
    assert L.srn_recommend_batch_device_at(index._h, store._h, p(hi), p(lo), p(it), p(con), None, n, T0, 2, K, M, 8, 0, p(out[0]), p(out[1]), p(out[2]), None) == capi.SRN_EINVAL
    obs = lambda times_p, n_, how_many=8: L.srn_feedback_observe_at(fb._h, p(hi), p(lo), p(it), p(con), times_p, n_, T0, p(capi.as_u64(ids)), None, p(capi.as_u32(cnt)),   # noqa: E731
                                                                    how_many, None)
    assert obs(None, n) == capi.SRN_EINVAL
    assert obs(p(tm), 2 ** 24 + 1) == capi.SRN_ERANGE
    assert obs(p(tm), n, how_many=9) == capi.SRN_ERANGE                            # above the log's row_cap
    assert L.srn_feedback_observe_device_at(fb._h, p(hi), p(lo), p(it), p(con), None, n, T0, p(capi.as_u64(ids)), None, p(capi.as_u32(cnt)), 8, None, None) == capi.SRN_EINVAL
    with pytest.raises(ValueError):
        recommend_batch(index, store, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], k=K, m=M, how_many=9, feedback=fb, times=times[sl])
    with pytest.raises(ValueError):
        recommend_batch(index, store, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], k=K, m=M, how_many=8, times=times[:n - 1])
    if capi.device_count() > 1:
        dev = index.info["device"]
        far = DeviceSessionStore(1 - dev if dev < 2 else 0, capacity=32, items_cap=8)
        assert rec(p(tm), n, st=far) == capi.SRN_EINVAL
        assert len(far.export(now=1)[1]) == 0
        far.close()
    assert (export_bytes(store.export(now=1)), hv.stats(), fb.stats(), fb.histogram()[0].tobytes()) == before
    for o in (store, hv, fb):
        o.close()


def test_replay_with_boundaries(index):
    """replay(batch=700, every=25) with a sweep and a trending refresh at every boundary against the same timed calls and boundary actions written out by hand"""
    keys, items, consent, times, _ = stream(index)
    cuts = [0] + [int(np.searchsorted(times, T0 + 25 * i)) for i in (1, 2, 3)] + [len(items)]       # T0 is a multiple of 25; the log is ~100 s long
    assert all(0 < b - a <= 700 for a, b in zip(cuts, cuts[1:]))

    def run(by_hand):
        store = DeviceSessionStore(index, capacity=8192, items_cap=8, ttl_secs=TTL, idle_secs=IDLE)
        hv = SessionHarvest(index, capacity=512, items_cap=8, min_len=2)
        store.set_harvest(hv)
        fb = ClickFeedback(index, capacity=8192, row_cap=HOW_MANY, ttl_secs=TTL, idle_secs=IDLE)
        seen = []

        def boundary(t):
            seen.append(t)
            store.sweep(t)
            index.set_fallback_trending(store, 16, now=t)
        kw = dict(k=K, m=M, how_many=HOW_MANY, max_items_in_session=2, fill=True, feedback=fb)
        if by_hand:
            rows, ranks = [], []
            for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
                if i:
                    boundary(T0 + 25 * i)
                sl = slice(a, b)
                rows.append(recommend_batch(index, store, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], times=times[sl], now=int(times[a]), **kw))
                ranks.append(fb.last_ranks)
            out = dict(ids=np.concatenate([r[0] for r in rows]), counts=np.concatenate([r[1] for r in rows]), ranks=np.concatenate(ranks), calls=len(rows),
                       boundaries=len(seen), feedback=fb.stats())
        else:
            out = replay(index, store, keys, items, times, consent, batch=700, every=25, on_boundary=boundary, collect=True, **kw)
        out["store"], out["sweeps"] = export_bytes(store.export(now=1)), store.stats["sweeps"]
        store.sweep(FAR)
        out["hv"], out["hv_stats"], out["seen"] = export_bytes(hv.export()), hv.stats(), seen
        for o in (store, hv, fb):
            o.close()
        return out

    try:
        hand, got = run(True), run(False)
    finally:
        index.set_fallback_popular(64)
    assert (got["calls"], got["boundaries"]) == REPLAY_700_25 == (hand["calls"], hand["boundaries"]) and got["requests"] == len(items)
    assert got["seen"] == hand["seen"] == [T0 + 25 * i for i in (1, 2, 3)] and got["sweeps"] == hand["sweeps"] == 3
    for name in ("ids", "counts", "ranks"):
        assert got[name].tobytes() == hand[name].tobytes(), name
    assert got["store"] == hand["store"] and got["hv"] == hand["hv"] and got["hv_stats"] == hand["hv_stats"] and got["feedback"] == hand["feedback"]
    assert got["hv_stats"]["from_rebuild"] > 0 and got["hv_stats"]["from_return"] > 0 and bool((got["counts"] > 0).all())
    bad = times.copy()
    bad[[10, 1500]] = bad[[1500, 10]]
    with pytest.raises(ValueError):
        replay(index, None, keys, items, bad, consent, k=K, m=M, how_many=HOW_MANY, on_boundary=lambda t: pytest.fail("a boundary before the check"))


def test_tensors_on_the_gpu_give_the_host_arrays_result(index):
    """the device-pointer entry points (srn_recommend_batch_device_at, srn_feedback_observe_device_at) through tensors, with the default sweep clock: times.min()"""
    import torch
    keys, items, consent, times, _ = stream(index)
    cfg = CONFIGS["h6_exclude_fill"]
    ref = serve(index, cfg, [(0, 1000, None), (1000, len(items), None)], (keys, items, consent, times))
    dev = torch.device("cuda", index.info["device"])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)   # noqa: E731
    store = DeviceSessionStore(index, capacity=8192, items_cap=8, ttl_secs=TTL, idle_secs=IDLE, history=6)
    hv = SessionHarvest(index, capacity=512, items_cap=8, min_len=2)
    store.set_harvest(hv)
    fb = ClickFeedback(index, capacity=8192, row_cap=HOW_MANY, ttl_secs=TTL, idle_secs=IDLE)
    rows, ranks = [], []
    for sl in (slice(0, 1000), slice(1000, len(items))):
        rows.append(recommend_batch(index, store, (t(keys[0][sl]), t(keys[1][sl])), t(items[sl]), t(consent[sl]), k=K, m=M, how_many=HOW_MANY, max_items_in_session=2,
                                    scores=True, feedback=fb, times=t(times[sl]), **cfg["flags"]))
        ranks.append(fb.last_ranks)
    torch.cuda.current_stream(index.info["device"]).synchronize()
    assert torch.cat([r[0] for r in rows]).cpu().numpy().view(np.uint64).tobytes() == ref["ids"].tobytes()
    assert torch.cat([r[1] for r in rows]).cpu().numpy().view(np.uint32).tobytes() == ref["counts"].tobytes()
    assert torch.cat([r[2] for r in rows]).cpu().numpy().tobytes() == ref["scores"].tobytes()
    assert torch.cat(ranks).cpu().numpy().view(np.uint32).tobytes() == ref["ranks"].tobytes()
    assert export_bytes(store.export(now=1)) == export_bytes(ref["store"]) and fb.stats() == ref["fb_stats"]
    store.sweep(FAR)
    assert export_bytes(hv.export()) == export_bytes(ref["hv"]) and hv.stats() == ref["hv_stats"]
    with pytest.raises(ValueError):
        recommend_batch(index, store, (t(keys[0][:4]), t(keys[1][:4])), t(items[:4]), None, k=K, m=M, how_many=HOW_MANY, times=times[:4])     # times on the host beside tensors
    for o in (store, hv, fb):
        o.close()
    # ... and replay() on tensors: the same two calls
    store = DeviceSessionStore(index, capacity=8192, items_cap=8, ttl_secs=TTL, idle_secs=IDLE, history=6)
    fb = ClickFeedback(index, capacity=8192, row_cap=HOW_MANY, ttl_secs=TTL, idle_secs=IDLE)
    out = replay(index, store, (t(keys[0]), t(keys[1])), t(items), t(times), t(consent), k=K, m=M, how_many=HOW_MANY, max_items_in_session=2, batch=1000, feedback=fb,
                 collect=True, **cfg["flags"])
    assert (out["requests"], out["calls"], out["boundaries"]) == (len(items), 2, 0) and out["feedback"] == ref["fb_stats"]
    assert out["ids"].cpu().numpy().view(np.uint64).tobytes() == ref["ids"].tobytes() and out["counts"].cpu().numpy().view(np.uint32).tobytes() == ref["counts"].tobytes()
    assert out["ranks"].cpu().numpy().view(np.uint32).tobytes() == ref["ranks"].tobytes()
    assert export_bytes(store.export(now=1)) == export_bytes(ref["store"])
    for o in (store, fb):
        o.close()
