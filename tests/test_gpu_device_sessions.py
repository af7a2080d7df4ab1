"""Device-resident session store and batched /v1/recommend (srn_device_sessions_*, srn_recommend_batch*): a batch must give what the reference's handler
(recommend_resource.rs:20-65 over sessions/mod.rs:37-72) gives for its requests served one after the other -- rows AND store.  Every request of every test is
compared against a Python model of the handler over the CPU oracle's canonical predict (ids and order identical, scores 1e-12 relative), except the scale test's
rows, which follow the sampling rule of the full-size parity gates."""
import threading

import numpy as np
import pytest

from helpers import flatten, small_dataset

pytestmark = pytest.mark.gpu

K, M, HOW_MANY = 50, 200, 21
U64 = 2**64 - 1
UNKNOWN = 999_999_999


class Model:
    """The handler's session logic: read under the idle rule, append unless the click repeats the last item, drop ONE from the front beyond the limit, store with now."""

    def __init__(self, idle=1200):
        self.idle, self.s = idle, {}

    def get(self, key, now):
        sess, t = self.s.get(key, ([], 0))
        return [] if now > t and now - t > self.idle else list(sess)

    def serve(self, key, item, consent, now, max_items):
        if not consent:
            return [item]
        sess = self.get(key, now)
        if not sess:
            sess.append(item)
        elif sess[-1] != item:
            sess.append(item)
            if len(sess) > max_items:
                sess.pop(0)
        self.s[key] = (sess, now)
        return list(sess)


@pytest.fixture(scope="module")
def small():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(33, n_sessions=3000, n_items=300)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 200, 12, 1.0)
    oix = O.OracleIndex(off, items, ts, 200, 12, 1.0, fast=True)
    yield gix, oix, ids
    gix.close()


def split_keys(keys):
    return np.array([k >> 64 for k in keys], np.uint64), np.array([k & U64 for k in keys], np.uint64)


def to_numpy(x):
    if isinstance(x, np.ndarray):
        return x
    a = x.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a.view(np.uint32) if a.dtype == np.int32 else a


def run(gix, store, keys, items, consent, now, max_items, entry, k=K, m=M, how_many=HOW_MANY):
    """One recommend_batch call through the host-pointer ('host') or the device-pointer ('device') entry point -> (ids, scores, counts) as NumPy arrays."""
    from serenade_amd.serving import recommend_batch
    hi, lo = split_keys(keys)
    it = np.asarray(items, np.uint64)
    con = None if consent is None else np.asarray(consent, np.uint8)
    if entry == "device":
        import torch
        dev = torch.device("cuda", gix.info["device"])
        hi, lo, it = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (hi, lo, it))
        con = None if con is None else torch.from_numpy(con).to(dev)
    ids, cnt, sc = recommend_batch(gix, store, (hi, lo), it, con, k=k, m=m, how_many=how_many, max_items_in_session=max_items, now=now, scores=True)
    if entry == "device":
        import torch
        torch.cuda.current_stream(gix.info["device"]).synchronize()
    return to_numpy(ids), to_numpy(sc), to_numpy(cnt)


def check_rows(oix, sessions, ids, sc, cnt, k=K, m=M, how_many=HOW_MANY, what=""):
    flat, qo = flatten(sessions)
    ref = oix.predict_batch("canonical", flat, qo, k, m, how_many, False, threads=4)
    assert np.array_equal(cnt, ref["counts"]), what
    bad = np.flatnonzero((ids != ref["ids"]).any(axis=1))
    assert len(bad) == 0, (what, bad[:5], [sessions[i] for i in bad[:5]])
    np.testing.assert_allclose(sc, ref["scores"], rtol=1e-12, atol=0)


def handler_stream(rng, ids, n_visitors, n_requests):
    """(session id, item, consent, seconds since the previous request): repeated clicks, 10 % unknown items, 15 % without consent, clock jumps past the idle limit."""
    out, last = [], {}
    for _ in range(n_requests):
        v = int(rng.integers(0, n_visitors))
        r = rng.random()
        if r < 0.25 and v in last:
            item = last[v]                                                      # the click repeats the visitor's previous one
        elif r < 0.35:
            item = UNKNOWN + int(rng.integers(0, 3))
        else:
            item = int(ids[rng.integers(0, len(ids))])
        last[v] = item
        dt = 1500 if rng.random() < 0.01 else int(rng.integers(0, 40))
        out.append(("visitor-%d" % v, item, rng.random() >= 0.15, dt))
    return out


@pytest.mark.parametrize("n_visitors", [12, 400])
def test_the_handler_replayed_in_batches(small, n_visitors):
    """The stream of test_recommend_follows_the_reference_handler, widened, cut into batches of 1..256 requests that share `now`; max_items_in_session changes between
    batches (also downwards).  Rows against the model over the oracle, the store against the model after every batch, and the same stream through srn_recommend."""
    from serenade_amd.serving import Batcher, DeviceSessionStore, SessionStore, recommend, session_key, session_keys
    gix, oix, ids = small
    rng = np.random.default_rng(5 + n_visitors)
    stream = handler_stream(rng, ids, n_visitors, 3200)
    all_sids = ["visitor-%d" % v for v in range(n_visitors)]
    key_of = {s: session_key(s) for s in all_sids}
    hi, lo = session_keys(all_sids)
    assert [(int(h) << 64) | int(l) for h, l in zip(hi, lo)] == [key_of[s] for s in all_sids]
    store = DeviceSessionStore(gix, capacity=1024, items_cap=8, ttl_secs=1800, idle_secs=1200)   # small enough for the capacity rule's count and sweep to run
    host_store, batcher = SessionStore(ttl_secs=1800, idle_secs=1200), Batcher(gix, K, M, HOW_MANY, False, max_batch=64, max_wait_us=50)
    model, now, at, batch_no = Model(), 10_000, 0, 0
    limits = [3, 5, 2, 1, 4, 2, 3]
    while at < len(stream):
        size = int(rng.integers(1, 257))
        chunk = stream[at:at + size]
        at += len(chunk)
        now += chunk[0][3] * (1 if batch_no % 5 else 40)                        # (every fifth batch: past the idle limit for most visitors)
        max_items = limits[batch_no % len(limits)]
        sessions = [model.serve(key_of[s], item, c, now, max_items) for s, item, c, _ in chunk]
        ids_, sc, cnt = run(gix, store, [key_of[s] for s, _, _, _ in chunk], [i for _, i, _, _ in chunk], [c for _, _, c, _ in chunk], now, max_items,
                            "device" if batch_no % 2 else "host")
        check_rows(oix, sessions, ids_, sc, cnt, what="batch %d" % batch_no)
        for s in all_sids:
            assert store.get_session_items(key_of[s], now=now) == model.get(key_of[s], now), (batch_no, s)
        for j, (s, item, c, _) in enumerate(chunk):                            # today's per-request path, request by request
            assert recommend(batcher, host_store, s, item, c, max_items, now=now) == [int(x) for x in ids_[j, :cnt[j]]], (batch_no, j)
        batch_no += 1
    st = store.stats
    assert st["refused"] == 0 and st["max_stored_len"] == 5 and st["live_bound"] <= 1024, st
    batcher.close()
    host_store.close()
    store.close()


def test_cut_invariance_and_entry_points(small):
    """One batch, and the same requests cut at random points into several calls (same now), write identical bytes and leave identical stores; so do the host-pointer and
    the device-pointer entry points."""
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    rng = np.random.default_rng(77)
    n, now, max_items = 3000, 50_000, 3
    keys = [(int(rng.integers(0, 2**63)) << 64) | int(rng.integers(0, 2**63)) for _ in range(300)]
    rk = [keys[int(rng.integers(0, len(keys)))] for _ in range(n)]
    items = [int(ids[rng.integers(0, 40)]) for _ in range(n)]
    consent = (rng.random(n) >= 0.15).astype(np.uint8)
    model = Model()
    sessions = [model.serve(k_, i, c, now, max_items) for k_, i, c in zip(rk, items, consent)]
    results, stores = [], []
    for entry, cuts in (("device", []), ("host", []), ("device", sorted(rng.integers(1, n, 9).tolist())), ("host", sorted(rng.integers(1, n, 14).tolist()))):
        store = DeviceSessionStore(gix, capacity=8192, items_cap=4)
        parts = [run(gix, store, rk[a:b], items[a:b], consent[a:b], now, max_items, entry) for a, b in zip([0] + cuts, cuts + [n]) if b > a]
        results.append(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)))
        stores.append(store)
    check_rows(oix, sessions, *results[0])
    for r in results[1:]:
        for a, b in zip(results[0], r):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for store in stores:
        assert [store.get_session_items(k_, now=now) for k_ in keys] == [model.get(k_, now) for k_ in keys]
        assert store.sweep(now=now) == len(model.s)
        store.close()


@pytest.mark.parametrize("timed", [False, True])
def test_the_scratch_grows_behind_a_call_that_may_still_run(small, timed):
    """Two device-pointer calls on one stream with nothing between them: one request, then 257 -- two blocks of 256 lanes and the n + 1 lane -- so the store's scratch is
    freed and reallocated while the first call may still read it: the grow rule waits for that call.  The second call repeats visitors, every seventh request does
    not consent and, timed, one gap lies above the idle limit.  Rows, counts and the store's export are the bytes of the same two calls on a fresh store with a
    synchronisation in between."""
    import torch
    from serenade_amd.serving import DeviceSessionStore, recommend_batch
    gix, oix, ids = small
    dev = torch.device("cuda", gix.info["device"])
    n, now, max_items, idle = 258, 90_000, 3, 1200
    vis = [((7 + v) << 64) | (11 * v + 1) for v in range(5)]
    hi, lo = split_keys([vis[j % 5] for j in range(n)])
    items = np.array([int(ids[(3 * j) % 17]) for j in range(n)], np.uint64)
    consent = (np.arange(n) % 7 != 3).astype(np.uint8)
    times = now + np.arange(n, dtype=np.uint64)
    times[200:] += np.uint64(idle + 1)
    assert consent[0] and consent[200] and not consent.all()
    hi, lo, items, times = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (hi, lo, items, times))   # every copy before the first call: none between the two
    consent = torch.from_numpy(consent).to(dev)
    stream = torch.cuda.current_stream(dev)
    results = []
    for synchronise in (False, True):
        store = DeviceSessionStore(gix, capacity=1024, items_cap=4, idle_secs=idle)   # (room for both calls by the host's bound: the capacity rule waits for nothing)
        stream.synchronize()
        rows = []
        for sl in (slice(0, 1), slice(1, n)):
            rows += recommend_batch(gix, store, (hi[sl], lo[sl]), items[sl], consent[sl], k=K, m=M, how_many=HOW_MANY, max_items_in_session=max_items, now=now,
                                    scores=True, times=times[sl] if timed else None)
            if synchronise:
                stream.synchronize()
        stream.synchronize()
        at = int(times[-1]) if timed else now
        (xhi, xlo), epoch, length, xitems = store.export(now=at)
        results.append([to_numpy(r) for r in rows] + [xhi, xlo, epoch, length, xitems])
        store.close()
    assert results[0][4].shape == (n - 1,) and len(results[0][-2]) == len(vis)       # counts of the second call; one stored session per visitor
    if timed:
        assert (results[0][-3] >= int(times[200])).all()                              # ... each of them stored behind the gap
    for a, b in zip(*results):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.timeout(300)
def test_hot_key(small):
    """65 536 requests on ONE key in one call (items from 5 ids: repeats and appends both occur), interleaved with 1 000 other keys: every row against the model."""
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    rng = np.random.default_rng(9)
    n_hot, n_other, now, max_items = 65_536, 1_000, 7_000, 3
    hot = (0x1234 << 64) | 0x5678
    others = [((i + 1) << 64) | (0x5678 + i) for i in range(n_other)]
    rk = [hot] * n_hot + others
    order = rng.permutation(len(rk))
    rk = [rk[i] for i in order]
    items = [int(ids[rng.integers(0, 5)]) for _ in rk]
    model = Model()
    sessions = [model.serve(k_, i, True, now, max_items) for k_, i in zip(rk, items)]
    assert len({tuple(s) for s in sessions}) > 50
    store = DeviceSessionStore(gix, capacity=70_000, items_cap=4)
    store.update_session_items(hot, [int(ids[7]), int(ids[8])], now=now - 10)           # the hot key starts from a stored session
    model2 = Model()
    model2.s[hot] = ([int(ids[7]), int(ids[8])], now - 10)
    sessions = [model2.serve(k_, i, True, now, max_items) for k_, i in zip(rk, items)]
    ids_, sc, cnt = run(gix, store, rk, items, None, now, max_items, "device")
    check_rows(oix, sessions, ids_, sc, cnt)
    assert store.get_session_items(hot, now=now) == model2.get(hot, now)
    for k_ in others[::37]:
        assert store.get_session_items(k_, now=now) == model2.get(k_, now)
    store.close()


def test_keys_are_compared_by_all_128_bits(small):
    """Keys that share lo and differ in hi, and the reverse; (0, 0) and (2^64 - 1, 2^64 - 1); 5 000 keys whose halves all have the same low 32 bits: sessions stay apart."""
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    low = 0xABCD1234
    keys = [0, (U64 << 64) | U64, U64, U64 << 64, 1, 1 << 64, (1 << 64) | 1, (7 << 64) | 9, (9 << 64) | 7, (7 << 64) | 7, (9 << 64) | 9]
    keys += [(((i // 71) << 32 | low) << 64) | ((i % 71) << 32 | low) for i in range(5000)]
    assert len(set(keys)) == len(keys)
    store = DeviceSessionStore(gix, capacity=3 * len(keys), items_cap=4)
    model, now = Model(), 1000
    rng = np.random.default_rng(3)
    for rnd in range(2):
        order = rng.permutation(len(keys))
        rk = [keys[i] for i in order] + [keys[i] for i in order[:1000]]
        items = [int(ids[(hash(k_) + 3 * rnd + j) % 120]) for j, k_ in enumerate(rk)]
        sessions = [model.serve(k_, i, True, now + rnd, 3) for k_, i in zip(rk, items)]
        ids_, sc, cnt = run(gix, store, rk, items, None, now + rnd, 3, "host" if rnd else "device")
        check_rows(oix, sessions, ids_, sc, cnt, what="round %d" % rnd)
        for k_ in keys:
            assert store.get_session_items(k_, now=now + rnd) == model.get(k_, now + rnd), hex(k_)
    assert store.sweep(now=now + 1) == len(keys)
    store.close()


def test_idle_and_ttl_clocks_of_the_device_store(small):
    """tests/test_session_store.py::test_idle_and_ttl_clocks through the device store's get / update / sweep; the sweep counts equal the host store's."""
    from serenade_amd import SerenadeError
    from serenade_amd.serving import DeviceSessionStore, SessionStore, session_key
    gix, _, _ = small
    st, host = DeviceSessionStore(gix.info["device"], 100, items_cap=8, ttl_secs=1800, idle_secs=1200), SessionStore()
    k_ = session_key("abc")
    other = session_key("abd")
    assert st.get_session_items(k_, now=1000) == []
    for s in (st, host):
        s.update_session_items(k_, [7, 8, 9], now=1000)
    assert st.get_session_items(k_, now=1000) == [7, 8, 9]
    assert st.get_session_items(other, now=1000) == []
    assert st.get_session_items(k_, now=1000 + 1200) == [7, 8, 9]
    assert st.get_session_items(k_, now=1000 + 1201) == []
    for s in (st, host):
        s.update_session_items(k_, [9], now=2300)
    assert st.get_session_items(k_, now=3400) == [9]
    assert st.sweep(now=2300 + 1800) == host.sweep(now=2300 + 1800) == 1
    assert st.sweep(now=2300 + 1801) == host.sweep(now=2300 + 1801) == 0
    assert st.get_session_items(k_, now=2300 + 1801) == []
    for s in (st, host):
        s.update_session_items(k_, [], now=5000)
        s.update_session_items(other, [4], now=5100)
    assert st.get_session_items(k_, now=5000) == []
    assert st.sweep(now=5000 + 1801) == host.sweep(now=5000 + 1801) == 1
    assert st.sweep(now=5100 + 1801) == host.sweep(now=5100 + 1801) == 0
    st.update_session_items(k_, list(range(8)), now=9000)
    with pytest.raises(SerenadeError) as e:
        st.update_session_items(k_, list(range(9)), now=9000)                       # items_cap bounds what a session may hold
    assert e.value.code == -4
    assert st.get_session_items(k_, now=9000) == list(range(8))
    with pytest.raises(SerenadeError) as e:
        st.get_session_items(k_, now=9000, cap=4)
    assert e.value.code == -4
    assert st.stats["sweeps"] == 4 and st.stats["ttl_secs"] == 1800 and st.stats["idle_secs"] == 1200 and st.stats["slots"] == 256
    st.close()
    host.close()
    d = DeviceSessionStore(gix.info["device"], 10, ttl_secs=0, idle_secs=0)       # 0 = the reference's defaults
    assert (d.stats["ttl_secs"], d.stats["idle_secs"], d.stats["slot_bytes"]) == (1800, 1200, 256)
    d.close()


class StoreTable:
    """helpers.capacity_rule_sequence's view of a DeviceSessionStore and the handler's Model: a request per key through recommend_batch, the rows not looked at"""

    def __init__(self, gix, ids, store):
        self.gix, self.ids, self.store, self.model = gix, ids, store, Model()

    def call(self, keys, now):
        items = [int(self.ids[j % 90]) for j in range(len(keys))]
        run(self.gix, self.store, keys, items, None, now, 2, "device")   # (a refusal raises here: the model stays as it was)
        for k_, i in zip(keys, items):
            self.model.serve(k_, i, True, now, 2)

    def stats(self):
        return self.store.stats

    def sweep(self, now):
        return self.store.sweep(now=now)

    def expire(self, now):
        self.model.s = {k_: (sess, t) for k_, (sess, t) in self.model.s.items() if not (now > t and now - t > 1800)}

    def check(self, keys):
        for k_ in keys:   # now = 1: whatever is stored, idle or not
            assert self.store.get_session_items(k_, now=1) == self.model.s.get(k_, ([], 0))[0], k_


@pytest.mark.parametrize("capacity", [1, 2, 3, 33, 1000])
def test_capacity_rule(small, capacity):
    from helpers import capacity_rule_sequence
    from serenade_amd import SerenadeError
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    if capacity != 1000:   # the rule at its smallest tables: 2, 4, 8 and 128 slots
        store = DeviceSessionStore(gix, capacity=capacity, items_cap=4, ttl_secs=1800, idle_secs=1200)
        assert store.stats["slots"] == {1: 2, 2: 4, 3: 8, 33: 128}[capacity]
        keys, extra = capacity_rule_sequence(StoreTable(gix, ids, store), capacity, 100_000, 1800)
        store.close()
        # with growth allowed, the visitor beyond the capacity makes the store grow instead: nothing is refused and nothing is lost
        store = DeviceSessionStore(gix, capacity=capacity, items_cap=4, ttl_secs=1800, idle_secs=1200, max_capacity=4 * capacity)
        table = StoreTable(gix, ids, store)
        table.call(keys, 100_000)
        table.call([extra], 100_000)
        st = store.stats
        assert store.growth()["grows"] == 1 and (st["refused"], st["sweeps"], st["live_bound"]) == (0, 0, capacity + 1), (st, store.growth())
        table.check(keys + [extra])
        store.close()
        return
    store = DeviceSessionStore(gix, capacity=1000, items_cap=4, ttl_secs=1800, idle_secs=1200)
    model, now = Model(), 100_000
    first = [(1 << 64) | i for i in range(600)]
    second = [(2 << 64) | i for i in range(600)]
    items = [int(ids[i % 90]) for i in range(600)]
    sessions = [model.serve(k_, i, True, now, 2) for k_, i in zip(first, items)]
    check_rows(oix, sessions, *run(gix, store, first, items, None, now, 2, "device"))
    with pytest.raises(SerenadeError) as e:
        run(gix, store, second, items, None, now, 2, "device")
    assert e.value.code == -2
    st = store.stats
    assert (st["live_bound"], st["sweeps"], st["refused"]) == (600, 0, 1), st
    for k_ in first:
        assert store.get_session_items(k_, now=now) == model.get(k_, now)
    for k_ in second[::50]:
        assert store.get_session_items(k_, now=now) == []
    later = now + 1800 + 1
    sessions = [model.serve(k_, i, True, later, 2) for k_, i in zip(second, items)]
    check_rows(oix, sessions, *run(gix, store, second, items, None, later, 2, "host"))   # the expired sessions make room: an automatic sweep
    st = store.stats
    assert (st["sweeps"], st["refused"]) == (1, 1) and st["live_bound"] == 600, st
    for k_ in first[::20] + second:
        assert store.get_session_items(k_, now=later) == model.get(k_, later)
    assert store.sweep(now=later) == 600
    store.close()


def _threaded_replay(gix, oix, ids, store_of_thread, n_threads, n_streams):
    import torch
    dev = gix.info["device"]
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_streams)]
    out, errs = [None] * n_threads, []

    def worker(t):
        try:
            rng = np.random.default_rng(100 + t)
            model, rows, keep = Model(), [], []
            visitors = [((t + 1) << 64) | v for v in range(60)]
            with torch.cuda.stream(streams[t % n_streams]):
                for b in range(12):
                    now = 20_000 + 30 * b
                    n = int(rng.integers(50, 400))
                    rk = [visitors[int(rng.integers(0, len(visitors)))] for _ in range(n)]
                    items = [int(ids[rng.integers(0, 30)]) for _ in range(n)]
                    consent = (rng.random(n) >= 0.1).astype(np.uint8)
                    sessions = [model.serve(k_, i, c, now, 3) for k_, i, c in zip(rk, items, consent)]
                    rows.append((sessions, run(gix, store_of_thread(t), rk, items, consent, now, 3, "device")))
            out[t] = (model, visitors, rows)
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(t,)) for t in range(n_threads)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for t, (model, visitors, rows) in enumerate(out):
        for sessions, r in rows:
            check_rows(oix, sessions, *r, what="thread %d" % t)
        for k_ in visitors:
            assert store_of_thread(t).get_session_items(k_, now=20_400) == model.get(k_, 20_400)


def test_four_threads_two_streams_one_store(small):
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    store = DeviceSessionStore(gix, capacity=32_768, items_cap=4)
    _threaded_replay(gix, oix, ids, lambda t: store, 4, 2)
    store.close()


def test_two_stores_on_two_streams(small):
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    stores = [DeviceSessionStore(gix, capacity=16_384, items_cap=4) for _ in range(2)]
    _threaded_replay(gix, oix, ids, lambda t: stores[t], 2, 2)
    [s.close() for s in stores]


def test_refusals(small):
    from serenade_amd import SerenadeError
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    store = DeviceSessionStore(gix, capacity=100, items_cap=4)
    key, item = [(5 << 64) | 6], [int(ids[0])]
    for entry in ("host", "device"):
        r = run(gix, store, [], [], None, 1000, 2, entry)                          # n = 0: nothing to do
        assert r[0].shape == (0, HOW_MANY) and r[2].shape == (0,)
        for kw, code in ((dict(max_items=0), -1), (dict(max_items=5), -4), (dict(max_items=2, how_many=513), -4), (dict(max_items=2, k=0), -1)):
            with pytest.raises(SerenadeError) as e:
                run(gix, store, key, item, None, 1000, entry=entry, **kw)
            assert e.value.code == code, (entry, kw)
        for consent in (None, [1]):
            with pytest.raises(SerenadeError) as e:
                run(gix, None, key, item, consent, 1000, 2, entry)                  # consent needs a store
            assert e.value.code == -1, (entry, consent)
        assert store.get_session_items(key[0], now=1000) == [] and store.stats["refused"] == 0      # nothing was changed by any of them
        check_rows(oix, [item, [UNKNOWN]], *run(gix, None, key * 2, item + [UNKNOWN], [0, 0], 1000, 2, entry))   # no consent: no store needed
        check_rows(oix, [item], *run(gix, store, key, item, [0], 1000, 2, entry))
        assert store.get_session_items(key[0], now=1000) == []                     # ... and none touched
    store.close()


def test_store_and_index_on_different_devices(small):
    from serenade_amd import SerenadeError, capi
    from serenade_amd.serving import DeviceSessionStore
    if capi.device_count() < 2:
        pytest.skip("a store and an index on different devices: this box has one GPU")
    gix, _, ids = small
    other = DeviceSessionStore(1 - gix.info["device"], capacity=100, items_cap=4)
    with pytest.raises(SerenadeError) as e:
        run(gix, other, [1], [int(ids[0])], None, 1000, 2, "host")
    assert e.value.code == -1
    other.close()


@pytest.mark.timeout(600)
def test_scale_on_the_tiny_config():
    """2^18 requests in calls of 2^16 over 50 000 visitors: the sessions the store emitted equal the model's for ALL requests; rows against the oracle for a seeded sample
    of 2 048 requests plus the first and last 32 of each call."""
    import torch
    import serenade_amd as sa
    from oracle import oracle as O
    from serenade_amd import synth
    from serenade_amd.serving import DeviceSessionStore, recommend_batch
    inter, n_items, k, m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    gix = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw)
    oix = O.OracleIndex(off, items, ts, m, 34, idfw, fast=True)
    known = np.unique(items)
    rng = np.random.default_rng(2024)
    n_calls, per_call, n_visitors, max_items = 4, 1 << 16, 50_000, 4
    n = n_calls * per_call
    vis = rng.integers(0, n_visitors, n)
    pop = np.minimum((rng.pareto(1.1, n) * 20).astype(np.int64), len(known) - 1)
    click = known[pop]
    click[rng.random(n) < 0.03] = UNKNOWN
    rep = np.flatnonzero(rng.random(n) < 0.2)
    rep = rep[rep >= 3]
    click[rep] = click[rep - 3]                                                    # (makes a share of the same visitor's consecutive clicks equal, with the next lines)
    vis[rep] = vis[rep - 3]
    consent = (rng.random(n) >= 0.1).astype(np.uint8)
    vkeys = [(int(a) << 64) | int(b) for a, b in zip(rng.integers(0, 2**63, n_visitors), rng.integers(0, 2**63, n_visitors))]
    hi, lo = split_keys([vkeys[v] for v in vis])
    store = DeviceSessionStore(gix, capacity=n_visitors + 2 * per_call, items_cap=8)
    dev = torch.device("cuda", gix.info["device"])
    model, sample = Model(), set(rng.choice(n, 2048, replace=False).tolist())
    sampled_sessions, sampled_rows, repeats_seen = [], [], 0
    for c in range(n_calls):
        a, b, now = c * per_call, (c + 1) * per_call, 1_000_000 + 700 * c             # (the third call finds some sessions idle)
        sessions = [model.serve(vkeys[v], int(i), bool(cs), now, max_items) for v, i, cs in zip(vis[a:b], click[a:b], consent[a:b])]
        t = [torch.from_numpy(x[a:b].view(np.int64)).to(dev) for x in (hi, lo, click)] + [torch.from_numpy(consent[a:b]).to(dev)]
        ids_, cnt, sc = recommend_batch(gix, store, (t[0], t[1]), t[2], t[3], k=k, m=m, how_many=21, max_items_in_session=max_items, now=now, scores=True)
        got_items, got_off = store.last_batch_sessions()
        flat, qo = flatten(sessions)
        assert np.array_equal(got_off, qo) and np.array_equal(got_items, flat), "call %d: emitted sessions differ from the model" % c
        repeats_seen += sum(1 for s in sessions if len(s) > 1)
        pick = sorted(set(range(32)) | set(range(per_call - 32, per_call)) | {j - a for j in sample if a <= j < b})
        ids_, sc, cnt = to_numpy(ids_), to_numpy(sc), to_numpy(cnt)
        sampled_sessions += [sessions[j] for j in pick]
        sampled_rows.append((ids_[pick], sc[pick], cnt[pick]))
    assert repeats_seen > n // 4
    check_rows(oix, sampled_sessions, *(np.concatenate([r[j] for r in sampled_rows]) for j in range(3)), k=k, m=m)
    assert store.stats["refused"] == 0
    store.close()
    gix.close()
