"""Trending items on the GPU (srn_device_sessions_top_items, srn_index_set_fallback_trending; srn_trending.hip).

Every comparison is exact, ids and counts, against serving.top_items_model on the same store's export(now=1): the model reads the arrays the store hands out, the device
path reads the table.  Stores are filled with import_entries, so the windows are the test's."""
import ctypes as C
import threading

import numpy as np
import pytest

from fill_cases import check_rows as check_filled_rows
from helpers import flatten, small_dataset

pytestmark = pytest.mark.gpu

K, M, HOW_MANY = 50, 200, 21
U64 = 2**64 - 1
UNKNOWN = 999_999_999
NO_CONSENT_ITEM = 777_777_777
TTL, IDLE = 1800, 1200
SENTINEL, SENTINEL32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A


def unknown(i):
    """an id the index does not know (the index's own ids lie above 10^12)"""
    return UNKNOWN <= int(i) < UNKNOWN + 100


@pytest.fixture(scope="module")
def small():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(33, n_sessions=3000, n_items=300)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 200, 12, 1.0)
    oix = O.OracleIndex(off, items, ts, 200, 12, 1.0, fast=True)
    yield gix, oix, ids
    gix.close()


def new_store(gix, capacity, items_cap, **kw):
    from serenade_amd.serving import DeviceSessionStore
    return DeviceSessionStore(gix, capacity=capacity, items_cap=items_cap, ttl_secs=TTL, idle_secs=IDLE, **kw)


def fill(store, windows, epochs, seed=1):
    """windows[i] (a list of ids) under a random distinct 128-bit key with epochs[i]"""
    rng = np.random.default_rng(seed)
    n = len(windows)
    hi = rng.integers(0, 2**63, size=n, dtype=np.uint64)
    lo = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(17)      # distinct
    ln = np.array([len(w) for w in windows], np.uint32)
    items = np.zeros((n, store.items_cap), np.uint64)
    for i, w in enumerate(windows):
        items[i, :len(w)] = np.array(w, np.uint64)
    store.import_entries((hi, lo), np.asarray(epochs, np.uint64), ln, items)


def top_raw(store, now, since, min_count, cap, arrays=True):
    """One call of the C entry point into buffers filled with a sentinel -> (ids[:written], counts[:written], ranked); nothing may be written beyond min(cap, ranked)."""
    from serenade_amd import capi
    ids, cnt, n = np.full(cap + 2, SENTINEL, np.uint64), np.full(cap + 2, SENTINEL32, np.uint32), C.c_size_t(12345)
    capi.check(capi.lib().srn_device_sessions_top_items(store._h, int(now), int(since), int(min_count), cap, capi.ptr(ids) if arrays else None,
                                                        capi.ptr(cnt) if arrays else None, C.byref(n)))
    got = min(cap, n.value)
    assert (ids[got:] == SENTINEL).all() and (cnt[got:] == SENTINEL32).all(), "written beyond min(cap, ranked)"
    return ids[:got], cnt[:got], n.value


def model_of(store, now, since=0, min_count=1, n=None):
    from serenade_amd.serving import top_items_model
    _, ep, ln, items = store.export(now=1)
    return top_items_model(ln, items, ep, n, now, TTL, since=since, min_count=min_count)


def check_against_model(store, now, since, min_counts=(1, 3), what=""):
    """cap in {0, 1, 7, ranked, ranked + 5} and cap = 0 with NULL arrays, for each min_count -> the ranked counts"""
    out = []
    for mc in min_counts:
        want_ids, want_cnt = model_of(store, now, since, mc)
        ranked = len(want_ids)
        for cap in (0, 1, 7, ranked, ranked + 5):
            ids, cnt, n = top_raw(store, now, since, mc, cap)
            assert n == ranked, (what, mc, cap, n, ranked)
            assert np.array_equal(ids, want_ids[:cap]) and np.array_equal(cnt, want_cnt[:cap]), (what, mc, cap)
        assert top_raw(store, now, since, mc, 0, arrays=False)[2] == ranked, (what, mc)
        out.append(ranked)
    return out


def zipf_windows(rng, n, items_cap, pool, repeat_share=1 / 3):
    """n windows of 1..items_cap ids drawn Zipf from pool; a share of them holds a repeated id (a copy of an earlier position)"""
    w = 1.0 / np.arange(1, len(pool) + 1) ** 1.1
    w /= w.sum()
    out = []
    for i in range(n):
        ln = int(rng.integers(1, items_cap + 1))
        win = [int(x) for x in pool[rng.choice(len(pool), size=ln, p=w)]]
        if ln >= 2 and rng.random() < repeat_share:
            a, b = sorted(int(x) for x in rng.choice(ln, size=2, replace=False))
            win[b] = win[a]
        out.append(win)
    return out


@pytest.mark.parametrize("items_cap", [12, 16, 40])
def test_slot_shapes(small, items_cap):
    """128-byte slots read by 8 lanes, 256-byte and larger ones by 16 (items_cap 40: 22 elements, two rounds of the lane group)."""
    gix, _, _ = small
    rng = np.random.default_rng(items_cap)
    pool = np.concatenate([np.array([0, U64], np.uint64), rng.integers(1, 2**63, size=200, dtype=np.uint64)])
    rng.shuffle(pool)                                                   # (0 and 2^64 - 1 somewhere in the Zipf order)
    n = 3000
    windows = zipf_windows(rng, n, items_cap, pool)
    windows[0], windows[1] = [0, U64, 0][:items_cap], [U64]
    epochs = 10_000 + (np.arange(n) * 7) % 2000
    now = 10_000 + TTL + 700                                            # entries with an epoch below 10 700 are past the TTL: 35 %
    store = new_store(gix, 4096, items_cap)
    try:
        assert store.stats["slot_bytes"] == {12: 128, 16: 256, 40: 384}[items_cap]
        fill(store, windows, epochs)
        old = int((epochs < 10_700).sum())
        assert 0.3 * n < old < 0.4 * n and store.count(now).live == n - old
        since = int(epochs[500])                                        # one entry's epoch exactly: it is in, the second below it is out
        assert since == 11_500
        ranked = check_against_model(store, now, 0, what="since 0") + check_against_model(store, now, since, what="since") + check_against_model(store, 1, 0, what="everything")
        assert ranked[0] >= ranked[1] > 0 and ranked[2] >= ranked[3] > 0 and ranked[4] >= ranked[0] >= ranked[2]
        ids_all, _ = model_of(store, 1)
        assert 0 in ids_all and U64 in ids_all
        assert model_of(store, now, since)[1].sum() > model_of(store, now, since + 1)[1].sum(), "the entry whose epoch is `since` is counted"
        # the Python method: the first n of the ranking
        ids, cnt = store.top_items(7, since=since, min_count=3, now=now)
        want = model_of(store, now, since, 3, n=7)
        assert np.array_equal(ids, want[0]) and np.array_equal(cnt, want[1]) and ids.dtype == np.uint64 and cnt.dtype == np.uint32
    finally:
        store.close()


def test_long_windows(small):
    """items_cap 255: 130 elements, nine rounds of the lane group; one id at positions 0, 100 and 254, another at 63 and 64 (two lanes, and the two halves of one pair's neighbours)."""
    gix, _, _ = small
    rng = np.random.default_rng(2)
    X, Y, n = 4_000_000_001, 4_000_000_002, 300
    windows = []
    for _ in range(n):
        win = [int(x) for x in rng.integers(1, 2000, size=255)]
        win[0] = win[100] = win[254] = X
        win[63] = win[64] = Y
        windows.append(win)
    store = new_store(gix, 512, 255)
    try:
        fill(store, windows, np.full(n, 5000))
        check_against_model(store, 1, 0, min_counts=(1, n))
        ids, cnt, ranked = top_raw(store, 1, 0, n, 10)
        assert ranked >= 2 and {X, Y} <= set(int(i) for i in ids) and (cnt == n).all(), "X and Y are counted once per entry"
        assert int(np.sum(model_of(store, 1)[1])) < n * 255
    finally:
        store.close()


def test_ties(small):
    """64 ids with the same count between ids with larger and smaller ones: id ascending inside the group, and a cap inside it cuts at the model's place."""
    gix, _, _ = small
    rng = np.random.default_rng(3)
    tied = [int(x) for x in rng.integers(1, 2**64 - 1, size=64, dtype=np.uint64)]
    above, below = list(range(100, 110)), list(range(200, 230))
    windows = []
    for t in range(8):                                                  # `above`: 8 entries each; tied: 5; below: 1..3
        windows += [[a] for a in above]
    for t in range(5):
        order = rng.permutation(64)
        windows += [[tied[i], tied[j], tied[i]] for i, j in zip(order[::2], order[1::2])]
    windows += [[b] for i, b in enumerate(below) for _ in range(1 + i % 3)]
    store = new_store(gix, 1024, 12)
    try:
        fill(store, [windows[i] for i in rng.permutation(len(windows))], np.full(len(windows), 5000))
        check_against_model(store, 1, 0, min_counts=(1, 5))
        ids, cnt, ranked = top_raw(store, 1, 0, 1, 10 + 64)
        assert ranked == 104 and (cnt[:10] == 8).all() and (cnt[10:] == 5).all()
        assert [int(i) for i in ids[10:]] == sorted(tied)
        for cap in (11, 30, 73):
            cut, _, _ = top_raw(store, 1, 0, 1, cap)
            assert [int(i) for i in cut[10:]] == sorted(tied)[:cap - 10]
    finally:
        store.close()


def test_same_set_same_answer(small, tmp_path):
    from serenade_amd.serving import DeviceSessionStore
    gix, _, _ = small
    rng = np.random.default_rng(4)
    pool = rng.integers(1, 2**63, size=150, dtype=np.uint64)
    n = 1000
    epochs = 10_000 + (np.arange(n) * 13) % 2000
    now = 10_000 + TTL + 500
    store = new_store(gix, 2048, 12)
    loaded = None
    try:
        fill(store, zipf_windows(rng, n, 12, pool), epochs)
        first = top_raw(store, now, 10_900, 2, 4096)
        assert first[2] > 20

        def same(what):
            again = top_raw(store if loaded is None else loaded, now, 10_900, 2, 4096)
            assert again[2] == first[2] and again[0].tobytes() == first[0].tobytes() and again[1].tobytes() == first[1].tobytes(), what
        same("two calls in a row")
        assert store.sweep(now=now) < n
        same("after a sweep")
        store.resize(5000, items_cap=20, now=now)
        assert store.stats["slot_bytes"] == 256
        same("after a resize to another capacity and items_cap")
        store.save(tmp_path / "s.snap", now=now)
        loaded = DeviceSessionStore.load(gix, tmp_path / "s.snap")
        same("after save / load")
    finally:
        store.close()
        if loaded is not None:
            loaded.close()


def test_many_workgroups_and_sort_blocks(small):
    """2^17 entries of items_cap 16, ids Zipf over 50 000: some two million ids through the sorts."""
    gix, _, _ = small
    rng = np.random.default_rng(5)
    n, cap = 1 << 17, 16
    pool = rng.permutation(np.arange(1, 50_001, dtype=np.uint64) * np.uint64(2**40 + 1))
    w = 1.0 / np.arange(1, 50_001) ** 1.05
    items = pool[rng.choice(50_000, size=(n, cap), p=w / w.sum())]
    ln = rng.integers(1, cap + 1, size=n).astype(np.uint32)
    hi, lo = rng.integers(0, 2**63, size=n, dtype=np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    epochs = (20_000 + np.arange(n) % 3000).astype(np.uint64)
    store = new_store(gix, n, cap)
    try:
        store.import_entries((hi, lo), epochs, ln, items)
        now = 20_000 + TTL + 1000
        want_ids, want_cnt = model_of(store, now, 21_500, 1)
        ids, cnt, ranked = top_raw(store, now, 21_500, 1, len(want_ids))
        assert ranked == len(want_ids) > 10_000
        assert np.array_equal(ids, want_ids) and np.array_equal(cnt, want_cnt)
        want_ids, want_cnt = model_of(store, 1, 0, 2)
        ids, cnt, ranked = top_raw(store, 1, 0, 2, 256)
        assert ranked == len(want_ids) and np.array_equal(ids, want_ids[:256]) and np.array_equal(cnt, want_cnt[:256])
    finally:
        store.close()


class Model:
    """The handler's session logic with `limit` items kept (tests/test_gpu_fill_sessions.py) -> (window, the session predict reads)."""

    def __init__(self, limit, idle=IDLE):
        self.limit, self.idle, self.s = limit, idle, {}

    def serve(self, key, item, consent, now, max_items):
        if not consent:
            return [item], [item]
        sess, t = self.s.get(key, ([], 0))
        sess = [] if now > t and now - t > self.idle else list(sess)
        if not sess or sess[-1] != item:
            sess.append(item)
            if len(sess) > self.limit:
                sess.pop(0)
        self.s[key] = (sess, now)
        return list(sess), sess[-max_items:]


def key_of(v):
    return (0x1234567800000000 + v) << 64 | (0xABCDEF0000000000 + 7919 * v)


def traffic(ids, n_calls, per_call, visitors, seed):
    """(now, [(visitor, item, consent)]): several requests per key in a call, a tenth without consent (their item is clicked by nobody else), a tenth unknown items"""
    rng = np.random.default_rng(seed)
    out, now = [], 50_000
    for _ in range(n_calls):
        now += 30
        reqs = []
        for _ in range(per_call):
            consent = bool(rng.random() >= 0.1)
            item = NO_CONSENT_ITEM if not consent else UNKNOWN + int(rng.integers(0, 3)) if rng.random() < 0.1 else int(ids[min(int(rng.zipf(1.3)) - 1, len(ids) - 1)])
            reqs.append((int(rng.integers(0, visitors)), item, consent))
        out.append((now, reqs))
    return out


def recommend(gix, store, reqs, now, max_items=2, **kw):
    from serenade_amd.serving import recommend_batch
    hi = np.array([key_of(v) >> 64 for v, _, _ in reqs], np.uint64)
    lo = np.array([key_of(v) & U64 for v, _, _ in reqs], np.uint64)
    it = np.array([i for _, i, _ in reqs], np.uint64)
    con = np.array([c for _, _, c in reqs], np.uint8)
    ids, cnt, sc = recommend_batch(gix, store, (hi, lo), it, con, k=K, m=M, how_many=HOW_MANY, max_items_in_session=max_items, now=now, scores=True, **kw)
    return ids, sc, cnt


def check_model_rows(oix, sessions, got, what):
    ids, sc, cnt = got
    flat, qo = flatten(sessions)
    ref = oix.predict_batch("canonical", flat, qo, K, M, HOW_MANY, False, threads=4)
    assert np.array_equal(cnt, ref["counts"]) and np.array_equal(ids, ref["ids"]), what
    np.testing.assert_allclose(sc, ref["scores"], rtol=1e-12, atol=0)


def same_export(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip((a[0][0], a[0][1]) + tuple(a[1:]), (b[0][0], b[0][1]) + tuple(b[1:])))


def test_between_batches_of_traffic(small):
    gix, oix, ids = small
    store = new_store(gix, 2048, 12, history=8)
    model = Model(8)
    try:
        for c, (now, reqs) in enumerate(traffic(ids, 5, 400, 150, seed=6)):
            sessions = [model.serve(key_of(v), item, con, now, 2)[1] for v, item, con in reqs]
            check_model_rows(oix, sessions, recommend(gix, store, reqs, now), "call %d" % c)        # (from the second call on: the batch behind a top_items)
            before = store.export(now=1)
            got = store.top_items(4096, now=now)
            after = store.export(now=1)
            assert same_export(before, after), "top_items changed the store"
            want = model_of(store, now)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), c
            assert NO_CONSENT_ITEM not in got[0], "a click without consent was counted"
            assert any(unknown(i) for i in got[0]), "ids unknown to the index are counted like any other"
            # and the model's windows are what was counted
            counts = {}
            for sess, t in model.s.values():
                for i in set(sess):
                    counts[i] = counts.get(i, 0) + 1
            assert {int(i): int(n) for i, n in zip(*got)} == counts, c
    finally:
        store.close()


@pytest.mark.timeout(120)
def test_two_threads(small):
    """The store's mutex makes a top_items call atomic against a batch: every result is the model's at one of the 21 batch boundaries."""
    gix, _, ids = small
    calls = traffic(ids, 20, 300, 200, seed=7)
    twin = new_store(gix, 8192, 12, history=8)
    store = new_store(gix, 8192, 12, history=8)
    try:
        boundaries = [model_of(twin, 1)]
        for now, reqs in calls:
            recommend(gix, twin, reqs, now)
            boundaries.append(model_of(twin, 1))
        assert len(boundaries[0][0]) == 0 and len(boundaries[-1][0]) > 50
        keys = [(b[0].tobytes(), b[1].tobytes()) for b in boundaries]
        results, errors, done = [], [], threading.Event()

        def batches():
            try:
                for now, reqs in calls:
                    recommend(gix, store, reqs, now)
            except Exception as e:      # noqa: BLE001
                errors.append(e)
            finally:
                done.set()

        def reader():
            try:
                while True:
                    last = done.is_set()
                    results.append(store.top_items(4096, now=1))
                    if last:
                        return
            except Exception as e:      # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=batches), threading.Thread(target=reader)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=100)
        assert not any(t.is_alive() for t in threads), "deadlock"
        assert not errors, errors
        seen = [keys.index((r[0].tobytes(), r[1].tobytes())) for r in results]      # (ValueError: a result that is no boundary's)
        assert seen == sorted(seen) and seen[-1] == 20, seen
        print("top_items ran %d times, at boundaries %s" % (len(results), sorted(set(seen))))
    finally:
        store.close()
        twin.close()


def test_empty(small):
    gix, _, _ = small
    store = new_store(gix, 256, 16)
    try:
        assert top_raw(store, 1, 0, 1, 8)[2] == 0 and top_raw(store, 0, 0, 0, 0, arrays=False)[2] == 0
        fill(store, [[1, 2], [2, 3], [5]], [1000, 1001, 1002])
        assert top_raw(store, 1000 + TTL, 0, 1, 8)[2] == 4
        assert top_raw(store, 1002 + TTL + 1, 0, 1, 8)[2] == 0, "every entry is older than the TTL"
        assert top_raw(store, 1, 1003, 1, 8)[2] == 0, "no epoch reaches since"
        ids, cnt = store.top_items(8, now=1002 + TTL + 1)
        assert len(ids) == 0 and len(cnt) == 0
        assert store.count(1).live == 3
    finally:
        store.close()


def clicked_store(gix, ids, n_visitors=120, seed=8):
    """A store filled through recommend_batch: Zipf clicks on 40 known items and on three ids the index does not know"""
    store = new_store(gix, 1024, 12, history=6)
    rng = np.random.default_rng(seed)
    pool = [int(x) for x in ids[:40]] + [UNKNOWN + 1, UNKNOWN + 2]
    rng.shuffle(pool)
    pool = [UNKNOWN] + pool                                             # (the most clicked id is one the index does not know)
    now = 70_000
    for _ in range(4):
        now += 20
        reqs = [(int(rng.integers(0, n_visitors)), pool[min(int(rng.zipf(1.4)) - 1, len(pool) - 1)], True) for _ in range(300)]
        recommend(gix, store, reqs, now)
    return store, now


def test_set_fallback_trending_list(small):
    import serenade_amd as sa
    from serenade_amd import capi
    gix, _, ids = small
    store, now = clicked_store(gix, ids)
    try:
        gix.set_fallback_popular(300)
        popular = [int(x) for x in gix.fallback()]
        assert len(popular) == 300
        trend = [int(x) for x in model_of(store, now)[0]]
        assert 10 < len(trend) <= 43 and unknown(trend[0]), "ids the index does not know are in the ranking"
        # fewer trending ids than n: the popularity order behind them, without repeats, n in all
        assert gix.set_fallback_trending(store, 64, now=now) == len(trend)
        want = trend + [p for p in popular if p not in set(trend)]
        assert [int(x) for x in gix.fallback()] == want[:64]
        # without the tail: the trending ids alone; min_count and since as top_items reads them
        assert gix.set_fallback_trending(store, 64, popular_tail=False, now=now) == len(trend)
        assert [int(x) for x in gix.fallback()] == trend
        t3 = [int(x) for x in model_of(store, now, since=now - 20, min_count=3)[0]]
        assert 0 < len(t3) < len(trend)
        assert gix.set_fallback_trending(store, 64, since=now - 20, min_count=3, popular_tail=False, now=now) == len(t3)
        assert [int(x) for x in gix.fallback()] == t3
        # more trending ids than n: the first n
        assert gix.set_fallback_trending(store, 10, now=now) == 10
        assert [int(x) for x in gix.fallback()] == trend[:10]
        # the limits
        assert gix.set_fallback_trending(store, capi.MAX_FALLBACK, now=now) == len(trend)
        assert [int(x) for x in gix.fallback()] == want
        with pytest.raises(sa.SerenadeError) as e:
            gix.set_fallback_trending(store, capi.MAX_FALLBACK + 1, now=now)
        assert e.value.code == capi.SRN_ERANGE
        with pytest.raises(sa.SerenadeError) as e:
            gix.set_fallback_trending(store, 0, now=now)
        assert e.value.code == capi.SRN_EINVAL
        assert [int(x) for x in gix.fallback()] == want
        # nothing in range and no tail: the ranking stays; with the tail it is the popularity order
        assert gix.set_fallback_trending(store, 64, since=now + 1, popular_tail=False, now=now) == 0
        assert [int(x) for x in gix.fallback()] == want
        assert gix.set_fallback_trending(store, 64, since=now + 1, now=now) == 0
        assert [int(x) for x in gix.fallback()] == popular[:64]
        got = C.c_size_t(99)
        capi.check(capi.lib().srn_index_set_fallback_trending(gix._h, store._h, now, 0, 1, 5, 0, None))           # out_trending may be NULL
        capi.check(capi.lib().srn_index_set_fallback_trending(gix._h, store._h, now, 0, 1, 5, 0, C.byref(got)))
        assert got.value == 5 and [int(x) for x in gix.fallback()] == trend[:5]
    finally:
        gix.clear_fallback()
        store.close()


def test_set_fallback_trending_serves(small):
    import serenade_amd as sa
    from serenade_amd import capi
    from serenade_amd.serving import fill_rows
    from serenade_amd.sharded import postings_view
    gix, oix, ids = small
    store, now = clicked_store(gix, ids)
    try:
        assert gix.set_fallback_trending(store, 64, now=now) > 10
        ranking = [int(x) for x in gix.fallback()]
        # queries whose clicked item the index does not know: the rows are the ranking's
        sessions = [[UNKNOWN + 7], [UNKNOWN], [int(ids[3]), UNKNOWN + 1], [UNKNOWN + 2, UNKNOWN + 9], [int(ids[5])]]
        flat, qo = flatten(sessions)
        ref = oix.predict_batch("canonical", flat, qo, K, M, HOW_MANY, False, threads=2)
        assert (ref["counts"][[0, 1, 3]] == 0).all()
        want = fill_rows(ref["ids"], ref["scores"], ref["counts"], sessions, ranking, HOW_MANY)
        got = sa.predict_batch(gix, sa.CSR(flat, qo), K, M, HOW_MANY, False, fill=True)
        check_filled_rows(got, want, "predict_batch with the trending ranking")
        assert (got[2] == HOW_MANY).all() and np.isneginf(got[1][0]).all()
        assert [int(x) for x in got[0][0]] == ranking[:HOW_MANY]
        assert UNKNOWN not in got[0][1] and any(unknown(x) for x in got[0][0])
        # behind the store: a visitor's window never comes back
        reqs = [(v, UNKNOWN + 5 if v % 3 == 0 else int(ids[v % 40]), True) for v in range(120)]
        rows, _, cnt = recommend(gix, store, reqs, now + 5, exclude_seen=True, fill=True)
        assert (cnt == HOW_MANY).all()
        for q, (v, _, _) in enumerate(reqs):
            window = store.get_session_items(key_of(v), now=now + 5)
            assert len(window) >= 1 and not set(window) & set(int(x) for x in rows[q]), (q, window)
        # refusals: an index without a device, a postings-only view
        off, items, ts, _ = small_dataset(3, n_sessions=200, n_items=40)
        host_only = sa.VMISIndex.from_sessions(off, items, ts, 100, 12, 1.0, device=-1)
        view = postings_view(gix, gix.info["device"])
        try:
            for ix, code in ((host_only, capi.SRN_ENODEV), (view, capi.SRN_EINVAL)):
                with pytest.raises(sa.SerenadeError) as e:
                    ix.set_fallback_trending(store, 8, now=now)
                assert e.value.code == code and "srn_index_set_fallback_trending" in str(e.value)
        finally:
            host_only.close()
            view.close()
    finally:
        gix.clear_fallback()
        store.close()
