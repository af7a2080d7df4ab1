"""The device session store with a history window (srn_device_sessions_set_history) and SRN_FLAG_EXCLUDE_SEEN: the store keeps the last H clicks of a
visitor, predict reads the last max_items_in_session of them, and with the flag a request's rows leave out its window as the request sees it.

A Python model of the handler keeps a history list per visitor; rows are compared with the canonical CPU oracle (ids and counts exact, scores 1e-12) and, where two GPU
stores are compared, bit for bit.
"""
import numpy as np
import pytest

from helpers import flatten, small_dataset

pytestmark = pytest.mark.gpu

K, M, HOW_MANY, H, MAX_ITEMS = 100, 500, 21, 8, 2
U64 = 2**64 - 1
NONE = 0xFFFFFFFF


class Model:
    """The handler's session logic with `limit` items kept (the history window, or max_items_in_session for a plain store): read under the idle rule, append unless the
    click repeats the last item, drop ONE from the front beyond the limit, store with now.  A request sees (window, the session predict reads)."""

    def __init__(self, limit, idle=1200):
        self.limit, self.idle, self.s = limit, idle, {}

    def get(self, key, now):
        sess, t = self.s.get(key, ([], 0))
        return [] if now > t and now - t > self.idle else list(sess)

    def serve(self, key, item, consent, now, max_items):
        if not consent:
            return [item], [item]
        sess = self.get(key, now)
        if not sess or sess[-1] != item:
            sess.append(item)
            if len(sess) > self.limit:
                sess.pop(0)
        self.s[key] = (sess, now)
        return list(sess), sess[-max_items:]


@pytest.fixture(scope="module")
def dense():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(31, n_sessions=6000, n_items=150, max_len=12)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 3000, 20, 1.0)
    oix = O.OracleIndex(off, items, ts, 3000, 20, 1.0)
    rng = np.random.default_rng(4)
    known = np.unique(items)
    flags = rng.choice(np.array([0, 1, 2, 3, 0xFF], np.uint8), size=len(known), p=[0.1, 0.05, 0.55, 0.2, 0.1])
    gix.set_attributes(known, flags)
    oix.set_attributes(known, flags)
    yield gix, oix, ids
    gix.close()


def key_of(v):
    return (0x1234567800000000 + v) << 64 | (0xABCDEF0000000000 + 7919 * v)


def calls(ids, seed=3):
    """Six calls of ~300 requests over 40 visitors: several requests per key in a call, repeated clicks, 15 % without consent, one jump of `now` past the idle limit.
    Visitor 0 clicks in every call (more than 8 clicks in all), visitor 1 has five requests in the third call."""
    rng = np.random.default_rng(seed)
    out, now, last = [], 50_000, {}
    top = [int(x) for x in ids[:40]]   # (popular items: a visitor's earlier clicks are candidates of the later ones)
    for c in range(6):
        now += 2000 if c == 4 else 30
        reqs = []
        for _ in range(300):
            v = int(rng.integers(0, 40))
            item = last[v] if v in last and rng.random() < 0.2 else top[int(rng.integers(0, len(top)))]
            last[v] = item
            reqs.append((v, item, bool(rng.random() >= 0.15)))
        reqs += [(0, top[(3 * c + j) % 40], True) for j in range(3)]
        if c == 2:
            reqs += [(1, top[j], True) for j in (5, 6, 6, 7, 8)]
        out.append((now, [reqs[i] for i in rng.permutation(len(reqs))]))
    return out


def run(gix, store, reqs, now, entry, max_items=MAX_ITEMS, exclude_seen=False, how_many=HOW_MANY):
    from serenade_amd.serving import recommend_batch
    hi = np.array([key_of(v) >> 64 for v, _, _ in reqs], np.uint64)
    lo = np.array([key_of(v) & U64 for v, _, _ in reqs], np.uint64)
    it = np.array([i for _, i, _ in reqs], np.uint64)
    con = np.array([c for _, _, c in reqs], np.uint8)
    if entry == "device":
        import torch
        dev = torch.device("cuda", gix.info["device"])
        hi, lo, it = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (hi, lo, it))
        con = torch.from_numpy(con).to(dev)
    ids, cnt, sc = recommend_batch(gix, store, (hi, lo), it, con, k=K, m=M, how_many=how_many, max_items_in_session=max_items, now=now, scores=True, exclude_seen=exclude_seen)
    if entry == "device":
        import torch
        torch.cuda.current_stream(gix.info["device"]).synchronize()
        ids, sc, cnt = ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)
    return ids, sc, cnt


def check_rows(oix, sessions, windows, got, how_many=HOW_MANY, what=""):
    """Rows = the oracle's rows over every candidate (how_many + the longest window is enough), without the window's items, cut to how_many."""
    ids, sc, cnt = got
    wide = how_many + max([len(w) for w in windows] + [0])
    flat, qo = flatten(sessions)
    ref = oix.predict_batch("canonical", flat, qo, K, M, wide, False, threads=4)
    changed = 0
    for q in range(len(sessions)):
        n = int(ref["counts"][q])
        gone = set(windows[q])
        keep = [j for j in range(n) if int(ref["ids"][q, j]) not in gone][:how_many]
        changed += keep != list(range(min(n, how_many)))
        assert cnt[q] == len(keep), (what, q, sessions[q], windows[q], cnt[q], len(keep))
        assert np.array_equal(ids[q, :cnt[q]], ref["ids"][q, keep]), (what, q, sessions[q], windows[q])
        np.testing.assert_allclose(sc[q, :cnt[q]], ref["scores"][q, keep], rtol=1e-12, atol=0)
    return changed


def same_rows(got, ref, what):
    assert np.array_equal(got[2], ref[2]), what
    inside = np.arange(got[0].shape[1])[None, :] < got[2].astype(np.int64)[:, None]
    assert np.array_equal(got[0][inside], ref[0][inside]), what
    assert np.array_equal(got[1][inside].view(np.uint64), ref[1][inside].view(np.uint64)), what


def test_history_window_predicts_like_a_plain_store(dense):
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = dense
    store = DeviceSessionStore(gix, capacity=1024, items_cap=12, ttl_secs=1800, idle_secs=1200, history=H)
    twin = DeviceSessionStore(gix, capacity=1024, items_cap=12, ttl_secs=1800, idle_secs=1200)
    assert store.history == H and twin.history == 0
    model, longest = Model(H), 0
    for c, (now, reqs) in enumerate(calls(ids)):
        entry = "device" if c % 2 else "host"
        seen = [model.serve(key_of(v), item, con, now, MAX_ITEMS) for v, item, con in reqs]
        got = run(gix, store, reqs, now, entry)
        emitted = store.last_batch_sessions()
        ref = run(gix, twin, reqs, now, entry)
        same_rows(got, ref, "call %d against the plain store" % c)
        twin_emitted = twin.last_batch_sessions()
        assert np.array_equal(emitted[0], twin_emitted[0]) and np.array_equal(emitted[1], twin_emitted[1])
        want_flat, want_off = flatten([s for _, s in seen])
        assert np.array_equal(emitted[0], want_flat) and np.array_equal(emitted[1], want_off)
        check_rows(oix, [s for _, s in seen], [[] for _ in seen], got, what="call %d" % c)
        for v in range(40):
            assert store.get_session_items(key_of(v), now=now) == model.get(key_of(v), now), (c, v)
        longest = max([longest] + [len(w) for w, _ in seen])
    assert longest == H and store.stats["max_stored_len"] == H
    store.close()
    twin.close()


def test_exclude_seen_leaves_out_the_window(dense):
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = dense
    store = DeviceSessionStore(gix, capacity=1024, items_cap=12, ttl_secs=1800, idle_secs=1200, history=H)
    model, changed, total, clicks0 = Model(H), 0, 0, 0
    for c, (now, reqs) in enumerate(calls(ids)):
        seen = [model.serve(key_of(v), item, con, now, MAX_ITEMS) for v, item, con in reqs]
        got = run(gix, store, reqs, now, "device" if c % 2 else "host", exclude_seen=True)
        changed += check_rows(oix, [s for _, s in seen], [w for w, _ in seen], got, what="call %d" % c)
        total += len(reqs)
        clicks0 += sum(1 for v, _, con in reqs if v == 0 and con)
        if c == 2:
            assert sum(1 for v, _, con in reqs if v == 1 and con) >= 5
    assert clicks0 > H
    print("exclude_seen: the window changes %d of %d rows" % (changed, total))
    assert changed >= total // 4
    store.close()


def test_errors_and_the_flag_on_a_store_without_history(dense):
    import serenade_amd as sa
    from serenade_amd import capi
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = dense
    store = DeviceSessionStore(gix, capacity=1024, items_cap=6)
    with pytest.raises(sa.SerenadeError) as e:
        store.set_history(7)
    assert e.value.code == capi.SRN_ERANGE and store.history == 0
    store.set_history(3)
    now, reqs = calls(ids)[0]
    model = Model(3)
    seen = [model.serve(key_of(v), item, con, now, 2) for v, item, con in reqs]
    run(gix, store, reqs, now, "host")
    with pytest.raises(sa.SerenadeError) as e:
        run(gix, store, reqs, now + 1, "host", max_items=4)   # max_items_in_session above the history window
    assert e.value.code == capi.SRN_ERANGE
    with pytest.raises(sa.SerenadeError) as e:
        run(gix, store, reqs, now + 1, "device", exclude_seen=True, how_many=510)   # 510 + 3 > SRN_MAX_HOW_MANY
    assert e.value.code == capi.SRN_ERANGE
    for v in range(40):
        assert store.get_session_items(key_of(v), now=now) == model.get(key_of(v), now), "a refused call changed the store"
    store.close()
    # H = 0 with the flag: the session window is excluded
    plain, model = DeviceSessionStore(gix, capacity=1024, items_cap=6), Model(4)
    changed = 0
    for c, (now, reqs) in enumerate(calls(ids)[:2]):
        seen = [model.serve(key_of(v), item, con, now, 4) for v, item, con in reqs]
        got = run(gix, plain, reqs, now, "device" if c else "host", max_items=4, exclude_seen=True)
        changed += check_rows(oix, [s for _, s in seen], [w for w, _ in seen], got, what="H = 0, call %d" % c)
    assert changed > 0
    plain.close()


def test_save_and_load_keep_the_windows(dense, tmp_path):
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = dense
    store = DeviceSessionStore(gix, capacity=1024, items_cap=12, ttl_secs=1800, idle_secs=1200, history=H)
    model, cs = Model(H), calls(ids)
    for now, reqs in cs[:3]:
        for v, item, con in reqs:
            model.serve(key_of(v), item, con, now, MAX_ITEMS)
        run(gix, store, reqs, now, "host")
    now = cs[2][0]
    path = str(tmp_path / "windows.snap")
    store.save(path, now=now)
    store.close()
    back = DeviceSessionStore.load(gix, path)
    assert back.history == 0, "the history window is a runtime setting: not saved"
    windows = [model.get(key_of(v), now) for v in range(40)]
    assert max(len(w) for w in windows) > MAX_ITEMS
    for v in range(40):
        assert back.get_session_items(key_of(v), now=now) == windows[v]
    back.set_history(H)
    now, reqs = cs[3]
    seen = [model.serve(key_of(v), item, con, now, MAX_ITEMS) for v, item, con in reqs]
    got = run(gix, back, reqs, now, "device", exclude_seen=True)
    assert check_rows(oix, [s for _, s in seen], [w for w, _ in seen], got, what="after load") > 0
    for v in range(40):
        assert back.get_session_items(key_of(v), now=now) == model.get(key_of(v), now)
    back.close()


def test_resize_below_the_history_window_is_refused_per_call(dense):
    """set_history checks H against items_cap, and a later resize may lower items_cap: the next call must refuse (SRN_ERANGE, store unchanged) instead of growing
    windows beyond the slots."""
    import serenade_amd as sa
    from serenade_amd import capi
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = dense
    store = DeviceSessionStore(gix, capacity=1024, items_cap=12, history=10)
    now, reqs = calls(ids)[0]
    store.resize(1024, items_cap=6, now=now)          # (nothing stored yet: the resize itself has nothing to refuse)
    assert store.history == 10 and store.stats["items_cap"] == 6
    for entry in ("host", "device"):
        with pytest.raises(sa.SerenadeError) as e:
            run(gix, store, reqs, now, entry)
        assert e.value.code == capi.SRN_ERANGE
    assert store.count(now).occupied == 0, "a refused call changed the store"
    store.set_history(6)
    model = Model(6)
    seen = [model.serve(key_of(v), item, con, now, MAX_ITEMS) for v, item, con in reqs]
    check_rows(oix, [s for _, s in seen], [[] for _ in seen], run(gix, store, reqs, now, "device"), what="after set_history(6)")
    for v in range(40):
        assert store.get_session_items(key_of(v), now=now) == model.get(key_of(v), now)
    store.close()
