"""Snapshot, restore, merge and grow of the device session store (srn_device_sessions_count / _export* / _import* / _resize / _set_max_capacity / _growth / _save /
_load): every store is compared against the Python model of the handler (tests/test_gpu_device_sessions.py) -- keys, lengths, items and epochs exactly -- and every
row that is served against the model over the CPU oracle's canonical predict (ids and order identical, scores 1e-12 relative)."""
import ctypes as C
import threading

import numpy as np
import pytest

from helpers import flatten, small_dataset

pytestmark = pytest.mark.gpu

K, M, HOW_MANY = 50, 200, 21
U64 = 2**64 - 1
UNKNOWN = 999_999_999
TTL, IDLE = 1800, 1200


class Model:
    """The handler's session logic: read under the idle rule, append unless the click repeats the last item, drop ONE from the front beyond the limit, store with now."""

    def __init__(self, idle=IDLE):
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

    def live(self, now, ttl=TTL):
        """what a sweep at `now` keeps: {key: (items, epoch)}"""
        return {k: (tuple(sess), t) for k, (sess, t) in self.s.items() if not (now > t and now - t > ttl)}


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


def handler_stream(rng, ids, n_visitors, n_requests, drift=0):
    """(visitor, item, consent, seconds since the previous request): repeated clicks, 10 % unknown items, 15 % without consent, clock jumps past the idle limit.
    drift: the visitors come from a window of n_visitors / 4 that moves over the stream, so that the early ones fall silent -- past the idle limit, then past the TTL."""
    out, last = [], {}
    for j in range(n_requests):
        if drift:
            v = (j * (n_visitors - n_visitors // 4) // n_requests + int(rng.integers(0, n_visitors // 4))) % n_visitors
        else:
            v = int(rng.integers(0, n_visitors))
        r = rng.random()
        if r < 0.25 and v in last:
            item = last[v]
        elif r < 0.35:
            item = UNKNOWN + int(rng.integers(0, 3))
        else:
            item = int(ids[rng.integers(0, len(ids))])
        last[v] = item
        dt = 1500 if rng.random() < 0.01 else int(rng.integers(0, 40))
        out.append((v, item, rng.random() >= 0.15, dt))
    return out


def key_of(v):
    """a 128-bit key per visitor; the halves repeat among visitors (hi has 7 values, lo 61), the pair does not below 427"""
    return ((0x9E3779B97F4A7C15 * (v % 7 + 1) & U64) << 64) | (0xC2B2AE3D27D4EB4F * (v % 61 + 1) & U64)


def serve_stream(gix, oix, stores, model, stream, now, rng, limits, entries=("host", "device"), rows=True):
    """Cuts the stream into batches of 1..256 requests that share `now`, serves each to every store and checks the rows (identical between the stores; against the oracle).
    -> the clock after the last batch."""
    at, batch_no = 0, 0
    while at < len(stream):
        chunk = stream[at:at + int(rng.integers(1, 257))]
        at += len(chunk)
        now += min(chunk[0][3] * (1 if batch_no % 5 else 40), 2000)               # (every fifth batch: past the idle limit for most visitors, at times past the TTL)
        max_items = limits[batch_no % len(limits)]
        sessions = [model.serve(key_of(v), item, c, now, max_items) for v, item, c, _ in chunk]
        got = [run(gix, st, [key_of(v) for v, _, _, _ in chunk], [i for _, i, _, _ in chunk], [c for _, _, c, _ in chunk], now, max_items,
                   entries[(batch_no + j) % len(entries)]) for j, st in enumerate(stores)]
        for g in got[1:]:
            for a, b in zip(got[0], g):
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), "batch %d: the stores' rows differ" % batch_no
        if rows:
            check_rows(oix, sessions, *got[0], what="batch %d" % batch_no)
        batch_no += 1
    return now


def export_arrays(store, now, device=False):
    (hi, lo), ep, ln, it = store.export(now=now, device=device)
    if device:
        import torch
        torch.cuda.current_stream(store.device).synchronize()
    return [np.ascontiguousarray(to_numpy(a)) for a in (hi, lo, ep, ln, it)]


def export_bytes(store, now=1):
    return b"|".join(a.tobytes() for a in export_arrays(store, now))


def as_dict(arrays):
    """the export as {key: (items, epoch)}: every key once, zero padding beyond len"""
    hi, lo, ep, ln, it = arrays
    assert hi.dtype == lo.dtype == ep.dtype == it.dtype == np.uint64 and ln.dtype == np.uint32
    assert len(hi) == len(lo) == len(ep) == len(ln) == len(it)
    out = {}
    for h, l, e, n, row in zip(hi, lo, ep, ln, it):
        assert not row[n:].any(), "items beyond len are not zero"
        out[(int(h) << 64) | int(l)] = (tuple(int(x) for x in row[:n]), int(e))
    assert len(out) == len(hi), "a key was exported twice"
    return out


def entries_of(d, stride):
    """{key: (items, epoch)} -> the arrays import_entries takes"""
    keys = list(d)
    hi, lo = split_keys(keys)
    ep = np.array([d[k][1] for k in keys], np.uint64)
    ln = np.array([len(d[k][0]) for k in keys], np.uint32)
    it = np.zeros((len(keys), stride), np.uint64)
    for i, k in enumerate(keys):
        it[i, :ln[i]] = d[k][0]
    return (hi, lo), ep, ln, it


def raw_entries(rows, stride):
    """[(key, epoch, items)] in that order, duplicates kept -> import_entries' arrays"""
    hi, lo = split_keys([r[0] for r in rows])
    it = np.zeros((len(rows), stride), np.uint64)
    for i, r in enumerate(rows):
        it[i, :len(r[2])] = r[2]
    return (hi, lo), np.array([r[1] for r in rows], np.uint64), np.array([len(r[2]) for r in rows], np.uint32), it


@pytest.mark.parametrize("items_cap", [1, 12, 13, 16])
def test_export_equals_the_model(small, items_cap):
    """400 visitors, 3 000 requests whose visitors drift so that the early ones pass the idle limit and then the TTL.  The export at `now` is the model restricted
    to the entries younger than the TTL, idle ones included; a second export has the same bytes; a too small cap is refused (host) or cut (device)."""
    import torch
    from serenade_amd import capi
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    rng = np.random.default_rng(11 + items_cap)
    stream = handler_stream(rng, ids, 400, 3000, drift=1)
    store = DeviceSessionStore(gix, capacity=4096, items_cap=items_cap, ttl_secs=TTL, idle_secs=IDLE)
    model = Model()
    limits = [min(l, items_cap) for l in (3, 5, 2, 1, 4, 16, 3)]
    end = serve_stream(gix, oix, [store], model, stream, 10_000, rng, limits, rows=False)
    again = [key_of(v) for v in range(380, 400)]                                 # 20 visitors come back 700 s later; the export is taken 600 s after that:
    for k in again:                                                              # the stream's last 500 s are idle but not expired, everything before is expired
        model.serve(k, int(ids[3]), True, end + 700, limits[0])
    run(gix, store, again, [int(ids[3])] * 20, None, end + 700, limits[0], "device")
    now = end + 1300
    want = model.live(now)
    n_idle = sum(1 for _, t in want.values() if now - t > IDLE)
    assert 0 < n_idle < len(want) < len(model.s), "the stream must leave expired entries, idle-but-not-expired ones and fresh ones"
    arrays = export_arrays(store, now)
    assert arrays[4].shape == (len(want), items_cap)
    assert as_dict(arrays) == want
    assert store.count(now).live == len(want) and store.count(now).occupied == len(model.s)
    assert as_dict(export_arrays(store, 1)) == model.live(1) and len(model.live(1)) == len(model.s)          # now = 1: everything
    assert b"|".join(a.tobytes() for a in arrays) == export_bytes(store, now)                                # the order is the slots': unchanged store, same bytes
    dev_arrays = export_arrays(store, now, device=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(arrays, dev_arrays))
    # cap = live - 1.  host form: SRN_ERANGE, *n = live, the arrays untouched
    live, L = len(want), capi.lib()
    hi, lo, ep = (np.full(live, 0xABABABABABABABAB, np.uint64) for _ in range(3))
    ln, it, n = np.full(live, 0xABABABAB, np.uint32), np.full((live, items_cap), 0xABABABABABABABAB, np.uint64), C.c_size_t()
    rc = L.srn_device_sessions_export(store._h, now, live - 1, capi.ptr(hi), capi.ptr(lo), capi.ptr(ep), capi.ptr(ln), capi.ptr(it), items_cap, C.byref(n))
    assert rc == capi.SRN_ERANGE and n.value == live
    assert (hi == 0xABABABABABABABAB).all() and (lo == hi).all() and (ep == hi).all() and (ln == 0xABABABAB).all() and (it == 0xABABABABABABABAB).all()
    assert L.srn_device_sessions_export(store._h, now, live, capi.ptr(hi), capi.ptr(lo), capi.ptr(ep), capi.ptr(ln), capi.ptr(it), items_cap, None) == capi.SRN_EINVAL
    if items_cap > 1:   # items_stride below the longest session the store may hold
        assert L.srn_device_sessions_export(store._h, now, live, capi.ptr(hi), capi.ptr(lo), capi.ptr(ep), capi.ptr(ln), capi.ptr(it), 1, C.byref(n)) == capi.SRN_ERANGE
    # device form: exactly cap entries written, d_n = live
    dev = torch.device("cuda", store.device)
    t_hi, t_lo, t_ep = (torch.full((live,), -2, dtype=torch.int64, device=dev) for _ in range(3))
    t_ln, t_it = torch.full((live,), -2, dtype=torch.int32, device=dev), torch.full((live, items_cap), -2, dtype=torch.int64, device=dev)
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    capi.check(L.srn_device_sessions_export_device(store._h, now, live - 1, *(C.c_void_p(t.data_ptr()) for t in (t_hi, t_lo, t_ep, t_ln, t_it)), items_cap,
                                                   C.c_void_p(d_n.data_ptr()), C.c_void_p(torch.cuda.current_stream(store.device).cuda_stream)))
    assert int(d_n.item()) == live
    for t, a in zip((t_hi, t_lo, t_ep, t_ln, t_it), arrays):
        got = to_numpy(t)
        assert got[:live - 1].tobytes() == a[:live - 1].tobytes() and (t[live - 1:] == -2).all()
    store.close()


def test_the_scan_spans_many_blocks(small):
    """40 000 keys through import_entries into a store of capacity 65 536 (131 072 slots: 512 blocks of flags): every key comes back once."""
    from serenade_amd.serving import DeviceSessionStore
    gix, _, _ = small
    n = 40_000
    i = np.arange(n, dtype=np.uint64)
    hi, lo = i * np.uint64(0x9E3779B97F4A7C15), (i % np.uint64(1000)) * np.uint64(0xD6E8FEB86659FD93)          # lo repeats 40 times
    ep, ln = i + np.uint64(5), (i % np.uint64(4)).astype(np.uint32)
    it = np.zeros((n, 3), np.uint64)
    for j in range(3):
        it[:, j] = np.where(ln > j, i * np.uint64(10) + np.uint64(j + 1), np.uint64(0))
    store = DeviceSessionStore(gix, capacity=65_536, items_cap=3)
    store.import_entries((hi, lo), ep, ln, it)
    assert store.count(1) == (n, n)
    g_hi, g_lo, g_ep, g_ln, g_it = export_arrays(store, 1)
    assert len(g_hi) == n
    back = np.argsort(g_ep, kind="stable")                                                                  # the epochs are distinct: they name the entries
    assert np.array_equal(g_ep[back], ep) and np.array_equal(g_hi[back], hi) and np.array_equal(g_lo[back], lo)
    assert np.array_equal(g_ln[back], ln) and np.array_equal(g_it[back], it)
    assert store.stats["live_bound"] == n and store.stats["max_stored_len"] == 3
    store.close()


@pytest.mark.parametrize("roomy", [False, True])
def test_round_trip_into_a_store_of_another_shape(small, roomy):
    """Export, import into a fresh store of another capacity (just fits -- it then has to grow to be served --, or 16 times that) and a larger items_cap: the reads
    agree inside and past the idle limit, and a further stream served to both gives identical rows (the oracle's) and identical stores."""
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    rng = np.random.default_rng(21)
    a = DeviceSessionStore(gix, capacity=2048, items_cap=5, ttl_secs=TTL, idle_secs=IDLE)
    model = Model()
    now = serve_stream(gix, oix, [a], model, handler_stream(rng, ids, 300, 1200), 10_000, rng, [3, 5, 2, 1, 4], rows=False)
    exported = export_arrays(a, 1)
    n = len(exported[0])
    assert n == len(model.s) > 100
    b = DeviceSessionStore(gix, capacity=16 * n if roomy else n, items_cap=12, ttl_secs=TTL, idle_secs=IDLE, max_capacity=None if roomy else 64 * n)
    if roomy:   # tensors on the GPU
        import torch
        dev = torch.device("cuda", b.device)
        t = [torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)).to(dev) for x in exported]
        b.import_entries((t[0], t[1]), t[2], t[3], t[4])
    else:
        b.import_entries((exported[0], exported[1]), *exported[2:])
    assert as_dict(export_arrays(b, 1)) == as_dict(exported) == model.live(1)
    assert b.stats["live_bound"] == n and b.stats["max_stored_len"] >= max(len(s) for s, _ in model.s.values())
    for t_read in (now, now + IDLE // 2, now + IDLE + 1):
        for k in model.s:
            assert a.get_session_items(k, now=t_read) == b.get_session_items(k, now=t_read) == model.get(k, t_read), (hex(k), t_read)
    now = serve_stream(gix, oix, [a, b], model, handler_stream(rng, ids, 340, 700), now + 5, rng, [3, 5, 2, 4])
    assert as_dict(export_arrays(a, now)) == as_dict(export_arrays(b, now)) == model.live(now)
    if roomy:
        assert as_dict(export_arrays(a, 1)) == as_dict(export_arrays(b, 1)) == model.live(1)
    else:   # (a resize drops what a sweep drops: the grown store may have lost entries older than the TTL, which read as empty anyway)
        assert b.growth()["grows"] >= 1 and b.stats["capacity"] > n and b.stats["refused"] == 0
    a.close()
    b.close()


def test_merge_rule(small):
    from serenade_amd.serving import DeviceSessionStore
    gix, _, _ = small
    store = DeviceSessionStore(gix, capacity=64, items_cap=4)
    older, equal, newer, fresh, triple, tie = [(3 << 64) | j for j in range(6)]
    for k in (older, equal, newer):
        store.update_session_items(k, [1, 2], now=100)
    rows = [(triple, 5, [50]), (older, 99, [9]), (tie, 7, [70]), (equal, 100, [10, 11, 12]), (triple, 9, [51, 52]), (newer, 101, []), (tie, 7, [71]),
            (fresh, 1, [4, 4, 4, 4]), (triple, 7, [53]), (tie, 7, [72, 73])]
    store.import_entries(*raw_entries(rows, 4))
    want = {older: ((1, 2), 100), equal: ((10, 11, 12), 100), newer: ((), 101), fresh: ((4, 4, 4, 4), 1), triple: ((51, 52), 9), tie: ((72, 73), 7)}
    assert as_dict(export_arrays(store, 1)) == want
    st = store.stats
    assert st["live_bound"] <= 3 + len(rows) and st["max_stored_len"] >= 4
    assert store.count(1) == (6, 6)
    store.close()
    # 60 keys that share key_lo in a store of capacity 64 (probe chains), then 4 more: load 0.5
    store = DeviceSessionStore(gix, capacity=64, items_cap=4)
    d = {(((j * 0x9E3779B97F4A7C15) & U64) << 64) | 0x77: (tuple(range(j, j + j % 5)), 1000 + j) for j in range(60)}
    store.import_entries(*entries_of(d, 4))
    assert as_dict(export_arrays(store, 1)) == d
    more = {(j << 64) | j: ((j,), 2000 + j) for j in range(1, 5)}
    store.import_entries(*entries_of(more, 4))
    d.update(more)
    assert as_dict(export_arrays(store, 1)) == d and store.count(1) == (64, 64) and store.stats["slots"] == 128
    for k, (items, t) in d.items():
        assert store.get_session_items(k, now=t) == list(items)
    # the same keys again in calls of 4, in each call two older than what is stored and two newer (every entry counts as a new key: the store needs the room)
    keys = list(d)
    store.resize(128, now=1)
    for at in range(0, 64, 4):
        rows = [(k, d[k][1] + (1 if i % 2 else -1), [7, i]) for i, k in enumerate(keys[at:at + 4])]
        store.import_entries(*raw_entries(rows, 2))
        for i, (k, t, items) in enumerate(rows):
            if i % 2:
                d[k] = (tuple(items), t)
    assert as_dict(export_arrays(store, 1)) == d
    store.close()


def test_errors_leave_the_store_as_it_was(small):
    from serenade_amd import SerenadeError
    from serenade_amd.serving import DeviceSessionStore
    gix, _, _ = small
    store = DeviceSessionStore(gix, capacity=64, items_cap=4)
    d = {(5 << 64) | j: (tuple(range(1, 1 + j % 5)), 100 + j) for j in range(40)}
    store.import_entries(*entries_of(d, 4))
    before = export_bytes(store)

    def refused(code, fn, *args, **kw):
        with pytest.raises(SerenadeError) as e:
            fn(*args, **kw)
        assert e.value.code == code, e.value
        assert export_bytes(store) == before

    refused(-4, store.import_entries, *raw_entries([((6 << 64) | 1, 5, [1]), ((6 << 64) | 2, 5, [1, 2, 3, 4, 5]), ((6 << 64) | 3, 5, [])], 5))   # one len > items_cap
    refused(-2, store.import_entries, *raw_entries([((7 << 64) | j, 5, [j]) for j in range(30)], 4))                                             # 40 + 30 > 64
    refused(-2, store.resize, 39, now=1)                                                                                                          # below the live count
    refused(-4, store.resize, 64, items_cap=3, now=1)                                                                                             # the longest session is 4
    refused(-4, store.resize, 2**31, now=1)
    st = store.stats
    assert (st["capacity"], st["items_cap"], st["slots"], st["refused"]) == (64, 4, 128, 1) and store.growth()["resizes"] == 0
    assert as_dict(export_arrays(store, 1)) == d
    store.import_entries(*raw_entries([((7 << 64) | j, 5, [j]) for j in range(24)], 4))                                                           # 40 + 24 fits
    assert store.count(1) == (64, 64)
    store.close()


def test_resize(small):
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    store = DeviceSessionStore(gix, capacity=64, items_cap=4, ttl_secs=TTL, idle_secs=IDLE)
    model = Model()
    for j in range(50):
        t = 1000 if j < 30 else 5000
        model.s[(9 << 64) | j] = ([int(ids[(j + i) % 40]) for i in range(1 + j % 4)], t)
    store.import_entries(*entries_of(model.live(1), 4))
    store.resize(4096, now=1)
    st = store.stats
    assert (st["capacity"], st["slots"], st["items_cap"], st["slot_bytes"], st["live_bound"]) == (4096, 8192, 4, 128, 50)
    assert as_dict(export_arrays(store, 1)) == model.live(1)
    now = 5100                                                                   # the 30 entries of t = 1000 are older than the TTL
    store.resize(20, items_cap=13, now=now)                                      # exactly the live count; a slot of two lines
    st = store.stats
    assert (st["capacity"], st["slots"], st["items_cap"], st["slot_bytes"], st["live_bound"]) == (20, 64, 13, 256, 20)
    assert store.count(1) == (20, 20) and store.items_cap == 13
    assert as_dict(export_arrays(store, 1)) == model.live(now) and len(model.live(now)) == 20
    model.s = {k: (list(s), t) for k, (s, t) in model.live(now).items()}
    store.resize(256, items_cap=6, now=now)
    assert store.growth() == {"max_capacity": 0, "grows": 0, "resizes": 3}
    keys = list(model.s)[:15] + [(10 << 64) | j for j in range(15)]
    items = [int(ids[(3 * j) % 50]) for j in range(30)]
    for entry, t in (("host", now + 10), ("device", now + 20)):
        sessions = [model.serve(k, i, True, t, 6) for k, i in zip(keys, items[::-1] if entry == "device" else items)]
        check_rows(oix, sessions, *run(gix, store, keys, items[::-1] if entry == "device" else items, None, t, 6, entry), what=entry)
    assert as_dict(export_arrays(store, 1)) == model.live(1)
    store.close()


def test_growth(small):
    from serenade_amd import SerenadeError
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, ids = small
    store = DeviceSessionStore(gix, capacity=32, items_cap=4, max_capacity=256)
    model, now = Model(), 50_000
    assert store.growth() == {"max_capacity": 256, "grows": 0, "resizes": 0}
    for b in range(4):                                                           # 200 distinct keys, 50 at a time, each clicked twice
        keys = [(11 << 64) | (50 * b + j % 50) for j in range(100)]
        items = [int(ids[(j * 7 + b) % 60]) for j in range(100)]
        sessions = [model.serve(k, i, True, now + b, 3) for k, i in zip(keys, items)]
        check_rows(oix, sessions, *run(gix, store, keys, items, None, now + b, 3, "device" if b % 2 else "host"), what="batch %d" % b)
        assert as_dict(export_arrays(store, 1)) == model.live(1)
    st = store.stats
    assert st["capacity"] == 256 and st["slots"] == 512 and st["refused"] == 0 and len(model.s) == 200
    assert store.growth() == {"max_capacity": 256, "grows": 2, "resizes": 2}      # 32 -> 128 (live 0 + 100 requests), 128 -> 256
    before = export_bytes(store)
    keys = [(12 << 64) | j for j in range(100)]                                  # 200 live + 100 > 256
    with pytest.raises(SerenadeError) as e:
        run(gix, store, keys, [int(ids[0])] * 100, None, now + 9, 3, "device")
    assert e.value.code == -2 and store.stats["refused"] == 1 and store.stats["capacity"] == 256 and store.growth()["grows"] == 2
    assert export_bytes(store) == before
    store.close()
    fixed = DeviceSessionStore(gix, capacity=32, items_cap=4)                    # no max_capacity: refused at 32 as ever
    with pytest.raises(SerenadeError) as e:
        run(gix, fixed, [(11 << 64) | j for j in range(50)], [int(ids[0])] * 50, None, now, 3, "host")
    assert e.value.code == -2
    st = fixed.stats
    assert (st["capacity"], st["refused"], st["live_bound"]) == (32, 1, 0) and fixed.growth() == {"max_capacity": 0, "grows": 0, "resizes": 0}
    assert fixed.count(1) == (0, 0)
    fixed.close()


def test_save_and_load(small, tmp_path):
    """The order of an export is the slots', and which of two colliding keys gets the earlier slot is decided by the order of their claims, so a loaded store equals
    the saved one as a set of entries.  Its BYTES are the saved store's where the placement is reproduced: the store below was filled by one import of 48 entries -- one
    wave, whose lanes claim in one instruction stream -- and load imports the same 48 entries, sorted by key as they were, into tables of the same shape."""
    from serenade_amd import SerenadeError, capi
    from serenade_amd.serving import DeviceSessionStore, read_session_snapshot, write_session_snapshot
    gix, oix, ids = small
    path = str(tmp_path / "sessions.snap")
    d = {(((j * 0x9E3779B97F4A7C15) & U64) << 64) | (j % 5): (tuple(int(ids[(j + i) % 30]) for i in range(j % 7)), 700 + j) for j in range(48)}
    store = DeviceSessionStore(gix, capacity=100, items_cap=8, ttl_secs=2000, idle_secs=900)
    store.import_entries(*entries_of(d, 8))
    store.save(path, now=1)
    back = read_session_snapshot(path)
    assert (back["n"], back["longest_session"], back["items_stride"], back["capacity"], back["items_cap"], back["ttl_secs"], back["idle_secs"], back["saved_at_secs"]) == \
        (48, 6, 6, 100, 8, 2000, 900, 1)
    info = capi.DeviceSessionsFileInfo()
    capi.check(capi.lib().srn_device_sessions_file_info(path.encode(), C.byref(info)))
    assert (info.n, info.longest_session) == (48, 6)
    loaded = DeviceSessionStore.load(gix, path)
    st = loaded.stats
    assert (st["capacity"], st["items_cap"], st["ttl_secs"], st["idle_secs"], st["live_bound"]) == (100, 8, 2000, 900, 48) and loaded.items_cap == 8
    assert as_dict(export_arrays(loaded, 1)) == d
    assert export_bytes(loaded) == export_bytes(store)
    loaded.close()
    other = DeviceSessionStore.load(gix.info["device"], path, capacity=48, items_cap=6, ttl_secs=3000, idle_secs=1000)
    st = other.stats
    assert (st["capacity"], st["items_cap"], st["ttl_secs"], st["idle_secs"]) == (48, 6, 3000, 1000) and as_dict(export_arrays(other, 1)) == d
    other.close()
    for kw, code in ((dict(items_cap=5), -4), (dict(capacity=47), -2)):
        with pytest.raises(SerenadeError) as e:
            DeviceSessionStore.load(gix, path, **kw)
        assert e.value.code == code, kw
    # only the entries younger than the TTL at `now` are saved
    store.save(path, now=700 + 2000 + 10)
    assert read_session_snapshot(path)["n"] == 38
    # a save over a snapshot that a reader has open: the reader keeps the old file (the rename)
    old = open(path, "rb").read()
    with open(path, "rb") as reader:
        head = reader.read(100)
        store.save(path, now=1)
        assert head + reader.read() == old
    assert read_session_snapshot(path)["n"] == 48
    # a truncated file: SRN_EIO and no store
    cut = str(tmp_path / "cut.snap")
    open(cut, "wb").write(open(path, "rb").read()[:-9])
    with pytest.raises(SerenadeError) as e:
        DeviceSessionStore.load(gix, cut)
    assert e.value.code == -5
    h = C.c_void_p(1)
    assert capi.lib().srn_device_sessions_load(cut.encode(), gix.info["device"], 0, 0, 0, 0, C.byref(h)) == capi.SRN_EIO and not h.value
    store.close()
    # a file from another system's dump loads and serves
    model, now = Model(), 9000
    for j in range(70):
        model.s[(13 << 64) | j] = ([int(ids[(j + 2 * i) % 45]) for i in range(j % 4)], now - 13 * j)
    seed = str(tmp_path / "seed.snap")
    live = model.live(1)
    write_session_snapshot(seed, list(live), [t for _, t in live.values()], [list(s) for s, _ in live.values()], capacity=500, items_cap=5, ttl_secs=TTL, idle_secs=IDLE)
    seeded = DeviceSessionStore.load(gix, seed)
    assert as_dict(export_arrays(seeded, 1)) == live and seeded.stats["capacity"] == 500
    keys = list(model.s)[::2] + [(14 << 64) | j for j in range(10)]
    items = [int(ids[(5 * j) % 45]) for j in range(len(keys))]
    sessions = [model.serve(k, i, True, now + 400, 4) for k, i in zip(keys, items)]     # (the oldest of the stored sessions are idle by then)
    check_rows(oix, sessions, *run(gix, seeded, keys, items, None, now + 400, 4, "device"))
    assert as_dict(export_arrays(seeded, 1)) == model.live(1)
    # an empty store saves and loads
    empty = str(tmp_path / "empty.snap")
    e_store = DeviceSessionStore(gix, capacity=10, items_cap=2)
    e_store.save(empty, now=1)
    assert read_session_snapshot(empty)["n"] == 0
    e_loaded = DeviceSessionStore.load(gix, empty)
    assert e_loaded.count(1) == (0, 0) and e_loaded.stats["capacity"] == 10 and len(export_arrays(e_loaded, 1)[0]) == 0
    for s in (seeded, e_store, e_loaded):
        s.close()


def test_exports_are_serialised_with_batches(small):
    """One thread serves 40 batches, another exports all the while: every export is the model after a whole number of batches."""
    from serenade_amd.serving import DeviceSessionStore
    gix, _, ids = small
    rng = np.random.default_rng(31)
    model, states, batches = Model(), [], []
    states.append(model.live(1))
    for b in range(40):
        n = int(rng.integers(20, 200))
        keys = [(15 << 64) | int(rng.integers(0, 150)) for _ in range(n)]
        items = [int(ids[rng.integers(0, 40)]) for _ in range(n)]
        for k, i in zip(keys, items):
            model.serve(k, i, True, 30_000 + b, 3)
        batches.append((keys, items, 30_000 + b))
        states.append(model.live(1))
    assert all(a != b for a, b in zip(states, states[1:]))                       # every batch changes the store, if only its clock
    store = DeviceSessionStore(gix, capacity=8192, items_cap=4)
    seen, errs, done = [], [], threading.Event()

    def serve():
        try:
            for j, (keys, items, now) in enumerate(batches):
                run(gix, store, keys, items, None, now, 3, "device" if j % 2 else "host")
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))
        finally:
            done.set()

    def export():
        try:
            while True:
                last = done.is_set()
                seen.append(as_dict(export_arrays(store, 1, device=len(seen) % 2 == 1)))
                if last:
                    return
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=serve), threading.Thread(target=export)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    at = [next((i for i, s in enumerate(states) if s == got), None) for got in seen]
    assert None not in at, "an export is no state between two batches"
    assert at == sorted(at) and at[-1] == 40
    store.close()
