"""Trending items (srn_device_sessions_top_items, srn_index_set_fallback_trending): what can be checked without a GPU -- the symbols, the argument
checks that come before any device work, and serving.top_items_model, the rule in NumPy, against answers written down by hand."""
import ctypes as C

import numpy as np

from helpers import small_dataset
from serenade_amd import capi
from serenade_amd.serving import top_items_model

NEW_SYMBOLS = ["srn_device_sessions_top_items", "srn_index_set_fallback_trending"]
U64 = 2**64 - 1
A, B, D = 70, 50, 60


def test_new_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1] and fn.restype == capi.SYMBOLS[name][0], name
    from serenade_amd import VMISIndex
    from serenade_amd.serving import DeviceSessionStore
    assert callable(DeviceSessionStore.top_items) and callable(VMISIndex.set_fallback_trending)
    assert capi.TRENDING_POPULAR_TAIL == 1


def last_error():
    return capi.lib().srn_last_error()


def test_top_items_argument_checks():
    L = capi.lib()
    n, ids, cnt = C.c_size_t(), np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    assert L.srn_device_sessions_top_items(None, 1, 0, 1, 4, capi.ptr(ids), capi.ptr(cnt), C.byref(n)) == capi.SRN_EINVAL
    assert b"srn_device_sessions_top_items" in last_error()
    # the two checks below come before the store is read: any non-NULL pointer stands for one
    dummy = np.zeros(512, np.uint64)
    assert L.srn_device_sessions_top_items(capi.ptr(dummy), 1, 0, 1, 4, capi.ptr(ids), capi.ptr(cnt), None) == capi.SRN_EINVAL
    assert b"srn_device_sessions_top_items" in last_error()
    assert L.srn_device_sessions_top_items(capi.ptr(dummy), 1, 0, 1, 4, None, None, C.byref(n)) == capi.SRN_EINVAL
    assert b"srn_device_sessions_top_items" in last_error()
    assert not dummy.any()


def test_set_fallback_trending_argument_checks():
    import serenade_amd as sa
    L = capi.lib()
    off, items, ts, _ = small_dataset(3, n_sessions=200, n_items=40)
    ix = sa.VMISIndex.from_sessions(off, items, ts, 100, 12, 1.0, device=-1)
    got = C.c_size_t(77)
    dummy = np.zeros(512, np.uint64)        # stands for a store: every check below comes before the store is read
    store = capi.ptr(dummy)
    try:
        ix.set_fallback_popular(5)
        before = ix.fallback()
        for args, code in (((None, store, 1, 0, 1, 8, 1), capi.SRN_EINVAL),                       # NULL index
                           ((ix._h, None, 1, 0, 1, 8, 1), capi.SRN_EINVAL),                       # NULL store
                           ((ix._h, store, 1, 0, 1, 0, 1), capi.SRN_EINVAL),                      # n == 0
                           ((ix._h, store, 1, 0, 1, capi.MAX_FALLBACK + 1, 1), capi.SRN_ERANGE),
                           ((ix._h, store, 1, 0, 1, capi.MAX_FALLBACK, 1), capi.SRN_ENODEV),      # a host-only index
                           ((ix._h, store, 1, 0, 1, 8, 0), capi.SRN_ENODEV)):
            assert L.srn_index_set_fallback_trending(*args, C.byref(got)) == code, args[2:]
            assert b"srn_index_set_fallback_trending" in last_error(), args[2:]
        assert L.srn_index_set_fallback_trending(ix._h, store, 1, 0, 1, 8, 1, None) == capi.SRN_ENODEV
        assert np.array_equal(ix.fallback(), before) and not dummy.any()
    finally:
        ix.close()


def rows(*windows, stride=None):
    """windows -> (len, items[n, stride]); a window is (items, len) or a list (len = all of it)"""
    windows = [w if isinstance(w, tuple) else (w, len(w)) for w in windows]
    stride = stride or max(len(w) for w, _ in windows)
    items = np.zeros((len(windows), stride), np.uint64)
    for i, (w, _) in enumerate(windows):
        items[i, :len(w)] = np.array(w, np.uint64)
    return np.array([l for _, l in windows], np.uint32), items


def model(ln, items, epoch=None, n=None, now=1, ttl=1800, **kw):
    epoch = np.full(len(ln), 1000, np.uint64) if epoch is None else np.array(epoch, np.uint64)
    ids, counts = top_items_model(ln, items, epoch, n, now, ttl, **kw)
    assert ids.dtype == np.uint64 and counts.dtype == np.uint32
    return [(int(i), int(c)) for i, c in zip(ids, counts)]


def test_model_counts_an_id_once_per_window():
    assert model(*rows([A, B, A], [A], [B, B, B, D])) == [(B, 2), (A, 2), (D, 1)]


def test_model_counts_id_zero_and_the_largest_id():
    assert model(*rows([0, U64], [U64, 0, 5], [0])) == [(0, 3), (U64, 2), (5, 1)]


def test_model_ignores_what_lies_beyond_len():
    ln, items = rows(([A, B, D, D], 2), ([B, 9, 9], 1), ([7, 7], 0))
    assert model(ln, items) == [(B, 2), (A, 1)]


def test_model_ties_come_out_id_ascending():
    assert model(*rows([9, 3], [3, 9], [5], [5], [1])) == [(3, 2), (5, 2), (9, 2), (1, 1)]


def test_model_ttl_boundary():
    ln, items = rows([A], [B], [D])
    now, ttl = 10_000, 1800
    assert model(ln, items, [now - ttl, now - ttl - 1, now + 5], now=now, ttl=ttl) == [(D, 1), (A, 1)]     # (an epoch ahead of now is live, as for a sweep)


def test_model_since_boundary():
    ln, items = rows([A], [B], [D])
    assert model(ln, items, [500, 499, 501], since=500) == [(D, 1), (A, 1)]
    assert model(ln, items, [500, 499, 501], since=0) == [(B, 1), (D, 1), (A, 1)]


def test_model_now_one_keeps_everything():
    ln, items = rows([A], [B], [D])
    assert model(ln, items, [0, 1, 10**12], now=1, ttl=1) == [(B, 1), (D, 1), (A, 1)]


def test_model_min_count():
    ln, items = rows([A, B], [A], [A, D], [D])
    assert model(ln, items, min_count=0) == model(ln, items, min_count=1) == [(A, 3), (D, 2), (B, 1)]
    assert model(ln, items, min_count=2) == [(A, 3), (D, 2)]
    assert model(ln, items, min_count=4) == []


def test_model_n_above_the_ranked_ids_returns_them_all():
    ln, items = rows([A, B], [A])
    assert model(ln, items, n=1) == [(A, 2)]
    assert model(ln, items, n=0) == []
    assert model(ln, items, n=2) == model(ln, items, n=50) == model(ln, items, n=None) == [(A, 2), (B, 1)]


def test_model_of_nothing():
    assert model(np.zeros(0, np.uint32), np.zeros((0, 4), np.uint64)) == []
    assert model(*rows([A]), epoch=[5], now=5000, ttl=10) == []
