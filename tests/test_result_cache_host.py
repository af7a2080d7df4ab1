"""The device result cache (srn_index_result_cache_*): what can be checked without a GPU -- the symbols, the argument checks of the C entry points on an
index without a device, and the Python wrappers' own checks."""
import ctypes as C

import pytest

from helpers import small_dataset
from serenade_amd import capi

NEW_SYMBOLS = ["srn_index_result_cache_enable", "srn_index_result_cache_disable", "srn_index_result_cache_clear", "srn_index_result_cache_stats"]


def test_new_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1], name


def test_the_stats_record_has_the_header_layout():
    """rows, ways, bytes | max_len, k, m, how_many, flags, reserved | lookups, hits, inserts, evictions, bypassed_calls, clears: 3 + 3 + 6 eight-byte words."""
    assert C.sizeof(capi.ResultCacheStats) == 12 * 8
    assert capi.ResultCacheStats.lookups.offset == 48 and capi.ResultCacheStats.clears.offset == 88


def test_null_index_is_refused():
    L = capi.lib()
    st = capi.ResultCacheStats()
    assert L.srn_index_result_cache_enable(None, 1024, 2, 100, 500, 21, 0) == capi.SRN_EINVAL
    assert L.srn_index_result_cache_disable(None) == capi.SRN_EINVAL
    assert L.srn_index_result_cache_clear(None) == capi.SRN_EINVAL
    assert L.srn_index_result_cache_stats(None, C.byref(st)) == capi.SRN_EINVAL


@pytest.fixture(scope="module")
def host_index():
    import serenade_amd as sa
    off, items, ts, _ids = small_dataset(3, n_sessions=200, n_items=40)
    ix = sa.VMISIndex.from_sessions(off, items, ts, 50, 12, 1.0, device=-1)
    yield ix
    ix.close()


def test_argument_errors_without_a_device(host_index):
    L, h = capi.lib(), host_index._h
    enable = L.srn_index_result_cache_enable
    assert enable(h, 0, 2, 100, 500, 21, 0) == capi.SRN_EINVAL               # rows 0
    assert enable(h, 1024, 0, 100, 500, 21, 0) == capi.SRN_ERANGE            # max_len outside 1..8
    assert enable(h, 1024, 9, 100, 500, 21, 0) == capi.SRN_ERANGE
    assert enable(h, 1024, 2, 100, 500, 21, 4) == capi.SRN_EINVAL            # a flag that is not the business-logic one
    assert enable(h, 1024, 2, 100, 500, 21, 0) == capi.SRN_ENODEV            # all well, but the index has no device
    assert b"no device" in L.srn_last_error()
    st = capi.ResultCacheStats()
    assert L.srn_index_result_cache_stats(h, C.byref(st)) == capi.SRN_ENODEV
    assert L.srn_index_result_cache_stats(h, None) == capi.SRN_EINVAL
    assert L.srn_index_result_cache_clear(h) == capi.SRN_ENODEV
    assert L.srn_index_result_cache_disable(h) == capi.SRN_OK                # nothing to free


def test_the_wrappers_check_their_arguments_before_the_library(host_index):
    for bad in (dict(rows=0), dict(rows=-5), dict(max_len=0), dict(max_len=9), dict(k=0), dict(m=0), dict(how_many=0)):
        kw = dict(rows=1024, max_len=2, k=100, m=500, how_many=21)
        kw.update(bad)
        with pytest.raises(ValueError):
            host_index.enable_result_cache(**kw)
    with pytest.raises(capi.SerenadeError) as e:
        host_index.enable_result_cache(1024, 2, 100, 500, 21)
    assert e.value.code == capi.SRN_ENODEV
    with pytest.raises(capi.SerenadeError) as e:
        host_index.result_cache_stats()
    assert e.value.code == capi.SRN_ENODEV
    host_index.disable_result_cache()
