"""Device-resident session store and batched recommend (srn_device_sessions_*, srn_recommend_batch*, srn_session_keys): what can be checked without a GPU --
the symbols, the batched session key, and the argument checks that come before any device work."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from serenade_amd import capi

NEW_SYMBOLS = ["srn_device_sessions_create", "srn_device_sessions_free", "srn_device_sessions_get", "srn_device_sessions_update", "srn_device_sessions_sweep",
               "srn_device_sessions_stats", "srn_device_sessions_timing", "srn_device_sessions_last_ms", "srn_session_keys", "srn_recommend_batch_device",
               "srn_recommend_batch", "srn_debug_device_sessions_last_batch"]


def test_new_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1], name


def test_session_keys_are_the_md5_digests_big_endian():
    from serenade_amd.serving import session_key, session_keys
    strings = ["", "a", "abc", "message digest", "x" * 55, "y" * 56, "z" * 63, "z" * 64, "w" * 119, "q" * 120, "q" * 1000, "sessie-éü"]
    hi, lo = session_keys(strings)
    assert hi.dtype == np.uint64 and lo.dtype == np.uint64 and len(hi) == len(lo) == len(strings)
    for s, h, l in zip(strings, hi, lo):
        want = int.from_bytes(hashlib.md5(s.encode()).digest(), "big")
        assert (int(h) << 64) | int(l) == want, s
        assert session_key(s) == want, s
    hi, lo = session_keys([])
    assert len(hi) == 0 and len(lo) == 0
    hi, lo = session_keys(["", ""])                       # empty strings only: no bytes at all
    assert [(int(h) << 64) | int(l) for h, l in zip(hi, lo)] == [0xd41d8cd98f00b204e9800998ecf8427e] * 2


def _create(device, capacity, items_cap, ttl, idle, null_out=False):
    h = C.c_void_p()
    return capi.lib().srn_device_sessions_create(device, capacity, items_cap, ttl, idle, None if null_out else C.byref(h)), h


def test_create_without_a_device_is_enodev():
    rc, h = _create(-1, 100, 16, 0, 0)
    assert rc == capi.SRN_ENODEV and not h.value
    rc, h = _create(10_000, 100, 16, 0, 0)                # no box has that many GPUs
    assert rc == capi.SRN_ENODEV and not h.value


def test_create_refuses_bad_arguments_before_it_looks_for_a_device():
    assert _create(0, 0, 16, 0, 0)[0] == capi.SRN_EINVAL                  # capacity 0
    assert _create(0, 100, 0, 0, 0)[0] == capi.SRN_EINVAL                 # items_cap 0
    assert _create(0, 100, 256, 0, 0)[0] == capi.SRN_ERANGE               # items_cap above SRN_MAX_SESSION_LEN
    assert _create(0, 100, 16, 600, 1200)[0] == capi.SRN_EINVAL           # ttl < idle
    assert _create(0, 100, 16, 600, 0)[0] == capi.SRN_EINVAL              # ttl below the DEFAULT idle limit of 20 minutes
    assert _create(0, 100, 16, 0, 1801)[0] == capi.SRN_EINVAL             # the default ttl of 30 minutes below idle
    assert _create(0, 100, 16, 0, 0, null_out=True)[0] == capi.SRN_EINVAL
    assert b"srn_device_sessions_create" in capi.lib().srn_last_error()


def test_null_handles_are_refused():
    L = capi.lib()
    n = C.c_size_t()
    assert L.srn_device_sessions_get(None, 1, 2, 3, None, 0, C.byref(n)) == capi.SRN_EINVAL
    assert L.srn_device_sessions_update(None, 1, 2, 3, None, 0) == capi.SRN_EINVAL
    assert L.srn_device_sessions_sweep(None, 3, None) == capi.SRN_EINVAL
    assert L.srn_device_sessions_stats(None, None) == capi.SRN_EINVAL
    L.srn_device_sessions_free(None)
    one = np.ones(1, np.uint64)
    out = np.zeros(21, np.uint64)
    assert L.srn_recommend_batch(None, None, capi.ptr(one), capi.ptr(one), capi.ptr(one), None, 1, 0, 2, 10, 10, 21, 0, capi.ptr(out), capi.ptr(out), capi.ptr(out)) == capi.SRN_EINVAL


class _NeverCalled:
    """Stands in for an index: any use of it means the library was reached."""
    def __getattr__(self, name):
        raise AssertionError("recommend_batch touched the index (%s) before refusing its inputs" % name)


def test_recommend_batch_refuses_inputs_of_unequal_length_before_the_library_is_called():
    from serenade_amd.serving import recommend_batch
    hi, lo = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    with pytest.raises(ValueError):
        recommend_batch(_NeverCalled(), None, (hi, lo), np.zeros(3, np.uint64), k=10, m=10, how_many=5)
    with pytest.raises(ValueError):
        recommend_batch(_NeverCalled(), None, (hi, lo[:2]), np.zeros(4, np.uint64), k=10, m=10, how_many=5)
    with pytest.raises(ValueError):
        recommend_batch(_NeverCalled(), None, (hi, lo), np.zeros(4, np.uint64), np.zeros(5, np.uint8), k=10, m=10, how_many=5)
    with pytest.raises(ValueError):
        recommend_batch(_NeverCalled(), None, ["a", "b", "c"], np.zeros(4, np.uint64), k=10, m=10, how_many=5)
