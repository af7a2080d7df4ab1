"""The device-resident index build's C ABI without a GPU: srn_index_from_events_device, srn_index_host_state and srn_index_materialize are exported and bound
with the signatures capi.py states, the checks that come before any device work answer as documented, and an index built on the host reports a complete host copy."""
import ctypes as C

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi

NEW = ("srn_index_from_events_device", "srn_index_host_state", "srn_index_materialize")


def _rows(n=4):
    a = np.arange(1, n + 1, dtype=np.uint64)
    return a, a.copy(), np.arange(n, dtype=np.float64)


def _call(s, i, t, n, flags=0, m=10, idfw=1.0, max_len=0, device=0):
    h = C.c_void_p()
    rc = capi.lib().srn_index_from_events_device(None if s is None else s.ctypes.data, None if i is None else i.ctypes.data, None if t is None else t.ctypes.data,
                                                 n, flags, m, idfw, max_len, device, None, C.byref(h))
    assert rc == capi.SRN_OK or not h.value
    return rc


def test_new_symbols_exported_and_bound():
    L = capi.lib()
    for name in NEW:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    vp, sz = C.c_void_p, C.c_size_t
    assert capi.SYMBOLS["srn_index_from_events_device"] == (C.c_int, [vp, vp, vp, sz, C.c_uint, sz, C.c_double, sz, C.c_int, vp, C.POINTER(vp)])
    assert capi.SYMBOLS["srn_index_host_state"] == (C.c_int, [vp, C.POINTER(capi.IndexHostState)])
    assert capi.SYMBOLS["srn_index_materialize"] == (C.c_int, [vp])
    assert [n for n, _ in capi.IndexHostState._fields_][:4] == ["host_complete", "reserved", "build_bytes_on_device", "materialisations"]
    assert C.sizeof(capi.IndexHostState) == 2 * 4 + 2 * 8 + 7 * 8


def test_no_device_is_enodev():
    s, i, t = _rows()
    assert _call(s, i, t, 4, device=-1) == capi.SRN_ENODEV
    with pytest.raises(capi.SerenadeError) as e:
        sa.VMISIndex.from_events(s, i, t, 10, 1.0, device=-1, builder="resident")
    assert e.value.code == capi.SRN_ENODEV


def test_argument_checks():
    s, i, t = _rows()
    for args in ((None, i, t), (s, None, t), (s, i, None)):
        assert _call(*args, 4) == capi.SRN_EINVAL
    assert capi.lib().srn_index_from_events_device(s.ctypes.data, i.ctypes.data, t.ctypes.data, 4, 0, 10, 1.0, 0, 0, None, None) == capi.SRN_EINVAL
    assert _call(s, i, t, 4, flags=0x80) == capi.SRN_EINVAL
    assert b"unknown flags" in capi.lib().srn_last_error()
    assert _call(s, i, t, 0) == capi.SRN_EINVAL
    assert b"no training rows" in capi.lib().srn_last_error()
    assert _call(None, None, None, 0) == capi.SRN_EINVAL       # (as srn_sessions_from_events: no arrays are needed to say that there are no rows)
    assert _call(s, i, t, 4, m=0) == capi.SRN_EINVAL
    assert _call(s, i, t, 0xFFFFFFFF) == capi.SRN_ERANGE         # 2^32 - 1 rows: refused before a byte is read
    assert capi.lib().srn_index_host_state(None, C.byref(capi.IndexHostState())) == capi.SRN_EINVAL
    assert capi.lib().srn_index_materialize(None) == capi.SRN_EINVAL


def test_unknown_builder_raises():
    s, i, t = _rows()
    with pytest.raises(ValueError):
        sa.VMISIndex.from_events(s, i, t, 10, 1.0, device=-1, builder="bogus")
    from serenade_amd import prepare, serving
    import inspect
    assert inspect.signature(prepare.backtest).parameters["builder"].default == "gpu"
    assert inspect.signature(serving.refreshed_index).parameters["builder"].default == "gpu"
    assert inspect.signature(sa.VMISIndex.from_events).parameters["builder"].default == "gpu"


def test_host_built_index_has_a_complete_host_copy(tmp_path):
    off = np.array([0, 2, 5, 6], np.uint64)
    items = np.array([3, 9, 1, 3, 7, 9], np.uint64)
    ts = np.array([10, 30, 20], np.uint32)
    ix = sa.VMISIndex.from_sessions(off, items, ts, 5, 10, 1.0, device=-1)
    st = ix.host_state()
    assert st["host_complete"] is True and st["build_bytes_on_device"] == 0 and st["materialisations"] == 0
    assert all(st[k] == 0.0 for k in st if k.startswith("ms_"))
    ix.materialize()                                             # a no-op on such an index
    assert ix.host_state() == st
    ix.save(str(tmp_path / "a.idx"))
    assert ix.host_state() == st
    ix.close()
