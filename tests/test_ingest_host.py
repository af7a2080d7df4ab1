"""The GPU loader's C ABI without a GPU: the new symbols are exported and bound, and the checks that come before any device work
(srn_sessions_from_tsv_gpu, srn_sessions_from_events, srn_index_new_from_csv_gpu, srn_sessions_load_info) answer as documented."""
import ctypes as C

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi
from serenade_amd.ingest import TrainingSessions

NEW = ("srn_sessions_from_tsv_gpu", "srn_sessions_from_events", "srn_sessions_load_info", "srn_index_new_from_csv_gpu")


def _write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


def test_new_symbols_exported_and_bound():
    L = capi.lib()
    for name in NEW:
        assert name in capi.SYMBOLS
        assert getattr(L, name) is not None
    assert [n for n, _ in capi.LoadInfo._fields_] == ["lines", "rows", "skipped", "host_parsed", "ms_read", "ms_upload", "ms_parse", "ms_group", "ms_download"]
    assert C.sizeof(capi.LoadInfo) == 4 * 8 + 5 * 8


def test_no_device_is_enodev(tmp_path):
    path = _write(tmp_path / "t.tsv", "SessionId\tItemId\tTime\n1\t2\t3\n1\t3\t4\n2\t2\t5\n")
    h = C.c_void_p()
    L = capi.lib()
    assert L.srn_sessions_from_tsv_gpu(path.encode(), -1, C.byref(h)) == capi.SRN_ENODEV and not h.value
    a = np.arange(4, dtype=np.uint64)
    t = np.arange(4, dtype=np.float64)
    assert L.srn_sessions_from_events(a.ctypes.data, a.ctypes.data, t.ctypes.data, 4, 0, -1, None, C.byref(h)) == capi.SRN_ENODEV and not h.value
    assert L.srn_index_new_from_csv_gpu(path.encode(), 10, 1.0, 0, -1, C.byref(h)) == capi.SRN_ENODEV and not h.value
    with pytest.raises(capi.SerenadeError) as e:
        sa.VMISIndex.new_from_csv(path, 10, 1.0, device=-1, loader="gpu")
    assert e.value.code == capi.SRN_ENODEV
    with pytest.raises(capi.SerenadeError) as e:
        sa.VMISIndex.from_events(a, a, t, 10, 1.0, device=-1)
    assert e.value.code == capi.SRN_ENODEV


def test_missing_file_is_eio(tmp_path):
    h = C.c_void_p()
    missing = str(tmp_path / "no_such_file.tsv").encode()
    assert capi.lib().srn_sessions_from_tsv_gpu(missing, 0, C.byref(h)) == capi.SRN_EIO and not h.value
    assert b"no_such_file" in capi.lib().srn_last_error()
    assert capi.lib().srn_index_new_from_csv_gpu(missing, 10, 1.0, 0, 0, C.byref(h)) == capi.SRN_EIO and not h.value


def test_argument_checks(tmp_path):
    L = capi.lib()
    h = C.c_void_p()
    assert L.srn_sessions_from_tsv_gpu(None, 0, C.byref(h)) == capi.SRN_EINVAL
    a = np.arange(4, dtype=np.uint64)
    assert L.srn_sessions_from_events(a.ctypes.data, None, a.ctypes.data, 4, 0, 0, None, C.byref(h)) == capi.SRN_EINVAL
    assert L.srn_sessions_from_events(a.ctypes.data, a.ctypes.data, a.ctypes.data, 4, 0x80, 0, None, C.byref(h)) == capi.SRN_EINVAL
    # no rows: "no training rows", as the host loader says of an empty file
    assert L.srn_sessions_from_events(a.ctypes.data, a.ctypes.data, a.ctypes.data, 0, 0, 0, None, C.byref(h)) == capi.SRN_EINVAL
    assert b"no training rows" in L.srn_last_error()
    assert L.srn_sessions_load_info(None, C.byref(capi.LoadInfo())) == capi.SRN_EINVAL
    with pytest.raises(ValueError):
        sa.VMISIndex.new_from_csv(str(tmp_path / "x.tsv"), 10, 1.0, loader="cuda")
    with pytest.raises(ValueError):
        TrainingSessions.from_tsv(str(tmp_path / "x.tsv"), loader="cuda")


def test_host_loaded_handle_has_zero_load_info(tmp_path):
    path = _write(tmp_path / "t.tsv", "SessionId\tItemId\tTime\n1\t2\t3\n1\t3\t4\n2\t2\t5\n")
    s = TrainingSessions.from_tsv(path)
    info = s.load_info()
    assert set(info.values()) == {0}
    off, items, ts = s.arrays()
    assert off.tolist() == [0, 2] and items.tolist() == [2, 3] and ts.tolist() == [4]
    s.close()
