"""Snapshot, restore, merge and grow of the device session store (srn_device_sessions_count / _export* / _import* / _resize / _set_max_capacity / _growth / _save /
_load / _file_info): what can be checked without a GPU -- the symbols, the argument checks that come before any device work, and the file form, which the library
verifies on the host and serving.write_session_snapshot / read_session_snapshot produce and read in pure NumPy."""
import ctypes as C
import struct

import numpy as np
import pytest

from serenade_amd import capi

NEW_SYMBOLS = ["srn_device_sessions_count", "srn_device_sessions_export_device", "srn_device_sessions_export", "srn_device_sessions_import_device",
               "srn_device_sessions_import", "srn_device_sessions_resize", "srn_device_sessions_set_max_capacity", "srn_device_sessions_growth",
               "srn_device_sessions_save", "srn_device_sessions_load", "srn_device_sessions_file_info"]
HEADER = 96


def test_new_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1], name
    from serenade_amd.serving import DeviceSessionStore
    for method in ("count", "export", "import_entries", "resize", "save", "load", "growth"):
        assert callable(getattr(DeviceSessionStore, method)), method


def test_null_arguments_are_einval(tmp_path):
    L = capi.lib()
    n, u, h = C.c_size_t(), C.c_uint64(), C.c_void_p()
    one, one32 = np.ones(1, np.uint64), np.ones(1, np.uint32)
    p = [capi.ptr(one)] * 3 + [capi.ptr(one32), capi.ptr(one)]
    assert L.srn_device_sessions_count(None, 1, C.byref(u), C.byref(u)) == capi.SRN_EINVAL
    assert L.srn_device_sessions_export(None, 1, 1, *p, 1, C.byref(n)) == capi.SRN_EINVAL
    assert L.srn_device_sessions_export_device(None, 1, 1, *p, 1, capi.ptr(one), None) == capi.SRN_EINVAL
    assert L.srn_device_sessions_import(None, *p, 1, 1) == capi.SRN_EINVAL
    assert L.srn_device_sessions_import_device(None, *p, 1, 1, None) == capi.SRN_EINVAL
    assert L.srn_device_sessions_resize(None, 10, 0, 1) == capi.SRN_EINVAL
    assert L.srn_device_sessions_set_max_capacity(None, 10) == capi.SRN_EINVAL
    assert L.srn_device_sessions_growth(None, C.byref(u), C.byref(u), C.byref(u)) == capi.SRN_EINVAL
    assert L.srn_device_sessions_save(None, str(tmp_path / "x").encode(), 1) == capi.SRN_EINVAL
    info = capi.DeviceSessionsFileInfo()
    assert L.srn_device_sessions_file_info(None, C.byref(info)) == capi.SRN_EINVAL                      # NULL path
    assert L.srn_device_sessions_file_info(str(tmp_path / "x").encode(), None) == capi.SRN_EINVAL       # NULL out
    assert L.srn_device_sessions_load(None, 0, 0, 0, 0, 0, C.byref(h)) == capi.SRN_EINVAL and not h.value
    assert L.srn_device_sessions_load(str(tmp_path / "x").encode(), 0, 0, 0, 0, 0, None) == capi.SRN_EINVAL
    assert b"srn_device_sessions_load" in L.srn_last_error()
    assert L.srn_device_sessions_file_info(str(tmp_path / "missing").encode(), C.byref(info)) == capi.SRN_EIO


def _entries():
    """sessions of length 0, 1 and 255 among others; keys that are equal in one half"""
    lens = [0, 1, 255, 3, 0, 16, 2]
    keys = [(7 << 64) | 1, (7 << 64) | 2, (8 << 64) | 2, (9 << 64) | 2, (2**64 - 1) << 64, 2**64 - 1, 0]
    epochs = [1000 + 10 * i for i in range(len(lens))]
    sessions = [[(i + 1) * 1000 + j for j in range(l)] for i, l in enumerate(lens)]
    return keys, epochs, sessions


def _info(path):
    info = capi.DeviceSessionsFileInfo()
    rc = capi.lib().srn_device_sessions_file_info(str(path).encode(), C.byref(info))
    return rc, {n: getattr(info, n) for n, _ in capi.DeviceSessionsFileInfo._fields_}


def test_a_written_snapshot_passes_file_info_and_reads_back(tmp_path):
    from serenade_amd.serving import read_session_snapshot, write_session_snapshot
    keys, epochs, sessions = _entries()
    path = tmp_path / "a.snap"
    write_session_snapshot(path, keys, epochs, sessions, capacity=100, items_cap=255, ttl_secs=1800, idle_secs=1200, saved_at=5000)
    rc, info = _info(path)
    assert rc == 0, capi.lib().srn_last_error()
    assert info == dict(version=1, n=7, longest_session=255, items_stride=255, capacity=100, items_cap=255, ttl_secs=1800, idle_secs=1200, saved_at_secs=5000,
                        payload_bytes=7 * 24 + 32 + 7 * 255 * 8)
    back = read_session_snapshot(path)
    assert [(int(h) << 64) | int(l) for h, l in zip(back["key_hi"], back["key_lo"])] == keys
    assert back["epoch"].tolist() == epochs and back["sessions"] == sessions and back["len"].tolist() == [len(s) for s in sessions]
    assert back["items"].shape == (7, 255) and all(not row[l:].any() for row, l in zip(back["items"], back["len"]))
    assert {k: back[k] for k in info if k != "version"} == {k: v for k, v in info.items() if k != "version"}
    # a wider stride than the longest session, keys given as (hi, lo)
    hi, lo = np.array([k >> 64 for k in keys], np.uint64), np.array([k & (2**64 - 1) for k in keys], np.uint64)
    write_session_snapshot(path, (hi[:2], lo[:2]), epochs[:2], sessions[:2], items_stride=4)
    rc, info = _info(path)
    assert rc == 0 and (info["n"], info["longest_session"], info["items_stride"], info["capacity"], info["items_cap"]) == (2, 1, 4, 2, 1)
    assert read_session_snapshot(path)["sessions"] == sessions[:2]


def test_an_empty_snapshot(tmp_path):
    from serenade_amd.serving import read_session_snapshot, write_session_snapshot
    path = tmp_path / "empty.snap"
    write_session_snapshot(path, [], [], [])
    assert path.stat().st_size == HEADER
    rc, info = _info(path)
    assert rc == 0 and (info["n"], info["longest_session"], info["payload_bytes"]) == (0, 0, 0)
    back = read_session_snapshot(path)
    assert back["sessions"] == [] and back["items"].shape == (0, 0)


def test_every_damage_is_eio(tmp_path):
    from serenade_amd.serving import read_session_snapshot, write_session_snapshot
    keys, epochs, sessions = _entries()
    good = tmp_path / "good.snap"
    write_session_snapshot(good, keys, epochs, sessions)
    raw = good.read_bytes()
    n, stride = 7, 255
    sections = [0, 8, HEADER, HEADER + 8 * n, HEADER + 16 * n, HEADER + 24 * n, HEADER + 24 * n + 32, len(raw) - 8 * stride]   # the boundaries of the header and every array
    damaged = {"cut at %d" % at: raw[:at] for at in sections}
    damaged["one byte short"] = raw[:-1]
    damaged["one byte long"] = raw + b"\0"
    for at in (HEADER + 3, HEADER + 24 * n + 5, HEADER + 24 * n + 32 + 17, len(raw) - 1):
        damaged["payload byte %d flipped" % at] = raw[:at] + bytes([raw[at] ^ 0x40]) + raw[at + 1:]
    for name, off in (("n", 16), ("items_stride", 32), ("payload_bytes", 80), ("header_bytes", 12)):
        damaged["header size %s flipped" % name] = raw[:off] + bytes([raw[off] ^ 1]) + raw[off + 1:]
    damaged["longest session flipped"] = raw[:24] + bytes([raw[24] ^ 1]) + raw[25:]
    damaged["wrong magic"] = b"SRNSESX\0" + raw[8:]
    damaged["wrong version"] = raw[:8] + struct.pack("<I", 2) + raw[12:]
    damaged["huge n"] = raw[:16] + struct.pack("<Q", 2**61) + raw[24:]                          # sizes that would overflow
    # a length above the file's stride, with the checksum made right again: only the length check can refuse it
    from serenade_amd.serving import _snap_checksum
    payload = bytearray(raw[HEADER:])
    payload[24 * n:24 * n + 4] = struct.pack("<I", 256)
    damaged["len above stride"] = raw[:88] + struct.pack("<Q", _snap_checksum(bytes(payload))) + bytes(payload)
    bad = tmp_path / "bad.snap"
    for name, data in damaged.items():
        bad.write_bytes(data)
        rc, _ = _info(bad)
        assert rc == capi.SRN_EIO, name
        with pytest.raises(ValueError):
            read_session_snapshot(bad)
    assert _info(good)[0] == 0
