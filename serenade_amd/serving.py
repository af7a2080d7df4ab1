"""Dynamic batching in front of the predict kernel (srn_batcher_*): the serving-side caller of the hot path.

The reference answers each /v1/recommend call with its own vmisknn::predict on an actix worker thread
(src/endpoints/recommend_resource.rs:56-62).  `Batcher.predict` has that call's shape and may be called from many threads
at once; the library folds the waiting calls into one kernel launch.  No HTTP and no session store here."""
import collections
import ctypes as C
import os
import struct
import time
import warnings

import numpy as np

from . import capi
from .evaluation import BOOTSTRAP_THRESHOLDS, _M64, _interval, _mix64
from .vmisknn import ItemScore


class Batcher:
    def __init__(self, index, k, m, how_many, enable_business_logic=False, max_batch=4096, max_wait_us=200):
        self._index = index           # keep the index alive
        self.how_many = int(how_many)
        h = C.c_void_p()
        capi.check(capi.lib().srn_batcher_create(index._h, int(max_batch), int(max_wait_us), int(k), int(m), int(how_many),
                                                 int(bool(enable_business_logic)), C.byref(h)))
        self._h = h

    def predict(self, evolving_session):
        """-> [ItemScore(id, score), ...] best first, like serenade_amd.predict; blocks until the batch it joined is done."""
        ev = capi.as_u64(evolving_session)
        ids, sc, n = np.zeros(self.how_many, np.uint64), np.zeros(self.how_many, np.float64), C.c_size_t()
        capi.check(capi.lib().srn_batcher_predict(self._h, capi.ptr(ev), len(ev), capi.ptr(ids), capi.ptr(sc), C.byref(n)))
        return [ItemScore(int(i), float(s)) for i, s in zip(ids[:n.value], sc[:n.value])]

    @property
    def stats(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().srn_batcher_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(requests=a.value, batches=b.value, max_batch_seen=c.value)

    def close(self):
        if getattr(self, "_h", None):
            capi.lib().srn_batcher_free(self._h)
            self._h = None

    __del__ = close


def session_key(session_id):
    """u128 key of a session_id string, as the reference builds it (MD5 digest read big-endian, recommend_resource.rs:27-28)."""
    raw = session_id.encode() if isinstance(session_id, str) else bytes(session_id)
    hi, lo = C.c_uint64(), C.c_uint64()
    capi.check(capi.lib().srn_session_key(raw, len(raw), C.byref(hi), C.byref(lo)))
    return (hi.value << 64) | lo.value


class SessionStore:
    """In-memory stand-in for RocksDBSessionStore (src/sessions/mod.rs): same get / update calls, same idle and TTL clocks."""

    def __init__(self, ttl_secs=30 * 60, idle_secs=20 * 60):
        h = C.c_void_p()
        capi.check(capi.lib().srn_session_store_create(int(ttl_secs), int(idle_secs), C.byref(h)))
        self._h = h

    def get_session_items(self, key, now=0, cap=256):
        out, n = np.zeros(cap, np.uint64), C.c_size_t()
        capi.check(capi.lib().srn_session_store_get(self._h, key >> 64, key & (2**64 - 1), int(now), capi.ptr(out), cap, C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def update_session_items(self, key, items, now=0):
        it = capi.as_u64(items)
        capi.check(capi.lib().srn_session_store_update(self._h, key >> 64, key & (2**64 - 1), int(now), capi.ptr(it), len(it)))

    def sweep(self, now=0):
        n = C.c_uint64()
        capi.check(capi.lib().srn_session_store_sweep(self._h, int(now), C.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "_h", None):
            capi.lib().srn_session_store_free(self._h)
            self._h = None

    __del__ = close


def recommend(batcher, store, session_id, item_id, user_consent=True, max_items_in_session=2, now=0):
    """Body of the reference's /v1/recommend handler (recommend_resource.rs:20-65) -> recommended item ids, best first."""
    raw = session_id.encode() if isinstance(session_id, str) else bytes(session_id)
    ids, n = np.zeros(batcher.how_many, np.uint64), C.c_size_t()
    capi.check(capi.lib().srn_recommend(batcher._h, store._h if store is not None else None, raw, len(raw), int(item_id),
                                        int(bool(user_consent)), int(max_items_in_session), int(now), capi.ptr(ids), None, C.byref(n)))
    return [int(i) for i in ids[:n.value]]


# ---- the device-resident store and /v1/recommend for a whole batch (srn_device_sessions_*, srn_recommend_batch*) ----

def filter_rows(ids, scores, counts, excl, how_many):
    """NumPy mirror of the exclusion filter (srn_exclude.hip): rows [nq, W] with `counts` valid entries each -> rows [nq, how_many] without the ids of
    excl[q] (a list of nq sequences of ids), order kept, counts = min(kept, how_many).  A count of 0xFFFFFFFF is passed on; the entries beyond a count are 0.  It needs no GPU:
    what the device path computes from the wide rows, and what the tests compare it with."""
    ids, scores, counts = np.asarray(ids, np.uint64), np.asarray(scores, np.float64), np.asarray(counts, np.uint32)
    nq, wide = ids.shape
    if len(excl) != nq:
        raise ValueError("excl must hold one list per row")
    out_ids, out_sc, out_cnt = np.zeros((nq, how_many), np.uint64), np.zeros((nq, how_many)), np.zeros(nq, np.uint32)
    for q in range(nq):
        if counts[q] == 0xFFFFFFFF:
            out_cnt[q] = 0xFFFFFFFF
            continue
        n = min(int(counts[q]), wide)
        keep = np.flatnonzero(~np.isin(ids[q, :n], np.asarray(list(excl[q]), np.uint64)))[:how_many]
        out_ids[q, :len(keep)], out_sc[q, :len(keep)], out_cnt[q] = ids[q, keep], scores[q, keep], len(keep)
    return out_ids, out_sc, out_cnt


def passes_business_rules(cur, reco):
    """passes_business_rules of the reference (src/vmisknn/mod.rs:162-182) on attribute bytes (capi.ATTR_*; ATTR_NONE = no attributes)."""
    if reco == capi.ATTR_NONE or not reco & capi.ATTR_FOR_SALE:
        return False
    return not reco & capi.ATTR_ADULT or (cur != capi.ATTR_NONE and bool(cur & capi.ATTR_ADULT))


def fill_rows(ids, scores, counts, sessions, ranking, how_many, excl=None, exclude_session=False, attrs=None, business=False):
    """NumPy mirror of the fill kernel (srn_fill.hip): rows [nq, how_many] with `counts` valid entries each, as a call without SRN_FLAG_FILL returns them
    (filter_rows' output where the call excludes) -> the rows the same call returns with the flag.  A row of c < how_many entries keeps them and takes the first
    how_many - c ids f of `ranking`, in its order, that are none of the row's c ids, not sessions[q][-1], not in excl[q] (the query's list; for recommend_batch with
    exclude_seen the request's window), not in sessions[q] with exclude_session, and -- with business -- pass passes_business_rules(attr(sessions[q][-1]), attr(f)),
    where attrs maps an item id to its attribute byte and an id it does not hold has none (capi.ATTR_NONE: every item the index does not know).  Filled entries score
    -inf; counts = c + filled.  Rows with c >= how_many and counts of 0xFFFFFFFF are passed on unchanged.  It needs no GPU."""
    ids, scores, counts = np.array(ids, np.uint64), np.array(scores, np.float64), np.array(counts, np.uint32)
    nq = ids.shape[0]
    if ids.shape != (nq, how_many) or scores.shape != ids.shape or counts.shape != (nq,) or len(sessions) != nq or (excl is not None and len(excl) != nq):
        raise ValueError("rows must be [nq, how_many] with one count, one session and (if given) one list per row")
    ranking = [int(f) for f in ranking]
    attrs = attrs if attrs is not None else {}
    for q in range(nq):
        c = int(counts[q])
        if c >= how_many:   # (0xFFFFFFFF included)
            continue
        s = [int(x) for x in sessions[q]]
        gone = set(int(x) for x in ids[q, :c]) | {s[-1]} | (set(s) if exclude_session else set()) | (set(int(x) for x in excl[q]) if excl is not None else set())
        cur = attrs.get(s[-1], capi.ATTR_NONE)
        for f in ranking:
            if c == how_many:
                break
            if f in gone or (business and not passes_business_rules(cur, attrs.get(f, capi.ATTR_NONE))):
                continue
            ids[q, c], scores[q, c] = f, -np.inf
            c += 1
        counts[q] = c
    return ids, scores, counts


def top_items_model(len, items, epoch, n, now, ttl_secs, since=0, min_count=1):
    """NumPy statement of DeviceSessionStore.top_items (srn_trending.hip) over the arrays export() returns: len[e], items[e, stride], epoch[e] ->
    (ids uint64[], counts uint32[]), the first n entries of the ranking (n = None: all of it, so its length is `ranked`).  An entry is in range when a sweep at `now` keeps
    it -- not (now > epoch and now - epoch > ttl_secs), so now = 1 keeps everything -- and epoch >= since.  count(id) = the in-range entries whose window items[e, :len[e]]
    holds id at least once; positions from len[e] on are never read.  Count descending, id ascending; counts below min_count (0 is read as 1) are left out.  It needs
    no GPU and no library."""
    ln, ep = np.asarray(len, np.int64), np.asarray(epoch, np.uint64)
    items = np.asarray(items, np.uint64)
    items = items.reshape(ln.shape[0], items.size // max(ln.shape[0], 1))
    now, ttl, since = np.uint64(now), np.uint64(ttl_secs), np.uint64(since)
    old = (now > ep) & ((now - np.minimum(ep, now)) > ttl)
    in_range = ~old & (ep >= since)
    e, j = np.nonzero((np.arange(items.shape[1])[None, :] < ln[:, None]) & in_range[:, None])
    v = items[e, j]
    order = np.lexsort((v, e))                                   # by entry, then id: the repeats of an id inside a window become neighbours
    e, v = e[order], v[order]
    first = np.ones(v.shape[0], bool)
    first[1:] = (e[1:] != e[:-1]) | (v[1:] != v[:-1])
    ids, counts = np.unique(v[first], return_counts=True)        # (ids ascending)
    keep = counts >= max(int(min_count), 1)
    ids, counts = ids[keep], counts[keep]
    order = np.argsort(-counts, kind="stable")                   # count descending; stable: id ascending among equal counts
    ids, counts = ids[order].astype(np.uint64), counts[order].astype(np.uint32)
    return (ids, counts) if n is None else (ids[:int(n)], counts[:int(n)])


def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


def _device_of(device_or_index):
    """A GPU's number, or the one an index is on."""
    return device_or_index if isinstance(device_or_index, int) else device_or_index.info["device"]


def _export_entries(cap, stride_of, device, export_device, export_host):
    """The grow-and-retry loop of DeviceSessionStore.export and SessionHarvest.export -> (hi, lo), epoch, len, items[n, stride].  cap: the caller's count of the
    entries, which may have grown by the time of the export: the call then reports the number and is made again with that much room.  stride_of(): the width of items,
    read before every try.  device: a GPU's number for tensors there, written on the current stream (export_device(cap, [hi, lo, ep, ln, it] as pointers, stride,
    d_n, stream) -> rc), or None for NumPy arrays (export_host(cap, the five as pointers, stride, byref(n)) -> rc)."""
    while True:
        stride = stride_of()
        if device is not None:
            import torch
            dev = torch.device("cuda", device)
            hi, lo, ep = (torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(3))
            ln = torch.zeros(cap, dtype=torch.int32, device=dev)
            it = torch.zeros((cap, stride), dtype=torch.int64, device=dev)
            d_n = torch.zeros(1, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(device).cuda_stream
            capi.check(export_device(cap, [C.c_void_p(t.data_ptr()) for t in (hi, lo, ep, ln, it)], stride, C.c_void_p(d_n.data_ptr()), C.c_void_p(stream)))
            n = int(d_n.item())
        else:
            hi, lo, ep = (np.zeros(cap, np.uint64) for _ in range(3))
            ln, it, got = np.zeros(cap, np.uint32), np.zeros((cap, stride), np.uint64), C.c_size_t()
            rc = export_host(cap, [capi.ptr(a) for a in (hi, lo, ep, ln, it)], stride, C.byref(got))
            n = got.value
            if rc != 0 and not (rc == capi.SRN_ERANGE and n > cap):
                capi.check(rc)
        if n <= cap:                                    # (more: entries arrived between the count and the export)
            return (hi[:n], lo[:n]), ep[:n], ln[:n], it[:n]
        cap = n


def session_keys(session_ids):
    """session_key for a list of strings in one call -> (hi, lo) as uint64 arrays."""
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in session_ids]
    n = len(raw)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    flat = np.frombuffer(b"".join(raw) or b"\0", np.uint8)
    hi, lo = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    capi.check(capi.lib().srn_session_keys(capi.ptr(flat), capi.ptr(off), n, capi.ptr(hi), capi.ptr(lo)))
    return hi, lo


SessionCount = collections.namedtuple("SessionCount", "occupied live")

# ---- the snapshot file of a device store, in pure NumPy: no GPU, no library ----
_SNAP_MAGIC, _SNAP_VERSION, _SNAP_HEADER = b"SRNSESS\0", 1, 96
_SNAP_FIELDS = ("n", "longest_session", "items_stride", "capacity", "items_cap", "ttl_secs", "idle_secs", "saved_at_secs", "payload_bytes", "checksum")


def _snap_checksum(payload):
    """sum of mix64(w[i] + (i + 1) * 0x9E3779B97F4A7C15) over the payload's little-endian 8-byte words, mod 2^64"""
    w = np.frombuffer(payload, "<u8").astype(np.uint64)
    x = w + np.arange(1, w.size + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xff51afd7ed558ccd)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xc4ceb9fe1a85ec53)
    x ^= x >> np.uint64(33)
    return int(x.sum(dtype=np.uint64))


def write_session_snapshot(path, keys, epochs, sessions, capacity=None, items_cap=None, ttl_secs=30 * 60, idle_secs=20 * 60, saved_at=0, items_stride=None):
    """Writes sessions[i] (a list of item ids) under keys[i] with epochs[i] as a snapshot file DeviceSessionStore.load reads: how a store is seeded from another
    system's dump.  keys: (hi, lo) uint64 arrays, or a list of 128-bit integers.  capacity / items_cap: what load uses by default (None: n / the longest session)."""
    if isinstance(keys, tuple):
        hi, lo = (capi.as_u64(a) for a in keys)
    else:
        hi = np.array([int(k) >> 64 for k in keys], np.uint64)
        lo = np.array([int(k) & (2**64 - 1) for k in keys], np.uint64)
    n = len(sessions)
    ep = capi.as_u64(epochs)
    if not (len(hi) == len(lo) == len(ep) == n):
        raise ValueError("keys, epochs and sessions differ in length")
    ln = np.array([len(s) for s in sessions], np.uint32)
    longest = int(ln.max()) if n else 0
    stride = longest if items_stride is None else int(items_stride)
    if stride < longest or stride > capi.MAX_SESSION_LEN:
        raise ValueError("items_stride must hold the longest session and be at most %d" % capi.MAX_SESSION_LEN)
    items = np.zeros((n, stride), np.uint64)
    for i, s in enumerate(sessions):
        items[i, :len(s)] = np.asarray(s, np.uint64)
    payload = b"".join([hi.astype("<u8").tobytes(), lo.astype("<u8").tobytes(), ep.astype("<u8").tobytes(), ln.astype("<u4").tobytes(), b"\0" * (-4 * n % 8),
                        items.astype("<u8").tobytes()])
    values = (n, longest, stride, max(int(capacity or n), 1), max(int(items_cap or longest), 1), int(ttl_secs), int(idle_secs), int(saved_at), len(payload),
              _snap_checksum(payload))
    header = _SNAP_MAGIC + struct.pack("<II10Q", _SNAP_VERSION, _SNAP_HEADER, *values)
    tmp = "%s.tmp.%d" % (os.fspath(path), os.getpid())
    with open(tmp, "wb") as f:
        f.write(header + payload)
    os.replace(tmp, path)


def read_session_snapshot(path):
    """-> {"key_hi", "key_lo", "epoch", "len", "items"[n, items_stride], "sessions" (lists), and the header's fields}; ValueError for anything but a whole snapshot."""
    raw = open(path, "rb").read()
    if len(raw) < _SNAP_HEADER or raw[:8] != _SNAP_MAGIC:
        raise ValueError("%s: not a session snapshot" % path)
    version, header_bytes, *values = struct.unpack("<II10Q", raw[8:_SNAP_HEADER])
    h = dict(zip(_SNAP_FIELDS, values))
    n, stride = h["n"], h["items_stride"]
    o_len = 24 * n
    o_items = o_len + (4 * n + 7) // 8 * 8
    if version != _SNAP_VERSION or header_bytes != _SNAP_HEADER or n > 2**30 or stride > capi.MAX_SESSION_LEN or h["longest_session"] > stride or \
            h["payload_bytes"] != o_items + 8 * n * stride or len(raw) != _SNAP_HEADER + h["payload_bytes"]:
        raise ValueError("%s: unknown version, or sizes that do not add up" % path)
    payload = raw[_SNAP_HEADER:]
    if _snap_checksum(payload) != h["checksum"]:
        raise ValueError("%s: checksum mismatch" % path)
    out = dict(h, version=version)
    out["key_hi"], out["key_lo"], out["epoch"] = (np.frombuffer(payload, "<u8", n, 8 * n * j).astype(np.uint64) for j in range(3))
    out["len"] = np.frombuffer(payload, "<u4", n, o_len).astype(np.uint32)
    out["items"] = np.frombuffer(payload, "<u8", n * stride, o_items).astype(np.uint64).reshape(n, stride)
    if n and int(out["len"].max()) != h["longest_session"]:
        raise ValueError("%s: a session's length disagrees with the header" % path)
    out["sessions"] = [[int(x) for x in row[:l]] for row, l in zip(out["items"], out["len"])]
    return out


class DeviceSessionStore:
    """The evolving sessions in the GPU's memory: what recommend_batch reads and updates.  get / update / sweep mirror SessionStore's, for one key, from the host."""

    def __init__(self, device_or_index, capacity, items_cap=16, ttl_secs=30 * 60, idle_secs=20 * 60, max_capacity=None, history=0):
        """max_capacity: opt-in growth -- a batch the capacity rule would refuse doubles the capacity (up to max_capacity) instead; None = a fixed capacity.
        history: the store keeps a window of the last `history` clicks (<= items_cap) and recommend_batch predicts on its last max_items_in_session items; 0 = the
        store keeps max_items_in_session items, as the reference does."""
        device = _device_of(device_or_index)
        h = C.c_void_p()
        capi.check(capi.lib().srn_device_sessions_create(int(device), int(capacity), int(items_cap), int(ttl_secs), int(idle_secs), C.byref(h)))
        self._h, self.device, self.items_cap = h, int(device), int(items_cap)
        if max_capacity:
            capi.check(capi.lib().srn_device_sessions_set_max_capacity(self._h, int(max_capacity)))
        if history:
            self.set_history(history)

    def set_history(self, history):
        """srn_device_sessions_set_history: the window of clicks the store keeps (0 = max_items_in_session).  A runtime setting, not saved: set it again after load."""
        capi.check(capi.lib().srn_device_sessions_set_history(self._h, int(history)))

    @property
    def history(self):
        h = C.c_size_t()
        capi.check(capi.lib().srn_device_sessions_history(self._h, C.byref(h)))
        return h.value

    @classmethod
    def load(cls, device_or_index, path, capacity=None, items_cap=None, ttl_secs=None, idle_secs=None):
        """A store on that GPU with the sessions of a snapshot file (save, write_session_snapshot); None = the value the file records."""
        device = _device_of(device_or_index)
        h = C.c_void_p()
        capi.check(capi.lib().srn_device_sessions_load(os.fsencode(path), int(device), int(capacity or 0), int(items_cap or 0), int(ttl_secs or 0), int(idle_secs or 0),
                                                       C.byref(h)))
        self = cls.__new__(cls)
        self._h, self.device = h, int(device)
        self.items_cap = int(self.stats["items_cap"])
        return self

    def save(self, path, now=0):
        """The live sessions at `now` as a snapshot file, written under a temporary name and renamed."""
        capi.check(capi.lib().srn_device_sessions_save(self._h, os.fsencode(path), int(now)))

    def count(self, now=0):
        """-> SessionCount(occupied, live): exact, from the device; live = what a sweep at `now` would keep."""
        o, l = C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().srn_device_sessions_count(self._h, int(now), C.byref(o), C.byref(l)))
        return SessionCount(o.value, l.value)

    def export(self, now=0, device=False):
        """The live sessions at `now`, in slot order -> (hi, lo), epoch, len, items[n, items_cap] (zero beyond len).  NumPy arrays, or with device=True tensors
        on the store's GPU, written on the current stream."""
        L = capi.lib()
        return _export_entries(self.count(now).live, lambda: int(self.stats["items_cap"]), self.device if device else None,
                               lambda cap, arrays, *rest: L.srn_device_sessions_export_device(self._h, int(now), cap, *arrays, *rest),
                               lambda cap, arrays, *rest: L.srn_device_sessions_export(self._h, int(now), cap, *arrays, *rest))

    def import_entries(self, keys, epoch, len, items):
        """Inserts the entries (keys[i], epoch[i], items[i, :len[i]]) under the merge rule: the larger epoch wins, a tie replaces.  NumPy arrays, or tensors on the
        store's GPU (read on the current stream)."""
        hi, lo = keys
        arrs = [hi, lo, epoch, len, items]
        n = arrs[0].shape[0]
        if any(a.shape[0] != n for a in arrs) or items.ndim != 2:
            raise ValueError("keys, epoch and len must have one entry per row of items[n, stride]")
        stride = int(items.shape[1])
        on_gpu = [_is_torch(a) and a.device.type == "cuda" for a in arrs]
        if any(on_gpu):
            import torch
            if not all(on_gpu) or any(a.device.index != self.device for a in arrs):
                raise ValueError("keys, epoch, len and items must all be tensors on the store's GPU (device %d), or none of them" % self.device)
            if any(a.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) for a in (hi, lo, epoch, items)) or \
                    len.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise TypeError("keys, epoch and items must be 64-bit and len 32-bit integer tensors")
            t = [a.contiguous() for a in arrs]
            stream = torch.cuda.current_stream(self.device).cuda_stream
            capi.check(capi.lib().srn_device_sessions_import_device(self._h, *(C.c_void_p(a.data_ptr()) for a in t), stride, n, C.c_void_p(stream)))
            return
        hi, lo, epoch, items = (capi.as_u64(a.numpy() if _is_torch(a) else a) for a in (hi, lo, epoch, items))
        ln = capi.as_u32(len.numpy() if _is_torch(len) else len)
        capi.check(capi.lib().srn_device_sessions_import(self._h, capi.ptr(hi), capi.ptr(lo), capi.ptr(epoch), capi.ptr(ln), capi.ptr(items), stride, n))

    def top_items(self, n, since=0, min_count=1, now=0):
        """srn_device_sessions_top_items: the n items the live sessions at `now` hold most often -> (ids uint64[], counts uint32[]), count descending, id ascending (fewer
        than n when fewer are ranked).  count = the sessions, with an epoch >= since, whose stored window holds the item at least once; counts below min_count are left
        out.  Counted and ranked on the GPU (top_items_model is the rule in NumPy); blocks, and changes nothing in the store."""
        ids, counts, ranked = np.zeros(int(n), np.uint64), np.zeros(int(n), np.uint32), C.c_size_t()
        capi.check(capi.lib().srn_device_sessions_top_items(self._h, int(now), int(since), int(min_count), int(n), capi.ptr(ids) if n else None,
                                                            capi.ptr(counts) if n else None, C.byref(ranked)))
        got = min(int(n), ranked.value)
        return ids[:got], counts[:got]

    def resize(self, capacity, items_cap=None, now=0):
        """Rebuilds the live sessions at `now` into tables of another capacity and / or items_cap; on an error the store is unchanged."""
        capi.check(capi.lib().srn_device_sessions_resize(self._h, int(capacity), int(items_cap or 0), int(now)))
        self.items_cap = int(self.stats["items_cap"])

    def growth(self):
        """-> {"max_capacity", "grows" (automatic resizes), "resizes" (all resizes)}."""
        m, g, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().srn_device_sessions_growth(self._h, C.byref(m), C.byref(g), C.byref(r)))
        return {"max_capacity": m.value, "grows": g.value, "resizes": r.value}

    def get_session_items(self, key, now=0, cap=256):
        out, n = np.zeros(max(cap, 1), np.uint64), C.c_size_t()
        capi.check(capi.lib().srn_device_sessions_get(self._h, key >> 64, key & (2**64 - 1), int(now), capi.ptr(out), cap, C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def update_session_items(self, key, items, now=0):
        it = capi.as_u64(items)
        capi.check(capi.lib().srn_device_sessions_update(self._h, key >> 64, key & (2**64 - 1), int(now), capi.ptr(it), len(it)))

    def sweep(self, now=0):
        n = C.c_uint64()
        capi.check(capi.lib().srn_device_sessions_sweep(self._h, int(now), C.byref(n)))
        return n.value

    def set_harvest(self, harvest):
        """srn_device_sessions_set_harvest: from now on `harvest` (a SessionHarvest) receives every session the store forgets -- a visitor's return after idle inside
        recommend_batch, and what a sweep, the capacity rule's automatic sweep, a resize or growth drops.  None detaches.  Nothing else about the store changes."""
        capi.check(capi.lib().srn_device_sessions_set_harvest(self._h, None if harvest is None else harvest._h))
        old = getattr(self, "_harvest", None)
        if old is not None:
            old._store = None
        self._harvest = harvest
        if harvest is not None:
            harvest._store = self

    @property
    def stats(self):
        st = capi.DeviceSessionsStats()
        capi.check(capi.lib().srn_device_sessions_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in capi.DeviceSessionsStats._fields_}

    def timing(self, enable=True):
        capi.check(capi.lib().srn_device_sessions_timing(self._h, int(bool(enable))))

    def last_ms(self):
        """-> (ms of the store's kernels, ms of predict's launches) of the most recent batch; needs timing(True)."""
        a, b = C.c_double(), C.c_double()
        capi.check(capi.lib().srn_device_sessions_last_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def last_batch_sessions(self):
        """(test aid) the sessions the most recent recommend_batch emitted -> (items_flat u64, q_off u32)."""
        n = C.c_size_t()
        capi.check(capi.lib().srn_debug_device_sessions_last_batch(self._h, None, None, C.byref(n), None, None, 0, None))
        q_off = np.zeros(n.value + 1, np.uint32)
        if n.value == 0:
            return np.zeros(0, np.uint64), q_off
        capi.check(capi.lib().srn_debug_device_sessions_last_batch(self._h, None, None, None, None, None, 0, capi.ptr(q_off)))
        items = np.zeros(max(int(q_off[-1]), 1), np.uint64)
        capi.check(capi.lib().srn_debug_device_sessions_last_batch(self._h, None, None, None, None, capi.ptr(items), len(items), capi.ptr(q_off)))
        return items[:int(q_off[-1])], q_off

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:
            capi.lib().srn_device_sessions_free(self._h)                # (detaches an attached harvest)
            self._h = None
            if getattr(self, "_harvest", None) is not None:
                self._harvest._store, self._harvest = None, None

    __del__ = close


# ---- session harvest: finished sessions logged on the GPU, and an index rebuilt from them (srn_harvest_*) ----
_HARVEST_COUNTERS = ("stored", "stored_items", "lost", "skipped_short", "from_return", "from_rebuild")


def harvest_model(state, keys, items, consent, now, *, limit=2, idle_secs=20 * 60, ttl_secs=30 * 60, min_len=1, capacity=None, sweep=False, times=None):
    """Pure-Python statement of the session harvest (srn_harvest.hip): a dictionary replay of the /v1/recommend handler's rule that keeps what the
    store forgets.  It needs no GPU and no library.
    state: dict, updated in place: 128-bit key -> (items list, epoch) for every stored session, and under the key "log" the harvest itself (created on first use).
    One call is one recommend_batch call at `now` -- keys = (hi, lo), items, consent (None: all consent); keys = None: no requests -- followed, with sweep=True, by
    store.sweep(now).  Requests j = 0..n-1 in order:
      no consent                              nothing is read or stored
      the key is stored with len > 0 and now > epoch and now - epoch > idle_secs (strict): the stored session is OFFERED (a return after idle) and the visitor
                                              starts from an empty session
      then the click is appended unless it repeats the session's last item; beyond `limit` items (max_items_in_session, or the store's history window H) the
      oldest one is dropped; the session is stored with epoch = now
    A sweep offers and removes every stored session with now > epoch and now - epoch > ttl_secs.  An offered session of fewer than min_len items is counted in
    skipped_short; one offered when the log holds `capacity` sessions (None: unbounded) in lost; every other one is stored with its epoch and items as they were.
    The log is appended in the device's order: the returns of one call in ascending key order (not request order), so the result does not depend on how the requests
    of one time step are cut into calls.  A sweep's sessions are appended in ascending key order here and in slot order on the device: which of them a FULL log loses
    is the one thing this model does not predict.
    times (rule T): request j's own clock -- the call is len(times) one-request calls, call j at times[j], in request order; `now` is then read by the
    sweep alone.  A visitor's stored session is tested against the time of the visitor's first consenting request; every later request of the visitor tests the time
    its predecessor stored, so sessions also end INSIDE the call.  The call's appends: the stored sessions the visitors' first requests found idle, in ascending key
    order as above, then the sessions ended inside the call in ascending key order and, within a key, request order.
    -> (sessions, counters): the stored sessions as (key, epoch, [items]) tuples in canonical order -- (epoch, key) ascending -- and the words of SessionHarvest.stats()
    plus "append_order": the same tuples in the order they were stored."""
    log = state.setdefault("log", {"sessions": [], "lost": 0, "skipped_short": 0, "from_return": 0, "from_rebuild": 0})
    now, min_len = int(now), max(int(min_len), 1)

    def offer(found, which, ordered=False):
        for key, (its, epoch) in (found if ordered else sorted(found, key=lambda e: e[0])):
            log[which] += 1
            if len(its) < min_len:
                log["skipped_short"] += 1
            elif capacity is not None and len(log["sessions"]) >= capacity:
                log["lost"] += 1
            else:
                log["sessions"].append((key, int(epoch), [int(x) for x in its]))

    if keys is not None:
        hi, lo = (np.asarray(a, np.uint64) for a in keys)
        items = np.asarray(items, np.uint64)
        if not (len(hi) == len(lo) == len(items)) or (consent is not None and len(consent) != len(items)):
            raise ValueError("keys, items and consent differ in length")
        if times is not None and len(times) != len(items):
            raise ValueError("times must have one entry per request")
        returned, inside, seen, sweep_now = [], [], set(), now
        for j in range(len(items)):
            if consent is not None and not consent[j]:
                continue
            key = (int(hi[j]) << 64) | int(lo[j])
            if times is not None:
                now = int(times[j])
            cur, epoch = state.get(key, ([], 0))
            if cur and now > epoch and now - epoch > idle_secs:
                (inside if key in seen else returned).append((key, (cur, epoch)))
                cur = []
            seen.add(key)
            item = int(items[j])
            if not cur or cur[-1] != item:
                cur = cur + [item]
                if len(cur) > limit:
                    cur = cur[1:]
            state[key] = (cur, now)
        offer(returned, "from_return")
        offer(sorted(inside, key=lambda e: e[0]), "from_return", ordered=True)   # (a stable sort: request order within a key)
        now = sweep_now
    if sweep:
        old = [(k, v) for k, v in state.items() if k != "log" and now > v[1] and now - v[1] > ttl_secs]
        for k, _ in old:
            del state[k]
        offer(old, "from_rebuild")
    counters = {n: log[n] for n in ("lost", "skipped_short", "from_return", "from_rebuild")}
    counters["stored"], counters["stored_items"] = len(log["sessions"]), sum(len(s[2]) for s in log["sessions"])
    counters["append_order"] = list(log["sessions"])
    return sorted(log["sessions"], key=lambda s: (s[1], s[0])), counters


class SessionHarvest:
    """A session harvest in the GPU's memory (srn_harvest_*): the log that receives every session a DeviceSessionStore forgets, once, on the serving call's stream.
    store.set_harvest(hv) attaches it; export / events read it in canonical order -- (epoch, key) ascending -- without consuming it."""

    def __init__(self, index_or_device, capacity, items_cap=16, min_len=1):
        device = _device_of(index_or_device)
        h = C.c_void_p()
        capi.check(capi.lib().srn_harvest_create(int(device), int(capacity), int(items_cap), int(min_len), C.byref(h)))
        self._h, self.device, self.capacity, self.items_cap = h, int(device), int(capacity), int(items_cap)
        self._store = None

    def stats(self):
        """srn_harvest_stats_t as a dict (blocks): capacity, items_cap, min_len; stored, stored_items -- what the log holds now; lost, skipped_short, from_return,
        from_rebuild, cleared.  from_return + from_rebuild = stored + cleared + lost + skipped_short."""
        st = capi.HarvestStats()
        capi.check(capi.lib().srn_harvest_stats(self._h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in capi.HarvestStats._fields_}

    def export(self, device=False):
        """The stored sessions in canonical order -> (hi, lo), epoch, len, items[n, items_cap] (zero beyond len), like DeviceSessionStore.export.  NumPy arrays, or with
        device=True tensors on the harvest's GPU, written on the current stream."""
        L = capi.lib()
        return _export_entries(int(self.stats()["stored"]), lambda: self.items_cap, self.device if device else None,
                               lambda cap, arrays, *rest: L.srn_harvest_export_device(self._h, cap, *arrays, *rest),
                               lambda cap, arrays, *rest: L.srn_harvest_export(self._h, cap, *arrays, *rest))

    def events(self, id_base=0):
        """srn_harvest_events_device: the stored sessions as training rows -> (session_ids, item_ids, times), int64 tensors on the harvest's GPU, written on the current
        stream: canonical session i has the id id_base + i and one row per item, in session order, each with time = the session's epoch.  What
        VMISIndex.from_events / TrainingSessions.from_events read."""
        import torch
        dev = torch.device("cuda", self.device)
        cap = int(self.stats()["stored_items"])
        while True:
            sid, item, t = (torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(3))
            d_rows = torch.zeros(1, dtype=torch.int64, device=dev)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            capi.check(capi.lib().srn_harvest_events_device(self._h, int(id_base), cap, *(C.c_void_p(x.data_ptr()) for x in (sid, item, t, d_rows)), C.c_void_p(stream)))
            n = int(d_rows.item())
            if n <= cap:
                return sid[:n], item[:n], t[:n]
            cap = n

    def clear(self):
        """Empties the log (stored sessions move to stats()["cleared"]); lost, skipped_short, from_return and from_rebuild keep running."""
        capi.check(capi.lib().srn_harvest_clear(self._h))

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:
            store = getattr(self, "_store", None)
            if store is not None and getattr(store, "_h", None):
                store.set_harvest(None)
            capi.lib().srn_harvest_free(self._h)
            self._h = None

    __del__ = close


def refreshed_index(base_session_ids, base_item_ids, base_times, harvest, m_most_recent_sessions, idf_weighting, max_session_len=0, device=0, builder="gpu"):
    """The index of the base training events with the harvested sessions appended: exactly VMISIndex.from_events over the base arrays (NumPy, CPU tensors or tensors
    on `device`, as from_events takes them) followed by harvest.events(id_base=max(base_session_ids) + 1), concatenated on the device.  That is what
    VMISIndex.new_from_csv gives for the training file with those rows appended -- read_from_file's quirk included: the file's final row closes its session and the
    last session is dropped, so the most recent harvested session does not enter the index.  The harvested times are epochs in seconds; base times above them are the
    caller's business.  The harvest is not consumed.  builder: as VMISIndex.from_events takes it ("resident": the build never leaves the device)."""
    import torch
    from .vmisknn import VMISIndex
    if builder not in ("gpu", "resident"):
        raise ValueError("builder must be 'gpu' or 'resident'")
    if harvest.device != int(device):
        raise ValueError("the harvest is on device %d, not %d" % (harvest.device, int(device)))
    dev = torch.device("cuda", int(device))

    def on_device(a, floating_ok=False):
        if not _is_torch(a):
            a = np.ascontiguousarray(a)
            if np.issubdtype(a.dtype, np.floating):
                a = a.astype(np.float64, copy=False)
            else:
                a = a.astype(np.uint64, copy=False).view(np.int64) if a.dtype == np.uint64 else a.astype(np.int64, copy=False)
            a = torch.from_numpy(a)
        if a.dtype == getattr(torch, "uint64", None):
            a = a.view(torch.int64)
        if a.is_floating_point():
            if not floating_ok:
                raise TypeError("session and item ids must be integers")
            a = a.to(torch.float64)
        elif a.dtype != torch.int64:
            a = a.to(torch.int64)
        return a.to(dev).contiguous()

    sid, item, t = on_device(base_session_ids), on_device(base_item_ids), on_device(base_times, True)
    if not (sid.numel() == item.numel() == t.numel()):
        raise ValueError("the base arrays differ in length")
    id_base = int(sid.max().item()) + 1 if sid.numel() else 0           # (session ids below 2^63, as everywhere a tensor carries them)
    h_sid, h_item, h_t = harvest.events(id_base)
    return VMISIndex.from_events(torch.cat([sid, h_sid]), torch.cat([item, h_item]), torch.cat([t, h_t.to(t.dtype)]), m_most_recent_sessions, idf_weighting,
                                 max_session_len=max_session_len, device=int(device), builder=builder)


# ---- click feedback: served rows scored against the visitor's next click (srn_feedback_*) ----
_FEEDBACK_COUNTERS = ("requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored")


def feedback_model(state, keys, items, consent, ids, counts, scores, now, idle_secs=20 * 60, row_cap=None, times=None):
    """NumPy statement of ClickFeedback.observe (srn_feedback.hip): what the device computes, bit for bit.  It needs no GPU and no library.
    state: dict, 128-bit key -> (ids uint64[c], n_model, epoch); updated in place.  keys = (hi, lo); consent / scores may be None (all consent / every entry a model
    entry).  ids[n, how_many], counts[n]: the rows just served to the requests.  Requests j = 0..n-1 in order, with one `now`:
      no consent                 rank NONE; nothing is read or stored
      no entry for the key       rank NONE (first_seen);   an entry with now > epoch and now - epoch > idle_secs: rank NONE (idle_expired)
      otherwise observed:        r = 1-based position of items[j] among the entry's ids (0: absent), FILLED or-ed in when r > n_model
      then, with consent:        the entry becomes (ids[j, :c], finite scores among those c, now), c = counts[j] (0xFFFFFFFF -> 0; above how_many -> how_many)
    times (rule T): request j's own clock, read in `now`'s place -- the call is n one-request calls, call j at times[j], in request order.
    -> (ranks uint32[n], counters): the words of ClickFeedback.stats() plus "hist_model" / "hist_filled", hits by rank ([0] unused): uint64[row_cap + 1], or with
    row_cap = None as long as the widest row of the call and the state needs."""
    hi, lo = (np.asarray(a, np.uint64) for a in keys)
    items, counts = np.asarray(items, np.uint64), np.asarray(counts, np.uint32)
    n = len(items)
    ids = np.asarray(ids, np.uint64).reshape(n, -1) if n else np.zeros((0, 1), np.uint64)
    how_many = ids.shape[1]
    sc = None if scores is None else np.asarray(scores, np.float64).reshape(n, how_many)
    if not (len(hi) == len(lo) == len(counts) == n) or (consent is not None and len(consent) != n):
        raise ValueError("keys, items, consent, ids and counts differ in length")
    ranks = np.full(n, capi.FEEDBACK_NONE, np.uint32)
    ctr = {name: 0 for name in _FEEDBACK_COUNTERS}
    widest = max([how_many] + [len(e[0]) for e in state.values()]) if row_cap is None else int(row_cap)   # (a stored row may be wider than this call's)
    ctr["hist_model"], ctr["hist_filled"] = np.zeros(widest + 1, np.uint64), np.zeros(widest + 1, np.uint64)
    now = int(now)
    if times is not None and len(times) != n:
        raise ValueError("times must have one entry per request")
    for j in range(n):
        if times is not None:
            now = int(times[j])
        ctr["requests"] += 1
        if consent is not None and not consent[j]:
            ctr["no_consent"] += 1
            continue
        key = (int(hi[j]) << 64) | int(lo[j])
        entry = state.get(key)
        if entry is None:
            ctr["first_seen"] += 1
        elif now > entry[2] and now - entry[2] > idle_secs:
            ctr["idle_expired"] += 1
        else:
            row, n_model, _ = entry
            at = np.flatnonzero(row == items[j])
            r = int(at[0]) + 1 if len(at) else 0
            filled = r > n_model
            ranks[j] = r | (capi.FEEDBACK_FILLED if filled else 0)
            ctr["observed"] += 1
            if r:
                ctr["hits_filled" if filled else "hits_model"] += 1
                ctr["hist_filled" if filled else "hist_model"][r] += 1
        c = 0 if counts[j] == capi.FEEDBACK_NONE else min(int(counts[j]), how_many)
        state[key] = (ids[j, :c].copy(), c if sc is None else int(np.isfinite(sc[j, :c]).sum()), now)
        ctr["stored"] += 1
    return ranks, ctr


def feedback_metrics(hist_model, hist_filled, observed):
    """hit_rate = hits / observed and mrr = sum over r of hist[r] / r / observed, added in ascending r -- each for all hits and split into model and filled entries
    (0.0 where nothing was observed): the reference's HitRate and Mrr at the row's length (metrics/hitrate.rs, mrr.rs) over the observed requests."""
    hm, hf = (np.asarray(h, np.uint64) for h in (hist_model, hist_filled))
    out = {}
    for name, h in (("", hm + hf), ("_model", hm), ("_filled", hf)):
        hits, mrr = 0, 0.0
        for r in range(1, len(h)):
            hits += int(h[r])
            mrr += int(h[r]) / r
        out["hit_rate" + name] = hits / observed if observed else 0.0
        out["mrr" + name] = mrr / observed if observed else 0.0
    return out


# ---- the visitor-clustered bootstrap of the log's counters (srn_feedback_bootstrap_*) ----
_FEEDBACK_METRICS = tuple(m + part for part in ("", "_model", "_filled") for m in ("hit_rate", "mrr"))
_FOLD = 0x9E3779B97F4A7C15


def feedback_fold(keys):
    """fold(key) = mix64(key_hi ^ 0x9E3779B97F4A7C15) ^ key_lo on uint64 arrays: the word the weight rule takes in the session index's place."""
    hi, lo = (np.asarray(a, np.uint64) for a in keys)
    return _mix64(hi ^ np.uint64(_FOLD)) ^ lo


def feedback_bootstrap_weights(seed, B, keys, first_replicate=0):
    """w(seed, b, key) for b = first_replicate .. first_replicate + B - 1 and keys = (hi, lo) -> uint8[B, n]: evaluation.bootstrap_weights' rule -- a Poisson(1)
    count cut at 12 -- at fold(key).  Row b depends on (seed, b, key) alone."""
    with np.errstate(over="ignore"):
        b = np.uint64(int(first_replicate)) + np.arange(int(B), dtype=np.uint64)
        rkey = _mix64(np.uint64(int(seed) & _M64) + (b + np.uint64(1)) * np.uint64(_FOLD))
        s = feedback_fold(keys).reshape(-1)
        u = _mix64(rkey[:, None] ^ (s * np.uint64(0xD1B54A32D192ED03) + np.uint64(1))[None, :]) >> np.uint64(32)
    return np.searchsorted(np.array(BOOTSTRAP_THRESHOLDS, np.uint64), u, side="right").astype(np.uint8)


def feedback_bootstrap_model(ranks, keys, B, seed, row_cap):
    """NumPy statement of the log's replicate words (srn_feedback.hip fb_boot), exactly: ranks uint32[n] as feedback_model (or ClickFeedback.observe) gives them for the
    requests of keys = (hi, lo), of any number of calls, concatenated.  Replicate b adds w(seed, b, key) per observed request -- rank not FEEDBACK_NONE -- to
    observed[b], and for a rank r > 0 to hist_model[b, r], or hist_filled[b, r] where the rank carries FEEDBACK_FILLED.
    -> {"observed": uint64[B], "hist_model": uint64[B, row_cap + 1], "hist_filled": the same}; integer sums, so the order of the requests does not matter."""
    ranks = np.asarray(ranks, np.uint32).reshape(-1)
    hi, lo = (np.asarray(a, np.uint64).reshape(-1) for a in keys)
    if not (len(hi) == len(lo) == len(ranks)):
        raise ValueError("one key per rank")
    B, R = int(B), int(row_cap) + 1
    out = {"observed": np.zeros(B, np.uint64), "hist_model": np.zeros((B, R), np.uint64), "hist_filled": np.zeros((B, R), np.uint64)}
    obs = np.flatnonzero(ranks != capi.FEEDBACK_NONE)
    if not len(obs):
        return out
    r = (ranks[obs] & np.uint32(0x7FFFFFFF)).astype(np.int64)
    if r.max() >= R:
        raise ValueError("a rank above row_cap")
    column = np.where((ranks[obs] & np.uint32(capi.FEEDBACK_FILLED)) != 0, R, 0) + r      # the request's column in [hist_model | hist_filled]; r = 0: a miss
    order = np.argsort(column, kind="stable")
    cols, starts = np.unique(column[order], return_index=True)
    visitors, of = np.unique(np.stack([hi[obs], lo[obs]], axis=1), axis=0, return_inverse=True)   # (a visitor's weight once)
    of = of.reshape(-1)[order]
    hist = np.zeros((B, 2 * R), np.uint64)
    step = max(1, (1 << 22) // len(visitors))
    for b0 in range(0, B, step):
        w = feedback_bootstrap_weights(seed, min(step, B - b0), (visitors[:, 0], visitors[:, 1]), first_replicate=b0)[:, of]
        sums = np.add.reduceat(w, starts, axis=1, dtype=np.uint64)
        out["observed"][b0:b0 + len(w)] = sums.sum(axis=1, dtype=np.uint64)
        hist[b0:b0 + len(w), cols] = sums
    hist[:, 0] = hist[:, R] = 0                                                          # (the misses count in observed alone)
    out["hist_model"], out["hist_filled"] = hist[:, :R].copy(), hist[:, R:].copy()
    return out


def _feedback_replicate_metrics(hist_model, hist_filled, observed):
    """feedback_metrics of every replicate's weighted histograms over its observed_w, replicate by replicate the same bits -> ({metric: float64[B]}, bool[B]: the
    replicate's observed_w is not 0; its values are 0 where it is)."""
    hm, hf = (np.asarray(h, np.uint64) for h in (hist_model, hist_filled))
    w = np.asarray(observed, np.uint64).astype(np.float64)
    ok = w > 0
    out = {}
    for name, h in (("", hm + hf), ("_model", hm), ("_filled", hf)):
        hits, mrr = np.zeros(len(w)), np.zeros(len(w))
        for r in range(1, h.shape[1]):   # ascending r, as feedback_metrics adds
            hits = hits + h[:, r].astype(np.float64)
            mrr = mrr + h[:, r].astype(np.float64) / r
        out["hit_rate" + name] = np.divide(hits, w, out=np.zeros_like(w), where=ok)
        out["mrr" + name] = np.divide(mrr, w, out=np.zeros_like(w), where=ok)
    return out, ok


def feedback_replicate_values(stats, metric="mrr"):
    """A bootstrapped ClickFeedback.stats()'s metric per replicate -> (float64[B], bool[B]: the replicate observed something)."""
    boot = stats.get("bootstrap")
    if boot is None:
        raise ValueError("the stats carry no bootstrap: enable it on the log (ClickFeedback(..., bootstrap=B))")
    if metric not in _FEEDBACK_METRICS:
        raise ValueError("metric must be one of %s" % ", ".join(_FEEDBACK_METRICS))
    values, ok = _feedback_replicate_metrics(boot["hist_model"], boot["hist_filled"], boot["observed"])
    return values[metric], ok


def feedback_compare(stats_a, stats_b, metric="mrr"):
    """Bootstrap comparison of two logs' stats() -- evaluation.compare's counterpart for the online numbers -> {"delta": a - b of the point estimates, "ci": the
    percentile interval of the replicate-by-replicate differences (at stats_a's level), "p_better": the share of replicates where a is above b, "replicates": how
    many entered (those with something observed on both sides), "paired"}.  ValueError when seed or B differ.
    A visitor's weight depends on (seed, replicate, key) alone.  The same log replayed under two configurations therefore resamples the same visitors on both sides
    -- whether a request is observed does not depend on the rows served, so the two `observed` arrays are equal, and exactly then "paired" is true: the interval is
    the paired one, the visitors' noise cancels in every difference.  Two logs with disjoint visitors (live traffic split over two logs) have independent
    replicates: the same differences then form an ordinary unpaired two-sample interval, "paired" is false, and nothing cancels."""
    ba, bb = stats_a.get("bootstrap"), stats_b.get("bootstrap")
    if ba is None or bb is None:
        raise ValueError("feedback_compare needs the stats of logs with the bootstrap enabled")
    if ba["seed"] != bb["seed"] or ba["replicates"] != bb["replicates"]:
        raise ValueError("the stats do not share their replicates: seed and replicates must be equal")
    va, oka = feedback_replicate_values(stats_a, metric)
    vb, okb = feedback_replicate_values(stats_b, metric)
    d = (va - vb)[oka & okb]
    return {"delta": float(stats_a[metric]) - float(stats_b[metric]), "ci": _interval(d, float(ba["ci"])),
            "p_better": float(np.count_nonzero(d > 0)) / len(d) if len(d) else 0.0, "replicates": int(len(d)),
            "paired": bool(np.array_equal(ba["observed"], bb["observed"]))}


def _with_feedback_bootstrap(out, boot, ci):
    """stats() of a log with the bootstrap enabled: the arrays under "bootstrap" and a percentile interval per metric over the replicates that observed something."""
    values, ok = _feedback_replicate_metrics(boot["hist_model"], boot["hist_filled"], boot["observed"])
    out["bootstrap"] = dict(boot, ci=ci, empty_replicates=int(np.count_nonzero(~ok)))
    for name in _FEEDBACK_METRICS:
        out[name + "_ci"] = _interval(values[name][ok], ci)
    return out


def _on_gpu(a):
    return _is_torch(a) and a.device.type == "cuda"


def _as_numpy(a):
    return a.numpy() if _is_torch(a) else a


def _visitor_batch(keys, item_ids, consent, times, device, who):
    """The request side of a visitor batch, marshalled for the C ABI -> (hi, lo, items, consent, times, on_gpu, p, tail): uint64 / uint8 NumPy arrays (CPU tensors
    count as arrays) or the contiguous tensors, consent and times None where not given; whether they are on the GPU; the function that makes a pointer argument of
    an array (None stays None); and what follows a call's last argument: the current stream for tensors, nothing for arrays.
    device(): the GPU the tensors must be on, asked only when there are tensors; who: that GPU's owner in a message."""
    hi, lo = keys
    n = len(item_ids)
    given = [a for a in (hi, lo, item_ids, consent) if a is not None]
    if any(len(a) != n for a in given):
        raise ValueError("keys, item_ids and consent differ in length")
    if times is not None and len(times) != n:
        raise ValueError("times must have one entry per request")
    if any(_on_gpu(a) for a in given):
        import torch
        dev = device()
        if not all(_on_gpu(a) and a.device.index == dev for a in given):
            raise ValueError("keys, item_ids and consent must all be tensors on %s's GPU (device %d), or none of them" % (who, dev))
        if times is not None and not (_on_gpu(times) and times.device.index == dev):
            raise ValueError("times must be a tensor on %s's GPU (device %d), like keys" % (who, dev))
        i64 = (torch.int64, getattr(torch, "uint64", torch.int64))
        if any(a.dtype not in i64 for a in (hi, lo, item_ids)):
            raise TypeError("keys and item_ids must be 64-bit integer tensors")
        if consent is not None and consent.dtype not in (torch.uint8, torch.bool):
            raise TypeError("consent must be a uint8 or bool tensor")
        if times is not None and times.dtype not in i64:
            raise TypeError("times must be a 64-bit integer tensor")
        arrs = [None if a is None else a.contiguous() for a in (hi, lo, item_ids, consent, times)]
        return (*arrs, True, lambda a: None if a is None else C.c_void_p(a.data_ptr()), [C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)])
    if times is not None and _on_gpu(times):
        raise ValueError("times must be where keys are: an array or CPU tensor here")
    hi, lo, it, tm = (None if a is None else capi.as_u64(_as_numpy(a)) for a in (hi, lo, item_ids, times))
    con = None if consent is None else np.ascontiguousarray(_as_numpy(consent)).astype(np.uint8)
    return hi, lo, it, con, tm, False, capi.ptr, []


def _call_visitor_batch(entry, handles, batch, now, rest):
    """The C ABI's form of `entry` for this batch: <entry>[_device][_at](*handles, key_hi, key_lo, item_ids, consent[, times], n, now, *rest[, stream]) -- _device for
    tensors, _at and the times behind consent for a timed batch."""
    hi, lo, it, con, tm, on_gpu, p, tail = batch
    name = entry + ("_device" if on_gpu else "") + ("_at" if tm is not None else "")
    args = list(handles) + [p(hi), p(lo), p(it), p(con)] + ([p(tm)] if tm is not None else []) + [len(it), int(now)] + list(rest) + tail
    capi.check(getattr(capi.lib(), name)(*args))


class ClickFeedback:
    """A click feedback log in the GPU's memory (srn_feedback_*): the last row served to every visitor, scored against the visitor's next click.  An object of its own
    beside the session store; recommend_batch(..., feedback=fb) feeds it.  bootstrap=B (and seed): enable_bootstrap(B, seed) at creation."""

    def __init__(self, index_or_device, capacity, row_cap=21, ttl_secs=30 * 60, idle_secs=20 * 60, bootstrap=0, seed=0):
        device = _device_of(index_or_device)
        h = C.c_void_p()
        capi.check(capi.lib().srn_feedback_create(int(device), int(capacity), int(row_cap), int(ttl_secs), int(idle_secs), C.byref(h)))
        self._h, self.device, self.row_cap = h, int(device), int(row_cap)
        self.last_ranks = None
        self.last_error = None          # recommend_batch(..., feedback=self): the error of a call the log refused (its rows were served all the same)
        if bootstrap:
            try:
                self.enable_bootstrap(bootstrap, seed)
            except Exception:
                self.close()
                raise

    def enable_bootstrap(self, replicates, seed=0):
        """From the next call on the log keeps, per replicate b < replicates, the observed count and both histograms with every request weighted by
        w(seed, b, visitor) (srn_feedback_bootstrap_enable): one more kernel per observe call; stats() then carries intervals.  The words start at 0."""
        capi.check(capi.lib().srn_feedback_bootstrap_enable(self._h, int(replicates), int(seed) & _M64))

    def disable_bootstrap(self):
        capi.check(capi.lib().srn_feedback_bootstrap_disable(self._h))

    def bootstrap(self):
        """-> {"replicates", "seed", "observed": uint64[B], "hist_model": uint64[B, row_cap + 1], "hist_filled": the same} (column 0 unused), or None when the
        bootstrap is off.  Blocks."""
        B, seed = C.c_uint32(), C.c_uint64()
        capi.check(capi.lib().srn_feedback_bootstrap_info(self._h, C.byref(B), C.byref(seed)))
        if not B.value:
            return None
        obs = np.zeros(B.value, np.uint64)
        hm, hf = np.zeros((B.value, self.row_cap + 1), np.uint64), np.zeros((B.value, self.row_cap + 1), np.uint64)
        capi.check(capi.lib().srn_feedback_bootstrap_read(self._h, capi.ptr(obs), capi.ptr(hm), capi.ptr(hf), B.value, self.row_cap + 1))
        return {"replicates": B.value, "seed": seed.value, "observed": obs, "hist_model": hm, "hist_filled": hf}

    def observe(self, keys, item_ids, consent, ids, counts, scores=None, now=0, times=None):
        """Requests (keys[i], item_ids[i], consent[i]) and the rows just served to them (ids[n, how_many], counts[n], scores or None) -> ranks[n]: the 1-based rank of
        the clicked item in the visitor's PREVIOUS row (0: a miss; capi.FEEDBACK_FILLED or-ed in for a filled entry) or capi.FEEDBACK_NONE where there is no previous
        row to score; then the rows are remembered.  NumPy arrays in, a uint32 array out; tensors on the log's GPU are read in place on the current stream, without
        synchronising, and the ranks are an int32 tensor there (the same bits).  The result is also left in self.last_ranks.
        times (srn_feedback_observe*_at): request i's own clock in seconds, an array or tensor like the others -- the call gives what one call per
        request at times[i] gives, in request order, and `now` is only the capacity rule's sweep clock: pass a lower bound of times (0 reads the wall clock, which is
        wrong for a recorded log)."""
        n = len(item_ids)
        rows_in = [a for a in (ids, counts, scores) if a is not None]
        if ids.ndim != 2 or len(ids) != n or len(counts) != n or (scores is not None and tuple(scores.shape) != tuple(ids.shape)):
            raise ValueError("keys, item_ids, consent and counts must have one entry per row of ids[n, how_many] (and scores its shape)")
        batch = _visitor_batch(keys, item_ids, consent, times, lambda: self.device, "the log")
        on_gpu, p = batch[5], batch[6]
        if on_gpu != all(_on_gpu(a) and a.device.index == self.device for a in rows_in) or on_gpu != any(_on_gpu(a) for a in rows_in):
            raise ValueError("keys, item_ids, consent, ids, counts and scores must all be tensors on the log's GPU (device %d), or none of them" % self.device)
        if on_gpu:
            import torch
            if ids.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)) or counts.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or \
                    (scores is not None and scores.dtype != torch.float64):
                raise TypeError("ids must be a 64-bit integer, counts a 32-bit integer and scores a float64 tensor")
            rows, cnt, sc = (None if a is None else a.contiguous() for a in (ids, counts, scores))
            ranks = torch.zeros(n, dtype=torch.int32, device=torch.device("cuda", self.device))
        else:
            rows, cnt = capi.as_u64(_as_numpy(ids)), capi.as_u32(_as_numpy(counts))
            sc = None if scores is None else np.ascontiguousarray(_as_numpy(scores), dtype=np.float64)
            ranks = np.zeros(n, np.uint32)
        _call_visitor_batch("srn_feedback_observe", [self._h], batch, now, [p(rows), p(sc), p(cnt), int(ids.shape[1]), p(ranks)])
        self.last_ranks = ranks
        return ranks

    def histogram(self):
        """-> (hits_model, hits_filled): uint64[row_cap + 1], hits by rank ([0] unused).  Blocks."""
        hm, hf = np.zeros(self.row_cap + 1, np.uint64), np.zeros(self.row_cap + 1, np.uint64)
        capi.check(capi.lib().srn_feedback_histogram(self._h, capi.ptr(hm), capi.ptr(hf), self.row_cap + 1))
        return hm, hf

    def stats(self, ci=0.95):
        """srn_feedback_stats_t as a dict (waits for the log's kernels), with feedback_metrics of the histograms: hit_rate, mrr and their _model / _filled parts.
        With the bootstrap enabled also "bootstrap" -- bootstrap()'s arrays, `ci` and "empty_replicates" -- and "<metric>_ci" for each of the six: the percentile
        interval at level `ci` of the replicates' values, feedback_metrics of a replicate's weighted histograms over its observed_w; replicates that observed
        nothing are left out and counted.  feedback_compare takes two such dicts."""
        st = capi.FeedbackStats()
        capi.check(capi.lib().srn_feedback_stats(self._h, C.byref(st)))
        out = {n: getattr(st, n) for n, _ in capi.FeedbackStats._fields_}
        out.update(feedback_metrics(*self.histogram(), out["observed"]))
        boot = self.bootstrap()
        return out if boot is None else _with_feedback_bootstrap(out, boot, float(ci))

    def reset_counters(self):
        capi.check(capi.lib().srn_feedback_reset_counters(self._h))

    def sweep(self, now=0):
        n = C.c_uint64()
        capi.check(capi.lib().srn_feedback_sweep(self._h, int(now), C.byref(n)))
        return n.value

    def get(self, key, now=1):
        """(test aid) -> (ids uint64[c], n_model, epoch) as a request at `now` would read the key's entry, or None (unknown, or idle at `now`); now = 1: whatever is stored."""
        out, c, nm, ep = np.zeros(self.row_cap, np.uint64), C.c_uint32(), C.c_uint32(), C.c_uint64()
        capi.check(capi.lib().srn_feedback_get(self._h, key >> 64, key & (2**64 - 1), int(now), capi.ptr(out), self.row_cap, C.byref(c), C.byref(nm), C.byref(ep)))
        return None if c.value == capi.FEEDBACK_NONE else (out[:c.value].copy(), nm.value, ep.value)

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:
            capi.lib().srn_feedback_free(self._h)
            self._h = None

    __del__ = close


def _observe_served(feedback, keys, item_ids, consent, ids, counts, scores, now, times=None):
    """recommend_batch's call of feedback.observe.  The session store has advanced and the rows are written by now, so a log that refuses the call (SRN_ENOMEM under the
    capacity rule, counted in stats()["refused"]) must not fail the serving call: the refusal becomes a warning, feedback.last_ranks None and feedback.last_error the
    exception; the log is as it was."""
    feedback.last_error = None
    try:
        feedback.observe(keys, item_ids, consent, ids, counts, scores, now=now, times=times)
    except capi.SerenadeError as e:
        if e.code != capi.SRN_ENOMEM:
            raise
        feedback.last_ranks, feedback.last_error = None, e
        warnings.warn("recommend_batch: the click feedback log did not take this call's rows: %s" % e, RuntimeWarning, stacklevel=3)


def recommend_batch(index, store, keys, item_ids, consent=None, *, k, m, how_many, max_items_in_session=2, enable_business_logic=False, now=0,
                    scores=False, exclude_seen=False, fill=False, feedback=None, times=None):
    """/v1/recommend for a batch: request i = (keys[i], item_ids[i], consent[i]); the result is what the requests served one after the other give.
    keys: (hi, lo) uint64 arrays / tensors, or a list of session-id strings.  -> (ids[n, how_many], counts[n]) and scores[n, how_many] with scores=True.
    NumPy arrays (or CPU tensors) in, NumPy arrays out; tensors on the index's GPU are read in place (on the current stream, without synchronising) and the
    outputs are tensors on it.  store may be None only if no request consents.
    exclude_seen (SRN_FLAG_EXCLUDE_SEEN): a request's rows leave out its visitor's window as the request sees it -- the store's history window, or the session window on a
    store without one; without consent nothing beyond the item itself.
    fill (SRN_FLAG_FILL): rows of fewer than how_many entries are filled from the index's fallback ranking (score -inf), leaving out what the request excludes.
    feedback (a ClickFeedback): the call's requests and rows also go through feedback.observe -- enqueued behind the recommend call on the same stream, with the same
    `now` (the clock is read once here when now = 0); the requests' ranks are left in feedback.last_ranks.  The return value is the same with or without it, also when
    the log refuses the call (its capacity is reached): that is a RuntimeWarning, feedback.last_ranks None and the error in feedback.last_error.
    times (srn_recommend_batch*_at): request i's own clock in seconds (uint64 / int64; 0 is a time like any other), an array or tensor like keys -- the
    call leaves rows, store, an attached harvest and the feedback log (which receives the same times) as one call per request at times[i] would, in request order;
    sessions end by idle time inside the call.  `now` is then only the SWEEP CLOCK of the capacity rule's automatic sweep and must be a lower bound of times; left at 0
    it is int(times.min()) -- for tensors that is ONE SYNCHRONISATION with the device, so a caller who knows a lower bound passes it.  (A log whose smallest time is
    0 still reads the wall clock there, as everywhere in the ABI.)"""
    n = len(item_ids)
    if times is not None and not int(now) and n:
        now = int(times.min())
    if feedback is not None:
        if how_many > feedback.row_cap:
            raise ValueError("how_many %d above the feedback log's row_cap %d" % (how_many, feedback.row_cap))
        if feedback.device != index.info["device"]:
            raise ValueError("the feedback log and the index are on different devices")
        now = int(now) or (int(time.time()) if times is None else 0)
    if isinstance(keys, list) and (not keys or isinstance(keys[0], (str, bytes))):
        if len(keys) != n:
            raise ValueError("keys, item_ids and consent differ in length")
        keys = session_keys(keys)
    flags = (capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0) | (capi.FLAG_EXCLUDE_SEEN if exclude_seen else 0) | (capi.FLAG_FILL if fill else 0)
    batch = _visitor_batch(keys, item_ids, consent, times, lambda: index.info["device"], "the index")
    hi, lo, it, con, tm, on_gpu, p, _ = batch
    if on_gpu:
        import torch
        dev = torch.device("cuda", index.info["device"])
        ids = torch.zeros((n, how_many), dtype=torch.int64, device=dev)
        sc = torch.zeros((n, how_many), dtype=torch.float64, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    else:
        ids, sc, cnt = np.zeros((n, how_many), np.uint64), np.zeros((n, how_many), np.float64), np.zeros(n, np.uint32)
    _call_visitor_batch("srn_recommend_batch", [index._h, store._h if store is not None else None], batch, now,
                        [int(max_items_in_session), int(k), int(m), int(how_many), flags, p(ids), p(sc), p(cnt)])
    if feedback is not None and n:
        _observe_served(feedback, (hi, lo), it, con, ids, cnt, sc, now, tm)
    return (ids, cnt, sc) if scores else (ids, cnt)


# ---- traffic split: one batch under several arms, sticky per visitor (srn_traffic_split_*) ----
_ARM_DOMAIN = 0x53524E5F41524D53


def _arm_weights(weights):
    """-> the weights as Python ints, checked as far as a uint32 array can hold them (the sums are the C ABI's to refuse)."""
    w = [int(x) for x in weights]
    if any(x < 0 or x >= 1 << 32 for x in w):
        raise ValueError("an arm's weight must be in 0 .. 2^32 - 1")
    return w


def arm_thresholds(weights):
    """T_a = floor(2^32 * (w_0 + .. + w_a) / W) for a = 0 .. A-1 as Python ints (the last one is 2^32).  ValueError for A outside 1 .. 16 or W outside 1 .. 2^32 - 1."""
    w = _arm_weights(weights)
    W = sum(w)
    if not 1 <= len(w) <= capi.MAX_ARMS or not 0 < W < 1 << 32:
        raise ValueError("a split has 1 .. %d arms whose weights sum to 1 .. 2^32 - 1" % capi.MAX_ARMS)
    out, cum = [], 0
    for x in w:
        cum += x
        out.append((cum << 32) // W)
    return out


def arm_draws(seed, keys):
    """u(seed, key) = mix64(mix64(seed ^ 0x53524E5F41524D53) ^ (fold(key) * 0xD1B54A32D192ED03 + 1)) >> 32 for keys = (hi, lo) -> uint64[n], each below 2^32."""
    with np.errstate(over="ignore"):
        rkey = _mix64(np.array([(int(seed) ^ _ARM_DOMAIN) & _M64], np.uint64))
        s = feedback_fold(keys).reshape(-1)
        return _mix64(rkey ^ (s * np.uint64(0xD1B54A32D192ED03) + np.uint64(1))) >> np.uint64(32)


def arms_model(seed, weights, keys):
    """The split's rule in NumPy, exactly (srn_arms.h): arm(key) = #{a < A - 1 : T_a <= u(seed, key)} -> uint8[n].  From (seed, weights, key) alone."""
    T = np.array(arm_thresholds(weights)[:-1], np.uint64)
    return np.searchsorted(T, arm_draws(seed, keys), side="right").astype(np.uint8)


class TrafficSplit:
    """A traffic split on one GPU (srn_traffic_split_*): (seed, weights) assign every visitor key to one of len(weights) arms, and recommend_batch_split serves a batch
    under the arms' parameters in one call.  Create it before serving: it allocates every buffer its calls use, about max_batch * (46 + 16 * max_how_many) bytes.
    After a call: last_arms (the requests' arms), last_ranks (their feedback ranks; capi.FEEDBACK_NONE where the arm has no log) and last_errors (per arm None, or
    the SerenadeError of a log that refused the arm's rows)."""

    def __init__(self, index_or_device, weights, seed=0, max_batch=1 << 20, max_how_many=21):
        device = _device_of(index_or_device)
        self.weights = _arm_weights(weights)
        h = C.c_void_p()
        capi.check(capi.lib().srn_traffic_split_create(int(device), capi.ptr(np.array(self.weights, np.uint32)), len(self.weights), int(seed) & _M64, int(max_batch),
                                                       int(max_how_many), C.byref(h)))
        self._h, self.device, self.seed, self.n_arms = h, int(device), int(seed) & _M64, len(self.weights)
        self.last_arms = self.last_ranks = None
        self.last_errors = [None] * self.n_arms

    def info(self):
        """srn_traffic_split_info_t as a dict; thresholds and served hold one entry per arm."""
        st = capi.TrafficSplitInfo()
        capi.check(capi.lib().srn_traffic_split_info(self._h, C.byref(st)))
        out = {n: getattr(st, n) for n, _ in capi.TrafficSplitInfo._fields_ if n not in ("thresholds", "served")}
        out["thresholds"], out["served"] = list(st.thresholds)[:st.n_arms], list(st.served)[:st.n_arms]
        return out

    def set_weights(self, weights):
        """The ramp: other weights for the same arms from the next call on.  Only the keys whose u lies between an old and a new threshold change their arm."""
        w = _arm_weights(weights)
        capi.check(capi.lib().srn_traffic_split_set_weights(self._h, capi.ptr(np.array(w, np.uint32)), len(w)))
        self.weights = w

    def arm_of(self, keys):
        """The rule on the host (srn_traffic_split_arms): the arms of keys = (hi, lo) under the split's seed and current weights -> uint8[n]."""
        hi, lo = (capi.as_u64(_as_numpy(a.cpu() if _on_gpu(a) else a)) for a in keys)
        if len(hi) != len(lo):
            raise ValueError("keys differ in length")
        out = np.zeros(len(hi), np.uint8)
        capi.check(capi.lib().srn_traffic_split_arms(self.seed, capi.ptr(np.array(self.weights, np.uint32)), self.n_arms, capi.ptr(hi), capi.ptr(lo), len(hi), capi.ptr(out)))
        return out

    def timing(self, enable=True):
        capi.check(capi.lib().srn_traffic_split_timing(self._h, 1 if enable else 0))

    def last_ms(self):
        """(assign + offsets + gather, scatter) of the last call in milliseconds, from HIP events (timing(True) first).  Blocks."""
        a, b = C.c_double(), C.c_double()
        capi.check(capi.lib().srn_traffic_split_last_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:
            capi.lib().srn_traffic_split_free(self._h)
            self._h = None

    __del__ = close


def _arm_array(arms):
    """The arms' dicts -- index, k, m, max_items_in_session (2), enable_business_logic, exclude_seen, fill, feedback -- as srn_arm_t[A]."""
    known = {"index", "k", "m", "max_items_in_session", "enable_business_logic", "exclude_seen", "fill", "feedback"}
    out = (capi.Arm * max(len(arms), 1))()
    for a, arm in enumerate(arms):
        if set(arm) - known:
            raise TypeError("an arm has no parameter %s" % ", ".join(sorted(set(arm) - known)))
        fb = arm.get("feedback")
        flags = (capi.FLAG_BUSINESS_LOGIC if arm.get("enable_business_logic") else 0) | (capi.FLAG_EXCLUDE_SEEN if arm.get("exclude_seen") else 0) | \
                (capi.FLAG_FILL if arm.get("fill") else 0)
        out[a] = capi.Arm(arm["index"]._h, None if fb is None else fb._h, int(arm.get("max_items_in_session", 2)), int(arm["k"]), int(arm["m"]), flags)
    return out


def recommend_batch_split(split, arms, store, keys, item_ids, consent=None, *, how_many, now=0, times=None, scores=False):
    """recommend_batch under a traffic split: request i is served with arms[arm(keys[i])] -- a dict of index, k, m and optionally max_items_in_session (2),
    enable_business_logic, exclude_seen, fill and feedback (a ClickFeedback of the arm's own) -- all arms against the one store.  The result is what one
    recommend_batch call per non-empty arm gives, arm 0 first, each over its arm's requests in request order with the call's one `now`: a visitor is in one arm, so
    the visitor's clicks stay in order.  -> (ids[n, how_many], counts[n]) and scores with scores=True, in request order; arrays and tensors as recommend_batch
    takes and gives them (tensors on the split's GPU are read in place on the current stream; the call waits for that stream once, to learn the arms' sizes).
    Left in the split: last_arms, last_ranks (the logs' ranks, capi.FEEDBACK_NONE for an arm without a log) and last_errors -- per arm None, or the SerenadeError
    of a log that refused its arm's rows under its capacity rule, which is a RuntimeWarning and does not fail the call.  The logs' own last_ranks are not touched.
    now / times: as recommend_batch (times given and now 0: int(times.min()), one synchronisation for tensors)."""
    n = len(item_ids)
    if times is not None and not int(now) and n:
        now = int(times.min())
    if isinstance(keys, list) and (not keys or isinstance(keys[0], (str, bytes))):
        if len(keys) != n:
            raise ValueError("keys, item_ids and consent differ in length")
        keys = session_keys(keys)
    batch = _visitor_batch(keys, item_ids, consent, times, lambda: split.device, "the split")
    hi, lo, it, con, tm, on_gpu, p, tail = batch
    if on_gpu:
        import torch
        dev = torch.device("cuda", split.device)
        ids = torch.zeros((n, how_many), dtype=torch.int64, device=dev)
        sc = torch.zeros((n, how_many), dtype=torch.float64, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        arm, rank = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    else:
        ids, sc, cnt = np.zeros((n, how_many), np.uint64), np.zeros((n, how_many), np.float64), np.zeros(n, np.uint32)
        arm, rank = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    arm_array, log_rc = _arm_array(arms), (C.c_int * max(len(arms), 1))()
    entry = getattr(capi.lib(), "srn_recommend_batch_split" + ("_device" if on_gpu else ""))
    capi.check(entry(split._h, arm_array, len(arms), store._h if store is not None else None, p(hi), p(lo), p(it), p(con), p(tm), n, int(now), int(how_many),
                     p(ids), p(sc), p(cnt), p(arm), p(rank), log_rc, *tail))
    split.last_arms, split.last_ranks = arm, rank
    split.last_errors = [None] * len(arms)
    for a in range(len(arms)):
        if log_rc[a]:
            split.last_errors[a] = capi.SerenadeError(log_rc[a], "arm %d's click feedback log did not take the call's rows (its capacity is reached)" % a)
            warnings.warn("recommend_batch_split: %s" % split.last_errors[a], RuntimeWarning, stacklevel=2)
    return (ids, cnt, sc) if scores else (ids, cnt)


def split_compare(stats, metric="mrr", baseline=0):
    """feedback_compare of every arm's log against the baseline arm's: stats = [fb.stats() per arm] -> a list with feedback_compare(stats[a], stats[baseline], metric)
    at a and None at the baseline.  The arms' visitors are disjoint, so the intervals are the unpaired ones."""
    if not 0 <= baseline < len(stats):
        raise ValueError("baseline must name one of the arms")
    return [None if a == baseline else feedback_compare(s, stats[baseline], metric) for a, s in enumerate(stats)]


# ---- replay: a recorded click log through the timed batch ----
def replay_plan(times, batch=1 << 20, every=None):
    """How replay() cuts a time-sorted log -> [(start, stop, boundary)]: the calls in order, requests start..stop-1 each, and `boundary` the multiple t of `every`
    that on_boundary is called with before the call (None: no boundary there).  With every=S there is a cut before every request i >= 1 whose time lies in another
    S-second interval than its predecessor's (times[i] // S != times[i - 1] // S), at t = times[i] // S * S -- a gap that spans several multiples is one cut, at the
    last of them; the stretches between those cuts are served in calls of at most `batch` requests.  ValueError if times decreases anywhere."""
    t = np.asarray(times).astype(np.uint64)
    n = len(t)
    if batch < 1 or (every is not None and every < 1):
        raise ValueError("batch and every must be positive")
    if n > 1 and bool((t[1:] < t[:-1]).any()):
        raise ValueError("replay: times must not decrease (sort the log by time first)")
    edges = [(0, None)]
    if every is not None and n > 1:
        q = t // np.uint64(every)
        edges += [(int(i), int(q[i]) * int(every)) for i in np.flatnonzero(q[1:] != q[:-1]) + 1]
    plan = []
    for (a, boundary), (b, _) in zip(edges, edges[1:] + [(n, None)]):
        for s in range(a, b, int(batch)):
            plan.append((s, min(s + int(batch), b), boundary if s == a else None))
    return plan


def replay(index, store, keys, item_ids, times, consent=None, *, k, m, how_many, max_items_in_session=2, batch=1 << 20, every=None, on_boundary=None, feedback=None,
           exclude_seen=False, fill=False, enable_business_logic=False, collect=False, split=None, arms=None):
    """Serves a recorded click log (keys[i], item_ids[i], times[i], consent[i]), sorted by time, through recommend_batch(..., times=...): every request sees the store,
    the harvest and the feedback log as it would have at its own second, at the speed of the batch path.  Arrays or tensors as recommend_batch takes them (times on the
    GPU are copied to the host once, to plan the cuts and read the sweep clocks).  The log is cut into calls by replay_plan(times, batch, every): at most `batch` requests each and, with
    every=S, a cut wherever the log crosses a multiple t of S seconds -- there on_boundary(t) is called before the requests at or after t are served: the place to
    store.sweep(t), or to refresh the ranking with index.set_fallback_trending(store, n, now=t).  Each call's sweep clock is its first request's time.  ValueError
    before anything is served if times decreases anywhere.  No device code of its own.
    -> {"requests", "calls", "boundaries"}, plus feedback.stats() under "feedback" with a feedback log, plus with collect=True the calls' concatenated "ids",
    "counts" and (with a feedback log) "ranks".
    split and arms (a TrafficSplit and its arms' dicts, both or neither): the calls go through recommend_batch_split(split, arms, store, ...) instead -- index, k, m,
    max_items_in_session, the flags and feedback are then the arms' and this call's are not read.  "feedback" is then a list per arm (the log's stats(), None for an
    arm without one), "arms" the requests served per arm, and collect=True adds "arm" and always "ranks" (split.last_arms / last_ranks)."""
    if (split is None) != (arms is None):
        raise ValueError("replay: split and arms go together")
    n = len(item_ids)
    if len(times) != n:
        raise ValueError("times must have one entry per request")
    host_times = times.cpu().numpy() if _is_torch(times) else np.asarray(times)
    plan = replay_plan(host_times, batch, every)
    if isinstance(keys, list) and (not keys or isinstance(keys[0], (str, bytes))):
        if len(keys) != n:
            raise ValueError("keys, item_ids and consent differ in length")
        keys = session_keys(keys)
    hi, lo = keys
    out = {"requests": n, "calls": 0, "boundaries": 0}
    parts = {"ids": [], "counts": [], "ranks": []}
    if split is not None:
        parts["arm"] = []
        out["arms"] = [0] * len(arms)
    for start, stop, boundary in plan:
        if boundary is not None:
            out["boundaries"] += 1
            if on_boundary is not None:
                on_boundary(boundary)
        if stop == start:
            continue
        sl = slice(start, stop)
        if split is not None:
            ids, counts = recommend_batch_split(split, arms, store, (hi[sl], lo[sl]), item_ids[sl], None if consent is None else consent[sl], how_many=how_many,
                                                now=int(host_times[start]), times=times[sl])
            out["calls"] += 1
            served = np.bincount(_as_numpy(split.last_arms.cpu() if _on_gpu(split.last_arms) else split.last_arms), minlength=len(arms))
            out["arms"] = [int(x + y) for x, y in zip(out["arms"], served)]
            if collect:
                for name, got in (("ids", ids), ("counts", counts), ("ranks", split.last_ranks), ("arm", split.last_arms)):
                    parts[name].append(got)
            continue
        ids, counts = recommend_batch(index, store, (hi[sl], lo[sl]), item_ids[sl], None if consent is None else consent[sl], k=k, m=m, how_many=how_many,
                                      max_items_in_session=max_items_in_session, enable_business_logic=enable_business_logic, now=int(host_times[start]),
                                      exclude_seen=exclude_seen, fill=fill, feedback=feedback, times=times[sl])
        out["calls"] += 1
        if collect:
            parts["ids"].append(ids)
            parts["counts"].append(counts)
            if feedback is not None:
                parts["ranks"].append(feedback.last_ranks)
    if split is not None:
        out["feedback"] = [None if arm.get("feedback") is None else arm["feedback"].stats() for arm in arms]
    elif feedback is not None:
        out["feedback"] = feedback.stats()
    if collect:
        for name, got in parts.items():
            if name == "ranks" and feedback is None and split is None:
                continue
            if got and _is_torch(got[0]):
                import torch
                out[name] = torch.cat(got)
            else:
                out[name] = np.concatenate(got) if got else np.zeros((0, how_many) if name == "ids" else 0, {"ids": np.uint64, "arm": np.uint8}.get(name, np.uint32))
    return out
