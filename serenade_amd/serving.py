"""Dynamic batching in front of the predict kernel (srn_batcher_*): the serving-side caller of the hot path.

The reference answers each /v1/recommend call with its own vmisknn::predict on an actix worker thread
(src/endpoints/recommend_resource.rs:56-62).  `Batcher.predict` has that call's shape and may be called from many threads
at once; the library folds the waiting calls into one kernel launch.  No HTTP and no session store here."""
import ctypes as C

import numpy as np

from . import capi
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

def _is_torch(x):
    return type(x).__module__.split(".")[0] == "torch"


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


class DeviceSessionStore:
    """The evolving sessions in the GPU's memory: what recommend_batch reads and updates.  get / update / sweep mirror SessionStore's, for one key, from the host."""

    def __init__(self, device_or_index, capacity, items_cap=16, ttl_secs=30 * 60, idle_secs=20 * 60):
        device = device_or_index if isinstance(device_or_index, int) else device_or_index.info["device"]
        h = C.c_void_p()
        capi.check(capi.lib().srn_device_sessions_create(int(device), int(capacity), int(items_cap), int(ttl_secs), int(idle_secs), C.byref(h)))
        self._h, self.device, self.items_cap = h, int(device), int(items_cap)

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
            capi.lib().srn_device_sessions_free(self._h)
            self._h = None

    __del__ = close


def recommend_batch(index, store, keys, item_ids, consent=None, *, k, m, how_many, max_items_in_session=2, enable_business_logic=False, now=0,
                    scores=False):
    """/v1/recommend for a batch: request i = (keys[i], item_ids[i], consent[i]); the result is what the requests served one after the other give.
    keys: (hi, lo) uint64 arrays / tensors, or a list of session-id strings.  -> (ids[n, how_many], counts[n]) and scores[n, how_many] with scores=True.
    NumPy arrays (or CPU tensors) in, NumPy arrays out; tensors on the index's GPU are read in place (on the current stream, without synchronising) and the
    outputs are tensors on it.  store may be None only if no request consents."""
    n = len(item_ids)
    if isinstance(keys, list) and (not keys or isinstance(keys[0], (str, bytes))):
        if len(keys) != n:
            raise ValueError("keys, item_ids and consent differ in length")
        keys = session_keys(keys)
    hi, lo = keys
    arrs = [hi, lo, item_ids] + ([consent] if consent is not None else [])
    if any(len(a) != n for a in arrs):
        raise ValueError("keys, item_ids and consent differ in length")
    flags = capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0
    sh = store._h if store is not None else None
    on_gpu = [_is_torch(a) and a.device.type == "cuda" for a in arrs]
    if any(on_gpu):
        import torch
        device = index.info["device"]
        if not all(on_gpu) or any(a.device.index != device for a in arrs):
            raise ValueError("keys, item_ids and consent must all be tensors on the index's GPU (device %d), or none of them" % device)
        hi, lo, it = (a.contiguous() for a in arrs[:3])
        for a in (hi, lo, it):
            if a.dtype not in (torch.int64, getattr(torch, "uint64", torch.int64)):
                raise TypeError("keys and item_ids must be 64-bit integer tensors")
        con = None
        if consent is not None:
            con = consent.contiguous()
            if con.dtype not in (torch.uint8, torch.bool):
                raise TypeError("consent must be a uint8 or bool tensor")
        dev = torch.device("cuda", device)
        ids = torch.zeros((n, how_many), dtype=torch.int64, device=dev)
        sc = torch.zeros((n, how_many), dtype=torch.float64, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(device).cuda_stream
        capi.check(capi.lib().srn_recommend_batch_device(
            index._h, sh, C.c_void_p(hi.data_ptr()), C.c_void_p(lo.data_ptr()), C.c_void_p(it.data_ptr()), None if con is None else C.c_void_p(con.data_ptr()),
            n, int(now), int(max_items_in_session), int(k), int(m), int(how_many), flags,
            C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(stream)))
        return (ids, cnt, sc) if scores else (ids, cnt)
    hi, lo, it = (capi.as_u64(a.numpy() if _is_torch(a) else a) for a in arrs[:3])
    con = None if consent is None else np.ascontiguousarray(consent.numpy() if _is_torch(consent) else consent).astype(np.uint8)
    ids, sc, cnt = np.zeros((n, how_many), np.uint64), np.zeros((n, how_many), np.float64), np.zeros(n, np.uint32)
    capi.check(capi.lib().srn_recommend_batch(index._h, sh, capi.ptr(hi), capi.ptr(lo), capi.ptr(it), capi.ptr(con), n, int(now), int(max_items_in_session),
                                              int(k), int(m), int(how_many), flags, capi.ptr(ids), capi.ptr(sc), capi.ptr(cnt)))
    return (ids, cnt, sc) if scores else (ids, cnt)
