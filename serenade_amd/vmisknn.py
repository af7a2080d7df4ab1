"""Host-side mirror of the reference's interface for the VMIS-kNN hot path, over the C ABI.

Reference (bolcom/serenade, Rust)                      here
---------------------------------------------------   -------------------------------------------
vmis_index::VMISIndex::new_from_csv(path, m, idf_w)    VMISIndex.new_from_csv(path, m, idf_w)
  (src/vmisknn/vmis_index.rs:38-83)
vmisknn::predict(&index, &session, k, m, how_many,     predict(index, session, k, m, how_many,
                 enable_business_logic)                        enable_business_logic)
  -> BinaryHeap<ItemScore>, callers take               -> list[ItemScore] already in
     .into_sorted_vec()  (src/vmisknn/mod.rs:118-215)     into_sorted_vec() order (score-descending)
ItemScore { id: u64, score: f64 } (mod.rs:45-49)       ItemScore(id, score)

All compute happens in libserenade_hip.so on the GPU.  There is no Python or CPU implementation of
the path in this package; without the library or without a GPU the calls raise.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import capi
from .capi import SerenadeError  # noqa: F401  (re-export)

ItemScore = namedtuple("ItemScore", ["id", "score"])


class VMISIndex:
    """Owns an srn_index_t handle (flat CSR index in HBM)."""

    def __init__(self, handle):
        self._h = handle

    # ---- constructors ---------------------------------------------------------------------
    @classmethod
    def new_from_csv(cls, path_to_training, m_most_recent_sessions, idf_weighting, max_session_len=0, device=0, loader="host"):
        """VMISIndex::new_from_csv (vmis_index.rs:38-83).  max_session_len=0: exact p99.5 of session lengths
        (the reference uses a t-digest estimate of the same quantile, vmis_index.rs:689-716).
        loader="gpu" parses and groups the file on the device (srn_index_new_from_csv_gpu: the same index; needs device >= 0)."""
        if loader not in ("host", "gpu"):
            raise ValueError("loader must be 'host' or 'gpu'")
        h = C.c_void_p()
        load = capi.lib().srn_index_new_from_csv_gpu if loader == "gpu" else capi.lib().srn_index_new_from_csv
        capi.check(load(str(path_to_training).encode(), int(m_most_recent_sessions), float(idf_weighting), int(max_session_len), int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def from_events(cls, session_ids, item_ids, times, m_most_recent_sessions, idf_weighting, max_session_len=0, device=0, builder="gpu"):
        """new_from_csv on rows already in memory, in file order: NumPy arrays, torch tensors on the CPU, or torch tensors on this
        device (read in place).  times: float (rounded like the file's) or integer seconds.  Grouped and built on the GPU.
        builder="gpu": the grouped sessions come to the host, go back up for the builder, and the built index comes down before it is attached
        (srn_sessions_from_events + srn_index_build_gpu).  builder="resident" (srn_index_from_events_device): the same index, bit for bit, with the large arrays never
        leaving the device; its host copy is fetched once, by the first call that reads it there (save, postings, items_for_session ...: host_state(), materialize())."""
        if builder not in ("gpu", "resident"):
            raise ValueError("builder must be 'gpu' or 'resident'")
        if builder == "resident":
            from .ingest import _event_args
            keep, (ps, pi, pt), n, flags, stream = _event_args(session_ids, item_ids, times, int(device))
            h = C.c_void_p()
            capi.check(capi.lib().srn_index_from_events_device(C.c_void_p(ps), C.c_void_p(pi), C.c_void_p(pt), n, flags, int(m_most_recent_sessions), float(idf_weighting),
                                                               int(max_session_len), int(device), None if stream is None else C.c_void_p(stream), C.byref(h)))
            del keep
            return cls(h)
        from .ingest import TrainingSessions
        ts = TrainingSessions.from_events(session_ids, item_ids, times, device=device)
        try:
            max_len = int(max_session_len) or ts.length_quantile(0.995)
            v = ts.view()
            h = C.c_void_p()
            capi.check(capi.lib().srn_index_build_gpu(C.byref(v), int(m_most_recent_sessions), max_len, float(idf_weighting), int(device), C.byref(h)))
        finally:
            ts.close()
        return cls(h)

    @classmethod
    def from_sessions(cls, sess_off, items, max_ts, m_index, max_session_len, idf_weighting=1.0, device=0, builder="host"):
        """prepare_hashmap (vmis_index.rs:422-528) on sessions already in (ascending, de-duplicated) row form.
        builder="gpu" constructs the identical index with rocPRIM sorts on the device (needs device >= 0)."""
        sess_off, items, max_ts = capi.as_u64(sess_off), capi.as_u64(items), capi.as_u32(max_ts)
        if len(sess_off) != len(max_ts) + 1 or (len(sess_off) and int(sess_off[-1]) != len(items)):
            raise ValueError("inconsistent session CSR")
        v = capi.SessionsView(sess_off.ctypes.data, items.ctypes.data, max_ts.ctypes.data, len(max_ts))
        h = C.c_void_p()
        build = capi.lib().srn_index_build_gpu if builder == "gpu" else capi.lib().srn_index_build
        capi.check(build(C.byref(v), int(m_index), int(max_session_len), float(idf_weighting), int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def new_from_avro(cls, base_path, device=0):
        """VMISIndex::new(base_path) (vmis_index.rs:85-314): pre-built index from <base>/itemindex and <base>/sessionindex Avro files."""
        h = C.c_void_p()
        capi.check(capi.lib().srn_index_new_from_avro(str(base_path).encode(), int(device), C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, path, device=0):
        h = C.c_void_p()
        capi.check(capi.lib().srn_index_load(str(path).encode(), int(device), C.byref(h)))
        return cls(h)

    def save(self, path):
        capi.check(capi.lib().srn_index_save(self._h, str(path).encode()))

    def close(self):
        if getattr(self, "_h", None) and capi is not None and getattr(capi, "lib", None) is not None:   # (None at interpreter shutdown)
            capi.lib().srn_index_free(self._h)
            self._h = None

    __del__ = close

    # ---- accessors ------------------------------------------------------------------------
    @property
    def info(self):
        out = capi.IndexInfo()
        capi.check(capi.lib().srn_index_info(self._h, C.byref(out)))
        return {n: getattr(out, n) for n, _ in capi.IndexInfo._fields_}

    def host_state(self):
        """srn_index_host_state as a dict: host_complete (False only for a builder="resident" index no host reader has asked yet), build_bytes_on_device (device bytes
        held for that deferred download alone; part of info["device_bytes"]), materialisations (0 or 1), and the resident build's stage times in ms."""
        st = capi.IndexHostState()
        capi.check(capi.lib().srn_index_host_state(self._h, C.byref(st)))
        out = {n: getattr(st, n) for n, _ in capi.IndexHostState._fields_ if n != "reserved"}
        out["host_complete"] = bool(out["host_complete"])
        return out

    def materialize(self):
        """Bring the host copy up to date now (what the first save / postings / items_for_session call would do); idempotent."""
        capi.check(capi.lib().srn_index_materialize(self._h))

    def set_attributes(self, item_ids, flags):
        ids, fl = capi.as_u64(item_ids), np.ascontiguousarray(flags, np.uint8)
        capi.check(capi.lib().srn_index_set_attributes(self._h, capi.ptr(ids), capi.ptr(fl), len(ids)))

    # ---- the fallback ranking (srn_index_set_fallback*): what short rows are filled from with fill=True ----
    def set_fallback(self, ids):
        """Up to capi.MAX_FALLBACK distinct public item ids, best first (ids the index does not know are allowed); replaces an earlier ranking.  Waits for the device:
        set it before serving, and with no call on the index in flight."""
        a = capi.as_u64(ids)
        capi.check(capi.lib().srn_index_set_fallback(self._h, capi.ptr(a), len(a)))

    def set_fallback_popular(self, n):
        """The first min(n, n_items) items of the index's popularity order (count of kept sessions that hold the item descending, id ascending)."""
        capi.check(capi.lib().srn_index_set_fallback_popular(self._h, int(n)))

    def set_fallback_trending(self, store, n, since=0, min_count=1, popular_tail=True, now=0):
        """srn_index_set_fallback_trending: the ranking becomes the first n entries of store.top_items(n, since, min_count, now) -- what the live sessions of a
        serving.DeviceSessionStore hold most often, products listed since the index was built included -- and, with popular_tail, when those are fewer than n, the index's
        popularity order without repeats behind them, n in all.  -> the number of entries taken from the store (0 with no tail: the ranking is left as it was).  The
        rule of set_fallback holds: no call on the index in flight."""
        got = C.c_size_t()
        capi.check(capi.lib().srn_index_set_fallback_trending(self._h, store._h, int(now), int(since), int(min_count), int(n),
                                                              capi.TRENDING_POPULAR_TAIL if popular_tail else 0, C.byref(got)))
        return got.value

    def fallback(self):
        """The ranking as set: uint64[R] (R = 0: none)."""
        n = C.c_size_t()
        capi.check(capi.lib().srn_index_fallback(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint64)
        capi.check(capi.lib().srn_index_fallback(self._h, capi.ptr(out) if n.value else None, n.value, C.byref(n)))
        return out

    def clear_fallback(self):
        capi.check(capi.lib().srn_index_clear_fallback(self._h))

    def postings(self, item_id):
        """(reference session indices most-recent-first, idf) of one item, or (None, None) if unknown."""
        n, idf = C.c_int64(), C.c_double()
        capi.check(capi.lib().srn_index_postings(self._h, int(item_id), None, 0, C.byref(n), C.byref(idf)))
        if n.value < 0:
            return None, None
        out = np.zeros(max(n.value, 1), np.uint32)
        capi.check(capi.lib().srn_index_postings(self._h, int(item_id), capi.ptr(out), n.value, C.byref(n), C.byref(idf)))
        return out[:n.value], idf.value

    # the trait's other accessors (SimilarityComputationNew, src/vmisknn/similarity_indexed.rs:9-23)
    def idf(self, item_id):
        """idf(&u64) -> f64 (vmis_index.rs:321-323).  The reference panics on an unknown item; here: KeyError."""
        n, idf = C.c_int64(), C.c_double()
        capi.check(capi.lib().srn_index_postings(self._h, int(item_id), None, 0, C.byref(n), C.byref(idf)))
        if n.value < 0:
            raise KeyError(item_id)
        return idf.value

    def items_for_session(self, session):
        """items_for_session(&u32) -> &[u64] (vmis_index.rs:317-319): ascending item ids of a kept session, by its reference session index."""
        n = C.c_size_t()
        capi.check(capi.lib().srn_index_items_for_session(self._h, int(session), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint64)
        capi.check(capi.lib().srn_index_items_for_session(self._h, int(session), capi.ptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def serve_start(self, k, m, how_many, enable_business_logic=False, lanes=1, max_items_in_session=4, idle_ms=2000):
        """srn_index_serve_start: park `lanes` resident workgroups that answer predict() calls of exactly these parameters without a kernel launch."""
        capi.check(capi.lib().srn_index_serve_start(self._h, int(k), int(m), int(how_many), int(bool(enable_business_logic)), int(lanes), int(max_items_in_session), int(idle_ms)))

    def serve_stop(self):
        capi.check(capi.lib().srn_index_serve_stop(self._h))

    def serve_stats(self):
        """(answered by a resident workgroup, sent to the launch path, kernel launches, resident workgroups)"""
        a, b, c, n = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        capi.check(capi.lib().srn_index_serve_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return a.value, b.value, c.value, n.value

    def serve_lane_counts(self, form):
        """srn_debug_serve_lane_counts: sessions each resident workgroup of `form` (0: <= 4 items, 1: 5..10) has answered itself; test aid."""
        n = C.c_size_t()
        out = np.zeros(256, np.uint64)
        capi.check(capi.lib().srn_debug_serve_lane_counts(self._h, int(form), capi.ptr(out), len(out), C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def enable_result_cache(self, rows, max_len, k, m, how_many, business_logic=False):
        """srn_index_result_cache_enable: keep served rows of sequences of 1..max_len (<= 8) items in a device table of `rows` entries; batch calls with exactly these
        parameters on the fast path then answer repeated sequences from it (the same bytes), every other call bypasses it."""
        rows, max_len, k, m, how_many = int(rows), int(max_len), int(k), int(m), int(how_many)
        if rows <= 0:
            raise ValueError("rows must be > 0")
        if not 1 <= max_len <= 8:
            raise ValueError("max_len must be 1..8")
        if k <= 0 or m <= 0 or how_many <= 0:
            raise ValueError("k, m and how_many must be > 0")
        capi.check(capi.lib().srn_index_result_cache_enable(self._h, rows, max_len, k, m, how_many, capi.FLAG_BUSINESS_LOGIC if business_logic else 0))

    def disable_result_cache(self):
        capi.check(capi.lib().srn_index_result_cache_disable(self._h))

    def clear_result_cache(self):
        capi.check(capi.lib().srn_index_result_cache_clear(self._h))

    def result_cache_stats(self):
        """srn_index_result_cache_stats as a dict (waits for the cache's kernels): rows, ways, bytes, the parameters, and since enable lookups, hits, inserts, evictions,
        bypassed_calls, clears."""
        st = capi.ResultCacheStats()
        capi.check(capi.lib().srn_index_result_cache_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in capi.ResultCacheStats._fields_ if n != "reserved"}

    def session_recency(self):
        """Recency rank of every reference session (0 = oldest; 0xFFFFFFFF: not kept): the total order behind "most recent", ties among equal timestamps included."""
        n = int(self.info["n_sessions_total"])
        out = np.zeros(max(n, 1), np.uint32)
        capi.check(capi.lib().srn_index_session_recency(self._h, capi.ptr(out), len(out)))
        return out[:n]

    def find_attributes(self, item_id):
        """find_attributes(&u64) -> Option<&ProductAttributes> (vmis_index.rs:417-419): the SRN_ATTR_* bits, or None."""
        fl = C.c_uint8()
        capi.check(capi.lib().srn_index_find_attributes(self._h, int(item_id), C.byref(fl)))
        return None if fl.value == capi.ATTR_NONE else int(fl.value)

    def find_neighbors(self, evolving_session, k, m):
        """find_neighbors(&[u64], k, m) (vmis_index.rs:325-415) -> (reference session indices u32[K], similarities f64[K]), best first."""
        ev = capi.as_u64(evolving_session)
        ses, sc, n = np.zeros(max(int(k), 1), np.uint32), np.zeros(max(int(k), 1)), C.c_size_t()
        capi.check(capi.lib().srn_find_neighbors(self._h, capi.ptr(ev), len(ev), int(k), int(m), capi.ptr(ses), capi.ptr(sc), C.byref(n)))
        return ses[:n.value], sc[:n.value]

    def kernel_timing(self, enable=True):
        """srn_kernel_timing: per-kernel HIP events on every batch call (what last_kernel_ms / kernel_times* read); off by default -- each event idles the stream ~6 us."""
        capi.check(capi.lib().srn_kernel_timing(self._h, 1 if enable else 0))

    def last_kernel_ms(self):
        """(avg ms of the main predict kernel, ms of the retry pass, #queries retried) for the last call."""
        a, b, r = C.c_double(), C.c_double(), C.c_uint32()
        capi.check(capi.lib().srn_last_kernel_ms(self._h, C.byref(a), C.byref(b), C.byref(r)))
        return a.value, b.value, r.value


    def last_path_counts(self):
        """(queries of the last call, served by the general kernel, served through the global-table pass)."""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        capi.check(capi.lib().srn_last_path_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def last_mid_count(self):
        """Queries of the last call that the lean fast kernel listed for its MID instantiation (sessions of <= 10 items, 5..8 lists); measurement aid."""
        a = C.c_uint32()
        capi.check(capi.lib().srn_debug_last_mid_count(self._h, C.byref(a)))
        return a.value

    def last_dedup_count(self):
        """Queries of the last call that got the row of an earlier query of the same call with the same item sequence instead of being served; measurement aid."""
        a = C.c_uint32()
        capi.check(capi.lib().srn_debug_last_dedup_count(self._h, C.byref(a)))
        return a.value

    def last_light_count(self):
        """Light representatives of the last call: distinct queries with one posting run of <= 64 kept entries, which the light form served one wave each (0: the form was
        off in that call -- SRN_LIGHT_MIN, a result-cache call); measurement aid."""
        a = C.c_uint32()
        capi.check(capi.lib().srn_debug_last_light_count(self._h, C.byref(a)))
        return a.value

    def last_big_count(self):
        """... and how many of those the MID instantiation listed for its BIG form (merged lists beyond the 53 KB layout's buffers); measurement aid."""
        a = C.c_uint32()
        capi.check(capi.lib().srn_debug_last_big_count(self._h, C.byref(a)))
        return a.value

    GEOMETRY_WORDS = ("masks", "slot64", "slot_bytes", "lds", "sess_may_overflow", "item_may_overflow", "sketch_may_wrap", "lds_max",
                      "sess_slots", "item_slots", "item_buckets", "hot_slots", "sketch_slots", "sketch_shift", "sum_bits", "num_bits", "q_cap",
                      "off_q", "off_wave", "off_b", "off_a", "region_a_bytes", "no_merge")

    def debug_geometry(self, k, m, max_len, flags=0):
        """srn_debug_geometry: what the runtime decides for one launch of the general kernel at (k, m, max_len, flags) under the current knobs -> {name: word}
        (GEOMETRY_WORDS).  Host code only, nothing is launched; test aid."""
        out = np.zeros(24, np.uint32)
        capi.check(capi.lib().srn_debug_geometry(self._h, int(k), int(m), int(max_len), int(flags), capi.ptr(out)))
        return dict(zip(self.GEOMETRY_WORDS, (int(x) for x in out)))

    def kernel_times(self, max_n=64):
        """Per-call (main kernel ms, retry pass ms) of the most recent predict calls, oldest first (HIP events
        recorded on the launch stream around each launch)."""
        a, b, n = np.zeros(max_n), np.zeros(max_n), C.c_uint32()
        capi.check(capi.lib().srn_kernel_times(self._h, max_n, capi.ptr(a), capi.ptr(b), C.byref(n)))
        return a[:n.value].copy(), b[:n.value].copy()


    def kernel_times_detail(self, max_n=64):
        """Per-call ms of (prep kernel, fast kernel alone, all predict launches, global-table retry pass), oldest first."""
        a, b, c, d, n = np.zeros(max_n), np.zeros(max_n), np.zeros(max_n), np.zeros(max_n), C.c_uint32()
        capi.check(capi.lib().srn_kernel_times_detail(self._h, max_n, capi.ptr(a), capi.ptr(b), capi.ptr(c), capi.ptr(d), C.byref(n)))
        return tuple(x[:n.value].copy() for x in (a, b, c, d))

    def debug_phase_cycles(self, enable):
        """Profiling aid: fetch-and-clear the per-phase shader-cycle counters, then switch accounting on/off."""
        out = np.zeros(16, np.uint64)
        capi.check(capi.lib().srn_debug_phase_cycles(self._h, int(bool(enable)), capi.ptr(out)))
        return out


CSR = namedtuple("CSR", ["items_flat", "q_off"])
CSR.__doc__ = "Explicit CSR batch: CSR(items_flat u64[nnz], q_off int[nq + 1]).  Unambiguous, unlike a bare tuple of two arrays."


def _is_csr_pair(sessions):
    """A bare tuple (items_flat, q_off) is read as CSR only if it cannot be two evolving sessions of the same kind: two 1-D integer numpy arrays whose second one starts
    at 0, is non-decreasing and ends at len(first), AND whose dtypes tell them apart -- q_off is uint32 (what the C ABI takes: nobody keeps item ids in it), or
    items_flat is uint64 and q_off any other integer dtype (what np.cumsum hands back).  Two arrays of ONE dtype that also read as (items, offsets) are refused
    (ValueError): since round 4 such a pair -- e.g. int64 items with int64 np.cumsum offsets, accepted as CSR before -- must be passed as
    `CSR(items_flat, q_off)` (README, "Python mirror"); a wrong guess would answer a different question silently."""
    if isinstance(sessions, CSR):
        flat, off = np.asarray(sessions.items_flat), np.asarray(sessions.q_off)
        if flat.ndim != 1 or off.ndim != 1 or len(off) < 1 or int(off[0]) != 0 or int(off[-1]) != len(flat) or (len(off) > 1 and not bool((off[1:] >= off[:-1]).all())):
            raise ValueError("CSR(items_flat, q_off): q_off must start at 0, be non-decreasing and end at len(items_flat)")
        return True
    if not (isinstance(sessions, tuple) and len(sessions) == 2 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in sessions)):
        return False
    flat, off = sessions
    if not np.issubdtype(off.dtype, np.integer) or not np.issubdtype(flat.dtype, np.integer) or len(off) < 1:
        return False
    looks = int(off[0]) == 0 and int(off[-1]) == len(flat) and (len(off) < 2 or bool((off[1:] >= off[:-1]).all()))
    if not looks:
        return False
    if (off.dtype == np.uint32 and flat.dtype != np.uint32) or (flat.dtype == np.uint64 and off.dtype != np.uint64):
        return True
    # two arrays of one kind whose second one also reads as offsets of the first: refuse to guess
    raise ValueError("ambiguous batch: a tuple of two %s / %s arrays that could be (items_flat, q_off) or two evolving sessions -- "
                     "pass serenade_amd.CSR(items_flat, q_off), or q_off as uint32, or the two sessions as lists" % (flat.dtype, off.dtype))


def _flatten(sessions):
    # CSR input is CSR(items_flat, q_off) or a tuple of two numpy arrays of different kinds, see _is_csr_pair; a tuple of two evolving sessions (lists, or arrays
    # that are not such a pair) is two queries
    if _is_csr_pair(sessions):
        if len(sessions[0]) > 0xFFFFFFFF:
            raise ValueError("more than 2^32 - 1 items in one batch: q_off is 32-bit in the C ABI")
        return capi.as_u64(sessions[0]), capi.as_u32(sessions[1])
    off = np.zeros(len(sessions) + 1, np.uint32)
    off[1:] = np.cumsum([len(s) for s in sessions])
    flat = np.fromiter((x for s in sessions for x in s), dtype=np.uint64, count=int(off[-1]))
    return flat, off


def predict(index, evolving_session, k, m, how_many, enable_business_logic):
    """vmisknn::predict (src/vmisknn/mod.rs:118-125); returns list[ItemScore], score-descending."""
    ev = capi.as_u64(evolving_session)
    ids, sc, n = np.zeros(max(how_many, 1), np.uint64), np.zeros(max(how_many, 1)), C.c_size_t()
    capi.check(capi.lib().srn_predict(index._h, capi.ptr(ev), len(ev), int(k), int(m), int(how_many),
                                      int(bool(enable_business_logic)), capi.ptr(ids), capi.ptr(sc), C.byref(n)))
    return [ItemScore(int(i), float(s)) for i, s in zip(ids[:n.value], sc[:n.value])]


def _flatten_exclude(exclude, nq):
    """The exclusion lists of a batch -- a list of nq sequences of item ids, or CSR(ids_flat, off) -> (ids u64, off u32, the longest list)."""
    if isinstance(exclude, CSR):
        _is_csr_pair(exclude)
        xf, xo = capi.as_u64(exclude[0]), capi.as_u32(exclude[1])
    else:
        xo = np.zeros(len(exclude) + 1, np.uint32)
        xo[1:] = np.cumsum([len(x) for x in exclude])
        xf = np.fromiter((i for x in exclude for i in x), dtype=np.uint64, count=int(xo[-1]))
    if len(xo) - 1 != nq:
        raise ValueError("exclude must hold one list per query (%d lists for %d queries)" % (len(xo) - 1, nq))
    return xf, xo, int(np.diff(xo.astype(np.int64)).max()) if nq else 0


def predict_batch(index, sessions, k, m, how_many, enable_business_logic=False, out=None, exclude=None, exclude_session=False, max_excl=None, fill=False):
    """Many evolving sessions in one call (list of sequences, or (items_flat, q_off)).
    -> (ids u64[nq, how_many], scores f64[nq, how_many], counts u32[nq]).  out = (ids, scores, counts) of an earlier call of the same
    shape: the result buffers are reused (what a serving / evaluator host does) instead of freshly allocated.
    exclude: per query a list of item ids that must not be recommended (a list of nq lists, or CSR(ids_flat, off)); exclude_session: neither may any item of the query's own
    session.  The rows are those of "remove the ids from all candidates, then cut to how_many" (srn_predict_batch_excl).  max_excl: the capacity of one list (default: the
    longest list given); how_many + max_excl (+ the longest session - 1 with exclude_session) may not exceed SRN_MAX_HOW_MANY.
    fill (SRN_FLAG_FILL): rows of fewer than how_many entries are filled from the index's fallback ranking (VMISIndex.set_fallback*), score -inf, leaving out what the call
    excludes (serving.fill_rows is the rule in NumPy); it takes the same entry point as exclude."""
    flat, off = _flatten(sessions)
    nq = len(off) - 1
    if exclude is not None or exclude_session or fill:
        if out is not None:
            raise ValueError("out is not supported together with exclude / exclude_session / fill")
        xf, xo, longest = _flatten_exclude(exclude, nq) if exclude is not None else (None, None, 0)
        cap = longest if max_excl is None else int(max_excl)
        ids, sc, cnt = np.zeros((nq, how_many), np.uint64), np.zeros((nq, how_many)), np.zeros(nq, np.uint32)
        capi.check(capi.lib().srn_predict_batch_excl(index._h, capi.ptr(flat), capi.ptr(off), nq, capi.ptr(xf) if cap else None, capi.ptr(xo) if cap else None, cap,
                                                     int(k), int(m), int(how_many),
                                                     (capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0) | (capi.FLAG_EXCLUDE_SESSION if exclude_session else 0)
                                                     | (capi.FLAG_FILL if fill else 0),
                                                     capi.ptr(ids), capi.ptr(sc), capi.ptr(cnt)))
        return ids, sc, cnt
    if out is not None:
        ids, sc, cnt = out
        if ids.shape != (nq, how_many) or sc.shape != (nq, how_many) or cnt.shape != (nq,) or ids.dtype != np.uint64 or sc.dtype != np.float64 or cnt.dtype != np.uint32 \
                or not (ids.flags.c_contiguous and sc.flags.c_contiguous and cnt.flags.c_contiguous):
            raise ValueError("out must be (u64[nq, how_many], f64[nq, how_many], u32[nq]), C-contiguous")
    else:
        ids, sc, cnt = np.zeros((nq, how_many), np.uint64), np.zeros((nq, how_many)), np.zeros(nq, np.uint32)
    capi.check(capi.lib().srn_predict_batch(index._h, capi.ptr(flat), capi.ptr(off), nq, int(k), int(m), int(how_many),
                                            capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0,
                                            capi.ptr(ids), capi.ptr(sc), capi.ptr(cnt)))
    return ids, sc, cnt


def predict_batch_debug(index, sessions, k, m, how_many, enable_business_logic=False, neighbours=True):
    """predict_batch plus per-query stats [nq, 8] = (P, C, K, I, D, H, L, status) and, optionally, the selected
    neighbour sessions (reference session indices) with their integer similarity numerators."""
    flat, off = _flatten(sessions)
    nq = len(off) - 1
    ids, sc, cnt = np.zeros((nq, how_many), np.uint64), np.zeros((nq, how_many)), np.zeros(nq, np.uint32)
    stats = np.zeros((nq, 8), np.uint32)
    nb_s = np.zeros((nq, k), np.uint32) if neighbours else None
    nb_n = np.zeros((nq, k), np.uint32) if neighbours else None
    nb_c = np.zeros(nq, np.uint32) if neighbours else None
    capi.check(capi.lib().srn_predict_batch_debug(index._h, capi.ptr(flat), capi.ptr(off), nq, int(k), int(m), int(how_many),
                                                  capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0,
                                                  capi.ptr(ids), capi.ptr(sc), capi.ptr(cnt), capi.ptr(stats),
                                                  capi.ptr(nb_s), capi.ptr(nb_n), capi.ptr(nb_c)))
    return dict(ids=ids, scores=sc, counts=cnt, stats=stats, nb_sessions=nb_s, nb_num=nb_n, nb_counts=nb_c)


def reserve(index, nq, max_len, k, m, how_many, enable_business_logic=False, stream=0):
    """srn_index_reserve: size the workspace bound to `stream` so that predict_batch_device calls of up to nq queries allocate nothing."""
    capi.check(capi.lib().srn_index_reserve(index._h, int(nq), int(max_len), int(k), int(m), int(how_many),
                                            capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0, C.c_void_p(stream)))


def predict_batch_device(index, d_items_flat, d_q_off, nq, max_len, k, m, how_many, enable_business_logic,
                         d_out_ids, d_out_scores, d_out_counts, stream=0, resident=False):
    """Device-resident variant: arguments are raw device addresses (e.g. torch.Tensor.data_ptr()) on the
    index's GPU and a hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream); asynchronous.  resident=True (SRN_FLAG_INPUTS_RESIDENT):
    the query buffers are complete in device memory now, not pending on `stream`."""
    capi.check(capi.lib().srn_predict_batch_device(index._h, C.c_void_p(d_items_flat), C.c_void_p(d_q_off), int(nq),
                                                   int(max_len), int(k), int(m), int(how_many),
                                                   (capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0) | (capi.FLAG_INPUTS_RESIDENT if resident else 0),
                                                   C.c_void_p(d_out_ids), C.c_void_p(d_out_scores),
                                                   C.c_void_p(d_out_counts), C.c_void_p(stream)))


def predict_batch_device_excl(index, d_items_flat, d_q_off, nq, max_len, d_excl_flat, d_excl_off, max_excl, k, m, how_many, enable_business_logic,
                              d_out_ids, d_out_scores, d_out_counts, stream=0, resident=False, exclude_session=False, fill=False):
    """predict_batch_device with exclusion lists (srn_predict_batch_device_excl): d_excl_flat / d_excl_off are the device addresses of a CSR of u64 ids and nq + 1 u32
    offsets (0 with max_excl = 0), max_excl the capacity of one list -- a query with a longer list gets the count 0xFFFFFFFF; exclude_session (SRN_FLAG_EXCLUDE_SESSION):
    the items of the query's own session are excluded too; fill (SRN_FLAG_FILL): short rows are filled in place from the index's fallback ranking.  Asynchronous on `stream`."""
    capi.check(capi.lib().srn_predict_batch_device_excl(index._h, C.c_void_p(d_items_flat), C.c_void_p(d_q_off), int(nq), int(max_len),
                                                        C.c_void_p(d_excl_flat or None), C.c_void_p(d_excl_off or None), int(max_excl), int(k), int(m), int(how_many),
                                                        (capi.FLAG_BUSINESS_LOGIC if enable_business_logic else 0) | (capi.FLAG_INPUTS_RESIDENT if resident else 0)
                                                        | (capi.FLAG_EXCLUDE_SESSION if exclude_session else 0) | (capi.FLAG_FILL if fill else 0),
                                                        C.c_void_p(d_out_ids), C.c_void_p(d_out_scores), C.c_void_p(d_out_counts), C.c_void_p(stream)))
