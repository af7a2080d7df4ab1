"""Synthetic workloads for BASELINE.json configs 2-5 -- wrapper of csrc/srn_synth.cpp."""
import ctypes as C
import os

import numpy as np

from . import build as _build

SEED = 0x5E4E4ADE
T0 = 1_500_000_000

# name -> (interactions, items, k, m, idf_weighting); m_index = m; last_items = 4; how_many = 21
CONFIGS = {
    "tiny": (200_000, 20_000, 100, 500, 1.0),          # tests / smoke
    "cfg2": (2_000_000, 100_000, 500, 1000, 1.0),      # "Synthetic 2M interactions / 100K items, k=500 m=1000"
    "cfg3": (60_000_000, 1_760_000, 1500, 2500, 2.0),  # "Synthetic 60M / 1.76M items, k=1500 m=2500 idf=2"
    "cfg4": (582_000_000, 6_500_000, 1500, 2500, 1.0),
    "cfg5": (2_300_000_000, 20_000_000, 1500, 2500, 1.0),
    "cfg5_8th": (287_500_000, 2_500_000, 1500, 2500, 1.0),   # config 5's shape at 1/8 scale: what one GPU of the 8 would see of the sessions if they were split too
}
ZIPF_ALPHA = 1.05
LAST_ITEMS = 4
HOW_MANY = 21

_lib = None


def lib():
    global _lib
    if _lib is None:
        try:
            _build.build_synth()          # no-op unless the source is newer than the .so
        except Exception:
            if not os.path.exists(_build.SYNTH_LIB):
                raise
        L = C.CDLL(_build.SYNTH_LIB)
        vp, u64 = C.c_void_p, C.c_uint64
        L.srn_synth_training.restype = vp
        L.srn_synth_training.argtypes = [u64, u64, u64, C.c_double, C.c_uint32, C.c_int]
        L.srn_synth_queries.restype = vp
        L.srn_synth_queries.argtypes = [u64, u64, u64, C.c_double, C.c_uint32, C.c_int]
        for n in ("srn_synth_n_sessions", "srn_synth_nnz", "srn_synth_n_queries", "srn_synth_q_nnz"):
            getattr(L, n).restype = u64
            getattr(L, n).argtypes = [vp]
        L.srn_synth_copy_training.argtypes = [vp, vp, vp, vp]
        L.srn_synth_copy_queries.argtypes = [vp, vp, vp]
        L.srn_synth_copy_next.argtypes = [vp, vp]
        L.srn_synth_free.argtypes = [vp]
        L.srn_synth_producer.restype = vp
        L.srn_synth_producer.argtypes = [vp, vp, vp, u64, u64, u64, C.c_double, C.c_int]
        L.srn_synth_producer_n_items.restype = u64
        L.srn_synth_producer_n_items.argtypes = [vp]
        L.srn_synth_producer_nnz.restype = u64
        L.srn_synth_producer_nnz.argtypes = [vp]
        L.srn_synth_producer_copy.argtypes = [vp, vp, vp, vp, vp]
        L.srn_synth_producer_set_idf.argtypes = [vp, vp]
        L.srn_synth_producer_free.argtypes = [vp]
        L.srn_synth_write_avro.restype = C.c_int
        L.srn_synth_write_avro.argtypes = [C.c_char_p, vp, vp, vp, vp, u64, C.c_int]
        _lib = L
    return _lib


def _threads():
    return max(1, min(32, os.cpu_count() or 1))


def training_sessions(n_interactions, n_items, seed=SEED, alpha=ZIPF_ALPHA, t0=T0):
    """-> (sess_off u64[n+1], items u64[nnz] ascending+dedup per session, max_ts u32[n] unique)."""
    L = lib()
    h = L.srn_synth_training(seed, int(n_interactions), int(n_items), float(alpha), int(t0), _threads())
    n, nnz = L.srn_synth_n_sessions(h), L.srn_synth_nnz(h)
    off, items, ts = np.empty(n + 1, np.uint64), np.empty(nnz, np.uint64), np.empty(n, np.uint32)
    L.srn_synth_copy_training(h, off.ctypes.data, items.ctypes.data, ts.ctypes.data)
    L.srn_synth_free(h)
    return off, items, ts


def queries(n_sessions, n_items, seed=SEED, alpha=ZIPF_ALPHA, max_items=LAST_ITEMS, with_next=False):
    """Evaluator-style query stream -> (items_flat u64, q_off u32[nq+1]); with_next: also next u64[nq], the held-out item that followed each prefix
    (src/bin/evaluator.rs:75 -- the item Mrr / HitRate score a recommendation list against)."""
    L = lib()
    h = L.srn_synth_queries(seed, int(n_sessions), int(n_items), float(alpha), int(max_items), _threads())
    nq, nnz = L.srn_synth_n_queries(h), L.srn_synth_q_nnz(h)
    items, off = np.empty(nnz, np.uint64), np.empty(nq + 1, np.uint32)
    L.srn_synth_copy_queries(h, items.ctypes.data, off.ctypes.data)
    nxt = None
    if with_next:
        nxt = np.empty(nq, np.uint64)
        L.srn_synth_copy_next(h, nxt.ctypes.data)
    L.srn_synth_free(h)
    return (items, off, nxt) if with_next else (items, off)


def test_sessions(n_sessions, n_items, seed=SEED, alpha=ZIPF_ALPHA):
    """The whole held-out sessions behind queries(): {session number: items in order}.  Sessions of one event give no query and are not listed.
    Rebuilt from the prefixes at a window of 255: a session starts at its one-item prefix, and every prefix's next item is its next event."""
    items, off, nxt = queries(n_sessions, n_items, seed=seed, alpha=alpha, max_items=255, with_next=True)
    lens = np.diff(off.astype(np.int64))
    starts = np.flatnonzero(lens == 1)
    ends = np.append(starts[1:], len(lens))
    first = items[off[starts].astype(np.int64)]
    return {i: [int(first[i])] + nxt[a:b].tolist() for i, (a, b) in enumerate(zip(starts, ends))}


TIE_MODES = {"ours": 0, "reverse": 1, "mixed": 2, "per-item": 3}


def tie_timestamps(ts, per_second, t0=T0):
    """The unique synthetic timestamps at a coarser clock: ~per_second sessions share each value (production data has second resolution)."""
    return (t0 + (ts.astype(np.int64) - t0) // int(per_second)).astype(np.uint32)


def avro_index(base, off, items, ts, m_index, max_len, idf_weighting, tie_mode="reverse", files=4, idf=None):
    """A stand-in for the reference's offline index producer (srn_synth.cpp): writes <base>/itemindex/*.avro + <base>/sessionindex/*.avro and returns what it
    wrote as arrays (item_ids ascending, list_off, list_sessions, idf) -- the lists AS GIVEN, for a checker.
    idf: the items' idf AS GIVEN in place of the builder's ln(total / count) * weighting -- a float64 array aligned with the returned ascending item_ids, or a callable
    item_ids -> such an array; the files and the returned idf carry it (lists, rows and tie modes are untouched).  None: the computed values."""
    L = lib()
    off, items, ts = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(items, np.uint64), np.ascontiguousarray(ts, np.uint32)
    n = len(ts)
    h = L.srn_synth_producer(off.ctypes.data, items.ctypes.data, ts.ctypes.data, n, int(m_index), int(max_len), float(idf_weighting), TIE_MODES[tie_mode])
    ni, nnz = L.srn_synth_producer_n_items(h), L.srn_synth_producer_nnz(h)
    ids, loff, lsess, idf_out = np.empty(ni, np.uint64), np.empty(ni + 1, np.uint64), np.empty(max(nnz, 1), np.uint32), np.empty(ni, np.float64)
    L.srn_synth_producer_copy(h, ids.ctypes.data, loff.ctypes.data, lsess.ctypes.data, idf_out.ctypes.data)
    try:
        if idf is not None:
            given = np.ascontiguousarray(idf(ids) if callable(idf) else idf, np.float64)
            if given.shape != (ni,):
                raise ValueError("idf must hold one value per item of the index (%d), aligned with the ascending item ids" % ni)
            L.srn_synth_producer_set_idf(h, given.ctypes.data)
            idf_out = given.copy()
        os.makedirs(os.path.join(base, "itemindex"), exist_ok=True)
        os.makedirs(os.path.join(base, "sessionindex"), exist_ok=True)
        rc = L.srn_synth_write_avro(str(base).encode(), h, off.ctypes.data, items.ctypes.data, ts.ctypes.data, n, int(files))
    finally:
        L.srn_synth_producer_free(h)
    if rc:
        raise IOError("could not write the Avro index under %s" % base)
    return ids, loff, lsess[:nnz], idf_out


def id_hash(ids, salt):
    """A fixed integer hash of item ids (splitmix64's finaliser over id + salt * golden ratio) -> u64 array."""
    x = np.asarray(ids).astype(np.uint64) + np.uint64(salt * 0x9E3779B97F4A7C15 & 0xFFFFFFFFFFFFFFFF)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def dense_rank(item_ids, list_sessions, off, items):
    """The dense index the Avro loader gives the items of avro_index()'s files (srn_avro.cpp): popularity over the rows of the sessions some list names, count
    descending, id ascending -> i64[n_items] aligned with the ascending item_ids."""
    listed = np.zeros(len(off) - 1, bool)
    listed[np.asarray(list_sessions, np.int64)] = True
    u, c = np.unique(np.asarray(items)[np.repeat(listed, np.diff(np.asarray(off).astype(np.int64)))], return_counts=True)
    if not np.array_equal(u, item_ids):
        raise ValueError("the listed sessions' rows do not hold exactly the index's items")
    r = np.empty(len(u), np.int64)
    r[np.lexsort((u, -c))] = np.arange(len(u))
    return r


IDF_PROFILES = ("near", "rising", "falling", "spike", "signs", "limits")
IDF_SERVED_MIN, IDF_SERVED_MAX = 2.0 ** -900, 2.0 ** 900           # the positive idf values the Avro loader serves (srn_avro.cpp)
IDF_SPIKES = {3: 60, 5: -60, 1030: 60, 1040: -60, 3970: 60, 3980: -60}   # dense rank -> exponent: the fast kernel's sample, its direct-mapped chunk 2, its sketch region


def idf_profile(name, item_ids, r, base):
    """idf AS GIVEN by a producer that does not follow the builder's rule, for avro_index(..., idf=): a pure function of (item id, dense rank r); base = the computed idf.
      near     B[h % 6] * (1 + s * 2^-44), B = {1, 1.5, 2, 3, 4, 6}, s hashed in +-1024: scores that share their top 32 bits and differ below
      rising   (1 + (r % 16) / 16) * 2^(-100 + 200 r / n); falling: the mirror image
      spike    1 everywhere but 2^60 / 2^-60 on the items of IDF_SPIKES
      signs    a hashed third of the items in {-3.5, -0.0, 0.0} (the un-weighted branch), the rest `base`
      limits   both ends of the range the loader serves, hashed: {2^900, 1.5 * 2^899, 2^-900, 1.5 * 2^-900, 1, base}[h % 6]"""
    item_ids, r = np.asarray(item_ids, np.uint64), np.asarray(r, np.int64)
    n = len(item_ids)
    h = id_hash(item_ids, 1)
    if name == "near":
        s = ((h >> np.uint64(8)) % np.uint64(2049)).astype(np.int64) - 1024
        return np.array([1.0, 1.5, 2.0, 3.0, 4.0, 6.0])[(h % np.uint64(6)).astype(np.int64)] * (1.0 + s * 2.0 ** -44)       # (exact: < 50 significant bits)
    if name in ("rising", "falling"):
        e = -100 + (200 * r) // n
        return np.ldexp(1.0 + (r % 16) / 16.0, (e if name == "rising" else -e).astype(np.int32))
    if name == "spike":
        out = np.ones(n)
        for rr, e in IDF_SPIKES.items():
            out[r == rr] = 2.0 ** e
        return out
    if name == "signs":
        h2 = id_hash(item_ids, 2)
        return np.where(h2 % np.uint64(3) == 0, np.array([-3.5, -0.0, 0.0])[((h2 >> np.uint64(4)) % np.uint64(3)).astype(np.int64)], np.asarray(base, np.float64))
    if name == "limits":
        vals = np.array([IDF_SERVED_MAX, 1.5 * 2.0 ** 899, IDF_SERVED_MIN, 1.5 * IDF_SERVED_MIN, 1.0, 0.0])
        return np.where(h % np.uint64(6) == 5, np.asarray(base, np.float64), vals[(h % np.uint64(6)).astype(np.int64)])
    raise KeyError(name)


def training_events(off, items, ts, seed=SEED, duplicates=0.01):
    """The sessions as click-log rows in shuffled order -> (session_ids u64, item_ids u64, times f64): a session's rows end at its timestamp, one
    second apart, about half of them on a half second (so both roundings occur); a `duplicates` fraction of rows repeats an earlier (session, item)."""
    rng = np.random.default_rng(seed)
    off = np.asarray(off, np.int64)
    lens = np.diff(off)
    sess = np.repeat(np.arange(len(lens), dtype=np.uint64) * 7 + 3, lens)
    pos = np.arange(len(items), dtype=np.int64) - np.repeat(off[:-1], lens)
    times = np.repeat(np.asarray(ts, np.float64), lens) - (np.repeat(lens, lens) - 1 - pos) + 0.5 * rng.integers(0, 2, len(items)) - 0.5
    it = np.asarray(items, np.uint64)
    dup = rng.random(len(items)) < duplicates
    sess, it, times = np.concatenate([sess, sess[dup]]), np.concatenate([it, it[dup]]), np.concatenate([times, times[dup] + 1.0])
    order = rng.permutation(len(sess))
    return sess[order], it[order], times[order]


def _digits(v, width):
    """u64 column -> (n x width) ASCII digits right-aligned, and the mask of the significant ones (at least one)."""
    out = np.empty((len(v), width), np.uint8)
    x = v.astype(np.uint64).copy()
    for c in range(width - 1, -1, -1):
        out[:, c] = (x % 10).astype(np.uint8) + 48
        x //= 10
    n = np.maximum(1, np.floor(np.log10(np.maximum(v.astype(np.float64), 1))).astype(np.int64) + 1)
    return out, np.arange(width)[None, :] >= (width - n)[:, None]


def write_training_tsv(path, session_ids, item_ids, times, bad_lines=0, seed=SEED, rows_per_block=1 << 22):
    """A training TSV ("SessionId\\tItemId\\tTime", header first) of the rows in the given order; times are written with one decimal
    (x.0 / x.5).  bad_lines unparsable lines go in at seeded positions.  Vectorised: tens of millions of rows take seconds."""
    rng = np.random.default_rng(seed)
    n = len(session_ids)
    bad_at = set(rng.integers(0, max(n, 1), bad_lines).tolist()) if bad_lines else set()
    tab, nl, dot = np.full((1, 1), 9, np.uint8), np.full((1, 1), 10, np.uint8), np.full((1, 1), 46, np.uint8)
    with open(path, "wb") as f:
        f.write(b"SessionId\tItemId\tTime\n")
        for a in range(0, n, rows_per_block):
            b = min(n, a + rows_per_block)
            t10 = np.round(np.asarray(times[a:b], np.float64) * 10).astype(np.int64)
            s, ms = _digits(np.asarray(session_ids[a:b], np.uint64), 20)
            i, mi = _digits(np.asarray(item_ids[a:b], np.uint64), 20)
            t, mt = _digits((t10 // 10).astype(np.uint64), 20)
            fr = ((t10 % 10).astype(np.uint8) + 48)[:, None]
            m = b - a
            rows = np.concatenate([s, np.repeat(tab, m, 0), i, np.repeat(tab, m, 0), t, np.repeat(dot, m, 0), fr, np.repeat(nl, m, 0)], axis=1)
            ones = np.ones((m, 1), bool)
            mask = np.concatenate([ms, ones, mi, ones, mt, ones, ones, ones], axis=1)
            cuts = sorted(x - a for x in bad_at if a <= x < b)
            if not cuts:
                f.write(rows[mask].tobytes())
                continue
            prev = 0
            for c in cuts + [m]:
                f.write(rows[prev:c][mask[prev:c]].tobytes())
                if c < m:
                    f.write(b"x%d\tnot-an-item\t1.0\n" % c)
                prev = c
