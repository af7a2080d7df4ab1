"""Exclusion lists on the device (srn_exclude.hip): srn_predict_batch_device_excl runs the launch sequence at the internal how_many W = how_many + max_excl
(+ max_len - 1 with SRN_FLAG_EXCLUDE_SESSION) into wide rows and one wave per query drops the listed ids and compacts the row to how_many.

Every result is compared with the canonical CPU oracle's rows at W, filtered here in plain Python: counts and ids exact, scores to 1e-12; where two GPU calls are
compared, bit for bit.  The index is dense (150 items over 6 000 sessions: rows of up to ~140 candidates), plus two training sessions {A, B} of a private pair of items:
the row of [A] is [B] alone, so a list can empty it.
"""
import os

import numpy as np
import pytest

from helpers import flatten, random_queries, small_dataset

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-12
KNOBS = ("SRN_ORDER_MIN", "SRN_NO_DEDUP", "SRN_NO_FAST")
K, M, MAX_LEN = 100, 500, 6
NONE = 0xFFFFFFFF
PAIR_A, PAIR_B = 10**12 + 9_000_001, 10**12 + 9_000_002
CASES = [(21, 8), (5, 3), (1, 1), (50, 30), (60, 5)]   # W = 29, 8, 2, 80 and 65 (rows beyond one chunk of the wave; test_second_chunk_of_the_wave makes the walk reach it)


@pytest.fixture
def knobs():
    from serenade_amd import capi

    def set_(**kv):
        for name in KNOBS:
            os.environ.pop(name, None)
        for name, v in kv.items():
            if v is not None:
                os.environ[name] = str(v)
        capi.reload_knobs()
    yield set_
    for name in KNOBS:
        os.environ.pop(name, None)
    capi.reload_knobs()


@pytest.fixture(scope="module")
def dense_index():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(31, n_sessions=6000, n_items=150, max_len=12)
    off = np.concatenate([off, off[-1] + np.array([2, 4], np.uint64)])
    items = np.concatenate([items, np.array([PAIR_A, PAIR_B] * 2, np.uint64)])
    ts = np.concatenate([ts, np.array([500, 501], np.uint32)])
    gix = sa.VMISIndex.from_sessions(off, items, ts, 3000, 20, 1.0)
    oix = O.OracleIndex(off, items, ts, 3000, 20, 1.0)
    rng = np.random.default_rng(4)
    known = np.unique(items)
    flags = rng.choice(np.array([0, 1, 2, 3, 0xFF], np.uint8), size=len(known), p=[0.1, 0.05, 0.55, 0.2, 0.1])
    flags[np.searchsorted(known, [PAIR_A, PAIR_B])] = 2
    gix.set_attributes(known, flags)
    oix.set_attributes(known, flags)
    return gix, oix, ids


class _Wide:
    """The oracle's rows at some how_many for a batch, computed once per (batch, how_many, business)."""

    def __init__(self, oix, qs):
        self.oix, self.qs, self.memo = oix, qs, {}
        self.sel = np.array([i for i, q in enumerate(qs) if 1 <= len(q) <= MAX_LEN], np.int64)
        self.flat, self.off = flatten([qs[i] for i in self.sel])

    def rows(self, wide, business):
        if (wide, business) not in self.memo:
            r = self.oix.predict_batch("canonical", self.flat, self.off, K, M, wide, business, threads=4)
            ids, sc, cnt = np.zeros((len(self.qs), wide), np.uint64), np.zeros((len(self.qs), wide)), np.full(len(self.qs), NONE, np.uint32)
            ids[self.sel], sc[self.sel], cnt[self.sel] = r["ids"], r["scores"], r["counts"]
            self.memo[(wide, business)] = (ids, sc, cnt)
        return self.memo[(wide, business)]


def _expected(wide_rows, excl, cap, how_many, sessions=None):
    """Filter then cut, in plain Python: [(ids, scores)] per query, or None where the count must be 0xFFFFFFFF."""
    ids, sc, cnt = wide_rows
    out = []
    for q in range(len(cnt)):
        if cnt[q] == NONE or len(excl[q]) > cap:
            out.append(None)
            continue
        gone = set(int(x) for x in excl[q]) | (set(int(x) for x in sessions[q]) if sessions is not None else set())
        keep = [j for j in range(int(cnt[q])) if int(ids[q, j]) not in gone][:how_many]
        out.append((ids[q, keep], sc[q, keep]))
    return out


def _check(got, want, what):
    ids, sc, cnt = got
    for q, w in enumerate(want):
        if w is None:
            assert cnt[q] == NONE, "%s: query %d should be marked 0xFFFFFFFF, count %d" % (what, q, cnt[q])
            continue
        assert cnt[q] == len(w[0]), "%s: query %d has count %d, expected %d" % (what, q, cnt[q], len(w[0]))
        assert np.array_equal(ids[q, :cnt[q]], w[0]), "%s: ids of query %d differ" % (what, q)
        np.testing.assert_allclose(sc[q, :cnt[q]], w[1], rtol=SCORE_RTOL, atol=0)


def _same_rows(got, ref, what):
    ids, sc, cnt = got
    rids, rsc, rcnt = ref
    assert np.array_equal(cnt, rcnt), "%s: counts differ at %s" % (what, np.flatnonzero(cnt != rcnt)[:8])
    n = ids.shape[1]
    inside = np.arange(n)[None, :] < np.where(cnt == NONE, 0, np.minimum(cnt, n)).astype(np.int64)[:, None]
    assert np.array_equal(ids[inside], rids[inside]), "%s: ids differ" % what
    assert np.array_equal(sc[inside].view(np.uint64), rsc[inside].view(np.uint64)), "%s: scores differ in their bits" % what


class _Device:
    def __init__(self, gix, qs, excl):
        import torch
        self.torch, self.gix, self.nq = torch, gix, len(qs)
        self.flat, self.off = flatten(qs)
        self.xflat, self.xoff = flatten(excl)
        up = lambda a, t: torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(t).copy()).to("cuda:0")   # noqa: E731
        self.d_flat, self.d_off, self.d_xflat, self.d_xoff = up(self.flat, np.int64), up(self.off, np.int32), up(self.xflat, np.int64), up(self.xoff, np.int32)

    def call(self, how_many, cap, business=False, session=False, lists=True, max_len=MAX_LEN):
        import serenade_amd as sa
        t = self.torch
        ids = t.full((self.nq * how_many,), 0x5A5A5A5A5A5A5A5A, dtype=t.int64, device="cuda:0")   # outputs and counts pre-filled with garbage
        sc = t.full((self.nq * how_many,), float("nan"), dtype=t.float64, device="cuda:0")
        cnt = t.full((self.nq,), int(np.array([0x80000001], np.uint32).view(np.int32)[0]), dtype=t.int32, device="cuda:0")
        sa.predict_batch_device_excl(self.gix, self.d_flat.data_ptr(), self.d_off.data_ptr(), self.nq, max_len, self.d_xflat.data_ptr() if lists else 0,
                                     self.d_xoff.data_ptr() if lists else 0, cap, K, M, how_many, business, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(),
                                     t.cuda.current_stream().cuda_stream, exclude_session=session)
        t.cuda.synchronize()
        return ids.cpu().numpy().view(np.uint64).reshape(self.nq, how_many), sc.cpu().numpy().reshape(self.nq, how_many), cnt.cpu().numpy().view(np.uint32)


def _queries(ids):
    qs = random_queries(5, ids, 400, max_len=MAX_LEN)
    special = dict(empty=len(qs), too_long=len(qs) + 1, unknown=len(qs) + 2, pair=len(qs) + 3, exact=0, over=1)
    qs += [[], [int(x) for x in ids[:MAX_LEN + 1]], [12345], [PAIR_A]]
    return qs, special


def _lists(wide_rows, qs, special, how_many, E):
    """Per query ids of its own wide row at positions 0, how_many - 1, how_many and W - 1, a stranger and a duplicate -- rotated by the query's number and cut to E;
    every seventh list empty; one of exactly E ids, one of E + 1; the pair's whole row."""
    ids, _sc, cnt = wide_rows
    W = how_many + E
    excl = []
    for q in range(len(qs)):
        n = 0 if cnt[q] == NONE else int(cnt[q])
        kinds = [int(ids[q, p]) for p in (0, how_many - 1, how_many, W - 1) if p < n] + [777]
        kinds.append(kinds[0])
        rot = q % len(kinds)
        excl.append([] if q % 7 == 3 else (kinds[rot:] + kinds[:rot])[:E])
    first = [int(ids[special["exact"], 0])] if cnt[special["exact"]] not in (0, NONE) else []
    excl[special["exact"]] = (first + [800 + j for j in range(E)])[:E]
    excl[special["over"]] = [800 + j for j in range(E + 1)]
    excl[special["pair"]] = [PAIR_B]
    return excl


@pytest.fixture(scope="module")
def batch(dense_index):
    gix, oix, ids = dense_index
    qs, special = _queries(ids)
    return qs, special, _Wide(oix, qs)


@pytest.mark.parametrize("how_many,E", CASES)
def test_lists_against_the_oracle(dense_index, batch, knobs, how_many, E):
    gix, oix, ids = dense_index
    qs, special, wide = batch
    knobs()
    rows = wide.rows(how_many + E, False)
    excl = _lists(rows, qs, special, how_many, E)
    assert len(excl[special["exact"]]) == E and len(excl[special["over"]]) == E + 1
    got = _Device(gix, qs, excl).call(how_many, E)
    want = _expected(rows, excl, E, how_many)
    _check(got, want, "how_many %d, E %d" % (how_many, E))
    cnt = got[2]
    assert cnt[special["over"]] == NONE and cnt[special["empty"]] == NONE and cnt[special["too_long"]] == NONE
    assert cnt[special["unknown"]] == 0 and cnt[special["pair"]] == 0
    assert rows[2][special["pair"]] == 1, "the pair's row is [B] alone before the exclusion"
    bites = sum(1 for q, w in enumerate(want) if w is not None and not np.array_equal(w[0], rows[0][q, :len(w[0])]))
    print("how_many %d, E %d: the lists change %d of %d rows" % (how_many, E, bites, len(qs)))
    assert bites >= len(qs) // 3   # (position 0 or how_many - 1 leads at least three of a list's six rotations, six of seven lists are not empty, 97 % of the rows are not)


def test_second_chunk_of_the_wave(dense_index, batch, knobs):
    """how_many 60, E 5, all five ids from positions below 64 of the query's own row: after the first chunk of 64 entries only 59 are kept, so the entry at position 64
    has to be written from the second chunk, at written + rank = 59."""
    gix, oix, ids = dense_index
    qs, special, wide = batch
    how_many, E = 60, 5
    knobs()
    rows = wide.rows(how_many + E, False)
    excl = [[int(rows[0][q, p]) for p in (0, 13, 31, 47, 63)] if rows[2][q] != NONE and rows[2][q] >= 65 else [] for q in range(len(qs))]
    long_rows = [q for q in range(len(qs)) if excl[q]]
    assert len(long_rows) >= 100, "rows of 65 and more candidates: %d" % len(long_rows)
    got = _Device(gix, qs, excl).call(how_many, E)
    _check(got, _expected(rows, excl, E, how_many), "second chunk")
    for q in long_rows:
        assert got[2][q] == how_many and got[0][q, 59] == rows[0][q, 64] and got[0][q, 58] == rows[0][q, 62]


@pytest.mark.parametrize("business", [False, True])
@pytest.mark.parametrize("how_many,E", [(21, 0), (21, 8), (50, 30), (10, 70)])
def test_exclude_session(dense_index, knobs, how_many, E, business):
    """SRN_FLAG_EXCLUDE_SESSION: sessions of 1..6 items that repeat items; alone (no lists at all) and with lists; (10, 70) has lists of 70 ids -- with the session's
    items more than the 64 one pass of the wave holds."""
    gix, oix, ids = dense_index
    knobs()
    qs = random_queries(9, ids, 300, max_len=MAX_LEN, unknown_rate=0.03, dup_rate=0.4) + [[], [int(x) for x in ids[:MAX_LEN + 1]], [PAIR_A], [PAIR_B, PAIR_A]]
    W = how_many + E + MAX_LEN - 1
    rows = _Wide(oix, qs).rows(W, business)
    rng = np.random.default_rng(E)
    excl = []
    for q in range(len(qs)):
        n = 0 if rows[2][q] == NONE else int(rows[2][q])
        pick = [int(rows[0][q, p]) for p in rng.choice(n, size=min(n, E // 2), replace=False)] if n and E else []
        excl.append((pick + [900 + j for j in range(E)])[:E] if q % 5 else [])
    got = _Device(gix, qs, excl).call(how_many, E, business=business, session=True, lists=E > 0)
    _check(got, _expected(rows, excl, E, how_many, sessions=qs), "exclude_session, how_many %d, E %d, business %s" % (how_many, E, business))
    inside = [q for q in range(len(qs)) if rows[2][q] != NONE and set(qs[q][:-1]) & set(int(x) for x in rows[0][q, :min(int(rows[2][q]), how_many)])]
    print("the session's earlier items are in the top %d of %d of %d queries" % (how_many, len(inside), len(qs)))
    assert len(inside) >= 50


@pytest.mark.parametrize("how_many,E", [(21, 8), (60, 5)])
def test_same_bytes_without_the_fast_kernels(dense_index, batch, knobs, how_many, E):
    gix, oix, ids = dense_index
    qs, special, wide = batch
    excl = _lists(wide.rows(how_many + E, True), qs, special, how_many, E)
    dv = _Device(gix, qs, excl)
    knobs(SRN_NO_FAST=1)
    ref = dv.call(how_many, E, business=True)
    nq, general, _g = gix.last_path_counts()
    assert general == nq == len(qs)
    knobs()
    got = dv.call(how_many, E, business=True)
    _same_rows(got, ref, "default against SRN_NO_FAST=1")


def test_merged_copies_with_different_lists(dense_index, knobs):
    """Sorted order with dedup on: 200 copies of one session are computed once, carry three different lists and get three different rows."""
    gix, oix, ids = dense_index
    how_many, E = 21, 8
    one = [int(ids[3]), int(ids[0]), int(ids[7])]
    qs = random_queries(6, ids, 200, max_len=MAX_LEN) + [one] * 200
    rows = _Wide(oix, qs).rows(how_many + E, False)
    r = [int(x) for x in rows[0][200, :how_many + E]]
    kinds = [[r[0], r[5], r[20]], [r[1], r[2], r[3], r[4], r[21], r[28], 777, 777], []]
    excl = [[int(rows[0][q, 0])] if rows[2][q] not in (0, NONE) else [] for q in range(200)] + [kinds[q % 3] for q in range(200)]
    dv = _Device(gix, qs, excl)
    knobs(SRN_ORDER_MIN=1)
    got = dv.call(how_many, E)
    assert gix.last_dedup_count() >= 199
    _check(got, _expected(rows, excl, E, how_many), "merged copies")
    assert not np.array_equal(got[0][200], got[0][201]) and not np.array_equal(got[0][201], got[0][202]) and not np.array_equal(got[0][200], got[0][202])
    knobs(SRN_ORDER_MIN=1, SRN_NO_DEDUP=1)
    _same_rows(got, dv.call(how_many, E), "merged against SRN_NO_DEDUP=1")


def test_result_cache_at_the_internal_how_many(dense_index, batch, knobs):
    gix, oix, ids = dense_index
    qs, special, wide = batch
    how_many, E = 21, 8
    excl = _lists(wide.rows(how_many + E, False), qs, special, how_many, E)
    dv = _Device(gix, qs, excl)
    knobs()
    ref = dv.call(how_many, E)
    gix.enable_result_cache(4096, 8, K, M, how_many + E)
    try:
        first = dv.call(how_many, E)
        st1 = gix.result_cache_stats()
        second = dv.call(how_many, E)
        st2 = gix.result_cache_stats()
        assert st1["inserts"] > 0 and st2["hits"] > st1["hits"] and st2["bypassed_calls"] == 0
        _same_rows(first, ref, "first call with the cache")
        _same_rows(second, ref, "second call, served from the cache")
        # ... and other lists over the cached wide rows
        other = [x[1:] for x in excl]
        _check(_Device(gix, qs, other).call(how_many, E), _expected(wide.rows(how_many + E, False), other, E, how_many), "other lists over cached rows")
    finally:
        gix.disable_result_cache()
    gix.enable_result_cache(4096, 8, K, M, how_many)
    try:
        got = dv.call(how_many, E)
        st = gix.result_cache_stats()
        assert st["bypassed_calls"] == 1 and st["lookups"] == 0
        _same_rows(got, ref, "cache enabled at the caller's how_many: bypassed")
    finally:
        gix.disable_result_cache()


def test_host_form_equals_the_device_form(dense_index, batch, knobs):
    import serenade_amd as sa
    gix, oix, ids = dense_index
    qs, special, wide = batch
    how_many, E = 21, 8
    knobs()
    keep = [q for q in range(len(qs)) if 1 <= len(qs[q]) <= MAX_LEN]   # (the host form refuses an empty session, like srn_predict_batch)
    excl = _lists(wide.rows(how_many + E, False), qs, special, how_many, E)
    hq, hx = [qs[q] for q in keep], [excl[q] for q in keep]
    for session in (False, True):
        ref = _Device(gix, hq, hx).call(how_many, E, session=session)
        got = sa.predict_batch(gix, hq, K, M, how_many, exclude=hx, exclude_session=session, max_excl=E)
        _same_rows(got, ref, "host form (exclude_session %s)" % session)
        inside = np.arange(how_many)[None, :] < np.where(got[2] == NONE, 0, got[2]).astype(np.int64)[:, None]
        assert not got[0][~inside].any() and not got[1][~inside].any(), "the tail of a host row reads as 0"
    plain = sa.predict_batch(gix, hq, K, M, how_many)
    _same_rows(sa.predict_batch(gix, hq, K, M, how_many, exclude=[[] for _ in hq]), plain, "empty lists: the plain call")


def test_errors(dense_index, knobs):
    import serenade_amd as sa
    from serenade_amd import capi
    gix, oix, ids = dense_index
    knobs()
    dv = _Device(gix, [[int(ids[0])]] * 4, [[1]] * 4)
    with pytest.raises(sa.SerenadeError) as e:
        dv.call(500, 13)
    assert e.value.code == capi.SRN_ERANGE
    with pytest.raises(sa.SerenadeError) as e:
        dv.call(508, 0, session=True, lists=False)   # 508 + (6 - 1) > 512
    assert e.value.code == capi.SRN_ERANGE
    with pytest.raises(sa.SerenadeError) as e:
        dv.call(21, 8, lists=False)
    assert e.value.code == capi.SRN_EINVAL
    got = dv.call(512, 0, lists=False)   # nothing to exclude: the plain call, at the limit
    assert (got[2] != NONE).all()
