"""Short rows filled from a fallback ranking on the device (srn_fill.hip): SRN_FLAG_FILL on srn_predict_batch_device_excl / srn_predict_batch_excl.

Expected rows are the canonical CPU oracle's rows at the call's internal how_many, passed through serving.filter_rows, then through serving.fill_rows (fill_cases.expected):
counts and ids exact, model scores to 1e-12, filled scores exactly -inf; where two GPU calls are compared, bit for bit.  The index is sparse (400 sessions of up to 4 items,
505 distinct items): of 600 queries at how_many 21, 95 rows are empty, 175 short and 330 full; at how_many 100, 66 short rows hold 65..99 entries (the comparison with the
row's own ids goes into a second pass of 64).
"""
import os

import numpy as np
import pytest

from fill_cases import (K, M, MAX_LEN, NONE, Device, OracleRows, census, check_rows, draw_attrs, expected, popularity_order, same_rows, sparse_dataset, sparse_queries,
                        unfilled)

pytestmark = pytest.mark.gpu

KNOBS = ("SRN_ORDER_MIN", "SRN_NO_DEDUP", "SRN_NO_FAST")
STRANGER = 123456789   # an id the index does not know


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


class Sparse:
    pass


@pytest.fixture(scope="module")
def sparse():
    import serenade_amd as sa
    from oracle import oracle as O
    s = Sparse()
    s.off, s.items, s.ts, s.ids = sparse_dataset()
    s.gix = sa.VMISIndex.from_sessions(s.off, s.items, s.ts, 500, 20, 1.0)
    s.oix = O.OracleIndex(s.off, s.items, s.ts, 500, 20, 1.0)
    s.known, s.flags = draw_attrs(s.items)
    s.gix.set_attributes(s.known, s.flags)
    s.oix.set_attributes(s.known, s.flags)
    s.attrs = {int(i): int(f) for i, f in zip(s.known, s.flags)}
    s.order = popularity_order(s.items)
    s.qs = sparse_queries(s.ids)
    s.orows = OracleRows(s.oix, s.qs)
    s.dev = Device(s.gix, s.qs)
    assert len(s.gix.fallback()) == 0
    s.before = {h: s.dev.call(h, fill=False) for h in (21, 100)}   # the rows of the calls before any ranking was set
    yield s
    s.gix.close()


def ranking_of(s, R):
    return [int(x) for x in s.order[:R]]


def test_popular_ranking_is_the_numpy_order(sparse, tmp_path):
    import serenade_amd as sa
    s = sparse
    s.gix.set_fallback_popular(256)
    assert np.array_equal(s.gix.fallback(), s.order[:256])
    counts = dict(zip(*[a.tolist() for a in np.unique(s.items, return_counts=True)]))
    assert counts[int(s.order[64])] == 2 and counts[int(s.order[128])] == 2, "the counts tie: the id decides"
    s.gix.set_fallback_popular(10**6)
    assert np.array_equal(s.gix.fallback(), s.order), "min(n, n_items) entries"
    s.gix.set_fallback_popular(256)
    path = str(tmp_path / "sparse.idx")
    s.gix.save(path)
    back = sa.VMISIndex.load(path)
    try:
        assert len(back.fallback()) == 0, "the file does not carry the ranking"
        back.set_fallback_popular(256)
        assert np.array_equal(back.fallback(), s.order[:256])
        back.set_attributes(s.known, s.flags)
        same_rows(Device(back, s.qs).call(21), s.dev.call(21), "the loaded index against the built one")
    finally:
        back.close()


@pytest.mark.parametrize("how_many", [21, 100])
def test_fill_against_the_oracle(sparse, knobs, how_many):
    s = sparse
    knobs()
    s.gix.set_fallback_popular(256)
    plain = s.orows.rows(how_many)[2]
    empty, short, full = census(plain, how_many)
    print("how_many %d: %d empty, %d short, %d full rows" % (how_many, empty, short, full))
    if how_many == 21:
        assert (empty, short, full) == (95, 175, 330) and min(empty, short, full) >= 50
    else:
        assert (empty, short, full) == (95, 365, 140)
        assert int(((plain > 64) & (plain < 100)).sum()) >= 30
    got = s.dev.call(how_many)
    check_rows(got, expected(s.orows, how_many, ranking_of(s, 256)), "how_many %d" % how_many)
    assert (got[2] == how_many).all(), "a ranking of 256 fills every row"
    short_rows = plain < how_many
    assert np.isneginf(got[1][short_rows, -1]).all() and not np.isneginf(got[1][~short_rows]).any()


def test_second_chunk_of_the_ranking_and_a_ranking_that_runs_out(sparse, knobs):
    s = sparse
    knobs()
    how_many = 70
    plain = s.orows.rows(how_many)[2]
    empty = np.flatnonzero(plain == 0)
    assert len(empty) == 95
    s.gix.set_fallback_popular(256)
    got = s.dev.call(how_many)
    check_rows(got, expected(s.orows, how_many, ranking_of(s, 256)), "how_many 70")
    assert (got[2][empty] == how_many).all()
    for q in empty:   # 70 entries of the ranking without the session's most recent item: the last one is entry 69 or 70, from the second chunk of 64
        assert int(got[0][q, -1]) == int(s.order[70 if s.qs[q][-1] in ranking_of(s, 70) else 69])
    s.gix.set_fallback_popular(16)
    got = s.dev.call(how_many)
    want = expected(s.orows, how_many, ranking_of(s, 16))
    check_rows(got, want, "a ranking of 16")
    assert (got[2][empty] <= 16).all() and (got[2][empty] == 16).sum() >= 50 and (got[2] < how_many).sum() >= 95
    s.gix.set_fallback_popular(256)


def test_full_rows_and_calls_without_the_flag_are_untouched(sparse, knobs):
    s = sparse
    knobs()
    s.gix.set_fallback_popular(256)
    for how_many in (21, 100):
        ref = s.before[how_many]
        off = s.dev.call(how_many, fill=False)
        for a, b in zip(off, ref):   # every byte of the buffers, the garbage beyond the counts included
            assert np.array_equal(a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32), b.view(np.uint64 if b.dtype.itemsize == 8 else np.uint32)), \
                "how_many %d: a call without the flag differs from the call before any ranking was set" % how_many
        on = s.dev.call(how_many)
        full = ref[2] >= how_many
        assert full.sum() >= 100
        assert np.array_equal(on[0][full], ref[0][full]) and np.array_equal(on[1][full].view(np.uint64), ref[1][full].view(np.uint64)) and np.array_equal(on[2][full], ref[2][full])
        short = ~full
        c = ref[2][short].astype(np.int64)
        inside = np.arange(how_many)[None, :] < c[:, None]
        assert np.array_equal(on[0][short][inside], ref[0][short][inside]) and np.array_equal(on[1][short][inside].view(np.uint64), ref[1][short][inside].view(np.uint64)), \
            "the model entries of a filled row are untouched"


def test_unserved_queries_pass_through(sparse, knobs):
    s = sparse
    knobs()
    s.gix.set_fallback_popular(256)
    qs = s.qs[:60] + [[], [int(x) for x in s.ids[:MAX_LEN + 1]], [STRANGER]]
    cap = 4
    excl = [[int(s.order[j]) for j in range(q % (cap + 1))] for q in range(len(qs))]
    over = 7
    excl[over] = [int(s.order[j]) for j in range(cap + 1)]
    orows = OracleRows(s.oix, qs)
    for how_many in (21, 100):
        got = Device(s.gix, qs, excl).call(how_many, cap=cap)
        check_rows(got, expected(orows, how_many, ranking_of(s, 256), excl=excl, cap=cap), "unserved, how_many %d" % how_many)
        assert got[2][60] == NONE and got[2][61] == NONE and got[2][over] == NONE
        assert got[2][62] == how_many and not set(int(x) for x in got[0][62]) & set(excl[62])
    got = Device(s.gix, qs).call(21)   # ... and in place, without lists
    check_rows(got, expected(orows, 21, ranking_of(s, 256)), "unserved, in place")
    assert got[2][60] == NONE and got[2][61] == NONE and got[2][62] == 21


def test_lists_and_sessions_made_of_the_head_of_the_ranking(sparse, knobs):
    s = sparse
    knobs()
    newcomer = STRANGER + 1000   # a product the index does not know leads the ranking
    ranking = [newcomer] + ranking_of(s, 255)
    s.gix.set_fallback(ranking)
    rng = np.random.default_rng(11)
    head = ranking[:12]
    qs = [[head[j] for j in rng.choice(12, size=int(rng.integers(2, MAX_LEN + 1)), replace=False)] for _ in range(120)]
    qs += [q[:-1] + [STRANGER + i] for i, q in enumerate(qs[:60])]   # the same with an unknown most recent item: fewer candidates, no attributes of r
    alone = list(range(len(qs), len(qs) + 12))
    qs += [[newcomer, STRANGER + 500 + i] for i in range(12)]   # nothing the index knows: an empty row for certain, and no neighbour that could make the newcomer a candidate
    cap, how_many = 8, 100
    excl = [[head[(q + j) % 12] for j in range(q % (cap + 1))] if q < alone[0] else [] for q in range(len(qs))]
    orows = OracleRows(s.oix, qs)
    dv = Device(s.gix, qs, excl)
    got = dv.call(how_many, cap=cap, session=True)
    check_rows(got, expected(orows, how_many, ranking, excl=excl, cap=cap, session=True), "lists and sessions of the head, SRN_FLAG_EXCLUDE_SESSION")
    # the oracle's census, so that the test cannot pass on nothing: 72 of the 180 rows are short before the fill (the head items have rows of 100 and more candidates)
    short_before = unfilled(orows, how_many, excl, cap, session=True)[2] < how_many
    assert short_before.sum() >= 50, short_before.sum()
    assert (got[2] == how_many).all() and np.array_equal(np.isneginf(got[1][:, -1]), short_before), "exactly the rows that were short end in a filled entry"
    for q in range(len(qs)):
        assert not set(int(x) for x in got[0][q]) & (set(excl[q]) | set(qs[q])), "query %d: a listed id or an item of the session came back" % q
    got = dv.call(how_many, cap=cap)
    want = expected(orows, how_many, ranking, excl=excl, cap=cap)
    check_rows(got, want, "lists and sessions of the head, without the flag")
    filled_older = sum(bool(set(int(x) for x in want[0][q][np.isneginf(want[1][q])]) & set(qs[q][:-1])) for q in range(len(qs)))
    assert filled_older >= 12, "rows of the expected result in which the FILL brings an older item of the session back: %d" % filled_older
    older = 0
    for q in range(len(qs)):
        row = set(int(x) for x in got[0][q])
        assert qs[q][-1] not in row and not row & set(excl[q])
        older += bool(row & (set(qs[q][:-1]) - set(excl[q]) - {qs[q][-1]}))
    assert older >= filled_older, "an older item of the session that is in the ranking may come back: %d rows" % older
    assert all(int(got[0][q, 0]) == newcomer and np.isneginf(got[1][q, 0]) for q in alone), "an empty row without the flag starts with the session's older item, the head of the ranking"
    s.gix.set_fallback_popular(256)


def test_business_rules(sparse, knobs):
    s = sparse
    knobs()
    o = [int(x) for x in s.order[:80]]
    not_for_sale, no_attrs, adult, adult_not_for_sale, plain_item, adult_r = o[1], o[2], o[3], o[4], o[0], o[10]
    ranking = [plain_item, STRANGER] + o[1:63]
    assert len(ranking) == 64
    attrs = dict(s.attrs)

    def set_attrs(pairs):
        ids, fl = np.array([p[0] for p in pairs], np.uint64), np.array([p[1] for p in pairs], np.uint8)
        s.gix.set_attributes(ids, fl)
        s.oix.set_attributes(ids, fl)
        attrs.update({int(i): int(f) for i, f in pairs})

    qs = [[adult_r], [o[20], adult_r], [plain_item], [o[21], plain_item], [STRANGER + 1], [o[22], STRANGER + 2], [no_attrs], [adult]] + s.qs[:100]
    dv = Device(s.gix, qs)
    try:
        set_attrs([(plain_item, 2), (not_for_sale, 0), (no_attrs, 0xFF), (adult, 3), (adult_not_for_sale, 1), (adult_r, 3), (o[20], 2), (o[21], 2), (o[22], 2)])
        s.gix.set_fallback(ranking)
        for round_ in range(2):
            orows = OracleRows(s.oix, qs)
            for how_many in (21, 100):
                got = dv.call(how_many)
                check_rows(got, expected(orows, how_many, ranking, attrs=attrs), "round %d, without the business rules" % round_)
                assert STRANGER in got[0][4], "without the business rules the unknown id is filled in"
                got = dv.call(how_many, business=True)
                check_rows(got, expected(orows, how_many, ranking, business=True, attrs=attrs), "round %d, business rules, how_many %d" % (round_, how_many))
                rows = [set(int(x) for x in got[0][q, :got[2][q]]) for q in range(8)]
                for q in range(8):
                    assert STRANGER not in rows[q] and no_attrs not in rows[q]
                if how_many != 100:   # (at 100 every one of these rows is short and takes the whole ranking that passes)
                    continue
                assert all(np.isneginf(got[1][q, got[2][q] - 1]) for q in range(8))
                if round_ == 0:
                    assert all(not_for_sale not in r and adult_not_for_sale not in r for r in rows)
                    assert adult in rows[0] and adult in rows[1], "an adult r takes adult items"
                    assert all(adult not in rows[q] for q in (2, 3, 4, 5, 6)), "a non-adult, an unknown and an attribute-less r take none"
                else:
                    assert all(adult not in r for r in rows) and not_for_sale in rows[2] and adult_not_for_sale not in rows[2]
                    assert adult_r in rows[2] and adult_r in rows[4], "no longer adult: passes for every r"
            # the flags flip: the ranking stays, the attributes are read at call time
            set_attrs([(not_for_sale, 2), (adult, 1), (adult_r, 2)])
    finally:
        s.gix.set_attributes(s.known, s.flags)
        s.oix.set_attributes(s.known, s.flags)
        s.gix.set_fallback_popular(256)


def test_errors(sparse, knobs):
    import serenade_amd as sa
    from serenade_amd import capi
    s = sparse
    knobs()
    s.gix.clear_fallback()
    assert len(s.gix.fallback()) == 0
    try:
        with pytest.raises(sa.SerenadeError) as e:
            s.dev.call(21)
        assert e.value.code == capi.SRN_ESTATE
        with pytest.raises(sa.SerenadeError) as e:
            sa.predict_batch(s.gix, s.qs[:8], K, M, 21, fill=True)
        assert e.value.code == capi.SRN_ESTATE
        same_rows(s.dev.call(21, fill=False), s.before[21], "without the flag no ranking is needed")
        for bad, code in (([5, 6, 5], capi.SRN_EINVAL), ([], capi.SRN_EINVAL), (list(range(1, capi.MAX_FALLBACK + 2)), capi.SRN_ERANGE)):
            with pytest.raises(sa.SerenadeError) as e:
                s.gix.set_fallback(bad)
            assert e.value.code == code, (len(bad), e.value)
            assert len(s.gix.fallback()) == 0
        s.gix.set_fallback(list(range(1, capi.MAX_FALLBACK + 1)))   # SRN_MAX_FALLBACK ids the index does not know: a legitimate ranking
        got = s.dev.call(21)
        assert (got[2] == 21).all() and int(got[0][np.flatnonzero(s.before[21][2] == 0)[0], 0]) == 1
        flat, off = np.array([int(s.order[0])], np.uint64), np.array([0, 1], np.uint32)
        ids, sc, cnt = np.zeros(21, np.uint64), np.zeros(21), np.zeros(1, np.uint32)
        with pytest.raises(sa.SerenadeError) as e:   # flags the entry points never knew stay unknown
            capi.check(capi.lib().srn_predict_batch_excl(s.gix._h, capi.ptr(flat), capi.ptr(off), 1, None, None, 0, K, M, 21, 32, capi.ptr(ids), capi.ptr(sc), capi.ptr(cnt)))
        assert e.value.code == capi.SRN_EINVAL
    finally:
        s.gix.set_fallback_popular(256)


@pytest.mark.parametrize("nq", [1, 3, 5])
def test_the_tail_of_a_workgroup(sparse, knobs, nq):
    s = sparse
    knobs()
    s.gix.set_fallback_popular(256)
    plain = s.before[21][2]
    kinds = [np.flatnonzero(plain == 0)[0], np.flatnonzero((plain > 0) & (plain < 21))[0], np.flatnonzero(plain >= 21)[0], np.flatnonzero((plain > 0) & (plain < 21))[1],
             np.flatnonzero(plain == 0)[1]]
    pick = [int(q) for q in kinds[:nq]]
    whole = s.dev.call(21)
    got = Device(s.gix, [s.qs[q] for q in pick]).call(21)
    same_rows(got, tuple(a[pick] for a in whole), "%d queries against the same queries inside the batch of 600" % nq)
    assert (got[2] == 21).all()


CAP = 8


def lists_of(s):
    return [[int(s.order[(q + j) % 20]) for j in range(q % (CAP + 1))] for q in range(len(s.qs))]


@pytest.mark.parametrize("how_many", [21, 100])
def test_knobs(sparse, knobs, how_many):
    s = sparse
    s.gix.set_fallback_popular(256)
    cap, excl = CAP, lists_of(s)
    dv = Device(s.gix, s.qs, excl)
    knobs()
    ref = dv.call(how_many, cap=cap)
    check_rows(ref, expected(s.orows, how_many, ranking_of(s, 256), excl=excl, cap=cap), "lists, how_many %d" % how_many)
    plain = s.dev.call(how_many)
    for kv in (dict(SRN_NO_FAST=1), dict(SRN_NO_DEDUP=1), dict(SRN_ORDER_MIN=0), dict(SRN_ORDER_MIN=1), dict(SRN_ORDER_MIN=1, SRN_NO_DEDUP=1)):
        knobs(**kv)
        same_rows(dv.call(how_many, cap=cap), ref, "%s against the defaults" % kv)
        same_rows(s.dev.call(how_many), plain, "%s against the defaults, in place" % kv)


def test_merged_copies_with_different_lists(sparse, knobs):
    """Copies of one short-row session, merged within the call (sorted order, dedup on), carry different lists: the fill runs per query behind the merge."""
    s = sparse
    s.gix.set_fallback_popular(256)
    cap, how_many = CAP, 21
    knobs(SRN_ORDER_MIN=1)
    short = int(np.flatnonzero((s.before[21][2] > 0) & (s.before[21][2] < 21))[0])
    qs = s.qs[:100] + [s.qs[short]] * 100
    xs = [[] for _ in range(100)] + [[int(s.order[j]) for j in range(q % 3)] for q in range(100)]
    got = Device(s.gix, qs, xs).call(how_many, cap=cap)
    assert s.gix.last_dedup_count() >= 99
    check_rows(got, expected(OracleRows(s.oix, qs), how_many, ranking_of(s, 256), excl=xs, cap=cap), "merged copies")
    assert not np.array_equal(got[0][100], got[0][101]) and not np.array_equal(got[0][101], got[0][102])


def test_result_cache_at_the_internal_how_many(sparse, knobs):
    """The cache keeps the unfilled rows: a cold and a warm call give the same filled rows, and a new ranking does not clear it."""
    s = sparse
    s.gix.set_fallback_popular(256)
    cap, how_many, excl = CAP, 21, lists_of(s)
    dv = Device(s.gix, s.qs, excl)
    knobs()
    ref = dv.call(how_many, cap=cap)
    s.gix.enable_result_cache(4096, 8, K, M, how_many + cap)
    try:
        cold = dv.call(how_many, cap=cap)
        st1 = s.gix.result_cache_stats()
        warm = dv.call(how_many, cap=cap)
        st2 = s.gix.result_cache_stats()
        same_rows(cold, ref, "cold call with the cache")
        same_rows(warm, ref, "warm call, served from the cache")
        assert st1["inserts"] > 0 and st2["hits"] > st1["hits"] and st2["bypassed_calls"] == 0
        assert (st2["how_many"], st2["k"], st2["m"]) == (how_many + cap, K, M)
        s.gix.set_fallback_popular(16)   # a new ranking does not clear the cache: the cached rows are the unfilled ones
        st3 = s.gix.result_cache_stats()
        assert st3["clears"] == st2["clears"] and st3["inserts"] == st2["inserts"]
        other = dv.call(how_many, cap=cap)
        st4 = s.gix.result_cache_stats()
        assert st4["hits"] > st3["hits"] and st4["inserts"] == st3["inserts"]
        check_rows(other, expected(s.orows, how_many, ranking_of(s, 16), excl=excl, cap=cap), "another ranking over the cached rows")
        nofill = dv.call(how_many, cap=cap, fill=False)
        check_rows(nofill, unfilled(s.orows, how_many, excl, cap), "the cached rows are the unfilled ones")
    finally:
        s.gix.disable_result_cache()
        s.gix.set_fallback_popular(256)


def test_host_form_equals_the_device_form(sparse, knobs):
    import serenade_amd as sa
    s = sparse
    knobs()
    s.gix.set_fallback_popular(256)
    cap, excl = CAP, lists_of(s)
    for how_many in (21, 100):
        same_rows(sa.predict_batch(s.gix, s.qs, K, M, how_many, fill=True), s.dev.call(how_many), "host form, no lists")
        for session in (False, True):
            ref = Device(s.gix, s.qs, excl).call(how_many, cap=cap, session=session)
            got = sa.predict_batch(s.gix, s.qs, K, M, how_many, exclude=excl, exclude_session=session, max_excl=cap, fill=True)
            same_rows(got, ref, "host form (exclude_session %s)" % session)
    s.gix.set_fallback_popular(16)
    try:
        got = sa.predict_batch(s.gix, s.qs, K, M, 70, fill=True)
        inside = np.arange(70)[None, :] < got[2].astype(np.int64)[:, None]
        assert (~inside).any() and not got[0][~inside].any() and not got[1][~inside].any(), "the tail of a host row that stays short reads as 0"
        plain = sa.predict_batch(s.gix, s.qs, K, M, 70)
        same_rows(plain, s.dev.call(70, fill=False), "the plain host call, ranking set")
    finally:
        s.gix.set_fallback_popular(256)
