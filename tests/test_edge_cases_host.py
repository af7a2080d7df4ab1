"""The designed index of tests/edge_cases.py on the CPU: the condition that keeps tests/test_gpu_edge_cases.py from passing vacuously.

(a) The census: every edge the module lists is hit, on both sides, by at least one (query, call shape) pair -- asserted edge by edge from the NumPy restatement, for both
    timestamp variants; a cell whose sessions miss its designed (len, kept) fails here.
(b) The restatement against the oracle: posting-list lengths, neighbors_canonical's K and (session, numerator) sets, and the counters P, C, K, I, D, H, L of
    predict_batch(..., want_stats=True), for every query at both call shapes.
(c) The oracle's rows for every 8th query against helpers.canonical_acc_over_given_lists with exact Fraction scores (as tests/test_gpu_given_idf.py does for its index).
(d) The tied variant: the designed counts are those of the distinct variant, and tie groups straddle x_lo and the k-cut's boundary (part of its census).
(e) edge_cases.wide_ids: a strictly increasing injection with two non-zero, different halves, under which the oracle's rows map id for id with the same score bits.
(f) The census of the persistent latency path: the single calls of tests/test_gpu_persistent_edges.py hold every kind of answer a resident form gives, on both sides of
    every edge (lengths 1..4 / 5, 6, 10; hand-overs; the row of 64 against 65 entries at the cut), and the designed interleave has the adjacencies it promises."""
from fractions import Fraction

import numpy as np
import pytest

import edge_cases as E
from helpers import canonical_acc_over_given_lists, flatten

HOW_MANY = 21
VARIANTS = [False, True]
IDS = ["distinct", "tied"]


@pytest.fixture(scope="module")
def oracles():
    from oracle import oracle as O
    out = {}
    for tied in VARIANTS:
        ix = E.build(tied)
        oix = O.OracleIndex(ix.off, ix.items, ix.ts, E.M_INDEX, E.ROW_MAX, 1.0, fast=True)
        flat, off = flatten(ix.queries)
        rows = [oix.predict_batch("canonical", flat, off, k, m, HOW_MANY, False, threads=4, want_stats=True) for k, m in E.SHAPES]
        out[tied] = (ix, oix, rows)
    return out


@pytest.mark.parametrize("tied", VARIANTS, ids=IDS)
def test_census_every_edge_on_both_sides(tied):
    ix = E.build(tied)
    hits = E.census(tied)
    n_sessions, nnz = len(ix.ts), len(ix.items)
    print("%d cells, %d sessions, %d interactions, %d queries; %d edges, the rarest hit %d times" % (len(ix.cells), n_sessions, nnz, len(ix.queries), len(hits), min(hits.values())))
    for name, c in hits.items():
        print("%5d  %s" % (c, name))
    assert n_sessions <= 260000 and nnz <= 1250000, "the index has outgrown its budget"
    assert len(ix.queries) > 256, "a host call of <= 256 sessions takes the latency path, not the launch sequence"
    assert (np.diff(ix.ts.astype(np.int64)) >= 0).all() and (tied or (np.diff(ix.ts.astype(np.int64)) > 0).all())
    for sh in (0, 1):
        print("routes at (k, m) = %s: %s" % (E.SHAPES[sh], E.route_counts(tied, sh)))
    # the derived edges are the ones the kernels' constants give
    assert (E.N_LEAN, E.N_MID, E.N_BIG, E.N_LONG, E.N_FUSED) == (6012, 5884, 9404, 7548, 3072)


@pytest.mark.parametrize("tied", VARIANTS, ids=IDS)
def test_restatement_equals_the_oracle(oracles, tied):
    ix, oix, rows = oracles[tied]
    for q in ix.queries:   # posting-list lengths
        for it in dict.fromkeys(q):
            sessions, _idf = oix.postings(it, cap=E.M_INDEX)
            mine = E._list_of(ix, it)
            assert (sessions is None) == (mine is None), it
            if mine is not None:
                assert np.array_equal(sessions.astype(np.int64), mine), it
    for sh, (k, m) in enumerate(E.SHAPES):
        R = E.restate(tied, sh)
        st = rows[sh]["stats"].astype(np.int64)
        for qi, (q, r) in enumerate(zip(ix.queries, R)):
            sid, num, U = oix.neighbors_canonical(q, k, m)
            assert len(sid) == r["K"] and U == r["U"] and sorted(zip(sid.tolist(), num.tolist())) == r["nb"], (qi, ix.cells[ix.q_cell[qi]]["name"], k, m)
            want = [r["P"], r["C"], r["K"], r["I"], r["D"], min(HOW_MANY, r["E"]), r["L"]]
            assert st[qi].tolist() == want, (qi, ix.cells[ix.q_cell[qi]]["name"], k, m, st[qi].tolist(), want)
            assert int(rows[sh]["counts"][qi]) == min(HOW_MANY, r["E"])


class _Rows:
    """rows[s] of the pure-Python canonical form: the session's items as a set, made when asked for."""

    def __init__(self, ix):
        self.ix, self.off = ix, ix.off.astype(np.int64)

    def __getitem__(self, s):
        return set(self.ix.items[self.off[s]:self.off[s + 1]].tolist())


@pytest.mark.parametrize("tied", VARIANTS, ids=IDS)
def test_oracle_rows_against_exact_fractions(oracles, tied):
    """Every 8th query at both shapes: acc and U from the pure-Python canonical form over the lists as given, score = Fraction(idf) * acc / (10 U) exactly.  The oracle's
    rows hold the doubles of `one multiply, one divide` bit for bit and their order never contradicts the exact one: a pair may stand inverted only where its two ROUNDED
    scores are equal (then the id decides)."""
    ix, oix, rows = oracles[tied]
    view = _Rows(ix)
    for sh, (k, m) in enumerate(E.SHAPES):
        ref = rows[sh]
        for qi in range(0, len(ix.queries), 8):
            q = ix.queries[qi]
            lists = {it: E._list_of(ix, it).tolist() for it in dict.fromkeys(q) if E._list_of(ix, it) is not None}
            acc, U = canonical_acc_over_given_lists(lists, view, ix.ts, q, k, m)
            idf = {}
            for it in acc:
                v = oix.postings(it, cap=E.M_INDEX)[1]
                idf[it] = v if v > 0 else 1.0
            exact = {it: Fraction(idf[it]) * a / (10 * U) for it, a in acc.items()}
            rounded = {it: idf[it] * float(a) / float(10 * U) for it, a in acc.items()}
            c = int(ref["counts"][qi])
            got = ref["ids"][qi, :c].tolist()
            assert c == min(HOW_MANY, len(acc)) and len(set(got)) == c and all(it in acc for it in got), (qi, q)
            assert all(np.float64(rounded[it]).tobytes() == ref["scores"][qi, j].tobytes() for j, it in enumerate(got)), (qi, q)
            for a, b in zip(got[:-1], got[1:]):
                assert exact[a] >= exact[b] or rounded[a] == rounded[b], (qi, a, b)
                assert rounded[a] > rounded[b] or (rounded[a] == rounded[b] and a < b), (qi, a, b)
            if c:
                last = got[-1]
                for it in set(acc) - set(got):
                    assert exact[it] <= exact[last] or rounded[it] == rounded[last], (qi, it, last)
                    assert rounded[it] < rounded[last] or (rounded[it] == rounded[last] and it > last), (qi, it, last)


def test_tied_variant_has_the_designed_counts():
    """Collapsing the timestamps in groups of 8 changes no (timestamp, session index) order: the same rows, the same ranks, the same restated quantities; the tie groups
    across x_lo and across the k-cut's boundary are edges of the tied census (test_census_every_edge_on_both_sides[tied])."""
    a, b = E.build(False), E.build(True)
    assert np.array_equal(a.off, b.off) and np.array_equal(a.items, b.items) and a.queries == b.queries
    assert len(np.unique(b.ts)) == (len(b.ts) + 7) // 8 and np.array_equal(a.rank, b.rank)
    for sh in (0, 1):
        for ra, rb in zip(E.restate(False, sh), E.restate(True, sh)):
            for key in ("len", "kept", "xlo", "n", "nr", "sumw", "C", "K", "nb", "E", "route", "P", "I", "D"):
                assert ra[key] == rb[key], key


def test_wide_ids_are_an_increasing_injection_and_the_oracle_commutes_with_them(oracles):
    """edge_cases.wide_ids over every id of the designed index and its batch: strictly increasing, both 32-bit halves non-zero and different, hi ^ lo different between
    neighbours (the persistent path's check word xors the halves: equal halves would cancel).  And what the GPU tests rely on instead of a second oracle run per world:
    the oracle on the MAPPED index answers the mapped batch with the narrow index's rows, ids mapped, counts equal, scores the same bits -- one variant, one shape."""
    from oracle import oracle as O
    ix, _oix, rows = oracles[True]
    ids = E.designed_ids(ix)
    wide = E.wide_ids(ids)
    hi, lo = (wide >> np.uint64(32)).astype(np.int64), (wide & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (np.diff(ids.astype(np.int64)) > 0).all() and (wide[1:] > wide[:-1]).all(), "strictly increasing"
    assert (hi != 0).all() and (lo != 0).all() and (hi != lo).all() and int(wide.max()) < 2**63
    assert (np.diff(hi ^ lo) != 0).all(), "hi ^ lo repeats between neighbours"
    assert len(np.unique(hi)) < len(hi) // 4 and len(np.unique(lo)) == len(lo), "ids 7 apart share a high half: the low half alone tells them apart"
    assert E.wide_ids([0])[0] == 0
    sh = 1
    k, m = E.SHAPES[sh]
    wix = O.OracleIndex(ix.off, E.wide_ids(ix.items), ix.ts, E.M_INDEX, E.ROW_MAX, 1.0, fast=True)
    flat, off = flatten(ix.queries)
    got = wix.predict_batch("canonical", E.wide_ids(flat), off, k, m, HOW_MANY, False, threads=4)
    ref = rows[sh]
    inside = np.arange(HOW_MANY)[None, :] < ref["counts"][:, None].astype(np.int64)
    assert np.array_equal(got["counts"], ref["counts"]) and inside.sum() > 5000
    assert np.array_equal(got["ids"][inside], E.wide_ids(ref["ids"])[inside])
    assert np.array_equal(got["scores"][inside].view(np.uint64), ref["scores"][inside].view(np.uint64))


@pytest.mark.parametrize("tied", VARIANTS, ids=IDS)
def test_census_of_the_persistent_path(tied):
    """What keeps tests/test_gpu_persistent_edges.py from passing vacuously: the single calls it posts (edge_cases.serve_calls) hold, at BOTH shapes, every kind of answer the
    resident forms can give, on both sides of every edge, and the designed interleave has the adjacencies its docstring promises."""
    ix = E.build(tied)
    attrs = E.business_attrs(ix)
    for sh, (k, m) in enumerate(E.SHAPES):
        calls = E.serve_calls(tied, sh)
        assert len(calls) >= 120 and all(1 <= c["r"]["L"] <= 10 for c in calls)
        # the routing half of the predicate: with L <= 4 on the lean form and 5..10 on the other one, a resident form keeps exactly what the launch sequence routes lean / mid
        for c in calls:
            assert (E.resident_route(c["r"]) in ("lean", "mid")) == (c["r"]["route"] in ("lean", "mid")), c["name"]
        for how_many, at, what in ((21, None, "default"), (64, None, "how_many 64"), (21, attrs, "business rules")):
            kinds = [E.resident_kind(ix, c["r"], how_many, at) for c in calls]
            count = {kd: kinds.count(kd) for kd in set(kinds)}
            print("%s, (k, m) = (%d, %d), %s: %d calls, %s" % ("tied" if tied else "distinct", k, m, what, len(calls), count))
            served = [c for c, kd in zip(calls, kinds) if kd == "served"]
            for L in (1, 2, 3, 4):
                assert any(c["r"]["L"] == L and c["r"]["route"] == "lean" and c["r"]["n"] > 0 for c in served), "no served lean query of %d items" % L
            for L in (5, 6, 10):   # (5: one control line, five items; 6: the second line's first item; 10: max_items)
                assert any(c["r"]["L"] == L and c["r"]["n"] > 0 for c in served), "no served query of %d items on the form for 5..10" % L
            assert count.get("general", 0) >= 1, "no query that a resident form hands to the general kernel"
            # the lean form's oversized route needs n > 6 012 from at most four lists of at most m entries: out of reach at m = 1 100, placed at m = 2 560
            assert (count.get("big", 0) >= 1) == (sh == 1) and (sh == 1 or 4 * m < E.N_LEAN)
            assert any(c["r"]["L"] > 4 for c, kd in zip(calls, kinds) if kd == "general"), "nothing that the form for 5..10 items hands over"
            assert sh == 0 or any(c["r"]["L"] <= 4 for c, kd in zip(calls, kinds) if kd == "general"), "nothing that the lean form hands to the general kernel"
            # a row of count 0 (no known item: the count is written at once, status 0), on both forms
            assert any(c["r"]["n"] == 0 and c["r"]["E"] == 0 and c["r"]["L"] == 1 for c in served) and any(c["r"]["n"] == 0 and c["r"]["L"] > 5 for c in served)
            # the row edge: T = tight_set, served iff T <= 64.  E <= 63 bounds T whatever the scores are
            by_E = {c["r"]["E"]: (c, kd) for c, kd in zip(calls, kinds) if c["name"].startswith("rows E=")}
            T = {e: E.tight_set(ix, by_E[e][0]["r"], how_many, at) for e in (63, 64, 65)}
            for c, kd in zip(calls, kinds):
                if kd in ("served", "over64") and c["r"]["E"] <= 63:
                    assert kd == "served" and E.tight_set(ix, c["r"], how_many, at) <= c["r"]["E"]
            if how_many == 64:      # the edge is live: 63 and 64 entries at the cut are finished in place, 65 are not
                assert (T[63], T[64], T[65]) == (63, 64, 65) and [by_E[e][1] for e in (63, 64, 65)] == ["served", "served", "over64"]
            else:                   # how_many-th best + ties: far fewer than the rows' scored items -- rows of 64 and 65 items ARE served (not `E <= 63`)
                assert all(how_many <= T[e] <= E.SERVE_MAX_ENTRIES and by_E[e][1] == "served" for e in (63, 64, 65)), T
                assert sum(1 for c in served if c["r"]["E"] > 63) >= 60, "large queries whose thresholds leave a short entry list"
            # the interleave
            orders, kinds2 = E.serve_orders(tied, sh, how_many, at)
            assert kinds2 == kinds and orders["cells"] == list(range(len(calls))) and orders["reversed"] == orders["cells"][::-1]
            order = orders["interleave"]
            assert set(order) == set(range(len(calls))), "the interleave leaves a call out"
            form = lambda i: calls[i]["r"]["L"] > 4   # noqa: E731
            for p, i in enumerate(order):
                if kinds[i] != "served":   # every call the form does not finish: a served one of the SAME form (the same workgroup, with one caller) directly behind it
                    assert p + 1 < len(order) and kinds[order[p + 1]] == "served" and form(order[p + 1]) == form(i), (calls[i]["name"], p)
            for f in (False, True):
                mine = [i for i in range(len(calls)) if form(i) == f and kinds[i] == "served"]
                heavy, light = max(mine, key=lambda i: (E.serve_weight(calls[i]), i)), min(mine, key=lambda i: (E.serve_weight(calls[i]), i))
                p = order.index(heavy)
                assert order[p + 1] == light and calls[light]["r"]["n"] == 0 and calls[heavy]["r"]["n"] == (E.N_MID if f else min(E.N_LEAN, 4 * m - 3)), (calls[heavy]["name"], calls[light]["name"])   # (the largest n the form takes; at m = 1 100 four lists under a cut)
                head = order[p:p + len(mine)]
                assert sorted(head) == sorted(mine) and all(E.serve_weight(calls[a]) >= E.serve_weight(calls[b]) for a, b in zip(head[0::2], head[1::2]))
                assert any(int((calls[i]["r"]["dense"] < E.N_HOT).sum()) >= 150 for i in head[0:8:2]), "the heaviest carry a hot-head payload"
