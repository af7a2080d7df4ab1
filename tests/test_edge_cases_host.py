"""The designed index of tests/edge_cases.py on the CPU: the condition that keeps tests/test_gpu_edge_cases.py from passing vacuously.

(a) The census: every edge the module lists is hit, on both sides, by at least one (query, call shape) pair -- asserted edge by edge from the NumPy restatement, for both
    timestamp variants; a cell whose sessions miss its designed (len, kept) fails here.
(b) The restatement against the oracle: posting-list lengths, neighbors_canonical's K and (session, numerator) sets, and the counters P, C, K, I, D, H, L of
    predict_batch(..., want_stats=True), for every query at both call shapes.
(c) The oracle's rows for every 8th query against helpers.canonical_acc_over_given_lists with exact Fraction scores (as tests/test_gpu_given_idf.py does for its index).
(d) The tied variant: the designed counts are those of the distinct variant, and tie groups straddle x_lo and the k-cut's boundary (part of its census)."""
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
