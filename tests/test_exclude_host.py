"""Exclusion lists, the argument on the CPU: a row is the first how_many entries of a total order over the query's candidates, so with at most E excluded
ids the first how_many + E entries hold the first how_many survivors in order.  serenade_amd.serving.filter_rows -- the NumPy mirror of the device filter -- over the
oracle's canonical rows at how_many + E must therefore equal the oracle's rows over ALL candidates (how_many 512), filtered and cut, ids and score bits alike.

A list is E - 1 ids drawn from the first how_many + E - 1 entries of the query's own full row plus one id the index has never seen; the test asserts that the lists
bite inside the top how_many on at least 90 % of the queries (it could pass with nothing excluded otherwise).  With (how_many, E) = (1, 1) the list is the stranger alone.
"""
import numpy as np
import pytest

from helpers import flatten, random_queries, small_dataset

K, M, FULL = 100, 500, 512
CASES = [(21, 8), (5, 3), (50, 30), (1, 1), (60, 5)]
STRANGER = 999


@pytest.fixture(scope="module")
def rows():
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(31, n_sessions=6000, n_items=150, max_len=12)
    oix = O.OracleIndex(off, items, ts, 3000, 20, 1.0)
    qs = random_queries(5, ids, 400, max_len=6)
    flat, qoff = flatten(qs)
    full = oix.predict_batch("canonical", flat, qoff, K, M, FULL, False, threads=4)
    assert int(full["counts"].max()) < FULL, "how_many 512 must hold every candidate of every query"
    return oix, flat, qoff, full


def _lists(full, how_many, E, rng):
    out = []
    for q in range(len(full["counts"])):
        head = min(int(full["counts"][q]), how_many + E - 1)
        pick = rng.choice(head, size=min(E - 1, head), replace=False) if head else np.zeros(0, np.int64)
        out.append([int(full["ids"][q, p]) for p in pick] + [STRANGER])
    return out


@pytest.mark.parametrize("how_many,E", CASES)
def test_filter_of_wide_rows_equals_filter_then_cut(rows, how_many, E):
    from serenade_amd.serving import filter_rows
    oix, flat, qoff, full = rows
    nq = len(qoff) - 1
    excl = _lists(full, how_many, E, np.random.default_rng(1000 * how_many + E))
    assert all(len(x) <= E for x in excl)
    wide = oix.predict_batch("canonical", flat, qoff, K, M, how_many + E, False, threads=4)
    ids, sc, cnt = filter_rows(wide["ids"], wide["scores"], wide["counts"], excl, how_many)
    mismatches = bites = 0
    for q in range(nq):
        n = int(full["counts"][q])
        gone = set(excl[q])
        want = [(int(i), float(s)) for i, s in zip(full["ids"][q, :n], full["scores"][q, :n]) if int(i) not in gone][:how_many]
        got = list(zip((int(i) for i in ids[q, :cnt[q]]), (float(s) for s in sc[q, :cnt[q]])))
        mismatches += got != want
        bites += any(int(i) in gone for i in full["ids"][q, :min(n, how_many)])
    print("how_many %d, E %d: %d mismatches, lists bite inside the top how_many on %d of %d queries, rows of up to %d candidates"
          % (how_many, E, mismatches, bites, nq, int(full["counts"].max())))
    assert mismatches == 0
    if E > 1:
        assert bites >= 0.9 * nq, "the lists bite on %d of %d queries only" % (bites, nq)


def test_filter_rows_passes_the_unserved_marker_on_and_zeroes_the_tail():
    from serenade_amd.serving import filter_rows
    ids = np.array([[5, 6, 7, 8], [1, 2, 3, 4], [9, 9, 9, 9]], np.uint64)
    sc = np.array([[4.0, 3.0, 2.0, 1.0]] * 3)
    got = filter_rows(ids, sc, np.array([4, 0xFFFFFFFF, 2], np.uint32), [[6, 6, 99], [], [9]], 3)
    assert got[2].tolist() == [3, 0xFFFFFFFF, 0]
    assert got[0][0].tolist() == [5, 7, 8] and got[1][0].tolist() == [4.0, 2.0, 1.0]
    assert not got[0][1:].any() and not got[1][1:].any()
