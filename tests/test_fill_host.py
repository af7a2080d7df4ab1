"""serving.fill_rows, the NumPy mirror of the fill kernel (srn_fill.hip), against a brute-force restatement of the rule, entry by entry, on the canonical
CPU oracle's rows of the sparse index: with and without lists, with exclude_session, with the business rules.  No GPU.
"""
import numpy as np
import pytest

from fill_cases import MAX_LEN, NONE, OracleRows, brute_force_fill, census, draw_attrs, popularity_order, sparse_dataset, sparse_queries, unfilled


@pytest.fixture(scope="module")
def sparse():
    from oracle import oracle as O
    off, items, ts, ids = sparse_dataset()
    assert len(np.unique(items)) == 505
    oix = O.OracleIndex(off, items, ts, 500, 20, 1.0)
    known, flags = draw_attrs(items)
    oix.set_attributes(known, flags)
    attrs = {int(i): int(f) for i, f in zip(known, flags)}
    qs = sparse_queries(ids)
    return OracleRows(oix, qs), popularity_order(items), attrs


def lists_for(qs, rows, ranking, E):
    """Per query: the head of the ranking, an id of its own row, a stranger and a duplicate, rotated by the query's number and cut to E; every seventh list empty."""
    ids, _sc, cnt = rows
    out = []
    for q in range(len(qs)):
        kinds = [int(ranking[0]), int(ranking[2]), int(ranking[5])] + ([int(ids[q, 0])] if cnt[q] not in (0, NONE) else []) + [777, int(ranking[0])]
        rot = q % len(kinds)
        out.append([] if q % 7 == 3 else (kinds[rot:] + kinds[:rot])[:E])
    return out


def test_the_census_of_the_sparse_index(sparse):
    orows, ranking, attrs = sparse
    assert census(orows.rows(21)[2], 21) == (95, 175, 330)
    c = orows.rows(100)[2]
    assert census(c, 100) == (95, 365, 140)
    assert int(((c >= 65) & (c <= 99)).sum()) == 66
    # counts tie massively: the order's id tie-break is exercised
    u, n = np.unique(sparse_dataset()[1], return_counts=True)
    by_id = dict(zip(u.tolist(), n.tolist()))
    assert by_id[int(ranking[64])] == 2 and by_id[int(ranking[128])] == 2


@pytest.mark.parametrize("how_many,E,session,business", [(21, 0, False, False), (21, 8, False, False), (21, 0, True, False), (21, 0, False, True), (21, 8, True, True),
                                                         (100, 0, False, False), (100, 8, True, True), (70, 0, False, False)])
@pytest.mark.parametrize("R", [256, 16])
def test_fill_rows_against_the_rule(sparse, how_many, E, session, business, R):
    from serenade_amd.serving import fill_rows
    orows, order, attrs = sparse
    qs, ranking = orows.qs, [int(x) for x in order[:R - 1]] + [123456789]   # (the last entry: an id the index does not know)
    excl = lists_for(qs, orows.rows(how_many + E + (MAX_LEN - 1 if session else 0), business), ranking, E) if E else None
    ids, sc, cnt = unfilled(orows, how_many, excl, E, session, business)
    empty, short, full = census(cnt, how_many)
    if how_many == 21:
        assert empty >= 50 and short >= 50 and full >= 50, (empty, short, full)
    if how_many == 100:
        assert int(((cnt > 64) & (cnt < 100)).sum()) >= 30
    before = (ids.copy(), sc.copy(), cnt.copy())
    got = fill_rows(ids, sc, cnt, qs, ranking, how_many, excl=excl, exclude_session=session, attrs=attrs, business=business)
    assert all(np.array_equal(a, b) for a, b in zip((ids, sc, cnt), before)), "fill_rows changed its inputs"
    mismatches = filled = 0
    for q in range(len(qs)):
        c = int(cnt[q])
        if c == NONE or c >= how_many:
            mismatches += not (got[2][q] == cnt[q] and np.array_equal(got[0][q], ids[q]) and np.array_equal(got[1][q].view(np.uint64), sc[q].view(np.uint64)))
            continue
        add = brute_force_fill([int(x) for x in ids[q, :c]], qs[q], ranking, how_many, excl[q] if excl else (), session, attrs, business)
        n = c + len(add)
        ok = got[2][q] == n and np.array_equal(got[0][q, :c], ids[q, :c]) and np.array_equal(got[1][q, :c].view(np.uint64), sc[q, :c].view(np.uint64)) \
            and [int(x) for x in got[0][q, c:n]] == add and np.isneginf(got[1][q, c:n]).all() and not got[0][q, n:].any() and not got[1][q, n:].any()
        mismatches += not ok
        filled += len(add)
    assert mismatches == 0
    assert filled > 0
    if R == 256 and not business:
        assert (got[2][got[2] != NONE] == how_many).all(), "a ranking of 256 fills every row"
    if R == 16 and how_many >= 70:
        assert (got[2][(cnt == 0)] < how_many).all(), "a ranking of 16 cannot fill an empty row of %d" % how_many


def test_passes_business_rules_is_the_reference_table():
    from serenade_amd.serving import passes_business_rules
    for cur in (0, 1, 2, 3, 0xFF):
        for reco in (0, 1, 2, 3, 0xFF):
            want = reco != 0xFF and bool(reco & 2) and (not reco & 1 or (cur != 0xFF and bool(cur & 1)))
            assert passes_business_rules(cur, reco) == want, (cur, reco)
