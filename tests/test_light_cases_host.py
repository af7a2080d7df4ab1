"""The designed cases of tests/light_cases.py are what they claim, checked on the CPU against the oracle: list lengths, neighbours, row lengths, scored items -- and the
module's prediction of what the light form admits and what it hands to the general kernel."""
import numpy as np
import pytest

import light_cases as LC


@pytest.fixture(scope="module")
def world():
    from oracle import oracle as O
    c = LC.build()
    oix = O.OracleIndex(c.off, c.items, c.ts, LC.M_INDEX, LC.ROW_MAX, 1.0, fast=True)
    return c, oix


def _case(c, name):
    return c.queries[c.names.index(name)]


def test_the_cases_are_what_they_claim(world):
    c, oix = world
    for n in (1, 2, 63, 64, 65):
        q = _case(c, "kept=%d" % n)
        p, _ = oix.postings(q[0])
        assert len(p) == n
        sid, _num, U = oix.neighbors_canonical(np.array(q, np.uint64), LC.K, LC.M)[:3]
        assert len(sid) == n and U == 1, "every entry of a list of <= 64 <= k, m entries is a neighbour"
        assert LC.predict_one(c, q)["admitted"] == (n <= 64)
    for name, ps, L in (("[unknown, a]", 0, 2), ("[a, unknown]", 1, 2), ("[a, a]", 0, 2), ("[unknown, unknown, a, unknown]", 1, 4)):
        r = LC.predict_one(c, _case(c, name))
        assert r["admitted"] and (r["ps"], r["L"], r["nr"], r["kept"]) == (ps, L, 1, 5), (name, r)
    assert LC.predict_one(c, _case(c, "[a, a]"))["U"] == 1 and LC.predict_one(c, _case(c, "[a, unknown]"))["U"] == 2
    r = LC.predict_one(c, _case(c, "two short lists"))
    assert not r["admitted"] and r["nr"] == 2
    assert LC.predict_one(c, _case(c, "unknown only"))["nr"] == 0 and not LC.predict_one(c, _case(c, "unknown only"))["admitted"]
    # the three row layouts, and a row that holds the current item (every neighbour's row does)
    q = _case(c, "rows of 15, 16, 34 items")
    p, _ = oix.postings(q[0])
    assert sorted(len(c.rows[int(s)]) for s in p) == [15, 16, 34]
    assert all(int(q[0]) in [LC.ID0 + LC.ID_STEP * x for x in c.rows[int(s)]] for s in p)
    r = LC.predict_one(c, q)
    assert r["admitted"] and not r["general"] and r["scored"] == 62 and r["T"] == 62
    r = LC.predict_one(c, _case(c, "table overflow"))
    assert r["admitted"] and r["general"] and r["distinct"] == 64 * 33 + 1 > LC.TABLE_SLOTS
    r = LC.predict_one(c, _case(c, "ties at the cut"))
    assert r["admitted"] and r["general"] and r["scored"] == 90 and r["T"] == 90 > LC.RANK_MAX
    for i in range(LC.N_HEAVY):
        assert not LC.predict_one(c, _case(c, "heavy %d" % i))["admitted"] and not LC.predict_one(c, _case(c, "heavy %d + tail" % i))["admitted"]


def test_scored_items_and_rows_are_the_oracles(world):
    """The prediction's scored items are the oracle's rows: the count of a row is min(scored, how_many) for every admitted query, at both widths."""
    c, oix = world
    from helpers import flatten
    flat, off = flatten(c.queries)
    for how_many in (21, 64):
        ref = oix.predict_batch("canonical", flat, off, LC.K, LC.M, how_many, False, threads=4)
        for qi, q in enumerate(c.queries):
            r = LC.predict_one(c, q, how_many)
            if r["admitted"]:
                assert int(ref["counts"][qi]) == min(r["scored"], how_many), (c.names[qi], r, int(ref["counts"][qi]))


def test_the_batch_covers_the_form(world):
    c, _ = world
    rs = [LC.predict_one(c, q) for q in c.queries]
    light, general = LC.predict(c, c.queries)
    light_all, general_all = LC.predict(c, c.queries, merge=False)
    print("%d queries, %d distinct; light %d of the distinct (%d of all), handed on %d (%d); scored > 64 and served: %d" % (
        len(c.queries), len({tuple(q) for q in c.queries}), light, light_all, general, general_all, sum(r["admitted"] and not r["general"] and r["scored"] > 64 for r in rs)))
    assert light >= 200 and light_all > light, "equal light queries several times over"
    assert general == 2 and general_all == 4, "the two designed overflow cases, each once more"
    assert sum(r["admitted"] and not r["general"] and r["scored"] > LC.RANK_MAX for r in rs) >= 20, "rows of more than 64 scored items that the wave cuts itself"
    assert sum(r["admitted"] and r["scored"] <= LC.RANK_MAX for r in rs) >= 50
    assert {r["ps"] for r in rs if r["admitted"]} == {0, 1} and {r["L"] for r in rs if r["admitted"]} >= {1, 2, 4}
    only = [q for q, r in zip(c.queries, rs) if r["admitted"]]
    none = [q for q, r in zip(c.queries, rs) if not r["admitted"]]
    assert LC.predict(c, only, merge=False)[0] == len(only) and LC.predict(c, none)[0] == 0 and len(none) >= 10
    assert LC.predict(c, c.queries, k=63) == (0, 0), "k < 64: K = kept does not hold, the form is off"
