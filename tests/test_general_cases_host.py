"""The designed index of tests/general_cases.py on the CPU: its census (both sides of every edge are hit), its restatement against the oracle's counters, neighbour sets and accumulators, a worked
shape of the geometry, and the sequential simulation of the two double-hashed tables that tells tests/test_gpu_general_edges.py where it may assert a
status word exactly.  No GPU."""
import numpy as np
import pytest

import general_cases as G
from helpers import flatten

VARIANTS = ["distinct", "tied"]
KM = sorted({(k, m) for _b, k, m in G.LAUNCHES})


def test_a_worked_shape_of_the_geometry():
    g = G.geometry(1500, 2500, 8, dict(n_kept=20000, n_items=4096, m_index=2500, max_row_len=34))
    want = dict(off_a=13920, sess_slots=16384, hot_slots=4096, sketch_slots=4096, item_buckets=1097, region_a_bytes=67872, wwords=20040, rb_slots=3072, CAP_S1=572,
                masks=1, slot64=0, legacy=0)
    assert {w: g[w] for w in want} == want
    assert G.geometry(1936, 2500, 255, dict(n_kept=1 << 18, n_items=1 << 17, m_index=3072, max_row_len=48)) is None, "the accumulators' range guard at 255 items"
    assert G.geometry(1900, 2500, 255, dict(n_kept=1 << 18, n_items=1 << 17, m_index=3072, max_row_len=48))["slot64"] == 1
    assert G.geometry(1500, 2500, 8, dict(n_kept=1 << 18, n_items=1 << 17, m_index=3072, max_row_len=48), dict(SRN_NO_MASKS=1))["masks"] == 0
    g = G.geometry(1500, 2500, 8, dict(n_kept=1 << 18, n_items=1 << 17, m_index=3072, max_row_len=48), dict(SRN_SKETCH_SLOTS=64, SRN_HOT_SLOTS=32))
    assert (g["hot_slots"], g["sketch_slots"], g["sketch_shift"]) == (32, 64, 26)


@pytest.mark.parametrize("variant", VARIANTS)
def test_census(variant):
    hits = G.census(variant == "tied")
    assert len(hits) >= 66 and min(hits.values()) >= 1
    fam = G.family_counts()
    print("%s: %d sessions, %d queries, %d edges; cells per family: %s" % (variant, G.build(variant == "tied").n_sess, len(G.build(variant == "tied").queries), len(hits), fam))
    assert set(fam) <= set(G.FAMILIES)


@pytest.fixture(scope="module", params=VARIANTS)
def oracle_index(request):
    from oracle import oracle as O
    ix = G.build(request.param == "tied")
    return ix, O.OracleIndex(ix.off, ix.items, ix.ts, G.M_INDEX, G.ROW_MAX, 1.0, fast=True)


@pytest.mark.parametrize("k,m", KM)
def test_restate_against_the_oracle(oracle_index, k, m):
    ix, oix = oracle_index
    flat, off = flatten(ix.queries)
    st = oix.predict_batch("canonical", flat, off, k, m, 21, False, threads=8, want_stats=True)["stats"].astype(np.int64)
    R = G.restate(ix.tied, k, m)
    mine = np.array([[r["P"], r["C"], r["K"], r["I"], r["D"], 0, r["L"]] for r in R], np.int64)
    for col, name in ((0, "P"), (1, "C"), (2, "K"), (3, "I"), (4, "D"), (6, "L")):
        bad = np.flatnonzero(mine[:, col] != st[:, col])
        assert len(bad) == 0, "%s differs from the oracle at %s: %s against %s" % (name, [ix.cells[ix.q_cell[q]]["name"] for q in bad[:4]], mine[bad[:4], col], st[bad[:4], col])
    # the neighbour (session, numerator) sets are neighbors_canonical's, the accumulators scores_canonical's: what the GPU test takes from the restatement
    for qi, (q, r) in enumerate(zip(ix.queries, R)):
        name = ix.cells[ix.q_cell[qi]]["name"]
        sid, num, U = oix.neighbors_canonical(q, k, m)
        assert U == r["U"] and len(sid) == r["K"] and sorted(zip(sid.tolist(), num.tolist())) == r["nb"], name
        ids, _sc, acc = oix.scores_canonical(q, k, m)
        mine_acc = dict(zip((G.ID0 + G.ID_STEP * r["scored"]).tolist(), r["acc"].tolist()))
        theirs = dict(zip(ids.tolist(), acc.tolist()))
        assert {i: a for i, a in mine_acc.items() if i in theirs} == theirs and len(theirs) >= len(mine_acc) - 1, name   # (the oracle may leave the current item out)


def test_a_sketch_word_shared_by_a_winner_and_a_loser(oracle_index):
    """Accumulators: two scored items outside the hot words whose dense indices share a sketch word, one of them in the oracle's top 21 and one not."""
    ix, oix = oracle_index
    launch = ("A", G.K, 2500)
    g = G.geometry_of(ix, launch)
    hits = 0
    for qi in G.batch(ix, "A"):
        r = G.restate(ix.tied, G.K, 2500)[qi]
        ids = oix.predict_canonical(ix.queries[qi], G.K, 2500, 21, False)[0]
        won = np.isin(G.ID0 + G.ID_STEP * r["scored"], np.asarray(ids, np.uint64).astype(np.int64))
        rest = r["dense"] >= g["hot_slots"]
        word = r["dense"] & (g["sketch_slots"] - 1)
        hits += len(np.intersect1d(word[rest & won], word[rest & ~won])) > 0
    print("%d queries with a sketch word shared by a winner and a loser" % hits)
    assert hits >= 3


def test_tables_where_a_status_may_be_asserted():
    ix = G.build(False)
    name_of = lambda qi: ix.cells[ix.q_cell[qi]]["name"]   # noqa: E731
    for launch, knobs in ((("A", G.K, 2500), None), (("A", G.K, 2500), dict(SRN_NO_MERGE=1)), (("B", G.K, 2500), None), (("C", G.K, 2500), None)):
        ex = dict(zip((name_of(qi) for qi in G.batch(ix, launch[0])), G.expect_status(ix, launch, knobs)))
        if launch[0] == "A":
            # `must fit`: half of the session table, within FIT_PROBES probes in three orders whether the merge tree or the hash table takes it
            assert ex["distinct kept = sess_slots/2"] == ("fit",), ex["distinct kept = sess_slots/2"]
            assert ex["distinct kept > sess_slots"] == ("global",)
            assert ex["k neighbours x 3 rare items"][:2] == ("parts", 2) and ex["k neighbours x 6 rare items"][:2] == ("parts", 4)
            assert ex["K=513"] == ("fit",) and ex["K=1"] == ("fit",)
        assert sum(e == ("global",) for e in ex.values()) >= 1 and sum(e == ("fit",) for e in ex.values()) >= 10, launch
    # 64-bit slots: a table of 4 096 slots, so every cell of more than that many kept sessions goes global
    assert sum(e == ("global",) for e in ex.values()) >= 8
    # the simulation itself: a table filled to the brim fails, half full stays within the budget
    keys = np.arange(1000, 1000 + 1024)
    assert G.sess_probes(keys, 1024) > G.FIT_PROBES and G.sess_probes(keys[:512], 1024) <= G.FIT_PROBES and G.sess_probes(np.arange(2000), 1024) == G.MAX_PROBES + 1
    assert G.item_probes(np.arange(5000, 5000 + 4 * 61 + 1), 61) == G.MAX_PROBES + 1 and G.item_probes(np.arange(5000, 5000 + 2 * 61), 61) <= G.FIT_PROBES
    assert np.array_equal(G.hash_part(keys, 4) // 2, G.hash_part(keys, 2)), "hash_part(it, 2 parts) refines hash_part(it, parts)"
