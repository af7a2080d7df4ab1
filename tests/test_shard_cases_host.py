"""The designed index of tests/shard_cases.py on the CPU: the condition that keeps tests/test_gpu_shard_edges.py from passing vacuously.

(a) The census: every edge the module lists is hit, on both sides, by at least one (query, shard) pair, for both timestamp variants and for 8 and 2 shards; the designed
    popularity order of shards 0..6 and every cell's designed quantities on its target shard are asserted there too.
(b) The restated owner map and shard-local order against the library, on shards cut without a device: postings(id) on a shard is None exactly for the ids the map gives
    to other shards, and the full index's set_fallback_popular(4 096), filtered by the map, is the head of every shard's restated order (a shard itself refuses a
    ranking; its whole order is checked on the GPU, where the accumulator cells' counters depend on it).
(c) The restated neighbours (K, sessions, numerators' weights) against the oracle's neighbors_canonical, and the oracle's fast form against its slow form on the index.
(d) The tied variant has the distinct variant's rows, ranks and restated quantities."""
import numpy as np
import pytest

import shard_cases as S
from helpers import flatten

VARIANTS = [False, True]
IDS = ["distinct", "tied"]


@pytest.mark.parametrize("G", [8, 2])
@pytest.mark.parametrize("tied", VARIANTS, ids=IDS)
def test_census_every_edge_on_both_sides(tied, G):
    ix = S.build(tied)
    hits = S.census(tied, G)
    print("%d cells, %d sessions (%d filler), %d interactions; G = %d: %d edges, the rarest hit %d times" % (len(ix.cells), len(ix.ts), ix.n_fill, len(ix.items), G, len(hits), min(hits.values())))
    for name, c in hits.items():
        print("%5d  %s" % (c, name))
    assert min(hits.values()) > 0
    assert len(ix.ts) <= 20000 and len(ix.items) <= 500000, "the index has outgrown its budget"
    assert S.uncertain_queries(tied, 8) == []
    assert (S.SB_LQ_CAP, S.SB_HIT_CAP, S.TABLE_SLOTS, S.TABLE_SAFE) == (448, 272, 244, 192)


def _postings(shard, item_id):
    """srn_index_postings on a shard handle -> the sessions, most recent first, or None for an id the shard does not hold."""
    import ctypes as C
    from serenade_amd import capi
    n, idf = C.c_int64(), C.c_double()
    capi.check(capi.lib().srn_index_postings(shard._h, item_id, None, 0, C.byref(n), C.byref(idf)))
    if n.value < 0:
        return None
    out = np.zeros(max(n.value, 1), np.uint32)
    capi.check(capi.lib().srn_index_postings(shard._h, item_id, capi.ptr(out), n.value, C.byref(n), C.byref(idf)))
    return out[:n.value]


@pytest.mark.parametrize("G", [8, 2])
def test_owner_map_and_shard_local_order_against_the_library(G):
    import serenade_amd as sa
    from serenade_amd import capi, sharded
    ix = S.build(False)
    full = sa.VMISIndex.from_sessions(ix.off, ix.items, ix.ts, S.M_INDEX, S.ROW_MAX, 1.0, device=-1)
    ids = (S.ID0 + S.ID_STEP * ix.l_items).astype(np.uint64)
    own = S.owner(ids, G)
    assert np.array_equal(own, ix.h8 % G)
    probe = np.concatenate([np.arange(0, len(ids), 37), np.flatnonzero(np.isin(ix.l_items, np.concatenate([c[:20] for c in ix.cat])))])
    for g in range(G):
        sh = sharded.ShardedVMISIndex.from_full(full, g, G, device=-1)
        v = S.view(False, G, g)
        assert sh.info["n_items"] == v.n_items
        for j in probe:
            sessions = _postings(sh, int(ids[j]))
            assert (sessions is None) == (own[j] != g), (g, int(ids[j]))
            if sessions is not None:
                assert np.array_equal(sessions.astype(np.int64), ix.l_sess[ix.l_off[j]:ix.l_off[j + 1]][:S.M_INDEX])
    # the order: a shard refuses a fallback ranking (it answers no call by itself), and shard_flat_index keeps the full index's relative order for the owned items
    # (srn_index.cpp:253-256) -- so the full index's popularity order, as far as a ranking reaches (4 096 items), filtered by the map, is the head of every shard's
    full.set_fallback_popular(capi.MAX_FALLBACK)
    head = full.fallback()
    assert len(head) == capi.MAX_FALLBACK and np.array_equal(head, ids[np.argsort(ix.dense)[:len(head)]])
    for g in range(G):
        mine = head[S.owner(head, G) == g]
        assert len(mine) >= 256 and np.array_equal(mine, S.popularity_order(False, G, g, len(mine))), "shard %d of %d: the restated popularity order is not the library's" % (g, G)


@pytest.fixture(scope="module")
def oracle_index():
    from oracle import oracle as O
    ix = S.build(False)
    known, flags = S.attributes(ix)
    fast = O.OracleIndex(ix.off, ix.items, ix.ts, S.M_INDEX, S.ROW_MAX, 1.0, fast=True)
    fast.set_attributes(known, flags)
    return ix, fast, known, flags


def test_restated_neighbours_equal_the_oracle(oracle_index):
    ix, oix, _known, _flags = oracle_index
    for k, m in S.SHAPES:
        for qi, q in enumerate(ix.queries):
            r = S.neighbours(ix, q, k, m)
            sid, num, U = oix.neighbors_canonical(q, k, m)
            assert len(sid) == r["K"] and U == r["U"], (ix.cells[qi]["name"], k, m)
            assert sorted(sid.tolist()) == sorted(r["sess"].tolist()), (ix.cells[qi]["name"], k, m)
            # weight = (9 - most recent matched position) * numerator: the numerator alone where the most recent item matches
            by = dict(zip(sid.tolist(), num.tolist()))
            assert all(w % by[s] == 0 and 2 <= w // by[s] <= 9 for s, w in zip(r["sess"].tolist(), r["w"].tolist())), (ix.cells[qi]["name"], k, m)


def test_oracle_fast_form_against_its_slow_form(oracle_index):
    from oracle import oracle as O
    ix, fast, known, flags = oracle_index
    slow = O.OracleIndex(ix.off, ix.items, ix.ts, S.M_INDEX, S.ROW_MAX, 1.0)
    slow.set_attributes(known, flags)
    pick = [qi for qi, ci in enumerate(ix.q_cell) if ix.cells[ci]["family"] in ("fragments", "accumulators", "capacity", "threshold", "shape") or ix.cells[ci]["name"] in ("K=257", "K=1536")]
    flat, off = flatten([ix.queries[qi] for qi in pick])
    for (k, m), how_many, business in ((S.SHAPES[0], 21, False), (S.SHAPES[1], 24, True)):
        a = fast.predict_batch("canonical", flat, off, k, m, how_many, business, threads=4)
        b = slow.predict_batch("canonical", flat, off, k, m, how_many, business, threads=4)
        assert np.array_equal(a["counts"], b["counts"])
        inside = np.arange(how_many)[None, :] < a["counts"][:, None].astype(np.int64)
        assert np.array_equal(a["ids"][inside], b["ids"][inside]) and np.array_equal(a["scores"][inside].view(np.uint64), b["scores"][inside].view(np.uint64))
        assert int(inside.sum()) > 200


def test_tied_variant_has_the_designed_counts():
    a, b = S.build(False), S.build(True)
    assert np.array_equal(a.off, b.off) and np.array_equal(a.items, b.items) and a.queries == b.queries and np.array_equal(a.rank, b.rank)
    assert len(np.unique(b.ts)) == (len(b.ts) + 7) // 8
    for G in (8, 2):
        ra, rb = S.restate(False, 1, 21, G), S.restate(True, 1, 21, G)
        for qa, qb in zip(ra, rb):
            for x, y in zip(qa, qb):
                assert all(x[key] == y[key] for key in ("outcome", "K", "nlq", "nlb", "ncand", "npass", "nh", "nt", "M", "t32", "c15"))


def test_small_shards_have_the_designed_sizes():
    """The tiny index of the small-shard tests: 0, 1, 15, 16, 17, 255, 256 and 257 items on the eight shards, by the restated map and by the library's shard cut."""
    import serenade_amd as sa
    from serenade_amd import sharded
    ix = S.small_build()
    assert tuple(ix.sizes.tolist()) == S.SMALL_SIZES
    full = sa.VMISIndex.from_sessions(ix.off, ix.items, ix.ts, S.M_INDEX, S.ROW_MAX, 1.0, device=-1)
    for g, n in enumerate(S.SMALL_SIZES):
        sh = sharded.ShardedVMISIndex.from_full(full, g, 8, device=-1)
        assert sh.info["n_items"] == n
    assert all(1 <= len(q) <= 5 for q in ix.queries) and len(ix.queries) == 96
