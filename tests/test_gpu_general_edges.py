"""The designed index of tests/general_cases.py through the GENERAL kernel (vmis_predict_kernel), against the canonical oracle.  The index places a query on either side
of the kernel's own thresholds -- merge-mode admission, the merge mode's k-cut forms, the m-cut, the session and item tables' capacities, the row walks' length
thresholds, the accumulator split, the top-n forms, 64-bit slots -- and tests/test_general_cases_host.py asserts on the CPU that it does (the census), so nothing here
passes vacuously.  One index per timestamp variant; one batch per launch shape of general_cases.LAUNCHES, under default knobs and SRN_NO_MERGE=1, the <= 8-item batches
also under SRN_NO_MASKS=1, SRN_HOT_SLOTS=0 and SRN_SKETCH_SLOTS=64 + SRN_HOT_SLOTS=32.

(a) Geometry: srn_debug_geometry equals general_cases.geometry word for word, for every launch and knob set used (the cells are designed from the restatement).
(b) Rows: predict_batch_debug (the sketch filter off) against the oracle -- counts, ids, order exact, scores to 1e-12 --, its counters P, C, K, I, D, H, L and, at
    k <= 1 536, its neighbour (session, numerator) sets exact; the product call under SRN_NO_FAST=1 (filter on) the same bytes.
(c) Status word: 1 for exactly the cells that must take the global-table pass, 0 where both tables must fit, 0x100 * parts within the pigeonhole bound (equal to the
    simulated value where general_cases.item_parts says it may be asserted), never 3 or 4; srn_last_path_counts' global_pass of the product call = the designed count.
(d) The 64-bit-slot launch gives the <= 21-item launch's rows for the queries they share; the top-n forms at how_many 24 | 25 | 64 | 65 | 512; default knobs (fast
    kernels on) give the SRN_NO_FAST bytes.
"""
import os
import time

import numpy as np
import pytest

import general_cases as G
from edge_world import _same_bytes, _vs_oracle
from helpers import flatten

pytestmark = pytest.mark.gpu

VARIANTS = ["distinct", "tied"]
KNOBS = ("SRN_NO_FAST", "SRN_NO_MERGE", "SRN_NO_MASKS", "SRN_HOT_SLOTS", "SRN_SKETCH_SLOTS")
KNOB_SETS = {"default": {}, "no_merge": dict(SRN_NO_MERGE=1), "no_masks": dict(SRN_NO_MASKS=1), "no_hot": dict(SRN_HOT_SLOTS=0), "tiny_sketch": dict(SRN_SKETCH_SLOTS=64, SRN_HOT_SLOTS=32)}
CASES = [(l, ks) for l in G.LAUNCHES for ks in KNOB_SETS if ks in ("default", "no_merge") or (l[0] == "A" and l[2] == 2500)]


@pytest.fixture
def knobs():
    from serenade_amd import capi

    def set_(**kv):
        for name in KNOBS:
            os.environ.pop(name, None)
        for name, v in kv.items():
            os.environ[name] = str(v)
        capi.reload_knobs()
    yield set_
    for name in KNOBS:
        os.environ.pop(name, None)
    capi.reload_knobs()


class World:
    """One timestamp variant: the index on the GPU and in the oracle, each launch's batch on the device, the reference rows -- each built once and never changed."""

    def __init__(self, tied):
        import serenade_amd as sa
        import torch
        from oracle import oracle as O
        t0 = time.time()
        self.torch, self.tied = torch, tied
        self.ix = ix = G.build(tied)
        self.gix = sa.VMISIndex.from_sessions(ix.off, ix.items, ix.ts, G.M_INDEX, G.ROW_MAX, 1.0, device=0)
        self.oix = O.OracleIndex(ix.off, ix.items, ix.ts, G.M_INDEX, G.ROW_MAX, 1.0, fast=True)
        self.batch, self.dev = {}, {}
        for b in G.BATCH_MAX_LEN:
            sel = G.batch(ix, b)
            qs = [ix.queries[qi] for qi in sel]
            flat, off = flatten(qs)
            self.batch[b] = (sel, qs, flat, off)
            self.dev[b] = (torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to("cuda:0"), torch.from_numpy(off.view(np.int32).copy()).to("cuda:0"))
        self._ref, self._slow = {}, {}
        self.seconds = time.time() - t0

    def ref(self, b, k, m, how_many=21):
        key = (b, k, m, how_many)
        if key not in self._ref:
            _sel, _qs, flat, off = self.batch[b]
            r = self.oix.predict_batch("canonical", flat, off, k, m, how_many, False, threads=8, want_stats=True)
            for a in (r["ids"], r["scores"], r["counts"], r["stats"]):
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def call(self, b, k, m, how_many=21):
        """srn_predict_batch_device over the launch's resident batch (the launch sequence: prep records, then whatever the knobs leave on)."""
        import serenade_amd as sa
        t = self.torch
        nq = len(self.batch[b][0])
        o = (t.zeros(nq * how_many, dtype=t.int64, device="cuda:0"), t.zeros(nq * how_many, dtype=t.float64, device="cuda:0"), t.zeros(nq, dtype=t.int32, device="cuda:0"))
        sa.predict_batch_device(self.gix, self.dev[b][0].data_ptr(), self.dev[b][1].data_ptr(), nq, G.BATCH_MAX_LEN[b], k, m, how_many, False,
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), t.cuda.current_stream().cuda_stream, resident=True)
        t.cuda.synchronize()
        return (o[0].cpu().numpy().view(np.uint64).reshape(-1, how_many).copy(), o[1].cpu().numpy().reshape(-1, how_many).copy(), o[2].cpu().numpy().view(np.uint32).copy())


@pytest.fixture(scope="module", params=VARIANTS)
def world(request):
    w = World(request.param == "tied")
    print("%s: %d cells, %d sessions, %d queries, fixture built in %.1f s" % (request.param, len(w.ix.cells), w.ix.n_sess, len(w.ix.queries), w.seconds))
    return w


_expect = {}


def expect_status(launch, knob_set):
    """general_cases.expect_status, once per (launch, knob set): the sessions and rows are the same in both timestamp variants (recency rank = index in both)."""
    key = (launch, knob_set)
    if key not in _expect:
        _expect[key] = G.expect_status(G.build(False), launch, KNOB_SETS[knob_set])
    return _expect[key]


def test_a_the_index_is_what_the_restatement_takes_it_for(world):
    info = world.gix.info
    got = dict(n_kept=int(info["n_sessions_kept"]), n_items=int(info["n_items"]), m_index=int(info["m_index"]), max_row_len=int(info["max_row_len"]))
    assert got == world.ix.info and int(info["incomplete_items"]) == 0, (got, world.ix.info)


@pytest.mark.parametrize("launch,knob_set", CASES, ids=["%s_k%d_m%d-%s" % (l + (ks,)) for l, ks in CASES])
def test_b_rows_counters_status(world, knobs, launch, knob_set):
    import serenade_amd as sa
    b, k, m = launch
    kn = KNOB_SETS[knob_set]
    sel, qs, _flat, _off = world.batch[b]
    name = lambda i: world.ix.cells[world.ix.q_cell[sel[i]]]["name"]   # noqa: E731
    knobs(SRN_NO_FAST=1, **kn)
    # (a) the accessor equals the restatement, word for word
    acc = world.gix.debug_geometry(k, m, G.BATCH_MAX_LEN[b])
    g = G.geometry_of(world.ix, launch, kn, lds_max=acc["lds_max"])
    assert g is not None and {w: g[w] for w in acc} == acc, "the restated geometry differs: %s" % {w: (g[w], acc[w]) for w in acc if g[w] != acc[w]}
    # (b) rows, counters, neighbours: the debug call (filter off), then the product call (filter on), bit for bit
    ref = world.ref(b, k, m)
    t0 = time.time()
    res = sa.predict_batch_debug(world.gix, qs, k, m, 21, False, neighbours=k <= 1536)
    _vs_oracle((res["ids"], res["scores"], res["counts"]), ref, "debug call")
    bad = np.flatnonzero((res["stats"][:, :7].astype(np.uint64) != ref["stats"]).any(axis=1))
    assert len(bad) == 0, "P,C,K,I,D,H,L differ at %s: %s against the oracle's %s" % ([name(i) for i in bad[:4]], res["stats"][bad[:4], :7], ref["stats"][bad[:4]])
    if k <= 1536:
        R = G.restate(world.tied, k, m)
        for i, qi in enumerate(sel):
            kq = int(res["nb_counts"][i])
            assert sorted(zip(res["nb_sessions"][i, :kq].tolist(), res["nb_num"][i, :kq].tolist())) == R[qi]["nb"], name(i)
    got = world.call(b, k, m)
    nq, general, glob = world.gix.last_path_counts()
    _same_bytes(got, (res["ids"], res["scores"], res["counts"]), "product call (SRN_NO_FAST=1) against the debug call")
    world._slow[(launch, knob_set)] = got
    # (c) the status word
    status = res["stats"][:, 7]
    assert not np.isin(status, (2, 3, 4)).any(), "status 2 / 3 / 4 at %s" % [name(i) for i in np.flatnonzero(np.isin(status, (2, 3, 4)))]
    assert (nq, general) == (len(sel), len(sel))
    if knob_set in ("default", "no_merge"):
        ex = expect_status(launch, knob_set)
        n_global = n_open = 0
        for i, e in enumerate(ex):
            s = int(status[i])
            if e == ("global",):
                n_global += 1
                assert s == 1, (name(i), s)
            elif e == ("fit",):
                assert s == 0, (name(i), hex(s))
            elif e is not None:
                _tag, lo, hi, exact = e
                assert s != 1 and s == 0x100 * (s >> 8) and lo <= max(s >> 8, 1) <= hi and (s >> 8) & ((s >> 8) - 1) == 0, (name(i), hex(s), lo, hi)
                if exact:
                    assert max(s >> 8, 1) == lo, (name(i), hex(s), lo)
            else:
                n_open += 1
                assert s in (0, 1) or s == 0x100 * (s >> 8), (name(i), hex(s))
        print("%s %s: %d queries, %d must go global, %d must fit, %d with partitions, %d open; global_pass %d; GPU calls %.3f s" % (
            launch, knob_set, len(sel), n_global, sum(e == ("fit",) for e in ex), sum(e is not None and e[0] == "parts" for e in ex), n_open, glob, time.time() - t0))
        assert int((status == 1).sum()) >= n_global and n_global <= glob <= n_global + n_open
        if n_open == 0:
            assert glob == n_global == int((status == 1).sum())


def test_d_64_bit_slots_give_the_same_rows(world, knobs):
    knobs(SRN_NO_FAST=1)
    B, C = ("B", G.K, 2500), ("C", G.K, 2500)
    rb = world._slow.get((B, "default")) or world.call(*B)
    rc = world._slow.get((C, "default")) or world.call(*C)
    selb, selc = world.batch["B"][0], world.batch["C"][0]
    at = [selc.index(qi) for qi in selb]
    assert len(selc) == len(selb) + 1
    _same_bytes(tuple(a[at] for a in rc), rb, "64-bit slots against 32-bit slots")


@pytest.mark.parametrize("how_many", G.HOW_MANY)
@pytest.mark.parametrize("b", ["A", "B"])
def test_d_top_n_forms(world, knobs, b, how_many):
    knobs(SRN_NO_FAST=1)
    _vs_oracle(world.call(b, G.K, 2500, how_many), world.ref(b, G.K, 2500, how_many), "how_many %d" % how_many)
    knobs(SRN_NO_FAST=1, SRN_NO_MERGE=1, SRN_HOT_SLOTS=0)
    _vs_oracle(world.call(b, G.K, 2500, how_many), world.ref(b, G.K, 2500, how_many), "how_many %d, no hot words" % how_many)


@pytest.mark.parametrize("launch", G.LAUNCHES, ids=["%s_k%d_m%d" % l for l in G.LAUNCHES])
def test_d_default_knobs_give_the_same_bytes(world, knobs, launch):
    knobs(SRN_NO_FAST=1)
    slow = world._slow.get((launch, "default")) or world.call(*launch)
    knobs()
    got = world.call(*launch)
    nq, general, _glob = world.gix.last_path_counts()
    _vs_oracle(got, world.ref(*launch), "default knobs")
    _same_bytes(got, slow, "default knobs against SRN_NO_FAST=1")
    print("%s: %d queries, %d reached the general kernel with the fast kernels on" % (launch, nq, general))
    assert nq == len(world.batch[launch[0]][0])
