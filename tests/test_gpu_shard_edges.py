"""The item shard's wave-per-query back end (vmis_shard_back_kernel, srn_sback.hip) on the designed index of tests/shard_cases.py, whose census
(tests/test_shard_cases_host.py) proves that both sides of every capacity, fragment length, accumulator address and K of the kernel are hit.

Rows: every form of the launch plumbing gives the oracle's rows and the unsharded path's bytes, for 2 and 8 shards, both call shapes, with and without the business rules.
Paths: WHICH code served a query is read from the kernel's own counters (srn_debug_phase_cycles) and compared, shard by shard and family by family, with the exact
integers of shard_cases.restate_shard -- under SRN_NO_SBACK_SECOND=1, so that slot 15 is this kernel's alone (the fast kernel's back-end form writes it with another layout,
srn_fast.hip:1440).  Slots 5, 6, 7, 14 and 15 are written by no other launch of a group call: the front end over a rank's slice (vmis_fast_kernel, FM_FRONT) leaves at
srn_fast.hip:1016-1021, before the back-end phases that count, and the general kernel ticks slots 0..4 and 8..13 only (srn_kernels.hip).
Per query: every capacity cell alone and in front of a light cell, where state left behind by a handed-over query would show.

Small shards: a second, tiny index whose eight shards hold 0, 1, 15 / 16 / 17 and 255 / 256 / 257 items, rows only.  Full-width ids: the designed index and its batch
through edge_cases.wide_ids (the hand-off record carries id ranks, not ids); the map moves every item to another shard, so only rows are compared there.

Which form a call took is asserted from the group's own statistics: one neighbours batch per call, and the bytes of its exchange -- position records of the
streaming form's stride, or k + 1 words of neighbour slots.  The streaming form's counters are compared with the same restatement.

Left out (said in shard_cases.py's docstring too): a call past SB_REC_ROOM (unreachable through the neighbours pipeline; the call with m one past F_M_MAX and a session
of nine items are pinned for their rows)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import edge_cases as E
import shard_cases as S
from edge_world import _same_bytes, _vs_oracle
from helpers import flatten

pytestmark = pytest.mark.gpu

KNOBS = ("SRN_SBACK_MIN_SHARDS", "SRN_SBACK_STREAM", "SRN_NO_SBACK", "SRN_NO_SBACK_SECOND", "SRN_ORDER_MIN", "SRN_FAST_RUNS")
FORMS = {"gather": {}, "stream": {"SRN_SBACK_STREAM": 1}, "no_sback": {"SRN_NO_SBACK": 1}, "no_second": {"SRN_NO_SBACK_SECOND": 1}, "ordered": {"SRN_ORDER_MIN": 1},
         "runs3": {"SRN_FAST_RUNS": 3}}
CALLS = {"A": (1, 21, False), "B": (0, 21, True), "C": (1, 24, False), "D": (1, 21, True), "E": (0, 24, False)}   # (shape, how_many, business rules): both shapes, each plain and with the rules


def _set_knobs(**kv):
    from serenade_amd import capi
    for name in KNOBS:
        os.environ.pop(name, None)
    for name, v in kv.items():
        os.environ[name] = str(v)
    capi.reload_knobs()


@pytest.fixture
def knobs():
    """Switches the SRN_* knobs of this module; SRN_SBACK_MIN_SHARDS=2 stays on while a test runs, everything is restored behind it."""
    def set_(**kv):
        _set_knobs(SRN_SBACK_MIN_SHARDS=2, **kv)
    set_()
    yield set_
    _set_knobs()


class World:
    """One timestamp variant: the full index on the GPU and in the oracle, its shards for 2 and 8 (attached with the wave-per-query rows), one local group each with
    the replicated postings, and the reference rows, computed once per call and read-only."""

    def __init__(self, tied, wide=False, small=False):
        import serenade_amd as sa
        import torch
        from serenade_amd import sharded
        from oracle import oracle as O
        t0 = time.time()
        self.torch, self.tied, self.wide = torch, tied, wide
        self.ix = ix = S.small_build() if small else S.build(tied)
        known, flags = (np.unique(ix.items), np.full(len(np.unique(ix.items)), S.ATTR_SALE, np.uint8)) if small else S.attributes(ix)
        _set_knobs(SRN_SBACK_MIN_SHARDS=2)
        try:
            self.full = sa.VMISIndex.from_sessions(ix.off, self.ids(ix.items), ix.ts, S.M_INDEX, S.ROW_MAX, 1.0, device=0)
            self.oix = O.OracleIndex(ix.off, ix.items, ix.ts, S.M_INDEX, S.ROW_MAX, 1.0, fast=True)
            self.full.set_attributes(self.ids(known), flags)
            self.oix.set_attributes(known, flags)
            self.view = sharded.postings_view(self.full)
            self.shards, self.grp = {}, {}
            for G in (2, 8):
                self.shards[G] = [sharded.ShardedVMISIndex.from_full(self.full, g, G) for g in range(G)]
                self.grp[G] = sharded.ShardGroup.local(self.shards[G])
                self.grp[G].set_postings(self.view)
        finally:
            _set_knobs()
        self.streams = set()
        self._ref, self._flat = {}, {}
        self.all = tuple(range(len(ix.queries)))
        self.seconds = time.time() - t0
        print("shard edge world (%s%s%s): %d sessions, %d queries, built in %.1f s" % ("tied" if tied else "distinct", ", full-width ids" if wide else "", ", small shards" if small else "", len(ix.ts), len(ix.queries), self.seconds))

    def ids(self, a):
        """Ids as the GPU sees them."""
        return E.wide_ids(a) if self.wide else np.asarray(a, dtype=np.uint64)

    def batch(self, queries):
        key = tuple(queries)
        if key not in self._flat:
            flat, off = flatten([self.ix.queries[qi] for qi in key])
            flat = self.ids(flat)
            t = self.torch
            self._flat[key] = (t.from_numpy(flat.view(np.int64).copy()).to("cuda:0"), t.from_numpy(off.view(np.int32).copy()).to("cuda:0"), len(key))
        return self._flat[key]

    def ref(self, call):
        """-> (the oracle's rows, the unsharded path's rows) over the whole batch."""
        import serenade_amd as sa
        if call not in self._ref:
            sh, how_many, business = CALLS[call]
            k, m = S.SHAPES[sh]
            flat, off = flatten(self.ix.queries)
            r = self.oix.predict_batch("canonical", flat, off, k, m, how_many, business, threads=8)
            u = sa.predict_batch(self.full, (self.ids(flat), off), k, m, how_many, business)
            if self.wide:
                r["ids"] = self.ids(r["ids"])
            for a in (r["ids"], r["scores"], r["counts"]) + tuple(u[:3]):
                a.setflags(write=False)
            self._ref[call] = (r, tuple(u[:3]))
        return self._ref[call]

    def serve(self, G, call, queries=None, stream=False):
        sh, how_many, business = CALLS[call]
        k, m = S.SHAPES[sh]
        if stream and G not in self.streams:          # (the fragments in posting order are copied when the postings are set under the knob)
            self.grp[G].set_postings(self.view)
            self.streams.add(G)
        d_flat, d_off, nq = self.batch(self.all if queries is None else queries)
        res = self.grp[G].predict_batch(d_flat, d_off, nq, S.MAX_LEN, k, m, how_many, business)
        self.torch.cuda.synchronize()
        return res[0].cpu().numpy().view(np.uint64), res[1].cpu().numpy(), res[2].cpu().numpy().view(np.uint32)

    def check(self, got, call, queries, what):
        r, u = self.ref(call)
        qs = np.array(self.all if queries is None else queries, np.int64)
        _vs_oracle(got, dict(ids=r["ids"][qs], scores=r["scores"][qs], counts=r["counts"][qs]), what)
        _same_bytes(got, tuple(a[qs] for a in u), what)
        inside = np.arange(got[0].shape[1])[None, :] < got[2][:, None].astype(np.int64)
        assert not got[0][~inside].any() and not got[1][~inside].any(), "%s: the unused tail of a row does not read 0" % what


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(tied, **kind):
        key = (tied,) + tuple(sorted(kind.items()))
        if key not in made:
            made[key] = World(tied, **kind)
        return made[key]
    yield get
    made.clear()
    _set_knobs()


def _cycles(shard, enable):
    from serenade_amd import capi
    out = np.zeros(16, np.uint64)
    capi.check(capi.lib().srn_debug_phase_cycles(shard._h, int(enable), capi.ptr(out)))
    return out


def _launches(shard):
    from serenade_amd import capi
    n = C.c_uint64()
    capi.check(capi.lib().srn_debug_sback_launches(shard._h, C.byref(n)))
    return n.value


def _exchanged(w, G):
    st = w.grp[G].stats
    return st["neighbour_batches"], st["bytes_neighbours"]


def _exchange_bytes(G, nq, call, stream):
    """What one batch of the neighbours pipeline ships in an in-process group: G blocks of ceil(nq / G) queries, k + 1 words of neighbour slots each -- or, in the
    streaming form, the position record's stride (srn_sback.hip, shard_nb_positions_stride: 2 + 8 ceil(m / 64) + ceil(k / 8) words, rounded up to an even number)."""
    k, m = S.SHAPES[CALLS[call][0]]
    stride = (2 + 8 * ((m + 63) // 64) + (min(k, S.F_K_MAX) + 7) // 8 + 1) // 2 * 2 if stream else k + 1
    return G * ((nq + G - 1) // G) * stride * 4


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
def test_rows_in_every_form(worlds, knobs, tied, G, call, form):
    """The whole designed batch through one form of the plumbing: the oracle's rows (scores to 1e-12), the unsharded path's bytes, tails of 0.  SRN_FAST_RUNS=3 is
    honoured by the group's front end (device_shard_nb_prep and the position kernel take fast_nb_of(n_kept, knobs), srn_runtime.hip:1082, :1097): the 29-bit-rank form,
    where nr = 3 / 4 switches `rel` (the cells "sumw=15" and "nr=4")."""
    w = worlds(tied)
    knobs(**FORMS[form])
    if form == "stream":
        w.serve(G, call, [0], stream=True)         # (the fragments in posting order are attached with the first call under the knob: outside the counted call)
    before, sent = _launches(w.shards[G][0]), _exchanged(w, G)
    got = w.serve(G, call, stream=form == "stream")
    w.check(got, call, None, "%s, G = %d, call %s" % (form, G, call))
    assert _launches(w.shards[G][0]) - before == (0 if form == "no_sback" else 1)
    # which form it was: one batch of the neighbours pipeline, and the bytes of ITS exchange -- position records in the streaming form, neighbour slots in every other
    after = _exchanged(w, G)
    assert after[0] - sent[0] == 1 and after[1] - sent[1] == _exchange_bytes(G, len(w.all), call, form == "stream"), (form, after[1] - sent[1])


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
def test_paths_are_the_restated_ones(worlds, knobs, tied, G, call, family):
    """One family per call, every shard's counters against the restatement: served queries (slot 14), hand-overs by cause (slot 15's three fields, slot 7's high half),
    live walks B (slot 7's low half), listed elements (slot 5) and the served queries' candidates (slot 6) -- exact integers, capacities at CAP and CAP + 1 included."""
    _paths(worlds(tied), knobs, tied, G, call, family, False)


@pytest.mark.parametrize("family", S.FAMILIES)
@pytest.mark.parametrize("call", ["A", "B"])
@pytest.mark.parametrize("G", [2, 8])
def test_paths_in_the_streaming_form(worlds, knobs, G, call, family):
    """The same counters from vmis_shard_back_kernel<STREAM>, which reads the neighbours as positions in the posting lists (kept prefixes of 63 / 64 / 65 and 640 / 641
    entries, neighbours of two lists marked in the first, a run with nothing kept): the position records describe exactly K neighbours, so no query is handed over for
    nmem != K and every count is the gather form's.  That the call streamed is asserted from the bytes of its exchange."""
    _paths(worlds(True), knobs, True, G, call, family, True)


def _paths(w, knobs, tied, G, call, family, stream):
    sh, how_many, business = CALLS[call]
    unsure = set(S.uncertain_queries(tied, G))
    queries = [qi for qi in S.family_queries(w.ix, family) if qi not in unsure]
    R = S.restate(tied, sh, how_many, G, business)
    knobs(SRN_NO_SBACK_SECOND=1, **({"SRN_SBACK_STREAM": 1} if stream else {}))
    if stream:
        w.serve(G, call, [0], stream=True)
    sent = _exchanged(w, G)
    for s in w.shards[G]:
        _cycles(s, 1)
    try:
        got = w.serve(G, call, queries, stream=stream)
    finally:
        cyc = [_cycles(s, 0) for s in w.shards[G]]
    after = _exchanged(w, G)
    assert after[0] - sent[0] == 1 and after[1] - sent[1] == _exchange_bytes(G, len(queries), call, stream)
    w.check(got, call, queries, "%s, G = %d, call %s" % (family, G, call))
    for g in range(G):
        want = S.counters(R, queries, g)
        c = [int(x) for x in cyc[g]]
        have = dict(c5=c[5], c6=c[6], c14=c[14], c7_live=c[7] & 0xFFFFFFFF, c7_table=c[7] >> 32, c15=(c[15] & 0xFFFFF, (c[15] >> 20) & 0xFFFFF, c[15] >> 40))
        print("%s shard %d of %d: %s" % (family, g, G, have))
        for key, v in have.items():
            assert v == want[key], "%s, shard %d of %d, call %s: %s is %s, restated %s; per query: %s" % (
                family, g, G, call, key, v, want[key], [(w.ix.cells[w.ix.q_cell[qi]]["name"], R[qi][g]["outcome"]) for qi in queries])


@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
def test_the_tier_behind_gets_exactly_the_handed_over_queries(worlds, knobs, tied, G):
    """The default pass: what the wave cannot hold goes on the list of the fast kernel's back-end form -- srn_debug_last_mid_count per shard is the restated number of
    hand-overs -- and the kernel is launched once per call."""
    from serenade_amd import capi
    w = worlds(tied)
    knobs()
    unsure = set(S.uncertain_queries(tied, G))
    queries = [qi for qi in w.all if qi not in unsure]
    for call in CALLS:
        sh, how_many, business = CALLS[call]
        R = S.restate(tied, sh, how_many, G, business)
        before = [_launches(s) for s in w.shards[G]]
        got = w.serve(G, call, queries)
        w.check(got, call, queries, "default pass, G = %d, call %s" % (G, call))
        for g, s in enumerate(w.shards[G]):
            listed = C.c_uint32()
            capi.check(capi.lib().srn_debug_last_mid_count(s._h, C.byref(listed)))
            assert listed.value == S.counters(R, queries, g)["listed"], (g, call, listed.value)
            assert _launches(s) - before[g] == 1


@pytest.mark.parametrize("G", [2, 8])
@pytest.mark.parametrize("tied", [False, True], ids=["distinct", "tied"])
def test_capacity_cells_alone_and_in_front_of_a_light_cell(worlds, knobs, tied, G):
    """Every capacity cell as a batch of one query and as the first of two with a light cell behind it, with and without the tier behind.  A batch this small gets one
    wave per query, so a third pass serves [cell, light, K=1536] under SRN_ORDER_MIN=1: an ordered batch of up to 256 queries is ONE wave's (the grid is 8 waves, one
    per XCD, and the first chunk of the order is XCD 0's), in the order of the queries' most popular items -- the cell's lies between the other two, so a served query
    stands directly behind it, where what a handed-over query leaves in the wave's LDS would show."""
    w = worlds(tied)
    by_name = {w.ix.cells[ci]["name"]: qi for qi, ci in enumerate(w.ix.q_cell)}
    light, heavy = by_name["light"], by_name["K=%d" % S.F_K_MAX]
    for kn, batches in (({"SRN_NO_SBACK_SECOND": 1}, 2), ({}, 2), ({"SRN_ORDER_MIN": 1}, 3)):
        knobs(**kn)
        for qi in S.family_queries(w.ix, "capacity"):
            c = w.ix.cells[w.ix.q_cell[qi]]
            call = "B" if c["business"] else "A"
            for queries in ([[qi], [qi, light]] if batches == 2 else [[qi, light, heavy]]):
                w.check(w.serve(G, call, queries), call, queries, "%s (%d queries, %s), G = %d" % (c["name"], len(queries), kn, G))


@pytest.mark.parametrize("form", ["gather", "no_second", "ordered", "stream"])
@pytest.mark.parametrize("G", [2, 8])
def test_small_shards(worlds, knobs, G, form):
    """Shards of 0, 1, 15 / 16 / 17 and 255 / 256 / 257 items (at G = 2: 288 and 529): the sample is padded with zero records and guarded by e < n_items, the floor
    chunks beyond the shard's last item are empty, and the shard with no item at all adds nothing to any row -- the rows are the oracle's and the unsharded path's."""
    w = worlds(False, small=True)
    knobs(**FORMS[form])
    for call in ("A", "B"):
        if form == "stream":
            w.serve(G, call, [0], stream=True)
        sent = _exchanged(w, G)
        w.check(w.serve(G, call, stream=form == "stream"), call, None, "small shards, %s, G = %d, call %s" % (form, G, call))
        after = _exchanged(w, G)
        assert after[0] - sent[0] == 1 and after[1] - sent[1] == _exchange_bytes(G, len(w.all), call, form == "stream"), (form, after[1] - sent[1])
    assert int(w.ref("A")[0]["counts"].max()) == 21 and int((w.ref("A")[0]["counts"] > 0).sum()) > 80


@pytest.mark.parametrize("form", ["gather", "no_second"])
def test_full_width_ids(worlds, knobs, form):
    """The designed index and its batch under edge_cases.wide_ids (strictly increasing: the oracle's rows are the narrow index's with the map applied -- asserted on the
    CPU by tests/test_edge_cases_host.py): both 32-bit halves of every id are live, and the back end's hand-off record carries id RANKS that the finish kernels turn
    back into ids.  The map gives every item another owner, so nothing of the design is restated here: rows only, at 8 shards."""
    w = worlds(True, wide=True)
    knobs(**FORMS[form])
    for call in ("A", "B"):
        w.check(w.serve(8, call), call, None, "full-width ids, %s, call %s" % (form, call))


@pytest.mark.parametrize("G", [2, 8])
def test_calls_that_are_not_this_kernels(worlds, knobs, G):
    """Two calls around the neighbours pipeline, pinned for their rows.  m = 2 561, one past F_M_MAX: the group serves the batch through the lists pipeline (no
    neighbours batch is counted) with the rows of m = 2 560 -- no list of the index has more than 1 536 sessions.  A session of nine items at max_len = 8: no front end
    takes it and it is nobody's query; the group gives it what the unsharded device call gives it, and the rows around it are untouched."""
    import serenade_amd as sa
    w, t = worlds(False), worlds(False).torch
    knobs()
    k, m = S.SHAPES[1]
    sent = _exchanged(w, G)
    d_flat, d_off, nq = w.batch(w.all)
    res = w.grp[G].predict_batch(d_flat, d_off, nq, S.MAX_LEN, k, m + 1, 21, False)
    t.cuda.synchronize()
    w.check((res[0].cpu().numpy().view(np.uint64), res[1].cpu().numpy(), res[2].cpu().numpy().view(np.uint32)), "A", None, "m = %d, G = %d" % (m + 1, G))
    assert _exchanged(w, G) == sent, "a batch with m > F_M_MAX went through the neighbours pipeline"
    by_name = {w.ix.cells[ci]["name"]: qi for qi, ci in enumerate(w.ix.q_cell)}
    nine = [S.UNKNOWN0 + 5000 + j for j in range(8)] + [w.ix.queries[by_name["light"]][-1]]
    qs = [w.ix.queries[by_name["K=63"]], nine, w.ix.queries[by_name["light"]]]
    flat, off = flatten(qs)
    d_flat, d_off = t.from_numpy(flat.view(np.int64).copy()).to("cuda:0"), t.from_numpy(off.view(np.int32).copy()).to("cuda:0")
    res = w.grp[G].predict_batch(d_flat, d_off, 3, S.MAX_LEN, k, m, 21, False)
    o = (t.zeros(3 * 21, dtype=t.int64, device="cuda:0"), t.zeros(3 * 21, dtype=t.float64, device="cuda:0"), t.zeros(3, dtype=t.int32, device="cuda:0"))
    sa.predict_batch_device(w.full, d_flat.data_ptr(), d_off.data_ptr(), 3, S.MAX_LEN, k, m, 21, False, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    got = [a.cpu().numpy().reshape(3, -1) for a in res[:2]] + [res[2].cpu().numpy().view(np.uint32)]
    ref = [a.cpu().numpy().reshape(3, -1) for a in o[:2]] + [o[2].cpu().numpy().view(np.uint32)]
    print("a session of nine items at max_len 8: count %#x in the group, %#x unsharded" % (int(got[2][1]), int(ref[2][1])))
    assert np.array_equal(got[2], ref[2]), (got[2], ref[2])
    for j in (0, 2):
        assert np.array_equal(got[0][j], ref[0][j]) and np.array_equal(got[1][j].view(np.uint64), ref[1][j].view(np.uint64))
        assert got[2][j] == w.ref("A")[0]["counts"][[by_name["K=63"], 0, by_name["light"]][j]]
