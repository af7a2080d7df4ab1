"""The launch-ready block of the prep record (PrepHead::ready, srn_kernels.h): 16 words per query -- the lean form's routing predicate `lean_ok`, its run count, which of
the 20 stage loads exist, and the runs' kept counts, positions and list starts -- written once by the prep kernel so that vmis_fast_kernel's lean forms start their posting-list
loads from readlanes of it instead of decoding the record's items in every wave.

(a) Record level: srn_debug_prep_records runs the prep kernel alone; the 16 words of every query are recomputed here with numpy from the LEGACY fields of the same records
(head words 0..17 and the items' kept / base / idx) and from the predicate as the kernel states it, and compared word by word.
(b) End to end: the same batch through srn_predict_batch_device against the canonical oracle (ids and order exact, scores to 1e-12) and, bit for bit, against a run with
SRN_NO_FAST=1 -- as chains per workgroup (SRN_GRID_MULT=1: records read from the parked LDS copy), one query per workgroup (records read from global memory), in the
serving order (SRN_ORDER_MIN=1) and in the 29-bit-rank form (SRN_FAST_RUNS=3: the block's `rel` bit).  The MID / BIG hand-over counts must be what the predicate says.

The batch: 4 096 sessions of the `tiny` data set over an index built with m = 2 048 (tiny's own m = 500 keeps every list under 512 entries: no edge of the load mask).
Sessions of 1..8 items; an item repeated (the older occurrence owns no run); unknown ids at every position, the most recent included; only unknown ids (n = 0); 5+ distinct
known items (nr > 4); 8 items with numerators summing above 15; 9 and 12 items (L > 8: the block is zero); lists cut by x_lo to kept = 1 and to the nearest the index
has to 512 / 513 / 1 024 / 1 025 (found by a first pass over pairs of popular items: the test prints what it reached and requires a kept count on either side of 512
and of 1 024 -- this index reaches 1, 510, 514, 1 021 and 1 029; the exact edges 512 / 513 / 1 024 no pair of its items has: tests/test_gpu_edge_cases.py places every
multiple of 512 up to 2 560, one below and one above, on a designed index, tests/edge_cases.py); the hottest items four at a time, and four at a time the most popular items with FEWER than m sessions (they set no cut: the largest n).
Which side of 2 n + 8 <= MW (12 032 words) the index reaches: both -- the second kind of four-item sessions stages up to 7 014 entries and goes to the BIG form; the
test requires both sides among the queries that pass every other term.  (The latency path's one-workgroup launches write a zero block and decode the items themselves,
srn_fast.hip: a zero block is always valid -- lean_ok clear -- and the existing latency tests cover that form.)
"""
import os

import numpy as np
import pytest

from helpers import flatten
from record_cases import K_NONE, MW_LEAN, READY0, READY_WORDS, legacy, prep_records, ready_from_legacy, routing   # (the record's layout and the ONE statement of the routing: shared with tests/test_gpu_edge_cases.py)

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-12
KNOBS = ("SRN_GRID_MULT", "SRN_ORDER_MIN", "SRN_NO_FAST", "SRN_FAST_RUNS")
NQ, MAX_LEN, N, M = 4096, 12, 21, 2048


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


def _batch(pop, counts, edges, rng, nq=NQ):
    """pop: the index's item ids, most popular first; counts: their session counts; edges: sessions found by the first pass (kept at the load mask's edges)."""
    w = 1.0 / np.arange(1, len(pop) + 1) ** 0.9
    w /= w.sum()
    known = lambda c: [int(x) for x in pop[rng.choice(len(pop), size=c, replace=False, p=w)]]   # noqa: E731  (distinct known items)
    beyond = int(pop.max()) + 1
    unknown = lambda c: [beyond + int(x) for x in rng.integers(0, 1000, size=c)]                    # noqa: E731  (ids the index has never seen)
    under_m = np.flatnonzero(counts < M)[:8]                                                        # the most popular items that set no cut
    qs = []
    for i in range(nq):
        kind = i % 16
        if kind < 4:      # 1..8 items, every position unknown with probability 0.3 (the most recent included)
            ln = int(rng.integers(1, 9))
            kn = known(ln)
            q = [unknown(1)[0] if rng.random() < 0.3 else kn[j] for j in range(ln)]
        elif kind == 4:   # an item repeated: its older occurrence owns no run
            q = known(int(rng.integers(2, 5)))
            q = [q[-1]] + q if rng.random() < 0.5 else q[:1] + q + unknown(1)
        elif kind == 5:   # only unknown ids: n = 0
            q = unknown(int(rng.integers(1, 9)))
        elif kind == 6:   # 5..8 distinct known items: nr > 4
            q = known(int(rng.integers(5, 9)))
        elif kind == 7:   # 8 items, the three most recent known: numerators 8 + 7 + 6 > 15 with three runs
            q = unknown(5) + known(3)
        elif kind == 8:   # 9 and 12 items: L > 8, the block is zero
            c = int(rng.integers(2, 6))
            q = known(c) + unknown((9 if i % 32 < 16 else 12) - c)
        elif kind == 9:   # four of the hottest items / of the most popular items without a full list (the largest n), now and then with an unknown id on top
            src = under_m if i % 32 < 16 else np.arange(8)
            q = [int(x) for x in pop[rng.choice(src, size=4, replace=False)]]
            if rng.random() < 0.3:
                q = q + unknown(1)
        elif kind in (10, 11):   # the load mask's edges, as they are and shifted by an unknown most recent item
            q = list(edges[(i // 16) % len(edges)])
            if kind == 11:
                q = q + unknown(1)
        elif kind == 12:  # one list: the known item oldest
            q = known(1) + unknown(int(rng.integers(0, 8)))
        elif kind == 13 and qs:  # a copy of an earlier session (merged in the serving order)
            q = list(qs[int(rng.integers(0, len(qs)))])
        else:             # short sessions of popular items: full lists, both cuts bite
            q = [int(x) for x in pop[rng.choice(40, size=int(rng.integers(1, 5)), replace=False)]]
        qs.append(q)
    order = rng.permutation(nq)
    return [qs[i] for i in order]


def _edge_sessions(gix, pop):
    """First pass: sessions [b, a] of a popular item b under the cut of a hotter item a (the most recent), and what the prep kernel keeps of b's list."""
    cand = [[int(pop[b]), int(pop[a])] for a in range(12) for b in range(64) if a != b] + [[int(pop[b]), int(pop[a])] for a in range(3) for b in range(64, 1024)]
    f = legacy(prep_records(gix, cand, M, MAX_LEN), MAX_LEN)
    kept_b = f["kept"][:, 1]
    found = {}
    for name, target, below in (("1", 1, True), ("<=512", 512, True), (">=513", 513, False), ("<=1024", 1024, True), (">=1025", 1025, False)):
        ok = np.flatnonzero((kept_b <= target) & (kept_b > 0) if below else kept_b >= target)
        assert len(ok), "no pair of popular items keeps %s entries" % name
        best = ok[np.argmin(np.abs(kept_b[ok] - target))]
        found[name] = (cand[best], int(kept_b[best]))
    return found


class _Device:
    """One batch on the device and device-resident calls over it: rows come back as numpy arrays (ids u64[nq, n], scores f64[nq, n], counts u32[nq])."""

    def __init__(self, gix, qs):
        import torch
        self.torch, self.gix, self.nq = torch, gix, len(qs)
        flat, off = flatten(qs)
        self.dev = torch.device("cuda:0")
        self.d_flat = torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to(self.dev)
        self.d_off = torch.from_numpy(off.view(np.int32).copy()).to(self.dev)

    def call(self, k, m):
        import serenade_amd as sa
        t = self.torch
        o = (t.zeros(self.nq * N, dtype=t.int64, device=self.dev), t.zeros(self.nq * N, dtype=t.float64, device=self.dev), t.zeros(self.nq, dtype=t.int32, device=self.dev))
        sa.predict_batch_device(self.gix, self.d_flat.data_ptr(), self.d_off.data_ptr(), self.nq, MAX_LEN, k, m, N, False,
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), t.cuda.current_stream().cuda_stream, resident=True)
        t.cuda.synchronize()
        return (o[0].cpu().numpy().view(np.uint64).reshape(-1, N).copy(), o[1].cpu().numpy().reshape(-1, N).copy(), o[2].cpu().numpy().view(np.uint32).copy())


def _same_bytes(got, ref, what):
    ids, sc, cnt = got
    rids, rsc, rcnt = ref
    assert np.array_equal(cnt, rcnt), "%s: counts differ at %s" % (what, np.flatnonzero(cnt != rcnt)[:8])
    inside = np.arange(N)[None, :] < np.minimum(cnt, N).astype(np.int64)[:, None]
    assert np.array_equal(ids[inside], rids[inside]), "%s: ids differ" % what
    assert np.array_equal(sc[inside].view(np.uint64), rsc[inside].view(np.uint64)), "%s: scores differ in their bits" % what


def _vs_oracle(got, ref, what):
    ids, sc, cnt = got
    assert np.array_equal(cnt, ref["counts"]), "%s: counts differ from the oracle at %s" % (what, np.flatnonzero(cnt != ref["counts"])[:8])
    inside = np.arange(N)[None, :] < ref["counts"][:, None].astype(np.int64)
    assert np.array_equal(ids[inside], ref["ids"][inside]), "%s: ranked ids differ from the oracle" % what
    np.testing.assert_allclose(sc[inside], ref["scores"][inside], rtol=SCORE_RTOL, atol=0)


@pytest.fixture(scope="module")
def world():
    """The `tiny` sessions under an index of m = 2 048, the batch on the device, its oracle rows and its rows without the fast kernels (computed once, shared, never changed)."""
    import serenade_amd as sa
    from serenade_amd import synth, capi
    from oracle import oracle as O
    inter, n_items, k, _m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    gix = sa.VMISIndex.from_sessions(off, items, ts, M, 34, idfw, device=0)
    oix = O.OracleIndex(off, items, ts, M, 34, idfw, fast=True)
    ids, counts = np.unique(items, return_counts=True)
    by_pop = np.argsort(-counts, kind="stable")
    pop, counts = ids[by_pop], counts[by_pop]
    edges = _edge_sessions(gix, pop)
    print("kept counts at the load mask's edges: " + ", ".join("%s -> %d" % (name, kept) for name, (_s, kept) in edges.items()))
    qs = _batch(pop, counts, [s for s, _kept in edges.values()], np.random.default_rng(23))
    flat, qoff = flatten(qs)
    ref = oix.predict_batch("canonical", flat, qoff, k, M, N, False, threads=4)
    dv = _Device(gix, qs)
    os.environ["SRN_NO_FAST"] = "1"
    capi.reload_knobs()
    try:
        slow = dv.call(k, M)
    finally:
        os.environ.pop("SRN_NO_FAST", None)
        capi.reload_knobs()
    return dict(gix=gix, k=k, qs=qs, dv=dv, ref=ref, slow=slow, edges=edges)


@pytest.mark.parametrize("wide", [False, True])
def test_every_word_of_every_query(world, knobs, wide):
    knobs(SRN_FAST_RUNS=3 if wide else None)
    rec = prep_records(world["gix"], world["qs"], M, MAX_LEN)
    got, want = rec[:, READY0:READY0 + READY_WORDS], ready_from_legacy(rec, wide, MAX_LEN)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, "%d records differ, the first: query %d %s\n got  %s\n want %s" % (len(bad), bad[0], world["qs"][bad[0]], got[bad[0]], want[bad[0]])
    # what the batch holds (conditions, so that the comparison above is about something)
    f = legacy(rec, MAX_LEN)
    L, nr = f["L"], (f["kept"][:, :8] > 0).sum(axis=1)
    ok = got[:, 0] & 1
    assert set(range(1, 9)) <= set(L[ok == 1].tolist()) and {9, 12} <= set(L.tolist())
    assert ((L <= 8) & (nr > 4)).any() and ((L == 8) & (f["sumw"] > 15) & (nr <= 4)).any() and ((L <= 8) & (f["n"] == 0)).any()
    assert ((L >= 2) & (L <= 8) & (f["idx"][:, 0] == K_NONE) & (nr > 0)).any(), "no session with an unknown most recent item and a run"
    assert (got[(L > 8) | (nr > 4)] == 0).all()
    kept = got[:, 4:8][ok == 1]
    for lo, hi in ((1, 1), (1, 512), (513, 1024), (1025, 1536), (1537, 2048)):   # a kept count in every class of the load mask
        assert ((kept >= lo) & (kept <= hi)).any(), "no lean query keeps %d..%d entries of a list" % (lo, hi)
    e = world["edges"]
    assert e["1"][1] == 1 and e["<=512"][1] <= 512 < e[">=513"][1] and e["<=1024"][1] <= 1024 < e[">=1025"][1]
    rest = (f["unsafe"] == 0) & (L >= 1) & (L <= 8) & (f["sumw"] <= 15) & (nr <= 4)   # every term of lean_ok but the merge room
    assert (rest & (2 * f["n"] + 8 <= MW_LEAN)).any() and (rest & (2 * f["n"] + 8 > MW_LEAN)).any(), "one side of 2 n + 8 <= MW only"
    assert wide == bool(((got[:, 0] >> 16) & 1).any()), "the rel bit follows the 29-bit-rank form"
    print("wide=%s: %d of %d lean_ok, %d with 4 runs, largest n %d" % (wide, int(ok.sum()), len(rec), int((nr[ok == 1] == 4).sum()), int(f["n"][L <= 8].max())))


@pytest.mark.parametrize("how", ["chains", "single", "ordered", "wide"])
def test_rows_and_routing(world, knobs, how):
    gix, dv, qs = world["gix"], world["dv"], world["qs"]
    wide = how == "wide"
    knobs(SRN_GRID_MULT=64 if how == "single" else 1, SRN_ORDER_MIN=1 if how == "ordered" else None, SRN_FAST_RUNS=3 if wide else None)
    rec = prep_records(gix, qs, M, MAX_LEN)
    got = dv.call(world["k"], M)
    nq, general, _glob = gix.last_path_counts()
    mid, big, merged = gix.last_mid_count(), gix.last_big_count(), gix.last_dedup_count()
    _vs_oracle(got, world["ref"], how)
    _same_bytes(got, world["slow"], "%s against SRN_NO_FAST=1" % how)
    # the routing is the predicate's: over the queries that were served themselves (a copy of an earlier query of the call is not, where the call merges them)
    route = routing(rec, MAX_LEN, wide)
    seen, served = set(), []
    for q, s in enumerate(qs):
        if merged and tuple(s) in seen:
            continue
        seen.add(tuple(s))
        served.append(route[q])
    if merged:
        assert merged == len(qs) - len(served)
    want_mid = sum(r.startswith("mid") for r in served)
    want_big = sum(r in ("big", "mid>big") for r in served)
    print("%s: %d queries, %d merged, lean %d, MID %d (want %d), BIG %d (want %d), general %d" % (how, nq, merged, served.count("lean"), mid, want_mid, big, want_big, general))
    assert nq == len(qs) and (mid, big) == (want_mid, want_big)
    assert served.count("lean") >= 0.6 * len(served) and want_mid > 0 and want_big > 0
