"""The fast kernel parks the NEXT query's prep record in LDS while it serves the current one (srn_fast.hip, `pre`): wave 1 requests it in walk A with a load the compiler
does not count and waits for it by hand at the end of phase 4a; a query that leaves before walk A (no known item, handed on to MID / BIG / LONG / the general kernel)
requests nothing -- its successor reads its record from global memory.  A workgroup's queries form a chain through that one LDS area, so what is checked here is chains: batches of 4 096 queries
of the `tiny` config at SRN_GRID_MULT=1 (every workgroup serves several queries) whose order mixes sessions of 1..8 items (8 items: the record's second 256 bytes),
one-list queries next to four-list ones, queries without a known item and sessions of 9-10 items in between (the chain breaks and resumes), every workgroup's last query;
unordered and in the serving order (SRN_ORDER_MIN=1: merged duplicates, each XCD's last entry).  Rows are compared with the canonical oracle (ids and order exact, scores
to 1e-12) and, bit for bit, with a run of one query per workgroup, which parks nothing at all.
"""
import os

import numpy as np
import pytest

from helpers import flatten

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-12
KNOBS = ("SRN_GRID_MULT", "SRN_ORDER_MIN", "SRN_NO_DEDUP")
NQ, MAX_LEN, N = 4096, 10, 21


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


def _chain_batch(pop, rng, nq=NQ):
    """nq sessions in random order (a workgroup's chain is a stride through the batch, or a run of the sorted order: every kind gets every kind as its neighbour).
    pop: the index's item ids, most popular first."""
    w = 1.0 / np.arange(1, len(pop) + 1) ** 0.9
    w /= w.sum()
    known = lambda c: [int(x) for x in pop[rng.choice(len(pop), size=c, replace=False, p=w)]]   # noqa: E731  (distinct known items)
    beyond = int(pop.max()) + 1
    unknown = lambda c: [beyond + int(x) for x in rng.integers(0, 1000, size=c)]                    # noqa: E731  (ids the index has never seen)
    qs = []
    for i in range(nq):
        kind = i % 16
        if kind < 5:      # one list, sessions of 1..8 items: the known item oldest, unknown ids behind it
            ln = int(rng.integers(1, 9))
            q = known(1) + unknown(ln - 1)
        elif kind < 9:    # four lists, 4..8 items: the known items oldest (their numerators sum to 10), unknown ids behind them
            ln = int(rng.integers(4, 9))
            q = known(4) + unknown(ln - 4)
        elif kind < 11:   # two or three lists, all items known, an item repeated now and then
            c = int(rng.integers(2, 4))
            q = known(c)
            if rng.random() < 0.3:
                q = q + [q[0]]
        elif kind == 11:  # eight items, the full record (its eighth item lies in the second 256 bytes): four or two known items oldest
            q = known(4) + unknown(4) if rng.random() < 0.5 else known(2) + unknown(6)
        elif kind == 12:  # no known item: empty result, nothing parked
            q = unknown(int(rng.integers(1, 9)))
        elif kind == 13:  # 9-10 items: handed on to the MID form, nothing parked
            c = int(rng.integers(5, 8))
            q = known(c) + unknown(int(rng.integers(9, 11)) - c)
        elif kind == 14:  # a copy of an earlier session (merged in the serving order)
            q = list(qs[int(rng.integers(0, len(qs)))])
        else:             # short sessions of popular items: full lists, both cuts bite
            q = [int(x) for x in pop[rng.choice(40, size=int(rng.integers(1, 5)), replace=False)]]
        qs.append(q)
    order = rng.permutation(nq)
    return [qs[i] for i in order]


class _Device:
    """One batch on the device and device-resident calls over it: rows come back as numpy arrays (ids u64[nq, n], scores f64[nq, n], counts u32[nq])."""

    def __init__(self, gix, qs):
        import torch
        self.torch, self.gix, self.nq = torch, gix, len(qs)
        flat, off = flatten(qs)
        self.dev = torch.device("cuda:0")
        self.d_flat = torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to(self.dev)
        self.d_off = torch.from_numpy(off.view(np.int32).copy()).to(self.dev)

    def buffers(self):
        t = self.torch
        return t.zeros(self.nq * N, dtype=t.int64, device=self.dev), t.zeros(self.nq * N, dtype=t.float64, device=self.dev), t.zeros(self.nq, dtype=t.int32, device=self.dev)

    def call(self, k, m, out=None, sync=True):
        import serenade_amd as sa
        o = out if out is not None else self.buffers()
        sa.predict_batch_device(self.gix, self.d_flat.data_ptr(), self.d_off.data_ptr(), self.nq, MAX_LEN, k, m, N, False,
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), self.torch.cuda.current_stream().cuda_stream, resident=True)
        if not sync:
            return o
        self.torch.cuda.synchronize()
        return self.rows(o)

    def rows(self, o):
        return (o[0].cpu().numpy().view(np.uint64).reshape(-1, N)[:self.nq].copy(), o[1].cpu().numpy().reshape(-1, N)[:self.nq].copy(), o[2].cpu().numpy().view(np.uint32)[:self.nq].copy())


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
def chains():
    """The `tiny` index, two batches on the device and their oracle rows (computed once, shared, never changed)."""
    import serenade_amd as sa
    from serenade_amd import synth
    from oracle import oracle as O
    inter, n_items, k, m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    gix = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0)
    oix = O.OracleIndex(off, items, ts, m, 34, idfw, fast=True)
    ids, counts = np.unique(items, return_counts=True)
    pop = ids[np.argsort(-counts, kind="stable")]
    out = []
    for seed in (11, 12):
        qs = _chain_batch(pop, np.random.default_rng(seed))
        flat, qoff = flatten(qs)
        ref = oix.predict_batch("canonical", flat, qoff, k, m, N, False, threads=4)
        out.append((qs, _Device(gix, qs), ref))
    return gix, k, m, out


def _fast_share(gix, nq, what):
    """Condition, not a measurement: the batch is the fast tiers' -- the lean form and the MID / BIG / LONG forms it hands on to -- not the general kernel's."""
    got_nq, general, _glob = gix.last_path_counts()
    mid = gix.last_mid_count()
    print("%s: %d queries, %d listed for the MID form, %d reached the general kernel" % (what, got_nq, mid, general))
    assert got_nq == nq
    assert nq - general >= 0.8 * nq, "%s: only %d of %d queries were served by the fast tiers" % (what, nq - general, nq)
    return mid


@pytest.mark.parametrize("order_min", [None, 1])
def test_chains_against_the_oracle_and_one_query_per_workgroup(chains, knobs, order_min):
    gix, k, m, batches = chains
    qs, dv, ref = batches[0]
    knobs(SRN_GRID_MULT=64, SRN_ORDER_MIN=order_min)   # more workgroups than queries: one query each, nothing is parked
    single = dv.call(k, m)
    _vs_oracle(single, ref, "one query per workgroup")
    knobs(SRN_GRID_MULT=1, SRN_ORDER_MIN=order_min)    # one workgroup per resident slot: chains of several queries
    got = dv.call(k, m)
    mid = _fast_share(gix, len(qs), "chains, SRN_ORDER_MIN=%s" % order_min)
    assert mid > 0, "no session of 9-10 items was handed on: the chains never broke"
    if order_min:
        assert gix.last_dedup_count() > 0, "no query was merged in the serving order"
    _vs_oracle(got, ref, "chains")
    _same_bytes(got, single, "chains against one query per workgroup")


def test_eight_calls_alternating_two_batches(chains, knobs):
    """A workgroup's parked record must never outlive its call: two batches alternate for eight device-resident calls in one process, the result buffers reused; every
    call's rows are read back behind it on the stream and are the same bytes call after call (and the first call of each batch is the oracle's)."""
    import torch
    gix, k, m, batches = chains
    knobs(SRN_GRID_MULT=1)
    nmax = max(b[1].nq for b in batches)
    shared = (torch.zeros(nmax * N, dtype=torch.int64, device="cuda:0"), torch.zeros(nmax * N, dtype=torch.float64, device="cuda:0"), torch.zeros(nmax, dtype=torch.int32, device="cuda:0"))
    copies = []
    for call in range(8):
        dv = batches[call % 2][1]
        dv.call(k, m, out=shared, sync=False)
        copies.append(tuple(t.clone() for t in shared))   # (on the same stream: behind the call, before the next one overwrites the buffers)
    torch.cuda.synchronize()
    _fast_share(gix, batches[1][1].nq, "the eighth call")
    first = [None, None]
    for call, c in enumerate(copies):
        qs, dv, ref = batches[call % 2]
        rows = dv.rows(c)
        if first[call % 2] is None:
            first[call % 2] = rows
            _vs_oracle(rows, ref, "call %d" % call)
        else:
            _same_bytes(rows, first[call % 2], "call %d against call %d" % (call, call % 2))
