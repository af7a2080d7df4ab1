"""Shared by the GPU tests over the designed index of tests/edge_cases.py (test_gpu_edge_cases.py, test_gpu_persistent_edges.py): one World per timestamp variant -- the
index on the GPU and in the oracle, the batch on the device, the reference rows, each computed once and never changed -- the two row comparisons, and the fixture that
switches the SRN_* knobs.  A plain module beside edge_cases.py; the test modules import what they use (the `knobs` fixture too).  Test-side only."""
import os
import time

import numpy as np
import pytest

import edge_cases as E
from fill_cases import draw_attrs
from helpers import flatten

SCORE_RTOL = 1e-12   # (as tests/test_gpu_parity.py: one f64 multiply + divide of an exact integer accumulator on both sides)
KNOBS = ("SRN_GRID_MULT", "SRN_ORDER_MIN", "SRN_NO_FAST", "SRN_FAST_RUNS", "SRN_NO_MID", "SRN_NO_BIG", "SRN_NO_LONG", "SRN_TINY_FUSED")


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
    """One timestamp variant: the index on the GPU and in the oracle, the batch on the device, and the reference rows, each computed once and never changed.
    wide_ids: everything the GPU sees -- the index, the attributes, the queries -- goes through edge_cases.wide_ids, and so do the ids of the reference rows; the oracle
    itself stays on the narrow ids (the map is strictly increasing: tests/test_edge_cases_host.py compares the oracle on the mapped index with that, row for row)."""

    def __init__(self, tied, wide_ids=False):
        import serenade_amd as sa
        import torch
        from oracle import oracle as O
        t0 = time.time()
        self.torch, self.tied, self.wide = torch, tied, wide_ids
        self.ix = ix = E.build(tied)
        self.gix = sa.VMISIndex.from_sessions(ix.off, self.ids(ix.items), ix.ts, E.M_INDEX, E.ROW_MAX, 1.0, device=0)
        self.oix = O.OracleIndex(ix.off, ix.items, ix.ts, E.M_INDEX, E.ROW_MAX, 1.0, fast=True)
        known, flags = draw_attrs(ix.items)
        self.gix.set_attributes(self.ids(known), flags)
        self.oix.set_attributes(known, flags)
        self.narrow_qs = ix.queries
        self.qs, self.nq = [self.session(q) for q in ix.queries], len(ix.queries)
        self.narrow_flat, self.off = flatten(self.narrow_qs)
        self.flat = self.ids(self.narrow_flat)
        self.d_flat = torch.from_numpy(np.concatenate([self.flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to("cuda:0")
        self.d_off = torch.from_numpy(self.off.view(np.int32).copy()).to("cuda:0")
        self._ref, self._slow = {}, {}
        self.seconds = time.time() - t0

    def ids(self, a):
        """Ids as the GPU sees them."""
        return E.wide_ids(a) if self.wide else np.asarray(a, dtype=np.uint64)

    def session(self, q):
        return [int(x) for x in self.ids(q)]

    def ref(self, k, m, how_many=21, business=False):
        key = (k, m, how_many, business)
        if key not in self._ref:
            r = self.oix.predict_batch("canonical", self.narrow_flat, self.off, k, m, how_many, business, threads=8, want_stats=True)
            if self.wide:
                r["ids"] = self.ids(r["ids"])
            for a in (r["ids"], r["scores"], r["counts"], r["stats"]):
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def ref_one(self, q, k, m, how_many=21, business=False):
        """The oracle's row for one NARROW session outside the batch -> (ids as the GPU sees them, scores)."""
        ids, sc = self.oix.predict_canonical(q, k, m, how_many, business)[:2]
        return self.ids(ids), np.asarray(sc, np.float64)

    def call(self, k, m, how_many=21, business=False):
        """srn_predict_batch_device over the resident batch -> (ids u64[nq, n], scores f64[nq, n], counts u32[nq])."""
        import serenade_amd as sa
        t = self.torch
        o = (t.zeros(self.nq * how_many, dtype=t.int64, device="cuda:0"), t.zeros(self.nq * how_many, dtype=t.float64, device="cuda:0"), t.zeros(self.nq, dtype=t.int32, device="cuda:0"))
        sa.predict_batch_device(self.gix, self.d_flat.data_ptr(), self.d_off.data_ptr(), self.nq, E.MAX_LEN, k, m, how_many, business,
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), t.cuda.current_stream().cuda_stream, resident=True)
        t.cuda.synchronize()
        return (o[0].cpu().numpy().view(np.uint64).reshape(-1, how_many).copy(), o[1].cpu().numpy().reshape(-1, how_many).copy(), o[2].cpu().numpy().view(np.uint32).copy())

    def slow(self, knobs, k, m, how_many=21, business=False):
        """The rows without the fast kernels (SRN_NO_FAST=1)."""
        key = (k, m, how_many, business)
        if key not in self._slow:
            knobs(SRN_NO_FAST=1)
            self._slow[key] = self.call(k, m, how_many, business)
            knobs()
        return self._slow[key]


def _vs_oracle(got, ref, what):
    ids, sc, cnt = got
    assert np.array_equal(cnt, ref["counts"]), "%s: counts differ from the oracle at queries %s" % (what, np.flatnonzero(cnt != ref["counts"])[:8])
    inside = np.arange(ids.shape[1])[None, :] < ref["counts"][:, None].astype(np.int64)
    bad = np.flatnonzero(((ids != ref["ids"]) & inside).any(axis=1))
    assert len(bad) == 0, "%s: ranked ids differ from the oracle at queries %s" % (what, bad[:8])
    np.testing.assert_allclose(sc[inside], ref["scores"][inside], rtol=SCORE_RTOL, atol=0)


def _same_bytes(got, ref, what):
    ids, sc, cnt = got
    rids, rsc, rcnt = ref
    assert np.array_equal(cnt, rcnt), "%s: counts differ at %s" % (what, np.flatnonzero(cnt != rcnt)[:8])
    inside = np.arange(ids.shape[1])[None, :] < np.minimum(cnt, ids.shape[1]).astype(np.int64)[:, None]
    assert np.array_equal(ids[inside], rids[inside]), "%s: ids differ" % what
    assert np.array_equal(sc[inside].view(np.uint64), rsc[inside].view(np.uint64)), "%s: scores differ in their bits" % what
