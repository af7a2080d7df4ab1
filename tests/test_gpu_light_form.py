"""The light form (vmis_light_kernel, srn_light.hip) on the designed cases of tests/light_cases.py -- that they are what they claim is tests/test_light_cases_host.py's.
With SRN_ORDER_MIN=1 SRN_LIGHT_MIN=1 the batch's light queries are served one wave each; every row must be the canonical oracle's (ids and order exact, scores to 1e-12)
and, bit for bit, the row of the same call with SRN_LIGHT_MIN=0 (the lean chain).  srn_debug_last_light_count EQUALS the CPU prediction and the general kernel's count
EQUALS the designed overflow cases: no light query slips to another path unnoticed."""
import ctypes as C
import os

import numpy as np
import pytest

import light_cases as LC
from edge_world import _same_bytes, _vs_oracle
from fill_cases import draw_attrs
from helpers import flatten

pytestmark = pytest.mark.gpu
KNOBS = ("SRN_ORDER_MIN", "SRN_LIGHT_MIN", "SRN_NO_DEDUP")


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
    def __init__(self):
        import serenade_amd as sa
        import torch
        from oracle import oracle as O
        self.t = torch
        self.c = c = LC.build()
        self.gix = sa.VMISIndex.from_sessions(c.off, c.items, c.ts, LC.M_INDEX, LC.ROW_MAX, 1.0, device=0)
        self.oix = O.OracleIndex(c.off, c.items, c.ts, LC.M_INDEX, LC.ROW_MAX, 1.0, fast=True)
        known, flags = draw_attrs(c.items)
        self.gix.set_attributes(known, flags)
        self.oix.set_attributes(known, flags)
        self.attrs = dict(zip(known.tolist(), flags.tolist()))
        self.batches, self._ref = {}, {}
        rs = [LC.predict_one(c, q) for q in c.queries]
        self.add("all", c.queries)
        self.add("reversed", c.queries[::-1])
        self.add("only light", [q for q, r in zip(c.queries, rs) if r["admitted"]])
        self.add("no light", [q for q, r in zip(c.queries, rs) if not r["admitted"]])

    def add(self, name, qs):
        flat, off = flatten(qs)
        d_flat = self.t.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to("cuda:0")
        d_off = self.t.from_numpy(off.view(np.int32).copy()).to("cuda:0")
        self.batches[name] = (qs, flat, off, d_flat, d_off)

    def ref(self, name, how_many=21, business=False):
        key = (name, how_many, business)
        if key not in self._ref:
            _qs, flat, off, _a, _b = self.batches[name]
            r = self.oix.predict_batch("canonical", flat, off, LC.K, LC.M, how_many, business, threads=8)
            for a in (r["ids"], r["scores"], r["counts"]):
                a.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def call(self, name, how_many=21, business=False, resident=False, k=LC.K):
        import serenade_amd as sa
        t = self.t
        qs, _flat, _off, d_flat, d_off = self.batches[name]
        nq = len(qs)
        o = (t.zeros(nq * how_many, dtype=t.int64, device="cuda:0"), t.zeros(nq * how_many, dtype=t.float64, device="cuda:0"), t.zeros(nq, dtype=t.int32, device="cuda:0"))
        sa.predict_batch_device(self.gix, d_flat.data_ptr(), d_off.data_ptr(), nq, LC.MAX_LEN, k, LC.M, how_many, business,
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), t.cuda.current_stream().cuda_stream, resident=resident)
        t.cuda.synchronize()
        return (o[0].cpu().numpy().view(np.uint64).reshape(-1, how_many).copy(), o[1].cpu().numpy().reshape(-1, how_many).copy(), o[2].cpu().numpy().view(np.uint32).copy())


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("merge", [True, False], ids=["merging", "no_merging"])
@pytest.mark.parametrize("how_many,business", [(21, False), (64, False), (21, True)], ids=["n21", "n64", "business"])
@pytest.mark.parametrize("batch", ["all", "only light", "no light"])
def test_rows_counts_and_routing(world, knobs, batch, how_many, business, merge):
    qs = world.batches[batch][0]
    extra = {} if merge else dict(SRN_NO_DEDUP=1)
    knobs(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=0, **extra)
    lean = world.call(batch, how_many, business)
    assert world.gix.last_light_count() == 0
    knobs(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=1, **extra)
    got = world.call(batch, how_many, business)
    light, (nq, general, _glob), merged = world.gix.last_light_count(), world.gix.last_path_counts(), world.gix.last_dedup_count()
    want_light, want_general = LC.predict(world.c, qs, how_many, world.attrs if business else None, merge=merge)
    print("%s, how_many %d, business %s, merge %s: %d queries, %d merged, light %d (want %d), general kernel %d (want %d)" % (batch, how_many, business, merge, nq, merged, light, want_light, general, want_general))
    _vs_oracle(got, world.ref(batch, how_many, business), "light form")
    _same_bytes(got, lean, "light form against SRN_LIGHT_MIN=0")
    assert nq == len(qs) and merged == (len(qs) - len({tuple(q) for q in qs}) if merge else 0)
    assert light == want_light, "srn_debug_last_light_count differs from the CPU prediction"
    assert general == want_general, "the general kernel serves the designed overflow cases and nothing else"
    if batch == "only light":
        assert light == (len({tuple(q) for q in qs}) if merge else len(qs))
    if batch == "no light":
        assert light == 0


def test_resident_calls_alternating_two_batches(world, knobs):
    knobs(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=0)
    lean = {b: world.call(b) for b in ("all", "reversed")}
    knobs(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=1)
    want = {b: LC.predict(world.c, world.batches[b][0]) for b in ("all", "reversed")}
    for i in range(6):
        b = ("all", "reversed")[i % 2]
        got = world.call(b, resident=True)
        _vs_oracle(got, world.ref(b), "resident call %d" % i)
        _same_bytes(got, lean[b], "resident call %d against SRN_LIGHT_MIN=0" % i)
        assert (world.gix.last_light_count(), world.gix.last_path_counts()[1]) == want[b], i


def test_calls_without_the_form_report_zero(world, knobs):
    import serenade_amd as sa
    from serenade_amd import capi, sharded
    qs = world.batches["all"][0]
    # below SRN_LIGHT_MIN (the default, and one query short of the batch), and k below 64
    for kv in (dict(SRN_ORDER_MIN=1), dict(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=len(qs) + 1)):
        knobs(**kv)
        _vs_oracle(world.call("all"), world.ref("all"), str(kv))
        assert world.gix.last_light_count() == 0, kv
    knobs(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=len(qs))
    world.call("all")
    assert world.gix.last_light_count() == LC.predict(world.c, qs)[0]
    world.call("all", k=63)
    assert world.gix.last_light_count() == 0, "k < 64"
    # a call that uses the result cache
    knobs(SRN_ORDER_MIN=1, SRN_LIGHT_MIN=1)
    world.gix.enable_result_cache(4096, LC.MAX_LEN, LC.K, LC.M, 21)
    try:
        for _ in range(2):
            _vs_oracle(world.call("all"), world.ref("all"), "result cache")
            assert world.gix.last_light_count() == 0
        assert world.gix.result_cache_stats()["hits"] > 0
    finally:
        world.gix.disable_result_cache()
    world.call("all")
    assert world.gix.last_light_count() == LC.predict(world.c, qs)[0], "the form is back once the cache is off"
    # a shard group's call: its pipelines never take the form
    shards = [sharded.ShardedVMISIndex.from_full(world.gix, g, 2) for g in range(2)]
    grp = sharded.ShardGroup.local(shards)
    _qs, _flat, _off, d_flat, d_off = world.batches["all"]
    out = grp.predict_batch(d_flat, d_off, len(qs), LC.MAX_LEN, LC.K, LC.M, 21)
    world.t.cuda.synchronize()
    got = (out[0].cpu().numpy().view(np.uint64).reshape(-1, 21), out[1].cpu().numpy().reshape(-1, 21), out[2].cpu().numpy().view(np.uint32))
    _vs_oracle(got, world.ref("all"), "shard group")
    for s in shards:
        v = C.c_uint32(0xFFFFFFFF)
        rc = capi.lib().srn_debug_last_light_count(s._h, C.byref(v))
        assert rc != 0 or v.value == 0, "a shard of the group reports light queries"   # (rc != 0: no launch sequence of its own ran on this shard)
    del sa
