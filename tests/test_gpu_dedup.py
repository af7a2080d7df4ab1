"""Queries of ONE call with the same item sequence are computed once (srn_dedup.hip): the launch sequence groups the batch on the device -- a hash table
over (length, raw ids in order), full sequences compared on every hit --, serves the smallest query index of each group and copies its row to the others at the end.

Every batch here goes through srn_predict_batch_device with the serving order forced on (SRN_ORDER_MIN=1: the pass is on exactly where the order is) and is compared
  * with the canonical CPU oracle (rows of 1..max_len items: what the oracle defines),
  * bit for bit -- counts, and ids and scores inside the count -- with the same call under SRN_NO_DEDUP=1,
and srn_debug_last_dedup_count must equal nq - (number of distinct sequences), counted here with numpy: nothing merged that differs, nothing equal left unmerged.
"""
import os

import numpy as np
import pytest

from helpers import flatten, random_queries, small_dataset

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-12
KNOBS = ("SRN_ORDER_MIN", "SRN_NO_DEDUP", "SRN_DEDUP_HASH_BITS")


def _oracle():
    from oracle import oracle
    return oracle


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


class _FlatBatch:
    """A CSR batch (items_flat, q_off) where a Python list per query would be too slow."""

    def __init__(self, flat, off):
        self.flat, self.off = np.ascontiguousarray(flat, np.uint64), np.ascontiguousarray(off, np.uint32)

    def __len__(self):
        return len(self.off) - 1


def _flat(qs):
    return (qs.flat, qs.off) if isinstance(qs, _FlatBatch) else flatten(qs)


def _distinct(qs):
    """Number of distinct (length, ids in order) among the queries, with numpy: rows padded to the longest query, the length in front."""
    width = max([len(q) for q in qs] + [1])
    a = np.zeros((len(qs), width + 1), np.uint64)
    for i, q in enumerate(qs):
        a[i, 0] = len(q)
        a[i, 1:1 + len(q)] = np.array(q, np.uint64)
    return len(np.unique(a, axis=0))


class _Device:
    """One batch on the device and calls over it: rows come back as numpy arrays (ids u64[nq, n], scores f64[nq, n], counts u32[nq])."""

    def __init__(self, gix, qs, max_len):
        import torch
        self.torch, self.gix, self.nq, self.max_len = torch, gix, len(qs), max_len
        flat, off = _flat(qs)
        self.flat, self.off = flat, off
        dev = torch.device("cuda:0")
        self.d_flat = torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to(dev)
        self.d_off = torch.from_numpy(off.view(np.int32).copy()).to(dev)
        self.dev = dev

    def buffers(self, n, count_fill=0):
        t = self.torch
        cnt = t.full((self.nq,), int(np.array([count_fill], np.uint32).view(np.int32)[0]), dtype=t.int32, device=self.dev)
        return t.zeros(self.nq * n, dtype=t.int64, device=self.dev), t.zeros(self.nq * n, dtype=t.float64, device=self.dev), cnt

    def call(self, k, m, n, business=False, out=None, resident=False, sync=True):
        import serenade_amd as sa
        o = out if out is not None else self.buffers(n)
        sa.predict_batch_device(self.gix, self.d_flat.data_ptr(), self.d_off.data_ptr(), self.nq, self.max_len, k, m, n, business,
                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), self.torch.cuda.current_stream().cuda_stream, resident=resident)
        if not sync:
            return o
        self.torch.cuda.synchronize()
        return self.rows(o, n)

    def rows(self, o, n):
        return (o[0].cpu().numpy().view(np.uint64).reshape(self.nq, n).copy(), o[1].cpu().numpy().reshape(self.nq, n).copy(), o[2].cpu().numpy().view(np.uint32).copy())


def _same_rows(got, ref, what):
    ids, sc, cnt = got
    rids, rsc, rcnt = ref
    assert np.array_equal(cnt, rcnt), "%s: counts differ at %s" % (what, np.flatnonzero(cnt != rcnt)[:8])
    n = ids.shape[1]
    inside = np.arange(n)[None, :] < np.where(cnt == 0xFFFFFFFF, 0, np.minimum(cnt, n)).astype(np.int64)[:, None]
    assert np.array_equal(ids[inside], rids[inside]), "%s: ids differ" % what
    assert np.array_equal(sc[inside].view(np.uint64), rsc[inside].view(np.uint64)), "%s: scores differ in their bits" % what


def _vs_oracle(got, oix, qs, max_len, k, m, n, business):
    sel = np.array([i for i, q in enumerate(qs) if 1 <= len(q) <= max_len], np.int64)
    flat, off = flatten([qs[i] for i in sel])
    ref = oix.predict_batch("canonical", flat, off, k, m, n, business, threads=4)
    ids, sc, cnt = (a[sel] for a in got)
    assert np.array_equal(cnt, ref["counts"]), "counts differ from the oracle at %s" % sel[np.flatnonzero(cnt != ref["counts"])[:8]]
    inside = np.arange(n)[None, :] < ref["counts"][:, None].astype(np.int64)
    assert np.array_equal(ids[inside], ref["ids"][inside]), "ranked ids differ from the oracle"
    np.testing.assert_allclose(sc[inside], ref["scores"][inside], rtol=SCORE_RTOL, atol=0)


def _hurting_batch(ids, rng):
    """Everything that could go wrong with merging, in one batch of ~3 000 queries (sessions of up to 20 items are the call's max_len; two are longer)."""
    unknown = lambda: int(7 + rng.integers(0, 1000))                      # noqa: E731  (ids the index has never seen)
    w = 1.0 / np.arange(1, len(ids) + 1) ** 0.9
    w /= w.sum()
    draw = lambda ln: [int(x) for x in ids[rng.choice(len(ids), size=ln, p=w)]]   # noqa: E731
    qs = []
    top = [int(x) for x in ids[:6]]
    qs += [[top[0]]] * 400 + [[top[1]]] * 3 + [[top[0], top[1]]] * 150 + [[top[1], top[0]]] * 150     # large and small groups; the same items in the other order
    qs += [[top[2], top[3], top[4]]] * 40 + [[top[4], top[3], top[2]]] * 2 + [[top[2], top[4], top[3]]]
    seq = draw(8)
    for ln in range(1, 9):                                                                              # a sequence and every prefix of it, twice each
        qs += [seq[:ln], seq[:ln]]
    x, y = top[5], top[0]
    hi = [x, x + (1 << 32), x + (5 << 32), x + (1 << 63)]                                              # equal in the low 32 bits, different above
    for a in hi:
        qs += [[a], [a, y], [y, a], [a]]
    qs += [[unknown()] for _ in range(20)] + [[12345], [12345], [12345, top[0]], [12345, top[0]], [top[0], 12345]]   # unknown ids: merged only where they are the same ids
    qs += [[top[0], top[0]], [top[0], top[0]], [top[0], top[1], top[0]], [top[0], top[1], top[0]], [top[1], top[0], top[0]], [top[0], top[0], top[0], top[0]]]   # items repeated inside a session
    qs += [[], [], []]                                                                                  # empty queries
    too_long = draw(25)
    qs += [too_long, list(too_long), too_long[:24]]                                                    # longer than the call's max_len
    for lo, hi_ in ((5, 10), (11, 20)):                                                                 # the MID, BIG and LONG tiers' sessions, with copies
        for _ in range(120):
            q = draw(int(rng.integers(lo, hi_ + 1)))
            if rng.random() < 0.2:
                q[int(rng.integers(1, len(q)))] = q[0]
            qs += [q] * int(rng.integers(1, 4))
    qs += random_queries(91, ids, 1200, max_len=4, unknown_rate=0.05, dup_rate=0.2)                    # the lean shape: a Zipf draw is full of equal short sessions
    rare = [int(x) for x in ids[-12:]]
    qs += [[r] for r in rare] * 3 + [[rare[0], rare[1]], [rare[0], rare[1]]]                            # small queries without a threshold (more than 63 entries: vmis_finish_big_kernel)
    order = rng.permutation(len(qs))
    return [list(qs[i]) for i in order]


@pytest.fixture(scope="module")
def dense_index():
    """150 items over 40 000 sessions: posting lists long enough for both cuts to bite, queries with more than 63 scored items, every tier of the launch sequence in use."""
    import serenade_amd as sa
    O = _oracle()
    off, items, ts, ids = small_dataset(31, n_sessions=40000, n_items=150, max_len=12)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 3000, 20, 1.0)
    oix = O.OracleIndex(off, items, ts, 3000, 20, 1.0)
    rng = np.random.default_rng(4)
    known = np.unique(items)
    flags = rng.choice(np.array([0, 1, 2, 3, 0xFF], np.uint8), size=len(known), p=[0.1, 0.05, 0.55, 0.2, 0.1])
    gix.set_attributes(known, flags)
    oix.set_attributes(known, flags)
    return gix, oix, ids


@pytest.mark.parametrize("hash_bits", [None, 4])
@pytest.mark.parametrize("k,m,n,business", [(1500, 2500, 21, False), (100, 500, 21, True), (700, 2560, 5, True)])
def test_batch_built_to_hurt(dense_index, knobs, hash_bits, k, m, n, business):
    """Exact copies in large and small groups; the same items in another order (NOT merged: the weights are positional); a sequence and its prefixes; ids equal in their
    low 32 bits; unknown ids; items repeated inside a session; empty queries and queries longer than max_len; copies among sessions of 5..10 and 11..20 items (MID, BIG,
    LONG) and among what reaches the general kernel; small queries without a threshold; business rules.  Also with the hash cut to 4 bits: unequal queries share hashes,
    the probe chains run through hundreds of slots, and only the comparison of the sequences keeps them apart -- same rows, same count.
    (m stays at or below 2 560, the fast kernels' F_M_MAX: the pass is on only where the fast path and its serving order are -- the test after the next one has m = 3 000.)"""
    gix, oix, ids = dense_index
    qs = _hurting_batch(ids, np.random.default_rng(77))
    dv = _Device(gix, qs, 20)
    knobs(SRN_ORDER_MIN=1, SRN_NO_DEDUP=1)
    ref = dv.call(k, m, n, business)
    assert gix.last_dedup_count() == 0
    knobs(SRN_ORDER_MIN=1, SRN_DEDUP_HASH_BITS=hash_bits)
    got = dv.call(k, m, n, business)
    merged = gix.last_dedup_count()
    nq, general, _glob = gix.last_path_counts()
    mid = gix.last_mid_count()
    print("hurting batch: %d queries, %d distinct, %d merged; listed for MID %d, reached the general kernel %d (k %d m %d n %d, business %s, hash bits %s)"
          % (len(qs), _distinct(qs), merged, mid, general, k, m, n, business, hash_bits))
    assert nq == len(qs)
    assert merged == len(qs) - _distinct(qs)
    _same_rows(got, ref, "merged against SRN_NO_DEDUP=1")
    _vs_oracle(got, oix, qs, 20, k, m, n, business)
    assert mid > 0 and general > 0, "the batch should reach the MID tier and the general kernel (%d, %d)" % (mid, general)


@pytest.mark.parametrize("fill", [0x80000000, 0x80000001])
def test_count_words_prefilled_with_the_finish_kernels_flags(dense_index, knobs, fill):
    """The finish kernels act on every row of [0, nq) whose count word is 0x80000000 / 0x80000001, and nobody serves a merged query: the grouping pass must put a
    non-flag value there whatever the caller's buffer held."""
    gix, oix, ids = dense_index
    qs = _hurting_batch(ids, np.random.default_rng(78))
    dv = _Device(gix, qs, 20)
    k, m, n = 1500, 2500, 21
    knobs(SRN_ORDER_MIN=1, SRN_NO_DEDUP=1)
    ref = dv.call(k, m, n)
    knobs(SRN_ORDER_MIN=1)
    for resident in (False, True):
        got = dv.call(k, m, n, out=dv.buffers(n, count_fill=fill), resident=resident)
        assert gix.last_dedup_count() == len(qs) - _distinct(qs)
        _same_rows(got, ref, "count words pre-filled with %#x (resident %s)" % (fill, resident))
    _vs_oracle(got, oix, qs, 20, k, m, n, False)


def test_resident_calls_alternating_two_batches(dense_index, knobs):
    """SRN_FLAG_INPUTS_RESIDENT: call i + 1's prep, grouping and sort run on the side stream while call i's kernels still read THEIR order, representatives and merged
    count -- two order sets.  Two different batches (different sizes, different groups) alternate for eight calls without a host synchronisation, the result buffers
    REUSED from call to call as a serving host does; every call's rows are read back behind it on the stream and must be right."""
    import torch
    gix, oix, ids = dense_index
    k, m, n = 1500, 2500, 21
    qa = _hurting_batch(ids, np.random.default_rng(79))
    qb = random_queries(5, ids, 1700, max_len=3, unknown_rate=0.02, dup_rate=0.1) + [[int(ids[0])]] * 300
    dvs = [_Device(gix, qa, 20), _Device(gix, qb, 20)]
    knobs(SRN_ORDER_MIN=1, SRN_NO_DEDUP=1)
    refs = [dv.call(k, m, n) for dv in dvs]
    knobs(SRN_ORDER_MIN=1)
    nmax = max(dv.nq for dv in dvs)
    shared = (torch.zeros(nmax * n, dtype=torch.int64, device="cuda:0"), torch.zeros(nmax * n, dtype=torch.float64, device="cuda:0"), torch.zeros(nmax, dtype=torch.int32, device="cuda:0"))
    copies = []
    for call in range(8):
        dv = dvs[call % 2]
        dv.call(k, m, n, out=shared, resident=True, sync=False)
        copies.append(tuple(t.clone() for t in shared))   # (on the same stream: behind the call, before the next one overwrites the buffers)
    torch.cuda.synchronize()
    assert gix.last_dedup_count() == len(qb) - _distinct(qb)
    for call, o in enumerate(copies):
        dv = dvs[call % 2]
        got = (o[0].cpu().numpy().view(np.uint64)[:dv.nq * n].reshape(dv.nq, n), o[1].cpu().numpy()[:dv.nq * n].reshape(dv.nq, n), o[2].cpu().numpy().view(np.uint32)[:dv.nq])
        _same_rows(got, refs[call % 2], "resident call %d" % call)
    _vs_oracle(refs[1], oix, qb, 20, k, m, n, False)


def test_all_the_same_query_and_no_two_alike(dense_index, knobs):
    gix, oix, ids = dense_index
    k, m, n = 1500, 2500, 21
    same = [[int(ids[3]), int(ids[0]), int(ids[7])]] * 2500
    rng = np.random.default_rng(12)
    seen, distinct = set(), []
    while len(distinct) < 2500:
        q = tuple(int(x) for x in ids[rng.integers(0, len(ids), size=int(rng.integers(1, 5)))])
        if q not in seen:
            seen.add(q)
            distinct.append(list(q))
    for qs, want in ((same, len(same) - 1), (distinct, 0)):
        dv = _Device(gix, qs, 4)
        knobs(SRN_ORDER_MIN=1, SRN_NO_DEDUP=1)
        ref = dv.call(k, m, n)
        knobs(SRN_ORDER_MIN=1)
        got = dv.call(k, m, n)
        assert gix.last_dedup_count() == want
        _same_rows(got, ref, "%d merged" % want)
        _vs_oracle(got, oix, qs, 4, k, m, n, False)


def test_below_the_order_threshold_nothing_is_merged(dense_index, knobs):
    """The pass is on exactly where the serving order is: a batch below SRN_ORDER_MIN (the default 131 072) is served query by query."""
    gix, oix, ids = dense_index
    qs = [[int(ids[0])]] * 500
    dv = _Device(gix, qs, 4)
    knobs()
    got = dv.call(100, 500, 21)
    assert gix.last_dedup_count() == 0
    _vs_oracle(got, oix, qs, 4, 100, 500, 21, False)


def test_off_the_fast_path_nothing_is_merged(dense_index, knobs):
    """m = 3 000 is beyond what the fast kernels take (F_M_MAX = 2 560): the whole batch goes through the general kernel, there is no serving order and no merging --
    every query is served, and the rows are the oracle's."""
    gix, oix, ids = dense_index
    qs = _hurting_batch(ids, np.random.default_rng(80))
    dv = _Device(gix, qs, 20)
    knobs(SRN_ORDER_MIN=1)
    got = dv.call(700, 3000, 5, True)
    nq, general, _glob = gix.last_path_counts()
    assert gix.last_dedup_count() == 0 and general == nq == len(qs)
    _vs_oracle(got, oix, qs, 20, 700, 3000, 5, True)


def test_counter_on_the_headline_stream(knobs):
    """The first 2^18 queries of the stream bench.py draws for config 3 (1.76 M items, Zipf; same seed, same session count as `--batch 1048576 --pool 2`), at the default
    SRN_ORDER_MIN, served from the tiny index (config 3's takes minutes to build: the grouping pass never looks at the index): the merged count equals numpy's, and the
    rows equal the unmerged call's."""
    import serenade_amd as sa
    from serenade_amd import synth
    inter, n_items, k, m, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    gix = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw)
    B = 1 << 18
    qi, qo = synth.queries(int((1 << 20) * 2 / 3.2) + 4096, synth.CONFIGS["cfg3"][1], seed=synth.SEED + 7919, max_items=synth.LAST_ITEMS)
    assert len(qo) - 1 >= B
    qo = qo[:B + 1]
    qi = qi[:qo[-1]]
    lens = np.diff(qo.astype(np.int64))
    a = np.zeros((B, synth.LAST_ITEMS + 1), np.uint64)
    a[:, 0] = lens
    for j in range(synth.LAST_ITEMS):
        has = lens > j
        a[has, 1 + j] = qi[qo[:-1].astype(np.int64)[has] + j]
    distinct = len(np.unique(a, axis=0))
    qs = _FlatBatch(qi, qo)
    dv = _Device(gix, qs, synth.LAST_ITEMS)
    knobs(SRN_NO_DEDUP=1)
    ref = dv.call(k, m, synth.HOW_MANY)
    knobs()
    got = dv.call(k, m, synth.HOW_MANY)
    merged = gix.last_dedup_count()
    print("headline stream, first %d queries: %d distinct, %d merged (%.1f %%)" % (B, distinct, merged, 100.0 * merged / B))
    assert merged == B - distinct
    _same_rows(got, ref, "headline stream")
