"""The designed index of tests/edge_cases.py through every form of the fast kernels, against the canonical oracle.  The index places a query exactly on each threshold of
vmis_fast_kernel's front end and of the prep record, one on either side (stage loads at every multiple of 512, the lean / MID / BIG / LONG merge-room limits, n = 3 072
between the fused and the two-pass cut, the x_lo search's small cases, both cuts' strict and non-strict sides, row sizes at the finish hand-off); that it does so is
asserted on the CPU by tests/test_edge_cases_host.py (the census), so nothing here passes vacuously.  One index per timestamp variant (distinct / tied in groups of 8),
every test one batch of all queries, at the call shapes (k, m) = (500, 1 100) and (1 536, 2 560).

(a) Record level: srn_debug_prep_records; the 16 launch-ready words equal record_cases.ready_from_legacy, and kept, n_staged, x_lo, sumw, nruns (and U, rmax, P, L) equal
    the NumPy restatement word for word; the routing the records give is the restatement's.  `wide` false and true (SRN_FAST_RUNS=3).
(b) Rows: without the fast kernels (SRN_NO_FAST=1) against the oracle -- counts, ids and order exact, scores to 1e-12 -- with the counters P, C, K, I, D, H, L and the
    neighbour (session, numerator) sets of predict_batch_debug exact and the product call equal to the debug call; then every fast path against the oracle and, bit for
    bit, against the SRN_NO_FAST rows: default, SRN_GRID_MULT=1, SRN_ORDER_MIN=1, SRN_FAST_RUNS=3, SRN_NO_MID / SRN_NO_BIG / SRN_NO_LONG, how_many 64, business rules with
    drawn attribute bytes.  The route counts are the restatement's where the C ABI has a count: queries listed for MID (last_mid_count) and for the BIG forms
    (last_big_count) and served by the general kernel (last_path_counts), all three exactly: the general kernel gets the front end's hand-overs and NOTHING else, so every
    other row is a fast form's own.  (The index's payload has a hot head so that the back end's threshold bites and no query outgrows F_CAND_CAP, F_HIT_CAP or the exact
    table; edge_cases.backend_fits states that on the CPU and the census asserts it.)  The ABI has no count for the LONG form's list or for rows of more than 63 entries.
(c) Outside the fast limits, (k, m) = (1 537, 2 560) and (1 536, 2 561): the whole batch goes to the general kernel and stays oracle-exact.
(d) The latency path: every cell of <= 10 items as a single srn_predict call (the TINY form, which decodes the items itself), fused and with SRN_TINY_FUSED=0; after
    each call last_path_counts says whether the TINY form served it (lean and MID routes) or the general kernel behind it (everything else).  The persistent form of
    that path -- resident workgroups, the same sessions posted one by one -- is tests/test_gpu_persistent_edges.py.
World, the row comparisons and the knobs fixture are tests/edge_world.py's, shared with that file."""
import numpy as np
import pytest

import edge_cases as E
import record_cases as RC
from edge_world import SCORE_RTOL, World, _same_bytes, _vs_oracle, knobs  # noqa: F401  (knobs: the fixture)

pytestmark = pytest.mark.gpu

VARIANTS = ["distinct", "tied"]
PATHS = {"default": {}, "grid1": dict(SRN_GRID_MULT=1), "ordered": dict(SRN_ORDER_MIN=1), "wide": dict(SRN_FAST_RUNS=3), "no_mid": dict(SRN_NO_MID=1), "no_big": dict(SRN_NO_BIG=1),
         "no_long": dict(SRN_NO_LONG=1), "how_many64": {}, "business": {}}


@pytest.fixture(scope="module", params=VARIANTS)
def world(request):
    w = World(request.param == "tied")
    print("%s: %d cells, %d sessions, %d queries, fixture built in %.1f s" % (request.param, len(w.ix.cells), len(w.ix.ts), w.nq, w.seconds))
    return w


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_a_records_word_for_word(world, knobs, wide):
    knobs(**(dict(SRN_FAST_RUNS=3) if wide else {}))
    for sh, (k, m) in enumerate(E.SHAPES):
        R = E.restate(world.tied, sh)
        rec = RC.prep_records(world.gix, world.qs, m, E.MAX_LEN)
        got, want = rec[:, RC.READY0:RC.READY0 + RC.READY_WORDS], RC.ready_from_legacy(rec, wide, E.MAX_LEN)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert len(bad) == 0, "m = %d: %d launch-ready blocks differ, the first: query %d (%s)\n got  %s\n want %s" % (
            m, len(bad), bad[0], world.ix.cells[world.ix.q_cell[bad[0]]]["name"], got[bad[0]], want[bad[0]])
        f = RC.legacy(rec, E.MAX_LEN)
        head = rec[:, :8].astype(np.int64)   # U rmax xlo sumw | P nruns L n_staged
        for qi, r in enumerate(R):
            name = world.ix.cells[world.ix.q_cell[qi]]["name"]
            kept = np.zeros(E.MAX_LEN, np.int64)
            kept[r["pos"]] = r["kept"]
            assert np.array_equal(f["kept"][qi], kept), (m, qi, name, f["kept"][qi][:r["L"]], kept[:r["L"]])
            assert head[qi].tolist() == [r["U"], r["rmax"], r["xlo"], r["sumw"], r["P"], len(r["len"]), r["L"], r["n"]], (m, qi, name, head[qi].tolist())
            assert f["unsafe"][qi] == 0
        assert RC.routing(rec, E.MAX_LEN, wide) == [r["route"] for r in R], "m = %d: the records route another way than the restatement" % m
        lean_ok = got[:, 0] & 1
        assert np.array_equal(lean_ok == 1, np.array([r["route"] == "lean" for r in R]))
        assert wide == bool(((got[:, 0] >> 16) & 1).any()), "the rel bit follows the 29-bit-rank form"
        # the load mask at every edge: (kept + 511) >> 9 loads of run 0
        loads = np.array([bin(int(x) & 31).count("1") for x in got[:, 1]])
        for v in E.STAGE_KEPT:
            sel = (lean_ok == 1) & (got[:, 4] == v)
            assert (sel.any() or v > m) and (loads[sel] == (v + 511) // 512).all(), (m, v)


@pytest.mark.parametrize("shape", [0, 1], ids=["k500_m1100", "k1536_m2560"])
def test_b_rows_without_the_fast_kernels(world, knobs, shape):
    import serenade_amd as sa
    k, m = E.SHAPES[shape]
    ref = world.ref(k, m)
    _vs_oracle(world.slow(knobs, k, m), ref, "SRN_NO_FAST=1")
    res = sa.predict_batch_debug(world.gix, world.qs, k, m, 21, False, neighbours=True)
    _vs_oracle((res["ids"], res["scores"], res["counts"]), ref, "debug call")
    assert np.array_equal(res["stats"][:, :7].astype(np.uint64), ref["stats"]), "P,C,K,I,D,H,L counters differ at queries %s" % np.flatnonzero((res["stats"][:, :7] != ref["stats"]).any(axis=1))[:8]
    for qi, r in enumerate(E.restate(world.tied, shape)):   # (the restatement's neighbours are the oracle's: tests/test_edge_cases_host.py)
        kq = int(res["nb_counts"][qi])
        assert sorted(zip(res["nb_sessions"][qi, :kq].tolist(), res["nb_num"][qi, :kq].tolist())) == r["nb"], (qi, world.ix.cells[world.ix.q_cell[qi]]["name"])
    ids, scores, counts = sa.predict_batch(world.gix, world.qs, k, m, 21, False)   # (more than 256 sessions: the launch sequence)
    assert np.array_equal(counts, res["counts"]) and np.array_equal(ids, res["ids"]) and np.array_equal(scores, res["scores"]), "the product call differs from the debug call"
    _same_bytes(world.call(k, m), (ids, scores, counts), "device-resident call against the host call")


@pytest.mark.parametrize("shape", [0, 1], ids=["k500_m1100", "k1536_m2560"])
@pytest.mark.parametrize("path", list(PATHS))
def test_b_rows_on_every_fast_path(world, knobs, path, shape):
    k, m = E.SHAPES[shape]
    how_many, business = 64 if path == "how_many64" else 21, path == "business"
    slow = world.slow(knobs, k, m, how_many, business)
    knobs(**PATHS[path])
    got = world.call(k, m, how_many, business)
    gix = world.gix
    nq, general, _glob = gix.last_path_counts()
    mid, big, merged = gix.last_mid_count(), gix.last_big_count(), gix.last_dedup_count()
    _vs_oracle(got, world.ref(k, m, how_many, business), path)
    _same_bytes(got, slow, "%s against SRN_NO_FAST=1" % path)
    routes = [r["route"] for r in E.restate(world.tied, shape)]
    want_mid = sum(r.startswith("mid") for r in routes)
    want_big = sum(r in ("big", "mid>big") for r in routes)
    want_general = sum(r in ("general", "mid>general", "long>general") for r in routes)
    print("%s (k %d, m %d): %d queries, %d merged, lean %d, MID %d (want %d), BIG %d (want %d), LONG's list %d (no count in the ABI), general %d (the front end hands over %d)" % (
        path, k, m, nq, merged, routes.count("lean"), mid, want_mid, big, want_big, routes.count("long") + routes.count("long>general"), general, want_general))
    assert nq == world.nq and merged == 0
    n_long = routes.count("long")
    if path == "no_mid":       # a batch with sessions of more than 8 items needs the MID tier to use the fast kernels at all (fast_plan, srn_runtime.hip)
        assert (mid, big, general) == (0, 0, nq)
    elif path == "no_big":     # no BIG list: the lean kernel lists its oversized queries for MID, which hands them and its own to the general kernel; no LONG form (a form of BIG) either
        assert (mid, big, general) == (want_mid + routes.count("big"), 0, want_general + want_big + n_long)
    elif path == "no_long":
        assert (mid, big, general) == (want_mid, want_big, want_general + n_long)
    else:                      # the general kernel serves the front end's hand-overs and nothing else: every other row compared above is a fast form's own (edge_cases.backend_fits)
        assert (mid, big, general) == (want_mid, want_big, want_general)
        assert routes.count("lean") >= 0.8 * nq and want_mid > 0 and want_general > 0 and want_big > 0


@pytest.mark.parametrize("k,m", [(E.F_K_MAX + 1, E.F_M_MAX), (E.F_K_MAX, E.F_M_MAX + 1)], ids=["k1537", "m2561"])
def test_c_outside_the_fast_limits(world, knobs, k, m):
    knobs()
    got = world.call(k, m)
    nq, general, _glob = world.gix.last_path_counts()
    _vs_oracle(got, world.ref(k, m), "k %d m %d" % (k, m))
    assert (nq, general) == (world.nq, world.nq), "beyond F_K_MAX / F_M_MAX the whole batch is the general kernel's"


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_d_single_calls_on_the_latency_path(world, knobs, fused):
    import serenade_amd as sa
    knobs(**({} if fused else dict(SRN_TINY_FUSED=0)))
    n = served = 0
    for shape, (k, m) in enumerate(E.SHAPES):
        ref = world.ref(k, m)
        R = E.restate(world.tied, shape)
        for qi, q in enumerate(world.qs):
            if world.ix.q_shift[qi] or len(q) > 10:
                continue
            recs = sa.predict(world.gix, q, k, m, 21, False)
            c = int(ref["counts"][qi])
            name = world.ix.cells[world.ix.q_cell[qi]]["name"]
            assert [r.id for r in recs] == ref["ids"][qi, :c].tolist(), (qi, name, k, m)
            np.testing.assert_allclose([r.score for r in recs], ref["scores"][qi, :c], rtol=SCORE_RTOL, atol=0)
            # served by the TINY form itself (lean or MID: the latency path has no BIG tier), or handed to the general kernel behind it, as the restatement's route says
            want_general = 0 if R[qi]["route"] in ("lean", "mid") else 1
            assert world.gix.last_path_counts()[:2] == (1, want_general), (qi, name, k, m, R[qi]["route"], world.gix.last_path_counts())
            served += 1 - want_general
            n += 1
    print("%d single calls, %d served by the TINY form" % (n, served))
    assert n >= 200 and served >= 0.9 * n
