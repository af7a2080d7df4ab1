"""Pins the CPU oracle (oracle/vmis_oracle.cpp) against every known answer the reference holds for the hot path
 before anything is compared with it.  No GPU needed."""
import os

import numpy as np
import pytest

from helpers import (GOLDEN, assert_valid_topn, evaluator_queries, extract_example, flatten,
                     mrr_hitrate, random_queries, read_test_data_evolving, small_dataset)
from oracle import oracle as O

KAT_OFF = np.array([0, 3, 7], np.uint64)
KAT_ITEMS = np.array([920004, 920005, 920006, 920002, 920003, 920004, 920005], np.uint64)   # rows ascending
KAT_TS = np.array([1, 1], np.uint32)


@pytest.mark.parametrize("fast", [False, True])
def test_kat1_should_train_and_predict(fast):
    """src/vmisknn/mod.rs:229-310: 2 sessions, n_most_recent=5, max_len=5, idf_weighting=1; predict([920005],
    k=500, m=500, how_many=20) -> exactly 4 recommendations, 920004 first."""
    ix = O.OracleIndex(KAT_OFF, KAT_ITEMS, KAT_TS, 5, 5, 1.0, fast=fast)
    post, idf = ix.postings(920005)
    assert post.tolist() == [1, 0]                                  # timestamp tie -> larger session index first (Q9)
    assert idf == pytest.approx(np.log(7 / 2), rel=1e-15)           # pairs / sessions-with-item (Q5)
    for predict in (ix.predict_literal, ix.predict_canonical):
        ids, sc = predict([920005], 500, 500, 20)
        assert len(ids) == 4
        assert ids[0] == 920004
        assert sc[0] == pytest.approx(2.2549733432916628, rel=1e-14)
        assert sorted(ids[1:].tolist()) == [920002, 920003, 920006]
        np.testing.assert_allclose(sc[1:], 1.751319134149782, rtol=1e-14)


def test_heap_order_known_answers():
    """src/vmisknn/mod.rs:313-411 and similarity_hashed.rs:35-58."""
    assert O.kat_itemscore_heap([123, 543, 234], [5000.0, 1.0, 100.0], 2) == [234, 123]      # min-heap on score
    assert O.kat_itemscore_sorted([123, 543, 234], [5000.0, 1.0, 100.0]) == [123, 234, 543]  # into_sorted_vec: score desc
    assert O.kat_sessiontime_heap([123, 345, 456, 234], [5000, 99, 1, 499], 2) == [234, 123]  # 8-ary heap, oldest at root


def test_panic_inputs_are_reported():
    ix = O.OracleIndex(KAT_OFF, KAT_ITEMS, KAT_TS, 5, 5, 1.0)
    with pytest.raises(RuntimeError):
        ix.predict_literal([], 10, 10, 5)            # mod.rs:157 unwrap on empty session
    with pytest.raises(RuntimeError):
        ix.predict_canonical([], 10, 10, 5)
    ids, _ = ix.predict_literal([1, 2, 3], 10, 10, 5)   # unknown items are skipped (vmis_index.rs:350)
    assert len(ids) == 0


def test_fast_index_builder_equals_literal_prepare_hashmap():
    for seed, tied in ((1, False), (2, True)):
        off, items, ts, ids = small_dataset(seed, n_sessions=2000, n_items=250, tied_timestamps=tied)
        a = O.OracleIndex(off, items, ts, 60, 9, 1.5, fast=False)
        b = O.OracleIndex(off, items, ts, 60, 9, 1.5, fast=True)
        assert a.num_items == b.num_items and a.total_pairs == b.total_pairs
        for it in ids:
            pa, ia = a.postings(int(it))
            pb, ib = b.postings(int(it))
            if pa is None:
                assert pb is None
                continue
            assert np.array_equal(pa, pb) and ia == ib


def test_literal_is_a_valid_instance_of_canonical_when_timestamps_are_unique():
    """With unique timestamps the reference's sequential find_neighbors equals the closed form;
    what is left to hash/heap order is only WHICH of several equal-score entries sit at a cut (N2/N3)."""
    off, items, ts, ids = small_dataset(7, n_sessions=3000, n_items=300)
    ix = O.OracleIndex(off, items, ts, 150, 12, 1.0)
    qs = random_queries(3, ids, 250, max_len=6)
    for (k, m, n) in [(40, 150, 21), (500, 60, 10)]:
        for q in qs:
            sid_l, sim_l = ix.find_neighbors_literal(q, k, m)
            sid_c, num_c, U = ix.neighbors_canonical(q, k, m)
            assert len(sid_l) == len(sid_c)
            if len(sid_c) == 0:
                continue
            sim_c = num_c / U
            # every candidate's similarity agrees with the closed form, and the literal set is a valid top-k by score
            full_sid, full_num, _ = ix.neighbors_canonical(q, 10**6, m)
            table = dict(zip(full_sid.tolist(), (full_num / U).tolist()))
            for s, v in zip(sid_l.tolist(), sim_l.tolist()):
                assert table[s] == pytest.approx(v, rel=1e-12)
            assert sorted(sim_l.tolist(), reverse=True) == pytest.approx(sorted(sim_c.tolist(), reverse=True), rel=1e-12)
            # same neighbour set -> same item scores
            if set(sid_l.tolist()) == set(sid_c.tolist()):
                ids_l, sc_l = ix.predict_literal(q, k, m, n)
                all_ids, all_sc, _ = ix.scores_canonical(q, k, m)
                assert_valid_topn(ids_l, sc_l, all_ids, all_sc, n, exclude=[q[-1]])


def test_canonical_topn_is_sorted_and_excludes_current_item():
    off, items, ts, ids = small_dataset(9, n_sessions=1500, n_items=150)
    ix = O.OracleIndex(off, items, ts, 100, 12, 1.0)
    for q in random_queries(4, ids, 100, max_len=5):
        out_ids, sc = ix.predict_canonical(q, 30, 100, 15)
        assert q[-1] not in out_ids.tolist()
        assert all(sc[i] > sc[i + 1] or (sc[i] == sc[i + 1] and out_ids[i] < out_ids[i + 1]) for i in range(len(sc) - 1))


def test_golden_fixture_is_reproduced_by_the_oracle():
    """tests/golden/example_golden.npz travels to the GPU box; the oracle must still produce exactly that."""
    g = np.load(os.path.join(GOLDEN, "example_golden.npz"))
    for tag in ("a", "b"):
        m, k, n, idfw, max_len = (int(x) for x in g["params_" + tag])
        ix = O.OracleIndex(g["sess_off"], g["items"], g["ts"], m, max_len, float(idfw), fast=True)
        r = ix.predict_batch("canonical", g["q_items_" + tag], g["q_off_" + tag], k, m, n, business=True, threads=4)
        assert np.array_equal(r["counts"], g["counts_" + tag])
        assert np.array_equal(r["ids"], g["ids_" + tag])
        assert np.array_equal(r["scores"], g["scores_" + tag])
    assert len(g["q_off_a"]) - 1 == 931                              # README.md:172 "Qty test evaluations: 931"


def test_reference_example_readme_vectors(tmp_path):
    """GV-1 and AGG-1/2 of SURVEY.md 8c, straight from the reference's example data and README."""
    d = extract_example(tmp_path)
    off, items, ts, _ = O.read_tsv(os.path.join(d, "train.txt"))
    assert len(ts) == 23753                                          # last session dropped by the loader quirk (Q8)
    lens = np.diff(off.astype(np.int64))
    max_len = int(round(float(np.quantile(lens, 0.995))))
    assert max_len == 15
    test = read_test_data_evolving(os.path.join(d, "test.txt"))

    # GV-1: README.md:154, /v1/recommend?item_id=13598 with the shipped example.toml (m=500, k=50, how_many=21)
    readme = [2835, 10, 12068, 4313, 3097, 8028, 3545, 7812, 17519, 1164, 17935, 1277, 13335, 8655, 14664, 14556, 6868,
              13509, 9248, 2498, 11724]
    ix = O.OracleIndex(off, items, ts, 500, max_len, 1.0, fast=True)
    all_ids, all_sc, _ = ix.scores_canonical([13598], 50, 500)
    table = dict(zip(all_ids.tolist(), all_sc.tolist()))
    assert_valid_topn(np.array(readme, np.uint64), np.array([table[i] for i in readme]), all_ids, all_sc, 21, exclude=[13598])
    for predict in (ix.predict_literal, ix.predict_canonical):
        ids, sc = predict([13598], 50, 500, 21, True)
        assert set(ids.tolist()) == set(readme)
        np.testing.assert_allclose(sc[:3], [10.134, 9.5101, 9.1452], rtol=2e-4)

    # AGG-1: README.md:170-172 -- 931 evaluations, HitRate@20 0.6402, Mrr@20 0.3277 (tie noise on MRR only)
    qs = evaluator_queries(test, 2)
    assert len(qs) == 931
    flat, qoff = flatten([q for q, _ in qs])
    nxt = [n for _, n in qs]
    for which, mrr_tol in (("literal", 0.002), ("canonical", 0.005)):
        r = ix.predict_batch(which, flat, qoff, 50, 500, 20, business=True, threads=4)
        recs = [r["ids"][i, :r["counts"][i]].tolist() for i in range(len(qs))]
        mrr, hit = mrr_hitrate(recs, nxt, 20)
        assert hit == pytest.approx(0.6402, abs=0.0025)
        assert mrr == pytest.approx(0.3277, abs=mrr_tol)
    mrr, hit = mrr_hitrate([r["ids"][i, :r["counts"][i]].tolist() for i in range(len(qs))], nxt, 20)
    assert round(hit, 4) == 0.6402                                  # canonical tie-break reproduces the README digit for digit

    # AGG-2: README.md:64-71 -- TPE optimum m=1502 k=288 last_items=4 idf_weighting=2 -> test MRR@20 0.3401
    ix2 = O.OracleIndex(off, items, ts, 1502, max_len, 2.0, fast=True)
    qs4 = evaluator_queries(test, 4)
    flat, qoff = flatten([q for q, _ in qs4])
    r = ix2.predict_batch("literal", flat, qoff, 288, 1502, 20, business=True, threads=4)
    mrr, _ = mrr_hitrate([r["ids"][i, :r["counts"][i]].tolist() for i in range(len(qs4))], [n for _, n in qs4], 20)
    assert mrr == pytest.approx(0.3401, abs=0.005)
    # no k/m cut is ever hit on this data, so literal and canonical neighbour sets coincide on all 931 queries
    for q, _ in qs4[::7]:
        a, _ = ix2.find_neighbors_literal(q, 288, 1502)
        b, _, _ = ix2.neighbors_canonical(q, 288, 1502)
        assert set(a.tolist()) == set(b.tolist())


def test_restricted_parallel_builder_equals_prepare_hashmap():
    """prepare_hashmap_restricted (posting lists only for a query sample's items, idf of every item, built on several threads -- what makes an oracle check of
    BASELINE configs[4], 2.3 B interactions, fit a test) against prepare_hashmap_fast, which the tests above pin on the literal builder: same lists (tied
    timestamps included), same idf, same total, same answers from both restatements; and it refuses a query about a known item it holds no list for."""
    from helpers import flatten, random_queries, small_dataset
    off, items, ts, ids = small_dataset(91, n_sessions=5000, n_items=300, tied_timestamps=True, max_len=20)
    qs = random_queries(5, ids, 300, max_len=6)
    flat, qoff = flatten(qs)
    full = O.OracleIndex(off, items, ts, 60, 12, 2.0, fast=True)
    lit = O.OracleIndex(off, items, ts, 60, 12, 2.0, fast=False)
    for thr in (1, 3, 8):
        r = O.OracleIndex(off, items, ts, 60, 12, 2.0, wanted=flat, threads=thr)
        assert r.num_items == full.num_items == lit.num_items and r.total_pairs == full.total_pairs
        for it in np.unique(flat):
            a, b, c = full.postings(int(it)), r.postings(int(it)), lit.postings(int(it))
            if a[0] is None:
                assert b[0] is None
                continue
            assert np.array_equal(a[0], b[0]) and np.array_equal(c[0], b[0]) and a[1] == b[1] == c[1]
        for which in ("canonical", "literal"):
            x, y = full.predict_batch(which, flat, qoff, 50, 60, 21, threads=2), r.predict_batch(which, flat, qoff, 50, 60, 21, threads=2)
            assert np.array_equal(x["ids"], y["ids"]) and np.array_equal(x["scores"], y["scores"]) and np.array_equal(x["counts"], y["counts"])
    seen = set(flat.tolist())
    other = next(int(i) for i in ids if int(i) not in seen)
    with pytest.raises(ValueError):
        r.predict_batch("canonical", np.array([other], np.uint64), np.array([0, 1], np.uint32), 50, 60, 21)


def _divergence(ix_a, which_a, ix_b, which_b, qs, k, m, n, training_items):
    """Two predict variants over one workload: share of queries whose top-n SETS differ, whose ranked lists differ, and the 8 metric deltas (b - a) @ n - 1."""
    from helpers import eight_metrics, flatten
    flat, qoff = flatten([q for q, _ in qs])
    nxt = [x for _, x in qs]
    ra = ix_a.predict_batch(which_a, flat, qoff, k, m, n, business=True, threads=4)
    rb = ix_b.predict_batch(which_b, flat, qoff, k, m, n, business=True, threads=4)
    la = [ra["ids"][i, :ra["counts"][i]].tolist() for i in range(len(qs))]
    lb = [rb["ids"][i, :rb["counts"][i]].tolist() for i in range(len(qs))]
    set_diff = sum(set(a) != set(b) for a, b in zip(la, lb)) / float(len(qs))
    order_diff = sum(a != b for a, b in zip(la, lb)) / float(len(qs))
    ma, mb = eight_metrics(la, nxt, training_items, n - 1), eight_metrics(lb, nxt, training_items, n - 1)
    return set_diff, order_diff, {kk: mb[kk] - ma[kk] for kk in ma}, ma


def _tied_workload(seed=77):
    """Tied-timestamp synthetic set: 6 000 training sessions on 750 distinct timestamps (8 sessions share one on average), 400 held-out sessions as evaluator prefixes."""
    from helpers import evaluator_queries, small_dataset
    off, items, ts, ids = small_dataset(seed, n_sessions=6000, n_items=400, tied_timestamps=True, max_len=12)
    rng = np.random.default_rng(seed + 1)
    w = 1.0 / np.arange(1, len(ids) + 1) ** 0.9
    w /= w.sum()
    test = {s: [int(x) for x in ids[rng.choice(len(ids), size=int(rng.integers(2, 9)), p=w)]] for s in range(400)}
    return off, items, ts, evaluator_queries(test, 4)


def test_what_canonical_costs_against_the_literal_reference_on_tied_data(capsys):
    """the canonical closed form replaces the reference's container-order-dependent behaviour at ties and
    the t-digest p99.5 (vmis_index.rs:689-716, Q10) by the exact quantile.  How far can that move the reference's own quality numbers?  Measured here against the
    LITERAL restatement (same loops, heaps and scan orders as vmis_index.rs:325-415 / mod.rs:118-215, with this oracle's map iteration order standing in for
    hashbrown's) on a tied-timestamp synthetic set, and on the reference's example data (tests/golden/example_sessions.zip: 306 of its sessions share a timestamp).
    The numbers are copied into DESIGN.md section 2; the asserts are the bounds that table claims."""
    rows = []
    off, items, ts, qs = _tied_workload()
    for (k, m) in ((50, 500), (100, 200)):                      # (no cut hit / m-cut and k-cut both hit)
        ix = O.OracleIndex(off, items, ts, m, 12, 1.0, fast=True)
        sd, od, dm, base = _divergence(ix, "literal", ix, "canonical", qs, k, m, 21, items)
        rows.append(("synthetic tied, k=%d m=%d" % (k, m), len(qs), sd, od, dm, base))
        assert abs(dm["Mrr"]) < 0.01 and abs(dm["HitRate"]) < 0.01 and abs(dm["Ndcg"]) < 0.01 and abs(dm["Recall"]) < 0.01, dm
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        d = extract_example(tmp)
        eoff, eitems, ets, _ = O.read_tsv(os.path.join(d, "train.txt"))
        test = read_test_data_evolving(os.path.join(d, "test.txt"))
        train_col = [int(l.split()[1]) for l in list(open(os.path.join(d, "train.txt")))[1:] if len(l.split()) >= 3]
    assert len(ets) - len(np.unique(ets)) > 100                                    # (timestamps do tie in the example)
    for (k, m, last, idfw) in ((50, 500, 2, 1.0), (288, 1502, 4, 2.0)):           # example.toml / BASELINE configs[0] (README TPE optimum)
        eqs = evaluator_queries(test, last)
        ix = O.OracleIndex(eoff, eitems, ets, m, 15, idfw, fast=True)
        sd, od, dm, base = _divergence(ix, "literal", ix, "canonical", eqs, k, m, 21, train_col)
        rows.append(("assets/example, k=%d m=%d last=%d" % (k, m, last), len(eqs), sd, od, dm, base))
        assert sd < 0.30 and abs(dm["Mrr"]) < 0.005 and abs(dm["HitRate"]) < 0.005, (sd, dm)
        # Q10: the reference's t-digest estimate of p99.5 may land one off the exact quantile (15): what a +-1 max_session_len does to canonical results
        for ml in (14, 16):
            ix2 = O.OracleIndex(eoff, eitems, ets, m, ml, idfw, fast=True)
            sd2, od2, dm2, _ = _divergence(ix, "canonical", ix2, "canonical", eqs, k, m, 21, train_col)
            rows.append(("assets/example, k=%d m=%d last=%d: max_session_len %d vs 15" % (k, m, last, ml), len(eqs), sd2, od2, dm2, None))
            assert abs(dm2["Mrr"]) < 0.01 and abs(dm2["HitRate"]) < 0.01, (ml, dm2)
    with capsys.disabled():
        for name, nq, sd, od, dm, base in rows:
            print("\n[canonical-vs-literal] %s: %d queries, top-21 set differs %.2f %%, ranked list differs %.2f %%; deltas %s%s" % (
                name, nq, 100 * sd, 100 * od, " ".join("%s %+.4f" % kv for kv in dm.items()),
                ("; literal: " + " ".join("%s %.4f" % kv for kv in base.items())) if base else ""))
