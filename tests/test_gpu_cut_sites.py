"""The lean fast kernel's two k-cut sites against the canonical CPU oracle: the fused cut (fast_cut<6>, merged runs of n <= 3 072 entries) and the two-pass cut
(n > 3 072).  Both count their numerator classes per wave with wave_class_counts (srn_device.h); the general kernel's site is covered by the `no_fast` parameter of
tests/test_gpu_parity.py.

Queries of exactly two distinct known items: two posting lists, numerators <= 3, and 2 n + 8 <= 12 032 words of merge buffers, so the lean form serves every one of
them (asserted: nothing reaches the general kernel).  A list is staged down to the m-th rank of the longest list (x_lo, srn_prep.h), so n <= 2 m: m = 1000 keeps
every query at the fused site; m = 2500 puts those whose lists overlap in time beyond 3 072.  n is restated here from the oracle's posting lists."""
import numpy as np
import pytest

from helpers import flatten, small_dataset

pytestmark = pytest.mark.gpu

SCORE_RTOL = 1e-12   # (as tests/test_gpu_parity.py: one f64 multiply + divide of an exact integer accumulator on both sides)
FUSED_MAX_N = 3072   # 6 entries per thread of a 512-thread workgroup
N_QUERIES = 48


def _two_item_queries(seed, ids, n):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, len(ids) + 1) ** 0.9
    w /= w.sum()
    return [[int(x) for x in ids[rng.choice(len(ids), size=2, replace=False, p=w)]] for _ in range(n)]


def _staged(oix, ts, query, m):
    """Entries of the merged run: every list cut to its m most recent sessions, then to the ranks at or above x_lo = the largest m-th rank of a list that has m
    entries (timestamps are distinct here: they order like the ranks)."""
    lists = []
    for item in dict.fromkeys(query):
        sessions, _idf = oix.postings(item)
        t = ts[sessions].astype(np.int64)
        assert (np.diff(t) < 0).all(), "a posting list runs from the most recent session down"
        lists.append(t[:m])
    x_lo = max([int(t[m - 1]) for t in lists if len(t) >= m], default=0)
    return sum(int((t >= x_lo).sum()) for t in lists)


@pytest.fixture(scope="module")
def data():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(21, n_sessions=30000, n_items=90, max_len=34)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 5000, 34, 1.0)
    oix = O.OracleIndex(off, items, ts, 5000, 34, 1.0)
    return gix, oix, ts, _two_item_queries(31, ids, N_QUERIES)


def _check_batch(gix, oix, queries, k, m, how_many):
    """tests/test_gpu_parity.py's _check_batch: ids, order, counters and neighbour sets identical, scores to 1e-12; the product call equal to the debug call."""
    import serenade_amd as sa
    res = sa.predict_batch_debug(gix, queries, k, m, how_many, False, neighbours=True)
    flat, off = flatten(queries)
    ref = oix.predict_batch("canonical", flat, off, k, m, how_many, False, threads=4, want_stats=True)
    assert np.array_equal(res["counts"], ref["counts"]), "result counts differ"
    for q in range(len(queries)):
        n = int(ref["counts"][q])
        assert np.array_equal(res["ids"][q, :n], ref["ids"][q, :n]), (q, queries[q], res["ids"][q, :n], ref["ids"][q, :n])
        np.testing.assert_allclose(res["scores"][q, :n], ref["scores"][q, :n], rtol=SCORE_RTOL, atol=0)
    assert np.array_equal(res["stats"][:, :7].astype(np.uint64), ref["stats"]), "P,C,K,I,D,H,L counters differ"
    ids, scores, counts = sa.predict_batch(gix, queries, k, m, how_many, False)
    assert gix.last_path_counts()[1] == 0, "a query went to the general kernel: the lean form's site did not serve it"
    assert np.array_equal(counts, res["counts"]) and np.array_equal(ids, res["ids"]) and np.array_equal(scores, res["scores"]), \
        "filtered (product) path differs from the unfiltered (debug) path"
    for q in range(len(queries)):
        sid, num, _U = oix.neighbors_canonical(queries[q], k, m)
        kq = int(res["nb_counts"][q])
        got = sorted(zip(res["nb_sessions"][q, :kq].tolist(), res["nb_num"][q, :kq].tolist()))
        assert got == sorted(zip(sid.tolist(), num.tolist())), (q, queries[q])
    return res


@pytest.mark.parametrize("k,m,two_pass", [(300, 1000, False), (1500, 2500, True)], ids=["fused_site", "two_pass_site"])
def test_cut_site_vs_oracle(data, k, m, two_pass):
    gix, oix, ts, queries = data
    n = np.array([_staged(oix, ts, q, m) for q in queries])
    assert 2 * int(n.max()) + 8 <= 12032, "a merged run beyond the lean form's merge buffers"
    res = _check_batch(gix, oix, queries, k, m, 21)
    st = res["stats"]
    assert (st[:, 1] == m).any() and (st[:, 2] == k).any(), "both cuts should be exercised"
    bites = st[:, 1].astype(np.int64) > k                     # more sessions behind the m-cut than k: the k-cut counts its classes
    assert (n <= st[:, 0].astype(np.int64)).all()              # (P = the lists cut to m entries each; x_lo can only shorten them)
    side = (n > FUSED_MAX_N) if two_pass else (st[:, 0].astype(np.int64) <= FUSED_MAX_N)
    assert two_pass or (n <= FUSED_MAX_N).all()
    share = float((bites & side).mean())
    print("k %d m %d: n %d..%d, share of queries whose k-cut bites at the %s site: %.3f" % (k, m, n.min(), n.max(), "two-pass" if two_pass else "fused", share))
    assert share >= 1.0 / 3.0, share
