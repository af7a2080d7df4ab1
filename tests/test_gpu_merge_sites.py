"""The fast kernel's merge tree at its call sites, against the canonical CPU oracle: the lean form's three shapes -- two runs (one merge), three (two levels, the second
against a single run) and four (two pairs side by side, the second team counted from thread 511 down, then one merge of the two results) -- and the MID form's tree of up
to three levels over 5..8 runs.  All of them call the same merge_pair (srn_fast.hip; alone in tests/test_gpu_merge_pair.py).

Data set and comparisons are those of tests/test_gpu_cut_sites.py: ids and order exact, scores to 1e-12, the P, C, K, I, D, H, L counters, the neighbour sets with
their numerators, and the product call equal to the debug call.  48 queries each of exactly 2, 3 and 4 distinct known items: L <= 4, weights summing to <= 10, <= 4
lists and n <= 4 m <= 5 600 entries, so 2 n + 8 <= 11 208 words fit the lean form's merge buffers and it serves every one (asserted: nothing reaches the general
kernel; the parent commit serves them all with seed 31 as well, so the seed is tests/test_gpu_cut_sites.py's).  How many runs a query really stages is restated from the
oracle's posting lists: a list is cut to its m most recent sessions and then to the ranks at or above x_lo, which can empty it."""
import numpy as np
import pytest

from helpers import small_dataset
from test_gpu_cut_sites import _check_batch

pytestmark = pytest.mark.gpu

PER_SIZE = 48


def _distinct_queries(seed, ids, sizes, per_size):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, len(ids) + 1) ** 0.9
    w /= w.sum()
    return [[int(x) for x in ids[rng.choice(len(ids), size=int(rng.choice(np.atleast_1d(s))), replace=False, p=w)]] for s in sizes for _ in range(per_size)]


def _staged_lists(oix, ts, query, m):
    """Entries each list of the query stages: cut to its m most recent sessions, then to the ranks at or above x_lo = the largest m-th rank of a list that has m entries
    (timestamps are distinct here: they order like the ranks)."""
    lists = []
    for item in dict.fromkeys(query):
        sessions, _idf = oix.postings(item)
        t = ts[sessions].astype(np.int64)
        assert (np.diff(t) < 0).all(), "a posting list runs from the most recent session down"
        lists.append(t[:m])
    x_lo = max([int(t[m - 1]) for t in lists if len(t) >= m], default=0)
    return [int((t >= x_lo).sum()) for t in lists]


@pytest.fixture(scope="module")
def data():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(21, n_sessions=30000, n_items=90, max_len=34)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 5000, 34, 1.0)
    oix = O.OracleIndex(off, items, ts, 5000, 34, 1.0)
    return gix, oix, ts, ids


@pytest.mark.parametrize("k,m", [(300, 1000), (500, 1400)])
def test_lean_merge_tree_vs_oracle(data, k, m):
    gix, oix, ts, ids = data
    queries = _distinct_queries(31, ids, [2, 3, 4], PER_SIZE)
    staged = [_staged_lists(oix, ts, q, m) for q in queries]
    runs = np.array([sum(1 for c in s if c > 0) for s in staged])
    n = np.array([sum(s) for s in staged])
    assert 2 * int(n.max()) + 8 <= 12032, "a merged run beyond the lean form's merge buffers"
    for want in (2, 3, 4):
        assert int((runs == want).sum()) >= 12, "queries that stage %d non-empty lists: %d" % (want, int((runs == want).sum()))
    for b in range(0, len(queries), PER_SIZE):    # (one call per session length: 48 queries, as tests/test_gpu_cut_sites.py -- a call of 49 .. 256 queries takes the latency path's general kernel)
        _check_batch(gix, oix, queries[b:b + PER_SIZE], k, m, 21)     # (asserts that the general kernel served none of them)
    print("k %d m %d: n %d..%d, queries by staged runs %s" % (k, m, n.min(), n.max(), np.bincount(runs, minlength=5).tolist()))


def test_mid_merge_tree_vs_oracle(data):
    """Sessions of 5..8 distinct known items (the MID form takes sessions of up to 10): 5..8 runs, three merge levels, a run without a partner copied by a merge with
    an empty one.  m = 700: n <= 5 600, so 2 n + 264 words fit the MID form's room."""
    gix, oix, ts, ids = data
    k, m = 300, 700
    queries = _distinct_queries(32, ids, [[5, 6, 7, 8]], 6 * PER_SIZE)   # (288 in one call: above the latency path, so the lean form lists them for the MID form)
    assert len(set(map(tuple, queries))) == len(queries)                 # (no two alike: none is served as another's copy)
    runs = np.array([sum(1 for c in _staged_lists(oix, ts, q, m) if c > 0) for q in queries])
    assert (runs >= 5).sum() >= 12, np.bincount(runs).tolist()
    _check_batch(gix, oix, queries, k, m, 21)
    mid = gix.last_mid_count()
    print("k %d m %d: queries by staged runs %s, %d listed for the MID form" % (k, m, np.bincount(runs, minlength=9).tolist(), mid))
    assert mid >= int((runs >= 5).sum()), "queries of more than four runs go through the MID form"
