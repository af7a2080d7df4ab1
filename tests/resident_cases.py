"""Event rows for the device-resident index build's tests (test_gpu_resident_build.py): designed sessions written out as the (session id, item id, time) rows that
srn_sessions_from_events groups back into them.  Test-side only; NumPy alone.

A case is a dict: sess, items (uint64[n]), times (float64[n] or int64[n]), m (m_most_recent_sessions), idfw, max_session_len (0: the p99.5 rule) and what a test
wants to know about the design (n_kept, quantile_overflow ...).  Rows are written session after session unless a case shuffles them; the file's last row is always a
one-row session of the largest id, which read_from_file's quirk drops whole, so every designed session arrives as designed."""
import numpy as np

LENS = (1, 2, 14, 15, 16, 17, 30, 31, 32, 40)     # around the slot kernels' limits: 15 items inline, 30 in a packed slot
BLOCK = 1024                                       # rows per block of rows_to_slots_kernel / rows_to_packed_kernel


def item_pool(rng, n_items, wide=False):
    """n_items distinct public ids; wide: spread over all 64 bits."""
    if wide:
        ids = np.unique(rng.integers(0, 2**64, size=2 * n_items, dtype=np.uint64))
        ids = rng.permutation(ids)[:n_items]
        ids[:2] = np.array([2**64 - 1, 2**63], np.uint64)
        return ids
    return (np.uint64(10**6) + rng.permutation(np.arange(7, 7 + 13 * n_items, 13, dtype=np.uint64)))[:n_items]


def rows_of(session_ids, rows, stamps, rng, shuffle=False, repeat=0.0, int_times=False):
    """Designed sessions -> event rows.  Session j has the id session_ids[j], the distinct items rows[j] and the timestamp stamps[j]: its rows carry times <= stamps[j],
    one of them exactly stamps[j].  repeat: that share of the rows is written a second time LATER in the session with a larger time (read_from_file ignores the repeat,
    its time included).  A closing one-row session of the largest id follows (dropped by the loader)."""
    s_col, i_col, t_col = [], [], []
    for sid, row, ts in zip(session_ids, rows, stamps):
        row = np.asarray(row, np.uint64)
        order = rng.permutation(len(row))
        t = np.full(len(row), float(ts)) - rng.integers(0, 3, size=len(row))
        t[rng.integers(0, len(row))] = float(ts)
        t = np.maximum(t, 0.0)
        items, times = row[order], t
        if repeat > 0.0:
            again = np.flatnonzero(rng.random(len(row)) < repeat)
            items = np.concatenate([items, items[again]])
            times = np.concatenate([times, np.full(len(again), float(ts) + 1000.0)])
        s_col.append(np.full(len(items), sid, np.uint64)); i_col.append(items); t_col.append(times)
    sess, items, times = np.concatenate(s_col), np.concatenate(i_col), np.concatenate(t_col)
    if shuffle:   # (the loader's sort by session is stable: a session's rows keep their relative order, which is all that a repeat's "later" needs)
        n = len(sess)
        key = rng.random(n)
        grouped = np.lexsort((np.arange(n), sess))          # rows by session, written order inside
        new_key = np.empty(n)
        new_key[grouped] = key[np.lexsort((key, sess))]      # ... get their session's keys in ascending order
        out = np.argsort(new_key, kind="stable")
        sess, items, times = sess[out], items[out], times[out]
    last = np.uint64(int(np.max(session_ids)) + 1)
    sess = np.concatenate([sess, [last]]).astype(np.uint64)
    items = np.concatenate([items, items[:1]]).astype(np.uint64)
    times = np.concatenate([times, [0.0]])
    if not int_times:
        times = times + np.where(rng.random(len(times)) < 0.5, 0.25, -0.25) * (times > 0)   # rounded back by the loader
    return sess, items, (times.astype(np.int64) if int_times else times.astype(np.float64))


def draw_rows(rng, pool, lengths):
    w = 1.0 / np.arange(1, len(pool) + 1) ** 0.8
    w /= w.sum()
    return [pool[rng.choice(len(pool), size=int(ln), replace=False, p=w)] for ln in lengths]


def block_edge_lengths(n_kept, max_len, rng):
    """Lengths of the KEPT sessions by recency rank: rows longer than 15 (and, where max_len allows, longer than 30) on the first and the last row of the first, a middle
    and the last block that holds rows, every other row at most 15 items -- so every second block has no overflow at all and two consecutive block_base entries are equal."""
    allowed = [ln for ln in LENS if ln <= max_len]
    short = [ln for ln in allowed if ln <= 15]
    long_ = [ln for ln in allowed if ln > 15] or short
    lens = rng.choice(short, size=n_kept)
    n_blocks = (n_kept + BLOCK - 1) // BLOCK
    marked = sorted({0, n_blocks - 1} | ({n_blocks // 2} if n_blocks >= 5 else set()))
    for b in marked:
        lo, hi = b * BLOCK, min(n_kept, (b + 1) * BLOCK)
        spots = sorted({lo, hi - 1} | set(rng.integers(lo, hi, size=min(2 * len(long_), hi - lo)).tolist()))
        for j, r in enumerate(spots):
            lens[r] = long_[j % len(long_)]
        lens[hi - 1] = long_[-1]     # the block's (and, in the last block, the index's) last row: the longest there is
    return lens, marked


def block_edges(n_kept, max_session_len, seed, huge=0, huge_share=False):
    """n_kept sessions survive an explicit max_session_len (40: all of them; 16: longer ones are dropped in between).  max_session_len = 0: the device quantile decides;
    huge: that many sessions of 4 100 items on top (past the length histogram's bins); huge_share: they are > 0.5 % of all sessions, so the p99.5 itself lies there."""
    rng = np.random.default_rng(seed)
    pool = item_pool(rng, 300)
    cap = max_session_len or 40
    lens, marked = block_edge_lengths(n_kept, cap, rng)
    lens = lens.tolist()
    dropped = [ln for ln in LENS if ln > cap]
    if dropped:   # sessions that the cut removes, between the kept ones
        at = sorted(rng.integers(0, n_kept + 1, size=max(1, n_kept // 10)).tolist(), reverse=True)
        for j, a in enumerate(at):
            lens.insert(a, dropped[j % len(dropped)])
    rows = draw_rows(rng, pool, lens)
    if huge:
        bulk = np.uint64(5 * 10**7) + np.arange(4100, dtype=np.uint64)
        for a in sorted(rng.integers(0, len(rows) + 1, size=huge).tolist(), reverse=True):
            rows.insert(a, bulk.copy())
    n = len(rows)
    sess, items, times = rows_of(np.arange(1, n + 1, dtype=np.uint64), rows, 1000 + np.arange(n), rng)   # ascending stamps: recency rank = order among the kept
    return dict(sess=sess, items=items, times=times, m=500, idfw=1.0, max_session_len=max_session_len, n_kept=n_kept if max_session_len else None, marked=marked,
                huge=huge, huge_share=huge_share)


def ties_and_cuts(m_index, idfw, seed=7, n=600):
    """Many sessions per timestamp (ranks fall back to session order) and items held by exactly 1, m_index - 1, m_index and m_index + 1 sessions."""
    rng = np.random.default_rng(seed)
    pool = item_pool(rng, 120)
    rows = [list(r) for r in draw_rows(rng, pool, rng.integers(1, 9, size=n))]
    marked = (np.uint64(9 * 10**8) + np.arange(4, dtype=np.uint64)).tolist()
    for item, count in zip(marked, (1, max(m_index - 1, 1), m_index, m_index + 1)):
        for s in rng.choice(n, size=count, replace=False).tolist():
            rows[s].append(item)
    sess, items, times = rows_of(np.arange(1, n + 1, dtype=np.uint64), rows, 5000 + np.arange(n) // 50, rng)
    return dict(sess=sess, items=items, times=times, m=m_index, idfw=idfw, max_session_len=40, marked_items=marked)


def row_forms(int_times, seed=21, n=700):
    """Shuffled file order, repeated (session, item) rows, session ids from 2^32 up and item ids over all 64 bits; times f64 or int64."""
    rng = np.random.default_rng(seed)
    pool = item_pool(rng, 150, wide=True)
    rows = draw_rows(rng, pool, rng.integers(1, 13, size=n))
    ids = np.uint64(2**32) + np.sort(rng.choice(2**40, size=n, replace=False).astype(np.uint64))
    ids[-1] = np.uint64(2**63 - 5)      # (below 2^63: a torch tensor carries the ids as int64; the closing session takes the next id)
    sess, items, times = rows_of(ids, rows, 10**6 + rng.permutation(n), rng, shuffle=True, repeat=0.15, int_times=int_times)
    return dict(sess=sess, items=items, times=times, m=50, idfw=1.0, max_session_len=0)


def one_row():
    return dict(sess=np.array([5], np.uint64), items=np.array([9], np.uint64), times=np.array([3.5]), m=10, idfw=1.0, max_session_len=0)


def all_too_long(seed=3):
    rng = np.random.default_rng(seed)
    pool = item_pool(rng, 60)
    rows = draw_rows(rng, pool, rng.integers(5, 12, size=40))
    sess, items, times = rows_of(np.arange(1, 41, dtype=np.uint64), rows, 100 + np.arange(40), rng)
    return dict(sess=sess, items=items, times=times, m=10, idfw=1.0, max_session_len=4)


def read_tsv_rows(path):
    """The rows of a reference-format TSV file as from_events takes them (header skipped)."""
    sess, items, times = [], [], []
    with open(path) as f:
        next(f)
        for line in f:
            p = line.split()
            if len(p) >= 3:
                sess.append(int(p[0])); items.append(int(p[1])); times.append(float(p[2]))
    return np.array(sess, np.uint64), np.array(items, np.uint64), np.array(times, np.float64)


def queries(case_items, seed, n=2000, max_len=10):
    """n evolving sessions over the case's own items (popular ones more often), 1..max_len items, an item repeated now and then, a few ids the index has never seen."""
    rng = np.random.default_rng(seed)
    ids, counts = np.unique(case_items, return_counts=True)
    pop = ids[np.argsort(-counts, kind="stable")]
    w = 1.0 / np.arange(1, len(pop) + 1) ** 0.9
    w /= w.sum()
    unknown = [int(x) for x in (np.uint64(3) + rng.integers(0, 2**62, size=16, dtype=np.uint64)) if x not in set(ids.tolist())]
    qs = []
    for j in range(n):
        ln = int(rng.integers(1, 5)) if j % 4 else int(rng.integers(1, max_len + 1))
        q = [int(x) for x in pop[rng.choice(len(pop), size=ln, p=w)]]
        if rng.random() < 0.05:
            q[int(rng.integers(0, ln))] = unknown[int(rng.integers(0, len(unknown)))]
        qs.append(q)
    qs[0] = [unknown[0]]
    return qs
