"""Click logs for the split tests (test_prepare_host.py, test_gpu_prepare.py): the case worked by hand and seeded random logs.  Test-side only."""
import numpy as np

A, B, C_, D, E = 101, 102, 103, 104, 105
# (session, item, time); S = 2, L = 2, cutoff 100, start 10, end 200, known items on
HAND_ROWS = [(1, A, 5), (1, B, 8), (2, A, 20), (3, A, 25), (2, B, 30), (2, C_, 40), (3, B, 50), (4, C_, 60), (4, D, 61), (5, A, 90), (5, C_, 120), (6, B, 130),
             (6, E, 140), (7, A, 150), (7, B, 250), (8, D, 110), (8, A, 111)]
HAND_RULE = dict(cutoff=100, start=10, end=200, min_item_support=2, min_session_len=2, test_known_items=True)
# session 1 ends at 8 < start and session 7 at 250 >= end: OUT.  Train side: sessions 2, 3, 4 (rows 2..8); D has one train-side row: RARE (row 8); session 4 is
# left with one row: SHORT_TRAIN (row 7) -- C keeps its TRAIN row 5.  Test side: sessions 5, 6, 8; E has no TRAIN row and D lost its only one: UNKNOWN (rows 12, 15);
# sessions 6 and 8 are left with one row each: SHORT_TEST (rows 11, 16).
HAND_CODES = [16, 16, 1, 1, 1, 1, 1, 18, 17, 2, 2, 20, 19, 16, 16, 19, 20]
HAND_INFO = dict(train_rows=5, train_sessions=2, train_items=3, test_rows=2, test_sessions=1, test_items=2, dropped_out=4, dropped_rare=1, dropped_short_train=1,
                 dropped_unknown=2, dropped_short_test=2, sessions=8, items=5, t_min=5, t_max=250)
NO_POS = 0xFFFFFFFF
DAY = 86400
T0 = 1_600_000_000


def hand():
    s, i, t = (np.array(c) for c in zip(*HAND_ROWS))
    return s.astype(np.uint64), i.astype(np.uint64), t.astype(np.int64)


def hand_f64():
    """The hand case on half seconds: x - 0.5 rounds up to x, x + 0.25 down to it; the two rows of session 1 (OUT either way) are a negative time and a nan."""
    s, i, t = hand()
    f = t.astype(np.float64) + np.where(np.arange(len(t)) % 2 == 0, -0.5, 0.25)
    f[0], f[1] = -3.0, np.nan
    return s, i, f


def random_log(seed, n=2000, n_sessions=300, n_items=60, days=3, f64=False, id_base=0):
    """n rows of n_sessions sessions over `days` days, items Zipf over n_items, rows in shuffled order (sessions interleaved), times on a 30-second grid (ties inside
    and across sessions); f64: about half of the times half a second early (both roundings occur).  id_base is added to both id columns (mod 2^64)."""
    rng = np.random.default_rng(seed)
    sess = rng.integers(0, n_sessions, n)
    begin = rng.integers(0, days * DAY - 3600, n_sessions)
    t = T0 + begin[sess] + 30 * rng.integers(0, 40, n)
    w = 1.0 / np.arange(1, n_items + 1)
    item = rng.choice(n_items, n, p=w / w.sum())
    with np.errstate(over="ignore"):
        s64 = (sess.astype(np.uint64) * np.uint64(7) + np.uint64(3)) + np.uint64(id_base)
        i64 = (item.astype(np.uint64) * np.uint64(11) + np.uint64(5)) + np.uint64(id_base)
    if f64:
        return s64, i64, t.astype(np.float64) - 0.5 * rng.integers(0, 2, n)
    return s64, i64, t.astype(np.int64)


def rule_for(times, **kw):
    """Cutoff at the last day of a random_log, the window starting half a day in."""
    rule = dict(cutoff=T0 + 2 * DAY, start=T0 + DAY // 2, end=T0 + 3 * DAY - 7200, min_item_support=5, min_session_len=2, test_known_items=True)
    rule.update(kw)
    return rule


def check_properties(sess, item, code, pos, rule):
    """What any split must satisfy."""
    code, pos = np.asarray(code), np.asarray(pos)
    assert set(np.unique(code).tolist()) <= {1, 2, 16, 17, 18, 19, 20}                         # the codes partition the rows: one of them each
    train, test = code == 1, code == 2
    side_train, side_test = np.isin(code, (1, 17, 18)), np.isin(code, (2, 19, 20))
    assert not set(sess[side_train].tolist()) & set(sess[side_test].tolist())                  # no session has rows on both sides
    assert not set(sess[code == 16].tolist()) & set(sess[code != 16].tolist())                 # ... and OUT takes whole sessions
    if rule.get("test_known_items", True):
        assert set(item[test].tolist()) <= set(item[train].tolist())                           # every TEST item has a TRAIN row
    L = max(int(rule.get("min_session_len", 2)), 1)
    for side in (train, test):
        if side.any():
            assert np.unique(sess[side], return_counts=True)[1].min() >= L
        assert np.array_equal(pos[side], np.arange(int(side.sum()), dtype=np.uint32))          # pos is a stable rank
    assert (pos[~(train | test)] == NO_POS).all()
