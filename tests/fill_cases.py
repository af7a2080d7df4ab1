"""Shared by the fill tests (test_fill_host.py, test_gpu_fill.py, test_gpu_fill_sessions.py): the sparse index and its queries, the popularity order in NumPy, the
brute-force restatement of DESIGN.md 4.9, and the expected rows of a call -- the canonical oracle's rows at the call's internal how_many, through filter_rows, then
through fill_rows.  Test-side only."""
import numpy as np

from helpers import flatten, random_queries, small_dataset

K, M, MAX_LEN = 100, 500, 6
NONE = 0xFFFFFFFF
SCORE_RTOL = 1e-12
ATTR_NONE, ATTR_ADULT, ATTR_FOR_SALE = 0xFF, 1, 2


def sparse_dataset():
    """400 sessions of up to 4 items over 2 000 ids: 505 distinct items, most of them in one or two sessions."""
    return small_dataset(41, n_sessions=400, n_items=2000, max_len=4)


def sparse_queries(ids):
    """600 sessions of up to 6 items drawn from all 2 000 ids, a tenth of the items unknown: most recent items the index has never seen give empty rows."""
    return random_queries(5, ids, 600, max_len=MAX_LEN, unknown_rate=0.1)


def popularity_order(items):
    """Count of sessions that hold the item descending, id ascending (every session is kept here, and a session holds an item once)."""
    u, c = np.unique(np.asarray(items, np.uint64), return_counts=True)
    return u[np.lexsort((u, -c))]


def draw_attrs(items, seed=4):
    """Attribute bytes as tests/test_gpu_exclude.py draws them -> (known ids, flags)."""
    rng = np.random.default_rng(seed)
    known = np.unique(items)
    return known, rng.choice(np.array([0, 1, 2, 3, 0xFF], np.uint8), size=len(known), p=[0.1, 0.05, 0.55, 0.2, 0.1])


def census(counts, how_many):
    c = np.asarray(counts)
    served = c != NONE
    return int((served & (c == 0)).sum()), int((served & (c > 0) & (c < how_many)).sum()), int((served & (c >= how_many)).sum())


class OracleRows:
    """The oracle's rows at some how_many for a batch (queries the kernels do not serve -- empty, longer than max_len -- get the count 0xFFFFFFFF), computed once each."""

    def __init__(self, oix, qs, max_len=MAX_LEN):
        self.oix, self.qs, self.memo = oix, qs, {}
        self.sel = np.array([i for i, q in enumerate(qs) if 1 <= len(q) <= max_len], np.int64)
        self.flat, self.off = flatten([qs[i] for i in self.sel])

    def rows(self, wide, business=False):
        if (wide, business) not in self.memo:
            r = self.oix.predict_batch("canonical", self.flat, self.off, K, M, wide, business, threads=4)
            ids, sc, cnt = np.zeros((len(self.qs), wide), np.uint64), np.zeros((len(self.qs), wide)), np.full(len(self.qs), NONE, np.uint32)
            ids[self.sel], sc[self.sel], cnt[self.sel] = r["ids"], r["scores"], r["counts"]
            for a in (ids, sc, cnt):
                a.setflags(write=False)
            self.memo[(wide, business)] = (ids, sc, cnt)
        return self.memo[(wide, business)]


def unfilled(orows, how_many, excl=None, cap=0, session=False, business=False, max_len=MAX_LEN):
    """What the call returns without the flag: the oracle's rows at the internal how_many, the lists (and the sessions) filtered out, cut to how_many; a list longer
    than cap marks its query 0xFFFFFFFF."""
    from serenade_amd.serving import filter_rows
    qs = orows.qs
    wide = how_many + cap + (max_len - 1 if session else 0)
    ids, sc, cnt = orows.rows(wide, business)
    if wide == how_many:
        return ids.copy(), sc.copy(), cnt.copy()
    gone = [list(excl[q] if excl is not None and cap else []) + (list(qs[q]) if session else []) for q in range(len(qs))]
    cnt = cnt.copy()
    if excl is not None and cap:
        cnt[[q for q in range(len(qs)) if len(excl[q]) > cap]] = NONE
    return filter_rows(ids, sc, cnt, gone, how_many)


def expected(orows, how_many, ranking, excl=None, cap=0, session=False, business=False, attrs=None, max_len=MAX_LEN):
    from serenade_amd.serving import fill_rows
    ids, sc, cnt = unfilled(orows, how_many, excl, cap, session, business, max_len)
    return fill_rows(ids, sc, cnt, orows.qs, ranking, how_many, excl=excl if excl is not None and cap else None, exclude_session=session, attrs=attrs, business=business)


def brute_force_fill(row_ids, session, ranking, how_many, excl=(), exclude_session=False, attrs=None, business=False):
    """DESIGN.md 4.9 restated entry by entry for ONE row of c = len(row_ids) < how_many model entries -> the ids appended to it."""
    r = session[-1]
    out = []
    for f in ranking:
        if len(row_ids) + len(out) >= how_many:
            break
        if f in row_ids or f == r or f in excl or (exclude_session and f in session):
            continue
        if business:
            fa = (attrs or {}).get(f)
            ra = (attrs or {}).get(r)
            if fa is None or fa == ATTR_NONE:       # f needs attributes: an id unknown to the index is dropped
                continue
            if not fa & ATTR_FOR_SALE:              # f must be for sale
                continue
            if fa & ATTR_ADULT and (ra is None or ra == ATTR_NONE or not ra & ATTR_ADULT):   # an adult f passes only when r has attributes and is adult
                continue
        out.append(f)
    return out


def check_rows(got, want, what):
    """Counts and ids exact, model scores within SCORE_RTOL, filled scores exactly -inf (assert_allclose compares infinities for equality)."""
    ids, sc, cnt = got
    wids, wsc, wcnt = want
    assert np.array_equal(cnt, wcnt), "%s: counts differ at queries %s (got %s, expected %s)" % (what, np.flatnonzero(cnt != wcnt)[:8], cnt[cnt != wcnt][:8], wcnt[cnt != wcnt][:8])
    inside = np.arange(ids.shape[1])[None, :] < np.where(cnt == NONE, 0, cnt).astype(np.int64)[:, None]
    bad = np.flatnonzero(((ids != wids) & inside).any(axis=1))
    assert len(bad) == 0, "%s: ids differ at queries %s" % (what, bad[:8])
    assert np.array_equal(np.isneginf(sc) & inside, np.isneginf(wsc) & inside), "%s: -inf in other places" % what
    np.testing.assert_allclose(sc[inside], wsc[inside], rtol=SCORE_RTOL, atol=0)


def same_rows(got, ref, what):
    """Two GPU calls, bit for bit (inside the counts)."""
    ids, sc, cnt = got
    rids, rsc, rcnt = ref
    assert np.array_equal(cnt, rcnt), "%s: counts differ at %s" % (what, np.flatnonzero(cnt != rcnt)[:8])
    n = ids.shape[1]
    inside = np.arange(n)[None, :] < np.where(cnt == NONE, 0, np.minimum(cnt, n)).astype(np.int64)[:, None]
    assert np.array_equal(ids[inside], rids[inside]), "%s: ids differ" % what
    assert np.array_equal(sc[inside].view(np.uint64), rsc[inside].view(np.uint64)), "%s: scores differ in their bits" % what


class Device:
    """A batch and its lists in device memory; call() = srn_predict_batch_device_excl into buffers pre-filled with garbage."""

    def __init__(self, gix, qs, excl=None):
        import torch
        self.torch, self.gix, self.nq = torch, gix, len(qs)
        self.flat, self.off = flatten(qs)
        self.xflat, self.xoff = flatten(excl if excl is not None else [[] for _ in qs])
        up = lambda a, t: torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(t).copy()).to("cuda:0")   # noqa: E731
        self.d_flat, self.d_off, self.d_xflat, self.d_xoff = up(self.flat, np.int64), up(self.off, np.int32), up(self.xflat, np.int64), up(self.xoff, np.int32)

    def call(self, how_many, cap=0, business=False, session=False, fill=True, max_len=MAX_LEN):
        import serenade_amd as sa
        t = self.torch
        ids = t.full((self.nq * how_many,), 0x5A5A5A5A5A5A5A5A, dtype=t.int64, device="cuda:0")
        sc = t.full((self.nq * how_many,), float("nan"), dtype=t.float64, device="cuda:0")
        cnt = t.full((self.nq,), int(np.array([0x80000001], np.uint32).view(np.int32)[0]), dtype=t.int32, device="cuda:0")
        sa.predict_batch_device_excl(self.gix, self.d_flat.data_ptr(), self.d_off.data_ptr(), self.nq, max_len, self.d_xflat.data_ptr() if cap else 0,
                                     self.d_xoff.data_ptr() if cap else 0, cap, K, M, how_many, business, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(),
                                     t.cuda.current_stream().cuda_stream, exclude_session=session, fill=fill)
        t.cuda.synchronize()
        return ids.cpu().numpy().view(np.uint64).reshape(self.nq, how_many), sc.cpu().numpy().reshape(self.nq, how_many), cnt.cpu().numpy().view(np.uint32)
