"""A DESIGNED index for the fast kernels' exact thresholds (test_edge_cases_host.py, test_gpu_edge_cases.py): every query's list lengths, kept counts, staged total,
candidate count and numerator classes are chosen, not drawn.  NumPy only, deterministic, no GPU.  Test-side only.

The index is a concatenation of CELLS; one cell serves one query (and, for sessions of up to 7 items, two more: the same session with an id the index has never seen
on top, which moves every position by one, and with a copy of its oldest known item on top, which makes that item's list run 0).  A cell owns its query items and its sessions; cells lie on disjoint, ascending stretches of the time line and session indices
ascend with time, so a session's recency rank (srn_index.cpp: position in (timestamp, session index) order) IS its index, in both timestamp variants:
  distinct   timestamp = T0 + session index
  tied       timestamp = T0 + session index // 8: groups of 8 equal timestamps, the same (timestamp, index) order and so the same designed counts -- but tie groups now
             straddle x_lo and the k-cut's boundary.
Inside a cell the time line is [below the cut][the cut session][above the cut]: a list with count >= m (a PIVOT) whose m-th most recent session is the cut session sets
x_lo; list i has kept_i sessions from the cut session on and count_i - kept_i before it, each stretch an even interleave of the lists.  With no pivot x_lo = 0 and
kept = count.  `shared` sessions hold the two most recent known items at once (numerator classes that are sums; C < n).  `touch` lists have the cut session as their
OLDEST kept entry (last entry == x_lo exactly).  Every session row = its query items + payload items, ascending ids, <= 34 items.

One index (m_index = F_M_MAX), two call shapes SHAPES = (k, m): every cell is designed for one m and is still a valid query at the other; `restate` works out every
designed quantity from the sessions ALONE for any (k, m), and `census` asserts from it, edge by edge, that both sides of every edge are hit.

The constants, with where they come from:
  F_M_MAX 2 560, F_K_MAX 1 536                           srn_kernels.h:84, :63
  a list is staged in (kept + 511) >> 9 loads             srn_prep.h:18 (ready_add), RW_LMASK srn_kernels.h:40
  lean:  L <= 8, sumw <= 15, nr <= 4, 2 n + 8 <= F_LEAN_MW (12 032)                       srn_prep.h:28, srn_fast.hip:651
  BIG :  the same shape, 2 n + 8 + 256 <= 19 072                                            srn_fast.hip:659-660
  MID :  L <= 10, sumw <= 63, nr <= 10, 2 n + 8 + 256 <= 12 032 (its BIG form: 19 072)     srn_fast.hip:650, :665-666
  LONG:  L 11..20, sumw <= 255, nr <= 20, 2 n + 8 + F_LONG_RES_WORDS <= 19 072             srn_fast.hip:649, srn_kernels.h:93-94
  fused cut iff a thread's chunk is <= 6 entries: n <= 6 * 512 = 3 072                      srn_fast.hip:891-901
  the x_lo search is 8-ary while hi - lo > 8, then 8 entries at once                        srn_prep.h:113-133
  F_FIN_ENTRIES 63 (a row finished in place), the finish kernel's hd.x > 31                 srn_kernels.h:86, srn_fast.hip:1568, :1638
  accumulators: idx < 16 replicated, < F_DIRECT = 3 968 direct, else sketch word idx & 4 095   srn_kernels.h:77-79, srn_fast.hip:113-114
Stage loads: every kept value is placed as run 0 of a whole list and as the last of four runs under a cut; the other two combinations (last of four, whole list; run 0
under a cut) for kept <= 1 025 only -- above that each costs a cell of 1 500..5 100 sessions, 53 000 in all, which the budget of about 250 000 sessions does not have.
NOT reachable by any query, so not placed: sumw = 63 / 64 at MID (a session of <= 10 items sums to <= 55) and sumw = 255 / 256 at LONG (<= 210 at 20 items)."""
import functools

import numpy as np

from record_cases import LONG_RES_WORDS, MW_BIG, MW_LEAN, route_of

F_K_MAX, F_M_MAX = 1536, 2560
M_INDEX = F_M_MAX
SHAPES = ((500, 1100), (F_K_MAX, F_M_MAX))
MAX_LEN = 21                      # the longest session of the batch (the L = 21 cell): what a host call passes as max_len
ROW_MAX = 34
LOAD = 512                        # entries per stage load
N_LEAN = (MW_LEAN - 8) // 2       # 6 012: the largest n of the lean form
N_MID = (MW_LEAN - 8 - 256) // 2  # 5 884: ... of the MID form
N_BIG = (MW_BIG - 8 - 256) // 2   # 9 404: ... of the BIG forms
N_LONG = (MW_BIG - 8 - LONG_RES_WORDS) // 2   # 7 548: ... of the LONG form
N_FUSED = 6 * 512                 # 3 072: the largest n of the fused cut
F_FIN_ENTRIES, FIN_LANES, F_REP_ITEMS, F_DIRECT, F_SK_WORDS = 63, 31, 16, 3968, 4096
STAGE_KEPT = tuple(sorted({1, 2, F_M_MAX - 1, F_M_MAX} | {j * LOAD + d for j in range(1, 5) for d in (-1, 0, 1)}))
SEARCH_KEPT, SEARCH_BELOW = (0, 1, 7, 8, 9, 10), (1, 8, 9, 64)
ROW_E = (20, 21, 22, 31, 32, 33, 63, 64, 65)
ROW_LENGTHS = (29, 30, 31, 32, 33, 34, 30, 31, 34, 2, 3, 1)
N_PAYLOAD = 8500
N_HOT, N_HOT_ROW, HOT_RATIO = 256, 3, 30.0
F_CAND_CAP, F_SURV_CAP, F_HIT_CAP, F_TABLE_SLOTS = 160, 256, 2047, 508   # srn_kernels.h:63, :67 (F_HOT_WORDS / 2 - 1), :59 (4 * F_TABLE_BUCKETS); srn_fast.hip:474
T0 = 1000
ID0, ID_STEP, UNKNOWN0 = 10**9, 7, 5 * 10**12


def cell(name, shape, L, pos, lists, shared=0, touch=(), fill="unknown", payload=None):
    """shape: which of SHAPES the cell is designed for; L: the session's length; pos: the known items' positions, 0 = most recent; lists: (count, kept) per known item at
    the designed m; fill: what stands at the other positions -- 'unknown' ids or 'repeat' (an older copy of the most recent known item; unknown where there is none);
    payload: explicit payload (catalogue numbers) of the cell's most recent sessions, most recent first."""
    assert len(pos) == len(lists) and list(pos) == sorted(set(pos)) and max(pos) < L
    return dict(name=name, shape=shape, L=L, pos=tuple(pos), lists=[tuple(x) for x in lists], shared=shared, touch=tuple(touch), fill=fill, payload=payload)


def cells():
    out = []
    (k1, m1), (k2, m2) = SHAPES
    # ---- stage loads: every kept value as run 0 with the whole list kept and as the last of four runs under a cut; the values up to 1 025 also the other way round ----
    for v in STAGE_KEPT:
        sh = 0 if v + 9 < m1 else 1
        m = SHAPES[sh][1]
        out.append(cell("load run0 whole kept=%d" % v, 1, 1, (0,), [(v, v)]))
        if v < m2:
            out.append(cell("load run3 cut kept=%d" % v, sh, 4, (0, 1, 2, 3), [(m, m), (5, 3), (7, 4), (v + 9, v)]))
        else:
            out.append(cell("load run3 cut kept=%d" % v, 1, 4, (0, 1, 2, 3), [(m2, m2), (5, 3), (7, 4), (v + 9, v)], touch=(3,)))
        if v <= 2 * LOAD + 1:
            out.append(cell("load run3 whole kept=%d" % v, 1, 4, (0, 1, 2, 3), [(3, 3), (5, 5), (7, 7), (v, v)]))
            out.append(cell("load run0 cut kept=%d" % v, sh, 2, (0, 1), [(v + 9, v), (m, m)]))
    # ---- the x_lo search (m = 1 100): kept x (len - kept), three searched lists behind the pivot and one alone ----
    for kept in SEARCH_KEPT:
        out.append(cell("search kept=%d below=1,8,9" % kept, 0, 4, (0, 1, 2, 3), [(m1, m1)] + [(kept + d, kept) for d in SEARCH_BELOW[:3]]))
        out.append(cell("search kept=%d below=64" % kept, 0, 2, (0, 1), [(kept + SEARCH_BELOW[3], kept), (m1, m1)]))
    out.append(cell("search last entry == x_lo", 0, 2, (0, 1), [(m1, m1), (20, 20)], touch=(1,)))
    for d in (-1, 0, 1, 7):
        out.append(cell("search len=m%+d (m=%d)" % (d, m1), 0, 1, (0,), [(m1 + d, min(m1 + d, m1))]))
    for d in (1, 7):
        out.append(cell("search len=m%+d (m=%d)" % (d, m2), 1, 1, (0,), [(m2 + d, m2)]))
    out.append(cell("search two lists reach m", 0, 2, (0, 1), [(m1, m1), (m1 + 200, 700)]))
    # ---- routing by n = sum of kept (m = 2 560, x_lo = 0) ----
    def split(n, parts):
        return [(n // parts + (1 if i < n % parts else 0),) * 2 for i in range(parts)]
    for n in (N_LEAN, N_LEAN + 1):
        out.append(cell("route lean/BIG n=%d" % n, 1, 3, (0, 1, 2), split(n, 3)))
    for n in (N_MID, N_MID + 1):
        out.append(cell("route MID/BIG n=%d" % n, 1, 6, (0, 1, 2, 3, 4, 5), split(n, 6)))
    for n in (N_BIG, N_BIG + 1):
        out.append(cell("route BIG/general n=%d" % n, 1, 4, (0, 1, 2, 3), split(n, 4)))
    for n in (N_LONG, N_LONG + 1):
        out.append(cell("route LONG/general n=%d" % n, 1, 12, tuple(range(12)), split(n, 12)))
    # ---- fused and two-pass cut ----
    for runs in (2, 3, 4):
        for n in (N_FUSED - 1, N_FUSED, N_FUSED + 1):
            out.append(cell("cut site n=%d runs=%d" % (n, runs), 1, runs, tuple(range(runs)), split(n, runs)))
    # ---- routing by numerators, runs and session length ----
    out.append(cell("sumw=15", 0, 6, (0, 1, 2), [(300, 300), (200, 200), (100, 100)]))
    out.append(cell("sumw=16", 0, 6, (0, 1, 2, 5), [(300, 300), (200, 200), (100, 100), (50, 50)]))
    out.append(cell("nr=4", 0, 5, (0, 1, 2, 3), [(300, 300), (200, 200), (100, 100), (50, 50)]))
    out.append(cell("nr=5", 0, 5, (0, 1, 2, 3, 4), [(300, 300), (200, 200), (100, 100), (50, 50), (25, 25)]))
    for L in (8, 9, 10, 11, 20, 21):
        out.append(cell("L=%d" % L, 0, L, (0, 1), [(300, 300), (400, 400)], fill="repeat" if L in (9, 11, 21) else "unknown"))
    # ---- the m-cut inside the kernel: no list reaches m ----
    for d in (-1, 0, 1):
        out.append(cell("m-cut C=m%+d disjoint" % d, 0, 2, (0, 1), [(600, 600), (m1 - 600 + d, m1 - 600 + d)]))
        out.append(cell("m-cut C=m%+d shared" % d, 0, 2, (0, 1), [(700, 700), (m1 - 700 + d + 199, m1 - 700 + d + 199)], shared=199))
    out.append(cell("m-cut C=m+1 disjoint (m=%d)" % m2, 1, 2, (0, 1), [(1300, 1300), (m2 - 1300 + 1, m2 - 1300 + 1)]))
    # ---- the k-cut, at both shapes ----
    for sh, (k, m) in enumerate(SHAPES):
        for d in (-1, 0, 1):
            out.append(cell("k-cut C=k%+d (k=%d)" % (d, k), sh, 2, (0, 1), [(300, 300), (k - 300 + d, k - 300 + d)]))
        out.append(cell("k-cut adjacent classes (k=%d)" % k, sh, 2, (0, 1), [(k, k), (200, 200)]))
        out.append(cell("k-cut one class (k=%d)" % k, sh, 1, (0,), [(k + 203, k + 203)]))
        for c, take in ((1, 1), (64, 32), (65, 33)):
            out.append(cell("k-cut boundary class of %d (k=%d)" % (c, k), sh, 3, (0, 1, 2), [(k - take, k - take), (c, c), (100, 100)]))
    # ---- row sizes at the hand-off: three neighbours whose rows hold exactly E distinct items besides the current one ----
    for i, E in enumerate(ROW_E):
        per = [list(range(j, E, 3)) for j in range(3)]
        out.append(cell("rows E=%d" % E, 0, 1, (0,), [(3, 3)], payload=[[1000 * i + 17 + 5 * x for x in p] for p in per]))
    # ---- rows of exactly 30, 31 and 34 items (the packed rows' overflow blocks) ----
    out.append(cell("row lengths", 0, 1, (0,), [(len(ROW_LENGTHS), len(ROW_LENGTHS))], payload=[[3000 + 3 * x + j % 3 for x in range(n - 1)] for j, n in enumerate(ROW_LENGTHS)]))   # (rows that overlap: about 100 distinct items, inside the candidate list)
    return out


def _interleave(counts):
    """Sessions of several groups, counts[g] each, evenly interleaved -> the group of every session, oldest first."""
    g = np.concatenate([np.full(c, i, np.int64) for i, c in enumerate(counts)] + [np.zeros(0, np.int64)])
    frac = np.concatenate([(np.arange(c) + 0.5) / c for c in counts] + [np.zeros(0)])
    return g[np.lexsort((g, frac))]


def _cell_masks(c):
    """The cell's sessions, oldest first, as bit masks of its known items (bit i = the item at pos[i])."""
    m = SHAPES[c["shape"]][1]
    lists, r = c["lists"], len(c["lists"])
    pivots = [i for i, (cnt, kept) in enumerate(lists) if cnt >= m and kept == m and i not in c["touch"]]
    assert all(kept <= min(cnt, m) for cnt, kept in lists)
    assert pivots or all(cnt == kept for cnt, kept in lists), "kept < len needs a pivot list"
    above = [kept for _cnt, kept in lists]
    below = [cnt - kept for cnt, kept in lists]
    head = 0
    if pivots:
        head = 1 << pivots[0]
        above[pivots[0]] -= 1
        for t in c["touch"]:
            head |= 1 << t
            above[t] -= 1
    s = c["shared"]
    if s:
        above[0] -= s
        above[1] -= s
    assert min(above) >= 0
    masks = np.array([1 << i for i in range(r)] + [3], np.int64)
    lo = masks[_interleave(below + [0])]
    hi = masks[_interleave(above + [s])]
    return np.concatenate([lo, np.full(1 if pivots else 0, head, np.int64), hi])


class Index:
    """off / items / ts of the designed index, its queries, and what the restatement needs."""


@functools.lru_cache(maxsize=None)
def build(tied=False):
    cs = cells()
    masks, first, qitem0 = [], [], []
    n_sess = n_qi = 0
    for c in cs:
        mk = _cell_masks(c)
        first.append(n_sess)
        qitem0.append(n_qi)
        masks.append(mk)
        n_sess += len(mk)
        n_qi += len(c["lists"])
    masks = np.concatenate(masks)
    first = np.array(first + [n_sess], np.int64)
    cell_of = np.repeat(np.arange(len(cs)), np.diff(first))
    # item numbers: the cells' query items first, then the payload catalogue; id = ID0 + ID_STEP * number, so numbers order like ids
    sess, num = [], []
    for b in range(20):
        s = np.flatnonzero((masks >> b) & 1)
        sess.append(s)
        num.append(np.array(qitem0, np.int64)[cell_of[s]] + b)
    # payload: every session holds N_HOT_ROW items of a HOT set of N_HOT items whose popularity falls geometrically (first : last = 30 : 1) and one item drawn uniformly
    # from the rest of the catalogue.  The hot set gives every query of more than a handful of neighbours a clear head of scores, as real traffic has: the fast kernels'
    # back end takes its threshold from the 512 most popular items (eight waves, 64 each) and hands a query whose candidates outgrow its lists to the general kernel --
    # with the cells' own query items alone at the head of the popularity order, nothing there would be scored and large cells would fall back (backend_fits below)
    rng = np.random.default_rng(20240607)
    explicit = np.zeros(n_sess, bool)
    for ci, c in enumerate(cs):
        if c["payload"] is not None:
            for j, p in enumerate(c["payload"]):
                s = first[ci + 1] - 1 - j
                explicit[s] = True
                sess.append(np.full(len(p), s, np.int64))
                num.append(n_qi + np.array(p, np.int64))
    plain = np.flatnonzero(~explicit)
    hot_p = HOT_RATIO ** (-np.arange(N_HOT) / (N_HOT - 1.0))
    hot = rng.choice(N_HOT, size=(len(plain), N_HOT_ROW), p=hot_p / hot_p.sum())
    tail = N_HOT + (rng.random(len(plain)) * (N_PAYLOAD - N_HOT)).astype(np.int64)
    ps = np.repeat(plain, N_HOT_ROW + 1)
    pn = np.concatenate([hot, tail[:, None]], axis=1).reshape(-1)
    sess.append(ps)
    num.append(n_qi + pn)
    key = np.unique(np.concatenate(sess) * (1 << 24) + np.concatenate(num))   # rows ascending and de-duplicated
    rs, rn = key >> 24, key & ((1 << 24) - 1)
    off = np.zeros(n_sess + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(rs, minlength=n_sess))
    assert int(np.diff(off.astype(np.int64)).max()) <= ROW_MAX and int(np.diff(off.astype(np.int64)).min()) >= 1
    ix = Index()
    ix.cells, ix.first, ix.tied = cs, first, tied
    ix.off, ix.items = off, (ID0 + ID_STEP * rn).astype(np.uint64)
    idx = np.arange(n_sess)
    ix.ts = (T0 + (idx // 8 if tied else idx)).astype(np.uint32)
    # queries: the cell's session (q_shift 0); and, up to 7 items, the same with an unknown id on top (1) or with a copy of its oldest known item on top (2)
    unknown = iter(range(UNKNOWN0, UNKNOWN0 + 10**6))
    ix.queries, ix.q_cell, ix.q_shift = [], [], []
    for ci, c in enumerate(cs):
        q = [None] * c["L"]
        for i, p in enumerate(c["pos"]):
            q[c["L"] - 1 - p] = ID0 + ID_STEP * (qitem0[ci] + i)
        for p in range(c["L"]):
            if q[c["L"] - 1 - p] is None:
                newer = [i for i, pp in enumerate(c["pos"]) if pp < p]
                q[c["L"] - 1 - p] = ID0 + ID_STEP * (qitem0[ci] + newer[0]) if c["fill"] == "repeat" and newer else next(unknown)
        ix.queries.append(q)
        ix.q_cell.append(ci)
        ix.q_shift.append(0)
        if c["L"] <= 7:
            ix.queries.append(q + [next(unknown)])
            ix.q_cell.append(ci)
            ix.q_shift.append(1)
            if len(c["pos"]) >= 2:                      # ... and with its OLDEST known item once more on top: that item's list is now run 0, its older copy owns no run
                ix.queries.append(q + [q[c["L"] - 1 - c["pos"][-1]]])
                ix.q_cell.append(ci)
                ix.q_shift.append(2)
    # what the restatement reads: recency ranks, the lists of every item (sessions, most recent first), the dense order
    order = np.lexsort((idx, ix.ts))
    ix.rank = np.empty(n_sess, np.int64)
    ix.rank[order] = idx
    ix.session_of_rank = order
    by_item = np.lexsort((-ix.rank[rs], rn))
    ix.l_items, l_start = np.unique(rn[by_item], return_index=True)
    ix.l_off = np.concatenate([l_start, [len(rn)]])
    ix.l_sess = rs[by_item]
    cnt = np.diff(ix.l_off)
    pop = np.lexsort((ix.l_items, -cnt))              # session count descending, id ascending (fill_cases.popularity_order)
    ix.dense = np.empty(len(pop), np.int64)
    ix.dense[pop] = np.arange(len(pop))               # dense idx of l_items[j]
    ix.row_num = rn
    for a in (ix.off, ix.items, ix.ts):
        a.setflags(write=False)
    return ix


def _list_of(ix, item_id):
    """The sessions that hold the item, most recent first, cut to m_index (None: unknown id)."""
    numb, rem = divmod(int(item_id) - ID0, ID_STEP)
    if int(item_id) < ID0 or rem:
        return None
    j = int(np.searchsorted(ix.l_items, numb))
    if j >= len(ix.l_items) or ix.l_items[j] != numb:
        return None
    return ix.l_sess[ix.l_off[j]:ix.l_off[j + 1]][:M_INDEX]


def restate_one(ix, q, k, m):
    """Every designed quantity of one query at (k, m), from the sessions alone."""
    L = len(q)
    seen, per = [], []
    for pos in range(L):
        it = q[L - 1 - pos]
        if it in seen:
            continue
        seen.append(it)
        lst = _list_of(ix, it)
        if lst is not None and len(lst):
            per.append((pos, ix.rank[lst[:m]]))
    xlo = max([int(r[m - 1]) for _p, r in per if len(r) >= m], default=0)
    out = dict(L=L, U=len(seen), xlo=xlo, pos=[p for p, _r in per], len=[len(r) for _p, r in per], kept=[int((r >= xlo).sum()) for _p, r in per])
    out["n"] = sum(out["kept"])
    out["nr"] = sum(1 for x in out["kept"] if x > 0)
    out["sumw"] = sum(L - p for p, _r in per)
    out["P"] = sum(out["len"])
    out["rmax"] = max([int(r[0]) for _p, r in per], default=0)
    out["below_tied"] = any(bool(((r < xlo) & (ix.ts[ix.session_of_rank[r]] == ix.ts[ix.session_of_rank[xlo]])).any()) for _p, r in per)
    out["last_is_xlo"] = [bool(xlo > 0 and len(r) < m and r[-1] == xlo) for _p, r in per]
    ranks = np.concatenate([r[r >= xlo] for _p, r in per] + [np.zeros(0, np.int64)])
    w = np.concatenate([np.full(int((r >= xlo).sum()), L - p, np.int64) for p, r in per] + [np.zeros(0, np.int64)])
    cr, inv = np.unique(ranks, return_inverse=True)
    num = np.bincount(inv, weights=w, minlength=len(cr)).astype(np.int64)
    cr, num = cr[::-1][:m], num[::-1][:m]                       # the m most recent of the union
    by = np.lexsort((-cr, -num))                                # numerator descending, recency descending
    cr, num = cr[by], num[by]
    out["C"], out["K"] = len(cr), min(k, len(cr))
    out["nb"] = sorted(zip(ix.session_of_rank[cr[:k]].tolist(), num[:k].tolist()))
    out["boundary"] = None
    if len(cr) > k:
        b = int(num[k - 1])
        out["boundary"] = dict(cls=b, next=int(num[k]), size=int((num == b).sum()), taken=int((num[:k] == b).sum()),
                               tied=bool(ix.ts[ix.session_of_rank[cr[k - 1]]] == ix.ts[ix.session_of_rank[cr[k]]]))
    nbs = ix.session_of_rank[cr[:k]]
    a, b = ix.off[nbs].astype(np.int64), ix.off[nbs + 1].astype(np.int64)
    rows = ix.row_num[np.repeat(a - np.concatenate([[0], np.cumsum(b - a)[:-1]]), b - a) + np.arange(int((b - a).sum()))] if len(nbs) else np.zeros(0, np.int64)
    scored = np.unique(rows)
    cur, rem = divmod(int(q[-1]) - ID0, ID_STEP)
    out["I"], out["D"] = len(rows), len(scored)
    out["E"] = len(scored) - int(rem == 0 and cur in scored)
    out["row_lengths"] = (b - a)
    out["dense"] = ix.dense[np.searchsorted(ix.l_items, scored)]
    # acc(item) = sum over the neighbours of w10 * numerator: the first match of a neighbour is the most recent session item its row holds
    owner = np.repeat(np.arange(len(nbs)), b - a)
    first_match = np.full(len(nbs), 10**6, np.int64)
    for pos in range(L - 1, -1, -1):
        numb, rem_ = divmod(int(q[L - 1 - pos]) - ID0, ID_STEP)
        if rem_ == 0 and numb >= 0:
            first_match[owner[rows == numb]] = pos + 1
    w10 = np.where(first_match < 100, 10 - first_match, 0)
    at = np.searchsorted(scored, rows)
    out["acc"] = np.bincount(at, weights=(w10 * num[:k])[owner], minlength=len(scored)).astype(np.int64)
    out["occ"] = np.bincount(at, minlength=len(scored))
    out["scored"] = scored
    out["cur"] = cur if rem == 0 else -1
    nr_rec = out["nr"] if 1 <= L <= MAX_LEN else 0
    out["route"] = route_of(L, out["n"], out["sumw"], out["rmax"] - xlo, nr_rec, 0, MAX_LEN)
    return out


@functools.lru_cache(maxsize=None)
def restate(tied, shape):
    ix = build(tied)
    k, m = SHAPES[shape]
    return [restate_one(ix, q, k, m) for q in ix.queries]


def census(tied=False):
    """-> {edge: number of (query, shape) pairs on it}; every edge of the module's docstring, both sides.  Raises AssertionError naming the edges nobody hits, and checks
    that every cell's designed (len, kept) are what its own query has at its own shape."""
    ix = build(tied)
    R = [restate(tied, 0), restate(tied, 1)]
    every = [(sh, qi, r) for sh in (0, 1) for qi, r in enumerate(R[sh])]
    hits = {}

    def edge(name, pred):
        hits[name] = sum(1 for sh, qi, r in every if pred(sh, qi, r))
    # the design holds: a cell's own query, at the shape it was designed for
    for qi, ci in enumerate(ix.q_cell):
        c = ix.cells[ci]
        r = R[c["shape"]][qi]
        m = SHAPES[c["shape"]][1]
        if ix.q_shift[qi] == 2:   # (the oldest known item leads: the same lists in another order)
            assert sorted(zip(r["len"], r["kept"])) == sorted((min(cnt, m), kept) for cnt, kept in c["lists"]) and r["pos"][0] == 0, c["name"]
            continue
        assert r["len"] == [min(cnt, m) for cnt, _kept in c["lists"]] and r["kept"] == [kept for _cnt, kept in c["lists"]], (c["name"], r["len"], r["kept"])
        assert r["pos"] == [p + ix.q_shift[qi] for p in c["pos"]] and r["L"] == c["L"] + ix.q_shift[qi], c["name"]
    lean = lambda r: r["route"] == "lean"   # noqa: E731
    for v in STAGE_KEPT:
        edge("load: kept %d is run 0, whole list" % v, lambda sh, qi, r, v=v: lean(r) and r["kept"][:1] == [v] and r["len"][0] == v)
        edge("load: kept %d is the last of four runs, under a cut" % v, lambda sh, qi, r, v=v: lean(r) and r["nr"] == 4 and r["kept"][-1] == v and r["xlo"] > 0 and
             (r["len"][-1] > v or v == SHAPES[sh][1]))
    for v in STAGE_KEPT:
        if v <= 2 * LOAD + 1:   # (the other two combinations are placed up to 1 025 only: see the module's docstring)
            edge("load: kept %d is the last of four runs, whole list" % v, lambda sh, qi, r, v=v: lean(r) and r["nr"] == 4 and r["kept"][-1] == v and r["len"][-1] == v and r["xlo"] == 0)
            edge("load: kept %d is run 0, under a cut" % v, lambda sh, qi, r, v=v: lean(r) and r["kept"][:1] == [v] and r["len"][0] > v and r["xlo"] > 0)
    for kept in SEARCH_KEPT:
        for d in SEARCH_BELOW:
            edge("search: kept %d of %d" % (kept, kept + d), lambda sh, qi, r, kept=kept, d=d: any(a == kept and b == kept + d for a, b in zip(r["kept"], r["len"])))
    edge("search: a list with nothing at or above x_lo owns no run", lambda sh, qi, r: lean(r) and 0 in r["kept"])
    edge("search: last entry == x_lo", lambda sh, qi, r: any(r["last_is_xlo"]))
    for sh_, (k, m) in enumerate(SHAPES):
        for d in (-1, 0):
            edge("search: len = m%+d, no cut (m=%d)" % (d, m), lambda sh, qi, r, sh_=sh_, m=m, d=d: sh == sh_ and r["len"] == [m + d] and r["kept"] == [m + d] and (r["xlo"] > 0) == (d == 0))
    for sh_, (k, m) in enumerate(SHAPES):
        for d in (1, 7):
            edge("search: %d sessions hold the item, cut to m = %d" % (m + d, m), lambda sh, qi, r, sh_=sh_, m=m, d=d: sh == sh_ and ix.cells[ix.q_cell[qi]]["lists"] == [(m + d, m)] and r["len"] == [m] and r["kept"] == [m])
    edge("search: two lists reach m, x_lo the larger m-th rank", lambda sh, qi, r: sum(1 for x in r["len"] if x >= SHAPES[sh][1]) >= 2 and min(r["kept"]) < SHAPES[sh][1])
    for name, a, b, n in (("lean", "lean", "big", N_LEAN), ("MID", "mid", "mid>big", N_MID), ("BIG", "big", "mid>general", N_BIG), ("LONG", "long", "long>general", N_LONG)):
        edge("route: %s at n = %d" % (name, n), lambda sh, qi, r, a=a, n=n: r["route"] == a and r["n"] == n)
        edge("route: past %s at n = %d" % (name, n + 1), lambda sh, qi, r, b=b, n=n: r["route"] == b and r["n"] == n + 1)
    for runs in (2, 3, 4):
        for n in (N_FUSED - 1, N_FUSED, N_FUSED + 1):
            for sh_ in ((0, 1) if runs > 2 else (1,)):   # (two lists of <= 1 100 entries stay under 3 072)
                edge("cut site: n = %d, %d runs, k = %d" % (n, runs, SHAPES[sh_][0]), lambda sh, qi, r, sh_=sh_, n=n, runs=runs: sh == sh_ and lean(r) and r["n"] == n and r["nr"] == runs and r["C"] > SHAPES[sh][0])
    edge("numerators: sumw = 15 is lean", lambda sh, qi, r: lean(r) and r["sumw"] == 15 and r["nr"] <= 4)
    edge("numerators: sumw = 16 is MID", lambda sh, qi, r: r["route"] == "mid" and r["sumw"] == 16 and r["nr"] <= 4 and r["L"] <= 8)
    edge("runs: nr = 4 is lean", lambda sh, qi, r: lean(r) and r["nr"] == 4)
    edge("runs: nr = 5 is MID", lambda sh, qi, r: r["route"] == "mid" and r["nr"] == 5 and r["sumw"] <= 15 and r["L"] <= 8)
    for L, route in ((8, "lean"), (9, "mid"), (10, "mid"), (11, "long"), (20, "long"), (21, "general")):
        edge("length: L = %d is %s" % (L, route), lambda sh, qi, r, L=L, route=route: r["L"] == L and r["route"] == route and r["nr"] == 2)
    for d in (-1, 0, 1):
        edge("m-cut: x_lo = 0, C = m%+d = n" % d, lambda sh, qi, r, d=d: r["xlo"] == 0 and r["n"] == SHAPES[sh][1] + d and r["C"] == min(r["n"], SHAPES[sh][1]))
        edge("m-cut: x_lo = 0, distinct = m%+d < n" % d, lambda sh, qi, r, d=d: r["xlo"] == 0 and r["n"] > SHAPES[sh][1] + 1 and _distinct(ix, sh, qi) == SHAPES[sh][1] + d)
    for sh_, (k, m) in enumerate(SHAPES):
        for d in (-1, 0, 1):
            edge("k-cut: C = k%+d (k=%d)" % (d, k), lambda sh, qi, r, sh_=sh_, d=d: sh == sh_ and r["C"] == SHAPES[sh][0] + d)
        edge("k-cut: C = m, far beyond k (k=%d)" % k, lambda sh, qi, r, sh_=sh_: sh == sh_ and r["C"] == SHAPES[sh][1] and r["n"] > r["C"])
        edge("k-cut: k-th and (k+1)-th in one class (k=%d)" % k, lambda sh, qi, r, sh_=sh_: sh == sh_ and r["boundary"] is not None and r["boundary"]["cls"] == r["boundary"]["next"])
        edge("k-cut: k-th and (k+1)-th in adjacent classes (k=%d)" % k, lambda sh, qi, r, sh_=sh_: sh == sh_ and r["boundary"] is not None and r["boundary"]["cls"] == r["boundary"]["next"] + 1)
        for c in (1, 64, 65):
            edge("k-cut: boundary class of %d (k=%d)" % (c, k), lambda sh, qi, r, sh_=sh_, c=c: sh == sh_ and r["boundary"] is not None and r["boundary"]["size"] == c and
                 (c == 1 or 0 < r["boundary"]["taken"] < c))
        for site, pred in (("fused", lambda n: n <= N_FUSED), ("two-pass", lambda n: n > N_FUSED)):
            edge("k-cut: bites at the %s site (k=%d)" % (site, k), lambda sh, qi, r, sh_=sh_, pred=pred: sh == sh_ and lean(r) and r["boundary"] is not None and pred(r["n"]))
    for E in ROW_E:
        edge("rows: E = %d" % E, lambda sh, qi, r, E=E: r["E"] == E and r["K"] == 3)
    for n in (30, 31, 34):
        edge("rows: a neighbour's row of %d items" % n, lambda sh, qi, r, n=n: lean(r) and bool((r["row_lengths"] == n).any()))
    for d in (F_REP_ITEMS - 1, F_REP_ITEMS, LOAD - 1, LOAD, F_DIRECT - 1, F_DIRECT):
        edge("accumulators: dense idx %d scored by a fast form" % d, lambda sh, qi, r, d=d: r["route"] in ("lean", "mid", "big", "mid>big", "long") and bool((r["dense"] == d).any()))
    edge("accumulators: two scored items share a sketch word", lambda sh, qi, r: r["route"] in ("lean", "mid", "big", "mid>big", "long") and _shares_sketch_word(r["dense"]))
    if tied:
        edge("tied: a tie group straddles x_lo", lambda sh, qi, r: r["xlo"] > 0 and r["below_tied"])
        edge("tied: a tie group straddles the k-cut's boundary", lambda sh, qi, r: r["boundary"] is not None and r["boundary"]["cls"] == r["boundary"]["next"] and r["boundary"]["tied"])
    # no query that the front end keeps on a fast form outgrows the back end's lists: the rows the GPU test compares are the fast kernels' own (it asserts the count)
    attrs = business_attrs(ix)
    for sh, qi, r in every:
        if r["route"] in FAST_ROUTES:
            for how_many, at in ((21, None), (64, None), (21, attrs)):
                why = backend_fits(ix, r, how_many, at)
                assert why is None, (ix.cells[ix.q_cell[qi]]["name"], SHAPES[sh], how_many, at is not None, why)
    missing = [name for name, c in hits.items() if c == 0]
    assert not missing, "edges that no query of the designed index hits: %s" % missing
    return hits


def _distinct(ix, sh, qi):
    """Distinct sessions of the query's lists (before the m-cut)."""
    q, m = ix.queries[qi], SHAPES[sh][1]
    s = [ix.rank[_list_of(ix, it)[:m]] for it in dict.fromkeys(q) if _list_of(ix, it) is not None]
    return len(np.unique(np.concatenate(s))) if s else 0


def backend_fits(ix, r, how_many, attrs=None):
    """A CONSERVATIVE statement of whether the fast kernels' back end (srn_fast.hip, phase 4) keeps the query: the candidate list (F_CAND_CAP), the floor survivors, walk B's
    hit list (F_HIT_CAP) and the exact table.  The threshold: the 512 most popular items, item e with wave e % 8; every wave's j-th largest x = idf * acc, j = max(3,
    ceil(how_many / 8)); the smallest of the eight (none if a wave has fewer: then every scored item is a candidate).  Conservative: the first, loose threshold with 1 % of
    slack stands for the second as well, and floors and live sketch words are taken with the LARGEST idf of the index.  attrs = {item number: byte}:
    business rules (an item that is not for sale, or adult under a current item that is not, is no candidate and sets no threshold).  -> None, or what overflows."""
    acc, dense, scored = r["acc"], r["dense"], r["scored"]
    cnt = np.diff(ix.l_off)[np.searchsorted(ix.l_items, scored)]
    idf = np.log(float(len(ix.row_num)) / cnt)
    idf_hi = float(np.log(float(len(ix.row_num)) / np.diff(ix.l_off).min()))
    valid = (acc > 0) & (scored != r["cur"])
    if attrs is not None:
        fl = np.array([attrs.get(int(x), 0xFF) for x in scored])
        cur_fl = attrs.get(r["cur"], 0xFF)
        cur_adult = cur_fl != 0xFF and bool(cur_fl & 1)
        valid &= (fl != 0xFF) & ((fl & 2) != 0) & (((fl & 1) == 0) | cur_adult)
    x = idf * acc
    j = max(3, (how_many + 7) // 8)
    t = np.inf
    for wv in range(8):
        xs = np.sort(x[valid & (dense < 512) & (dense % 8 == wv)])[::-1]
        t = min(t, xs[j - 1] if len(xs) >= j else 0.0)
    if t == 0 and int(valid.sum()) < how_many and (r["route"].startswith("long") or (r["route"].startswith("mid") and r["L"] == 10)):
        return "fewer positive scores than how_many where neighbours of weight 0 may exist (srn_fast.hip:1495)"
    cand = valid & (x >= 0.99 * t)                                                       # (the second, tighter threshold can only drop some of these)
    surv = valid & (dense >= 512) & (dense < F_DIRECT) & (idf_hi * acc >= 0.99 * t)      # (a chunk's floor comes from ITS largest idf: at most the index's)
    if int(cand.sum()) > F_CAND_CAP or int(surv.sum()) > F_SURV_CAP:
        return "%d candidates, %d floor survivors" % (int(cand.sum()), int(surv.sum()))
    sk = dense >= F_DIRECT
    word = dense[sk] & (F_SK_WORDS - 1)
    sums = np.bincount(word, weights=np.maximum(acc[sk], 0), minlength=F_SK_WORDS)
    live = sums[word] * idf_hi >= 0.99 * t if t > 0 else np.ones(len(word), bool)
    if int(r["occ"][sk][live].sum()) > F_HIT_CAP or int(live.sum()) > F_TABLE_SLOTS:
        return "walk B: %d hits, %d items" % (int(r["occ"][sk][live].sum()), int(live.sum()))
    return None


FAST_ROUTES = ("lean", "big", "mid", "mid>big", "long")


def _shares_sketch_word(dense):
    d = dense[dense >= F_DIRECT]
    return bool(len(d)) and len(np.unique(d & (F_SK_WORDS - 1))) < len(d)


def business_attrs(ix):
    """The attribute bytes the GPU test sets (fill_cases.draw_attrs over the index's items) -> {item number: byte}."""
    from fill_cases import draw_attrs
    known, flags = draw_attrs(ix.items)
    return dict(zip(((known.astype(np.int64) - ID0) // ID_STEP).tolist(), flags.tolist()))


def route_counts(tied, shape):
    """How many queries of the batch the restatement sends where."""
    out = {}
    for r in restate(tied, shape):
        out[r["route"]] = out.get(r["route"], 0) + 1
    return out


# ---- full-width ids (test_gpu_persistent_edges.py, test_edge_cases_host.py) -------------------------------------------------------------------------------------------
# The designed ids stay below 2^43 (ID0 + ID_STEP * number, UNKNOWN0 + j).  wide_ids is a strictly increasing injection into 64 bits: the id itself in bits 20..62 and 20
# mixed bits below it, so that both 32-bit halves are non-zero, the halves differ, and hi ^ lo differs between neighbours (ids 7 apart share their high half: the low half
# alone tells them apart, and a lost or swapped half names another item or none).  Strictly increasing, so the canonical order (score descending, id ascending) of the
# mapped index is the map of the narrow index's: the expected rows are the oracle's with the map applied to the ids, the scores the same bits (asserted on the CPU).
WIDE_SHIFT = 20


def _mix64(x):
    """The splitmix64 finaliser on a uint64 array."""
    x = x.astype(np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def wide_ids(ids):
    """u64 array of the mapped ids (0 stays 0: the unused tail of a row)."""
    a = np.asarray(ids, dtype=np.uint64)
    assert a.size == 0 or int(a.max()) < (1 << (63 - WIDE_SHIFT))
    out = (a << np.uint64(WIDE_SHIFT)) | (_mix64(a) & np.uint64((1 << WIDE_SHIFT) - 1))
    return np.where(a == 0, np.uint64(0), out)


def designed_ids(ix):
    """Every id the index or a query of the batch holds, ascending."""
    return np.unique(np.concatenate([ix.items, np.array([x for q in ix.queries for x in q], np.uint64), serve_extra_ids()]))


# ---- the persistent latency path in the restatement's terms (srn_latency.hip: device_serve_predict; srn_fast.hip: the serving loop of vmis_fast_kernel<TINY>) ----------
# A session of 1..4 items goes to the resident lean form, one of 5..max_items (<= 10) to the resident form for 5..10 items; neither has a tier behind it.  The workgroup
# answers status 0 iff a finishing path wrote the row's count over its sentinel:
#   (1) the form's own `fits`: lean   L <= 4, sumw <= 15, nr <= 4, 2 n + 8 <= 12 032
#                              5..10  sumw <= 63, nr <= 10, 2 n + 8 + 256 <= 12 032        (what the launch sequence would list for BIG or hand over is NOT served),
#   (2) no known item (n = 0): the count 0 is written at once -- served;
#   (3) the back end keeps the query (backend_fits: asserted by the census for every fast route), and wave 0 finishes the row from its registers: M <= 63 entries, or
#       M > 63 and, of the M keys' top 32 bits, at most 64 lie at or above ONE STEP BELOW the how_many-th largest (srn_fast.hip: `if (S <= 64u && S >= p.how_many)`).
# M itself depends on the sample's thresholds, but every entry set the back end can arrive at holds ALL valid items down to one step below the how_many-th best (that is
# what its thresholds guarantee), so with  T = |{valid items: hi32(idf_eff * acc) >= (how_many-th largest hi32) - 1}|  (all valid items where there are fewer than
# how_many): M <= 63 implies T <= 63, and M > 63 gives S = T.  Served iff T <= 64.  Valid: acc > 0, not the current item, and under the business rules what they let
# through.  A row of E <= 63 scored items has T <= 63 whatever the scores are; rows of 64 and of 65 items are served or not by their ties at the cut (tight_set).
SERVE_MAX_ENTRIES = 64


def tight_set(ix, r, how_many, attrs=None):
    """T of the comment above, from the restatement's accumulators and idf = ln(interactions / sessions that hold the item), the index's own formula in the same libm."""
    import math
    acc, scored = r["acc"], r["scored"]
    cnt = np.diff(ix.l_off)[np.searchsorted(ix.l_items, scored)]
    total = float(len(ix.row_num))
    idf = np.array([math.log(total / float(c)) for c in cnt], np.float64)
    idf = np.where(idf > 0.0, idf, 1.0)
    valid = (acc > 0) & (scored != r["cur"])
    if attrs is not None:
        fl = np.array([attrs.get(int(x), 0xFF) for x in scored], np.int64)
        cur_fl = attrs.get(r["cur"], 0xFF)
        cur_adult = cur_fl != 0xFF and bool(cur_fl & 1)
        valid &= (fl != 0xFF) & ((fl & 2) != 0) & (((fl & 1) == 0) | cur_adult)
    hi = ((idf * acc.astype(np.float64)).view(np.uint64) >> np.uint64(32)).astype(np.int64)[valid]
    if len(hi) < how_many:
        return len(hi)
    cut = int(np.sort(hi)[::-1][how_many - 1]) - 1
    return int((hi >= cut).sum())


def resident_route(r, max_items=10):
    """What the resident form that gets the session does with it at the front end: 'none' (not posted: length outside 1..max_items), 'lean' / 'mid' (its own), 'big' (the
    lean form's oversized query: the launch sequence's BIG list, nobody's here), 'general' (every other hand-over)."""
    L = r["L"]
    if not 1 <= L <= max_items:
        return "none"
    span = r["rmax"] - r["xlo"]
    if L <= 4:
        route = route_of(L, r["n"], r["sumw"], span, r["nr"], 0, 8)
        return route if route in ("lean", "big") else "general"
    nb = max(r["nr"], 4)
    return "mid" if r["sumw"] <= 63 and r["nr"] <= 10 and span < (1 << (32 - nb)) and 2 * r["n"] + 8 + 256 <= MW_LEAN else "general"


def resident_kind(ix, r, how_many=21, attrs=None, max_items=10):
    """'served' or why not: 'none', 'big', 'general', 'over64' (T > 64: the row is left to a finish kernel nobody launches)."""
    route = resident_route(r, max_items)
    if route not in ("lean", "mid"):
        return route
    return "served" if r["n"] == 0 or tight_set(ix, r, how_many, attrs) <= SERVE_MAX_ENTRIES else "over64"


def serve_extra_ids():
    return np.array([UNKNOWN0 + 2 * 10**6 + j for j in range(3)], np.uint64)


def serve_extras():
    """Sessions outside the batch that the persistent tests post as well: no known item at all -- the row of count 0, which the workgroup writes at once (both forms)."""
    u = [int(x) for x in serve_extra_ids()]
    return [("no known item, L=1", [u[0]]), ("no known item, L=2", [u[1], u[0]]), ("no known item, L=6", [u[0], u[1], u[2], u[0], u[1], u[2]])]


@functools.lru_cache(maxsize=None)
def serve_calls(tied, shape, max_items=10):
    """The single calls of the persistent tests at one shape, in cell order: every query of the batch of at most max_items items and no q_shift (the selection of
    test_gpu_edge_cases.py (d)), then serve_extras.  -> [dict(name, q, qi (None for an extra), r = the restatement)]."""
    ix = build(tied)
    k, m = SHAPES[shape]
    R = restate(tied, shape)
    out = [dict(name=ix.cells[ix.q_cell[qi]]["name"], q=list(q), qi=qi, r=R[qi]) for qi, q in enumerate(ix.queries) if not ix.q_shift[qi] and len(q) <= max_items]
    return out + [dict(name=name, q=q, qi=None, r=restate_one(ix, q, k, m)) for name, q in serve_extras()]


def serve_weight(c):
    """How much a call leaves behind in a workgroup: (staged entries, scored items, hot-head accumulators in use)."""
    r = c["r"]
    return (r["n"], r["E"], int((r["dense"] < N_HOT).sum()) if len(r["dense"]) else 0)


def serve_orders(tied, shape, how_many=21, attrs=None):
    """-> {'cells': ..., 'reversed': ..., 'interleave': ...}: index lists into serve_calls.  The interleave, per resident form (a workgroup keeps only ITS form's state):
    the served calls sorted by weight, dealt heaviest, lightest, second heaviest, second lightest, ...; then every call the form does not finish itself, each with a served
    call directly behind it (the light half first: a light row behind a handed-over heavy one is where left-over state would show)."""
    ix = build(tied)
    calls = serve_calls(tied, shape)
    kinds = [resident_kind(ix, c["r"], how_many, attrs) for c in calls]
    inter = []
    for form in (0, 1):
        mine = [i for i, c in enumerate(calls) if (c["r"]["L"] > 4) == bool(form)]
        served = sorted((i for i in mine if kinds[i] == "served"), key=lambda i: (serve_weight(calls[i]), i))
        rest = [i for i in mine if kinds[i] != "served"]
        a, b = 0, len(served) - 1
        while a <= b:
            inter.append(served[b])
            if a < b:
                inter.append(served[a])
            a, b = a + 1, b - 1
        for j, i in enumerate(rest):
            inter += [i, served[j % len(served)]]
    n = len(calls)
    return dict(cells=list(range(n)), reversed=list(range(n - 1, -1, -1)), interleave=inter), kinds
