"""A DESIGNED index and query list for the light form (srn_light.hip; test_light_cases_host.py, test_gpu_light_form.py), in the style of edge_cases.py: every query's list
lengths, row lengths and scored items are chosen, not drawn.  NumPy only, deterministic, no GPU.  Test-side only.

A query is LIGHT when its prep record says lean_ok (here: always, the sessions have <= 4 items and the lists are short), it has ONE posting run and that run keeps at most
64 entries.  The light form serves it with one wave: the rows' items into an exact table of 251 buckets of 4 slots, the current item dropped, <= 64 scored items ranked
at once, more cut to the how_many best and their ties first; a full table, or more than 64 entries at the cut, sends the query to the general kernel.

Sessions ascend in time (timestamp = T0 + session index), so a session's recency rank is its index.  A TAIL item t with n sessions has a list of n entries; each of its
sessions holds t, PAY_HOT items of a small hot pool (geometric popularity: scores with a clear head) and one item that no other session holds.

The cases (name -> query), and what each claims:
  kept=1, 2, 63, 64, 65       one-item sessions; 64 is admitted, 65 is not
  [unknown, a], [a, unknown]  one run at position 0 / 1 of a two-item session; [a, a]: the older copy owns no run
  two short lists             two runs: not admitted
  rows of 15, 16, 34 items    the row slot's three layouts (items in words 1..15 | 14 in the slot + row_ext), 62 scored items, all tied
  table overflow              64 rows of 34 items, 2 113 distinct: the table cannot hold them -> the general kernel
  ties at the cut             3 rows of 31 items, 90 scored items with one and the same score: more than 64 entries at the cut -> the general kernel
  unknown only                no run at all: not admitted (the lean chain writes the empty row)
  heavy                       items with 200 sessions: the lean chain's
and N_TAIL drawn tail items (1..64 sessions) with their one-item, [unknown, a] and [a, unknown] sessions, some of them several times over (merging)."""
import functools
import math

import numpy as np

K, M, M_INDEX, MAX_LEN, ROW_MAX = 100, 500, 500, 4, 34
KEPT_MAX, TABLE_SLOTS, RANK_MAX = 64, 251 * 4, 64   # srn_kernels.h RW_LIGHT_KEPT; srn_light.hip LT_BUCKETS * 4; finish_inline's lanes
T0, ID0, ID_STEP, UNKNOWN0 = 1000, 10**9, 7, 5 * 10**12
N_HOT, PAY_HOT, HOT_RATIO = 96, 3, 4.0
N_TAIL, N_HEAVY, HEAVY_SESSIONS = 160, 6, 200


class Cases:
    pass


@functools.lru_cache(maxsize=None)
def build():
    rng = np.random.default_rng(20241021)
    counter = [0]

    def new(n=1):
        a = list(range(counter[0], counter[0] + n))
        counter[0] += n
        return a if n > 1 else a[0]
    hot = new(N_HOT)
    hot_p = HOT_RATIO ** (-np.arange(N_HOT) / (N_HOT - 1.0))
    hot_p /= hot_p.sum()
    sessions = []

    def tail_item(n, rows=None, fresh=True):
        """An item with n sessions -> its number.  rows: explicit row lengths (items besides the tail item are fresh), else the hot payload + one fresh item (fresh=False:
        one more hot item instead -- the heavy items' rows score the hot pool alone, so the lean chain's candidate list never outgrows its room)."""
        t = new()
        for j in range(n):
            if rows is not None:
                sessions.append([t] + (new(rows[j] - 1) if rows[j] > 2 else [new()] * (rows[j] - 1)))
            else:
                sessions.append([t] + [hot[i] for i in rng.choice(N_HOT, PAY_HOT + (0 if fresh else 1), replace=False, p=hot_p)] + ([new()] if fresh else []))
        return t
    unknown = iter(range(UNKNOWN0, UNKNOWN0 + 10**6))
    ident = lambda num: ID0 + ID_STEP * num   # noqa: E731
    named = []   # (name, query as ids)
    for n in (1, 2, 63, 64, 65):
        named.append(("kept=%d" % n, [ident(tail_item(n))]))
    a = tail_item(5)
    named += [("[unknown, a]", [next(unknown), ident(a)]), ("[a, unknown]", [ident(a), next(unknown)]), ("[a, a]", [ident(a), ident(a)]),
              ("[unknown, unknown, a, unknown]", [next(unknown), next(unknown), ident(a), next(unknown)])]
    named.append(("two short lists", [ident(tail_item(3)), ident(tail_item(4))]))
    named.append(("rows of 15, 16, 34 items", [ident(tail_item(3, rows=[15, 16, 34]))]))
    named.append(("table overflow", [ident(tail_item(64, rows=[34] * 64))]))
    named.append(("ties at the cut", [ident(tail_item(3, rows=[31, 31, 31]))]))
    named.append(("unknown only", [next(unknown)]))
    heavy = [tail_item(HEAVY_SESSIONS, fresh=False) for _ in range(N_HEAVY)]
    for i, h in enumerate(heavy):
        named.append(("heavy %d" % i, [ident(h)]))
        named.append(("heavy %d + tail" % i, [ident(a), ident(h)]))
    tails = [tail_item(int(n)) for n in rng.integers(1, KEPT_MAX + 1, N_TAIL)]
    for i, t in enumerate(tails):
        named.append(("tail %d" % i, [ident(t)]))
        if i % 3 == 0:
            named.append(("tail %d under an unknown id" % i, [ident(t), next(unknown)]))
        if i % 5 == 0:
            named.append(("tail %d over an unknown id" % i, [next(unknown), ident(t)]))
    # equal queries several times over: every seventh query twice more, the designed cases once more
    extra = [named[i] for i in range(0, len(named), 7)] * 2 + named[:14]
    order = rng.permutation(len(named) + len(extra))
    allq = named + [(nm + " (again)", q) for nm, q in extra]
    c = Cases()
    c.names, c.queries = [allq[i][0] for i in order], [list(allq[i][1]) for i in order]
    rows = [sorted(set(s)) for s in sessions]
    assert max(len(r) for r in rows) <= ROW_MAX
    c.off = np.zeros(len(rows) + 1, np.uint64)
    c.off[1:] = np.cumsum([len(r) for r in rows])
    c.items = np.array([ident(x) for r in rows for x in r], np.uint64)
    c.ts = (T0 + np.arange(len(rows))).astype(np.uint32)
    c.rows = rows
    c.lists = {}
    for s, r in enumerate(rows):
        for x in r:
            c.lists.setdefault(ident(x), []).append(s)
    for a_ in (c.off, c.items, c.ts):
        a_.setflags(write=False)
    return c


def idf_of(c, item_id):
    """The index's idf with idf_weighting 1: ln(interactions / sessions that hold the item), <= 0 counted as 1 (edge_cases.tight_set)."""
    v = math.log(float(len(c.items)) / float(len(c.lists[item_id])))
    return v if v > 0.0 else 1.0


def predict_one(c, q, how_many=21, attrs=None, k=K, m=M):
    """What the light form does with one query -> dict(admitted, general, kept, L, ps, scored, T).  admitted: the prep record's RW_LIGHT; general: the wave hands the query
    to the general kernel (table full, or more than 64 entries at the cut).  attrs: {item id: attribute byte} under business rules, else None."""
    L = len(q)
    seen, runs = [], []
    for pos in range(L):
        it = q[L - 1 - pos]
        if it in seen:
            continue
        seen.append(it)
        lst = c.lists.get(it)
        if lst:
            runs.append((pos, lst[::-1][:m]))
    out = dict(L=L, U=len(seen), nr=len(runs), admitted=False, general=False, kept=0, scored=0, T=0)
    if len(runs) != 1 or len(runs[0][1]) > KEPT_MAX or not (1 <= L <= MAX_LEN) or k < KEPT_MAX:
        return out
    ps, lst = runs[0]
    assert len(lst) < m and sum(L - p for p, _ in runs) <= 15   # (x_lo = 0: the whole list is kept; lean_ok)
    out.update(admitted=True, kept=len(lst), ps=ps)
    w = (9 - ps) * (L - ps)
    acc = {}
    for s in lst:
        for x in c.rows[s]:
            acc[ID0 + ID_STEP * x] = acc.get(ID0 + ID_STEP * x, 0) + w
    distinct = out["distinct"] = len(acc)
    assert distinct > TABLE_SLOTS or distinct <= 0.7 * TABLE_SLOTS, "a designed query fills the exact table beyond 70 %: its probes may run out"
    cur = q[-1]
    acc.pop(cur, None)
    if attrs is not None:
        cur_fl = attrs.get(cur, 0xFF)
        cur_adult = cur_fl != 0xFF and bool(cur_fl & 1)
        acc = {x: v for x, v in acc.items() if attrs.get(x, 0xFF) != 0xFF and (attrs[x] & 2) and (not (attrs[x] & 1) or cur_adult)}
    out["scored"] = len(acc)
    if distinct > TABLE_SLOTS:   # (the table cannot hold the rows' items: the wave hands the query on before it looks at a score)
        out["general"] = True
        return out
    if len(acc) <= RANK_MAX:
        out["T"] = len(acc)
        return out
    hi = np.array([idf_of(c, x) * float(v) for x, v in acc.items()], np.float64).view(np.uint64) >> np.uint64(32)
    hi = hi.astype(np.int64)
    cut = int(np.sort(hi)[::-1][how_many - 1]) - 1
    out["T"] = int((hi >= cut).sum())
    out["general"] = out["T"] > RANK_MAX
    return out


def predict(c, queries, how_many=21, attrs=None, merge=True, k=K):
    """-> (light count, general count of the light form): over the representatives (the first of every group of equal queries) when the call merges, over all otherwise."""
    seen, light, general = set(), 0, 0
    for q in queries:
        key = tuple(q)
        if merge and key in seen:
            continue
        seen.add(key)
        r = predict_one(c, q, how_many, attrs, k)
        light += r["admitted"]
        general += r["general"]
    return light, general
