"""A DESIGNED index for the item shard's wave-per-query back end (vmis_shard_back_kernel, srn_sback.hip; test_shard_cases_host.py, test_gpu_shard_edges.py): every
fragment length, accumulator address, candidate / floor-list / queue / hit-list / table count is chosen, not drawn.  NumPy only, deterministic, no GPU.  Test-side only.
Written beside edge_cases.py: the same id scheme (id = ID0 + ID_STEP * number), the same Index attributes (edge_cases._list_of works on it), the same timestamp variants.

THE OWNER MAP.  owner(id, G) = murmur3 finaliser of (id ^ 0x9E3779B97F4A7C15) mod G (srn_internal.h:28-32, :93).  Everything is designed against h8 = owner(id, 8); the
same ids are on shard h8 % 4 of four and h8 % 2 of two.  Catalogue numbers are found by walking the arithmetic id sequence and sorting the numbers by h8.

SHARD-LOCAL INDEX = position in the shard's popularity order: kept sessions that hold the item descending, id ascending (srn_index.cpp:181-186 for the full index;
shard_flat_index :253-256 keeps that relative order for the owned items).  Shard g of eight holds N_SHARD catalogue items cat[g][0..2304), ascending ids, in three tiers
of EQUAL session counts, so that cat[g][i] HAS LOCAL INDEX i:
  [0, 16)      HOT      1 000 sessions each (the replicated accumulators; the capacity cells put their long fragments on these)
  [16, 256)    BALLAST     24 sessions each (with HOT: the shard's threshold sample)
  [256, 2304)  TAIL         8 sessions each (direct-mapped up to 895, sketch words from 896 on; 1024 + 896 = 1920 and 2047 / 2048 exist)
Every item is PADDED to its tier's count by filler sessions older than every cell; they hold no query item and so are nobody's neighbours.  All QUERY items (the cells'
known items, with their own large counts) have h8 = 7: shard 7 of eight is nobody's target, its order is restated from the data like every other shard's, and shards 0..6
have exactly the designed order (asserted by the census).  A cell whose rows hold fewer than how_many HOT / BALLAST items has t32 = 0 on every shard: no threshold, floor
1, every valid scored item below 896 a candidate, every element on a sketch item a walk-B hit -- ncand, npass, nlq, nlb, nh, the table's distinct items and M are then
exact integers of the design.  All capacity cells are built this way.

CELLS.  One per query, on a disjoint stretch of the time line (sessions ascend with time: recency rank = session index).  A cell's sessions = its known items' lists,
evenly interleaved, all kept (no list reaches m unless said); `rows[j]` = the catalogue items (g, i) that the j-th most recent session holds besides.  Each cell names its
target shard g of eight; on two shards it lies on shard g % 2, where the tail items of four catalogues interleave by id: there NO designed tail item is direct-mapped
(the first 1 024 local indices are the four shards' HOT and BALLAST items), fragment lengths are the same, and what the kernel does is restated from the data, not designed.
The census for G = 2 therefore asserts the G-independent edges (K, shape, fragment lengths, long-fragment queue, hit list, table, M) and the path test's exact counters hold there too.

RESTATEMENT.  restate_shard works from the sessions alone and follows the kernel line by line (srn_sback.hip): K and the neighbours' weights ((9 - most recent matched
position) * numerator, :252-260), fragments and the long-fragment queue (:397-427), the sample, t32 = the largest multiple of 256 with at least how_many sample keys
(top 32 bits of idf_eff * acc) at or above it (:465-481), candidates down to one step below (:484-495), integer floors per chunk of 256 (:496-529), the floor list's
survivors (:530-544), the live check (:547-554), walk B's queue and hit list (:567-660), the exact table (:661-679, srn_device.h:122-140), M and the hand-off (:704-746).
idf = ln(pairs of all kept sessions / sessions that hold the item), the index's own formula in the same libm.  Edges, with where they come from:
  SB_CAND_CAP 128 (:46, :544)   PLIST_CAP 256 (:505, :529)   SB_LQ_CAP 448 (:50, :427)   SB_LQB_CAP 160 (:51, :642)   SB_HIT_CAP 272 (:51, :660)
  61 buckets x 4 slots, 48 probes (:46, srn_device.h:10)   F_FIN_ENTRIES 63 (srn_kernels.h:88, :722)   F_K_MAX 1 536 (:271)   fragments 4 / 5 (:90), 8 / 9 (:436), 16 / 17 (:439)
  local index 15 / 16 (SB_REP_ITEMS, :66), 255 / 256 .. 767 / 768 (floor chunks, :509-528), 895 / 896 (SB_DIRECT, :67), 1023 / 1024 (idx & 1023)
  walk B's groups of four chunks: K 255 / 256 / 257 (:588)   shape: L <= 8, nr <= 4, sumw <= 15 at the front end (srn_fast.hip:651), marker 0xFFFFFFFF (:271)
  streaming form: kept prefixes 63 / 64 / 65 (a bitmap word) and 640 / 641 (one sweep of SB_PF x 64, :320) -- the K cells' single lists --, a neighbour of two lists
  marked in the first (:849), a run with nothing kept (it_kept == 0 drops the run from rm, nr and ps[], :246-254, :788-801)
  keys at the cut t32, at t32 - 1 (kept) and at t32 - 2 (dropped): t32m1 (:484), k4 >= t32m1 (:488)
HELD CONSERVATIVELY: `table` -- whether an insertion finds a free slot within 48 probes can depend on the insertion order when 193..244 distinct items go in.  The
restatement says 'ok' for <= 192 items (48 full buckets hold 192) or when no bucket is the FIRST choice of more than four items (every item then sits in its first
bucket, in any order), 'fail' for > 244, and 'uncertain' otherwise; the census asserts that no (query, shard) pair of the index is uncertain.

NOT PLACED, because no query reaches it or this module does not design it:
  shard_nb_positions_stride = 0: needs 32 ceil(m / 64) + 8 ceil(k / 8) > 3 584, but the neighbours pipeline takes k <= 1 536 and m <= 2 560 only (2 816): unreachable.
  nmem != K in the streaming form: needs a front end and a position kernel that disagree.
  Keys at the cut on the FLOOR LIST's comparison (:536, the same expression as the sample's :488, which IS placed): an item of local index >= 256 has at most 23
  sessions in this index, too few (count, acc) pairs for three adjacent keys at a multiple of 256; the sample's triple comes from 531 counts x 900 sums (cut_search).
  A batch with m > 2 560 (the lists pipeline serves it) and a session of nine items (nobody's query at max_len 8): nothing of this kernel runs for them; the GPU
  module pins their rows in one call each.
SMALL SHARDS.  small_build() is a second, tiny index whose eight shards hold 0, 1, 15, 16, 17, 255, 256 and 257 items (the sample padded with zero records and guarded
by e < n_items; a shard with nothing at all): drawn rows and queries over those items, compared row for row only -- nothing of it is restated."""
import functools
import math

import numpy as np

import edge_cases as E
from record_cases import route_of

ID0, ID_STEP, UNKNOWN0, T0 = E.ID0, E.ID_STEP, E.UNKNOWN0, E.T0
M_INDEX, F_K_MAX = E.M_INDEX, E.F_K_MAX
SHAPES = ((500, 1100), (F_K_MAX, 2560))
MAX_LEN, ROW_MAX = 8, 80
SB_H, SB_S, SB_DIRECT, SB_REP_ITEMS, SB_REP, SAMPLE = 1024, 1024, 896, 16, 8, 256
SB_CAND_CAP, PLIST_CAP, SB_LQ_CAP, SB_LQB_CAP, SB_HIT_CAP = 128, 256, 448, 160, 272
SB_BUCKETS, MAX_PROBES, F_FIN_ENTRIES = 61, 48, 63
TABLE_SLOTS, TABLE_SAFE = 4 * SB_BUCKETS, 4 * MAX_PROBES
N_SHARD, N_HOT, QUERY_SHARD = 2304, 16, 7
HOT_COUNT, BALLAST_COUNT, TAIL_COUNT = 1000, 24, 8
ATTR_SALE, ATTR_UNSOLD, ATTR_NONE = 2, 0, 0xFF
FRAG_LENGTHS = (0, 1, 3, 4, 5, 8, 9, 16, 17, 24, 25)
ACC_INDICES = (15, 16, 255, 256, 511, 512, 767, 768, 895, 896, 1023, 1024, 1919, 1920, 2047, 2048)
K_VALUES = (1, 63, 64, 65, 255, 256, 257, 640, 641, F_K_MAX - 1, F_K_MAX)


# ---- the owner map ------------------------------------------------------------------------------------------------------------------------------------
def mix64(x):
    """srn_internal.h mix64 on a uint64 array."""
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xFF51AFD7ED558CCD)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xC4CEB9FE1A85EC53)
        x ^= x >> np.uint64(33)
    return x


def owner(ids, G):
    """item_owner(id, G) for an array of ids."""
    return (mix64(np.asarray(ids, dtype=np.uint64) ^ np.uint64(0x9E3779B97F4A7C15)) % np.uint64(G)).astype(np.int64)


def table_bucket(it):
    """item_insert's first bucket of shard-local index `it` (srn_device.h:123)."""
    return (((np.asarray(it, np.int64) * 0x9E3779B1) & 0xFFFFFFFF) * SB_BUCKETS) >> 32


X_BUDGET, X_ITEMS = 2000, 3   # sessions that the three tunable items and their slack item hold together, whatever the search gives each


@functools.lru_cache(maxsize=None)
def catalogue():
    """-> (cat, qpool): cat[g][i] = the item NUMBER of shard g's catalogue item i (ascending); qpool = numbers with h8 == QUERY_SHARD beyond the catalogue."""
    n = 8 * N_SHARD * 2 + 40000
    num = np.arange(n, dtype=np.int64)
    h8 = owner(ID0 + ID_STEP * num, 8)
    cat = [num[h8 == g][:N_SHARD] for g in range(8)]
    assert all(len(c) == N_SHARD for c in cat)
    qpool = num[(h8 == QUERY_SHARD) & (num > cat[QUERY_SHARD][-1])]
    return cat, qpool


def balanced_sketch_items(n):
    """n <= 244 shard-local indices from 896 up, at most four per first bucket of the exact table: they fill it in any insertion order."""
    it = np.arange(SB_DIRECT, N_SHARD)
    b = table_bucket(it)
    out = np.concatenate([it[b == x][:4] for x in range(SB_BUCKETS)])
    assert len(out) == TABLE_SLOTS
    return sorted(out.tolist())[:n] if n < TABLE_SLOTS else sorted(out.tolist())


# ---- cells --------------------------------------------------------------------------------------------------------------------------------------------
def cell(name, family, g, counts, rows, L=None, pos=None, shared=0, fill="unknown", expect=None, business=False, unsold=(), stack=False, xcount=()):
    """g: target shard of eight; counts: sessions per known item (pos: their positions, 0 = most recent; default 0, 1, ..); rows[j]: catalogue items (g, i) of the j-th
    most recent session; shared: sessions that hold the two most recent known items at once; expect: what restate_shard must say for the target shard at SHAPES[1],
    how_many 21 (under the business rules if `business`); unsold: catalogue items (g, i) that are not for sale; stack: the lists one after the other on the time
    line, the last one oldest, not interleaved; xcount: the session counts of the tunable items ('x', j) the cell's rows name (see cut_search)."""
    pos = tuple(range(len(counts))) if pos is None else tuple(pos)
    L = (max(pos) + 1 if pos else 1) if L is None else L
    assert len(pos) == len(counts) and all(p < L for p in pos) and L <= MAX_LEN
    return dict(name=name, family=family, g=g, counts=tuple(counts), rows=rows, L=L, pos=pos, shared=shared, fill=fill, expect=expect or {}, business=business, unsold=tuple(unsold), stack=stack, xcount=tuple(xcount))


def _hi32(x):
    return (np.asarray(x, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64)


CUT_LISTS, CUT_SHARED = (40, 40), 10   # the cut cell: 30 sessions of the most recent item alone (weight 18), 30 of the older one (8), 10 of both (27)


def cut_search(total_pairs):
    """Three (session count, acc) pairs whose keys hi32(ln(total / count) * acc) are v, v - 1 and v - 2 with v a multiple of 256 -- the cut t32 itself, one step below
    it (kept: srn_sback.hip:484-488 keeps down to t32 - 1) and two below (dropped).  acc = 18 a + 8 b + 27 c from a <= 30, b <= 30, c <= 10 neighbours; counts 70..600
    (an item is in at least a + b + c sessions); x < 4 000, below the twenty items that stand above the cut.  -> [(count, (a, b, c))] * 3, the first v found."""
    ways = {}
    for c in range(CUT_SHARED + 1):
        for a in range(CUT_LISTS[0] - CUT_SHARED + 1):
            for b in range(CUT_LISTS[1] - CUT_SHARED + 1):
                ways.setdefault(18 * a + 8 * b + 27 * c, (a, b, c))
    accs = np.array(sorted(x for x in ways if x > 0), np.int64)
    cnt = np.arange(70, 601)
    idf = np.array([math.log(float(total_pairs) / float(c)) for c in cnt], np.float64)
    x = idf[:, None] * accs[None, :].astype(np.float64)
    k = np.where((x > 300.0) & (x < 4000.0), _hi32(x), -1)
    vals = np.unique(k[k > 0])
    v = vals[vals % 256 == 0]
    v = v[np.isin(v - 1, vals) & np.isin(v - 2, vals)]
    assert len(v), "no three adjacent keys at a multiple of 256"
    out = []
    for d in range(3):
        i, j = np.argwhere(k == v[0] - d)[0]
        out.append((int(cnt[i]), ways[int(accs[j])]))
    return out


@functools.lru_cache(maxsize=None)
def cells():
    out = []
    D0, S0 = SAMPLE, SB_DIRECT   # the first direct-mapped tail item, the first sketch item
    # ---- fragments: neighbours whose rows hold exactly n items of the target shard, on direct-mapped and on sketch items ----
    for what, base in (("direct", D0), ("sketch", S0)):
        rows, at = [], base
        for n in FRAG_LENGTHS:
            rows.append([(2, at + x) for x in range(n)])
            at += n
        tot = sum(FRAG_LENGTHS)
        exp = dict(outcome="served_big", nlq=7, ncand=tot, live=False) if what == "direct" else dict(outcome="served_big", nlq=7, nlb=7, ncand=0, nh=tot, nt=tot, live=True)
        out.append(cell("fragments %s" % what, "fragments", 2, [len(rows)], rows, expect=exp))
    out.append(cell("fragment of 79", "fragments", 2, [1], [[(2, 400 + x) for x in range(ROW_MAX - 1)]], expect=dict(outcome="served_big", nlq=1, ncand=79)))
    # ---- accumulators: one scored item per neighbour at every index where the addressing changes; 896 and 1920 share sketch word 896 ----
    out.append(cell("accumulator indices", "accumulators", 4, [len(ACC_INDICES)], [[(4, i)] for i in ACC_INDICES],
                    expect=dict(outcome="served", ncand=9, nh=7, nt=7, live=True, t32=0)))
    out.append(cell("accumulator replicas", "accumulators", 4, [16], [[(4, 3), (4, 17)] for _ in range(16)], expect=dict(outcome="served", ncand=2, live=False)))
    # ---- K and shape ----
    for j, K in enumerate(K_VALUES):
        first = list(range(min(16, K)))
        last = [x for x in range(max(0, K - 16), K) if x not in first]
        rows = [[] for _ in range(K)]
        for n, x in enumerate(first + last):
            rows[x] = [(6, 300 + 32 * j + n)]
        out.append(cell("K=%d" % K, "K", 6, [K], rows, expect=dict(outcome="served", K=K, ncand=len(first + last), nlq=0, live=False)))
    two = lambda n, b: [[(0, b + 2 * x), (0, b + 2 * x + 1)] for x in range(n)]   # noqa: E731
    out.append(cell("nr=4", "shape", 0, [5, 5, 5, 5], two(20, 600), expect=dict(outcome="served", K=20)))
    out.append(cell("nr=5", "shape", 0, [5, 5, 5, 5, 5], two(25, 640), expect=dict(outcome="shape")))
    out.append(cell("sumw=15", "shape", 0, [5, 5, 5], two(15, 690), L=6, pos=(0, 1, 2), expect=dict(outcome="served")))
    out.append(cell("sumw=16", "shape", 0, [5, 5, 5, 5], two(20, 720), L=6, pos=(0, 1, 2, 5), expect=dict(outcome="shape")))
    out.append(cell("L=8", "shape", 0, [6], two(6, 760), L=8, pos=(0,), expect=dict(outcome="served", K=6)))
    out.append(cell("L=8 repeats", "shape", 0, [6], two(6, 772), L=8, pos=(0,), fill="repeat", expect=dict(outcome="served", K=6)))
    out.append(cell("no known item", "shape", 0, [], [], L=3, pos=(), expect=dict(outcome="empty", K=0)))
    out.append(cell("only the current item known", "shape", 0, [6], two(6, 784), L=3, pos=(0,), expect=dict(outcome="served", K=6)))
    out.append(cell("only an older item known", "shape", 0, [6], two(6, 796), L=3, pos=(2,), expect=dict(outcome="served", K=6)))
    out.append(cell("light", "shape", 0, [1], [[(0, 810)]], expect=dict(outcome="served", K=1, ncand=1)))
    # ---- capacities, threshold-free, each at CAP and CAP + 1 ----
    for n in (SB_CAND_CAP, SB_CAND_CAP + 1):      # candidates: two neighbours, n direct-mapped tail items
        items = [(0, D0 + x) for x in range(n)]
        out.append(cell("candidates %d" % n, "capacity", 0, [2], [items[:64], items[64:]],
                        expect=dict(outcome="served_big" if n <= SB_CAND_CAP else "fail_cand", ncand=n, npass=n, live=False)))
    for n in (PLIST_CAP, PLIST_CAP + 1):          # the floor list: n direct-mapped items that are not for sale -- under the rules they pass their floor and are no candidates
        items = [(1, D0 + x) for x in range(n)]
        out.append(cell("floor list %d" % n, "capacity", 1, [4], [items[0:64], items[64:128], items[128:192], items[192:]], business=True, unsold=items,
                        expect=dict(outcome="served" if n <= PLIST_CAP else "fail_cand", npass=n, ncand=0, live=False)))
    for n in (SB_LQ_CAP, SB_LQ_CAP + 1):          # walk A's queue: n neighbours, each a fragment of five HOT (replicated) items
        b = 0 if n == SB_LQ_CAP else 5
        out.append(cell("long queue %d" % n, "capacity", 5, [n], [[(5, b + x) for x in range(5)] for _ in range(n)],
                        expect=dict(outcome="served" if n <= SB_LQ_CAP else "fail_long", nlq=n, live=False)))
    for n in (SB_LQB_CAP, SB_LQB_CAP + 1):        # walk B's queue: n neighbours, each four HOT items and a sketch item of its own
        out.append(cell("walk B queue %d" % n, "capacity", 6, [n], [[(6, 10 + x) for x in range(4)] + [(6, 1000 + j)] for j in range(n)],
                        expect=dict(outcome="served_big" if n <= SB_LQB_CAP else "fail_long", nlq=n, nlb=n, live=True, nh=n if n <= SB_LQB_CAP else 0)))
    for n in (SB_HIT_CAP, SB_HIT_CAP + 1):        # the hit list: n neighbours with one element each, on 34 (35) sketch items
        b = 1200 if n == SB_HIT_CAP else 1300
        out.append(cell("hit list %d" % n, "capacity", 4, [n], [[(4, b + j // TAIL_COUNT)] for j in range(n)],
                        expect=dict(outcome="served" if n <= SB_HIT_CAP else "fail_hits", nh=n, live=True, nlq=0)))
    bal = balanced_sketch_items(TABLE_SLOTS)
    extra = [i for i in range(SB_DIRECT, N_SHARD) if i not in set(bal)][:3]
    for n, its in ((TABLE_SLOTS, bal), (TABLE_SLOTS + 1, bal + extra[:1]), (TABLE_SLOTS + 3, bal + extra)):   # the exact table: 244 items, four per first bucket; one and three more
        items = [(2, i) for i in its]
        out.append(cell("table %d" % n, "capacity", 2, [4], [items[0:64], items[64:128], items[128:192], items[192:]],
                        expect=dict(outcome="served_big" if n <= TABLE_SLOTS else "fail_table", nh=n, table="ok" if n <= TABLE_SLOTS else "fail", live=True)))
    for n in (F_FIN_ENTRIES, F_FIN_ENTRIES + 1):  # M = ncand + nt: 60 candidates + 3 (4) contenders of the exact table
        out.append(cell("M=%d" % n, "capacity", 3, [2], [[(3, D0 + x) for x in range(60)], [(3, S0 + x) for x in range(n - 60)]],
                        expect=dict(outcome="served" if n <= F_FIN_ENTRIES else "served_big", ncand=60, nt=n - 60, M=n, live=True)))
    # ---- threshold: N sample items scored 18 by a neighbour of the most recent item; 30 direct-mapped and 5 sketch items scored 8 by a neighbour of the older one ----
    for n in (20, 21, 22, 23, 24, 25):
        rows = [[(3, 1400 + x) for x in range(5)] + [(3, 500 + x) for x in range(30)], [(3, 20 + x) for x in range(n)]]   # (the older item's session is the more recent one: weight 8; the other: 18)
        out.append(cell("threshold %d sample items" % n, "threshold", 3, [1, 1], rows, expect=dict(valid_sample=n)))
    rows = [[(3, 1500 + x) for x in range(5)] + [(3, 560 + x) for x in range(30)], [(3, 60 + x) for x in range(21)]]
    out.append(cell("threshold 21 sample items, one not for sale", "threshold", 3, [1, 1], rows, business=True, unsold=[(3, 60)], expect=dict(valid_sample=20, t32=0, ncand=50, live=True)))
    # ---- streaming: two lists that share sessions (list-set nibbles that are sums; marked in the first list only) ----
    out.append(cell("shared sessions", "streaming", 2, [70, 70], [[(2, 700 + j % 100)] for j in range(110)], shared=30, expect=dict(outcome="served_big", K=110, ncand=100)))
    # ---- a run with nothing kept: the older item's five sessions lie below the 1 200 of the most recent one -- at m = 1 100 wholly below x_lo (nr = 1, no run);
    #      at m = 2 560 every session is kept (K = 1 205).  The newest 16 and the older list's rows hold an item each ----
    rows = [[] for _ in range(1205)]
    for j in list(range(16)) + list(range(1200, 1205)):
        rows[j] = [(1, 600 + j % 1000)]
    out.append(cell("run with nothing kept", "streaming", 1, [1200, 5], rows, stack=True, expect=dict(outcome="served", K=1205, ncand=21)))
    # ---- keys at the cut, one step and two steps below it (kept, kept, dropped), on shard 7, whose sample holds the tunable items: sixteen HOT and three BALLAST
    #      items and the cell's older known item stand above, the 21st largest key is v itself ----
    total = 8 * (N_HOT * HOT_COUNT + (SAMPLE - N_HOT) * BALLAST_COUNT + (N_SHARD - SAMPLE) * TAIL_COUNT) + X_BUDGET + sum(CUT_LISTS) + sum(sum(c["counts"]) for c in out)
    found = cut_search(total)
    mk = _masks(dict(counts=CUT_LISTS, shared=CUT_SHARED, stack=False))[::-1]
    only_a, only_b, both = np.flatnonzero(mk == 1), np.flatnonzero(mk == 2), np.flatnonzero(mk == 3)
    rows = [[] for _ in range(len(mk))]
    for j in list(only_a) + list(both):
        rows[j] += [(QUERY_SHARD, i) for i in range(N_HOT)]
    for j in list(only_a[:14]) + list(both):
        rows[j] += [(QUERY_SHARD, N_HOT + i) for i in range(3)]
    for x, (_count, (a, b, c)) in enumerate(found):
        for j in list(only_a[:a]) + list(only_b[:b]) + list(both[:c]):
            rows[j].append(("x", x))
    out.append(cell("keys at the cut", "threshold", QUERY_SHARD, CUT_LISTS, rows, shared=CUT_SHARED, xcount=[cnt for cnt, _w in found],
                    expect=dict(outcome="served", valid_sample=23, ncand=22, cut_keys=(1, 1, 1))))
    return out


def _masks(c):
    """The cell's sessions, oldest first, as bit masks of its known items."""
    counts, s = list(c["counts"]), c["shared"]
    if not counts:
        return np.zeros(0, np.int64)
    if c["stack"]:
        return np.concatenate([np.full(n, 1 << i, np.int64) for i, n in reversed(list(enumerate(counts)))])
    if s:
        counts[0] -= s
        counts[1] -= s
    masks = np.array([1 << i for i in range(len(counts))] + [3], np.int64)
    return masks[E._interleave(counts + [s])]


@functools.lru_cache(maxsize=None)
def build(tied=False):
    cs = cells()
    cat, qpool = catalogue()
    cell_first, qnum, sess, num = [], [], [], []
    n_sess = nq = 0
    cell_sessions = []
    for c in cs:
        cell_sessions.append(_masks(c))
    # filler sessions first (the oldest): their number is known once the cells' use of every catalogue item is
    use = {}
    for c in cs:
        for row in c["rows"]:
            assert len(set(row)) == len(row)
            for gi in row:
                use[gi] = use.get(gi, 0) + 1
    pad_item, pad_n = [], []
    for g in range(8):
        for i in range(N_SHARD):
            want = HOT_COUNT if i < N_HOT else BALLAST_COUNT if i < SAMPLE else TAIL_COUNT
            u = use.get((g, i), 0)
            assert u <= want, "catalogue item (%d, %d) is used %d times, its tier allows %d" % (g, i, u, want)
            pad_item.append(cat[g][i])
            pad_n.append(want - u)
    # the tunable items and their slack item (numbers of the query pool far behind the query items): X_BUDGET sessions together, whatever the search gave each
    xnum = [int(x) for x in qpool[600:600 + X_ITEMS + 1]]
    xcount = [n for c in cs for n in c["xcount"]]
    assert len(xcount) == X_ITEMS and X_BUDGET - sum(xcount) >= 1
    for x, want in enumerate(xcount + [X_BUDGET - sum(xcount)]):
        u = use.get(("x", x), 0)
        assert u <= want
        pad_item.append(xnum[x])
        pad_n.append(want - u)
    number_of = lambda gi: xnum[gi[1]] if gi[0] == "x" else cat[gi[0]][gi[1]]   # noqa: E731
    pairs = np.repeat(np.array(pad_item, np.int64), np.array(pad_n, np.int64))
    pairs = pairs[np.argsort(pairs, kind="stable")]
    n_fill = max(int(max(pad_n)), -(-len(pairs) // ROW_MAX))
    sess.append(np.arange(len(pairs), dtype=np.int64) % n_fill)
    num.append(pairs)
    n_sess = n_fill
    for ci, c in enumerate(cs):
        mk = cell_sessions[ci]
        cell_first.append(n_sess)
        qn = [int(qpool[nq + i]) for i in range(len(c["counts"]))]
        qnum.append(qn)
        nq += len(qn)
        for b, x in enumerate(qn):
            s = np.flatnonzero((mk >> b) & 1)
            sess.append(n_sess + s)
            num.append(np.full(len(s), x, np.int64))
        assert len(c["rows"]) <= len(mk), c["name"]
        for j, row in enumerate(c["rows"]):
            sess.append(np.full(len(row), n_sess + len(mk) - 1 - j, np.int64))
            num.append(np.array([number_of(gi) for gi in row], np.int64))
        n_sess += len(mk)
    key = np.unique(np.concatenate(sess) * (1 << 24) + np.concatenate(num))
    assert int(np.concatenate(num).max()) < (1 << 24)
    rs, rn = key >> 24, key & ((1 << 24) - 1)
    off = np.zeros(n_sess + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(rs, minlength=n_sess))
    lens = np.diff(off.astype(np.int64))
    assert int(lens.max()) <= ROW_MAX and int(lens.min()) >= 1, (int(lens.min()), int(lens.max()))
    ix = E.Index()
    ix.cells, ix.first, ix.tied, ix.n_fill = cs, np.array(cell_first + [n_sess], np.int64), tied, n_fill
    ix.off, ix.items = off, (ID0 + ID_STEP * rn).astype(np.uint64)
    idx = np.arange(n_sess)
    ix.ts = (T0 + (idx // 8 if tied else idx)).astype(np.uint32)
    unknown = iter(range(UNKNOWN0, UNKNOWN0 + 10**6))
    ix.queries, ix.q_cell = [], []
    for ci, c in enumerate(cs):
        q = [None] * c["L"]
        for i, p in enumerate(c["pos"]):
            q[c["L"] - 1 - p] = ID0 + ID_STEP * qnum[ci][i]
        for p in range(c["L"]):
            if q[c["L"] - 1 - p] is None:
                newer = [i for i, pp in enumerate(c["pos"]) if pp < p]
                q[c["L"] - 1 - p] = ID0 + ID_STEP * qnum[ci][newer[0]] if c["fill"] == "repeat" and newer else next(unknown)
        ix.queries.append(q)
        ix.q_cell.append(ci)
    order = np.lexsort((idx, ix.ts))
    ix.rank = np.empty(n_sess, np.int64)
    ix.rank[order] = idx
    ix.session_of_rank = order
    by_item = np.lexsort((-ix.rank[rs], rn))
    ix.l_items, l_start = np.unique(rn[by_item], return_index=True)
    ix.l_off = np.concatenate([l_start, [len(rn)]])
    ix.l_sess = rs[by_item]
    cnt = np.diff(ix.l_off)
    pop = np.lexsort((ix.l_items, -cnt))
    ix.dense = np.empty(len(pop), np.int64)
    ix.dense[pop] = np.arange(len(pop))
    ix.row_num = rn
    ix.row_pos = np.searchsorted(ix.l_items, rn)
    ix.count = cnt
    ix.h8 = owner(ID0 + ID_STEP * ix.l_items, 8)
    ix.idf = np.array([math.log(float(len(rn)) / float(x)) for x in cnt], np.float64)
    ix.cat = cat
    # attribute bytes: everything for sale, but what a cell says is not
    attr = np.full(len(ix.l_items), ATTR_SALE, np.uint8)
    for c in cs:
        for g, i in c["unsold"]:
            attr[np.searchsorted(ix.l_items, cat[g][i])] = ATTR_UNSOLD
    ix.attr = attr
    for a in (ix.off, ix.items, ix.ts, ix.attr):
        a.setflags(write=False)
    return ix


def attributes(ix):
    """-> (known ids ascending, attribute bytes) for set_attributes."""
    return (ID0 + ID_STEP * ix.l_items).astype(np.uint64), ix.attr.copy()


# ---- the per-shard view -----------------------------------------------------------------------------------------------------------------------------
class ShardView:
    """Shard g of G: which items it owns, their local index, and the constants the kernel gets at attach time."""


@functools.lru_cache(maxsize=None)
def view(tied, G, g):
    ix = build(tied)
    assert 8 % G == 0
    v = ShardView()
    own = (ix.h8 % G) == g
    by_pop = np.argsort(ix.dense)                       # positions in l_items, most popular first
    mine = by_pop[own[by_pop]]                          # ... of this shard: local index -> position in l_items
    v.G, v.g, v.n_items, v.pos_of = G, g, len(mine), mine
    v.local = np.full(len(ix.l_items), -1, np.int64)
    v.local[mine] = np.arange(len(mine))
    idf = ix.idf[mine]
    v.idf_eff = np.where(idf > 0.0, idf, 1.0)
    v.attr = ix.attr[mine].astype(np.int64)
    every = np.where(ix.idf > 0.0, ix.idf, 1.0)[own]
    v.inv_all = 1.0 / float(every.max()) if len(every) else 1.0
    v.inv_chunk = []
    for c in range(SB_H // 256):
        e = v.idf_eff[256 * c:256 * c + 256]
        v.inv_chunk.append(1.0 / float(e.max()) if len(e) else 1.0)
    return v


def popularity_order(tied, G, g, n):
    """The first n ids of shard g's popularity order (what set_fallback_popular(n) on the shard must give)."""
    ix, v = build(tied), view(tied, G, g)
    return (ID0 + ID_STEP * ix.l_items[v.pos_of[:n]]).astype(np.uint64)


def business_ok(cur, reco):
    """srn_device.h:13-20 on attribute bytes."""
    if reco == ATTR_NONE or not reco & 2:
        return False
    return not reco & 1 or (cur != ATTR_NONE and bool(cur & 1))


def neighbours(ix, q, k, m):
    """The front end's answer for one query, from the sessions alone (edge_cases.restate_one's logic): route, K, and per neighbour its session and weight."""
    L = len(q)
    seen, per = [], []
    for pos in range(L):
        it = q[L - 1 - pos]
        if it in seen:
            continue
        seen.append(it)
        lst = E._list_of(ix, it)
        if lst is not None and len(lst):
            per.append((pos, ix.rank[lst[:m]]))
    xlo = max([int(r[m - 1]) for _p, r in per if len(r) >= m], default=0)
    kept = [r[r >= xlo] for _p, r in per]
    out = dict(L=L, U=len(seen), xlo=xlo, kept=[len(x) for x in kept], n=sum(len(x) for x in kept), nr=sum(1 for x in kept if len(x)))
    out["sumw"] = sum(L - p for p, _r in per)
    rmax = max([int(r[0]) for _p, r in per], default=0)
    out["route"] = route_of(L, out["n"], out["sumw"], rmax - xlo, out["nr"] if 1 <= L <= MAX_LEN else 0, 0, MAX_LEN)
    ranks = np.concatenate(kept + [np.zeros(0, np.int64)])
    w = np.concatenate([np.full(len(x), L - p, np.int64) for (p, _r), x in zip(per, kept)] + [np.zeros(0, np.int64)])
    ps = np.concatenate([np.full(len(x), p, np.int64) for (p, _r), x in zip(per, kept)] + [np.zeros(0, np.int64)])
    cr, inv = np.unique(ranks, return_inverse=True)
    num = np.bincount(inv, weights=w, minlength=len(cr)).astype(np.int64)
    mp = np.full(len(cr), 99, np.int64)
    np.minimum.at(mp, inv, ps)
    lists = np.bincount(inv, minlength=len(cr))
    sel = np.arange(len(cr))[::-1][:m]
    sel = sel[np.lexsort((-cr[sel], -num[sel]))][:k]
    out["C"], out["K"] = min(len(cr), m), len(sel)
    out["sess"], out["rank"], out["w"], out["lists"] = ix.session_of_rank[cr[sel]], cr[sel], ((9 - mp[sel]) * num[sel]).astype(np.int64), lists[sel]
    cur, rem = divmod(int(q[-1]) - ID0, ID_STEP)
    j = int(np.searchsorted(ix.l_items, cur)) if rem == 0 and cur >= 0 else len(ix.l_items)
    out["cur_pos"] = j if j < len(ix.l_items) and ix.l_items[j] == cur else -1
    return out


def restate_shard(ix, q, k, m, how_many, G, g, business=False, nb=None):
    """What vmis_shard_back_kernel does with one query on shard g of G -> dict(outcome, live, K, nlq, nlb, ncand, npass, nh, nt, M, t32, valid_sample, table, frag_len,
    and the counter words it adds: c5, c6, c7_live, c7_table, c14, c15 = (candidates | floor list, long-fragment queues, hit list), listed = handed to the tier behind)."""
    v = view(ix.tied, G, g)
    r = nb if nb is not None else neighbours(ix, q, k, m)
    out = dict(outcome=None, live=False, K=r["K"], nlq=0, nlb=0, ncand=0, npass=0, nh=0, nt=0, M=0, t32=0, valid_sample=0, table="ok", c5=0, c6=0, c7_live=0, c7_table=0,
               c14=0, c15=[0, 0, 0], listed=0, cut_keys=(0, 0, 0), kept=tuple(r["kept"]), frag_len=np.zeros(0, np.int64), scored=np.zeros(0, np.int64), cur_idx=-1)
    if r["route"] != "lean":
        out["outcome"] = "shape"
        return out
    if r["n"] == 0:
        out["outcome"] = "empty"
        return out
    K, sess, w = r["K"], r["sess"], r["w"]
    a, b = ix.off[sess].astype(np.int64), ix.off[sess + 1].astype(np.int64)
    lens = b - a
    at = np.repeat(a - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum()))
    loc, own = v.local[ix.row_pos[at]], np.repeat(np.arange(K), lens)
    loc, own = loc[loc >= 0], own[loc >= 0]
    flen = np.bincount(own, minlength=K)
    out["frag_len"] = flen
    is_long = flen > 4
    nlq = int(is_long.sum())
    out["nlq"] = nlq
    fail = None
    if nlq > SB_LQ_CAP:                                   # (:427-429: the queue's blocks are not walked; the harvest runs over what the short fragments added)
        fail = "fail_long"
        out["c15"][1] += 1
        loc, own = loc[~is_long[own]], own[~is_long[own]]
    size = max(v.n_items, SB_H) + 1
    acc = np.bincount(loc, weights=w[own], minlength=size).astype(np.int64)
    out["scored"] = np.flatnonzero(acc)
    sk = loc >= SB_DIRECT
    sketch = np.bincount(loc[sk] & (SB_S - 1), weights=w[own][sk], minlength=SB_S).astype(np.int64)
    cur_idx = int(v.local[r["cur_pos"]]) if r["cur_pos"] >= 0 else -1
    cur_attr = int(ix.attr[r["cur_pos"]]) if r["cur_pos"] >= 0 else ATTR_NONE
    out["cur_idx"] = cur_idx
    ok = (lambda e: business_ok(cur_attr, int(v.attr[e]))) if business else (lambda e: True)
    # the sample
    e = np.arange(SAMPLE)
    valid = (acc[:SAMPLE] != 0) & (e != cur_idx) & (e < v.n_items)
    if business:
        valid &= np.array([x < v.n_items and ok(x) for x in e])
    idf_s = np.concatenate([v.idf_eff[:SAMPLE], np.ones(max(0, SAMPLE - v.n_items))])
    x4 = np.where(valid, idf_s * acc[:SAMPLE].astype(np.float64), 0.0)
    k4 = _hi32(x4)
    out["valid_sample"] = int(valid.sum())
    t32 = 0
    for bit in range(30, 7, -1):
        c = t32 | (1 << bit)
        if int((k4 >= c).sum()) >= how_many:
            t32 = c
    out["t32"] = t32
    t32m1 = t32 - 1 if t32 else 0
    ncand = int(((x4 != 0.0) & (k4 >= t32m1)).sum())
    scored4 = k4[x4 != 0.0]
    out["cut_keys"] = (int((scored4 == t32).sum()), int((scored4 == t32 - 1).sum()), int((scored4 == t32 - 2).sum())) if t32 else (0, 0, 0)
    x_lo = float(np.array([t32m1 << 32], np.uint64).view(np.float64)[0])
    floor_of = lambda inv: int(min(4.0e9, max(1.0, math.floor(x_lo * inv * (1.0 - 1e-9)) - 1.0)))   # noqa: E731
    floor_b = floor_of(v.inv_all)
    e = np.arange(SAMPLE, SB_DIRECT)
    fls = np.repeat(np.array([floor_of(v.inv_chunk[ch]) for ch in range(1, SB_H // 256)], np.int64), 256)[:len(e)]
    passed = e[(acc[SAMPLE:SB_DIRECT] >= fls) & (e != cur_idx)]
    out["npass"] = len(passed)
    if len(passed) > PLIST_CAP:
        fail = fail or "fail_cand"
        out["c15"][0] += 1
        passed = passed[:0]
    take = _hi32(v.idf_eff[passed] * acc[passed].astype(np.float64)) >= t32m1
    ncand += sum(1 for x in passed[take] if ok(x))
    out["ncand"] = ncand
    if ncand > SB_CAND_CAP:
        fail = fail or "fail_cand"
        out["c15"][0] += 1
    live = bool(sketch.max() >= floor_b)
    out["live"] = live
    nt = 0
    if live and fail is None:
        out["c7_live"] = 1
        hit = sk & (sketch[loc & (SB_S - 1)] >= floor_b)
        out["nlb"] = nlq
        if nlq > SB_LQB_CAP:                              # (:642: the long fragments' elements are not listed)
            fail = "fail_long"
            out["c15"][1] += 1
            hit &= ~is_long[own]
        nh = int(hit.sum())
        out["nh"] = out["c5"] = nh
        if nh > SB_HIT_CAP:
            fail = fail or "fail_hits"
            out["c15"][2] += 1
        else:
            items = np.unique(loc[hit])
            items = np.array([x for x in items if ok(x)], np.int64)
            if len(items) <= TABLE_SAFE:
                table = "ok"
            elif len(items) > TABLE_SLOTS:
                table = "fail"
            else:
                table = "ok" if int(np.bincount(table_bucket(items), minlength=SB_BUCKETS).max()) <= 4 else "uncertain"
            out["table"] = table
            if table != "ok":
                fail = fail or "fail_table"
                out["c7_table"] = 1
            elif fail is None:
                nt = int(((items != cur_idx) & (acc[items] >= floor_b)).sum())
    out["nt"] = nt
    if fail is not None:
        out["outcome"], out["listed"] = fail, 1
        return out
    out["M"] = ncand + nt
    out["outcome"] = "served_big" if out["M"] > F_FIN_ENTRIES else "served"
    out["c6"], out["c14"] = ncand, 1
    return out


@functools.lru_cache(maxsize=None)
def restate(tied, shape, how_many, G, business=False):
    """-> R[query][shard]"""
    ix = build(tied)
    k, m = SHAPES[shape]
    out = []
    for q in ix.queries:
        nb = neighbours(ix, q, k, m)
        out.append([restate_shard(ix, q, k, m, how_many, G, g, business, nb) for g in range(G)])
    return out


def counters(R, queries, g):
    """The counter words of shard g after a call over `queries` (indices into R): slot 5, 6, 14, 15's three fields, slot 7's halves, and the list for the tier behind."""
    rs = [R[qi][g] for qi in queries]
    return dict(c5=sum(r["c5"] for r in rs), c6=sum(r["c6"] for r in rs), c14=sum(r["c14"] for r in rs), c7_live=sum(r["c7_live"] for r in rs),
                c7_table=sum(r["c7_table"] for r in rs), c15=tuple(sum(r["c15"][j] for r in rs) for j in range(3)), listed=sum(r["listed"] for r in rs))


def uncertain_queries(tied, G):
    """Queries whose exact table the restatement cannot decide on some shard of G, at any shape: none at G = 8 (census)."""
    out = set()
    for sh in (0, 1):
        for business in (False, True):
            R = restate(tied, sh, 21, G, business)
            out |= {qi for qi in range(len(R)) if any(r["table"] == "uncertain" for r in R[qi])}
    return sorted(out)


def family_queries(ix, family):
    return [qi for qi, ci in enumerate(ix.q_cell) if ix.cells[ci]["family"] == family]


FAMILIES = ("fragments", "accumulators", "K", "shape", "capacity", "threshold", "streaming")


def census(tied=False, G=8):
    """-> {edge: (query, shard) pairs on it}.  Raises AssertionError with the names of the edges nobody hits; checks the designed order of shards 0..6, every cell's
    `expect` on its own target shard (G = 8), and that no pair's exact table is 'uncertain'."""
    ix = build(tied)
    hits = {}
    if G == 8:
        for g in range(7):       # the designed order: cat[g][i] has local index i
            v = view(tied, 8, g)
            assert v.n_items == N_SHARD and np.array_equal(ix.l_items[v.pos_of], ix.cat[g]), "shard %d is not in its designed order" % g
        assert view(tied, 8, QUERY_SHARD).n_items > N_SHARD
        for ci, c in enumerate(ix.cells):
            r = restate(tied, 1, 21, 8, c["business"])[ci][c["g"]]
            for key, want in c["expect"].items():
                assert r[key] == want, (c["name"], key, r[key], want)
    every = []
    for sh in (0, 1):
        for how_many in (21, 24):
            for business in (False, True):
                R = restate(tied, sh, how_many, G, business)
                every += [(sh, how_many, business, qi, g, R[qi][g]) for qi in range(len(R)) for g in range(G)]
    # (designed at G = 8: no pair is uncertain.  On two shards the 244 balanced items of "table 244" have other local indices: that pair hits no edge, and
    #  uncertain_queries names it for the path test)
    assert G != 8 or not any(r["table"] == "uncertain" for *_x, r in every), "a query's exact table depends on the insertion order"
    every = [t for t in every if t[5]["table"] != "uncertain"]

    def edge(name, pred, only8=False):
        if G == 8 or not only8:
            hits[name] = sum(1 for t in every if pred(t[5], t))
    took = lambda r: r["outcome"] not in ("shape", "empty")   # noqa: E731
    for n in FRAG_LENGTHS:
        edge("fragment of %d items, walk A only" % n, lambda r, t, n=n: took(r) and not r["live"] and bool((r["frag_len"] == n).any()), only8=True)
        edge("fragment of %d items, walk B live" % n, lambda r, t, n=n: took(r) and r["live"] and r["nh"] > 0 and bool((r["frag_len"] == n).any()))
    edge("fragment of 79 items", lambda r, t: took(r) and bool((r["frag_len"] == ROW_MAX - 1).any()))
    for i in ACC_INDICES:
        edge("accumulators: local index %d scored" % i, lambda r, t, i=i: r["outcome"] in ("served", "served_big") and bool((r["scored"] == i).any()), only8=True)
    edge("accumulators: two scored items share a sketch word", lambda r, t: r["outcome"] in ("served", "served_big") and r["nt"] > 0 and
         len(np.unique(r["scored"][r["scored"] >= SB_DIRECT] & (SB_S - 1))) < int((r["scored"] >= SB_DIRECT).sum()), only8=True)
    edge("accumulators: a replicated item scored by >= 16 neighbours", lambda r, t: took(r) and r["K"] >= 16 and bool((r["scored"] < SB_REP_ITEMS).any()) and not r["nlq"], only8=True)
    edge("accumulators: the current item is a sample item", lambda r, t: took(r) and 0 <= r["cur_idx"] < SAMPLE)
    edge("accumulators: the current item is a sketch item", lambda r, t: took(r) and r["cur_idx"] >= SB_DIRECT)
    for K in (0,) + K_VALUES:
        edge("K = %d" % K, lambda r, t, K=K: r["K"] == K and r["outcome"] in ("served", "empty"))
    edge("K: cut by k below the list's length", lambda r, t: r["K"] == SHAPES[0][0] and t[0] == 0 and r["outcome"] == "served")
    edge("shape: the front end's marker", lambda r, t: r["outcome"] == "shape")
    for name, lo, cap in (("candidates", "ncand", SB_CAND_CAP), ("floor list", "npass", PLIST_CAP)):
        edge("%s = %d, kept" % (name, cap), lambda r, t, lo=lo, cap=cap: r[lo] == cap and r["outcome"] in ("served", "served_big"), only8=True)
        edge("%s = %d, handed over" % (name, cap + 1), lambda r, t, lo=lo, cap=cap: r[lo] == cap + 1 and r["outcome"] == "fail_cand" and r["c15"][0] == 1, only8=True)
    edge("long queue = %d, kept" % SB_LQ_CAP, lambda r, t: r["nlq"] == SB_LQ_CAP and r["outcome"] in ("served", "served_big"))
    edge("long queue = %d, handed over" % (SB_LQ_CAP + 1), lambda r, t: r["nlq"] == SB_LQ_CAP + 1 and r["outcome"] == "fail_long")
    edge("walk B queue = %d, kept" % SB_LQB_CAP, lambda r, t: r["nlb"] == SB_LQB_CAP and r["live"] and r["outcome"] in ("served", "served_big"))
    edge("walk B queue = %d, handed over" % (SB_LQB_CAP + 1), lambda r, t: r["nlb"] == SB_LQB_CAP + 1 and r["live"] and r["outcome"] == "fail_long")
    edge("hit list = %d, kept" % SB_HIT_CAP, lambda r, t: r["nh"] == SB_HIT_CAP and r["outcome"] in ("served", "served_big"))
    edge("hit list = %d, handed over" % (SB_HIT_CAP + 1), lambda r, t: r["nh"] == SB_HIT_CAP + 1 and r["outcome"] == "fail_hits")
    edge("table = %d items, kept" % TABLE_SLOTS, lambda r, t: r["nt"] == TABLE_SLOTS and r["outcome"] == "served_big", only8=True)
    edge("table = %d items, handed over" % (TABLE_SLOTS + 1), lambda r, t: r["nh"] == TABLE_SLOTS + 1 and r["outcome"] == "fail_table")
    edge("M = %d, finished in the record" % F_FIN_ENTRIES, lambda r, t: r["M"] == F_FIN_ENTRIES and r["outcome"] == "served" and r["nt"] > 0)
    edge("M = %d, the big-ticket arena" % (F_FIN_ENTRIES + 1), lambda r, t: r["M"] == F_FIN_ENTRIES + 1 and r["outcome"] == "served_big" and r["nt"] > 0)
    for hm in (21, 24):
        edge("threshold: %d valid sample items, how_many %d: none" % (hm - 1, hm), lambda r, t, hm=hm: t[1] == hm and r["valid_sample"] == hm - 1 and r["t32"] == 0 and took(r), only8=True)
        for d in (0, 1):
            edge("threshold: %d valid sample items, how_many %d: set" % (hm + d, hm), lambda r, t, hm=hm, d=d: t[1] == hm and r["valid_sample"] == hm + d and r["t32"] > 0, only8=True)
    edge("threshold: set, scored direct-mapped items dropped", lambda r, t: r["t32"] > 0 and r["outcome"] == "served" and r["ncand"] < int((r["scored"] < SB_DIRECT).sum()) - 1, only8=True)
    edge("threshold: set, scored sketch items and no walk B", lambda r, t: r["t32"] > 0 and not r["live"] and bool((r["scored"] >= SB_DIRECT).any()), only8=True)
    edge("threshold: a sample item the rules exclude sets none", lambda r, t: t[2] and t[1] == 21 and r["valid_sample"] == 20 and r["t32"] == 0 and int((r["scored"] < SAMPLE).sum()) == 21, only8=True)
    edge("streaming: neighbours in two lists", lambda r, t: took(r) and r["K"] == 110)
    edge("streaming: a run with nothing kept", lambda r, t: r["outcome"] == "served" and t[0] == 0 and 0 in r["kept"] and r["kept"][0] == SHAPES[0][1])
    edge("streaming: the same lists, every session kept", lambda r, t: r["outcome"] == "served" and t[0] == 1 and r["kept"] == (1200, 5))
    edge("threshold: sample keys at the cut, one step below (kept) and two below (dropped)", lambda r, t: r["outcome"] == "served" and r["t32"] > 0 and r["t32"] % 256 == 0 and
         r["cut_keys"] == (1, 1, 1) and r["ncand"] == r["valid_sample"] - 1, only8=True)
    missing = [name for name, c in hits.items() if c == 0]
    assert not missing, "edges that no (query, shard) pair of the designed index hits at G = %d: %s" % (G, missing)
    return hits


# ---- small shards ---------------------------------------------------------------------------------------------------------------------------------
SMALL_SIZES = (0, 1, 15, 16, 17, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def small_build():
    """-> Index with off / items / ts / queries: 817 items, SMALL_SIZES[g] of them on shard g of eight; 640 drawn sessions of 1..12 items, popular items first, and 21
    sessions that hold every item once; 96 queries of 1..4 items, every tenth with an id the index does not know."""
    cat, _qpool = catalogue()
    nums = np.concatenate([cat[g][:n] for g, n in enumerate(SMALL_SIZES)])
    rng = np.random.default_rng(20250311)
    nums = nums[rng.permutation(len(nums))]
    p = 1.0 / (1.0 + np.arange(len(nums))) ** 0.7
    p /= p.sum()
    rows = [nums[j:j + 40] for j in range(0, len(nums), 40)]
    rows += [rng.choice(nums, size=1 + s % 12, replace=False, p=p) for s in range(640)]
    ix = E.Index()
    ix.off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    ix.items = (ID0 + ID_STEP * np.concatenate([np.sort(r) for r in rows])).astype(np.uint64)
    ix.ts = (T0 + np.arange(len(rows)) // 3).astype(np.uint32)
    unknown = iter(range(UNKNOWN0, UNKNOWN0 + 1000))
    ix.queries = []
    for j in range(96):
        q = [int(ID0 + ID_STEP * x) for x in rng.choice(nums, size=1 + j % 4, replace=False, p=p)]
        if j % 10 == 9:
            q.insert(j % len(q), next(unknown))
        ix.queries.append(q)
    ix.sizes = np.bincount(owner(ID0 + ID_STEP * nums, 8), minlength=8)
    for a in (ix.off, ix.items, ix.ts):
        a.setflags(write=False)
    return ix
