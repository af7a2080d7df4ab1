"""A second DESIGNED index, for the thresholds of the GENERAL kernel (vmis_predict_kernel, srn_kernels.hip) and of the launch geometry that shapes it (make_geometry,
srn_runtime.hip): tests/test_general_cases_host.py (no GPU) and tests/test_gpu_general_edges.py.  NumPy only, deterministic.  Test-side only.  The approach is
tests/edge_cases.py's: cells on disjoint, ascending stretches of the time line, so a session's recency rank IS its index, in a `distinct` (T0 + index) and a `tied`
(T0 + index // 8) timestamp variant; `restate_one` works every designed quantity out from the sessions ALONE for any (k, m); `census` asserts that both sides of every
edge are hit.  A cell = one query: known items at chosen positions of the session, each with a posting list of chosen length; the lists of a cell are disjoint and evenly
interleaved (plus `shared` groups that hold several of the items at once).

1.  The geometry.  `geometry` restates make_geometry for a plain predict launch; the caller's min_region_b IS 0 there (srn_runtime.hip:934, predict_core; only stage B of
    the sharded pipeline asks for sort room, :993).  Where each constant comes from:
      MISC_WORDS 64, CAND_CAP 1 024, SEL_WORDS 2 048 + 64, BLOCK 512        srn_kernels.h:11-15
      off_q = 64 * 4 + 1 024; off_wave = off_b; region B = max(k * slot, 12 288) rounded to 16          srn_runtime.hip:450-455
      budget 80 KB, the device's maximum (<= 160 KB) where off_a + 32 KB does not fit                   :456-461
      sess_slots = min(floor_pow2(a_max / slot), ceil_pow2(2 need_sess)), >= 256                        :462-463
      hot words 4 096 at k >= 1 024, else 2 048, 0 where count + sum bits pass 32; sketch 8 192         :484-495
      item_buckets = the largest prime <= min((a_max - 4 hot - 4 sketch) / 32, need_item / 2 + 8)       :496-498
      the 32-bit accumulators' range guard (k <= 1 900 or so at 255 items)                              :473-480
    From it (srn_kernels.hip): wwords :530, the merge admission :532, sslots :534, rb_slots :836, CAP_S1 :838, legacy :843.  A worked shape: k 1 500,
    m 2 500, max_len 8 -> off_a 13 920, sess_slots 16 384, hot 4 096, sketch 4 096, item_buckets 1 097, region A 67 872, wwords 20 040, rb_slots 3 072, CAP_S1 572.
    At max_len 21 and k 1 500 the hot words are OFF (sum bits 23 + count bits 11 > 32), so no sketch either: the item table takes every scored item.

2.  Launches (LAUNCHES): batch A = the queries of <= 8 items (position sets, walk_rounds), B = those of <= 21 (numerator slots), C = B and one session of 255 items
    (64-bit slots for every query: rank bits 18 + numerator bits 15).  (k, m): (1 500, 2 500); (1 500, 3 000): CAP_S1 = 72; (1 500, 3 040): CAP_S1 = 32 < 64, `legacy`
    launch-wide; (500, 1 100): the only way to an m-cut inside a rank span of 2 047 (an m-cut has more than m distinct ranks in the span); and B at (1 500, 7 700):
    m > m_index, the only way to Cm > 3 072 and > 7 680.

3.  Cell families (family_counts): merge admission; merge k-cut forms; m-cut; hash bins (the boundary bins of the hash mode's m-cut and k-cut); session table; item
    table; rows; accumulators (no cells of their own: the census finds them among the others; `a sketch word shared by a winner and a loser` needs the oracle's rows and is
    asserted by tests/test_general_cases_host.py); top-n; the 255-item session.

NOT PLACED, and why:
  * boundary-bin overflow at CAP_S1 >= 572 needs a rank span of 2^21: beyond the budget of 400 000 sessions;
  * LEFT OUT AFTER A HANG ON THE GPU, cause not found: cells for the sketch filter's floor (rows of hot items only: no live sketch word | exactly one), for scores that
    are all non-positive (known items at positions beyond 10, with a (500, 1 100) launch of the <= 21-item batch, where the hot words are on), for more than 1 024
    candidates above a weak threshold (the S_COVF redo round: 1 200 items seen once above hot items seen once) and for tie groups of two around x_lo were added
    together; the module's first batch call with them in it did not return within seven minutes on the GPU.  Which cell, and whether the debug call or the product
    call, is not known.  They are out again, with their census edges, until the cause is found from the kernel's code; the general kernel's source is unchanged;
  * a tie group of exactly one rank is one session: no tie.  The tied variant has groups of 8.
"""
import functools

import numpy as np

from edge_cases import _interleave

M_INDEX, ROW_MAX = 3072, 48
K = 1500
LAUNCHES = (("A", K, 2500), ("A", K, 3000), ("A", K, 3040), ("A", 500, 1100), ("B", K, 2500), ("B", K, 7700), ("C", K, 2500))   # (batch, k, m)
BATCH_MAX_LEN = dict(A=8, B=21, C=255)
HOW_MANY = (24, 25, 64, 65, 512)                  # the top-n forms; every other call asks for 21
ROW_LENGTHS = (7, 8, 14, 15, 16, 22, 23, 38, 39, 46, 47, 48)
K_SIZES = (1, 65, 512, 513)                       # (K = 64: the cell of 64 long rows)
N_LOW, N_HOT, N_TAIL = 2048, 4300, 60000
T0, ID0, ID_STEP, UNKNOWN0 = 1000, 10**9, 7, 5 * 10**12
MAX_PROBES, CAND_CAP, SEL_WORDS, BLOCK = 48, 1024, 2048 + 64, 512   # srn_device.h:10, srn_kernels.h:11, :14-15, :13
FIT_PROBES = 24                                   # a table `must fit` where a sequential simulation never needs more bucket probes than this


# ---- make_geometry, restated -----------------------------------------------------------------------------------------------------------------------------------------
def _bits(v):
    return int(v).bit_length()


def _is_prime(n):
    return n >= 2 and all(n % d for d in range(2, int(n ** 0.5) + 1))


def _prime_at_most(n):
    while n > 2 and not _is_prime(n):
        n -= 1
    return max(n, 2)


def _round_up(v, a):
    return (v + a - 1) // a * a


def _floor_pow2(v):
    return 1 << (max(int(v), 1).bit_length() - 1)


def _ceil_pow2(v):
    return 1 if v <= 1 else 1 << (int(v) - 1).bit_length()


def geometry(k, m, max_len, info, knobs=None, lds_max=160 * 1024):
    """make_geometry (srn_runtime.hip:434-506) with min_region_b = 0.  info: n_kept, n_items, m_index, max_row_len (lists complete); knobs: {SRN_NO_MASKS, SRN_NO_MERGE,
    SRN_HOT_SLOTS, SRN_SKETCH_SLOTS, SRN_LDS_BUDGET_KB} as the environment gives them.  -> the accessor's words by name, or None where the runtime refuses the launch."""
    kn = knobs or {}
    no_masks, no_merge = bool(int(kn.get("SRN_NO_MASKS", 0))), bool(int(kn.get("SRN_NO_MERGE", 0)))
    hot_knob, sk_knob, budget_kb = int(kn.get("SRN_HOT_SLOTS", -1)), int(kn.get("SRN_SKETCH_SLOTS", -1)), int(kn.get("SRN_LDS_BUDGET_KB", 0))
    L, n_kept, n_items = max_len, info["n_kept"], info["n_items"]
    g = {}
    g["masks"] = int(L <= 8 and m <= info["m_index"] and not no_masks)                       # :438
    num_bits = L if g["masks"] else max(1, _bits(L * (L + 1) // 2))                            # :439
    rank_bits = max(1, _bits(n_kept - 1 if n_kept else 0))                                     # :440
    g["slot64"] = int(rank_bits + num_bits > 32 or n_kept >= 0xFFFFFFF0)                       # :441
    sb = g["slot_bytes"] = 8 if g["slot64"] else 4
    m_eff = min(m, info["m_index"])
    need_sess = max(1, min(L * m_eff, n_kept))                                                 # :446
    need_item = max(1, min(k * max(1, info["max_row_len"]), n_items))                          # :447
    g["num_bits"], g["q_cap"] = num_bits, _round_up(L + 1, 4)
    g["off_q"] = 64 * 4 + 1024                                                                 # :451
    g["off_wave"] = g["off_b"] = _round_up(g["off_q"] + g["q_cap"] * 24 + (g["q_cap"] + 4) * 4, 16)
    region_b = _round_up(max(k * sb, CAND_CAP * 12), 16)                                       # :454
    g["off_a"] = g["off_b"] + region_b
    lds_max = min(lds_max, 160 * 1024)
    budget = budget_kb * 1024 if budget_kb else 80 * 1024                                      # :457-458
    if g["off_a"] + 32 * 1024 > budget:
        budget = lds_max
    if g["off_a"] + 8 * 1024 > budget:
        return None
    a_max = budget - g["off_a"]
    g["sess_slots"] = max(min(_floor_pow2(a_max // sb), min(1 << 30, _ceil_pow2(need_sess * 2))), 256)   # :462-463
    w_abs = 9 if g["masks"] else max(9, min(L, 99) - 10 if min(L, 99) > 10 else 0)             # :468
    w_max = k * w_abs * (L * (L + 1) // 2) + 1
    wn_max = max((10 - q if q <= 10 else q - 10) * ((L - q + 1) * (L - q + 2) // 2) for q in range(1, min(L, 99) + 1))
    if k * wn_max >= 1 << 31:                                                                  # :479
        return None
    g["sketch_may_wrap"] = int(k * max(1, info["max_row_len"]) * 9 * (L * (L + 1) // 2) >= 1 << 32)   # :432
    sbits, cbits = max(2, _bits(w_max) + 1), _bits(k)                                          # :484
    fits32 = sbits + cbits <= 32
    hot = (4096 if k >= 1024 else 2048) if fits32 else 0                                       # :487
    if hot_knob >= 0:
        hot = hot_knob if fits32 else 0
    hot = min(hot, a_max // 8, _round_up(min(n_items, 1 << 20), 4)) // 4 * 4                   # :489
    g["hot_slots"], g["sum_bits"] = hot, sbits
    sk = 8192 if hot and not g["sketch_may_wrap"] else 0                                       # :492
    if sk_knob >= 0:
        sk = _floor_pow2(sk_knob) if hot and not g["sketch_may_wrap"] and sk_knob > 0 else 0
    while sk and sk * 4 * 8 > (a_max - hot * 4) * 5:                                           # :494
        sk >>= 1
    g["sketch_slots"], g["sketch_shift"] = sk, (32 - (_bits(sk) - 1) if sk else 31)
    want_buckets = max(61, need_item // 2 + 8)                                                 # :496
    g["item_buckets"] = _prime_at_most(min((a_max - hot * 4 - sk * 4) // 32, want_buckets))
    g["item_slots"] = g["item_buckets"] * 4
    g["region_a_bytes"] = max(hot * 4 + sk * 4 + g["item_slots"] * 8, g["sess_slots"] * sb)    # :499
    g["no_merge"] = int(no_merge)
    g["lds"] = g["off_a"] + g["region_a_bytes"]
    g["sess_may_overflow"], g["item_may_overflow"] = int(g["sess_slots"] < need_sess * 2), int(g["item_slots"] < need_item * 2)   # :504
    g["lds_max"] = lds_max
    # what the kernel derives from those words (srn_kernels.hip)
    g["wwords"] = ((g["off_a"] - g["off_b"]) + g["region_a_bytes"]) // 4                       # :530
    g["rb_slots"] = (g["off_a"] - g["off_b"]) // sb                                            # :836
    g["CAP_S1"] = max(g["rb_slots"] - m, 0)                                                    # :838
    g["legacy"] = int(g["CAP_S1"] < 64 or g["region_a_bytes"] < SEL_WORDS * 4 + (k + m) * sb)  # :843 (launch-uniform part)
    return g


def sslots_of(g, P):
    """The session table of one query (srn_kernels.hip:534)."""
    s = 256
    while s < g["sess_slots"] and s * 2 < P * 3:
        s <<= 1
    return s


def merge_mode(g, r):
    """srn_kernels.hip:532 (stage 0, LDS tables, u32 slots, prep records: every batch call has them)."""
    return bool(not g["slot64"] and r["nruns"] <= 8 and r["sumw"] <= 63 and 2 * r["P"] + 64 <= g["wwords"] and not g["no_merge"])


def kcut_form(g, r, k, m):
    """The merge mode's k-cut (srn_kernels.hip:669-743): 'all' (Cm <= k) | 'packed' / 'ballot' class counts + 'regs' / 'loop' selection."""
    Cm = min(r["Call"], m)
    if Cm <= k:
        return "all"
    return ("packed" if r["sumw"] <= 15 and Cm <= 15 * BLOCK else "ballot") + "+" + ("regs" if (Cm + BLOCK - 1) // BLOCK <= 6 else "loop")


# ---- the double-hashed tables, sequentially (srn_kernels.hip:61-63, :244-266; srn_device.h:122-140) ---------------------------------------------------------------------
def _u32(x):
    return x & 0xFFFFFFFF


def sess_probes(keys, sslots):
    """Insert the ranks in the given order into `sslots` slots of 4-slot buckets -> the largest number of bucket probes any insert needed (MAX_PROBES + 1: one failed)."""
    bmask = sslots // 4 - 1
    fill = np.zeros(bmask + 1, np.int64)
    worst = 0
    for r in keys:
        r = int(r)
        b, step = (_u32(r * 0x9E3779B1) >> 7) & bmask, ((_u32(r * 0x85EBCA6B) >> 9) | 1) & bmask
        p = 0
        while p < MAX_PROBES and fill[b] == 4:
            b, p = (b + step) & bmask, p + 1
        if p == MAX_PROBES:
            return MAX_PROBES + 1
        fill[b] += 1
        worst = max(worst, p + 1)
    return worst


def item_probes(keys, nb):
    """... the item table: nb (prime) buckets."""
    fill = np.zeros(nb, np.int64)
    worst = 0
    for it in keys:
        it = int(it)
        b, step = (_u32(it * 0x9E3779B1) * nb) >> 32, 1 + ((_u32(it * 0x85EBCA6B) * (nb - 1)) >> 32)
        p = 0
        while p < MAX_PROBES and fill[b] == 4:
            b, p = (b + step) % nb, p + 1
        if p == MAX_PROBES:
            return MAX_PROBES + 1
        fill[b] += 1
        worst = max(worst, p + 1)
    return worst


def hash_part(keys, parts):
    return (_u32(np.asarray(keys, np.int64) * 0xC2B2AE35) * parts) >> 32


def orders(keys):
    """Three insertion orders: ascending, descending, a fixed shuffle."""
    a = np.sort(np.asarray(keys, np.int64))
    return a, a[::-1], np.random.default_rng(7).permutation(a)


def item_parts(g, nonhot):
    """What the partition loop (srn_kernels.hip:1412-1470) must arrive at for these non-hot scored items with the filter off -> (lo, hi, exact): parts is a power of two,
    lo <= parts <= hi; exact: lo == hi and at that level every partition fits within FIT_PROBES probes in three orders -- the GPU test may assert equality."""
    nonhot = np.asarray(nonhot, np.int64)
    lo = 1
    while lo < 64 and np.bincount(hash_part(nonhot, lo), minlength=lo).max() > g["item_slots"]:   # (pigeonhole: that level MUST overflow)
        lo *= 2
    hi = lo
    while hi < 64:
        part = hash_part(nonhot, hi)
        if all(item_probes(o, g["item_buckets"]) <= FIT_PROBES for p in range(hi) for o in orders(nonhot[part == p])):
            break
        hi *= 2
    return lo, hi, lo == hi


# ---- the cells --------------------------------------------------------------------------------------------------------------------------------------------------------
def cell(name, family, L, pos, counts, shared=(), payload=None, query=True, align=None):
    """L: the session's length; pos: the known items' positions (0 = most recent; unknown ids elsewhere); counts: sessions that hold item i ALONE; shared: ((bit mask of
    items, sessions), ...); payload: None (3 hot items + 1 of the tail), ('rare', r): 3 hot + r items nobody else has, ('rows', where, lengths): the cell's most recent
    sessions get rows of exactly those lengths from items nobody else has, where = 'high' (the query's item first in the row) | 'low' (last); align = (least first rank, modulus, residue): sessions that hold no
    query item are put in front of the cell until its first session's rank is at least that and congruent to the residue."""
    assert len(pos) == len(counts) and list(pos) == sorted(set(pos)) and max(pos) < L
    return dict(name=name, family=family, L=L, pos=tuple(pos), counts=tuple(counts), shared=tuple(shared), payload=payload, query=query, align=align)


def _info_guess():
    return dict(n_kept=1 << 18, n_items=1 << 17, m_index=M_INDEX, max_row_len=ROW_MAX)   # (the cells need wwords only, which no field of the index moves at these sizes: asserted by census)


def cells():
    out = []
    gA, gB = geometry(K, 2500, 8, _info_guess()), geometry(K, 2500, 21, _info_guess())
    k, m = K, 2500
    # ---- merge admission ----
    out.append(cell("nruns=8", "merge admission", 8, range(8), [40] * 8))
    out.append(cell("nruns=9", "merge admission", 9, range(9), [40] * 9))
    out.append(cell("sumw=63", "merge admission", 12, range(7), [40] * 7))
    out.append(cell("sumw=64", "merge admission", 12, list(range(7)) + [11], [40] * 8))
    for d in (0, 1):
        P = (gA["wwords"] - 64) // 2 + d
        out.append(cell("2P+64=wwords%+d (<= 8 items)" % (2 * d), "merge admission", 4, range(4), [P // 4 + (1 if i < P % 4 else 0) for i in range(4)]))
        P = (gB["wwords"] - 64) // 2 + d
        out.append(cell("2P+64=wwords%+d (<= 21 items)" % (2 * d), "merge admission", 9, range(4), [P // 4 + (1 if i < P % 4 else 0) for i in range(4)]))
    # ---- merge k-cut ----
    out.append(cell("Cm=k", "merge k-cut", 2, (0, 1), [k // 2, k // 2]))
    out.append(cell("Cm=k+1", "merge k-cut", 2, (0, 1), [k // 2, k // 2 + 1]))
    out.append(cell("k-cut sumw=15", "merge k-cut", 5, range(5), [400] * 5))
    out.append(cell("k-cut sumw=16", "merge k-cut", 6, (0, 1, 2, 5), [500] * 4))
    out.append(cell("Cm=3072", "merge k-cut", 2, (0, 1), [1536, 1536]))
    out.append(cell("Cm=3073", "merge k-cut", 2, (0, 1), [1536, 1537]))
    out.append(cell("Cm=7680", "merge k-cut", 3, (0, 1, 2), [2560, 2560, 2560]))
    out.append(cell("Cm=7681", "merge k-cut", 3, (0, 1, 2), [2560, 2560, 2561]))
    out.append(cell("k-th the last of its class", "merge k-cut", 2, (0, 1), [k, 300]))
    out.append(cell("k-th the first of the next class", "merge k-cut", 2, (0, 1), [k - 1, 300]))
    # ---- m-cut ----
    for mm in (2500, 3000):
        out.append(cell("Call=m, no list reaches m (m=%d)" % mm, "m-cut", 2, (0, 1), [mm // 2, mm // 2]))
        out.append(cell("Call=m+1, no list reaches m (m=%d)" % mm, "m-cut", 2, (0, 1), [mm // 2, mm // 2 + 1]))
    out.append(cell("Call=m, a list reaches m", "m-cut", 2, (0, 1), [m - 1, 0], shared=((3, 1),)))
    out.append(cell("Call=m+1, a list reaches m", "m-cut", 2, (0, 1), [m, 1]))
    out.append(cell("a list far beyond m_index", "m-cut", 1, (0,), [M_INDEX + 4500]))
    # ---- session table ----
    out.append(cell("distinct kept = sess_slots/2", "session table", 8, range(8), [gA["sess_slots"] // 16] * 8))
    out.append(cell("distinct kept > sess_slots", "session table", 8, range(8), [2499] * 8))
    # ---- item table ----
    for r in (1, 3, 6):   # (besides the one tail item every plain row has: about 3 000 | 6 000 | 10 500 scored items outside the hot words, against 4 388 slots)
        out.append(cell("k neighbours x %d rare items" % r, "item table", 1, (0,), [k], payload=("rare", r)))
    # ---- rows ----
    for where in ("high", "low"):
        out.append(cell("row lengths, the query's item %s" % ("first" if where == "high" else "last"), "rows", 1, (0,), [len(ROW_LENGTHS)], payload=("rows", where, ROW_LENGTHS)))
    out.append(cell("K=64, every row of 48 items", "rows", 1, (0,), [64], payload=("rows", "high", (48,) * 64)))
    for n in K_SIZES:
        out.append(cell("K=%d" % n, "rows", 1, (0,), [n]))
    out.append(cell("two items, rows of 39 and 47", "rows", 3, (0, 2), [20, 20], payload=("rows", "low", (39, 47) * 20)))
    # ---- top-n ----
    out.append(cell("64 candidates", "top-n", 1, (0,), [3], payload=("rows", "high", (23, 22, 22))))
    out.append(cell("65 candidates", "top-n", 1, (0,), [3], payload=("rows", "high", (23, 23, 22))))
    out.append(cell("ties across the n-th place", "top-n", 1, (0,), [2], payload=("rows", "high", (31, 31))))   # 60 items with one and the same score: the id decides at every how_many below
    # ---- hash bins (they bite in the hash mode: every launch also runs under SRN_NO_MERGE=1).  Ranks beyond 2^17 with x_lo = 0: rb_all = 18, so the m-cut's bins are 128
    # ranks wide (sh1 = 7) and, at sumw = 1, the k-cut's 512 (sh2 = 9); a cell is a contiguous stretch of ranks, so where it STARTS inside a bin sets the boundary bin's count ----
    cap = gA["rb_slots"] - 3000                       # CAP_S1 of the (1 500, 3 000) launch
    for d in (0, 1):
        out.append(cell("m-cut boundary bin n1=CAP_S1%+d (m=3000)" % d, "hash bins", 2, (0, 1), [1505, 1505], align=(1 << 17, 128, 128 - cap - d)))
        out.append(cell("k-cut boundary bin n2=%d" % (128 + d), "hash bins", 1, (0,), [1600], align=(1 << 17, 512, 512 - 128 - d)))
    # a rank span of 2 047 | 2 048 under an m-cut (sh1 0 | 1) needs m < 2 048: the (500, 1 100) launch.  The list that reaches m sets x_lo = the cell's oldest session
    for d in (0, 1):
        out.append(cell("rank span %d under an m-cut (m=1100)" % (2047 + d), "hash bins", 2, (0, 1), [1100, 948 + d]))
    # ---- the 64-bit-slot launch's long session ----
    out.append(cell("L=255", "slot64", 255, (0, 100), [300, 400]))
    return out


class Index:
    pass


@functools.lru_cache(maxsize=None)
def build(tied=False):
    cs = cells()
    masks, first, end, qitem0 = [], [], [], []
    n_sess = n_qi = 0
    for c in cs:
        groups = [(1 << i, n) for i, n in enumerate(c["counts"])] + list(c["shared"])
        mk = np.array([g[0] for g in groups], np.int64)[_interleave([g[1] for g in groups])]
        if c["align"]:
            least, mod, res = c["align"]
            pad = max(least - n_sess, 0)
            pad += (res - (n_sess + pad)) % mod
            masks.append(np.zeros(pad, np.int64))
            n_sess += pad
        first.append(n_sess)
        end.append(n_sess + len(mk))
        qitem0.append(n_qi)
        masks.append(mk)
        n_sess += len(mk)
        n_qi += len(c["counts"])
    masks = np.concatenate(masks)
    first = np.array(first + [n_sess], np.int64)
    cell_of = np.searchsorted(first, np.arange(n_sess), side="right") - 1   # (the sessions put in front of an aligned cell hold no query item: never looked up)
    # item numbers: a `low` catalogue below the query items, the query items, the hot set, the tail, then items nobody shares; id = ID0 + ID_STEP * number
    q0 = N_LOW
    hot0, tail0 = q0 + n_qi, q0 + n_qi + N_HOT
    rare0 = tail0 + N_TAIL
    sess, num = [], []
    for b in range(int(masks.max()).bit_length()):
        s = np.flatnonzero((masks >> b) & 1)
        sess.append(s)
        num.append(q0 + np.array(qitem0, np.int64)[cell_of[s]] + b)
    rng = np.random.default_rng(20240921)
    explicit = np.zeros(n_sess, bool)
    n_rare = n_low = 0
    extra_rare = np.zeros(n_sess, np.int64)
    for ci, c in enumerate(cs):
        p = c["payload"]
        if p and p[0] == "rows":
            for j, n in enumerate(p[2]):
                s = end[ci] - 1 - j
                explicit[s] = True
                want = n - bin(int(masks[s])).count("1")
                if p[1] == "low":
                    ids = (n_low + np.arange(want)) % N_LOW
                    n_low += want
                else:
                    ids = rare0 + n_rare + np.arange(want)
                    n_rare += want
                sess.append(np.full(want, s, np.int64))
                num.append(ids.astype(np.int64))
        elif p and p[0] == "rare":
            extra_rare[first[ci]:end[ci]] = p[1]
    assert n_low <= N_LOW
    plain = np.flatnonzero(~explicit)
    hot = rng.integers(0, N_HOT, size=(len(plain), 3))
    tail = rng.integers(0, N_TAIL, size=len(plain))
    sess += [np.repeat(plain, 3), plain]
    num += [hot0 + hot.reshape(-1), tail0 + tail]
    er = extra_rare[plain]
    sess.append(np.repeat(plain, er))
    num.append(rare0 + n_rare + np.arange(int(er.sum())))
    key = np.unique(np.concatenate(sess) * (1 << 24) + np.concatenate(num))   # rows ascending and de-duplicated
    assert int(np.concatenate(num).max()) < 1 << 24
    rs, rn = key >> 24, key & ((1 << 24) - 1)
    off = np.zeros(n_sess + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(rs, minlength=n_sess))
    lens = np.diff(off.astype(np.int64))
    assert int(lens.max()) <= ROW_MAX and int(lens.min()) >= 1
    ix = Index()
    ix.cells, ix.first, ix.tied, ix.n_sess = cs, first, tied, n_sess
    ix.off, ix.items = off, (ID0 + ID_STEP * rn).astype(np.uint64)
    idx = np.arange(n_sess)
    ix.ts = (T0 + (idx // 8 if tied else idx)).astype(np.uint32)
    unknown = iter(range(UNKNOWN0, UNKNOWN0 + 10**6))
    ix.queries, ix.q_cell = [], []
    for ci, c in enumerate(cs):
        if not c["query"]:
            continue
        q = [None] * c["L"]
        for i, p in enumerate(c["pos"]):
            q[c["L"] - 1 - p] = ID0 + ID_STEP * (q0 + qitem0[ci] + i)
        ix.queries.append([x if x is not None else next(unknown) for x in q])
        ix.q_cell.append(ci)
    ix.rank, ix.session_of_rank = idx, idx          # (recency rank = index, in both variants: tests/test_general_cases_host.py holds the restatement against the oracle's counters, neighbours and accumulators)
    by_item = np.lexsort((-rs, rn))
    ix.l_items, l_start = np.unique(rn[by_item], return_index=True)
    ix.l_off = np.concatenate([l_start, [len(rn)]])
    ix.l_sess = rs[by_item]
    cnt = np.diff(ix.l_off)
    pop = np.lexsort((ix.l_items, -cnt))            # session count descending, id ascending (fill_cases.popularity_order)
    ix.dense = np.empty(len(pop), np.int64)
    ix.dense[pop] = np.arange(len(pop))
    ix.row_num = rn
    ix.info = dict(n_kept=n_sess, n_items=len(ix.l_items), m_index=M_INDEX, max_row_len=int(lens.max()))
    for a in (ix.off, ix.items, ix.ts):
        a.setflags(write=False)
    return ix


def batch(ix, name):
    """The query numbers of a launch's batch."""
    return [qi for qi, q in enumerate(ix.queries) if len(q) <= BATCH_MAX_LEN[name]]


def _list_of(ix, item_id):
    numb, rem = divmod(int(item_id) - ID0, ID_STEP)
    if int(item_id) < ID0 or rem:
        return None
    j = int(np.searchsorted(ix.l_items, numb))
    if j >= len(ix.l_items) or ix.l_items[j] != numb:
        return None
    return ix.l_sess[ix.l_off[j]:ix.l_off[j + 1]][:M_INDEX]


def restate_one(ix, q, k, m):
    """Every designed quantity of one query at (k, m), from the sessions alone (edge_cases.restate_one without the fast kernels' routing)."""
    L = len(q)
    seen, per, stored = [], [], []
    for pos in range(L):
        it = q[L - 1 - pos]
        if it in seen:
            continue
        seen.append(it)
        lst = _list_of(ix, it)
        if lst is not None and len(lst):
            per.append((pos, ix.rank[lst[:m]]))
            stored.append(ix.rank[lst])
    xlo = max([int(r[m - 1]) for _p, r in per if len(r) >= m], default=0)
    out = dict(L=L, U=len(seen), xlo=xlo, nruns=len(per), P=sum(len(r) for _p, r in per), sumw=sum(L - p for p, _r in per))
    out["rmax"] = max([int(r[0]) for _p, r in per], default=0)
    ranks = np.concatenate([r[r >= xlo] for _p, r in per] + [np.zeros(0, np.int64)])
    w = np.concatenate([np.full(int((r >= xlo).sum()), L - p, np.int64) for p, r in per] + [np.zeros(0, np.int64)])
    cr, inv = np.unique(ranks, return_inverse=True)
    num = np.bincount(inv, weights=w, minlength=len(cr)).astype(np.int64)
    out["Call"], out["kept_ranks"] = len(cr), cr
    cr, num = cr[::-1][:m], num[::-1][:m]
    by = np.lexsort((-cr, -num))
    cr, num = cr[by], num[by]
    out["C"], out["K"] = len(cr), min(k, len(cr))
    # the hash mode's two boundary bins (srn_kernels.hip:845-847, :849, :894): bins of (rank - x_lo) >> sh1 for the m-cut, of (numerator << rb_all | rank - x_lo) >> sh2 for the k-cut
    rb_all = _bits(out["rmax"] - xlo)
    out["sh1"], out["sh2"] = max(rb_all - 11, 0), max(_bits(out["sumw"]) + rb_all - 11, 0)
    out["n1"] = out["n2"] = None
    if out["Call"] > m:
        bins = (out["kept_ranks"] - xlo) >> out["sh1"]
        out["n1"] = int((bins == bins[len(bins) - m]).sum())            # (kept_ranks ascends: the m-th most recent)
    if len(cr) > k:
        bins = ((num << rb_all) | (cr - xlo)) >> out["sh2"]
        out["n2"] = int((bins == bins[k - 1]).sum())
    out["nb"] = sorted(zip(ix.session_of_rank[cr[:k]].tolist(), num[:k].tolist()))
    out["boundary"] = None
    if len(cr) > k:
        b = int(num[k - 1])
        out["boundary"] = dict(cls=b, next=int(num[k]), size=int((num == b).sum()), taken=int((num[:k] == b).sum()),
                               tied=bool(ix.ts[cr[k - 1]] == ix.ts[cr[k]]))
    nbs = ix.session_of_rank[cr[:k]]
    a, b = ix.off[nbs].astype(np.int64), ix.off[nbs + 1].astype(np.int64)
    rows = ix.row_num[np.repeat(a - np.concatenate([[0], np.cumsum(b - a)[:-1]]), b - a) + np.arange(int((b - a).sum()))] if len(nbs) else np.zeros(0, np.int64)
    scored = np.unique(rows)
    cur, rem = divmod(int(q[-1]) - ID0, ID_STEP)
    out["I"], out["D"], out["row_lengths"] = len(rows), len(scored), b - a
    out["dense"] = ix.dense[np.searchsorted(ix.l_items, scored)]
    out["below_adjacent"] = bool(xlo > 0 and any(bool((r == xlo - 1).any()) for r in stored))   # (the session just below the cut holds an item of the query)
    # acc(item) = sum over the neighbours of (10 - first match position) * numerator: the first match of a neighbour is the most recent session item its row holds
    owner = np.repeat(np.arange(len(nbs)), b - a)
    first_match = np.full(len(nbs), 10**6, np.int64)
    for pos in range(L - 1, -1, -1):
        numb, rem_ = divmod(int(q[L - 1 - pos]) - ID0, ID_STEP)
        if rem_ == 0 and numb >= 0:
            first_match[owner[rows == numb]] = pos + 1
    w10 = np.where(first_match < 100, 10 - first_match, 0)
    at = np.searchsorted(scored, rows)
    out["acc"] = np.bincount(at, weights=(w10 * num[:k])[owner], minlength=len(scored)).astype(np.int64)
    out["scored"] = scored
    out["cur"] = cur if rem == 0 else -1
    j = int(np.searchsorted(ix.l_items, cur)) if rem == 0 else len(ix.l_items)
    out["cur_dense"] = int(ix.dense[j]) if j < len(ix.l_items) and ix.l_items[j] == cur else -1
    return out


@functools.lru_cache(maxsize=None)
def restate(tied, k, m):
    ix = build(tied)
    return [restate_one(ix, q, k, m) for q in ix.queries]


def geometry_of(ix, launch, knobs=None, lds_max=160 * 1024):
    b, k, m = launch
    return geometry(k, m, BATCH_MAX_LEN[b], ix.info, knobs, lds_max)


def expect_status(ix, launch, knobs=None):
    """Per query of the launch's batch, with the debug outputs on (filter off): ('global',) | ('fit',) | ('parts', lo, hi, exact) | None (nothing may be asserted beyond
    'not 3, not 4').  global: the distinct kept sessions outnumber the query's session table (pigeonhole); fit: both tables within FIT_PROBES probes in three orders."""
    b, k, m = launch
    g = geometry_of(ix, launch, knobs)
    R = restate(ix.tied, k, m)
    out = []
    for qi in batch(ix, b):
        r = R[qi]
        mm = merge_mode(g, r)
        sl = sslots_of(g, r["P"])
        if not mm and r["Call"] > sl:
            out.append(("global",))
            continue
        sess_fit = mm or all(sess_probes(o, sl) <= FIT_PROBES for o in orders(r["kept_ranks"]))   # (the load is <= 2/3 by :534 wherever P fits)
        nonhot = r["dense"][r["dense"] >= g["hot_slots"]]
        lo, hi, exact = item_parts(g, nonhot)
        if not sess_fit:
            out.append(None)
        elif (lo, hi) == (1, 1):
            out.append(("fit",))
        else:
            out.append(("parts", lo, hi, exact))
    return out


FAMILIES = ("merge admission", "merge k-cut", "m-cut", "hash bins", "session table", "item table", "rows", "accumulators", "top-n", "slot64")


def census(tied=False):
    """-> {edge: (query, launch) pairs on it}.  AssertionError names the edges nobody hits."""
    ix = build(tied)
    G = {l: geometry_of(ix, l) for l in LAUNCHES}
    assert all(g is not None for g in G.values())
    guess = _info_guess()
    for (b, k, m) in LAUNCHES:   # the cells were sized with a guessed index: the words they used are the real index's
        gg = geometry(k, m, BATCH_MAX_LEN[b], guess)
        assert all(gg[w] == G[(b, k, m)][w] for w in ("wwords", "sess_slots", "rb_slots", "CAP_S1")), (b, k, m)
    every = [(l, qi, restate(tied, l[1], l[2])[qi]) for l in LAUNCHES for qi in batch(ix, l[0])]
    hits = {}

    def edge(name, pred):
        hits[name] = sum(1 for l, qi, r in every if pred(l, G[l], r))
    mg = lambda g, r: merge_mode(g, r)   # noqa: E731
    A, B, C_ = ("A", K, 2500), ("B", K, 2500), ("C", K, 2500)
    # geometry
    assert G[A]["masks"] and not G[B]["masks"] and not G[A]["slot64"] and not G[B]["slot64"] and G[C_]["slot64"] and not G[("B", K, 7700)]["masks"]
    assert 64 <= G[("A", K, 3000)]["CAP_S1"] <= 73 and not G[("A", K, 3000)]["legacy"] and G[("A", K, 3040)]["CAP_S1"] < 64 and G[("A", K, 3040)]["legacy"] and not G[A]["legacy"]
    assert ix.n_sess >= 131073 and ix.n_sess <= 400000
    # merge admission
    edge("admission: nruns = 8 merges", lambda l, g, r: r["nruns"] == 8 and mg(g, r))
    edge("admission: nruns = 9 does not", lambda l, g, r: r["nruns"] == 9 and r["sumw"] <= 63 and 2 * r["P"] + 64 <= g["wwords"] and not g["slot64"] and not mg(g, r))
    edge("admission: sumw = 63 merges", lambda l, g, r: r["sumw"] == 63 and mg(g, r))
    edge("admission: sumw = 64 does not", lambda l, g, r: r["sumw"] == 64 and r["nruns"] <= 8 and not g["slot64"] and not mg(g, r))
    for b in ("A", "B"):
        edge("admission: 2 P + 64 = wwords merges (batch %s)" % b, lambda l, g, r, b=b: l[0] == b and 2 * r["P"] + 64 == g["wwords"] and mg(g, r))
        edge("admission: 2 P + 64 = wwords + 2 does not (batch %s)" % b, lambda l, g, r, b=b: l[0] == b and 2 * r["P"] + 64 == g["wwords"] + 2 and r["nruns"] <= 8 and not mg(g, r))
    edge("admission: no merge mode on 64-bit slots", lambda l, g, r: g["slot64"] and r["nruns"] <= 8 and r["sumw"] <= 63 and 2 * r["P"] + 64 <= g["wwords"])
    # merge k-cut
    kf = lambda l, g, r: kcut_form(g, r, l[1], l[2]) if mg(g, r) else None   # noqa: E731
    edge("k-cut: Cm = k, every candidate a neighbour", lambda l, g, r: mg(g, r) and min(r["Call"], l[2]) == l[1])
    edge("k-cut: Cm = k + 1", lambda l, g, r: mg(g, r) and min(r["Call"], l[2]) == l[1] + 1)
    edge("k-cut: sumw = 15, packed class fields", lambda l, g, r: r["sumw"] == 15 and (kf(l, g, r) or "").startswith("packed"))
    edge("k-cut: sumw = 16, ballot loop", lambda l, g, r: r["sumw"] == 16 and (kf(l, g, r) or "").startswith("ballot"))
    edge("k-cut: Cm = 7680 at sumw <= 15, packed", lambda l, g, r: min(r["Call"], l[2]) == 7680 and (kf(l, g, r) or "").startswith("packed"))
    edge("k-cut: Cm = 7681 at sumw <= 15, ballot loop", lambda l, g, r: r["sumw"] <= 15 and min(r["Call"], l[2]) == 7681 and (kf(l, g, r) or "").startswith("ballot"))
    edge("k-cut: Cm = 3072, candidates in registers", lambda l, g, r: min(r["Call"], l[2]) == 3072 and (kf(l, g, r) or "").endswith("regs"))
    edge("k-cut: Cm = 3073, loop form", lambda l, g, r: min(r["Call"], l[2]) == 3073 and (kf(l, g, r) or "").endswith("loop"))
    edge("k-cut: the k-th best is the last of its class", lambda l, g, r: mg(g, r) and r["boundary"] is not None and r["boundary"]["taken"] == r["boundary"]["size"] and r["boundary"]["next"] < r["boundary"]["cls"])
    edge("k-cut: the k-th best is the first of its class", lambda l, g, r: mg(g, r) and r["boundary"] is not None and r["boundary"]["taken"] == 1 and r["boundary"]["size"] > 1)
    # m-cut
    for mm in (2500, 3000):
        for d in (0, 1):
            edge("m-cut: Call = m%+d, no list reaches m (m=%d)" % (d, mm), lambda l, g, r, mm=mm, d=d: l[2] == mm and r["xlo"] == 0 and r["Call"] == mm + d)
    for d in (0, 1):
        edge("m-cut: Call = m%+d, a list reaches m" % d, lambda l, g, r, d=d: r["xlo"] > 0 and r["Call"] == l[2] + d and r["nruns"] == 2)
    edge("m-cut: a list cut at m_index, m beyond it", lambda l, g, r: l[2] > M_INDEX and r["P"] == M_INDEX and r["xlo"] == 0)
    if tied:
        edge("tied: a tie group straddles the k-cut's boundary", lambda l, g, r: r["boundary"] is not None and r["boundary"]["cls"] == r["boundary"]["next"] and r["boundary"]["tied"])
    # hash bins (the hash mode's scan: SRN_NO_MERGE=1 for these queries)
    A2 = ("A", K, 3000)
    for d in (0, 1):
        edge("hash bins: the m-cut's boundary bin holds CAP_S1%+d sessions" % d, lambda l, g, r, d=d: l == A2 and not g["legacy"] and r["n1"] == g["CAP_S1"] + d and r["sh1"] == 7)
        edge("hash bins: the k-cut's boundary bin holds %d sessions at sh2 >= 8" % (128 + d), lambda l, g, r, d=d: not g["legacy"] and r["n2"] == 128 + d and r["sh2"] >= 8 and (r["n1"] is None or r["n1"] <= g["CAP_S1"]))
    for d in (0, 1):
        edge("hash bins: rank span %d, sh1 = %d, under an m-cut" % (2047 + d, d), lambda l, g, r, d=d: not g["legacy"] and r["n1"] is not None and r["rmax"] - r["xlo"] == 2047 + d and r["sh1"] == d)
    # session table
    edge("session table: distinct kept = sess_slots / 2, hash mode under SRN_NO_MERGE", lambda l, g, r: r["Call"] * 2 == g["sess_slots"] and sslots_of(g, r["P"]) == g["sess_slots"])
    edge("session table: distinct kept > sess_slots, the global-table pass", lambda l, g, r: not mg(g, r) and r["Call"] > g["sess_slots"])
    # item table (debug outputs on: every non-hot scored item is inserted)
    nh = lambda g, r: int((r["dense"] >= g["hot_slots"]).sum())   # noqa: E731
    edge("item table: non-hot scored <= item_slots / 2 at K >= 512", lambda l, g, r: r["K"] >= 512 and nh(g, r) * 2 <= g["item_slots"])
    edge("item table: non-hot scored > item_slots", lambda l, g, r: g["item_slots"] < nh(g, r) <= 2 * g["item_slots"])
    edge("item table: non-hot scored > 2 item_slots", lambda l, g, r: nh(g, r) > 2 * g["item_slots"])
    # rows
    for n in ROW_LENGTHS:
        edge("rows: a neighbour's row of %d items" % n, lambda l, g, r, n=n: r["K"] <= 64 and bool((r["row_lengths"] == n).any()))
    edge("rows: 64 neighbours, every row of 48 items", lambda l, g, r: r["K"] == 64 and bool((r["row_lengths"] == 48).all()))
    for n in (1, 64, 65, 512, 513):
        edge("rows: K = %d" % n, lambda l, g, r, n=n: r["K"] == n)
    # accumulators
    edge("accumulators: dense idx H - 1 scored", lambda l, g, r: g["hot_slots"] > 0 and bool((r["dense"] == g["hot_slots"] - 1).any()))
    edge("accumulators: dense idx H scored", lambda l, g, r: g["hot_slots"] > 0 and bool((r["dense"] == g["hot_slots"]).any()))
    edge("accumulators: the current item among the hot ones", lambda l, g, r: g["hot_slots"] > 0 and 0 <= r["cur_dense"] < g["hot_slots"])
    edge("accumulators: the current item beyond them", lambda l, g, r: g["hot_slots"] > 0 and r["cur_dense"] >= g["hot_slots"])
    edge("accumulators: no hot words at all (21 items, k = 1500)", lambda l, g, r: g["hot_slots"] == 0 and r["K"] > 0)
    # the two cells that had no edge of their own
    def one_score(r):
        valid = r["scored"] != r["cur"]
        cnt = np.diff(ix.l_off)[np.searchsorted(ix.l_items, r["scored"])]
        return bool(valid.sum() > 1 and len(set(r["acc"][valid].tolist())) == 1 and len(set(cnt[valid].tolist())) == 1)
    edge("top-n: 60 items with one score across the n-th place", lambda l, g, r: r["K"] == 2 and r["D"] == 61 and one_score(r))
    edge("rows: two items, every neighbour's row of 39 or 47 items", lambda l, g, r: r["nruns"] == 2 and r["K"] == 40 and sorted(set(r["row_lengths"].tolist())) == [39, 47])
    if tied:
        edge("tied: a group of eight across x_lo", lambda l, g, r: r["xlo"] > 1 and r["below_adjacent"] and ix.ts[r["xlo"] - 1] == ix.ts[r["xlo"]])
    # top-n
    for n in (64, 65):
        edge("top-n: %d scored items besides the current one" % n, lambda l, g, r, n=n: r["K"] == 3 and r["D"] == n + 1)
    edge("top-n: more scored items than the largest how_many", lambda l, g, r: r["D"] > max(HOW_MANY) + 1)
    edge("slot64: a session of 255 items", lambda l, g, r: r["L"] == 255 and g["slot64"] and g["num_bits"] == 15)
    missing = [name for name, c in hits.items() if c == 0]
    assert not missing, "edges that no query of the designed index hits: %s" % missing
    return hits


def family_counts():
    out = {}
    for c in cells():
        out[c["family"]] = out.get(c["family"], 0) + 1
    return out
