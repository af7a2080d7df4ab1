"""Shared by the prep-record tests (test_gpu_ready_record.py, test_gpu_edge_cases.py, test_edge_cases_host.py) and by edge_cases.py: the record's layout, its legacy fields,
the launch-ready block recomputed from them, and ONE statement of where the launch sequence sends a query (`route_of`: the kernels' predicates of srn_fast.hip, on plain
integers; `routing` applies it to records).  Test-side only."""
import ctypes as C

import numpy as np

from helpers import flatten

HEAD_WORDS, READY0, READY_WORDS, ITEM_WORDS = 34, 18, 16, 6
MW_LEAN = 12032                  # F_LEAN_MW: words of the 53 KB layout's merge room
MW_BIG = 19072                   # ... and of the BIG form's 80 KB layout
LONG_RES_WORDS = 1536 * 2 + 2560 // 4 + 256   # F_LONG_RES_WORDS: the tail of the BIG layout's merge room that the LONG form reserves
K_NONE = 0xFFFFFFFF


def prep_records(gix, qs, m, max_len):
    """The prep kernel's records of a batch as u32 [nq, stride / 4]."""
    from serenade_amd import capi
    flat, off = flatten(qs)
    flat = np.concatenate([flat, np.zeros(1, np.uint64)])
    stride = C.c_size_t(0)
    out = np.zeros(len(qs) * (HEAD_WORDS + ITEM_WORDS * max_len), np.uint32)
    capi.check(capi.lib().srn_debug_prep_records(gix._h, C.c_void_p(flat.ctypes.data), C.c_void_p(off.ctypes.data), len(qs), m, max_len, C.c_void_p(out.ctypes.data), out.nbytes, C.byref(stride)))
    assert stride.value == 4 * (HEAD_WORDS + ITEM_WORDS * max_len) == 136 + 24 * max_len
    return out.reshape(len(qs), -1)


def legacy(rec, max_len):
    """The record's fields from before the block: head words and the items' (idx, kept, base)."""
    h = rec[:, :READY0].astype(np.int64)
    it = rec[:, HEAD_WORDS:].reshape(len(rec), max_len, ITEM_WORDS)
    return dict(rmax=h[:, 1], xlo=h[:, 2], sumw=h[:, 3], L=h[:, 6], n=h[:, 7], unsafe=h[:, 17], idx=it[:, :, 0], kept=it[:, :, 3].astype(np.int64), blo=it[:, :, 4], bhi=it[:, :, 5])


def ready_from_legacy(rec, wide, max_len):
    """The 16 words as srn_kernels.h defines them, from the legacy fields alone."""
    f = legacy(rec, max_len)
    out = np.zeros((len(rec), READY_WORDS), np.uint32)
    for q in range(len(rec)):
        L = int(f["L"][q])
        if not (1 <= L <= 8 and L <= max_len):
            continue
        runs = [p for p in range(L) if f["kept"][q, p] > 0]
        nr = len(runs)
        if nr > 4:
            continue
        rel = wide and nr > 3
        lean_ok = (f["unsafe"][q] == 0 and f["sumw"][q] <= 15 and 2 * f["n"][q] + 8 <= MW_LEAN and (not rel or f["rmax"][q] - f["xlo"][q] < (1 << 28)))
        out[q, 0] = int(lean_ok) | (nr << 8) | (int(rel) << 16)
        out[q, 2] = f["idx"][q, 0]
        for r, p in enumerate(runs):
            kept = int(f["kept"][q, p])
            out[q, 1] |= sum(1 << (5 * r + j) for j in range(5) if j * 512 < kept)
            out[q, 3] |= p << (8 * r)
            out[q, 4 + r] = kept
            out[q, 8 + 2 * r], out[q, 9 + 2 * r] = f["blo"][q, p], f["bhi"][q, p]
    return out


def route_of(L, n, sumw, span, nr, unsafe, max_len, wide=False):
    """Where the launch sequence sends ONE query, from plain integers and the kernels' predicates (srn_fast.hip): 'lean', 'big', 'mid', 'long', 'general'; the MID form's
    own hand-overs ('mid>big', 'mid>general') and the LONG form's ('long>general') included.  span = rmax - x_lo; nr = lists with kept > 0 (0 where L is outside 1..max_len)."""
    ok_len = 1 <= L <= max_len
    rel = wide and nr > 3
    if unsafe:
        return "general"
    if ok_len and L <= 8 and sumw <= 15 and nr <= 4 and 2 * n + 8 <= MW_LEAN and (not rel or span < (1 << 28)):
        return "lean"
    if ok_len and L <= 8 and sumw <= 15 and nr <= 4 and span < (1 << 28) and 2 * n + 8 + 256 <= MW_BIG:
        return "big"
    if ok_len and L <= 10:
        nb = max(nr, 4)
        shape = sumw <= 63 and nr <= 10 and span < (1 << (32 - nb))
        return "mid" if shape and 2 * n + 8 + 256 <= MW_LEAN else "mid>big" if shape and 2 * n + 8 + 256 <= MW_BIG else "mid>general"
    if ok_len and 10 < L <= 20:
        return "long" if sumw <= 255 and nr <= 20 and 2 * n + 8 + LONG_RES_WORDS <= MW_BIG and span < (1 << 27) else "long>general"
    return "general"


def routing(rec, max_len, wide=False):
    """route_of for every record of a batch, from the legacy fields."""
    f = legacy(rec, max_len)
    out = []
    for q in range(len(rec)):
        L = int(f["L"][q])
        nr = int((f["kept"][q, :L] > 0).sum()) if 1 <= L <= max_len else 0
        out.append(route_of(L, int(f["n"][q]), int(f["sumw"][q]), int(f["rmax"][q] - f["xlo"][q]), nr, int(f["unsafe"][q]), max_len, wide))
    return out
