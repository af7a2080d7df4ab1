"""From a click log to evaluated folds on the GPU: read the log's rows, split them by time, and run a walk-forward backtest.

    events = read_events("clicks.tsv")                         # three int64 tensors on the device (srn_events_from_tsv_gpu)
    sp = split_events(*events, cutoff=T)                       # Split(train, test, code, pos, info): srn_events_split + srn_events_take
    folds = backtest(events, trials, m=500, idf_weighting=1.0, folds=3, test_span=86400)

The split rule (include/serenade_hip.h, srn_events_split), in this order -- a later step sees only rows no earlier step dropped.  Times are rounded seconds
(floats as the file's: half away from zero, negative and nan -> 0; integers: negative -> 0) and every comparison is on them.
  1. last(s) = the largest time of any row of session s.  Sessions are never cut.
  2. OUT (16): every row of a session with last(s) < start, or with end > 0 and last(s) >= end.
  3. the other sessions are on the test side if last(s) >= cutoff, else on the train side.
  4. RARE (17): a train-side row whose item occurs in fewer than min_item_support train-side rows (rows, not sessions).
  5. SHORT_TRAIN (18): the remaining rows of a train session with fewer than min_session_len rows left.  One pass and no fixed point: an item's support
     may end up below min_item_support.
  6. TRAIN (1): what is left on the train side.
  7. UNKNOWN (19), with test_known_items: a test-side row whose item has no TRAIN row.
  8. SHORT_TEST (20): the remaining rows of a test session with fewer than min_session_len rows left.
  9. TEST (2): the rest.
pos is a TRAIN or TEST row's rank among the rows of its code (0xFFFFFFFF for the others).  split_model states the rule in NumPy and needs no GPU; the
device's code, pos and info are the model's, bit for bit.

backtest builds each fold's index with VMISIndex.from_events, which keeps read_from_file's quirk: the last row in session order -- and with it the last
session -- of the training side is dropped.  backtest does not compensate for it: a fold is what new_from_csv on the training file gives.

    python -m serenade_amd.prepare LOG --cutoff T [--start --end --min-item-support --min-session-len] --train-out A --test-out B

writes the two sides as TSV files (header, integer seconds) and prints info.  --device -1 runs the NumPy model on the host instead of the GPU.
"""
import collections
import ctypes as C

import numpy as np

from . import capi
from .ingest import _event_args, _is_torch

TRAIN, TEST, OUT, RARE, SHORT_TRAIN, UNKNOWN, SHORT_TEST = capi.SPLIT_TRAIN, capi.SPLIT_TEST, capi.SPLIT_OUT, capi.SPLIT_RARE, capi.SPLIT_SHORT_TRAIN, \
    capi.SPLIT_UNKNOWN, capi.SPLIT_SHORT_TEST
NO_POS = capi.SPLIT_NO_POS
INFO_FIELDS = tuple(n for n, _ in capi.SplitInfo._fields_)

Split = collections.namedtuple("Split", "train test code pos info")


def round_times(times):
    """The rounded seconds every comparison is made on -> uint64: floats half away from zero with negative and nan -> 0, integers with negative -> 0."""
    t = np.asarray(times)
    if np.issubdtype(t.dtype, np.floating):
        t = t.astype(np.float64)
        with np.errstate(invalid="ignore"):
            t = np.where(t >= 0, t, 0.0)
            r = np.trunc(t)
            r = r + (t - r >= 0.5)
            big = r >= 9223372036854775808.0
            return np.where(big, np.uint64(1 << 63), np.where(big, 0.0, r).astype(np.uint64))
    t = t.astype(np.int64, copy=False)
    return np.where(t < 0, 0, t).astype(np.uint64)


def _check_rule(cutoff, start, end, min_item_support, min_session_len):
    cutoff, start, end, S, L = int(cutoff), int(start), int(end), int(min_item_support), int(min_session_len)
    if cutoff <= 0:
        raise ValueError("cutoff must be > 0")
    if start < 0 or end < 0 or S < 0 or L < 0:
        raise ValueError("start, end, min_item_support and min_session_len must not be negative")
    if start and start >= cutoff:
        raise ValueError("start must be below cutoff")
    if end and end <= cutoff:
        raise ValueError("end must be above cutoff")
    return cutoff, start, end, max(S, 1), max(L, 1)


def split_model(session_ids, item_ids, times, cutoff, start=0, end=0, min_item_support=5, min_session_len=2, test_known_items=True):
    """The split rule on the host -> (code uint8[n], pos uint32[n], info dict with the fields of srn_split_info_t)."""
    cutoff, start, end, S, L = _check_rule(cutoff, start, end, min_item_support, min_session_len)
    sess = np.asarray(session_ids).astype(np.uint64, copy=False).reshape(-1)
    item = np.asarray(item_ids).astype(np.uint64, copy=False).reshape(-1)
    t = round_times(times).reshape(-1)
    n = len(sess)
    if n == 0 or len(item) != n or len(t) != n:
        raise ValueError("session_ids, item_ids and times must be of one length > 0")
    s_ids, s_of = np.unique(sess, return_inverse=True)
    i_ids, i_of = np.unique(item, return_inverse=True)
    s_of, i_of = s_of.reshape(-1), i_of.reshape(-1)
    last = np.zeros(len(s_ids), np.uint64)                                    # 1.
    np.maximum.at(last, s_of, t)
    s_out = (last < np.uint64(start)) | ((last >= np.uint64(end)) if end else np.zeros(len(last), bool))   # 2.
    s_test = ~s_out & (last >= np.uint64(cutoff))                             # 3.
    s_train = ~s_out & ~s_test
    code = np.zeros(n, np.uint8)
    code[s_out[s_of]] = OUT
    on_train, on_test = s_train[s_of], s_test[s_of]
    support = np.bincount(i_of[on_train], minlength=len(i_ids))               # 4.
    rare = on_train & (support[i_of] < S)
    code[rare] = RARE
    left = on_train & ~rare                                                   # 5.
    short = left & (np.bincount(s_of[left], minlength=len(s_ids))[s_of] < L)
    code[short] = SHORT_TRAIN
    train = left & ~short                                                     # 6.
    code[train] = TRAIN
    known = np.zeros(len(i_ids), bool)                                        # 7.
    known[i_of[train]] = True
    unknown = on_test & ~known[i_of] if test_known_items else np.zeros(n, bool)
    code[unknown] = UNKNOWN
    left = on_test & ~unknown                                                 # 8.
    short = left & (np.bincount(s_of[left], minlength=len(s_ids))[s_of] < L)
    code[short] = SHORT_TEST
    test = left & ~short                                                      # 9.
    code[test] = TEST
    pos = np.full(n, NO_POS, np.uint32)
    pos[train] = np.arange(int(train.sum()), dtype=np.uint32)
    pos[test] = np.arange(int(test.sum()), dtype=np.uint32)
    info = {"train_rows": int(train.sum()), "train_sessions": len(np.unique(s_of[train])), "train_items": len(np.unique(i_of[train])),
            "test_rows": int(test.sum()), "test_sessions": len(np.unique(s_of[test])), "test_items": len(np.unique(i_of[test])),
            "dropped_out": int((code == OUT).sum()), "dropped_rare": int((code == RARE).sum()), "dropped_short_train": int((code == SHORT_TRAIN).sum()),
            "dropped_unknown": int((code == UNKNOWN).sum()), "dropped_short_test": int((code == SHORT_TEST).sum()),
            "sessions": len(s_ids), "items": len(i_ids), "t_min": int(t.min()), "t_max": int(t.max())}
    return code, pos, info


def _device_of(arrs, device):
    for a in arrs:
        if _is_torch(a) and a.device.type == "cuda":
            return a.device.index if device is None else int(device)
    return 0 if device is None else int(device)


def _vp(p):
    return C.c_void_p(p)


def split_events(session_ids, item_ids, times, cutoff, start=0, end=0, min_item_support=5, min_session_len=2, test_known_items=True, device=None):
    """srn_events_split, then srn_events_take for both sides -> Split(train, test, code, pos, info); train and test are (session_ids, item_ids, times) of the
    TRAIN and the TEST rows in input order, times as given.  NumPy arrays in: NumPy arrays out (the rows go to GPU `device`, default 0, and come back).  Device
    tensors in: device tensors out, read in place on the current stream, nothing but the counts comes to the host; code is uint8, pos uint32."""
    cutoff, start, end, S, L = _check_rule(cutoff, start, end, min_item_support, min_session_len)
    device = _device_of((session_ids, item_ids, times), device)
    keep, (ps, pi, pt), n, flags, stream = _event_args(session_ids, item_ids, times, device)
    if n == 0:
        raise ValueError("no rows to split")
    rule = capi.Split(cutoff, start, end, S, L, capi.SPLIT_TEST_KNOWN_ITEMS if test_known_items else 0, 0)
    info = capi.SplitInfo()
    L_ = capi.lib()
    st = None if stream is None else _vp(stream)
    on_gpu = bool(flags & capi.EVENTS_DEVICE)
    if on_gpu:
        import torch
        dev = torch.device("cuda", device)
        code = torch.empty(n, dtype=torch.uint8, device=dev)
        pos = torch.empty(n, dtype=torch.uint32, device=dev)
        new = lambda like, m: torch.empty(m, dtype=like.dtype, device=dev)
        addr = lambda a: a.data_ptr()
    else:
        code, pos = np.empty(n, np.uint8), np.empty(n, np.uint32)
        new = lambda like, m: np.empty(m, like.dtype)
        addr = lambda a: a.ctypes.data
    capi.check(L_.srn_events_split(_vp(ps), _vp(pi), _vp(pt), n, flags, C.byref(rule), device, st, _vp(addr(code)), _vp(addr(pos)), C.byref(info)))
    sides = []
    for which, rows in ((TRAIN, info.train_rows), (TEST, info.test_rows)):
        out = tuple(new(a, int(rows)) for a in keep)
        if rows:
            capi.check(L_.srn_events_take(_vp(addr(code)), _vp(addr(pos)), n, which, _vp(ps), _vp(pi), _vp(pt), flags, _vp(addr(out[0])), _vp(addr(out[1])),
                                          _vp(addr(out[2])), device, st))
        sides.append(out)
    del keep
    return Split(sides[0], sides[1], code, pos, {f: int(getattr(info, f)) for f in INFO_FIELDS})


def read_events(path, device=0):
    """The rows of a TSV click log, parsed on the GPU as TrainingSessions.from_tsv(loader="gpu") parses them -> (session_ids, item_ids, times): three int64
    tensors on the device, in file order, times in rounded seconds."""
    import torch
    h = C.c_void_p()
    capi.check(capi.lib().srn_events_from_tsv_gpu(str(path).encode(), int(device), C.byref(h)))
    try:
        v = capi.EventsView()
        capi.check(capi.lib().srn_events_view(h, C.byref(v)))
        dev = torch.device("cuda", int(device))

        def column(ptr):
            if v.n == 0:
                return torch.empty(0, dtype=torch.int64, device=dev)

            class _Raw:   # a torch view of raw device memory: through the __cuda_array_interface__ protocol
                pass
            raw = _Raw()
            raw.__cuda_array_interface__ = {"shape": (int(v.n) * 8,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
            return torch.as_tensor(raw, device=dev).view(torch.int64).clone()
        out = (column(v.session_ids), column(v.item_ids), column(v.times))
        torch.cuda.synchronize(dev)
        return out
    finally:
        capi.lib().srn_events_free(h)


def _t_max(times):
    if _is_torch(times):
        import torch
        t = times
        if t.dtype == torch.float64:
            t = torch.where(t >= 0, t, torch.zeros((), dtype=t.dtype, device=t.device))
        return int(round_times(np.array([t.max().item()]))[0])
    return int(round_times(times).max())


def backtest(events, trials, m, idf_weighting, cutoffs=None, folds=None, test_span=86400, train_span=None, bootstrap=0, seed=0, ci=0.95, segments=None, builder="gpu", **split_kwargs):
    """Walk-forward evaluation of a click log.  events: (session_ids, item_ids, times), NumPy or device tensors; trials as evaluate() takes them; m and
    idf_weighting as VMISIndex.from_events takes them.  cutoffs: the folds' cutoffs; or folds=K: cutoff j = t_max + 1 - (K - j) * test_span, j = 0 .. K - 1.
    Per cutoff c: start = c - train_span (0 = all the past without train_span), end = c + test_span; split_events(..., **split_kwargs), VMISIndex.from_events
    on the training side, EvalSet.from_events on the test side and the training side's item column, evaluate(trials, bootstrap, seed, ci); the index and the set
    are closed again.  -> [{"cutoff", "start", "end", "info", "reports"}] in cutoff order.  With device tensors nothing but counts and reports leaves the GPU,
    except inside from_events with builder="gpu" (the default), which hands the grouped sessions to the index builder through the host and brings the built index
    down before attaching it; builder="resident" (VMISIndex.from_events) keeps all of that on the device -- same index, same reports.
    split_kwargs may also hold max_session_len (VMISIndex.from_events) and device.
    segments: evaluate()'s spec by position or by an item count -- every fold's reports then hold their "segments".  by="labels" is refused:
    a fold's session order is its own, so one label array cannot fit the folds."""
    from .evaluation import EvalSet, evaluate
    from .vmisknn import VMISIndex
    sess, items, times = events
    if segments is not None and segments.get("by") == "labels":
        raise ValueError("backtest takes no segments by labels: a fold's session order is its own")
    max_session_len = int(split_kwargs.pop("max_session_len", 0))
    device = _device_of(events, split_kwargs.pop("device", None))
    test_span = int(test_span)
    if test_span <= 0:
        raise ValueError("test_span must be > 0")
    if (cutoffs is None) == (folds is None):
        raise ValueError("give either cutoffs or folds")
    if cutoffs is None:
        K = int(folds)
        if K < 1:
            raise ValueError("folds must be >= 1")
        t_max = _t_max(times)
        cutoffs = [t_max + 1 - (K - j) * test_span for j in range(K)]
    out = []
    for c in cutoffs:
        c = int(c)
        start = max(c - int(train_span), 0) if train_span else 0
        sp = split_events(sess, items, times, c, start=start, end=c + test_span, device=device, **split_kwargs)
        index = VMISIndex.from_events(*sp.train, m, idf_weighting, max_session_len=max_session_len, device=device, builder=builder)
        try:
            es = EvalSet.from_events(index, sp.test, sp.train[1])
            try:
                reports = evaluate(es, trials, bootstrap=bootstrap, seed=seed, ci=ci, segments=segments)
            finally:
                es.close()
        finally:
            index.close()
        out.append({"cutoff": c, "start": start, "end": c + test_span, "info": sp.info, "reports": reports})
    return out


# ---- the command line ----
def parse_tsv_host(path):
    """The log's rows parsed in Python, for the host model: the header is skipped, and so is a line without two leading decimal ids and a time float() reads."""
    sess, items, times = [], [], []
    with open(path, "rb") as f:
        for k, line in enumerate(f):
            if k == 0:
                continue
            p = line.rstrip(b"\r\n").split(b"\t")
            if len(p) < 3 or not p[0].isdigit() or not p[1].isdigit():
                continue
            try:
                t = float(p[2])
            except ValueError:
                continue
            sess.append(int(p[0])); items.append(int(p[1])); times.append(t)
    return np.array(sess, np.uint64), np.array(items, np.uint64), np.array(times, np.float64)


def write_tsv(path, session_ids, item_ids, seconds):
    """"SessionId\\tItemId\\tTime" after a header, integer seconds."""
    cols = np.stack([np.asarray(a).astype(np.uint64, copy=False) for a in (session_ids, item_ids, seconds)], axis=1) if len(session_ids) else np.zeros((0, 3), np.uint64)
    with open(path, "wb") as f:
        f.write(b"SessionId\tItemId\tTime\n")
        np.savetxt(f, cols, fmt="%d", delimiter="\t")


def main(argv=None):
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="python -m serenade_amd.prepare", description="split a TSV click log by time into a training and a test file")
    ap.add_argument("log")
    ap.add_argument("--cutoff", type=int, required=True)
    ap.add_argument("--start", type=int, default=0)
    ap.add_argument("--end", type=int, default=0)
    ap.add_argument("--min-item-support", type=int, default=5)
    ap.add_argument("--min-session-len", type=int, default=2)
    ap.add_argument("--keep-unknown-items", action="store_true", help="keep test rows whose item has no training row")
    ap.add_argument("--device", type=int, default=0, help="the GPU; -1: the NumPy model on the host")
    ap.add_argument("--train-out", required=True)
    ap.add_argument("--test-out", required=True)
    a = ap.parse_args(argv)
    rule = dict(cutoff=a.cutoff, start=a.start, end=a.end, min_item_support=a.min_item_support, min_session_len=a.min_session_len, test_known_items=not a.keep_unknown_items)
    if a.device < 0:
        sess, items, times = parse_tsv_host(a.log)
        code, _, info = split_model(sess, items, times, **rule)
        secs = round_times(times)
        sides = [(sess[code == w], items[code == w], secs[code == w]) for w in (TRAIN, TEST)]
    else:
        sp = split_events(*read_events(a.log, a.device), device=a.device, **rule)
        info = sp.info
        sides = [tuple(x.cpu().numpy() for x in side) for side in (sp.train, sp.test)]
    write_tsv(a.train_out, *sides[0])
    write_tsv(a.test_out, *sides[1])
    print(json.dumps(info))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
