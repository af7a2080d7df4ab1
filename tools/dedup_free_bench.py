"""What the grouping pass of srn_dedup.hip costs where it buys nothing: the headline stream of bench.py (config 3, same seed) with ONE query kept per distinct item
sequence until the batch is full, served through srn_predict_batch_device and timed with HIP events; then, for comparison, the stream's first nq queries as they come
(the headline's batch 0).  The library is whatever SRN_LIB_PATH names (A/B against another build: run this twice); SRN_NO_DEDUP=1 in the environment switches the
pass off in this build.  Prints per batch: queries, distinct sequences, merged queries as the library counts them, ms per call (median and range over the calls).
usage: python tools/dedup_free_bench.py [cfg3] [nq] [calls]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import serenade_amd as sa
from serenade_amd import synth, capi

cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 10
inter, n_items, k, m, idfw = synth.CONFIGS[cfg]
L, n = synth.LAST_ITEMS, synth.HOW_MANY
off, items, ts = synth.training_sessions(inter, n_items)
ix = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, builder="gpu")
del off, items, ts

n_sess = int(B * 2 / 3.2) + 4096            # bench.py's draw for --batch B --pool 2
while True:
    qi, qo = synth.queries(n_sess, n_items, seed=synth.SEED + 7919, max_items=L)
    lens = np.diff(qo.astype(np.int64))
    a = np.zeros((len(lens), L + 1), np.uint64)
    a[:, 0] = lens
    for j in range(L):
        has = lens > j
        a[has, 1 + j] = qi[qo[:-1].astype(np.int64)[has] + j]
    _, first = np.unique(a, axis=0, return_index=True)
    if len(first) >= B:
        break
    n_sess = int(n_sess * 1.5)              # (the same seed: a longer stream starts with the shorter one)
keep = np.sort(first)[:B]                    # the first occurrence of each distinct sequence, in stream order


def csr(rows):
    ln = lens[rows]
    o = np.zeros(len(rows) + 1, np.int64)
    o[1:] = np.cumsum(ln)
    src = np.repeat(qo[:-1].astype(np.int64)[rows], ln) + (np.arange(o[-1]) - np.repeat(o[:-1], ln))
    return qi[src], o.astype(np.uint32)


has_counter = hasattr(capi.lib(), "srn_debug_last_dedup_count")
dev = torch.device("cuda:0")
stream = torch.cuda.current_stream()
for name, rows in (("one query per distinct sequence", keep), ("the stream as it comes (headline batch 0)", np.arange(B))):
    f, o = csr(rows)
    distinct = len(np.unique(a[rows], axis=0))
    d_flat = torch.from_numpy(f.view(np.int64).copy()).to(dev)
    d_off = torch.from_numpy(o.view(np.int32).copy()).to(dev)
    out = (torch.zeros(B * n, dtype=torch.int64, device=dev), torch.zeros(B * n, dtype=torch.float64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    sa.reserve(ix, B, L, k, m, n, False, stream.cuda_stream)
    run = lambda: sa.predict_batch_device(ix, d_flat.data_ptr(), d_off.data_ptr(), B, L, k, m, n, False, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream.cuda_stream)   # noqa: E731
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):                   # (one call at a time: nothing of a neighbouring call overlaps the timed one)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream); run(); e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    merged = ix.last_dedup_count() if has_counter else -1
    print("%s %d: %s: %d queries, %d distinct, %d merged by the library; ms per call median %.4f (min %.4f, max %.4f over %d calls)"
          % (cfg, B, name, B, distinct, merged, float(np.median(ms)), min(ms), max(ms), calls), flush=True)
