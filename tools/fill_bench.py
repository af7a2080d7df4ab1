"""What SRN_FLAG_FILL costs on the headline stream: config 3, the stream bench.py draws, one batch of `--batch` queries, a fallback ranking of the
`--ranking` most popular items.  Arms, ALTERNATING in one process, `--reps` times each:
  (a) plain        srn_predict_batch_device_excl at how_many 21 without the flag (= srn_predict_batch_device)
  (b) fill         the same call with SRN_FLAG_FILL on the headline stream (nearly every row is full: the kernel reads the counts and leaves)
  (c) fill_sparse  the same call with the flag on the stream with 10 % of its queries replaced by one unknown item each (empty rows: the whole row comes from the ranking)
  kernel           the fill kernel alone over (a)'s rows, from HIP events (srn_debug_fill): on the headline rows, and on the rows of the 10 % stream
  copy             a device-to-device copy of the counts array, from HIP events in the same run: the floor of the case without short rows
(b) - (a) is the feature's price where nothing is short.  Writes one JSON file.

    python tools/fill_bench.py [--config cfg3] [--batch 1048576] [--reps 5] [--ranking 256] [--out profiles/fill_cfg3.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranking", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fill_cfg3.json"))
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    index.set_fallback_popular(a.ranking)
    B, how_many, max_len = a.batch, synth.HOW_MANY, synth.LAST_ITEMS
    qi, qo = synth.queries(int(B / 3.2 * 1.05) + 4096, n_items, seed=synth.SEED + 7919, max_items=max_len)
    if len(qo) - 1 < B:
        raise SystemExit("the stream holds %d queries, %d needed" % (len(qo) - 1, B))
    qo = qo[:B + 1]
    # the second stream: every tenth query is one item the index does not know
    lens = np.diff(qo.astype(np.int64))
    lens[::10] = 1
    so = np.zeros(B + 1, np.uint32)
    so[1:] = np.cumsum(lens)
    si = np.zeros(int(so[-1]), np.uint64)
    keep = np.ones(B, bool)
    keep[::10] = False
    si[np.repeat(keep, lens)] = qi[:qo[-1]][np.repeat(keep, np.diff(qo.astype(np.int64)))]
    si[so[:-1][~keep]] = np.uint64(2**63) + np.arange((~keep).sum(), dtype=np.uint64)
    dev = torch.device("cuda:0")
    up = lambda flat, offs: (torch.from_numpy(np.concatenate([flat, np.zeros(1, np.uint64)]).view(np.int64).copy()).to(dev), torch.from_numpy(offs.astype(np.int32)).to(dev))   # noqa: E731
    head, sparse = up(qi[:qo[-1]], qo), up(si, so)
    stream = torch.cuda.current_stream().cuda_stream
    out = (torch.empty(B * how_many, dtype=torch.int64, device=dev), torch.empty(B * how_many, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    cnt_copy = torch.empty(B, dtype=torch.int32, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def call(q, fill):
        sa.predict_batch_device_excl(index, q[0].data_ptr(), q[1].data_ptr(), B, max_len, 0, 0, 0, k, m, how_many, False, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream,
                                     fill=fill)

    def kernel(q):
        capi.check(capi.lib().srn_debug_fill(index._h, B, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), C.c_void_p(out[2].data_ptr()), how_many, None, None,
                                             C.c_void_p(q[0].data_ptr()), C.c_void_p(q[1].data_ptr()), 0, C.c_void_p(stream)))

    def short_rows(q):
        call(q, False)
        torch.cuda.synchronize()
        c = out[2].view(torch.int32)
        return int(((c >= 0) & (c < how_many)).sum().item())

    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "batch": B, "reps": a.reps, "ranking": a.ranking,
           "short_rows_headline": short_rows(head), "short_rows_sparse": short_rows(sparse),
           "plain_ms": [], "fill_ms": [], "plain_sparse_ms": [], "fill_sparse_ms": [], "kernel_headline_ms": [], "kernel_sparse_ms": [], "copy_counts_ms": []}
    for _ in range(a.reps):
        res["plain_ms"].append(round(timed(lambda: call(head, False)), 4))
        res["kernel_headline_ms"].append(round(events(lambda: kernel(head)), 4))     # (over the rows the plain call just wrote)
        res["fill_ms"].append(round(timed(lambda: call(head, True)), 4))
        res["plain_sparse_ms"].append(round(timed(lambda: call(sparse, False)), 4))
        res["kernel_sparse_ms"].append(round(events(lambda: kernel(sparse)), 4))
        res["fill_sparse_ms"].append(round(timed(lambda: call(sparse, True)), 4))
        res["copy_counts_ms"].append(round(events(lambda: cnt_copy.copy_(out[2])), 4))
    med = lambda v: float(np.median(v))   # noqa: E731
    res["fill_minus_plain_ms"] = round(med(res["fill_ms"]) - med(res["plain_ms"]), 4)
    res["fill_sparse_minus_plain_sparse_ms"] = round(med(res["fill_sparse_ms"]) - med(res["plain_sparse_ms"]), 4)
    res["kernel_headline_over_copy"] = round(med(res["kernel_headline_ms"]) / med(res["copy_counts_ms"]), 3)
    print(json.dumps(res), flush=True)
    index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
