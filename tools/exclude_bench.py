"""What exclusion lists cost on the headline stream: config 3, the stream bench.py draws, one batch of `--batch` queries.  Arms, ALTERNATING in one
process, `--reps` times each:
  (a) plain       srn_predict_batch_device at how_many 21
  (b) wide        srn_predict_batch_device at how_many 21 + E                      (E = 8 and 16)
  (c) exclusion   srn_predict_batch_device_excl at how_many 21 with lists of E ids taken from each query's own row (positions spread over the wide row)
  filter          the filter kernel alone over (b)'s rows, from HIP events (srn_debug_exclude_filter)
  copy            a device-to-device copy of the bytes the filter reads plus writes, from HIP events in the same run
(b) - (a) is predict's own cost at a larger how_many; (c) - (b) is the filter, to be held against the copy.  Writes one JSON file.

    python tools/exclude_bench.py [--config cfg3] [--batch 1048576] [--reps 5] [--out profiles/exclude_cfg3.json]
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
    ap.add_argument("--excl", default="8,16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exclude_cfg3.json"))
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    B, how_many, max_len = a.batch, synth.HOW_MANY, synth.LAST_ITEMS
    qi, qo = synth.queries(int(B / 3.2 * 1.05) + 4096, n_items, seed=synth.SEED + 7919, max_items=max_len)
    if len(qo) - 1 < B:
        raise SystemExit("the stream holds %d queries, %d needed" % (len(qo) - 1, B))
    qo = qo[:B + 1]
    dev = torch.device("cuda:0")
    d_flat = torch.from_numpy(np.concatenate([qi[:qo[-1]], np.zeros(1, np.uint64)]).view(np.int64).copy()).to(dev)
    d_off = torch.from_numpy(qo.astype(np.int32)).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def rows(n):
        return (torch.empty(B * n, dtype=torch.int64, device=dev), torch.empty(B * n, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev))

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

    out = rows(how_many)
    plain = lambda n, o: sa.predict_batch_device(index, d_flat.data_ptr(), d_off.data_ptr(), B, max_len, k, m, n, False, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), stream)   # noqa: E731
    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "batch": B, "reps": a.reps, "runs": []}
    for E in [int(x) for x in a.excl.split(",")]:
        W = how_many + E
        wide = rows(W)
        plain(W, wide)
        torch.cuda.synchronize()
        cnt = wide[2].view(torch.int32).clamp(min=0, max=W).to(torch.int64)                      # (an unserved query's marker reads as -1)
        # E ids from each query's own wide row, spread over it: entry (j * W) // E of the row, a stranger where the row is shorter
        pos = (torch.arange(E, device=dev, dtype=torch.int64) * W) // E
        ids2 = wide[0].view(B, W)
        x_flat = torch.where(pos[None, :] < cnt[:, None], ids2[:, pos], torch.full((1, 1), 7, dtype=torch.int64, device=dev)).contiguous().view(-1)
        x_flat = torch.cat([x_flat, torch.zeros(1, dtype=torch.int64, device=dev)])
        x_off = (torch.arange(B + 1, device=dev, dtype=torch.int64) * E).to(torch.int32)
        excl = lambda: sa.predict_batch_device_excl(index, d_flat.data_ptr(), d_off.data_ptr(), B, max_len, x_flat.data_ptr(), x_off.data_ptr(), E, k, m, how_many, False,   # noqa: E731
                                                    out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream)
        filt = lambda: capi.check(capi.lib().srn_debug_exclude_filter(index._h, B, C.c_void_p(wide[0].data_ptr()), C.c_void_p(wide[1].data_ptr()), C.c_void_p(wide[2].data_ptr()), W,   # noqa: E731
                                                                      C.c_void_p(x_flat.data_ptr()), C.c_void_p(x_off.data_ptr()), E, None, None, how_many,
                                                                      C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), C.c_void_p(out[2].data_ptr()), C.c_void_p(stream)))
        # what the filter moves: the wide rows inside their counts and the counts, the lists and their offsets; the kept rows and their counts
        excl()
        torch.cuda.synchronize()
        kept = out[2].view(torch.int32).clamp(min=0, max=how_many).to(torch.int64)
        moved = int(cnt.sum().item()) * 16 + B * 4 + B * E * 8 + (B + 1) * 4 + int(kept.sum().item()) * 16 + B * 4
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)   # (a copy of n bytes reads n and writes n)
        copy = lambda: dst.copy_(src)   # noqa: E731
        row = {"E": E, "wide": W, "plain_ms": [], "wide_ms": [], "excl_ms": [], "filter_ms": [], "copy_ms": [], "filter_bytes": moved,
               "rows_changed": int((out[0].view(B, how_many)[:, 0] != ids2[:, 0]).sum().item())}
        for _ in range(a.reps):
            row["plain_ms"].append(round(timed(lambda: plain(how_many, out)), 4))
            row["wide_ms"].append(round(timed(lambda: plain(W, wide)), 4))
            row["excl_ms"].append(round(timed(excl), 4))
            row["filter_ms"].append(round(events(filt), 4))
            row["copy_ms"].append(round(events(copy), 4))
        med = lambda v: float(np.median(v))   # noqa: E731
        row["wide_minus_plain_ms"] = round(med(row["wide_ms"]) - med(row["plain_ms"]), 4)
        row["excl_minus_wide_ms"] = round(med(row["excl_ms"]) - med(row["wide_ms"]), 4)
        row["filter_over_copy"] = round(med(row["filter_ms"]) / med(row["copy_ms"]), 3)
        res["runs"].append(row)
        print(json.dumps(row), flush=True)
    index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
