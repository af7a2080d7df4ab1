"""Snapshot, restore and resize of the device session store on one GPU, next to the yardstick of these bandwidth-bound passes: a device-to-device hipMemcpy of the
current table's bytes, taken in the same run, alternating with the pass it is compared with.

A store of --sessions live sessions (4 M; items_cap 16; the items are the clicks of config 3's query stream, 1 to 16 per session) is filled through import_entries, then
  export        srn_device_sessions_export_device into preallocated device arrays (HIP events)
  import        srn_device_sessions_import_device of those arrays into a fresh, empty store of the same shape (wall clock: the call blocks)
  resize x 2    srn_device_sessions_resize to twice the capacity, and back (wall clock: the call blocks; includes the allocation of the new pair and the free of the old)
  save / load   to --dir (default: the system's temporary directory), page cache warm (wall clock)
Every figure is a median over --reps repetitions after --warmup unrecorded ones, with the minimum and the maximum beside it.  The passes never read the index, so
config 3's index itself is only built with --with-index (a recommend_batch on the loaded store then checks that it serves).  Writes one JSON file.

    python tools/session_snapshot_bench.py [--sessions 4000000] [--reps 7] [--warmup 2] [--with-index] [--out profiles/session_snapshot_cfg3.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--sessions", type=int, default=4_000_000)
    ap.add_argument("--items-cap", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--with-index", action="store_true")
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_snapshot_cfg3.json"))
    a = ap.parse_args()
    import torch
    from serenade_amd import capi, synth
    from serenade_amd.serving import DeviceSessionStore

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    n, cap = a.sessions, a.items_cap
    rng = np.random.default_rng(17)
    qi, _ = synth.queries(1 << 16, n_items, seed=synth.SEED + 4201, max_items=1)
    ln = rng.integers(1, cap + 1, n).astype(np.uint32)
    items = np.resize(np.ascontiguousarray(qi, np.uint64), (n, cap))
    items[np.arange(cap)[None, :] >= ln[:, None]] = 0
    hi, lo = rng.integers(0, 2**63, n).astype(np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)   # lo: distinct
    now = 1_700_000_000
    epoch = (now - rng.integers(0, 1000, n)).astype(np.uint64)
    dev = torch.device("cuda:0")
    L, stream = capi.lib(), torch.cuda.current_stream().cuda_stream
    store = DeviceSessionStore(0, capacity=n, items_cap=cap)
    store.import_entries((hi, lo), epoch, ln, items)
    assert store.count(now).live == n
    st = store.stats
    table_bytes = st["slots"] * st["slot_bytes"]
    res = {"config": a.config, "sessions": n, "items_cap": cap, "slots": st["slots"], "slot_bytes": st["slot_bytes"], "table_bytes": table_bytes,
           "dense_bytes": n * (28 + 8 * cap), "reps": a.reps, "warmup": a.warmup}
    src, dst = torch.empty(table_bytes, dtype=torch.uint8, device=dev), torch.empty(table_bytes, dtype=torch.uint8, device=dev)
    src.zero_()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def copy_ms():
        ev0.record()
        dst.copy_(src)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    # export (device form), alternating with the copy
    t = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)] + [torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, cap), dtype=torch.int64, device=dev)]
    d_n = torch.zeros(1, dtype=torch.int64, device=dev)
    ptrs = [C.c_void_p(x.data_ptr()) for x in t]
    exp, cpy = [], []
    for rep in range(a.warmup + a.reps):
        ev0.record()
        capi.check(L.srn_device_sessions_export_device(store._h, now, n, *ptrs, cap, C.c_void_p(d_n.data_ptr()), C.c_void_p(stream)))
        ev1.record()
        ev1.synchronize()
        e, c = ev0.elapsed_time(ev1), copy_ms()
        if rep >= a.warmup:
            exp.append(e)
            cpy.append(c)
    assert int(d_n.item()) == n
    res["copy_table_d2d"] = dict(summary(cpy), GBps=round(2 * table_bytes / (statistics.median(cpy) * 1e-3) / 1e9, 1))
    res["export_device"] = dict(summary(exp), over_copy=round(statistics.median(exp) / statistics.median(cpy), 3))
    print(json.dumps({"copy_table_d2d": res["copy_table_d2d"], "export_device": res["export_device"]}), flush=True)

    # import of the exported arrays into an empty store of the same shape (a fresh store per repetition; its creation is not timed)
    imp, cpy = [], []
    for rep in range(a.warmup + a.reps):
        fresh = DeviceSessionStore(0, capacity=n, items_cap=cap)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        capi.check(L.srn_device_sessions_import_device(fresh._h, *ptrs, cap, n, C.c_void_p(stream)))
        w = (time.perf_counter() - t0) * 1e3
        c = copy_ms()
        if rep >= a.warmup:
            imp.append(w)
            cpy.append(c)
        if rep == 0:
            assert fresh.count(now).live == n
        fresh.close()
    res["import_device_into_empty"] = dict(summary(imp), over_copy=round(statistics.median(imp) / statistics.median(cpy), 3))
    print(json.dumps({"import_device_into_empty": res["import_device_into_empty"]}), flush=True)

    # resize to twice the capacity and back
    del src, dst
    up, down, cpy = [], [], []
    src, dst = torch.empty(table_bytes, dtype=torch.uint8, device=dev), torch.empty(table_bytes, dtype=torch.uint8, device=dev)
    src.zero_()
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        store.resize(2 * n, now=now)
        t1 = time.perf_counter()
        store.resize(n, now=now)
        t2 = time.perf_counter()
        c = copy_ms()
        if rep >= a.warmup:
            up.append((t1 - t0) * 1e3)
            down.append((t2 - t1) * 1e3)
            cpy.append(c)
    res["resize_x2"] = dict(summary(up), over_copy=round(statistics.median(up) / statistics.median(cpy), 3))
    res["resize_back"] = dict(summary(down), over_copy=round(statistics.median(down) / statistics.median(cpy), 3))
    print(json.dumps({"resize_x2": res["resize_x2"], "resize_back": res["resize_back"]}), flush=True)
    assert store.count(now).live == n

    # save / load, page cache warm
    path = os.path.join(a.dir, "session_snapshot_bench.%d.snap" % os.getpid())
    sv, ld, cpy = [], [], []
    try:
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            store.save(path, now=now)
            t1 = time.perf_counter()
            loaded = DeviceSessionStore.load(0, path)
            t2 = time.perf_counter()
            c = copy_ms()
            if rep >= a.warmup:
                sv.append((t1 - t0) * 1e3)
                ld.append((t2 - t1) * 1e3)
                cpy.append(c)
            if rep == 0:
                assert loaded.count(now).live == n
                if a.with_index:
                    import serenade_amd as sa
                    from serenade_amd.serving import recommend_batch
                    off, tr_items, ts = synth.training_sessions(inter, n_items)
                    index = sa.VMISIndex.from_sessions(off, tr_items, ts, m, 34, idfw, device=0, builder="gpu")
                    ids, cnt = recommend_batch(index, loaded, (hi[:4096], lo[:4096]), np.ascontiguousarray(qi[:4096], np.uint64), k=k, m=m, how_many=synth.HOW_MANY,
                                               max_items_in_session=cap, now=now)
                    res["served_after_load"] = {"requests": 4096, "rows_with_recommendations": int((cnt > 0).sum())}
                    index.close()
            loaded.close()
        res["file_bytes"] = os.path.getsize(path)
    finally:
        if os.path.exists(path):
            os.remove(path)
    res["save"] = dict(summary(sv), over_copy=round(statistics.median(sv) / statistics.median(cpy), 1), GBps=round(res["file_bytes"] / (statistics.median(sv) * 1e-3) / 1e9, 2))
    res["load"] = dict(summary(ld), over_copy=round(statistics.median(ld) / statistics.median(cpy), 1), GBps=round(res["file_bytes"] / (statistics.median(ld) * 1e-3) / 1e9, 2))
    print(json.dumps({"save": res["save"], "load": res["load"]}), flush=True)
    store.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
