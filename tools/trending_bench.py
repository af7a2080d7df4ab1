"""Trending items on one GPU: DeviceSessionStore.top_items and VMISIndex.set_fallback_trending on a store of live sessions whose items follow the training data's own
popularity, timed in one process beside what they replace and what bounds them --
  (1) top_items(n = 256): count and rank on the device (srn_trending.hip);
  (2) set_fallback_trending(n = 256): (1) + the popularity tail + srn_index_set_fallback;
  (3) a device-to-device copy of the table's bytes: what one pass over the table costs;
  (4) export() of the whole store to the host, and (5) serving.top_items_model, the NumPy rule, on the exported arrays: the round trip (1) removes.
There is no gate: the numbers are recorded.  Writes one JSON file.

    python tools/trending_bench.py [--config cfg3] [--sessions 4194304] [--items-cap 16] [--reps 5] [--out profiles/trending_cfg3.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, sync):
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        r = fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return r, [round(x, 3) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--sessions", type=int, default=1 << 22)
    ap.add_argument("--items-cap", type=int, default=16)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=1 << 20, help="entries per import call")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trending_cfg3.json"))
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import synth
    from serenade_amd.serving import DeviceSessionStore, top_items_model

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    n, cap, now = a.sessions, a.items_cap, 1_700_000_000
    ttl = 1800
    store = DeviceSessionStore(index, capacity=n, items_cap=cap, ttl_secs=ttl, idle_secs=1200)
    # the windows: every position a uniformly drawn event of the training data, so an item's share is its share of the clicks; lengths 1..items_cap; epochs inside the TTL
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    train = torch.from_numpy(np.ascontiguousarray(items, np.uint64).view(np.int64)).to(dev)
    for at in range(0, n, a.chunk):
        c = min(a.chunk, n - at)
        it = train[torch.randint(0, train.numel(), (c, cap), device=dev, generator=g)]
        ln = torch.randint(1, cap + 1, (c,), device=dev, generator=g, dtype=torch.int32)
        hi = torch.randint(0, 2**62, (c,), device=dev, generator=g)
        lo = torch.arange(at, at + c, device=dev, dtype=torch.int64)
        ep = now - torch.randint(0, ttl, (c,), device=dev, generator=g)
        store.import_entries((hi, lo), ep, ln, it)
    sync()
    del train
    st = store.stats
    res = {"config": a.config, "sessions": n, "items_cap": cap, "n": a.n, "live": store.count(now).live, "slots": st["slots"], "slot_bytes": st["slot_bytes"],
           "table_bytes": st["slots"] * st["slot_bytes"], "n_items_index": int(index.info["n_items"])}
    (ids, counts), ms = timed(lambda: store.top_items(a.n, now=now), a.reps, sync)
    res["1_top_items_ms"] = ms
    trending, ms = timed(lambda: index.set_fallback_trending(store, a.n, now=now), a.reps, sync)
    res["2_set_fallback_trending_ms"], res["2_trending_entries"] = ms, trending
    src = torch.empty(res["table_bytes"], dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    _, ms = timed(lambda: dst.copy_(src), a.reps, sync)
    res["3_table_copy_d2d_ms"] = ms
    res["3_table_copy_gb_per_s"] = round(2 * res["table_bytes"] / (min(ms) * 1e-3) / 1e9, 1)     # (read + write)
    del src, dst
    exported, ms = timed(lambda: store.export(now=now), 1, sync)
    res["4_export_to_host_ms"] = ms
    _, ep, ln, it = exported
    (m_ids, m_counts), ms = timed(lambda: top_items_model(ln, it, ep, a.n, now, ttl), 1, sync)
    res["5_numpy_model_ms"] = ms
    res["equal_to_model"] = bool(np.array_equal(ids, m_ids) and np.array_equal(counts, m_counts))
    res["top_counts"] = [int(c) for c in counts[:8]]
    res["1_over_3"] = round(min(res["1_top_items_ms"]) / min(res["3_table_copy_d2d_ms"]), 2)
    res["4_plus_5_over_1"] = round((res["4_export_to_host_ms"][0] + res["5_numpy_model_ms"][0]) / min(res["1_top_items_ms"]), 1)
    store.close()
    index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not res["equal_to_model"]:
        raise SystemExit("top_items differs from the NumPy model")


if __name__ == "__main__":
    main()
