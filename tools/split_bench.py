"""What a traffic split costs beside the batched /v1/recommend call: config 3, 2^20 requests per call, about four clicks per visitor in a batch with
a fifth of them repeating the click before (tools/feedback_bench.py's key mix), max_items_in_session 2, device tensors.  Arms, ALTERNATING in one process, `--reps`
times each after three warm-up rounds, every arm on a session store of its own driven with the same requests:
  (a) plain        recommend_batch
  (b) parent       the same call through the parent commit's library (--parent-lib), loaded beside this one with an index of its own
  (c) one_arm      recommend_batch_split with a one-arm split: the shortcut
  (d) split_50_50 / split_90_10    two identical arms
  (e) parts_50_50 / parts_90_10    the same two sub-batches, partitioned beforehand, as two plain calls: what the arms themselves cost, the floor for (d)
  (f) front / scatter   assign + offsets + gather, and the scatter, alone from HIP events (srn_traffic_split_timing), beside a device-to-device copy of the bytes they move
Every arm's rows must be (a)'s.  There is no gate: the numbers are recorded.  Writes one JSON file.

    python tools/split_bench.py [--config cfg3] [--requests 1048576] [--reps 5] [--parent-lib PATH | --skip-parent] [--out profiles/traffic_split_cfg3.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traffic_split_cfg3.json"))
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "serenade_amd", "variants", "libserenade_hip_parent.so"), help="the parent commit's library")
    ap.add_argument("--skip-parent", action="store_true", help="no parent arm; the run then cannot tell whether the plain call moved")
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    from serenade_amd.serving import DeviceSessionStore, TrafficSplit, arms_model, recommend_batch, recommend_batch_split, session_keys
    from harvest_bench import ParentLibrary

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, n, max_items, seed = synth.HOW_MANY, a.requests, 2, 7
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    if a.skip_parent:
        print("WARNING: --skip-parent: no arm runs the parent commit's library, so this run does not show whether the plain call moved", file=sys.stderr, flush=True)
        parent = None
    elif not os.path.exists(a.parent_lib):
        raise SystemExit("the parent commit's library %s is missing: build it from the parent commit and pass --parent-lib, or pass --skip-parent" % a.parent_lib)
    else:
        parent = ParentLibrary(a.parent_lib, capi)
    p_index = parent.index(off, items, ts, m, 34, idfw) if parent else None
    qi, _ = synth.queries(max(1024, n // 3), n_items, seed=synth.SEED + 4201, max_items=1)
    clicks = np.ascontiguousarray(np.resize(qi, n), np.uint64)
    rng = np.random.default_rng(11)
    vis = rng.integers(0, max(1, n // 4), n)                                         # about four clicks per visitor in a batch
    order = np.argsort(vis, kind="stable")
    same = np.flatnonzero((vis[order][1:] == vis[order][:-1]) & (rng.random(n - 1) < 0.2)) + 1
    clicks[order[same]] = clicks[order[same - 1]]                                    # a fifth of a visitor's clicks repeat the previous one
    h_hi, h_lo = session_keys(["visitor-%d" % v for v in vis])
    dev = torch.device("cuda:0")
    hi, lo = (torch.from_numpy(x.view(np.int64)).to(dev) for x in (h_hi, h_lo))
    t_its = [torch.from_numpy(np.roll(clicks, 7 * r).view(np.int64)).to(dev) for r in range(4)]   # a round's clicks differ from the previous round's: the sessions move
    mixes = {"50_50": [1, 1], "90_10": [9, 1]}
    parts = {x: [torch.from_numpy(np.flatnonzero(arms_model(seed, w, (h_hi, h_lo)) == arm)).to(dev) for arm in (0, 1)] for x, w in mixes.items()}   # (e)'s partition, made beforehand
    names = ["plain"] + (["parent"] if parent else []) + ["one_arm"] + ["split_" + x for x in mixes] + ["parts_" + x for x in mixes]
    rounds = 3 + a.reps
    stores = {x: DeviceSessionStore(index, capacity=(rounds + 2) * n, items_cap=8) for x in names if x != "parent"}
    p_store = parent.store((rounds + 2) * n, 8, 30 * 60, 20 * 60) if parent else None
    p_out = (torch.zeros((n, how_many), dtype=torch.int64, device=dev), torch.zeros((n, how_many), dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    splits = {"one_arm": TrafficSplit(index, [1], seed=seed, max_batch=n, max_how_many=how_many)}
    for x, w in mixes.items():
        splits["split_" + x] = TrafficSplit(index, w, seed=seed, max_batch=n, max_how_many=how_many)
        splits["split_" + x].timing(True)
    arm = dict(index=index, k=k, m=m, max_items_in_session=max_items)
    kw = dict(k=k, m=m, how_many=how_many, max_items_in_session=max_items, scores=True)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    def events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def parent_call(it, now):
        for o in p_out:
            o.zero_()
        parent.recommend(p_index, p_store, hi, lo, it, now, max_items, k, m, how_many, p_out, torch.cuda.current_stream(0).cuda_stream)
        return p_out[0], p_out[2], p_out[1]

    def parts_call(x, it, now):
        """two plain calls over the partition made beforehand; the rows stay in arm order (putting them back is the split's scatter, measured in (f))"""
        return [recommend_batch(index, stores["parts_" + x], (hi[at], lo[at]), it[at], now=now, **kw) for at in parts[x]]

    # (f)'s copies: as many bytes read and written as the kernels move per request -- front: key_hi, key_lo, item and the 4-byte perm entry plus the arm byte;
    # scatter: a row's ids and scores, count, rank, perm entry and arm byte
    front_bytes, scatter_bytes = n * (3 * 8 + 4 + 1), n * (how_many * 16 + 4 + 4 + 4 + 1)
    src = torch.zeros(max(front_bytes, scatter_bytes), dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    ms = {x: [] for x in names}
    ev = {x: {"front_ms": [], "scatter_ms": []} for x in splits if x != "one_arm"}
    copies = {"front_copy_ms": [], "scatter_copy_ms": []}
    now = 1_700_000_000
    for rep in range(rounds):
        now += 60
        it = t_its[rep % len(t_its)]
        t = {}
        ref, t["plain"] = timed(lambda: recommend_batch(index, stores["plain"], (hi, lo), it, now=now, **kw))
        if parent:
            got, t["parent"] = timed(lambda: parent_call(it, now))
            if not all(torch.equal(x, y) for x, y in zip(got, ref)):
                raise SystemExit("the rows differ between the parent library and this one")
        for x in splits:
            n_arms = 1 if x == "one_arm" else 2
            got, t[x] = timed(lambda: recommend_batch_split(splits[x], [arm] * n_arms, stores[x], (hi, lo), it, how_many=how_many, now=now, scores=True))
            if not all(torch.equal(g, r) for g, r in zip(got, ref)):
                raise SystemExit("%s: the rows differ from the plain call's" % x)
        for x in mixes:
            got, t["parts_" + x] = timed(lambda: parts_call(x, it, now))
            if not all(torch.equal(g[0], ref[0][at]) and torch.equal(g[1], ref[1][at]) for g, at in zip(got, parts[x])):
                raise SystemExit("parts_%s: the rows differ from the plain call's" % x)
        c_front, c_scatter = events(lambda: dst[:front_bytes].copy_(src[:front_bytes])), events(lambda: dst[:scatter_bytes].copy_(src[:scatter_bytes]))
        if rep >= 3:
            for x in names:
                ms[x].append(round(t[x], 4))
            for x in ev:
                f_ms, s_ms = splits[x].last_ms()
                ev[x]["front_ms"].append(round(f_ms, 4)); ev[x]["scatter_ms"].append(round(s_ms, 4))
            copies["front_copy_ms"].append(round(c_front, 4)); copies["scatter_copy_ms"].append(round(c_scatter, 4))
    med = lambda v: float(np.median(v))   # noqa: E731
    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "requests_per_call": n, "distinct_keys": int(len(np.unique(vis))), "reps": a.reps, "seed": seed,
           "parent_lib": bool(parent), "arm_sizes": {x: [int(len(at)) for at in parts[x]] for x in mixes}, "arms": {}, "kernels": {}}
    for x in names:
        res["arms"][x] = {"wall_ms": ms[x], "wall_ms_median": round(med(ms[x]), 4), "wall_ms_spread": round(max(ms[x]) - min(ms[x]), 4)}
    if parent:
        res["plain_minus_parent_ms"] = round(med(ms["plain"]) - med(ms["parent"]), 4)
        res["plain_within_spread"] = bool(abs(res["plain_minus_parent_ms"]) <= max(res["arms"]["plain"]["wall_ms_spread"], res["arms"]["parent"]["wall_ms_spread"]))
    res["one_arm_minus_plain_ms"] = round(med(ms["one_arm"]) - med(ms["plain"]), 4)
    for x in mixes:
        res["split_minus_parts_ms_" + x] = round(med(ms["split_" + x]) - med(ms["parts_" + x]), 4)
        res["split_minus_plain_ms_" + x] = round(med(ms["split_" + x]) - med(ms["plain"]), 4)
        res["kernels"]["split_" + x] = {name: {"event_ms": v, "event_ms_median": round(med(v), 4)} for name, v in ev["split_" + x].items()}
    res["kernels"]["copies"] = {"front_bytes": front_bytes, "scatter_bytes": scatter_bytes,
                                **{name: {"event_ms": v, "event_ms_median": round(med(v), 4)} for name, v in copies.items()}}
    res["split_info"] = {x: {k_: v for k_, v in s.info().items() if k_ in ("served", "calls", "shortcut_calls", "device_bytes")} for x, s in splits.items()}
    print(json.dumps(res), flush=True)
    if parent:
        parent.L.srn_device_sessions_free(p_store)
        parent.L.srn_index_free(p_index)
    for o in list(stores.values()) + list(splits.values()):
        o.close()
    index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
