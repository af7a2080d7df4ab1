"""What click feedback costs beside the batched /v1/recommend call: config 3, 2^20 requests per call, about four clicks per visitor in a batch with
a fifth of them repeating the click before (tools/recommend_bench.py's second key mix), max_items_in_session 2.  Arms, ALTERNATING in one process, `--reps` times each,
on two session stores driven with the same requests:
  (a) plain      recommend_batch on device tensors, without feedback= -- the code of the commit before the feature
  (b) feedback   the same call with feedback=: srn_recommend_batch_device and srn_feedback_observe_device on one stream
  observe        srn_feedback_observe_device alone over (a)'s rows, from HIP events
There is no gate: the numbers are recorded.  Writes one JSON file.

    python tools/feedback_bench.py [--config cfg3] [--requests 1048576] [--reps 5] [--out profiles/feedback_cfg3.json]

With --bootstrap it measures the visitor-clustered bootstrap of the log's counters instead (bootstrap_main below names the arms):

    python tools/feedback_bench.py --bootstrap [256 1024] [--reps 5] [--parent-lib PATH | --skip-parent] [--out profiles/feedback_bootstrap_cfg3.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bootstrap_main(a):
    """--bootstrap: what the visitor-clustered bootstrap of the log's counters costs.  recommend_batch(..., feedback=) on device tensors, each arm
    on a store and a log of its own, ALTERNATING in one process, medians of `--reps`:
      parent_off   the call through the parent commit's library (--parent-lib, loaded beside this one, with its own index): srn_recommend_batch_device and
                   srn_feedback_observe_device on one stream, its output rows cleared inside the timed region as recommend_batch hands out cleared ones
      off          this library, the bootstrap off: against parent_off it shows whether the existing path moved (`off_within_spread`: the medians differ by no
                   more than the larger of the two arms' min-max spreads)
      boot_<B>     this library with ClickFeedback(..., bootstrap=B), for each B (default 256 and 1024)
      pass alone   srn_feedback_observe_device alone over `off`'s rows from HIP events, with the bootstrap off and at each B: the differences are the fb_boot pass
    The logs of the boot arms must count what `off`'s log counts, and each arm's rows are `off`'s."""
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    from serenade_amd.serving import ClickFeedback, DeviceSessionStore, recommend_batch, session_keys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from harvest_bench import ParentLibrary

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, n, max_items = synth.HOW_MANY, a.requests, 2
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    if a.skip_parent:
        print("WARNING: --skip-parent: no arm runs the parent commit's library, so this run does not show whether the bootstrap-off path moved", file=sys.stderr, flush=True)
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
    clicks[order[same]] = clicks[order[same - 1]]
    dev = torch.device("cuda:0")
    hi, lo = (torch.from_numpy(x.view(np.int64)).to(dev) for x in session_keys(["visitor-%d" % v for v in vis]))
    t_its = [torch.from_numpy(np.roll(clicks, 7 * r).view(np.int64)).to(dev) for r in range(4)]
    Bs = [int(b) for b in a.bootstrap] or [256, 1024]
    arms = ["off"] + ["boot_%d" % b for b in Bs]
    stores = {x: DeviceSessionStore(index, capacity=12 * n, items_cap=8) for x in arms}
    fbs = {x: ClickFeedback(index, capacity=12 * n, row_cap=how_many, bootstrap=b, seed=1) for x, b in zip(arms, [0] + Bs)}
    alone = {x: ClickFeedback(index, capacity=12 * n, row_cap=how_many, bootstrap=b, seed=1) for x, b in zip(arms, [0] + Bs)}
    p_store, p_fb = (parent.store(12 * n, 8, 30 * 60, 20 * 60), parent.feedback(12 * n, how_many, 30 * 60, 20 * 60)) if parent else (None, None)
    p_out = (torch.zeros((n, how_many), dtype=torch.int64, device=dev), torch.zeros((n, how_many), dtype=torch.float64, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev))
    p_ranks = torch.zeros(n, dtype=torch.int32, device=dev)
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

    def parent_call(it, now, stream):
        for o in p_out + (p_ranks,):
            o.zero_()
        parent.recommend(p_index, p_store, hi, lo, it, now, max_items, k, m, how_many, p_out, stream)
        parent.observe(p_fb, hi, lo, it, now, p_out, how_many, p_ranks, stream)

    ms = {x: [] for x in (["parent_off"] if parent else []) + arms}
    alone_ms = {x: [] for x in arms}
    now, warm = 1_700_000_000, 3
    for rep in range(warm + a.reps):
        now += 60
        it = t_its[rep % len(t_its)]
        stream = torch.cuda.current_stream(0).cuda_stream
        if parent:
            tp = timed(lambda: parent_call(it, now, stream))[1]
        rows, t = {}, {}
        for x in arms:
            rows[x], t[x] = timed(lambda: recommend_batch(index, stores[x], (hi, lo), it, now=now, feedback=fbs[x], **kw))
            if not (torch.equal(rows[x][0], rows["off"][0]) and torch.equal(rows[x][1], rows["off"][1]) and torch.equal(fbs[x].last_ranks, fbs["off"].last_ranks)):
                raise SystemExit("%s: the rows or the ranks differ from the bootstrap-off arm's" % x)
        if parent and not (torch.equal(rows["off"][0], p_out[0]) and torch.equal(rows["off"][1], p_out[2]) and torch.equal(fbs["off"].last_ranks, p_ranks)):
            raise SystemExit("the rows or the ranks differ between the parent library and this one")
        ids, cnt, sc = rows["off"]
        ta = {x: events(lambda: alone[x].observe((hi, lo), it, None, ids, cnt, sc, now=now)) for x in arms}
        if rep >= warm:
            if parent:
                ms["parent_off"].append(round(tp, 4))
            for x in arms:
                ms[x].append(round(t[x], 4))
                alone_ms[x].append(round(ta[x], 4))
    med = lambda v: float(np.median(v))   # noqa: E731
    stats = {x: fbs[x].stats() for x in arms}
    for x in arms[1:]:
        if any(stats[x][c] != stats["off"][c] for c in ("requests", "observed", "hits_model", "hits_filled", "mrr", "hit_rate")):
            raise SystemExit("%s: the log's counters differ from the bootstrap-off arm's" % x)
    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "requests_per_call": n, "distinct_keys": int(len(np.unique(vis))), "reps": a.reps, "seed": 1,
           "parent_lib": bool(parent), "arms": {}, "observe_alone": {}}
    for x in ms:
        res["arms"][x] = {"wall_ms": ms[x], "wall_ms_median": round(med(ms[x]), 4), "wall_ms_spread": round(max(ms[x]) - min(ms[x]), 4)}
    for x in arms:
        res["observe_alone"][x] = {"event_ms": alone_ms[x], "event_ms_median": round(med(alone_ms[x]), 4)}
    if parent:
        res["off_minus_parent_ms"] = round(med(ms["off"]) - med(ms["parent_off"]), 4)
        res["off_minus_parent_by_rep_ms"] = [round(x - y, 4) for x, y in zip(ms["off"], ms["parent_off"])]   # (a rep's clicks differ from the previous rep's: the arms move together)
        res["off_within_spread"] = bool(abs(res["off_minus_parent_ms"]) <= max(res["arms"]["off"]["wall_ms_spread"], res["arms"]["parent_off"]["wall_ms_spread"]))
    for x, b in zip(arms[1:], Bs):
        st = stats[x]
        res["arms"][x].update({"minus_off_ms": round(med(ms[x]) - med(ms["off"]), 4), "over_off": round(med(ms[x]) / med(ms["off"]), 4),
                               "mrr": st["mrr"], "mrr_ci": list(st["mrr_ci"]), "hit_rate": st["hit_rate"], "hit_rate_ci": list(st["hit_rate_ci"]),
                               "empty_replicates": st["bootstrap"]["empty_replicates"]})
        res["observe_alone"][x]["boot_pass_ms"] = round(med(alone_ms[x]) - med(alone_ms["off"]), 4)
        res["observe_alone"][x]["weights_per_ns"] = round(n * b / (max(res["observe_alone"][x]["boot_pass_ms"], 1e-6) * 1e6), 2)   # (requests x replicates, reused weights counted)
    res["observed"] = stats["off"]["observed"]
    print(json.dumps(res), flush=True)
    if parent:
        parent.L.srn_device_sessions_free(p_store)
        parent.L.srn_feedback_free(p_fb)
        parent.L.srn_index_free(p_index)
    for o in list(stores.values()) + list(fbs.values()) + list(alone.values()):
        o.close()
    index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bootstrap", nargs="*", default=None, metavar="B", help="measure the visitor-clustered bootstrap instead (default B: 256 1024)")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "serenade_amd", "variants", "libserenade_hip_parent.so"), help="--bootstrap: the parent commit's library")
    ap.add_argument("--skip-parent", action="store_true", help="--bootstrap: no parent arm; the run then cannot tell whether the bootstrap-off call moved")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "feedback_bootstrap_cfg3.json" if a.bootstrap is not None else "feedback_cfg3.json")
    if a.bootstrap is not None:
        return bootstrap_main(a)
    import torch
    import serenade_amd as sa
    from serenade_amd import synth
    from serenade_amd.serving import ClickFeedback, DeviceSessionStore, recommend_batch, session_keys

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, n, max_items = synth.HOW_MANY, a.requests, 2
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    qi, _ = synth.queries(max(1024, n // 3), n_items, seed=synth.SEED + 4201, max_items=1)
    clicks = np.ascontiguousarray(np.resize(qi, n), np.uint64)
    rng = np.random.default_rng(11)
    vis = rng.integers(0, max(1, n // 4), n)                                         # about four clicks per visitor in a batch
    order = np.argsort(vis, kind="stable")
    same = np.flatnonzero((vis[order][1:] == vis[order][:-1]) & (rng.random(n - 1) < 0.2)) + 1
    clicks[order[same]] = clicks[order[same - 1]]                                    # a fifth of a visitor's clicks repeat the previous one
    hi, lo = session_keys(["visitor-%d" % v for v in vis])
    dev = torch.device("cuda:0")
    t_hi, t_lo = (torch.from_numpy(x.view(np.int64)).to(dev) for x in (hi, lo))
    t_its = [torch.from_numpy(np.roll(clicks, 7 * r).view(np.int64)).to(dev) for r in range(4)]   # a round's clicks differ from the previous round's: the sessions move
    stores = [DeviceSessionStore(index, capacity=4 * n, items_cap=8) for _ in range(2)]
    fb, fb_alone = (ClickFeedback(index, capacity=4 * n, row_cap=how_many) for _ in range(2))   # (the store's head room: the host's bound reaches the capacity every fourth call)
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

    st = fb.stats()
    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "requests_per_call": n, "distinct_keys": int(len(np.unique(vis))), "reps": a.reps,
           "log_slots": st["slots"], "log_slot_bytes": st["slot_bytes"], "log_table_bytes": st["slots"] * st["slot_bytes"],
           "plain_ms": [], "feedback_ms": [], "observe_alone_ms": []}
    now, warm = 1_700_000_000, 3                                                     # (workspaces grow, the sessions reach max_items_in_session items, the log fills)
    for rep in range(warm + a.reps):
        now += 60
        it = t_its[rep % len(t_its)]
        (ids, cnt, sc), plain = timed(lambda: recommend_batch(index, stores[0], (t_hi, t_lo), it, now=now, **kw))
        alone = events(lambda: fb_alone.observe((t_hi, t_lo), it, None, ids, cnt, sc, now=now))
        (ids2, cnt2, _), with_fb = timed(lambda: recommend_batch(index, stores[1], (t_hi, t_lo), it, now=now, feedback=fb, **kw))
        if not (torch.equal(ids, ids2) and torch.equal(cnt, cnt2) and torch.equal(fb.last_ranks, fb_alone.last_ranks)):
            raise SystemExit("the rows or the ranks differ between the arms")
        if rep >= warm:
            res["plain_ms"].append(round(plain, 4)); res["feedback_ms"].append(round(with_fb, 4)); res["observe_alone_ms"].append(round(alone, 4))
    med = lambda v: float(np.median(v))   # noqa: E731
    res["feedback_minus_plain_ms"] = round(med(res["feedback_ms"]) - med(res["plain_ms"]), 4)
    res["feedback_over_plain"] = round(med(res["feedback_ms"]) / med(res["plain_ms"]), 4)
    res["observe_alone_over_plain"] = round(med(res["observe_alone_ms"]) / med(res["plain_ms"]), 4)
    res["stats"] = fb.stats()
    print(json.dumps(res), flush=True)
    for o in stores + [fb, fb_alone]:
        o.close()
    index.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
