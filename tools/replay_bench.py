"""What a clock per request costs in the batched recommend path, on config 3, in one process with the arms ALTERNATING and medians of `--reps`.
recommend_batch on device tensors, 2^20 requests per call, about four clicks per visitor:
  (a) the untimed call
  (b) the timed call with all times equal (the same result as (a): what the timed kernels and the gather cost where nothing breaks)
  (c) the timed call over `--spread` seconds, sorted by time as a recorded log is: a visitor's clicks lie further apart than idle_secs, so runs break inside the call
  (d) (a) (b) (c) through the parent commit's library (--parent-lib, loaded beside this one through ctypes, with an index and stores of its own), each right before
      its namesake: an arm against its parent arm shows whether that path moved beyond the spread of the repeated runs (`<arm>_within_spread`: the medians differ by
      no more than the larger of the two arms' min-max spreads) -- the same kernels are enqueued.  A parent arm clears its output rows inside its timed region, as
      recommend_batch hands out cleared ones inside its own
  (e) the log of (c) served as it had to be before: one untimed call per distinct second (`--stepped-reps` runs, not alternated: each takes seconds)
and, with --feedback, (a) (b) (c) and their parent arms again with a click feedback log attached (feedback=; the parent's through srn_feedback_observe_device*).
There is no gate: the numbers are recorded.  Writes one JSON file.

    python tools/replay_bench.py [--config cfg3] [--requests 1048576] [--reps 5] [--spread 3600] [--parent-lib PATH | --skip-parent] [--out profiles/replay_cfg3.json]
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

from harvest_bench import ParentLibrary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stepped-reps", type=int, default=2)
    ap.add_argument("--spread", type=int, default=3600, help="seconds the log of (c) and (e) covers")
    ap.add_argument("--feedback", action="store_true", help="also measure (a) (b) (c) with a click feedback log attached")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "serenade_amd", "variants", "libserenade_hip_parent.so"))
    ap.add_argument("--skip-parent", action="store_true", help="leave out (d): the run then cannot tell whether the untimed path moved")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replay_cfg3.json"))
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    from serenade_amd.serving import ClickFeedback, DeviceSessionStore, recommend_batch, session_keys

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, n, max_items = synth.HOW_MANY, a.requests, 2
    off, items, ts = synth.training_sessions(inter, n_items)
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))   # noqa: E731
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else x.dtype)).to(dev)   # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    if a.skip_parent:
        print("WARNING: --skip-parent: no arm runs the parent commit's library, so this run does not show whether the untimed path moved", file=sys.stderr, flush=True)
        parent = None
    elif not os.path.exists(a.parent_lib):
        raise SystemExit("the parent commit's library %s is missing: build it from the parent commit and pass --parent-lib, or pass --skip-parent" % a.parent_lib)
    else:
        parent = ParentLibrary(a.parent_lib, capi)
    p_index = parent.index(off, items, ts, m, 34, idfw) if parent else None
    qi, _ = synth.queries(max(1024, n // 3), n_items, seed=synth.SEED + 4201, max_items=1)
    clicks = np.ascontiguousarray(np.resize(qi, n), np.uint64)
    rng = np.random.default_rng(11)
    n_vis = max(10, n // 4)
    vis = rng.integers(0, n_vis, n)                                                      # about four clicks per visitor in a batch
    hi, lo = (to_dev(x) for x in session_keys(["visitor-%d" % v for v in vis]))
    t_its = [to_dev(np.roll(clicks, 7 * r)) for r in range(4)]
    offsets = np.sort(rng.integers(0, a.spread, n)).astype(np.int64)                      # the log of (c): sorted by time
    seconds, first = np.unique(offsets, return_index=True)
    edges = np.concatenate([first, [n]])
    idle, ttl, step = 100, 10 ** 6, 60
    # a visitor's consecutive clicks in the log of (c): how many lie more than idle apart (the breaks inside runs of one call)
    by_vis = np.lexsort((np.arange(n), vis))
    same = vis[by_vis][1:] == vis[by_vis][:-1]
    breaks = int((same & (np.diff(offsets[by_vis]) > idle)).sum())
    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "requests_per_call": n, "reps": a.reps, "distinct_keys": int(len(np.unique(vis))), "idle_secs": idle,
           "spread_secs": a.spread, "distinct_seconds": int(len(seconds)), "breaks_inside_runs_per_call": breaks, "parent_lib": bool(parent)}
    kw = dict(k=k, m=m, how_many=how_many, max_items_in_session=max_items, scores=True)
    t_off = to_dev(offsets)

    for with_fb in ([False, True] if a.feedback else [False]):
        arms = ["untimed", "timed_equal", "timed_spread"]
        stores = {x: DeviceSessionStore(index, capacity=12 * n, items_cap=8, ttl_secs=ttl, idle_secs=idle) for x in arms}
        fbs = {x: ClickFeedback(index, capacity=12 * n, row_cap=how_many, ttl_secs=ttl, idle_secs=idle) if with_fb else None for x in arms}
        p_stores = {x: parent.store(12 * n, 8, ttl, idle) for x in arms} if parent else {}
        p_fbs = {x: parent.feedback(12 * n, how_many, ttl, idle) for x in arms} if parent and with_fb else {}
        p_out = (torch.zeros((n, how_many), dtype=torch.int64, device=dev), torch.zeros((n, how_many), dtype=torch.float64, device=dev),
                 torch.zeros(n, dtype=torch.int32, device=dev))
        p_ranks = torch.zeros(n, dtype=torch.int32, device=dev)
        ms = {x: [] for x in arms + (["parent_" + x for x in arms] if parent else [])}
        now, warm = 1_700_000_000, 3

        def parent_call(x, it, now, times, stream):   # what recommend_batch(..., feedback=) enqueues, through the parent's library
            for o in p_out + ((p_ranks,) if with_fb else ()):
                o.zero_()                                                                # (recommend_batch and observe hand out cleared rows: the fills belong to both arms' time)
            parent.recommend(p_index, p_stores[x], hi, lo, it, now, max_items, k, m, how_many, p_out, stream, times)
            if with_fb:
                parent.observe(p_fbs[x], hi, lo, it, now, p_out, how_many, p_ranks, stream, times)

        for rep in range(warm + a.reps):
            now += a.spread + step
            it = t_its[rep % len(t_its)]
            stream = torch.cuda.current_stream(0).cuda_stream
            times = {"untimed": None, "timed_equal": torch.full((n,), now, dtype=torch.int64, device=dev), "timed_spread": t_off + now}
            rows = {}
            for x in arms:                                                               # parent, this library, arm by arm
                if parent:
                    tp = timed(lambda: parent_call(x, it, now, times[x], stream))[1]
                rows[x], t = timed(lambda: recommend_batch(index, stores[x], (hi, lo), it, now=now, times=times[x], feedback=fbs[x], **kw))
                if parent and not (torch.equal(rows[x][0], p_out[0]) and torch.equal(rows[x][1], p_out[2]) and (not with_fb or torch.equal(fbs[x].last_ranks, p_ranks))):
                    raise SystemExit("%s: the rows%s differ between the parent library and this one" % (x, " or ranks" if with_fb else ""))
                if rep >= warm:
                    ms[x].append(round(t, 4))
                    if parent:
                        ms["parent_" + x].append(round(tp, 4))
            if not all(torch.equal(x, y) for x, y in zip(rows["untimed"], rows["timed_equal"])):
                raise SystemExit("the rows differ between the untimed call and the timed call with all times equal")
        r = {"ms": ms}
        for x in ms:
            r[x + "_ms"] = round(med(ms[x]), 4)
            r[x + "_spread_ms"] = round(max(ms[x]) - min(ms[x]), 4)
        r["timed_equal_minus_untimed_ms"] = round(med(ms["timed_equal"]) - med(ms["untimed"]), 4)
        r["timed_spread_minus_untimed_ms"] = round(med(ms["timed_spread"]) - med(ms["untimed"]), 4)
        if parent:   # an arm has not moved when the medians differ by no more than the larger of the two arms' own min-max spreads
            for x in arms:
                r[x + "_minus_parent_ms"] = round(med(ms[x]) - med(ms["parent_" + x]), 4)
                r[x + "_within_spread"] = bool(abs(r[x + "_minus_parent_ms"]) <= max(r[x + "_spread_ms"], r["parent_" + x + "_spread_ms"]))
            for h in p_stores.values():
                parent.L.srn_device_sessions_free(h)
            for h in p_fbs.values():
                parent.L.srn_feedback_free(h)
        if with_fb:
            r["feedback_idle_expired"] = {x: fbs[x].stats()["idle_expired"] for x in arms}
        res["with_feedback" if with_fb else "serving"] = r
        print(json.dumps({("with_feedback" if with_fb else "serving"): r}), flush=True)
        for o in list(stores.values()) + [f for f in fbs.values() if f is not None]:
            o.close()

    # (e) the log of (c), one untimed call per distinct second, against one timed call: the same rows
    it = t_its[0]
    stepped_ms, calls = [], len(seconds)
    for rep in range(a.stepped_reps):
        now = 1_700_000_000 + rep * (a.spread + step)
        ref_store = DeviceSessionStore(index, capacity=2 * n, items_cap=8, ttl_secs=ttl, idle_secs=idle)
        one_store = DeviceSessionStore(index, capacity=2 * n, items_cap=8, ttl_secs=ttl, idle_secs=idle)
        want = recommend_batch(index, one_store, (hi, lo), it, now=now, times=t_off + now, **kw)

        def stepped():
            return [recommend_batch(index, ref_store, (hi[x:y], lo[x:y]), it[x:y], now=now + int(s), **kw) for s, x, y in zip(seconds, edges, edges[1:])]
        rows, t = timed(stepped)
        stepped_ms.append(round(t, 2))
        if rep == 0 and not all(torch.equal(torch.cat([r_[i] for r_ in rows]), want[i]) for i in range(3)):
            raise SystemExit("the rows differ between one timed call and one untimed call per distinct second")
        ref_store.close(); one_store.close()
    res["stepped"] = {"calls": calls, "ms": stepped_ms, "stepped_ms": round(med(stepped_ms), 2) if stepped_ms else None,
                      "over_timed_spread": round(med(stepped_ms) / res["serving"]["timed_spread_ms"], 2) if stepped_ms else None}
    print(json.dumps({"stepped": res["stepped"]}), flush=True)
    if parent:
        parent.L.srn_index_free(p_index)
    index.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
