"""What click feedback costs beside the batched /v1/recommend call: config 3, 2^20 requests per call, about four clicks per visitor in a batch with
a fifth of them repeating the click before (tools/recommend_bench.py's second key mix), max_items_in_session 2.  Arms, ALTERNATING in one process, `--reps` times each,
on two session stores driven with the same requests:
  (a) plain      recommend_batch on device tensors, without feedback= -- the code of the commit before the feature
  (b) feedback   the same call with feedback=: srn_recommend_batch_device and srn_feedback_observe_device on one stream
  observe        srn_feedback_observe_device alone over (a)'s rows, from HIP events
There is no gate: the numbers are recorded.  Writes one JSON file.

    python tools/feedback_bench.py [--config cfg3] [--requests 1048576] [--reps 5] [--out profiles/feedback_cfg3.json]
"""
import argparse
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
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feedback_cfg3.json"))
    a = ap.parse_args()
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
