"""What the session harvest costs, on config 3, in one process with the arms ALTERNATING and medians of `--reps`:
  serving   recommend_batch on device tensors, 2^20 requests per call, about four clicks per visitor, `now` advancing so that 0 % and about 10 % of the run heads
            return after idle.  Arms: (p) the parent commit's library (--parent-lib, built with build.build_variant or kept from the commit before; loaded beside this
            one through ctypes, with an index and a store of its own), (d) this library with the harvest detached, (a) attached.  (p) against (d) shows whether the
            untouched path moved beyond the spread of the repeated runs; (a) over (d) is the harvest's cost.
  sweep     store.sweep at 4 M stored sessions, with and without a harvest, where it drops nothing and where it drops everything, beside a device-to-device copy
            of the table
  refresh   hv.events + refreshed_index on config 3's events plus 1 M harvested sessions, beside VMISIndex.from_events on the base alone
There is no gate: the numbers are recorded.  Writes one JSON file.

    python tools/harvest_bench.py [--config cfg3] [--requests 1048576] [--reps 5] [--parent-lib PATH | --skip-parent] [--out profiles/harvest_cfg3.json]
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


class ParentLibrary:
    """The few entry points the serving arm needs, bound on another build of the library: an index from the same sessions, a store, the batch call."""
    NAMES = ("srn_index_build_gpu", "srn_index_free", "srn_device_sessions_create", "srn_device_sessions_free", "srn_recommend_batch_device", "srn_last_error")
    NEWER = ("srn_recommend_batch_device_at", "srn_feedback_create", "srn_feedback_free", "srn_feedback_observe_device", "srn_feedback_observe_device_at")   # bound where the build has them

    def __init__(self, path, capi):
        self.L = C.CDLL(path)
        for name in self.NAMES + tuple(x for x in self.NEWER if hasattr(self.L, x)):
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        self.capi = capi

    def check(self, rc):
        if rc:
            raise RuntimeError("parent library: %d %s" % (rc, self.L.srn_last_error().decode(errors="replace")))

    def index(self, off, items, ts, m, max_len, idfw):
        capi = self.capi
        off, items, ts = capi.as_u64(off), capi.as_u64(items), capi.as_u32(ts)
        v = capi.SessionsView(off.ctypes.data, items.ctypes.data, ts.ctypes.data, len(ts))
        h = C.c_void_p()
        self.check(self.L.srn_index_build_gpu(C.byref(v), m, max_len, idfw, 0, C.byref(h)))
        return h

    def store(self, capacity, items_cap, ttl, idle):
        h = C.c_void_p()
        self.check(self.L.srn_device_sessions_create(0, capacity, items_cap, ttl, idle, C.byref(h)))
        return h

    def recommend(self, index, store, hi, lo, it, now, max_items, k, m, how_many, out, stream, times=None):
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        args = [index, store, p(hi), p(lo), p(it), None, len(it), now, max_items, k, m, how_many, 0, p(out[0]), p(out[1]), p(out[2]), C.c_void_p(stream)]
        if times is not None:
            args.insert(6, p(times))
        self.check((self.L.srn_recommend_batch_device if times is None else self.L.srn_recommend_batch_device_at)(*args))

    def feedback(self, capacity, row_cap, ttl, idle):
        h = C.c_void_p()
        self.check(self.L.srn_feedback_create(0, capacity, row_cap, ttl, idle, C.byref(h)))
        return h

    def observe(self, fb, hi, lo, it, now, out, how_many, ranks, stream, times=None):
        """the rows `out` = (ids, scores, counts) just served to the requests, as recommend_batch(..., feedback=) hands them on"""
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        args = [fb, p(hi), p(lo), p(it), None, len(it), now, p(out[0]), p(out[1]), p(out[2]), how_many, p(ranks), C.c_void_p(stream)]
        if times is not None:
            args.insert(5, p(times))
        self.check((self.L.srn_feedback_observe_device if times is None else self.L.srn_feedback_observe_device_at)(*args))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep-sessions", type=int, default=4_000_000)
    ap.add_argument("--harvested", type=int, default=1_000_000)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "serenade_amd", "variants", "libserenade_hip_parent.so"))
    ap.add_argument("--skip-parent", action="store_true", help="run the serving part without the parent commit's library: it then cannot tell whether the detached path moved")
    ap.add_argument("--skip", default="", help="comma-separated parts to leave out: serving, sweep, refresh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "harvest_cfg3.json"))
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    from serenade_amd.serving import DeviceSessionStore, SessionHarvest, recommend_batch, refreshed_index, session_keys

    skip = set(x for x in a.skip.split(",") if x)
    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, n, max_items = synth.HOW_MANY, a.requests, 2
    off, items, ts = synth.training_sessions(inter, n_items)
    dev = torch.device("cuda:0")
    med = lambda v: float(np.median(v))   # noqa: E731
    to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else np.int32 if x.dtype == np.uint32 else x.dtype)).to(dev)   # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3

    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "requests_per_call": n, "reps": a.reps}

    if "serving" not in skip:
        index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
        if a.skip_parent:
            print("WARNING: --skip-parent: no arm runs the parent commit's library, so this run does not show whether the detached path moved", file=sys.stderr, flush=True)
            parent = None
        elif not os.path.exists(a.parent_lib):
            raise SystemExit("the parent commit's library %s is missing: build it from the parent commit (build.build_hip there, or build.build_variant) and pass "
                             "--parent-lib, or pass --skip-parent to measure only detached against attached" % a.parent_lib)
        else:
            parent = ParentLibrary(a.parent_lib, capi)
        p_index = parent.index(off, items, ts, m, 34, idfw) if parent else None
        qi, _ = synth.queries(max(1024, n // 3), n_items, seed=synth.SEED + 4201, max_items=1)
        clicks = np.ascontiguousarray(np.resize(qi, n), np.uint64)
        rng = np.random.default_rng(11)
        n_vis = max(10, n // 4)
        vis = rng.integers(0, n_vis, n)                                                  # about four clicks per visitor in a batch
        t_its = [to_dev(np.roll(clicks, 7 * r)) for r in range(4)]
        idle, ttl, step = 100, 10 ** 6, 60
        # a tenth of the visitors come from one of two groups that take turns: a member is back every second call, 120 s > idle after its last click
        rotating = vis < n_vis // 10
        names = [["visitor-%d%s" % (v, "-g%d" % g if r else "") for v, r in zip(vis, rotating)] for g in range(2)]
        keysets = [tuple(to_dev(x) for x in session_keys(nm)) for nm in names]
        res["serving"] = {"distinct_keys": int(len(np.unique(vis))), "rotating_keys": int(len(np.unique(vis[rotating]))), "idle_secs": idle, "step_secs": step,
                          "parent_lib": bool(parent)}
        kw = dict(k=k, m=m, how_many=how_many, max_items_in_session=max_items, scores=True)
        for mode in ("no_returns", "tenth_returns"):
            stores = [DeviceSessionStore(index, capacity=12 * n, items_cap=8, ttl_secs=ttl, idle_secs=idle) for _ in range(2)]
            hv = SessionHarvest(index, capacity=2_000_000, items_cap=8, min_len=1)
            stores[1].set_harvest(hv)
            p_store = parent.store(12 * n, 8, ttl, idle) if parent else None
            p_out = (torch.zeros((n, how_many), dtype=torch.int64, device=dev), torch.zeros((n, how_many), dtype=torch.float64, device=dev),
                     torch.zeros(n, dtype=torch.int32, device=dev))
            ms = {"parent": [], "detached": [], "attached": []}
            now, warm = 1_700_000_000, 3
            for rep in range(warm + a.reps):
                now += step
                hi, lo = keysets[rep % 2 if mode == "tenth_returns" else 0]
                it = t_its[rep % len(t_its)]
                stream = torch.cuda.current_stream(0).cuda_stream
                def parent_call():   # (recommend_batch hands out cleared rows: the fills belong to both arms' time, and a row's tail beyond its count must not be the previous call's)
                    for o in p_out:
                        o.zero_()
                    parent.recommend(p_index, p_store, hi, lo, it, now, max_items, k, m, how_many, p_out, stream)
                tp = timed(parent_call)[1] if parent else None
                (ids, cnt, sc), td = timed(lambda: recommend_batch(index, stores[0], (hi, lo), it, now=now, **kw))
                (ids2, cnt2, sc2), ta = timed(lambda: recommend_batch(index, stores[1], (hi, lo), it, now=now, **kw))
                if not (torch.equal(ids, ids2) and torch.equal(cnt, cnt2) and torch.equal(sc, sc2)):
                    raise SystemExit("the rows differ between the detached and the attached arm")
                if parent and not (torch.equal(ids, p_out[0]) and torch.equal(cnt, p_out[2])):
                    raise SystemExit("the rows differ between the parent library and this one")
                if rep >= warm:
                    ms["detached"].append(round(td, 4)); ms["attached"].append(round(ta, 4))
                    if parent:
                        ms["parent"].append(round(tp, 4))
            st = hv.stats()
            r = {"ms": ms, "detached_ms": round(med(ms["detached"]), 4), "attached_ms": round(med(ms["attached"]), 4),
                 "attached_minus_detached_ms": round(med(ms["attached"]) - med(ms["detached"]), 4), "attached_over_detached": round(med(ms["attached"]) / med(ms["detached"]), 4),
                 "harvest": {x: st[x] for x in ("stored", "lost", "from_return", "from_rebuild", "skipped_short")}}
            if parent:
                r["parent_ms"] = round(med(ms["parent"]), 4)
                r["parent_spread_ms"] = round(max(ms["parent"]) - min(ms["parent"]), 4)
                r["detached_minus_parent_ms"] = round(med(ms["detached"]) - med(ms["parent"]), 4)
                parent.L.srn_device_sessions_free(p_store)
            res["serving"][mode] = r
            print(json.dumps({mode: r}), flush=True)
            for o in (hv, *stores):
                o.close()
        if parent:
            parent.L.srn_index_free(p_index)
        index.close()

    T0 = 1_700_000_000
    if "sweep" not in skip:
        ns, ttl = a.sweep_sessions, 1800
        rng = np.random.default_rng(12)
        e_hi, e_lo = to_dev(rng.integers(0, 2 ** 63, ns, dtype=np.uint64)), to_dev(np.arange(1, ns + 1, dtype=np.uint64))
        e_len = to_dev(rng.integers(1, 9, ns).astype(np.uint32))
        e_items = to_dev(rng.integers(1, n_items, (ns, 8)).astype(np.uint64))
        e_ep = torch.full((ns,), T0, dtype=torch.int64, device=dev)
        stores = [DeviceSessionStore(0, capacity=ns + ns // 8, items_cap=8, ttl_secs=ttl, idle_secs=1200) for _ in range(2)]
        hv = SessionHarvest(0, capacity=ns, items_cap=8, min_len=1)
        stores[1].set_harvest(hv)
        st = stores[0].stats
        table = torch.zeros(st["slots"] * st["slot_bytes"] // 8, dtype=torch.int64, device=dev)
        ms = {"keep_detached": [], "keep_attached": [], "drop_detached": [], "drop_attached": [], "table_copy": []}
        for rep in range(1 + a.reps):
            for s in stores:
                s.import_entries((e_hi, e_lo), e_ep, e_len, e_items)
            hv.clear()
            t = [timed(lambda s=s: s.sweep(T0 + 1))[1] for s in stores]                  # nothing is old: flags and a scan over the slots, no copy
            u = [timed(lambda s=s: s.sweep(T0 + ttl + 1))[1] for s in stores]            # everything is old: every session is copied to the log
            c = timed(lambda: table.clone())[1]
            if rep >= 1:
                for name, v in zip(ms, t + u + [c]):
                    ms[name].append(round(v, 4))
        r = {"sessions": ns, "slots": st["slots"], "slot_bytes": st["slot_bytes"], "table_bytes": st["slots"] * st["slot_bytes"], "ms": ms, "harvest": hv.stats()}
        r.update({name + "_ms": round(med(v), 4) for name, v in ms.items()})
        res["sweep"] = r
        print(json.dumps({"sweep": r}), flush=True)
        for o in (hv, *stores):
            o.close()
        del table, e_hi, e_lo, e_len, e_items, e_ep

    if "refresh" not in skip:
        nh = a.harvested
        s_ids, s_items, s_t = synth.training_events(off, items, ts)
        b = tuple(to_dev(np.ascontiguousarray(x).astype(np.uint64) if x.dtype.kind in "ui" else np.ascontiguousarray(x, np.float64)) for x in (s_ids, s_items, s_t))
        rng = np.random.default_rng(13)
        store = DeviceSessionStore(0, capacity=nh + nh // 8, items_cap=8, ttl_secs=1800, idle_secs=1200)
        hv = SessionHarvest(0, capacity=nh, items_cap=8, min_len=2)
        store.set_harvest(hv)
        t_last = int(np.max(s_t)) + 1
        store.import_entries((to_dev(rng.integers(0, 2 ** 63, nh, dtype=np.uint64)), to_dev(np.arange(1, nh + 1, dtype=np.uint64))),
                             to_dev((t_last + rng.integers(0, 86400, nh)).astype(np.uint64)), to_dev(rng.integers(2, 9, nh).astype(np.uint32)),
                             to_dev(rng.integers(1, n_items, (nh, 8)).astype(np.uint64)))
        store.sweep(t_last + 10 ** 6)
        ms = {"from_events_base": [], "events": [], "refreshed_index": []}
        for rep in range(1 + a.reps):
            ix, t0 = timed(lambda: sa.VMISIndex.from_events(*b, m, idfw, device=0))
            ix.close()
            _, t1 = timed(lambda: hv.events(int(np.max(s_ids)) + 1))
            ix, t2 = timed(lambda: refreshed_index(*b, hv, m, idfw, device=0))
            info = ix.info
            ix.close()
            if rep >= 1:
                for name, v in zip(ms, (t0, t1, t2)):
                    ms[name].append(round(v, 4))
        r = {"base_rows": int(len(s_ids)), "harvest": hv.stats(), "ms": ms, "n_sessions_total": int(info["n_sessions_total"]), "n_items": int(info["n_items"])}
        r.update({name + "_ms": round(med(v), 4) for name, v in ms.items()})
        res["refresh"] = r
        print(json.dumps({"refresh": r}), flush=True)
        hv.close()
        store.close()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
