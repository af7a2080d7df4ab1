"""Evaluation throughput on one GPU: one trial through srn_evaluate (a) against predict's floor on the same prefixes, device-resident
(srn_predict_batch_device, b) and against the evaluator's path -- host expansion, srn_predict_batch from pageable memory, metrics on one host
core -- in C++ (tools/eval_host_path.cpp, c); then a 24-trial grid in one srn_evaluate call.  Writes one JSON file.

    python tools/eval_bench.py [--config cfg3] [--queries 1048576] [--reps 3] [--out profiles/eval_bench_cfg3.json]

--serving: what the serving rules cost.  Four trials alternate in one process, --reps rounds: the plain trial at how_many 21, the plain trial at
how_many 21 + H' (the launch sequence of an excluding trial without its filter and expansion), exclude_seen at 21 with history H', and the same with handler_sessions.
A library without the serving rules runs the two plain arms only, so the same file measures the commit before them.  Writes profiles/eval_serving_<config>.json.

    python tools/eval_bench.py --serving [--history 8] [--reps 5]

--bootstrap [B ...]: what the bootstrap of DESIGN.md 10.2 costs.  The same trial alternates in one process, --reps rounds (default here 5), through srn_evaluate of the
parent commit's library loaded beside this one (--parent-lib; its own index and set from the same data), srn_evaluate of this library, and srn_evaluate_bootstrap at each
B (default 256 and 1024); medians of the wall times.  The yardstick of the cost is the plain arm of the same run; the plain arm against the parent's shows whether the
call without bootstrap moved.  Writes profiles/eval_bootstrap_<config>.json.

    python tools/eval_bench.py --bootstrap [256 1024] [--reps 5] [--parent-lib PATH | --skip-parent]

--segments: what the segments of DESIGN.md 10.4 cost.  The same trial alternates in one process, --reps rounds (default 5), medians of the wall times: without a
bootstrap through the parent commit's library (as above), srn_evaluate of this library, srn_evaluate_segments with position:8 and with 64 label segments; with one,
srn_evaluate_bootstrap at B = 256 and srn_evaluate_segments at B = 256 with position:8.  The segment kernels alone come from HIP events (srn_debug_eval_segment_ms),
next to ms_eval of the same call.  Writes profiles/eval_segments_<config>.json.

    python tools/eval_bench.py --segments [--reps 5] [--parent-lib PATH | --skip-parent]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_path_lib():
    from serenade_amd import build
    src = os.path.join(ROOT, "tools", "eval_host_path.cpp")
    out = os.path.join(ROOT, "serenade_amd", "bin", "libeval_host_path.so")
    if build._stale(out, [src, build.LIB]):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, src, "-L" + os.path.dirname(build.LIB), "-lserenade_hip",
                               "-Wl,-rpath," + os.path.dirname(build.LIB), "-Wl,-rpath,/opt/rocm/lib"])
    L = C.CDLL(out)
    L.srn_host_eval_path.restype = C.c_int
    L.srn_host_eval_path.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_size_t] * 5 + [C.c_uint, C.c_void_p, C.c_void_p]
    return L


def serving_arms(a, es, trial, res):
    from serenade_amd import capi, evaluation
    H = a.history
    arms = {"plain_21": dict(trial), "plain_21_plus_H": dict(trial, how_many=trial["how_many"] + H)}
    if hasattr(capi, "FLAG_EVAL_HANDLER"):
        arms["exclude_seen"] = dict(trial, exclude_seen=True, history=H)
        arms["exclude_seen_handler"] = dict(trial, exclude_seen=True, history=H, handler_sessions=True)
    out = {n: {"wall_ms": [], "ms_predict": [], "ms_eval": []} for n in arms}
    for n, t in arms.items():   # first calls size the workspaces
        evaluation.evaluate(es, [t])
    for _ in range(a.reps):
        for n, t in arms.items():
            t0 = time.perf_counter()
            rep = evaluation.evaluate(es, [t])[0]
            out[n]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            out[n]["ms_predict"].append(rep["ms_predict"])
            out[n]["ms_eval"].append(rep["ms_eval"])
            out[n]["Mrr@20"], out[n]["HitRate@20"] = rep["Mrr@20"], rep["HitRate@20"]
    for n in arms:
        w = out[n]["wall_ms"]
        out[n]["wall_ms_min"], out[n]["wall_ms_max"] = min(w), max(w)
    res.update({"history": H, "reps": a.reps, "serving_rules": hasattr(capi, "FLAG_EVAL_HANDLER"), "arms": out})
    if "exclude_seen" in out:
        base = out["plain_21_plus_H"]["wall_ms_min"]
        res["exclude_seen_over_plain_21_plus_H"] = round(out["exclude_seen"]["wall_ms_min"] / base, 4)
        res["exclude_seen_handler_over_plain_21_plus_H"] = round(out["exclude_seen_handler"]["wall_ms_min"] / base, 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


class ParentLibrary:
    """srn_evaluate on another build of the library: an index and an evaluation set of its own from the same arrays."""
    NAMES = ("srn_index_build_gpu", "srn_index_free", "srn_eval_set_create", "srn_eval_set_free", "srn_evaluate", "srn_last_error")

    def __init__(self, path, capi):
        self.L = C.CDLL(path)
        for name in self.NAMES:
            fn = getattr(self.L, name)
            fn.restype, fn.argtypes = capi.SYMBOLS[name]
        self.capi = capi

    def check(self, rc):
        if rc:
            raise RuntimeError("parent library: %d %s" % (rc, self.L.srn_last_error().decode(errors="replace")))

    def eval_set(self, off, items, ts, m, max_len, idfw, sessions):
        capi = self.capi
        off, items, ts = capi.as_u64(off), capi.as_u64(items), capi.as_u32(ts)
        v = capi.SessionsView(off.ctypes.data, items.ctypes.data, ts.ctypes.data, len(ts))
        self.index = C.c_void_p()
        self.check(self.L.srn_index_build_gpu(C.byref(v), m, max_len, idfw, 0, C.byref(self.index)))
        s_off = np.zeros(len(sessions) + 1, np.uint64)
        s_off[1:] = np.cumsum([len(ev) for ev in sessions.values()])
        s_items = np.fromiter((x for ev in sessions.values() for x in ev), dtype=np.uint64, count=int(s_off[-1]))
        ids, counts = np.unique(items, return_counts=True)
        ids, counts = capi.as_u64(ids), capi.as_u64(counts)
        self.set = C.c_void_p()
        self.check(self.L.srn_eval_set_create(self.index, capi.ptr(s_items), capi.ptr(s_off), len(sessions), capi.ptr(ids), capi.ptr(counts), len(ids), C.byref(self.set)))

    def evaluate(self, trial):
        res = self.capi.EvalResult()
        self.check(self.L.srn_evaluate(self.set, C.byref(trial), 1, C.byref(res), None))
        return res

    def close(self):
        self.L.srn_eval_set_free(self.set)
        self.L.srn_index_free(self.index)


def bootstrap_arms(a, es, trial, res, parent):
    from serenade_amd import evaluation
    reps = a.reps
    Bs = a.bootstrap or [256, 1024]
    arms = {}
    if parent:
        t_parent = evaluation._trial(trial)
        arms["parent_plain"] = lambda: parent.evaluate(t_parent).sum_mrr
    arms["plain"] = lambda: evaluation.evaluate(es, [trial])[0]["sums"]["mrr"]
    for B in Bs:
        arms["bootstrap_%d" % B] = lambda B=B: evaluation.evaluate(es, [trial], bootstrap=B, seed=1)[0]
    out = {n: {"wall_ms": []} for n in arms}
    for f in arms.values():   # first calls size the workspaces
        f()
    for _ in range(reps):
        for n, f in arms.items():
            t0 = time.perf_counter()
            got = f()
            out[n]["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 4))
            if n.startswith("bootstrap_"):
                out[n]["Mrr@20"], out[n]["Mrr@20_ci"], got = got["Mrr@20"], got["Mrr@20_ci"], got["sums"]["mrr"]
            out[n]["sum_mrr"] = got
    if len({o["sum_mrr"] for o in out.values()}) != 1:
        raise SystemExit("the arms' Mrr sums differ: %s" % {n: o["sum_mrr"] for n, o in out.items()})
    med = lambda v: float(np.median(v))   # noqa: E731
    for o in out.values():
        o["wall_ms_median"], o["wall_ms_spread"] = round(med(o["wall_ms"]), 4), round(max(o["wall_ms"]) - min(o["wall_ms"]), 4)
    res.update({"reps": reps, "seed": 1, "parent_lib": bool(parent), "arms": out})
    for B in Bs:
        res["bootstrap_%d_minus_plain_ms" % B] = round(out["bootstrap_%d" % B]["wall_ms_median"] - out["plain"]["wall_ms_median"], 4)
    if parent:
        res["plain_minus_parent_ms"] = round(out["plain"]["wall_ms_median"] - out["parent_plain"]["wall_ms_median"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def segment_arms(a, es, trial, res, parent):
    from serenade_amd import capi, evaluation
    B = 256
    n_sessions = res["test_sessions"]
    position, labels = dict(by="position", n=8), dict(by="labels", labels=np.arange(n_sessions) % 64, n=64)
    arms = {}
    if parent:
        t_parent = evaluation._trial(trial)
        arms["parent_plain"] = lambda: parent.evaluate(t_parent).sum_mrr
    arms["plain"] = lambda: evaluation.evaluate(es, [trial])[0]
    arms["position_8"] = lambda: evaluation.evaluate(es, [trial], segments=position)[0]
    arms["labels_64"] = lambda: evaluation.evaluate(es, [trial], segments=labels)[0]
    arms["bootstrap_%d" % B] = lambda: evaluation.evaluate(es, [trial], bootstrap=B, seed=1)[0]
    arms["bootstrap_%d_position_8" % B] = lambda: evaluation.evaluate(es, [trial], bootstrap=B, seed=1, segments=position)[0]
    out = {n: {"wall_ms": [], "ms_eval": [], "ms_segments": [], "ms_segment_bootstrap": []} for n in arms}
    for f in arms.values():   # first calls size the workspaces
        f()
    ms = (C.c_double(), C.c_double())
    for _ in range(a.reps):
        for n, f in arms.items():
            t0 = time.perf_counter()
            got = f()
            out[n]["wall_ms"].append(round((time.perf_counter() - t0) * 1e3, 4))
            if n == "parent_plain":
                out[n]["sum_mrr"] = got
                continue
            out[n]["sum_mrr"] = got["sums"]["mrr"]
            out[n]["ms_eval"].append(round(got["ms_eval"], 4))
            if "segments" in got:
                capi.check(capi.lib().srn_debug_eval_segment_ms(es._h, C.byref(ms[0]), C.byref(ms[1])))
                out[n]["ms_segments"].append(round(ms[0].value, 4))
                out[n]["ms_segment_bootstrap"].append(round(ms[1].value, 4))
                out[n]["segment_evaluations"] = [x["qty_evaluations"] for x in got["segments"]]
                if sum(out[n]["segment_evaluations"]) != got["qty_evaluations"]:
                    raise SystemExit("%s: the segments' queries do not add up" % n)
    if len({o["sum_mrr"] for o in out.values()}) != 1:
        raise SystemExit("the arms' Mrr sums differ: %s" % {n: o["sum_mrr"] for n, o in out.items()})
    med = lambda v: round(float(np.median(v)), 4) if len(v) else None   # noqa: E731
    for o in out.values():
        o["wall_ms_median"], o["wall_ms_spread"] = med(o["wall_ms"]), round(max(o["wall_ms"]) - min(o["wall_ms"]), 4)
        for key in ("ms_eval", "ms_segments", "ms_segment_bootstrap"):
            o[key + "_median"] = med(o[key])
    res.update({"reps": a.reps, "seed": 1, "replicates": B, "parent_lib": bool(parent), "arms": out})
    plain, boot = out["plain"]["wall_ms_median"], out["bootstrap_%d" % B]["wall_ms_median"]
    res["position_8_minus_plain_ms"] = round(out["position_8"]["wall_ms_median"] - plain, 4)
    res["labels_64_minus_plain_ms"] = round(out["labels_64"]["wall_ms_median"] - plain, 4)
    res["bootstrap_minus_plain_ms"] = round(boot - plain, 4)
    res["segmented_bootstrap_minus_bootstrap_ms"] = round(out["bootstrap_%d_position_8" % B]["wall_ms_median"] - boot, 4)
    res["naive_segmented_bootstrap_ms"] = round(8 * (boot - plain), 4)   # boot_group_kernel once per segment: S times the bootstrap's added cost
    if parent:
        res["plain_minus_parent_ms"] = round(plain - out["parent_plain"]["wall_ms_median"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--reps", type=int, default=None, help="default 3, with --bootstrap 5")
    ap.add_argument("--skip-host", action="store_true", help="leave out (c)")
    ap.add_argument("--grid", type=int, default=1, help="0: leave out the 24-trial call")
    ap.add_argument("--out", default=None, help="default: profiles/eval_bench_cfg3.json, with --serving profiles/eval_serving_<config>.json")
    ap.add_argument("--serving", action="store_true", help="the serving-rule arms instead of (a), (b), (c) and the grid")
    ap.add_argument("--history", type=int, default=8, help="--serving: H' (>= --window)")
    ap.add_argument("--bootstrap", type=int, nargs="*", default=None, metavar="B", help="the bootstrap arms (default B: 256 1024) instead of (a), (b), (c) and the grid")
    ap.add_argument("--segments", action="store_true", help="the segment arms (DESIGN.md 10.4) instead of (a), (b), (c) and the grid")
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "serenade_amd", "variants", "libserenade_hip_parent.so"), help="--bootstrap, --segments: the parent commit's library")
    ap.add_argument("--skip-parent", action="store_true", help="--bootstrap: no parent arm; the run then cannot tell whether the plain call moved")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 5 if a.bootstrap is not None or a.segments else 3
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "eval_segments_%s.json" % a.config if a.segments else "eval_bootstrap_%s.json" % a.config if a.bootstrap is not None else
                             "eval_serving_%s.json" % a.config if a.serving else "eval_bench_cfg3.json")
    if (a.bootstrap is not None or a.segments) and not a.skip_parent and not os.path.exists(a.parent_lib):
        raise SystemExit("the parent commit's library %s is missing: build it from the parent commit and pass --parent-lib, or pass --skip-parent" % a.parent_lib)
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, evaluation, synth

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, length, W = 21, 20, a.window
    t0 = time.time()
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    t_index = time.time() - t0
    n_sess = max(1024, int(a.queries / 3.2) + 4096)
    sessions = synth.test_sessions(n_sess, n_items, seed=synth.SEED + 7919)
    keep, nq = {}, 0
    for s, ev in sessions.items():   # whole sessions up to the query budget
        if nq + len(ev) - 1 > a.queries:
            break
        keep[s] = ev
        nq += len(ev) - 1
    sessions = keep
    t0 = time.time()
    es = evaluation.EvalSet(index, sessions, items)
    t_set = time.time() - t0
    trial = dict(k=k, m=m, max_items_in_session=W, how_many=how_many, length=length)
    res = {"config": a.config, "k": k, "m": m, "window": W, "how_many": how_many, "length": length, "test_sessions": len(sessions), "queries": nq,
           "index_build_s": round(t_index, 2), "eval_set_create_s": round(t_set, 3)}

    if a.serving:
        serving_arms(a, es, trial, res)
        return
    if a.segments:
        parent = None
        if not a.skip_parent:
            parent = ParentLibrary(a.parent_lib, capi)
            parent.eval_set(off, items, ts, m, 34, idfw, sessions)
        segment_arms(a, es, trial, res, parent)
        if parent:
            parent.close()
        return
    if a.bootstrap is not None:
        parent = None
        if not a.skip_parent:
            parent = ParentLibrary(a.parent_lib, capi)
            parent.eval_set(off, items, ts, m, 34, idfw, sessions)
        bootstrap_arms(a, es, trial, res, parent)
        if parent:
            parent.close()
        return

    # (a) srn_evaluate, one trial per call
    evaluation.evaluate(es, [trial])
    wall, rep = [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        rep = evaluation.evaluate(es, [trial])[0]
        wall.append((time.perf_counter() - t0) * 1e3)
    res["a_evaluate"] = {"wall_ms": wall, "ms_predict": rep["ms_predict"], "ms_eval": rep["ms_eval"], "Mrr@20": rep["Mrr@20"], "HitRate@20": rep["HitRate@20"]}

    # (b) the same prefixes through srn_predict_batch_device alone
    prefixes = [ev[max(0, st - W):st] for ev in sessions.values() for st in range(1, len(ev))]   # evaluator.rs:46-56
    qoff = np.zeros(len(prefixes) + 1, np.uint32)
    qoff[1:] = np.cumsum([len(p) for p in prefixes])
    flat = np.fromiter((x for p in prefixes for x in p), dtype=np.uint64, count=int(qoff[-1]))
    dev = torch.device("cuda:0")
    d_items = torch.from_numpy(flat.view(np.int64)).to(dev)
    d_qoff = torch.from_numpy(qoff.view(np.int32)).to(dev)
    d_ids = torch.empty(nq * how_many, dtype=torch.int64, device=dev)
    d_sc = torch.empty(nq * how_many, dtype=torch.float64, device=dev)
    d_cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    max_len = int(np.diff(qoff.astype(np.int64)).max())

    def run_b():
        sa.predict_batch_device(index, d_items.data_ptr(), d_qoff.data_ptr(), nq, max_len, k, m, how_many, False, d_ids.data_ptr(), d_sc.data_ptr(),
                                d_cnt.data_ptr(), stream)
    run_b()
    torch.cuda.synchronize()
    wall_b = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run_b()
        torch.cuda.synchronize()
        wall_b.append((time.perf_counter() - t0) * 1e3)
    res["b_predict_device"] = {"wall_ms": wall_b}
    res["a_over_b"] = round(min(wall) / min(wall_b), 3)
    res["eval_kernels_share_of_predict"] = round(rep["ms_eval"] / rep["ms_predict"], 4) if rep["ms_predict"] else None

    # (c) the evaluator's path in C++
    if not a.skip_host:
        L = host_path_lib()
        s_items = np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint64) for v in sessions.values()]), np.uint64)
        s_off = np.zeros(len(sessions) + 1, np.uint64)
        s_off[1:] = np.cumsum([len(v) for v in sessions.values()])
        tr = np.ascontiguousarray(items, np.uint64)
        ms3, mrr = (C.c_double * 3)(), C.c_double()
        rows = []
        for _ in range(max(1, a.reps - 1)):
            capi.check(L.srn_host_eval_path(index._h, capi.ptr(s_items), capi.ptr(s_off), len(sessions), capi.ptr(tr), len(tr), k, m, how_many, W, length, 0,
                                            ms3, C.byref(mrr)))
            rows.append(list(ms3))
        res["c_host_path"] = {"expand_predict_metrics_ms": rows, "total_ms": [sum(r) for r in rows], "Mrr@20": mrr.value}
        res["c_over_a"] = round(min(sum(r) for r in rows) / min(wall), 2)

    # a 24-trial grid in one call
    if a.grid:
        grid = [dict(k=kk, m=mm, max_items_in_session=w, how_many=how_many, length=length) for mm in (1000, m) for kk in (100, 500, 1000) for w in (1, 2, 3, 4)
                if kk <= mm]
        grid = grid[:24]
        t0 = time.perf_counter()
        reps = evaluation.evaluate(es, grid)
        res["grid"] = {"trials": len(grid), "wall_ms": (time.perf_counter() - t0) * 1e3, "ms_predict": sum(r["ms_predict"] for r in reps),
                       "ms_eval": sum(r["ms_eval"] for r in reps), "queries_per_trial": nq,
                       "best_mrr": max((r["Mrr@20"], i) for i, r in enumerate(reps))[0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
