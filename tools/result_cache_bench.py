"""What the device result cache is worth on the headline stream: config 3, the stream bench.py draws, cut into a pool of >= 8 DIFFERENT batches -- the
repeats a cache sees are the stream's own, not one batch replayed.  Batch sizes 4 096, 65 536 and 2^20; two entry points:
  predict    srn_predict_batch_device over the pool's batches (sessions of up to 4 items; the cache keeps sequences of 1..4);
  recommend  recommend_batch with max_items_in_session 2: one click per request from the stream, a third of the requests without consent (cache max_len 2).
Cache off and on ALTERNATE in one process, `--reps` times each; with the cache on the first pass over the pool (cold) and the later passes (steady state) are reported
apart.  Per run: queries/s, hit rate (hits / lookups from srn_index_result_cache_stats), and -- from a `rocprofv3 --kernel-trace --stats` run of their own, a child process
of this tool -- the mean time of the lookup and the insert kernel per call.  Writes one JSON file.

    python tools/result_cache_bench.py [--config cfg3] [--batches 4096,65536,1048576] [--pool 8] [--reps 3] [--rows 4194304] [--no-trace] [--out profiles/result_cache_cfg3.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEADY_PASSES = 2


def setup(config, batches, pool):
    import torch
    import serenade_amd as sa
    from serenade_amd import synth
    inter, n_items, k, m, idfw = synth.CONFIGS[config]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    need = max(batches) * pool
    qi, qo = synth.queries(int(need / 3.2 * 1.05) + 4096, n_items, seed=synth.SEED + 7919, max_items=synth.LAST_ITEMS)
    if len(qo) - 1 < need:
        raise SystemExit("the stream holds %d queries, %d needed" % (len(qo) - 1, need))
    dev = torch.device("cuda:0")
    pools = {}
    for B in batches:
        pools[B] = []
        for b in range(pool):
            o = qo[b * B:(b + 1) * B + 1].astype(np.int64)
            flat = np.concatenate([qi[o[0]:o[-1]], np.zeros(1, np.uint64)])
            pools[B].append((torch.from_numpy(flat.view(np.int64).copy()).to(dev), torch.from_numpy((o - o[0]).astype(np.int32)).to(dev),
                             torch.from_numpy(qi[o[1:] - 1].view(np.int64).copy()).to(dev)))     # ... and each query's most recent item: the recommend mode's click
    return index, pools, (k, m, synth.HOW_MANY, synth.LAST_ITEMS)


def run_pass(mode, index, batch_pool, B, par, out, store_state):
    """One pass over the pool: every batch enqueued, one synchronisation at the end -> seconds."""
    import torch
    import serenade_amd as sa
    from serenade_amd import capi
    k, m, how_many, max_len = par
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for flat, qoff, clicks in batch_pool:
        if mode == "predict":
            sa.predict_batch_device(index, flat.data_ptr(), qoff.data_ptr(), B, max_len, k, m, how_many, False, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream)
        else:
            store, hi, lo, consent = store_state["store"], store_state["hi"], store_state["lo"], store_state["consent"]
            store_state["now"] += 1
            capi.check(capi.lib().srn_recommend_batch_device(index._h, store._h, hi.data_ptr(), lo.data_ptr(), clicks.data_ptr(), consent.data_ptr(), B, store_state["now"], 2,
                                                             k, m, how_many, 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def measure(index, pools, par, reps, rows, modes):
    import torch
    from serenade_amd.serving import DeviceSessionStore
    k, m, how_many, max_len = par
    dev = torch.device("cuda:0")
    runs = []
    for mode in modes:
        for B, batch_pool in pools.items():
            out = (torch.empty(B * how_many, dtype=torch.int64, device=dev), torch.empty(B * how_many, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
            rng = np.random.default_rng(B)
            vis = rng.integers(0, max(1, B // 2), B).astype(np.uint64)                  # about two clicks per visitor in a batch
            state = {"hi": torch.from_numpy((vis * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)).to(dev), "lo": torch.from_numpy(vis.view(np.int64)).to(dev),
                     "consent": torch.from_numpy((rng.random(B) >= 1.0 / 3.0).astype(np.uint8)).to(dev), "now": 1_700_000_000}
            row = {"mode": mode, "batch": B, "pool": len(batch_pool), "off_qps": [], "on_cold_qps": [], "on_steady_qps": [], "on_cold_hit_rate": [], "on_steady_hit_rate": []}
            nq_pass = B * len(batch_pool)
            for rep in range(reps):
                for cache_on in (False, True):
                    if mode == "recommend":
                        state["store"] = DeviceSessionStore(index, capacity=4 * B + 4096, items_cap=8)
                    if cache_on:
                        index.enable_result_cache(rows, max_len if mode == "predict" else 2, k, m, how_many)
                    try:
                        if not cache_on:
                            run_pass(mode, index, batch_pool, B, par, out, state)                    # (workspaces grow, the store fills)
                            row["off_qps"].append(round(nq_pass * STEADY_PASSES / sum(run_pass(mode, index, batch_pool, B, par, out, state) for _ in range(STEADY_PASSES))))
                        else:
                            s0 = index.result_cache_stats()
                            cold = run_pass(mode, index, batch_pool, B, par, out, state)
                            s1 = index.result_cache_stats()
                            steady = sum(run_pass(mode, index, batch_pool, B, par, out, state) for _ in range(STEADY_PASSES))
                            s2 = index.result_cache_stats()
                            row["on_cold_qps"].append(round(nq_pass / cold))
                            row["on_steady_qps"].append(round(nq_pass * STEADY_PASSES / steady))
                            row["on_cold_hit_rate"].append(round((s1["hits"] - s0["hits"]) / max(1, s1["lookups"] - s0["lookups"]), 4))
                            row["on_steady_hit_rate"].append(round((s2["hits"] - s1["hits"]) / max(1, s2["lookups"] - s1["lookups"]), 4))
                            row["cache"] = {n: s2[n] for n in ("rows", "ways", "bytes", "max_len", "lookups", "hits", "inserts", "evictions", "bypassed_calls")}
                    finally:
                        if cache_on:
                            index.disable_result_cache()
                        if mode == "recommend":
                            state["store"].close()
            row["steady_on_over_off"] = round(max(row["on_steady_qps"]) / max(row["off_qps"]), 4)
            runs.append(row)
            print(json.dumps(row), flush=True)
    return runs


def traced_child(a):
    """Under rocprofv3: the cache on, one cold and one warm pass per batch size and mode -- nothing is timed here, the trace is."""
    batches = [int(x) for x in a.batches.split(",")]
    index, pools, par = setup(a.config, batches, a.pool)
    measure(index, pools, par, 1, a.rows, a.modes.split(","))


def trace(a):
    """-> {kernel: {grid: mean us}} of the two cache kernels, from the child's kernel trace (the grid says which batch size a launch belongs to)."""
    rocprof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    d = tempfile.mkdtemp(prefix="rcache_trace_")
    try:
        cmd = [rocprof, "--kernel-trace", "--stats", "-d", d, "-o", "kt", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--traced-child",
               "--config", a.config, "--batches", a.batches, "--pool", str(a.pool), "--rows", str(a.rows), "--modes", a.modes]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=a.trace_timeout)
        per = {}
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                name = r["Kernel_Name"]
                for kern in ("vmis_rcache_lookup_kernel", "vmis_rcache_insert_kernel"):
                    if kern in name:
                        queries = int(r.get("Grid_Size_X", r.get("Grid_Size", 0))) // 256 * 32          # (256 threads serve 32 queries)
                        per.setdefault(kern, {}).setdefault(queries, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        return {kern: {str(q): {"launches": len(v), "mean_us": round(float(np.mean(v)), 2), "max_us": round(float(np.max(v)), 2)} for q, v in sorted(g.items())} for kern, g in per.items()}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--batches", default="4096,65536,1048576")
    ap.add_argument("--pool", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--modes", default="predict,recommend")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-timeout", type=int, default=600)
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "result_cache_cfg3.json"))
    a = ap.parse_args()
    if a.traced_child:
        return traced_child(a)
    batches = [int(x) for x in a.batches.split(",")]
    index, pools, par = setup(a.config, batches, a.pool)
    res = {"config": a.config, "k": par[0], "m": par[1], "how_many": par[2], "pool": a.pool, "reps": a.reps, "cache_rows": a.rows, "steady_passes": STEADY_PASSES,
           "runs": measure(index, pools, par, a.reps, a.rows, a.modes.split(","))}
    index.close()
    if not a.no_trace:
        res["cache_kernels_by_queries_per_launch"] = trace(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
