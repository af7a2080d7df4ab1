"""/v1/recommend for whole batches on one GPU: three things timed in one process, alternating --
  (1) srn_recommend_batch_device: the device-resident session store + predict, 2^20 requests per call;
  (2) srn_predict_batch_device alone on exactly the sessions (1) emitted: the floor;
  (3) the per-request path: 16 host threads calling srn_recommend on a host store and a batcher (tools/recommend_host_path.cpp), on the same requests --
for two key mixes (every key distinct | about four clicks per visitor in a batch, with repeated clicks), each at max_items_in_session 2 and 5.
Reports requests/s and the device time of the store's kernels apart from predict's (HIP events).  Writes one JSON file.

    python tools/recommend_bench.py [--config cfg3] [--requests 1048576] [--reps 3] [--host-requests 262144] [--out profiles/recommend_batch_cfg3.json]
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
    src = os.path.join(ROOT, "tools", "recommend_host_path.cpp")
    out = os.path.join(ROOT, "serenade_amd", "bin", "librecommend_host_path.so")
    if build._stale(out, [src, build.LIB]):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", out, src, "-L" + os.path.dirname(build.LIB), "-lserenade_hip",
                               "-Wl,-rpath," + os.path.dirname(build.LIB), "-Wl,-rpath,/opt/rocm/lib"])
    L = C.CDLL(out)
    L.srn_host_recommend_path.restype = C.c_int
    L.srn_host_recommend_path.argtypes = [C.c_void_p] * 6 + [C.c_size_t, C.c_size_t, C.c_uint64, C.c_size_t, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--requests", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-requests", type=int, default=1 << 18, help="requests of each mix sent through (3); 0: leave (3) out")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recommend_batch_cfg3.json"))
    a = ap.parse_args()
    import torch
    import serenade_amd as sa
    from serenade_amd import capi, synth
    from serenade_amd.serving import Batcher, DeviceSessionStore, SessionStore, recommend_batch, session_keys

    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    how_many, n = synth.HOW_MANY, a.requests
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, device=0, builder="gpu")
    # the clicks: the items of the evaluator-style query stream, in order (a visitor's consecutive clicks are then a held-out session's consecutive items)
    qi, _ = synth.queries(max(1024, n // 3), n_items, seed=synth.SEED + 4201, max_items=1)
    clicks = np.ascontiguousarray(np.resize(qi, n), np.uint64)
    rng = np.random.default_rng(11)
    mixes = {}
    mixes["distinct"] = (np.arange(n), clicks)
    vis = rng.integers(0, max(1, n // 4), n)                                         # about four clicks per visitor in a batch
    rep_clicks = clicks.copy()
    order = np.argsort(vis, kind="stable")
    same = np.flatnonzero((vis[order][1:] == vis[order][:-1]) & (rng.random(n - 1) < 0.2)) + 1
    rep_clicks[order[same]] = rep_clicks[order[same - 1]]                            # a fifth of a visitor's clicks repeat the previous one
    mixes["four_per_visitor"] = (vis, rep_clicks)
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    d_ids = torch.empty(n * how_many, dtype=torch.int64, device=dev)
    d_sc = torch.empty(n * how_many, dtype=torch.float64, device=dev)
    d_cnt = torch.empty(n, dtype=torch.int32, device=dev)
    res = {"config": a.config, "k": k, "m": m, "how_many": how_many, "requests_per_call": n, "host_threads": a.threads, "host_requests": a.host_requests, "runs": []}
    L = host_path_lib() if a.host_requests else None
    for mix, (vis, clk) in mixes.items():
        sids = ["visitor-%d" % v for v in vis]
        hi, lo = session_keys(sids)
        t_hi, t_lo = (torch.from_numpy(x.view(np.int64)).to(dev) for x in (hi, lo))
        t_its = [torch.from_numpy(np.roll(clk, 7 * r).view(np.int64)).to(dev) for r in range(4)]   # a round's clicks differ from the previous round's: the sessions move
        raw = [s.encode() for s in sids[:a.host_requests]]
        s_off = np.zeros(len(raw) + 1, np.uint64)
        s_off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
        s_flat = np.frombuffer(b"".join(raw) or b"\0", np.uint8)
        for max_items in (2, 5):
            store = DeviceSessionStore(index, capacity=4 * n, items_cap=8)
            store.timing(True)
            now = 1_700_000_000
            row = {"mix": mix, "max_items_in_session": max_items, "distinct_keys": int(len(np.unique(vis)))}
            wall1, wall2, ms_store, ms_pred, wall3 = [], [], [], [], []
            warm = max_items + 1                                                       # (workspaces grow, the sessions reach max_items_in_session items)
            for rep in range(warm + a.reps):
                now += 60
                t_it = t_its[rep % len(t_its)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                capi.check(capi.lib().srn_recommend_batch_device(index._h, store._h, t_hi.data_ptr(), t_lo.data_ptr(), t_it.data_ptr(), None, n, now, max_items,
                                                                 k, m, how_many, 0, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), stream))
                torch.cuda.synchronize()
                w1 = (time.perf_counter() - t0) * 1e3
                a_ms, b_ms = store.last_ms()
                # (2) predict alone on the sessions (1) just emitted, where they lie
                p_items, p_qoff, p_n, p_len = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
                capi.check(capi.lib().srn_debug_device_sessions_last_batch(store._h, C.byref(p_items), C.byref(p_qoff), C.byref(p_n), C.byref(p_len), None, 0, None))
                t0 = time.perf_counter()
                sa.predict_batch_device(index, p_items.value, p_qoff.value, p_n.value, p_len.value, k, m, how_many, False, d_ids.data_ptr(), d_sc.data_ptr(),
                                        d_cnt.data_ptr(), stream)
                torch.cuda.synchronize()
                w2 = (time.perf_counter() - t0) * 1e3
                if rep >= warm:
                    wall1.append(w1); wall2.append(w2); ms_store.append(a_ms); ms_pred.append(b_ms)
            row.update({"1_recommend_batch_wall_ms": wall1, "1_ms_store_kernels": ms_store, "1_ms_predict": ms_pred, "2_predict_alone_wall_ms": wall2,
                        "1_requests_per_s": round(n / (min(wall1) * 1e-3)), "2_requests_per_s": round(n / (min(wall2) * 1e-3)),
                        "1_over_2": round(min(wall1) / min(wall2), 4), "store_kernels_over_predict": round(min(ms_store) / min(ms_pred), 4),
                        "stats": store.stats})
            store.close()
            if L is not None:
                host_store, batcher = SessionStore(), Batcher(index, k, m, how_many, False, max_batch=4096, max_wait_us=200)
                secs, chk = C.c_double(), C.c_uint64()
                for rep in range(2):
                    clk_r = np.ascontiguousarray(np.roll(clk, 7 * rep))
                    capi.check(L.srn_host_recommend_path(batcher._h, host_store._h, capi.ptr(s_flat), capi.ptr(s_off), capi.ptr(clk_r), None, len(raw), max_items,
                                                         now + 60 * rep, how_many, a.threads, C.byref(secs), C.byref(chk)))
                    wall3.append(secs.value * 1e3)
                batcher.close()
                host_store.close()
                row.update({"3_per_request_path_wall_ms": wall3, "3_requests_per_s": round(len(raw) / (min(wall3) * 1e-3)),
                            "1_over_3_requests_per_s": round(row["1_requests_per_s"] / (len(raw) / (min(wall3) * 1e-3)), 1)})
            res["runs"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"written": a.out}))


if __name__ == "__main__":
    main()
