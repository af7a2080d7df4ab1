"""What do the light queries of the headline batch cost on the lean chain?  (Step 0 of the light form, profiles/light_form_ab.txt.)

A query is light when it has ONE posting run (one distinct known item with a non-empty list, wherever it stands in the session) of at most 64 kept entries.  The tool
draws the headline stream (bench.py's draw_batches: synth.queries(..., seed = SEED + 7919, max_items = LAST_ITEMS)) until it holds N distinct light queries, serves
those N as ONE batch with the library in use (SRN_LIB_PATH selects it) under `rocprofv3 --kernel-trace`, and reports from the trace, per query: the lean launch of
vmis_fast_kernel, vmis_finish_kernel and vmis_finish_big_kernel.  Time per query x the light representatives of headline batch 0 (counted here) is the ceiling of what
a form of their own can take out of a step.

usage: python tools/light_form_bench.py [--n 131072] [--config cfg3] [--calls 10] [--out DIR]
(the tool starts itself again under rocprofv3 as a fresh process; the outer process never opens the GPU)"""
import argparse, csv, glob, json, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEPT_MAX = 64


def light_mask(q_items, q_off, ids_sorted, list_len, last_items):
    """-> (light bool[nq], kept u32[nq], key rows u64[nq, last_items + 1]).  The prep kernel's rule on the CPU: runs = the session's distinct known items with a
    non-empty list (most recent occurrence only); light = one run of <= KEPT_MAX entries (such a list is shorter than m: nothing is cut, kept = its length)."""
    nq = len(q_off) - 1
    lo = q_off[:-1].astype(np.int64); L = np.diff(q_off.astype(np.int64))
    NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
    seq = np.full((nq, last_items), NONE, np.uint64)
    for j in range(last_items):   # column j = position j, most recent first
        have = L > j
        seq[have, j] = q_items[lo[have] + L[have] - 1 - j]
    at = np.minimum(np.searchsorted(ids_sorted, seq), len(ids_sorted) - 1)
    known = ids_sorted[at] == seq
    ln = np.where(known, list_len[at], 0).astype(np.int64)
    first = np.ones((nq, last_items), bool)
    for j in range(1, last_items):
        for i in range(j):
            first[:, j] &= seq[:, j] != seq[:, i]
    run = first & (ln > 0) & (seq != NONE)
    nr = run.sum(1)
    kept = (ln * run).sum(1)
    light = (nr == 1) & (kept <= KEPT_MAX) & (L >= 1) & (L <= last_items)
    key = np.concatenate([seq, L[:, None].astype(np.uint64)], axis=1)
    return light, kept.astype(np.uint32), key


def child(args):
    import torch
    import serenade_amd as sa
    from serenade_amd import synth
    inter, n_items, k, m, idfw = synth.CONFIGS[args.config]
    off, items, ts = synth.training_sessions(inter, n_items)
    ix = sa.VMISIndex.from_sessions(off, items, ts, m, 34, idfw, builder="gpu")
    ids_sorted, cnt = np.unique(items, return_counts=True)   # (a training session holds an item once: the count is the list's length before the index's cut)
    list_len = np.minimum(cnt, m).astype(np.int64)
    B = 1 << 20
    n_sess = int(2 * B / 3.2) + 4096
    res = {}
    while True:
        qi, qo = synth.queries(n_sess, n_items, seed=synth.SEED + 7919, max_items=synth.LAST_ITEMS)
        light, kept, key = light_mask(qi, qo, ids_sorted, list_len, synth.LAST_ITEMS)
        if "batch0" not in res and len(qo) - 1 >= B:
            k0 = key[:B]
            n_distinct = len(np.unique(k0, axis=0))
            l0 = light[:B]
            res["batch0"] = {"queries": B, "distinct": int(n_distinct), "light_representatives": int(len(np.unique(k0[l0], axis=0))), "light_queries": int(l0.sum()),
                             "light_one_item_sessions": int((l0 & (np.diff(qo[:B + 1].astype(np.int64)) == 1)).sum())}
        lk = key[light]
        _, firsts = np.unique(lk, axis=0, return_index=True)
        if len(firsts) >= args.n:
            break
        n_sess = int(n_sess * max(1.5, 1.2 * args.n / max(1, len(firsts))))
    pick = np.flatnonzero(light)[np.sort(firsts)[:args.n]]   # the first N distinct light queries, in stream order
    lo = qo[:-1].astype(np.int64)[pick]; L = np.diff(qo.astype(np.int64))[pick]
    q_off = np.zeros(args.n + 1, np.uint32); q_off[1:] = np.cumsum(L)
    take = np.repeat(lo - q_off[:-1].astype(np.int64), L) + np.arange(int(q_off[-1]), dtype=np.int64)
    flat = np.ascontiguousarray(qi[take])
    res["served"] = {"queries": int(args.n), "stream_queries_drawn": int(len(qo) - 1), "one_item_sessions": int((L == 1).sum()), "mean_kept": float(kept[pick].mean()),
                     "kept_hist_le_1_4_16_64": [int((kept[pick] <= v).sum()) for v in (1, 4, 16, 64)]}
    # distinct scored items of a sample (host copy of the index): more than 63 of them and no threshold = the hand-off of vmis_finish_big_kernel
    rng = np.random.default_rng(synth.SEED)
    M = []
    for q in rng.choice(args.n, min(args.n, 1500), replace=False):
        s = flat[q_off[q]:q_off[q + 1]]
        seen = set()
        for it in s[::-1]:
            p, _ = ix.postings(int(it))
            if p is not None and len(p):
                for ses in p:
                    seen.update(ix.items_for_session(int(ses)).tolist())
                break
        seen.discard(int(s[-1]))
        M.append(len(seen))
    M = np.array(M)
    res["sample"] = {"queries": int(len(M)), "distinct_scored_items_mean": float(M.mean()), "p99": float(np.percentile(M, 99)), "max": int(M.max()),
                     "share_over_63": float((M > 63).mean())}
    dev = torch.device("cuda:0"); n = synth.HOW_MANY; nq = args.n
    d_flat = torch.from_numpy(flat.view(np.int64).copy()).to(dev); d_off = torch.from_numpy(q_off.view(np.int32).copy()).to(dev)
    o_ids = torch.zeros(nq * n, dtype=torch.int64, device=dev); o_sc = torch.zeros(nq * n, dtype=torch.float64, device=dev); o_cnt = torch.zeros(nq, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    sa.reserve(ix, nq, synth.LAST_ITEMS, k, m, n, False, st)
    for _ in range(3 + args.calls):
        sa.predict_batch_device(ix, d_flat.data_ptr(), d_off.data_ptr(), nq, synth.LAST_ITEMS, k, m, n, False, o_ids.data_ptr(), o_sc.data_ptr(), o_cnt.data_ptr(), st)
    torch.cuda.synchronize()
    _, general, glob_ = ix.last_path_counts()
    cnt_h = o_cnt.cpu().numpy()
    res["served"].update({"handed_to_general_kernel": int(general), "global_pass": int(glob_), "merged": int(ix.last_dedup_count()),
                          "rows_with_results": int((cnt_h > 0).sum()), "mean_row_count": float(cnt_h.mean())})
    try:
        res["served"]["light_form"] = int(ix.last_light_count())
    except AttributeError:   # (an older library loaded through SRN_LIB_PATH has no such counter)
        pass
    json.dump(res, open(args.child, "w"))


def summarize(d, calls, nq):
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        rows += list(csv.DictReader(open(f)))
    per = {}
    for r in rows:
        nm = r["Kernel_Name"]
        for kname in ("vmis_light_kernel", "vmis_fast_kernel", "vmis_finish_big_kernel", "vmis_finish_kernel", "vmis_prep_kernel", "vmis_predict_kernel"):
            if kname in nm:
                per.setdefault(kname, []).append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6))
                break
    out = {}
    for kname, v in per.items():
        if kname in ("vmis_fast_kernel", "vmis_predict_kernel"):   # one launch per call: the longest (the lean form; the BIG form's launch / the global-table pass leave at once)
            v = sorted(v, key=lambda x: -x[1])[:3 + calls]
        v.sort()   # in start order: the first three are the warm-up calls
        timed = np.array([x[1] for x in v[-calls:]])
        out[kname] ={"launches": int(len(v)), "median_ms": float(np.median(timed)), "min_ms": float(timed.min()), "max_ms": float(timed.max()), "ns_per_query": float(np.median(timed) * 1e6 / nq)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory for the raw trace (default: a temporary one)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    d = args.out or tempfile.mkdtemp(prefix="light_form_")
    os.makedirs(d, exist_ok=True)
    side = os.path.join(d, "light_form_child.json")
    cmd = ["rocprofv3", "--kernel-trace", "-d", d, "-o", "kt", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
           "--n", str(args.n), "--config", args.config, "--calls", str(args.calls), "--child", side]
    rc = subprocess.call(cmd, stdout=sys.stderr)
    if rc != 0:
        print("light_form_bench: the traced run ended with %d" % rc, file=sys.stderr)
        sys.exit(1)
    res = json.load(open(side))
    res["library"] = os.path.basename(os.environ.get("SRN_LIB_PATH", "default"))
    res["kernels"] = summarize(d, args.calls, args.n)
    kn = res["kernels"]
    chain = sum(kn[x]["ns_per_query"] for x in ("vmis_light_kernel", "vmis_fast_kernel", "vmis_finish_kernel", "vmis_finish_big_kernel") if x in kn)
    reps = res["batch0"]["light_representatives"]
    res["chain_ns_per_query"] = chain
    res["ceiling_ms_per_headline_step"] = chain * reps / 1e6
    print(json.dumps(res))
    print("light queries served %d: lean + finish kernels %.1f ns per query; headline batch 0 holds %d light representatives of %d distinct queries: ceiling %.3f ms per step"
          % (args.n, chain, reps, res["batch0"]["distinct"], res["ceiling_ms_per_headline_step"]))


if __name__ == "__main__":
    main()
