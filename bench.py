#!/usr/bin/env python3
"""bench.py -- VMIS-kNN predict_next throughput on MI355X (BASELINE.json metric).

A "step" is one pass of the hot path (libserenade_hip.so) over one batch of synthetic evolving sessions, with the index and the
query / result buffers already resident in HBM.  The workload is BASELINE.json configs[2] -- the 60 M-interaction / 1.76 M-item
synthetic index the metric's target is quoted on (k=1500, m=2500, idf_weighting=2).

  One process per GPU (launched by torch.distributed.run -- or by this script itself when started bare with --gpus N), and at EVERY N, N = 1 included,
  with --full BOTH modes of SURVEY.md 8(e) in one line, so that a 1/2/4/8 curve can be read mode by mode (a plain run: the mode of `value` alone):
    value_replicas      every GPU holds the whole index and serves its own slice of the query stream through srn_predict_batch_device (2^20 evolving sessions
                        per step and GPU), no data-path collective (how the reference scales: replicas + session affinity, src/endpoints/recommend_resource.rs:17-19)
    value_item_sharded  the north star's partitioning: the index ITEM-SHARDED over the N GPUs (owner = hash of the item id), every rank sees the whole
                        batch, srn_shard_group_predict_batch exchanges the posting lists and merges the per-shard top-n over RCCL (called from inside the
                        library); at N = 1 a group of one shard on a 1-rank communicator
    value / value_mode  N = 1: the replicas figure (the metric's configuration on one GPU, "scaling": "weak"); N > 1: the item-sharded figure ("strong"),
                        as BASELINE.json's north star asks -- value_mode says which, the other one is beside it
  --mode replicas | item-sharded runs one of them alone.  --rehearse N: N processes on device 0 over the callback transport (gloo) -- the N > 1 code path,
  line assembly included, on a one-GPU box (tests/test_gpu_bench_rehearsal.py).
  At N > 1 the item-sharded mode is timed twice: first with the exchange of batch i + 1 NOT overlapped with batch i (one communicator busy at a time),
  then overlapped (two communicators in flight) under a watchdog; the line says which run `value_item_sharded` comes from and carries both.

A plain run (`bench.py --gpus N --steps K --warmup W`) does only what the headline figure needs: it generates the workload, builds the index, warms up, times the K steps,
writes the last step's outputs if `--dump-outputs DIR` is given, and prints the line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).  At N = 1 that is
the replicas mode alone; at N > 1 the item-sharded mode alone (its non-overlapped, overlapped and streaming runs: `value` is the best of them), the unsharded index kept
resident as its posting lists as in a --full run.  Everything else -- the parity gate, the top-n property check, the roofline and its counter passes, the batch-size
sweep, the long-session and single-query latencies, the CPU baseline, the replicas mode at N > 1, the group of one shard and the 8-shard block at N = 1 -- runs with
`--full` only, in the order below.

  --dump-outputs DIR  after the timed steps: the rows the timed path wrote in its last step, as DIR/ids.npy, DIR/scores.npy, DIR/counts.npy (float64; ids are
                      48-bit and exact; slots past a row's count are 0) and DIR/rows.npy (which rows of the batch: all of them up to 65 536 rows, above that a
                      fixed seeded sample of 65 536).  Same arguments, same inputs: two builds can be compared output for output.

Order of events with --full (no timing counts before parity):
  1. PARITY GATE  `--parity` queries drawn uniformly over batch 0 (seeded permutation; the launch's first and last 32 always among them) FROM THE ROWS THE FULL-SIZE
                  LAUNCH WROTE, through the product call of every mode that is timed, against the canonical CPU oracle (the closed form of DESIGN.md section 1: a valid
                  refinement of the reference, NOT its literal tie behaviour -- on the reference's own example 13-17 % of the queries differ from the literal loops in which
                  equal-scored items close the top-21): item ids and order exact, scores to 1e-12 relative; a mismatch aborts the run with exit code 1
  2. warm-up, then K timed steps between barrier + synchronize on both sides, max over ranks
  3. (N=1) batch-size sweep {1, 16, 64, 256, 4096, 65536, 2^20}: queries/s and p90 latency, device-resident and host-inclusive
  4. (N=1) CPU baseline: the oracle's literal restatement of the reference loops on the host cores, bounded sample

Prints ONE JSON line on rank 0:
  value         whole-job predict_next queries/s of the K timed steps (max-over-ranks wall time); see value_mode above
  roofline      N=1: dominant kernel (vmis_fast_kernel): algorithmic bytes of the queries it served / its HIP-event duration, `frac` against
                8 TB/s and `frac_counter` = measured HBM traffic / time / 8 TB/s; N>1: the item-sharded step against N x 8 TB/s
  cpu_baseline  see 4.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); the device-to-device copy rate is measured in every run (roofline.measured_copy_gbs: 5.3-5.4 TB/s on the driver's boxes)
SCORE_RTOL = 1e-12      # north star: 1e-5; integer-exact accumulation holds 1e-12


def algorithmic_bytes(stats):
    """B(q) = 4P + 4C + 8K + 4I + 8D + 16H + 8L, every datum counted once in the compact layout."""
    s = stats.astype(np.float64)
    return 4 * s[:, 0] + 4 * s[:, 1] + 8 * s[:, 2] + 4 * s[:, 3] + 8 * s[:, 4] + 16 * s[:, 5] + 8 * s[:, 6]


class c_stdout_to_stderr:
    """RCCL prints a version banner through C stdio when a communicator is created; the contract of this script is ONE JSON line on stdout.  Inside the block
    file descriptor 1 points at stderr, and the C library's buffers are flushed before it is restored."""

    def __enter__(self):
        import ctypes
        sys.stdout.flush()
        self.libc = ctypes.CDLL(None)
        self.libc.fflush(None)
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        self.libc.fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def usable_cores():
    """Host cores this process may actually use: affinity mask capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return max(1, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg3", help="tiny | cfg2 | cfg3 | cfg4 (synth.CONFIGS)")
    ap.add_argument("--batch", type=int, default=1 << 20, help="evolving sessions per step and per GPU")
    ap.add_argument("--pool", type=int, default=2, help="distinct query batches cycled through")
    ap.add_argument("--mode", default="auto", choices=["auto", "replicas", "item-sharded"],
                    help="auto: N=1 the whole index on the GPU; N>1 BOTH modes in one line (value = item-sharded over RCCL, replicas = the ceiling). "
                         "replicas: every GPU holds the index and serves its own queries (no data-path collective); "
                         "item-sharded: the north star's partitioning, index split by item over the GPUs, srn_shard_group_predict_batch")
    ap.add_argument("--shard-batch", type=int, default=1 << 18, help="evolving sessions per item-sharded step (every rank sees the whole batch)")
    ap.add_argument("--resident-flag", action="store_true", help="call srn_predict_batch_device with SRN_FLAG_INPUTS_RESIDENT (a step's prep kernel then runs beside the previous "
                    "step's kernels; measured on config 3: the prep kernel's 0.44 ms disappear from the step but the fast kernel slows down by 0.7 ms -- 40.5 M against 41.3 M queries/s -- "
                    "so it is off by default)")
    ap.add_argument("--shard-timeout", type=int, default=420, help="seconds the item-sharded phase may take before the line falls back to the replicas mode alone")
    ap.add_argument("--rehearse", type=int, default=0, help="N processes on device 0 over the callback transport (gloo): the N > 1 code path of this script on a one-GPU box")
    ap.add_argument("--overlap-probe-timeout", type=float, default=30.0, help="seconds (plus three times the non-overlapped run's duration) the overlapped item-sharded run may take at N > 1")
    ap.add_argument("--no-stream-probe", action="store_true", help="N > 1: skip the third item-sharded run (the streaming form of the neighbours exchange, not overlapped)")
    ap.add_argument("--shard-steps", type=int, default=0, help="timed steps of the item-sharded phase (0: --steps)")
    ap.add_argument("--measure-traffic", dest="measure_traffic", action="store_true", default=True, help="N=1 (default ON where rocprofv3 exists): two extra rocprofv3 --pmc passes "
                    "(FETCH_SIZE, WRITE_SIZE) of this script with 1 + 2 steps, so that roofline.traffic is measured in this run; the committed summary under profiles/ is only a labelled fallback")
    ap.add_argument("--no-measure-traffic", dest="measure_traffic", action="store_false")
    ap.add_argument("--no-sq-passes", action="store_true", help="with --measure-traffic: only the two HBM passes, not the three SQ / L2 counter passes behind roofline_secondary")
    ap.add_argument("--no-local-g8", action="store_true", help="N = 1: skip the item_sharded.local_g8 block (one rank's work of an 8-way item-sharded index, all 8 shards on this GPU)")
    ap.add_argument("--no-postings", action="store_true", help="N > 1: the lists pipeline (posting lists sharded too: every rank redoes all candidate work on exchanged list prefixes) instead of the neighbours pipeline")
    ap.add_argument("--selftest-launch", action="store_true", help="CPU check of the launcher and the control plane (gloo): no GPU, no timing")
    ap.add_argument("--index", default="csr", help="csr: the index built by this library from the synthetic sessions (the headline); avro[:PRODUCER]: the same sessions through the "
                    "reference's production route -- a stand-in for its offline producer (synth.avro_index; PRODUCER = ours | reverse | mixed | per-item: how it orders sessions of equal "
                    "timestamp when it cuts a list; default reverse) writes <tmp>/itemindex + sessionindex Avro files, sessions of more than --producer-max-len items into the session index only, "
                    "and srn_index_new_from_avro loads them (VMISIndex::new, vmis_index.rs:85-314); the parity gate then checks against the oracle's restatement of that constructor "
                    "(lists as given).  N = 1 only; use with --tie-per-second > 1 (unique timestamps leave a producer nothing to do differently)")
    ap.add_argument("--tie-per-second", type=int, default=1, help="coarsen the synthetic timestamps so that ~this many sessions share each value (1: unique, the headline)")
    ap.add_argument("--max-session-len", type=int, default=34, help="csr: max_session_len of the build (34 keeps every synthetic session)")
    ap.add_argument("--producer-max-len", type=int, default=30, help="avro: the producer's session-length cut (longer sessions are in the session index only)")
    ap.add_argument("--builder", default="gpu", choices=["gpu", "host"], help="index construction: rocPRIM sorts on the GPU, or the host builder (same bytes)")
    ap.add_argument("--parity", type=int, default=2048, help="queries of batch 0 checked against the canonical oracle before anything is timed (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sweep", action="store_true", help="skip the batch-size sweep")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU time of the baseline sample")
    ap.add_argument("--traffic-file", default=None, help="profiles/*_traffic_<config>.json from the PMC passes (default: newest match)")
    ap.add_argument("--full", action="store_true", help="besides the headline: parity gate, property check, roofline (with its counter passes), sweeps, latencies, CPU baseline "
                    "and the other mode / shard configurations (the --no-* options above switch parts of it off); a plain run times the headline alone")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write the last timed step's results (ids, scores, counts, rows; float64 .npy) under DIR")
    args = ap.parse_args()

    rehearse = args.rehearse > 1 or os.environ.get("SRN_BENCH_REHEARSE") == "1"
    if "WORLD_SIZE" not in os.environ and args.rehearse > 1:
        args.gpus = args.rehearse
        os.environ["SRN_BENCH_REHEARSE"] = "1"
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # started bare (`python bench.py --gpus N ...`): launch the N ranks ourselves -- one process per GPU under torch.distributed.run, rendezvous on
        # 127.0.0.1 -- and hand their exit code back; rank 0 prints the one JSON line
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus, "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        print("bench.py: rank %s of %d started (local rank %s)" % (os.environ.get("RANK", "0"), world, os.environ.get("LOCAL_RANK", "0")), file=sys.stderr); sys.stderr.flush()
    args.gpus = world
    if args.selftest_launch:
        # the launcher + control plane on CPU: process group over gloo, barrier, the max-over-ranks reduction of the timing, the broadcast that carries
        # the shard group's 256-byte id to the other ranks
        import torch
        import torch.distributed as dist
        from serenade_amd import distributed as D
        D.init("gloo")
        D.barrier()
        mx = D.max_over_ranks(1.0 + rank)
        t = torch.tensor([7 * (i + 1) % 251 for i in range(256)] if rank == 0 else [0] * 256, dtype=torch.uint8)
        if world > 1:
            dist.broadcast(t, src=0)
        ok = mx == float(world) and int(t.sum()) == sum(7 * (i + 1) % 251 for i in range(256))
        if rank == 0:
            print(json.dumps({"selftest_launch": True, "world": world, "max_over_ranks": mx, "id_broadcast_ok": bool(ok)}))
        if world > 1:
            dist.destroy_process_group()
        sys.exit(0 if ok else 1)

    import torch
    import torch.distributed as dist
    import serenade_amd as sa
    from serenade_amd import distributed as D
    from serenade_amd import synth

    if not torch.cuda.is_available():
        print("bench.py: no GPU visible; the predict path has no CPU fallback", file=sys.stderr)
        sys.exit(2)
    if rehearse:
        local_rank = 0        # every rank on the one GPU of the box; process group over gloo, the shard group's collectives through application callbacks
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    with c_stdout_to_stderr():
        D.init("gloo" if rehearse else "nccl", dev)   # RCCL; the process group is the control plane (barrier, max-over-ranks, the shard group's id); the data-path collectives are the library's own
    ctl_dev = "cpu" if rehearse else dev

    inter, n_items, k, m, idfw = synth.CONFIGS[args.config]
    how_many, last_items = synth.HOW_MANY, synth.LAST_ITEMS
    if args.mode != "auto":
        mode = args.mode
    elif args.full:
        mode = "both"
    else:       # a plain run times the mode of the headline alone
        mode = "replicas" if world == 1 else "item-sharded"
    do_rep, do_shard = mode in ("replicas", "both"), mode in ("item-sharded", "both")
    keep_index = do_rep or args.mode == "auto"   # the unsharded index stays resident as the item-sharded phase's posting lists, plain or --full alike
    t0 = time.time()
    off, items, ts = synth.training_sessions(inter, n_items)
    if args.tie_per_second > 1:
        ts = synth.tie_timestamps(ts, args.tie_per_second)
    t_gen = time.time() - t0
    t0 = time.time()
    avro = None   # --index avro: what the producer wrote (the lists as given), for the checker
    if args.index.startswith("avro"):
        if world != 1:
            print("bench.py: --index avro is a one-GPU line", file=sys.stderr)
            sys.exit(2)
        import shutil
        import tempfile
        producer = args.index.split(":", 1)[1] if ":" in args.index else "reverse"
        tmpd = tempfile.mkdtemp(prefix="srn_avro_")
        try:
            t1 = time.time()
            p_ids, p_off, p_sess, p_idf = synth.avro_index(tmpd, off, items, ts, m, args.producer_max_len, idfw, producer)
            t_write = time.time() - t1
            avro_bytes = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(tmpd) for f in fs)
            t1 = time.time()
            index = sa.VMISIndex.new_from_avro(tmpd, device=local_rank)
            t_load = time.time() - t1
        finally:
            shutil.rmtree(tmpd, ignore_errors=True)
        avro = {"producer": producer, "ids": p_ids, "off": p_off, "sess": p_sess, "idf": p_idf, "write_s": t_write, "load_s": t_load, "file_bytes": int(avro_bytes)}
        args.no_local_g8 = True   # (the 8-shard block cuts shards from a CSR-built index)
    else:
        # the whole index: what the replicas serve from, and (rank 0) where the per-query counters of the roofline come from
        index = sa.VMISIndex.from_sessions(off, items, ts, m, args.max_session_len, idfw, device=local_rank, builder=args.builder) if (do_rep or rank == 0 or (do_shard and world > 1 and not args.no_postings)) else None
    t_build = time.time() - t0
    shard = group = None
    t_shard = None
    if do_shard:
        from serenade_amd import sharded as SH
        t0 = time.time()
        # every rank cuts ITS shard out of one unsharded index (built on its GPU or -- a production start -- loaded from one file: srn_index_load_shard)
        shard = SH.ShardedVMISIndex.from_full(index, rank, world, device=local_rank) if index is not None else \
            SH.ShardedVMISIndex(off, items, ts, m, 34, idfw, rank, world, device=local_rank)
        t_shard = time.time() - t0
    info = (index if index is not None else shard).info
    stream = torch.cuda.current_stream()
    common = {"metric": "predict_next queries/sec", "unit": "queries/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
              "higher_is_better": True, "vs_baseline": None, "dtype": "u32 ids / i32 accumulators / f64 scores", "data": "synthetic"}

    def draw_batches(B, pool, seed_rank):
        need = B * pool
        n_sess = max(1024, int(need / 3.2) + 4096)
        while True:
            q_items, q_off, q_next = synth.queries(n_sess, n_items, seed=synth.SEED + 7919 * (seed_rank + 1), max_items=last_items, with_next=True)
            if len(q_off) - 1 >= need:
                break
            n_sess = int(n_sess * 1.5)
        out = []
        draw_batches.next_items = [q_next[b * B:(b + 1) * B] for b in range(pool)]   # the held-out item behind each query (evaluator.rs:75), for literal_vs_canonical
        for b in range(pool):
            lo, hi = b * B, (b + 1) * B
            fo = q_off[lo:hi + 1].astype(np.int64)
            flat = q_items[fo[0]:fo[-1]]
            qo = (fo - fo[0]).astype(np.uint32)
            out.append((torch.from_numpy(flat.view(np.int64).copy()).to(dev), torch.from_numpy(qo.view(np.int32).copy()).to(dev), flat, qo))
        return out

    oracle_box = {"oix": None, "t_build": None}

    def oracle_index():
        if oracle_box["oix"] is None:
            from oracle import oracle as O   # the CPU oracle is the checker here (and the timed baseline at the end), never the thing measured
            t1 = time.time()
            if avro is not None:   # VMISIndex::new restated: the producer's lists, idf and flags as given; ties among equal timestamps in the order the product serves with
                oracle_box["oix"] = O.OracleIndex.from_parts(avro["ids"], (avro["off"], avro["sess"]), avro["idf"], np.full(len(avro["ids"]), 2, np.uint8), off, items, ts,
                                                             tie_rank=index.session_recency())
            else:
                oracle_box["oix"] = O.OracleIndex(off, items, ts, m, args.max_session_len, idfw, fast=True)
            oracle_box["t_build"] = time.time() - t1
        return oracle_box["oix"]

    def gate_positions(B, n_par):
        """Which rows of a B-query launch the oracle checks: n_par positions drawn uniformly over the WHOLE batch (a seeded permutation), the launch's first and last 32
        queries always among them -- a defect that depends on where a query sits in a large launch (a hand-off list that overflows late, the last workgroups) must not pass
        because only a prefix was looked at."""
        n_par = int(min(B, n_par))
        if n_par >= B:
            return np.arange(B, dtype=np.int64)
        edge = np.unique(np.concatenate([np.arange(min(32, B)), np.arange(max(0, B - 32), B)])).astype(np.int64)
        if len(edge) >= n_par:
            return edge
        perm = np.random.default_rng(0x5E4E4ADE).permutation(B).astype(np.int64)
        rest = perm[~np.isin(perm, edge)][:n_par - len(edge)]
        return np.sort(np.concatenate([edge, rest]))

    def gate(g_ids, g_sc, g_cnt, flat0, qo0, pos, what):
        """The rows `pos` of a FULL-SIZE launch (g_* = those rows of what it wrote) against the canonical oracle on the same queries."""
        qo64 = qo0.astype(np.int64)
        lens = qo64[pos + 1] - qo64[pos]
        sub_off = np.zeros(len(pos) + 1, np.uint32); sub_off[1:] = np.cumsum(lens)
        take = np.repeat(qo64[pos] - sub_off[:-1].astype(np.int64), lens) + np.arange(int(sub_off[-1]), dtype=np.int64)
        ref = oracle_index().predict_batch("canonical", np.ascontiguousarray(flat0[take]), sub_off, k, m, how_many, False, threads=usable_cores())
        ok = np.array_equal(g_cnt, ref["counts"])
        if ok:
            mask = np.arange(how_many)[None, :] < ref["counts"][:, None].astype(np.int64)
            ok = np.array_equal(g_ids[mask], ref["ids"][mask]) and np.allclose(g_sc[mask], ref["scores"][mask], rtol=SCORE_RTOL, atol=0)
        if not ok:
            print("bench.py: PARITY GATE FAILED (%s) on %d queries drawn uniformly over batch 0 -- nothing is timed" % (what, len(pos)), file=sys.stderr)
            os._exit(1)
        return int(len(pos))

    def timed(step_fn, steps=None):
        steps = args.steps if steps is None else steps
        for i in range(args.warmup):
            step_fn(i)
        torch.cuda.synchronize()
        D.barrier()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        t0 = time.perf_counter()
        for i in range(steps):
            ev[i][0].record(stream)
            step_fn(args.warmup + i)
            ev[i][1].record(stream)
        torch.cuda.synchronize()
        D.barrier()
        elapsed = D.max_over_ranks(time.perf_counter() - t0, ctl_dev)
        return elapsed, np.array([a.elapsed_time(b) for a, b in ev])

    # --dump-outputs: the mode whose line is printed writes what its last timed step computed (rank 0's rows)
    dump_from = "replicas" if (do_rep and (world == 1 or not do_shard)) else "item-sharded"
    DUMP_ROWS = 1 << 16           # 65 536 rows of 21 ids + 21 scores in float64: 22 MB, under the 64 MB the dump may take

    def dump_outputs(d_ids, d_sc, d_cnt, B):
        """The rows of a B-query launch (device tensors: int64 ids, float64 scores, int32 counts) as float64 .npy files under --dump-outputs: every row up to
        DUMP_ROWS rows, above that a fixed seeded sample of DUMP_ROWS of them (rows.npy says which).  Slots past a row's count are written as 0."""
        if not args.dump_outputs:
            return
        torch.cuda.synchronize()
        rows = np.arange(B, dtype=np.int64) if B <= DUMP_ROWS else np.sort(np.random.default_rng(synth.SEED).choice(B, DUMP_ROWS, replace=False))
        sel = torch.from_numpy(rows).to(dev)
        ids = d_ids.view(B, how_many).index_select(0, sel).cpu().numpy().view(np.uint64)
        sc = d_sc.view(B, how_many).index_select(0, sel).cpu().numpy()
        cnt = d_cnt.view(B).index_select(0, sel).cpu().numpy().view(np.uint32)
        n = np.where(cnt == 0xFFFFFFFF, 0, np.minimum(cnt, how_many)).astype(np.int64)
        inside = np.arange(how_many)[None, :] < n[:, None]
        if ids[inside].size and int(ids[inside].max()) >= (1 << 53):
            raise RuntimeError("--dump-outputs: an item id above 2^53 has no exact float64")
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in (("ids", np.where(inside, ids, 0).astype(np.float64)), ("scores", np.where(inside, sc, 0.0)),
                        ("counts", cnt.astype(np.float64)), ("rows", rows.astype(np.float64))):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), a)

    # =========================== item-sharded index over the N GPUs (srn_shard_group_*, RCCL inside the library) ===========================
    shard_steps = args.shard_steps or args.steps
    pending = {"line": None}      # what the overlap watchdog prints if the overlapped run never comes back: the line built on the non-overlapped run

    def sharded_phase(make_line):
        nonlocal group
        t0g = time.time()
        with c_stdout_to_stderr():
            if rehearse:
                group = SH.ShardGroup.over(shard, rank, world, SH.DistComm())   # the collectives as callbacks over gloo: every line of the N > 1 path but RCCL itself
            else:
                group = SH.ShardGroup.rccl(shard, rank, world)  # RCCL communicators created inside the library; the id travels over the process group
        nonlocal index
        Bs = args.shard_batch
        sbatches = draw_batches(Bs, args.pool, 0)                     # every rank sees the SAME batches
        postings = None
        bq_mean = None
        resident = {"shard": int(shard.info["device_bytes"]), "unsharded_index_kept_for_the_replicas_phase": int(index.info["device_bytes"]) if (index is not None and do_rep) else 0, "replicated_postings": 0}
        if rank == 0 and index is not None and args.full:   # (the roofline's per-query byte counters come from the unsharded index: taken before it may be let go below)
            nstat = min(Bs, 8192)
            dbg = sa.predict_batch_debug(index, (sbatches[0][2][:sbatches[0][3][nstat]], sbatches[0][3][:nstat + 1]), k, m, how_many, False, neighbours=False)
            bq_mean = float(algorithmic_bytes(dbg["stats"]).mean())
        if world > 1 and not args.no_postings:
            # the NEIGHBOURS pipeline: every rank keeps the posting lists of the whole index beside its shard of the rows, runs find_neighbors for its slice of
            # the batch only, the neighbour lists are all-gathered (srn_shard_group_set_postings).  Where the unsharded index stays resident anyway (mode both: the
            # replicas phase serves from it) IT is the postings -- no second copy of the lists; in item-sharded mode alone the rows-free view is cut and the unsharded
            # index leaves HBM, so that a rank holds what an item-sharded deployment holds: its shard + the replicated lists
            if index is None:
                raise RuntimeError("the neighbours pipeline needs the unsharded index on every rank to cut the postings view from")
            if keep_index:
                postings = index
                if not do_rep:
                    resident["replicated_postings"] = int(index.info["device_bytes"])
            else:
                postings = SH.postings_view(index, device=local_rank)
                resident["replicated_postings"] = int(postings.info["device_bytes"])
                index.close(); index = None
                torch.cuda.empty_cache()
            # the exchange FORMAT of the neighbours pipeline: the first two timed runs use the gather form (SRN_SBACK_STREAM=0: the form every earlier round's tests and
            # rehearsals ran), the streaming form (a third of the bytes, more compute; the library's AUTO for a non-overlapped exchange) is a third run under the watchdog
            stream_env_user = os.environ.get("SRN_SBACK_STREAM")
            if stream_env_user is None:
                from serenade_amd import capi as _capi0
                os.environ["SRN_SBACK_STREAM"] = "0"; _capi0.reload_knobs()
            group.set_postings(postings)
        t_group = time.time() - t0g
        s_out = (torch.empty((Bs, how_many), dtype=torch.int64, device=dev), torch.empty((Bs, how_many), dtype=torch.float64, device=dev),
                 torch.empty(Bs, dtype=torch.int32, device=dev))

        def sstep(i):
            d_flat, d_off, _, _ = sbatches[i % args.pool]
            group.predict_batch(d_flat, d_off, Bs, last_items, k, m, how_many, False, stream.cuda_stream, resident=True, out=s_out)

        # the non-overlapped form first wherever there are peers: one communicator busy at a time, nothing in it that can wait on a peer's other collective
        group.set_overlap(world == 1)
        s_parity = 0
        if args.parity > 0 and args.full:                             # (a collective call: every rank runs it, rank 0 checks)
            sstep(0)
            torch.cuda.synchronize()
            if rank == 0:
                pos = gate_positions(Bs, args.parity)
                s_parity = gate(s_out[0].cpu().numpy().view(np.uint64)[pos], s_out[1].cpu().numpy()[pos], s_out[2].cpu().numpy().view(np.uint32)[pos],
                                sbatches[0][2], sbatches[0][3], pos, "item-sharded")
        def one_run(overlap):
            group.set_overlap(overlap)
            sstep(0); sstep(1)                                        # both buffer slots sized (setup, not one of the W warm-up steps)
            torch.cuda.synchronize()
            st0 = group.stats
            s_elapsed, s_step_ms = timed(sstep, shard_steps)
            st1 = group.stats
            served = int((s_out[2].cpu().numpy().view(np.uint32) != 0xFFFFFFFF).sum())
            nqs = max(1, st1["queries"] - st0["queries"])
            return {"value": shard_steps * Bs / s_elapsed, "ms_per_step": s_elapsed / shard_steps * 1e3, "elapsed_s": s_elapsed,
                    "step_ms_p50": float(np.percentile(s_step_ms, 50)), "step_ms_p90": float(np.percentile(s_step_ms, 90)),
                    "exchange_overlapped_with_previous_batch": bool(st1["overlapped"]), "queries_served_last_step": served, "timed_batches": int(st1["batches"] - st0["batches"]),
                    "transport": {0: "in-process", 1: "rccl", 2: "callbacks"}[st1["transport"]],
                    "neighbour_batches": int(st1["neighbour_batches"] - st0["neighbour_batches"]),
                    "per_q": {kk: (st1[kk] - st0[kk]) / nqs for kk in ("bytes_head", "bytes_counts", "bytes_lists", "bytes_results", "bytes_lists_max_rank", "bytes_neighbours")}}

        def shard_line_of(run, probe):
            ach = bq_mean * Bs / (run["ms_per_step"] * 1e-3) / 1e9 if bq_mean is not None else None
            per_q = run["per_q"]
            line = dict(common)
            line.update({
                "value": run["value"], "ms_per_step": run["ms_per_step"], "steps": shard_steps, "scaling": "strong",
                "config": {"workload": ("BASELINE configs[2]: synthetic %d interactions / %d items, k=%d m=%d idf_weighting=%g last_items=%d how_many=%d" % (inter, n_items, k, m, idfw, last_items, how_many)
                                        if args.config == "cfg3" else "synth.CONFIGS[%s]" % args.config) + "; index item-sharded over %d GPU(s), every rank sees the whole batch" % world,
                           "name": args.config, "batch": Bs, "query_pool_batches": args.pool,
                           "parallelism": ("item-sharded x%d (rows, idf and top-n by owner = hash of the item id; posting lists replicated): rank r runs find_neighbors for its 1/%d of the batch, "
                                           "all-gather of the neighbour lists + all-gather of the per-shard top-n per batch" % (world, world) if run["neighbour_batches"] else
                                           "item-sharded x%d (owner = hash of the item id): all-reduce(max) of the cuts + all-gather of the kept counts + variable-length exchange of "
                                           "the posting-list prefixes + all-gather of the per-shard top-n per batch" % world) + ", RCCL called from inside libserenade_hip.so (srn_shard_group_predict_batch)",
                           "pipeline": "neighbours" if run["neighbour_batches"] else "lists",
                           "rccl_ranks": (int(dist.get_world_size()) if world > 1 else 1) if not rehearse else 0, "transport": run["transport"],
                           "rehearsal": "%d processes on ONE GPU over gloo callbacks: control flow only, not a scaling measurement" % world if rehearse else None,
                           "exchange_overlapped_with_previous_batch": run["exchange_overlapped_with_previous_batch"], "overlap_probe": probe,
                           "items_on_rank0": int(shard.info["n_items"]), "index_bytes_hbm_rank0": int(shard.info["device_bytes"]), "hbm_resident_bytes_rank0": resident,
                           "setup_s": {"generate": round(t_gen, 2), "index_build_upload": round(t_build, 2), "shard_cut_attach": round(t_shard, 2), "group_create": round(t_group, 2)}},
                "roofline": {"bound": "hbm", "kernel": "item-sharded step: list exchange + unsharded kernels over the rank's row fragments + top-n merge", "achieved": ach,
                             "peak": HBM_PEAK_GBS * world, "unit": "GB/s", "frac": ach / (HBM_PEAK_GBS * world), "traffic": None,
                             "algorithmic_bytes_per_query": bq_mean, "queries_per_launch": Bs,
                             "note": "the same algorithmic bytes as the unsharded path (every datum is touched once, on the shard that owns it) against the whole step and N x 8 TB/s"} if ach is not None else None,
                "exchange_bytes_per_query_rank0": {"cuts_all_reduce": per_q["bytes_head"], "kept_counts_all_gather": per_q["bytes_counts"], "list_prefixes_sent": per_q["bytes_lists"],
                                                   "list_prefixes_fullest_rank": per_q["bytes_lists_max_rank"], "neighbour_lists_all_gather": per_q["bytes_neighbours"],
                                                   "topn_all_gather": per_q["bytes_results"]},
                "latency": {"step_ms_p50": run["step_ms_p50"], "step_ms_p90": run["step_ms_p90"]},
                "parity_checked": s_parity, "parity_checked_positions": "uniform over batch", "queries_served_last_step": run["queries_served_last_step"], "timed_batches": run["timed_batches"]})
            if ach is None:          # (a plain run: no per-query byte counters, no roofline)
                del line["roofline"]
            return line

        first = one_run(world == 1)
        if world == 1:
            if rank == 0 and dump_from == "item-sharded":
                dump_outputs(s_out[0], s_out[1], s_out[2], Bs)
            return (shard_line_of(first, None) if rank == 0 else None), sbatches
        # N > 1: the overlapped form (two communicators in flight: batch i + 1's exchange beside batch i's kernels and result gather) under a watchdog.  If it never comes
        # back, the line of the non-overlapped run is printed from the watchdog and the process leaves: a SCALE run cannot end without a line.
        import threading
        limit = args.overlap_probe_timeout + 3.0 * first["elapsed_s"] * (1.0 + (args.warmup + 2.0) / max(1, shard_steps))
        probe_off = {"non_overlapped": {"value": first["value"], "ms_per_step": first["ms_per_step"]}, "overlapped": None, "timed_run": "non-overlapped", "watchdog_s": round(limit, 1)}
        if rank == 0:
            pending["line"] = make_line(shard_line_of(first, dict(probe_off, overlapped="did not finish within the watchdog: this line was printed by it")))

        def probe_hung():
            if rank == 0 and pending["line"] is not None:
                print(json.dumps(pending["line"])); sys.stdout.flush()
            print("bench.py: rank %d: the overlapped item-sharded run did not finish within %.0f s; leaving" % (rank, limit), file=sys.stderr); sys.stderr.flush()
            os._exit(0)
        wd2 = threading.Timer(limit, probe_hung)
        wd2.daemon = True
        D.barrier()
        wd2.start()
        second = one_run(True)
        wd2.cancel()
        best_is_second = second["value"] >= first["value"]
        probe = {"non_overlapped": {"value": first["value"], "ms_per_step": first["ms_per_step"]}, "overlapped": {"value": second["value"], "ms_per_step": second["ms_per_step"]},
                 "timed_run": "overlapped" if best_is_second else "non-overlapped", "watchdog_s": round(limit, 1), "streaming_non_overlapped": None}
        best = second if best_is_second else first
        # third: the streaming form of the exchange, not overlapped (what the library's AUTO takes for a group with real peers) -- set_postings again (a collective: the
        # ranks agree on it), under the watchdog like the overlapped run; it only replaces the line if it is faster
        if postings is not None and os.environ.get("SRN_SBACK_STREAM") == "0" and not args.no_stream_probe:
            if rank == 0:
                pending["line"] = make_line(shard_line_of(best, dict(probe, streaming_non_overlapped="did not finish within the watchdog: this line was printed by it")))
            wd3 = threading.Timer(limit, probe_hung)
            wd3.daemon = True
            D.barrier()
            wd3.start()
            try:
                from serenade_amd import capi as _capi1
                ref_rows = (s_out[0].clone(), s_out[2].clone())     # (the last timed step of every run serves the same batch: the rows must be the same bytes)
                os.environ.pop("SRN_SBACK_STREAM", None); _capi1.reload_knobs()
                group.set_postings(postings)
                third = one_run(False)
                rows_equal = bool(torch.equal(ref_rows[0], s_out[0]) and torch.equal(ref_rows[1], s_out[2]))
                streamed = third["per_q"]["bytes_neighbours"] < 0.75 * first["per_q"]["bytes_neighbours"]
                probe["streaming_non_overlapped"] = {"value": third["value"], "ms_per_step": third["ms_per_step"], "streaming_form_ran": bool(streamed),
                                                     "neighbour_exchange_bytes_per_query_rank0": third["per_q"]["bytes_neighbours"], "rows_equal_the_gather_form_rows": rows_equal}
                if third["value"] > best["value"] and rows_equal and streamed:   # (a group whose shards have no streaming form -- fewer than SRN_SBACK_MIN_SHARDS -- just ran the gather form again)
                    best = third; probe["timed_run"] = "streaming, non-overlapped"
            except Exception as e:
                probe["streaming_non_overlapped"] = {"error": repr(e)[:300]}
            wd3.cancel()
        pending["line"] = None
        if rank == 0 and dump_from == "item-sharded":       # (every run's last step served the same batch; the streaming run checks that its rows equal the gather form's)
            dump_outputs(s_out[0], s_out[1], s_out[2], Bs)
        return (shard_line_of(best, probe) if rank == 0 else None), sbatches

    def measure_traffic_now(B):
        """HBM traffic of the dominant kernel, measured NOW: this script again under rocprofv3 --pmc, FETCH_SIZE and WRITE_SIZE in separate passes (kernel trace only,
        as MI355X_MICROARCH.md prescribes), 1 warm-up + 2 timed steps, the full-batch launches averaged; FETCH_SIZE doubled (gfx950 tallies 128-byte requests as 64)."""
        import shutil
        import subprocess
        import tempfile
        exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
        if not os.path.exists(exe):
            return None, None
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import rocprof_summarize as RS
        vals = {}
        # (round 6) beside the two HBM passes: the SQ counters behind roofline_secondary and the L2's hit / miss / request counters, at THIS batch size, in this run --
        # own passes each (counters only with --kernel-trace: MI355X_MICROARCH.md); a pass that fails costs its block, not the line
        passes = [("FETCH_SIZE",), ("WRITE_SIZE",)]
        if not args.no_sq_passes:
            passes += [("SQ_WAVES", "SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS"),
                       ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_INST_CYCLES_SALU", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_VMEM_RD", "SQ_WAIT_INST_LDS"),
                       ("TCC_HIT_sum", "TCC_MISS_sum", "TCC_REQ_sum", "TCP_TCC_READ_REQ_sum")]
        with tempfile.TemporaryDirectory(dir="/tmp") as tmp:
            for pi, ctrs in enumerate(passes):
                d = os.path.join(tmp, "pass%d" % pi)
                cmd = [exe, "--pmc"] + list(ctrs) + ["--kernel-trace", "-d", d, "-o", "pmc", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--mode", "replicas",
                       "--config", args.config, "--batch", str(B), "--steps", "2", "--warmup", "1", "--no-sweep", "--no-cpu-baseline", "--no-measure-traffic", "--no-local-g8", "--parity", "0", "--builder", args.builder]
                env = dict(os.environ, TMPDIR="/tmp")
                ok = True
                try:
                    r = subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240)
                    ok = r.returncode == 0
                except subprocess.TimeoutExpired:
                    ok = False
                got = RS.counters(d, "vmis_fast_kernel") if ok else {}
                for ctr in ctrs:
                    c = got.get(ctr, [])
                    if not c:
                        continue
                    top = max(g for _, _, g in c)
                    full = [x for _, x, g in sorted(c) if g >= 0.5 * top][:3]
                    vals[ctr] = sum(full) / len(full)
                if pi < 2 and ctrs[0] not in vals:
                    return None, None
        measure_traffic_now.counters = {k: v for k, v in vals.items() if k not in ("FETCH_SIZE", "WRITE_SIZE")}
        return (2.0 * vals["FETCH_SIZE"] + vals["WRITE_SIZE"]) * 1024.0, "measured in this run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, own passes, 3 full-batch launches each"

    # =========================== the whole index on every GPU: replicas, query-sharded (N = 1: THE bench line) ===========================
    def replicas_phase():
        B = args.batch
        batches = draw_batches(B, args.pool, rank)                        # every rank draws its own slice of the query stream
        next0 = draw_batches.next_items[0]
        out_ids = torch.zeros(B * how_many, dtype=torch.int64, device=dev)
        out_sc = torch.zeros(B * how_many, dtype=torch.float64, device=dev)
        out_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
        _, _, flat0, qo0 = batches[0]

        def step(i, nq=None):
            d_flat, d_off, _, _ = batches[i % args.pool]
            sa.predict_batch_device(index, d_flat.data_ptr(), d_off.data_ptr(), B if nq is None else nq, last_items, k, m, how_many, False,
                                    out_ids.data_ptr(), out_sc.data_ptr(), out_cnt.data_ptr(), stream.cuda_stream, resident=args.resident_flag)

        # ---- 1. parity gate (rank 0; the other ranks wait at the barrier below) --------------------------------------------
        parity_checked = 0
        if rank == 0 and args.parity > 0 and args.full:
            pos = gate_positions(B, args.parity)
            step(0)                              # the FULL-SIZE launch of batch 0, the one the timed region repeats: the checked rows are rows IT wrote
            torch.cuda.synchronize()
            parity_checked = gate(out_ids.cpu().numpy().view(np.uint64).reshape(B, how_many)[pos], out_sc.cpu().numpy().reshape(B, how_many)[pos],
                                  out_cnt.cpu().numpy().view(np.uint32)[pos], flat0, qo0, pos, "whole index")
        sa.reserve(index, B, last_items, k, m, how_many, False, stream.cuda_stream)   # size the stream's workspace up front (srn_index_reserve): no call of the run allocates
        if args.full:
            index.kernel_timing(True)  # per-kernel HIP events on the launch stream for the timed region (the roofline's launch duration); off again for the sweeps below
        elapsed, step_ms = timed(step)
        if rank == 0 and dump_from == "replicas":
            dump_outputs(out_ids, out_sc, out_cnt, B)
        served = int((out_cnt.cpu().numpy().view(np.uint32) != 0xFFFFFFFF).sum())
        if not args.full:
            if rank != 0:
                return None
            return dict(common, **{
                "value": args.gpus * args.steps * B / elapsed, "ms_per_step": elapsed / args.steps * 1e3, "scaling": "weak",
                "config": {"workload": "BASELINE configs[2]: synthetic %d interactions / %d items, k=%d m=%d idf_weighting=%g "
                                       "last_items=%d how_many=%d" % (inter, n_items, k, m, idfw, last_items, how_many)
                                       if args.config == "cfg3" else "synth.CONFIGS[%s]" % args.config,
                           "name": args.config, "batch_per_gpu": B, "query_pool_batches": args.pool,
                           "parallelism": "query-sharded replicas x%d (no data-path collective)" % args.gpus,
                           "setup_s": {"generate": round(t_gen, 2), "index_build_upload": round(t_build, 2), "index_builder": args.builder if avro is None else "avro loader"},
                           "index": "csr (built by this library)" if avro is None else "avro (pre-built: VMISIndex::new, vmis_index.rs:85-314)"},
                "latency": {"step_ms_p50": float(np.percentile(step_ms, 50)), "step_ms_p90": float(np.percentile(step_ms, 90))},
                "queries_served_last_step": served,
                "_parity_checked": 0, "_props_ok": None, "_B": B})
        # size-independent properties of the WHOLE last batch (the oracle gate above covers 2 048 queries): every row is a valid top-n list --
        # count <= n, scores positive-or-not but non-increasing, equal scores in ascending id order, no item twice
        cnt = out_cnt.to(torch.int64)
        ok_rows = (cnt >= 0) & (cnt <= how_many)
        col = torch.arange(how_many, device=dev).view(1, -1)
        inside = col < cnt.view(-1, 1)
        sc2 = out_sc.view(B, how_many); id2 = out_ids.view(B, how_many)
        pair = inside[:, 1:] & inside[:, :-1]
        desc = (~pair) | (sc2[:, :-1] > sc2[:, 1:]) | ((sc2[:, :-1] == sc2[:, 1:]) & ((id2[:, :-1] ^ torch.iinfo(torch.int64).min) < (id2[:, 1:] ^ torch.iinfo(torch.int64).min)))
        srt = torch.sort(torch.where(inside, id2, torch.arange(how_many, device=dev).view(1, -1) - how_many - 1), dim=1).values   # (fillers: distinct negatives no real id... u64 ids as int64 may be negative: collisions only flag, never pass wrongly)
        uniq = (srt[:, 1:] != srt[:, :-1]).all(dim=1)
        props_ok = bool((ok_rows & desc.all(dim=1) & uniq).all().item())
        if not props_ok:
            print("bench.py: the last batch's results violate the top-n list properties", file=sys.stderr)
            os._exit(1)

        t_prep, t_fast, t_pred, t_retry = index.kernel_times_detail(min(64, args.steps))
        index.kernel_timing(False)
        nq_last, general_last, global_last = index.last_path_counts()

        if rank != 0:
            return None

        # ---- roofline of the dominant kernel: algorithmic bytes per launch / measured launch duration -------
        # per-query counters come from the general kernel's stats output (validated against the oracle in tests/)
        nstat = min(B, 32768)
        dbg = sa.predict_batch_debug(index, (flat0[:qo0[nstat]], qo0[:nstat + 1]), k, m, how_many, False, neighbours=False)
        bq = algorithmic_bytes(dbg["stats"])
        bytes_per_launch = float(bq.mean()) * B
        fast_used = len(t_fast) > 0 and float(t_fast.mean()) > 0.0
        fast_share = (nq_last - general_last) / float(nq_last) if fast_used else 0.0
        kernel_ms = float(t_fast.mean()) if fast_used else float(t_pred.mean())
        kernel_bytes = bytes_per_launch * (fast_share if fast_used else 1.0)
        achieved = kernel_bytes / (kernel_ms * 1e-3) / 1e9
        step_achieved = bytes_per_launch / (float(np.median(step_ms)) * 1e-3) / 1e9
        retried = int((dbg["stats"][:, 7] == 1).sum())
        # the measured-copy denominator: a device-to-device copy of 1 GiB in this run (read + write bytes per second)
        src = torch.empty(1 << 28, dtype=torch.float32, device=dev); dst = torch.empty_like(src)
        dst.copy_(src); torch.cuda.synchronize()
        ce = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
        for a, b in ce:
            a.record(stream); dst.copy_(src); b.record(stream)
        torch.cuda.synchronize()
        copy_gbs = 2.0 * src.numel() * 4 / (min(a.elapsed_time(b) for a, b in ce) * 1e-3) / 1e9
        del src, dst

        # ---- 3. batch-size sweep: queries/s and p90 latency per batch size -----------------
        sweep = []
        lat_single = None
        if not args.no_sweep and world == 1:
            d_flat, d_off, _, _ = batches[0]
            for s in [1, 16, 64, 256, 4096, 65536, 1 << 20]:
                if s > B:
                    continue
                reps = 30 if s <= 65536 else 10
                for _ in range(3):
                    step(0, s)
                torch.cuda.synchronize()
                es = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
                for a, b in es:
                    a.record(stream); step(0, s); b.record(stream)
                torch.cuda.synchronize()
                dms = np.array([a.elapsed_time(b) for a, b in es])
                hf, ho = flat0[:qo0[s]], qo0[:s + 1]
                hms, hout = [], None
                for _ in range(reps // 3 + 3):   # (the host keeps its result buffers between calls, like a serving / evaluator process: first call allocates, untimed)
                    t1 = time.perf_counter()
                    hout = sa.predict_batch(index, (hf, ho), k, m, how_many, False, out=hout)
                    hms.append((time.perf_counter() - t1) * 1e3)
                hms = np.array(hms[2:])
                sweep.append({"batch": s, "device_resident": {"queries_per_s": s / (float(np.median(dms)) * 1e-3), "ms_p50": float(np.median(dms)), "ms_p90": float(np.percentile(dms, 90))},
                              "host_inclusive": {"queries_per_s": s / (float(np.median(hms)) * 1e-3), "ms_p50": float(np.median(hms)), "ms_p90": float(np.percentile(hms, 90))}})
            # the reference's call shape: one evolving session per call, host pointers (srn_predict).  Since round 6 the C entry point is called directly with buffers that
            # live across the calls, as a serving host would (until round 5 through serenade_amd.predict, whose per-call numpy allocations and result objects were ~9 us of
            # the figure); profiles/r06_latency_resident_cfg3.json has the C++ host's percentiles
            import ctypes as _C
            from serenade_amd import capi as _capi2
            _L = _capi2.lib()
            r_ids, r_sc, r_n = np.zeros(how_many, np.uint64), np.zeros(how_many), _C.c_size_t()
            q_list = [np.ascontiguousarray(flat0[qo0[i]:qo0[i + 1]]) for i in range(600)]

            def one_call(q):
                t1 = time.perf_counter()
                rc = _L.srn_predict(index._h, q.ctypes.data, len(q), k, m, how_many, 0, r_ids.ctypes.data, r_sc.ctypes.data, _C.byref(r_n))
                dt = (time.perf_counter() - t1) * 1e6
                if rc:
                    raise RuntimeError("srn_predict failed")
                return dt
            lat = [one_call(q) for q in q_list[:300]]
            lat_single = np.array(lat[50:])
            # ... and the same calls through a RESIDENT workgroup of the persistent latency path (round 6: srn_index_serve_start -- no kernel launch per call); a workgroup
            # leaves by itself after 2 s without a request, so nothing outlives this block whatever happens
            lat_resident = None
            try:
                index.serve_start(k, m, how_many, False, lanes=1, max_items_in_session=last_items, idle_ms=2000)
                lat = [one_call(q) for q in q_list]
                sv = index.serve_stats()
                lat_resident = {"us": np.array(lat[100:]), "answered_without_a_launch": int(sv[0]), "sent_to_the_launch_path": int(sv[1])}
            except Exception as e:
                lat_resident = {"error": repr(e)[:200]}
            finally:
                try:
                    index.serve_stop()
                except Exception:
                    pass

        # ---- 3b. sessions longer than the headline's last_items (the reference's hyper-parameter grid of last_items_in_session goes to 10,
        # src/hyperparameter/hyperparamgrid.rs:93-139; its README's range to 20): the same index, evaluator-style queries keeping their last 8 / 10 / 20 items, resident
        # batches of 2^18; each gated against the oracle on 256 queries drawn over the whole batch; at 10 items also without the fast kernel's MID instantiation
        # (SRN_NO_MID=1: the launch sequence of round 3), at 20 also without its LONG instantiation (SRN_NO_LONG=1: sessions of 11..20 items on the general kernel, round 4)
        long_sessions = None
        if not args.no_sweep and world == 1 and args.config in ("cfg3", "cfg2", "tiny", "small"):
            from serenade_amd import capi as _capi
            long_sessions = []
            BL = int(min(B, 1 << 18))
            for mi in (8, 10, 20):   # (20: the reference's README lets last_items_in_session_range go to 20; round 5: the fast kernel's LONG instantiation)
                n_sess = max(1024, int(BL / 2.0) + 4096)
                while True:
                    lq_items, lq_off = synth.queries(n_sess, n_items, seed=synth.SEED + 104729, max_items=mi)
                    if len(lq_off) - 1 >= BL:
                        break
                    n_sess = int(n_sess * 1.5)
                lq_off = lq_off[:BL + 1]; lq_items = lq_items[:lq_off[-1]]
                l_flat = torch.from_numpy(lq_items.view(np.int64).copy()).to(dev); l_off = torch.from_numpy(lq_off.view(np.int32).copy()).to(dev)
                lens = np.diff(lq_off.astype(np.int64))
                entry = {"max_items_in_session": mi, "batch": BL, "mean_session_items": float(lens.mean()), "share_of_sessions_over_4_items": float((lens > 4).mean())}
                for tag in (("mid_tier", "without_mid_tier") if mi == 10 else ("mid_tier", "without_long_tier") if mi == 20 else ("mid_tier",)):
                    if tag == "without_mid_tier":
                        os.environ["SRN_NO_MID"] = "1"
                    if tag == "without_long_tier":
                        os.environ["SRN_NO_LONG"] = "1"
                    _capi.reload_knobs()

                    def lstep():
                        sa.predict_batch_device(index, l_flat.data_ptr(), l_off.data_ptr(), BL, mi, k, m, how_many, False, out_ids.data_ptr(), out_sc.data_ptr(), out_cnt.data_ptr(),
                                                stream.cuda_stream)
                    lstep(); torch.cuda.synchronize()
                    if tag == "mid_tier":
                        lpos = gate_positions(BL, 256)
                        gate(out_ids.cpu().numpy().view(np.uint64).reshape(B, how_many)[lpos], out_sc.cpu().numpy().reshape(B, how_many)[lpos],
                             out_cnt.cpu().numpy().view(np.uint32)[lpos], lq_items, lq_off, lpos, "sessions of up to %d items" % mi)
                    es = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(5)]
                    for a_, b_ in es:
                        a_.record(stream); lstep(); b_.record(stream)
                    torch.cuda.synchronize()
                    ms = float(np.median([a_.elapsed_time(b_) for a_, b_ in es]))
                    _, g_last, _ = index.last_path_counts()
                    entry[tag] = {"queries_per_s": BL / (ms * 1e-3), "ms_p50": ms, "listed_for_mid_instantiation": int(index.last_mid_count()), "reached_general_kernel": int(g_last)}
                    os.environ.pop("SRN_NO_MID", None); os.environ.pop("SRN_NO_LONG", None)
                    _capi.reload_knobs()
                entry["parity_checked"] = int(len(gate_positions(BL, 256))); entry["parity_checked_positions"] = "uniform over batch"
                long_sessions.append(entry)

        # HBM traffic per launch comes from separate rocprofv3 --pmc passes over this same command (tools/pmc_bench.sh);
        # the committed summary is read back here so that the line carries it (null if no summary matches the workload)
        traffic, traffic_src, traffic_in_run = None, None, False
        if args.measure_traffic and world == 1:
            t_tr = time.time()
            try:
                traffic, traffic_src = measure_traffic_now(B)
            except Exception as e:   # (a profiler that is absent or misbehaves must not cost the line)
                print("bench.py: traffic passes failed: %r" % (e,), file=sys.stderr)
                traffic, traffic_src = None, None
            traffic_in_run = traffic is not None
            print("bench.py: HBM traffic passes (2 x rocprofv3 --pmc): %.1f s, %s" % (time.time() - t_tr, "ok" if traffic_in_run else "FAILED: falling back to the committed summary"), file=sys.stderr)
        if traffic is None:
            try:
                import glob
                cand = [args.traffic_file] if args.traffic_file else sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*traffic_%s.json" % args.config)))
                if cand:
                    tj = json.load(open(cand[-1]))
                    if tj.get("config") == args.config and tj.get("batch_per_gpu") == B:
                        traffic, traffic_src = tj["traffic_bytes_per_launch"], os.path.relpath(cand[-1], ROOT)
            except Exception:
                pass

        # the kernel's OTHER bounds (the memory system moves half the contract's bytes -- frac_measured_copy > 1 --, so the HBM roofline does not explain the
        # kernel): issue and LDS-pipe utilisation from the SQ counters of the committed PMC passes over this kernel (tools/profiles.sh; never measured inside this run: the
        # counter passes serialise dispatches)
        secondary = None
        try:
            import glob
            cand = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0*_sq_counters_%s.json" % args.config)))
            cin = getattr(measure_traffic_now, "counters", None) if traffic_in_run else None
            sq_in_run = bool(cin) and all(kk in cin for kk in ("SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE"))
            if sq_in_run and fast_used:
                wc = cin["SQ_WAVE_CYCLES"]
                pq = {kk: vv / float(B) for kk, vv in cin.items()}
                dq = {"valu_busy_per_simd": 6.0 * cin["SQ_ACTIVE_INST_VALU"] / wc, "wave_time_issuing": cin["SQ_ACTIVE_INST_ANY"] / wc, "wave_time_parked_waitcnt_or_barrier": cin["SQ_WAIT_ANY"] / wc,
                      "wave_time_waiting_for_issue": cin["SQ_WAIT_INST_ANY"] / wc, "lds_bank_conflict_share_of_lds_cycles": cin["SQ_LDS_BANK_CONFLICT"] / cin["SQ_LDS_IDX_ACTIVE"],
                      "lds_pipe_busy": cin["SQ_LDS_IDX_ACTIVE"] / (wc * 4.0 / 8.0 / 3.0)}
            if (sq_in_run or cand) and fast_used:
                if not sq_in_run:
                    sq = json.load(open(cand[-1]))
                    dq, pq = sq["derived"], sq["per_query"]
                secondary = [
                    {"bound": "valu_issue", "frac": dq["valu_busy_per_simd"], "unit": "share of SIMD cycles the vector ALU is busy", "wave_instructions_per_query": {"valu": pq["SQ_INSTS_VALU"], "salu": pq["SQ_INSTS_SALU"], "lds": pq["SQ_INSTS_LDS"]},
                     "wave_time": {"issuing": dq["wave_time_issuing"], "parked_at_waitcnt_or_barrier": dq["wave_time_parked_waitcnt_or_barrier"], "ready_but_waiting_for_an_issue_slot": dq["wave_time_waiting_for_issue"]}},
                    {"bound": "lds_atomic", "frac": dq.get("lds_pipe_busy"), "unit": "share of cycles the CU's LDS pipe is active", "bank_conflict_share_of_lds_cycles": dq["lds_bank_conflict_share_of_lds_cycles"],
                     "lds_cycles_per_query": pq["SQ_LDS_IDX_ACTIVE"], "of_them_bank_conflicts": pq["SQ_LDS_BANK_CONFLICT"]},
                ]
                l2 = None
                if sq_in_run and cin.get("TCC_HIT_sum") is not None and cin.get("TCC_MISS_sum") is not None:
                    req = cin.get("TCC_REQ_sum", cin["TCC_HIT_sum"] + cin["TCC_MISS_sum"])
                    # (a TCC request moves up to one 128-byte line: the upper bound of what the L2s delivered; peak 34.5 TB/s aggregate, MI355X_MICROARCH.md "L2 (per XCD)")
                    l2 = {"bound": "l2", "hit_rate": cin["TCC_HIT_sum"] / max(1.0, cin["TCC_HIT_sum"] + cin["TCC_MISS_sum"]), "requests_per_launch": req, "tcp_read_requests_per_launch": cin.get("TCP_TCC_READ_REQ_sum"),
                          "bytes_per_launch_upper_bound": req * 128.0, "achieved_upper_bound_GBps": req * 128.0 / (kernel_ms * 1e-3) / 1e9, "peak_GBps": 34500.0,
                          "frac_upper_bound": req * 128.0 / (kernel_ms * 1e-3) / 1e9 / 34500.0, "requests_per_query": req / float(B)}
                    secondary.append(l2)
                # (round 6) the request side: the rate at which the GPU serves RANDOM 64-byte row slots in this kernel's access shape (one 16-byte load per lane, three in
                # flight, a second 16 bytes for one row in four; 24 waves per CU) -- measured now with serenade_amd/bin/row_fetch_bench over a region that lives in one XCD's L2
                # (2 MB), one in the Infinity Cache (64 MB) and one far beyond both (4 GB), blended with the L2 hit rate measured above; the kernel fetches K rows per query
                try:
                    import subprocess as _sp
                    from serenade_amd import build as _bld
                    exe_rf = _bld.ROW_FETCH_BENCH
                    if os.path.exists(exe_rf) and args.measure_traffic:   # (not in the counter passes' child runs of this script)
                        torch.cuda.synchronize()
                        out_rf = _sp.run([exe_rf], capture_output=True, text=True, timeout=120).stdout
                        ceil = {}
                        for ln in out_rf.splitlines():
                            if ln.startswith("{"):
                                jj = json.loads(ln)["row_gather_ceiling"]; ceil[int(jj["region_mb"])] = float(jj["g_rows_per_s"]) * 1e9
                        if len(ceil) == 3:
                            hit = l2["hit_rate"] if l2 else 0.95
                            c_hit, c_mall, c_miss = ceil[min(ceil)], ceil[sorted(ceil)[1]], ceil[max(ceil)]
                            blended = 1.0 / (hit / c_hit + (1.0 - hit) / c_miss)
                            rows_per_launch = float(dbg["stats"][:, 2].astype(np.float64).mean()) * B * (fast_share if fast_used else 1.0)   # K: neighbours = rows fetched
                            ach_rows = rows_per_launch / (kernel_ms * 1e-3)
                            secondary.append({"bound": "row_gather", "unit": "random 64-byte row slots per second, chip-wide, in the kernel's access shape", "achieved": ach_rows,
                                              "ceiling_l2_resident": c_hit, "ceiling_infinity_cache": c_mall, "ceiling_hbm": c_miss, "l2_hit_rate_used": hit, "peak": blended, "frac": ach_rows / blended,
                                              "peak_note": "harmonic blend: hits at the L2-resident rate, misses at the HBM rate (at the Infinity-Cache rate: %.3g)" % (1.0 / (hit / c_hit + (1.0 - hit) / c_mall)),
                                              "rows_per_query": rows_per_launch / float(B), "measured_in_this_run": True,
                                              "note": "the neighbours' rows are the kernel's scattered requests (a query's posting lists, record and hand-off are coalesced, its resolve fetches few); "
                                                      "a request that hits the L2 costs a CU ~2.4 cycles of its request path, one that misses 10-14"})
                except Exception:
                    pass
                secondary = {"entries": secondary, "source": "rocprofv3 --pmc passes of this command at the timed batch size" if sq_in_run else os.path.relpath(cand[-1], ROOT),
                             "measured_in_this_run": bool(sq_in_run), "queries_per_dispatch": int(B) if sq_in_run else None,
                             "note": "no single unit is saturated: the kernel is held by dependent LDS / HBM round trips on three workgroups per CU and by issue-slot contention between them (DESIGN.md 4.1); "
                                     "what moved it in round 5 was memory locality -- the serving order -- not a unit's throughput"}
        except Exception:
            secondary = None

        result = dict(common)
        result.update({
            "value": args.gpus * args.steps * B / elapsed, "ms_per_step": elapsed / args.steps * 1e3, "scaling": "weak",
            "config": {"workload": "BASELINE configs[2]: synthetic %d interactions / %d items, k=%d m=%d idf_weighting=%g "
                                   "last_items=%d how_many=%d" % (inter, n_items, k, m, idfw, last_items, how_many)
                                   if args.config == "cfg3" else "synth.CONFIGS[%s]" % args.config,
                       "name": args.config, "batch_per_gpu": B, "query_pool_batches": args.pool,
                       "sessions": int(info["n_sessions_kept"]), "items": int(info["n_items"]), "interactions": int(info["nnz_rows"]),
                       "posting_entries": int(info["nnz_postings"]), "index_bytes_hbm": int(info["device_bytes"]),
                       "parallelism": "query-sharded replicas x%d (no data-path collective)" % args.gpus,
                       "setup_s": {"generate": round(t_gen, 2), "index_build_upload": round(t_build, 2), "index_builder": args.builder if avro is None else "avro loader"},
                       "index": "csr (built by this library)" if avro is None else "avro (pre-built: VMISIndex::new, vmis_index.rs:85-314)",
                       "timestamps": "unique" if args.tie_per_second <= 1 else "~%d sessions per timestamp value" % args.tie_per_second,
                       "max_session_len": args.max_session_len if avro is None else None,
                       "avro": None if avro is None else {
                           "producer_tie_order": avro["producer"], "producer_max_session_len": args.producer_max_len, "file_bytes": avro["file_bytes"],
                           "write_s": round(avro["write_s"], 2), "load_parse_infer_upload_s": round(avro["load_s"], 2),
                           "sessions_in_the_session_index": int(info["n_sessions_total"]), "sessions_named_by_some_list": int(info["n_sessions_kept"]),
                           "incomplete_items": int(info["incomplete_items"]),
                           "tie_order_inference": "off (SRN_AVRO_NO_TIE_INFERENCE)" if os.environ.get("SRN_AVRO_NO_TIE_INFERENCE") else "on",
                           "queries_of_the_last_step_on_the_general_kernel": int(general_last), "share_on_the_fast_kernels": (nq_last - general_last) / float(max(1, nq_last)),
                           "checker": "oracle restatement of VMISIndex::new (orc_index_from_parts): lists, idf, flags as given; ties among equal timestamps in the order the index serves with (srn_index_session_recency)"}},
            "parity_checked": parity_checked, "parity_checked_positions": "uniform over batch (seeded permutation of the full-size launch's rows, its first and last 32 included)", "full_batch_properties_ok": props_ok,
            "roofline": {"bound": "hbm", "kernel": "vmis_fast_kernel" if fast_used else "vmis_predict_kernel", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_unit": "bytes per launch (2*FETCH_SIZE + WRITE_SIZE)",
                         "frac_counter": (traffic / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if traffic else None,
                         "frac_counter_note": "measured HBM traffic of the launch / its duration / 8 TB/s: what the memory system really moves (frac prices the contract's algorithmic bytes)",
                         "traffic_source": traffic_src, "traffic_measured_in_this_run": traffic_in_run,
                         "traffic_note": None if traffic_in_run else "FALLBACK: read back from the committed PMC summary named in traffic_source (the in-run rocprofv3 --pmc passes were switched off or failed)",
                         "measured_copy_gbs": copy_gbs, "frac_measured_copy": achieved / copy_gbs,
                         "algorithmic_bytes_per_query": float(bq.mean()), "queries_per_launch": B,
                         "queries_served_by_this_kernel": int(nq_last - general_last) if fast_used else int(nq_last),
                         "algorithmic_bytes_per_launch": kernel_bytes,
                         "kernel_ms_avg": kernel_ms, "kernel_ms_min": float(t_fast.min()) if fast_used else float(t_pred.min()),
                         "other_launches_ms_avg": {"prep_kernel": float(t_prep.mean()), "general_kernel_over_handed_over_queries_plus_finish_kernel": float((t_pred - t_fast).mean()) if fast_used else 0.0,
                                                   "global_table_retry_pass": float(t_retry.mean())},
                         "queries_handed_to_general_kernel_last_step": int(general_last), "queries_via_global_table_pass_last_step": int(global_last),
                         "whole_step": {"achieved": step_achieved, "frac": step_achieved / HBM_PEAK_GBS, "note": "all launches of a step (prep + fast + general + finish kernels) against the same algorithmic bytes"},
                         "queries_via_global_table_pass_in_sample": retried, "stats_sample_queries": nstat},
            "roofline_secondary": secondary,
            "latency": {"step_ms_p50": float(np.percentile(step_ms, 50)), "step_ms_p90": float(np.percentile(step_ms, 90)),
                        "single_query_us_p50": float(np.percentile(lat_single, 50)) if lat_single is not None else None,
                        "single_query_us_p90": float(np.percentile(lat_single, 90)) if lat_single is not None else None,
                        "single_query_note": "srn_predict called through ctypes with preallocated buffers (round 6; rounds 1-5: through serenade_amd.predict, ~9 us of Python per call more): the one-launch latency path",
                        "single_query_resident_workgroup": None if (lat_single is None or lat_resident is None) else (lat_resident if "error" in lat_resident else {
                            "us_p50": float(np.percentile(lat_resident["us"], 50)), "us_p90": float(np.percentile(lat_resident["us"], 90)), "us_p99": float(np.percentile(lat_resident["us"], 99)),
                            "answered_without_a_launch": lat_resident["answered_without_a_launch"], "sent_to_the_launch_path": lat_resident["sent_to_the_launch_path"],
                            "note": "srn_predict (ctypes, preallocated buffers) with one resident workgroup of the persistent latency path parked on the GPU (srn_index_serve_start): no kernel launch per call; C++ host: profiles/r06_latency_resident_cfg3.json"}),
                        "batch_sweep": sweep,
                        "long_sessions": long_sessions,
                        "note": "batch_sweep: srn_predict_batch_device on resident buffers (HIP events) vs srn_predict_batch on host buffers (pageable numpy arrays, result buffers "
                                "reused between calls: upload + launches + download, wall clock; <= 256 sessions: zero-copy latency path, above: chunked pipeline); "
                                "single_query = srn_predict (host pointers, one evolving session per call, PCIe-inclusive)"},
            "queries_served_last_step": served,
        })

        if args.gpus == 1 and not args.no_cpu_baseline:
            # 4. the oracle is used here ONLY as the timed CPU baseline (literal restatement of the reference loops)
            oix = oracle_index()
            t_obuild = oracle_box["t_build"]
            cores = usable_cores()
            probe_n = min(B, 64 * cores)
            r = oix.predict_batch("literal", flat0[:qo0[probe_n]], qo0[:probe_n + 1], k, m, how_many, False, threads=cores, want_results=False)
            rate = probe_n / max(r["elapsed"], 1e-6)
            n_cpu = int(min(B, max(probe_n, rate * args.cpu_seconds)))
            r = oix.predict_batch("literal", flat0[:qo0[n_cpu]], qo0[:n_cpu + 1], k, m, how_many, False, threads=cores,
                                  want_results=False, want_latency=True)
            lat_cpu = r["lat_us"]
            # ONE thread, one query per call, per-call microseconds -- the reference evaluator's report (src/bin/evaluator.rs:82-89, src/stopwatch.rs:28-52;
            # there: whole microseconds through a t-digest(100) estimate, here exact quantiles of the same per-call durations)
            n_one = int(min(n_cpu, max(256, rate / cores * min(args.cpu_seconds, 6.0))))
            r1 = oix.predict_batch("literal", flat0[:qo0[n_one]], qo0[:n_one + 1], k, m, how_many, False, threads=1, want_results=False, want_latency=True)
            one = {"p%s" % str(q).replace(".", "_"): float(np.percentile(r1["lat_us"], q)) for q in (25, 50, 75, 90, 95, 99.5)}
            one.update({"queries": n_one, "seconds": float(r1["elapsed"]), "queries_per_s": n_one / r1["elapsed"],
                        "note": "one host thread, one evolving session per call like evaluator.rs:46-76; the percentiles the reference prints (p25/50/75/90/95/99.5, microseconds)"})
            # What the canonical refinement costs against the literal loops AT THIS CONFIG: the first n_lvc queries of the timed batch through both
            # restatements and through the product, the evaluator's Mrr@20 / HitRate@20 against the held-out next item of each query
            from oracle import refinement as RF
            n_lvc = int(min(n_cpu, 32768))
            hip_rows = sa.predict_batch(index, (flat0[:qo0[n_lvc]], qo0[:n_lvc + 1]), k, m, how_many, False)
            t1 = time.time()
            lvc = RF.literal_vs_canonical(oix, flat0[:qo0[n_lvc]], qo0[:n_lvc + 1], next0[:n_lvc], k, m, how_many, threads=cores, hip=hip_rows)
            lvc["seconds"] = round(time.time() - t1, 2)
            lvc["sample"] = "first %d queries of the timed batch" % n_lvc
            result["literal_vs_canonical"] = lvc
            result["cpu_baseline"] = {
                "single_thread_per_call_us": one,
                "value": n_cpu / r["elapsed"], "unit": "queries/s", "cores": cores, "kind": "port",
                "sample": "first %d queries of the same batch, %d threads over one shared read-only index (%.1f s); "
                          "oracle/vmis_oracle.cpp literal restatement of the reference's Rust loops, not the Rust binary"
                          % (n_cpu, cores, r["elapsed"]),
                "per_call_us_p50": float(np.percentile(lat_cpu, 50)), "per_call_us_p90": float(np.percentile(lat_cpu, 90)),
                "index_build_s": round(t_obuild, 2)}
        else:
            result["cpu_baseline"] = None
        result["_parity_checked"] = parity_checked; result["_props_ok"] = props_ok; result["_B"] = B
        return result

    def local_g8_block():
        """N = 1: what ONE rank of an 8-way item-sharded index does per batch, measured every round by the driver's own run: the index cut in 8, all
        shards in this process on the one GPU (srn_shard_group_create_local), the NEIGHBOURS pipeline -- the one a multi-GPU run takes -- with the unsharded index as the
        replicated postings; HIP events around shard 0's own launches (SRN_GROUP_TIMING: the measurement form synchronises per batch).  The collectives degenerate to
        kernels: their cost over xGMI is NOT in it; the projected node rate is batch / (shard 0's front + back + merge), i.e. one batch stream with free exchanges."""
        import ctypes as C
        from serenade_amd import capi as _capi
        from serenade_amd import sharded as SH8
        Gl, Bl = 8, int(min(args.shard_batch, 1 << 17))
        os.environ["SRN_GROUP_TIMING"] = "1"
        t0 = time.time()
        shards8 = [SH8.ShardedVMISIndex.from_full(index, g, Gl, device=local_rank) for g in range(Gl)]
        grp8 = SH8.ShardGroup.local(shards8)
        os.environ.pop("SRN_GROUP_TIMING", None)
        grp8.set_postings(index)
        t_setup = time.time() - t0
        b8 = draw_batches(Bl, 1, 0)[0]
        out8 = (torch.empty((Bl, how_many), dtype=torch.int64, device=dev), torch.empty((Bl, how_many), dtype=torch.float64, device=dev), torch.empty(Bl, dtype=torch.int32, device=dev))
        times = []
        for it in range(7):
            grp8.predict_batch(b8[0], b8[1], Bl, last_items, k, m, how_many, False, stream.cuda_stream, out=out8)
            torch.cuda.synchronize()
            t3 = (C.c_double * 3)()
            _capi.check(_capi.lib().srn_debug_shard_group_times(grp8._h, t3))
            times.append(list(t3))
        t = np.median(np.array(times[2:]), axis=0)
        checked = 0
        if args.parity > 0:
            pos = gate_positions(Bl, min(args.parity, 1024))
            checked = gate(out8[0].cpu().numpy().view(np.uint64)[pos], out8[1].cpu().numpy()[pos], out8[2].cpu().numpy().view(np.uint32)[pos], b8[2], b8[3], pos, "8 local shards, neighbours pipeline")
        st8 = grp8.stats
        blk = {"n_shards": Gl, "batch": Bl, "pipeline": "neighbours" if st8["neighbour_batches"] else "lists",
               "rank0_ms": {"prep_and_front_end_over_1_of_%d_of_the_batch" % Gl: float(t[0]), "back_end_over_the_whole_batch": float(t[1]), "topn_merge": float(t[2])},
               "rank0_ms_total": float(t.sum()), "projected_node_queries_per_s_without_exchanges": Bl / (float(t.sum()) * 1e-3),
               "ratio_to_one_unsharded_gpu": (Bl / (float(t.sum()) * 1e-3)) / (result["value"] if result is not None else float("nan")),
               "exchange_bytes_per_query_and_rank": {"neighbour_lists_all_gather": (k + 1) * 4 / Gl, "topn_all_gather": 16 * how_many + 4},
               "shard0_bytes_hbm": int(shards8[0].info["device_bytes"]), "parity_checked": checked, "parity_checked_positions": "uniform over batch", "setup_s": round(t_setup, 2),
               "note": "all 8 shards on ONE GPU, collectives degenerate to kernels: what a rank computes per batch, not what xGMI costs; results checked against the oracle"}
        # ---- the exchange term: the same rank once more in the STREAMING form (neighbours shipped as posting positions: a third of the bytes, more
        # compute), then both forms priced with what their exchanges ship per rank over xGMI.  A MODEL: no collective of this library has crossed xGMI yet (SCALE runs skipped).
        try:
            grp8.set_postings(None)
            os.environ["SRN_SBACK_STREAM"] = "1"; os.environ["SRN_GROUP_TIMING"] = "1"; _capi.reload_knobs()
            grp8.set_postings(index)
            times_s = []
            for it in range(7):
                grp8.predict_batch(b8[0], b8[1], Bl, last_items, k, m, how_many, False, stream.cuda_stream, out=out8)
                torch.cuda.synchronize()
                t3 = (C.c_double * 3)()
                _capi.check(_capi.lib().srn_debug_shard_group_times(grp8._h, t3))
                times_s.append(list(t3))
            ts_ = np.median(np.array(times_s[2:]), axis=0)
            streamed = grp8.stats["bytes_neighbours"] > st8["bytes_neighbours"]
            checked_s = 0
            if args.parity > 0:
                pos = gate_positions(Bl, min(args.parity, 512))
                checked_s = gate(out8[0].cpu().numpy().view(np.uint64)[pos], out8[1].cpu().numpy()[pos], out8[2].cpu().numpy().view(np.uint32)[pos], b8[2], b8[3], pos, "8 local shards, streaming back end")
            # bytes ONE rank sends to EACH of its G - 1 peers per batch (and receives from each): its slice of the neighbour exchange + its partial top-n of every query
            per_q_gather, per_q_stream, per_q_topn = (k + 1) * 4, int(_capi.lib().srn_debug_shard_nb_positions_stride(k, m)) * 4, 16 * how_many + 4
            out_gather = Bl / Gl * per_q_gather + Bl * per_q_topn
            out_stream = Bl / Gl * per_q_stream + Bl * per_q_topn
            rates = {"per_link_and_direction_GBps_conservative": 76.8, "per_link_and_direction_GBps_optimistic": 153.6}
            model = {"source_of_the_rate": "the round's task statement and SURVEY.md section 5: xGMI is point-to-point, 7 links x ~153 GB/s per GPU (one link per peer in an 8-GPU node); "
                                           "conservative = that figure read as both directions together (76.8 GB/s each way), optimistic = per direction",
                     "bytes_to_each_peer_per_batch": {"gather": int(out_gather), "streaming": int(out_stream)},
                     "bytes_received_per_rank_and_batch": {"gather": int(out_gather * (Gl - 1)), "streaming": int(out_stream * (Gl - 1))},
                     "rank_compute_ms": {"gather": float(t.sum()), "streaming": float(ts_.sum()), "streaming_form_really_ran": bool(streamed), "streaming_parity_checked": checked_s}}
            for name, gbps in rates.items():
                xg, xs = out_gather / (gbps * 1e9) * 1e3, out_stream / (gbps * 1e9) * 1e3   # every peer pair has its own link: the 7 transfers of a rank run side by side
                model[name] = {"GBps": gbps, "exchange_ms": {"gather": xg, "streaming": xs},
                               "projected_node_queries_per_s": {"gather_not_overlapped": Bl / ((float(t.sum()) + xg) * 1e-3), "streaming_not_overlapped": Bl / ((float(ts_.sum()) + xs) * 1e-3),
                                                                "gather_overlapped": Bl / (max(float(t.sum()), xg) * 1e-3), "streaming_overlapped": Bl / (max(float(ts_.sum()), xs) * 1e-3)}}
            model["what_the_library_does"] = ("SRN_SBACK_STREAM unset (round 6): a group with real peers whose exchanges are NOT overlapped (the default) takes the form with the lower modelled total -- "
                                              "streaming iff the bytes it saves per query and link / SRN_XGMI_GBPS (default 76.8 GB/s per direction) exceed the 8.5 ns of extra compute per query (at the default rate: 6.45 ns saved -- the gather form); "
                                              "with srn_shard_group_set_overlap(1) the gather form (its smaller compute decides)")
            blk["exchange_model"] = model
        except Exception as e:   # (the block is an extra: its failure must not cost the line)
            blk["exchange_model"] = {"error": repr(e)[:300]}
        finally:
            os.environ.pop("SRN_SBACK_STREAM", None); os.environ.pop("SRN_GROUP_TIMING", None); _capi.reload_knobs()
        grp8.close()
        for s8 in shards8:
            s8.close()
        return blk

    # ---- the phases.  Replicas first (no data-path collective: nothing in it can hang on a peer); the item-sharded phase runs under a watchdog, and if it
    # fails or stalls the line that is printed is the replicas' with the reason -- a SCALE run never ends without a line. ----
    result = replicas_phase() if do_rep else None
    rep_extra = {}
    if rank == 0 and result is not None:
        rep_extra = {"parity_checked": result.pop("_parity_checked"), "props_ok": result.pop("_props_ok"), "B": result.pop("_B")}

    def make_line(shard_line, shard_error=None, sb=None):
        """The ONE line (rank 0).  Every line carries value_replicas and value_item_sharded (null where a mode did not run) and value_mode = which of them `value` is:
        N = 1 the replicas figure (BASELINE's metric on one GPU), N > 1 the item-sharded figure (the north star's partitioning)."""
        v_rep = result["value"] if result is not None else None
        v_sh = shard_line["value"] if shard_line is not None else None
        if shard_line is not None and (world > 1 or result is None):
            line = dict(shard_line)
            line["value_mode"] = "item-sharded"
            if result is not None:
                line["replicas"] = {"value": result["value"], "ms_per_step": result["ms_per_step"], "scaling": "weak", "batch_per_gpu": rep_extra["B"], "parallelism": result["config"]["parallelism"],
                                    "parity_checked": rep_extra["parity_checked"], "full_batch_properties_ok": rep_extra["props_ok"],
                                    "kernel": {kk: result["roofline"][kk] for kk in ("kernel", "achieved", "frac", "kernel_ms_avg", "algorithmic_bytes_per_query")},
                                    "note": "every GPU holds the whole index and serves its own slice of the query stream: no data-path collective, the throughput ceiling of any index that fits 288 GB"}
                line["cpu_baseline"] = result["cpu_baseline"]
            else:
                cpu = None
                if world == 1 and args.full and not args.no_cpu_baseline and sb is not None:
                    cores = usable_cores()
                    n_cpu = int(min(args.shard_batch, 4096))
                    r = oracle_index().predict_batch("literal", sb[0][2][:sb[0][3][n_cpu]], sb[0][3][:n_cpu + 1], k, m, how_many, False, threads=cores, want_results=False)
                    cpu = {"value": n_cpu / r["elapsed"], "unit": "queries/s", "cores": cores, "kind": "port",
                           "sample": "first %d queries of the same batch, %d threads (%.1f s); oracle/vmis_oracle.cpp literal restatement" % (n_cpu, cores, r["elapsed"])}
                line["cpu_baseline"] = cpu
        elif result is not None:
            line = dict(result)
            line["value_mode"] = "replicas"
            if shard_line is not None:     # N = 1, both modes: the group of one shard beside the fused path
                line["item_sharded"] = {kk: shard_line[kk] for kk in ("value", "ms_per_step", "steps", "scaling", "parity_checked", "queries_served_last_step", "exchange_bytes_per_query_rank0", "latency")}
                line["item_sharded"].update({"batch": shard_line["config"]["batch"], "parallelism": shard_line["config"]["parallelism"], "rccl_ranks": shard_line["config"]["rccl_ranks"],
                                             "transport": shard_line["config"]["transport"], "exchange_overlapped_with_previous_batch": shard_line["config"]["exchange_overlapped_with_previous_batch"],
                                             "setup_s": shard_line["config"]["setup_s"], "roofline_whole_step_frac": shard_line["roofline"]["frac"],
                                             "ratio_to_replicas_time": (result["value"] / shard_line["value"]) if shard_line["value"] else None})
            elif do_shard:
                line["item_sharded_error"] = shard_error
        else:
            line = dict(common, value=None, value_mode=None, item_sharded_error=shard_error)
        line["value_replicas"], line["value_item_sharded"] = v_rep, v_sh
        line["full"] = bool(args.full)
        return line

    shard_line, shard_error, sb = None, None, None
    if do_shard:
        import threading

        def give_up():
            if rank == 0:
                line = pending["line"] if pending["line"] is not None else \
                    make_line(None, "the item-sharded phase did not finish within %d s; this line is the replicas mode alone" % args.shard_timeout)
                print(json.dumps(line)); sys.stdout.flush()
            os._exit(0)
        wd = threading.Timer(args.shard_timeout + (0 if rank == 0 else 10), give_up)
        wd.daemon = True
        wd.start()
        try:
            shard_line, sb = sharded_phase(make_line)
        except Exception as e:   # (RCCL missing, communicator creation failed, ...): say so in the line instead of dying without one
            import traceback
            traceback.print_exc()
            shard_error = repr(e)
        wd.cancel()
    g8 = None
    if rank == 0 and world == 1 and index is not None and args.full and not args.no_local_g8 and args.config in ("cfg3", "cfg2", "tiny", "small"):
        try:
            g8 = local_g8_block()
        except Exception as e:
            import traceback
            traceback.print_exc()
            g8 = {"error": repr(e)}
    if rank == 0:
        final_line = make_line(shard_line, shard_error, sb)
        if g8 is not None:
            final_line.setdefault("item_sharded", {})["local_g8"] = g8
        print(json.dumps(final_line))
        sys.stdout.flush()
    if shard_error is not None:      # (a communicator in an unknown state: its teardown may wait for peers that are gone -- the line is out, leave)
        sys.stderr.flush()
        os._exit(0)
    with c_stdout_to_stderr():
        if group is not None:
            group.close()
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
