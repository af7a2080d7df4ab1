"""Training-data loading, host against GPU, on BASELINE-shaped TSV files (README "Loading training data on the GPU").

    python tools/ingest_bench.py [--configs cfg2,cfg3] [--dir DIR] [--gpu-only] [--no-index]

For each config, writes a training TSV from synth.training_sessions (rows shuffled, times with .0 / .5 decimals, ~1 % duplicate rows, a few
unparsable lines), reads it once to warm the page cache, then times in this process:
  * srn_sessions_from_tsv (host) against srn_sessions_from_tsv_gpu, with the GPU loader's stage breakdown, and asserts identical sessions;
  * VMISIndex.new_from_csv end to end, loader="host" against loader="gpu" (both build on the GPU), and asserts equal index info.
Prints one JSON line.  --gpu-only skips the host side (for a profiler run of the GPU loader's kernels).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import serenade_amd as sa  # noqa: E402
from serenade_amd import synth  # noqa: E402
from serenade_amd.ingest import TrainingSessions  # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def _warm(path):
    with open(path, "rb") as f:
        while f.read(1 << 24):
            pass


def run_config(name, d, gpu_only, index):
    inter, n_items, k, m, idfw = synth.CONFIGS[name]
    path = os.path.join(d, "train_%s.tsv" % name)
    t0 = time.perf_counter()
    off, items, ts = synth.training_sessions(inter, n_items)
    s, it, t = synth.training_events(off, items, ts)
    synth.write_training_tsv(path, s, it, t, bad_lines=8)
    del off, items, ts, s, it, t
    res = {"config": name, "file_bytes": os.path.getsize(path), "write_s": round(time.perf_counter() - t0, 1)}
    _warm(path)
    TrainingSessions.from_tsv(path, loader="gpu").close()          # first use of the device: runtime start-up, code objects
    g, ms_gpu = _timed(lambda: TrainingSessions.from_tsv(path, loader="gpu"))
    info = g.load_info()
    res.update(rows=info["rows"], lines=info["lines"], host_parsed=info["host_parsed"], ms_gpu_loader=round(ms_gpu, 1),
               gpu_stages_ms={k2: round(info[k2], 2) for k2 in ("ms_read", "ms_upload", "ms_parse", "ms_group", "ms_download")})
    garr = g.arrays()
    res["sessions"] = len(garr[0]) - 1
    g.close()
    if not gpu_only:
        h, ms_host = _timed(lambda: TrainingSessions.from_tsv(path, loader="host"))
        harr = h.arrays()
        h.close()
        assert all(np.array_equal(a, b) for a, b in zip(garr, harr)), "GPU and host loaders disagree"
        res.update(ms_host_loader=round(ms_host, 1), loader_speedup=round(ms_host / ms_gpu, 2), identical_sessions=True)
    del garr
    if index:
        gi, ms_gi = _timed(lambda: sa.VMISIndex.new_from_csv(path, m, idfw, device=0, loader="gpu"))
        res["ms_new_from_csv_gpu"] = round(ms_gi, 1)
        if not gpu_only:
            hi, ms_hi = _timed(lambda: sa.VMISIndex.new_from_csv(path, m, idfw, device=0, loader="host"))
            assert hi.info == gi.info, "index info differs"
            res.update(ms_new_from_csv_host=round(ms_hi, 1), new_from_csv_speedup=round(ms_hi / ms_gi, 2), identical_index_info=True)
            hi.close()
        gi.close()
    os.remove(path)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg3")
    ap.add_argument("--dir", default=None, help="where the TSV files go (default: a temporary directory)")
    ap.add_argument("--gpu-only", action="store_true")
    ap.add_argument("--no-index", action="store_true")
    a = ap.parse_args(argv)
    out = {"tool": "ingest_bench", "results": []}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for name in a.configs.split(","):
            r = run_config(name, d, a.gpu_only, not a.no_index)
            print("# %s" % json.dumps(r), file=sys.stderr, flush=True)
            out["results"].append(r)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
