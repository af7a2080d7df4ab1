"""The split of a click log, the evaluation set built from events and one backtest fold on one GPU, next to their yardsticks (README "From a click log to evaluated folds").

    python tools/prepare_bench.py [--config cfg3] [--reps 5] [--test-share 0.01] [--no-host] [--out profiles/prepare_cfg3.json]
    python tools/prepare_bench.py --resident [--config cfg3] [--reps 5] [--out profiles/resident_build_cfg3.json]

The rows are synth.training_events of the config's training sessions (shuffled, f64 times on half seconds, ~1 % repeated rows), resident on the device.  Medians of
--reps runs, milliseconds of wall time around a synchronised device:
  * split_events on the device tensors, against a device-to-device copy of the three input columns (the traffic floor of ONE pass over the rows) and against
    split_model on the host (one run);
  * the same split with k_side's plain atomics (SRN_SPLIT_NO_COMBINE=1) instead of the block's LDS combining of equal items;
  * EvalSet.from_events on the split's two sides, against EvalSet.from_tsv on files written from the same rows (one run);
  * one backtest fold end to end, against the device time of its evaluate alone.
The cutoff leaves --test-share of the sessions on the test side.  Prints one JSON line and, with --out, writes it there.

--resident measures the index build alone (README "The index build without the host round trip"), on the same split's training side, the two builders alternating
run by run: VMISIndex.from_events with builder="gpu" and with builder="resident" (for the latter the library's own stage times, medians too), the peak of device
memory above the level before the call (sampled from a second thread), one backtest fold under each builder, and the first save of a resident index next to the
save of a "gpu" one -- the deferred download, so that its cost is shown and not hidden.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import serenade_amd as sa  # noqa: E402
from serenade_amd import capi, prepare, synth  # noqa: E402
from serenade_amd.evaluation import EvalSet, evaluate  # noqa: E402


def say(msg):
    print("# " + msg, file=sys.stderr, flush=True)


def timed(fn, reps, sync):
    ms, out = [], None
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, round(statistics.median(ms), 3), [round(x, 3) for x in ms]


class PeakSampler:
    """Device memory in use above the level at start, sampled every millisecond from a second thread while the builder runs inside the library."""

    def __init__(self, torch, dev):
        import threading
        self.torch, self.dev, self.stop = torch, dev, threading.Event()
        self.base = torch.cuda.mem_get_info(dev)[0]
        self.low = self.base
        self.thread = threading.Thread(target=self.run, daemon=True)

    def run(self):
        while not self.stop.is_set():
            self.low = min(self.low, self.torch.cuda.mem_get_info(self.dev)[0])
            time.sleep(0.001)

    def __enter__(self):
        self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop.set()
        self.thread.join()
        self.low = min(self.low, self.torch.cuda.mem_get_info(self.dev)[0])

    @property
    def peak(self):
        return int(self.base - self.low)


def resident_section(res, d, sp, trial, m, idfw, cutoff, reps, sync, torch, dev):
    """from_events, one fold and the first save under builder="gpu" and builder="resident", alternating."""
    med = lambda v: round(statistics.median(v), 3)   # noqa: E731
    arms = ("gpu", "resident")
    for b in arms:                                      # first use of each path: code objects, allocator
        sa.VMISIndex.from_events(*sp.train, m, idfw, device=0, builder=b).close()
    build = {b: [] for b in arms}
    peak = {b: [] for b in arms}
    stages = []
    infos = {}
    for _ in range(reps):
        for b in arms:
            sync()
            with PeakSampler(torch, dev) as ps:
                t0 = time.perf_counter()
                ix = sa.VMISIndex.from_events(*sp.train, m, idfw, device=0, builder=b)
                sync()
                build[b].append((time.perf_counter() - t0) * 1e3)
            peak[b].append(ps.peak)
            infos[b] = {k: v for k, v in ix.info.items() if k != "device_bytes"}
            if b == "resident":
                stages.append(ix.host_state())
            ix.close()
    assert infos["gpu"] == infos["resident"], "the two builders disagree about the index"
    res.update(train_rows=int(sp.train[0].numel()), index=infos["gpu"])
    for b in arms:
        res["ms_from_events_" + b] = med(build[b])
        res["ms_from_events_%s_runs" % b] = [round(x, 3) for x in build[b]]
        res["peak_device_bytes_" + b] = int(max(peak[b]))
    res["resident_stages_ms"] = {k: med([st[k] for st in stages]) for k in ("ms_upload", "ms_group", "ms_quantile", "ms_build", "ms_items", "ms_attach")}
    res["resident_build_bytes_on_device"] = int(stages[-1]["build_bytes_on_device"])
    res["from_events_gpu_over_resident"] = round(res["ms_from_events_gpu"] / res["ms_from_events_resident"], 2)
    say("from_events: gpu %s ms, resident %s ms, stages %s" % (res["ms_from_events_gpu"], res["ms_from_events_resident"], res["resident_stages_ms"]))

    # the first save: for a resident index it holds the deferred download
    save = {b: [] for b in arms}
    down = []
    with tempfile.TemporaryDirectory() as tmp:
        for r in range(reps):
            for b in arms:
                ix = sa.VMISIndex.from_events(*sp.train, m, idfw, device=0, builder=b)
                sync()
                t0 = time.perf_counter()
                ix.save(os.path.join(tmp, b + ".idx"))
                save[b].append((time.perf_counter() - t0) * 1e3)
                if b == "resident":
                    down.append(ix.host_state()["ms_materialize"])
                ix.close()
        import filecmp
        res["saved_files_identical"] = bool(filecmp.cmp(os.path.join(tmp, "gpu.idx"), os.path.join(tmp, "resident.idx"), shallow=False))
        res["saved_file_bytes"] = os.path.getsize(os.path.join(tmp, "gpu.idx"))
    for b in arms:
        res["ms_first_save_" + b] = med(save[b])
        res["ms_first_save_%s_runs" % b] = [round(x, 3) for x in save[b]]
    res["ms_deferred_download"] = med(down)
    say("first save: gpu %s ms, resident %s ms of which the download %s ms" % (res["ms_first_save_gpu"], res["ms_first_save_resident"], res["ms_deferred_download"]))

    # one fold end to end under each builder
    fold = lambda b: prepare.backtest(d, trial, m, idfw, cutoffs=[cutoff], test_span=1 << 40, builder=b)   # noqa: E731
    folds = {b: [] for b in arms}
    ev = {}
    for b in arms:
        fold(b)
    for _ in range(reps):
        for b in arms:
            sync()
            t0 = time.perf_counter()
            out = fold(b)
            sync()
            folds[b].append((time.perf_counter() - t0) * 1e3)
            r = out[0]["reports"][0]
            ev[b] = ({k: v for k, v in r.items() if not k.startswith("ms_")}, r["ms_predict"] + r["ms_eval"])
    res["fold_reports_identical"] = bool(ev["gpu"][0] == ev["resident"][0])
    for b in arms:
        res["ms_backtest_fold_" + b] = med(folds[b])
        res["ms_backtest_fold_%s_runs" % b] = [round(x, 3) for x in folds[b]]
        res["fold_ms_evaluate_" + b] = round(ev[b][1], 3)
    res["fold_gpu_over_resident"] = round(res["ms_backtest_fold_gpu"] / res["ms_backtest_fold_resident"], 2)
    res["resident_fold_beside_build_and_evaluate_ms"] = round(res["ms_backtest_fold_resident"] - res["ms_from_events_resident"] - res["fold_ms_evaluate_resident"], 3)
    say("fold: gpu %s ms, resident %s ms" % (res["ms_backtest_fold_gpu"], res["ms_backtest_fold_resident"]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--test-share", type=float, default=0.01)
    ap.add_argument("--no-host", action="store_true", help="skip split_model and EvalSet.from_tsv (the host yardsticks)")
    ap.add_argument("--resident", action="store_true", help="the index build alone: builder='gpu' against builder='resident' (from_events, one fold, the first save)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import torch
    dev = torch.device("cuda", 0)
    sync = lambda: torch.cuda.synchronize(dev)
    inter, n_items, k, m, idfw = synth.CONFIGS[a.config]
    t0 = time.perf_counter()
    off, items, ts = synth.training_sessions(inter, n_items)
    s, it, t = synth.training_events(off, items, ts)
    cutoff = int(np.quantile(ts, 1.0 - a.test_share))
    del off, items, ts
    res = {"tool": "prepare_bench --resident" if a.resident else "prepare_bench", "config": a.config, "rows": int(len(s)), "reps": a.reps, "generate_s": round(time.perf_counter() - t0, 1)}
    say("rows generated: %s" % res)
    rule = dict(cutoff=cutoff, min_item_support=5, min_session_len=2, test_known_items=True)
    d = tuple(torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev) for x in (s, it, t))
    sync()
    if a.resident:
        sp = prepare.split_events(*d, **rule)
        resident_section(res, d, sp, [dict(k=k, m=m, max_items_in_session=synth.LAST_ITEMS)], m, idfw, cutoff, a.reps, sync, torch, dev)
        line = json.dumps(res)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0

    # the split
    prepare.split_events(*d, **rule)                                  # first use: code objects, allocator
    sp, ms_split, all_split = timed(lambda: prepare.split_events(*d, **rule), a.reps, sync)
    res.update(info=sp.info, ms_split_events=ms_split, ms_split_events_runs=all_split)
    _, ms_copy, _ = timed(lambda: [x.clone() for x in d], a.reps, sync)
    res.update(ms_copy_of_the_inputs=ms_copy, split_over_copy=round(ms_split / ms_copy, 2))
    say("split: %s ms, copy %s ms" % (ms_split, ms_copy))
    os.environ["SRN_SPLIT_NO_COMBINE"] = "1"
    capi.reload_knobs()
    plain, ms_plain, all_plain = timed(lambda: prepare.split_events(*d, **rule), a.reps, sync)
    del os.environ["SRN_SPLIT_NO_COMBINE"]
    capi.reload_knobs()
    assert plain.info == sp.info and torch.equal(plain.code, sp.code) and torch.equal(plain.pos.view(torch.int32), sp.pos.view(torch.int32))
    res.update(ms_split_events_plain_atomics=ms_plain, ms_split_events_plain_atomics_runs=all_plain)
    say("split with plain atomics: %s ms" % ms_plain)
    del plain
    if not a.no_host:
        t0 = time.perf_counter()
        code, pos, info = prepare.split_model(s, it, t, **rule)
        res["ms_split_model_host"] = round((time.perf_counter() - t0) * 1e3, 1)
        assert info == sp.info and np.array_equal(code, sp.code.cpu().numpy()) and np.array_equal(pos, sp.pos.cpu().numpy()), "the device split is not the model's"
        res.update(identical_to_the_model=True, split_speedup_over_host=round(res["ms_split_model_host"] / ms_split, 1))
        say("split_model on the host: %s ms" % res["ms_split_model_host"])
        del pos

    # the evaluation set
    index = sa.VMISIndex.from_events(*sp.train, m, idfw, device=0)
    trial = [dict(k=k, m=m, max_items_in_session=synth.LAST_ITEMS)]
    try:
        def make():
            es = EvalSet.from_events(index, sp.test, sp.train[1])
            es.close()
        make()
        _, ms_set, all_set = timed(make, a.reps, sync)
        res.update(ms_eval_set_from_events=ms_set, ms_eval_set_from_events_runs=all_set)
        say("EvalSet.from_events: %s ms" % ms_set)
        es = EvalSet.from_events(index, sp.test, sp.train[1])
        rep = evaluate(es, trial)[0]
        es.close()
        if not a.no_host:
            with tempfile.TemporaryDirectory() as tmp:
                secs = prepare.round_times(t)
                train, test = os.path.join(tmp, "train.tsv"), os.path.join(tmp, "test.tsv")
                synth.write_training_tsv(train, s[code == 1], it[code == 1], secs[code == 1])
                synth.write_training_tsv(test, s[code == 2], it[code == 2], secs[code == 2])
                t0 = time.perf_counter()
                ref = EvalSet.from_tsv(index, test, train)
                res["ms_eval_set_from_tsv"] = round((time.perf_counter() - t0) * 1e3, 1)
                ref_rep = evaluate(ref, trial)[0]
                ref.close()
            same = all(rep[key] == ref_rep[key] for key in ref_rep if not key.startswith("ms_"))
            res.update(eval_set_speedup_over_tsv=round(res["ms_eval_set_from_tsv"] / ms_set, 1), reports_identical_to_from_tsv=bool(same))
            say("EvalSet.from_tsv: %s ms, reports identical: %s" % (res["ms_eval_set_from_tsv"], same))
    finally:
        index.close()

    # one fold end to end
    fold = lambda: prepare.backtest(d, trial, m, idfw, cutoffs=[cutoff], test_span=1 << 40)
    fold()
    out, ms_fold, all_fold = timed(fold, a.reps, sync)
    r = out[0]["reports"][0]
    res.update(ms_backtest_fold=ms_fold, ms_backtest_fold_runs=all_fold, fold_ms_evaluate=round(r["ms_predict"] + r["ms_eval"], 3), fold_qty_evaluations=r["qty_evaluations"],
               fold_over_evaluate=round(ms_fold / (r["ms_predict"] + r["ms_eval"]), 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
