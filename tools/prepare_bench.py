"""The split of a click log, the evaluation set built from events and one backtest fold on one GPU, next to their yardsticks (README "From a click log to evaluated folds").

    python tools/prepare_bench.py [--config cfg3] [--reps 5] [--test-share 0.01] [--no-host] [--out profiles/prepare_cfg3.json]

The rows are synth.training_events of the config's training sessions (shuffled, f64 times on half seconds, ~1 % repeated rows), resident on the device.  Medians of
--reps runs, milliseconds of wall time around a synchronised device:
  * split_events on the device tensors, against a device-to-device copy of the three input columns (the traffic floor of ONE pass over the rows) and against
    split_model on the host (one run);
  * the same split with k_side's plain atomics (SRN_SPLIT_NO_COMBINE=1) instead of the block's LDS combining of equal items;
  * EvalSet.from_events on the split's two sides, against EvalSet.from_tsv on files written from the same rows (one run);
  * one backtest fold end to end, against the device time of its evaluate alone.
The cutoff leaves --test-share of the sessions on the test side.  Prints one JSON line and, with --out, writes it there.
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--test-share", type=float, default=0.01)
    ap.add_argument("--no-host", action="store_true", help="skip split_model and EvalSet.from_tsv (the host yardsticks)")
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
    res = {"tool": "prepare_bench", "config": a.config, "rows": int(len(s)), "reps": a.reps, "generate_s": round(time.perf_counter() - t0, 1)}
    say("rows generated: %s" % res)
    rule = dict(cutoff=cutoff, min_item_support=5, min_session_len=2, test_known_items=True)
    d = tuple(torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev) for x in (s, it, t))
    sync()

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
