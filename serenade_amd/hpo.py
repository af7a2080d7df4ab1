"""Hyper-parameter search over srn_evaluate: the reference's exhaustive_grid_search.rs and hyperparameter_search.rs on the GPU.

One index serves every m up to its m_index (posting lists are most-recent-first and the m-cut never admits an entry past position m,
vmis_index.rs:325-390), and only idf_weighting is baked into an index (mod.rs:146-152).  So search() builds one index per distinct
idf weighting, at the largest m asked for with it, and evaluates all of that weighting's trials in one srn_evaluate call.

    python -m serenade_amd.hpo <config.toml> [--random N --seed S] [--exclude-seen] [--exclude-session] [--history H] [--handler-sessions] [--fill]
                               [--bootstrap B [--seed S] [--ci C] [--ci-csv PATH]] [--segments SPEC]

reads the [hyperparam] keys of the reference's configuration (training_data_path, test_data_path, save_records, out_path,
enable_business_logic), writes exhaustive_grid_search.rs's CSV and prints its "Best ..." lines.  TPE (tpe_hyperparameter_optm.rs) is
not restated: evaluate() takes any list of trials, so an external optimiser can drive it.  The serving rules (evaluation.py: exclude_seen, exclude_session,
history, handler_sessions, fill) are options of the whole search, not grid axes: every trial runs under them, and the CSV keeps the reference's columns.
--bootstrap B runs every trial with B bootstrap replicates (--seed seeds them too): one more line after the "Best ..." lines gives the best trial's
Mrr interval and how many other trials are within noise of it (the interval of their paired difference to the best contains 0); the intervals go to --ci-csv, never into
the reference's CSV.
--segments SPEC (position:N, target_count:B1,B2,... or current_count:B1,B2,...) evaluates every trial by segment too and prints the best trial's
metrics per segment after the "Best ..." lines; the CSV keeps the reference's columns.
"""
import argparse
import ctypes as C
import itertools
import random as _random
import sys

import numpy as np

from . import capi
from .evaluation import EvalSet, compare, evaluate
from .vmisknn import VMISIndex

# exhaustive_grid_search.rs:22-25, loop order m > k > window > idf (:48-51)
EXHAUSTIVE_GRID = {"m": [100, 500, 1000, 2500], "k": [50, 100, 500, 1000, 1500], "max_items_in_session": [1, 2, 3, 5, 7, 10],
                   "idf_weighting": [1, 2, 3, 5, 7, 10]}
# hyperparameter_search.rs:12-21 (150 random combinations, kept only where k <= m)
RANDOM_GRID = {"m": [100, 250, 500, 750, 1000, 2500], "k": [50, 100, 500, 1000, 1500], "max_items_in_session": [1, 2, 3, 5, 7, 15, 100],
               "idf_weighting": [1, 2, 3]}
_KEYS = ("m", "k", "max_items_in_session", "idf_weighting")
GOAL = "MRR@20"
FILL_RANKING = 64   # search(fill=True): the fallback ranking is this many of the most popular training items


def exhaustive(grid=EXHAUSTIVE_GRID):
    """The Cartesian product in the reference's loop order -> list of trial dicts (m, k, max_items_in_session, idf_weighting)."""
    return [dict(zip(_KEYS, c)) for c in itertools.product(*(grid[k] for k in _KEYS))]


def random(grid=RANDOM_GRID, n=150, seed=0, k_le_m=False):
    """n distinct combinations drawn with a seeded generator (the reference draws from thread_rng); k_le_m drops those with k > m afterwards,
    as hyperparameter_search.rs does."""
    every = exhaustive(grid)
    picks = [every[i] for i in _random.Random(seed).sample(range(len(every)), min(int(n), len(every)))]
    return [t for t in picks if t["k"] <= t["m"]] if k_le_m else picks


def index_plan(trials):
    """{idf_weighting: m_index}: one index per distinct idf weighting, at the largest m of its trials."""
    plan = {}
    for t in trials:
        w = float(t["idf_weighting"])
        plan[w] = max(plan.get(w, 0), int(t["m"]))
    return plan


def _build_index(sessions, m_index, idf_weighting, device):
    """VMISIndex::new_from_csv's index (p99.5 session-length cut) on sessions read once."""
    q = C.c_uint64()
    capi.check(capi.lib().srn_sessions_length_quantile(sessions, 0.995, C.byref(q)))
    v = capi.SessionsView()
    capi.check(capi.lib().srn_sessions_view(sessions, C.byref(v)))
    h = C.c_void_p()
    capi.check(capi.lib().srn_index_build_gpu(C.byref(v), int(m_index), int(q.value), float(idf_weighting), int(device), C.byref(h)))
    return VMISIndex(h)


def search(train_path, test_path, trials, business_logic=False, device=0, how_many=20, length=20, loader="host", exclude_seen=False, exclude_session=False, history=0,
           handler_sessions=False, fill=False, bootstrap=0, seed=0, ci=0.95, segments=None):
    """objective() (src/objective.rs:8-52) for every trial: Mrr@length of predict(k, m, how_many) over every windowed prefix.
    loader="gpu" reads the training sessions with the GPU loader (srn_sessions_from_tsv_gpu: the same sessions).
    exclude_seen, exclude_session, history, handler_sessions, fill: the serving rules of evaluation.py, applied to every trial (fill: from the most popular
    training items, set on each index the search builds).
    bootstrap, seed, ci: evaluate()'s -- every record's report then holds its replicate arrays and intervals, paired across the search's indices.
    segments: evaluate()'s spec -- every record's report then holds its "segments"; a by="labels" spec labels the test file's sessions in
    ascending SessionId.
    -> {"records": [one per trial, in trial order], "best": the first record of the highest Mrr}."""
    trials = [dict(t) for t in trials]
    for i, t in enumerate(trials):   # what srn_evaluate refuses with SRN_ERANGE, said before any index is built: a store's history window is never below the session window
        if history and int(t["max_items_in_session"]) > int(history):
            raise ValueError("history=%d is below max_items_in_session=%d of trial %d: the seen-items window holds at least the session window" %
                             (history, int(t["max_items_in_session"]), i))
    sessions = C.c_void_p()
    if loader == "gpu":
        capi.check(capi.lib().srn_sessions_from_tsv_gpu(str(train_path).encode(), int(device), C.byref(sessions)))
    elif loader == "host":
        capi.check(capi.lib().srn_sessions_from_tsv(str(train_path).encode(), C.byref(sessions)))
    else:
        raise ValueError("loader must be 'host' or 'gpu'")
    records = [None] * len(trials)
    try:
        for w, m_index in index_plan(trials).items():
            index = _build_index(sessions, m_index, w, device)
            if fill:
                index.set_fallback_popular(FILL_RANKING)
            es = EvalSet.from_tsv(index, test_path, train_path)
            mine = [i for i, t in enumerate(trials) if float(t["idf_weighting"]) == w]
            reps = evaluate(es, [dict(k=trials[i]["k"], m=trials[i]["m"], max_items_in_session=trials[i]["max_items_in_session"], how_many=how_many,
                                      length=length, business_logic=business_logic, exclude_seen=exclude_seen, exclude_session=exclude_session, history=history,
                                      handler_sessions=handler_sessions, fill=fill) for i in mine], bootstrap=bootstrap, seed=seed, ci=ci, segments=segments)
            for i, rep in zip(mine, reps):
                t = trials[i]
                records[i] = {"iteration": i, "n_most_recent_sessions": int(t["m"]), "neighborhood_size_k": int(t["k"]),
                              "last_items_in_session": int(t["max_items_in_session"]), "idf_weighting": t["idf_weighting"],
                              GOAL: rep["Mrr@%d" % length], "report": rep}
            es.close()
            index.close()
    finally:
        capi.lib().srn_sessions_free(sessions)
    best = None
    for r in records:   # strictly greater: the first of equal values wins, as in the reference
        if best is None or r[GOAL] > best[GOAL]:
            best = r
    return {"records": records, "best": best}


def rust_f64(v):
    """f64's Display in Rust: shortest round-trip digits, no exponent, no trailing ".0"."""
    v = float(v)
    if v != v or v in (float("inf"), float("-inf")):
        return {True: "NaN", False: "inf" if v > 0 else "-inf"}[v != v]
    return np.format_float_positional(v, unique=True, trim="-")


def read_toml(path):
    """The small TOML subset the evaluator reads (serenade_amd/csrc/host/evaluator.cpp read_toml): [section] headers, key = value, # comments,
    quoted strings unquoted -> {"section.key": "value"}."""
    kv, section = {}, ""
    with open(path) as f:
        for line in f:
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            if line.startswith("["):
                section = line[1:line.index("]")].strip()
                continue
            if "=" not in line:
                continue
            k, v = (x.strip() for x in line.split("=", 1))
            if len(v) >= 2 and v[0] == '"' and v[-1] == '"':
                v = v[1:-1]
            kv[section + "." + k] = v
    return kv


def hyperparam_config(path):
    kv = read_toml(path)
    return {"training_data_path": kv.get("hyperparam.training_data_path", ""), "test_data_path": kv.get("hyperparam.test_data_path", ""),
            "save_records": kv.get("hyperparam.save_records", "false") == "true", "out_path": kv.get("hyperparam.out_path", "results.csv"),
            "enable_business_logic": kv.get("hyperparam.enable_business_logic", "false") == "true"}


def within_noise(records, best, metric="Mrr"):
    """Bootstrapped records against the best one -> [(record, compare(best, record))] for every other record; a record is within noise of the best when the
    interval of the paired difference contains 0."""
    return [(r, compare(best["report"], r["report"], metric)) for r in records if r is not best]


def parse_segments(text):
    """--segments: "position:8", "target_count:1,10,100" or "current_count:1,10,100" -> evaluate()'s spec (labels come from a caller, not from a command line)."""
    by, _, arg = str(text).partition(":")
    try:
        if by == "position":
            return dict(by=by, n=int(arg))
        if by in ("target_count", "current_count"):
            return dict(by=by, bounds=[int(x) for x in arg.split(",") if x.strip()])
    except ValueError:
        pass
    raise argparse.ArgumentTypeError("--segments takes position:N, target_count:B1,B2,... or current_count:B1,B2,...")


def segment_table(report):
    """A report's segments as lines of text: one row per segment, the seven metrics in the report's order."""
    keys = [k for k in report["segments"][0] if "@" in k and not k.endswith("_ci")] if report["segments"] else []
    width = max([len(s["name"]) for s in report["segments"]] + [7])
    lines = ["%-*s %12s %s" % (width, "segment", "evaluations", " ".join("%13s" % k for k in keys))]
    for s in report["segments"]:
        lines.append("%-*s %12d %s" % (width, s["name"], s["qty_evaluations"], " ".join("%13.6f" % s[k] for k in keys)))
    return lines


def parser():
    ap = argparse.ArgumentParser(prog="python -m serenade_amd.hpo", description="exhaustive (or random) hyper-parameter search on the GPU")
    ap.add_argument("config")
    ap.add_argument("--random", type=int, default=0, help="N random combinations of the exhaustive grid instead of all of it")
    ap.add_argument("--seed", type=int, default=0, help="of --random's draw and of --bootstrap's weights")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--gpu-loader", action="store_true", help="read the training file with the GPU loader (the same sessions)")
    ap.add_argument("--exclude-seen", action="store_true", help="every trial leaves out what the visitor has seen (the last --history items, or the session window)")
    ap.add_argument("--exclude-session", action="store_true", help="every trial leaves out the items of the query's own session")
    ap.add_argument("--history", type=int, default=0, metavar="H", help="the seen-items window of --exclude-seen (0: the session window); at least the largest last_items_in_session of the grid (10)")
    ap.add_argument("--handler-sessions", action="store_true", help="queries are the sessions /v1/recommend builds: repeated clicks dropped")
    ap.add_argument("--fill", action="store_true", help="short rows are filled from the most popular training items before they are scored")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="B", help="B bootstrap replicates per trial (0: none): confidence intervals next to the point estimates")
    ap.add_argument("--ci", type=float, default=0.95, metavar="C", help="the intervals' level")
    ap.add_argument("--ci-csv", default=None, metavar="PATH", help="with --bootstrap: every trial's Mrr interval and its paired difference to the best trial")
    ap.add_argument("--segments", type=parse_segments, default=None, metavar="SPEC", help="position:N, target_count:B1,B2,... or current_count:B1,B2,...: the best trial's "
                    "metrics by segment, printed after the Best ... lines (the CSV keeps its columns)")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    cfg = hyperparam_config(a.config)
    trials = random(EXHAUSTIVE_GRID, a.random, a.seed) if a.random else exhaustive()
    rules = dict(exclude_seen=a.exclude_seen, exclude_session=a.exclude_session, history=a.history, handler_sessions=a.handler_sessions, fill=a.fill)
    res = search(cfg["training_data_path"], cfg["test_data_path"], trials, cfg["enable_business_logic"], a.device,
                 loader="gpu" if a.gpu_loader else "host", bootstrap=a.bootstrap, seed=a.seed if a.bootstrap else 0, ci=a.ci, segments=a.segments, **rules)
    with open(cfg["out_path"], "w") as f:   # exhaustive_grid_search.rs:34-46 (the file is created either way)
        if cfg["save_records"]:
            f.write("iteration,n_most_recent_sessions,neighborhood_size_k,last_items_in_session,idf_weighting,%s\n" % GOAL)
            for r in res["records"]:
                f.write("%d,%d,%d,%d,%d,%s\n" % (r["iteration"], r["n_most_recent_sessions"], r["neighborhood_size_k"], r["last_items_in_session"],
                                                 int(r["idf_weighting"]), rust_f64(r[GOAL])))
    b = res["best"]
    none = b is None
    if any(rules.values()):
        print("Serving rules: %s" % ", ".join("%s=%d" % (n, v) if n == "history" else n for n, v in rules.items() if v))
    print("Best n_most_recent_sessions: %d" % (-1 if none else b["n_most_recent_sessions"]))
    print("Best neighborhood_size_k: %d" % (-1 if none else b["neighborhood_size_k"]))
    print("Best last_items_in_session: %d" % (-1 if none else b["last_items_in_session"]))
    print("Best idf_weighting: %d" % (-1 if none else int(b["idf_weighting"])))
    print("Business logic were %s." % ("enabled" if cfg["enable_business_logic"] else "disabled"))
    print("Best value for the goal metric: %s" % rust_f64(float("-inf") if none else b[GOAL]))
    if a.segments is not None and not none:
        print("Best trial by segment (%s):" % a.segments["by"])
        for line in segment_table(b["report"]):
            print(line)
    if a.bootstrap and not none:
        key = [k for k in b["report"] if k.startswith("Mrr@") and k.endswith("_ci")][0]
        lo, hi = b["report"][key]
        others = within_noise(res["records"], b)
        near = sum(1 for _, c in others if c["ci"][0] <= 0.0 <= c["ci"][1])
        print("Bootstrap (%d replicates, seed %d): best %s %d%% interval [%s, %s]; %d of %d other trials within noise of the best" %
              (a.bootstrap, a.seed, key[:-3], round(a.ci * 100), rust_f64(lo), rust_f64(hi), near, len(others)))
        if a.ci_csv:
            by_id = {id(r): c for r, c in others}
            with open(a.ci_csv, "w") as f:
                f.write("iteration,%s,ci_lo,ci_hi,best_minus_trial,diff_lo,diff_hi,p_best_better\n" % GOAL)
                for r in res["records"]:
                    c = by_id.get(id(r), {"delta": 0.0, "ci": (0.0, 0.0), "p_better": 0.0})
                    f.write("%d,%s,%s\n" % (r["iteration"], rust_f64(r[GOAL]), ",".join(rust_f64(v) for v in (*r["report"][key], c["delta"], *c["ci"], c["p_better"]))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
