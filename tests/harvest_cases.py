"""The seeded request stream of the session-harvest tests (tests/test_harvest_host.py, tests/test_gpu_harvest.py) and its replay through serving.harvest_model.
Test-side only; needs no GPU."""
import numpy as np

from serenade_amd.serving import harvest_model

IDLE, TTL = 20, 30
T0 = 1_700_000_000
FAR = T0 + 10 ** 6
SEED = 1                      # chosen on the CPU with replay() below: test_harvest_host.py asserts that it gives every case the replay test is about
U64 = 2 ** 64 - 1


def make_stream(seed=SEED, n_steps=40, per_step=50, n_visitors=150, n_items=40):
    """-> list of steps {"now", "hi", "lo", "items", "consent", "sweep"}: about n_steps * per_step requests.  A step's requests share one `now`; steps are 1..4 s
    apart, so a visitor's gaps fall on both sides of IDLE and TTL.  A quarter of a step's requests repeat a visitor of the same step; one request in seven has no
    consent; a click repeats the visitor's previous one one time in four.  Keys share their high or low words with other keys.  A sweep follows every sixth step."""
    rng = np.random.default_rng(seed)
    his = rng.integers(1, 2 ** 63, 4, dtype=np.uint64)
    half = n_visitors // 2
    hidx = rng.integers(0, 4, n_visitors)
    vlo = rng.integers(1, 2 ** 63, n_visitors, dtype=np.uint64)
    vlo[half:2 * half] = vlo[:half]                                       # the same low word under another high word
    hidx[half:2 * half] = (hidx[:half] + 1) % 4
    vhi = his[hidx]
    pool = (np.arange(n_items, dtype=np.uint64) * np.uint64(7919) + np.uint64(10 ** 12))
    last = {}
    steps, now = [], T0
    for s in range(n_steps):
        now += int(rng.integers(1, 5))
        n = int(per_step + rng.integers(-10, 11))
        vis = rng.integers(0, n_visitors, n)
        again = rng.random(n) < 0.25
        vis[1:][again[1:]] = vis[:-1][again[1:]]                           # several requests of one visitor in a step
        vis = rng.permutation(vis)
        items = pool[rng.integers(0, n_items, n)]
        for j in range(n):
            if vis[j] in last and rng.random() < 0.25:
                items[j] = last[vis[j]]
            last[vis[j]] = items[j]
        consent = (rng.random(n) >= 1 / 7).astype(np.uint8)
        steps.append(dict(now=now, hi=vhi[vis].copy(), lo=vlo[vis].copy(), items=items, consent=consent, sweep=(s % 6 == 5)))
    return steps


def cut(step, parts):
    """the requests of a step as `parts` consecutive slices (the last one may be the longest)"""
    n = len(step["items"])
    edges = [n * i // parts for i in range(parts)] + [n]
    return [slice(a, b) for a, b in zip(edges, edges[1:])]


def replay(steps, parts=1, limit=2, min_len=2, capacity=None):
    """the stream through harvest_model, every step cut into `parts` calls, with the final sweep far in the future -> (sessions, counters, properties)"""
    state = {}
    kw = dict(limit=limit, idle_secs=IDLE, ttl_secs=TTL, min_len=min_len, capacity=capacity)
    props = dict(return_at_run_head=0, by_explicit_sweep=0)
    out = ([], {})
    for st in steps:
        # a return after idle at the head of a run that goes on: a consenting visitor with >= 2 consenting requests in the step whose stored session is idle now
        keys = [(int(h) << 64) | int(l) for h, l, c in zip(st["hi"], st["lo"], st["consent"]) if c]
        for k in set(keys):
            cur = state.get(k)
            if keys.count(k) >= 2 and cur and cur[0] and st["now"] - cur[1] > IDLE:
                props["return_at_run_head"] += 1
        for sl in cut(st, parts):
            out = harvest_model(state, (st["hi"][sl], st["lo"][sl]), st["items"][sl], st["consent"][sl], st["now"], **kw)
        if st["sweep"]:
            before = out[1]["from_rebuild"]
            out = harvest_model(state, None, None, None, st["now"], sweep=True, **kw)
            props["by_explicit_sweep"] += out[1]["from_rebuild"] - before
    out = harvest_model(state, None, None, None, FAR, sweep=True, **kw)
    return out[0], out[1], props


def as_arrays(sessions, items_cap):
    """model sessions -> the arrays SessionHarvest.export() returns"""
    n = len(sessions)
    hi = np.array([k >> 64 for k, _, _ in sessions], np.uint64)
    lo = np.array([k & U64 for k, _, _ in sessions], np.uint64)
    ep = np.array([e for _, e, _ in sessions], np.uint64)
    ln = np.array([len(s) for _, _, s in sessions], np.uint32)
    it = np.zeros((n, items_cap), np.uint64)
    for i, (_, _, s) in enumerate(sessions):
        it[i, :len(s)] = np.asarray(s, np.uint64)
    return (hi, lo), ep, ln, it
