"""Click feedback log on the GPU (srn_feedback_*, serving.ClickFeedback): every comparison is exact -- ranks, counters, histograms and every key's
stored entry against serving.feedback_model -- and a replay of a test set through recommend_batch(..., feedback=) reproduces the offline trial's Mrr / HitRate terms."""
import ctypes as C
import threading
from collections import Counter

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, evaluation, serving, synth
from serenade_amd.serving import ClickFeedback, feedback_model

pytestmark = pytest.mark.gpu

NONE, FILLED = capi.FEEDBACK_NONE, capi.FEEDBACK_FILLED
COUNTERS = ("requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored")
NOW, TTL, IDLE = 1_700_000_000, 1800, 1200
M64 = 2**64 - 1


def make_stream(seed, keys, how_many, consent=None, none_rate=0.03):
    """Requests on keys[j] (128-bit integers) with the rows served to them.  Rows are distinct ids of a small pool (0 among them); a click is, 7 times in 10, an id of
    the visitor's previous row -- at any of its how_many positions, so beyond its count too -- and the positions >= count of that previous row are then POISONED with
    the clicked id: a read past count shows up as a false hit.  Scores descend, with a -inf tail that starts at or before count and finite values beyond count."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    pool = np.arange(3 * how_many + 5, dtype=np.uint64)
    ids = np.stack([rng.permutation(pool)[:how_many] for _ in range(n)])
    counts = rng.integers(0, how_many + 1, n).astype(np.uint32)
    counts[rng.random(n) < 0.5] = how_many                     # full rows are the common case
    sc = -np.sort(-rng.random((n, how_many)), axis=1)
    for j in range(n):
        c = int(counts[j])
        sc[j, int(rng.integers(0, c + 1)):c] = -np.inf          # the filled tail inside the row; what lies beyond count stays finite
    counts[rng.random(n) < none_rate] = NONE
    consent = np.ones(n, np.uint8) if consent is None else np.asarray(consent, np.uint8)
    items = rng.choice(pool, n)
    last = {}
    for j in range(n):
        if not consent[j]:
            continue
        p = last.get(keys[j])
        if p is not None:
            if rng.random() < 0.7:                               # (the last position more often than the others: a full row's last entry is hit at every width)
                items[j] = ids[p, how_many - 1 if rng.random() < 0.15 else int(rng.integers(0, how_many))]
            c = 0 if counts[p] == NONE else int(counts[p])
            ids[p, c:] = items[j]
        last[keys[j]] = j
    hi = np.array([k >> 64 for k in keys], np.uint64)
    lo = np.array([k & M64 for k in keys], np.uint64)
    return dict(hi=hi, lo=lo, items=items, consent=consent, ids=ids, counts=counts, sc=sc, n=n, how_many=how_many)


def observe(fb, s, a, b, now, device=False, scores=True, consent=True):
    sl = slice(a, b)
    args = [s["hi"][sl], s["lo"][sl], s["items"][sl], s["consent"][sl] if consent else None, s["ids"][sl], s["counts"][sl], s["sc"][sl] if scores else None]
    if not device:
        return fb.observe((args[0], args[1]), args[2], args[3], args[4], args[5], args[6], now=now)
    import torch
    dev = torch.device("cuda", fb.device)
    t = [None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else np.int32 if x.dtype == np.uint32 else x.dtype)).to(dev)
         for x in args]
    r = fb.observe((t[0], t[1]), t[2], t[3], t[4], t[5], t[6], now=now)
    assert r is fb.last_ranks and r.dtype == torch.int32
    return r.cpu().numpy().view(np.uint32)


def model(state, s, a, b, now, row_cap, scores=True, consent=True):
    sl = slice(a, b)
    return feedback_model(state, (s["hi"][sl], s["lo"][sl]), s["items"][sl], s["consent"][sl] if consent else None, s["ids"][sl], s["counts"][sl],
                          s["sc"][sl] if scores else None, now, IDLE, row_cap=row_cap)


def add(total, ctr):
    for k, v in ctr.items():
        total[k] = total.get(k, 0) + v
    return total


def check_log(fb, state, total, keys=()):
    st = fb.stats()
    for name in COUNTERS:
        assert st[name] == total.get(name, 0), (name, st[name], total.get(name, 0))
    hm, hf = fb.histogram()
    assert np.array_equal(hm, total["hist_model"]) and np.array_equal(hf, total["hist_filled"])
    assert st["requests"] == st["no_consent"] + st["first_seen"] + st["idle_expired"] + st["observed"]
    assert st["hits_model"] == int(hm.sum()) and st["hits_filled"] == int(hf.sum()) and hm[0] == 0 and hf[0] == 0
    for k in set(keys) | set(state):
        got, want = fb.get(k), state.get(k)
        if want is None:
            assert got is None, k
        else:
            assert got is not None and np.array_equal(got[0], want[0]) and got[1:] == want[1:], (k, got, want)
    return st


def drive(fb, s, cuts, now=NOW, device=False, **kw):
    """the calls s[cuts[i]:cuts[i+1]] on the log and on the model -> (ranks, state, counters), compared"""
    state, total, ranks = {}, {}, []
    for a, b in zip(cuts, cuts[1:]):
        got = observe(fb, s, a, b, now, device=device, **kw)
        want, ctr = model(state, s, a, b, now, fb.row_cap, **kw)
        assert np.array_equal(got, want), (a, b, np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
        ranks.append(got)
        add(total, ctr)
    keys = [(int(h) << 64) | int(l) for h, l in zip(s["hi"], s["lo"])]
    check_log(fb, state, total, keys)
    return np.concatenate(ranks), state, total


def key_pattern(pattern, n, seed):
    rng = np.random.default_rng(seed)
    if pattern == "distinct":       # two calls, the same n distinct keys in each, in another order
        ks = [(int(rng.integers(1, 2**63)) << 64) | (j + 1) for j in range(n)]
        return ks + [ks[i] for i in rng.permutation(n)], [0, n, 2 * n]
    if pattern == "zipf":
        ks = [(int(rng.integers(1, 2**63)) << 64) | int(rng.integers(1, 2**63)) for _ in range(max(n // 4, 1))]
        return [ks[min(int(z) - 1, len(ks) - 1)] for z in rng.zipf(1.3, n)], [0, n]
    # keys that agree in hi, in lo, or in the low 32 bits of both
    parts = [a + (b << 32) for a in (1, 2, 3) for b in (0, 1, 2, 1 << 31)]
    ks = [(h << 64) | l for h in parts for l in parts]
    return [ks[int(i)] for i in rng.integers(0, len(ks), n)], [0, n]


@pytest.mark.parametrize("pattern", ["distinct", "zipf", "close"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_ranks_counters_and_entries_match_the_model(n, pattern):
    keys, cuts = key_pattern(pattern, n, 100 + n)
    rng = np.random.default_rng(n)
    consent = (rng.random(len(keys)) < 0.8) if pattern == "zipf" else None
    s = make_stream(n, keys, 21, consent)
    fb = ClickFeedback(0, capacity=2 * len(keys) + 1, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)
    ranks, state, total = drive(fb, s, cuts)
    if n >= 255:   # no vacuous pass: hits of both kinds, misses, and (zipf) requests without consent
        assert total["hits_model"] > 0 and total["hits_filled"] > 0 and total["observed"] > total["hits_model"] + total["hits_filled"]
        assert pattern != "zipf" or total["no_consent"] > 0
    fb.close()


@pytest.mark.parametrize("n,how_many", [(40_000, 21), (70_000, 8)])
def test_batches_beyond_the_rank_kernels_grid_cap(n, how_many):
    """fb_rank's grid is capped at 2048 workgroups of 16 (rows wider than 8 ids) or 32 lane groups: from 32 768 / 65 536 requests on a group makes several trips, the
    last one partial"""
    keys, cuts = key_pattern("zipf", n, n)
    s = make_stream(n, keys, how_many, np.random.default_rng(n).random(n) < 0.9)
    fb = ClickFeedback(0, capacity=n, row_cap=how_many, ttl_secs=TTL, idle_secs=IDLE)
    ranks, state, total = drive(fb, s, [0, n], device=True)
    assert total["hits_model"] > 0 and total["hits_filled"] > 0 and total["no_consent"] > 0
    fb.close()


def test_three_thousand_requests_on_one_key():
    s = make_stream(3, [(9 << 64) | 9] * 3000, 21)
    fb = ClickFeedback(0, capacity=4096, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)
    ranks, state, total = drive(fb, s, [0, 3000])
    assert total["first_seen"] == 1 and total["observed"] == 2999 and len(state) == 1
    fb.close()


@pytest.mark.parametrize("how_many", [1, 8, 9, 11, 12, 21, 64, 65, 130])
def test_row_widths(how_many):
    """lane-group edges (8 / 9), rows of several rounds (21 .. 130) and the 128-byte slot boundary (11 / 12), on device tensors"""
    keys, _ = key_pattern("zipf", 700, how_many)
    s = make_stream(how_many, keys, how_many, np.random.default_rng(how_many).random(700) < 0.9)
    fb = ClickFeedback(0, capacity=1024, row_cap=how_many, ttl_secs=TTL, idle_secs=IDLE)
    assert fb.stats()["slot_bytes"] == (40 + 8 * how_many + 127) // 128 * 128
    ranks, state, total = drive(fb, s, [0, 300, 700], device=True)
    assert total["hits_model"] > 0 and total["observed"] > total["hits_model"] + total["hits_filled"]
    assert how_many == 1 or total["hits_filled"] > 0
    if how_many > 1:   # the last position of a full row is hit
        assert total["hist_model"][how_many] + total["hist_filled"][how_many] > 0
    fb.close()


@pytest.mark.parametrize("device", [False, True])
def test_timed_call_on_eight_lane_groups(device):
    """observe(..., times=) at row_cap = how_many = 8, where a request is an 8-lane group (test_gpu_replay.py drives the timed kernels at row_cap = 21 only): one call of
    257 requests from 3 visitors, every fifth without consent, with gaps above idle_secs before requests 255 and 256 -- both in the run of the visitor with the largest
    key, the second one past the first 256 positions.  Ranks, counters, histograms and the three entries are the model's, exactly."""
    n, how_many = 257, 8
    vis = [(7 << 64) | 11, (7 << 64) | 12, (9 << 64) | 3]
    keys = [vis[j % 3] for j in range(n)]
    keys[255] = keys[256] = vis[2]
    consent = (np.arange(n) % 5 != 0).astype(np.uint8)
    consent[255:] = 1
    s = make_stream(4108, keys, how_many, consent)
    times = NOW + np.arange(n, dtype=np.uint64)
    times[255:] += np.uint64(IDLE + 1)
    times[256:] += np.uint64(IDLE + 1)
    state = {}
    want, total = feedback_model(state, (s["hi"], s["lo"]), s["items"], s["consent"], s["ids"], s["counts"], s["sc"], NOW, IDLE, row_cap=how_many, times=times)
    assert total["idle_expired"] >= 2 and total["hits_model"] + total["hits_filled"] >= 1 and total["no_consent"] > 0   # no vacuous pass
    fb = ClickFeedback(0, capacity=2 * n, row_cap=how_many, ttl_secs=TTL, idle_secs=IDLE)
    args = [s["hi"], s["lo"], s["items"], s["consent"], s["ids"], s["counts"], s["sc"], times]
    if device:
        import torch
        args = [torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else np.int32 if x.dtype == np.uint32 else x.dtype)).to(torch.device("cuda", fb.device))
                for x in args]
    got = fb.observe((args[0], args[1]), args[2], args[3], args[4], args[5], args[6], now=NOW, times=args[7])
    got = got.cpu().numpy().view(np.uint32) if device else got
    assert np.array_equal(got, want), (np.flatnonzero(got != want)[:8], got[got != want][:8], want[got != want][:8])
    check_log(fb, state, total, vis)
    fb.close()


@pytest.mark.parametrize("timed", [False, True])
def test_the_scratch_grows_behind_a_call_that_may_still_run(timed):
    """Two device-pointer calls on one stream with nothing between them: one request, then 257 -- two blocks of 256 lanes and one more -- so the log's scratch is freed
    and reallocated while the first call may still read it: the grow rule waits for that call.  The second call repeats visitors, every seventh request does not
    consent and, timed, one gap lies above idle_secs.  Ranks, counters, histograms and entries are those of the same two calls on a fresh log with a synchronisation
    in between."""
    import torch
    n, how_many = 258, 8
    vis = [((7 + v) << 64) | (11 * v + 1) for v in range(5)]
    consent = (np.arange(n) % 7 != 3).astype(np.uint8)
    s = make_stream(4109, [vis[j % 5] for j in range(n)], how_many, consent)
    times = NOW + np.arange(n, dtype=np.uint64)
    times[200:] += np.uint64(IDLE + 1)
    assert consent[195] and consent[200] and consent[0]
    dev = torch.device("cuda", 0)
    t = {name: torch.from_numpy(np.ascontiguousarray(x).view(np.int64 if x.dtype == np.uint64 else np.int32 if x.dtype == np.uint32 else x.dtype)).to(dev)
         for name, x in dict(s, times=times).items() if isinstance(x, np.ndarray)}           # every copy before the first call: none between the two
    stream = torch.cuda.current_stream(dev)
    results = []
    for synchronise in (False, True):
        fb = ClickFeedback(0, capacity=1024, row_cap=how_many, ttl_secs=TTL, idle_secs=IDLE)   # (room for both calls by the host's bound: the capacity rule waits for nothing)
        stream.synchronize()
        ranks = []
        for sl in (slice(0, 1), slice(1, n)):
            ranks.append(fb.observe((t["hi"][sl], t["lo"][sl]), t["items"][sl], t["consent"][sl], t["ids"][sl], t["counts"][sl], t["sc"][sl], now=NOW,
                                    times=t["times"][sl] if timed else None))
            if synchronise:
                stream.synchronize()
        stream.synchronize()
        st = fb.stats()
        results.append(([r.cpu().numpy() for r in ranks], [st[c] for c in COUNTERS], fb.histogram(), [fb.get(k) for k in vis]))
        fb.close()
    (ranks, counters, hist, entries), (ranks_s, counters_s, hist_s, entries_s) = results
    assert counters[COUNTERS.index("observed")] > 100 and counters[COUNTERS.index("no_consent")] > 0 and (counters[COUNTERS.index("idle_expired")] > 0) == timed
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ranks, ranks_s)) and counters == counters_s
    assert all(np.array_equal(a, b) for a, b in zip(hist, hist_s))
    assert all(a is not None and np.array_equal(a[0], b[0]) and a[1:] == b[1:] for a, b in zip(entries, entries_s))


def test_rows_narrower_than_the_log():
    keys, _ = key_pattern("zipf", 600, 5)
    s = make_stream(5, keys, 5)
    fb = ClickFeedback(0, capacity=1024, row_cap=9, ttl_secs=TTL, idle_secs=IDLE)
    drive(fb, s, [0, 100, 600])
    with pytest.raises(capi.SerenadeError) as e:
        observe(fb, make_stream(6, keys[:4], 10), 0, 4, NOW)
    assert e.value.code == capi.SRN_ERANGE
    fb.close()


class LogTable:
    """helpers.capacity_rule_sequence's view of a ClickFeedback and feedback_model's state: a request per key, rows of 4"""

    def __init__(self, fb):
        self.fb, self.state, self.total = fb, {}, {}

    def call(self, keys, now):
        s = make_stream(len(keys), keys, 4)
        got = observe(self.fb, s, 0, len(keys), now)          # (a refusal raises here: the model stays as it was)
        want, ctr = model(self.state, s, 0, len(keys), now, 4)
        assert np.array_equal(got, want)
        add(self.total, ctr)

    def stats(self):
        return check_log(self.fb, self.state, self.total)

    def sweep(self, now):
        return self.fb.sweep(now)

    def expire(self, now):
        self.state = {k: e for k, e in self.state.items() if not (now > e[2] and now - e[2] > TTL)}

    def check(self, keys):
        check_log(self.fb, self.state, self.total, keys)


@pytest.mark.parametrize("capacity", [1, 2, 3, 33, 64])
def test_capacity_rule_refusal_and_sweeps(capacity):
    if capacity != 64:   # the rule at its smallest tables: 2, 4, 8 and 128 slots
        from helpers import capacity_rule_sequence
        fb = ClickFeedback(0, capacity=capacity, row_cap=4, ttl_secs=TTL, idle_secs=IDLE)
        assert fb.stats()["slots"] == {1: 2, 2: 4, 3: 8, 33: 128}[capacity]
        capacity_rule_sequence(LogTable(fb), capacity, NOW, TTL)
        fb.close()
        return
    T0 = NOW
    ks = [(int(h) << 64) | 5 for h in range(1, 66)]
    s = make_stream(11, ks, 4)
    fb = ClickFeedback(0, capacity=64, row_cap=4, ttl_secs=TTL, idle_secs=IDLE)
    assert fb.stats()["slots"] == 128
    state, total = {}, {}
    for a, b, now in ((0, 32, T0), (32, 64, T0 + 1000)):
        got = observe(fb, s, a, b, now)
        want, ctr = model(state, s, a, b, now, 4)
        assert np.array_equal(got, want)
        add(total, ctr)
    before = check_log(fb, state, total)
    assert before["live_bound"] == 64
    with pytest.raises(capi.SerenadeError) as e:   # one more key: every entry is younger than the TTL
        observe(fb, s, 64, 65, T0 + 1000)
    assert e.value.code == capi.SRN_ENOMEM
    after = check_log(fb, state, total, ks)
    assert after["refused"] == 1 and after["sweeps"] == 0 and {k: v for k, v in after.items() if k != "refused"} == {k: v for k, v in before.items() if k != "refused"}
    # the first 32 keys are now older than the TTL: the same call goes through the automatic sweep
    now = T0 + TTL + 200
    got = observe(fb, s, 64, 65, now)
    want, ctr = model(state, s, 64, 65, now, 4)
    assert np.array_equal(got, want) and got[0] == NONE
    add(total, ctr)
    for k in ks[:32]:
        del state[k]
    st = check_log(fb, state, total, ks)
    assert st["sweeps"] == 1 and st["refused"] == 1 and st["live_bound"] == 33   # (32 live entries + the batch)
    # sweep keeps exactly the live rows: "older" is now - epoch > ttl
    assert fb.sweep(T0 + 1000 + TTL) == 33
    check_log(fb, state, total, ks)
    assert fb.sweep(T0 + 1000 + TTL + 1) == 1
    for k in ks[32:64]:
        del state[k]
    st = check_log(fb, state, total, ks)
    assert st["sweeps"] == 3 and st["live_bound"] == 1
    fb.close()


def test_any_cut_into_calls_gives_the_same_ranks_counters_and_table():
    keys, _ = key_pattern("zipf", 6000, 77)
    s = make_stream(77, keys, 21, np.random.default_rng(5).random(6000) < 0.85)
    one = ClickFeedback(0, capacity=8192, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)
    want_ranks, want_state, want_total = drive(one, s, [0, 6000])
    cuts, sizes = [0], [1, 7, 256, 4096]
    while cuts[-1] < 6000:
        cuts.append(min(6000, cuts[-1] + sizes[(len(cuts) - 1) % 4]))
    assert len(cuts) > 8
    cut = ClickFeedback(0, capacity=8192, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)
    ranks, state, total = drive(cut, s, cuts)
    assert np.array_equal(ranks, want_ranks)
    for k in want_total:
        assert np.array_equal(total[k], want_total[k]), k
    a, b = one.stats(), cut.stats()
    assert {k: a[k] for k in COUNTERS} == {k: b[k] for k in COUNTERS} and (a["mrr"], a["hit_rate"]) == (b["mrr"], b["hit_rate"])
    assert all(np.array_equal(x, y) for x, y in zip(one.histogram(), cut.histogram()))
    assert state.keys() == want_state.keys()
    # a second run gives the same bits
    again = ClickFeedback(0, capacity=8192, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)
    assert np.array_equal(observe(again, s, 0, 6000, NOW), want_ranks)
    for fb in (one, cut, again):
        fb.close()


def test_null_scores_null_ranks_reset_and_metrics():
    keys, _ = key_pattern("zipf", 900, 31)
    s = make_stream(31, keys, 12)
    s["items"][::5] = 0                                        # item id 0 is an id like any other (the pool holds it)
    fb = ClickFeedback(0, capacity=1024, row_cap=12, ttl_secs=TTL, idle_secs=IDLE)
    ranks, state, total = drive(fb, s, [0, 400, 900], scores=False, consent=False)   # NULL d_scores, NULL d_consent: every entry a model entry
    assert total["hits_filled"] == 0 and total["hits_model"] > 0 and all(v[1] == len(v[0]) for v in state.values())
    assert int(((ranks != NONE) & (ranks > 0) & (s["items"] == 0)).sum()) > 0
    st = fb.stats()
    m = serving.feedback_metrics(total["hist_model"], total["hist_filled"], total["observed"])
    assert st["mrr"] == m["mrr"] > 0 and st["hit_rate"] == m["hit_rate"] == st["hits_model"] / st["observed"] and st["mrr_filled"] == 0.0
    # NULL out_rank: the counters and the table move as with it
    fb2 = ClickFeedback(0, capacity=1024, row_cap=12, ttl_secs=TTL, idle_secs=IDLE)
    for a, b in ((0, 400), (400, 900)):
        capi.check(capi.lib().srn_feedback_observe(fb2._h, capi.ptr(s["hi"][a:b]), capi.ptr(s["lo"][a:b]), capi.ptr(s["items"][a:b]), None, b - a, NOW,
                                                   capi.ptr(np.ascontiguousarray(s["ids"][a:b])), None, capi.ptr(s["counts"][a:b]), 12, None))
    check_log(fb2, state, total)
    fb2.reset_counters()
    zero = {"hist_model": np.zeros(13, np.uint64), "hist_filled": np.zeros(13, np.uint64)}
    check_log(fb2, state, zero)                                # the table is untouched
    assert fb2.stats()["mrr"] == 0.0
    fb.close()
    fb2.close()


def test_nothing_is_written_beyond_n():
    import torch
    n, how_many, pad = 257, 9, 64
    keys, _ = key_pattern("zipf", n, 41)
    s = make_stream(41, keys, how_many)
    dev = torch.device("cuda", 0)
    fb = ClickFeedback(0, capacity=1024, row_cap=how_many, ttl_secs=TTL, idle_secs=IDLE)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.int32)).to(dev)
    hi, lo, it, ids, cnt = (up(s[k]) for k in ("hi", "lo", "items", "ids", "counts"))
    sc = torch.from_numpy(s["sc"]).to(dev)
    ranks = torch.full((n + pad,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    for _ in range(2):
        capi.check(capi.lib().srn_feedback_observe_device(fb._h, p(hi), p(lo), p(it), None, n, NOW, p(ids), p(sc), p(cnt), how_many, p(ranks),
                                                          C.c_void_p(torch.cuda.current_stream(0).cuda_stream)))
    torch.cuda.synchronize()
    state = {}
    model(state, s, 0, n, NOW, how_many, consent=False)
    want, _ = model(state, s, 0, n, NOW, how_many, consent=False)
    got = ranks.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:n], want) and (got[n:] == 0x5A5A5A5A).all()
    for t, k in ((hi, "hi"), (lo, "lo"), (it, "items"), (ids, "ids"), (cnt, "counts")):   # the inputs are read only
        assert np.array_equal(t.cpu().numpy().view(s[k].dtype), s[k]), k
    fb.close()


def test_null_out_rank_on_the_device_and_counts_above_the_stride():
    """srn_feedback_observe_device with d_out_rank = NULL (the host entry point always hands the kernel a staging buffer): counters, histograms and every key's entry
    move as with it.  Some counts lie above the row stride: they are read as the stride."""
    import torch
    n, how_many = 1500, 12
    keys, _ = key_pattern("zipf", n, 61)
    s = make_stream(61, keys, how_many, np.random.default_rng(61).random(n) < 0.9)
    full = np.flatnonzero(s["counts"] == how_many)[::3]
    clamped = dict(s, counts=s["counts"].copy())
    clamped["counts"][full] = how_many + 3
    assert len(full) > 50
    dev = torch.device("cuda", 0)
    fb = ClickFeedback(0, capacity=2048, row_cap=how_many, ttl_secs=TTL, idle_secs=IDLE)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype, a.dtype))).to(dev)   # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    state, total = {}, {}
    for a, b in ((0, 1), (1, 600), (600, n)):
        t = {k: up(clamped[k][a:b]) for k in ("hi", "lo", "items", "consent", "ids", "counts", "sc")}
        capi.check(capi.lib().srn_feedback_observe_device(fb._h, p(t["hi"]), p(t["lo"]), p(t["items"]), p(t["consent"]), b - a, NOW, p(t["ids"]), p(t["sc"]), p(t["counts"]),
                                                          how_many, None, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)))
        torch.cuda.synchronize()
        add(total, model(state, s, a, b, NOW, how_many)[1])     # (the model on the counts within the stride)
    assert total["hits_model"] > 0 and total["hits_filled"] > 0 and total["no_consent"] > 0
    check_log(fb, state, total, keys)
    same, ctr = {}, {}
    add(ctr, model(same, clamped, 0, n, NOW, how_many)[1])     # the model reads such counts as the stride too
    assert all(np.array_equal(ctr[k], total[k]) for k in total)
    fb.close()


def test_argument_checks_on_a_live_log_change_nothing():
    L = capi.lib()
    keys, _ = key_pattern("zipf", 300, 71)
    s = make_stream(71, keys, 9)
    fb = ClickFeedback(0, capacity=512, row_cap=9, ttl_secs=TTL, idle_secs=IDLE)
    ranks, state, total = drive(fb, s, [0, 300])
    before = fb.stats()
    hi, lo, it, ids, cnt, rk = s["hi"], s["lo"], s["items"], np.ascontiguousarray(s["ids"]), s["counts"], np.full(300, 0x5A5A5A5A, np.uint32)
    good = [capi.ptr(hi), capi.ptr(lo), capi.ptr(it), None, 300, NOW, capi.ptr(ids), None, capi.ptr(cnt), 9, capi.ptr(rk)]

    def both(args):
        return L.srn_feedback_observe(fb._h, *args), L.srn_feedback_observe_device(fb._h, *args, None)   # (refused before any pointer is used)
    for at, value, code in [(4, 0, capi.SRN_OK)] + [(i, None, capi.SRN_EINVAL) for i in (0, 1, 2, 6, 8)] + \
                           [(4, (1 << 24) + 1, capi.SRN_ERANGE), (9, 0, capi.SRN_EINVAL), (9, 10, capi.SRN_ERANGE)]:
        args = list(good)
        args[at] = value
        assert both(args) == (code, code), (at, value)
    assert both([None, None, None, None, 0, NOW, None, None, None, 9, None]) == (capi.SRN_OK, capi.SRN_OK)   # n = 0 comes first
    hm = np.zeros(9, np.uint64)
    assert L.srn_feedback_histogram(fb._h, capi.ptr(hm), None, 9) == capi.SRN_ERANGE        # fewer than row_cap + 1 entries
    assert (rk == 0x5A5A5A5A).all() and not hm.any()
    assert check_log(fb, state, total, keys) == before
    fb.close()


def test_two_threads_on_one_log_with_disjoint_keys():
    streams, cuts = [], [0, 300, 301, 900, 1500]
    for t in range(2):
        rng = np.random.default_rng(50 + t)
        ks = [((t + 1) << 64) | int(rng.integers(1, 200)) for _ in range(1500)]
        streams.append(make_stream(50 + t, ks, 21, rng.random(1500) < 0.9))
    fb = ClickFeedback(0, capacity=16384, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)
    got, errors = [[], []], []

    def run(t):
        try:
            for a, b in zip(cuts, cuts[1:]):
                got[t].append(observe(fb, streams[t], a, b, NOW).copy())
        except Exception as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    state, total = {}, {}
    for t in range(2):
        want, ctr = model(state, streams[t], 0, 1500, NOW, 21)
        assert np.array_equal(np.concatenate(got[t]), want)
        add(total, ctr)
    check_log(fb, state, total)
    fb.close()


# ---- offline = online: a test set replayed through the endpoint reproduces the offline trial's Mrr / HitRate terms ----
K, M, HOW_MANY, W = 100, 500, 20, 2


@pytest.fixture(scope="module")
def tiny():
    from test_gpu_evaluate_serving import make_sessions
    inter, n_items, _, _, idfw = synth.CONFIGS["tiny"]
    off, items, ts = synth.training_sessions(inter, n_items)
    index = sa.VMISIndex.from_sessions(off, items, ts, M, 34, idfw, device=0)
    sessions, _ = make_sessions(Counter(int(x) for x in items), n_items)
    es = evaluation.EvalSet(index, sessions, items)
    yield dict(index=index, seqs=list(sessions.values()), es=es)
    es.close()


@pytest.mark.parametrize("arm", ["plain", "seen+fill"])
@pytest.mark.parametrize("packing", ["by_click", "one_call", "one_call_device"])   # (the last: device tensors)
def test_replaying_a_test_set_reproduces_the_offline_terms(tiny, arm, packing):
    index, es, seqs = tiny["index"], tiny["es"], tiny["seqs"]
    rules = dict(exclude_seen=True, fill=True) if arm == "seen+fill" else {}
    H = 8 if arm == "seen+fill" else 0
    sess = np.concatenate([np.full(len(s), i, np.int64) for i, s in enumerate(seqs)])
    step = np.concatenate([np.arange(len(s)) for s in seqs])
    clicks = np.array([x for s in seqs for x in s], np.uint64)
    if packing == "by_click":   # the t-th clicks of all sessions per call
        order = np.lexsort((sess, step))
        calls = np.flatnonzero(np.diff(step[order], prepend=-1, append=-1))
    else:
        order, calls = np.arange(len(clicks)), np.array([0, len(clicks)])
    on_device = packing == "one_call_device"
    hi, lo = np.full(len(clicks), 77, np.uint64), (sess + 1).astype(np.uint64)
    store = serving.DeviceSessionStore(index, capacity=4096, items_cap=16, history=H)
    fb = ClickFeedback(index, capacity=4096, row_cap=HOW_MANY)
    ranks, n_model_prev, filled_rows = np.zeros(len(clicks), np.uint32), np.zeros(len(clicks), np.int64), 0
    if rules:
        index.set_fallback_popular(64)
    try:
        got, rep = es.terms(dict(k=K, m=M, max_items_in_session=W, how_many=HOW_MANY, length=HOW_MANY, history=H, handler_sessions=True, **rules))
        for a, b in zip(calls, calls[1:]):
            req = order[a:b]
            args = [hi[req], lo[req], clicks[req]]
            if on_device:
                import torch
                args = [torch.from_numpy(x.view(np.int64)).to(torch.device("cuda", 0)) for x in args]
            out = serving.recommend_batch(index, store, (args[0], args[1]), args[2], k=K, m=M, how_many=HOW_MANY, max_items_in_session=W,
                                          now=NOW, scores=True, feedback=fb, **rules)
            ids, cnt, sc = (x.cpu().numpy() for x in out) if on_device else out
            ranks[req] = fb.last_ranks.cpu().numpy().view(np.uint32) if on_device else fb.last_ranks
            finite = (np.isfinite(sc) & (np.arange(HOW_MANY)[None, :] < cnt[:, None])).sum(axis=1)
            filled_rows += int((finite < cnt).sum())
            nxt = req + 1                                      # the row is scored by the session's next click
            n_model_prev[nxt[nxt < len(clicks)]] = finite[nxt < len(clicks)]
    finally:
        if rules:
            index.clear_fallback()
        store.close()
    first = step == 0
    assert (ranks[first] == NONE).all() and (ranks[~first] != NONE).all()
    r = (ranks[~first] & 0x7FFFFFFF).astype(np.int64)          # request of click e_{t+1} <-> state t: the set's query order
    assert got.shape[0] == len(r) == rep["qty_evaluations"]
    want_mrr = np.where(r > 0, 1.0 / np.maximum(r, 1), 0.0)
    assert np.array_equal(got[:, 0], want_mrr) and np.array_equal(got[:, 1], (r > 0).astype(np.float64))
    assert np.array_equal((ranks[~first] & FILLED) != 0, r > n_model_prev[~first])   # the filled hits are those at a rank beyond the model count
    st = fb.stats()
    assert st["observed"] == rep["qty_evaluations"] and st["first_seen"] == len(seqs) and st["idle_expired"] == 0 and st["no_consent"] == 0
    assert st["hits_model"] + st["hits_filled"] == rep["sums"]["hit_rate"] == int((r > 0).sum()) > 0
    assert st["hits_filled"] == int(((ranks[~first] & FILLED) != 0).sum())
    # (the log adds hist[r] / r in ascending r, the trial its terms in query order: fewer than 2^10 terms of at most 1, so the sums agree to 2^10 * 2^-53 ~ 1e-13)
    assert abs(st["mrr"] - rep["Mrr@%d" % HOW_MANY]) <= 1e-12 and st["hit_rate"] == rep["HitRate@%d" % HOW_MANY]
    print("%s / %s: observed %d, hits on model entries %d, on filled entries %d, rows with filled entries %d" %
          (arm, packing, st["observed"], st["hits_model"], st["hits_filled"], filled_rows))
    if arm == "seen+fill":
        assert filled_rows > 0 and st["hits_filled"] > 0       # no vacuous pass: rows were filled (35 of them when this was written) and clicks landed there (8)
    else:
        assert st["hits_filled"] == 0 and filled_rows == 0
    fb.close()


def test_a_log_that_refuses_a_call_does_not_fail_recommend_batch(tiny):
    index, seqs = tiny["index"], tiny["seqs"]
    clicks = np.array([s[0] for s in seqs[:7]], np.uint64)
    hi, lo = np.full(7, 5, np.uint64), np.arange(1, 8, dtype=np.uint64)
    stores = [serving.DeviceSessionStore(index, capacity=64, items_cap=16) for _ in range(2)]
    fb = ClickFeedback(index, capacity=4, row_cap=HOW_MANY)
    kw = dict(k=K, m=M, how_many=HOW_MANY, max_items_in_session=W, now=NOW, scores=True)
    serving.recommend_batch(index, stores[0], (hi[:4], lo[:4]), clicks[:4], feedback=fb, **kw)
    serving.recommend_batch(index, stores[1], (hi[:4], lo[:4]), clicks[:4], **kw)
    before = fb.stats()
    assert before["first_seen"] == 4 and fb.last_error is None and fb.last_ranks is not None
    want = serving.recommend_batch(index, stores[1], (hi[4:], lo[4:]), clicks[4:], **kw)
    with pytest.warns(RuntimeWarning, match="feedback"):      # three more visitors: live entries + batch > capacity
        got = serving.recommend_batch(index, stores[0], (hi[4:], lo[4:]), clicks[4:], feedback=fb, **kw)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and int(got[1].max()) > 0
    assert fb.last_ranks is None and fb.last_error.code == capi.SRN_ENOMEM
    after = fb.stats()
    assert after["refused"] == 1 and {k: v for k, v in after.items() if k != "refused"} == {k: v for k, v in before.items() if k != "refused"}
    for st in stores:
        st.close()
    fb.close()
