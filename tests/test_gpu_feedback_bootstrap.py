"""Visitor-clustered bootstrap of the click feedback log on the GPU (srn_feedback_bootstrap_*, ClickFeedback(..., bootstrap=B)).  The replicate
words are exact integers, so every comparison is equality: with serving.feedback_bootstrap_model on the ranks serving.feedback_model gives, across cuts of a stream
into calls, across the entry points, and between a timed call and one call per request."""
import ctypes as C
import os

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, serving
from serenade_amd.serving import ClickFeedback, feedback_bootstrap_model, feedback_compare, feedback_model

pytestmark = pytest.mark.gpu

NONE, FILLED = capi.FEEDBACK_NONE, capi.FEEDBACK_FILLED
COUNTERS = ("requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored")
WORDS = ("observed", "hist_model", "hist_filled")
NOW, TTL, IDLE = 1_700_000_000, 1800, 1200
M64 = 2**64 - 1


def visitors(n, seed):
    """n requests on about n / 4 visitors: about four clicks each, so that in sorted order a visitor's run often straddles two staged blocks of positions.  The keys
    come from a grid of few hi and few lo words: most of them agree with others in one half."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(max(n // 4, 1))))
    hi_words = [int(x) for x in rng.integers(1, 2**63, side)]
    lo_words = [0] + [int(x) for x in rng.integers(1, 2**63, side)][1:]
    pool = [(h << 64) | l for h in hi_words for l in lo_words][:max(n // 4, 1)]
    return [pool[int(i)] for i in rng.integers(0, len(pool), n)]


def make_stream(seed, keys, how_many, consent=None, none_rate=0.03):
    """Requests on keys[j] (128-bit integers) with the rows served to them, in the style of test_gpu_feedback.py: rows of distinct ids from a small pool; a click is,
    7 times in 10, an id of the visitor's previous row, the last position more often than the others; scores descend into a -inf tail (the filled entries) that
    starts at or before count; some counts are NONE (not served)."""
    rng = np.random.default_rng(seed)
    n = len(keys)
    pool = np.arange(3 * how_many + 5, dtype=np.uint64)
    ids = np.stack([rng.permutation(pool)[:how_many] for _ in range(n)])
    counts = rng.integers(0, how_many + 1, n).astype(np.uint32)
    counts[rng.random(n) < 0.5] = how_many
    sc = -np.sort(-rng.random((n, how_many)), axis=1)
    for j in range(n):
        c = int(counts[j])
        sc[j, int(rng.integers(0, c + 1)):c] = -np.inf
    counts[rng.random(n) < none_rate] = NONE
    consent = np.ones(n, np.uint8) if consent is None else np.asarray(consent, np.uint8)
    items = rng.choice(pool, n)
    last = {}
    for j in range(n):
        if not consent[j]:
            continue
        p = last.get(keys[j])
        if p is not None:
            if rng.random() < 0.7:
                items[j] = ids[p, how_many - 1 if rng.random() < 0.15 else int(rng.integers(0, how_many))]
            c = 0 if counts[p] == NONE else int(counts[p])
            ids[p, c:] = items[j]                              # a read past count would show up as a false hit
        last[keys[j]] = j
    hi = np.array([k >> 64 for k in keys], np.uint64)
    lo = np.array([k & M64 for k in keys], np.uint64)
    return dict(hi=hi, lo=lo, items=items, consent=consent, ids=ids, counts=counts, sc=sc, n=n, how_many=how_many)


def stream(n, how_many, seed, consent_rate=0.85):
    keys = visitors(n, seed)
    consent = np.random.default_rng(seed + 1).random(n) < consent_rate if n > 1 else None
    return make_stream(seed + 2, keys, how_many, consent)


def to_device(x, device=0):
    import torch
    if x is None:
        return None
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(x.dtype, x.dtype)
    return torch.from_numpy(np.ascontiguousarray(x).view(view)).to(torch.device("cuda", device))


def observe(fb, s, a, b, now=NOW, device=False, times=None):
    args = [s[k][a:b] for k in ("hi", "lo", "items", "consent", "ids", "counts", "sc")] + [None if times is None else times[a:b]]
    if device:
        args = [to_device(x) for x in args]
    r = fb.observe((args[0], args[1]), args[2], args[3], args[4], args[5], args[6], now=now, times=args[7])
    return r.cpu().numpy().view(np.uint32) if device else r


def model_ranks(s, row_cap, times=None):
    """the whole stream's ranks by serving.feedback_model: one call holds for any cut"""
    return feedback_model({}, (s["hi"], s["lo"]), s["items"], s["consent"], s["ids"], s["counts"], s["sc"], NOW, IDLE, row_cap=row_cap, times=times)


def drive(fb, s, cuts, **kw):
    return np.concatenate([observe(fb, s, a, b, **kw) for a, b in zip(cuts, cuts[1:])])


def same_words(got, want):
    for k in WORDS:
        assert got[k].dtype == np.uint64 and got[k].shape == want[k].shape, k
        bad = np.argwhere(got[k] != want[k])
        assert not len(bad), (k, len(bad), bad[:6].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


# row_cap: 8 | 9 the lane-group switch of the rank kernel, 21 the default, 31 | 32 the replicate tile's switch (256 -> 64 lanes), 64 the limit.  B: one lane, a wave
# less and more than one lane, a wide tile plus one, 1024 plus one, the limit.  n: one request, a staged block of 128 less and more than filled twice, many blocks
CASES = [(1, 1, 1), (1, 4096, 257), (8, 63, 255), (8, 1025, 5000), (9, 65, 257), (9, 1, 5000), (21, 257, 5000), (21, 4096, 5000), (21, 63, 1),
         (31, 257, 255), (32, 257, 257), (32, 1025, 5000), (64, 4096, 255), (64, 65, 5000), (64, 1, 257)]


@pytest.mark.parametrize("row_cap,B,n", CASES)
def test_the_words_equal_the_model(row_cap, B, n):
    seed = 1000 * row_cap + n
    s = stream(n, row_cap, seed)
    fb = ClickFeedback(0, capacity=2 * n + 1, row_cap=row_cap, ttl_secs=TTL, idle_secs=IDLE, bootstrap=B, seed=seed)
    cuts = [0, n] if n < 5000 else [0, 2000, n]            # (the second call's run heads find their rows in the table)
    got_ranks = drive(fb, s, cuts, device=n == 257)
    ranks, ctr = model_ranks(s, row_cap)
    assert np.array_equal(got_ranks, ranks)
    got = fb.bootstrap()
    assert (got["replicates"], got["seed"]) == (B, seed)
    want = feedback_bootstrap_model(ranks, (s["hi"], s["lo"]), B, seed, row_cap)
    same_words(got, want)
    assert not got["hist_model"][:, 0].any() and not got["hist_filled"][:, 0].any()
    if n >= 255:   # no vacuous pass: observed requests, requests without consent and unserved rows, hits of both kinds, one of them at the row's last position
        assert ctr["observed"] > n // 3 and ctr["no_consent"] > 0 and (s["counts"] == NONE).any() and int(want["observed"].sum()) > 0
        assert ctr["hits_model"] > 0 and (row_cap == 1 or ctr["hits_filled"] > 0)
        assert ctr["hist_model"][row_cap] + ctr["hist_filled"][row_cap] > 0
        if B >= 63:
            assert want["hist_model"].any() and (row_cap == 1 or want["hist_filled"].any())
    # the sums of a replicate whose weights are all 1 would be the log's own counters: the words stay in that scale
    st = fb.stats()
    assert st["observed"] == ctr["observed"] and int(got["observed"].max()) <= 12 * st["observed"]
    fb.close()


@pytest.fixture(scope="module")
def five_thousand():
    """one stream and its model, shared by the tests below (none of them changes it)"""
    s = stream(5000, 21, 77)
    ranks, ctr = model_ranks(s, 21)
    want = feedback_bootstrap_model(ranks, (s["hi"], s["lo"]), 300, 9, 21)
    assert ctr["hits_model"] > 0 and ctr["hits_filled"] > 0 and ctr["no_consent"] > 0
    return dict(s=s, ranks=ranks, ctr=ctr, want=want)


def new_log(n=5000, row_cap=21, B=300, seed=9):
    return ClickFeedback(0, capacity=2 * n + 1, row_cap=row_cap, ttl_secs=TTL, idle_secs=IDLE, bootstrap=B, seed=seed)


def test_any_cut_into_calls_gives_the_same_words(five_thousand):
    s, want = five_thousand["s"], five_thousand["want"]
    one = new_log()
    assert np.array_equal(drive(one, s, [0, 5000]), five_thousand["ranks"])
    same_words(one.bootstrap(), want)
    cuts, sizes = [0], [1, 7, 1000]
    while cuts[-1] < 5000:
        cuts.append(min(5000, cuts[-1] + sizes[(len(cuts) - 1) % 3]))
    assert len(cuts) > 12
    cut = new_log()
    assert np.array_equal(drive(cut, s, cuts), five_thousand["ranks"])
    same_words(cut.bootstrap(), want)
    for fb in (one, cut):
        fb.close()


def test_entry_points_and_a_null_rank_buffer_give_the_same_words(five_thousand):
    import torch
    s, want, ctr = five_thousand["s"], five_thousand["want"], five_thousand["ctr"]
    plain = ClickFeedback(0, capacity=10001, row_cap=21, ttl_secs=TTL, idle_secs=IDLE)           # the bootstrap off: ranks and counters are what they are with it
    assert plain.bootstrap() is None and "bootstrap" not in plain.stats() and "mrr_ci" not in plain.stats()
    want_ranks = drive(plain, s, [0, 1500, 5000])
    host, dev, null = new_log(), new_log(), new_log()
    assert np.array_equal(drive(host, s, [0, 1500, 5000]), want_ranks) and np.array_equal(host.last_ranks, want_ranks[1500:])
    assert np.array_equal(drive(dev, s, [0, 1500, 5000], device=True), want_ranks)
    assert np.array_equal(dev.last_ranks.cpu().numpy().view(np.uint32), want_ranks[1500:])
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    for a, b in ((0, 1500), (1500, 5000)):   # d_out_rank = NULL: the log's own scratch carries the ranks to the bootstrap
        t = {k: to_device(s[k][a:b]) for k in ("hi", "lo", "items", "consent", "ids", "counts", "sc")}
        capi.check(capi.lib().srn_feedback_observe_device(null._h, p(t["hi"]), p(t["lo"]), p(t["items"]), p(t["consent"]), b - a, NOW, p(t["ids"]), p(t["sc"]),
                                                          p(t["counts"]), 21, None, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)))
        torch.cuda.synchronize()
    want_stats = plain.stats()
    for fb in (host, dev, null):
        same_words(fb.bootstrap(), want)
        st = fb.stats()
        assert {k: st[k] for k in COUNTERS} == {k: want_stats[k] for k in COUNTERS} == {k: ctr[k] for k in COUNTERS}
        assert all(np.array_equal(x, y) for x, y in zip(fb.histogram(), plain.histogram()))
        assert all(st[k] == want_stats[k] for k in want_stats)                                    # every existing key, the metrics among them
        # stats(): the arrays, and an interval per metric that holds the replicates' middle
        assert st["bootstrap"]["replicates"] == 300 and st["bootstrap"]["ci"] == 0.95 and st["bootstrap"]["empty_replicates"] == 0
        same_words(st["bootstrap"], want)
        for m in ("hit_rate", "mrr", "hit_rate_model", "mrr_model", "hit_rate_filled", "mrr_filled"):
            lo, hi = st[m + "_ci"]
            assert lo < st[m] < hi, (m, lo, st[m], hi)
        narrow = fb.stats(ci=0.5)
        assert st["mrr_ci"][0] < narrow["mrr_ci"][0] < narrow["mrr_ci"][1] < st["mrr_ci"][1] and narrow["bootstrap"]["ci"] == 0.5
    for fb in (plain, host, dev, null):
        fb.close()


@pytest.mark.parametrize("device", [False, True])
def test_a_timed_call_equals_one_call_per_request(device):
    """observe(..., times=) with gaps above idle_secs inside runs: the requests behind a gap are not observed and add nothing.  257 requests of 40 visitors in one
    call, against 257 calls at times[i], against the model."""
    n, row_cap, B, seed = 257, 8, 130, 4
    rng = np.random.default_rng(12)
    pool = [(int(h) << 64) | int(l) for h in (5, 6) for l in range(20)]
    keys = [pool[int(i)] for i in rng.integers(0, 40, n)]
    consent = (np.arange(n) % 6 != 0).astype(np.uint8)
    s = make_stream(21, keys, row_cap, consent)
    times = NOW + np.cumsum(np.where(rng.random(n) < 0.04, IDLE + 300, 2)).astype(np.uint64)   # a jump every 25 requests or so breaks every run that spans it
    ranks, ctr = model_ranks(s, row_cap, times=times)
    assert ctr["idle_expired"] >= 20 and ctr["observed"] >= 50 and ctr["hits_model"] + ctr["hits_filled"] > 0 and ctr["no_consent"] > 0
    want = feedback_bootstrap_model(ranks, (s["hi"], s["lo"]), B, seed, row_cap)
    timed, stepped = new_log(n, row_cap, B, seed), new_log(n, row_cap, B, seed)
    assert np.array_equal(observe(timed, s, 0, n, device=device, times=times), ranks)
    got = np.concatenate([observe(stepped, s, i, i + 1, now=int(times[i])) for i in range(n)])
    assert np.array_equal(got, ranks)
    same_words(timed.bootstrap(), want)
    same_words(stepped.bootstrap(), want)
    assert timed.stats()["idle_expired"] == ctr["idle_expired"]
    timed.close()
    stepped.close()


def test_lifecycle():
    L = capi.lib()
    s = stream(600, 9, 5)
    ranks, _ = model_ranks(s, 9)
    fb = ClickFeedback(0, capacity=2048, row_cap=9, ttl_secs=TTL, idle_secs=IDLE)
    B, seed = C.c_uint32(7), C.c_uint64(7)
    capi.check(L.srn_feedback_bootstrap_info(fb._h, C.byref(B), C.byref(seed)))
    assert (B.value, seed.value) == (0, 0) and fb.bootstrap() is None
    obs = np.zeros(8, np.uint64)
    assert L.srn_feedback_bootstrap_read(fb._h, capi.ptr(obs), None, None, 8, 10) == capi.SRN_ESTATE      # not enabled
    assert L.srn_feedback_bootstrap_disable(fb._h) == capi.SRN_OK                                        # ... which disable does not mind
    assert L.srn_feedback_bootstrap_enable(fb._h, 0, 1) == capi.SRN_EINVAL
    assert L.srn_feedback_bootstrap_enable(fb._h, capi.MAX_BOOTSTRAP + 1, 1) == capi.SRN_ERANGE
    observe(fb, s, 0, 200)                                                                               # before it is enabled: not in the words
    fb.enable_bootstrap(8, seed=3)
    assert L.srn_feedback_bootstrap_enable(fb._h, 8, 3) == capi.SRN_ESTATE                               # a second enable
    assert not fb.bootstrap()["observed"].any()
    observe(fb, s, 200, 600)
    want = feedback_bootstrap_model(ranks[200:], (s["hi"][200:], s["lo"][200:]), 8, 3, 9)
    assert want["observed"].all() and want["hist_model"].any()
    same_words(fb.bootstrap(), want)
    # read: caps too small are refused, wider ones are filled with 0; either histogram may be NULL
    hm = np.full((8, 12), 9, np.uint64)
    assert L.srn_feedback_bootstrap_read(fb._h, capi.ptr(obs), capi.ptr(hm), None, 7, 12) == capi.SRN_ERANGE
    assert L.srn_feedback_bootstrap_read(fb._h, capi.ptr(obs), capi.ptr(hm), None, 8, 9) == capi.SRN_ERANGE
    assert (hm == 9).all()
    capi.check(L.srn_feedback_bootstrap_read(fb._h, capi.ptr(obs), capi.ptr(hm), None, 8, 12))
    assert np.array_equal(obs, want["observed"]) and np.array_equal(hm[:, :10], want["hist_model"]) and not hm[:, 10:].any()
    # a sweep keeps the words (and drops every row: the clock is far ahead)
    assert fb.sweep(NOW + 10 * TTL) == 0
    same_words(fb.bootstrap(), want)
    # reset_counters zeroes them
    fb.reset_counters()
    assert fb.stats()["observed"] == 0 and fb.stats()["bootstrap"]["empty_replicates"] == 8 and fb.stats()["mrr_ci"] == (0.0, 0.0)
    assert not any(fb.bootstrap()[k].any() for k in WORDS)
    # disable, then enable with another B: from zero, with the new seed
    observe(fb, s, 0, 200)
    fb.disable_bootstrap()
    assert fb.bootstrap() is None and "bootstrap" not in fb.stats()
    observe(fb, s, 200, 400)                                                                             # while it is off
    fb.enable_bootstrap(70, seed=4)
    assert fb.bootstrap()["replicates"] == 70 and not fb.bootstrap()["observed"].any()
    got_ranks = observe(fb, s, 400, 600)
    assert np.array_equal(got_ranks, ranks[400:])                                                        # (the table kept its rows throughout)
    same_words(fb.bootstrap(), feedback_bootstrap_model(ranks[400:], (s["hi"][400:], s["lo"][400:]), 70, 4, 9))
    fb.close()
    # a log with rows wider than 64 ids cannot carry the bootstrap
    wide = ClickFeedback(0, capacity=64, row_cap=65, ttl_secs=TTL, idle_secs=IDLE)
    assert L.srn_feedback_bootstrap_enable(wide._h, 8, 1) == capi.SRN_ERANGE and wide.bootstrap() is None
    wide.close()
    with pytest.raises(capi.SerenadeError) as e:
        ClickFeedback(0, capacity=64, row_cap=65, ttl_secs=TTL, idle_secs=IDLE, bootstrap=8)
    assert e.value.code == capi.SRN_ERANGE


def test_a_call_refused_for_capacity_leaves_the_words():
    ks = [(int(h) << 64) | 5 for h in range(1, 6)]
    s = make_stream(13, ks[:2] + ks[:2] + ks[2:], 4)                   # two visitors twice in one call, then three more: live entries + batch > capacity, nothing is old
    fb = ClickFeedback(0, capacity=4, row_cap=4, ttl_secs=TTL, idle_secs=IDLE, bootstrap=33, seed=2)
    ranks = drive(fb, s, [0, 4])
    before, stats = fb.bootstrap(), fb.stats()
    assert stats["observed"] == 2 and before["observed"].any()
    same_words(before, feedback_bootstrap_model(ranks, (s["hi"][:4], s["lo"][:4]), 33, 2, 4))
    with pytest.raises(capi.SerenadeError) as e:
        observe(fb, s, 4, 7)
    assert e.value.code == capi.SRN_ENOMEM
    same_words(fb.bootstrap(), before)
    assert fb.stats()["refused"] == 1 and fb.stats()["observed"] == 2
    fb.close()


def test_two_replays_of_the_example_pair(tmp_path):
    """The reference's toy example: its test set replayed as a click log under k = 50 and under k = 100, on fresh stores and logs with one seed.  Whether a request is
    observed does not depend on the rows, so both logs resample the same visitors: equal `observed` arrays, a paired comparison."""
    from helpers import extract_example
    root = extract_example(tmp_path)
    index = sa.VMISIndex.new_from_csv(os.path.join(root, "train.txt"), 500, 1.0, device=0)
    rows = []
    with open(os.path.join(root, "test.txt")) as f:
        next(f)
        for line in f:
            parts = line.split()
            if len(parts) >= 3:
                rows.append((round(float(parts[2])), int(parts[0]), int(parts[1])))
    order = sorted(range(len(rows)), key=lambda i: rows[i][0])          # by time, the file's order within a second
    times = np.array([rows[i][0] for i in order], np.uint64)
    keys = (np.full(len(rows), 77, np.uint64), np.array([rows[i][1] for i in order], np.uint64))
    items = np.array([rows[i][2] for i in order], np.uint64)
    out = {}
    for k in (50, 100):
        store = serving.DeviceSessionStore(index, capacity=4096, items_cap=16)
        fb = ClickFeedback(index, capacity=4096, row_cap=20, bootstrap=256, seed=31)
        out[k] = serving.replay(index, store, keys, items, times, k=k, m=500, how_many=20, max_items_in_session=2, batch=400, feedback=fb)["feedback"]
        store.close()
        fb.close()
    a, b = out[50], out[100]
    assert a["observed"] == b["observed"] > 500 and a["bootstrap"]["replicates"] == 256
    assert np.array_equal(a["bootstrap"]["observed"], b["bootstrap"]["observed"]) and a["bootstrap"]["empty_replicates"] == 0
    for st in (a, b):
        for m in ("mrr", "hit_rate", "mrr_model", "hit_rate_model"):
            lo, hi = st[m + "_ci"]
            print("%s %.4f in (%.4f, %.4f)" % (m, st[m], lo, hi))
            assert 0.0 < lo <= st[m] <= hi < 1.0, (m, lo, st[m], hi)
        assert st["hit_rate_filled"] == 0.0 and st["hit_rate_filled_ci"] == (0.0, 0.0)       # nothing is filled here
    c = feedback_compare(a, b)
    print("k = 50 against k = 100: delta %.5f, ci (%.5f, %.5f), p_better %.3f" % (c["delta"], c["ci"][0], c["ci"][1], c["p_better"]))
    assert c["paired"] is True and c["replicates"] == 256 and c["delta"] == a["mrr"] - b["mrr"]
    assert c["ci"][0] <= c["ci"][1] and c["ci"][1] - c["ci"][0] < (a["mrr_ci"][1] - a["mrr_ci"][0])   # pairing: the difference is known better than either value
