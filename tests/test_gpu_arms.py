"""The traffic split on the GPU (srn_recommend_batch_split*, serving.TrafficSplit / recommend_batch_split): the device's assignment against the NumPy
rule, and the served rows, the shared store, an attached harvest and the arms' feedback logs against plain recommend_batch calls -- the code as it stood before.
The index, the stream of 2 000 requests and the two configurations are tests/test_gpu_replay.py's; arm_cases.py designs the keys."""
import ctypes as C
import threading
import warnings

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi
from serenade_amd.serving import (ClickFeedback, DeviceSessionStore, SessionHarvest, TrafficSplit, arm_draws, arm_thresholds, arms_model, recommend_batch,
                                  recommend_batch_split, replay)

import arm_cases as ac
from helpers import small_dataset
from test_gpu_replay import CONFIGS, FAR, HOW_MANY, IDLE, K, M, T0, TTL, export_bytes, index, stream  # noqa: F401  (index: the module's fixture)

pytestmark = pytest.mark.gpu

SEED = 7
FB_COUNTERS = ("live_bound", "requests", "no_consent", "first_seen", "idle_expired", "observed", "hits_model", "hits_filled", "stored")
NONE = capi.FEEDBACK_NONE


@pytest.fixture(scope="module")
def index2():
    off, items, ts, _ = small_dataset(34, n_sessions=1500, n_items=200)
    gix = sa.VMISIndex.from_sessions(off, items, ts, 200, 12, 1.0)
    gix.set_fallback_popular(64)
    yield gix
    gix.close()


def new_store(index, history=0, capacity=8192, harvest=True):
    store = DeviceSessionStore(index, capacity=capacity, items_cap=8, ttl_secs=TTL, idle_secs=IDLE, history=history)
    hv = None
    if harvest:
        hv = SessionHarvest(index, capacity=4096, items_cap=8, min_len=2)           # (room for every session: what a full harvest loses depends on the append order)
        store.set_harvest(hv)
    return store, hv


def new_log(index, capacity=8192, row_cap=HOW_MANY):
    return ClickFeedback(index, capacity=capacity, row_cap=row_cap, ttl_secs=TTL, idle_secs=IDLE)


def close(*objects):
    for o in objects:
        if o is not None:
            o.close()


def summed(logs):
    """the logs' integer counters and histograms, summed"""
    stats, hists = [fb.stats() for fb in logs], [fb.histogram() for fb in logs]
    assert all(s["sweeps"] == 0 and s["refused"] == 0 for s in stats)
    return {n: sum(s[n] for s in stats) for n in FB_COUNTERS}, (sum(h[0] for h in hists), sum(h[1] for h in hists))


def serve(index, cfg, calls, reqs, split=None, arms=None):
    """test_gpu_replay.serve, through one log and recommend_batch -- or, with a split, through recommend_batch_split and a log per arm (arms: the dicts without
    their logs).  calls: [(start, stop, now or None)], None: a timed call"""
    (hi, lo), items, consent, times = reqs
    store, hv = new_store(index, cfg["history"])
    logs = [new_log(index) for _ in range(len(arms) if split is not None else 1)]
    rows, ranks, got_arms = [], [], []
    for a, b, now in calls:
        sl = slice(a, b)
        kw = dict(now=now) if now is not None else dict(times=times[sl])
        con = None if consent is None else consent[sl]
        if split is None:
            rows.append(recommend_batch(index, store, (hi[sl], lo[sl]), items[sl], con, k=K, m=M, how_many=HOW_MANY, max_items_in_session=2, scores=True, feedback=logs[0],
                                        **cfg["flags"], **kw))
            ranks.append(logs[0].last_ranks)
        else:
            rows.append(recommend_batch_split(split, [dict(arm, feedback=fb) for arm, fb in zip(arms, logs)], store, (hi[sl], lo[sl]), items[sl], con, how_many=HOW_MANY,
                                              scores=True, **kw))
            ranks.append(split.last_ranks)
            got_arms.append(split.last_arms)
            assert split.last_errors == [None] * len(arms) and all(fb.last_ranks is None for fb in logs)      # the logs' own last_ranks are not touched
    out = dict(ids=np.concatenate([r[0] for r in rows]), counts=np.concatenate([r[1] for r in rows]), scores=np.concatenate([r[2] for r in rows]),
               ranks=np.concatenate(ranks), arms=np.concatenate(got_arms) if got_arms else None, store=store.export(now=1), store_stats=store.stats)
    out["fb"], out["fb_hist"] = summed(logs)
    out["per_log"] = [fb.stats() for fb in logs]
    store.sweep(FAR)
    out["hv"], out["hv_stats"] = hv.export(), hv.stats()
    close(store, hv, *logs)
    return out


def assert_same(got, ref, what):
    for name in ("ids", "counts", "scores", "ranks"):
        assert got[name].tobytes() == ref[name].tobytes(), (what, name, np.flatnonzero((got[name] != ref[name]).reshape(len(ref[name]), -1).any(axis=1))[:8])
    assert export_bytes(got["store"]) == export_bytes(ref["store"]) and len(got["store"][1]) == len(ref["store"][1]), (what, "store")
    assert got["store_stats"] == ref["store_stats"], (what, got["store_stats"], ref["store_stats"])
    assert got["store_stats"]["sweeps"] == 0 and got["store_stats"]["refused"] == 0                           # no automatic sweep ran (the logs': summed())
    assert export_bytes(got["hv"]) == export_bytes(ref["hv"]), (what, "harvest", len(got["hv"][1]), len(ref["hv"][1]))
    for name in ("stored", "stored_items", "skipped_short", "lost"):
        assert got["hv_stats"][name] == ref["hv_stats"][name], (what, name)
    assert got["hv_stats"]["from_return"] + got["hv_stats"]["from_rebuild"] == ref["hv_stats"]["from_return"] + ref["hv_stats"]["from_rebuild"], what
    assert got["fb"] == ref["fb"], (what, got["fb"], ref["fb"])
    assert all(np.array_equal(x, y) for x, y in zip(got["fb_hist"], ref["fb_hist"])), what


def same_arms(index, cfg, n_arms):
    return [dict(index=index, k=K, m=M, max_items_in_session=2, **cfg["flags"]) for _ in range(n_arms)]


def to_gpu(index, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(torch.device("cuda", index.info["device"]))


# ---- 1. the assignment on the device equals the model ----
@pytest.mark.parametrize("weights", ac.WEIGHT_SETS, ids=lambda w: "w%d_%d" % (len(w), w[0] % 97))
def test_assignment_on_the_device_equals_the_model(index, weights):
    A = len(weights)
    sizes = [1, 63, 64, 65, 255, 256, 257, 1000] + ([65795] if A in (2, 3, 16) and weights[0] == 1 else [])   # 65 795 requests: 258 blocks, the offsets scan loops
    split = TrafficSplit(index, weights, seed=SEED, max_batch=max(sizes), max_how_many=4)
    store, _ = new_store(index, capacity=1 << 18, harvest=False)
    arms = [dict(index=index, k=K, m=M) for _ in range(A)]
    rng = np.random.default_rng(A)
    (thi, tlo), _, tarm = ac.threshold_keys(SEED, weights)
    served = np.zeros(A, np.int64)
    for j, n in enumerate(sizes):
        hi, lo = rng.integers(0, 2 ** 64, n, dtype=np.uint64), rng.integers(0, 2 ** 64, n, dtype=np.uint64)
        at = rng.permutation(n)[:len(thi)]                                        # the designed threshold keys mixed in, as many as fit
        hi[at], lo[at] = thi[:len(at)], tlo[:len(at)]
        items = index.known_ids[rng.integers(0, 40, n)]
        want = arms_model(SEED, weights, (hi, lo))
        assert np.array_equal(want[at], tarm[:len(at)])
        if j % 2:                                                                 # tensors, read in place
            ids, counts = recommend_batch_split(split, arms, store, (to_gpu(index, hi), to_gpu(index, lo)), to_gpu(index, items), how_many=4, now=T0)
            got, ranks = split.last_arms.cpu().numpy(), split.last_ranks.cpu().numpy().view(np.uint32)
            counts = counts.cpu().numpy().view(np.uint32)
        else:
            ids, counts = recommend_batch_split(split, arms, store, (hi, lo), items, how_many=4, now=T0)
            got, ranks = split.last_arms, split.last_ranks
        assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (n, np.flatnonzero(got != want)[:8])
        assert bool((ranks == NONE).all()) and bool((counts <= 4).all())
        served += np.bincount(want, minlength=A)
    info = split.info()
    assert info["served"] == served.tolist() and info["thresholds"] == arm_thresholds(weights) and info["n_arms"] == A and info["seed"] == SEED
    assert (info["calls"], info["shortcut_calls"]) == (len(sizes), 0) and info["device_bytes"] > 0
    assert np.array_equal(split.arm_of((thi, tlo)), tarm)
    close(split, store)


# ---- 2. identical arms are the plain call ----
@pytest.mark.parametrize("n_arms", [2, 3])
@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_identical_arms_are_the_plain_call(index, name, timed, n_arms):
    cfg = CONFIGS[name]
    keys, items, consent, times, edges = stream(index)
    n = len(items)
    weights = [9, 1] if n_arms == 2 else [1, 2, 1]
    calls = [(0, 1000, None), (1000, n, None)] if timed else [(int(a), int(b), int(times[a])) for a, b in zip(edges, edges[1:])]
    split = TrafficSplit(index, weights, seed=SEED, max_batch=1000, max_how_many=HOW_MANY)
    seqs = ac.sequences(n, n_arms)
    for seq_name in (("alternating", "runs_of_64") if n_arms == 2 else ("runs_of_63", "runs_of_65")):
        reqs = (ac.rekey(SEED, weights, keys, seqs[seq_name]), items, consent, times)
        ref = serve(index, cfg, calls, reqs)
        got = serve(index, cfg, calls, reqs, split=split, arms=same_arms(index, cfg, n_arms))
        assert np.array_equal(got["arms"], seqs[seq_name])
        assert_same(got, ref, (name, timed, n_arms, seq_name))
        assert int(ref["counts"].max()) > 0 and ref["fb"]["hits_model"] + ref["fb"]["hits_filled"] > 0 and len(ref["hv"][1]) > 20
        assert [s["requests"] for s in got["per_log"]] == np.bincount(seqs[seq_name], minlength=n_arms).tolist()
    split.close()


# ---- 3. different arms ----
@pytest.mark.parametrize("timed", [False, True], ids=["untimed", "timed"])
def test_different_arms_are_their_sub_batches_served_one_after_the_other(index, index2, timed):
    keys, items, consent, times, edges = stream(index)
    n = len(items)
    weights = [2, 1, 1]
    arms = [dict(index=index, k=K, m=M, max_items_in_session=2), dict(index=index2, k=30, m=100, max_items_in_session=4, exclude_seen=True, fill=True),
            dict(index=index, k=20, m=150, max_items_in_session=4, fill=True)]
    calls = [(0, 700, None), (700, n, None)] if timed else [(int(a), int(b), int(times[a])) for a, b in zip(edges[:-1:4], list(edges[4::4]) + [n])]
    split = TrafficSplit(index, weights, seed=SEED, max_batch=2000, max_how_many=HOW_MANY)
    want_arm = arms_model(SEED, weights, keys)
    assert all(np.count_nonzero(want_arm == a) > 200 for a in range(3))
    store, hv = new_store(index, history=6)
    ref_store, ref_hv = new_store(index, history=6)
    logs, ref_logs = [new_log(index) for _ in arms], [new_log(index) for _ in arms]
    for a, b, now in calls:
        sl = slice(a, b)
        kw = dict(now=int(times[a])) if timed else dict(now=now)                 # (timed: the sweep clock, the same for the arms' reference calls)
        ids, counts, scores = recommend_batch_split(split, [dict(arm, feedback=fb) for arm, fb in zip(arms, logs)], store, (keys[0][sl], keys[1][sl]), items[sl], consent[sl],
                                                    how_many=HOW_MANY, scores=True, times=times[sl] if timed else None, **kw)
        assert np.array_equal(split.last_arms, want_arm[sl])
        for x, arm in enumerate(arms):                                           # the reference: the arm's requests alone, in order, arm 0 first
            sub = a + np.flatnonzero(want_arm[sl] == x)
            if not len(sub):
                continue
            params = {k_: v for k_, v in arm.items() if k_ != "index"}
            r_ids, r_counts, r_scores = recommend_batch(arm["index"], ref_store, (keys[0][sub], keys[1][sub]), items[sub], consent[sub], how_many=HOW_MANY, scores=True,
                                                        feedback=ref_logs[x], times=times[sub] if timed else None, **params, **kw)
            at = sub - a
            assert ids[at].tobytes() == r_ids.tobytes() and counts[at].tobytes() == r_counts.tobytes() and scores[at].tobytes() == r_scores.tobytes(), (a, x)
            assert split.last_ranks[at].tobytes() == ref_logs[x].last_ranks.tobytes(), (a, x)
    assert export_bytes(store.export(now=1)) == export_bytes(ref_store.export(now=1)) and store.stats == ref_store.stats and store.stats["sweeps"] == 0
    for fb, ref_fb in zip(logs, ref_logs):
        assert fb.stats() == ref_fb.stats() and all(np.array_equal(x, y) for x, y in zip(fb.histogram(), ref_fb.histogram()))
        assert fb.stats()["observed"] > 50
    store.sweep(FAR), ref_store.sweep(FAR)
    assert export_bytes(hv.export()) == export_bytes(ref_hv.export())
    assert split.info()["served"] == np.bincount(want_arm, minlength=3).tolist()
    close(split, store, hv, ref_store, ref_hv, *logs, *ref_logs)


# ---- 4. one visitor's clicks stay in order ----
def test_one_visitor_of_3000_requests_among_others(index):
    cfg = CONFIGS["h6_exclude_fill"]
    rng = np.random.default_rng(11)
    n_one, n_other = 3000, 1500
    n = n_one + n_other
    mine = np.zeros(n, bool)
    mine[rng.permutation(n)[:n_one]] = True
    hi, lo = np.where(mine, np.uint64(77), rng.integers(100, 400, n).astype(np.uint64)), np.where(mine, np.uint64(99), np.uint64(5))
    items = index.known_ids[rng.integers(0, 12, n)]
    weights = [1, 1]
    split = TrafficSplit(index, weights, seed=SEED, max_batch=n, max_how_many=HOW_MANY)
    reqs = ((hi, lo), items, None, np.full(n, T0, np.uint64))
    ref = serve(index, cfg, [(0, n, T0)], reqs)
    got = serve(index, cfg, [(0, n, T0)], reqs, split=split, arms=same_arms(index, cfg, 2))
    assert_same(got, ref, "one visitor")
    assert len(set(got["arms"][mine].tolist())) == 1 and len(set(got["arms"][~mine].tolist())) == 2
    # the visitor's final window (compared with the plain call's by assert_same) is full and ends with its last click
    at = int(np.flatnonzero((got["store"][0][0] == 77) & (got["store"][0][1] == 99))[0])
    assert got["store"][2][at] == 6 and int(got["store"][3][at][5]) == int(items[mine][-1])
    split.close()


# ---- 5. empty arms, 6. one arm ----
def test_empty_arms_and_one_request(index):
    cfg = CONFIGS["limit2"]
    keys, items, consent, times, _ = stream(index)
    sl = slice(0, 300)
    for weights, full in (([1, 1, 1], 0), ([1, 1, 1], 1), ([1, 1, 1], 2), ([1, 0, 1], None), ([0, 0, 5], None), ([5, 0, 0], None)):
        split = TrafficSplit(index, weights, seed=SEED, max_batch=300, max_how_many=HOW_MANY)
        k_ = (keys[0][sl], keys[1][sl]) if full is None else ac.rekey(SEED, weights, (keys[0][sl], keys[1][sl]), np.full(300, full, np.uint8))
        reqs = (k_, items[sl], consent[sl], times[sl])
        ref = serve(index, cfg, [(0, 300, T0)], reqs)
        got = serve(index, cfg, [(0, 300, T0)], reqs, split=split, arms=same_arms(index, cfg, 3))
        assert_same(got, ref, (weights, full))
        want = arms_model(SEED, weights, k_)
        assert np.array_equal(got["arms"], want) and split.info()["served"] == np.bincount(want, minlength=3).tolist()
        assert all(np.count_nonzero(want == a) == 0 for a in range(3) if weights[a] == 0) and (full is None or bool((want == full).all()))
        # n = 1, and n = 0
        one = serve(index, cfg, [(7, 8, T0)], reqs, split=split, arms=same_arms(index, cfg, 3))
        assert_same(one, serve(index, cfg, [(7, 8, T0)], reqs), (weights, full, "n = 1"))
        store, _ = new_store(index, harvest=False)
        ids, counts = recommend_batch_split(split, same_arms(index, cfg, 3), store, (k_[0][:0], k_[1][:0]), items[:0], how_many=HOW_MANY, now=T0)
        assert ids.shape == (0, HOW_MANY) and counts.shape == (0,) and split.info()["calls"] == 2
        close(split, store)


def test_one_arm_is_the_plain_call_on_the_callers_buffers(index):
    keys, items, consent, times, edges = stream(index)
    n = len(items)
    for name, cfg in CONFIGS.items():
        split = TrafficSplit(index, [3], seed=SEED, max_batch=n, max_how_many=HOW_MANY)
        assert split.info()["device_bytes"] == 0                                  # no scratch
        calls = [(0, 1000, None), (1000, n, None)]
        reqs = (keys, items, consent, times)
        got = serve(index, cfg, calls, reqs, split=split, arms=same_arms(index, cfg, 1))
        assert_same(got, serve(index, cfg, calls, reqs), name)
        info = split.info()
        assert (info["calls"], info["shortcut_calls"], info["served"]) == (0, 2, [n]) and not got["arms"].any()
        split.close()


# ---- 7. nothing is written beyond n; the optional outputs may be NULL ----
def test_guard_rows_and_null_outputs_on_the_device_form(index):
    import torch
    keys, items, consent, times, _ = stream(index)
    n, guard, hm = 300, 16, HOW_MANY
    dev = torch.device("cuda", index.info["device"])
    split = TrafficSplit(index, [1, 1], seed=SEED, max_batch=n, max_how_many=hm)
    store, _ = new_store(index, harvest=False)
    fb = new_log(index)
    d = [to_gpu(index, a[:n]) for a in (keys[0], keys[1], items, consent)]
    ids = torch.full(((n + guard) * hm,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    sc = torch.full(((n + guard) * hm,), -7.5, dtype=torch.float64, device=dev)
    cnt, rank = torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=dev), torch.full((n + guard,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    arm = torch.full((n + guard,), 0x5A, dtype=torch.uint8, device=dev)
    arms = (capi.Arm * 2)(capi.Arm(index._h, fb._h, 2, K, M, 0), capi.Arm(index._h, None, 2, K, M, 0))
    stream_p = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    call = lambda arm_p, rank_p, rc_p: capi.lib().srn_recommend_batch_split_device(   # noqa: E731
        split._h, arms, 2, store._h, ptr(d[0]), ptr(d[1]), ptr(d[2]), ptr(d[3]), None, n, T0, hm, ptr(ids), ptr(sc), ptr(cnt), arm_p, rank_p, rc_p, stream_p)
    rc = (C.c_int * 2)(5, 5)
    capi.check(call(ptr(arm), ptr(rank), rc))
    torch.cuda.current_stream(dev).synchronize()
    assert list(rc) == [0, 0]
    assert bool((ids[n * hm:] == 0x5A5A5A5A5A5A5A5A).all()) and bool((sc[n * hm:] == -7.5).all()) and bool((cnt[n:] == 0x5A5A5A5A).all())
    assert bool((rank[n:] == 0x5A5A5A5A).all()) and bool((arm[n:] == 0x5A).all())
    h_cnt, h_arm, h_ids = cnt[:n].cpu().numpy(), arm[:n].cpu().numpy(), ids[:n * hm].cpu().numpy().reshape(n, hm)
    assert np.array_equal(h_arm, arms_model(SEED, [1, 1], (keys[0][:n], keys[1][:n]))) and bool((h_cnt >= 0).all()) and bool((h_cnt <= hm).all()) and int(h_cnt.max()) > 0
    beyond = np.arange(hm)[None, :] >= h_cnt[:, None]
    assert bool((h_ids[beyond] == 0x5A5A5A5A5A5A5A5A).all()) and not bool((h_ids[~beyond] == 0x5A5A5A5A5A5A5A5A).any())   # as the plain call: entries beyond a row's count are not written
    assert bool((rank[:n].cpu().numpy().view(np.uint32)[h_arm == 1] == NONE).all())                           # arm 1 has no log
    capi.check(call(None, None, None))
    torch.cuda.current_stream(dev).synchronize()
    assert fb.stats()["requests"] == 2 * int(np.count_nonzero(h_arm == 0)) and split.info()["calls"] == 2
    close(split, store, fb)


# ---- 8. refusals change nothing ----
def test_refusals_change_nothing(index):
    keys, items, consent, times, _ = stream(index)
    cfg = CONFIGS["limit2"]
    weights = [1, 1]
    split = TrafficSplit(index, weights, seed=SEED, max_batch=400, max_how_many=HOW_MANY)
    store, hv = new_store(index, history=3)
    logs = [new_log(index), new_log(index)]
    small_log = new_log(index, row_cap=8)
    good = [dict(index=index, k=K, m=M, max_items_in_session=2, feedback=fb) for fb in logs]
    sl = slice(0, 400)
    args = ((keys[0][sl], keys[1][sl]), items[sl], consent[sl])
    recommend_batch_split(split, good, store, *args, how_many=HOW_MANY, now=T0)
    state = lambda: (export_bytes(store.export(now=1)), [fb.stats() for fb in logs], [fb.histogram()[0].tobytes() for fb in logs], split.info(), hv.stats())   # noqa: E731
    before = state()

    def refused(code, arms=good, how_many=HOW_MANY, n=400, st=store):
        with pytest.raises(capi.SerenadeError) as e:
            recommend_batch_split(split, arms, st, (keys[0][:n], keys[1][:n]), items[:n], consent[:n], how_many=how_many, now=T0)
        assert e.value.code == code, (e.value.code, code, str(e.value))
        assert state() == before

    bad_flag = (capi.Arm * 2)(capi.Arm(index._h, logs[0]._h, 2, K, M, 0), capi.Arm(index._h, logs[1]._h, 2, K, M, 64))
    hi, lo, it = (capi.as_u64(a[sl]) for a in (keys[0], keys[1], items))
    con = np.ascontiguousarray(consent[sl])
    out = np.zeros((400, HOW_MANY), np.uint64), np.zeros((400, HOW_MANY)), np.zeros(400, np.uint32)
    p = capi.ptr
    raw = lambda arm_array, n_arms=2, n=400, ids=out[0]: capi.lib().srn_recommend_batch_split(   # noqa: E731
        split._h, arm_array, n_arms, store._h, p(hi), p(lo), p(it), p(con), None, n, T0, HOW_MANY, p(ids), p(out[1]), p(out[2]), None, None, None)
    assert raw(bad_flag) == capi.SRN_EINVAL and state() == before                                            # a bad flag in arm 1
    assert raw(bad_flag, n_arms=3) == capi.SRN_EINVAL and raw(bad_flag, n_arms=17) == capi.SRN_ERANGE and raw(None) == capi.SRN_EINVAL
    assert raw((capi.Arm * 2)(bad_flag[0], bad_flag[0])) == capi.SRN_EINVAL                                  # one log in two arms
    assert raw((capi.Arm * 2)(bad_flag[0], capi.Arm(index._h, None, 2, K, M, 0)), ids=None) == capi.SRN_EINVAL   # a NULL output
    assert raw((capi.Arm * 2)(bad_flag[0], capi.Arm(None, None, 2, K, M, 0))) == capi.SRN_EINVAL             # a NULL index
    assert raw((capi.Arm * 2)(bad_flag[0], capi.Arm(index._h, None, 2, 0, M, 0))) == capi.SRN_EINVAL         # k = 0
    assert raw((capi.Arm * 2)(bad_flag[0], capi.Arm(index._h, None, 2, K, M, 0)), n=0) == capi.SRN_OK and state() == before
    refused(capi.SRN_ERANGE, [good[0], dict(good[1], max_items_in_session=4)])                                # arm 1's window above the history (3), arm 0 valid
    refused(capi.SRN_ERANGE, [good[0], dict(good[1], max_items_in_session=9)])                                # ... and above the store's items_cap
    no_ranking = sa.VMISIndex.from_sessions(*small_dataset(35, n_sessions=200, n_items=50)[:3], 200, 12, 1.0)
    refused(capi.SRN_ESTATE, [good[0], dict(index=no_ranking, k=K, m=M, fill=True)])                         # fill without a ranking on arm 1's index
    refused(capi.SRN_ERANGE, n=401)                                                                           # n > max_batch
    refused(capi.SRN_ERANGE, how_many=HOW_MANY + 1)                                                           # how_many > max_how_many
    refused(capi.SRN_ERANGE, [good[0], dict(good[1], feedback=small_log)])                                    # a log's row_cap below how_many
    with pytest.raises(capi.SerenadeError) as e:
        split.set_weights([1, 1, 1])
    assert e.value.code == capi.SRN_EINVAL and state() == before
    # a store that arm 0's share fits and the whole batch does not: refused whole, nothing stored
    tight, _ = new_store(index, capacity=300, harvest=False)
    share = int(np.count_nonzero(arms_model(SEED, weights, args[0]) == 0))
    assert share <= 300 < 400
    with pytest.raises(capi.SerenadeError) as e:
        recommend_batch_split(split, good, tight, *args, how_many=HOW_MANY, now=T0)
    assert e.value.code == capi.SRN_ENOMEM and len(tight.export(now=1)[1]) == 0 and tight.stats["refused"] == 1 and state() == before
    close(split, store, hv, tight, small_log, no_ranking, *logs)


# ---- 9. a log that refuses does not fail the call ----
def test_a_log_that_refuses_does_not_fail_the_call(index):
    keys, items, consent, times, _ = stream(index)
    cfg = CONFIGS["limit2"]
    weights = [1, 1]
    sl = slice(0, 600)
    reqs = ((keys[0][sl], keys[1][sl]), items[sl], consent[sl])
    want = arms_model(SEED, weights, reqs[0])
    split = TrafficSplit(index, weights, seed=SEED, max_batch=600, max_how_many=HOW_MANY)
    store, _ = new_store(index, harvest=False)
    ref_store, _ = new_store(index, harvest=False)
    full, other = new_log(index, capacity=16), new_log(index)
    arms = [dict(index=index, k=K, m=M, feedback=full), dict(index=index, k=K, m=M, feedback=other)]
    with pytest.warns(RuntimeWarning):
        ids, counts = recommend_batch_split(split, arms, store, *reqs, how_many=HOW_MANY, now=T0)
    r_ids, r_counts = recommend_batch(index, ref_store, *reqs, k=K, m=M, how_many=HOW_MANY, now=T0)
    assert ids.tobytes() == r_ids.tobytes() and counts.tobytes() == r_counts.tobytes()                       # the rows are served
    assert isinstance(split.last_errors[0], capi.SerenadeError) and split.last_errors[0].code == capi.SRN_ENOMEM and split.last_errors[1] is None
    assert bool((split.last_ranks[want == 0] == NONE).all())
    assert full.stats()["requests"] == 0 and full.stats()["refused"] == 1 and other.stats()["requests"] == int(np.count_nonzero(want == 1))   # the other arm's log is fed
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        recommend_batch_split(split, [dict(arms[0], feedback=None), arms[1]], store, *reqs, how_many=HOW_MANY, now=T0 + 1)
    assert split.last_errors == [None, None] and other.stats()["observed"] > 0 and bool((split.last_ranks[want == 1] != NONE).any())
    close(split, store, ref_store, full, other)


# ---- 10. any cut into calls; replay; the ramp ----
def test_any_cut_into_calls_and_replay(index, index2):
    keys, items, consent, times, _ = stream(index)
    n = len(items)
    cfg = CONFIGS["h6_exclude_fill"]
    weights = [3, 1]
    arms = [dict(index=index, k=K, m=M, max_items_in_session=2, **cfg["flags"]), dict(index=index2, k=30, m=100, max_items_in_session=4, fill=True)]
    split = TrafficSplit(index, weights, seed=SEED, max_batch=n, max_how_many=HOW_MANY)
    reqs = (keys, items, consent, times)
    ref = serve(index, cfg, [(0, n, None)], reqs, split=split, arms=arms)
    assert np.array_equal(ref["arms"], arms_model(SEED, weights, keys))
    for cut in (1, 7, 256):
        if cut == 1:                                                              # one request per call: the first 300, against the same cut of 300 in one call
            got = serve(index, cfg, [(i, i + 1, None) for i in range(300)], reqs, split=split, arms=arms)
            want = serve(index, cfg, [(0, 300, None)], reqs, split=split, arms=arms)
        else:
            got, want = serve(index, cfg, [(a, min(a + cut, n), None) for a in range(0, n, cut)], reqs, split=split, arms=arms), ref
        assert_same(got, want, cut)
        assert np.array_equal(got["arms"], want["arms"]) and got["per_log"] == want["per_log"]
    # replay(split=, arms=) against the loop written out by hand
    def run(by_hand):
        store, hv = new_store(index, history=6)
        logs = [new_log(index), new_log(index)]
        with_logs = [dict(arm, feedback=fb) for arm, fb in zip(arms, logs)]
        if by_hand:
            rows = []
            for a in range(0, n, 700):
                sl = slice(a, min(a + 700, n))
                r = recommend_batch_split(split, with_logs, store, (keys[0][sl], keys[1][sl]), items[sl], consent[sl], how_many=HOW_MANY, times=times[sl], now=int(times[a]))
                rows.append(r + (split.last_ranks, split.last_arms))
            out = {name: np.concatenate([r[j] for r in rows]) for j, name in enumerate(("ids", "counts", "ranks", "arm"))}
            out.update(calls=len(rows), feedback=[fb.stats() for fb in logs], arms=np.bincount(out["arm"], minlength=2).tolist())
        else:
            out = replay(None, store, keys, items, times, consent, k=0, m=0, how_many=HOW_MANY, batch=700, collect=True, split=split, arms=with_logs)
        out["store"] = export_bytes(store.export(now=1))
        close(store, hv, *logs)
        return out
    hand, got = run(True), run(False)
    assert got["calls"] == hand["calls"] == 3 and got["requests"] == n and got["arms"] == hand["arms"] and got["feedback"] == hand["feedback"]
    for name in ("ids", "counts", "ranks", "arm"):
        assert got[name].tobytes() == hand[name].tobytes(), name
    assert got["store"] == hand["store"]
    # the ramp: set_weights between calls moves only the keys whose u lies between the old and the new threshold
    store, _ = new_store(index, harvest=False)
    plain = [dict(index=index, k=K, m=M), dict(index=index, k=K, m=M)]
    recommend_batch_split(split, plain, store, keys, items, consent, how_many=HOW_MANY, now=T0)
    old = split.last_arms.copy()
    split.set_weights([1, 1])
    recommend_batch_split(split, plain, store, keys, items, consent, how_many=HOW_MANY, now=T0)
    u = arm_draws(SEED, keys)
    lo_T, hi_T = arm_thresholds([1, 1])[0], arm_thresholds(weights)[0]
    assert np.array_equal(split.last_arms != old, (u >= np.uint64(lo_T)) & (u < np.uint64(hi_T))) and bool((split.last_arms != old).any())
    assert np.array_equal(split.last_arms, arms_model(SEED, [1, 1], keys)) and split.info()["thresholds"] == arm_thresholds([1, 1])
    close(split, store)


# ---- 11. two threads on one handle ----
def test_two_threads_on_one_handle_with_disjoint_keys(index, index2):
    keys, items, consent, times, _ = stream(index)
    half = 1000
    hi = keys[0].copy()
    hi[half:] ^= np.uint64(1 << 40)                                               # the second thread's visitors are nobody the first one serves
    weights = [1, 1]
    arms = [dict(index=index, k=K, m=M), dict(index=index2, k=30, m=100, fill=True)]
    split = TrafficSplit(index, weights, seed=SEED, max_batch=half, max_how_many=HOW_MANY)
    store, _ = new_store(index, harvest=False)
    results, errors = {}, []

    def work(which):
        try:
            sl = slice(which * half, (which + 1) * half)
            rows = []
            for a in range(sl.start, sl.stop, 250):
                s2 = slice(a, a + 250)
                ids, counts = recommend_batch_split(split, arms, store, (hi[s2], keys[1][s2]), items[s2], consent[s2], how_many=HOW_MANY, now=T0)
                rows.append((ids, counts))
            results[which] = (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]))
        except Exception as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,)) for w in (0, 1)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    ref_store, _ = new_store(index, harvest=False)
    want_arm = arms_model(SEED, weights, (hi, keys[1]))
    for which in (0, 1):                                                          # every request is served, each with its arm's row
        for a in range(which * half, (which + 1) * half, 250):
            s2 = slice(a, a + 250)
            for x, arm in enumerate(arms):
                sub = a + np.flatnonzero(want_arm[s2] == x)
                params = {k_: v for k_, v in arm.items() if k_ != "index"}
                r_ids, r_counts = recommend_batch(arm["index"], ref_store, (hi[sub], keys[1][sub]), items[sub], consent[sub], how_many=HOW_MANY, now=T0, **params)
                at = sub - which * half
                assert results[which][0][at].tobytes() == r_ids.tobytes() and results[which][1][at].tobytes() == r_counts.tobytes(), (which, a, x)
    assert export_bytes(store.export(now=1)) == export_bytes(ref_store.export(now=1))
    info = split.info()
    assert info["calls"] == 8 and sum(info["served"]) == 2 * half
    close(split, store, ref_store)
