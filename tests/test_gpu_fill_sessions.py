"""SRN_FLAG_FILL behind the session store and in the evaluation (srn_fill.hip): srn_recommend_batch* fills a request's short row leaving out what the request
excludes (with SRN_FLAG_EXCLUDE_SEEN its window), and a trial of srn_evaluate with the flag scores the filled rows.

The requests are served by the per-request Python model of tests/test_gpu_exclude_sessions.py, their rows are the canonical CPU oracle's through filter_rows and fill_rows.
"""
import os

import numpy as np
import pytest

from fill_cases import K, M, OracleRows, check_rows, popularity_order, sparse_dataset
from helpers import eight_metrics, evaluator_queries, extract_example, flatten, read_test_data_evolving

pytestmark = pytest.mark.gpu

HOW_MANY, H, MAX_ITEMS = 21, 4, 2
U64 = 2**64 - 1


class Model:
    """The handler's session logic with `limit` items kept: read under the idle rule, append unless the click repeats the last item, drop ONE from the front beyond the
    limit, store with now.  A request sees (window, the session predict reads)."""

    def __init__(self, limit, idle=1200):
        self.limit, self.idle, self.s = limit, idle, {}

    def get(self, key, now):
        sess, t = self.s.get(key, ([], 0))
        return [] if now > t and now - t > self.idle else list(sess)

    def serve(self, key, item, consent, now, max_items):
        if not consent:
            return [item], [item]
        sess = self.get(key, now)
        if not sess or sess[-1] != item:
            sess.append(item)
            if len(sess) > self.limit:
                sess.pop(0)
        self.s[key] = (sess, now)
        return list(sess), sess[-max_items:]


def key_of(v):
    return (0x1234567800000000 + v) << 64 | (0xABCDEF0000000000 + 7919 * v)


def calls(order, n_calls=4, per_call=500, visitors=300, seed=7):
    """2 000 requests over 300 keys in four calls: items by popularity, 10 % of them unknown to the index, 10 % of the requests without consent."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, len(order) + 1) ** 0.9
    w /= w.sum()
    out, now = [], 50_000
    for _ in range(n_calls):
        now += 30
        reqs = []
        for _ in range(per_call):
            item = int(900_000 + rng.integers(0, 1000)) if rng.random() < 0.1 else int(order[rng.choice(len(order), p=w)])
            reqs.append((int(rng.integers(0, visitors)), item, bool(rng.random() >= 0.1)))
        out.append((now, reqs))
    return out


def run(gix, store, reqs, now, entry, exclude_seen, fill):
    from serenade_amd.serving import recommend_batch
    hi = np.array([key_of(v) >> 64 for v, _, _ in reqs], np.uint64)
    lo = np.array([key_of(v) & U64 for v, _, _ in reqs], np.uint64)
    it = np.array([i for _, i, _ in reqs], np.uint64)
    con = np.array([c for _, _, c in reqs], np.uint8)
    if entry == "device":
        import torch
        dev = torch.device("cuda", gix.info["device"])
        hi, lo, it = (torch.from_numpy(a.view(np.int64)).to(dev) for a in (hi, lo, it))
        con = torch.from_numpy(con).to(dev)
    ids, cnt, sc = recommend_batch(gix, store, (hi, lo), it, con, k=K, m=M, how_many=HOW_MANY, max_items_in_session=MAX_ITEMS, now=now, scores=True, exclude_seen=exclude_seen,
                                   fill=fill)
    if entry == "device":
        import torch
        torch.cuda.current_stream(gix.info["device"]).synchronize()
        ids, sc, cnt = ids.cpu().numpy().view(np.uint64), sc.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)
    return ids, sc, cnt


@pytest.fixture(scope="module")
def sparse():
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = sparse_dataset()
    gix = sa.VMISIndex.from_sessions(off, items, ts, 500, 20, 1.0)
    oix = O.OracleIndex(off, items, ts, 500, 20, 1.0)
    order = popularity_order(items)
    gix.set_fallback_popular(256)
    yield gix, oix, order
    gix.close()


@pytest.mark.parametrize("exclude_seen", [False, True])
def test_recommend_batch_fills_short_rows(sparse, exclude_seen):
    from serenade_amd.serving import DeviceSessionStore, fill_rows, filter_rows
    gix, oix, order = sparse
    ranking = [int(x) for x in order[:256]]
    store = DeviceSessionStore(gix, capacity=2048, items_cap=12, ttl_secs=1800, idle_secs=1200, history=H)
    twin = DeviceSessionStore(gix, capacity=2048, items_cap=12, ttl_secs=1800, idle_secs=1200, history=H)
    model = Model(H)
    total = short = in_window = 0
    try:
        for c, (now, reqs) in enumerate(calls(order)):
            entry = "device" if c % 2 else "host"
            seen = [model.serve(key_of(v), item, con, now, MAX_ITEMS) for v, item, con in reqs]
            windows, sessions = [w for w, _ in seen], [s for _, s in seen]
            got = run(gix, store, reqs, now, entry, exclude_seen, True)
            ref = run(gix, twin, reqs, now, entry, exclude_seen, False)
            wide = HOW_MANY + (H if exclude_seen else 0)
            rows = OracleRows(oix, sessions).rows(wide)
            unfilled = filter_rows(*rows, windows, HOW_MANY) if exclude_seen else tuple(a.copy() for a in rows)
            check_rows(ref, unfilled, "call %d without the flag" % c)
            want = fill_rows(*unfilled, sessions, ranking, HOW_MANY, excl=windows if exclude_seen else None)
            check_rows(got, want, "call %d, exclude_seen %s" % (c, exclude_seen))
            total += len(reqs)
            short += int((unfilled[2] < HOW_MANY).sum())
            for q in range(len(reqs)):
                row = set(int(x) for x in got[0][q, :got[2][q]])
                assert sessions[q][-1] not in row
                if exclude_seen:
                    assert not row & set(windows[q]), "request %d of call %d: an item of the window came back" % (q, c)
                else:
                    in_window += bool(row & set(windows[q]))
            assert (got[2] == HOW_MANY).all(), "a ranking of 256 fills every row"
            # the store's content is that of the same call without the flag
            a, b = store.last_batch_sessions(), twin.last_batch_sessions()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
            for v in range(300):
                assert store.get_session_items(key_of(v), now=now) == twin.get_session_items(key_of(v), now=now) == model.get(key_of(v), now), (c, v)
    finally:
        store.close()
        twin.close()
    print("exclude_seen %s: %d of %d rows were short; %d rows hold an item of their window" % (exclude_seen, short, total, in_window))
    assert total == 2000 and short >= 500
    if not exclude_seen:
        assert in_window > 0, "without the flag an earlier click that is in the ranking may come back"


def test_recommend_batch_without_a_ranking(sparse):
    import serenade_amd as sa
    from serenade_amd import capi
    from serenade_amd.serving import DeviceSessionStore
    gix, oix, order = sparse
    store = DeviceSessionStore(gix, capacity=1024, items_cap=12, history=H)
    now, reqs = calls(order)[0]
    gix.clear_fallback()
    try:
        for entry in ("host", "device"):
            with pytest.raises(sa.SerenadeError) as e:
                run(gix, store, reqs, now, entry, True, True)
            assert e.value.code == capi.SRN_ESTATE
        assert store.count(now).occupied == 0, "a refused call changed the store"
    finally:
        gix.set_fallback_popular(256)
        store.close()


RAW = ("n_evaluations", "mrr", "ndcg", "hit_rate", "popularity", "precision", "coverage", "recall", "f1score", "sum_mrr", "sum_ndcg", "sum_hit_rate",
       "sum_popularity", "sum_precision", "sum_recall", "covered_items", "unique_training_items")


def evaluate_raw(es, trials):
    from serenade_amd import capi, evaluation
    arr = (capi.EvalTrial * len(trials))(*[evaluation._trial(t) for t in trials])
    res = (capi.EvalResult * len(trials))()
    capi.check(capi.lib().srn_evaluate(es._h, arr, len(trials), res, None))
    return [tuple(getattr(r, f) for f in RAW) for r in res]


@pytest.mark.parametrize("business", [False, True])
def test_evaluate_scores_the_filled_rows(tmp_path, business):
    import serenade_amd as sa
    from serenade_amd import capi, evaluation
    d = extract_example(tmp_path)
    train, test = os.path.join(d, "train.txt"), os.path.join(d, "test.txt")
    index = sa.VMISIndex.new_from_csv(train, 500, 1.0)
    es = evaluation.EvalSet.from_tsv(index, test, train)
    try:
        trial = dict(k=50, m=500, max_items_in_session=2, how_many=20, length=20, business_logic=business)
        with pytest.raises(sa.SerenadeError) as e:
            evaluation.evaluate(es, [dict(trial, fill=True)])
        assert e.value.code == capi.SRN_ESTATE
        index.set_fallback_popular(256)
        filled, plain = evaluation.evaluate(es, [dict(trial, fill=True), trial])
        qs = evaluator_queries(read_test_data_evolving(test), 2)
        flat, off = flatten([q for q, _ in qs])
        ids, sc, cnt = sa.predict_batch(index, sa.CSR(flat, off), 50, 500, 20, business, fill=True)
        n_filled = int(np.isneginf(sc).any(axis=1).sum())
        print("business %s: %d of %d rows were short" % (business, n_filled, len(qs)))
        assert n_filled > 0
        with open(train) as f:
            next(f)
            train_items = [int(line.split()[1]) for line in f if len(line.split()) >= 3]
        host = eight_metrics([ids[q, :cnt[q]].tolist() for q in range(len(qs))], [n for _, n in qs], train_items, 20)
        for name in evaluation.METRICS:
            assert abs(filled[name + "@20"] - host[name]) <= 1e-12 * abs(host[name]), (name, filled[name + "@20"], host[name])
        assert filled["qty_evaluations"] == plain["qty_evaluations"] == len(qs)
        assert filled["HitRate@20"] >= plain["HitRate@20"]
        assert any(filled[name + "@20"] != plain[name + "@20"] for name in evaluation.METRICS), "the filled rows score like the unfilled ones"
        whole = evaluate_raw(es, [dict(trial, fill=True)])
        assert evaluate_raw(es, [dict(trial, fill=True, max_chunk_queries=256)]) == whole
        assert evaluate_raw(es, [dict(trial, fill=True, max_chunk_queries=512), trial])[0] == whole[0]
    finally:
        es.close()
        index.close()
