"""The traffic split's rule on the host (srn_traffic_split_arms, serving.arms_model): the C statement against the NumPy one bit for bit, on keys
designed to sit on every threshold (arm_cases.py) and on 10^6 random ones; the arms' shares; stickiness; the argument checks that need no GPU."""
import ctypes as C

import numpy as np
import pytest

from serenade_amd import capi, serving
from serenade_amd.serving import arm_thresholds, arms_model, feedback_compare, replay, replay_plan, split_compare

import arm_cases as ac
from test_replay_host import REPLAY_700_25, flat
import harvest_cases as hc

SEED, N = 7, 10 ** 6
NAMES = ("srn_traffic_split_create", "srn_traffic_split_free", "srn_traffic_split_info", "srn_traffic_split_set_weights", "srn_traffic_split_arms",
         "srn_recommend_batch_split_device", "srn_recommend_batch_split", "srn_traffic_split_timing", "srn_traffic_split_last_ms")


@pytest.fixture(scope="module")
def random_keys():
    rng = np.random.default_rng(20261021)
    return rng.integers(0, 2 ** 64, N, dtype=np.uint64), rng.integers(0, 2 ** 64, N, dtype=np.uint64)


def host_arms(seed, weights, keys):
    hi, lo = (capi.as_u64(a) for a in keys)
    out = np.full(len(hi), 0xEE, np.uint8)
    capi.check(capi.lib().srn_traffic_split_arms(seed, capi.ptr(np.array(weights, np.uint32)), len(weights), capi.ptr(hi), capi.ptr(lo), len(hi), capi.ptr(out)))
    return out


def test_symbols_and_exports():
    L = capi.lib()
    assert all(n in capi.SYMBOLS and hasattr(L, n) for n in NAMES)
    import serenade_amd as sa
    assert all(hasattr(sa, n) for n in ("TrafficSplit", "recommend_batch_split", "arms_model", "split_compare"))
    assert C.sizeof(capi.Arm) == 32 and C.sizeof(capi.TrafficSplitInfo) == 8 + 3 * 8 + 2 * 16 * 8 + 16 and capi.MAX_ARMS == 16


def test_unmix64_round_trip_and_designed_draws():
    rng = np.random.default_rng(5)
    for x in [0, 1, ac.M64, 1 << 63] + rng.integers(0, 2 ** 64, 2000, dtype=np.uint64).tolist():
        assert ac.unmix64(ac.mix64(x)) == x and ac.mix64(ac.unmix64(x)) == x
    for hi in ac.HIS:
        for u in (0, 1, 2 ** 31, 2 ** 32 - 1):
            for low in (0, 12345, 2 ** 32 - 1):
                assert ac.draw(SEED, hi, ac.lo_for(SEED, hi, u, low)) == u
    # the NumPy statement of the draw against the Python-integer one
    hi, lo = rng.integers(0, 2 ** 64, 500, dtype=np.uint64), rng.integers(0, 2 ** 64, 500, dtype=np.uint64)
    assert serving.arm_draws(SEED, (hi, lo)).tolist() == [ac.draw(SEED, h, l) for h, l in zip(hi.tolist(), lo.tolist())]


@pytest.mark.parametrize("weights", ac.WEIGHT_SETS, ids=lambda w: "w%d_%d" % (len(w), w[0] % 97))
def test_host_rule_equals_model_on_designed_keys(weights):
    assert arm_thresholds(weights) == ac.thresholds(weights) and arm_thresholds(weights)[-1] == 2 ** 32
    keys, us, arm = ac.threshold_keys(SEED, weights)
    T = ac.thresholds(weights)[:-1]
    assert {0, 2 ** 32 - 1} <= set(us) and all(t in us for t in T if t < 2 ** 32) and all(t - 1 in us for t in T if t > 0)
    assert serving.arm_draws(SEED, keys).tolist() == us
    got = host_arms(SEED, weights, keys)
    assert got.tobytes() == arms_model(SEED, weights, keys).tobytes() == arm.tobytes()
    assert all(weights[a] > 0 for a in set(got.tolist()))                          # an arm of weight 0 holds nothing, not even a key on its threshold
    # keys equal in one half alone are different visitors: what they draw is their own
    assert len({(h, l) for h, l in zip(keys[0].tolist(), keys[1].tolist())}) == len(us)


@pytest.mark.parametrize("weights", ac.WEIGHT_SETS, ids=lambda w: "w%d_%d" % (len(w), w[0] % 97))
def test_host_rule_equals_model_and_shares_on_random_keys(random_keys, weights):
    got = host_arms(SEED, weights, random_keys)
    model = arms_model(SEED, weights, random_keys)
    assert got.tobytes() == model.tobytes()
    W = sum(weights)
    counts = np.bincount(got, minlength=len(weights))
    for a, w in enumerate(weights):
        p = w / W
        assert abs(int(counts[a]) - N * p) <= 5 * np.sqrt(N * p * (1 - p)), (a, int(counts[a]), N * p)
        if w == 0:
            assert counts[a] == 0
    # another seed moves about 1 - sum p_a^2 of the keys
    q = 1.0 - sum((w / W) ** 2 for w in weights)
    moved = int(np.count_nonzero(host_arms(SEED + 1, weights, random_keys) != got))
    assert abs(moved - N * q) <= 5 * np.sqrt(N * q * (1 - q)) + 0.5, (moved, N * q)


def test_a_key_keeps_its_arm_at_any_position_and_in_any_batch(random_keys):
    hi, lo = random_keys[0][:5000], random_keys[1][:5000]
    w = [3, 0, 2, 5]
    whole = host_arms(SEED, w, (hi, lo))
    perm = np.random.default_rng(9).permutation(5000)
    assert np.array_equal(host_arms(SEED, w, (hi[perm], lo[perm])), whole[perm])
    for a, b in ((0, 1), (17, 18), (100, 777), (4999, 5000)):
        assert np.array_equal(host_arms(SEED, w, (hi[a:b], lo[a:b])), whole[a:b])
    rep = np.repeat(np.arange(50), 7)
    assert np.array_equal(host_arms(SEED, w, (hi[rep], lo[rep])), whole[rep])
    # a ramp moves only the keys whose u lies between an old and a new threshold
    u = serving.arm_draws(SEED, (hi, lo))
    old_T, new_T = arm_thresholds([9, 1])[0], arm_thresholds([5, 5])[0]
    moved = host_arms(SEED, [9, 1], (hi, lo)) != host_arms(SEED, [5, 5], (hi, lo))
    assert np.array_equal(moved, (u >= np.uint64(new_T)) & (u < np.uint64(old_T))) and moved.any()


def test_rekey_prescribes_the_arms():
    steps = hc.make_stream()
    keys, _, _, _ = flat(steps)
    for weights, A in (([1, 1], 2), ([9, 1], 2), ([1, 2, 1], 3)):
        for name, seq in ac.sequences(len(keys[0]), A).items():
            hi, lo = ac.rekey(SEED, weights, keys, seq)
            assert np.array_equal(host_arms(SEED, weights, (hi, lo)), seq), (weights, name)


def test_errors_and_empty_calls():
    L, p = capi.lib(), capi.ptr
    hi = lo = np.arange(4, dtype=np.uint64)
    out = np.zeros(4, np.uint8)
    w = lambda *x: p(np.array(x, np.uint32))   # noqa: E731
    arms = lambda weights, n_arms, n=4, o=out: L.srn_traffic_split_arms(SEED, weights, n_arms, p(hi), p(lo), n, None if o is None else p(o))   # noqa: E731
    assert arms(w(1, 1), 2) == capi.SRN_OK
    assert arms(w(1, 1), 2, n=0, o=None) == capi.SRN_OK                            # n = 0 needs no arrays
    assert arms(w(1, 1), 2, o=None) == capi.SRN_EINVAL
    assert arms(None, 2) == capi.SRN_EINVAL
    assert arms(w(1), 0) == capi.SRN_ERANGE and arms(p(np.ones(17, np.uint32)), 17) == capi.SRN_ERANGE
    assert arms(w(0, 0), 2) == capi.SRN_EINVAL                                     # W = 0
    assert arms(w(2 ** 32 - 1, 1), 2) == capi.SRN_ERANGE                           # W = 2^32
    assert arms(w(2 ** 32 - 1), 1) == capi.SRN_OK and not out.any()                # W = 2^32 - 1, one arm
    # create refuses the same before it looks for a GPU; a NULL handle is refused everywhere
    h = C.c_void_p()
    create = lambda weights, n_arms, max_batch=64, max_how_many=21: L.srn_traffic_split_create(0, weights, n_arms, SEED, max_batch, max_how_many, C.byref(h))   # noqa: E731
    assert create(w(1), 0) == capi.SRN_ERANGE and create(p(np.ones(17, np.uint32)), 17) == capi.SRN_ERANGE
    assert create(w(0, 0), 2) == capi.SRN_EINVAL and create(w(2 ** 31, 2 ** 31), 2) == capi.SRN_ERANGE
    assert create(w(1, 1), 2, max_batch=0) == capi.SRN_EINVAL and create(w(1, 1), 2, max_how_many=0) == capi.SRN_EINVAL
    assert create(w(1, 1), 2, max_batch=2 ** 24 + 1) == capi.SRN_ERANGE and create(w(1, 1), 2, max_how_many=513) == capi.SRN_ERANGE
    assert L.srn_traffic_split_create(0, w(1, 1), 2, SEED, 64, 21, None) == capi.SRN_EINVAL
    assert h.value is None
    info = capi.TrafficSplitInfo()
    assert L.srn_traffic_split_info(None, C.byref(info)) == capi.SRN_EINVAL and L.srn_traffic_split_set_weights(None, w(1, 1), 2) == capi.SRN_EINVAL
    assert L.srn_traffic_split_free(None) == capi.SRN_OK
    arm = (capi.Arm * 2)()
    ids, sc, cnt = np.zeros((4, 21), np.uint64), np.zeros((4, 21)), np.zeros(4, np.uint32)
    assert L.srn_recommend_batch_split(None, arm, 2, None, p(hi), p(lo), p(hi), None, None, 4, 1, 21, p(ids), p(sc), p(cnt), None, None, None) == capi.SRN_EINVAL
    assert L.srn_recommend_batch_split_device(None, arm, 2, None, None, None, None, None, None, 0, 1, 21, None, None, None, None, None, None, None) == capi.SRN_EINVAL
    with pytest.raises(ValueError):
        arms_model(SEED, [0, 0], (hi, lo))
    with pytest.raises(ValueError):
        arms_model(SEED, [1] * 17, (hi, lo))
    with pytest.raises(ValueError):
        arm_thresholds([-1, 2])
    assert arms_model(SEED, [3], (hi, lo)).tolist() == [0] * 4 and arms_model(SEED, [1, 1], (hi[:0], lo[:0])).shape == (0,)


def _stats(observed, hist_model, seed=3):
    """a log's stats() with a bootstrap of 4 replicates, constructed"""
    B, R = 4, 3
    hm = np.array(hist_model, np.uint64).reshape(B, R)
    boot = {"replicates": B, "seed": seed, "observed": np.array(observed, np.uint64), "hist_model": hm, "hist_filled": np.zeros((B, R), np.uint64)}
    out = serving.feedback_metrics(hm.sum(axis=0), np.zeros(R, np.uint64), int(np.sum(observed)))
    return serving._with_feedback_bootstrap(out, boot, 0.9)


def test_split_compare_is_feedback_compare_against_the_baseline():
    stats = [_stats([10, 12, 9, 11], [0, 3, 1, 0, 4, 2, 0, 2, 2, 0, 5, 0]), _stats([5, 4, 6, 5], [0, 1, 1, 0, 2, 0, 0, 0, 3, 0, 1, 1]),
             _stats([7, 0, 8, 7], [0, 2, 2, 0, 0, 0, 0, 4, 0, 0, 1, 3])]
    for metric in ("mrr", "hit_rate"):
        for base in range(3):
            got = split_compare(stats, metric=metric, baseline=base)
            assert got[base] is None
            for a in range(3):
                if a != base:
                    assert got[a] == feedback_compare(stats[a], stats[base], metric)
    assert split_compare(stats, baseline=0)[2]["replicates"] == 3                  # the replicate in which arm 2 observed nothing is left out
    with pytest.raises(ValueError):
        split_compare(stats, baseline=3)
    with pytest.raises(ValueError):
        split_compare([stats[0], _stats([1, 1, 1, 1], [0] * 12, seed=4)])            # logs that do not share their replicates


def test_replay_plan_is_unaffected_and_replay_wants_split_and_arms_together():
    steps = hc.make_stream()
    _, items, _, times = flat(steps)
    plan = replay_plan(times, 700, 25)
    assert (len([c for c in plan if c[1] > c[0]]), sum(1 for c in plan if c[2] is not None)) == REPLAY_700_25
    assert replay_plan(times, 1 << 20) == [(0, len(items), None)]
    with pytest.raises(ValueError):
        replay(None, None, (times, times), items, times, k=1, m=1, how_many=1, split=object())
    with pytest.raises(ValueError):
        replay(None, None, (times, times), items, times, k=1, m=1, how_many=1, arms=[{}])
