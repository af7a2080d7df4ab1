"""The split of a click log without a GPU: prepare.split_model -- the rule of srn_split.hip in NumPy -- on cases worked by hand, its properties on
random logs, the refusals that need no device, the command line on the host model, and the new entry points in the built library."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from serenade_amd import capi, prepare
from serenade_amd.prepare import split_model

import prepare_cases as pc

NEW_SYMBOLS = ["srn_events_from_tsv_gpu", "srn_events_view", "srn_events_free", "srn_events_split", "srn_events_take", "srn_eval_set_from_events"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_bound_and_exported():
    L = capi.lib()
    for name in NEW_SYMBOLS:
        assert name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1] and fn.restype == capi.SYMBOLS[name][0], name
    assert C.sizeof(capi.Split) == 40 and C.sizeof(capi.SplitInfo) == 120 and C.sizeof(capi.EventsView) == 40
    import serenade_amd as sa
    assert sa.split_model is split_model and sa.split_events is prepare.split_events and sa.backtest is prepare.backtest and sa.read_events is prepare.read_events
    assert sa.Split is prepare.Split and callable(sa.EvalSet.from_events)
    assert (prepare.TRAIN, prepare.TEST, prepare.OUT, prepare.RARE, prepare.SHORT_TRAIN, prepare.UNKNOWN, prepare.SHORT_TEST) == (1, 2, 16, 17, 18, 19, 20)


def test_the_case_worked_by_hand():
    s, i, t = pc.hand()
    code, pos, info = split_model(s, i, t, **pc.HAND_RULE)
    assert code.dtype == np.uint8 and pos.dtype == np.uint32
    assert code.tolist() == pc.HAND_CODES
    assert pos[2:7].tolist() == [0, 1, 2, 3, 4] and pos[9:11].tolist() == [0, 1]
    assert (np.delete(pos, [2, 3, 4, 5, 6, 9, 10]) == pc.NO_POS).all()
    assert info == pc.HAND_INFO
    pc.check_properties(s, i, code, pos, pc.HAND_RULE)


def test_half_seconds_round_both_ways_and_negative_and_nan_read_as_zero():
    s, i, f = pc.hand_f64()
    r = prepare.round_times(f)
    assert r[0] == 0 and r[1] == 0 and np.array_equal(r[2:], pc.hand()[2][2:].astype(np.uint64))
    assert ((f[2:] - np.floor(f[2:])) == 0.5).any() and ((f[2:] - np.floor(f[2:])) == 0.25).any()
    code, pos, info = split_model(s, i, f, **pc.HAND_RULE)
    assert code.tolist() == pc.HAND_CODES
    assert info == dict(pc.HAND_INFO, t_min=0)
    assert prepare.round_times(np.array([0.49999, 0.5, 1.5, 2.4999, -0.5, 7.0])).tolist() == [0, 1, 2, 2, 0, 7]
    assert prepare.round_times(np.array([-5, 0, 9], np.int64)).tolist() == [0, 0, 9]


def test_other_small_cases():
    s, i, t = pc.hand()
    # the flag off: E and D stay; sessions 6 and 8 keep both rows
    code, pos, info = split_model(s, i, t, **dict(pc.HAND_RULE, test_known_items=False))
    assert code.tolist() == [16, 16, 1, 1, 1, 1, 1, 18, 17, 2, 2, 2, 2, 16, 16, 2, 2]
    assert pos[[9, 10, 11, 12, 15, 16]].tolist() == [0, 1, 2, 3, 4, 5] and info["test_sessions"] == 3 and info["test_items"] == 5 and info["dropped_unknown"] == 0
    # S = 1 and L = 1 drop nothing on the train side; no window: sessions 1 and 7 come in
    code, _, info = split_model(s, i, t, cutoff=100, min_item_support=1, min_session_len=1)
    assert code.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 19, 2, 2, 2, 2]
    assert info["train_rows"] == 9 and info["train_sessions"] == 4 and info["dropped_unknown"] == 1 and info["dropped_out"] == 0
    # 0 reads as 1
    assert np.array_equal(split_model(s, i, t, cutoff=100, min_item_support=0, min_session_len=0)[0], code)
    # all OUT, all train, all test
    assert (split_model(s, i, t, cutoff=1000, start=999)[0] == 16).all()
    assert set(split_model(s, i, t, cutoff=1000, min_item_support=1, min_session_len=1)[0].tolist()) == {1}
    assert set(split_model(s, i, t, cutoff=1, min_item_support=1, min_session_len=1, test_known_items=False)[0].tolist()) == {2}
    # one pass, no fixed point: dropping the short session 4 leaves C with one TRAIN row although S = 2
    code = split_model(s, i, t, **pc.HAND_RULE)[0]
    assert int(((i == pc.C_) & (code == 1)).sum()) == 1
    # a test session's early rows may lie before the cutoff (row 9, time 90)
    assert code[9] == 2 and t[9] < 100


@pytest.mark.parametrize("seed,f64", [(1, False), (2, True), (3, False)])
def test_properties_on_random_logs(seed, f64):
    s, i, t = pc.random_log(seed, f64=f64, id_base=(1 << 63) + 12345 if seed == 3 else 0)
    for rule in (pc.rule_for(t), pc.rule_for(t, test_known_items=False, start=0, end=0), pc.rule_for(t, min_item_support=1, min_session_len=1)):
        code, pos, info = split_model(s, i, t, **rule)
        pc.check_properties(s, i, code, pos, rule)
        assert info["train_rows"] + info["test_rows"] + sum(info[k] for k in info if k.startswith("dropped_")) == len(s)
        assert info["train_rows"] > 100 and info["test_rows"] > 50
        assert info["sessions"] == len(np.unique(s)) and info["items"] == len(np.unique(i))
    code, _, info = split_model(s, i, t, **pc.rule_for(t))
    assert all(info[k] > 0 for k in info if k.startswith("dropped_")), info     # every drop code occurs in these logs


def test_the_model_refuses():
    s, i, t = pc.hand()
    for kw in (dict(cutoff=0), dict(cutoff=100, start=100), dict(cutoff=100, start=150), dict(cutoff=100, end=100), dict(cutoff=100, end=50), dict(cutoff=-5)):
        with pytest.raises(ValueError):
            split_model(s, i, t, **kw)
    with pytest.raises(ValueError):
        split_model(s[:0], i[:0], t[:0], cutoff=100)
    with pytest.raises(ValueError):
        split_model(s, i[:-1], t, cutoff=100)


def test_the_library_refuses_before_it_needs_a_device():
    s, i, t = pc.hand()
    n = len(s)
    code, pos, info = np.zeros(n, np.uint8), np.zeros(n, np.uint32), capi.SplitInfo()
    L = capi.lib()

    def split(rule, n=n, flags=capi.EVENTS_TIME_I64, device=0, sess=s, code=code, info=info):
        return L.srn_events_split(capi.ptr(sess), capi.ptr(i), capi.ptr(t), n, flags, None if rule is None else C.byref(rule), device, None, capi.ptr(code), capi.ptr(pos),
                                  None if info is None else C.byref(info))
    ok = (100, 10, 200, 2, 2, 1, 0)
    assert split(capi.Split(0, 0, 0, 2, 2, 1, 0)) == capi.SRN_EINVAL and b"cutoff" in L.srn_last_error()
    assert split(capi.Split(100, 100, 0, 2, 2, 1, 0)) == capi.SRN_EINVAL
    assert split(capi.Split(100, 0, 100, 2, 2, 1, 0)) == capi.SRN_EINVAL
    assert split(capi.Split(100, 0, 0, 2, 2, 2, 0)) == capi.SRN_EINVAL          # an unknown split flag
    assert split(capi.Split(100, 0, 0, 2, 2, 1, 7)) == capi.SRN_EINVAL          # reserved
    assert split(capi.Split(*ok), flags=8) == capi.SRN_EINVAL
    assert split(capi.Split(*ok), n=0) == capi.SRN_EINVAL
    assert split(None) == capi.SRN_EINVAL
    assert split(capi.Split(*ok), sess=None) == capi.SRN_EINVAL and split(capi.Split(*ok), code=None) == capi.SRN_EINVAL and split(capi.Split(*ok), info=None) == capi.SRN_EINVAL
    assert split(capi.Split(*ok), n=(1 << 32) - 1) == capi.SRN_ERANGE
    assert split(capi.Split(*ok), device=-1) == capi.SRN_ENODEV

    def take(which=1, n=n, device=0, out=s, flags=capi.EVENTS_TIME_I64):
        return L.srn_events_take(capi.ptr(code), capi.ptr(pos), n, which, capi.ptr(s), capi.ptr(i), capi.ptr(t), flags, capi.ptr(out), capi.ptr(i), capi.ptr(t), device, None)
    assert take(which=3) == capi.SRN_EINVAL and take(which=16) == capi.SRN_EINVAL and take(n=0) == capi.SRN_EINVAL and take(out=None) == capi.SRN_EINVAL
    assert take(n=(1 << 32) - 1) == capi.SRN_ERANGE and take(device=-1) == capi.SRN_ENODEV and take(flags=4) == capi.SRN_EINVAL
    h = C.c_void_p()
    assert L.srn_events_from_tsv_gpu(b"/nonexistent", -1, C.byref(h)) == capi.SRN_ENODEV and L.srn_events_from_tsv_gpu(None, 0, C.byref(h)) == capi.SRN_EINVAL
    assert L.srn_events_view(None, C.byref(capi.EventsView())) == capi.SRN_EINVAL
    L.srn_events_free(None)
    assert L.srn_eval_set_from_events(None, None, None, None, 0, None, 0, 0, None, C.byref(h)) == capi.SRN_EINVAL


def test_take_on_host_arrays_is_the_stable_compaction():
    s, i, t = pc.random_log(5, n=500, n_sessions=80, n_items=30)
    code, pos, _ = split_model(s, i, t, **pc.rule_for(t))
    f = t.astype(np.float64) - 0.5
    for which in (1, 2):
        m = int((code == which).sum())
        for times, flags in ((t, capi.EVENTS_TIME_I64), (f, 0)):
            os_, oi, ot = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, times.dtype)
            capi.check(capi.lib().srn_events_take(capi.ptr(code), capi.ptr(pos), len(s), which, capi.ptr(s), capi.ptr(i), capi.ptr(times), flags, capi.ptr(os_), capi.ptr(oi),
                                                  capi.ptr(ot), 0, None))
            assert np.array_equal(os_, s[code == which]) and np.array_equal(oi, i[code == which]) and np.array_equal(ot, times[code == which])


def test_the_command_line_round_trip(tmp_path):
    s, i, f = pc.random_log(7, n=600, n_sessions=90, n_items=30, f64=True)
    rule = pc.rule_for(f)
    log = tmp_path / "log.tsv"
    with open(log, "w") as out:
        out.write("SessionId\tItemId\tTime\n")
        for k in range(len(s)):
            if k == 100:
                out.write("\nnot a row\t1\t2\n12\tx\t3\n")
            out.write("%d\t%d\t%.1f\n" % (s[k], i[k], f[k]))
    a, b = tmp_path / "train.tsv", tmp_path / "test.tsv"
    r = subprocess.run([sys.executable, "-m", "serenade_amd.prepare", str(log), "--cutoff", str(rule["cutoff"]), "--start", str(rule["start"]), "--end", str(rule["end"]),
                        "--min-item-support", "5", "--min-session-len", "2", "--device", "-1", "--train-out", str(a), "--test-out", str(b)],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "RuntimeWarning" not in r.stderr, r.stderr
    code, _, info = split_model(s, i, f, **rule)
    assert json.loads(r.stdout.strip().splitlines()[-1]) == info
    secs = prepare.round_times(f)
    for path, which in ((a, 1), (b, 2)):
        lines = open(path).read().splitlines()
        assert lines[0] == "SessionId\tItemId\tTime"
        got = np.array([[int(x) for x in ln.split("\t")] for ln in lines[1:]], np.uint64).reshape(-1, 3)
        assert np.array_equal(got[:, 0], s[code == which]) and np.array_equal(got[:, 1], i[code == which]) and np.array_equal(got[:, 2], secs[code == which])
    # and in process, with unknown items kept
    assert prepare.main([str(log), "--cutoff", str(rule["cutoff"]), "--keep-unknown-items", "--device", "-1", "--train-out", str(a), "--test-out", str(b)]) == 0
    code2 = split_model(s, i, f, cutoff=rule["cutoff"], test_known_items=False)[0]
    assert len(open(b).read().splitlines()) - 1 == int((code2 == 2).sum()) > 0
