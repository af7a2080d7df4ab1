"""A click log on the GPU: srn_events_split / srn_events_take against prepare.split_model bit for bit, read_events against a Python parse and the loader, EvalSet.from_events
against EvalSet.from_tsv on files holding the same rows, and backtest against the same folds done by hand through files."""
import ctypes as C
import os

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, prepare
from serenade_amd.evaluation import EvalSet, evaluate
from serenade_amd.ingest import TrainingSessions
from serenade_amd.prepare import split_events, split_model
from helpers import extract_example

import prepare_cases as pc

pytestmark = pytest.mark.gpu

KNOBS = ("SRN_SPLIT_HASH_BITS", "SRN_INGEST_CHUNK_BYTES")
U64 = (1 << 64) - 1


@pytest.fixture
def knobs():
    saved = {k: os.environ.get(k) for k in KNOBS}

    def set_knobs(**kw):
        for k, v in kw.items():
            os.environ[k] = str(v)
        capi.reload_knobs()
    yield set_knobs
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    capi.reload_knobs()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _host(x):
    x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return x.view(np.uint64) if x.dtype == np.int64 else x


def _with_the_empty_key(log):
    """One session and one item of the log get the id 2^64 - 1, the tables' own empty mark."""
    s, i, t = (a.copy() for a in log)
    s[s == s[0]] = np.uint64(U64)
    i[i == i[1]] = np.uint64(U64)
    return s, i, t


def _cases():
    hand, rnd = pc.hand(), pc.random_log(11)
    big = pc.random_log(15, n=65537, n_sessions=3000, n_items=4000)
    out = [("hand", hand, pc.HAND_RULE), ("hand_f64", pc.hand_f64(), pc.HAND_RULE),
           ("random", rnd, pc.rule_for(None)), ("random_f64", pc.random_log(12, f64=True), pc.rule_for(None)),
           ("ids_above_2_32", pc.random_log(13, id_base=(1 << 32) + 99), pc.rule_for(None)), ("ids_above_2_63", pc.random_log(14, id_base=(1 << 63) + 12345), pc.rule_for(None)),
           ("the_empty_key", _with_the_empty_key(rnd), pc.rule_for(None)),
           ("n_1", tuple(a[:1] for a in rnd), dict(cutoff=1, min_item_support=1, min_session_len=1, test_known_items=False)),
           ("n_257", tuple(a[:257] for a in rnd), pc.rule_for(None, min_item_support=2)),
           ("n_65537", big, pc.rule_for(None)),
           ("all_out", rnd, dict(cutoff=pc.T0 + 10 * pc.DAY, start=pc.T0 + 9 * pc.DAY)),
           ("all_train", rnd, dict(cutoff=pc.T0 + 10 * pc.DAY, min_item_support=1, min_session_len=1)),
           ("all_test", rnd, dict(cutoff=1, min_item_support=1, min_session_len=1, test_known_items=False)),
           ("S_1_L_1", rnd, pc.rule_for(None, min_item_support=1, min_session_len=1)),
           ("flag_off", rnd, pc.rule_for(None, test_known_items=False)),
           ("no_window", rnd, pc.rule_for(None, start=0, end=0))]
    return out


CASES = _cases()
_MODEL = {}


def _model(name):
    if name not in _MODEL:   # computed once, shared by the forms and knob settings of a case
        _, log, rule = next(c for c in CASES if c[0] == name)
        _MODEL[name] = split_model(*log, **rule)
    return _MODEL[name]


def _check_split(name, log, rule, on_device):
    code, pos, info = _model(name)
    sp = split_events(*(tuple(_dev(a) for a in log) if on_device else log), **rule)
    got_code, got_pos = _host(sp.code), _host(sp.pos)
    assert got_code.dtype == np.uint8 and got_pos.dtype == np.uint32
    assert np.array_equal(got_code, code), name
    assert np.array_equal(got_pos, pos), name
    assert sp.info == info, name
    for side, which in ((sp.train, 1), (sp.test, 2)):
        keep = code == which
        for got, col in zip(side, log):
            got = _host(got)
            want = col[keep]
            assert got.dtype.itemsize == 8 and np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), name   # the 8 bytes as given: f64 stays f64
    return sp


@pytest.mark.parametrize("on_device", [False, True], ids=["host_arrays", "device_tensors"])
@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_split_and_take_equal_the_model(name, on_device):
    _, log, rule = next(c for c in CASES if c[0] == name)
    _check_split(name, log, rule, on_device)


def test_the_cases_cover_what_they_are_named_for():
    assert _model("hand")[0].tolist() == pc.HAND_CODES and _model("hand_f64")[0].tolist() == pc.HAND_CODES
    for name in ("random_f64", "ids_above_2_32"):
        assert all(_model(name)[2][k] > 0 for k in _model(name)[2] if k.startswith("dropped_")), name
    assert (_model("all_out")[0] == 16).all() and (_model("all_train")[0] == 1).all() and (_model("all_test")[0] == 2).all()
    big = _model("n_65537")[2]
    assert big["train_rows"] > 20000 and big["test_rows"] > 5000 and big["dropped_rare"] > 1000 and big["dropped_unknown"] > 1000
    log = next(c for c in CASES if c[0] == "the_empty_key")[1]
    assert (log[0] == np.uint64(U64)).any() and (log[1] == np.uint64(U64)).any()


@pytest.mark.parametrize("on_device", [False, True], ids=["host_arrays", "device_tensors"])
def test_long_probe_chains_change_nothing(knobs, on_device):
    knobs(SRN_SPLIT_HASH_BITS=4)     # 16 homes for every key of both tables: every probe chain is long, and only the comparison of the keys keeps them apart
    for name, log, rule in CASES:
        _check_split(name, log, rule, on_device)


def test_two_runs_give_the_same_bytes():
    _, log, rule = next(c for c in CASES if c[0] == "n_65537")
    dev = tuple(_dev(a) for a in log)
    a, b = split_events(*dev, **rule), split_events(*dev, **rule)
    assert bytes(_host(a.code)) == bytes(_host(b.code)) and bytes(_host(a.pos)) == bytes(_host(b.pos)) and a.info == b.info


def test_refusals():
    import torch
    s, i, t = pc.hand()
    for log in ((s, i, t), tuple(_dev(a) for a in (s, i, t))):
        for kw in (dict(cutoff=0), dict(cutoff=100, start=100), dict(cutoff=100, end=100), dict(cutoff=100, end=7)):
            with pytest.raises(ValueError):
                split_events(*log, **kw)
    ds, di, dt = (_dev(a) for a in (s, i, t))
    with pytest.raises(ValueError):
        split_events(ds, di, dt, cutoff=100, device=1)                       # tensors of device 0 handed over as device 1's
    with pytest.raises(ValueError):
        split_events(ds, di, t, cutoff=100)                                  # some on the GPU, some not
    # the C ABI: null buffers, and device rows that are not device memory of that device -- refused before any kernel reads them
    L, n = capi.lib(), len(s)
    code, pos, info = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"), capi.SplitInfo()
    rule = capi.Split(100, 10, 200, 2, 2, 1, 0)
    flags = capi.EVENTS_DEVICE | capi.EVENTS_TIME_I64
    vp = lambda x: None if x is None else C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data)
    call = lambda a, b, c, device=0, code=code: L.srn_events_split(vp(a), vp(b), vp(c), n, flags, C.byref(rule), device, None, vp(code), vp(pos), C.byref(info))
    assert call(ds, di, dt) == capi.SRN_OK and info.train_rows == 5
    assert call(None, di, dt) == capi.SRN_EINVAL and call(ds, di, None) == capi.SRN_EINVAL and call(ds, di, dt, code=None) == capi.SRN_EINVAL
    assert call(ds, di, dt, device=1) == capi.SRN_EINVAL and b"device" in L.srn_last_error()
    assert call(s, di, dt) == capi.SRN_EINVAL and b"not device memory" in L.srn_last_error()   # a host array under SRN_EVENTS_DEVICE
    ix = sa.VMISIndex.from_sessions(np.array([0, 2, 4], np.uint64), np.array([1, 2, 2, 3], np.uint64), np.array([1, 2], np.uint32), 5, 5, 1.0, device=0)
    try:
        with pytest.raises(ValueError):
            EvalSet.from_events(ix, (ds, di, dt), i)                         # test rows on the GPU, training items not
        h = C.c_void_p()
        ev = lambda a, tr, n_test=n, n_train=n, fl=flags: L.srn_eval_set_from_events(ix._h, vp(a), vp(di), vp(dt), n_test, vp(tr), n_train, fl, None, C.byref(h))
        assert ev(None, di) == capi.SRN_EINVAL and ev(ds, None) == capi.SRN_EINVAL and ev(ds, di, fl=64) == capi.SRN_EINVAL
        assert ev(s, di) == capi.SRN_EINVAL and ev(ds, i) == capi.SRN_EINVAL                     # host arrays under SRN_EVENTS_DEVICE
        assert ev(ds, di, n_test=(1 << 32) - 1) == capi.SRN_ERANGE
    finally:
        ix.close()


# ---- reading a log ----
def test_read_events_equals_a_python_parse(tmp_path, knobs):
    knobs(SRN_INGEST_CHUNK_BYTES=300)
    rng = np.random.default_rng(21)
    lines, want = ["SessionId\tItemId\tTime"], []
    for k in range(90):
        s, i, t = int(rng.integers(1, 40)), int(rng.integers(1, 1 << 40)), 1_600_000_000 + int(rng.integers(0, 5000))
        if k % 10 == 3:
            lines.append("")                                                 # blank
        if k % 10 == 5:
            lines.append("x%d\tnot-an-item\t1.0" % k)                        # bad ids
        if k % 10 == 7:
            lines.append("%d\t%d\tabc" % (s, i))                             # a time the device hands to the host, which rejects it
        if k % 4 == 0:
            lines.append("%d\t%d\t %d" % (s, i, t)); want.append((s, i, t))  # leading blank: the host re-reads the line
        elif k % 4 == 1:
            lines.append("%d\t%d\t%d.5" % (s, i, t)); want.append((s, i, t + 1))
        elif k % 4 == 2:
            lines.append("%d\t%d\t.5e1" % (s, i)); want.append((s, i, 5))    # no digit before the point: the host's again
        else:
            lines.append("%d\t%d\t%d.25" % (s, i, t)); want.append((s, i, t))
    p = tmp_path / "log.tsv"
    p.write_text("\n".join(lines) + "\n")
    import torch
    got = sa.read_events(p)
    assert all(x.dtype == torch.int64 and x.is_cuda for x in got)
    assert np.array_equal(np.stack([x.cpu().numpy() for x in got], 1), np.array(want, np.int64))
    # and the sessions grouped from these rows are the loader's
    a = TrainingSessions.from_events(*got)
    b = TrainingSessions.from_tsv(p)
    try:
        assert all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays()))
    finally:
        a.close(); b.close()


def test_read_events_of_the_example_gives_the_loaders_sessions(tmp_path):
    d = extract_example(tmp_path)
    p = os.path.join(d, "train.txt")
    ev = sa.read_events(p)
    a, b = TrainingSessions.from_events(*ev), TrainingSessions.from_tsv(p)
    try:
        assert len(ev[0]) > 50000 and all(np.array_equal(x, y) for x, y in zip(a.arrays(), b.arrays()))
    finally:
        a.close(); b.close()


# ---- evaluation set and backtest ----
TRIALS = [dict(k=50, m=500, max_items_in_session=2), dict(k=100, m=500, max_items_in_session=5, how_many=21, length=10)]


def _same_reports(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in w:
            if key in ("ms_predict", "ms_eval"):
                continue
            if key == "bootstrap":
                assert g[key]["replicates"] == w[key]["replicates"] and g[key]["empty_replicates"] == w[key]["empty_replicates"]
                assert np.array_equal(g[key]["weights"], w[key]["weights"])
                assert all(np.array_equal(g[key]["sums"][n], w[key]["sums"][n]) for n in w[key]["sums"])
            else:
                assert g[key] == w[key], key                                 # == on floats: bit for bit (no nan in a report)


def _read_rows(path):
    rows = [ln.split("\t") for ln in open(path).read().splitlines()[1:] if ln]
    return np.array([int(r[0]) for r in rows], np.uint64), np.array([int(r[1]) for r in rows], np.uint64), np.array([float(r[2]) for r in rows], np.float64)


def _sets_agree(index, test_path, train_path):
    test, train = _read_rows(test_path), _read_rows(train_path)
    ref = EvalSet.from_tsv(index, test_path, train_path)
    try:
        want = evaluate(ref, TRIALS, bootstrap=8, seed=3)
    finally:
        ref.close()
    assert want[0]["qty_evaluations"] > 100 and want[0]["Mrr@20"] > 0
    for form in (lambda x: x, _dev):
        es = EvalSet.from_events(index, tuple(form(a) for a in test), form(train[1]))
        try:
            _same_reports(evaluate(es, TRIALS, bootstrap=8, seed=3), want)
        finally:
            es.close()
    # integer seconds give the same set
    es = EvalSet.from_events(index, (test[0], test[1], prepare.round_times(test[2]).astype(np.int64)), train[1])
    try:
        _same_reports(evaluate(es, TRIALS), [{k: v for k, v in w.items() if not k.endswith("_ci") and k != "bootstrap"} for w in want])
    finally:
        es.close()


def test_eval_set_from_events_on_the_reference_example(tmp_path):
    d = extract_example(tmp_path)
    train, test = os.path.join(d, "train.txt"), os.path.join(d, "test.txt")
    index = sa.VMISIndex.new_from_csv(train, 500, 1.0)
    try:
        _sets_agree(index, test, train)
    finally:
        index.close()


def test_eval_set_from_events_with_tied_times(tmp_path, knobs):
    s, i, t = pc.random_log(31, n=3600, n_sessions=600, n_items=80)
    code = split_model(s, i, t, **pc.rule_for(None))[0]
    assert 150 <= len(np.unique(s[code == 2])) <= 250
    ts = t[code == 2]
    assert len(np.unique(ts)) < len(ts)                                      # tied times, inside sessions too
    assert any(len(np.unique(ts[s[code == 2] == x])) < (s[code == 2] == x).sum() for x in np.unique(s[code == 2])[:50])
    train, test = tmp_path / "train.tsv", tmp_path / "test.tsv"
    prepare.write_tsv(train, s[code == 1], i[code == 1], t[code == 1])
    prepare.write_tsv(test, s[code == 2], i[code == 2], t[code == 2])
    index = sa.VMISIndex.new_from_csv(str(train), 500, 1.0)
    try:
        _sets_agree(index, str(test), str(train))
        knobs(SRN_SPLIT_HASH_BITS=4)                                         # the training items' counting table with 16 homes for every id
        _sets_agree(index, str(test), str(train))
    finally:
        index.close()


@pytest.mark.parametrize("on_device", [False, True], ids=["host_arrays", "device_tensors"])
def test_backtest_equals_the_folds_done_by_hand(tmp_path, on_device):
    s, i, t = pc.random_log(41, n=3000, n_sessions=450, n_items=60, f64=True)
    events = tuple(_dev(a) for a in (s, i, t)) if on_device else (s, i, t)
    trials = TRIALS[:1]
    got = sa.backtest(events, trials, 500, 1.0, folds=2, test_span=pc.DAY, min_item_support=3)
    t_max = int(prepare.round_times(t).max())
    assert [f["cutoff"] for f in got] == [t_max + 1 - 2 * pc.DAY, t_max + 1 - pc.DAY]
    secs = prepare.round_times(t)
    for f in got:
        c = f["cutoff"]
        assert f["start"] == 0 and f["end"] == c + pc.DAY
        code, _, info = split_model(s, i, t, cutoff=c, start=0, end=c + pc.DAY, min_item_support=3)
        assert f["info"] == info and info["train_rows"] > 300 and info["test_rows"] > 100
        train, test = tmp_path / ("train_%d.tsv" % c), tmp_path / ("test_%d.tsv" % c)
        prepare.write_tsv(train, s[code == 1], i[code == 1], secs[code == 1])
        prepare.write_tsv(test, s[code == 2], i[code == 2], secs[code == 2])
        index = sa.VMISIndex.new_from_csv(str(train), 500, 1.0)
        try:
            es = EvalSet.from_tsv(index, str(test), str(train))
            try:
                _same_reports(f["reports"], evaluate(es, trials))
            finally:
                es.close()
        finally:
            index.close()
    # a training window: the second fold trained on one day only
    one = sa.backtest(events, trials, 500, 1.0, cutoffs=[got[1]["cutoff"]], test_span=pc.DAY, train_span=pc.DAY, min_item_support=3)
    assert one[0]["start"] == got[1]["cutoff"] - pc.DAY and one[0]["info"] == split_model(s, i, t, cutoff=got[1]["cutoff"], start=one[0]["start"], end=one[0]["end"], min_item_support=3)[2]
    assert one[0]["info"]["train_rows"] < got[1]["info"]["train_rows"]
