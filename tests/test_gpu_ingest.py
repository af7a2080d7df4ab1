"""The GPU loader (srn_ingest.hip) against the host loader: every comparison reads off, items and ts through srn_sessions_view and
checks them bit for bit against srn_sessions_from_tsv (and, where the file is plain, against the oracle's read_tsv)."""
import os

import numpy as np
import pytest

import serenade_amd as sa
from serenade_amd import capi, synth
from serenade_amd.ingest import TrainingSessions
from helpers import extract_example
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HEADER = "SessionId\tItemId\tTime\n"


def _write(path, text, mode="w"):
    with open(path, "wb" if isinstance(text, bytes) else mode) as f:
        f.write(text)
    return str(path)


def _load(path, loader):
    s = TrainingSessions.from_tsv(path, loader=loader, device=0)
    try:
        return s.arrays(), s.length_quantile(0.995), s.load_info()
    finally:
        s.close()


def _same(path, oracle=False):
    (ho, hi, ht), hq, _ = _load(path, "host")
    (go, gi, gt), gq, info = _load(path, "gpu")
    assert go.dtype == ho.dtype and gi.dtype == hi.dtype and gt.dtype == ht.dtype
    assert np.array_equal(go, ho) and np.array_equal(gi, hi) and np.array_equal(gt, ht), path
    assert gq == hq
    if oracle:
        oo, oi, ot, _ = O.read_tsv(str(path))
        assert np.array_equal(go, oo) and np.array_equal(gi, oi) and np.array_equal(gt, ot)
    return (go, gi, gt), info


def _both_fail(path):
    codes = []
    for loader in ("host", "gpu"):
        with pytest.raises(capi.SerenadeError) as e:
            TrainingSessions.from_tsv(path, loader=loader, device=0)
        codes.append(e.value.code)
    assert codes[0] == codes[1] == capi.SRN_EINVAL


def test_reference_example(tmp_path):
    path = os.path.join(extract_example(tmp_path), "train.txt")
    (off, _, _), info = _same(path, oracle=True)
    assert len(off) - 1 == 23753
    s = TrainingSessions.from_tsv(path, loader="gpu")
    assert s.length_quantile(0.995) == 15
    s.close()
    assert info["rows"] + info["skipped"] == info["lines"] and info["skipped"] >= 1 and info["host_parsed"] == 0
    assert info["ms_group"] > 0 and info["ms_read"] > 0


QUIRKS = {
    # the host test's hand-made cases (test_tsv_loader_matches_read_from_file_quirks)
    "final_row_dropped": [(7, 30, "10.4"), (9, 5, "20.0"), (7, 10, "11.6"), (7, 30, "99.0"), (9, 6, "21.0"), (9, 8, "22.0")],
    "trailing_single_row_session": [(7, 30, "10.0"), (7, 10, "11.0"), (9, 5, "20.0")],
    "duplicates_later_larger_times": [(1, 5, "10"), (1, 6, "11"), (1, 5, "900"), (1, 6, "901"), (2, 5, "3"), (2, 5, "1e9"), (2, 7, "4"), (3, 1, "1")],
    "half_times_both_signs": [(1, 1, "0.5"), (1, 2, "1.5"), (2, 1, "-0.5"), (2, 2, "-1.5"), (2, 3, "2.5"), (3, 1, "-0"), (3, 2, "4.4999999999999999"),
                              (3, 3, "0.49999999999999994"), (4, 1, "1.5e1"), (4, 2, "25E-1"), (4, 3, "+7.5"), (5, 1, "1")],
    "u64_wrap": [(18446744073709551615, 1, "1"), (18446744073709551616, 2, "2"), (99999999999999999999999, 3, "3"), (5, 18446744073709551617, "4"),
                 (5, 1, "5"), (6, 6, "6")],
    "one_session": [(42, i % 7, "%d.5" % i) for i in range(40)],
    "one_row": [(1, 2, "3.5")],
    "two_rows": [(1, 2, "3.5"), (1, 3, "4.5")],
    "two_rows_two_sessions": [(2, 2, "3.5"), (1, 3, "4.5")],
}


@pytest.mark.parametrize("name", sorted(QUIRKS))
def test_quirk_files(tmp_path, name):
    path = _write(tmp_path / "q.tsv", HEADER + "".join("%d\t%d\t%s\n" % r for r in QUIRKS[name]))
    # (the oracle's restatement neither wraps ids past 2^64 nor clamps negative times to 0 as the host loader does)
    (off, items, ts), info = _same(path, oracle=name not in ("u64_wrap", "half_times_both_signs"))
    if name == "one_row":
        assert len(off) == 1 and info["rows"] == 1
    if name == "final_row_dropped":
        assert off.tolist() == [0, 2, 4] and items.tolist() == [10, 30, 5, 6] and ts.tolist() == [12, 21]


def test_line_structure(tmp_path):
    """CRLF endings, blank lines, a missing final newline, unparsable rows, a fourth column, a header that parses, NUL bytes."""
    body = (b"1\t2\t3\n"                                   # the first line is the header whatever it holds
            b"1\t5\t10.5\r\n" b"\n" b"1\t6\t11\r\n" b"\r\n" b"2\t5\t12 \r\n" b"2\t6\t13\t4th column\n" b"3\t7\t14\t\n"
            b"x\t1\t1\n" b"1\tx\t1\n" b"1\t1\n" b"1\t1\t\n" b"1 \t1\t1\n" b"\t1\t1\n" b"1\t\t1\n" b"1\t1\t1x\n" b"1\t1\t1.5e\n" b"1\t1\t5.\n"
            b"4\t1\t15\x00junk\n" b"4\t2\t16\n" b"5\t1\t17")
    path = _write(tmp_path / "l.tsv", body)
    (_, _, _), info = _same(path)
    assert info["lines"] == body.count(b"\n") + 1
    _, info2 = _same(_write(tmp_path / "l2.tsv", body + b"\n"))
    assert info2["lines"] == info["lines"]


def test_empty_and_header_only_files_fail_like_the_host(tmp_path):
    _both_fail(_write(tmp_path / "e.tsv", ""))
    _both_fail(_write(tmp_path / "h.tsv", HEADER))
    _both_fail(_write(tmp_path / "b.tsv", HEADER + "x\ty\tz\n\n"))


def test_host_fallback(tmp_path):
    # (times that would round to >= 2^63, where the host's llround is undefined, are out of scope)
    rows = [(1, 1, "0x1p30"), (1, 2, "nan"), (1, 3, "1234567890123456789012345"), (2, 1, "  17.5"), (2, 2, "-nan"), (2, 3, "\t5"), (3, 1, "1e18"),
            (3, 2, "0x10"), (3, 3, ".5"), (4, 1, "5."), (4, 2, "1" + "0" * 10 + " " * 60), (4, 3, "1.5" + " " * 70 + "x"), (5, 1, "2" + " " * 62 + "junk"),
            (5, 2, "1e-400"), (5, 3, "12345678901234567.5"), (6, 1, "0.0000000000000000000000015e25"), (6, 2, "1.5x"), (6, 3, "7"), (7, 1, "8")]
    path = _write(tmp_path / "f.tsv", HEADER + "".join("%d\t%d\t%s\n" % r for r in rows))
    _, info = _same(path)
    assert info["host_parsed"] > 0 and info["rows"] < len(rows)


def test_chunk_boundaries(tmp_path, monkeypatch):
    rng = np.random.default_rng(11)
    lines = []
    for j in range(3000):
        t = "%d.%d" % (rng.integers(0, 10 ** 9), rng.integers(0, 10))
        lines.append("%d\t%d\t%s%s\n" % (rng.integers(0, 300), rng.integers(0, 50), t, "\r" if j % 7 == 0 else ""))
        if j % 500 == 3:
            lines.append("%d\t%d\t%s\t%s\n" % (rng.integers(0, 300), rng.integers(0, 50), t, "y" * 700))   # longer than a chunk
    path = _write(tmp_path / "c.tsv", HEADER + "".join(lines))
    ref, _ = _same(path)
    monkeypatch.setenv("SRN_INGEST_CHUNK_BYTES", "256")
    capi.reload_knobs()
    try:
        got, info = _same(path)
    finally:
        monkeypatch.delenv("SRN_INGEST_CHUNK_BYTES")
        capi.reload_knobs()
    assert all(np.array_equal(a, b) for a, b in zip(ref, got))
    assert info["lines"] == len(lines) + 1


TIME_FORMS = ["%d", "%d.5", "%d.0", "-%d.5", "%de0", "%d.25", "0x%x", " %d", "%d.5000000000000000000001", "nan", "%d\r", "%d  "]


@pytest.mark.parametrize("seed", range(6))
def test_seeded_random_files(tmp_path, seed, monkeypatch):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(1, 4000))
    n_sess = int(rng.integers(1, 60))
    out = [HEADER if rng.random() < 0.8 else "1\t2\t3\n"]
    for _ in range(n):
        r = rng.random()
        if r < 0.03:
            out.append(["\n", "garbage\n", "1\t\n", "\r\n", "1\t2\n"][int(rng.integers(0, 5))])
            continue
        s = int(rng.integers(0, n_sess)) if rng.random() < 0.97 else int(rng.integers(0, 2 ** 63))
        it = int(rng.integers(0, 30))
        form = TIME_FORMS[int(rng.integers(0, len(TIME_FORMS)))] if rng.random() < 0.2 else "%d.5"
        v = int(rng.integers(0, 2 ** 31))
        t = form % v if "%" in form else form
        extra = "\tx" if rng.random() < 0.02 else ""
        out.append("%d\t%d\t%s%s%s" % (s, it, t, extra, "\r\n" if rng.random() < 0.1 else "\n"))
    text = "".join(out)
    if rng.random() < 0.3:
        text = text.rstrip("\n")
    path = _write(tmp_path / "r.tsv", text)
    if seed % 2:
        monkeypatch.setenv("SRN_INGEST_CHUNK_BYTES", str(int(rng.integers(64, 2048))))
        capi.reload_knobs()
    try:
        ok = True
        try:
            TrainingSessions.from_tsv(path, loader="host").close()
        except capi.SerenadeError:
            ok = False
        if ok:
            _same(path)
        else:
            _both_fail(path)
    finally:
        if seed % 2:
            monkeypatch.delenv("SRN_INGEST_CHUNK_BYTES")
            capi.reload_knobs()


def _event_rows(seed=5, n=5000):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 400, n).astype(np.uint64)
    s[::97] = np.uint64(2 ** 64 - 5)
    it = rng.integers(0, 60, n).astype(np.uint64)
    t = rng.integers(-5, 10 ** 9, n) + 0.5 * rng.integers(-1, 2, n)
    return s, it, t.astype(np.float64)


def test_from_events_equals_the_tsv(tmp_path):
    import torch
    s, it, t = _event_rows()
    path = _write(tmp_path / "e.tsv", HEADER + "".join("%d\t%d\t%r\n" % (a, b, c) for a, b, c in zip(s.tolist(), it.tolist(), t.tolist())))
    (ho, hi, ht), _, _ = _load(path, "host")
    ti = np.trunc(t).astype(np.int64)
    path_i = _write(tmp_path / "ei.tsv", HEADER + "".join("%d\t%d\t%d\n" % (a, b, c) for a, b, c in zip(s.tolist(), it.tolist(), ti.tolist())))
    (io, ii, it_), _, _ = _load(path_i, "host")
    dev = torch.device("cuda", 0)
    forms = {
        "numpy": (s, it, t, ti),
        "torch_cpu": (torch.from_numpy(s.view(np.int64)), torch.from_numpy(it.view(np.int64)), torch.from_numpy(t), torch.from_numpy(ti)),
        "torch_gpu": tuple(torch.from_numpy(a).to(dev) for a in (s.view(np.int64), it.view(np.int64), t, ti)),
    }
    for name, (a, b, c, ci) in forms.items():
        g = TrainingSessions.from_events(a, b, c, device=0)
        go, gi, gt = g.arrays()
        g.close()
        assert np.array_equal(go, ho) and np.array_equal(gi, hi) and np.array_equal(gt, ht), name
        g = TrainingSessions.from_events(a, b, ci, device=0)
        go, gi, gt = g.arrays()
        g.close()
        assert np.array_equal(go, io) and np.array_equal(gi, ii) and np.array_equal(gt, it_), name + " int64"
    one = TrainingSessions.from_events(s[:1], it[:1], t[:1])
    assert len(one.arrays()[0]) == 1
    one.close()


def _check_new_from_csv(path, m, idfw, k, n_items_hint):
    host = sa.VMISIndex.new_from_csv(path, m, idfw, device=0, loader="host")
    gpu = sa.VMISIndex.new_from_csv(path, m, idfw, device=0, loader="gpu")
    assert gpu.info == host.info
    s = TrainingSessions.from_tsv(path)
    _, items, _ = s.arrays()
    s.close()
    for item in np.unique(items).tolist():
        pa, ia = gpu.postings(item)
        pb, ib = host.postings(item)
        assert (pa is None) == (pb is None)
        if pb is not None:
            assert np.array_equal(pa, pb) and ia == ib
    qi, qo = synth.queries(4096, n_items_hint)
    rng = np.random.default_rng(3)
    known = np.unique(items)
    qi = known[rng.integers(0, len(known), len(qi))]          # queries over the file's own items
    ga = sa.predict_batch(gpu, (qi, qo), k, m, synth.HOW_MANY, False)
    hb = sa.predict_batch(host, (qi, qo), k, m, synth.HOW_MANY, False)
    for x, y in zip(ga, hb):
        assert np.array_equal(x, y)
    return host, gpu


def test_new_from_csv_gpu_matches_host_on_the_example(tmp_path):
    path = os.path.join(extract_example(tmp_path), "train.txt")
    _check_new_from_csv(path, 500, 1.0, 100, 30000)


def test_new_from_csv_gpu_matches_host_on_a_config2_file(tmp_path):
    inter, n_items, k, m, idfw = synth.CONFIGS["cfg2"]
    off, items, ts = synth.training_sessions(inter, n_items)
    s, it, t = synth.training_events(off, items, ts)
    path = str(tmp_path / "cfg2.tsv")
    synth.write_training_tsv(path, s, it, t, bad_lines=5)
    _, info = _same(path)
    assert info["skipped"] >= 6 and info["host_parsed"] >= 0
    host, _ = _check_new_from_csv(path, m, idfw, k, n_items)
    ev = sa.VMISIndex.from_events(s, it, t, m, idfw, device=0)   # the same rows from memory
    assert ev.info == host.info
