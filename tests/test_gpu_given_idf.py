"""The scoring kernels on idf AS GIVEN (VMISIndex::new, the Avro route: vmis_index.rs:201-228 takes idf from the item files): near-ties, wide ranges, spikes, mixed signs.

Every other index of the suite has idf = ln(total / count) * weighting -- one smooth positive curve over a decade, falling with the dense index.  Here one Avro index per
idf PROFILE is written by the synthetic producer (synth.avro_index(..., idf=)); profiles differ in the item files' idf only, each a pure function of (item id, dense
popularity rank r), so the files, the oracle and the exact check below all start from the same doubles.  Both sides then do one IEEE multiply and one IEEE divide
(DESIGN.md 1): rows are compared BIT FOR BIT with the canonical oracle over the lists as given (orc_index_from_parts), on every kernel path.

  near     B[h % 6] * (1 + s * 2^-44), B = {1, 1.5, 2, 3, 4, 6}, s hashed in +-1024: scores that share their top 32 bits and differ below, for equal acc and across
           different acc (2 * 3 against 3 * 2); the id order is the wrong answer about half the time
  rising   (1 + (r % 16) / 16) * 2^(-100 + 200 r / n): idf_hi sits in the sketch region, the sample's x values are tiny
  falling  the mirror image: huge x in the sample, the integer floors clamp
  spike    1 everywhere but 2^60 / 2^-60 on one item each of the sample, of a direct-mapped chunk >= 2 and of the sketch region
  signs    a hashed third of the items has idf in {-3.5, -0.0, 0.0} (the un-weighted branch, mod.rs:146-152), the rest the builder's rule
  limits   both ends of the range the loader serves, 2^900 and 2^-900, side by side
  edge     as signs plus NaN, +-inf or a positive value outside 2^-900 .. 2^900 (subnormals among them) on one item: REFUSED at load, per class (DESIGN.md 5,
           INTEGRATION.md) -- pinned on the host below

Host part (no GPU): the producer's idf= argument, the byte identity of idf=None, the exact-rational cross-check of fixture and oracle, and the fixture-quality
conditions, which are computed from the oracle's rows alone.  Measured shares (768 queries, k 40, m 64 = m_index, how_many 21; see test_fixture_quality):
  near:    0.995 of the queries have two adjacent returned scores with equal top words and unequal low words, 0.647 have such a pair AT the cut
           (21st against the best one left out), 0.647 both
  rising / falling / spike: 0.992 of the queries score items of all three accumulator classes (sample idx < 512, direct-mapped 512..3967, sketch >= 3968);
           a returned row holds all three in 0.025 / 0.001 / 0.056 of the queries (rising returns sketch items, falling sample items: that is the point)

GPU part: 768 sessions per batch through every path, with the path counters asserted.  Default path, queries handed to the general kernel (of 768): near 0, rising 375,
falling 0, spike 0, signs 0, limits 0 -- rising's loose thresholds collect more candidates than the lean layout holds; the general kernel answers those, bit for bit too.
"""
import hashlib
import os
from fractions import Fraction

import numpy as np
import pytest

import avro_spec_reader as ASR
from helpers import canonical_acc_over_given_lists, small_dataset
from serenade_amd import synth
from serenade_amd.synth import dense_rank, id_hash as _hash, idf_profile as profile_idf

NQ = 768                       # one batch: above SRN_TINY_MAX (256), below SRN_ORDER_MIN
PROFILES = ["near", "rising", "falling", "spike", "signs", "limits"]
BIG = dict(k=40, m=64, m_index=64, max_len=34, n_items=6000, interactions=150_000)
SMALL = dict(k=100, m=500, m_index=2500, max_len=14)        # test_gpu_mid_tier.py's LONG dataset: MID / BIG / LONG admit its sessions
DENSE = dict(k=1500, m=2500, m_index=3000, max_len=12)      # test_gpu_mid_tier.py's BIG dataset: 150 items, dense lists -- merged lists beyond the 53 KB layout
HOW_MANY = 21
SAMPLE_END, DIRECT_END = 512, 3968                          # the fast kernel's accumulator classes by dense idx


# the profiles are pure functions of (id, r), defined beside the producer (synth.idf_profile) so that tools/fuzz_parity.py draws the same ones
EDGE_VALUES = {"subnormal": 5e-324 * 1000, "below": 2.0 ** -901, "above": 2.0 ** 901, "inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}


def item_flags(ids):
    """Real product flags (bit0 IsAdult, bit1 ForSale; 0xFF: no attributes at all), hashed: about a quarter of the items may not be recommended."""
    h = _hash(ids, 3) % np.uint64(20)
    return np.select([h < 2, h < 3, h < 14, h < 18], [0, 1, 2, 3], 0xFF).astype(np.uint8)


# ---- datasets and per-profile indices, built once per module -------------------------------------------------------------------------------------------------

_CACHE = {}


def _long_queries(seed, ids, n, lo, hi, unknown_rate=0.03, dup_rate=0.08):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, len(ids) + 1) ** 0.9
    w /= w.sum()
    qs = []
    for _ in range(n):
        ln = int(rng.integers(lo, hi + 1))
        q = ids[rng.choice(len(ids), size=ln, p=w)].tolist()
        for j in range(ln):
            if rng.random() < unknown_rate:
                q[j] = int(7 + rng.integers(0, 1000))
            elif j and rng.random() < dup_rate:
                q[j] = q[int(rng.integers(0, j))]
        qs.append([int(x) for x in q])
    return qs


def _flat(qs):
    off = np.zeros(len(qs) + 1, np.uint32)
    off[1:] = np.cumsum([len(q) for q in qs])
    return np.array([x for q in qs for x in q], np.uint64), off


def dataset(which, root):
    """-> dict: training sessions, the producer's lists and computed idf (idf=None), dense ranks, the index's recency order, the query batches."""
    if which in _CACHE:
        return _CACHE[which]
    import serenade_amd as sa
    if which == "big":
        P = BIG
        off, items, ts = synth.training_sessions(P["interactions"], P["n_items"])
        qi, qo = synth.queries(600, P["n_items"], max_items=6)
        assert len(qo) - 1 >= NQ
        queries = {"1-6": (qi[:qo[NQ]].copy(), qo[:NQ + 1].copy())}
    elif which == "dense":
        P = DENSE
        off, items, ts, pub = small_dataset(31, n_sessions=40000, n_items=150, max_len=12)
        queries = {"4-10": _flat(_long_queries(13, pub, NQ, 4, 10, unknown_rate=0.05, dup_rate=0.1))}
    else:
        P = SMALL
        off, items, ts, pub = small_dataset(41, n_sessions=40000, n_items=400, max_len=14)
        longq = _long_queries(22, pub, NQ, 11, 20)
        for i in range(0, NQ, 3):                               # a third: only positions 11.. hold known items -- every weight is <= 0, negative scores ARE returned (mod.rs:143-153)
            longq[i][-10:] = [int(7 + (i * 10 + j) % 1000) for j in range(10)]
        queries = {"5-10": _flat(_long_queries(21, pub, NQ, 5, 10)), "11-20": _flat(longq)}
    base_dir = os.path.join(root, which + "-base")
    ids, loff, lsess, base = synth.avro_index(base_dir, off, items, ts, P["m_index"], P["max_len"], 1.0, "ours", files=2)
    host = sa.VMISIndex.new_from_avro(base_dir, device=-1)
    assert host.info["incomplete_items"] == 0
    r = dense_rank(ids, lsess, off, items)
    host.set_fallback_popular(4096)                             # the LOADER's dense order (its first 4 096 items): the restatement the profiles aim with must be that order
    assert np.array_equal(host.fallback(), ids[np.argsort(r)][:4096]), "synth.dense_rank is not the dense index the Avro loader builds"
    d = dict(P, name=which, off=off, items=items, ts=ts, ids=ids, loff=loff, lsess=lsess, base=base, r=r, rank=host.session_recency(),
             queries=queries, root=root, base_dir=base_dir, flags=item_flags(ids))
    _CACHE[which] = d
    return d


def profile(which, name, root):
    """The Avro index of one profile, its oracle (lists, idf, flags as given; canonical form in the index's own recency order) and the oracle's rows, cached."""
    key = (which, name)
    if key in _CACHE:
        return _CACHE[key]
    from oracle import oracle as O
    D = dataset(which, root)
    idf = profile_idf(name, D["ids"], D["r"], D["base"])
    path = os.path.join(root, "%s-%s" % (which, name))
    ids, loff, lsess, got_idf = synth.avro_index(path, D["off"], D["items"], D["ts"], D["m_index"], D["max_len"], 1.0, "ours", files=2, idf=idf)
    assert np.array_equal(ids, D["ids"]) and np.array_equal(lsess, D["lsess"]) and got_idf.tobytes() == idf.tobytes()
    oix = O.OracleIndex.from_parts(ids, (loff, lsess), idf, np.full(len(ids), 2, np.uint8), D["off"], D["items"], D["ts"], tie_rank=D["rank"])
    oix.set_attributes(ids, D["flags"])
    p = dict(D=D, name=name, idf=idf, path=path, oix=oix, refs={})
    _CACHE[key] = p
    return p


def oracle_rows(p, span, how_many=HOW_MANY, business=False):
    key = (span, how_many, business)
    if key not in p["refs"]:
        qi, qo = p["D"]["queries"][span]
        p["refs"][key] = p["oix"].predict_batch("canonical", qi, qo, p["D"]["k"], p["D"]["m"], how_many, business, threads=4)
    return p["refs"][key]


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    yield str(tmp_path_factory.mktemp("given_idf"))
    _CACHE.clear()


# ---- host: the producer's idf= argument ----------------------------------------------------------------------------------------------------------------------

def _files(base):
    out = {}
    for sub in ("itemindex", "sessionindex"):
        for f in sorted(os.listdir(os.path.join(base, sub))):
            with open(os.path.join(base, sub, f), "rb") as fh:
                out[sub + "/" + f] = fh.read()
    return out


def test_idf_none_writes_the_same_bytes_as_before(tmp_path):
    """avro_index(..., idf=None) does not go through the idf setter: the files of a fixed small index hash to PINNED_SHA256_IDF_NONE -- the digest the generator of the
    commit before the idf= argument gives for the same call (idf weighting 0: every idf is 0.0 whatever the libm, so the pin holds on any machine) -- and handing the
    computed idf back through idf=, as an array or a callable, changes no byte."""
    off, items, ts, _ = small_dataset(46, n_sessions=700, n_items=90, tied_timestamps=True)
    synth.avro_index(tmp_path / "zero", off, items, ts, 40, 9, 0.0, "mixed", files=3)
    digest = hashlib.sha256(b"".join(k.encode() + v for k, v in sorted(_files(tmp_path / "zero").items()))).hexdigest()
    assert digest == PINNED_SHA256_IDF_NONE, digest
    ids, loff, lsess, idf = synth.avro_index(tmp_path / "none", off, items, ts, 40, 9, 2.0, "per-item", files=3)
    assert (idf > 0).all()
    for how, arg in (("array", idf.copy()), ("callable", lambda got_ids: idf[np.searchsorted(ids, got_ids)])):
        ids2, loff2, lsess2, idf2 = synth.avro_index(tmp_path / how, off, items, ts, 40, 9, 2.0, "per-item", files=3, idf=arg)
        assert np.array_equal(ids, ids2) and np.array_equal(loff, loff2) and np.array_equal(lsess, lsess2) and idf2.tobytes() == idf.tobytes()
        assert _files(tmp_path / how) == _files(tmp_path / "none")


PINNED_SHA256_IDF_NONE = "28e19543030f80a60335f7ba62d87f79a15a99d429f67acf9c1659759c7738b0"


def test_given_idf_reaches_the_files_and_the_loader(tmp_path):
    """idf= overrides the computed values in the item files (read back by the independent spec-level reader) and in what the loader serves with; nothing else changes;
    a wrong length is refused."""
    import serenade_amd as sa
    off, items, ts, _ = small_dataset(46, n_sessions=700, n_items=90, tied_timestamps=True)
    ids, loff, lsess, base = synth.avro_index(tmp_path / "a", off, items, ts, 40, 9, 1.0, "reverse", files=2)
    given = profile_idf("signs", ids, np.arange(len(ids)), base) * np.where(_hash(ids, 9) % np.uint64(2) == 0, 2.0 ** 70, 2.0 ** -70)
    ids2, loff2, lsess2, idf2 = synth.avro_index(tmp_path / "b", off, items, ts, 40, 9, 1.0, "reverse", files=2, idf=lambda x: given)
    assert np.array_equal(ids, ids2) and np.array_equal(loff, loff2) and np.array_equal(lsess, lsess2) and idf2.tobytes() == given.tobytes()
    fa, fb = _files(tmp_path / "a"), _files(tmp_path / "b")
    assert all(fa[k] == fb[k] for k in fa if k.startswith("sessionindex/")) and all(len(fa[k]) == len(fb[k]) and fa[k] != fb[k] for k in fa if k.startswith("itemindex/"))
    recs = {}
    for part in range(2):
        for rec in ASR.read_container(f"{tmp_path}/b/itemindex/part-{part}.avro")[2]:
            recs[rec["ItemId"]] = rec
    want = dict(zip(ids.tolist(), given.tolist()))
    assert sorted(recs) == sorted(want)
    for it, rec in recs.items():
        assert np.float64(rec["idf"]).tobytes() == np.float64(want[it]).tobytes()                       # (-0.0 stays -0.0)
    ix = sa.VMISIndex.new_from_avro(tmp_path / "b", device=-1)
    for j in range(0, len(ids), 7):
        sess, f = ix.postings(int(ids[j]))
        assert np.float64(f).tobytes() == np.float64(given[j]).tobytes() and sorted(sess.tolist()) == sorted(lsess[int(loff[j]):int(loff[j + 1])].tolist())
    with pytest.raises(ValueError):
        synth.avro_index(tmp_path / "c", off, items, ts, 40, 9, 1.0, "reverse", idf=given[:-1])


@pytest.mark.parametrize("value_class", sorted(EDGE_VALUES))
def test_edge_idf_is_refused_at_load(tmp_path, value_class):
    """The `edge` profile.  The reference reads these doubles as they are; this library REFUSES at load, with an error that names the item:
    NaN, +inf and -inf, and every positive value outside 2^-900 .. 2^900 -- positive subnormals among them.  Inside that range idf * acc, times and over 10 U, stays a
    finite normal double, which is what the kernels' thresholds and integer floors assume; outside it the general kernel's floor overflows and drops items.  One item is
    enough; the same index with both ends of the served range on those items loads (and is served bit for bit: the `limits` profile on the GPU)."""
    import serenade_amd as sa
    off, items, ts, _ = small_dataset(46, n_sessions=700, n_items=90, tied_timestamps=True)
    ids, _, lsess, base = synth.avro_index(tmp_path / "ok", off, items, ts, 40, 9, 1.0, "ours", files=2)
    r = dense_rank(ids, lsess, off, items)
    bad = profile_idf("signs", ids, r, base)
    synth.avro_index(tmp_path / "signs", off, items, ts, 40, 9, 1.0, "ours", files=2, idf=bad)
    assert sa.VMISIndex.new_from_avro(tmp_path / "signs", device=-1).info["n_items"] == len(ids)       # (mixed signs and -0.0 ARE served)
    bad[r == 11] = EDGE_VALUES[value_class]
    synth.avro_index(tmp_path / "bad", off, items, ts, 40, 9, 1.0, "ours", files=2, idf=bad)
    with pytest.raises(sa.SerenadeError) as e:
        sa.VMISIndex.new_from_avro(tmp_path / "bad", device=-1)
    assert e.value.code == -1 and "idf" in str(e.value) and str(int(ids[r == 11][0])) in str(e.value), str(e.value)
    bad[r == 11] = synth.IDF_SERVED_MIN
    bad[r == 12] = synth.IDF_SERVED_MAX
    synth.avro_index(tmp_path / "limits", off, items, ts, 40, 9, 1.0, "ours", files=2, idf=bad)
    assert sa.VMISIndex.new_from_avro(tmp_path / "limits", device=-1).info["n_items"] == len(ids)


# ---- host: fixture and oracle against exact rationals; fixture quality ---------------------------------------------------------------------------------------

def _python_view(D):
    if "lists" not in D:
        off, items = D["off"].astype(np.int64), D["items"]
        D["rows"] = [set(items[off[s]:off[s + 1]].tolist()) for s in range(len(off) - 1)]
        D["lists"] = {int(it): D["lsess"][int(a):int(b)].tolist() for it, a, b in zip(D["ids"], D["loff"][:-1], D["loff"][1:])}
    return D["lists"], D["rows"]


@pytest.mark.parametrize("name", PROFILES)
def test_oracle_order_never_contradicts_the_exact_order(root, name):
    """Every 8th query: score = Fraction(idf) * acc / (10 U) exactly, acc and U from the pure-Python statement of the canonical form over the lists as given.  The oracle's
    rows hold the doubles of `one multiply, one divide` bit for bit, and their order never contradicts the exact one: a pair may stand inverted -- within the row, or between
    the row's last entry and anything left out -- only where its two ROUNDED scores are equal (then the id decides)."""
    p = profile("big", name, root)
    D = p["D"]
    lists, rows = _python_view(D)
    idf_eff = {int(i): (float(v) if v > 0 else 1.0) for i, v in zip(D["ids"], p["idf"])}
    ref = oracle_rows(p, "1-6")
    qi, qo = D["queries"]["1-6"]
    for q in range(0, NQ, 8):
        session = qi[qo[q]:qo[q + 1]].tolist()
        acc, U = canonical_acc_over_given_lists(lists, rows, D["ts"], session, D["k"], D["m"], rank=D["rank"])
        exact = {it: Fraction(idf_eff[it]) * a / (10 * U) for it, a in acc.items()}
        rounded = {it: idf_eff[it] * float(a) / float(10 * U) for it, a in acc.items()}
        c = int(ref["counts"][q])
        got = ref["ids"][q, :c].tolist()
        assert c == min(HOW_MANY, len(acc)) and len(set(got)) == c and all(it in acc for it in got), (q, session)
        assert all(np.float64(rounded[it]).tobytes() == ref["scores"][q, j].tobytes() for j, it in enumerate(got)), (q, session)
        for a, b in zip(got[:-1], got[1:]):
            assert exact[a] >= exact[b] or rounded[a] == rounded[b], (q, a, b)
            assert rounded[a] > rounded[b] or (rounded[a] == rounded[b] and a < b), (q, a, b)
        if c:
            last = got[-1]
            for it in set(acc) - set(got):
                assert exact[it] <= exact[last] or rounded[it] == rounded[last], (q, it, last)
                assert rounded[it] < rounded[last] or (rounded[it] == rounded[last] and it > last), (q, it, last)


def _near_pair(a, b):
    a, b = np.float64(a).view(np.uint64), np.float64(b).view(np.uint64)
    return (a >> np.uint64(32)) == (b >> np.uint64(32)) and a != b


def fixture_quality(root, name):
    p = profile("big", name, root)
    D = p["D"]
    qi, qo = D["queries"]["1-6"]
    out = {}
    if name == "near":
        ref = p["oix"].predict_batch("canonical", qi, qo, D["k"], D["m"], HOW_MANY + 1, False, threads=4)
        inside = at_cut = both = 0
        for q in range(NQ):
            c, sc = int(ref["counts"][q]), ref["scores"][q]
            a = any(_near_pair(sc[j], sc[j + 1]) for j in range(min(c, HOW_MANY) - 1))
            b = c == HOW_MANY + 1 and _near_pair(sc[HOW_MANY - 1], sc[HOW_MANY])
            inside += a; at_cut += b; both += a and b
        out = dict(inside=inside / NQ, at_cut=at_cut / NQ, both=both / NQ)
    else:
        cls_of = dict(zip(D["ids"].tolist(), np.digitize(D["r"], [SAMPLE_END, DIRECT_END]).tolist()))
        ref = oracle_rows(p, "1-6")
        scored = returned = 0
        for q in range(NQ):
            ids_q, _, _ = p["oix"].scores_canonical(qi[qo[q]:qo[q + 1]], D["k"], D["m"])
            scored += len({cls_of[int(i)] for i in ids_q}) == 3
            returned += len({cls_of[int(i)] for i in ref["ids"][q, :int(ref["counts"][q])]}) == 3
        out = dict(scored=scored / NQ, returned=returned / NQ)
    return out


@pytest.mark.parametrize("name", ["near", "rising", "falling", "spike"])
def test_fixture_quality(root, name):
    """A profile must keep testing what it claims -- from the ORACLE's rows alone.  near: in at least a quarter of the queries the returned row has two adjacent scores with
    equal top 32 bits and unequal low words AND the how_many-th candidate and the best one left out (the oracle asked for how_many + 1) are such a pair.  rising / falling /
    spike: at least a quarter of the queries score items of all three accumulator classes.  The catalogue is larger than 4 096, so the classes and the replicated hot items exist."""
    D = dataset("big", root)
    assert len(D["ids"]) > 4096 and (np.diff(D["off"].astype(np.int64)) > 30).any()
    qual = fixture_quality(root, name)
    print("fixture quality, %s: %s" % (name, qual))
    assert (qual["both"] if name == "near" else qual["scored"]) >= 0.25, qual
    if name == "spike":
        assert all((D["r"] == rr).any() for rr in synth.IDF_SPIKES)


def test_signs_profile_mixes_both_branches(root):
    p = profile("big", "signs", root)
    assert 0.25 < (p["idf"] <= 0).mean() < 0.45 and (np.signbit(p["idf"]) & (p["idf"] == 0)).any() and (p["idf"] < 0).any() and (p["idf"] > 0).any()
    ref = oracle_rows(p, "1-6")
    eff = dict(zip(p["D"]["ids"].tolist(), (p["idf"] <= 0).tolist()))
    rows_mixed = sum(len({eff[int(i)] for i in ref["ids"][q, :int(ref["counts"][q])]}) == 2 for q in range(NQ))
    assert rows_mixed >= NQ // 2, rows_mixed                   # both branches within one returned row


# ---- GPU: every path, bit for bit ----------------------------------------------------------------------------------------------------------------------------

def gpu_index(which, name, root):
    key = ("gix", which, name)
    if key not in _CACHE:
        import serenade_amd as sa
        p = profile(which, name, root)
        gix = sa.VMISIndex.new_from_avro(p["path"])
        assert np.array_equal(gix.session_recency(), p["D"]["rank"]) and gix.info["incomplete_items"] == 0
        gix.set_attributes(p["D"]["ids"], p["D"]["flags"])
        _CACHE[key] = gix
    return _CACHE[key]


def assert_same_bits(got, ref, what):
    ids, sc, cnt = got
    assert np.array_equal(cnt, ref["counts"]), (what, "counts", np.flatnonzero(cnt != ref["counts"])[:5].tolist())
    bad = np.flatnonzero((ids != ref["ids"]).any(axis=1))
    assert bad.size == 0, (what, "ids", len(bad), int(bad[0]), ids[bad[0]].tolist(), ref["ids"][bad[0]].tolist())
    bits, rbits = np.ascontiguousarray(sc).view(np.uint64), ref["scores"].view(np.uint64)
    bad = np.flatnonzero((bits != rbits).any(axis=1))
    assert bad.size == 0, (what, "score bits", len(bad), int(bad[0]), sc[bad[0]].tolist(), ref["scores"][bad[0]].tolist())


@pytest.fixture
def knobs(monkeypatch):
    from serenade_amd import capi

    def switch(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capi.reload_knobs()
    yield switch
    monkeypatch.undo()
    capi.reload_knobs()


# path -> (knobs, how_many, business rules)
PATHS = {
    "default": ({}, HOW_MANY, False),
    "no_fast": ({"SRN_NO_FAST": "1"}, HOW_MANY, False),
    "no_merge": ({"SRN_NO_MERGE": "1"}, HOW_MANY, False),
    "sketch64": ({"SRN_SKETCH_SLOTS": "64", "SRN_HOT_SLOTS": "32"}, HOW_MANY, False),
    "fast_runs3": ({"SRN_FAST_RUNS": "3"}, HOW_MANY, False),
    "serving_order": ({"SRN_ORDER_MIN": "1"}, HOW_MANY, False),
    "business": ({}, HOW_MANY, True),
    "how_many5": ({}, 5, False),
    "how_many50": ({}, 50, False),
    "how_many64": ({}, 64, False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", PROFILES)
def test_batch_paths_bit_for_bit(root, knobs, name, path):
    """One batch of 768 sessions of 1..6 items through each kernel path: counts, ids and score BITS equal the canonical oracle's (hence the same bytes on every path),
    and the counters say the intended path served the batch where a counter exists: the general kernel's share (all of it for SRN_NO_FAST and the non-default
    geometries, at most half on the default path, for every profile), the serving order's merged repeats.  SRN_FAST_RUNS=3 and the how_many paths have no counter of their
    own -- the 29-bit slot form and the ceil(n / 8) sample leave no trace in the C ABI -- so there only `not everything was handed over` is asserted."""
    import serenade_amd as sa
    env, how_many, business = PATHS[path]
    p = profile("big", name, root)
    D = p["D"]
    gix = gpu_index("big", name, root)
    ref = oracle_rows(p, "1-6", how_many, business)
    knobs(env)
    got = sa.predict_batch(gix, D["queries"]["1-6"], D["k"], D["m"], how_many, business)
    nq, general, glob = gix.last_path_counts()
    dedup = gix.last_dedup_count()
    print("path counts, %s / %s: %d queries, %d general kernel, %d global-table pass, %d MID, %d BIG, %d deduplicated" % (name, path, nq, general, glob, gix.last_mid_count(), gix.last_big_count(), dedup))
    assert_same_bits(got, ref, (name, path))
    assert nq == NQ
    if path in ("no_fast", "no_merge", "sketch64"):            # (a non-default geometry is the general kernel's: its hash mode, its sketch words)
        assert general == NQ
    elif path == "default":
        assert general <= NQ // 2, "%s: %d of %d queries left the fast kernels" % (name, general, NQ)
        assert dedup == 0
    elif path == "serving_order":
        qi, qo = D["queries"]["1-6"]
        assert len({qi[qo[q]:qo[q + 1]].tobytes() for q in range(NQ)}) < NQ
        assert dedup > 0, "the serving order merges the batch's repeated sessions: it did not run"
        assert general < NQ
    else:
        assert general < NQ, "%s / %s: every query was handed to the general kernel" % (name, path)
    if business:
        allowed = dict(zip(D["ids"].tolist(), D["flags"].tolist()))
        assert all(allowed[int(i)] != 0xFF and allowed[int(i)] & 2 for q in range(NQ) for i in got[0][q, :int(got[2][q])])
        plain = oracle_rows(p, "1-6", how_many, False)
        assert not np.array_equal(plain["ids"], ref["ids"])      # (the rules did exclude something)


@pytest.mark.gpu
@pytest.mark.parametrize("span", ["5-10", "11-20"])
@pytest.mark.parametrize("name", PROFILES)
def test_mid_and_long_forms_bit_for_bit(root, knobs, name, span):
    """The small dataset (400 items, lists of up to 2 500): sessions of 5..10 items (MID: the listed count is asserted) and of 11..20 items (LONG; negative weights from
    the eleventh position on, so negative scores order by idf * acc too).  The library has no counter of the queries LONG served: what is asserted is that the general
    kernel got no more than the third whose scores are all <= 0, which only it answers.  MID's BIG form: test_big_form_bit_for_bit."""
    import serenade_amd as sa
    p = profile("small", name, root)
    D = p["D"]
    gix = gpu_index("small", name, root)
    ref = oracle_rows(p, span)
    knobs({})
    got = sa.predict_batch(gix, D["queries"][span], D["k"], D["m"], HOW_MANY, False)
    nq, general, glob = gix.last_path_counts()
    print("path counts, small %s / %s: %d queries, %d general kernel, %d global-table pass, %d MID, %d BIG" % (name, span, nq, general, glob, gix.last_mid_count(), gix.last_big_count()))
    assert_same_bits(got, ref, (name, span))
    assert nq == NQ
    if span == "5-10":
        assert gix.last_mid_count() >= NQ // 4 and general <= NQ // 4
    else:
        assert (ref["scores"] < 0).any() and (ref["scores"] > 0).any()
        assert general <= (NQ + 2) // 3, "sessions of 11..20 items with positive scores belong to the LONG form (%d reached the general kernel)" % general


@pytest.mark.gpu
@pytest.mark.parametrize("name", PROFILES)
def test_big_form_bit_for_bit(root, knobs, name):
    """MID's BIG form (80 KB of LDS): 150 items with lists of up to 3 000, sessions of 4..10 items, k 1 500 over m 2 500 -- merged lists beyond the 53 KB layout.  The
    BIG list's count is asserted, and that BIG serves most of it.  (vmis_finish_big_kernel, the finish of queries with more than 63 entries, has no counter the C ABI
    exposes: whether a query of these batches went through it cannot be asserted, only that every row is right.)"""
    import serenade_amd as sa
    p = profile("dense", name, root)
    D = p["D"]
    gix = gpu_index("dense", name, root)
    ref = oracle_rows(p, "4-10")
    knobs({})
    got = sa.predict_batch(gix, D["queries"]["4-10"], D["k"], D["m"], HOW_MANY, False)
    nq, general, glob = gix.last_path_counts()
    mid, big = gix.last_mid_count(), gix.last_big_count()
    print("path counts, dense %s: %d queries, %d general kernel, %d global-table pass, %d MID, %d BIG" % (name, nq, general, glob, mid, big))
    assert_same_bits(got, ref, name)
    assert nq == NQ and 0 < big <= mid
    assert general < big, "the BIG form should serve most of what MID lists for it (%d listed, %d reached the general kernel)" % (big, general)


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", PROFILES)
def test_single_calls_bit_for_bit(root, knobs, name, fused):
    """40 srn_predict calls (the reference's call shape): the latency path's fused launch, then SRN_TINY_FUSED=0.  The library counts the queries of a call and those the
    general kernel served, not the launches: no counter tells the fused launch from the unfused sequence, so the knob is the only statement of the path here."""
    import serenade_amd as sa
    p = profile("big", name, root)
    D = p["D"]
    gix = gpu_index("big", name, root)
    ref = oracle_rows(p, "1-6")
    qi, qo = D["queries"]["1-6"]
    knobs({} if fused else {"SRN_TINY_FUSED": "0"})
    for q in range(0, 40 * 19, 19):
        recs = sa.predict(gix, qi[qo[q]:qo[q + 1]], D["k"], D["m"], HOW_MANY, False)
        c = int(ref["counts"][q])
        assert [r.id for r in recs] == ref["ids"][q, :c].tolist(), (name, q)
        assert np.array([r.score for r in recs], np.float64).tobytes() == ref["scores"][q, :c].tobytes(), (name, q)
        assert gix.last_path_counts()[0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n_shards", [2, 8])
@pytest.mark.parametrize("name", PROFILES)
def test_shard_group_bit_for_bit(root, knobs, name, n_shards):
    """A local shard group cut from the same index (ShardedVMISIndex.from_full), neighbours pipeline: the merge of the shards' rows at G = 2, the wave-per-query back end
    (floors per chunk of 256) at G = 8."""
    import ctypes as C
    import torch
    from serenade_amd import capi, sharded
    p = profile("big", name, root)
    D = p["D"]
    gix = gpu_index("big", name, root)
    ref = oracle_rows(p, "1-6")
    qi, qo = D["queries"]["1-6"]
    knobs({})
    dev = torch.device("cuda:0")
    d_f, d_o = torch.from_numpy(qi.view(np.int64).copy()).to(dev), torch.from_numpy(qo.view(np.int32).copy()).to(dev)
    shards = [sharded.ShardedVMISIndex.from_full(gix, g, n_shards) for g in range(n_shards)]
    grp = sharded.ShardGroup.local(shards)
    try:
        for with_postings in (False, True):
            if with_postings:
                grp.set_postings(sharded.postings_view(gix))
            res = grp.predict_batch(d_f, d_o, NQ, 6, D["k"], D["m"], HOW_MANY, False)
            torch.cuda.synchronize()
            got = (res[0].cpu().numpy().view(np.uint64), res[1].cpu().numpy(), res[2].cpu().numpy().view(np.uint32))
            assert_same_bits(got, ref, (name, n_shards, with_postings))
        assert grp.stats["neighbour_batches"] == 1
        launches = C.c_uint64()
        capi.check(capi.lib().srn_debug_sback_launches(shards[0]._h, C.byref(launches)))
        assert (launches.value >= 1) if n_shards >= 8 else (launches.value == 0), launches.value
    finally:
        grp.close()
