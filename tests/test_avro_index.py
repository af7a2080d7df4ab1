"""The reference's pre-built index format (Avro item / session index, vmis_index.rs:85-314) -> flat index.

CPU part: the files written by tests/avro_write.py (same schemas, codecs null and snappy) are parsed and the index contents are
what went in.  GPU part: an index loaded from Avro predicts exactly what the index built from the same sessions predicts when
the Avro files carry that index's own posting lists and idf (i.e. the offline producer and the TSV builder agree)."""
import numpy as np
import pytest

import avro_spec_reader as ASR
import avro_write as AW
from helpers import canonical_over_given_lists as _canonical_over_given_lists, flatten, random_queries, small_dataset


def pyarrow_snappy(data):
    """THIRD-PARTY compressor (Google's snappy as bundled by pyarrow): raw-format streams this repository's author did not produce."""
    import pyarrow as pa
    return pa.Codec("snappy").compress(bytes(data)).to_pybytes()


def _write_index(base, off, items, ts, m_index, idf_of, attrs=None, codec="snappy", files=2, reorder_ties=False, compressor=None):
    """The producer side: per item its m_index most recent sessions (by (time, session index)), idf, flags; per session its row."""
    n = len(ts)
    order = np.lexsort((np.arange(n), ts))            # ascending (time, index) = recency rank
    rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    per_item = {}
    for s in range(n):
        for it in items[off[s]:off[s + 1]].tolist():
            per_item.setdefault(it, []).append(s)
    item_recs = []
    for it, ss in sorted(per_item.items()):
        ss = sorted(ss, key=lambda s: -rank[s])[:m_index]
        if reorder_ties:
            ss = ss[::-1]                                # the loader re-orders by its own recency: any order in the file is fine
        a = attrs.get(it, (True, False)) if attrs else (True, False)
        item_recs.append(AW.enc_item(it, ss, idf_of[it], a[0], a[1]))
    sess_recs = [AW.enc_session(s, items[off[s]:off[s + 1]].tolist(), int(ts[s])) for s in range(n)]
    for part in range(files):
        AW.write_container(f"{base}/itemindex/part-{part}.avro", AW.ITEM_SCHEMA, item_recs[part::files], codec, block_records=97, compressor=compressor)
        AW.write_container(f"{base}/sessionindex/part-{part}.avro", AW.SESSION_SCHEMA, sess_recs[part::files], codec, block_records=211, compressor=compressor)
    return per_item


def _idf_like_builder(off, items, weighting):
    pairs = int(off[-1]); u, c = np.unique(items, return_counts=True)
    return {int(i): float(np.log(pairs / k) * weighting) for i, k in zip(u, c)}


def test_snappy_writer_uses_every_element_kind_and_decodes_independently():
    """The test-side compressor emits literals and copies with 1-, 2- and 4-byte offsets, overlapping ones included, and an
    independent pure-Python decoder of the format description gets the input back -- so the streams the C++ reader is fed are
    valid snappy by a second opinion, not only by its own."""
    rng = np.random.default_rng(3)
    base = bytes(rng.integers(0, 7, size=5000, dtype=np.uint8)) + b"\x00" * 300 + bytes(rng.integers(0, 255, size=70000, dtype=np.uint8))
    data = base + base[100:68000] + b"abcd" * 50          # a far repeat (offset > 65535 -> 4-byte form only), near repeats, runs
    st = {}
    z = AW.snappy_with_copies(data, st)
    assert AW.snappy_decode(z) == data
    assert st.get(1, 0) > 0 and st.get(2, 0) > 0 and st.get(3, 0) > 0 and st.get("overlap", 0) > 0, st
    assert AW.snappy_decode(AW.snappy_literal_only(data)) == data


def test_third_party_snappy_and_the_test_writer_agree_both_ways():
    """pyarrow's decompressor accepts the test writer's streams (all element kinds) and the test decoder accepts pyarrow's compressor's."""
    import pyarrow as pa
    rng = np.random.default_rng(5)
    data = bytes(rng.integers(0, 5, size=40000, dtype=np.uint8)) + b"\x07" * 1000 + bytes(rng.integers(0, 255, size=3000, dtype=np.uint8))
    for z in (AW.snappy_with_copies(data), AW.snappy_literal_only(data)):
        assert pa.Codec("snappy").decompress(z, decompressed_size=len(data)).to_pybytes() == data
    z = pyarrow_snappy(data)
    assert len(z) < len(data) * 3 // 4 and AW.snappy_decode(z) == data           # (it really compressed: copies inside)


@pytest.mark.parametrize("codec", ["null", "snappy", "snappy-copies", "snappy-pyarrow"])
def test_container_files_pass_an_independent_spec_level_reader(tmp_path, codec):
    """The files srn_avro.cpp is tested on, read back by tests/avro_spec_reader.py (generic over the header's writer schema, third-party snappy
    inflate, CRC by zlib): header magic / metadata map / sync markers / zig-zag longs / array blocks / snappy framing are the specification's,
    and the records are what went in (schemas: vmis_index.rs:184-192, 249-255)."""
    off, items, ts, ids = small_dataset(46, n_sessions=700, n_items=90, tied_timestamps=True)
    idf = _idf_like_builder(off, items, 1.0)
    attrs = {int(ids[0]): (False, True), int(ids[1]): (True, True)}
    compressor = {"snappy-copies": AW.snappy_with_copies, "snappy-pyarrow": pyarrow_snappy}.get(codec)
    per_item = _write_index(str(tmp_path), off, items, ts, 40, idf, attrs, "null" if codec == "null" else "snappy", compressor=compressor)
    got_items, got_sessions = {}, {}
    for part in range(2):
        schema, cdc, recs = ASR.read_container(f"{tmp_path}/itemindex/part-{part}.avro")
        assert schema == AW.ITEM_SCHEMA and cdc == ("null" if codec == "null" else "snappy")
        for r in recs:
            got_items[r["ItemId"]] = r
        schema, cdc, recs = ASR.read_container(f"{tmp_path}/sessionindex/part-{part}.avro")
        assert schema == AW.SESSION_SCHEMA
        for r in recs:
            got_sessions[r["SessionIndex"]] = r
    n = len(ts)
    assert sorted(got_sessions) == list(range(n)) and sorted(got_items) == sorted(per_item)
    for s in range(n):
        assert got_sessions[s]["item_ids_asc"] == items[off[s]:off[s + 1]].tolist() and got_sessions[s]["Time"] == int(ts[s])
    order = np.lexsort((np.arange(n), ts)); rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    for it, ss in per_item.items():
        r = got_items[it]
        assert r["session_indices_time_ordered"] == sorted(ss, key=lambda s: -rank[s])[:40]
        assert r["idf"] == idf[it] and (r["ForSale"], r["IsAdult"]) == attrs.get(it, (True, False))
    # and the reader under test sees the same index in them
    import serenade_amd as sa
    ix = sa.VMISIndex.new_from_avro(tmp_path, device=-1)
    for it in list(per_item)[:40]:
        sess, f = ix.postings(it)
        assert sess.tolist() == got_items[it]["session_indices_time_ordered"] and f == got_items[it]["idf"]
    # damaged files are refused by the second reader too (so "valid" above means something)
    for how, what in (("crc", "CRC"), ("sync", "sync"), ("truncate", "truncated")):
        if codec == "null" and how == "crc":
            continue
        pth = f"{tmp_path}/bad-{how}.avro"
        AW.write_container(pth, AW.SESSION_SCHEMA, [AW.enc_session(1, [2, 3], 4)] * 30, "null" if codec == "null" else "snappy", block_records=7, compressor=compressor, corrupt=how)
        with pytest.raises(ValueError):
            ASR.read_container(pth)


@pytest.mark.parametrize("codec", ["null", "snappy", "snappy-copies", "snappy-pyarrow"])
def test_avro_index_contents_on_host(tmp_path, codec):
    import serenade_amd as sa
    off, items, ts, ids = small_dataset(41, n_sessions=900, n_items=120, tied_timestamps=True)
    idf = _idf_like_builder(off, items, 1.0)
    attrs = {int(ids[0]): (False, True), int(ids[1]): (True, True)}
    compressor = {"snappy-copies": AW.snappy_with_copies, "snappy-pyarrow": pyarrow_snappy}.get(codec)
    codec = "snappy" if codec.startswith("snappy") else codec
    per_item = _write_index(str(tmp_path), off, items, ts, 40, idf, attrs, codec, reorder_ties=True, compressor=compressor)
    ix = sa.VMISIndex.new_from_avro(tmp_path, device=-1)
    ref = sa.VMISIndex.from_sessions(off, items, ts, 40, 10**6, 1.0, device=-1)
    info, rinfo = ix.info, ref.info
    for key in ("n_items", "nnz_postings", "m_index", "n_sessions_total"):
        assert info[key] == rinfo[key], key
    # rows and ranks only for the sessions some list names (round 6): the others can never be neighbours
    n = len(ts)
    order = np.lexsort((np.arange(n), ts)); rank = np.empty(n, np.int64); rank[order] = np.arange(n)
    listed = sorted(set(s for ss in per_item.values() for s in sorted(ss, key=lambda s: -rank[s])[:40]))
    assert info["n_sessions_kept"] == len(listed) < rinfo["n_sessions_kept"] and info["nnz_rows"] == sum(int(off[s + 1] - off[s]) for s in listed)
    assert info["incomplete_items"] == 0
    rec = ix.session_recency()
    assert np.flatnonzero(rec != 0xFFFFFFFF).tolist() == listed and np.array_equal(np.argsort(rec[listed]), np.argsort(rank[listed]))
    assert ix.items_for_session(listed[0]).tolist() == items[off[listed[0]]:off[listed[0] + 1]].tolist()
    with pytest.raises(sa.SerenadeError):
        ix.items_for_session(next(s for s in range(n) if s not in set(listed)))
    for it in list(per_item)[:60] + [int(ids[0]), int(ids[1])]:
        a, b = ix.postings(it), ref.postings(it)
        assert np.array_equal(a[0], b[0]) and a[1] == pytest.approx(b[1], rel=0, abs=0)      # same sessions, same order, the file's idf
    assert ix.postings(123456789)[0] is None


def test_avro_index_rejects_what_it_cannot_represent(tmp_path):
    import serenade_amd as sa
    off, items, ts, ids = small_dataset(42, n_sessions=300, n_items=40)
    idf = _idf_like_builder(off, items, 1.0)
    with pytest.raises(sa.SerenadeError) as e:
        sa.VMISIndex.new_from_avro(tmp_path / "nothing-here", device=-1)
    assert e.value.code == -5          # SRN_EIO
    n = len(ts)
    item_recs, sess_recs, _ = _records(off, items, ts, idf)
    # malformed containers: a CRC that does not match, a wrong sync marker, a block cut in half
    for how in ("crc", "sync", "truncate"):
        base = tmp_path / how
        AW.write_container(f"{base}/itemindex/a.avro", AW.ITEM_SCHEMA, item_recs, "snappy", block_records=50, compressor=AW.snappy_with_copies, corrupt=how)
        AW.write_container(f"{base}/sessionindex/a.avro", AW.SESSION_SCHEMA, sess_recs, "snappy", block_records=50, compressor=AW.snappy_with_copies)
        with pytest.raises(sa.SerenadeError) as e:
            sa.VMISIndex.new_from_avro(base, device=-1)
        assert e.value.code == -1, how
        assert {"crc": "CRC", "sync": "sync", "truncate": "truncated"}[how] in str(e.value), (how, str(e.value))
    # a session row naming an item without an item-index record (the reference would panic when scoring it)
    AW.write_container(f"{tmp_path}/orphan/itemindex/a.avro", AW.ITEM_SCHEMA, item_recs[1:], "null")
    AW.write_container(f"{tmp_path}/orphan/sessionindex/a.avro", AW.SESSION_SCHEMA, sess_recs, "null")
    with pytest.raises(sa.SerenadeError) as e:
        sa.VMISIndex.new_from_avro(tmp_path / "orphan", device=-1)
    assert e.value.code == -1


def _records(off, items, ts, idf, m_index=10**9, tie_break=-1, max_session_len=10**9):
    """Item / session records as a producer with its own tie-break among equal timestamps would write them
    (tie_break = -1: larger session index first, as prepare_hashmap does; +1: smaller first; a callable: j-th item (ascending id) -> -1 / +1).
    Sessions of more than max_session_len items are in the session index only, in no list (as the CSV path keeps them: vmis_index.rs:79, 452).
    -> (item records, session records, lists {item: sessions in the producer's order})"""
    n = len(ts)
    per_item = {}
    for s in range(n):
        if off[s + 1] - off[s] > max_session_len:
            continue
        for it in items[off[s]:off[s + 1]].tolist():
            per_item.setdefault(it, []).append(s)
    lists = {}
    for j, (it, ss) in enumerate(sorted(per_item.items())):
        tb = tie_break(j) if callable(tie_break) else tie_break
        lists[it] = sorted(ss, key=lambda s: (-int(ts[s]), tb * s))[:m_index]
    item_recs = [AW.enc_item(it, ss, idf[it], True, False) for it, ss in sorted(lists.items())]
    sess_recs = [AW.enc_session(s, items[off[s]:off[s + 1]].tolist(), int(ts[s])) for s in range(n)]
    return item_recs, sess_recs, lists


def test_avro_schema_with_reordered_and_extra_fields(tmp_path):
    """avro-rs writes the fields in the order of the producer's struct: the reader takes them by NAME from the writer schema,
    skips what it does not know (here a string and a nullable union) and accepts logical-type wrappers."""
    import serenade_amd as sa
    off, items, ts, ids = small_dataset(44, n_sessions=200, n_items=30)
    idf = _idf_like_builder(off, items, 1.0)
    item_schema = {"type": "record", "name": "ItemIndex", "fields": [
        {"name": "note", "type": "string"},
        {"name": "idf", "type": "double"},
        {"name": "IsAdult", "type": "boolean"},
        {"name": "ItemId", "type": {"type": "long", "logicalType": "whatever"}},
        {"name": "maybe", "type": ["null", "long"]},
        {"name": "ForSale", "type": "boolean"},
        {"name": "session_indices_time_ordered", "type": {"type": "array", "items": "int"}}]}
    n = len(ts)
    per_item = {}
    for s in range(n):
        for it in items[off[s]:off[s + 1]].tolist():
            per_item.setdefault(it, []).append(s)
    recs = []
    for j, (it, ss) in enumerate(sorted(per_item.items())):
        ss = sorted(ss, key=lambda s: (-int(ts[s]), -s))
        recs.append(AW.zz(3) + b"abc" + __import__("struct").pack("<d", idf[it]) + bytes([0]) + AW.zz(it) + (AW.zz(1) + AW.zz(j) if j % 2 else AW.zz(0)) + bytes([1]) + AW.enc_array(ss))
    _, sess_recs, _ = _records(off, items, ts, idf)
    AW.write_container(f"{tmp_path}/itemindex/a.avro", item_schema, recs, "snappy", compressor=AW.snappy_with_copies)
    AW.write_container(f"{tmp_path}/sessionindex/a.avro", AW.SESSION_SCHEMA, sess_recs, "null")
    ix = sa.VMISIndex.new_from_avro(tmp_path, device=-1)
    ref = sa.VMISIndex.from_sessions(off, items, ts, 10**6, 10**6, 1.0, device=-1)
    for it in list(per_item)[:30]:
        a, b = ix.postings(it), ref.postings(it)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]


def _write(tmp_path, item_recs, sess_recs):
    AW.write_container(f"{tmp_path}/itemindex/a.avro", AW.ITEM_SCHEMA, item_recs, "snappy", compressor=AW.snappy_with_copies)
    AW.write_container(f"{tmp_path}/sessionindex/a.avro", AW.SESSION_SCHEMA, sess_recs, "snappy")


def _heavily_tied_dataset():
    """3 000 sessions over 30 distinct timestamps (100 per second), 60 items: list cuts fall INSIDE large groups of equal Time."""
    off, items, ts, ids = small_dataset(47, n_sessions=3000, n_items=60, tied_timestamps=True, max_len=12)
    ts = (1000 + (ts.astype(np.int64) - 1000) * 8 // 100).astype(np.uint32)
    return off, items, ts, ids


def _violations(lists, rows, rank, m_index):
    """Python restatement of FlatIndex::viol (srn_avro.cpp): per item, 1 + the highest recency rank of a LISTED session that holds the item but is not in its list
    (0: none), and the number of items that fail the completeness test."""
    listed = set(s for l in lists.values() for s in l)
    viol, bad = {}, 0
    for it, l in lists.items():
        ls = set(l)
        v = [int(rank[s]) for s in listed if it in rows[s] and s not in ls]
        viol[it] = max(v) + 1 if v else 0
        if viol[it] and not (len(l) == m_index and viol[it] <= min(int(rank[s]) for s in l)):
            bad += 1
    return viol, bad


def test_the_loader_infers_the_producers_tie_order():
    """srn_avro.cpp: the recency order among sessions of equal Time is inferred from the producer's list cuts.  (a) ties by larger SessionIndex (prepare_hashmap's
    order): the index is what the TSV builder makes; (b) ties by SMALLER SessionIndex, consistently: a different but equally valid order, every list complete under it;
    (c) ties broken one way on every other item and the other way on the rest, 100 sessions per timestamp: under (Time, SessionIndex) a third of the lists would be
    incomplete; the inferred order explains all cuts but one (two items want two sessions in opposite orders) -- that item is counted and carries FlatIndex::viol."""
    import tempfile
    import serenade_amd as sa
    off, items, ts, ids = _heavily_tied_dataset()
    idf = _idf_like_builder(off, items, 1.0)
    n = len(ts)
    rows = [set(items[off[s]:off[s + 1]].tolist()) for s in range(n)]
    canon = np.empty(n, np.int64); canon[np.lexsort((np.arange(n), ts))] = np.arange(n)
    m_index, max_len = 40, 9
    for name, tb in (("ours", -1), ("reverse", +1), ("mixed", lambda j: +1 if j % 2 == 0 else -1)):
        with tempfile.TemporaryDirectory() as d:
            item_recs, sess_recs, lists = _records(off, items, ts, idf, m_index=m_index, tie_break=tb, max_session_len=max_len)
            _write(d, item_recs, sess_recs)
            ix = sa.VMISIndex.new_from_avro(d, device=-1)
        rank = ix.session_recency()
        kept = np.flatnonzero(rank != 0xFFFFFFFF)
        assert kept.tolist() == sorted(set(s for l in lists.values() for s in l))   # the sessions some list names keep a row and a rank; the others (> max_len items) neither
        assert sorted(rank[kept].tolist()) == list(range(len(kept)))
        by_rank = kept[np.argsort(rank[kept])]
        assert all(ts[a] <= ts[b] for a, b in zip(by_rank[:-1], by_rank[1:]))   # ... ordered by Time; only the order among equal Times is the loader's
        canon = np.full(n, 0xFFFFFFFF, np.int64); canon[kept[np.lexsort((kept, ts[kept]))]] = np.arange(len(kept))
        viol, bad = _violations(lists, rows, rank, m_index)
        assert ix.info["incomplete_items"] == bad, name
        for it in list(lists)[:25]:                                          # the lists are the producer's SETS, most recent first under the index's order
            got, f = ix.postings(it)
            assert sorted(got.tolist()) == sorted(lists[it]) and got.tolist() == sorted(lists[it], key=lambda s: -int(rank[s])) and f == idf[it]
        if name == "ours":
            assert bad == 0 and np.array_equal(rank, canon)
        elif name == "reverse":
            assert bad == 0 and not np.array_equal(rank, canon)
            _, bad_canon = _violations(lists, rows, canon, m_index)
            assert bad_canon > 0, "under (Time, SessionIndex) these lists are not most-recent prefixes: the fixture should need the inferred order"
        else:
            _, bad_canon = _violations(lists, rows, canon, m_index)
            assert 0 < bad <= 3 and bad_canon >= 15, (bad, bad_canon)
        # the flat on-disk format keeps what the loader found
        with tempfile.TemporaryDirectory() as d:
            ix.save(d + "/ix.bin")
            ix2 = sa.VMISIndex.load(d + "/ix.bin", device=-1)
            assert ix2.info["incomplete_items"] == bad and np.array_equal(ix2.session_recency(), rank)


def _check_against_lists_as_given(sa, gix, lists, rows, off, items, ts, idf, qs, k, m, nrec, python_share=4):
    """HIP answers == the canonical closed form over the lists AS GIVEN, recency = the index's own order: by the oracle's restatement of VMISIndex::new
    (orc_index_from_parts) on every query and by the pure-Python statement above on every python_share-th."""
    from oracle import oracle as O
    rank = gix.session_recency()
    n = len(ts)
    kept = np.flatnonzero(rank != 0xFFFFFFFF)
    order = kept[np.argsort(rank[kept])]
    assert all(ts[a] <= ts[b] for a, b in zip(order[:-1], order[1:]))       # the order the product serves with refines Time: only ties are its own
    its = sorted(lists)
    oix = O.OracleIndex.from_parts(its, [lists[i] for i in its], [idf[i] for i in its], [2] * len(its), off, items, ts, tie_rank=rank)
    flat, qo = flatten(qs)
    got_ids, got_sc, got_cnt = sa.predict_batch(gix, qs, k, m, nrec, False)
    ref = oix.predict_batch("canonical", flat, qo, k, m, nrec, False, threads=2)
    assert np.array_equal(got_cnt, ref["counts"]) and np.array_equal(got_ids, ref["ids"])
    np.testing.assert_allclose(got_sc, ref["scores"], rtol=1e-12, atol=0)
    for q in range(0, len(qs), python_share):
        want_ids, want_sc = _canonical_over_given_lists(lists, rows, ts, idf, qs[q], k, m, nrec, rank=rank)
        c = int(got_cnt[q])
        assert c == len(want_ids) and got_ids[q, :c].tolist() == want_ids, (q, qs[q])
        np.testing.assert_allclose(got_sc[q, :c], want_sc, rtol=1e-12, atol=0)
    return got_ids, got_sc, got_cnt


@pytest.mark.gpu
def test_avro_index_with_a_different_tie_break_uses_the_lists_as_given(tmp_path):
    """Timestamps tie and the producer truncated its lists with ANOTHER tie-break than ours: the lists are not most-recent prefixes under (Time, SessionIndex), the load
    must not fail and the answers are those of the lists as given.  Round 6: the loader infers the producer's order among equal timestamps, under which the
    lists ARE complete -- the whole index stays on the fast kernels."""
    import serenade_amd as sa
    off, items, ts, ids = small_dataset(45, n_sessions=600, n_items=40, tied_timestamps=True)
    idf = _idf_like_builder(off, items, 1.0)
    m_index = 12
    item_recs, sess_recs, lists = _records(off, items, ts, idf, m_index=m_index, tie_break=+1)
    _write(tmp_path, item_recs, sess_recs)
    gix = sa.VMISIndex.new_from_avro(tmp_path)
    n = len(ts)
    rows = [set(items[off[s]:off[s + 1]].tolist()) for s in range(n)]
    canon = np.empty(n, np.int64); canon[np.lexsort((np.arange(n), ts))] = np.arange(n)
    assert _violations(lists, rows, canon, m_index)[1] > 0, "the fixture should contain lists that are not most-recent prefixes under our order"
    assert gix.info["incomplete_items"] == 0
    qs = random_queries(7, ids, 300, max_len=4, unknown_rate=0.0)
    _check_against_lists_as_given(sa, gix, lists, rows, off, items, ts, idf, qs, 8, m_index, 10, python_share=2)
    nq, general, _ = gix.last_path_counts()
    assert nq == len(qs) and general == 0


@pytest.mark.gpu
def test_avro_index_of_an_inconsistent_producer_stays_on_the_fast_kernels(tmp_path):
    """VERDICT r5 item 1.  A production index (VMISIndex::new, vmis_index.rs:85-314, lists as given :201-228) whose producer (i) broke timestamp ties the other way on SOME
    items -- no tie order explains all its cuts -- and (ii) kept the sessions longer than its length cut in the session index only (as the CSV path does, :79, :452).
    Until round 5 one such list sent every query of every batch to the general kernel.  Now: answers == the lists as given; the prep kernel flags only the queries an
    incomplete list can reach (PrepHead::unsafe), >= 95 % of the batch is served by the fast kernels, and a single-session call is the one-launch latency path."""
    import serenade_amd as sa
    off, items, ts, ids = _heavily_tied_dataset()
    idf = _idf_like_builder(off, items, 1.0)
    m_index, max_len = 40, 9
    item_recs, sess_recs, lists = _records(off, items, ts, idf, m_index=m_index, tie_break=lambda j: +1 if j % 2 == 0 else -1, max_session_len=max_len)
    _write(tmp_path, item_recs, sess_recs)
    gix = sa.VMISIndex.new_from_avro(tmp_path)
    n = len(ts)
    assert sum(off[s + 1] - off[s] > max_len for s in range(n)) > 100          # (ii): sessions that are in no list
    rows = [set(items[off[s]:off[s + 1]].tolist()) for s in range(n)]
    rank = gix.session_recency()
    viol, bad = _violations(lists, rows, rank, m_index)
    assert gix.info["incomplete_items"] == bad and bad > 0
    qs = random_queries(8, ids, 2000, max_len=4, unknown_rate=0.02)
    # which queries CAN an incomplete list reach?  (srn_prep.h: max viol of the query's known items > x_lo, the most recent m-th entry of its full lists)
    k, m, nrec = 30, m_index, 21
    unsafe = []
    for q in qs:
        xlo = vm = 0
        for it in set(q):
            if it in lists:
                l = sorted((int(rank[s]) for s in lists[it]), reverse=True)
                if len(l) >= m:
                    xlo = max(xlo, l[m - 1])
                vm = max(vm, viol[it])
        unsafe.append(vm > xlo)
    assert 0 < sum(unsafe) <= len(qs) // 20
    _check_against_lists_as_given(sa, gix, lists, rows, off, items, ts, idf, qs, k, m, nrec, python_share=8)
    nq, general, _ = gix.last_path_counts()
    assert nq == len(qs) and sum(unsafe) <= general <= len(qs) // 20, (general, sum(unsafe))   # (>= 95 % on the fast kernels)
    # the same answers with the per-item test switched off (every query through the general kernel's row pass, as until round 5) -- and that IS what SRN_NO_VIOL does
    import os
    ref_rows = sa.predict_batch(gix, qs, k, m, nrec, False)
    from serenade_amd import capi
    os.environ["SRN_NO_VIOL"] = "1"; capi.reload_knobs()
    try:
        old_rows = sa.predict_batch(gix, qs, k, m, nrec, False)
        assert gix.last_path_counts()[1] == len(qs)
    finally:
        del os.environ["SRN_NO_VIOL"]; capi.reload_knobs()
    for x, y in zip(ref_rows, old_rows):
        assert np.array_equal(x, y)
    # single-session calls (srn_predict, the reference's call shape): a safe session is one fused launch, an unsafe one gets the general kernel behind it; both exact
    safe_q = next(q for q, u in zip(qs, unsafe) if not u and all(it in lists for it in q))
    unsafe_q = next(q for q, u in zip(qs, unsafe) if u)
    for q, want_general in ((safe_q, 0), (unsafe_q, 1)):
        got = sa.predict(gix, q, k, m, nrec, False)
        want_ids, want_sc = _canonical_over_given_lists(lists, rows, ts, idf, q, k, m, nrec, rank=rank)
        assert [i for i, _ in got] == want_ids
        np.testing.assert_allclose([x for _, x in got], want_sc, rtol=1e-12, atol=0)
        assert gix.last_path_counts()[:2] == (1, want_general), (q, gix.last_path_counts())


@pytest.mark.gpu
@pytest.mark.parametrize("compressor", ["pyarrow", "copies"])
def test_avro_index_predicts_what_the_oracle_predicts(tmp_path, compressor):
    """VMISIndex::new(base_path) (vmis_index.rs:85-314) on files compressed by a third-party snappy (pyarrow) -> HIP predictions == the CPU ORACLE's
    (prepare_hashmap + canonical predict on the same sessions, real product flags: mod.rs:162-182), not another HIP index's."""
    import serenade_amd as sa
    from oracle import oracle as O
    off, items, ts, ids = small_dataset(43, n_sessions=5000, n_items=400, tied_timestamps=True)
    idf = _idf_like_builder(off, items, 2.0)
    attrs = {int(i): (bool(j % 3), bool(j % 5 == 0)) for j, i in enumerate(ids)}
    _write_index(str(tmp_path), off, items, ts, 150, idf, attrs, "snappy", compressor=pyarrow_snappy if compressor == "pyarrow" else AW.snappy_with_copies)
    a = sa.VMISIndex.new_from_avro(tmp_path)
    flags = [(1 if ad else 0) | (2 if fs else 0) for fs, ad in attrs.values()]
    oix = O.OracleIndex(off, items, ts, 150, 10**6, 2.0, fast=True)
    oix.set_attributes(list(attrs), flags)
    qs = random_queries(6, ids, 400, max_len=6)
    flat, qo = flatten(qs)
    for business in (False, True):
        ids_a, sc_a, cnt_a = sa.predict_batch(a, qs, 80, 150, 21, business)
        ref = oix.predict_batch("canonical", flat, qo, 80, 150, 21, business, threads=2)
        assert np.array_equal(cnt_a, ref["counts"]) and np.array_equal(ids_a, ref["ids"]), business
        np.testing.assert_allclose(sc_a, ref["scores"], rtol=1e-12, atol=0)          # (the files' idf is numpy's log, the oracle's is libm's)
    # and, as before, bit-identical to the HIP index built from the same sessions (idf from the same doubles)
    b = sa.VMISIndex.from_sessions(off, items, ts, 150, 10**6, 2.0)
    b.set_attributes(list(attrs), flags)
    for business in (False, True):
        for x, y in zip(sa.predict_batch(a, qs, 80, 150, 21, business), sa.predict_batch(b, qs, 80, 150, 21, business)):
            assert np.array_equal(x, y)
