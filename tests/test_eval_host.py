"""Offline evaluation and hyper-parameter search: what runs without a GPU -- the ABI's symbols and refusals, the trial generators, the index
plan and the configuration reader."""
import ctypes as C
import os

import numpy as np
import pytest

from serenade_amd import capi, evaluation, hpo

EVAL_SYMBOLS = ("srn_eval_set_create", "srn_eval_set_from_tsv", "srn_evaluate", "srn_eval_set_free", "srn_debug_eval_terms")


def _trial(**kw):
    t = dict(k=50, m=500, how_many=20, max_items_in_session=2, length=20)
    t.update(kw)
    return evaluation._trial(t)


def test_eval_symbols_are_exported_and_bound():
    L = capi.lib()
    for name in EVAL_SYMBOLS:
        assert name in capi.SYMBOLS
        fn = getattr(L, name)
        assert fn.argtypes == capi.SYMBOLS[name][1]
    assert C.sizeof(capi.EvalTrial) == 32
    assert C.sizeof(capi.EvalResult) == 8 + 14 * 8 + 2 * 8 + 2 * 8


def test_eval_set_on_a_host_only_index_is_enodev():
    from serenade_amd import VMISIndex
    ix = VMISIndex.from_sessions(np.array([0, 2, 4], np.uint64), np.array([1, 2, 2, 3], np.uint64), np.array([1, 2], np.uint32), 10, 10, 1.0, device=-1)
    with pytest.raises(capi.SerenadeError) as e:
        evaluation.EvalSet(ix, {1: [1, 2, 3]}, [1, 2, 2, 3])
    assert e.value.code == capi.SRN_ENODEV
    h = C.c_void_p()
    assert capi.lib().srn_eval_set_from_tsv(ix._h, b"test.txt", b"train.txt", C.byref(h)) == capi.SRN_ENODEV


def test_over_long_window_and_length_are_refused_before_anything_runs():
    L = capi.lib()
    r = capi.EvalResult()
    for t, code in ((_trial(max_items_in_session=capi.MAX_SESSION_LEN + 1), capi.SRN_ERANGE), (_trial(length=capi.MAX_HOW_MANY + 1), capi.SRN_ERANGE),
                    (_trial(how_many=capi.MAX_HOW_MANY + 1), capi.SRN_ERANGE), (_trial(max_items_in_session=0), capi.SRN_EINVAL),
                    (_trial(length=0), capi.SRN_EINVAL), (_trial(k=0), capi.SRN_EINVAL)):
        assert L.srn_evaluate(None, C.byref(t), 1, C.byref(r), None) == code
    # a good trial gets as far as the missing set
    assert L.srn_evaluate(None, C.byref(_trial()), 1, C.byref(r), None) == capi.SRN_EINVAL
    with pytest.raises(capi.SerenadeError) as e:
        evaluation.evaluate(None, [dict(k=50, m=500, max_items_in_session=300)])
    assert e.value.code == capi.SRN_ERANGE


def test_exhaustive_grid_is_the_reference_grid_in_its_loop_order():
    trials = hpo.exhaustive()
    assert len(trials) == 4 * 5 * 6 * 6 == 720
    assert trials[0] == dict(m=100, k=50, max_items_in_session=1, idf_weighting=1)
    assert trials[1] == dict(m=100, k=50, max_items_in_session=1, idf_weighting=2)        # idf innermost
    assert trials[6] == dict(m=100, k=50, max_items_in_session=2, idf_weighting=1)        # then the window
    assert trials[36] == dict(m=100, k=100, max_items_in_session=1, idf_weighting=1)      # then k
    assert trials[180] == dict(m=500, k=50, max_items_in_session=1, idf_weighting=1)      # m outermost
    assert trials[-1] == dict(m=2500, k=1500, max_items_in_session=10, idf_weighting=10)
    assert len({tuple(sorted(t.items())) for t in trials}) == 720


def test_random_combinations_are_distinct_and_seeded():
    a, b, c = hpo.random(hpo.RANDOM_GRID, 150, seed=7), hpo.random(hpo.RANDOM_GRID, 150, seed=7), hpo.random(hpo.RANDOM_GRID, 150, seed=8)
    assert a == b and a != c
    assert len(a) == 150 and len({tuple(sorted(t.items())) for t in a}) == 150
    grid = hpo.RANDOM_GRID
    assert all(t[k] in grid[k] for t in a for k in grid)
    kept = hpo.random(hpo.RANDOM_GRID, 150, seed=7, k_le_m=True)
    assert kept == [t for t in a if t["k"] <= t["m"]] and len(kept) < 150
    assert len(hpo.random({"m": [1, 2], "k": [1], "max_items_in_session": [1], "idf_weighting": [1]}, 10, seed=1)) == 2


def test_index_plan_is_one_index_per_idf_weighting_at_its_largest_m():
    assert hpo.index_plan(hpo.exhaustive()) == {float(w): 2500 for w in (1, 2, 3, 5, 7, 10)}
    trials = [dict(m=100, k=5, max_items_in_session=1, idf_weighting=1), dict(m=500, k=5, max_items_in_session=2, idf_weighting=1),
              dict(m=300, k=5, max_items_in_session=1, idf_weighting=0)]
    assert hpo.index_plan(trials) == {1.0: 500, 0.0: 300}


def test_cli_reads_the_example_configuration(tmp_path):
    p = tmp_path / "example.toml"
    p.write_text('config_type = "toml"\n\n[server]\nhost = "0.0.0.0"\nport = 8080\n\n[data]\ntraining_data_path="train.txt"\n\n'
                 '[model]\nm_most_recent_sessions = 500\nneighborhood_size_k = 50\n\n[logic]\nenable_business_logic = true\n\n'
                 '[hyperparam]\ntraining_data_path = "train.txt"\ntest_data_path = "test.txt"\nvalidation_data_path = "valid.txt"\n'
                 'num_iterations = 15\nsave_records = true\nout_path = "results.csv"  # the records\nenable_business_logic = true\n'
                 'n_most_recent_sessions_range = [100, 2500]\nidf_weighting_range = [0, 5]\n')
    cfg = hpo.hyperparam_config(str(p))
    assert cfg == {"training_data_path": "train.txt", "test_data_path": "test.txt", "save_records": True, "out_path": "results.csv",
                   "enable_business_logic": True}
    assert hpo.read_toml(str(p))["model.neighborhood_size_k"] == "50"


def test_goal_values_print_as_rust_does():
    assert hpo.rust_f64(0.3401) == "0.3401"
    assert hpo.rust_f64(1.0) == "1" and hpo.rust_f64(0.0) == "0"
    assert hpo.rust_f64(1e-7) == "0.0000001"
    assert hpo.rust_f64(0.1 + 0.2) == "0.30000000000000004"
    assert hpo.rust_f64(float("-inf")) == "-inf"


def test_synthetic_test_sessions_rebuild_the_query_stream():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import helpers
    from serenade_amd import synth
    ts = synth.test_sessions(2000, 20000)
    qi, qo, nx = synth.queries(2000, 20000, max_items=4, with_next=True)
    qs = helpers.evaluator_queries(ts, 4)
    flat, off = helpers.flatten([q for q, _ in qs])
    assert np.array_equal(flat, qi) and np.array_equal(off, qo)
    assert np.array_equal(np.array([n[0] for _, n in qs], np.uint64), nx)
