"""wave_class_counts (srn_device.h): the k-cut's wave-wide class counts on the matrix unit, through srn_debug_class_counts.

A lane holds sixteen 4-bit counts in one 64-bit word (field c = class c); the helper returns, per wave, the sum over its 64 lanes of every field.  Integers: the
comparison with numpy is exact.  The cases catch a wrong lane-to-class or byte-to-class map of the MFMA operands (the two one-hot forms, single lanes), a partial sum
that leaves its byte (all fields 6: 384 per class; all fields 15: 60 per stage-1 partial, 960 per class), and the padding of a partly filled workgroup (9 waves)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_WAVES = [1, 8, 9]   # 8 = one whole workgroup of 512 threads, 9 = a second, partly filled one


def _pack(fields):
    """fields [n_waves, 64, 16] of 0..15 -> acc words [n_waves * 64]"""
    f = np.asarray(fields, np.uint64)
    assert f.max(initial=0) <= 15
    acc = np.zeros(f.shape[:2], np.uint64)
    for c in range(16):
        acc |= f[:, :, c] << np.uint64(4 * c)
    return np.ascontiguousarray(acc.reshape(-1))


def _gpu_counts(fields):
    from serenade_amd import capi
    fields = np.asarray(fields)
    n_waves = fields.shape[0]
    acc = _pack(fields)
    out = np.full(n_waves * 16, 0xDEADBEEF, np.uint32)
    capi.check(capi.lib().srn_debug_class_counts(C.c_void_p(acc.ctypes.data), n_waves, C.c_void_p(out.ctypes.data), 0))
    return out.reshape(n_waves, 16)


def _check(fields):
    fields = np.asarray(fields, np.uint32)
    want = fields.sum(axis=1, dtype=np.uint32)        # [n_waves, 16]
    got = _gpu_counts(fields)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())


@pytest.mark.parametrize("n_waves", N_WAVES)
@pytest.mark.parametrize("value", [0, 6, 15])
def test_constant_fields(n_waves, value):
    _check(np.full((n_waves, 64, 16), value, np.uint32))


@pytest.mark.parametrize("n_waves", N_WAVES)
def test_one_hot_lane_and_15(n_waves):
    """lane l counts 1 in class l & 15 only: 4 per class"""
    f = np.zeros((n_waves, 64, 16), np.uint32)
    lanes = np.arange(64)
    f[:, lanes, lanes & 15] = 1
    _check(f)


@pytest.mark.parametrize("n_waves", N_WAVES)
def test_one_hot_lane_shr_2(n_waves):
    """lane l counts 1 in class l >> 2 only: 4 per class, from four neighbouring lanes"""
    f = np.zeros((n_waves, 64, 16), np.uint32)
    lanes = np.arange(64)
    f[:, lanes, lanes >> 2] = 1
    _check(f)


@pytest.mark.parametrize("n_waves", N_WAVES)
@pytest.mark.parametrize("lane", [0, 15, 16, 47, 63])
def test_single_lane(n_waves, lane):
    """one lane with sixteen different counts (wave w: rotated by w), every other lane 0"""
    f = np.zeros((n_waves, 64, 16), np.uint32)
    for w in range(n_waves):
        f[w, lane, :] = (np.arange(16) + w) % 16
    _check(f)


@pytest.mark.parametrize("n_waves", N_WAVES)
@pytest.mark.parametrize("top", [6, 15])
def test_random_fields(n_waves, top):
    rng = np.random.default_rng(1000 * top + n_waves)
    _check(rng.integers(0, top + 1, size=(n_waves, 64, 16)))
