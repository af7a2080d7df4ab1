"""merge_pair (srn_fast.hip): the fast kernel's merge of two adjacent descending runs, alone, through srn_debug_merge_pair.

One 512-thread workgroup holds the lean form's merge room (12 032 words): the runs lie in the lower half, A = in[sa, sa + la) and B = in[sa + la, sa + la + lb), and a team
of 2^lg threads writes their merge to out[sa, sa + la + lb) in the upper half.  All values are distinct and none is 0, as in the kernel (a staged slot carries its list bit).
The reference is numpy's descending sort of the two runs' union: integers, compared exactly.  Per case three things are checked: the merged range, the canary everywhere
else in the output half, and the input half word for word.  The words of the input half outside the runs hold 0xFFFFFFFF: the merge loop may look one word past a run and
must not use what it finds there, and the largest value is the one a compare or a max would let through.

Shapes: an empty run on either side, single entries, a total of one wave's worth of single outputs (64 + 64), one past a team boundary (513), a run of one against a
long one on either side, and the largest pair the lean form admits (3 006 + 3 006).  Patterns: all of A above all of B, all of B above all of A, strictly alternating,
seeded random.  Every case runs at the team size merge_team gives and at one size either side of it (the thread's share g = ceil(total / 2^lg) | 1 covers the total at
any lg), at sa = 0 and at sa = 3 with the filler in front of the runs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOM = 12032
HALF = ROOM // 2
CANARY = 0xCA11AB1E
FILLER = 0xFFFFFFFF
MERGE_G = 8

SHAPES = [(0, 1), (1, 0), (1, 1), (0, 700), (700, 0), (63, 1), (1, 63), (64, 64), (33, 480), (2047, 1), (1, 2047), (1500, 1500), (3006, 3006)]
PATTERNS = ["a_above", "b_above", "alternating", "random"]


def merge_team(total):
    """log2 of the team size (srn_fast.hip): 64 .. 512 threads, >= total / 8"""
    want = (total + MERGE_G - 1) // MERGE_G
    return 6 if want <= 64 else 7 if want <= 128 else 8 if want <= 256 else 9


def _values(rng, n):
    """n distinct values, descending: the value 1, the value 0xFFFFFFFE and steps of random width between them (about half have bit 31 set)"""
    if n == 1:
        return np.array([1], np.uint32)
    width = (2 ** 32 - 4) // n
    v = 1 + np.concatenate([[0], np.cumsum(rng.integers(1, width + 1, size=n - 1, dtype=np.int64))])
    v[-1] = 0xFFFFFFFE
    assert v[-2] < v[-1] and (np.diff(v) > 0).all()
    return v[::-1].astype(np.uint32)


def _runs(pattern, la, lb, seed):
    rng = np.random.default_rng(seed)
    u = _values(rng, la + lb)
    to_a = np.zeros(la + lb, bool)
    if pattern == "a_above":
        to_a[:la] = True
    elif pattern == "b_above":
        to_a[lb:] = True
    elif pattern == "alternating":      # A, B, A, B ... while both last, the rest to the longer run
        both = 2 * min(la, lb)
        to_a[:both:2] = True
        to_a[both:] = la > lb
    else:
        to_a[rng.choice(la + lb, size=la, replace=False)] = True
    a, b = u[to_a], u[~to_a]
    assert len(a) == la and len(b) == lb
    if la + lb > 1:
        assert int(u[0]) >> 31 == 1 and int(u[-1]) == 1
    return a, b


def _merge(pairs):
    """pairs: (sa, A, B, lg, reversed) -> the room before and after the call"""
    from serenade_amd import capi
    room = np.empty(ROOM, np.uint32)
    room[:HALF] = FILLER
    room[HALF:] = CANARY
    desc = []
    for sa, a, b, lg, rev in pairs:
        room[sa:sa + len(a)] = a
        room[sa + len(a):sa + len(a) + len(b)] = b
        desc += [sa, len(a), len(b), lg, int(rev)]
    before = room.copy()
    desc = np.array(desc, np.uint32)
    capi.check(capi.lib().srn_debug_merge_pair(C.c_void_p(room.ctypes.data), C.c_void_p(desc.ctypes.data), len(pairs), 0))
    return before, room


def _check(pairs):
    before, after = _merge(pairs)
    want = before[HALF:].copy()
    for sa, a, b, _lg, _rev in pairs:
        want[sa:sa + len(a) + len(b)] = np.sort(np.concatenate([a, b]))[::-1]
    got = after[HALF:]
    for sa, a, b, lg, rev in pairs:
        n = len(a) + len(b)
        bad = np.flatnonzero(got[sa:sa + n] != want[sa:sa + n])
        assert bad.size == 0, "la %d lb %d sa %d lg %d reversed %d: %d outputs differ, the first at %d" % (len(a), len(b), sa, lg, rev, bad.size, bad[0])
    assert np.array_equal(got, want), "the output half was written outside the merged ranges"
    assert np.array_equal(after[:HALF], before[:HALF]), "the input half changed"


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("la,lb", SHAPES)
def test_merge_pair(la, lb, pattern):
    lg0 = merge_team(la + lb)
    for sa in (0, 3):
        a, b = _runs(pattern, la, lb, 1000 * la + lb + sa)
        for lg in (lg0 - 1, lg0, lg0 + 1):
            if 6 <= lg <= 9:
                _check([(sa, a, b, lg, False)])
                _check([(sa, a, b, lg, True)])


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("first,second", [((200, 150), (33, 300)), ((1500, 1200), (1300, 1400))], ids=["teams_of_64", "teams_of_512"])
def test_two_pairs_in_one_launch(first, second, pattern):
    """Level 0 of a four-list query: the second pair's team counts from thread 511 down and no barrier separates the two merges.  Teams of 64: waves 0 and 7, one pair
    each; teams of 512: every wave merges the first pair, then the second."""
    a1, b1 = _runs(pattern, first[0], first[1], 7)
    a2, b2 = _runs(pattern, second[0], second[1], 8)
    lg1, lg2 = merge_team(sum(first)), merge_team(sum(second))
    assert lg1 == lg2 == (6 if sum(first) <= 512 else 9)
    _check([(0, a1, b1, lg1, False), (sum(first), a2, b2, lg2, True)])
