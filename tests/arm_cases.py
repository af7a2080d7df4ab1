"""Designed keys for the traffic split's rule.  mix64 is a bijection and so is s -> s * 0xD1B54A32D192ED03 + 1 (an odd multiplier), so the rule
    u = mix64(rkey ^ (fold(key) * MUL + 1)) >> 32,   fold(key) = mix64(key_hi ^ FOLD) ^ key_lo,   rkey = mix64(seed ^ DOMAIN)
can be inverted: for a chosen key_hi (any 64-bit value) and a chosen u there is a key_lo whose key draws exactly u -- one for each value of the draw's low 32 bits.
Everything here is Python integers, independent of the NumPy statement in serenade_amd.serving (arms_model), which the tests compare against."""
import numpy as np

M64 = (1 << 64) - 1
FOLD, DOMAIN, MUL = 0x9E3779B97F4A7C15, 0x53524E5F41524D53, 0xD1B54A32D192ED03
C1, C2 = 0xff51afd7ed558ccd, 0xc4ceb9fe1a85ec53
C1_INV, C2_INV, MUL_INV = pow(C1, -1, 1 << 64), pow(C2, -1, 1 << 64), pow(MUL, -1, 1 << 64)

WEIGHT_SETS = ([1, 1], [9, 1], [1, 0, 1], [0, 0, 5], [5, 0, 0], [1] * 16, [2 ** 32 - 2, 1])
HIS = (0, 1, 0x8000000000000000, M64, 0x0123456789ABCDEF)          # chosen key_hi values, full 64-bit ones included


def mix64(x):
    x ^= x >> 33
    x = x * C1 & M64
    x ^= x >> 33
    x = x * C2 & M64
    return x ^ (x >> 33)


def unmix64(y):
    """mix64's inverse: x ^= x >> 33 undoes itself (2 * 33 > 64), the multipliers are odd."""
    y ^= y >> 33
    y = y * C2_INV & M64
    y ^= y >> 33
    y = y * C1_INV & M64
    return y ^ (y >> 33)


def draw(seed, hi, lo):
    """the rule's u for one key, in Python integers"""
    fold = mix64(hi ^ FOLD) ^ lo
    return mix64(mix64((seed ^ DOMAIN) & M64) ^ ((fold * MUL + 1) & M64)) >> 32


def thresholds(weights):
    """T_a, a = 0 .. A-1 (the last is 2^32)"""
    W, cum, out = sum(weights), 0, []
    for w in weights:
        cum += w
        out.append((cum << 32) // W)
    return out


def arm_of_draw(weights, u):
    return sum(1 for T in thresholds(weights)[:-1] if T <= u)


def lo_for(seed, hi, u, low=0):
    """the key_lo whose key (hi, lo) draws exactly u under `seed`; low: the 32 bits the rule shifts out"""
    fold = ((unmix64((u << 32) | low) ^ mix64((seed ^ DOMAIN) & M64)) - 1) * MUL_INV & M64
    return fold ^ mix64(hi ^ FOLD)


def threshold_keys(seed, weights, his=HIS):
    """-> (hi, lo) uint64 arrays, u list, arm uint8: for every threshold T of the weights and every chosen hi the keys that draw T - 1, T, 0 and 2^32 - 1 (those
    that exist: u is in 0 .. 2^32 - 1), plus keys equal in hi alone and in lo alone"""
    us = {0, 2 ** 32 - 1}
    for T in thresholds(weights)[:-1]:
        us.update(u for u in (T - 1, T) if 0 <= u < 2 ** 32)
    hi, lo, u_out = [], [], []
    for i, h in enumerate(his):
        for u in sorted(us):
            hi.append(h), lo.append(lo_for(seed, h, u, low=i)), u_out.append(u)
    # equal in hi alone: the same hi, another lo (whatever it draws); equal in lo alone: the same lo under another hi
    for h, l in list(zip(hi, lo))[:8]:
        hi.append(h), lo.append(l ^ 1), u_out.append(draw(seed, h, l ^ 1))
        hi.append(h ^ 1), lo.append(l), u_out.append(draw(seed, h ^ 1, l))
    arm = np.array([arm_of_draw(weights, u) for u in u_out], np.uint8)
    return (np.array(hi, np.uint64), np.array(lo, np.uint64)), u_out, arm


def rekey(seed, weights, keys, arms):
    """Keys for a request sequence whose arms are prescribed position by position: request i of visitor keys[i] gets the key of the visitor (keys[i], arms[i]) --
    an original visitor whose requests fall into several arms becomes one visitor per arm -- designed to draw a u inside arm arms[i]'s interval.  The same
    (visitor, arm) gives the same key, distinct ones distinct keys (checked).  Every prescribed arm must have a positive weight."""
    T = [0] + thresholds(weights)
    hi_in, lo_in = (np.asarray(a, np.uint64) for a in keys)
    made, hi, lo = {}, [], []
    for h, l, a in zip(hi_in.tolist(), lo_in.tolist(), np.asarray(arms).tolist()):
        if (h, l, a) not in made:
            width = T[a + 1] - T[a]
            assert width > 0, "arm %d has weight 0" % a
            nh = (mix64(h ^ mix64(l)) + a) & M64
            made[(h, l, a)] = (nh, lo_for(seed, nh, T[a] + mix64(nh) % width, low=len(made) & 0xFFFFFFFF))
        hi.append(made[(h, l, a)][0]), lo.append(made[(h, l, a)][1])
    assert len(set(made.values())) == len(made)
    return np.array(hi, np.uint64), np.array(lo, np.uint64)


def sequences(n, n_arms):
    """the prescribed arm sequences over n requests and arms 0 .. n_arms - 1 -> {name: uint8[n]}"""
    i = np.arange(n)
    out = {"alternating": (i % n_arms).astype(np.uint8)}
    for run in (63, 64, 65):
        out["runs_of_%d" % run] = ((i // run) % n_arms).astype(np.uint8)
    return out
