"""A numpy model of the MSM sort's ranking rule (halo_amd/csrc/sort.hip, k_rs_scatter).

The sort is LSD: pass p orders by digit p of the key and must leave the array ordered by the key's
low shift + bits bits.  k_rs_scatter gives every wave a slice of consecutive entries (1024 in an 8-bit
pass, 896 in a 9-bit one); the output of a pass lists, per digit, the slices in order and within a slice
the wave's ranking.  A wave ranks stably, except where all entries of its slice agree in the bits
already sorted: there it ranks equal digits in arrival order, any order.  The model permutes such
(slice, digit) groups at random and checks that the result is still sorted by key with the (key, value)
pairs preserved -- for two- and three-pass plans, 8- and 9-bit passes, random and skewed keys and an
entry count that is no multiple of the tile.  A negative control applies the same permutation to a
slice that is not uniform and must come out unsorted: the check can fail.
"""
import numpy as np
import pytest

SLICE = {8: 1024, 9: 896}  # entries per wave of a pass of that many bits (a tile is 8 slices)


def plan_of(key_bits, fused=False):
    """sort.hip rs_plan: (shift, bits) per pass."""
    if key_bits == 17 or (key_bits == 18 and not fused):
        b0 = 9 if key_bits == 18 else 8
        return [(0, b0), (b0, key_bits - b0)]
    return [(8 * p, 8) for p in range(max(1, (key_bits + 7) // 8))]


def model_sort(keys, vals, plan, rng, force_any_order=False, full_slices_only=False):
    """-> keys, vals, number of slices ranked in any order in the passes after the first."""
    keys, vals = keys.copy(), vals.copy()
    n = len(keys)
    free = 0
    for shift, bits in plan:
        digit = (keys >> shift) & ((1 << bits) - 1)
        low = keys & ((1 << shift) - 1)
        order = np.arange(n)
        L = SLICE[bits]
        for a in range(0, n, L):
            b = min(n, a + L)
            uniform = bool((low[a:b] == low[a]).all()) and not (full_slices_only and b - a < L)
            if not (uniform or force_any_order):
                continue
            free += shift > 0
            d = digit[a:b]
            for v in np.unique(d):
                idx = a + np.flatnonzero(d == v)
                order[idx] = rng.permutation(idx)
        # per digit: the slices in order, within a slice the wave's ranking
        order = order[np.argsort(digit[order], kind="stable")]
        keys, vals = keys[order], vals[order]
    return keys, vals, free


def pairs(keys, vals):
    return np.sort(keys.astype(np.uint64) << np.uint64(32) | vals.astype(np.uint64))


def make_keys(kind, key_bits, n, rng):
    if kind == "random":
        return rng.integers(0, 1 << key_bits, n, dtype=np.uint32)
    if kind == "few_low":  # a handful of low-digit values: long runs, uniform slices and run boundaries
        lowbits = 9 if key_bits == 18 else 8
        low = rng.choice(rng.integers(0, 1 << lowbits, 5), n)
        return ((rng.integers(0, 1 << (key_bits - lowbits), n) << lowbits) | low).astype(np.uint32)
    if kind == "geometric":  # most entries in a few buckets
        return np.minimum(rng.geometric(0.002, n), (1 << key_bits) - 1).astype(np.uint32)
    if kind == "one_key":
        return np.full(n, (1 << key_bits) - 3, dtype=np.uint32)
    raise ValueError(kind)


@pytest.mark.parametrize("full_slices_only", (False, True))
@pytest.mark.parametrize("kind", ("random", "few_low", "geometric", "one_key"))
@pytest.mark.parametrize("key_bits,fused", ((16, False), (17, False), (18, False), (18, True)))
def test_any_order_in_uniform_slices_keeps_the_sort(key_bits, fused, kind, full_slices_only):
    rng = np.random.default_rng(key_bits * 100 + fused)
    n = 5 * 8192 + 8 * 896 + 333  # no multiple of either tile, a partial last slice
    keys = make_keys(kind, key_bits, n, rng)
    vals = np.arange(n, dtype=np.uint32)
    plan = plan_of(key_bits, fused)
    assert len(plan) == (3 if (key_bits, fused) == (18, True) else 2)
    k, v, free = model_sort(keys, vals, plan, rng, full_slices_only=full_slices_only)
    assert (np.diff(k.astype(np.int64)) >= 0).all()
    assert np.array_equal(pairs(k, v), pairs(keys, vals))
    assert np.array_equal(keys[v], k)  # every value still beside its key
    if kind in ("few_low", "one_key"):
        assert free > 0  # the rule under test was exercised
    if kind == "few_low":
        assert free < (len(plan) - 1) * (n // 896 + 1)  # ... and so was the stable ranking


def test_any_order_in_a_mixed_slice_breaks_the_sort():
    """Negative control: one slice, one second-pass digit, two values of the low byte."""
    rng = np.random.default_rng(7)
    keys = np.array([0x0100] * 500 + [0x0101] * 524, dtype=np.uint32)
    vals = np.arange(len(keys), dtype=np.uint32)
    plan = plan_of(16)
    k, v, free = model_sort(keys, vals, plan, rng)
    assert free == 0 and (np.diff(k.astype(np.int64)) >= 0).all()
    k, v, _ = model_sort(keys, vals, plan, rng, force_any_order=True)
    assert np.array_equal(pairs(k, v), pairs(keys, vals))
    assert not (np.diff(k.astype(np.int64)) >= 0).all()
