"""GPU: the MSM sort's two rankings and the three recodings, through whole MSMs.

k_rs_scatter ranks a wave's slice stably (ballots) unless the slice is uniform in the bits already
sorted, where it ranks with one returning LDS add per entry; the fused first pass recodes the scalars
with a constant window width (c = 16, 17) or a run-time one.  Over a synthetic SRS of 2^16 points
(G_j = k_j G, halo_srs_synthesize) with full window-shifted sets of width 17 (constant-width recoding,
8 + 8-bit passes), 16 (constant-width) and 19 (run-time recoding, three passes), every MSM is checked
against (sum_j s_j k_j) G from the known logs.  An MSM has about 2^20 entries, so a low-byte value
spans about 4000 of them: slices that are uniform and slices across a boundary between two low-byte
values occur in one launch.  The constructed scalars force one path: digits with low byte 0 make the
whole second pass rank with the LDS add over all high bytes, digits with one high byte put the whole
second pass on one LDS counter per wave.  Their digits lie in [1, 2^(c-1) - 1], so no carry arises and
the scalar is sum_w d_w 2^(c w) < p / 2.  The pair MSMs of an IPA opening (keys of 17 bits: an 8-bit
and a 9-bit pass) are compared with the same opening over the SRS's default-width copies.
"""
import random

import numpy as np
import pytest

import pasta as P
from halo_amd import group, pcdl

pytestmark = pytest.mark.gpu

N = 1 << 16
SEED = 0x52414E4B
WIDTHS = (17, 16, 19)


def synth_scalars_np(seed: int, n: int) -> np.ndarray:
    """numpy restatement of halo_synth_scalar (splitmix64 stream per index; top word masked)."""
    j = np.arange(n, dtype=np.uint64)
    st = np.uint64(seed) ^ (j * np.uint64(0xD1B54A32D192ED03))
    out = np.zeros((n, 4), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for i in range(4):
            st = st + np.uint64(0x9E3779B97F4A7C15)
            z = st.copy()
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            out[:, i] = z ^ (z >> np.uint64(31))
    out[:, 3] &= np.uint64(0x1FFFFFFFFFFFFFFF)
    zero = (out == 0).all(axis=1)
    out[zero, 0] = 1
    return out


def ints_of(limbs: np.ndarray) -> list:
    b = np.ascontiguousarray(limbs, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[32 * j:32 * j + 32], "little") for j in range(len(limbs))]


def mont(canon: list, r: int) -> np.ndarray:
    """canonical integers -> ark Montgomery limbs"""
    R = (1 << 256) % r
    b = b"".join((v * R % r).to_bytes(32, "little") for v in canon)
    return np.ascontiguousarray(np.frombuffer(b, dtype=np.uint64).reshape(-1, 4))


def windows(c):
    return (255 + c - 1) // c


def from_digits(digits: np.ndarray, c: int) -> list:
    """digits (n, W) of at most 31 bits, each < 2^c -> sum_w d_w 2^(c w), as 4 x u64 limbs -> integers"""
    n, W = digits.shape
    limbs = np.zeros((n, 5), dtype=np.uint64)
    for w in range(W):
        d = digits[:, w].astype(np.uint64)
        q, s = divmod(c * w, 64)
        with np.errstate(over="ignore"):
            limbs[:, q] |= d << np.uint64(s)
        if s + c > 64:
            limbs[:, q + 1] |= d >> np.uint64(64 - s)
    assert not limbs[:, 4].any()
    return ints_of(limbs[:, :4])


@pytest.fixture(scope="module")
def logs():
    return ints_of(synth_scalars_np(SEED, N))


@pytest.fixture(scope="module")
def plain_cases(logs):
    """name -> (ark scalars, expected WrappedPoint): the cases that do not depend on the width."""
    c = P.PALLAS
    r = c.scalar
    rng = random.Random(1)
    nprng = np.random.default_rng(2)
    cases = {}
    cases["random"] = [rng.randrange(r) for _ in range(N)]
    cases["partial_tile"] = [rng.randrange(r) for _ in range(N - 37)]
    cases["all_equal"] = [r - 424242] * N
    cases["two_values"] = [r - 99] * (N // 2) + [(1 << 201) + 3] * (N // 2)
    sparse = [0] * N
    for j in nprng.choice(N, size=N // 64, replace=False):
        sparse[int(j)] = rng.randrange(1, r)
    cases["one_in_64"] = sparse
    return {name: (mont(s, r), expected(s, logs)) for name, s in cases.items()}


def expected(canon, logs):
    c = P.PALLAS
    acc = sum(s * k for s, k in zip(canon, logs)) % c.scalar
    return P.point_to_wrapped(c, P.mul_fast(c, acc, c.generator))


def constructed(c_s, kind):
    """Scalars from chosen digits in [1, 2^(c-1) - 1] (0 in the top window of `one_high_byte`)."""
    W = windows(c_s)
    rng = np.random.default_rng(c_s * 10 + len(kind))
    top = 1 << (253 - (W - 1) * c_s)  # the top digit stays below this, so the scalar stays below 2^253 < p / 2
    d = np.zeros((N, W), dtype=np.uint64)
    if kind == "low_byte_zero":  # d = 256 h + 1: entry key |d| - 1 = 256 h
        hmax = (1 << (c_s - 1)) // 256 - 1
        d[:, : W - 1] = 256 * rng.integers(0, hmax + 1, size=(N, W - 1), dtype=np.uint64) + 1
        d[:, W - 1] = 256 * rng.integers(0, max(1, (top - 2) // 256 + 1), size=N, dtype=np.uint64) + 1
        assert (d[:, W - 1] < top).all()
    else:  # one_high_byte: key = 256 + random low byte
        d[:, : W - 1] = 256 + rng.integers(0, 256, size=(N, W - 1), dtype=np.uint64) + 1
    assert (d[:, : W - 1] >= 1).all() and (d < (1 << (c_s - 1))).all()
    return from_digits(d, c_s)


@pytest.fixture(scope="module", params=WIDTHS)
def shifted_srs(request, hal):
    c_s = request.param
    L = hal.load()
    group.PublicParams.synthesize("pallas", N, SEED, precompute_windows=False)
    hal.check(L.halo_srs_precompute_window_range(0, c_s, 0, 0))
    assert L.halo_srs_window_bits(0) == c_s
    return c_s


@pytest.mark.parametrize("name", ("random", "partial_tile", "all_equal", "two_values", "one_in_64"))
def test_msm_over_shifted_set(hal, shifted_srs, plain_cases, name):
    sc, exp = plain_cases[name]
    assert hal.load().halo_srs_window_bits(0) == shifted_srs and group.PublicParams.len("pallas") == N
    got = pcdl.commit(sc, N - 1, None, "pallas")
    assert list(got) == exp, (shifted_srs, name)


@pytest.mark.parametrize("kind", ("low_byte_zero", "one_high_byte"))
def test_msm_constructed_digits(hal, shifted_srs, logs, kind):
    canon = constructed(shifted_srs, kind)
    assert max(canon) < (P.PALLAS.scalar - 1) // 2
    assert hal.load().halo_srs_window_bits(0) == shifted_srs and group.PublicParams.len("pallas") == N
    got = pcdl.commit(mont(canon, P.PALLAS.scalar), N - 1, None, "pallas")
    assert list(got) == expected(canon, logs), (shifted_srs, kind)


def test_ipa_pair_msm_c17_equals_default_width(hal):
    """The weighted rounds' L / R pair MSMs over c = 17 copies sort 17-bit keys (an 8-bit fused first
    pass, a 9-bit second pass): the opening's L, R, U, c equal those over the default-width copies."""
    c = P.PALLAS
    r = c.scalar
    n = 1 << 14
    L = hal.load()
    rng = random.Random(17)
    cs = mont([rng.randrange(r) for _ in range(n)], r)
    zz = mont([rng.randrange(r)], r)
    Hw = np.array(P.point_to_wrapped(c, P.mul_fast(c, rng.randrange(1, r), c.generator)), dtype=np.uint64)
    x0 = mont([rng.randrange(1, r)], r)
    chal = [rng.randrange(1, r) for _ in range(14)]
    inv = mont([P.inv(x, r) for x in chal], r)
    chal = mont(chal, r)

    def opening():
        s_ = pcdl.IpaSession.with_xi(cs, zz, Hw, x0, "pallas")
        lr = []
        for rd in range(14):
            lr += [a.copy() for a in s_.round_lr()]
            s_.fold(chal[rd], inv[rd])
        return lr + list(s_.end())

    group.PublicParams.synthesize("pallas", n, SEED + 1, precompute_windows=True)
    assert L.halo_srs_window_bits(0) < 17
    ref = opening()
    hal.check(L.halo_srs_precompute_window_range(0, 17, 0, 0))
    assert L.halo_srs_window_bits(0) == 17
    got = opening()
    for a, b in zip(ref, got):
        assert np.array_equal(a, b)
