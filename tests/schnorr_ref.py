"""CPU restatement of crates/schnorr/src/lib.rs for the tests (TEST INFRASTRUCTURE ONLY), built from the
oracle's curve arithmetic (oracle/pasta.py) and Poseidon sponge (oracle/poseidon.py).

Points are affine (x, y) with canonical coordinates, None = the identity; scalars and message elements
are canonical integers.  G = Affine::generator() = (-1, 2).
"""
import numpy as np
import pasta as P
import poseidon


def hash_message(curve: str, pk, R, msg) -> int:
    """lib.rs:24-35: Sponge::new(SIGNATURE); absorb_g_affine(&[pk, R]); absorb_fq(message); challenge()."""
    sp = poseidon.Sponge(curve, poseidon.SIGNATURE)
    sp.absorb_g([pk, R])
    sp.inner.absorb(list(msg))  # absorb_fq: base-field elements go into the inner sponge as they are
    return sp.challenge()


def public_key(curve: str, sk: int):
    c = P.CURVES[curve]
    return P.mul_fast(c, sk, c.generator)


def sign(curve: str, sk: int, k: int, msg):
    """lib.rs:49-66 with the nonce k given: R = k G, e = H(pk, R, m), s = k + e sk."""
    c = P.CURVES[curve]
    R = P.mul_fast(c, k, c.generator)
    e = hash_message(curve, public_key(curve, sk), R, msg)
    return R, (k + e * sk) % c.scalar


_verdicts = {}


def verify(curve: str, pk, msg, R, s: int) -> bool:
    """lib.rs:71-79: s G == R + e pk.  A pk or R off the curve is False (the reference's Affine type
    cannot hold one; the library's rule for its raw WrappedPoint input).  Verdicts are memoised: the
    batches of the tests repeat items."""
    key = (curve, pk, tuple(msg), R, s)
    if key not in _verdicts:
        c = P.CURVES[curve]
        if not (P.on_curve(c, pk) and P.on_curve(c, R)):
            _verdicts[key] = False
        else:
            e = hash_message(curve, pk, R, msg)
            _verdicts[key] = P.mul_fast(c, s, c.generator) == P.add(c, R, P.mul_fast(c, e, pk))
    return _verdicts[key]


# ---- ABI encodings (ark Montgomery limbs)
def fe(x: int, m: int):
    return P.int_to_limbs(P.to_mont(x % m, m))


def fe_rows(xs, m: int) -> np.ndarray:
    return np.array([fe(x, m) for x in xs], dtype=np.uint64).reshape(-1, 4)


def points(curve: str, pts) -> np.ndarray:
    c = P.CURVES[curve]
    return np.array([P.point_to_wrapped(c, p) for p in pts], dtype=np.uint64).reshape(-1, 8)


def from_fe(limbs, m: int) -> int:
    return P.from_mont(P.limbs_to_int(limbs), m)
