"""Pure-Python restatement of the wire format of the reference's proof objects: ark-serialize 0.5, compressed mode,
little endian, concatenation the only framing.  The checker of halo_amd/wire.py and of the kernels of
halo_amd/csrc/wire.hip; nothing here touches the GPU.

    usize        u64 LE
    Vec<T>       u64 LE length, then the items
    Option<T>    one byte 0 / 1, then the item if 1
    scalar       32 bytes, the canonical value (not Montgomery), below the modulus
    point        33 bytes: canonical x in bytes 0..31, flags in byte 32: 0x80 y is the larger root (y > p - y),
                 0x40 infinity with x = 0, both set invalid, bits 0..5 zero
    Instance     C, d, z, v, pi          (pcdl.rs:28-34)
    EvalProof    Ls, Rs, U, c, C_bar: Option, w_prime: Option   (pcdl.rs:161-168)
    Accumulator  its q: Instance         (acc.rs:22)

Points are affine tuples (x, y) of canonical integers, pasta.INF for the identity; an instance is the dict
{C, d, z, v, Ls, Rs, U, c, C_bar, w_prime} with C_bar / w_prime None when the proof does not hide.
"""
from __future__ import annotations

import pasta as P

POINT_BYTES, SCALAR_BYTES = 33, 32
FLAG_NEG, FLAG_INF = 0x80, 0x40


class WireError(ValueError):
    """The bytes do not deserialize (where the reference's deserialize_compressed returns Err)."""


# ---------------------------------------------------------------------------------------------
# square roots: Tonelli-Shanks as the textbook states it (data-dependent loops are fine here)
# ---------------------------------------------------------------------------------------------
def is_square(a: int, p: int) -> bool:
    """Euler's criterion; 0 counts as a square."""
    a %= p
    return a == 0 or pow(a, (p - 1) // 2, p) == 1


def sqrt(a: int, p: int):
    """The smaller root of a mod p as a canonical integer, or None for a non-residue."""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = pow(P.GENERATOR, t, p)  # 5 is a non-residue of both Pasta fields
    m, c, u, r = s, z, pow(a, t, p), pow(a, (t + 1) // 2, p)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % p, i + 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c, u, r = i, b * b % p, u * b * b % p, r * b % p
    assert r * r % p == a
    return min(r, p - r)


# ---------------------------------------------------------------------------------------------
# items
# ---------------------------------------------------------------------------------------------
def encode_scalar(x: int, m: int) -> bytes:
    assert 0 <= x < m
    return x.to_bytes(32, "little")


def decode_scalar(b: bytes, m: int) -> int:
    x = int.from_bytes(b[:32], "little")
    if len(b) < 32 or x >= m:
        raise WireError("scalar not below the modulus")
    return x


def encode_point(c: P.Curve, pt) -> bytes:
    if pt is P.INF:
        return bytes(32) + bytes([FLAG_INF])
    x, y = pt
    return x.to_bytes(32, "little") + bytes([FLAG_NEG if y > c.base - y else 0])


def decode_point(c: P.Curve, b: bytes):
    """The point of a 33-byte record; WireError for the records the library refuses."""
    if len(b) < 33:
        raise WireError("truncated point")
    x, flags = int.from_bytes(b[:32], "little"), b[32]
    if flags & 0x3F or flags == (FLAG_NEG | FLAG_INF):
        raise WireError("bad flags")
    if x >= c.base:
        raise WireError("x not below the modulus")
    if flags & FLAG_INF:
        if x:
            raise WireError("non-canonical infinity")  # the library's own rule: only x = 0 is accepted
        return P.INF
    y = sqrt((x * x * x + c.b) % c.base, c.base)
    if y is None:
        raise WireError("x^3 + 5 is not a square")
    return (x, c.base - y if flags & FLAG_NEG else y)  # y != 0: the groups have odd prime order, so no 2-torsion


def point_valid(c: P.Curve, b: bytes) -> bool:
    try:
        decode_point(c, b)
        return True
    except WireError:
        return False


# ---------------------------------------------------------------------------------------------
# Instance
# ---------------------------------------------------------------------------------------------
def encode_instance(c: P.Curve, q: dict) -> bytes:
    m = c.scalar
    out = [encode_point(c, q["C"]), int(q["d"]).to_bytes(8, "little"), encode_scalar(q["z"], m), encode_scalar(q["v"], m)]
    for key in ("Ls", "Rs"):
        out.append(len(q[key]).to_bytes(8, "little"))
        out += [encode_point(c, pt) for pt in q[key]]
    out += [encode_point(c, q["U"]), encode_scalar(q["c"], m)]
    out.append(b"\0" if q["C_bar"] is None else b"\1" + encode_point(c, q["C_bar"]))
    out.append(b"\0" if q["w_prime"] is None else b"\1" + encode_scalar(q["w_prime"], m))
    return b"".join(out)


def instance_size(lg: int, hiding: bool) -> int:
    return 33 + 8 + 64 + 2 * (8 + 33 * lg) + 33 + 32 + 2 + (65 if hiding else 0)


class _Reader:
    def __init__(self, buf: bytes, off: int):
        self.buf, self.off = buf, off

    def take(self, n: int) -> bytes:
        if n > len(self.buf) - self.off:
            raise WireError("truncated")
        self.off += n
        return self.buf[self.off - n: self.off]

    def u64(self) -> int:
        return int.from_bytes(self.take(8), "little")

    def tag(self) -> int:
        t = self.take(1)[0]
        if t > 1:
            raise WireError("option tag")
        return t


def decode_instance(c: P.Curve, buf: bytes, off: int = 0):
    """(instance dict, end offset).  Structure errors and undecodable items raise WireError."""
    r, m = _Reader(buf, off), c.scalar
    q = {"C": decode_point(c, r.take(33)), "d": r.u64()}
    q["z"], q["v"] = decode_scalar(r.take(32), m), decode_scalar(r.take(32), m)
    for key in ("Ls", "Rs"):
        n = r.u64()
        if n > (len(buf) - r.off) // 33:
            raise WireError("length prefix beyond the buffer")
        q[key] = [decode_point(c, r.take(33)) for _ in range(n)]
    q["U"], q["c"] = decode_point(c, r.take(33)), decode_scalar(r.take(32), m)
    q["C_bar"] = decode_point(c, r.take(33)) if r.tag() else None
    q["w_prime"] = decode_scalar(r.take(32), m) if r.tag() else None
    return q, r.off


def encode_instances(c: P.Curve, qs, vec: bool = False) -> bytes:
    return (len(qs).to_bytes(8, "little") if vec else b"") + b"".join(encode_instance(c, q) for q in qs)


def decode_instances(c: P.Curve, buf: bytes, vec: bool = False):
    off, out = 0, []
    count = None
    if vec:
        count, off = int.from_bytes(buf[:8], "little"), 8
    while (off < len(buf)) if count is None else (len(out) < count):
        q, off = decode_instance(c, buf, off)
        out.append(q)
    if off != len(buf):
        raise WireError("trailing bytes")
    return out


# ---------------------------------------------------------------------------------------------
# the library's arrays: WrappedPoint rows (ark Montgomery limbs, (0, 0) the identity), ark Montgomery scalars
# ---------------------------------------------------------------------------------------------
SENTINEL = (0, 1)  # off both curves: what an invalid record decodes to


def wrapped(c: P.Curve, pt) -> list:
    return P.point_to_wrapped(c, pt)


def unwrapped(c: P.Curve, limbs):
    """WrappedPoint limbs -> affine tuple without the on-curve assertion of pasta.wrapped_to_point."""
    x, y = P.limbs_to_int(limbs[0:4]), P.limbs_to_int(limbs[4:8])
    if x == 0 and y == 0:
        return P.INF
    return (P.from_mont(x, c.base), P.from_mont(y, c.base))


def ark_scalar(x: int, m: int) -> list:
    return P.int_to_limbs(P.to_mont(x, m))
