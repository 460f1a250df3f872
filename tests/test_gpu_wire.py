"""GPU tests of the wire format on the device (halo_amd/csrc/wire.hip, field_sqrt.hpp; halo_amd/wire.py,
pcdl.check_bytes) against tests/wire_ref.py, a pure-Python restatement, and against the reference's own bytes
(tests/golden/wire_qs_head.bin, 18 Pallas instances; wire_qs_head.npz what wire_ref decodes from them).

  1. square roots in both fields: bit-exact smaller root and Euler's criterion, with for every k = 0..32 elements
     whose component in the order-2^32 subgroup has order exactly 2^k (each bit of the subgroup logarithm);
  2. point records -> points: both curves, every refusal, counts that leave a partial wave and a partial block;
  3. points -> records, and 4. scalars both ways;
  5. instances: the fixture by the host and the device form, offsets a device form cannot trust, then openings the
     library makes itself through encode -> check_bytes, whole and damaged.
"""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import pasta as P
import wire_ref as W
from halo_amd import group, pcdl, wire

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEAD = open(os.path.join(GOLDEN, "wire_qs_head.bin"), "rb").read()
EXP = np.load(os.path.join(GOLDEN, "wire_qs_head.npz"))
T = np.load(os.path.join(GOLDEN, "transcript.npz"))
FIELD_OF = {"fp": P.FP_MODULUS, "fq": P.FQ_MODULUS}


def limbs(x: int):
    return P.int_to_limbs(x)


def mont_rows(xs, m):
    return np.array([limbs(P.to_mont(x, m)) for x in xs], dtype=np.uint64).reshape(-1, 4)


def dev(a):
    import torch
    a = np.array(a, copy=True, order="C")
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def host(t, dtype=np.uint64):
    return t.cpu().numpy().view(dtype)


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------
# 1. square roots
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrt_inputs(fname):
    p = FIELD_OF[fname]
    rng = random.Random(0x5152 + len(fname) + (fname == "fq"))
    t = (p - 1) >> 32
    g = pow(5, t, p)  # generates the subgroup of order 2^32
    xs = [0, 1, p - 1, 4, 5] + [rng.randrange(p) for _ in range(1024)]
    for k in range(33):  # order exactly 2^k in the subgroup, times a random element of odd order
        for _ in range(3):
            two_part = pow(g, (rng.randrange(1 << 32) | 1) << (32 - k), p) if k else 1
            xs.append(two_part * pow(rng.randrange(1, p), 1 << 32, p) % p)
    return xs


@pytest.mark.parametrize("fname", ["fp", "fq"])
def test_sqrt(hal, fname):
    p = FIELD_OF[fname]
    xs = sqrt_inputs(fname)
    exp = [W.sqrt(x, p) for x in xs]
    assert exp[:5] == [0, 1, W.sqrt(p - 1, p), 2, None]
    assert all(e is None for e in exp[-3:]) and all(e is not None for e in exp[5 + 1024:-3])  # k = 32: non-residues
    got, sq = wire.sqrt(mont_rows(xs, p), fname)
    assert sq.tolist() == [int(W.is_square(x, p)) for x in xs]
    assert np.array_equal(got, mont_rows([e or 0 for e in exp], p))
    # the device form on its own buffers
    import torch
    d_out = torch.zeros((len(xs), 4), dtype=torch.int64, device="cuda")
    d_sq = torch.full((len(xs),), 7, dtype=torch.uint8, device="cuda")
    d_in = dev(mont_rows(xs, p))  # (a tensor the call reads stays referenced until the synchronise)
    hal.check(hal.load().halo_fe_sqrt_batch_dev(hal.FIELDS[fname], d_in.data_ptr(), len(xs), d_out.data_ptr(),
                                                d_sq.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert np.array_equal(host(d_out), got) and np.array_equal(host(d_sq, np.uint8), sq)


# ---------------------------------------------------------------------------------------------
# 2. / 3. point records
# ---------------------------------------------------------------------------------------------
BAD = "refused"  # what a record the format refuses is expected to decode to (pasta.INF is None: the identity)


def x_bytes(x: int, flags: int = 0) -> bytes:
    return x.to_bytes(32, "little") + bytes([flags])


@functools.lru_cache(maxsize=None)
def good_points(cname):
    """Pallas: every point of the fixture; Vesta: 64 points of the SRS recipe."""
    cv = P.CURVES[cname]
    if cname == "pallas":
        return [pt for q in W.decode_instances(cv, HEAD) for pt in [q["C"], *q["Ls"], *q["Rs"], q["U"], q["C_bar"]]]
    return [P.srs_hash_point(cv, P.srs_index(j)) for j in range(64)]


@functools.lru_cache(maxsize=None)
def records(cname):
    """(records, expected points or BAD) with every edge of the format behind the good points."""
    cv = P.CURVES[cname]
    p = cv.base
    pts = good_points(cname)
    recs = [W.encode_point(cv, pt) for pt in pts]
    gx, gy = cv.generator
    small, large = min(gy, p - gy), max(gy, p - gy)
    rng = random.Random(77)
    non_residues = []
    while len(non_residues) < 8:
        x = rng.randrange(p)
        if not W.is_square((x ** 3 + 5) % p, p):
            non_residues.append(x)
    edges = [(x_bytes(gx, 0x00), (gx, small)), (x_bytes(gx, 0x80), (gx, large)),   # both signs of one point
             (x_bytes(0, 0x40), P.INF),                                            # the infinity record
             (x_bytes(7, 0x40), BAD), (x_bytes(gx, 0xC0), BAD), (x_bytes(0, 0xC0), BAD),
             (x_bytes(gx, 0x01), BAD), (x_bytes(gx, 0x20), BAD), (x_bytes(gx, 0xA0), BAD),
             (x_bytes(p), BAD), (x_bytes(p + gx), BAD), (x_bytes(2 ** 255 - 1), BAD), (x_bytes(2 ** 256 - 1), BAD),
             (x_bytes(0), BAD), (x_bytes(p, 0x40), BAD)]
    edges += [(x_bytes(x, f), BAD) for x, f in zip(non_residues, [0, 0x80] * 4)]
    for rec, exp in edges:
        assert (exp != BAD) == W.point_valid(cv, rec) and (exp == BAD or W.decode_point(cv, rec) == exp)
    return recs + [r for r, _ in edges], list(pts) + [e for _, e in edges]


def expected_rows(cname, exp):
    cv = P.CURVES[cname]
    pts = np.array([W.wrapped(cv, W.SENTINEL if e == BAD else e) for e in exp], dtype=np.uint64)
    return pts, np.array([e != BAD for e in exp], dtype=np.uint8)


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_decompress(hal, cname):
    recs, exp = records(cname)
    pts, ok = expected_rows(cname, exp)
    got, got_ok = wire.decompress_points(b"".join(recs), cname)
    assert got_ok.tolist() == ok.tolist()
    assert np.array_equal(got, pts)
    assert not got[ok == 0][:, :4].any() and len(got[ok == 0]) == len(recs) - int(ok.sum())  # the sentinel: x = 0
    # counts that end inside a wave and inside a block, the edges first so that every count meets some
    order = list(range(len(recs) - 23, len(recs))) + list(range(len(recs) - 23))
    for k in (1, 63, 65, 257):
        take = [order[i % len(order)] for i in range(k)]
        got, got_ok = wire.decompress_points(b"".join(recs[i] for i in take), cname)
        assert got_ok.tolist() == ok[take].tolist() and np.array_equal(got, pts[take]), k
    # the device form, with a canary behind the last output
    import torch
    k = 65
    d_out = torch.full((k + 1, 8), 0x5A5A, dtype=torch.int64, device="cuda")
    d_ok = torch.full((k + 1,), 9, dtype=torch.uint8, device="cuda")
    buf = np.frombuffer(b"".join(recs[i] for i in order[:k]), dtype=np.uint8)
    d_in = dev(buf)
    hal.check(hal.load().halo_points_decompress_dev(hal.CURVES[cname], d_in.data_ptr(), k, d_out.data_ptr(), d_ok.data_ptr(),
                                                    stream()))
    torch.cuda.synchronize()
    assert np.array_equal(host(d_out)[:k], pts[order[:k]]) and host(d_ok, np.uint8)[:k].tolist() == ok[order[:k]].tolist()
    assert (host(d_out)[k] == 0x5A5A).all() and host(d_ok, np.uint8)[k] == 9


@pytest.mark.parametrize("cname", ["pallas", "vesta"])
def test_compress(hal, cname):
    cv = P.CURVES[cname]
    recs, exp = records(cname)
    keep = [i for i, e in enumerate(exp) if e != BAD]
    pts, _ = expected_rows(cname, [exp[i] for i in keep])
    want = b"".join(W.encode_point(cv, exp[i]) for i in keep)
    assert want == b"".join(recs[i] for i in keep)  # every accepted record is the canonical one
    assert wire.compress_points(pts, cname) == want
    assert wire.compress_points(np.zeros((1, 8), dtype=np.uint64), cname) == bytes(32) + b"\x40"
    for k in (1, 63, 65, 257):
        take = [i % len(keep) for i in range(k)]
        assert wire.compress_points(pts[take], cname) == b"".join(want[33 * i: 33 * i + 33] for i in take), k
    assert wire.decompress_points(want, cname)[1].all()
    # neither (0, 0) nor on the curve: refused by the host form, flagged by the device form
    bad = pts[:5].copy()
    bad[3] = W.wrapped(cv, W.SENTINEL)
    with pytest.raises(hal.HaloError, match="point 3 is neither") as e:
        wire.compress_points(bad, cname)
    assert e.value.code == 1
    import torch
    d_out = torch.full((5 * 33 + 1,), 0x5A, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((6,), 9, dtype=torch.uint8, device="cuda")
    d_bad, d_pts = dev(bad), dev(pts)
    hal.check(hal.load().halo_points_compress_dev(hal.CURVES[cname], d_bad.data_ptr(), 5, d_out.data_ptr(), d_ok.data_ptr(),
                                                  stream()))
    torch.cuda.synchronize()
    out = host(d_out, np.uint8).tobytes()
    assert host(d_ok, np.uint8).tolist() == [1, 1, 1, 0, 1, 9] and out[-1] == 0x5A
    assert out[:99] == want[:99] and out[132:165] == want[132:165] and out[99:132] == bytes(32) + b"\xc0"
    assert not W.point_valid(cv, out[99:132])
    hal.check(hal.load().halo_points_compress_dev(hal.CURVES[cname], d_pts.data_ptr(), 5, d_out.data_ptr(), None, stream()))
    torch.cuda.synchronize()
    assert host(d_out, np.uint8).tobytes()[:165] == want[:165]  # the device form writes what the host form returns


# ---------------------------------------------------------------------------------------------
# 4. scalars
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", ["fp", "fq"])
def test_scalars(hal, fname):
    m = FIELD_OF[fname]
    rng = random.Random(5)
    xs = [0, 1, m - 1, m, m + 1, 2 ** 255, 2 ** 256 - 1] + [rng.randrange(m) for _ in range(66)]
    buf = b"".join(x.to_bytes(32, "little") for x in xs)
    got, ok = wire.scalars_from_bytes(buf, fname)
    assert ok.tolist() == [int(x < m) for x in xs]
    assert np.array_equal(got, mont_rows([x if x < m else 0 for x in xs], m))
    good = [x for x in xs if x < m]
    assert wire.scalars_to_bytes(mont_rows(good, m), fname) == b"".join(x.to_bytes(32, "little") for x in good)
    import torch
    d_out = torch.zeros((len(xs), 4), dtype=torch.int64, device="cuda")
    d_ok = torch.full((len(xs),), 9, dtype=torch.uint8, device="cuda")
    d_back = torch.zeros(32 * len(xs), dtype=torch.uint8, device="cuda")
    L = hal.load()
    d_in = dev(np.frombuffer(buf, dtype=np.uint8))
    hal.check(L.halo_scalars_from_bytes_dev(hal.FIELDS[fname], d_in.data_ptr(), len(xs),
                                            d_out.data_ptr(), d_ok.data_ptr(), stream()))
    hal.check(L.halo_scalars_to_bytes_dev(hal.FIELDS[fname], d_out.data_ptr(), len(xs), d_back.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert np.array_equal(host(d_out), got) and host(d_ok, np.uint8).tolist() == ok.tolist()
    assert host(d_back, np.uint8).tobytes() == b"".join((x if x < m else 0).to_bytes(32, "little") for x in xs)


# ---------------------------------------------------------------------------------------------
# 5. instances
# ---------------------------------------------------------------------------------------------
def assert_fixture_instance(q, i):
    a, b = EXP["rounds"][i], EXP["rounds"][i + 1]
    assert q.d == EXP["d"][i]
    for name, got in (("C", q.C), ("z", q.z), ("v", q.v), ("U", q.pi["U"]), ("c", q.pi["c"]), ("C_bar", q.pi["C_bar"]),
                      ("w_prime", q.pi["w_prime"])):
        assert np.array_equal(got, EXP[name][i]), (i, name)
    assert np.array_equal(np.stack(q.pi["Ls"]), EXP["Ls"][a:b]) and np.array_equal(np.stack(q.pi["Rs"]), EXP["Rs"][a:b]), i


def test_fixture_decodes_by_the_host_form(hal):
    qs, ok = wire.decode_instances(HEAD, curve="pallas")
    assert ok.tolist() == [1] * 18 and len(qs) == 18
    for i, q in enumerate(qs):
        assert_fixture_instance(q, i)
    qs2, ok2 = wire.decode_instances((18).to_bytes(8, "little") + HEAD, vec=True, curve="pallas")
    assert ok2.all() and all(np.array_equal(a.C, b.C) and np.array_equal(a.pi["c"], b.pi["c"]) for a, b in zip(qs, qs2))
    assert wire.encode_instances(qs, curve="pallas") == HEAD  # and back, byte for byte
    with pytest.raises(hal.HaloError, match="has d = 7, the call is for d = 3"):
        off = np.array([0, 770], dtype=np.uint64)
        rows = [np.zeros((4, 8), dtype=np.uint64) for _ in range(12)]
        b = np.frombuffer(HEAD, dtype=np.uint8)
        hal.check(hal.load().halo_pcdl_instances_decode(0, 3, 2, hal.ptr(b), len(b), hal.ptr(off), *[hal.ptr(r) for r in rows[:11]]))


def decode_dev(hal, buf, d, offsets, length=None):
    """halo_pcdl_instances_decode_dev over torch buffers: (rows in ABI order, ok)."""
    import torch
    n, lg = len(offsets), (d + 1).bit_length() - 1
    words = lambda m, w: torch.full((m, w), 0x5A5A, dtype=torch.int64, device="cuda")  # noqa: E731
    flags = lambda: torch.full((n,), 9, dtype=torch.uint8, device="cuda")  # noqa: E731
    arrays = [words(n, 8), words(n, 4), words(n, 4), words(n * lg, 8), words(n * lg, 8), words(n, 8), words(n, 4), flags(),
              words(n, 8), words(n, 4)]
    d_ok = flags()
    b = np.frombuffer(buf, dtype=np.uint8)
    d_bytes, d_off = dev(b), dev(np.array(offsets, dtype=np.uint64))
    hal.check(hal.load().halo_pcdl_instances_decode_dev(
        0, d, n, d_bytes.data_ptr(), len(b) if length is None else length, d_off.data_ptr(),
        *[t.data_ptr() for t in arrays], d_ok.data_ptr(), stream()))
    torch.cuda.synchronize()
    return [host(t, np.uint64 if t.dtype == torch.int64 else np.uint8) for t in arrays], host(d_ok, np.uint8)


def test_fixture_decodes_by_the_device_form(hal):
    from halo_amd.wire import _instance
    for d in sorted(set(EXP["d"].tolist())):
        idx = [i for i in range(18) if EXP["d"][i] == d]
        rows, ok = decode_dev(hal, HEAD, d, EXP["offsets"][idx].tolist())
        assert ok.tolist() == [1, 1] and rows[7].tolist() == [1, 1]
        for j, i in enumerate(idx):
            assert_fixture_instance(_instance(d, rows, j, (d + 1).bit_length() - 1), i)


def test_device_form_trusts_no_offset(hal):
    """Offsets and a d the device form was not given by the walk: each is a failed decode of that instance alone."""
    cv = P.PALLAS
    sentinel = np.array(W.wrapped(cv, W.SENTINEL), dtype=np.uint64)
    offsets = [0, len(HEAD), len(HEAD) + 5, 2 ** 63, 2 ** 64 - 1, len(HEAD) - 100, 770, 385]  # 770: an instance of d = 7
    rows, ok = decode_dev(hal, HEAD, 3, offsets)
    assert ok.tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    C, z, v, Ls, Rs, U, c, hid, cb, wp = rows
    assert hid.tolist() == [1, 0, 0, 0, 0, 0, 0, 1]
    assert np.array_equal(C[0], EXP["C"][0]) and np.array_equal(C[7], EXP["C"][1]) and np.array_equal(wp[7], EXP["w_prime"][1])
    for i in range(1, 7):
        for pts in (C[i], U[i], cb[i], Ls[2 * i], Ls[2 * i + 1], Rs[2 * i], Rs[2 * i + 1]):
            assert np.array_equal(pts, sentinel)
        assert not (z[i].any() or v[i].any() or c[i].any() or wp[i].any())
    # a length that cuts the second instance short: the device reads `len`, not the allocation
    rows, ok = decode_dev(hal, HEAD, 3, [0, 385], length=769)
    assert ok.tolist() == [1, 0]
    rows, ok = decode_dev(hal, HEAD, 3, [0, 385], length=385 + 320)  # the plain size fits, the hiding one does not
    assert ok.tolist() == [1, 0]


# ---- openings the library makes itself -------------------------------------------------------
@pytest.fixture(scope="module")
def fs(hal):
    """The reference's Poseidon constants installed for both fields."""
    from halo_amd import schnorr
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, T[f"poseidon_{f}_mds"], T[f"poseidon_{f}_rc"])
    return hal


def det_scalars(seed: int, k: int) -> np.ndarray:
    a = np.random.default_rng(seed).integers(0, 2**64 - 1, size=(k, 4), dtype=np.uint64, endpoint=True)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return np.ascontiguousarray(a)


SHAPES = [(4, False), (8, True), (4, True), (8, False), (4, True)]  # k = 5, two degree bounds, hiding and plain mixed


@pytest.fixture(scope="module")
def five(fs, golden, corc):
    """(instances, wire_ref's bytes): five openings by pcdl.open_device over the recipe SRS of 8 points."""
    S, Hh = golden["ref_sh_pallas"]
    group.PublicParams.upload("pallas", corc.srs_generate("pallas", 8), S, Hh, precompute_windows=True)
    insts = []
    for i, (n, hiding) in enumerate(SHAPES):
        ins = det_scalars(4400 + i, 2 * n + 4)
        p, z = ins[:n], ins[2 * n]
        q = w = w_bar = None
        if hiding:
            q, w, w_bar = ins[n: 2 * n - 1], ins[2 * n + 1], ins[2 * n + 2]
        C = pcdl.commit(p, n - 1, w=w, curve="pallas")
        pi = pcdl.open_device(p, C, n - 1, z, w=w, q=q, w_bar=w_bar, curve="pallas")
        insts.append(pcdl.Instance(C, n - 1, z, pi["v"], pi))
    return insts, W.encode_instances(P.PALLAS, [to_ref(q) for q in insts])


def to_ref(q):
    cv = P.PALLAS
    pt = lambda a: W.unwrapped(cv, [int(x) for x in np.asarray(a).reshape(8)])  # noqa: E731
    sc = lambda a: P.from_mont(P.limbs_to_int(np.asarray(a).reshape(4)), cv.scalar)  # noqa: E731
    hid = q.pi["C_bar"] is not None
    return {"C": pt(q.C), "d": q.d, "z": sc(q.z), "v": sc(q.v), "Ls": [pt(x) for x in q.pi["Ls"]],
            "Rs": [pt(x) for x in q.pi["Rs"]], "U": pt(q.pi["U"]), "c": sc(q.pi["c"]),
            "C_bar": pt(q.pi["C_bar"]) if hid else None, "w_prime": sc(q.pi["w_prime"]) if hid else None}


def starts(insts):
    sizes = [W.instance_size((q.d + 1).bit_length() - 1, q.pi["C_bar"] is not None) for q in insts]
    return np.cumsum([0] + sizes).tolist()


def rhos(seed, k):
    return det_scalars(seed, k) | np.array([1, 0, 0, 0], dtype=np.uint64)


def test_own_openings_round_trip(hal, five):
    insts, ref = five
    assert wire.encode_instances(insts, curve="pallas") == ref
    assert wire.encode_instances(insts, vec=True, curve="pallas") == (5).to_bytes(8, "little") + ref
    assert pcdl.check_batch(insts, curve="pallas", verdicts=True).tolist() == [0] * 5  # the parent's path agrees
    assert pcdl.check_bytes(ref, curve="pallas", verdicts=True).tolist() == [0] * 5
    assert pcdl.check_bytes(ref, curve="pallas") is None
    assert pcdl.check_bytes((5).to_bytes(8, "little") + ref, vec=True, curve="pallas", verdicts=True).tolist() == [0] * 5
    assert pcdl.check_bytes(ref, rhos=rhos(9, 5), curve="pallas", verdicts=True).tolist() == [0] * 5
    back, ok = wire.decode_instances(ref, curve="pallas")
    assert ok.all() and [to_ref(q) for q in back] == [to_ref(q) for q in insts]
    assert pcdl.check_bytes(b"", curve="pallas", verdicts=True).tolist() == []


def test_forged_opening_fails_the_decider(hal, golden, five):
    """An opening that passes the succinct check and fails the decider (tests/test_gpu_decider.py forged_u): code 2,
    also where the random combination of the whole batch is rejected first and the verdicts come from the exact
    rerun on the device, or from the bisection."""
    from test_gpu_decider import forged_u
    insts, _ = five
    q = insts[3]
    C, z, v, pi = forged_u("pallas", golden, q.d, (q.C, q.z, q.v, dict(q.pi, Ls=np.stack(q.pi["Ls"]), Rs=np.stack(q.pi["Rs"]))))
    forged = insts[:3] + [pcdl.Instance(C, q.d, z, v, dict(pi, Ls=list(pi["Ls"]), Rs=list(pi["Rs"])))] + insts[4:]
    buf = W.encode_instances(P.PALLAS, [to_ref(x) for x in forged])
    assert pcdl.check_bytes(buf, curve="pallas", verdicts=True).tolist() == [0, 0, 0, 2, 0]
    for bisect in (False, True):
        assert pcdl.check_bytes(buf, rhos=rhos(12, 5), curve="pallas", verdicts=True, bisect=bisect).tolist() == [0, 0, 0, 2, 0]
    with pytest.raises(pcdl.CheckFailed) as e:
        pcdl.check_bytes(buf, curve="pallas")
    assert e.value.index == 3 and e.value.msg == pcdl.DECIDER_MSG


def test_damaged_bytes(hal, five):
    insts, ref = five
    at = starts(insts)
    assert at[-1] == len(ref)
    # the sign of one L of instance 2 (n = 4: Ls at 113): a valid point, the wrong one
    flipped = bytearray(ref)
    flipped[at[2] + 113 + 33 + 32] ^= 0x80
    assert pcdl.check_bytes(bytes(flipped), curve="pallas", verdicts=True).tolist() == [0, 0, 1, 0, 0]
    for bisect in (False, True):
        assert pcdl.check_bytes(bytes(flipped), rhos=rhos(10, 5), curve="pallas", verdicts=True,
                                bisect=bisect).tolist() == [0, 0, 1, 0, 0]
    with pytest.raises(pcdl.CheckFailed) as e:
        pcdl.check_bytes(bytes(flipped), curve="pallas")
    assert e.value.index == 2 and e.value.msg == pcdl.SUCCINCT_MSG
    # one x of instance 3 (its U, n = 8: at 121 + 66 * 3) replaced by an x with x^3 + 5 a non-residue
    x = next(x for x in range(2, 100) if not W.is_square((x ** 3 + 5) % P.PALLAS.base, P.PALLAS.base))
    nonres = ref[:at[3] + 319] + x.to_bytes(32, "little") + ref[at[3] + 351:]
    assert pcdl.check_bytes(nonres, curve="pallas", verdicts=True).tolist() == [0, 0, 0, 3, 0]
    assert pcdl.check_bytes(nonres, rhos=rhos(11, 5), curve="pallas", verdicts=True).tolist() == [0, 0, 0, 3, 0]
    with pytest.raises(ValueError, match="instance 3: the bytes do not deserialize"):
        pcdl.check_bytes(nonres, curve="pallas")
    back, ok = wire.decode_instances(nonres, curve="pallas")
    assert ok.tolist() == [1, 1, 1, 0, 1]
    sentinel = np.array(W.wrapped(P.PALLAS, W.SENTINEL), dtype=np.uint64)
    assert np.array_equal(back[3].C, sentinel) and np.array_equal(back[3].pi["Ls"][2], sentinel)
    assert not back[3].z.any() and not back[3].pi["c"].any() and np.array_equal(back[2].C, insts[2].C)
    # a scalar set to the modulus: z of instance 0, then w_prime of instance 4
    m = P.PALLAS.scalar.to_bytes(32, "little")
    assert pcdl.check_bytes(m.join([ref[:41], ref[73:]]), curve="pallas", verdicts=True).tolist() == [3, 0, 0, 0, 0]
    assert pcdl.check_bytes(ref[:-32] + m, curve="pallas", verdicts=True).tolist() == [0, 0, 0, 0, 3]
    # broken structure: the walk's error, before any launch
    for cut in (len(ref) - 1, at[4] + 10, 20):
        with pytest.raises(hal.HaloError, match="the buffer ends inside an instance"):
            pcdl.check_bytes(ref[:cut], curve="pallas", verdicts=True)
    with pytest.raises(hal.HaloError, match="a length prefix exceeds"):
        pcdl.check_bytes((6000).to_bytes(8, "little") + ref, vec=True, curve="pallas")
    with pytest.raises(hal.HaloError, match="the buffer ends inside an instance"):
        pcdl.check_bytes((6).to_bytes(8, "little") + ref, vec=True, curve="pallas")
