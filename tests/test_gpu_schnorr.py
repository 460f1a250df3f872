"""GPU tests of the batched Poseidon hash and Schnorr verification (halo_amd/csrc/schnorr.hip):
Poseidon against the reference's own vectors (tests/golden/transcript.npz), hash_message bit-exact and
PublicKey::verify verdict by verdict against the CPU restatement of crates/schnorr/src/lib.rs
(tests/schnorr_ref.py), both curves, both lane layouts of the sponge kernels (poseidon_lanes)."""
import ctypes
import os

import numpy as np
import pytest

import pasta as P
import poseidon
import schnorr_ref as SR

pytestmark = pytest.mark.gpu

CURVES = ["pallas", "vesta"]
BASE_FIELD = {"pallas": "fq", "vesta": "fp"}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transcript.npz")


@pytest.fixture(scope="module")
def sch(hal):
    """halo_amd.schnorr with the reference's Poseidon constants installed for both fields."""
    from halo_amd import schnorr
    g = np.load(GOLDEN)
    for f in ("fp", "fq"):
        schnorr.set_poseidon_params(f, g[f"poseidon_{f}_mds"], g[f"poseidon_{f}_rc"])
    return schnorr


@pytest.fixture(scope="module")
def keys():
    """Per curve: three key pairs and, per message length, a pool of signed messages (shared, read-only)."""
    rng = np.random.default_rng(2024)
    out = {}
    for cname in CURVES:
        c = P.CURVES[cname]
        sks = [int.from_bytes(rng.bytes(32), "little") % c.scalar for _ in range(3)]
        out[cname] = {"sk": sks, "pk": [SR.public_key(cname, sk) for sk in sks], "rng": rng}
    return out


def rand_msg(rng, m, n):
    return tuple(int.from_bytes(rng.bytes(32), "little") % m for _ in range(n))


def vectors():
    g = np.load(GOLDEN)
    vs = []
    i = 0
    while f"kimchi_{i}_in" in g:
        vs.append((f"kimchi_{i}", "fq", g[f"kimchi_{i}_in"], g[f"kimchi_{i}_out"]))
        i += 1
    assert i == 6
    for tag, field in (("mina_fq", "fp"), ("mina_fp", "fq")):  # as tests/test_oracle.py:266 drives them
        vs.append((tag, field, g[f"{tag}_in"], g[f"{tag}_out"]))
    return vs


@pytest.mark.parametrize("lanes", [1, 3])
def test_poseidon_reference_vectors(hal, sch, lanes):
    """The six Kimchi vectors (kimchi-vecs.json) and the two Mina vectors (inner_sponge.rs:323-368), each
    as a batch of one."""
    with hal.tuning(poseidon_lanes=lanes):
        for tag, field, vin, vout in vectors():
            m = P.FIELDS[field]
            xs = [P.limbs_to_int(x) for x in np.asarray(vin).reshape(-1, 4)]
            rows = SR.fe_rows(xs, m).reshape(1, len(xs), 4)
            got = sch.poseidon_hash_batch(rows, field)
            assert SR.from_fe(got[0], m) == P.limbs_to_int(vout), (tag, lanes)


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("k", [65, 257])
def test_poseidon_batch_boundaries(hal, sch, lanes, k):
    """One vector replicated over several waves and blocks, one row altered: every row gets its own hash."""
    tag, field, vin, vout = max(vectors()[:6], key=lambda v: len(v[2]))
    m = P.FIELDS[field]
    xs = [P.limbs_to_int(x) for x in np.asarray(vin).reshape(-1, 4)]
    assert len(xs) >= 2
    alt = list(xs)
    alt[-1] = (alt[-1] + 1) % m
    sp = poseidon.InnerSponge(field)
    sp.absorb(alt)
    exp_alt = sp.squeeze()
    rows = np.repeat(SR.fe_rows(xs, m).reshape(1, len(xs), 4), k, axis=0)
    j = k - 2
    rows[j] = SR.fe_rows(alt, m)
    with hal.tuning(poseidon_lanes=lanes):
        got = sch.poseidon_hash_batch(rows, field)
    exp = [exp_alt if i == j else P.limbs_to_int(vout) for i in range(k)]
    assert [SR.from_fe(r, m) for r in got] == exp


@pytest.mark.parametrize("msg_len", [0, 1, 2, 10, 11])
@pytest.mark.parametrize("cname", CURVES)
def test_hash_message_batch(hal, sch, keys, cname, msg_len):
    """halo_schnorr_hash_batch == hash_message, bit-exact: k = 1, 3, 65, both lane layouts; item 1 of the
    larger batches has R = identity.  (Label + four coordinates = 5 elements before the message, so the
    lengths cover both parities of the rate-2 boundary; Vesta takes the shifted challenge.)"""
    c = P.CURVES[cname]
    rng = keys[cname]["rng"]
    pts = keys[cname]["pk"]
    for k in (1, 3, 65):
        pk = [pts[i % 3] for i in range(k)]
        R = [pts[(i + 1) % 3] for i in range(k)]
        if k >= 3:
            R[1] = None
        msgs = [rand_msg(rng, c.base, msg_len) for _ in range(k)]
        exp = [SR.hash_message(cname, pk[i], R[i], msgs[i]) for i in range(k)]
        marr = np.array([SR.fe_rows(mm, c.base) for mm in msgs], dtype=np.uint64).reshape(k, msg_len, 4)
        for lanes in (1, 3):
            with hal.tuning(poseidon_lanes=lanes):
                got = sch.hash_message_batch(SR.points(cname, pk), SR.points(cname, R), marr, cname)
            assert [SR.from_fe(r, c.scalar) for r in got] == exp, (k, lanes)


def verification_batch(cname, keys, msg_len, k):
    """k items in interleaved classes (so valid and invalid ones share waves and quads):
    0 valid, 1 wrong message, 2 s replaced, 3 wrong public key, 4 s = 0, 5 R = identity with matching s,
    6 pk = identity (signed by sk = 0 on even rounds -- valid by the reference's arithmetic -- else by a
    real key), 7 R off the curve, 8 pk off the curve."""
    c = P.CURVES[cname]
    rng = keys[cname]["rng"]
    sks, pks = keys[cname]["sk"], keys[cname]["pk"]
    pool = []  # (key index, msg, R, s): two signed messages per key
    for ki in range(3):
        for _ in range(2):
            msg = rand_msg(rng, c.base, msg_len)
            R, s = SR.sign(cname, sks[ki], int.from_bytes(rng.bytes(32), "little") % c.scalar, msg)
            pool.append((ki, msg, R, s))
    # a signature over another message: for the empty message, one made over a one-element message
    other = rand_msg(rng, c.base, max(msg_len, 1))
    wrong_R, wrong_s = SR.sign(cname, sks[0], 12345, other)
    id_R, id_s = SR.sign(cname, sks[1], 0, pool[2][1])       # nonce 0: R = identity, s = e sk
    zero_R, zero_s = SR.sign(cname, 0, 777, pool[0][1])      # sk = 0: pk = identity, s = k
    items = []
    for i in range(k):
        ki, msg, R, s = pool[(i // 9) % len(pool)]
        pk = pks[ki]
        cls = i % 9
        if cls == 1:
            if msg_len:
                msg = msg[:-1] + ((msg[-1] + 1) % c.base,)
            else:
                pk, R, s = pks[0], wrong_R, wrong_s
        elif cls == 2:
            s = (s + 1 + i) % c.scalar
        elif cls == 3:
            pk = pks[(ki + 1) % 3]
        elif cls == 4:
            s = 0
        elif cls == 5:
            pk, msg, R, s = pks[1], pool[2][1], id_R, id_s
        elif cls == 6:
            if (i // 9) % 2 == 0:
                pk, msg, R, s = None, pool[0][1], zero_R, zero_s
            else:
                pk = None
        elif cls == 7:
            R = (R[0], (R[1] + 1) % c.base)
        elif cls == 8:
            pk = ((pk[0] + 1) % c.base, pk[1])
        items.append((pk, msg, R, s))
    return items


def encode(cname, items, msg_len):
    c = P.CURVES[cname]
    k = len(items)
    pk = SR.points(cname, [it[0] for it in items])
    R = SR.points(cname, [it[2] for it in items])
    s = SR.fe_rows([it[3] for it in items], c.scalar)
    msgs = np.array([SR.fe_rows(it[1], c.base) for it in items], dtype=np.uint64).reshape(k, msg_len, 4)
    return pk, R, s, msgs


@pytest.fixture(scope="module")
def batches(keys):
    """The verification batches and the restatement's verdicts, computed once per (curve, msg_len)."""
    cache = {}

    def get(cname, msg_len):
        if (cname, msg_len) not in cache:
            items = verification_batch(cname, keys, msg_len, 257)
            exp = np.array([SR.verify(cname, *it) for it in items], dtype=np.uint8)
            cache[(cname, msg_len)] = (items, exp)
        return cache[(cname, msg_len)]
    return get


@pytest.mark.parametrize("msg_len", [10, 0])
@pytest.mark.parametrize("cname", CURVES)
def test_verify_batch_classes(hal, sch, batches, cname, msg_len):
    items, exp = batches(cname, msg_len)
    assert exp.min() == 0 and exp.max() == 1
    for cls, want in ((0, 1), (5, 1), (1, 0), (2, 0), (3, 0), (4, 0), (7, 0), (8, 0)):
        assert all(exp[i] == want for i in range(cls, len(items), 9)), cls
    assert exp[6] == 1 and exp[15] == 0  # pk = identity: valid when signed by sk = 0
    got = sch.verify_batch(*encode(cname, items, msg_len), cname)
    assert got.dtype == np.uint8 and got.shape == exp.shape
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0]


def _dev(t):
    return ctypes.c_void_p(t.data_ptr())


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("cname", CURVES)
def test_dev_variants_match(hal, sch, batches, cname):
    """The _dev entry points over device pointers give the host entry points' outputs."""
    import torch
    L = hal.load()
    curve = hal.CURVES[cname]
    field = hal.FIELDS[BASE_FIELD[cname]]
    c = P.CURVES[cname]
    items, exp = batches(cname, 10)
    pk, R, s, msgs = encode(cname, items, 10)
    k = len(items)
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_pk, d_R, d_s, d_m = _cuda(pk), _cuda(R), _cuda(s), _cuda(msgs)
    d_ok = torch.zeros(k, dtype=torch.uint8, device="cuda")
    hal.check(L.halo_schnorr_verify_batch_dev(curve, _dev(d_pk), _dev(d_R), _dev(d_s), _dev(d_m), 10, k, _dev(d_ok), sp))
    assert np.array_equal(d_ok.cpu().numpy(), exp)
    d_e = torch.zeros((k, 4), dtype=torch.int64, device="cuda")
    hal.check(L.halo_schnorr_hash_batch_dev(curve, _dev(d_pk), _dev(d_R), _dev(d_m), 10, k, _dev(d_e), sp))
    assert np.array_equal(d_e.cpu().numpy().view(np.uint64), sch.hash_message_batch(pk, R, msgs, cname))
    d_h = torch.zeros((k, 4), dtype=torch.int64, device="cuda")
    hal.check(L.halo_poseidon_hash_batch_dev(field, _dev(d_m), 10, k, _dev(d_h), sp))
    assert np.array_equal(d_h.cpu().numpy().view(np.uint64), sch.poseidon_hash_batch(msgs, BASE_FIELD[cname]))
    assert SR.from_fe(d_h.cpu().numpy().view(np.uint64)[0], c.base) < c.base


@pytest.mark.parametrize("cname", CURVES)
def test_the_ladder_agrees_with_the_linear_combination(hal, sch, keys, cname):
    """The two users of the shared quad ladder (quad_ladder.hpp) on one statement: the verdict of
    halo_schnorr_verify_batch for item i and the "valid and the identity" byte of halo_point_lincomb_batch_dev for
    -R_i + s_i G - e_i pk_i (e_i from halo_schnorr_hash_batch), each against the CPU restatement's verdict.
    17 signatures over one-element messages: one quad more than a wave's 16; among them a wrong s, an identity pk
    (signed by sk = 0: valid) and a pk off the curve.  The _dev form is the one called: the host form returns the
    affine sums only, where an invalid item and an identity sum are both (0, 0); the byte is the _dev form's."""
    import torch
    c = P.CURVES[cname]
    rng = np.random.default_rng(17)
    sks, pks = keys[cname]["sk"], keys[cname]["pk"]
    k = 17
    items = []
    for i in range(k):
        msg = rand_msg(rng, c.base, 1)
        sk, pk = (0, None) if i == 7 else (sks[i % 3], pks[i % 3])
        R, s = SR.sign(cname, sk, int.from_bytes(rng.bytes(32), "little") % c.scalar, msg)
        if i == 3:
            s = (s + 1) % c.scalar
        if i == 12:
            pk = ((pk[0] + 1) % c.base, pk[1])
        items.append((pk, msg, R, s))
    exp = np.array([SR.verify(cname, *it) for it in items], dtype=np.uint8)
    assert exp[3] == 0 and exp[7] == 1 and exp[12] == 0 and exp.sum() == k - 2
    pk, R, s, msgs = encode(cname, items, 1)
    got = sch.verify_batch(pk, R, s, msgs, cname)
    assert np.array_equal(got, exp), np.nonzero(got != exp)[0]

    e = [SR.from_fe(row, c.scalar) for row in sch.hash_message_batch(pk, R, msgs, cname)]
    assert e == [SR.hash_message(cname, it[0], it[2], it[1]) for it in items]
    neg_R = SR.points(cname, [None if it[2] is None else (it[2][0], -it[2][1] % c.base) for it in items])
    G = SR.points(cname, [c.generator])[0]
    pts = np.stack([np.stack([G, pk[i]]) for i in range(k)])
    sc = np.stack([SR.fe_rows([items[i][3], -e[i] % c.scalar], c.scalar) for i in range(k)])
    d_add, d_pts, d_sc = _cuda(neg_R), _cuda(pts), _cuda(sc)
    d_out = torch.zeros((k, 16), dtype=torch.int64, device="cuda")
    d_id = torch.full((k,), 7, dtype=torch.uint8, device="cuda")
    sp = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    hal.check(hal.load().halo_point_lincomb_batch_dev(hal.CURVES[cname], _dev(d_add), _dev(d_pts), _dev(d_sc), k, 2,
                                                     _dev(d_out), _dev(d_id), sp))
    is_id = d_id.cpu().numpy()
    assert np.array_equal(is_id, exp), np.nonzero(is_id != exp)[0]


def test_reference_shape_and_asynchrony(hal, sch, keys):
    """crates/plonk/src/main.rs:39-43 verifies ONE (pk, message, signature) many times over: 4096 copies
    all verify.  The device-pointer call is asynchronous: several batches are queued and the stream is
    still busy when the last call has returned (the queued work is tens of host call times long; a host
    stalled for longer than that between the two lines would fail this spuriously)."""
    import torch
    cname = "pallas"
    c = P.CURVES[cname]
    rng = keys[cname]["rng"]
    msg = rand_msg(rng, c.base, 10)
    R, s = SR.sign(cname, keys[cname]["sk"][0], 424242, msg)
    assert SR.verify(cname, keys[cname]["pk"][0], msg, R, s)
    k = 4096
    pk, Ra, sa, msgs = encode(cname, [(keys[cname]["pk"][0], msg, R, s)] * k, 10)
    got = sch.verify_batch(pk, Ra, sa, msgs, cname)
    assert got.shape == (k,) and np.all(got == 1)

    L = hal.load()
    d_pk, d_R, d_s, d_m = _cuda(pk), _cuda(Ra), _cuda(sa), _cuda(msgs)
    d_ok = torch.zeros((8, k), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)
    torch.cuda.synchronize()
    for r in range(8):
        hal.check(L.halo_schnorr_verify_batch_dev(hal.CURVES[cname], _dev(d_pk), _dev(d_R), _dev(d_s), _dev(d_m), 10, k,
                                                  _dev(d_ok[r]), sp))
    busy = not stream.query()
    torch.cuda.synchronize()
    assert busy, "halo_schnorr_verify_batch_dev returned only after its work had finished"
    assert bool((d_ok == 1).all())
