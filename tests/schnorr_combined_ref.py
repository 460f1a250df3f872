"""CPU restatement of the combined Schnorr batch (halo_amd/csrc/schnorr_combined.hip behind
halo_schnorr_verify_combined and halo_schnorr_batch_rho; include/halo_gpu.h and DESIGN §4.6 state both) over
oracle/pasta.py, oracle/poseidon.py and the tree of tests/rho_ref.py.  TEST INFRASTRUCTURE ONLY.  The method is this
backend's own: the reference has no batched verification.

An item is (pk, msg, R, s) as tests/schnorr_ref.py takes it: affine points with canonical coordinates (None = the
identity), canonical integers.  It is live iff pk and R are each the identity or on the curve.

  D        (sum rho_i s_i) G - sum rho_i R_i - sum (rho_i e_i) pk_i over the live items, e_i = hash_message(pk_i, R_i, m_i)
  leaf_i   live: Sponge(SIG_BATCH_LEAF = 7).absorb_fr([e_i, s_i]), then the INNER sponge's squeeze().  Not live: 0.
  tree     rho_ref.root
  seed     Sponge(SIG_BATCH_SEED = 8), its inner sponge absorbs root, k, msg_len, squeezed once.
  rho_i    live: Sponge(SIG_BATCH_WEIGHT = 9), its inner sponge absorbs seed, i; challenge(), 0 replaced by 1.  Not live: 0.
"""
import pasta as P
import poseidon
import rho_ref
import schnorr_ref as SR

SIG_BATCH_LEAF, SIG_BATCH_SEED, SIG_BATCH_WEIGHT = 7, 8, 9


_pools = {}


def signature_pool(cname: str, msg_len: int, n: int = 6, seed: int = 811):
    """n valid items (pk, msg, R, s) under three keys, the same for every caller (memoised, read-only)."""
    import numpy as np
    key = (cname, msg_len, n, seed)
    if key not in _pools:
        c = P.CURVES[cname]
        rng = np.random.default_rng(seed + msg_len)
        r = lambda m: int.from_bytes(rng.bytes(32), "little") % m  # noqa: E731
        sks = [r(c.scalar) for _ in range(3)]
        items = []
        for j in range(n):
            msg = tuple(r(c.base) for _ in range(msg_len))
            R, s = SR.sign(cname, sks[j % 3], r(c.scalar), msg)
            items.append((SR.public_key(cname, sks[j % 3]), msg, R, s))
        _pools[key] = (sks, items)
    return _pools[key]


def live(cname: str, item) -> bool:
    c = P.CURVES[cname]
    pk, _, R, _ = item
    return P.on_curve(c, pk) and P.on_curve(c, R)


_hashes = {}


def challenge(cname: str, item) -> int:
    """e of a live item (memoised: the batches of the tests repeat items)."""
    pk, msg, R, _ = item
    key = (cname, pk, tuple(msg), R)
    if key not in _hashes:
        _hashes[key] = SR.hash_message(cname, pk, R, msg)
    return _hashes[key]


def defect(cname: str, items, rhos):
    """D as an affine point (None: the identity); the weights of items that are not live are not read."""
    c = P.CURVES[cname]
    m = c.scalar
    t = 0
    D = None
    for it, rho in zip(items, rhos):
        if not live(cname, it):
            continue
        pk, _, R, s = it
        e = challenge(cname, it)
        t = (t + rho * s) % m
        D = P.add(c, D, P.mul_fast(c, (-rho) % m, R))
        D = P.add(c, D, P.mul_fast(c, (-rho * e) % m, pk))
    return P.add(c, D, P.mul_fast(c, t, c.generator))


def leaf(cname: str, e: int, s: int) -> int:
    sp = poseidon.Sponge(cname, SIG_BATCH_LEAF)
    sp.absorb_fr([e, s])
    return sp.inner.squeeze()


def weights_from(cname: str, es, ss, on, msg_len: int, k=None) -> list[int]:
    """The weights as canonical integers from the challenges, the s values and the liveness of the items; k: the
    count that the seed binds (the batch's own unless a test says otherwise)."""
    n = len(es)
    if n == 0:
        return []
    r = rho_ref.root(cname, [leaf(cname, e, s) if o else 0 for e, s, o in zip(es, ss, on)])
    sd = poseidon.Sponge(cname, SIG_BATCH_SEED)
    sd.inner.absorb([r, n if k is None else k, msg_len])
    seed = sd.inner.squeeze()
    out = []
    for i in range(n):
        if not on[i]:
            out.append(0)
            continue
        w = poseidon.Sponge(cname, SIG_BATCH_WEIGHT)
        w.inner.absorb([seed, i])
        out.append(rho_ref.zero_becomes_one(w.challenge()))
    return out


def weights_int(cname: str, items, msg_len: int) -> list[int]:
    on = [live(cname, it) for it in items]
    es = [challenge(cname, it) if o else 0 for it, o in zip(items, on)]
    return weights_from(cname, es, [it[3] for it in items], on, msg_len)


def weights(cname: str, items, msg_len: int):
    """... as (k, 4) ark scalars, what halo_schnorr_batch_rho writes"""
    return rho_ref.to_ark(cname, weights_int(cname, items, msg_len))
