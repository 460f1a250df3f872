"""Mirror of crates/schnorr/src/lib.rs (generate_keypair, SecretKey::sign, hash_message, PublicKey::verify) and of
the inner Poseidon sponge (crates/poseidon/src/inner_sponge.rs) on the MI355X backend, as batches of independent
items: the reference's benchmark verifies 40 000 signatures in a parallel loop (crates/plonk/src/main.rs:35-47).

verify_batch's default is exact, one ladder per signature; with ``rhos`` it checks the whole batch by one MSM of
2 k + 1 terms under the caller's random weights or under weights derived from the batch (batch_weights), which the
reference does not have: an accept is then sound up to about k / 2^254, a reject is resolved exactly, by every ladder
or, with ``bisect=True``, by a descent that halves the failing parts of the batch.

Key derivation and signing run on the device too (public_key_batch, sign_batch: a fixed-base comb over the
generator, halo_generator_mul_batch / halo_schnorr_sign_batch).  The library never draws randomness: secrets and
nonces are the caller's, and where this module is asked to draw them (generate_keypairs, sign_batch without
nonces) it does so here, from ``secrets``.  The kernels are not hardened against side channels.  The Poseidon
constants are the caller's as well (``PastaConfig::POSEIDON_*``): install them once per field with
set_poseidon_params.
"""
from __future__ import annotations

import secrets

import numpy as np

from . import _lib as H
from .group import _curve, _field

SCALAR_MODULUS = {  # ark_pallas::Fr (Pallas scalars) and ark_pallas::Fq (Vesta scalars)
    H.PALLAS: 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,
    H.VESTA: 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001,
}


def set_poseidon_params(field, mds, rc) -> None:
    """Install the Poseidon parameters of `field`: mds (9, 4) row-major, rc (165, 4), ark Montgomery limbs
    (host-only; the hashing and Schnorr calls of that field need it first)."""
    mds, rc = H.fe_array(mds, 9), H.fe_array(rc, 165)
    H.check(H.load().halo_poseidon_set_params(_field(field), H.ptr(mds), H.ptr(rc)))


def poseidon_hash_batch(rows, field="fq") -> np.ndarray:
    """k independent inner sponges: rows (k, len, 4) -> absorb row i, squeeze once -> (k, 4)."""
    H.ensure_device()
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.uint64))
    assert rows.ndim == 3 and rows.shape[2] == 4, "rows: (k, len, 4) uint64"
    k, ln = rows.shape[0], rows.shape[1]
    out = np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_poseidon_hash_batch(_field(field), H.ptr(rows) if ln else None, ln, k, H.ptr(out)))
    return out


def _messages(msgs, k: int):
    msgs = np.ascontiguousarray(np.asarray(msgs, dtype=np.uint64))
    if msgs.size == 0:
        return None, 0
    msgs = msgs.reshape(k, -1, 4)
    return msgs, msgs.shape[1]


def hash_message_batch(pk, R, msgs, curve="pallas") -> np.ndarray:
    """lib.rs:24-35 ``hash_message`` for k (pk, R, message) triples: pk, R (k, 8) WrappedPoints, msgs
    (k, msg_len, 4) base-field elements -> (k, 4) scalars e."""
    H.ensure_device()
    pk, R = H.point_array(pk), H.point_array(R)
    k = len(pk)
    assert len(R) == k
    m, ml = _messages(msgs, k)
    out = np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_schnorr_hash_batch(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(m), ml, k, H.ptr(out)))
    return out


def verify_batch(pk, R, s, msgs, curve="pallas", rhos=None, return_combined=False, bisect=False):
    """lib.rs:71-79 ``PublicKey::verify`` for k signatures (R[i], s[i]) over msgs[i] under pk[i]:
    (k,) uint8, 1 = valid.  A pk or R that is neither (0, 0) nor on the curve gives 0.

    ``rhos`` (the convention of pcdl.decide_batch): None is the exact call, one ladder per signature.  A (k, 4) array
    of nonzero scalars, or "fs" for the weights of batch_weights, takes the combined pass instead
    (halo_schnorr_verify_combined): ONE MSM of 2 k + 1 terms, and only if that rejects the exact ladders, so the
    verdicts are per item either way.  The caller's weights must be drawn uniformly AFTER the signatures are fixed; an
    accept is then sound up to about k / 2^254 (derived weights: Q k / 2^254 over Q batches tried), a reject is exact.
    ``return_combined``: also return the combined pass's byte (1 = it held; None for the exact call).

    ``bisect`` (needs ``rhos``): a rejected combined batch is resolved by bisection on the device (tuning key
    schnorr_bisect = 1 for this call; halo_schnorr_verify_bisect_dev states the method) instead of the ladder over every
    item: a failing node is halved at the cost of one MSM over its left half, down to single items or to slices small
    enough for the ladder.  The contract changes for the items of a rejected batch: a reject found by the descent is
    exact; an item in a half that passes is accepted up to about 1 / 2^254 per node tested, for weights drawn after
    the signatures were fixed (with weights known in advance, errors that cancel inside one half pass there)."""
    if bisect and rhos is None:
        raise ValueError("bisect=True needs rhos (weights, or 'fs'): the exact call has no combined batch to bisect")
    H.ensure_device()
    pk, R, s = H.point_array(pk), H.point_array(R), H.fe_array(s)
    k = len(pk)
    assert len(R) == k and len(s) == k
    m, ml = _messages(msgs, k)
    out = np.zeros(k, dtype=np.uint8)
    if rhos is None:
        H.check(H.load().halo_schnorr_verify_batch(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(out)))
        return (out, None) if return_combined else out
    rho, _ = H.fs_rhos(rhos, k)
    comb = np.zeros(1, dtype=np.uint8)
    with H.tuning(schnorr_bisect=1) if bisect else H.tuning():
        H.check(H.load().halo_schnorr_verify_combined(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(rho),
                                                      H.ptr(out), H.ptr(comb)))
    return (out, int(comb[0])) if return_combined else out


def batch_weights(pk, R, s, msgs, curve="pallas") -> np.ndarray:
    """The weights that ``verify_batch(..., rhos="fs")`` runs under (halo_schnorr_batch_rho), derived on the device
    from the batch itself: (k, 4) scalars, 0 for an item whose pk or R is neither (0, 0) nor on the curve."""
    H.ensure_device()
    pk, R, s = H.point_array(pk), H.point_array(R), H.fe_array(s)
    k = len(pk)
    assert len(R) == k and len(s) == k
    m, ml = _messages(msgs, k)
    out = np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_schnorr_batch_rho(_curve(curve), H.ptr(pk), H.ptr(R), H.ptr(s), H.ptr(m), ml, k, H.ptr(out)))
    return out


def _random_scalars(k: int, curve="pallas") -> np.ndarray:
    """k scalars of `curve`, uniform in [1, r - 1], from the operating system's generator (``secrets``), as
    (k, 4) ark Montgomery limbs: what generate_keypairs and sign_batch draw when the caller passes none."""
    r = SCALAR_MODULUS[_curve(curve)]
    out = np.zeros((k, 4), dtype=np.uint64)
    for i in range(k):
        v = ((secrets.randbelow(r - 1) + 1) << 256) % r
        out[i] = [(v >> (64 * j)) & (2**64 - 1) for j in range(4)]
    return out


def public_key_batch(sk, curve="pallas") -> np.ndarray:
    """lib.rs:41-43 ``generate_keypair``'s pk = sk G for k secrets the caller drew: sk (k, 4) scalars below the
    modulus -> (k, 8) WrappedPoints; sk = 0 gives (0, 0)."""
    H.ensure_device()
    sk = H.fe_array(sk)
    out = np.zeros((len(sk), 8), dtype=np.uint64)
    H.check(H.load().halo_generator_mul_batch(_curve(curve), H.ptr(sk), len(sk), H.ptr(out)))
    return out


def generate_keypairs(k: int, curve="pallas"):
    """lib.rs:38-46 ``generate_keypair`` k times: (sk (k, 4), pk (k, 8)), the secrets drawn here from ``secrets``, uniform in [1, r - 1]."""
    sk = _random_scalars(k, curve)
    return sk, public_key_batch(sk, curve)


def sign_batch(sk, msgs, curve="pallas", nonces=None, pk=None):
    """lib.rs:49-66 ``SecretKey::sign`` for k (sk[i], msgs[i]) pairs: (R (k, 8), s (k, 4)) with R = nonce G,
    s = nonce + hash_message(pk, R, m) sk.  ``nonces``: (k, 4) scalars below the modulus, each uniform, secret and
    used once; None draws them here from ``secrets``.  ``pk``: the keys of sk where the caller has them (hashed as
    given); None derives pk = sk G on the device, as the reference does on every sign."""
    H.ensure_device()
    sk = H.fe_array(sk)
    k = len(sk)
    nonces = _random_scalars(k, curve) if nonces is None else H.fe_array(nonces, k)
    pk = None if pk is None else H.point_array(pk)
    assert pk is None or len(pk) == k
    m, ml = _messages(msgs, k)
    R, s = np.zeros((k, 8), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_schnorr_sign_batch(_curve(curve), H.ptr(sk), H.ptr(pk), H.ptr(nonces), H.ptr(m), ml, k, H.ptr(R),
                                             H.ptr(s)))
    return R, s
