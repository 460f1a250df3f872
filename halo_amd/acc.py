"""Mirror of crates/accumulation/src/acc.rs:128-217 (common_subroutine, prover, verifier, decider) on the
MI355X backend.

The Fiat-Shamir sponges stay with the caller: ``new_transcript(label)`` returns a fresh sponge with the
reference's interface (absorb_g, absorb_fr, challenge over WrappedPoints / ark scalars) for the label
"ASDL" (one per common_subroutine, acc.rs:135) or "PCDL" (one per succinct check and per opening,
pcdl.rs:336,496).  The m succinct checks of common_subroutine run as one batch on the device
(pcdl.succinct_check_many; with ``device_transcripts=True`` their PCDL sponges run there too,
pcdl.succinct_check_device, and so does the sponge of the prover's opening, pcdl.open_device).  An accumulator is the ``pcdl.Instance`` acc.q of the reference.
"""
from __future__ import annotations

import numpy as np

from . import _lib as H
from . import group, pcdl
from .group import _curve
from .pcdl import CheckFailed, Instance


def _alphas_dot_h(hs, alphas, z, cid: int) -> np.ndarray:
    """AccumulatedHPolys::eval (acc.rs:95-101): sum_i alphas[i] h_i(z)."""
    r = pcdl._SCALAR[cid]
    v = sum(pcdl._ark_int(h.eval(z)) * pcdl._ark_int(a) for h, a in zip(hs, alphas)) % r
    return pcdl._ark_limbs(v * pow(1 << 256, -1, r) % r)  # the product of two Montgomery forms carries R twice


def common_subroutine(qs, new_transcript, curve="pallas", device_transcripts=False):
    """acc.rs:128-176.  Returns (C_bar, d, z, hs, alphas): hs the HPolys h_i and alphas the powers of alpha
    (AccumulatedHPolys).  device_transcripts: the PCDL sponges of the succinct checks run on the device
    (pcdl.succinct_check_device); the ASDL sponge stays new_transcript's."""
    cid = _curve(curve)
    qs = [Instance(*q) for q in qs]
    m = len(qs)
    if not m:
        raise CheckFailed("No instances given")
    d = qs[0].d
    transcript = new_transcript("ASDL")
    # 4. the succinct checks, in one batch; 5. d_i = d.  The reference checks instance by instance, so an
    # instance of another degree bound ends the batch: a failing check before it is reported first.
    bad = next((i for i, q in enumerate(qs) if q.d != d), None)
    upto = m if bad is None else bad + 1
    if device_transcripts:
        res = pcdl.succinct_check_device(qs[:upto], cid)
    else:
        res = pcdl.succinct_check_many(qs[:upto], [new_transcript("PCDL") for _ in range(upto)], cid)
    if bad is not None:
        raise CheckFailed("d_i ≠ d", bad)
    hs = [h for h, _ in res]
    Us = [U for _, U in res]
    # 6. alpha := rho_1([h_i, U_i])
    transcript.absorb_fr([x for h in hs for x in h.xis])
    transcript.absorb_g(Us)
    alpha = np.ascontiguousarray(transcript.challenge(), dtype=np.uint64)
    alphas = group.construct_powers(alpha, m, H.SCALAR_FIELD[cid])
    # 8. C := sum alpha^i U_i
    C = pcdl.point_lincomb(np.stack(Us)[None], alphas[None], curve=cid)[0]
    # 9. z := rho_1(C, h)
    z = np.ascontiguousarray(transcript.challenge(), dtype=np.uint64)
    return C, d, z, hs, alphas


def prover(qs, new_transcript, curve="pallas", device_transcripts=False) -> Instance:
    """acc.rs:178-198: the accumulator ((C_bar, d, z, v), pi) of the instances qs.  device_transcripts: the PCDL
    sponges of the succinct checks and of the opening run on the device (pcdl.succinct_check_device,
    pcdl.open_device); the ASDL sponge stays new_transcript's, as in ``verifier``."""
    cid = _curve(curve)
    C_bar, d, z, hs, alphas = common_subroutine(qs, new_transcript, cid, device_transcripts)
    v = _alphas_dot_h(hs, alphas, z, cid)
    h = pcdl.HPoly.combine(hs, alphas)
    if device_transcripts:
        pi = pcdl.open_device(h, C_bar, d, z, curve=cid)
    else:
        pi = pcdl.open(h, C_bar, d, z, w=None, transcript=new_transcript("PCDL"), curve=cid)
    return Instance(C_bar, d, z, v, pi)


def verifier(qs, acc, new_transcript, curve="pallas", device_transcripts=False) -> None:
    """acc.rs:200-213."""
    cid = _curve(curve)
    acc = Instance(*acc)
    C_bar_prime, d_prime, z_prime, hs, alphas = common_subroutine(qs, new_transcript, cid, device_transcripts)
    if not np.array_equal(C_bar_prime, H.point_array(acc.C).reshape(8)):
        raise CheckFailed("C_bar' ≠ C_bar")
    if not np.array_equal(z_prime, H.fe_array(acc.z, 1)[0]):
        raise CheckFailed("z' = z")
    if d_prime != acc.d:
        raise CheckFailed("d' = d")
    if not np.array_equal(_alphas_dot_h(hs, alphas, z_prime, cid), H.fe_array(acc.v, 1)[0]):
        raise CheckFailed("h(z) = v")


def decider(acc, new_transcript, curve="pallas") -> None:
    """acc.rs:215-217: pcdl::check of the accumulator's instance."""
    acc = Instance(*acc)
    pcdl.check(acc.C, acc.d, acc.z, acc.v, acc.pi, new_transcript("PCDL"), curve)


def decider_batch(accs, rhos=None, curve="pallas", bisect: bool = False) -> None:
    """acc.rs:215-217 for many accumulators at once: pcdl.check_batch of their instances, the transcripts and
    the deciders on the device (rhos and bisect as in pcdl.decide_batch).  Raises CheckFailed naming the first
    failing one."""
    pcdl.check_batch([Instance(*a) for a in accs], rhos=rhos, curve=curve, bisect=bisect)
