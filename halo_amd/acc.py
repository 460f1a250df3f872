"""Mirror of crates/accumulation/src/acc.rs:128-217 (common_subroutine, prover, verifier, decider) on the
MI355X backend.

The Fiat-Shamir sponges are the caller's choice: ``new_transcript(label)`` returns a fresh sponge with the
reference's interface (absorb_g, absorb_fr, challenge over WrappedPoints / ark scalars;
``halo_amd.sponge.new_transcript(curve)`` is the library's own, on the device) for the label
"ASDL" (one per common_subroutine, acc.rs:135) or "PCDL" (one per succinct check and per opening,
pcdl.rs:336,496).  The m succinct checks of common_subroutine run as one batch on the device
(pcdl.succinct_check_many; with ``device_transcripts=True`` their PCDL sponges run there too,
pcdl.succinct_check_device, and so does the sponge of the prover's opening, pcdl.open_device).  An accumulator is the ``pcdl.Instance`` acc.q of the reference.

``common_subroutine_device``, ``prover_device``, ``verifier_device`` and ``verifier_batch`` take no ``new_transcript``:
the ASDL sponge runs on the device too, and each is one library call (halo_acc_prover, halo_acc_verifier_batch;
halo_amd/csrc/acc_fs.hip).  They return and raise what the functions above do.
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


# ---------------------------------------------------------------------------------------------
# the ASDL sponge on the device too: one call per accumulation step (halo_amd/csrc/acc_fs.hip)
# ---------------------------------------------------------------------------------------------
ACCEPT, INSTANCE, C_BAR, Z, V = range(5)  # halo_acc_verdict_t
_MSGS = {INSTANCE: pcdl.SUCCINCT_MSG, C_BAR: "C_bar' ≠ C_bar", Z: "z' = z", V: "h(z) = v"}


def _checked_instances(qs, cid: int):
    """What common_subroutine establishes before the ASDL sponge is touched, in the reference's order: some
    instance, shapes, and d_i = d (an instance of another degree bound ends the batch: a failing succinct check
    up to and including it is reported first).  Returns (instances, d)."""
    qs = [Instance(*q) for q in qs]
    if not qs:
        raise CheckFailed("No instances given")
    pcdl._check_shapes(qs, cid)
    d = qs[0].d
    bad = next((i for i, q in enumerate(qs) if q.d != d), None)
    if bad is not None:
        pcdl.succinct_check_device(qs[: bad + 1], cid)
        raise CheckFailed("d_i ≠ d", bad)
    return qs, d


def verifier_codes(groups, accs, d: int, curve="pallas"):
    """halo_acc_verifier_batch: k accumulations (``groups``: k lists of m instances of degree bound d each) against
    ``accs`` (k accumulators, or None: common_subroutine and the evaluation alone).  Returns (verdict (k,) uint8,
    first_bad (k,) uint32, asdl (k, 2, 4) = alpha, z', C_bar (k, 8), v (k, 4))."""
    H.ensure_device()
    k, m = len(groups), len(groups[0])
    assert all(len(g) == m for g in groups), "one m per call"
    rows = pcdl.instance_rows([q for g in groups for q in g], d)
    acc_rows = [None, None, None]
    if accs is not None:
        accs = [Instance(*a) for a in accs]
        acc_rows = [np.stack([H.point_array(a.C).reshape(8) for a in accs]), np.stack([H.fe_array(a.z, 1)[0] for a in accs]),
                    np.stack([H.fe_array(a.v, 1)[0] for a in accs])]
    verdict, first_bad = np.zeros(k, dtype=np.uint8), np.zeros(k, dtype=np.uint32)
    asdl, C_bar, v = np.zeros((k, 2, 4), dtype=np.uint64), np.zeros((k, 8), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64)
    H.check(H.load().halo_acc_verifier_batch(_curve(curve), d, k, m, *[H.ptr(a) for a in rows], *[H.ptr(a) for a in acc_rows],
                                             H.ptr(verdict), H.ptr(first_bad), H.ptr(asdl), H.ptr(C_bar), H.ptr(v)))
    return verdict, first_bad, asdl, C_bar, v


def common_subroutine_device(qs, curve="pallas"):
    """common_subroutine with every sponge on the device, the ASDL one included (halo_acc_verifier_batch without an
    accumulator): no new_transcript.  Returns (C_bar, d, z, hs, alphas) and raises CheckFailed as common_subroutine
    does.  The HPolys come from a second call (pcdl.succinct_check_device); prover_device and verifier_device, which
    need none, make one call."""
    cid = _curve(curve)
    qs, d = _checked_instances(qs, cid)
    verdict, first_bad, asdl, C_bar, _ = verifier_codes([qs], None, d, cid)
    if verdict[0] != ACCEPT:
        raise CheckFailed(_MSGS[INSTANCE], int(first_bad[0]))
    hs = [h for h, _ in pcdl.succinct_check_device(qs, cid)]
    alphas = group.construct_powers(np.ascontiguousarray(asdl[0, 0]), len(qs), H.SCALAR_FIELD[cid])
    return C_bar[0], d, np.ascontiguousarray(asdl[0, 1]), hs, alphas


def prover_device(qs, curve="pallas") -> Instance:
    """acc.rs:178-198 in one call (halo_acc_prover): the succinct checks, the ASDL sponge, h = sum alpha^i h_i and its
    opening all on the device; h never visits the host.  No new_transcript; the result and the CheckFailed texts
    are ``prover``'s."""
    H.ensure_device()
    cid = _curve(curve)
    qs, d = _checked_instances(qs, cid)
    lg = (d + 1).bit_length() - 1
    rows = pcdl.instance_rows(qs, d)
    C, z, v = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    Ls, Rs = np.zeros((max(lg, 1), 8), dtype=np.uint64), np.zeros((max(lg, 1), 8), dtype=np.uint64)
    U, c = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    verdict, first_bad = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    H.check(H.load().halo_acc_prover(cid, d, len(qs), *[H.ptr(a) for a in rows], H.ptr(C), H.ptr(z), H.ptr(v), H.ptr(Ls),
                                     H.ptr(Rs), H.ptr(U), H.ptr(c), H.ptr(verdict), H.ptr(first_bad)))
    if verdict[0] != ACCEPT:
        raise CheckFailed(_MSGS[INSTANCE], int(first_bad[0]))
    pi = {"Ls": [Ls[j].copy() for j in range(lg)], "Rs": [Rs[j].copy() for j in range(lg)], "U": U, "c": c,
          "C_bar": None, "w_prime": None, "v": v.copy()}
    return Instance(C, d, z, v, pi)


def _raise_verdict(code: int, first_bad: int, d: int, acc_d: int, index=None) -> None:
    """The reference's order (acc.rs:149,207-210): the instances, C_bar, z, d, v."""
    if code == INSTANCE:
        raise CheckFailed(_MSGS[INSTANCE], first_bad if index is None else index)
    if code in (C_BAR, Z):
        raise CheckFailed(_MSGS[code], index)
    if d != acc_d:
        raise CheckFailed("d' = d", index)
    if code == V:
        raise CheckFailed(_MSGS[V], index)


def verifier_device(qs, acc, curve="pallas") -> None:
    """acc.rs:200-213 in one call (halo_acc_verifier_batch, k = 1), every sponge on the device."""
    cid = _curve(curve)
    acc = Instance(*acc)
    qs, d = _checked_instances(qs, cid)
    verdict, first_bad, *_ = verifier_codes([qs], [acc], d, cid)
    _raise_verdict(int(verdict[0]), int(first_bad[0]), d, acc.d)


def verifier_batch(pairs, curve="pallas", verdicts: bool = False):
    """acc::verifier for many (qs, acc) pairs of one m and one d in one call.  Raises CheckFailed for the first
    failing pair, ``index`` naming the pair; with verdicts=True returns the k codes (halo_acc_verdict_t) instead."""
    cid = _curve(curve)
    if not pairs:
        return np.zeros(0, dtype=np.uint8) if verdicts else None
    groups, accs = [], []
    for qs, a in pairs:
        g, d = _checked_instances(qs, cid)
        groups.append(g)
        accs.append(Instance(*a))
    if any(g[0].d != d for g in groups):
        raise ValueError("verifier_batch needs one degree bound per call")
    codes, first_bad, *_ = verifier_codes(groups, accs, d, cid)
    if verdicts:
        return codes
    for i, (code, fb) in enumerate(zip(codes, first_bad)):
        _raise_verdict(int(code), int(fb), d, accs[i].d, index=i)
    return None


def decider(acc, new_transcript, curve="pallas") -> None:
    """acc.rs:215-217: pcdl::check of the accumulator's instance."""
    acc = Instance(*acc)
    pcdl.check(acc.C, acc.d, acc.z, acc.v, acc.pi, new_transcript("PCDL"), curve)


def decider_batch(accs, rhos=None, curve="pallas", bisect: bool = False) -> None:
    """acc.rs:215-217 for many accumulators at once: pcdl.check_batch of their instances, the transcripts and
    the deciders on the device (rhos -- None, "fs" or the caller's weights -- and bisect as in pcdl.decide_batch).  Raises CheckFailed naming the first
    failing one."""
    pcdl.check_batch([Instance(*a) for a in accs], rhos=rhos, curve=curve, bisect=bisect)
