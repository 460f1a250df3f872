"""Mirror of crates/accumulation/src/pcdl.rs (commit, the IPA round loop, succinct_check and check) on the
MI355X backend.

The Fiat-Shamir transcript (Poseidon sponge, crates/poseidon) stays with the caller: the round loop
of ``open_without_eval`` (pcdl.rs:404-438) asks a ``challenge(xi_prev, L, R) -> xi`` callable for
each round's challenge, exactly where the reference calls ``transcript.challenge()``.  Both sides also exist
without a caller's transcript: ``succinct_check_device`` / ``check_device`` derive the PCDL challenges of a batch
of instances on the device (halo_pcdl_succinct_check_fs_batch), and ``open_device`` /
``open_without_eval_device`` / ``open_device_many`` are the opening in one call with its sponge on the device
(halo_pcdl_open_fs, halo_pcdl_open_fs_dev_multi).
"""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple

import numpy as np

from . import _lib as H
from .group import _curve


def commit(p, d: int, w=None, curve="pallas") -> np.ndarray:
    """pcdl.rs:275-287: n = d + 1 must be a power of two, deg(p) <= d <= D, then
    pedersen::commit(w, Gs[0..n], p.coeffs) over the resident SRS."""
    H.ensure_device()
    c = H.fe_array(p) if len(p) else np.zeros((0, 4), dtype=np.uint64)
    wa = H.fe_array(w, 1) if w is not None else None
    out = np.zeros(8, dtype=np.uint64)
    H.check(H.load().halo_pcdl_commit(_curve(curve), H.ptr(c) if len(c) else None, len(c), d, H.ptr(wa), H.ptr(out)))
    return out


def hiding_blind(q, d: int, z, w_bar, curve="pallas", want_p_bar: bool = True):
    """pcdl.rs:344-355 as one host call (halo_pcdl_hiding_blind): p_bar = (X - z) q for the d
    coefficients q, C_bar = commit(p_bar, d, w_bar) over the resident SRS.  Returns (p_bar, C_bar);
    p_bar is None when it is not asked for."""
    H.ensure_device()
    p_bar = np.zeros((d + 1, 4), dtype=np.uint64) if want_p_bar else None
    C_bar = np.zeros(8, dtype=np.uint64)
    H.check(H.load().halo_pcdl_hiding_blind(_curve(curve), H.ptr(H.fe_array(q, d)), d, H.ptr(H.fe_array(z, 1)),
                                            H.ptr(H.fe_array(w_bar, 1)), H.ptr(p_bar), H.ptr(C_bar)))
    return p_bar, C_bar


def hiding_combine(p, p_bar, d: int, alpha, C, C_bar, w, w_bar, curve="pallas"):
    """pcdl.rs:366-371 as one host call (halo_pcdl_hiding_combine): p' = p + alpha p_bar (p padded to
    d + 1), w' = w + alpha w_bar, C' = C + alpha C_bar - w' S.  Returns (p', w', C')."""
    H.ensure_device()
    pa = H.fe_array(p) if p is not None and len(p) else None
    p_prime = np.zeros((d + 1, 4), dtype=np.uint64)
    w_prime = np.zeros(4, dtype=np.uint64)
    C_prime = np.zeros(8, dtype=np.uint64)
    H.check(H.load().halo_pcdl_hiding_combine(
        _curve(curve), H.ptr(pa), 0 if pa is None else len(pa), H.ptr(H.fe_array(p_bar, d + 1)), d,
        H.ptr(H.fe_array(alpha, 1)), H.ptr(H.point_array(C)), H.ptr(H.point_array(C_bar)), H.ptr(H.fe_array(w, 1)),
        H.ptr(H.fe_array(w_bar, 1)), H.ptr(p_prime), H.ptr(w_prime), H.ptr(C_prime)))
    return p_prime, w_prime, C_prime


class IpaSession:
    """Device-resident (G, c, z) of one opening; mirrors the loop state of pcdl.rs:392-438."""

    def __init__(self, cs, z, H_prime, curve="pallas"):
        H.ensure_device()
        self.curve = _curve(curve)
        cs = H.fe_array(cs)
        self.n = len(cs)
        zz = H.fe_array(z, 1)
        hp = H.point_array(H_prime)
        s = ctypes.c_void_p()
        H.check(H.load().halo_ipa_begin(self.curve, H.ptr(cs), self.n, H.ptr(zz), H.ptr(hp), ctypes.byref(s)))
        self._s = s

    @classmethod
    def with_xi(cls, cs, z, H_point, xi0, curve="pallas") -> "IpaSession":
        """Session whose H' = xi_0 H (pcdl.rs:390-391) is formed on the device (halo_ipa_begin_xi):
        no host scalar multiplication, and the 2^i H table is shared by every opening under H."""
        H.ensure_device()
        self = cls.__new__(cls)
        self.curve = _curve(curve)
        c = H.fe_array(cs)
        self.n = len(c)
        zz = H.fe_array(z, 1)
        hp = H.point_array(H_point)
        x0 = H.fe_array(xi0, 1)
        s = ctypes.c_void_p()
        H.check(H.load().halo_ipa_begin_xi(self.curve, H.ptr(c), self.n, H.ptr(zz), H.ptr(hp), H.ptr(x0),
                                           ctypes.byref(s)))
        self._s = s
        return self

    @classmethod
    def from_vectors(cls, gs, cs, zs, H_prime, curve="pallas") -> "IpaSession":
        """Session over explicit (G, c, z) of length n (a shard of a distributed opening,
        halo_amd.dist.sharded_ipa_rounds)."""
        H.ensure_device()
        self = cls.__new__(cls)
        self.curve = _curve(curve)
        g = H.point_array(gs)
        c = H.fe_array(cs)
        z = H.fe_array(zs)
        if not (len(g) == len(c) == len(z)):
            raise ValueError("G, c and z must have the same length")
        self.n = len(c)
        hp = H.point_array(H_prime)
        s = ctypes.c_void_p()
        H.check(H.load().halo_ipa_begin_vectors(self.curve, H.ptr(g), H.ptr(c), H.ptr(z), self.n, H.ptr(hp),
                                                ctypes.byref(s)))
        self._s = s
        return self

    def _stage(self):
        """Per-session staging arrays with their addresses taken once: a round's ctypes call then
        passes plain integers (numpy's per-call ctypes pointer objects cost a few us each, on a
        ~100 us round of the small openings)."""
        st = getattr(self, "_st", None)
        if st is None:
            lr, xi = np.zeros((2, 8), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
            st = self._st = (lr, lr.ctypes.data, lr.ctypes.data + 64, xi, xi.ctypes.data, H.load())
        return st

    def round_lr(self):
        lr, pl, pr, _, _, lib = self._stage()
        H.check(lib.halo_ipa_round_lr(self._s, pl, pr))
        return lr[0].copy(), lr[1].copy()

    def round_lr_dev(self, d_lr: int, stream: int) -> None:
        """halo_ipa_round_lr_dev: the round's L and R land in the 256 device bytes at d_lr as packed XYZZ,
        ordered before later work on `stream`; no host wait."""
        _, _, _, _, _, lib = self._stage()
        H.check(lib.halo_ipa_round_lr_dev(self._s, ctypes.c_void_p(d_lr), ctypes.c_void_p(stream)))

    def fold(self, xi, xi_inv=None):
        """xi_inv None: the library forms xi^-1 itself (halo_ipa_fold with a NULL xi_inv)."""
        _, _, _, xb, px, lib = self._stage()
        if xi_inv is not None:
            H.check(lib.halo_ipa_fold(self._s, H.ptr(H.fe_array(xi, 1)), H.ptr(H.fe_array(xi_inv, 1))))
            return
        np.copyto(xb, np.asarray(xi, dtype=np.uint64).reshape(4))
        H.check(lib.halo_ipa_fold(self._s, px, None))

    def state(self, with_gs: bool = True):
        """(m, gs, cs, zs): the folded vectors (length 2m).  Sessions over the resident SRS do not
        materialise G in their weighted / tail rounds: with_gs=False there (gs is None)."""
        m = ctypes.c_size_t(0)
        H.check(H.load().halo_ipa_state(self._s, ctypes.byref(m), None, None, None))
        k = max(2 * m.value, 1)
        gs = np.zeros((k, 8), dtype=np.uint64) if with_gs else None
        cs = np.zeros((k, 4), dtype=np.uint64)
        zs = np.zeros((k, 4), dtype=np.uint64)
        H.check(H.load().halo_ipa_state(self._s, ctypes.byref(m), H.ptr(gs) if with_gs else None, H.ptr(cs),
                                        H.ptr(zs)))
        return m.value, gs, cs, zs

    def end(self):
        U = np.zeros(8, dtype=np.uint64)
        c = np.zeros(4, dtype=np.uint64)
        # halo_ipa_end returns the session to the pool even when it reports an error, so the handle
        # is dropped first: no caller path can end (release) it a second time
        s, self._s = self._s, None
        H.check(H.load().halo_ipa_end(s, H.ptr(U), H.ptr(c)))
        return U, c

    @staticmethod
    def end_many(sessions):
        """end() of lockstep sessions in one halo_ipa_end_multi call (their final U sums overlap on the
        device); [(U, c)] in order."""
        k = len(sessions)
        U = np.zeros((k, 8), dtype=np.uint64)
        c = np.zeros((k, 4), dtype=np.uint64)
        handles = [s_._s for s_ in sessions]
        # the library's argument checks first, here: they release nothing, so the handles must stay
        if any(h is None for h in handles):
            raise ValueError("end_many: a session was already ended")
        if len({h.value for h in handles}) != k:
            raise ValueError("end_many: a session is listed twice")
        arr = (ctypes.c_void_p * k)(*[h.value for h in handles])
        rc = H.load().halo_ipa_end_multi(arr, k, H.ptr(U), H.ptr(c))
        # past its argument checks the call releases every session, also on an error (halo_gpu.h); an
        # argument error (its own "halo_ipa_end_multi:" messages) releases none, and the handles stay
        # with their wrappers so that end() can still release them
        if rc == H.HALO_OK or not H.last_error().startswith("halo_ipa_end_multi:"):
            for s_ in sessions:
                s_._s = None
        H.check(rc)
        return [(U[i].copy(), c[i].copy()) for i in range(k)]


def ipa_rounds(cs, z, H_prime, challenge: Callable, inverse: Callable, curve="pallas"):
    """The round loop of open_without_eval (pcdl.rs:392-450) given p'.coeffs resized to n, z, H' and
    the caller's transcript.  ``challenge(xi_prev, L, R)`` returns the next xi (ark limbs, shape (4,));
    ``inverse(xi)`` returns xi^-1.  Returns (Ls, Rs, U, c)."""
    ses = IpaSession(cs, z, H_prime, curve)
    n = ses.n
    lg_n = n.bit_length() - 1
    Ls, Rs = [], []
    xi = None
    for _ in range(lg_n):
        L, R = ses.round_lr()
        Ls.append(L)
        Rs.append(R)
        xi = challenge(xi, L, R)
        ses.fold(xi, inverse(xi))
    U, c = ses.end()
    return Ls, Rs, U, c


_SCALAR = {0: 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001,   # Pallas: Fp
           1: 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001}   # Vesta: Fq


def _ark_inverse(x: np.ndarray, cid: int) -> np.ndarray:
    """x^-1 for an ark Montgomery scalar (x R -> x^-1 R), host big integers."""
    r = _SCALAR[cid]
    v = int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192
    inv = pow(v, -1, r) * pow(2, 512, r) % r  # (x R)^-1 R^2 = x^-1 R: one modular inverse
    return np.array([(inv >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def open_without_eval(p, C, d: int, z, v, w=None, transcript=None, q=None, w_bar=None, curve="pallas") -> dict:
    """pcdl::open_without_eval (pcdl.rs:326-453) on the device, hiding branch included.

    p: coefficients (ark scalars, degree <= d); C its commitment; z, v ark scalars; w the commitment
    randomness (None: non-hiding).  ``transcript`` is the caller's Fiat-Shamir sponge with the
    reference's interface (outer_sponge.rs: absorb_g(points), absorb_fr(scalars), challenge()) over
    WrappedPoints / ark scalars -- a fresh PCDL sponge, as pcdl.rs:336 creates; it is required
    (``halo_amd.sponge.Sponge(curve, "PCDL")`` is the library's own).  q (d coefficients) and w_bar are the random draws the
    reference takes from its rng (pcdl.rs:347,352).  p, p_bar and p' stay in the session's device
    buffers from the blind to the rounds (halo_pcdl_open_begin / _blind / _combine / _start).
    Returns the EvalProof: dict(Ls, Rs, U, c, C_bar, w_prime)."""
    if transcript is None:
        raise ValueError("open_without_eval needs the caller's PCDL transcript (pcdl.rs:336 Sponge::new(PCDL))")
    H.ensure_device()
    L = H.load()
    cid = _curve(curve)
    n = d + 1
    p = H.fe_array(p) if len(p) else np.zeros((0, 4), dtype=np.uint64)
    zz = H.fe_array(z, 1)[0]
    vv = H.fe_array(v, 1)[0] if v is not None else None
    C = H.point_array(C).reshape(8)
    s = ctypes.c_void_p()
    # asserts n > 1, n a power of two, p.degree() <= d, d <= D (pcdl.rs:338-341)
    v_out = np.zeros(4, dtype=np.uint64) if v is None else None  # pcdl::open: v = p(z) on the device
    H.check(L.halo_pcdl_open_begin(cid, H.ptr(p) if len(p) else None, len(p), d, H.ptr(zz), H.ptr(v_out),
                                   ctypes.byref(s)))
    if v is None:
        vv = v_out
    ses = IpaSession.__new__(IpaSession)
    ses.curve, ses.n, ses._s = cid, n, s
    try:
        C_bar = w_prime = None
        if w is not None:
            C_bar = np.zeros(8, dtype=np.uint64)
            H.check(L.halo_pcdl_open_blind(s, H.ptr(H.fe_array(q, d)), H.ptr(H.fe_array(w_bar, 1)), H.ptr(C_bar)))
            transcript.absorb_g([C, C_bar])
            transcript.absorb_fr([zz, vv])
            alpha = np.ascontiguousarray(transcript.challenge(), dtype=np.uint64)
            w_prime = np.zeros(4, dtype=np.uint64)
            C_prime = np.zeros(8, dtype=np.uint64)
            H.check(L.halo_pcdl_open_combine(s, H.ptr(alpha), H.ptr(C), H.ptr(H.fe_array(w, 1)), H.ptr(w_prime),
                                             H.ptr(C_prime)))
        else:
            C_prime = C
        transcript.absorb_g([C_prime])
        transcript.absorb_fr([zz, vv])
        xi = np.ascontiguousarray(transcript.challenge(), dtype=np.uint64)
        H.check(L.halo_pcdl_open_start(s, None, H.ptr(xi)))  # H' = xi_0 pp.H (pcdl.rs:390)
        Ls, Rs = [], []
        for _ in range(n.bit_length() - 1):
            Lp, Rp = ses.round_lr()
            Ls.append(Lp)
            Rs.append(Rp)
            transcript.absorb_fr([xi])
            transcript.absorb_g([Lp, Rp])
            xi = np.ascontiguousarray(transcript.challenge(), dtype=np.uint64)
            ses.fold(xi)  # xi^-1 formed by the library (pcdl.rs:430)
        U, c = ses.end()
    finally:
        if ses._s is not None:  # an assertion or error above: return the session to the pool
            L.halo_ipa_end(ses._s, None, None)
            ses._s = None
    return {"Ls": Ls, "Rs": Rs, "U": U, "c": c, "C_bar": C_bar, "w_prime": w_prime, "v": vv}


class StandInTranscript:
    """A stand-in for the reference's Poseidon PCDL sponge (outer_sponge.rs) with its interface, for
    timing runs only: challenges are SHA-256 of everything absorbed, reduced mod r.  (The Fiat-Shamir
    transcript is host logic outside the device path; tests drive the device with the restated
    Poseidon sponge, tests/test_gpu_transcript.py.)"""

    def __init__(self, curve="pallas"):
        import hashlib
        self._h = hashlib.sha256(b"PCDL")
        self._r = _SCALAR[_curve(curve)]

    def absorb_g(self, pts):
        for q in pts:
            self._h.update(np.ascontiguousarray(q, dtype=np.uint64).tobytes())

    def absorb_fr(self, xs):
        for x in xs:
            self._h.update(np.ascontiguousarray(x, dtype=np.uint64).tobytes())

    def challenge(self) -> np.ndarray:
        d = self._h.digest()
        self._h.update(d)
        v = (int.from_bytes(d, "little") % self._r) or 1
        m = v * (1 << 256) % self._r
        return np.array([(m >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def evaluate(p, z, curve="pallas") -> np.ndarray:
    """DensePolynomial::evaluate (pcdl.rs:49,471) on the device (halo_poly_eval_batch)."""
    import ctypes as _ct
    H.ensure_device()
    c = H.fe_array(p)
    out = np.zeros((1, 4), dtype=np.uint64)
    ptrs = (_ct.c_void_p * 1)(c.ctypes.data)
    lens = (_ct.c_size_t * 1)(len(c))
    field = H.FP if _curve(curve) == 0 else H.FQ
    H.check(H.load().halo_poly_eval_batch(field, ptrs, lens, 1, H.ptr(H.fe_array(z, 1)), H.ptr(out)))
    return out[0]


def open(p, C, d: int, z, w=None, transcript=None, q=None, w_bar=None, curve="pallas") -> dict:  # noqa: A001
    """pcdl::open (pcdl.rs:463-473): v = p(z) (evaluated on the device inside the session start,
    halo_pcdl_open_begin), then open_without_eval.  The EvalProof dict carries v."""
    return open_without_eval(p, C, d, z, None, w=w, transcript=transcript, q=q, w_bar=w_bar, curve=curve)


def open_without_eval_device(p, C, d: int, z, v, w=None, q=None, w_bar=None, curve="pallas") -> dict:
    """pcdl::open_without_eval (pcdl.rs:326-453) in one call with the PCDL transcript on the device
    (halo_pcdl_open_fs): no caller's sponge and no host trip per round.  The arguments and the returned
    EvalProof dict are open_without_eval's; v None is pcdl::open (v = p(z) on the device).
    halo_poseidon_set_params must have installed the parameters of the curve's base field."""
    H.ensure_device()
    cid = _curve(curve)
    lg = (d + 1).bit_length() - 1
    p = H.fe_array(p) if len(p) else np.zeros((0, 4), dtype=np.uint64)
    hid = w is not None
    Ls, Rs = np.zeros((max(lg, 1), 8), dtype=np.uint64), np.zeros((max(lg, 1), 8), dtype=np.uint64)
    U, c, v_out = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    C_bar = np.zeros(8, dtype=np.uint64) if hid else None
    w_prime = np.zeros(4, dtype=np.uint64) if hid else None
    H.check(H.load().halo_pcdl_open_fs(
        cid, H.ptr(p) if len(p) else None, len(p), d, H.ptr(H.fe_array(z, 1)),
        H.ptr(H.fe_array(v, 1)) if v is not None else None, H.ptr(H.point_array(C).reshape(8)),
        H.ptr(H.fe_array(w, 1)) if hid else None, H.ptr(H.fe_array(q, d)) if hid and q is not None else None,
        H.ptr(H.fe_array(w_bar, 1)) if hid and w_bar is not None else None, H.ptr(Ls), H.ptr(Rs), H.ptr(U), H.ptr(c),
        H.ptr(C_bar), H.ptr(w_prime), H.ptr(v_out)))
    return {"Ls": [Ls[j].copy() for j in range(lg)], "Rs": [Rs[j].copy() for j in range(lg)], "U": U, "c": c,
            "C_bar": C_bar, "w_prime": w_prime, "v": v_out}


def open_device(p, C, d: int, z, w=None, q=None, w_bar=None, curve="pallas") -> dict:
    """pcdl::open (pcdl.rs:463-473) in one call with the transcript on the device: open_without_eval_device with
    v = p(z) formed on the device."""
    return open_without_eval_device(p, C, d, z, None, w=w, q=q, w_bar=w_bar, curve=curve)


def open_device_many(ps, Cs, d: int, zs, curve="pallas") -> list:
    """k plain pcdl::open calls of one degree bound over device-resident coefficient vectors
    (halo_pcdl_open_fs_dev_multi): ps are k torch device tensors of ark scalars (int64, 4 words per
    coefficient, at most d + 1 coefficients), Cs their commitments (k, 8), zs the points (k, 4).  Every
    opening's whole chain of launches is enqueued before any is waited for.  Returns k EvalProof dicts."""
    import torch
    H.ensure_device()
    k = len(ps)
    if k == 0:
        return []
    lg = (d + 1).bit_length() - 1
    ts = [t.contiguous() for t in ps]
    torch.cuda.current_stream().synchronize()  # the library orders its reads after the null stream only
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
    lens = (ctypes.c_size_t * k)(*[t.numel() // 4 for t in ts])
    Ls, Rs = np.zeros((k, max(lg, 1), 8), dtype=np.uint64), np.zeros((k, max(lg, 1), 8), dtype=np.uint64)
    U, c, v = np.zeros((k, 8), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64)
    if lg:
        Ls, Rs = Ls.reshape(k * lg, 8), Rs.reshape(k * lg, 8)
    H.check(H.load().halo_pcdl_open_fs_dev_multi(_curve(curve), k, ptrs, lens, d, H.ptr(H.fe_array(zs, k)),
                                                 H.ptr(H.point_array(Cs)), H.ptr(Ls), H.ptr(Rs), H.ptr(U), H.ptr(c),
                                                 H.ptr(v)))
    return [{"Ls": [Ls[i * lg + j].copy() for j in range(lg)], "Rs": [Rs[i * lg + j].copy() for j in range(lg)],
             "U": U[i].copy(), "c": c[i].copy(), "C_bar": None, "w_prime": None, "v": v[i].copy()} for i in range(k)]


class HPoly:
    """pcdl.rs:184-229 HPoly: h(X) = prod_{i < lg n} (1 + xi_{lg n - i} X^(2^i)) from the round
    challenges xis (ark Montgomery scalars, xis[0] unused by h as in the reference)."""

    def __init__(self, xis, curve="pallas"):
        self.curve = _curve(curve)
        self.field = H.FP if self.curve == 0 else H.FQ
        self.xis = H.fe_array(xis)

    def get_poly(self) -> np.ndarray:
        """Coefficients (2^(len(xis) - 1) of them), generated on the device (halo_hpoly_coeffs)."""
        H.ensure_device()
        n = 1 << (len(self.xis) - 1)
        out = np.zeros((n, 4), dtype=np.uint64)
        H.check(H.load().halo_hpoly_coeffs(self.field, H.ptr(self.xis), len(self.xis), H.ptr(out)))
        return out

    def eval(self, z) -> np.ndarray:  # noqa: A003
        """HPoly::eval (pcdl.rs:222-235): lg n products on the host."""
        r = _SCALAR[self.curve]
        r_inv = pow(1 << 256, -1, r)
        x = [_ark_int(v) * r_inv % r for v in self.xis]
        zi = _ark_int(z) * r_inv % r
        lg_n = len(x) - 1
        v = (1 + x[lg_n] * zi) % r
        for i in range(1, lg_n):
            zi = zi * zi % r
            v = v * (1 + x[lg_n - i] * zi) % r
        return _ark_limbs(v * (1 << 256) % r)

    @staticmethod
    def combine(hs: list["HPoly"], alphas) -> np.ndarray:
        """sum_i alphas[i] * h_i(X) (acc.rs:89), trimmed like DensePolynomial."""
        H.ensure_device()
        k = len(hs)
        xis = np.ascontiguousarray(np.concatenate([h.xis for h in hs]))
        a = H.fe_array(alphas, k)
        n = 1 << (len(hs[0].xis) - 1)
        out = np.zeros((n, 4), dtype=np.uint64)
        m = ctypes.c_size_t(0)
        H.check(H.load().halo_hpoly_combine(hs[0].field, H.ptr(xis), k, len(hs[0].xis), H.ptr(a), H.ptr(out),
                                            ctypes.byref(m)))
        return out[: m.value]


def decider_commit(xis, d: int, curve="pallas") -> np.ndarray:
    """pcdl.rs:579 (check step 5): pedersen::commit(None, &pp.Gs[0..d+1], &h.get_poly().coeffs)."""
    H.ensure_device()
    x = H.fe_array(xis)
    out = np.zeros(8, dtype=np.uint64)
    H.check(H.load().halo_pcdl_decider_commit(_curve(curve), H.ptr(x), len(x), d, H.ptr(out)))
    return out


class CheckFailed(Exception):
    """A verifier's ``ensure!`` failed (pcdl.rs:494,547,580; acc.rs:154,207-210): the message is the
    reference's.  ``index``: the failing instance of a batch (None for a single check)."""

    def __init__(self, msg: str, index: int | None = None):
        super().__init__(msg if index is None else f"{msg} (instance {index})")
        self.msg = msg
        self.index = index


class Instance(NamedTuple):
    """pcdl.rs Instance: ((C, d, z, v), pi), pi the EvalProof dict of ``open`` (Ls, Rs, U, c, C_bar, w_prime)."""
    C: np.ndarray
    d: int
    z: np.ndarray
    v: np.ndarray
    pi: dict


SUCCINCT_MSG = "C_(log_n) \u2260 CM.Commit_\u03a3(c || v')"
DECIDER_MSG = "U \u2260 CM.Commit(ck, h_vec)"


def _ark_int(x) -> int:
    x = np.asarray(x, dtype=np.uint64).reshape(4)
    return int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192


def _ark_limbs(v: int) -> np.ndarray:
    return np.array([(v >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def _ark_neg(x, cid: int) -> np.ndarray:
    """-x for an ark Montgomery scalar (the Montgomery form is linear)."""
    return _ark_limbs((_SCALAR[cid] - _ark_int(x)) % _SCALAR[cid])


def point_lincomb(pts, scalars, add=None, curve="pallas") -> np.ndarray:
    """out[i] = add[i] + sum_j scalars[i, j] pts[i, j] for k items of t terms (halo_point_lincomb_batch):
    pts (k, t, 8) WrappedPoints, scalars (k, t, 4) ark scalars, add (k, 8) or None.  Returns (k, 8)."""
    H.ensure_device()
    p = np.ascontiguousarray(np.asarray(pts, dtype=np.uint64))
    k, t = p.shape[0], p.shape[1]
    sc = np.ascontiguousarray(np.asarray(scalars, dtype=np.uint64).reshape(k, t, 4))
    a = np.ascontiguousarray(np.asarray(add, dtype=np.uint64).reshape(k, 8)) if add is not None else None
    out = np.zeros((k, 8), dtype=np.uint64)
    H.check(H.load().halo_point_lincomb_batch(_curve(curve), H.ptr(a), H.ptr(p) if t else None, H.ptr(sc) if t else None,
                                              k, t, H.ptr(out)))
    return out


def succinct_check_verdicts(C_primes, d: int, zs, vs, xis, Ls, Rs, Us, cs, curve="pallas") -> np.ndarray:
    """halo_pcdl_succinct_check_batch: steps 5-10 of succinct_check for k instances of degree bound d given
    their challenges xis (k, lg n + 1).  Returns k bytes, 1 where C_(lg n) == c U + v' H'."""
    H.ensure_device()
    Cp = H.point_array(C_primes)
    k = len(Cp)
    lg = (d + 1).bit_length() - 1
    ok = np.zeros(k, dtype=np.uint8)
    H.check(H.load().halo_pcdl_succinct_check_batch(
        _curve(curve), d, k, H.ptr(Cp), H.ptr(H.fe_array(zs, k)), H.ptr(H.fe_array(vs, k)),
        H.ptr(H.fe_array(xis, k * (lg + 1))), H.ptr(H.point_array(Ls)) if lg else None,
        H.ptr(H.point_array(Rs)) if lg else None, H.ptr(H.point_array(Us)), H.ptr(H.fe_array(cs, k)), H.ptr(ok)))
    return ok


def succinct_check_many(instances, transcripts, curve="pallas"):
    """pcdl::succinct_check (pcdl.rs:483-554) for many instances at once.  instances: (C, d, z, v, pi) each
    (``Instance``); transcripts: one fresh PCDL sponge per instance (pcdl.rs:496), with the reference's
    interface.  Every challenge is derived on the host in the reference's absorb order; the hiding
    instances' C' = C + alpha C_bar - w' S come from one halo_point_lincomb_batch call and all verdicts
    from one halo_pcdl_succinct_check_batch call per distinct d.  Returns [(HPoly, U)]; raises CheckFailed
    naming the first failing instance."""
    from .group import PublicParams
    H.ensure_device()
    cid = _curve(curve)
    insts = [Instance(*q) for q in instances]
    ts = list(transcripts)
    if len(ts) != len(insts):
        raise ValueError("succinct_check_many needs one PCDL transcript per instance")
    D = PublicParams.len(cid) - 1
    for i, q in enumerate(insts):
        n = q.d + 1
        if n & (n - 1) or n == 0:
            raise H.HaloAssertion(4, f"n ({n}) is not a power of two")
        if q.d > D:
            raise CheckFailed("d was larger than D!", i)
    zs = [H.fe_array(q.z, 1)[0] for q in insts]
    vs = [H.fe_array(q.v, 1)[0] for q in insts]
    Cs = [H.point_array(q.C).reshape(8) for q in insts]
    # 3-4. alpha and C' of the hiding instances (pcdl.rs:506-515)
    C_primes = list(Cs)
    hid = [i for i, q in enumerate(insts) if q.pi.get("C_bar") is not None]
    if hid:
        S, _ = PublicParams.sh(cid)
        pts, sc = [], []
        for i in hid:
            pi = insts[i].pi
            C_bar = H.point_array(pi["C_bar"]).reshape(8)
            ts[i].absorb_g([Cs[i], C_bar])
            ts[i].absorb_fr([zs[i], vs[i]])
            alpha = np.ascontiguousarray(ts[i].challenge(), dtype=np.uint64)
            pts.append([C_bar, S])
            sc.append([alpha, _ark_neg(pi["w_prime"], cid)])
        out = point_lincomb(np.array(pts), np.array(sc), add=np.array([Cs[i] for i in hid]), curve=cid)
        for i, cp in zip(hid, out):
            C_primes[i] = cp
    # 5, 7.a the challenges xi_0 .. xi_lg_n (pcdl.rs:518-534)
    xis = []
    for i, q in enumerate(insts):
        t = ts[i]
        lg = (q.d + 1).bit_length() - 1
        Ls, Rs = H.point_array(q.pi["Ls"]), H.point_array(q.pi["Rs"])
        if len(Ls) != lg or len(Rs) != lg:
            raise ValueError(f"instance {i}: the proof has {len(Ls)} rounds, d = {q.d} needs {lg}")
        t.absorb_g([C_primes[i]])
        t.absorb_fr([zs[i], vs[i]])
        x = [np.ascontiguousarray(t.challenge(), dtype=np.uint64)]
        for j in range(lg):
            t.absorb_fr([x[j]])
            t.absorb_g([Ls[j], Rs[j]])
            x.append(np.ascontiguousarray(t.challenge(), dtype=np.uint64))
        xis.append(np.stack(x))
    # 6, 7.b, 9, 10 on the device, one call per degree bound
    ok = np.zeros(len(insts), dtype=np.uint8)
    for d in sorted({q.d for q in insts}):
        idx = [i for i, q in enumerate(insts) if q.d == d]
        ok[idx] = succinct_check_verdicts(
            np.stack([C_primes[i] for i in idx]), d, np.stack([zs[i] for i in idx]), np.stack([vs[i] for i in idx]),
            np.concatenate([xis[i] for i in idx]),
            np.concatenate([H.point_array(insts[i].pi["Ls"]) for i in idx]) if d else None,
            np.concatenate([H.point_array(insts[i].pi["Rs"]) for i in idx]) if d else None,
            np.stack([H.point_array(insts[i].pi["U"]).reshape(8) for i in idx]),
            np.stack([H.fe_array(insts[i].pi["c"], 1)[0] for i in idx]), curve=cid)
    for i in range(len(insts)):
        if not ok[i]:
            raise CheckFailed(SUCCINCT_MSG, i)
    return [(HPoly(xis[i], cid), H.point_array(q.pi["U"]).reshape(8).copy()) for i, q in enumerate(insts)]


def succinct_check(C, d: int, z, v, pi: dict, transcript, curve="pallas"):
    """pcdl::succinct_check (pcdl.rs:483-554) under the caller's fresh PCDL sponge.  Returns (HPoly, U);
    raises CheckFailed("C_(log_n) != CM.Commit_Sigma(c || v')", in the reference's spelling)."""
    try:
        return succinct_check_many([Instance(C, d, z, v, pi)], [transcript], curve)[0]
    except CheckFailed as e:
        raise CheckFailed(e.msg) from None


def check(C, d: int, z, v, pi: dict, transcript, curve="pallas") -> None:
    """pcdl::check (pcdl.rs:563-583): succinct_check, then U == CM.Commit(ck, h_vec) over Gs[0..d]."""
    h, U = succinct_check(C, d, z, v, pi, transcript, curve)
    if not np.array_equal(decider_commit(h.xis, d, curve), U):
        raise CheckFailed(DECIDER_MSG)


def succinct_check_fs_verdicts(Cs, d: int, zs, vs, Ls, Rs, Us, cs, hiding=None, C_bars=None, w_primes=None,
                               curve="pallas"):
    """halo_pcdl_succinct_check_fs_batch: succinct_check of k raw instances of degree bound d, their transcripts
    on the device.  hiding: k flags (None: no instance hides); C_bars (k, 8) and w_primes (k, 4) are read
    where the flag is set.  Returns (ok, xis, alphas): k bytes, (k, lg n + 1, 4) challenges, (k, 4) alphas
    (zero where the instance does not hide).  halo_poseidon_set_params must have installed the parameters
    of the curve's base field."""
    H.ensure_device()
    C = H.point_array(Cs)
    k = len(C)
    lg = (d + 1).bit_length() - 1
    ok = np.zeros(k, dtype=np.uint8)
    xis = np.zeros((k, lg + 1, 4), dtype=np.uint64)
    alphas = np.zeros((k, 4), dtype=np.uint64)
    hid = cb = wp = None
    if hiding is not None:
        hid = np.ascontiguousarray(np.asarray(hiding, dtype=np.uint8).reshape(k))
        cb, wp = H.point_array(C_bars), H.fe_array(w_primes, k)
        assert len(cb) == k
    H.check(H.load().halo_pcdl_succinct_check_fs_batch(
        _curve(curve), d, k, H.ptr(C), H.ptr(H.fe_array(zs, k)), H.ptr(H.fe_array(vs, k)),
        H.ptr(H.point_array(Ls)) if lg else None, H.ptr(H.point_array(Rs)) if lg else None, H.ptr(H.point_array(Us)),
        H.ptr(H.fe_array(cs, k)), H.ptr(hid), H.ptr(cb), H.ptr(wp), H.ptr(xis), H.ptr(alphas), H.ptr(ok)))
    return ok, xis, alphas


def _check_shapes(insts, cid: int) -> None:
    """What succinct_check asserts before any device call (pcdl.rs:491-494), for every instance of a list."""
    from .group import PublicParams
    D = PublicParams.len(cid) - 1
    for i, q in enumerate(insts):
        n = q.d + 1
        if n & (n - 1) or n == 0:
            raise H.HaloAssertion(4, f"n ({n}) is not a power of two")
        if q.d > D:
            raise CheckFailed("d was larger than D!", i)
        lg = n.bit_length() - 1
        if len(H.point_array(q.pi["Ls"])) != lg or len(H.point_array(q.pi["Rs"])) != lg:
            raise ValueError(f"instance {i}: the proof has {len(q.pi['Ls'])} rounds, d = {q.d} needs {lg}")


def instance_rows(qs, d: int) -> list:
    """The arrays of halo_pcdl_succinct_check_fs_batch for a list of instances of one degree bound d, in its
    argument order: C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime.  Ls / Rs are None at d = 0; the last three are
    None when no instance hides, else C_bar / w_prime are zero where the flag is not set."""
    hid = [q.pi.get("C_bar") is not None for q in qs]
    zero_pt, zero_fe = np.zeros(8, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    rows = [np.stack([H.point_array(q.C).reshape(8) for q in qs]), np.stack([H.fe_array(q.z, 1)[0] for q in qs]),
            np.stack([H.fe_array(q.v, 1)[0] for q in qs]),
            np.ascontiguousarray(np.concatenate([H.point_array(q.pi["Ls"]) for q in qs])) if d else None,
            np.ascontiguousarray(np.concatenate([H.point_array(q.pi["Rs"]) for q in qs])) if d else None,
            np.stack([H.point_array(q.pi["U"]).reshape(8) for q in qs]), np.stack([H.fe_array(q.pi["c"], 1)[0] for q in qs])]
    if not any(hid):
        return rows + [None, None, None]
    return rows + [np.array(hid, dtype=np.uint8),
                   np.stack([H.point_array(q.pi["C_bar"]).reshape(8) if h else zero_pt for q, h in zip(qs, hid)]),
                   np.stack([H.fe_array(q.pi["w_prime"], 1)[0] if h else zero_fe for q, h in zip(qs, hid)])]


def succinct_check_device(instances, curve="pallas"):
    """succinct_check_many without transcripts: the device derives every challenge itself
    (halo_pcdl_succinct_check_fs_batch, one call per distinct d).  Returns [(HPoly, U)]; raises CheckFailed
    naming the first failing instance."""
    H.ensure_device()
    cid = _curve(curve)
    insts = [Instance(*q) for q in instances]
    _check_shapes(insts, cid)
    ok = np.zeros(len(insts), dtype=np.uint8)
    xis = [None] * len(insts)
    for d in sorted({q.d for q in insts}):
        idx = [i for i, q in enumerate(insts) if q.d == d]
        qs = [insts[i] for i in idx]
        C, z, v, Ls, Rs, U, c, hid, cb, wp = instance_rows(qs, d)
        ok_d, xis_d, _ = succinct_check_fs_verdicts(C, d, z, v, Ls, Rs, U, c, hiding=hid, C_bars=cb, w_primes=wp, curve=cid)
        for j, i in enumerate(idx):
            ok[i], xis[i] = ok_d[j], xis_d[j]
    for i in range(len(insts)):
        if not ok[i]:
            raise CheckFailed(SUCCINCT_MSG, i)
    return [(HPoly(xis[i], cid), H.point_array(q.pi["U"]).reshape(8).copy()) for i, q in enumerate(insts)]


def check_device(C, d: int, z, v, pi: dict, curve="pallas") -> None:
    """pcdl::check (pcdl.rs:563-583) with the transcript on the device: succinct_check_device, then
    U == CM.Commit(ck, h_vec) over Gs[0..d]."""
    try:
        h, U = succinct_check_device([Instance(C, d, z, v, pi)], curve)[0]
    except CheckFailed as e:
        raise CheckFailed(e.msg) from None
    if not np.array_equal(decider_commit(h.xis, d, curve), U):
        raise CheckFailed(DECIDER_MSG)


def decide_rho(xis, Us, d: int, live=None, curve="pallas") -> np.ndarray:
    """halo_pcdl_decide_rho: the weights that rhos="fs" stands for, derived on the device from the batch itself
    (d, k, the live flags and every live instance's U and xi_1 .. xi_lg n) by Fiat-Shamir over the curve's sponge;
    include/halo_gpu.h states the derivation and its soundness bound.  xis, Us, live as in decide_batch.  Returns
    (k, 4) ark scalars: nonzero where the instance is live, zero where it is not.  Needs the Poseidon parameters
    (schnorr.set_poseidon_params) and no SRS."""
    H.ensure_device()
    U = H.point_array(Us)
    k = len(U)
    lg = (d + 1).bit_length() - 1
    out = np.zeros((k, 4), dtype=np.uint64)
    lv = np.ascontiguousarray(np.asarray(live, dtype=np.uint8).reshape(k)) if live is not None else None
    H.check(H.load().halo_pcdl_decide_rho(_curve(curve), d, k, H.ptr(H.fe_array(xis, k * (lg + 1))), H.ptr(U), H.ptr(lv),
                                          H.ptr(out)))
    return out


def decide_batch(xis, Us, d: int, rhos=None, live=None, curve="pallas", bisect: bool = False) -> np.ndarray:
    """halo_pcdl_decide_batch: acc::decider for k instances of degree bound d.  xis (k, lg n + 1, 4) challenges
    (the layout succinct_check_fs_verdicts returns), Us (k, 8).  rhos None: one commitment per instance (exact
    mode); rhos "fs": one random linear combination and one MSM under weights that the device derives from the
    batch itself by Fiat-Shamir (decide_rho; no random number generator is needed, and two runs agree), with an
    exact rerun if it fails, or with bisect=True a descent through the halves that fail (one MSM per failing node;
    tuning key decide_bisect); rhos (k, 4): the same under the caller's own weights, nonzero scalars drawn
    uniformly AFTER the proofs were fixed.  live: k flags, 0 skips the instance (verdict 0).  Returns k bytes, 1
    where U == CM.Commit(ck, h_vec)."""
    H.ensure_device()
    U = H.point_array(Us)
    k = len(U)
    lg = (d + 1).bit_length() - 1
    ok = np.zeros(k, dtype=np.uint8)
    lv = np.ascontiguousarray(np.asarray(live, dtype=np.uint8).reshape(k)) if live is not None else None
    rh, derive = H.fs_rhos(rhos, k)
    with H.bisecting(bisect), H.deriving(derive):
        H.check(H.load().halo_pcdl_decide_batch(_curve(curve), d, k, H.ptr(H.fe_array(xis, k * (lg + 1))), H.ptr(U),
                                                H.ptr(lv), H.ptr(rh), H.ptr(ok)))
    return ok


def check_fs_codes(Cs, d: int, zs, vs, Ls, Rs, Us, cs, hiding=None, C_bars=None, w_primes=None, rhos=None,
                   curve="pallas", bisect: bool = False) -> np.ndarray:
    """halo_pcdl_check_fs_batch: pcdl::check of k raw instances of degree bound d (the arguments of
    succinct_check_fs_verdicts, plus rhos and bisect as in decide_batch).  Returns k codes: 0 accept, 1 the succinct check
    failed, 2 the decider failed."""
    H.ensure_device()
    C = H.point_array(Cs)
    k = len(C)
    lg = (d + 1).bit_length() - 1
    code = np.zeros(k, dtype=np.uint8)
    hid = cb = wp = None
    if hiding is not None:
        hid = np.ascontiguousarray(np.asarray(hiding, dtype=np.uint8).reshape(k))
        cb, wp = H.point_array(C_bars), H.fe_array(w_primes, k)
        assert len(cb) == k
    rh, derive = H.fs_rhos(rhos, k)
    with H.bisecting(bisect), H.deriving(derive):
        H.check(H.load().halo_pcdl_check_fs_batch(
            _curve(curve), d, k, H.ptr(C), H.ptr(H.fe_array(zs, k)), H.ptr(H.fe_array(vs, k)),
            H.ptr(H.point_array(Ls)) if lg else None, H.ptr(H.point_array(Rs)) if lg else None, H.ptr(H.point_array(Us)),
            H.ptr(H.fe_array(cs, k)), H.ptr(hid), H.ptr(cb), H.ptr(wp), H.ptr(rh), H.ptr(code)))
    return code


def check_batch(instances, rhos=None, curve="pallas", verdicts: bool = False, bisect: bool = False):
    """pcdl::check (pcdl.rs:563-583) for many instances (C, d, z, v, pi), every transcript and every decider on
    the device: one halo_pcdl_check_fs_batch call per distinct d.  rhos: None for exact deciders, "fs" for
    weights derived on the device (each call, i.e. each d, derives its own), or one nonzero scalar per instance
    drawn by the caller after the proofs were fixed (decide_batch); bisect as in decide_batch.  Raises
    CheckFailed(msg, index) for the first failing instance; with verdicts=True returns the codes instead
    (0 accept, 1 succinct check, 2 decider) and raises only for a d beyond the SRS."""
    H.ensure_device()
    cid = _curve(curve)
    insts = [Instance(*q) for q in instances]
    rh, derive = H.fs_rhos(rhos, len(insts))
    _check_shapes(insts, cid)
    codes = np.zeros(len(insts), dtype=np.uint8)
    for d in sorted({q.d for q in insts}):
        idx = [i for i, q in enumerate(insts) if q.d == d]
        qs = [insts[i] for i in idx]
        C, z, v, Ls, Rs, U, c, hid, cb, wp = instance_rows(qs, d)
        codes[idx] = check_fs_codes(C, d, z, v, Ls, Rs, U, c, hiding=hid, C_bars=cb, w_primes=wp,
                                    rhos="fs" if derive else rh[idx] if rh is not None else None, curve=cid,
                                    bisect=bisect)
    if verdicts:
        return codes
    for i, c in enumerate(codes):
        if c:
            raise CheckFailed(SUCCINCT_MSG if c == 1 else DECIDER_MSG, i)
    return None


WIRE_MSG = "the bytes do not deserialize"


def check_bytes(buf, rhos=None, vec: bool = False, curve="pallas", verdicts: bool = False, bisect: bool = False):
    """pcdl::check for the instances of a serialized buffer (ark-serialize compressed bytes: concatenated Instances,
    or with vec=True a Vec<Instance>): the layout is walked on the host, the points and scalars are decoded on the
    device (halo_pcdl_instances_decode_dev) and checked there (halo_pcdl_check_fs_batch_dev), one pair of calls per
    distinct d, the decoded arrays staying on the device.  rhos and bisect as in check_batch.  Codes: those of
    check_batch, plus 3: the bytes of that instance do not deserialize (a point or scalar the format refuses), where
    the reference's deserialize_compressed returns Err.  A buffer whose structure is broken (truncated, a bad length
    or tag) raises HaloError with the walk's message before any launch.  Without verdicts: raises CheckFailed with
    the reference's messages for 1 / 2 and ValueError naming the instance for 3."""
    from . import wire
    codes = wire.check_codes(buf, rhos=rhos, vec=vec, curve=curve, bisect=bisect)
    if verdicts:
        return codes
    for i, c in enumerate(codes):
        if c == 3:
            raise ValueError(f"instance {i}: {WIRE_MSG}")
        if c:
            raise CheckFailed(SUCCINCT_MSG if c == 1 else DECIDER_MSG, i)
    return None


def trace_commit_batch(evals, d: int, curve="pallas", want_coeffs: bool = False):
    """Trace::new's interpolate + commit (crates/plonk/src/circuit/trace.rs:165-192) for k evaluation
    vectors at once: Evals::from_vec_and_domain -> interpolate_by_ref -> pcdl::commit(poly, d, None).
    evals: (k, n, 4) ark scalars.  Returns the k commitments (k, 8) and, if asked, the trimmed
    coefficient vectors."""
    H.ensure_device()
    e = np.ascontiguousarray(np.asarray(evals, dtype=np.uint64))
    k, n = e.shape[0], e.shape[1]
    log_n = n.bit_length() - 1
    if 1 << log_n != n:
        raise ValueError("domain size must be a power of two")
    commits = np.zeros((k, 8), dtype=np.uint64)
    coeffs = np.zeros((k, n, 4), dtype=np.uint64) if want_coeffs else None
    lens = (ctypes.c_size_t * k)()
    H.check(H.load().halo_trace_commit_batch(_curve(curve), H.ptr(e), k, log_n, d,
                                             H.ptr(coeffs) if want_coeffs else None, lens, H.ptr(commits)))
    if want_coeffs:
        return commits, [coeffs[i, : lens[i]] for i in range(k)]
    return commits
