"""Mirror of crates/poseidon/src/outer_sponge.rs (``Sponge<P>``: new, absorb_g, absorb_g_affine, absorb_fq,
absorb_fr, challenge, reset) on the MI355X backend: the Fiat-Shamir sponge as an object whose state lives in device
memory between calls (halo_sponge_*, halo_amd/csrc/sponge.hip).

``Sponge(curve, label)`` is one sponge over WrappedPoints / ark scalars -- the ``transcript`` that halo_amd.pcdl
(open, check, succinct_check) takes, and through ``new_transcript(curve)`` the factory that halo_amd.acc and
halo_amd.prover.naive_prover take.  ``SpongeBatch(curve, label, k)`` is k sponges that advance in lockstep: every
call applies one operation to all of them, on k rows of data.

The Poseidon constants are the caller's: install them once per field with halo_amd.schnorr.set_poseidon_params.
"""
from __future__ import annotations

import ctypes
import weakref

import numpy as np

from . import _lib as H
from .group import _curve

LABELS = {"PCDL": 0, "ASDL": 1, "PLONK": 2, "SIGNATURE": 3}  # outer_sponge.rs:17-22, Protocols


def _free(handle: int) -> None:
    try:
        H.load().halo_sponge_free(ctypes.c_uint64(handle))
    except Exception:  # the interpreter is going down
        pass


class SpongeBatch:
    """k sponges of one protocol in lockstep.  Arrays are (k, n, 8) WrappedPoints or (k, n, 4) field elements (ark
    Montgomery words); row i belongs to sponge i.  The ``_dev`` methods take torch tensors of the same shapes (int64
    words) on the current device and only enqueue on the current torch stream."""

    def __init__(self, curve, label: str, k: int):
        if label not in LABELS:
            raise ValueError(f"label {label!r} is none of {sorted(LABELS)}")
        H.ensure_device()
        self.curve, self.label, self.k = _curve(curve), label, int(k)
        self._L = H.load()
        hid = ctypes.c_uint64(0)
        H.check(self._L.halo_sponge_new(self.curve, LABELS[label], self.k, ctypes.byref(hid)))
        self._id = hid.value
        self._fin = weakref.finalize(self, _free, self._id)
        self._fin.atexit = False  # at exit the process's device memory goes with it

    # -- host arrays
    def _rows(self, a, words: int) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(a, dtype=np.uint64))
        return a.reshape(self.k, -1, words) if a.size else a.reshape(self.k, 0, words)

    def _absorb(self, fn, a, words: int) -> None:
        a = self._rows(a, words)
        if a.shape[1]:
            H.check(fn(self._id, H.ptr(a), a.shape[1]))

    def absorb_g(self, points) -> None:
        self._absorb(self._L.halo_sponge_absorb_g, points, 8)

    absorb_g_affine = absorb_g  # the WrappedPoint is the affine form (outer_sponge.rs:51-61)

    def absorb_fr(self, xs) -> None:
        self._absorb(self._L.halo_sponge_absorb_fr, xs, 4)

    def absorb_fq(self, xs) -> None:
        self._absorb(self._L.halo_sponge_absorb_fq, xs, 4)

    def challenge(self, n: int = 1) -> np.ndarray:
        """The next n challenges of every sponge: (k, n, 4) ark scalars."""
        out = np.zeros((self.k, n, 4), dtype=np.uint64)
        if n:
            H.check(self._L.halo_sponge_challenge(self._id, n, H.ptr(out)))
        return out

    # -- device tensors, the current stream
    @staticmethod
    def _stream():
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _absorb_dev(self, fn, t, words: int) -> None:
        assert t.is_cuda and t.is_contiguous() and t.element_size() == 8 and t.numel() % (self.k * words) == 0
        n = t.numel() // (self.k * words)
        if n:
            H.check(fn(self._id, ctypes.c_void_p(t.data_ptr()), n, self._stream()))

    def absorb_g_dev(self, points) -> None:
        self._absorb_dev(self._L.halo_sponge_absorb_g_dev, points, 8)

    def absorb_fr_dev(self, xs) -> None:
        self._absorb_dev(self._L.halo_sponge_absorb_fr_dev, xs, 4)

    def absorb_fq_dev(self, xs) -> None:
        self._absorb_dev(self._L.halo_sponge_absorb_fq_dev, xs, 4)

    def challenge_dev(self, n: int = 1):
        """(k, n, 4) int64 tensor of ark words, written on the current stream."""
        import torch
        out = torch.empty((self.k, n, 4), dtype=torch.int64, device="cuda")
        if n:
            H.check(self._L.halo_sponge_challenge_dev(self._id, n, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def reset(self) -> None:
        """Sponge::reset (outer_sponge.rs:97-99): the zero state with nothing absorbed -- no label either."""
        H.check(self._L.halo_sponge_reset(self._id))

    def close(self) -> None:
        """Free the device state now (garbage collection does the same)."""
        if self._fin.detach():
            H.check(self._L.halo_sponge_free(self._id))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class Sponge(SpongeBatch):
    """``Sponge::<P>::new(label)``: one sponge.  absorb_g(points) / absorb_fr(xs) / absorb_fq(xs) take a sequence of
    WrappedPoints (8 words each) or field elements (4 words each); challenge() returns (4,) uint64."""

    def __init__(self, curve, label: str):
        super().__init__(curve, label, 1)

    def challenge(self) -> np.ndarray:  # noqa: D102
        return super().challenge(1).reshape(4)

    def challenge_dev(self):  # noqa: D102
        return super().challenge_dev(1).reshape(4)


def new_transcript(curve):
    """The ``new_transcript(label)`` factory of halo_amd.acc and halo_amd.prover.naive_prover, on the device."""
    return lambda label: Sponge(curve, label)
