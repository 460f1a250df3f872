"""The wire format of the reference's proof objects (ark-serialize 0.5, compressed mode; include/halo_gpu.h, "the
wire format") on the MI355X backend: what ``serialize_compressed`` writes for a pcdl ``Instance``, an ``EvalProof``
inside it and an ``Accumulator`` (the same bytes as its instance), decoded and encoded on the device
(halo_amd/csrc/wire.hip: one square root per compressed point).

Points are (n, 8) WrappedPoint arrays and scalars (n, 4) ark Montgomery arrays, as everywhere in this package; the
serialized side is ``bytes``.  A record that does not decode comes back as the off-curve sentinel (0, 1) with
validity 0, never as an exception, so a batch keeps its shape; ``pcdl.check_bytes`` turns it into code 3.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as H
from .group import _curve

POINT_BYTES, SCALAR_BYTES = 33, 32


def _field(field) -> int:
    return H.FIELDS[field] if isinstance(field, str) else int(field)


def _u8(buf) -> np.ndarray:
    return np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, dtype=np.uint8)


def sqrt(xs, field="fq"):
    """halo_fe_sqrt_batch: (roots, is_square) of (n, 4) field elements; the smaller root as a canonical integer,
    zero and flag 0 for a non-residue."""
    H.ensure_device()
    x = H.fe_array(xs)
    out, sq = np.zeros_like(x), np.zeros(len(x), dtype=np.uint8)
    H.check(H.load().halo_fe_sqrt_batch(_field(field), H.ptr(x), len(x), H.ptr(out), H.ptr(sq)))
    return out, sq


def decompress_points(buf, curve="pallas"):
    """halo_points_decompress over len(buf) / 33 records: ((k, 8) points, k validity bytes)."""
    H.ensure_device()
    b = _u8(buf)
    if len(b) % POINT_BYTES:
        raise ValueError(f"{len(b)} bytes are not a whole number of 33-byte records")
    k = len(b) // POINT_BYTES
    out, ok = np.zeros((k, 8), dtype=np.uint64), np.zeros(k, dtype=np.uint8)
    H.check(H.load().halo_points_decompress(_curve(curve), H.ptr(b), k, H.ptr(out), H.ptr(ok)))
    return out, ok


def compress_points(pts, curve="pallas") -> bytes:
    """halo_points_compress: 33 bytes per point; HaloError for a point that is neither (0, 0) nor on the curve."""
    H.ensure_device()
    p = H.point_array(pts)
    out = np.zeros(len(p) * POINT_BYTES, dtype=np.uint8)
    H.check(H.load().halo_points_compress(_curve(curve), H.ptr(p), len(p), H.ptr(out)))
    return out.tobytes()


def scalars_from_bytes(buf, field="fp"):
    """halo_scalars_from_bytes: ((k, 4) ark scalars, k flags: the value was below the modulus)."""
    H.ensure_device()
    b = _u8(buf)
    if len(b) % SCALAR_BYTES:
        raise ValueError(f"{len(b)} bytes are not a whole number of 32-byte scalars")
    k = len(b) // SCALAR_BYTES
    out, ok = np.zeros((k, 4), dtype=np.uint64), np.zeros(k, dtype=np.uint8)
    H.check(H.load().halo_scalars_from_bytes(_field(field), H.ptr(b), k, H.ptr(out), H.ptr(ok)))
    return out, ok


def scalars_to_bytes(xs, field="fp") -> bytes:
    H.ensure_device()
    x = H.fe_array(xs)
    out = np.zeros(len(x) * SCALAR_BYTES, dtype=np.uint8)
    H.check(H.load().halo_scalars_to_bytes(_field(field), H.ptr(x), len(x), H.ptr(out)))
    return out.tobytes()


def walk(buf, vec: bool = False):
    """halo_pcdl_instances_walk (host only): (offsets (k + 1), ds (k), hiding (k)) of the instances of buf, offsets[i + 1]
    the end of instance i.  vec: the buffer is a Vec<Instance> with its u64 count first.  HaloError with the plan's
    message, naming the instance, for a buffer that is not a sequence of well-formed instances."""
    b = _u8(buf)
    max_k = len(b) // 188 + 1  # 188 bytes: the shortest instance (d = 0, not hiding)
    offsets, ds = np.zeros(max_k + 1, dtype=np.uint64), np.zeros(max_k, dtype=np.uint64)
    hiding, k = np.zeros(max_k, dtype=np.uint8), ctypes.c_size_t(0)
    H.check(H.load().halo_pcdl_instances_walk(H.ptr(b) if len(b) else None, len(b), int(vec), max_k, H.ptr(offsets),
                                              H.ptr(ds), H.ptr(hiding), ctypes.byref(k)))
    return offsets[: k.value + 1].copy(), ds[: k.value].copy(), hiding[: k.value].copy()


def _instance(d: int, rows, j: int, lg: int):
    from .pcdl import Instance
    C, z, v, Ls, Rs, U, c, hid, cb, wp = rows
    pi = {"Ls": [Ls[j * lg + r].copy() for r in range(lg)], "Rs": [Rs[j * lg + r].copy() for r in range(lg)],
          "U": U[j].copy(), "c": c[j].copy(), "C_bar": cb[j].copy() if hid[j] else None,
          "w_prime": wp[j].copy() if hid[j] else None}
    return Instance(C[j].copy(), d, z[j].copy(), v[j].copy(), pi)


def decode_instances(buf, vec: bool = False, curve="pallas"):
    """walk, then one halo_pcdl_instances_decode per distinct d: (list of pcdl.Instance in buffer order, ok mask).
    An instance with ok 0 holds sentinel points and zero scalars."""
    H.ensure_device()
    cid = _curve(curve)
    b = _u8(buf)
    offsets, ds, _ = walk(b, vec)
    k = len(ds)
    out, ok = [None] * k, np.zeros(k, dtype=np.uint8)
    for d in sorted({int(x) for x in ds}):
        idx = [i for i in range(k) if int(ds[i]) == d]
        lg, n = (d + 1).bit_length() - 1, len(idx)
        off = np.ascontiguousarray(offsets[idx])
        pt, fe = (lambda m: np.zeros((m, 8), dtype=np.uint64)), (lambda m: np.zeros((m, 4), dtype=np.uint64))
        rows = [pt(n), fe(n), fe(n), pt(n * lg), pt(n * lg), pt(n), fe(n), np.zeros(n, dtype=np.uint8), pt(n), fe(n)]
        ok_d = np.zeros(n, dtype=np.uint8)
        H.check(H.load().halo_pcdl_instances_decode(cid, d, n, H.ptr(b), len(b), H.ptr(off),
                                                    *[H.ptr(r) if len(r) else None for r in rows], H.ptr(ok_d)))
        for j, i in enumerate(idx):
            out[i], ok[i] = _instance(d, rows, j, lg), ok_d[j]
    return out, ok


def encode_instances(instances, vec: bool = False, curve="pallas") -> bytes:
    """halo_pcdl_instances_encode, one call per run of instances of one d (the order is kept); an Accumulator is the
    bytes of its instance.  vec: prepend the u64 count, as a Vec<Instance> serializes."""
    from .pcdl import Instance, instance_rows
    H.ensure_device()
    cid = _curve(curve)
    insts = [Instance(*q) for q in instances]
    out = [len(insts).to_bytes(8, "little")] if vec else []
    i = 0
    while i < len(insts):
        j = i
        while j < len(insts) and insts[j].d == insts[i].d:
            j += 1
        d, qs = insts[i].d, insts[i:j]
        rows = instance_rows(qs, d)
        n = ctypes.c_size_t(0)
        args = [cid, d, len(qs), *[H.ptr(r) for r in rows]]
        H.check(H.load().halo_pcdl_instances_encode(*args, None, ctypes.byref(n)))
        buf = np.zeros(n.value, dtype=np.uint8)
        H.check(H.load().halo_pcdl_instances_encode(*args, H.ptr(buf), ctypes.byref(n)))
        out.append(buf.tobytes())
        i = j
    return b"".join(out)


def check_codes(buf, rhos=None, vec: bool = False, curve="pallas", bisect: bool = False) -> np.ndarray:
    """pcdl.check_bytes's codes: walk on the host, then per distinct d halo_pcdl_instances_decode_dev and
    halo_pcdl_check_fs_batch_dev on one stream, the decoded arrays never leaving the device."""
    import torch
    from . import pcdl
    H.ensure_device()
    cid = _curve(curve)
    b = _u8(buf)
    offsets, ds, _ = walk(b, vec)  # raises before any launch
    k = len(ds)
    rh, derive = H.fs_rhos(rhos, k)  # "fs": each d derives its own weights on the device
    codes = np.zeros(k, dtype=np.uint8)
    if k == 0:
        return codes
    L = H.load()
    dev = lambda a: torch.from_numpy(np.array(a, order="C").view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()  # noqa: E731
    d_bytes = dev(b)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for d in sorted({int(x) for x in ds}):
        idx = [i for i in range(k) if int(ds[i]) == d]
        lg, n = (d + 1).bit_length() - 1, len(idx)
        d_off = dev(np.ascontiguousarray(offsets[idx]))
        words = lambda m, w: torch.zeros((max(m, 1), w), dtype=torch.int64, device="cuda")  # noqa: E731
        flags = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")  # noqa: E731
        arrays = [words(n, 8), words(n, 4), words(n, 4), words(n * lg, 8), words(n * lg, 8), words(n, 8), words(n, 4), flags(),
                  words(n, 8), words(n, 4)]
        d_ok, d_code, d_comb = flags(), flags(), flags()
        ptrs = [t.data_ptr() for t in arrays]
        H.check(L.halo_pcdl_instances_decode_dev(cid, d, n, d_bytes.data_ptr(), len(b), d_off.data_ptr(), *ptrs,
                                                 d_ok.data_ptr(), stream))
        d_rho = dev(rh[idx]) if rh is not None else None
        with H.deriving(derive):
            H.check(L.halo_pcdl_check_fs_batch_dev(cid, d, n, *ptrs, d_rho.data_ptr() if rh is not None else None,
                                                   d_code.data_ptr(), d_comb.data_ptr(), stream))
        torch.cuda.current_stream().synchronize()
        if (rh is not None or derive) and n > 1 and not int(d_comb[0]):
            # the combination was rejected: per-instance verdicts by bisection (the host form's route) or exactly
            if bisect:
                host = [t.cpu().numpy().view(np.uint64 if t.dtype == torch.int64 else np.uint8) for t in arrays]
                C, z, v, Ls, Rs, U, c, hid, cb, wp = host
                got = pcdl.check_fs_codes(C, d, z, v, Ls if lg else None, Rs if lg else None, U, c, hiding=hid, C_bars=cb,
                                          w_primes=wp, rhos="fs" if derive else rh[idx], curve=cid, bisect=True)
            else:
                H.check(L.halo_pcdl_check_fs_batch_dev(cid, d, n, *ptrs, None, d_code.data_ptr(), d_comb.data_ptr(), stream))
                torch.cuda.current_stream().synchronize()
                got = d_code.cpu().numpy()
        else:
            got = d_code.cpu().numpy()
        codes[idx] = np.where(d_ok.cpu().numpy() == 0, 3, got)
    return codes
