"""CPU tests of the argument refusals of the evals entry points of libhalo_gpu.so (include/halo_gpu.h, "f1:
evaluation algebra"): each returns HALO_EINVAL with its message before any device lookup, so none needs a GPU, and
leaves the caller's output alone.  The `len < n` path of halo_divide_by_vanishing is host code throughout and is
checked for its results.  The kernels behind these calls are in tests/test_gpu_evals.py."""
import ctypes

import numpy as np
import pytest

from halo_amd import _lib as H

EINVAL = 1
SENTINEL = np.uint64(0x5A5AA5A5C3C33C3C)


@pytest.fixture(scope="module")
def L():
    return H.load()


def buf(rows=4):
    return np.full((rows, 4), SENTINEL, dtype=np.uint64)


def untouched(*arrays):
    return all((a == SENTINEL).all() for a in arrays)


def refused(rc, needle):
    return rc == EINVAL and needle in H.last_error()


def gate_arrays():
    x = buf()
    vp = ctypes.c_void_p
    return (vp * 16)(*[x.ctypes.data] * 16), (vp * 15)(*[x.ctypes.data] * 15), (vp * 10)(*[x.ctypes.data] * 10), x


def test_unknown_field_on_every_entry_point(L):
    x, out, out2 = buf(), buf(), buf()
    p, o, o2 = H.ptr(x), H.ptr(out), H.ptr(out2)
    ql, rl = ctypes.c_size_t(77), ctypes.c_size_t(77)
    dw, dr, dq, _ = gate_arrays()
    lens = (ctypes.c_size_t * 1)(4)
    ptrs = (ctypes.c_void_p * 1)(x.ctypes.data)
    for field in (2, -1):
        assert refused(L.halo_evals_op(field, 0, p, p, p, 0, o, 4), "unknown field id")
        assert refused(L.halo_evals_op_dev(field, 0, p, p, p, 0, o, 4, None), "unknown field id")
        assert refused(L.halo_divide_by_vanishing(field, p, 4, 2, o, ctypes.byref(ql), o2, ctypes.byref(rl)),
                       "unknown field id")
        assert refused(L.halo_divide_by_vanishing_dev(field, p, 4, 2, o, o2, None), "unknown field id")
        assert refused(L.halo_gate_constraints_dev(field, dw, dr, dq, p, p, 4, 1, o, None), "unknown field id")
        assert refused(L.halo_evals_scan_dev(field, 0, p, o, 4, None), "unknown field id")
        assert refused(L.halo_poly_lincomb_dev(field, ptrs, lens, 1, p, o, 4, None), "unknown field id")
    assert untouched(out, out2) and ql.value == 77 and rl.value == 77


@pytest.mark.parametrize("dev", [False, True])
def test_evals_op_refusals(L, dev):
    x, out = buf(), buf()
    p, o = H.ptr(x), H.ptr(out)

    def call(op, a, b, s, e, o_, n):
        if dev:
            return L.halo_evals_op_dev(0, op, a, b, s, e, o_, n, None)
        return L.halo_evals_op(0, op, a, b, s, e, o_, n)

    for op in (-1, 7):
        assert refused(call(op, p, p, p, 0, o, 4), f"unknown evals op {op}")
    for op in range(7):
        assert refused(call(op, None, p, p, 0, o, 4), "null buffer")
        assert refused(call(op, p, p, p, 0, None, 4), "null buffer")
    for op in (0, 1, 2):
        assert refused(call(op, p, None, p, 0, o, 4), f"op {op} needs a second operand")
    for op in (3, 4, 5):
        assert refused(call(op, p, p, None, 0, o, 4), "null scalar")
    # n = 0 is a success with null buffers
    for op in (0, 1, 2, 6):
        assert call(op, None, None, None, 0, None, 0) == 0
    for op in (3, 4, 5):
        assert call(op, None, None, p, 0, None, 0) == 0
    assert untouched(out)


def test_divide_by_vanishing_host_refusals_and_short_input(L):
    q, r = buf(8), buf(8)
    ql, rl = ctypes.c_size_t(77), ctypes.c_size_t(77)
    c = np.arange(1, 21, dtype=np.uint64).reshape(5, 4).copy()
    a = (H.ptr(c), 5)
    msg = "halo_divide_by_vanishing: null argument"
    assert refused(L.halo_divide_by_vanishing(0, *a, 0, H.ptr(q), ctypes.byref(ql), H.ptr(r), ctypes.byref(rl)), msg)
    assert refused(L.halo_divide_by_vanishing(0, None, 5, 8, H.ptr(q), ctypes.byref(ql), H.ptr(r), ctypes.byref(rl)), msg)
    assert refused(L.halo_divide_by_vanishing(0, *a, 8, None, ctypes.byref(ql), H.ptr(r), ctypes.byref(rl)), msg)
    assert refused(L.halo_divide_by_vanishing(0, *a, 8, H.ptr(q), None, H.ptr(r), ctypes.byref(rl)), msg)
    assert refused(L.halo_divide_by_vanishing(0, *a, 8, H.ptr(q), ctypes.byref(ql), None, ctypes.byref(rl)), msg)
    assert refused(L.halo_divide_by_vanishing(0, *a, 8, H.ptr(q), ctypes.byref(ql), H.ptr(r), None), msg)
    assert untouched(q, r) and ql.value == 77 and rl.value == 77
    # len < n: quotient zero, remainder the input itself
    assert L.halo_divide_by_vanishing(0, *a, 8, H.ptr(q), ctypes.byref(ql), H.ptr(r), ctypes.byref(rl)) == 0
    assert ql.value == 0 and rl.value == 5 and np.array_equal(r[:5], c) and untouched(q, r[5:])
    # trailing zero coefficients are trimmed before the comparison with n: 8 coefficients of which 3 count, n = 4
    c8 = np.zeros((8, 4), dtype=np.uint64)
    c8[:3] = c[:3]
    r = buf(8)
    assert L.halo_divide_by_vanishing(1, H.ptr(c8), 8, 4, H.ptr(q), ctypes.byref(ql), H.ptr(r), ctypes.byref(rl)) == 0
    assert ql.value == 0 and rl.value == 3 and np.array_equal(r[:3], c[:3]) and untouched(q, r[3:])
    # the zero polynomial, also as a null pointer of length 0
    r = buf(8)
    z4 = np.zeros((4, 4), dtype=np.uint64)
    for cp, ln in ((H.ptr(z4), 4), (None, 0)):
        ql.value = rl.value = 77
        assert L.halo_divide_by_vanishing(0, cp, ln, 1, H.ptr(q), ctypes.byref(ql), H.ptr(r), ctypes.byref(rl)) == 0
        assert ql.value == 0 and rl.value == 0 and untouched(q, r)


def test_divide_by_vanishing_dev_refusals(L):
    x, q, r = buf(8), buf(8), buf(8)
    p = H.ptr(x)
    msg = "halo_divide_by_vanishing_dev: bad argument"
    assert refused(L.halo_divide_by_vanishing_dev(0, p, 8, 0, H.ptr(q), H.ptr(r), None), msg)
    assert refused(L.halo_divide_by_vanishing_dev(0, p, 3, 4, H.ptr(q), H.ptr(r), None), msg + " (len 3, n 4)")
    assert refused(L.halo_divide_by_vanishing_dev(0, None, 8, 4, H.ptr(q), H.ptr(r), None), msg)
    assert refused(L.halo_divide_by_vanishing_dev(0, p, 8, 4, H.ptr(q), None, None), msg)
    assert refused(L.halo_divide_by_vanishing_dev(0, p, 8, 4, None, H.ptr(r), None), msg)
    assert untouched(q, r)


def test_gate_constraints_refusals(L):
    dw, dr, dq, x = gate_arrays()
    out = buf()
    p, o = H.ptr(x), H.ptr(out)
    msg = "halo_gate_constraints_dev: bad argument"
    for n in (0, 3, 12):
        assert refused(L.halo_gate_constraints_dev(0, dw, dr, dq, p, p, n, 1, o, None), msg)
    good = [dw, dr, dq, p, p]
    for k in range(5):
        args = good[:k] + [None] + good[k + 1:]
        assert refused(L.halo_gate_constraints_dev(1, *args, 4, 1, o, None), msg)
    assert refused(L.halo_gate_constraints_dev(1, *good, 4, 1, None, None), msg)
    assert untouched(out)


def test_scan_refusals(L):
    x, out = buf(), buf()
    p, o = H.ptr(x), H.ptr(out)
    for rev in (0, 1):
        assert refused(L.halo_evals_scan_dev(0, rev, None, o, 4, None), "halo_evals_scan_dev: null buffer")
        assert refused(L.halo_evals_scan_dev(0, rev, p, None, 4, None), "halo_evals_scan_dev: null buffer")
        assert L.halo_evals_scan_dev(0, rev, None, None, 0, None) == 0
        # 256 * 4096 blocks of 2048 elements is the most that one block can scan the totals of; refused before any launch
        for n in (256 * 4096 * 2048 + 1, 2**64 - 1):
            assert refused(L.halo_evals_scan_dev(1, rev, p, o, n, None), "halo_evals_scan_dev: n too large")
    assert untouched(out)


def test_lincomb_refusals(L):
    x, out = buf(), buf()
    p, o = H.ptr(x), H.ptr(out)
    vp = ctypes.c_void_p
    ptrs65 = (vp * 65)(*[x.ctypes.data] * 65)
    lens65 = (ctypes.c_size_t * 65)(*[4] * 65)
    assert refused(L.halo_poly_lincomb_dev(0, ptrs65, lens65, 65, p, o, 4, None), "halo_poly_lincomb_dev: k = 65 > 64")
    assert refused(L.halo_poly_lincomb_dev(0, ptrs65, lens65, 2, None, o, 4, None), "halo_poly_lincomb_dev: null argument")
    assert refused(L.halo_poly_lincomb_dev(0, ptrs65, lens65, 2, p, None, 4, None), "halo_poly_lincomb_dev: null argument")
    assert refused(L.halo_poly_lincomb_dev(0, None, lens65, 2, p, o, 4, None), "halo_poly_lincomb_dev: null argument")
    assert refused(L.halo_poly_lincomb_dev(0, ptrs65, None, 2, p, o, 4, None), "halo_poly_lincomb_dev: null argument")
    lens = (ctypes.c_size_t * 3)(4, 4, 2**32)
    assert refused(L.halo_poly_lincomb_dev(0, ptrs65, lens, 3, p, o, 4, None), "halo_poly_lincomb_dev: bad polynomial 2")
    ptrs = (vp * 3)(x.ctypes.data, None, x.ctypes.data)
    lens = (ctypes.c_size_t * 3)(4, 1, 4)
    assert refused(L.halo_poly_lincomb_dev(1, ptrs, lens, 3, p, o, 4, None), "halo_poly_lincomb_dev: bad polynomial 1")
    # n_out = 0 writes nothing and succeeds, with or without inputs
    assert L.halo_poly_lincomb_dev(0, ptrs65, lens65, 64, p, None, 0, None) == 0
    assert L.halo_poly_lincomb_dev(1, None, None, 0, p, None, 0, None) == 0
    assert untouched(out)
