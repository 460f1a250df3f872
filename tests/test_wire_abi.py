"""CPU tests of the wire-format entry points of libhalo_gpu.so (include/halo_gpu.h, "the wire format"): the ABI
version, argument checks that need no device, and halo_pcdl_instances_walk, which is host code throughout, against
the reference's bytes (tests/golden/wire_qs_head.bin) and the layout tests/wire_ref.py decodes from them."""
import ctypes
import os

import numpy as np
import pytest

from halo_amd import _lib as H
from halo_amd import wire

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def L():
    return H.load()


@pytest.fixture(scope="module")
def head():
    return open(os.path.join(GOLDEN, "wire_qs_head.bin"), "rb").read()


def test_abi_version_110(L):
    assert L.halo_abi_version() >= 110


def test_walk_of_the_fixture(L, head):
    exp = np.load(os.path.join(GOLDEN, "wire_qs_head.npz"))
    for vec in (False, True):
        buf = (len(exp["d"]).to_bytes(8, "little") if vec else b"") + head
        offsets, ds, hiding = wire.walk(buf, vec=vec)
        shift = 8 if vec else 0
        assert (offsets[:-1] - shift).tolist() == exp["offsets"].tolist()
        assert (offsets[1:] - shift).tolist() == exp["ends"].tolist() and offsets[-1] == len(buf)
        assert ds.tolist() == exp["d"].tolist() and hiding.tolist() == exp["hiding"].tolist()
    offsets, ds, hiding = wire.walk(b"")
    assert offsets.tolist() == [0] and len(ds) == 0 and len(hiding) == 0


@pytest.mark.parametrize("damage,code,message", [
    (lambda b: b[:700], 1, r"instance 1: the buffer ends inside an instance"),
    (lambda b: b[:105] + (2**64 - 1).to_bytes(8, "little") + b[113:], 1, r"instance 0: a length prefix exceeds"),
    (lambda b: b[:385 + 179] + (3).to_bytes(8, "little") + b[385 + 187:], 1, r"instance 1: Ls and Rs must both hold"),
    (lambda b: b[:33] + (4).to_bytes(8, "little") + b[41:], 4, r"instance 0: d \+ 1 is not a power of two"),
    (lambda b: b[:318] + b"\2" + b[319:], 1, r"instance 0: an option tag is neither 0 nor 1"),
    (lambda b: b[:352] + b"\0" + b[353:], 1, r"instance 0: C_bar and w_prime must be present together"),
])
def test_walk_refusals_carry_the_plan_message(L, head, damage, code, message):
    with pytest.raises(H.HaloError, match=message) as e:
        wire.walk(damage(head))
    assert e.value.code == code


def test_walk_capacity_and_nulls(L, head):
    k = ctypes.c_size_t(9)
    off, ds, hid = np.zeros(3, dtype=np.uint64), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint8)
    b = np.frombuffer(head, dtype=np.uint8)
    assert L.halo_pcdl_instances_walk(H.ptr(b), len(b), 0, 2, H.ptr(off), H.ptr(ds), H.ptr(hid), ctypes.byref(k)) == 1
    assert "more instances than max_k" in H.last_error() and k.value == 0 and not off.any()
    assert L.halo_pcdl_instances_walk(H.ptr(b), 770, 0, 2, H.ptr(off), H.ptr(ds), H.ptr(hid), ctypes.byref(k)) == 0
    assert k.value == 2 and off.tolist() == [0, 385, 770]
    assert L.halo_pcdl_instances_walk(H.ptr(b), len(b), 0, 2, None, H.ptr(ds), H.ptr(hid), ctypes.byref(k)) == 1
    assert L.halo_pcdl_instances_walk(H.ptr(b), len(b), 0, 2, H.ptr(off), H.ptr(ds), H.ptr(hid), None) == 1


def test_argument_checks_before_any_device_work(L):
    x = np.zeros((2, 8), dtype=np.uint64)
    p = H.ptr(x)
    n = ctypes.c_size_t(0)
    assert L.halo_fe_sqrt_batch(7, p, 2, p, None) == 1 and "unknown field" in H.last_error()
    assert L.halo_fe_sqrt_batch(0, None, 2, p, None) == 1
    assert L.halo_fe_sqrt_batch_dev(0, p, 2, None, None, None) == 1
    assert L.halo_points_decompress(5, p, 2, p, None) == 1 and "unknown curve" in H.last_error()
    assert L.halo_points_decompress(0, None, 2, p, None) == 1
    assert L.halo_points_compress_dev(0, None, 2, p, None, None) == 1
    assert L.halo_scalars_from_bytes(0, p, 2, None, None) == 1
    assert L.halo_scalars_to_bytes_dev(0, p, 2, None, None) == 1
    for name, extra in (("halo_pcdl_instances_decode", ()), ("halo_pcdl_instances_decode_dev", (None,))):
        fn = getattr(L, name)
        assert fn(0, 4, 1, p, 64, p, *[p] * 11, *extra) == 4 and "n (5) is not a power of two" in H.last_error()
        assert fn(0, 3, 1, None, 64, p, *[p] * 11, *extra) == 1
        assert fn(0, 3, 1, p, 64, p, *[p] * 10, None, *extra) == 1
        assert fn(0, 3, 0, None, 0, None, *[None] * 11, *extra) == 0
    # the host form walks every instance before it touches the device: 64 zero bytes end inside an instance
    off = np.zeros(1, dtype=np.uint64)
    assert L.halo_pcdl_instances_decode(0, 3, 1, p, 64, H.ptr(off), *[p] * 11) == 1
    assert "the buffer ends inside an instance" in H.last_error()
    # the size query of encode needs neither arrays nor a device: two plain and one hiding instance at d = 7
    hid = np.array([0, 1, 0], dtype=np.uint8)
    assert L.halo_pcdl_instances_encode(0, 7, 3, *[None] * 7, H.ptr(hid), None, None, None, ctypes.byref(n)) == 0
    assert n.value == 3 * 386 + 65  # 386 bytes plain at lg = 3; C_bar and w_prime add 65
    assert L.halo_pcdl_instances_encode(0, 6, 3, *[None] * 7, H.ptr(hid), None, None, None, ctypes.byref(n)) == 4
    n.value = 10
    assert L.halo_pcdl_instances_encode(0, 7, 3, *[p] * 7, H.ptr(hid), p, p, p, ctypes.byref(n)) == 1
    assert "bytes needed" in H.last_error() and n.value == 3 * 386 + 65
