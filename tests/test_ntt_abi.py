"""CPU tests of the argument refusals of the device NTT entry points of libhalo_gpu.so (include/halo_gpu.h,
halo_ntt_dev and halo_ntt_dev_zero_tail): each returns HALO_EINVAL with its message before any shift by log_n, any
buffer is sized and any device lookup, so none needs a GPU, and leaves the caller's buffer alone.  An empty batch
is a success that launches nothing.  The transforms themselves are in tests/test_gpu_ntt.py, the rule behind the
refusals (ntt_check) in tests/test_ntt_plan.py."""
import numpy as np
import pytest

from halo_amd import _lib as H

EINVAL = 1
SENTINEL = np.uint64(0x5A5AA5A5C3C33C3C)


@pytest.fixture(scope="module")
def L():
    return H.load()


def buf(rows=8):
    return np.full((rows, 4), SENTINEL, dtype=np.uint64)


def refused(rc, needle):
    return rc == EINVAL and needle in H.last_error()


def test_unknown_field(L):
    x = buf()
    for field in (2, -1):
        assert refused(L.halo_ntt_dev(field, H.ptr(x), 3, 1, 0, None), "unknown field id")
        assert refused(L.halo_ntt_dev_zero_tail(field, H.ptr(x), 3, 1, 4, None), "unknown field id")
    assert (x == SENTINEL).all()


def test_null_buffer(L):
    assert refused(L.halo_ntt_dev(0, None, 3, 1, 0, None), "halo_ntt_dev: null buffer")
    assert refused(L.halo_ntt_dev_zero_tail(0, None, 3, 1, 4, None), "halo_ntt_dev_zero_tail: null buffer")


@pytest.mark.parametrize("log_n", [31, 64, 2**32 - 1])
def test_domain_too_large(L, log_n):
    x = buf()
    for field in (0, 1):
        for inverse in (0, 1):
            assert refused(L.halo_ntt_dev(field, H.ptr(x), log_n, 1, inverse, None), "NTT domain 2^%d too large" % log_n)
        # whatever nonzero_len says: it is compared with N only once log_n has passed
        for nz in (0, 4, 2**64 - 1):
            assert refused(L.halo_ntt_dev_zero_tail(field, H.ptr(x), log_n, 1, nz, None),
                           "NTT domain 2^%d too large" % log_n)
        # ... and before the batch is looked at
        assert refused(L.halo_ntt_dev(field, H.ptr(x), log_n, 0, 0, None), "NTT domain 2^%d too large" % log_n)
        assert refused(L.halo_ntt_dev(field, H.ptr(x), log_n, 65536, 0, None), "NTT domain 2^%d too large" % log_n)
    assert (x == SENTINEL).all()


def test_batch_too_large(L):
    x = buf()
    for batch in (65536, 2**64 - 1):
        for log_n in (0, 3, 30):
            assert refused(L.halo_ntt_dev(0, H.ptr(x), log_n, batch, 0, None), "65535")
            assert "batch" in H.last_error()
            assert refused(L.halo_ntt_dev_zero_tail(1, H.ptr(x), log_n, batch, 1, None), "65535")
            assert "batch" in H.last_error()
    assert (x == SENTINEL).all()


def test_nonzero_len_above_n(L):
    x = buf(16)
    for log_n, nz in ((3, 9), (0, 2), (3, 2**64 - 1)):
        assert refused(L.halo_ntt_dev_zero_tail(0, H.ptr(x), log_n, 1, nz, None), "halo_ntt_dev_zero_tail: nonzero_len > N")
        # also for an empty batch: the arguments are checked first
        assert refused(L.halo_ntt_dev_zero_tail(0, H.ptr(x), log_n, 0, nz, None), "halo_ntt_dev_zero_tail: nonzero_len > N")
    assert (x == SENTINEL).all()


def test_empty_batch_is_a_success_without_a_device(L):
    x = buf()
    for log_n in (0, 3, 30):
        for inverse in (0, 1):
            assert L.halo_ntt_dev(0, H.ptr(x), log_n, 0, inverse, None) == 0
        assert L.halo_ntt_dev_zero_tail(1, H.ptr(x), log_n, 0, 1, None) == 0
    assert (x == SENTINEL).all()
