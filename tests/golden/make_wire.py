#!/usr/bin/env python3
"""Regenerate tests/golden/wire_qs_head.bin and wire_qs_head.npz (committed).  Run in the build container, where the
reference checkout is mounted read-only at /root/reference:

    python3 tests/golden/make_wire.py

The source is crates/accumulation/.precompute/qs.bin: ark-serialize compressed bytes of
Vec<(usize n, Instance, Instance, (Vec<Scalar>, Point, Scalar))> over Pallas, 19 entries, n = 2^2 .. 2^20.  The
whole file is parsed with the rules of tests/wire_ref.py (every byte must be consumed); the byte ranges of the two
Instances of each of the FIRST NINE entries (n = 4 .. 1024) are concatenated into wire_qs_head.bin: 18 instances,
nothing between them.  They are decode fixtures only: the transcript they were made with is not the current one.

wire_qs_head.npz (uint64 limbs, ark Montgomery, WrappedPoint rows; what wire_ref decodes):
  offsets, ends, d, hiding (18)      where each instance lies in wire_qs_head.bin, its degree bound and option tag
  C, U, C_bar (18, 8); z, v, c, w_prime (18, 4)
  Ls, Rs (sum lg, 8)                 instance i owns rows [rounds[i], rounds[i + 1])
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))
import pasta as P  # noqa: E402
import wire_ref as W  # noqa: E402

SRC = "/root/reference/crates/accumulation/.precompute/qs.bin"
ENTRIES = 9


def main():
    buf = open(SRC, "rb").read()
    cv = P.PALLAS
    count, off = int.from_bytes(buf[:8], "little"), 8
    ranges, insts = [], []
    for e in range(count):
        n, off = int.from_bytes(buf[off:off + 8], "little"), off + 8
        for _ in range(2):
            q, end = W.decode_instance(cv, buf, off)
            assert q["d"] == n - 1 and len(q["Ls"]) == len(q["Rs"]) == n.bit_length() - 1
            if e < ENTRIES:
                ranges.append((off, end))
                insts.append(q)
            off = end
        m, off = int.from_bytes(buf[off:off + 8], "little"), off + 8
        for _ in range(m):
            W.decode_scalar(buf[off:off + 32], cv.scalar)
            off += 32
        W.decode_point(cv, buf[off:off + 33])
        W.decode_scalar(buf[off + 33:off + 65], cv.scalar)
        off += 65
    assert off == len(buf) == 39965 and count == 19, (off, len(buf), count)

    head = b"".join(buf[a:b] for a, b in ranges)
    assert W.encode_instances(cv, insts) == head
    with open(os.path.join(HERE, "wire_qs_head.bin"), "wb") as f:
        f.write(head)

    sizes = [b - a for a, b in ranges]
    offsets = np.cumsum([0] + sizes[:-1]).astype(np.uint64)
    pt = lambda p: W.wrapped(cv, p)  # noqa: E731
    sc = lambda x: W.ark_scalar(x, cv.scalar)  # noqa: E731
    u64 = lambda rows: np.array(rows, dtype=np.uint64)  # noqa: E731
    np.savez_compressed(
        os.path.join(HERE, "wire_qs_head.npz"),
        offsets=offsets, ends=offsets + u64(sizes), d=u64([q["d"] for q in insts]),
        hiding=np.array([q["C_bar"] is not None for q in insts], dtype=np.uint8),
        rounds=np.cumsum([0] + [len(q["Ls"]) for q in insts]).astype(np.int64),
        C=u64([pt(q["C"]) for q in insts]), U=u64([pt(q["U"]) for q in insts]),
        C_bar=u64([pt(q["C_bar"]) for q in insts]), z=u64([sc(q["z"]) for q in insts]),
        v=u64([sc(q["v"]) for q in insts]), c=u64([sc(q["c"]) for q in insts]),
        w_prime=u64([sc(q["w_prime"] or 0) for q in insts]),
        Ls=u64([pt(p) for q in insts for p in q["Ls"]]), Rs=u64([pt(p) for q in insts for p in q["Rs"]]))
    print(f"{len(insts)} instances, {len(head)} bytes, {sum(len(q['Ls']) for q in insts) * 2 + 3 * len(insts)} points")


if __name__ == "__main__":
    main()
