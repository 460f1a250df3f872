"""The edge scalars of the fixed-base comb's tests (TEST INFRASTRUCTURE ONLY), shared by the plan's CPU test
(tests/test_fixed_base_plan.py) and the GPU tests (tests/test_gpu_schnorr_sign.py).

    * the powers of two hit every window boundary of any width, with leading and trailing zero windows;
    * the 0x80 patterns drive the carry of the signed recoding through every window;
    * 2^255 - r is the doubling case: under signed recoding with c = 8 or c = 4 its top digit is
      2^254 / 2^(c (W - 1)) and the lower windows sum to 2^254 - r = 2^254 (mod r), so an unfolded comb that adds the
      top window last adds a point to itself; its negative 2 r - 2^255 covers a folded variant.
"""
import pasta as P


def edge_scalars(cname: str) -> list:
    r = P.CURVES[cname].scalar
    e = [0, 1, 2, 3, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, 1 << 254, (1 << 254) - 1, (1 << 128) - 1, 1 << 128,
         (1 << 128) + 1, (1 << 255) - r, 2 * r - (1 << 255)]
    for byte in (b"\x80", b"\x7f", b"\xff", b"\x81"):
        e.append(int.from_bytes(byte * 32, "little") % r)
    e.append(int.from_bytes(b"\x01\x00" * 16, "big") % r)  # 0x0100...0100
    e += [1 << j for j in range(255)]
    e += [(1 << j) - 1 for j in range(0, 255, 4)]
    assert all(0 <= x < r for x in e)
    return e
