// Pieces of the quad-cooperative variable-base ladder shared by the Schnorr verification
// (schnorr.hip, k_schnorr_verify) and the batched linear combinations of points (lincomb.hip,
// k_lincomb_terms): the on-curve test of an input point, the signed 4-bit recoding of a GLV half-scalar
// and the broadcast of a quad addition's sum, in the arithmetic namespace of the including unit.
#pragma once
#include "curve.hpp"
#include "tree.hpp"

HALO_ARITH_BEGIN

// The point of the quad's lane 2 (where xyzz_add_quad assembles its sum) in every lane of the quad, by
// DPP quad broadcasts: no trip through the LDS crossbar.
template <class F>
HALO_DEV XYZZ<F> xyzz_quad_lane2(const XYZZ<F>& p) {
    constexpr int B2 = qp(2, 2, 2, 2);
    XYZZ<F> r;
    r.X = qperm<B2>(p.X);
    r.Y = qperm<B2>(p.Y);
    r.ZZ = qperm<B2>(p.ZZ);
    r.ZZZ = qperm<B2>(p.ZZZ);
    return r;
}

template <class F>
HALO_DEV bool aff_on_curve_or_id(const Affine<F>& a, const Fe<F>& b) {
    if (aff_is_id(a)) return true;
    return fe_eq(fe_sqr(a.y), fe_add(fe_mul(fe_sqr(a.x), a.x), b));
}

// A magnitude k < 2^130 (5 words) as 33 signed 4-bit digits, k = sum d_w 16^w with d_w in [-8, 7]: from
// the bottom, a window value u = nibble + carry >= 8 becomes u - 16 and carries 1 (the top window is at
// most 3 + 1, so nothing is carried out).  The digits are two's complement nibbles, digit 32 in the top
// nibble of r[4] and the lower ones below it: the ladder reads the top nibble and shifts left by 4.
struct SignedDigits {
    uint32_t r[5];
    HALO_DEV void recode(const uint32_t (&k)[5]) {
        uint32_t t[5] = {0, 0, 0, 0, 0};
        uint32_t carry = 0;
#pragma unroll
        for (int w = 0; w < 33; w++) {
            const int q = (4 * w) >> 5, sh = (4 * w) & 31;
            const uint32_t u = ((k[q] >> sh) & 15u) + carry;  // 0..16
            carry = u >> 3 ? 1u : 0u;
            t[q] |= (u & 15u) << sh;
        }
#pragma unroll
        for (int i = 4; i >= 1; i--) r[i] = (t[i] << 28) | (t[i - 1] >> 4);
        r[0] = t[0] << 28;
    }
    // the next digit from the top: its magnitude (0..8) and sign
    HALO_DEV uint32_t next(bool& neg) {
        const uint32_t n = r[4] >> 28;
        neg = n >= 8u;
#pragma unroll
        for (int i = 4; i >= 1; i--) r[i] = (r[i] << 4) | (r[i - 1] >> 28);
        r[0] <<= 4;
        return neg ? 16u - n : n;
    }
};

HALO_ARITH_END
