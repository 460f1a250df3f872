// Square roots in the Pasta fields on the device (each field is the base field of one curve: a compressed point
// is an x and a sign, wire.hip).
//
// Both fields have 2-adicity 32: p - 1 = 2^32 t, t odd, and 5 is a non-residue, so g = 5^t generates the subgroup
// of order 2^32.  Tonelli-Shanks with the subgroup logarithm taken bit by bit (Pohlig-Hellman):
//   w = a^((t - 1) / 2)          fixed 2-bit-window chain over the constant exponent (SQRT_EXP64)
//   x = a w  = a^((t + 1) / 2),  b = x w = a^t, which lies in <g>;  x^2 = a b
//   for i = 0 .. 31:             b holds g^e with the low i bits of e cleared;  b^(2^(31 - i)) = (-1)^(bit i of e)
//       bit set:                 b *= g^(-2^i), and for i >= 1  x *= g^(-2^(i - 1))
//   then x^2 = a g^(e mod 2): a root iff e is even, i.e. iff a is a square.
// The closing test x^2 == a is the non-residue test (it also covers a = 0: w = x = 0).  Every trip count is a
// constant and every data-dependent step is a select, so the lanes of a wave, which hold different inputs, never
// diverge.  Cost per root: ~222 + 496 squarings and ~56 + 64 multiplications.  The table g^(-2^i) is
// OMEGA_INV[32 - i] of consts.hpp (the NTT's inverse roots of unity: 5^(-(p - 1) / 2^(32 - i))).
#pragma once
#include "fields.hpp"

HALO_ARITH_BEGIN

// A root of a (internal Montgomery form, either sign) and whether a is a square; 0 and false for a non-residue.
template <class C>
HALO_DEV Fe<C> fe_sqrt(const Fe<C>& a, bool& is_square) {
    static_assert(MAX_LOG_DOMAIN == 32, "fe_sqrt walks the 32 bits of the subgroup logarithm");
    const Fe<C> a2 = fe_sqr(a);
    const Fe<C> a3 = fe_mul(a2, a);
    Fe<C> w = fe_one<C>();
#pragma unroll 1
    for (int i = C::SQRT_EXP_WINDOWS - 1; i >= 0; i--) {
        w = fe_sqr(fe_sqr(w));
        const uint32_t d = (uint32_t)(C::SQRT_EXP64[i >> 5] >> ((i & 31) * 2)) & 3u;  // the same in every lane
        if (d) w = fe_mul(w, d == 1 ? a : (d == 2 ? a2 : a3));
    }
    Fe<C> x = fe_mul(a, w);
    Fe<C> b = fe_mul(x, w);
    const Fe<C> one = fe_one<C>();
#pragma unroll 1
    for (int i = 0; i < 32; i++) {
        Fe<C> c = b;
#pragma unroll 1
        for (int j = 0; j < 31 - i; j++) c = fe_sqr(c);
        const bool bit = !fe_eq(c, one);
        b = fe_select(bit, fe_mul(b, fe_from_const<C>(C::OMEGA_INV[32 - i])), b);
        if (i) x = fe_select(bit, fe_mul(x, fe_from_const<C>(C::OMEGA_INV[33 - i])), x);
    }
    is_square = fe_eq(fe_sqr(x), a);
    return fe_select(is_square, x, fe_zero<C>());
}

// ---- canonical integers <-> internal form (8 x u32 little-endian words) --------------------------------------
template <class C>
HALO_DEV Fe<C> fe_from_canonical_words(const uint32_t (&w)[8]) {  // any value below 2^256; reduced mod p
    return fe_mul(fe_unpack<C>(w), fe_from_const<C>(C::R2));
}
template <class C>
HALO_DEV void fe_to_canonical_words(const Fe<C>& x, uint32_t (&w)[8]) {
    Fe<C> raw_one = fe_zero<C>();
    raw_one.v[0] = 1;  // the integer 1: x R' * 1 / R' = x
    fe_pack(fe_canon(fe_mul(x, raw_one)), w);
}

// w < p, and w > (p - 1) / 2, for 256-bit words
template <class C>
HALO_DEV bool words_below_modulus(const uint32_t (&w)[8]) {
    bool lt = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {  // from the low word up: the highest differing word decides
        const uint32_t m = (uint32_t)(C::MODULUS64[i >> 1] >> (32 * (i & 1)));
        lt = w[i] < m || (w[i] == m && lt);
    }
    return lt;
}
template <class C>
HALO_DEV bool words_above_half(const uint32_t (&w)[8]) {
    bool gt = false;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t m = (uint32_t)(C::MODULUS64[i >> 1] >> (32 * (i & 1)));
        const uint32_t mh = i < 7 ? (uint32_t)(C::MODULUS64[(i + 1) >> 1] >> (32 * ((i + 1) & 1))) : 0u;
        const uint32_t h = (m >> 1) | (mh << 31);  // word i of (p - 1) / 2 = p >> 1
        gt = w[i] > h || (w[i] == h && gt);
    }
    return gt;
}

HALO_ARITH_END
