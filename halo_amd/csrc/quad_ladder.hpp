// The quad-cooperative variable-base ladder of the Schnorr verification (schnorr.hip, k_schnorr_verify) and
// of the batched linear combinations of points (lincomb.hip, k_lincomb_terms), in the arithmetic namespace of the
// including unit: the on-curve test of an input point, the signed 4-bit recoding of a GLV half-scalar, the quad
// addition with its trivial-case rule and the build of a quad's table d P (1 <= d <= 8) in LDS.  A kernel keeps its
// own load, validity rule, decomposition, window loop (doublings and table terms) and epilogue.
//
// One aligned quad of lanes works on one point, every lane of the quad holding the same values (tree.hpp's
// quad doubling / addition); role = lane & 3, s1 = the wave lane of the quad's lane 0.  Quads of one wave stay
// in lockstep: an addition is skipped only when it is trivial for every quad.
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

// Eight canonical words as two uint4 (k_schnorr_hash's e_words).
HALO_DEV void words_from_u4(const uint4* p, uint32_t (&w)[8]) {
    const uint4 lo = p[0], hi = p[1];
    w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w, w[4] = hi.x, w[5] = hi.y, w[6] = hi.z, w[7] = hi.w;
}

// acc + t (t the same in every lane of the quad; trivial when either is the identity)
template <class F>
HALO_DEV XYZZ<F> quad_add(const XYZZ<F>& acc, const XYZZ<F>& t, bool t_is_id, uint32_t role, uint32_t s1) {
    const bool idp = xyzz_is_id(acc), idq = t_is_id || xyzz_is_id(t);
    XYZZ<F> r = xyzz_id<F>();
    if (!__all(idp || idq)) r = xyzz_add_quad(role == 1 ? t : acc, s1, s1 + 1, idp, idq);
    const XYZZ<F> sum = xyzz_quad_lane2(r);
    return idq ? acc : (idp ? t : sum);
}

constexpr int QUAD_TAB_U4 = 8 * 8;  // d P at d - 1 (1 <= d <= 8): XYZZ, 128 B each

// The quad's table in its LDS slice `pt` of QUAD_TAB_U4: d P at entry d - 1, P affine.  Eight block barriers: every
// lane of the block runs it.  (The first barrier also completes whatever the block staged before.)  A macro, not a
// function: with this loop one inlining level down, the compiler gives k_schnorr_verify 243 VGPRs for 237 and
// k_lincomb_terms other SGPRs; expanded in the kernel's body both compile as they always did.
#define QUAD_TABLE_BUILD(F, pt, P, role, s1)                                                                       \
    do {                                                                                                           \
        const XYZZ<F> p1_ = xyzz_from_aff(P);                                                                      \
        if ((role) == 0) xyzz_store((pt), p1_);                                                                    \
        __syncthreads();                                                                                           \
        XYZZ<F> prev_ = p1_;                                                                                       \
        for (int d_ = 2; d_ <= 8; d_++) {                                                                          \
            const XYZZ<F> v_ = (d_ & 1) ? quad_add(prev_, p1_, false, (role), (s1))                                \
                                        : xyzz_dbl_quad(xyzz_load<F>((pt) + 8 * (d_ / 2 - 1)));                    \
            if ((role) == 0) xyzz_store((pt) + 8 * (d_ - 1), v_);                                                  \
            __syncthreads();                                                                                       \
            prev_ = v_;                                                                                            \
        }                                                                                                          \
    } while (0)

HALO_ARITH_END
