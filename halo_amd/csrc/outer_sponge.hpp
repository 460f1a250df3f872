// Device Fiat-Shamir sponge of a Pasta curve (crates/poseidon/src/outer_sponge.rs:11-100, Sponge<P>) over
// the base-field Poseidon sponge of poseidon.hpp, in either lane layout: the protocol label absorbed
// first, absorb_g of a WrappedPoint (x then y; the identity is its own (0, 0) limbs), absorb_fr of a
// scalar and challenge().
//
// The two fields of a curve differ in size, and the two directions are asymmetric (outer_sponge.rs:63-95):
//   scalar field < base field (Vesta)   absorb_fr absorbs the scalar's canonical integer as ONE base-field
//                                       element; challenge() shifts the squeezed integer right by one bit
//   scalar field > base field (Pallas)  absorb_fr absorbs x >> 1 and then the low bit, TWO elements;
//                                       challenge() takes the squeezed integer unchanged
//
// Every absorb call site inlines a copy of the 55-round permutation (about 3000 instructions in the
// one-lane layout), so the reference's calls are offered element by element: the label absorb is
// absorb(label_element(protocol)), absorb_g(P) is absorb(g_element(P, 0)), absorb(g_element(P, 1)), and
// absorb_fr(s) is absorb(fr_element(s, j)) for j < FR_ELEMENTS.  A kernel walks its transcript as a
// sequence of such elements through ONE absorb() call in a loop, as k_schnorr_hash does.
#pragma once
#include "curve.hpp"
#include "poseidon.hpp"

HALO_ARITH_BEGIN
namespace poseidon {

// canonical integer of a base-field element: the Montgomery product with the plain integer 1 divides R' out
template <class F>
HALO_DEV void fe_to_canonical_words(const Fe<F>& v, uint32_t (&w)[8]) {
    Fe<F> raw1 = fe_zero<F>();
    raw1.v[0] = 1;
    fe_pack(fe_canon(fe_mul(v, raw1)), w);
}
// ... and back, for an integer below 2^256 (reduced by the multiplication)
template <class F>
HALO_DEV Fe<F> fe_from_canonical_words(const uint32_t (&w)[8]) {
    return fe_mul(fe_unpack<F>(w), fe_from_const<F>(F::R2));
}

// a small integer (a count, an index) as a field element
template <class F>
HALO_DEV Fe<F> fe_from_u64(uint64_t x) {
    const uint32_t e[8] = {(uint32_t)x, (uint32_t)(x >> 32), 0u, 0u, 0u, 0u, 0u, 0u};
    return fe_from_canonical_words<F>(e);
}

template <class Cv, int LANES>
struct OuterSponge {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    // the moduli differ in limb 1 first
    static constexpr bool SCALAR_BELOW_BASE = S::MODULUS64[1] < F::MODULUS64[1];
    static constexpr int FR_ELEMENTS = SCALAR_BELOW_BASE ? 1 : 2;  // base-field elements per absorbed scalar

    Sponge<F, LANES> inner;

    // A fresh sponge; the first element of every transcript is label_element(protocol).
    HALO_DEV void init(const uint32_t* lds_tab) { inner.init(lds_tab); }
    // A transcript carried through device memory between two kernels (poseidon::STATE_U4 uint4, the same
    // bytes in both lane layouts); mine: this lane belongs to the sponge that is stored.
    HALO_DEV void store(uint4* dst, bool mine) const { inner.store(dst, mine); }
    HALO_DEV void load(const uint32_t* lds_tab, const uint4* src) { inner.load(lds_tab, src); }

    // Protocols::{PCDL = 0, ASDL = 1, PLONK = 2, SIGNATURE = 3} as a field element (outer_sponge.rs:17-29)
    static HALO_DEV Fe<F> label_element(int protocol) {
        Fe<F> r = fe_zero<F>();
        const Fe<F> one = fe_one<F>();
        for (int i = 0; i < protocol; i++) r = fe_add(r, one);
        return r;
    }
    // coordinate j (0: x, 1: y) of a WrappedPoint
    static HALO_DEV Fe<F> g_element(const uint4* wrapped, int j) { return fe_from_ark<F>(wrapped + 2 * j); }
    // element j < FR_ELEMENTS of a scalar given as its canonical integer
    static HALO_DEV Fe<F> fr_element(const uint32_t (&w)[8], int j) {
        uint32_t e[8];
#pragma unroll
        for (int q = 0; q < 8; q++) {
            if (SCALAR_BELOW_BASE)
                e[q] = w[q];
            else if (j == 0)
                e[q] = (w[q] >> 1) | (q < 7 ? w[q + 1] << 31 : 0u);
            else
                e[q] = q == 0 ? (w[0] & 1u) : 0u;
        }
        return fe_from_canonical_words<F>(e);
    }

    HALO_DEV void absorb(const Fe<F>& x) { inner.absorb(x); }

    // The next challenge as the scalar's canonical integer (below the scalar modulus in both directions).
    HALO_DEV void challenge(uint32_t (&w)[8]) { challenge_words(inner.squeeze(), w); }
    // ... of an element that the inner sponge squeezed (a kernel whose one squeeze call serves several sponges)
    static HALO_DEV void challenge_words(const Fe<F>& squeezed, uint32_t (&w)[8]) {
        fe_to_canonical_words(squeezed, w);
        if (SCALAR_BELOW_BASE) {
#pragma unroll
            for (int q = 0; q < 8; q++) w[q] = (w[q] >> 1) | (q < 7 ? w[q + 1] << 31 : 0u);
        }
    }
};

// A challenge's canonical integer as an ark scalar of the curve
template <class S>
HALO_DEV void scalar_words_to_ark(uint4* out, const uint32_t (&w)[8]) {
    fe_to_ark(out, fe_from_canonical_words<S>(w));
}

}  // namespace poseidon
HALO_ARITH_END
