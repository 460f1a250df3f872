// Signed-window recoding of one MSM scalar (shared by k_digits in msm.hip and the fused first sort
// pass in sort.hip): the device wrapper around digits_core.hpp.
#pragma once
#include "digits_core.hpp"
#include "fields.hpp"

namespace halo {

// Step one of the recoding: the ark scalar as its folded canonical integer min(s, p - s) < 2^254 with
// the fold's sign in bit 255 (digits_core.hpp digits_fold) -- the one Montgomery multiplication, the
// comparison with p / 2 and the subtraction from p that a scalar's recoding costs before any window is cut.
template <class S>
HALO_DEV void scalar_fold(const uint4* scalar, uint32_t (&f8)[8]) {
    fe_ark_to_canonical_words<S>(scalar, f8);
    uint32_t p8[8];
#pragma unroll
    for (int q = 0; q < 8; q++) p8[q] = (uint32_t)(S::MODULUS64[q >> 1] >> (32 * (q & 1)));
    digits_fold(f8, p8);
}

// Step two: the windows of a folded scalar (scalar_fold's 8 words), f(w, digit) as below.
template <int WMAX = 0, int C = 0, class Fn>
HALO_DEV void folded_signed_digits(const uint32_t (&f8)[8], int c, int W, Fn&& f) {
    uint32_t w8[8];
#pragma unroll
    for (int q = 0; q < 8; q++) w8[q] = f8[q];
    const uint32_t flip = digits_unfold(w8);
    signed_digit_entries<C, WMAX>(w8, flip, c, W, f);
}

// The W signed c-bit digits of an ark scalar, as sort entries: DIGIT_NONE for a zero digit, else
// (|d| - 1) with bit 31 = sign.  s > p / 2 is replaced by p - s and every digit's sign flipped
// (s P = -(p - s) P), so W = ceil(255 / c) windows suffice.  f(w, digit) is called for w < W in order.
// WMAX > 0: the window loop is unrolled WMAX times (W <= WMAX), so f sees a compile-time w (register
// arrays indexed by w stay in registers); WMAX = 0: a runtime loop.
// C > 0: the window width is the compile-time constant C (the caller uses this instantiation only
// for c == C and W == ceil(255 / C), which it then ignores): every window is one funnel shift and one
// mask, and the loop is unrolled whatever WMAX.
template <class S, int WMAX = 0, int C = 0, class Fn>
HALO_DEV void scalar_signed_digits(const uint4* scalar, int c, int W, Fn&& f) {
    uint32_t f8[8];
    scalar_fold<S>(scalar, f8);
    folded_signed_digits<WMAX, C>(f8, c, W, f);
}

}  // namespace halo
