// Signed-window recoding of one MSM scalar (shared by k_digits in msm.hip and the fused first sort
// pass in sort.hip): the device wrapper around digits_core.hpp.
#pragma once
#include "digits_core.hpp"
#include "fields.hpp"

namespace halo {

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
    uint32_t w8[8];
    fe_ark_to_canonical_words<S>(scalar, w8);
    // t = p - s, and the borrow of t - s: set when p - s < s
    uint32_t t8[8];
    int64_t br = 0, lt = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int64_t d = (int64_t)(uint32_t)(S::MODULUS64[q >> 1] >> (32 * (q & 1))) - (int64_t)w8[q] + br;
        t8[q] = (uint32_t)d;
        br = d >> 32;
        lt = ((int64_t)t8[q] - (int64_t)w8[q] + lt) >> 32;
    }
    const bool neg = lt != 0;
#pragma unroll
    for (int q = 0; q < 8; q++) w8[q] = neg ? t8[q] : w8[q];
    signed_digit_entries<C, WMAX>(w8, neg ? 0x80000000u : 0u, c, W, f);
}

}  // namespace halo
