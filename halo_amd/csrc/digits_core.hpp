// Signed-window recoding of a 256-bit integer into the MSM's sort entries: the arithmetic core of
// digits.hpp.  Free of HIP types and of the field code, so a plain C++17 compiler builds it
// (tests/test_digits_core.py, tests/test_digits_two_step.py); hipcc compiles the same text for the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define HALO_DIGITS_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define HALO_DIGITS_FN inline
#endif
#if defined(__clang__)
#define HALO_DIGITS_UNROLL _Pragma("unroll")
#else
#define HALO_DIGITS_UNROLL  // (a host compiler that does not know the pragma)
#endif

namespace halo {

constexpr uint32_t DIGIT_NONE = 0xffffffffu;

// The low 32 bits of (hi : lo) >> s, 0 <= s < 32 (v_alignbit_b32; s = 0 gives lo)
HALO_DIGITS_FN uint32_t digits_funnel(uint32_t hi, uint32_t lo, uint32_t s) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
}

// One window.  v = raw + carry <= 2^c is the unsigned digit; v > 2^(c-1) becomes d = v - 2^c < 0 with a
// carry into the next window.  The entry is (|d| - 1) | sign, and DIGIT_NONE for d = 0 -- which needs no
// test of its own: |d| - 1 is then 0xffffffff, and OR-ing the sign into it changes nothing.  No branch:
// m is all ones for a negative digit, (v ^ m) + ((2^c + 1) & m) = 2^c - v.
HALO_DIGITS_FN uint32_t digits_entry(uint32_t raw, uint32_t& carry, uint32_t half, uint32_t full, uint32_t flip) {
    const uint32_t v = raw + carry;
    carry = (uint32_t)(v > half);
    const uint32_t m = 0u - carry;
    const uint32_t mag = (v ^ m) + ((full + 1u) & m);
    return (mag - 1u) | ((carry << 31) ^ flip);
}

// The recoding in two steps, so that a scalar's conversion and fold are done once and its windows cut
// wherever they are needed (the fused first sort pass: the histogram kernel folds and stores, the
// scatter loads and cuts).
// Step one, digits_fold: the canonical integer s < p in w8 (p8: the modulus' words) becomes
// min(s, p - s) <= (p - 1) / 2 < 2^254, with the fold's sign in the spare bit 255: set when p - s < s, i.e. when
// p - s was taken and every digit's sign is to be inverted (s P = -(p - s) P).  32 B, as the scalar.
// Step two, digits_unfold: the folded integer back in w8 and the flip (0 or 0x80000000) as
// signed_digit_entries takes them.
HALO_DIGITS_FN void digits_fold(uint32_t (&w8)[8], const uint32_t (&p8)[8]) {
    // t = p - s, and the borrow of t - s: set when p - s < s
    uint32_t t8[8];
    int64_t br = 0, lt = 0;
    HALO_DIGITS_UNROLL
    for (int q = 0; q < 8; q++) {
        const int64_t d = (int64_t)p8[q] - (int64_t)w8[q] + br;
        t8[q] = (uint32_t)d;
        br = d >> 32;
        lt = ((int64_t)t8[q] - (int64_t)w8[q] + lt) >> 32;
    }
    const bool neg = lt != 0;
    HALO_DIGITS_UNROLL
    for (int q = 0; q < 8; q++) w8[q] = neg ? t8[q] : w8[q];
    w8[7] |= neg ? 0x80000000u : 0u;
}
HALO_DIGITS_FN uint32_t digits_unfold(uint32_t (&w8)[8]) {
    const uint32_t flip = w8[7] & 0x80000000u;
    w8[7] &= 0x7fffffffu;
    return flip;
}

// The W signed c-bit digits of the integer in w8 (8 words of 32 bits, least significant first; the
// caller has folded it to at most p / 2 < 2^254, so W = ceil(255 / c) windows take the last carry), as
// sort entries: DIGIT_NONE for a zero digit, else (|d| - 1) with bit 31 = the digit's sign, inverted when
// flip = 0x80000000 (the caller recodes p - s for s).  f(w, entry) is called for w < W in order.
//   C > 0: the window width is the constant C, and c and W are ignored: all ceil(255 / C) windows
//          are produced.  Every word index and shift of a window is a constant, so a window costs one
//          funnel shift and one mask, and the loop has a constant trip count and is unrolled.
//   C = 0: run-time width 1 <= c < 32.  The integer is shifted down by c after every window (seven
//          funnel shifts and a shift, all by the same amount) and the window read from word 0, so no word is
//          selected by a run-time index.  WMAX > 0 unrolls the loop WMAX times (W <= WMAX), so that f
//          sees a constant w: the windows from W on are skipped one by one, not by leaving the loop,
//          which would make the trip count a run-time value and keep the compiler from unrolling.
//          WMAX = 0 is a run-time loop.
template <int C>
constexpr int digits_windows() { return C > 0 ? (255 + C - 1) / C : 0; }

template <int C, int WMAX = 0, class Fn>
HALO_DIGITS_FN void signed_digit_entries(const uint32_t (&w8)[8], uint32_t flip, int c, int W, Fn&& f) {
    static_assert(C >= 0 && C < 32, "window width");
    uint32_t carry = 0;
    if constexpr (C > 0) {
        constexpr uint32_t full = 1u << C, half = full >> 1;
        static_assert(WMAX == 0 || WMAX >= digits_windows<C>(), "W <= WMAX");
        HALO_DIGITS_UNROLL
        for (int w = 0; w < digits_windows<C>(); w++) {
            const int bit = w * C, q = bit >> 5, s = bit & 31;  // q <= 7: bit <= 254
            const uint32_t hi = (q + 1 < 8 && s + C > 32) ? w8[q + 1] : 0u;
            const uint32_t raw = digits_funnel(hi, w8[q], (uint32_t)s) & (full - 1u);
            f(w, digits_entry(raw, carry, half, full, flip));
        }
    } else {
        const uint32_t full = 1u << c, half = full >> 1;
        uint32_t x[8];
        HALO_DIGITS_UNROLL
        for (int q = 0; q < 8; q++) x[q] = w8[q];
        auto window = [&](int w) {
            const uint32_t raw = x[0] & (full - 1u);
            HALO_DIGITS_UNROLL
            for (int q = 0; q < 7; q++) x[q] = digits_funnel(x[q + 1], x[q], (uint32_t)c);
            x[7] >>= c;
            f(w, digits_entry(raw, carry, half, full, flip));
        };
        if constexpr (WMAX > 0) {
            HALO_DIGITS_UNROLL
            for (int w = 0; w < WMAX; w++)
                if (w < W) window(w);
        } else {
            for (int w = 0; w < W; w++) window(w);
        }
    }
}

}  // namespace halo
