// The shape of the generator's fixed-base comb (fixed_base.hip): the window width, the recoding of
// a scalar into signed digits, the table index of (window, digit) and the grid of a batch.  Free of HIP types and
// of the field code, so a plain C++17 compiler builds it (tests/fixed_base_plan_dump.cpp,
// tests/test_fixed_base_plan.py); hipcc compiles the same text for the device.
//
// k G = sum_w d_w 2^(C w) G over W = ceil(256 / C) windows of C bits with signed digits |d_w| <= 2^(C-1): the
// table holds the affine multiples d 2^(C w) G for 1 <= d <= 2^(C-1), a negative digit negates y as the entry is
// read, a zero digit adds nothing.  No doublings.
//
// The recoding is NOT folded: the scalar k < r is recoded as it stands (the MSM's s -> min(s, r - s) would save
// nothing here, the digits are signed either way), so there is no sign rule beyond the digit's own sign:
// sum_w d_w 2^(C w) = k exactly.  No carry leaves the top window: both moduli are below 2^254 + 2^127, so the
// top window's raw value is at most floor((2^255 - 1) / 2^(C (W - 1))), and FB_TOP_MAX + 1 <= 2^(C-1) is asserted
// below for every integer under 2^255, which covers both fields.
#pragma once
#include <cstddef>
#include <cstdint>

#include "digits_core.hpp"

namespace halo {

#ifndef HALO_FB_C
#define HALO_FB_C 8  // an A/B build passes another width (make EXTRA=-DHALO_FB_C=4); DESIGN §4.6.2 has the measurement
#endif
constexpr int FB_C = HALO_FB_C;                     // window bits
constexpr int FB_WINDOWS = (256 + FB_C - 1) / FB_C;  // W
constexpr int FB_HALF = 1 << (FB_C - 1);            // entries per window: 1 <= d <= FB_HALF
constexpr int FB_ENTRIES = FB_WINDOWS * FB_HALF;
constexpr int FB_ENTRY_BYTES = 64;                  // internal affine (x, y), as the SRS points
constexpr size_t FB_TABLE_BYTES = (size_t)FB_ENTRIES * FB_ENTRY_BYTES;
constexpr int FB_THREADS = 128;                     // lanes per workgroup: one scalar each, one shared inversion

static_assert(256 % FB_C == 0 && FB_C >= 2 && FB_C <= 16, "the windows tile the 256 bits of the words exactly");
// top window of an integer below 2^255, plus the carry of the window below, is no negative digit
constexpr uint32_t FB_TOP_MAX = (uint32_t)(((1ull << 63) - 1) >> (64 - FB_C));
static_assert(FB_TOP_MAX + 1 <= (uint32_t)FB_HALF, "no carry out of the top window");

// The digits of one scalar, least significant window first, one per call of next(): the integer is shifted down
// by C bits after every window (seven funnel shifts and a shift) and the window read from word 0, so a rolled
// loop selects no word by a run-time index.  An entry is digits_core's: DIGIT_NONE for d = 0, else
// (|d| - 1) | (d < 0 ? 0x80000000 : 0).
struct FbRecoder {
    uint32_t x[8];
    uint32_t carry;
    HALO_DIGITS_FN void init(const uint32_t (&w8)[8]) {
        HALO_DIGITS_UNROLL
        for (int q = 0; q < 8; q++) x[q] = w8[q];
        carry = 0;
    }
    HALO_DIGITS_FN uint32_t next() {
        constexpr uint32_t full = 1u << FB_C, half = full >> 1;
        const uint32_t raw = x[0] & (full - 1u);
        HALO_DIGITS_UNROLL
        for (int q = 0; q < 7; q++) x[q] = digits_funnel(x[q + 1], x[q], (uint32_t)FB_C);
        x[7] >>= FB_C;
        return digits_entry(raw, carry, half, full, 0u);
    }
};

// An entry that is not DIGIT_NONE: its table slot, and whether y is negated.
HALO_DIGITS_FN uint32_t fb_table_index(int w, uint32_t entry) { return (uint32_t)w * FB_HALF + (entry & 0x7fffffffu); }
HALO_DIGITS_FN bool fb_entry_negative(uint32_t entry) { return (entry >> 31) != 0; }

// Workgroups of FB_THREADS lanes over `lanes` scalars (at least one).
inline unsigned fb_blocks(size_t lanes) {
    const size_t b = (lanes + FB_THREADS - 1) / FB_THREADS;
    return (unsigned)(b ? b : 1);
}

}  // namespace halo
