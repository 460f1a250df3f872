// Prints what halo_amd/csrc/digits_core.hpp computes, one line of space-separated entries (hex) per
// command line read from stdin (tests/test_digits_core.py).  Built by the host C++ compiler alone:
// the header is free of HIP.
//   <mode> <c> <W> <flip 0|1> <64 hex digits: the folded integer, most significant first>
// modes: rt   run-time width c, run-time loop           (k_digits, k_rs_hist_sc<S, 0>)
//        rtu  run-time width c, loop unrolled 16 times  (the fused k_rs_scatter<8, S, false, 0>)
//        c16  constant width 16 (c and W ignored: all 16 windows)
//        c17  constant width 17 (all 15 windows)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "digits_core.hpp"

using namespace halo;

int main() {
    char line[512], mode[8], hex[80];
    while (fgets(line, sizeof line, stdin)) {
        int c = 0, W = 0, flip = 0;
        if (sscanf(line, "%7s %d %d %d %79s", mode, &c, &W, &flip, hex) != 5 || strlen(hex) != 64) {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
        uint32_t w8[8];
        for (int q = 0; q < 8; q++) {
            char part[9];
            memcpy(part, hex + 8 * (7 - q), 8);
            part[8] = 0;
            w8[q] = (uint32_t)strtoul(part, nullptr, 16);
        }
        const uint32_t fl = flip ? 0x80000000u : 0u;
        uint32_t out[32];
        int n = 0;
        auto put = [&](int w, uint32_t e) {
            if (w != n || n >= 32) {  // in order, each window once
                fprintf(stderr, "window %d out of order\n", w);
                out[31] = 0;
                n = 33;
                return;
            }
            out[n++] = e;
        };
        if (!strcmp(mode, "rt"))
            signed_digit_entries<0, 0>(w8, fl, c, W, put);
        else if (!strcmp(mode, "rtu") && W <= 16)
            signed_digit_entries<0, 16>(w8, fl, c, W, put);
        else if (!strcmp(mode, "c16"))
            signed_digit_entries<16, 16>(w8, fl, c, W, put);
        else if (!strcmp(mode, "c17"))
            signed_digit_entries<17, 0>(w8, fl, c, W, put);
        else {
            fprintf(stderr, "bad mode: %s", line);
            return 2;
        }
        if (n > 32) return 3;
        for (int i = 0; i < n; i++) printf("%s%08" PRIx32, i ? " " : "", out[i]);
        printf("\n");
    }
    return 0;
}
