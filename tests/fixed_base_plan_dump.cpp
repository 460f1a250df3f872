// Prints what halo_amd/csrc/fixed_base_plan.hpp computes (tests/test_fixed_base_plan.py).  Built by the host C++
// compiler alone: the header is free of HIP.  One command per line, read from stdin, one JSON object each:
//   plan             the constants: window bits, windows, entries per window, table entries and bytes, lanes
//   digits w0 .. w7  the recoding of the integer with these eight 32-bit words (least significant first, decimal):
//                    the W signed digits, least significant window first, the table index of each nonzero one
//                    (-1 for a zero digit) and the carry out of the top window
//   grid k           the workgroups and lanes per workgroup of a batch of k scalars
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "fixed_base_plan.hpp"

using namespace halo;

int main() {
    char line[512], cmd[16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[8] = {};
        const int got = sscanf(line, "%15s %llu %llu %llu %llu %llu %llu %llu %llu", cmd, a, a + 1, a + 2, a + 3, a + 4, a + 5,
                               a + 6, a + 7);
        if (got < 1) continue;
        if (!strcmp(cmd, "plan") && got == 1) {
            printf("{\"c\": %d, \"windows\": %d, \"half\": %d, \"entries\": %d, \"entry_bytes\": %d, \"table_bytes\": %zu, "
                   "\"threads\": %d}\n",
                   FB_C, FB_WINDOWS, FB_HALF, FB_ENTRIES, FB_ENTRY_BYTES, FB_TABLE_BYTES, FB_THREADS);
        } else if (!strcmp(cmd, "digits") && got == 9) {
            uint32_t w8[8], all[FB_WINDOWS];
            for (int q = 0; q < 8; q++) w8[q] = (uint32_t)a[q];
            FbRecoder rc;  // what the kernel runs
            rc.init(w8);
            printf("{\"digits\": [");
            for (int w = 0; w < FB_WINDOWS; w++) {
                const uint32_t e = all[w] = rc.next();
                const long long mag = e == DIGIT_NONE ? 0 : (long long)(e & 0x7fffffffu) + 1;
                printf("%s%lld", w ? ", " : "", e != DIGIT_NONE && fb_entry_negative(e) ? -mag : mag);
            }
            printf("], \"index\": [");
            for (int w = 0; w < FB_WINDOWS; w++)
                printf("%s%lld", w ? ", " : "", all[w] == DIGIT_NONE ? -1ll : (long long)fb_table_index(w, all[w]));
            printf("], \"carry\": %u}\n", rc.carry);
        } else if (!strcmp(cmd, "grid") && got == 2) {
            printf("{\"blocks\": %u, \"threads\": %d}\n", fb_blocks((size_t)a[0]), FB_THREADS);
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
