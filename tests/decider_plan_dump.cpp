// Prints what halo_amd/csrc/decider_plan.hpp computes (tests/test_decider_plan.py).  Built by the host C++
// compiler alone: the header is free of HIP.  One command line per sweep, read from stdin:
//   sweep lg_lo lg_hi k_hi budget W    for every n in {2^lg - 1, 2^lg, 2^lg + 1 : lg_lo <= lg <= lg_hi} (n >= 1) and
//                                      every 1 <= k <= k_hi, checks the plan's properties and prints one JSON
//                                      object: the number of plans checked, the violations, a few samples
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "decider_plan.hpp"

using namespace halo;

int main() {
    char line[256], cmd[16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[5] = {};
        const int got = sscanf(line, "%15s %llu %llu %llu %llu %llu", cmd, a, a + 1, a + 2, a + 3, a + 4);
        if (got < 2) continue;
        if (!strcmp(cmd, "sweep") && got == 6) {
            const size_t budget = a[3];
            const int W = (int)a[4];
            unsigned long long checked = 0, bad_g = 0, bad_budget = 0, bad_cover = 0, bad_entries = 0, bad_clamp = 0;
            for (unsigned lg = (unsigned)a[0]; lg <= (unsigned)a[1]; lg++)
                for (int off = -1; off <= 1; off++) {
                    const size_t n = ((size_t)1 << lg) + off;
                    if (n < 1 || n > ((size_t)1 << a[1])) continue;
                    for (size_t k = 1; k <= a[2]; k++) {
                        const size_t g = decider_group(n, k, budget, W), groups = decider_groups(k, g);
                        checked++;
                        if (g < 1) bad_g++;
                        if (g > k) bad_clamp++;
                        if (g * n > budget && g != 1) bad_budget++;
                        // the groups [j g, min((j + 1) g, k)) cover 0 .. k exactly: the last one is not empty
                        if (g >= 1 && (groups * g < k || (groups - 1) * g >= k)) bad_cover++;
                        if ((unsigned __int128)g * (unsigned)W * n >= ((unsigned __int128)1 << 32)) bad_entries++;
                    }
                }
            printf("{\"checked\": %llu, \"g_below_1\": %llu, \"g_above_k\": %llu, \"over_budget\": %llu, \"cover\": %llu, "
                   "\"entries\": %llu}\n",
                   checked, bad_g, bad_clamp, bad_budget, bad_cover, bad_entries);
        } else if (!strcmp(cmd, "plan") && got == 5) {
            const size_t g = decider_group(a[0], a[1], a[2], (int)a[3]);
            printf("{\"g\": %zu, \"groups\": %zu}\n", g, decider_groups(a[1], g));
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
