// Prints what halo_amd/csrc/rho_plan.hpp computes (tests/test_rho_plan.py).  Built by the host C++ compiler alone:
// the header is free of HIP.  One command per line, read from stdin, one JSON object each:
//   levels k_hi     for every 1 <= k <= k_hi walks the level counts of the tree and checks them: each is
//                   ceil(previous / 2) (pairs hashed, an odd element promoted), the walk ends at 1 after
//                   rho_levels(k) steps, that is ceil(lg k), and rho_launches(k) is two more
//   counts k        the level counts of one k, the leaves first
//   leaf lg_hi      the leaf's element and permutation counts for both directions at lg n = 0 .. lg_hi
//   zero w0 .. w7   rho_zero_becomes_one of the eight words
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "rho_plan.hpp"

using namespace halo;

static unsigned ceil_lg(size_t k) {
    unsigned l = 0;
    while (((size_t)1 << l) < k) l++;
    return l;
}

int main() {
    char line[256], cmd[16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[8] = {};
        const int got = sscanf(line, "%15s %llu %llu %llu %llu %llu %llu %llu %llu", cmd, a, a + 1, a + 2, a + 3, a + 4, a + 5,
                               a + 6, a + 7);
        if (got < 2) continue;
        if (!strcmp(cmd, "levels") && got == 2) {
            unsigned long long checked = 0, bad_halving = 0, bad_end = 0, bad_levels = 0, bad_launches = 0;
            for (size_t k = 1; k <= a[0]; k++) {
                unsigned steps = 0;
                size_t c = k;
                while (c > 1) {
                    const size_t next = rho_next_level(c);
                    if (next != c / 2 + (c & 1)) bad_halving++;
                    c = next;
                    steps++;
                }
                checked++;
                if (c != 1) bad_end++;
                if (steps != rho_levels(k) || rho_levels(k) != ceil_lg(k)) bad_levels++;
                if (rho_launches(k) != 2 + ceil_lg(k)) bad_launches++;
            }
            printf("{\"checked\": %llu, \"halving\": %llu, \"end\": %llu, \"levels\": %llu, \"launches\": %llu, \"launches_0\": %u}\n",
                   checked, bad_halving, bad_end, bad_levels, bad_launches, rho_launches(0));
        } else if (!strcmp(cmd, "counts") && got == 2) {
            printf("{\"counts\": [%llu", a[0]);
            for (size_t c = a[0]; c > 1;) printf(", %zu", c = rho_next_level(c));
            printf("], \"levels\": %u, \"launches\": %u}\n", rho_levels(a[0]), rho_launches(a[0]));
        } else if (!strcmp(cmd, "leaf") && got == 2) {
            printf("{\"below\": [");
            for (unsigned lg = 0; lg <= a[0]; lg++)
                printf("%s[%zu, %zu]", lg ? ", " : "", rho_leaf_elements(true, lg), rho_leaf_permutations(true, lg));
            printf("], \"above\": [");
            for (unsigned lg = 0; lg <= a[0]; lg++)
                printf("%s[%zu, %zu]", lg ? ", " : "", rho_leaf_elements(false, lg), rho_leaf_permutations(false, lg));
            printf("]}\n");
        } else if (!strcmp(cmd, "zero") && got == 9) {
            uint32_t w[8];
            for (int q = 0; q < 8; q++) w[q] = (uint32_t)a[q];
            rho_zero_becomes_one(w);
            printf("{\"w\": [%u, %u, %u, %u, %u, %u, %u, %u]}\n", w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]);
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
