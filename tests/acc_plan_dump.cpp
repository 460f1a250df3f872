// Prints what halo_amd/csrc/acc_plan.hpp counts (tests/test_acc_plan.py).  One command per input line:
//   sweep M LG    every m in 1 .. M, lg in 0 .. LG, ns in {1, 2}: one line "m lg ns elements permutations steps"
#include <cstdio>

#include "acc_plan.hpp"

int main() {
    char cmd[16];
    unsigned long M, LG;
    while (std::scanf("%15s %lu %lu", cmd, &M, &LG) == 3)
        for (size_t m = 1; m <= M; m++)
            for (size_t lg = 0; lg <= LG; lg++)
                for (size_t ns = 1; ns <= 2; ns++)
                    std::printf("%zu %zu %zu %zu %zu %d\n", m, lg, ns, halo::acc_transcript_elements(m, lg, ns),
                                halo::acc_absorb_permutations(m, lg, ns), halo::acc_ladder_steps(m));
    return 0;
}
