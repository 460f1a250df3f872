// Prints what halo_amd/csrc/sponge_plan.hpp plans (tests/test_sponge_plan.py).  One command per input line:
//   steps E C    from each of Absorbed(0), Absorbed(1), Absorbed(2), Squeezed(1), Squeezed(2), e <= E absorbed elements
//                and then c <= C squeezes: one line "s squeezed n e c squeezed' n' permutations"
//   items 0 0    one line "i kind pallas elements" per kind (0 point, 1 fr, 2 fq) and curve (1 Pallas, 0 Vesta)
//   plan T CU K  the launch of K sponges with tuning value T (1 or 3 pins the lanes, 0 leaves them free) on CU compute
//                units: one line "p T CU K lanes blocks threads"
#include <cstdio>
#include <cstring>

#include "sponge_plan.hpp"

int main() {
    char cmd[16];
    unsigned long E, C;
    while (std::scanf("%15s %lu %lu", cmd, &E, &C) == 3) {
        if (!std::strcmp(cmd, "plan")) {
            unsigned long K;
            if (std::scanf("%lu", &K) != 1) return 1;
            const int lanes = halo::sponge_lanes((long long)E, K, (int)C);
            const halo::HashGrid g = halo::hash_grid(K, lanes);
            std::printf("p %lu %lu %lu %d %u %u\n", E, C, K, lanes, g.blocks, g.threads);
            continue;
        }
        if (!std::strcmp(cmd, "items")) {
            for (int kind = 0; kind < 3; kind++)
                for (int pallas = 0; pallas < 2; pallas++)
                    std::printf("i %d %d %zu\n", kind, pallas, halo::sponge_item_elements(kind, pallas != 0));
            continue;
        }
        const halo::SpongeMode starts[5] = {{false, 0}, {false, 1}, {false, 2}, {true, 1}, {true, 2}};
        for (const halo::SpongeMode& m : starts)
            for (size_t e = 0; e <= E; e++)
                for (size_t c = 0; c <= C; c++) {
                    const halo::SpongeStep s = halo::sponge_step(m, e, c);
                    std::printf("s %d %d %zu %zu %d %d %zu\n", (int)m.squeezed, m.n, e, c, (int)s.mode.squeezed, s.mode.n,
                                s.permutations);
                }
    }
    return 0;
}
