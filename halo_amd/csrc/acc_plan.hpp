// The counts of an accumulation's ASDL transcript and of its alpha^j ladder (acc_fs.hip).  Free of HIP: standard
// headers only, so the host C++ compiler builds it alone (tests/acc_plan_dump.cpp, tests/test_acc_plan.py); the
// functions are constexpr, which also makes them callable from the kernels.
#pragma once
#include <cstddef>

namespace halo {

// Elements the ASDL sponge of one accumulation absorbs (acc.rs:135,158-166): the label, the m (lg + 1) challenges
// of its instances at ns base-field elements each (2 on Pallas, 1 on Vesta), the two coordinates of the m points U.
constexpr size_t acc_transcript_elements(size_t m, size_t lg, size_t ns) { return 1 + ns * m * (lg + 1) + 2 * m; }

// Permutations of the rate-2 sponge while it absorbs them; the two squeezes follow.
constexpr size_t acc_absorb_permutations(size_t m, size_t lg, size_t ns) { return (acc_transcript_elements(m, lg, ns) + 1) / 2; }

// Steps of the square-and-multiply ladder that forms alpha^j for every j < m: the bit length of m - 1.
constexpr int acc_ladder_steps(size_t m) {
    int b = 0;
    for (size_t x = m ? m - 1 : 0; x; x >>= 1) b++;
    return b;
}

}  // namespace halo
