// What the host knows about a Fiat-Shamir sponge handle without asking the device (sponge.hip): the base-field
// elements of an absorbed item and the (squeezed, n) mode of the rate-2 sponge after a call, with the permutations
// the call runs (inner_sponge.rs absorb / squeeze).  Free of HIP: standard headers only, so the host C++ compiler
// builds it alone (tests/sponge_plan_dump.cpp, tests/test_sponge_plan.py); the functions are constexpr.
// Also the launch plan of every kernel that runs one sponge per lane or per three lanes (sponge_launch.hpp): the
// lane rule and the grid.
#pragma once
#include <cstddef>

namespace halo {

enum SpongeKind { SPONGE_G = 0, SPONGE_FR = 1, SPONGE_FQ = 2 };  // absorb_g, absorb_fr, absorb_fq
constexpr int SPONGE_RATE = 2;

// Elements per absorbed item: a point is (x, y); a scalar is one element where the scalar field is the smaller one
// (Vesta) and (x >> 1, x & 1) where it is the larger (Pallas; outer_sponge.rs:63-84); an fq is itself.
constexpr size_t sponge_item_elements(int kind, bool pallas) {
    return kind == SPONGE_G ? 2 : kind == SPONGE_FR ? (pallas ? 2 : 1) : 1;
}

struct SpongeMode {  // Absorbed(n) or Squeezed(n); a fresh sponge is Absorbed(0)
    bool squeezed;
    int n;
};
struct SpongeStep {
    SpongeMode mode;
    size_t permutations;
};

// r more operations of the kind the sponge is in, from fill n <= RATE (n + r >= 1): every operation that finds the
// rate full permutes first and leaves fill 1.
constexpr SpongeStep sponge_run(bool squeezed, size_t n, size_t r) {
    const size_t t = n + r, perms = (t - 1) / SPONGE_RATE;
    return {{squeezed, (int)(t - SPONGE_RATE * perms)}, perms};
}

// The mode after e absorbed elements and then c squeezes, and the permutations on the way.  The first absorb after
// a squeeze only changes the mode (fill 1); the first squeeze after an absorb always permutes.
constexpr SpongeStep sponge_step(SpongeMode m, size_t e, size_t c) {
    size_t perms = 0;
    if (e) {
        const SpongeStep a = m.squeezed ? sponge_run(false, 1, e - 1) : sponge_run(false, (size_t)m.n, e);
        m = a.mode;
        perms += a.permutations;
    }
    if (c) {
        const SpongeStep s = m.squeezed ? sponge_run(true, (size_t)m.n, c) : sponge_run(true, 1, c - 1);
        perms += s.permutations + (m.squeezed ? 0 : 1);
        m = s.mode;
    }
    return {m, perms};
}

// ---- the launch plan of a batch of k sponges -------------------------------------------------------------------
constexpr size_t SPONGES_PER_WAVE_1 = 64;  // one lane per sponge
constexpr size_t SPONGES_PER_WAVE_3 = 21;  // three lanes per sponge; lane 63 idles along with sponge 20
constexpr size_t sponge_waves(size_t k, int lanes) {
    const size_t per = lanes == 1 ? SPONGES_PER_WAVE_1 : SPONGES_PER_WAVE_3;
    return (k + per - 1) / per;
}

// Lanes per sponge.  Three lanes triple the waves and cut the dependent chain to a third, which pays while the
// batch leaves SIMDs short of work: measured on the MI355X, 40 000 hashes of 15 elements take
// 1.77 ms on 1905 three-lane waves against 2.72 ms on 625 one-lane waves, but 65 536 take 3.46 ms on 3121 three-lane
// waves against 2.72 ms on 1024 one-lane waves, and from there on the one-lane layout stays 5-20 % ahead (its lanes
// are all busy and it has no crossbar traffic).  So: three lanes while their waves number at most two per SIMD
// (eight per CU).  `tune` is the poseidon_lanes tuning key: 1 or 3 pins the layout, anything else leaves it free.
constexpr int sponge_lanes(long long tune, size_t k, int num_cu) {
    if (tune == 1 || tune == 3) return (int)tune;
    return sponge_waves(k, 3) <= (size_t)8 * (size_t)num_cu ? 3 : 1;
}

struct HashGrid {
    unsigned blocks, threads;
};
// Whole waves that cover k sponges: one wave per block while they are few (small batches spread over the CUs),
// four from 4097 waves on.  The last block may hold waves with no sponge: less than one block is wasted.
constexpr HashGrid hash_grid(size_t k, int lanes) {
    const size_t waves = sponge_waves(k, lanes);
    const unsigned wpb = waves > 4096 ? 4 : 1;
    return {(unsigned)((waves + wpb - 1) / wpb), 64 * wpb};
}

}  // namespace halo
