// The descent of the bisecting decider (decider.hip decide_bisect_device): which instances of a rejected combined
// batch are the wrong ones.  Host-only and free of HIP types, like decider_plan.hpp, so a plain C++17 compiler
// builds it and a CPU stand-in runs the same loop as the device code (tests/test_decider_bisect.py).
//
// D(S) = sum_{i in S} rho_i U_i - Commit(sum_{i in S} rho_i h_i) is additive over disjoint sets of instances and
// nonzero iff S holds a wrong instance (up to a prover guessing rho; exactly so for a single instance, rho_i != 0).
// A failing node [lo, hi) of two or more instances splits into left = [lo, lo + (hi - lo) / 2) and the rest: one
// combined pass over the left half gives D(left), and D(right) = D(node) - D(left) costs no pass.  One level of the
// tree is one step: its failing internal nodes (the frontier) give one coefficient row each, the rows are
// committed in groups (decider_group, as in exact mode), and the two flags of every node (left fails, right fails)
// make the next frontier; a failing child of one instance is a verdict.  With b wrong instances among k the rows
// beyond the root pass number at most min(k - 1, b ceil(lg k)), over at most ceil(lg k) levels.
#pragma once
#include <vector>

#include "decider_plan.hpp"

namespace halo {

struct BisectNode {  // a failing node of two or more instances
    uint32_t lo, mid, hi;  // left = [lo, mid), right = [mid, hi)
    uint32_t src;          // where its defect lies among the child defects of the level above: 2 parent + side
};

inline uint32_t bisect_mid(uint32_t lo, uint32_t hi) { return lo + (hi - lo) / 2; }
inline BisectNode bisect_node(uint32_t lo, uint32_t hi, uint32_t src) { return BisectNode{lo, bisect_mid(lo, hi), hi, src}; }

// From a level's nodes and their flags (flags[2 s] = the left half of node s fails, flags[2 s + 1] = the right one)
// to the next level's nodes; a failing half of one instance i is a leaf: ok[i] = 0.
inline void bisect_step(const std::vector<BisectNode>& level, const uint8_t* flags, std::vector<BisectNode>& next,
                        uint8_t* ok) {
    next.clear();
    for (size_t s = 0; s < level.size(); s++) {
        const BisectNode& nd = level[s];
        const uint32_t lo[2] = {nd.lo, nd.mid}, hi[2] = {nd.mid, nd.hi};
        for (int side = 0; side < 2; side++) {
            if (!flags[2 * s + side]) continue;
            if (hi[side] - lo[side] == 1)
                ok[lo[side]] = 0;
            else
                next.push_back(bisect_node(lo[side], hi[side], (uint32_t)(2 * s + side)));
        }
    }
}

// The descent below a failing root [0, k), k >= 2, of instances with n coefficients each.  ok: k bytes the caller
// has set to 1 for every instance that takes part; the wrong ones are cleared.  `ev` does the work of a level:
//   int ev.rows(const BisectNode* level, size_t f, size_t r0, size_t m)
//       D(left) of the nodes r0 .. r0 + m - 1, one group: their m coefficient rows and one batch of commitments
//   int ev.split(const BisectNode* level, size_t f, uint8_t* flags)
//       the child defects of all f nodes (child 2 s + side of this level is what BisectNode::src names in the
//       next) and their 2 f flags
// both returning 0 or an error code that ends the descent.  budget and W: decider_group's.
template <class Eval>
int bisect_descend(size_t k, size_t n, size_t budget, int W, Eval& ev, uint8_t* ok) {
    std::vector<BisectNode> level{bisect_node(0, (uint32_t)k, 0)}, next;
    std::vector<uint8_t> flags;
    while (!level.empty()) {
        const size_t f = level.size(), g = decider_group(n, f, budget, W);
        for (size_t r0 = 0; r0 < f; r0 += g)
            if (const int rc = ev.rows(level.data(), f, r0, std::min(g, f - r0))) return rc;
        flags.assign(2 * f, 0);
        if (const int rc = ev.split(level.data(), f, flags.data())) return rc;
        bisect_step(level, flags.data(), next, ok);
        level.swap(next);
    }
    return 0;
}

}  // namespace halo
