// The descent of the bisecting Schnorr batch (schnorr_bisect.hip sig_bisect_device): which signatures of a rejected
// combined batch are the wrong ones.  Host-only and free of HIP types, like decider_bisect.hpp, whose nodes and split
// rule it shares, so a plain C++17 compiler builds it and a CPU stand-in runs the same loop as the device code
// (tests/test_schnorr_bisect.py).
//
// D(S) = (sum_{i in S} rho_i s_i) G - sum_{i in S} rho_i R_i - sum_{i in S} rho_i e_i pk_i is additive over disjoint
// sets of items and nonzero iff S holds a wrong live item (up to a signer guessing rho; exactly so for a single item,
// rho_i != 0).  A failing node [lo, hi) splits into left = [lo, lo + (hi - lo) / 2) and the rest: one pass over the
// left half gives D(left), and D(right) = D(node) - D(left) costs no pass.  A failing child of one item is a verdict.
//
// Unlike the decider's rows, a pass here competes with a cheap exact test, the ladder over a slice of the batch
// (k_schnorr_verify, about as dear per item whatever the slice).  With c the number of ladder items that cost as
// much as one pass, two rules keep the descent from costing more than it saves:
//
//   leaf    a failing node of 2 .. L items is resolved by the ladder over its slice, not split further.
//   budget  before a level of f nodes, with p passes done so far: if (p + f) c > k the descent stops and every node
//           of that level goes to the ladder.  So passes c <= k always: all the passes together cost no more than the
//           ladder over the whole batch, and the ladder slices, being disjoint, cost no more than that either.  A
//           rejected batch costs at most about twice the whole-batch ladder, whatever the forger does.
//
// At k < c (budget) or 2 <= k <= L (leaf) the root itself goes to the ladder: the behaviour without the descent.
#pragma once
#include <algorithm>
#include <vector>

#include "decider_bisect.hpp"

namespace halo {

// The defaults of the tuning keys schnorr_bisect_pass_items (c) and schnorr_bisect_leaf (L = 2 c: descending a node
// of m items with one wrong item pays c to halve the ladder, which pays off iff m > 2 c).  Measured by
// tools/bench_schnorr_bisect.py (profiles/schnorr_bisect_bench.json): 2^14 is the smallest m from
// which one pass over m items costs no more than the ladder over m items at every larger m measured.  Below it the
// ladder sits on one wave's latency (0.85 ms for 2^10 items as for 2^12) and is not linear in its items, which c
// assumes: c = 1024, where the two floors first cross, let 1023 passes run at k = 2^20, 7.7 x the cost without the
// descent.
constexpr long long SIG_BISECT_PASS_ITEMS_DEFAULT = 16384;
constexpr long long SIG_BISECT_LEAF_DEFAULT = 2 * SIG_BISECT_PASS_ITEMS_DEFAULT;

struct SigBisectRules {
    size_t leaf;        // L >= 1
    size_t pass_items;  // c >= 1
};

// The descent below a failing root [0, k), k >= 1.  ok: k bytes the caller has set to 1 for every live item; a wrong
// single item is cleared here, and `ev` clears its own copy (the device's verdict bytes).  `ev` does the work:
//   int ev.passes(const BisectNode* level, size_t f)
//       D(left) of the f nodes of a level
//   int ev.split(const BisectNode* level, size_t f, uint8_t* flags)
//       the child defects of all f nodes (child 2 s + side of this level is what BisectNode::src names in the next),
//       their 2 f flags (1 = the half fails), and the verdict 0 for a failing half of one item
//   int ev.ladder(uint32_t lo, uint32_t hi)
//       the exact verdicts of the items lo .. hi - 1
// each returning 0 or an error code that ends the descent.
template <class Eval>
int sig_bisect_descend(size_t k, const SigBisectRules& rules, Eval& ev, uint8_t* ok) {
    const size_t L = std::max<size_t>(rules.leaf, 1), c = std::max<size_t>(rules.pass_items, 1);
    if (k == 1) {  // the root's defect is the item's own
        ok[0] = 0;
        return 0;
    }
    if (k <= L) return ev.ladder(0, (uint32_t)k);
    std::vector<BisectNode> level{bisect_node(0, (uint32_t)k, 0)}, next;
    std::vector<uint8_t> flags;
    size_t passes = 0;
    while (!level.empty()) {
        const size_t f = level.size();
        if ((passes + f) * c > k) {  // the budget: the ladder over what is left costs less than going on
            for (const BisectNode& nd : level)
                if (const int rc = ev.ladder(nd.lo, nd.hi)) return rc;
            return 0;
        }
        if (const int rc = ev.passes(level.data(), f)) return rc;
        passes += f;
        flags.assign(2 * f, 0);
        if (const int rc = ev.split(level.data(), f, flags.data())) return rc;
        next.clear();
        for (size_t s = 0; s < f; s++) {
            const BisectNode& nd = level[s];
            const uint32_t lo[2] = {nd.lo, nd.mid}, hi[2] = {nd.mid, nd.hi};
            for (int side = 0; side < 2; side++) {
                if (!flags[2 * s + side]) continue;
                const size_t m = hi[side] - lo[side];
                if (m == 1) {
                    ok[lo[side]] = 0;
                } else if (m <= L) {
                    if (const int rc = ev.ladder(lo[side], hi[side])) return rc;
                } else {
                    next.push_back(bisect_node(lo[side], hi[side], (uint32_t)(2 * s + side)));
                }
            }
        }
        level.swap(next);
    }
    return 0;
}

}  // namespace halo
