// The group plan of the exact batched decider (decider.hip): k instances of n = d + 1 coefficients each are
// decided g at a time, the g coefficient rows of one group living in one buffer.  Host-only and free of HIP
// types, so a plain C++17 compiler builds it (tests/test_decider_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace halo {

// Instances per group.  The rows of a group hold g n scalars, at most `budget` of them (tuning key
// "decide_group_scalars") unless one instance alone exceeds it; the one-MSM batch path sorts g W n entries (W
// windows per scalar) and refuses 2^32 or more, so g W n stays below that as well.  1 <= g <= max(k, 1).
inline size_t decider_group(size_t n, size_t k, size_t budget, int W) {
    n = std::max<size_t>(n, 1);
    const size_t per_instance = n * (size_t)std::max(W, 1);
    size_t g = std::max<size_t>(budget / n, 1);
    g = std::min(g, std::max<size_t>((((uint64_t)1 << 32) - 1) / per_instance, 1));
    return std::min(g, std::max<size_t>(k, 1));
}

// groups that cover k instances, the last one ragged
inline size_t decider_groups(size_t k, size_t g) { return (k + g - 1) / g; }

}  // namespace halo
