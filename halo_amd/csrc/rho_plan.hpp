// The shape of the derived decider weights (decide_rho.hip): the hash tree over the k leaves, the
// length of a leaf's transcript and the launches of one derivation.  Host-only and free of HIP types, so a plain
// C++17 compiler builds it (tests/rho_plan_dump.cpp, tests/test_rho_plan.py); the one function the kernel shares
// with the host is HALO_HD.
#pragma once
#include <cstddef>
#include <cstdint>

#ifndef HALO_HD
#if defined(__HIPCC__)
#define HALO_HD __host__ __device__ inline
#else
#define HALO_HD inline
#endif
#endif

namespace halo {

// The protocol labels of the three sponges.  They continue Protocols::{PCDL, ASDL, PLONK, SIGNATURE} = 0..3 of
// the reference (outer_sponge.rs:17-22) and are this backend's own: the reference has no batched decider.
constexpr int RHO_BATCH_LEAF = 4, RHO_BATCH_SEED = 5, RHO_BATCH_WEIGHT = 6;
// ... and of the weights of a combined Schnorr batch (schnorr_combined.hip), which share the tree above the leaves.
// This backend's own as well: the reference has no batched signature verification.
constexpr int SIG_BATCH_LEAF = 7, SIG_BATCH_SEED = 8, SIG_BATCH_WEIGHT = 9;

// Elements of level l + 1 of the tree from those of level l: pairs are hashed, an element left alone is promoted.
inline size_t rho_next_level(size_t count) { return (count + 1) / 2; }

// Levels above the leaves until one element remains: ceil(lg k), one k_rho_level launch each (0 for k <= 1).
inline unsigned rho_levels(size_t k) {
    unsigned l = 0;
    for (size_t c = k; c > 1; c = rho_next_level(c)) l++;
    return l;
}

// Base-field elements of a live leaf's transcript: the label, U's two coordinates, and xi_1 .. xi_lg as one
// element each where the scalar field is the smaller one (Vesta), else as two (x >> 1, x & 1).
inline size_t rho_leaf_elements(bool scalar_below_base, unsigned lg) { return 3 + (scalar_below_base ? 1 : 2) * (size_t)lg; }

// Permutations of that transcript up to and including its one squeeze (rate 2).
inline size_t rho_leaf_permutations(bool scalar_below_base, unsigned lg) { return (rho_leaf_elements(scalar_below_base, lg) + 1) / 2; }

// Kernel launches of one derivation: the leaves, the levels, the weights (which recompute the seed per sponge).
inline unsigned rho_launches(size_t k) { return k ? 2 + rho_levels(k) : 0; }

// A weight of zero would leave a live instance unchecked: it becomes one (w: the canonical integer's words).
HALO_HD void rho_zero_becomes_one(uint32_t (&w)[8]) {
    uint32_t any = 0;
    for (int q = 0; q < 8; q++) any |= w[q];
    if (!any) w[0] = 1;
}

}  // namespace halo
