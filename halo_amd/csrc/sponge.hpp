// The Fiat-Shamir sponge as an object (sponge.hip; crates/poseidon/src/outer_sponge.rs:11-100, Sponge<P>): a handle
// owns k sponges that advance in lockstep, their states in device memory between calls in Sponge::store's format.
#pragma once
#include "runtime.hpp"
#include "sponge_plan.hpp"

namespace halo {

// How a launch of k_sponge_absorb comes by its state.
enum SpongeInit {
    SPONGE_LOAD = 0,   // the stored state
    SPONGE_FRESH = 1,  // Sponge::new: zero, Absorbed(0), then label_element(protocol) absorbed
    SPONGE_RESET = 2   // Sponge::reset (outer_sponge.rs:97-99): zero, Absorbed(0), no label
};

struct SpongeHandle {
    DeviceState* st;
    int curve;
    int protocol;
    size_t k;
    DevBuf state;     // k x poseidon::STATE_U4 uint4
    SpongeMode mode;  // the mirror of every stored (squeezed, n): the k sponges share it
};

// Enqueue on `s`: absorb row i of d_in ((k, n) items of `kind`, row-major; ark Montgomery words) into sponge i, after
// `init`.  Updates the mirror and the profile's permutation count.  st->mu held.
int sponge_absorb_launch(SpongeHandle& h, int init, int kind, const void* d_in, size_t n, hipStream_t s);
// Enqueue on `s`: n challenges of every sponge to d_out ((k, n) ark scalars).  st->mu held.
int sponge_challenge_launch(SpongeHandle& h, size_t n, void* d_out, hipStream_t s);

}  // namespace halo
