// What the kernels that run one Poseidon sponge per lane or per three lanes share (schnorr.hip, pcdl_fs.hip,
// plonk_verify.hip, pcdl_open_fs.hip): the lane -> sponge map, the launch grid, the lane layout rule and its
// dispatch (DISPATCH_LANES), and the installed parameters: the entry points' "they are set" check and the
// device's copy (defined in schnorr.hip).
#pragma once
#include "poseidon.hpp"
#include "runtime.hpp"

namespace halo {

// Index of this lane's sponge and whether this lane reports its result.
template <int LANES>
HALO_DEV size_t sponge_index(bool& writer) {
    if (LANES == 1) {
        writer = true;
        return (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    }
    const size_t wave = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned lane = threadIdx.x & 63u;
    writer = lane % 3u == 0 && lane != 63u;
    return wave * poseidon::SPONGES_PER_WAVE_3 + (lane == 63u ? 20u : lane / 3u);
}

struct HashGrid {
    unsigned blocks, threads;
};
inline HashGrid hash_grid(size_t k, int lanes) {
    const size_t waves = lanes == 1 ? (k + 63) / 64 : (k + poseidon::SPONGES_PER_WAVE_3 - 1) / poseidon::SPONGES_PER_WAVE_3;
    const unsigned wpb = waves > 4096 ? 4 : 1;  // small batches spread one wave per block over the CUs
    return {(unsigned)((waves + wpb - 1) / wpb), 64 * wpb};
}

// The runtime lane count -> the LANES template argument, in the idiom of DISPATCH_CURVE: the body is written
// once, with L a constexpr int of 1 or 3.
#define DISPATCH_LANES(lanes, L, ...) \
    do {                              \
        if ((lanes) == 1) {           \
            constexpr int L = 1;      \
            __VA_ARGS__;              \
        } else {                      \
            constexpr int L = 3;      \
            __VA_ARGS__;              \
        }                             \
    } while (0)

inline int base_field(int curve) { return curve == HALO_PALLAS ? HALO_FQ : HALO_FP; }
// halo_poseidon_set_params has installed parameters for `field`
bool poseidon_params_set(int field);
// ... for the base field of `curve`, or the error of the entry point `call`
inline int require_poseidon_params(const char* call, int curve) {
    if (!poseidon_params_set(base_field(curve)))
        return set_error(HALO_EINVAL, "%s: no Poseidon parameters for the curve's base field (halo_poseidon_set_params)",
                         call);
    return HALO_OK;
}
// This device's copy of the parameters of `field` (st->mu held).
int poseidon_device_params(DeviceState* st, int field, const uint32_t** out);
// Lanes per sponge for a batch of k (1 or 3; the poseidon_lanes tuning key pins either).
int poseidon_lanes(const DeviceState* st, size_t k);

}  // namespace halo
