// What the kernels that run one Poseidon sponge per lane or per three lanes share (schnorr.hip, decide_rho.hip,
// schnorr_combined.hip, pcdl_fs.hip, acc_fs.hip, plonk_verify.hip, sponge.hip, pcdl_open_fs.hip): the lane -> sponge
// map, the one launcher (SPONGE_LAUNCH, over sponge_plan.hpp's lane rule and grid), and the installed parameters:
// the entry points' "they are set" check and the device's copy (defined in schnorr.hip).
#pragma once
#include "dispatch.hpp"
#include "poseidon.hpp"
#include "runtime.hpp"
#include "sponge_plan.hpp"

namespace halo {

// Index of this lane's sponge and whether this lane reports its result.  The grid is whole waves and every lane of a
// wave takes part in the sponge's shuffles, so no lane returns early: a kernel clamps the index of a lane past its
// batch of k to the last sponge, ic = i < k ? i : k - 1 (whose inputs it may read), and stores under writer && i < k.
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

// How a sponge kernel opens: stages the constants into the kernel's `tab` (poseidon::TABLE_WORDS of LDS; a block
// barrier) and maps the lane.  Declares, under the names the kernel gives: i, the lane's sponge; ic, i clamped to the
// batch of k (a lane past the batch works on the last sponge, whose inputs it may read: every lane of a wave takes
// part in the shuffles, so none returns early); writer: the lane stores the sponge's results under writer && i < k,
// a lane past the batch nothing.  A macro, and the store test left to the kernel's end, on measurement: with
// sponge_index one inlining level down (a helper that returns a struct, or one that fills references), or with the
// test behind a function or a lambda, every three-lane kernel compiles to other code and one more VGPR
// (k_poseidon_hash 116 for 115).
// It expands to statements and declarations, not to one statement: use it as a line of its own at kernel scope.
#define SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer) \
    poseidon::stage_params((params), (tab));                  \
    bool writer;                                              \
    const size_t i = sponge_index<LANES>(writer);             \
    const size_t ic = i < (k) ? i : (k)-1

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

// Lanes per sponge for a batch of k on this device (1 or 3; the poseidon_lanes tuning key pins either).
inline int poseidon_lanes(const DeviceState* st, size_t k) { return sponge_lanes(tuning(TUNE_POSEIDON_LANES), k, st->num_cu); }
struct SpongeLaunchPlan {
    int lanes;
    HashGrid grid;
};
inline SpongeLaunchPlan sponge_launch_plan(const DeviceState* st, size_t k) {
    const int lanes = poseidon_lanes(st, k);
    return {lanes, hash_grid(k, lanes)};
}

// The launch of a sponge kernel, an expression of type int (HALO_OK, or the launch's error set).  T and L name the
// dispatched type and the lane count in `kern`, as in DISPATCH_CURVE and DISPATCH_LANES: `Cv, L, (k_rho_leaves<Cv, L>)`;
// `name` is the profile name, null for an untimed launch; the kernel's arguments follow.
//   SPONGE_LAUNCH_AT     the given lanes and grid (pcdl_open_fs.hip's single-wave transcript kernels)
//   SPONGE_LAUNCH        k sponges of `curve`: the lane rule and the grid of sponge_plan.hpp
//   SPONGE_LAUNCH_FIELD  the same for a kernel over a field alone
#define SPONGE_LAUNCH_AT(DISPATCH, id, T, L, plan, name, stream, kern, ...)                                          \
    [&]() -> int {                                                                                                \
        const ::halo::SpongeLaunchPlan p_ = (plan);                                                               \
        ::halo::ProfScope prof_((name), (stream));                                                                \
        DISPATCH(id, T, {                                                                                         \
            DISPATCH_LANES(p_.lanes, L, {                                                                         \
                HALO_LAUNCH(prof_, kern, dim3(p_.grid.blocks), dim3(p_.grid.threads), 0, (stream), __VA_ARGS__);  \
            });                                                                                                   \
        });                                                                                                       \
        HALO_HIP(hipGetLastError());                                                                              \
        return HALO_OK;                                                                                           \
    }()
#define SPONGE_LAUNCH(st, curve, Cv, L, k, name, stream, kern, ...) \
    SPONGE_LAUNCH_AT(DISPATCH_CURVE, curve, Cv, L, ::halo::sponge_launch_plan((st), (k)), name, stream, kern, __VA_ARGS__)
#define SPONGE_LAUNCH_FIELD(st, field, F, L, k, name, stream, kern, ...) \
    SPONGE_LAUNCH_AT(DISPATCH_FIELD, field, F, L, ::halo::sponge_launch_plan((st), (k)), name, stream, kern, __VA_ARGS__)

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

}  // namespace halo
