// The device-level batched decider of decider.hip for the units that build on it.
#pragma once
#include "runtime.hpp"

namespace halo {

struct DecideCall {  // k instances of one degree bound d, all device pointers
    int curve;
    size_t d, k;
    const void *xis, *U;  // k rows of lg n + 1 ark scalars (fs_device's layout); k WrappedPoints
    const void* live;     // k bytes or null: 0 = skip the instance, verdict 0
    const void* rho;      // k ark scalars: combined mode; null: exact mode, or with `derive` the derived weights
    void* ok;             // k bytes
    void* combined;       // 1 byte, written only with rho; may be null
    // rho null and k >= 2: combined mode with the weights of decide_rho.hip.  The entry point resolves it, once, from
    // tuning key decide_rho_fs (decide_derives); nothing below reads the key.
    bool derive = false;
};

// What a null rho means to this call: tuning key decide_rho_fs, read here and nowhere else.
inline bool decide_derives(const void* rho) { return !rho && tuning(TUNE_DECIDE_RHO_FS) > 0; }

// A stage that is more than one kernel (an MSM, the derivation of the weights): its halo_profile_read time is the
// span on `s` between begin and end, its launch count the number of stages.
struct StageScope {
    ProfScope p;
    StageScope(const char* name, hipStream_t s) : p(name, s) {
        if (p.slot >= 0) (void)hipEventRecord(p.a, s);
    }
    void end() {
        if (p.slot >= 0) (void)hipEventRecord(p.b, p.s);
    }
};

// The launches of one call, all on `s`, no host wait: st->mu and a ScratchUse of `s` held, a.k >= 1, d + 1 a power
// of two.  Checks the resident SRS.  Works in st->decider[0..2] and, in combined mode, st->lincomb_terms; with
// a.derive also in st->decide_rho.
int decide_device(DeviceState* st, const DecideCall& a, hipStream_t s);

// Per-instance verdicts of a weighted batch by bisection (a.rho given or derived; without it, or for a.k = 1,
// decide_device's exact mode): the combined pass over all of it, and when that rejects, a descent through the halves
// that fail, one MSM per failing internal node (decider_bisect.hpp).  Unlike decide_device it waits for `s`: once after the
// root pass and once per level, at most 1 + ceil(lg k) times.  An instance whose U is neither (0, 0) nor on the
// curve, or whose rho is zero or not below the modulus, is rejected before the root pass and weighs nothing.
// a.combined, when given, receives the root pass's byte.  Works in st->decider[0..2], st->lincomb_terms and
// st->bisect[0..2].
int decide_bisect_device(DeviceState* st, const DecideCall& a, hipStream_t s);

// What the host forms run (halo_pcdl_decide_batch, halo_pcdl_check_fs_batch, halo_plonk_verify_batch): decide_device,
// and for a weighted batch of two or more that the combined pass rejects, the per-instance verdicts: by the exact
// rerun, or with tuning key decide_bisect = 1 by decide_bisect_device.  Waits for `s` where it has to decide.
int decide_resolved(DeviceState* st, const DecideCall& a, hipStream_t s);

// decide_rho.hip.  The weights of k >= 1 instances (DESIGN §4.9 "derived weights") as k ark scalars at d_rho_out:
// 2 + ceil(lg k) launches on `s`, no host wait.  st->mu and a ScratchUse of `s` held, the Poseidon parameters of
// the curve's base field installed, d + 1 a power of two.  Works in st->decide_rho[1].
int decide_rho_device(DeviceState* st, int curve, size_t d, size_t k, const void* xis, const void* U, const void* live,
                      void* rho_out, hipStream_t s);
// What tells one derivation's weights kernel from another's: the labels of the seed and weight sponges, the third
// integer the seed absorbs after the root and k, and the profile name of the launch.
struct RhoWeights {
    int seed_label, weight_label;
    size_t third;
    const char* profile;
};
// The two buffers of a derivation over k >= 1 leaves, carved from `work`: buf[0] of k packed base-field elements
// (the leaves), buf[1] of rho_next_level(k).
int rho_buffers(DevBuf& work, size_t k, uint4* (&buf)[2]);
// From the leaves in buf[0] to the weights: the hash tree (k_rho_level, ceil(lg k) launches between the two
// buffers) and k_rho_weights over its root, k ark scalars at rho_out (0 where `live`, which may be null, has 0).
// Shared with the weights of a combined Schnorr batch (schnorr_combined.hip).  params: the device's Poseidon
// parameters of the curve's base field.
int rho_derive_device(DeviceState* st, int curve, const uint32_t* params, uint4* const (&buf)[2], size_t k, const RhoWeights& w,
                      const void* live, void* rho_out, hipStream_t s);
// a.derive, no rho and k >= 2: derives the weights into st->decide_rho[0] and makes them a.rho.  Else nothing.
int decide_rho_weights(DeviceState* st, DecideCall& a, hipStream_t s);

}  // namespace halo
