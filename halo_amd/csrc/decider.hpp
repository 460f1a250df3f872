// The device-level batched decider of decider.hip for the units that build on it.
#pragma once
#include "runtime.hpp"

namespace halo {

struct DecideCall {  // k instances of one degree bound d, all device pointers
    int curve;
    size_t d, k;
    const void *xis, *U;  // k rows of lg n + 1 ark scalars (fs_device's layout); k WrappedPoints
    const void* live;     // k bytes or null: 0 = skip the instance, verdict 0
    const void* rho;      // k ark scalars: combined mode; null: exact mode
    void* ok;             // k bytes
    void* combined;       // 1 byte, written only with rho; may be null
};

// The launches of one call, all on `s`, no host wait: st->mu and a ScratchUse of `s` held, a.k >= 1, d + 1 a power
// of two.  Checks the resident SRS.  Works in st->decider[0..2] and, in combined mode, st->lincomb_terms.
int decide_device(DeviceState* st, const DecideCall& a, hipStream_t s);

// Per-instance verdicts of a weighted batch by bisection (a.rho given; without it, or for a.k = 1, decide_device's
// exact mode): the combined pass over all of it, and when that rejects, a descent through the halves that fail,
// one MSM per failing internal node (decider_bisect.hpp).  Unlike decide_device it waits for `s`: once after the
// root pass and once per level, at most 1 + ceil(lg k) times.  An instance whose U is neither (0, 0) nor on the
// curve, or whose rho is zero or not below the modulus, is rejected before the root pass and weighs nothing.
// a.combined, when given, receives the root pass's byte.  Works in st->decider[0..2], st->lincomb_terms and
// st->bisect[0..2].
int decide_bisect_device(DeviceState* st, const DecideCall& a, hipStream_t s);

// What the host forms run (halo_pcdl_decide_batch, halo_pcdl_check_fs_batch, halo_plonk_verify_batch): decide_device,
// and for a weighted batch of two or more that the combined pass rejects, the per-instance verdicts: by the exact
// rerun, or with tuning key decide_bisect = 1 by decide_bisect_device.  Waits for `s` where it has to decide.
int decide_resolved(DeviceState* st, const DecideCall& a, hipStream_t s);

}  // namespace halo
