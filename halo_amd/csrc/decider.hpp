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

}  // namespace halo
