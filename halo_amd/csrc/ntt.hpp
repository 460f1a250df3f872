// What ntt.hip offers the other translation units (the polynomial products and trace commitments, poly.hip).
#pragma once
#include "runtime.hpp"

namespace halo {

struct NttPlan;  // ntt_plan.hpp

// plan: the transform's plan (null: ntt_plan under the current tunings, without pruning); a caller that sized
// anything by the plan (the zero-tail prune's read_end) passes the one it used.  d_tmp2: needed by an in-place
// transform with an odd pass count above one (NttPlan::needs_tmp2)
int ntt_device_dispatch(DeviceState* st, int field, const void* d_in, void* d_out, void* d_tmp, unsigned logn,
                        size_t batch, int inverse, hipStream_t s, void* d_tmp2 = nullptr, const NttPlan* plan = nullptr);

}  // namespace halo
