// The device-level pieces of fixed_base.hip: scalar multiples of the generator G = (-1, 2) over a precomputed
// comb table (fixed_base_plan.hpp), for any unit that multiplies G by a batch of scalars.
#pragma once
#include "runtime.hpp"

namespace halo {

// This device's table of `curve` (FB_ENTRIES internal affine points, d 2^(C w) G at fb_table_index).  st->mu held;
// the first call per device and curve builds the table on the device and waits for it, later calls read it
// from any stream.
int fixed_base_table(DeviceState* st, int curve, const void** d_tab);

// out_a[i] = a[i] G for i < k and, when d_b is not null, out_b[i] = b[i] G, as ONE launch on `s` (the two halves
// of a signature: R = nonce G and pk = sk G).  Scalars of `curve` (ark), outputs WrappedPoints, all on the device;
// the zero scalar gives (0, 0).  st->mu held.
int generator_mul_device(DeviceState* st, int curve, const void* d_a, void* d_out_a, const void* d_b, void* d_out_b,
                         size_t k, hipStream_t s);

}  // namespace halo
