// The plain opening of pcdl_open_fs.hip, its transcript on the device, for the units that build on it (acc_fs.hip:
// acc::prover opens h at z).
#pragma once
#include "runtime.hpp"

namespace halo {

// What an opening asserts about its shape before the device is touched: n = d + 1 > 1 a power of two, at most
// SM_ROUNDS_MAX rounds.
int open_fs_check_shape(const char* call, int curve, size_t d);

// The body of halo_pcdl_open_fs_dev_multi: k plain pcdl::open calls of degree bound d over device-resident
// coefficients d_p[i] (lens[i] ark scalars, ordered on the null stream) at z[i] with commitment C[i].  st->mu held,
// the arguments checked; the SRS is checked here.  Waits once per session at the end; every session goes back to the
// pool on every path.
int open_fs_dev_chain(const char* call, DeviceState* st, int curve, size_t k, const void* const* d_p, const size_t* lens,
                      size_t d, const halo_fe_t* z, const halo_wrapped_point_t* C, halo_wrapped_point_t* Ls,
                      halo_wrapped_point_t* Rs, halo_wrapped_point_t* U, halo_fe_t* c, halo_fe_t* v_out);

}  // namespace halo
