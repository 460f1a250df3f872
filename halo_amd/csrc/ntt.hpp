// What ntt.hip offers the other translation units (the polynomial products and trace commitments, poly.hip).
#pragma once
#include <vector>

#include "runtime.hpp"

namespace halo {

// rad: the pass split to launch (null: ntt_radices(logn)); a caller that sized anything by the split
// (the zero-tail prune) passes the vector it used
int ntt_device_dispatch(DeviceState* st, int field, const void* d_in, void* d_out, void* d_tmp, unsigned logn,
                        size_t batch, int inverse, hipStream_t s, void* d_tmp2 = nullptr, unsigned prune = 0,
                        const std::vector<unsigned>* rad = nullptr);

}  // namespace halo
