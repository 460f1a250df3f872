// What poly.hip offers the IPA sessions (ipa.hip, pcdl_open.hip): field-only work on device buffers.
#pragma once
#include "runtime.hpp"

namespace halo {

// dot product of two device ark vectors -> device ark scalar (out_ark), using tmp (>= 2048*32 B)
int dot_device(int field, const void* x, const void* y, size_t n, void* out_ark, void* tmp, hipStream_t s);
// out[i] = z^i, i < n (device ark scalar z_ark, ark out), stream-ordered on s
int powers_device(int field, const void* z_ark, size_t n, void* out, hipStream_t s);

}  // namespace halo
