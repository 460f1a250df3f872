// The batched linear combination of lincomb.hip for the other units that build on it (pcdl_fs.hip).
#pragma once
#include "fields.hpp"
#include "runtime.hpp"

namespace halo {

// The ark limbs at p are below the modulus of S.
template <class S>
HALO_DEV bool ark_is_canonical(const uint4* p) {
    const uint4 lo = p[0], hi = p[1];
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    bool below = false, decided = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const uint32_t m = (uint32_t)(S::MODULUS64[i >> 1] >> (32 * (i & 1)));
        if (!decided && w[i] != m) {
            below = w[i] < m;
            decided = true;
        }
    }
    return below;
}

constexpr size_t LINCOMB_MAX_ITEMS = 0x7fffffffu;  // one block per item

// out_i = A_i + sum_{j < t} s_ij P_ij for k >= 1 items over device pointers, asynchronous on `s`: d_add k
// WrappedPoints or null, d_pts / d_scalars k t WrappedPoints / ark scalars, d_out k packed XYZZ sums, d_is_id
// (may be null) k bytes, 1 where the item is valid and its sum is the identity.  The caller holds st->mu and
// a ScratchUse of `s` (st->lincomb_terms is shared by the calls on every stream).
int lincomb_device(DeviceState* st, int curve, const void* d_add, const void* d_pts, const void* d_scalars, size_t k,
                   size_t t, void* d_out, void* d_is_id, hipStream_t s);

}  // namespace halo
