// The host point / scalar conversions of points.hpp by curve id, over host_mont.hpp: Pallas has the
// base field Fq and the scalar field Fp, Vesta the other way round (curve.hpp).
#include "host_mont.hpp"
#include "points.hpp"

namespace halo {

void host_xyzz_to_wrapped2(int curve, const void* const* xyzz, void* const* wrapped, int k) {
    if (curve == HALO_PALLAS)
        host_xyzz_to_wrapped2_t<FqCfg>(xyzz, wrapped, k);
    else
        host_xyzz_to_wrapped2_t<FpCfg>(xyzz, wrapped, k);
}

bool host_scalar_inverse(int curve, const void* x_ark, void* out_ark) {
    return curve == HALO_PALLAS ? host_scalar_inverse_t<FpCfg>(x_ark, out_ark)
                                : host_scalar_inverse_t<FqCfg>(x_ark, out_ark);
}

void host_xyzz_to_wrapped(int curve, const void* xyzz, void* wrapped) {
    if (curve == HALO_PALLAS)
        host_xyzz_to_wrapped_t<FqCfg>(xyzz, wrapped);
    else
        host_xyzz_to_wrapped_t<FpCfg>(xyzz, wrapped);
}

}  // namespace halo
