// Point utilities shared by the MSM, the SRS and the IPA: the wrapped <-> internal conversions
// (points.hip) and the host conversions of packed XYZZ points and scalars (host_point.cpp over
// host_mont.hpp).
#pragma once
#include "runtime.hpp"

namespace halo {

// HALO_EINVAL (with the error set) unless c is HALO_PALLAS or HALO_VESTA
int check_curve(halo_curve_t c);
// HALO_EINVAL (with the error set) unless f is HALO_FP or HALO_FQ
int check_field(halo_field_t f);

// Host conversion of a 128-B packed XYZZ point (internal format, each coordinate < 2p) to an ark
// WrappedPoint: one inversion in 4 x 64-bit Montgomery arithmetic on the CPU (identity -> (0, 0)).
void host_xyzz_to_wrapped(int curve, const void* xyzz, void* wrapped);
// x^-1 of an ark (Montgomery) scalar of the curve's scalar field, on the host (binary extended Euclid);
// false for x = 0
bool host_scalar_inverse(int curve, const void* x_ark, void* out_ark);
// k <= 16 points at once with one inversion (Montgomery's trick)
void host_xyzz_to_wrapped2(int curve, const void* const* xyzz, void* const* wrapped, int k);
int convert_wrapped_to_internal(int curve, const void* in, void* out, size_t n, hipStream_t s);
int convert_internal_to_wrapped(int curve, const void* in, void* out, size_t n, hipStream_t s);
// count packed XYZZ points (128 B each) -> internal affine (64 B each), one lane per point
int xyzz_to_affine_device(int curve, const void* xyzz, void* aff, int count, hipStream_t s);
// Host-output entry points: the MSM leaves its sum as 128-B packed XYZZ on the device, and the affine
// conversion (one inversion) runs on the host after the copy -- not as a one-lane chain at the end
// of the reduction tail.
int d2h_point(int curve, const void* d_xyzz, halo_wrapped_point_t* out, hipStream_t s);

}  // namespace halo
