// What field_ops.hip offers the hiding open (pcdl_open.hip): the pcdl_* steps on device buffers.
#pragma once
#include "runtime.hpp"

namespace halo {

// The hiding branch of pcdl::open_without_eval on device buffers (field_ops.hip), stream-ordered on s:
// p_bar = (X - z) q (q: d ark coefficients, z: ark scalar) -> d + 1 ark coefficients;
// p' = p (len coefficients, zero-padded to n) + alpha p_bar (p' may alias p), w' = w + alpha w_bar,
// C' = C + alpha C_bar - w' S (C, C_bar, C' WrappedPoints; S internal affine).
int pcdl_pbar_device(int curve, const void* q, size_t d, const void* z, void* p_bar, hipStream_t s);
int pcdl_combine_device(int curve, const void* p, size_t len, const void* p_bar, size_t n, const void* alpha,
                        const void* w, const void* w_bar, const void* C, const void* C_bar, const void* S_int,
                        void* p_prime, void* C_prime, void* w_prime, hipStream_t s);
// p[i] += alpha p_bar[i] and p_bar[i] = alpha p_bar[i] in place (i < n); w' = w + alpha w_bar, negw = -w.
int pcdl_combine_scalars_device(int curve, void* p, void* p_bar, size_t n, const void* alpha, const void* w,
                                const void* w_bar, void* w_prime, void* negw, hipStream_t s);
// xyzz (128 B packed XYZZ) = xyzz (or, from_wrapped, the WrappedPoint first_wrapped) + the WrappedPoint
// at wrapped (one lane).
int xyzz_add_wrapped_device(int curve, void* xyzz, const void* wrapped, hipStream_t s, bool from_wrapped = false,
                            const void* first_wrapped = nullptr);

}  // namespace halo
