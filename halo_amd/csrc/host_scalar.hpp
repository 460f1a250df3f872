// What the host entry points decide about the scalars of a call before any device work: the one "below the
// scalar modulus" predicate, the check of a decider's weights, and scalar arithmetic on ark Montgomery limbs
// (the host-scalar succinct check of lincomb.hip).  Free of HIP like host_mont.hpp: standard headers, the C ABI
// header (halo_fe_t, the curve ids, the error codes), consts.hpp and host_mont.hpp only, so the host C++ compiler
// builds it alone (tests/host_mont_dump.cpp, tests/test_host_mont.py).
#pragma once
#include "../../include/halo_gpu.h"
#include "consts.hpp"
#include "host_mont.hpp"

namespace halo {

// runtime.cpp's (runtime.hpp); a stand-alone program that calls check_rho supplies its own
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// The scalar field of `curve` (Pallas: Fp, Vesta: Fq) and its base field.
inline const HostMont& scalar_mont(int curve) {
    static const HostMont fp(FpCfg::MODULUS64), fq(FqCfg::MODULUS64);
    return curve == HALO_PALLAS ? fp : fq;
}
inline const HostMont& base_mont(int curve) { return scalar_mont(curve == HALO_PALLAS ? HALO_VESTA : HALO_PALLAS); }

// x, or each of the n values at x (none: true), is below the scalar modulus of `curve` (the constant: no look-up).
inline bool scalar_below(int curve, const halo_fe_t& x) {
    const uint64_t(&p)[4] = curve == HALO_PALLAS ? FpCfg::MODULUS64 : FqCfg::MODULUS64;
    for (int q = 3; q >= 0; q--)
        if (x.l[q] != p[q]) return x.l[q] < p[q];
    return false;
}
inline bool scalar_below(int curve, const halo_fe_t* x, size_t n) {
    for (size_t j = 0; j < n; j++)
        if (!scalar_below(curve, x[j])) return false;
    return true;
}

// A combined decider's weights (null: none) are below the modulus and not zero, which would leave an instance unchecked.
inline int check_rho(const char* call, int curve, const halo_fe_t* rho, size_t k) {
    for (size_t i = 0; rho && i < k; i++) {
        if (!(rho[i].l[0] | rho[i].l[1] | rho[i].l[2] | rho[i].l[3]))
            return set_error(HALO_EINVAL, "%s: rho[%zu] is zero", call, i);
        if (!scalar_below(curve, rho[i])) return set_error(HALO_EINVAL, "%s: rho[%zu] is not below the modulus", call, i);
    }
    return HALO_OK;
}

// Arithmetic of one field on ark Montgomery limbs (the succinct check's h(z) and e).  Inputs below the modulus.
struct HostScalar {
    const HostMont& M;
    static bool is_zero(const uint64_t (&a)[4]) { return !(a[0] | a[1] | a[2] | a[3]); }
    void add(const uint64_t (&a)[4], const uint64_t (&b)[4], uint64_t (&r)[4]) const {  // a + b < 2^256
        unsigned __int128 c = 0;
        uint64_t t[4];
        for (int i = 0; i < 4; i++) {
            c += (unsigned __int128)a[i] + b[i];
            t[i] = (uint64_t)c;
            c >>= 64;
        }
        if (M.geq_p(t)) M.sub_p(t);
        for (int i = 0; i < 4; i++) r[i] = t[i];
    }
    void neg(const uint64_t (&a)[4], uint64_t (&r)[4]) const {
        if (is_zero(a)) {
            for (int i = 0; i < 4; i++) r[i] = 0;
            return;
        }
        unsigned __int128 bw = 0;
        for (int i = 0; i < 4; i++) {
            const unsigned __int128 d = (unsigned __int128)M.p[i] - a[i] - bw;
            r[i] = (uint64_t)d;
            bw = (d >> 64) & 1;
        }
    }
    void sub(const uint64_t (&a)[4], const uint64_t (&b)[4], uint64_t (&r)[4]) const {
        uint64_t nb[4];
        neg(b, nb);
        add(a, nb, r);
    }
};

}  // namespace halo
