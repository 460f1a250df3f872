// Host field arithmetic for the points and scalars the library hands back to its callers: 4 x 64-bit
// Montgomery arithmetic with a binary-GCD inversion, the packed XYZZ -> ark WrappedPoint conversions
// built on it and the scalar inverse.  Free of HIP: standard headers and consts.hpp only, so the host
// C++ compiler builds it alone (tests/host_mont_dump.cpp, tests/test_host_mont.py).  F is a field
// config of consts.hpp (FpCfg / FqCfg); host_point.cpp maps the curve ids onto them.
#pragma once
#include <algorithm>
#include <cstdint>

#include "consts.hpp"

namespace halo {

// ---------------------------------------------------------------------------------------------
// Host-side XYZZ -> affine (the IPA's per-round L and R, and every entry point that returns one point
// to the host): the lane-side conversion is a ~30 us dependent chain on one lane (fe_inv) at the end
// of the reduction tail; on the host it is a few microseconds.  A packed internal coordinate is an integer < 2p congruent to v 2^261, so
// x = X / ZZ and y = Y / ZZZ need no change of representation; 4 x 64-bit Montgomery arithmetic
// (R = 2^256) then yields x R mod p, which is the ark word form directly.
// ---------------------------------------------------------------------------------------------
struct HostMont {
    uint64_t p[4], pinv, r2[4], one[4], inv_fix[4];
    uint32_t p32[8];
    explicit HostMont(const uint64_t (&m)[4]) {
        for (int i = 0; i < 4; i++) p[i] = m[i];
        uint64_t inv = 1;  // p[0]^-1 mod 2^64 by Newton's iteration
        for (int i = 0; i < 6; i++) inv *= 2 - p[0] * inv;
        pinv = 0 - inv;
        uint64_t x[4] = {1, 0, 0, 0};
        for (int i = 0; i < 512; i++) {  // 2^256 mod p (= one), then 2^512 mod p (= r2)
            dbl(x);
            if (i == 255)
                for (int k = 0; k < 4; k++) one[k] = x[k];
        }
        for (int k = 0; k < 4; k++) r2[k] = x[k];
        for (int k = 0; k < 8; k++) p32[k] = (uint32_t)(p[k >> 1] >> (32 * (k & 1)));
        mul(r2, r2, inv_fix);  // R^3 = 2^768 mod p (inv)
    }
    bool geq_p(const uint64_t (&a)[4]) const {
        for (int i = 3; i >= 0; i--)
            if (a[i] != p[i]) return a[i] > p[i];
        return true;
    }
    void sub_p(uint64_t (&a)[4]) const {
        unsigned __int128 b = 0;
        for (int i = 0; i < 4; i++) {
            const unsigned __int128 d = (unsigned __int128)a[i] - p[i] - b;
            a[i] = (uint64_t)d;
            b = (d >> 64) & 1;
        }
    }
    void dbl(uint64_t (&a)[4]) const {  // a < p (p < 2^255): 2a < 2^256
        uint64_t c = 0;
        for (int i = 0; i < 4; i++) {
            const uint64_t t = (a[i] << 1) | c;
            c = a[i] >> 63;
            a[i] = t;
        }
        if (geq_p(a)) sub_p(a);
    }
    void mul(const uint64_t (&a)[4], const uint64_t (&b)[4], uint64_t (&out)[4]) const {  // a b R^-1 mod p (CIOS)
        uint64_t t[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 4; i++) {
            unsigned __int128 c = 0;
            for (int j = 0; j < 4; j++) {
                c += (unsigned __int128)a[j] * b[i] + t[j];
                t[j] = (uint64_t)c;
                c >>= 64;
            }
            c += t[4];
            t[4] = (uint64_t)c;
            t[5] = (uint64_t)(c >> 64);
            const uint64_t m = t[0] * pinv;
            c = ((unsigned __int128)m * p[0] + t[0]) >> 64;
            for (int j = 1; j < 4; j++) {
                c += (unsigned __int128)m * p[j] + t[j];
                t[j - 1] = (uint64_t)c;
                c >>= 64;
            }
            c += t[4];
            t[3] = (uint64_t)c;
            t[4] = t[5] + (uint64_t)(c >> 64);
        }
        uint64_t r[4] = {t[0], t[1], t[2], t[3]};
        if (t[4] || geq_p(r)) sub_p(r);
        for (int i = 0; i < 4; i++) out[i] = r[i];
    }
    // Montgomery domain (a = x R mod p, a < p): Pornin's optimized binary GCD, the same algorithm as the
    // device's fe_inv (fields.hpp: 17 rounds of 30 steps on 62-bit approximations, each round's 2x2
    // factors applied to a, b and, with a Montgomery division by 2^30, to the coefficients u, v).  It
    // leaves v = a^-1 = x^-1 R^-1 (the invariants a = x u, b = x v mod p survive the rounds' common
    // division by 2^30); one product with inv_fix = R^3 makes it x^-1 R.
    // (Host: about 3x faster than the Fermat chain a^(p-2), 384 products, and 1.7x faster than a
    // plain binary extended Euclid.)
    static int bitlen8(const uint32_t (&a)[8]) {
        for (int i = 7; i >= 0; i--)
            if (a[i]) return 32 * i + 32 - __builtin_clz(a[i]);
        return 0;
    }
    static uint32_t align30(uint32_t hi, uint32_t lo, int s) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> s); }
    static uint64_t approx(const uint32_t (&a)[8], int n) {  // (a mod 2^30) + 2^30 floor(a / 2^(n - 32))
        const int s = n - 32, i = s >> 5;
        const uint32_t lo = a[i], hi = i + 1 < 8 ? a[i + 1] : 0u;
        return (uint64_t)(a[0] & 0x3fffffffu) | ((uint64_t)align30(hi, lo, s & 31) << 30);
    }
    static bool lin(const uint32_t (&a)[8], const uint32_t (&b)[8], int64_t f, int64_t g, uint32_t (&r)[8]) {
        uint32_t t[8];
        int64_t c = 0;
        for (int i = 0; i < 8; i++) {  // |a f + b g| / 2^30, exact; returns the sign
            const int64_t x = (int64_t)a[i] * f + (int64_t)b[i] * g + c;
            t[i] = (uint32_t)x;
            c = x >> 32;
        }
        const bool neg = c < 0;
        uint64_t br = 1;
        for (int i = 0; i < 8; i++) {
            const uint32_t sh = align30(i < 7 ? t[i + 1] : (uint32_t)c, t[i], 30);
            const uint64_t ng = (uint64_t)(~sh) + br;
            br = ng >> 32;
            r[i] = neg ? (uint32_t)ng : sh;
        }
        return neg;
    }
    void lin_mod(const uint32_t (&u)[8], const uint32_t (&v)[8], int64_t f, int64_t g, uint32_t (&r)[8]) const {
        uint32_t t[8];
        int64_t c = 0;
        for (int i = 0; i < 8; i++) {  // (u f + v g) / 2^30 mod p (p = 1 mod 2^32)
            const int64_t x = (int64_t)u[i] * f + (int64_t)v[i] * g + c;
            t[i] = (uint32_t)x;
            c = x >> 32;
        }
        const uint32_t q = (0u - t[0]) & 0x3fffffffu;
        int64_t c2 = 0;
        for (int i = 0; i < 8; i++) {
            const int64_t x = (int64_t)t[i] + (int64_t)((uint64_t)q * p32[i]) + c2;
            t[i] = (uint32_t)x;
            c2 = x >> 32;
        }
        const int64_t top = c + c2;
        uint32_t s[8];
        for (int i = 0; i < 8; i++) s[i] = align30(i < 7 ? t[i + 1] : (uint32_t)top, t[i], 30);
        int32_t hi = (int32_t)(top >> 30);
        for (int k = 0; k < 2 && hi < 0; k++) {
            uint64_t cy = 0;
            for (int i = 0; i < 8; i++) {
                const uint64_t x = (uint64_t)s[i] + p32[i] + cy;
                s[i] = (uint32_t)x;
                cy = x >> 32;
            }
            hi += (int32_t)cy;
        }
        uint64_t bw = 0;
        uint32_t w[8];
        for (int i = 0; i < 8; i++) {
            const uint64_t x = (uint64_t)s[i] - p32[i] - bw;
            w[i] = (uint32_t)x;
            bw = (x >> 32) & 1u;
        }
        for (int i = 0; i < 8; i++) r[i] = bw == 0 ? w[i] : s[i];
    }
    void inv(const uint64_t (&x)[4], uint64_t (&out)[4]) const {
        uint32_t a[8], b[8], u[8], v[8];
        for (int i = 0; i < 8; i++) {
            a[i] = (uint32_t)(x[i >> 1] >> (32 * (i & 1)));
            b[i] = p32[i];
            u[i] = i == 0 ? 1u : 0u;
            v[i] = 0u;
        }
        for (int it = 0; it < 17; it++) {  // ceil((2 * 255 - 1) / 30) rounds: b = gcd = 1
            const int n = std::max(std::max(bitlen8(a), bitlen8(b)), 62);
            uint64_t ab = approx(a, n), bb = approx(b, n);
            int32_t f0 = 1, g0 = 0, f1 = 0, g1 = 1;
            for (int j = 0; j < 30; j++) {
                const bool odd = ab & 1u;
                const bool sw = odd && ab < bb;
                const uint64_t ta = sw ? bb : ab, tb = sw ? ab : bb;
                const int32_t tf0 = sw ? f1 : f0, tg0 = sw ? g1 : g0, tf1 = sw ? f0 : f1, tg1 = sw ? g0 : g1;
                ab = (odd ? ta - tb : ta) >> 1;
                bb = tb;
                f0 = odd ? tf0 - tf1 : tf0;
                g0 = odd ? tg0 - tg1 : tg0;
                f1 = tf1 * 2;
                g1 = tg1 * 2;
            }
            uint32_t na[8], nb[8], nu[8], nv[8];
            if (lin(a, b, f0, g0, na)) {
                f0 = -f0;
                g0 = -g0;
            }
            if (lin(a, b, f1, g1, nb)) {
                f1 = -f1;
                g1 = -g1;
            }
            lin_mod(u, v, f0, g0, nu);
            lin_mod(u, v, f1, g1, nv);
            for (int i = 0; i < 8; i++) {
                a[i] = na[i];
                b[i] = nb[i];
                u[i] = nu[i];
                v[i] = nv[i];
            }
        }
        uint64_t r[4];
        for (int i = 0; i < 4; i++) r[i] = (uint64_t)v[2 * i] | ((uint64_t)v[2 * i + 1] << 32);
        mul(r, inv_fix, out);
    }
};

template <class F>
void host_xyzz_to_wrapped_t(const void* xyzz, void* wrapped) {
    static const HostMont M(F::MODULUS64);
    const uint64_t* q = (const uint64_t*)xyzz;
    uint64_t c[4][4];  // X, Y, ZZ, ZZZ reduced below p
    for (int k = 0; k < 4; k++) {
        for (int i = 0; i < 4; i++) c[k][i] = q[4 * k + i];
        if (M.geq_p(c[k])) M.sub_p(c[k]);
    }
    uint64_t* out = (uint64_t*)wrapped;
    if (!(c[2][0] | c[2][1] | c[2][2] | c[2][3])) {  // ZZ = 0: the identity, WrappedPoint (0, 0)
        for (int i = 0; i < 8; i++) out[i] = 0;
        return;
    }
    uint64_t m[4][4], t[4], iv[4], u[4], x[4], y[4];
    for (int k = 0; k < 4; k++) M.mul(c[k], M.r2, m[k]);  // to the Montgomery domain
    M.mul(m[2], m[3], t);
    M.inv(t, iv);  // (ZZ ZZZ)^-1
    M.mul(m[0], m[3], u);
    M.mul(u, iv, x);  // X / ZZ, times R
    M.mul(m[1], m[2], u);
    M.mul(u, iv, y);  // Y / ZZZ, times R
    for (int i = 0; i < 4; i++) {
        out[i] = x[i];
        out[4 + i] = y[i];
    }
}
// k points with one inversion (Montgomery's trick over the ZZ ZZZ products; k <= 16)
template <class F>
void host_xyzz_to_wrapped2_t(const void* const* xyzz, void* const* wrapped, int k) {
    static const HostMont M(F::MODULUS64);
    uint64_t m[16][4][4], t[16][4], pre[17][4];
    bool id[16];
    for (int j = 0; j < 4; j++) pre[0][j] = M.one[j];
    for (int i = 0; i < k; i++) {
        const uint64_t* q = (const uint64_t*)xyzz[i];
        uint64_t c[4][4];
        for (int a = 0; a < 4; a++) {
            for (int j = 0; j < 4; j++) c[a][j] = q[4 * a + j];
            if (M.geq_p(c[a])) M.sub_p(c[a]);
        }
        id[i] = !(c[2][0] | c[2][1] | c[2][2] | c[2][3]);
        for (int a = 0; a < 4; a++) M.mul(c[a], M.r2, m[i][a]);
        if (id[i])
            for (int j = 0; j < 4; j++) t[i][j] = M.one[j];
        else
            M.mul(m[i][2], m[i][3], t[i]);
        M.mul(pre[i], t[i], pre[i + 1]);
    }
    uint64_t inv[4];
    M.inv(pre[k], inv);  // (prod_i ZZ_i ZZZ_i)^-1
    for (int i = k - 1; i >= 0; i--) {
        uint64_t iv[4], u[4], x[4], y[4];
        M.mul(inv, pre[i], iv);  // (ZZ_i ZZZ_i)^-1
        M.mul(inv, t[i], inv);
        uint64_t* out = (uint64_t*)wrapped[i];
        if (id[i]) {
            for (int j = 0; j < 8; j++) out[j] = 0;
            continue;
        }
        M.mul(m[i][0], m[i][3], u);
        M.mul(u, iv, x);
        M.mul(m[i][1], m[i][2], u);
        M.mul(u, iv, y);
        for (int j = 0; j < 4; j++) {
            out[j] = x[j];
            out[4 + j] = y[j];
        }
    }
}

template <class S>
bool host_scalar_inverse_t(const void* x_ark, void* out_ark) {
    static const HostMont M(S::MODULUS64);
    uint64_t x[4];
    for (int i = 0; i < 4; i++) x[i] = ((const uint64_t*)x_ark)[i];
    if (M.geq_p(x)) M.sub_p(x);
    if (!(x[0] | x[1] | x[2] | x[3])) return false;
    uint64_t r[4];
    M.inv(x, r);  // Montgomery-domain inverse: (x R)^-1 R^2 = x^-1 R, the ark form of x^-1
    for (int i = 0; i < 4; i++) ((uint64_t*)out_ark)[i] = r[i];
    return true;
}

}  // namespace halo
