// Batched linear combinations of points, out_i = A_i + sum_{j < t} s_ij P_ij, and on top of them the
// PCDL verifier's succinct check (crates/accumulation/src/pcdl.rs:483-554): per instance 2 lg n + 2
// variable-base scalar multiplications by full-width challenges, one sum and one comparison with the
// identity.  Every challenge of the verifier depends on the proof's own points only, so the caller's
// transcript derives all of them before any device work and a batch of instances is one launch pair.
//
//   k_lincomb_terms   one aligned quad of lanes per term s P: the GLV split s = k1 + lambda k2, both halves
//                     as 33 signed 4-bit digits, the quad's table d P (1 <= d <= 8) in LDS, 33 windows of
//                     four quad doublings and two table additions (phi applied as an entry is read)
//   k_lincomb_sum     one wave per item: its t terms and the optional affine addend, summed with the
//                     complete addition (equal and opposite partial sums, identity terms)
// The host-scalar succinct check computes h(z) and e with HostScalar (host_scalar.hpp).
#include "curve.hpp"
#include "dispatch.hpp"
#include "glv.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "points.hpp"
#include "quad_ladder.hpp"
#include "runtime.hpp"
#include "tree.hpp"

#include <vector>

namespace halo {

constexpr int LINCOMB_THREADS = 64;  // one wave: 16 terms
constexpr int LINCOMB_TAB_U4 = QUAD_TAB_U4;  // d P at d - 1 (1 <= d <= 8) per quad: XYZZ, 128 B each; 16 KB per block
// Waves per SIMD the term kernel is compiled for: at 206 VGPRs it spills nothing; compiled for three it
// spills 116 VGPRs and the 16 KB tables admit only 2.5, and it measured 16 % slower.
constexpr int LINCOMB_TERM_WAVES = 2;

// Term i = s_i P_i as packed XYZZ, ok[i] = 1; a P_i that is neither (0, 0) nor on the curve, or an s_i
// that is not below the modulus, gives the identity and ok[i] = 0.  One aligned quad of lanes per term,
// every lane of the quad holding the same values (tree.hpp's quad doubling / addition); quads of one
// wave stay in lockstep: an addition is skipped only when it is trivial for every quad.
template <class Cv>
__global__ __launch_bounds__(LINCOMB_THREADS, LINCOMB_TERM_WAVES) void k_lincomb_terms(const uint4* __restrict__ pts,
                                                                   const uint4* __restrict__ scalars, size_t n,
                                                                   uint4* __restrict__ terms, uint8_t* __restrict__ ok) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint4 lds[(LINCOMB_THREADS / 4) * LINCOMB_TAB_U4];
    uint4* pt = lds + LINCOMB_TAB_U4 * (threadIdx.x >> 2);
    const uint32_t lane = threadIdx.x & 63u, role = lane & 3u, s1 = lane & ~3u;
    const size_t i = ((size_t)blockIdx.x * LINCOMB_THREADS + threadIdx.x) >> 2;
    const size_t ic = i < n ? i : n - 1;  // quads past the batch repeat its last term (no store): every lane reaches the barriers
    Affine<F> P = aff_from_wrapped<F>(pts + 4 * ic);
    const bool valid = aff_on_curve_or_id(P, fe_from_const<F>(Cv::K::B)) && ark_is_canonical<S>(scalars + 2 * ic);
    if (!valid) P.x = P.y = fe_zero<F>();  // the ladder then runs over the identity
    bool n1, n2;
    SignedDigits g1, g2;
    {
        uint32_t sw[8], k1[5], k2[5];
        fe_ark_to_canonical_words<S>(scalars + 2 * ic, sw);
        glv::decompose<typename Cv::K>(sw, n1, k1, n2, k2);
        g1.recode(k1);
        g2.recode(k2);
    }
    QUAD_TABLE_BUILD(F, pt, P, role, s1);
    const Fe<F> beta = fe_from_const<F>(Cv::K::BETA);
    XYZZ<F> acc = xyzz_id<F>();
#pragma unroll 1
    for (int w = 32; w >= 0; w--) {  // 33 windows cover 132 bits
        if (w != 32)
            for (int q = 0; q < 4; q++) acc = xyzz_dbl_quad(acc);
        bool neg;
        uint32_t d = g1.next(neg);  // + k1 P
        XYZZ<F> t = xyzz_load<F>(pt + 8 * (d ? d - 1 : 0));
        if (n1 != neg) t.Y = fe_neg(t.Y);
        acc = quad_add(acc, t, d == 0, role, s1);
        d = g2.next(neg);  // + k2 phi(P)
        t = xyzz_load<F>(pt + 8 * (d ? d - 1 : 0));
        t.X = fe_mul(t.X, beta);
        if (n2 != neg) t.Y = fe_neg(t.Y);
        acc = quad_add(acc, t, d == 0, role, s1);
    }
    if (role == 0 && i < n) {
        xyzz_store(terms + 8 * i, acc);
        ok[i] = valid ? 1 : 0;
    }
}

// Item b = blockIdx.x: A_b (when add is given) plus its t terms, the row form of k_point_sum_xyzz
// (points.hip): every lane adds a strided share with the complete addition, then an LDS tree.  An
// invalid term, or an addend that is neither (0, 0) nor on the curve, makes the item invalid: the
// identity, and is_id[b] = 0.  Otherwise is_id[b] tells whether the sum is the identity.
template <class Cv>
__global__ __launch_bounds__(LINCOMB_THREADS) void k_lincomb_sum(const uint4* __restrict__ add,
                                                                 const uint4* __restrict__ terms,
                                                                 const uint8_t* __restrict__ ok, size_t t,
                                                                 uint4* __restrict__ out, uint8_t* __restrict__ is_id) {
    using F = typename Cv::Base;
    __shared__ uint4 red[LINCOMB_THREADS * 8];
    const size_t b = blockIdx.x;
    terms += 8 * t * b;
    ok += t * b;
    bool valid = true;
    XYZZ<F> acc = xyzz_id<F>();
    if (add && threadIdx.x == 0) {
        const Affine<F> A = aff_from_wrapped<F>(add + 4 * b);
        valid = aff_on_curve_or_id(A, fe_from_const<F>(Cv::K::B));
        if (valid) acc = xyzz_from_aff(A);
    }
    for (size_t j = threadIdx.x; j < t; j += LINCOMB_THREADS) {
        valid = valid && ok[j] != 0;
        acc = xyzz_add(acc, xyzz_load<F>(terms + 8 * j));
    }
    xyzz_store(red + 8 * threadIdx.x, acc);
    __syncthreads();
    for (int off = LINCOMB_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            xyzz_store(red + 8 * threadIdx.x,
                       xyzz_add(xyzz_load<F>(red + 8 * threadIdx.x), xyzz_load<F>(red + 8 * (threadIdx.x + off))));
        __syncthreads();
    }
    valid = __all(valid);  // the block is one wave
    if (threadIdx.x == 0) {
        const XYZZ<F> r = valid ? xyzz_load<F>(red) : xyzz_id<F>();
        xyzz_store(out + 8 * b, r);
        if (is_id) is_id[b] = (valid && xyzz_is_id(r)) ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// (0, 0) or y^2 = x^3 + 5 over the curve's base field, ark limbs below the modulus
static bool host_on_curve_or_id(int curve, const halo_wrapped_point_t& P) {
    const HostScalar F{base_mont(curve)};
    if (F.M.geq_p(P.x) || F.M.geq_p(P.y)) return false;
    if (HostScalar::is_zero(P.x) && HostScalar::is_zero(P.y)) return true;
    uint64_t y2[4], x2[4], x3[4], five[4], rhs[4];
    F.M.mul(P.y, P.y, y2);
    F.M.mul(P.x, P.x, x2);
    F.M.mul(x2, P.x, x3);
    F.add(F.M.one, F.M.one, five);
    F.add(five, five, five);
    F.add(five, F.M.one, five);
    F.add(x3, five, rhs);
    for (int i = 0; i < 4; i++)
        if (y2[i] != rhs[i]) return false;
    return true;
}

// The two launches.  st->mu and a ScratchUse of `s` held by the caller (st->lincomb_terms is shared by the
// calls on every stream).  k >= 1.
int lincomb_device(DeviceState* st, int curve, const void* d_add, const void* d_pts, const void* d_scalars, size_t k,
                   size_t t, void* d_out, void* d_is_id, hipStream_t s) {
    const size_t n = k * t;
    HALO_CHECK(st->lincomb_terms.reserve(std::max<size_t>(n, 1) * 129));
    uint4* terms = st->lincomb_terms.as<uint4>();
    uint8_t* ok = st->lincomb_terms.as<uint8_t>() + 128 * n;
    if (n) {
        const unsigned blocks = (unsigned)((4 * n + LINCOMB_THREADS - 1) / LINCOMB_THREADS);
        ProfScope prof("lincomb_terms", s);
        DISPATCH_CURVE(curve, Cv, {
            HALO_LAUNCH(prof, k_lincomb_terms<Cv>, dim3(blocks), dim3(LINCOMB_THREADS), 0, s, (const uint4*)d_pts,
                        (const uint4*)d_scalars, n, terms, ok);
        });
        HALO_HIP(hipGetLastError());
    }
    ProfScope prof("lincomb_sum", s);
    DISPATCH_CURVE(curve, Cv, {
        HALO_LAUNCH(prof, k_lincomb_sum<Cv>, dim3((unsigned)k), dim3(LINCOMB_THREADS), 0, s, (const uint4*)d_add,
                    (const uint4*)terms, (const uint8_t*)ok, t, (uint4*)d_out, (uint8_t*)d_is_id);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

static int check_lincomb_args(const char* call, halo_curve_t curve, const void* pts, const void* scalars, size_t k, size_t t,
                              const void* out, bool& done) {
    done = false;
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    if (!out || (t && (!pts || !scalars))) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > LINCOMB_MAX_ITEMS) return set_error(HALO_EINVAL, "%s: %zu items (at most %zu)", call, k, LINCOMB_MAX_ITEMS);
    if (t > (SIZE_MAX / 256) / k) return set_error(HALO_EINVAL, "%s: k * t overflows", call);
    if (4 * k * t > (size_t)0x7fffffffu * LINCOMB_THREADS)
        return set_error(HALO_EINVAL, "%s: %zu terms in one call", call, k * t);
    return HALO_OK;
}

// Host arrays -> device, the two launches, and `want` of the results back: out_wrapped (k affine sums,
// converted on the host) and / or is_id (k bytes).  st->mu held.
static int lincomb_host(DeviceState* st, int curve, const halo_wrapped_point_t* add, const halo_wrapped_point_t* pts,
                        const halo_fe_t* scalars, size_t k, size_t t, halo_wrapped_point_t* out_wrapped, uint8_t* is_id) {
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t n = k * t;
    HALO_CHECK(st->scratch[0].reserve(k * 64));
    HALO_CHECK(st->scratch[1].reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(st->scratch[2].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[3].reserve(k * 128));
    HALO_CHECK(st->scratch[4].reserve(k));
    if (add) HALO_CHECK(copy_h2d(st->scratch[0].ptr, add, k * 64, s));
    HALO_CHECK(copy_h2d(st->scratch[1].ptr, pts, n * 64, s));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, scalars, n * 32, s));
    HALO_CHECK(lincomb_device(st, curve, add ? st->scratch[0].ptr : nullptr, st->scratch[1].ptr, st->scratch[2].ptr, k, t,
                              st->scratch[3].ptr, st->scratch[4].ptr, s));
    if (is_id) HALO_CHECK(copy_d2h(is_id, st->scratch[4].ptr, k, s));
    if (out_wrapped) {
        std::vector<uint64_t> xyzz(k * 16);
        HALO_CHECK(copy_d2h(xyzz.data(), st->scratch[3].ptr, k * 128, s));
        for (size_t i = 0; i < k; i += 16) {  // sixteen sums per host inversion
            const int m = (int)std::min<size_t>(16, k - i);
            const void* src[16];
            void* dst[16];
            for (int j = 0; j < m; j++) {
                src[j] = xyzz.data() + 16 * (i + j);
                dst[j] = out_wrapped + i + j;
            }
            host_xyzz_to_wrapped2(curve, src, dst, m);
        }
    }
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_point_lincomb_batch(halo_curve_t curve, const halo_wrapped_point_t* add, const halo_wrapped_point_t* pts,
                                        const halo_fe_t* scalars, size_t k, size_t t, halo_wrapped_point_t* out) {
    clear_error();
    bool done;
    HALO_CHECK(check_lincomb_args("halo_point_lincomb_batch", curve, pts, scalars, k, t, out, done));
    if (done) return HALO_OK;
    for (size_t j = 0; j < k * t; j++)
        if (!scalar_below(curve, scalars[j]))
            return set_error(HALO_EINVAL, "halo_point_lincomb_batch: scalar %zu is not below the modulus", j);
    if (t == 0) {  // no term: the addends themselves, on the host
        for (size_t i = 0; i < k; i++) {
            const bool keep = add && host_on_curve_or_id(curve, add[i]);
            for (int q = 0; q < 4; q++) {
                out[i].x[q] = keep ? add[i].x[q] : 0;
                out[i].y[q] = keep ? add[i].y[q] : 0;
            }
        }
        return HALO_OK;
    }
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return lincomb_host(st, curve, add, pts, scalars, k, t, out, nullptr);
}

extern "C" int halo_point_lincomb_batch_dev(halo_curve_t curve, const void* d_add, const void* d_pts, const void* d_scalars,
                                            size_t k, size_t t, void* d_out_xyzz, void* d_is_identity, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(check_lincomb_args("halo_point_lincomb_batch_dev", curve, d_pts, d_scalars, k, t, d_out_xyzz, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return lincomb_device(st, curve, d_add, d_pts, d_scalars, k, t, d_out_xyzz, d_is_identity, s);
}

extern "C" int halo_pcdl_succinct_check_batch(halo_curve_t curve, size_t d, size_t k, const halo_wrapped_point_t* C_prime,
                                              const halo_fe_t* z, const halo_fe_t* v, const halo_fe_t* xis,
                                              const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
                                              const halo_wrapped_point_t* U, const halo_fe_t* c, uint8_t* ok_out) {
    clear_error();
    const char* call = "halo_pcdl_succinct_check_batch";
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) return HALO_OK;
    const size_t n = d + 1;
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    const size_t lg = ilog2(n), t = 2 * lg + 2;
    if (!C_prime || !z || !v || !xis || !U || !c || !ok_out || (lg && (!Ls || !Rs)))
        return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > LINCOMB_MAX_ITEMS / t) return set_error(HALO_EINVAL, "%s: %zu instances in one call", call, k);
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_verifier_srs(call, st, curve, d, true));
    const SrsState& srs = st->srs[curve];
    // the scalars of every term, on the host
    const HostScalar Sc{scalar_mont(curve)};
    const HostMont& M = Sc.M;
    for (size_t i = 0; i < k; i++) {
        if (!scalar_below(curve, z[i]) || !scalar_below(curve, v[i]) || !scalar_below(curve, c[i]))
            return set_error(HALO_EINVAL, "%s: a scalar of instance %zu is not below the modulus", call, i);
        for (size_t j = 0; j <= lg; j++)
            if (!scalar_below(curve, xis[i * (lg + 1) + j]))
                return set_error(HALO_EINVAL, "%s: xi_%zu of instance %zu is not below the modulus", call, j, i);
        for (size_t j = 1; j <= lg; j++)
            if (HostScalar::is_zero(xis[i * (lg + 1) + j].l))
                return set_error(HALO_EINVAL, "%s: xi_%zu of instance %zu is zero (it has no inverse)", call, j, i);
    }
    std::vector<halo_wrapped_point_t> pts(k * t);
    std::vector<halo_fe_t> sc(k * t);
    // xi_(j+1)^-1 for every instance and round with one inversion (Montgomery's trick): slot 2 j of an
    // instance's scalars first holds the prefix product before it, then the inverse
    {
        uint64_t run[4] = {M.one[0], M.one[1], M.one[2], M.one[3]};
        for (size_t i = 0; i < k; i++)
            for (size_t j = 0; j < lg; j++) {
                for (int q = 0; q < 4; q++) sc[i * t + 2 * j].l[q] = run[q];
                M.mul(run, xis[i * (lg + 1) + j + 1].l, run);
            }
        uint64_t inv[4];
        if (lg) M.inv(run, inv);
        for (size_t i = k; i-- > 0;)
            for (size_t j = lg; j-- > 0;) {
                uint64_t pre[4];
                for (int q = 0; q < 4; q++) pre[q] = sc[i * t + 2 * j].l[q];
                M.mul(inv, pre, sc[i * t + 2 * j].l);
                M.mul(inv, xis[i * (lg + 1) + j + 1].l, inv);
            }
    }
    for (size_t i = 0; i < k; i++) {
        const halo_fe_t* xi = xis + i * (lg + 1);
        halo_wrapped_point_t* P = pts.data() + i * t;
        halo_fe_t* s_ = sc.data() + i * t;
        for (size_t j = 0; j < lg; j++) {  // xi_(j+1)^-1 L_j + xi_(j+1) R_j (pcdl.rs:537)
            P[2 * j] = Ls[i * lg + j];
            P[2 * j + 1] = Rs[i * lg + j];
            s_[2 * j + 1] = xi[j + 1];
        }
        // h(z), HPoly::eval (pcdl.rs:222-235)
        uint64_t h[4], zi[4], w[4];
        M.mul(xi[lg].l, z[i].l, w);
        Sc.add(M.one, w, h);
        for (int q = 0; q < 4; q++) zi[q] = z[i].l[q];
        for (size_t j = 1; j < lg; j++) {
            M.mul(zi, zi, zi);
            M.mul(xi[lg - j].l, zi, w);
            Sc.add(M.one, w, w);
            M.mul(h, w, h);
        }
        // C' + v H' + sum (...) == c U + c h(z) H' with H' = xi_0 H: e = xi_0 (v - c h(z)) on H, - c on U
        M.mul(c[i].l, h, w);
        Sc.sub(v[i].l, w, w);
        M.mul(xi[0].l, w, s_[2 * lg].l);
        P[2 * lg] = srs.H_wrapped;
        Sc.neg(c[i].l, s_[2 * lg + 1].l);
        P[2 * lg + 1] = U[i];
    }
    return lincomb_host(st, curve, C_prime, pts.data(), sc.data(), k, t, nullptr, ok_out);
}
