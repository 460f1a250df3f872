// pcdl::succinct_check (crates/accumulation/src/pcdl.rs:483-554) from raw proofs: the Fiat-Shamir
// transcript of every instance (Sponge::new(Protocols::PCDL), outer_sponge.rs) runs on the device, so a
// batch of k instances is one upload, one chain of launches on one stream and one download.
//
//   k_pcdl_alpha        hiding calls only: label, absorb_g(C, C_bar), absorb_fr(z, v), alpha = challenge; writes
//                       the two term rows alpha C_bar and -w' S that the t = 2 linear combination reads
//   (lincomb_device)    C + alpha C_bar - w' S as packed XYZZ
//   k_pcdl_cprime       C' as a WrappedPoint: that sum made affine (the transcript absorbs affine
//                       coordinates), or C itself for an instance that does not hide
//   k_pcdl_challenges   one sponge per instance: [the hiding prefix again,] absorb_g(C'), absorb_fr(z, v), xi_0,
//                       then lg n times absorb_fr(xi_j), absorb_g(L_j, R_j), xi_(j+1)
//   k_pcdl_terms        one lane per instance, in the scalar field: xi_(j+1)^-1 (one inversion), h(z), e, and
//                       the 2 lg n + 2 term rows of halo_pcdl_succinct_check_batch (lincomb.hip)
//   (lincomb_device)    the verdicts: C' + sum of the terms is the identity
//
// The reference continues ONE sponge from alpha into xi_0.  k_pcdl_challenges replays the hiding prefix (four
// or five of an instance's 60-90 permutations at lg n = 14-20) instead of carrying the sponge's state
// through device memory: both kernels are then the same walk over the transcript and no state format
// exists.  Hiding and plain instances reach the rate-2 boundary at different elements, so a wave that
// mixes them runs its permutations in two groups; a call whose instances all hide, or none, does not
// diverge.  The host side's shared pieces: scratch_layout.hpp, host_scalar.hpp, sponge_launch.hpp, runtime.hpp.
#include "curve.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "outer_sponge.hpp"
#include "pcdl_fs.hpp"
#include "pcdl_transcript.hpp"
#include "quad_ladder.hpp"
#include "runtime.hpp"
#include "sponge_launch.hpp"

namespace halo {

constexpr int FS_THREADS = 64;  // k_pcdl_cprime, k_pcdl_terms: one lane per instance

struct PackedAffine {  // SrsState::S
    uint32_t w[16];
};

// alpha of every instance of a call that has hiding ones (pcdl.rs:506-510), and the rows of the t = 2 linear
// combination C + alpha C_bar - w' S.  An instance that does not hide gets alpha = 0 and two empty rows;
// bad[i] = 1 for a hiding instance whose C or C_bar is neither (0, 0) nor on the curve or whose w' is not
// below the modulus.
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_pcdl_alpha(const uint32_t* __restrict__ params, const uint8_t* __restrict__ hiding,
                                                    const uint4* __restrict__ C, const uint4* __restrict__ C_bar,
                                                    const uint4* __restrict__ z, const uint4* __restrict__ v,
                                                    const uint4* __restrict__ w_prime, PackedAffine S_int, size_t k,
                                                    uint4* __restrict__ alpha_out, uint4* __restrict__ pts,
                                                    uint4* __restrict__ sc, uint8_t* __restrict__ bad) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    poseidon::OuterSponge<Cv, LANES> sp;
    sp.init(tab);
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    transcript_stretch(sp, true, false, C + 4 * ic, C_bar + 4 * ic, 2, true, z + 2 * ic, v + 2 * ic, w);
    if (!(writer && i < k)) return;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    if (!hiding[i]) {
        for (int q = 0; q < 8; q++) pts[8 * i + q] = zero;
        for (int q = 0; q < 4; q++) sc[4 * i + q] = zero;
        if (alpha_out) alpha_out[2 * i] = alpha_out[2 * i + 1] = zero;
        bad[i] = 0;
        return;
    }
    const Fe<F> b = fe_from_const<F>(Cv::K::B);
    bad[i] = aff_on_curve_or_id(aff_from_wrapped<F>(C + 4 * i), b) && aff_on_curve_or_id(aff_from_wrapped<F>(C_bar + 4 * i), b) &&
                     ark_is_canonical<S>(w_prime + 2 * i)
                 ? 0
                 : 1;
    for (int q = 0; q < 4; q++) pts[8 * i + q] = C_bar[4 * i + q];
    Affine<F> Sp;
    {
        uint32_t sx[8], sy[8];
        for (int q = 0; q < 8; q++) sx[q] = S_int.w[q], sy[q] = S_int.w[8 + q];
        Sp.x = fe_unpack<F>(sx);
        Sp.y = fe_unpack<F>(sy);
    }
    aff_to_wrapped(pts + 8 * i + 4, Sp);
    poseidon::scalar_words_to_ark<S>(sc + 4 * i, w);
    fe_to_ark(sc + 4 * i + 2, fe_neg(fe_from_ark<S>(w_prime + 2 * i)));
    if (alpha_out) alpha_out[2 * i] = sc[4 * i], alpha_out[2 * i + 1] = sc[4 * i + 1];
}

// C'[i]: the XYZZ sum made affine (one inversion per hiding instance; the identity becomes (0, 0)), or C[i].
template <class Cv>
__global__ __launch_bounds__(FS_THREADS) void k_pcdl_cprime(const uint8_t* __restrict__ hiding, const uint4* __restrict__ C,
                                                            const uint4* __restrict__ sum, size_t k,
                                                            uint4* __restrict__ C_prime) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= k) return;
    if (hiding[i])
        aff_to_wrapped(C_prime + 4 * i, xyzz_to_aff(xyzz_load<F>(sum + 8 * i)));
    else
        for (int q = 0; q < 4; q++) C_prime[4 * i + q] = C[4 * i + q];
}

// xi_0 .. xi_lg of every instance (pcdl.rs:518-534) into xis[i (lg + 1) + j], ark.
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_pcdl_challenges(const uint32_t* __restrict__ params,
                                                         const uint8_t* __restrict__ hiding, const uint4* __restrict__ C,
                                                         const uint4* __restrict__ C_bar, const uint4* __restrict__ C_prime,
                                                         const uint4* __restrict__ z, const uint4* __restrict__ v,
                                                         const uint4* __restrict__ Ls, const uint4* __restrict__ Rs, size_t lg,
                                                         size_t k, uint4* __restrict__ xis) {
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    poseidon::OuterSponge<Cv, LANES> sp;
    sp.init(tab);
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int first = hiding && hiding[ic] ? -1 : 0;
    // stretch -1: the hiding prefix (its challenge, alpha, is dropped); 0: C', z, v -> xi_0; j >= 1: xi_(j-1), L_(j-1), R_(j-1) -> xi_j
#pragma unroll 1
    for (int j = first; j <= (int)lg; j++) {
        const uint4* p0 = j < 0 ? C + 4 * ic : j == 0 ? C_prime + 4 * ic : Ls + 4 * (ic * lg + (j - 1));
        const uint4* p1 = j < 0 ? C_bar + 4 * ic : j == 0 ? p0 : Rs + 4 * (ic * lg + (j - 1));
        transcript_stretch(sp, j == first, j > 0, p0, p1, j == 0 ? 1 : 2, j <= 0, z + 2 * ic, v + 2 * ic, w);
        if (j >= 0 && writer && i < k) poseidon::scalar_words_to_ark<S>(xis + 2 * (i * (lg + 1) + j), w);
    }
}

// The term rows of instance i, in the layout halo_pcdl_succinct_check_batch builds on the host: rows 2 j,
// 2 j + 1 are xi_(j+1)^-1 L_j and xi_(j+1) R_j (pcdl.rs:537), row 2 lg is e H with e = xi_0 (v - c h(z)), h(z) as
// HPoly::eval (pcdl.rs:222-235), row 2 lg + 1 is -c U.  Row 2 j of the scalars first holds the prefix product
// before xi_(j+1) (internal form), then the inverse: one inversion per instance.  An instance that cannot
// have a verdict -- bad[i] set, z, v or c not below the modulus, a zero xi_(j+1) (the reference unwraps
// its inverse) -- gets an e that is not below the modulus, which k_lincomb_terms answers with an invalid
// term and so verdict 0.
template <class Cv>
__global__ __launch_bounds__(FS_THREADS) void k_pcdl_terms(const uint4* __restrict__ xis, const uint4* __restrict__ z,
                                                           const uint4* __restrict__ v, const uint4* __restrict__ c,
                                                           const uint4* __restrict__ Ls, const uint4* __restrict__ Rs,
                                                           const uint4* __restrict__ U, halo_wrapped_point_t H,
                                                           const uint8_t* __restrict__ bad, size_t lg, size_t k,
                                                           uint4* __restrict__ pts, uint4* __restrict__ sc) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= k) return;
    const size_t t = 2 * lg + 2;
    const uint4* xi = xis + 2 * i * (lg + 1);
    pts += 4 * i * t;
    sc += 2 * i * t;
    bool reject = (bad && bad[i]) || !ark_is_canonical<S>(z + 2 * i) || !ark_is_canonical<S>(v + 2 * i) ||
                  !ark_is_canonical<S>(c + 2 * i);
    Fe<S> run = fe_one<S>();
#pragma unroll 1
    for (size_t j = 0; j < lg; j++) {
        const Fe<S> x = fe_from_ark<S>(xi + 2 * (j + 1));
        reject = reject || fe_is_zero(x);
        fe_store(sc + 4 * j, run);
        run = fe_mul(run, x);
        sc[4 * j + 2] = xi[2 * (j + 1)];
        sc[4 * j + 3] = xi[2 * (j + 1) + 1];
        for (int q = 0; q < 4; q++) {
            pts[8 * j + q] = Ls[4 * (i * lg + j) + q];
            pts[8 * j + 4 + q] = Rs[4 * (i * lg + j) + q];
        }
    }
    Fe<S> inv = fe_inv(run);
#pragma unroll 1
    for (size_t j = lg; j-- > 0;) {
        const Fe<S> pre = fe_load<S>(sc + 4 * j);
        fe_to_ark(sc + 4 * j, fe_mul(inv, pre));
        inv = fe_mul(inv, fe_from_ark<S>(xi + 2 * (j + 1)));
    }
    const Fe<S> one = fe_one<S>();
    Fe<S> zi = fe_from_ark<S>(z + 2 * i);
    Fe<S> h = fe_add(one, fe_mul(fe_from_ark<S>(xi + 2 * lg), zi));
#pragma unroll 1
    for (size_t j = 1; j < lg; j++) {
        zi = fe_sqr(zi);
        h = fe_mul(h, fe_add(one, fe_mul(fe_from_ark<S>(xi + 2 * (lg - j)), zi)));
    }
    const Fe<S> cc = fe_from_ark<S>(c + 2 * i);
    const Fe<S> e = fe_mul(fe_from_ark<S>(xi), fe_sub(fe_from_ark<S>(v + 2 * i), fe_mul(cc, h)));
    if (reject)
        sc[4 * lg] = sc[4 * lg + 1] = make_uint4(~0u, ~0u, ~0u, ~0u);
    else
        fe_to_ark(sc + 4 * lg, e);
    fe_to_ark(sc + 4 * lg + 2, fe_neg(cc));
    auto u4 = [](uint64_t lo, uint64_t hi) {
        return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
    };
    for (int q = 0; q < 2; q++) {
        pts[8 * lg + q] = u4(H.x[2 * q], H.x[2 * q + 1]);
        pts[8 * lg + 2 + q] = u4(H.y[2 * q], H.y[2 * q + 1]);
    }
    for (int q = 0; q < 4; q++) pts[8 * lg + 4 + q] = U[4 * i + q];
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// Everything that needs no device; done: an empty batch.
int check_fs_args(const char* call, const FsCall& a, bool& done) {
    done = false;
    if (!valid_curve(a.curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (a.k == 0) {
        done = true;
        return HALO_OK;
    }
    const size_t n = a.d + 1;
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    const size_t lg = ilog2(n);
    if (!a.C || !a.z || !a.v || !a.U || !a.c || !a.ok || (lg && (!a.Ls || !a.Rs)))
        return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (a.hiding && (!a.C_bar || !a.w_prime)) return set_error(HALO_EINVAL, "%s: hiding without C_bar and w_prime", call);
    if (a.k > LINCOMB_MAX_ITEMS / (2 * lg + 2)) return set_error(HALO_EINVAL, "%s: %zu instances in one call", call, a.k);
    return require_poseidon_params(call, a.curve);
}

// The launches of one call over device pointers, all on `s`.  st->mu and a ScratchUse of `s` held; a.k >= 1.
int fs_device(const char* call, DeviceState* st, const FsCall& a, hipStream_t s) {
    HALO_CHECK(check_verifier_srs(call, st, a.curve, a.d, true));
    const SrsState& srs = st->srs[a.curve];
    const size_t k = a.k, lg = ilog2(a.d + 1), t = 2 * lg + 2;
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(a.curve), &params));
    // one scratch buffer: the term rows, the sums, and what the caller did not ask to see
    ScratchLayout lay;
    const size_t o_pts = lay.take(k * t * 64), o_sc = lay.take(k * t * 32), o_sum = lay.take(k * 128),
                 o_xis = lay.take(a.xis_out ? 0 : k * (lg + 1) * 32), o_cp = lay.take(a.hiding ? k * 64 : 0),
                 o_bad = lay.take(a.hiding ? k : 0);
    HALO_CHECK(st->scratch[7].reserve(lay.total()));
    HALO_CHECK(st->lincomb_terms.reserve(k * t * 129));  // both linear combinations, before anything is in flight
    uint8_t* base = st->scratch[7].as<uint8_t>();
    uint4 *pts = (uint4*)(base + o_pts), *sc = (uint4*)(base + o_sc), *sum = (uint4*)(base + o_sum);
    uint4* xis = a.xis_out ? (uint4*)a.xis_out : (uint4*)(base + o_xis);
    const uint4* Cp = (const uint4*)a.C;
    uint8_t* bad = nullptr;
    const dim3 per_lane(grid_for(k, FS_THREADS));
    if (a.hiding) {
        bad = base + o_bad;
        PackedAffine S_int;
        for (int q = 0; q < 16; q++) S_int.w[q] = srs.S[q];
        HALO_CHECK(SPONGE_LAUNCH(st, a.curve, Cv, L, k, "pcdl_alpha", s, (k_pcdl_alpha<Cv, L>), params, (const uint8_t*)a.hiding,
                                 (const uint4*)a.C, (const uint4*)a.C_bar, (const uint4*)a.z, (const uint4*)a.v,
                                 (const uint4*)a.w_prime, S_int, k, (uint4*)a.alpha_out, pts, sc, bad));
        HALO_CHECK(lincomb_device(st, a.curve, a.C, pts, sc, k, 2, sum, nullptr, s));
        uint4* cp = (uint4*)(base + o_cp);
        DISPATCH_CURVE(a.curve, Cv, {
            hipLaunchKernelGGL(k_pcdl_cprime<Cv>, per_lane, dim3(FS_THREADS), 0, s, (const uint8_t*)a.hiding,
                               (const uint4*)a.C, (const uint4*)sum, k, cp);
        });
        HALO_HIP(hipGetLastError());
        Cp = cp;
    } else if (a.alpha_out) {
        HALO_HIP(hipMemsetAsync(a.alpha_out, 0, k * 32, s));
    }
    HALO_CHECK(SPONGE_LAUNCH(st, a.curve, Cv, L, k, "pcdl_challenges", s, (k_pcdl_challenges<Cv, L>), params,
                             (const uint8_t*)a.hiding, (const uint4*)a.C, (const uint4*)a.C_bar, Cp, (const uint4*)a.z,
                             (const uint4*)a.v, (const uint4*)a.Ls, (const uint4*)a.Rs, lg, k, xis));
    {
        ProfScope prof("pcdl_terms", s);
        DISPATCH_CURVE(a.curve, Cv, {
            HALO_LAUNCH(prof, k_pcdl_terms<Cv>, per_lane, dim3(FS_THREADS), 0, s, (const uint4*)xis, (const uint4*)a.z,
                        (const uint4*)a.v, (const uint4*)a.c, (const uint4*)a.Ls, (const uint4*)a.Rs, (const uint4*)a.U,
                        srs.H_wrapped, (const uint8_t*)bad, lg, k, pts, sc);
        });
        HALO_HIP(hipGetLastError());
    }
    return lincomb_device(st, a.curve, Cp, pts, sc, k, t, sum, a.ok, s);
}

// The host form's scalars: z, v, c and every w' that is read are below the modulus.
int fs_host_scalars(const char* call, const FsCall& host) {
    const halo_fe_t *z = (const halo_fe_t*)host.z, *v = (const halo_fe_t*)host.v, *c = (const halo_fe_t*)host.c,
                    *w_prime = (const halo_fe_t*)host.w_prime;
    const uint8_t* hiding = (const uint8_t*)host.hiding;
    for (size_t i = 0; i < host.k; i++)
        if (!scalar_below(host.curve, z[i]) || !scalar_below(host.curve, v[i]) || !scalar_below(host.curve, c[i]) ||
            (hiding && hiding[i] && !scalar_below(host.curve, w_prime[i])))
            return set_error(HALO_EINVAL, "%s: a scalar of instance %zu is not below the modulus", call, i);
    return HALO_OK;
}

// The inputs of a host call as the rows of upload_parts, and the same call over the device pointers `at` that
// upload_parts answers for them, its outputs null.
HostParts fs_host_parts(const FsCall& host) {
    const size_t k = host.k, lg = ilog2(host.d + 1), hid = host.hiding ? k : 0;
    return HostParts{{host.C, k * 64},       {host.z, k * 32}, {host.v, k * 32}, {host.Ls, k * lg * 64},
                     {host.Rs, k * lg * 64}, {host.U, k * 64}, {host.c, k * 32}, {host.hiding, hid},
                     {host.C_bar, hid * 64}, {host.w_prime, hid * 32}};
}
FsCall fs_dev_call(const FsCall& host, const std::vector<const void*>& at) {
    return FsCall{host.curve, host.d, host.k, at[0], at[1], at[2], at[3], at[4], at[5], at[6], at[7], at[8], at[9],
                  nullptr, nullptr, nullptr};
}

}  // namespace halo

using namespace halo;

extern "C" int halo_pcdl_succinct_check_fs_batch_dev(halo_curve_t curve, size_t d, size_t k, const void* d_C, const void* d_z,
                                                     const void* d_v, const void* d_Ls, const void* d_Rs, const void* d_U,
                                                     const void* d_c, const void* d_hiding, const void* d_C_bar,
                                                     const void* d_w_prime, void* d_xis_out, void* d_alpha_out, void* d_ok,
                                                     void* stream) {
    clear_error();
    const char* call = "halo_pcdl_succinct_check_fs_batch_dev";
    const FsCall a{(int)curve, d, k, d_C, d_z, d_v, d_Ls, d_Rs, d_U, d_c, d_hiding, d_C_bar, d_w_prime, d_xis_out, d_alpha_out, d_ok};
    bool done;
    HALO_CHECK(check_fs_args(call, a, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return fs_device(call, st, a, s);
}

extern "C" int halo_pcdl_succinct_check_fs_batch(halo_curve_t curve, size_t d, size_t k, const halo_wrapped_point_t* C,
                                                 const halo_fe_t* z, const halo_fe_t* v, const halo_wrapped_point_t* Ls,
                                                 const halo_wrapped_point_t* Rs, const halo_wrapped_point_t* U,
                                                 const halo_fe_t* c, const uint8_t* hiding, const halo_wrapped_point_t* C_bar,
                                                 const halo_fe_t* w_prime, halo_fe_t* xis_out, halo_fe_t* alpha_out,
                                                 uint8_t* ok_out) {
    clear_error();
    const char* call = "halo_pcdl_succinct_check_fs_batch";
    const FsCall host{(int)curve, d, k, C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, xis_out, alpha_out, ok_out};
    bool done;
    HALO_CHECK(check_fs_args(call, host, done));
    if (done) return HALO_OK;
    HALO_CHECK(fs_host_scalars(call, host));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t lg = ilog2(d + 1);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, fs_host_parts(host), s, at));
    FsCall a = fs_dev_call(host, at);
    ScratchLayout out;
    const size_t o_xis = out.take(xis_out ? k * (lg + 1) * 32 : 0), o_alpha = out.take(alpha_out ? k * 32 : 0), o_ok = out.total();
    HALO_CHECK(st->scratch[1].reserve(o_ok + k));  // the last part is not padded
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    a.xis_out = xis_out ? dout + o_xis : nullptr;
    a.alpha_out = alpha_out ? dout + o_alpha : nullptr;
    a.ok = dout + o_ok;
    HALO_CHECK(fs_device(call, st, a, s));
    if (xis_out) HALO_CHECK(copy_d2h(xis_out, dout + o_xis, k * (lg + 1) * 32, s));
    if (alpha_out) HALO_CHECK(copy_d2h(alpha_out, dout + o_alpha, k * 32, s));
    return copy_d2h(ok_out, dout + o_ok, k, s);
}
