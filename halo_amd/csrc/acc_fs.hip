// The accumulation scheme (crates/accumulation/src/acc.rs:128-213) in one call each: common_subroutine, verifier and
// prover with the ASDL transcript (Sponge::new(Protocols::ASDL), acc.rs:135) on the device, for k accumulations of m
// instances of one degree bound, as one chain of launches on one stream.
//
//   (fs_device)          pcdl::succinct_check of the k m instances, their challenges kept (pcdl_fs.hip)
//   k_acc_challenges     one ASDL sponge per accumulation: label, absorb_fr of the m (lg n + 1) xis in instance order,
//                        absorb_g(U_0 .. U_(m-1)), alpha, z' (acc.rs:158-169; nothing is absorbed between the squeezes)
//   k_acc_terms          one lane per (accumulation, instance): alpha^j by square-and-multiply, h_j(z') in product
//                        form (HPoly::eval, pcdl.rs:222-235), the row (U_j, alpha^j) and the share alpha^j h_j(z')
//   k_acc_finish         one lane per accumulation: v' = the sum of its shares (AccumulatedHPolys::eval,
//                        acc.rs:95-101); verifier mode: the addend -acc.C and the bits z' != acc.z, v' != acc.v
//   (lincomb_device)     t = m: C_bar' = sum alpha^j U_j, in verifier mode minus acc.C, whose "valid and the identity"
//                        byte is C_bar' = C_bar
//   k_acc_cbar           where C_bar' is an output: the packed XYZZ sum (plus acc.C again) made affine
//   k_acc_verdict        one lane per accumulation: the first failing check in the reference's order
//
// halo_acc_prover goes on from the resident xis and weights: h = sum alpha^j h_j (hpoly_combine_device) into a
// device buffer, one copy of (C_bar, alpha, z, v, verdict, first_bad) home and one wait, then the plain opening of h
// at z (pcdl_open_fs.hpp).  As in pcdl_fs.hip no sponge state passes between kernels and lanes past the batch
// repeat its last accumulation.  Host side: ScratchLayout / HostParts, scalar_below, DISPATCH_LANES.
#include "acc_fs.hpp"

#include <cstring>

#include "acc_plan.hpp"
#include "curve.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "outer_sponge.hpp"
#include "pcdl_fs.hpp"
#include "pcdl_open_fs.hpp"
#include "poly.hpp"
#include "quad_ladder.hpp"
#include "sponge_launch.hpp"

namespace halo {

constexpr int ACC_ASDL_LABEL = 1;  // Protocols::ASDL (outer_sponge.rs:17-22)
constexpr int ACC_THREADS = 64;    // the kernels with one lane per accumulation or per instance

// asdl[2 i ..] = alpha, z' (ark).  One walk over 1 + NS m (lg + 1) + 2 m elements through the one absorb call, then
// the two challenges through the one challenge call.
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_acc_challenges(const uint32_t* __restrict__ params, const uint4* __restrict__ xis,
                                                        const uint4* __restrict__ U, size_t lg, size_t k, size_t m,
                                                        uint4* __restrict__ asdl) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using S = typename Cv::Scalar;
    constexpr int NS = Sp::FR_ELEMENTS;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    xis += 2 * m * (lg + 1) * ic;
    U += 4 * m * ic;
    Sp sp;
    sp.init(tab);
    // (the counts fit an int: check_acc_args bounds m (lg + 1))
    const int n_fr = NS * (int)m * (int)(lg + 1), total = (int)acc_transcript_elements(m, lg, NS);
#pragma unroll 1
    for (int e = 0; e < total; e++) {
        const int q = e - 1;
        Fe<typename Cv::Base> x;
        if (q < 0) {
            x = Sp::label_element(ACC_ASDL_LABEL);
        } else if (q < n_fr) {
            uint32_t sw[8];
            fe_ark_to_canonical_words<S>(xis + 2 * (q / NS), sw);
            x = Sp::fr_element(sw, q % NS);
        } else {
            x = Sp::g_element(U + 4 * ((q - n_fr) >> 1), (q - n_fr) & 1);
        }
        sp.absorb(x);
    }
#pragma unroll 1
    for (int c = 0; c < 2; c++) {
        uint32_t w[8];
        sp.challenge(w);
        if (writer && i < k) poseidon::scalar_words_to_ark<S>(asdl + 2 * (2 * i + c), w);
    }
}

// Lane g = i m + j: row g of the linear combination, (U_j, alpha^j), and shares[g] = alpha^j h_j(z') (internal form).
// steps: the bit length of m - 1; every lane of the launch runs that many ladder steps, a zero bit keeping the
// square by a select.
template <class Cv>
__global__ __launch_bounds__(ACC_THREADS) void k_acc_terms(const uint4* __restrict__ asdl, const uint4* __restrict__ xis,
                                                           const uint4* __restrict__ U, size_t lg, size_t k, size_t m,
                                                           int steps, uint4* __restrict__ pts, uint4* __restrict__ sc,
                                                           uint4* __restrict__ shares) {
    using S = typename Cv::Scalar;
    const size_t g = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
    if (g >= k * m) return;
    const size_t i = g / m, j = g % m;
    const Fe<S> one = fe_one<S>(), alpha = fe_from_ark<S>(asdl + 4 * i), z = fe_from_ark<S>(asdl + 4 * i + 2);
    Fe<S> ap = one;
#pragma unroll 1
    for (int b = steps - 1; b >= 0; b--) {
        ap = fe_sqr(ap);
        ap = fe_select((j >> b) & 1, fe_mul(ap, alpha), ap);
    }
    const uint4* xi = xis + 2 * g * (lg + 1);
    Fe<S> zi = z, h = one;
    if (lg) h = fe_add(one, fe_mul(fe_from_ark<S>(xi + 2 * lg), zi));
#pragma unroll 1
    for (size_t q = 1; q < lg; q++) {
        zi = fe_sqr(zi);
        h = fe_mul(h, fe_add(one, fe_mul(fe_from_ark<S>(xi + 2 * (lg - q)), zi)));
    }
    fe_store(shares + 2 * g, fe_mul(h, ap));
    fe_to_ark(sc + 2 * g, ap);
    for (int q = 0; q < 4; q++) pts[4 * g + q] = U[4 * g + q];
}

// Lane i: v' = sum_j shares[i m + j] to v_out[i] (ark; null: not kept).  With acc_C: neg_C[i] = -acc_C[i] and
// bits[i] |= ACC_BIT_Z / ACC_BIT_V where z' / v' differ from acc_z[i] / acc_v[i] or those are not below the modulus.
template <class Cv>
__global__ __launch_bounds__(ACC_THREADS) void k_acc_finish(const uint4* __restrict__ asdl, const uint4* __restrict__ shares,
                                                            const uint4* __restrict__ acc_C, const uint4* __restrict__ acc_z,
                                                            const uint4* __restrict__ acc_v, size_t k, size_t m,
                                                            uint4* __restrict__ neg_C, uint8_t* __restrict__ bits,
                                                            uint4* __restrict__ v_out) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
    if (i >= k) return;
    Fe<S> hv = fe_zero<S>();
#pragma unroll 1
    for (size_t j = 0; j < m; j++) hv = fe_add(hv, fe_load<S>(shares + 2 * (i * m + j)));
    if (v_out) fe_to_ark(v_out + 2 * i, hv);
    if (!acc_C) return;
    Affine<F> C = aff_from_wrapped<F>(acc_C + 4 * i);
    if (!aff_is_id(C)) C.y = fe_neg(C.y);
    aff_to_wrapped(neg_C + 4 * i, C);
    const bool z_eq = ark_is_canonical<S>(acc_z + 2 * i) && fe_eq(fe_from_ark<S>(asdl + 4 * i + 2), fe_from_ark<S>(acc_z + 2 * i));
    const bool v_eq = ark_is_canonical<S>(acc_v + 2 * i) && fe_eq(hv, fe_from_ark<S>(acc_v + 2 * i));
    bits[i] |= (z_eq ? 0 : ACC_BIT_Z) | (v_eq ? 0 : ACC_BIT_V);
}

// C_bar'[i] as a WrappedPoint (the identity becomes (0, 0)): the lincomb's sum, to which verifier mode adds back the
// acc_C it subtracted (unspecified where acc_C[i] is no point: that item's sum is the identity).
template <class Cv>
__global__ __launch_bounds__(ACC_THREADS) void k_acc_cbar(const uint4* __restrict__ sum, const uint4* __restrict__ acc_C,
                                                          size_t k, uint4* __restrict__ out) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
    if (i >= k) return;
    XYZZ<F> P = xyzz_load<F>(sum + 8 * i);
    if (acc_C) P = xyzz_madd(P, aff_from_wrapped<F>(acc_C + 4 * i));
    aff_to_wrapped(out + 4 * i, xyzz_to_aff(P));
}

// verdict[i]: the instances in order, then C_bar, z, v (acc.rs:149,207-210); first_bad[i] (or null): the failing
// instance, else m.  c_is_id null: common_subroutine alone, ACCEPT or INSTANCE.
__global__ __launch_bounds__(ACC_THREADS) void k_acc_verdict(const uint8_t* __restrict__ ok, const uint8_t* __restrict__ c_is_id,
                                                             const uint8_t* __restrict__ bits, size_t k, size_t m,
                                                             uint8_t* __restrict__ verdict, uint32_t* __restrict__ first_bad) {
    const size_t i = (size_t)blockIdx.x * ACC_THREADS + threadIdx.x;
    if (i >= k) return;
    size_t bad = m;
#pragma unroll 1
    for (size_t j = m; j-- > 0;)
        if (!ok[i * m + j]) bad = j;
    uint8_t v = HALO_ACC_ACCEPT;
    if (bad < m)
        v = HALO_ACC_INSTANCE;
    else if (c_is_id && !c_is_id[i])
        v = HALO_ACC_C_BAR;
    else if (c_is_id && (bits[i] & ACC_BIT_Z))
        v = HALO_ACC_Z;
    else if (c_is_id && (bits[i] & ACC_BIT_V))
        v = HALO_ACC_V;
    verdict[i] = v;
    if (first_bad) first_bad[i] = (uint32_t)bad;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int acc_challenges_launch(DeviceState* st, int curve, const void* d_xis, const void* d_U, size_t lg, size_t k, size_t m,
                          void* d_asdl, hipStream_t s, const char* prof_name) {
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(curve), &params));
    return SPONGE_LAUNCH(st, curve, Cv, L, k, prof_name, s, (k_acc_challenges<Cv, L>), params, (const uint4*)d_xis,
                         (const uint4*)d_U, lg, k, m, (uint4*)d_asdl);
}

int acc_terms_launch(int curve, const void* d_asdl, const void* d_xis, const void* d_U, const void* d_acc_C,
                     const void* d_acc_z, const void* d_acc_v, size_t lg, size_t k, size_t m, void* d_pts, void* d_sc,
                     void* d_shares, void* d_neg_C, void* d_bits, void* d_v_out, hipStream_t s, const char* prof_name) {
    ProfScope prof(prof_name, s);
    DISPATCH_CURVE(curve, Cv, {
        HALO_LAUNCH(prof, k_acc_terms<Cv>, dim3(grid_for(k * m, ACC_THREADS)), dim3(ACC_THREADS), 0, s, (const uint4*)d_asdl,
                    (const uint4*)d_xis, (const uint4*)d_U, lg, k, m, acc_ladder_steps(m), (uint4*)d_pts, (uint4*)d_sc,
                    (uint4*)d_shares);
        hipLaunchKernelGGL(k_acc_finish<Cv>, dim3(grid_for(k, ACC_THREADS)), dim3(ACC_THREADS), 0, s, (const uint4*)d_asdl,
                           (const uint4*)d_shares, (const uint4*)d_acc_C, (const uint4*)d_acc_z, (const uint4*)d_acc_v, k, m,
                           (uint4*)d_neg_C, (uint8_t*)d_bits, (uint4*)d_v_out);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int acc_common_device(const char* call, DeviceState* st, const AccCall& a, hipStream_t s) {
    const size_t k = a.k, m = a.m, km = k * m, lg = ilog2(a.d + 1);
    const bool ver = a.acc_C != nullptr;
    ScratchLayout sl;
    const size_t o_xis = sl.take(km * (lg + 1) * 32), o_ok = sl.take(km), o_pts = sl.take(km * 64), o_sc = sl.take(km * 32),
                 o_sh = sl.take(km * 32), o_sum = sl.take(k * 128), o_asdl = sl.take(a.asdl_out ? 0 : k * 64),
                 o_neg = sl.take(ver ? k * 64 : 0), o_bits = sl.take(k), o_cid = sl.take(ver ? k : 0);
    HALO_CHECK(st->scratch[5].reserve(sl.total()));
    // every linear combination of the chain, before anything is in flight
    HALO_CHECK(st->lincomb_terms.reserve(km * (2 * lg + 2) * 129));
    uint8_t* base = st->scratch[5].as<uint8_t>();
    uint8_t *ok = base + o_ok, *bits = base + o_bits, *cid = ver ? base + o_cid : nullptr;
    void* asdl = a.asdl_out ? a.asdl_out : base + o_asdl;
    const FsCall fs{a.curve, a.d, km, a.C, a.z, a.v, a.Ls, a.Rs, a.U, a.c, a.hiding, a.C_bar, a.w_prime, base + o_xis, nullptr, ok};
    HALO_CHECK(fs_device(call, st, fs, s));
    HALO_CHECK(acc_challenges_launch(st, a.curve, base + o_xis, a.U, lg, k, m, asdl, s, "acc_challenges"));
    HALO_HIP(hipMemsetAsync(bits, 0, k, s));
    HALO_CHECK(acc_terms_launch(a.curve, asdl, base + o_xis, a.U, a.acc_C, a.acc_z, a.acc_v, lg, k, m, base + o_pts, base + o_sc,
                                base + o_sh, ver ? base + o_neg : nullptr, bits, a.v_out, s, "acc_terms"));
    HALO_CHECK(lincomb_device(st, a.curve, ver ? base + o_neg : nullptr, base + o_pts, base + o_sc, k, m, base + o_sum, cid, s));
    const dim3 per_acc(grid_for(k, ACC_THREADS)), blk(ACC_THREADS);
    if (a.C_bar_out) {
        DISPATCH_CURVE(a.curve, Cv, {
            hipLaunchKernelGGL(k_acc_cbar<Cv>, per_acc, blk, 0, s, (const uint4*)(base + o_sum), (const uint4*)a.acc_C, k,
                               (uint4*)a.C_bar_out);
        });
        HALO_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_acc_verdict, per_acc, blk, 0, s, (const uint8_t*)ok, (const uint8_t*)cid, (const uint8_t*)bits, k, m,
                       (uint8_t*)a.verdict, (uint32_t*)a.first_bad);
    HALO_HIP(hipGetLastError());
    if (a.resident) *a.resident = AccResident{base + o_xis, base + o_sc};
    return HALO_OK;
}

namespace {

FsCall instances_of(const AccCall& a) {
    return FsCall{a.curve, a.d, a.k * a.m, a.C, a.z, a.v, a.Ls, a.Rs, a.U, a.c, a.hiding, a.C_bar, a.w_prime, nullptr, nullptr, nullptr};
}

// Everything that needs no device; done (null where k is 1 by construction): an empty batch.  What the call shares
// with a succinct check of its k m instances is check_fs_args' (the shape, the instances' pointers with `verdict` in
// the place of its verdict bytes, hiding, the Poseidon parameters); the accumulation's own conditions follow.
int check_acc_args(const char* call, const AccCall& a, bool* done) {
    if (!valid_curve(a.curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (done) *done = a.k == 0;
    if (a.k == 0) return HALO_OK;
    if (a.m == 0) return set_error(HALO_EINVAL, "%s: No instances given", call);
    if (a.m > LINCOMB_MAX_ITEMS || a.k > LINCOMB_MAX_ITEMS / std::max<size_t>(a.m, 1))  // (k m does not wrap)
        return set_error(HALO_EINVAL, "%s: %zu accumulations of %zu instances in one call", call, a.k, a.m);
    FsCall fs = instances_of(a);
    fs.ok = a.verdict;
    bool none;
    HALO_CHECK(check_fs_args(call, fs, none));
    if ((a.acc_C || a.acc_z || a.acc_v) && !(a.acc_C && a.acc_z && a.acc_v))
        return set_error(HALO_EINVAL, "%s: acc_C, acc_z and acc_v are given together or not at all", call);
    if (!a.acc_C && (!a.C_bar_out || !a.asdl_out || !a.v_out))
        return set_error(HALO_EINVAL, "%s: null pointer (without an accumulator C_bar_out, asdl_out and v_out are the result)", call);
    // (the ASDL walk's 1 + 2 m (lg + 1) + 2 m elements are counted in an int)
    if (a.m > LINCOMB_MAX_ITEMS / (8 * ilog2(a.d + 1) + 8))
        return set_error(HALO_EINVAL, "%s: %zu instances in one accumulation", call, a.m);
    return HALO_OK;
}


// The host form's scalars: those of the instances, and acc_z, acc_v.
int acc_host_scalars(const char* call, const AccCall& host) {
    HALO_CHECK(fs_host_scalars(call, instances_of(host)));
    for (size_t i = 0; host.acc_C && i < host.k; i++)
        if (!scalar_below(host.curve, (const halo_fe_t*)host.acc_z + i, 1) || !scalar_below(host.curve, (const halo_fe_t*)host.acc_v + i, 1))
            return set_error(HALO_EINVAL, "%s: a scalar of accumulator %zu is not below the modulus", call, i);
    return HALO_OK;
}

// The inputs of a host call on the device: the instances' rows (fs_host_parts), then acc_C, acc_z, acc_v.
int upload_acc(DeviceState* st, const AccCall& host, hipStream_t s, AccCall& a) {
    HostParts in = fs_host_parts(instances_of(host));
    const size_t first = in.rows.size(), ka = host.acc_C ? host.k : 0;
    in.add(host.acc_C, ka * 64);
    in.add(host.acc_z, ka * 32);
    in.add(host.acc_v, ka * 32);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, in, s, at));
    const FsCall f = fs_dev_call(instances_of(host), at);
    a = host;
    a.C = f.C, a.z = f.z, a.v = f.v, a.Ls = f.Ls, a.Rs = f.Rs, a.U = f.U, a.c = f.c;
    a.hiding = f.hiding, a.C_bar = f.C_bar, a.w_prime = f.w_prime;
    a.acc_C = at[first], a.acc_z = at[first + 1], a.acc_v = at[first + 2];
    return HALO_OK;
}

}  // namespace
}  // namespace halo

using namespace halo;

extern "C" int halo_acc_verifier_batch_dev(halo_curve_t curve, size_t d, size_t k, size_t m, const void* d_C, const void* d_z,
                                           const void* d_v, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c,
                                           const void* d_hiding, const void* d_C_bar, const void* d_w_prime, const void* d_acc_C,
                                           const void* d_acc_z, const void* d_acc_v, void* d_verdict, void* d_first_bad,
                                           void* d_asdl_out, void* d_C_bar_out, void* d_v_out, void* stream) {
    clear_error();
    const char* call = "halo_acc_verifier_batch_dev";
    const AccCall a{(int)curve, d, k, m, d_C, d_z, d_v, d_Ls, d_Rs, d_U, d_c, d_hiding, d_C_bar, d_w_prime, d_acc_C, d_acc_z,
                    d_acc_v, d_verdict, d_first_bad, d_asdl_out, d_C_bar_out, d_v_out};
    bool done;
    HALO_CHECK(check_acc_args(call, a, &done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return acc_common_device(call, st, a, s);
}

extern "C" int halo_acc_verifier_batch(halo_curve_t curve, size_t d, size_t k, size_t m, const halo_wrapped_point_t* C,
                                       const halo_fe_t* z, const halo_fe_t* v, const halo_wrapped_point_t* Ls,
                                       const halo_wrapped_point_t* Rs, const halo_wrapped_point_t* U, const halo_fe_t* c,
                                       const uint8_t* hiding, const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime,
                                       const halo_wrapped_point_t* acc_C, const halo_fe_t* acc_z, const halo_fe_t* acc_v,
                                       uint8_t* verdict, uint32_t* first_bad, halo_fe_t* asdl_out,
                                       halo_wrapped_point_t* C_bar_out, halo_fe_t* v_out) {
    clear_error();
    const char* call = "halo_acc_verifier_batch";
    const AccCall host{(int)curve, d, k, m, C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, acc_C, acc_z, acc_v, verdict, first_bad,
                       asdl_out, C_bar_out, v_out};
    bool done;
    HALO_CHECK(check_acc_args(call, host, &done));
    if (done) return HALO_OK;
    HALO_CHECK(acc_host_scalars(call, host));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    AccCall a;
    HALO_CHECK(upload_acc(st, host, s, a));
    ScratchLayout out;
    const size_t o_fb = out.take(first_bad ? k * 4 : 0), o_asdl = out.take(asdl_out ? k * 64 : 0),
                 o_cb = out.take(C_bar_out ? k * 64 : 0), o_vo = out.take(v_out ? k * 32 : 0), o_v = out.total();
    HALO_CHECK(st->scratch[1].reserve(o_v + k));  // the last part is not padded
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    a.verdict = dout + o_v;
    a.first_bad = first_bad ? dout + o_fb : nullptr;
    a.asdl_out = asdl_out ? dout + o_asdl : nullptr;
    a.C_bar_out = C_bar_out ? dout + o_cb : nullptr;
    a.v_out = v_out ? dout + o_vo : nullptr;
    HALO_CHECK(acc_common_device(call, st, a, s));
    if (first_bad) HALO_CHECK(copy_d2h(first_bad, dout + o_fb, k * 4, s));
    if (asdl_out) HALO_CHECK(copy_d2h(asdl_out, dout + o_asdl, k * 64, s));
    if (C_bar_out) HALO_CHECK(copy_d2h(C_bar_out, dout + o_cb, k * 64, s));
    if (v_out) HALO_CHECK(copy_d2h(v_out, dout + o_vo, k * 32, s));
    return copy_d2h(verdict, dout + o_v, k, s);
}

extern "C" int halo_acc_prover(halo_curve_t curve, size_t d, size_t m, const halo_wrapped_point_t* C, const halo_fe_t* z,
                               const halo_fe_t* v, const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
                               const halo_wrapped_point_t* U, const halo_fe_t* c, const uint8_t* hiding,
                               const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime, halo_wrapped_point_t* acc_C,
                               halo_fe_t* acc_z, halo_fe_t* acc_v, halo_wrapped_point_t* acc_Ls, halo_wrapped_point_t* acc_Rs,
                               halo_wrapped_point_t* acc_U, halo_fe_t* acc_c, uint8_t* verdict, uint32_t* first_bad) {
    clear_error();
    const char* call = "halo_acc_prover";
    struct Home {  // what comes back in the one copy before the opening
        halo_wrapped_point_t C_bar;
        halo_fe_t asdl[2], v;
        uint32_t first_bad;
        uint8_t verdict;
    } home;
    AccCall host{(int)curve, d, 1, m, C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, nullptr, nullptr, nullptr,
                 &home.verdict, &home.first_bad, home.asdl, &home.C_bar, &home.v};
    HALO_CHECK(check_acc_args(call, host, nullptr));
    if (!acc_C || !acc_z || !acc_v || !acc_Ls || !acc_Rs || !acc_U || !acc_c || !verdict)
        return set_error(HALO_EINVAL, "%s: null pointer", call);
    HALO_CHECK(open_fs_check_shape(call, curve, d));
    HALO_CHECK(acc_host_scalars(call, host));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    const size_t n = d + 1, lg = ilog2(n);
    hipStream_t s = 0;
    const void* h = nullptr;
    {
        ScratchUse su(st, s);
        AccCall a;
        HALO_CHECK(upload_acc(st, host, s, a));
        ScratchLayout out;  // the parts of Home, in its order, as one block
        static_assert(offsetof(Home, asdl) == 64 && offsetof(Home, v) == 128 && offsetof(Home, first_bad) == 160 &&
                          offsetof(Home, verdict) == 164,
                      "Home");
        const size_t o_home = out.take(sizeof(Home)), o_h = out.take(n * 32), o_tab = out.take(hpoly_table_elems(m, lg) * 32);
        HALO_CHECK(st->scratch[1].reserve(out.total()));
        uint8_t* dout = st->scratch[1].as<uint8_t>() + o_home;
        AccResident res{};
        a.C_bar_out = dout, a.asdl_out = dout + 64, a.v_out = dout + 128, a.first_bad = dout + 160, a.verdict = dout + 164;
        a.resident = &res;
        HALO_CHECK(acc_common_device(call, st, a, s));
        // h(X) = sum alpha^j h_j(X) from the resident challenges and weights; it never visits the host
        void* hbuf = st->scratch[1].as<uint8_t>() + o_h;
        HALO_CHECK(hpoly_combine_device(host.curve == HALO_PALLAS ? HALO_FP : HALO_FQ, res.xis, m, (uint32_t)lg, res.weights,
                                        st->scratch[1].as<uint8_t>() + o_tab, hbuf, s, "acc_hpoly_combine"));
        h = hbuf;
        HALO_CHECK(copy_d2h(&home, dout, sizeof(Home), s));  // the one copy and the one wait before the opening's own
    }
    *verdict = home.verdict;
    if (first_bad) *first_bad = home.first_bad;
    if (home.verdict != HALO_ACC_ACCEPT) return HALO_OK;  // acc.rs:149: no accumulator, no session, the outputs untouched
    const size_t len = n;
    halo_fe_t v_open;
    HALO_CHECK(open_fs_dev_chain(call, st, host.curve, 1, &h, &len, d, &home.asdl[1], &home.C_bar, acc_Ls, acc_Rs, acc_U, acc_c,
                                 &v_open));
    // the opener evaluated the coefficients it was given; k_acc_finish the product forms: two routes to one h(z)
    if (memcmp(&v_open, &home.v, sizeof v_open) != 0)
        return set_error(HALO_EDEVICE, "%s: the opening's v = h(z) differs from sum alpha^j h_j(z)", call);
    *acc_C = home.C_bar;
    *acc_z = home.asdl[1];
    *acc_v = home.v;
    return HALO_OK;
}
