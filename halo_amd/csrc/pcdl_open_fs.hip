// pcdl::open / pcdl::open_without_eval (crates/accumulation/src/pcdl.rs:326-473) as one call: the opening's
// Fiat-Shamir transcript (Sponge::new(Protocols::PCDL), pcdl.rs:336) runs on the device, so the lg n rounds
// of an opening are one chain of launches on the session's stream with one wait at the end, and k
// openings advance side by side with no host in between.
//
// The sponge lives in the session's small buffer between the kernels (SM_SPONGE, poseidon::STATE_U4: three
// base-field elements below 2p as packed words, then the squeezed flag and the counter n of
// poseidon::Sponge): a prefix replay as in pcdl_fs.hip would cost lg^2 n permutations here.
//
//   k_open_fs_start   one wave.  mode 0: label, absorb_g(C'), absorb_fr(z, v), xi_0 = challenge -> SM_XI0
//                     (pcdl.rs:387-389).  Hiding: mode 1 is label, absorb_g(C, C_bar), absorb_fr(z, v),
//                     alpha = challenge -> SM_ALPHA (pcdl.rs:356-360), which goes home once for
//                     halo_pcdl_open_combine; mode 2 loads that sponge and continues into C' as mode 0.
//   (ipa_round_launch)  L_j, R_j as packed XYZZ at SM_L / SM_R, as for every session
//   k_open_fs_round   one wave after each round: L_j, R_j to affine with one shared inversion (the identity
//                     becomes (0, 0)) into the proof rows at SM_PROOF, absorb_fr(xi_j), absorb_g(L_j, R_j),
//                     xi_(j+1) = challenge (pcdl.rs:413-425), xi_(j+1)^-1, both to SM_XI | SM_XINV; a zero
//                     challenge (the reference unwraps its inverse) sets the status word
//   (ipa_fold_launch)   the fold reads SM_XI | SM_XINV (ipa_session.hpp: xi_dev)
//   (ipa_end_enqueue)   U, c; then Ls, Rs, the status word and v come home with them after one wait
// k openings are enqueued round by round (round j of every session, then round j + 1), each on its own stream.
#include <cstring>
#include <vector>

#include "dispatch.hpp"
#include "ipa_session.hpp"
#include "pcdl_open_fs.hpp"
#include "pcdl_transcript.hpp"
#include "runtime.hpp"
#include "sponge_launch.hpp"

namespace halo {

struct OpenFsStart {
    uint4 p0[4], p1[4];  // mode 0 / 2: C'; mode 1: C, C_bar (WrappedPoints)
    uint4 v[2];          // the caller's v (has_v), else v is already at SM_V (ipa_eval_cs_enqueue)
    int mode, has_v;
};

template <class Cv, int LANES>
__global__ __launch_bounds__(64) void k_open_fs_start(const uint32_t* __restrict__ params, uint4* sm, const OpenFsStart a) {
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    __shared__ uint4 in[10];  // p0 | p1 | v
    poseidon::stage_params(params, tab);
    uint4* smv = sm + SM_V / 16;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            in[q] = a.p0[q];
            in[4 + q] = a.p1[q];
        }
#pragma unroll
        for (int q = 0; q < 2; q++) {
            in[8 + q] = a.has_v ? a.v[q] : smv[q];
            if (a.has_v) smv[q] = a.v[q];
        }
    }
    __syncthreads();
    bool writer;
    const bool mine = sponge_index<LANES>(writer) == 0;  // every sponge of the wave walks the same transcript
    uint4* state = sm + SM_SPONGE / 16;
    poseidon::OuterSponge<Cv, LANES> sp;
    if (a.mode == 2)
        sp.load(tab, state);
    else
        sp.init(tab);
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    transcript_stretch(sp, a.mode != 2, false, in, in + 4, a.mode == 1 ? 2 : 1, true, sm + SM_Z / 16, in + 8, w);
    sp.store(state, mine);
    if (threadIdx.x != 0) return;
    poseidon::scalar_words_to_ark<S>(sm + (a.mode == 1 ? SM_ALPHA : SM_XI0) / 16, w);
    if (a.mode != 2) *(uint32_t*)(sm + SM_STATUS / 16) = 0u;  // a fresh transcript
}

// proof_j: the round's rows L_j | R_j (8 uint4); xi_prev: xi_j (SM_XI0 in round 0, SM_XI afterwards)
template <class Cv, int LANES>
__global__ __launch_bounds__(64) void k_open_fs_round(const uint32_t* __restrict__ params, uint4* sm, const uint4* xi_prev,
                                                      uint4* proof_j) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    __shared__ uint4 lr[8];
    poseidon::stage_params(params, tab);
    if (threadIdx.x == 0) {
        const XYZZ<F> L = xyzz_load<F>(sm + SM_L / 16), R = xyzz_load<F>(sm + SM_R / 16);
        const bool il = xyzz_is_id(L), ir = xyzz_is_id(R);
        const Fe<F> zl = il ? fe_one<F>() : fe_mul(L.ZZ, L.ZZZ), zr = ir ? fe_one<F>() : fe_mul(R.ZZ, R.ZZZ);
        const Fe<F> t = fe_inv(fe_mul(zl, zr));
        const Fe<F> tl = fe_mul(t, zr), tr = fe_mul(t, zl);  // 1 / (ZZ ZZZ) of L and of R
        Affine<F> al, ar;
        al.x = il ? fe_zero<F>() : fe_mul(L.X, fe_mul(tl, L.ZZZ));
        al.y = il ? fe_zero<F>() : fe_mul(L.Y, fe_mul(tl, L.ZZ));
        ar.x = ir ? fe_zero<F>() : fe_mul(R.X, fe_mul(tr, R.ZZZ));
        ar.y = ir ? fe_zero<F>() : fe_mul(R.Y, fe_mul(tr, R.ZZ));
        aff_to_wrapped(lr, al);
        aff_to_wrapped(lr + 4, ar);
#pragma unroll
        for (int q = 0; q < 8; q++) proof_j[q] = lr[q];
    }
    __syncthreads();
    bool writer;
    const bool mine = sponge_index<LANES>(writer) == 0;
    uint4* state = sm + SM_SPONGE / 16;
    poseidon::OuterSponge<Cv, LANES> sp;
    sp.load(tab, state);
    uint32_t w[8];
    fe_ark_to_canonical_words<S>(xi_prev, w);
    transcript_stretch(sp, false, true, lr, lr + 4, 2, false, (const uint4*)nullptr, (const uint4*)nullptr, w);
    sp.store(state, mine);
    if (threadIdx.x != 0) return;
    uint32_t any = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) any |= w[q];
    const Fe<S> x = poseidon::fe_from_canonical_words<S>(w);
    if (!any) *(uint32_t*)(sm + SM_STATUS / 16) = 1u;
    fe_to_ark(sm + SM_XI / 16, x);
    fe_to_ark(sm + SM_XINV / 16, any ? fe_inv(x) : fe_zero<S>());
}

namespace {

// one block of one wave: the transcript of one opening, in the lane layout its caller chose
inline SpongeLaunchPlan one_wave(int lanes) { return {lanes, {1, 64}}; }

int launch_start(halo_ipa_session* ses, const uint32_t* params, int lanes, int mode, const halo_wrapped_point_t* p0,
                 const halo_wrapped_point_t* p1, const halo_fe_t* v) {
    OpenFsStart a{};
    memcpy(a.p0, p0, 64);
    if (p1) memcpy(a.p1, p1, 64);
    if (v) memcpy(a.v, v, 32);
    a.mode = mode;
    a.has_v = v != nullptr;
    return SPONGE_LAUNCH_AT(DISPATCH_CURVE, ses->op.curve, Cv, L, one_wave(lanes), nullptr, ses->s, (k_open_fs_start<Cv, L>), params,
                            ses->small.as<uint4>(), a);
}

// Round j of an opening whose xi_0 is resident: L_j and R_j, the transcript kernel, the fold.  Nothing here
// waits for the device.
int enqueue_round(DeviceState* st, halo_ipa_session* ses, const uint32_t* params, int lanes, size_t j) {
    hipStream_t s = ses->s;
    char* sm = ses->small.as<char>();
    HALO_CHECK(ipa_round_launch(st, ses));
    ses->poll_pending = false;  // (what a tail / pair round emits to the pinned staging is not waited for)
    const uint4* xi_prev = (const uint4*)(sm + (j ? SM_XI : SM_XI0));
    uint4* row = (uint4*)(sm + SM_PROOF + 128 * j);
    HALO_CHECK(SPONGE_LAUNCH_AT(DISPATCH_CURVE, ses->op.curve, Cv, L, one_wave(lanes), "open_fs_round", s, (k_open_fs_round<Cv, L>),
                                params, (uint4*)sm, xi_prev, row));
    return ipa_fold_launch(st, ses, nullptr, nullptr);
}

// U and c, and the copies of the proof rows, the status word and v to the pinned staging
int enqueue_end(DeviceState* st, halo_ipa_session* ses) {
    hipStream_t s = ses->s;
    char* sm = ses->small.as<char>();
    HALO_CHECK(ipa_end_enqueue(st, ses));
    HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_PROOF, sm + SM_PROOF, ilog2(ses->op.n) * 128, hipMemcpyDeviceToHost, s));
    HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_STATUS, sm + SM_STATUS, 4, hipMemcpyDeviceToHost, s));
    HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_V, sm + SM_V, 32, hipMemcpyDeviceToHost, s));
    return HALO_OK;
}

// Everything after the start kernels of k sessions: H' = xi_0 H, then the rounds of all sessions round by round
// (as the lockstep entry points enqueue them: each stream keeps its own MSM scratch slot, msm.hip, where a
// session enqueued whole would take every slot and its neighbours would queue behind it), then the ends.
int enqueue_chains(DeviceState* st, halo_ipa_session* const* ses, size_t k, const uint32_t* params, int lanes) {
    for (size_t i = 0; i < k; i++)
        HALO_CHECK(ipa_start(st, ses[i], nullptr, nullptr, &st->srs[ses[i]->op.curve].H_wrapped, true));
    const size_t lg = ilog2(ses[0]->op.n);
    for (size_t j = 0; j < lg; j++)
        for (size_t i = 0; i < k; i++) HALO_CHECK(enqueue_round(st, ses[i], params, lanes, j));
    for (size_t i = 0; i < k; i++) HALO_CHECK(enqueue_end(st, ses[i]));
    return HALO_OK;
}

// The one wait, and the proof from the pinned staging
int finish(const char* call, halo_ipa_session* ses, halo_wrapped_point_t* Ls, halo_wrapped_point_t* Rs, halo_wrapped_point_t* U,
           halo_fe_t* c, halo_fe_t* v_out) {
    HALO_CHECK(ipa_end_finish(ses, U, c));
    const size_t lg = ilog2(ses->op.n);
    for (size_t j = 0; j < lg; j++) {
        memcpy(&Ls[j], ses->pinned + PIN_PROOF + 128 * j, 64);
        memcpy(&Rs[j], ses->pinned + PIN_PROOF + 128 * j + 64, 64);
    }
    if (v_out) memcpy(v_out, ses->pinned + PIN_V, 32);
    uint32_t status;
    memcpy(&status, ses->pinned + PIN_STATUS, 4);
    if (status) return set_error(HALO_EINVAL, "%s: a round challenge is zero (no inverse)", call);
    return HALO_OK;
}

// what both entry points check before the device is touched
int check_shape(const char* call, halo_curve_t curve, size_t d) {
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    const size_t n = d + 1;
    if (n <= 1) return set_error(HALO_EINVAL, "%s: assertion failed: n > 1", call);
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    if (ilog2(n) > SM_ROUNDS_MAX) return set_error(HALO_EINVAL, "%s: more than %zu rounds", call, SM_ROUNDS_MAX);
    return HALO_OK;
}

int check_srs(const char* call, DeviceState* st, int curve, size_t d) {
    const SrsState& srs = st->srs[curve];
    if (!srs.n || d > srs.n - 1) return set_error(HALO_ESRSRANGE, "assertion failed: d <= pp.D");
    if (!srs.has_sh) return set_error(HALO_ESRSRANGE, "%s: no (S, H) uploaded", call);
    return HALO_OK;
}

}  // namespace

// k plain openings over device-resident coefficients, each in its own pooled session: every session's whole chain is
// enqueued before any is waited for, and every session goes back to the pool on every path.
int open_fs_dev_chain(const char* call, DeviceState* st, int curve, size_t k, const void* const* d_p, const size_t* lens,
                      size_t d, const halo_fe_t* z, const halo_wrapped_point_t* C, halo_wrapped_point_t* Ls,
                      halo_wrapped_point_t* Rs, halo_wrapped_point_t* U, halo_fe_t* c, halo_fe_t* v_out) {
    const size_t n = d + 1, lg = ilog2(n);
    HALO_CHECK(check_srs(call, st, curve, d));
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(curve), &params));
    const int lanes = poseidon_lanes(st, 1);
    // every session's whole chain is enqueued before any is waited for
    std::vector<halo_ipa_session*> ses;
    int rc = HALO_OK;
    for (size_t i = 0; i < k && !rc; i++) {
        halo_ipa_session* s = ipa_acquire(st);
        if (!s) {
            rc = HALO_EDEVICE;
            break;
        }
        ses.push_back(s);
        rc = ipa_setup(st, s, curve, n, nullptr, (const halo_fe_t*)d_p[i], lens[i], true, nullptr, &z[i]);
        s->op.xi_dev = true;
        s->solo = k == 1;
        if (!rc) rc = ipa_eval_cs_enqueue(s, lens[i]);
        if (!rc) rc = launch_start(s, params, lanes, 0, &C[i], nullptr, nullptr);
    }
    if (!rc) rc = enqueue_chains(st, ses.data(), k, params, lanes);
    for (size_t i = 0; i < ses.size(); i++) {
        if (rc) continue;
        rc = finish(call, ses[i], Ls + i * lg, Rs + i * lg, U + i, c + i, v_out ? v_out + i : nullptr);
    }
    for (halo_ipa_session* s : ses) ipa_release(s);  // on every path; each waits for its stream
    return rc;
}

int open_fs_check_shape(const char* call, int curve, size_t d) { return check_shape(call, (halo_curve_t)curve, d); }

}  // namespace halo

using namespace halo;

extern "C" int halo_pcdl_open_fs(halo_curve_t curve, const halo_fe_t* p, size_t len, size_t d, const halo_fe_t* z,
                                 const halo_fe_t* v, const halo_wrapped_point_t* C, const halo_fe_t* w, const halo_fe_t* q,
                                 const halo_fe_t* w_bar, halo_wrapped_point_t* Ls, halo_wrapped_point_t* Rs,
                                 halo_wrapped_point_t* U, halo_fe_t* c, halo_wrapped_point_t* C_bar, halo_fe_t* w_prime,
                                 halo_fe_t* v_out) {
    clear_error();
    const char* call = "halo_pcdl_open_fs";
    if ((len && !p) || !z || !C || !Ls || !Rs || !U || !c) return set_error(HALO_EINVAL, "%s: null argument", call);
    HALO_CHECK(check_shape(call, curve, d));
    if (w && (!q || !w_bar || !C_bar || !w_prime))
        return set_error(HALO_EINVAL, "%s: hiding (w) without q, w_bar, C_bar and w_prime", call);
    const size_t n = d + 1;
    // p.degree() <= d: trailing zero coefficients do not count towards the degree
    size_t deg_len = len;
    while (deg_len > 0 && !(p[deg_len - 1].l[0] | p[deg_len - 1].l[1] | p[deg_len - 1].l[2] | p[deg_len - 1].l[3])) deg_len--;
    if (deg_len > n) return set_error(HALO_EDEGREE, "assertion failed: p.degree() <= d");
    HALO_CHECK(require_poseidon_params(call, curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    halo_ipa_session* ses = nullptr;
    const uint32_t* params = nullptr;
    int lanes = 3, rc = HALO_OK;
    {
        std::lock_guard<std::mutex> g(st->mu);
        HALO_CHECK(check_srs(call, st, curve, d));
        HALO_CHECK(poseidon_device_params(st, base_field(curve), &params));
        lanes = poseidon_lanes(st, 1);
        ses = ipa_acquire(st);
        if (!ses) return HALO_EDEVICE;
        rc = ipa_setup(st, ses, curve, n, nullptr, p, deg_len, false, nullptr, z);
        ses->op.xi_dev = true;
        ses->solo = true;
        if (!rc && !v) rc = ipa_eval_cs_enqueue(ses, deg_len);  // pcdl::open: v = p(z) (pcdl.rs:471)
    }
    halo_wrapped_point_t C_prime = *C;
    if (!rc && w) {  // pcdl.rs:344-371: the blind and the combine keep their two host trips
        halo_fe_t alpha;
        rc = halo_pcdl_open_blind(ses, q, w_bar, C_bar);
        if (!rc) {
            std::lock_guard<std::mutex> g(st->mu);
            rc = launch_start(ses, params, lanes, 1, C, C_bar, v);
            if (!rc && (hipMemcpyAsync(ses->pinned + PIN_ALPHA, ses->small.as<char>() + SM_ALPHA, 32, hipMemcpyDeviceToHost,
                                       ses->s) != hipSuccess ||
                        hipStreamSynchronize(ses->s) != hipSuccess))
                rc = set_error(HALO_EDEVICE, "%s: alpha did not come back", call);
            memcpy(&alpha, ses->pinned + PIN_ALPHA, 32);
        }
        if (!rc) rc = halo_pcdl_open_combine(ses, &alpha, C, w, w_prime, &C_prime);
    }
    if (!rc) {
        std::lock_guard<std::mutex> g(st->mu);
        // (v went to SM_V with the hiding prefix; the continued sponge absorbs it from there)
        rc = launch_start(ses, params, lanes, w ? 2 : 0, &C_prime, nullptr, w ? nullptr : v);
        if (!rc) rc = enqueue_chains(st, &ses, 1, params, lanes);
        if (!rc) rc = finish(call, ses, Ls, Rs, U, c, v_out);
    }
    ipa_release(ses);  // (waits for the stream: nothing of a failed opening is left running)
    return rc;
}

extern "C" int halo_pcdl_open_fs_dev_multi(halo_curve_t curve, size_t k, const void* const* d_p, const size_t* lens, size_t d,
                                           const halo_fe_t* z, const halo_wrapped_point_t* C, halo_wrapped_point_t* Ls,
                                           halo_wrapped_point_t* Rs, halo_wrapped_point_t* U, halo_fe_t* c,
                                           halo_fe_t* v_out) {
    clear_error();
    const char* call = "halo_pcdl_open_fs_dev_multi";
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) return HALO_OK;
    if (!d_p || !lens || !z || !C || !Ls || !Rs || !U || !c) return set_error(HALO_EINVAL, "%s: null argument", call);
    HALO_CHECK(check_shape(call, curve, d));
    const size_t n = d + 1;
    for (size_t i = 0; i < k; i++) {
        if (lens[i] && !d_p[i]) return set_error(HALO_EINVAL, "%s: null argument (polynomial %zu)", call, i);
        // (the coefficients are on the device: the length stands for the degree)
        if (lens[i] > n) return set_error(HALO_EDEGREE, "assertion failed: p.degree() <= d");
    }
    HALO_CHECK(require_poseidon_params(call, curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return open_fs_dev_chain(call, st, (int)curve, k, d_p, lens, d, z, C, Ls, Rs, U, c, v_out);
}
