// Batched Schnorr verification as ONE MSM under random weights (DESIGN §4.6 "combined pass"), the method of the
// batched decider (§4.9) applied to signatures.  For weights rho_i, all of s_i G == R_i + e_i pk_i hold, up to
// k / 2^254 over a uniform choice of the weights, iff
//
//   D = (sum_i rho_i s_i) G - sum_i rho_i R_i - sum_i (rho_i e_i) pk_i == identity
//
// (Pallas and Vesta have cofactor 1: no subgroup caveat).  D is one MSM of 2 k + 1 terms whatever k, where
// k_schnorr_verify runs k four-term ladders.  Item i is live iff pk_i and R_i are each (0, 0) or on the curve
// (k_schnorr_verify's rule); an item that is not live has verdict 0, weighs nothing in D and is the leaf 0 of the
// derivation.  An identity pk or R is a legal point and takes part: the MSM tests its bases for the identity.
//
//   (k_schnorr_hash)  e_i, once, in both forms: ark for the products, canonical words for the leaves and for the
//                     exact ladder that the host form runs over a rejected batch (schnorr_ladder_device)
//   k_sig_live        live_i
//   k_sig_prepare     one item per lane: bases[2 i] = R_i with scalar -rho_i, bases[2 i + 1] = pk_i with scalar
//                     -rho_i e_i, internal affine and ark scalars as msm_device takes them; (0, 0) and 0 for an item
//                     that is not live; t_i = rho_i s_i summed over the block, one partial per block, beside a flag
//                     for a live item whose rho is zero or not below the modulus
//   k_sig_sum         one block: the sum of the partials -> slot 2 k = (G, sum_i rho_i s_i), the OR of the flags.
//                     Addition mod r is exact and associative: the sum does not depend on the order, no atomics
//   (msm_device)      D over the 2 k + 1 terms, MsmOpts::Sync(): the stream waits for the tail on the device
//   k_sig_finish      combined = D is the identity and no flag; ok[i] = live_i && combined
//
// A rejected pass leaves its terms, liveness bytes, e and D on the device (SigScratch, schnorr.hpp): the host form
// resolves it by the ladder over every item or, under the tuning key schnorr_bisect, by the descent of
// schnorr_bisect.hip, which halo_schnorr_verify_bisect_dev always takes.
//
// Derived weights (no caller RNG), after decide_rho.hip, under labels of their own (rho_plan.hpp):
//   k_sig_leaves      leaf_i = the inner sponge's squeeze after Sponge(SIG_BATCH_LEAF).absorb_fr(e_i).absorb_fr(s_i);
//                     0 with nothing read for an item that is not live.  e_i is already a collision-resistant digest
//                     of (pk_i, R_i, m_i) under SIGNATURE, so the points and the message are not hashed again (that
//                     would double the batch's dominant cost)
//   (k_rho_level, k_rho_weights)  decide_rho.hip's tree and weights (rho_derive_device): seed = squeeze of
//                     Sponge(SIG_BATCH_SEED) after root, k, msg_len; rho_i = challenge of Sponge(SIG_BATCH_WEIGHT) after
//                     seed, i, zero replaced by one; 0 for an item that is not live
#include "curve.hpp"
#include "decider.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "msm.hpp"
#include "outer_sponge.hpp"
#include "quad_ladder.hpp"
#include "rho_plan.hpp"
#include "schnorr.hpp"
#include "sponge_launch.hpp"

namespace halo {

template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_live(const uint4* __restrict__ pk, const uint4* __restrict__ R, size_t k,
                                                          uint8_t* __restrict__ live) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    if (i >= k) return;
    const Fe<F> b = fe_from_const<F>(Cv::K::B);
    live[i] = aff_on_curve_or_id(aff_from_wrapped<F>(pk + 4 * i), b) && aff_on_curve_or_id(aff_from_wrapped<F>(R + 4 * i), b) ? 1 : 0;
}

// The block's sum of t and OR of flag, in thread 0 (every thread of the block calls it).
template <class S>
HALO_DEV Fe<S> sig_block_sum(Fe<S> t, bool& flag, uint32_t (*wsum)[NLIMB], uint32_t* wflag) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Fe<S> o;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) o.v[l] = __shfl_xor(t.v[l], off);
        t = fe_add(t, o);
    }
    const bool wave_flag = __any(flag ? 1 : 0) != 0;
    const unsigned wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) {
#pragma unroll
        for (int l = 0; l < NLIMB; l++) wsum[wave][l] = t.v[l];
        wflag[wave] = wave_flag ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        flag = wflag[0] != 0;
        for (int w = 1; w < SIG_WAVES; w++) {
            Fe<S> o;
#pragma unroll
            for (int l = 0; l < NLIMB; l++) o.v[l] = wsum[w][l];
            t = fe_add(t, o);
            flag = flag || wflag[w] != 0;
        }
    }
    return t;
}

template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_prepare(const uint4* __restrict__ pk, const uint4* __restrict__ R,
                                                             const uint4* __restrict__ rho, const uint4* __restrict__ e_ark,
                                                             const uint4* __restrict__ s, const uint8_t* __restrict__ live,
                                                             size_t k, uint4* __restrict__ bases, uint4* __restrict__ scalars,
                                                             uint4* __restrict__ partials, uint8_t* __restrict__ bad) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint32_t wsum[SIG_WAVES][NLIMB];
    __shared__ uint32_t wflag[SIG_WAVES];
    const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    Fe<S> t = fe_zero<S>();
    bool bad_rho = false;
    if (i < k) {
        Affine<F> Rp, P;
        Rp.x = Rp.y = P.x = P.y = fe_zero<F>();
        Fe<S> nr = fe_zero<S>(), nre = fe_zero<S>();
        if (live[i] != 0) {
            Rp = aff_from_wrapped<F>(R + 4 * i);
            P = aff_from_wrapped<F>(pk + 4 * i);
            const Fe<S> r = fe_from_ark<S>(rho + 2 * i);
            bad_rho = !ark_is_canonical<S>(rho + 2 * i) || fe_is_zero(r);
            nr = fe_neg(r);
            nre = fe_neg(fe_mul(r, fe_from_ark<S>(e_ark + 2 * i)));
            t = fe_mul(r, fe_from_ark<S>(s + 2 * i));
        }
        aff_store(bases + 4 * (2 * i), Rp);
        aff_store(bases + 4 * (2 * i + 1), P);
        fe_to_ark(scalars + 2 * (2 * i), nr);
        fe_to_ark(scalars + 2 * (2 * i + 1), nre);
    }
    t = sig_block_sum(t, bad_rho, wsum, wflag);
    if (threadIdx.x == 0) {
        fe_store(partials + 2 * (size_t)blockIdx.x, t);
        bad[blockIdx.x] = bad_rho ? 1 : 0;
    }
}

// One block: slot 2 k of the MSM and the batch's flag, bad[nb], from the nb partials.
template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_sum(const uint4* __restrict__ partials, uint8_t* __restrict__ bad, size_t nb,
                                                         size_t k, uint4* __restrict__ bases, uint4* __restrict__ scalars) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint32_t wsum[SIG_WAVES][NLIMB];
    __shared__ uint32_t wflag[SIG_WAVES];
    Fe<S> t = fe_zero<S>();
    bool any_bad = false;
    for (size_t j = threadIdx.x; j < nb; j += SIG_THREADS) {
        t = fe_add(t, fe_load<S>(partials + 2 * j));
        any_bad = any_bad || bad[j] != 0;
    }
    t = sig_block_sum(t, any_bad, wsum, wflag);
    if (threadIdx.x != 0) return;
    Affine<F> G;
    G.x = fe_from_const<F>(Cv::K::GX);
    G.y = fe_from_const<F>(Cv::K::GY);
    aff_store(bases + 4 * (2 * k), G);
    fe_to_ark(scalars + 2 * (2 * k), t);
    bad[nb] = any_bad ? 1 : 0;
}

template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_finish(const uint4* __restrict__ D, const uint8_t* __restrict__ flag,
                                                            const uint8_t* __restrict__ live, size_t k, uint8_t* __restrict__ ok,
                                                            uint8_t* __restrict__ combined, uint8_t* __restrict__ combined_own) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    const bool comb = xyzz_is_id(xyzz_load<F>(D)) && flag[0] == 0;
    if (i == 0 && combined) combined[0] = comb ? 1 : 0;
    if (i == 0) combined_own[0] = comb ? 1 : 0;  // the pass's own copy, beside the flag (SigScratch::bad)
    if (i < k) ok[i] = live[i] != 0 && comb ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// derived weights
// ---------------------------------------------------------------------------------------------
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_sig_leaves(const uint32_t* __restrict__ params, const uint4* __restrict__ e_words,
                                                    const uint4* __restrict__ s, const uint8_t* __restrict__ live, size_t k,
                                                    uint4* __restrict__ leaves) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    constexpr unsigned NS = Sp::FR_ELEMENTS;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    const bool on = live[ic] != 0;  // nothing of an item that is not live is read
    Sp sp;
    sp.init(tab);
#pragma unroll 1
    for (unsigned e = 0; e < 1 + 2 * NS; e++) {
        Fe<F> x = fe_zero<F>();
        if (e == 0) {
            x = Sp::label_element(SIG_BATCH_LEAF);
        } else if (!on) {
            // what this sponge hashes is discarded
        } else {
            const unsigned q = e - 1;
            uint32_t w[8];
            if (q < NS) {
                words_from_u4(e_words + 2 * ic, w);
            } else {
                fe_ark_to_canonical_words<S>(s + 2 * ic, w);
            }
            x = Sp::fr_element(w, (int)(q % NS));
        }
        sp.absorb(x);
    }
    const Fe<F> leaf = fe_select(on, sp.inner.squeeze(), fe_zero<F>());
    if (writer && i < k) fe_store(leaves + 2 * i, leaf);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// SigScratch (schnorr.hpp) for a batch of k, in st->schnorr_comb[0].
static int sig_scratch(DeviceState* st, size_t k, SigScratch& w) {
    const size_t n = 2 * k + 1;
    w.nb = grid_for(k, SIG_THREADS);
    ScratchLayout lay;
    const size_t o_e = lay.take(k * 32), o_live = lay.take(k), o_rho = lay.take(k * 32), o_bases = lay.take(n * 64),
                 o_scalars = lay.take(n * 32), o_part = lay.take(w.nb * 32), o_bad = lay.take(w.nb + 2), o_D = lay.take(128);
    HALO_CHECK(st->schnorr_comb[0].reserve(lay.total()));
    uint8_t* base = st->schnorr_comb[0].as<uint8_t>();
    w.e_ark = base + o_e, w.live = base + o_live, w.rho = base + o_rho, w.bases = base + o_bases;
    w.scalars = base + o_scalars, w.partials = base + o_part, w.bad = base + o_bad, w.D = base + o_D;
    w.rho_used = nullptr;
    return HALO_OK;
}

// e in both forms (w.e_ark, st->schnorr_e) and the liveness bytes.
static int sig_hash_live(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_msgs, size_t msg_len,
                         size_t k, const SigScratch& w, hipStream_t s) {
    HALO_CHECK(st->schnorr_e.reserve(k * 32));
    StageScope stage("sig_hash", s);
    HALO_CHECK(schnorr_hash_device(st, curve, d_pk, d_R, d_msgs, msg_len, k, w.e_ark, st->schnorr_e.ptr, s));
    stage.end();
    ProfScope prof("sig_live", s);
    DISPATCH_CURVE(curve, Cv, {
        HALO_LAUNCH(prof, k_sig_live<Cv>, dim3(grid_for(k, SIG_THREADS)), dim3(SIG_THREADS), 0, s, (const uint4*)d_pk,
                    (const uint4*)d_R, k, w.live);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The derived weights of the batch whose e and liveness sig_hash_live left, as k ark scalars at d_rho_out:
// 2 + ceil(lg k) launches on `s`.  Works in st->schnorr_comb[1].
static int sig_rho_device(DeviceState* st, int curve, const void* d_s, size_t msg_len, size_t k, const SigScratch& w,
                          void* d_rho_out, hipStream_t s) {
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(curve), &params));
    uint4* buf[2];
    HALO_CHECK(rho_buffers(st->schnorr_comb[1], k, buf));
    StageScope stage("sig_rho", s);
    HALO_CHECK(SPONGE_LAUNCH(st, curve, Cv, L, k, "sig_leaves", s, (k_sig_leaves<Cv, L>), params, st->schnorr_e.as<const uint4>(),
                             (const uint4*)d_s, (const uint8_t*)w.live, k, buf[0]));
    HALO_CHECK(rho_derive_device(st, curve, params, buf, k, RhoWeights{SIG_BATCH_SEED, SIG_BATCH_WEIGHT, msg_len, "sig_weights"},
                                 w.live, d_rho_out, s));
    stage.end();
    return HALO_OK;
}

// The combined pass (schnorr.hpp).
int sig_combined_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s, const void* d_msgs,
                        size_t msg_len, size_t k, const void* d_rho, void* d_ok, void* d_combined, hipStream_t s, SigScratch& w) {
    HALO_CHECK(sig_scratch(st, k, w));
    HALO_CHECK(sig_hash_live(st, curve, d_pk, d_R, d_msgs, msg_len, k, w, s));
    if (!d_rho) {
        HALO_CHECK(sig_rho_device(st, curve, d_s, msg_len, k, w, w.rho, s));
        d_rho = w.rho;
    }
    w.rho_used = d_rho;
    {
        ProfScope prof("sig_prepare", s);
        DISPATCH_CURVE(curve, Cv, {
            HALO_LAUNCH(prof, k_sig_prepare<Cv>, dim3((unsigned)w.nb), dim3(SIG_THREADS), 0, s, (const uint4*)d_pk,
                        (const uint4*)d_R, (const uint4*)d_rho, (const uint4*)w.e_ark, (const uint4*)d_s,
                        (const uint8_t*)w.live, k, (uint4*)w.bases, (uint4*)w.scalars, (uint4*)w.partials, w.bad);
        });
        HALO_HIP(hipGetLastError());
    }
    {
        ProfScope prof("sig_sum", s);
        DISPATCH_CURVE(curve, Cv, {
            HALO_LAUNCH(prof, k_sig_sum<Cv>, dim3(1), dim3(SIG_THREADS), 0, s, (const uint4*)w.partials, w.bad, w.nb, k,
                        (uint4*)w.bases, (uint4*)w.scalars);
        });
        HALO_HIP(hipGetLastError());
    }
    StageScope stage("sig_msm", s);
    HALO_CHECK(msm_device(st, curve, w.bases, w.scalars, 2 * k + 1, nullptr, nullptr, w.D, s, MsmOpts::Sync().xyzz()));
    stage.end();
    ProfScope prof("sig_finish", s);
    DISPATCH_CURVE(curve, Cv, {
        HALO_LAUNCH(prof, k_sig_finish<Cv>, dim3(grid_for(k, SIG_THREADS)), dim3(SIG_THREADS), 0, s, (const uint4*)w.D,
                    (const uint8_t*)(w.bad + w.nb), (const uint8_t*)w.live, k, (uint8_t*)d_ok, (uint8_t*)d_combined,
                    w.bad + w.nb + 1);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The pass's two bytes on the host, after a wait for `s`: descend iff it rejected and no live item had a bad rho.
static int sig_rejected(const SigScratch& w, hipStream_t s, uint8_t& combined, bool& descend) {
    uint8_t two[2] = {0, 0};  // the bad-rho flag, the combined byte
    HALO_CHECK(copy_d2h(two, w.bad + w.nb, 2, s));
    combined = two[1];
    descend = !two[1] && !two[0];
    return HALO_OK;
}

// check_schnorr_args, and the k whose 2 k + 1 terms msm_device takes.
int sig_check_args(const char* call, int curve, const void* pk, const void* R, const void* s, const void* msgs,
                          size_t msg_len, size_t k, const void* out, bool& done) {
    HALO_CHECK(check_schnorr_args(call, curve, pk, R, s, true, msgs, msg_len, k, out, done));
    if (!done && k > (MSM_DEVICE_MAX_N - 1) / 2)
        return set_error(HALO_EINVAL, "%s: %zu signatures in one call (at most %zu)", call, k, (MSM_DEVICE_MAX_N - 1) / 2);
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_schnorr_batch_rho_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                          const void* d_msgs, size_t msg_len, size_t k, void* d_rho_out, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(sig_check_args("halo_schnorr_batch_rho_dev", curve, d_pk, d_R, d_s, d_msgs, msg_len, k, d_rho_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    SigScratch w;
    HALO_CHECK(sig_scratch(st, k, w));
    HALO_CHECK(sig_hash_live(st, curve, d_pk, d_R, d_msgs, msg_len, k, w, s));
    return sig_rho_device(st, curve, d_s, msg_len, k, w, d_rho_out, s);
}

extern "C" int halo_schnorr_batch_rho(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                                      const halo_fe_t* s_in, const halo_fe_t* msgs, size_t msg_len, size_t k,
                                      halo_fe_t* rho_out) {
    clear_error();
    bool done;
    HALO_CHECK(sig_check_args("halo_schnorr_batch_rho", curve, pk, R, s_in, msgs, msg_len, k, rho_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{pk, k * 64}, {R, k * 64}, {s_in, k * 32}, {msgs, msg_len * k * 32}}, s, at));
    SigScratch w;
    HALO_CHECK(sig_scratch(st, k, w));
    HALO_CHECK(sig_hash_live(st, curve, at[0], at[1], at[3], msg_len, k, w, s));
    HALO_CHECK(sig_rho_device(st, curve, at[2], msg_len, k, w, w.rho, s));
    return copy_d2h(rho_out, w.rho, k * 32, s);
}

extern "C" int halo_schnorr_verify_combined_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                                const void* d_msgs, size_t msg_len, size_t k, const void* d_rho, void* d_ok,
                                                void* d_combined, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(sig_check_args("halo_schnorr_verify_combined_dev", curve, d_pk, d_R, d_s, d_msgs, msg_len, k, d_ok, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    SigScratch w;
    return sig_combined_device(st, curve, d_pk, d_R, d_s, d_msgs, msg_len, k, d_rho, d_ok, d_combined, s, w);
}

extern "C" int halo_schnorr_verify_bisect_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                              const void* d_msgs, size_t msg_len, size_t k, const void* d_rho, void* d_ok,
                                              void* d_combined, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(sig_check_args("halo_schnorr_verify_bisect_dev", curve, d_pk, d_R, d_s, d_msgs, msg_len, k, d_ok, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    SigScratch w;
    HALO_CHECK(sig_combined_device(st, curve, d_pk, d_R, d_s, d_msgs, msg_len, k, d_rho, d_ok, d_combined, s, w));
    uint8_t combined;
    bool descend;
    HALO_CHECK(sig_rejected(w, s, combined, descend));
    if (!descend) return HALO_OK;  // accepted, or a live item's rho is bad: every byte stays 0
    return sig_bisect_device(st, curve, d_pk, d_R, d_s, k, w, d_ok, s);
}

extern "C" int halo_schnorr_verify_combined(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                                            const halo_fe_t* s_in, const halo_fe_t* msgs, size_t msg_len, size_t k,
                                            const halo_fe_t* rho, uint8_t* ok_out, uint8_t* combined_out) {
    clear_error();
    const char* call = "halo_schnorr_verify_combined";
    bool done;
    HALO_CHECK(sig_check_args(call, curve, pk, R, s_in, msgs, msg_len, k, ok_out, done));
    if (done) return HALO_OK;
    HALO_CHECK(check_rho(call, curve, rho, k));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{pk, k * 64}, {R, k * 64}, {s_in, k * 32}, {msgs, msg_len * k * 32},
                                          {rho, rho ? k * 32 : 0}}, s, at));
    HALO_CHECK(st->scratch[1].reserve(align256(k) + 1));
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    uint8_t* dcomb = dout + align256(k);
    SigScratch w;
    HALO_CHECK(sig_combined_device(st, curve, at[0], at[1], at[2], at[3], msg_len, k, at[4], dout, dcomb, s, w));
    uint8_t combined = 0;
    bool descend;
    HALO_CHECK(sig_rejected(w, s, combined, descend));
    if (!combined) {  // some live item fails: the exact verdicts, over the e already on the device
        if (descend && tuning(TUNE_SCHNORR_BISECT) > 0)
            HALO_CHECK(sig_bisect_device(st, curve, at[0], at[1], at[2], k, w, dout, s));
        else
            HALO_CHECK(schnorr_ladder_device(st, curve, at[0], at[1], at[2], st->schnorr_e.ptr, k, dout, s));
    }
    if (combined_out) *combined_out = combined;
    return copy_d2h(ok_out, dout, k, s);
}
