// The weights of the combined batched decider derived from the batch itself by Fiat-Shamir, on the device (DESIGN
// §4.9 "derived weights"; tests/rho_ref.py restates it).  The decider's statement for instance i is
// "U_i == Commit(Gs[0..d], h(xi_{i,1..lg n}))", so the batch is d, k, the live mask and the pairs (U_i, xi_{i,1..lg n});
// xi_{i,0} is not read by the decider and is not hashed.  All hashing is the curve's own sponge (outer_sponge.hpp),
// under three labels that continue the reference's 0..3 and are this backend's own (rho_plan.hpp): the reference
// has no batched decider.
//
//   k_rho_leaves   leaf_i = squeeze of Sponge(BATCH_LEAF).absorb_g(U_i).absorb_fr(xi_{i,1}) ... absorb_fr(xi_{i,lg n}),
//                  a base-field element; the element 0, with nothing read, for an instance that is not live
//   k_rho_level    level l + 1 [j] = N(level l [2 j], level l [2 j + 1]), or level l [2 j] unchanged when it is alone;
//                  N(a, b): a fresh unlabelled inner sponge absorbs a, b and squeezes once.  ceil(lg k) launches
//                  between two buffers, until the root remains
//   k_rho_weights  seed = squeeze of Sponge(seed label) after root, k and a third integer (recomputed by every
//                  sponge: two permutations, cheaper than a launch); rho_i = challenge of Sponge(weight label) after
//                  seed, i, zero replaced by one; rho_i = 0 for an instance that is not live.  The decider's labels
//                  are BATCH_SEED and BATCH_WEIGHT and its third integer is d
// The tree and the weights are one driver, rho_derive_device, which the weights of a combined Schnorr batch share
// under labels of their own (schnorr_combined.hip).
//
// One sponge per instance / node in either lane layout.  Each kernel walks its transcript as an element stream
// through ONE absorb call and ONE squeeze call (outer_sponge.hpp says why).
#include "curve.hpp"
#include "decider.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "outer_sponge.hpp"
#include "rho_plan.hpp"
#include "sponge_launch.hpp"

namespace halo {

template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_rho_leaves(const uint32_t* __restrict__ params, const uint4* __restrict__ xis,
                                                    const uint4* __restrict__ U, const uint8_t* __restrict__ live,
                                                    unsigned lg, size_t k, uint4* __restrict__ leaves) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    constexpr unsigned NS = Sp::FR_ELEMENTS;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    const bool on = !live || live[ic] != 0;  // the row of an instance that is not live is not read
    const uint4* row = xis + 2 * (size_t)(lg + 1) * ic;
    Sp sp;
    sp.init(tab);
    const unsigned total = 3 + NS * lg;
#pragma unroll 1
    for (unsigned e = 0; e < total; e++) {
        Fe<F> x = fe_zero<F>();
        if (e == 0) {
            x = Sp::label_element(RHO_BATCH_LEAF);
        } else if (!on) {
            // nothing is read; what this sponge hashes is discarded
        } else if (e < 3) {
            x = Sp::g_element(U + 4 * ic, (int)e - 1);
        } else {
            const unsigned q = e - 3;
            uint32_t sw[8];
            fe_ark_to_canonical_words<S>(row + 2 * (1 + q / NS), sw);
            x = Sp::fr_element(sw, (int)(q % NS));
        }
        sp.absorb(x);
    }
    const Fe<F> leaf = fe_select(on, sp.inner.squeeze(), fe_zero<F>());
    if (writer && i < k) fe_store(leaves + 2 * i, leaf);
}

// out[j] for j < ceil(count / 2)
template <class F, int LANES>
__global__ __launch_bounds__(256) void k_rho_level(const uint32_t* __restrict__ params, const uint4* __restrict__ in, size_t count,
                                                   uint4* __restrict__ out) {
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    const size_t nodes = (count + 1) / 2;
    SPONGE_PROLOGUE(LANES, params, tab, nodes, j, jc, writer);
    const bool pair = 2 * jc + 1 < count;
    const Fe<F> a = fe_load<F>(in + 2 * (2 * jc));
    const Fe<F> b = pair ? fe_load<F>(in + 2 * (2 * jc + 1)) : fe_zero<F>();
    poseidon::Sponge<F, LANES> sp;
    sp.init(tab);
#pragma unroll 1
    for (int e = 0; e < 2; e++) sp.absorb(e == 0 ? a : b);
    const Fe<F> node = fe_select(pair, sp.squeeze(), a);
    if (writer && j < nodes) fe_store(out + 2 * j, node);
}

template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_rho_weights(const uint32_t* __restrict__ params, const uint4* __restrict__ root, size_t k,
                                                     int seed_label, int weight_label, size_t third,
                                                     const uint8_t* __restrict__ live, uint4* __restrict__ rho) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    Sp sp;
    Fe<F> out = fe_load<F>(root);  // the root, then the seed, then the squeezed weight
#pragma unroll 1
    for (int phase = 0; phase < 2; phase++) {
        sp.init(tab);
        const int total = phase == 0 ? 4 : 3;
#pragma unroll 1
        for (int e = 0; e < total; e++) {
            Fe<F> x;
            if (e == 0)
                x = Sp::label_element(phase == 0 ? seed_label : weight_label);
            else if (e == 1)
                x = out;
            else
                x = poseidon::fe_from_u64<F>(phase == 1 ? (uint64_t)ic : e == 2 ? (uint64_t)k : (uint64_t)third);
            sp.absorb(x);
        }
        out = sp.inner.squeeze();
    }
    uint32_t w[8];
    Sp::challenge_words(out, w);
    rho_zero_becomes_one(w);
    if (live && live[ic] == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = 0;
    }
    if (writer && i < k) poseidon::scalar_words_to_ark<S>(rho + 2 * i, w);
}

int rho_buffers(DevBuf& work, size_t k, uint4* (&buf)[2]) {
    ScratchLayout lay;
    const size_t o_ping = lay.take(k * 32), o_pong = lay.take(rho_next_level(k) * 32);
    HALO_CHECK(work.reserve(lay.total()));
    uint8_t* base = work.as<uint8_t>();
    buf[0] = (uint4*)(base + o_ping), buf[1] = (uint4*)(base + o_pong);
    return HALO_OK;
}

int rho_derive_device(DeviceState* st, int curve, const uint32_t* params, uint4* const (&buf)[2], size_t k, const RhoWeights& w,
                      const void* live, void* rho_out, hipStream_t s) {
    int cur = 0;
    for (size_t count = k; count > 1; count = rho_next_level(count), cur ^= 1)
        HALO_CHECK(SPONGE_LAUNCH(st, curve, Cv, L, rho_next_level(count), "rho_level", s, (k_rho_level<typename Cv::Base, L>), params,
                                 (const uint4*)buf[cur], count, buf[cur ^ 1]));
    return SPONGE_LAUNCH(st, curve, Cv, L, k, w.profile, s, (k_rho_weights<Cv, L>), params, (const uint4*)buf[cur], k, w.seed_label,
                         w.weight_label, w.third, (const uint8_t*)live, (uint4*)rho_out);
}

int decide_rho_device(DeviceState* st, int curve, size_t d, size_t k, const void* xis, const void* U, const void* live,
                      void* rho_out, hipStream_t s) {
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(curve), &params));
    uint4* buf[2];
    HALO_CHECK(rho_buffers(st->decide_rho[1], k, buf));
    StageScope stage("decide_rho", s);
    HALO_CHECK(SPONGE_LAUNCH(st, curve, Cv, L, k, "rho_leaves", s, (k_rho_leaves<Cv, L>), params, (const uint4*)xis, (const uint4*)U,
                             (const uint8_t*)live, ilog2(d + 1), k, buf[0]));
    HALO_CHECK(rho_derive_device(st, curve, params, buf, k, RhoWeights{RHO_BATCH_SEED, RHO_BATCH_WEIGHT, d, "rho_weights"}, live,
                                 rho_out, s));
    stage.end();
    return HALO_OK;
}

int decide_rho_weights(DeviceState* st, DecideCall& a, hipStream_t s) {
    if (!a.derive || a.rho || a.k < 2) return HALO_OK;
    HALO_CHECK(st->decide_rho[0].reserve(a.k * 32));
    HALO_CHECK(decide_rho_device(st, a.curve, a.d, a.k, a.xis, a.U, a.live, st->decide_rho[0].ptr, s));
    a.rho = st->decide_rho[0].ptr;
    return HALO_OK;
}

// Everything that needs no device; done: an empty batch.  (The rules of halo_pcdl_decide_batch.)
static int check_rho_args(const char* call, int curve, size_t d, size_t k, const void* xis, const void* U, const void* out,
                          bool& done) {
    done = false;
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    const size_t n = d + 1;
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    if (ilog2(n) > 28) return set_error(HALO_EINVAL, "%s: n (%zu) out of range", call, n);
    if (!xis || !U || !out) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > LINCOMB_MAX_ITEMS / 4) return set_error(HALO_EINVAL, "%s: %zu instances in one call", call, k);
    return require_poseidon_params(call, curve);
}

}  // namespace halo

using namespace halo;

extern "C" int halo_pcdl_decide_rho_dev(halo_curve_t curve, size_t d, size_t k, const void* d_xis, const void* d_U,
                                        const void* d_live, void* d_rho_out, void* stream) {
    clear_error();
    const char* call = "halo_pcdl_decide_rho_dev";
    bool done;
    HALO_CHECK(check_rho_args(call, curve, d, k, d_xis, d_U, d_rho_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return decide_rho_device(st, curve, d, k, d_xis, d_U, d_live, d_rho_out, s);
}

extern "C" int halo_pcdl_decide_rho(halo_curve_t curve, size_t d, size_t k, const halo_fe_t* xis, const halo_wrapped_point_t* U,
                                    const uint8_t* live, halo_fe_t* rho_out) {
    clear_error();
    const char* call = "halo_pcdl_decide_rho";
    bool done;
    HALO_CHECK(check_rho_args(call, curve, d, k, xis, U, rho_out, done));
    if (done) return HALO_OK;
    const size_t row = ilog2(d + 1) + 1;
    for (size_t j = 0; j < k * row; j++)
        if (!scalar_below(curve, xis[j]))
            return set_error(HALO_EINVAL, "%s: xi_%zu of instance %zu is not below the modulus", call, j % row, j / row);
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{xis, k * row * 32}, {U, k * 64}, {live, live ? k : 0}}, s, at));
    HALO_CHECK(st->decide_rho[0].reserve(k * 32));
    HALO_CHECK(decide_rho_device(st, curve, d, k, at[0], at[1], at[2], st->decide_rho[0].ptr, s));
    return copy_d2h(rho_out, st->decide_rho[0].ptr, k * 32, s);
}
