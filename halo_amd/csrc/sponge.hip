// The Fiat-Shamir sponge of a Pasta curve as an object (crates/poseidon/src/outer_sponge.rs:11-100, Sponge<P>: new,
// absorb_g, absorb_g_affine, absorb_fq, absorb_fr, challenge, reset) behind the halo_sponge_* entry points: the
// transcripts the fused kernels (pcdl_fs.hip, plonk_verify.hip, pcdl_open_fs.hip, acc_fs.hip) do not walk, the
// prover's PLONK transcript first.
//
// A handle owns k sponges that advance in LOCKSTEP: every call applies one operation to all of them, on different
// data, so their (squeezed, n) mode is one value.  The host keeps it (sponge_plan.hpp) and hands it to each launch as
// a kernel argument: the branches around the permutation are uniform by construction, whatever the stored flags
// say.  The states live in device memory between calls, k x poseidon::STATE_U4 uint4 in Sponge::store's format: the
// same bytes in both lane layouts, so consecutive calls on a handle may run one or three lanes per sponge.
//
//   k_sponge_absorb      load (or a fresh / reset state), `count` base-field elements through the one absorb call, store
//   k_sponge_challenge   load, c squeezes through the one challenge call, each written as an ark scalar, store
//
// Lanes past the batch repeat its last sponge (they take part in the shuffles of the three-lane layout) and store
// nothing.  They may read that sponge's state while its own lanes, in another wave, store it; what they compute
// from it goes nowhere.
#include "sponge.hpp"

#include <map>
#include <memory>

#include "curve.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "outer_sponge.hpp"
#include "sponge_launch.hpp"

namespace halo {

// this lane belongs to sponge i of the batch (lane 63 of a three-lane wave to none)
template <int LANES>
HALO_DEV bool sponge_mine(size_t i, size_t k) {
    return i < k && (LANES == 1 || (threadIdx.x & 63u) != 63u);
}

// The walk: the label where init is SPONGE_FRESH, then the elements of the n items of row i.  squeezed, fill: the
// handle's mode before the call (false, 0 unless init is SPONGE_LOAD).
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_sponge_absorb(const uint32_t* __restrict__ params, uint4* __restrict__ state,
                                                       const uint4* __restrict__ in, int kind, size_t n, size_t k, int init,
                                                       int protocol, int squeezed, int fill) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    constexpr size_t NS = Sp::FR_ELEMENTS;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    uint4* mine_state = state + (size_t)poseidon::STATE_U4 * ic;
    Sp sp;
    if (init == SPONGE_LOAD)
        sp.load(tab, mine_state);
    else
        sp.init(tab);
    sp.inner.squeezed = squeezed != 0;
    sp.inner.n = fill;
    const size_t lead = init == SPONGE_FRESH ? 1 : 0;
    const size_t total = lead + n * (kind == SPONGE_G ? 2 : kind == SPONGE_FR ? NS : 1);
    const uint4* row = in + (kind == SPONGE_G ? 4 : 2) * n * ic;
#pragma unroll 1
    for (size_t e = 0; e < total; e++) {
        Fe<F> x;
        if (e < lead) {
            x = Sp::label_element(protocol);
        } else if (kind == SPONGE_G) {
            const size_t q = e - lead;
            x = Sp::g_element(row + 4 * (q >> 1), (int)(q & 1));
        } else if (kind == SPONGE_FR) {
            const size_t q = e - lead;
            uint32_t sw[8];
            fe_ark_to_canonical_words<S>(row + 2 * (q / NS), sw);
            x = Sp::fr_element(sw, (int)(q % NS));
        } else {
            x = fe_from_ark<F>(row + 2 * (e - lead));
        }
        sp.absorb(x);
    }
    sp.store(mine_state, sponge_mine<LANES>(i, k));
}

// out[i c + q] = challenge q of sponge i (ark)
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_sponge_challenge(const uint32_t* __restrict__ params, uint4* __restrict__ state,
                                                          size_t c, size_t k, int squeezed, int fill, uint4* __restrict__ out) {
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    uint4* mine_state = state + (size_t)poseidon::STATE_U4 * ic;
    poseidon::OuterSponge<Cv, LANES> sp;
    sp.load(tab, mine_state);
    sp.inner.squeezed = squeezed != 0;
    sp.inner.n = fill;
#pragma unroll 1
    for (size_t q = 0; q < c; q++) {
        uint32_t w[8];
        sp.challenge(w);
        if (writer && i < k) poseidon::scalar_words_to_ark<S>(out + 2 * (i * c + q), w);
    }
    sp.store(mine_state, sponge_mine<LANES>(i, k));
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int sponge_absorb_launch(SpongeHandle& h, int init, int kind, const void* d_in, size_t n, hipStream_t s) {
    DeviceState* st = h.st;
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(h.curve), &params));
    const SpongeMode before = init == SPONGE_LOAD ? h.mode : SpongeMode{false, 0};
    const size_t elements = (init == SPONGE_FRESH ? 1 : 0) + n * sponge_item_elements(kind, h.curve == HALO_PALLAS);
    const SpongeStep step = sponge_step(before, elements, 0);
    HALO_CHECK(SPONGE_LAUNCH(st, h.curve, Cv, L, h.k, "sponge_absorb", s, (k_sponge_absorb<Cv, L>), params, h.state.as<uint4>(),
                             (const uint4*)d_in, kind, n, h.k, init, h.protocol, before.squeezed ? 1 : 0, before.n));
    h.mode = step.mode;
    prof_count("sponge_permutations", h.k * step.permutations);
    return HALO_OK;
}

int sponge_challenge_launch(SpongeHandle& h, size_t n, void* d_out, hipStream_t s) {
    DeviceState* st = h.st;
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(h.curve), &params));
    const SpongeStep step = sponge_step(h.mode, 0, n);
    HALO_CHECK(SPONGE_LAUNCH(st, h.curve, Cv, L, h.k, "sponge_challenge", s, (k_sponge_challenge<Cv, L>), params,
                             h.state.as<uint4>(), n, h.k, h.mode.squeezed ? 1 : 0, h.mode.n, (uint4*)d_out));
    h.mode = step.mode;
    prof_count("sponge_permutations", h.k * step.permutations);
    return HALO_OK;
}

namespace {

// The live handles by id.  Ids count up and are never reused, so a stale id finds nothing: a handle is not an
// address that a later allocation could take over.  Read and written under the DeviceState lock of the caller's
// device (and g_sponge_mu, for processes that drive several devices).
std::mutex g_sponge_mu;
std::map<uint64_t, std::unique_ptr<SpongeHandle>> g_sponges;
uint64_t g_sponge_next = 1;

// The handle `id` on the device of st (st->mu held), or HALO_EINVAL naming `call`.
int sponge_find(const char* call, DeviceState* st, uint64_t id, SpongeHandle** out) {
    std::lock_guard<std::mutex> g(g_sponge_mu);
    const auto it = g_sponges.find(id);
    if (it == g_sponges.end())
        return set_error(HALO_EINVAL, "%s: no sponge with id %llu (never made, or freed)", call, (unsigned long long)id);
    if (it->second->st != st)
        return set_error(HALO_EINVAL, "%s: sponge %llu lives on device %d, the current device is %d", call,
                         (unsigned long long)id, it->second->st->device, st->device);
    *out = it->second.get();
    return HALO_OK;
}

size_t item_bytes(int kind) { return kind == SPONGE_G ? 64 : 32; }

// One absorb call.  host: `in` is host memory, checked, copied in, and the call waits; else a device pointer on `s`.
int sponge_absorb(const char* call, uint64_t id, int kind, const void* in, size_t n, bool host, hipStream_t s) {
    clear_error();
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SpongeHandle* h;
    HALO_CHECK(sponge_find(call, st, id, &h));
    if (n == 0) return HALO_OK;
    if (!in) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (n > (SIZE_MAX / 64) / h->k) return set_error(HALO_EINVAL, "%s: k * n overflows", call);
    HALO_CHECK(require_poseidon_params(call, h->curve));
    if (!host) return sponge_absorb_launch(*h, SPONGE_LOAD, kind, in, n, s);
    const size_t items = h->k * n;
    if (kind == SPONGE_FR) {
        if (!scalar_below(h->curve, (const halo_fe_t*)in, items))
            return set_error(HALO_EINVAL, "%s: a scalar is not below the modulus", call);
    } else {
        const HostMont& M = base_mont(h->curve);
        const halo_fe_t* x = (const halo_fe_t*)in;  // a WrappedPoint is two of them
        for (size_t j = 0; j < items * (kind == SPONGE_G ? 2 : 1); j++)
            if (M.geq_p(x[j].l))
                return set_error(HALO_EINVAL, "%s: %s is not below the base modulus", call,
                                 kind == SPONGE_G ? "a coordinate" : "an element");
    }
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(items * item_bytes(kind)));
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, in, items * item_bytes(kind), s));
    HALO_CHECK(sponge_absorb_launch(*h, SPONGE_LOAD, kind, st->scratch[0].ptr, n, s));
    HALO_HIP(hipStreamSynchronize(s));
    return HALO_OK;
}

int sponge_challenge(const char* call, uint64_t id, size_t n, void* out, bool host, hipStream_t s) {
    clear_error();
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SpongeHandle* h;
    HALO_CHECK(sponge_find(call, st, id, &h));
    if (n == 0) return HALO_OK;
    if (!out) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (n > (SIZE_MAX / 32) / h->k) return set_error(HALO_EINVAL, "%s: k * n overflows", call);
    HALO_CHECK(require_poseidon_params(call, h->curve));
    if (!host) return sponge_challenge_launch(*h, n, out, s);
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[1].reserve(h->k * n * 32));
    HALO_CHECK(sponge_challenge_launch(*h, n, st->scratch[1].ptr, s));
    return copy_d2h(out, st->scratch[1].ptr, h->k * n * 32, s);
}

}  // namespace
}  // namespace halo

using namespace halo;

extern "C" int halo_sponge_new(halo_curve_t curve, int protocol, size_t k, uint64_t* id) {
    clear_error();
    const char* call = "halo_sponge_new";
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (protocol < 0 || protocol > 3)
        return set_error(HALO_EINVAL, "%s: protocol %d is none of PCDL = 0, ASDL = 1, PLONK = 2, SIGNATURE = 3", call, protocol);
    if (k == 0) return set_error(HALO_EINVAL, "%s: k = 0 sponges", call);
    if (k > SIZE_MAX / (poseidon::STATE_U4 * sizeof(uint4))) return set_error(HALO_EINVAL, "%s: k overflows", call);
    if (!id) return set_error(HALO_EINVAL, "%s: null pointer", call);
    HALO_CHECK(require_poseidon_params(call, curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    std::unique_ptr<SpongeHandle> h(new SpongeHandle{st, (int)curve, protocol, k, {}, {false, 0}});
    HALO_CHECK(h->state.reserve(k * poseidon::STATE_U4 * sizeof(uint4)));
    // the state is complete before the id exists, whichever stream the first call on it names
    int rc = sponge_absorb_launch(*h, SPONGE_FRESH, SPONGE_FQ, nullptr, 0, 0);
    if (rc == HALO_OK && hipStreamSynchronize(0) != hipSuccess) rc = set_error(HALO_EDEVICE, "%s: the first launch failed", call);
    if (rc != HALO_OK) {
        h->state.release();
        return rc;
    }
    std::lock_guard<std::mutex> gm(g_sponge_mu);
    *id = g_sponge_next++;
    g_sponges[*id] = std::move(h);
    return HALO_OK;
}

extern "C" int halo_sponge_free(uint64_t id) {
    clear_error();
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SpongeHandle* h;
    HALO_CHECK(sponge_find("halo_sponge_free", st, id, &h));
    h->state.release();  // hipFree waits for the launches that still read it
    std::lock_guard<std::mutex> gm(g_sponge_mu);
    g_sponges.erase(id);
    return HALO_OK;
}

extern "C" int halo_sponge_reset(uint64_t id) {
    clear_error();
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SpongeHandle* h;
    HALO_CHECK(sponge_find("halo_sponge_reset", st, id, &h));
    HALO_CHECK(require_poseidon_params("halo_sponge_reset", h->curve));
    HALO_HIP(hipDeviceSynchronize());  // the callers' streams are done with the old state
    HALO_CHECK(sponge_absorb_launch(*h, SPONGE_RESET, SPONGE_FQ, nullptr, 0, 0));
    HALO_HIP(hipStreamSynchronize(0));
    return HALO_OK;
}

extern "C" int halo_sponge_absorb_g(uint64_t id, const halo_wrapped_point_t* pts, size_t n) {
    return sponge_absorb("halo_sponge_absorb_g", id, SPONGE_G, pts, n, true, 0);
}
extern "C" int halo_sponge_absorb_fr(uint64_t id, const halo_fe_t* xs, size_t n) {
    return sponge_absorb("halo_sponge_absorb_fr", id, SPONGE_FR, xs, n, true, 0);
}
extern "C" int halo_sponge_absorb_fq(uint64_t id, const halo_fe_t* xs, size_t n) {
    return sponge_absorb("halo_sponge_absorb_fq", id, SPONGE_FQ, xs, n, true, 0);
}
extern "C" int halo_sponge_challenge(uint64_t id, size_t n, halo_fe_t* out) {
    return sponge_challenge("halo_sponge_challenge", id, n, out, true, 0);
}

extern "C" int halo_sponge_absorb_g_dev(uint64_t id, const void* d_pts, size_t n, void* stream) {
    return sponge_absorb("halo_sponge_absorb_g_dev", id, SPONGE_G, d_pts, n, false, (hipStream_t)stream);
}
extern "C" int halo_sponge_absorb_fr_dev(uint64_t id, const void* d_xs, size_t n, void* stream) {
    return sponge_absorb("halo_sponge_absorb_fr_dev", id, SPONGE_FR, d_xs, n, false, (hipStream_t)stream);
}
extern "C" int halo_sponge_absorb_fq_dev(uint64_t id, const void* d_xs, size_t n, void* stream) {
    return sponge_absorb("halo_sponge_absorb_fq_dev", id, SPONGE_FQ, d_xs, n, false, (hipStream_t)stream);
}
extern "C" int halo_sponge_challenge_dev(uint64_t id, size_t n, void* d_out, void* stream) {
    return sponge_challenge("halo_sponge_challenge_dev", id, n, d_out, false, (hipStream_t)stream);
}
