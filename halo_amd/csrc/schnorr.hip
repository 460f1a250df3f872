// Batched Poseidon hashing and Schnorr signature verification (crates/poseidon/src/inner_sponge.rs,
// crates/poseidon/src/outer_sponge.rs:24-43,51-61,86-95, crates/schnorr/src/lib.rs:24-35,71-79): the
// reference's benchmark verifies 40 000 independent signatures (crates/plonk/src/main.rs:35-47), each
// one Poseidon hash of 5 + msg_len field elements and two scalar multiplications.
//
//   k_poseidon_hash / k_schnorr_hash   one sponge per lane or per three lanes (poseidon.hpp), the
//                                      constants staged in LDS per block
//   k_schnorr_verify                   one quad of lanes per signature: s G - e pk as ONE joint ladder
//                                      over the four GLV half-scalars (132 shared quad doublings, four
//                                      4-bit table additions per window), then - R and the identity test
#include "curve.hpp"
#include "dispatch.hpp"
#include "glv.hpp"
#include "host_scalar.hpp"
#include "poseidon.hpp"
#include "quad_ladder.hpp"
#include "runtime.hpp"
#include "schnorr.hpp"
#include "sponge_launch.hpp"
#include "tree.hpp"

#include <cstring>
#include <vector>

namespace halo {

// ---------------------------------------------------------------------------------------------
// hashing
// ---------------------------------------------------------------------------------------------
// k inner sponges: absorb row i of `in` (len ark elements), squeeze once.
template <class F, int LANES>
__global__ __launch_bounds__(256) void k_poseidon_hash(const uint32_t* __restrict__ params, const uint4* __restrict__ in,
                                                       size_t len, size_t k, uint4* __restrict__ out) {
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    poseidon::Sponge<F, LANES> sp;
    sp.init(tab);
    for (size_t j = 0; j < len; j++) sp.absorb(fe_from_ark<F>(in + 2 * (ic * len + j)));
    const Fe<F> v = sp.squeeze();
    if (writer && i < k) fe_to_ark(out + 2 * i, v);
}

// hash_message (schnorr/src/lib.rs:24-35): Sponge::new(SIGNATURE = 3), absorb_g_affine([pk, R]) (x then
// y, the identity as (0, 0): the WrappedPoint's own limbs), absorb_fq(message), challenge().  The
// squeezed base-field element becomes the scalar unchanged when the base field is the smaller one
// (Pallas) and shifted right by one bit otherwise (Vesta; outer_sponge.rs:86-95).  e_ark: the scalar in
// ark form; e_words: its canonical integer (the verification kernel's input); either may be null.
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_schnorr_hash(const uint32_t* __restrict__ params, const uint4* __restrict__ pk,
                                                      const uint4* __restrict__ R, const uint4* __restrict__ msgs,
                                                      size_t msg_len, size_t k, uint4* __restrict__ e_ark,
                                                      uint4* __restrict__ e_words) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    poseidon::Sponge<F, LANES> sp;
    sp.init(tab);
    const Fe<F> one = fe_one<F>();
    const Fe<F> label = fe_add(one, fe_add(one, one));  // Protocols::SIGNATURE = 3
    // element 0: the label; 1..4: pk.x, pk.y, R.x, R.y; then the message (one loop: one copy of the permutation)
#pragma unroll 1
    for (size_t j = 0; j < 5 + msg_len; j++) {
        const uint4* src = j < 3 ? pk + 4 * ic + (j == 2 ? 2 : 0) : j < 5 ? R + 4 * ic + (j == 4 ? 2 : 0)
                                                                        : msgs + 2 * (ic * msg_len + (j - 5));
        const Fe<F> x = fe_from_ark<F>(src);
        sp.absorb(j == 0 ? label : x);
    }
    const Fe<F> v = sp.squeeze();
    // canonical integer: the Montgomery product with the plain integer 1 divides R' out
    Fe<F> raw1 = fe_zero<F>();
    raw1.v[0] = 1;
    uint32_t w[8];
    fe_pack(fe_canon(fe_mul(v, raw1)), w);
    constexpr bool shift = Cv::Scalar::MODULUS64[1] < Cv::Base::MODULUS64[1];  // the moduli differ in limb 1 first
    if (shift) {
#pragma unroll
        for (int q = 0; q < 8; q++) w[q] = (w[q] >> 1) | (q < 7 ? w[q + 1] << 31 : 0u);
    }
    if (!(writer && i < k)) return;
    if (e_words) {
        e_words[2 * i] = make_uint4(w[0], w[1], w[2], w[3]);
        e_words[2 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    }
    if (e_ark) fe_to_ark(e_ark + 2 * i, fe_mul(fe_unpack<S>(w), fe_from_const<S>(S::R2)));
}

// ---------------------------------------------------------------------------------------------
// verification
// ---------------------------------------------------------------------------------------------
constexpr int VERIFY_THREADS = 64;                    // one wave: 16 signatures
constexpr int GTAB_U4 = 16 * 8;                       // d G at d - 1, phi(d G) at 8 + d - 1 (1 <= d <= 8): XYZZ, 128 B each
constexpr int PKTAB_U4 = QUAD_TAB_U4;                 // d pk at d - 1 (1 <= d <= 8) per quad
constexpr size_t VERIFY_LDS = (size_t)(GTAB_U4 + (VERIFY_THREADS / 4) * PKTAB_U4) * sizeof(uint4);  // 18 KB: 8 blocks per CU

template <class Cv>
__global__ void k_schnorr_gtab(uint4* tab) {
    using F = typename Cv::Base;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Affine<F> G;
    G.x = fe_from_const<F>(Cv::K::GX);
    G.y = fe_from_const<F>(Cv::K::GY);
    const Fe<F> beta = fe_from_const<F>(Cv::K::BETA);
    XYZZ<F> v = xyzz_from_aff(G);
    for (int d = 1; d <= 8; d++) {
        xyzz_store(tab + 8 * (d - 1), v);
        XYZZ<F> ph = v;
        ph.X = fe_mul(v.X, beta);
        xyzz_store(tab + 8 * (8 + d - 1), ph);
        v = xyzz_madd(v, G);
    }
}

// PublicKey::verify (schnorr/src/lib.rs:71-79): s G == R + e pk, tested as s G - e pk - R == identity in
// XYZZ (no inversion).  One aligned quad of lanes per signature (every lane of the quad holds the
// same values; tree.hpp's quad doubling / addition).  With s = s1 + lambda s2 and e = e1 + lambda e2
// (glv.hpp, |.| < 2^128) the sum is one ladder over 33 signed four-bit windows: four quad doublings,
// then +-(d G), +-phi(d G) from the block's copy of the fixed-base table and -+(d pk), -+phi(d pk) from
// the quad's own table of pk, 1 <= d <= 8 (phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ), applied as the
// entry is read).  Signed digits halve the tables: 18 KB of LDS per block, two waves per SIMD.
// A pk or R that is neither the identity nor on the curve gives 0.  Quads of one wave stay in
// lockstep: an addition is skipped only when it is trivial for every quad.
template <class Cv>
__global__ __launch_bounds__(VERIFY_THREADS) void k_schnorr_verify(const uint4* __restrict__ pk, const uint4* __restrict__ R,
                                                                   const uint4* __restrict__ s, const uint4* __restrict__ e_words,
                                                                   const uint4* __restrict__ gtab, size_t k,
                                                                   uint8_t* __restrict__ ok) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    extern __shared__ uint4 lds[];
    uint4* gt = lds;
    uint4* pt = lds + GTAB_U4 + PKTAB_U4 * (threadIdx.x >> 2);
    for (int j = threadIdx.x; j < GTAB_U4; j += VERIFY_THREADS) gt[j] = gtab[j];
    const uint32_t lane = threadIdx.x & 63u, role = lane & 3u, s1 = lane & ~3u;
    const size_t i = ((size_t)blockIdx.x * VERIFY_THREADS + threadIdx.x) >> 2;
    const size_t ic = i < k ? i : k - 1;  // quads past the batch repeat its last item (no store): every lane reaches the barriers
    Affine<F> P = aff_from_wrapped<F>(pk + 4 * ic);
    const Affine<F> Rp = aff_from_wrapped<F>(R + 4 * ic);
    const Fe<F> b = fe_from_const<F>(Cv::K::B);
    const bool valid = aff_on_curve_or_id(P, b) && aff_on_curve_or_id(Rp, b);
    if (!valid) P.x = P.y = fe_zero<F>();  // the ladder then runs over the identity; the verdict is 0 below
    bool ns1, ns2, ne1, ne2;
    SignedDigits gs1, gs2, ge1, ge2;
    {
        uint32_t sw[8], ew[8], k1[5], k2[5];
        fe_ark_to_canonical_words<S>(s + 2 * ic, sw);
        words_from_u4(e_words + 2 * ic, ew);
        glv::decompose<typename Cv::K>(sw, ns1, k1, ns2, k2);
        gs1.recode(k1);
        gs2.recode(k2);
        glv::decompose<typename Cv::K>(ew, ne1, k1, ne2, k2);
        ge1.recode(k1);
        ge2.recode(k2);
    }
    QUAD_TABLE_BUILD(F, pt, P, role, s1);  // (its first barrier: the block's copy of the G table is complete)
    const Fe<F> beta = fe_from_const<F>(Cv::K::BETA);
    XYZZ<F> acc = xyzz_id<F>();
#pragma unroll 1
    for (int w = 32; w >= 0; w--) {  // 33 windows cover 132 bits
        if (w != 32)
            for (int q = 0; q < 4; q++) acc = xyzz_dbl_quad(acc);
        bool neg;
        uint32_t d = gs1.next(neg);
        XYZZ<F> t = xyzz_load<F>(gt + 8 * (d ? d - 1 : 0));
        if (ns1 != neg) t.Y = fe_neg(t.Y);
        acc = quad_add(acc, t, d == 0, role, s1);
        d = gs2.next(neg);
        t = xyzz_load<F>(gt + 8 * (8 + (d ? d - 1 : 0)));
        if (ns2 != neg) t.Y = fe_neg(t.Y);
        acc = quad_add(acc, t, d == 0, role, s1);
        d = ge1.next(neg);  // - e1 pk
        t = xyzz_load<F>(pt + 8 * (d ? d - 1 : 0));
        if (ne1 == neg) t.Y = fe_neg(t.Y);
        acc = quad_add(acc, t, d == 0, role, s1);
        d = ge2.next(neg);  // - e2 phi(pk)
        t = xyzz_load<F>(pt + 8 * (d ? d - 1 : 0));
        t.X = fe_mul(t.X, beta);
        if (ne2 == neg) t.Y = fe_neg(t.Y);
        acc = quad_add(acc, t, d == 0, role, s1);
    }
    acc = xyzz_madd(acc, aff_neg(Rp));
    if (role == 0 && i < k) ok[i] = (valid && xyzz_is_id(acc)) ? 1 : 0;
}


// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// The installed parameters of each field, as the kernels read them (limb form); process-wide, copied to
// a device when a call there finds its copy older.
struct PoseidonParams {
    std::mutex mu;
    uint64_t ver[2] = {0, 0};  // 0: not set
    uint32_t tab[2][poseidon::TABLE_WORDS];
};
static PoseidonParams g_poseidon;
static uint64_t g_poseidon_next = 1;

// ark Montgomery limbs (a 2^256 mod p, canonical) -> the kernels' form (a 2^261 mod p as nine 29-bit
// limbs): five modular doublings on the host.  False when the input is not below the modulus of M.
static bool ark_to_limbs(const HostMont& M, const halo_fe_t& in, uint32_t* out) {
    if (M.geq_p(in.l)) return false;
    uint64_t x[4] = {in.l[0], in.l[1], in.l[2], in.l[3]};
    for (int d = 0; d < 5; d++) M.dbl(x);
    for (int i = 0; i < NLIMB; i++) {
        const int bit = i * LIMB_BITS, j = bit >> 6, sh = bit & 63;
        uint64_t v = x[j] >> sh;
        if (sh + LIMB_BITS > 64 && j + 1 < 4) v |= x[j + 1] << (64 - sh);
        out[i] = (uint32_t)v & LIMB_MASK;
    }
    return true;
}

bool poseidon_params_set(int field) {
    std::lock_guard<std::mutex> g(g_poseidon.mu);
    return g_poseidon.ver[field] != 0;
}

// This device's copy of the parameters of `field` (st->mu held).
int poseidon_device_params(DeviceState* st, int field, const uint32_t** out) {
    std::lock_guard<std::mutex> g(g_poseidon.mu);
    if (st->poseidon_ver[field] != g_poseidon.ver[field]) {
        HALO_CHECK(st->poseidon[field].reserve(sizeof(g_poseidon.tab[field])));
        HALO_HIP(hipDeviceSynchronize());  // no kernel still reads the previous version
        HALO_HIP(hipMemcpy(st->poseidon[field].ptr, g_poseidon.tab[field], sizeof(g_poseidon.tab[field]),
                           hipMemcpyHostToDevice));
        st->poseidon_ver[field] = g_poseidon.ver[field];
    }
    *out = st->poseidon[field].as<const uint32_t>();
    return HALO_OK;
}

static int poseidon_hash_device(DeviceState* st, int field, const void* d_in, size_t len, size_t k, void* d_out,
                                hipStream_t s) {
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, field, &params));
    return SPONGE_LAUNCH_FIELD(st, field, F, L, k, nullptr, s, (k_poseidon_hash<F, L>), params, (const uint4*)d_in, len, k,
                               (uint4*)d_out);
}

int schnorr_hash_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_msgs, size_t msg_len,
                        size_t k, void* d_e_ark, void* d_e_words, hipStream_t s) {
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(curve), &params));
    return SPONGE_LAUNCH(st, curve, Cv, L, k, nullptr, s, (k_schnorr_hash<Cv, L>), params, (const uint4*)d_pk, (const uint4*)d_R,
                         (const uint4*)d_msgs, msg_len, k, (uint4*)d_e_ark, (uint4*)d_e_words);
}

// The ladder over challenges already on the device (e_words: k_schnorr_hash's canonical words).  st->mu held.
int schnorr_ladder_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s,
                          const void* d_e_words, size_t k, void* d_ok, hipStream_t s) {
    DevBuf& gt = st->schnorr_gtab[curve];
    if (!gt.ptr) {
        HALO_CHECK(gt.reserve(GTAB_U4 * sizeof(uint4)));
        DISPATCH_CURVE(curve, Cv, { hipLaunchKernelGGL(k_schnorr_gtab<Cv>, dim3(1), dim3(64), 0, 0, gt.as<uint4>()); });
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(0);  // built once; later calls read it from any stream
        if (e != hipSuccess) {
            gt.release();
            return set_error(HALO_EDEVICE, "halo_schnorr_verify_batch: building the generator table failed: %s",
                             hipGetErrorString(e));
        }
    }
    const unsigned blocks = (unsigned)((4 * k + VERIFY_THREADS - 1) / VERIFY_THREADS);
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_schnorr_verify<Cv>, dim3(blocks), dim3(VERIFY_THREADS), VERIFY_LDS, s, (const uint4*)d_pk,
                           (const uint4*)d_R, (const uint4*)d_s, (const uint4*)d_e_words, gt.as<const uint4>(), k,
                           (uint8_t*)d_ok);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// Hash into st->schnorr_e, then the ladder.  st->mu and a ScratchUse of `s` held by the caller.
static int schnorr_verify_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s,
                                 const void* d_msgs, size_t msg_len, size_t k, void* d_ok, hipStream_t s) {
    HALO_CHECK(st->schnorr_e.reserve(k * 32));
    HALO_CHECK(schnorr_hash_device(st, curve, d_pk, d_R, d_msgs, msg_len, k, nullptr, st->schnorr_e.ptr, s));
    return schnorr_ladder_device(st, curve, d_pk, d_R, d_s, st->schnorr_e.ptr, k, d_ok, s);
}

int check_schnorr_args(const char* call, int curve, const void* pk, const void* R, const void* s, bool need_s,
                       const void* msgs, size_t msg_len, size_t k, const void* out, bool& done) {
    done = false;
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    if (!pk || !R || (need_s && !s) || !out || (msg_len && !msgs)) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (msg_len > (SIZE_MAX / 32) / k) return set_error(HALO_EINVAL, "%s: msg_len * k overflows", call);
    return require_poseidon_params(call, curve);
}

}  // namespace halo

using namespace halo;

extern "C" int halo_poseidon_set_params(halo_field_t field, const halo_fe_t* mds, const halo_fe_t* rc) {
    clear_error();
    if (!valid_field(field) || !mds || !rc) return set_error(HALO_EINVAL, "halo_poseidon_set_params: invalid argument");
    static uint32_t tmp[poseidon::TABLE_WORDS];
    std::lock_guard<std::mutex> g(g_poseidon.mu);
    const HostMont& M = scalar_mont(field == HALO_FP ? HALO_PALLAS : HALO_VESTA);  // Fp is Pallas's scalar field
    for (int i = 0; i < poseidon::N_CONST; i++) {
        const halo_fe_t& x = i < 9 ? mds[i] : rc[i - 9];
        if (!ark_to_limbs(M, x, tmp + i * NLIMB))
            return set_error(HALO_EINVAL, "halo_poseidon_set_params: constant %d is not a canonical field element", i);
    }
    memcpy(g_poseidon.tab[field], tmp, sizeof(tmp));
    g_poseidon.ver[field] = g_poseidon_next++;
    return HALO_OK;
}

static int check_hash_args(const char* call, halo_field_t field, const void* in, size_t len, size_t k, const void* out,
                           bool& done) {
    done = false;
    if (!valid_field(field)) return set_error(HALO_EINVAL, "%s: unknown field", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    if (!out || (len && !in)) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (len > (SIZE_MAX / 32) / k) return set_error(HALO_EINVAL, "%s: len * k overflows", call);
    if (!poseidon_params_set(field))
        return set_error(HALO_EINVAL, "%s: no Poseidon parameters for this field (halo_poseidon_set_params)", call);
    return HALO_OK;
}

extern "C" int halo_poseidon_hash_batch(halo_field_t field, const halo_fe_t* in, size_t len, size_t k, halo_fe_t* out) {
    clear_error();
    bool done;
    HALO_CHECK(check_hash_args("halo_poseidon_hash_batch", field, in, len, k, out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{in, len * k * 32}}, s, at));
    HALO_CHECK(st->scratch[1].reserve(k * 32));
    HALO_CHECK(poseidon_hash_device(st, field, at[0], len, k, st->scratch[1].ptr, s));
    return copy_d2h(out, st->scratch[1].ptr, k * 32, s);
}

extern "C" int halo_poseidon_hash_batch_dev(halo_field_t field, const void* d_in, size_t len, size_t k, void* d_out,
                                            void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(check_hash_args("halo_poseidon_hash_batch_dev", field, d_in, len, k, d_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return poseidon_hash_device(st, field, d_in, len, k, d_out, (hipStream_t)stream);
}

extern "C" int halo_schnorr_hash_batch(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                                       const halo_fe_t* msgs, size_t msg_len, size_t k, halo_fe_t* e_out) {
    clear_error();
    bool done;
    HALO_CHECK(check_schnorr_args("halo_schnorr_hash_batch", curve, pk, R, nullptr, false, msgs, msg_len, k, e_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{pk, k * 64}, {R, k * 64}, {msgs, msg_len * k * 32}}, s, at));
    HALO_CHECK(st->scratch[1].reserve(k * 32));
    HALO_CHECK(schnorr_hash_device(st, curve, at[0], at[1], at[2], msg_len, k, st->scratch[1].ptr, nullptr, s));
    return copy_d2h(e_out, st->scratch[1].ptr, k * 32, s);
}

extern "C" int halo_schnorr_hash_batch_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_msgs,
                                           size_t msg_len, size_t k, void* d_e_out, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(check_schnorr_args("halo_schnorr_hash_batch_dev", curve, d_pk, d_R, nullptr, false, d_msgs, msg_len, k,
                                  d_e_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return schnorr_hash_device(st, curve, d_pk, d_R, d_msgs, msg_len, k, d_e_out, nullptr, (hipStream_t)stream);
}

extern "C" int halo_schnorr_verify_batch(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                                         const halo_fe_t* s_in, const halo_fe_t* msgs, size_t msg_len, size_t k,
                                         uint8_t* ok_out) {
    clear_error();
    bool done;
    HALO_CHECK(check_schnorr_args("halo_schnorr_verify_batch", curve, pk, R, s_in, true, msgs, msg_len, k, ok_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{pk, k * 64}, {R, k * 64}, {s_in, k * 32}, {msgs, msg_len * k * 32}}, s, at));
    HALO_CHECK(st->scratch[1].reserve(k));
    HALO_CHECK(schnorr_verify_device(st, curve, at[0], at[1], at[2], at[3], msg_len, k, st->scratch[1].ptr, s));
    return copy_d2h(ok_out, st->scratch[1].ptr, k, s);
}

extern "C" int halo_schnorr_verify_batch_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                             const void* d_msgs, size_t msg_len, size_t k, void* d_ok, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(check_schnorr_args("halo_schnorr_verify_batch_dev", curve, d_pk, d_R, d_s, true, d_msgs, msg_len, k, d_ok,
                                  done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);  // st->schnorr_e is shared by the calls on every stream
    return schnorr_verify_device(st, curve, d_pk, d_R, d_s, d_msgs, msg_len, k, d_ok, s);
}
