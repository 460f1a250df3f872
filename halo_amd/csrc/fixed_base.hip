// Fixed-base scalar multiplication of the generator G = (-1, 2), and on it the signer's half of
// crates/schnorr/src/lib.rs: generate_keypair's pk = sk G (lib.rs:41-43) and SecretKey::sign (lib.rs:49-66) with
// the random scalars given by the caller, as batches of independent items.
//
//   k_fb_bases / k_fb_multiples / k_fb_to_affine   build the comb table d 2^(C w) G once per device and curve
//   k_generator_mul     one lane per scalar: W table additions into an XYZZ accumulator (no doublings), then the
//                       workgroup's shared inversion (Montgomery's trick) and the WrappedPoint
//   k_schnorr_s         s = nonce + e sk in the scalar field
// The shape (window width, recoding, table index, grid) is fixed_base_plan.hpp's.
//
// NOT HARDENED AGAINST SIDE CHANNELS: the table is indexed by the secret's digits, zero digits skip their
// addition, and the exceptional cases of the addition branch.
#include "curve.hpp"
#include "dispatch.hpp"
#include "fixed_base.hpp"
#include "fixed_base_plan.hpp"
#include "host_scalar.hpp"
#include "runtime.hpp"
#include "schnorr.hpp"
#include "sponge_launch.hpp"
#include <vector>

namespace halo {

// ---------------------------------------------------------------------------------------------
// XYZZ -> affine with one inversion per workgroup
// ---------------------------------------------------------------------------------------------
struct FbNormLds {
    uint32_t pre[FB_THREADS][NLIMB], suf[FB_THREADS][NLIMB];
    uint32_t tinv[NLIMB];
};

template <class F>
HALO_DEV Fe<F> fb_lds_get(const uint32_t (&row)[NLIMB]) {
    Fe<F> o;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) o.v[l] = row[l];
    return o;
}
template <class F>
HALO_DEV void fb_lds_put(uint32_t (&row)[NLIMB], const Fe<F>& x) {
#pragma unroll
    for (int l = 0; l < NLIMB; l++) row[l] = x.v[l];
}

// The affine form of every lane's point, by Montgomery's trick as in k_ipa_fold: z = ZZ ZZZ per lane, inclusive
// prefix and suffix products over the workgroup in LDS, ONE inversion of the product of all z, and
// 1 / z_t = inv * pre[t - 1] * suf[t + 1].  An identity takes no part in the products (its z is 1) and comes out
// as (0, 0); a workgroup that holds only identities inverts nothing.  Every lane of the workgroup calls it
// (barriers); blockDim.x = FB_THREADS.
template <class F>
HALO_DEV Affine<F> fb_block_to_affine(const XYZZ<F>& acc, FbNormLds& lds) {
    const int tid = threadIdx.x;
    const bool id = xyzz_is_id(acc);
    Affine<F> r;
    r.x = fe_zero<F>();
    r.y = fe_zero<F>();
    if (!__syncthreads_or(!id)) return r;
    Fe<F> pv = id ? fe_one<F>() : fe_mul(acc.ZZ, acc.ZZZ), sv = pv;
    for (int off = 1; off < FB_THREADS; off <<= 1) {
        fb_lds_put(lds.pre[tid], pv);
        fb_lds_put(lds.suf[tid], sv);
        __syncthreads();
        if (tid >= off) pv = fe_mul(pv, fb_lds_get<F>(lds.pre[tid - off]));
        if (tid + off < FB_THREADS) sv = fe_mul(sv, fb_lds_get<F>(lds.suf[tid + off]));
        __syncthreads();
    }
    fb_lds_put(lds.pre[tid], pv);
    fb_lds_put(lds.suf[tid], sv);
    if (tid == FB_THREADS - 1) fb_lds_put(lds.tinv, fe_inv(pv));  // the product of all z: no factor is zero
    __syncthreads();
    if (id) return r;
    Fe<F> inv = fb_lds_get<F>(lds.tinv);
    if (tid > 0) inv = fe_mul(inv, fb_lds_get<F>(lds.pre[tid - 1]));
    if (tid + 1 < FB_THREADS) inv = fe_mul(inv, fb_lds_get<F>(lds.suf[tid + 1]));
    r.x = fe_mul(acc.X, fe_mul(inv, acc.ZZZ));  // X / ZZ
    r.y = fe_mul(acc.Y, fe_mul(inv, acc.ZZ));   // Y / ZZZ
    return r;
}

// ---------------------------------------------------------------------------------------------
// the table
// ---------------------------------------------------------------------------------------------
// 2^(C w) G for w < W, XYZZ (one lane: 256 - C dependent doublings, once per device and curve)
template <class Cv>
__global__ void k_fb_bases(uint4* out) {
    using F = typename Cv::Base;
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    Affine<F> G;
    G.x = fe_from_const<F>(Cv::K::GX);
    G.y = fe_from_const<F>(Cv::K::GY);
    XYZZ<F> v = xyzz_from_aff(G);
    for (int w = 0; w < FB_WINDOWS; w++) {
        xyzz_store(out + 8 * w, v);
        for (int j = 0; j < FB_C; j++) v = xyzz_dbl(v);
    }
}

// n XYZZ points -> internal affine (the table's format), FB_THREADS per workgroup
template <class Cv>
__global__ __launch_bounds__(FB_THREADS) void k_fb_to_affine(const uint4* __restrict__ in, size_t n, uint4* __restrict__ out) {
    using F = typename Cv::Base;
    __shared__ FbNormLds lds;
    const size_t i = (size_t)blockIdx.x * FB_THREADS + threadIdx.x;
    const XYZZ<F> p = i < n ? xyzz_load<F>(in + 8 * i) : xyzz_id<F>();
    const Affine<F> a = fb_block_to_affine(p, lds);
    if (i < n) aff_store(out + 4 * i, a);
}

// d 2^(C w) G at fb_table_index(w, d - 1), XYZZ: one lane per entry, double-and-add over the C bits of d
template <class Cv>
__global__ __launch_bounds__(FB_THREADS) void k_fb_multiples(const uint4* __restrict__ bases, uint4* __restrict__ out) {
    using F = typename Cv::Base;
    const uint32_t t = blockIdx.x * FB_THREADS + threadIdx.x;
    if (t >= (uint32_t)FB_ENTRIES) return;
    const uint32_t w = t / FB_HALF, d = t % FB_HALF + 1;
    const Affine<F> B = aff_load<F>(bases + 4 * w);
    XYZZ<F> acc = xyzz_id<F>();
#pragma unroll 1
    for (int bit = FB_C - 1; bit >= 0; bit--) {
        acc = xyzz_dbl(acc);
        if ((d >> bit) & 1u) acc = xyzz_madd(acc, B);
    }
    xyzz_store(out + 8 * t, acc);
}

// ---------------------------------------------------------------------------------------------
// the comb
// ---------------------------------------------------------------------------------------------
// Lane i < k takes a[i] -> out_a[i], lane k <= i < total takes b[i - k] -> out_b[i - k] (total = k or 2 k).
// Every wave walks the windows in the same order, least significant first, so one step's gathers fall into one
// window's slice of the table (FB_HALF entries).  The additions are xyzz_madd: the accumulator is the identity
// until the first nonzero digit, and it can meet the table entry itself (2^255 - r under c = 8 or 4: the
// windows below the top one sum to 2^254 mod r, the top digit's own multiple) or its negative.
template <class Cv>
__global__ __launch_bounds__(FB_THREADS) void k_generator_mul(const uint4* __restrict__ tab, const uint4* __restrict__ a,
                                                              uint4* __restrict__ out_a, const uint4* __restrict__ b,
                                                              uint4* __restrict__ out_b, size_t k, size_t total) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ FbNormLds lds;
    const size_t i = (size_t)blockIdx.x * FB_THREADS + threadIdx.x;
    const bool live = i < total, second = i >= k;
    const size_t j = second ? i - k : i;
    uint32_t w8[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // a lane past the batch multiplies by zero: the identity, no table read
    if (live) fe_ark_to_canonical_words<S>((second ? b : a) + 2 * j, w8);
    FbRecoder rc;
    rc.init(w8);
    XYZZ<F> acc = xyzz_id<F>();
#pragma unroll 1
    for (int w = 0; w < FB_WINDOWS; w++) {
        const uint32_t e = rc.next();
        if (e == DIGIT_NONE) continue;
        Affine<F> q = aff_load<F>(tab + 4 * (size_t)fb_table_index(w, e));
        if (fb_entry_negative(e)) q.y = fe_neg(q.y);
        acc = xyzz_madd(acc, q);
    }
    const Affine<F> r = fb_block_to_affine(acc, lds);
    if (live) aff_to_wrapped((second ? out_b : out_a) + 4 * j, r);
}

// s = nonce + e sk (lib.rs:63), ark scalars in and out
template <class Cv>
__global__ __launch_bounds__(256) void k_schnorr_s(const uint4* __restrict__ nonce, const uint4* __restrict__ e,
                                                   const uint4* __restrict__ sk, size_t k, uint4* __restrict__ out) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const Fe<S> es = fe_mul(fe_from_ark<S>(e + 2 * i), fe_from_ark<S>(sk + 2 * i));
    fe_to_ark(out + 2 * i, fe_add(fe_from_ark<S>(nonce + 2 * i), es));
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
int fixed_base_table(DeviceState* st, int curve, const void** d_tab) {
    DevBuf& tab = st->fixed_base_tab[curve];
    if (!tab.ptr) {
        // scratch of the build: the W bases in XYZZ and affine, every entry in XYZZ
        DevBuf tmp;
        const size_t bases_xyzz = (size_t)FB_WINDOWS * 128, bases_aff = (size_t)FB_WINDOWS * 64;
        HALO_CHECK(tmp.reserve(bases_xyzz + bases_aff + (size_t)FB_ENTRIES * 128));
        int rc = tab.reserve(FB_TABLE_BYTES);
        if (rc != HALO_OK) {
            tmp.release();
            return rc;
        }
        uint4* bx = tmp.as<uint4>();
        uint4* ba = bx + bases_xyzz / sizeof(uint4);
        uint4* ex = ba + bases_aff / sizeof(uint4);
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_fb_bases<Cv>, dim3(1), dim3(64), 0, 0, bx);
            hipLaunchKernelGGL(k_fb_to_affine<Cv>, dim3(fb_blocks(FB_WINDOWS)), dim3(FB_THREADS), 0, 0, (const uint4*)bx,
                               (size_t)FB_WINDOWS, ba);
            hipLaunchKernelGGL(k_fb_multiples<Cv>, dim3(fb_blocks(FB_ENTRIES)), dim3(FB_THREADS), 0, 0, (const uint4*)ba, ex);
            hipLaunchKernelGGL(k_fb_to_affine<Cv>, dim3(fb_blocks(FB_ENTRIES)), dim3(FB_THREADS), 0, 0, (const uint4*)ex,
                               (size_t)FB_ENTRIES, tab.as<uint4>());
        });
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(0);  // built once; later calls read it from any stream
        tmp.release();
        if (e != hipSuccess) {
            tab.release();
            return set_error(HALO_EDEVICE, "building the generator's fixed-base table failed: %s", hipGetErrorString(e));
        }
    }
    *d_tab = tab.ptr;
    return HALO_OK;
}

int generator_mul_device(DeviceState* st, int curve, const void* d_a, void* d_out_a, const void* d_b, void* d_out_b,
                         size_t k, hipStream_t s) {
    const void* tab;
    HALO_CHECK(fixed_base_table(st, curve, &tab));
    const size_t total = d_b ? 2 * k : k;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_generator_mul<Cv>, dim3(fb_blocks(total)), dim3(FB_THREADS), 0, s, (const uint4*)tab,
                           (const uint4*)d_a, (uint4*)d_out_a, (const uint4*)d_b, (uint4*)d_out_b, k, total);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// R = nonce G (and pk = sk G when d_pk is null), e = hash_message(pk, R, m), s = nonce + e sk.  st->mu and a
// ScratchUse of `s` held (st->schnorr_sign is shared by the calls on every stream).
static int schnorr_sign_device(DeviceState* st, int curve, const void* d_sk, const void* d_pk, const void* d_nonce,
                               const void* d_msgs, size_t msg_len, size_t k, void* d_R, void* d_s, hipStream_t s) {
    HALO_CHECK(st->schnorr_sign.reserve(k * 96));  // the derived keys (k x 64 B), then e (k x 32 B): nothing secret
    uint8_t* own_pk = st->schnorr_sign.as<uint8_t>();
    uint8_t* e = own_pk + k * 64;
    HALO_CHECK(generator_mul_device(st, curve, d_nonce, d_R, d_pk ? nullptr : d_sk, d_pk ? nullptr : own_pk, k, s));
    HALO_CHECK(schnorr_hash_device(st, curve, d_pk ? d_pk : own_pk, d_R, d_msgs, msg_len, k, e, nullptr, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_schnorr_s<Cv>, dim3(grid_for(k, 256)), dim3(256), 0, s, (const uint4*)d_nonce, (const uint4*)e,
                           (const uint4*)d_sk, k, (uint4*)d_s);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

static int check_mul_args(const char* call, int curve, const void* scalars, size_t k, const void* out, bool& done) {
    done = false;
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    if (!scalars || !out) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > SIZE_MAX / 128) return set_error(HALO_EINVAL, "%s: k overflows", call);
    return HALO_OK;
}

// pk may be null (derived).  Everything a signing entry point checks before the device lookup.
static int check_sign_args(const char* call, int curve, const void* sk, const void* nonce, const void* msgs, size_t msg_len,
                           size_t k, const void* R_out, const void* s_out, bool& done) {
    done = false;
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    if (!sk || !nonce || !R_out || !s_out || (msg_len && !msgs)) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > SIZE_MAX / 128) return set_error(HALO_EINVAL, "%s: k overflows", call);
    if (msg_len > (SIZE_MAX / 32) / k) return set_error(HALO_EINVAL, "%s: msg_len * k overflows", call);
    return require_poseidon_params(call, curve);
}

// The first entry of `x` that is not below the scalar modulus, as the error of `call`.
static int check_canonical(const char* call, const char* what, int curve, const halo_fe_t* x, size_t k) {
    const HostMont& M = scalar_mont(curve);
    for (size_t i = 0; i < k; i++)
        if (M.geq_p(x[i].l)) return set_error(HALO_EINVAL, "%s: %s[%zu] is not below the modulus", call, what, i);
    return HALO_OK;
}

// Zeroes the device staging of a host call's secrets on the call's stream and waits, however the call ends.  The
// staging is upload_parts' st->scratch[0]; the secrets are the leading `secret` rows of the call's table, so their
// bytes are [0, end of the last secret row) of that buffer.  arm() reserves the buffer that upload_parts then finds
// in place, before a byte is copied: a failure part-way through the upload is wiped like any other return.
struct SecretWipe {
    hipStream_t s;
    void* base = nullptr;
    size_t bytes = 0;
    int arm(DeviceState* st, const HostParts& parts, size_t secret) {
        if (secret == 0 || secret > parts.rows.size() || parts.rows[0].off != 0)
            return set_error(HALO_EINVAL, "SecretWipe: the secrets are not the leading rows of the table");
        HALO_CHECK(st->scratch[0].reserve(parts.total()));
        base = st->scratch[0].ptr;
        bytes = parts.rows[secret - 1].off + parts.rows[secret - 1].bytes;
        return HALO_OK;
    }
    ~SecretWipe() {
        if (base) (void)hipMemsetAsync(base, 0, bytes, s);
        (void)hipStreamSynchronize(s);
    }
};

}  // namespace halo

using namespace halo;

extern "C" int halo_generator_mul_batch(halo_curve_t curve, const halo_fe_t* scalars, size_t k, halo_wrapped_point_t* out) {
    clear_error();
    bool done;
    HALO_CHECK(check_mul_args("halo_generator_mul_batch", curve, scalars, k, out, done));
    if (done) return HALO_OK;
    HALO_CHECK(check_canonical("halo_generator_mul_batch", "scalars", curve, scalars, k));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const HostParts parts{{scalars, k * 32}};  // the secret row first: SecretWipe wipes the leading rows
    SecretWipe wipe{s};
    HALO_CHECK(wipe.arm(st, parts, 1));
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, parts, s, at));
    HALO_CHECK(st->scratch[1].reserve(k * 64));
    HALO_CHECK(generator_mul_device(st, curve, at[0], st->scratch[1].ptr, nullptr, nullptr, k, s));
    return copy_d2h(out, st->scratch[1].ptr, k * 64, s);
}

extern "C" int halo_generator_mul_batch_dev(halo_curve_t curve, const void* d_scalars, size_t k, void* d_out, void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(check_mul_args("halo_generator_mul_batch_dev", curve, d_scalars, k, d_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return generator_mul_device(st, curve, d_scalars, d_out, nullptr, nullptr, k, (hipStream_t)stream);
}

extern "C" int halo_schnorr_sign_batch(halo_curve_t curve, const halo_fe_t* sk, const halo_wrapped_point_t* pk,
                                       const halo_fe_t* nonce, const halo_fe_t* msgs, size_t msg_len, size_t k,
                                       halo_wrapped_point_t* R_out, halo_fe_t* s_out) {
    clear_error();
    bool done;
    HALO_CHECK(check_sign_args("halo_schnorr_sign_batch", curve, sk, nonce, msgs, msg_len, k, R_out, s_out, done));
    if (done) return HALO_OK;
    HALO_CHECK(check_canonical("halo_schnorr_sign_batch", "sk", curve, sk, k));
    HALO_CHECK(check_canonical("halo_schnorr_sign_batch", "nonce", curve, nonce, k));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    // sk and nonce first: SecretWipe wipes the leading rows, so a secret row must not move behind a public one
    const HostParts parts{{sk, k * 32}, {nonce, k * 32}, {pk, pk ? k * 64 : 0}, {msgs, msg_len * k * 32}};
    SecretWipe wipe{s};
    HALO_CHECK(wipe.arm(st, parts, 2));
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, parts, s, at));
    ScratchLayout out;
    const size_t o_R = out.take(k * 64), o_s = out.take(k * 32);
    HALO_CHECK(st->scratch[1].reserve(out.total()));
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    HALO_CHECK(schnorr_sign_device(st, curve, at[0], at[2], at[1], at[3], msg_len, k, dout + o_R, dout + o_s, s));
    HALO_CHECK(copy_d2h(R_out, dout + o_R, k * 64, s));
    return copy_d2h(s_out, dout + o_s, k * 32, s);
}

extern "C" int halo_schnorr_sign_batch_dev(halo_curve_t curve, const void* d_sk, const void* d_pk, const void* d_nonce,
                                           const void* d_msgs, size_t msg_len, size_t k, void* d_R_out, void* d_s_out,
                                           void* stream) {
    clear_error();
    bool done;
    HALO_CHECK(check_sign_args("halo_schnorr_sign_batch_dev", curve, d_sk, d_nonce, d_msgs, msg_len, k, d_R_out, d_s_out, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return schnorr_sign_device(st, curve, d_sk, d_pk, d_nonce, d_msgs, msg_len, k, d_R_out, d_s_out, s);
}
