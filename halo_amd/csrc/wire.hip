// The wire format of the reference's proof objects on gfx950 (ark-serialize 0.5, compressed mode):
// field square roots, compressed points and canonical scalars <-> the library's WrappedPoint / ark Montgomery
// arrays, and serialized pcdl Instances <-> the argument arrays of halo_pcdl_check_fs_batch.
//
// One lane handles one item (a 33-byte point record, a 32-byte scalar) with plain byte loads at any byte offset: a
// point costs one square root (field_sqrt.hpp, ~840 dependent multiplications), next to which its 33 loads are
// nothing, so there is no LDS staging.  The layout of an instance is wire_plan.hpp's, shared with the host walk.
#include <vector>

#include "dispatch.hpp"
#include "field_sqrt.hpp"
#include "points.hpp"
#include "runtime.hpp"
#include "wire_plan.hpp"

namespace halo {

constexpr int WIRE_THREADS = 64;
constexpr uint8_t WIRE_FLAG_NEG = 0x80, WIRE_FLAG_INF = 0x40;

// ---------------------------------------------------------------------------------------------
// items
// ---------------------------------------------------------------------------------------------
HALO_DEV void load_words(const uint8_t* p, uint32_t (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++)
        w[j] = (uint32_t)p[4 * j] | (uint32_t)p[4 * j + 1] << 8 | (uint32_t)p[4 * j + 2] << 16 | (uint32_t)p[4 * j + 3] << 24;
}
HALO_DEV void store_words(uint8_t* p, const uint32_t (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        p[4 * j] = (uint8_t)w[j];
        p[4 * j + 1] = (uint8_t)(w[j] >> 8);
        p[4 * j + 2] = (uint8_t)(w[j] >> 16);
        p[4 * j + 3] = (uint8_t)(w[j] >> 24);
    }
}
HALO_DEV uint64_t load_u64(const uint8_t* p) {
    uint64_t x = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) x = x << 8 | p[j];
    return x;
}
HALO_DEV void store_u64(uint8_t* p, uint64_t x) {
#pragma unroll
    for (int j = 0; j < 8; j++) p[j] = (uint8_t)(x >> (8 * j));
}

// What an undecodable point is written as: (0, 1), on neither curve, so every batch verifier rejects the instance
// that holds it and only that one.
template <class F>
HALO_DEV void store_sentinel(uint4* out) {
    Affine<F> s;
    s.x = fe_zero<F>();
    s.y = fe_one<F>();
    aff_to_wrapped(out, s);
}
HALO_DEV void store_zero_point(uint4* out) {
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = make_uint4(0, 0, 0, 0);
}
HALO_DEV void store_zero_scalar(uint4* out) { out[0] = out[1] = make_uint4(0, 0, 0, 0); }

// One 33-byte record -> WrappedPoint.  Refused (sentinel written, false returned): x not below the modulus, bits
// 0..5 of the flag byte set, both flags set, infinity with x != 0, x^3 + 5 not a square (x = 0 among them: 5 is a
// non-residue of both fields).  Every lane runs the root, whatever its record, so a wave stays in step.
template <class Cv>
HALO_DEV bool decode_point(const uint8_t* rec, uint4* out) {
    using F = typename Cv::Base;
    uint32_t w[8];
    load_words(rec, w);
    const uint8_t flags = rec[32];
    const bool inf = flags & WIRE_FLAG_INF, neg = flags & WIRE_FLAG_NEG;
    bool good = !(flags & 0x3f) && !(inf && neg) && words_below_modulus<F>(w);
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) any |= w[j];
    Affine<F> a;
    a.x = fe_from_canonical_words<F>(w);
    bool sq;
    a.y = fe_sqrt(fe_add(fe_mul(fe_sqr(a.x), a.x), fe_from_const<F>(Cv::K::B)), sq);
    uint32_t yw[8];
    fe_to_canonical_words(a.y, yw);
    if (words_above_half<F>(yw) != neg) a.y = fe_neg(a.y);
    good = good && (inf ? any == 0 : sq);
    if (!good)
        store_sentinel<F>(out);
    else if (inf)
        store_zero_point(out);
    else
        aff_to_wrapped(out, a);
    return good;
}

// WrappedPoint -> one 33-byte record.  A point that is neither (0, 0) nor on the curve has no encoding: false, and
// the record written is x = 0 with BOTH flags, which no decoder accepts.
template <class Cv>
HALO_DEV bool encode_point(const uint4* in, uint8_t* rec) {
    using F = typename Cv::Base;
    const Affine<F> a = aff_from_wrapped<F>(in);
    const bool id = aff_is_id(a);
    const bool on = fe_eq(fe_sqr(a.y), fe_add(fe_mul(fe_sqr(a.x), a.x), fe_from_const<F>(Cv::K::B)));
    uint32_t xw[8], yw[8];
    fe_to_canonical_words(a.x, xw);
    fe_to_canonical_words(a.y, yw);
    const bool good = id || on;
    if (!good || id) {
#pragma unroll
        for (int j = 0; j < 8; j++) xw[j] = 0;
    }
    store_words(rec, xw);
    rec[32] = !good ? (uint8_t)(WIRE_FLAG_INF | WIRE_FLAG_NEG) : id ? WIRE_FLAG_INF : words_above_half<F>(yw) ? WIRE_FLAG_NEG : 0;
    return good;
}

// 32 canonical bytes -> ark Montgomery scalar; not below the modulus: zero written, false.
template <class S>
HALO_DEV bool decode_scalar(const uint8_t* rec, uint4* out) {
    uint32_t w[8];
    load_words(rec, w);
    const bool good = words_below_modulus<S>(w);
    if (good)
        fe_to_ark(out, fe_from_canonical_words<S>(w));
    else
        store_zero_scalar(out);
    return good;
}
template <class S>
HALO_DEV void encode_scalar(const uint4* in, uint8_t* rec) {
    uint32_t w[8];
    fe_ark_to_canonical_words<S>(in, w);
    store_words(rec, w);
}

// ---------------------------------------------------------------------------------------------
// batch kernels over consecutive items
// ---------------------------------------------------------------------------------------------
// out[i]: the smaller root of in[i] as a canonical integer (ark Montgomery form, like every field element of the
// ABI), is_square[i] = 1; zero and 0 for a non-residue
template <class F>
__global__ __launch_bounds__(WIRE_THREADS) void k_fe_sqrt(const uint4* in, size_t k, uint4* out, uint8_t* is_square) {
    const size_t i = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x;
    if (i >= k) return;
    bool sq;
    Fe<F> r = fe_sqrt(fe_from_ark<F>(in + 2 * i), sq);
    uint32_t w[8];
    fe_to_canonical_words(r, w);
    if (words_above_half<F>(w)) r = fe_neg(r);
    fe_to_ark(out + 2 * i, r);
    if (is_square) is_square[i] = sq;
}

template <class Cv>
__global__ __launch_bounds__(WIRE_THREADS) void k_points_decompress(const uint8_t* bytes, size_t k, uint4* out, uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x;
    if (i >= k) return;
    const bool good = decode_point<Cv>(bytes + WIRE_POINT * i, out + 4 * i);
    if (ok) ok[i] = good;
}

template <class Cv>
__global__ __launch_bounds__(WIRE_THREADS) void k_points_compress(const uint4* pts, size_t k, uint8_t* bytes, uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x;
    if (i >= k) return;
    const bool good = encode_point<Cv>(pts + 4 * i, bytes + WIRE_POINT * i);
    if (ok) ok[i] = good;
}

template <class S>
__global__ __launch_bounds__(WIRE_THREADS) void k_scalars_from_bytes(const uint8_t* bytes, size_t k, uint4* out, uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x;
    if (i >= k) return;
    const bool good = decode_scalar<S>(bytes + WIRE_SCALAR * i, out + 2 * i);
    if (ok) ok[i] = good;
}

template <class S>
__global__ __launch_bounds__(WIRE_THREADS) void k_scalars_to_bytes(const uint4* in, size_t k, uint8_t* bytes) {
    const size_t i = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x;
    if (i >= k) return;
    encode_scalar<S>(in + 2 * i, bytes + WIRE_SCALAR * i);
}

// ---------------------------------------------------------------------------------------------
// Instances.  The arrays are those of halo_pcdl_check_fs_batch, in its order.
// ---------------------------------------------------------------------------------------------
struct WireArrays {
    uint4 *C, *z, *v, *Ls, *Rs, *U, *c;
    uint8_t* hiding;
    uint4 *C_bar, *w_prime;
    uint8_t* ok;
};

// items of one instance: 2 lg + 3 points (C, Ls, Rs, U, C_bar), then 4 scalars (z, v, c, w_prime)
constexpr size_t wire_items(size_t lg) { return 2 * lg + 7; }

// One lane per instance: the structure the host walk checks, checked again where the offsets cannot be trusted
// (halo_pcdl_instances_decode_dev): the instance lies inside [0, len), its d is the call's, Ls and Rs hold lg
// points, the tags are 0 / 1 and equal.  Nothing at or past `len` is read.  ok[i] = 1 and hiding[i] = the tag, or
// both 0.
__global__ __launch_bounds__(WIRE_THREADS) void k_wire_headers(const uint8_t* bytes, size_t len, const uint64_t* offsets,
                                                               size_t k, uint64_t d, size_t lg, uint8_t* hiding, uint8_t* ok) {
    const size_t i = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x;
    if (i >= k) return;
    const WireLayout lay = wire_layout(lg);
    const uint64_t o = offsets[i];
    bool good = o <= len && wire_instance_size(lg, false) <= len - o;
    uint8_t tag = 0;
    if (good) {
        const uint8_t* q = bytes + o;
        tag = q[lay.tag_cbar];
        good = load_u64(q + lay.d) == d && load_u64(q + lay.ls_len) == lg && load_u64(q + lay.rs_len) == lg && tag <= 1;
        if (good && tag) good = wire_instance_size(lg, true) <= len - o;
        if (good) good = q[lay.tag_cbar + 1 + (tag ? WIRE_POINT : 0)] == tag;
    }
    hiding[i] = good ? tag : 0;
    ok[i] = good;
}

// One lane per item.  pass 0 decodes the items of the instances whose header held and clears ok[i] where an item
// does not decode; pass 1 rewrites every item of an instance with ok[i] = 0 (sentinel points, zero scalars), so
// the verifier that follows rejects that instance alone and meets no scalar it would refuse.
template <class Cv>
__global__ __launch_bounds__(WIRE_THREADS) void k_wire_items(const uint8_t* bytes, const uint64_t* offsets, size_t k, size_t lg,
                                                             WireArrays a, int pass) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    const size_t g = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x, T = wire_items(lg);
    if (g >= k * T) return;
    const size_t i = g / T, t = g % T;
    const bool live = a.ok[i];  // pass 0: may already be 0 from another lane's failure, which is the final answer
    if (pass == 1 && live) return;
    const WireLayout lay = wire_layout(lg);
    const bool hid = a.hiding[i];
    const uint8_t* q = bytes + (live ? offsets[i] : 0);  // not read unless live
    const size_t npts = 2 * lg + 3;
    if (t < npts) {
        uint4* out;
        size_t at;
        bool present = true;
        if (t == 0) {
            out = a.C + 4 * i, at = lay.C;
        } else if (t <= lg) {
            out = a.Ls + 4 * (i * lg + (t - 1)), at = lay.ls + WIRE_POINT * (t - 1);
        } else if (t <= 2 * lg) {
            out = a.Rs + 4 * (i * lg + (t - 1 - lg)), at = lay.rs + WIRE_POINT * (t - 1 - lg);
        } else if (t == 2 * lg + 1) {
            out = a.U + 4 * i, at = lay.U;
        } else {
            out = a.C_bar + 4 * i, at = lay.tag_cbar + 1, present = hid;
        }
        if (!live) {
            store_sentinel<F>(out);
        } else if (!present) {
            store_zero_point(out);
        } else if (!decode_point<Cv>(q + at, out)) {
            a.ok[i] = 0;
        }
    } else {
        const size_t s = t - npts;
        uint4* out = (s == 0 ? a.z : s == 1 ? a.v : s == 2 ? a.c : a.w_prime) + 2 * i;
        const size_t at = s == 0 ? lay.z : s == 1 ? lay.v : s == 2 ? lay.c : lay.tag_cbar + 2 + WIRE_POINT;
        if (!live || (s == 3 && !hid)) {
            store_zero_scalar(out);
        } else if (!decode_scalar<S>(q + at, out)) {
            a.ok[i] = 0;
        }
    }
}

// The inverse: one lane per item writes its bytes at offsets[i]; the lane of C also writes d, the two lengths and
// the tags.  ok[i] (set to 1 before the launch) is cleared by a point without an encoding.
template <class Cv>
__global__ __launch_bounds__(WIRE_THREADS) void k_wire_encode(uint8_t* bytes, const uint64_t* offsets, size_t k, uint64_t d,
                                                              size_t lg, WireArrays a) {
    using S = typename Cv::Scalar;
    const size_t g = (size_t)blockIdx.x * WIRE_THREADS + threadIdx.x, T = wire_items(lg);
    if (g >= k * T) return;
    const size_t i = g / T, t = g % T;
    const WireLayout lay = wire_layout(lg);
    const bool hid = a.hiding && a.hiding[i];
    uint8_t* q = bytes + offsets[i];
    const size_t npts = 2 * lg + 3;
    if (t < npts) {
        const uint4* in;
        size_t at;
        if (t == 0) {
            in = a.C + 4 * i, at = lay.C;
            store_u64(q + lay.d, d);
            store_u64(q + lay.ls_len, lg);
            store_u64(q + lay.rs_len, lg);
            q[lay.tag_cbar] = hid;
            q[lay.tag_cbar + 1 + (hid ? WIRE_POINT : 0)] = hid;
        } else if (t <= lg) {
            in = a.Ls + 4 * (i * lg + (t - 1)), at = lay.ls + WIRE_POINT * (t - 1);
        } else if (t <= 2 * lg) {
            in = a.Rs + 4 * (i * lg + (t - 1 - lg)), at = lay.rs + WIRE_POINT * (t - 1 - lg);
        } else if (t == 2 * lg + 1) {
            in = a.U + 4 * i, at = lay.U;
        } else {
            if (!hid) return;
            in = a.C_bar + 4 * i, at = lay.tag_cbar + 1;
        }
        if (!encode_point<Cv>(in, q + at)) a.ok[i] = 0;
    } else {
        const size_t s = t - npts;
        if (s == 3 && !hid) return;
        const uint4* in = (s == 0 ? a.z : s == 1 ? a.v : s == 2 ? a.c : a.w_prime) + 2 * i;
        encode_scalar<S>(in, q + (s == 0 ? lay.z : s == 1 ? lay.v : s == 2 ? lay.c : lay.tag_cbar + 2 + WIRE_POINT));
    }
}

// ---------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------
static int launch_sqrt(int field, const void* in, size_t k, void* out, void* sq, hipStream_t s) {
    if (!k) return HALO_OK;
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_fe_sqrt<F>, dim3(grid_for(k, WIRE_THREADS)), dim3(WIRE_THREADS), 0, s, (const uint4*)in, k,
                           (uint4*)out, (uint8_t*)sq);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
static int launch_decompress(int curve, const void* bytes, size_t k, void* out, void* ok, hipStream_t s) {
    if (!k) return HALO_OK;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_points_decompress<Cv>, dim3(grid_for(k, WIRE_THREADS)), dim3(WIRE_THREADS), 0, s,
                           (const uint8_t*)bytes, k, (uint4*)out, (uint8_t*)ok);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
static int launch_compress(int curve, const void* pts, size_t k, void* bytes, void* ok, hipStream_t s) {
    if (!k) return HALO_OK;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_points_compress<Cv>, dim3(grid_for(k, WIRE_THREADS)), dim3(WIRE_THREADS), 0, s, (const uint4*)pts,
                           k, (uint8_t*)bytes, (uint8_t*)ok);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
static int launch_scalars_from(int field, const void* bytes, size_t k, void* out, void* ok, hipStream_t s) {
    if (!k) return HALO_OK;
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_scalars_from_bytes<F>, dim3(grid_for(k, WIRE_THREADS)), dim3(WIRE_THREADS), 0, s,
                           (const uint8_t*)bytes, k, (uint4*)out, (uint8_t*)ok);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
static int launch_scalars_to(int field, const void* in, size_t k, void* bytes, hipStream_t s) {
    if (!k) return HALO_OK;
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_scalars_to_bytes<F>, dim3(grid_for(k, WIRE_THREADS)), dim3(WIRE_THREADS), 0, s, (const uint4*)in, k,
                           (uint8_t*)bytes);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// d + 1 = 2^lg, as every pcdl entry point requires
static int check_d(size_t d, size_t& lg) {
    const size_t n = d + 1;
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    lg = ilog2(n);
    return HALO_OK;
}
static int check_grid(const char* call, size_t k, size_t lg) {
    if (k > (size_t)0x7fffffff * WIRE_THREADS / wire_items(lg))
        return set_error(HALO_EINVAL, "%s: %zu instances of %zu items are more than one launch covers", call, k, wire_items(lg));
    return HALO_OK;
}

static int launch_decode(int curve, size_t d, size_t lg, size_t k, const void* bytes, size_t len, const void* offsets,
                         const WireArrays& a, hipStream_t s) {
    if (!k) return HALO_OK;
    hipLaunchKernelGGL(k_wire_headers, dim3(grid_for(k, WIRE_THREADS)), dim3(WIRE_THREADS), 0, s, (const uint8_t*)bytes, len,
                       (const uint64_t*)offsets, k, (uint64_t)d, lg, a.hiding, a.ok);
    const unsigned grid = grid_for(k * wire_items(lg), WIRE_THREADS);
    for (int pass = 0; pass < 2; pass++)
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_wire_items<Cv>, dim3(grid), dim3(WIRE_THREADS), 0, s, (const uint8_t*)bytes,
                               (const uint64_t*)offsets, k, lg, a, pass);
        });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The eleven arrays of a call as parts of one device buffer: C z v Ls Rs U c hiding C_bar w_prime ok
struct WireParts {
    size_t bytes[11], off[11];
    ScratchLayout lay;
    WireParts(size_t k, size_t lg) {
        const size_t b[11] = {64 * k, 32 * k, 32 * k, 64 * k * lg, 64 * k * lg, 64 * k, 32 * k, k, 64 * k, 32 * k, k};
        for (int j = 0; j < 11; j++) bytes[j] = b[j], off[j] = lay.take(b[j]);
    }
    WireArrays at(uint8_t* base) const {
        WireArrays a;
        a.C = (uint4*)(base + off[0]), a.z = (uint4*)(base + off[1]), a.v = (uint4*)(base + off[2]);
        a.Ls = (uint4*)(base + off[3]), a.Rs = (uint4*)(base + off[4]), a.U = (uint4*)(base + off[5]);
        a.c = (uint4*)(base + off[6]), a.hiding = base + off[7], a.C_bar = (uint4*)(base + off[8]);
        a.w_prime = (uint4*)(base + off[9]), a.ok = base + off[10];
        return a;
    }
};

}  // namespace halo

using namespace halo;

// A host call over one input and up to two outputs of consecutive items: the input goes to scratch, `run` is
// launched on the null stream, the outputs come back.
template <class Run>
static int host_items(const void* in, size_t in_bytes, void* out0, size_t out0_bytes, void* out1,
                      size_t out1_bytes, Run run) {
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    ScratchLayout lay;
    const size_t o_in = lay.take(in_bytes), o0 = lay.take(out0_bytes), o1 = lay.take(out1_bytes);
    HALO_CHECK(st->scratch[0].reserve(lay.total()));
    uint8_t* base = st->scratch[0].as<uint8_t>();
    HALO_CHECK(copy_h2d(base + o_in, in, in_bytes, s));
    HALO_CHECK(run(base + o_in, base + o0, base + o1, s));
    if (out1) HALO_CHECK(copy_d2h(out1, base + o1, out1_bytes, s));
    return copy_d2h(out0, base + o0, out0_bytes, s);
}

extern "C" int halo_fe_sqrt_batch(halo_field_t field, const halo_fe_t* in, size_t k, halo_fe_t* out, uint8_t* is_square) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!k) return HALO_OK;
    if (!in || !out) return set_error(HALO_EINVAL, "halo_fe_sqrt_batch: null buffer");
    return host_items(in, 32 * k, out, 32 * k, is_square, k,
                      [&](void* i, void* o, void* f, hipStream_t s) { return launch_sqrt(field, i, k, o, f, s); });
}

extern "C" int halo_fe_sqrt_batch_dev(halo_field_t field, const void* d_in, size_t k, void* d_out, void* d_is_square,
                                      void* stream) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!k) return HALO_OK;
    if (!d_in || !d_out) return set_error(HALO_EINVAL, "halo_fe_sqrt_batch_dev: null buffer");
    return launch_sqrt(field, d_in, k, d_out, d_is_square, (hipStream_t)stream);
}

extern "C" int halo_points_decompress(halo_curve_t curve, const uint8_t* bytes, size_t k, halo_wrapped_point_t* out_pts,
                                      uint8_t* ok) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!k) return HALO_OK;
    if (!bytes || !out_pts) return set_error(HALO_EINVAL, "halo_points_decompress: null buffer");
    return host_items(bytes, WIRE_POINT * k, out_pts, 64 * k, ok, k,
                      [&](void* i, void* o, void* f, hipStream_t s) { return launch_decompress(curve, i, k, o, f, s); });
}

extern "C" int halo_points_decompress_dev(halo_curve_t curve, const void* d_bytes, size_t k, void* d_out_pts, void* d_ok,
                                          void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!k) return HALO_OK;
    if (!d_bytes || !d_out_pts) return set_error(HALO_EINVAL, "halo_points_decompress_dev: null buffer");
    return launch_decompress(curve, d_bytes, k, d_out_pts, d_ok, (hipStream_t)stream);
}

extern "C" int halo_points_compress(halo_curve_t curve, const halo_wrapped_point_t* pts, size_t k, uint8_t* out_bytes) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!k) return HALO_OK;
    if (!pts || !out_bytes) return set_error(HALO_EINVAL, "halo_points_compress: null buffer");
    std::vector<uint8_t> ok(k);
    HALO_CHECK(host_items(pts, 64 * k, out_bytes, WIRE_POINT * k, ok.data(), k,
                          [&](void* i, void* o, void* f, hipStream_t s) { return launch_compress(curve, i, k, o, f, s); }));
    for (size_t i = 0; i < k; i++)
        if (!ok[i]) return set_error(HALO_EINVAL, "halo_points_compress: point %zu is neither (0, 0) nor on the curve", i);
    return HALO_OK;
}

extern "C" int halo_points_compress_dev(halo_curve_t curve, const void* d_pts, size_t k, void* d_out_bytes, void* d_ok,
                                        void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!k) return HALO_OK;
    if (!d_pts || !d_out_bytes) return set_error(HALO_EINVAL, "halo_points_compress_dev: null buffer");
    return launch_compress(curve, d_pts, k, d_out_bytes, d_ok, (hipStream_t)stream);
}

extern "C" int halo_scalars_from_bytes(halo_field_t field, const uint8_t* bytes, size_t k, halo_fe_t* out, uint8_t* ok) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!k) return HALO_OK;
    if (!bytes || !out) return set_error(HALO_EINVAL, "halo_scalars_from_bytes: null buffer");
    return host_items(bytes, WIRE_SCALAR * k, out, 32 * k, ok, k,
                      [&](void* i, void* o, void* f, hipStream_t s) { return launch_scalars_from(field, i, k, o, f, s); });
}

extern "C" int halo_scalars_from_bytes_dev(halo_field_t field, const void* d_bytes, size_t k, void* d_out, void* d_ok,
                                           void* stream) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!k) return HALO_OK;
    if (!d_bytes || !d_out) return set_error(HALO_EINVAL, "halo_scalars_from_bytes_dev: null buffer");
    return launch_scalars_from(field, d_bytes, k, d_out, d_ok, (hipStream_t)stream);
}

extern "C" int halo_scalars_to_bytes(halo_field_t field, const halo_fe_t* in, size_t k, uint8_t* out_bytes) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!k) return HALO_OK;
    if (!in || !out_bytes) return set_error(HALO_EINVAL, "halo_scalars_to_bytes: null buffer");
    return host_items(in, 32 * k, out_bytes, WIRE_SCALAR * k, nullptr, 0,
                      [&](void* i, void* o, void*, hipStream_t s) { return launch_scalars_to(field, i, k, o, s); });
}

extern "C" int halo_scalars_to_bytes_dev(halo_field_t field, const void* d_in, size_t k, void* d_out_bytes, void* stream) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!k) return HALO_OK;
    if (!d_in || !d_out_bytes) return set_error(HALO_EINVAL, "halo_scalars_to_bytes_dev: null buffer");
    return launch_scalars_to(field, d_in, k, d_out_bytes, (hipStream_t)stream);
}

// ---- instances ------------------------------------------------------------------------------
static int wire_error(const char* call, int status, size_t index) {
    const int code = status == WIRE_NOT_POW2 ? HALO_ENOTPOW2 : HALO_EINVAL;
    return set_error(code, "%s: instance %zu: %s", call, index, wire_status_message(status));
}

extern "C" int halo_pcdl_instances_walk(const uint8_t* bytes, size_t len, int vec_prefix, size_t max_k, uint64_t* offsets,
                                        uint64_t* ds, uint8_t* hiding, size_t* k_out) {
    clear_error();
    if (!k_out || (len && !bytes) || (max_k && (!offsets || !ds || !hiding)))
        return set_error(HALO_EINVAL, "halo_pcdl_instances_walk: null buffer");
    std::vector<WireInstance> w(max_k);
    size_t bad = 0;
    const uint8_t none = 0;
    const int rc = wire_walk(len ? bytes : &none, len, vec_prefix != 0, max_k, w.data(), k_out, &bad);
    if (rc) {
        *k_out = 0;
        return wire_error("halo_pcdl_instances_walk", rc, bad);
    }
    for (size_t i = 0; i < *k_out; i++) offsets[i] = w[i].offset, ds[i] = w[i].d, hiding[i] = w[i].hiding;
    if (offsets) offsets[*k_out] = *k_out ? w[*k_out - 1].end : (vec_prefix ? WIRE_U64 : 0);
    return HALO_OK;
}

static bool null_arrays(const void* const (&p)[11], size_t lg) {
    for (int j = 0; j < 11; j++)
        if (!p[j] && !(lg == 0 && (j == 3 || j == 4))) return true;
    return false;
}

extern "C" int halo_pcdl_instances_decode(halo_curve_t curve, size_t d, size_t k, const uint8_t* bytes, size_t len,
        const uint64_t* offsets, halo_wrapped_point_t* C, halo_fe_t* z, halo_fe_t* v, halo_wrapped_point_t* Ls,
        halo_wrapped_point_t* Rs, halo_wrapped_point_t* U, halo_fe_t* c, uint8_t* hiding, halo_wrapped_point_t* C_bar,
        halo_fe_t* w_prime, uint8_t* ok) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    size_t lg;
    HALO_CHECK(check_d(d, lg));
    if (!k) return HALO_OK;
    void* const host[11] = {C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, ok};
    const void* const chk[11] = {C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, ok};
    if (!bytes || !offsets || null_arrays(chk, lg)) return set_error(HALO_EINVAL, "halo_pcdl_instances_decode: null buffer");
    HALO_CHECK(check_grid("halo_pcdl_instances_decode", k, lg));
    // the structure of every instance, on the host, before anything is copied
    for (size_t i = 0; i < k; i++) {
        if (offsets[i] > len) return wire_error("halo_pcdl_instances_decode", WIRE_TRUNCATED, i);
        WireCursor cur{bytes, len, (size_t)offsets[i]};
        WireInstance w;
        const int rc = wire_walk_instance(cur, w);
        if (rc) return wire_error("halo_pcdl_instances_decode", rc, i);
        if (w.d != d)
            return set_error(HALO_EINVAL, "halo_pcdl_instances_decode: instance %zu has d = %llu, the call is for d = %zu", i,
                             (unsigned long long)w.d, d);
    }
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    WireParts parts(k, lg);
    const size_t o_bytes = parts.lay.take(len), o_off = parts.lay.take(8 * k);
    HALO_CHECK(st->scratch[0].reserve(parts.lay.total()));
    uint8_t* base = st->scratch[0].as<uint8_t>();
    HALO_CHECK(copy_h2d(base + o_bytes, bytes, len, s));
    HALO_CHECK(copy_h2d(base + o_off, offsets, 8 * k, s));
    HALO_CHECK(launch_decode(curve, d, lg, k, base + o_bytes, len, base + o_off, parts.at(base), s));
    for (int j = 0; j < 11; j++) HALO_CHECK(copy_d2h(host[j], base + parts.off[j], parts.bytes[j], s));
    return HALO_OK;
}

extern "C" int halo_pcdl_instances_decode_dev(halo_curve_t curve, size_t d, size_t k, const void* d_bytes, size_t len,
        const void* d_offsets, void* d_C, void* d_z, void* d_v, void* d_Ls, void* d_Rs, void* d_U, void* d_c, void* d_hiding,
        void* d_C_bar, void* d_w_prime, void* d_ok, void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    size_t lg;
    HALO_CHECK(check_d(d, lg));
    if (!k) return HALO_OK;
    const void* const chk[11] = {d_C, d_z, d_v, d_Ls, d_Rs, d_U, d_c, d_hiding, d_C_bar, d_w_prime, d_ok};
    if (!d_bytes || !d_offsets || null_arrays(chk, lg))
        return set_error(HALO_EINVAL, "halo_pcdl_instances_decode_dev: null buffer");
    HALO_CHECK(check_grid("halo_pcdl_instances_decode_dev", k, lg));
    WireArrays a;
    a.C = (uint4*)d_C, a.z = (uint4*)d_z, a.v = (uint4*)d_v, a.Ls = (uint4*)d_Ls, a.Rs = (uint4*)d_Rs, a.U = (uint4*)d_U;
    a.c = (uint4*)d_c, a.hiding = (uint8_t*)d_hiding, a.C_bar = (uint4*)d_C_bar, a.w_prime = (uint4*)d_w_prime;
    a.ok = (uint8_t*)d_ok;
    return launch_decode(curve, d, lg, k, d_bytes, len, d_offsets, a, (hipStream_t)stream);
}

extern "C" int halo_pcdl_instances_encode(halo_curve_t curve, size_t d, size_t k, const halo_wrapped_point_t* C,
        const halo_fe_t* z, const halo_fe_t* v, const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c, const uint8_t* hiding, const halo_wrapped_point_t* C_bar,
        const halo_fe_t* w_prime, uint8_t* out_bytes, size_t* out_len) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    size_t lg;
    HALO_CHECK(check_d(d, lg));
    if (!out_len) return set_error(HALO_EINVAL, "halo_pcdl_instances_encode: null out_len");
    bool any_hid = false;
    std::vector<uint64_t> offsets(k + 1, 0);
    for (size_t i = 0; i < k; i++) {
        const bool h = hiding && hiding[i];
        any_hid |= h;
        offsets[i + 1] = offsets[i] + wire_instance_size(lg, h);
    }
    const size_t total = offsets[k], cap = *out_len;
    *out_len = total;
    if (!out_bytes || !k) return HALO_OK;  // the size query
    if (cap < total) return set_error(HALO_EINVAL, "halo_pcdl_instances_encode: %zu bytes needed, out_bytes holds %zu", total, cap);
    if (!C || !z || !v || (lg && (!Ls || !Rs)) || !U || !c || (any_hid && (!C_bar || !w_prime)))
        return set_error(HALO_EINVAL, "halo_pcdl_instances_encode: null buffer");
    HALO_CHECK(check_grid("halo_pcdl_instances_encode", k, lg));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    WireParts parts(k, lg);
    const size_t o_bytes = parts.lay.take(total), o_off = parts.lay.take(8 * k);
    HALO_CHECK(st->scratch[0].reserve(parts.lay.total()));
    uint8_t* base = st->scratch[0].as<uint8_t>();
    const void* const host[10] = {C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime};
    for (int j = 0; j < 7; j++) HALO_CHECK(copy_h2d(base + parts.off[j], host[j], parts.bytes[j], s));
    if (any_hid) {
        for (int j = 7; j < 10; j++) HALO_CHECK(copy_h2d(base + parts.off[j], host[j], parts.bytes[j], s));
    } else {
        HALO_HIP(hipMemsetAsync(base + parts.off[7], 0, k, s));  // no flag set: the C_bar / w_prime rows are never read
    }
    HALO_HIP(hipMemsetAsync(base + parts.off[10], 1, k, s));
    HALO_CHECK(copy_h2d(base + o_off, offsets.data(), 8 * k, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_wire_encode<Cv>, dim3(grid_for(k * wire_items(lg), WIRE_THREADS)), dim3(WIRE_THREADS), 0, s,
                           base + o_bytes, (const uint64_t*)(base + o_off), k, (uint64_t)d, lg, parts.at(base));
    });
    HALO_HIP(hipGetLastError());
    std::vector<uint8_t> ok(k);
    HALO_CHECK(copy_d2h(ok.data(), base + parts.off[10], k, s));
    for (size_t i = 0; i < k; i++)
        if (!ok[i])
            return set_error(HALO_EINVAL, "halo_pcdl_instances_encode: instance %zu holds a point that is neither (0, 0) nor on the curve", i);
    return copy_d2h(out_bytes, base + o_bytes, total, s);
}
