// The resident SRS (the PublicParams provider, crates/group/src/pp.rs:26-94): everything that writes
// or describes it.  Synthetic bases, the upload and the bincode decoder, the tables derived from the
// points (the window-shifted copies 2^(c w) G_i and the hiding table 2^i S) and the halo_srs_* queries.
// The MSMs that read it are in msm.hip, the multiples table of its prefix in tail.hip.
#include <algorithm>
#include <vector>

#include "dispatch.hpp"
#include "msm.hpp"
#include "points.hpp"
#include "runtime.hpp"

namespace halo {

// ---------------------------------------------------------------------------------------------
// synthetic bases / scalars (shared host/device definition)
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline uint64_t splitmix64(uint64_t& x) {
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__host__ __device__ inline void synth_scalar(uint64_t seed, uint64_t j, uint64_t out[4]) {
    uint64_t st = seed ^ (j * 0xd1b54a32d192ed03ull);
    for (int i = 0; i < 4; i++) out[i] = splitmix64(st);
    out[3] &= 0x1fffffffffffffffull;  // < 2^253 < p
    if ((out[0] | out[1] | out[2] | out[3]) == 0) out[0] = 1;
}

template <class Cv>
__global__ __launch_bounds__(64) void k_synth_bases(uint4* out, size_t n, uint64_t seed) {
    using F = typename Cv::Base;
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    uint64_t k[4];
    synth_scalar(seed, j, k);
    uint32_t w[8];
    for (int i = 0; i < 4; i++) {
        w[2 * i] = (uint32_t)k[i];
        w[2 * i + 1] = (uint32_t)(k[i] >> 32);
    }
    Affine<F> G;
    G.x = fe_from_const<F>(Cv::K::GX);
    G.y = fe_from_const<F>(Cv::K::GY);
    aff_store(out + 4 * j, xyzz_to_aff(xyzz_scalar_mul(G, w)));
}

// ---------------------------------------------------------------------------------------------
// SRS precomputation: window-shifted bases 2^(c w) G_i (w < W) and the hiding table 2^i S
// ---------------------------------------------------------------------------------------------
// copies w in [w_lo, w_hi) -> out[(w - w_lo) n + i] (a rank of a window partition holds only its own)
template <class Cv>
__global__ __launch_bounds__(64) void k_shift_windows(const uint4* gs, size_t n, int c, int w_lo, int w_hi, uint4* out,
                                                      uint32_t* has_id) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> g = aff_load<F>(gs + 4 * i);
    if (aff_is_id(g)) has_id[0] = 1u;  // (every copy of an identity is the identity; a prime-order
                                       // group has no other point with 2^(c w) g = 0)
    if (w_lo == 0) aff_store(out + 4 * i, g);
    XYZZ<F> p = xyzz_from_aff(g);
    for (int w = 1; w < w_hi; w++) {
        for (int k = 0; k < c; k++) p = xyzz_dbl(p);
        if (w >= w_lo) aff_store(out + 4 * ((size_t)(w - w_lo) * n + i), xyzz_to_aff(p));
    }
}

template <class Cv>
__global__ __launch_bounds__(64) void k_pow2_points(const uint4* P_int, uint4* out_xyzz, int count) {
    using F = typename Cv::Base;
    if (threadIdx.x != 0) return;
    XYZZ<F> p = xyzz_from_aff(aff_load<F>(P_int));
    for (int i = 0; i < count; i++) {
        xyzz_store(out_xyzz + 8 * i, p);
        p = xyzz_dbl(p);
    }
}

// hiding table 2^i S (i < 256), internal affine
static int build_s_table(DeviceState* st, int curve, hipStream_t s) {
    SrsState& srs = st->srs[curve];
    HALO_CHECK(srs.s_table.reserve(256 * 64));
    HALO_CHECK(st->scratch[7].reserve(256 * 128 + 64));
    char* tmp = (char*)st->scratch[7].ptr;
    HALO_CHECK(copy_h2d(tmp + 256 * 128, srs.S, 64, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_pow2_points<Cv>, dim3(1), dim3(64), 0, s, (const uint4*)(tmp + 256 * 128), (uint4*)tmp,
                           256);
    });
    HALO_HIP(hipGetLastError());
    return xyzz_to_affine_device(curve, tmp, srs.s_table.ptr, 256, s);
}

// The window-shifted copies 2^(c w) G_i for w in [w_lo, w_hi) (c = 0: the default width for the SRS
// length; w_hi = 0: every window).  The full set serves every SRS MSM; a partial range (one rank of a
// window-partitioned MSM, BASELINE configs[4]) serves halo_msm_srs_windows_dev over that range only.
int srs_precompute_windows(DeviceState* st, int curve, hipStream_t s, int c, int w_lo, int w_hi) {
    SrsState& srs = st->srs[curve];
    if (!srs.n) return set_error(HALO_ESRSRANGE, "no resident SRS to precompute");
    if (c == 0) c = msm_shifted_window_bits(srs.n);
    if (c < 2 || c > 20) return set_error(HALO_EINVAL, "window bits %d outside [2, 20]", c);
    const int W = msm_windows(c);
    if (w_hi == 0) w_hi = W;
    if (w_lo < 0 || w_hi > W || w_lo >= w_hi)
        return set_error(HALO_EINVAL, "window range [%d, %d) outside [0, %d)", w_lo, w_hi, W);
    srs.shifted_c = srs.part_c = 0;  // nothing valid while the copies are rewritten
    // asynchronous MSMs (halo_msm_srs_windows_dev, the pipelined MSM sets) and weighted IPA rounds on
    // other streams may still be reading the copies: drain the device before they are rewritten or
    // reallocated (a precompute is a setup step, never on a timed path)
    HALO_HIP(hipDeviceSynchronize());
    HALO_CHECK(srs.shifted.reserve((size_t)(w_hi - w_lo) * srs.n * 64));
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[7].reserve(4));
    uint32_t* flag = st->scratch[7].as<uint32_t>();
    HALO_HIP(hipMemsetAsync(flag, 0, 4, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_shift_windows<Cv>, dim3(grid_for(srs.n, 64)), dim3(64), 0, s, srs.gs.as<const uint4>(),
                           srs.n, c, w_lo, w_hi, srs.shifted.as<uint4>(), flag);
    });
    HALO_HIP(hipGetLastError());
    uint32_t has_id = 1;
    HALO_HIP(hipMemcpyAsync(&has_id, flag, 4, hipMemcpyDeviceToHost, s));
    HALO_HIP(hipStreamSynchronize(s));
    srs.shifted_has_id = has_id != 0;
    if (w_lo == 0 && w_hi == W) {
        srs.shifted_c = c;
    } else {
        srs.part_c = c;
        srs.part_w0 = w_lo;
        srs.part_w1 = w_hi;
    }
    return HALO_OK;
}

// Installs n WrappedPoints already in device memory (d_wrapped, may be scratch[0]) as the resident
// SRS of `curve`, plus (S, H) when given (host WrappedPoints).
static int srs_install(DeviceState* st, int curve, const void* d_wrapped, size_t n, const halo_wrapped_point_t* S,
                       const halo_wrapped_point_t* H, hipStream_t s) {
    SrsState& srs = st->srs[curve];
    HALO_CHECK(srs.gs.reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(convert_wrapped_to_internal(curve, d_wrapped, srs.gs.ptr, n, s));
    srs.n = n;
    srs.invalidate_derived();
    if (S && H) {
        HALO_CHECK(st->scratch[1].reserve(256));
        char* tmp = (char*)st->scratch[1].ptr;
        HALO_CHECK(copy_h2d(tmp, S, 64, s));
        HALO_CHECK(copy_h2d(tmp + 64, H, 64, s));
        HALO_CHECK(convert_wrapped_to_internal(curve, tmp, tmp + 128, 2, s));
        HALO_CHECK(copy_d2h(srs.S, tmp + 128, 64, s));
        HALO_CHECK(copy_d2h(srs.H, tmp + 192, 64, s));
        srs.H_wrapped = *H;
        srs.has_sh = true;
        HALO_CHECK(build_s_table(st, curve, s));
    }
    HALO_HIP(hipStreamSynchronize(s));
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

// ---------------------------------------------------------------------------------------------
// the SRS wire format (bincode-v2 `standard()` Vec<WrappedPoint> per block,
// pp.rs:36-53; (S, H) tuple in sh.bin) decoded on the device.  A block whose records are all in the
// fixed 72-byte form (every u64 limb as 0xFD + 8 LE bytes -- what the reference's generator writes
// for Montgomery limbs >= 2^32) is decoded by k_decode_points, one record per lane; any other
// record (a small limb gets a shorter varint) sends that block through the sequential host decoder.
// Every point is then checked on the curve on the device (wrappers.rs:606 `assert!(is_on_curve)`).
// ---------------------------------------------------------------------------------------------
__global__ void k_decode_points(const uint8_t* rec0, size_t count, uint4* out, uint32_t* bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const uint8_t* r = rec0 + 72 * i;
    uint32_t w[16];
    bool ok = true;
#pragma unroll
    for (int l = 0; l < 8; l++) {
        const uint8_t* f = r + 9 * l;
        ok &= (f[0] == 0xFD);
        w[2 * l] = (uint32_t)f[1] | ((uint32_t)f[2] << 8) | ((uint32_t)f[3] << 16) | ((uint32_t)f[4] << 24);
        w[2 * l + 1] = (uint32_t)f[5] | ((uint32_t)f[6] << 8) | ((uint32_t)f[7] << 16) | ((uint32_t)f[8] << 24);
    }
    if (!ok) atomicOr(bad, 1u);
    out[4 * i] = make_uint4(w[0], w[1], w[2], w[3]);
    out[4 * i + 1] = make_uint4(w[4], w[5], w[6], w[7]);
    out[4 * i + 2] = make_uint4(w[8], w[9], w[10], w[11]);
    out[4 * i + 3] = make_uint4(w[12], w[13], w[14], w[15]);
}

template <class Cv>
__global__ void k_check_on_curve(const uint4* pts_wrapped, size_t n, uint32_t* bad) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Affine<F> a = aff_from_wrapped<F>(pts_wrapped + 4 * i);
    // y^2 == x^3 + 5 (the identity (0, 0) is not on the curve, as for ark's Affine::new_unchecked)
    const Fe<F> lhs = fe_sqr(a.y);
    const Fe<F> rhs = fe_add(fe_mul(fe_sqr(a.x), a.x), fe_from_const<F>(Cv::K::B));
    if (!fe_eq(lhs, rhs)) atomicAdd(bad, 1u);
}

// bincode-v2 standard() unsigned varint
static bool bc_varint(const uint8_t* b, size_t len, size_t& off, uint64_t& v) {
    if (off >= len) return false;
    const uint8_t t = b[off];
    if (t < 251) {
        v = t;
        off += 1;
        return true;
    }
    const int width = t == 251 ? 2 : t == 252 ? 4 : t == 253 ? 8 : 0;
    if (!width || off + 1 + width > len) return false;
    v = 0;
    for (int i = 0; i < width; i++) v |= (uint64_t)b[off + 1 + i] << (8 * i);
    off += 1 + width;
    return true;
}

static bool bc_point(const uint8_t* b, size_t len, size_t& off, halo_wrapped_point_t& p) {
    for (int l = 0; l < 4; l++)
        if (!bc_varint(b, len, off, p.x[l])) return false;
    for (int l = 0; l < 4; l++)
        if (!bc_varint(b, len, off, p.y[l])) return false;
    return true;
}

extern "C" int halo_srs_window_bits(halo_curve_t curve) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    const SrsState& srs = st->srs[curve];
    return srs.shifted_c ? srs.shifted_c : srs.part_c;
}

extern "C" int halo_srs_read(halo_curve_t curve, size_t offset, size_t n, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!out && n) return set_error(HALO_EINVAL, "halo_srs_read: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (offset + n > srs.n) return set_error(HALO_ESRSRANGE, "range [%zu, %zu) exceeds the SRS length %zu", offset, offset + n, srs.n);
    if (!n) return HALO_OK;
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(n * 64));
    HALO_CHECK(convert_internal_to_wrapped(curve, srs.gs.as<const char>() + offset * 64, st->scratch[0].ptr, n, s));
    return copy_d2h(out, st->scratch[0].ptr, n * 64, s);
}

extern "C" void halo_synth_scalar(halo_curve_t curve, uint64_t seed, uint64_t j, uint64_t out_canonical[4]) {
    (void)curve;
    synth_scalar(seed, j, out_canonical);
}

extern "C" int halo_srs_upload(halo_curve_t curve, const halo_wrapped_point_t* gs, size_t n,
                               const halo_wrapped_point_t* S, const halo_wrapped_point_t* H) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if ((n && !gs)) return set_error(HALO_EINVAL, "halo_srs_upload: null gs");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(n, 2) * 64));
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, gs, n * 64, s));
    return srs_install(st, curve, st->scratch[0].ptr, n, S, H, s);
}

extern "C" int halo_srs_load_bincode(halo_curve_t curve, const uint8_t* const* blocks, const size_t* block_lens,
                                     size_t nblocks, const uint8_t* sh, size_t sh_len, size_t n) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "assertion failed: n.is_power_of_two()");
    if (nblocks && (!blocks || !block_lens)) return set_error(HALO_EINVAL, "halo_srs_load_bincode: null blocks");
    halo_wrapped_point_t SH[2];
    if (sh) {
        size_t off = 0;
        if (!bc_point(sh, sh_len, off, SH[0]) || !bc_point(sh, sh_len, off, SH[1]))
            return set_error(HALO_EINVAL, "Failed to get SH data for curve %s", curve == HALO_PALLAS ? "pallas" : "vesta");
    }
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(n, 2) * 64));
    HALO_CHECK(st->scratch[2].reserve(16));
    uint4* d_pts = st->scratch[0].as<uint4>();
    uint32_t* d_bad = st->scratch[2].as<uint32_t>();
    size_t have = 0;
    std::vector<halo_wrapped_point_t> host_pts;
    for (size_t bi = 0; bi < nblocks && have < n; bi++) {
        const uint8_t* b = blocks[bi];
        const size_t len = block_lens[bi];
        size_t off = 0;
        uint64_t count = 0;
        if (!b || !bc_varint(b, len, off, count)) return set_error(HALO_EINVAL, "Failed to decode G_BLOCKS_NO %zu", bi);
        const size_t take = std::min<size_t>(count, n - have);
        bool fast = (len - off) >= 72 * take;
        if (fast && take) {
            HALO_CHECK(st->scratch[3].reserve(72 * take));
            HALO_HIP(hipMemsetAsync(d_bad, 0, 4, s));
            HALO_CHECK(copy_h2d(st->scratch[3].ptr, b + off, 72 * take, s));
            hipLaunchKernelGGL(k_decode_points, dim3(grid_for(take, 256)), dim3(256), 0, s,
                               st->scratch[3].as<const uint8_t>(), take, d_pts + 4 * have, d_bad);
            HALO_HIP(hipGetLastError());
            uint32_t bad = 0;
            HALO_CHECK(copy_d2h(&bad, d_bad, 4, s));
            fast = (bad == 0);
        }
        if (!fast) {  // general varints: sequential host decode of this block
            host_pts.resize(take);
            for (size_t i = 0; i < take; i++)
                if (!bc_point(b, len, off, host_pts[i])) return set_error(HALO_EINVAL, "Failed to decode G_BLOCKS_NO %zu", bi);
            HALO_CHECK(copy_h2d(d_pts + 4 * have, host_pts.data(), take * 64, s));
        }
        have += take;
    }
    if (have < n) return set_error(HALO_ESRSRANGE, "assertion failed: n <= N (%zu points available)", have);
    HALO_HIP(hipMemsetAsync(d_bad, 0, 4, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_check_on_curve<Cv>, dim3(grid_for(n, 256)), dim3(256), 0, s, (const uint4*)d_pts, n, d_bad);
    });
    HALO_HIP(hipGetLastError());
    uint32_t bad = 0;
    HALO_CHECK(copy_d2h(&bad, d_bad, 4, s));
    if (bad) return set_error(HALO_EINVAL, "assertion failed: affine.is_on_curve() (%u points)", bad);
    return srs_install(st, curve, d_pts, n, sh ? &SH[0] : nullptr, sh ? &SH[1] : nullptr, s);
}

// PublicParams' (S, H) (pp.rs:26-61) as ark WrappedPoints
extern "C" int halo_srs_sh(halo_curve_t curve, halo_wrapped_point_t* S, halo_wrapped_point_t* H) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!S || !H) return set_error(HALO_EINVAL, "halo_srs_sh: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (!srs.has_sh) return set_error(HALO_ESRSRANGE, "no (S, H) uploaded");
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(256));
    char* b = st->scratch[0].as<char>();
    HALO_CHECK(copy_h2d(b, srs.S, 64, s));
    HALO_CHECK(copy_h2d(b + 64, srs.H, 64, s));
    HALO_CHECK(convert_internal_to_wrapped(curve, b, b + 128, 2, s));
    HALO_CHECK(copy_d2h(S, b + 128, 64, s));
    return copy_d2h(H, b + 192, 64, s);
}

extern "C" int halo_srs_len(halo_curve_t curve, size_t* n) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!n) return set_error(HALO_EINVAL, "null n");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    *n = st->srs[curve].n;
    return HALO_OK;
}

extern "C" int halo_srs_synthesize(halo_curve_t curve, size_t n, uint64_t seed) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    SrsState& srs = st->srs[curve];
    HALO_CHECK(srs.gs.reserve(std::max<size_t>(n, 1) * 64));
    if (n) {
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_synth_bases<Cv>, dim3(grid_for(n, 64)), dim3(64), 0, s, srs.gs.as<uint4>(), n, seed);
        });
        HALO_HIP(hipGetLastError());
    }
    HALO_HIP(hipStreamSynchronize(s));
    srs.n = n;
    srs.invalidate_derived();
    return HALO_OK;
}

extern "C" int halo_srs_precompute_windows(halo_curve_t curve) {
    return halo_srs_precompute_window_range(curve, 0, 0, 0);
}

extern "C" int halo_srs_precompute_window_range(halo_curve_t curve, int c, int w_lo, int w_hi) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    ScratchUse su(st, 0);
    return srs_precompute_windows(st, curve, 0, c, w_lo, w_hi);
}
