// The hiding open: the steps of pcdl::open that fill an IPA session before its rounds (ipa.hip).
//
// pcdl::open_without_eval (pcdl.rs:326-392) with p, p_bar and p' kept in the session's buffers
// (the hiding open used to download p_bar / p' and upload p, p_bar, p' between three
// host calls).  The caller owns the transcript, as in the reference:
//   halo_pcdl_open_begin(p, d, z)          asserts of pcdl.rs:338-341; c = p padded to n on the device
//   [hiding] halo_pcdl_open_blind(q, w_bar) -> C_bar      p_bar = (X - z) q, C_bar = commit(p_bar, w_bar)
//            (transcript: absorb C, C_bar, z, v; alpha = challenge)
//            halo_pcdl_open_combine(alpha, C, w) -> C', w'   c = p + alpha p_bar (in place), pcdl.rs:366-371
//   (transcript: absorb C', z, v; xi_0 = challenge)
//   halo_pcdl_open_start(H, xi_0)           H' = xi_0 H; then halo_ipa_round_lr / fold / end
#include <algorithm>
#include <cstring>

#include "dispatch.hpp"
#include "field_ops.hpp"
#include "ipa_session.hpp"
#include "msm.hpp"
#include "points.hpp"
#include "runtime.hpp"
#include "tail.hpp"

namespace halo {

// Small host values passed by value and stored by one launch (instead of one H2D copy per value, each
// a blit kernel of ~4 us on the stream): segment i is cnt[i] uint4 at dst[i], taken in order from v.
struct PutArgs {
    uint4* dst[4];
    int cnt[4];
    uint4 v[16];
};
__global__ void k_put_args(PutArgs a) {
    int base = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        if ((int)threadIdx.x < a.cnt[i]) a.dst[i][threadIdx.x] = a.v[base + threadIdx.x];
        base += a.cnt[i];
    }
}

}  // namespace halo

using namespace halo;

// The hiding combine's scalars for a small SRS MSM in one launch (was k_put_args + k_combine_scalars +
// k_tail_scalars): p' = p + alpha p_bar in place, p_bar <- alpha p_bar, the MSM scalars alpha p_bar as
// GLV words and sides in the small MSM's scratch, w' = w + alpha w_bar and -w, and C (by value) to its
// staging slot for the final's + C.  alpha, w, C by value (no host-to-device copy).
struct CombineSmallArgs {
    uint4 alpha[2], w[2], C[4];  // ark / WrappedPoint words
};
template <class Cv>
__global__ __launch_bounds__(256) void k_combine_small(const CombineSmallArgs a, uint4* p, uint4* pb, size_t n,
                                                       const uint4* w_bar, uint4* w_prime, uint4* negw, uint4* C_out,
                                                       uint32_t* scal, uint8_t* side) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fe<S> al = fe_from_ark<S>(a.alpha);
    if (i < n) {
        const Fe<S> t = fe_mul(al, fe_from_ark<S>(pb + 2 * i));
        fe_to_ark(p + 2 * i, fe_add(fe_from_ark<S>(p + 2 * i), t));
        fe_to_ark(pb + 2 * i, t);
        tail_scalar_val<Cv>(t, 0, i, scal, side);
    }
    if (i == 0) {
        const Fe<S> wv = fe_from_ark<S>(a.w);
        fe_to_ark(w_prime, fe_add(wv, fe_mul(al, fe_from_ark<S>(w_bar))));
        fe_to_ark(negw, fe_neg(wv));
#pragma unroll
        for (int k = 0; k < 4; k++) C_out[k] = a.C[k];
    }
}

// The hiding blind's scalars for a small SRS MSM in one launch (was an H2D copy of w_bar + k_pbar +
// k_tail_scalars): p_bar = (X - z) q (d + 1 coefficients, pcdl.rs:344-347) to p_bar_out and as GLV words
// and sides in the small MSM's scratch, and w_bar (by value) to its staging slot (the MSM's hiding scalar).
template <class Cv>
__global__ __launch_bounds__(256) void k_pbar_small(const uint4* q, size_t d, const uint4* z, const ArkScalarPair wb,
                                                    uint4* w_bar_out, uint4* p_bar_out, uint32_t* scal, uint8_t* side) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        w_bar_out[0] = wb.v[0];
        w_bar_out[1] = wb.v[1];
    }
    if (i > d) return;
    const Fe<S> a = i >= 1 ? fe_from_ark<S>(q + 2 * (i - 1)) : fe_zero<S>();
    const Fe<S> b = i < d ? fe_from_ark<S>(q + 2 * i) : fe_zero<S>();
    const Fe<S> t = fe_sub(a, fe_mul(fe_from_ark<S>(z), b));
    fe_to_ark(p_bar_out + 2 * i, t);
    tail_scalar_val<Cv>(t, 0, i, scal, side);
}

// Up to COMBINE_MSM_MAX coefficients halo_pcdl_open_combine forms C' through an MSM of alpha p_bar (see there)
constexpr size_t COMBINE_MSM_MAX = (size_t)1 << 16;

extern "C" int halo_pcdl_open_begin(halo_curve_t curve, const halo_fe_t* p, size_t len, size_t d, const halo_fe_t* z,
                                    halo_fe_t* v_out, halo_ipa_session** out) {
    clear_error();
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "unknown curve");
    if ((len && !p) || !z || !out) return set_error(HALO_EINVAL, "halo_pcdl_open_begin: null argument");
    const size_t n = d + 1;
    if (n <= 1) return set_error(HALO_EINVAL, "assertion failed: n > 1");
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    // p.degree() <= d: trailing zero coefficients do not count towards the degree
    size_t deg_len = len;
    while (deg_len > 0 && !(p[deg_len - 1].l[0] | p[deg_len - 1].l[1] | p[deg_len - 1].l[2] | p[deg_len - 1].l[3]))
        deg_len--;
    if (deg_len > n) return set_error(HALO_EDEGREE, "assertion failed: p.degree() <= d");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (!srs.n || d > srs.n - 1) return set_error(HALO_ESRSRANGE, "assertion failed: d <= pp.D");
    halo_ipa_session* ses = ipa_acquire(st);
    if (!ses) return HALO_EDEVICE;
    int rc = ipa_setup(st, ses, curve, n, nullptr, p, deg_len, false, nullptr, z);
    if (!rc && v_out) rc = ipa_eval_cs(ses, deg_len, v_out);  // v = p(z) (pcdl::open, pcdl.rs:471)
    if (rc) {
        ipa_release(ses);
        return rc;
    }
    *out = ses;
    return HALO_OK;
}

extern "C" int halo_pcdl_open_blind(halo_ipa_session* ses, const halo_fe_t* q, const halo_fe_t* w_bar,
                                    halo_wrapped_point_t* C_bar) {
    clear_error();
    if (!ses || !q || !w_bar || !C_bar) return set_error(HALO_EINVAL, "halo_pcdl_open_blind: null argument");
    if (ses->op.started || ses->op.blinded)
        return set_error(HALO_EINVAL, "halo_pcdl_open_blind: session already blinded or started");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[ses->op.curve];
    if (!srs.has_sh) return set_error(HALO_ESRSRANGE, "hiding commitment needs S: upload the SRS (S, H) first");
    hipStream_t s = ses->s;
    const size_t n = ses->op.n, d = n - 1;
    char* sm = ses->small.as<char>();
    HALO_CHECK(ses->pbar.reserve(n * 32));
    HALO_CHECK(ses->tmp.reserve(std::max<size_t>(4096 * 32, d * 32)));
    HALO_CHECK(copy_h2d(ses->tmp.ptr, q, d * 32, s));
    // C_bar as packed XYZZ, converted on the host: the MSM's last lane no longer runs an inversion (~0.1 ms
    // of dependent multiplications at the end of the blind)
    if (n <= std::min(srs_small_max(), srs.n)) {  // p_bar, its GLV words and w_bar in one launch (k_pbar_small)
        SmallMsmScratch scr;
        HALO_CHECK(small_msm_scratch(st, ses->op.curve, n, s, &scr));
        ArkScalarPair wb;
        memcpy(&wb.v[0], w_bar, 32);
        DISPATCH_CURVE(ses->op.curve, Cv, {
            hipLaunchKernelGGL(k_pbar_small<Cv>, dim3(grid_for(n, 256)), dim3(256), 0, s, ses->tmp.as<const uint4>(), d,
                               (const uint4*)(sm + SM_Z), wb, (uint4*)(sm + SM_WBAR), ses->pbar.as<uint4>(), scr.scal,
                               scr.side);
        });
        HALO_HIP(hipGetLastError());
        HALO_CHECK(small_msm_sums(st, ses->op.curve, scr, n, sm + SM_WBAR, sm + SM_T, s, true, nullptr, nullptr, nullptr));
    } else {
        HALO_CHECK(copy_h2d(sm + SM_WBAR, w_bar, 32, s));
        HALO_CHECK(pcdl_pbar_device(ses->op.curve, ses->tmp.ptr, d, sm + SM_Z, ses->pbar.ptr, s));
        HALO_CHECK(msm_srs_device(st, ses->op.curve, ses->pbar.ptr, n, sm + SM_WBAR, sm + SM_T, s, MsmOpts::Sync().xyzz()));
    }
    HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_T, sm + SM_T, 128, hipMemcpyDeviceToHost, s));
    HALO_HIP(hipStreamSynchronize(s));
    host_xyzz_to_wrapped(ses->op.curve, ses->pinned + PIN_T, C_bar);
    if (n > COMBINE_MSM_MAX) {  // pcdl_combine_device reads C_bar on the device
        memcpy(ses->pinned + PIN_T, C_bar, 64);
        HALO_HIP(hipMemcpyAsync(sm + SM_CBAR, ses->pinned + PIN_T, 64, hipMemcpyHostToDevice, s));
    }
    ses->op.blinded = true;
    return HALO_OK;
}

extern "C" int halo_pcdl_open_combine(halo_ipa_session* ses, const halo_fe_t* alpha, const halo_wrapped_point_t* C,
                                      const halo_fe_t* w, halo_fe_t* w_prime, halo_wrapped_point_t* C_prime) {
    clear_error();
    if (!ses || !alpha || !C || !w || !w_prime || !C_prime)
        return set_error(HALO_EINVAL, "halo_pcdl_open_combine: null argument");
    if (!ses->op.blinded || ses->op.combined || ses->op.started)
        return set_error(HALO_EINVAL, "halo_pcdl_open_combine: needs exactly one halo_pcdl_open_blind before it");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = ses->s;
    char* sm = ses->small.as<char>();
    const bool small = ses->op.n <= std::min(srs_small_max(), st->srs[ses->op.curve].n);  // (k_combine_small takes them by value)
    if (!small) {  // alpha, w, C and S (internal) in one launch
        PutArgs a{};
        const void* src[4] = {alpha, w, C, st->srs[ses->op.curve].S};
        const size_t off[4] = {SM_ALPHA, SM_W, SM_C, SM_S};
        const int cnt[4] = {2, 2, 4, 4};
        int k = 0;
        for (int i = 0; i < 4; i++) {
            a.dst[i] = (uint4*)(sm + off[i]);
            a.cnt[i] = cnt[i];
            memcpy(&a.v[k], src[i], 16 * cnt[i]);
            k += cnt[i];
        }
        hipLaunchKernelGGL(k_put_args, dim3(1), dim3(64), 0, s, a);
        HALO_HIP(hipGetLastError());
    }
    // c (= p padded) += alpha p_bar in place: p' (pcdl.rs:366); C' = C + alpha C_bar - w' S, w' = w + alpha w_bar.
    // Up to COMBINE_MSM_MAX coefficients C' is formed as C + MSM(G, alpha p_bar) - w S (= C + alpha C_bar - w' S,
    // since C_bar = MSM(G, p_bar) + w_bar S): an MSM (the table path, or the bucket pipeline) instead of
    // the lone-lane scalar multiplications of k_hiding_point (~1.3 ms of dependent curve operations).
    if (ses->op.n <= COMBINE_MSM_MAX) {
        // the MSM as packed XYZZ (no inversion on the device), + C, converted on the host below
        if (small) {
            // one launch for every scalar (k_combine_small), then the small MSM whose final block adds C and
            // puts w' beside the sum: one device-to-host copy of both
            SmallMsmScratch scr;
            HALO_CHECK(small_msm_scratch(st, ses->op.curve, ses->op.n, s, &scr));
            CombineSmallArgs a;
            memcpy(a.alpha, alpha, 32);
            memcpy(a.w, w, 32);
            memcpy(a.C, C, 64);
            DISPATCH_CURVE(ses->op.curve, Cv, {
                hipLaunchKernelGGL(k_combine_small<Cv>, dim3(grid_for(ses->op.n, 256)), dim3(256), 0, s, a, ses->cs.as<uint4>(),
                                   ses->pbar.as<uint4>(), ses->op.n, (const uint4*)(sm + SM_WBAR), (uint4*)(sm + SM_WP),
                                   (uint4*)(sm + SM_NEGW), (uint4*)(sm + SM_C), scr.scal, scr.side);
            });
            HALO_HIP(hipGetLastError());
            HALO_CHECK(small_msm_sums(st, ses->op.curve, scr, ses->op.n, sm + SM_NEGW, sm + SM_T, s, true, sm + SM_C, sm + SM_WP,
                                      sm + SM_T + 128));
            HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_T, sm + SM_T, 160, hipMemcpyDeviceToHost, s));
            HALO_HIP(hipStreamSynchronize(s));
            memcpy(w_prime, ses->pinned + PIN_T_WP, 32);
            host_xyzz_to_wrapped(ses->op.curve, ses->pinned + PIN_T, C_prime);
            ses->op.combined = true;
            return HALO_OK;
        } else {
            HALO_CHECK(pcdl_combine_scalars_device(ses->op.curve, ses->cs.ptr, ses->pbar.ptr, ses->op.n, sm + SM_ALPHA,
                                                   sm + SM_W, sm + SM_WBAR, sm + SM_WP, sm + SM_NEGW, s));
            HALO_CHECK(msm_srs_device(st, ses->op.curve, ses->pbar.ptr, ses->op.n, sm + SM_NEGW, sm + SM_T, s,
                                      MsmOpts::Sync().xyzz()));
            HALO_CHECK(xyzz_add_wrapped_device(ses->op.curve, sm + SM_T, sm + SM_C, s, false));
        }
        HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_FE, sm + SM_WP, 32, hipMemcpyDeviceToHost, s));
        HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_T, sm + SM_T, 128, hipMemcpyDeviceToHost, s));
        HALO_HIP(hipStreamSynchronize(s));
        memcpy(w_prime, ses->pinned + PIN_FE, 32);
        host_xyzz_to_wrapped(ses->op.curve, ses->pinned + PIN_T, C_prime);
    } else {
        HALO_CHECK(pcdl_combine_device(ses->op.curve, ses->cs.ptr, ses->op.n, ses->pbar.ptr, ses->op.n, sm + SM_ALPHA, sm + SM_W,
                                       sm + SM_WBAR, sm + SM_C, sm + SM_CBAR, sm + SM_S, ses->cs.ptr, sm + SM_CP,
                                       sm + SM_WP, s));
        HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_FE, sm + SM_WP, 32, hipMemcpyDeviceToHost, s));
        HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_CP, sm + SM_CP, 64, hipMemcpyDeviceToHost, s));
        HALO_HIP(hipStreamSynchronize(s));
        memcpy(w_prime, ses->pinned + PIN_FE, 32);
        memcpy(C_prime, ses->pinned + PIN_CP, 64);
    }
    ses->op.combined = true;
    return HALO_OK;
}

extern "C" int halo_pcdl_open_start(halo_ipa_session* ses, const halo_wrapped_point_t* H, const halo_fe_t* xi0) {
    clear_error();
    if (!ses || !xi0) return set_error(HALO_EINVAL, "halo_pcdl_open_start: null argument");
    if (ses->op.started) return set_error(HALO_EINVAL, "halo_pcdl_open_start: session already started");
    if (ses->op.blinded && !ses->op.combined)
        return set_error(HALO_EINVAL, "halo_pcdl_open_start: a blinded opening needs halo_pcdl_open_combine first");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    if (!H) {  // the resident SRS's H (pp.H, pcdl.rs:390)
        const SrsState& srs = st->srs[ses->op.curve];
        if (!srs.has_sh) return set_error(HALO_ESRSRANGE, "no (S, H) uploaded");
        H = &srs.H_wrapped;
    }
    return ipa_start(st, ses, nullptr, xi0, H);
}
