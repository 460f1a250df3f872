// acc::decider for k instances (crates/accumulation/src/acc.rs decider; the second half of pcdl::check,
// pcdl.rs:563-583, and of PlonkProof::verify, protocol.rs:493-502): U_i == Commit(Gs[0..d], h_i.coeffs), from
// challenges and points that are already on the device, without a host trip per instance.
//
// Exact mode, in groups of g instances (decider_plan.hpp):
//   (hpoly_rows_device)  the g coefficient rows of the group from its xi rows (poly.hip k_hpoly_tables, k_hpoly_rows)
//   (msm_batch_device)   U'_i of the group: one (polynomial, bucket)-keyed MSM up to msm_multi_max, pipelined above
//   k_decide_compare     one lane per instance: ok[i] = live[i] && U_i is (0, 0) or on the curve && U'_i == U_i
// Combined mode, sum_i rho_i (U_i - Commit(h_i)) = sum_i rho_i U_i - Commit(sum_i rho_i h_i) with the caller's
// random rho: one MSM whatever k.
//   k_decide_mask        rho_i = 0 and U_i = (0, 0) where the instance is not live: it contributes nothing
//   (hpoly_combine_device)  sum_i rho_i h_i(X) as one coefficient vector (k_hpoly_tables with weights, k_hpoly_coeffs)
//   (msm_srs_device)     its commitment P
//   k_decide_negate      -P, the addend of
//   (lincomb_device)     one item of t = k terms: -P + sum_i rho_i U_i; its "valid and the identity" byte is `combined`
//   k_decide_spread      ok[i] = live[i] && combined
// On top of the core: halo_pcdl_decide_batch, halo_pcdl_check_fs_batch (fs_device, then the decider with
// live = the succinct verdicts, the xis never leaving the device) and their _dev forms.
#include <vector>

#include "curve.hpp"
#include "decider.hpp"
#include "decider_plan.hpp"
#include "dispatch.hpp"
#include "lincomb.hpp"
#include "msm.hpp"
#include "pcdl_fs.hpp"
#include "poly.hpp"
#include "quad_ladder.hpp"
#include "runtime.hpp"

namespace halo {

constexpr int DEC_THREADS = 64;  // one lane per instance

// ok[i] = live[i] && U_i is (0, 0) or on the curve && U'_i == U_i, on the canonical affine words (U' is the MSM's
// ark WrappedPoint, so a U that matches it is below the modulus).
template <class Cv>
__global__ __launch_bounds__(DEC_THREADS) void k_decide_compare(const uint4* __restrict__ U, const uint4* __restrict__ Up,
                                                                const uint8_t* __restrict__ live, size_t k,
                                                                uint8_t* __restrict__ ok) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= k) return;
    bool same = !live || live[i] != 0;
    for (int q = 0; q < 4; q++) {
        const uint4 a = U[4 * i + q], b = Up[4 * i + q];
        same = same && a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
    }
    ok[i] = same && aff_on_curve_or_id(aff_from_wrapped<F>(U + 4 * i), fe_from_const<F>(Cv::K::B)) ? 1 : 0;
}

// The weights and points combined mode reads: those of a live instance, zero and (0, 0) for the others.
__global__ __launch_bounds__(DEC_THREADS) void k_decide_mask(const uint8_t* __restrict__ live, const uint4* __restrict__ rho,
                                                             const uint4* __restrict__ U, size_t k,
                                                             uint4* __restrict__ rho_m, uint4* __restrict__ U_m) {
    const size_t i = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= k) return;
    const bool on = !live || live[i] != 0;
#pragma unroll
    for (int q = 0; q < 6; q++) {
        uint4 w = make_uint4(0, 0, 0, 0);
        if (on) w = q < 2 ? rho[2 * i + q] : U[4 * i + q - 2];
        if (q < 2)
            rho_m[2 * i + q] = w;
        else
            U_m[4 * i + q - 2] = w;
    }
}

template <class Cv>
__global__ void k_decide_negate(const uint4* __restrict__ P, uint4* __restrict__ neg) {
    using F = typename Cv::Base;
    if (blockIdx.x | threadIdx.x) return;
    Affine<F> A = aff_from_wrapped<F>(P);
    if (!aff_is_id(A)) A.y = fe_neg(A.y);
    aff_to_wrapped(neg, A);
}

__global__ __launch_bounds__(DEC_THREADS) void k_decide_spread(const uint8_t* __restrict__ live,
                                                               const uint8_t* __restrict__ combined, size_t k,
                                                               uint8_t* __restrict__ ok) {
    const size_t i = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= k) return;
    ok[i] = (!live || live[i] != 0) && combined[0] != 0 ? 1 : 0;
}

// k = 1 with a weight: the exact verdict is also the combined one
__global__ void k_decide_single(const uint8_t* __restrict__ live, const uint8_t* __restrict__ ok, uint8_t* __restrict__ combined) {
    if (blockIdx.x | threadIdx.x) return;
    combined[0] = (live && live[0] == 0) || ok[0] != 0 ? 1 : 0;
}

// code[i] of pcdl::check: 0 accept, 1 the succinct check failed, 2 the decider failed
__global__ __launch_bounds__(DEC_THREADS) void k_check_codes(const uint8_t* __restrict__ succinct,
                                                             const uint8_t* __restrict__ decided, size_t k,
                                                             uint8_t* __restrict__ code) {
    const size_t i = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= k) return;
    code[i] = !succinct[i] ? 1 : !decided[i] ? 2 : 0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// A stage that is more than one kernel (an MSM): its halo_profile_read time is the span on `s` between begin
// and end, its launch count the number of stages.
struct StageScope {
    ProfScope p;
    StageScope(const char* name, hipStream_t s) : p(name, s) {
        if (p.slot >= 0) (void)hipEventRecord(p.a, s);
    }
    void end() {
        if (p.slot >= 0) (void)hipEventRecord(p.b, p.s);
    }
};

static int check_decider_srs(const DeviceState* st, int curve, size_t d) {
    const SrsState& srs = st->srs[curve];
    // (n = d + 1 here, so the SRS prefix Gs[0..d] is never shorter than the coefficients: pedersen::commit's
    // "ms must be larger than Gs", halo_pcdl_decider_commit's HALO_ELENGTH, cannot arise once d <= D)
    if (!srs.n || d > srs.n - 1) return set_error(HALO_ESRSRANGE, "d was larger than D!");
    return HALO_OK;
}

static int decide_exact(DeviceState* st, const DecideCall& a, hipStream_t s) {
    const SrsState& srs = st->srs[a.curve];
    const size_t k = a.k, n = a.d + 1;
    const uint32_t lg = ilog2(n);
    const int field = a.curve == HALO_PALLAS ? HALO_FP : HALO_FQ;
    const int W = srs.shifted_c ? msm_windows(srs.shifted_c) : 1;
    const size_t g = decider_group(n, k, (size_t)std::max<long long>(tuning(TUNE_DECIDE_GROUP_SCALARS), 1), W);
    HALO_CHECK(st->decider[0].reserve(g * n * 32));
    HALO_CHECK(st->decider[1].reserve(hpoly_table_elems(g, lg) * 32));
    HALO_CHECK(st->decider[2].reserve(k * 64));
    uint8_t* rows = st->decider[0].as<uint8_t>();
    uint4* Up = st->decider[2].as<uint4>();
    std::vector<const void*> ptrs(g);
    std::vector<size_t> lens(g, n);
    for (size_t j = 0; j < g; j++) ptrs[j] = rows + j * n * 32;
    for (size_t i0 = 0; i0 < k; i0 += g) {
        const size_t m = std::min(g, k - i0);
        HALO_CHECK(hpoly_rows_device(field, (const uint8_t*)a.xis + i0 * (lg + 1) * 32, m, lg, st->decider[1].ptr, rows, s));
        {
            StageScope st_msm("decide_msm", s);
            HALO_CHECK(msm_batch_device(st, a.curve, ptrs.data(), lens.data(), m, Up + 4 * i0, s));
            HALO_CHECK(msm_join(st, s));  // the next group rewrites the rows
            st_msm.end();
        }
        DISPATCH_CURVE(a.curve, Cv, {
            hipLaunchKernelGGL(k_decide_compare<Cv>, dim3(grid_for(m, DEC_THREADS)), dim3(DEC_THREADS), 0, s,
                               (const uint4*)a.U + 4 * i0, (const uint4*)Up + 4 * i0,
                               a.live ? (const uint8_t*)a.live + i0 : nullptr, m, (uint8_t*)a.ok + i0);
        });
        HALO_HIP(hipGetLastError());
    }
    return HALO_OK;
}

static int decide_combined(DeviceState* st, const DecideCall& a, hipStream_t s) {
    const size_t k = a.k, n = a.d + 1;
    const uint32_t lg = ilog2(n);
    const int field = a.curve == HALO_PALLAS ? HALO_FP : HALO_FQ;
    const size_t o_rho = 0, o_U = o_rho + align256(k * 32), o_P = o_U + align256(k * 64), o_neg = o_P + 256, o_sum = o_neg + 256,
                 o_comb = o_sum + 256, total = o_comb + 256;
    HALO_CHECK(st->decider[0].reserve(n * 32));
    HALO_CHECK(st->decider[1].reserve(hpoly_table_elems(k, lg) * 32));
    HALO_CHECK(st->decider[2].reserve(total));
    HALO_CHECK(st->lincomb_terms.reserve(k * 129));
    uint8_t* base = st->decider[2].as<uint8_t>();
    uint4 *rho_m = (uint4*)(base + o_rho), *U_m = (uint4*)(base + o_U), *P = (uint4*)(base + o_P), *neg = (uint4*)(base + o_neg);
    uint8_t* comb = a.combined ? (uint8_t*)a.combined : base + o_comb;
    const dim3 per_lane(grid_for(k, DEC_THREADS)), blk(DEC_THREADS);
    hipLaunchKernelGGL(k_decide_mask, per_lane, blk, 0, s, (const uint8_t*)a.live, (const uint4*)a.rho, (const uint4*)a.U, k, rho_m,
                       U_m);
    HALO_HIP(hipGetLastError());
    HALO_CHECK(hpoly_combine_device(field, a.xis, k, lg, rho_m, st->decider[1].ptr, st->decider[0].ptr, s, "hpoly_combine"));
    {
        StageScope st_msm("decide_msm", s);
        HALO_CHECK(msm_srs_device(st, a.curve, st->decider[0].ptr, n, nullptr, P, s, MsmOpts::Sync()));
        st_msm.end();
    }
    DISPATCH_CURVE(a.curve, Cv, { hipLaunchKernelGGL(k_decide_negate<Cv>, dim3(1), dim3(1), 0, s, (const uint4*)P, neg); });
    HALO_HIP(hipGetLastError());
    HALO_CHECK(lincomb_device(st, a.curve, neg, U_m, rho_m, 1, k, base + o_sum, comb, s));
    hipLaunchKernelGGL(k_decide_spread, per_lane, blk, 0, s, (const uint8_t*)a.live, (const uint8_t*)comb, k, (uint8_t*)a.ok);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int decide_device(DeviceState* st, const DecideCall& a, hipStream_t s) {
    HALO_CHECK(check_decider_srs(st, a.curve, a.d));
    if (a.rho && a.k > 1) return decide_combined(st, a, s);
    HALO_CHECK(decide_exact(st, a, s));
    if (a.rho && a.combined) {  // k = 1 costs the same either way
        hipLaunchKernelGGL(k_decide_single, dim3(1), dim3(1), 0, s, (const uint8_t*)a.live, (const uint8_t*)a.ok,
                           (uint8_t*)a.combined);
        HALO_HIP(hipGetLastError());
    }
    return HALO_OK;
}

// Everything that needs no device; done: an empty batch.
static int check_decide_args(const char* call, int curve, size_t d, size_t k, const void* xis, const void* U, const void* ok,
                             bool& done) {
    done = false;
    if (curve != HALO_PALLAS && curve != HALO_VESTA) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (k == 0) {
        done = true;
        return HALO_OK;
    }
    const size_t n = d + 1;
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    if (ilog2(n) > 28) return set_error(HALO_EINVAL, "%s: n (%zu) out of range", call, n);
    if (!xis || !U || !ok) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > LINCOMB_MAX_ITEMS / 4) return set_error(HALO_EINVAL, "%s: %zu instances in one call", call, k);
    return HALO_OK;
}

static bool host_below(int curve, const halo_fe_t& x) {
    const uint64_t(&p)[4] = curve == HALO_PALLAS ? FpCfg::MODULUS64 : FqCfg::MODULUS64;  // the scalar field
    for (int q = 3; q >= 0; q--)
        if (x.l[q] != p[q]) return x.l[q] < p[q];
    return false;
}

// A zero weight would leave its instance unchecked.
static int check_rho(const char* call, int curve, const halo_fe_t* rho, size_t k) {
    for (size_t i = 0; rho && i < k; i++) {
        if (!(rho[i].l[0] | rho[i].l[1] | rho[i].l[2] | rho[i].l[3]))
            return set_error(HALO_EINVAL, "%s: rho[%zu] is zero", call, i);
        if (!host_below(curve, rho[i])) return set_error(HALO_EINVAL, "%s: rho[%zu] is not below the modulus", call, i);
    }
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_pcdl_decide_batch_dev(halo_curve_t curve, size_t d, size_t k, const void* d_xis, const void* d_U,
                                          const void* d_live, const void* d_rho, void* d_ok, void* d_combined, void* stream) {
    clear_error();
    const char* call = "halo_pcdl_decide_batch_dev";
    bool done;
    HALO_CHECK(check_decide_args(call, curve, d, k, d_xis, d_U, d_ok, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return decide_device(st, DecideCall{(int)curve, d, k, d_xis, d_U, d_live, d_rho, d_ok, d_combined}, s);
}

extern "C" int halo_pcdl_decide_batch(halo_curve_t curve, size_t d, size_t k, const halo_fe_t* xis,
                                      const halo_wrapped_point_t* U, const uint8_t* live, const halo_fe_t* rho,
                                      uint8_t* ok_out) {
    clear_error();
    const char* call = "halo_pcdl_decide_batch";
    bool done;
    HALO_CHECK(check_decide_args(call, curve, d, k, xis, U, ok_out, done));
    if (done) return HALO_OK;
    const size_t lg = ilog2(d + 1), row = lg + 1;
    for (size_t j = 0; j < k * row; j++)
        if (!host_below(curve, xis[j]))
            return set_error(HALO_EINVAL, "%s: xi_%zu of instance %zu is not below the modulus", call, j % row, j / row);
    HALO_CHECK(check_rho(call, curve, rho, k));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_decider_srs(st, curve, d));
    // only the live instances travel
    std::vector<size_t> idx;
    for (size_t i = 0; i < k; i++) {
        ok_out[i] = 0;
        if (!live || live[i]) idx.push_back(i);
    }
    const size_t m = idx.size();
    if (!m) return HALO_OK;
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t o_xis = 0, o_U = o_xis + align256(m * row * 32), o_rho = o_U + align256(m * 64),
                 n_in = o_rho + align256(rho ? m * 32 : 0);
    HALO_CHECK(st->scratch[0].reserve(n_in));
    HALO_CHECK(st->scratch[1].reserve(m + 256));
    uint8_t *di = st->scratch[0].as<uint8_t>(), *dout = st->scratch[1].as<uint8_t>();
    if (m == k) {
        HALO_CHECK(copy_h2d(di + o_xis, xis, k * row * 32, s));
        HALO_CHECK(copy_h2d(di + o_U, U, k * 64, s));
        if (rho) HALO_CHECK(copy_h2d(di + o_rho, rho, k * 32, s));
    } else {
        std::vector<halo_fe_t> hx(m * row), hr(rho ? m : 0);
        std::vector<halo_wrapped_point_t> hU(m);
        for (size_t j = 0; j < m; j++) {
            std::copy(xis + idx[j] * row, xis + (idx[j] + 1) * row, hx.begin() + j * row);
            hU[j] = U[idx[j]];
            if (rho) hr[j] = rho[idx[j]];
        }
        // pageable sources: each copy returns once the source has been read
        HALO_CHECK(copy_h2d(di + o_xis, hx.data(), m * row * 32, s));
        HALO_CHECK(copy_h2d(di + o_U, hU.data(), m * 64, s));
        if (rho) HALO_CHECK(copy_h2d(di + o_rho, hr.data(), m * 32, s));
        HALO_HIP(hipStreamSynchronize(s));
    }
    uint8_t* d_comb = dout + align256(m);
    DecideCall a{(int)curve, d, m, di + o_xis, di + o_U, nullptr, rho ? di + o_rho : nullptr, dout, d_comb};
    HALO_CHECK(decide_device(st, a, s));
    if (rho && m > 1) {
        uint8_t combined = 0;
        HALO_CHECK(copy_d2h(&combined, d_comb, 1, s));
        if (!combined) {  // some instance fails: the exact verdicts
            a.rho = nullptr;
            HALO_CHECK(decide_device(st, a, s));
        }
    }
    std::vector<uint8_t> got(m);
    HALO_CHECK(copy_d2h(got.data(), dout, m, s));
    for (size_t j = 0; j < m; j++) ok_out[idx[j]] = got[j];
    return HALO_OK;
}

// pcdl::check over device pointers: fs_device, then the decider over the xis it leaves in st->decider[3].
// host_fallback: read `combined` back and rerun a rejected combined batch in exact mode.
static int check_fs_run(const char* call, DeviceState* st, FsCall a, const void* d_rho, void* d_code, void* d_combined,
                        bool host_fallback, hipStream_t s) {
    const size_t k = a.k, lg = ilog2(a.d + 1);
    HALO_CHECK(check_decider_srs(st, a.curve, a.d));
    const size_t o_xis = 0, o_succ = o_xis + align256(k * (lg + 1) * 32), o_dec = o_succ + align256(k), o_comb = o_dec + align256(k);
    HALO_CHECK(st->decider[3].reserve(o_comb + 256));
    uint8_t* base = st->decider[3].as<uint8_t>();
    a.xis_out = base + o_xis;
    a.alpha_out = nullptr;
    a.ok = base + o_succ;
    HALO_CHECK(fs_device(call, st, a, s));
    uint8_t* comb = d_combined ? (uint8_t*)d_combined : base + o_comb;
    DecideCall dc{a.curve, a.d, k, base + o_xis, a.U, base + o_succ, d_rho, base + o_dec, comb};
    HALO_CHECK(decide_device(st, dc, s));
    if (host_fallback && d_rho && k > 1) {
        uint8_t combined = 0;
        HALO_CHECK(copy_d2h(&combined, comb, 1, s));
        if (!combined) {
            dc.rho = nullptr;
            HALO_CHECK(decide_device(st, dc, s));
        }
    }
    hipLaunchKernelGGL(k_check_codes, dim3(grid_for(k, DEC_THREADS)), dim3(DEC_THREADS), 0, s, (const uint8_t*)(base + o_succ),
                       (const uint8_t*)(base + o_dec), k, (uint8_t*)d_code);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

extern "C" int halo_pcdl_check_fs_batch_dev(halo_curve_t curve, size_t d, size_t k, const void* d_C, const void* d_z,
                                            const void* d_v, const void* d_Ls, const void* d_Rs, const void* d_U,
                                            const void* d_c, const void* d_hiding, const void* d_C_bar, const void* d_w_prime,
                                            const void* d_rho, void* d_ok, void* d_combined, void* stream) {
    clear_error();
    const char* call = "halo_pcdl_check_fs_batch_dev";
    const FsCall a{(int)curve, d, k, d_C, d_z, d_v, d_Ls, d_Rs, d_U, d_c, d_hiding, d_C_bar, d_w_prime, nullptr, nullptr, d_ok};
    bool done;
    HALO_CHECK(check_fs_args(call, a, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return check_fs_run(call, st, a, d_rho, d_ok, d_combined, false, s);
}

extern "C" int halo_pcdl_check_fs_batch(halo_curve_t curve, size_t d, size_t k, const halo_wrapped_point_t* C,
                                        const halo_fe_t* z, const halo_fe_t* v, const halo_wrapped_point_t* Ls,
                                        const halo_wrapped_point_t* Rs, const halo_wrapped_point_t* U, const halo_fe_t* c,
                                        const uint8_t* hiding, const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime,
                                        const halo_fe_t* rho, uint8_t* ok_out) {
    clear_error();
    const char* call = "halo_pcdl_check_fs_batch";
    const FsCall host{(int)curve, d, k, C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime, nullptr, nullptr, ok_out};
    bool done;
    HALO_CHECK(check_fs_args(call, host, done));
    if (done) return HALO_OK;
    HALO_CHECK(fs_host_scalars(call, host));
    HALO_CHECK(check_rho(call, curve, rho, k));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_decider_srs(st, curve, d));
    hipStream_t s = 0;
    ScratchUse su(st, s);
    FsCall a;
    HALO_CHECK(fs_upload(st, host, a, s));
    HALO_CHECK(st->scratch[1].reserve(align256(k) + align256(rho ? k * 32 : 0)));
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    void* d_rho = nullptr;
    if (rho) {
        d_rho = dout + align256(k);
        HALO_CHECK(copy_h2d(d_rho, rho, k * 32, s));
    }
    HALO_CHECK(check_fs_run(call, st, a, d_rho, dout, nullptr, true, s));
    return copy_d2h(ok_out, dout, k, s);
}
