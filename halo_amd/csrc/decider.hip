// acc::decider for k instances (crates/accumulation/src/acc.rs decider; the second half of pcdl::check,
// pcdl.rs:563-583, and of PlonkProof::verify, protocol.rs:493-502): U_i == Commit(Gs[0..d], h_i.coeffs), from
// challenges and points that are already on the device, without a host trip per instance.
//
// Exact mode, in groups of g instances (decider_plan.hpp):
//   (hpoly_rows_device)  the g coefficient rows of the group from its xi rows (poly.hip k_hpoly_tables, k_hpoly_rows)
//   (msm_batch_device)   U'_i of the group: one (polynomial, bucket)-keyed MSM up to msm_multi_max, pipelined above
//   k_decide_compare     one lane per instance: ok[i] = live[i] && U_i is (0, 0) or on the curve && U'_i == U_i
// Combined mode, sum_i rho_i (U_i - Commit(h_i)) = sum_i rho_i U_i - Commit(sum_i rho_i h_i) with the caller's
// random rho, or with DecideCall::derive the weights that decide_rho.hip derives from the batch (decide_rho_weights,
// first thing in each of the three cores below): one MSM whatever k.
//   k_decide_mask        rho_i = 0 and U_i = (0, 0) where the instance is not live: it contributes nothing
//   (hpoly_combine_device)  sum_i rho_i h_i(X) as one coefficient vector (k_hpoly_tables with weights, k_hpoly_coeffs)
//   (msm_srs_device)     its commitment P
//   k_decide_negate      -P, the addend of
//   (lincomb_device)     one item of t = k terms: -P + sum_i rho_i U_i; its "valid and the identity" byte is `combined`
//   k_decide_spread      ok[i] = live[i] && combined
// Bisect mode (decide_bisect_device, decider_bisect.hpp): the combined pass with k_bisect_mask in place of
// k_decide_mask, and when it rejects, level by level through the halves that fail.  D(S) = sum_{i in S} rho_i U_i -
// Commit(sum_{i in S} rho_i h_i) is additive, so a failing node needs one pass, over its left half:
//   (hpoly_segments_device)  one coefficient row per node from the half-tables the root pass left
//   (msm_batch_device)   their commitments P_s, in groups as in exact mode
//   k_bisect_left        D(left_s) = -P_s + the root pass's terms rho_i U_i over the left half
//   k_bisect_split       D(right_s) = D(node_s) - D(left_s), the two flags, ok[i] = 0 for a failing leaf
// On top of the core: halo_pcdl_decide_batch, halo_pcdl_check_fs_batch (fs_device, then the decider with
// live = the succinct verdicts, the xis never leaving the device) and their _dev forms.  The scratch carving and
// the uploads are scratch_layout.hpp's / upload_parts, the scalar checks host_scalar.hpp's (check_rho).
#include <vector>

#include "curve.hpp"
#include "decider.hpp"
#include "decider_bisect.hpp"
#include "decider_plan.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "msm.hpp"
#include "pcdl_fs.hpp"
#include "poly.hpp"
#include "quad_ladder.hpp"
#include "runtime.hpp"
#include "sponge_launch.hpp"

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

// Bisect mode's k_decide_mask: an instance that is live but whose U is neither (0, 0) nor on the curve, or whose
// rho is zero or not below the modulus, is masked out as well and valid[i] = 0: it is rejected here and no node's
// sum sees it.
template <class Cv>
__global__ __launch_bounds__(DEC_THREADS) void k_bisect_mask(const uint8_t* __restrict__ live, const uint4* __restrict__ rho,
                                                             const uint4* __restrict__ U, size_t k, uint4* __restrict__ rho_m,
                                                             uint4* __restrict__ U_m, uint8_t* __restrict__ valid) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (i >= k) return;
    const uint4 r0 = rho[2 * i], r1 = rho[2 * i + 1];
    const bool nonzero = (r0.x | r0.y | r0.z | r0.w | r1.x | r1.y | r1.z | r1.w) != 0;
    const bool below = ark_is_canonical<S>(rho + 2 * i);
    const bool curve_ok = aff_on_curve_or_id(aff_from_wrapped<F>(U + 4 * i), fe_from_const<F>(Cv::K::B));
    const bool on = (!live || live[i] != 0) && nonzero && below && curve_ok;
    const uint32_t keep = on ? ~0u : 0u;
    rho_m[2 * i] = make_uint4(r0.x & keep, r0.y & keep, r0.z & keep, r0.w & keep);
    rho_m[2 * i + 1] = make_uint4(r1.x & keep, r1.y & keep, r1.z & keep, r1.w & keep);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint4 w = U[4 * i + q];
        U_m[4 * i + q] = make_uint4(w.x & keep, w.y & keep, w.z & keep, w.w & keep);
    }
    valid[i] = on ? 1 : 0;
}

// Segment b = blockIdx.x, one wave: D(left_b) = -P_b + sum_{lo_b <= i < mid_b} terms[i] as packed XYZZ, P_b the
// commitment of the segment's coefficient row (a WrappedPoint), the terms those of the root pass's lincomb.  Every
// lane adds a strided share with the complete addition, then an LDS tree (k_lincomb_sum's shape).
template <class Cv>
__global__ __launch_bounds__(DEC_THREADS) void k_bisect_left(const uint4* __restrict__ terms, const uint4* __restrict__ P,
                                                             const uint4* __restrict__ segs, uint4* __restrict__ left) {
    using F = typename Cv::Base;
    __shared__ uint4 red[DEC_THREADS * 8];
    const size_t b = blockIdx.x;
    const uint4 seg = segs[b];
    XYZZ<F> acc = xyzz_id<F>();
    if (threadIdx.x == 0) {
        Affine<F> A = aff_from_wrapped<F>(P + 4 * b);
        if (!aff_is_id(A)) A.y = fe_neg(A.y);
        acc = xyzz_from_aff(A);
    }
    for (size_t j = (size_t)seg.x + threadIdx.x; j < seg.y; j += DEC_THREADS) acc = xyzz_add(acc, xyzz_load<F>(terms + 8 * j));
    xyzz_store(red + 8 * threadIdx.x, acc);
    __syncthreads();
    for (int off = DEC_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            xyzz_store(red + 8 * threadIdx.x,
                       xyzz_add(xyzz_load<F>(red + 8 * threadIdx.x), xyzz_load<F>(red + 8 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) xyzz_store(left + 8 * b, xyzz_load<F>(red));
}

// One lane per node s = (lo, mid, hi, src): D(right) = D(node) - D(left) by the general addition (the operands are
// equal when only the left half fails, D(left) is the identity when only the right one does), the children's
// defects at 2 s and 2 s + 1 of `next`, their flags (1 = not the identity: the half holds a wrong instance), and
// ok = 0 for a failing half of one instance.  D(node) is entry src of `cur`.
template <class Cv>
__global__ __launch_bounds__(DEC_THREADS) void k_bisect_split(const uint4* __restrict__ cur, const uint4* __restrict__ left,
                                                              const uint4* __restrict__ segs, size_t f, uint4* __restrict__ next,
                                                              uint8_t* __restrict__ flags, uint8_t* __restrict__ ok) {
    using F = typename Cv::Base;
    const size_t sidx = (size_t)blockIdx.x * DEC_THREADS + threadIdx.x;
    if (sidx >= f) return;
    const uint4 seg = segs[sidx];
    const XYZZ<F> Dl = xyzz_load<F>(left + 8 * sidx);
    const XYZZ<F> Dr = xyzz_add(xyzz_load<F>(cur + 8 * (size_t)seg.w), xyzz_neg(Dl));
    xyzz_store(next + 8 * (2 * sidx), Dl);
    xyzz_store(next + 8 * (2 * sidx + 1), Dr);
    const bool fl = !xyzz_is_id(Dl), fr = !xyzz_is_id(Dr);
    flags[2 * sidx] = fl ? 1 : 0;
    flags[2 * sidx + 1] = fr ? 1 : 0;
    if (fl && seg.y - seg.x == 1) ok[seg.x] = 0;
    if (fr && seg.z - seg.y == 1) ok[seg.y] = 0;
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

// Where a combined pass left its `combined` byte and, in bisect mode, the batch's defect and the validity bytes.
struct CombinedOut {
    uint8_t* comb;
    uint4* sum;
    uint8_t* valid;
};

// bisect: k_bisect_mask's validity test up front; the pass's half-tables, terms and defect are what the descent reads.
static int decide_combined(DeviceState* st, const DecideCall& a, hipStream_t s, bool bisect = false, CombinedOut* out = nullptr) {
    const size_t k = a.k, n = a.d + 1;
    const uint32_t lg = ilog2(n);
    const int field = a.curve == HALO_PALLAS ? HALO_FP : HALO_FQ;
    ScratchLayout lay;  // the masked weights and points, P, -P (WrappedPoints), the sum (XYZZ), its byte, the validity bytes
    const size_t o_rho = lay.take(k * 32), o_U = lay.take(k * 64), o_P = lay.take(64), o_neg = lay.take(64), o_sum = lay.take(128),
                 o_comb = lay.take(1), o_valid = lay.take(bisect ? k : 0);
    HALO_CHECK(st->decider[0].reserve(n * 32));
    HALO_CHECK(st->decider[1].reserve(hpoly_table_elems(k, lg) * 32));
    HALO_CHECK(st->decider[2].reserve(lay.total()));
    HALO_CHECK(st->lincomb_terms.reserve(k * 129));
    uint8_t* base = st->decider[2].as<uint8_t>();
    uint4 *rho_m = (uint4*)(base + o_rho), *U_m = (uint4*)(base + o_U), *P = (uint4*)(base + o_P), *neg = (uint4*)(base + o_neg);
    uint8_t* comb = a.combined ? (uint8_t*)a.combined : base + o_comb;
    const uint8_t* live = (const uint8_t*)a.live;
    const dim3 per_lane(grid_for(k, DEC_THREADS)), blk(DEC_THREADS);
    if (bisect) {
        DISPATCH_CURVE(a.curve, Cv, {
            hipLaunchKernelGGL(k_bisect_mask<Cv>, per_lane, blk, 0, s, live, (const uint4*)a.rho, (const uint4*)a.U, k, rho_m, U_m,
                               base + o_valid);
        });
        live = base + o_valid;
    } else {
        hipLaunchKernelGGL(k_decide_mask, per_lane, blk, 0, s, live, (const uint4*)a.rho, (const uint4*)a.U, k, rho_m, U_m);
    }
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
    hipLaunchKernelGGL(k_decide_spread, per_lane, blk, 0, s, live, (const uint8_t*)comb, k, (uint8_t*)a.ok);
    HALO_HIP(hipGetLastError());
    if (out) *out = CombinedOut{comb, (uint4*)(base + o_sum), base + o_valid};
    return HALO_OK;
}

int decide_device(DeviceState* st, const DecideCall& call, hipStream_t s) {
    // (n = d + 1 here, so the SRS prefix Gs[0..d] is never shorter than the coefficients: pedersen::commit's
    // "ms must be larger than Gs", halo_pcdl_decider_commit's HALO_ELENGTH, cannot arise once d <= D)
    HALO_CHECK(check_verifier_srs(nullptr, st, call.curve, call.d, false));
    DecideCall a = call;
    HALO_CHECK(decide_rho_weights(st, a, s));
    if (a.rho && a.k > 1) return decide_combined(st, a, s);
    HALO_CHECK(decide_exact(st, a, s));
    if (a.rho && a.combined) {  // k = 1 costs the same either way
        hipLaunchKernelGGL(k_decide_single, dim3(1), dim3(1), 0, s, (const uint8_t*)a.live, (const uint8_t*)a.ok,
                           (uint8_t*)a.combined);
        HALO_HIP(hipGetLastError());
    }
    return HALO_OK;
}

// The work of one level of the descent (decider_bisect.hpp's Eval) on the device.
struct BisectDevice {
    DeviceState* st;
    const DecideCall& a;
    hipStream_t s;
    const uint4* cur;   // the defects of this level's nodes (BisectNode::src indexes it)
    uint4* pong[2];     // the children's defects, level by level in turn
    int turn = 0;
    uint4 *segs, *P, *left;  // per level: the node table, the rows' commitments, D(left)
    uint8_t* flags;
    const uint4* terms;  // the root pass's rho_i U_i
    std::vector<const void*> ptrs;
    std::vector<size_t> lens;

    int rows(const BisectNode* level, size_t f, size_t r0, size_t m) {
        const size_t n = a.d + 1;
        const int field = a.curve == HALO_PALLAS ? HALO_FP : HALO_FQ;
        if (r0 == 0) HALO_CHECK(copy_h2d(segs, level, f * sizeof(BisectNode), s));
        // (every launch of the level above has completed: its flags were read)
        HALO_CHECK(st->bisect[0].reserve(m * n * 32));
        uint8_t* rows = st->bisect[0].as<uint8_t>();
        HALO_CHECK(hpoly_segments_device(field, st->decider[1].ptr, a.k, ilog2(n), segs + r0, m, rows, s));
        ptrs.resize(m);
        lens.assign(m, n);
        for (size_t j = 0; j < m; j++) ptrs[j] = rows + j * n * 32;
        {
            StageScope st_msm("decide_msm", s);
            HALO_CHECK(msm_batch_device(st, a.curve, ptrs.data(), lens.data(), m, P + 4 * r0, s));
            HALO_CHECK(msm_join(st, s));  // the next group rewrites the rows
            st_msm.end();
        }
        DISPATCH_CURVE(a.curve, Cv, {
            hipLaunchKernelGGL(k_bisect_left<Cv>, dim3((unsigned)m), dim3(DEC_THREADS), 0, s, terms, (const uint4*)P + 4 * r0,
                               (const uint4*)segs + r0, left + 8 * r0);
        });
        HALO_HIP(hipGetLastError());
        return HALO_OK;
    }

    int split(const BisectNode*, size_t f, uint8_t* host_flags) {
        uint4* next = pong[turn];
        DISPATCH_CURVE(a.curve, Cv, {
            hipLaunchKernelGGL(k_bisect_split<Cv>, dim3(grid_for(f, DEC_THREADS)), dim3(DEC_THREADS), 0, s, cur, (const uint4*)left,
                               (const uint4*)segs, f, next, flags, (uint8_t*)a.ok);
        });
        HALO_HIP(hipGetLastError());
        cur = next;
        turn ^= 1;
        return copy_d2h(host_flags, flags, 2 * f, s);  // the level's one host wait
    }
};
static_assert(sizeof(BisectNode) == sizeof(uint4), "the kernels read a node as one uint4");

int decide_bisect_device(DeviceState* st, const DecideCall& call, hipStream_t s) {
    HALO_CHECK(check_verifier_srs(nullptr, st, call.curve, call.d, false));
    DecideCall a = call;
    HALO_CHECK(decide_rho_weights(st, a, s));
    if (!a.rho || a.k < 2) return decide_device(st, a, s);
    const SrsState& srs = st->srs[a.curve];
    const size_t k = a.k, n = a.d + 1;
    CombinedOut root;
    HALO_CHECK(decide_combined(st, a, s, true, &root));
    uint8_t combined = 0;
    HALO_CHECK(copy_d2h(&combined, root.comb, 1, s));
    if (combined) return HALO_OK;  // ok = the validity bytes
    // The descent's own buffers: the root pass's tables, terms and defect stay where they are.  A level has at
    // most k / 2 nodes and k children.
    const size_t fmax = k / 2;
    ScratchLayout l1, l2;
    const size_t o_terms = l1.take(k * 128), o_pong0 = l1.take(k * 128), o_pong1 = l1.take(k * 128);
    const size_t o_segs = l2.take(fmax * 16), o_P = l2.take(fmax * 64), o_left = l2.take(fmax * 128), o_flags = l2.take(2 * fmax);
    HALO_CHECK(st->bisect[1].reserve(l1.total()));
    HALO_CHECK(st->bisect[2].reserve(l2.total()));
    uint8_t *b1 = st->bisect[1].as<uint8_t>(), *b2 = st->bisect[2].as<uint8_t>();
    HALO_HIP(hipMemcpyAsync(b1 + o_terms, st->lincomb_terms.ptr, k * 128, hipMemcpyDeviceToDevice, s));  // lincomb_device reuses its buffer
    HALO_HIP(hipMemcpyAsync(a.ok, root.valid, k, hipMemcpyDeviceToDevice, s));
    BisectDevice ev{st, a, s, root.sum, {(uint4*)(b1 + o_pong0), (uint4*)(b1 + o_pong1)}, 0, (uint4*)(b2 + o_segs), (uint4*)(b2 + o_P),
                    (uint4*)(b2 + o_left), b2 + o_flags, (const uint4*)(b1 + o_terms), {}, {}};
    const int W = srs.shifted_c ? msm_windows(srs.shifted_c) : 1;
    std::vector<uint8_t> host_ok(k, 1);  // the kernels clear a.ok themselves
    return bisect_descend(k, n, (size_t)std::max<long long>(tuning(TUNE_DECIDE_GROUP_SCALARS), 1), W, ev, host_ok.data());
}

int decide_resolved(DeviceState* st, const DecideCall& call, hipStream_t s) {
    HALO_CHECK(check_verifier_srs(nullptr, st, call.curve, call.d, false));
    DecideCall a = call;
    HALO_CHECK(decide_rho_weights(st, a, s));
    if (!a.rho || a.k < 2) return decide_device(st, a, s);
    if (tuning(TUNE_DECIDE_BISECT) > 0) return decide_bisect_device(st, a, s);
    CombinedOut root;
    HALO_CHECK(decide_combined(st, a, s, false, &root));
    uint8_t combined = 0;
    HALO_CHECK(copy_d2h(&combined, root.comb, 1, s));
    if (combined) return HALO_OK;
    DecideCall exact = a;  // some instance fails: the exact verdicts
    exact.rho = nullptr;
    exact.derive = false;
    return decide_device(st, exact, s);
}

// Everything that needs no device; done: an empty batch.
static int check_decide_args(const char* call, int curve, size_t d, size_t k, const void* xis, const void* U, const void* ok,
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
    if (!xis || !U || !ok) return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (k > LINCOMB_MAX_ITEMS / 4) return set_error(HALO_EINVAL, "%s: %zu instances in one call", call, k);
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
    const bool derive = decide_derives(d_rho);
    if (derive) HALO_CHECK(require_poseidon_params(call, curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return decide_device(st, DecideCall{(int)curve, d, k, d_xis, d_U, d_live, d_rho, d_ok, d_combined, derive}, s);
}

extern "C" int halo_pcdl_decide_bisect_dev(halo_curve_t curve, size_t d, size_t k, const void* d_xis, const void* d_U,
                                           const void* d_live, const void* d_rho, void* d_ok, void* stream) {
    clear_error();
    const char* call = "halo_pcdl_decide_bisect_dev";
    bool done;
    HALO_CHECK(check_decide_args(call, curve, d, k, d_xis, d_U, d_ok, done));
    if (done) return HALO_OK;
    const bool derive = decide_derives(d_rho);
    if (!d_rho && !derive) return set_error(HALO_EINVAL, "%s: null d_rho", call);
    if (derive) HALO_CHECK(require_poseidon_params(call, curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return decide_bisect_device(st, DecideCall{(int)curve, d, k, d_xis, d_U, d_live, d_rho, d_ok, nullptr, derive}, s);
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
        if (!scalar_below(curve, xis[j]))
            return set_error(HALO_EINVAL, "%s: xi_%zu of instance %zu is not below the modulus", call, j % row, j / row);
    HALO_CHECK(check_rho(call, curve, rho, k));
    const bool derive = decide_derives(rho);
    if (derive) HALO_CHECK(require_poseidon_params(call, curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_verifier_srs(call, st, curve, d, false));
    // only the live instances travel (derived weights are those of the batch that travels: its m instances, all live)
    std::vector<size_t> idx;
    for (size_t i = 0; i < k; i++) {
        ok_out[i] = 0;
        if (!live || live[i]) idx.push_back(i);
    }
    const size_t m = idx.size();
    if (!m) return HALO_OK;
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[1].reserve(m + 256));
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    std::vector<halo_fe_t> hx, hr;
    std::vector<halo_wrapped_point_t> hU;
    if (m != k) {  // the live rows, gathered
        hx.resize(m * row), hU.resize(m), hr.resize(rho ? m : 0);
        for (size_t j = 0; j < m; j++) {
            std::copy(xis + idx[j] * row, xis + (idx[j] + 1) * row, hx.begin() + j * row);
            hU[j] = U[idx[j]];
            if (rho) hr[j] = rho[idx[j]];
        }
        xis = hx.data(), U = hU.data(), rho = rho ? hr.data() : nullptr;
    }
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, HostParts{{xis, m * row * 32}, {U, m * 64}, {rho, rho ? m * 32 : 0}}, s, at));
    if (m != k) HALO_HIP(hipStreamSynchronize(s));  // pageable sources: each copy returns once the source has been read
    DecideCall a{(int)curve, d, m, at[0], at[1], nullptr, at[2], dout, dout + align256(m), derive};
    HALO_CHECK(decide_resolved(st, a, s));
    std::vector<uint8_t> got(m);
    HALO_CHECK(copy_d2h(got.data(), dout, m, s));
    for (size_t j = 0; j < m; j++) ok_out[idx[j]] = got[j];
    return HALO_OK;
}

// pcdl::check over device pointers: fs_device, then the decider over the xis it leaves in st->decider[3].
// host_fallback: a rejected combined batch is resolved to per-instance verdicts (decide_resolved).
static int check_fs_run(const char* call, DeviceState* st, FsCall a, const void* d_rho, bool derive, void* d_code,
                        void* d_combined, bool host_fallback, hipStream_t s) {
    const size_t k = a.k, lg = ilog2(a.d + 1);
    HALO_CHECK(check_verifier_srs(call, st, a.curve, a.d, false));
    ScratchLayout lay;
    const size_t o_xis = lay.take(k * (lg + 1) * 32), o_succ = lay.take(k), o_dec = lay.take(k), o_comb = lay.take(1);
    HALO_CHECK(st->decider[3].reserve(lay.total()));
    uint8_t* base = st->decider[3].as<uint8_t>();
    a.xis_out = base + o_xis;
    a.alpha_out = nullptr;
    a.ok = base + o_succ;
    HALO_CHECK(fs_device(call, st, a, s));
    uint8_t* comb = d_combined ? (uint8_t*)d_combined : base + o_comb;
    DecideCall dc{a.curve, a.d, k, base + o_xis, a.U, base + o_succ, d_rho, base + o_dec, comb, derive};
    HALO_CHECK(host_fallback ? decide_resolved(st, dc, s) : decide_device(st, dc, s));
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
    const bool derive = decide_derives(d_rho);  // (check_fs_args has required the Poseidon parameters)
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return check_fs_run(call, st, a, d_rho, derive, d_ok, d_combined, false, s);
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
    const bool derive = decide_derives(rho);
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_verifier_srs(call, st, curve, d, false));
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HostParts in = fs_host_parts(host);
    in.add(rho, rho ? k * 32 : 0);  // the decider's weights, after the succinct check's own rows
    std::vector<const void*> at;
    HALO_CHECK(upload_parts(st, in, s, at));
    HALO_CHECK(st->scratch[1].reserve(k));
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    HALO_CHECK(check_fs_run(call, st, fs_dev_call(host, at), at.back(), derive, dout, nullptr, true, s));
    return copy_d2h(ok_out, dout, k, s);
}
