// The descent below a rejected combined Schnorr batch (schnorr_bisect.hpp holds the loop and its two
// rules): which items are the wrong ones, without rerunning every ladder.  For a set S of items
//
//   D(S) = (sum_{i in S} rho_i s_i) G - sum_{i in S} rho_i R_i - sum_{i in S} (rho_i e_i) pk_i
//
// is additive over disjoint sets and the root's D is what the combined pass left (SigScratch::D).  That pass also left
// item i's two MSM terms at 2 i and 2 i + 1 of its bases and scalars, so the point part of D([lo, mid)) is msm_device
// over the slice at 2 lo with 2 (mid - lo) terms: nothing is hashed or prepared again.  The G part is
// (P[mid] - P[lo]) G with P the prefix sums mod r of t_i = rho_i s_i (0 for an item that is not live), P[0] = 0.
//
//   k_sig_t             t_i and the inclusive scan of a block of 256 items -> P[i + 1], the block's total
//   k_sig_scan_totals   one block: the exclusive scan of the block totals, 256 at a time with a carry
//   k_sig_scan_add      P[i + 1] += the total of the blocks before i's; P[0] = 0
//                       (once per rejected batch; addition mod r is exact: no ordering caveat, no atomics)
//   per level of f nodes (lo, mid, hi, src):
//   k_sig_node_scalars  P[mid] - P[lo] per node
//   (generator_mul_device)  those scalars times G over the fixed-base comb, one launch; zero gives (0, 0)
//   (msm_device)        per node, the slice's point part as packed XYZZ
//   k_sig_split         one lane per node: D(left) = MSM + comb point, D(right) = D(node) - D(left), the two flags,
//                       ok[i] = 0 for a failing child of one item
//   (schnorr_ladder_device)  over the slice of a node that the leaf or the budget rule ends at
#include "curve.hpp"
#include "decider.hpp"
#include "dispatch.hpp"
#include "fixed_base.hpp"
#include "msm.hpp"
#include "schnorr.hpp"
#include "schnorr_bisect.hpp"

namespace halo {

// The inclusive scan of t over the block, every thread calling; wsum afterwards holds the four waves' totals.
template <class S>
HALO_DEV Fe<S> sig_block_scan(Fe<S> t, uint32_t (*wsum)[NLIMB]) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __syncthreads();  // a caller in a loop: the previous round's wave totals have been read
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Fe<S> o;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) o.v[l] = __shfl_up(t.v[l], off);
        const Fe<S> sum = fe_add(t, o);
        if (lane >= (unsigned)off) t = sum;
    }
    if (lane == 63u) {
#pragma unroll
        for (int l = 0; l < NLIMB; l++) wsum[wave][l] = t.v[l];
    }
    __syncthreads();
    for (unsigned w = 0; w < wave; w++) {  // wave-uniform
        Fe<S> o;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) o.v[l] = wsum[w][l];
        t = fe_add(t, o);
    }
    return t;
}

template <class S>
HALO_DEV Fe<S> sig_block_total(uint32_t (*wsum)[NLIMB]) {
    Fe<S> t = fe_zero<S>();
    for (int w = 0; w < SIG_WAVES; w++) {
        Fe<S> o;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) o.v[l] = wsum[w][l];
        t = fe_add(t, o);
    }
    return t;
}

// t_i = rho_i s_i as k_sig_prepare forms it (the descent runs only when no live item's rho was bad).
template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_t(const uint4* __restrict__ rho, const uint4* __restrict__ s,
                                                       const uint8_t* __restrict__ live, size_t k, uint4* __restrict__ P,
                                                       uint4* __restrict__ totals) {
    using S = typename Cv::Scalar;
    __shared__ uint32_t wsum[SIG_WAVES][NLIMB];
    const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    Fe<S> t = fe_zero<S>();
    if (i < k && live[i] != 0) t = fe_mul(fe_from_ark<S>(rho + 2 * i), fe_from_ark<S>(s + 2 * i));
    t = sig_block_scan(t, wsum);
    if (i < k) fe_store(P + 2 * (i + 1), t);
    if (threadIdx.x == SIG_THREADS - 1) fe_store(totals + 2 * (size_t)blockIdx.x, t);
}

// One block: totals[b] <- the sum of the totals before b.
template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_scan_totals(uint4* __restrict__ totals, size_t nb) {
    using S = typename Cv::Scalar;
    __shared__ uint32_t wsum[SIG_WAVES][NLIMB];
    Fe<S> carry = fe_zero<S>();  // the same in every thread
    for (size_t base = 0; base < nb; base += SIG_THREADS) {
        const size_t j = base + threadIdx.x;
        const Fe<S> own = j < nb ? fe_load<S>(totals + 2 * j) : fe_zero<S>();
        const Fe<S> inc = sig_block_scan(own, wsum);
        if (j < nb) fe_store(totals + 2 * j, fe_add(carry, fe_sub(inc, own)));
        carry = fe_add(carry, sig_block_total<S>(wsum));
    }
}

template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_scan_add(const uint4* __restrict__ totals, size_t k, uint4* __restrict__ P) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    if (i == 0) fe_store(P, fe_zero<S>());
    if (i >= k) return;
    fe_store(P + 2 * (i + 1), fe_add(fe_load<S>(P + 2 * (i + 1)), fe_load<S>(totals + 2 * (size_t)blockIdx.x)));
}

// One lane per node (lo, mid, hi, src): the scalar of the left half's G part, ark.
template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_node_scalars(const uint4* __restrict__ P, const uint4* __restrict__ segs,
                                                                  size_t f, uint4* __restrict__ out) {
    using S = typename Cv::Scalar;
    const size_t n = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    if (n >= f) return;
    const uint4 seg = segs[n];
    fe_to_ark(out + 2 * n, fe_sub(fe_load<S>(P + 2 * (size_t)seg.y), fe_load<S>(P + 2 * (size_t)seg.x)));
}

// One lane per node: D(left) = the slice's MSM (packed XYZZ) + the comb point (a WrappedPoint), either of which may
// be the identity (a half whose items are all dead is an MSM of (0, 0) bases and zero scalars) or the other's
// negative; D(right) = D(node) - D(left) by the general addition (the operands are equal when only the left half
// fails); the children's defects at 2 n and 2 n + 1 of `next`, their flags, and ok = 0 for a failing half of one
// item.  D(node) is entry src of `cur`.
template <class Cv>
__global__ __launch_bounds__(SIG_THREADS) void k_sig_split(const uint4* __restrict__ cur, const uint4* __restrict__ msm,
                                                           const uint4* __restrict__ comb, const uint4* __restrict__ segs, size_t f,
                                                           uint4* __restrict__ next, uint8_t* __restrict__ flags,
                                                           uint8_t* __restrict__ ok) {
    using F = typename Cv::Base;
    const size_t n = (size_t)blockIdx.x * SIG_THREADS + threadIdx.x;
    if (n >= f) return;
    const uint4 seg = segs[n];
    const XYZZ<F> Dl = xyzz_madd(xyzz_load<F>(msm + 8 * n), aff_from_wrapped<F>(comb + 4 * n));
    const XYZZ<F> Dr = xyzz_add(xyzz_load<F>(cur + 8 * (size_t)seg.w), xyzz_neg(Dl));
    xyzz_store(next + 8 * (2 * n), Dl);
    xyzz_store(next + 8 * (2 * n + 1), Dr);
    const bool fl = !xyzz_is_id(Dl), fr = !xyzz_is_id(Dr);
    flags[2 * n] = fl ? 1 : 0;
    flags[2 * n + 1] = fr ? 1 : 0;
    if (fl && seg.y - seg.x == 1) ok[seg.x] = 0;
    if (fr && seg.z - seg.y == 1) ok[seg.y] = 0;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(BisectNode) == sizeof(uint4), "the kernels read a node as one uint4");

// The work of the descent (schnorr_bisect.hpp's Eval) on the device.
struct SigBisectDevice {
    DeviceState* st;
    int curve;
    const uint8_t *pk, *R, *sig_s;
    size_t k, fmax;
    const SigScratch& w;
    uint8_t* ok;
    hipStream_t s;
    const uint4* cur;  // the defects of this level's nodes (BisectNode::src indexes it)
    uint4* pong[2];    // the children's defects, level by level in turn
    uint4 *P, *totals, *segs, *nsc, *comb, *left;
    uint8_t* flags;
    int turn = 0;
    bool scanned = false;

    int scan() {
        const dim3 per_lane(grid_for(k, SIG_THREADS)), blk(SIG_THREADS);
        DISPATCH_CURVE(curve, Cv, {
            ProfScope p0("sig_t", s);
            HALO_LAUNCH(p0, k_sig_t<Cv>, per_lane, blk, 0, s, (const uint4*)w.rho_used, (const uint4*)sig_s,
                        (const uint8_t*)w.live, k, P, totals);
            ProfScope p1("sig_scan_totals", s);
            HALO_LAUNCH(p1, k_sig_scan_totals<Cv>, dim3(1), blk, 0, s, totals, w.nb);
            ProfScope p2("sig_scan_add", s);
            HALO_LAUNCH(p2, k_sig_scan_add<Cv>, per_lane, blk, 0, s, (const uint4*)totals, k, P);
        });
        HALO_HIP(hipGetLastError());
        scanned = true;
        return HALO_OK;
    }

    int passes(const BisectNode* level, size_t f) {
        if (f > fmax) return set_error(HALO_EINVAL, "sig_bisect: a level of %zu nodes (at most %zu)", f, fmax);
        if (!scanned) HALO_CHECK(scan());
        // (every launch of the level above has completed: its flags were read)
        StageScope pass("sig_bisect_pass", s);  // with sig_split, what one level costs on the device
        HALO_CHECK(copy_h2d(segs, level, f * sizeof(BisectNode), s));
        {
            ProfScope prof("sig_node_scalars", s);
            DISPATCH_CURVE(curve, Cv, {
                HALO_LAUNCH(prof, k_sig_node_scalars<Cv>, dim3(grid_for(f, SIG_THREADS)), dim3(SIG_THREADS), 0, s, (const uint4*)P,
                            (const uint4*)segs, f, nsc);
            });
            HALO_HIP(hipGetLastError());
        }
        HALO_CHECK(generator_mul_device(st, curve, nsc, comb, nullptr, nullptr, f, s));
        StageScope stage("sig_bisect_msm", s);
        for (size_t n = 0; n < f; n++)
            HALO_CHECK(msm_device(st, curve, w.bases + 64 * (2 * (size_t)level[n].lo), w.scalars + 32 * (2 * (size_t)level[n].lo),
                                  2 * (size_t)(level[n].mid - level[n].lo), nullptr, nullptr, left + 8 * n, s,
                                  MsmOpts::Sync().xyzz()));
        stage.end();
        pass.end();
        return HALO_OK;
    }

    int split(const BisectNode*, size_t f, uint8_t* host_flags) {
        uint4* next = pong[turn];
        {
            ProfScope prof("sig_split", s);
            DISPATCH_CURVE(curve, Cv, {
                HALO_LAUNCH(prof, k_sig_split<Cv>, dim3(grid_for(f, SIG_THREADS)), dim3(SIG_THREADS), 0, s, cur, (const uint4*)left,
                            (const uint4*)comb, (const uint4*)segs, f, next, flags, ok);
            });
            HALO_HIP(hipGetLastError());
        }
        cur = next;
        turn ^= 1;
        return copy_d2h(host_flags, flags, 2 * f, s);  // the level's one host wait
    }

    int ladder(uint32_t lo, uint32_t hi) {
        StageScope stage("sig_bisect_ladder", s);
        HALO_CHECK(schnorr_ladder_device(st, curve, pk + 64 * (size_t)lo, R + 64 * (size_t)lo, sig_s + 32 * (size_t)lo,
                                         st->schnorr_e.as<uint8_t>() + 32 * (size_t)lo, hi - lo, ok + lo, s));
        stage.end();
        return HALO_OK;
    }
};

int sig_bisect_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s, size_t k,
                      const SigScratch& w, void* d_ok, hipStream_t s) {
    if (k == 1) return HALO_OK;  // the root's defect is the item's own: k_sig_finish wrote its 0
    const SigBisectRules rules{(size_t)std::max<long long>(tuning(TUNE_SCHNORR_BISECT_LEAF), 1),
                               (size_t)std::max<long long>(tuning(TUNE_SCHNORR_BISECT_PASS_ITEMS), 1)};
    // A level's nodes are disjoint and hold two items or more, and the budget rule admits (p + f) c <= k only.
    const size_t fmax = std::max<size_t>(1, std::min(k / 2, k / rules.pass_items));
    ScratchLayout lay;  // the derivation's buffers here are dead once k_sig_prepare has run
    const size_t o_P = lay.take((k + 1) * 32), o_tot = lay.take(w.nb * 32), o_segs = lay.take(fmax * 16), o_nsc = lay.take(fmax * 32),
                 o_comb = lay.take(fmax * 64), o_left = lay.take(fmax * 128), o_pong0 = lay.take(2 * fmax * 128),
                 o_pong1 = lay.take(2 * fmax * 128), o_flags = lay.take(2 * fmax);
    HALO_CHECK(st->schnorr_comb[1].reserve(lay.total()));
    uint8_t* b = st->schnorr_comb[1].as<uint8_t>();
    HALO_HIP(hipMemcpyAsync(d_ok, w.live, k, hipMemcpyDeviceToDevice, s));  // items in passing nodes keep this value
    SigBisectDevice ev{st, curve, (const uint8_t*)d_pk, (const uint8_t*)d_R, (const uint8_t*)d_s, k, fmax, w, (uint8_t*)d_ok, s,
                       (const uint4*)w.D, {(uint4*)(b + o_pong0), (uint4*)(b + o_pong1)}, (uint4*)(b + o_P), (uint4*)(b + o_tot),
                       (uint4*)(b + o_segs), (uint4*)(b + o_nsc), (uint4*)(b + o_comb), (uint4*)(b + o_left), b + o_flags};
    std::vector<uint8_t> host_ok(k, 1);  // the kernels and the ladder clear d_ok themselves
    return sig_bisect_descend(k, rules, ev, host_ok.data());
}

}  // namespace halo
