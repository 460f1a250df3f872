// Pippenger multi-scalar multiplication on gfx950.
//
// Replaces `VariableBaseMSM::msm_unchecked` as called by group::point_dot_affine
// (crates/group/src/group.rs:48-50) and pedersen::commit (crates/accumulation/src/pedersen.rs:21),
// plus the SRS provider PublicParams (crates/group/src/pp.rs:26-94).
//
// Pipeline (all on the device, no host round trip):
//   1. digits   : scalar (ark Montgomery) -> canonical -> W signed c-bit digits
//                 (|d| <= 2^(c-1), W = ceil(256 / c)); key = (window, |d| - 1), value = index|sign.
//   2. sort     : LSD radix sort (8-bit digits, LDS-staged coalesced runs; sort.hip) of the
//                 W*n (bucket key, point ref) pairs: grouped by key, ascending, the order within a
//                 key unspecified; bucket starts from the sorted keys.
//   3. tasks    : every bucket is cut into tasks of <= K entries (skew-proof: an all-equal scalar
//                 vector becomes n/K equal tasks instead of one serial bucket).
//   4. acc      : one thread per task sums its points with XYZZ mixed additions (8M + 2S).
//   5. merge    : bucket sum = sum of its task partials.
//   6. reduce   : per window, segments of L buckets -> (sum_t t B_t, sum_t B_t) by running sums;
//                 one workgroup per window forms sum_j (acc_j + jL sum_j) and tree-reduces in LDS.
//   7. final    : Horner over the windows (+ w * S for hiding commitments), XYZZ -> affine -> ark.
//
// This file: the digit kernels, k_acc and the hiding-term kernels; the scratch-set pipeline (MsmScratch /
// MsmPipe); the four drivers behind one MsmPlan (msm_plan.hpp) with the batch kernels; and the ABI entries
// that run or describe an MSM (halo_msm*, halo_srs_windows, halo_point_dot_projective,
// halo_pedersen_commit, halo_pcdl_commit).  The sort is in sort.hip, the reduction tail in msm_tail.hip,
// the resident SRS and its window-shifted copies in srs.hip, the point conversions and sums in
// points.hip, the host field arithmetic in host_mont.hpp.
#include <algorithm>
#include <type_traits>
#include <vector>
#include <cstdlib>

#include "acc_entries.hpp"
#include "digits.hpp"
#include "dispatch.hpp"
#include "glv.hpp"
#include "msm.hpp"
#include "points.hpp"
#include "runtime.hpp"
#include "sort.hpp"
#include "tree.hpp"

namespace halo {

static_assert(MSM_PARTIAL_U4 == PARTIAL_U4, "msm_plan.hpp lays the partials out in curve.hpp's PARTIAL_U4 words");

// ---------------------------------------------------------------------------------------------
// 1. digits
// ---------------------------------------------------------------------------------------------
// digits[(w - w_lo) * ld + i] for the windows w_lo <= w < w_hi (ld >= n: the leading dimension, the
// batched MSMs' per-polynomial stride; a window range: one rank's share of a window-partitioned MSM)
template <class S>
__global__ void k_digits(const uint4* scalars, size_t n, int c, int W, uint32_t* digits, size_t ld, int w_lo,
                         int w_hi) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    scalar_signed_digits<S>(scalars + 2 * i, c, W, [&](int w, uint32_t out) {
        if (w >= w_lo && w < w_hi) digits[(size_t)(w - w_lo) * ld + i] = out;
    });
}

// k_digits over up to 8 scalar vectors of one length n in one launch (blockIdx.y = vector p, digits at
// digits + p SN): the pair MSMs' L and R sides, which took one launch each, one after the other
struct DigitSrcs {
    const uint4* s[8];
};
template <class S>
__global__ void k_digits_multi(DigitSrcs src, size_t n, int c, int W, uint32_t* digits, size_t SN) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* d = digits + (size_t)blockIdx.y * SN;
    scalar_signed_digits<S>(src.s[blockIdx.y] + 2 * i, c, W, [&](int w, uint32_t out) { d[(size_t)w * n + i] = out; });
}

// GLV recoding (bases not window-shifted): s = k1 + lambda k2 with |k1|, |k2| < 2^128, so each
// scalar gives W = ceil(129 / c) signed digits for point i (k1) and W for phi(G_i) (k2, entry
// n + i): the same number of bucket additions as W = ceil(255 / c) digits of s, but the Horner
// over the window sums needs ~128 doublings instead of ~255 (the latency of small MSMs).
template <class Cv>
__global__ void k_digits_glv(const uint4* scalars, size_t n, int c, int W, uint32_t* digits) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w8[8];
    fe_ark_to_canonical_words<S>(scalars + 2 * i, w8);
    bool neg[2];
    uint32_t mag[2][5];
    glv::decompose<typename Cv::K>(w8, neg[0], mag[0], neg[1], mag[1]);
    const uint32_t half = 1u << (c - 1);
    const uint32_t full = 1u << c;
    for (int h = 0; h < 2; h++) {
        const uint32_t nflip = neg[h] ? 0x80000000u : 0u;
        uint32_t carry = 0;
        for (int w = 0; w < W; w++) {
            const int bit = w * c;
            uint32_t raw = 0;
            if (bit < 160) {
                const int q = bit >> 5, sh = bit & 31;
                const uint64_t lo = mag[h][q];
                const uint64_t hi = (q + 1 < 5) ? mag[h][q + 1] : 0;
                raw = (uint32_t)(((hi << 32) | lo) >> sh) & (full - 1);
            }
            const uint32_t v = raw + carry;
            uint32_t out;
            if (v > half) {
                carry = 1;
                const uint32_t m = full - v;
                out = (m == 0) ? DIGIT_NONE : (((m - 1) | 0x80000000u) ^ nflip);
            } else {
                carry = 0;
                out = (v == 0) ? DIGIT_NONE : ((v - 1) | nflip);
            }
            digits[(size_t)w * 2 * n + (size_t)h * n + i] = out;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 3-5. tasks, accumulation, merge
// ---------------------------------------------------------------------------------------------
// Uniform chunks: thread t accumulates the sorted entries [t K, t K + K) (every lane does the same
// number of mixed additions, whatever the bucket sizes).  A chunk may cross bucket boundaries: its
// first segment's sum goes to first[t], its last segment's (when there are >= 2) to last[t], and the
// buckets strictly inside the chunk are complete, so they go straight to bucket_sums.  k_merge then
// completes the buckets that straddle chunk boundaries.
// The sorted keys and values come through a cursor (acc_entries.hpp) that loads them four entries at a
// time, one 16-byte load per array at the chunk's start and at every multiple of four after it: the lanes
// of a wave are K entries apart, so a 4-byte load per entry asked for a line per lane (per two lanes at
// K = 16) and asked for it again for each of the line's other entries.  Only keys[beg - 1] is still a load
// of its own.
// k_acc's register budget is sized for 4 workgroups per CU (the compiler's own allocation, 124 VGPRs
// with the peeled second entry, the three-chain addition and the cursor's two groups; 5 / 6 per CU
// measured slower).
constexpr int ACC_MIN_BLOCKS = 4;
// npw_lg: log2 n_per_window when it is a power of two (the window of a shifted entry is a shift,
// not a division), else 0xff.
// (Measured and rejected: an LDS-DMA double buffer gathering entry e + 1's point while entry e's
// addition runs -- no change, 1.07 ms: the kernel is bound by its multiply-add issue, not the gathers.)
// One thread's chunk: the sorted entries [t K, t K + K) (see k_acc).
template <class Cv>
__device__ __forceinline__ void acc_chunk(size_t t, uint32_t cnt, const uint32_t* keys, const uint32_t* vals, uint32_t K,
                                          const uint4* bases, uint32_t n_per_window, uint32_t npw_lg, size_t stride,
                                          uint32_t blk_lg, uint32_t glv_n, uint4* first, uint4* last,
                                          uint4* bucket_sums, uint32_t* bstart, uint32_t NB, uint32_t key_lg,
                                          uint32_t poly_off, bool check_q) {
    using F = typename Cv::Base;
    const size_t beg = t * K;
    if (beg >= cnt) {
        if (t == 0)  // no entries at all: every bucket is empty
            for (uint32_t b = 0; b <= NB; b++) bstart[b] = 0;
        return;
    }
    const uint32_t end = (uint32_t)min((size_t)cnt, beg + K);
    AccEntries<> ent(keys, vals);
    ent.start((uint32_t)beg);
    uint32_t cur = ent.key((uint32_t)beg);
    // bucket starts (the tail's k_merge): bstart[b] = first sorted position of key b, for every b
    // whose first position (or, for empty buckets, the next bucket's) falls in this chunk
    {
        const uint32_t prev = beg ? keys[beg - 1] : 0xffffffffu;
        if (prev != cur)
            for (uint32_t b = prev + 1; b <= cur; b++) bstart[b] = (uint32_t)beg;
    }
    bool first_done = false;
    XYZZ<F> acc = xyzz_id<F>();
    bool fresh = true;  // acc is the identity (xyzz_madd_run)
    uint32_t sneg = 0;  // the sign xyzz_madd_run carries beside acc: the sum is (X, -Y, ZZ, ZZZ) when ~0u
    // one entry: the bucket boundary before it, its base point, the addition.  pos: 0 = the chunk's first
    // entry (key cur, acc the identity: a copy), 1 = its second (acc the identity or the affine copy of the
    // first), 2 = any later one.
    auto step = [&](uint32_t e, auto pos) {
        constexpr int POS = decltype(pos)::value;
        if (POS != 0) ent.next(e);
        const uint32_t k = POS == 0 ? cur : ent.key(e);
        if (POS != 0 && k != cur) {  // bucket boundary inside the chunk
            for (uint32_t b = cur + 1; b <= k; b++) bstart[b] = e;
            if (!first_done) {
                partial_store(first + PARTIAL_U4 * t, acc, sneg);  // as it stands (curve.hpp, chunk partials)
                first_done = true;
            } else {
                xyzz_store(bucket_sums + 8 * (size_t)cur, xyzz_settle(xyzz_run_out(acc, sneg)));
            }
            acc = xyzz_id<F>();
            fresh = true;
            sneg = 0;
            cur = k;
        }
        const uint32_t v = ent.val(e);
        size_t idx = v & 0x7fffffffu;
        if (stride) {  // window-shifted SRS: entry w * n_per_window + i -> point w * stride + i
            const uint32_t w = npw_lg < 32 ? (uint32_t)idx >> npw_lg : (uint32_t)idx / n_per_window;
            uint32_t i = (uint32_t)idx - w * n_per_window;
            if (blk_lg < 32) i += (i >> blk_lg) << blk_lg;  // blocks of 2^blk_lg at stride 2^(blk_lg+1)
            // + the point offset of the entry's output (msm_srs_pairs: output k >> key_lg, odd = R at m)
            idx = (size_t)w * stride + i + (size_t)((k >> key_lg) & 1u) * poly_off;
        }
        const bool phi = glv_n && idx >= glv_n;  // GLV: phi(G_i)
        if (phi) idx -= glv_n;
        Affine<F> p = aff_load<F>(bases + 4 * idx);
        if (phi) p.x = fe_mul(p.x, fe_from_const<F>(Cv::K::BETA));
        const uint32_t negmask = (v & 0x80000000u) ? ~0u : 0u;
        if constexpr (POS == 0) {  // acc is the identity: the copy that xyzz_madd_run's fresh branch makes
            if (!(check_q && aff_is_id(p))) {
                fresh = false;
                sneg = negmask;
                acc.X = p.x;
                acc.Y = p.y;
                acc.ZZ = fe_one<F>();
                acc.ZZZ = fe_one<F>();
            }
        } else if constexpr (POS == 1) {
            acc = xyzz_madd_run_aff(acc, sneg, fresh, p, negmask, check_q);
        } else {
            acc = xyzz_madd_run(acc, sneg, fresh, p, negmask, check_q);
        }
    };
    // The first two entries are peeled: every lane of the wave is at its second entry together, whose
    // accumulator is the affine copy of the first (ZZ = ZZZ = 1), so that addition runs without the four
    // multiplications by one.  A lane whose second entry opens a new bucket stores its one-point first
    // segment and starts fresh in that step, as in the loop.
    uint32_t e = (uint32_t)beg;
    step(e++, std::integral_constant<int, 0>{});
    if (e < end) step(e++, std::integral_constant<int, 1>{});
    for (; e < end; e++) step(e, std::integral_constant<int, 2>{});
    partial_store((first_done ? last : first) + PARTIAL_U4 * t, acc, sneg);
    if (end == cnt)
        for (uint32_t b = cur + 1; b <= NB; b++) bstart[b] = cnt;
}

template <class Cv>
__global__ __launch_bounds__(256, ACC_MIN_BLOCKS) void k_acc(const uint32_t* keys, const uint32_t* vals, const uint32_t* count,
                                             uint32_t K, const uint4* bases, uint32_t n_per_window, uint32_t npw_lg,
                                             size_t stride, uint32_t blk_lg, uint32_t glv_n, uint4* first, uint4* last,
                                             uint4* bucket_sums, uint32_t* bstart, uint32_t NB, uint32_t key_lg = 31,
                                             uint32_t poly_off = 0, uint32_t check_q = 1) {
    acc_chunk<Cv>((size_t)blockIdx.x * blockDim.x + threadIdx.x, *count, keys, vals, K, bases, n_per_window, npw_lg,
                  stride, blk_lg, glv_n, first, last, bucket_sums, bstart, NB, key_lg, poly_off, check_q != 0);
}

// ---------------------------------------------------------------------------------------------
// 7. final: Horner over the windows (wave 0), hiding term w * S from the table 2^i S (waves 1-4),
//    XYZZ -> affine -> ark WrappedPoint.
// ---------------------------------------------------------------------------------------------
// The hiding term w * P = sum of the 2^i P table entries over the set bits of w (an 8-level tree),
// -> hide_out (XYZZ).  glv: the table holds 2^i P for i < 128 only and w = k1 + lambda k2
// (|k1|, |k2| < 2^128, glv.hpp): lanes 0-127 take the bits of k1 with 2^i P, lanes 128-255 those of
// k2 with phi(2^i P) = (beta x, y) -- the IPA's 2^i H' table, whose doubling chain is then half as
// long.  Launched on the tail stream when the MSM starts, so it runs beside the digit / sort /
// accumulation phase instead of on the tail's critical path.
template <class Cv>
__device__ __forceinline__ void hide_term_block(const uint4* hide_table, const uint4* hide_scalar, int glv,
                                                uint4* hide_out) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint4 red[128 * 8];
    __shared__ uint32_t kw[8];
    __shared__ uint32_t neg[2];
    const int i = threadIdx.x;
    if (i == 0) {
        uint32_t w8[8];
        fe_ark_to_canonical_words<S>(hide_scalar, w8);
        if (glv) {
            bool n1, n2;
            uint32_t k1[5], k2[5];
            glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
            for (int q = 0; q < 4; q++) {
                kw[q] = k1[q];
                kw[4 + q] = k2[q];
            }
            neg[0] = n1;
            neg[1] = n2;
        } else {
            for (int q = 0; q < 8; q++) kw[q] = w8[q];
        }
    }
    __syncthreads();
    XYZZ<F> v = xyzz_id<F>();
    if ((kw[i >> 5] >> (i & 31)) & 1u) {
        Affine<F> p = aff_load<F>(hide_table + 4 * (glv ? (i & 127) : i));
        if (glv) {
            if (i >= 128) p.x = fe_mul(p.x, fe_from_const<F>(Cv::K::BETA));
            if (neg[i >> 7]) p.y = fe_neg(p.y);
        }
        v = xyzz_from_aff(p);
    }
    v = block_group_sum<F>(v, 256, red);
    if (i == 0) xyzz_store(hide_out, v);
}

template <class Cv>
__global__ __launch_bounds__(256) void k_hide_term(const uint4* hide_table /* internal affine 2^i P */,
                                                   const uint4* hide_scalar /* ark */, int glv, uint4* hide_out) {
    hide_term_block<Cv>(hide_table, hide_scalar, glv, hide_out);
}

// up to 8 hiding terms (msm_srs_pairs): block b -> hide_out + 8 b
struct HideScalars {
    const uint4* sc[8];
};
template <class Cv>
__global__ __launch_bounds__(256) void k_hide_terms(const uint4* hide_table, HideScalars hs, int glv, uint4* hide_out) {
    hide_term_block<Cv>(hide_table, hs.sc[blockIdx.x], glv, hide_out + 8 * blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------
// Four scratch sets in two slots of two, a slot per issuing stream (least recently used slot
// reassigned): consecutive MSMs of one stream alternate between their slot's two sets (the tail of
// k overlaps k+1), two concurrent streams (two IPA openings in lockstep) never wait for each
// other's scratch, and a lone stream with a backlog borrows the idle slot (msm_pick_set).
// (Measured: rotating every MSM over all four sets made the 2^19-2^17 IPA rounds ~50 % slower,
// two sets only made back-to-back commitment batches slower.)
constexpr int MSM_SETS = 4;
struct MsmScratch {
    DevBuf digits, bstart, partials, bucket_sums, seg_acc, seg_sum, bits, window_sums, scan_tmp, conv;
    const uint32_t* skeys = nullptr;   // sorted keys of the current MSM (sort scratch)
    const uint32_t* scount = nullptr;  // device count of valid entries
    SortScratch sort;
    hipEvent_t acc_done = nullptr, tail_done = nullptr, start = nullptr, front_done = nullptr;
    bool tail_pending = false;
    hipStream_t owner = nullptr;  // stream the set's last MSM was enqueued on (msm_join)
};
// Two scratch sets per device: MSM k+1's digit/sort/accumulation phase (throughput-bound, whole
// GPU) runs on the caller's stream while MSM k's reduction tail (latency-bound, a few waves) runs
// on the per-device tail stream.
struct MsmPipe {
    MsmScratch set[MSM_SETS];
    hipStream_t slot_owner[2] = {nullptr, nullptr};
    int slot_next[2] = {0, 0};
    uint64_t slot_used[2] = {0, 0}, clock = 0;
    hipStream_t tail[MSM_SETS] = {};  // one per scratch set: consecutive tails run concurrently
};
static MsmPipe g_msm_pipe[64];  // per device

static bool set_busy(const MsmScratch& m) {
    return m.tail_pending && hipEventQuery(m.tail_done) == hipErrorNotReady;
}

// scratch set of the next MSM issued on stream s (advance: claim it).  A stream whose own slot is
// still busy (a batch of back-to-back commitments) borrows the other slot when that one is idle, so
// one stream alone pipelines four deep; a latency-bound caller (an IPA round, whose previous MSMs
// have completed) stays on its own two sets.
static int msm_pick_set(MsmPipe& P, hipStream_t s, bool advance) {
    int slot = (P.slot_owner[0] == s) ? 0 : (P.slot_owner[1] == s) ? 1 : -1;
    if (slot < 0) slot = (P.slot_used[0] <= P.slot_used[1]) ? 0 : 1;
    int set = 2 * slot + P.slot_next[slot];
    if (set_busy(P.set[set])) {
        const int o = slot ^ 1;
        const int oset = 2 * o + P.slot_next[o];
        if (!set_busy(P.set[2 * o]) && !set_busy(P.set[2 * o + 1])) {
            slot = o;
            set = oset;
        }
    }
    if (advance) {
        P.slot_owner[slot] = s;
        P.slot_next[slot] ^= 1;
        P.slot_used[slot] = ++P.clock;
    }
    return set;
}

// (Measured and rejected, round 4: tail streams restricted to a CU mask (32 / 64 / 128 of the 256
// CUs, hipExtStreamCreateWithCUMask) so that the tail would not share CUs with the next MSM's sort:
// 2^20 step 1.34 -> 2.71 / 2.08 / 1.89 ms -- the tail chain is throughput-bound on fewer CUs and
// becomes the critical path.)
static int pipe_init(MsmPipe& P) {
    if (P.tail[0]) return HALO_OK;
    for (auto& t : P.tail) HALO_HIP(hipStreamCreateWithFlags(&t, hipStreamNonBlocking));
    for (auto& m : P.set) {
        HALO_HIP(hipEventCreateWithFlags(&m.acc_done, hipEventDisableTiming));
        HALO_HIP(hipEventCreateWithFlags(&m.tail_done, hipEventDisableTiming));
        HALO_HIP(hipEventCreateWithFlags(&m.start, hipEventDisableTiming));
        HALO_HIP(hipEventCreateWithFlags(&m.front_done, hipEventDisableTiming));
    }
    return HALO_OK;
}

// halo_shutdown: destroys the pipeline's streams and events while the HIP runtime is alive (a
// static destructor must not outlive it); pipe_init recreates them if the library is used again
void msm_shutdown() {
    for (auto& P : g_msm_pipe) {
        if (!P.tail[0]) continue;
        for (auto& t : P.tail) {
            (void)hipStreamSynchronize(t);
            (void)hipStreamDestroy(t);
            t = nullptr;
        }

        for (auto& m : P.set) {
            for (hipEvent_t* e : {&m.acc_done, &m.tail_done, &m.start, &m.front_done}) {
                if (*e) (void)hipEventDestroy(*e);
                *e = nullptr;
            }
            m.tail_pending = false;
            m.owner = nullptr;
        }
        P.slot_owner[0] = P.slot_owner[1] = nullptr;
    }
}

template <class Cv>
constexpr int curve_id() {
    return std::is_same<Cv, PallasCurve>::value ? HALO_PALLAS : HALO_VESTA;
}

// ---------------------------------------------------------------------------------------------
// What the four drivers below share, all from one MsmPlan (msm_plan.hpp) built once per MSM: the
// scratch reservation, the k_acc launch and the tail's arguments.  Scratch is MsmScratch or
// BatchScratch; the latter has its own digit and list arrays and no reduction grid (batch_windows).
// ---------------------------------------------------------------------------------------------
template <class Scratch>
constexpr bool has_grid = std::is_same<Scratch, MsmScratch>::value;

// hide_slots: hiding terms kept behind the SW window sums (plan_hide_slot)
template <class Scratch>
static int plan_reserve(Scratch& S, const MsmPlan& p, size_t hide_slots) {
    if constexpr (has_grid<Scratch>) {
        HALO_CHECK(S.digits.reserve(p.digits_bytes));
        HALO_CHECK(S.seg_acc.reserve(p.rows_bytes));
        HALO_CHECK(S.seg_sum.reserve(p.cols_bytes));
        HALO_CHECK(S.bits.reserve(p.terms_bytes));
    }
    HALO_CHECK(S.bstart.reserve(p.bstart_bytes));
    HALO_CHECK(S.partials.reserve(p.partials_bytes));
    HALO_CHECK(S.bucket_sums.reserve(p.bucket_sums_bytes));
    HALO_CHECK(S.window_sums.reserve(p.window_sums_bytes(hide_slots)));
    return HALO_OK;
}
static uint4* plan_hide_slot(const MsmScratch& M, const MsmPlan& p) { return M.window_sums.as<uint4>() + 8 * (size_t)p.SW; }

// k_acc's inputs beside the plan and the scratch set.  The defaults are an MSM over plain bases:
// entry value = point index, one output, bases tested for the identity.
struct AccArgs {
    const uint32_t *keys, *vals, *count;  // the sorted entries and their device count
    const uint4* bases;
    uint32_t n_per_window = 1;  // window-shifted bases (stride != 0): entry w n_per_window + i is point
    uint32_t npw_lg = 0;        // w stride + i; npw_lg = log2 n_per_window, or 0xff when no power of two
    size_t stride = 0;
    uint32_t blk_lg = 32;   // < 32: i skips every other block of 2^blk_lg points
    uint32_t glv_n = 0;     // GLV: entries >= glv_n are phi of point - glv_n
    uint32_t key_lg = 31;   // pair MSMs: bit key_lg of the key set = the R side, poly_off points on
    uint32_t poly_off = 0;
    uint32_t check_q = 1;   // 0: the bases hold no identity point
    bool profiled = true;   // timed as "msm_acc"
};
template <class Cv, class Scratch>
static int acc_launch(const MsmPlan& p, Scratch& S, const AccArgs& a, hipStream_t s) {
    // k_acc reads both arrays in 16-byte groups (acc_entries.hpp)
    if ((((uintptr_t)a.keys | (uintptr_t)a.vals) & 15u) != 0)
        return set_error(HALO_EINVAL, "k_acc: sorted keys / values not 16-byte aligned (%p, %p)", (const void*)a.keys,
                         (const void*)a.vals);
    ProfScope prof(a.profiled ? "msm_acc" : nullptr, s);
    uint4* parts = S.partials.template as<uint4>();
    HALO_LAUNCH(prof, k_acc<Cv>, dim3(grid_for(p.nchunks, 256)), dim3(256), 0, s, a.keys, a.vals, a.count, p.K, a.bases,
                a.n_per_window, a.npw_lg, a.stride, a.blk_lg, a.glv_n, parts + p.off_first, parts + p.off_last,
                S.bucket_sums.template as<uint4>(), S.bstart.template as<uint32_t>(), (uint32_t)p.NB, a.key_lg, a.poly_off,
                a.check_q);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The tail's arguments but for what is a driver's own (final_*, pair_*, batch_windows).  n: 0 for an
// empty MSM, whose tail launches nothing.
template <class Scratch>
static MsmTailArgs plan_tail_args(const DeviceState* st, const MsmPlan& p, Scratch& S, size_t n, const uint32_t* skeys,
                                  const uint32_t* scount) {
    MsmTailArgs ta;
    uint4* parts = S.partials.template as<uint4>();
    ta.p = p;
    ta.num_cu = (uint32_t)st->num_cu;
    ta.n = n;
    ta.skeys = skeys;
    ta.scount = scount;
    ta.first = parts + p.off_first;
    ta.last = parts + p.off_last;
    ta.g1 = parts + p.off_g1;
    ta.g2 = parts + p.off_g2;
    ta.bstart = S.bstart.template as<uint32_t>();
    ta.bucket_sums = S.bucket_sums.template as<uint4>();
    ta.rows = ta.cols = ta.terms = nullptr;
    if constexpr (has_grid<Scratch>) {
        ta.rows = S.seg_acc.template as<uint4>();
        ta.cols = S.seg_sum.template as<uint4>();
        ta.terms = S.bits.template as<uint4>();
    }
    ta.window_sums = S.window_sums.template as<uint4>();
    return ta;
}

// window range (shifted bases only): the windows [w_lo, w_hi) of the scalars (w_hi <= 0: all), over
// shifted copies that start at window base_w0 (a partially precomputed range)
struct MsmWindowRange {
    int w_lo = 0, w_hi = 0, base_w0 = 0;
};

// bases_int: n internal affine points, or (shifted) W * n window-shifted points (single bucket set).
template <class Cv>
static int msm_device_t(DeviceState* st, const uint4* bases_int, bool shifted, size_t shift_stride,
                        const uint4* scalars_ark, size_t n, int c_req, const uint4* hide_table, const uint4* hide_scalar,
                        uint4* d_out_wrapped, hipStream_t s, const MsmOpts& o, MsmWindowRange wr = {}) {
    MsmPipe& PP = g_msm_pipe[st->device & 63];
    HALO_CHECK(pipe_init(PP));
    // preset: the set the caller already claimed (and waited for) to stage converted bases in
    const int set = o.preset >= 0 ? o.preset : msm_pick_set(PP, s, true);
    MsmScratch& M = PP.set[set];
    // the previous user of this scratch set must have finished its tail
    if (M.tail_pending && o.preset < 0) HALO_HIP(hipStreamWaitEvent(s, M.tail_done, 0));
    const hipStream_t ts = PP.tail[set];
    const size_t nn = std::max<size_t>(n, 1);
    // non-shifted bases: GLV (2n half-size scalars, ~128-bit windows) -- see k_digits_glv
    const bool glv = !shifted;
    const size_t NP = glv ? 2 * nn : nn;  // digit entries per window
    const int c = c_req ? c_req : msm_window_bits(NP);
    const int W_all = glv ? (129 + c - 1) / c : msm_windows(c);
    // the partials of a partition of the windows add up
    int w_lo = wr.w_lo, w_hi = wr.w_hi;
    if (w_hi <= 0 || glv) {
        w_lo = 0;
        w_hi = W_all;
    }
    if (w_lo < 0 || w_hi > W_all || w_lo >= w_hi)
        return set_error(HALO_EINVAL, "window range [%d, %d) outside [0, %d)", w_lo, w_hi, W_all);
    const int W = w_hi - w_lo;
    if (shifted && w_lo != wr.base_w0) bases_int += 4 * (size_t)(w_lo - wr.base_w0) * shift_stride;
    const uint32_t B = 1u << (c - 1);
    // sort geometry: SW windows of SN entries each (shifted: one window over all W * n digits)
    const int SW = shifted ? 1 : W;
    const MsmPlan pl = msm_plan((size_t)W * NP, (size_t)SW * B, SW, B, c, st->num_cu, W, shifted ? (size_t)W * nn : NP);
    HALO_CHECK(plan_reserve(M, pl, 1));  // + the hiding term's slot

    // the hiding term (k_hide_term) runs on the tail stream beside the accumulation phase
    uint4* hide_slot = nullptr;
    if (hide_table && hide_scalar) {
        hide_slot = plan_hide_slot(M, pl);
        HALO_HIP(hipEventRecord(M.start, s));
        HALO_HIP(hipStreamWaitEvent(ts, M.start, 0));
        if (o.hide_ready) HALO_HIP(hipStreamWaitEvent(ts, o.hide_ready, 0));  // table built on a side stream
        hipLaunchKernelGGL(k_hide_term<Cv>, dim3(1), dim3(256), 0, ts, hide_table, hide_scalar, (int)o.hide_glv,
                           hide_slot);
        HALO_HIP(hipGetLastError());
    }

    if (n > 0) {
        // shifted, all windows: digit recoding fused into the sort's first pass
        const bool fuse = shifted && w_lo == 0 && w_hi == W_all && msm_fuse_first_pass(1, n, W_all, B, pl.key_bits);
        if (glv)
            hipLaunchKernelGGL(k_digits_glv<Cv>, dim3(grid_for(n, 256)), dim3(256), 0, s, scalars_ark, n, c, W,
                               M.digits.as<uint32_t>());
        else if (!fuse)
            hipLaunchKernelGGL(k_digits<typename Cv::Scalar>, dim3(grid_for(n, 256)), dim3(256), 0, s, scalars_ark,
                               n, c, W_all, M.digits.as<uint32_t>(), n, w_lo, w_hi);
        HALO_HIP(hipGetLastError());
        uint32_t *skeys = nullptr, *svals = nullptr;
        const uint32_t* scount = nullptr;
        RsFused fz{scalars_ark, n, c, W_all, curve_id<Cv>() == HALO_PALLAS ? HALO_FP : HALO_FQ};
        HALO_CHECK(msm_radix_sort(M.digits.as<const uint32_t>(), pl.E, pl.SN, B, pl.key_bits, M.sort, &skeys, &svals,
                                  &scount, nullptr, pl.NB, s, fuse ? &fz : nullptr));
        // the resident window-shifted SRS without identity points: k_acc skips the bases' identity test
        const SrsState& srs_c = st->srs[curve_id<Cv>()];
        const bool srs_bases = shifted && srs_c.shifted_c != 0 && srs_c.shifted.ptr &&
                               (const char*)bases_int >= srs_c.shifted.as<const char>() &&
                               (const char*)bases_int < srs_c.shifted.as<const char>() + srs_c.shifted.bytes;
        AccArgs a{skeys, svals, scount, bases_int};
        a.n_per_window = (uint32_t)nn;
        a.npw_lg = is_pow2(nn) ? ilog2(nn) : 0xffu;
        a.stride = (shifted && (shift_stride != nn || o.blk_lg < 32)) ? shift_stride : (size_t)0;
        a.blk_lg = o.blk_lg;
        a.glv_n = glv ? (uint32_t)nn : 0u;
        a.check_q = (srs_bases && !srs_c.shifted_has_id) ? 0u : 1u;
        HALO_CHECK(acc_launch<Cv>(pl, M, a, s));
        M.skeys = skeys;
        M.scount = scount;
    } else {
        HALO_HIP(hipMemsetAsync(M.window_sums.ptr, 0, (size_t)SW * 128, s));
    }
    // ---- tail (latency-bound: task merge and bucket reduction) on the tail stream, overlapping the
    // caller's next MSM
    HALO_HIP(hipEventRecord(M.acc_done, s));
    HALO_HIP(hipStreamWaitEvent(ts, M.acc_done, 0));
    MsmTailArgs ta = plan_tail_args(st, pl, M, n, M.skeys, M.scount);
    // one window set with a nonempty MSM (the tail reaches k_bitcombine): it also finishes the MSM
    const bool fuse = SW == 1 && n > 0;
    if (fuse) {
        ta.final_mode = o.out_xyzz ? 2 : 1;
        ta.final_hide = (const uint4*)hide_slot;
        ta.final_out = (uint4*)d_out_wrapped;
    }
    HALO_CHECK(msm_tail_launch(curve_id<Cv>(), ta, ts));
    if (!fuse)
        HALO_CHECK(msm_final_launch(curve_id<Cv>(), M.window_sums.as<const uint4>(), SW, c, (const uint4*)hide_slot,
                                    d_out_wrapped, (int)o.out_xyzz, ts));
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipEventRecord(M.tail_done, ts));
    M.tail_pending = true;
    M.owner = s;
    if (!o.async) HALO_HIP(hipStreamWaitEvent(s, M.tail_done, 0));
    return HALO_OK;
}

// ---------------------------------------------------------------------------------------------
// Batched commitments as ONE MSM (halo_msm_batch_dev for small polynomials): k scalar vectors over
// the resident window-shifted SRS share one digit pass, one sort (key = (polynomial, bucket)), one
// accumulation and one reduction tail with a window per polynomial; k_sums_out converts each
// polynomial's bucket-weighted sum.  At n = 2^16 one MSM is latency-bound (a few thousand
// workgroups, a ~1 ms reduction tail); sixteen of them in one pass fill the GPU once.
// ---------------------------------------------------------------------------------------------
template <class Cv>
__global__ __launch_bounds__(64) void k_sums_out(const uint4* window_sums, uint32_t k, uint4* out_wrapped) {
    using F = typename Cv::Base;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    aff_to_wrapped(out_wrapped + 4 * (size_t)i, xyzz_to_aff(xyzz_load<F>(window_sums + 8 * (size_t)i)));
}

template <class Cv>
static int msm_multi_device_t(DeviceState* st, const void* const* scalars, const size_t* lens, size_t k,
                              uint4* d_out, hipStream_t s) {
    SrsState& srs = st->srs[curve_id<Cv>()];
    MsmPipe& PP = g_msm_pipe[st->device & 63];
    HALO_CHECK(pipe_init(PP));
    const int set = msm_pick_set(PP, s, true);
    MsmScratch& M = PP.set[set];
    if (M.tail_pending) HALO_HIP(hipStreamWaitEvent(s, M.tail_done, 0));
    size_t nmax = 1;
    bool ragged = false;
    for (size_t p = 0; p < k; p++) nmax = std::max(nmax, lens[p]);
    size_t ld = 1;
    while (ld < nmax) ld <<= 1;
    if (ld > srs.n) ld = nmax;
    for (size_t p = 0; p < k; p++) ragged |= lens[p] != ld;
    const int c = srs.shifted_c, W = msm_windows(c);
    const uint32_t B = 1u << (c - 1);
    const size_t SN = (size_t)W * ld, E = k * SN;
    if (E >= (1ull << 32)) return set_error(HALO_EINVAL, "halo_msm_batch_dev: batch too large");
    const MsmPlan pl = msm_plan(E, k * (size_t)B, (int)k, B, c, st->num_cu, W, SN);
    HALO_CHECK(plan_reserve(M, pl, 0));
    uint32_t* digits = M.digits.as<uint32_t>();
    if (ragged) HALO_HIP(hipMemsetAsync(digits, 0xff, E * 4, s));  // DIGIT_NONE past each length
    for (size_t p = 0; p < k; p++)
        if (lens[p])
            hipLaunchKernelGGL(k_digits<typename Cv::Scalar>, dim3(grid_for(lens[p], 256)), dim3(256), 0, s,
                               (const uint4*)scalars[p], lens[p], c, W, digits + p * SN, ld, 0, W);
    HALO_HIP(hipGetLastError());
    uint32_t *skeys = nullptr, *svals = nullptr;
    const uint32_t* scount = nullptr;
    HALO_CHECK(msm_radix_sort(digits, E, SN, B, pl.key_bits, M.sort, &skeys, &svals, &scount, nullptr, pl.NB, s));
    AccArgs a{skeys, svals, scount, srs.shifted.as<const uint4>()};
    a.n_per_window = (uint32_t)ld;
    a.npw_lg = is_pow2(ld) ? ilog2(ld) : 0xffu;
    a.stride = srs.n;
    a.check_q = srs.shifted_has_id ? 1u : 0u;
    HALO_CHECK(acc_launch<Cv>(pl, M, a, s));
    const MsmTailArgs ta = plan_tail_args(st, pl, M, E, skeys, scount);
    HALO_CHECK(msm_tail_launch(curve_id<Cv>(), ta, s));
    hipLaunchKernelGGL(k_sums_out<Cv>, dim3(grid_for(k, 64)), dim3(64), 0, s, M.window_sums.as<const uint4>(),
                       (uint32_t)k, d_out);
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipEventRecord(M.tail_done, s));
    M.tail_pending = true;
    M.owner = s;
    return HALO_OK;
}

// ---------------------------------------------------------------------------------------------
// The IPA's weighted-round pairs (ipa.hip): L = sum_i sl[i] G[map(i)] and R = sum_i sr[i] G[m + map(i)],
// map(i) = i + (i >> lg m) << lg m (the left / right halves of the 2m-blocks), each plus its hiding
// term dot H' from the 2^i table, for np <= 4 sessions in lockstep -- ONE MSM over the window-shifted
// SRS with key (output, bucket): one digit pass, one sort, one accumulation and one reduction tail
// (SW = 2 np) instead of 2 np MSMs whose fronts and accumulations run one after the other.  Outputs
// packed XYZZ (128 B each).
// ---------------------------------------------------------------------------------------------
template <class Cv>
static int msm_srs_pairs_t(DeviceState* st, size_t np, const MsmPairIO* io, size_t half, uint32_t lgm,
                           const uint4* hide_table, hipStream_t s, hipEvent_t hide_ready, const MsmPreHide* pre_hide,
                           uint32_t* emit_host, uint32_t seq) {
    SrsState& srs = st->srs[curve_id<Cv>()];
    const size_t m = (size_t)1 << lgm;
    if (!srs.shifted_c) return set_error(HALO_EINVAL, "msm_srs_pairs: no window-shifted SRS");
    if (!np || np > 4) return set_error(HALO_EINVAL, "msm_srs_pairs: %zu pairs (1..4)", np);
    if (!half || (half & (half - 1)) || half % m || 2 * half > srs.n)
        return set_error(HALO_EINVAL, "msm_srs_pairs: %zu terms per side, blocks of %zu, SRS %zu", half, m, srs.n);
    MsmPipe& PP = g_msm_pipe[st->device & 63];
    HALO_CHECK(pipe_init(PP));
    const int set = msm_pick_set(PP, s, true);
    MsmScratch& M = PP.set[set];
    if (M.tail_pending) HALO_HIP(hipStreamWaitEvent(s, M.tail_done, 0));
    const hipStream_t ts = PP.tail[set];
    const int P = (int)(2 * np);  // outputs: L0, R0, L1, R1, ...
    const int c = srs.shifted_c, W = msm_windows(c);
    const uint32_t B = 1u << (c - 1);
    const size_t SN = (size_t)W * half, E = P * SN;
    if (E >= (1ull << 32)) return set_error(HALO_EINVAL, "msm_srs_pairs: too large");
    const MsmPlan pl = msm_plan(E, P * (size_t)B, P, B, c, st->num_cu, W, SN);
    HALO_CHECK(plan_reserve(M, pl, P));  // + the hiding terms
    uint4* hide_slot = plan_hide_slot(M, pl);
    // the hiding terms on the tail stream, beside the front and the accumulation
    HALO_HIP(hipEventRecord(M.start, s));
    HALO_HIP(hipStreamWaitEvent(ts, M.start, 0));
    if (hide_ready) HALO_HIP(hipStreamWaitEvent(ts, hide_ready, 0));
    if (pre_hide) {
        pre_hide->fn(ts, pre_hide->ctx);
        HALO_HIP(hipGetLastError());
    }
    HideScalars hs{};
    MsmOuts8 outs{};
    for (size_t q = 0; q < np; q++) {
        hs.sc[2 * q] = (const uint4*)io[q].hide_l;
        hs.sc[2 * q + 1] = (const uint4*)io[q].hide_r;
        outs.o[2 * q] = (uint4*)io[q].out_l;
        outs.o[2 * q + 1] = (uint4*)io[q].out_r;
    }
    hipLaunchKernelGGL(k_hide_terms<Cv>, dim3(P), dim3(256), 0, ts, hide_table, hs, 1, hide_slot);
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipEventRecord(M.front_done, ts));
    uint32_t* digits = M.digits.as<uint32_t>();
    DigitSrcs ds{};
    for (int p = 0; p < P; p++) ds.s[p] = (const uint4*)(p & 1 ? io[p / 2].sr : io[p / 2].sl);
    // the digit recoding fused into the sort's first pass (thread = scalar, round = window), as the
    // headline MSM's: no digit array written and read back
    const bool fuse = msm_fuse_first_pass(P, half, W, B, pl.key_bits);
    RsFused fz{nullptr, half, c, W, curve_id<Cv>() == HALO_PALLAS ? HALO_FP : HALO_FQ, P, {}};
    for (int p = 0; p < P; p++) fz.srcs[p] = ds.s[p];
    if (!fuse) {
        hipLaunchKernelGGL(k_digits_multi<typename Cv::Scalar>, dim3(grid_for(half, 256), P), dim3(256), 0, s, ds, half,
                           c, W, digits, SN);
        HALO_HIP(hipGetLastError());
    }
    uint32_t *skeys = nullptr, *svals = nullptr;
    const uint32_t* scount = nullptr;
    HALO_CHECK(msm_radix_sort(digits, E, SN, B, pl.key_bits, M.sort, &skeys, &svals, &scount, nullptr, pl.NB, s,
                              fuse ? &fz : nullptr));
    AccArgs a{skeys, svals, scount, srs.shifted.as<const uint4>()};
    a.n_per_window = (uint32_t)half;
    a.npw_lg = ilog2(half);
    a.stride = srs.n;
    a.blk_lg = lgm;
    a.key_lg = (uint32_t)(c - 1);  // output = key >> key_lg, its R sides m points on
    a.poly_off = (uint32_t)m;
    a.check_q = srs.shifted_has_id ? 1u : 0u;
    HALO_CHECK(acc_launch<Cv>(pl, M, a, s));
    MsmTailArgs ta = plan_tail_args(st, pl, M, E, skeys, scount);
    ta.pair_hide = hide_slot;  // k_bitcombine adds the hiding terms and writes the outputs
    ta.pair_outs = outs;
    if (np == 1) {
        ta.pair_host = emit_host;
        ta.pair_seq = seq;
    }
    HALO_HIP(hipStreamWaitEvent(s, M.front_done, 0));  // the hiding terms (done beside the front)
    HALO_CHECK(msm_tail_launch(curve_id<Cv>(), ta, s));
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipEventRecord(M.tail_done, s));
    M.tail_pending = true;
    M.owner = s;
    return HALO_OK;
}

int msm_srs_pairs_device(DeviceState* st, int curve, size_t np, const MsmPairIO* io, size_t half, uint32_t lgm,
                         const void* hide_table, hipStream_t s, hipEvent_t hide_ready, const MsmPreHide* pre_hide,
                         uint32_t* emit_host, uint32_t seq) {
    int rc;
    DISPATCH_CURVE(curve, Cv, {
        rc = msm_srs_pairs_t<Cv>(st, np, io, half, lgm, (const uint4*)hide_table, s, hide_ready, pre_hide, emit_host,
                                 seq);
    });
    return rc;
}

// polynomials up to this length take the one-MSM batch path (tuning "msm_multi_max", default 2^18;
// 0 = off)
static size_t msm_multi_max() { return (size_t)tuning(TUNE_MSM_MULTI_MAX); }

// Claims the scratch set of the next MSM on stream s and orders s after that set's previous tail
// (the caller stages converted bases in its conv buffer before the MSM is enqueued; the MSM then
// runs on the same set, msm_device's preset).
int msm_claim_set(DeviceState* st, hipStream_t s, int* set, DevBuf** conv) {
    MsmPipe& PP = g_msm_pipe[st->device & 63];
    HALO_CHECK(pipe_init(PP));
    *set = msm_pick_set(PP, s, true);
    MsmScratch& M = PP.set[*set];
    if (M.tail_pending) HALO_HIP(hipStreamWaitEvent(s, M.tail_done, 0));
    *conv = &M.conv;
    return HALO_OK;
}

// Makes `s` wait (device-side) for the tails of the MSMs enqueued on `s` that are still in flight.
// Forgets which issuing streams own the two scratch-set slots and restarts each slot at its first set
// (only when no set's tail is still running; every set still waits for its own previous tail when
// reused).  An IPA opening calls it before its first two-stream round, so its two streams claim the
// same sets in the same order however many MSMs earlier callers issued on which streams (measured: after
// 23 two-stream MSMs the 2^20 opening took 21.7-22.6 ms, after 32 -- or after a reset -- 19.6-20.0).
void msm_slots_reset(DeviceState* st) {
    MsmPipe& P = g_msm_pipe[st->device & 63];
    for (const auto& m : P.set)
        if (set_busy(m)) return;
    for (int k = 0; k < 2; k++) {
        P.slot_owner[k] = nullptr;
        P.slot_next[k] = 0;
        P.slot_used[k] = 0;
    }
    P.clock = 0;
}

int msm_join(DeviceState* st, hipStream_t s) {
    MsmPipe& PP = g_msm_pipe[st->device & 63];
    for (auto& m : PP.set)
        if (m.tail_pending && m.owner == s) HALO_HIP(hipStreamWaitEvent(s, m.tail_done, 0));
    return HALO_OK;
}

int msm_device(DeviceState* st, int curve, const void* bases_int, const void* scalars_ark, size_t n,
               const void* hide_table, const void* hide_scalar, void* d_out_wrapped, hipStream_t s, const MsmOpts& o) {
    int rc;
    DISPATCH_CURVE(curve, Cv, {
        rc = msm_device_t<Cv>(st, (const uint4*)bases_int, false, 0, (const uint4*)scalars_ark, n, 0,
                              (const uint4*)hide_table, (const uint4*)hide_scalar, (uint4*)d_out_wrapped, s, o);
    });
    return rc;
}

// MSM over the resident SRS prefix Gs[0..n): uses the window-shifted copies when present.
int msm_srs_device(DeviceState* st, int curve, const void* scalars_ark, size_t n, const void* hide_scalar,
                   void* d_out_wrapped, hipStream_t s, const MsmOpts& o) {
    SrsState& srs = st->srs[curve];
    if (n > srs.n) return set_error(HALO_ESRSRANGE, "n (%zu) exceeds the resident SRS length (%zu)", n, srs.n);
    const void* table = hide_scalar ? srs.s_table.ptr : nullptr;
    if (hide_scalar && !srs.has_sh) return set_error(HALO_ESRSRANGE, "hiding commitment needs S: upload (S, H)");
    if (!o.async && n >= 1 && n <= srs_small_max())
        return msm_srs_small(st, curve, scalars_ark, n, hide_scalar, d_out_wrapped, s, o.out_xyzz);
    MsmOpts od = o.async ? MsmOpts::Async() : MsmOpts::Sync();
    od.out_xyzz = o.out_xyzz;
    int rc;
    // the shifted copies hold W windows of srs.n points each; an MSM of n <= srs.n points uses the
    // prefix of every window (point index w * srs.n + i)
    const bool use_shifted = srs.shifted_c != 0;
    DISPATCH_CURVE(curve, Cv, {
        rc = msm_device_t<Cv>(st, use_shifted ? srs.shifted.as<const uint4>() : srs.gs.as<const uint4>(), use_shifted,
                              srs.n, (const uint4*)scalars_ark, n, use_shifted ? srs.shifted_c : 0, (const uint4*)table,
                              (const uint4*)hide_scalar, (uint4*)d_out_wrapped, s, od);
    });
    return rc;
}

int msm_srs_range_device(DeviceState* st, int curve, size_t offset, const void* scalars_ark, size_t n, const void* hide_table,
                         const void* hide_scalar, void* d_out_wrapped, hipStream_t s, const MsmOpts& o) {
    SrsState& srs = st->srs[curve];
    const uint32_t blk_lg = o.blk_lg;
    if (!srs.shifted_c) return set_error(HALO_EINVAL, "msm_srs_range_device: no window-shifted SRS");
    // highest point touched: offset + map(n - 1), map(i) = i + (i >> blk_lg) << blk_lg
    const size_t last = n ? (n - 1) + (blk_lg < 32 ? ((n - 1) >> blk_lg) << blk_lg : 0) : 0;
    if (n && offset + last >= srs.n)
        return set_error(HALO_ESRSRANGE, "range [%zu, %zu] exceeds the SRS (%zu)", offset, offset + last, srs.n);
    if (n >= (1u << 31)) return set_error(HALO_EINVAL, "msm_srs_range_device: n too large");
    int rc;
    // window w of point offset + i lives at shifted[w * srs.n + offset + i]: shift the base pointer
    DISPATCH_CURVE(curve, Cv, {
        rc = msm_device_t<Cv>(st, srs.shifted.as<const uint4>() + 4 * offset, true, srs.n, (const uint4*)scalars_ark, n,
                              srs.shifted_c, (const uint4*)hide_table, (const uint4*)hide_scalar,
                              (uint4*)d_out_wrapped, s, o);
    });
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Batched MSM with shared scalars (the IPA's switch from weighted to tail rounds, ipa.hip):
//   out[i] = sum_{u < T} w[u] bases[i + u len],  i < len.
// Every output has the same digit lists, so there is no sort: one workgroup groups the (window,
// scalar) digits by bucket (counting sort in LDS, k_batch_lists), and k_batch_expand replicates that
// order for every output (key = (i W + win) B + b, value = base index i + u len) -- exactly the
// sorted layout k_acc and the reduction tail take, with SW = len W windows of B buckets.  A batched
// Horner (one lane per output) finishes.
// ---------------------------------------------------------------------------------------------
constexpr int BATCH_C_MAX = 8;  // unshifted window bits: at most 32 windows of 128 buckets
constexpr uint32_t BATCH_B_MAX = 256;  // buckets per window (shifted: two 8-bit sub-digit windows)

__global__ __launch_bounds__(256) void k_batch_lists(const uint32_t* digits, uint32_t T, int W, uint32_t B,
                                                     uint32_t len, uint32_t* ent, uint32_t* ekey, uint32_t* tot) {
    __shared__ uint32_t cnt[BATCH_B_MAX + 1];
    __shared__ uint32_t base;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) base = 0;
    for (int w = 0; w < W; w++) {
        for (uint32_t b = tid; b < B; b += blockDim.x) cnt[b] = 0;
        __syncthreads();
        for (uint32_t u = tid; u < T; u += blockDim.x) {
            const uint32_t d = digits[(size_t)w * T + u];
            if (d != DIGIT_NONE) atomicAdd(&cnt[d & 0x7fffffffu], 1u);
        }
        __syncthreads();
        if (tid == 0) {  // exclusive scan over the B buckets, continuing after the previous windows
            uint32_t run = base;
            for (uint32_t b = 0; b < B; b++) {
                const uint32_t c = cnt[b];
                cnt[b] = run;
                run += c;
            }
            cnt[B] = run;
        }
        __syncthreads();
        for (uint32_t u = tid; u < T; u += blockDim.x) {
            const uint32_t d = digits[(size_t)w * T + u];
            if (d == DIGIT_NONE) continue;
            const uint32_t b = d & 0x7fffffffu;
            const uint32_t pos = atomicAdd(&cnt[b], 1u);
            ent[pos] = u | (d & 0x80000000u);
            ekey[pos] = (uint32_t)w * B + b;
        }
        __syncthreads();
        if (tid == 0) base = cnt[B];
        __syncthreads();
    }
    if (tid == 0) {
        tot[0] = base;        // entries per output
        tot[1] = base * len;  // entries in total (k_acc's count)
    }
}

// entry e of the lists: scalar u = e & tmask of shifted copy e >> tlog (tlog 31: no copies)
__global__ __launch_bounds__(256) void k_batch_expand(const uint32_t* ent, const uint32_t* ekey, const uint32_t* tot,
                                                      uint32_t len, uint32_t WB, uint32_t tlog, uint32_t wstride,
                                                      uint32_t* keys, uint32_t* vals) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t per = tot[0];
    if (per == 0 || p >= per * len) return;
    const uint32_t i = p / per, r = p - i * per;
    const uint32_t e = ent[r], ee = e & 0x7fffffffu;
    keys[p] = i * WB + ekey[r];
    vals[p] = (i + (ee & ((1u << tlog) - 1u)) * len + (ee >> tlog) * wstride) | (e & 0x80000000u);
}

// Shifted-SRS batches: the signed c_s-bit digit of (copy w, scalar u) -> nsub unsigned sub-digits
// d_0 + 2^cb d_1 (+ 2^(2 cb) d_2) of its magnitude (mag <= 2^(c_s - 1) <= 2^(nsub cb)), window q at
// sub[q][w T + u] (its sign carried along; DIGIT_NONE for 0).  Sub-digit values run 1 .. 2^cb (bucket
// v - 1 of B = 2^cb): the one magnitude whose top sub-digit would be 2^cb, mag = 2^(nsub cb), is written
// as top = 2^cb - 1 and 2^cb in the sub-digit below.  Two sub-digits while 2^(c_s / 2) <= BATCH_B_MAX
// (c_s <= 17), three above (window widths 18-20 would otherwise need 512-1024 buckets).
// (Round 4: two windows of 2^8 buckets instead of three of 2^6 at c_s = 17 -- a third fewer bucket
// additions, the dominant cost of the IPA's switch to the tail rounds: 47M -> 31M at 2^20.)
__global__ __launch_bounds__(256) void k_batch_subdigits(const uint32_t* digits, uint32_t TW, int cb, int nsub,
                                                         uint32_t* sub) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= TW) return;
    const uint32_t d = digits[e];
    const uint32_t mag = d == DIGIT_NONE ? 0u : (d & 0x7fffffffu) + 1u, sign = d & 0x80000000u;
    const uint32_t full = 1u << cb;
    uint32_t q[3];
    q[0] = mag & (full - 1u);
    q[1] = nsub == 2 ? mag >> cb : (mag >> cb) & (full - 1u);
    q[2] = nsub == 2 ? 0u : mag >> (2 * cb);
    if (q[nsub - 1] == full) {
        q[nsub - 1] = full - 1u;
        q[nsub - 2] += full;
    }
    for (int k = 0; k < nsub; k++) sub[(size_t)k * TW + e] = q[k] ? ((q[k] - 1u) | sign) : DIGIT_NONE;
}

template <class Cv>
__global__ __launch_bounds__(64) void k_batch_horner(const uint4* window_sums, uint32_t len, int W, int c,
                                                     uint4* out, int xyzz_out) {
    using F = typename Cv::Base;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const uint4* ws = window_sums + 8 * (size_t)i * W;
    XYZZ<F> h = xyzz_id<F>();
    for (int w = W - 1; w >= 0; w--) {
        if (w != W - 1 && !xyzz_is_id(h)) {
            Jac<F> j = jac_from_xyzz(h);
            for (int k = 0; k < c; k++) j = jac_dbl(j);
            h = jac_to_xyzz(j);
        }
        h = xyzz_add(h, xyzz_load<F>(ws + 8 * w));
    }
    if (xyzz_out)
        xyzz_store(out + 8 * (size_t)i, h);
    else
        aff_store(out + 4 * (size_t)i, xyzz_to_aff(h));
}

template <class Cv>
static int msm_shared_batch_t(DeviceState* st, const uint4* bases, const uint4* w_ark, size_t T, size_t len,
                              uint4* out, bool xyzz_out, BatchScratch& S, hipStream_t s, size_t shift_stride, int c_s) {
    if (!T || !len) return set_error(HALO_EINVAL, "msm_shared_batch: empty batch");
    // shifted: the lists run over TS = W_s T (copy, scalar) entries with nsub sub-digit windows of
    // 2^cb buckets (magnitudes 1..2^(c_s-1) <= 2^(nsub cb), k_batch_subdigits)
    const bool shifted = shift_stride && c_s && (T & (T - 1)) == 0 &&
                         (size_t)msm_windows(c_s) * shift_stride < (1ull << 31);
    const int W_s = shifted ? msm_windows(c_s) : 1;
    const int nsub = (shifted && (1u << (c_s / 2)) > BATCH_B_MAX) ? 3 : 2;
    const int cb = shifted ? (nsub == 2 ? c_s / 2 : (c_s + 1) / 3) : 0;
    // unshifted window bits: about T / 4 buckets per window, so that the per-window reduction
    // (2 B additions) stays below the accumulation (T mixed additions)
    const int c = shifted ? cb : std::max(5, std::min(BATCH_C_MAX, (int)ilog2(std::max<size_t>(T, 2)) - 1));
    const int W = shifted ? nsub : msm_windows(c);
    const uint32_t B = shifted ? 1u << cb : 1u << (c - 1);
    const size_t TS = (size_t)W_s * T;
    const size_t SW = len * (size_t)W, NB = SW * B, E = SW * TS;
    if (E >= (1ull << 32) || T * len >= (1ull << 31) || B > BATCH_B_MAX)
        return set_error(HALO_EINVAL, "msm_shared_batch: batch too large (len %zu, T %zu)", len, T);
    const MsmPlan pl = msm_plan(E, NB, (int)SW, B, c, st->num_cu, W, TS);
    HALO_CHECK(S.digits.reserve((size_t)(shifted ? W_s + W : W) * TS * 4));
    HALO_CHECK(S.lists.reserve((size_t)W * TS * 8 + 16));
    HALO_CHECK(S.keys.reserve(acc_entries_bytes(E)));  // whole groups of four: k_acc's 16-byte loads
    HALO_CHECK(S.vals.reserve(acc_entries_bytes(E)));
    HALO_CHECK(plan_reserve(S, pl, 0));
    uint32_t* ent = S.lists.as<uint32_t>();
    uint32_t* ekey = ent + (size_t)W * TS;
    uint32_t* tot = ekey + (size_t)W * TS;

    const uint32_t* lists_in = S.digits.as<const uint32_t>();
    if (shifted) {
        hipLaunchKernelGGL(k_digits<typename Cv::Scalar>, dim3(grid_for(T, 256)), dim3(256), 0, s, w_ark, T, c_s, W_s,
                           S.digits.as<uint32_t>(), T, 0, W_s);
        uint32_t* sub = S.digits.as<uint32_t>() + TS;
        hipLaunchKernelGGL(k_batch_subdigits, dim3(grid_for(TS, 256)), dim3(256), 0, s, S.digits.as<const uint32_t>(),
                           (uint32_t)TS, cb, nsub, sub);
        lists_in = sub;
    } else {
        hipLaunchKernelGGL(k_digits<typename Cv::Scalar>, dim3(grid_for(T, 256)), dim3(256), 0, s, w_ark, T, c, W,
                           S.digits.as<uint32_t>(), T, 0, W);
    }
    hipLaunchKernelGGL(k_batch_lists, dim3(1), dim3(256), 0, s, lists_in, (uint32_t)TS, W, B, (uint32_t)len, ent, ekey,
                       tot);
    hipLaunchKernelGGL(k_batch_expand, dim3(grid_for(E, 256)), dim3(256), 0, s, (const uint32_t*)ent,
                       (const uint32_t*)ekey, (const uint32_t*)tot, (uint32_t)len, (uint32_t)(W * B),
                       shifted ? (uint32_t)ilog2(T) : 31u, shifted ? (uint32_t)shift_stride : 0u,
                       S.keys.as<uint32_t>(), S.vals.as<uint32_t>());
    // the entry values are point indices already; tot[1]: the entries in total
    AccArgs a{S.keys.as<const uint32_t>(), S.vals.as<const uint32_t>(), tot + 1, bases};
    a.profiled = false;
    HALO_CHECK(acc_launch<Cv>(pl, S, a, s));
    MsmTailArgs ta = plan_tail_args(st, pl, S, T, S.keys.as<const uint32_t>(), tot + 1);
    ta.batch_windows = true;  // k_batch_window_sums needs no grid scratch
    HALO_CHECK(msm_tail_launch(curve_id<Cv>(), ta, s));
    hipLaunchKernelGGL(k_batch_horner<Cv>, dim3(grid_for(len, 64)), dim3(64), 0, s, S.window_sums.as<const uint4>(),
                       (uint32_t)len, W, c, out, (int)xyzz_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int msm_shared_batch(DeviceState* st, int curve, const void* bases_int, const void* w_ark, size_t T, size_t len,
                     void* out, bool xyzz_out, BatchScratch& S, hipStream_t s, size_t shift_stride, int c_s) {
    int rc;
    DISPATCH_CURVE(curve, Cv, {
        rc = msm_shared_batch_t<Cv>(st, (const uint4*)bases_int, (const uint4*)w_ark, T, len, (uint4*)out, xyzz_out,
                                    S, s, shift_stride, c_s);
    });
    return rc;
}

// ark Projective (Jacobian X, Y, Z, Montgomery, 96 B) -> internal affine; Z = 0 -> (0, 0).  One
// Fermat inversion per lane (Projective::normalize_batch of point_dot, group.rs:53-56).
template <class Cv>
__global__ void k_jacobian_to_internal(const uint4* in, uint4* out, size_t n) {
    using F = typename Cv::Base;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fe<F> Z = fe_from_ark<F>(in + 6 * i + 4);
    Affine<F> a;
    if (fe_is_zero(Z)) {
        a.x = fe_zero<F>();
        a.y = fe_zero<F>();
    } else {
        const Fe<F> zi = fe_inv(Z);
        const Fe<F> zi2 = fe_sqr(zi);
        a.x = fe_mul(fe_from_ark<F>(in + 6 * i), zi2);
        a.y = fe_mul(fe_from_ark<F>(in + 6 * i + 2), fe_mul(zi2, zi));
    }
    aff_store(out + 4 * i, a);
}

// k commitments over the resident SRS prefix (lens[i] scalars at d_scalars[i]) -> d_out + 64 i,
// asynchronous on s (msm_join before reading)
int msm_batch_device(DeviceState* st, int curve, const void* const* d_scalars, const size_t* lens, size_t k, void* d_out,
                     hipStream_t s) {
    SrsState& srs = st->srs[curve];
    size_t nmax = 0;
    for (size_t i = 0; i < k; i++) {
        if (lens[i] && !d_scalars[i]) return set_error(HALO_EINVAL, "halo_msm_batch_dev: null scalars %zu", i);
        if (lens[i] > srs.n) return set_error(HALO_ESRSRANGE, "n (%zu) exceeds the resident SRS length (%zu)", lens[i], srs.n);
        nmax = std::max(nmax, lens[i]);
    }
    // (Measured and removed: the fronts on a side stream beside the accumulations -- slower, the
    // sort kernels starve beside k_acc's gathers)
    if (k > 1 && srs.shifted_c && nmax <= msm_multi_max()) {
        int rc;
        DISPATCH_CURVE(curve, Cv, { rc = msm_multi_device_t<Cv>(st, d_scalars, lens, k, (uint4*)d_out, s); });
        return rc;
    }
    for (size_t i = 0; i < k; i++)
        HALO_CHECK(msm_srs_device(st, curve, d_scalars[i], lens[i], nullptr, (char*)d_out + 64 * i, s, MsmOpts::Async()));
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_msm_window_bits(size_t n) { return msm_window_bits(n); }

// group::point_dot(xs, &[Projective]) (crates/group/src/group.rs:53-56): the bases arrive as ark
// Projective (Jacobian) points, normalised on the device, then the MSM of halo_msm.
extern "C" int halo_point_dot_projective(halo_curve_t curve, const halo_fe_t* scalars, size_t n_scalars,
                                         const uint64_t (*bases)[12], size_t n_bases, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    const size_t n = std::min(n_bases, n_scalars);
    if (!out || (n && (!bases || !scalars))) return set_error(HALO_EINVAL, "halo_point_dot_projective: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(n, 1) * 96));
    HALO_CHECK(st->scratch[1].reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(st->scratch[2].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[3].reserve(128));
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, bases, n * 96, s));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, scalars, n * 32, s));
    if (n) {
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_jacobian_to_internal<Cv>, dim3(grid_for(n, 256)), dim3(256), 0, s,
                               st->scratch[0].as<const uint4>(), st->scratch[1].as<uint4>(), n);
        });
        HALO_HIP(hipGetLastError());
    }
    HALO_CHECK(msm_device(st, curve, st->scratch[1].ptr, st->scratch[2].ptr, n, nullptr, nullptr, st->scratch[3].ptr, s,
                          MsmOpts::Sync().xyzz()));
    return d2h_point(curve, st->scratch[3].ptr, out, s);
}

// host arrays: bases (ark WrappedPoint), scalars (ark) -> out (host)
extern "C" int halo_msm(halo_curve_t curve, const halo_wrapped_point_t* bases, size_t n_bases,
                        const halo_fe_t* scalars, size_t n_scalars, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    const size_t n = std::min(n_bases, n_scalars);
    if (!out || (n && (!bases || !scalars))) return set_error(HALO_EINVAL, "halo_msm: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(st->scratch[1].reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(st->scratch[2].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[3].reserve(128));
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, bases, n * 64, s));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, scalars, n * 32, s));
    HALO_CHECK(convert_wrapped_to_internal(curve, st->scratch[0].ptr, st->scratch[1].ptr, n, s));
    if (n >= 1 && n <= msm_tiny_max()) {  // a few points: GLV windows + one 32-window Horner (tail.hip)
        HALO_CHECK(st->scratch[3].reserve(128 + 32 * 128));
        HALO_CHECK(msm_tiny(curve, st->scratch[1].ptr, st->scratch[2].ptr, n, st->scratch[3].as<char>() + 128,
                            st->scratch[3].ptr, s));
    } else {
        HALO_CHECK(msm_device(st, curve, st->scratch[1].ptr, st->scratch[2].ptr, n, nullptr, nullptr, st->scratch[3].ptr,
                              s, MsmOpts::Sync().xyzz()));
    }
    return d2h_point(curve, st->scratch[3].ptr, out, s);
}

extern "C" int halo_msm_srs(halo_curve_t curve, const halo_fe_t* scalars, size_t n, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!out || (n && !scalars)) return set_error(HALO_EINVAL, "halo_msm_srs: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[2].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[3].reserve(128));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, scalars, n * 32, s));
    HALO_CHECK(msm_srs_device(st, curve, st->scratch[2].ptr, n, nullptr, st->scratch[3].ptr, s, MsmOpts::Sync().xyzz()));
    return d2h_point(curve, st->scratch[3].ptr, out, s);
}

extern "C" int halo_msm_dev(halo_curve_t curve, const void* d_bases, const void* d_scalars, size_t n,
                            halo_wrapped_point_t* out, void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!out || (n && !d_scalars)) return set_error(HALO_EINVAL, "halo_msm_dev: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[7].reserve(128));
    if (!d_bases) {
        HALO_CHECK(msm_srs_device(st, curve, d_scalars, n, nullptr, st->scratch[7].ptr, s, MsmOpts::Sync().xyzz()));
    } else {
        HALO_CHECK(st->scratch[6].reserve(std::max<size_t>(n, 1) * 64));
        HALO_CHECK(convert_wrapped_to_internal(curve, d_bases, st->scratch[6].ptr, n, s));
        HALO_CHECK(msm_device(st, curve, st->scratch[6].ptr, d_scalars, n, nullptr, nullptr, st->scratch[7].ptr, s,
                              MsmOpts::Sync().xyzz()));
    }
    return d2h_point(curve, st->scratch[7].ptr, out, s);
}

extern "C" int halo_msm_dev_async(halo_curve_t curve, const void* d_bases, const void* d_scalars, size_t n,
                                  void* d_out, void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!d_out || (n && !d_scalars)) return set_error(HALO_EINVAL, "halo_msm_dev_async: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    if (!d_bases) return msm_srs_device(st, curve, d_scalars, n, nullptr, d_out, s, MsmOpts::Async());
    // the set is claimed once: its previous tail is waited for before the conversion overwrites conv,
    // and the MSM runs on that same set
    int set = -1;
    DevBuf* conv = nullptr;
    HALO_CHECK(msm_claim_set(st, s, &set, &conv));
    HALO_CHECK(conv->reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(convert_wrapped_to_internal(curve, d_bases, conv->ptr, n, s));
    return msm_device(st, curve, conv->ptr, d_scalars, n, nullptr, nullptr, d_out, s, MsmOpts::Async().on_set(set));
}

extern "C" int halo_msm_batch_dev(halo_curve_t curve, const void* const* d_scalars, const size_t* lens, size_t k,
                                  void* d_out, void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (k && (!d_scalars || !lens || !d_out)) return set_error(HALO_EINVAL, "halo_msm_batch_dev: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return msm_batch_device(st, curve, d_scalars, lens, k, d_out, (hipStream_t)stream);
}

// One rank's share of a window-partitioned MSM over the resident window-shifted SRS (BASELINE
// configs[4]): the digits of windows [w_lo, w_hi) only, against the copies 2^(c w) G, w in range; the
// partials of a partition of [0, W) sum to the MSM.  Asynchronous like halo_msm_dev_async.
extern "C" int halo_msm_srs_windows_dev(halo_curve_t curve, const void* d_scalars, size_t n, int w_lo, int w_hi,
                                        void* d_out, void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!d_out || (n && !d_scalars)) return set_error(HALO_EINVAL, "halo_msm_srs_windows_dev: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    // the full set of copies, or this rank's range of them (halo_srs_precompute_window_range)
    const int c = srs.shifted_c ? srs.shifted_c : srs.part_c;
    const int w0 = srs.shifted_c ? 0 : srs.part_w0, w1 = srs.shifted_c ? msm_windows(c) : srs.part_w1;
    if (!c) return set_error(HALO_EINVAL, "halo_msm_srs_windows_dev: no window-shifted SRS");
    if (n > srs.n) return set_error(HALO_ESRSRANGE, "n (%zu) exceeds the resident SRS length (%zu)", n, srs.n);
    if (w_hi <= w_lo) return set_error(HALO_EINVAL, "empty window range [%d, %d)", w_lo, w_hi);
    if (w_lo < w0 || w_hi > w1)
        return set_error(HALO_EINVAL, "window range [%d, %d) not resident (copies of [%d, %d))", w_lo, w_hi, w0, w1);
    int rc;
    DISPATCH_CURVE(curve, Cv, {
        rc = msm_device_t<Cv>(st, srs.shifted.as<const uint4>(), true, srs.n, (const uint4*)d_scalars, n, c, nullptr,
                              nullptr, (uint4*)d_out, (hipStream_t)stream, MsmOpts::Async(),
                              MsmWindowRange{w_lo, w_hi, w0});
    });
    return rc;
}

extern "C" int halo_srs_windows(halo_curve_t curve) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    const SrsState& srs = st->srs[curve];
    const int c = srs.shifted_c ? srs.shifted_c : srs.part_c;
    return c ? msm_windows(c) : 0;
}

extern "C" int halo_msm_join(void* stream) {
    clear_error();
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    return msm_join(st, (hipStream_t)stream);
}

// pedersen::commit(w, Gs, ms) -- crates/accumulation/src/pedersen.rs:7-27
extern "C" int halo_pedersen_commit(halo_curve_t curve, const halo_fe_t* w, const halo_wrapped_point_t* gs,
                                    size_t n_gs, const halo_fe_t* ms, size_t n_ms, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!out || (n_ms && !ms) || (n_gs && !gs)) return set_error(HALO_EINVAL, "halo_pedersen_commit: null buffer");
    if (n_gs < n_ms)
        return set_error(HALO_ELENGTH, "ms must be larger than Gs: (Gs: %zu), (ms: %zu)", n_gs, n_ms);
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (w && !srs.has_sh) return set_error(HALO_ESRSRANGE, "hiding commitment needs S: upload the SRS (S, H) first");
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t n = n_ms;
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(st->scratch[1].reserve(std::max<size_t>(n, 1) * 64));
    HALO_CHECK(st->scratch[2].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[3].reserve(128 + 32));
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, gs, n * 64, s));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, ms, n * 32, s));
    HALO_CHECK(convert_wrapped_to_internal(curve, st->scratch[0].ptr, st->scratch[1].ptr, n, s));
    char* small = (char*)st->scratch[3].ptr;  // [0, 128) the XYZZ sum, [128, 160) w
    if (w) HALO_CHECK(copy_h2d(small + 128, w, 32, s));
    HALO_CHECK(msm_device(st, curve, st->scratch[1].ptr, st->scratch[2].ptr, n, w ? srs.s_table.ptr : nullptr,
                          w ? small + 128 : nullptr, small, s, MsmOpts::Sync().xyzz()));
    return d2h_point(curve, small, out, s);
}

static size_t poly_degree(const halo_fe_t* c, size_t len) {
    // DensePolynomial::degree(): index of the last nonzero coefficient (0 for the zero polynomial)
    size_t n = len;
    while (n > 0 && !(c[n - 1].l[0] | c[n - 1].l[1] | c[n - 1].l[2] | c[n - 1].l[3])) n--;
    return n ? n - 1 : 0;
}

// pcdl::commit(p, d, w) -- crates/accumulation/src/pcdl.rs:275-287
extern "C" int halo_pcdl_commit(halo_curve_t curve, const halo_fe_t* coeffs, size_t len, size_t d,
                                const halo_fe_t* w, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!out || (len && !coeffs)) return set_error(HALO_EINVAL, "halo_pcdl_commit: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (!srs.n) return set_error(HALO_ESRSRANGE, "no resident SRS: call halo_srs_upload first");
    const size_t D = srs.n - 1;
    const size_t n = d + 1;
    const size_t p_deg = poly_degree(coeffs, len);
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    if (p_deg > d) return set_error(HALO_EDEGREE, "p_deg (%zu) <= d (%zu)", p_deg, d);
    if (d > D) return set_error(HALO_ESRSRANGE, "d (%zu) <= D (%zu) (pp_len = %zu)", d, D, D + 1);
    if (w && !srs.has_sh) return set_error(HALO_ESRSRANGE, "hiding commitment needs S: upload the SRS (S, H) first");
    // coefficients past the degree are zero and contribute nothing to the MSM
    const size_t m = std::min(len, n);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[2].reserve(std::max<size_t>(m, 1) * 32));
    HALO_CHECK(st->scratch[3].reserve(128 + 32));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, coeffs, m * 32, s));
    char* small = (char*)st->scratch[3].ptr;  // [0, 128) the XYZZ sum, [128, 160) w
    if (w) HALO_CHECK(copy_h2d(small + 128, w, 32, s));
    HALO_CHECK(msm_srs_device(st, curve, st->scratch[2].ptr, m, w ? small + 128 : nullptr, small, s,
                              MsmOpts::Sync().xyzz()));
    return d2h_point(curve, small, out, s);
}
