// Every host-side decision of a device NTT (ntt.hip) as one value: the pass split, the zero-tail pruning of
// pass 0, each pass's launch geometry and buffers, and which pre-twiddle tables exist.  Host-only and free of
// HIP types, so a plain C++17 compiler builds it (tests/test_ntt_plan.py sweeps it on the CPU).  ntt.hip performs
// what the records say and decides nothing itself.
//
// The two tunings ("ntt_big_max_log", "ntt_even_split") are arguments: ntt.hip reads them once per transform and
// hands the plan down, so a concurrent halo_set_tuning cannot pair the tables built for one split with the passes
// of another, nor the span halo_ntt_dev_zero_tail clears with another pass 0.
//
// What holds for every plan of ntt_plan (log n <= NTT_MAX_LOG_N); the sweep checks each line:
//   * log n = 0 has no pass (the transform is a copy); otherwise there are 1..NTT_MAX_PASSES passes, every radix
//     log_r is in [1, NTT_MAX_LOG_R_BIG], and the radices sum to log n;
//   * a radix of at most NTT_MAX_LOG_R_MULTI runs on NTT_E-element blocks, a larger one on NTT_E_BIG: the ranges
//     (r = 1..8 on 1024, r = 9..11 on 2048) over which ntt.hip's NttSwz constants were searched conflict-free;
//   * a transform with per-pass tables (log n <= NTT_FULL_TABLE_MAX_LOG) has at most NTT_MAX_PASSES passes, one slot
//     of DeviceState::Twiddles::pass each, and a radix fits the NTT_KEY_BITS bits the cache key gives it;
//   * prune is 0 or in [ntt_g0(ne, log_r), log_r): the kernel skips ntt_first when it prunes, so the pruned stages
//     must cover the first register group; on the wide blocks log_r - prune is then even, because a trailing
//     one-stage group of a one-column block would reach past the column;
//   * out_scaled holds exactly on the last pass of a transform with tables and more than one pass: that pass's
//     table carries the output constant, so the kernel multiplies the rho = 0 inputs by it and no output;
//   * passes chain (each source is the previous destination), the last destination is Out, and Tmp2 is only ever
//     pass 0's destination, and only in place;
//   * no pass reads and writes one buffer (In and Out are one buffer in place), except the single pass of an in-place
//     transform of log n <= 8.  That one is safe because grid_x = 1: one workgroup holds the whole transform in LDS
//     and has read every input before its first store (the barriers between the phases).
#pragma once
#include <cstddef>
#include <cstdint>

namespace halo {

constexpr int NTT_E = 1024;      // elements per workgroup for passes with R <= 256
constexpr int NTT_E_BIG = 2048;  // ... and for the two-pass split of 2^17..2^22 (R up to 2048)
// Elements per thread: radix-4 register groups, two stages per LDS round trip.  (Round 3 measured radix-8
// groups on the 2048-element blocks -- 4 LDS round trips per 11-bit pass instead of 6 -- slower: 192 VGPRs
// leave 2 waves per SIMD and the barrier waits were hidden worse than they were saved.)
constexpr int NTT_EPT = 4;
constexpr int NTT_MAX_LOG_R_MULTI = 8;
constexpr unsigned NTT_MAX_LOG_R_BIG = 11;
constexpr unsigned NTT_FULL_TABLE_MAX_LOG = 24;  // per-pass twiddle tables up to 2^24
constexpr unsigned NTT_LDS_BYTES_PER_ELEM = 36;  // 9 limbs of 4 B, limb-major
constexpr unsigned NTT_MAX_LOG_N = 30;
constexpr size_t NTT_MAX_BATCH = 65535;  // a batch is the launch's grid.y
constexpr unsigned NTT_MAX_PASSES = 4;
constexpr unsigned NTT_KEY_BITS = 5;  // per pass in NttPlan::split_key

static_assert((1 << NTT_MAX_LOG_R_MULTI) <= NTT_E && (1u << NTT_MAX_LOG_R_BIG) <= (unsigned)NTT_E_BIG,
              "a column of a pass fits its block");
static_assert(NTT_MAX_PASSES * NTT_MAX_LOG_R_MULTI >= NTT_MAX_LOG_N, "passes of <= 8 bits reach the largest domain");
static_assert(2 * NTT_MAX_LOG_R_BIG <= NTT_FULL_TABLE_MAX_LOG && NTT_FULL_TABLE_MAX_LOG <= NTT_MAX_LOG_N,
              "every transform that gets tables has at most NTT_MAX_PASSES passes");
static_assert(NTT_MAX_LOG_R_BIG < (1u << NTT_KEY_BITS) && NTT_MAX_PASSES * NTT_KEY_BITS <= 64, "the split fits its key");

// The block a pass of radix 2^log_r runs on
constexpr int ntt_block(unsigned log_r) { return log_r > (unsigned)NTT_MAX_LOG_R_MULTI ? NTT_E_BIG : NTT_E; }

// Stages of a pass's first register group, done straight from the loads (k_ntt_pass G0; tools/ntt_model.py
// restates it): on the wide blocks the short group goes first (r mod 2 stages), so later groups stay in range.
constexpr unsigned ntt_g0(int ne, unsigned r) { return (ne >= NTT_E_BIG && (r & 1u)) ? 1u : (r < 2u ? r : 2u); }

// Pass split: N <= 2^8 in one pass; 2^17..2^22 in two passes of up to 11 bits on 2048-element
// blocks (one fewer pass than the 8-bit split: one pre-twiddle multiplication and one HBM round
// trip per element saved; measured A/B on one box: 2^20 pair 0.28 -> 0.25 ms, 2^22 equal at
// 1.03 ms, where the single-column 11-bit pass loses on its strided 32-B loads what it saves in
// work); everything else in passes of <= 8 bits on 1024-element blocks.  big_max_log above 22 acts as 22.
struct NttSplit {
    unsigned npass = 0;
    unsigned log_r[NTT_MAX_PASSES] = {};
};
inline NttSplit ntt_split(unsigned logn, long long big_max_log, bool even_split) {
    constexpr unsigned M = NTT_MAX_LOG_R_MULTI;
    NttSplit sp;
    if (logn == 0) return sp;
    if (logn <= M) {
        sp.npass = 1;
        sp.log_r[0] = logn;
        return sp;
    }
    if (logn >= 17 && logn <= 2 * NTT_MAX_LOG_R_BIG && (long long)logn <= big_max_log) {
        sp.npass = 2;
        sp.log_r[0] = (logn + 1) / 2;
        sp.log_r[1] = logn / 2;
        return sp;
    }
    const unsigned passes = sp.npass = (logn + M - 1) / M;
    if (even_split) {
        // even radices where possible (an odd pass ends in a one-stage group: a whole LDS round trip
        // and normalization for half a group's butterflies): 8s, trimmed by 2 from the back, at most
        // one odd pass (2^22 = 8 + 8 + 6, 2^23 = 8 + 8 + 7)
        for (unsigned p = 0; p < passes; p++) sp.log_r[p] = M;
        unsigned excess = passes * M - logn;
        for (unsigned k = passes; excess >= 2; k = (k == 1 ? passes : k - 1)) {
            sp.log_r[k - 1] -= 2;
            excess -= 2;
        }
        if (excess) sp.log_r[passes - 1] -= 1;
        return sp;
    }
    unsigned left = logn;
    for (unsigned p = 0; p < passes; p++) {
        sp.log_r[p] = (left + (passes - p) - 1) / (passes - p);
        left -= sp.log_r[p];
    }
    return sp;
}

// the split as one key (NTT_KEY_BITS per pass) for the twiddle-table cache
inline uint64_t ntt_split_key(const NttSplit& sp) {
    uint64_t k = 0;
    for (unsigned p = 0; p < sp.npass; p++) k = (k << NTT_KEY_BITS) | sp.log_r[p];
    return k;
}

// Stages of pass 0 (radix 2^lr) that a zero tail lets the pass skip (NttPassPlan::prune), for `request` stages
// of zeros: only when they cover its first register group; on one-column wide blocks a trailing single-stage
// group would reach past the column, so the stages left after the pruned ones must pair up (as G0 = 1 arranges).
inline unsigned ntt_pass0_prune(unsigned lr, unsigned request) {
    if (!request) return 0;
    const int ne = ntt_block(lr);
    unsigned pr = request < lr ? request : lr;
    if (ne == NTT_E_BIG && pr > 0 && ((lr - pr) & 1u)) pr--;
    return (pr >= ntt_g0(ne, lr) && pr < lr) ? pr : 0u;
}

// The buffers of a transform by role: the caller's input and output (one buffer in place), the ping-pong
// scratch, and a second scratch that takes the first pass of an in-place transform with an odd pass count
enum class NttBuf : uint8_t { In, Out, Tmp, Tmp2 };

struct NttPassPlan {
    unsigned log_r, log_ns;  // this pass's radix; the product of the earlier ones (Stockham Ns)
    int ne;                  // the block: NTT_E or NTT_E_BIG elements, ne / NTT_EPT threads, ne * 36 B of LDS
    unsigned t, grid_x;      // columns per workgroup, workgroups per transform
    bool full;               // the block's t 2^log_r positions fill all ne (k_ntt_pass FULL)
    unsigned threads, lds_bytes;
    bool in_ark, out_ark;  // the first pass reads ark words, the last writes them
    unsigned prune;        // pass 0 of a forward transform: leading stages skipped (ntt_pass0_prune)
    bool table;            // reads a per-pass pre-twiddle table (else pass 0, or the two-level lo / hi tables)
    size_t table_entries;  // ... of 2^(log_r + log_ns) entries
    bool out_scaled;       // ... that carries the output constant (NttPassArgs::out_scaled)
    NttBuf src, dst;
};

struct NttPlan {
    unsigned logn;
    bool inverse, in_place;
    unsigned npass;
    NttPassPlan pass[NTT_MAX_PASSES];
    uint64_t split_key;
    unsigned lo_bits;  // the two-level tables: omega^e for e < nlo, omega^(e nlo) for e < nhi
    size_t nlo, nhi;
    bool tables;      // per-pass tables exist
    bool needs_tmp2;  // some pass writes NttBuf::Tmp2
    size_t read_end;  // pass 0 reads the input's elements [0, read_end): N >> prune, or N
};

// The transform of 2^logn elements (logn <= NTT_MAX_LOG_N: ntt_check).  prune_request: the input's elements from
// index N >> prune_request on are zero (forward transforms only).
inline NttPlan ntt_plan(unsigned logn, bool inverse, bool in_place, unsigned prune_request, long long big_max_log,
                        bool even_split) {
    NttPlan pl{};
    pl.logn = logn;
    pl.inverse = inverse;
    pl.in_place = in_place;
    const NttSplit sp = ntt_split(logn, big_max_log, even_split);
    const unsigned P = pl.npass = sp.npass;
    pl.split_key = ntt_split_key(sp);
    pl.lo_bits = (logn + 1) / 2;
    pl.nlo = (size_t)1 << pl.lo_bits;
    pl.nhi = (size_t)1 << (logn - pl.lo_bits);
    pl.tables = logn <= NTT_FULL_TABLE_MAX_LOG;
    const size_t N = (size_t)1 << logn;
    pl.read_end = N;
    if (!P) return pl;
    unsigned log_ns = 0;
    for (unsigned p = 0; p < P; p++) {
        NttPassPlan& q = pl.pass[p];
        const unsigned lr = q.log_r = sp.log_r[p];
        q.log_ns = log_ns;
        q.ne = ntt_block(lr);
        const size_t nj = N >> lr, cols = (size_t)q.ne >> lr;  // columns of the pass, columns a block holds
        q.t = (unsigned)(nj < cols ? nj : cols);
        q.grid_x = (unsigned)(nj / q.t);
        q.full = ((size_t)q.t << lr) == (size_t)q.ne;
        q.threads = (unsigned)(q.ne / NTT_EPT);
        q.lds_bytes = (unsigned)q.ne * NTT_LDS_BYTES_PER_ELEM;
        q.in_ark = p == 0;
        q.out_ark = p == P - 1;
        q.prune = (p == 0 && !inverse) ? ntt_pass0_prune(lr, prune_request) : 0u;
        q.table = pl.tables && p > 0;  // one multiplication per element instead of two
        q.table_entries = q.table ? (size_t)1 << (lr + log_ns) : 0;
        q.out_scaled = q.table && q.out_ark;
        log_ns += lr;
    }
    if (pl.pass[0].prune) pl.read_end = N >> pl.pass[0].prune;
    // the passes ping-pong between Out and Tmp so that the last one writes Out; where that makes the first pass
    // of an in-place transform write the buffer it reads, Tmp2 takes its output
    pl.pass[P - 1].dst = NttBuf::Out;
    for (unsigned p = P - 1; p-- > 0;) pl.pass[p].dst = pl.pass[p + 1].dst == NttBuf::Out ? NttBuf::Tmp : NttBuf::Out;
    if (in_place && P > 1 && pl.pass[0].dst == NttBuf::Out) {
        pl.pass[0].dst = NttBuf::Tmp2;
        pl.needs_tmp2 = true;
    }
    for (unsigned p = 0; p < P; p++) pl.pass[p].src = p ? pl.pass[p - 1].dst : NttBuf::In;
    return pl;
}

// What an entry point refuses before it shifts by log_n, sizes a buffer or looks up the device; the entry point
// owns the message.  Empty: nothing to do, success.
enum class NttCheck { Ok, Empty, LogTooLarge, BatchTooLarge };
constexpr NttCheck ntt_check(unsigned log_n, size_t batch) {
    return log_n > NTT_MAX_LOG_N   ? NttCheck::LogTooLarge
           : batch > NTT_MAX_BATCH ? NttCheck::BatchTooLarge
           : batch == 0            ? NttCheck::Empty
                                   : NttCheck::Ok;
}

}  // namespace halo
