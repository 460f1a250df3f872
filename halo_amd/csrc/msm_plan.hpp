// The launch plan of the bucket MSM pipeline (digit recoding, sort, k_acc, reduction tail): the
// geometry, the partials layout and the scratch sizes that every host driver in msm.hip uses, stated
// once.  Host-only and free of HIP types, so a plain C++17 compiler builds it (tests/test_msm_plan.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace halo {

// Columns of the bucket reduction grid (k_rowcol): 256 x 256 at 2^16 buckets keeps the row, column
// and bit-sliced tree depths at ~9 additions each (measured against 32 columns: single-MSM latency
// 2.15 -> 2.02 ms at 2^20, IPA opening 36.8 -> 35.2 ms; the pipelined step unchanged).
constexpr int MSM_SEG_L = 256;

// chunk-partial group size of the skew guard (msm_tail.hip k_group_sums)
constexpr uint32_t MSM_GROUP = 64;

// uint4 words of one chunk partial (curve.hpp PARTIAL_U4; msm.hip asserts that the two agree)
constexpr size_t MSM_PARTIAL_U4 = 9;

inline unsigned msm_ilog2(size_t n) {  // floor(log2 n), 0 for n <= 1
    unsigned r = 0;
    while ((size_t(1) << (r + 1)) <= n) r++;
    return r;
}

// windows of c bits for scalars reduced to [0, p/2] (k_digits): 254 bits + the signed-digit carry
inline int msm_windows(int c) { return (255 + c - 1) / c; }

inline int msm_window_bits(size_t n) {
    unsigned lg = n > 1 ? msm_ilog2(n - 1) + 1 : 1;
    int c = (int)lg - 4;
    return std::max(6, std::min(16, c));
}

// window bits of the window-shifted SRS copies: one more bit than the plain MSM choice when that
// saves a window (c = 17 at 2^20: 15 windows instead of 16; the single bucket set of 2^16 buckets
// keeps the reduction and the 2-pass sort cheap)
inline int msm_shifted_window_bits(size_t n) {
    int c = msm_window_bits(n);
    if (msm_windows(c + 1) < msm_windows(c) && c + 1 <= 17) c++;
    // the top window holds only the 255 - (W - 1) c remaining bits, so its digits pile into the
    // lowest 2^(top - 1) buckets: n / 2^(top - 1) extra entries each, against W n / 2^(c - 1) on
    // average, and k_merge's longest runs (the latency of a small MSM) grow with that ratio.  Widen the
    // window until the ratio is at most 1/2 (c = 13 at 2^16: top 8 bits, ratio 1.6 -> c = 15, top 15).
    auto top_bits = [](int cc) { return 255 - (msm_windows(cc) - 1) * cc; };
    while (c < 17 && (1 << (c - top_bits(c))) * 2 > msm_windows(c)) c++;
    return c;
}

// Chunk length K of k_acc for E sorted entries.  Large MSMs (E > 16 x the resident lanes, 256 CUs x
// 16 waves x 64): >= 4 rounds of resident lanes, 16 <= K <= 64 -- every lane does the same number
// of mixed additions, and several rounds absorb the CU slots held by the previous MSM's tail kernels,
// which one exact round would not (measured: K = 60 at 2^20 is 1 round and 15 % slower than K = 16;
// round 4, pipelined 2^20 step: 2 rounds (K = 30) 1.378, 3 rounds (K = 20) 1.365, 4 rounds 1.354 ms,
// and 6 / 8 rounds (K = 10 / 8: k_acc 0.87 / 0.85 ms, but twice the chunk partials for k_merge)
// 1.362 / 1.374 ms).
// Smaller MSMs are latency-bound (a commitment, an IPA round): their critical path is a lane's K
// dependent additions in k_acc plus k_merge's run of about E / (NB K) partials per bucket, so K =
// ceil(sqrt(E / NB)) balances the two -- but at least ceil(E / resident lanes), one round.
inline uint32_t msm_chunk_len(int num_cu, size_t E, size_t NB) {
    const size_t resident = (size_t)num_cu * 16 * 64;
    if (E > 16 * resident) return (uint32_t)std::max<size_t>(16, std::min<size_t>(64, (E + 4 * resident - 1) / (4 * resident)));
    size_t k = 1;
    while (k * k * std::max<size_t>(NB, 1) < E) k++;
    return (uint32_t)std::min<size_t>(16, std::max<size_t>(k, (E + resident - 1) / resident));
}

// One MSM's plan: SW windows (bucket sets) of B buckets each, NB = SW B buckets in all, E sorted
// entries cut into nchunks chunks of K (k_acc), the chunk partials grouped by MSM_GROUP twice
// (k_group_sums), every window reduced on an H x L grid with NT bit terms (k_rowcol, k_bitterms).
// c, W (windows of the scalar recoding) and SN (entries per sort window) are the driver's own and are
// carried along for its launches; nothing else is derived from them.
struct MsmPlan {
    int c, W, SW;  // (these seven: msm_plan's arguments)
    uint32_t B;
    size_t SN, NB, E;
    uint32_t L, logL, H, logH, NT, key_bits, K;
    size_t nchunks, ng1, ng2;
    // the partials buffer, in uint4 units: first[max(nchunks, 1)], last[max(nchunks, 1)], g1[ng1 + 1],
    // g2[ng2 + 1], each entry MSM_PARTIAL_U4 words
    size_t off_first, off_last, off_g1, off_g2;
    // bytes of the scratch buffers
    size_t digits_bytes, bstart_bytes, partials_bytes, bucket_sums_bytes, rows_bytes, cols_bytes, terms_bytes;
    // the SW window sums, then hide_slots hiding terms (window_sums + 8 SW): 128 B packed XYZZ each
    size_t window_sums_bytes(size_t hide_slots) const { return ((size_t)SW + hide_slots) * 128; }
};

inline MsmPlan msm_plan(size_t E, size_t NB, int SW, uint32_t B, int c, int num_cu, int W, size_t SN) {
    MsmPlan p{c, W, SW, B, SN, NB, E};
    p.L = std::min<uint32_t>(MSM_SEG_L, B);
    p.logL = msm_ilog2(p.L);
    p.H = B / p.L;
    p.logH = msm_ilog2(p.H);
    p.NT = 1 + p.logH + p.logL;  // reduction bit terms per window (<= 64)
    p.key_bits = NB > 1 ? msm_ilog2(NB - 1) + 1 : 1;
    p.K = msm_chunk_len(num_cu, E, NB);
    p.nchunks = (E + p.K - 1) / p.K;
    p.ng1 = p.nchunks / MSM_GROUP;
    p.ng2 = p.nchunks / (MSM_GROUP * MSM_GROUP);
    const size_t slots = std::max<size_t>(p.nchunks, 1);  // (an empty MSM keeps one slot per region)
    p.off_first = 0;
    p.off_last = MSM_PARTIAL_U4 * slots;
    p.off_g1 = MSM_PARTIAL_U4 * 2 * slots;
    p.off_g2 = p.off_g1 + MSM_PARTIAL_U4 * (p.ng1 + 1);
    p.partials_bytes = (p.off_g2 + MSM_PARTIAL_U4 * (p.ng2 + 1)) * 16;
    p.digits_bytes = E * 4;
    p.bstart_bytes = (NB + 1) * 4;
    p.bucket_sums_bytes = NB * 128;
    p.rows_bytes = (size_t)SW * p.H * 128;  // row sums
    p.cols_bytes = (size_t)SW * p.L * 128;  // column sums
    p.terms_bytes = (size_t)SW * p.NT * 128;
    return p;
}

// Whether the digit recoding is fused into the sort's first pass (sort.hip k_rs_hist_sc: thread =
// scalar, round = window, no digit array written and read back), for P outputs of n scalars each.
// The one statement of the rule; msm_device_t adds what is its own (shifted bases, every window).
//   W <= 16: a tile's 16 rounds hold one scalar's windows.  Both drivers asked it.
//   P == 1 (msm_device_t, which wrote `W_all <= 16 && n < 2^31 / 16`): n within the fused pass's limit
//     on scalars.  B % 256 == 0 holds, W <= 16 meaning c >= 16.  `key_bits <= 17` does not: key_bits
//     is c - 1 there, and c = 19 / 20 (W = 14 / 13) fuse, over 8-bit passes (rs_plan) -- so it is a
//     term of the pairs only.
//   P > 1 (msm_srs_pairs_t, which wrote `W <= 16 && key_bits <= 17`): keys of <= 17 bits, so that the
//     first pass is an 8-bit one, and B a multiple of 256: the fused histogram takes the low byte of
//     |d| - 1 for that of the key p B + |d| - 1 (msm_radix_sort checks it; constant here as well,
//     B >= 2^15).  The limit on the P n scalars stays with msm_radix_sort, which refuses more.
inline bool msm_fuse_first_pass(int P, size_t n, int W, uint32_t B, uint32_t key_bits) {
    if (W > 16) return false;
    if (P == 1) return n < (1ull << 31) / 16;
    return key_bits <= 17 && (B & 255u) == 0;
}

}  // namespace halo
