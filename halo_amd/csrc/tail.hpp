// The multiples-table MSM (tail.hip): sums over a table d 2^(4 w) G0[k] of a few thousand points, as the
// IPA's tail rounds, the small MSMs over the SRS prefix and the tiny MSM use it.  Its constants, the
// kernels' argument structs, the device helpers that other units' kernels call, and the launchers.
// Nothing here knows an IPA session.
#pragma once
#include "curve.hpp"
#include "glv.hpp"
#include "runtime.hpp"

namespace halo {

constexpr int TAIL_DB = 4;                            // digit bits
constexpr int TAIL_TBL = 128 / TAIL_DB;               // table windows per 128-bit GLV half
constexpr int TAIL_MUL = 1 << (TAIL_DB - 1);           // multiples d = 1..8 per window (signed digits)
constexpr int TAIL_WIN = 2 * TAIL_TBL;  // terms per point: 32 windows x (k1, k2)
// threads per tail block: 256, one wave per SIMD (512 measured slower, opening 2^10 1.93 -> 2.13 ms: two
// waves' quad trees then share a SIMD's issue slots)
constexpr int TAIL_THREADS = 256;

// n0 up to this: one launch per round (k_tail_round, scalars formed in the points' waves); above it the
// three-launch round (k_tail_digits, k_tail_msm, k_tail_final) is faster (measured per 2^10 / 2^12 round:
// 0.118 / 0.195 vs 0.125-0.131 / 0.206 ms fused; 2^4 / 2^6 / 2^8: 0.103 / 0.110 / 0.114 vs 0.092-0.094 /
// 0.094-0.097 / 0.097-0.109 ms for the fused one)
constexpr size_t TAIL_FUSE_N = 256;

// Signed windows: a GLV half |k| < 0.47 x 2^128 (the lattice bound, tests/test_field_bounds.py) is kept
// as k + 0x8888...8 (< 2^128), whose nibble e of window w is the digit e - 8 in [-8, 7] of k.
HALO_DEV void tail_bias(uint32_t (&k)[5]) {
    uint64_t c = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        c += (uint64_t)k[q] + 0x88888888u;
        k[q] = (uint32_t)c;
        c >>= 32;
    }
}
// window bw of a biased word: |digit| (0..8) and whether the digit is negative
HALO_DEV uint32_t tail_digit(uint32_t word, uint32_t bw, bool& neg) {
    const uint32_t e = (word >> (TAIL_DB * (bw % (32 / TAIL_DB)))) & 15u;
    neg = e < 8;
    return neg ? 8 - e : e - 8;
}

// the GLV digits of term k's scalar v (internal form) and its side
template <class Cv>
HALO_DEV void tail_scalar_val(const Fe<typename Cv::Scalar>& v, uint8_t sd, size_t k, uint32_t* scal, uint8_t* side) {
    using S = typename Cv::Scalar;
    Fe<S> one_raw = fe_zero<S>();  // internal (x 2^261) -> canonical: Montgomery product with 1
    one_raw.v[0] = 1;
    uint32_t w8[8], k1[5], k2[5];
    bool n1, n2;
    fe_pack(fe_canon(fe_mul(v, one_raw)), w8);
    glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
    tail_bias(k1);
    tail_bias(k2);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        scal[8 * k + q] = k1[q];
        scal[8 * k + 4 + q] = k2[q];
    }
    side[k] = sd | (n1 ? 2 : 0) | (n2 ? 4 : 0);
}

// The previous round's fold (pcdl.rs:430-435, w' = interleave(w, xi w)) deferred into this launch:
// halo_ipa_fold only records xi (passed here by value -- no H2D copy, no k_tail_fold launch); the
// scalar blocks read the unfolded c, w and fold the entries they need on the fly, the dots block
// writes the folded c, z, w to the other buffers of their ping-pong pairs.
struct TailFoldArgs {
    uint4 xi[2], xinv[2];  // ark
    uint4 *cs_out, *zs_out, *w_out;
    size_t wlen_in;  // fold weights before the fold
    int active;
    uint4* w_one;  // the first tail round: w = [1] (not yet in memory): use 1, and store it here
    // non-null: xi | xi^-1 (ark, 64 B) are read from device memory instead of xi / xinv above (an opening whose
    // transcript runs on the device, pcdl_open_fs.hip: the host never sees the challenge).  The launchers then
    // pick the kernels' XI_DEV instantiation, so the by-value kernels carry no test of it.
    const uint4* xi_dev;
};
// The fold's challenge and its inverse: the arguments, or (XI_DEV) device memory
template <class S, bool XI_DEV>
HALO_DEV Fe<S> tail_fold_xi(const TailFoldArgs& f) {
    return XI_DEV ? fe_from_ark<S>(f.xi_dev) : fe_from_ark<S>(f.xi);
}
template <class S, bool XI_DEV>
HALO_DEV Fe<S> tail_fold_xinv(const TailFoldArgs& f) {
    return XI_DEV ? fe_from_ark<S>(f.xi_dev + 2) : fe_from_ark<S>(f.xinv);
}

// One tail round's inputs and outputs (k_tail_round; k_tail_digits reads the scalar vectors)
struct TailRoundArgs {
    const uint4* table;
    size_t ld, n0, m;
    const uint4 *cs, *zs, *w;
    uint32_t nbs;              // point blocks per side
    const uint4* xi0_ark;      // xi mode: dots scaled by xi_0
    const uint4* htab;         // 2^i H' (or 2^i H in xi mode), i < 128
    uint4* dots_ark;           // [2] out
    uint4* part;               // [2][nbs + 1] XYZZ partials
    uint32_t* ctr;             // [2] arrival counters (zero between launches)
    uint4* out_xyzz;           // [2] L, R
    uint32_t* host;            // the session's pinned L | R staging (tail_emit_host) or null
    uint32_t seq;              // this round's flag value
};

template <class F>
HALO_DEV void tail_publish_fe(uint32_t* d, const Fe<F>& v) {
    uint32_t x[8];
    fe_pack(v, x);
#pragma unroll
    for (int i = 0; i < 8; i++) __hip_atomic_store(d + i, x[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class F>
HALO_DEV void tail_publish(uint4* dst, const XYZZ<F>& v) {  // relaxed agent-scope stores (sc1), one lane
    uint32_t* d = (uint32_t*)dst;
    tail_publish_fe(d, v.X);
    tail_publish_fe(d + 8, v.Y);
    tail_publish_fe(d + 16, v.ZZ);
    tail_publish_fe(d + 24, v.ZZZ);
}

// true in the block whose release add on *c returned total - 1 (then acquired); block-uniform
HALO_DEV bool tail_arrive(uint32_t* c, uint32_t total, uint32_t* flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t got = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        *flag = got == total - 1;
        if (*flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    return *flag != 0;
}

// ---- launchers (tail.hip): every tail kernel is instantiated there -------------------------------
// Blocks of TAIL_THREADS lanes over `terms` table terms at tpl terms per lane
inline size_t tail_blocks_at(size_t terms, uint32_t tpl) {
    return (terms + TAIL_THREADS * tpl - 1) / ((size_t)TAIL_THREADS * tpl);
}
// k_tail_msm's terms per lane and its blocks for one side of `terms` table terms (TAIL_WIN per point),
// `sides` such sides in the launch.  A scratch reservation and the launch that fills it both take
// their counts from here.
struct TailBlocks {
    uint32_t tpl;
    size_t nblk;
};
TailBlocks tail_blocks(const DeviceState* st, size_t terms, size_t sides = 1);

// The multiples table of n0 points gs (internal affine, or packed XYZZ with gs_xyzz): k_tail_table's
// doubling chains, then k_tail_mults.  table: TAIL_TBL * TAIL_MUL * n0 XYZZ entries.
int tail_table_build(int curve, const void* gs, bool gs_xyzz, size_t n0, void* table, hipStream_t s);

// The sums over a multiples table: k_tail_msm's block trees and, where the caller asks for it,
// k_tail_final over their partials.  Fields left unset are null / zero.
struct TailSums {
    const uint4* table = nullptr;  // multiples table and the number of points it was built for
    size_t ld = 0;
    const uint32_t* scal = nullptr;  // the n0 scalars' biased GLV words and sides (tail_scalar_val)
    const uint8_t* side = nullptr;
    size_t n0 = 0, m = 0;
    int mode = 1;       // 0: L | R of a round over len = 2m (two sides of blk.nblk blocks); 1: one sum
    TailBlocks blk{};   // terms per lane, blocks per side (tail_blocks)
    uint4* part = nullptr;  // 2 XYZZ partials per block
    // hiding term of each side, added in the side's first block: hide_scalar[sd] * P from the GLV table
    // htab = {2^i P : i < 128}; hkw: the scalars' GLV splits (10 words each) when already formed
    const uint4* htab = nullptr;
    const uint4* hide_scalar = nullptr;
    const uint32_t* hkw = nullptr;
    uint4* out = nullptr;         // the result(s) of k_tail_final: packed XYZZ (out_xyzz) or a WrappedPoint
    bool out_xyzz = true;
    uint4* out_direct = nullptr;  // where k_tail_msm itself writes a side that is one block (XYZZ)
    uint32_t* host = nullptr;     // pinned L | R staging with flags = seq (tail_emit_host), or null
    uint32_t seq = 0;
    const uint4* plus = nullptr;      // WrappedPoint added to the result
    const uint4* copy_src = nullptr;  // 32 B copied beside the result by its last block
    uint4* copy_dst = nullptr;
};
int tail_sums(int curve, const TailSums& a, bool with_final, hipStream_t s);

// One tail round in one launch (k_tail_round, n0 <= TAIL_FUSE_N)
int tail_round_launch(int curve, const TailRoundArgs& a, const TailFoldArgs& f, hipStream_t s);
// The first launch of a three-launch round (k_tail_digits): the round's scalars to scal / side, the
// dots to a.dots_ark and their GLV splits to hkw
int tail_digits_launch(int curve, const TailRoundArgs& a, const TailFoldArgs& f, uint32_t* scal, uint8_t* side,
                       uint32_t* hkw, hipStream_t s);
// k_tail_scalars (mode 1: s[k] = w[k])
int tail_scalars_launch(int curve, const void* cs, const void* w, size_t n0, size_t len, size_t m, int mode,
                        uint32_t* scal, uint8_t* side, hipStream_t s);

// Scratch of a small SRS MSM over n points (SrsState::small_scr): the scalars' GLV words, their sides,
// the block partials, and the launch's block counts.
struct SmallMsmScratch {
    uint32_t* scal;
    uint8_t* side;
    uint4* part;
    TailBlocks blk;
};
int small_msm_scratch(DeviceState* st, int curve, size_t n, hipStream_t s, SmallMsmScratch* scr);
int small_msm_sums(DeviceState* st, int curve, const SmallMsmScratch& scr, size_t n, const void* hide_scalar, void* d_out,
                   hipStream_t s, bool out_xyzz, const void* plus_wrapped, const void* copy_src, void* copy_dst);

}  // namespace halo
