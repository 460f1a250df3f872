// The multiples-table MSM: the IPA's tail rounds, the small MSMs over the SRS prefix (msm_srs_small)
// and the tiny MSM of caller points (msm_tiny).  Sessions reach it through the launchers of tail.hpp.
//
// Tail rounds of the opening (length <= IPA_TAIL_N): instead of folding G (one ~128-doubling scalar
// multiplication per element per round, a ~1 ms dependent chain however few elements are left) the
// session keeps G0 = G at the switch round and the fold weights w (G_j[i] = sum_u w[u] G0[i + u len],
// fold: w' = interleave(w, xi w)).  L and R are then direct sums over G0 with expanded scalars
//   k = j + u len:  s[k] = c[m + j] w[u] (j < m, -> L),  c[j - m] w[u] (j >= m, -> R),
// evaluated from a table d 2^(4 win) G0[k] (win < 32, 1 <= d <= 8, built once per session): each
// scalar is split by GLV, s = k1 + lambda k2 with |k1|, |k2| < 0.47 x 2^128, so every (k, win, half)
// term is one table entry (or phi of it, x -> beta x, or its negative) selected by a signed 4-bit
// digit in [-8, 7] -- no per-term double-and-add chain on the rounds' critical path -- and the terms
// go through block trees.  The table's doubling chain is 124 doublings instead of 248; the 8
// multiples of each 2^(4 win) G0[k] cost 7 curve operations per (win, k), once (round 5: signed
// digits, was 15 unsigned multiples -- half the table build and half the table's footprint).
// U = sum_u w[u] G0[u] at the end.  c and z keep their ordinary elementwise folds (pcdl.rs:430-435).
#include <algorithm>

#include "dispatch.hpp"
#include "glv.hpp"
#include "msm.hpp"
#include "runtime.hpp"
#include "tail.hpp"
#include "tree.hpp"

namespace halo {

// the doubling chain by a quad of lanes per point (xyzz_dbl_quad: three product rounds per doubling,
// 4.0 k cycles against 6.3 k for the Jacobian jac_dbl_quad -- fewer products, but a longer tail of
// additions and doublings on every lane; tools/micro/tree_parts.hip; TAIL_TABLE_LANES = 4) -- the
// chain is latency-bound and the grid is small (n0 <= 8192 points)
constexpr int TAIL_TABLE_LANES = 4;
template <class Cv>
__global__ __launch_bounds__(64) void k_tail_table(const uint4* gs, int gs_xyzz, size_t n0, uint4* table) {
    using F = typename Cv::Base;
    const size_t k = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / TAIL_TABLE_LANES;
    if (k >= n0) return;  // (whole quads leave)
    const bool lead = threadIdx.x % TAIL_TABLE_LANES == 0;
    const XYZZ<F> p0 = gs_xyzz ? xyzz_load<F>(gs + 8 * k) : xyzz_from_aff(aff_load<F>(gs + 4 * k));
    if (lead) xyzz_store(table + 8 * k, p0);
    XYZZ<F> q = p0;
    for (int w = 1; w < TAIL_TBL; w++) {
        for (int b = 0; b < TAIL_DB; b++) q = xyzz_dbl_quad(q);
        if (lead) xyzz_store(table + 8 * ((size_t)w * TAIL_MUL * n0 + k), q);
    }
}

// entry (w, d, k) of the tail table: d 2^(4 w) G0[k], 1 <= d <= 8 (XYZZ); ld = the number of
// points the table was built for (a session may use a prefix of the SRS's table)
HALO_DEV size_t tail_entry(size_t w, uint32_t d, size_t ld, size_t k) {
    return 8 * ((w * TAIL_MUL + (d - 1)) * ld + k);
}

// The multiples 2..8 of each window base P = 2^(4 w) G0[k] written by k_tail_table.  Lane
// (j, w, k), j < 4, owns d = 2j + 1, 2j + 2: it forms (2j + 1) P by double-and-add, then adds P --
// at most 5 dependent curve operations per lane.
constexpr int TAIL_MLANES = 4;
template <class Cv>
__global__ __launch_bounds__(64) void k_tail_mults(size_t n0, uint4* table) {
    using F = typename Cv::Base;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)TAIL_MLANES * TAIL_TBL * n0) return;
    const uint32_t j = (uint32_t)(t / ((size_t)TAIL_TBL * n0));
    const size_t r = t % ((size_t)TAIL_TBL * n0), w = r / n0, k = r % n0;
    const XYZZ<F> p = xyzz_load<F>(table + tail_entry(w, 1, n0, k));
    const uint32_t s = 2 * j + 1;
    XYZZ<F> cur = p;
#pragma unroll 1
    for (int b = 31 - __clz(s) - 1; b >= 0; b--) {  // s P, s = 2 j + 1 (bit 0 set: the last step adds)
        cur = xyzz_dbl(cur);
        if ((s >> b) & 1u) cur = xyzz_add(cur, p);
    }
    if (j) xyzz_store(table + tail_entry(w, s, n0, k), cur);
    xyzz_store(table + tail_entry(w, s + 1, n0, k), j ? xyzz_add(cur, p) : xyzz_dbl(p));
}

// mode 0: L/R scalars of the current round (len = 2m); mode 1: U's scalars s[k] = w[k]
template <class Cv>
HALO_DEV void tail_scalar_one(const uint4* cs, const uint4* w, size_t k, size_t len, size_t m, int mode, uint32_t* scal,
                              uint8_t* side) {
    using S = typename Cv::Scalar;
    if (mode == 0) {
        const size_t j = k % len, u = k / len;
        const size_t ci = (j < m) ? m + j : j - m;
        tail_scalar_val<Cv>(fe_mul(fe_from_ark<S>(cs + 2 * ci), fe_from_ark<S>(w + 2 * u)), (j < m) ? 0 : 1, k, scal,
                            side);
    } else {
        tail_scalar_val<Cv>(fe_from_ark<S>(w + 2 * k), 0, k, scal, side);
    }
}

template <class Cv>
__global__ __launch_bounds__(256) void k_tail_scalars(const uint4* cs, const uint4* w, size_t n0, size_t len, size_t m,
                                                      int mode, uint32_t* scal, uint8_t* side) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n0) tail_scalar_one<Cv>(cs, w, k, len, m, mode, scal, side);
}

template <class Cv>
HALO_DEV void glv_split_words(const uint4* x_ark, uint32_t* out10) {
    using S = typename Cv::Scalar;
    uint32_t w8[8], k1[5], k2[5];
    bool n1, n2;
    fe_ark_to_canonical_words<S>(x_ark, w8);
    glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
    for (int q = 0; q < 4; q++) {
        out10[q] = k1[q];
        out10[4 + q] = k2[q];
    }
    out10[8] = n1;
    out10[9] = n2;
}

// The hiding term dot * P' of one side as lane terms: lane t < 256 returns the table entry for bit t
// of the GLV split dot = k1 + lambda k2 (lanes 0-127: k1 with 2^t P', 128-255: k2 with phi(2^(t-128) P'))
// or the identity.  Block-uniform call (it synchronises).
// pre: the split already formed (glv_split_words, 10 words), else lane 0 forms it.
template <class Cv>
HALO_DEV XYZZ<typename Cv::Base> hiding_lane_term(const uint4* htab, const uint4* dot_ark, const uint32_t* pre,
                                                  uint32_t (&kw)[10]) {
    using F = typename Cv::Base;
    const int tid = threadIdx.x;
    if (pre) {
        if (tid < 10) kw[tid] = pre[tid];
    } else if (tid == 0) {
        glv_split_words<Cv>(dot_ark, kw);
    }
    __syncthreads();
    XYZZ<F> acc = xyzz_id<F>();
    if ((kw[tid >> 5] >> (tid & 31)) & 1u) {
        Affine<F> p = aff_load<F>(htab + 4 * (tid & 127));
        if (tid >= 128) p.x = fe_mul(p.x, fe_from_const<F>(Cv::K::BETA));
        if (kw[8 + (tid >> 7)]) p.y = fe_neg(p.y);
        acc = xyzz_from_aff(p);
    }
    return acc;
}

// A tail round's side sum straight into the session's pinned staging (coherent host memory): 32
// words with system-scope stores, then the side's flag = seq with a system-scope release.  The host
// polls the two flags instead of a D2H copy plus a stream synchronisation (round 3 measurement,
// tools/micro/sync_bench.hip: 5.8 vs 11 us per host round trip).  host: L at [0, 32), R at [32, 64)
// words; flags[0..2).
template <class F>
HALO_DEV void tail_emit_host(uint32_t* host, uint32_t* flags, uint32_t sd, const XYZZ<F>& v, uint32_t seq) {
    const Fe<F>* c[4] = {&v.X, &v.Y, &v.ZZ, &v.ZZZ};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t w[8];
        fe_pack(*c[k], w);
#pragma unroll
        for (int i = 0; i < 8; i++)
            __hip_atomic_store(host + 32 * sd + 8 * k + i, w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __hip_atomic_store(flags + sd, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Block partial sums part[block][side].  mode 0 (L and R of a round, 2m = len): the first nbs blocks
// take side 0's terms, the rest side 1's (each block one side: one tree, not two); the term q of a
// side is (win, u, j) = window, fold weight, j < m, at point k = j + u 2m + side m.  mode 1 (U): terms
// t = win n0 + k, all on side 0.
template <class Cv>
// With htab: side sd's first block also adds the hiding term dots[sd] * P (GLV table htab of 2^i P;
// hkw: the dots' GLV splits when already formed) into its tree; with out_xyzz and nbs == 1 (the side
// is one block) it writes the side's sum straight to out_xyzz + 8 sd (no k_tail_final).  Mode 1 is
// one side of nbs blocks.
__global__ __launch_bounds__(TAIL_THREADS) void k_tail_msm(const uint4* table, size_t ld, const uint32_t* scal,
                                                            const uint8_t* side, size_t n0, size_t m, int mode, uint32_t nbs,
                                                            uint4* part, const uint4* htab, const uint4* dots_ark,
                                                            const uint32_t* hkw, uint4* out_xyzz,
                                                            uint32_t* host = nullptr, uint32_t seq = 0,
                                                            const uint4* plus_wrapped = nullptr,
                                                            const uint4* copy_src = nullptr, uint4* copy_dst = nullptr,
                                                            uint32_t tpl = 1) {
    using F = typename Cv::Base;
    __shared__ uint4 red[TAIL_THREADS / 2 * 8];
    __shared__ uint32_t kw[10];
    const int tid = threadIdx.x;
    XYZZ<F> acc = xyzz_id<F>();
    const uint32_t bsd = mode == 0 ? (uint32_t)(blockIdx.x >= nbs) : 0u;
    const bool first = htab && blockIdx.x == bsd * nbs;
    if (first) acc = hiding_lane_term<Cv>(htab, dots_ark + 2 * bsd, hkw ? hkw + 10 * bsd : nullptr, kw);
    const uint32_t sd = bsd;
    const size_t hn = n0 / 2, total = mode == 0 ? (size_t)TAIL_WIN * hn : (size_t)TAIL_WIN * n0;
    const size_t q0 = (size_t)(blockIdx.x - sd * nbs) * TAIL_THREADS + tid, qstride = (size_t)nbs * TAIL_THREADS;
    // term q of the side: mode 0 (win, u, j) at point k = j + u 2m + sd m; mode 1 t = win n0 + k
    auto term = [&](size_t q) {
        XYZZ<F> t = xyzz_id<F>();
        if (q >= total) return t;
        size_t win, k;
        if (mode == 0) {
            win = q / hn;
            const size_t r = q % hn, u = r / m, j = r % m;
            k = j + u * 2 * m + sd * m;
        } else {
            win = q / n0;
            k = q % n0;
        }
        constexpr uint32_t DPW = 32 / TAIL_DB;  // digits per scalar word
        const uint32_t half = (uint32_t)win / TAIL_TBL, bw = (uint32_t)win % TAIL_TBL;
        bool dneg;
        const uint32_t d = tail_digit(scal[8 * k + 4 * half + bw / DPW], bw, dneg);
        const uint32_t sk = side[k];
        if (d) {
            t = xyzz_load<F>(table + tail_entry(bw, d, ld, k));
            if (half) t.X = fe_mul(t.X, fe_from_const<F>(Cv::K::BETA));  // phi
            if ((((sk >> (1 + half)) & 1u) != 0) != dneg) t = xyzz_neg(t);
        }
        return t;
    };
    // tpl = 2 (grids beyond one block per CU): each lane first adds its two terms, so the trees run at
    // one wave per SIMD instead of two sharing a SIMD's issue slots
    XYZZ<F> t = term(q0);
    if (tpl == 2) t = xyzz_add(t, term(q0 + qstride));
    acc = first ? xyzz_add(acc, t) : t;
    acc = block_group_sum<F>(acc, TAIL_THREADS, red);
    if (out_xyzz && nbs == 1) {
        if (tid == 0) {
            if (plus_wrapped) acc = xyzz_madd(acc, aff_from_wrapped<F>(plus_wrapped));
            xyzz_store(out_xyzz + 8 * bsd, acc);
            if (copy_src) {  // 32 B beside the result, so that one D2H copy takes both
                copy_dst[0] = copy_src[0];
                copy_dst[1] = copy_src[1];
            }
            if (host) tail_emit_host(host, host + 64, bsd, acc, seq);
        }
    } else if (tid == 0) {
        xyzz_store(part + 8 * (2 * (size_t)blockIdx.x + sd), acc);
        xyzz_store(part + 8 * (2 * (size_t)blockIdx.x + (sd ^ 1)), xyzz_id<F>());
    }
}

HALO_DEV uint32_t tail_word(const uint32_t (&k)[5], uint32_t i) {  // k[i], i < 4, without dynamic indexing
    uint32_t r = k[0];
    r = i == 1 ? k[1] : r;
    r = i == 2 ? k[2] : r;
    return i == 3 ? k[3] : r;
}

template <class Cv>
HALO_DEV void tail_side_final(const TailRoundArgs& a, uint32_t sd, uint4* red) {
    using F = typename Cv::Base;
    const uint32_t np = a.nbs + 1;
    // partial j to lane j / 4 of wave j % 4: every wave gets a quarter, and its tree skips the identity
    // lanes above them (as k_tail_final deals them)
    const uint32_t tid = threadIdx.x, j0 = (tid & 63) * (TAIL_THREADS / 64) + (tid >> 6);
    XYZZ<F> acc = xyzz_id<F>();
    for (uint32_t j = j0; j < np; j += TAIL_THREADS) acc = xyzz_add(acc, xyzz_load<F>(a.part + 8 * ((size_t)sd * np + j)));
    acc = block_group_sum<F>(acc, TAIL_THREADS, red);
    if (tid == 0) {
        xyzz_store(a.out_xyzz + 8 * sd, acc);
        if (a.host) tail_emit_host(a.host, a.host + 64, sd, acc, a.seq);
        __hip_atomic_store(a.ctr + sd, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Side sd's dot (0: <c_r, z_l>, 1: <c_l, z_r>) by one block, scaled by xi_0 in xi mode, to dots_ark +
// 2 sd and its GLV split to kw (10 words: k1, k2 words, signs; visible to the block on return).  With a
// deferred fold the block folds the halves its dot reads and writes them to the ping-pong buffers (side
// 0: c_r, z_l and the even w'; side 1: c_l, z_r and the odd w').
template <class Cv, bool XI_DEV>
HALO_DEV void tail_side_dot(const uint4* cs, const uint4* zs, const uint4* w, size_t m, uint32_t sd, const TailFoldArgs& f,
                            const uint4* xi0_ark, uint4* dots_ark, uint32_t* kw) {
    using S = typename Cv::Scalar;
    const int tid = threadIdx.x;
    const size_t len = 2 * m;
    const size_t oc = sd ? 0 : m, oz = sd ? m : 0;  // c_r z_l (side 0), c_l z_r (side 1)
    Fe<S> acc_s = fe_zero<S>();
    if (f.active) {
        const Fe<S> xi = tail_fold_xi<S, XI_DEV>(f), xinv = tail_fold_xinv<S, XI_DEV>(f);
        for (size_t i = tid; i < m; i += TAIL_THREADS) {
            const Fe<S> c = fe_add(fe_from_ark<S>(cs + 2 * (oc + i)), fe_mul(fe_from_ark<S>(cs + 2 * (oc + i + len)), xinv));
            const Fe<S> z = fe_add(fe_from_ark<S>(zs + 2 * (oz + i)), fe_mul(fe_from_ark<S>(zs + 2 * (oz + i + len)), xi));
            fe_to_ark(f.cs_out + 2 * (oc + i), c);
            fe_to_ark(f.zs_out + 2 * (oz + i), z);
            acc_s = fe_add(acc_s, fe_mul(c, z));
        }
        for (size_t u = tid; u < f.wlen_in; u += TAIL_THREADS) {
            const Fe<S> wv = fe_from_ark<S>(w + 2 * u);
            fe_to_ark(f.w_out + 2 * (2 * u + sd), sd ? fe_mul(wv, xi) : wv);
        }
    } else {
        for (size_t i = tid; i < m; i += TAIL_THREADS)
            acc_s = fe_add(acc_s, fe_mul(fe_from_ark<S>(cs + 2 * (oc + i)), fe_from_ark<S>(zs + 2 * (oz + i))));
    }
    // block sum: lane shuffles inside each wave, then the four wave sums through LDS
    for (int off = 32; off > 0; off >>= 1) {
        Fe<S> o;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) o.v[l] = __shfl_xor(acc_s.v[l], off);
        acc_s = fe_add(acc_s, o);
    }
    __shared__ uint4 wsum[TAIL_THREADS / 64][2];
    if ((tid & 63) == 0) fe_store(wsum[tid >> 6], acc_s);
    __syncthreads();
    if (tid == 0) {
        Fe<S> d = fe_load<S>(wsum[0]);
        for (int q = 1; q < TAIL_THREADS / 64; q++) d = fe_add(d, fe_load<S>(wsum[q]));
        if (xi0_ark) d = fe_mul(d, fe_from_ark<S>(xi0_ark));
        fe_to_ark(dots_ark + 2 * sd, d);
        Fe<S> one_raw = fe_zero<S>();
        one_raw.v[0] = 1;
        uint32_t w8[8], k1[5], k2[5];
        bool n1, n2;
        fe_pack(fe_canon(fe_mul(d, one_raw)), w8);
        glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
        for (int i = 0; i < 4; i++) {
            kw[i] = k1[i];
            kw[4 + i] = k2[i];
        }
        kw[8] = n1;
        kw[9] = n2;
    }
    __syncthreads();
}

// The round's n0 point scalars c[ci] w[u] (with a deferred fold applied on the fly) as GLV words, one
// lane per point, and (the last two blocks) the two sides' dots with their GLV splits (hkw, for
// k_tail_msm's hiding terms) and the folded c, z, w: the first launch of a tail round over more than
// TAIL_FUSE_N points, where forming the scalars once per point beats forming them in each point's
// wave of k_tail_round (64 times the instructions).
template <class Cv, bool XI_DEV>
__global__ __launch_bounds__(256) void k_tail_digits(const uint4* cs, const uint4* zs, const uint4* w, size_t n0, size_t m,
                                                     const TailFoldArgs f, uint32_t* scal, uint8_t* side,
                                                     const uint4* xi0_ark, uint4* dots_ark, uint32_t* hkw) {
    using S = typename Cv::Scalar;
    const uint32_t nsb = (uint32_t)((n0 + 255) / 256);
    if (blockIdx.x >= nsb) {
        __shared__ uint32_t kw[10];
        const uint32_t sd = blockIdx.x - nsb;
        tail_side_dot<Cv, XI_DEV>(cs, zs, w, m, sd, f, xi0_ark, dots_ark, kw);
        if (threadIdx.x < 10) hkw[10 * sd + threadIdx.x] = kw[threadIdx.x];
        return;
    }
    const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n0) return;
    const size_t len = 2 * m, j = k % len, u = k / len;
    const size_t ci = (j < m) ? m + j : j - m;
    Fe<S> c, wu;
    if (f.active) {
        c = fe_add(fe_from_ark<S>(cs + 2 * ci), fe_mul(fe_from_ark<S>(cs + 2 * (ci + len)), tail_fold_xinv<S, XI_DEV>(f)));
        wu = fe_from_ark<S>(w + 2 * (u >> 1));
        if (u & 1) wu = fe_mul(wu, tail_fold_xi<S, XI_DEV>(f));
    } else {
        c = fe_from_ark<S>(cs + 2 * ci);
        wu = f.w_one ? fe_one<S>() : fe_from_ark<S>(w + 2 * u);
        if (f.w_one && k == 0) fe_to_ark(f.w_one, wu);
    }
    tail_scalar_val<Cv>(fe_mul(c, wu), (j < m) ? 0 : 1, k, scal, side);
}


// One tail round (L and R with their hiding terms) in ONE launch (round 4; was k_tail_prep + k_tail_msm +
// k_tail_final).  Blocks [0, 2 nbs) own 4 points each (one per wave), all on one side: side sd's point
// q = (block - sd nbs) 4 + wave (q < n0 / 2) is k = j + u 2m + sd m with u = q / m, j = q % m, and its
// 64 lanes are its 64 window terms (32 4-bit GLV windows x (k1, k2)).  Every lane of the wave forms the
// point's scalar c[ci] w[u] and its GLV split itself (wave-uniform work: the SIMD issues it once), so
// no preparation launch is needed; with a deferred fold the unfolded c / w are folded on the fly as
// k_tail_prep did.  Blocks 2 nbs + sd form side sd's dot product (with a deferred fold they also write
// their halves of the folded c, z, w), scale it by xi_0 in xi mode, and add the side's hiding term
// dot_sd * H' as one more partial -- one block per side, in parallel with the point blocks.  Each block
// publishes its partial (relaxed agent-scope stores drained, then an agent-scope release add on its
// side's counter); the last block to arrive on a side takes an agent acquire, sums the side's nbs + 1
// partials and writes the side's XYZZ sum to out_xyzz + 8 sd, then resets the counter.  No block waits
// for another.
template <class Cv, bool XI_DEV>
__global__ __launch_bounds__(TAIL_THREADS, 1) void k_tail_round(const TailRoundArgs a, const TailFoldArgs f) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint4 red[TAIL_THREADS / 2 * 8];
    __shared__ uint32_t flag;
    const int tid = threadIdx.x;
    const size_t m = a.m, len = 2 * m, hn = a.n0 / 2;
    if (blockIdx.x < 2 * a.nbs) {
        const uint32_t sd = blockIdx.x >= a.nbs;
        const size_t q = (size_t)(blockIdx.x - sd * a.nbs) * (TAIL_THREADS / 64) + (tid >> 6);
        XYZZ<F> acc = xyzz_id<F>();
        if (q < hn) {  // (wave-uniform)
            const size_t u = q / m, j = q % m, k = j + u * len + sd * m;
            const size_t ci = sd ? j : m + j;
            Fe<S> c, wu;
            if (f.active) {  // c' = c_l + xi^-1 c_r over the unfolded c; w'[u] = w[u / 2] (xi w[u / 2] for odd u)
                c = fe_add(fe_from_ark<S>(a.cs + 2 * ci), fe_mul(fe_from_ark<S>(a.cs + 2 * (ci + len)), tail_fold_xinv<S, XI_DEV>(f)));
                wu = fe_from_ark<S>(a.w + 2 * (u >> 1));
                if (u & 1) wu = fe_mul(wu, tail_fold_xi<S, XI_DEV>(f));
            } else {
                c = fe_from_ark<S>(a.cs + 2 * ci);
                wu = f.w_one ? fe_one<S>() : fe_from_ark<S>(a.w + 2 * u);
                if (f.w_one && k == 0 && (tid & 63) == 0) fe_to_ark(f.w_one, wu);
            }
            Fe<S> one_raw = fe_zero<S>();  // internal (x 2^261) -> canonical: Montgomery product with 1
            one_raw.v[0] = 1;
            uint32_t w8[8], k1[5], k2[5];
            bool n1, n2;
            fe_pack(fe_canon(fe_mul(fe_mul(c, wu), one_raw)), w8);
            glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
            tail_bias(k1);
            tail_bias(k2);
            constexpr uint32_t DPW = 32 / TAIL_DB;  // digits per scalar word
            const uint32_t win = tid & 63, half = win / TAIL_TBL, bw = win % TAIL_TBL;
            const uint32_t word = half ? tail_word(k2, bw / DPW) : tail_word(k1, bw / DPW);
            bool dneg;
            const uint32_t d = tail_digit(word, bw, dneg);
            if (d) {
                XYZZ<F> t = xyzz_load<F>(a.table + tail_entry(bw, d, a.ld, k));
                if (half) t.X = fe_mul(t.X, fe_from_const<F>(Cv::K::BETA));  // phi
                if ((half ? n2 : n1) != dneg) t = xyzz_neg(t);
                acc = t;
            }
        }
        acc = block_group_sum<F>(acc, TAIL_THREADS, red);
        if (tid == 0) tail_publish(a.part + 8 * ((size_t)sd * (a.nbs + 1) + (blockIdx.x - sd * a.nbs)), acc);
        if (tail_arrive(a.ctr + sd, a.nbs + 1, &flag)) tail_side_final<Cv>(a, sd, red);
        return;
    }
    // ---- hiding blocks 2 nbs + sd: side sd's dot, its GLV split and the term dot_sd H'
    const uint32_t sd = blockIdx.x - 2 * a.nbs;
    __shared__ uint32_t kw[10];
    tail_side_dot<Cv, XI_DEV>(a.cs, a.zs, a.w, m, sd, f, a.xi0_ark, a.dots_ark, kw);
    // dot H': lane t < 128 bit t of k1 with 2^t H', t >= 128 bit t - 128 of k2 with phi(2^(t-128) H')
    XYZZ<F> acc = xyzz_id<F>();
    if ((kw[tid >> 5] >> (tid & 31)) & 1u) {
        Affine<F> p = aff_load<F>(a.htab + 4 * (tid & 127));
        if (tid >= 128) p.x = fe_mul(p.x, fe_from_const<F>(Cv::K::BETA));
        if (kw[8 + (tid >> 7)]) p.y = fe_neg(p.y);
        acc = xyzz_from_aff(p);
    }
    acc = block_group_sum<F>(acc, TAIL_THREADS, red);
    if (tid == 0) tail_publish(a.part + 8 * ((size_t)sd * (a.nbs + 1) + a.nbs), acc);
    if (tail_arrive(a.ctr + sd, a.nbs + 1, &flag)) tail_side_final<Cv>(a, sd, red);
}

// block b (0: L, 1: R): sum of the partials + dot_b * H' (from the 2^i H' table), -> WrappedPoint
template <class Cv>
__global__ __launch_bounds__(TAIL_THREADS) void k_tail_final(const uint4* part, int nblk, const uint4* htab,
                                                              const uint4* dots_ark, uint4* out_wrapped,
                                                              int xyzz_out, uint32_t* host = nullptr,
                                                              uint32_t seq = 0, const uint4* plus_wrapped = nullptr,
                                                              const uint4* copy_src = nullptr, uint4* copy_dst = nullptr) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    __shared__ uint4 red[TAIL_THREADS / 2 * 8];
    __shared__ uint32_t kw[8];
    __shared__ uint32_t neg[2];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (htab && tid == 0) {  // dot_b = k1 + lambda k2: lanes 0-127 k1 with 2^i H', 128-255 k2 with phi(2^i H')
        uint32_t w8[8], k1[5], k2[5];
        bool n1, n2;
        fe_ark_to_canonical_words<S>(dots_ark + 2 * b, w8);
        glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
        for (int q = 0; q < 4; q++) {
            kw[q] = k1[q];
            kw[4 + q] = k2[q];
        }
        neg[0] = n1;
        neg[1] = n2;
    }
    __syncthreads();
    // lane tid: its partials plus, for bit tid of (k1 | k2), the table entry -- one tree
    XYZZ<F> acc = xyzz_id<F>();
    if (htab && ((kw[tid >> 5] >> (tid & 31)) & 1u)) {
        Affine<F> p = aff_load<F>(htab + 4 * (tid & 127));
        if (tid >= 128) p.x = fe_mul(p.x, fe_from_const<F>(Cv::K::BETA));
        if (neg[tid >> 7]) p.y = fe_neg(p.y);
        acc = xyzz_from_aff(p);
    }
    // this side's partials (blocks [b per_side, (b + 1) per_side)), dealt round-robin over the waves so
    // that every SIMD's wave sums a quarter of them
    const int per_side = nblk / (int)gridDim.x, j0 = (tid & 63) * (TAIL_THREADS / 64) + (tid >> 6);
    for (int j = j0; j < per_side; j += TAIL_THREADS)
        acc = xyzz_add(acc, xyzz_load<F>(part + 8 * (2 * (size_t)(b * per_side + j) + b)));
    acc = block_group_sum<F>(acc, TAIL_THREADS, red);
    if (tid == 0) {
        if (plus_wrapped) acc = xyzz_madd(acc, aff_from_wrapped<F>(plus_wrapped));  // (the combine's + C)
        if (copy_src) {  // 32 B beside the result, so that one D2H copy takes both
            copy_dst[0] = copy_src[0];
            copy_dst[1] = copy_src[1];
        }
        if (xyzz_out) {  // 128 B per side, converted on the host (host_xyzz_to_wrapped)
            xyzz_store(out_wrapped + 8 * b, acc);
            if (host) tail_emit_host(host, host + 64, b, acc, seq);
        } else {
            aff_to_wrapped(out_wrapped + 4 * b, xyzz_to_aff(acc));
        }
    }
}

}  // namespace halo

using namespace halo;

// k_tail_msm's terms per lane: 2 once a one-term grid would put more than one block on a CU (two waves
// sharing a SIMD's issue slots through the whole tree): a lane's own addition of its two terms costs
// less than the slower tree (opening 2^16, n0 = 2048: 512 blocks of one term or 256 of two)
TailBlocks halo::tail_blocks(const DeviceState* st, size_t terms, size_t sides) {
    const uint32_t tpl = sides * tail_blocks_at(terms, 1) > (size_t)st->num_cu ? 2u : 1u;
    return {tpl, tail_blocks_at(terms, tpl)};
}

int halo::tail_table_build(int curve, const void* gs, bool gs_xyzz, size_t n0, void* table, hipStream_t s) {
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_tail_table<Cv>, dim3(grid_for((size_t)TAIL_TABLE_LANES * n0, 64)), dim3(64), 0, s, (const uint4*)gs,
                           (int)gs_xyzz, n0, (uint4*)table);
        hipLaunchKernelGGL(k_tail_mults<Cv>, dim3(grid_for((size_t)TAIL_MLANES * TAIL_TBL * n0, 64)), dim3(64), 0, s, n0,
                           (uint4*)table);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int halo::tail_sums(int curve, const TailSums& a, bool with_final, hipStream_t s) {
    const unsigned sides = a.mode == 0 ? 2 : 1, nblk = (unsigned)(sides * a.blk.nblk);
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_tail_msm<Cv>, dim3(nblk), dim3(TAIL_THREADS), 0, s, a.table, a.ld, a.scal, a.side, a.n0, a.m,
                           a.mode, (uint32_t)a.blk.nblk, a.part, a.htab, a.hide_scalar, a.hkw, a.out_direct, a.host, a.seq,
                           a.plus, a.copy_src, a.copy_dst, a.blk.tpl);
        if (with_final)  // (the hiding terms rode in k_tail_msm's first blocks: none here)
            hipLaunchKernelGGL(k_tail_final<Cv>, dim3(sides), dim3(TAIL_THREADS), 0, s, (const uint4*)a.part, (int)nblk,
                               (const uint4*)nullptr, (const uint4*)nullptr, a.out, (int)a.out_xyzz, a.host, a.seq, a.plus,
                               a.copy_src, a.copy_dst);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int halo::tail_round_launch(int curve, const TailRoundArgs& a, const TailFoldArgs& f, hipStream_t s) {
    DISPATCH_CURVE(curve, Cv, {
        if (f.xi_dev)
            hipLaunchKernelGGL((k_tail_round<Cv, true>), dim3(2 * a.nbs + 2), dim3(TAIL_THREADS), 0, s, a, f);
        else
            hipLaunchKernelGGL((k_tail_round<Cv, false>), dim3(2 * a.nbs + 2), dim3(TAIL_THREADS), 0, s, a, f);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int halo::tail_digits_launch(int curve, const TailRoundArgs& a, const TailFoldArgs& f, uint32_t* scal, uint8_t* side,
                             uint32_t* hkw, hipStream_t s) {
    DISPATCH_CURVE(curve, Cv, {
        if (f.xi_dev)
            hipLaunchKernelGGL((k_tail_digits<Cv, true>), dim3(grid_for(a.n0, 256) + 2), dim3(256), 0, s, a.cs, a.zs, a.w, a.n0,
                               a.m, f, scal, side, a.xi0_ark, a.dots_ark, hkw);
        else
            hipLaunchKernelGGL((k_tail_digits<Cv, false>), dim3(grid_for(a.n0, 256) + 2), dim3(256), 0, s, a.cs, a.zs, a.w, a.n0,
                               a.m, f, scal, side, a.xi0_ark, a.dots_ark, hkw);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int halo::tail_scalars_launch(int curve, const void* cs, const void* w, size_t n0, size_t len, size_t m, int mode,
                              uint32_t* scal, uint8_t* side, hipStream_t s) {
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_tail_scalars<Cv>, dim3(grid_for(n0, 256)), dim3(256), 0, s, (const uint4*)cs, (const uint4*)w, n0,
                           len, m, mode, scal, side);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// 8192 points (0.5 GB of XYZZ multiples per curve): the small MSMs up to 2^13 and the openings up to
// 2^13 run entirely on the table (tail rounds from round 1, no weighted rounds, no materialisation)
size_t halo::srs_tab_n() { return 8192; }
size_t halo::srs_small_max() { return srs_tab_n(); }

// scratch of a small SRS MSM over n points: GLV words (n x 32 B) | sides (n B, 256-B aligned) | partials;
// stream s waits for the previous small MSM (done with the scratch) and for the SRS multiples table
int halo::small_msm_scratch(DeviceState* st, int curve, size_t n, hipStream_t s, SmallMsmScratch* scr) {
    SrsState& srs = st->srs[curve];
    const size_t nmax = std::min(srs_small_max(), srs.n);
    if (n < 1 || n > nmax) return set_error(HALO_EINVAL, "small SRS MSM: n (%zu) outside [1, %zu]", n, nmax);
    scr->blk = tail_blocks(st, TAIL_WIN * n);
    const size_t o_side = n * 32, o_part = o_side + ((n + 255) & ~(size_t)255);
    if (srs.small_ev) HALO_HIP(hipStreamWaitEvent(s, srs.small_ev, 0));  // the previous small MSM is done with small_scr
    else HALO_HIP(hipEventCreateWithFlags(&srs.small_ev, hipEventDisableTiming));
    HALO_CHECK(srs.small_scr.reserve(o_part + scr->blk.nblk * 256));
    HALO_CHECK(srs_small_table(st, curve, s));
    char* base = (char*)srs.small_scr.ptr;
    scr->scal = (uint32_t*)base;
    scr->side = (uint8_t*)(base + o_side);
    scr->part = (uint4*)(base + o_part);
    return HALO_OK;
}

// The small MSM after its scalars' GLV words are in the scratch (small_msm_scratch): the table sums with
// the hiding term w S in block 0 (2^i S table), an XYZZ result from the one block or k_tail_final, plus an
// optional point added at the end and a 32-B side copy (copy_src -> copy_dst) beside it.
int halo::small_msm_sums(DeviceState* st, int curve, const SmallMsmScratch& scr, size_t n, const void* hide_scalar,
                         void* d_out, hipStream_t s, bool out_xyzz, const void* plus_wrapped, const void* copy_src,
                         void* copy_dst) {
    SrsState& srs = st->srs[curve];
    const bool direct = out_xyzz && scr.blk.nblk == 1;  // the one block writes the XYZZ sum itself
    TailSums a;
    a.table = srs.small_tab->as<const uint4>();
    a.ld = srs.small_n0;
    a.scal = scr.scal;
    a.side = scr.side;
    a.n0 = n;
    a.blk = scr.blk;
    a.part = scr.part;
    if (hide_scalar) a.htab = srs.s_table.as<const uint4>();
    a.hide_scalar = (const uint4*)hide_scalar;
    a.out = (uint4*)d_out;
    a.out_xyzz = out_xyzz;
    if (direct) a.out_direct = (uint4*)d_out;
    a.plus = (const uint4*)plus_wrapped;
    a.copy_src = (const uint4*)copy_src;
    a.copy_dst = (uint4*)copy_dst;
    HALO_CHECK(tail_sums(curve, a, !direct, s));
    HALO_HIP(hipEventRecord(srs.small_ev, s));
    return HALO_OK;
}

// MSM of at most TINY_MSM_MAX caller points (acc::prover's C = sum alpha^i U_i, acc.rs:166): the bucket
// pipeline's latency there is its Horner over 43 windows of 6 bits (~250 quad doublings in k_final).
// Here every scalar is split by GLV into two 128-bit halves with signed 4-bit windows (tail_bias), so
// 32 windows suffice: wave w forms window w's term d P_i (or phi(d P_i)) for its 2n (point, half) lanes
// by double-and-add (|d| <= 8: at most four curve operations), sums them with the wave's quad tree, and
// k_final's Horner over the 32 window sums (4 quad doublings each) finishes: ~124 doublings in all.
constexpr size_t TINY_MSM_MAX = 32;
template <class Cv>
__global__ __launch_bounds__(256) void k_tiny_window_sums(const uint4* bases, const uint4* scalars_ark, uint32_t n,
                                                          uint4* window_sums) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    XYZZ<F> acc = xyzz_id<F>();
    if (lane < 2 * n && w < (uint32_t)TAIL_TBL) {
        const uint32_t i = lane >> 1, half = lane & 1u;
        uint32_t w8[8], k1[5], k2[5];
        bool n1, n2;
        fe_ark_to_canonical_words<S>(scalars_ark + 2 * i, w8);
        glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
        tail_bias(k1);
        tail_bias(k2);
        bool dneg;
        const uint32_t bw = w, word = half ? tail_word(k2, bw / 8) : tail_word(k1, bw / 8);
        const uint32_t d = tail_digit(word, bw, dneg);
        Affine<F> a = aff_load<F>(bases + 4 * i);
        if (d && !aff_is_id(a)) {
            if (half) a.x = fe_mul(a.x, fe_from_const<F>(Cv::K::BETA));  // phi
            if ((half ? n2 : n1) != dneg) a.y = fe_neg(a.y);
            const XYZZ<F> P = xyzz_from_aff(a);
            XYZZ<F> t = P;
#pragma unroll 1
            for (int b = 31 - __clz(d) - 1; b >= 0; b--) {
                t = xyzz_dbl(t);
                if ((d >> b) & 1u) t = xyzz_add(t, P);
            }
            acc = t;
        }
    }
    acc = wave_group_sum<F>(acc, 64u);
    if (lane == 0 && w < (uint32_t)TAIL_TBL) xyzz_store(window_sums + 8 * w, acc);
}

// sum_i scalars[i] bases[i] (internal affine bases, ark scalars, n <= TINY_MSM_MAX) -> packed XYZZ at
// out_xyzz (device), stream-ordered on s; scratch: 32 XYZZ window sums (4 KiB).
int halo::msm_tiny(int curve, const void* bases_int, const void* scalars_ark, size_t n, void* scratch, void* out_xyzz,
                   hipStream_t s) {
    if (n < 1 || n > TINY_MSM_MAX) return set_error(HALO_EINVAL, "tiny MSM: n (%zu) outside [1, %zu]", n, TINY_MSM_MAX);
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_tiny_window_sums<Cv>, dim3(TAIL_TBL / 4), dim3(256), 0, s, (const uint4*)bases_int,
                           (const uint4*)scalars_ark, (uint32_t)n, (uint4*)scratch);
    });
    HALO_HIP(hipGetLastError());
    return msm_final_launch(curve, (const uint4*)scratch, TAIL_TBL, TAIL_DB, nullptr, (uint4*)out_xyzz, 1, s);
}
size_t halo::msm_tiny_max() { return TINY_MSM_MAX; }

// The SRS prefix's multiples table d 2^(4 w) G_k (k < n0 = min(srs_tab_n(), srs.n)), built on first
// use per SRS (k_tail_table + k_tail_mults on stream s; small_tab_ev marks its completion for other
// streams).  SrsState::invalidate_derived() (every writer of the SRS points) forces a rebuild.  The
// table is versioned: while an open IPA session holds the current buffer (table_ref),
// the rebuild goes into a fresh one and the old buffer lives until its last session is released;
// otherwise it is rebuilt in place after the last small MSM that read it (small_ev).
int halo::srs_small_table(DeviceState* st, int curve, hipStream_t s) {
    SrsState& srs = st->srs[curve];
    const size_t n0 = std::min(srs_tab_n(), srs.n);
    if (!n0) return set_error(HALO_ESRSRANGE, "no resident SRS: call halo_srs_upload first");
    if (!srs.small_tab_ev) HALO_HIP(hipEventCreateWithFlags(&srs.small_tab_ev, hipEventDisableTiming));
    if (srs.small_n0 == n0 && srs.small_tab) {
        HALO_HIP(hipStreamWaitEvent(s, srs.small_tab_ev, 0));
        return HALO_OK;
    }
    if (!srs.small_tab || srs.small_tab.use_count() > 1) srs.small_tab = std::make_shared<DevBuf>();
    if (srs.small_ev) HALO_HIP(hipStreamWaitEvent(s, srs.small_ev, 0));  // the old table's last small MSM
    HALO_CHECK(srs.small_tab->reserve((size_t)TAIL_TBL * TAIL_MUL * n0 * 128));
    HALO_CHECK(tail_table_build(curve, srs.gs.ptr, false, n0, srs.small_tab->ptr, s));
    HALO_HIP(hipEventRecord(srs.small_tab_ev, s));
    srs.small_n0 = n0;
    return HALO_OK;
}

// Small MSM over the resident SRS prefix (msm.hpp): the tail rounds' machinery over G0 = Gs[0..n)
// with the SRS's multiples table (leading dimension small_n0 >= n); mode 1 of k_tail_scalars /
// k_tail_msm gives sum_k s[k] G0[k] (64 n table terms), k_tail_final adds w S from the 2^i S table.
int halo::msm_srs_small(DeviceState* st, int curve, const void* scalars_ark, size_t n, const void* hide_scalar,
                  void* d_out_wrapped, hipStream_t s, bool out_xyzz, const void* plus_wrapped) {
    if (plus_wrapped && !out_xyzz) return set_error(HALO_EINVAL, "small SRS MSM: + point needs the XYZZ output");
    SmallMsmScratch scr;
    HALO_CHECK(small_msm_scratch(st, curve, n, s, &scr));
    HALO_CHECK(tail_scalars_launch(curve, nullptr, scalars_ark, n, 1, 0, 1, scr.scal, scr.side, s));
    return small_msm_sums(st, curve, scr, n, hide_scalar, d_out_wrapped, s, out_xyzz, plus_wrapped, nullptr, nullptr);
}
