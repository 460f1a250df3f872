// PlonkProof::verify_succinct (crates/plonk/src/plonk/protocol.rs:357-491) for k raw proofs of one circuit:
// the PLONK transcript, the gate identity at xi, the two evaluation instances and acc::verifier
// (crates/accumulation/src/acc.rs:128-213) as one chain of launches on one stream.
//
//   k_plonk_points      one lane per point of the batch: a point that is neither (0, 0) nor on the curve marks
//                       its proof malformed
//   k_plonk_challenges  one PLONK sponge per proof: label, absorb_g(C_ws), beta, gamma, absorb_g(C_z), alpha,
//                       absorb_g(C_ts), zeta, xi (protocol.rs:366-395)
//   k_plonk_identity    one lane per proof, in the scalar field: f', g', the five custom gates, the public
//                       input and l1 terms over one shared inversion, f, t z_H and the bit f == t z_H
//                       (protocol.rs:401-444); v_r, v_r_omega and the term rows of C_r (43 powers of zeta) and
//                       C_r_omega (4) (protocol.rs:453-475)
//   (lincomb_device)    C_r and C_r_omega as packed XYZZ
//   k_plonk_instances   the 3 k instance commitments: acc_prev.C, C_r and C_r_omega made affine (the PCDL
//                       transcript absorbs affine coordinates)
//   (fs_device)         pcdl::succinct_check of the 3 k instances, their challenges kept (pcdl_fs.hip)
//   (acc_challenges_launch)  one ASDL sponge per proof, m = 3: label, absorb_fr of the 3 (lg n + 1) xis,
//                       absorb_g(U_0, U_1, U_2), alpha, z' (acc.rs:157-169; k_acc_challenges, acc_fs.hip)
//   (acc_terms_launch)  the rows of sum alpha^i U_i - acc_next.C, z' == acc_next.z and
//                       sum alpha^i h_i(z') == acc_next.v (acc.rs:207-210; k_acc_terms, k_acc_finish)
//   (lincomb_device)    C_bar' - C_bar is the identity
//   k_plonk_verdict     the stage bits folded into one byte per proof, in the reference's order
//
// PlonkProof::verify (protocol.rs:493-502, halo_plonk_verify_batch) is the same chain with four PCDL instances
// per proof, the fourth acc_next itself, and acc::decider after it (decider.hip):
//   k_plonk_next        before fs_device: the instance 4 i + 3 and the evaluation proofs of all 4 k instances in
//                       fs_device's layout
//   k_plonk_split_xis   after it: the challenges of the first three instances three per proof (what the ASDL
//                       kernels read, unchanged) and those of acc_next as decide_device's rows
//   (decide_device)     the deciders of the proofs whose verdict is still ACCEPT; k_plonk_decided folds them in
//
// As in pcdl_fs.hip no sponge state passes between kernels, and lanes past the batch repeat its last
// proof because they take part in the shuffles.  Host side: one ScratchLayout, one HostParts table
// (scratch_layout.hpp), scalar_below / check_rho (host_scalar.hpp), DISPATCH_LANES (sponge_launch.hpp).
#include "acc_fs.hpp"
#include "curve.hpp"
#include "decider.hpp"
#include "dispatch.hpp"
#include "host_scalar.hpp"
#include "lincomb.hpp"
#include "outer_sponge.hpp"
#include "pcdl_fs.hpp"
#include "quad_ladder.hpp"
#include "runtime.hpp"
#include "sponge_launch.hpp"

namespace halo {

constexpr int PLONK_LABEL = 2;  // Protocols::PLONK (outer_sponge.rs:17-22)
constexpr int PV_THREADS = 64;                  // the kernels with one lane per proof or per point
constexpr int N_W = 16, N_R = 15, N_Q = 10, N_T = 16, N_S = 8;  // crates/plonk/src/utils.rs:16-24
// PlonkProofEvals in struct order (protocol.rs:36-46)
constexpr int V_WS = 0, V_RS = V_WS + N_W, V_QS = V_RS + N_R, V_TS = V_QS + N_Q, V_IDS = V_TS + N_T, V_SIGMAS = V_IDS + N_S,
              V_Z = V_SIGMAS + N_S, V_Z_OMEGA = V_Z + 1, V_W_OMEGAS = V_Z_OMEGA + 1, N_VS = V_W_OMEGAS + 3;
static_assert(N_VS == HALO_PLONK_EVALS, "halo_gpu.h");
constexpr int R_TERMS = N_Q + N_W + N_T + 1, RO_TERMS = 4;  // C_r, C_r_omega (protocol.rs:465-475)
enum { BIT_IDENTITY = 1, BIT_Z = ACC_BIT_Z, BIT_V = ACC_BIT_V };  // stage bits of a proof: set = the check failed

// ---------------------------------------------------------------------------------------------
// points
// ---------------------------------------------------------------------------------------------
// Point p of proof i, p < 38 + 6 lg + N_Q: C_ws, C_z, C_ts, acc_prev.C, acc_next.C, U, Ls, Rs, the shared C_qs.
template <class Cv>
__global__ __launch_bounds__(PV_THREADS) void k_plonk_points(const uint4* __restrict__ C_qs, const uint4* __restrict__ C_ws,
                                                             const uint4* __restrict__ C_z, const uint4* __restrict__ C_ts,
                                                             const uint4* __restrict__ prev_C,
                                                             const uint4* __restrict__ next_C, const uint4* __restrict__ U,
                                                             const uint4* __restrict__ Ls, const uint4* __restrict__ Rs,
                                                             size_t lg, size_t k, uint8_t* __restrict__ mal) {
    using F = typename Cv::Base;
    const size_t per = N_W + 1 + N_T + 2 + 3 + 6 * lg + N_Q;
    const size_t g = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (g >= k * per) return;
    const size_t i = g / per;
    size_t p = g % per;
    const uint4* src;
    if (p < N_W)
        src = C_ws + 4 * (N_W * i + p);
    else if ((p -= N_W) < 1)
        src = C_z + 4 * i;
    else if ((p -= 1) < N_T)
        src = C_ts + 4 * (N_T * i + p);
    else if ((p -= N_T) < 1)
        src = prev_C + 4 * i;
    else if ((p -= 1) < 1)
        src = next_C + 4 * i;
    else if ((p -= 1) < 3)
        src = U + 4 * (3 * i + p);
    else if ((p -= 3) < 3 * lg)
        src = Ls + 4 * (3 * lg * i + p);
    else if ((p -= 3 * lg) < 3 * lg)
        src = Rs + 4 * (3 * lg * i + p);
    else
        src = C_qs + 4 * (p - 3 * lg);
    if (!aff_on_curve_or_id(aff_from_wrapped<F>(src), fe_from_const<F>(Cv::K::B))) mal[i] = 1;  // every writer stores 1
}

// ---------------------------------------------------------------------------------------------
// the PLONK transcript
// ---------------------------------------------------------------------------------------------
// chal[5 i ..] = beta, gamma, alpha, zeta, xi (ark).  Three stretches, each the coordinates of its points
// through the one absorb call and then its challenges through the one challenge call.
template <class Cv, int LANES>
__global__ __launch_bounds__(256) void k_plonk_challenges(const uint32_t* __restrict__ params, const uint4* __restrict__ C_ws,
                                                          const uint4* __restrict__ C_z, const uint4* __restrict__ C_ts,
                                                          size_t k, uint4* __restrict__ chal) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using S = typename Cv::Scalar;
    __shared__ uint32_t tab[poseidon::TABLE_WORDS];
    SPONGE_PROLOGUE(LANES, params, tab, k, i, ic, writer);
    Sp sp;
    sp.init(tab);
    int out = 0;
#pragma unroll 1
    for (int st = 0; st < 3; st++) {
        const uint4* pts = st == 0 ? C_ws + 4 * N_W * ic : st == 1 ? C_z + 4 * ic : C_ts + 4 * N_T * ic;
        const int n_label = st == 0 ? 1 : 0, total = n_label + 2 * (st == 0 ? N_W : st == 1 ? 1 : N_T);
#pragma unroll 1
        for (int e = 0; e < total; e++) {
            const int q = e - n_label;
            sp.absorb(q < 0 ? Sp::label_element(PLONK_LABEL) : Sp::g_element(pts + 4 * (q >> 1), q & 1));
        }
#pragma unroll 1
        for (int c = 0; c < (st == 1 ? 1 : 2); c++, out++) {
            uint32_t w[8];
            sp.challenge(w);
            if (writer && i < k) poseidon::scalar_words_to_ark<S>(chal + 2 * (5 * i + out), w);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the identity at xi
// ---------------------------------------------------------------------------------------------
// The terms that affine_add_constraints_generic and the R = Q + G half of affine_mul_constraints_generic
// share (protocol.rs:712-760, 873-921): P + Q = R with the witnesses al, ga, de, lam; l_be is the factor
// 1 - x beta, whose x the two gates take from different columns.
template <class S>
HALO_DEV Fe<S> gate_add_core(const Fe<S>& xp, const Fe<S>& yp, const Fe<S>& xq, const Fe<S>& yq, const Fe<S>& xr,
                             const Fe<S>& yr, const Fe<S>& al, const Fe<S>& ga, const Fe<S>& de, const Fe<S>& lam,
                             const Fe<S>& l_be) {
    const Fe<S> one = fe_one<S>();
    const Fe<S> dx = fe_sub(xq, xp), sy = fe_add(yq, yp);
    Fe<S> r = fe_mul(dx, fe_sub(fe_mul(dx, lam), fe_sub(yq, yp)));
    const Fe<S> xx = fe_sqr(xp);
    r = fe_add(r, fe_mul(fe_sub(one, fe_mul(dx, al)),
                         fe_sub(fe_mul(fe_add(yp, yp), lam), fe_add(fe_add(xx, xx), xx))));
    const Fe<S> xpxq = fe_mul(xp, xq);
    const Fe<S> ll_x = fe_sub(fe_sub(fe_sub(fe_sqr(lam), xp), xq), xr);
    const Fe<S> l_y = fe_sub(fe_sub(fe_mul(lam, fe_sub(xp, xr)), yp), yr);
    const Fe<S> both = fe_add(ll_x, l_y);
    r = fe_add(r, fe_mul(fe_mul(xpxq, fe_add(dx, sy)), both));  // xp xq ((xq - xp) + (yq + yp)) (ll_x + l_y)
    r = fe_add(r, fe_mul(l_be, fe_add(fe_sub(xr, xq), fe_sub(yr, yq))));
    r = fe_add(r, fe_mul(fe_sub(one, fe_mul(xq, ga)), fe_add(fe_sub(xr, xp), fe_sub(yr, yp))));
    const Fe<S> l_ad = fe_sub(fe_sub(one, fe_mul(dx, al)), fe_mul(sy, de));
    return fe_add(r, fe_mul(l_ad, fe_add(xr, yr)));
}

// One lane per proof.  den: m = max(npi, 1) elements per proof for the prefix products of the shared
// inversion.  Writes sides[2 i ..] = f, t z_H; bits[i] = BIT_IDENTITY when they differ; the scalars z, v of the
// instances ipp i + 0 .. 2 (ipp instances per proof); the term rows of C_r and C_r_omega.  mal[i] = 1 for a scalar that is not below the
// modulus or a zero denominator n (xi - omega^j), 1 <= j <= m.
template <class Cv>
__global__ __launch_bounds__(PV_THREADS) void k_plonk_identity(
    const uint4* __restrict__ vs, const uint4* __restrict__ pub, size_t npi, const uint4* __restrict__ chal,
    const uint4* __restrict__ mds, const uint4* __restrict__ C_qs, const uint4* __restrict__ C_ws,
    const uint4* __restrict__ C_z, const uint4* __restrict__ C_ts, const uint4* __restrict__ prev_z,
    const uint4* __restrict__ prev_v, const uint4* __restrict__ next_z, const uint4* __restrict__ next_v,
    const uint4* __restrict__ c, unsigned lg, size_t k, size_t ipp, uint4* __restrict__ den, uint4* __restrict__ r_pts,
    uint4* __restrict__ r_sc, uint4* __restrict__ ro_pts, uint4* __restrict__ ro_sc, uint4* __restrict__ inst_z,
    uint4* __restrict__ inst_v, uint4* __restrict__ sides, uint8_t* __restrict__ bits, uint8_t* __restrict__ mal) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (i >= k) return;
    vs += 2 * N_VS * i;
    pub += 2 * npi * i;
    chal += 2 * 5 * i;
    auto V = [&](int j) { return fe_from_ark<S>(vs + 2 * j); };
    const Fe<S> one = fe_one<S>();

    bool bad = !ark_is_canonical<S>(prev_z + 2 * i) || !ark_is_canonical<S>(prev_v + 2 * i) ||
               !ark_is_canonical<S>(next_z + 2 * i) || !ark_is_canonical<S>(next_v + 2 * i);
#pragma unroll 1
    for (int j = 0; j < N_VS; j++) bad = bad || !ark_is_canonical<S>(vs + 2 * j);
#pragma unroll 1
    for (size_t j = 0; j < npi; j++) bad = bad || !ark_is_canonical<S>(pub + 2 * j);
#pragma unroll 1
    for (int j = 0; j < 3; j++) bad = bad || !ark_is_canonical<S>(c + 2 * (3 * i + j));
#pragma unroll 1
    for (int j = 0; j < 9; j++) bad = bad || !ark_is_canonical<S>(mds + 2 * j);

    // Every value is loaded where it is used and the sum f grows gate by gate: what stays live across the
    // gates is f, t z_H and the gates' own columns.
    const Fe<S> xi = fe_from_ark<S>(chal + 8);
    const Fe<S> omega = fe_from_const<S>(S::OMEGA[lg]);
    Fe<S> xi_n = xi, n_fe = one;
#pragma unroll 1
    for (unsigned j = 0; j < lg; j++) {  // pow_n (protocol.rs:532-540)
        xi_n = fe_sqr(xi_n);
        n_fe = fe_add(n_fe, n_fe);
    }
    const Fe<S> z_h = fe_sub(xi_n, one);

    // 1 / (n (xi - omega^j)), 1 <= j <= m: prefix products, one inversion, then backwards.  l1 reads j = 1;
    // public_input_eval_generic (protocol.rs:564-589) reads j = 1 .. npi.
    const size_t m = npi ? npi : 1;
    den += 2 * m * i;
    Fe<S> run = one, w_j = omega;
#pragma unroll 1
    for (size_t j = 0; j < m; j++) {
        Fe<S> d = fe_mul(n_fe, fe_sub(xi, w_j));
        if (fe_is_zero(d)) {
            bad = true;
            d = one;
        }
        fe_store(den + 2 * j, run);
        run = fe_mul(run, d);
        w_j = fe_mul(w_j, omega);
    }
    Fe<S> inv = fe_inv(run);
    const Fe<S> omega_inv = fe_from_const<S>(S::OMEGA_INV[lg]);
    Fe<S> pi_xi = fe_zero<S>(), l1 = fe_zero<S>();
#pragma unroll 1
    for (size_t j = m; j-- > 0;) {
        w_j = fe_mul(w_j, omega_inv);  // omega^(j + 1)
        const Fe<S> d_inv = fe_mul(inv, fe_load<S>(den + 2 * j));
        Fe<S> d = fe_mul(n_fe, fe_sub(xi, w_j));
        if (fe_is_zero(d)) d = one;
        inv = fe_mul(inv, d);
        const Fe<S> l_j = fe_mul(fe_mul(z_h, w_j), d_inv);
        if (j < npi) pi_xi = fe_sub(pi_xi, fe_mul(l_j, fe_from_ark<S>(pub + 2 * j)));
        if (j == 0) l1 = l_j;
    }

    // t_reconstruct_generic (protocol.rs:519-530), Horner from the top
    Fe<S> rhs = V(V_TS + N_T - 1);
#pragma unroll 1
    for (int j = N_T - 2; j >= 0; j--) rhs = fe_add(fe_mul(rhs, xi_n), V(V_TS + j));
    rhs = fe_mul(rhs, z_h);

    // f', g' (protocol.rs:403-408), then PI + alpha F_CC1 + alpha^2 F_CC2 (protocol.rs:430-438)
    Fe<S> f;
    {
        const Fe<S> beta = fe_from_ark<S>(chal), gamma = fe_from_ark<S>(chal + 2), alpha = fe_from_ark<S>(chal + 4);
        Fe<S> f_prime = one, g_prime = one;
#pragma unroll 1
        for (int j = 0; j < N_S; j++) {
            const Fe<S> wg = fe_add(V(V_WS + j), gamma);
            f_prime = fe_mul(f_prime, fe_add(wg, fe_mul(beta, V(V_IDS + j))));
            g_prime = fe_mul(g_prime, fe_add(wg, fe_mul(beta, V(V_SIGMAS + j))));
        }
        const Fe<S> z_xi = V(V_Z);
        const Fe<S> f_cc1 = fe_mul(l1, fe_sub(z_xi, one));
        const Fe<S> f_cc2 = fe_sub(fe_mul(z_xi, f_prime), fe_mul(V(V_Z_OMEGA), g_prime));
        f = fe_add(pi_xi, fe_mul(alpha, fe_add(f_cc1, fe_mul(alpha, f_cc2))));
    }

    // poseidon_constraints_generic (protocol.rs:623-648): a round sums its three rows, so the S-boxes meet
    // the column sums of the MDS matrix
    {
        Fe<S> pos = fe_zero<S>();
        Fe<S> col[3];
        for (int j = 0; j < 3; j++)
            col[j] = fe_add(fe_add(fe_from_ark<S>(mds + 2 * j), fe_from_ark<S>(mds + 2 * (3 + j))), fe_from_ark<S>(mds + 2 * (6 + j)));
#pragma unroll 1
        for (int rd = 0; rd < 5; rd++) {
#pragma unroll
            for (int j = 0; j < 3; j++) {  // unrolled: col[] stays in registers
                const Fe<S> x = fe_from_ark<S>(vs + 2 * (V_WS + 3 * rd + j));
                const Fe<S> x2 = fe_sqr(x), x4 = fe_sqr(x2);
                const Fe<S> nxt = rd < 4 ? fe_from_ark<S>(vs + 2 * (V_WS + 3 * rd + 3 + j)) : V(V_W_OMEGAS + j);
                pos = fe_add(pos, fe_sub(fe_sub(nxt, V(V_RS + 3 * rd + j)), fe_mul(fe_mul(fe_mul(x4, x2), x), col[j])));
            }
        }
        f = fe_add(f, fe_mul(V(V_QS + 5), pos));
    }

    // range_check_generic (protocol.rs:966-990)
    {
        Fe<S> g_rc = fe_sub(V(V_W_OMEGAS), V(V_WS));
#pragma unroll 1
        for (int j = 0; j < N_R; j++) g_rc = fe_sub(g_rc, fe_mul(V(V_WS + 1 + j), V(V_RS + j)));
        f = fe_add(f, fe_mul(V(V_QS + 9), g_rc));
    }

    Fe<S> w[N_W];
#pragma unroll
    for (int j = 0; j < N_W; j++) w[j] = V(V_WS + j);

    // A(x) Q_l + B(x) Q_r + C(x) Q_o + A(x) B(x) Q_m + Q_c (protocol.rs:420-424)
    f = fe_add(f, fe_add(fe_add(fe_mul(w[0], V(V_QS)), fe_mul(w[1], V(V_QS + 1))), fe_mul(w[2], V(V_QS + 2))));
    f = fe_add(f, fe_add(fe_mul(fe_mul(w[0], w[1]), V(V_QS + 3)), V(V_QS + 4)));

    // eq_generic (protocol.rs:1001-1011): a b one eq inv
    {
        const Fe<S> ab = fe_sub(w[0], w[1]);
        const Fe<S> g_eq = fe_add(fe_mul(ab, w[3]), fe_sub(fe_add(fe_mul(ab, w[4]), w[3]), w[2]));
        f = fe_add(f, fe_mul(V(V_QS + 8), g_eq));
    }

    // affine_add_constraints_generic (protocol.rs:705-761): xp yp xq yq xr yr alpha beta gamma delta lambda
    f = fe_add(f, fe_mul(V(V_QS + 6), gate_add_core<S>(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[8], w[9], w[10],
                                                      fe_sub(one, fe_mul(w[0], w[7])))));

    // affine_mul_constraints_generic (protocol.rs:851-937): xp yp a xg yg b xq yq xr yr beta_q lambda_q
    // alpha_r gamma_r delta_r lambda_r; two_pow_i = rs[0]
    {
        const Fe<S>&xp = w[0], &yp = w[1], &a = w[2], &xg = w[3], &yg = w[4], &b = w[5], &xq = w[6], &yq = w[7], &xr = w[8],
              &yr = w[9], &bq = w[10], &lq = w[11];
        const Fe<S> l_be = fe_sub(one, fe_mul(xp, bq));
        const Fe<S> xx = fe_sqr(xp);
        Fe<S> r = fe_mul(l_be, fe_add(xq, yq));
        r = fe_add(r, fe_sub(fe_mul(fe_add(yp, yp), lq), fe_add(fe_add(xx, xx), xx)));
        r = fe_add(r, fe_sub(fe_sub(fe_sqr(lq), fe_add(xp, xp)), xq));
        r = fe_add(r, fe_sub(fe_sub(fe_mul(lq, fe_sub(xp, xq)), yp), yq));
        r = fe_add(r, gate_add_core<S>(xq, yq, xg, yg, xr, yr, w[12], w[13], w[14], w[15], l_be));
        r = fe_add(r, fe_mul(b, fe_sub(b, one)));
        const Fe<S> nb = fe_sub(one, b);
        r = fe_add(r, fe_sub(V(V_W_OMEGAS), fe_add(fe_mul(b, xr), fe_mul(nb, xq))));
        r = fe_add(r, fe_sub(V(V_W_OMEGAS + 1), fe_add(fe_mul(b, yr), fe_mul(nb, yq))));
        r = fe_sub(fe_add(r, V(V_W_OMEGAS + 2)), fe_add(a, fe_mul(b, V(V_RS))));
        f = fe_add(f, fe_mul(V(V_QS + 7), r));
    }
    fe_to_ark(sides + 4 * i, f);
    fe_to_ark(sides + 4 * i + 2, rhs);
    bits[i] = fe_eq(f, rhs) ? 0 : BIT_IDENTITY;
    if (bad) mal[i] = 1;

    // the rows of C_r and C_r_omega, and v_r, v_r_omega (geometric_generic, protocol.rs:453-475)
    r_pts += 4 * R_TERMS * i;
    r_sc += 2 * R_TERMS * i;
    ro_pts += 4 * RO_TERMS * i;
    ro_sc += 2 * RO_TERMS * i;
    const Fe<S> zeta = fe_from_ark<S>(chal + 6);
    Fe<S> zp = one, v_r = fe_zero<S>(), v_ro = fe_zero<S>();
#pragma unroll 1
    for (int j = 0; j < R_TERMS; j++) {
        const uint4* src;
        int ev;
        if (j < N_Q)
            src = C_qs + 4 * j, ev = V_QS + j;
        else if (j < N_Q + N_W)
            src = C_ws + 4 * (N_W * i + j - N_Q), ev = V_WS + j - N_Q;
        else if (j < N_Q + N_W + N_T)
            src = C_ts + 4 * (N_T * i + j - N_Q - N_W), ev = V_TS + j - N_Q - N_W;
        else
            src = C_z + 4 * i, ev = V_Z;
        for (int q = 0; q < 4; q++) r_pts[4 * j + q] = src[q];
        fe_to_ark(r_sc + 2 * j, zp);
        v_r = fe_add(v_r, fe_mul(V(ev), zp));
        if (j < RO_TERMS) {
            const uint4* so = j < 3 ? C_ws + 4 * (N_W * i + j) : C_z + 4 * i;
            for (int q = 0; q < 4; q++) ro_pts[4 * j + q] = so[q];
            fe_to_ark(ro_sc + 2 * j, zp);
            v_ro = fe_add(v_ro, fe_mul(V(j < 3 ? V_W_OMEGAS + j : V_Z_OMEGA), zp));
        }
        zp = fe_mul(zp, zeta);
    }
    inst_z += 2 * ipp * i;  // the proof's instances 0 .. 2 of ipp
    inst_v += 2 * ipp * i;
    for (int q = 0; q < 2; q++) {
        inst_z[q] = prev_z[2 * i + q];
        inst_v[q] = prev_v[2 * i + q];
        inst_z[2 + q] = chal[8 + q];
    }
    fe_to_ark(inst_z + 4, fe_mul(fe_from_ark<S>(chal + 8), fe_from_const<S>(S::OMEGA[lg])));
    fe_to_ark(inst_v + 2, v_r);
    fe_to_ark(inst_v + 4, v_ro);
}

// C of the instances ipp i + 0 .. 2: acc_prev.C, C_r, C_r_omega (the sums made affine; the identity becomes (0, 0)).
template <class Cv>
__global__ __launch_bounds__(PV_THREADS) void k_plonk_instances(const uint4* __restrict__ prev_C,
                                                                const uint4* __restrict__ sum_r,
                                                                const uint4* __restrict__ sum_ro, size_t k, size_t ipp,
                                                                uint4* __restrict__ inst_C) {
    using F = typename Cv::Base;
    const size_t g = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (g >= 3 * k) return;
    const size_t i = g / 3, j = g % 3, o = ipp * i + j;
    if (j == 0)
        for (int q = 0; q < 4; q++) inst_C[4 * o + q] = prev_C[4 * i + q];
    else
        aff_to_wrapped(inst_C + 4 * o, xyzz_to_aff(xyzz_load<F>((j == 1 ? sum_r : sum_ro) + 8 * i)));
}

// verdict[i]: HALO_PLONK_MALFORMED first (the reference has no value for such a proof), then the reference's
// checks in its order.
__global__ __launch_bounds__(PV_THREADS) void k_plonk_verdict(const uint8_t* __restrict__ mal, const uint8_t* __restrict__ bits,
                                                              const uint8_t* __restrict__ ok3,
                                                              const uint8_t* __restrict__ c_is_id, size_t k, size_t ipp,
                                                              uint8_t* __restrict__ verdict, uint8_t* __restrict__ live) {
    const size_t i = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (i >= k) return;
    uint8_t v = HALO_PLONK_ACCEPT;
    if (mal[i])
        v = HALO_PLONK_MALFORMED;
    else if (bits[i] & BIT_IDENTITY)
        v = HALO_PLONK_IDENTITY;
    else if (!ok3[ipp * i])
        v = HALO_PLONK_INSTANCE_0;
    else if (!ok3[ipp * i + 1])
        v = HALO_PLONK_INSTANCE_1;
    else if (!ok3[ipp * i + 2])
        v = HALO_PLONK_INSTANCE_2;
    else if (!c_is_id[i])
        v = HALO_PLONK_C_BAR;
    else if (bits[i] & BIT_Z)
        v = HALO_PLONK_Z;
    else if (bits[i] & BIT_V)
        v = HALO_PLONK_V;
    else if (ipp > 3 && !ok3[ipp * i + 3])
        v = HALO_PLONK_DECIDER_SUCCINCT;
    verdict[i] = v;
    if (live) live[i] = v == HALO_PLONK_ACCEPT ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// PlonkProof::verify: acc_next as a fourth instance per proof, then its decider
// ---------------------------------------------------------------------------------------------
// One lane per proof: the instance 4 i + 3 = (acc_next.C, d, acc_next.z, acc_next.v) and the evaluation proofs of
// the proof's four instances as fs_device reads them (row 4 i + q).
__global__ __launch_bounds__(PV_THREADS) void k_plonk_next(
    const uint4* __restrict__ Ls, const uint4* __restrict__ Rs, const uint4* __restrict__ U, const uint4* __restrict__ c,
    const uint4* __restrict__ next_Ls, const uint4* __restrict__ next_Rs, const uint4* __restrict__ next_U,
    const uint4* __restrict__ next_c, const uint4* __restrict__ next_C, const uint4* __restrict__ next_z,
    const uint4* __restrict__ next_v, size_t lg, size_t k, uint4* __restrict__ Ls4, uint4* __restrict__ Rs4,
    uint4* __restrict__ U4, uint4* __restrict__ c4, uint4* __restrict__ inst_C, uint4* __restrict__ inst_z,
    uint4* __restrict__ inst_v) {
    const size_t i = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (i >= k) return;
#pragma unroll 1
    for (size_t q = 0; q < 4; q++) {
        const size_t o = 4 * i + q;
        const uint4 *sl = q < 3 ? Ls + 4 * (3 * i + q) * lg : next_Ls + 4 * i * lg,
                    *sr = q < 3 ? Rs + 4 * (3 * i + q) * lg : next_Rs + 4 * i * lg,
                    *su = q < 3 ? U + 4 * (3 * i + q) : next_U + 4 * i, *sc = q < 3 ? c + 2 * (3 * i + q) : next_c + 2 * i;
#pragma unroll 1
        for (size_t j = 0; j < 4 * lg; j++) {
            Ls4[4 * o * lg + j] = sl[j];
            Rs4[4 * o * lg + j] = sr[j];
        }
        for (int w = 0; w < 4; w++) U4[4 * o + w] = su[w];
        for (int w = 0; w < 2; w++) c4[2 * o + w] = sc[w];
    }
    const size_t o = 4 * i + 3;
    for (int w = 0; w < 4; w++) inst_C[4 * o + w] = next_C[4 * i + w];
    for (int w = 0; w < 2; w++) {
        inst_z[2 * o + w] = next_z[2 * i + w];
        inst_v[2 * o + w] = next_v[2 * i + w];
    }
}

// The xi rows of a full call, four per proof, split for their readers: those of the instances 4 i + 0 .. 2 three
// per proof (the ASDL kernels' layout, which verify_succinct's chain writes directly) and those of the instances
// 4 i + 3 one after the other (decide_device's layout).  One lane per scalar.
__global__ __launch_bounds__(PV_THREADS) void k_plonk_split_xis(const uint4* __restrict__ xis, size_t lg, size_t k,
                                                                uint4* __restrict__ three, uint4* __restrict__ next) {
    const size_t g = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (g >= 4 * k * (lg + 1)) return;
    const size_t inst = g / (lg + 1), j = g % (lg + 1), i = inst / 4, q = inst % 4;
    uint4* dst = q < 3 ? three + 2 * ((3 * i + q) * (lg + 1) + j) : next + 2 * (i * (lg + 1) + j);
    dst[0] = xis[2 * g];
    dst[1] = xis[2 * g + 1];
}

// A proof that was still accepted takes the decider's verdict.
__global__ __launch_bounds__(PV_THREADS) void k_plonk_decided(const uint8_t* __restrict__ live,
                                                              const uint8_t* __restrict__ decided, size_t k,
                                                              uint8_t* __restrict__ verdict) {
    const size_t i = (size_t)blockIdx.x * PV_THREADS + threadIdx.x;
    if (i >= k) return;
    if (live[i]) verdict[i] = decided[i] ? HALO_PLONK_ACCEPT : HALO_PLONK_DECIDER;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
struct PlonkCall {  // the arguments of either entry point
    int curve;
    size_t rows, k, npi;
    const void *C_qs, *pub, *C_ws, *C_z, *C_ts, *vs, *Ls, *Rs, *U, *c, *prev_C, *prev_z, *prev_v, *next_C, *next_z, *next_v, *mds;
    void *verdict, *chal_out, *sides_out, *asdl_out;
    // PlonkProof::verify only (full): acc_next.pi, the decider's weights (or null) and its `combined` byte (or null)
    bool full = false;
    const void *next_Ls = nullptr, *next_Rs = nullptr, *next_U = nullptr, *next_c = nullptr, *rho = nullptr;
    void* combined = nullptr;
    bool derive = false;  // a null rho means derived weights (decider.hpp decide_derives, resolved at the entry point)
};

// What the decider of a full call reads, left in scratch by plonk_device (plonk_decide runs it).
struct PlonkDecide {
    const void *xis, *live;
    void *decided, *combined;
};

// Everything that needs no device; done: an empty batch.
static int check_plonk_args(const char* call, const PlonkCall& a, bool& done) {
    done = false;
    if (!valid_curve(a.curve)) return set_error(HALO_EINVAL, "%s: unknown curve", call);
    if (a.k == 0) {
        done = true;
        return HALO_OK;
    }
    if (!is_pow2(a.rows)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", a.rows);
    if (a.rows < 4 || ilog2(a.rows) > MAX_LOG_DOMAIN) return set_error(HALO_EINVAL, "%s: %zu rows", call, a.rows);
    if (!a.C_qs || !a.C_ws || !a.C_z || !a.C_ts || !a.vs || !a.Ls || !a.Rs || !a.U || !a.c || !a.prev_C || !a.prev_z ||
        !a.prev_v || !a.next_C || !a.next_z || !a.next_v || !a.mds || !a.verdict || (a.npi && !a.pub))
        return set_error(HALO_EINVAL, "%s: null pointer", call);
    if (a.full && (!a.next_Ls || !a.next_Rs || !a.next_U || !a.next_c)) return set_error(HALO_EINVAL, "%s: null pointer", call);
    const size_t lg = ilog2(a.rows), ipp = a.full ? 4 : 3;
    if (a.k > LINCOMB_MAX_ITEMS / (ipp * (2 * lg + 2)) || a.k > LINCOMB_MAX_ITEMS / R_TERMS || a.npi > (SIZE_MAX / 64) / a.k)
        return set_error(HALO_EINVAL, "%s: %zu proofs in one call", call, a.k);
    return require_poseidon_params(call, a.curve);
}

// acc::decider of the proofs that are still accepted (rho null: exact mode), then their verdicts.  resolve: the
// host form, which waits for a rejected combined batch's per-proof verdicts (decide_resolved).
static int plonk_decide(DeviceState* st, const PlonkCall& a, const PlonkDecide& pd, const void* rho, bool resolve,
                        hipStream_t s) {
    const DecideCall dc{a.curve, a.rows - 1, a.k, pd.xis, a.next_U, pd.live, rho, pd.decided, pd.combined, a.derive};
    HALO_CHECK(resolve ? decide_resolved(st, dc, s) : decide_device(st, dc, s));
    hipLaunchKernelGGL(k_plonk_decided, dim3(grid_for(a.k, PV_THREADS)), dim3(PV_THREADS), 0, s, (const uint8_t*)pd.live,
                       (const uint8_t*)pd.decided, a.k, (uint8_t*)a.verdict);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The launches of one call over device pointers, all on `s`.  st->mu and a ScratchUse of `s` held; a.k >= 1,
// check_verifier_srs passed.  ipp = 3 instances per proof (verify_succinct), or 4 with acc_next (a.full), whose PCDL
// transcript then runs inside the same fs_device chain and whose decider follows (resolve: see plonk_decide).
static int plonk_device(const char* call, DeviceState* st, const PlonkCall& a, hipStream_t s, bool resolve = false) {
    const size_t k = a.k, lg = ilog2(a.rows), d = a.rows - 1, m = a.npi ? a.npi : 1, ipp = a.full ? 4 : 3;
    const size_t nx = a.full ? k : 0;  // proofs with a fourth instance
    const uint32_t* params;
    HALO_CHECK(poseidon_device_params(st, base_field(a.curve), &params));
    // one scratch buffer; the succinct checks work in scratch[7]
    ScratchLayout sl;
    const size_t o_rp = sl.take(k * R_TERMS * 64), o_rs = sl.take(k * R_TERMS * 32), o_op = sl.take(k * RO_TERMS * 64),
                 o_os = sl.take(k * RO_TERMS * 32), o_sr = sl.take(k * 128), o_so = sl.take(k * 128),
                 o_ic = sl.take(ipp * k * 64), o_iz = sl.take(ipp * k * 32), o_iv = sl.take(ipp * k * 32),
                 o_xis = sl.take(ipp * k * (lg + 1) * 32), o_den = sl.take(k * m * 32), o_ap = sl.take(3 * k * 64),
                 o_as = sl.take(3 * k * 32), o_sh = sl.take(3 * k * 32), o_neg = sl.take(k * 64), o_sum = sl.take(k * 128),
                 o_chal = sl.take(a.chal_out ? 0 : k * 5 * 32), o_sides = sl.take(a.sides_out ? 0 : k * 2 * 32),
                 o_asdl = sl.take(a.asdl_out ? 0 : k * 2 * 32), o_mal = sl.take(k), o_bits = sl.take(k),
                 o_ok3 = sl.take(ipp * k), o_cid = sl.take(k), o_l4 = sl.take(4 * nx * lg * 64),
                 o_r4 = sl.take(4 * nx * lg * 64), o_u4 = sl.take(4 * nx * 64), o_c4 = sl.take(4 * nx * 32),
                 o_nxis = sl.take(nx * (lg + 1) * 32), o_xis3 = sl.take(3 * nx * (lg + 1) * 32), o_live = sl.take(nx),
                 o_dec = sl.take(nx), o_comb = sl.take(a.full ? 1 : 0);
    HALO_CHECK(st->scratch[6].reserve(sl.total()));
    // every linear combination of the chain, before anything is in flight
    HALO_CHECK(st->lincomb_terms.reserve(k * std::max<size_t>(R_TERMS, ipp * (2 * lg + 2)) * 129));
    uint8_t* base = st->scratch[6].as<uint8_t>();
    auto u4 = [&](size_t o) { return (uint4*)(base + o); };
    uint4* chal = a.chal_out ? (uint4*)a.chal_out : u4(o_chal);
    uint4* sides = a.sides_out ? (uint4*)a.sides_out : u4(o_sides);
    uint4* asdl = a.asdl_out ? (uint4*)a.asdl_out : u4(o_asdl);
    uint8_t *mal = base + o_mal, *bits = base + o_bits, *ok3 = base + o_ok3, *cid = base + o_cid;
    const dim3 per_proof(grid_for(k, PV_THREADS)), blk(PV_THREADS);
    auto cp = [](const void* p) { return (const uint4*)p; };

    HALO_HIP(hipMemsetAsync(mal, 0, k, s));
    {
        ProfScope prof("plonk_points", s);
        const size_t per = N_W + 1 + N_T + 2 + 3 + 6 * lg + N_Q;
        DISPATCH_CURVE(a.curve, Cv, {
            HALO_LAUNCH(prof, k_plonk_points<Cv>, dim3(grid_for(k * per, PV_THREADS)), blk, 0, s, cp(a.C_qs), cp(a.C_ws),
                        cp(a.C_z), cp(a.C_ts), cp(a.prev_C), cp(a.next_C), cp(a.U), cp(a.Ls), cp(a.Rs), lg, k, mal);
        });
        HALO_HIP(hipGetLastError());
    }
    HALO_CHECK(SPONGE_LAUNCH(st, a.curve, Cv, L, k, "plonk_challenges", s, (k_plonk_challenges<Cv, L>), params, cp(a.C_ws),
                             cp(a.C_z), cp(a.C_ts), k, chal));
    {
        ProfScope prof("plonk_identity", s);
        DISPATCH_CURVE(a.curve, Cv, {
            HALO_LAUNCH(prof, k_plonk_identity<Cv>, per_proof, blk, 0, s, cp(a.vs), cp(a.pub), a.npi, (const uint4*)chal,
                        cp(a.mds), cp(a.C_qs), cp(a.C_ws), cp(a.C_z), cp(a.C_ts), cp(a.prev_z), cp(a.prev_v), cp(a.next_z),
                        cp(a.next_v), cp(a.c), (unsigned)lg, k, ipp, u4(o_den), u4(o_rp), u4(o_rs), u4(o_op), u4(o_os),
                        u4(o_iz), u4(o_iv), sides, bits, mal);
        });
        HALO_HIP(hipGetLastError());
    }
    HALO_CHECK(lincomb_device(st, a.curve, nullptr, u4(o_rp), u4(o_rs), k, R_TERMS, u4(o_sr), nullptr, s));
    HALO_CHECK(lincomb_device(st, a.curve, nullptr, u4(o_op), u4(o_os), k, RO_TERMS, u4(o_so), nullptr, s));
    DISPATCH_CURVE(a.curve, Cv, {
        hipLaunchKernelGGL(k_plonk_instances<Cv>, dim3(grid_for(3 * k, PV_THREADS)), blk, 0, s, cp(a.prev_C),
                           (const uint4*)u4(o_sr), (const uint4*)u4(o_so), k, ipp, u4(o_ic));
    });
    HALO_HIP(hipGetLastError());
    const void *fs_Ls = a.Ls, *fs_Rs = a.Rs, *fs_U = a.U, *fs_c = a.c;
    if (a.full) {
        hipLaunchKernelGGL(k_plonk_next, per_proof, blk, 0, s, cp(a.Ls), cp(a.Rs), cp(a.U), cp(a.c), cp(a.next_Ls),
                           cp(a.next_Rs), cp(a.next_U), cp(a.next_c), cp(a.next_C), cp(a.next_z), cp(a.next_v), lg, k, u4(o_l4),
                           u4(o_r4), u4(o_u4), u4(o_c4), u4(o_ic), u4(o_iz), u4(o_iv));
        HALO_HIP(hipGetLastError());
        fs_Ls = u4(o_l4), fs_Rs = u4(o_r4), fs_U = u4(o_u4), fs_c = u4(o_c4);
    }
    const FsCall fs{a.curve, d, ipp * k, u4(o_ic), u4(o_iz), u4(o_iv), fs_Ls, fs_Rs, fs_U, fs_c, nullptr, nullptr, nullptr,
                    u4(o_xis), nullptr, ok3};
    HALO_CHECK(fs_device(call, st, fs, s));
    const uint4* xis3 = u4(o_xis);  // the challenges of the instances 3 i + 0 .. 2
    if (a.full) {
        hipLaunchKernelGGL(k_plonk_split_xis, dim3(grid_for(4 * k * (lg + 1), PV_THREADS)), blk, 0, s, (const uint4*)u4(o_xis),
                           lg, k, u4(o_xis3), u4(o_nxis));
        HALO_HIP(hipGetLastError());
        xis3 = u4(o_xis3);
    }
    // acc::verifier's transcript and terms: the general-m launches of acc_fs.hip with m = 3
    HALO_CHECK(acc_challenges_launch(st, a.curve, xis3, a.U, lg, k, 3, asdl, s, "asdl_challenges"));
    HALO_CHECK(acc_terms_launch(a.curve, asdl, xis3, a.U, a.next_C, a.next_z, a.next_v, lg, k, 3, u4(o_ap), u4(o_as), u4(o_sh),
                                u4(o_neg), bits, nullptr, s, "asdl_terms"));
    HALO_CHECK(lincomb_device(st, a.curve, u4(o_neg), u4(o_ap), u4(o_as), k, 3, u4(o_sum), cid, s));
    hipLaunchKernelGGL(k_plonk_verdict, per_proof, blk, 0, s, (const uint8_t*)mal, (const uint8_t*)bits, (const uint8_t*)ok3,
                       (const uint8_t*)cid, k, ipp, (uint8_t*)a.verdict, a.full ? base + o_live : (uint8_t*)nullptr);
    HALO_HIP(hipGetLastError());
    if (!a.full) return HALO_OK;
    const PlonkDecide dec{base + o_nxis, base + o_live, base + o_dec, a.combined ? a.combined : (void*)(base + o_comb)};
    return plonk_decide(st, a, dec, a.rho, resolve, s);
}

// Either host entry point: the scalar checks, one buffer of inputs and one of outputs and the chain; in a full
// call a rejected combined batch of deciders is resolved to per-proof verdicts.
static int plonk_host(const char* call, const PlonkCall& host) {
    bool done;
    HALO_CHECK(check_plonk_args(call, host, done));
    if (done) return HALO_OK;
    const size_t k = host.k, npi = host.npi, lg = ilog2(host.rows);
    auto below = [&](const void* p, size_t first, size_t n) { return scalar_below(host.curve, (const halo_fe_t*)p + first, n); };
    if (!below(host.mds, 0, 9)) return set_error(HALO_EINVAL, "%s: an MDS entry is not below the modulus", call);
    for (size_t i = 0; i < k; i++)
        if (!below(host.vs, N_VS * i, N_VS) || !below(host.pub, npi * i, npi) || !below(host.c, 3 * i, 3) ||
            !below(host.prev_z, i, 1) || !below(host.prev_v, i, 1) || !below(host.next_z, i, 1) || !below(host.next_v, i, 1) ||
            (host.full && !below(host.next_c, i, 1)))
            return set_error(HALO_EINVAL, "%s: a scalar of proof %zu is not below the modulus", call, i);
    HALO_CHECK(check_rho(call, host.curve, (const halo_fe_t*)host.rho, k));
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_verifier_srs(call, st, host.curve, host.rows - 1, true));
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t nx = host.full ? k : 0;
    const HostParts in{{host.C_qs, N_Q * 64},        {host.pub, k * npi * 32},   {host.C_ws, k * N_W * 64},
                       {host.C_z, k * 64},           {host.C_ts, k * N_T * 64},  {host.vs, k * N_VS * 32},
                       {host.Ls, k * 3 * lg * 64},   {host.Rs, k * 3 * lg * 64}, {host.U, k * 3 * 64},
                       {host.c, k * 3 * 32},         {host.prev_C, k * 64},      {host.prev_z, k * 32},
                       {host.prev_v, k * 32},        {host.next_C, k * 64},      {host.next_z, k * 32},
                       {host.next_v, k * 32},        {host.mds, 9 * 32},         {host.next_Ls, nx * lg * 64},
                       {host.next_Rs, nx * lg * 64}, {host.next_U, nx * 64},     {host.next_c, nx * 32},
                       {host.rho, host.rho ? nx * 32 : 0}};
    ScratchLayout out;
    const size_t o_chal = out.take(host.chal_out ? k * 5 * 32 : 0), o_sides = out.take(host.sides_out ? k * 2 * 32 : 0),
                 o_asdl = out.take(host.asdl_out ? k * 2 * 32 : 0), o_v = out.total();
    HALO_CHECK(st->scratch[1].reserve(o_v + k));  // the last part is not padded
    std::vector<const void*> dev;
    HALO_CHECK(upload_parts(st, in, s, dev));
    uint8_t* dout = st->scratch[1].as<uint8_t>();
    PlonkCall a{host.curve, host.rows, k,       npi,     dev[0],  dev[1],  dev[2],  dev[3],  dev[4],
                dev[5],     dev[6],    dev[7],  dev[8],  dev[9],  dev[10], dev[11], dev[12], dev[13],
                dev[14],    dev[15],   dev[16], dout + o_v, host.chal_out ? dout + o_chal : nullptr,
                host.sides_out ? dout + o_sides : nullptr, host.asdl_out ? dout + o_asdl : nullptr};
    a.full = host.full;
    a.next_Ls = dev[17], a.next_Rs = dev[18], a.next_U = dev[19], a.next_c = dev[20], a.rho = dev[21];
    a.derive = host.derive;
    HALO_CHECK(plonk_device(call, st, a, s, true));
    if (host.chal_out) HALO_CHECK(copy_d2h(host.chal_out, dout + o_chal, k * 5 * 32, s));
    if (host.sides_out) HALO_CHECK(copy_d2h(host.sides_out, dout + o_sides, k * 2 * 32, s));
    if (host.asdl_out) HALO_CHECK(copy_d2h(host.asdl_out, dout + o_asdl, k * 2 * 32, s));
    return copy_d2h(host.verdict, dout + o_v, k, s);
}

static int plonk_dev(const char* call, const PlonkCall& a, void* stream) {
    bool done;
    HALO_CHECK(check_plonk_args(call, a, done));
    if (done) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    HALO_CHECK(check_verifier_srs(call, st, a.curve, a.rows - 1, true));
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return plonk_device(call, st, a, s);
}

}  // namespace halo

using namespace halo;

extern "C" int halo_plonk_verify_succinct_batch_dev(
    halo_curve_t curve, size_t rows, size_t k, const void* d_C_qs, const void* d_public_inputs, size_t npi, const void* d_C_ws,
    const void* d_C_z, const void* d_C_ts, const void* d_vs, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c,
    const void* d_acc_prev_C, const void* d_acc_prev_z, const void* d_acc_prev_v, const void* d_acc_next_C,
    const void* d_acc_next_z, const void* d_acc_next_v, const void* d_mds, void* d_verdict, void* d_challenges_out,
    void* d_sides_out, void* d_asdl_out, void* stream) {
    clear_error();
    const PlonkCall a{(int)curve, rows, k, npi, d_C_qs, d_public_inputs, d_C_ws, d_C_z, d_C_ts, d_vs, d_Ls, d_Rs, d_U, d_c,
                      d_acc_prev_C, d_acc_prev_z, d_acc_prev_v, d_acc_next_C, d_acc_next_z, d_acc_next_v, d_mds,
                      d_verdict, d_challenges_out, d_sides_out, d_asdl_out};
    return plonk_dev("halo_plonk_verify_succinct_batch_dev", a, stream);
}

extern "C" int halo_plonk_verify_succinct_batch(
    halo_curve_t curve, size_t rows, size_t k, const halo_wrapped_point_t* C_qs, const halo_fe_t* public_inputs, size_t npi,
    const halo_wrapped_point_t* C_ws, const halo_wrapped_point_t* C_z, const halo_wrapped_point_t* C_ts, const halo_fe_t* vs,
    const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs, const halo_wrapped_point_t* U, const halo_fe_t* c,
    const halo_wrapped_point_t* acc_prev_C, const halo_fe_t* acc_prev_z, const halo_fe_t* acc_prev_v,
    const halo_wrapped_point_t* acc_next_C, const halo_fe_t* acc_next_z, const halo_fe_t* acc_next_v, const halo_fe_t* mds,
    uint8_t* verdict, halo_fe_t* challenges_out, halo_fe_t* sides_out, halo_fe_t* asdl_out) {
    clear_error();
    const PlonkCall host{(int)curve, rows, k, npi, C_qs, public_inputs, C_ws, C_z, C_ts, vs, Ls, Rs, U, c, acc_prev_C,
                         acc_prev_z, acc_prev_v, acc_next_C, acc_next_z, acc_next_v, mds, verdict, challenges_out, sides_out,
                         asdl_out};
    return plonk_host("halo_plonk_verify_succinct_batch", host);
}

extern "C" int halo_plonk_verify_batch_dev(
    halo_curve_t curve, size_t rows, size_t k, const void* d_C_qs, const void* d_public_inputs, size_t npi, const void* d_C_ws,
    const void* d_C_z, const void* d_C_ts, const void* d_vs, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c,
    const void* d_acc_prev_C, const void* d_acc_prev_z, const void* d_acc_prev_v, const void* d_acc_next_C,
    const void* d_acc_next_z, const void* d_acc_next_v, const void* d_acc_next_Ls, const void* d_acc_next_Rs,
    const void* d_acc_next_U, const void* d_acc_next_c, const void* d_mds, const void* d_rho, void* d_verdict,
    void* d_combined, void* stream) {
    clear_error();
    PlonkCall a{(int)curve, rows, k, npi, d_C_qs, d_public_inputs, d_C_ws, d_C_z, d_C_ts, d_vs, d_Ls, d_Rs, d_U, d_c,
                d_acc_prev_C, d_acc_prev_z, d_acc_prev_v, d_acc_next_C, d_acc_next_z, d_acc_next_v, d_mds,
                d_verdict, nullptr, nullptr, nullptr};
    a.full = true;
    a.next_Ls = d_acc_next_Ls, a.next_Rs = d_acc_next_Rs, a.next_U = d_acc_next_U, a.next_c = d_acc_next_c;
    a.rho = d_rho, a.combined = d_combined;
    a.derive = decide_derives(d_rho);
    return plonk_dev("halo_plonk_verify_batch_dev", a, stream);
}

extern "C" int halo_plonk_verify_batch(
    halo_curve_t curve, size_t rows, size_t k, const halo_wrapped_point_t* C_qs, const halo_fe_t* public_inputs, size_t npi,
    const halo_wrapped_point_t* C_ws, const halo_wrapped_point_t* C_z, const halo_wrapped_point_t* C_ts, const halo_fe_t* vs,
    const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs, const halo_wrapped_point_t* U, const halo_fe_t* c,
    const halo_wrapped_point_t* acc_prev_C, const halo_fe_t* acc_prev_z, const halo_fe_t* acc_prev_v,
    const halo_wrapped_point_t* acc_next_C, const halo_fe_t* acc_next_z, const halo_fe_t* acc_next_v,
    const halo_wrapped_point_t* acc_next_Ls, const halo_wrapped_point_t* acc_next_Rs, const halo_wrapped_point_t* acc_next_U,
    const halo_fe_t* acc_next_c, const halo_fe_t* mds, const halo_fe_t* rho, uint8_t* verdict) {
    clear_error();
    PlonkCall host{(int)curve, rows, k, npi, C_qs, public_inputs, C_ws, C_z, C_ts, vs, Ls, Rs, U, c, acc_prev_C,
                   acc_prev_z, acc_prev_v, acc_next_C, acc_next_z, acc_next_v, mds, verdict, nullptr, nullptr, nullptr};
    host.full = true;
    host.next_Ls = acc_next_Ls, host.next_Rs = acc_next_Rs, host.next_U = acc_next_U, host.next_c = acc_next_c;
    host.rho = rho;
    host.derive = decide_derives(rho);
    return plonk_host("halo_plonk_verify_batch", host);
}
