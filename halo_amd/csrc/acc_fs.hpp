// The accumulation scheme of acc_fs.hip (acc.rs:128-213) for the units that build on it: the device-level
// common_subroutine, and the two general-m ASDL launches on their own (plonk_verify.hip runs them with m = 3).
#pragma once
#include "runtime.hpp"

namespace halo {

// The stage bits the terms launch ORs into bits[i]; set = the check failed.  plonk_verify.hip keeps its
// BIT_IDENTITY = 1 beside them in the same byte.
enum { ACC_BIT_Z = 2, ACC_BIT_V = 4 };

// The ASDL transcript of k accumulations of m instances (acc.rs:135,158-169): asdl[2 i ..] = alpha, z' (ark).
// xis: the (lg + 1) challenges of instance i m + j at row i m + j (what fs_device writes), U likewise.  On `s`;
// prof_name: the halo_profile_read name of the launch.
int acc_challenges_launch(DeviceState* st, int curve, const void* d_xis, const void* d_U, size_t lg, size_t k, size_t m,
                          void* d_asdl, hipStream_t s, const char* prof_name);

// The scalar-field work of acc.rs:95-101,166 in two launches: per (i, j) the row (U_j, alpha^j) at pts / sc[i m + j]
// (sc is also the weights array of hpoly_combine_device) and the share alpha^j h_j(z') at shares[i m + j]; then per
// accumulation v' = the sum of its shares to v_out[i] (null: not kept) and, with acc_C (verifier mode), the addend
// -acc_C at neg_C[i] and bits[i] |= ACC_BIT_Z where z' differs from acc_z[i] (or acc_z[i] is not below the
// modulus), ACC_BIT_V likewise for v'.
int acc_terms_launch(int curve, const void* d_asdl, const void* d_xis, const void* d_U, const void* d_acc_C,
                     const void* d_acc_z, const void* d_acc_v, size_t lg, size_t k, size_t m, void* d_pts, void* d_sc,
                     void* d_shares, void* d_neg_C, void* d_bits, void* d_v_out, hipStream_t s, const char* prof_name);

// What acc_common_device leaves on the device for halo_acc_prover (in st->scratch[5], valid until the next call).
struct AccResident {
    const void *xis, *weights;  // k m (lg + 1) challenges; k m powers of alpha
};

struct AccCall {  // the arguments of halo_acc_verifier_batch over device pointers
    int curve;
    size_t d, k, m;
    const void *C, *z, *v, *Ls, *Rs, *U, *c, *hiding, *C_bar, *w_prime;  // the k m instances, row i m + j
    const void *acc_C, *acc_z, *acc_v;                                   // null together: common_subroutine alone
    void *verdict, *first_bad, *asdl_out, *C_bar_out, *v_out;            // first_bad .. v_out may be null
    AccResident* resident = nullptr;
};

// common_subroutine (and, with acc_C, the verifier's comparisons) for k accumulations, all on `s` with no host wait:
// fs_device over the k m instances, the ASDL transcript, the terms, the t = m linear combination, the verdicts.
// st->mu and a ScratchUse of `s` held, a.k >= 1, the arguments checked.  Works in st->scratch[5] (and, through
// fs_device, st->scratch[7] and st->lincomb_terms).
int acc_common_device(const char* call, DeviceState* st, const AccCall& a, hipStream_t s);

}  // namespace halo
