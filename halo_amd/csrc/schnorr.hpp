// The device-level pieces of schnorr.hip for the units that build on them (schnorr_combined.hip, schnorr_bisect.hip),
// and those of schnorr_combined.hip for schnorr_bisect.hip.
#pragma once
#include "runtime.hpp"

namespace halo {

// hash_message for k (pk, R, message) triples on `s`: e as ark scalars at d_e_ark and as canonical words at
// d_e_words (k x 32 B each; either may be null).  st->mu held, the Poseidon parameters installed.
int schnorr_hash_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_msgs, size_t msg_len,
                        size_t k, void* d_e_ark, void* d_e_words, hipStream_t s);
// The exact verdicts s_i G == R_i + e_i pk_i over challenges already on the device (d_e_words: what
// schnorr_hash_device wrote): one k_schnorr_verify launch on `s`.  st->mu held; the first call per device and
// curve builds the generator's table and waits for it.
int schnorr_ladder_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s,
                          const void* d_e_words, size_t k, void* d_ok, hipStream_t s);
// Everything a Schnorr entry point checks before the device lookup; done: an empty batch.
int check_schnorr_args(const char* call, int curve, const void* pk, const void* R, const void* s, bool need_s,
                       const void* msgs, size_t msg_len, size_t k, const void* out, bool& done);

// ---- the combined pass (schnorr_combined.hip) for the descent below it (schnorr_bisect.hip) ----
constexpr int SIG_THREADS = 256;
constexpr int SIG_WAVES = SIG_THREADS / 64;

// st->schnorr_comb[0] for a batch of k: what one combined pass or one derivation keeps on the device.
struct SigScratch {
    size_t nb;  // blocks of k_sig_prepare
    // bad: nb block flags, then the batch's flag (a live item with a bad rho), then the pass's `combined` byte
    uint8_t *e_ark, *live, *rho, *bases, *scalars, *partials, *bad, *D;
    const void* rho_used;  // the weights the pass ran under: the caller's, or `rho`
};
// The combined pass, every launch on `s`, no host wait: d_ok[i] = live_i && combined, the byte also at d_combined
// (may be null) and at w.bad[w.nb + 1].  d_rho null: derived weights.  st->mu and a ScratchUse of `s` held, k >= 1
// within sig_check_args' bound.  Leaves e's canonical words in st->schnorr_e for the exact ladder, and in `w` the MSM's
// terms (item i: bases and scalars 2 i, 2 i + 1), the liveness bytes and the defect D (packed XYZZ).
int sig_combined_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s, const void* d_msgs,
                        size_t msg_len, size_t k, const void* d_rho, void* d_ok, void* d_combined, hipStream_t s, SigScratch& w);
// check_schnorr_args, and the k whose 2 k + 1 terms msm_device takes.
int sig_check_args(const char* call, int curve, const void* pk, const void* R, const void* s, const void* msgs, size_t msg_len,
                   size_t k, const void* out, bool& done);
// A rejected combined pass resolved per item (schnorr_bisect.hpp's descent under the tuning keys schnorr_bisect_leaf
// and schnorr_bisect_pass_items): d_ok[i] = live_i, cleared for every wrong item.  `w`: what sig_combined_device left,
// its combined byte 0 and its bad-rho flag clear.  Waits for `s` once per level.  Works in st->schnorr_comb[1].
int sig_bisect_device(DeviceState* st, int curve, const void* d_pk, const void* d_R, const void* d_s, size_t k,
                      const SigScratch& w, void* d_ok, hipStream_t s);

}  // namespace halo
