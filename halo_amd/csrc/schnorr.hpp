// The device-level pieces of schnorr.hip for the unit that builds on them (schnorr_combined.hip).
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

}  // namespace halo
