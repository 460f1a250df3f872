// The device-level succinct check of pcdl_fs.hip for the units that build on it (plonk_verify.hip).
#pragma once
#include "runtime.hpp"

namespace halo {

struct FsCall {  // the arguments of either entry point of halo_pcdl_succinct_check_fs_batch
    int curve;
    size_t d, k;
    const void *C, *z, *v, *Ls, *Rs, *U, *c, *hiding, *C_bar, *w_prime;
    void *xis_out, *alpha_out, *ok;
};

// The launches of one call over device pointers, all on `s`: st->mu and a ScratchUse of `s` held, a.k >= 1,
// the arguments checked.  Works in st->scratch[7] and st->lincomb_terms.
int fs_device(const char* call, DeviceState* st, const FsCall& a, hipStream_t s);

// What the host entry points share (halo_pcdl_check_fs_batch, decider.hip): the checks that need no device
// (done: an empty batch), the scalars of a host call below the modulus (host_scalar.hpp), its inputs as the rows
// of upload_parts, and the call over the device pointers `at` that upload_parts answers (its outputs null).
int check_fs_args(const char* call, const FsCall& a, bool& done);
int fs_host_scalars(const char* call, const FsCall& host);
HostParts fs_host_parts(const FsCall& host);
FsCall fs_dev_call(const FsCall& host, const std::vector<const void*>& at);

}  // namespace halo
