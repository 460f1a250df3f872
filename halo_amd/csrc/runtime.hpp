// Host-side runtime shared by every translation unit of libhalo_gpu.so: error reporting,
// per-device state, device memory helpers.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/halo_gpu.h"
#include "scratch_layout.hpp"

namespace halo {

// ---- errors ---------------------------------------------------------------------------------
int set_error(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();

#define HALO_HIP(expr)                                                                      \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return ::halo::set_error(HALO_EDEVICE, "%s failed: %s (%s:%d)", #expr,          \
                                     hipGetErrorString(_e), __FILE__, __LINE__);            \
    } while (0)

#define HALO_CHECK(expr)              \
    do {                              \
        int _rc = (expr);             \
        if (_rc != HALO_OK) return _rc; \
    } while (0)

// ---- tuning (halo_set_tuning): path selections the parity tests pin; read on every use
enum TuneKey { TUNE_IPA_WEIGHTED, TUNE_IPA_TAIL, TUNE_IPA_SRS_TAIL_N, TUNE_IPA_MAT_N, TUNE_MSM_MULTI_MAX, TUNE_IPA_POOL_KEEP,
               TUNE_NTT_BIG_MAX_LOG, TUNE_NTT_EVEN_SPLIT, TUNE_IPA_PAIR_MAX, TUNE_POSEIDON_LANES, TUNE_DECIDE_GROUP_SCALARS,
               TUNE_DECIDE_BISECT, TUNE_DECIDE_RHO_FS, TUNE_SCHNORR_BISECT, TUNE_SCHNORR_BISECT_LEAF,
               TUNE_SCHNORR_BISECT_PASS_ITEMS, TUNE_COUNT };
long long tuning(TuneKey k);

// ---- device buffers ---------------------------------------------------------------------------
// Grow-only device buffer (no shrinking; reused across calls so that timed regions never allocate).
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    int reserve(size_t n);  // ensures capacity >= n bytes
    void release();         // hipFree now (the caller has ordered every user of the buffer before it)
    template <class T>
    T* as() const { return static_cast<T*>(ptr); }
    ~DevBuf();
};

// Per-device, per-curve state (the OnceLock<PublicParams> analogue, crates/group/src/pp.rs:63-94)
struct SrsState {
    DevBuf gs;          // n internal-format affine points (64 B each)
    size_t n = 0;
    bool has_sh = false;
    uint32_t S[16];     // internal packed (x, y)
    uint32_t H[16];
    halo_wrapped_point_t H_wrapped;  // H as uploaded (the key of its 2^i H table)
    DevBuf s_table;     // 2^i S (i < 256), internal affine: hiding term of pedersen::commit
    // 2^i H (i < 128), internal affine: the IPA's H' = xi_0 H terms (halo_ipa_begin_xi), one table per
    // distinct H, never rewritten while the library lives (open sessions keep pointers into them)
    struct HTable {
        uint64_t key[8];  // the WrappedPoint H the table was built from
        DevBuf t;
    };
    std::vector<std::unique_ptr<HTable>> h_tables;
    // d 2^(4 w) G_k (k < small_n0, w < 32, 1 <= d <= 8), XYZZ: small SRS MSMs, IPA tails (tail.hip); shared
    // with the open IPA sessions that read it, so a rebuild never overwrites a buffer in use
    std::shared_ptr<DevBuf> small_tab;
    size_t small_n0 = 0;             // 0 = not built for the current SRS
    hipEvent_t small_tab_ev = nullptr;  // small_tab's build completed
    DevBuf small_scr;                // GLV digits, block partials of a small MSM
    hipEvent_t small_ev = nullptr;   // last small MSM's completion (orders reuse of small_scr)
    DevBuf shifted;     // optional window-shifted copies
    int shifted_c = 0;  // window bits of `shifted` when it holds every window (0: not built)
    int part_c = 0, part_w0 = 0, part_w1 = 0;  // ... or only the windows [part_w0, part_w1) of width part_c
    bool shifted_has_id = true;  // some SRS point is the identity (k_acc then tests every base)
    int shifted_windows = 0;
    // Every writer of `gs` calls this: the tables derived from the old points (window-shifted copies,
    // the small-MSM / tail multiples table) are rebuilt on next use.  (a synthesize after
    // a small commit used to keep the old SRS's table.)
    void invalidate_derived() {
        shifted_c = part_c = 0;
        shifted_windows = 0;
        shifted_has_id = true;
        small_n0 = 0;
    }
};

struct DeviceState {
    int device = -1;
    int num_cu = 256;              // compute units (MI355X: 256), sizes one-round launches
    std::mutex mu;                 // serialises API calls on this device
    SrsState srs[2];               // per curve
    // scratch
    DevBuf scratch[8];
    DevBuf scan_tmp;     // halo_evals_scan_dev block totals
    DevBuf gate_tmp;     // halo_gate_constraints_dev partial vectors
    DevBuf eval_meta[2]; // halo_poly_eval_batch_dev: pointer/length tables, partial sums
    // NTT twiddle caches: key (field, log, inverse)
    struct Twiddles {
        int field, logn, inverse;
        DevBuf hi, lo;
        int lo_bits;
        DevBuf stage;    // stage twiddles: entry 2^s - 1 + k = omega_{2^(s+1)}^k, s < 11 (9 limbs, 48 B each)
        DevBuf pass[4];  // per-pass pre-twiddle tables (logn <= 24), see ntt.hip
        bool has_pass = false;
        uint64_t split = 0;  // the pass split the tables were built for (NttPlan::split_key, tuning-dependent)
    };
    std::vector<std::unique_ptr<Twiddles>> tw;
    struct RTable {
        int field, logr, inverse;
        DevBuf t;
    };
    std::vector<std::unique_ptr<RTable>> rt;
    // Poseidon parameters of each field as the kernels read them (schnorr.hip): 174 constants in limb
    // form, re-uploaded when halo_poseidon_set_params has installed a newer version
    DevBuf poseidon[2];
    uint64_t poseidon_ver[2] = {0, 0};
    DevBuf schnorr_gtab[2];  // per curve: d G and phi(d G), 1 <= d <= 8, XYZZ (the fixed-base table of s G)
    DevBuf schnorr_e;        // the challenges of a verification batch (canonical words)
    // fixed_base.hip: per curve the comb table d 2^(c w) G (internal affine, built on first use, released by
    // halo_shutdown); the derived keys and challenges of a signing batch
    DevBuf fixed_base_tab[2];
    DevBuf schnorr_sign;
    // schnorr_combined.hip: the combined pass's e, liveness, derived weights, MSM terms and outputs; the hash tree,
    // and once the pass has run the descent's prefix sums, node tables and defects (schnorr_bisect.hip)
    DevBuf schnorr_comb[2];
    DevBuf lincomb_terms;   // the terms of a batch of linear combinations (lincomb.hip): packed XYZZ, then a byte each
    DevBuf decider[4];       // decider.hip: h rows / coefficients, half-tables, U' and masks, the xis of a check
    DevBuf bisect[3];        // decider.hip's descent: segment rows, the root's terms, node tables / commitments / defects
    DevBuf decide_rho[2];    // decide_rho.hip: the derived weights (no reserve of decider[] or bisect[] moves them), the hash tree
    // ScratchUse state: completion event of the last scratch user and its stream
    hipEvent_t scratch_ev = nullptr;
    hipStream_t scratch_last = nullptr;
    bool scratch_used = false;
};

// Shared-scratch fence: the device-global scratch buffers (scratch[], scan_tmp, gate_tmp, eval_meta)
// are used by calls on different streams (the caller's torch stream, IPA session streams, the null
// stream of the host-array calls).  Every call that touches them holds a ScratchUse for its stream:
// the stream first waits for the last other-stream user's completion event, and the call records a
// new one when it ends, so the uses are ordered on the device whatever the streams.  (The API mutex
// only orders the enqueueing.)
struct ScratchUse {
    DeviceState* st;
    hipStream_t s;
    ScratchUse(DeviceState* st, hipStream_t s);
    ~ScratchUse();
};

// Current device's state (calls halo_init(current device) lazily).  Returns nullptr on failure
// (with the error set).
DeviceState* current_state();

// Pinned staging helpers
int copy_h2d(void* dst, const void* src, size_t bytes, hipStream_t s);
int copy_d2h(void* dst, const void* src, size_t bytes, hipStream_t s);
// The arrays of a host call (scratch_layout.hpp) as one buffer, st->scratch[0], copied on `s`; dev[j]: row j on
// the device, null for a row of no bytes.  st->mu and a ScratchUse of `s` held.
int upload_parts(DeviceState* st, const HostParts& parts, hipStream_t s, std::vector<const void*>& dev);

// Preconditions the entry points share (each keeps its own message for a bad id).
inline bool valid_curve(int c) { return c == HALO_PALLAS || c == HALO_VESTA; }
inline bool valid_field(int f) { return f == HALO_FP || f == HALO_FQ; }
// The resident SRS of `curve` covers the degree bound d and, where the call needs them, has (S, H).  st->mu held.
// `call` names the entry point in the (S, H) message only: it may be null when need_sh is false, never otherwise.
int check_verifier_srs(const char* call, const DeviceState* st, int curve, size_t d, bool need_sh);

// ---- measurement hooks (halo_profile_*) ----------------------------------------------------
// ProfScope owns a start/stop hipEvent pair for one launch when profiling is enabled; the launch
// goes through hipExtLaunchKernelGGL, which records the kernel's own start/stop on its stream
// (HALO_LAUNCH), so the measured time is the kernel's execution only.
bool prof_enabled();
struct ProfScope {
    int slot = -1;
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s = nullptr;
    ProfScope(const char* name, hipStream_t stream);  // name null: an untimed launch
    ~ProfScope();
};

// A count that is no launch (the permutations of the sponge handles, sponge.hip): added to the `launches` that
// halo_profile_read reports under `name`, while profiling is enabled.
void prof_count(const char* name, size_t count);

#define HALO_LAUNCH(prof, kern, grid, block, shmem, stream, ...)                                      \
    do {                                                                                              \
        if ((prof).slot >= 0)                                                                         \
            hipExtLaunchKernelGGL(kern, grid, block, shmem, stream, (prof).a, (prof).b, 0, __VA_ARGS__); \
        else                                                                                          \
            hipLaunchKernelGGL(kern, grid, block, shmem, stream, __VA_ARGS__);                        \
    } while (0)

// ---- halo_shutdown: what each subsystem releases while the HIP runtime is alive -----------------
// Destroys the MSM pipeline's streams and events (halo_shutdown).
void msm_shutdown();
// Releases the pooled IPA sessions (halo_shutdown, ipa.hip).
void ipa_shutdown();

inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
inline unsigned ilog2(size_t n) {
    unsigned r = 0;
    while ((size_t(1) << (r + 1)) <= n) r++;
    return r;
}
// blocks of `threads` lanes that cover n items (at least one)
inline unsigned grid_for(size_t n, unsigned threads) { return (unsigned)std::max<size_t>(1, (n + threads - 1) / threads); }

}  // namespace halo
