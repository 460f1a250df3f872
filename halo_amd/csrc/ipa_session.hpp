// The IPA session as its units see it (ipa.hip: the pool, the rounds and folds; pcdl_open.hip: the
// hiding open that fills a session before its rounds; pcdl_open_fs.hip: the opening whose transcript runs
// on the device): the struct, the pool, the layouts of the session's small device buffer and pinned staging.
#pragma once
#include <memory>

#include "ipa_plan.hpp"
#include "msm.hpp"
#include "runtime.hpp"

using halo::BatchScratch;
using halo::DevBuf;
using halo::GForm;
using halo::IpaPlan;

// The per-opening half of a session: value-initialised by ipa_acquire (halo_ipa_session::reset_state is one
// assignment, so a field added here cannot survive into the next pooled opening).
struct IpaOpening {
    int curve = 0;
    size_t n = 0;
    // The form of G, the half-length m of the next round and, in the weighted and tail rounds, n0 and the length
    // of the fold weights: ipa_plan.hpp, which also decides what every round and fold launches.
    IpaPlan g;
    int wcur = 0;                  // w[wcur] holds the fold weights
    const uint4* table = nullptr;  // tail multiples table: own_table, or the SRS's small table
    size_t table_ld = 0;
    std::shared_ptr<DevBuf> table_ref;  // keeps the SRS's table alive while the session reads it
    bool slots_reset = false;         // this opening restarted the MSM slot assignment (msm_slots_reset)
    bool fold_inflight = false;       // a fold's H2D copy of xi may still read `pinned`
    bool fold_pending = false;        // tail rounds: the last fold is applied by the next launch (k_tail_prep)
    bool w_one_pending = false;       // entered the tail rounds: w = [1] is written by the next tail launch
    halo_fe_t pend_xi{}, pend_xinv{};
    size_t pend_m = 0;                // the half-length m the pending fold folds (g.m is half of it already)
    bool htab_waited = false;         // round 1 waited for it (later rounds follow a host sync of round 1)
    // xi mode (halo_ipa_begin_xi / _dev_xi / halo_pcdl_open_start): the hiding terms use the resident
    // 2^i H table and the dots scaled by xi_0 (dot H' = (dot xi_0) H), so there is neither H' nor a
    // per-session table
    bool xi_mode = false;
    const void* htab_ptr = nullptr;  // 2^i H' (own table) or 2^i H (SrsState::h_tables)
    bool started = false;            // rounds may run (a pcdl open session starts at halo_pcdl_open_start)
    bool blinded = false;            // halo_pcdl_open_blind ran (pbar holds p_bar)
    bool combined = false;           // halo_pcdl_open_combine ran
    // the transcript runs on the device (pcdl_open_fs.hip): the folds read xi | xi^-1 at SM_XI, which the
    // round's transcript kernel wrote, and no round or fold waits for the host
    bool xi_dev = false;

    bool tail() const { return g.form == GForm::Tail; }
    bool weighted() const { return g.form == GForm::Weighted; }
};

// One opening.  Sessions are pooled per device (ipa_acquire / ipa_release): the streams, events,
// pinned staging and every device buffer survive halo_ipa_end and are reused by the next opening,
// so an opening allocates nothing once the pool is warm (~11 hipMallocs, two stream
// creations and a pinned allocation per opening; ADVICE r02: the buffers leaked at end).
struct halo_ipa_session {
    // ---- resources (kept across pooled uses)
    int device = -1;
    hipStream_t s = nullptr;
    hipStream_t s2 = nullptr;           // weighted rounds above ipa_pair_max: R's MSM (created on first use)
    bool solo = true;                   // the round call advances this session alone (s2 is used then)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t htab_ready = nullptr;  // recorded after the session's own 2^i H' table
    hipEvent_t lr_ready = nullptr;    // halo_ipa_round_lr_dev: L, R copied out (created on first use)
    uint8_t* pinned = nullptr;  // coherent host staging (layout: PIN_* below)
    uint32_t poll_seq = 0;      // the last tail round's flag value (monotonic over the session object's life)
    bool poll_pending = false;  // the last round emits L / R to `pinned` itself: poll instead of synchronising
    DevBuf gs, cs, zs, htab, small, tmp, pbar;
    DevBuf cs2, zs2;  // ping-pong partners of cs / zs (tail rounds with a deferred fold)
    DevBuf own_table, w[2], scal, side, part;
    BatchScratch mat;  // weighted -> tail switch (msm_shared_batch)
    // handed out by ipa_acquire and not yet returned by ipa_release (guarded by g_pool_mu): every
    // session entry point refuses a handle that is not open, and a second end cannot pool it twice
    bool in_use = false;
    // ---- per-opening state (reset by ipa_acquire)
    IpaOpening op;

    void reset_state() { op = IpaOpening{}; }

    // every device buffer; sized_by_n: all but the small staging and the H' table
    template <class F>
    void each_buffer(F&& f) {
        for (DevBuf* d : {&htab, &small}) f(*d, false);
        for (DevBuf* d : {&gs, &cs, &zs, &cs2, &zs2, &tmp, &pbar, &own_table, &w[0], &w[1], &scal, &side, &part,
                          &mat.digits, &mat.lists, &mat.keys, &mat.vals, &mat.bstart, &mat.partials, &mat.bucket_sums,
                          &mat.window_sums})
            f(*d, true);
    }
    size_t buffer_bytes() {
        size_t b = 0;
        each_buffer([&](DevBuf& d, bool) { b += d.bytes; });
        return b;
    }
    void release_large() {  // everything sized by n (the small staging and the H' table stay)
        each_buffer([](DevBuf& d, bool sized_by_n) {
            if (sized_by_n) d.release();
        });
    }
    void destroy() {
        if (s) (void)hipStreamSynchronize(s);
        if (s2) (void)hipStreamSynchronize(s2);
        if (htab_ready) (void)hipEventDestroy(htab_ready);
        if (lr_ready) (void)hipEventDestroy(lr_ready);
        lr_ready = nullptr;
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (s) (void)hipStreamDestroy(s);
        if (s2) (void)hipStreamDestroy(s2);
        s2 = nullptr;
        ev_fork = ev_join = nullptr;
        if (pinned) (void)hipHostFree(pinned);
        s = nullptr;
        htab_ready = nullptr;
        pinned = nullptr;
        each_buffer([](DevBuf& d, bool) { d.release(); });
    }
};

// layout of a session's pinned staging (ses->pinned, PIN_BYTES of coherent host memory):
//   [128, 192) xi|xi_inv (H2D), [256, 512) L|R XYZZ (D2H or tail_emit_host),
//   [512, 520) the L / R flags of tail_emit_host: coherent, several sessions in flight
//   [0, 32) a scalar out (v, w') | [32, 96) C' out (wrapped); the hiding open's XYZZ sums C_bar / C' at
//   [128, 256) with w' beside them; at the end U at [256) with c after it (wrapped: [320), XYZZ: [384))
//   an opening with its transcript on the device: [528) status word, [544) v, [576) alpha, [1024, 5120) the
//   proof's L_j | R_j (WrappedPoints, 128 B per round)
constexpr size_t PIN_FE = 0, PIN_CP = 32, PIN_XI = 128, PIN_XINV = 160, PIN_T = 128, PIN_T_WP = 256, PIN_L = 256,
                 PIN_R = 384, PIN_FLAGS = 512, PIN_U = 256, PIN_U_C = 320, PIN_U_C_XYZZ = 384;
constexpr size_t PIN_STATUS = 528, PIN_V = 544, PIN_ALPHA = 576, PIN_PROOF = 1024, PIN_BYTES = 5120;

// small-buffer layout of a session (ses->small, device):
//   [0, 32) z | [64, 128) H' (or H) | [128, 192) dots | [192, 224) xi_0 | [256, 384) U | c
//   [384, 448) xi | xi^-1 | [512, 768) L | R XYZZ
//   hiding open: [1024) w_bar, [1056) alpha, [1088) w, [1120) w' out, [1152) C, [1216) C_bar out,
//   [1280) S (internal), [1344) C' out
//   transcript on the device (pcdl_open_fs.hip): [2048, 2160) the PCDL sponge's state (poseidon::STATE_U4: three
//   base-field elements, then the squeezed flag and the counter n), [2176) the status word (nonzero: a round
//   challenge was zero), [4096, 8192) the proof's L_j | R_j as WrappedPoints (SM_ROUNDS_MAX rounds)
constexpr size_t SM_BYTES = 8192;
constexpr size_t SM_Z = 0, SM_HP = 64, SM_DOT_L = 128, SM_DOT_R = 160, SM_XI0 = 192, SM_U = 256,
                 SM_U_C = 320, SM_U_C_XYZZ = 384,  // c beside U: after a WrappedPoint, after a packed XYZZ point
                 SM_XI = 384, SM_XINV = 416, SM_L = 512, SM_R = 640;
constexpr size_t SM_WBAR = 1024, SM_ALPHA = 1056, SM_W = 1088, SM_WP = 1120, SM_C = 1152, SM_CBAR = 1216, SM_S = 1280,
                 SM_CP = 1344, SM_NEGW = 1408, SM_T = 1536, SM_V = 1696,  // SM_T: 128 B XYZZ
                 SM_HKW = 1728,  // 2 x 10 words: the dots' GLV splits (k_tail_digits -> k_tail_round)
                 SM_CTR = 1856;  // 2 x u32 arrival counters of k_tail_round, 1 of k_weighted_prep (zero between launches)
constexpr size_t SM_SPONGE = 2048, SM_STATUS = 2176, SM_PROOF = 4096, SM_ROUNDS_MAX = 32;

namespace halo {

// xi | xi^-1 (ark words) as one by-value kernel argument
struct ArkScalarPair {
    uint4 v[4];
};

// ---- the session pool (ipa.hip) ---------------------------------------------------------------
// A session for the current device: from the pool, or new with its streams and pinned staging.
halo_ipa_session* ipa_acquire(DeviceState* st);
// the handle is an open session: handed out by ipa_acquire and not yet released
bool ipa_is_open(const halo_ipa_session* ses);
// Back to the pool once its stream is idle; beyond the pool's size its resources are released.
void ipa_release(halo_ipa_session* ses);

// ---- what the hiding open (pcdl_open.hip) needs from the session unit (ipa.hip) ---------------
// Phase 1 of a session: G, c (cs_len coefficients, zero-padded to n) and z's powers on the device
int ipa_setup(DeviceState* st, halo_ipa_session* ses, int curve, size_t n, const halo_wrapped_point_t* gs_host,
              const halo_fe_t* cs, size_t cs_len, bool cs_on_device, const halo_fe_t* zs_host, const halo_fe_t* z);
// Phase 2: the hiding terms' table; the rounds may run afterwards
// (xi0_resident: xi mode with xi_0 already at SM_XI0, written by a kernel on the session's stream)
int ipa_start(DeviceState* st, halo_ipa_session* ses, const halo_wrapped_point_t* H_prime, const halo_fe_t* xi0,
              const halo_wrapped_point_t* Hpt, bool xi0_resident = false);
// v = c(z) over the session's first len coefficients, to the host (stream sync)
int ipa_eval_cs(halo_ipa_session* ses, size_t len, halo_fe_t* v_out);
// ... its launches alone: v (ark) at SM_V, no copy and no wait
int ipa_eval_cs_enqueue(halo_ipa_session* ses, size_t len);

// ---- what an opening with its transcript on the device (pcdl_open_fs.hip) drives, st->mu held -----
// Enqueues one round's L and R (packed XYZZ at SM_L / SM_R when the session's stream reaches that point)
int ipa_round_launch(DeviceState* st, halo_ipa_session* ses);
// Enqueues one fold; xi / xi_inv may be null for a session with xi_dev set (SM_XI / SM_XINV are read)
int ipa_fold_launch(DeviceState* st, halo_ipa_session* ses, const halo_fe_t* xi, const halo_fe_t* xi_inv);
// halo_ipa_end in two halves: U and c enqueued with their copy to the pinned staging; the wait and the
// host conversion
int ipa_end_enqueue(DeviceState* st, halo_ipa_session* ses);
int ipa_end_finish(halo_ipa_session* ses, halo_wrapped_point_t* U, halo_fe_t* c);

}  // namespace halo
