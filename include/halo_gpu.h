/*
 * halo_gpu.h -- C ABI of the MI355X (gfx950) backend for the rasmus-kirk/halo proving hot path.
 *
 * Every entry point replaces one reference function (or the arkworks call inside it) on the path
 * named by BASELINE.json's north_star, or on its batched Schnorr verification (crates/plonk/src/main.rs:
 * 35-47; the Poseidon hashes of that batch run on the device, a single Fiat-Shamir transcript remains
 * the caller's); the reference interface each one stands in for is cited
 * next to it (paths relative to the reference root).  A Rust `extern "C"` shim that binds these
 * symbols is given in INTEGRATION.md.
 *
 * Conventions
 *  - Field elements (`halo_fe_t`): 4 x u64 little-endian limbs in arkworks Montgomery form
 *    (R = 2^256), canonical in [0, p) -- the in-memory layout of `ark_ff::Fp256` / `BigInt<4>`,
 *    so `&[Fr]` can be passed zero-copy.
 *  - Points (`halo_wrapped_point_t`): `WrappedPoint { x: [u64; 4], y: [u64; 4] }`
 *    (crates/group/src/wrappers.rs:592-597, #[repr(C)]), affine, Montgomery limbs; the identity is
 *    (0, 0) (`PastaAffine::identity`, wrappers.rs:91-93).  Every point-valued result is returned in
 *    this canonical affine form, so results compare bit-exactly.
 *  - Curves: HALO_PALLAS (base field Fq, scalars Fp = ark_pallas::Fr), HALO_VESTA (base Fp,
 *    scalars Fq).  Fields: HALO_FP (ark_pallas::Fr), HALO_FQ (ark_pallas::Fq)
 *    (crates/group/src/lib.rs:8-9).
 *  - Host-pointer entry points take caller-owned host buffers, borrowed for the call only.
 *    `_dev` entry points take device pointers (hipMalloc'd on the current device) plus a
 *    `hipStream_t` passed as `void*` (NULL = default stream) and are asynchronous with respect to
 *    the host unless stated otherwise.
 *  - Errors: the reference panics (`assert!`) on contract violations; this ABI never aborts and
 *    returns a nonzero `halo_status_t` instead, with the reference's panic message available from
 *    `halo_last_error()` (thread-local).
 *  - Thread safety: every call is re-entrant.  Device-resident state (SRS, twiddles, scratch) is
 *    per (device, curve/field), created once under a mutex (mirrors the `OnceLock<PublicParams>`
 *    of crates/group/src/pp.rs:63-94 and wrappers.rs:28-29).
 */
#ifndef HALO_GPU_H
#define HALO_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } halo_fe_t;
typedef struct { uint64_t x[4]; uint64_t y[4]; } halo_wrapped_point_t;

typedef enum { HALO_PALLAS = 0, HALO_VESTA = 1 } halo_curve_t;
typedef enum { HALO_FP = 0, HALO_FQ = 1 } halo_field_t;

typedef enum {
    HALO_OK = 0,
    HALO_EINVAL = 1,     /* bad argument (null pointer, unknown curve/field, length mismatch) */
    HALO_ENOMEM = 2,     /* device allocation failed */
    HALO_EDEVICE = 3,    /* HIP runtime / kernel error, or no GPU */
    HALO_ENOTPOW2 = 4,   /* "n ({n}) is not a power of two"  (pcdl.rs:282, pp.rs:32) */
    HALO_ESRSRANGE = 5,  /* "d ({d}) <= D ({D})" / SRS too short (pcdl.rs:284, pp.rs:33) */
    HALO_EDEGREE = 6,    /* "p_deg ({p_deg}) <= d ({d})" (pcdl.rs:283) */
    HALO_ELENGTH = 7     /* "ms must be larger than Gs" (pedersen.rs:14-19) */
} halo_status_t;

/* ------------------------------------------------------------------ runtime */
/* Selects the HIP device used by subsequent calls from this thread and creates its context. */
int halo_init(int device);
/* Number of visible GPUs (0 when no GPU is present). */
int halo_device_count(void);
/* Message of the last failed call on this thread ("" if none). */
const char* halo_last_error(void);
/* ABI version (major * 100 + minor). */
int halo_abi_version(void);
/* Releases the library's streams, events and pending profiling events while the HIP runtime is
 * alive (call before process exit; the Python mirror registers it with atexit).  Idempotent; the
 * library remains usable afterwards. */
int halo_shutdown(void);
/* Blocks until all work queued by this library on `stream` is complete. */
int halo_stream_sync(void* stream);
/* Path-selection tuning (library-wide, read by every later call; value -1 restores the default).
 * Keys: "ipa_weighted" (1: IPA rounds over the resident window-shifted SRS without folding G; 0:
 * GLV-fold G every round), "ipa_tail" (1: switch to the direct-sum tail rounds at length 2048),
 * "ipa_srs_tail_n" (SRS openings of n <= this run tail rounds from round 1; default 4096),
 * "ipa_mat_n" (weighted rounds materialise G at this length; 0 = never; default 2048),
 * "msm_multi_max" (commitment batches of polynomials up to this length run as one MSM; default
 * 2^18), "ipa_pool_keep_bytes" (an idle pooled IPA session keeps at most this many bytes of device
 * buffers; default 2^30), "ipa_pair_max" (weighted rounds up to this half-length form L and R as one
 * MSM; default 2^19), "ntt_big_max_log" (NTTs up to 2^this use 11-bit passes; default 22),
 * "ntt_even_split" (1: stages split evenly over the passes; default 0), "poseidon_lanes" (lanes per sponge
 * of the batched Poseidon kernels, 1 or 3; default 0: by batch size), "decide_group_scalars" (the exact batched
 * decider commits its instances in groups whose coefficient rows hold at most this many scalars; default 2^25),
 * "decide_bisect" (what the host forms of the batched decider do with a combined batch that is rejected: 0, the
 * default, decide every live instance again in exact mode; 1 bisect the batch on the device, see
 * halo_pcdl_decide_bisect_dev), "decide_rho_fs" (what a NULL rho means to the batched decider's entry points: 0, the
 * default, exact mode; 1 combined mode with weights derived from the batch by Fiat-Shamir on the device, see
 * halo_pcdl_decide_rho; each call reads it once, on entry), "schnorr_bisect" (what halo_schnorr_verify_combined does
 * with a combined batch that is rejected: 0, the default, the ladder over every item; 1 the descent of
 * halo_schnorr_verify_bisect_dev), "schnorr_bisect_leaf" and "schnorr_bisect_pass_items" (that descent's L and c).
 * Every setting but "decide_rho_fs" = 1 and "schnorr_bisect" = 1 yields the same results (the first trades the exact
 * accept of a NULL rho for the bound stated at halo_pcdl_decide_rho, the second the exact accept of an item inside a
 * rejected batch for the bound stated at halo_schnorr_verify_bisect_dev); the parity
 * tests pin each path with it.  The reference has no counterpart (host-side knob of this backend only).
 * HALO_EINVAL on an unknown key. */
int halo_set_tuning(const char* key, long long value);
int halo_get_tuning(const char* key, long long* value);

/* ------------------------------------------------------------------ a10: SRS provider
 * Replaces PublicParams::{new, set_pp, get_pp} (crates/group/src/pp.rs:26-94): the SRS bases Gs,
 * S and H become device-resident once per (device, curve).  `gs` is the decoded
 * `Vec<WrappedPoint>` of crates/group/.precompute/<curve>/gs-XX.bin (or any prefix of it). */
int halo_srs_upload(halo_curve_t curve, const halo_wrapped_point_t* gs, size_t n,
                    const halo_wrapped_point_t* S, const halo_wrapped_point_t* H);
/* f3: PublicParams::new(n) from the wire format (pp.rs:26-61): `blocks` are the gs-XX.bin files
 * (bincode-v2 standard() Vec<WrappedPoint>, decoded in order until n points), `sh` is sh.bin
 * ((S, H); may be NULL).  Decoded and curve-checked on the device; the reference's panics map to
 * HALO_ENOTPOW2 ("assertion failed: n.is_power_of_two()"), HALO_ESRSRANGE (n > available points),
 * HALO_EINVAL ("Failed to decode G_BLOCKS_NO i", "assertion failed: affine.is_on_curve()"). */
int halo_srs_load_bincode(halo_curve_t curve, const uint8_t* const* blocks, const size_t* block_lens, size_t nblocks,
                          const uint8_t* sh, size_t sh_len, size_t n);
/* Current resident SRS length (0 if none). */
int halo_srs_len(halo_curve_t curve, size_t* n);
/* The resident PublicParams' (S, H) (crates/group/src/pp.rs:26-61) as WrappedPoints. */
int halo_srs_sh(halo_curve_t curve, halo_wrapped_point_t* S, halo_wrapped_point_t* H);
/* Synthetic SRS for sizes beyond the reference's N = 2^20 (crates/group/src/consts.rs:1):
 * G_j = k_j * (-1, 2) with k_j from halo_synth_scalar(seed, j), generated on the device.
 * S, H as in the reference are left unchanged if already uploaded. */
int halo_srs_synthesize(halo_curve_t curve, size_t n, uint64_t seed);
/* The canonical (non-Montgomery) discrete log k_j used by halo_srs_synthesize (host function; lets
 * a verifier check MSM results over synthetic bases in O(n) field operations). */
void halo_synth_scalar(halo_curve_t curve, uint64_t seed, uint64_t j, uint64_t out_canonical[4]);
/* Precomputes the window-shifted copies 2^(c*w) * G_i of the resident SRS used by the
 * single-bucket-set MSM (trades HBM capacity for the per-window combination); optional. */
int halo_srs_precompute_windows(halo_curve_t curve);
/* The copies of windows [w_lo, w_hi) only, of width c bits (c = 0: the default width for the SRS
 * length; w_hi = 0: every window): one rank of a window-partitioned MSM holds just its own windows
 * (BASELINE configs[4]); such a partial set serves halo_msm_srs_windows_dev over that range only (the
 * other SRS MSMs then run without shifted copies). */
int halo_srs_precompute_window_range(halo_curve_t curve, int c, int w_lo, int w_hi);

/* Copies resident SRS points Gs[offset .. offset + n) back to the host as WrappedPoints. */
int halo_srs_read(halo_curve_t curve, size_t offset, size_t n, halo_wrapped_point_t* out);

/* ------------------------------------------------------------------ a3/a4: MSM
 * sum_{i < min(n_bases, n_scalars)} scalars[i] * bases[i]
 * Replaces `Projective::msm_unchecked` as called by group::point_dot_affine
 * (crates/group/src/group.rs:48-50) and pedersen::commit (crates/accumulation/src/pedersen.rs:21).
 * Empty input -> identity (0, 0). */
int halo_msm(halo_curve_t curve, const halo_wrapped_point_t* bases, size_t n_bases,
             const halo_fe_t* scalars, size_t n_scalars, halo_wrapped_point_t* out);
/* Same over the resident SRS prefix Gs[0..n) (the pcdl::commit path, pcdl.rs:286). */
int halo_msm_srs(halo_curve_t curve, const halo_fe_t* scalars, size_t n, halo_wrapped_point_t* out);
/* pedersen::commit(w, Gs, ms) (crates/accumulation/src/pedersen.rs:7-27): asserts
 * Gs.len() >= ms.len(), MSM, then + S*w when `w` is non-NULL. */
int halo_pedersen_commit(halo_curve_t curve, const halo_fe_t* w, const halo_wrapped_point_t* gs,
                         size_t n_gs, const halo_fe_t* ms, size_t n_ms, halo_wrapped_point_t* out);
/* pcdl::commit(p, d, w) (crates/accumulation/src/pcdl.rs:275-287): n = d + 1 must be a power of
 * two, deg(p) <= d <= D, then pedersen::commit(w, Gs[0..n], p.coeffs) over the resident SRS.
 * `coeffs` has `len` entries (trailing zeros allowed). */
int halo_pcdl_commit(halo_curve_t curve, const halo_fe_t* coeffs, size_t len, size_t d,
                     const halo_fe_t* w, halo_wrapped_point_t* out);
/* The hiding branch of pcdl::open_without_eval (crates/accumulation/src/pcdl.rs:344-371), in the
 * two steps around the caller's transcript challenge alpha = rho(C, C_bar, z, v):
 *   blind:   p_bar = (X - z) q (q: d coefficients, the reference's random q of degree d - 1) and the
 *            hiding commitment C_bar = pcdl::commit(p_bar, d, w_bar); p_bar_out (d + 1, optional).
 *   combine: p' = p + alpha p_bar (d + 1 coefficients; p has len <= d + 1), w' = w + alpha w_bar,
 *            C' = C + alpha C_bar - w' S, over the resident SRS's S.
 * Same assertions as the reference (n = d + 1 > 1 a power of two, d <= D); needs (S, H) uploaded. */
int halo_pcdl_hiding_blind(halo_curve_t curve, const halo_fe_t* q, size_t d, const halo_fe_t* z,
                           const halo_fe_t* w_bar, halo_fe_t* p_bar_out, halo_wrapped_point_t* C_bar_out);
int halo_pcdl_hiding_combine(halo_curve_t curve, const halo_fe_t* p, size_t len, const halo_fe_t* p_bar, size_t d,
                             const halo_fe_t* alpha, const halo_wrapped_point_t* C, const halo_wrapped_point_t* C_bar,
                             const halo_fe_t* w, const halo_fe_t* w_bar, halo_fe_t* p_prime_out,
                             halo_fe_t* w_prime_out, halo_wrapped_point_t* C_prime_out);
/* group::point_dot(xs, &[Projective]) (crates/group/src/group.rs:53-56, called at
 * crates/accumulation/src/acc.rs:166): bases are ark Projective points -- Jacobian (X, Y, Z), each
 * coordinate 4 x u64 Montgomery, 96 B per point, Z = 0 the identity -- normalised on the device
 * (Projective::normalize_batch), then the MSM; length = min(n_bases, n_scalars). */
int halo_point_dot_projective(halo_curve_t curve, const halo_fe_t* scalars, size_t n_scalars,
                              const uint64_t (*bases)[12], size_t n_bases, halo_wrapped_point_t* out);
/* Device-pointer MSM: d_bases (n WrappedPoints, or NULL to use the resident SRS prefix) and
 * d_scalars (n halo_fe_t) in HBM; result written to host `out`.  Synchronous on `stream`. */
int halo_msm_dev(halo_curve_t curve, const void* d_bases, const void* d_scalars, size_t n,
                 halo_wrapped_point_t* out, void* stream);
/* Asynchronous device MSM for batches of commitments: enqueues the MSM on `stream` and returns;
 * the 64-B result lands in device memory d_out.  Consecutive calls pipeline: the reduction tail
 * of MSM k overlaps the accumulation of MSM k+1 (two scratch sets, a per-device tail stream).
 * Buffers must stay valid until halo_msm_join(stream) has been ordered before their reuse. */
int halo_msm_dev_async(halo_curve_t curve, const void* d_bases, const void* d_scalars, size_t n,
                       void* d_out, void* stream);
/* Makes `stream` wait (device-side, no host sync) for every asynchronous MSM still in flight. */
int halo_msm_join(void* stream);
/* Batched commitments over the resident SRS prefix: k independent MSMs, MSM i over d_scalars[i]
 * (device pointer, lens[i] <= SRS length ark scalars), result i (64-B WrappedPoint) at
 * d_out + 64 i.  Replaces a loop of pcdl::commit / pedersen::commit calls over one SRS -- the
 * reference's commitment batches (crates/plonk/src/plonk/protocol.rs:114,263 -- 16 commits each;
 * crates/plonk/src/plonk/trace.rs:188-192).  All inputs must be ready on `stream` at the call;
 * asynchronous like halo_msm_dev_async (halo_msm_join before reading d_out).  Polynomials of up to
 * 2^18 coefficients (HALO_MSM_MULTI_MAX) form ONE MSM whose sort keys are (polynomial, bucket); longer
 * ones run as back-to-back pipelined MSMs. */
int halo_msm_batch_dev(halo_curve_t curve, const void* const* d_scalars, const size_t* lens, size_t k, void* d_out,
                       void* stream);
/* Window-partitioned MSM (BASELINE configs[4]): one rank's share -- the signed digits of windows
 * [w_lo, w_hi) of the n scalars against the resident window-shifted copies 2^(c w) G_i -- as a 64-B
 * partial sum at d_out (asynchronous, halo_msm_join).  Partials of a partition of [0, W) add up to
 * the full MSM (pedersen.rs:21).  halo_srs_windows gives W (0 without the shifted copies); the range
 * must lie inside the resident copies (all of them, or halo_srs_precompute_window_range's range). */
int halo_msm_srs_windows_dev(halo_curve_t curve, const void* d_scalars, size_t n, int w_lo, int w_hi, void* d_out,
                             void* stream);
int halo_srs_windows(halo_curve_t curve);
/* Sum of k points (host arrays) on the device: the combine step after an RCCL all-gather of
 * per-rank partial MSMs (RCCL has no elliptic-curve reduction operator). */
int halo_point_sum(halo_curve_t curve, const halo_wrapped_point_t* pts, size_t k, halo_wrapped_point_t* out);
/* Device variant: k WrappedPoints at d_pts (stride_bytes = 64) summed into d_out, on `stream`. */
int halo_point_sum_dev(halo_curve_t curve, const void* d_pts, size_t k, size_t stride_bytes, void* d_out,
                       void* stream);
/* rows independent sums at once (one launch): row b sums the k WrappedPoints d_pts[b k .. b k + k) into
 * d_out[b] -- the combine of `rows` point-partitioned MSMs after one all-gather (bench.py --gpus N). */
int halo_point_sum_rows_dev(halo_curve_t curve, const void* d_pts, size_t rows, size_t k, void* d_out, void* stream);
/* The same sum over packed XYZZ points (128 B each: X, Y, ZZ, ZZZ in the library's internal Montgomery
 * form, as halo_ipa_round_lr_dev writes them), stride_bytes apart, into one packed XYZZ point: no
 * affine conversion (and no inversion) on the device.  A distributed opening sums its ranks' L_r, R_r
 * with it and converts the one sum on the host (halo_xyzz_to_wrapped). */
int halo_point_sum_xyzz_dev(halo_curve_t curve, const void* d_pts, size_t k, size_t stride_bytes, void* d_out,
                            void* stream);
/* k packed XYZZ points (host memory) -> affine WrappedPoints (host binary extended Euclid). */
int halo_xyzz_to_wrapped(halo_curve_t curve, const void* xyzz, size_t k, halo_wrapped_point_t* out);
/* Window size the device MSM uses for n points. */
int halo_msm_window_bits(size_t n);
/* Window size of the resident SRS's window-shifted copies (halo_srs_precompute_windows), or 0 when
 * they are not built (MSMs against the resident SRS then use halo_msm_window_bits). */
int halo_srs_window_bits(halo_curve_t curve);

/* ------------------------------------------------------------------ a5/a6/a7: NTT
 * Radix-2 domain of size N = 2^log_n, omega = 5^((p-1)/N) (ark-poly Radix2EvaluationDomain,
 * crates/group/src/poly.rs:11).  Natural order in and out. */
/* In-place forward (evals[i] = p(omega^i)) or inverse (includes the N^-1 scaling). */
int halo_ntt(halo_field_t field, halo_fe_t* inout, unsigned log_n, int inverse);
/* Evals::from_poly(_ref) / DensePolynomial::evaluate_over_domain(_by_ref) (poly.rs:56-64):
 * `len` coefficients (len may exceed N: reduced mod X^N - 1 first) -> N evaluations. */
int halo_evaluate_over_domain(halo_field_t field, const halo_fe_t* coeffs, size_t len,
                              unsigned log_n, halo_fe_t* evals);
/* Evals::interpolate(_by_ref) (poly.rs:133-139): N evaluations -> coefficients with trailing
 * zeros trimmed (`*out_len` = trimmed length, <= N). */
int halo_interpolate(halo_field_t field, const halo_fe_t* evals, unsigned log_n, halo_fe_t* coeffs,
                     size_t* out_len);
/* &DensePolynomial * &DensePolynomial (FFT multiply; protocol.rs:132-139, pcdl.rs:215):
 * out has room for la + lb - 1 entries; *out_len = trimmed length. */
int halo_poly_mul(halo_field_t field, const halo_fe_t* a, size_t la, const halo_fe_t* b, size_t lb,
                  halo_fe_t* out, size_t* out_len);
/* Batched device NTT: `batch` contiguous transforms of size 2^log_n at d_data, in place.  log_n <= 30 and
 * batch <= 65535 (HALO_EINVAL otherwise, before the device is looked up); batch = 0 is a success that launches
 * nothing, as the empty shapes of halo_transpose_dev and halo_ntt_twiddle_dev are.  The same limits hold for
 * halo_ntt_dev_zero_tail, whose nonzero_len <= 2^log_n is checked once log_n has passed. */
int halo_ntt_dev(halo_field_t field, void* d_data, unsigned log_n, size_t batch, int inverse,
                 void* stream);
/* Forward halo_ntt_dev for inputs that are zero from index nonzero_len on (a polynomial of degree
 * < nonzero_len evaluated over a larger domain, protocol.rs:89-106): the tail's contents are ignored
 * (the caller need not clear it) and the first pass skips the stages that only replicate values. */
int halo_ntt_dev_zero_tail(halo_field_t field, void* d_data, unsigned log_n, size_t batch,
                           size_t nonzero_len, void* stream);
/* Distributed-NTT building blocks (four-step decomposition, halo_amd/dist.py sharded_ntt; SURVEY
 * §8e).  halo_ntt_twiddle_dev: element (a, b) of the rows x cols matrix at d_data (ark format) is
 * multiplied by omega_N^((row0 + a)(col0 + b)) (omega^-1 when inverse), N = 2^log_n.
 * halo_transpose_dev: for `batch` consecutive rows x cols matrices whose elements are runs of `run`
 * 32-byte field elements: dst[s][b][a] = src[s][a][b]. */
int halo_ntt_twiddle_dev(halo_field_t field, void* d_data, unsigned log_n, size_t rows, size_t cols, size_t row0,
                         size_t col0, int inverse, void* stream);
int halo_transpose_dev(const void* d_src, void* d_dst, size_t batch, size_t rows, size_t cols, size_t run,
                       void* stream);

/* ------------------------------------------------------------------ f4: h(X) and the decider MSM
 * HPoly::get_poly (pcdl.rs:198-219): coefficients of h(X) = prod_{i<lg n} (1 + xi_{lg n-i} X^(2^i)),
 * lg n = n_xis - 1, generated directly (coef[j] = product of xi_{lg n-b} over the set bits b of j). */
int halo_hpoly_coeffs(halo_field_t field, const halo_fe_t* xis, size_t n_xis, halo_fe_t* out);
/* sum_i alphas[i] * h_i(X) over k h-polynomials (xis: k rows of n_xis; acc.rs:89); alphas NULL = 1;
 * *out_len (if not NULL) = trimmed length. */
int halo_hpoly_combine(halo_field_t field, const halo_fe_t* xis, size_t k, size_t n_xis, const halo_fe_t* alphas,
                       halo_fe_t* out, size_t* out_len);
/* The same combination into a device buffer d_out (2^(n_xis - 1) ark coefficients, untrimmed), stream-
 * ordered on `stream` (acc::prover's h(X) stays on the device for its commitment and opening). */
int halo_hpoly_combine_dev(halo_field_t field, const halo_fe_t* xis, size_t k, size_t n_xis,
                           const halo_fe_t* alphas, void* d_out, void* stream);
/* pcdl::check step 5 (pcdl.rs:579): pedersen::commit(None, &pp.Gs[0..d+1], &h.get_poly().coeffs)
 * against the resident SRS, the coefficients never leaving the device. */
int halo_pcdl_decider_commit(halo_curve_t curve, const halo_fe_t* xis, size_t n_xis, size_t d,
                             halo_wrapped_point_t* out);

/* ------------------------------------------------------------------ f2: Trace::new batch
 * trace.rs:165-192: k evaluation vectors (k x 2^log_n, row-major) -> Evals::from_vec_and_domain
 * (rotate right by one) -> interpolate (iNTT) -> pcdl::commit(poly, d, None) each; the pcdl::commit
 * assertions and messages apply per row.  coeffs_out (k x 2^log_n, untrimmed) and lens_out (trimmed
 * lengths) are optional. */
int halo_trace_commit_batch(halo_curve_t curve, const halo_fe_t* evals, size_t k, unsigned log_n, size_t d,
                            halo_fe_t* coeffs_out, size_t* lens_out, halo_wrapped_point_t* commits_out);

/* ------------------------------------------------------------------ f1: evaluation algebra
 * Evals ops (crates/group/src/poly.rs:90-327), elementwise over n ark scalars:
 *   op 0 add (a + b), 1 sub (a - b), 2 mul (a * b), 3 scale (a * scalar), 4 add_scalar, 5 sub_scalar,
 *   6 pow (a^exponent, e.g. the Poseidon S-box x^7).  out may alias a or b. */
int halo_evals_op(halo_field_t field, int op, const halo_fe_t* a, const halo_fe_t* b, const halo_fe_t* scalar,
                  uint32_t exponent, halo_fe_t* out, size_t n);
int halo_evals_op_dev(halo_field_t field, int op, const void* d_a, const void* d_b, const halo_fe_t* scalar,
                      uint32_t exponent, void* d_out, size_t n, void* stream);
/* DensePolynomial::divide_by_vanishing_poly (ark-poly 0.5.0; protocol.rs:256): division by
 * X^n - 1; quotient (room for len - n) and remainder (room for n), both trimmed. */
int halo_divide_by_vanishing(halo_field_t field, const halo_fe_t* coeffs, size_t len, size_t n, halo_fe_t* quotient,
                             size_t* q_len, halo_fe_t* remainder, size_t* r_len);
/* Device-resident variant (no trimming): d_coeffs has len >= n entries; quotient len - n entries
 * (may be null when len == n), remainder n entries. */
int halo_divide_by_vanishing_dev(halo_field_t field, const void* d_coeffs, size_t len, size_t n,
                                 void* d_quotient, void* d_remainder, void* stream);
/* Gate-constraint evaluation of naive_prover round 4 (protocol.rs:170-191 with the constraint
 * polynomials of protocol.rs:591-1011), fused into one pass over the n-point (8x) domain: d_w (16),
 * d_r (15), d_q (10) device evaluation vectors, d_pi the public-input evaluations, w_omega = d_w[0..3]
 * shifted left by `shift`; mds = the 3 x 3 Poseidon MDS matrix (row-major, ark).  d_out = f_gc. */
int halo_gate_constraints_dev(halo_field_t field, const void* const* d_w, const void* const* d_r,
                              const void* const* d_q, const void* d_pi, const halo_fe_t* mds, size_t n,
                              unsigned shift, void* d_out, void* stream);
/* Running product of the permutation argument (protocol.rs:143-154): inclusive prefix product
 * out[i] = prod_{j<=i} in[j] over n device elements (reverse != 0: suffix product prod_{j>=i}). */
int halo_evals_scan_dev(halo_field_t field, int reverse, const void* d_in, void* d_out, size_t n, void* stream);
/* sum_i zeta^i p_i (protocol.rs:542-548, the geometric combinations of round 5) over k <= 64 device
 * coefficient vectors d_polys[i] of lens[i] ark elements (shorter ones zero-extended) into d_out
 * (n_out elements, n_out >= max lens[i]), one launch on `stream`. */
int halo_poly_lincomb_dev(halo_field_t field, const void* const* d_polys, const size_t* lens, size_t k,
                          const halo_fe_t* zeta, void* d_out, size_t n_out, void* stream);

/* ------------------------------------------------------------------ a8: evaluation / dots */
/* DensePolynomial::evaluate (Horner; pcdl.rs:49,471), k polynomials at one point z. */
int halo_poly_eval_batch(halo_field_t field, const halo_fe_t* const* polys, const size_t* lens,
                         size_t k, const halo_fe_t* z, halo_fe_t* out);
/* Device-resident variant: d_polys is a host array of k device pointers (ark coefficients);
 * d_out receives k device field elements.  Stream-ordered. */
int halo_poly_eval_batch_dev(halo_field_t field, const void* const* d_polys, const size_t* lens, size_t k,
                             const halo_fe_t* z, void* d_out, void* stream);
/* group::scalar_dot (crates/group/src/group.rs:43-45). */
int halo_scalar_dot(halo_field_t field, const halo_fe_t* xs, const halo_fe_t* ys, size_t n,
                    halo_fe_t* out);
/* group::construct_powers (crates/group/src/group.rs:58-66): out[i] = z^i, i < n. */
int halo_construct_powers(halo_field_t field, const halo_fe_t* z, size_t n, halo_fe_t* out);

/* ------------------------------------------------------------------ a9: IPA folding
 * The round loop of pcdl::open_without_eval (crates/accumulation/src/pcdl.rs:404-438) with the
 * vectors device-resident across rounds; the caller keeps the Fiat-Shamir transcript and
 * supplies xi each round.  Session lifecycle:
 *   begin(cs = p'.coeffs resized to n, z, H') -> per round: round_lr -> (transcript) -> fold
 *   -> end(U = G[0], c = c[0]).  gs starts as the resident SRS prefix Gs[0..n) (pcdl.rs:393). */
typedef struct halo_ipa_session halo_ipa_session;
int halo_ipa_begin(halo_curve_t curve, const halo_fe_t* cs, size_t n, const halo_fe_t* z,
                   const halo_wrapped_point_t* H_prime, halo_ipa_session** out);
/* As halo_ipa_begin with the n coefficients already on the device (ark format; null stream order). */
int halo_ipa_begin_dev(halo_curve_t curve, const void* d_cs, size_t n, const halo_fe_t* z,
                       const halo_wrapped_point_t* H_prime, halo_ipa_session** out);
/* The same sessions with pcdl::open_without_eval's H' = xi_0 H (pcdl.rs:390-391) formed inside:
 * the caller passes H (WrappedPoint) and xi_0 (ark) instead of H'; the hiding terms <c, z> H' of
 * every round use a 2^i H table (built once per H and kept) with the dots scaled by xi_0, so a
 * session needs neither the scalar multiplication for H' nor its own 2^i H' doubling chain. */
int halo_ipa_begin_xi(halo_curve_t curve, const halo_fe_t* cs, size_t n, const halo_fe_t* z,
                      const halo_wrapped_point_t* H, const halo_fe_t* xi0, halo_ipa_session** out);
int halo_ipa_begin_dev_xi(halo_curve_t curve, const void* d_cs, size_t n, const halo_fe_t* z,
                          const halo_wrapped_point_t* H, const halo_fe_t* xi0, halo_ipa_session** out);
/* Session over explicit vectors G (WrappedPoints), c, z of length n (power of two >= 2) instead of
 * the SRS prefix and the powers of z: one rank's shard of a distributed opening (the
 * strided split G[i P + r] keeps every fold pair on one rank) and its collapsed final rounds. */
int halo_ipa_begin_vectors(halo_curve_t curve, const halo_wrapped_point_t* gs, const halo_fe_t* cs,
                           const halo_fe_t* zs, size_t n, const halo_wrapped_point_t* H_prime,
                           halo_ipa_session** out);
/* pcdl::open_without_eval (crates/accumulation/src/pcdl.rs:326-392) as one session whose p, p_bar
 * and p' never leave the device; the caller keeps the transcript between the steps, as the
 * reference does:
 *   halo_pcdl_open_begin(p: len coefficients, d, z)    n = d + 1 > 1 a power of two, p.degree() <= d,
 *                                                      d <= D (pcdl.rs:338-341); c = p padded to n;
 *                                                      v_out (optional) = p(z), pcdl::open's evaluation (pcdl.rs:471)
 *   hiding (w = Some):
 *     halo_pcdl_open_blind(q: d coefficients, w_bar) -> C_bar       p_bar = (X - z) q,
 *                                                      C_bar = pcdl::commit(p_bar, d, w_bar) (pcdl.rs:344-355)
 *     (transcript: absorb_g(C, C_bar), absorb_fr(z, v), alpha = challenge)
 *     halo_pcdl_open_combine(alpha, C, w) -> w', C'  c = p + alpha p_bar, w' = w + alpha w_bar,
 *                                                      C' = C + alpha C_bar - w' S (pcdl.rs:366-371)
 *   (transcript: absorb_g(C'), absorb_fr(z, v), xi_0 = challenge)
 *   halo_pcdl_open_start(H, xi_0)                     H' = xi_0 H (pcdl.rs:390; H = NULL: the resident
 *                                                      SRS's pp.H), then the rounds
 * followed by halo_ipa_round_lr / halo_ipa_fold / halo_ipa_end as for the other sessions.  The
 * rounds refuse a session that was not started. */
int halo_pcdl_open_begin(halo_curve_t curve, const halo_fe_t* p, size_t len, size_t d, const halo_fe_t* z,
                         halo_fe_t* v_out, halo_ipa_session** out);
int halo_pcdl_open_blind(halo_ipa_session* s, const halo_fe_t* q, const halo_fe_t* w_bar, halo_wrapped_point_t* C_bar);
int halo_pcdl_open_combine(halo_ipa_session* s, const halo_fe_t* alpha, const halo_wrapped_point_t* C,
                           const halo_fe_t* w, halo_fe_t* w_prime, halo_wrapped_point_t* C_prime);
int halo_pcdl_open_start(halo_ipa_session* s, const halo_wrapped_point_t* H, const halo_fe_t* xi0);
/* pcdl::open_without_eval / pcdl::open (pcdl.rs:326-473) as ONE call over host arrays and the resident SRS
 * with its (S, H): the PCDL transcript (Sponge::new(Protocols::PCDL), pcdl.rs:336) runs on the device, so
 * the lg n rounds are one chain of launches with one wait at the end; the caller brings no sponge.
 * halo_poseidon_set_params must have installed the parameters of the curve's base field.
 *   p: len coefficients; the assertions of halo_pcdl_open_begin: n = d + 1 > 1 a power of two,
 *      p.degree() <= d, d <= D
 *   v: the claimed evaluation, or NULL: pcdl::open, v = p(z) is formed on the device (pcdl.rs:471)
 *   w: the commitment's randomness, or NULL: the plain branch.  With w: q (d coefficients) and w_bar are the
 *      draws the reference takes from its rng (pcdl.rs:347,352), and C_bar, w_prime receive the proof's
 *      hiding part (all four required; alpha comes back to the host once, between halo_pcdl_open_blind's
 *      and halo_pcdl_open_combine's work)
 *   Ls, Rs: lg n WrappedPoints each; U, c; v_out (optional): the v the transcript absorbed
 * A round challenge that is zero (the reference unwraps its inverse, pcdl.rs:430) is HALO_EINVAL.  Argument
 * errors name the call and are reported before the device is touched; missing Poseidon parameters are
 * HALO_EINVAL, no GPU is HALO_EDEVICE.  The session the call uses goes back to the pool on every path. */
int halo_pcdl_open_fs(halo_curve_t curve, const halo_fe_t* p, size_t len, size_t d, const halo_fe_t* z,
                      const halo_fe_t* v, const halo_wrapped_point_t* C, const halo_fe_t* w, const halo_fe_t* q,
                      const halo_fe_t* w_bar, halo_wrapped_point_t* Ls, halo_wrapped_point_t* Rs,
                      halo_wrapped_point_t* U, halo_fe_t* c, halo_wrapped_point_t* C_bar, halo_fe_t* w_prime,
                      halo_fe_t* v_out);
/* k plain pcdl::open calls of one degree bound d over device-resident coefficient vectors (d_p[i]: lens[i] <=
 * d + 1 ark scalars on the device, ordered on the null stream as for halo_ipa_begin_dev; the length
 * stands for the degree), at z[i] with commitment C[i]: each opening has its own pooled session and
 * stream, and every session's whole chain is enqueued before any is waited for (Instance::open twice
 * in the prover's round 5).  Opening i's rounds are Ls[i lg n + j], Rs[i lg n + j]; U[i], c[i]; v_out
 * (optional) receives v[i] = p_i(z[i]).  k = 0 is HALO_OK.  An argument error opens no session. */
int halo_pcdl_open_fs_dev_multi(halo_curve_t curve, size_t k, const void* const* d_p, const size_t* lens, size_t d,
                                const halo_fe_t* z, const halo_wrapped_point_t* C, halo_wrapped_point_t* Ls,
                                halo_wrapped_point_t* Rs, halo_wrapped_point_t* U, halo_fe_t* c, halo_fe_t* v_out);
/* L = <c_r, G_l> + H' <c_r, z_l>,  R = <c_l, G_r> + H' <c_l, z_r>  (pcdl.rs:412-418) */
int halo_ipa_round_lr(halo_ipa_session* s, halo_wrapped_point_t* L, halo_wrapped_point_t* R);
/* G_l[j] = G_l[j] + xi G_r[j] (affine), c_l[j] += xi^-1 c_r[j], z_l[j] += xi z_r[j]; m /= 2
 * (pcdl.rs:427-437).  xi_inv may be NULL: the library forms xi^-1 on the host (binary extended
 * Euclid), as the reference's fold does itself; xi = 0 is HALO_EINVAL. */
int halo_ipa_fold(halo_ipa_session* s, const halo_fe_t* xi, const halo_fe_t* xi_inv);
/* k independent openings advanced in lockstep (each session has its own stream; all k rounds /
 * folds are enqueued before any is waited for, so the openings overlap on the device): L[i], R[i]
 * of session i; xi[i], xi_inv[i] for session i (xi_inv NULL: formed on the host).  The fold checks
 * every session and xi before it enqueues any fold: an argument error (a null, closed or repeated
 * session, xi = 0) leaves all k sessions unfolded. */
int halo_ipa_round_lr_multi(halo_ipa_session* const* ses, size_t k, halo_wrapped_point_t* L,
                            halo_wrapped_point_t* R);
int halo_ipa_fold_multi(halo_ipa_session* const* ses, size_t k, const halo_fe_t* xi, const halo_fe_t* xi_inv);
/* One round whose L, R stay on the device: d_lr (256 B of device memory) receives L then R as packed XYZZ
 * (halo_point_sum_xyzz_dev's format), ordered before later work on `stream`; no host wait.  The
 * distributed opening's per-round reduce (pcdl.rs:412-418 summed over the ranks' shards):
 * round_lr_dev -> all-gather -> halo_point_sum_xyzz_dev -> one D2H -> halo_xyzz_to_wrapped. */
int halo_ipa_round_lr_dev(halo_ipa_session* s, void* d_lr, void* stream);
/* Current half-length m, and the folded vectors (length 2m) copied back to the host (any of the
 * output pointers may be NULL).  Sessions over the resident SRS do not materialise G in their
 * weighted / tail rounds (the default; HALO_IPA_WEIGHTED=0 and HALO_IPA_TAIL=0 keep G folded every
 * round): asking for gs there is HALO_EINVAL. */
int halo_ipa_state(halo_ipa_session* s, size_t* m, halo_wrapped_point_t* gs, halo_fe_t* cs,
                   halo_fe_t* zs);
/* U = G_0 and c_0 after the last round (in weighted / tail rounds U is only defined then).  The
 * session's streams and device buffers go back to a per-device pool (reused by the next opening;
 * released by halo_shutdown), so a warm opening allocates nothing.  After its end a handle must not
 * be used again: every entry point refuses (HALO_EINVAL) a handle whose session was destroyed or is
 * idle in the pool, but once the pool hands that session to a later opening the old handle names the
 * new opening. */
int halo_ipa_end(halo_ipa_session* s, halo_wrapped_point_t* U, halo_fe_t* c);
/* halo_ipa_end of k lockstep sessions (U[i], c[i] of session i; U or c may be NULL): every session's
 * final U sum is enqueued on its own stream before any is waited for.  Argument errors (a null,
 * closed or repeated session) release nothing; otherwise every listed session is released, also on
 * an error. */
int halo_ipa_end_multi(halo_ipa_session* const* ses, size_t k, halo_wrapped_point_t* U, halo_fe_t* c);
/* One stateless fold over host vectors of length 2m (the loop body of pcdl.rs:427-435), in place
 * on the left halves. */
int halo_ipa_fold_host(halo_curve_t curve, halo_wrapped_point_t* gs, halo_fe_t* cs, halo_fe_t* zs,
                       size_t m, const halo_fe_t* xi, const halo_fe_t* xi_inv);

/* ------------------------------------------------------------------ Poseidon and Schnorr batches
 * The reference's first benchmark verifies 40 000 independent signatures (crates/plonk/src/main.rs:35-47);
 * each is one Poseidon hash of 5 + msg_len base-field elements and two scalar multiplications.  A
 * single Fiat-Shamir transcript stays with the caller (serial host logic); these calls run k
 * independent sponges / verifications as one batch on the device. */
/* Poseidon parameters of `field` (PastaConfig's POSEIDON_MDS / POSEIDON_ROUND_CONSTANTS,
 * crates/group/src/poseidon_consts.rs as used by crates/poseidon/src/inner_sponge.rs:3-108): the 3 x 3
 * MDS matrix row-major and the 55 x 3 round constants, ark Montgomery limbs, canonical.  They are not
 * compiled into the library; set once per process and field (host-only call; each device copies them on
 * its next use), before the hashing and Schnorr calls, which otherwise return HALO_EINVAL. */
int halo_poseidon_set_params(halo_field_t field, const halo_fe_t* mds, const halo_fe_t* rc);
/* k independent inner sponges (inner_sponge.rs:66-108): row i of `in` (k x len, row-major, len >= 0)
 * is absorbed into a fresh sponge, which is squeezed once into out[i].  k = 0 touches nothing; `in`
 * may be NULL when len = 0. */
int halo_poseidon_hash_batch(halo_field_t field, const halo_fe_t* in, size_t len, size_t k, halo_fe_t* out);
int halo_poseidon_hash_batch_dev(halo_field_t field, const void* d_in, size_t len, size_t k, void* d_out, void* stream);
/* hash_message (crates/schnorr/src/lib.rs:24-35) for k (pk, R, message) triples: Sponge::new(
 * Protocols::SIGNATURE), absorb_g_affine(&[pk, R]) (x then y; the identity as (0, 0)), absorb_fq(message),
 * challenge() (crates/poseidon/src/outer_sponge.rs:24-43,51-61,86-95) -> k scalars e of `curve` (ark).
 * msgs: k x msg_len base-field elements of `curve`, row-major; NULL allowed when msg_len = 0. */
int halo_schnorr_hash_batch(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                            const halo_fe_t* msgs, size_t msg_len, size_t k, halo_fe_t* e_out);
int halo_schnorr_hash_batch_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_msgs,
                                size_t msg_len, size_t k, void* d_e_out, void* stream);
/* PublicKey::verify (crates/schnorr/src/lib.rs:71-79) for k signatures (R[i], s[i]) on messages
 * msgs[i] under keys pk[i]: ok_out[i] = 1 iff s G == R + e pk with e = hash_message(pk, R, m) and
 * G = Affine::generator() = (-1, 2), else 0.  s: scalars of `curve` (ark).  Identity pk, identity R and
 * s = 0 follow the reference's arithmetic.  A pk or R that is neither the identity (0, 0) nor on the
 * curve gives 0: the reference's Affine type makes that case unrepresentable (wrappers.rs:606 asserts
 * is_on_curve on conversion), so it has no verdict there. */
int halo_schnorr_verify_batch(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                              const halo_fe_t* s, const halo_fe_t* msgs, size_t msg_len, size_t k, uint8_t* ok_out);
/* The same over device pointers; d_ok: k bytes of device memory.  Asynchronous on `stream` (the first
 * call per device and curve builds the generator's table and waits for it). */
int halo_schnorr_verify_batch_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                  const void* d_msgs, size_t msg_len, size_t k, void* d_ok, void* stream);
/* The same k verifications as ONE MSM under random weights, the method of halo_pcdl_decide_batch's combined mode
 * (opt-in; the calls above and their results are unchanged).  For weights rho_i all of s_i G == R_i + e_i pk_i hold
 * iff D = (sum rho_i s_i) G - sum rho_i R_i - sum (rho_i e_i) pk_i is the identity, up to the bound below; Pallas and
 * Vesta have cofactor 1, so no subgroup caveat applies.  D is one MSM of 2 k + 1 terms whatever k, where the exact
 * call runs k ladders; each e_i is hashed once.  Item i is live iff pk_i and R_i are each (0, 0) or on the curve
 * (the rule above): an item that is not live has verdict 0 and weighs nothing in D; (0, 0) is a legal point and
 * takes part.  k is at most 119 304 646: the 2 k + 1 terms must not exceed 238 609 294 = floor((2^32 - 1) / 18), the
 * largest MSM over caller bases (its sort counts 9 windows of 2 (2 k + 1) GLV half-scalars in 32 bits).
 * rho: k scalars of `curve`, or NULL for the weights of halo_schnorr_batch_rho (no generator needed).
 * If the combined pass holds, ok_out[i] = live_i and *combined_out (may be NULL) = 1.  If it fails, the live items
 * are decided by the exact ladder over the e already on the device and *combined_out = 0: the verdicts are always
 * per item and exact for rejects.  For s below the modulus they equal halo_schnorr_verify_batch's.
 * Soundness: a rho that the caller passes must be drawn uniformly, from the caller's random number generator, AFTER
 * the signatures are fixed (with rho known in advance, errors that cancel pass: s_0 + x, s_1 - x under rho = (1, 1)).
 * An accept is then sound up to a signer guessing rho, probability about k / 2^254; for derived weights about
 * Q k / 2^254 over Q batches tried.  A reject is exact.
 * Before any device work: the errors of halo_schnorr_verify_batch, HALO_EINVAL for a k above the bound and for a
 * rho entry that is zero (its item would go unchecked) or not below the modulus.  k = 0: HALO_OK, nothing touched. */
int halo_schnorr_verify_combined(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                                 const halo_fe_t* s, const halo_fe_t* msgs, size_t msg_len, size_t k, const halo_fe_t* rho,
                                 uint8_t* ok_out, uint8_t* combined_out);
/* The combined pass over device pointers, asynchronous on `stream`, no host wait; d_rho NULL: derived weights, from
 * the inputs as they are on the device.  d_ok[i] = live_i && combined; d_combined (1 byte, may be NULL) = 1 iff the
 * pass held.  It never falls back: with combined = 0 every d_ok byte is 0 and the caller runs
 * halo_schnorr_verify_batch_dev.  A live item whose rho is zero or not below the modulus gives combined = 0. */
int halo_schnorr_verify_combined_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                     const void* d_msgs, size_t msg_len, size_t k, const void* d_rho, void* d_ok,
                                     void* d_combined, void* stream);
/* The combined pass and, where it rejects, per-item verdicts by bisection on the device instead of every ladder
 * (arguments and refusals those of halo_schnorr_verify_combined_dev; d_rho NULL: derived weights; k = 0: HALO_OK).
 * With D(S) the defect above restricted to the items of S, D is additive over disjoint sets, so a failing node
 * [lo, hi) splits into [lo, lo + (hi - lo) / 2) and the rest at the cost of ONE pass: the left half's defect is an MSM
 * over that half's 2 (mid - lo) terms, which the combined pass left on the device, plus one generator multiple from a
 * prefix sum of rho_i s_i, and D(right) = D(node) - D(left).  Nothing is hashed again.  A failing node of one item is
 * a verdict.  Two rules bound the cost under the tuning keys "schnorr_bisect_leaf" (L) and
 * "schnorr_bisect_pass_items" (c, the ladder items that cost as much as one pass): a failing node of at most L items
 * is resolved by the exact ladder over its slice, and before a level of f nodes with p passes done the descent stops
 * if (p + f) c > k, every node of that level going to the ladder.  The passes then never cost more than the ladder
 * over the whole batch, and the ladder slices are disjoint: a rejected batch costs at most about twice the
 * whole-batch ladder, whatever the forger does.  At k < c or k <= L the root goes straight to the ladder (k = 1: the
 * root's defect is the item's own verdict, no ladder runs).
 * d_ok: the per-item verdicts; d_combined (1 byte, may be NULL): the root pass's byte.  The call reads that byte and
 * so waits on `stream`, then once per level of the descent.  A live item whose rho is zero or not below the modulus
 * still gives combined = 0 and every d_ok byte 0, with no descent.
 * Contract: a reject found by the descent is exact (a single item's defect is nonzero iff the item is wrong, its rho
 * being nonzero; the ladder is exact).  An item in a half that passes is accepted up to a signer guessing the
 * weights, about 1 / 2^254 per node tested, for weights drawn after the signatures were fixed: with weights known in
 * advance, errors that cancel inside one half pass there (s_0 + x, s_1 - x under rho = (1, 1)).
 * halo_schnorr_verify_combined takes this descent over a rejected batch, in place of the whole-batch ladder, when the
 * tuning key "schnorr_bisect" is 1 (default 0: unchanged). */
int halo_schnorr_verify_bisect_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s,
                                   const void* d_msgs, size_t msg_len, size_t k, const void* d_rho, void* d_ok,
                                   void* d_combined, void* stream);
/* The weights that a NULL rho means above, derived from the batch itself by Fiat-Shamir on the device, as
 * halo_pcdl_decide_rho derives the decider's: rho_out is k scalars of `curve`, and two runs over one batch agree.
 * All hashing is the curve's sponge (Sponge<P> of outer_sponge.rs) under three protocol labels SIG_BATCH_LEAF = 7,
 * SIG_BATCH_SEED = 8, SIG_BATCH_WEIGHT = 9 that continue halo_pcdl_decide_rho's 4..6.  THE LABELS AND THE DERIVATION
 * ARE THIS BACKEND'S OWN: the reference has no batched verification.
 *   leaf_i   live: a sponge with label 7 does absorb_fr(e_i), absorb_fr(s_i), e_i = hash_message(pk_i, R_i, m_i); the
 *            leaf is its inner sponge's squeeze(), a base-field element.  Not live: the element 0, nothing is read.
 *            e_i is already a collision-resistant digest of (pk_i, R_i, m_i) under SIGNATURE, so it stands for them:
 *            hashing the points and the message a second time would double the dominant cost of the batch.
 *   tree     that of halo_pcdl_decide_rho over the k leaves: N(a, b) a fresh unlabelled inner sponge, an odd node
 *            carried up unchanged.
 *   seed     a sponge with label 8 whose inner sponge absorbs root, k, msg_len, squeezed once.
 *   rho_i    live: a sponge with label 9 whose inner sponge absorbs seed, i; challenge() is the weight, 0 replaced by
 *            1.  Not live: 0.
 * Errors as for halo_schnorr_verify_combined; an s that is not below the modulus is hashed as its residue. */
int halo_schnorr_batch_rho(halo_curve_t curve, const halo_wrapped_point_t* pk, const halo_wrapped_point_t* R,
                           const halo_fe_t* s, const halo_fe_t* msgs, size_t msg_len, size_t k, halo_fe_t* rho_out);
/* The same over device pointers, asynchronous on `stream`: the hash, 3 + ceil(lg k) launches, no host wait. */
int halo_schnorr_batch_rho_dev(halo_curve_t curve, const void* d_pk, const void* d_R, const void* d_s, const void* d_msgs,
                               size_t msg_len, size_t k, void* d_rho_out, void* stream);
/* The signer's half of crates/schnorr/src/lib.rs, with every random scalar drawn by the CALLER: the library never
 * draws randomness.  Both calls multiply the generator G = Affine::generator() = (-1, 2) over a fixed-base comb: a
 * table of the affine multiples d 2^(8 w) G (1 <= d <= 128, w < 32; 256 KiB per device and curve, built on the
 * device by the first call, which waits for it, and released by halo_shutdown), about 32 mixed additions per scalar
 * and no doublings, then one shared inversion per workgroup for the affine results.
 * SECRETS: the host forms zero the device staging that held the scalars before they return.  The kernels index the
 * table by the scalars' digits, skip zero digits and branch on exceptional additions: they are NOT hardened against
 * side channels (timing, cache).  Do not sign on a device shared with an adversary.
 *
 * out[i] = scalars[i] G: generate_keypair's public key (lib.rs:41-43) for caller-drawn secrets.  Scalars of `curve`
 * (ark Montgomery limbs); 0 gives the identity (0, 0).  Needs no Poseidon parameters.
 * Before any device work: HALO_EINVAL for an unknown curve, a null pointer, a k too large to address, and the first
 * scalar that is not below the modulus (naming its index).  k = 0: HALO_OK, nothing touched. */
int halo_generator_mul_batch(halo_curve_t curve, const halo_fe_t* scalars, size_t k, halo_wrapped_point_t* out);
/* The same over device pointers, asynchronous on `stream`.  The scalars must be below the modulus: this is the
 * caller's to ensure and is not checked (a larger value is reduced). */
int halo_generator_mul_batch_dev(halo_curve_t curve, const void* d_scalars, size_t k, void* d_out, void* stream);
/* SecretKey::sign (lib.rs:49-66) for k (sk, message) pairs with the nonces given: R_out[i] = nonce[i] G (affine: the
 * hash absorbs it), e_i = hash_message(pk_i, R_i, msgs[i]) as halo_schnorr_hash_batch, s_out[i] = nonce[i] + e_i sk[i].
 * pk NULL: pk_i = sk[i] G is derived, as the reference does on every sign (lib.rs:59).  A pk that is passed is
 * hashed AS GIVEN: that it belongs to sk is the caller's business, and a wrong one yields signatures that do not
 * verify.  nonce = 0 gives R = (0, 0) and sk = 0 gives pk = (0, 0): the reference's arithmetic, which
 * halo_schnorr_verify_batch follows too.  A nonce must be uniform, secret and never reused across messages.
 * msgs: k x msg_len base-field elements, row-major; NULL allowed only when msg_len = 0.
 * Before any device work: HALO_EINVAL for an unknown curve, a null pointer, msg_len * k overflow, Poseidon parameters
 * not installed, and the first sk or nonce entry that is not below the modulus (naming the array and the index).
 * k = 0: HALO_OK, nothing touched. */
int halo_schnorr_sign_batch(halo_curve_t curve, const halo_fe_t* sk, const halo_wrapped_point_t* pk, const halo_fe_t* nonce,
                            const halo_fe_t* msgs, size_t msg_len, size_t k, halo_wrapped_point_t* R_out, halo_fe_t* s_out);
/* The same over device pointers (d_pk may be NULL), asynchronous on `stream`, no host wait.  d_sk and d_nonce must be
 * below the modulus: not checked.  The caller owns the secrets' device memory and clears it. */
int halo_schnorr_sign_batch_dev(halo_curve_t curve, const void* d_sk, const void* d_pk, const void* d_nonce,
                                const void* d_msgs, size_t msg_len, size_t k, void* d_R_out, void* d_s_out, void* stream);

/* ------------------------------------------------------------------ the PCDL verifier
 * k linear combinations of t terms each, out[i] = add[i] + sum_{j < t} scalars[i t + j] pts[i t + j]
 * (row-major k x t; add NULL: no addend): one variable-base ladder per term over its GLV halves, then one
 * sum per item (equal, opposite and identity partial sums included).  Scalars of `curve` (ark), below the
 * modulus, else HALO_EINVAL.  A term point or an addend that is neither the identity (0, 0) nor on the
 * curve makes its item invalid, and the item's result is (0, 0): the reference's Affine type cannot hold
 * such a point (the rule of halo_schnorr_verify_batch).  t = 0 returns the addends.  The hiding pre-step
 * of the succinct check, C' = C + alpha C_bar - w' S (pcdl.rs:506-515), is one call with t = 2 whose
 * affine result goes back to the caller's transcript. */
int halo_point_lincomb_batch(halo_curve_t curve, const halo_wrapped_point_t* add, const halo_wrapped_point_t* pts,
                             const halo_fe_t* scalars, size_t k, size_t t, halo_wrapped_point_t* out);
/* The same over device pointers, asynchronous on `stream`: d_out_xyzz receives k packed XYZZ points (128 B
 * each, halo_ipa_round_lr_dev's format; convert with halo_xyzz_to_wrapped), d_is_identity (k bytes, may be
 * NULL) 1 where item i is valid and its sum is the identity.  An invalid item -- here also one with a
 * scalar that is not below the modulus -- gives the identity and byte 0. */
int halo_point_lincomb_batch_dev(halo_curve_t curve, const void* d_add, const void* d_pts, const void* d_scalars,
                                 size_t k, size_t t, void* d_out_xyzz, void* d_is_identity, void* stream);
/* Steps 5-10 of pcdl::succinct_check (pcdl.rs:517-550) for k instances of one degree bound d, given the
 * challenges the caller's transcript derived: C_prime[i] (C, or C + alpha C_bar - w' S when hiding), z[i],
 * v[i], xis[i (lg n + 1) + j] = xi_j, Ls / Rs[i lg n + j], U[i], c[i].  The host forms xi_(j+1)^-1, h(z)
 * (HPoly::eval, pcdl.rs:222-235) and e = xi_0 (v - c h(z)); the device sums, per instance,
 * C' + sum_j (xi_(j+1)^-1 L_j + xi_(j+1) R_j) + e H - c U over the resident SRS's H in one lincomb launch
 * of t = 2 lg n + 2 terms.  ok_out[i] = 1 iff every point of instance i is valid and that sum is the
 * identity, i.e. C_(lg n) == c U + v' H' (pcdl.rs:547-550).  Before any device work: HALO_ENOTPOW2
 * "n ({n}) is not a power of two", HALO_ESRSRANGE "d was larger than D!", HALO_EINVAL for a null pointer,
 * a scalar not below the modulus or a zero xi_(j+1) (the reference unwraps its inverse).  k = 0: HALO_OK. */
int halo_pcdl_succinct_check_batch(halo_curve_t curve, size_t d, size_t k, const halo_wrapped_point_t* C_prime,
                                   const halo_fe_t* z, const halo_fe_t* v, const halo_fe_t* xis,
                                   const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
                                   const halo_wrapped_point_t* U, const halo_fe_t* c, uint8_t* ok_out);
/* pcdl::succinct_check (pcdl.rs:483-554) for k raw instances of one degree bound d: each instance's transcript
 * (Sponge::new(Protocols::PCDL), outer_sponge.rs) runs on the device.  Per instance i: C[i], z[i], v[i],
 * Ls/Rs[i lg n + j], U[i], c[i]; hiding (may be NULL: no instance hides) hiding[i] != 0 => C_bar[i], w_prime[i]
 * are read (pcdl.rs:503-515), else ignored.  Optional outputs: xis_out[i (lg n + 1) + j] = xi_j (ark),
 * alpha_out[i] (zero for a non-hiding instance).  ok_out[i] = 1 iff C_(lg n) == c U + v' H'.
 * Needs the resident SRS with (S, H) and halo_poseidon_set_params for the curve's base field.  Before any
 * device work: HALO_ENOTPOW2 "n ({n}) is not a power of two", HALO_EINVAL for a null required pointer, for
 * hiding without C_bar and w_prime, for unset Poseidon parameters and for a z, v, c or read w' that is not
 * below the modulus; then HALO_ESRSRANGE "d was larger than D!" or for a missing (S, H).  k = 0: HALO_OK.
 * A point that is neither (0, 0) nor on the curve gives verdict 0 for its instance alone (that instance's
 * xis_out row is then unspecified).  One deviation from the reference: a derived xi_(j+1) = 0 (probability
 * about 2^-254), whose inverse the reference unwraps, gives verdict 0 here. */
int halo_pcdl_succinct_check_fs_batch(halo_curve_t curve, size_t d, size_t k,
        const halo_wrapped_point_t* C, const halo_fe_t* z, const halo_fe_t* v,
        const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c,
        const uint8_t* hiding, const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime,
        halo_fe_t* xis_out, halo_fe_t* alpha_out, uint8_t* ok_out);
/* The same over device pointers, asynchronous on `stream`; no host wait, no host arithmetic.  Here a
 * scalar that is not below the modulus also gives verdict 0 for its instance. */
int halo_pcdl_succinct_check_fs_batch_dev(halo_curve_t curve, size_t d, size_t k, const void* d_C, const void* d_z,
        const void* d_v, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c, const void* d_hiding,
        const void* d_C_bar, const void* d_w_prime, void* d_xis_out, void* d_alpha_out, void* d_ok, void* stream);

/* acc::decider for k instances of one degree bound d (n = d + 1 a power of two): ok_out[i] = 1 iff
 * U[i] == Commit(Gs[0..d], h_i.coeffs), h_i from xis[i (lg n + 1) + j] = xi_j (the layout xis_out returns; xi_0 is
 * not read).  live (may be NULL: all) live[i] = 0 skips instance i, verdict 0.  A U that is neither (0, 0) nor on
 * the curve gives verdict 0.  A zero xi is legal: h then has zero coefficients, as DensePolynomial would trim.
 * rho NULL, or k = 1: exact mode, one commitment per instance, in groups whose coefficient rows hold at most
 * the tuning key "decide_group_scalars" scalars (default 2^25); up to "msm_multi_max" coefficients a group is one
 * MSM, above it pipelined ones.
 * rho given (k scalars of `curve`): combined mode, sum_i rho_i U_i == Commit(sum_i rho_i h_i) over the live
 * instances, ONE MSM whatever k.  If that fails the live instances are decided again in exact mode (or, with the
 * tuning key "decide_bisect" = 1, the batch is bisected: halo_pcdl_decide_bisect_dev), so the verdicts are always
 * per instance and exact for rejects.  An accept in combined mode is sound up to a prover
 * guessing rho (probability about k / 2^254 over a uniform choice): a rho that the caller passes must be drawn
 * AFTER the proofs are fixed, uniformly, from the caller's random number generator.  The library draws no
 * randomness; with the tuning key "decide_rho_fs" = 1 it derives the weights instead: rho NULL and k >= 2 then
 * means combined mode under the weights of halo_pcdl_decide_rho (for this host form, of the live instances that
 * travel: they are gathered first), and no generator is needed.  k = 1 stays in exact mode.
 * Before any device work: HALO_ENOTPOW2 "n ({n}) is not a power of two", HALO_EINVAL for a null required pointer,
 * an xi that is not below the modulus, a rho entry that is zero (its instance would go unchecked) or not below
 * the modulus, with "decide_rho_fs" = 1 and rho NULL missing Poseidon parameters of the curve's base field; then
 * HALO_ESRSRANGE "d was larger than D!".  k = 0: HALO_OK. */
int halo_pcdl_decide_batch(halo_curve_t curve, size_t d, size_t k, const halo_fe_t* xis, const halo_wrapped_point_t* U,
                           const uint8_t* live, const halo_fe_t* rho, uint8_t* ok_out);
/* The same over device pointers, asynchronous on `stream`, no host wait.  d_combined (1 byte, may be NULL) is
 * written only in combined mode (d_rho given, or derived under "decide_rho_fs" = 1 from d_xis, d_U and d_live as
 * they are on the device, with no host wait): 1 iff the combined check held.  It never falls back: with
 * d_combined = 0 every d_ok byte is 0 and the caller calls again in exact mode (d_rho NULL under "decide_rho_fs" = 0)
 * or bisects.  Skipped instances are still computed in exact mode (the host form leaves them out).  A rho or xi that is not below the modulus gives combined = 0 / an unspecified
 * verdict for its instance. */
int halo_pcdl_decide_batch_dev(halo_curve_t curve, size_t d, size_t k, const void* d_xis, const void* d_U,
                               const void* d_live, const void* d_rho, void* d_ok, void* d_combined, void* stream);
/* Per-instance verdicts of a weighted batch by bisection, over device pointers; d_rho is required unless the
 * tuning key "decide_rho_fs" is 1, when a NULL d_rho means the weights of halo_pcdl_decide_rho_dev.  The combined
 * pass runs first; when it rejects, D(S) = sum_{i in S} rho_i U_i - Commit(sum_{i in S} rho_i h_i) is followed down
 * a binary tree over the instances (left half = the first floor(size / 2) of a node): one combined pass over the
 * left half of every failing node gives D(left), and D(right) = D(node) - D(left) is one point subtraction, so b
 * wrong instances among k cost at most min(k - 1, b ceil(lg k)) MSMs beyond the first, where exact mode costs k.
 * The half-tables and the terms rho_i U_i of the first pass are reused; no scalar multiplication is repeated.
 * UNLIKE THE OTHER _dev FORMS THIS ONE WAITS FOR `stream`: once after the first pass and once per level of the
 * tree, at most 1 + ceil(lg k) times (the launches of a level depend on the flags of the one above).
 * A live instance whose U is neither (0, 0) nor on the curve, or whose rho is zero or not below the modulus, is
 * rejected before the first pass and weighs nothing in any node; U = (0, 0) is a legal point and is decided.
 * Soundness: a reject is exact (a single instance has D != 0 iff it is wrong, because rho_i != 0).  An accept of
 * any subset is sound up to a prover guessing rho: the union bound over the at most 2 k - 1 nodes of the tree
 * gives about 2 k / 2^254 for rho drawn uniformly after the proofs are fixed (for derived weights, Q 2 k / 2^254
 * over Q batches tried).  k = 1 is exact mode.
 * The host forms halo_pcdl_decide_batch, halo_pcdl_check_fs_batch and halo_plonk_verify_batch take this route for
 * a rejected combined batch when the tuning key "decide_bisect" is 1 (the default 0 keeps the exact rerun).
 * Errors: those of halo_pcdl_decide_batch_dev, and HALO_EINVAL for a null d_rho under "decide_rho_fs" = 0. */
int halo_pcdl_decide_bisect_dev(halo_curve_t curve, size_t d, size_t k, const void* d_xis, const void* d_U,
                                const void* d_live, const void* d_rho, void* d_ok, void* stream);
/* The weights of the combined decider derived from the batch itself by Fiat-Shamir, on the device: what a NULL rho
 * means to the calls above and to halo_plonk_verify_batch under the tuning key "decide_rho_fs" = 1, so that a caller
 * brings no random number generator and two runs over the same batch give the same verdicts.  xis, U, live as in
 * halo_pcdl_decide_batch; rho_out: k scalars of `curve`.
 * The decider's statement for instance i is "U_i == Commit(Gs[0..d], h(xi_(i,1..lg n)))", so the batch is d, k, the
 * live mask and the pairs (U_i, xi_(i,1..lg n)); xi_(i,0) is not hashed, and nothing of an instance that is not
 * live is read.  All hashing is the curve's Fiat-Shamir sponge (Sponge<P> of outer_sponge.rs: Poseidon over the
 * base field, absorb_g, absorb_fr, challenge) under three protocol labels BATCH_LEAF = 4, BATCH_SEED = 5,
 * BATCH_WEIGHT = 6 that continue the reference's 0..3.  THE LABELS AND THE DERIVATION ARE THIS BACKEND'S OWN: the
 * reference has no batched decider.
 *   leaf_i   live: a sponge with label 4 does absorb_g(U_i), absorb_fr(xi_(i,1)), ..., absorb_fr(xi_(i,lg n)); the
 *            leaf is its inner sponge's squeeze(), a base-field element.  Not live: the element 0.
 *   tree     level 0 is the k leaves; level l+1 [j] = N(level l [2j], level l [2j+1]) if 2j+1 < count, else
 *            level l [2j] unchanged, until one element, the root, remains.  N(a, b): a fresh unlabelled inner
 *            sponge absorbs a, then b, and squeezes once.  The shape is fixed by k, which the seed binds.
 *   seed     a sponge with label 5 whose inner sponge absorbs root, k, d (the integers as field elements), squeezed once.
 *   rho_i    live: a sponge with label 6 whose inner sponge absorbs seed, i; challenge() is the weight, and a
 *            result of 0 (probability about 2^-254) is replaced by 1.  Not live: 0.
 * Soundness: in the random-oracle model each rho_i is an independent uniform function of the whole statement.  An
 * accept is sound up to a prover who tries Q batches and finds one whose weights cancel, about Q k / 2^254; for the
 * bisection the bound is Q 2 k / 2^254.  A reject stays exact.
 * Before any device work: the argument errors of halo_pcdl_decide_batch (an xi not below the modulus included) and
 * HALO_EINVAL without Poseidon parameters for the curve's base field.  No SRS is needed.  k = 0: HALO_OK; k = 1
 * gives a weight like any other k. */
int halo_pcdl_decide_rho(halo_curve_t curve, size_t d, size_t k, const halo_fe_t* xis, const halo_wrapped_point_t* U,
                         const uint8_t* live, halo_fe_t* rho_out);
/* The same over device pointers, asynchronous on `stream`: 2 + ceil(lg k) launches and no host wait.  An xi that is
 * not below the modulus is hashed as its residue. */
int halo_pcdl_decide_rho_dev(halo_curve_t curve, size_t d, size_t k, const void* d_xis, const void* d_U,
                             const void* d_live, void* d_rho_out, void* stream);
/* pcdl::check (pcdl.rs:563-583) for k raw instances: halo_pcdl_succinct_check_fs_batch, then the decider above
 * with live = the succinct verdicts, the challenges never leaving the device.  The inputs and errors of
 * halo_pcdl_succinct_check_fs_batch, plus rho (NULL: exact mode, or under "decide_rho_fs" = 1 derived weights,
 * with the device's own succinct verdicts as the live mask) with the rule and the errors of halo_pcdl_decide_batch.  ok_out[i]: 0 accept, 1 the succinct check failed ("C_(log_n) != CM.Commit_Sigma(c || v')"),
 * 2 the decider failed ("U != CM.Commit(ck, h_vec)"). */
int halo_pcdl_check_fs_batch(halo_curve_t curve, size_t d, size_t k,
        const halo_wrapped_point_t* C, const halo_fe_t* z, const halo_fe_t* v,
        const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c,
        const uint8_t* hiding, const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime,
        const halo_fe_t* rho, uint8_t* ok_out);
/* The same over device pointers, asynchronous on `stream`; d_combined as in halo_pcdl_decide_batch_dev: with
 * d_rho (or derived weights) and d_combined = 0 the codes 2 are not verdicts (every instance that passed the
 * succinct check has one) and the caller calls again in exact mode (d_rho NULL under "decide_rho_fs" = 0). */
int halo_pcdl_check_fs_batch_dev(halo_curve_t curve, size_t d, size_t k, const void* d_C, const void* d_z,
        const void* d_v, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c, const void* d_hiding,
        const void* d_C_bar, const void* d_w_prime, const void* d_rho, void* d_ok, void* d_combined, void* stream);

/* ------------------------------------------------------------------ the Plonk verifier
 * PlonkProof::verify_succinct (crates/plonk/src/plonk/protocol.rs:357-491) for k raw proofs of one circuit:
 * rows = n (a power of two >= 4, d = n - 1, omega = 5^((r - 1) / n)), the circuit's selector commitments
 * C_qs[10], the scalar Poseidon MDS matrix mds[9] (P::SCALAR_POSEIDON_MDS, row-major) and npi public inputs
 * per proof (public_inputs[i npi + j]; npi may be 0, public_inputs then NULL).  The proofs do not hide
 * (naive_prover and acc::prover open with w = None), so no C_bar / w_prime is carried.  Per proof i:
 *   C_ws[16 i + j], C_z[i], C_ts[16 i + j]         PlonkProofCommitments
 *   vs[78 i + j]                                   PlonkProofEvals in struct order (protocol.rs:36-46): ws 16,
 *                                                  rs 15, qs 10, ts 16, ids 8, sigmas 8, z, z_omega, w_omegas 3
 *   Ls / Rs[(3 i + q) lg n + j], U[3 i + q], c[3 i + q]   the EvalProofs of qs = [acc_prev, instance_1 (r),
 *                                                  instance_2 (r_omega)] (protocol.rs:487), q = 0, 1, 2
 *   acc_prev_{C, z, v}[i], acc_next_{C, z, v}[i]   acc_next.pi is not read (acc.rs:201)
 * Every transcript runs on the device: the PLONK sponge (beta, gamma, alpha, zeta, xi), the PCDL sponge of each
 * of the 3 k instances (halo_pcdl_succinct_check_fs_batch) and the ASDL sponge of acc::verifier.
 * verdict[i] is HALO_PLONK_ACCEPT or the first failing check in the reference's order (halo_plonk_verdict_t).
 * HALO_PLONK_MALFORMED stands for a proof the reference has no verdict for and comes before every check: a
 * point that is neither (0, 0) nor on the curve (the reference's Affine type cannot hold one), or a derived
 * xi with n (xi - omega^j) = 0 for some 1 <= j <= max(npi, 1) (probability about npi 2^-254), where the
 * reference divides by zero in l1 or public_input_eval_generic and panics.  A malformed proof never
 * disturbs its neighbours; its optional outputs are unspecified.
 * Optional outputs (may be NULL): challenges_out[5 i ..] = beta, gamma, alpha, zeta, xi; sides_out[2 i ..] =
 * f(xi) and t(xi) z_H(xi), the two sides of protocol.rs:441-444; asdl_out[2 i ..] = the accumulation's
 * alpha and z' (acc.rs:160,169).
 * Needs the resident SRS with (S, H) and halo_poseidon_set_params for the curve's base field.  Before any
 * device work: HALO_ENOTPOW2 "n ({n}) is not a power of two", HALO_EINVAL for rows < 4, a null required
 * pointer, unset Poseidon parameters or a scalar that is not below the modulus; then HALO_ESRSRANGE
 * "d was larger than D!" or for a missing (S, H).  k = 0: HALO_OK. */
#define HALO_PLONK_EVALS 78
typedef enum {
    HALO_PLONK_ACCEPT = 0,
    HALO_PLONK_IDENTITY = 1,   /* "T(z) != (F_GC(z) + a F_CC1(z) + a^2 F_CC2(z) + ...) / Z_H(z)" (protocol.rs:441-444) */
    HALO_PLONK_INSTANCE_0 = 2, /* succinct check of acc_prev (acc.rs:149) */
    HALO_PLONK_INSTANCE_1 = 3, /* ... of (C_r, d, xi, v_r, pi_r) */
    HALO_PLONK_INSTANCE_2 = 4, /* ... of (C_r_omega, d, xi omega, v_r_omega, pi_r_omega) */
    HALO_PLONK_C_BAR = 5,      /* "C_bar' != C_bar" (acc.rs:207) */
    HALO_PLONK_Z = 6,          /* "z' = z" (acc.rs:208) */
    HALO_PLONK_V = 7,          /* "h(z) = v" (acc.rs:210) */
    HALO_PLONK_MALFORMED = 8,
    HALO_PLONK_DECIDER_SUCCINCT = 9, /* halo_plonk_verify_batch: pcdl::check's succinct check of acc_next (pcdl.rs:547) */
    HALO_PLONK_DECIDER = 10          /* ... "U != CM.Commit(ck, h_vec)" (pcdl.rs:580) */
} halo_plonk_verdict_t;
int halo_plonk_verify_succinct_batch(halo_curve_t curve, size_t rows, size_t k,
        const halo_wrapped_point_t* C_qs, const halo_fe_t* public_inputs, size_t npi,
        const halo_wrapped_point_t* C_ws, const halo_wrapped_point_t* C_z, const halo_wrapped_point_t* C_ts,
        const halo_fe_t* vs, const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c,
        const halo_wrapped_point_t* acc_prev_C, const halo_fe_t* acc_prev_z, const halo_fe_t* acc_prev_v,
        const halo_wrapped_point_t* acc_next_C, const halo_fe_t* acc_next_z, const halo_fe_t* acc_next_v,
        const halo_fe_t* mds, uint8_t* verdict, halo_fe_t* challenges_out, halo_fe_t* sides_out, halo_fe_t* asdl_out);
/* The same over device pointers, asynchronous on `stream`; no host wait, no host arithmetic.  Here a
 * scalar that is not below the modulus gives HALO_PLONK_MALFORMED for its proof (an MDS entry: for all). */
int halo_plonk_verify_succinct_batch_dev(halo_curve_t curve, size_t rows, size_t k,
        const void* d_C_qs, const void* d_public_inputs, size_t npi, const void* d_C_ws, const void* d_C_z,
        const void* d_C_ts, const void* d_vs, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c,
        const void* d_acc_prev_C, const void* d_acc_prev_z, const void* d_acc_prev_v,
        const void* d_acc_next_C, const void* d_acc_next_z, const void* d_acc_next_v, const void* d_mds,
        void* d_verdict, void* d_challenges_out, void* d_sides_out, void* d_asdl_out, void* stream);

/* PlonkProof::verify (protocol.rs:493-502) for k raw proofs of one circuit: verify_succinct as above, then
 * acc::decider of acc_next, i.e. pcdl::check of (acc_next.C, d, acc_next.z, acc_next.v) with
 * acc_next.pi = acc_next_{Ls[i lg n + j], Rs[i lg n + j], U[i], c[i]}.  acc_next's PCDL transcript runs as a fourth
 * instance per proof inside the same chain of launches; the deciders follow as in halo_pcdl_decide_batch, over
 * the proofs whose verdict is still HALO_PLONK_ACCEPT, with rho (NULL: exact mode, or under the tuning key
 * "decide_rho_fs" = 1 the derived weights of halo_pcdl_decide_rho_dev over those proofs) under that call's rule and
 * errors.  verdict[i] is the verify_succinct code if that is nonzero, else HALO_PLONK_DECIDER_SUCCINCT,
 * HALO_PLONK_DECIDER or HALO_PLONK_ACCEPT.  A point of acc_next.pi that is neither (0, 0) nor on the curve gives
 * HALO_PLONK_DECIDER_SUCCINCT.  The errors of halo_plonk_verify_succinct_batch, acc_next_c included. */
int halo_plonk_verify_batch(halo_curve_t curve, size_t rows, size_t k,
        const halo_wrapped_point_t* C_qs, const halo_fe_t* public_inputs, size_t npi,
        const halo_wrapped_point_t* C_ws, const halo_wrapped_point_t* C_z, const halo_wrapped_point_t* C_ts,
        const halo_fe_t* vs, const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c,
        const halo_wrapped_point_t* acc_prev_C, const halo_fe_t* acc_prev_z, const halo_fe_t* acc_prev_v,
        const halo_wrapped_point_t* acc_next_C, const halo_fe_t* acc_next_z, const halo_fe_t* acc_next_v,
        const halo_wrapped_point_t* acc_next_Ls, const halo_wrapped_point_t* acc_next_Rs,
        const halo_wrapped_point_t* acc_next_U, const halo_fe_t* acc_next_c,
        const halo_fe_t* mds, const halo_fe_t* rho, uint8_t* verdict);
/* The same over device pointers, asynchronous on `stream`.  d_combined (1 byte, may be NULL) is written only in
 * combined mode (d_rho, or derived weights); with d_combined = 0 every proof that reached the decider reports
 * HALO_PLONK_DECIDER and the caller calls again in exact mode, d_rho NULL under "decide_rho_fs" = 0 (it never
 * falls back). */
int halo_plonk_verify_batch_dev(halo_curve_t curve, size_t rows, size_t k,
        const void* d_C_qs, const void* d_public_inputs, size_t npi, const void* d_C_ws, const void* d_C_z,
        const void* d_C_ts, const void* d_vs, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c,
        const void* d_acc_prev_C, const void* d_acc_prev_z, const void* d_acc_prev_v,
        const void* d_acc_next_C, const void* d_acc_next_z, const void* d_acc_next_v,
        const void* d_acc_next_Ls, const void* d_acc_next_Rs, const void* d_acc_next_U, const void* d_acc_next_c,
        const void* d_mds, const void* d_rho, void* d_verdict, void* d_combined, void* stream);

/* ------------------------------------------------------------------ the accumulation scheme
 * acc::verifier (crates/accumulation/src/acc.rs:128-176,200-213) for k accumulations of m >= 1 instances each, all of
 * one degree bound d.  Instance j of accumulation i is row i m + j of C, z, v, Ls, Rs, U, c, hiding, C_bar, w_prime,
 * in the layouts and with the meaning of halo_pcdl_succinct_check_fs_batch (hiding NULL: no instance hides); its
 * accumulator is (acc_C[i], d, acc_z[i], acc_v[i]) (acc.pi is not read, acc.rs:201).  Every transcript runs on the
 * device: the PCDL sponge of each of the k m succinct checks and the ASDL sponge of each accumulation (label,
 * absorb_fr of the m (lg n + 1) challenges, absorb_g(U_0 .. U_(m-1)), alpha, z').
 * verdict[i] is HALO_ACC_ACCEPT or the first failing check in the reference's order: the instances in order, then
 * C_bar, z, v.  first_bad[i] (may be NULL) is the index of the failing instance, or m.  Optional outputs:
 * asdl_out[2 i ..] = alpha, z'; C_bar_out[i] = C_bar' = sum_j alpha^j U_j; v_out[i] = sum_j alpha^j h_j(z').
 * acc_C, acc_z, acc_v may be NULL together: the call is then common_subroutine plus the evaluation, the verdicts
 * are ACCEPT or INSTANCE only, and asdl_out, C_bar_out and v_out are required.
 * A point of an instance that is neither (0, 0) nor on the curve gives HALO_ACC_INSTANCE for its accumulation alone;
 * an acc_C that is no point, or differs from C_bar', gives HALO_ACC_C_BAR (C_bar_out[i] is unspecified for an acc_C
 * that is no point or an accumulation with an invalid U).  lg n = 0 (d = 0) is accepted, Ls / Rs may then be NULL.
 * Needs the resident SRS with (S, H) and halo_poseidon_set_params for the curve's base field.  Before any device
 * work: HALO_EINVAL "No instances given" for m = 0, for a null required pointer, for hiding without C_bar and
 * w_prime, for acc_C / acc_z / acc_v only partly given, for unset Poseidon parameters and for a scalar (z, v, c, a
 * read w', acc_z, acc_v) that is not below the modulus; HALO_ENOTPOW2 "n ({n}) is not a power of two"; then
 * HALO_ESRSRANGE "d was larger than D!" or for a missing (S, H).  k = 0: HALO_OK.  No GPU: HALO_EDEVICE. */
typedef enum {
    HALO_ACC_ACCEPT = 0,
    HALO_ACC_INSTANCE = 1, /* a succinct check failed (acc.rs:149); first_bad names the instance */
    HALO_ACC_C_BAR = 2,    /* "C_bar' != C_bar" (acc.rs:207) */
    HALO_ACC_Z = 3,        /* "z' = z" (acc.rs:208) */
    HALO_ACC_V = 4         /* "h(z) = v" (acc.rs:210) */
} halo_acc_verdict_t;
int halo_acc_verifier_batch(halo_curve_t curve, size_t d, size_t k, size_t m,
        const halo_wrapped_point_t* C, const halo_fe_t* z, const halo_fe_t* v,
        const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c,
        const uint8_t* hiding, const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime,
        const halo_wrapped_point_t* acc_C, const halo_fe_t* acc_z, const halo_fe_t* acc_v,
        uint8_t* verdict, uint32_t* first_bad, halo_fe_t* asdl_out, halo_wrapped_point_t* C_bar_out, halo_fe_t* v_out);
/* The same over device pointers, asynchronous on `stream`; no host wait, no host arithmetic.  Here a scalar that
 * is not below the modulus gives its accumulation a failing verdict and leaves the neighbours alone: HALO_ACC_INSTANCE
 * for an instance's scalar, HALO_ACC_Z / HALO_ACC_V for acc_z / acc_v. */
int halo_acc_verifier_batch_dev(halo_curve_t curve, size_t d, size_t k, size_t m, const void* d_C, const void* d_z,
        const void* d_v, const void* d_Ls, const void* d_Rs, const void* d_U, const void* d_c, const void* d_hiding,
        const void* d_C_bar, const void* d_w_prime, const void* d_acc_C, const void* d_acc_z, const void* d_acc_v,
        void* d_verdict, void* d_first_bad, void* d_asdl_out, void* d_C_bar_out, void* d_v_out, void* stream);
/* acc::prover (acc.rs:178-198) of the m instances C[j], z[j], v[j], Ls / Rs[j lg n + ..], U[j], c[j] (hiding, C_bar,
 * w_prime as above) of degree bound d, n = d + 1 >= 2 a power of two: common_subroutine on the device, h(X) =
 * sum_j alpha^j h_j(X) formed on the device from the resident challenges (it never visits the host), one copy of
 * (C_bar, z, v, the verdict) home and one wait, then the plain opening of h at z with commitment C_bar
 * (halo_pcdl_open_fs_dev_multi's chain for k = 1, its PCDL transcript on the device).  That copy of 168 bytes lands
 * in ordinary host memory of the call, not in pinned staging: the only pinned buffers belong to pooled sessions, and
 * none is open before the verdict is known.  The opener's own v = h(z), from the coefficients, is compared with
 * sum_j alpha^j h_j(z) from the product forms; a difference is HALO_EDEVICE.  The accumulator is
 * (acc_C, d, acc_z, acc_v) with acc.pi = (acc_Ls, acc_Rs: lg n WrappedPoints each; acc_U, acc_c).
 * If a succinct check fails the call is still HALO_OK: *verdict = HALO_ACC_INSTANCE, *first_bad (may be NULL) names the
 * instance, no session is opened and the acc_ outputs are untouched; otherwise *verdict = HALO_ACC_ACCEPT and
 * *first_bad = m.  The errors of halo_acc_verifier_batch, and the opener's: HALO_EINVAL "assertion failed: n > 1".
 * The session the opening uses goes back to the pool on every path. */
int halo_acc_prover(halo_curve_t curve, size_t d, size_t m,
        const halo_wrapped_point_t* C, const halo_fe_t* z, const halo_fe_t* v,
        const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c,
        const uint8_t* hiding, const halo_wrapped_point_t* C_bar, const halo_fe_t* w_prime,
        halo_wrapped_point_t* acc_C, halo_fe_t* acc_z, halo_fe_t* acc_v,
        halo_wrapped_point_t* acc_Ls, halo_wrapped_point_t* acc_Rs, halo_wrapped_point_t* acc_U, halo_fe_t* acc_c,
        uint8_t* verdict, uint32_t* first_bad);

/* ------------------------------------------------------------------ the Fiat-Shamir sponge as an object
 * Sponge<P> (crates/poseidon/src/outer_sponge.rs:11-100) for the transcripts no fused call walks: a handle owns k
 * sponges that advance in lockstep (every call applies one operation to all k, on different data; k = 1 is the
 * ordinary sponge), their states in device memory between calls.  protocol: Protocols::{PCDL = 0, ASDL = 1,
 * PLONK = 2, SIGNATURE = 3}, absorbed as the first element (Sponge::new).  A handle is an integer id that is never
 * reused within a process; it belongs to the device that was current when it was made.  Arrays are (k, n)
 * row-major: row i goes to / comes from sponge i.  Points are WrappedPoints (the identity is (0, 0); a point is
 * absorbed as its two coordinates and is NOT checked to lie on the curve), scalars and base-field elements ark
 * Montgomery words.  absorb_g is also the reference's absorb_g_affine.  n = 0 is a no-op, HALO_OK.
 *
 * Host forms: copy in, run on the library's stream and wait.  A scalar (absorb_fr) that is not below the scalar
 * modulus, or a coordinate / element (absorb_g, absorb_fq) that is not below the base modulus, is HALO_EINVAL and
 * leaves the handle's state as it was.
 * _dev forms: device pointers, enqueued on `stream`, no host wait.  Their inputs are a precondition: a value that
 * breaks it is reduced by the Montgomery multiplication, a defined result that is not the reference's.  Calls on
 * one handle must be ordered by the caller (one stream, or events); halo_sponge_new has completed when it returns,
 * and halo_sponge_reset / halo_sponge_free first wait for the device.
 *
 * halo_sponge_reset: Sponge::reset (outer_sponge.rs:97-99): the zero state, nothing absorbed, NO label.
 * HALO_EINVAL, with the call's name in halo_last_error: protocol outside 0..3, k = 0, an id that was never made or
 * has been freed, a null pointer with n > 0, Poseidon parameters not set for the curve's base field
 * (halo_poseidon_set_params).  No GPU: HALO_EDEVICE. */
int halo_sponge_new(halo_curve_t curve, int protocol, size_t k, uint64_t* id);
int halo_sponge_free(uint64_t id);
int halo_sponge_reset(uint64_t id);
int halo_sponge_absorb_g(uint64_t id, const halo_wrapped_point_t* pts, size_t n);
int halo_sponge_absorb_fr(uint64_t id, const halo_fe_t* xs, size_t n);
int halo_sponge_absorb_fq(uint64_t id, const halo_fe_t* xs, size_t n);
int halo_sponge_challenge(uint64_t id, size_t n, halo_fe_t* out);
int halo_sponge_absorb_g_dev(uint64_t id, const void* d_pts, size_t n, void* stream);
int halo_sponge_absorb_fr_dev(uint64_t id, const void* d_xs, size_t n, void* stream);
int halo_sponge_absorb_fq_dev(uint64_t id, const void* d_xs, size_t n, void* stream);
int halo_sponge_challenge_dev(uint64_t id, size_t n, void* d_out, void* stream);

/* ------------------------------------------------------------------ the wire format (ABI 110)
 * The reference's proof objects travel as ark-serialize 0.5 compressed bytes, little endian, concatenation the only
 * framing (pcdl.rs:26,159, acc.rs:22; written by accumulation/src/main.rs:80-81):
 *   usize u64 | Vec<T> u64 length, items | Option<T> one byte 0 / 1, then the item if 1
 *   scalar  32 bytes, the canonical value (not Montgomery), below the modulus
 *   point   33 bytes: canonical x in bytes 0..31; byte 32: 0x80 y is the larger root (y > p - y), 0x40 infinity
 *           with x = 0, both set invalid, bits 0..5 zero
 *   Instance C, d, z, v, pi;  EvalProof (pi) Ls, Rs, U, c, C_bar: Option, w_prime: Option;  Accumulator = its Instance
 * A point record is REFUSED when x is not below the modulus, x^3 + 5 is not a square (x = 0 among them), a flag
 * bit is bad, or it is an infinity whose x is not 0 (only the canonical encoding is accepted; arkworks may be more
 * lenient there).  A refused record decodes to the off-curve sentinel (0, 1) with validity 0, so by the rule of
 * every batch verifier ("neither (0, 0) nor on the curve: that instance alone is rejected") it fails exactly the
 * instance that holds it.  Host forms run on the null stream and return when the outputs are written; _dev forms
 * take device pointers, are asynchronous on `stream` and wait for nothing.  k = 0: HALO_OK. */

/* Square roots in either Pasta field, one lane per element: out[i] the SMALLER root of in[i] as a canonical
 * integer (ark Montgomery limbs like every field element here) and is_square[i] = 1; zero and 0 for a
 * non-residue; sqrt(0) = 0 with flag 1.  is_square may be NULL. */
int halo_fe_sqrt_batch(halo_field_t field, const halo_fe_t* in, size_t k, halo_fe_t* out, uint8_t* is_square);
int halo_fe_sqrt_batch_dev(halo_field_t field, const void* d_in, size_t k, void* d_out, void* d_is_square, void* stream);
/* k consecutive 33-byte records -> WrappedPoints and validity bytes (ok may be NULL). */
int halo_points_decompress(halo_curve_t curve, const uint8_t* bytes, size_t k, halo_wrapped_point_t* out_pts, uint8_t* ok);
int halo_points_decompress_dev(halo_curve_t curve, const void* d_bytes, size_t k, void* d_out_pts, void* d_ok, void* stream);
/* The inverse; (0, 0) gives the infinity record.  A point that is neither (0, 0) nor on the curve has no encoding:
 * HALO_EINVAL naming it in the host form; in the _dev form d_ok[i] = 0 (d_ok may be NULL) and the record written
 * carries both flags, which no decoder accepts. */
int halo_points_compress(halo_curve_t curve, const halo_wrapped_point_t* pts, size_t k, uint8_t* out_bytes);
int halo_points_compress_dev(halo_curve_t curve, const void* d_pts, size_t k, void* d_out_bytes, void* d_ok, void* stream);
/* 32 canonical bytes <-> ark Montgomery limbs.  From bytes: ok[i] = 0 and a zero scalar where the value is not
 * below the modulus (ok may be NULL).  To bytes: the value is reduced first. */
int halo_scalars_from_bytes(halo_field_t field, const uint8_t* bytes, size_t k, halo_fe_t* out, uint8_t* ok);
int halo_scalars_from_bytes_dev(halo_field_t field, const void* d_bytes, size_t k, void* d_out, void* d_ok, void* stream);
int halo_scalars_to_bytes(halo_field_t field, const halo_fe_t* in, size_t k, uint8_t* out_bytes);
int halo_scalars_to_bytes_dev(halo_field_t field, const void* d_in, size_t k, void* d_out_bytes, void* stream);
/* The layout of a buffer of concatenated Instances, on the host alone (no device work, no GPU needed): with
 * vec_prefix a Vec<Instance> (u64 count first, no byte after the last instance), else instances up to the last
 * byte.  Reads only lengths, d and option tags.  offsets holds max_k + 1 entries: offsets[i] the first byte of
 * instance i, offsets[i + 1] its end (instances are contiguous), so offsets[*k_out] is where the walk ended;
 * ds[i], hiding[i] its degree bound and option tag.  Refused before anything is written, with a message of its own
 * naming the instance: a buffer that ends inside an instance; a length prefix whose items the remaining bytes
 * could not hold; Ls / Rs lengths that differ from each other or from lg(d + 1); d + 1 not a power of two
 * (HALO_ENOTPOW2; the others HALO_EINVAL); a tag other than 0 / 1; one of C_bar / w_prime without the other;
 * more than max_k instances; bytes after the last instance of a Vec. */
int halo_pcdl_instances_walk(const uint8_t* bytes, size_t len, int vec_prefix, size_t max_k, uint64_t* offsets,
                             uint64_t* ds, uint8_t* hiding, size_t* k_out);
/* k instances of ONE degree bound d at offsets[0..k) of bytes[0, len) -> the argument arrays of
 * halo_pcdl_check_fs_batch, in its order (Ls / Rs: k lg n rows; hiding, C_bar, w_prime always written: zero rows
 * where the flag is 0).  The structure of every instance is checked first, on the host, with the refusals of
 * halo_pcdl_instances_walk; an instance of another d is HALO_EINVAL.  ok[i] = 0 if any point or scalar of instance i
 * does not decode: ALL its points are then the sentinel and all its scalars zero, so the verifier that follows
 * rejects that instance alone and meets no scalar it would answer HALO_EINVAL for. */
int halo_pcdl_instances_decode(halo_curve_t curve, size_t d, size_t k, const uint8_t* bytes, size_t len,
        const uint64_t* offsets, halo_wrapped_point_t* C, halo_fe_t* z, halo_fe_t* v, halo_wrapped_point_t* Ls,
        halo_wrapped_point_t* Rs, halo_wrapped_point_t* U, halo_fe_t* c, uint8_t* hiding, halo_wrapped_point_t* C_bar,
        halo_fe_t* w_prime, uint8_t* ok);
/* The same over device pointers.  Nothing is checked on the host: the device checks again that every instance lies
 * inside [0, len), that its d is the call's, that Ls and Rs hold lg n points and that the tags are 0 / 1 and equal,
 * reading nothing at or past len; a mismatch is a failed decode (ok 0, sentinels, zeros, hiding 0), so
 * halo_pcdl_check_fs_batch_dev can consume the arrays on the same stream without a trip home. */
int halo_pcdl_instances_decode_dev(halo_curve_t curve, size_t d, size_t k, const void* d_bytes, size_t len,
        const void* d_offsets, void* d_C, void* d_z, void* d_v, void* d_Ls, void* d_Rs, void* d_U, void* d_c, void* d_hiding,
        void* d_C_bar, void* d_w_prime, void* d_ok, void* stream);
/* The inverse of halo_pcdl_instances_decode: the k instances, concatenated, with no Vec prefix.  hiding NULL: none
 * hides.  *out_len: in, the capacity of out_bytes; out, the length.  Size query: out_bytes NULL returns the length
 * alone.  HALO_EINVAL naming the instance for a point that is neither (0, 0) nor on the curve. */
int halo_pcdl_instances_encode(halo_curve_t curve, size_t d, size_t k, const halo_wrapped_point_t* C,
        const halo_fe_t* z, const halo_fe_t* v, const halo_wrapped_point_t* Ls, const halo_wrapped_point_t* Rs,
        const halo_wrapped_point_t* U, const halo_fe_t* c, const uint8_t* hiding, const halo_wrapped_point_t* C_bar,
        const halo_fe_t* w_prime, uint8_t* out_bytes, size_t* out_len);

/* ------------------------------------------------------------------ measurement hooks
 * When enabled, the library brackets its dominant kernels (MSM bucket accumulation, NTT passes)
 * with hipEvents on the stream they run on; halo_profile_read returns the number of launches and
 * the summed kernel time in ms for a kernel name ("msm_acc", "ntt_pass") since the last reset.
 * One name counts no launches: under "sponge_permutations" `launches` is the number of Poseidon
 * permutations the sponge handles ran (k per permutation of a handle of k), from the host's plan. */
int halo_profile_enable(int on);
int halo_profile_read(const char* name, size_t* launches, double* total_ms);
int halo_profile_reset(void);

/* ------------------------------------------------------------------ field self-test helpers
 * Elementwise device field ops over host arrays (used by the parity tests of a1):
 * op 0 = mul, 1 = add, 2 = sub, 3 = sqr(a), 4 = inverse(a) (0 -> 0), 5 = neg(a). */
int halo_field_op(halo_field_t field, int op, const halo_fe_t* a, const halo_fe_t* b, size_t n,
                  halo_fe_t* out);
/* Elementwise device curve ops over host arrays (parity tests of a2):
 * op 0 = a + b, 1 = 2a, 2 = k * a (k = scalars, Montgomery). */
int halo_curve_op(halo_curve_t curve, int op, const halo_wrapped_point_t* a,
                  const halo_wrapped_point_t* b, const halo_fe_t* k, size_t n,
                  halo_wrapped_point_t* out);

#ifdef __cplusplus
}
#endif
#endif /* HALO_GPU_H */
