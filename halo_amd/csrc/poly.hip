// Field-only reductions and polynomial helpers: polynomial evaluation, dot products, powers, FFT
// multiplication, the h-polynomial and the trace commitments.  Nothing
// here touches an IPA session; the sessions call dot_device / powers_device (poly.hpp).
//
//  * DensePolynomial::evaluate (Horner, pcdl.rs:49,471): chunked Horner + z^offset + tree sum.
//  * group::scalar_dot / construct_powers (crates/group/src/group.rs:43-45,58-66).
//  * &Poly * &Poly (protocol.rs:132-139, pcdl.rs:215): NTT, pointwise product, iNTT, trim.
#include <algorithm>
#include <cstring>
#include <vector>

#include "dispatch.hpp"
#include "msm.hpp"
#include "ntt.hpp"
#include "points.hpp"
#include "poly.hpp"
#include "runtime.hpp"

namespace halo {

// ---------------------------------------------------------------------------------------------
// reductions / elementwise
// ---------------------------------------------------------------------------------------------
constexpr int RED_THREADS = 256;

// partial[blockIdx] = sum_{i in block range} x[i] * y[i].  x is read raw (ark value X = x 2^256) and
// y converted to internal (y R'), so fe_mul(X, Y) = x y 2^256: every partial is the product already
// in ark form and the final sum only needs canonicalising.
template <class F>
__global__ __launch_bounds__(RED_THREADS) void k_dot_partial(const uint4* x, const uint4* y, size_t n, size_t per_block,
                                                             uint4* partial) {
    __shared__ uint4 red[RED_THREADS * 2];
    const size_t beg = (size_t)blockIdx.x * per_block, end = min(n, beg + per_block);
    Fe<F> acc = fe_zero<F>();
    for (size_t i = beg + threadIdx.x; i < end; i += RED_THREADS)
        acc = fe_add(acc, fe_mul(fe_load<F>(x + 2 * i), fe_from_ark<F>(y + 2 * i)));
    fe_store(red + 2 * threadIdx.x, acc);
    __syncthreads();
    for (int off = RED_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            fe_store(red + 2 * threadIdx.x, fe_add(fe_load<F>(red + 2 * threadIdx.x), fe_load<F>(red + 2 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) fe_store(partial + 2 * blockIdx.x, fe_load<F>(red));
}

// out_ark = ARK(sum_b partial[b]) where partial values are "ark-valued products" (see above)
template <class F>
__global__ __launch_bounds__(RED_THREADS) void k_sum_partials_to_ark(const uint4* partial, size_t nb, uint4* out_ark) {
    __shared__ uint4 red[RED_THREADS * 2];
    Fe<F> acc = fe_zero<F>();
    for (size_t i = threadIdx.x; i < nb; i += RED_THREADS) acc = fe_add(acc, fe_load<F>(partial + 2 * i));
    fe_store(red + 2 * threadIdx.x, acc);
    __syncthreads();
    for (int off = RED_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            fe_store(red + 2 * threadIdx.x, fe_add(fe_load<F>(red + 2 * threadIdx.x), fe_load<F>(red + 2 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // acc holds sum of ark-form values (x y 2^256 mod p, weakly reduced): canonicalize
        fe_store(out_ark, fe_canon(fe_reduce_2p(fe_load<F>(red))));
    }
}

// out[i] = z^i, i < n (ark in / out); each thread produces a run of `run` consecutive powers
template <class F>
__global__ void k_powers(const uint4* z_ark, size_t n, size_t run, uint4* out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t beg = t * run;
    if (beg >= n) return;
    const Fe<F> z = fe_from_ark<F>(z_ark);
    Fe<F> p = fe_one<F>(), b = z;
    for (size_t e = beg; e; e >>= 1) {
        if (e & 1) p = fe_mul(p, b);
        b = fe_sqr(b);
    }
    const size_t end = min(n, beg + run);
    for (size_t i = beg; i < end; i++) {
        fe_to_ark(out + 2 * i, p);
        p = fe_mul(p, z);
    }
}

// Chunked Horner: partial[(poly, chunk)] = z^start * sum_{i in chunk} c_i z^(i - start)  (internal)
template <class F>
__global__ __launch_bounds__(RED_THREADS) void k_eval_chunks(const uint4* const* polys, const size_t* lens,
                                                             const uint4* z_ark, size_t chunk, int nchunks,
                                                             uint4* partial) {
    __shared__ uint4 red[RED_THREADS * 2];
    const int pi = blockIdx.y;
    const size_t len = lens[pi];
    const uint4* c = polys[pi];
    const Fe<F> z = fe_from_ark<F>(z_ark);
    const size_t per_block = chunk * RED_THREADS;
    const size_t tbeg = (size_t)blockIdx.x * per_block + (size_t)threadIdx.x * chunk;
    Fe<F> acc = fe_zero<F>();
    if (tbeg < len) {
        const size_t tend = min(len, tbeg + chunk);
        for (size_t i = tend; i-- > tbeg;) acc = fe_add(fe_mul(acc, z), fe_from_ark<F>(c + 2 * i));
        Fe<F> p = fe_one<F>(), b = z;
        for (size_t e = tbeg; e; e >>= 1) {
            if (e & 1) p = fe_mul(p, b);
            b = fe_sqr(b);
        }
        acc = fe_mul(acc, p);
    }
    fe_store(red + 2 * threadIdx.x, acc);
    __syncthreads();
    for (int off = RED_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            fe_store(red + 2 * threadIdx.x, fe_add(fe_load<F>(red + 2 * threadIdx.x), fe_load<F>(red + 2 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) fe_store(partial + 2 * ((size_t)pi * nchunks + blockIdx.x), fe_load<F>(red));
}

template <class F>
__global__ __launch_bounds__(RED_THREADS) void k_sum_internal_to_ark(const uint4* partial, int per, uint4* out_ark) {
    __shared__ uint4 red[RED_THREADS * 2];
    const int pi = blockIdx.x;
    Fe<F> acc = fe_zero<F>();
    for (int i = threadIdx.x; i < per; i += RED_THREADS) acc = fe_add(acc, fe_load<F>(partial + 2 * ((size_t)pi * per + i)));
    fe_store(red + 2 * threadIdx.x, acc);
    __syncthreads();
    for (int off = RED_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            fe_store(red + 2 * threadIdx.x, fe_add(fe_load<F>(red + 2 * threadIdx.x), fe_load<F>(red + 2 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) fe_to_ark(out_ark + 2 * pi, fe_load<F>(red));
}

// pointwise a[i] *= b[i] (ark in / out)
template <class F>
__global__ void k_pointwise_mul(uint4* a, const uint4* b, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe_to_ark(a + 2 * i, fe_mul(fe_from_ark<F>(a + 2 * i), fe_from_ark<F>(b + 2 * i)));
}

// ---------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------
// dot product of two device ark vectors -> device ark scalar (out_ark), using tmp (>= 2048*32 B)
int dot_device(int field, const void* x, const void* y, size_t n, void* out_ark, void* tmp, hipStream_t s) {
    const size_t per_block = std::max<size_t>(RED_THREADS * 8, (n + 1023) / 1024);
    const size_t nb = std::max<size_t>(1, (n + per_block - 1) / per_block);
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_dot_partial<F>, dim3((unsigned)nb), dim3(RED_THREADS), 0, s, (const uint4*)x,
                           (const uint4*)y, n, per_block, (uint4*)tmp);
        hipLaunchKernelGGL(k_sum_partials_to_ark<F>, dim3(1), dim3(RED_THREADS), 0, s, (const uint4*)tmp, nb,
                           (uint4*)out_ark);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// out[i] = z^i, i < n (device ark in / out), `run` consecutive powers per thread
static int powers_launch(int field, const void* z_ark, size_t n, size_t run, void* out, hipStream_t s) {
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_powers<F>, dim3(grid_for((n + run - 1) / run, 128)), dim3(128), 0, s, (const uint4*)z_ark, n, run,
                           (uint4*)out);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int powers_device(int field, const void* z_ark, size_t n, void* out, hipStream_t s) {
    // consecutive powers per thread: a thread's chain is its exponentiation (~log2 n + popcount
    // products) plus `run`; small n is latency-bound (short runs), large n throughput-bound
    return powers_launch(field, z_ark, n, n <= 4096 ? 2 : 16, out, s);
}

// halo_poly_eval_batch / _dev: coefficients per thread of k_eval_chunks, and the chunks (blocks) of the
// longest polynomial
constexpr size_t EVAL_CHUNK = 32;
static int eval_nchunks(size_t maxlen) {
    return (int)std::max<size_t>(1, (maxlen + EVAL_CHUNK * RED_THREADS - 1) / (EVAL_CHUNK * RED_THREADS));
}
// The chunked Horner evaluation of k polynomials at z, then one sum per polynomial to out_ark[k].
// meta (device): k coefficient pointers | k lengths | z; part (device): k * nchunks elements.
static int eval_batch_launch(int field, const char* meta, size_t k, int nchunks, char* part, void* out_ark, hipStream_t s) {
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_eval_chunks<F>, dim3(nchunks, (unsigned)k), dim3(RED_THREADS), 0, s,
                           (const uint4* const*)meta, (const size_t*)(meta + k * sizeof(void*)),
                           (const uint4*)(meta + k * (sizeof(void*) + sizeof(size_t))), EVAL_CHUNK, nchunks, (uint4*)part);
        hipLaunchKernelGGL(k_sum_internal_to_ark<F>, dim3((unsigned)k), dim3(RED_THREADS), 0, s, (const uint4*)part,
                           nchunks, (uint4*)out_ark);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_scalar_dot(halo_field_t field, const halo_fe_t* xs, const halo_fe_t* ys, size_t n, halo_fe_t* out) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!out || (n && (!xs || !ys))) return set_error(HALO_EINVAL, "halo_scalar_dot: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[1].reserve(std::max<size_t>(n, 1) * 32));
    HALO_CHECK(st->scratch[2].reserve(2048 * 32 + 64));
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, xs, n * 32, s));
    HALO_CHECK(copy_h2d(st->scratch[1].ptr, ys, n * 32, s));
    char* t = (char*)st->scratch[2].ptr;
    HALO_CHECK(dot_device(field, st->scratch[0].ptr, st->scratch[1].ptr, n, t + 2048 * 32, t, s));
    return copy_d2h(out, t + 2048 * 32, 32, s);
}

extern "C" int halo_construct_powers(halo_field_t field, const halo_fe_t* z, size_t n, halo_fe_t* out) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!z || (n && !out)) return set_error(HALO_EINVAL, "halo_construct_powers: null buffer");
    if (!n) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(n * 32 + 32));
    char* b = (char*)st->scratch[0].ptr;
    HALO_CHECK(copy_h2d(b, z, 32, s));
    HALO_CHECK(powers_launch(field, b, n, 16, b + 32, s));
    return copy_d2h(out, b + 32, n * 32, s);
}

extern "C" int halo_poly_eval_batch(halo_field_t field, const halo_fe_t* const* polys, const size_t* lens, size_t k,
                                    const halo_fe_t* z, halo_fe_t* out) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!z || (k && (!polys || !lens || !out))) return set_error(HALO_EINVAL, "halo_poly_eval_batch: null buffer");
    if (!k) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    size_t total = 0, maxlen = 0;
    for (size_t i = 0; i < k; i++) {
        if (lens[i] && !polys[i]) return set_error(HALO_EINVAL, "halo_poly_eval_batch: null polynomial %zu", i);
        total += lens[i];
        maxlen = std::max(maxlen, lens[i]);
    }
    const int nchunks = eval_nchunks(maxlen);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(total, 1) * 32));
    HALO_CHECK(st->scratch[1].reserve(k * (sizeof(void*) + sizeof(size_t)) + 64));
    HALO_CHECK(st->scratch[2].reserve((size_t)k * nchunks * 32 + k * 32));
    std::vector<const void*> dptr(k);
    size_t off = 0;
    char* base = (char*)st->scratch[0].ptr;
    for (size_t i = 0; i < k; i++) {
        dptr[i] = base + off * 32;
        HALO_CHECK(copy_h2d(base + off * 32, polys[i], lens[i] * 32, s));
        off += lens[i];
    }
    char* meta = (char*)st->scratch[1].ptr;
    HALO_CHECK(copy_h2d(meta, dptr.data(), k * sizeof(void*), s));
    HALO_CHECK(copy_h2d(meta + k * sizeof(void*), lens, k * sizeof(size_t), s));
    HALO_CHECK(copy_h2d(meta + k * (sizeof(void*) + sizeof(size_t)), z, 32, s));
    char* part = (char*)st->scratch[2].ptr;
    HALO_CHECK(eval_batch_launch(field, meta, k, nchunks, part, part + (size_t)k * nchunks * 32, s));
    return copy_d2h(out, part + (size_t)k * nchunks * 32, k * 32, s);
}

// Device-resident variant (the prover's 78 evaluations at xi, protocol.rs:315-323): d_polys is a
// host array of k device pointers (ark coefficients), results (ark) to d_out[k].  Stream-ordered;
// the pointer table is staged through a per-device buffer, so calls on one stream may be queued back
// to back.
extern "C" int halo_poly_eval_batch_dev(halo_field_t field, const void* const* d_polys, const size_t* lens, size_t k,
                                        const halo_fe_t* z, void* d_out, void* stream) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (!z || (k && (!d_polys || !lens || !d_out))) return set_error(HALO_EINVAL, "halo_poly_eval_batch_dev: null buffer");
    if (!k) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    size_t maxlen = 0;
    for (size_t i = 0; i < k; i++) {
        if (lens[i] && !d_polys[i]) return set_error(HALO_EINVAL, "halo_poly_eval_batch_dev: null polynomial %zu", i);
        maxlen = std::max(maxlen, lens[i]);
    }
    const int nchunks = eval_nchunks(maxlen);
    const size_t meta_bytes = k * (sizeof(void*) + sizeof(size_t)) + 32;
    HALO_CHECK(st->eval_meta[0].reserve(meta_bytes));
    HALO_CHECK(st->eval_meta[1].reserve((size_t)k * nchunks * 32));
    std::vector<unsigned char> host(meta_bytes);
    memcpy(host.data(), d_polys, k * sizeof(void*));
    memcpy(host.data() + k * sizeof(void*), lens, k * sizeof(size_t));
    memcpy(host.data() + k * (sizeof(void*) + sizeof(size_t)), z, 32);
    char* meta = (char*)st->eval_meta[0].ptr;
    HALO_CHECK(copy_h2d(meta, host.data(), meta_bytes, s));
    char* part = (char*)st->eval_meta[1].ptr;
    return eval_batch_launch(field, meta, k, nchunks, part, d_out, s);
}

extern "C" int halo_poly_mul(halo_field_t field, const halo_fe_t* a, size_t la, const halo_fe_t* b, size_t lb,
                             halo_fe_t* out, size_t* out_len) {
    clear_error();
    HALO_CHECK(check_field(field));
    if ((la && !a) || (lb && !b) || !out_len) return set_error(HALO_EINVAL, "halo_poly_mul: null buffer");
    if (la == 0 || lb == 0) {
        *out_len = 0;  // the zero polynomial
        return HALO_OK;
    }
    if (!out) return set_error(HALO_EINVAL, "halo_poly_mul: null out");
    const size_t rl = la + lb - 1;
    unsigned logn = 0;
    while (((size_t)1 << logn) < rl) logn++;
    if (logn > 28) return set_error(HALO_EINVAL, "halo_poly_mul: product too large");
    const size_t N = (size_t)1 << logn;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    for (int i = 0; i < 5; i++) HALO_CHECK(st->scratch[i].reserve(N * 32));
    char* A = (char*)st->scratch[0].ptr;
    char* Bv = (char*)st->scratch[1].ptr;
    char* FA = (char*)st->scratch[2].ptr;
    char* FB = (char*)st->scratch[3].ptr;
    char* T = (char*)st->scratch[4].ptr;
    HALO_HIP(hipMemsetAsync(A, 0, N * 32, s));
    HALO_HIP(hipMemsetAsync(Bv, 0, N * 32, s));
    HALO_CHECK(copy_h2d(A, a, la * 32, s));
    HALO_CHECK(copy_h2d(Bv, b, lb * 32, s));
    HALO_CHECK(ntt_device_dispatch(st, field, A, FA, T, logn, 1, 0, s));
    HALO_CHECK(ntt_device_dispatch(st, field, Bv, FB, T, logn, 1, 0, s));
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_pointwise_mul<F>, dim3(grid_for(N, 256)), dim3(256), 0, s, (uint4*)FA, (const uint4*)FB, N);
    });
    HALO_HIP(hipGetLastError());
    HALO_CHECK(ntt_device_dispatch(st, field, FA, A, T, logn, 1, 1, s));
    std::vector<halo_fe_t> tmp(rl);
    HALO_CHECK(copy_d2h(tmp.data(), A, rl * 32, s));
    size_t n = rl;
    while (n > 0 && !(tmp[n - 1].l[0] | tmp[n - 1].l[1] | tmp[n - 1].l[2] | tmp[n - 1].l[3])) n--;
    std::copy(tmp.begin(), tmp.begin() + n, out);
    *out_len = n;
    return HALO_OK;
}

// ---------------------------------------------------------------------------------------------
// h(X) coefficients and the decider commitment.
//
// HPoly::get_poly (crates/accumulation/src/pcdl.rs:198-219) builds
//   h(X) = prod_{i < lg n} (1 + xi_{lg n - i} X^(2^i))
// with lg n growing FFT multiplications; its coefficient j is simply the product of
// xi_{lg n - b} over the set bits b of j (the identity pcdl.rs:735-758 tests).  Generated directly:
// j = hi * 2^LB + lo, coef[j] = T_lo[lo] * T_hi[hi] (two small tables, one multiplication per
// coefficient).  The ASDL combination sum_i alpha_i h_i(X) (acc.rs:89) folds alpha_i into T_hi,i.
// ---------------------------------------------------------------------------------------------
template <class F>
__global__ void k_hpoly_tables(const uint4* xis_ark, size_t k, uint32_t lg_n, uint32_t lb, const uint4* alphas_ark,
                               uint4* t_lo, uint4* t_hi) {
    const size_t nlo = (size_t)1 << lb, nhi = (size_t)1 << (lg_n - lb);
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= k * (nlo + nhi)) return;
    const size_t i = idx / (nlo + nhi), x = idx % (nlo + nhi);
    const uint4* xi = xis_ark + 2 * i * (lg_n + 1);
    Fe<F> v = fe_one<F>();
    if (x < nlo) {
        for (uint32_t b = 0; b < lb; b++)
            if ((x >> b) & 1) v = fe_mul(v, fe_from_ark<F>(xi + 2 * (lg_n - b)));
        fe_store(t_lo + 2 * (i * nlo + x), v);
    } else {
        const size_t y = x - nlo;
        if (alphas_ark) v = fe_from_ark<F>(alphas_ark + 2 * i);
        for (uint32_t b = 0; b < lg_n - lb; b++)
            if ((y >> b) & 1) v = fe_mul(v, fe_from_ark<F>(xi + 2 * (lg_n - lb - b)));
        fe_store(t_hi + 2 * (i * nhi + y), v);
    }
}

template <class F>
__global__ void k_hpoly_coeffs(const uint4* t_lo, const uint4* t_hi, size_t k, uint32_t lg_n, uint32_t lb,
                               uint4* out_ark) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >> lg_n) return;
    const size_t nlo = (size_t)1 << lb, nhi = (size_t)1 << (lg_n - lb);
    const size_t lo = j & (nlo - 1), hi = j >> lb;
    Fe<F> acc = fe_zero<F>();
    size_t i = 0;
    // two polynomials per step as one double product with one reduction (entries are < 2p: the sum is far below
    // fe_mul2's bound of ~127 p^2)
    for (; i + 1 < k; i += 2)
        acc = fe_add(acc, fe_mul2(fe_load<F>(t_lo + 2 * (i * nlo + lo)), fe_load<F>(t_hi + 2 * (i * nhi + hi)),
                                  fe_load<F>(t_lo + 2 * ((i + 1) * nlo + lo)), fe_load<F>(t_hi + 2 * ((i + 1) * nhi + hi))));
    if (i < k) acc = fe_add(acc, fe_mul(fe_load<F>(t_lo + 2 * (i * nlo + lo)), fe_load<F>(t_hi + 2 * (i * nhi + hi))));
    fe_to_ark(out_ark + 2 * j, acc);
}

// One coefficient row per polynomial instead of their sum: rows[i n + j] = coefficient j of h_i (ark, the form
// k_digits reads), one multiplication per coefficient from the same two half-tables (built without weights).
template <class F>
__global__ __launch_bounds__(256) void k_hpoly_rows(const uint4* __restrict__ t_lo, const uint4* __restrict__ t_hi, size_t g,
                                                    uint32_t lg_n, uint32_t lb, uint4* __restrict__ rows_ark) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((idx >> lg_n) >= g) return;
    const size_t nlo = (size_t)1 << lb, nhi = (size_t)1 << (lg_n - lb);
    const size_t i = idx >> lg_n, j = idx & (((size_t)1 << lg_n) - 1);
    const size_t lo = j & (nlo - 1), hi = j >> lb;
    fe_to_ark(rows_ark + 2 * idx, fe_mul(fe_load<F>(t_lo + 2 * (i * nlo + lo)), fe_load<F>(t_hi + 2 * (i * nhi + hi))));
}

// One coefficient row per segment of instances: rows[s n + j] = sum_{lo_s <= i < mid_s} T_lo,i[lo] T_hi,i[hi], the
// partial sums of k_hpoly_coeffs over the half-tables it read (weights folded into T_hi).  segs[s] = (lo_s, mid_s,
// ., .) with lo_s < mid_s; two instances per step as in k_hpoly_coeffs, a last odd one alone.
template <class F>
__global__ __launch_bounds__(256) void k_hpoly_segments(const uint4* __restrict__ t_lo, const uint4* __restrict__ t_hi,
                                                        const uint4* __restrict__ segs, size_t g, uint32_t lg_n, uint32_t lb,
                                                        uint4* __restrict__ rows_ark) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((idx >> lg_n) >= g) return;
    const size_t nlo = (size_t)1 << lb, nhi = (size_t)1 << (lg_n - lb);
    const size_t j = idx & (((size_t)1 << lg_n) - 1);
    const size_t lo = j & (nlo - 1), hi = j >> lb;
    const uint4 seg = segs[idx >> lg_n];
    const size_t end = seg.y;
    Fe<F> acc = fe_zero<F>();
    size_t i = seg.x;
    for (; i + 1 < end; i += 2)
        acc = fe_add(acc, fe_mul2(fe_load<F>(t_lo + 2 * (i * nlo + lo)), fe_load<F>(t_hi + 2 * (i * nhi + hi)),
                                  fe_load<F>(t_lo + 2 * ((i + 1) * nlo + lo)), fe_load<F>(t_hi + 2 * ((i + 1) * nhi + hi))));
    if (i < end) acc = fe_add(acc, fe_mul(fe_load<F>(t_lo + 2 * (i * nlo + lo)), fe_load<F>(t_hi + 2 * (i * nhi + hi))));
    fe_to_ark(rows_ark + 2 * idx, acc);
}

namespace halo {

size_t hpoly_table_elems(size_t k, uint32_t lg_n) {
    const uint32_t lb = lg_n / 2;
    return k * (((size_t)1 << lb) + ((size_t)1 << (lg_n - lb)));
}

static void hpoly_tables_launch(int field, const void* d_xis, size_t k, uint32_t lg_n, const void* d_alphas, uint4* t_lo,
                                uint4* t_hi, hipStream_t s) {
    const uint32_t lb = lg_n / 2;
    const size_t nlo = (size_t)1 << lb, nhi = (size_t)1 << (lg_n - lb);
    DISPATCH_FIELD(field, F, {
        hipLaunchKernelGGL(k_hpoly_tables<F>, dim3(grid_for(k * (nlo + nhi), 128)), dim3(128), 0, s, (const uint4*)d_xis, k,
                           lg_n, lb, (const uint4*)d_alphas, t_lo, t_hi);
    });
}

// sum_i alpha_i h_i coefficients (ark, 2^lg_n entries) at d_out from k xi rows (lg_n + 1 ark elements each) and
// k weights (or null) that are device pointers; d_tables: hpoly_table_elems(k, lg_n) elements.  On stream s.
int hpoly_combine_device(int field, const void* d_xis, size_t k, uint32_t lg_n, const void* d_alphas, void* d_tables,
                         void* d_out, hipStream_t s, const char* prof_name) {
    const uint32_t lb = lg_n / 2;
    uint4* t_lo = (uint4*)d_tables;
    uint4* t_hi = t_lo + 2 * k * ((size_t)1 << lb);
    hpoly_tables_launch(field, d_xis, k, lg_n, d_alphas, t_lo, t_hi, s);
    ProfScope prof(prof_name, s);
    DISPATCH_FIELD(field, F, {
        HALO_LAUNCH(prof, k_hpoly_coeffs<F>, dim3(grid_for((size_t)1 << lg_n, 256)), dim3(256), 0, s, (const uint4*)t_lo,
                    (const uint4*)t_hi, k, lg_n, lb, (uint4*)d_out);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The g coefficient rows of h_0 .. h_(g-1) (ark, g 2^lg_n entries) at d_rows; g 2^lg_n < 2^32.  On stream s.
int hpoly_rows_device(int field, const void* d_xis, size_t g, uint32_t lg_n, void* d_tables, void* d_rows, hipStream_t s) {
    const uint32_t lb = lg_n / 2;
    uint4* t_lo = (uint4*)d_tables;
    uint4* t_hi = t_lo + 2 * g * ((size_t)1 << lb);
    hpoly_tables_launch(field, d_xis, g, lg_n, nullptr, t_lo, t_hi, s);
    ProfScope prof("hpoly_rows", s);
    DISPATCH_FIELD(field, F, {
        HALO_LAUNCH(prof, k_hpoly_rows<F>, dim3(grid_for(g << lg_n, 256)), dim3(256), 0, s, (const uint4*)t_lo,
                    (const uint4*)t_hi, g, lg_n, lb, (uint4*)d_rows);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// g coefficient rows (ark, row s at d_rows + 32 s 2^lg_n) from the half-tables hpoly_combine_device left at d_tables
// for k instances: row s sums the instances [x, y) of d_segs[s] (uint4 each, x < y <= k); g 2^lg_n < 2^32.
int hpoly_segments_device(int field, const void* d_tables, size_t k, uint32_t lg_n, const void* d_segs, size_t g, void* d_rows,
                          hipStream_t s) {
    const uint32_t lb = lg_n / 2;
    const uint4* t_lo = (const uint4*)d_tables;
    const uint4* t_hi = t_lo + 2 * k * ((size_t)1 << lb);
    ProfScope prof("hpoly_segments", s);
    DISPATCH_FIELD(field, F, {
        HALO_LAUNCH(prof, k_hpoly_segments<F>, dim3(grid_for(g << lg_n, 256)), dim3(256), 0, s, t_lo, t_hi, (const uint4*)d_segs, g,
                    lg_n, lb, (uint4*)d_rows);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo

// k h-polynomials (xis: k rows of n_xis ark elements, host) -> sum_i alpha_i h_i coefficients (ark) at d_out
// (2^(n_xis - 1) entries), on stream s.  Uses scratch[6] for the xis/alphas and tables.
static int hpoly_device(DeviceState* st, int field, const halo_fe_t* xis, size_t k, size_t n_xis,
                        const halo_fe_t* alphas, void* d_out, hipStream_t s) {
    const uint32_t lg_n = (uint32_t)(n_xis - 1);
    const size_t in_elems = k * n_xis + (alphas ? k : 0);
    HALO_CHECK(st->scratch[6].reserve((in_elems + hpoly_table_elems(k, lg_n)) * 32));
    uint4* d_xis = st->scratch[6].as<uint4>();
    uint4* d_alpha = alphas ? d_xis + 2 * k * n_xis : nullptr;
    HALO_CHECK(copy_h2d(d_xis, xis, k * n_xis * 32, s));
    if (alphas) HALO_CHECK(copy_h2d(d_alpha, alphas, k * 32, s));
    return hpoly_combine_device(field, d_xis, k, lg_n, d_alpha, d_xis + 2 * in_elems, d_out, s, nullptr);
}

extern "C" int halo_hpoly_combine(halo_field_t field, const halo_fe_t* xis, size_t k, size_t n_xis,
                                  const halo_fe_t* alphas, halo_fe_t* out, size_t* out_len) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (n_xis < 1 || n_xis > 29) return set_error(HALO_EINVAL, "halo_hpoly: n_xis %zu out of range [1, 29]", n_xis);
    if (!k || !xis || !out) return set_error(HALO_EINVAL, "halo_hpoly: null buffer or k = 0");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t n = (size_t)1 << (n_xis - 1);
    HALO_CHECK(st->scratch[7].reserve(n * 32));
    HALO_CHECK(hpoly_device(st, field, xis, k, n_xis, alphas, st->scratch[7].ptr, s));
    HALO_CHECK(copy_d2h(out, st->scratch[7].ptr, n * 32, s));
    if (out_len) {  // DensePolynomial trims trailing zeros
        size_t m = n;
        while (m > 0 && !(out[m - 1].l[0] | out[m - 1].l[1] | out[m - 1].l[2] | out[m - 1].l[3])) m--;
        *out_len = m;
    }
    return HALO_OK;
}

// Device-resident variant (acc::prover's h(X), acc.rs:89 / pcdl.rs:198-219): the 2^(n_xis - 1)
// coefficients (ark, untrimmed) go to d_out on `stream`; h never crosses PCIe.
extern "C" int halo_hpoly_combine_dev(halo_field_t field, const halo_fe_t* xis, size_t k, size_t n_xis,
                                      const halo_fe_t* alphas, void* d_out, void* stream) {
    clear_error();
    HALO_CHECK(check_field(field));
    if (n_xis < 1 || n_xis > 29) return set_error(HALO_EINVAL, "halo_hpoly: n_xis %zu out of range [1, 29]", n_xis);
    if (!k || !xis || !d_out) return set_error(HALO_EINVAL, "halo_hpoly: null buffer or k = 0");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = (hipStream_t)stream;
    ScratchUse su(st, s);
    return hpoly_device(st, field, xis, k, n_xis, alphas, d_out, s);
}

extern "C" int halo_hpoly_coeffs(halo_field_t field, const halo_fe_t* xis, size_t n_xis, halo_fe_t* out) {
    return halo_hpoly_combine(field, xis, 1, n_xis, nullptr, out, nullptr);
}

// pcdl::check step 5 (pcdl.rs:579): U' = pedersen::commit(None, &pp.Gs[0..d+1], &h.get_poly().coeffs),
// computed without leaving the device (h coefficients -> resident-SRS MSM).
extern "C" int halo_pcdl_decider_commit(halo_curve_t curve, const halo_fe_t* xis, size_t n_xis, size_t d,
                                        halo_wrapped_point_t* out) {
    clear_error();
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "unknown curve id %d", (int)curve);
    if (n_xis < 1 || n_xis > 29) return set_error(HALO_EINVAL, "halo_pcdl_decider_commit: n_xis %zu out of range", n_xis);
    if (!xis || !out) return set_error(HALO_EINVAL, "halo_pcdl_decider_commit: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    const size_t n = (size_t)1 << (n_xis - 1);
    if (d + 1 > srs.n)
        return set_error(HALO_ESRSRANGE, "range end index %zu out of range for slice of length %zu", d + 1, srs.n);
    // all coefficients are products of nonzero challenges: no trailing zeros, ms.len() = n
    if (d + 1 < n)
        return set_error(HALO_ELENGTH, "ms must be larger than Gs: (Gs: %zu), (ms: %zu)", d + 1, n);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[7].reserve(n * 32 + 128));
    const int field = (curve == HALO_PALLAS) ? HALO_FP : HALO_FQ;
    HALO_CHECK(hpoly_device(st, field, xis, 1, n_xis, nullptr, st->scratch[7].ptr, s));
    char* d_out = (char*)st->scratch[7].ptr + n * 32;
    HALO_CHECK(msm_srs_device(st, curve, st->scratch[7].ptr, n, nullptr, d_out, s, MsmOpts::Sync().xyzz()));
    alignas(16) uint64_t xyzz[16];  // converted on the host (points.hip d2h_point)
    HALO_CHECK(copy_d2h(xyzz, d_out, 128, s));
    host_xyzz_to_wrapped(curve, xyzz, out);
    return HALO_OK;
}

// ---------------------------------------------------------------------------------------------
// Trace::new's interpolate + commit batch (crates/plonk/src/circuit/trace.rs
// :165-192): k evaluation vectors on the 2^log_n domain -> Evals::from_vec_and_domain (rotate right
// by one, poly.rs:21-31) -> interpolate_by_ref (iNTT, trailing zeros trimmed) -> pcdl::commit(poly,
// d, None).  One batched iNTT, then k resident-SRS MSMs enqueued back to back (pipelined: each
// MSM's reduction tail overlaps the next one's accumulation), one host sync at the end.
// ---------------------------------------------------------------------------------------------
__global__ void k_rotate_right(const uint4* in, uint4* out, size_t k, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k * n) return;
    const size_t r = i / n, j = i % n;
    const size_t from = r * n + (j == 0 ? n - 1 : j - 1);
    out[2 * i] = in[2 * from];
    out[2 * i + 1] = in[2 * from + 1];
}

// lens[r] = 1 + index of the last nonzero element of row r (0 if all zero); one block per row
__global__ __launch_bounds__(256) void k_row_lengths(const uint4* a, size_t n, uint32_t* lens) {
    __shared__ uint32_t best;
    if (threadIdx.x == 0) best = 0;
    __syncthreads();
    const uint4* row = a + 2 * (size_t)blockIdx.x * n;
    uint32_t m = 0;
    for (size_t j = threadIdx.x; j < n; j += 256) {
        const uint4 x = row[2 * j], y = row[2 * j + 1];
        if (x.x | x.y | x.z | x.w | y.x | y.y | y.z | y.w) m = (uint32_t)j + 1;
    }
    if (m) atomicMax(&best, m);
    __syncthreads();
    if (threadIdx.x == 0) lens[blockIdx.x] = best;
}

extern "C" int halo_trace_commit_batch(halo_curve_t curve, const halo_fe_t* evals, size_t k, unsigned log_n, size_t d,
                                       halo_fe_t* coeffs_out, size_t* lens_out, halo_wrapped_point_t* commits_out) {
    clear_error();
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "unknown curve id %d", (int)curve);
    if (!k) return HALO_OK;
    if (!evals || !commits_out) return set_error(HALO_EINVAL, "halo_trace_commit_batch: null buffer");
    if (log_n > 28) return set_error(HALO_EINVAL, "log_n %u too large", log_n);
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (!srs.n) return set_error(HALO_ESRSRANGE, "no resident SRS: call halo_srs_upload first");
    const size_t n = (size_t)1 << log_n, D = srs.n - 1, nc = d + 1;
    if (!is_pow2(nc)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", nc);
    if (d > D) return set_error(HALO_ESRSRANGE, "d (%zu) <= D (%zu) (pp_len = %zu)", d, D, D + 1);
    const int field = (curve == HALO_PALLAS) ? HALO_FP : HALO_FQ;
    hipStream_t s = 0;
    ScratchUse su(st, s);
    const size_t bytes = k * n * 32;
    HALO_CHECK(st->scratch[0].reserve(bytes));
    HALO_CHECK(st->scratch[1].reserve(bytes));
    HALO_CHECK(st->scratch[2].reserve(bytes));
    HALO_CHECK(st->scratch[3].reserve(bytes));
    HALO_CHECK(st->scratch[7].reserve(k * (64 + 4)));
    uint4* A = st->scratch[0].as<uint4>();
    uint4* B = st->scratch[1].as<uint4>();
    HALO_CHECK(copy_h2d(A, evals, bytes, s));
    hipLaunchKernelGGL(k_rotate_right, dim3(grid_for(k * n, 256)), dim3(256), 0, s, (const uint4*)A, B, k, n);
    HALO_HIP(hipGetLastError());
    // batched in-place iNTT of the k rows of B (ping-pong through scratch 2 and 3)
    HALO_CHECK(ntt_device_dispatch(st, field, B, B, st->scratch[2].ptr, log_n, k, 1, s, st->scratch[3].ptr));
    uint32_t* d_lens = (uint32_t*)((char*)st->scratch[7].ptr + k * 64);
    hipLaunchKernelGGL(k_row_lengths, dim3((unsigned)k), dim3(256), 0, s, (const uint4*)B, n, d_lens);
    HALO_HIP(hipGetLastError());
    std::vector<uint32_t> lens(k);
    HALO_CHECK(copy_d2h(lens.data(), d_lens, k * 4, s));
    for (size_t r = 0; r < k; r++) {
        const size_t p_deg = lens[r] ? lens[r] - 1 : 0;
        if (p_deg > d) return set_error(HALO_EDEGREE, "p_deg (%zu) <= d (%zu)", p_deg, d);
    }
    uint4* d_commits = st->scratch[7].as<uint4>();
    std::vector<const void*> ptrs(k);
    std::vector<size_t> szs(k);
    for (size_t r = 0; r < k; r++) {
        ptrs[r] = B + 2 * r * n;
        szs[r] = lens[r];
    }
    HALO_CHECK(msm_batch_device(st, curve, ptrs.data(), szs.data(), k, d_commits, s));
    HALO_CHECK(msm_join(st, s));
    HALO_CHECK(copy_d2h(commits_out, d_commits, k * 64, s));
    if (coeffs_out) HALO_CHECK(copy_d2h(coeffs_out, B, bytes, s));
    if (lens_out)
        for (size_t r = 0; r < k; r++) lens_out[r] = lens[r];
    return HALO_OK;
}
