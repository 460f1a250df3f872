// IPA inner-product folding: the sessions of pcdl::open's round loop.
//
//  * IPA session: the round loop of pcdl::open_without_eval (crates/accumulation/src/pcdl.rs:404-438)
//    with G, c, z device-resident across rounds.  Per round the host (which owns the Poseidon
//    transcript, pcdl.rs:421-425) asks for L, R and then supplies xi.
//      L = <c_r, G_l> + H' <c_r, z_l>,  R = <c_l, G_r> + H' <c_l, z_r>     (pcdl.rs:412-418)
//      G_l[j] = (G_l[j] + xi G_r[j]).into_affine(); c_l[j] += xi^-1 c_r[j]; z_l[j] += xi z_r[j]
//                                                                       (pcdl.rs:427-435)
//    The G fold multiplies every lane by the SAME scalar xi, so all lanes follow one control path
//    (the NAF of xi, computed once per workgroup into LDS and read wave-uniformly); the dot products
//    are device reductions whose results feed the MSM's hiding-term slot (k_final) directly, so a
//    round never round-trips scalars through the host.
//  * Here: the fold and weighted-round kernels, the session pool and the session entry points.  The
//    session's declarations are in ipa_session.hpp, the choice of every round's and fold's path in ipa_plan.hpp
//    (host-only: this file performs its records), the tail rounds' multiples-table sums in tail.hip,
//    the dot products and powers in poly.hip, the hiding open's steps in pcdl_open.hip, the opening with its
//    transcript on the device in pcdl_open_fs.hip.
#include <algorithm>
#include <cstring>
#include <unordered_set>
#include <vector>

#include <chrono>
#include <thread>

#include "dispatch.hpp"
#include "glv.hpp"
#include "ipa_session.hpp"
#include "msm.hpp"
#include "points.hpp"
#include "poly.hpp"
#include "runtime.hpp"
#include "tail.hpp"
#include "tree.hpp"

namespace halo {

// ---------------------------------------------------------------------------------------------
// IPA fold
// ---------------------------------------------------------------------------------------------

// G'[j] = G_l[j] + xi G_r[j] for j < m, c'[j] = c_l + xi^-1 c_r, z'[j] = z_l + xi z_r.
// gs: internal affine (2m points), cs/zs: ark scalars (2m).  xi / xi_inv: ark.
// xi G_r = k1 G_r + k2 phi(G_r), phi(x, y) = (beta x, y) (GLV): one interleaved NAF double-and-add
// of ~128 doublings (digit schedule wave-uniform, in LDS) instead of 255.  The affine conversion
// shares one inversion per workgroup (Montgomery's trick over prefix / suffix product scans).
constexpr int FOLD_THREADS = 128;
template <class Cv>
__global__ __launch_bounds__(FOLD_THREADS, 4) void k_ipa_fold(uint4* gs, uint4* cs, uint4* zs, size_t m,
                                                           const uint4* xi_ark, const uint4* xi_inv_ark) {
    using F = typename Cv::Base;
    using S = typename Cv::Scalar;
    constexpr int ND = 132;
    __shared__ int8_t naf1[ND], naf2[ND];
    __shared__ int top_s, neg1_s, neg2_s;
    __shared__ uint32_t pre[FOLD_THREADS][NLIMB], suf[FOLD_THREADS][NLIMB];
    __shared__ uint32_t tinv[NLIMB];
    const int tid = threadIdx.x;
    if (tid == 0) {
        uint32_t w8[8];
        fe_ark_to_canonical_words<S>(xi_ark, w8);
        bool n1, n2;
        uint32_t k1[5], k2[5];
        glv::decompose<typename Cv::K>(w8, n1, k1, n2, k2);
        const int t1 = glv::naf_digits(k1, naf1, ND), t2 = glv::naf_digits(k2, naf2, ND);
        top_s = t1 > t2 ? t1 : t2;
        neg1_s = n1;
        neg2_s = n2;
    }
    __syncthreads();
    const int top = top_s;
    const size_t j = (size_t)blockIdx.x * FOLD_THREADS + tid;
    const bool live = j < m;
    XYZZ<F> acc = xyzz_id<F>();
    if (live) {
        const Fe<S> xi = fe_from_ark<S>(xi_ark);
        const Fe<S> xinv = fe_from_ark<S>(xi_inv_ark);
        fe_to_ark(cs + 2 * j, fe_add(fe_from_ark<S>(cs + 2 * j), fe_mul(fe_from_ark<S>(cs + 2 * (j + m)), xinv)));
        fe_to_ark(zs + 2 * j, fe_add(fe_from_ark<S>(zs + 2 * j), fe_mul(fe_from_ark<S>(zs + 2 * (j + m)), xi)));
        const Affine<F> gr = aff_load<F>(gs + 4 * (j + m));
        Affine<F> p1 = gr, p2;
        p2.x = fe_mul(gr.x, fe_from_const<F>(Cv::K::BETA));
        p2.y = gr.y;
        if (aff_is_id(gr)) p2 = gr;
        const int s1 = neg1_s ? -1 : 1, s2 = neg2_s ? -1 : 1;
        for (int i = top; i >= 0; i--) {
            acc = xyzz_dbl(acc);
            const int d1 = __builtin_amdgcn_readfirstlane((int)naf1[i] * s1);
            const int d2 = __builtin_amdgcn_readfirstlane((int)naf2[i] * s2);
            if (d1) {
                Affine<F> q = p1;
                if (d1 < 0) q.y = fe_neg(q.y);
                acc = xyzz_madd(acc, q);
            }
            if (d2) {
                Affine<F> q = p2;
                if (d2 < 0) q.y = fe_neg(q.y);
                acc = xyzz_madd(acc, q);
            }
        }
        acc = xyzz_madd(acc, aff_load<F>(gs + 4 * j));
    }
    // batched affine conversion: z = ZZ * ZZZ (1 for identity / idle lanes)
    // (measured and rejected: a Jacobian accumulator (dbl-2009-l + madd-2007-bl, ~27 % fewer
    // multiplications) was 13 % slower -- its fully reduced additions cost more than they save)
    const bool id = xyzz_is_id(acc);
    const Fe<F> z = (live && !id) ? fe_mul(acc.ZZ, acc.ZZZ) : fe_one<F>();
    // inclusive prefix and suffix products (Hillis-Steele in LDS)
    Fe<F> pv = z, sv = z;
    for (int off = 1; off < FOLD_THREADS; off <<= 1) {
        for (int l = 0; l < NLIMB; l++) {
            pre[tid][l] = pv.v[l];
            suf[tid][l] = sv.v[l];
        }
        __syncthreads();
        if (tid >= off) {
            Fe<F> o;
            for (int l = 0; l < NLIMB; l++) o.v[l] = pre[tid - off][l];
            pv = fe_mul(pv, o);
        }
        if (tid + off < FOLD_THREADS) {
            Fe<F> o;
            for (int l = 0; l < NLIMB; l++) o.v[l] = suf[tid + off][l];
            sv = fe_mul(sv, o);
        }
        __syncthreads();
    }
    for (int l = 0; l < NLIMB; l++) {
        pre[tid][l] = pv.v[l];
        suf[tid][l] = sv.v[l];
    }
    __syncthreads();
    if (tid == FOLD_THREADS - 1) {
        const Fe<F> t = fe_inv(pv);  // inverse of the product of all z
        for (int l = 0; l < NLIMB; l++) tinv[l] = t.v[l];
    }
    __syncthreads();
    if (!live) return;
    Fe<F> inv;
    for (int l = 0; l < NLIMB; l++) inv.v[l] = tinv[l];
    if (tid > 0) {
        Fe<F> o;
        for (int l = 0; l < NLIMB; l++) o.v[l] = pre[tid - 1][l];
        inv = fe_mul(inv, o);
    }
    if (tid + 1 < FOLD_THREADS) {
        Fe<F> o;
        for (int l = 0; l < NLIMB; l++) o.v[l] = suf[tid + 1][l];
        inv = fe_mul(inv, o);
    }
    Affine<F> r;
    if (id) {
        r.x = fe_zero<F>();
        r.y = fe_zero<F>();
    } else {
        r.x = fe_mul(acc.X, fe_mul(inv, acc.ZZZ));  // X / ZZ
        r.y = fe_mul(acc.Y, fe_mul(inv, acc.ZZ));   // Y / ZZZ
    }
    aff_store(gs + 4 * j, r);
}

// 2^i P (i < count) as XYZZ from a WrappedPoint: one doubling chain (one thread)
template <class Cv>
__global__ __launch_bounds__(64) void k_pow2_xyzz_from_wrapped(const uint4* P_wrapped, uint4* out_xyzz, int count) {
    using F = typename Cv::Base;
    // quad-cooperative XYZZ doublings on lanes 0-3 (xyzz_dbl_quad: three product rounds, 4.0 k cycles
    // against 6.3 k for the Jacobian jac_dbl_quad with its longer add / double tail, tools/micro/tree_parts.hip)
    if (threadIdx.x >= 4) return;
    XYZZ<F> q = xyzz_from_aff(aff_from_wrapped<F>(P_wrapped));
    for (int i = 0; i < count; i++) {
        if (threadIdx.x == 0) xyzz_store(out_xyzz + 8 * i, q);
        q = xyzz_dbl_quad(q);
    }
}

template <class Cv>
__global__ void k_copy_first_wrapped(const uint4* gs_int, const uint4* cs, uint4* out_U, uint4* out_c) {
    using F = typename Cv::Base;
    if (threadIdx.x != 0) return;
    aff_to_wrapped(out_U, aff_load<F>(gs_int));
    out_c[0] = cs[0];
    out_c[1] = cs[1];
}

// rounds of length <= IPA_TAIL_N run as tail rounds over a multiples table (tail.hip)
constexpr size_t IPA_TAIL_N = 2048;
constexpr int IPA_HTAB = 128;  // entries 2^i H' of the session's hiding table (GLV split of the scalar)

template <class S>
__global__ void k_set_one_ark(uint4* out) {
    if (threadIdx.x == 0) fe_to_ark(out, fe_one<S>());
}

// x[i] *= k (ark scalars, i < count): the IPA's dots scaled by xi_0 in xi mode
template <class S>
__global__ void k_scale_ark(uint4* x, int count, const uint4* k) {
    const int i = threadIdx.x;
    if (i < count) fe_to_ark(x + 2 * i, fe_mul(fe_from_ark<S>(x + 2 * i), fe_from_ark<S>(k)));
}

// c / z folds (pcdl.rs:430-435) and the weight update w' = interleave(w, xi w)
template <class Cv>
__global__ __launch_bounds__(256) void k_tail_fold(uint4* cs, uint4* zs, size_t m, ArkScalarPair x,
                                                   const uint4* w_in, uint4* w_out, size_t wlen) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fe<S> xi = fe_from_ark<S>(x.v);
    if (i < m) {
        const Fe<S> xinv = fe_from_ark<S>(x.v + 2);
        fe_to_ark(cs + 2 * i, fe_add(fe_from_ark<S>(cs + 2 * i), fe_mul(fe_from_ark<S>(cs + 2 * (i + m)), xinv)));
        fe_to_ark(zs + 2 * i, fe_add(fe_from_ark<S>(zs + 2 * i), fe_mul(fe_from_ark<S>(zs + 2 * (i + m)), xi)));
    }
    if (i < wlen) {
        const Fe<S> wv = fe_from_ark<S>(w_in + 2 * i);
        fe_to_ark(w_out + 2 * (2 * i), wv);
        fe_to_ark(w_out + 2 * (2 * i + 1), fe_mul(wv, xi));
    }
}

// k_tail_fold with xi | xi^-1 (ark, 64 B) read from device memory: the fold of an opening whose transcript
// runs on the device (pcdl_open_fs.hip)
template <class Cv>
__global__ __launch_bounds__(256) void k_tail_fold_dev(uint4* cs, uint4* zs, size_t m, const uint4* x_dev,
                                                       const uint4* w_in, uint4* w_out, size_t wlen) {
    using S = typename Cv::Scalar;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const Fe<S> xi = fe_from_ark<S>(x_dev);
    if (i < m) {
        const Fe<S> xinv = fe_from_ark<S>(x_dev + 2);
        fe_to_ark(cs + 2 * i, fe_add(fe_from_ark<S>(cs + 2 * i), fe_mul(fe_from_ark<S>(cs + 2 * (i + m)), xinv)));
        fe_to_ark(zs + 2 * i, fe_add(fe_from_ark<S>(zs + 2 * i), fe_mul(fe_from_ark<S>(zs + 2 * (i + m)), xi)));
    }
    if (i < wlen) {
        const Fe<S> wv = fe_from_ark<S>(w_in + 2 * i);
        fe_to_ark(w_out + 2 * (2 * i), wv);
        fe_to_ark(w_out + 2 * (2 * i + 1), fe_mul(wv, xi));
    }
}

// Weighted rounds (sessions over the resident SRS, length > IPA_TAIL_N): G is never folded.  With
// len = 2m and the fold weights w (as in the tail rounds, G_i = sum_u w[u] SRS[i + u len]),
//   L = sum_{u, i < m} c[m + i] w[u] SRS[u len + i],   R = sum_{u, i < m} c[i] w[u] SRS[u len + m + i],
// two MSMs of n/2 terms over the resident window-shifted SRS (msm_srs_range_device, block map
// blk_lg = lg m).  Term j = u m + i of both: sl[j] = c[m + i] w[u], sr[j] = c[i] w[u].
template <class S>
__global__ __launch_bounds__(256) void k_weighted_scalars(const uint4* cs, const uint4* w, size_t m, int lgm,
                                                          size_t total, uint4* sl, uint4* sr) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const size_t u = j >> lgm, i = j & (m - 1);
    const Fe<S> wu = fe_from_ark<S>(w + 2 * u);
    fe_to_ark(sl + 2 * j, fe_mul(fe_from_ark<S>(cs + 2 * (m + i)), wu));
    fe_to_ark(sr + 2 * j, fe_mul(fe_from_ark<S>(cs + 2 * i), wu));
}

// A weighted round's preparation in one launch (was five: two dot products of two kernels each, the
// xi_0 scaling and k_weighted_scalars): the weighted scalars of both sides (when sl is non-null: w has
// more than one entry), and the two dots <c_r, z_l>, <c_l, z_r> as block partials whose last arriving
// block (release / acquire on *ctr, reset by it) sums them, canonicalises, scales by xi_0 (xi0_ark
// non-null) and writes dots_ark[0..2).  Same products and sums as k_dot_partial /
// k_sum_partials_to_ark / k_scale_ark, so the results are identical.  part: 2 x ndot elements
// (ndot <= gridDim.x blocks carry the dots).
template <class S>
__global__ __launch_bounds__(256) void k_weighted_prep(const uint4* cs, const uint4* zs, const uint4* w, size_t m,
                                                       int lgm, size_t total, uint4* sl, uint4* sr, uint4* part,
                                                       uint32_t* ctr, const uint4* xi0_ark, uint4* dots_ark,
                                                       uint32_t ndot) {
    __shared__ uint4 red[256 * 4];
    __shared__ uint32_t flag;
    const uint32_t tid = threadIdx.x;
    const size_t j = (size_t)blockIdx.x * 256 + tid;
    if (sl && j < total) {
        const size_t u = j >> lgm, i = j & (m - 1);
        const Fe<S> wu = fe_from_ark<S>(w + 2 * u);
        fe_to_ark(sl + 2 * j, fe_mul(fe_from_ark<S>(cs + 2 * (m + i)), wu));
        fe_to_ark(sr + 2 * j, fe_mul(fe_from_ark<S>(cs + 2 * i), wu));
    }
    // the dots: the first ndot blocks only (grid-stride over m), so that at most ndot arrivals meet on
    // the one counter (2048 same-address adds cost more than the launches they replace)
    if (blockIdx.x >= ndot) return;
    const size_t stride = (size_t)ndot * 256;
    Fe<S> a = fe_zero<S>(), b = fe_zero<S>();
    for (size_t i = j; i < m; i += stride) {
        a = fe_add(a, fe_mul(fe_load<S>(cs + 2 * (m + i)), fe_from_ark<S>(zs + 2 * i)));
        b = fe_add(b, fe_mul(fe_load<S>(cs + 2 * i), fe_from_ark<S>(zs + 2 * (m + i))));
    }
    auto block_sum2 = [&](Fe<S>& x, Fe<S>& y) {
        fe_store(red + 4 * tid, x);
        fe_store(red + 4 * tid + 2, y);
        __syncthreads();
        for (uint32_t off = 128; off > 0; off >>= 1) {
            if (tid < off) {
                fe_store(red + 4 * tid, fe_add(fe_load<S>(red + 4 * tid), fe_load<S>(red + 4 * (tid + off))));
                fe_store(red + 4 * tid + 2, fe_add(fe_load<S>(red + 4 * tid + 2), fe_load<S>(red + 4 * (tid + off) + 2)));
            }
            __syncthreads();
        }
        x = fe_load<S>(red);
        y = fe_load<S>(red + 2);
    };
    block_sum2(a, b);
    if (tid == 0) {
        tail_publish_fe((uint32_t*)(part + 4 * (size_t)blockIdx.x), a);
        tail_publish_fe((uint32_t*)(part + 4 * (size_t)blockIdx.x + 2), b);
    }
    if (!tail_arrive(ctr, ndot, &flag)) return;
    a = fe_zero<S>();
    b = fe_zero<S>();
    for (uint32_t q = tid; q < ndot; q += 256) {
        a = fe_add(a, fe_load<S>(part + 4 * (size_t)q));
        b = fe_add(b, fe_load<S>(part + 4 * (size_t)q + 2));
    }
    __syncthreads();  // (red is reused)
    block_sum2(a, b);
    if (tid != 0) return;
    *ctr = 0u;
    Fe<S> d[2] = {fe_canon(fe_reduce_2p(a)), fe_canon(fe_reduce_2p(b))};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (xi0_ark) {
            fe_store(dots_ark + 2 * k, d[k]);  // (ark words, as k_sum_partials_to_ark leaves them)
            fe_to_ark(dots_ark + 2 * k, fe_mul(fe_from_ark<S>(dots_ark + 2 * k), fe_from_ark<S>(xi0_ark)));
        } else {
            fe_store(dots_ark + 2 * k, d[k]);
        }
    }
}

// The dot blocks of k_weighted_prep alone (no scalars), as a MsmPreHide hook of the pair MSM
struct WeightedDots {
    const uint4 *cs, *zs;
    size_t m;
    uint4* part;
    uint32_t* ctr;
    const uint4* xi0;
    uint4* dots;
    uint32_t ndot;
    int curve;
};
static void weighted_dots_launch(hipStream_t ts, void* ctx) {
    const WeightedDots& d = *(const WeightedDots*)ctx;
    DISPATCH_CURVE(d.curve, Cv, {
        hipLaunchKernelGGL(k_weighted_prep<typename Cv::Scalar>, dim3(d.ndot), dim3(256), 0, ts, d.cs, d.zs,
                           (const uint4*)nullptr, d.m, 0, (size_t)0, (uint4*)nullptr, (uint4*)nullptr, d.part, d.ctr,
                           d.xi0, d.dots, d.ndot);
    });
}

}  // namespace halo

using namespace halo;

namespace {
constexpr size_t IPA_POOL_MAX = 8;  // idle sessions kept per device
std::mutex g_pool_mu;
std::vector<halo_ipa_session*> g_pool;
// every session object that exists (open or pooled), guarded by g_pool_mu: a handle is looked up here
// before anything dereferences it, so a handle whose session was destroyed (the pool was full at its
// end, or halo_shutdown ran) is refused instead of read after free
std::unordered_set<const halo_ipa_session*> g_live;

void ipa_destroy(halo_ipa_session* ses) {
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        g_live.erase(ses);
    }
    ses->destroy();
    delete ses;
}
}  // namespace

// A session for the current device: from the pool, or new with its streams and pinned staging.
halo_ipa_session* halo::ipa_acquire(DeviceState* st) {
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        for (size_t i = g_pool.size(); i-- > 0;)
            if (g_pool[i]->device == st->device) {
                halo_ipa_session* ses = g_pool[i];
                g_pool.erase(g_pool.begin() + i);
                ses->reset_state();
                ses->in_use = true;
                return ses;
            }
    }
    auto* ses = new halo_ipa_session();
    ses->device = st->device;
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        g_live.insert(ses);
    }
    // one stream per session (a side stream for the H' table of explicit-H' sessions was measured: with
    // HIP's default 4 hardware queues it shares a queue with the MSM tail streams, ~0.3 ms per 2^16
    // round; the prover's and pcdl::open's sessions use the resident 2^i H tables and build none)
    if (hipStreamCreateWithFlags(&ses->s, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&ses->htab_ready, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void**)&ses->pinned, PIN_BYTES, hipHostMallocCoherent) != hipSuccess) {
        ipa_destroy(ses);
        set_error(HALO_EDEVICE, "halo_ipa_begin: stream / pinned buffer allocation failed");
        return nullptr;
    }
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        ses->in_use = true;
    }
    return ses;
}

// the handle is an open session (checked before anything touches its state).  A
// handle of a destroyed session, or of one idle in the pool, is refused; a pooled session handed to a
// later opening is that opening's again, so a handle must not be used after its end (halo_gpu.h)
bool halo::ipa_is_open(const halo_ipa_session* ses) {
    std::lock_guard<std::mutex> g(g_pool_mu);
    return ses && g_live.count(ses) && ses->in_use;
}

// Back to the pool once its stream is idle (the pinned staging is then free); beyond IPA_POOL_MAX
// idle sessions on the device the resources are released.
void halo::ipa_release(halo_ipa_session* ses) {
    if (!ses) return;
    {
        // a handle that is not open (a second end of the same handle) is neither touched nor pooled
        // twice: two later openings would otherwise share its streams and buffers
        std::lock_guard<std::mutex> g(g_pool_mu);
        if (!g_live.count(ses) || !ses->in_use) return;
        ses->in_use = false;
    }
    if (ses->s) (void)hipStreamSynchronize(ses->s);
    ses->op.table_ref.reset();  // a retired SRS multiples table is freed with its last session
    // an idle session keeps at most "ipa_pool_keep_bytes" of device buffers (tuning, default 1 GB: a
    // 2^20 opening's ~0.6 GB stay pooled for the next one): above it the per-size buffers
    // are released here
    if ((long long)ses->buffer_bytes() > tuning(TUNE_IPA_POOL_KEEP)) ses->release_large();
    {
        std::lock_guard<std::mutex> g(g_pool_mu);
        size_t same = 0;
        for (halo_ipa_session* p : g_pool) same += p->device == ses->device;
        if (same < IPA_POOL_MAX) {
            g_pool.push_back(ses);
            return;
        }
    }
    ipa_destroy(ses);
}

// halo_shutdown: releases the pooled sessions while the HIP runtime is alive.
void halo::ipa_shutdown() {
    std::lock_guard<std::mutex> g(g_pool_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (halo_ipa_session* ses : g_pool) {
        (void)hipSetDevice(ses->device);
        g_live.erase(ses);
        ses->destroy();
        delete ses;
    }
    g_pool.clear();
    (void)hipSetDevice(cur);
}

// ------------------------------------------------------------------------------------------ IPA
// Session start shared by halo_ipa_begin (G = resident SRS prefix, z powers generated on the
// device) and halo_ipa_begin_vectors (explicit G, c, z: a shard of a distributed opening or its
// final collapsed rounds, halo_amd/dist.py).

// What the session's plan (ipa_plan.hpp) is asked with: the constants, the SRS and the tunings as they are now
// (a round reads "ipa_mat_n", "ipa_tail" and "ipa_pair_max" when it is launched).
static IpaPlanConsts ipa_plan_consts() { return {IPA_TAIL_N, TAIL_FUSE_N}; }
static IpaPlanSrs ipa_plan_srs(const SrsState& srs) { return {srs.n, srs.shifted_c != 0, srs_tab_n()}; }
static IpaPlanTunings ipa_plan_tunings() {
    IpaPlanTunings t;
    // tuning "ipa_tail" / "ipa_weighted" (default 1): 0 = no tail rounds / fold G every round
    t.tail = tuning(TUNE_IPA_TAIL) != 0;
    t.weighted = tuning(TUNE_IPA_WEIGHTED) != 0;
    // SRS sessions of n <= this start in the tail rounds over the SRS's table.  A tail round costs ~64 n0
    // table terms: measured per round (hiding open, tools/pcdl_open_time.py) 0.23 ms at n0 = 4096 against
    // 0.29 ms for the weighted path's average (opening 2^12: 5.95 -> 3.86 ms), but 0.33 ms at n0 = 8192,
    // where the weighted rounds are cheaper.
    // (tuning "ipa_srs_tail_n", default 4096; the tests pin the other paths)
    t.srs_tail_n = (size_t)tuning(TUNE_IPA_SRS_TAIL_N);
    // Length at which weighted rounds materialise G = sum_u w[u] SRS[i + u len] (one batched MSM with
    // the fold weights as shared scalars, msm_shared_batch) and continue as tail rounds: a weighted
    // round costs two n/2-term MSMs whatever the length (~0.75 ms at 2^16), a tail round ~0.25 ms.
    // Measured (opening 2^12 / 2^16 / 2^20, ms): 1024: 6.2 / 10.4 / 29.3; 2048: 5.6 / 9.3 / 27.6;
    // 4096 (tail 4096): 6.5 / 10.7 / 27.4; 8192: 6.4 / 12.8 / 28.4.
    // (tuning "ipa_mat_n", default 2048; 0 keeps the weighted rounds to the end)
    t.mat_n = (size_t)tuning(TUNE_IPA_MAT_N);
    // L and R as one MSM (key = (side, bucket)) while the round is latency-bound; at 2^19 terms per
    // side two MSMs win (R's front and accumulation overlap L's reduction tail).  Measured, opening
    // 2^14 / 2^17 / 2^18 / 2^19 / 2^20 ms, two MSMs vs one: 7.5 / 11.3 / 14.4 / 19.3 / 27.2 vs
    // 6.9 / 10.3 / 13.2 / 17.8 / 29.0 (round 4, after the sort and accumulation changes: 2^20
    // 21.7 vs 22.7 ms)
    t.pair_max = (size_t)tuning(TUNE_IPA_PAIR_MAX);
    return t;
}

// The 2^i H tables (i < IPA_HTAB, internal affine) of xi-mode sessions, kept per device and curve,
// one per distinct H and never rewritten (open sessions hold pointers into them; ADVICE r02: a new H
// used to rebuild the one shared table under live sessions).  One ~1 ms doubling chain per H, then
// shared by every later opening.  Past IPA_HTABLES_MAX distinct H, *out = nullptr: the session builds
// its own table.
constexpr size_t IPA_HTABLES_MAX = 8;
static int ipa_h_table(DeviceState* st, int curve, const halo_wrapped_point_t* Hpt, const void** out) {
    SrsState& srs = st->srs[curve];
    *out = nullptr;
    for (auto& t : srs.h_tables)
        if (!memcmp(t->key, Hpt, 64)) {
            *out = t->t.ptr;
            return HALO_OK;
        }
    if (srs.h_tables.size() >= IPA_HTABLES_MAX) return HALO_OK;
    auto ht = std::make_unique<SrsState::HTable>();
    HALO_CHECK(ht->t.reserve(IPA_HTAB * 64));
    const hipStream_t s = nullptr;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[7].reserve(IPA_HTAB * 128 + 64));
    char* tmp = (char*)st->scratch[7].ptr;
    HALO_CHECK(copy_h2d(tmp + IPA_HTAB * 128, Hpt, 64, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_pow2_xyzz_from_wrapped<Cv>, dim3(1), dim3(64), 0, s, (const uint4*)(tmp + IPA_HTAB * 128),
                           (uint4*)tmp, IPA_HTAB);
    });
    HALO_HIP(hipGetLastError());
    HALO_CHECK(xyzz_to_affine_device(curve, tmp, ht->t.ptr, IPA_HTAB, s));
    HALO_HIP(hipStreamSynchronize(s));  // sessions on other streams read it
    memcpy(ht->key, Hpt, 64);
    *out = ht->t.ptr;
    srs.h_tables.push_back(std::move(ht));
    return HALO_OK;
}


// Phase 1 of a session: G (resident SRS prefix, or explicit gs_host), c (cs_len coefficients, host or
// device (ordered on the null stream), zero-padded to n), z = powers of z (or explicit zs_host) on the
// device.  st->mu held; ses freshly acquired.
int halo::ipa_setup(DeviceState* st, halo_ipa_session* ses, int curve, size_t n, const halo_wrapped_point_t* gs_host,
                    const halo_fe_t* cs, size_t cs_len, bool cs_on_device, const halo_fe_t* zs_host, const halo_fe_t* z) {
    SrsState& srs = st->srs[curve];
    ses->op.curve = curve;
    ses->op.n = n;
    const IpaBegin b = ipa_plan_begin({n, gs_host != nullptr}, ipa_plan_srs(srs), ipa_plan_tunings(), ipa_plan_consts());
    ses->op.g = b.plan;
    hipStream_t s = ses->s;
    if (b.copy_gs) HALO_CHECK(ses->gs.reserve(n * 64));
    if (ses->op.weighted()) {  // w = [1]; scal holds the two n/2-term scalar vectors of a round
        HALO_CHECK(ses->w[0].reserve(n * 32));
        HALO_CHECK(ses->w[1].reserve(n * 32));
        HALO_CHECK(ses->scal.reserve(n * 32));
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_set_one_ark<typename Cv::Scalar>, dim3(1), dim3(64), 0, s, ses->w[0].as<uint4>());
        });
        ses->op.wcur = 0;
    }
    HALO_CHECK(ses->cs.reserve(n * 32));
    HALO_CHECK(ses->zs.reserve(n * 32));
    HALO_CHECK(ses->small.reserve(SM_BYTES));
    HALO_HIP(hipMemsetAsync(ses->small.as<char>() + SM_CTR, 0, 12, s));  // k_tail_round's / k_weighted_prep's counters
    // (n / 4: k_weighted_prep's block partials, 64 B per 256 terms of a side)
    HALO_CHECK(ses->tmp.reserve(std::max<size_t>({4096 * 32, gs_host ? n * 64 : 0, n / 4})));
    if (gs_host) {
        HALO_CHECK(copy_h2d(ses->tmp.ptr, gs_host, n * 64, s));
        HALO_CHECK(convert_wrapped_to_internal(curve, ses->tmp.ptr, ses->gs.ptr, n, s));
    } else if (b.copy_gs) {
        HALO_HIP(hipMemcpyAsync(ses->gs.ptr, srs.gs.ptr, n * 64, hipMemcpyDeviceToDevice, s));
    }
    if (cs_len < n) HALO_HIP(hipMemsetAsync(ses->cs.as<char>() + cs_len * 32, 0, (n - cs_len) * 32, s));
    if (cs_on_device) {  // the producer ran on the null stream: order the session's stream after it
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, 0) != hipSuccess ||
            hipStreamWaitEvent(s, ev, 0) != hipSuccess || hipEventDestroy(ev) != hipSuccess)
            return set_error(HALO_EDEVICE, "halo_ipa_begin_dev: stream ordering failed");
        if (cs_len) HALO_HIP(hipMemcpyAsync(ses->cs.ptr, cs, cs_len * 32, hipMemcpyDeviceToDevice, s));
    } else {
        HALO_CHECK(copy_h2d(ses->cs.ptr, cs, cs_len * 32, s));
    }
    char* sm = (char*)ses->small.ptr;
    if (zs_host) {
        HALO_CHECK(copy_h2d(ses->zs.ptr, zs_host, n * 32, s));
    } else {
        HALO_CHECK(copy_h2d(sm + SM_Z, z, 32, s));
        HALO_CHECK(powers_device(curve == HALO_PALLAS ? HALO_FP : HALO_FQ, sm + SM_Z, n, ses->zs.ptr, s));
    }
    if (gs_host) HALO_HIP(hipStreamSynchronize(s));  // tmp held the staged bases
    return HALO_OK;
}

// G of a session that skipped its copy of the SRS prefix (ipa_setup: it was to start in the tail
// rounds) but folds G before any round ran (pcdl.rs:627-687 test_u_check drives folds only), or builds its
// own tail table: the plan's fetch_gs.  G is still the prefix of length 2m.
static int ipa_fetch_gs(DeviceState* st, halo_ipa_session* ses) {
    const size_t len = 2 * ses->op.g.m;
    HALO_CHECK(ses->gs.reserve(ses->op.n * 64));
    HALO_HIP(hipMemcpyAsync(ses->gs.ptr, st->srs[ses->op.curve].gs.ptr, len * 64, hipMemcpyDeviceToDevice, ses->s));
    ses->op.g.gs_current = true;
    return HALO_OK;
}

// Phase 2: the hiding terms' table.  xi mode (xi0 and H): the shared 2^i H table and dots scaled by
// xi_0; otherwise (H_prime) a per-session 2^i H' table.  The rounds may run afterwards.
int halo::ipa_start(DeviceState* st, halo_ipa_session* ses, const halo_wrapped_point_t* H_prime, const halo_fe_t* xi0,
                    const halo_wrapped_point_t* Hpt, bool xi0_resident) {
    hipStream_t s = ses->s;
    char* sm = (char*)ses->small.ptr;
    ses->op.xi_mode = xi0 != nullptr || xi0_resident;
    const halo_wrapped_point_t* own = H_prime;  // the point of a per-session table, if one is needed
    if (ses->op.xi_mode) {  // xi_0 at [192, 224)
        HALO_CHECK(ipa_h_table(st, ses->op.curve, Hpt, &ses->op.htab_ptr));
        if (!xi0_resident) HALO_CHECK(copy_h2d(sm + SM_XI0, xi0, 32, s));
        own = ses->op.htab_ptr ? nullptr : Hpt;
    }
    ses->op.started = true;
    if (!own) {
        ses->op.htab_waited = true;
        return HALO_OK;
    }
    HALO_CHECK(ses->htab.reserve(IPA_HTAB * (64 + 128)));  // affine table + XYZZ chain scratch
    ses->op.htab_ptr = ses->htab.ptr;
    HALO_CHECK(copy_h2d(sm + SM_HP, own, 64, s));
    // 2^i H' for i < 128 (the hiding terms use the GLV split of their scalar, k_hide_term): a
    // quad-cooperative doubling chain on the session's stream; the hiding-term kernels wait for htab_ready
    const hipStream_t hs = s;
    uint4* chain = ses->htab.as<uint4>() + 4 * IPA_HTAB;  // XYZZ scratch after the affine table
    DISPATCH_CURVE(ses->op.curve, Cv, {
        hipLaunchKernelGGL(k_pow2_xyzz_from_wrapped<Cv>, dim3(1), dim3(64), 0, hs, (const uint4*)(sm + SM_HP), chain, IPA_HTAB);
    });
    HALO_HIP(hipGetLastError());
    HALO_CHECK(xyzz_to_affine_device(ses->op.curve, chain, ses->htab.ptr, IPA_HTAB, hs));
    HALO_HIP(hipEventRecord(ses->htab_ready, hs));
    ses->op.htab_waited = false;
    return HALO_OK;
}

static int ipa_begin(halo_curve_t curve, size_t n, const halo_wrapped_point_t* gs_host, const halo_fe_t* cs,
                     const halo_fe_t* zs_host, const halo_fe_t* z, const halo_wrapped_point_t* H_prime,
                     halo_ipa_session** out, bool cs_on_device = false, const halo_fe_t* xi0 = nullptr,
                     const halo_wrapped_point_t* Hpt = nullptr) {
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "unknown curve");
    if (!cs || !(z || zs_host) || !(H_prime || (xi0 && Hpt)) || !out)
        return set_error(HALO_EINVAL, "halo_ipa_begin: null argument");
    if (n <= 1) return set_error(HALO_EINVAL, "assertion failed: n > 1");
    if (!is_pow2(n)) return set_error(HALO_ENOTPOW2, "n (%zu) is not a power of two", n);
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    SrsState& srs = st->srs[curve];
    if (!gs_host && n > srs.n) return set_error(HALO_ESRSRANGE, "d (%zu) <= D (%zu)", n - 1, srs.n ? srs.n - 1 : 0);
    halo_ipa_session* ses = ipa_acquire(st);
    if (!ses) return HALO_EDEVICE;
    int rc = ipa_setup(st, ses, curve, n, gs_host, cs, n, cs_on_device, zs_host, z);
    if (!rc) rc = ipa_start(st, ses, H_prime, xi0, Hpt);
    if (rc) {
        ipa_release(ses);
        return rc;
    }
    *out = ses;
    return HALO_OK;
}

extern "C" int halo_ipa_begin(halo_curve_t curve, const halo_fe_t* cs, size_t n, const halo_fe_t* z,
                              const halo_wrapped_point_t* H_prime, halo_ipa_session** out) {
    clear_error();
    return ipa_begin(curve, n, nullptr, cs, nullptr, z, H_prime, out);
}

// Device-resident coefficients (the prover's opened polynomials never leave HBM): d_cs holds n ark
// coefficients on the device, ordered on the null stream.
extern "C" int halo_ipa_begin_dev(halo_curve_t curve, const void* d_cs, size_t n, const halo_fe_t* z,
                                  const halo_wrapped_point_t* H_prime, halo_ipa_session** out) {
    clear_error();
    return ipa_begin(curve, n, nullptr, (const halo_fe_t*)d_cs, nullptr, z, H_prime, out, true);
}

// pcdl::open_without_eval's H' = xi_0 H (pcdl.rs:390-391) inside the session: the caller passes H and
// xi_0 instead of H'; the hiding terms use a cached 2^i H table with the dots scaled by xi_0.
extern "C" int halo_ipa_begin_xi(halo_curve_t curve, const halo_fe_t* cs, size_t n, const halo_fe_t* z,
                                 const halo_wrapped_point_t* H, const halo_fe_t* xi0, halo_ipa_session** out) {
    clear_error();
    if (!xi0 || !H) return set_error(HALO_EINVAL, "halo_ipa_begin_xi: null argument");
    return ipa_begin(curve, n, nullptr, cs, nullptr, z, nullptr, out, false, xi0, H);
}
extern "C" int halo_ipa_begin_dev_xi(halo_curve_t curve, const void* d_cs, size_t n, const halo_fe_t* z,
                                     const halo_wrapped_point_t* H, const halo_fe_t* xi0, halo_ipa_session** out) {
    clear_error();
    if (!xi0 || !H) return set_error(HALO_EINVAL, "halo_ipa_begin_dev_xi: null argument");
    return ipa_begin(curve, n, nullptr, (const halo_fe_t*)d_cs, nullptr, z, nullptr, out, true, xi0, H);
}

extern "C" int halo_ipa_begin_vectors(halo_curve_t curve, const halo_wrapped_point_t* gs, const halo_fe_t* cs,
                                      const halo_fe_t* zs, size_t n, const halo_wrapped_point_t* H_prime,
                                      halo_ipa_session** out) {
    clear_error();
    if (!gs || !zs) return set_error(HALO_EINVAL, "halo_ipa_begin_vectors: null argument");
    return ipa_begin(curve, n, gs, cs, zs, nullptr, H_prime, out);
}

// v = c(z) over the session's first len coefficients, to the host (stream sync): the dot product of c
// with the session's z^i vector (ipa_setup wrote it), one parallel multiplication per coefficient
// instead of chunked Horner chains (2^10: 44 + 5 us of dependent chains -> one short dot launch pair)
int halo::ipa_eval_cs_enqueue(halo_ipa_session* ses, size_t len) {
    hipStream_t s = ses->s;
    char* sm = ses->small.as<char>();
    if (!len) {
        HALO_HIP(hipMemsetAsync(sm + SM_V, 0, 32, s));
        return HALO_OK;
    }
    HALO_CHECK(ses->tmp.reserve(4096 * 32));  // dot_device: at most 1024 block partials
    const int sf = ses->op.curve == HALO_PALLAS ? HALO_FP : HALO_FQ;
    return dot_device(sf, ses->cs.ptr, ses->zs.ptr, len, sm + SM_V, ses->tmp.ptr, s);
}

int halo::ipa_eval_cs(halo_ipa_session* ses, size_t len, halo_fe_t* v_out) {
    hipStream_t s = ses->s;
    char* sm = ses->small.as<char>();
    if (!len) {
        memset(v_out, 0, 32);
        return HALO_OK;
    }
    HALO_CHECK(ipa_eval_cs_enqueue(ses, len));
    HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_FE, sm + SM_V, 32, hipMemcpyDeviceToHost, s));
    HALO_HIP(hipStreamSynchronize(s));
    memcpy(v_out, ses->pinned + PIN_FE, 32);
    return HALO_OK;
}

// Switch to the tail rounds: G0 = current G (length 2m), w = [1], and the multiples table of G0:
// the SRS's own table when G0 is still the SRS prefix (a session of n <= IPA_TAIL_N over the SRS:
// the reference's small pcdl_open shapes, benches/pcdl.rs:35-57), else built for the session.
static int ipa_enter_tail(DeviceState* st, halo_ipa_session* ses, const IpaRound& r, hipStream_t s) {
    const size_t n0 = 2 * ses->op.g.m;
    // the largest grid of a later round: one term per lane (+ a round's per-side rounding)
    const size_t nblk = tail_blocks_at(TAIL_WIN * n0, 1) + 2;
    HALO_CHECK(ses->w[0].reserve(n0 * 32));
    HALO_CHECK(ses->w[1].reserve(n0 * 32));
    HALO_CHECK(ses->cs2.reserve(n0 * 32));
    HALO_CHECK(ses->zs2.reserve(n0 * 32));
    HALO_CHECK(ses->scal.reserve(n0 * 32));
    HALO_CHECK(ses->side.reserve(n0));
    HALO_CHECK(ses->part.reserve(nblk * 2 * 128));
    SrsState& srs = st->srs[ses->op.curve];
    if (r.tail_srs_table) {
        HALO_CHECK(srs_small_table(st, ses->op.curve, s));
        ses->op.table_ref = srs.small_tab;  // an SRS write rebuilds into a fresh buffer while this is held
        ses->op.table = srs.small_tab->as<const uint4>();
        ses->op.table_ld = srs.small_n0;
    } else {
        // a session that skipped its copy of the SRS prefix at setup but builds its own table here (the SRS
        // table is off or shorter than n0) copies the prefix now
        if (r.tail_fetch_gs) HALO_CHECK(ipa_fetch_gs(st, ses));
        HALO_CHECK(ses->own_table.reserve((size_t)TAIL_TBL * TAIL_MUL * n0 * 128));
        HALO_CHECK(tail_table_build(ses->op.curve, ses->gs.ptr, r.plan.gs_xyzz, n0, ses->own_table.ptr, s));
        ses->op.table = ses->own_table.as<const uint4>();
        ses->op.table_ld = n0;
    }
    // w = [1]: the next round's first launch uses 1 and stores it (TailFoldArgs::w_one), no launch here
    ses->op.w_one_pending = true;
    ses->op.wcur = 0;
    return HALO_OK;
}

// A tail round: L, R of the current round (with their dot * H' terms) -> small[512..768) as XYZZ; the round's
// scalars and dots come from k_tail_prep (one launch), the hiding terms ride in each side's first
// k_tail_msm block, and k_tail_final runs only when a side spans several blocks.  L and R reach `pinned`
// from the kernels: no copy.
static int ipa_round_tail(const DeviceState* st, halo_ipa_session* ses, IpaRoundKind kind, hipStream_t s) {
    const size_t n0 = ses->op.g.n0, m = ses->op.g.m;
    char* sm = (char*)ses->small.ptr;
    TailFoldArgs f{};
    f.active = ses->op.fold_pending;
    if (ses->op.w_one_pending) {  // (no fold is pending right after the switch to the tail rounds)
        f.w_one = ses->w[ses->op.wcur].as<uint4>();
        ses->op.w_one_pending = false;
    }
    if (f.active) {  // the previous round's fold, applied here (halo_ipa_fold deferred it)
        memcpy(&f.xi, &ses->op.pend_xi, 32);
        memcpy(&f.xinv, &ses->op.pend_xinv, 32);
        if (ses->op.xi_dev) f.xi_dev = (const uint4*)(sm + SM_XI);
        f.cs_out = ses->cs2.as<uint4>();
        f.zs_out = ses->zs2.as<uint4>();
        f.w_out = ses->w[ses->op.wcur ^ 1].as<uint4>();
        f.wlen_in = ses->op.g.wlen / 2;  // (the plan's wlen counts the pending fold)
    }
    TailRoundArgs ra{};
    ra.table = ses->op.table;
    ra.ld = ses->op.table_ld;
    ra.n0 = n0;
    ra.m = m;
    ra.cs = ses->cs.as<const uint4>();
    ra.zs = ses->zs.as<const uint4>();
    ra.w = ses->w[ses->op.wcur].as<const uint4>();
    ra.nbs = (uint32_t)((n0 / 2 + TAIL_THREADS / 64 - 1) / (TAIL_THREADS / 64));
    ra.xi0_ark = ses->op.xi_mode ? (const uint4*)(sm + SM_XI0) : nullptr;
    ra.htab = (const uint4*)ses->op.htab_ptr;
    ra.dots_ark = (uint4*)(sm + SM_DOT_L);
    ra.part = ses->part.as<uint4>();
    ra.ctr = (uint32_t*)(sm + SM_CTR);
    ra.out_xyzz = (uint4*)(sm + SM_L);
    ra.host = (uint32_t*)(ses->pinned + PIN_L);
    ra.seq = ++ses->poll_seq;
    if (ra.seq == 0) ra.seq = ++ses->poll_seq;  // (0 is the flags' initial value)
    ses->poll_pending = true;
    if (kind == IpaRoundKind::TailFused) {  // one fused launch (k_tail_round) up to TAIL_FUSE_N points
        HALO_CHECK(tail_round_launch(ses->op.curve, ra, f, s));
    } else {  // k_tail_digits (the point scalars and the dots) + k_tail_msm + k_tail_final
        uint32_t* hkw = (uint32_t*)(sm + SM_HKW);
        HALO_CHECK(tail_digits_launch(ses->op.curve, ra, f, ses->scal.as<uint32_t>(), ses->side.as<uint8_t>(), hkw, s));
        TailSums a;
        a.table = ses->op.table;
        a.ld = ses->op.table_ld;
        a.scal = ses->scal.as<const uint32_t>();
        a.side = ses->side.as<const uint8_t>();
        a.n0 = n0;
        a.m = m;
        a.mode = 0;
        a.blk = tail_blocks(st, TAIL_WIN * (n0 / 2), 2);  // per side: the grid is 2 blk.nblk blocks
        a.part = ses->part.as<uint4>();
        a.htab = ra.htab;
        a.hide_scalar = ra.dots_ark;
        a.hkw = hkw;
        a.out = a.out_direct = ra.out_xyzz;
        a.host = ra.host;
        a.seq = ra.seq;
        HALO_CHECK(tail_sums(ses->op.curve, a, a.blk.nblk > 1, s));  // a one-block side wrote its sum itself
    }
    if (f.active) {
        std::swap(ses->cs.ptr, ses->cs2.ptr);
        std::swap(ses->cs.bytes, ses->cs2.bytes);
        std::swap(ses->zs.ptr, ses->zs2.ptr);
        std::swap(ses->zs.bytes, ses->zs2.bytes);
        ses->op.wcur ^= 1;
        ses->op.fold_pending = false;
    }
    return HALO_OK;
}

// U = sum_u w[u] G0[u] after the last tail round -> small[256..384) as XYZZ (converted on the host)
static int ipa_tail_u(const DeviceState* st, halo_ipa_session* ses, hipStream_t s, const void* copy_src, void* copy_dst) {
    const size_t n0 = ses->op.g.n0, m = ses->op.g.m;
    char* sm = (char*)ses->small.ptr;
    if (ses->op.w_one_pending) {
        DISPATCH_CURVE(ses->op.curve, Cv, {
            hipLaunchKernelGGL(k_set_one_ark<typename Cv::Scalar>, dim3(1), dim3(64), 0, s,
                               ses->w[ses->op.wcur].as<uint4>());
        });
        HALO_HIP(hipGetLastError());
        ses->op.w_one_pending = false;
    }
    HALO_CHECK(tail_scalars_launch(ses->op.curve, ses->cs.ptr, ses->w[ses->op.wcur].ptr, n0, 2 * m, m, 1,
                                   ses->scal.as<uint32_t>(), ses->side.as<uint8_t>(), s));
    TailSums a;
    a.table = ses->op.table;
    a.ld = ses->op.table_ld;
    a.scal = ses->scal.as<const uint32_t>();
    a.side = ses->side.as<const uint8_t>();
    a.n0 = n0;
    a.m = m;
    a.blk = tail_blocks(st, TAIL_WIN * n0);
    a.part = ses->part.as<uint4>();
    a.out = a.out_direct = (uint4*)(sm + SM_U);
    a.copy_src = (const uint4*)copy_src;
    a.copy_dst = (uint4*)copy_dst;
    return tail_sums(ses->op.curve, a, a.blk.nblk > 1, s);  // one block wrote U itself
}

static int ipa_copy_out(halo_ipa_session* ses) {
    // L, R as packed XYZZ (128 B each): the affine conversion runs on the host (host_xyzz_to_wrapped)
    HALO_HIP(hipMemcpyAsync(ses->pinned + PIN_L, (char*)ses->small.ptr + SM_L, 256, hipMemcpyDeviceToHost, ses->s));
    return HALO_OK;
}

// G (length 2m) = sum_u w[u] SRS[i + u 2m] of a weighted session into gs (XYZZ for the tail table, else affine):
// from here on an ordinary session
static int ipa_materialise_g(DeviceState* st, halo_ipa_session* ses, bool xyzz, hipStream_t s) {
    const size_t len = 2 * ses->op.g.m;
    HALO_CHECK(ses->gs.reserve(len * 128));
    // over the window-shifted copies (three-window Horner) when they are resident
    const SrsState& srs = st->srs[ses->op.curve];
    const bool sh = srs.shifted_c != 0;
    return msm_shared_batch(st, ses->op.curve, sh ? srs.shifted.ptr : srs.gs.ptr, ses->w[ses->op.wcur].ptr, ses->op.g.wlen,
                            len, ses->gs.ptr, xyzz, ses->mat, s, sh ? srs.n : 0, sh ? srs.shifted_c : 0);
}

// A weighted round: the round's weighted scalars (k_weighted_prep without its dot blocks) on s, and in the pair
// path its two dots (scaled by xi_0) on the MSM's tail stream just before the hiding terms that read them
// (MsmPreHide), beside the digit / sort / accumulation phase
static int ipa_round_weighted(DeviceState* st, halo_ipa_session* ses, IpaRoundKind kind, hipEvent_t hr, hipStream_t s) {
    const size_t m = ses->op.g.m, wlen = ses->op.g.wlen;
    const int curve = ses->op.curve;
    const void* htab = ses->op.htab_ptr;
    char* sm = (char*)ses->small.ptr;
    const char* cs = ses->cs.as<const char>();
    const char* zs = ses->zs.as<const char>();
    const size_t half = ses->op.g.n0 / 2;  // = wlen * m terms per side
    const uint32_t lgm = ilog2(m);
    const char* sl = cs + m * 32;  // round 0 (w = [1]): the scalars are c_r, c_l themselves
    const char* sr = cs;
    char* sb = (char*)ses->scal.ptr;
    const unsigned nbk = grid_for(half, 256), ndot = std::min(nbk, 256u);
    HALO_CHECK(ses->tmp.reserve((size_t)ndot * 64));
    const bool pair = kind == IpaRoundKind::WeightedPair;
    WeightedDots wd{(const uint4*)cs, (const uint4*)zs, m, ses->tmp.as<uint4>(), (uint32_t*)(sm + SM_CTR + 8),
                    ses->op.xi_mode ? (const uint4*)(sm + SM_XI0) : nullptr, (uint4*)(sm + SM_DOT_L), ndot, curve};
    if (wlen > 1 || !pair) {
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_weighted_prep<typename Cv::Scalar>, dim3(wlen > 1 ? nbk : ndot), dim3(256), 0, s,
                               (const uint4*)cs, (const uint4*)zs, ses->w[ses->op.wcur].as<const uint4>(), m, (int)lgm,
                               half, wlen > 1 ? (uint4*)sb : nullptr, (uint4*)(sb + half * 32), wd.part, wd.ctr, wd.xi0,
                               wd.dots, pair ? 0u : ndot);
        });
        HALO_HIP(hipGetLastError());
    }
    if (wlen > 1) {
        sl = sb;
        sr = sb + half * 32;
    }
    // (the two-MSM form: the even half-blocks of 2^lgm points, dot H' from the GLV table, L / R as XYZZ)
    const MsmOpts blocks = MsmOpts::Async().blocks(lgm).glv_hide().xyzz().after(hr);
    if (pair) {
        // L and R reach `pinned` from k_bitcombine itself (polled, as the tail rounds): no copy
        const MsmPairIO io{sl, sr, sm + SM_DOT_L, sm + SM_DOT_R, sm + SM_L, sm + SM_R};
        const MsmPreHide pre{weighted_dots_launch, &wd};
        uint32_t seq = ++ses->poll_seq;
        if (seq == 0) seq = ++ses->poll_seq;  // (0 is the flags' initial value)
        HALO_CHECK(msm_srs_pairs_device(st, curve, 1, &io, half, lgm, htab, s, hr, &pre,
                                        (uint32_t*)(ses->pinned + PIN_L), seq));
        HALO_CHECK(msm_join(st, s));
        ses->poll_pending = true;
        return HALO_OK;
    }
    if (kind == IpaRoundKind::WeightedTwoStreams) {
        // L on the session stream and R on its second stream: the two MSMs' fronts, accumulations and
        // reduction tails overlap, instead of R's front waiting for L's accumulation (measured, 2^20
        // opening 20.5-20.8 -> 19.7-19.9 ms; with k sessions in lockstep their streams already overlap,
        // and 2k streams over the default 4 hardware queues made the prover's three openings ~2 ms
        // slower, so lockstep rounds keep one stream per session)
        if (!ses->s2) {
            HALO_HIP(hipStreamCreateWithFlags(&ses->s2, hipStreamNonBlocking));
            HALO_HIP(hipEventCreateWithFlags(&ses->ev_fork, hipEventDisableTiming));
            HALO_HIP(hipEventCreateWithFlags(&ses->ev_join, hipEventDisableTiming));
        }
        if (!ses->op.slots_reset) {
            msm_slots_reset(st);
            ses->op.slots_reset = true;
        }
        HALO_HIP(hipEventRecord(ses->ev_fork, s));
        HALO_HIP(hipStreamWaitEvent(ses->s2, ses->ev_fork, 0));
        HALO_CHECK(msm_srs_range_device(st, curve, 0, sl, half, htab, sm + SM_DOT_L, sm + SM_L, s, blocks));
        HALO_CHECK(msm_srs_range_device(st, curve, m, sr, half, htab, sm + SM_DOT_R, sm + SM_R, ses->s2, blocks));
        HALO_CHECK(msm_join(st, ses->s2));
        HALO_HIP(hipEventRecord(ses->ev_join, ses->s2));
        HALO_HIP(hipStreamWaitEvent(s, ses->ev_join, 0));
    } else {
        HALO_CHECK(msm_srs_range_device(st, curve, 0, sl, half, htab, sm + SM_DOT_L, sm + SM_L, s, blocks));
        HALO_CHECK(msm_srs_range_device(st, curve, m, sr, half, htab, sm + SM_DOT_R, sm + SM_R, s, blocks));
    }
    HALO_CHECK(msm_join(st, s));
    return ipa_copy_out(ses);
}

// A round over G itself: the two dots, then L and R as two MSMs over the SRS ranges or over gs
static int ipa_round_lr_g(DeviceState* st, halo_ipa_session* ses, IpaRoundKind kind, hipEvent_t hr, hipStream_t s) {
    const size_t m = ses->op.g.m;
    const int curve = ses->op.curve;
    const void* htab = ses->op.htab_ptr;
    const int sf = curve == HALO_PALLAS ? HALO_FP : HALO_FQ;
    char* sm = (char*)ses->small.ptr;
    const char* cs = ses->cs.as<const char>();
    const char* zs = ses->zs.as<const char>();
    const char* gs = ses->gs.as<const char>();
    HALO_CHECK(dot_device(sf, cs + m * 32, zs, m, sm + SM_DOT_L, ses->tmp.ptr, s));        // <c_r, z_l>
    HALO_CHECK(dot_device(sf, cs, zs + m * 32, m, sm + SM_DOT_R, ses->tmp.ptr, s));        // <c_l, z_r>
    if (ses->op.xi_mode) {  // dot H' = (dot xi_0) H
        DISPATCH_CURVE(curve, Cv, {
            hipLaunchKernelGGL(k_scale_ark<typename Cv::Scalar>, dim3(1), dim3(64), 0, s, (uint4*)(sm + SM_DOT_L), 2,
                               (const uint4*)(sm + SM_XI0));
        });
        HALO_HIP(hipGetLastError());
    }
    // L and R are independent: the second MSM's accumulation overlaps the first one's tail
    const MsmOpts lr = MsmOpts::Async().glv_hide().xyzz().after(hr);
    if (kind == IpaRoundKind::LrSrsRanges) {  // G_l = SRS[0, m), G_r = SRS[m, 2m): resident shifted copies, no Horner
        HALO_CHECK(msm_srs_range_device(st, curve, 0, cs + m * 32, m, htab, sm + SM_DOT_L, sm + SM_L, s, lr));
        HALO_CHECK(msm_srs_range_device(st, curve, m, cs, m, htab, sm + SM_DOT_R, sm + SM_R, s, lr));
    } else {
        HALO_CHECK(msm_device(st, curve, gs, cs + m * 32, m, htab, sm + SM_DOT_L, sm + SM_L, s, lr));
        HALO_CHECK(msm_device(st, curve, gs + m * 64, cs, m, htab, sm + SM_DOT_R, sm + SM_R, s, lr));
    }
    HALO_CHECK(msm_join(st, s));
    return ipa_copy_out(ses);
}

// A round may run: rounds are left and the session was started
static int ipa_round_ready(const halo_ipa_session* ses) {
    if (ses->op.g.m == 0) return set_error(HALO_EINVAL, "halo_ipa_round_lr: no rounds left");
    if (!ses->op.started) return set_error(HALO_EINVAL, "halo_ipa_round_lr: session not started (halo_pcdl_open_start)");
    return HALO_OK;
}

// Enqueues one round's L and R (with their H' terms) and their D2H copy into ses->pinned: what the plan's
// record of the round says, in its order.
int halo::ipa_round_launch(DeviceState* st, halo_ipa_session* ses) {
    HALO_CHECK(ipa_round_ready(ses));
    hipStream_t s = ses->s;
    const IpaRound r = ipa_plan_round(ses->op.g, ipa_plan_srs(st->srs[ses->op.curve]), ipa_plan_tunings(),
                                      ipa_plan_consts(), ses->solo);
    if (r.materialise) HALO_CHECK(ipa_materialise_g(st, ses, r.mat_xyzz, s));
    if (r.enter_tail) HALO_CHECK(ipa_enter_tail(st, ses, r, s));
    ses->op.g = r.plan;
    // only round 1 orders its hiding terms after the side-stream table: every later round starts after
    // the host has synchronised on round 1's results, which needed the table (a cross-stream wait in
    // every round cost ~0.3 ms per 2^16 round)
    hipEvent_t hr = ses->op.htab_waited ? nullptr : ses->htab_ready;
    ses->op.htab_waited = true;
    switch (r.kind) {
        case IpaRoundKind::TailFused:
        case IpaRoundKind::TailSplit:  // k_tail_prep forms the dots (scaled by xi_0) with the round's scalars
            if (hr) HALO_HIP(hipStreamWaitEvent(s, hr, 0));
            return ipa_round_tail(st, ses, r.kind, s);
        case IpaRoundKind::WeightedPair:
        case IpaRoundKind::WeightedTwoStreams:
        case IpaRoundKind::WeightedOneStream: return ipa_round_weighted(st, ses, r.kind, hr, s);
        case IpaRoundKind::LrSrsRanges:
        case IpaRoundKind::LrMsm: return ipa_round_lr_g(st, ses, r.kind, hr, s);
    }
    return HALO_OK;
}

// Enqueues the launches of one fold of half-length m with challenge xi (pcdl.rs:427-435): the weight fold of
// wlen weights (c, z and w), or the G fold (c, z and gs).
static int ipa_fold_enqueue(DeviceState* st, halo_ipa_session* ses, IpaFoldKind kind, bool fetch_gs, size_t m, size_t wlen,
                            const halo_fe_t* xi, const halo_fe_t* xi_inv) {
    hipStream_t s = ses->s;
    char* sm = (char*)ses->small.ptr;
    // the previous fold's H2D copy from the pinned staging must have completed (a round in between
    // synchronises the stream; two folds in a row wait here)
    if (ses->op.fold_inflight) HALO_HIP(hipStreamSynchronize(s));
    // a device transcript's xi | xi^-1 are already at SM_XI (no by-value pair, no staging copy)
    const uint4* x_dev = ses->op.xi_dev ? (const uint4*)(sm + SM_XI) : nullptr;
    if (kind == IpaFoldKind::Weights) {
        // xi, xi^-1 as kernel arguments: no staging copy, so nothing for a later fold to wait on
        ArkScalarPair x{};
        if (!x_dev) {
            memcpy(&x.v[0], xi, 32);
            memcpy(&x.v[2], xi_inv, 32);
        }
        const dim3 grid(grid_for(std::max(m, wlen), 256));
        const uint4* w_in = ses->w[ses->op.wcur].as<const uint4>();
        uint4* w_out = ses->w[ses->op.wcur ^ 1].as<uint4>();
        DISPATCH_CURVE(ses->op.curve, Cv, {
            if (x_dev)
                hipLaunchKernelGGL(k_tail_fold_dev<Cv>, grid, dim3(256), 0, s, ses->cs.as<uint4>(), ses->zs.as<uint4>(), m,
                                   x_dev, w_in, w_out, wlen);
            else
                hipLaunchKernelGGL(k_tail_fold<Cv>, grid, dim3(256), 0, s, ses->cs.as<uint4>(), ses->zs.as<uint4>(), m, x,
                                   w_in, w_out, wlen);
        });
        HALO_HIP(hipGetLastError());
        ses->op.wcur ^= 1;
        return HALO_OK;
    }
    if (!x_dev) {
        ses->op.fold_inflight = true;
        memcpy(ses->pinned + PIN_XI, xi, 32);
        memcpy(ses->pinned + PIN_XINV, xi_inv, 32);
        HALO_HIP(hipMemcpyAsync(sm + SM_XI, ses->pinned + PIN_XI, 64, hipMemcpyHostToDevice, s));
    }
    if (fetch_gs) HALO_CHECK(ipa_fetch_gs(st, ses));
    {
        DISPATCH_CURVE(ses->op.curve, Cv, {
            ProfScope prof("ipa_fold", s);
            HALO_LAUNCH(prof, k_ipa_fold<Cv>, dim3(grid_for(m, FOLD_THREADS)), dim3(FOLD_THREADS), 0, s, ses->gs.as<uint4>(),
                        ses->cs.as<uint4>(), ses->zs.as<uint4>(), m, (const uint4*)(sm + SM_XI),
                        (const uint4*)(sm + SM_XINV));
        });
        HALO_HIP(hipGetLastError());
    }
    return HALO_OK;
}

// A deferred tail-round fold applied on its own (before U at the end, a state read, or a second fold); the
// plan advanced when it was deferred.
static int ipa_apply_pending_fold(DeviceState* st, halo_ipa_session* ses) {
    if (!ses->op.fold_pending) return HALO_OK;
    ses->op.fold_pending = false;
    return ipa_fold_enqueue(st, ses, IpaFoldKind::Weights, false, ses->op.pend_m, ses->op.g.wlen / 2, &ses->op.pend_xi,
                            &ses->op.pend_xinv);
}

// Enqueues one fold with challenge xi; the session advances to the next round.
int halo::ipa_fold_launch(DeviceState* st, halo_ipa_session* ses, const halo_fe_t* xi, const halo_fe_t* xi_inv) {
    if (ses->op.g.m == 0) return set_error(HALO_EINVAL, "halo_ipa_fold: no rounds left");
    if (!ses->op.started) return set_error(HALO_EINVAL, "halo_ipa_fold: session not started (halo_pcdl_open_start)");
    if (!ses->op.xi_dev && (!xi || !xi_inv)) return set_error(HALO_EINVAL, "halo_ipa_fold: null argument");
    const IpaFold f = ipa_plan_fold(ses->op.g);
    if (f.kind == IpaFoldKind::Deferred) {  // applied by the next round's k_tail_prep (no launch, no copy now)
        HALO_CHECK(ipa_apply_pending_fold(st, ses));
        if (!ses->op.xi_dev) {  // (a device transcript's challenge stays at SM_XI until the round that applies it)
            ses->op.pend_xi = *xi;
            ses->op.pend_xinv = *xi_inv;
        }
        ses->op.pend_m = ses->op.g.m;
        ses->op.fold_pending = true;
    } else {
        HALO_CHECK(ipa_fold_enqueue(st, ses, f.kind, f.fetch_gs, ses->op.g.m, ses->op.g.wlen, xi, xi_inv));
    }
    ses->op.g = f.plan;
    return HALO_OK;
}

// Waits for a tail round's L and R in `pinned` (tail_emit_host): spins on the two flags; after 2 s
// (a failed or very late launch) it synchronises the stream, which reports a launch error, and takes
// L, R from the device copy instead.
static int ipa_poll_lr(halo_ipa_session* ses) {
    ses->poll_pending = false;
    const volatile uint32_t* fl = (const volatile uint32_t*)(ses->pinned + PIN_FLAGS);
    const uint32_t seq = ses->poll_seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; spin++) {
        if (__atomic_load_n(&fl[0], __ATOMIC_ACQUIRE) == seq && __atomic_load_n(&fl[1], __ATOMIC_ACQUIRE) == seq) {
            // the flags are the round's last stores, stream-ordered after any fold it followed
            ses->op.fold_inflight = false;
            return HALO_OK;
        }
        // spin politely: a pause per probe, and past ~1 ms (a round is 0.1-2 ms) give the core up between
        // probes (the spin holds the device mutex)
        __builtin_ia32_pause();
        if (spin > (1u << 16)) std::this_thread::yield();
        if ((spin & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) break;
    }
    HALO_HIP(hipStreamSynchronize(ses->s));
    HALO_HIP(hipMemcpy(ses->pinned + PIN_L, (char*)ses->small.ptr + SM_L, 256, hipMemcpyDeviceToHost));
    return HALO_OK;
}

// The session list of a _multi call: every entry an open session, none listed twice.  Checked before the call
// touches any session, so a refused call leaves all k where they were (lockstep openings stay in step; ADVICE
// r05).  not_open_note: what the call's "is not open" text adds.
static int ipa_check_sessions(const char* call, halo_ipa_session* const* ses, size_t k, const char* not_open_note = "") {
    if (k && !ses) return set_error(HALO_EINVAL, "%s: null session list", call);
    for (size_t i = 0; i < k; i++) {
        if (!ses[i]) return set_error(HALO_EINVAL, "%s: null session %zu", call, i);
        if (!ipa_is_open(ses[i])) return set_error(HALO_EINVAL, "%s: session %zu is not open%s", call, i, not_open_note);
        for (size_t j = 0; j < i; j++)
            if (ses[j] == ses[i]) return set_error(HALO_EINVAL, "%s: session %zu listed twice", call, i);
    }
    return HALO_OK;
}

extern "C" int halo_ipa_round_lr(halo_ipa_session* ses, halo_wrapped_point_t* L, halo_wrapped_point_t* R) {
    clear_error();
    if (!ses || !L || !R) return set_error(HALO_EINVAL, "halo_ipa_round_lr: null argument");
    return halo_ipa_round_lr_multi(&ses, 1, L, R);
}

// k independent openings advanced in lockstep: every session's round is enqueued on its own stream
// before any is waited for, so their latency-bound kernels overlap on the device.
extern "C" int halo_ipa_round_lr_multi(halo_ipa_session* const* ses, size_t k, halo_wrapped_point_t* L,
                                       halo_wrapped_point_t* R) {
    clear_error();
    if (!ses || !L || !R) return set_error(HALO_EINVAL, "halo_ipa_round_lr_multi: null argument");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    // every session checked before the first round is enqueued (a session listed twice would run two rounds
    // on one state and return the second one's L, R for both)
    HALO_CHECK(ipa_check_sessions("halo_ipa_round_lr_multi", ses, k));
    for (size_t i = 0; i < k; i++) HALO_CHECK(ipa_round_ready(ses[i]));
    for (size_t i = 0; i < k; i++) {
        ses[i]->solo = k == 1;
        HALO_CHECK(ipa_round_launch(st, ses[i]));
    }
    for (size_t i = 0; i < k; i++) {
        if (ses[i]->poll_pending) {
            HALO_CHECK(ipa_poll_lr(ses[i]));
        } else {
            HALO_HIP(hipStreamSynchronize(ses[i]->s));
            ses[i]->op.fold_inflight = false;
        }
        const void* src[2] = {ses[i]->pinned + PIN_L, ses[i]->pinned + PIN_R};
        void* dst[2] = {&L[i], &R[i]};
        host_xyzz_to_wrapped2(ses[i]->op.curve, src, dst, 2);
    }
    return HALO_OK;
}

// One round whose L and R stay on the device (the distributed opening's per-round reduce):
// the round is enqueued as halo_ipa_round_lr enqueues it, L and R (packed XYZZ, 2 x 128 B) are copied to
// d_lr on the session's stream, and `stream` is ordered after that copy.  No host wait: the caller
// gathers and sums the ranks' pairs on the device (halo_point_sum_xyzz_dev) and brings one sum home.
extern "C" int halo_ipa_round_lr_dev(halo_ipa_session* ses, void* d_lr, void* stream) {
    clear_error();
    if (!ses || !d_lr) return set_error(HALO_EINVAL, "halo_ipa_round_lr_dev: null argument");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    if (!ipa_is_open(ses)) return set_error(HALO_EINVAL, "halo_ipa_round_lr_dev: the session is not open");
    ses->solo = true;
    HALO_CHECK(ipa_round_launch(st, ses));
    ses->poll_pending = false;  // (the copy a tail / pair round emits to the pinned staging is not waited for)
    HALO_HIP(hipMemcpyAsync(d_lr, (char*)ses->small.ptr + SM_L, 256, hipMemcpyDeviceToDevice, ses->s));
    if (!ses->lr_ready) HALO_HIP(hipEventCreateWithFlags(&ses->lr_ready, hipEventDisableTiming));
    HALO_HIP(hipEventRecord(ses->lr_ready, ses->s));
    HALO_HIP(hipStreamWaitEvent((hipStream_t)stream, ses->lr_ready, 0));
    return HALO_OK;
}

extern "C" int halo_ipa_fold(halo_ipa_session* ses, const halo_fe_t* xi, const halo_fe_t* xi_inv) {
    clear_error();
    if (!ses || !xi) return set_error(HALO_EINVAL, "halo_ipa_fold: null argument");
    return halo_ipa_fold_multi(&ses, 1, xi, xi_inv);
}

extern "C" int halo_ipa_fold_multi(halo_ipa_session* const* ses, size_t k, const halo_fe_t* xi,
                                   const halo_fe_t* xi_inv) {
    clear_error();
    if (!ses || !xi) return set_error(HALO_EINVAL, "halo_ipa_fold_multi: null argument");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    // every session checked and every inverse formed before the first fold is enqueued: an argument
    // error leaves all k sessions where they were
    HALO_CHECK(ipa_check_sessions("halo_ipa_fold_multi", ses, k));
    std::vector<halo_fe_t> inv(xi_inv ? 0 : k);
    for (size_t i = 0; i < k; i++) {
        // xi_inv == NULL: xi^-1 formed here, as the reference's fold does (pcdl.rs:430)
        if (!xi_inv && !host_scalar_inverse(ses[i]->op.curve, &xi[i], &inv[i]))
            return set_error(HALO_EINVAL, "halo_ipa_fold_multi: xi %zu is zero (no inverse)", i);
    }
    for (size_t i = 0; i < k; i++) HALO_CHECK(ipa_fold_launch(st, ses[i], &xi[i], xi_inv ? &xi_inv[i] : &inv[i]));
    // no host wait: the fold is stream-ordered before the next round (which synchronises), so the host
    // goes on to the transcript and the next round's launches while it runs
    return HALO_OK;
}

extern "C" int halo_ipa_state(halo_ipa_session* ses, size_t* m, halo_wrapped_point_t* gs, halo_fe_t* cs, halo_fe_t* zs) {
    clear_error();
    if (!ses) return set_error(HALO_EINVAL, "halo_ipa_state: null session");
    if (!ipa_is_open(ses)) return set_error(HALO_EINVAL, "halo_ipa_state: the session is not open");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = ses->s;
    HALO_CHECK(ipa_apply_pending_fold(st, ses));
    const size_t len = std::max<size_t>(2 * ses->op.g.m, 1);
    if (m) *m = ses->op.g.m;
    if (gs && (ses->op.tail() || ses->op.weighted() || !ses->op.g.gs_current))
        return set_error(HALO_EINVAL,
                         "halo_ipa_state: G is not materialised in the weighted / tail rounds (HALO_IPA_WEIGHTED=0, "
                         "HALO_IPA_TAIL=0)");
    if (gs) {
        HALO_CHECK(ses->tmp.reserve(std::max<size_t>(len * 64, 4096 * 32)));
        HALO_CHECK(convert_internal_to_wrapped(ses->op.curve, ses->gs.ptr, ses->tmp.ptr, len, s));
        HALO_CHECK(copy_d2h(gs, ses->tmp.ptr, len * 64, s));
    }
    if (cs) HALO_CHECK(copy_d2h(cs, ses->cs.ptr, len * 32, s));
    if (zs) HALO_CHECK(copy_d2h(zs, ses->zs.ptr, len * 32, s));
    return HALO_OK;
}

// halo_ipa_end in two halves: the device work enqueued on the session's stream (st->mu held), then the
// wait, the host conversion and the release -- halo_ipa_end_multi enqueues every session's end before
// it waits for any, so the lockstep openings' final U sums overlap on the device.
int halo::ipa_end_enqueue(DeviceState* st, halo_ipa_session* ses) {
    hipStream_t s = ses->s;
    char* sm = (char*)ses->small.ptr;
    int rc = HALO_OK;
    if (!ses->op.started) {
        rc = set_error(HALO_EINVAL, "halo_ipa_end: session not started");
    } else if ((rc = ipa_apply_pending_fold(st, ses))) {
    } else if (ses->op.tail() || ses->op.weighted()) {
        // U = G_0 = sum_u w[u] G0[u] (len = 1 once every round ran)
        if (ses->op.g.m != 0)
            rc = set_error(HALO_EINVAL, "halo_ipa_end: U needs every round in the weighted / tail rounds (m = %zu)",
                           ses->op.g.m);
        else if (ses->op.tail())  // XYZZ at [256, 384), converted below; c = cs[0] copied to [384, 416) by its last block
            rc = ipa_tail_u(st, ses, s, ses->cs.ptr, sm + SM_U_C_XYZZ);
        else
            rc = msm_srs_range_device(st, ses->op.curve, 0, ses->w[ses->op.wcur].ptr, ses->op.g.n0, nullptr, nullptr,
                                      sm + SM_U, s, MsmOpts::Sync());
        if (!rc && !ses->op.tail() && hipMemcpyAsync(sm + SM_U_C, ses->cs.ptr, 32, hipMemcpyDeviceToDevice, s) != hipSuccess)
            rc = set_error(HALO_EDEVICE, "ipa end copy failed");
    } else if (!ses->op.g.gs_current && (rc = ipa_fetch_gs(st, ses))) {  // (no round and no fold ran: G is the SRS prefix)
    } else {
        DISPATCH_CURVE(ses->op.curve, Cv, {
            hipLaunchKernelGGL(k_copy_first_wrapped<Cv>, dim3(1), dim3(64), 0, s, ses->gs.as<const uint4>(),
                               ses->cs.as<const uint4>(), (uint4*)(sm + SM_U), (uint4*)(sm + SM_U_C));
        });
        if (hipGetLastError() != hipSuccess) rc = set_error(HALO_EDEVICE, "ipa end launch failed");
    }
    // one copy through the pinned staging: U (wrapped, or XYZZ [256, 384) after tail rounds), c
    const size_t u_bytes = ses->op.tail() ? 160 : 96;
    if (!rc && hipMemcpyAsync(ses->pinned + PIN_U, sm + SM_U, u_bytes, hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = set_error(HALO_EDEVICE, "ipa end copy failed");
    return rc;
}

int halo::ipa_end_finish(halo_ipa_session* ses, halo_wrapped_point_t* U, halo_fe_t* c) {
    const bool u_xyzz = ses->op.tail();
    if (hipStreamSynchronize(ses->s) != hipSuccess) return set_error(HALO_EDEVICE, "ipa end synchronisation failed");
    if (U) {
        if (u_xyzz)
            host_xyzz_to_wrapped(ses->op.curve, ses->pinned + PIN_U, U);
        else
            memcpy(U, ses->pinned + PIN_U, 64);
    }
    if (c) memcpy(c, ses->pinned + (u_xyzz ? PIN_U_C_XYZZ : PIN_U_C), 32);
    return HALO_OK;
}

extern "C" int halo_ipa_end(halo_ipa_session* ses, halo_wrapped_point_t* U, halo_fe_t* c) {
    clear_error();
    if (!ses) return set_error(HALO_EINVAL, "halo_ipa_end: null session");
    if (!ipa_is_open(ses)) return set_error(HALO_EINVAL, "halo_ipa_end: the session is not open (already ended)");
    int rc = HALO_OK;
    if (U || c) {
        DeviceState* st = current_state();
        if (!st) {
            ipa_release(ses);
            return HALO_EDEVICE;
        }
        std::lock_guard<std::mutex> g(st->mu);
        rc = ipa_end_enqueue(st, ses);
        if (!rc) rc = ipa_end_finish(ses, U, c);
    }
    ipa_release(ses);
    return rc;
}

extern "C" int halo_ipa_end_multi(halo_ipa_session* const* ses, size_t k, halo_wrapped_point_t* U, halo_fe_t* c) {
    clear_error();
    HALO_CHECK(ipa_check_sessions("halo_ipa_end_multi", ses, k, " (already ended)"));
    int rc = HALO_OK;
    if (k && (U || c)) {
        DeviceState* st = current_state();
        if (!st) {
            for (size_t i = 0; i < k; i++) ipa_release(ses[i]);
            return HALO_EDEVICE;
        }
        std::lock_guard<std::mutex> g(st->mu);
        for (size_t i = 0; i < k && !rc; i++) rc = ipa_end_enqueue(st, ses[i]);
        // every stream is drained before any session goes back to the pool, failed or not
        for (size_t i = 0; i < k; i++) {
            const int r = rc ? (hipStreamSynchronize(ses[i]->s) == hipSuccess ? HALO_OK : HALO_EDEVICE)
                             : ipa_end_finish(ses[i], U ? U + i : nullptr, c ? c + i : nullptr);
            if (!rc && r) rc = r;
        }
    }
    for (size_t i = 0; i < k; i++) ipa_release(ses[i]);
    return rc;
}

extern "C" int halo_ipa_fold_host(halo_curve_t curve, halo_wrapped_point_t* gs, halo_fe_t* cs, halo_fe_t* zs, size_t m,
                                  const halo_fe_t* xi, const halo_fe_t* xi_inv) {
    clear_error();
    if (!valid_curve(curve)) return set_error(HALO_EINVAL, "unknown curve");
    if (!xi || !xi_inv || (m && (!gs || !cs || !zs))) return set_error(HALO_EINVAL, "halo_ipa_fold_host: null argument");
    if (!m) return HALO_OK;
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(2 * m * 64));
    HALO_CHECK(st->scratch[1].reserve(2 * m * 64));
    HALO_CHECK(st->scratch[2].reserve(2 * m * 32));
    HALO_CHECK(st->scratch[3].reserve(2 * m * 32));
    HALO_CHECK(st->scratch[4].reserve(64));
    char* xb = (char*)st->scratch[4].ptr;  // xi | xi^-1
    HALO_CHECK(copy_h2d(st->scratch[0].ptr, gs, 2 * m * 64, s));
    HALO_CHECK(copy_h2d(st->scratch[2].ptr, cs, 2 * m * 32, s));
    HALO_CHECK(copy_h2d(st->scratch[3].ptr, zs, 2 * m * 32, s));
    HALO_CHECK(copy_h2d(xb, xi, 32, s));
    HALO_CHECK(copy_h2d(xb + 32, xi_inv, 32, s));
    HALO_CHECK(convert_wrapped_to_internal(curve, st->scratch[0].ptr, st->scratch[1].ptr, 2 * m, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_ipa_fold<Cv>, dim3(grid_for(m, 128)), dim3(128), 0, s, st->scratch[1].as<uint4>(),
                           st->scratch[2].as<uint4>(), st->scratch[3].as<uint4>(), m, (const uint4*)xb,
                           (const uint4*)(xb + 32));
    });
    HALO_HIP(hipGetLastError());
    HALO_CHECK(convert_internal_to_wrapped(curve, st->scratch[1].ptr, st->scratch[0].ptr, m, s));
    HALO_CHECK(copy_d2h(gs, st->scratch[0].ptr, m * 64, s));
    HALO_CHECK(copy_d2h(cs, st->scratch[2].ptr, m * 32, s));
    HALO_CHECK(copy_d2h(zs, st->scratch[3].ptr, m * 32, s));
    return HALO_OK;
}
