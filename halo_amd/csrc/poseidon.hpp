// Device Poseidon sponge over a Pasta field (crates/poseidon/src/inner_sponge.rs:3-108): state width 3,
// rate 2, 55 full rounds, each S-box x^7, then the MDS matrix, then the round constants, with the
// reference's Absorbed(n) / Squeezed(n) state machine.
//
// The 9 + 165 constants are the caller's (halo_poseidon_set_params); a block stages them in LDS once
// (stage_params) as 29-bit limbs, MDS row-major first, then the round constants round-major.
//
// Two lane layouts with the same interface and the same results:
//   Sponge<F, 1>  one lane holds the whole state: 21 multiplications per round on the lane's chain,
//                 every constant read at a wave-uniform LDS address.
//   Sponge<F, 3>  three neighbouring lanes hold one state element each (21 sponges per wave, lane 63
//                 idle): 4 multiplications for x^7, the two other elements over the lane crossbar, 3
//                 for the lane's MDS row (kept in registers) -- a 7-multiplication chain per round and
//                 three times the waves for the same batch.
#pragma once
#include "fields.hpp"
#include "sponge_plan.hpp"

HALO_ARITH_BEGIN
namespace poseidon {

constexpr int WIDTH = 3, RATE = 2, ROUNDS = 55;
constexpr int N_CONST = WIDTH * WIDTH + ROUNDS * WIDTH;  // 174
constexpr int TABLE_WORDS = N_CONST * NLIMB;
constexpr int SPONGES_PER_WAVE_3 = (int)::halo::SPONGES_PER_WAVE_3;  // sponge_plan.hpp: the launch plan counts with it
constexpr int STATE_U4 = 2 * WIDTH + 1;  // a sponge's state in memory (Sponge::store): 3 x 32 B, then (squeezed, n)

// global table -> LDS, by the whole block
HALO_DEV void stage_params(const uint32_t* __restrict__ g, uint32_t* lds) {
    for (int i = threadIdx.x; i < TABLE_WORDS; i += blockDim.x) lds[i] = g[i];
    __syncthreads();
}

template <class F>
HALO_DEV Fe<F> table_fe(const uint32_t* tab, int idx) {
    Fe<F> r;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) r.v[l] = tab[idx * NLIMB + l];
    return r;
}

template <class F>
HALO_DEV Fe<F> fe_shfl(const Fe<F>& a, int src) {
    Fe<F> r;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) r.v[l] = __shfl(a.v[l], src);
    return r;
}

// x^7 for a normalized x < 8p; result < 2p
template <class F>
HALO_DEV Fe<F> sbox(const Fe<F>& x) {
    const Fe<F> x2 = fe_sqr(x);
    const Fe<F> x4 = fe_sqr(x2);
    return fe_mul(fe_mul(x4, x2), x);
}

// m0 t0 + m1 t1 + m2 t2 + c: two Montgomery reductions, the sums left unreduced -- normalized limbs,
// value < 2p + 2p + p = 5p, a valid multiplication / squaring input (fields.hpp).
template <class F>
HALO_DEV Fe<F> mds_row(const Fe<F>& m0, const Fe<F>& t0, const Fe<F>& m1, const Fe<F>& t1, const Fe<F>& m2,
                       const Fe<F>& t2, const Fe<F>& c) {
    return fe_norm(fe_add_nc(fe_add_nc(fe_mul2(m0, t0, m1, t1), fe_mul(m2, t2)), c));
}

template <class F, int LANES>
struct Sponge;

template <class F>
struct Sponge<F, 1> {
    Fe<F> s[WIDTH];  // each normalized, < 5p
    const uint32_t* tab;
    bool squeezed;
    int n;

    HALO_DEV void init(const uint32_t* lds_tab) {
        tab = lds_tab;
        for (int i = 0; i < WIDTH; i++) s[i] = fe_zero<F>();
        squeezed = false;
        n = 0;
    }
    // The stored state (STATE_U4 uint4): the three elements below 2p as packed words, then (squeezed, n).
    // mine: this lane's sponge is the one stored.
    HALO_DEV void store(uint4* dst, bool mine) const {
        if (!mine) return;
        for (int i = 0; i < WIDTH; i++) fe_store(dst + 2 * i, fe_reduce_8p(s[i]));
        dst[2 * WIDTH] = make_uint4(squeezed ? 1u : 0u, (uint32_t)n, 0u, 0u);
    }
    HALO_DEV void load(const uint32_t* lds_tab, const uint4* src) {
        tab = lds_tab;
        for (int i = 0; i < WIDTH; i++) s[i] = fe_load<F>(src + 2 * i);
        const uint4 fl = src[2 * WIDTH];
        squeezed = fl.x != 0;
        n = (int)fl.y;
    }
    HALO_DEV void permute() {
#pragma unroll 1
        for (int r = 0; r < ROUNDS; r++) {
            const Fe<F> t0 = sbox(s[0]), t1 = sbox(s[1]), t2 = sbox(s[2]);
#pragma unroll
            for (int i = 0; i < WIDTH; i++)
                s[i] = mds_row(table_fe<F>(tab, 3 * i), t0, table_fe<F>(tab, 3 * i + 1), t1, table_fe<F>(tab, 3 * i + 2),
                               t2, table_fe<F>(tab, WIDTH * WIDTH + 3 * r + i));
        }
    }
    HALO_DEV void add_to(int i, const Fe<F>& x) {  // i < RATE, wave-uniform
        if (i == 0)
            s[0] = fe_add(fe_reduce_8p(s[0]), x);
        else
            s[1] = fe_add(fe_reduce_8p(s[1]), x);
    }
    // inner_sponge.rs absorb, one element (x < 2p)
    HALO_DEV void absorb(const Fe<F>& x) {
        if (!squeezed && n < RATE) {
            add_to(n, x);
            n++;
        } else {
            if (!squeezed) permute();  // Absorbed(RATE)
            squeezed = false;
            n = 1;
            add_to(0, x);
        }
    }
    HALO_DEV Fe<F> squeeze() {
        if (squeezed && n < RATE) {
            n++;
            return fe_reduce_8p(n == 1 ? s[0] : s[1]);
        }
        permute();
        squeezed = true;
        n = 1;
        return fe_reduce_8p(s[0]);
    }
};

template <class F>
struct Sponge<F, 3> {
    Fe<F> s;           // state element `role` of this lane's sponge
    Fe<F> m0, m1, m2;  // MDS[role][role], MDS[role][role + 1], MDS[role][role + 2] (indices mod 3)
    const uint32_t* tab;
    int role, base, la, lb;
    bool squeezed;
    int n;

    // Every lane of the wave calls every member; lane 63 belongs to no sponge and talks to itself.
    HALO_DEV void init(const uint32_t* lds_tab) {
        tab = lds_tab;
        const int lane = threadIdx.x & 63;
        role = lane % 3;
        base = lane - role;
        la = base + (role + 1) % 3;
        lb = base + (role + 2) % 3;
        if (lane == 63) la = lb = 63;
        m0 = table_fe<F>(tab, 3 * role + role);
        m1 = table_fe<F>(tab, 3 * role + (role + 1) % 3);
        m2 = table_fe<F>(tab, 3 * role + (role + 2) % 3);
        s = fe_zero<F>();
        squeezed = false;
        n = 0;
    }
    // The same stored state as the one-lane layout's: each of the sponge's three lanes stores / loads its element.
    HALO_DEV void store(uint4* dst, bool mine) const {
        if (!mine) return;
        fe_store(dst + 2 * role, fe_reduce_8p(s));
        if (role == 0) dst[2 * WIDTH] = make_uint4(squeezed ? 1u : 0u, (uint32_t)n, 0u, 0u);
    }
    HALO_DEV void load(const uint32_t* lds_tab, const uint4* src) {
        init(lds_tab);
        s = fe_load<F>(src + 2 * role);
        const uint4 fl = src[2 * WIDTH];
        squeezed = fl.x != 0;
        n = (int)fl.y;
    }
    HALO_DEV void permute() {
#pragma unroll 1
        for (int r = 0; r < ROUNDS; r++) {
            const Fe<F> t = sbox(s);
            s = mds_row(m0, t, m1, fe_shfl(t, la), m2, fe_shfl(t, lb), table_fe<F>(tab, WIDTH * WIDTH + 3 * r + role));
        }
    }
    HALO_DEV void add_to(int i, const Fe<F>& x) {
        const Fe<F> sum = fe_add(fe_reduce_8p(s), x);
        s = fe_select(role == i, sum, s);
    }
    HALO_DEV void absorb(const Fe<F>& x) {
        if (!squeezed && n < RATE) {
            add_to(n, x);
            n++;
        } else {
            if (!squeezed) permute();
            squeezed = false;
            n = 1;
            add_to(0, x);
        }
    }
    // the squeezed element, in every lane of the sponge
    HALO_DEV Fe<F> squeeze() {
        if (squeezed && n < RATE) {
            n++;
            return fe_reduce_8p(fe_shfl(s, (threadIdx.x & 63) == 63 ? 63 : base + n - 1));
        }
        permute();
        squeezed = true;
        n = 1;
        return fe_reduce_8p(fe_shfl(s, base));
    }
};

}  // namespace poseidon
HALO_ARITH_END
