// The walk over a PCDL transcript (Sponge::new(Protocols::PCDL), pcdl.rs:336-425, 496-534) that the
// verifier's kernels (pcdl_fs.hip) and the prover's (pcdl_open_fs.hip) share.
#pragma once
#include "curve.hpp"
#include "outer_sponge.hpp"

namespace halo {

constexpr int PCDL_LABEL = 0;  // Protocols::PCDL (outer_sponge.rs:17-22)

// One stretch of a transcript, between two challenges: [the label] [the scalar w] the coordinates of np <= 2
// points [z, v], every element through the one absorb call, then the next challenge into w.
template <class Cv, int LANES>
HALO_DEV void transcript_stretch(poseidon::OuterSponge<Cv, LANES>& sp, bool label, bool pre, const uint4* p0, const uint4* p1,
                                 int np, bool post, const uint4* z, const uint4* v, uint32_t (&w)[8]) {
    using Sp = poseidon::OuterSponge<Cv, LANES>;
    using F = typename Cv::Base;
    constexpr int NS = Sp::FR_ELEMENTS;
    const int n_label = label ? 1 : 0, n_pre = pre ? NS : 0, n_g = 2 * np, total = n_label + n_pre + n_g + (post ? 2 * NS : 0);
#pragma unroll 1
    for (int e = 0; e < total; e++) {
        int q = e - n_label;
        Fe<F> x;
        if (q < 0) {
            x = Sp::label_element(PCDL_LABEL);
        } else if (q < n_pre) {
            x = Sp::fr_element(w, q);
        } else if (q < n_pre + n_g) {
            q -= n_pre;
            x = Sp::g_element(q < 2 ? p0 : p1, q & 1);
        } else {
            q -= n_pre + n_g;
            uint32_t sw[8];
            fe_ark_to_canonical_words<typename Cv::Scalar>(q < NS ? z : v, sw);
            x = Sp::fr_element(sw, q < NS ? q : q - NS);
        }
        sp.absorb(x);
    }
    sp.challenge(w);
}

}  // namespace halo
