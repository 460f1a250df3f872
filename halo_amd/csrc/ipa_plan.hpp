// The path of an IPA session (ipa.hip) as a value and a stepper: which form G has, what a round launches and
// what a fold does, for given (n, SRS, tunings).  Host-only and free of HIP types, so a plain C++17 compiler
// builds it (tests/test_ipa_plan.py).  ipa.hip performs what the records say and decides nothing itself.
//
// The forms of G (length 2m in a round of half-length m), and what can follow what:
//
//   begin -+-> Folded      G was given explicitly (halo_ipa_begin_vectors): gs holds it, every fold folds it
//          |
//          +-> Weighted    over the SRS, the window-shifted copies resident, n > IPA_TAIL_N, not tail_from_srs,
//          |   |           ipa_weighted: G is never folded, G_i = sum_u w[u] SRS[i + u 2m] is carried by the fold
//          |   |           weights w (wlen of them, wlen 2m = n0 = n); L / R are MSMs over the shifted SRS
//          |   |
//          |   +-> Folded  the first round with 2m <= ipa_mat_n materialises G into gs by one shared-scalar MSM:
//          |               as XYZZ when that round also enters the tail (ipa_tail, 2m <= IPA_TAIL_N), else affine.
//          |               ipa_mat_n = 0: never, U = sum_u w[u] SRS[u] at the end
//          |
//          +-> SrsPrefix   over the SRS otherwise: G = SRS[0, 2m) until the first fold.  L / R over the shifted
//              |           SRS ranges when the copies are resident, else by MSM over gs.  gs holds a copy of the
//              |           prefix unless the session is to enter the tail in its first round; a G fold or an own
//              |           tail table that finds no copy fetches it first
//              |
//              +-> Folded  the first fold (folds before any round: pcdl.rs test_u_check)
//
//   SrsPrefix, Folded -> Tail   in a round with allow_tail and (2m <= IPA_TAIL_N or tail_from_srs): G0 = G is
//                          fixed (n0 = 2m), w = [1], and L / R are sums over a multiples table of G0: the SRS's
//                          own table while G0 is the unfolded prefix and n0 <= min(srs_tab_n, srs.n), else a
//                          table built from gs in the layout gs was written in.  Folds only update w, and are
//                          deferred into the next round's launch.  Tail is never left.
//
// allow_tail is fixed at begin (over the SRS and ipa_tail; off in Weighted, and read again from ipa_tail when G
// is materialised), tail_from_srs at begin (allow_tail and n <= min(ipa_srs_tail_n, srs_tab_n, srs.n): tail
// rounds from round 1 over the SRS's table).  The tunings are arguments of every step: ipa_mat_n, ipa_tail and
// ipa_pair_max act when a round is launched.
#pragma once
#include <algorithm>
#include <cstddef>

namespace halo {

enum class GForm { SrsPrefix, Folded, Weighted, Tail };

// what a round launches for L and R
enum class IpaRoundKind {
    TailFused,           // one launch over the multiples table (n0 <= TAIL_FUSE_N)
    TailSplit,           // digits, table sums and the final sum as separate launches
    WeightedPair,        // L and R as one MSM over the shifted SRS (terms per side <= ipa_pair_max)
    WeightedTwoStreams,  // two MSMs, R's on the session's second stream (the call advances this session alone)
    WeightedOneStream,   // two MSMs on the session's stream (sessions in lockstep)
    LrSrsRanges,         // G_l = SRS[0, m), G_r = SRS[m, 2m) on the resident shifted copies
    LrMsm,               // plain MSMs over gs
};

enum class IpaFoldKind {
    Deferred,  // Tail: applied by the next round's launch
    Weights,   // Weighted: c, z and w' = interleave(w, xi w)
    G,         // SrsPrefix, Folded: c, z and G itself
};

struct IpaPlanSession {
    size_t n;
    bool explicit_g;  // G given by the caller, not the SRS prefix
};
struct IpaPlanSrs {
    size_t n;      // points resident
    bool shifted;  // the window-shifted copies are resident
    size_t tab_n;  // srs_tab_n(): points the SRS's multiples table covers at most
};
struct IpaPlanTunings {
    bool tail, weighted;  // "ipa_tail", "ipa_weighted" != 0
    size_t srs_tail_n, mat_n, pair_max;
};
struct IpaPlanConsts {
    size_t tail_n;  // IPA_TAIL_N
    size_t fuse_n;  // TAIL_FUSE_N
};

struct IpaPlan {
    GForm form = GForm::SrsPrefix;
    size_t m = 0;             // half-length of the next round; 0: every round ran
    size_t n0 = 0, wlen = 0;  // Weighted, Tail: length of G0 and of w after every fold so far (wlen 2m = n0)
    bool gs_current = false;  // gs holds the current G
    bool gs_xyzz = false;     // ... as XYZZ points (materialised for the tail table only), else affine
    bool srs_table = false;   // Tail: the table is the SRS's, not the session's own
    // fixed at begin
    bool allow_tail = false, tail_from_srs = false;
    bool srs_shifted = false;  // SrsPrefix: L / R on the shifted copies
};

struct IpaBegin {
    IpaPlan plan;
    bool copy_gs;  // gs is filled at setup: the caller's G, or a copy of the SRS prefix
};

struct IpaRound {
    IpaPlan plan;  // after the round's materialisation and tail entry (m is the round's own)
    bool materialise = false, mat_xyzz = false;  // first gs = sum_u w[u] SRS[i + u 2m], as XYZZ or affine
    bool enter_tail = false;                     // then G0 = G, on ...
    bool tail_srs_table = false;                 // ... the SRS's table, or the session's own, built from gs ...
    bool tail_fetch_gs = false;                  // ... after fetching the SRS prefix into gs
    IpaRoundKind kind = IpaRoundKind::LrMsm;
};

struct IpaFold {
    IpaPlan plan;  // after the fold
    IpaFoldKind kind = IpaFoldKind::G;
    bool fetch_gs = false;  // G: gs has no copy of the SRS prefix yet
};

inline IpaBegin ipa_plan_begin(const IpaPlanSession& ses, const IpaPlanSrs& srs, const IpaPlanTunings& t,
                               const IpaPlanConsts& c) {
    IpaPlan p;
    p.m = ses.n / 2;
    p.allow_tail = !ses.explicit_g && t.tail;
    p.tail_from_srs = p.allow_tail && ses.n <= std::min({t.srs_tail_n, srs.tab_n, srs.n});
    const bool weighted = !ses.explicit_g && srs.shifted && ses.n > c.tail_n && !p.tail_from_srs && t.weighted;
    p.form = ses.explicit_g ? GForm::Folded : weighted ? GForm::Weighted : GForm::SrsPrefix;
    if (weighted) {
        p.allow_tail = false;
        p.n0 = ses.n;
        p.wlen = 1;
    }
    p.srs_shifted = p.form == GForm::SrsPrefix && srs.shifted;
    // an SRS session that starts in the tail rounds never reads G itself (the SRS's table does)
    const bool first_round_tail = p.allow_tail && (ses.n <= c.tail_n || p.tail_from_srs);
    p.gs_current = ses.explicit_g || (p.form == GForm::SrsPrefix && !first_round_tail);
    return {p, p.gs_current};
}

// The round of half-length p.m > 0
inline IpaRound ipa_plan_round(const IpaPlan& p, const IpaPlanSrs& srs, const IpaPlanTunings& t, const IpaPlanConsts& c,
                               bool solo) {
    IpaRound r;
    IpaPlan& q = r.plan = p;
    const size_t len = 2 * p.m;
    if (q.form == GForm::Weighted && len <= t.mat_n) {  // from here on an ordinary (tail) session
        q.allow_tail = t.tail;
        r.materialise = true;
        r.mat_xyzz = q.allow_tail && len <= c.tail_n;  // the tail table reads XYZZ directly
        q.form = GForm::Folded;
        q.gs_current = true;
        q.gs_xyzz = r.mat_xyzz;
        q.n0 = q.wlen = 0;
    }
    if (q.form != GForm::Tail && q.allow_tail && (len <= c.tail_n || q.tail_from_srs)) {
        r.enter_tail = true;
        r.tail_srs_table = q.form == GForm::SrsPrefix && len <= std::min(srs.tab_n, srs.n);
        r.tail_fetch_gs = !r.tail_srs_table && !q.gs_current;
        if (r.tail_fetch_gs) q.gs_current = true;
        q.form = GForm::Tail;
        q.srs_table = r.tail_srs_table;
        q.n0 = len;
        q.wlen = 1;
    }
    switch (q.form) {
        case GForm::Tail: r.kind = q.n0 <= c.fuse_n ? IpaRoundKind::TailFused : IpaRoundKind::TailSplit; break;
        case GForm::Weighted:
            r.kind = q.n0 / 2 <= t.pair_max ? IpaRoundKind::WeightedPair
                     : solo                 ? IpaRoundKind::WeightedTwoStreams
                                            : IpaRoundKind::WeightedOneStream;
            break;
        case GForm::SrsPrefix: r.kind = q.srs_shifted ? IpaRoundKind::LrSrsRanges : IpaRoundKind::LrMsm; break;
        case GForm::Folded: r.kind = IpaRoundKind::LrMsm; break;
    }
    return r;
}

// The fold of half-length p.m > 0
inline IpaFold ipa_plan_fold(const IpaPlan& p) {
    IpaFold f;
    IpaPlan& q = f.plan = p;
    switch (p.form) {
        case GForm::Tail: f.kind = IpaFoldKind::Deferred; break;
        case GForm::Weighted: f.kind = IpaFoldKind::Weights; break;
        case GForm::SrsPrefix:
        case GForm::Folded:
            f.kind = IpaFoldKind::G;
            f.fetch_gs = !p.gs_current;
            q.form = GForm::Folded;
            q.gs_current = true;
            q.srs_shifted = false;
            break;
    }
    if (f.kind != IpaFoldKind::G) q.wlen *= 2;
    q.m /= 2;
    return f;
}

}  // namespace halo
