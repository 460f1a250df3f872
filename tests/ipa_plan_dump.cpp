// Drives what halo_amd/csrc/ipa_plan.hpp computes (tests/test_ipa_plan.py).  Built by the host C++ compiler
// alone: the header is free of HIP.  One command per line, read from stdin, one JSON object per command:
//   sweep            every combination listed in sweep() below, rounds and folds alternately and folds only;
//                    prints the number of runs and the violations of each property
//   trace n explicit srs_n shifted tab_n tail weighted srs_tail_n mat_n pair_max solo
//                    one opening, rounds and folds alternately: what begin says, every round and every fold
#include <cstdio>
#include <cstring>
#include <string>

#include "ipa_plan.hpp"

using namespace halo;

static const IpaPlanConsts kConsts{2048, 256};  // IPA_TAIL_N (ipa.hip), TAIL_FUSE_N (tail.hpp)
static const size_t kTabN = 8192;               // srs_tab_n() (tail.hip)

static const char* kind_name(IpaRoundKind k) {
    switch (k) {
        case IpaRoundKind::TailFused: return "tail_fused";
        case IpaRoundKind::TailSplit: return "tail_split";
        case IpaRoundKind::WeightedPair: return "weighted_pair";
        case IpaRoundKind::WeightedTwoStreams: return "weighted_two_streams";
        case IpaRoundKind::WeightedOneStream: return "weighted_one_stream";
        case IpaRoundKind::LrSrsRanges: return "lr_srs_ranges";
        case IpaRoundKind::LrMsm: return "lr_msm";
    }
    return "?";
}
static const char* form_name(GForm f) {
    return f == GForm::SrsPrefix ? "srs_prefix" : f == GForm::Folded ? "folded" : f == GForm::Weighted ? "weighted" : "tail";
}

struct Bad {
    unsigned long long runs = 0, rounds = 0, tail_left = 0, weighted_cond = 0, explicit_g = 0, gs_read = 0, srs_table = 0,
                       mat = 0, deferred = 0, wlen = 0;
};

// One opening under fixed inputs.  with_rounds: a round before every fold; else folds only (pcdl.rs test_u_check).
// gs is modelled beside the plan (what was written into it, and in which layout), so the plan's own gs_current
// and gs_xyzz are checked, not trusted.
static void run(const IpaPlanSession& ses, const IpaPlanSrs& srs, const IpaPlanTunings& t, bool solo, bool with_rounds,
                Bad& bad, std::string* trace) {
    const IpaBegin b = ipa_plan_begin(ses, srs, t, kConsts);
    IpaPlan p = b.plan;
    bool gs_written = b.copy_gs, gs_is_xyzz = false;  // the model of gs
    size_t folds = 0, rounds = 0, mats = 0;
    bool mat_due_seen = false;
    bad.runs++;
    if (trace) *trace += std::string("\"begin\": \"") + form_name(p.form) + (b.copy_gs ? "+copy_gs" : "") + "\", \"rounds\": [";
    std::string fold_trace;
    auto check_state = [&](const IpaPlan& q) {
        if (q.form == GForm::Weighted && (ses.explicit_g || !srs.shifted)) bad.weighted_cond++;
        if (ses.explicit_g && q.form != GForm::Folded) bad.explicit_g++;
        if (q.gs_current && !gs_written) bad.gs_read++;
        if (q.gs_current && q.gs_xyzz != gs_is_xyzz) bad.gs_read++;
        if (q.form == GForm::Weighted || q.form == GForm::Tail)
            if (q.m ? q.wlen * 2 * q.m != q.n0 : q.wlen != q.n0) bad.wlen++;
    };
    check_state(p);
    while (p.m) {
        if (with_rounds) {
            const IpaRound r = ipa_plan_round(p, srs, t, kConsts, solo);
            rounds++;
            const size_t len = 2 * p.m;
            const bool due = p.form == GForm::Weighted && len <= t.mat_n;
            if (r.materialise) {
                mats++;
                if (!due || mat_due_seen || mats > 1) bad.mat++;
                gs_written = true;
                gs_is_xyzz = r.mat_xyzz;
            } else if (due) {
                bad.mat++;
            }
            mat_due_seen |= due;
            if (p.form == GForm::Tail && (r.plan.form != GForm::Tail || r.enter_tail)) bad.tail_left++;
            if (r.enter_tail) {
                if (r.plan.form != GForm::Tail || r.plan.n0 != len) bad.tail_left++;
                if (r.tail_srs_table) {
                    const bool unfolded_prefix = !ses.explicit_g && folds == 0 && !mats && p.form == GForm::SrsPrefix;
                    if (!unfolded_prefix || len > std::min(srs.tab_n, srs.n)) bad.srs_table++;
                    if (ses.explicit_g) bad.explicit_g++;
                } else {  // the own table is built from gs
                    if (r.tail_fetch_gs) {
                        if (ses.explicit_g || folds || mats) bad.gs_read++;  // only the unfolded prefix can be fetched
                        gs_written = true;
                        gs_is_xyzz = false;
                    }
                    if (!gs_written || r.plan.gs_xyzz != gs_is_xyzz) bad.gs_read++;
                }
            } else if (r.tail_srs_table || r.tail_fetch_gs) {
                bad.srs_table++;
            }
            if (r.kind == IpaRoundKind::LrMsm && (!gs_written || gs_is_xyzz)) bad.gs_read++;
            const bool tail_kind = r.kind == IpaRoundKind::TailFused || r.kind == IpaRoundKind::TailSplit;
            const bool w_kind = r.kind == IpaRoundKind::WeightedPair || r.kind == IpaRoundKind::WeightedTwoStreams ||
                                r.kind == IpaRoundKind::WeightedOneStream;
            if (tail_kind != (r.plan.form == GForm::Tail) || w_kind != (r.plan.form == GForm::Weighted)) bad.tail_left++;
            if (r.plan.m != p.m) bad.rounds++;
            if (trace) {
                if (rounds > 1) *trace += ", ";
                *trace += "\"";
                if (r.materialise) *trace += r.mat_xyzz ? "mat_xyzz>" : "mat_affine>";
                if (r.enter_tail) *trace += r.tail_srs_table ? "tail_srs>" : r.tail_fetch_gs ? "tail_own_fetch>" : "tail_own>";
                *trace += std::string(kind_name(r.kind)) + "\"";
            }
            p = r.plan;
            check_state(p);
        }
        const IpaFold f = ipa_plan_fold(p);
        if ((f.kind == IpaFoldKind::Deferred) != (p.form == GForm::Tail)) bad.deferred++;
        if (p.form == GForm::Tail && f.plan.form != GForm::Tail) bad.tail_left++;
        if (f.kind == IpaFoldKind::G) {
            if (f.fetch_gs) {
                if (ses.explicit_g || folds || mats) bad.gs_read++;
                gs_written = true;
                gs_is_xyzz = false;
            }
            if (!gs_written || gs_is_xyzz) bad.gs_read++;
        } else if (f.fetch_gs) {
            bad.gs_read++;
        }
        if (ses.explicit_g && (f.kind != IpaFoldKind::G || f.fetch_gs)) bad.explicit_g++;
        if (f.plan.m != p.m / 2) bad.rounds++;
        if (!fold_trace.empty()) fold_trace += ", ";
        fold_trace += f.kind == IpaFoldKind::Deferred  ? "\"deferred\""
                      : f.kind == IpaFoldKind::Weights ? "\"weights\""
                      : f.fetch_gs                     ? "\"g_fetch\""
                                                       : "\"g\"";
        folds++;
        p = f.plan;
        check_state(p);
    }
    size_t lg = 0;
    while (((size_t)1 << lg) < ses.n) lg++;
    if (folds != lg || (with_rounds && rounds != lg)) bad.rounds++;
    if (trace) *trace += "], \"folds\": [" + fold_trace + "], \"end\": \"" + form_name(p.form) + "\"";
}

static void sweep() {
    Bad bad;
    const IpaPlanTunings def{true, true, 4096, 2048, (size_t)1 << 19};
    for (unsigned lg = 1; lg <= 24; lg++) {
        const size_t n = (size_t)1 << lg;
        IpaPlanTunings sets[8] = {def, def, def, def, def, def, def, def};
        sets[1].srs_tail_n = 0;
        sets[2].srs_tail_n = n;
        sets[3].weighted = false;
        sets[4].tail = false;
        sets[5].mat_n = 0;
        sets[6].pair_max = 0;
        sets[7].weighted = false;  // tests/test_gpu_prover.py's "fold" modes pin two keys at once
        sets[7].srs_tail_n = 0;
        for (int ex = 0; ex < 2; ex++)
            for (size_t srs_n : {n, 2 * n})
                for (int sh = 0; sh < 2; sh++)
                    for (const IpaPlanTunings& t : sets)
                        for (int solo = 0; solo < 2; solo++)
                            for (int with_rounds = 0; with_rounds < 2; with_rounds++)
                                run({n, ex != 0}, {srs_n, sh != 0, kTabN}, t, solo != 0, with_rounds != 0, bad, nullptr);
    }
    printf("{\"runs\": %llu, \"rounds\": %llu, \"tail_left\": %llu, \"weighted_cond\": %llu, \"explicit_g\": %llu, "
           "\"gs_read\": %llu, \"srs_table\": %llu, \"mat\": %llu, \"deferred\": %llu, \"wlen\": %llu}\n",
           bad.runs, bad.rounds, bad.tail_left, bad.weighted_cond, bad.explicit_g, bad.gs_read, bad.srs_table, bad.mat,
           bad.deferred, bad.wlen);
}

int main() {
    char line[512], cmd[16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[11] = {};
        const int got = sscanf(line, "%15s %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu %llu", cmd, a, a + 1, a + 2, a + 3,
                               a + 4, a + 5, a + 6, a + 7, a + 8, a + 9, a + 10);
        if (got < 1) continue;
        if (!strcmp(cmd, "sweep") && got == 1) {
            sweep();
        } else if (!strcmp(cmd, "trace") && got == 12) {
            Bad bad;
            std::string tr;
            run({(size_t)a[0], a[1] != 0}, {(size_t)a[2], a[3] != 0, (size_t)a[4]},
                {a[5] != 0, a[6] != 0, (size_t)a[7], (size_t)a[8], (size_t)a[9]}, a[10] != 0, true, bad, &tr);
            const unsigned long long nbad = bad.rounds + bad.tail_left + bad.weighted_cond + bad.explicit_g + bad.gs_read +
                                            bad.srs_table + bad.mat + bad.deferred + bad.wlen;
            printf("{%s, \"violations\": %llu}\n", tr.c_str(), nbad);
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
