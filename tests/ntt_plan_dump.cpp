// Drives what halo_amd/csrc/ntt_plan.hpp computes (tests/test_ntt_plan.py).  Built by the host C++ compiler
// alone: the header is free of HIP.  One command per line, read from stdin, one JSON object per command:
//   split logn big_max_log even_split                          the radices and their cache key
//   prune lr request                                           ntt_pass0_prune
//   g0 ne r                                                    ntt_g0
//   check log_n batch                                          ntt_check
//   plan logn inverse in_place prune_request big_max_log even  the whole plan
//   sweep            every combination listed in sweep() below; prints the number of plans, the violations of
//                    each property, and every (ne, r) a pass had
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <utility>

#include "ntt_plan.hpp"

using namespace halo;

static const char* buf_name(NttBuf b) {
    return b == NttBuf::In ? "IN" : b == NttBuf::Out ? "OUT" : b == NttBuf::Tmp ? "TMP" : "TMP2";
}

static void print_plan(const NttPlan& pl) {
    printf("{\"logn\": %u, \"npass\": %u, \"split_key\": %llu, \"lo_bits\": %u, \"nlo\": %zu, \"nhi\": %zu, \"tables\": %d, "
           "\"needs_tmp2\": %d, \"read_end\": %zu, \"pass\": [",
           pl.logn, pl.npass, (unsigned long long)pl.split_key, pl.lo_bits, pl.nlo, pl.nhi, (int)pl.tables, (int)pl.needs_tmp2,
           pl.read_end);
    for (unsigned p = 0; p < pl.npass; p++) {
        const NttPassPlan& q = pl.pass[p];
        printf("%s{\"log_r\": %u, \"log_ns\": %u, \"ne\": %d, \"t\": %u, \"grid_x\": %u, \"full\": %d, \"threads\": %u, "
               "\"lds_bytes\": %u, \"in_ark\": %d, \"out_ark\": %d, \"prune\": %u, \"table\": %d, \"table_entries\": %zu, "
               "\"out_scaled\": %d, \"src\": \"%s\", \"dst\": \"%s\"}",
               p ? ", " : "", q.log_r, q.log_ns, q.ne, q.t, q.grid_x, (int)q.full, q.threads, q.lds_bytes, (int)q.in_ark,
               (int)q.out_ark, q.prune, (int)q.table, q.table_entries, (int)q.out_scaled, buf_name(q.src), buf_name(q.dst));
    }
    printf("]}\n");
}

// In place the caller's one buffer plays both In and Out
static bool ntt_same_buffer(const NttPlan& pl, NttBuf a, NttBuf b) {
    return a == b || (pl.in_place && (a == NttBuf::In || a == NttBuf::Out) && (b == NttBuf::In || b == NttBuf::Out));
}

struct Bad {
    unsigned long long plans = 0, radix = 0, block = 0, geometry = 0, tables = 0, key = 0, prune = 0, chain = 0, tmp2 = 0,
                       alias = 0, out_scaled = 0, read_end = 0, ark = 0, two_level = 0;
};

// The properties listed at the top of ntt_plan.hpp, counted per plan
static void check(const NttPlan& pl, unsigned request, Bad& bad, std::set<std::pair<int, unsigned>>& seen) {
    bad.plans++;
    const unsigned P = pl.npass, logn = pl.logn;
    const size_t N = (size_t)1 << logn;
    if ((P == 0) != (logn == 0) || P > NTT_MAX_PASSES) bad.radix++;
    unsigned sum = 0;
    uint64_t key = 0;
    for (unsigned p = 0; p < P; p++) {
        const NttPassPlan& q = pl.pass[p];
        seen.insert({q.ne, q.log_r});
        if (q.log_r < 1 || q.log_r > NTT_MAX_LOG_R_BIG) bad.radix++;
        if (q.log_ns != sum) bad.radix++;
        // the ranges NttSwz was searched for
        if (q.ne != (q.log_r <= 8 ? 1024 : 2048)) bad.block++;
        if (q.threads != (unsigned)q.ne / 4 || q.lds_bytes != (unsigned)q.ne * 36) bad.block++;
        if ((size_t)q.t * q.grid_x != (N >> q.log_r) || q.t == 0 || ((size_t)q.t << q.log_r) > (size_t)q.ne) bad.geometry++;
        if (q.full != (((size_t)q.t << q.log_r) == (size_t)q.ne)) bad.geometry++;
        // a block holds as many columns as fit, or all there are
        if (q.t != (unsigned)q.ne >> q.log_r && q.grid_x != 1) bad.geometry++;
        if (q.table != (pl.tables && p > 0)) bad.tables++;
        if (q.table_entries != (q.table ? (size_t)1 << (q.log_r + q.log_ns) : 0)) bad.tables++;
        if (q.out_scaled != (pl.tables && P > 1 && p == P - 1)) bad.out_scaled++;
        if (q.in_ark != (p == 0) || q.out_ark != (p == P - 1)) bad.ark++;
        if (p > 0 || pl.inverse) {
            if (q.prune) bad.prune++;
        } else {
            if (q.prune != ntt_pass0_prune(q.log_r, request) || q.prune > request) bad.prune++;
            if (q.prune && (q.prune < ntt_g0(q.ne, q.log_r) || q.prune >= q.log_r)) bad.prune++;
            if (q.prune && q.ne == 2048 && ((q.log_r - q.prune) & 1)) bad.prune++;
        }
        if (q.src != (p ? pl.pass[p - 1].dst : NttBuf::In)) bad.chain++;
        if (q.src == NttBuf::Tmp2 && p != 1) bad.tmp2++;
        if (q.dst == NttBuf::In || (q.dst == NttBuf::Tmp2 && (p != 0 || !pl.in_place))) bad.tmp2++;
        if (ntt_same_buffer(pl, q.src, q.dst) && !(P == 1 && q.grid_x == 1)) bad.alias++;
        if (q.log_r >> NTT_KEY_BITS) bad.key++;
        key = (key << 5) | q.log_r;
        sum += q.log_r;
    }
    if (sum != logn) bad.radix++;
    if (key != pl.split_key) bad.key++;
    if (pl.tables != (logn <= 24)) bad.tables++;
    if (P && pl.pass[P - 1].dst != NttBuf::Out) bad.chain++;
    bool any_tmp2 = false;
    for (unsigned p = 0; p < P; p++) any_tmp2 |= pl.pass[p].dst == NttBuf::Tmp2;
    if (any_tmp2 != pl.needs_tmp2) bad.tmp2++;
    const unsigned pr = P ? pl.pass[0].prune : 0;
    if (pl.read_end != (pr ? N >> pr : N)) bad.read_end++;
    if (pl.lo_bits != (logn + 1) / 2 || pl.nlo != (size_t)1 << pl.lo_bits || pl.nlo * pl.nhi != N) bad.two_level++;
}

static void sweep() {
    Bad bad;
    std::set<std::pair<int, unsigned>> seen;
    for (unsigned logn = 0; logn <= 30; logn++)
        for (long long big : {0, 16, 17, 20, 22, 99})
            for (int even = 0; even < 2; even++)
                for (int in_place = 0; in_place < 2; in_place++)
                    for (int inverse = 0; inverse < 2; inverse++)
                        for (unsigned request = 0; request <= logn; request++)
                            check(ntt_plan(logn, inverse != 0, in_place != 0, request, big, even != 0), request, bad, seen);
    printf("{\"plans\": %llu, \"radix\": %llu, \"block\": %llu, \"geometry\": %llu, \"tables\": %llu, \"key\": %llu, "
           "\"prune\": %llu, \"chain\": %llu, \"tmp2\": %llu, \"alias\": %llu, \"out_scaled\": %llu, \"read_end\": %llu, "
           "\"ark\": %llu, \"two_level\": %llu, \"seen\": [",
           bad.plans, bad.radix, bad.block, bad.geometry, bad.tables, bad.key, bad.prune, bad.chain, bad.tmp2, bad.alias,
           bad.out_scaled, bad.read_end, bad.ark, bad.two_level);
    bool first = true;
    for (const auto& s : seen) {
        printf("%s[%d, %u]", first ? "" : ", ", s.first, s.second);
        first = false;
    }
    printf("]}\n");
}

static const char* check_name(NttCheck c) {
    switch (c) {
        case NttCheck::Ok: return "ok";
        case NttCheck::Empty: return "empty";
        case NttCheck::LogTooLarge: return "log_too_large";
        case NttCheck::BatchTooLarge: return "batch_too_large";
    }
    return "?";
}

int main() {
    char line[256], cmd[16];
    while (fgets(line, sizeof line, stdin)) {
        long long a[6] = {};
        const int got = sscanf(line, "%15s %lld %lld %lld %lld %lld %lld", cmd, a, a + 1, a + 2, a + 3, a + 4, a + 5);
        if (got < 1) continue;
        if (!strcmp(cmd, "sweep") && got == 1) {
            sweep();
        } else if (!strcmp(cmd, "split") && got == 4) {
            const NttSplit sp = ntt_split((unsigned)a[0], a[1], a[2] != 0);
            printf("{\"radices\": [");
            for (unsigned p = 0; p < sp.npass; p++) printf("%s%u", p ? ", " : "", sp.log_r[p]);
            printf("], \"key\": %llu}\n", (unsigned long long)ntt_split_key(sp));
        } else if (!strcmp(cmd, "prune") && got == 3) {
            printf("{\"granted\": %u}\n", ntt_pass0_prune((unsigned)a[0], (unsigned)a[1]));
        } else if (!strcmp(cmd, "g0") && got == 3) {
            printf("{\"g0\": %u}\n", ntt_g0((int)a[0], (unsigned)a[1]));
        } else if (!strcmp(cmd, "check") && got == 3) {
            printf("{\"check\": \"%s\"}\n", check_name(ntt_check((unsigned)a[0], (size_t)a[1])));
        } else if (!strcmp(cmd, "plan") && got == 7) {
            print_plan(ntt_plan((unsigned)a[0], a[1] != 0, a[2] != 0, (unsigned)a[3], a[4], a[5] != 0));
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
