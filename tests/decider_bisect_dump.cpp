// Runs the descent of halo_amd/csrc/decider_bisect.hpp against a toy additive group (tests/test_decider_bisect.py).
// Built by the host C++ compiler alone: the header is free of HIP.  The stand-in for the device works in Z / p,
// p = 2^61 - 1: D(S) = sum_{i in S, i wrong} rho_i delta_i mod p with fixed nonzero rho, chosen so that no sum over a
// nonempty set of wrong instances vanishes (weights "inc": rho_i = i + 1, delta_i = 1; weights "signed", k <= 60:
// rho_i = 2^i, delta_i = +-1 alternating, where an unweighted sum of two neighbours would cancel).
// One command per line on stdin, one JSON object per command on stdout:
//   sweep k n budget W weights           every subset of the k instances as the wrong ones
//   random k n budget W count seed       `count` random subsets, their density varying from one wrong instance to all
//   trace k n budget W i j ...           one descent with the wrong instances i j ..., level by level
// n, budget, W: decider_group's arguments (coefficients per instance, scalars per group, windows per scalar).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "decider_bisect.hpp"

using namespace halo;

static const uint64_t P = ((uint64_t)1 << 61) - 1;
static uint64_t addp(uint64_t a, uint64_t b) { return (a + b) % P; }
static uint64_t subp(uint64_t a, uint64_t b) { return (a + P - b) % P; }

struct Toy {  // the Eval of bisect_descend
    size_t k, n, budget;
    int W;
    std::vector<uint64_t> term;  // rho_i delta_i, 0 for a good instance
    std::vector<uint64_t> cur, next, left;
    std::vector<uint8_t> have;
    // what the test reads
    std::vector<std::vector<size_t>> groups;  // per level: the rows of each group
    std::vector<std::vector<BisectNode>> levels;
    size_t rows_total = 0, bad_group = 0, bad_defect = 0;
    size_t expect_r0 = 0;

    uint64_t D(size_t lo, size_t hi) const {
        uint64_t s = 0;
        for (size_t i = lo; i < hi; i++) s = addp(s, term[i]);
        return s;
    }
    int rows(const BisectNode* level, size_t f, size_t r0, size_t m) {
        if (r0 == 0) {
            levels.emplace_back(level, level + f);
            groups.emplace_back();
            left.assign(f, 0);
            have.assign(f, 0);
            expect_r0 = 0;
        }
        const size_t g = decider_group(n, f, budget, W);
        // the decider_group properties: groups in order without gaps, none empty, none above g; within the budget
        // unless it is one row; below the 2^32 entries of the one-MSM path
        if (r0 != expect_r0 || m < 1 || m > g || r0 + m > f) bad_group++;
        if (m * n > budget && m != 1) bad_group++;
        if ((unsigned __int128)m * (unsigned)W * n >= ((unsigned __int128)1 << 32)) bad_group++;
        if (r0 + m < f && m != g) bad_group++;  // only the last group is ragged
        expect_r0 = r0 + m;
        groups.back().push_back(m);
        for (size_t s = r0; s < r0 + m; s++) {
            const BisectNode& nd = level[s];
            if (nd.mid != nd.lo + (nd.hi - nd.lo) / 2 || nd.hi - nd.lo < 2) bad_group++;  // the split rule
            left[s] = D(nd.lo, nd.mid);
            have[s] = 1;
        }
        rows_total += m;
        return 0;
    }
    int split(const BisectNode* level, size_t f, uint8_t* flags) {
        if (expect_r0 != f) bad_group++;  // the groups covered the level
        next.assign(2 * f, 0);
        for (size_t s = 0; s < f; s++) {
            if (!have[s]) bad_group++;
            const uint64_t Dn = cur[level[s].src];
            if (Dn != D(level[s].lo, level[s].hi) || Dn == 0) bad_defect++;  // src names the node's own defect, a failing one
            next[2 * s] = left[s];
            next[2 * s + 1] = subp(Dn, left[s]);
            flags[2 * s] = next[2 * s] != 0;
            flags[2 * s + 1] = next[2 * s + 1] != 0;
        }
        cur.swap(next);
        return 0;
    }
};

static size_t ceil_lg(size_t k) {
    size_t l = 0;
    while (((size_t)1 << l) < k) l++;
    return l;
}

// failing internal nodes of the tree over [lo, hi)
static size_t failing_nodes(const std::vector<uint8_t>& wrong, size_t lo, size_t hi) {
    if (hi - lo < 2) return 0;
    bool any = false;
    for (size_t i = lo; i < hi; i++) any = any || wrong[i];
    if (!any) return 0;
    const size_t mid = lo + (hi - lo) / 2;
    return 1 + failing_nodes(wrong, lo, mid) + failing_nodes(wrong, mid, hi);
}

struct Tally {
    unsigned long long cases = 0, bad_verdict = 0, bad_rows = 0, over_bound = 0, bad_group = 0, bad_defect = 0, deep = 0;
};

// One batch: the combined root pass decides whether the descent runs at all, as decide_bisect_device does.
static void run_case(size_t k, size_t n, size_t budget, int W, bool signed_w, const std::vector<uint8_t>& wrong, Tally& t,
                     Toy* keep = nullptr, std::vector<uint8_t>* ok_out = nullptr) {
    Toy toy{k, n, budget, W};
    toy.term.assign(k, 0);
    size_t b = 0;
    for (size_t i = 0; i < k; i++)
        if (wrong[i]) {
            b++;
            const uint64_t rho = signed_w ? (uint64_t)1 << i : i + 1;
            toy.term[i] = signed_w && (i & 1) ? P - rho : rho;
        }
    std::vector<uint8_t> ok(k, 1);
    const uint64_t root = toy.D(0, k);
    if (k == 1) {
        ok[0] = root == 0;  // the exact path
    } else if (root != 0) {
        toy.cur.assign(1, root);
        if (bisect_descend(k, n, budget, W, toy, ok.data())) t.bad_verdict++;
    }
    t.cases++;
    for (size_t i = 0; i < k; i++)
        if (ok[i] != !wrong[i]) {
            t.bad_verdict++;
            break;
        }
    if (toy.rows_total != failing_nodes(wrong, 0, k)) t.bad_rows++;
    const size_t bound = std::min(k - 1, b * ceil_lg(k));
    if (toy.rows_total > bound) t.over_bound++;
    if (toy.levels.size() > ceil_lg(k)) t.deep++;
    t.bad_group += toy.bad_group;
    t.bad_defect += toy.bad_defect;
    if (ok_out) *ok_out = ok;
    if (keep) *keep = toy;
}

static void print_tally(const Tally& t) {
    printf("{\"cases\": %llu, \"bad_verdict\": %llu, \"bad_rows\": %llu, \"over_bound\": %llu, \"bad_group\": %llu, "
           "\"bad_defect\": %llu, \"deep\": %llu}\n",
           t.cases, t.bad_verdict, t.bad_rows, t.over_bound, t.bad_group, t.bad_defect, t.deep);
}

int main() {
    std::string line;
    char buf[4096];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string cmd;
        size_t k = 0, n = 0, budget = 0;
        int W = 0;
        if (!(in >> cmd >> k >> n >> budget >> W) || k < 1) {
            fprintf(stderr, "bad command: %s", buf);
            return 2;
        }
        if (cmd == "sweep") {
            std::string weights;
            in >> weights;
            if (k > 20 || (weights != "inc" && weights != "signed")) return 2;
            Tally t;
            std::vector<uint8_t> wrong(k);
            for (uint32_t mask = 0; mask < ((uint32_t)1 << k); mask++) {
                for (size_t i = 0; i < k; i++) wrong[i] = (mask >> i) & 1;
                run_case(k, n, budget, W, weights == "signed", wrong, t);
            }
            print_tally(t);
        } else if (cmd == "random") {
            size_t count = 0;
            uint64_t seed = 0;
            in >> count >> seed;
            Tally t;
            std::vector<uint8_t> wrong(k);
            uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
            auto rnd = [&]() {  // xorshift64*
                x ^= x >> 12, x ^= x << 25, x ^= x >> 27;
                return x * 0x2545F4914F6CDD1Dull;
            };
            for (size_t c = 0; c < count; c++) {
                // densities 1 / k .. 1: the first cases are single wrong instances, the last one is all of them
                const uint64_t per = c + 1 == count ? 1 : std::max<uint64_t>(1, k >> (c % 13));
                bool any = false;
                for (size_t i = 0; i < k; i++) any |= (wrong[i] = (per == 1 || rnd() % per == 0));
                if (!any) wrong[rnd() % k] = 1;
                run_case(k, n, budget, W, false, wrong, t);
            }
            print_tally(t);
        } else if (cmd == "trace") {
            std::vector<uint8_t> wrong(k, 0), ok;
            size_t i;
            while (in >> i)
                if (i < k) wrong[i] = 1;
            Tally t;
            Toy toy{};
            run_case(k, n, budget, W, false, wrong, t, &toy, &ok);
            printf("{\"ok\": [");
            for (size_t j = 0; j < k; j++) printf("%s%d", j ? ", " : "", ok[j]);
            printf("], \"rows\": %zu, \"levels\": [", toy.rows_total);
            for (size_t l = 0; l < toy.levels.size(); l++) {
                printf("%s{\"nodes\": [", l ? ", " : "");
                for (size_t s = 0; s < toy.levels[l].size(); s++) {
                    const BisectNode& nd = toy.levels[l][s];
                    printf("%s[%u, %u, %u, %u]", s ? ", " : "", nd.lo, nd.mid, nd.hi, nd.src);
                }
                printf("], \"groups\": [");
                for (size_t q = 0; q < toy.groups[l].size(); q++) printf("%s%zu", q ? ", " : "", toy.groups[l][q]);
                printf("]}");
            }
            printf("], \"clean\": %s}\n", t.bad_verdict + t.bad_rows + t.over_bound + t.bad_group + t.bad_defect + t.deep ? "false" : "true");
        } else {
            fprintf(stderr, "bad command: %s", buf);
            return 2;
        }
    }
    return 0;
}
