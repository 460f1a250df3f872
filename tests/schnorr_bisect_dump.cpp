// Runs the descent of halo_amd/csrc/schnorr_bisect.hpp against a toy additive group (tests/test_schnorr_bisect.py).
// Built by the host C++ compiler alone: the header is free of HIP.  The stand-in for the device works in Z / p,
// p = 2^61 - 1: D(S) = sum_{i in S, i wrong} rho_i mod p with rho_i = i + 1, so that no sum over a nonempty set of
// wrong items vanishes; its ladder over a slice is exact.
// One command per line on stdin, one JSON object per command on stdout:
//   sweep k L c               every subset of the k items as the wrong ones
//   random k L c count seed   `count` random subsets, their density varying from one wrong item to all
//   trace k L c i j ...       one descent with the wrong items i j ..., level by level
// L, c: the leaf and budget rules' parameters (SigBisectRules).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "schnorr_bisect.hpp"

using namespace halo;

static const uint64_t P = ((uint64_t)1 << 61) - 1;
static uint64_t addp(uint64_t a, uint64_t b) { return (a + b) % P; }
static uint64_t subp(uint64_t a, uint64_t b) { return (a + P - b) % P; }

struct Toy {  // the Eval of sig_bisect_descend
    size_t k;
    std::vector<uint64_t> term;  // rho_i, 0 for a good item
    std::vector<uint8_t>* ok;    // the verdict bytes: split and ladder clear them, as the device's kernels do
    std::vector<uint64_t> cur, next, left;
    std::vector<uint8_t> have;
    // what the test reads
    std::vector<std::vector<BisectNode>> levels;
    std::vector<std::pair<uint32_t, uint32_t>> ladders;
    size_t passes_total = 0, bad_defect = 0, bad_order = 0;

    uint64_t D(size_t lo, size_t hi) const {
        uint64_t s = 0;
        for (size_t i = lo; i < hi; i++) s = addp(s, term[i]);
        return s;
    }
    int passes(const BisectNode* level, size_t f) {
        levels.emplace_back(level, level + f);
        left.assign(f, 0);
        have.assign(f, 0);
        for (size_t s = 0; s < f; s++) {
            const BisectNode& nd = level[s];
            if (nd.mid != nd.lo + (nd.hi - nd.lo) / 2 || nd.hi - nd.lo < 2 || nd.hi > k) bad_defect++;  // the split rule
            left[s] = D(nd.lo, nd.mid);
            have[s] = 1;
        }
        passes_total += f;
        return 0;
    }
    int split(const BisectNode* level, size_t f, uint8_t* flags) {
        if (have.size() != f) bad_order++;  // a pass over this level came first
        next.assign(2 * f, 0);
        for (size_t s = 0; s < f; s++) {
            if (s >= have.size() || !have[s]) {
                bad_order++;
                continue;
            }
            const BisectNode& nd = level[s];
            const uint64_t Dn = nd.src < cur.size() ? cur[nd.src] : 0;
            if (Dn != D(nd.lo, nd.hi) || Dn == 0) bad_defect++;  // src names the node's own defect, a failing one
            next[2 * s] = left[s];
            next[2 * s + 1] = subp(Dn, left[s]);
            flags[2 * s] = next[2 * s] != 0;
            flags[2 * s + 1] = next[2 * s + 1] != 0;
            if (flags[2 * s] && nd.mid - nd.lo == 1) (*ok)[nd.lo] = 0;
            if (flags[2 * s + 1] && nd.hi - nd.mid == 1) (*ok)[nd.mid] = 0;
        }
        have.clear();
        cur.swap(next);
        return 0;
    }
    int ladder(uint32_t lo, uint32_t hi) {
        ladders.emplace_back(lo, hi);
        for (size_t i = lo; i < hi && i < k; i++) (*ok)[i] = term[i] == 0;
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

// [lo, hi) is a node of the tree over [0, k)
static bool is_node(size_t lo, size_t hi, size_t k) {
    size_t a = 0, b = k;
    while (true) {
        if (a == lo && b == hi) return true;
        if (b - a < 2) return false;
        const size_t mid = a + (b - a) / 2;
        if (hi <= mid)
            b = mid;
        else if (lo >= mid)
            a = mid;
        else
            return false;
    }
}

struct Tally {
    unsigned long long cases = 0, bad_verdict = 0, over_budget = 0, bad_ladder = 0, bad_full = 0, bad_root = 0, bad_defect = 0;
};

// One batch: the combined root pass decides whether the descent runs at all, as sig_bisect_device's callers do.
static void run_case(size_t k, size_t L, size_t c, const std::vector<uint8_t>& wrong, Tally& t, Toy* keep = nullptr,
                     std::vector<uint8_t>* ok_out = nullptr) {
    std::vector<uint8_t> ok(k, 1);
    Toy toy{k};
    toy.ok = &ok;
    toy.term.assign(k, 0);
    size_t b = 0;
    for (size_t i = 0; i < k; i++)
        if (wrong[i]) {
            b++;
            toy.term[i] = i + 1;
        }
    const uint64_t root = toy.D(0, k);
    if (root != 0) {
        toy.cur.assign(1, root);
        std::vector<uint8_t> host_ok(k, 1);
        if (sig_bisect_descend(k, SigBisectRules{L, c}, toy, host_ok.data())) t.bad_verdict++;
        if (k == 1) ok[0] = host_ok[0];  // no kernel runs for a batch of one: the root pass's own byte stands
        for (size_t i = 0; i < k; i++)
            if (!host_ok[i] && ok[i]) t.bad_verdict++;  // the header's single-item verdicts are the split's
    }
    t.cases++;
    for (size_t i = 0; i < k; i++)
        if (ok[i] != !wrong[i]) {
            t.bad_verdict++;
            break;
        }
    if (toy.passes_total * c > k) t.over_budget++;
    // the ladder slices: inside [0, k), nodes of the tree, failing, of two items or more, pairwise disjoint
    std::vector<uint8_t> seen(k, 0);
    for (const auto& sl : toy.ladders) {
        if (sl.first >= sl.second || sl.second > k || sl.second - sl.first < 2 || !is_node(sl.first, sl.second, k)) {
            t.bad_ladder++;
            continue;
        }
        if (toy.D(sl.first, sl.second) == 0) t.bad_ladder++;
        for (size_t i = sl.first; i < sl.second; i++) {
            if (seen[i]) t.bad_ladder++;
            seen[i] = 1;
        }
    }
    if (L == 1 && c == 1) {  // the full descent
        if (!toy.ladders.empty()) t.bad_full++;
        if (toy.passes_total != failing_nodes(wrong, 0, k)) t.bad_full++;
        if (toy.passes_total > std::min(k - 1, b * ceil_lg(k))) t.bad_full++;
        if (toy.levels.size() > ceil_lg(k)) t.bad_full++;
    }
    if (root != 0 && (k < c || k <= L)) {  // the root goes straight to the ladder; a batch of one needs none
        if (toy.passes_total != 0) t.bad_root++;
        if (k == 1 ? !toy.ladders.empty()
                   : toy.ladders.size() != 1 || toy.ladders[0] != std::make_pair((uint32_t)0, (uint32_t)k))
            t.bad_root++;
    }
    if (root == 0 && (toy.passes_total || !toy.ladders.empty())) t.bad_root++;
    t.bad_defect += toy.bad_defect + toy.bad_order;
    if (ok_out) *ok_out = ok;
    if (keep) *keep = toy;
}

static void print_tally(const Tally& t) {
    printf("{\"cases\": %llu, \"bad_verdict\": %llu, \"over_budget\": %llu, \"bad_ladder\": %llu, \"bad_full\": %llu, "
           "\"bad_root\": %llu, \"bad_defect\": %llu}\n",
           t.cases, t.bad_verdict, t.over_budget, t.bad_ladder, t.bad_full, t.bad_root, t.bad_defect);
}

int main() {
    char buf[65536];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string cmd;
        size_t k = 0, L = 0, c = 0;
        if (!(in >> cmd >> k >> L >> c) || k < 1 || L < 1 || c < 1) {
            fprintf(stderr, "bad command: %s", buf);
            return 2;
        }
        if (cmd == "sweep") {
            if (k > 20) return 2;
            Tally t;
            std::vector<uint8_t> wrong(k);
            for (uint32_t mask = 0; mask < ((uint32_t)1 << k); mask++) {
                for (size_t i = 0; i < k; i++) wrong[i] = (mask >> i) & 1;
                run_case(k, L, c, wrong, t);
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
            for (size_t n = 0; n < count; n++) {
                // densities 1 / k .. 1: the first cases are single wrong items, the last one is all of them
                const uint64_t per = n + 1 == count ? 1 : std::max<uint64_t>(1, k >> (n % 13));
                bool any = false;
                for (size_t i = 0; i < k; i++) any |= (wrong[i] = (per == 1 || rnd() % per == 0));
                if (!any) wrong[rnd() % k] = 1;
                run_case(k, L, c, wrong, t);
            }
            print_tally(t);
        } else if (cmd == "trace") {
            std::vector<uint8_t> wrong(k, 0), ok;
            size_t i;
            while (in >> i)
                if (i < k) wrong[i] = 1;
            Tally t;
            Toy toy{};
            run_case(k, L, c, wrong, t, &toy, &ok);
            printf("{\"ok\": [");
            for (size_t j = 0; j < k; j++) printf("%s%d", j ? ", " : "", ok[j]);
            printf("], \"passes\": %zu, \"levels\": [", toy.passes_total);
            for (size_t l = 0; l < toy.levels.size(); l++) {
                printf("%s[", l ? ", " : "");
                for (size_t s = 0; s < toy.levels[l].size(); s++) {
                    const BisectNode& nd = toy.levels[l][s];
                    printf("%s[%u, %u, %u, %u]", s ? ", " : "", nd.lo, nd.mid, nd.hi, nd.src);
                }
                printf("]");
            }
            printf("], \"ladders\": [");
            for (size_t q = 0; q < toy.ladders.size(); q++)
                printf("%s[%u, %u]", q ? ", " : "", toy.ladders[q].first, toy.ladders[q].second);
            printf("], \"clean\": %s}\n",
                   t.bad_verdict + t.over_budget + t.bad_ladder + t.bad_full + t.bad_root + t.bad_defect ? "false" : "true");
        } else {
            fprintf(stderr, "bad command: %s", buf);
            return 2;
        }
    }
    return 0;
}
