// Prints the sort entries of ark scalars recoded in one step and in two (halo_amd/csrc/digits_core.hpp),
// for tests/test_digits_two_step.py.  Built by the host C++ compiler alone: digits_core.hpp and
// host_mont.hpp are free of HIP.  One command line read from stdin per scalar:
//   <fp|fq> <mode> <c> <W> <64 hex digits: the ark (Montgomery, R = 2^256) scalar, most significant first>
// modes as tests/digits_core_dump.cpp: rt, rtu (W <= 16), c16, c17.
// Three output lines per command (hex words):
//   the one-step entries: the canonical scalar folded here with 64-bit host arithmetic (min(s, p - s) and
//     the flip held in a variable, as the device wrapper did before the split), then signed_digit_entries;
//   the 8 stored words of step one (digits_fold: the folded integer, the fold's sign in bit 255), least
//     significant first;
//   the two-step entries: those 8 words copied through memory, digits_unfold, signed_digit_entries.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "digits_core.hpp"
#include "host_mont.hpp"

using namespace halo;

static int entries(const char* mode, const uint32_t (&w8)[8], uint32_t flip, int c, int W, uint32_t* out) {
    int n = 0;
    auto put = [&](int w, uint32_t e) {
        if (w != n || n >= 32) {  // in order, each window once
            n = 33;
            return;
        }
        out[n++] = e;
    };
    if (!strcmp(mode, "rt"))
        signed_digit_entries<0, 0>(w8, flip, c, W, put);
    else if (!strcmp(mode, "rtu") && W <= 16)
        signed_digit_entries<0, 16>(w8, flip, c, W, put);
    else if (!strcmp(mode, "c16"))
        signed_digit_entries<16, 16>(w8, flip, c, W, put);
    else if (!strcmp(mode, "c17"))
        signed_digit_entries<17, 0>(w8, flip, c, W, put);
    else
        return -1;
    return n;
}

static void print_words(const uint32_t* w, int n) {
    for (int i = 0; i < n; i++) printf("%s%08" PRIx32, i ? " " : "", w[i]);
    printf("\n");
}

template <class S>
static int one(const char* mode, int c, int W, const char* hex) {
    const HostMont M(S::MODULUS64);
    uint64_t ark[4], s[4];
    for (int q = 0; q < 4; q++) {
        char part[17];
        memcpy(part, hex + 16 * (3 - q), 16);
        part[16] = 0;
        ark[q] = strtoull(part, nullptr, 16);
    }
    const uint64_t unit[4] = {1, 0, 0, 0};
    M.mul(ark, unit, s);  // s R R^-1: the canonical scalar
    // one step: t = p - s with 64-bit words, taken when t < s
    uint64_t t[4];
    unsigned __int128 b = 0;
    for (int i = 0; i < 4; i++) {
        const unsigned __int128 d = (unsigned __int128)M.p[i] - s[i] - b;
        t[i] = (uint64_t)d;
        b = (d >> 64) & 1;
    }
    bool lt = false;
    for (int i = 3; i >= 0; i--)
        if (t[i] != s[i]) {
            lt = t[i] < s[i];
            break;
        }
    uint32_t a8[8], w8[8], out[34];
    for (int q = 0; q < 8; q++) a8[q] = (uint32_t)((lt ? t : s)[q >> 1] >> (32 * (q & 1)));
    int n = entries(mode, a8, lt ? 0x80000000u : 0u, c, W, out);
    if (n < 0 || n > 32) return 3;
    print_words(out, n);
    // two steps, the stored words through memory
    for (int q = 0; q < 8; q++) w8[q] = (uint32_t)(s[q >> 1] >> (32 * (q & 1)));
    digits_fold(w8, M.p32);
    unsigned char stored[32];
    memcpy(stored, w8, 32);
    print_words(w8, 8);
    uint32_t r8[8];
    memcpy(r8, stored, 32);
    const uint32_t flip = digits_unfold(r8);
    n = entries(mode, r8, flip, c, W, out);
    if (n < 0 || n > 32) return 3;
    print_words(out, n);
    return 0;
}

int main() {
    char line[512], field[8], mode[8], hex[80];
    while (fgets(line, sizeof line, stdin)) {
        int c = 0, W = 0;
        if (sscanf(line, "%7s %7s %d %d %79s", field, mode, &c, &W, hex) != 5 || strlen(hex) != 64 || c < 1 || c > 31 ||
            W < 1 || W > 32) {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
        int rc;
        if (!strcmp(field, "fp"))
            rc = one<FpCfg>(mode, c, W, hex);
        else if (!strcmp(field, "fq"))
            rc = one<FqCfg>(mode, c, W, hex);
        else
            rc = 2;
        if (rc) {
            fprintf(stderr, "failed (%d): %s", rc, line);
            return rc;
        }
    }
    return 0;
}
