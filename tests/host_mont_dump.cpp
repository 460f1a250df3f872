// Prints what halo_amd/csrc/host_mont.hpp computes, one line of space-separated 64-bit words (hex, least
// significant first) per command line read from stdin (tests/test_host_mont.py).  Built by the host
// C++ compiler alone: the header is free of HIP.  A value is 64 hex digits, most significant first.
//   w1 <fp|fq> <X> <Y> <ZZ> <ZZZ>            host_xyzz_to_wrapped_t: 8 words (x, y)
//   w2 <fp|fq> <k> <X Y ZZ ZZZ> * k          host_xyzz_to_wrapped2_t (k <= 16): 8 k words
//   inv <fp|fq> <a>                          host_scalar_inverse_t: "0", or "1" and 4 words
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "host_mont.hpp"

using namespace halo;

static bool read_value(uint64_t* w) {  // 4 words, least significant first
    std::string hex;
    if (!(std::cin >> hex) || hex.size() != 64) return false;
    for (int q = 0; q < 4; q++) w[q] = strtoull(hex.substr(16 * (3 - q), 16).c_str(), nullptr, 16);
    return true;
}

static void print_words(const uint64_t* w, int n) {
    for (int i = 0; i < n; i++) printf("%s%016" PRIx64, i ? " " : "", w[i]);
    printf("\n");
}

int main() {
    std::string mode, field;
    while (std::cin >> mode >> field) {
        const bool fp = field == "fp";
        if (!fp && field != "fq") {
            fprintf(stderr, "bad field: %s\n", field.c_str());
            return 2;
        }
        if (mode == "w1") {
            uint64_t in[16], out[8];
            for (int c = 0; c < 4; c++)
                if (!read_value(in + 4 * c)) return 2;
            for (auto& o : out) o = 0xa5a5a5a5a5a5a5a5ull;
            if (fp)
                host_xyzz_to_wrapped_t<FpCfg>(in, out);
            else
                host_xyzz_to_wrapped_t<FqCfg>(in, out);
            print_words(out, 8);
        } else if (mode == "w2") {
            int k = 0;
            if (!(std::cin >> k) || k < 1 || k > 16) {
                fprintf(stderr, "bad batch size\n");
                return 2;
            }
            uint64_t in[16][16], out[16][8];
            const void* src[16];
            void* dst[16];
            for (int i = 0; i < k; i++) {
                for (int c = 0; c < 4; c++)
                    if (!read_value(in[i] + 4 * c)) return 2;
                for (auto& o : out[i]) o = 0xa5a5a5a5a5a5a5a5ull;
                src[i] = in[i];
                dst[i] = out[i];
            }
            if (fp)
                host_xyzz_to_wrapped2_t<FpCfg>(src, dst, k);
            else
                host_xyzz_to_wrapped2_t<FqCfg>(src, dst, k);
            print_words(&out[0][0], 8 * k);
        } else if (mode == "inv") {
            uint64_t a[4], out[4] = {0, 0, 0, 0};
            if (!read_value(a)) return 2;
            const bool ok = fp ? host_scalar_inverse_t<FpCfg>(a, out) : host_scalar_inverse_t<FqCfg>(a, out);
            if (ok) {
                printf("1 ");
                print_words(out, 4);
            } else {
                printf("0\n");
            }
        } else {
            fprintf(stderr, "bad mode: %s\n", mode.c_str());
            return 2;
        }
    }
    return 0;
}
