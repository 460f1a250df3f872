// Prints what halo_amd/csrc/host_mont.hpp computes, one line of space-separated 64-bit words (hex, least
// significant first) per command line read from stdin (tests/test_host_mont.py).  Built by the host
// C++ compiler alone: the header is free of HIP.  A value is 64 hex digits, most significant first.
//   w1 <fp|fq> <X> <Y> <ZZ> <ZZZ>            host_xyzz_to_wrapped_t: 8 words (x, y)
//   w2 <fp|fq> <k> <X Y ZZ ZZZ> * k          host_xyzz_to_wrapped2_t (k <= 16): 8 k words
//   inv <fp|fq> <a>                          host_scalar_inverse_t: "0", or "1" and 4 words
// and of host_scalar.hpp, for the curve whose scalar field is named (fp: Pallas, fq: Vesta):
//   below <fp|fq> <n> <a> * n                scalar_below: bit i = value i alone, then the span form over all n
//   rho <fp|fq> <n> <a> * n                  check_rho: "<code>|<message>" (n = -1: a null rho, k = 3)
//   arith <fp|fq> <a> <b>                    HostScalar add, sub, neg(a): 12 words
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "host_mont.hpp"
#include "host_scalar.hpp"

using namespace halo;

// check_rho reports through the library's set_error; here the message is kept for printing
static std::string g_error;
int halo::set_error(int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
    return code;
}

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
        const int curve = fp ? HALO_PALLAS : HALO_VESTA;  // the curve whose scalar field it is (host_scalar.hpp)
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
        } else if (mode == "below") {
            int n = 0;
            if (!(std::cin >> n) || n < 0 || n > 16) return 2;
            halo_fe_t x[16];
            int each = 0;
            for (int i = 0; i < n; i++) {
                if (!read_value(x[i].l)) return 2;
                each |= (scalar_below(curve, x[i]) ? 1 : 0) << i;
            }
            printf("%x %x\n", each, scalar_below(curve, n ? x : nullptr, (size_t)n) ? 1 : 0);
        } else if (mode == "rho") {
            int n = 0;
            if (!(std::cin >> n) || n < -1 || n > 16) return 2;  // -1: a null rho
            halo_fe_t x[16];
            for (int i = 0; i < n; i++)
                if (!read_value(x[i].l)) return 2;
            g_error.clear();
            const int rc = check_rho("the_call", curve, n < 0 ? nullptr : x, n < 0 ? 3 : (size_t)n);
            printf("%d|%s\n", rc, g_error.c_str());
        } else if (mode == "arith") {
            uint64_t a[4], b[4], out[3][4];
            if (!read_value(a) || !read_value(b)) return 2;
            const HostScalar S{scalar_mont(curve)};
            S.add(a, b, out[0]);
            S.sub(a, b, out[1]);
            S.neg(a, out[2]);
            print_words(&out[0][0], 12);
        } else {
            fprintf(stderr, "bad mode: %s\n", mode.c_str());
            return 2;
        }
    }
    return 0;
}
