// Prints what halo_amd/csrc/scratch_layout.hpp lays out, one line of decimal numbers per command line read from
// stdin (tests/test_scratch_layout.py).  Built by the host C++ compiler alone: the header is free of HIP.
//   layout <n> <bytes> * n     ScratchLayout: the n offsets take() returned, then total()
//   parts <n> <bytes> * n      HostParts of n rows: at(j) of each row (-1: absent), then total()
//   align <bytes>              align256
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "scratch_layout.hpp"

using namespace halo;

int main() {
    std::string mode;
    while (std::cin >> mode) {
        if (mode == "align") {
            size_t b;
            if (!(std::cin >> b)) return 2;
            printf("%zu\n", align256(b));
            continue;
        }
        size_t n;
        if (!(std::cin >> n) || n > 64) return 2;
        std::vector<size_t> bytes(n);
        for (size_t& b : bytes)
            if (!(std::cin >> b)) return 2;
        if (mode == "layout") {
            ScratchLayout lay;
            for (size_t b : bytes) printf("%zu ", lay.take(b));
            printf("%zu\n", lay.total());
        } else if (mode == "parts") {
            static const char src[1] = {0};  // the table keeps the pointer, nothing reads it here
            HostParts parts;
            for (size_t b : bytes) parts.add(b ? src : nullptr, b);
            for (size_t j = 0; j < n; j++) {
                if (parts.at(j) == HostParts::ABSENT)
                    printf("-1 ");
                else
                    printf("%zu ", parts.at(j));
            }
            printf("%zu\n", parts.total());
        } else {
            fprintf(stderr, "bad mode: %s\n", mode.c_str());
            return 2;
        }
    }
    return 0;
}
