// Stand-alone driver of halo_amd/csrc/wire_plan.hpp for tests/test_wire_plan.py (host compiler only).
// stdin: one case per line, "<hex bytes or -> <vec_prefix 0|1> <max_k>"; stdout: one JSON object per case.
// Every case is walked in a heap block of exactly its length, so a read past the end is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "wire_plan.hpp"

static int nib(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

int main() {
    std::string hex;
    int vec;
    size_t max_k;
    while (std::cin >> hex >> vec >> max_k) {
        if (hex == "-") hex.clear();
        const size_t len = hex.size() / 2;
        uint8_t* buf = (uint8_t*)malloc(len ? len : 1);
        for (size_t i = 0; i < len; i++) buf[i] = (uint8_t)(nib(hex[2 * i]) << 4 | nib(hex[2 * i + 1]));
        std::vector<halo::WireInstance> out(max_k);
        size_t k = 0, bad = 0;
        const int rc = halo::wire_walk(buf, len, vec != 0, max_k, out.data(), &k, &bad);
        printf("{\"status\": %d, \"message\": \"%s\", \"k\": %zu, \"bad\": %zu, \"instances\": [", rc,
               halo::wire_status_message(rc), k, bad);
        for (size_t i = 0; i < k; i++)
            printf("%s[%llu, %llu, %llu, %d]", i ? ", " : "", (unsigned long long)out[i].offset,
                   (unsigned long long)out[i].end, (unsigned long long)out[i].d, (int)out[i].hiding);
        printf("]}\n");
        free(buf);
    }
    return 0;
}
