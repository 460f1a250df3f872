// Prints what halo_amd/csrc/msm_plan.hpp computes, one JSON object per command line read from stdin
// (tests/test_msm_plan.py).  Built by the host C++ compiler alone: the header is free of HIP.
//   plan E NB SW B c num_cu W SN     the whole MsmPlan
//   fuse P n W B key_bits            msm_fuse_first_pass
//   bits n                           msm_window_bits, msm_shifted_window_bits
//   windows c                        msm_windows
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "msm_plan.hpp"

using namespace halo;

int main() {
    char line[256], cmd[16];
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[8] = {};
        const int k = sscanf(line, "%15s %llu %llu %llu %llu %llu %llu %llu %llu", cmd, a, a + 1, a + 2, a + 3, a + 4,
                             a + 5, a + 6, a + 7);
        if (k < 2) continue;
        if (!strcmp(cmd, "plan") && k == 9) {
            const MsmPlan p = msm_plan(a[0], a[1], (int)a[2], (uint32_t)a[3], (int)a[4], (int)a[5], (int)a[6], a[7]);
#define U(f) printf("\"" #f "\": %llu, ", (unsigned long long)p.f)
            printf("{");
            U(c), U(W), U(SW), U(B), U(L), U(logL), U(H), U(logH), U(NT), U(key_bits), U(K), U(SN), U(NB), U(E);
            U(nchunks), U(ng1), U(ng2), U(off_first), U(off_last), U(off_g1), U(off_g2);
            U(digits_bytes), U(bstart_bytes), U(partials_bytes), U(bucket_sums_bytes), U(rows_bytes), U(cols_bytes);
            U(terms_bytes);
#undef U
            printf("\"window_sums_bytes\": [%zu, %zu, %zu]}\n", p.window_sums_bytes(0), p.window_sums_bytes(1),
                   p.window_sums_bytes(p.SW));
        } else if (!strcmp(cmd, "fuse") && k == 6) {
            printf("{\"fuse\": %s}\n",
                   msm_fuse_first_pass((int)a[0], a[1], (int)a[2], (uint32_t)a[3], (uint32_t)a[4]) ? "true" : "false");
        } else if (!strcmp(cmd, "bits") && k == 2) {
            printf("{\"window_bits\": %d, \"shifted_window_bits\": %d}\n", msm_window_bits(a[0]),
                   msm_shifted_window_bits(a[0]));
        } else if (!strcmp(cmd, "windows") && k == 2) {
            printf("{\"windows\": %d}\n", msm_windows((int)a[0]));
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
    }
    return 0;
}
