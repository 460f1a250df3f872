// Walks halo_amd/csrc/acc_entries.hpp's cursor over every chunk of a sorted array the way acc_chunk
// (msm.hip) does, for the chunk lengths and counts given on the command line (tests/test_acc_entries.py
// builds this with the address and undefined-behaviour sanitizers and runs it as a program).
//   acc_entries_walk K...      for every K: every count 0 .. 3 K + 5
//   acc_entries_walk old K...  the same with the arrays at max(count, 1) * 4 bytes, the reservation before
//                              the cursor: the control that shows the sanitizer sees an over-read
// The arrays are allocated at exactly acc_entries_bytes(count), the drivers' reservation for E = count
// entries (the tightest: E >= count), so a load past it is the sanitizer's to report.  Prints one line
// "K <K> counts <n> chunks <n> entries <n> loads <n>" per K and exits non-zero on the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "acc_entries.hpp"

using namespace halo;

static std::vector<uint32_t> g_loads;  // the e4 of every 16-byte load of the key array, in order
static const uint32_t* g_keys;
static const uint32_t* g_vals;
static uint64_t g_val_loads;
static bool g_old_size;

struct CountingLoad {
    static AccQuad quad(const uint32_t* a, uint32_t e4) {
        if (a == g_keys) g_loads.push_back(e4);
        else if (a == g_vals) g_val_loads++;
        else {
            std::printf("load from an array that is neither keys nor vals\n");
            std::exit(1);
        }
        return AccQuadLoad::quad(a, e4);
    }
};

static uint32_t key_of(uint32_t i) { return i * 2654435761u + 12345u; }
static uint32_t val_of(uint32_t i) { return (i * 40503u) ^ 0x80000000u ^ (i << 17); }

#define FAIL(...)                 \
    do {                          \
        std::printf(__VA_ARGS__); \
        std::printf("\n");        \
        return 1;                 \
    } while (0)

static int walk(uint32_t K, uint32_t cnt, uint64_t& chunks, uint64_t& entries, uint64_t& loads) {
    const size_t bytes = acc_entries_bytes(cnt);
    if (bytes % 16 || bytes < 4 * (size_t)(cnt ? cnt : 1) || bytes >= 4 * (size_t)(cnt ? cnt : 1) + 16)
        FAIL("acc_entries_bytes(%u) = %zu", cnt, bytes);
    const size_t alloc = g_old_size ? 4 * (size_t)(cnt ? cnt : 1) : bytes;
    uint32_t *keys = nullptr, *vals = nullptr;
    if (posix_memalign((void**)&keys, 16, alloc) || posix_memalign((void**)&vals, 16, alloc))
        FAIL("allocation of %zu bytes", alloc);
    for (uint32_t i = 0; i < alloc / 4; i++) {  // past the count: readable, never to be handed out
        keys[i] = i < cnt ? key_of(i) : 0xdeadbeefu;
        vals[i] = i < cnt ? val_of(i) : 0xdeadbeefu;
    }
    g_keys = keys;
    g_vals = vals;
    for (size_t t = 0; t * K < cnt; t++) {
        const size_t beg = t * K;
        const uint32_t end = (uint32_t)(beg + K < cnt ? beg + K : cnt);
        g_loads.clear();
        g_val_loads = 0;
        std::vector<uint32_t> want;  // chunk start, then every multiple of four inside (beg, end)
        AccEntries<CountingLoad> ent(keys, vals);
        ent.start((uint32_t)beg);
        want.push_back((uint32_t)beg & ~3u);
        for (uint32_t e = (uint32_t)beg; e < end; e++) {
            if (e != beg) {
                ent.next(e);
                if ((e & 3u) == 0) want.push_back(e);
            }
            // acc_chunk reads the key (twice for the first entry: cur and the step's) and then the value
            if (ent.key(e) != key_of(e) || ent.key(e) != keys[e])
                FAIL("K %u count %u chunk %zu: key(%u) = %08x, want %08x", K, cnt, t, e, ent.key(e), key_of(e));
            if (ent.val(e) != val_of(e) || ent.val(e) != vals[e])
                FAIL("K %u count %u chunk %zu: val(%u) = %08x, want %08x", K, cnt, t, e, ent.val(e), val_of(e));
        }
        if (g_loads != want || g_val_loads != want.size()) {
            std::printf("K %u count %u chunk %zu [%zu, %u): key loads at", K, cnt, t, beg, end);
            for (uint32_t x : g_loads) std::printf(" %u", x);
            std::printf(", want");
            for (uint32_t x : want) std::printf(" %u", x);
            FAIL("; %llu value loads", (unsigned long long)g_val_loads);
        }
        chunks++;
        entries += end - beg;
        loads += want.size();
    }
    std::free(keys);
    std::free(vals);
    return 0;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; a++) {
        if (a == 1 && argv[a][0] == 'o') {
            g_old_size = true;
            continue;
        }
        const uint32_t K = (uint32_t)std::strtoul(argv[a], nullptr, 10);
        if (!K) FAIL("chunk length %s", argv[a]);
        uint64_t chunks = 0, entries = 0, loads = 0;
        for (uint32_t cnt = 0; cnt <= 3 * K + 5; cnt++)
            if (walk(K, cnt, chunks, entries, loads)) return 1;
        std::printf("K %u counts %u chunks %llu entries %llu loads %llu\n", K, 3 * K + 6, (unsigned long long)chunks,
                    (unsigned long long)entries, (unsigned long long)loads);
    }
    return 0;
}
