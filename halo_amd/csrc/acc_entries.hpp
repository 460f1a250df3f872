// k_acc's reads of the sorted entries (msm.hip acc_chunk): a cursor that holds, for the key array and
// the value array, the 16-byte-aligned group of four entries around the current entry.  Free of HIP
// types, so a plain C++17 compiler builds it (tests/test_acc_entries.py); hipcc compiles the same text
// for the device.
//
// Why: thread t reads the entries [t K, t K + K) one after the other, so the lanes of a wave are K * 4
// bytes apart and a 4-byte load per entry asks for up to 64 lines of which it uses 4 bytes each -- and
// asks for the same lines again for the chunk's next entries.  One 16-byte load per four entries makes
// a quarter of those requests.
//
// The group of entry e is the entries [e & ~3, (e & ~3) + 4).  It may begin before the chunk (always
// inside the array) and end up to three entries past the last one, so the arrays' owners reserve
// acc_entries_bytes(E) bytes, a whole number of groups, for E entries.  Entries past the device count
// are loaded and never handed out.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HALO_ACC_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define HALO_ACC_FN inline
#endif

namespace halo {

constexpr uint32_t ACC_GROUP = 4;  // entries per load

// the reservation of an array of E sorted entries (keys or values) that k_acc reads
constexpr size_t acc_entries_bytes(size_t E) {
    return ((E > 0 ? E : 1) + ACC_GROUP - 1) / ACC_GROUP * (ACC_GROUP * sizeof(uint32_t));
}

struct alignas(16) AccQuad {
    uint32_t x, y, z, w;
};

// component r (0..3) by selects: no run-time index into the registers
HALO_ACC_FN uint32_t acc_quad_pick(const AccQuad& q, uint32_t r) {
    const uint32_t lo = (r & 1u) ? q.y : q.x;
    const uint32_t hi = (r & 1u) ? q.w : q.z;
    return (r & 2u) ? hi : lo;
}

// the plain 16-byte load (global_load_dwordx4 on the device); e4 is a multiple of four
struct AccQuadLoad {
    static HALO_ACC_FN AccQuad quad(const uint32_t* a, uint32_t e4) { return *reinterpret_cast<const AccQuad*>(a + e4); }
};

// Use: start(beg), then for e = beg, beg + 1, ...: next(e) before the first read of every e > beg, and
// key(e) / val(e) any number of times.  Both arrays are 16-byte aligned.  Load: the 16-byte load (the host
// test counts them through it).
template <class Load = AccQuadLoad>
struct AccEntries {
    const uint32_t* keys;
    const uint32_t* vals;
    AccQuad k, v;

    HALO_ACC_FN AccEntries(const uint32_t* keys_, const uint32_t* vals_) : keys(keys_), vals(vals_), k{}, v{} {}
    HALO_ACC_FN void load(uint32_t e4) {
        k = Load::quad(keys, e4);
        v = Load::quad(vals, e4);
    }
    // the chunk's first entry
    HALO_ACC_FN void start(uint32_t beg) { load(beg & ~(ACC_GROUP - 1u)); }
    // e is the entry after the previous one: a new group where e is a multiple of four (uniform over the
    // wave when K is a multiple of four, a load in some of its lanes otherwise)
    HALO_ACC_FN void next(uint32_t e) {
        if ((e & (ACC_GROUP - 1u)) == 0) load(e);
    }
    HALO_ACC_FN uint32_t key(uint32_t e) const { return acc_quad_pick(k, e & (ACC_GROUP - 1u)); }
    HALO_ACC_FN uint32_t val(uint32_t e) const { return acc_quad_pick(v, e & (ACC_GROUP - 1u)); }
};

}  // namespace halo
