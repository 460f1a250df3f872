// The layout of serialized pcdl Instances (ark-serialize 0.5, compressed mode) as the host walks
// it: where each instance of a byte buffer starts and ends, its degree bound and whether it hides, read from the
// lengths, `d` and the option tags alone.  No point or scalar is decoded here (wire.hip does that on the device).
// Free of HIP: standard headers only, so the host C++ compiler builds it alone (tests/wire_plan_dump.cpp,
// tests/test_wire_plan.py, also under the address and undefined-behaviour sanitizers).
//
// The input is untrusted.  Every read goes through WireCursor, which compares a wanted byte count with the bytes
// that remain BEFORE it forms an offset, and every multiplication of a length read from the buffer is replaced by a
// division of the remaining byte count, so nothing overflows and nothing past `len` is read.
//
//   Instance   C 33 | d u64 | z 32 | v 32 | Ls: u64 n, 33 n | Rs: u64 n, 33 n | U 33 | c 32
//              | tag, C_bar 33 if 1 | tag, w_prime 32 if 1            (pcdl.rs:28-34, 161-168)
#pragma once
#include <cstddef>
#include <cstdint>

namespace halo {

constexpr size_t WIRE_POINT = 33, WIRE_SCALAR = 32, WIRE_U64 = 8;

enum WireStatus {
    WIRE_OK = 0,
    WIRE_TRUNCATED = 1,      // the buffer ends inside an instance
    WIRE_LENGTH_PREFIX = 2,  // a Vec length that its items could not fit in the bytes that remain
    WIRE_ROUNDS = 3,         // Ls and Rs lengths differ from each other or from lg(d + 1)
    WIRE_NOT_POW2 = 4,       // d + 1 is not a power of two
    WIRE_TAG = 5,            // an Option tag other than 0 / 1
    WIRE_OPTION_PAIR = 6,    // one of C_bar / w_prime without the other
    WIRE_TOO_MANY = 7,       // more instances than the caller's arrays hold
    WIRE_TRAILING = 8,       // bytes after the last instance of a Vec
};

constexpr const char* wire_status_message(int s) {
    return s == WIRE_OK ? "ok"
         : s == WIRE_TRUNCATED ? "the buffer ends inside an instance"
         : s == WIRE_LENGTH_PREFIX ? "a length prefix exceeds the bytes that remain"
         : s == WIRE_ROUNDS ? "Ls and Rs must both hold lg(d + 1) points"
         : s == WIRE_NOT_POW2 ? "d + 1 is not a power of two"
         : s == WIRE_TAG ? "an option tag is neither 0 nor 1"
         : s == WIRE_OPTION_PAIR ? "C_bar and w_prime must be present together"
         : s == WIRE_TOO_MANY ? "more instances than max_k"
         : s == WIRE_TRAILING ? "bytes after the last instance"
                              : "unknown status";
}

// Byte offsets of the items of one instance of lg rounds, from its first byte.  The kernels of wire.hip read and
// write through the same table.
struct WireLayout {
    size_t C, d, z, v, ls_len, ls, rs_len, rs, U, c, tag_cbar;
};
constexpr WireLayout wire_layout(size_t lg) {
    WireLayout w{};
    w.C = 0;
    w.d = w.C + WIRE_POINT;
    w.z = w.d + WIRE_U64;
    w.v = w.z + WIRE_SCALAR;
    w.ls_len = w.v + WIRE_SCALAR;
    w.ls = w.ls_len + WIRE_U64;
    w.rs_len = w.ls + WIRE_POINT * lg;
    w.rs = w.rs_len + WIRE_U64;
    w.U = w.rs + WIRE_POINT * lg;
    w.c = w.U + WIRE_POINT;
    w.tag_cbar = w.c + WIRE_SCALAR;
    return w;
}
// plain: ... tag 0 | tag 0; hiding: ... tag 1 | C_bar | tag 1 | w_prime
constexpr size_t wire_instance_size(size_t lg, bool hiding) {
    return wire_layout(lg).tag_cbar + 2 + (hiding ? WIRE_POINT + WIRE_SCALAR : 0);
}
constexpr size_t WIRE_MIN_INSTANCE = wire_instance_size(0, false);

struct WireInstance {
    uint64_t offset, end, d;
    uint8_t hiding;
};

struct WireCursor {
    const uint8_t* buf;
    size_t len, off;
    size_t left() const { return len - off; }  // off <= len always
    // n more bytes are there: true moves past them and hands back where they began
    bool take(size_t n, size_t& at) {
        if (n > left()) return false;
        at = off;
        off += n;
        return true;
    }
    bool u64(uint64_t& x) {
        size_t at;
        if (!take(WIRE_U64, at)) return false;
        x = 0;
        for (int i = 7; i >= 0; i--) x = x << 8 | buf[at + i];
        return true;
    }
    bool byte(uint8_t& x) {
        size_t at;
        if (!take(1, at)) return false;
        x = buf[at];
        return true;
    }
};

// Steps over a Vec<Point> whose length must be lg.  A length the remaining bytes cannot hold is a truncation when
// it is the expected one and a bad prefix otherwise.
inline int wire_skip_points(WireCursor& cur, uint64_t lg) {
    uint64_t n;
    if (!cur.u64(n)) return WIRE_TRUNCATED;
    if (n > cur.left() / WIRE_POINT) return n == lg ? WIRE_TRUNCATED : WIRE_LENGTH_PREFIX;
    if (n != lg) return WIRE_ROUNDS;
    size_t at;
    cur.take((size_t)n * WIRE_POINT, at);  // fits: checked above
    return WIRE_OK;
}

inline int wire_walk_instance(WireCursor& cur, WireInstance& out) {
    size_t at;
    out.offset = cur.off;
    if (!cur.take(WIRE_POINT, at)) return WIRE_TRUNCATED;
    uint64_t d;
    if (!cur.u64(d)) return WIRE_TRUNCATED;
    if (d == UINT64_MAX || ((d + 1) & d)) return WIRE_NOT_POW2;
    uint64_t lg = 0;
    while ((uint64_t(2) << lg) <= d + 1 && lg < 63) lg++;  // d + 1 = 2^lg
    if (!cur.take(2 * WIRE_SCALAR, at)) return WIRE_TRUNCATED;
    int rc = wire_skip_points(cur, lg);
    if (rc) return rc;
    rc = wire_skip_points(cur, lg);
    if (rc) return rc;
    if (!cur.take(WIRE_POINT + WIRE_SCALAR, at)) return WIRE_TRUNCATED;
    uint8_t t_cbar, t_w;
    if (!cur.byte(t_cbar)) return WIRE_TRUNCATED;
    if (t_cbar > 1) return WIRE_TAG;
    if (t_cbar && !cur.take(WIRE_POINT, at)) return WIRE_TRUNCATED;
    if (!cur.byte(t_w)) return WIRE_TRUNCATED;
    if (t_w > 1) return WIRE_TAG;
    if (t_w != t_cbar) return WIRE_OPTION_PAIR;
    if (t_w && !cur.take(WIRE_SCALAR, at)) return WIRE_TRUNCATED;
    out.end = cur.off;
    out.d = d;
    out.hiding = t_cbar;
    return WIRE_OK;
}

// The instances of buf[0, len): with vec_prefix a Vec<Instance> (u64 count first, nothing after the last one),
// else instances until the last byte.  out holds max_k entries; *k_out the number found; *bad (may be null) the
// index of the instance a refusal is about.  Nothing is written past out[max_k - 1].
inline int wire_walk(const uint8_t* buf, size_t len, bool vec_prefix, size_t max_k, WireInstance* out, size_t* k_out,
                     size_t* bad = nullptr) {
    WireCursor cur{buf, len, 0};
    uint64_t count = 0;
    *k_out = 0;
    if (bad) *bad = 0;
    if (vec_prefix) {
        if (!cur.u64(count)) return WIRE_TRUNCATED;
        if (count > cur.left() / WIRE_MIN_INSTANCE) return WIRE_LENGTH_PREFIX;
    }
    size_t k = 0;
    while (vec_prefix ? k < count : cur.left() > 0) {
        if (bad) *bad = k;
        if (k >= max_k) return WIRE_TOO_MANY;
        const int rc = wire_walk_instance(cur, out[k]);
        if (rc) return rc;
        *k_out = ++k;
    }
    if (cur.left()) return WIRE_TRAILING;
    return WIRE_OK;
}

}  // namespace halo
