// One scratch buffer carved into 256-byte-aligned parts, and the arrays of a host call as such parts.  Free of
// HIP: standard headers only, so the host C++ compiler builds it alone (tests/scratch_layout_dump.cpp,
// tests/test_scratch_layout.py).  upload_parts (runtime.hpp) puts a HostParts table into st->scratch[0].
#pragma once
#include <cstddef>
#include <initializer_list>
#include <utility>
#include <vector>

namespace halo {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Parts in the order they are taken; a part of no bytes takes nothing and shares the next part's offset.
struct ScratchLayout {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += align256(bytes);
        return o;
    }
    size_t total() const { return off; }
};

// The arrays a host call sends to the device, in upload order.
struct HostParts {
    static constexpr size_t ABSENT = ~(size_t)0;
    struct Row {
        const void* src;
        size_t bytes, off;
    };
    std::vector<Row> rows;
    ScratchLayout lay;
    HostParts(std::initializer_list<std::pair<const void*, size_t>> parts = {}) {  // a call's table: {src, bytes} rows
        for (const auto& p : parts) add(p.first, p.second);
    }
    void add(const void* src, size_t bytes) { rows.push_back(Row{src, bytes, lay.take(bytes)}); }
    size_t total() const { return lay.total(); }
    size_t at(size_t j) const { return rows[j].bytes ? rows[j].off : ABSENT; }  // ABSENT: a part of no bytes
};

}  // namespace halo
