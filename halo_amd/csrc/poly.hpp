// What poly.hip offers the IPA sessions (ipa.hip, pcdl_open.hip): field-only work on device buffers.
#pragma once
#include "runtime.hpp"

namespace halo {

// dot product of two device ark vectors -> device ark scalar (out_ark), using tmp (>= 2048*32 B)
int dot_device(int field, const void* x, const void* y, size_t n, void* out_ark, void* tmp, hipStream_t s);
// out[i] = z^i, i < n (device ark scalar z_ark, ark out), stream-ordered on s
int powers_device(int field, const void* z_ark, size_t n, void* out, hipStream_t s);
// h(X) of pcdl.rs:198-219 from xi rows (lg_n + 1 ark scalars each) and weights that are device pointers.
// d_tables: hpoly_table_elems(k, lg_n) field elements of scratch.  prof_name (or null): the halo_profile_read
// name of the coefficient kernel.
size_t hpoly_table_elems(size_t k, uint32_t lg_n);
// sum_i alphas[i] h_i as one coefficient vector (ark, 2^lg_n entries); d_alphas null: every weight is one
int hpoly_combine_device(int field, const void* d_xis, size_t k, uint32_t lg_n, const void* d_alphas, void* d_tables,
                         void* d_out, hipStream_t s, const char* prof_name);
// the g separate coefficient rows (ark, row i at d_rows + 32 i 2^lg_n); g 2^lg_n < 2^32
int hpoly_rows_device(int field, const void* d_xis, size_t g, uint32_t lg_n, void* d_tables, void* d_rows, hipStream_t s);
// g partial sums of hpoly_combine_device's k weighted polynomials, from the half-tables it left at d_tables: row s
// (ark, at d_rows + 32 s 2^lg_n) sums the instances [x, y) of the uint4 d_segs[s], x < y <= k; g 2^lg_n < 2^32
int hpoly_segments_device(int field, const void* d_tables, size_t k, uint32_t lg_n, const void* d_segs, size_t g, void* d_rows,
                          hipStream_t s);

}  // namespace halo
