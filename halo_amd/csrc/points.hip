// Point utilities on gfx950: the ark WrappedPoint <-> internal affine conversions, packed XYZZ ->
// affine, the point sums (halo_point_sum*) and the host-output step of every entry point that returns
// one point (d2h_point, halo_xyzz_to_wrapped).
#include <algorithm>

#include "dispatch.hpp"
#include "points.hpp"
#include "runtime.hpp"

namespace halo {

// ---------------------------------------------------------------------------------------------
// conversion kernels
// ---------------------------------------------------------------------------------------------
template <class F>
__global__ void k_wrapped_to_internal(const uint4* in, uint4* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    aff_store(out + 4 * i, aff_from_wrapped<F>(in + 4 * i));
}

template <class F>
__global__ void k_internal_to_wrapped(const uint4* in, uint4* out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    aff_to_wrapped(out + 4 * i, aff_load<F>(in + 4 * i));
}

template <class Cv>
__global__ __launch_bounds__(64) void k_xyzz_to_aff(const uint4* in, uint4* out, int count) {
    using F = typename Cv::Base;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    aff_store(out + 4 * i, xyzz_to_aff(xyzz_load<F>(in + 8 * i)));
}

// one block per row: row b sums the k WrappedPoints at pts_wrapped + 4 k b into out_wrapped + 4 b
template <class Cv>
__global__ __launch_bounds__(256) void k_point_sum(const uint4* pts_wrapped, size_t k, uint4* out_wrapped) {
    using F = typename Cv::Base;
    __shared__ uint4 red[256 * 8];
    pts_wrapped += 4 * k * (size_t)blockIdx.x;
    out_wrapped += 4 * (size_t)blockIdx.x;
    XYZZ<F> acc = xyzz_id<F>();
    for (size_t i = threadIdx.x; i < k; i += 256) acc = xyzz_madd(acc, aff_from_wrapped<F>(pts_wrapped + 4 * i));
    xyzz_store(red + 8 * threadIdx.x, acc);
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            xyzz_store(red + 8 * threadIdx.x,
                       xyzz_add(xyzz_load<F>(red + 8 * threadIdx.x), xyzz_load<F>(red + 8 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) aff_to_wrapped(out_wrapped, xyzz_to_aff(xyzz_load<F>(red)));
}

// Sum of k packed XYZZ points (stride_bytes apart) -> packed XYZZ (no affine conversion on the device)
template <class Cv>
__global__ __launch_bounds__(256) void k_point_sum_xyzz(const uint4* pts, size_t k, size_t stride_u4, uint4* out) {
    using F = typename Cv::Base;
    __shared__ uint4 red[256 * 8];
    XYZZ<F> acc = xyzz_id<F>();
    for (size_t i = threadIdx.x; i < k; i += 256) acc = xyzz_add(acc, xyzz_load<F>(pts + stride_u4 * i));
    xyzz_store(red + 8 * threadIdx.x, acc);
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off)
            xyzz_store(red + 8 * threadIdx.x,
                       xyzz_add(xyzz_load<F>(red + 8 * threadIdx.x), xyzz_load<F>(red + 8 * (threadIdx.x + off))));
        __syncthreads();
    }
    if (threadIdx.x == 0) xyzz_store(out, xyzz_load<F>(red));
}

// ---------------------------------------------------------------------------------------------
// host orchestration
// ---------------------------------------------------------------------------------------------
int check_curve(halo_curve_t c) {
    if (!valid_curve(c)) return set_error(HALO_EINVAL, "unknown curve id %d", (int)c);
    return HALO_OK;
}

int check_field(halo_field_t f) {
    if (!valid_field(f)) return set_error(HALO_EINVAL, "unknown field id %d", (int)f);
    return HALO_OK;
}

int d2h_point(int curve, const void* d_xyzz, halo_wrapped_point_t* out, hipStream_t s) {
    alignas(16) uint64_t buf[16];
    HALO_CHECK(copy_d2h(buf, d_xyzz, 128, s));
    host_xyzz_to_wrapped(curve, buf, out);
    return HALO_OK;
}

int convert_wrapped_to_internal(int curve, const void* in, void* out, size_t n, hipStream_t s) {
    if (!n) return HALO_OK;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_wrapped_to_internal<typename Cv::Base>, dim3(grid_for(n, 256)), dim3(256), 0, s,
                           (const uint4*)in, (uint4*)out, n);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int convert_internal_to_wrapped(int curve, const void* in, void* out, size_t n, hipStream_t s) {
    if (!n) return HALO_OK;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_internal_to_wrapped<typename Cv::Base>, dim3(grid_for(n, 256)), dim3(256), 0, s,
                           (const uint4*)in, (uint4*)out, n);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int xyzz_to_affine_device(int curve, const void* xyzz, void* aff, int count, hipStream_t s) {
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_xyzz_to_aff<Cv>, dim3(grid_for(count, 64)), dim3(64), 0, s, (const uint4*)xyzz, (uint4*)aff,
                           count);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" int halo_point_sum(halo_curve_t curve, const halo_wrapped_point_t* pts, size_t k, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!out || (k && !pts)) return set_error(HALO_EINVAL, "halo_point_sum: null buffer");
    DeviceState* st = current_state();
    if (!st) return HALO_EDEVICE;
    std::lock_guard<std::mutex> g(st->mu);
    hipStream_t s = 0;
    ScratchUse su(st, s);
    HALO_CHECK(st->scratch[0].reserve(std::max<size_t>(k, 1) * 64 + 64));
    char* buf = (char*)st->scratch[0].ptr;
    HALO_CHECK(copy_h2d(buf + 64, pts, k * 64, s));
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_point_sum<Cv>, dim3(1), dim3(256), 0, s, (const uint4*)(buf + 64), k, (uint4*)buf);
    });
    HALO_HIP(hipGetLastError());
    return copy_d2h(out, buf, 64, s);
}

extern "C" int halo_point_sum_dev(halo_curve_t curve, const void* d_pts, size_t k, size_t stride_bytes, void* d_out,
                                  void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!d_out || (k && !d_pts)) return set_error(HALO_EINVAL, "halo_point_sum_dev: null buffer");
    if (stride_bytes != 64) return set_error(HALO_EINVAL, "halo_point_sum_dev: only contiguous (64-B stride) points");
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_point_sum<Cv>, dim3(1), dim3(256), 0, s, (const uint4*)d_pts, k, (uint4*)d_out);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

extern "C" int halo_point_sum_rows_dev(halo_curve_t curve, const void* d_pts, size_t rows, size_t k, void* d_out,
                                       void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!rows) return HALO_OK;
    if (!d_out || (k && !d_pts)) return set_error(HALO_EINVAL, "halo_point_sum_rows_dev: null buffer");
    if (rows > 65535) return set_error(HALO_EINVAL, "halo_point_sum_rows_dev: %zu rows (at most 65535)", rows);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_point_sum<Cv>, dim3((unsigned)rows), dim3(256), 0, s, (const uint4*)d_pts, k, (uint4*)d_out);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

extern "C" int halo_point_sum_xyzz_dev(halo_curve_t curve, const void* d_pts, size_t k, size_t stride_bytes, void* d_out,
                                       void* stream) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (!d_out || (k && !d_pts)) return set_error(HALO_EINVAL, "halo_point_sum_xyzz_dev: null buffer");
    if (stride_bytes < 128 || stride_bytes % 16)
        return set_error(HALO_EINVAL, "halo_point_sum_xyzz_dev: stride %zu (a multiple of 16, at least 128)", stride_bytes);
    hipStream_t s = (hipStream_t)stream;
    DISPATCH_CURVE(curve, Cv, {
        hipLaunchKernelGGL(k_point_sum_xyzz<Cv>, dim3(1), dim3(256), 0, s, (const uint4*)d_pts, k, stride_bytes / 16,
                           (uint4*)d_out);
    });
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

extern "C" int halo_xyzz_to_wrapped(halo_curve_t curve, const void* xyzz, size_t k, halo_wrapped_point_t* out) {
    clear_error();
    HALO_CHECK(check_curve(curve));
    if (k && (!xyzz || !out)) return set_error(HALO_EINVAL, "halo_xyzz_to_wrapped: null buffer");
    for (size_t i = 0; i < k; i++) host_xyzz_to_wrapped(curve, (const char*)xyzz + 128 * i, out + i);
    return HALO_OK;
}
