// otmb_prims.hip -- the library's one copy of "size query, reserve, run" around rocPRIM's scan and radix sort, and its trivial element kernels
// (otmb_prims.h).  No other file includes rocPRIM: a change of type or configuration here is a change for every caller at once.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "otmb_prims.h"

// run(nullptr, bytes) sizes rocPRIM's temporary, run(tmp.p, bytes) does the work
template <class Run>
static int32_t prims_run(otmb_ctx *ctx, DevBuf &tmp, const char *what_size, const char *what, Run run) {
    size_t bytes = 0;
    if (run(nullptr, bytes) != hipSuccess) return otmb_fail(ctx, OTMB_ERR_HIP, what_size);
    int32_t rc;
    if ((rc = otmb_reserve(ctx, tmp, bytes + 16))) return rc;
    if (run(tmp.p, bytes) != hipSuccess) return otmb_fail(ctx, OTMB_ERR_HIP, what);
    return OTMB_OK;
}

int32_t otmb_exclusive_scan(otmb_ctx *ctx, DevBuf &tmp, const i64 *in, i64 *out, i64 n) {
    return prims_run(ctx, tmp, "scan (size)", "scan", [&](void *t, size_t &bytes) {
        return rocprim::exclusive_scan(t, bytes, in, out, (i64)0, (size_t)n, rocprim::plus<i64>(), ctx->stream);
    });
}
int32_t otmb_inclusive_scan(otmb_ctx *ctx, DevBuf &tmp, const i64 *in, i64 *out, i64 n) {
    return prims_run(ctx, tmp, "scan (size)", "scan", [&](void *t, size_t &bytes) {
        return rocprim::inclusive_scan(t, bytes, in, out, (size_t)n, rocprim::plus<i64>(), ctx->stream);
    });
}

template <class KI, class K, class VI, class V>
static int32_t prims_sort(otmb_ctx *ctx, DevBuf &tmp, KI keys_in, K *keys_out, VI vals_in, V *vals_out, i64 n, int bits) {
    return prims_run(ctx, tmp, "radix_sort_pairs (size)", "radix_sort_pairs", [&](void *t, size_t &bytes) {
        return rocprim::radix_sort_pairs(t, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, (unsigned)bits, ctx->stream);
    });
}
int32_t otmb_sort_pairs(otmb_ctx *ctx, DevBuf &tmp, u64 *keys_in, u64 *keys_out, u64 *vals_in, u64 *vals_out, i64 n, int bits) {
    return prims_sort(ctx, tmp, keys_in, keys_out, vals_in, vals_out, n, bits);
}
int32_t otmb_sort_pairs(otmb_ctx *ctx, DevBuf &tmp, const i64 *keys_in, i64 *keys_out, const i64 *vals_in, i64 *vals_out, i64 n, int bits) {
    return prims_sort(ctx, tmp, keys_in, keys_out, vals_in, vals_out, n, bits);
}
int32_t otmb_sort_pairs(otmb_ctx *ctx, DevBuf &tmp, const unsigned *keys_in, unsigned *keys_out, const i64 *vals_in, i64 *vals_out, i64 n, int bits) {
    return prims_sort(ctx, tmp, keys_in, keys_out, vals_in, vals_out, n, bits);
}

// ---- element kernels (grid-stride) -------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void prims_widen_kernel(const T *__restrict__ in, i64 n, i64 add, i64 *__restrict__ out) {
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < n; q += (i64)gridDim.x * 256) out[q] = (i64)in[q] + add;
}
__global__ __launch_bounds__(256) void prims_iota_kernel(i64 *__restrict__ a, i64 n, i64 first) {
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < n; q += (i64)gridDim.x * 256) a[q] = first + q;
}

void otmb_widen(hipStream_t st, const uint8_t *in, i64 n, i64 add, i64 *out) { hipLaunchKernelGGL(prims_widen_kernel<uint8_t>, OTMB_GRID_STRIDE(n, st), in, n, add, out); }
void otmb_widen(hipStream_t st, const unsigned *in, i64 n, i64 add, i64 *out) { hipLaunchKernelGGL(prims_widen_kernel<unsigned>, OTMB_GRID_STRIDE(n, st), in, n, add, out); }
void otmb_widen(hipStream_t st, const int *in, i64 n, i64 add, i64 *out) { hipLaunchKernelGGL(prims_widen_kernel<int>, OTMB_GRID_STRIDE(n, st), in, n, add, out); }
void otmb_iota(hipStream_t st, i64 *a, i64 n, i64 first) { hipLaunchKernelGGL(prims_iota_kernel, OTMB_GRID_STRIDE(n, st), a, n, first); }
