// otmb_sink.hip -- buildTsink: the settling operator S of particles that sink at a speed w >= 0 (otmb_build_sink[_dev]).  include/otmb.h states
// the contract; tests/sink_ref.py restates it in numpy.  No function of the reference builds S: the contract is this library's own, in the
// style of vertical_diffusion_operator_sparse_entries (src/matrixbuilding.jl:438-479).
//
// Per wet cell c at (i, j, k), ascending in wet order: a = area2D[i, j], w_c the speed at c's bottom face, b the wet cell below, if any:
//     (c, c) = (w_c * a) / v3D[c];   (b, c) = -((w_c * a) / v3D[b]);   closed seafloor and no b: (c, c) = +0.0, stored.
// One operation per statement, no FMA (-ffp-contract=off).
//
// Column c holds (c, c) and then (b, c): b > c in wet order, so the rows ascend and the matrix is CSC as it is generated -- no triplets, no
// sort.  Column c starts at c + the cells before c that have a wet cell below: one exclusive scan of the column lengths (otmb_prims.h).
// Two passes over the wet cells: sk_count_kernel derives every cell (its checks included) and stores the column's length; after the scan the
// host reads the flags and nnz, and only when every check passed sk_fill_kernel derives the cells again and writes the three arrays.
#include <hip/hip_runtime.h>

#include <cmath>

#include "otmb_prims.h"

enum { SK_BAD_W = 1, SK_NAN = 2, SK_BAD_IDX = 4 };

struct SkGrid {
    const double *v3d, *area, *w;
    const i64 *lwet3d, *lwet;
    i64 n, nx, ny, nz;
    double ws;
    int form, closed;
};
struct SkCell {
    i64 b;  // the wet rank (0-based) of the cell below, -1: none
    double diag, off;
    unsigned bad;
};

// every index is checked before anything is read through it; w is read on wet cells only
__device__ __forceinline__ SkCell sk_cell(const SkGrid &g, i64 c) {
    SkCell r = {-1, 0.0, 0.0, 0u};
    const i64 plane = g.nx * g.ny;
    const i64 L = g.lwet[c] - 1;
    if (L < 0 || L >= plane * g.nz || g.lwet3d[L] != c + 1) {
        r.bad = SK_BAD_IDX;
        return r;
    }
    const i64 k = L / plane, ij = L - k * plane;
    if (k + 1 < g.nz) {
        const i64 q = g.lwet3d[L + plane];
        if (q != 0) {
            if (q <= c + 1 || q > g.n) {
                r.bad = SK_BAD_IDX;
                return r;
            }
            r.b = q - 1;
        }
    }
    const double wc = g.form == 0 ? g.ws : (g.form == 1 ? g.w[k] : g.w[L]);
    if (!(wc >= 0.0) || isinf(wc)) {
        r.bad = SK_BAD_W;
        return r;
    }
    const double wa = wc * g.area[ij];
    if (r.b >= 0) {
        r.diag = wa / g.v3d[L];
        r.off = -(wa / g.v3d[L + plane]);
    } else {
        r.diag = g.closed ? 0.0 : wa / g.v3d[L];
    }
    if (isnan(r.diag) || isnan(r.off)) r.bad = SK_NAN;
    return r;
}

__global__ __launch_bounds__(256) void sk_count_kernel(SkGrid g, i64 *__restrict__ inc, unsigned *__restrict__ flags) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c > g.n) return;
    if (c == g.n) {
        inc[c] = 0;
        return;
    }
    const SkCell r = sk_cell(g, c);
    inc[c] = r.b >= 0 ? 2 : 1;
    if (r.bad) atomicOr(flags, r.bad);
}

// start[c] + 1 < start[n] = nnz <= cap for a column of two entries: the scan of the lengths this kernel derives again
__global__ __launch_bounds__(256) void sk_fill_kernel(SkGrid g, const i64 *__restrict__ start, i64 *__restrict__ colptr, i64 *__restrict__ rowval,
                                                      double *__restrict__ nzval) {
    const i64 c = (i64)blockIdx.x * 256 + threadIdx.x;
    if (c > g.n) return;
    const i64 p = start[c];
    colptr[c] = p + 1;
    if (c == g.n) return;
    const SkCell r = sk_cell(g, c);
    rowval[p] = c + 1;
    nzval[p] = r.diag;
    if (r.b >= 0) {
        rowval[p + 1] = r.b + 1;
        nzval[p + 1] = r.off;
    }
}

static int32_t sk_check_sizes(otmb_ctx *ctx, int32_t w_form, i64 n_wet, i64 nx, i64 ny, i64 nz, i64 cap) {
    if (w_form < 0 || w_form > 2) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "buildTsink: w_form must be 0 (scalar), 1 (nz values) or 2 (nx*ny*nz values)");
    if (nx < 0 || ny < 0 || nz < 0 || n_wet < 0 || cap < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "buildTsink: sizes");
    const i64 lim = (i64)1 << 20;  // (no product below overflows)
    if (nx >= lim || ny >= lim || nz >= lim || nx * ny * nz >= ((i64)1 << 40) || cap >= ((i64)1 << 41)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "buildTsink: grid too large");
    if (n_wet > nx * ny * nz) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "buildTsink: more wet cells than cells");
    return OTMB_OK;
}

extern "C" {

int32_t otmb_build_sink_dev(otmb_ctx *ctx, int32_t w_form, double w_scalar, const double *w, const double *v3d, const double *area2d,
                            const int64_t *lwet3d, const int64_t *lwet, int64_t n_wet, int64_t nx, int64_t ny, int64_t nz, int32_t closed,
                            int64_t *colptr, int64_t *rowval, double *nzval, int64_t cap, int64_t *nnz) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sk_check_sizes(ctx, w_form, n_wet, nx, ny, nz, cap))) return rc;
    if (!colptr || !nnz || (w_form != 0 && !w)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (n_wet > 0 && (!v3d || !area2d || !lwet3d || !lwet || !rowval || !nzval)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    otmb_ctx::SinkScratch &S = ctx->sink;
    if ((rc = otmb_reserve(ctx, S.inc, (size_t)(n_wet + 1) * 8)) || (rc = otmb_reserve(ctx, S.start, (size_t)(n_wet + 1) * 8)) ||
        (rc = otmb_reserve(ctx, S.flags, 16)))
        return rc;
    const SkGrid g = {v3d, area2d, w, lwet3d, lwet, n_wet, nx, ny, nz, w_scalar, w_form, closed ? 1 : 0};
    unsigned *flags = (unsigned *)S.flags.p;
    i64 *inc = (i64 *)S.inc.p, *start = (i64 *)S.start.p;
    HIP_TRY(ctx, hipMemsetAsync(flags, 0, 16, ctx->stream));
    hipLaunchKernelGGL(sk_count_kernel, OTMB_GRID_EXACT(n_wet + 1, ctx->stream), g, inc, flags);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = otmb_exclusive_scan(ctx, S.prim_tmp, inc, start, n_wet + 1))) return rc;
    unsigned bad = 0;
    i64 total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&total, start + n_wet, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (bad & SK_BAD_IDX) return otmb_fail(ctx, OTMB_ERR_NONCANONICAL_INDICES);
    if (bad & SK_BAD_W) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "buildTsink: w must be finite and >= 0 on the bottom face of every wet cell");
    if (bad & SK_NAN) return otmb_fail(ctx, OTMB_ERR_TSINK_NAN);
    *nnz = total;
    if (total > cap) {
        char msg[128];
        snprintf(msg, sizeof msg, "buildTsink: nnz = %lld, capacity %lld", (long long)total, (long long)cap);
        return otmb_fail(ctx, OTMB_ERR_CAPACITY, msg);
    }
    hipLaunchKernelGGL(sk_fill_kernel, OTMB_GRID_EXACT(n_wet + 1, ctx->stream), g, (const i64 *)start, colptr, rowval, nzval);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_build_sink(otmb_ctx *ctx, int32_t w_form, double w_scalar, const double *w, const double *v3d, const double *area2d,
                        const int64_t *lwet3d, const int64_t *lwet, int64_t n_wet, int64_t nx, int64_t ny, int64_t nz, int32_t closed,
                        int64_t *colptr, int64_t *rowval, double *nzval, int64_t cap, int64_t *nnz) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sk_check_sizes(ctx, w_form, n_wet, nx, ny, nz, cap))) return rc;
    if (!colptr || !nnz || (w_form != 0 && !w) || !v3d || !area2d || !lwet3d || !lwet || !rowval || !nzval)
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const i64 G = nx * ny * nz, P = nx * ny, nw = w_form == 0 ? 0 : (w_form == 1 ? nz : G);
    DevArena A;
    const size_t o_v = A.take((size_t)G * 8), o_a = A.take((size_t)P * 8), o_l3 = A.take((size_t)G * 8), o_l = A.take((size_t)n_wet * 8),
                 o_w = A.take((size_t)nw * 8), o_cp = A.take((size_t)(n_wet + 1) * 8), o_rv = A.take((size_t)cap * 8), o_nz = A.take((size_t)cap * 8);
    if ((rc = otmb_reserve_some(ctx, ctx->sink.host, A.total()))) return rc;
    char *base = (char *)ctx->sink.host.p;
    const struct { size_t off; const void *host; i64 bytes; } up[5] = {{o_v, v3d, G * 8}, {o_a, area2d, P * 8}, {o_l3, lwet3d, G * 8}, {o_l, lwet, n_wet * 8}, {o_w, w, nw * 8}};
    for (const auto &u : up)
        if (u.bytes > 0) {
            HIP_TRY(ctx, hipMemcpyAsync(base + u.off, u.host, (size_t)u.bytes, hipMemcpyHostToDevice, ctx->stream));
            ctx->uploaded_bytes += u.bytes;
        }
    rc = otmb_build_sink_dev(ctx, w_form, w_scalar, (const double *)(base + o_w), (const double *)(base + o_v), (const double *)(base + o_a),
                             (const i64 *)(base + o_l3), (const i64 *)(base + o_l), n_wet, nx, ny, nz, closed, (i64 *)(base + o_cp), (i64 *)(base + o_rv),
                             (double *)(base + o_nz), cap, nnz);
    if (rc) {
        const std::string msg = ctx->err;
        (void)hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's arrays)
        ctx->err = msg;
        return rc;
    }
    HIP_TRY(ctx, hipMemcpyAsync(colptr, base + o_cp, (size_t)(n_wet + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (*nnz > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(rowval, base + o_rv, (size_t)*nnz * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(nzval, base + o_nz, (size_t)*nnz * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OTMB_OK;
}

}  // extern "C"
