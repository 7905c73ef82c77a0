// otmb_spmv.hip -- a resident sparse operator: Y = α·A·X + β·Y and Y = α·Aᵀ·X + β·Y on the device (otmb_op_*).
//
// Semantics: SparseArrays' 5-argument mul! for Julia 1.10 (the reference's floor), restated as published (no reference test pins them):
//   * β step first (LinearAlgebra._rmul_or_fill!): β == 0 fills Y with +0.0 (NaN / Inf already in Y are discarded), β == 1 leaves Y,
//     otherwise Y[i,c] = Y[i,c] * β;
//   * A·X (_spmatmul!): for each tracer c, for col = 1..n in order, αxj = X[col,c] * α, then Y[rowval[j],c] += nzval[j] * αxj for the
//     stored j of column col in stored order.  Every Y[i,c] is a left fold from the β step's value over its contributions in STORAGE
//     order (by column, inside a column by position; duplicate / unsorted rows included);
//   * Aᵀ·X (_At_or_Ac_mul_B!; real, so the adjoint is the transpose): tmp = +0.0, tmp += nzval[j] * X[rowval[j],c] in stored order,
//     then Y[col,c] += tmp * α (an empty column adds +0.0 * α).
// No FMA (the library is built with -ffp-contract=off).  Exactness means ONE sequential fold per output element: parallelism comes from
// rows, columns and tracers only, and a long row or column is one lane's dependent chain.
//
// Layouts, built once per pattern by the plan (otmb_op_create[_dev]); the operator owns every array, no caller array is read afterwards:
//   CSC copy     colptr (Int64), rowval - 1 as Int32, nzval: what Aᵀ·X reads.  A wave takes 64 columns, whose entries are ONE contiguous
//                run; it is staged through LDS in chunks by coalesced loads, then every lane folds its own column from LDS.
//   row slices   the rows of A in groups of 64 (a slice = a wave).  Entry e of the slice's rows lies at sbase[slice] + 64 e + lane, for
//                values (Float64) and column indices (Int32): the loads of one step e coalesce across the wave.  Each slice is as wide
//                as its longest short row; a lane stops at its own row's length (padding is skipped, never added).  Inside a row the
//                entries are in storage order: the plan's stable radix sort of (row, position) is the stable transposition.
//   long rows    rows longer than SP_ELL_MAX, or longer than 32 and four times their slice's mean, would widen their whole slice: they
//                are stored contiguously behind the slices and folded by spmv_long_kernel, one workgroup per row (coalesced chunks in
//                LDS, one lane per tracer).
//   dst          the position of every stored entry (CSC order) in the two layouts above: "set values" is one streaming scatter.
#include <hip/hip_runtime.h>

#include "otmb_op_fold.h"  // struct otmb_op, SP_ELL_MAX, SP_TCH; the walks over the layouts
#include "otmb_prims.h"

#define SP_GRID(n) OTMB_GRID_STRIDE(n, op->ctx->stream)

// ---- device helpers ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double sp_beta(const double *__restrict__ y, int bmode, double beta) {
    // LinearAlgebra._rmul_or_fill!: β == 0 -> +0.0 (Y is not read), β == 1 -> Y, otherwise Y * β
    return bmode == 0 ? 0.0 : (bmode == 1 ? *y : *y * beta);
}

// ---- plan --------------------------------------------------------------------------------------------------------------------
enum { SP_BAD_CP = 1, SP_BAD_RV = 2 };
__global__ __launch_bounds__(256) void spmv_check_colptr_kernel(const i64 *__restrict__ p, i64 n, i64 nnz, unsigned *__restrict__ bad) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < n; c += (i64)gridDim.x * 256) {
        const i64 a = p[c], b = p[c + 1];
        if (a < 1 || b < a || b > nnz + 1) atomicOr(bad, (unsigned)SP_BAD_CP);
    }
}
// rowval in 1..m; writes rowval - 1 as Int32 (the sort keys and Aᵀ's row stream) and the identity permutation
__global__ __launch_bounds__(256) void spmv_check_rowval_kernel(const i64 *__restrict__ r, i64 nnz, i64 m, int *__restrict__ rv32, i64 *__restrict__ iota,
                                                                unsigned *__restrict__ bad) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (i64)gridDim.x * 256) {
        const i64 i = r[e];
        if (i < 1 || i > m) atomicOr(bad, (unsigned)SP_BAD_RV);
        rv32[e] = (int)(i - 1);
        iota[e] = e;
    }
}
// rowptr[i] = first position p of the sorted keys with key >= i (i = 0..m)
__global__ __launch_bounds__(256) void spmv_rowptr_kernel(const unsigned *__restrict__ keys, i64 nnz, i64 m, i64 *__restrict__ rowptr) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i <= m; i += (i64)gridDim.x * 256) {
        i64 lo = 0, hi = nnz;
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if ((i64)keys[mid] < i) lo = mid + 1; else hi = mid;
        }
        rowptr[i] = lo;
    }
}
// one wave per slice: long rows, the slice's width; elen (-1: long), swidth (64 * width), lflag, lent (entries of a long row)
__global__ __launch_bounds__(256) void spmv_slice_kernel(const i64 *__restrict__ rowptr, i64 m, i64 nslices, int *__restrict__ elen, i64 *__restrict__ swidth,
                                                         i64 *__restrict__ lflag, i64 *__restrict__ lent) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 s = i >> 6;
    const int lane = threadIdx.x & 63;
    if (s > nslices) return;  // (whole waves: s is uniform across a wave)
    const i64 len = i < m ? rowptr[i + 1] - rowptr[i] : 0;
    i64 sum = len;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    const i64 rows = (s < nslices) ? min((i64)64, m - (s << 6)) : 1;
    const i64 mean = (sum + rows - 1) / rows;
    const bool lng = i < m && (len > SP_ELL_MAX || (len > 32 && len > 4 * mean));
    i64 w = lng ? 0 : len;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) w = max(w, (i64)__shfl_xor(w, d));
    if (i < m) {
        elen[i] = lng ? -1 : (int)len;
        lflag[i] = lng ? 1 : 0;
        lent[i] = lng ? len : 0;
    } else if (i == m) {
        lflag[i] = 0;
        lent[i] = 0;
    }
    if (lane == 0) swidth[s] = s < nslices ? 64 * w : 0;
}
// dst[perm[p]]: where the p-th entry in row order lies in the slices / behind them
__global__ __launch_bounds__(256) void spmv_dst_kernel(const i64 *__restrict__ perm, const unsigned *__restrict__ keys, const i64 *__restrict__ rowptr,
                                                       const int *__restrict__ elen, const i64 *__restrict__ sbase, const i64 *__restrict__ loff, i64 nnz, i64 ell,
                                                       i64 *__restrict__ dst) {
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nnz; p += (i64)gridDim.x * 256) {
        const i64 i = keys[p], e = p - rowptr[i];
        dst[perm[p]] = elen[i] >= 0 ? sbase[i >> 6] + 64 * e + (i & 63) : ell + loff[i] + e;
    }
}
__global__ __launch_bounds__(256) void spmv_lrows_kernel(const i64 *__restrict__ lflag, const i64 *__restrict__ lidx, i64 m, i64 *__restrict__ lrows) {
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < m; i += (i64)gridDim.x * 256)
        if (lflag[i]) lrows[lidx[i]] = i;
}
__global__ __launch_bounds__(256) void spmv_colidx_kernel(const i64 *__restrict__ cp, i64 n, const i64 *__restrict__ dst, int *__restrict__ col) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < n; c += (i64)gridDim.x * 256)
        for (i64 j = cp[c] - 1; j < cp[c + 1] - 1; ++j) col[dst[j]] = (int)c;
}
// "set values": every stored value to its place in the slices / long rows (a streaming read, a scatter)
__global__ __launch_bounds__(256) void spmv_relayout_kernel(const double *__restrict__ nz, const i64 *__restrict__ dst, i64 nnz, double *__restrict__ val) {
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j < nnz; j += (i64)gridDim.x * 256) val[dst[j]] = nz[j];
}

// ---- A·X: one lane per row ------------------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void spmv_rows_kernel(const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ sbase,
                                                        const int *__restrict__ elen, i64 m, const double *__restrict__ X, i64 ldx, double *__restrict__ Y,
                                                        i64 ldy, double alpha, double beta, int bmode) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int len = elen[i];
    if (len < 0) return;  // a long row: spmv_long_kernel
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) acc[c] = sp_beta(Y + i + c * ldy, bmode, beta);
    op_fold_slice_row(val, col, sbase, i, len, [&](double v, i64 j) {
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            const double axj = X[j + c * ldx] * alpha;
            acc[c] = acc[c] + v * axj;
        }
    });
#pragma unroll
    for (int c = 0; c < KB; ++c) Y[i + c * ldy] = acc[c];
}

// one workgroup per long row: the row's entries in coalesced chunks through LDS, lane c folds tracer c (groups of 64 tracers)
__global__ __launch_bounds__(64) void spmv_long_kernel(const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ lrows,
                                                       const i64 *__restrict__ loff, i64 ell, int k, const double *__restrict__ X, i64 ldx,
                                                       double *__restrict__ Y, i64 ldy, double alpha, double beta, int bmode) {
    __shared__ double sv[SP_TCH];
    __shared__ int sc[SP_TCH];
    const int lane = threadIdx.x;
    const i64 i = lrows[blockIdx.x];
    const i64 b0 = ell + loff[i], len = loff[i + 1] - loff[i];
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int c = c0 + lane;
        double acc = c < k ? sp_beta(Y + i + c * ldy, bmode, beta) : 0.0;
        op_fold_long_row(val, col, b0, len, sv, sc, lane, c < k, [&](double v, i64 j) {
            const double axj = X[j + c * ldx] * alpha;
            acc = acc + v * axj;
        });
        if (c < k) Y[i + c * ldy] = acc;
    }
}

// ---- Aᵀ·X: one lane per column of A, the wave's contiguous run of entries staged through LDS ---------------------------------------
template <int KB>
__global__ __launch_bounds__(64) void spmv_cols_kernel(const i64 *__restrict__ cp, const int *__restrict__ rv, const double *__restrict__ nz, i64 n,
                                                       const double *__restrict__ X, i64 ldx, double *__restrict__ Y, i64 ldy, double alpha, double beta,
                                                       int bmode) {
    __shared__ double sv[SP_TCH];
    __shared__ int sr[SP_TCH];
    const int lane = threadIdx.x;
    i64 colm;
    double tmp[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) tmp[c] = 0.0;
    const bool has = op_fold_csc_run(cp, rv, nz, n, sv, sr, (i64)blockIdx.x * 64, lane, colm, [&](double v, i64 r) {
#pragma unroll
        for (int c = 0; c < KB; ++c) tmp[c] = tmp[c] + v * X[r + c * ldx];
    });
    if (has) {
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            const double y0 = sp_beta(Y + colm + c * ldy, bmode, beta);
            const double t = tmp[c] * alpha;
            Y[colm + c * ldy] = y0 + t;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static int32_t sp_reserve(otmb_op *op, DevBuf &b, size_t bytes) { return otmb_reserve_some(op->ctx, b, bytes); }
static void sp_free_all(otmb_op *op) {
    // the slots own the value arrays; an operator whose plan never stood has no slot yet, and nz and val are then its own
    for (OpSlot &s : op->slots) {
        otmb_free(s.nz);
        otmb_free(s.val);
    }
    if (!op->slots.empty()) op->nz = op->val = DevBuf();
    op->slots.clear();
    for (DevBuf *b : {&op->cp, &op->rv, &op->nz, &op->dst, &op->elen, &op->sbase, &op->loff, &op->lrows, &op->val, &op->col, &op->xs, &op->ys, &op->ds, &op->sw, &op->st,
                      &op->pd, &op->mean.nz, &op->mean.val, &op->interp.nz, &op->interp.val, &op->season, &op->setab, &op->cb, &op->am, &op->ln, &op->ob, &op->oh, &op->src})
        otmb_free(*b);
}

// The plan, on op->cp / a copy of rowval / op->nz already on the device (nnz known): checks, then the layouts.  Scratch is released before
// returning.
static int32_t sp_plan(otmb_op *op, const i64 *rowval) {
    otmb_ctx *ctx = op->ctx;
    const i64 m = op->m, n = op->n, nnz = op->nnz;
    int32_t rc;
    DevScratch S;
    DevBuf &flags = S.add(), &iota = S.add(), &keys = S.add(), &perm = S.add(), &rowptr = S.add(), &tmpb = S.add(), &lflag = S.add(), &lent = S.add(),
           &lidx = S.add(), &swidth = S.add();
    if ((rc = sp_reserve(op, flags, 16))) return rc;
    if ((rc = sp_reserve(op, op->rv, (size_t)nnz * 4))) return rc;
    if ((rc = sp_reserve(op, iota, (size_t)nnz * 8))) return rc;
    unsigned *bad = (unsigned *)flags.p;
    HIP_TRY(ctx, hipMemsetAsync(bad, 0, 16, ctx->stream));
    const i64 *cp = (const i64 *)op->cp.p;
    if (n > 0) hipLaunchKernelGGL(spmv_check_colptr_kernel, SP_GRID(n), cp, n, nnz, bad);
    if (nnz > 0) hipLaunchKernelGGL(spmv_check_rowval_kernel, SP_GRID(nnz), rowval, nnz, m, (int *)op->rv.p, (i64 *)iota.p, bad);
    HIP_TRY(ctx, hipGetLastError());
    unsigned hb = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (hb & SP_BAD_CP) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "colptr not non-decreasing inside [1, nnz + 1]");
    if (hb & SP_BAD_RV) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "row index outside 1:m");
    // stable transposition: radix sort of (row) keys with the storage position as value (LSD radix sort is stable)
    const i64 ns = (m + 63) / 64;
    op->nslices = ns;
    if ((rc = sp_reserve(op, keys, (size_t)nnz * 4))) return rc;
    if ((rc = sp_reserve(op, perm, (size_t)nnz * 8))) return rc;
    if ((rc = sp_reserve(op, rowptr, (size_t)(m + 1) * 8))) return rc;
    unsigned *sk = (unsigned *)keys.p;
    i64 *pm = (i64 *)perm.p;
    if (nnz > 0 && (rc = otmb_sort_pairs(ctx, tmpb, (const unsigned *)op->rv.p, sk, (const i64 *)iota.p, pm, nnz, otmb_bits(m)))) return rc;
    otmb_free(iota);
    i64 *rp = (i64 *)rowptr.p;
    hipLaunchKernelGGL(spmv_rowptr_kernel, SP_GRID(m + 1), (const unsigned *)sk, nnz, m, rp);
    // slices and long rows
    if ((rc = sp_reserve(op, op->elen, (size_t)m * 4))) return rc;
    if ((rc = sp_reserve(op, swidth, (size_t)(ns + 1) * 8))) return rc;
    if ((rc = sp_reserve(op, op->sbase, (size_t)(ns + 1) * 8))) return rc;
    if ((rc = sp_reserve(op, lflag, (size_t)(m + 1) * 8))) return rc;
    if ((rc = sp_reserve(op, lent, (size_t)(m + 1) * 8))) return rc;
    if ((rc = sp_reserve(op, lidx, (size_t)(m + 1) * 8))) return rc;
    if ((rc = sp_reserve(op, op->loff, (size_t)(m + 1) * 8))) return rc;
    i64 *sw = (i64 *)swidth.p, *sb = (i64 *)op->sbase.p, *lf = (i64 *)lflag.p, *le = (i64 *)lent.p, *li = (i64 *)lidx.p, *lo = (i64 *)op->loff.p;
    int *el = (int *)op->elen.p;
    {
        const i64 threads = (ns + 1) * 64;  // every slice and one more wave for the trailing zeros
        hipLaunchKernelGGL(spmv_slice_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, ctx->stream, (const i64 *)rp, m, ns, el, sw, lf, le);
    }
    if ((rc = otmb_exclusive_scan(ctx, tmpb, sw, sb, ns + 1))) return rc;
    if ((rc = otmb_exclusive_scan(ctx, tmpb, lf, li, m + 1))) return rc;
    if ((rc = otmb_exclusive_scan(ctx, tmpb, le, lo, m + 1))) return rc;
    HIP_TRY(ctx, hipGetLastError());
    i64 tot[3] = {0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&tot[0], sb + ns, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&tot[1], li + m, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&tot[2], lo + m, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    op->ell = tot[0];
    op->nlong = tot[1];
    const i64 total = tot[0] + tot[2];
    op->nval = total;
    if ((rc = sp_reserve(op, op->val, (size_t)total * 8))) return rc;
    if ((rc = sp_reserve(op, op->col, (size_t)total * 4))) return rc;
    if ((rc = sp_reserve(op, op->lrows, (size_t)op->nlong * 8))) return rc;
    if ((rc = sp_reserve(op, op->dst, (size_t)nnz * 8))) return rc;
    i64 *dst = (i64 *)op->dst.p;
    if (nnz > 0) hipLaunchKernelGGL(spmv_dst_kernel, SP_GRID(nnz), (const i64 *)pm, (const unsigned *)sk, (const i64 *)rp, (const int *)el, (const i64 *)sb,
                                    (const i64 *)lo, nnz, op->ell, dst);
    if (op->nlong > 0) hipLaunchKernelGGL(spmv_lrows_kernel, SP_GRID(m), (const i64 *)lf, (const i64 *)li, m, (i64 *)op->lrows.p);
    if (n > 0 && nnz > 0) hipLaunchKernelGGL(spmv_colidx_kernel, SP_GRID(n), cp, n, (const i64 *)dst, (int *)op->col.p);
    if (nnz > 0) hipLaunchKernelGGL(spmv_relayout_kernel, SP_GRID(nnz), (const double *)op->nz.p, (const i64 *)dst, nnz, (double *)op->val.p);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

// (declared in otmb_op.h: otmb_op_submatrix's child starts here, from arrays it made on the device)
int32_t sp_plan_resident(otmb_op *op, const i64 *rowval) {
    int32_t rc;
    if ((rc = sp_plan(op, rowval))) return rc;
    op->slots.push_back(OpSlot{op->nz, op->val});  // slot 0, selected
    return OTMB_OK;
}

// n + 1 column pointers are on the device at op->cp: read the first and the last, size nnz
static int32_t sp_ends(otmb_op *op) {
    otmb_ctx *ctx = op->ctx;
    i64 e[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&e[0], op->cp.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&e[1], (const i64 *)op->cp.p + op->n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (e[0] != 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "colptr[1] must be 1");
    if (e[1] < 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "colptr[n + 1] - 1 (nnz) is negative");
    op->nnz = e[1] - 1;
    return OTMB_OK;
}

extern "C" void otmb_op_destroy(otmb_op *op);

static int32_t sp_create(otmb_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, otmb_op **out,
                         hipMemcpyKind kind) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    if (!out) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!colptr) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (m < 0 || n < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "sizes");
    if (m >= (1ll << 31) || n >= (1ll << 31)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "matrix too large (m and n must be < 2^31)");
    if (kind == hipMemcpyHostToDevice) {  // the host copy can be checked before anything is uploaded
        if (colptr[0] != 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "colptr[1] must be 1");
        if (colptr[n] < 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "colptr[n + 1] - 1 (nnz) is negative");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    struct Guard {  // the operator is handed out only when the plan succeeded
        otmb_op *op = new otmb_op();
        ~Guard() { otmb_op_destroy(op); }
    } G;
    otmb_op *op = G.op;
    op->ctx = ctx;
    op->device = ctx->device;
    op->m = m;
    op->n = n;
    int32_t rc;
    if ((rc = sp_reserve(op, op->cp, (size_t)(n + 1) * 8))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(op->cp.p, colptr, (size_t)(n + 1) * 8, kind, ctx->stream));
    if ((rc = sp_ends(op))) return rc;
    const i64 nnz = op->nnz;
    if (nnz >= (1ll << 40)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "matrix too large");
    if (nnz > 0 && (!rowval || !nzval)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    struct Rows {  // rowval as given (Int64), for the plan's checks only
        DevBuf b;
        ~Rows() { otmb_free(b); }
    } rows;
    if ((rc = sp_reserve(op, rows.b, (size_t)nnz * 8))) return rc;
    if ((rc = sp_reserve(op, op->nz, (size_t)nnz * 8))) return rc;
    if (nnz > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(rows.b.p, rowval, (size_t)nnz * 8, kind, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(op->nz.p, nzval, (size_t)nnz * 8, kind, ctx->stream));
        if (kind == hipMemcpyHostToDevice) ctx->uploaded_bytes += 16 * nnz + 8 * (n + 1);
    }
    if ((rc = sp_plan_resident(op, (const i64 *)rows.b.p))) return rc;
    *out = op;
    G.op = nullptr;
    return OTMB_OK;
}

// the scatter into slot `slot`, or into the selected one (slot == -1)
static int32_t sp_set_values(otmb_op *op, int64_t slot, const double *nzval, int64_t nnz, hipMemcpyKind kind) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    if (slot < -1 || slot >= (i64)op->slots.size()) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "set_values: slot out of range (otmb_op_set_slots)");
    const OpSlot &to = op->slots[(size_t)(slot < 0 ? op->sel : slot)];
    if (nnz != op->nnz) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "set_values: nnz differs from the operator's");
    if (nnz > 0 && !nzval) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(op->device));
    if (nnz == 0) return OTMB_OK;
    HIP_TRY(ctx, hipMemcpyAsync(to.nz.p, nzval, (size_t)nnz * 8, kind, ctx->stream));
    if (kind == hipMemcpyHostToDevice) ctx->uploaded_bytes += 8 * nnz;
    hipLaunchKernelGGL(spmv_relayout_kernel, SP_GRID(nnz), (const double *)to.nz.p, (const i64 *)op->dst.p, nnz, (double *)to.val.p);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

template <int KB>
static void sp_launch(otmb_op *op, int adjoint, const double *X, int64_t ldx, double *Y, int64_t ldy, double alpha, double beta, int bmode) {
    hipStream_t s = op->ctx->stream;
    if (adjoint) {
        if (op->n > 0)
            hipLaunchKernelGGL(spmv_cols_kernel<KB>, dim3((unsigned)((op->n + 63) / 64)), dim3(64), 0, s, (const i64 *)op->cp.p, (const int *)op->rv.p,
                               (const double *)op->nz.p, op->n, X, ldx, Y, ldy, alpha, beta, bmode);
    } else if (op->m > 0) {
        hipLaunchKernelGGL(spmv_rows_kernel<KB>, dim3((unsigned)((op->m + 255) / 256)), dim3(256), 0, s, (const double *)op->val.p, (const int *)op->col.p,
                           (const i64 *)op->sbase.p, (const int *)op->elen.p, op->m, X, ldx, Y, ldy, alpha, beta, bmode);
    }
}

static int32_t sp_check_mul(otmb_op *op, int32_t adjoint, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy) {
    otmb_ctx *ctx = op->ctx;
    const i64 rx = adjoint ? op->m : op->n, ry = adjoint ? op->n : op->m;
    if (k < 1 || k >= (1ll << 31)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "k (tracers) must be >= 1");
    if (ldx < rx || ldx < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "ldx is smaller than the rows of X");
    if (ldy < ry || ldy < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "ldy is smaller than the rows of Y");
    if ((rx > 0 && !X) || (ry > 0 && !Y)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    return OTMB_OK;
}

extern "C" {

int32_t otmb_op_create_dev(otmb_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, otmb_op **out) {
    return sp_create(ctx, m, n, colptr, rowval, nzval, out, hipMemcpyDeviceToDevice);
}

int32_t otmb_op_create(otmb_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, otmb_op **out) {
    return sp_create(ctx, m, n, colptr, rowval, nzval, out, hipMemcpyHostToDevice);
}

int32_t otmb_op_set_values_dev(otmb_op *op, const double *nzval, int64_t nnz) { return sp_set_values(op, -1, nzval, nnz, hipMemcpyDeviceToDevice); }

static int32_t sp_set_values_host(otmb_op *op, int64_t slot, const double *nzval, int64_t nnz) {
    const int32_t rc = sp_set_values(op, slot, nzval, nnz, hipMemcpyHostToDevice);
    if (rc == OTMB_OK && op->nnz > 0) HIP_TRY(op->ctx, hipStreamSynchronize(op->ctx->stream));  // (the caller may reuse its array at once)
    return rc;
}
int32_t otmb_op_set_values(otmb_op *op, const double *nzval, int64_t nnz) { return sp_set_values_host(op, -1, nzval, nnz); }

// ---- value slots: nslots copies of nzval / val over ONE pattern (dst, the index arrays and the lines are shared) -------------------
// a slot's array at its exact size (otmb_reserve rounds up by an eighth for buffers that grow; a year of slots does not grow)
static int32_t sp_exact(otmb_op *op, DevBuf &b, size_t bytes) {
    bytes = bytes > 0 ? bytes : 8;
    if (hipMalloc(&b.p, bytes) != hipSuccess) {
        b.p = nullptr;
        (void)hipGetLastError();  // (the refusal is reported here, not by the next call's error check)
        return otmb_fail(op->ctx, OTMB_ERR_ALLOC, "hipMalloc (set_slots)");
    }
    b.cap = bytes;
    return OTMB_OK;
}
static int32_t sp_slot_arg(otmb_op *op, int64_t slot, const char *what) {
    if (slot >= 0 && slot < (i64)op->slots.size()) return OTMB_OK;
    char msg[128];
    snprintf(msg, sizeof msg, "%s: slot %lld is outside 0..%lld (otmb_op_set_slots)", what, (long long)slot, (long long)op->slots.size() - 1);
    return otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, msg);
}
static void sp_select(otmb_op *op, i64 slot) {
    op->sel = slot;
    op->nz = op->slots[(size_t)slot].nz;
    op->val = op->slots[(size_t)slot].val;
}

int32_t otmb_op_set_slots(otmb_op *op, int64_t nslots) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    if (nslots < 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "set_slots: nslots must be >= 1");
    HIP_TRY(ctx, hipSetDevice(op->device));
    const i64 have = (i64)op->slots.size();
    if (nslots > have) {  // every new slot is allocated before the operator changes: a failure leaves the slots it had
        std::vector<OpSlot> add;
        try {  // (the host's table of slots itself: a count no machine can hold is an allocation failure like the device's)
            add.resize((size_t)(nslots - have));
            op->slots.reserve((size_t)nslots);
        } catch (const std::exception &) {
            return otmb_fail(ctx, OTMB_ERR_ALLOC, "set_slots: the table of slots");
        }
        int32_t rc = OTMB_OK;
        for (OpSlot &s : add)
            if ((rc = sp_exact(op, s.nz, (size_t)op->nnz * 8)) || (rc = sp_exact(op, s.val, (size_t)op->nval * 8))) break;
        hipError_t e = hipSuccess;
        for (OpSlot &s : add) {  // a device copy of the selected slot: never undefined
            if (rc || e != hipSuccess) break;
            if (op->nnz > 0) e = hipMemcpyAsync(s.nz.p, op->nz.p, (size_t)op->nnz * 8, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess && op->nval > 0) e = hipMemcpyAsync(s.val.p, op->val.p, (size_t)op->nval * 8, hipMemcpyDeviceToDevice, ctx->stream);
        }
        if (rc || e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);
            for (OpSlot &s : add) {
                otmb_free(s.nz);
                otmb_free(s.val);
            }
            return rc ? rc : otmb_fail(ctx, OTMB_ERR_HIP, "set_slots: copying the selected slot");
        }
        op->slots.insert(op->slots.end(), add.begin(), add.end());
    } else if (nslots < have) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (enqueued work may still read the slots that go; a failure changes nothing)
        if (op->sel >= nslots) sp_select(op, 0);
        for (i64 s = nslots; s < have; ++s) {
            otmb_free(op->slots[(size_t)s].nz);
            otmb_free(op->slots[(size_t)s].val);
        }
        op->slots.resize((size_t)nslots);
    }
    return OTMB_OK;
}

// a pointer switch: nothing is enqueued, no data moves; products, solves and preconditioners enqueued from now on read this slot
int32_t otmb_op_select_slot(otmb_op *op, int64_t slot) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sp_slot_arg(op, slot, "select_slot"))) return rc;
    sp_select(op, slot);
    return OTMB_OK;
}

int32_t otmb_op_slots(const otmb_op *op, int64_t *nslots, int64_t *selected) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    if (nslots) *nslots = (int64_t)op->slots.size();
    if (selected) *selected = op->sel;
    return OTMB_OK;
}

int32_t otmb_op_set_values_slot_dev(otmb_op *op, int64_t slot, const double *nzval, int64_t nnz) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sp_slot_arg(op, slot, "set_values_slot"))) return rc;
    return sp_set_values(op, slot, nzval, nnz, hipMemcpyDeviceToDevice);
}

int32_t otmb_op_set_values_slot(otmb_op *op, int64_t slot, const double *nzval, int64_t nnz) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sp_slot_arg(op, slot, "set_values_slot"))) return rc;
    return sp_set_values_host(op, slot, nzval, nnz);
}

int32_t otmb_op_mul_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, double alpha, double beta) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sp_check_mul(op, adjoint, k, X, ldx, Y, ldy))) return rc;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    const int bmode = beta == 0.0 ? 0 : (beta == 1.0 ? 1 : 2);
    op_blocks<8>(0, k, [&](auto kb, i64 c0) {
        sp_launch<decltype(kb)::value>(op, adjoint, X ? X + c0 * ldx : nullptr, ldx, Y ? Y + c0 * ldy : nullptr, ldy, alpha, beta, bmode);
    });
    if (!adjoint && op->nlong > 0)
        hipLaunchKernelGGL(spmv_long_kernel, dim3((unsigned)op->nlong), dim3(64), 0, ctx->stream, (const double *)op->val.p, (const int *)op->col.p,
                           (const i64 *)op->lrows.p, (const i64 *)op->loff.p, op->ell, (int)k, X, ldx, Y, ldy, alpha, beta, bmode);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_op_mul(otmb_op *op, int32_t adjoint, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, double alpha, double beta) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sp_check_mul(op, adjoint, k, X, ldx, Y, ldy))) return rc;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    const i64 rx = adjoint ? op->m : op->n, ry = adjoint ? op->n : op->m;
    if ((rc = op_reserve_xy(op, rx, ry, k))) return rc;
    double *dx = (double *)op->xs.p, *dy = (double *)op->ys.p;
    if (rx > 0 && (rc = op_upload(ctx, dx, X, ldx, rx, k))) return rc;
    if (ry > 0 && beta != 0.0 && (rc = op_upload(ctx, dy, Y, ldy, ry, k))) return rc;  // (β == 0 discards Y)
    if ((rc = otmb_op_mul_dev(op, adjoint, k, dx, rx, dy, ry, alpha, beta))) return rc;
    return op_finish(ctx, OTMB_OK, Y, ldy, dy, ry, k);
}

int32_t otmb_op_info(const otmb_op *op, int64_t *m, int64_t *n, int64_t *nnz) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    if (m) *m = op->m;
    if (n) *n = op->n;
    if (nnz) *nnz = op->nnz;
    return OTMB_OK;
}

// touches no context (a finalizer may call it after the context is gone): the operator's own device buffers only
void otmb_op_destroy(otmb_op *op) {
    if (!op) return;
    (void)hipSetDevice(op->device);
    (void)hipDeviceSynchronize();
    sp_free_all(op);
    delete op;
}

}  // extern "C"
