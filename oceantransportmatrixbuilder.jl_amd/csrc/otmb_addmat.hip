// otmb_addmat.hip -- slot = slot + α·B in place on a resident operator, for a matrix B whose pattern lies inside the operator's:
// otmb_op_add_matrix[_dev].  include/otmb.h states the contract; tests/sink_ref.py restates it by positions (add_matrix_ref).
//
// Three steps, the first two once per call, whatever the number of slots:
//   check   B's colptr (non-decreasing inside [1, nnz(B) + 1]) and rows (1..m), before anything is read through them;
//   match   one lane per column c: each stored entry e of B's column, in stored order, is looked up in the operator's column c, in stored
//           order: pos[e] = the FIRST position with e's row, or a miss (the smallest missed e wins an atomicMin).  The same lane notes
//           whether two entries of its column found one position: B then has duplicates, and the update must keep their order.
//   update  ONE launch for all requested slots.  Without duplicates: one lane per entry e of B, t = α·B[e] once, then for every slot
//           v = nz[p] + t, stored to nz[p] and to val[dst[p]] (the row layout's copy: the same bits).  With duplicates: one lane per column
//           of B walks its entries in stored order, so the additions into one position happen in B's stored order.
// Up to AM_ARGS slots' two pointers travel as kernel arguments (AM_ARGS pairs: 16 pointers); more come from a table on the device (op->am).
// Nothing is written before the match has passed: after any refusal every slot has the bits it had.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "otmb_op.h"
#include "otmb_prims.h"

#define AM_ARGS 8  // slots whose pointers travel as kernel arguments

enum { AM_BAD_CP = 1, AM_BAD_RV = 2, AM_DUP = 4 };

struct AmSlots {
    double *nz[AM_ARGS], *val[AM_ARGS];
};
struct AmState {  // the words the kernels leave for the host
    unsigned flags, pad;
    unsigned long long miss;  // the smallest entry of B without a partner (0-based); ~0: none
};

__global__ __launch_bounds__(256) void am_check_colptr_kernel(const i64 *__restrict__ p, i64 n, i64 nnz, AmState *__restrict__ st) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < n; c += (i64)gridDim.x * 256) {
        const i64 a = p[c], b = p[c + 1];
        if (a < 1 || b < a || b > nnz + 1) atomicOr(&st->flags, (unsigned)AM_BAD_CP);
    }
}
__global__ __launch_bounds__(256) void am_check_rowval_kernel(const i64 *__restrict__ r, i64 nnz, i64 m, AmState *__restrict__ st) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (i64)gridDim.x * 256) {
        const i64 i = r[e];
        if (i < 1 || i > m) atomicOr(&st->flags, (unsigned)AM_BAD_RV);
    }
}

// B's colptr and rows have passed their checks; the operator's own arrays (cp: Int64, 1-based; rv: Int32, 0-based) passed theirs at its creation
__global__ __launch_bounds__(256) void am_match_kernel(const i64 *__restrict__ bp, const i64 *__restrict__ bi, i64 n, const i64 *__restrict__ cp,
                                                       const int *__restrict__ rv, i64 *__restrict__ pos, AmState *__restrict__ st) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < n; c += (i64)gridDim.x * 256) {
        const i64 e0 = bp[c] - 1, e1 = bp[c + 1] - 1, a0 = cp[c] - 1, a1 = cp[c + 1] - 1;
        for (i64 e = e0; e < e1; ++e) {
            const int r = (int)(bi[e] - 1);
            i64 p = -1;
            for (i64 j = a0; j < a1; ++j)
                if (rv[j] == r) {
                    p = j;
                    break;
                }
            pos[e] = p;
            if (p < 0) {
                atomicMin(&st->miss, (unsigned long long)e);
                continue;
            }
            for (i64 f = e0; f < e; ++f)
                if (bi[f] == bi[e]) {
                    atomicOr(&st->flags, (unsigned)AM_DUP);
                    break;
                }
        }
    }
}

__device__ __forceinline__ void am_add(const AmSlots &q, const double *const *tab, int ns, i64 p, i64 d, double t) {
    for (int s = 0; s < ns; ++s) {
        double *nz = tab ? (double *)tab[s] : q.nz[s];
        double *val = tab ? (double *)tab[ns + s] : q.val[s];
        const double v = nz[p] + t;
        nz[p] = v;
        val[d] = v;
    }
}

// tab: ns nz pointers, then ns val pointers (device), or null: q's
__global__ __launch_bounds__(256) void am_update_kernel(AmSlots q, const double *const *__restrict__ tab, int ns, const i64 *__restrict__ pos,
                                                        const double *__restrict__ bx, i64 nnzb, const i64 *__restrict__ dst, double alpha) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < nnzb; e += (i64)gridDim.x * 256) {
        const i64 p = pos[e];
        const double t = alpha * bx[e];
        am_add(q, tab, ns, p, dst[p], t);
    }
}
// B stores some position twice: a column's entries one after the other
__global__ __launch_bounds__(256) void am_update_cols_kernel(AmSlots q, const double *const *__restrict__ tab, int ns, const i64 *__restrict__ bp, i64 n,
                                                             const i64 *__restrict__ pos, const double *__restrict__ bx, const i64 *__restrict__ dst,
                                                             double alpha) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < n; c += (i64)gridDim.x * 256)
        for (i64 e = bp[c] - 1; e < bp[c + 1] - 1; ++e) {
            const i64 p = pos[e];
            const double t = alpha * bx[e];
            am_add(q, tab, ns, p, dst[p], t);
        }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the requested slots, checked: nsel different slots of the operator, or every slot (slots == NULL)
static int32_t am_slots(otmb_op *op, i64 nsel, const i64 *slots, std::vector<i64> &out) {
    otmb_ctx *ctx = op->ctx;
    const i64 nslots = (i64)op->slots.size();
    out.clear();
    if (!slots) {
        for (i64 s = 0; s < nslots; ++s) out.push_back(s);
        return OTMB_OK;
    }
    if (nsel < 0 || nsel > nslots) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: the number of requested slots is outside 0..nslots");
    std::vector<char> seen((size_t)nslots, 0);
    for (i64 q = 0; q < nsel; ++q) {
        const i64 s = slots[q];
        char msg[160];
        if (s < 0 || s >= nslots) {
            snprintf(msg, sizeof msg, "add_matrix: slot %lld is outside 0..%lld (otmb_op_set_slots)", (long long)s, (long long)nslots - 1);
            return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
        }
        if (seen[(size_t)s]) {
            snprintf(msg, sizeof msg, "add_matrix: slot %lld is requested twice", (long long)s);
            return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
        }
        seen[(size_t)s] = 1;
        out.push_back(s);
    }
    return OTMB_OK;
}

// B on the device, nnzb known and colptr's two ends checked
static int32_t am_run(otmb_op *op, const i64 *bp, const i64 *bi, const double *bx, i64 nnzb, double alpha, const std::vector<i64> &sel) {
    otmb_ctx *ctx = op->ctx;
    const i64 m = op->m, n = op->n;
    hipStream_t st = ctx->stream;
    const size_t ns = sel.size();
    // op->am: the state words | pos (nnzb) | the table of pointers (2·ns, beyond AM_ARGS)
    DevArena A;
    const size_t o_st = A.take(sizeof(AmState)), o_pos = A.take((size_t)nnzb * 8), o_tab = A.take(ns > AM_ARGS ? 2 * ns * 8 : 0);
    int32_t rc;
    if ((rc = otmb_reserve_some(ctx, op->am, A.total()))) return rc;
    char *base = (char *)op->am.p;
    AmState *dstate = (AmState *)(base + o_st);
    i64 *pos = (i64 *)(base + o_pos);
    AmState h = {0u, 0u, ~0ull};
    HIP_TRY(ctx, hipMemsetAsync(dstate, 0xff, sizeof(AmState), st));  // miss = ~0 (none), then no flags
    HIP_TRY(ctx, hipMemsetAsync(dstate, 0, 8, st));
    if (n > 0) hipLaunchKernelGGL(am_check_colptr_kernel, OTMB_GRID_STRIDE(n, st), bp, n, nnzb, dstate);
    if (nnzb > 0) hipLaunchKernelGGL(am_check_rowval_kernel, OTMB_GRID_STRIDE(nnzb, st), bi, nnzb, m, dstate);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&h, dstate, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h.flags & AM_BAD_CP) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: colptr not non-decreasing inside [1, nnz + 1]");
    if (h.flags & AM_BAD_RV) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: row index outside 1:m");
    if (nnzb == 0) return OTMB_OK;
    hipLaunchKernelGGL(am_match_kernel, OTMB_GRID_STRIDE(n, st), bp, bi, n, (const i64 *)op->cp.p, (const int *)op->rv.p, pos, dstate);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(&h, dstate, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h.miss != ~0ull) {  // name it: its row, and its column by a search of B's colptr (an error path: the column pointers come to the host)
        const i64 e = (i64)h.miss;
        i64 row = 0;
        std::vector<i64> cp((size_t)n + 1);
        HIP_TRY(ctx, hipMemcpy(&row, bi + e, 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(cp.data(), bp, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost));
        const i64 col = (i64)(std::upper_bound(cp.begin(), cp.end(), e + 1) - cp.begin());  // the last column that starts at or before e
        char msg[200];
        snprintf(msg, sizeof msg, "add_matrix: entry %lld of B, (row %lld, column %lld), is not stored in the operator", (long long)e + 1, (long long)row,
                 (long long)col);
        return otmb_fail(ctx, OTMB_ERR_PATTERN_NOT_CONTAINED, msg);
    }
    if (alpha == 0.0 || ns == 0) return OTMB_OK;
    AmSlots q = {};
    const double *const *tab = nullptr;
    if (ns > AM_ARGS) {
        std::vector<unsigned long long> host(2 * ns);
        for (size_t s = 0; s < ns; ++s) {
            host[s] = (unsigned long long)(uintptr_t)op->slots[(size_t)sel[s]].nz.p;
            host[ns + s] = (unsigned long long)(uintptr_t)op->slots[(size_t)sel[s]].val.p;
        }
        HIP_TRY(ctx, hipMemcpy(base + o_tab, host.data(), host.size() * 8, hipMemcpyHostToDevice));  // (the stream is idle: synchronised above)
        tab = (const double *const *)(base + o_tab);
    } else {
        for (size_t s = 0; s < ns; ++s) {
            q.nz[s] = (double *)op->slots[(size_t)sel[s]].nz.p;
            q.val[s] = (double *)op->slots[(size_t)sel[s]].val.p;
        }
    }
    if (h.flags & AM_DUP)
        hipLaunchKernelGGL(am_update_cols_kernel, OTMB_GRID_STRIDE(n, st), q, tab, (int)ns, bp, n, (const i64 *)pos, bx, (const i64 *)op->dst.p, alpha);
    else
        hipLaunchKernelGGL(am_update_kernel, OTMB_GRID_STRIDE(nnzb, st), q, tab, (int)ns, (const i64 *)pos, bx, nnzb, (const i64 *)op->dst.p, alpha);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

static int32_t am_check_args(otmb_op *op, i64 m, i64 n, const i64 *colptr, double alpha) {
    otmb_ctx *ctx = op->ctx;
    if (m != op->m || n != op->n) {
        char msg[160];
        snprintf(msg, sizeof msg, "add_matrix: B is %lld x %lld, the operator %lld x %lld", (long long)m, (long long)n, (long long)op->m, (long long)op->n);
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
    }
    if (!colptr) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (!std::isfinite(alpha)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: alpha is not finite");
    return OTMB_OK;
}
static int32_t am_check_ends(otmb_op *op, i64 first, i64 last, const i64 *rowval, const double *nzval) {
    otmb_ctx *ctx = op->ctx;
    if (first != 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: colptr[1] must be 1");
    if (last < 1) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: colptr[n + 1] - 1 (nnz) is negative");
    if (last - 1 >= (1ll << 40)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "add_matrix: matrix too large");
    if (last > 1 && (!rowval || !nzval)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    return OTMB_OK;
}

extern "C" {

int32_t otmb_op_add_matrix_dev(otmb_op *op, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, double alpha,
                               int64_t nsel, const int64_t *slots) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    int32_t rc;
    std::vector<i64> sel;
    if ((rc = am_check_args(op, m, n, colptr, alpha)) || (rc = am_slots(op, nsel, slots, sel))) return rc;
    HIP_TRY(ctx, hipSetDevice(op->device));
    i64 e[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&e[0], colptr, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&e[1], colptr + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = am_check_ends(op, e[0], e[1], rowval, nzval))) return rc;
    return am_run(op, colptr, rowval, nzval, e[1] - 1, alpha, sel);
}

int32_t otmb_op_add_matrix(otmb_op *op, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, double alpha,
                           int64_t nsel, const int64_t *slots) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    int32_t rc;
    std::vector<i64> sel;
    if ((rc = am_check_args(op, m, n, colptr, alpha)) || (rc = am_slots(op, nsel, slots, sel))) return rc;
    if ((rc = am_check_ends(op, colptr[0], colptr[n], rowval, nzval))) return rc;
    HIP_TRY(ctx, hipSetDevice(op->device));
    const i64 nnzb = colptr[n] - 1;
    DevArena A;
    const size_t o_p = A.take((size_t)(n + 1) * 8), o_i = A.take((size_t)nnzb * 8), o_x = A.take((size_t)nnzb * 8);
    DevScratch S;
    DevBuf &stage = S.add();
    if ((rc = otmb_reserve_some(ctx, stage, A.total()))) return rc;
    char *base = (char *)stage.p;
    HIP_TRY(ctx, hipMemcpyAsync(base + o_p, colptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nnzb > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(base + o_i, rowval, (size_t)nnzb * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(base + o_x, nzval, (size_t)nnzb * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    ctx->uploaded_bytes += 8 * (n + 1) + 16 * nnzb;
    rc = am_run(op, (const i64 *)(base + o_p), (const i64 *)(base + o_i), (const double *)(base + o_x), nnzb, alpha, sel);
    const std::string msg = ctx->err;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (the uploads read the caller's arrays; the staging goes with this call)
    ctx->err = msg;
    return rc;
}

}  // extern "C"
