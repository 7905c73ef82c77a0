// otmb_submatrix.hip -- the resident operator's domain: A[rows, cols] as a new operator (otmb_op_submatrix[_dev]), the refresh of its value
// slots from the parent's (otmb_op_take_values), and what an operator can say of itself (otmb_op_fetch[_dev], otmb_op_get_lines[_dev]).
// include/otmb.h states the contract; tests/submatrix_ref.py restates the rule.
//
// The plan of a submatrix is entry-parallel and deterministic: no lane walks a column or a row, nothing whose order matters is an atomic.
//   1  rank tables: rrank[i] / crank[j] = the position of row i / column j in the selection, -1 when dropped (Int32; the same kernel checks
//      the lists -- strictly ascending inside 1..m / 1..n -- and whether the selection is principal);
//   2  keep[e] = 1 when the parent's stored entry e lies in a selected row and column (its column is col[dst[e]] of the parent's row layout);
//   3  pos = the exclusive scan of keep (otmb_prims.h): the child's position of every kept entry, pos[nnz] = the child's nnz;
//   4  colptr'[j'] = 1 + pos[colptr[cols[j']] - 1], colptr'[nc] = 1 + pos[nnz]: dropped columns hold no kept entry in between;
//   5  every kept entry to pos[e]: its row's rank (Int64, 1-based: what the plan of otmb_op_create_dev reads), src[pos[e]] = e (the gather
//      table the child keeps) and the value of the parent's slot 0.
// The child is then planned by sp_plan_resident (otmb_spmv.hip), as otmb_op_create_dev plans the arrays a caller gives: the same checks, layouts
// and bits.  Slots beyond the first are filled by sub_take_kernel, one streaming launch per slot, which otmb_op_take_values runs again when
// the parent's values have changed: per child entry p, v = parent_nz[src[p]], nz[p] = v, val[dst[p]] = v -- the gather fused with the scatter of
// spmv_relayout_kernel, two entries per lane (16-byte loads of src and dst, a 16-byte store of nz), no temporary nzval.
#include <hip/hip_runtime.h>

#include "otmb_op.h"
#include "otmb_prims.h"

typedef unsigned long long ull;

// ---- the plan's kernels ------------------------------------------------------------------------------------------------------------------
// rank[idx[p] - 1] = p for a list idx (1-based) that must ascend strictly inside 1..lim; bad = the first position p (0-based) whose entry is
// outside 1..lim or not above its predecessor.  rank is preset to -1; an entry outside 1..lim writes nothing.  other: a second list of the
// same length; differs = 1 when some position differs (the selection is then not principal).
__global__ __launch_bounds__(256) void sub_rank_kernel(const i64 *__restrict__ idx, i64 cnt, i64 lim, int *__restrict__ rank, ull *__restrict__ bad,
                                                       const i64 *__restrict__ other, unsigned *__restrict__ differs) {
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < cnt; p += (i64)gridDim.x * 256) {
        const i64 v = idx[p];
        const bool inside = v >= 1 && v <= lim;
        if (!inside || (p > 0 && idx[p - 1] >= v)) atomicMin(bad, (ull)p);
        if (inside) rank[v - 1] = (int)p;
        if (other && other[p] != v) atomicOr(differs, 1u);
    }
}
// keep[e] = the parent's entry e survives (e = nnz: 0, so that the scan's last value is the total)
__global__ __launch_bounds__(256) void sub_keep_kernel(const int *__restrict__ rv, const int *__restrict__ col, const i64 *__restrict__ dst, i64 nnz,
                                                       const int *__restrict__ rrank, const int *__restrict__ crank, i64 *__restrict__ keep) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e <= nnz; e += (i64)gridDim.x * 256)
        keep[e] = e < nnz && rrank[rv[e]] >= 0 && crank[col[dst[e]]] >= 0;
}
// the child's colptr: one read of the scan per selected column
__global__ __launch_bounds__(256) void sub_colptr_kernel(const i64 *__restrict__ cp, const i64 *__restrict__ cols, i64 nc, const i64 *__restrict__ pos, i64 nnz,
                                                         i64 *__restrict__ out) {
    for (i64 j = (i64)blockIdx.x * 256 + threadIdx.x; j <= nc; j += (i64)gridDim.x * 256) out[j] = 1 + pos[j < nc ? cp[cols[j] - 1] - 1 : nnz];
}
// every kept entry to its scanned position: the row's rank (1-based), the gather table and the value of the parent's first slot
__global__ __launch_bounds__(256) void sub_scatter_kernel(const i64 *__restrict__ keep, const i64 *__restrict__ pos, const int *__restrict__ rv,
                                                          const double *__restrict__ pnz, i64 nnz, const int *__restrict__ rrank, i64 *__restrict__ rows,
                                                          i64 *__restrict__ src, double *__restrict__ nz) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (i64)gridDim.x * 256) {
        if (!keep[e]) continue;
        const i64 p = pos[e];
        rows[p] = (i64)rrank[rv[e]] + 1;
        src[p] = e;
        nz[p] = pnz[e];
    }
}
// next'[rank(i)] = rank(next[i]) + 1 when i and next[i] are both selected, otherwise 0 (nxt: the parent's Int32 table, -1 = none)
__global__ __launch_bounds__(256) void sub_lines_kernel(const i64 *__restrict__ rows, i64 nr, const int *__restrict__ nxt, const int *__restrict__ rrank,
                                                        i64 *__restrict__ next) {
    for (i64 p = (i64)blockIdx.x * 256 + threadIdx.x; p < nr; p += (i64)gridDim.x * 256) {
        const int j = nxt[rows[p] - 1];
        next[p] = j >= 0 ? (i64)rrank[j] + 1 : 0;  // (a dropped successor has rank -1: 0, the line ends here)
    }
}

// ---- the value gather: a slot of the child from a slot of the parent ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sub_take_kernel(const double *__restrict__ pnz, const i64 *__restrict__ src, const i64 *__restrict__ dst, i64 nnz,
                                                       double *__restrict__ nz, double *__restrict__ val) {
    const i64 pairs = nnz >> 1;  // (src, dst and nz are allocations of their own: entry 2q lies on a 16-byte boundary)
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < pairs; q += (i64)gridDim.x * 256) {
        const longlong2 s = ((const longlong2 *)src)[q], d = ((const longlong2 *)dst)[q];
        double2 v;
        v.x = pnz[s.x];
        v.y = pnz[s.y];
        ((double2 *)nz)[q] = v;
        val[d.x] = v.x;
        val[d.y] = v.y;
    }
    if ((nnz & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const double v = pnz[src[nnz - 1]];
        nz[nnz - 1] = v;
        val[dst[nnz - 1]] = v;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
// the Int32 row indices (0-based) and successors (-1 = none) back as otmb_op_create / otmb_op_set_lines took them: + 1, Int64
static void sb_widen(hipStream_t st, const int *in, i64 cnt, i64 *out) { otmb_widen(st, in, cnt, 1, out); }

static void sb_take(otmb_op *child, const double *pnz, const OpSlot &to) {
    hipLaunchKernelGGL(sub_take_kernel, OTMB_GRID_STRIDE((child->nnz + 1) / 2, child->ctx->stream), pnz, (const i64 *)child->src.p, (const i64 *)child->dst.p, child->nnz,
                       (double *)to.nz.p, (double *)to.val.p);
}

static int32_t sb_bad_index(otmb_ctx *ctx, const char *what, ull pos, i64 lim) {
    char msg[192];
    snprintf(msg, sizeof msg, "submatrix: the %s index at position %llu is outside 1..%lld or not above the one before it (1-based; the first such position; "
             "the lists must ascend strictly)", what, pos + 1, (long long)lim);
    return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
}

extern "C" void otmb_op_destroy(otmb_op *op);

// rows, cols: device pointers
static int32_t sb_submatrix(otmb_op *parent, i64 nr, const i64 *rows, i64 nc, const i64 *cols, otmb_op **out) {
    otmb_ctx *ctx = parent->ctx;
    hipStream_t st = ctx->stream;
    const i64 m = parent->m, n = parent->n, nnz = parent->nnz;
    int32_t rc;
    DevScratch S;
    DevBuf &ranks = S.add(), &words = S.add();
    if ((rc = otmb_reserve_some(ctx, ranks, (size_t)(m + n) * 4))) return rc;
    if ((rc = otmb_reserve_some(ctx, words, 24))) return rc;
    int *rrank = (int *)ranks.p, *crank = rrank + m;
    ull *bad = (ull *)words.p;  // the first offending row position, column position; whether rows and cols differ
    unsigned *differs = (unsigned *)(bad + 2);
    if (m + n > 0) HIP_TRY(ctx, hipMemsetAsync(rrank, 0xff, (size_t)(m + n) * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(bad, 0xff, 16, st));
    HIP_TRY(ctx, hipMemsetAsync(differs, 0, 8, st));
    if (nr > 0) hipLaunchKernelGGL(sub_rank_kernel, OTMB_GRID_STRIDE(nr, st), rows, nr, m, rrank, bad, (const i64 *)nullptr, differs);
    if (nc > 0) hipLaunchKernelGGL(sub_rank_kernel, OTMB_GRID_STRIDE(nc, st), cols, nc, n, crank, bad + 1, nr == nc ? rows : (const i64 *)nullptr, differs);
    HIP_TRY(ctx, hipGetLastError());
    ull hw[3] = {0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(hw, bad, 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (hw[0] != ~0ull) return sb_bad_index(ctx, "row", hw[0], m);
    if (hw[1] != ~0ull) return sb_bad_index(ctx, "column", hw[1], n);
    const bool principal = nr == nc && (unsigned)hw[2] == 0;
    // the kept entries and their positions
    DevBuf &keepb = S.add(), &posb = S.add(), &tmpb = S.add();
    if ((rc = otmb_reserve_some(ctx, keepb, (size_t)(nnz + 1) * 8))) return rc;
    if ((rc = otmb_reserve_some(ctx, posb, (size_t)(nnz + 1) * 8))) return rc;
    i64 *keep = (i64 *)keepb.p, *pos = (i64 *)posb.p;
    hipLaunchKernelGGL(sub_keep_kernel, OTMB_GRID_STRIDE(nnz + 1, st), (const int *)parent->rv.p, (const int *)parent->col.p, (const i64 *)parent->dst.p, nnz,
                       (const int *)rrank, (const int *)crank, keep);
    if ((rc = otmb_exclusive_scan(ctx, tmpb, keep, pos, nnz + 1))) return rc;
    HIP_TRY(ctx, hipGetLastError());
    i64 total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, pos + nnz, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (total < 0 || total > nnz) return otmb_fail(ctx, OTMB_ERR_HIP, "submatrix: the count of kept entries");  // (cannot happen)
    // the child: its arrays, then the plan of otmb_op_create_dev
    struct Guard {  // the operator is handed out only when everything succeeded
        otmb_op *op = new otmb_op();
        ~Guard() { otmb_op_destroy(op); }
    } G;
    otmb_op *op = G.op;
    op->ctx = ctx;
    op->device = parent->device;
    op->m = nr;
    op->n = nc;
    op->nnz = total;
    DevBuf &rowsb = S.add();
    if ((rc = otmb_reserve_some(ctx, op->cp, (size_t)(nc + 1) * 8))) return rc;
    if ((rc = otmb_reserve_some(ctx, rowsb, (size_t)total * 8))) return rc;
    if ((rc = otmb_reserve_some(ctx, op->nz, (size_t)total * 8))) return rc;
    if ((rc = otmb_reserve_some(ctx, op->src, (size_t)total * 8))) return rc;
    hipLaunchKernelGGL(sub_colptr_kernel, OTMB_GRID_STRIDE(nc + 1, st), (const i64 *)parent->cp.p, cols, nc, (const i64 *)pos, nnz, (i64 *)op->cp.p);
    if (total > 0)
        hipLaunchKernelGGL(sub_scatter_kernel, OTMB_GRID_STRIDE(nnz, st), (const i64 *)keep, (const i64 *)pos, (const int *)parent->rv.p,
                           (const double *)parent->slots[0].nz.p, nnz, (const int *)rrank, (i64 *)rowsb.p, (i64 *)op->src.p, (double *)op->nz.p);
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = sp_plan_resident(op, (const i64 *)rowsb.p))) return rc;
    // the parent's other slots, restricted; its selection
    const size_t ns = parent->slots.size();
    if (ns > 1 && (rc = otmb_op_set_slots(op, (int64_t)ns))) return rc;
    for (size_t s = 1; s < ns && total > 0; ++s) sb_take(op, (const double *)parent->slots[s].nz.p, op->slots[s]);
    HIP_TRY(ctx, hipGetLastError());
    if (parent->sel != 0 && (rc = otmb_op_select_slot(op, parent->sel))) return rc;
    // the lines of a principal selection, through the line setup that makes the predecessor and head tables
    if (principal && parent->lines && parent->m == parent->n) {
        DevBuf &nextb = S.add();
        if ((rc = otmb_reserve_some(ctx, nextb, (size_t)nr * 8))) return rc;
        if (nr > 0) hipLaunchKernelGGL(sub_lines_kernel, OTMB_GRID_STRIDE(nr, st), rows, nr, (const int *)parent->ln.p, (const int *)rrank, (i64 *)nextb.p);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = otmb_op_set_lines_dev(op, (const int64_t *)nextb.p))) return rc;
    }
    op->parent_serial = parent->serial;
    op->parent_nnz = nnz;
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (the scratch goes when this returns)
    *out = op;
    G.op = nullptr;
    return OTMB_OK;
}

static int32_t sb_submatrix_args(otmb_op *parent, int64_t nr, const int64_t *rows, int64_t nc, const int64_t *cols, otmb_op **out) {
    if (!parent) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = parent->ctx;
    if (!out) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (nr < 0 || nc < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "submatrix: nr and nc must be >= 0");
    if ((nr > 0 && !rows) || (nc > 0 && !cols)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(parent->device));
    return OTMB_OK;
}

// slot (-1: the selected one) of an operator, or the refusal
static int32_t sb_slot(const otmb_op *op, int64_t slot, const char *what, const OpSlot *&s) {
    if (slot < -1 || slot >= (i64)op->slots.size()) {
        char msg[160];
        snprintf(msg, sizeof msg, "%s: slot %lld is outside 0..%lld (otmb_op_set_slots)", what, (long long)slot, (long long)op->slots.size() - 1);
        return otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, msg);
    }
    s = &op->slots[(size_t)(slot < 0 ? op->sel : slot)];
    return OTMB_OK;
}

extern "C" {

int32_t otmb_op_submatrix_dev(otmb_op *parent, int64_t nr, const int64_t *rows, int64_t nc, const int64_t *cols, otmb_op **out) {
    int32_t rc;
    if ((rc = sb_submatrix_args(parent, nr, rows, nc, cols, out))) return rc;
    return sb_submatrix(parent, nr, rows, nc, cols, out);
}

int32_t otmb_op_submatrix(otmb_op *parent, int64_t nr, const int64_t *rows, int64_t nc, const int64_t *cols, otmb_op **out) {
    int32_t rc;
    if ((rc = sb_submatrix_args(parent, nr, rows, nc, cols, out))) return rc;
    otmb_ctx *ctx = parent->ctx;
    DevScratch S;
    DevBuf &lists = S.add();
    if ((rc = otmb_reserve_some(ctx, lists, (size_t)(nr + nc) * 8))) return rc;
    i64 *dr = (i64 *)lists.p, *dc = dr + nr;
    if (nr > 0) HIP_TRY(ctx, hipMemcpyAsync(dr, rows, (size_t)nr * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nc > 0) HIP_TRY(ctx, hipMemcpyAsync(dc, cols, (size_t)nc * 8, hipMemcpyHostToDevice, ctx->stream));
    ctx->uploaded_bytes += 8 * (nr + nc);
    return sb_submatrix(parent, nr, dr, nc, dc, out);  // (it waits for the stream before it returns: the caller may reuse its lists at once)
}

int32_t otmb_op_take_values(otmb_op *child, const otmb_op *parent, int64_t parent_slot, int64_t child_slot) {
    if (!child) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = child->ctx;
    if (!parent) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (child->parent_serial == 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "take_values: the operator was not made by otmb_op_submatrix");
    if (parent->serial != child->parent_serial || parent->ctx != ctx || parent->nnz != child->parent_nnz)
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "take_values: the operator given is not the one this submatrix was taken from");
    const OpSlot *from = nullptr, *to = nullptr;
    int32_t rc;
    if (parent_slot < 0 || child_slot < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "take_values: a slot is negative (there is no \"selected slot\" here)");
    if ((rc = sb_slot(parent, parent_slot, "take_values (parent)", from))) return rc;  // (the parent is on this context: the message is where the caller looks)
    if ((rc = sb_slot(child, child_slot, "take_values", to))) return rc;
    HIP_TRY(ctx, hipSetDevice(child->device));
    if (child->nnz == 0) return OTMB_OK;
    sb_take(child, (const double *)from->nz.p, *to);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_op_fetch_dev(const otmb_op *op, int64_t slot, int64_t *colptr, int64_t *rowval, double *nzval) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    const OpSlot *from = nullptr;
    int32_t rc;
    if ((rc = sb_slot(op, slot, "fetch", from))) return rc;
    HIP_TRY(ctx, hipSetDevice(op->device));
    hipStream_t st = ctx->stream;
    if (colptr) HIP_TRY(ctx, hipMemcpyAsync(colptr, op->cp.p, (size_t)(op->n + 1) * 8, hipMemcpyDeviceToDevice, st));
    if (rowval && op->nnz > 0) sb_widen(st, (const int *)op->rv.p, op->nnz, rowval);
    if (nzval && op->nnz > 0) HIP_TRY(ctx, hipMemcpyAsync(nzval, from->nz.p, (size_t)op->nnz * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_op_fetch(const otmb_op *op, int64_t slot, int64_t *colptr, int64_t *rowval, double *nzval) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    const OpSlot *from = nullptr;
    int32_t rc;
    if ((rc = sb_slot(op, slot, "fetch", from))) return rc;
    HIP_TRY(ctx, hipSetDevice(op->device));
    hipStream_t st = ctx->stream;
    DevScratch S;
    if (colptr) HIP_TRY(ctx, hipMemcpyAsync(colptr, op->cp.p, (size_t)(op->n + 1) * 8, hipMemcpyDeviceToHost, st));
    if (rowval && op->nnz > 0) {  // widened on the device, in scratch: the operator is not touched
        DevBuf &wide = S.add();
        if ((rc = otmb_reserve_some(ctx, wide, (size_t)op->nnz * 8))) return rc;
        sb_widen(st, (const int *)op->rv.p, op->nnz, (i64 *)wide.p);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(rowval, wide.p, (size_t)op->nnz * 8, hipMemcpyDeviceToHost, st));
    }
    if (nzval && op->nnz > 0) HIP_TRY(ctx, hipMemcpyAsync(nzval, from->nz.p, (size_t)op->nnz * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return OTMB_OK;
}

int32_t otmb_op_get_lines_dev(const otmb_op *op, int64_t *next, int32_t *has_lines) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    if (has_lines) *has_lines = op->lines ? 1 : 0;
    if (!op->lines || !next || op->n == 0) return OTMB_OK;
    HIP_TRY(ctx, hipSetDevice(op->device));
    sb_widen(ctx->stream, (const int *)op->ln.p, op->n, next);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_op_get_lines(const otmb_op *op, int64_t *next, int32_t *has_lines) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    if (has_lines) *has_lines = op->lines ? 1 : 0;
    if (!op->lines || !next || op->n == 0) return OTMB_OK;
    HIP_TRY(ctx, hipSetDevice(op->device));
    DevScratch S;
    DevBuf &wide = S.add();
    int32_t rc;
    if ((rc = otmb_reserve_some(ctx, wide, (size_t)op->n * 8))) return rc;
    sb_widen(ctx->stream, (const int *)op->ln.p, op->n, (i64 *)wide.p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(next, wide.p, (size_t)op->n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OTMB_OK;
}

}  // extern "C"
