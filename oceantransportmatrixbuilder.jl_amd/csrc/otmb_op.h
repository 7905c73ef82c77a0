// otmb_op.h -- the resident sparse operator's record and the host helpers shared by its products (otmb_spmv.hip) and its solver
// (otmb_solve.hip): register blocks of columns, compact staging of host matrices, of d and of a stepped call.  The device walks over the layouts: otmb_op_fold.h.
// The layouts are described at the head of otmb_spmv.hip, which builds them and owns every buffer (sp_free_all).
#pragma once
#include <algorithm>
#include <atomic>
#include <type_traits>
#include <vector>

#include "otmb_common.h"
#include "otmb_sched.h"

#define SP_ELL_MAX 256   // longest row a slice takes
#define SP_TCH 512       // entries per LDS chunk of the Aᵀ and long-row kernels

struct OpSlot {  // one value set of the pattern (otmb_op_set_slots): nzval of the CSC copy, val of the row layout
    DevBuf nz, val;
};

// every operator of the process has another serial number: a child of otmb_op_submatrix knows its parent by it, not by an address
inline uint64_t op_new_serial() {
    static std::atomic<uint64_t> next{1};
    return next.fetch_add(1);
}

struct otmb_op {
    otmb_ctx *ctx = nullptr;
    uint64_t serial = op_new_serial();
    int device = 0;
    i64 m = 0, n = 0, nnz = 0;
    i64 nslices = 0, ell = 0, nlong = 0;  // slices, entries of the slice layout (padding included), long rows
    DevBuf cp, rv, nz;                    // CSC copy: colptr (n + 1, Int64), rowval - 1 (Int32), nzval (of the SELECTED slot: see slots)
    DevBuf dst;                           // per stored entry: its position in val / col
    DevBuf elen, sbase, loff, lrows;      // per row: length or -1 (long); per slice: first position; per row: long-row offset; long rows
    DevBuf val, col;                      // slices then long rows: values (of the SELECTED slot) and column indices (Int32, 0-based)
    std::vector<OpSlot> slots;            // the value slots, which own every nz / val array once the plan stands: nz and val above are
    i64 sel = 0, nval = 0;                // copies of slots[sel]'s records (otmb_op_select_slot switches them); nval: doubles of a val array
    DevBuf xs, ys;                        // host entry points' staging (op_reserve_xy): otmb_op_mul X, Y; otmb_op_solve_pc B, X; otmb_op_precond Y, Z
    DevBuf ds, sw;                        // staging of d (op_stage_d); the solver's arrays (SvWork, otmb_solve.hip): vectors, partial sums, column records
    DevBuf st;                            // otmb_op_step: the right-hand side and the preconditioners of the slots it visits (otmb_step.hip)
    DevBuf pd;                            // otmb_op_periodic: the Krylov bases, the cycle's in/out columns, partial sums and scalars (otmb_periodic.hip)
    OpSlot mean;                          // otmb_op_periodic_pc, OTMB_OUTER_MEAN: the cycle-mean values, private like pd (made once per call)
    OpSlot interp;                        // otmb_op_step_interp: the values of a blended step, (1 - w)·(slot a) + w·(slot b) (otmb_interp.hip); never mean
    DevBuf season, setab;                 // otmb_op_step_season: d and the source of a blended step (n·kc + n·k doubles); the fold's table of terms beyond 16 (otmb_season.hip)
    DevBuf ob, oh;                        // the observations (otmb_observe.hip): the partial sums; the host entry points' staging of obs, W, X / Xbar
    DevBuf cb;                            // otmb_op_combine_slots: the table of slot pointers and weights, beyond the 16 that travel as arguments
    DevBuf am;                            // otmb_op_add_matrix: the state words, B's positions in nzval, the table of slot pointers beyond 8 slots (otmb_addmat.hip)
    DevBuf ln;                            // otmb_op_set_lines (Int32, 0-based, -1 = none): successor (n), predecessor (n), line heads ascending (nheads)
    i64 nheads = 0;
    bool lines = false;                   // lines are set (they belong to the pattern: otmb_op_set_values keeps them)
    DevBuf src;                           // otmb_op_submatrix's child: per stored entry, its position in the parent's nzval (the gather table)
    uint64_t parent_serial = 0;           // ... and the parent's serial (0: not such a child), its nnz: what otmb_op_take_values accepts
    i64 parent_nnz = 0;
};

// otmb_spmv.hip, for otmb_submatrix.hip: the rest of a creation from arrays the library already owns -- op->cp (n + 1), op->nz and rowval
// (Int64, 1-based; read by the plan only) on the device, m, n and nnz set: the plan's checks and layouts, then slot 0
int32_t sp_plan_resident(otmb_op *op, const i64 *rowval);

// Register blocks of columns: f(std::integral_constant<int, B>, first column) for blocks of KB columns while that many are left from c0,
// then of KB / 2, ..., 1 (the matrix is read once per block).
template <int KB, class F>
static void op_blocks(i64 c0, i64 k, F f) {
    for (; k - c0 >= KB; c0 += KB) f(std::integral_constant<int, KB>(), c0);
    if constexpr (KB > 1) op_blocks<KB / 2>(c0, k, f);
}

// Host matrices (rows x k, leading dimension ld) are staged compactly (leading dimension = rows): the caller's padding rows are neither
// read nor written.
static int32_t op_upload(otmb_ctx *ctx, double *dev, const double *host, i64 ld, i64 rows, i64 k) {
    HIP_TRY(ctx, hipMemcpy2DAsync(dev, (size_t)rows * 8, host, (size_t)ld * 8, (size_t)rows * 8, (size_t)k, hipMemcpyHostToDevice, ctx->stream));
    ctx->uploaded_bytes += 8 * rows * k;
    return OTMB_OK;
}
static int32_t op_download(otmb_ctx *ctx, double *host, i64 ld, const double *dev, i64 rows, i64 k) {
    HIP_TRY(ctx, hipMemcpy2DAsync(host, (size_t)ld * 8, dev, (size_t)rows * 8, (size_t)rows * 8, (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    return OTMB_OK;
}
// The tail of a host entry point that returns rc: the staged result (rows x k at dev; no rows: nothing) comes back and the stream is waited
// for.  The context's message is rc's (a solver's report of columns that did not converge) and still is afterwards.
static int32_t op_finish(otmb_ctx *ctx, int32_t rc, double *host, i64 ld, const double *dev, i64 rows, i64 k) {
    const std::string msg = ctx->err;
    int32_t rcd;
    if (rows > 0 && (rcd = op_download(ctx, host, ld, dev, rows, k))) return rcd;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->err = msg;
    return rc;
}
// xs and ys for staged matrices of rx x k and ry x k (never empty buffers)
static int32_t op_reserve_xy(otmb_op *op, i64 rx, i64 ry, i64 k) {
    int32_t rc;
    if ((rc = otmb_reserve(op->ctx, op->xs, std::max<size_t>((size_t)(rx * k) * 8, 8)))) return rc;
    return otmb_reserve(op->ctx, op->ys, std::max<size_t>((size_t)(ry * k) * 8, 8));
}
// An optional d (n host values) staged in ds: dev is its device copy, or null when there is none
static int32_t op_stage_d(otmb_op *op, const double *d, double *&dev) {
    otmb_ctx *ctx = op->ctx;
    int32_t rc;
    if ((rc = otmb_reserve(ctx, op->ds, (size_t)op->n * 8 + 8))) return rc;
    dev = d ? (double *)op->ds.p : nullptr;
    if (d && op->n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(dev, d, (size_t)op->n * 8, hipMemcpyHostToDevice, ctx->stream));
        ctx->uploaded_bytes += 8 * op->n;
    }
    return OTMB_OK;
}
// The same for the per-column calls (otmb_op_*_dk): ldd == 0 is the above (devld = 0); otherwise D's n x k block is staged compactly, once per
// host call (devld = n).
static int32_t op_stage_dk(otmb_op *op, const double *D, i64 ldd, i64 k, const double *&dev, i64 &devld) {
    devld = 0;
    if (!D || ldd == 0) {
        double *one;
        const int32_t rc = op_stage_d(op, D, one);
        dev = one;
        return rc;
    }
    otmb_ctx *ctx = op->ctx;
    int32_t rc;
    if ((rc = otmb_reserve(ctx, op->ds, (size_t)(op->n * k) * 8 + 8))) return rc;
    dev = (const double *)op->ds.p;
    devld = op->n;
    return op->n > 0 ? op_upload(ctx, (double *)op->ds.p, D, ldd, op->n, k) : OTMB_OK;
}
// The same for a list of nd blocks with the one ldd (otmb_op_*_season): nd <= 1 is the above with the one block or none; otherwise block j is
// staged compactly behind block j - 1 (n values each when ldd == 0, n x k otherwise).  dev: the nd device pointers (one, maybe null, for nd <= 1)
static int32_t op_stage_dl(otmb_op *op, i64 nd, const double *const *D, i64 ldd, i64 k, std::vector<const double *> &dev, i64 &devld) {
    dev.assign((size_t)std::max<i64>(nd, 1), nullptr);
    if (nd <= 1) return op_stage_dk(op, nd == 1 ? D[0] : nullptr, ldd, k, dev[0], devld);
    otmb_ctx *ctx = op->ctx;
    const i64 n = op->n, kc = ldd == 0 ? 1 : k;
    int32_t rc;
    if ((rc = otmb_reserve(ctx, op->ds, (size_t)(nd * n * kc) * 8 + 8))) return rc;
    devld = ldd == 0 ? 0 : n;
    for (i64 j = 0; j < nd; ++j) {
        double *to = (double *)op->ds.p + j * n * kc;
        dev[(size_t)j] = to;
        if (n > 0 && (rc = op_upload(ctx, to, D[j], ldd == 0 ? n : ldd, n, kc))) return rc;
    }
    return OTMB_OK;
}

// What the host variant of a step or periodic call runs on: X compact in op->xs (n x k; uploaded when X is not null), source block j compact
// behind block j - 1 in op->ys, the d blocks in op->ds (op_stage_dl), and the lists of their device pointers as the device variant takes
// them.  d and src point into the record's own vectors: it stays where it was filled.
struct OpStaged {
    double *X;
    std::vector<const double *> dptr, sptr;
    StD d;
    StSrc src;
};
static int32_t op_stage_call(otmb_op *op, i64 k, const StD &d, const StSrc &src, const double *X, i64 ldx, OpStaged &g) {
    otmb_ctx *ctx = op->ctx;
    const i64 n = op->n;
    int32_t rc;
    i64 lddev = 0;
    if ((rc = op_reserve_xy(op, n, src.nsrc * n, k)) || (rc = op_stage_dl(op, d.nd, d.D, d.ldd, k, g.dptr, lddev))) return rc;
    g.X = (double *)op->xs.p;
    g.sptr.resize((size_t)src.nsrc);
    for (i64 j = 0; j < src.nsrc; ++j) g.sptr[(size_t)j] = (const double *)op->ys.p + j * n * k;
    if (n > 0) {  // staged once, however many steps or cycles
        if (X && (rc = op_upload(ctx, g.X, X, ldx, n, k))) return rc;
        for (i64 j = 0; j < src.nsrc; ++j)
            if ((rc = op_upload(ctx, (double *)op->ys.p + j * n * k, src.S[j], src.lds, n, k))) return rc;
    }
    g.d = StD{g.dptr[0] ? d.nd : 0, g.dptr.data(), lddev};
    g.src = StSrc{src.nsrc, g.sptr.data(), n, src.scale};
    return OTMB_OK;
}
