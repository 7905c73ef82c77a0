// otmb_solve_lines.hip -- the line preconditioner of otmb_op_solve_pc / otmb_op_precond: P is the part of M = σ·I + diag(d) + A (adjoint:
// Aᵀ) on caller-given lines (otmb_op_set_lines[_dev]: next[i] = the successor of unknown i on its line, or 0), a block Jacobi whose blocks
// are tridiagonal and are solved by the Thomas recurrence.  For the transport matrices a line is one water column, top to bottom: the
// vertical coupling (TκVML: ~1e-3 s⁻¹ against horizontal rates of ~1e-7 s⁻¹) is then inside the preconditioner.
//
// Per solve and, where every column has its own d (otmb_op_*_dk), per column -- a is the column's, u and l are not --, with j = next[i] (include/otmb.h states this as the contract; tests/solve_lines_ref.py restates it bit for bit):
//     a_i = Jacobi's diag[i];  u_i = Σ stored (i, j) of A, l_i = Σ stored (j, i) of A, each from +0.0 in storage order (adjoint: swapped)
//     piv_head = a_head;  m_j = l_i / piv_i;  piv_j = a_j - m_j·u_i            (no pivoting, no FMA; a zero or non-finite pivot is refused)
//     z = P⁻¹·y:  y'_head = y_head, y'_j = y_j - m_j·y'_i;  z_tail = y'_tail / piv_tail, z_i = (y'_i - u_i·z_j) / piv_i
//
// Factorisation and sweep: ONE LANE OWNS ONE LINE and walks it, head to tail and back; the right-hand-side columns are register-blocked
// like the solver's other kernels.  The heads are kept in ascending order, so lanes c, c + 1, ... hold neighbouring lines: on an ocean grid
// (wet cells numbered level by level) the cells they touch at the same depth are nearly adjacent unknowns, and the loads of a wave coalesce
// without a permuted copy of anything.  The limit: a line is a sequential recurrence, so a long line is one lane's dependent chain (as a
// long row is for the adjoint product), and a wave takes as long as its longest line.  The result is deterministic (no sums across lanes)
// and a column never sees another column.
#include <hip/hip_runtime.h>

#include "otmb_prims.h"
#include "otmb_solve.h"

typedef unsigned long long ull;

// ---- the lines: validation, Int32 tables, heads ------------------------------------------------------------------------------------
// next (1-based, 0 = none) -> nxt / prv (0-based, -1 = none); cnt[j] = how many unknowns name j; bad = the first i whose entry is neither
// 0 nor in (i, n] (1-based).  prv is preset to -1.
__global__ __launch_bounds__(256) void ln_check_kernel(const i64 *__restrict__ next, i64 n, int *__restrict__ nxt, int *__restrict__ prv,
                                                       int *__restrict__ cnt, ull *__restrict__ bad) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const i64 v = next[i];
    int j = -1;
    if (v != 0) {
        if (v <= i + 1 || v > n) atomicMin(bad, (ull)i);
        else j = (int)(v - 1);
    }
    nxt[i] = j;
    if (j >= 0) {
        prv[j] = (int)i;  // (two writers only when cnt[j] > 1, which is refused)
        atomicAdd(&cnt[j], 1);
    }
}
// flag[i] = i is a head (nobody's successor), flag[n] = 0; bad = the first index that is the successor of two unknowns
__global__ __launch_bounds__(256) void ln_flag_kernel(const int *__restrict__ cnt, i64 n, i64 *__restrict__ flag, ull *__restrict__ bad) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        flag[i] = 0;
        return;
    }
    flag[i] = cnt[i] == 0;
    if (cnt[i] > 1) atomicMin(bad, (ull)i);
}
__global__ __launch_bounds__(256) void ln_heads_kernel(const i64 *__restrict__ flag, const i64 *__restrict__ pos, i64 n, int *__restrict__ heads) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < n && flag[i]) heads[pos[i]] = (int)i;
}

// ---- u and l: one thread per unknown scans two columns of the CSC copy ----------------------------------------------------------
__global__ __launch_bounds__(256) void ln_ul_kernel(const i64 *__restrict__ cp, const int *__restrict__ rv, const double *__restrict__ nz, i64 n,
                                                    const int *__restrict__ nxt, int adjoint, double *__restrict__ u, double *__restrict__ l) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = nxt[i];
    double up = 0.0, lo = 0.0;
    if (j >= 0) {
        for (i64 e = cp[j] - 1; e < cp[j + 1] - 1; ++e)  // (i, j): in column j
            if (rv[e] == (int)i) up = up + nz[e];
        for (i64 e = cp[i] - 1; e < cp[i + 1] - 1; ++e)  // (j, i): in column i
            if (rv[e] == j) lo = lo + nz[e];
    }
    u[i] = adjoint ? lo : up;
    l[i] = adjoint ? up : lo;
}

// ---- the factorisation: u and l (by i) are the lines' own; diag, m (the multipliers, by j; 0 at a head) and piv are a column's ------------
// One lane owns one line of ONE column: a line is a short dependent chain of divisions, so the kc columns go to more lanes (the workgroups
// of column c follow those of column c - 1), not to a loop inside the lane that owns the line.  Column c's arrays lie at + c·cs.  l == null
// (one column): m holds l on entry, as ln_ul_kernel left it; otherwise l is an array of its own, which every column reads.
// bad: the smallest (column << 32 | index): with one column, the smallest index.
__global__ __launch_bounds__(64) void ln_factor_kernel(const int *__restrict__ heads, i64 nheads, const int *__restrict__ nxt,
                                                       const double *__restrict__ diag, const double *__restrict__ u, double *m,
                                                       double *__restrict__ piv, ull *__restrict__ bad, const double *l = nullptr, i64 cs = 0) {
    const i64 nhb = (nheads + 63) / 64;
    const ull c = (ull)(blockIdx.x / nhb);
    const i64 h = ((i64)blockIdx.x - (i64)c * nhb) * 64 + threadIdx.x;
    if (h >= nheads) return;
    const i64 o = (i64)c * cs;
    if (!l) l = m;
    int i = heads[h];
    double pv = diag[i + o], lv = l[i];
    m[i + o] = 0.0;
    for (;;) {
        piv[i + o] = pv;
        if (pv == 0.0 || !isfinite(pv)) atomicMin(bad, c << 32 | (ull)i);
        const int j = nxt[i];
        if (j < 0) break;
        const double mj = lv / pv;
        lv = l[j];
        m[j + o] = mj;
        const double t = mj * u[i];
        pv = diag[j + o] - t;
        i = j;
    }
}

// ---- the sweep: Z = P⁻¹·Y, forward to the tail (y' is parked in Z), then back ------------------------------------------------------
// Only columns in state SV_ACTIVE are read or written (cs == nullptr: all of them).  Y and Z may be the same array.  PC: column c's multipliers
// and pivots lie at + c·ps; otherwise there is one set for all columns, read once per row of the register block as before columns could
// have their own.
template <int KB, bool PC = false>
__global__ __launch_bounds__(64) void ln_sweep_kernel(const SvCol *__restrict__ cs, const int *__restrict__ heads, i64 nheads,
                                                      const int *__restrict__ nxt, const int *__restrict__ prv, const double *__restrict__ m,
                                                      const double *__restrict__ u, const double *__restrict__ piv, const double *Y, i64 ldy,
                                                      double *Z, i64 ldz, i64 ps = 0) {
    bool on[KB], any = false;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        on[c] = !cs || cs[c].state == SV_ACTIVE;
        any |= on[c];
    }
    if (!any) return;  // (uniform over the grid)
    const i64 h = (i64)blockIdx.x * 64 + threadIdx.x;
    if (h >= nheads) return;
    int i = heads[h];
    double y[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) y[c] = on[c] ? Y[i + c * ldy] : 0.0;
    for (int j = nxt[i]; j >= 0; j = nxt[i]) {
        const double mj = PC ? 0.0 : m[j];
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            if (!on[c]) continue;
            Z[i + c * ldz] = y[c];
            const double t = (PC ? m[j + c * ps] : mj) * y[c];
            y[c] = Y[j + c * ldy] - t;
        }
        i = j;
    }
    double pv = PC ? 0.0 : piv[i];
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        if (!on[c]) continue;
        y[c] = y[c] / (PC ? piv[i + c * ps] : pv);
        Z[i + c * ldz] = y[c];
    }
    for (int p = prv[i]; p >= 0; p = prv[i]) {
        const double up = u[p];
        if (!PC) pv = piv[p];
#pragma unroll
        for (int c = 0; c < KB; ++c) {
            if (!on[c]) continue;
            const double t = up * y[c];
            y[c] = (Z[p + c * ldz] - t) / (PC ? piv[p + c * ps] : pv);
            Z[p + c * ldz] = y[c];
        }
        i = p;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct LnTables { const int *nxt, *prv, *heads; };  // op->ln as otmb_op_set_lines_dev leaves it: n successors, n predecessors, the heads
static LnTables ln_tables(const otmb_op *op) {
    const int *nxt = (const int *)op->ln.p;
    return {nxt, nxt + op->n, nxt + 2 * op->n};
}

void ln_factor(otmb_op *op, int adjoint, const SvPrec &p, double *l, ull *bad) {
    if (p.kc == 1) l = nullptr;  // one column: l goes through m, no scratch
    hipStream_t st = op->ctx->stream;
    const i64 n = op->n;
    const LnTables ln = ln_tables(op);
    hipLaunchKernelGGL(ln_ul_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const i64 *)op->cp.p, (const int *)op->rv.p,
                       (const double *)op->nz.p, n, ln.nxt, adjoint, p.u, l ? l : p.m);
    hipLaunchKernelGGL(ln_factor_kernel, dim3((unsigned)((op->nheads + 63) / 64 * p.kc)), dim3(64), 0, st, ln.heads, op->nheads, ln.nxt,
                       (const double *)p.diag, (const double *)p.u, p.m, p.piv, bad, (const double *)l, p.cs);
}

void ln_sweep(otmb_op *op, const SvCol *cs, i64 k, const SvPrec &p, const double *Y, i64 ldy, double *Z, i64 ldz) {
    hipStream_t st = op->ctx->stream;
    const LnTables ln = ln_tables(op);
    op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
        constexpr int KB = decltype(kb)::value;
        hipLaunchKernelGGL((p.cs ? ln_sweep_kernel<KB, true> : ln_sweep_kernel<KB, false>), dim3((unsigned)((op->nheads + 63) / 64)), dim3(64), 0, st, cs ? cs + c0 : nullptr,
                           ln.heads, op->nheads, ln.nxt, ln.prv, (const double *)p.m + c0 * p.cs, (const double *)p.u, (const double *)p.piv + c0 * p.cs, Y + c0 * ldy,
                           ldy, Z + c0 * ldz, ldz, p.cs);
    });
}

extern "C" {

int32_t otmb_op_set_lines_dev(otmb_op *op, const int64_t *next) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    if (op->m != op->n) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "set_lines: the operator's matrix must be square");
    if (!next) {
        op->lines = false;
        op->nheads = 0;
        return OTMB_OK;
    }
    const i64 n = op->n;
    if (n == 0) {
        op->lines = true;
        op->nheads = 0;
        return OTMB_OK;
    }
    HIP_TRY(ctx, hipSetDevice(op->device));
    hipStream_t st = ctx->stream;
    // everything is checked in scratch memory; the operator's own tables are written only afterwards
    DevScratch S;
    DevBuf &tables = S.add(), &scan_tmp = S.add();
    int32_t rc;
    const size_t ints = 3 * (size_t)n + 2;  // nxt, prv, cnt (+ padding to 8 bytes)
    if ((rc = otmb_reserve(ctx, tables, ints * 4 + 2 * (size_t)(n + 1) * 8 + 16))) return rc;
    int *nxt = (int *)tables.p, *prv = nxt + n, *cnt = prv + n;
    i64 *flag = (i64 *)(nxt + (ints & ~(size_t)1)), *pos = flag + (n + 1);
    ull *bad = (ull *)(pos + (n + 1));
    HIP_TRY(ctx, hipMemsetAsync(prv, 0xff, (size_t)n * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(cnt, 0, (size_t)n * 4, st));
    HIP_TRY(ctx, hipMemsetAsync(bad, 0xff, 16, st));
    hipLaunchKernelGGL(ln_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const i64 *)next, n, nxt, prv, cnt, bad);
    hipLaunchKernelGGL(ln_flag_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, st, (const int *)cnt, n, flag, bad + 1);
    HIP_TRY(ctx, hipGetLastError());
    ull hb[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(hb, bad, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    char msg[160];
    if (hb[0] != ~0ull) {
        snprintf(msg, sizeof msg, "set_lines: next[%lld] must be 0 or an index above %lld and at most n = %lld (1-based; the first such entry)",
                 (long long)hb[0] + 1, (long long)hb[0] + 1, (long long)n);
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
    }
    if (hb[1] != ~0ull) {
        snprintf(msg, sizeof msg, "set_lines: index %lld is the successor of two unknowns (1-based; the first such index)", (long long)hb[1] + 1);
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
    }
    if ((rc = otmb_exclusive_scan(ctx, scan_tmp, flag, pos, n + 1))) return rc;
    i64 nheads = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&nheads, pos + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (nheads < 1 || nheads > n) return otmb_fail(ctx, OTMB_ERR_HIP, "set_lines: the count of line heads");  // (cannot happen: index 1 has no predecessor)
    // (growing op->ln frees the old tables first: from here on the operator has no lines until the new ones are in place, so an
    // allocation failure leaves it cleared, never pointing at freed tables)
    op->lines = false;
    op->nheads = 0;
    if ((rc = otmb_reserve(ctx, op->ln, (size_t)(2 * n + nheads) * 4))) return rc;
    int *keep = (int *)op->ln.p;
    HIP_TRY(ctx, hipMemcpyAsync(keep, nxt, (size_t)(2 * n) * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(ln_heads_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const i64 *)flag, (const i64 *)pos, n, keep + 2 * n);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));  // (the scratch goes when this returns)
    op->nheads = nheads;
    op->lines = true;
    return OTMB_OK;
}

int32_t otmb_op_set_lines(otmb_op *op, const int64_t *next) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    otmb_ctx *ctx = op->ctx;
    if (!next || op->m != op->n || op->n == 0) return otmb_op_set_lines_dev(op, next);
    HIP_TRY(ctx, hipSetDevice(op->device));
    int32_t rc;
    if ((rc = otmb_reserve(ctx, op->xs, (size_t)op->n * 8 + 8))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(op->xs.p, next, (size_t)op->n * 8, hipMemcpyHostToDevice, ctx->stream));
    ctx->uploaded_bytes += 8 * op->n;
    return otmb_op_set_lines_dev(op, (const int64_t *)op->xs.p);
}

}  // extern "C"
