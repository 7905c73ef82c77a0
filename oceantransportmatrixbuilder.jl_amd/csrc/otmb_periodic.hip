// otmb_periodic.hip -- the periodic state of the stepped cycle, x = F(x), on a resident operator with value slots: otmb_op_periodic[_dev].
// F(x) = the step call over the cycle's ncycle steps with the source S; F is affine, F(x) = Φ·x + g with Φ·v the same call without S
// and g = F(0).  include/otmb.h states the contract; tests/periodic_ref.py restates it in numpy.
//
// Per column (columns are independent; a stopped column is frozen): restarted GMRES(m) on (I - Φ)·δ = r, r = F(x) - x, no preconditioner.
//     r = F(x) - x, β = ‖r‖;  accepted when β <= ptol·‖g‖ (only ever on this explicit value);  V_0 = r / β, the rotated right-hand side = β·e_0
//     iteration i:  w = V_i - Φ·V_i                                   (one step call for every column that iterates; pd_defect_kernel)
//                   h' = V_0..iᵀ·w;  w -= V_0..i·h'                    (pd_dots_kernel + pd_fold_kernel, pd_update_kernel)
//                   h'' = V_0..iᵀ·w; w -= V_0..i·h'', ‖w‖²             (the same two kernels again: CGS2; the update leaves ‖w‖²'s partials)
//                   the host: H(0..i, i) = h' + h'', H(i+1, i) = ‖w‖, the old rotations, a new one, the recursive residual   (GmresLsq::push)
//                   V_{i+1} = w / ‖w‖                                  (pd_scale_kernel)
//     at a recursive residual <= ptol·‖g‖, at i + 1 = m, at ‖w‖ = 0 and when one cycle of maxcycles is left:
//                   y from the triangle (GmresLsq::solve);  x += V_0..i·y  (pd_combine_kernel), then r = F(x) - x again (one step call with S)
// h', h'' and ‖w‖² stay on the device between the kernels (the update reads them where the fold wrote them); the host reads them once per
// round, for every column together: 2·(i + 2) doubles a column.
//
// Every sum is deterministic and a column's own: a workgroup of 256 lanes takes PD_ROWS rows fixed by n, lane t the row pairs t, t + 256, ...
// of them in that order (16-byte loads: every array of the workspace has an even leading dimension on a 256-byte base), one accumulator per
// basis vector in a register block (op_blocks over the basis, as the products block columns), the workgroup's tree is the solver's, the one
// copy of otmb_op_sum.h (xor shuffles in a wave, the four waves in order), ONE partial per workgroup and quantity, and pd_fold_kernel adds a
// quantity's partials in index order.  No floating-point atomics, no FMA (-ffp-contract=off), one operation per statement where the order is
// the contract.  LDS: the workgroup reduction only.
//
// The host part: the column's least-squares problem is otmb_gmres.h's and the schedule's rules are otmb_sched.h's (host C++ alone, each
// tested without a device); every export states its call as one record (PdCall, otmb_solve.h: the step call's head and the outer
// iteration's arguments); PdRun holds one call -- that record, the workspace, the columns, the host's copies -- and its member functions are
// the steps of pd_run's outline: the sources' norms, the first call, the rounds (cycle, orthogonalise, read_hs, judged, advance) and the
// report (sv_report_open, which the solver shares, as it shares the step's argument checks: otmb_solve.h).
//
// otmb_op_periodic_pc[_dev] with OTMB_OUTER_MEAN: flexible GMRES, right-preconditioned by the cycle-mean operator.  M̄ = diag(d) + Ā, Ā the
// visit-weighted mean of the cycle's slots (cb_combine of otmb_combine.hip into op->mean, once per call), P = ncycle·δt; one implicit-Euler
// step over the whole period gives Φ ≈ (I + P·M̄)⁻¹, so (I - Φ)⁻¹ ≈ I + (P·M̄)⁻¹.  Iteration i becomes
//     q = M̄⁻¹·V_i      (the solver's own path on the mean values, σ = 0, from zero, the call's rtol / maxiter / precond: PdRun::msolve)
//     Z_i = V_i + q / P  (pd_precond_kernel), kept behind the V block;   w = Z_i - Φ·Z_i;   CGS2 against V as before;   x += Z_0..i·y
// and everything else -- the restart, verify and stop rules, cycles, defect -- is as above.  OTMB_OUTER_NONE is the method above, bit for bit.
//
// otmb_op_periodic_dk[_dev], every column with its own d (D, n x k): the step calls and the mean solves take the columns that iterate
// gathered compactly, so their columns of D are gathered beside their states and sources (w.Dg), and the mean's preconditioner, made once
// for all k columns, lends the gathered columns' sh, diag, multipliers and pivots to a compact copy (w.mpg).  The step and the solver give a
// column the same bits at every position of a block, so a column's path does not depend on which other columns still run.
//
// What the record's fields switch on.  F is ONE step call (PdRun::cycle -> st_call of otmb_step.hip) of the columns that iterate, gathered
// compactly, with the record's schedule, and everything the step does with a field it does here:
//   sched  cyclic (otmb_op_periodic, _pc, _dk: substeps = 1; otmb_op_periodic_sched) or listed (otmb_op_periodic_interp, _season).  The
//          mean's weights are the schedule's (StSched::mean_weights): the slots' shares of the cycle's steps, a blended step counting for
//          its two slots by its weights.  op->mean and a blended step's op->interp are different value sets: the call needs both at once.
//   d      one block for every column, or per column (D, n x k): the gathered step calls and mean solves then carry the live columns of D
//          beside their states and sources (w.Dg), and the mean's preconditioner, made once for all k columns, lends the gathered columns'
//          sh, diag, multipliers and pivots to a compact copy (w.mpg).  The step and the solver give a column the same bits at every
//          position of a block, so a column's path does not depend on which other columns still run.  Per slot (otmb_op_periodic_season):
//          w.Dg holds block j's live columns behind block j - 1's, and the mean operator is diag(d̄) + Ā with d̄ the fold of the d blocks
//          under the mean's own weights (se_fold of otmb_season.hip into w.dbar, once per call, before the mean's preconditioner is made).
//          With one block d̄ is that block, untouched.
//   src    one block (its live columns in w.Sb or, the first call's 2k, in the bases) or a block per slot (w.Sg: block j's columns behind
//          block j - 1's); a column is zero only when it is zero in every block.  Never a scale: a history is not periodic.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "otmb_gmres.h"
#include "otmb_op_sum.h"
#include "otmb_solve.h"

#define PD_ROWS 2048  // rows per workgroup: 256 lanes x 4 pairs
#define PD_NB 4       // the largest register block of basis vectors (op_blocks: 4, 2, 1)

enum { PD_ARNOLDI = 0, PD_VERIFY = 1, PD_STOPPED = 2 };

struct Pd2 {
    double a, b;
};
// rows i (even) and i + 1 of p; row i + 1 counts only below n.  al: p + i is 16-byte aligned (p is, and its leading dimension is even).
__device__ __forceinline__ Pd2 pd_load(const double *__restrict__ p, i64 i, i64 n, bool al) {
    if (al && i + 1 < n) {
        const double2 v = *reinterpret_cast<const double2 *>(p + i);
        return {v.x, v.y};
    }
    return {p[i], i + 1 < n ? p[i + 1] : 0.0};
}
__device__ __forceinline__ void pd_store(double *__restrict__ p, i64 i, i64 n, bool al, Pd2 v) {
    if (al && i + 1 < n) {
        *reinterpret_cast<double2 *>(p + i) = make_double2(v.a, v.b);
        return;
    }
    p[i] = v.a;
    if (i + 1 < n) p[i + 1] = v.b;
}
// the q-th row pair of this lane: its first row (>= n: the lane is done)
__device__ __forceinline__ i64 pd_row(int q) { return 2 * ((i64)blockIdx.x * (PD_ROWS / 2) + threadIdx.x + 256 * q); }

// ---- h = Vᵀ·w for NB basis vectors (leading dimension ldv) and, NORM, ‖w‖²: a lane's share ------------------------------------------------
template <int NB, bool NORM>
__device__ __forceinline__ void pd_dots_lane(i64 n, const double *__restrict__ V, i64 ldv, const double *__restrict__ w, double (&acc)[NB + 1]) {
#pragma unroll
    for (int b = 0; b <= NB; ++b) acc[b] = 0.0;
    for (int q = 0; q < PD_ROWS / 512; ++q) {
        const i64 i = pd_row(q);
        if (i >= n) break;
        const Pd2 x = pd_load(w, i, n, true);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const Pd2 v = pd_load(V + b * ldv, i, n, true);
            const double pa = v.a * x.a;
            acc[b] = acc[b] + pa;
            if (i + 1 < n) {
                const double pb = v.b * x.b;
                acc[b] = acc[b] + pb;
            }
        }
        if (NORM) {
            const double pa = x.a * x.a;
            acc[NB] = acc[NB] + pa;
            if (i + 1 < n) {
                const double pb = x.b * x.b;
                acc[NB] = acc[NB] + pb;
            }
        }
    }
}
// part: the partials of the block's first basis vector (quantity j at part[j * np + workgroup]); pnorm: those of ‖w‖²
template <int NB, bool NORM>
__global__ __launch_bounds__(256) void pd_dots_kernel(i64 n, const double *__restrict__ V, i64 ldv, const double *__restrict__ w, double *__restrict__ part,
                                                      i64 np, double *__restrict__ pnorm) {
    __shared__ double red[4 * (NB + 1)];
    double acc[NB + 1];
    pd_dots_lane<NB, NORM>(n, V, ldv, w, acc);
    op_block_sum<NB + 1>(acc, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int b = 0; b < NB; ++b) part[(i64)b * np + blockIdx.x] = acc[b];
        if (NORM) pnorm[blockIdx.x] = acc[NB];
    }
}
// one workgroup: out[q] = the np partials of quantity q, added in index order
__global__ __launch_bounds__(256) void pd_fold_kernel(const double *__restrict__ part, i64 np, i64 nq, double *__restrict__ out) {
    for (i64 q = threadIdx.x; q < nq; q += 256) {
        double s = part[q * np];
        for (i64 b = 1; b < np; ++b) s = s + part[q * np + b];
        out[q] = s;
    }
}

// ---- w -= Σ_j h_j·V_j, j ascending (h: device, where the fold wrote it); NORM: ‖w‖²'s partials of the result ------------------------------
template <bool NORM>
__device__ __forceinline__ double pd_update_lane(i64 n, const double *__restrict__ V, i64 ldv, i64 nj, const double *__restrict__ h, double *__restrict__ w) {
    double acc = 0.0;
    for (int q = 0; q < PD_ROWS / 512; ++q) {
        const i64 i = pd_row(q);
        if (i >= n) break;
        Pd2 x = pd_load(w, i, n, true);
        for (i64 j = 0; j < nj; ++j) {
            const Pd2 v = pd_load(V + j * ldv, i, n, true);
            const double hj = h[j];
            const double pa = hj * v.a;
            x.a = x.a - pa;
            const double pb = hj * v.b;
            x.b = x.b - pb;
        }
        pd_store(w, i, n, true, x);
        if (NORM) {
            const double pa = x.a * x.a;
            acc = acc + pa;
            if (i + 1 < n) {
                const double pb = x.b * x.b;
                acc = acc + pb;
            }
        }
    }
    return acc;
}
template <bool NORM>
__global__ __launch_bounds__(256) void pd_update_kernel(i64 n, const double *__restrict__ V, i64 ldv, i64 nj, const double *__restrict__ h, double *__restrict__ w,
                                                        double *__restrict__ pnorm) {
    __shared__ double red[4];
    double acc[1] = {pd_update_lane<NORM>(n, V, ldv, nj, h, w)};
    if (NORM) {
        op_block_sum<1>(acc, red);
        if (threadIdx.x == 0) pnorm[blockIdx.x] = acc[0];
    }
}

// ---- x += Σ_j y_j·V_j, j ascending, at a restart (y: device) ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_combine_kernel(i64 n, const double *__restrict__ V, i64 ldv, i64 nj, const double *__restrict__ y, double *__restrict__ x,
                                                         bool alx) {
    for (int q = 0; q < PD_ROWS / 512; ++q) {
        const i64 i = pd_row(q);
        if (i >= n) break;
        Pd2 s = pd_load(x, i, n, alx);
        for (i64 j = 0; j < nj; ++j) {
            const Pd2 v = pd_load(V + j * ldv, i, n, true);
            const double yj = y[j];
            const double pa = yj * v.a;
            s.a = s.a + pa;
            const double pb = yj * v.b;
            s.b = s.b + pb;
        }
        pd_store(x, i, n, alx, s);
    }
}

// ---- r = f - x (x null: r = f) into out (null: not stored) and ‖r‖²'s partials (pnorm null: none): the defect, and w = v - Φ·v ------------
__global__ __launch_bounds__(256) void pd_defect_kernel(i64 n, const double *__restrict__ f, const double *__restrict__ x, bool alx, double *__restrict__ out,
                                                        double *__restrict__ pnorm) {
    __shared__ double red[4];
    double acc[1] = {0.0};
    for (int q = 0; q < PD_ROWS / 512; ++q) {
        const i64 i = pd_row(q);
        if (i >= n) break;
        Pd2 r = pd_load(f, i, n, true);
        if (x) {
            const Pd2 s = pd_load(x, i, n, alx);
            r.a = r.a - s.a;
            r.b = r.b - s.b;
        }
        if (out) pd_store(out, i, n, true, r);
        const double pa = r.a * r.a;
        acc[0] = acc[0] + pa;
        if (i + 1 < n) {
            const double pb = r.b * r.b;
            acc[0] = acc[0] + pb;
        }
    }
    if (pnorm) {  // (uniform over the workgroup: every lane reaches the barrier)
        op_block_sum<1>(acc, red);
        if (threadIdx.x == 0) pnorm[blockIdx.x] = acc[0];
    }
}

// ---- z = v + q / P: the preconditioned direction of OTMB_OUTER_MEAN (one division, one addition) ----------------------------------------
__global__ __launch_bounds__(256) void pd_precond_kernel(i64 n, const double *__restrict__ v, const double *__restrict__ qv, double P, double *__restrict__ z) {
    for (int q = 0; q < PD_ROWS / 512; ++q) {
        const i64 i = pd_row(q);
        if (i >= n) break;
        Pd2 x = pd_load(v, i, n, true);
        const Pd2 y = pd_load(qv, i, n, true);
        const double ta = y.a / P;
        x.a = x.a + ta;
        const double tb = y.b / P;
        x.b = x.b + tb;
        pd_store(z, i, n, true, x);
    }
}

// ---- v = w / s, in place: the new basis vector ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pd_scale_kernel(i64 n, double *__restrict__ w, double s) {
    for (int q = 0; q < PD_ROWS / 512; ++q) {
        const i64 i = pd_row(q);
        if (i >= n) break;
        Pd2 x = pd_load(w, i, n, true);
        x.a = x.a / s;
        x.b = x.b / s;
        pd_store(w, i, n, true, x);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
struct PdCol {  // one column's iteration; ls (otmb_gmres.h): the triangle, the rotations, the rotated right-hand side and the iteration ls.i
    int phase = PD_ARNOLDI, reason = OTMB_PERIODIC_CONVERGED;
    i64 cycles = 0, msolve_iters = 0;  // msolve_iters: the BiCGStab iterations of its mean solves (OTMB_OUTER_MEAN)
    double defect = NAN, gnorm = 0.0;
    GmresLsq ls;
    void stop(int why) { phase = PD_STOPPED, reason = why; }
};

struct PdWork {  // the arrays inside op->pd; every vector has the leading dimension ld (even)
    i64 n, k, m, ld, np;
    double *V, *W, *Sb, *part, *hs, *yv;  // V: k bases of m + 1 vectors; W, Sb: k columns each (contiguous: 2k for the first call)
    double *Z = nullptr, *mp = nullptr;   // OTMB_OUTER_MEAN: k blocks of m preconditioned directions behind Sb; the mean's preconditioner
    double *mpg = nullptr, *Dg = nullptr; // per-column d: the gathered columns of that preconditioner, and of D (2k columns: the first call's)
    double *Sg = nullptr;                 // more than one source block: the gathered columns of all of them (nsrc blocks of 2k columns)
    double *dbar = nullptr;               // OTMB_OUTER_MEAN with a d per slot: the cycle-mean d̄ (n values, or n x k with the leading dimension ld)
    double *v(i64 c, i64 j) const { return V + (c * (m + 1) + j) * ld; }
    double *z(i64 c, i64 j) const { return Z + (c * m + j) * ld; }
    double *partc(i64 c) const { return part + c * (m + 2) * np; }
    i64 hso(i64 c) const { return c * 2 * (m + 2); }  // column c's scalars: h' (m + 2 doubles), then h''; the host's copy has the same layout
    double *hsc(i64 c) const { return hs + hso(c); }
};

// zvecs: the vectors of the Z block a column (0, or m with OTMB_OUTER_MEAN); pdbl: the doubles of the mean's preconditioner (0 without);
// percol: every column has its own d (a second block of pdbl doubles, and 2k gathered columns of D); nsrc: the source blocks (more than
// one: nsrc·2k gathered columns behind everything else; one block's columns lie in Sb or, the first call's 2k, in the bases as ever)
// nd: the d blocks (with percol the 2k gathered columns of each; more than one and a mean: d̄ behind everything else)
static int32_t pd_work(otmb_op *op, i64 k, i64 m, i64 zvecs, size_t pdbl, bool percol, i64 nsrc, i64 nd, PdWork &w) {
    const i64 n = op->n;
    w.n = n, w.k = k, w.m = m, w.ld = (n + 1) & ~(i64)1, w.np = (n + PD_ROWS - 1) / PD_ROWS;
    const i64 ndg = percol ? std::max<i64>(nd, 1) : 0;
    if ((double)(nsrc + ndg + 1) * 2.0 * (double)k * (double)w.ld >= 1.0e18) return otmb_fail(op->ctx, OTMB_ERR_ALLOC, "periodic: the workspace's size overflows");
    const size_t head = (percol ? 2 : 1) * pdbl + (size_t)(ndg * 2 * k * w.ld);
    const size_t body = head + (nsrc > 1 ? (size_t)(nsrc * 2 * k * w.ld) : 0);
    const size_t tail = body + (nd > 1 && pdbl ? (size_t)((percol ? k : 1) * w.ld) : 0);
    const double need = ((double)(m + 3 + zvecs) * (double)w.ld + (double)(m + 2) * (double)w.np + 3.0 * (double)(m + 2)) * (double)k * 8.0 +
                        (double)tail * 8.0;
    if (need >= 9.0e18) return otmb_fail(op->ctx, OTMB_ERR_ALLOC, "periodic: the workspace's size overflows");
    const size_t vec = (size_t)(m + 3 + zvecs) * (size_t)w.ld * (size_t)k;
    const size_t scal = (size_t)((m + 2) * w.np * k) + (size_t)(3 * (m + 2) * k);
    int32_t rc;
    if ((rc = otmb_reserve(op->ctx, op->pd, (vec + scal + tail) * 8))) return rc;
    w.V = (double *)op->pd.p;
    w.W = w.V + (size_t)(m + 1) * (size_t)w.ld * (size_t)k;
    w.Sb = w.W + w.ld * k;
    w.Z = zvecs ? w.Sb + w.ld * k : nullptr;
    w.part = w.V + vec;
    w.hs = w.part + (m + 2) * w.np * k;
    w.yv = w.hs + 2 * (m + 2) * k;
    w.mp = pdbl ? w.V + vec + scal : nullptr;
    w.mpg = pdbl && percol ? w.mp + pdbl : nullptr;
    w.Dg = percol ? w.V + vec + scal + 2 * pdbl : nullptr;
    w.Sg = nsrc > 1 ? w.V + vec + scal + head : nullptr;
    w.dbar = nd > 1 && pdbl ? w.V + vec + scal + body : nullptr;
    return OTMB_OK;
}

// The checks of a periodic call, in the step's order (st_call): the arguments it shares with the step and its own, then D and ldd under the
// export's name (a season call's d is a list, which has its own checks), then the schedule's (st_check_sched).
static int32_t pd_check(otmb_op *op, const PdCall &c) {
    const char *more = !c.cycles || !c.defect || !c.reason
                           ? "null argument"
                           : sv_step_complaint(op, c.rtol, c.maxiter, c.dt, c.theta, c.nsteps >= 1, "ncycle must be >= 1", c.sched.first_slot);
    if (!more)
        more = !(c.ptol > 0.0)                               ? "ptol must be > 0"
               : c.restart < 1 || c.restart >= (1ll << 20)   ? "restart must be >= 1 (and below 2^20)"
               : c.maxcycles < 0                             ? "maxcycles must be >= 0"
                                                             : nullptr;
    int32_t rc = sv_check_step(op, c.precond, c.k, c.src.nsrc > 0 && c.src.S ? c.src.S[0] : nullptr, c.src.lds, c.X, c.ldx, more);
    if (rc == OTMB_OK && c.outer != OTMB_OUTER_NONE && c.outer != OTMB_OUTER_MEAN)
        rc = otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, "outer must be OTMB_OUTER_NONE or OTMB_OUTER_MEAN");
    if (rc || (!c.season && (rc = sv_check_d(op, c.call, c.d.nd ? c.d.D[0] : nullptr, c.d.ldd)))) return rc;
    return c.sched_checks ? st_check_sched(op, c) : OTMB_OK;
}

// g = 0: x = 0 at no cost
static int32_t pd_all_zero(i64 k, int64_t *cycles, double *defect, int32_t *reason, int64_t *msolve_iters) {
    for (i64 c = 0; c < k; ++c) cycles[c] = 0, defect[c] = 0.0, reason[c] = OTMB_PERIODIC_CONVERGED;
    if (msolve_iters)
        for (i64 c = 0; c < k; ++c) msolve_iters[c] = 0;
    return OTMB_OK;
}

struct PdItem {  // a column of one step call: column col's state from its basis vector (from >= 0), from X (-1) or zero (-2)
    i64 col, from;
};

struct PdRun {  // one call: the operator, the call's record, the workspace, the columns and the host's copies
    otmb_op *op;
    otmb_ctx *ctx;
    hipStream_t st;
    const PdCall &call;  // (restart is the m of the method's description)
    PdWork w{};
    dim3 grid, block;
    bool alx = false;  // X takes the 16-byte path
    std::vector<PdCol> col;
    std::vector<double> hs, yh;  // the host's copy of w.hs (read_hs; hsh), the y of the restarts
    std::string step_msg;        // the text of the first step call that left a column not converged
    std::string msolve_msg;      // the same of the first mean solve
    SvPrec mean_pc{};            // OTMB_OUTER_MEAN: the mean's preconditioner (σ = 0; in w.mp, for all k columns), and P = ncycle·δt
    double period = 0.0;
    std::vector<int64_t> s_it;   // a step call's report
    std::vector<double> s_rr;
    std::vector<int32_t> s_why;

    const double *hsh(i64 c) const { return hs.data() + w.hso(c); }  // column c's scalars as the last read_hs left them
    void fold(i64 c, i64 nq, double *out) { hipLaunchKernelGGL(pd_fold_kernel, dim3(1), block, 0, st, (const double *)w.partc(c), w.np, nq, out); }
    SvD d() const { return call.d.at(0); }  // one d for every column, or D (n x k); of a list of blocks, the first
    const double *dir(i64 c, i64 i) const { return call.outer == OTMB_OUTER_MEAN ? w.z(c, i) : w.v(c, i); }  // the direction Φ is applied to in iteration i
    int32_t prepare();
    int32_t mean_setup();
    int32_t msolve(std::vector<PdItem> &items);
    int32_t read_hs();
    double *sources(bool first) const { return call.src.nsrc > 1 ? w.Sg : first && call.use_x0 ? w.V : w.Sb; }  // where a step call's gathered sources go
    int32_t cycle(std::vector<PdItem> &items, bool withS, double *sbuf);
    void defect_of(i64 c, i64 p, bool minus_x);
    void judged(i64 c, double beta);
    int32_t source_norms(std::vector<PdItem> &items);
    int32_t first_call(std::vector<PdItem> &items);
    void orthogonalise(i64 c, i64 i, i64 p);
    int32_t advance(i64 c);
    int32_t round(bool &more);
    int32_t report();
};

int32_t PdRun::prepare() {
    int32_t rc;
    const bool mean = call.outer == OTMB_OUTER_MEAN;
    if ((rc = pd_work(op, call.k, call.restart, mean ? call.restart : 0, mean ? sv_prec_doubles(op->n, call.precond == OTMB_PRECOND_LINES, sv_prec_cols(d(), call.k)) : 0, d().percol(), call.src.nsrc, call.d.nd, w))) return rc;
    grid = dim3((unsigned)w.np), block = dim3(256);
    alx = ((uintptr_t)call.X & 15) == 0 && (call.ldx & 1) == 0;
    col.resize((size_t)call.k);
    hs.resize((size_t)(2 * (call.restart + 2) * call.k)), yh.resize((size_t)(call.restart * call.k));
    return OTMB_OK;
}

int32_t PdRun::read_hs() {
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hs.data(), w.hs, hs.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return OTMB_OK;
}

// OTMB_OUTER_MEAN, once per call and before X is touched: the mean values Σ_s wt[s]·(slot s) into op->mean, wt the schedule's mean weights
// (the slots' shares of the cycle's steps), and their preconditioner at σ = 0 (a singular one is refused here).
int32_t PdRun::mean_setup() {
    const i64 nslots = (i64)op->slots.size();
    int32_t rc;
    for (DevBuf *b : {&op->mean.nz, &op->mean.val}) {  // at their exact sizes, like the slots
        const size_t bytes = std::max<size_t>((size_t)(b == &op->mean.nz ? op->nnz : op->nval) * 8, 8);
        if (b->p && b->cap == bytes) continue;
        if (b->p) (void)hipFree(b->p);
        b->p = nullptr, b->cap = 0;
        if (hipMalloc(&b->p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            b->p = nullptr;
            return otmb_fail(ctx, OTMB_ERR_ALLOC, "hipMalloc (periodic: the mean values)");
        }
        b->cap = bytes;
    }
    std::vector<double> wt((size_t)nslots);
    call.sched.mean_weights(call.nsteps, nslots, wt.data());
    if ((rc = cb_combine(op, wt.data(), op->mean))) return rc;
    SvD dm = d();
    if (call.d.nd > 1) {  // d̄: the fold of the d blocks under the same weights -- the slots with a weight that is not zero, in ascending order
        std::vector<const double *> blocks;
        std::vector<double> terms;
        for (i64 s = 0; s < nslots; ++s)
            if (wt[(size_t)s] != 0.0) blocks.push_back(call.d.D[s]), terms.push_back(wt[(size_t)s]);
        if ((rc = se_fold(op, blocks, terms, w.n, sv_prec_cols(d(), call.k), call.d.ldd, w.dbar, w.ld))) return rc;
        dm = SvD{w.dbar, d().percol() ? w.ld : 0};
    }
    period = (double)call.nsteps * call.dt;
    mean_pc = sv_prec_carve(w.mp, w.n, call.precond == OTMB_PRECOND_LINES, sv_prec_cols(d(), call.k), d().percol());
    SvValues on(op, op->mean);
    if ((rc = sv_prec_prepare(op, call.adjoint, call.precond, dm, 0.0, mean_pc))) ctx->err += " (the cycle-mean operator)";
    return rc;
}

// OTMB_OUTER_MEAN: Z_i = V_i + M̄⁻¹·V_i / P for `items` (the columns that iterate; from = i).  One solve for all of them, gathered compactly:
// right-hand sides in Sb (no source is in use in an iterating round), answers in W.  A solve that leaves columns not converged stops those
// (PRECOND_FAILED) and is repeated without them; a column's msolve_iters counts the solve that completes, and the one that stopped it.
int32_t PdRun::msolve(std::vector<PdItem> &items) {
    const i64 n = w.n, ld = w.ld;
    while (!items.empty()) {
        const i64 kk = (i64)items.size();
        for (i64 p = 0; p < kk; ++p)
            HIP_TRY(ctx, hipMemcpyAsync(w.Sb + p * ld, w.v(items[(size_t)p].col, items[(size_t)p].from), (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        s_it.assign((size_t)kk, 0), s_rr.assign((size_t)kk, 0.0), s_why.assign((size_t)kk, 0);
        SvPrec pc = mean_pc;
        if (d().percol()) {  // the solve's column p is column items[p].col: its arrays of the preconditioner, gathered (u is every column's)
            pc = sv_prec_carve(w.mpg, n, call.precond == OTMB_PRECOND_LINES, call.k, true);
            pc.u = mean_pc.u;
            double *const from[] = {mean_pc.sh, mean_pc.diag, mean_pc.m, mean_pc.piv}, *const to[] = {pc.sh, pc.diag, pc.m, pc.piv};
            for (int a = 0; a < (pc.m ? 4 : 2); ++a)
                for (i64 p = 0; p < kk; ++p)
                    HIP_TRY(ctx, hipMemcpyAsync(to[a] + p * n, from[a] + items[(size_t)p].col * n, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        }
        int32_t rc;
        {
            SvValues on(op, op->mean);
            rc = sv_solve(op, call.adjoint, kk, pc, w.Sb, ld, w.W, ld, 0, call.rtol, call.maxiter, s_it.data(), s_rr.data(), s_why.data(), call.precond);
        }
        if (rc == OTMB_OK) {
            for (i64 p = 0; p < kk; ++p) {
                const PdItem &it = items[(size_t)p];
                col[(size_t)it.col].msolve_iters += s_it[(size_t)p];
                hipLaunchKernelGGL(pd_precond_kernel, grid, block, 0, st, n, (const double *)w.v(it.col, it.from), (const double *)(w.W + p * ld), period,
                                   w.z(it.col, it.from));
            }
            return OTMB_OK;
        }
        if (rc != OTMB_ERR_NOT_CONVERGED) return rc;
        if (msolve_msg.empty()) msolve_msg = ctx->err;
        std::vector<PdItem> left;
        for (i64 p = 0; p < kk; ++p) {
            PdCol &q = col[(size_t)items[(size_t)p].col];
            if (s_why[(size_t)p] != OTMB_SOLVE_CONVERGED) {
                q.msolve_iters += s_it[(size_t)p];
                q.stop(OTMB_PERIODIC_PRECOND_FAILED);
            } else {
                left.push_back(items[(size_t)p]);
            }
        }
        if (left.size() == items.size()) return otmb_fail(ctx, OTMB_ERR_HIP, "periodic: a mean solve failed without a failing column");  // (cannot happen)
        items.swap(left);
    }
    return OTMB_OK;
}

// One step call for `items` (in this order, compact in W from column 0; withS: their sources, gathered into sbuf, block j's kk columns
// behind block j - 1's): W = the cycle's end states.  A call that leaves columns not converged stops those (STEP_FAILED) and is repeated without them; the call that completes
// counts one cycle for each of its columns.  items comes back as the columns of that call (their positions in W).
int32_t PdRun::cycle(std::vector<PdItem> &items, bool withS, double *sbuf) {
    const i64 n = w.n, ld = w.ld;
    while (!items.empty()) {
        const i64 kk = (i64)items.size();
        for (i64 p = 0; p < kk; ++p) {
            const PdItem &it = items[(size_t)p];
            if (it.from == -2)
                HIP_TRY(ctx, hipMemsetAsync(w.W + p * ld, 0, (size_t)n * 8, st));
            else
                HIP_TRY(ctx, hipMemcpyAsync(w.W + p * ld, it.from >= 0 ? dir(it.col, it.from) : call.X + it.col * call.ldx, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
            for (i64 j = 0; withS && j < call.src.nsrc; ++j)
                HIP_TRY(ctx, hipMemcpyAsync(sbuf + (j * kk + p) * ld, call.src.S[j] + it.col * call.src.lds, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
            for (i64 j = 0; d().percol() && j < call.d.nd; ++j)
                HIP_TRY(ctx, hipMemcpyAsync(w.Dg + (j * kk + p) * ld, call.d.D[j] + it.col * call.d.ldd, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
        }
        s_it.assign((size_t)(call.nsteps * kk), 0), s_rr.assign((size_t)(call.nsteps * kk), 0.0), s_why.assign((size_t)(call.nsteps * kk), 0);
        int64_t done = 0;
        std::vector<const double *> sp((size_t)(withS ? call.src.nsrc : 0));
        for (size_t j = 0; j < sp.size(); ++j) sp[j] = sbuf + (i64)j * kk * ld;
        std::vector<const double *> dp((size_t)call.d.nd);  // the step call's d blocks: the gathered columns, or the shared blocks as they are
        for (size_t j = 0; j < dp.size(); ++j) dp[j] = d().percol() ? w.Dg + (i64)j * kk * ld : call.d.D[j];
        // the cycle as a step call of the gathered columns, under the name of the step export of this call's family and behind its checks
        StCall step = {call, &done, s_it.data(), s_rr.data(), s_why.data(), ST_PLAIN};
        step.call = call.season ? "otmb_op_step_season" : call.sched.listed ? "otmb_op_step_interp" : "otmb_op_step_sched";
        step.sched_checks = true;
        step.k = kk, step.X = w.W, step.ldx = ld;
        step.d = StD{(i64)dp.size(), dp.data(), d().percol() ? ld : 0};
        step.src = StSrc{(i64)sp.size(), sp.data(), ld, nullptr};
        const int32_t rc = st_call<true>(op, step);
        if (rc == OTMB_OK) {
            std::vector<char> seen((size_t)call.k, 0);  // (the first call holds a column twice: one call, one cycle)
            for (const PdItem &it : items)
                if (!seen[(size_t)it.col]++) col[(size_t)it.col].cycles += 1;
            return OTMB_OK;
        }
        if (rc == OTMB_ERR_SINGULAR_PRECONDITIONER && d().percol()) {
            // the step names the column by its place in the gathered block: the caller reads its own column and k.  (items hold the columns
            // in rising order, a second copy of each behind them in the first call, so the smallest place is the smallest column.)
            const size_t at = ctx->err.rfind(" (column "), end = at == std::string::npos ? at : ctx->err.find(')', at);
            long long place = 0;
            if (end != std::string::npos && sscanf(ctx->err.c_str() + at, " (column %lld", &place) == 1 && place >= 1 && place <= kk)
                ctx->err.replace(at, end + 1 - at, " (column " + std::to_string(items[(size_t)(place - 1)].col + 1) + " of " + std::to_string(call.k) + ")");
        }
        if (rc != OTMB_ERR_NOT_CONVERGED) return rc;
        if (step_msg.empty()) step_msg = ctx->err;
        std::vector<PdItem> left;
        for (i64 p = 0; p < kk; ++p)
            if (s_why[(size_t)(done * kk + p)] != OTMB_SOLVE_CONVERGED) col[(size_t)items[(size_t)p].col].stop(OTMB_PERIODIC_STEP_FAILED);
        for (const PdItem &it : items)
            if (col[(size_t)it.col].phase != PD_STOPPED) left.push_back(it);
        if (left.size() == items.size()) return otmb_fail(ctx, OTMB_ERR_HIP, "periodic: a step call failed without a failing column");  // (cannot happen)
        items.swap(left);
    }
    return OTMB_OK;
}

// r = W[p] - x (or W[p]) -> V_0 of column c, ‖r‖² -> hs[c][0]
void PdRun::defect_of(i64 c, i64 p, bool minus_x) {
    hipLaunchKernelGGL(pd_defect_kernel, grid, block, 0, st, w.n, (const double *)(w.W + p * w.ld), minus_x ? (const double *)(call.X + c * call.ldx) : nullptr, alx,
                       w.v(c, 0), w.partc(c));
    fold(c, 1, w.hsc(c));
}

// column c starts a Krylov space from its explicit r (in V_0, norm beta), or is accepted on it
void PdRun::judged(i64 c, double beta) {
    PdCol &q = col[(size_t)c];
    q.defect = beta / q.gnorm;
    if (!std::isfinite(beta)) return q.stop(OTMB_PERIODIC_NONFINITE);
    if (beta <= call.ptol * q.gnorm) return q.stop(OTMB_PERIODIC_CONVERGED);
    hipLaunchKernelGGL(pd_scale_kernel, grid, block, 0, st, w.n, w.v(c, 0), beta);
    q.phase = PD_ARNOLDI;
    q.ls.start(call.restart, beta);
}

// the sources' norms, block by block: a column that is zero in every block has g = 0.  items: the columns of the first call
int32_t PdRun::source_norms(std::vector<PdItem> &items) {
    int32_t rc;
    std::vector<char> zero((size_t)call.k, 1);
    for (i64 j = 0; j < call.src.nsrc; ++j) {
        for (i64 c = 0; c < call.k; ++c) {
            HIP_TRY(ctx, hipMemcpyAsync(w.W + c * w.ld, call.src.S[j] + c * call.src.lds, (size_t)w.n * 8, hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(pd_defect_kernel, grid, block, 0, st, w.n, (const double *)(w.W + c * w.ld), (const double *)nullptr, false, (double *)nullptr, w.partc(c));
            fold(c, 1, w.hsc(c));
        }
        if ((rc = read_hs())) return rc;
        for (i64 c = 0; c < call.k; ++c)
            if (!(hsh(c)[0] == 0.0)) zero[(size_t)c] = 0;
    }
    for (i64 c = 0; c < call.k; ++c) {
        PdCol &q = col[(size_t)c];
        if (zero[(size_t)c]) {
            q.stop(OTMB_PERIODIC_CONVERGED), q.defect = 0.0;
        } else if (call.maxcycles < 1) {
            q.stop(OTMB_PERIODIC_MAXCYCLES);
        } else {
            items.push_back({c, call.use_x0 ? (i64)-1 : (i64)-2});
        }
    }
    return OTMB_OK;
}

// the first call: F(x) (and, with a start, g beside it), then every live column's first explicit r
int32_t PdRun::first_call(std::vector<PdItem> &items) {
    const i64 n = w.n, ld = w.ld;
    int32_t rc;
    if (call.use_x0)
        for (size_t p = 0, live = items.size(); p < live; ++p) items.push_back({items[p].col, -2});
    if ((rc = cycle(items, true, sources(true)))) return rc;  // (with a start one block's 2k sources lie in the bases, which are not in use yet)
    // from here on X is written: the zero columns, and a start of zero
    for (i64 c = 0; c < call.k; ++c)
        if (!call.use_x0 || (col[(size_t)c].phase == PD_STOPPED && col[(size_t)c].reason == OTMB_PERIODIC_CONVERGED))
            HIP_TRY(ctx, hipMemsetAsync(call.X + c * call.ldx, 0, (size_t)n * 8, st));
    const i64 live = call.use_x0 ? (i64)items.size() / 2 : (i64)items.size();
    if (call.use_x0)  // ‖g‖² first: the defect's fold would overwrite the same slot, so it goes to the second half of the column's scalars
        for (i64 p = 0; p < live; ++p) {
            const i64 c = items[(size_t)p].col;
            hipLaunchKernelGGL(pd_defect_kernel, grid, block, 0, st, n, (const double *)(w.W + (live + p) * ld), (const double *)nullptr, false, (double *)nullptr,
                               w.partc(c));
            fold(c, 1, w.hsc(c) + (call.restart + 2));
        }
    for (i64 p = 0; p < live; ++p) defect_of(items[(size_t)p].col, p, call.use_x0 != 0);
    if ((rc = read_hs())) return rc;
    for (i64 p = 0; p < live; ++p) {
        const i64 c = items[(size_t)p].col;
        PdCol &q = col[(size_t)c];
        const double beta = std::sqrt(hsh(c)[0]);
        q.gnorm = call.use_x0 ? std::sqrt(hsh(c)[call.restart + 2]) : beta;
        if (q.gnorm == 0.0) {  // (a source that is not zero whose cycle underflows to zero)
            HIP_TRY(ctx, hipMemsetAsync(call.X + c * call.ldx, 0, (size_t)n * 8, st));
            q.stop(OTMB_PERIODIC_CONVERGED), q.defect = 0.0;
        } else if (!std::isfinite(q.gnorm)) {
            q.stop(OTMB_PERIODIC_NONFINITE);
        } else {
            judged(c, beta);
        }
    }
    return OTMB_OK;
}

// iteration i of column c on the device, from Φ·V_i in W[p] (OTMB_OUTER_MEAN: Z_i for V_i): w = V_i - Φ·V_i into V_{i+1}, then CGS2 against V_0..i; h', h'' and ‖w‖² -> hs[c]
void PdRun::orthogonalise(i64 c, i64 i, i64 p) {
    const i64 n = w.n, ld = w.ld, np = w.np;
    double *wv = w.v(c, i + 1), *h1 = w.hsc(c), *h2 = w.hsc(c) + (call.restart + 2);
    const double *V = w.v(c, 0);
    hipLaunchKernelGGL(pd_defect_kernel, grid, block, 0, st, n, dir(c, i), (const double *)(w.W + p * ld), true, wv, (double *)nullptr);
    for (int pass = 0; pass < 2; ++pass) {
        double *h = pass ? h2 : h1;
        op_blocks<PD_NB>(0, i + 1, [&](auto nb, i64 j0) {
            constexpr int NB = decltype(nb)::value;
            hipLaunchKernelGGL((j0 == 0 ? pd_dots_kernel<NB, true> : pd_dots_kernel<NB, false>), grid, block, 0, st, n, V + j0 * ld, ld, (const double *)wv,
                               w.partc(c) + j0 * np, np, w.partc(c) + (i + 1) * np);
        });
        fold(c, i + 2, h);
        if (pass == 0) {
            hipLaunchKernelGGL(pd_update_kernel<false>, grid, block, 0, st, n, V, ld, i + 1, (const double *)h, wv, (double *)nullptr);
        } else {
            hipLaunchKernelGGL(pd_update_kernel<true>, grid, block, 0, st, n, V, ld, i + 1, (const double *)h, wv, w.partc(c) + (i + 1) * np);
            hipLaunchKernelGGL(pd_fold_kernel, dim3(1), block, 0, st, (const double *)(w.partc(c) + (i + 1) * np), np, (i64)1, h + (i + 1));
        }
    }
}

// the host's part of column c's iteration, from the scalars read_hs left: the triangle's new column, then the next basis vector or,
// where the column ends its Krylov space, y, x += V·y and the verifying cycle next
int32_t PdRun::advance(i64 c) {
    PdCol &q = col[(size_t)c];
    const i64 i = q.ls.i;
    double hn, est;
    if (!q.ls.push(hsh(c), hsh(c) + (call.restart + 2), &hn, &est)) {
        q.stop(OTMB_PERIODIC_NONFINITE);
        return OTMB_OK;
    }
    if (!(est <= call.ptol * q.gnorm || q.ls.i == call.restart || hn == 0.0 || q.cycles + 1 >= call.maxcycles)) {
        hipLaunchKernelGGL(pd_scale_kernel, grid, block, 0, st, w.n, w.v(c, i + 1), hn);
        return OTMB_OK;
    }
    double *y = yh.data() + c * call.restart;
    q.ls.solve(y);
    HIP_TRY(ctx, hipMemcpyAsync(w.yv + c * call.restart, y, (size_t)q.ls.i * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(pd_combine_kernel, grid, block, 0, st, w.n, dir(c, 0), w.ld, q.ls.i, (const double *)(w.yv + c * call.restart), call.X + c * call.ldx, alx);
    q.phase = PD_VERIFY;
    return OTMB_OK;
}

// one round: one step call for the columns that iterate, one for those that verify.  more = false: every column has stopped
int32_t PdRun::round(bool &more) {
    int32_t rc;
    std::vector<PdItem> ia, iv;
    for (i64 c = 0; c < call.k; ++c) {
        PdCol &q = col[(size_t)c];
        if (q.phase == PD_ARNOLDI && q.ls.i == 0 && q.cycles + 2 > call.maxcycles) q.stop(OTMB_PERIODIC_MAXCYCLES);  // no verifying cycle could follow
        if (q.phase == PD_ARNOLDI) ia.push_back({c, q.ls.i});
        if (q.phase == PD_VERIFY) iv.push_back({c, -1});
    }
    more = !(ia.empty() && iv.empty());
    if (!more) return OTMB_OK;
    if (call.outer == OTMB_OUTER_MEAN && (rc = msolve(ia))) return rc;
    if ((rc = cycle(ia, false, nullptr))) return rc;
    for (size_t p = 0; p < ia.size(); ++p) orthogonalise(ia[p].col, ia[p].from, (i64)p);
    if ((rc = cycle(iv, true, sources(false)))) return rc;
    for (size_t p = 0; p < iv.size(); ++p) defect_of(iv[p].col, (i64)p, true);
    if ((rc = read_hs())) return rc;
    for (const PdItem &it : iv) judged(it.col, std::sqrt(hsh(it.col)[0]));
    for (const PdItem &it : ia)
        if ((rc = advance(it.col))) return rc;
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t PdRun::report() {
    int64_t *cycles = call.cycles, *msolve_iters = call.msolve_iters;
    double *defect = call.defect;
    int32_t *reason = call.reason;
    for (i64 c = 0; c < call.k; ++c) cycles[c] = col[(size_t)c].cycles, defect[c] = col[(size_t)c].defect, reason[c] = col[(size_t)c].reason;
    if (msolve_iters)
        for (i64 c = 0; c < call.k; ++c) msolve_iters[c] = col[(size_t)c].msolve_iters;
    static const char *const names[] = {"converged", "maxcycles", "step failed", "nonfinite", "precond failed"};
    return sv_report_open(ctx, "periodic: %lld of %lld columns; the first is column %lld: %s after %lld cycles, defect %.3e", names, call.k, reason, cycles, defect,
                          (step_msg.empty() ? step_msg : "; the step: " + step_msg) + (msolve_msg.empty() ? msolve_msg : "; the mean solve: " + msolve_msg), 5);
}

// The call proper: device pointers (c.src.S, c.d.D: host arrays of them), the arguments checked.
static int32_t pd_run(otmb_op *op, const PdCall &c) {
    int32_t rc;
    otmb_ctx *ctx = op->ctx;
    // the trivial answers: no rows, no source
    if (op->n == 0) return pd_all_zero(c.k, c.cycles, c.defect, c.reason, c.msolve_iters);
    HIP_TRY(ctx, hipSetDevice(op->device));
    if (c.src.nsrc == 0) {
        HIP_TRY(ctx, hipMemset2DAsync(c.X, (size_t)c.ldx * 8, 0, (size_t)op->n * 8, (size_t)c.k, ctx->stream));
        return pd_all_zero(c.k, c.cycles, c.defect, c.reason, c.msolve_iters);
    }
    PdRun r{op, ctx, ctx->stream, c};
    std::vector<PdItem> items;
    if ((rc = r.prepare()) || (c.outer == OTMB_OUTER_MEAN && (rc = r.mean_setup())) || (rc = r.source_norms(items)) || (rc = r.first_call(items))) return rc;
    for (bool more = true; more;)
        if ((rc = r.round(more))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (yh's uploads have been read)
    return r.report();
}

// One body for every periodic call (DEV: device pointers).  The host variant stages the start, every source block and every d block once
// (op_stage_call) and brings X home once.
template <bool DEV>
static int32_t pd_call(otmb_op *op, const PdCall &c) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = pd_check(op, c))) return rc;
    if (DEV) return pd_run(op, c);
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    const i64 n = op->n;
    OpStaged g;
    if ((rc = op_stage_call(op, c.k, c.d, c.src, c.use_x0 ? c.X : nullptr, c.ldx, g))) return rc;
    PdCall dev = c;
    dev.d = g.d, dev.src = g.src, dev.X = g.X, dev.ldx = n;
    rc = pd_run(op, dev);
    if (rc != OTMB_OK && rc != OTMB_ERR_NOT_CONVERGED) return rc;
    return op_finish(ctx, rc, c.X, c.ldx, g.X, n, c.k);
}

extern "C" {

// the listed schedule with d and the source per slot: nd, D (nd pointers), ldd in place of D, ldd; F is the step call of otmb_op_step_season
int32_t otmb_op_periodic_season_dev(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta,
                                    int64_t ncycle, const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S,
                                    int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol,
                                    int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    return pd_call<true>(op, {{"otmb_op_periodic_season", true, true, adjoint, k, StD{nd, D, ldd}, dt, theta, ncycle, StSched::list(slot_a, slot_b, weight), StSrc{nsrc, S, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

int32_t otmb_op_periodic_season(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds, double *X,
                                int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles,
                                int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    return pd_call<false>(op, {{"otmb_op_periodic_season", true, true, adjoint, k, StD{nd, D, ldd}, dt, theta, ncycle, StSched::list(slot_a, slot_b, weight), StSrc{nsrc, S, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

// the cyclic schedule with sub-steps and a list of source blocks; F is the step call of otmb_op_step_sched
int32_t otmb_op_periodic_sched_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                   int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, double *X, int64_t ldx,
                                   int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles,
                                   int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    const double *const one[1] = {D};
    return pd_call<true>(op, {{"otmb_op_periodic_sched", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, ncycle, StSched::cyclic(first_slot, substeps), StSrc{nsrc, S, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

int32_t otmb_op_periodic_sched(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                               int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0,
                               double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect,
                               int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    const double *const one[1] = {D};
    return pd_call<false>(op, {{"otmb_op_periodic_sched", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, ncycle, StSched::cyclic(first_slot, substeps), StSrc{nsrc, S, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

// the listed schedule: slot_a, slot_b, weight (ncycle host values each) in place of first_slot, substeps; F is the step call of otmb_op_step_interp
int32_t otmb_op_periodic_interp_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                    const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                                    double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart,
                                    int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    const double *const one[1] = {D};
    return pd_call<true>(op, {{"otmb_op_periodic_interp", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, ncycle, StSched::list(slot_a, slot_b, weight), StSrc{nsrc, S, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

int32_t otmb_op_periodic_interp(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds, double *X,
                                int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles,
                                int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    const double *const one[1] = {D};
    return pd_call<false>(op, {{"otmb_op_periodic_interp", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, ncycle, StSched::list(slot_a, slot_b, weight), StSrc{nsrc, S, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

// the calls from before the schedule: substeps = 1, the one source or none, none of the schedule's checks
int32_t otmb_op_periodic_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter,
                                int32_t precond, double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason,
                                int32_t outer, int64_t *msolve_iters) {
    const double *const one[1] = {D}, *const src[1] = {S};
    return pd_call<true>(op, {{"otmb_op_periodic_dk", false, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, ncycle, StSched::cyclic(first_slot, 1), StSrc{S ? 1 : 0, src, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

int32_t otmb_op_periodic_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle, int64_t first_slot,
                            const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol,
                            int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    const double *const one[1] = {D}, *const src[1] = {S};
    return pd_call<false>(op, {{"otmb_op_periodic_dk", false, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, ncycle, StSched::cyclic(first_slot, 1), StSrc{S ? 1 : 0, src, lds, nullptr},
                            X, ldx, rtol, maxiter, precond},
                           use_x0, ptol, restart, maxcycles, outer, cycles, defect, reason, msolve_iters});
}

// the calls with one d for every column: ldd = 0 (otmb_op_periodic: OTMB_OUTER_NONE as well)
int32_t otmb_op_periodic_pc_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                                const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond,
                                double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer,
                                int64_t *msolve_iters) {
    return otmb_op_periodic_dk_dev(op, adjoint, k, d, 0, dt, theta, ncycle, first_slot, S, lds, X, ldx, use_x0, rtol, maxiter, precond, ptol, restart, maxcycles,
                                   cycles, defect, reason, outer, msolve_iters);
}

int32_t otmb_op_periodic_pc(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                            const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol,
                            int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters) {
    return otmb_op_periodic_dk(op, adjoint, k, d, 0, dt, theta, ncycle, first_slot, S, lds, X, ldx, use_x0, rtol, maxiter, precond, ptol, restart, maxcycles,
                               cycles, defect, reason, outer, msolve_iters);
}

int32_t otmb_op_periodic_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                             const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond,
                             double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason) {
    return otmb_op_periodic_pc_dev(op, adjoint, k, d, dt, theta, ncycle, first_slot, S, lds, X, ldx, use_x0, rtol, maxiter, precond, ptol, restart, maxcycles,
                                   cycles, defect, reason, OTMB_OUTER_NONE, nullptr);
}

int32_t otmb_op_periodic(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                         const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol,
                         int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason) {
    return otmb_op_periodic_pc(op, adjoint, k, d, dt, theta, ncycle, first_slot, S, lds, X, ldx, use_x0, rtol, maxiter, precond, ptol, restart, maxcycles, cycles,
                               defect, reason, OTMB_OUTER_NONE, nullptr);
}

}  // extern "C"
