// otmb_solve.h -- what the solver (otmb_solve.hip), its line preconditioner (otmb_solve_lines.hip), the step (otmb_step.hip) and the periodic
// state (otmb_periodic.hip) share: a column's record and state, the register block of right-hand sides, the preconditioner's record, the
// host entry points around it, the step's argument checks and the report of columns that did not converge.
#pragma once
#include "otmb_op.h"

#define SV_KB 4  // the solver's largest register block of columns (op_blocks: 4, 2, 1)

enum { SV_ACTIVE = 0, SV_VERIFY = 1, SV_STOPPED = 2 };  // state; a stopped column's reason: otmb_solve_reason

struct SvCol {  // one column's record (device; the host reads all k of them)
    double rho, alpha, omega, beta, bnorm, relres, rhn;  // rhn = ‖r̂‖
    int state, reason, restart, bzero;
    i64 iters;
};

// A preconditioner: sh = σ + d, diag (Jacobi's diagonal) and, for the lines, the multipliers, u and the pivots -- n doubles each (m, u, piv:
// null for Jacobi).  For a fixed (values, d, σ, adjoint) the arrays are always the same bits, so otmb_op_step (otmb_step.hip) computes them
// once per slot and call.
struct SvPrec {
    double *sh, *diag, *m, *u, *piv;
};
// the record's arrays in a block of (lines ? 5 : 2) * n doubles: sh | diag | m | u | piv
static inline SvPrec sv_prec_carve(double *a, i64 n, bool lines) {
    return {a, a + n, lines ? a + 2 * n : nullptr, lines ? a + 3 * n : nullptr, lines ? a + 4 * n : nullptr};
}

// The line preconditioner (otmb_solve_lines.hip); both enqueue on the context's stream and need op->lines.
// ln_factor: p.u, l from the CSC copy, then p.piv and p.m head to tail, from p.diag (Jacobi's diagonal, a).
//            *bad (preset to ~0) receives the smallest 0-based index whose pivot is zero or not finite.
// ln_sweep:  Z = P⁻¹·Y for the columns whose record is SV_ACTIVE (cs == nullptr: every column).  Y and Z may be the same array.
void ln_factor(otmb_op *op, int adjoint, const SvPrec &p, unsigned long long *bad);
void ln_sweep(otmb_op *op, const SvCol *cs, i64 k, const SvPrec &p, const double *Y, i64 ldy, double *Z, i64 ldz);

// sv_prec_prepare: computes p's arrays from the SELECTED values; a singular preconditioner is refused (OTMB_ERR_SINGULAR_PRECONDITIONER).
//                  Waits for the device.
// sv_solve:        otmb_op_solve_pc_dev (n > 0) after its argument checks and its preconditioner: p is prepared, for this adjoint and
//                  precond and for the call's d, σ and selected values.
// sv_check_step:   the argument checks the step shares with the solver (S may be null), then `more`, then the preconditioner.
int32_t sv_prec_prepare(otmb_op *op, int adjoint, int32_t precond, const double *d, double sigma, const SvPrec &p);
int32_t sv_solve(otmb_op *op, int adjoint, i64 k, const SvPrec &p, const double *B, i64 ldb, double *X, i64 ldx, int use_x0, double rtol, i64 maxiter,
                 int64_t *iters, double *relres, int32_t *reason, int32_t precond);
// sv_step_complaint: the first complaint among rtol, maxiter, dt, theta, the count of steps (count_ok; the caller's text) and first_slot, in
//                  that order, or null: what otmb_op_step and otmb_op_periodic ask of the arguments they share.
// sv_report_open:  the end of a call that reports per column: OTMB_OK when every reason is 0 (converged); otherwise OTMB_ERR_NOT_CONVERGED with
//                  fmt filled from the open columns' number, k, the first of them (1-based), names[its reason], count[it] and value[it],
//                  and `tail` behind it.  names holds nnames texts (a reason beyond them reads as names[0]).
int32_t sv_check_step(otmb_op *op, int32_t precond, int64_t k, const double *S, int64_t lds, double *X, int64_t ldx, const char *more);
const char *sv_step_complaint(const otmb_op *op, double rtol, int64_t maxiter, double dt, double theta, bool count_ok, const char *count_text,
                              int64_t first_slot);
int32_t sv_report_open(otmb_ctx *ctx, const char *fmt, const char *const *names, i64 k, const int32_t *reason, const int64_t *count, const double *value,
                       const std::string &tail = std::string(), int nnames = 4);

// The solver, its preconditioner and the products read the values op->nz / op->val point at (the selected slot's).  SvValues points them at
// another value set of the same pattern for its lifetime: sv_prec_prepare and sv_solve on an explicit value set (the periodic state's mean).
struct SvValues {
    otmb_op *op;
    DevBuf nz, val;
    SvValues(otmb_op *o, const OpSlot &s) : op(o), nz(o->nz), val(o->val) { op->nz = s.nz, op->val = s.val; }
    ~SvValues() { op->nz = nz, op->val = val; }
    SvValues(const SvValues &) = delete;
    SvValues &operator=(const SvValues &) = delete;
};

// cb_combine (otmb_combine.hip): Σ_s w[s]·(slot s) into both value arrays of `to`, a slot of the operator or op->mean; w: nslots finite host
// values.  Enqueued on the context's stream.
int32_t cb_combine(otmb_op *op, const double *w, const OpSlot &to);

// The observation pass (otmb_observe.hip), which the step runs after every completed step.
// ob_reserve:   the partial sums of q x k entries in op->ob (may wait for the stream: before the loop, never inside it).
// ob_pass:      obs (q x k, device) = Wᵀ·X and, Xbar not null, Xbar = (first ? +0.0 : Xbar) + tw·X, enqueued on the context's stream; q == 0
//               runs no reduction, Xbar == null stores nothing but obs.
// ob_complaint: the first complaint about the observers and the mean (tw: nsteps host values), naming otmb_op_step_obs (step) or
//               otmb_op_observe, or null.
int32_t ob_reserve(otmb_op *op, i64 k, i64 q);
void ob_pass(otmb_op *op, i64 k, i64 q, const double *W, i64 ldw, const double *X, i64 ldx, double *obs, double *Xbar, i64 ldm, double tw, bool first);
const char *ob_complaint(const otmb_op *op, bool step, i64 nsteps, i64 q, const double *W, i64 ldw, const double *obs, const double *tw, const double *Xbar,
                         i64 ldm);

// the report of an empty system (n = 0): every entry converged at once
static inline int32_t sv_report_empty(i64 entries, int64_t *iters, double *relres, int32_t *reason) {
    for (i64 e = 0; e < entries; ++e) { iters[e] = 0; relres[e] = 0.0; reason[e] = OTMB_SOLVE_CONVERGED; }
    return OTMB_OK;
}
