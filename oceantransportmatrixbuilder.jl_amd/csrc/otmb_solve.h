// otmb_solve.h -- what the solver (otmb_solve.hip) and its line preconditioner (otmb_solve_lines.hip) share: a column's record and
// state, the register block of right-hand sides, and the host entry points of the line kernels.
#pragma once
#include "otmb_op.h"

#define SV_KB 4  // the solver's largest register block of columns (op_blocks: 4, 2, 1)

enum { SV_ACTIVE = 0, SV_VERIFY = 1, SV_STOPPED = 2 };  // state; a stopped column's reason: otmb_solve_reason

struct SvCol {  // one column's record (device; the host reads all k of them)
    double rho, alpha, omega, beta, bnorm, relres, rhn;  // rhn = ‖r̂‖
    int state, reason, restart, bzero;
    i64 iters;
};

// The line preconditioner (otmb_solve_lines.hip); both enqueue on the context's stream and need op->lines.
// ln_factor: u, l from the CSC copy, then pivots and multipliers head to tail.  diag: Jacobi's diagonal (a).  m, u, piv: n doubles each.
//            *bad (preset to ~0) receives the smallest 0-based index whose pivot is zero or not finite.
// ln_sweep:  Z = P⁻¹·Y for the columns whose record is SV_ACTIVE (cs == nullptr: every column).  Y and Z may be the same array.
void ln_factor(otmb_op *op, int adjoint, const double *diag, double *m, double *u, double *piv, unsigned long long *bad);
void ln_sweep(otmb_op *op, const SvCol *cs, i64 k, const double *m, const double *u, const double *piv, const double *Y, i64 ldy, double *Z,
              i64 ldz);

// A prepared preconditioner: sh = σ + d, diag (Jacobi's diagonal) and, for the lines, the multipliers, u and the pivots -- n doubles each
// (m, u, piv: null for Jacobi).  For a fixed (values, d, σ, adjoint) the arrays are always the same bits, so otmb_op_step (otmb_step.hip)
// computes them once per slot and call.
struct SvPrec {
    double *sh, *diag, *m, *u, *piv;
};
// sv_prec_prepare: computes p's arrays from the SELECTED values; a singular preconditioner is refused (OTMB_ERR_SINGULAR_PRECONDITIONER).
//                  Waits for the device.
// sv_solve:        otmb_op_solve_pc_dev without its argument checks; prep != nullptr: d and σ are not read, the preconditioner is prep's.
// sv_check_step:   the argument checks the step shares with the solver (S may be null), then `more`, then the preconditioner.
int32_t sv_prec_prepare(otmb_op *op, int adjoint, int32_t precond, const double *d, double sigma, const SvPrec &p);
int32_t sv_solve(otmb_op *op, int adjoint, i64 k, const double *d, double sigma, const double *B, i64 ldb, double *X, i64 ldx, int use_x0, double rtol,
                 i64 maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond, const SvPrec *prep);
int32_t sv_check_step(otmb_op *op, int32_t precond, int64_t k, const double *S, int64_t lds, double *X, int64_t ldx, const char *more);
