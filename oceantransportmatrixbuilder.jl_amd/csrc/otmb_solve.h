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
