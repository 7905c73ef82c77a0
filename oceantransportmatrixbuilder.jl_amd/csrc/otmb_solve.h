// otmb_solve.h -- what the solver (otmb_solve.hip), its line preconditioner (otmb_solve_lines.hip), the step (otmb_step.hip) and the periodic
// state (otmb_periodic.hip) share: a column's record and state, the register block of right-hand sides, the preconditioner's record, the
// host entry points around it, the step's argument checks, the call records of the step and the periodic state (StCall, PdCall) and the
// report of columns that did not converge.  The schedule's own types and rules are otmb_sched.h's, which otmb_op.h includes.
#pragma once
#include "otmb_op.h"

#define SV_KB 4  // the solver's largest register block of columns (op_blocks: 4, 2, 1)

enum { SV_ACTIVE = 0, SV_VERIFY = 1, SV_STOPPED = 2 };  // state; a stopped column's reason: otmb_solve_reason

struct SvCol {  // one column's record (device; the host reads all k of them)
    double rho, alpha, omega, beta, bnorm, relres, rhn;  // rhn = ‖r̂‖
    int state, reason, restart, bzero;
    i64 iters;
};

// The checks of D and ldd that the _dk calls add (`call`: the export's name), after the call's other checks and before anything is touched
int32_t sv_check_d(otmb_op *op, const char *call, const double *D, int64_t ldd);

// A preconditioner: sh = σ + d, diag (Jacobi's diagonal) and, for the lines, the multipliers, the pivots and u (m, piv, u: null for
// Jacobi).  u does not depend on d and is n doubles; the others are n doubles when d is shared (cs = 0, kc = 1) and n x kc, column c at
// + c·cs, when every column has its own d (cs = n, kc = the call's k).  For a fixed (values, d, σ, adjoint) the arrays are always the same
// bits, so otmb_op_step (otmb_step.hip) computes them once per slot and call.
struct SvPrec {
    double *sh, *diag, *m, *piv, *u;
    i64 cs, kc;
};
// the record's doubles, and its arrays in a block of that many: sh | diag | m | piv (n·kc each) | u (n)
static inline size_t sv_prec_doubles(i64 n, bool lines, i64 kc) { return (size_t)(lines ? 4 * kc + 1 : 2 * kc) * (size_t)n; }
static inline SvPrec sv_prec_carve(double *a, i64 n, bool lines, i64 kc, bool percol) {
    const i64 b = n * kc;
    return {a, a + b, lines ? a + 2 * b : nullptr, lines ? a + 3 * b : nullptr, lines ? a + 4 * b : nullptr, percol ? n : 0, kc};
}
// the columns a preconditioner for d and k columns holds
static inline i64 sv_prec_cols(const SvD &d, i64 k) { return d.percol() ? k : 1; }
// Column c's offset into arrays that are per column (PC: c·stride) or one for all (0).  The kernels that read sh, diag, m, piv or d inside a
// register block are templates on PC: with one d the offset is the constant 0, the block's KB reads are one load of one address, and the
// instantiation is the kernel as it was before columns could have their own d, in instructions and registers.
template <bool PC>
__device__ __forceinline__ i64 sv_pc(int c, i64 stride) {
    return PC ? c * stride : 0;
}

// The line preconditioner (otmb_solve_lines.hip); both enqueue on the context's stream and need op->lines.
// ln_factor: p.u and l (n doubles of scratch, which the factorisation alone reads) from the CSC copy, then every column's p.piv and p.m
//            head to tail, from its p.diag (Jacobi's diagonal, a).  *bad (preset to ~0) receives the smallest (column << 32 | 0-based
//            index) whose pivot is zero or not finite: the smallest column that has one, and its first.
// ln_sweep:  Z = P⁻¹·Y for the columns whose record is SV_ACTIVE (cs == nullptr: every column).  Y and Z may be the same array.
void ln_factor(otmb_op *op, int adjoint, const SvPrec &p, double *l, unsigned long long *bad);
void ln_sweep(otmb_op *op, const SvCol *cs, i64 k, const SvPrec &p, const double *Y, i64 ldy, double *Z, i64 ldz);

// sv_prec_prepare: computes p's arrays (p.kc columns of them) from the SELECTED values; a singular preconditioner is refused
//                  (OTMB_ERR_SINGULAR_PRECONDITIONER; per column: the message names the smallest column).  Waits for the device.
// sv_solve:        otmb_op_solve_pc_dev (n > 0) after its argument checks and its preconditioner: p is prepared, for this adjoint and
//                  precond and for the call's d, σ and selected values.
// sv_check_step:   the argument checks the step shares with the solver (S may be null), then `more`, then the preconditioner.
int32_t sv_prec_prepare(otmb_op *op, int adjoint, int32_t precond, const SvD &d, double sigma, const SvPrec &p);
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

// The blended values of otmb_op_step_interp (otmb_interp.hip).
// ip_reserve: op->interp at the slots' sizes (allocated on first use; may wait for the device).
// ip_blend:   wa·(slot a) + wb·(slot b) into both value arrays of op->interp, ONE launch enqueued on the context's stream.
int32_t ip_reserve(otmb_op *op);
int32_t ip_blend(otmb_op *op, i64 a, i64 b, double wa, double wb);


// The fold of dense blocks (otmb_season.hip): a blended step's d and source, and the cycle-mean d̄.
// se_reserve: op->season at that many doubles (allocated on first use; may wait for the device).
// se_fold:    Σ_t wt[t]·src[t] in the vectors' order (each rows x cols with leading dimension ld) into dst (leading dimension ldo), ONE launch
//             enqueued on the context's stream; more than 16 terms travel through a device table, whose write waits for the stream.
int32_t se_reserve(otmb_op *op, size_t doubles);
int32_t se_fold(otmb_op *op, const std::vector<const double *> &src, const std::vector<double> &wt, i64 rows, i64 cols, i64 ld, double *dst, i64 ldo);

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

// What otmb_op_step_obs adds to a step call: q observers W (obs: q x k x nsteps) and the mean's weights and array (null: none).
struct StObs {
    i64 q;
    const double *W;
    i64 ldw;
    double *obs;
    const double *tw;
    double *Xbar;
    i64 ldm;
};
static const StObs ST_PLAIN = {0, nullptr, 0, nullptr, nullptr, nullptr, 0};  // no observers, no mean

// One stepped call, as every export of otmb_step.hip and otmb_periodic.hip states it.  The head is what the two families share:
//   call            the export that refusals cite
//   sched_checks, season   which checks follow the call's own (and sv_check_d, which every call but a season call runs under `call`):
//                   sched_checks -- the schedule's (sv_sched_complaint, or sv_interp_complaint when the schedule is listed) and the scale's; season -- d is a list
//                   of blocks: no sv_check_d, a source per slot is in order under a listed schedule, the list's own checks come last
//   d               at most one block for every call but a season call (a shared d: ldd = 0); per slot, plain steps take their slot's block
//                   and blended steps the fold of the two slots' blocks
//   nsteps          the steps of the call, or of the periodic state's cycle
//   sched           cyclic, or listed: a listed schedule may blend (op->interp, and op->season for fields per slot)
//   src             nsrc = nslots: a block per slot, picked and folded like d; scale: a factor per step and tracer (never periodic)
// A record never outlives its call: the arrays it points at may live on the export's stack.
struct StHead {
    const char *call;
    bool sched_checks, season;
    int32_t adjoint;
    i64 k;
    StD d;
    double dt, theta;
    i64 nsteps;
    StSched sched;
    StSrc src;
    double *X;
    i64 ldx;
    double rtol;
    i64 maxiter;
    int32_t precond;
};
struct StCall : StHead {  // a step call: the head, the report (nsteps x k, step-major) and the observers (ST_PLAIN: none)
    int64_t *steps_done, *iters;
    double *relres;
    int32_t *reason;
    StObs obs;
};
struct PdCall : StHead {  // a periodic call: the head (nsteps = ncycle), the outer iteration's arguments and its report, one entry per column
    int32_t use_x0;
    double ptol;
    i64 restart, maxcycles;
    int32_t outer;
    int64_t *cycles;
    double *defect;
    int32_t *reason;
    int64_t *msolve_iters;
};
// (otmb_step.hip) st_check_sched: the checks `sched_checks` and `season` select, the refusal under h.call.
//                 st_call:        a step call behind its checks; DEV: device pointers (otmb_periodic.hip's cycle is st_call<true>)
int32_t st_check_sched(otmb_op *op, const StHead &h);
template <bool DEV>
int32_t st_call(otmb_op *op, const StCall &c);

// the report of an empty system (n = 0): every entry converged at once
static inline int32_t sv_report_empty(i64 entries, int64_t *iters, double *relres, int32_t *reason) {
    for (i64 e = 0; e < entries; ++e) { iters[e] = 0; relres[e] = 0.0; reason[e] = OTMB_SOLVE_CONVERGED; }
    return OTMB_OK;
}
