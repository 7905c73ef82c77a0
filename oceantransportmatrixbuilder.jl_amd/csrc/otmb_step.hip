// otmb_step.hip -- θ-steps of ∂x/∂t + (diag(d) + A)·x = s on a resident operator whose value slots hold a cycle of matrices (a year of
// monthly transport matrices): otmb_op_step[_dev] advances k tracers through nsteps steps, step t with slot (first_slot + t) mod nslots,
//     (σ·I + diag(d) + A)·x⁺ = b,   σ = 1 / (θ·δt),
//     θ = 1:  b_i = σ·x_i + s_i
//     θ < 1:  w = A·x;  e_i = d_i·x_i + w_i;  b_i = (σ·x_i + s_i/θ) - c·e_i,  c = (1 - θ) / θ
// (adjoint: Aᵀ; without S the s terms are absent, without d e = w), then the solver of otmb_solve.hip from x.  include/otmb.h states this as
// a contract in public calls: every state has the bits of otmb_op_select_slot, otmb_op_mul_dev (α = 1, β = 0), the elementwise line above in
// that association without FMA (-ffp-contract=off), otmb_op_solve_pc_dev with use_x0 = 1.
//
// What the call saves over that composition: the right-hand side is ONE kernel per step and register block -- the product's fold (the walks
// of otmb_op_fold.h, in the product's order) ends in the elementwise line in the same lane, so w is never stored; θ = 1 reads no matrix --
// and each slot's preconditioner (σ + d, Jacobi's diagonal, for the lines u, the multipliers and the pivots) is computed on the slot's first
// visit and kept in op->st for the rest of the call: d, σ, adjoint and the values are fixed inside one call, so nothing can go stale, and
// the arrays have the bits a solve of its own would compute.  The host variant stages X, S and d once and downloads X once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "otmb_op_fold.h"
#include "otmb_solve.h"

struct StLine {  // the elementwise line's constants
    double sigma, theta, c;
};
// b from x, the finished fold w and the row's s and d (null: none; d: the tracer's own column, or the one all share).  One operation per
// statement: the contract's association.
__device__ __forceinline__ double st_line(const StLine &q, double x, double w, const double *__restrict__ d, i64 i, const double *__restrict__ s) {
    double e = w;
    if (d) {
        const double dx = d[i] * x;
        e = dx + w;
    }
    const double ce = q.c * e;
    double a = q.sigma * x;
    if (s) {
        const double st = *s / q.theta;
        a = a + st;
    }
    return a - ce;
}

// ---- θ = 1: b = σ·x + s, no matrix read ----------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void st_stream_kernel(i64 n, double sigma, const double *__restrict__ X, i64 ldx, const double *__restrict__ S, i64 lds,
                                                        double *__restrict__ B, i64 ldb) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        const double a = sigma * X[i + c * ldx];
        B[i + c * ldb] = S ? a + S[i + c * lds] : a;
    }
}

// ---- θ < 1, A: one lane per short row; the long rows are st_long_kernel's.  PC (here and below): tracer c's d lies at d + c·ldd, otherwise all share one --
template <int KB, bool PC = false>
__global__ __launch_bounds__(256) void st_rows_kernel(StLine q, const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ sbase,
                                                      const int *__restrict__ elen, i64 n, const double *__restrict__ d, const double *__restrict__ X, i64 ldx,
                                                      const double *__restrict__ S, i64 lds, double *__restrict__ B, i64 ldb, i64 ldd = 0) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int len = elen[i];
    if (len < 0) return;
    double w[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) w[c] = 0.0;  // (the product's β = 0 start: +0.0)
    op_fold_slice_row(val, col, sbase, i, len, [&](double a, i64 j) {
#pragma unroll
        for (int c = 0; c < KB; ++c) w[c] = w[c] + a * X[j + c * ldx];
    });
#pragma unroll
    for (int c = 0; c < KB; ++c) B[i + c * ldb] = st_line(q, X[i + c * ldx], w[c], d ? d + (PC ? c * ldd : 0) : nullptr, i, S ? S + i + c * lds : nullptr);
}

// one workgroup per long row, lane c folds tracer c (groups of 64 tracers)
template <bool PC = false>
__global__ __launch_bounds__(64) void st_long_kernel(StLine q, const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ lrows,
                                                     const i64 *__restrict__ loff, i64 ell, int k, const double *__restrict__ d, const double *__restrict__ X,
                                                     i64 ldx, const double *__restrict__ S, i64 lds, double *__restrict__ B, i64 ldb, i64 ldd = 0) {
    __shared__ double sv[SP_TCH];
    __shared__ int sc[SP_TCH];
    const int lane = threadIdx.x;
    const i64 i = lrows[blockIdx.x];
    const i64 b0 = ell + loff[i], len = loff[i + 1] - loff[i];
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int c = c0 + lane;
        double w = 0.0;
        op_fold_long_row(val, col, b0, len, sv, sc, lane, c < k, [&](double a, i64 j) { w = w + a * X[j + c * ldx]; });
        if (c < k) B[i + c * ldb] = st_line(q, X[i + c * ldx], w, d ? d + (PC ? c * ldd : 0) : nullptr, i, S ? S + i + c * lds : nullptr);
    }
}

// ---- θ < 1, Aᵀ: one lane per column of A over the CSC copy ------------------------------------------------------------------------------
template <int KB, bool PC = false>
__global__ __launch_bounds__(64) void st_cols_kernel(StLine q, const i64 *__restrict__ cp, const int *__restrict__ rv, const double *__restrict__ nz, i64 n,
                                                     const double *__restrict__ d, const double *__restrict__ X, i64 ldx, const double *__restrict__ S, i64 lds,
                                                     double *__restrict__ B, i64 ldb, i64 ldd = 0) {
    __shared__ double sv[SP_TCH];
    __shared__ int sr[SP_TCH];
    const int lane = threadIdx.x;
    i64 colm;
    double tmp[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) tmp[c] = 0.0;
    const bool has = op_fold_csc_run(cp, rv, nz, n, sv, sr, (i64)blockIdx.x * 64, lane, colm, [&](double a, i64 r) {
#pragma unroll
        for (int c = 0; c < KB; ++c) tmp[c] = tmp[c] + a * X[r + c * ldx];
    });
    if (!has) return;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        const double w = 0.0 + tmp[c];  // (the product's last step, y = +0.0 + tmp·1: a sum of -0.0 becomes +0.0)
        B[colm + c * ldb] = st_line(q, X[colm + c * ldx], w, d ? d + (PC ? c * ldd : 0) : nullptr, colm, S ? S + colm + c * lds : nullptr);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// B (n x k, leading dimension n) = the step's right-hand side from X, with the SELECTED slot's matrix
static void st_rhs(otmb_op *op, int adjoint, i64 k, const StLine &q, const SvD &dk, const double *X, i64 ldx, const double *S, i64 lds, double *B) {
    hipStream_t st = op->ctx->stream;
    const i64 n = op->n, ldd = dk.percol() ? dk.ld : 0;
    const double *d = dk.p;
    if (q.theta == 1.0) {
        op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
            hipLaunchKernelGGL((st_stream_kernel<decltype(kb)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, q.sigma, X + c0 * ldx, ldx,
                               S ? S + c0 * lds : nullptr, lds, B + c0 * n, n);
        });
        return;
    }
    if (!adjoint && op->nlong > 0)
        hipLaunchKernelGGL((ldd ? st_long_kernel<true> : st_long_kernel<false>), dim3((unsigned)op->nlong), dim3(64), 0, st, q, (const double *)op->val.p, (const int *)op->col.p,
                           (const i64 *)op->lrows.p, (const i64 *)op->loff.p, op->ell, (int)k, d, X, ldx, S, lds, B, n, ldd);
    op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
        constexpr int KB = decltype(kb)::value;
        const double *Sc = S ? S + c0 * lds : nullptr, *dc = d ? d + c0 * ldd : nullptr;
        if (adjoint)
            hipLaunchKernelGGL((ldd ? st_cols_kernel<KB, true> : st_cols_kernel<KB, false>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, q, (const i64 *)op->cp.p, (const int *)op->rv.p,
                               (const double *)op->nz.p, n, dc, X + c0 * ldx, ldx, Sc, lds, B + c0 * n, n, ldd);
        else
            hipLaunchKernelGGL((ldd ? st_rows_kernel<KB, true> : st_rows_kernel<KB, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, (const double *)op->val.p, (const int *)op->col.p,
                               (const i64 *)op->sbase.p, (const int *)op->elen.p, n, dc, X + c0 * ldx, ldx, Sc, lds, B + c0 * n, n, ldd);
    });
}

struct StObs {  // what otmb_op_step_obs adds to a step call: q observers W (obs: q x k x nsteps) and the mean's weights and array (null: none)
    i64 q;
    const double *W;
    i64 ldw;
    double *obs;
    const double *tw;
    double *Xbar;
    i64 ldm;
};
static const StObs ST_PLAIN = {0, nullptr, 0, nullptr, nullptr, nullptr, 0};  // no observers, no mean

static int32_t st_check(otmb_op *op, int64_t k, double dt, double theta, int64_t nsteps, int64_t first_slot, const double *S, int64_t lds, double *X,
                        int64_t ldx, double rtol, int64_t maxiter, int32_t precond, const int64_t *steps_done, const int64_t *iters, const double *relres,
                        const int32_t *reason, const StObs &o) {
    const char *more = !steps_done || (nsteps > 0 && (!iters || !relres || !reason))
                           ? "null argument"
                           : sv_step_complaint(op, rtol, maxiter, dt, theta, nsteps >= 0, "nsteps must be >= 0", first_slot);
    if (!more) more = ob_complaint(op, true, nsteps, o.q, o.W, o.ldw, o.obs, o.tw, o.Xbar, o.ldm);
    return sv_check_step(op, precond, k, S, lds, X, ldx, more);
}

// The ONE loop behind otmb_op_step[_dev] (o = ST_PLAIN) and otmb_op_step_obs[_dev]: device pointers, the arguments checked.  After a step
// whose solve left every column converged the observation pass reads X where the solve left it and its fold writes the step's q x k block
// of o.obs; nothing of it waits for the host.
static int32_t st_run(otmb_op *op, int32_t adjoint, int64_t k, const SvD &d, double dt, double theta, int64_t nsteps, int64_t first_slot, const double *S,
                      int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres,
                      int32_t *reason, const StObs &o) {
    int32_t rc;
    *steps_done = 0;
    if (nsteps == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    const i64 n = op->n, nslots = (i64)op->slots.size();
    if (n == 0) {
        *steps_done = nsteps;
        if (o.q > 0) {  // empty sums: +0.0
            HIP_TRY(ctx, hipSetDevice(op->device));
            HIP_TRY(ctx, hipMemsetAsync(o.obs, 0, (size_t)(o.q * k * nsteps) * 8, ctx->stream));
        }
        return sv_report_empty(nsteps * k, iters, relres, reason);
    }
    HIP_TRY(ctx, hipSetDevice(op->device));
    const bool lines = precond == OTMB_PRECOND_LINES, watch = o.q > 0 || o.Xbar;
    const double tdt = theta * dt;
    const StLine q = {1.0 / tdt, theta, (1.0 - theta) / theta};
    // op->st: B, then one preconditioner per slot the call visits (per column where every tracer has its own d)
    const i64 used = std::min(nsteps, nslots), kc = sv_prec_cols(d, k);
    const size_t per = sv_prec_doubles(n, lines, kc);
    if ((double)n * (double)k + (double)used * (double)per >= 1.0e18) return otmb_fail(ctx, OTMB_ERR_ALLOC, "step: the workspace's size overflows");
    if ((rc = otmb_reserve(ctx, op->st, ((size_t)(n * k) + (size_t)used * per) * 8))) return rc;
    if (watch && (rc = ob_reserve(op, k, o.q))) return rc;
    double *B = (double *)op->st.p, *pool = B + n * k;
    std::vector<SvPrec> prec((size_t)nslots, SvPrec{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0});
    i64 taken = 0;
    struct Reselect {  // the caller's selection comes back on every return
        otmb_op *op;
        i64 slot;
        ~Reselect() { (void)otmb_op_select_slot(op, slot); }
    } back{op, op->sel};
    for (i64 t = 0; t < nsteps; ++t) {
        const i64 slot = (first_slot + t) % nslots;
        if ((rc = otmb_op_select_slot(op, slot))) return rc;
        const auto here = [&](int32_t status) {  // the failure's message names the step and the slot
            ctx->err += " (step " + std::to_string(t) + ", slot " + std::to_string(slot) + ")";
            return status;
        };
        SvPrec &p = prec[(size_t)slot];
        if (!p.sh) {  // the slot's first visit
            p = sv_prec_carve(pool + (size_t)(taken++) * per, n, lines, kc, d.percol());
            if ((rc = sv_prec_prepare(op, adjoint, precond, d, q.sigma, p))) return here(rc);
        }
        st_rhs(op, adjoint, k, q, d, X, ldx, S, lds, B);
        HIP_TRY(ctx, hipGetLastError());
        if ((rc = sv_solve(op, adjoint, k, p, B, n, X, ldx, 1, rtol, maxiter, iters + t * k, relres + t * k, reason + t * k, precond))) return here(rc);
        if (watch) {
            ob_pass(op, k, o.q, o.W, o.ldw, X, ldx, o.q > 0 ? o.obs + o.q * k * t : nullptr, o.Xbar, o.ldm, o.tw ? o.tw[t] : 0.0, t == 0);
            HIP_TRY(ctx, hipGetLastError());
        }
        *steps_done = t + 1;
    }
    return OTMB_OK;
}

// The host variant of the loop: X, S, d, W staged once; X, the written rows of obs and Xbar come home once.
static int32_t st_run_host(otmb_op *op, int32_t adjoint, int64_t k, const SvD &d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                           const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                           int64_t *iters, double *relres, int32_t *reason, const StObs &o) {
    int32_t rc;
    *steps_done = 0;
    const i64 n = op->n;
    if (nsteps == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    SvD dd;
    if ((rc = op_reserve_xy(op, n, S ? n : 0, k)) || (rc = op_stage_dk(op, d.p, d.ld, k, dd.p, dd.ld))) return rc;
    double *dx = (double *)op->xs.p, *ds = S ? (double *)op->ys.p : nullptr;
    if (n > 0) {  // staged once, however many steps
        if ((rc = op_upload(ctx, dx, X, ldx, n, k))) return rc;
        if (S && (rc = op_upload(ctx, ds, S, lds, n, k))) return rc;
    }
    StObs od = ST_PLAIN;
    if (o.q > 0 || o.Xbar) {  // op->oh: obs (q x k x nsteps) | W (n x q) | Xbar (n x k), compact
        const i64 nobs = o.q * k * nsteps;
        if ((rc = otmb_reserve(ctx, op->oh, std::max<size_t>((size_t)(nobs + n * o.q + (o.Xbar ? n * k : 0)) * 8, 8)))) return rc;
        double *dobs = (double *)op->oh.p, *dw = dobs + nobs, *dm = dw + n * o.q;
        if (o.q > 0 && n > 0 && (rc = op_upload(ctx, dw, o.W, o.ldw, n, o.q))) return rc;
        od = {o.q, o.q > 0 ? dw : nullptr, n, o.q > 0 ? dobs : nullptr, o.tw, o.Xbar ? dm : nullptr, n};
    }
    rc = st_run(op, adjoint, k, dd, dt, theta, nsteps, first_slot, ds, n, dx, n, rtol, maxiter, precond, steps_done, iters, relres, reason, od);
    // X comes back when it holds an answer: every step done, a step's last iterates, or the state before a slot whose preconditioner is singular
    if (rc != OTMB_OK && rc != OTMB_ERR_NOT_CONVERGED && !(rc == OTMB_ERR_SINGULAR_PRECONDITIONER && *steps_done > 0)) return rc;
    // ... and with it the observations of the completed steps and their mean
    const std::string msg = ctx->err;
    int32_t rcd;
    if (od.q > 0 && *steps_done > 0 && (rcd = op_download(ctx, o.obs, od.q * k * *steps_done, od.obs, od.q * k * *steps_done, 1))) return rcd;
    if (od.Xbar && *steps_done > 0 && n > 0 && (rcd = op_download(ctx, o.Xbar, o.ldm, od.Xbar, n, k))) return rcd;
    ctx->err = msg;
    return op_finish(ctx, rc, X, ldx, dx, n, k);
}

extern "C" {

int32_t otmb_op_step_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond,
                            int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs,
                            const double *tw, double *Xbar, int64_t ldm) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    const StObs o = {q, W, ldw, obs, tw, Xbar, ldm};
    int32_t rc;
    if ((rc = st_check(op, k, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o)) ||
        (rc = sv_check_d(op, "otmb_op_step_dk", D, ldd)))
        return rc;
    return st_run(op, adjoint, k, SvD{D, ldd}, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o);
}

int32_t otmb_op_step_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps, int64_t first_slot,
                        const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                        int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                        double *Xbar, int64_t ldm) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    const StObs o = {q, W, ldw, obs, tw, Xbar, ldm};
    int32_t rc;
    if ((rc = st_check(op, k, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o)) ||
        (rc = sv_check_d(op, "otmb_op_step_dk", D, ldd)))
        return rc;
    return st_run_host(op, adjoint, k, SvD{D, ldd}, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o);
}

// the calls with one d for every tracer: ldd = 0 (otmb_op_step: no observers, no mean either)
int32_t otmb_op_step_obs_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                             const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                             int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                             double *Xbar, int64_t ldm) {
    return otmb_op_step_dk_dev(op, adjoint, k, d, 0, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, q,
                               W, ldw, obs, tw, Xbar, ldm);
}

int32_t otmb_op_step_obs(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                         const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                         int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                         double *Xbar, int64_t ldm) {
    return otmb_op_step_dk(op, adjoint, k, d, 0, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, q, W,
                           ldw, obs, tw, Xbar, ldm);
}

int32_t otmb_op_step_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                         const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                         int64_t *iters, double *relres, int32_t *reason) {
    return otmb_op_step_dk_dev(op, adjoint, k, d, 0, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, 0,
                               nullptr, 0, nullptr, nullptr, nullptr, 0);
}

int32_t otmb_op_step(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                     const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                     int64_t *iters, double *relres, int32_t *reason) {
    return otmb_op_step_dk(op, adjoint, k, d, 0, dt, theta, nsteps, first_slot, S, lds, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, 0,
                           nullptr, 0, nullptr, nullptr, nullptr, 0);
}

}  // extern "C"
