// otmb_step.hip -- θ-steps of ∂x/∂t + (diag(d) + A)·x = s on a resident operator whose value slots hold a cycle of matrices (a year of
// monthly transport matrices): a call advances k tracers through nsteps steps, step t with the slot its schedule gives it,
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
//
// Every export states its call as one record (StCall, otmb_solve.h) and runs the one loop, st_run, behind the one set of checks, st_call.
// What the record's fields switch on, for one step t (the rules themselves are otmb_sched.h's, host C++ that is tested without a device):
//   sched  cyclic (otmb_op_step, _obs, _dk: substeps = 1; otmb_op_step_sched): the step is plain on slot (first_slot + t / substeps) mod
//          nslots.  Listed (otmb_op_step_interp, _season: slot_a, slot_b, weight per step): plain on a (a == b or w == 0.0), plain on b
//          (w == 1.0), or blended.  A plain step selects its slot and makes the slot's preconditioner on the first visit.  A blended step
//          writes (1 - w)·(slot a) + w·(slot b) into op->interp (ip_blend of otmb_interp.hip, one launch), points the values at it (SvValues)
//          and makes its preconditioner afresh into the one block all blended steps share -- the setup and its wait for the device on
//          every such step are the cost of the convention.
//   d      none, one block (n values, or n x k: every tracer its own) or, for otmb_op_step_season, a block per slot: a plain step takes its
//          slot's, a blended step folds the two slots' blocks with the step's weights into op->season (se_fold of otmb_season.hip, one
//          launch) before its preconditioner is made.  A field given once is never folded.
//   src    none, one block or a block per slot, picked and folded like d; with a scale, s·f for the step's factor f of the tracer -- one more
//          multiplication in the lane that holds s, before the line above touches it.  The factors are staged once per call behind the
//          preconditioners; a kernel gets the step's k of them as a device pointer (null: none).
//   obs    observers and a time-weighted mean (otmb_observe.hip's pass after every completed step), or ST_PLAIN.
#include <hip/hip_runtime.h>

#include <cmath>
#include <optional>
#include <string>
#include <vector>

#include "otmb_op_fold.h"
#include "otmb_solve.h"

struct StLine {  // the elementwise line's constants
    double sigma, theta, c;
};
// b from x, the finished fold w and the row's s and d (null: none; d: the tracer's own column, or the one all share); f: the step's scale
// of this tracer's source (null: none), sf = s * f before anything else touches s.  One operation per statement: the contract's association.
__device__ __forceinline__ double st_line(const StLine &q, double x, double w, const double *__restrict__ d, i64 i, const double *__restrict__ s,
                                          const double *__restrict__ f) {
    double e = w;
    if (d) {
        const double dx = d[i] * x;
        e = dx + w;
    }
    const double ce = q.c * e;
    double a = q.sigma * x;
    if (s) {
        double sf = *s;
        if (f) sf = sf * *f;
        const double st = sf / q.theta;
        a = a + st;
    }
    return a - ce;
}

// ---- θ = 1: b = σ·x + s, no matrix read.  f (here and below, the last argument): the step's scales of this block's tracers, f[c] tracer c's
// (null: none)
template <int KB>
__global__ __launch_bounds__(256) void st_stream_kernel(i64 n, double sigma, const double *__restrict__ X, i64 ldx, const double *__restrict__ S, i64 lds,
                                                        double *__restrict__ B, i64 ldb, const double *__restrict__ f = nullptr) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        const double a = sigma * X[i + c * ldx];
        if (S) {
            double sf = S[i + c * lds];
            if (f) sf = sf * f[c];
            B[i + c * ldb] = a + sf;
        } else {
            B[i + c * ldb] = a;
        }
    }
}

// ---- θ < 1, A: one lane per short row; the long rows are st_long_kernel's.  PC (here and below): tracer c's d lies at d + c·ldd, otherwise all share one --
template <int KB, bool PC = false>
__global__ __launch_bounds__(256) void st_rows_kernel(StLine q, const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ sbase,
                                                      const int *__restrict__ elen, i64 n, const double *__restrict__ d, const double *__restrict__ X, i64 ldx,
                                                      const double *__restrict__ S, i64 lds, double *__restrict__ B, i64 ldb, i64 ldd = 0,
                                                      const double *__restrict__ f = nullptr) {
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
    for (int c = 0; c < KB; ++c) B[i + c * ldb] = st_line(q, X[i + c * ldx], w[c], d ? d + (PC ? c * ldd : 0) : nullptr, i, S ? S + i + c * lds : nullptr, f ? f + c : nullptr);
}

// one workgroup per long row, lane c folds tracer c (groups of 64 tracers) and reads its scale f[c]: f is the whole step's, not a block's
template <bool PC = false>
__global__ __launch_bounds__(64) void st_long_kernel(StLine q, const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ lrows,
                                                     const i64 *__restrict__ loff, i64 ell, int k, const double *__restrict__ d, const double *__restrict__ X,
                                                     i64 ldx, const double *__restrict__ S, i64 lds, double *__restrict__ B, i64 ldb, i64 ldd = 0,
                                                     const double *__restrict__ f = nullptr) {
    __shared__ double sv[SP_TCH];
    __shared__ int sc[SP_TCH];
    const int lane = threadIdx.x;
    const i64 i = lrows[blockIdx.x];
    const i64 b0 = ell + loff[i], len = loff[i + 1] - loff[i];
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int c = c0 + lane;
        double w = 0.0;
        op_fold_long_row(val, col, b0, len, sv, sc, lane, c < k, [&](double a, i64 j) { w = w + a * X[j + c * ldx]; });
        if (c < k) B[i + c * ldb] = st_line(q, X[i + c * ldx], w, d ? d + (PC ? c * ldd : 0) : nullptr, i, S ? S + i + c * lds : nullptr, f ? f + c : nullptr);
    }
}

// ---- θ < 1, Aᵀ: one lane per column of A over the CSC copy ------------------------------------------------------------------------------
template <int KB, bool PC = false>
__global__ __launch_bounds__(64) void st_cols_kernel(StLine q, const i64 *__restrict__ cp, const int *__restrict__ rv, const double *__restrict__ nz, i64 n,
                                                     const double *__restrict__ d, const double *__restrict__ X, i64 ldx, const double *__restrict__ S, i64 lds,
                                                     double *__restrict__ B, i64 ldb, i64 ldd = 0, const double *__restrict__ f = nullptr) {
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
        B[colm + c * ldb] = st_line(q, X[colm + c * ldx], w, d ? d + (PC ? c * ldd : 0) : nullptr, colm, S ? S + colm + c * lds : nullptr,
                                    f ? f + c : nullptr);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// B (n x k, leading dimension n) = the step's right-hand side from X, with the SELECTED slot's matrix; f: the step's k scales on the device
// (null: none), of which register block c0 reads f + c0
static void st_rhs(otmb_op *op, int adjoint, i64 k, const StLine &q, const SvD &dk, const double *X, i64 ldx, const double *S, i64 lds, const double *f,
                   double *B) {
    hipStream_t st = op->ctx->stream;
    const i64 n = op->n, ldd = dk.percol() ? dk.ld : 0;
    const double *d = dk.p;
    if (q.theta == 1.0) {
        op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
            hipLaunchKernelGGL((st_stream_kernel<decltype(kb)::value>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, q.sigma, X + c0 * ldx, ldx,
                               S ? S + c0 * lds : nullptr, lds, B + c0 * n, n, S && f ? f + c0 : nullptr);
        });
        return;
    }
    if (!adjoint && op->nlong > 0)
        hipLaunchKernelGGL((ldd ? st_long_kernel<true> : st_long_kernel<false>), dim3((unsigned)op->nlong), dim3(64), 0, st, q, (const double *)op->val.p, (const int *)op->col.p,
                           (const i64 *)op->lrows.p, (const i64 *)op->loff.p, op->ell, (int)k, d, X, ldx, S, lds, B, n, ldd, S ? f : nullptr);
    op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
        constexpr int KB = decltype(kb)::value;
        const double *Sc = S ? S + c0 * lds : nullptr, *dc = d ? d + c0 * ldd : nullptr, *fc = S && f ? f + c0 : nullptr;
        if (adjoint)
            hipLaunchKernelGGL((ldd ? st_cols_kernel<KB, true> : st_cols_kernel<KB, false>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, q, (const i64 *)op->cp.p, (const int *)op->rv.p,
                               (const double *)op->nz.p, n, dc, X + c0 * ldx, ldx, Sc, lds, B + c0 * n, n, ldd, fc);
        else
            hipLaunchKernelGGL((ldd ? st_rows_kernel<KB, true> : st_rows_kernel<KB, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, (const double *)op->val.p, (const int *)op->col.p,
                               (const i64 *)op->sbase.p, (const int *)op->elen.p, n, dc, X + c0 * ldx, ldx, Sc, lds, B + c0 * n, n, ldd, fc);
    });
}

// the call's own checks: the report's arrays, the arguments the step shares with the periodic state and the solver, the observers
static int32_t st_check(otmb_op *op, const StCall &c) {
    const StObs &o = c.obs;
    const char *more = !c.steps_done || (c.nsteps > 0 && (!c.iters || !c.relres || !c.reason))
                           ? "null argument"
                           : sv_step_complaint(op, c.rtol, c.maxiter, c.dt, c.theta, c.nsteps >= 0, "nsteps must be >= 0", c.sched.first_slot);
    if (!more) more = ob_complaint(op, true, c.nsteps, o.q, o.W, o.ldw, o.obs, o.tw, o.Xbar, o.ldm);
    return sv_check_step(op, c.precond, c.k, c.src.nsrc > 0 && c.src.S ? c.src.S[0] : nullptr, c.src.lds, c.X, c.ldx, more);
}

// What the scheduled calls add to the checks of the calls they extend, for the step and the periodic state alike: the schedule's and the
// sources' complaints (otmb_sched.h), then the step's own -- a scale needs a source and finite entries --, then the d blocks' of a season call.
int32_t st_check_sched(otmb_op *op, const StHead &h) {
    const i64 n = op->n, nslots = (i64)op->slots.size();
    const StSrc &src = h.src;
    char text[160];
    const char *more = h.sched.listed ? sv_interp_complaint(n, nslots, h.nsteps, h.sched.mix, src.nsrc, src.S, src.lds, text, h.season)
                                      : sv_sched_complaint(n, nslots, h.sched.substeps, src.nsrc, src.S, src.lds);
    if (!more && src.scale) {
        if (src.nsrc == 0) more = "scale needs a source (nsrc > 0)";
        for (i64 e = 0; !more && e < h.nsteps * h.k; ++e)
            if (!std::isfinite(src.scale[e])) more = "a scale value is not finite";
    }
    if (!more && h.season) more = sv_season_complaint(n, nslots, h.d.nd, h.d.D, h.d.ldd);
    return more ? otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, (std::string(h.call) + ": " + more).c_str()) : OTMB_OK;
}

// The ONE loop behind every step call.  Device pointers (c.d.D, c.src.S: host arrays of them; c.src.scale: host values), the arguments
// checked.  Step t resolves what it runs on -- d, the source, the values and the preconditioner's block, and whether that block is made
// now -- from the schedule (the head of this file says how), and then has one tail: sv_prec_prepare when the block is due, the right-hand
// side, the solve, the observation pass.  After a step whose solve left every column converged the pass reads X where the solve left it
// and its fold writes the step's q x k block of obs; nothing of it waits for the host.
static int32_t st_run(otmb_op *op, const StCall &c) {
    int32_t rc;
    *c.steps_done = 0;
    if (c.nsteps == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    const StObs &o = c.obs;
    const StSrc &src = c.src;
    const i64 n = op->n, nslots = (i64)op->slots.size(), k = c.k, nsteps = c.nsteps;
    if (n == 0) {
        *c.steps_done = nsteps;
        if (o.q > 0) {  // empty sums: +0.0
            HIP_TRY(ctx, hipSetDevice(op->device));
            HIP_TRY(ctx, hipMemsetAsync(o.obs, 0, (size_t)(o.q * k * nsteps) * 8, ctx->stream));
        }
        return sv_report_empty(nsteps * k, c.iters, c.relres, c.reason);
    }
    HIP_TRY(ctx, hipSetDevice(op->device));
    const bool lines = c.precond == OTMB_PRECOND_LINES, watch = o.q > 0 || o.Xbar;
    const double tdt = c.theta * c.dt;
    const StLine q = {1.0 / tdt, c.theta, (1.0 - c.theta) / c.theta};
    // op->st: B, then the schedule's preconditioner blocks (per column where every tracer has its own d), then the scales (nsteps x k)
    const i64 kc = c.d.percol() ? k : 1;
    bool blended;
    const i64 used = c.sched.blocks(nsteps, nslots, blended);
    if (blended) {
        if ((rc = ip_reserve(op))) return rc;
        if ((c.d.nd > 1 || src.nsrc > 1) && (rc = se_reserve(op, (size_t)(n * kc) + (size_t)(n * k)))) return rc;
    }
    const size_t per = sv_prec_doubles(n, lines, kc);
    const double nscale = src.scale ? (double)nsteps * (double)k : 0.0;
    if ((double)n * (double)k + (double)used * (double)per + nscale >= 1.0e18) return otmb_fail(ctx, OTMB_ERR_ALLOC, "step: the workspace's size overflows");
    if ((rc = otmb_reserve(ctx, op->st, ((size_t)(n * k) + (size_t)used * per + (size_t)nscale) * 8))) return rc;
    if (watch && (rc = ob_reserve(op, k, o.q))) return rc;
    double *B = (double *)op->st.p, *pool = B + n * k, *fdev = src.scale ? pool + (size_t)used * per : nullptr;
    if (fdev) {  // staged once per call; the first preconditioner's setup waits for the stream before the call can return
        HIP_TRY(ctx, hipMemcpyAsync(fdev, src.scale, (size_t)(nsteps * k) * 8, hipMemcpyHostToDevice, ctx->stream));
        ctx->uploaded_bytes += 8 * nsteps * k;
    }
    std::vector<SvPrec> prec((size_t)nslots + 1, SvPrec{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0});  // a block per slot; the last: the blended steps'
    i64 taken = 0;
    struct Reselect {  // the caller's selection comes back on every return
        otmb_op *op;
        i64 slot;
        ~Reselect() { (void)otmb_op_select_slot(op, slot); }
    } back{op, op->sel};
    for (i64 t = 0; t < nsteps; ++t) {
        const StStep s = c.sched.at(t, nslots);
        const auto here = [&](int32_t status) {  // the failure's message names the step and the slot(s) the schedule gave it
            ctx->err += c.sched.describe(t, s.slot);
            return status;
        };
        {
            SvD d = c.d.at(s.slot);
            const double *St = src.at(s.slot);
            i64 ldst = src.lds;
            std::optional<SvValues> on;  // a blended step's values, for its preconditioner, its right-hand side and its solve
            if (s.blend) {
                const i64 a = c.sched.mix.a[t], b = c.sched.mix.b[t];
                double wa, wb;
                c.sched.weights(t, wa, wb);
                if ((rc = ip_blend(op, a, b, wa, wb))) return here(rc);
                if (c.d.nd > 1) {  // d of the step: wa·(block a) + wb·(block b), compact in op->season
                    double *Dt = (double *)op->season.p;
                    if ((rc = se_fold(op, {c.d.D[a], c.d.D[b]}, {wa, wb}, n, kc, c.d.ldd, Dt, n))) return here(rc);
                    d = SvD{Dt, c.d.ldd ? n : 0};
                }
                if (src.nsrc > 1) {  // and its source, behind it; the step's scale multiplies the blend (st_line)
                    double *Sm = (double *)op->season.p + n * kc;
                    if ((rc = se_fold(op, {src.S[a], src.S[b]}, {wa, wb}, n, k, src.lds, Sm, n))) return here(rc);
                    St = Sm, ldst = n;
                }
                on.emplace(op, op->interp);
            } else if ((rc = otmb_op_select_slot(op, s.slot))) {
                return rc;
            }
            SvPrec &p = prec[(size_t)(s.blend ? nslots : s.slot)];
            const bool due = s.blend || !p.sh;  // a slot's block is made on its first visit, the blended steps' on every one of them
            if (!p.sh) p = sv_prec_carve(pool + (size_t)(taken++) * per, n, lines, kc, c.d.percol());
            if (due && (rc = sv_prec_prepare(op, c.adjoint, c.precond, d, q.sigma, p))) return here(rc);
            st_rhs(op, c.adjoint, k, q, d, c.X, c.ldx, St, ldst, fdev ? fdev + t * k : nullptr, B);
            HIP_TRY(ctx, hipGetLastError());
            if ((rc = sv_solve(op, c.adjoint, k, p, B, n, c.X, c.ldx, 1, c.rtol, c.maxiter, c.iters + t * k, c.relres + t * k, c.reason + t * k, c.precond))) return here(rc);
        }
        if (watch) {
            ob_pass(op, k, o.q, o.W, o.ldw, c.X, c.ldx, o.q > 0 ? o.obs + o.q * k * t : nullptr, o.Xbar, o.ldm, o.tw ? o.tw[t] : 0.0, t == 0);
            HIP_TRY(ctx, hipGetLastError());
        }
        *c.steps_done = t + 1;
    }
    return OTMB_OK;
}

// The host variant of the loop: X, every source block, d, W staged once; X, the written rows of obs and Xbar come home once.
static int32_t st_run_host(otmb_op *op, const StCall &c) {
    int32_t rc;
    *c.steps_done = 0;
    const i64 n = op->n, k = c.k;
    if (c.nsteps == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    OpStaged g;
    if ((rc = op_stage_call(op, k, c.d, c.src, c.X, c.ldx, g))) return rc;
    const StObs &o = c.obs;
    StCall dev = c;
    dev.d = g.d, dev.src = g.src, dev.X = g.X, dev.ldx = n, dev.obs = ST_PLAIN;
    if (o.q > 0 || o.Xbar) {  // op->oh: obs (q x k x nsteps) | W (n x q) | Xbar (n x k), compact
        const i64 nobs = o.q * k * c.nsteps;
        if ((rc = otmb_reserve(ctx, op->oh, std::max<size_t>((size_t)(nobs + n * o.q + (o.Xbar ? n * k : 0)) * 8, 8)))) return rc;
        double *dobs = (double *)op->oh.p, *dw = dobs + nobs, *dm = dw + n * o.q;
        if (o.q > 0 && n > 0 && (rc = op_upload(ctx, dw, o.W, o.ldw, n, o.q))) return rc;
        dev.obs = {o.q, o.q > 0 ? dw : nullptr, n, o.q > 0 ? dobs : nullptr, o.tw, o.Xbar ? dm : nullptr, n};
    }
    const StObs &od = dev.obs;
    rc = st_run(op, dev);
    // X comes back when it holds an answer: every step done, a step's last iterates, or the state before a slot whose preconditioner is singular
    if (rc != OTMB_OK && rc != OTMB_ERR_NOT_CONVERGED && !(rc == OTMB_ERR_SINGULAR_PRECONDITIONER && *c.steps_done > 0)) return rc;
    // ... and with it the observations of the completed steps and their mean
    const std::string msg = ctx->err;
    const i64 done = *c.steps_done;
    int32_t rcd;
    if (od.q > 0 && done > 0 && (rcd = op_download(ctx, o.obs, od.q * k * done, od.obs, od.q * k * done, 1))) return rcd;
    if (od.Xbar && done > 0 && n > 0 && (rcd = op_download(ctx, o.Xbar, o.ldm, od.Xbar, n, k))) return rcd;
    ctx->err = msg;
    return op_finish(ctx, rc, c.X, c.ldx, g.X, n, k);
}

// One body for every step call (DEV: device pointers): the call's own checks, those of D and ldd under the export's name (a season call's d
// is a list, which has its own), then the schedule's; then the loop.
template <bool DEV>
int32_t st_call(otmb_op *op, const StCall &c) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = st_check(op, c)) || (!c.season && (rc = sv_check_d(op, c.call, c.d.nd ? c.d.D[0] : nullptr, c.d.ldd))) ||
        (c.sched_checks && (rc = st_check_sched(op, c))))
        return rc;
    return DEV ? st_run(op, c) : st_run_host(op, c);
}
template int32_t st_call<true>(otmb_op *, const StCall &);  // (otmb_periodic.hip's cycle)

extern "C" {

int32_t otmb_op_step_sched_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                               int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X,
                               int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres,
                               int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    const double *const one[1] = {D};
    return st_call<true>(op, {{"otmb_op_step_sched", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, StSched::cyclic(first_slot, substeps),
                               StSrc{nsrc, S, lds, scale}, X, ldx, rtol, maxiter, precond},
                              steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

int32_t otmb_op_step_sched(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                           int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X, int64_t ldx,
                           double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q,
                           const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    const double *const one[1] = {D};
    return st_call<false>(op, {{"otmb_op_step_sched", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, StSched::cyclic(first_slot, substeps),
                                StSrc{nsrc, S, lds, scale}, X, ldx, rtol, maxiter, precond},
                               steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

// the listed schedule: slot_a, slot_b, weight (nsteps host values each) in place of first_slot, substeps
int32_t otmb_op_step_interp_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                                const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                                double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar,
                                int64_t ldm) {
    const double *const one[1] = {D};
    return st_call<true>(op, {{"otmb_op_step_interp", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, StSched::list(slot_a, slot_b, weight),
                               StSrc{nsrc, S, lds, scale}, X, ldx, rtol, maxiter, precond},
                              steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

int32_t otmb_op_step_interp(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                            const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                            double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    const double *const one[1] = {D};
    return st_call<false>(op, {{"otmb_op_step_interp", true, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, StSched::list(slot_a, slot_b, weight),
                                StSrc{nsrc, S, lds, scale}, X, ldx, rtol, maxiter, precond},
                               steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

// the listed schedule with d and the source per slot: nd, D (nd pointers), ldd in place of D, ldd; nsrc may be the number of slots
int32_t otmb_op_step_season_dev(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta,
                                int64_t nsteps, const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S,
                                int64_t lds, const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                                int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                                double *Xbar, int64_t ldm) {
    return st_call<true>(op, {{"otmb_op_step_season", true, true, adjoint, k, StD{nd, D, ldd}, dt, theta, nsteps, StSched::list(slot_a, slot_b, weight),
                               StSrc{nsrc, S, lds, scale}, X, ldx, rtol, maxiter, precond},
                              steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

int32_t otmb_op_step_season(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                            const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                            double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    return st_call<false>(op, {{"otmb_op_step_season", true, true, adjoint, k, StD{nd, D, ldd}, dt, theta, nsteps, StSched::list(slot_a, slot_b, weight),
                                StSrc{nsrc, S, lds, scale}, X, ldx, rtol, maxiter, precond},
                               steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

// the calls from before the schedule: substeps = 1, the one source or none, no scale, none of the schedule's checks
int32_t otmb_op_step_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond,
                            int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs,
                            const double *tw, double *Xbar, int64_t ldm) {
    const double *const one[1] = {D}, *const src[1] = {S};
    return st_call<true>(op, {{"otmb_op_step_dk", false, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, StSched::cyclic(first_slot, 1),
                               StSrc{S ? 1 : 0, src, lds, nullptr}, X, ldx, rtol, maxiter, precond},
                              steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
}

int32_t otmb_op_step_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps, int64_t first_slot,
                        const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                        int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                        double *Xbar, int64_t ldm) {
    const double *const one[1] = {D}, *const src[1] = {S};
    return st_call<false>(op, {{"otmb_op_step_dk", false, false, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, StSched::cyclic(first_slot, 1),
                                StSrc{S ? 1 : 0, src, lds, nullptr}, X, ldx, rtol, maxiter, precond},
                               steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}});
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
