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
//
// otmb_op_step_sched[_dev] is the same loop with a schedule (StSrc): step t takes slot (first_slot + t / substeps) mod nslots, the source
// block of that slot (or the one block, or none) and, with a scale, s·f for the step's factor f of the tracer -- one more multiplication in
// the lane that holds s, before the line above touches it.  The factors are staged once per call behind the preconditioners; a kernel gets
// the step's k of them as a device pointer (null: none).  Every other step call is this one with substeps = 1, at most one block, no scale.
//
// otmb_op_step_interp[_dev] is the same loop again with an interpolated schedule (StMix: slot_a, slot_b, weight per step): a step whose two
// slots are one, or whose weight is 0 or 1, is a step of the loop as it stands; a blended step writes (1 - w)·(slot a) + w·(slot b) into
// op->interp (ip_blend of otmb_interp.hip, one launch), points the values at it (SvValues) and makes its preconditioner afresh into one
// block that all blended steps share -- the setup and its wait for the device on every such step are the cost of the convention.
//
// otmb_op_step_season[_dev] is that loop with d, and the source, per slot as well (StD, StSrc with nsrc = nslots): a plain step takes its
// slot's blocks, a blended step folds the two slots' blocks with the step's own weights into op->season (se_fold of otmb_season.hip, one
// launch per field) before its preconditioner is made.  A field given once is never folded.
#include <hip/hip_runtime.h>

#include <cmath>
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

// The schedule of otmb_op_step_sched: step t runs with slot (first_slot + t / substeps) mod nslots and the source block at(slot) of nsrc
// (0: none; 1: block 0 on every step; nslots: the slot's), each n x k with leading dimension lds; scale: nsteps·k HOST values or null.
struct StSrc {
    i64 substeps, nsrc;
    const double *const *S;
    i64 lds;
    const double *scale;
    const double *at(i64 slot) const { return nsrc == 0 ? nullptr : S[nsrc == 1 ? 0 : slot]; }
};

// What the interpolated schedule makes of step t: its slot when it is plain (a == b or w == 0.0: a; w == 1.0: b), or a blend of a and b.
struct StStep {
    i64 slot;
    bool blend;
};
static StStep st_step_of(const StMix &mix, i64 t) {
    const i64 a = mix.a[t], b = mix.b[t];
    const double w = mix.w[t];
    if (a == b || w == 0.0) return {a, false};
    if (w == 1.0) return {b, false};
    return {a, true};
}

static int32_t st_check(otmb_op *op, int64_t k, double dt, double theta, int64_t nsteps, int64_t first_slot, const StSrc &src, double *X, int64_t ldx, double rtol,
                        int64_t maxiter, int32_t precond, const int64_t *steps_done, const int64_t *iters, const double *relres, const int32_t *reason,
                        const StObs &o) {
    const char *more = !steps_done || (nsteps > 0 && (!iters || !relres || !reason))
                           ? "null argument"
                           : sv_step_complaint(op, rtol, maxiter, dt, theta, nsteps >= 0, "nsteps must be >= 0", first_slot);
    if (!more) more = ob_complaint(op, true, nsteps, o.q, o.W, o.ldw, o.obs, o.tw, o.Xbar, o.ldm);
    return sv_check_step(op, precond, k, src.nsrc > 0 && src.S ? src.S[0] : nullptr, src.lds, X, ldx, more);
}

// What the scheduled calls add to the checks of the calls they extend (sv_sched_complaint, shared with otmb_op_periodic_sched), and the
// step's own: a scale needs a source and finite entries.
const char *sv_sched_complaint(const otmb_op *op, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds) {
    if (substeps < 1) return "substeps must be >= 1";
    if (nsrc != 0 && nsrc != 1 && nsrc != (i64)op->slots.size()) return "nsrc must be 0, 1 or the number of slots";
    if (nsrc > 0) {
        if (!S) return "S is null with nsrc > 0";
        for (i64 j = 0; j < nsrc; ++j)
            if (!S[j]) return "a source block is null";
        if (lds < op->n) return "lds is smaller than the rows of S";
    }
    return nullptr;
}
// What otmb_op_step_interp and otmb_op_periodic_interp add (shared like the above): nsrc is 0 or 1, then the schedule's complaints about the
// source, then the three arrays -- none null, every slot one of the operator's, every weight finite and in [0, 1].
const char *sv_interp_complaint(const otmb_op *op, int64_t count, const StMix &mix, int64_t nsrc, const double *const *S, int64_t lds, char *text,
                                bool per_slot) {
    if (!per_slot && nsrc != 0 && nsrc != 1) return "nsrc must be 0 or 1 (a source per slot is not built with interpolation)";
    if (const char *more = sv_sched_complaint(op, 1, nsrc, S, lds)) return more;
    if (count > 0 && (!mix.a || !mix.b || !mix.w)) return "slot_a, slot_b or weight is null";
    const i64 nslots = (i64)op->slots.size();
    for (i64 t = 0; t < count; ++t) {
        for (const int64_t s : {mix.a[t], mix.b[t]})
            if (s < 0 || s >= nslots) {
                snprintf(text, 160, "step %lld: slot %lld is outside 0..%lld (otmb_op_set_slots)", (long long)t, (long long)s, (long long)nslots - 1);
                return text;
            }
        if (!std::isfinite(mix.w[t]) || mix.w[t] < 0.0 || mix.w[t] > 1.0) {
            snprintf(text, 160, "step %lld: the weight %g is not finite or outside [0, 1]", (long long)t, mix.w[t]);
            return text;
        }
    }
    return nullptr;
}
// What otmb_op_step_season and otmb_op_periodic_season add (shared like the above): the list of d blocks.
const char *sv_season_complaint(const otmb_op *op, int64_t nd, const double *const *D, int64_t ldd) {
    if (nd != 0 && nd != 1 && nd != (i64)op->slots.size()) return "nd must be 0, 1 or the number of slots";
    if (nd > 0) {
        if (!D) return "D is null with nd > 0";
        for (i64 j = 0; j < nd; ++j)
            if (!D[j]) return "a d block is null";
        if (ldd != 0 && ldd < op->n) return "ldd must be 0 (the n values of a block serve every column) or >= n";
    }
    return nullptr;
}
// (call: the export the message names; mix: the interpolated schedule, null without one; dl: the season call's list of d blocks, null
// without one -- a source per slot is then in order under interpolation)
static int32_t st_check_sched(otmb_op *op, const char *call, int64_t k, int64_t nsteps, const StSrc &src, const StMix *mix, const StD *dl = nullptr) {
    char text[160];
    const char *more = mix ? sv_interp_complaint(op, nsteps, *mix, src.nsrc, src.S, src.lds, text, dl != nullptr) : sv_sched_complaint(op, src.substeps, src.nsrc, src.S, src.lds);
    if (!more && src.scale) {
        if (src.nsrc == 0) more = "scale needs a source (nsrc > 0)";
        for (i64 e = 0; !more && e < nsteps * k; ++e)
            if (!std::isfinite(src.scale[e])) more = "a scale value is not finite";
    }
    if (!more && dl) more = sv_season_complaint(op, dl->nd, dl->D, dl->ldd);
    return more ? otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, (std::string(call) + ": " + more).c_str()) : OTMB_OK;
}

// The ONE loop behind every step call: otmb_op_step_sched[_dev], and otmb_op_step_dk[_dev] with what is layered on it (substeps = 1, at
// most one source, no scale; o = ST_PLAIN: no record).  Device pointers (src.S: a host array of them; src.scale: host values), the arguments
// checked.  After a step whose solve left every column converged the observation pass reads X where the solve left it and its fold writes
// the step's q x k block of o.obs; nothing of it waits for the host.
//
// mix (null: none) is the interpolated schedule of otmb_op_step_interp: step t is plain on mix->a[t] (a == b or w == 0.0), plain on mix->b[t]
// (w == 1.0) or blended.  A blended step points the values at op->interp (SvValues) for its blend, its preconditioner -- made afresh into
// the ONE block all blended steps share, behind the plain slots' --, its right-hand side and its solve.  Without mix nothing here differs
// from the loop as it was: the same launches in the same order.
//
// dl is d as a list of blocks: at most one for every call but otmb_op_step_season, whose plain steps take their slot's block -- d is then a
// function of the slot, so a slot's kept preconditioner stays exact -- and whose blended steps fold the two slots' blocks of d, and of the
// source when it is per slot, into op->season (se_fold of otmb_season.hip, one launch each) before the preconditioner is made.  With one
// block each nothing is folded and nothing is reserved.
static int32_t st_run(otmb_op *op, int32_t adjoint, int64_t k, const StD &dl, double dt, double theta, int64_t nsteps, int64_t first_slot, const StSrc &src,
                      double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason,
                      const StObs &o, const StMix *mix = nullptr) {
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
    // op->st: B, then one preconditioner per slot the call visits (per column where every tracer has its own d), then the scales (nsteps x k)
    i64 used = std::min((nsteps - 1) / src.substeps + 1, nslots);
    const i64 kc = dl.percol() ? k : 1;
    if (mix) {  // the plain slots the schedule visits, and one block for every blended step together
        std::vector<char> seen((size_t)nslots, 0);
        bool blended = false;
        used = 0;
        for (i64 t = 0; t < nsteps; ++t) {
            const StStep s = st_step_of(*mix, t);
            if (s.blend)
                blended = true;
            else if (!seen[(size_t)s.slot]++)
                used += 1;
        }
        if (blended) {
            used += 1;
            if ((rc = ip_reserve(op))) return rc;
            if ((dl.nd > 1 || src.nsrc > 1) && (rc = se_reserve(op, (size_t)(n * kc) + (size_t)(n * k)))) return rc;
        }
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
    std::vector<SvPrec> prec((size_t)nslots, SvPrec{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0});
    i64 taken = 0;
    struct Reselect {  // the caller's selection comes back on every return
        otmb_op *op;
        i64 slot;
        ~Reselect() { (void)otmb_op_select_slot(op, slot); }
    } back{op, op->sel};
    SvPrec shared{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};  // the blended steps' block, carved on the first of them
    for (i64 t = 0; t < nsteps; ++t) {
        const StStep s = mix ? st_step_of(*mix, t) : StStep{(first_slot + t / src.substeps) % nslots, false};
        const i64 slot = s.slot;
        const auto here = [&](int32_t status) {  // the failure's message names the step and the slot(s) the schedule gave it
            if (mix) {
                char w[40];
                snprintf(w, sizeof w, "%.17g", mix->w[t]);
                ctx->err += " (step " + std::to_string(t) + ", slots " + std::to_string(mix->a[t]) + " and " + std::to_string(mix->b[t]) + ", weight " + w + ")";
            } else {
                ctx->err += " (step " + std::to_string(t) + ", slot " + std::to_string(slot) + ")";
            }
            return status;
        };
        if (s.blend) {
            const double w = mix->w[t];
            const double wa = 1.0 - w;
            if ((rc = ip_blend(op, mix->a[t], mix->b[t], wa, w))) return here(rc);
            SvD d = dl.at(slot);
            const double *St = src.at(slot);
            i64 ldst = src.lds;
            if (dl.nd > 1) {  // d of the step: wa·(block a) + w·(block b), compact in op->season
                double *Dt = (double *)op->season.p;
                if ((rc = se_fold(op, {dl.D[mix->a[t]], dl.D[mix->b[t]]}, {wa, w}, n, kc, dl.ldd, Dt, n))) return here(rc);
                d = SvD{Dt, dl.ldd ? n : 0};
            }
            if (src.nsrc > 1) {  // and its source, behind it; the step's scale multiplies the blend (st_line)
                double *Sm = (double *)op->season.p + n * kc;
                if ((rc = se_fold(op, {src.S[mix->a[t]], src.S[mix->b[t]]}, {wa, w}, n, k, src.lds, Sm, n))) return here(rc);
                St = Sm, ldst = n;
            }
            SvValues on(op, op->interp);
            if (!shared.sh) shared = sv_prec_carve(pool + (size_t)(taken++) * per, n, lines, kc, dl.percol());
            if ((rc = sv_prec_prepare(op, adjoint, precond, d, q.sigma, shared))) return here(rc);
            st_rhs(op, adjoint, k, q, d, X, ldx, St, ldst, fdev ? fdev + t * k : nullptr, B);
            HIP_TRY(ctx, hipGetLastError());
            if ((rc = sv_solve(op, adjoint, k, shared, B, n, X, ldx, 1, rtol, maxiter, iters + t * k, relres + t * k, reason + t * k, precond))) return here(rc);
        } else {
            if ((rc = otmb_op_select_slot(op, slot))) return rc;
            const SvD d = dl.at(slot);
            SvPrec &p = prec[(size_t)slot];
            if (!p.sh) {  // the slot's first visit
                p = sv_prec_carve(pool + (size_t)(taken++) * per, n, lines, kc, dl.percol());
                if ((rc = sv_prec_prepare(op, adjoint, precond, d, q.sigma, p))) return here(rc);
            }
            st_rhs(op, adjoint, k, q, d, X, ldx, src.at(slot), src.lds, fdev ? fdev + t * k : nullptr, B);
            HIP_TRY(ctx, hipGetLastError());
            if ((rc = sv_solve(op, adjoint, k, p, B, n, X, ldx, 1, rtol, maxiter, iters + t * k, relres + t * k, reason + t * k, precond))) return here(rc);
        }
        if (watch) {
            ob_pass(op, k, o.q, o.W, o.ldw, X, ldx, o.q > 0 ? o.obs + o.q * k * t : nullptr, o.Xbar, o.ldm, o.tw ? o.tw[t] : 0.0, t == 0);
            HIP_TRY(ctx, hipGetLastError());
        }
        *steps_done = t + 1;
    }
    return OTMB_OK;
}

// The host variant of the loop: X, every source block, d, W staged once; X, the written rows of obs and Xbar come home once.
static int32_t st_run_host(otmb_op *op, int32_t adjoint, int64_t k, const StD &dl, double dt, double theta, int64_t nsteps, int64_t first_slot,
                           const StSrc &src, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                           double *relres, int32_t *reason, const StObs &o, const StMix *mix = nullptr) {
    int32_t rc;
    *steps_done = 0;
    const i64 n = op->n;
    if (nsteps == 0) return OTMB_OK;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    std::vector<const double *> dd;
    i64 lddev = 0;
    if ((rc = op_reserve_xy(op, n, src.nsrc * n, k)) || (rc = op_stage_dl(op, dl.nd, dl.D, dl.ldd, k, dd, lddev))) return rc;
    double *dx = (double *)op->xs.p;
    std::vector<const double *> ds((size_t)src.nsrc);  // block j compact behind block j - 1
    for (i64 j = 0; j < src.nsrc; ++j) ds[(size_t)j] = (const double *)op->ys.p + j * n * k;
    if (n > 0) {  // staged once, however many steps
        if ((rc = op_upload(ctx, dx, X, ldx, n, k))) return rc;
        for (i64 j = 0; j < src.nsrc; ++j)
            if ((rc = op_upload(ctx, (double *)op->ys.p + j * n * k, src.S[j], src.lds, n, k))) return rc;
    }
    StObs od = ST_PLAIN;
    if (o.q > 0 || o.Xbar) {  // op->oh: obs (q x k x nsteps) | W (n x q) | Xbar (n x k), compact
        const i64 nobs = o.q * k * nsteps;
        if ((rc = otmb_reserve(ctx, op->oh, std::max<size_t>((size_t)(nobs + n * o.q + (o.Xbar ? n * k : 0)) * 8, 8)))) return rc;
        double *dobs = (double *)op->oh.p, *dw = dobs + nobs, *dm = dw + n * o.q;
        if (o.q > 0 && n > 0 && (rc = op_upload(ctx, dw, o.W, o.ldw, n, o.q))) return rc;
        od = {o.q, o.q > 0 ? dw : nullptr, n, o.q > 0 ? dobs : nullptr, o.tw, o.Xbar ? dm : nullptr, n};
    }
    const StSrc sd = {src.substeps, src.nsrc, ds.data(), n, src.scale};
    rc = st_run(op, adjoint, k, StD{dd[0] ? dl.nd : 0, dd.data(), lddev}, dt, theta, nsteps, first_slot, sd, dx, n, rtol, maxiter, precond, steps_done, iters, relres, reason, od, mix);
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

// one body for the two variants of a call (DEV: device pointers); call: the export named by the refusals of D / ldd; sched: the scheduled
// call's own checks, after those of the call it extends, under the name `sched` (null: none); mix: the interpolated schedule (null: none)
template <bool DEV>
static int32_t st_call(otmb_op *op, const char *call, const char *sched, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta,
                       int64_t nsteps, int64_t first_slot, const StSrc &src, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond,
                       int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, const StObs &o, const StMix *mix = nullptr) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = st_check(op, k, dt, theta, nsteps, first_slot, src, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o)) ||
        (rc = sv_check_d(op, call, D, ldd)) || (sched && (rc = st_check_sched(op, sched, k, nsteps, src, mix))))
        return rc;
    const double *const one[1] = {D};
    return (DEV ? st_run : st_run_host)(op, adjoint, k, StD{D ? 1 : 0, one, ldd}, dt, theta, nsteps, first_slot, src, X, ldx, rtol, maxiter, precond, steps_done,
                                        iters, relres, reason, o, mix);
}
// the season calls: d as a list of blocks (dl), the interpolated schedule, a source per slot in order; their own checks come last
template <bool DEV>
static int32_t st_call_season(otmb_op *op, int32_t adjoint, int64_t k, const StD &dl, double dt, double theta, int64_t nsteps, const StMix &mix, const StSrc &src,
                              double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres,
                              int32_t *reason, const StObs &o) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = st_check(op, k, dt, theta, nsteps, 0, src, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o)) ||
        (rc = st_check_sched(op, "otmb_op_step_season", k, nsteps, src, &mix, &dl)))
        return rc;
    return (DEV ? st_run : st_run_host)(op, adjoint, k, dl, dt, theta, nsteps, 0, src, X, ldx, rtol, maxiter, precond, steps_done, iters, relres, reason, o, &mix);
}

extern "C" {

int32_t otmb_op_step_sched_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                               int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X,
                               int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres,
                               int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    return st_call<true>(op, "otmb_op_step_sched", "otmb_op_step_sched", adjoint, k, D, ldd, dt, theta, nsteps, first_slot, StSrc{substeps, nsrc, S, lds, scale}, X, ldx, rtol,
                         maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm});
}

int32_t otmb_op_step_sched(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                           int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X, int64_t ldx,
                           double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q,
                           const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    return st_call<false>(op, "otmb_op_step_sched", "otmb_op_step_sched", adjoint, k, D, ldd, dt, theta, nsteps, first_slot, StSrc{substeps, nsrc, S, lds, scale}, X, ldx, rtol,
                          maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm});
}

// the interpolated schedule: slot_a, slot_b, weight (nsteps host values each) in place of first_slot, substeps
int32_t otmb_op_step_interp_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                                const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                                double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar,
                                int64_t ldm) {
    const StMix mix = {slot_a, slot_b, weight};
    return st_call<true>(op, "otmb_op_step_interp", "otmb_op_step_interp", adjoint, k, D, ldd, dt, theta, nsteps, 0, StSrc{1, nsrc, S, lds, scale}, X, ldx, rtol,
                         maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}, &mix);
}

int32_t otmb_op_step_interp(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                            const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                            double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    const StMix mix = {slot_a, slot_b, weight};
    return st_call<false>(op, "otmb_op_step_interp", "otmb_op_step_interp", adjoint, k, D, ldd, dt, theta, nsteps, 0, StSrc{1, nsrc, S, lds, scale}, X, ldx, rtol,
                          maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm}, &mix);
}

// the interpolated schedule with d and the source per slot: nd, D (nd pointers), ldd in place of D, ldd; nsrc may be the number of slots
int32_t otmb_op_step_season_dev(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta,
                                int64_t nsteps, const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S,
                                int64_t lds, const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                                int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                                double *Xbar, int64_t ldm) {
    return st_call_season<true>(op, adjoint, k, StD{nd, D, ldd}, dt, theta, nsteps, StMix{slot_a, slot_b, weight}, StSrc{1, nsrc, S, lds, scale}, X, ldx, rtol,
                                maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm});
}

int32_t otmb_op_step_season(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                            const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                            double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm) {
    return st_call_season<false>(op, adjoint, k, StD{nd, D, ldd}, dt, theta, nsteps, StMix{slot_a, slot_b, weight}, StSrc{1, nsrc, S, lds, scale}, X, ldx, rtol,
                                 maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm});
}

// the calls from before the schedule: substeps = 1, the one source or none, no scale
int32_t otmb_op_step_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond,
                            int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs,
                            const double *tw, double *Xbar, int64_t ldm) {
    const double *const one[1] = {S};
    return st_call<true>(op, "otmb_op_step_dk", nullptr, adjoint, k, D, ldd, dt, theta, nsteps, first_slot, StSrc{1, S ? 1 : 0, one, lds, nullptr}, X, ldx, rtol,
                         maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm});
}

int32_t otmb_op_step_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps, int64_t first_slot,
                        const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                        int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                        double *Xbar, int64_t ldm) {
    const double *const one[1] = {S};
    return st_call<false>(op, "otmb_op_step_dk", nullptr, adjoint, k, D, ldd, dt, theta, nsteps, first_slot, StSrc{1, S ? 1 : 0, one, lds, nullptr}, X, ldx, rtol,
                          maxiter, precond, steps_done, iters, relres, reason, StObs{q, W, ldw, obs, tw, Xbar, ldm});
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
