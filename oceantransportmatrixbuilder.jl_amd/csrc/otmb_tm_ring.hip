// otmb_tm_ring.hip -- the asynchronous protocol's state ring: every otmb_transportmatrix_dev / otmb_step_dev call (otmb_transportmatrix.hip)
// leaves its flags and totals in a ring slot; here they are fetched, folded into per-step verdicts and handed out.
#include "otmb_tm.h"

// The state blocks of the asynchronous steps, device ring -> pinned host mirror, once the stream has drained.
int32_t otmb_tm_fetch_ring(otmb_ctx *ctx) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_ring, ctx->ring.p, (size_t)OTMB_RING * OTMB_TM_STATE_BYTES, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OTMB_OK;
}

// Fold the completed pending steps [tm_first, tm_next) of the asynchronous protocol: every step's verdict and nnz go to
// ctx->tm_hist (otmb_transportmatrix_result_step), the first failing step into the sticky (status, step) pair, and a step
// whose T had exact cancellations is compacted in ITS OWN output arrays (every otmb_transportmatrix_dev call recorded
// them) -- unless a later pending step was given the same arrays, which then hold that later step's matrix.
// The stream is idle on entry (the steps' state blocks have landed in h_ring).
int32_t otmb_tm_fold_pending(otmb_ctx *ctx) {
    int32_t ret = OTMB_OK;
    for (i64 s = ctx->tm_first; s < ctx->tm_next; ++s) {
        const int *f = otmb_ring_tm(ctx->h_ring, s);
        const i64 *tot = (const i64 *)(f + OTMB_NFLAGS);
        otmb_ctx::TmStepResult r;
        const size_t q = (size_t)(s - ctx->tm_first);
        const otmb_ctx::TmStepRec *rec = q < ctx->tm_rec.size() ? &ctx->tm_rec[q] : nullptr;
        r.status = otmb_tm_check_flags(ctx, f, rec ? rec->ignore_ops : 0);  // sets ctx->err
        for (int m = 0; m < 5; ++m) r.nnz[m] = tot[m];
        if (rec) otmb_tm_kept_on_fold(ctx, *rec, f, tot, r);
        if (r.status && !ctx->tm_sticky) { ctx->tm_sticky = r.status; ctx->tm_sticky_step = s; ctx->tm_sticky_msg = ctx->err; }
        if (!r.status && f[FLAG_T_CANCEL] && rec) {
            bool superseded = false;
            for (size_t l = q + 1; l < ctx->tm_rec.size(); ++l)
                superseded |= ctx->tm_rec[l].colptrT == rec->colptrT || ctx->tm_rec[l].rowvalT == rec->rowvalT || ctx->tm_rec[l].nzvalT == rec->nzvalT;
            if (!superseded && !ret) {
                i64 actual = r.nnz[0];
                ret = otmb_tm_t_fixup(ctx, rec->n_wet, rec->nnz_base0, r.nnz[0], (i64 *)rec->colptrT, (i64 *)rec->rowvalT, (double *)rec->nzvalT, &actual);
                r.nnz[0] = actual;
                otmb_tm_kept_after_fixup(ctx, rec->colptrT, rec->rowvalT);
            }
        }
        ctx->tm_hist.push_back(r);
    }
    if (ctx->tm_sticky) ctx->err = ctx->tm_sticky_msg;
    ctx->tm_rec.clear();
    ctx->tm_first = ctx->tm_next;
    return ret;
}

extern "C" {

int32_t otmb_transportmatrix_failed_step(otmb_ctx *ctx, int64_t *step) {
    if (!ctx || !step) return OTMB_ERR_INVALID_ARG;
    *step = ctx->tm_failed_step;
    return OTMB_OK;
}

int32_t otmb_transportmatrix_result(otmb_ctx *ctx, int64_t nnz[5]) {
    if (!ctx || !nnz) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (!ctx->plan || !ctx->plan->onepass_pending) return otmb_fail(ctx, OTMB_ERR_NO_PLAN);
    int32_t frc;
    if ((frc = otmb_tm_fetch_ring(ctx))) return frc;
    ctx->plan->onepass_pending = false;
    // every step enqueued since the previous result: the FIRST one that failed is reported (the reference would have
    // thrown there, src/matrixbuilding.jl:39,61,90,114,233), with its position in the error text; every step that did
    // not fail has its own nnz (and its T compacted if entries cancelled): otmb_transportmatrix_result_step
    const i64 n_steps = ctx->tm_next;
    frc = otmb_tm_fold_pending(ctx);
    const int32_t st = ctx->tm_sticky;
    ctx->tm_failed_step = ctx->tm_sticky_step;
    ctx->tm_sticky = 0; ctx->tm_sticky_step = -1;
    ctx->tm_first = ctx->tm_next = 0;
    ctx->tm_hist_final = true;
    if (st) {
        if (n_steps > 1) {
            char where[96];
            snprintf(where, sizeof where, " (asynchronous step %lld of %lld)", (long long)ctx->tm_failed_step + 1, (long long)n_steps);
            ctx->err += where;
        }
        return st;
    }
    if (frc) return frc;
    if (ctx->tm_hist.empty()) return otmb_fail(ctx, OTMB_ERR_NO_PLAN);
    for (int m = 0; m < 5; ++m) nnz[m] = ctx->plan->nnz[m] = ctx->tm_hist.back().nnz[m];
    return OTMB_OK;
}

int32_t otmb_transportmatrix_result_step(otmb_ctx *ctx, int64_t step, int64_t nnz[5]) {
    if (!ctx || !nnz) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (!ctx->tm_hist_final || step < 0 || (size_t)step >= ctx->tm_hist.size()) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "no such asynchronous step");
    for (int m = 0; m < 5; ++m) nnz[m] = ctx->tm_hist[(size_t)step].nnz[m];
    return ctx->tm_hist[(size_t)step].status;
}

}  // extern "C"
