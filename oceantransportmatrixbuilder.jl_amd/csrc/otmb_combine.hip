// otmb_combine.hip -- Σ_s w_s·(slot s) into a slot of a resident operator, on the device: otmb_op_combine_slots[_dev], and cb_combine, which
// the periodic state's cycle-mean preconditioner (otmb_periodic.hip) calls on the operator's private value set.  include/otmb.h states the
// contract; tests/periodic_pc_ref.py restates it (combine_ref).
//
// Per stored entry: the slots with w_s != 0 in ascending s; acc = w_s·v_s for the first of them, acc = acc + w_s·v_s for the rest, one
// operation per statement, no FMA (-ffp-contract=off); no such slot: +0.0.  The host drops the zero weights, so the kernel's list holds the
// terms only.  Both value arrays of the destination are written -- nzval of the CSC copy and the row layout's values, its padding included
// (padding is never read by a product, so what the arithmetic makes of it does not matter) -- by the same kernel: the work is elementwise,
// the position table is not involved, and the destination may be one of the sources (a lane reads an entry of every source before it
// writes that entry).
//
// Streaming: a workgroup of 256 lanes takes CB_SPAN entries, lane t the entry pairs t, t + 256, ... of them as 16-byte loads and stores
// (every value array is an allocation of its own, so its base is aligned; the last entry of an odd count goes alone).  The loop over the
// slots is innermost: each output is written once, each input read once.  Up to CB_ARGS slot pointers and weights travel as kernel
// arguments; more come from a table on the device (op->cb).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "otmb_solve.h"

#define CB_SPAN 2048  // entries per workgroup: 256 lanes x 4 pairs
#define CB_ARGS 16    // terms that travel as kernel arguments

struct CbTerms {  // the terms in ascending slot order: the slot's array and its weight (never zero)
    const double *src[CB_ARGS];
    double w[CB_ARGS];
};

struct Cb2 {
    double a, b;
};
// entries i (even) and i + 1 of p; entry i + 1 counts only below count
__device__ __forceinline__ Cb2 cb_load(const double *p, i64 i, i64 count) {
    if (i + 1 < count) {
        const double2 v = *reinterpret_cast<const double2 *>(p + i);
        return {v.x, v.y};
    }
    return {p[i], 0.0};
}
__device__ __forceinline__ void cb_store(double *p, i64 i, i64 count, Cb2 v) {
    if (i + 1 < count) {
        *reinterpret_cast<double2 *>(p + i) = make_double2(v.a, v.b);
        return;
    }
    p[i] = v.a;
}

// dst[i] = the fold over the nt terms, i < count.  TABLE: the terms are tsrc / tw (device); otherwise q's.  dst may be one of the sources.
template <bool TABLE>
__global__ __launch_bounds__(256) void cb_combine_kernel(CbTerms q, const double *const *tsrc, const double *tw, int nt, i64 count, double *dst) {
    for (int r = 0; r < CB_SPAN / 512; ++r) {
        const i64 i = 2 * ((i64)blockIdx.x * (CB_SPAN / 2) + threadIdx.x + 256 * r);
        if (i >= count) break;
        Cb2 acc = {0.0, 0.0};
        for (int s = 0; s < nt; ++s) {
            const double w = TABLE ? tw[s] : q.w[s];
            const Cb2 v = cb_load(TABLE ? tsrc[s] : q.src[s], i, count);
            const double pa = w * v.a;
            const double pb = w * v.b;
            if (s == 0) {
                acc.a = pa;
                acc.b = pb;
            } else {
                acc.a = acc.a + pa;
                acc.b = acc.b + pb;
            }
        }
        cb_store(dst, i, count, acc);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// one value array: src[t] (nt of them, weights wt) -> dst, count entries; tab: the device table (nt > CB_ARGS), pointers then weights
static void cb_launch(hipStream_t st, const std::vector<const double *> &src, const std::vector<double> &wt, const void *tab, i64 count, double *dst) {
    if (count == 0) return;
    const int nt = (int)src.size();
    const dim3 grid((unsigned)((count + CB_SPAN - 1) / CB_SPAN)), block(256);
    CbTerms q = {};
    if (nt > CB_ARGS) {
        const double *const *tsrc = (const double *const *)tab;
        hipLaunchKernelGGL(cb_combine_kernel<true>, grid, block, 0, st, q, tsrc, (const double *)(tsrc + nt), nt, count, dst);
        return;
    }
    for (int t = 0; t < nt; ++t) q.src[t] = src[(size_t)t], q.w[t] = wt[(size_t)t];
    hipLaunchKernelGGL(cb_combine_kernel<false>, grid, block, 0, st, q, (const double *const *)nullptr, (const double *)nullptr, nt, count, dst);
}

// Σ_s w[s]·(slot s) -> `to` (a slot of the operator, or its private value set): both value arrays.  w: nslots finite host values (checked by
// the caller).  Enqueued on the context's stream.
int32_t cb_combine(otmb_op *op, const double *w, const OpSlot &to) {
    otmb_ctx *ctx = op->ctx;
    const i64 nslots = (i64)op->slots.size();
    std::vector<const double *> nz, val;
    std::vector<double> wt;
    for (i64 s = 0; s < nslots; ++s)
        if (w[s] != 0.0) {
            nz.push_back((const double *)op->slots[(size_t)s].nz.p);
            val.push_back((const double *)op->slots[(size_t)s].val.p);
            wt.push_back(w[s]);
        }
    const size_t nt = wt.size();
    const char *tab = nullptr;
    if (nt > CB_ARGS) {  // two tables, one per value array: nt pointers, then nt weights
        int32_t rc;
        if ((rc = otmb_reserve(ctx, op->cb, 4 * nt * 8))) return rc;
        tab = (const char *)op->cb.p;
        std::vector<unsigned long long> host(4 * nt);
        for (size_t t = 0; t < nt; ++t) {
            host[t] = (unsigned long long)(uintptr_t)nz[t];
            host[2 * nt + t] = (unsigned long long)(uintptr_t)val[t];
            memcpy(&host[nt + t], &wt[t], 8);
            memcpy(&host[3 * nt + t], &wt[t], 8);
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier call's kernels may still read the table)
        HIP_TRY(ctx, hipMemcpy(op->cb.p, host.data(), host.size() * 8, hipMemcpyHostToDevice));
    }
    cb_launch(ctx->stream, nz, wt, tab, op->nnz, (double *)to.nz.p);
    cb_launch(ctx->stream, val, wt, tab ? tab + 2 * nt * 8 : nullptr, op->nval, (double *)to.val.p);
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

static int32_t cb_check(otmb_op *op, const double *w, int64_t dst) {
    otmb_ctx *ctx = op->ctx;
    const i64 nslots = (i64)op->slots.size();
    if (!w) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (dst < 0 || dst >= nslots) {
        char msg[160];
        snprintf(msg, sizeof msg, "combine_slots: slot %lld is outside 0..%lld (otmb_op_set_slots)", (long long)dst, (long long)nslots - 1);
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
    }
    for (i64 s = 0; s < nslots; ++s)
        if (!std::isfinite(w[s])) {
            char msg[160];
            snprintf(msg, sizeof msg, "combine_slots: the weight of slot %lld is not finite", (long long)s);
            return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, msg);
        }
    return OTMB_OK;
}

extern "C" {

int32_t otmb_op_combine_slots_dev(otmb_op *op, const double *w, int64_t dst) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = cb_check(op, w, dst))) return rc;
    HIP_TRY(op->ctx, hipSetDevice(op->device));
    return cb_combine(op, w, op->slots[(size_t)dst]);
}

int32_t otmb_op_combine_slots(otmb_op *op, const double *w, int64_t dst) {
    const int32_t rc = otmb_op_combine_slots_dev(op, w, dst);
    if (rc == OTMB_OK) HIP_TRY(op->ctx, hipStreamSynchronize(op->ctx->stream));
    return rc;
}

}  // extern "C"
