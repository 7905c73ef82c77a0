// otmb_season.hip -- the weighted fold of nt dense blocks of the caller's (each rows x cols with the one leading dimension ld) into a compact
// destination of the operator's: the fields of a blended step of otmb_op_step_season[_dev] (otmb_step.hip) -- d and the source of step t,
// (1 - w)·(block a) + w·(block b) -- and the cycle-mean d̄ of otmb_op_periodic_season[_dev] with OTMB_OUTER_MEAN (otmb_periodic.hip), ONE
// launch over all columns each.  include/otmb.h states the contract; tests/season_ref.py restates it.
//
// Per entry: acc = w_0 * v_0 for the first term, then acc = acc + w_s * v_s in the order the terms are given, one operation per statement,
// no FMA (-ffp-contract=off): the fold of otmb_op_combine_slots.  The host drops zero weights (d̄) and gives a blended step's two terms as
// (1.0 - w, a), (w, b); no term at all: +0.0.
//
// It is not cb_combine_kernel, which reads 16-byte pairs from value arrays the operator allocated itself.  Here the blocks are the caller's
// tensors: separate allocations, any 8-byte alignment that may differ from block to block, padded leading dimensions, and with an odd n
// every second column 8 bytes off a 16-byte boundary.  So the access width is decided PER COLUMN, uniformly over the workgroup: when the
// column's first entry in the destination and in every term lies on a 16-byte boundary a lane takes its row pairs as 16-byte loads and
// stores, otherwise as two 8-byte ones each.  The arithmetic is the same either way, entry by entry, so the bits do not depend on it.
//
// A workgroup of 256 lanes takes SE_SPAN rows of one column (grid: x over the rows, y over the columns), lane t the row pairs t, t + 256,
// t + 512, t + 768; the last row of an odd count goes alone.  The loop over the terms is innermost: each output is written once, each
// input read once: (nt + 1)·8·rows·cols bytes.  Up to SE_ARGS terms travel as kernel arguments; more come from a table on the device
// (op->setab: nt pointers, then nt weights).  The destination is never one of the sources.  No LDS, no atomics, no host synchronisation
// on the argument path.  At the sizes of a tracer field (n·k doubles) the launch itself is most of the cost.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "otmb_solve.h"

#define SE_SPAN 2048  // rows of one column per workgroup: 256 lanes x 4 pairs
#define SE_ARGS 16    // terms that travel as kernel arguments

struct SeTerms {  // the terms in the order of the fold: the block and its weight
    const double *src[SE_ARGS];
    double w[SE_ARGS];
};

struct Se2 {
    double a, b;
};
// rows i (even) and i + 1 of the column at p; two: row i + 1 exists; wide: p + i is 16-byte aligned
__device__ __forceinline__ Se2 se_load(const double *__restrict__ p, i64 i, bool two, bool wide) {
    if (wide && two) {
        const double2 v = *reinterpret_cast<const double2 *>(p + i);
        return {v.x, v.y};
    }
    return {p[i], two ? p[i + 1] : 0.0};
}
__device__ __forceinline__ void se_store(double *__restrict__ p, i64 i, bool two, bool wide, Se2 v) {
    if (wide && two) {
        *reinterpret_cast<double2 *>(p + i) = make_double2(v.a, v.b);
        return;
    }
    p[i] = v.a;
    if (two) p[i + 1] = v.b;
}

// dst[i + c·ldo] = the fold over the nt terms of src_s[i + c·ld], i < rows, c < cols.  TABLE: the terms are tsrc / tw (device); otherwise q's.
template <bool TABLE>
__global__ __launch_bounds__(256) void se_fold_kernel(SeTerms q, const double *const *__restrict__ tsrc, const double *__restrict__ tw, int nt, i64 rows,
                                                      i64 cols, i64 ld, double *__restrict__ dst, i64 ldo) {
    for (i64 c = blockIdx.y; c < cols; c += gridDim.y) {
        const i64 off = c * ld;
        double *__restrict__ out = dst + c * ldo;
        bool wide = ((uintptr_t)out & 15) == 0;  // (uniform over the workgroup: pointers and the column only)
        for (int s = 0; s < nt; ++s) wide = wide && ((uintptr_t)((TABLE ? tsrc[s] : q.src[s]) + off) & 15) == 0;
#pragma unroll
        for (int r = 0; r < SE_SPAN / 512; ++r) {
            const i64 i = 2 * ((i64)blockIdx.x * (SE_SPAN / 2) + threadIdx.x + 256 * r);
            if (i >= rows) break;
            const bool two = i + 1 < rows;
            Se2 acc = {0.0, 0.0};
            for (int s = 0; s < nt; ++s) {
                const double w = TABLE ? tw[s] : q.w[s];
                const Se2 v = se_load((TABLE ? tsrc[s] : q.src[s]) + off, i, two, wide);
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
            se_store(out, i, two, wide, acc);
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// op->season at `doubles` doubles (allocated on first use, kept with the operator); may wait for the device: before a loop, never inside
int32_t se_reserve(otmb_op *op, size_t doubles) { return otmb_reserve(op->ctx, op->season, std::max<size_t>(doubles * 8, 8)); }

// Σ_t wt[t]·src[t] (each rows x cols, leading dimension ld; the fold's order is the vectors') -> dst (leading dimension ldo >= rows), one
// launch enqueued on the context's stream.  More than SE_ARGS terms: the table is written first, which waits for the stream.
int32_t se_fold(otmb_op *op, const std::vector<const double *> &src, const std::vector<double> &wt, i64 rows, i64 cols, i64 ld, double *dst, i64 ldo) {
    otmb_ctx *ctx = op->ctx;
    if (rows <= 0 || cols <= 0) return OTMB_OK;
    const size_t nt = src.size();
    if (nt == 0) {  // an empty fold: +0.0
        HIP_TRY(ctx, hipMemset2DAsync(dst, (size_t)ldo * 8, 0, (size_t)rows * 8, (size_t)cols, ctx->stream));
        return OTMB_OK;
    }
    const dim3 grid((unsigned)((rows + SE_SPAN - 1) / SE_SPAN), (unsigned)std::min<i64>(cols, 65535)), block(256);
    SeTerms q = {};
    if (nt > SE_ARGS) {
        int32_t rc;
        if ((rc = otmb_reserve(ctx, op->setab, 2 * nt * 8))) return rc;
        std::vector<unsigned long long> host(2 * nt);
        for (size_t t = 0; t < nt; ++t) {
            host[t] = (unsigned long long)(uintptr_t)src[t];
            memcpy(&host[nt + t], &wt[t], 8);
        }
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (an earlier call's kernel may still read the table)
        HIP_TRY(ctx, hipMemcpy(op->setab.p, host.data(), host.size() * 8, hipMemcpyHostToDevice));
        const double *const *tsrc = (const double *const *)op->setab.p;
        hipLaunchKernelGGL(se_fold_kernel<true>, grid, block, 0, ctx->stream, q, tsrc, (const double *)(tsrc + nt), (int)nt, rows, cols, ld, dst, ldo);
    } else {
        for (size_t t = 0; t < nt; ++t) q.src[t] = src[t], q.w[t] = wt[t];
        hipLaunchKernelGGL(se_fold_kernel<false>, grid, block, 0, ctx->stream, q, (const double *const *)nullptr, (const double *)nullptr, (int)nt, rows, cols, ld,
                           dst, ldo);
    }
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}
