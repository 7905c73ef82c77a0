// otmb_tm_fixup.hip -- T after an exact cancellation: compaction of the columns the fill pass (otmb_transportmatrix.hip) left with gaps.
#include "otmb_tm.h"

// ---- rare path: T had exact-zero sums, so its columns were written left-aligned in slots reserved for the
// union pattern.  Compact: per-column actual counts (tcount) -> scan -> move.  One thread per column.
#define TFIX_THREADS 256
#define TFIX_PER 4
// An entry is kept iff its value is not a zero (bits << 1 != 0: +0.0 and -0.0 alike).  T never stores an exact zero (:147), so this holds for
// both layouts the fill pass leaves: a full write (entries left-aligned, unused slots row 0 and value 0) and a values-only write on the kept
// pattern (OTMB_KEPT_T_PATTERN: entries at their union positions, a cancelled slot holds its zero sum).
__device__ __forceinline__ bool tfix_live(const i64 *__restrict__ valbits, i64 e) { return ((u64)valbits[e] << 1) != 0; }
__global__ __launch_bounds__(TFIX_THREADS) void tfix_derive(const i64 *__restrict__ colptr, const i64 *__restrict__ valbits, i64 n, i64 nnz_base,
                                                            uint8_t *__restrict__ tcount) {
    const i64 c = (i64)blockIdx.x * TFIX_THREADS + threadIdx.x;
    if (c >= n) return;
    const i64 lo = colptr[c] - 1 - nnz_base, hi = colptr[c + 1] - 1 - nnz_base;
    unsigned cnt = 0;
    for (i64 e = lo; e < hi && e < lo + TM_MAXROWS; ++e) cnt += tfix_live(valbits, e);
    tcount[c] = (uint8_t)cnt;
}
__global__ __launch_bounds__(TFIX_THREADS) void tfix_count(const uint8_t *__restrict__ tcount, i64 n, uint32_t *tilesums) {
    __shared__ unsigned part[TFIX_THREADS / 64];
    unsigned x = 0;
    for (int q = 0; q < TFIX_PER; ++q) {
        const i64 c = ((i64)blockIdx.x * TFIX_PER + q) * TFIX_THREADS + threadIdx.x;
        if (c < n) x += tcount[c];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) tilesums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ __launch_bounds__(TFIX_THREADS) void tfix_move(const uint8_t *__restrict__ tcount, i64 n, const i64 *__restrict__ tileoffs,
                                                          const i64 *__restrict__ old_colptr, const i64 *__restrict__ old_row,
                                                          const double *__restrict__ old_val, i64 nnz_base, i64 *new_colptr,
                                                          i64 *new_row, double *new_val) {
    __shared__ unsigned wave_tot[TFIX_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    i64 run = tileoffs[blockIdx.x];
    for (int q = 0; q < TFIX_PER; ++q) {
        const i64 c = ((i64)blockIdx.x * TFIX_PER + q) * TFIX_THREADS + tid;
        const unsigned mine = (c < n) ? tcount[c] : 0;
        unsigned incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            unsigned y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wave_tot[wid] = incl;
        __syncthreads();
        unsigned before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < TFIX_THREADS / 64; ++w) {
            const unsigned v = wave_tot[w];
            if (w < wid) before += v;
            all += v;
        }
        __syncthreads();
        if (c < n) {
            const i64 dst = run + before + incl - mine;  // entries before this column (this launch)
            const i64 lo = old_colptr[c] - 1 - nnz_base, hi = old_colptr[c + 1] - 1 - nnz_base;
            new_colptr[c] = nnz_base + dst + 1;
            unsigned q = 0;
            for (i64 e = lo; e < hi && e < lo + TM_MAXROWS; ++e) {  // the live entries in stored order (tfix_derive counted them)
                if (!tfix_live((const i64 *)old_val, e)) continue;
                new_row[dst + q] = old_row[e];
                new_val[dst + q] = old_val[e];
                ++q;
            }
        }
        run += all;
    }
}

// After a fill launch has completed and flagged FLAG_T_CANCEL: compact T in place (through temporaries).  n columns whose
// reserved (union-pattern) entries number `reserved`; *actual receives the final nnz.  The stream is idle on entry.
int32_t otmb_tm_t_fixup(otmb_ctx *ctx, i64 n, i64 nnz_base, i64 reserved, i64 *colptrT, i64 *rowvalT, double *nzvalT, i64 *actual_out) {
    *actual_out = reserved;
    if (n == 0) return OTMB_OK;
    const i64 per = (i64)TFIX_THREADS * TFIX_PER;
    const i64 nt = (n + per - 1) / per;
    int32_t rc;
    if ((rc = otmb_reserve(ctx, ctx->tcount, (size_t)n + 16))) return rc;
    if ((rc = otmb_reserve(ctx, ctx->blocksums, (size_t)(nt + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = otmb_reserve(ctx, ctx->blockoffs, (size_t)(nt + 1) * sizeof(i64) + otmb_scan_scratch(nt, 1)))) return rc;
    if ((rc = otmb_reserve(ctx, ctx->tfix[0], (size_t)(n + 1) * sizeof(i64)))) return rc;
    if ((rc = otmb_reserve(ctx, ctx->tfix[1], (size_t)(reserved + 1) * sizeof(i64)))) return rc;
    if ((rc = otmb_reserve(ctx, ctx->tfix[2], (size_t)(reserved + 1) * sizeof(double)))) return rc;
    int *dflags = (int *)ctx->flags.p;
    i64 *dtot = (i64 *)(dflags + OTMB_NFLAGS) + 8;
    uint8_t *tc = (uint8_t *)ctx->tcount.p;
    hipLaunchKernelGGL(tfix_derive, dim3((unsigned)((n + TFIX_THREADS - 1) / TFIX_THREADS)), dim3(TFIX_THREADS), 0, ctx->stream,
                       (const i64 *)colptrT, (const i64 *)nzvalT, n, nnz_base, tc);
    hipLaunchKernelGGL(tfix_count, dim3((unsigned)nt), dim3(TFIX_THREADS), 0, ctx->stream, (const uint8_t *)tc, n, (uint32_t *)ctx->blocksums.p);
    otmb_launch_tilescan(ctx->stream, (const uint32_t *)ctx->blocksums.p, (i64 *)ctx->blockoffs.p, dtot, nt, 1,
                         (i64 *)ctx->blockoffs.p + (nt + 1));
    hipLaunchKernelGGL(tfix_move, dim3((unsigned)nt), dim3(TFIX_THREADS), 0, ctx->stream, (const uint8_t *)tc, n, (const i64 *)ctx->blockoffs.p,
                       (const i64 *)colptrT, (const i64 *)rowvalT, (const double *)nzvalT, nnz_base,
                       (i64 *)ctx->tfix[0].p, (i64 *)ctx->tfix[1].p, (double *)ctx->tfix[2].p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_tot + 8, dtot, sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const i64 actual = ctx->h_tot[8];
    HIP_TRY(ctx, hipMemcpyAsync(colptrT, ctx->tfix[0].p, (size_t)n * sizeof(i64), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(rowvalT, ctx->tfix[1].p, (size_t)actual * sizeof(i64), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(nzvalT, ctx->tfix[2].p, (size_t)actual * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    const i64 last = nnz_base + actual + 1;
    HIP_TRY(ctx, hipMemcpyAsync(colptrT + n, &last, sizeof(i64), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *actual_out = actual;
    return OTMB_OK;
}
