// otmb_coarsen.hip -- the coarse operator C = LUMP * T * SPRAY (src/extratools.jl:14-16, test/local_full.jl:161) on the device.
//
// Semantics, restated from LinearAlgebra / SparseArrays as published (no reference test pins them):
//   * `LUMP * T * SPRAY` is the 3-argument `*`; _tri_matmul takes A*(B*C) only when that is strictly cheaper, and for shapes
//     (m x N)(N x M)(M x n) both costs are the same expression, so the product is (LUMP * T) * SPRAY;
//   * each `*` is spmatmul: column j of A * B walks B's entries (k, b) of column j in stored order and, for each, A's entries
//     (i, a) of column k in stored order; the first touch of row i COPIES a * b, later ones add it; rows come out ascending and
//     every touched row is stored, exact zeros included (no drop, unlike map(+) / otmb_spadd).
// The sum therefore has two levels: P[i,j] = sum_k LUMP[i,k] * T[k,j] is completed (sequentially over T's column j) before
// P[i,j] * SPRAY[j,J] enters C[i,J] (sequentially over SPRAY's column J).  A flat sum over all (j, k) differs in the last bit
// whenever two entries of one fine column land in one coarse row -- the common case inside a block.
// LUMP may hold at most one entry per column (every aggregation operator; lump_and_spray gives exactly one), which is what
// makes the contributions of one output column a short list: Σ_{j in SPRAY[:,J]} nnz(T[:,j]) of them.
//
// Two passes like every plan/fill pair here.  Plan: check the three matrices (every index before it is dereferenced), the work
// of every output column, then count its distinct rows -> colptr (kept in the context) and nnz.  Fill: rowval and nzval.
//   small path   every column's work <= CO_MAX_CAP: one 64-lane workgroup per output column lists the column's contributions in
//                LDS as keys (row << CO_SEQ_BITS | iteration index), bitonic-sorts them (the index makes the sort stable) and
//                sums every run of one row in iteration order -- iteration order is (position in SPRAY's column, position in
//                T's column), so a row's run is grouped by j and the two levels fall out of one walk.
//   sorted path  some column has more work (a huge block, a user-made SPRAY with everything in one column): the WHOLE call
//                expands every contribution into global memory in iteration order, radix-sorts (column, row) keys stably and
//                walks each (column, row) segment with the same two-level sum.  Slow but exact, like sparse() does for
//                sparse(I, J, V) (otmb_coo.hip); one path per call keeps the output positions a plain scan in both.
#include <hip/hip_runtime.h>

#include "otmb_prims.h"

#define CO_SEQ_BITS 12                      // iteration index inside a column (< CO_MAX_CAP)
#define CO_MAX_CAP 2048                     // largest per-column work of the small path (LDS: 22 B per contribution)
#define CO_MAX_ROW (1ll << (64 - CO_SEQ_BITS - 1))
enum { CO_BAD_AP = 1, CO_BAD_MULTI = 2, CO_BAD_AI = 4, CO_BAD_BP = 8, CO_BAD_BI = 16, CO_BAD_SP = 32, CO_BAD_SI = 64 };
#define CO_GRID(n) OTMB_GRID_STRIDE(n, ctx->stream)  // (every 256-thread kernel of this file strides over the grid)

struct CoArgs {
    const i64 *Ap, *Ai, *Bp, *Bi, *Sp, *Si;
    const double *Ax, *Bx, *Sx;
};

// ---- checks: nothing is dereferenced through an index before it has been checked ----------------------------------------
// colptr: p[c] <= p[c+1] inside [1, nnz + 1] (the host has read p[0] == 1 and p[ncols] == nnz + 1); maxper >= 0: at most that many
// entries per column (LUMP)
__global__ __launch_bounds__(256) void co_check_colptr_kernel(const i64 *__restrict__ p, i64 ncols, i64 nnz, int maxper, unsigned bit,
                                                              unsigned *__restrict__ bad) {
    for (i64 c = (i64)blockIdx.x * 256 + threadIdx.x; c < ncols; c += (i64)gridDim.x * 256) {
        const i64 a = p[c], b = p[c + 1];
        if (a < 1 || b < a || b > nnz + 1) atomicOr(bad, bit);
        else if (maxper >= 0 && b - a > maxper) atomicOr(bad, CO_BAD_MULTI);
    }
}
__global__ __launch_bounds__(256) void co_check_rowval_kernel(const i64 *__restrict__ r, i64 len, i64 maxrow, unsigned bit, unsigned *__restrict__ bad) {
    for (i64 e = (i64)blockIdx.x * 256 + threadIdx.x; e < len; e += (i64)gridDim.x * 256) {
        const i64 i = r[e];
        if (i < 1 || i > maxrow) atomicOr(bad, bit);
    }
}

// w[s] = nnz(B[:, Si[s]]) for every entry s of S (w[nnzS] = 0: the exclusive scan then ends with the total)
__global__ __launch_bounds__(256) void co_width_kernel(const i64 *__restrict__ Si, const i64 *__restrict__ Bp, i64 nnzS, const unsigned *__restrict__ bad,
                                                       i64 *__restrict__ w) {
    if (*bad) return;
    for (i64 s = (i64)blockIdx.x * 256 + threadIdx.x; s <= nnzS; s += (i64)gridDim.x * 256) {
        i64 v = 0;
        if (s < nnzS) {
            const i64 j = Si[s] - 1;
            v = Bp[j + 1] - Bp[j];
        }
        w[s] = v;
    }
}

// the work of output column J: max(contributions, entries of S's column); the largest over all columns -> *wmax
__global__ __launch_bounds__(256) void co_colwork_kernel(const i64 *__restrict__ Sp, const i64 *__restrict__ woff, i64 n, const unsigned *__restrict__ bad,
                                                         unsigned long long *__restrict__ wmax) {
    if (*bad) return;
    i64 best = 0;
    for (i64 J = (i64)blockIdx.x * 256 + threadIdx.x; J < n; J += (i64)gridDim.x * 256) {
        const i64 s0 = Sp[J] - 1, s1 = Sp[J + 1] - 1;
        const i64 w = woff[s1] - woff[s0];
        best = max(best, max(w, s1 - s0));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) best = max(best, (i64)__shfl_xor(best, d));
    if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(wmax, (unsigned long long)best);
}

// ---- the two-level sum over one row's run, in iteration order --------------------------------------------------------------
// x: a * b of a contribution, s: its position in S (the j it belongs to).  P = Σ_k x (first touch copies) over one s, then
// C = Σ_s P * S[s] (first touch copies).
struct CoSum {
    double c = 0.0, p = 0.0;
    i64 cur = -1;
    bool cfirst = true;
    __device__ __forceinline__ void flush(const double *__restrict__ Sx) {
        const double y = p * Sx[cur];
        c = cfirst ? y : c + y;
        cfirst = false;
    }
    __device__ __forceinline__ void add(i64 s, double x, const double *__restrict__ Sx) {
        if (s != cur) {
            if (cur >= 0) flush(Sx);
            p = x;
            cur = s;
        } else {
            p = p + x;
        }
    }
};

// ---- small path: one 64-lane workgroup per output column -----------------------------------------------------------------
// count: cnt[J + 1] = distinct rows of column J.  write: rowval / nzval at colptr[J].
template <int CAP, bool WRITE>
__global__ __launch_bounds__(64) void co_small_kernel(const CoArgs a, const i64 *__restrict__ woff, i64 *__restrict__ cnt, const i64 *__restrict__ colptr,
                                                      i64 *__restrict__ Ci, double *__restrict__ Cx) {
    __shared__ u64 key[CAP];
    __shared__ double xv[WRITE ? CAP : 1];
    __shared__ unsigned short sl[WRITE ? CAP : 1];
    __shared__ int wo[CAP + 1];
    const int lane = threadIdx.x;
    const i64 J = blockIdx.x;
    const i64 s0 = a.Sp[J] - 1, s1 = a.Sp[J + 1] - 1;
    const int ns = (int)(s1 - s0);
    const i64 base = woff[s0];
    const int W = (int)(woff[s1] - base);  // <= CAP (the plan picked CAP from the largest column)
    for (int q = lane; q <= ns; q += 64) wo[q] = (int)(woff[s0 + q] - base);
    __syncthreads();
    int P2 = 64;
    while (P2 < W) P2 <<= 1;
    for (int e = lane; e < P2; e += 64) {
        u64 k = ~0ull;  // no contribution (padding, or an empty LUMP column): sorts behind every row
        if (e < W) {
            int lo = 0, hi = ns;  // the entry of S this contribution belongs to: wo[lo] <= e < wo[hi]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (wo[mid] <= e) lo = mid; else hi = mid;
            }
            const i64 j = a.Si[s0 + lo] - 1;
            const i64 bpos = a.Bp[j] - 1 + (e - wo[lo]);
            const i64 kk = a.Bi[bpos] - 1;
            const i64 ap = a.Ap[kk] - 1;
            if (a.Ap[kk + 1] - 1 > ap) {
                k = ((u64)a.Ai[ap] << CO_SEQ_BITS) | (u64)e;
                if (WRITE) {
                    xv[e] = a.Ax[ap] * a.Bx[bpos];
                    sl[e] = (unsigned short)lo;
                }
            }
        }
        key[e] = k;
    }
    __syncthreads();
    for (int kk = 2; kk <= P2; kk <<= 1) {  // bitonic sort of key[0, P2): ascending (row, iteration index)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int t = lane; t < (P2 >> 1); t += 64) {
                const int e = 2 * jj * (t / jj) + (t % jj), f = e + jj;
                const bool up = (e & kk) == 0;
                const u64 x = key[e], y = key[f];
                if ((x > y) == up) {
                    key[e] = y;
                    key[f] = x;
                }
            }
            __syncthreads();
        }
    }
    const i64 out0 = WRITE ? colptr[J] - 1 : 0;
    int nhead = 0;
    for (int e0 = 0; e0 < W; e0 += 64) {
        const int e = e0 + lane;
        const u64 k = (e < W) ? key[e] : ~0ull;
        const u64 row = k >> CO_SEQ_BITS;
        const bool head = k != ~0ull && (e == 0 || (key[e - 1] >> CO_SEQ_BITS) != row);
        const u64 b = __ballot(head);
        if (WRITE && head) {
            CoSum sum;
            for (int f = e; f < W; ++f) {
                const u64 kf = key[f];
                if (kf == ~0ull || (kf >> CO_SEQ_BITS) != row) break;
                const int q = (int)(kf & ((1u << CO_SEQ_BITS) - 1));
                sum.add(s0 + sl[q], xv[q], a.Sx);
            }
            sum.flush(a.Sx);
            const i64 pos = out0 + nhead + __popcll(b & ((1ull << lane) - 1ull));
            Ci[pos] = (i64)row;
            Cx[pos] = sum.c;
        }
        nhead += __popcll(b);
    }
    if (!WRITE && lane == 0) cnt[J + 1] = nhead;
}

// ---- sorted path ---------------------------------------------------------------------------------------------------------
// every contribution in iteration order: e = woff[s] + t; key (J << rowbits) | i, or `invalid` (sorts last) for an empty LUMP column
__global__ __launch_bounds__(256) void co_expand_kernel(const CoArgs a, const i64 *__restrict__ woff, i64 nnzS, i64 n, int rowbits, u64 invalid,
                                                        u64 *__restrict__ keys, u64 *__restrict__ idx, double *__restrict__ val, i64 *__restrict__ sid) {
    for (i64 s = (i64)blockIdx.x * 256 + threadIdx.x; s < nnzS; s += (i64)gridDim.x * 256) {
        i64 lo = 0, hi = n;  // the column of S holding entry s: Sp[lo] - 1 <= s < Sp[lo + 1] - 1
        while (hi - lo > 1) {
            const i64 mid = (lo + hi) >> 1;
            if (a.Sp[mid] - 1 <= s) lo = mid; else hi = mid;
        }
        const i64 j = a.Si[s] - 1, b0 = a.Bp[j] - 1, b1 = a.Bp[j + 1] - 1;
        i64 e = woff[s];
        for (i64 bpos = b0; bpos < b1; ++bpos, ++e) {
            const i64 k = a.Bi[bpos] - 1, ap = a.Ap[k] - 1;
            const bool has = a.Ap[k + 1] - 1 > ap;
            keys[e] = has ? (((u64)(lo + 1) << rowbits) | (u64)a.Ai[ap]) : invalid;
            idx[e] = (u64)e;
            val[e] = has ? a.Ax[ap] * a.Bx[bpos] : 0.0;
            sid[e] = s;
        }
    }
}
// heads of the sorted (column, row) keys: h[f] = 1 at the first key of a segment, h[len] = 0
__global__ __launch_bounds__(256) void co_heads_kernel(const u64 *__restrict__ keys, i64 len, u64 invalid, i64 *__restrict__ h) {
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f <= len; f += (i64)gridDim.x * 256)
        h[f] = (f < len && keys[f] != invalid && (f == 0 || keys[f - 1] != keys[f])) ? 1 : 0;
}
// colptr[J] = 1 + heads before the first key of column J + 1 (1-based columns in the keys)
__global__ __launch_bounds__(256) void co_sorted_colptr_kernel(const u64 *__restrict__ keys, const i64 *__restrict__ hr, i64 len, i64 n, int rowbits,
                                                               i64 *__restrict__ colptr) {
    for (i64 J = (i64)blockIdx.x * 256 + threadIdx.x; J <= n; J += (i64)gridDim.x * 256) {
        const u64 want = (u64)(J + 1) << rowbits;
        i64 lo = 0, hi = len;  // first f with keys[f] >= want
        while (lo < hi) {
            const i64 mid = (lo + hi) >> 1;
            if (keys[mid] < want) lo = mid + 1; else hi = mid;
        }
        colptr[J] = 1 + hr[lo];
    }
}
__global__ __launch_bounds__(256) void co_sorted_fill_kernel(const u64 *__restrict__ keys, const u64 *__restrict__ idx, const double *__restrict__ val,
                                                             const i64 *__restrict__ sid, const i64 *__restrict__ hr, i64 len, u64 invalid, int rowbits,
                                                             const double *__restrict__ Sx, i64 *__restrict__ Ci, double *__restrict__ Cx) {
    for (i64 f = (i64)blockIdx.x * 256 + threadIdx.x; f < len; f += (i64)gridDim.x * 256) {
        const u64 k = keys[f];
        if (k == invalid || (f > 0 && keys[f - 1] == k)) continue;
        CoSum sum;
        for (i64 g = f; g < len && keys[g] == k; ++g) {
            const u64 e = idx[g];
            sum.add(sid[e], val[e], Sx);
        }
        sum.flush(Sx);
        const i64 q = hr[f];
        Ci[q] = (i64)(k & ((1ull << rowbits) - 1ull));
        Cx[q] = sum.c;
    }
}

__global__ void co_one_kernel(i64 *p) { p[0] = 1; }

static CoArgs co_args(const otmb_ctx::CoPlan &p) { return CoArgs{p.Ap, p.Ai, p.Bp, p.Bi, p.Sp, p.Si, p.Ax, p.Bx, p.Sx}; }

template <bool WRITE>
static void co_small_launch(otmb_ctx *ctx, int cap, const CoArgs &a, const i64 *woff, i64 n, i64 *cnt, const i64 *colptr, i64 *Ci, double *Cx) {
    const dim3 g((unsigned)n), b(64);
    switch (cap) {
        case 64: hipLaunchKernelGGL((co_small_kernel<64, WRITE>), g, b, 0, ctx->stream, a, woff, cnt, colptr, Ci, Cx); break;
        case 256: hipLaunchKernelGGL((co_small_kernel<256, WRITE>), g, b, 0, ctx->stream, a, woff, cnt, colptr, Ci, Cx); break;
        default: hipLaunchKernelGGL((co_small_kernel<CO_MAX_CAP, WRITE>), g, b, 0, ctx->stream, a, woff, cnt, colptr, Ci, Cx); break;
    }
}

extern "C" {

int32_t otmb_coarsen_plan_dev(otmb_ctx *ctx, int64_t m, int64_t N, const int64_t *Ap, const int64_t *Ai, const double *Ax, int64_t M,
                              const int64_t *Bp, const int64_t *Bi, const double *Bx, int64_t n, const int64_t *Sp, const int64_t *Si,
                              const double *Sx, int64_t *nnz) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    ctx->co_plan.nnz = -1;  // no valid plan until this one succeeds
    if (!nnz || !Ap || !Bp || !Sp) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (m < 0 || N < 0 || M < 0 || n < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "sizes");
    if (m >= CO_MAX_ROW || n >= (1ll << 31) || N >= (1ll << 40) || M >= (1ll << 40)) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "matrix too large");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // first and last column pointers of the three matrices
    i64 ends[6] = {0, 0, 0, 0, 0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(&ends[0], Ap, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[1], Ap + N, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[2], Bp, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[3], Bp + M, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[4], Sp, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&ends[5], Sp + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const i64 nA = ends[1] - 1, nB = ends[3] - 1, nS = ends[5] - 1;
    if (ends[0] != 1 || nA < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "LUMP: colptr");
    if (ends[2] != 1 || nB < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "T: colptr");
    if (ends[4] != 1 || nS < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "SPRAY: colptr");
    if ((nA > 0 && (!Ai || !Ax)) || (nB > 0 && (!Bi || !Bx)) || (nS > 0 && (!Si || !Sx))) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    int32_t rc;
    otmb_ctx::CoScratch &S = ctx->co;  // (otmb_common.h says what each member holds)
    if ((rc = otmb_reserve(ctx, S.flags, 64))) return rc;
    if ((rc = otmb_reserve(ctx, S.woff, (size_t)(nS + 1) * 16 + 16))) return rc;
    unsigned *bad = (unsigned *)S.flags.p;
    unsigned long long *wmax = (unsigned long long *)((char *)S.flags.p + 8);
    i64 *w = (i64 *)S.woff.p, *woff = w + (nS + 1);
    HIP_TRY(ctx, hipMemsetAsync(S.flags.p, 0, 16, ctx->stream));
    if (N > 0) hipLaunchKernelGGL(co_check_colptr_kernel, CO_GRID(N), (const i64 *)Ap, (i64)N, (i64)nA, 1, (unsigned)CO_BAD_AP, bad);
    if (M > 0) hipLaunchKernelGGL(co_check_colptr_kernel, CO_GRID(M), (const i64 *)Bp, (i64)M, (i64)nB, -1, (unsigned)CO_BAD_BP, bad);
    if (n > 0) hipLaunchKernelGGL(co_check_colptr_kernel, CO_GRID(n), (const i64 *)Sp, (i64)n, (i64)nS, -1, (unsigned)CO_BAD_SP, bad);
    if (nA > 0) hipLaunchKernelGGL(co_check_rowval_kernel, CO_GRID(nA), (const i64 *)Ai, (i64)nA, (i64)m, (unsigned)CO_BAD_AI, bad);
    if (nB > 0) hipLaunchKernelGGL(co_check_rowval_kernel, CO_GRID(nB), (const i64 *)Bi, (i64)nB, (i64)N, (unsigned)CO_BAD_BI, bad);
    if (nS > 0) hipLaunchKernelGGL(co_check_rowval_kernel, CO_GRID(nS), (const i64 *)Si, (i64)nS, (i64)M, (unsigned)CO_BAD_SI, bad);
    // (the kernels below return at once when a check failed: they would dereference the offending index)
    hipLaunchKernelGGL(co_width_kernel, CO_GRID(nS + 1), (const i64 *)Si, (const i64 *)Bp, (i64)nS, (const unsigned *)bad, w);
    if ((rc = otmb_exclusive_scan(ctx, S.prim_tmp, w, woff, nS + 1))) return rc;
    if (n > 0) hipLaunchKernelGGL(co_colwork_kernel, CO_GRID(n), (const i64 *)Sp, (const i64 *)woff, (i64)n, (const unsigned *)bad, wmax);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long st[2] = {0, 0};
    i64 total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(st, S.flags.p, 16, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(&total, woff + nS, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned b = (unsigned)st[0];
    if (b & CO_BAD_AP) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "LUMP: colptr not ascending inside [1, nnz + 1]");
    if (b & CO_BAD_BP) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "T: colptr not ascending inside [1, nnz + 1]");
    if (b & CO_BAD_SP) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "SPRAY: colptr not ascending inside [1, nnz + 1]");
    if (b & CO_BAD_MULTI) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "LUMP has a column with two or more stored entries");
    if (b & CO_BAD_AI) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "LUMP: row index outside 1:m");
    if (b & CO_BAD_BI) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "T: row index outside 1:N");
    if (b & CO_BAD_SI) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "SPRAY: row index outside 1:M");
    const i64 work = (i64)st[1];
    otmb_ctx::CoPlan &p = ctx->co_plan;
    p.Ap = Ap; p.Ai = Ai; p.Ax = Ax; p.Bp = Bp; p.Bi = Bi; p.Bx = Bx; p.Sp = Sp; p.Si = Si; p.Sx = Sx;
    p.m = m; p.N = N; p.M = M; p.n = n; p.nS = nS; p.len = total;
    p.cap = work <= 64 ? 64 : work <= 256 ? 256 : work <= CO_MAX_CAP ? CO_MAX_CAP : 0;
    if ((rc = otmb_reserve(ctx, S.cnt, (size_t)(n + 1) * 8))) return rc;
    if ((rc = otmb_reserve(ctx, S.colptr, (size_t)(n + 1) * 8))) return rc;
    i64 *cnt = (i64 *)S.cnt.p, *colptr = (i64 *)S.colptr.p;
    const CoArgs a = co_args(p);
    if (p.cap > 0) {
        hipLaunchKernelGGL(co_one_kernel, dim3(1), dim3(1), 0, ctx->stream, cnt);
        if (n > 0) co_small_launch<false>(ctx, p.cap, a, woff, n, cnt, nullptr, nullptr, nullptr);
        if ((rc = otmb_inclusive_scan(ctx, S.prim_tmp, cnt, colptr, n + 1))) return rc;  // colptr[J] = 1 + Σ_{J' < J} cnt
    } else {
        const i64 L = total;
        const int rowbits = otmb_bits(m), colbits = otmb_bits(n + 1);
        if (rowbits + colbits > 64) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "matrix too large for 64-bit (column, row) sort keys");
        const u64 invalid = (rowbits + colbits == 64) ? ~0ull : (1ull << (rowbits + colbits)) - 1ull;
        for (DevBuf *b : {&S.keys, &S.idx, &S.val, &S.sid})
            if ((rc = otmb_reserve(ctx, *b, (size_t)L * 16 + 16))) return rc;
        if ((rc = otmb_reserve(ctx, S.heads, (size_t)(L + 1) * 16 + 16))) return rc;
        u64 *k0 = (u64 *)S.keys.p, *k1 = k0 + L, *v0 = (u64 *)S.idx.p, *v1 = v0 + L;
        double *val = (double *)S.val.p;
        i64 *sid = (i64 *)S.sid.p, *h = (i64 *)S.heads.p, *hr = h + (L + 1);
        if (nS > 0) hipLaunchKernelGGL(co_expand_kernel, CO_GRID(nS), a, (const i64 *)woff, (i64)nS, (i64)n, rowbits, invalid, k0, v0, val, sid);
        if (L > 0 && (rc = otmb_sort_pairs(ctx, S.prim_tmp, k0, k1, v0, v1, L, rowbits + colbits))) return rc;
        hipLaunchKernelGGL(co_heads_kernel, CO_GRID(L + 1), (const u64 *)k1, (i64)L, invalid, h);
        if ((rc = otmb_exclusive_scan(ctx, S.prim_tmp, h, hr, L + 1))) return rc;
        hipLaunchKernelGGL(co_sorted_colptr_kernel, CO_GRID(n + 1), (const u64 *)k1, (const i64 *)hr, (i64)L, (i64)n, rowbits, colptr);
        p.rowbits = rowbits;
        p.invalid = invalid;
    }
    HIP_TRY(ctx, hipGetLastError());
    i64 last = 1;
    HIP_TRY(ctx, hipMemcpyAsync(&last, colptr + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    p.nnz = last - 1;
    *nnz = p.nnz;
    return OTMB_OK;
}

int32_t otmb_coarsen_fill_dev(otmb_ctx *ctx, int64_t *Cp, int64_t *Ci, double *Cx) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    otmb_ctx::CoPlan &p = ctx->co_plan;
    if (p.nnz < 0) return otmb_fail(ctx, OTMB_ERR_NO_PLAN);
    if (!Cp || (p.nnz > 0 && (!Ci || !Cx))) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const i64 n = p.n;
    const otmb_ctx::CoScratch &S = ctx->co;
    const i64 *colptr = (const i64 *)S.colptr.p;
    const CoArgs a = co_args(p);
    if (p.nnz > 0) {
        if (p.cap > 0) {
            const i64 *woff = (const i64 *)S.woff.p + (p.nS + 1);  // (behind w)
            co_small_launch<true>(ctx, p.cap, a, woff, n, nullptr, colptr, (i64 *)Ci, Cx);
        } else {
            const i64 L = p.len;
            const u64 *k1 = (const u64 *)S.keys.p + L, *v1 = (const u64 *)S.idx.p + L;
            const i64 *hr = (const i64 *)S.heads.p + (L + 1);
            hipLaunchKernelGGL(co_sorted_fill_kernel, CO_GRID(L), k1, v1, (const double *)S.val.p, (const i64 *)S.sid.p, hr, L, p.invalid,
                               p.rowbits, p.Sx, (i64 *)Ci, Cx);
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(Cp, colptr, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    p.nnz = -1;  // one fill per plan
    return OTMB_OK;
}

// host pointers: upload everything (every call: nothing is keyed to host addresses), plan on the device
int32_t otmb_coarsen_plan(otmb_ctx *ctx, int64_t m, int64_t N, const int64_t *Ap, const int64_t *Ai, const double *Ax, int64_t M,
                          const int64_t *Bp, const int64_t *Bi, const double *Bx, int64_t n, const int64_t *Sp, const int64_t *Si,
                          const double *Sx, int64_t *nnz) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    ctx->co_plan.nnz = -1;
    if (!nnz || !Ap || !Bp || !Sp) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    if (m < 0 || N < 0 || M < 0 || n < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "sizes");
    const i64 nA = Ap[N] - 1, nB = Bp[M] - 1, nS = Sp[n] - 1;
    if (Ap[0] != 1 || nA < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "LUMP: colptr");
    if (Bp[0] != 1 || nB < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "T: colptr");
    if (Sp[0] != 1 || nS < 0) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "SPRAY: colptr");
    if ((nA > 0 && (!Ai || !Ax)) || (nB > 0 && (!Bi || !Bx)) || (nS > 0 && (!Si || !Sx))) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevArena R;
    const size_t o_ap = R.take((size_t)(N + 1) * 8), o_ai = R.take((size_t)nA * 8), o_ax = R.take((size_t)nA * 8), o_bp = R.take((size_t)(M + 1) * 8),
                 o_bi = R.take((size_t)nB * 8), o_bx = R.take((size_t)nB * 8), o_sp = R.take((size_t)(n + 1) * 8), o_si = R.take((size_t)nS * 8),
                 o_sx = R.take((size_t)nS * 8);
    int32_t rc;
    if ((rc = otmb_reserve(ctx, ctx->co_host, R.total() + 256))) return rc;
    char *d = (char *)ctx->co_host.p;
    const struct { size_t o; const void *h; size_t bytes; } up[9] = {
        {o_ap, Ap, (size_t)(N + 1) * 8}, {o_ai, Ai, (size_t)nA * 8}, {o_ax, Ax, (size_t)nA * 8},
        {o_bp, Bp, (size_t)(M + 1) * 8}, {o_bi, Bi, (size_t)nB * 8}, {o_bx, Bx, (size_t)nB * 8},
        {o_sp, Sp, (size_t)(n + 1) * 8}, {o_si, Si, (size_t)nS * 8}, {o_sx, Sx, (size_t)nS * 8}};
    for (const auto &u : up)
        if (u.bytes) {
            HIP_TRY(ctx, hipMemcpyAsync(d + u.o, u.h, u.bytes, hipMemcpyHostToDevice, ctx->stream));
            ctx->uploaded_bytes += (i64)u.bytes;
        }
    return otmb_coarsen_plan_dev(ctx, m, N, (const i64 *)(d + o_ap), (const i64 *)(d + o_ai), (const double *)(d + o_ax), M, (const i64 *)(d + o_bp),
                                 (const i64 *)(d + o_bi), (const double *)(d + o_bx), n, (const i64 *)(d + o_sp), (const i64 *)(d + o_si),
                                 (const double *)(d + o_sx), nnz);
}

// fill the pending plan and download: Cp (n + 1), Ci / Cx (nnz of the plan)
int32_t otmb_coarsen_fetch(otmb_ctx *ctx, int64_t *Cp, int64_t *Ci, double *Cx) {
    if (!ctx) return OTMB_ERR_INVALID_ARG;
    const i64 nnz = ctx->co_plan.nnz, n = ctx->co_plan.n;
    if (nnz < 0) return otmb_fail(ctx, OTMB_ERR_NO_PLAN);
    if (!Cp || (nnz > 0 && (!Ci || !Cx))) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "null output");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int32_t rc;
    const size_t o_ci = ((size_t)(n + 1) * 8 + 255) & ~(size_t)255, o_cx = o_ci + (((size_t)nnz * 8 + 255) & ~(size_t)255);
    if ((rc = otmb_reserve(ctx, ctx->co_out, o_cx + (size_t)nnz * 8 + 256))) return rc;
    char *d = (char *)ctx->co_out.p;
    if ((rc = otmb_coarsen_fill_dev(ctx, (int64_t *)d, (int64_t *)(d + o_ci), (double *)(d + o_cx)))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(Cp, d, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (nnz > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(Ci, d + o_ci, (size_t)nnz * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(Cx, d + o_cx, (size_t)nnz * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return OTMB_OK;
}

}  // extern "C"
