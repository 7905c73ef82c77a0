// otmb_op_fold.h -- the walk over each layout of the resident operator (described at the head of otmb_spmv.hip), once: the products
// (otmb_spmv.hip) and the solver (otmb_solve.hip) differ only in what they pass as f.  Each walk calls f(value, index) once per stored
// entry of the lane's row or column, in storage order; the start value, the arithmetic and what becomes of the sum are the caller's.
#pragma once
#include "otmb_op.h"

// a short row i (len = elen[i] >= 0) in its slice: index = the entry's column
template <class F>
__device__ __forceinline__ void op_fold_slice_row(const double *__restrict__ val, const int *__restrict__ col, const i64 *__restrict__ sbase, i64 i, int len,
                                                  F f) {
    const i64 base = sbase[i >> 6] + (i & 63);
    for (int e = 0; e < len; ++e) {
        const double v = val[base + 64 * (i64)e];
        const i64 j = col[base + 64 * (i64)e];
        f(v, j);
    }
}

// a long row, len entries from position b0, by a workgroup of 64 lanes: EVERY lane stages each chunk (coalesced) into sv / sc (SP_TCH
// entries of LDS each), the lanes with `on` fold it: index = the entry's column
template <class F>
__device__ __forceinline__ void op_fold_long_row(const double *__restrict__ val, const int *__restrict__ col, i64 b0, i64 len, double *sv, int *sc, int lane,
                                                 bool on, F f) {
    for (i64 lo = 0; lo < len; lo += SP_TCH) {
        const int w = (int)min((i64)SP_TCH, len - lo);
        __syncthreads();
        for (int t = lane; t < w; t += 64) {
            sv[t] = val[b0 + lo + t];
            sc[t] = col[b0 + lo + t];
        }
        __syncthreads();
        if (on)
            for (int t = 0; t < w; ++t) f(sv[t], (i64)sc[t]);
    }
}

// the CSC copy, by a workgroup of 64 lanes for the columns c0 .. c0 + 63: their entries are one contiguous run, staged in chunks through
// sv / sr; every lane folds the part of its own column colm = c0 + lane that lies in the chunk: index = the entry's row.
// Returns whether the lane has a column (colm < n); a lane without one calls f never.
template <class F>
__device__ __forceinline__ bool op_fold_csc_run(const i64 *__restrict__ cp, const int *__restrict__ rv, const double *__restrict__ nz, i64 n, double *sv,
                                                int *sr, i64 c0, int lane, i64 &colm, F f) {
    colm = c0 + lane;
    const bool has = colm < n;
    const i64 last = min(c0 + 64, n);
    const i64 wb = cp[c0] - 1, we = cp[last] - 1;
    const i64 mb = has ? cp[colm] - 1 : 0, me = has ? cp[colm + 1] - 1 : 0;
    for (i64 lo = wb; lo < we; lo += SP_TCH) {
        const int w = (int)min((i64)SP_TCH, we - lo);
        __syncthreads();
        for (int t = lane; t < w; t += 64) {
            sv[t] = nz[lo + t];
            sr[t] = rv[lo + t];
        }
        __syncthreads();
        const i64 a = max(mb, lo), b = min(me, lo + w);
        for (i64 e = a; e < b; ++e) {
            const double v = sv[e - lo];
            const i64 r = sr[e - lo];
            f(v, r);
        }
    }
    return has;
}
