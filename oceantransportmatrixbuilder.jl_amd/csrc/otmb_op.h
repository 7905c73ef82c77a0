// otmb_op.h -- the resident sparse operator's record, shared by its products (otmb_spmv.hip) and its solver (otmb_solve.hip).
// The layouts are described at the head of otmb_spmv.hip, which builds them and owns every buffer (sp_free_all).
#pragma once
#include "otmb_common.h"

#define SP_ELL_MAX 256   // longest row a slice takes
#define SP_TCH 512       // entries per LDS chunk of the Aᵀ and long-row kernels

struct otmb_op {
    otmb_ctx *ctx = nullptr;
    int device = 0;
    i64 m = 0, n = 0, nnz = 0;
    i64 nslices = 0, ell = 0, nlong = 0;  // slices, entries of the slice layout (padding included), long rows
    DevBuf cp, rv, nz;                    // CSC copy: colptr (n + 1, Int64), rowval - 1 (Int32), nzval
    DevBuf dst;                           // per stored entry: its position in val / col
    DevBuf elen, sbase, loff, lrows;      // per row: length or -1 (long); per slice: first position; per row: long-row offset; long rows
    DevBuf val, col;                      // slices then long rows: values and column indices (Int32, 0-based)
    DevBuf xs, ys;                        // staging of otmb_op_mul / otmb_op_solve (X and Y; B and X)
    DevBuf ds, sw;                        // otmb_op_solve: staging of d; the solver's vectors, partial sums and per-column records
};
