// otmb_tm.h -- what the translation units of the transport-matrix assembly share on the HOST side: the tile geometry, the pending plan and
// the functions that cross files.  otmb_transportmatrix.hip holds the counting and the fill kernel, the two protocols and the entry points;
// otmb_tm_given.hip the operators a caller passes, otmb_tm_kept.hip the operators (and T's pattern) a caller kept, otmb_tm_order.hip the march
// order of the tiles, otmb_tm_fixup.hip T's compaction, otmb_tm_ring.hip the asynchronous steps' state ring and its fold.
// No device code here: files that need TmParams' fields include otmb_tm_column.h.
#pragma once
#include "otmb_common.h"

#ifndef TM_THREADS
#define TM_THREADS 256  // measured: one-wave (64-thread) tiles are no faster in fill
#endif
#define TM_NF 5
#ifndef TM_WAVES_PER_SIMD
// Governs every tm_kernel instantiation but the lean kept ones (GIVEN bit 6: <., 4 | 16 | 32 | 64> and <., 12 | 16 | 32 | 64>), which are bounded at
// four waves per SIMD and fit 128 VGPRs without scratch.  Measured on the five-matrix kernel: capping it at 128 VGPRs spills and is 8 % slower.
#define TM_WAVES_PER_SIMD 3
#endif
#define TM_MAXROWS 7  // rows per column: A, S, W, SELF, E, N|fold, B

struct TmPlan {
    otmb_tm_args args;  // device pointers
    i64 ntiles = 0;
    i64 nnz[5] = {0, 0, 0, 0, 0};
    bool valid = false;
    bool onepass_pending = false;
    i64 wet_base = 0;
    i64 nnz_base[5] = {0, 0, 0, 0, 0};
    bool rho_in_fill = false;  // the plan took its counts from facefluxes: no pass has looked at ρ yet, the fill pass does (:233)
    // otmb_tm_args.given: operators the caller passes (bit m).  derived: bit for bit what the fill pass computes -- re-derived in registers, not
    // materialised; foreign: any other matrix -- T is then the device sparse add of the four operands (two-phase protocol only)
    unsigned given = 0, derived = 0, foreign = 0;
    unsigned read = 0;         // (subset of derived) the derived ROWS with other values: not materialised either, but the fill pass reads the values
    unsigned skip = 0;         // matrices the kernels neither count nor write (TmParams.skip)
    bool want_t = true;        // the caller wants T (otmb_tm_args.skip_ops bit 0 clear)
    i64 built_nnz[5] = {0, 0, 0, 0, 0};  // (foreign) the counts of the matrices the kernel writes; nnz[0] is then the sparse adds' bound
    unsigned kept = 0;         // (subset of skip) otmb_tm_args.kept_ops honoured: the operator is where the previous write left it
    bool tpat = false;         // (two-phase) the plan honoured OTMB_KEPT_T_PATTERN: fill must be handed the recorded T arrays
};

// The operators a caller may promise to have kept (otmb_tm_args.kept_ops): functions of the grid and κ alone (src/matrixbuilding.jl:51-120)
static constexpr unsigned KEPT_OPS = (1u << OTMB_TKH) | (1u << OTMB_TKVML) | (1u << OTMB_TKVDEEP);

struct TmParams;  // otmb_tm_column.h

// ---- otmb_transportmatrix.hip
void otmb_tm_fill_params(TmParams &p, const otmb_tm_args &a, otmb_ctx *ctx, const TmPlan *pl);
// ignore: otmb_tm_args.ignore_ops; f: a step's flag words (NULL: ctx->h_flags)
int32_t otmb_tm_check_flags(otmb_ctx *ctx, const int *f = nullptr, int ignore = 0);
void otmb_tm_plan_free(otmb_ctx *ctx);
void otmb_tm_plan_invalidate(otmb_ctx *ctx);
int32_t otmb_tm_plan_query(otmb_ctx *ctx, int64_t *nnz, int64_t *N);
bool otmb_tm_plan_foreign(otmb_ctx *ctx);   // T of the last plan came out of the sparse adds
unsigned otmb_tm_plan_skip(otmb_ctx *ctx);  // matrices (bit m) the pending plan does not hand out

// ---- otmb_tm_ring.hip
int32_t otmb_tm_fetch_ring(otmb_ctx *ctx);
int32_t otmb_tm_fold_pending(otmb_ctx *ctx);

// ---- otmb_tm_fixup.hip
int32_t otmb_tm_t_fixup(otmb_ctx *ctx, i64 n, i64 nnz_base, i64 reserved, i64 *colptrT, i64 *rowvalT, double *nzvalT, i64 *actual_out);

// ---- otmb_tm_order.hip
int32_t otmb_tm_build_tile_order(otmb_ctx *ctx, const otmb_tm_args &a, i64 ntiles, const unsigned **order, unsigned *nheavy);

// ---- otmb_tm_given.hip
int32_t otmb_tm_classify_given(otmb_ctx *ctx, const otmb_tm_args &a, TmPlan &pl);
int32_t otmb_tm_foreign_sum(otmb_ctx *ctx, TmPlan &pl, const TmParams &p);

// ---- otmb_tm_kept.hip (the lifecycle of the records is stated there, once)
void otmb_tm_kept_decide(otmb_ctx *ctx, const otmb_tm_args &a, TmPlan &pl, int64_t *const colptr[5], int64_t *const rowval[5], double *const nzval[5],
                         const int64_t capacity[5], bool two_phase);
void otmb_tm_kept_plan_counts(otmb_ctx *ctx, TmPlan &pl, int64_t nnz[5]);
int32_t otmb_tm_kept_check_fill(otmb_ctx *ctx, TmPlan &pl, int64_t *const colptr[5], int64_t *const rowval[5], double *const nzval[5]);
void otmb_tm_kept_drop(otmb_ctx *ctx, unsigned keep, bool rho_promised);
int32_t otmb_tm_kept_before_fill(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, TmParams &p, bool two_phase, bool *tpat);
void otmb_tm_tpat_drop(otmb_ctx *ctx);
void otmb_tm_kept_after_sync_fill(otmb_ctx *ctx, const TmPlan &pl, const TmParams &p, bool tpat, bool t_cancel);
unsigned otmb_tm_kept_after_async_enqueue(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, const TmParams &p, const int64_t capacity[5],
                                          uint64_t serial, bool tpat);
void otmb_tm_kept_on_fold(otmb_ctx *ctx, const otmb_ctx::TmStepRec &rec, const int *f, const i64 *tot, otmb_ctx::TmStepResult &r);
void otmb_tm_kept_after_fixup(otmb_ctx *ctx, const void *colptrT, const void *rowvalT);
void otmb_tm_kept_stream_changed(otmb_ctx *ctx);
