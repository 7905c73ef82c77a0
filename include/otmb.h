/*
 * otmb.h -- C ABI of libotmb_hip.so: the MI355X (gfx950) implementation of the sparse
 * transport-operator assembly path of TMIP-code/OceanTransportMatrixBuilder.jl v0.8.3.
 *
 * The reference is pure Julia and has no FFI layer; its
 * boundary for this path is the keyword-argument API exported at
 * src/OceanTransportMatrixBuilder.jl:31-36.  Each entry point below names the reference
 * function it replaces; julia/OceanTransportMatrixBuilderAMD.jl binds them with `ccall`
 * behind the reference's own function names.
 *
 * Conventions
 *  - Arrays are Julia's: column-major (nx,ny,nz), i fastest; Float64 values; Int64 indices,
 *    1-based exactly as Julia stores them (colptr, rowval, Lwet, Lwet3D).  `missing` in
 *    Lwet3D is 0; `missing`/`nothing` in Float64 inputs is NaN.
 *  - `_dev` entry points take DEVICE pointers and enqueue on the context's stream; the
 *    entry points without the suffix take HOST pointers (what Julia's ccall passes) and
 *    stage through device memory owned by the context.
 *  - Every function returns an otmb_status; otmb_last_error(ctx) gives the message, which
 *    for the reference's own failures is the reference's exact error string.
 *  - A context is bound to one GPU, is not shared between threads, and has no global state.
 */
#ifndef OTMB_H
#define OTMB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct otmb_ctx otmb_ctx;

typedef enum {
    OTMB_OK = 0,
    OTMB_ERR_RHO_NAN = 1,          /* "ρ contains NaNs"        src/matrixbuilding.jl:233 */
    OTMB_ERR_TADV_NAN = 2,         /* "Tadv contains NaNs."    src/matrixbuilding.jl:39  */
    OTMB_ERR_TKH_NAN = 3,          /* "TκH contains NaNs."     src/matrixbuilding.jl:61  */
    OTMB_ERR_TKVML_NAN = 4,        /* "TκVML contains NaNs."   src/matrixbuilding.jl:90  */
    OTMB_ERR_TKVDEEP_NAN = 5,      /* "TκVdeep contains NaNs." src/matrixbuilding.jl:114 */
    OTMB_ERR_FLUX_INTO_LAND = 6,   /* reference throws from Lwet3D[nothing] / push!(…, missing) */
    OTMB_ERR_UNKNOWN_TOPOLOGY = 7, /* "Unknown grid type"      src/gridtopology.jl:111-116 */
    OTMB_ERR_ALL_MISSING = 8,      /* AssertionError           src/velocities.jl:199-200 */
    OTMB_ERR_ALLOC = 9,
    OTMB_ERR_HIP = 10,
    OTMB_ERR_INVALID_ARG = 11,
    OTMB_ERR_NO_PLAN = 12,         /* fill/fetch without a successful plan */
    OTMB_ERR_NONCANONICAL_INDICES = 13, /* Lwet3D is not what makeindices(v3D) returns */
    OTMB_ERR_CAPACITY = 14,
    OTMB_ERR_PUSH_MASK = 15,       /* args.push_mask does not describe args.phi / args.lwet3d (nothing was written) */
    OTMB_ERR_ASYMMETRIC_PATTERN = 16, /* lump_and_spray: Graphs.SimpleGraph's ArgumentError for a one-directional T pattern */
    OTMB_ERR_GIVEN_FOREIGN = 17,   /* otmb_tm_args.given: an operator that is NOT what this library derives for these arguments was handed to an
                                    * entry point that cannot add it (the asynchronous and the multi-slab builds): use otmb_transportmatrix_plan[_dev] */
    OTMB_ERR_SINGULAR_PRECONDITIONER = 18, /* otmb_op_solve: an entry of diag(σ·I + diag(d) + A) -- with OTMB_PRECOND_LINES: a pivot of the line
                                              factorisation -- is zero or not finite (the message names the first) */
    OTMB_ERR_NOT_CONVERGED = 19,   /* otmb_op_solve: some column stopped for another reason than convergence (reason[], relres[], iters[] say which) */
    OTMB_ERR_TSINK_NAN = 20,       /* "Tsink contains NaNs."  otmb_build_sink: the wording of the reference's own operators (no reference function) */
    OTMB_ERR_PATTERN_NOT_CONTAINED = 21 /* otmb_op_add_matrix: B stores an entry the operator does not (the message names the first; nothing was written) */
} otmb_status;

/* gridmetrics.gridtopology (src/gridtopology.jl:1-16) */
typedef enum { OTMB_BIPOLAR = 0, OTMB_TRIPOLAR = 1, OTMB_UNKNOWN_TOPOLOGY = 2 } otmb_topology;

/* order of the face-flux arrays: the fields of the NamedTuple returned at src/velocities.jl:245-252 */
enum { OTMB_EAST = 0, OTMB_WEST = 1, OTMB_NORTH = 2, OTMB_SOUTH = 3, OTMB_TOP = 4, OTMB_BOTTOM = 5 };
/* order of the per-direction (nx,ny) metric arrays edge_length_2D[dir], distance_to_neighbour_2D[dir] */
enum { OTMB_DIR_WEST = 0, OTMB_DIR_EAST = 1, OTMB_DIR_SOUTH = 2, OTMB_DIR_NORTH = 3 };
/* order of the five returned matrices: (; T, Tadv, TκH, TκVML, TκVdeep), src/matrixbuilding.jl:149 */
enum { OTMB_T = 0, OTMB_TADV = 1, OTMB_TKH = 2, OTMB_TKVML = 3, OTMB_TKVDEEP = 4 };

/* ---- context ------------------------------------------------------------------------------ */
int32_t otmb_ctx_create(int32_t device_id, otmb_ctx **out);
void otmb_ctx_destroy(otmb_ctx *ctx);
/* Borrow a hipStream_t (e.g. torch's current stream) for every _dev call; NULL = the ctx's own. */
int32_t otmb_ctx_set_stream(otmb_ctx *ctx, void *hip_stream);
/* Enqueue on the device's DEFAULT (null) stream instead -- the stream a framework uses when it has not been given
 * another one (torch's default stream has handle 0, which otmb_ctx_set_stream reads as "the ctx's own"): the
 * library's kernels are then ordered with the caller's own kernels and copies on that stream.                  */
int32_t otmb_ctx_use_default_stream(otmb_ctx *ctx);
int32_t otmb_ctx_synchronize(otmb_ctx *ctx);
/* Host-pointer entry points only.  The grid (gridmetrics, indices) does not change between the time slices a TMIP script
 * loops over (README.md:65-80), but every call hands the same host arrays over again: with reuse_grid on, a
 * grid-constant array (v3D, thkcello, Lwet3D, Lwet, wet3D, the 2-D metrics, zt) whose host pointer and size equal those
 * of the previous upload into its staging slot is NOT copied again -- the caller promises not to have modified it in
 * between.  Off by default (every call uploads everything, like the reference reads everything).                   */
int32_t otmb_ctx_set_reuse_grid(otmb_ctx *ctx, int32_t on);
/* Host-pointer entry points only.  otmb_facefluxes leaves the six ϕ arrays in the context's device staging; with
 * reuse_fluxes on, an otmb_transportmatrix_plan that is handed those very host arrays back (same pointers, same size)
 * does not upload them again (259 MB at 1 degree) -- the caller promises not to have modified them in between, which
 * is what a script that passes facefluxesfrommasstransport's result straight to transportmatrix does (README.md:65-80).
 * Off by default.                                                                                                */
int32_t otmb_ctx_set_reuse_fluxes(otmb_ctx *ctx, int32_t on);
/* reuse_grid and reuse_fluxes are independent promises (either may be on without the other).  Diagnostics: the bytes the
 * host-pointer entry points of this context have copied to the device so far -- what the two flags save.            */
int64_t otmb_ctx_uploaded_bytes(const otmb_ctx *ctx);
/* Pinned (page-locked) host memory owned by the context, for the arrays a caller hands to the host-pointer entry points:
 * a buffer inside such a block is the DMA's own source / target -- no staging copy, no page faults on freshly allocated
 * output arrays (1 GB of them per transportmatrix at 1 degree).  Julia: unsafe_wrap(Array, ptr, n) + a finalizer calling
 * otmb_host_free.  Freed blocks are kept and handed out again (up to 4 GiB idle).  ctx may be NULL (a caller that only uses an
 * otmb_mgpu has no single-device context): the pool belongs to no context.                                          */
int32_t otmb_host_alloc(otmb_ctx *ctx, int64_t bytes, void **out);
/* Lifetime and threads: the blocks belong to ONE pool of the process, behind a lock, which no context owns: otmb_ctx_destroy
 * frees none of them, and otmb_host_free IGNORES its context argument (NULL and an already destroyed context are fine) and may
 * be called from any thread at any time -- a garbage collector's finalizer thread while another thread is inside a call on the
 * context, or a finalizer that runs after the atexit hook that destroyed the context (Julia runs atexit hooks BEFORE its final
 * finalizer sweep).  Returns OTMB_ERR_INVALID_ARG for a pointer that is not a live block (e.g. freed twice).              */
int32_t otmb_host_free(otmb_ctx *ctx_ignored, void *p);
/* blocks handed out and not yet freed, their bytes, and the bytes kept idle for reuse (any argument may be NULL) */
int32_t otmb_host_pool_stats(int64_t *blocks_in_use, int64_t *bytes_in_use, int64_t *bytes_idle);
/* Speed only, never results: the order in which the fill pass of transportmatrix takes its tiles of 256 columns.
 * rows_per_band = 0: ascending wet rank (i, then j, then k).  R > 0: MARCH order -- the tiles of a band of R grid rows
 * are taken level after level before the next band starts, so that the levels above / below a tile (the vertical
 * neighbours of src/matrixbuilding.jl:280-296, :450-477) were read moments ago and are still in the L2 / Infinity Cache
 * instead of one whole level (124 MB of inputs on a 0.25 degree grid) earlier.  -1 (default): the library's choice (bands of
 * 8 rows: with the matrices written by non-temporal stores, 8 % faster than wet-rank order at 1 and at 0.25 degree).
 * On grids whose rows are longer than 1536 cells a band is further cut into equal blocks of columns (3 x 1200 on a 3600-cell
 * row): what an XCD's L2 keeps from one level to the next is rows x columns cells -- HBM fetch of the fill pass on the 0.1 degree
 * grid 70 -> 48 GB, its time unchanged (profiles/r04/README.md section 10).  Environment, read when a context is created, for
 * experiments only: OTMB_MARCH_ROWS, OTMB_MARCH_COLS (0 = whole rows).                                                       */
int32_t otmb_ctx_set_tile_order(otmb_ctx *ctx, int32_t rows_per_band);
const char *otmb_last_error(const otmb_ctx *ctx);
const char *otmb_status_string(int32_t status); /* the reference's error text for codes 1-8 */
const char *otmb_version(void);
/* Optional per-kernel timing: when enabled every kernel launch is bracketed by two hipEvents on
 * the launch stream.  collect() synchronises, adds the elapsed times per kernel id, returns the
 * sums (ms) and launch counts since the previous collect for ids 0..n-1 and resets them.      */
int32_t otmb_ctx_timing_enable(otmb_ctx *ctx, int32_t on);
int32_t otmb_ctx_timing_collect(otmb_ctx *ctx, double *ms_sum, int64_t *count, int32_t n);
const char *otmb_kernel_name(int32_t kernel_id);
/* Diagnostic (not part of any result): what the box this context runs on sustains for one plain HBM read stream and one plain
 * non-temporal HBM write stream (2 GiB each, all CUs, 16 bytes per lane, eight accesses in flight), in GB/s.  bench.py reports a
 * kernel's time as a fraction of the rate these two give for the kernel's own read : write mix.  Allocates 2 GiB for the call.   */
int32_t otmb_ctx_box_ceilings(otmb_ctx *ctx, double *read_gbs, double *write_gbs);
/* Diagnostic, DESTRUCTIVE for the outputs: the plainest kernel there is over the very arrays a kernel reads and writes -- every byte of the
 * n_in input arrays read once, every byte of the n_out output arrays written once (device pointers, 16-byte aligned; at most 24 each), cut
 * into `tiles` proportional slices taken by one workgroup each in the fill pass's XCD-contiguous order.  *gbs = bytes / time: what an ideal
 * streaming kernel with this byte mix reaches ON THESE ALLOCATIONS -- the fill pass's time depends reproducibly on where its ~30 arrays lie
 * in the HBM (profiles/r04 section 12), which the two plain streams of otmb_ctx_box_ceilings do not see.                              */
int32_t otmb_ctx_stream_mix(otmb_ctx *ctx, int32_t n_in, const void *const *in, const int64_t *in_bytes, int32_t n_out,
                            void *const *out, const int64_t *out_bytes, int64_t tiles, double *gbs);

/* ---- makeindices(v3D)  -- src/matrixbuilding.jl:10-24 ------------------------------------- *
 * wet = !isnan(v3D).  Outputs (any may be NULL): lwet3d (nx*ny*nz) wet rank or 0;
 * lwet (capacity nx*ny*nz; first N valid) ascending 1-based linear indices of wet cells;
 * wet3d (nx*ny*nz bytes, 0/1).  *n_wet receives N (host memory in both variants).        */
int32_t otmb_makeindices_dev(otmb_ctx *ctx, const double *v3d, int64_t nx, int64_t ny, int64_t nz,
                             int64_t *lwet3d, int64_t *lwet, uint8_t *wet3d, int64_t *n_wet);
int32_t otmb_makeindices(otmb_ctx *ctx, const double *v3d, int64_t nx, int64_t ny, int64_t nz,
                         int64_t *lwet3d, int64_t *lwet, uint8_t *wet3d, int64_t *n_wet);

/* ---- facefluxes(umo, vmo, gridmetrics, indices; FillValue) -- src/velocities.jl:190-255,
 *      including nofluxboundaries! (:154-179) and the Float64 conversion of
 *      facefluxesfrommasstransport (:118-130).
 * umo/vmo: (nx,ny,nz), Float64 (src_is_f32 == 0) or Float32 (== 1, the CMIP on-disk type);
 * they are NOT modified (the reference mutates only its converted copies).  `fill` is the
 * _FillValue promoted to Float64.  phi[6]: outputs in OTMB_EAST..OTMB_BOTTOM order.         */
int32_t otmb_facefluxes_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32,
                            const uint8_t *wet3d, double fill, int64_t nx, int64_t ny, int64_t nz,
                            int32_t topology, double *const phi[6]);
int32_t otmb_facefluxes(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32,
                        const uint8_t *wet3d, double fill, int64_t nx, int64_t ny, int64_t nz,
                        int32_t topology, double *const phi[6]);

/* Depth-slab variant for multi-GPU runs (no counterpart in the single-process reference; it continues
 * the bottom-up continuity recurrence of src/velocities.jl:236-243 across slabs without re-association):
 * the nz levels handed in are levels [k0,k1) of a deeper grid and top_below (nx*ny, NULL for the deepest
 * slab) is ϕtop of level k1 from the slab below.  Asynchronous; the :199-200 assertion concerns the
 * whole grid, so each slab's two validity flags are read with otmb_facefluxes_slab_flags (synchronises)
 * and OR-ed across slabs by the caller.                                                             */
int32_t otmb_facefluxes_slab_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32,
                                 const uint8_t *wet3d, double fill, int64_t nx, int64_t ny, int64_t nz,
                                 int32_t topology, double *const phi[6], const double *top_below, uint16_t *push_mask);
/* The same for ONE ROW BAND of the plane: rows [j0, j1) (0-based) of every level.  A cell's fluxes depend on its own column's
 * top_below and on INPUTS of its west / south neighbours only, so the chain over depth slabs can run piece by piece -- slab s piece c
 * waits for slab s + 1 piece c, not for its whole plane (src/velocities.jl:236-243) -- with bit-identical arrays for any
 * partition of the rows.  top_below / the phi arrays are whole-plane arrays as above; first = 1 on the first piece of a field
 * (all pieces of a field share one pair of validity flags).                                                               */
int32_t otmb_facefluxes_rows_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32,
                                 const uint8_t *wet3d, double fill, int64_t nx, int64_t ny, int64_t nz,
                                 int32_t topology, double *const phi[6], const double *top_below, uint16_t *push_mask,
                                 int64_t j0, int64_t j1, int32_t first);
int32_t otmb_facefluxes_slab_flags(otmb_ctx *ctx, int32_t *u_valid, int32_t *v_valid);
/* Speed only.  nofluxboundaries! (src/velocities.jl:161-175) looks at the wet byte of every cell AND of its east, west,
 * south and north (or fold) neighbours, for every level of every time slice -- all grid constants.  otmb_wetflags_dev folds
 * the five into one byte per cell (bit 0 the cell, bits 1-4 east, west, south, north; asynchronous; once per grid), and
 * otmb_facefluxes_flags_dev is otmb_facefluxes_slab_dev reading that array instead of wet3d: five loads per cell and
 * level instead of nine, the same six ϕ arrays and push mask bit for bit.                                      */
int32_t otmb_wetflags_dev(otmb_ctx *ctx, const uint8_t *wet3d, int64_t nx, int64_t ny, int64_t nz, int32_t topology,
                          uint8_t *wetflags);
int32_t otmb_facefluxes_flags_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32,
                                  const uint8_t *wetflags, double fill, int64_t nx, int64_t ny, int64_t nz,
                                  int32_t topology, double *const phi[6], const double *top_below, uint16_t *push_mask);
/* Speed only: facefluxes that ALSO counts.  Which rows the four operators of transportmatrix hold in column c
 * (src/matrixbuilding.jl:244-296, :348-415, :450-477) follows from the wet mask, the mixed-layer mask zt[k] < mlotst[i,j] (:85) and the
 * signs of the fluxes c's six neighbours push with -- which, for fluxes facefluxes itself writes, are c's OWN six fluxes
 * (ϕwest[E] = ϕeast[c], ..., ϕbottom[A] = ϕtop[c]: src/velocities.jl:206-224, :238-240).  otmb_facefluxes_counts_dev is
 * otmb_facefluxes_flags_dev whose kernel also accumulates, per tile of 256 matrix columns, the row counts of Tadv and TκVML that
 * transportmatrix's counting pass would derive (the counts of TκH, TκVdeep and T's reserved union depend on the wet mask alone and come
 * from the grid's tables); an otmb_transportmatrix_dev / _plan_dev that is then handed EXACTLY these ϕ arrays, this push_mask pointer,
 * mlotst, zt, lwet3d, n_wet, topology, upwind and only_t -- with no other facefluxes call on the context in between -- skips its
 * counting pass (6-7 % of a device-resident step).  Any other transportmatrix call counts for itself as before, and the fill pass
 * compares every tile's counts with the columns it builds (OTMB_ERR_PUSH_MASK), so stale counts cannot produce a wrong matrix.
 * In this mode push_mask is NOT written: the pointer only names the fluxes (the library knows and never reads it as a mask).  Whole
 * grids only (no top_below, wet ranks from 1).  Falls back to otmb_facefluxes_flags_dev's behaviour (mask written, no counts) when
 * nx < 3 or OTMB_COUNT_IN_FF=0.
 * tables: once per grid by otmb_count_tables_dev from the indices and otmb_wetflags_dev's bytes (otmb_count_tables_bytes bytes: the wet
 * rank of the first wet cell of every segment a wave of the kernel covers -- 64 cells, or 32 where it marches two levels per wave,
 * otmb_ctx_ff_pairs -- and the static counts of every tile).  Both
 * asynchronous.                                                                                                                   */
typedef struct {
    const void *tables;      /* otmb_count_tables_dev */
    const int64_t *lwet3d;   /* indices.Lwet3D */
    const double *mlotst;    /* (nx,ny) */
    const double *zt;        /* (nz) */
    int64_t n_wet;
    int32_t upwind;          /* as otmb_tm_args.upwind */
    int32_t only_t;          /* as otmb_tm_args.only_t */
} otmb_ff_counts;
int64_t otmb_count_tables_bytes(const otmb_ctx *ctx, int64_t nx, int64_t ny, int64_t nz, int64_t n_wet);
int32_t otmb_count_tables_dev(otmb_ctx *ctx, const int64_t *lwet3d, const int64_t *lwet, const uint8_t *wetflags, int64_t n_wet,
                              int64_t nx, int64_t ny, int64_t nz, int32_t topology, void *tables);
int32_t otmb_facefluxes_counts_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32,
                                   const uint8_t *wetflags, double fill, int64_t nx, int64_t ny, int64_t nz,
                                   int32_t topology, double *const phi[6], uint16_t *push_mask, const otmb_ff_counts *counts);
/* The same for a depth slab (otmb_facefluxes_slab_dev / _rows_dev: SURVEY 8e, the chain over depth slabs).  The slab's nz levels are
 * levels [k_own0, k_own0 + nz) of its EXTENDED local grid of nz_ext levels -- the owned levels plus one halo level above (k_own0 = 1)
 * and / or below (k_own0 + nz < nz_ext), whose cells are neighbours of owned cells and rows of the slab's matrices but not columns.
 * wetflags (otmb_wetflags_dev of the extended grid's mask), counts->zt and counts->lwet3d are arrays of the EXTENDED grid, exactly the
 * ones the slab's otmb_tm_args will name; umo, vmo, phi[6], push_mask and top_below hold the owned levels only, as for
 * otmb_facefluxes_rows_dev.  counts->n_wet: the slab's owned wet cells; wet_base: the global 0-based wet rank of the first of them
 * (otmb_transportmatrix_set_slab).  The transportmatrix call that may skip its counting pass is the one whose arguments are the extended
 * arrays these owned-level pointers lie in (phi[d] - k_own0 * nx * ny, ...), after the halo planes' fluxes have been put in place.
 * j0, j1, first: a row band, as for otmb_facefluxes_rows_dev (bands other than the whole plane count only under the four-row wave
 * geometry of large planes; otherwise -- and wherever otmb_facefluxes_counts_dev falls back -- the mask is written and nothing is
 * counted).                                                                                                                       */
typedef struct {
    int64_t k_own0;   /* first owned level inside the extended local grid (0-based): 0 or 1 */
    int64_t nz_ext;   /* levels of the extended local grid (<= nz + 2) */
    int64_t wet_base; /* global 0-based wet rank of the slab's first owned wet cell */
} otmb_ff_slab;
int32_t otmb_count_tables_slab_dev(otmb_ctx *ctx, const int64_t *lwet3d, const int64_t *lwet, const uint8_t *wetflags, int64_t n_wet,
                                   int64_t nx, int64_t ny, int64_t nz, int32_t topology, const otmb_ff_slab *slab, void *tables);
int32_t otmb_facefluxes_slab_counts_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32, const uint8_t *wetflags,
                                        double fill, int64_t nx, int64_t ny, int64_t nz, int32_t topology, double *const phi[6],
                                        const double *top_below, uint16_t *push_mask, const otmb_ff_counts *counts,
                                        const otmb_ff_slab *slab, int64_t j0, int64_t j1, int32_t first);
/* 1 when the last facefluxes call on this context counted (its push_mask argument was therefore not written, and need not be completed
 * for halo planes by otmb_push_mask_dev), 0 when it took the plain kernel or the counts have been consumed.  No device work.   */
int32_t otmb_facefluxes_counts_pending(const otmb_ctx *ctx);
/* Which kernel the last facefluxes call on this context ran: 1 the one that marches two levels per wave (whole-plane counting calls on
 * whole grids of two levels or more whose ceil(nx ny / 32) waves are all resident at once; OTMB_FF_PAIRS=0 never, =1 whatever the size),
 * 0 the one-level kernel, -1 no call yet.  The count tables of such a grid hold segments of 32 columns: build them and call facefluxes
 * on contexts created under the same OTMB_FF_PAIRS and OTMB_FF_ROWS (tables of another geometry are recognised: the transportmatrix
 * then reports OTMB_ERR_PUSH_MASK, as for any counts that do not describe the fluxes).  No device work.                          */
int32_t otmb_ctx_ff_pairs(const otmb_ctx *ctx);
/* The tile scan of a transportmatrix.  Up to otmb_ctx_tm_infill_groups scan groups of 1024 tiles (64; OTMB_TM_INFILL_GROUPS = 0 .. 64,
 * read when the context is created and clamped, lowers it for tests) a one-pass call scans inside the groups only and its fill pass adds
 * the group bases; beyond, and in the two-phase plan, all scan levels run.  otmb_ctx_tm_infill: which of the two the last transportmatrix
 * call with at least one tile took -- 1 the fill pass adds the bases, 0 all levels, -1 no such call yet.  The matrices are the same
 * either way.  No device work.                                                                                                     */
int32_t otmb_ctx_tm_infill_groups(const otmb_ctx *ctx);
int32_t otmb_ctx_tm_infill(const otmb_ctx *ctx);
/* The same two flags for EVERY facefluxes call on this context since the previous call of this function, oldest
 * first (a pipeline of asynchronous steps: the reference asserts per call, src/velocities.jl:199-200, so a field
 * without a single valid value in step 3 of 12 must not be hidden by steps 4-12).  Synchronises.  At most the 64
 * most recent calls are remembered: drain the pipeline at least that often.                                  */
int32_t otmb_facefluxes_pending_flags(otmb_ctx *ctx, int32_t capacity, int32_t *u_valid, int32_t *v_valid,
                                      int32_t *n_calls);

/* Push mask: what the pattern of the advection operator needs to know about a cell's six fluxes, 16 bits per
 * cell.  Bits 0-5: the cell sends mass through its west, east, south, north, bottom, top face under upwind
 * weighting, i.e. max(ϕwest,0), min(ϕeast,0), max(ϕsouth,0), min(ϕnorth,0), max(ϕbottom,0), min(ϕtop,0) is
 * non-zero (src/matrixbuilding.jl:244,253,262,271,280,289); bit 6: the cell is wet; bits 8-14: the same for
 * centred weighting (ϕ/2 non-zero).  otmb_facefluxes_slab_dev writes it for the cells it computes when
 * push_mask is not NULL (the fluxes are in registers there); otmb_push_mask_dev derives it from existing ϕ
 * arrays for the cells [first, first+count) (0-based linear indices; halo planes of a depth slab, or fluxes
 * that were modified after facefluxes).  Asynchronous.                                                  */
int32_t otmb_push_mask_dev(otmb_ctx *ctx, const double *const phi[6], const int64_t *lwet3d, int64_t first,
                           int64_t count, uint16_t *push_mask);

/* ---- velocity2fluxes / fluxes2velocity -- src/velocities.jl:10-39, :50-74 (nanmean2 :89-93, nanmin2 :108);
 *      with facefluxes they make facefluxesfromvelocities (:140-151).  Default C-grid (u on east faces, v on
 *      north faces; the reference passes C-grid fields through, src/gridcellgeometry.jl:104).
 * u/v (or phi_i/phi_j): (nx,ny,nz) Float64 or Float32 (src_is_f32); rho: (nx,ny,nz) or NULL with rho_scalar;
 * edge_east/edge_north: gridmetrics.edge_length_2D[:east], [:north] (nx,ny).  Every cell is computed, as in
 * the reference.  A bipolar topology is an error (the reference indexes thkcello[nothing] at j == ny).    */
/* B-grid (u, v on the NE corner, e.g. ACCESS-ESM1-5 uo/vo) -> default C-grid:
 * interpolateontodefaultCgrid(…, ::BGridCell), src/gridcellgeometry.jl:106-140: _FillValue -> 0, then
 * u2 = 0.5 (u + u one row south), v2 = 0.5 (v + v one cell west), zero shifted in at j == 1 / i == 1.    */
int32_t otmb_bgrid_to_cgrid_dev(otmb_ctx *ctx, const void *u, const void *v, int32_t src_is_f32, double fill,
                                int64_t nx, int64_t ny, int64_t nz, double *u2, double *v2);
int32_t otmb_bgrid_to_cgrid(otmb_ctx *ctx, const void *u, const void *v, int32_t src_is_f32, double fill,
                            int64_t nx, int64_t ny, int64_t nz, double *u2, double *v2);
int32_t otmb_velocity2fluxes_dev(otmb_ctx *ctx, const void *u, const void *v, int32_t src_is_f32, const double *rho,
                                 double rho_scalar, const double *thkcello, const double *edge_east,
                                 const double *edge_north, int64_t nx, int64_t ny, int64_t nz, int32_t topology,
                                 double *phi_i, double *phi_j);
int32_t otmb_fluxes2velocity_dev(otmb_ctx *ctx, const void *phi_i, const void *phi_j, int32_t src_is_f32,
                                 const double *rho, double rho_scalar, const double *thkcello, const double *edge_east,
                                 const double *edge_north, int64_t nx, int64_t ny, int64_t nz, int32_t topology,
                                 double *u, double *v);
int32_t otmb_velocity2fluxes(otmb_ctx *ctx, const void *u, const void *v, int32_t src_is_f32, const double *rho,
                             double rho_scalar, const double *thkcello, const double *edge_east,
                             const double *edge_north, int64_t nx, int64_t ny, int64_t nz, int32_t topology,
                             double *phi_i, double *phi_j);
int32_t otmb_fluxes2velocity(otmb_ctx *ctx, const void *phi_i, const void *phi_j, int32_t src_is_f32, const double *rho,
                             double rho_scalar, const double *thkcello, const double *edge_east,
                             const double *edge_north, int64_t nx, int64_t ny, int64_t nz, int32_t topology,
                             double *u, double *v);

/* ---- transportmatrix(; ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind)
 *      -- src/matrixbuilding.jl:128-150 with buildTadv/TκH/TκVML/TκVdeep (:31-120), the three
 *      *_operator_sparse_entries generators (:221-299, :337-418, :438-479), sparse() x4 and
 *      T = Tadv + TκH + TκVML + TκVdeep (:147), fused: each wet cell's column of all five
 *      matrices is produced directly in CSC order.                                          */
/* A SparseMatrixCSC{Float64,Int64} by its three arrays, 1-based as Julia stores them: colptr (columns + 1), rowval / nzval (nnz). */
typedef struct {
    const int64_t *colptr;
    const int64_t *rowval;
    const double *nzval;
    int64_t nnz;
} otmb_csc;

typedef struct {
    int64_t nx, ny, nz;
    int32_t topology;            /* otmb_topology */
    int32_t upwind;              /* 1: upwind (default), 0: centred */
    int64_t n_wet;               /* indices.N */
    const double *phi[6];        /* ϕ.east, west, north, south, top, bottom: (nx,ny,nz) */
    const double *v3d;           /* gridmetrics.v3D      (nx,ny,nz), NaN on land */
    const double *thkcello;      /* gridmetrics.thkcello (nx,ny,nz) */
    const double *rho;           /* ρ as (nx,ny,nz) array, or NULL to use rho_scalar */
    double rho_scalar;
    const int64_t *lwet3d;       /* indices.Lwet3D (nx,ny,nz), 0 = missing */
    const int64_t *lwet;         /* indices.Lwet (n_wet): ascending 1-based linear indices of the wet cells */
    const double *edge_length[4];/* gridmetrics.edge_length_2D[dir]           (nx,ny), OTMB_DIR_* order */
    const double *dist_nbr[4];   /* gridmetrics.distance_to_neighbour_2D[dir] (nx,ny) */
    const double *area2d;        /* gridmetrics.area2D (nx,ny) */
    const double *zt;            /* gridmetrics.zt (nz) */
    const double *mlotst;        /* mlotst (nx,ny), NaN = missing */
    double kappa_h, kappa_vml, kappa_vdeep;
    const uint16_t *push_mask;   /* optional (device pointer, NULL = derived from phi and lwet3d by the library): the
                                  * per-cell push mask written by otmb_facefluxes_slab_dev / otmb_push_mask_dev for
                                  * exactly these phi and this wet mask; lets the counting pass read 2 bytes per
                                  * neighbour instead of re-reading the six ϕ arrays.  Host-pointer entry points
                                  * ignore it.                                                                   */
    int32_t only_t;              /* extension (0 = the reference's behaviour): non-zero builds T alone -- the four operator
                                  * matrices are still evaluated (T is their sum) but neither counted nor written: their
                                  * nnz come out 0 and their output pointers may be NULL.  Halves the bytes written.      */
    int32_t ignore_ops;          /* bit m (m = OTMB_TADV .. OTMB_TKVDEEP): the caller already HAS operator m (transportmatrix's
                                  * Tadv / TκH / TκVML / TκVdeep keywords, src/matrixbuilding.jl:133-143) -- the reference then never
                                  * builds it, so nothing it alone would have raised is raised: "Tadv contains NaNs.", "ρ contains
                                  * NaNs" and a flux into land for Tadv, "TκH / TκVML / TκVdeep contains NaNs." for the others.  The
                                  * matrices of ignored operators and T are still written and are the caller's to discard.       */
    int32_t skip_ops;            /* extension: bit m (m = OTMB_T .. OTMB_TKVDEEP): the caller does not WANT matrix m -- it is evaluated where T needs
                                  * it but neither counted, written nor copied home (its nnz comes out 0, its outputs may be NULL).  only_t is
                                  * skip_ops = the four operator bits.  buildTadv / buildTκH / buildTκVML / buildTκVdeep (src/matrixbuilding.jl:31-120)
                                  * are this call with every bit but one set, and ignore_ops for the operators they do not build.               */
    otmb_csc given[5];           /* given[m].colptr != NULL (m = OTMB_TADV .. OTMB_TKVDEEP; given[OTMB_T] stays zero): transportmatrix's
                                  * Tadv = / TκH = / TκVML = / TκVdeep = keyword (src/matrixbuilding.jl:133-143) -- the caller PASSES operator m
                                  * (N x N; device arrays for the _dev entry points, host arrays for the others).  As in the reference it
                                  * is then NOT built: not counted, not stored, not copied home (nnz[m] comes back 0, the outputs of m may be
                                  * NULL: the caller returns the very object it passed, :149), nothing it alone would raise is raised (as
                                  * ignore_ops), and T = ((Tadv + TκH) + TκVML) + TκVdeep (:147) is formed with the GIVEN matrix:
                                  *  - TκH / TκVdeep are functions of the grid and κ alone.  A given one whose three arrays are bit for bit
                                  *    what this library derives for these gridmetrics / indices / κ ("derived": checked on the device by
                                  *    one pass that compares instead of stores, the verdict kept per context and operator until one of
                                  *    the arrays it names changes -- otmb_ctx_forget_given) is re-derived in registers by the fill pass:
                                  *    its 16 nnz + 8 (N + 1) bytes are not written (29 % of the fill pass's bytes at 1 degree for
                                  *    TκH + TκVdeep, 40 % of the bytes a host caller waits for); TκH's values are read where they lie when
                                  *    that is cheaper than re-deriving them.
                                  *  - A given TκH / TκVdeep with exactly the derived ROWS and other values -- built with another κ, which is
                                  *    what a caller passes who leaves the call's own κH / κVdeep at their defaults -- is treated alike, and
                                  *    the fill pass READS its values where they lie: T carries the given values, in every protocol.
                                  *  - any other given matrix (another pattern, Tadv, TκVML) is "foreign": the built operators
                                  *    are written as usual and T is formed by the device sparse add (otmb_spadd_*_dev: left fold, exact
                                  *    zeros dropped) from the given arrays where they lie.  Two-phase entry points only
                                  *    (otmb_transportmatrix_plan[_dev] + fill / fetch: the plan's nnz[0] is then the sum of the four
                                  *    operands' counts); the asynchronous and multi-slab builds return OTMB_ERR_GIVEN_FOREIGN.
                                  * In a depth-slab launch (otmb_transportmatrix_set_slab) given[m] names the slab's columns: colptr
                                  * its n_wet + 1 entries (global numbering), rowval / nzval the entries from colptr[0] on, nnz their number. */
    int32_t kept_ops;            /* _dev entry points only (the host-pointer and multi-slab builds ignore it); 0 = the reference's behaviour.
                                  * Bit m (m = OTMB_TKH, OTMB_TKVML, OTMB_TKVDEEP -- grid constants, src/matrixbuilding.jl:51-120): the caller
                                  * PROMISES that the output arrays it passes for operator m are the ones this context's previous successful
                                  * call wrote for m, untouched since.  The library keeps a record per operator (output pointers, capacity,
                                  * grid array addresses, κ, topology, n_wet, slab, the otmb_ctx_forget_given epoch, the nnz it wrote) and
                                  * honours the bit only when the record matches this call: operator m is then re-derived in registers (T
                                  * needs it) but neither counted nor stored, and its nnz comes back from the record.  Anything else --
                                  * no record, other arguments, a given operator / skip_ops / only_t that left the slot unwritten, an
                                  * asynchronous step that wrote it and failed, otmb_ctx_forget_given -- writes it in full.  An
                                  * asynchronous step that relied on a step which then failed reports that step's status.  Two-phase
                                  * protocol: fill must be handed the recorded arrays for a kept operator (otherwise OTMB_ERR_INVALID_ARG:
                                  * plan again without the bit).  A write to those arrays the caller does not tell the library about
                                  * (another library call, a raw pointer) must be followed by a call without the bit.  When all three
                                  * bits are honoured, TκH's values are not re-derived either: they come from a table this context
                                  * keeps (built by the first such call after any call without the TκH bit; OTMB_KEPT_HTAB=0: re-derived),
                                  * so T itself then depends on it.  A write the library is not told about to a grid array TκH is
                                  * derived from (v3d, thkcello, edge_length, dist_nbr, lwet3d, lwet) must therefore also be followed by
                                  * a call without the bit.
                                  * Bit 5, OTMB_KEPT_T_PATTERN: the colptr / rowval arrays passed for T are the ones this context last
                                  * wrote T's pattern into, untouched since.  T's reserved pattern is a function of the wet mask and the
                                  * topology alone, so a fill that keeps all three operators and reads the TκH table then stores T's
                                  * VALUES only, at the positions that write left (otmb_ctx_kept_t_pattern).  The library honours it only
                                  * when its own record matches: the last writer of T's pattern into exactly these arrays, for these
                                  * arguments, finished without error or exact cancellation (a pending asynchronous step does not count).
                                  * Anything else writes T in full.  Two-phase protocol: fill must be handed the recorded arrays when the
                                  * plan honoured the bit (otherwise OTMB_ERR_INVALID_ARG).
                                  * Bit 6, OTMB_KEPT_RHO: `rho` is the array, with the contents, of this context's previous successful
                                  * call.  ρ is not among the kept operators' keys, so the library cannot know it is unchanged; with the
                                  * promise, a fill that keeps all three operators and reads the neighbour table takes v3D and ρ (3-D
                                  * only) from a table in wet-rank order that it builds from `rho` once (otmb_ctx_kept_vrtab;
                                  * OTMB_KEPT_VRTAB=0: gathered as before).  Honoured on that path only; a call without the bit drops
                                  * the table, so a loop whose ρ changes every step never builds it.                                   */
} otmb_tm_args;
#define OTMB_KEPT_T_PATTERN (1 << 5)
#define OTMB_KEPT_RHO (1 << 6)
/* The verdicts on otmb_tm_args.given are keyed to array ADDRESSES (the given matrix's and the gridmetrics / indices arrays') and κ.
 * A device-resident caller that rewrites one of those arrays in place calls this before the next transportmatrix; the host-pointer
 * entry points do it themselves whenever they upload such an array (i.e. always, unless otmb_ctx_set_reuse_grid promises otherwise). */
int32_t otmb_ctx_forget_given(otmb_ctx *ctx);
/* Diagnostics: how the last plan / _dev call on this context treated operator m: 0 not given, 1 given and derived, 2 given and foreign,
 * 3 given with the derived rows and other values (read by the fill pass). */
int32_t otmb_ctx_given_state(const otmb_ctx *ctx, int32_t m);
/* ... and how many comparing passes the context has run so far (a time loop with resident arrays runs ONE). */
int64_t otmb_ctx_given_checks(const otmb_ctx *ctx);
/* ... and whether the last fill pass on this context that kept all three diffusive operators (otmb_tm_args.kept_ops) read TκH from the
 * context's table: 1 yes, 0 no (OTMB_KEPT_HTAB=0, nx < 3, the table could not be allocated), -1 no such fill yet. */
int32_t otmb_ctx_kept_htab(const otmb_ctx *ctx);
/* ... and whether it took the neighbours' wet ranks from the context's per-grid table instead of gathering Lwet3D: 1 yes, 0 no
 * (OTMB_KEPT_NBTAB=0 or no TκH table, a depth slab, the table could not be allocated), -1 no such fill yet. */
int32_t otmb_ctx_kept_nbtab(const otmb_ctx *ctx);
/* ... and whether it took v3D and ρ from the context's {v3D, ρ} table in wet-rank order instead of gathering them: 1 yes, 0 no
 * (no OTMB_KEPT_RHO promise, OTMB_KEPT_VRTAB=0 or no neighbour table, a scalar ρ, a depth slab, the table could not be allocated),
 * -1 no such fill yet. */
int32_t otmb_ctx_kept_vrtab(const otmb_ctx *ctx);
/* ... and whether it ran as the lean instantiation of the fill kernel, which fits four waves per SIMD instead of three: 1 yes (whenever
 * the {v3D, ρ} table is read), 0 no (that table is not read, or OTMB_KEPT_OCC4=0 in the environment), -1 no such fill yet.  The columns
 * written are bit for bit the same either way. */
int32_t otmb_ctx_kept_occ4(const otmb_ctx *ctx);
/* ... and whether that fill stored T's values only (otmb_tm_args.kept_ops & OTMB_KEPT_T_PATTERN honoured): 1 yes, 0 no (T written in full),
 * -1 no such fill yet.  OTMB_KEPT_TPAT=0 in the environment always writes T in full. */
int32_t otmb_ctx_kept_t_pattern(const otmb_ctx *ctx);
/* ... and how many fills on this context have stored T's values only so far: unlike otmb_ctx_kept_t_pattern (which a fill that does not keep all
 * three operators leaves as it was), the count changes with every such fill -- read it before and after a call to learn what THAT call did
 * (DeviceAssembler decides with it whether a resident operator over T may keep its plan, otmb_op_*). */
int64_t otmb_ctx_kept_t_pattern_fills(const otmb_ctx *ctx);

/* Two-phase protocol so the CALLER allocates the outputs (Julia owns its SparseMatrixCSC buffers).
 * plan: the nnz of the four operator matrices (exact: their patterns depend on the wet mask, the flux
 *   signs and the mixed-layer mask only) and an UPPER BOUND for T = the union pattern (T drops entries
 *   whose sum is exactly zero, src/matrixbuilding.jl:147 -- rare, and only known once values exist).
 * fill (synchronous): writes colptr[m] (n_wet+1), rowval[m], nzval[m] for the five matrices in
 *   OTMB_T..OTMB_TKVDEEP order, raises the reference's errors, compacts T if entries cancelled;
 *   otmb_transportmatrix_nnz then gives the final counts (nnz[0] <= the planned bound).
 * The args of the last plan are remembered by the context; a plan is consumed by its fill (fill again = plan again). */
int32_t otmb_transportmatrix_plan_dev(otmb_ctx *ctx, const otmb_tm_args *args, int64_t nnz[5]);
int32_t otmb_transportmatrix_fill_dev(otmb_ctx *ctx, int64_t *const colptr[5], int64_t *const rowval[5],
                                      double *const nzval[5]);
/* Asynchronous variant for device-resident callers that preallocate the outputs at an upper bound (a column
 * holds at most 7, 7, 5, 3, 3 entries of T, Tadv, TκH, TκVML, TκVdeep): count -> scan -> fill are enqueued back
 * to back with no host round trip.  capacity[m] = entries rowval[m]/nzval[m] can hold; colptr[m] holds
 * n_wet+1.  otmb_transportmatrix_result synchronises, raises the reference's errors / OTMB_ERR_CAPACITY,
 * compacts T if entries cancelled and returns the five nnz.
 * One exception to "no host round trip": the FIRST call for a grid (and the first after otmb_ctx_set_stream changed the stream)
 * builds the fill pass's tile order and waits for its number of heavy tiles -- one stream synchronisation per grid, not per step. */
int32_t otmb_transportmatrix_dev(otmb_ctx *ctx, const otmb_tm_args *args, int64_t *const colptr[5],
                                 int64_t *const rowval[5], double *const nzval[5], const int64_t capacity[5]);
/* Extension for device-resident pipelines that go from (umo, vmo) straight to the matrices and do not need the six ϕ arrays themselves:
 * ONE call = otmb_facefluxes_counts_dev + otmb_transportmatrix_dev with the SAME five matrices bit for bit, but only ϕtop is ever stored
 * (phi_top: nx*ny*nz doubles of the caller's; it holds facefluxes' ϕtop afterwards).  The other five fluxes are what facefluxes would have
 * stored -- ϕeast / ϕwest / ϕnorth / ϕsouth are masked copies of umo / vmo (nofluxboundaries! + replace + shift, src/velocities.jl:161-175,
 * :203-224), ϕbottom is ϕtop of the level below (:238-240) -- and the fill pass re-derives them where it uses them: 64 bytes per cell less
 * HBM traffic than writing six arrays and reading them back (~14 % of a step).  args->phi and args->push_mask are ignored; wetflags /
 * count_tables as for otmb_facefluxes_counts_dev; asynchronous like otmb_transportmatrix_dev (otmb_transportmatrix_result,
 * otmb_facefluxes_pending_flags collect the verdicts).  Whole grids, nx >= 3, nz <= 128.  NOT a replacement for the two-call API:
 * facefluxesfrommasstransport returns the six arrays (src/velocities.jl:245-254).                                                       */
int32_t otmb_step_dev(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32, double fill, const uint8_t *wetflags,
                      const void *count_tables, double *phi_top, const otmb_tm_args *args, int64_t *const colptr[5],
                      int64_t *const rowval[5], double *const nzval[5], const int64_t capacity[5]);
int32_t otmb_transportmatrix_result(otmb_ctx *ctx, int64_t nnz[5]);
/* Several otmb_transportmatrix_dev calls may be enqueued before one otmb_transportmatrix_result (a pipeline over time
 * slices).  Every call keeps its own error flags, its own nnz and its own output arrays: like every transportmatrix call of
 * the reference returns its own five matrices (src/matrixbuilding.jl:147-149).  result reports the FIRST call that
 * failed -- where the reference would have thrown (src/matrixbuilding.jl:39,61,90,114,233) -- with "(asynchronous step k
 * of n)" appended to otmb_last_error; when none failed it returns the nnz of the last call, and EVERY call's T has been
 * compacted in that call's own arrays if entries of it cancelled.  The outputs of a call are defined until a later call is
 * handed the same arrays (a caller that keeps one result set, like bench.py, keeps the last call's matrices).
 * failed_step: 0-based index of the failing call among the calls since the previous result, -1 if the last result found
 * no failure.  result_step (after result): status and nnz of the k-th of those calls.                              */
int32_t otmb_transportmatrix_failed_step(otmb_ctx *ctx, int64_t *step);
int32_t otmb_transportmatrix_result_step(otmb_ctx *ctx, int64_t step, int64_t nnz[5]);

/* Depth-slab partition (multi-GPU).  The wet index is k-slowest (src/matrixbuilding.jl:14-15), so a slab
 * of levels owns a contiguous column range of every matrix.  set_slab (before plan / _dev): the local
 * grid holds this rank's levels plus halo levels that act as neighbours only; args.lwet lists the OWNED
 * wet cells (local linear indices), args.n_wet their number, lwet3d holds GLOBAL wet ranks and wet_base
 * = (global rank of the first owned wet cell) - 1.  set_nnz_base (before fill / _dev): entries of each
 * matrix owned by the slabs above, so that colptr (n_wet+1 entries, local columns) is written with
 * global offsets and the slabs' arrays concatenate into the global CSC.  set_slab(ctx, 0) resets.   */
int32_t otmb_transportmatrix_set_slab(otmb_ctx *ctx, int64_t wet_base);
int32_t otmb_transportmatrix_set_nnz_base(otmb_ctx *ctx, const int64_t nnz_base[5]);
int32_t otmb_transportmatrix_plan(otmb_ctx *ctx, const otmb_tm_args *args, int64_t nnz[5]);
int32_t otmb_transportmatrix_nnz(otmb_ctx *ctx, int64_t nnz[5]);
/* host variant of fill: nnz_out receives the final counts (trim T's arrays to nnz_out[0]) */
int32_t otmb_transportmatrix_fetch(otmb_ctx *ctx, int64_t *const colptr[5], int64_t *const rowval[5],
                                   double *const nzval[5], int64_t nnz_out[5]);

/* ---- the same two calls over SEVERAL GPUs of one process: transportmatrix(...; devices = 0:7) ---------------------------
 * No counterpart in the single-threaded reference (src/matrixbuilding.jl:128-150 is the call shape that is kept).  The wet
 * index is k-slowest (src/matrixbuilding.jl:14-15): a slab of consecutive levels owns a contiguous column range of every matrix
 * and a contiguous range of every (nx,ny,nz) array.  An otmb_mgpu owns one context and one host thread per device, cuts the
 * levels with otmb_balanced_partition (wet counts as even as a sweep gets them) and moves every slab over ITS device's PCIe
 * link.  HOST pointers of the WHOLE grid go in and come out, exactly as for otmb_facefluxes / otmb_transportmatrix_plan /
 * _fetch, and the results are the same bit for bit:
 *   otmb_mgpu_facefluxes            the continuity recurrence (src/velocities.jl:236-243) is a chain in k with a fixed
 *                                   association: slabs run deepest first and hand ONE (nx,ny) plane of ϕtop per boundary to
 *                                   the slab above -- a grouped ncclSend / ncclRecv pair on a single-process communicator
 *                                   (ncclCommInitAll: RCCL over xGMI) between different devices; a device-to-device copy
 *                                   when the slabs share a device (every device id equal: tests on a one-GPU box);
 *   otmb_mgpu_transportmatrix_plan  every slab uploads its levels plus one halo level each side (neighbours only) from the
 *                                   host arrays -- nothing crosses devices; nnz = sums over the slabs (T: the union bound);
 *   otmb_mgpu_transportmatrix_fetch every slab fills its column range with global colptr offsets and copies it into its
 *                                   range of the caller's five matrices; T is compacted across slabs if entries cancelled.
 * device_ids: all different (RCCL; OTMB_MGPU_TRANSPORT=peer selects hipMemcpyPeerAsync) or all equal.  Errors: the status of
 * the first failing check in the reference's order over all slabs; otmb_mgpu_last_error names the slab.  An otmb_mgpu is not
 * shared between threads.  transport: 0 same-device copy, 1 RCCL, 2 peer copy.                                            */
typedef struct otmb_mgpu otmb_mgpu;
int32_t otmb_mgpu_create(int32_t ndev, const int32_t *device_ids, otmb_mgpu **out);
void otmb_mgpu_destroy(otmb_mgpu *mg);
const char *otmb_mgpu_last_error(const otmb_mgpu *mg);
int32_t otmb_mgpu_ndev(const otmb_mgpu *mg);
int32_t otmb_mgpu_transport(const otmb_mgpu *mg);
/* level bounds of the last facefluxes / plan: ndev + 1 entries, slab s = levels [bounds[s], bounds[s+1]) (0-based) */
int32_t otmb_mgpu_partition(const otmb_mgpu *mg, int64_t *bounds);
/* nslabs consecutive slabs of >= 1 level each with wet counts as even as a greedy sweep gets them (upper levels are wetter);
 * bounds: nslabs + 1 entries.  Pure host arithmetic, no GPU.                                                              */
int32_t otmb_balanced_partition(const int64_t *level_counts, int64_t nz, int32_t nslabs, int64_t *bounds);
/* The two promises of otmb_ctx_set_reuse_grid / otmb_ctx_set_reuse_fluxes, for the slabs (independent, both off by default): grid-constant
 * host arrays that are the very arrays of the previous plan (same pointers, same cut) are not uploaded again; ϕ that otmb_mgpu_facefluxes
 * computed and copied to these very host arrays is used where it is -- every slab keeps its levels on its device in the layout the plan
 * wants, with the one flux each halo level pushes into an owned cell filled in (ϕbottom above = the slab's first ϕtop,
 * src/velocities.jl:240; ϕtop below = the plane received from the slab below).  otmb_mgpu_uploaded_bytes: host -> device bytes so far. */
int32_t otmb_mgpu_set_reuse(otmb_mgpu *mg, int32_t reuse_grid, int32_t reuse_fluxes);
/* Speed only: the facefluxes chain hands its plane from slab to slab in `pieces` row bands (whole rows), so that slab s starts piece c
 * as soon as piece c of slab s + 1 has arrived: critical path of one field t_ff / W x (1 + (W - 1) / pieces) instead of t_ff
 * (src/velocities.jl:236-243).  0 (default): 4 on grids of 2^19 columns and more, else 1.  Same arrays for any number. */
int32_t otmb_mgpu_set_chain_pieces(otmb_mgpu *mg, int32_t pieces);
int64_t otmb_mgpu_uploaded_bytes(const otmb_mgpu *mg);
int32_t otmb_mgpu_facefluxes(otmb_mgpu *mg, const void *umo, const void *vmo, int32_t src_is_f32, const uint8_t *wet3d,
                             double fill, int64_t nx, int64_t ny, int64_t nz, int32_t topology, double *const phi[6]);
int32_t otmb_mgpu_transportmatrix_plan(otmb_mgpu *mg, const otmb_tm_args *args, int64_t nnz[5]);
int32_t otmb_mgpu_transportmatrix_fetch(otmb_mgpu *mg, int64_t *const colptr[5], int64_t *const rowval[5],
                                        double *const nzval[5], int64_t nnz_out[5]);
/* The same build in ONE call, pipelined over the slabs (speed only; the same five matrices bit for bit): the caller hands output arrays
 * of `capacity[m]` entries -- 7N, 7N, 5N, 3N, 3N always suffice (src/matrixbuilding.jl:244-296, :348-415, :450-477: a column of Tadv / T
 * holds at most the cell and its six neighbours, of TκH five, of TκVML / TκVdeep three) -- and gets the counts back in nnz_out; a host
 * binding wraps the first nnz_out[m] entries (Julia: unsafe_wrap with that length).  Slab s uploads its levels while slab s - 1 counts,
 * fills and copies its columns home, so the PCIe link carries both directions at once, which the two-phase protocol cannot do (every
 * upload precedes the count there, every download follows it): slabs that share a device take the link in turn for their uploads,
 * and a slab's column offsets are the running sums of the FINAL counts above it.  Meant for device_ids = {d, d, d, d}: four to eight
 * slabs on ONE device hide most of a time slice's upload behind its download; with one slab per device it saves the
 * nnz round trip.  OTMB_ERR_CAPACITY when an array is too small.                                                          */
int32_t otmb_mgpu_transportmatrix_onepass(otmb_mgpu *mg, const otmb_tm_args *args, int64_t *const colptr[5], int64_t *const rowval[5],
                                          double *const nzval[5], const int64_t capacity[5], int64_t nnz_out[5]);
/* Capacities that always suffice for otmb_mgpu_transportmatrix_onepass / otmb_transportmatrix_dev, from the wet mask ALONE (indices.wet3D
 * bytes; pure host arithmetic on all cores, no GPU, no context; once per grid): a column holds a row per wet neighbour of its cell (+ the
 * diagonal), whatever the fluxes are (src/velocities.jl:167-173 zeroes every flux towards land) -- so cap[OTMB_T] = cap[OTMB_TADV] = the union
 * pattern's count, cap[OTMB_TKH] and cap[OTMB_TKVDEEP] the horizontal / vertical neighbour counts (exact but for coinciding row-mates on
 * the tripolar seam), cap[OTMB_TKVML] = cap[OTMB_TKVDEEP].  About 24.6 N on an ocean grid against the 7 + 7 + 5 + 3 + 3 = 25 N of the per-column
 * maxima: what varies from time slice to time slice (Tadv: 3.9 N, TκVML: 0.6 N) is bounded by the host layers from the PREVIOUS slice's counts. */
int32_t otmb_static_capacity(const uint8_t *wet3d, int64_t nx, int64_t ny, int64_t nz, int32_t topology, int64_t cap[5]);

/* ---- makegridmetrics(; areacello, volcello, lon, lat, lev, lon_vertices, lat_vertices) -- the array work of
 *      src/gridcellgeometry.jl:265-311 (device pointers; vertex permutation :158-178 and topology detection
 *      src/gridtopology.jl:33-53 are host decisions passed in as `perm` (0-based) and `topology`).
 * volcello (nx,ny,nz), areacello (nx,ny) with `missing` as NaN; fill_area/fill_vol: their _FillValue (NaN if none);
 * lon, lat (nx,ny); lon_vertices, lat_vertices (4,nx,ny) as given.  Outputs: area2d, v3d, thkcello, z3d and the
 * three groups of four (nx,ny) arrays in OTMB_DIR_* order: edge_length_2D, distance_to_edge_2D,
 * distance_to_neighbour_2D.  Transcendentals use the device math library: ~1e-15 relative to a host build. */
int32_t otmb_makegridmetrics_dev(otmb_ctx *ctx, const double *volcello, const double *areacello, double fill_area,
                                 double fill_vol, const double *lon, const double *lat, const double *lon_vertices,
                                 const double *lat_vertices, const int32_t perm[4], int64_t nx, int64_t ny, int64_t nz,
                                 int32_t topology, double *area2d, double *v3d, double *thkcello, double *z3d,
                                 double *const edge_length[4], double *const dist_edge[4], double *const dist_nbr[4]);
/* the same on host arrays (what a Julia / C caller has): inputs up, the seventeen derived arrays back; blocking */
int32_t otmb_makegridmetrics(otmb_ctx *ctx, const double *volcello, const double *areacello, double fill_area, double fill_vol,
                             const double *lon, const double *lat, const double *lon_vertices, const double *lat_vertices,
                             const int32_t perm[4], int64_t nx, int64_t ny, int64_t nz, int32_t topology, double *area2d, double *v3d,
                             double *thkcello, double *z3d, double *const edge_length[4], double *const dist_edge[4],
                             double *const dist_nbr[4]);

/* ---- bolus_GM_velocity(ρ, gridmetrics, indices; κGM = 600, maxslope = 0.01) -- src/RediGM.jl:46-79 with
 *      globalverticalfacetriadderivative (src/triads.jl:84-146) and globalverticaldyadderivative
 *      (src/dyads.jl:38-78).  Experimental in the reference, not connected to transportmatrix, and unpinned by
 *      any reference test.  rho, z3d (gridmetrics.Z3D): (nx,ny,nz); wet3d: indices.wet3D bytes; dist_east /
 *      dist_north: gridmetrics.distance_to_neighbour_2D[:east] / [:north].  u, v: (nx,ny,nz), NaN off Lwet.
 *      A bipolar topology is an error (the reference evaluates k₋₁(nothing) at j == ny).               */
int32_t otmb_bolus_gm_velocity_dev(otmb_ctx *ctx, const double *rho, const double *z3d, const uint8_t *wet3d,
                                   const double *dist_east, const double *dist_north, int64_t nx, int64_t ny,
                                   int64_t nz, int32_t topology, double kappa_gm, double maxslope, double *u, double *v);
int32_t otmb_bolus_gm_velocity(otmb_ctx *ctx, const double *rho, const double *z3d, const uint8_t *wet3d,
                               const double *dist_east, const double *dist_north, int64_t nx, int64_t ny, int64_t nz,
                               int32_t topology, double kappa_gm, double maxslope, double *u, double *v);

/* ---- the reference's two-step formulation as a general (non-fused) device path -------------------------
 * otmb_sparse_entries_*: the COO generators in the reference's emission order -- which = 0
 *   advection_operator_sparse_entries (src/matrixbuilding.jl:221-299), 1 horizontal_diffusion_… (:337-418),
 *   2 vertical_diffusion_… with the mixed-layer mask (:438-479, Ω of :85), 3 the same with Ω = all (:109).
 *   plan -> number of triplets (and the reference's errors), fill -> I, J, V (device arrays of that length).
 * otmb_sparse_*: SparseArrays.sparse(I, J, V, m, n) as called at :41,63,92,116 -- duplicates summed in input
 *   order, explicit zeros kept, rows ascending per column.  plan -> nnz, fill -> colptr (n+1), rowval, nzval.
 * Device pointers; one plan/fill pair at a time per context.                                             */
int32_t otmb_sparse_entries_plan_dev(otmb_ctx *ctx, int32_t which, const otmb_tm_args *args, int64_t *len);
int32_t otmb_sparse_entries_fill_dev(otmb_ctx *ctx, int64_t *I, int64_t *J, double *V);
int32_t otmb_sparse_plan_dev(otmb_ctx *ctx, const int64_t *I, const int64_t *J, const double *V, int64_t len, int64_t m,
                             int64_t n, int64_t *nnz);
int32_t otmb_sparse_fill_dev(otmb_ctx *ctx, int64_t *colptr, int64_t *rowval, double *nzval);

/* ---- A + B for SparseMatrixCSC{Float64,Int64} -- SparseArrays' map(+, A, B), the `+` of
 *      src/matrixbuilding.jl:147 used when the caller passes precomputed operators (:133-143): per column a
 *      sorted merge, a missing operand counts as +0.0, results that are exactly zero are not stored.
 * _dev: device pointers, two-phase (plan -> nnz, fill).  otmb_spadd: host pointers, Ci/Cx capacity nnz(A)+nnz(B). */
int32_t otmb_spadd_plan_dev(otmb_ctx *ctx, int64_t n, const int64_t *Ap, const int64_t *Ai, const double *Ax,
                            const int64_t *Bp, const int64_t *Bi, const double *Bx, int64_t *nnz_out);
int32_t otmb_spadd_fill_dev(otmb_ctx *ctx, int64_t n, const int64_t *Ap, const int64_t *Ai, const double *Ax,
                            const int64_t *Bp, const int64_t *Bi, const double *Bx, int64_t *Cp, int64_t *Ci, double *Cx);
int32_t otmb_spadd(otmb_ctx *ctx, int64_t n, const int64_t *Ap, const int64_t *Ai, const double *Ax, const int64_t *Bp,
                   const int64_t *Bi, const double *Bx, int64_t *Cp, int64_t *Ci, double *Cx, int64_t *nnz_out);

/* ---- buildTsink: the settling operator S of particles that sink through the water column at a speed w >= 0 (m/s, positive downward),
 *      ∂x/∂t + (T + S)·x = …  No function of the reference builds it: the contract below is this library's own, written in the style of
 *      vertical_diffusion_operator_sparse_entries (src/matrixbuilding.jl:438-479) and restated in numpy by tests/sink_ref.py.
 * For every wet cell c at (i, j, k), ascending in wet order: a = area2d[i, j], w_c = the speed at the BOTTOM face of c, b = the wet cell at
 *      (i, j, k + 1) if there is one.  Entry (c, c) = (w_c * a) / v3d[c]; if b exists, entry (b, c) = -((w_c * a) / v3d[b]).  One IEEE
 *      operation per step, no FMA.  closed != 0 (a closed seafloor): a cell without a wet cell below stores (c, c) = +0.0; closed == 0: it
 *      stores the value above, and what leaves through the seafloor is buried.
 * The pattern is a grid constant under both options: nnz = n_wet + the wet cells with a wet cell below; CSC with ascending rows (b > c in wet
 *      order), every diagonal entry stored.  Its entries are among those TκVdeep stores, so the pattern lies inside T's: otmb_op_add_matrix.
 * w by w_form: 0 the scalar w_scalar (w unused); 1 w[nz], the bottom face of each level; 2 w[nx*ny*nz], the bottom face of each cell.  The
 *      three give the same bits where they agree.  w is read on wet cells only (garbage on land does not matter).  A negative, NaN or
 *      infinite w on the bottom face of a wet cell, n_wet or a size below zero, another w_form: OTMB_ERR_INVALID_ARG; a NaN value in the
 *      result (from the metrics): OTMB_ERR_TSINK_NAN; lwet / lwet3d that are not makeindices' (each index is checked before anything is read
 *      through it): OTMB_ERR_NONCANONICAL_INDICES; nnz > cap: OTMB_ERR_CAPACITY.  *nnz (host memory) is written whenever the checks on w,
 *      the result and the indices passed.  Nothing is written to colptr / rowval / nzval unless the call returns OTMB_OK.
 * colptr: n_wet + 1; rowval, nzval: capacity cap entries (2 * n_wet always suffices).
 * otmb_build_sink_dev: device pointers, on the context's stream (the call waits for its own checks).  otmb_build_sink: host pointers. */
int32_t otmb_build_sink_dev(otmb_ctx *ctx, int32_t w_form, double w_scalar, const double *w, const double *v3d, const double *area2d,
                            const int64_t *lwet3d, const int64_t *lwet, int64_t n_wet, int64_t nx, int64_t ny, int64_t nz, int32_t closed,
                            int64_t *colptr, int64_t *rowval, double *nzval, int64_t cap, int64_t *nnz);
int32_t otmb_build_sink(otmb_ctx *ctx, int32_t w_form, double w_scalar, const double *w, const double *v3d, const double *area2d,
                        const int64_t *lwet3d, const int64_t *lwet, int64_t n_wet, int64_t nx, int64_t ny, int64_t nz, int32_t closed,
                        int64_t *colptr, int64_t *rowval, double *nzval, int64_t cap, int64_t *nnz);

/* ---- lump_and_spray(wet3D, vol, T, mask = trues(size(wet3D)); di = 2, dj = 2, dk = 1) -- src/extratools.jl:38-119:
 *      the coarsening operators LUMP (Nc x N, volume weighted: LUMP * x is the coarse vector), SPRAY (N x Nc, ones:
 *      LUMP * T * SPRAY is the coarse operator) and the coarse volumes vol_c.  Cells are lumped in di x dj x dk blocks,
 *      inside `mask` only, never across cells that T's pattern does not connect (connected components of the block,
 *      Graphs.connected_components; T's pattern must be symmetric inside every block like Graphs.SimpleGraph demands:
 *      OTMB_ERR_ASYMMETRIC_PATTERN otherwise -- e.g. an advection-only operator).  Only the PATTERN of T is read.
 * _dev (device pointers, two-phase): plan takes wet3d / lwet3d / lwet / n_wet as makeindices returns them, mask (bytes,
 *   NULL = all true) and T's colptr / rowval; it returns Nc.  fill writes LUMP (colptr N+1 = 1..N+1: one entry per column,
 *   rowval N, nzval N), SPRAY (colptr Nc+1, rowval N, nzval N) and vol_c (Nc).  Limits: nx <= 4900, di*dj*dk <= 4096.
 * otmb_lump_and_spray (host pointers, what the Julia shim calls): outputs with capacity N (N+1 for spray_colptr); the
 *   trivial arrays (LUMP's colptr, SPRAY's ones) are left to the caller.                                            */
int32_t otmb_lump_and_spray_plan_dev(otmb_ctx *ctx, const uint8_t *wet3d, const uint8_t *mask, const int64_t *lwet3d,
                                     const int64_t *lwet, int64_t n_wet, int64_t nx, int64_t ny, int64_t nz,
                                     const int64_t *t_colptr, const int64_t *t_rowval, int64_t di, int64_t dj, int64_t dk,
                                     int64_t *n_coarse);
int32_t otmb_lump_and_spray_fill_dev(otmb_ctx *ctx, const double *vol, int64_t *lump_colptr, int64_t *lump_rowval,
                                     double *lump_nzval, int64_t *spray_colptr, int64_t *spray_rowval, double *spray_nzval,
                                     double *vol_c);
int32_t otmb_lump_and_spray(otmb_ctx *ctx, const uint8_t *wet3d, const uint8_t *mask, int64_t nx, int64_t ny, int64_t nz,
                            const double *vol, int64_t n_wet, const int64_t *t_colptr, const int64_t *t_rowval, int64_t di,
                            int64_t dj, int64_t dk, int64_t *lump_rowval, double *lump_nzval, int64_t *spray_colptr,
                            int64_t *spray_rowval, double *vol_c, int64_t *n_coarse);

/* ---- C = LUMP * T * SPRAY, the coarse operator of lump_and_spray's docstring (src/extratools.jl:14-16, test/local_full.jl:161):
 *      SparseArrays' (LUMP * T) * SPRAY bit for bit (the 3-argument `*` multiplies left to right for these shapes; each `*` is
 *      spmatmul: per column, the first touch of a row copies, later touches add in stored order, every touched row is stored,
 *      exact zeros included).  A (LUMP): m x N with at most one stored entry per column; B (T or any operator): N x M; S (SPRAY):
 *      M x n; all SparseMatrixCSC{Float64,Int64} arrays, 1-based, rows ascending inside a column.  A LUMP column with two or more
 *      entries, a colptr that is not ascending inside [1, nnz + 1] or a row index out of range: OTMB_ERR_INVALID_ARG (checked
 *      before anything is read through it).
 * _dev: device pointers, two-phase (plan -> nnz of C, fill -> Cp (n+1), Ci, Cx (nnz)); one plan/fill pair per context at a time,
 *   the inputs must stay alive and unchanged until the fill.
 * otmb_coarsen_plan (host pointers, what the Julia shim calls): uploads the three matrices (every call) and plans;
 *   otmb_coarsen_fetch fills and downloads.                                                                                  */
int32_t otmb_coarsen_plan_dev(otmb_ctx *ctx, int64_t m, int64_t N, const int64_t *Ap, const int64_t *Ai, const double *Ax, int64_t M,
                              const int64_t *Bp, const int64_t *Bi, const double *Bx, int64_t n, const int64_t *Sp, const int64_t *Si,
                              const double *Sx, int64_t *nnz);
int32_t otmb_coarsen_fill_dev(otmb_ctx *ctx, int64_t *Cp, int64_t *Ci, double *Cx);
int32_t otmb_coarsen_plan(otmb_ctx *ctx, int64_t m, int64_t N, const int64_t *Ap, const int64_t *Ai, const double *Ax, int64_t M,
                          const int64_t *Bp, const int64_t *Bi, const double *Bx, int64_t n, const int64_t *Sp, const int64_t *Si,
                          const double *Sx, int64_t *nnz);
int32_t otmb_coarsen_fetch(otmb_ctx *ctx, int64_t *Cp, int64_t *Ci, double *Cx);

/* ---- A resident sparse operator: Y = α·A·X + β·Y and Y = α·Aᵀ·X + β·Y on the device -- what the reference's consumer checks compute
 *      with the matrices it builds (test/local_full.jl:96-107: norm(T * e1), norm(T' * v)) and what a tracer simulation steps with
 *      (README: ∂x/∂t + T x = …).  Bit for bit SparseArrays' 5-argument mul! of Julia 1.10 (Project.toml: julia = "1.10"):
 *        β step first: β == 0 fills Y with +0.0, β == 1 leaves it, otherwise Y .*= β;
 *        A·X: for each column c of X, for col = 1..n, αxj = X[col,c] * α, then Y[rowval[j],c] += nzval[j] * αxj in stored order;
 *        Aᵀ·X: tmp = +0.0, tmp += nzval[j] * X[rowval[j],c] in stored order, then Y[col,c] += tmp * α.
 *      No FMA.  A: m x n SparseMatrixCSC{Float64,Int64} arrays (1-based; rows need not be sorted or distinct inside a column); X, Y:
 *      column-major Float64 with k >= 1 columns and leading dimensions ldx / ldy >= their rows.  `A * x` and `A' * v` are alpha = 1,
 *      beta = 0.
 * otmb_op_create_dev (device pointers, copied on the device) / otmb_op_create (host pointers, uploaded): checks colptr[1] == 1, colptr
 *   non-decreasing, every rowval in 1:m (OTMB_ERR_INVALID_ARG before anything is read through them), then plans the row layout of A·X.
 *   The operator owns copies of everything: no caller array is read after a call returns.  An opaque handle, not keyed to addresses.
 * otmb_op_set_values[_dev]: new nzval (nnz of them) for the same pattern.
 * otmb_op_mul_dev: X, Y device pointers, enqueued on the context's stream without a host sync.  otmb_op_mul: host pointers (uploads X,
 *   and Y when beta != 0; downloads Y; the rows between ld and the row count are neither read nor written).
 * Null arguments, k < 1, ldx / ldy too small: OTMB_ERR_INVALID_ARG with a message (otmb_last_error of the operator's context); the
 *   operator stays usable.  An operator uses its context's stream and messages: destroy operators before their context.
 *   otmb_op_destroy touches no context (a finalizer may run it after the context is gone); it waits for the device.            */
typedef struct otmb_op otmb_op;
int32_t otmb_op_create_dev(otmb_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, otmb_op **out);
int32_t otmb_op_create(otmb_ctx *ctx, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, otmb_op **out);
int32_t otmb_op_set_values_dev(otmb_op *op, const double *nzval, int64_t nnz);
int32_t otmb_op_set_values(otmb_op *op, const double *nzval, int64_t nnz);
int32_t otmb_op_mul_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, double alpha, double beta);
int32_t otmb_op_mul(otmb_op *op, int32_t adjoint, int64_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, double alpha, double beta);
int32_t otmb_op_info(const otmb_op *op, int64_t *m, int64_t *n, int64_t *nnz);
void otmb_op_destroy(otmb_op *op);

/* ---- M·X = B on the device with M = σ·I + diag(d) + A (adjoint: σ·I + diag(d) + Aᵀ), A the operator's matrix (square, otherwise
 *      OTMB_ERR_INVALID_ARG): the `\` of the reference's ideal-age problem, Γ_c = (T_c + M_c) \ (LUMP * ones(N)) (test/local_full.jl:151-188),
 *      a steady state, or an implicit time step (I/δt + T)·x⁺ = x/δt + s.  The operator is not modified: otmb_op_set_values then another solve
 *      is the time loop.
 *      Method: BiCGStab, right-preconditioned with P = diag(M) (Jacobi); diag(M)[i] = σ + d[i] plus the stored entries (i, i) of A in storage
 *      order.  An entry that is zero or not finite: OTMB_ERR_SINGULAR_PRECONDITIONER before anything is iterated or written, the message names
 *      the first such index.  d: n values or NULL (zero).  B, X: column-major n x k with leading dimensions ldb, ldx >= n (rows beyond n are
 *      neither read nor written).  use_x0 = 0: X is not read, the start is zero.  rtol > 0, maxiter >= 0.
 *      The k columns advance together, each with its own scalars; a column that has stopped is frozen.  Every sum is taken in a fixed order
 *      that depends on n alone (no floating-point atomics): the same call gives the same bits, and column c of a k-column solve has the bits
 *      of that column solved alone.
 *      Stopping, per column: when the recursive residual reaches ‖r‖₂ <= rtol·‖b‖₂ the true residual b - M·x is computed; the column stops as
 *      converged when that passes and otherwise goes on from the true residual with r̂ = r.  So it does when ρ = r̂·r is no more than the
 *      rounding error of its own sum (|ρ| <= 2^-52·‖r̂‖₂·‖r‖₂, zero included): with B = 1 and a mass-conserving A, the first r̂ is a left
 *      eigenvector of M and ρ is noise.  b = 0: x = 0, zero iterations, converged.  Otherwise it stops with OTMB_SOLVE_MAXITER (maxiter
 *      iterations done), OTMB_SOLVE_BREAKDOWN (r̂·v, t·t or ω is zero) or OTMB_SOLVE_NONFINITE (a scalar is NaN or Inf: NaN in B, for
 *      instance); X then holds the LAST iterate (not the best one).
 *      iters[k], relres[k], reason[k] (HOST arrays in both variants; the call waits for the device): completed iterations, the residual
 *      ratio ‖r‖₂/‖b‖₂ of the column's last residual evaluation -- the explicitly computed b - M·x when the column stopped on one (every
 *      converged column, a start that already passes, maxiter reached on a failed check), the recursive one otherwise -- and an
 *      otmb_solve_reason.  They are filled whenever the call returns OTMB_OK or OTMB_ERR_NOT_CONVERGED; the latter when any column's reason is
 *      not OTMB_SOLVE_CONVERGED (X and the three arrays are valid: not converged is an answer, not a failure of the call).
 * otmb_op_solve_dev: d, B, X device pointers, on the context's stream.  otmb_op_solve: host pointers, staged like otmb_op_mul.      */
typedef enum { OTMB_SOLVE_CONVERGED = 0, OTMB_SOLVE_MAXITER = 1, OTMB_SOLVE_BREAKDOWN = 2, OTMB_SOLVE_NONFINITE = 3 } otmb_solve_reason;
int32_t otmb_op_solve_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X,
                          int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason);
int32_t otmb_op_solve(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X, int64_t ldx,
                      int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason);

/* ---- A second preconditioner for the solver: P = the part of M on caller-given LINES (block Jacobi whose blocks are tridiagonal, solved by
 *      the Thomas recurrence).  A line is a chain of unknowns; for the transport matrices it is one water column, top to bottom, which puts the
 *      vertical coupling (TκVML: ~1e-3 s⁻¹ against horizontal rates of ~1e-7 s⁻¹) inside the preconditioner: the implicit vertical solve of
 *      an ocean model.  On the time-stepping systems (σ = 1/month, 1/year) this takes one and a half to three orders of magnitude fewer
 *      iterations than Jacobi; each iteration costs two line sweeps more.
 * otmb_op_set_lines_dev (device pointer) / otmb_op_set_lines (host pointer): next[n] (Int64, 1-based like rowval): next[i] is the successor of
 *      unknown i on its line, or 0 for none.  NULL clears the lines.  The operator must be square.  Checked on the device before anything is
 *      kept, each with OTMB_ERR_INVALID_ARG and the first offending 1-based index in the message (the operator keeps the lines it had; only a failed device allocation for the new tables, OTMB_ERR_ALLOC, leaves it with none):
 *        every entry is 0 or satisfies i < next[i] <= n (so no cycle is possible; wet-cell numbering satisfies it: the cell below has the
 *        larger index);  no index is the successor of two unknowns.
 *      Lines belong to the pattern: they survive otmb_op_set_values.  The operator keeps O(n) Int32 tables whatever the lines' lengths.
 * The preconditioner, as a contract (tests/solve_lines_ref.py restates it bit for bit), for the non-adjoint system with j = next[i]:
 *        a_i = Jacobi's diag(M)[i]: σ + d[i], then the stored entries (i, i) in storage order;
 *        u_i = the stored entries (i, j) of A, l_i = the stored entries (j, i) of A, each folded from +0.0 in storage order;
 *        the adjoint swaps u and l;  all three are taken from the operator's values on each call.
 *      Factorisation, head to tail: piv_head = a_head;  m_j = l_i / piv_i;  piv_j = a_j - m_j·u_i.  No pivoting, no FMA.  A pivot that is zero
 *      or not finite: OTMB_ERR_SINGULAR_PRECONDITIONER before anything is iterated or written, the message names the smallest such index
 *      (the diagonal itself is not checked: only the pivots divide).
 *      z = P⁻¹·y:  forward y'_head = y_head, y'_j = y_j - m_j·y'_i;  backward z_tail = y'_tail / piv_tail, z_i = (y'_i - u_i·z_j) / piv_i.
 *      A line is one sequential recurrence: the result is deterministic and a column's result does not depend on the other columns.  With
 *      no successor anywhere (next all zero) z = y ./ diag(M), the bits of the Jacobi preconditioner.
 * otmb_op_solve_pc[_dev]: otmb_op_solve[_dev] with the preconditioner named (otmb_op_solve[_dev] is this call with OTMB_PRECOND_JACOBI).
 *      OTMB_PRECOND_LINES on an operator without lines, or any other value: OTMB_ERR_INVALID_ARG.  Everything said of otmb_op_solve holds.
 * otmb_op_precond[_dev]: Z = P⁻¹·Y alone, for a caller with a Krylov method of their own.  Y, Z: column-major n x k, ldy, ldz >= n (rows
 *      beyond n are neither read nor written); Z may be Y.  _dev: device pointers, on the context's stream.                              */
typedef enum { OTMB_PRECOND_JACOBI = 0, OTMB_PRECOND_LINES = 1 } otmb_precond;
int32_t otmb_op_set_lines_dev(otmb_op *op, const int64_t *next);
int32_t otmb_op_set_lines(otmb_op *op, const int64_t *next);
int32_t otmb_op_solve_pc_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X,
                             int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason,
                             int32_t precond);
int32_t otmb_op_solve_pc(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X,
                         int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason,
                         int32_t precond);
int32_t otmb_op_precond_dev(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *d, double sigma, const double *Y,
                            int64_t ldy, double *Z, int64_t ldz);
int32_t otmb_op_precond(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *d, double sigma, const double *Y, int64_t ldy,
                        double *Z, int64_t ldz);

/* ---- Value slots: several value sets over ONE pattern, resident together -- a year of monthly transport matrices, cycled by a time loop
 *      without uploading or scattering anything again.  The operator holds nslots copies of its two value arrays (nzval of the CSC copy and
 *      the row layout's values: 8·nnz bytes and 8·(nnz + the slices' padding) bytes per slot); the pattern, the index arrays and the lines
 *      are shared.  A fresh operator has one slot, slot 0, selected.
 * otmb_op_set_slots: nslots >= 1.  Growing keeps the existing slots; every new slot is a device copy of the SELECTED slot's values (never
 *      undefined).  Shrinking frees the slots from nslots on (it waits for the stream); when the selected slot goes, slot 0 is selected.
 *      A failed allocation (OTMB_ERR_ALLOC) leaves the operator with the slots it had.
 * otmb_op_set_values_slot[_dev]: otmb_op_set_values[_dev] into slot `slot` (0-based), whichever is selected.
 *      otmb_op_set_values[_dev] writes the selected slot.
 * otmb_op_select_slot: a pointer switch -- nothing is enqueued, no data moves.  otmb_op_mul*, otmb_op_solve*, otmb_op_precond* called
 *      afterwards read that slot (work already enqueued keeps the slot it was enqueued with).
 * otmb_op_slots: the number of slots and the selected one (either pointer may be NULL).
 * A slot outside 0..nslots-1, nslots < 1 or an nnz that is not the operator's: OTMB_ERR_INVALID_ARG with a message; the operator stays usable. */
int32_t otmb_op_set_slots(otmb_op *op, int64_t nslots);
int32_t otmb_op_set_values_slot_dev(otmb_op *op, int64_t slot, const double *nzval, int64_t nnz);
int32_t otmb_op_set_values_slot(otmb_op *op, int64_t slot, const double *nzval, int64_t nnz);
int32_t otmb_op_select_slot(otmb_op *op, int64_t slot);
int32_t otmb_op_slots(const otmb_op *op, int64_t *nslots, int64_t *selected);

/* ---- otmb_op_combine_slots[_dev]: slot dst = Σ_s w[s]·(slot s), on the device -- the annual mean of a year of monthly matrices without
 *      downloading one of them.  w: HOST array of nslots weights (both variants); dst: a slot, which may be one of the sources.
 * In bits: for every stored entry, the slots with w[s] != 0 in ascending s; acc = w[s]·v_s for the first of them, acc = acc + w[s]·v_s for
 *      each of the rest (one multiplication, one addition, no FMA); all w[s] zero: +0.0.  Both value arrays of slot dst are written with the
 *      same arithmetic, elementwise (the row layout's padding included, which no product reads); the other slots and the selection are not
 *      touched.  otmb_op_mul*, otmb_op_solve* on slot dst afterwards have the bits of otmb_op_set_values_slot with that fold of the nzvals.
 * A weight that is not finite, dst outside 0..nslots-1 or w == NULL: OTMB_ERR_INVALID_ARG before anything is written; the operator stays
 *      usable.  otmb_op_combine_slots_dev enqueues on the context's stream; otmb_op_combine_slots waits for it.                          */
int32_t otmb_op_combine_slots_dev(otmb_op *op, const double *w, int64_t dst);
int32_t otmb_op_combine_slots(otmb_op *op, const double *w, int64_t dst);

/* ---- otmb_op_add_matrix[_dev]: slot = slot + α·B in place, for a matrix B whose pattern lies inside the operator's -- the settling operator
 *      of otmb_build_sink added to a year of monthly T, or a diffusivity retuned without a rebuild (T is linear in κH, κVML and κVdeep:
 *      B = TκH, α = κ'/κ - 1).  The pattern, the layouts, the lines and every other slot stay as they are.
 * B: m x n CSC arrays (Int64, 1-based) of the operator's shape, rows in any order.  Checked before anything is read through them, each
 *      OTMB_ERR_INVALID_ARG: m, n are the operator's, colptr[1] == 1, colptr non-decreasing, every row in 1..m.
 * Matching: the stored entry (r, c) of B belongs to the FIRST stored entry (r, c) of the operator's column c in stored order (an operator may
 *      store unsorted and duplicate rows: later duplicates are never written).  An entry of B without a partner:
 *      OTMB_ERR_PATTERN_NOT_CONTAINED, the message names the first such entry in B's stored order (its 1-based position, row and column).
 *      Match first, write afterwards: after any error every slot has the bits it had.
 * In bits, for each requested slot, each matched position p and the entries e of B that belong to it, in B's stored order:
 *      nz[p] = nz[p] + (α * B[e]), one multiplication and one addition, no FMA; the row layout's copy of p receives the same bits.  Entries B
 *      does not name are not rewritten.  α == 0 (and an empty B, and nsel == 0) checks everything and writes nothing.
 * slots: HOST array (both variants) of nsel different slots in 0..nslots-1, or NULL: every slot.  α must be finite.
 * Cost: a match of Σ_c len_B(c)·len_A(c) index comparisons (columns of a transport matrix hold at most 19 entries), once per call; then one
 *      streaming launch over B's entries that updates all requested slots: a read-modify-write of nnz(B) entries in two arrays per slot.
 * A child of otmb_op_submatrix does not follow: otmb_op_take_values refreshes it.
 * otmb_op_add_matrix_dev: B in device memory, on the context's stream (the call waits for its own checks).  otmb_op_add_matrix: host pointers. */
int32_t otmb_op_add_matrix_dev(otmb_op *op, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, double alpha,
                               int64_t nsel, const int64_t *slots);
int32_t otmb_op_add_matrix(otmb_op *op, int64_t m, int64_t n, const int64_t *colptr, const int64_t *rowval, const double *nzval, double alpha,
                           int64_t nsel, const int64_t *slots);

/* ---- The operator's domain: A[rows, cols] as a new resident operator, without leaving the device -- prescribed (Dirichlet) boundary values
 *      (A_II·x_I = s_I - A_IB·x_B needs the blocks A[I, I] and A[I, B]), regional problems -- and what an operator can say of itself.
 * otmb_op_submatrix_dev (device pointers) / otmb_op_submatrix (host pointers): rows[nr], cols[nc] (Int64, 1-based like rowval), each STRICTLY
 *      ASCENDING inside 1..m / 1..n.  Checked on the device before anything is allocated for the child: a violation is OTMB_ERR_INVALID_ARG, the
 *      message names the first offending 1-based position of the list and says whether it is a row or a column.  The parent is never modified;
 *      *out is written only on success.  The child is a new, independent operator on the parent's context (destroy it like any other; the parent
 *      may be destroyed first).
 * In bits: the child is the operator otmb_op_create makes from SparseArrays' A[rows, cols] -- column j' holds the stored entries of column
 *      cols[j'] whose row is selected, IN STORED ORDER (unsorted and duplicate rows survive as they are), rows renumbered by their rank in
 *      `rows`, values copied bit for bit (NaN payloads, -0.0) -- planned by otmb_op_create_dev's own plan, so every product, solve, step and
 *      observation on it has the bits of that operator.  It has the parent's number of slots, slot s holding the parent's slot s restricted,
 *      and the parent's selection.  Lines: when the selection is PRINCIPAL (nr == nc and rows[i] == cols[i] for all i, decided on the device)
 *      and the parent has lines, the child has next'[rank(i)] = rank(next[i]) where i and next[i] are both selected and 0 elsewhere (a dropped
 *      cell cuts its line in two; the renumbering is monotone, so otmb_op_set_lines' rules are inherited), set through otmb_op_set_lines_dev;
 *      otherwise it has none.  An empty selection (nr == 0 or nc == 0) is what otmb_op_create_dev makes of the empty nr x nc matrix.
 * otmb_op_take_values: slot child_slot of a child becomes slot parent_slot of its parent, restricted -- the monthly refresh when the parent's
 *      values were rebuilt.  Device work only, ONE streaming launch enqueued on the context's stream (the child keeps its gather table; it keeps
 *      no pointer to the parent).  In bits it is otmb_op_set_values_slot_dev(child, child_slot, the gathered nzval): both value arrays of the
 *      slot are written, nothing else; the selection and the lines are untouched.  The child knows its parent by a process-wide serial number
 *      every operator gets at creation, not by its address: an operator that is not the parent (one created at a destroyed parent's address
 *      included), one on another context, a `child` that no otmb_op_submatrix made, and a slot outside either operator's 0..nslots-1 (there is no
 *      "selected slot" here) are each OTMB_ERR_INVALID_ARG with nothing written.  The parent's pattern cannot change, so a child stays valid
 *      for as long as the parent lives, whatever is done to the parent's values, slots and lines.
 * otmb_op_fetch_dev (device pointers, enqueued) / otmb_op_fetch (host pointers, waits): the operator's matrix as otmb_op_create took it: colptr
 *      (n + 1), rowval (nnz, 1-based: widened back from the operator's Int32 copy) and nzval (nnz) of slot `slot`, -1: the selected slot.  Any of
 *      the three may be NULL.  fetch after create returns the arrays given, bit for bit; sizes: otmb_op_info.
 * otmb_op_get_lines_dev (next: device pointer) / otmb_op_get_lines (host pointer): *has_lines (a HOST int32 in both variants; may be NULL) = 1
 *      and next[n] in otmb_op_set_lines' convention when the operator has lines; *has_lines = 0 and next not written when it has none.  next may
 *      be NULL (the question alone).
 * Every argument error leaves every operator involved usable.  Not built: permutations and repeated indices (the lists must ascend strictly;
 *      a caller who needs an order permutes the vectors), a submatrix of a submatrix refreshed from the grandparent (take_values takes the
 *      direct parent only), and a child that follows a parent's later otmb_op_set_slots (a slot it lacks is refused; otmb_op_set_slots on the
 *      child, then take_values, fills it).                                                                                              */
int32_t otmb_op_submatrix_dev(otmb_op *parent, int64_t nr, const int64_t *rows, int64_t nc, const int64_t *cols, otmb_op **out);
int32_t otmb_op_submatrix(otmb_op *parent, int64_t nr, const int64_t *rows, int64_t nc, const int64_t *cols, otmb_op **out);
int32_t otmb_op_take_values(otmb_op *child, const otmb_op *parent, int64_t parent_slot, int64_t child_slot);
int32_t otmb_op_fetch_dev(const otmb_op *op, int64_t slot, int64_t *colptr, int64_t *rowval, double *nzval);
int32_t otmb_op_fetch(const otmb_op *op, int64_t slot, int64_t *colptr, int64_t *rowval, double *nzval);
int32_t otmb_op_get_lines_dev(const otmb_op *op, int64_t *next, int32_t *has_lines);
int32_t otmb_op_get_lines(const otmb_op *op, int64_t *next, int32_t *has_lines);

/* ---- θ-steps of ∂x/∂t + (diag(d) + A)·x = s over the slots: X (n x k, in and out) advances through nsteps steps of length dt, step t
 *      (0-based) with the matrix A of slot (first_slot + t) mod nslots (adjoint: Aᵀ).  S: the source, n x k with leading dimension lds, or NULL
 *      (zero); d: n values or NULL.  dt > 0 and finite, 0 < theta <= 1 (1: implicit Euler, 0.5: Crank-Nicolson), nsteps >= 0,
 *      0 <= first_slot < nslots, the operator square, rtol > 0, maxiter >= 0, precond as in otmb_op_solve_pc (OTMB_PRECOND_LINES needs lines),
 *      ldx, lds >= n, steps_done not NULL, iters / relres / reason not NULL unless nsteps == 0: otherwise OTMB_ERR_INVALID_ARG before X is
 *      touched.  The selected slot is the same after the call as before it.
 * One step, as a contract in public calls -- every state has the bits of this composition, column by column, and column c of k has the bits of
 * that column stepped alone:
 *        σ = 1 / (theta·dt): the product theta * dt, then its reciprocal;
 *        theta == 1:  b_i = σ·x_i + s_i (one multiplication, one addition);  without S: b_i = σ·x_i;
 *        theta <  1:  w = A·x as otmb_op_mul_dev(alpha = 1, beta = 0) gives it;  c = (1 - theta) / theta;  e_i = d_i·x_i + w_i (without d: w_i);
 *                     b_i = (σ·x_i + s_i/theta) - c·e_i in exactly that association (without S the s_i/theta term is absent);  no FMA;
 *        then otmb_op_solve_pc_dev(op, adjoint, k, d, σ, B, X, use_x0 = 1, rtol, maxiter, ..., precond): the previous state is the start.
 *      The right-hand side is one kernel per step (the product's fold ends in the elementwise line; theta == 1 reads no matrix).  A slot's
 *      preconditioner -- Jacobi's diagonal or the line factorisation -- is computed on the slot's first visit of the call and reused on every
 *      later visit: d, σ, adjoint and the values are fixed inside a call, and the factorisation is deterministic, so the bits are those of
 *      separate solves.
 * Stopping: a step whose solve leaves any column not converged ends the call: OTMB_ERR_NOT_CONVERGED, *steps_done = the number of steps
 *      completed with every column converged, X = that step's last iterates.  A slot whose preconditioner is singular ends it with
 *      OTMB_ERR_SINGULAR_PRECONDITIONER on the slot's first visit: X = the state after *steps_done steps.
 *      iters, relres, reason: HOST arrays of nsteps·k entries, step-major (entry t·k + c), as otmb_op_solve reports them; written for the
 *      steps 0 .. min(*steps_done, nsteps - 1) -- after a singular preconditioner for the steps before *steps_done only -- the rest is not
 *      written.  nsteps == 0: OTMB_OK, *steps_done = 0, nothing else is touched.
 * otmb_op_step_dev: d, S, X device pointers, on the context's stream.  otmb_op_step: host pointers; X, S and d are uploaded once and X is
 *      downloaded once, however many steps.                                                                                           */
int32_t otmb_op_step_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                         const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                         int64_t *iters, double *relres, int32_t *reason);
int32_t otmb_op_step(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                     const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                     int64_t *iters, double *relres, int32_t *reason);

/* ---- Observations of a state, and a record along the steps: obs[j, c] = Σ_i W[i, j]·X[i, c] for q observers -- the columns of W, n x q with
 *      leading dimension ldw >= n: cell volumes for an inventory, a unit vector for a station, a region's weights -- and k tracers, X n x k
 *      with ldx >= n, n the operator's columns.  obs: column-major q x k, entry j + q·c.  Rows beyond n are not read.
 * The order of every sum is fixed by n alone and is a contract (tests/observe_ref.py restates it): the same call gives the same bits, and entry
 *      (j, c) has the bits that observer and that tracer have alone, whatever q and k.
 *        A workgroup has 256 lanes and takes 2048 rows; lane t of workgroup g takes the row pairs starting at rows 2·(1024·g + t + 256·p),
 *        p = 0..3, in that order.  Within a lane acc starts at +0.0 and takes acc = acc + W[i,j]·X[i,c] for the pair's first row i, then for
 *        row i + 1 if it is below n: one multiplication, one addition, no FMA.
 *        The workgroup's sum: in each wave of 64 lanes xor shuffles at distances 32, 16, 8, 4, 2, 1 (x = x + the partner's x), then the four
 *        waves' sums in wave order, ((w0 + w1) + w2) + w3: one partial per entry and workgroup.
 *        An entry's partials are added in workgroup order, starting from partial 0.  n == 0: every entry is +0.0.
 *      16-byte loads are taken where the base pointer is 16-byte aligned and the leading dimension even, 8-byte loads otherwise: the same bits.
 * otmb_op_observe_dev: W, X, obs device pointers, enqueued on the context's stream.  otmb_op_observe: host pointers; W and X are staged
 *      compactly and the call waits.  q == 0: nothing is done.  W and obs must not overlap X (not checked).
 * q < 0, q > 0 with W or obs NULL or ldw < n, k < 1, ldx < n, X NULL with n > 0: OTMB_ERR_INVALID_ARG before anything is written, the message
 *      names the call; the operator stays usable.
 *
 * otmb_op_step_obs[_dev]: otmb_op_step[_dev] -- the same 19 arguments, the same states, reports and stopping, bit for bit -- with a record:
 *      after step t's solve has returned with every column converged, the pass above runs on the state where the solve left it.
 *        obs: column-major (q, k, nsteps); obs[j + q·(c + k·t)] is observer j of tracer c after step t.
 *        tw, Xbar (both or neither; NULL: no mean): tw holds nsteps finite weights, a HOST pointer in both variants; Xbar is n x k with
 *        leading dimension ldm >= n.  After step t, in the same pass and from the same loads of X:  Xbar[i,c] = Xbar[i,c] + tw[t]·X[i,c], the
 *        product first, then the sum (no FMA); at t = 0 the old value is +0.0, not what Xbar held.  With tw[t] = 1 / nsteps over one cycle
 *        from the state otmb_op_periodic returned, Xbar is the cycle's mean state.
 *      q == 0 runs no reduction, no mean stores nothing; with q == 0 and tw == NULL the call is otmb_op_step[_dev], which is this loop.
 *      A step that does not converge, or a singular preconditioner, ends the call as it ends otmb_op_step: the blocks t >= *steps_done of obs
 *      are left as passed in, and Xbar holds the fold over the completed steps (untouched when there were none).  n == 0: every observation
 *      is +0.0.  nsteps == 0: nothing is touched.
 *      otmb_op_step_obs_dev: d, S, X, W, obs, Xbar device pointers; the fold writes obs on the device and no wait for the host is added per
 *      step.  otmb_op_step_obs: host pointers; W is staged once, and the written blocks of obs and Xbar come home once, when X does.
 *      Refused with OTMB_ERR_INVALID_ARG before anything is written, after otmb_op_step's own checks, the message naming otmb_op_step_obs:
 *      q < 0; q > 0 with W or obs NULL or ldw < n; one of tw / Xbar without the other; a weight that is not finite; ldm < n.
 *      W, obs and Xbar must not overlap X or each other (not checked).                                                                  */
int32_t otmb_op_observe_dev(otmb_op *op, int64_t k, int64_t q, const double *W, int64_t ldw, const double *X, int64_t ldx, double *obs);
int32_t otmb_op_observe(otmb_op *op, int64_t k, int64_t q, const double *W, int64_t ldw, const double *X, int64_t ldx, double *obs);
int32_t otmb_op_step_obs_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                             const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                             int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                             double *Xbar, int64_t ldm);
int32_t otmb_op_step_obs(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t nsteps, int64_t first_slot,
                         const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                         int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                         double *Xbar, int64_t ldm);

/* ---- The periodic (cyclo-stationary) state of the stepped cycle: x = F(x), F(x) = otmb_op_step_dev over ncycle >= 1 steps from first_slot
 *      with the source S (ncycle need not be a multiple of the slot count).  F is affine: F(x) = Φ·x + g, Φ·v the same call without S,
 *      g = F(0).  X returns the state at the START of the cycle with ‖F(x) - x‖₂ <= ptol·‖g‖₂, column by column.
 * Method (a contract; tests/periodic_ref.py restates it): per column restarted GMRES(restart) on (I - Φ)·δ = r, r = F(x) - x, without a
 *      preconditioner.  One iteration is one step call (w = v - Φ·v) for the columns that iterate, then classical Gram-Schmidt twice against
 *      the column's own basis; the Hessenberg column and the Givens rotations are the host's, in double.  When the recursive residual
 *      reaches ptol·‖g‖, when the basis is full (restart vectors) or exhausted (‖w‖ = 0), and when only one cycle of maxcycles is left:
 *      x += V·y, then r = F(x) - x explicitly (one cycle with S).  A column is accepted on that explicit value only; otherwise it goes on
 *      from it.  An iteration is only begun when a verifying cycle can follow it (cycles + 2 <= maxcycles), so X is always the state of the
 *      column's last explicit F(x) - x, and defect[c] = ‖F(x) - x‖₂ / ‖g‖₂ of exactly that X (NaN when none was computed).
 *      cycles[c]: the step calls column c took part in, the verifying ones included; maxcycles bounds it.  With use_x0 the first call
 *      carries x and 0 side by side (F(x) and g: 2k columns, one call); without, X is not read, the start is zero and g is the first r.
 *      A call that another column's failure ended is repeated without that column and not counted.
 *      S == NULL, or a column of S that is zero: g = 0, so x = 0, zero cycles, converged.
 * Columns are independent and a stopped column is frozen: X, cycles and defect of column c of k have the bits of that column alone, and the
 *      same call twice gives the same bits (every sum runs in an order fixed by n and the basis index; no floating-point atomics, no FMA).
 * Arguments: as otmb_op_step (ncycle for nsteps, but >= 1), and ptol > 0, restart >= 1, maxcycles >= 0, cycles / defect / reason not NULL:
 *      otherwise OTMB_ERR_INVALID_ARG before X is touched.  The selected slot is the same after the call as before it.
 * Returns OTMB_OK, or OTMB_ERR_NOT_CONVERGED when any column's reason is not OTMB_PERIODIC_CONVERGED (X and the three arrays are valid: an
 *      answer).  An inner step that leaves a column not converged stops that column with OTMB_PERIODIC_STEP_FAILED and the message carries
 *      the step's own text (step and slot); a non-finite norm or product stops it with OTMB_PERIODIC_NONFINITE.  Such a column keeps the
 *      state of its last explicit F(x) - x.  A singular preconditioner is the error otmb_op_step gives (X not written); the workspace --
 *      (restart + 3)·n·k doubles and the partial sums, owned by the operator -- that cannot be had is OTMB_ERR_ALLOC with X untouched.
 * cycles, defect, reason: HOST arrays of k entries.  otmb_op_periodic_dev: d, S, X device pointers, on the context's stream.
 *      otmb_op_periodic: host pointers, staged once like otmb_op_step.                                                                  */
typedef enum { OTMB_PERIODIC_CONVERGED = 0, OTMB_PERIODIC_MAXCYCLES = 1, OTMB_PERIODIC_STEP_FAILED = 2, OTMB_PERIODIC_NONFINITE = 3 } otmb_periodic_reason;
int32_t otmb_op_periodic_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                             const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond,
                             double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason);
int32_t otmb_op_periodic(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                         const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond,
                         double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason);

/* ---- otmb_op_periodic_pc[_dev]: otmb_op_periodic[_dev] with a choice of preconditioner for the outer GMRES.  The arguments are
 *      otmb_op_periodic's, then outer (otmb_outer) and msolve_iters (HOST array of k entries or NULL).  otmb_op_periodic[_dev] is this call
 *      with OTMB_OUTER_NONE and NULL.
 * OTMB_OUTER_NONE: the method stated above, bit for bit; msolve_iters, if given, is zero.
 * OTMB_OUTER_MEAN (a contract; tests/periodic_pc_ref.py restates it): flexible GMRES, right-preconditioned by the cycle-mean operator.  With
 *      P = ncycle·dt and M̄ = diag(d) + Ā, Ā the visit-weighted mean of the cycle's slots, one implicit-Euler step over the whole period gives
 *      Φ ≈ (I + P·M̄)⁻¹, hence (I - Φ)⁻¹ ≈ I + (P·M̄)⁻¹: one solve with M̄ at σ = 0.
 *      The mean values: otmb_op_combine_slots' fold with w[s] = count_s / ncycle (one double division), count_s the visits of slot s by the
 *      steps first_slot .. first_slot + ncycle - 1, into a value set private to the operator, made once per call; the caller's slots and
 *      the selected slot are untouched.  P = (double)ncycle * dt.  The mean's preconditioner (precond, σ = 0, the call's d and adjoint) is
 *      factorised once per call before X is touched: a singular one is OTMB_ERR_SINGULAR_PRECONDITIONER with X not written.
 *      Iteration i, per column:  q from (diag(d) + Ā)·q = V_i by otmb_op_solve_pc_dev's own path on the mean values (σ = 0, use_x0 = 0, the
 *      call's rtol, maxiter, precond), for the columns that iterate together, gathered compactly as for the step;
 *      Z_i = V_i + q / P (one division, one addition);  w = Z_i - Φ·Z_i (one step call without the source);  Gram-Schmidt twice against V, the
 *      Hessenberg column, the rotations and V_{i+1} as above;  at a restart x += Σ_j y_j·Z_j, j ascending.  The restart, verify and stop
 *      rules, cycles (a mean solve is not a cycle) and defect are as above: an answer is accepted on the explicit F(x) - x only.
 *      A column whose mean solve does not converge stops alone with OTMB_PERIODIC_PRECOND_FAILED, keeps the state of its last explicit
 *      F(x) - x, and the message carries the solver's report; the solve is repeated without it, as a step call is.
 *      msolve_iters[c]: the BiCGStab iterations column c spent in mean solves (those of a solve repeated for another column's sake are not
 *      counted twice).  Columns stay independent: X, cycles, defect and msolve_iters of column c of k have the bits of the column alone.
 *      Workspace: (2·restart + 3)·n·k doubles (the Z block behind the V block) and the mean's values and preconditioner; only this mode
 *      allocates them, and a failure is OTMB_ERR_ALLOC with X untouched.
 * outer neither value: OTMB_ERR_INVALID_ARG before X is touched.                                                                          */
typedef enum { OTMB_OUTER_NONE = 0, OTMB_OUTER_MEAN = 1 } otmb_outer;
typedef enum { OTMB_PERIODIC_PRECOND_FAILED = 4 } otmb_periodic_pc_reason; /* continues otmb_periodic_reason */
int32_t otmb_op_periodic_pc_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                                const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond,
                                double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer,
                                int64_t *msolve_iters);
int32_t otmb_op_periodic_pc(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double dt, double theta, int64_t ncycle, int64_t first_slot,
                            const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond,
                            double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer,
                            int64_t *msolve_iters);

/* ---- Per-column d: otmb_op_solve_dk, otmb_op_precond_dk, otmb_op_step_dk and otmb_op_periodic_dk [_dev].  Tracers that differ in their sink --
 *      ideal age (a surface restoring rate), radiocarbon (the same plus a decay rate λ on every cell), a dye restored over its own patch --
 *      share one call, one pass over the matrix per register block and one outer driver.  The arguments are those of otmb_op_solve_pc,
 *      otmb_op_precond, otmb_op_step_obs (q == 0 and tw == NULL: the plain step) and otmb_op_periodic_pc, with `const double *d` replaced by
 *      `const double *D, int64_t ldd`: D is column-major n x k with leading dimension ldd, column c the d of column c of B / S / X / x0.
 * The contract: column c of a per-column call has the bits of the existing call made with k = 1, that column of B / S / X / x0, and
 *      d = D[:, c], whatever the other columns hold and however many there are -- the state, iters, relres, reason, steps_done, the
 *      observations and the mean, cycles, defect and msolve_iters, and what a column that did not converge leaves behind.
 * D and ldd: D == NULL means zero, as for d.  Otherwise ldd >= n (rows beyond n are not read), or ldd == 0: the n values at D serve every
 *      column, and the call is the existing one, bit for bit -- the existing entry points ARE these calls with ldd = 0.  Any other ldd is
 *      OTMB_ERR_INVALID_ARG before anything is touched, and the message names the call.  _dev: D is a device pointer; the host variants
 *      upload D's n x k block once per call.
 * Workspace: with ldd != 0 a preconditioner holds σ + d, Jacobi's diagonal and, for the lines, the multipliers and the pivots per column,
 *      and u once (it does not depend on d): 2·n·k doubles (Jacobi) or 4·n·k + n (lines) where the shared d takes 2·n or 5·n.  The step's
 *      pool is n·k + used·(lines ? 4·k + 1 : 2·k)·n doubles, used = min(nsteps, slots): still one preconditioner per visited slot and call;
 *      a failed reservation is OTMB_ERR_ALLOC with X untouched.  otmb_op_periodic_dk adds 2·k columns of gathered D and, with
 *      OTMB_OUTER_MEAN, the mean's preconditioner for all k columns (made once per call) and a gathered copy of it.
 * A singular preconditioner is refused before anything is iterated or written, as in the existing calls; with ldd != 0 the message is theirs
 *      followed by " (column C of k)": C is the smallest 1-based column that has a bad entry, and the index is that column's first bad one.
 *      otmb_op_periodic_dk names the caller's column and k as well; a column whose source is zero is answered with zero and never stepped,
 *      as in the call with k = 1, so the step's preconditioner of such a column is not examined.  */
int32_t otmb_op_solve_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double sigma, const double *B, int64_t ldb,
                             double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason,
                             int32_t precond);
int32_t otmb_op_solve_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double sigma, const double *B, int64_t ldb, double *X,
                         int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond);
int32_t otmb_op_precond_dk_dev(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *D, int64_t ldd, double sigma, const double *Y,
                               int64_t ldy, double *Z, int64_t ldz);
int32_t otmb_op_precond_dk(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *D, int64_t ldd, double sigma, const double *Y,
                           int64_t ldy, double *Z, int64_t ldz);
int32_t otmb_op_step_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond,
                            int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs,
                            const double *tw, double *Xbar, int64_t ldm);
int32_t otmb_op_step_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                        int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond,
                        int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs,
                        const double *tw, double *Xbar, int64_t ldm);
int32_t otmb_op_periodic_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter,
                                int32_t precond, double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason,
                                int32_t outer, int64_t *msolve_iters);
int32_t otmb_op_periodic_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                            int64_t first_slot, const double *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter,
                            int32_t precond, double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason,
                            int32_t outer, int64_t *msolve_iters);

/* ---- A schedule for the time axis: otmb_op_step_sched[_dev] and otmb_op_periodic_sched[_dev].  Several steps inside one slot (four
 *      implicit steps inside January before February begins), a source per slot (gas exchange under a seasonal ice cover) and, for the step,
 *      a history: one factor per step and tracer on a fixed spatial pattern (CFC-11, SF6, bomb radiocarbon).  The arguments are those of
 *      otmb_op_step_dk and otmb_op_periodic_dk with `const double *S, int64_t lds` replaced by
 *      `int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale` (the periodic call takes no scale: a history
 *      is not periodic).  For a call of nsteps steps from first_slot on an operator with nslots slots:
 *        substeps = m >= 1: step t (0-based) runs with slot(t) = (first_slot + t / m) mod nslots, the division an integer one; m = 1 is the
 *          rule of otmb_op_step.
 *        S: an array of nsrc pointers to blocks, each n x k with leading dimension lds >= n (separate arrays need no stacking copy).  nsrc is
 *          0 (no source; S may be NULL), 1 (every step takes block 0) or nslots (step t takes block slot(t): the source of the month).
 *        scale: NULL, or a HOST array (in both variants, like tw) of nsteps·k finite values, step-major, entry t·k + c.  The source of step t,
 *          tracer c, row i is S_j[i,c] * scale[t·k + c]: one multiplication, made before anything else touches s.
 *        Everything else is otmb_op_step_dk's: D / ldd, dt, theta, the observers, tw / Xbar, the reports, the stopping rules and the
 *          restored selection.
 * In bits: step t of a scheduled call has the bits of otmb_op_step_dk_dev(nsteps = 1, first_slot = slot(t), S = S_eff) made from the state
 *      step t - 1 left, S_eff[i,c] = S_j[i,c] * scale[t·k + c], and S_j itself without scale.  The reports land at t·k + c, the observation
 *      block at t, and the mean's fold runs over t, as in otmb_op_step_obs.  Column c of k has the bits of that column alone with its own column
 *      of every source block, of scale and of D.  In the elementwise line:  sf = s * f;  theta == 1: b = a + sf;  theta < 1: sf / theta -- one
 *      operation per statement, no FMA; a scale of all 1.0 gives the bits of no scale (finite sources).  The k scale values of a step reach
 *      the right-hand-side kernels as a device pointer into a block of nsteps·k doubles staged once per call.
 *      A slot's preconditioner is made on the slot's first visit of the call and reused on every later step in that slot, the sub-steps
 *      included: sigma, d, adjoint and the values are fixed inside a call, so the bits are those of separate solves.  The workspace is still
 *      one preconditioner per visited slot: n·k + used·(a preconditioner's doubles) + (scale ? nsteps·k : 0) doubles,
 *      used = min(ceil(nsteps / m), nslots).  A failure's message names the step and the slot the schedule gave it.
 *      otmb_op_step_dk[_dev] and everything layered on it ARE this loop with substeps = 1, nsrc = (S ? 1 : 0) and scale = NULL, bit for bit.
 *      otmb_op_step_sched_dev: S is a HOST array of nsrc device pointers; D, X, W, obs, Xbar device pointers.  otmb_op_step_sched: nsrc host
 *      pointers; every block and D are staged once, and X, the observations and the mean come home once.
 * otmb_op_periodic_sched[_dev]: F is the scheduled step over ncycle steps, Φ·v the same call without sources, g = F(0); the method, the
 *      restart / verify / stop rules, the reasons and column independence are otmb_op_periodic_dk's for both values of outer.  A column is
 *      answered with zero and never stepped only when it is zero in EVERY source block.  With OTMB_OUTER_MEAN w[s] = count_s / ncycle, count_s
 *      the number of steps t in 0 .. ncycle - 1 with slot(t) = s, and P = (double)ncycle * dt.  The step calls take the columns that iterate
 *      gathered compactly, with those columns of all nsrc blocks: with nsrc > 1 the operator's workspace grows by nsrc·2k·n doubles (the
 *      first call's 2k columns need every block twice); with nsrc <= 1 it is otmb_op_periodic_dk's.  A failed reservation is OTMB_ERR_ALLOC
 *      with X untouched.  otmb_op_periodic_dk[_dev] and everything layered on it ARE this call with substeps = 1 and nsrc = (S ? 1 : 0).
 * Refused with OTMB_ERR_INVALID_ARG before anything is written, after the checks of the call they extend, the message naming
 *      otmb_op_step_sched or otmb_op_periodic_sched, the operator staying usable: substeps < 1; nsrc outside {0, 1, nslots}; nsrc > 0 with S
 *      NULL or any block NULL; lds < n; scale without a source, or with an entry that is not finite.
 * Not built: sources at sub-step resolution (interpolation of the matrices between slots: below).                                       */
int32_t otmb_op_step_sched_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                               int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X,
                               int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres,
                               int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm);
int32_t otmb_op_step_sched(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                           int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X, int64_t ldx,
                           double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters, double *relres, int32_t *reason, int64_t q,
                           const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm);
int32_t otmb_op_periodic_sched_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                   int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, double *X, int64_t ldx,
                                   int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles,
                                   int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters);
int32_t otmb_op_periodic_sched(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                               int64_t first_slot, int64_t substeps, int64_t nsrc, const double *const *S, int64_t lds, double *X, int64_t ldx, int32_t use_x0,
                               double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect,
                               int32_t *reason, int32_t outer, int64_t *msolve_iters);

/* ---- Matrices interpolated between slots: otmb_op_step_interp[_dev] and otmb_op_periodic_interp[_dev].  The convention of offline
 *      transport-matrix models (Khatiwala 2007): a monthly mean is valid at mid-month, and every time step takes the linear interpolation of
 *      the two neighbouring months.  The arguments are those of otmb_op_step_sched[_dev] and otmb_op_periodic_sched[_dev] with
 *      `int64_t first_slot, int64_t substeps` replaced by `const int64_t *slot_a, const int64_t *slot_b, const double *weight`: three HOST
 *      arrays (in both variants, like scale and tw) of nsteps entries, ncycle for the periodic call.  The schedule is explicit: the library
 *      blends what it is told to blend, and the convention is one small host rule (interp_schedule of the Python package, interpschedule of
 *      the Julia shim).
 *      The step's matrix: for step t let a = slot_a[t], b = slot_b[t], w = weight[t].  The step is PLAIN on slot a when a == b or w == 0.0,
 *      plain on slot b when w == 1.0, and otherwise BLENDED with
 *          A_t = (1.0 - w)·A_a + w·A_b:   wa = 1.0 - w, one double subtraction on the host;  per stored entry  pa = wa * va;  pb = w * vb;
 *          v = pa + pb  -- one operation per statement, no FMA: otmb_op_combine_slots' fold for two terms (IEEE addition commutes, so the
 *      order of the two terms cannot matter).  The same A_t stands on both sides of the θ-step, in the right-hand side and in the system.
 * In bits: a plain step has the bits of otmb_op_step_dk_dev(nsteps = 1, first_slot = that slot, S = S_eff); a blended step those of
 *      otmb_op_combine_slots_dev with the weights 1.0 - w at a, w at b and zero elsewhere into a spare slot c, followed by
 *      otmb_op_step_dk_dev(nsteps = 1, first_slot = c, S = S_eff); both from the state step t - 1 left, S_eff as in the scheduled step.  This
 *      holds for the states, steps_done, iterations, relres and reasons; the observation blocks and the mean are those of the chain's
 *      states; column c of k has the bits of that column alone.
 *      Sources and scale: nsrc is 0 or 1 (a source block per slot together with interpolation is refused), scale is the scheduled step's;
 *      the periodic call takes no scale.  The observers, tw and Xbar are otmb_op_step_sched's tail, unchanged.
 *      On the device a blended step writes its values into a private value set of the operator (two arrays sized like a slot's, allocated
 *      on the first blended step and freed with the operator; not the set of OTMB_OUTER_MEAN, which the periodic call keeps beside it) in
 *      ONE launch, makes its preconditioner afresh into one block that all blended steps share, then forms the right-hand side and solves.
 *      A plain slot's preconditioner is made on the slot's first plain visit and kept for the call.  The workspace does not grow with the
 *      number of blended steps: n·k + used·(a preconditioner's doubles) + (scale ? nsteps·k : 0) doubles, used = (the distinct slots of the
 *      plain steps) + (1 if any step is blended).  That the preconditioner's setup, its wait for the device included, runs on EVERY blended
 *      step is the cost of the convention.  A failure inside step t names the step, both slots and the weight; the caller's selection is
 *      restored on every return.
 * otmb_op_periodic_interp[_dev]: F is otmb_op_step_interp_dev over the ncycle steps of the schedule, Φ·v the same call without a source,
 *      g = F(0); the cycle map stays affine; the method, the restart / verify / stop rules, the reasons and column independence are
 *      otmb_op_periodic_dk's for both values of outer.  With OTMB_OUTER_MEAN w[s] = acc_s / (double)ncycle, acc_s accumulated over t in
 *      ascending order -- a plain step adds 1.0 to its slot, a blended step adds 1.0 - w to a, then w to b -- and P = (double)ncycle * dt.
 * Refused with OTMB_ERR_INVALID_ARG before anything is written, after the checks of the call they extend, the message naming
 *      otmb_op_step_interp or otmb_op_periodic_interp, the operator staying usable: nsrc outside {0, 1}; what the scheduled calls refuse about
 *      S, lds and scale; a NULL schedule array with nsteps > 0; a slot outside 0 .. nslots - 1; a weight that is not finite or lies outside
 *      [0, 1].
 * Not built here: a source block per slot under interpolation (otmb_op_step_season, below, takes one).  Not built at all: a periodic scale,
 *      different matrices on the two sides of a θ-step, and reusing a blended preconditioner across steps of equal (a, b, w).              */
int32_t otmb_op_step_interp_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                                const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                                double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar,
                                int64_t ldm);
int32_t otmb_op_step_interp(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                            const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                            double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm);
int32_t otmb_op_periodic_interp_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                    const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds,
                                    double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart,
                                    int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters);
int32_t otmb_op_periodic_interp(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S, int64_t lds, double *X,
                                int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles,
                                int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters);

/* ---- d and the source per slot, blended with the matrices: otmb_op_step_season[_dev] and otmb_op_periodic_season[_dev].  Gas exchange under
 *      a seasonal ice cover scales the source kw·(1 - ice)·C_sat/Δz AND the restoring rate d = kw·(1 - ice)/Δz by the same factor; so do
 *      CFCs, SF6, radiocarbon, oxygen and any surface restoring under a seasonal mixed layer.  Here every per-step field follows the calendar
 *      the way the matrix does.  The arguments are those of otmb_op_step_interp[_dev] and otmb_op_periodic_interp[_dev] with
 *      `const double *D, int64_t ldd` replaced by `int64_t nd, const double *const *D, int64_t ldd`.  The schedule is the explicit one
 *      (slot_a, slot_b, weight: three HOST arrays in both variants); a step with a == b is plain, so it holds the piecewise-constant schedule
 *      of otmb_op_step_sched as well (plain_schedule of the Python package, plainschedule of the Julia shim).
 *        D: a HOST array of nd pointers (device pointers in _dev, as S is) to blocks with the one ldd: ldd == 0, the n values of a block serve
 *          every column; ldd >= n, a block is n x k and column c is tracer c's.  nd is 0 (no d; D may be NULL), 1 (the block serves every
 *          step) or nslots (a block per slot).
 *        S: as in otmb_op_step_sched; nsrc is 0, 1 or nslots -- a block per slot is in order under interpolation in this family.
 *      The field of step t, with a = slot_a[t], b = slot_b[t], w = weight[t] and plain / blended decided exactly as for the matrix:
 *        a field given once (nd == 1, nsrc == 1) is used as it is on every step; it is never blended with itself (wa·x + w·x is not x in bits);
 *        a field given per slot is, on a plain step, the slot's block -- a's, or b's when w == 1.0;
 *        on a blended step wa = 1.0 - w (the host's subtraction, the matrix's), and per entry  pa = wa * xa;  pb = w * xb;  x = pa + pb  -- one
 *          operation per statement, no FMA: the fold the matrix gets.  The blended source is formed first; the step's scale then
 *          multiplies it as in the scheduled step.
 * In bits: step t has the bits of the chain of existing calls -- otmb_op_combine_slots_dev into a spare slot on a blended step, then the
 *      one-step otmb_op_step_dk_dev with D = D_t and S = S_t·scale from the state step t - 1 left -- in the states, steps_done, iters, relres,
 *      reason, the observation blocks and the mean.  Column c of k has the bits of that column alone with its own column of every block.
 *      With nd <= 1 and nsrc <= 1 the call has the bits of otmb_op_step_interp[_dev] / otmb_op_periodic_interp[_dev].
 *      A plain slot's preconditioner is made on the slot's first plain visit with that slot's d and kept for the call: d is a function of
 *      the slot, so this stays exact.  A blended step makes its own from D_t into the one shared block.  The workspace formula is
 *      otmb_op_step_interp's; the blended fields live in a scratch of the operator's, n·kc + n·k doubles (kc = k with ldd != 0, else 1),
 *      reserved by the first call with a blended step that needs it and freed with the operator.  On the device the two-term fold of a
 *      field is ONE launch over all columns (csrc/otmb_season.hip), which reads the caller's blocks where they lie: any 8-byte alignment,
 *      padded leading dimensions, 16-byte accesses only in a column whose every operand allows them.
 *      A failure names step, slots and weight as otmb_op_step_interp does; a singular preconditioner with a d per column adds
 *      " (column C of k)".
 * otmb_op_periodic_season[_dev]: F is otmb_op_step_season_dev over the schedule, Φ·v the same call without sources and with the same D blocks,
 *      g = F(0); the map stays affine; the method, the restart / verify / stop rules, the reasons and column independence are unchanged.  A
 *      column is answered with zero and never stepped only when it is zero in EVERY source block.  The step calls take the live columns
 *      gathered compactly; with ldd != 0 and nd > 1 that includes those columns of every D block: nd·2k·n doubles more, on the pattern of the
 *      sources' nsrc·2k·n.  A failed reservation is OTMB_ERR_ALLOC with X untouched.
 *      OTMB_OUTER_MEAN: the weights wt[s] = acc_s / ncycle are otmb_op_periodic_interp's, and M̄ = diag(d̄) + Ā.  With nd == nslots d̄ is the
 *      fold of otmb_op_combine_slots over the D blocks: the slots with wt[s] != 0.0 in ascending s, acc = wt[s]·D_s for the first, then
 *      acc = acc + wt[s]·D_s, no FMA -- the same kernel, one launch, up to 16 terms as kernel arguments and more through a table on the
 *      device -- written once per call before the mean's preconditioner is made.  With nd <= 1 d̄ is the given block, untouched.  d̄ changes
 *      only how fast the outer iteration converges: an answer is still accepted on the explicit F(x) - x alone.
 * Refused with OTMB_ERR_INVALID_ARG before anything is written, after the checks of the calls they extend, the message naming
 *      otmb_op_step_season or otmb_op_periodic_season, the operator staying usable: what otmb_op_step_interp / otmb_op_periodic_interp refuse
 *      about S, lds, scale and the schedule, except that nsrc = nslots is in order; nd outside {0, 1, nslots}; nd > 0 with D NULL or any
 *      block NULL; ldd neither 0 nor >= n.
 * Not built: a periodic scale, different matrices on the two sides of a θ-step, reuse of a blended preconditioner.                          */
int32_t otmb_op_step_season_dev(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta,
                                int64_t nsteps, const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S,
                                int64_t lds, const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done,
                                int64_t *iters, double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw,
                                double *Xbar, int64_t ldm);
int32_t otmb_op_step_season(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta, int64_t nsteps,
                            const int64_t *slot_a, const int64_t *slot_b, const double *weight,
                            int64_t nsrc, const double *const *S, int64_t lds, const double *scale, double *X, int64_t ldx, double rtol, int64_t maxiter, int32_t precond, int64_t *steps_done, int64_t *iters,
                            double *relres, int32_t *reason, int64_t q, const double *W, int64_t ldw, double *obs, const double *tw, double *Xbar, int64_t ldm);
int32_t otmb_op_periodic_season_dev(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta,
                                    int64_t ncycle, const int64_t *slot_a, const int64_t *slot_b, const double *weight, int64_t nsrc, const double *const *S,
                                    int64_t lds, double *X, int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol,
                                    int64_t restart, int64_t maxcycles, int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters);
int32_t otmb_op_periodic_season(otmb_op *op, int32_t adjoint, int64_t k, int64_t nd, const double *const *D, int64_t ldd, double dt, double theta, int64_t ncycle,
                                const int64_t *slot_a, const int64_t *slot_b, const double *weight,
                                int64_t nsrc, const double *const *S, int64_t lds, double *X,
                                int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int32_t precond, double ptol, int64_t restart, int64_t maxcycles,
                                int64_t *cycles, double *defect, int32_t *reason, int32_t outer, int64_t *msolve_iters);

#ifdef __cplusplus
}
#endif
#endif /* OTMB_H */
