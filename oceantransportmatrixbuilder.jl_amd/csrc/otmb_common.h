// otmb_common.h -- shared declarations of libotmb_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/otmb.h"

typedef int64_t i64;
typedef uint64_t u64;

// One growable device buffer owned by the context (cached between calls).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct TmPlan;  // otmb_tm.h
struct OtmbXfer;  // otmb_xfer.h: pinned staging ring + host copy threads of the host-pointer entry points

// pending plan of the general path (otmb_coo.hip): COO generator and sparse()
struct CooPlan { int which = -1; otmb_tm_args args; int64_t ntiles = 0, len = 0; };
struct SpPlan { const int64_t *I = nullptr, *J = nullptr; const double *V = nullptr; int64_t len = -1, m = 0, n = 0, nnz = 0; int rowbits = 32; };  // rowbits: the sort keys are (column << rowbits) | row
struct SpScratch {   // sparse()'s sort: L = max(len, 1) words each
    DevBuf keys_in;  // u64 L: the keys as packed; the fill hands it over to the list of long runs of empty columns
    DevBuf keys_out, idx_in, idx_out;  // u64 L each: the sorted keys (the fill reads them), the input positions before and after the sort
    DevBuf prim_tmp;                   // rocPRIM's temporary
};

// kernel ids for the optional HIP-event timing (otmb_ctx_timing_*)
enum {
    K_TM_COUNT = 0, K_TILESCAN, K_TM_FILL, K_TM_FINISH, K_FACEFLUXES, K_IDX_COUNT, K_IDX_WRITE, K_VELFLUX, K_GM, K_GRIDMETRICS, K_PUSHMASK, K_TM_ORDER, K_FF_BASES, K_TM_HTAB, K_TM_NBTAB, K_TM_VRTAB, K_NKERNELS
};
#define OTMB_TIMING_POOL 2048

struct otmb_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream or a borrowed one
    std::string err;
    // scratch for the scans / flags
    DevBuf blocksums, blockoffs, flags, stamps, tcount, tfix[3];  // (stamps: diagnostic builds, OTMB_DBG_STAMPS)
    SpScratch sort;           // of the general sparse() path (otmb_coo.hip)
    DevBuf tm_sums, tm_offs;  // tile sums/offsets of the pending transportmatrix plan (must survive until fill)
    DevBuf mask;              // push mask derived by the library when the caller passes none
    DevBuf order;             // tile order of the fill pass (march order: otmb_ctx_set_tile_order) + its bucket scratch
    int march_rows = -1;      // rows per band of the march order; 0 = wet-rank order; -1 = the library's default
    int march_cols = -1;      // columns (i) per block of a band; 0 = whole rows; -1 = the library's default (experiments: OTMB_MARCH_COLS)
    struct OrderKey {
        const void *lwet = nullptr; int64_t n = 0, nx = 0, ny = 0, nz = 0; int rows = 0, topo = -1, cols = 0;
        bool operator==(const OrderKey &o) const { return lwet == o.lwet && n == o.n && nx == o.nx && ny == o.ny && nz == o.nz && rows == o.rows && topo == o.topo && cols == o.cols; }
    } order_key;              // what ctx->order was built for
    int deal_heavy = 1;         // 0: the heavy tiles stay in the first XCD's share (experiments: OTMB_DEAL_HEAVY)
    unsigned order_nheavy = 0;  // the order's first entries are this many heavy tiles (tripolar seam row), dealt over the XCDs
    int ff_xcd_chunks = 1;    // facefluxes: XCD x takes the x-th contiguous eighth of the column blocks (0 = blockIdx order; experiments: OTMB_FF_XCD)
    int ff_nt = -1;           // facefluxes' ϕ stores non-temporal (1), plain (0), by size (-1: beyond a gigabyte of fluxes) (experiments: OTMB_FF_NT)
    int ff_rows = 0;          // facefluxes: rows per workgroup, 1 or 4; 0 = by grid size (experiments: OTMB_FF_ROWS)
    int ff_pairs = -1;        // facefluxes: two levels per wave on whole-plane counting calls (facefluxes_pair_kernel): 1 wherever eligible, 0 never, -1 where all its waves are resident at once (OTMB_FF_PAIRS)
    int ff_pairs_last = -1;   // the last facefluxes call ran facefluxes_pair_kernel (1) or facefluxes_kernel (0); -1: none yet (otmb_ctx_ff_pairs)
    int n_cu = 0;             // compute units of the device
    int count_order = 2;      // counting pass: 0 = blockIdx (wet-rank) order, 1 = XCD-contiguous eighths of wet-rank order, 2 = of the fill pass's tile order (default: HBM fetch 1.06-1.11 x its inputs instead of 2.1-2.7 x, +2-4 % of this pass's time; OTMB_COUNT_ORDER)
    // ---- counts in facefluxes (otmb_facefluxes_counts_dev): the five per-tile row counts of the transportmatrix that will be built from the
    // fluxes a facefluxes call is writing are accumulated by that call (packed 64-bit atomics, one word per tile of 256 columns), so the
    // device-resident step has no counting pass.  Two buffers: the call after next may run beside the fill pass that consumes this one.
    int count_in_ff = 1;      // 0: otmb_facefluxes_counts_dev behaves as otmb_facefluxes_flags_dev (experiments / A-B: OTMB_COUNT_IN_FF)
    int tm_infill_groups = 64;  // up to this many scan groups the fill pass adds the group bases itself; beyond, the one-pass protocol scans all
                                // levels (tests reach that path on a grid of two groups: OTMB_TM_INFILL_GROUPS, 0 .. 64)
    int tm_infill_last = -1;    // the last tile scan of a transportmatrix left the group bases to the fill pass (1) or scanned all levels (0); -1: none yet (otmb_ctx_tm_infill)
    DevBuf ffc_sums[2];
    bool ffc_dirty[2] = {true, true};  // the buffer is not known to be all zero
    int ffc_next = 0;
    struct FfCountsKey {      // what the pending counts describe; consumed (valid = false) by the transportmatrix that uses them
        bool valid = false;
        int buf = 0, gen = 0;
        const void *phi[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        const void *mask = nullptr, *mlotst = nullptr, *zt = nullptr, *lwet3d = nullptr;
        const void *stat = nullptr;  // the grid's static per-tile counts (otmb_count_tables_dev), added by the scan
        int64_t nx = 0, ny = 0, nz = 0, n_wet = 0;  // (nz: of the grid the transportmatrix sees -- a depth slab's extended local grid)
        int64_t k_own0 = 0, wet_base = 0;           // depth slab: phi / mask name its owned levels, k_own0 levels into the extended arrays
        int topo = -1, upwind = -1, only_t = -1;
        bool pieces_open = false;  // the last facefluxes call counted: a further row band of it (otmb_facefluxes_slab_counts_dev, first = 0) adds to the same buffer
    } ffc;
    const void *ffc_partial_mask = nullptr;  // the push_mask argument of the last counting facefluxes call: NOT written by it, never a counting pass's input
    // lump_and_spray (otmb_lump.hip): the plan's scratch, which the fill goes on using.  G cells, N wet cells, Nc coarse cells, numbers 2 .. cmax - 1.
    // A member that is handed over to another array in the course of a call says so here and at the hand-over.
    struct LumpScratch {
        DevBuf isanchor;  // u8 G
        DevBuf owner;     // u32 G: the last anchor whose block covers a cell
        DevBuf ncomp;     // u32 G: components of every anchor's block; handed over to counts (u32 Nc + 1, the coarse cells' sizes), which the fill reads
        DevBuf arank;     // i64 G + 2: anchors before a cell
        DevBuf inc;       // i64 G + 2: what a scan reads -- anchor flags, numbers consumed per cell, `used` widened, in the fill the counts widened (+ their offsets)
        DevBuf cbase;     // i64 G + 2: the counter c at every cell; handed over to the fill's sort: keys out, values in, values out (i64 N each)
        DevBuf labels;    // u16 per anchor and block cell: component numbers
        DevBuf cnum;      // i64 N numbers of the wet cells | i64 N their coarse rows (crow)
        DevBuf used;      // i64 cmax + 2 newidx (number -> coarse row) | u8 cmax + 1 used (the number holds a wet cell)
        DevBuf prim_tmp;  // rocPRIM's temporary (scans, the fill's sort)
        DevBuf covk;      // int nx * ny, dk > 1 only: the last level a column is covered to
    } lump;
    DevBuf lump_host;         // staging of the host-pointer entry point
    bool lump_valid = false;
    i64 lump_N = 0, lump_Nc = 0;
    int *h_flags = nullptr;  // pinned host mirror of the state block (flag words first)
    i64 *h_tot = nullptr;    // the totals inside it (h_flags + OTMB_NFLAGS)
    int ff_gen = 0;          // facefluxes call counter: a validity flag is set by writing the current value (no reset pass)
    int ff_first = 1;        // oldest facefluxes call whose validity flags have not been handed out (otmb_facefluxes_pending_flags)
    // asynchronous pipeline: every otmb_transportmatrix_dev call gets its own state block (flags + totals) and every
    // facefluxes call its own pair of validity words, in rings of OTMB_RING slots (device) mirrored in pinned host
    // memory, so that a failure in step 3 of 12 is still there when the host finally looks (otmb_transportmatrix_result)
    DevBuf ring;
    int *h_ring = nullptr;
    unsigned long long ring_clean = 0;  // ring slots (bit per slot) known to be zero on the device and unused
    i64 tm_first = 0, tm_next = 0;   // pending asynchronous transportmatrix steps [tm_first, tm_next)
    int32_t tm_sticky = 0;           // first failure folded out of the ring when it wrapped (status, step index)
    i64 tm_sticky_step = -1;
    std::string tm_sticky_msg;
    i64 tm_failed_step = -1;         // what the last otmb_transportmatrix_result found
    struct TmStepRec { void *colptrT, *rowvalT, *nzvalT; i64 n_wet, nnz_base0; int ignore_ops; unsigned wrote, kept; uint64_t serial; bool tpat; };
                                     // (wrote / kept: the operators m = 2..4 the step stored / took from an earlier step, otmb_tm_args.kept_ops;
                                     // tpat: the step stored T's values only, on the pattern tpat_rec names)
    uint64_t tm_serial = 0;          // asynchronous steps issued on this context so far
    std::vector<TmStepRec> tm_rec;   // T's output arrays of the pending steps [tm_first, tm_next) (compaction after exact cancellation)
    struct TmStepResult { int32_t status; i64 nnz[5]; };
    std::vector<TmStepResult> tm_hist;  // verdict and nnz of every step since the previous otmb_transportmatrix_result
    bool tm_hist_final = false;      // tm_hist describes a finished pipeline (cleared by the next otmb_transportmatrix_dev)
    int gm_lds_limit = -1;    // bolus_GM_velocity: LDS bytes the fused kernel may use (-1: not queried yet; 0: use the two streaming kernels)
    size_t gm_lds_set = 0;    // ... and the dynamic-LDS size its function attribute currently allows
    TmPlan *plan = nullptr;
    // ---- otmb_tm_args.given: is a given TκH / TκVdeep bit for bit what the fill pass derives?  One verdict per operator, keyed to every
    // array address and scalar the answer depends on, and to an epoch that otmb_ctx_forget_given (and every host upload of such an array) bumps.
    struct GivenVerdict {
        bool valid = false, derived = false, pattern = false;  // pattern: the same rows in the same order, other values (another κ)
        uint64_t epoch = 0;
        otmb_csc g = {nullptr, nullptr, nullptr, 0};
        const void *lwet3d = nullptr, *lwet = nullptr, *v3d = nullptr, *thk = nullptr, *edge[4] = {nullptr, nullptr, nullptr, nullptr},
                   *dist[4] = {nullptr, nullptr, nullptr, nullptr}, *area = nullptr, *zt = nullptr;
        int64_t nx = 0, ny = 0, nz = 0, n_wet = 0, wet_base = 0;
        int topo = -1;
        double kappa = 0.0;
    } given_verdict[5];
    uint64_t given_epoch = 1;
    int given_state[5] = {0, 0, 0, 0, 0};  // the last plan's treatment of operator m: 0 not given, 1 derived, 2 foreign, 3 derived pattern with other values (otmb_ctx_given_state)
    long given_checks = 0;                 // comparing passes run so far (tests: the verdict is cached)
    // ---- otmb_tm_args.kept_ops: what the last call that STORED operator m (TκH, TκVML, TκVdeep) wrote, and for which arguments.  A kept bit is
    // honoured only when the record matches the call; every call that writes the slot refreshes it, every call that leaves it unwritten drops it.
    struct KeptRecord {
        bool valid = false;
        bool nnz_known = false;   // the writing step has been folded (asynchronous) or was synchronous
        uint64_t serial = 0;      // the writing asynchronous step (tm_serial), 0: a synchronous fill
        uint64_t epoch = 0;       // given_epoch: otmb_ctx_forget_given and host uploads of grid arrays bump it
        const void *colptr = nullptr, *rowval = nullptr, *nzval = nullptr;
        int64_t cap = 0;
        const void *lwet3d = nullptr, *lwet = nullptr, *v3d = nullptr, *thk = nullptr, *edge[4] = {nullptr, nullptr, nullptr, nullptr},
                   *dist[4] = {nullptr, nullptr, nullptr, nullptr}, *area = nullptr, *zt = nullptr, *ml = nullptr;
        int64_t nx = 0, ny = 0, nz = 0, n_wet = 0, wet_base = 0, nnz_base = 0;
        int topo = -1;
        double kappa = 0.0;
        int64_t nnz = 0;
    } kept_rec[5];
    // ... and, in the order the asynchronous steps were issued, the most recent folded step that wrote operator m: its nnz and status are those of
    // every later step that kept m (fold_pending)
    int64_t kept_fold_nnz[5] = {0, 0, 0, 0, 0};
    int32_t kept_fold_status[5] = {0, 0, 0, 0, 0};
    // ... and the TκH table of the steps that keep all three operators (otmb_tm_kept.hip, kept_htab): five doubles per owned wet column and
    // a NaN word, built for the arguments in htab_key; dropped by every call that does not keep TκH (kept_drop) and by a change of stream
    DevBuf htab;
    bool htab_valid = false;
    KeptRecord htab_key;
    size_t htab_nofit = 0;  // an allocation of this many bytes failed: the kept fill re-derives TκH instead
    int htab_used = -1;     // the last fill that kept all three operators read the table (1) or re-derived TκH (0); -1: none yet (otmb_ctx_kept_htab)
    // ... and, behind the TκH table in the same allocation and valid with it, the neighbour table (kept_htab, tm_nbtab_kernel)
    bool nbtab_built = false; // it was built for htab_key
    size_t nbtab_nofit = 0;   // an allocation of this many bytes (both tables) failed: the TκH table alone is tried
    int nbtab_used = -1;      // the last fill that kept all three operators read the neighbour table (1) or gathered Lwet3D (0); -1: none yet
    int nbtab_beyond = -1;    // the neighbour table names a rank beyond n_own (a first depth slab's halo level): 1, none: 0; -1: its word has not been read
    // ... and the {v3D, ρ} table in wet-rank order (kept_vrtab, tm_vrtab_kernel), in a buffer of its own: valid while the two tables above are,
    // ρ is the array it was built from and every call since promised that ρ is unchanged (OTMB_KEPT_RHO)
    DevBuf vrtab;
    bool vrtab_valid = false;
    const void *vrtab_rho = nullptr;  // the ρ array it was built from
    size_t vrtab_nofit = 0;   // an allocation of this many bytes failed: the kept fill gathers v3D and ρ instead
    int vrtab_used = -1;      // the last fill that kept all three operators read it (1) or gathered v3D and ρ (0); -1: none yet (otmb_ctx_kept_vrtab)
    int occ4_used = -1;       // ... and ran the lean instantiation, four waves per SIMD (1), or another (0); -1: none yet (otmb_ctx_kept_occ4, launch_fill)
    // ... and T's pattern (OTMB_KEPT_T_PATTERN): the last call that wrote T's full union pattern (colptr, rowval; nzval unused), its serial and
    // arguments.  nnz_known: that writer finished cleanly -- folded without error or FLAG_T_CANCEL, or a synchronous fill without cancellation --
    // and nnz is T's reserved count.  Dropped by a call that writes T elsewhere or not at all, a failed step that used it, a compaction of its
    // arrays, and with the TκH table (a change of stream).
    KeptRecord tpat_rec;
    int tpat_used = -1;     // the last fill that kept all three operators stored T's values only (1) or all of T (0); -1: none yet
    int64_t tpat_fills = 0; // fills that stored T's values only, so far (otmb_ctx_kept_t_pattern_fills)
    DevBuf given_tmp[6];                   // temporaries of the foreign path's sparse adds: two (colptr, rowval, nzval) triples
    CooPlan coo;
    SpPlan sp;
    // LUMP * T * SPRAY (otmb_coarsen.hip): the pending plan (nnz < 0: none), its scratch, the staging of the host-pointer calls
    struct CoPlan {
        const int64_t *Ap = nullptr, *Ai = nullptr, *Bp = nullptr, *Bi = nullptr, *Sp = nullptr, *Si = nullptr;
        const double *Ax = nullptr, *Bx = nullptr, *Sx = nullptr;
        int64_t m = 0, N = 0, M = 0, n = 0, nS = 0, len = 0, nnz = -1;
        int cap = 0;  // LDS capacity of the small path; 0: the sorted path
        int rowbits = 0;
        uint64_t invalid = 0;
    } co_plan;
    struct CoScratch {
        DevBuf flags;     // bad bits (unsigned) | wmax (u64 at + 8)
        DevBuf woff;      // i64 nS + 1 widths w | i64 nS + 1 their exclusive scan woff (the fill reads woff)
        DevBuf cnt;       // i64 n + 1: 1, then the distinct rows of every column (small path)
        DevBuf colptr;    // i64 n + 1: kept for the fill
        // sorted path (len = contributions):
        DevBuf keys;      // u64 len as expanded | u64 len sorted
        DevBuf idx;       // u64 len iteration indices | u64 len sorted
        DevBuf val, sid;  // f64 len products a * b; i64 len the entry of S they belong to
        DevBuf heads;     // i64 len + 1 segment heads | i64 len + 1 their exclusive scan
        DevBuf prim_tmp;  // rocPRIM's temporary (scans, the sort)
    } co;
    DevBuf co_host, co_out;
    // buildTsink (otmb_sink.hip): the scratch of a call, kept between calls (the pattern is a grid constant: a year of calls has one size)
    struct SinkScratch {
        DevBuf inc;       // i64 N + 1: entries of every column (1 or 2), then 0
        DevBuf start;     // i64 N + 1: their exclusive scan; start[N] = nnz
        DevBuf flags;     // unsigned: the SK_* bits
        DevBuf prim_tmp;  // rocPRIM's temporary
        DevBuf host;      // staging of the host-pointer entry point
    } sink;
    // staging for the host-pointer entry points
    std::vector<DevBuf> stage;
    OtmbXfer *xfer = nullptr;
    DevBuf xfer_narrow;       // Int32 copies of the `narrow` items of a download (otmb_xfer.h)
    int xfer_threads = 0;     // host copy threads of this context's transfer engine; 0 = default (8, OTMB_XFER_THREADS); otmb_mgpu shares the cores among its slabs
    bool reuse_grid = false;  // otmb_ctx_set_reuse_grid: grid-constant host arrays are uploaded once (see include/otmb.h)
    i64 uploaded_bytes = 0;     // host -> device bytes of the host-pointer entry points (otmb_ctx_uploaded_bytes)
    bool reuse_fluxes = false;  // otmb_ctx_set_reuse_fluxes: ϕ that otmb_facefluxes left in the staging slots is not uploaded again
    struct StageKey { const void *host = nullptr; size_t bytes = 0; };
    std::vector<StageKey> stage_key;  // what each staging slot currently holds (host pointer it was uploaded from)
    // optional per-kernel timing with HIP events recorded on the launch stream
    bool timing = false;
    std::vector<hipEvent_t> ev;   // 2 * OTMB_TIMING_POOL events, created on first enable
    std::vector<int> ev_kernel;   // kernel id of each recorded pair
    double t_ms[K_NKERNELS] = {0};
    long t_n[K_NKERNELS] = {0};
};

// Brackets one kernel launch with events when timing is on.
struct KernelTimer {
    otmb_ctx *c;
    int slot;
    KernelTimer(otmb_ctx *ctx, int kernel_id) : c(ctx), slot(-1) {
        if (c->timing && c->ev_kernel.size() < (size_t)OTMB_TIMING_POOL) {
            slot = (int)c->ev_kernel.size();
            c->ev_kernel.push_back(kernel_id);
            (void)hipEventRecord(c->ev[2 * slot], c->stream);
        }
    }
    ~KernelTimer() {
        if (slot >= 0) (void)hipEventRecord(c->ev[2 * slot + 1], c->stream);
    }
};

#define OTMB_NFLAGS 16
// the 16 i64 totals behind the flag words (ctx->h_tot and its device twin): [0, 8) transportmatrix, [8] T's compaction, [9] the sparse add,
// then the general path's three (otmb_coo.hip), [13] makeindices, [14] the tile order's histogram word
enum { TOT_COO_LEN = 10 /* triplets of a COO generator */, TOT_SP_NNZ = 11 /* sparse(): stored entries */, TOT_SP_BAD = 12 /* ... triplets with an index out of range */ };
enum {
    FLAG_RHO_NAN = 0, FLAG_TADV_NAN, FLAG_TKH_NAN, FLAG_TKVML_NAN, FLAG_TKVDEEP_NAN,
    FLAG_FLUX_INTO_LAND, FLAG_NONCANONICAL, FLAG_GIVEN_MISMATCH /* the comparing pass (otmb_tm_args.given): an entry differs */, FLAG_CAPACITY,
    FLAG_T_CANCEL,  // some T entry summed to exactly zero: T was written with gaps and needs compaction
    FLAG_COUNT_MISMATCH,  // a tile's fill pass found other counts than its counting pass: push_mask does not describe ϕ
    OTMB_NFLAGS_TM = 12,            // words [0, OTMB_NFLAGS_TM) belong to transportmatrix and are reset by it
    // owned by facefluxes, behind the 16 scan totals: untouched by transportmatrix, which resets and fetches the
    // flag words and its totals as ONE block (one fill and one copy kernel per call instead of two of each)
    FLAG_U_VALID = 16 + 2 * 16, FLAG_V_VALID = FLAG_U_VALID + 1
};
// device state block (ctx->flags) and its pinned host mirror (ctx->h_flags): 16 flag words | 16 i64 totals | 4 words
#define OTMB_STATE_BYTES (OTMB_NFLAGS * sizeof(int) + 16 * sizeof(i64) + 4 * sizeof(int))
#define OTMB_TM_STATE_BYTES (OTMB_NFLAGS * sizeof(int) + 8 * sizeof(i64))  // flags + the totals transportmatrix uses
#define OTMB_RING 64
#define OTMB_RING_BYTES (OTMB_RING * OTMB_TM_STATE_BYTES + OTMB_RING * 2 * sizeof(int))
static inline int *otmb_ring_tm(int *ring, i64 step) { return (int *)((char *)ring + (size_t)(step % OTMB_RING) * OTMB_TM_STATE_BYTES); }
static inline int *otmb_ring_ff(int *ring, int gen) { return (int *)((char *)ring + OTMB_RING * OTMB_TM_STATE_BYTES) + 2 * (gen % OTMB_RING); }

int32_t otmb_fail(otmb_ctx *ctx, int32_t status, const char *detail = nullptr);
int32_t otmb_reserve(otmb_ctx *ctx, DevBuf &b, size_t bytes);
// counts in facefluxes: bit layout of a tile's packed word (the block scan's: T:11 | Tadv:11 | TκH:11 | TκVML:10 | TκVdeep:10) + two flag bits
#define FFC_TILE_SHIFT 8                  // tiles of 256 columns (TM_THREADS)
#define FFC_BAD_FLUX (1ull << 63)         // some cell of the tile pushes a non-zero flux into land / out of the grid
#define FFC_BAD_TABLE (1ull << 62)        // the bases table was built for another wave geometry
void otmb_launch_tilescan_packed(hipStream_t s, unsigned long long *packed, const unsigned long long *stat, uint32_t *sums, i64 *offs, i64 *tot, i64 *gsum, i64 ntiles,
                                 int *flags, unsigned long long keep, bool all_levels);  // otmb_scan.hip (keep: count fields of the matrices that are materialised)
int32_t otmb_launch_push_mask(otmb_ctx *ctx, const double *const phi[6], const int64_t *lwet3d, int64_t first, int64_t count,
                              uint16_t *push_mask);  // otmb_facefluxes.hip
int32_t otmb_facefluxes_top_counts(otmb_ctx *ctx, const void *umo, const void *vmo, int32_t src_is_f32, const uint8_t *wetflags, double fill,
                                   int64_t nx, int64_t ny, int64_t nz, int32_t topology, double *const phi[6], uint16_t *token,
                                   const otmb_ff_counts *counts);  // otmb_facefluxes.hip (the fused step)
void otmb_xfer_free(otmb_ctx *ctx);                                  // otmb_host.hip
bool otmb_host_is_pinned(const otmb_ctx *ctx, const void *p, size_t bytes);  // otmb_host.hip: inside a block of otmb_host_alloc

#define HIP_TRY(ctx, call)                                                              \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            char msg_[256];                                                             \
            snprintf(msg_, sizeof msg_, "%s -> %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return otmb_fail((ctx), OTMB_ERR_HIP, msg_);                                \
        }                                                                               \
    } while (0)

// ---- device-side scan of per-tile sums (otmb_scan.hip) -------------------------------------
// sums: [ntiles][nf] u32 ; offs: [ntiles][nf] i64 exclusive prefix ; tot: [nf] i64 (device)
// gsum: scratch of (ntiles / 1024 + 1) * nf i64 (see otmb_scan_scratch)
void otmb_launch_tilescan(hipStream_t s, const uint32_t *sums, i64 *offs, i64 *tot, i64 ntiles, int nf, i64 *gsum);
#define OTMB_SCAN_GROUP 1024  // tiles per first-level scan group (SCAN_THREADS of otmb_scan.hip)
void otmb_launch_tilescan_groups(hipStream_t s, const uint32_t *sums, i64 *offs, i64 *gsum, i64 ntiles, int nf);
static inline size_t otmb_scan_scratch(i64 ntiles, int nf) { return (size_t)(ntiles / 1024 + 2) * nf * sizeof(i64); }

// ---- push mask (include/otmb.h, otmb_push_mask_dev): bits 0-5 west, east, south, north, bottom, top;
// bit 6 wet; the centred-weighting variant in the high byte.  x / 2 is the reference's ϕ / 2 (:244-289).
enum { PM_W = 1u << 0, PM_E = 1u << 1, PM_S = 1u << 2, PM_N = 1u << 3, PM_B = 1u << 4, PM_T = 1u << 5, PM_WET = 1u << 6 };
__device__ __forceinline__ unsigned otmb_push_bits(double w, double e, double s, double n, double b, double t, bool wet) {
    const double hw = w / 2, he = e / 2, hs = s / 2, hn = n / 2, hb = b / 2, ht = t / 2;
    const unsigned lo = (w > 0.0 ? PM_W : 0u) | (e < 0.0 ? PM_E : 0u) | (s > 0.0 ? PM_S : 0u) | (n < 0.0 ? PM_N : 0u) |
                        (b > 0.0 ? PM_B : 0u) | (t < 0.0 ? PM_T : 0u) | (wet ? PM_WET : 0u);
    const unsigned hi = (((hw > 0.0) | (hw < 0.0)) ? PM_W : 0u) | (((he > 0.0) | (he < 0.0)) ? PM_E : 0u) |
                        (((hs > 0.0) | (hs < 0.0)) ? PM_S : 0u) | (((hn > 0.0) | (hn < 0.0)) ? PM_N : 0u) |
                        (((hb > 0.0) | (hb < 0.0)) ? PM_B : 0u) | (((ht > 0.0) | (ht < 0.0)) ? PM_T : 0u) | (wet ? PM_WET : 0u);
    return lo | (hi << 8);
}
