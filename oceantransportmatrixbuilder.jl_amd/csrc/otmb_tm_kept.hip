// otmb_tm_kept.hip -- what a context remembers about the operators a caller kept (otmb_tm_args.kept_ops) and about T's pattern
// (OTMB_KEPT_T_PATTERN).  Every read and write of ctx->kept_rec[2..4], ctx->htab_key / htab_valid and ctx->tpat_rec is in this file; the two
// protocols (otmb_transportmatrix.hip) and the change of stream (otmb_ctx.hip) call the functions at its end.
//
// THE RECORDS.  kept_rec[m], m = TκH, TκVML, TκVdeep: the last call that STORED operator m, with its output arrays and arguments.  htab_key /
// htab_valid: the arguments the TκH table was built for.  tpat_rec: the last call that stored T's full union pattern (colptr, rowval).
// A record matches a call whose grid arrays, shape, slab, κ and given_epoch are the record's (record_matches; otmb_ctx_forget_given and host
// uploads of grid arrays move the epoch, so they retire every record without touching it).
//
// VALID: the store the record describes has been enqueued.
//   - a two-phase fill stores kept_rec[m] for every operator it wrote once its flags have been read clean, and tpat_rec when in addition no
//     entry of T cancelled -- both only while no asynchronous step is pending, whose fold would take the counts for ITS keepers (kept_after_sync_fill);
//   - a one-pass call stores them right after its enqueue, under the step's serial (kept_after_async_enqueue);
//   - the table: its build has been enqueued in front of a kept fill (kept_htab).  The neighbour table (tm_nbtab_kernel) lives in the same
//     allocation, is built with it and is valid exactly while it is (nbtab_built: false when it was not built for htab_key).
//   - the {v3D, ρ} table (tm_vrtab_kernel, a buffer of its own): its build has been enqueued in front of a kept fill that reads the neighbour
//     table and promised OTMB_KEPT_RHO (kept_vrtab); valid while the two tables above are, ρ is the array it was built from and every call
//     since made the promise.
// KNOWN (nnz_known): the writer has finished and nnz is its count.  At once for a synchronous fill; for an asynchronous step when it is folded
//   without error -- for T also without FLAG_T_CANCEL -- and is still the record's writer (kept_on_fold).  The two-phase plan honours known
//   records only, and only with no step pending: it hands the count out.  A one-pass call honours a valid kept_rec[m] whose arrays and capacity
//   are the call's; the count follows at the fold (kept_fold_nnz).  T's record is taken only when known, in both protocols (tpat_matches).
// DROPPED:
//   - kept_rec[m]: by every fill or one-pass call that does not keep m, before it enqueues anything (kept_drop; a plan drops nothing); all
//     three by a fill that is refused (kept_check_fill); by its writer folding with an error (kept_on_fold).
//   - the table: with kept_rec[TκH] (kept_drop); when it was built for other arguments (kept_htab rebuilds it); by a change of stream.
//   - the {v3D, ρ} table: with the TκH table (htab_drop); by every fill or one-pass call without OTMB_KEPT_RHO (kept_drop); when ρ is another array.
//   - tpat_rec: by a two-phase fill that does not take it, before its launch (a clean full write records itself afterwards), that fails its
//     flags, or that compacts T; by a one-pass call that does not take it (the call is the new writer, or T stays unwritten: no record); by a
//     folded step that took it and failed; by its writer folding with an error or a cancellation; by a compaction of the arrays it names
//     (kept_after_fixup); by a refused fill; by a change of stream (valid only: the record cannot match again before a new writer sets both).
#include <cstdlib>

#include "otmb_tm_column.h"
#include "otmb_tm.h"

// ---- otmb_tm_args.kept_ops (host side) ------------------------------------------------------------------------------------------
static double kept_kappa(const otmb_tm_args &a, int m) { return m == OTMB_TKH ? a.kappa_h : m == OTMB_TKVML ? a.kappa_vml : a.kappa_vdeep; }
// Does record r (of operator m) describe what this call would write?  out: the output arrays and capacity (two-phase plan: not known yet, NULL).
static bool record_matches(const otmb_ctx::KeptRecord &r, const otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, int m, const void *const out[3],
                           i64 cap) {
    if (!r.valid || r.epoch != ctx->given_epoch) return false;
    if (out && (r.colptr != out[0] || r.rowval != out[1] || r.nzval != out[2] || r.cap != cap)) return false;
    if (r.lwet3d != a.lwet3d || r.lwet != a.lwet || r.v3d != a.v3d || r.thk != a.thkcello || r.area != a.area2d || r.zt != a.zt ||
        r.ml != a.mlotst)
        return false;
    for (int d = 0; d < 4; ++d)
        if (r.edge[d] != a.edge_length[d] || r.dist[d] != a.dist_nbr[d]) return false;
    return r.nx == a.nx && r.ny == a.ny && r.nz == a.nz && r.n_wet == a.n_wet && r.wet_base == pl.wet_base && r.nnz_base == pl.nnz_base[m] &&
           r.topo == a.topology && r.kappa == kept_kappa(a, m);
}
static bool kept_matches(const otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, int m, const void *const out[3], i64 cap) {
    return record_matches(ctx->kept_rec[m], ctx, a, pl, m, out, cap);
}
// record r (of operator m): this call's arguments
static void record_set(otmb_ctx::KeptRecord &r, const otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, int m) {
    r.valid = true; r.epoch = ctx->given_epoch;
    r.lwet3d = a.lwet3d; r.lwet = a.lwet; r.v3d = a.v3d; r.thk = a.thkcello; r.area = a.area2d; r.zt = a.zt; r.ml = a.mlotst;
    for (int d = 0; d < 4; ++d) { r.edge[d] = a.edge_length[d]; r.dist[d] = a.dist_nbr[d]; }
    r.nx = a.nx; r.ny = a.ny; r.nz = a.nz; r.n_wet = a.n_wet; r.wet_base = pl.wet_base; r.nnz_base = pl.nnz_base[m];
    r.topo = a.topology; r.kappa = kept_kappa(a, m);
}
// after a call has stored operator m into out[0..2] (nnz: its count, or < 0 while the asynchronous step `serial` is pending)
static void kept_store(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, int m, void *const out[3], i64 cap, i64 nnz, uint64_t serial) {
    otmb_ctx::KeptRecord &r = ctx->kept_rec[m];
    record_set(r, ctx, a, pl, m);
    r.serial = serial;
    r.colptr = out[0]; r.rowval = out[1]; r.nzval = out[2]; r.cap = cap;
    r.nnz_known = nnz >= 0; r.nnz = nnz >= 0 ? nnz : 0;
}
// every slot this call writes or leaves unwritten (all but the kept ones) loses its record before anything is enqueued -- and a call that does not
// keep TκH, the TκH table: the table is valid only while no call has written TκH since it was built
// -- and a call that does not promise OTMB_KEPT_RHO, the {v3D, ρ} table: ρ may have changed
static void htab_drop(otmb_ctx *ctx) { ctx->htab_valid = false; ctx->vrtab_valid = false; }  // (the {v3D, ρ} table is valid only while the TκH table is)
void otmb_tm_kept_drop(otmb_ctx *ctx, unsigned keep, bool rho_promised) {
    for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m)
        if (!((keep >> m) & 1u)) ctx->kept_rec[m].valid = false;
    if (!((keep >> OTMB_TKH) & 1u)) htab_drop(ctx);
    if (!rho_promised) ctx->vrtab_valid = false;
}

// A kept fill: all three operators kept and nothing of a given operator read (the instantiations tm_kernel<FUSED, 4 | 12>)
static bool kept_is_kept_fill(const TmPlan &pl, const TmParams &p) { return pl.kept == KEPT_OPS && p.skip == KEPT_OPS && !p.hcp && !p.dcp; }

// ---- the kept operators' TκH table ---------------------------------------------------------------------------------------------------------
// A step that keeps all three diffusive operators still needs TκH's values in T.  Re-deriving them per column costs 5 thkcello and 16 metric
// loads and 8 divisions -- a third of the fill pass's L1 requests.  The context keeps them instead: h_regular's five values of every regular
// owned column, one array per slot (H_S, H_WC, H_SELF, H_EC, H_N), in memory the caller never sees (the kept output arrays may have been
// overwritten behind the library's back: T must not depend on them).  One thread per column, wet-rank order (once per grid); the loads and their
// clamps are fast_column's, so every stored value is bit for bit what the fill pass derives.  Irregular columns (tripolar seam row, nx < 3) are
// not stored: the fill pass builds them with build_column.  *nan: some wet neighbour's pair is NaN (the fill pass raises FLAG_TKH_NAN from it).
__global__ __launch_bounds__(256) void tm_htab_kernel(const TmParams p, double *__restrict__ tab, int *nan) {
    const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
    if (w >= p.n_own) return;
    const i64 L = p.lwet[w] - 1;
    if (L < 0 || L >= p.G) return;  // (indices that are not a makeindices result: the fill pass flags them)
    const Cell cell = cell_of(L, p.nx, p.ny, p.P);
    const int nx = p.nx, i = cell.i, j = cell.j;
    if (nx < 3 || (p.topo == OTMB_TRIPOLAR && j == p.ny - 1)) return;
    const bool hS = j > 0, hN = j + 1 < p.ny;
    const int di_e = (i + 1 < nx) ? 1 : 1 - nx, di_w = (i > 0) ? -1 : nx - 1;
    const i64 LE = L + di_e, LW = L + di_w, LS = hS ? L - nx : L, LN = hN ? L + nx : L;
    const i64 s2 = (i64)j * nx + i, sE = s2 + di_e, sW = s2 + di_w, sS = hS ? s2 - nx : s2, sN = hN ? s2 + nx : s2;
    const double *eW = p.edge[OTMB_DIR_WEST], *eE = p.edge[OTMB_DIR_EAST], *eS = p.edge[OTMB_DIR_SOUTH], *eN = p.edge[OTMB_DIR_NORTH];
    const double *dW = p.dist[OTMB_DIR_WEST], *dE = p.dist[OTMB_DIR_EAST], *dS = p.dist[OTMB_DIR_SOUTH], *dN = p.dist[OTMB_DIR_NORTH];
    Stencil s;
    s.vC = p.v[L]; s.vE = p.v[LE]; s.vW = p.v[LW]; s.vS = p.v[LS]; s.vN = p.v[LN];
    s.tC = p.thk[L]; s.tE = p.thk[LE]; s.tW = p.thk[LW]; s.tS = p.thk[LS]; s.tN = p.thk[LN];
    s.eW_c = eW[s2]; s.eE_c = eE[s2]; s.eS_c = eS[s2]; s.eN_c = eN[s2];
    s.dW_c = dW[s2]; s.dE_c = dE[s2]; s.dS_c = dS[s2]; s.dN_c = dN[s2];
    s.eE_w = eE[sW]; s.dE_w = dE[sW]; s.eW_e = eW[sE]; s.dW_e = dW[sE];
    s.eN_s = eN[sS]; s.dN_s = dN[sS]; s.eS_n = eS[sN]; s.dS_n = dS[sN];
    const bool wE = p.lw[LE] != 0, wW = p.lw[LW] != 0, wS = hS && p.lw[LS] != 0, wN = hN && p.lw[LN] != 0;
    double h5[NHTAB];
    const bool bad = h_regular(p.kH, s, wW, wE, wS, wN, h5);
#pragma unroll
    for (int q = 0; q < NHTAB; ++q) tab[(i64)q * p.n_own + w] = h5[q];
    if (bad) raise_flag(nan, 0);
}

// ---- the kept operators' neighbour table ---------------------------------------------------------------------------------------------------
// The fill pass gathers Lwet3D at a column's cell and its six neighbours: 7 loads in CELL order, where the dry cells between the wet ones spread
// a wave's 64 columns over more cache lines than 64 values need -- and the pass is bound by the L1 requests in flight.  Lwet3D is
// a grid constant, so the context keeps its content in WET-RANK order, the order the fill walks in: per regular owned column w the six
// neighbours' wet ranks (fast_column's clamps; 0: the neighbour does not exist or is dry -- what the masked gather yields), as one 16-byte record
// {S, N, A, B} (nb16) and one 8-byte record {E, W} (nb8) of 32-bit words, read by the fill with two coalesced loads.  One thread per column,
// wet-rank order, once per grid.  Irregular columns (tripolar seam row) are not read back: build_column reads Lwet3D.  *word: Lwet3D[Lwet[w]] !=
// w + 1 for some column, or a neighbour's entry lies outside 0 .. G and would not fit a word (the fill raises FLAG_NONCANONICAL from it).  wet_base == 0 and
// G < 2^31 (the host's conditions): every rank fits a word.  word[1]: some rank exceeds n_own (a first depth slab names its halo level's ranks): the
// {v3D, ρ} table, which holds the owned columns only, is then not used (kept_vrtab reads the word once per build).
__global__ __launch_bounds__(256) void tm_nbtab_kernel(const TmParams p, unsigned *__restrict__ nb16, unsigned *__restrict__ nb8, int *word) {
    const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
    if (w >= p.n_own) return;
    unsigned rS = 0, rN = 0, rA = 0, rB = 0, rE = 0, rW = 0;
    const i64 L = p.lwet[w] - 1;
    const bool inside = L >= 0 && L < p.G;  // (indices that are not a makeindices result: the fill pass flags them)
    if (!inside || p.lw[L] != w + 1) raise_flag(word, 0);
    const Cell cell = cell_of(inside ? L : 0, p.nx, p.ny, p.P);
    const int nx = p.nx, i = cell.i, j = cell.j, k = cell.k;
    if (inside && !(p.topo == OTMB_TRIPOLAR && j == p.ny - 1)) {
        const bool hS = j > 0, hN = j + 1 < p.ny, hA = k > 0, hB = k + 1 < p.nz;
        const int di_e = (i + 1 < nx) ? 1 : 1 - nx, di_w = (i > 0) ? -1 : nx - 1;
        auto rank = [&](bool exists, i64 LX) -> unsigned {
            if (!exists) return 0u;
            const i64 r = p.lw[LX];
            // (G, not n_own: the first slab of a deeper grid has wet_base == 0 and names its halo level's ranks, which lie beyond n_own; ranks are
            // stored as row indices only, exactly as the gathers pass them on unverified -- the bound only keeps them inside a word)
            if (r < 0 || r > p.G) { raise_flag(word, 0); return 0u; }
            if (r > p.n_own) raise_flag(word, 1);
            return (unsigned)r;
        };
        rE = rank(true, L + di_e); rW = rank(true, L + di_w); rS = rank(hS, L - nx); rN = rank(hN, L + nx);
        rA = rank(hA, L - p.P); rB = rank(hB, L + p.P);
    }
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    u32x4 q; q.x = rS; q.y = rN; q.z = rA; q.w = rB;
    u32x2 e; e.x = rE; e.y = rW;
    ((u32x4 *)nb16)[w] = q;
    ((u32x2 *)nb8)[w] = e;
}
// OTMB_KEPT_NBTAB=0 (read once per process): no neighbour table.  OTMB_KEPT_HTAB=0 implies it.
static bool nbtab_env_on() {
    static const bool on = [] { const char *e = getenv("OTMB_KEPT_NBTAB"); return !(e && e[0] == '0'); }();
    return on;
}

// Point p at a valid table when this call keeps all three operators (the HTAB fill kernel), building it first -- on the call's stream, in front
// of its fill -- when none is valid.  Valid: built after the last call on this context that did not keep TκH (kept_drop), for this call's grid
// arrays, κH, topology, n_wet and slab (kept_matches' fields), and in the current given_epoch.  OTMB_KEPT_HTAB=0, or a table that cannot be
// allocated: p is left alone, the kept fill re-derives TκH as before (no error).
static int32_t kept_htab(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, TmParams &p) {
    static const bool env_on = [] { const char *e = getenv("OTMB_KEPT_HTAB"); return !(e && e[0] == '0'); }();
    if (!kept_is_kept_fill(pl, p)) return OTMB_OK;
    ctx->htab_used = 0;  // (otmb_ctx_kept_htab: set to 1 below once p points at a valid table)
    ctx->nbtab_used = 0;  // (otmb_ctx_kept_nbtab likewise)
    ctx->vrtab_used = 0;  // (otmb_ctx_kept_vrtab likewise: kept_vrtab)
    ctx->occ4_used = 0;   // (otmb_ctx_kept_occ4 likewise: launch_fill)
    if (!env_on || a.nx < 3 || a.n_wet <= 0) return OTMB_OK;
    const size_t n = (size_t)a.n_wet, vals = (size_t)NHTAB * n * sizeof(double), hbytes = vals + 256;  // (+ the NaN word)
    // ... and behind it, 256-byte aligned: the neighbour table's word, nb16, nb8.  Wanted when every rank fits a record's 31 bits: ranks count
    // from this grid's first cell (no depth slab: wet_base == 0) and the grid has fewer than 2^31 cells
    const NbLayout lay = nb_layout(n);
    const size_t nbbytes = lay.bytes;
    bool want_nb = pl.wet_base == 0 && a.nx * a.ny * a.nz < (1ll << 31) && nbtab_env_on();
    if (want_nb && ctx->nbtab_nofit && nbbytes >= ctx->nbtab_nofit && ctx->htab.cap < nbbytes) want_nb = false;
    size_t bytes = want_nb ? nbbytes : hbytes;
    if (ctx->htab_valid && !record_matches(ctx->htab_key, ctx, a, pl, OTMB_TKH, nullptr, 0)) htab_drop(ctx);
    if (!ctx->htab_valid) {
        if (ctx->htab.cap < bytes) {
            if (ctx->htab_nofit && bytes >= ctx->htab_nofit) return OTMB_OK;  // (a size that did not fit is not tried again every step)
            // (a buffer that still holds the TκH table alone is given up for the larger one before that is tried: after a failure the TκH
            // table is allocated anew.  Deliberate: one sync, free and malloc more, once -- nbtab_nofit keeps it from happening again)
            if (ctx->htab.p) {
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (earlier fills may still read it)
                (void)hipFree(ctx->htab.p);
                ctx->htab.p = nullptr;
                ctx->htab.cap = 0;
            }
            if (want_nb && hipMalloc(&ctx->htab.p, bytes) != hipSuccess) {  // (both did not fit: the TκH table alone)
                (void)hipGetLastError();
                ctx->htab.p = nullptr;
                ctx->nbtab_nofit = bytes;
                want_nb = false;
                bytes = hbytes;
            }
            if (!ctx->htab.p && hipMalloc(&ctx->htab.p, bytes) != hipSuccess) {
                (void)hipGetLastError();
                ctx->htab.p = nullptr;
                ctx->htab_nofit = bytes;
                return OTMB_OK;
            }
            ctx->htab.cap = bytes;
        }
        ctx->nbtab_built = false;
        ctx->nbtab_beyond = -1;
        ctx->vrtab_valid = false;
        int *nanw = (int *)((char *)ctx->htab.p + vals);
        HIP_TRY(ctx, hipMemsetAsync(nanw, 0, sizeof(int), ctx->stream));
        {
            KernelTimer kt(ctx, K_TM_HTAB);
            hipLaunchKernelGGL(tm_htab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, (double *)ctx->htab.p, nanw);
        }
        HIP_TRY(ctx, hipGetLastError());
        if (want_nb) {
            char *b = (char *)ctx->htab.p;
            int *word = (int *)(b + lay.word);
            HIP_TRY(ctx, hipMemsetAsync(word, 0, 2 * sizeof(int), ctx->stream));
            {
                KernelTimer kt(ctx, K_TM_NBTAB);
                hipLaunchKernelGGL(tm_nbtab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, (unsigned *)(b + lay.nb16),
                                   (unsigned *)(b + lay.nb8), word);
            }
            HIP_TRY(ctx, hipGetLastError());
            ctx->nbtab_built = true;
        }
        record_set(ctx->htab_key, ctx, a, pl, OTMB_TKH);
        ctx->htab_valid = true;
    }
    if (ctx->nbtab_built) {  // (the fill finds the table behind p.htab: nb_layout(p.htab_n))
        p.nbtab = 1;
        ctx->nbtab_used = 1;
    }
    p.htab = (const double *)ctx->htab.p;
    p.htab_n = (i64)n;
    p.htab_nan = (const int *)((const char *)ctx->htab.p + vals);
    ctx->htab_used = 1;
    return OTMB_OK;
}

// ---- the kept operators' {v3D, ρ} table ---------------------------------------------------------------------------------------------------------
// With the neighbour table in registers the largest group of gathers left in a regular column are 7 v3D and 7 ρ loads in CELL order.  The context
// keeps both in WET-RANK order instead, one 16-byte record {v3D[Lwet[w] - 1], ρ[Lwet[w] - 1]} per owned column w, so the fill issues 7 loads of 16
// bytes at the ranks the neighbour table names (fast_column<..., VR>).  The values are copied: every loaded value is bit for bit the gathered one.
// v3D is a key of the TκH table's record; ρ is not (it is no grid constant), so the caller vouches for it: OTMB_KEPT_RHO.
__global__ __launch_bounds__(256) void tm_vrtab_kernel(const TmParams p, double *__restrict__ tab) {
    const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
    if (w >= p.n_own) return;
    const i64 L = p.lwet[w] - 1;
    const bool inside = L >= 0 && L < p.G;  // (indices that are not a makeindices result: the fill pass flags them)
    f64x2 r;
    r.x = inside ? p.v[L] : 0.0;
    r.y = inside ? p.rho[L] : 0.0;
    ((f64x2 *)tab)[w] = r;
}
// After kept_htab: point p at a valid {v3D, ρ} table when this fill reads the neighbour table (which implies wet_base == 0, nx >= 3 and a kept
// fill), ρ is 3-D, every record's byte offset fits 32 bits, no neighbour rank lies beyond the owned columns and the caller promised
// OTMB_KEPT_RHO -- building it first, on the call's stream in front of the fill, when none is valid.  OTMB_KEPT_VRTAB=0 (OTMB_KEPT_NBTAB=0 and
// OTMB_KEPT_HTAB=0 imply it: no neighbour table), or a table that cannot be allocated: p is left alone, the fill gathers as before (no error).
static int32_t kept_vrtab(otmb_ctx *ctx, const otmb_tm_args &a, TmParams &p) {
    static const bool env_on = [] { const char *e = getenv("OTMB_KEPT_VRTAB"); return !(e && e[0] == '0'); }();
    if (!p.nbtab || !p.htab) return OTMB_OK;
    const size_t n = (size_t)a.n_wet, bytes = 16 * n;
    if (!env_on || !a.rho || !(((unsigned)a.kept_ops & OTMB_KEPT_RHO) != 0) || bytes >= (1ull << 32)) return OTMB_OK;
    if (ctx->nbtab_beyond < 0) {
        // (once per build of the neighbour table: its word[1], whether a rank beyond n_own is named -- one stream synchronisation, like the tile order's)
        int beyond = 1;
        const int *word = (const int *)((const char *)ctx->htab.p + nb_layout(n).word);
        HIP_TRY(ctx, hipMemcpyAsync(&beyond, word + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ctx->nbtab_beyond = beyond != 0;
    }
    if (ctx->nbtab_beyond) return OTMB_OK;
    if (ctx->vrtab_valid && ctx->vrtab_rho != (const void *)a.rho) ctx->vrtab_valid = false;
    if (!ctx->vrtab_valid) {
        if (ctx->vrtab.cap < bytes) {
            if (ctx->vrtab_nofit && bytes >= ctx->vrtab_nofit) return OTMB_OK;  // (a size that did not fit is not tried again every step)
            if (ctx->vrtab.p) {
                HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (earlier fills may still read it)
                (void)hipFree(ctx->vrtab.p);
                ctx->vrtab.p = nullptr;
                ctx->vrtab.cap = 0;
            }
            if (hipMalloc(&ctx->vrtab.p, bytes) != hipSuccess) {
                (void)hipGetLastError();
                ctx->vrtab.p = nullptr;
                ctx->vrtab_nofit = bytes;
                return OTMB_OK;
            }
            ctx->vrtab.cap = bytes;
        }
        {
            KernelTimer kt(ctx, K_TM_VRTAB);
            hipLaunchKernelGGL(tm_vrtab_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, (double *)ctx->vrtab.p);
        }
        HIP_TRY(ctx, hipGetLastError());
        ctx->vrtab_rho = a.rho;
        ctx->vrtab_valid = true;
    }
    p.vrtab = ctx->vrtab.p;
    ctx->vrtab_used = 1;
    return OTMB_OK;
}

// ---- otmb_tm_args.kept_ops & OTMB_KEPT_T_PATTERN (host side) --------------------------------------------------------------------------------
// T's reserved rows are uni = padv | phh | pml | pdp, and padv ⊆ phh | pdp (an advective row is a wet neighbour's, the diagonal comes with one),
// pml ⊆ pdp: the pattern, colptr and rowval, is a function of the wet mask and the topology alone.  A kept fill whose T arrays hold the union
// pattern of a clean earlier write stores T's values only (tm_kernel<FUSED, 12>).  The record (ctx->tpat_rec) names that write's arrays and
// arguments; it counts once its writer is known to have finished without error or exact cancellation (nnz_known).
static bool tpat_matches(const otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, const void *colptrT, const void *rowvalT) {
    const otmb_ctx::KeptRecord &r = ctx->tpat_rec;
    return r.nnz_known && r.colptr == colptrT && r.rowval == rowvalT && record_matches(r, ctx, a, pl, OTMB_T, nullptr, 0);
}
// After kept_htab, for a fill with its outputs in p: does it store T's values only?  Only where the table is read (every invalidation of the kept
// operators is then one of this promise too) and `allowed` (the two-phase plan honoured the bit).  A fill that keeps all three operators sets
// otmb_ctx_kept_t_pattern's answer.
static bool tpat_take(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, const TmParams &p, bool allowed) {
    static const bool env_on = [] { const char *e = getenv("OTMB_KEPT_TPAT"); return !(e && e[0] == '0'); }();
    if (!kept_is_kept_fill(pl, p)) return false;
    const bool t = allowed && env_on && p.htab && (((unsigned)a.kept_ops & OTMB_KEPT_T_PATTERN) != 0) && tpat_matches(ctx, a, pl, p.colptr[0], p.rowval[0]);
    ctx->tpat_used = t ? 1 : 0;
    if (t) ctx->tpat_fills += 1;
    return t;
}
// A fill that did not take the record: it wrote T's full pattern into colptrT / rowvalT (the record's new writer: the asynchronous step `serial`,
// pending, or a clean synchronous fill with serial 0 and count nnz) or left T unwritten (NULL: no record).
static void tpat_store(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, void *colptrT, void *rowvalT, uint64_t serial, i64 nnz) {
    otmb_ctx::KeptRecord &r = ctx->tpat_rec;
    if (!colptrT || !rowvalT) { r.valid = false; r.nnz_known = false; return; }
    record_set(r, ctx, a, pl, OTMB_T);
    r.serial = serial;
    r.colptr = colptrT; r.rowval = rowvalT; r.nzval = nullptr; r.cap = 0;
    r.nnz_known = nnz >= 0; r.nnz = nnz >= 0 ? nnz : 0;
}
void otmb_tm_tpat_drop(otmb_ctx *ctx) { ctx->tpat_rec.valid = false; ctx->tpat_rec.nnz_known = false; }

// ---- what the protocols call (the lifecycle at the top of this file) ------------------------------------------------------------------------
// Which of the operators the caller says it kept does this call honour?  Sets pl.kept and adds it to pl.skip.  The one-pass call knows its output
// arrays and capacities and compares them; it needs no count (fold_pending supplies it).  The two-phase plan knows neither (NULL: the fill
// compares them, kept_check_fill) but hands the counts out: the record must be known, no asynchronous step may be pending, and no sparse add
// may read the operator (a foreign build).  It also decides pl.tpat: a clean record of T's pattern for these arguments (its arrays are the
// fill's to check, its count kept_plan_counts').
void otmb_tm_kept_decide(otmb_ctx *ctx, const otmb_tm_args &a, TmPlan &pl, int64_t *const colptr[5], int64_t *const rowval[5], double *const nzval[5],
                         const int64_t capacity[5], bool two_phase) {
    pl.kept = 0;
    if (!two_phase || (!pl.foreign && ctx->tm_next == ctx->tm_first))
        for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m) {
            if (!((((unsigned)a.kept_ops & KEPT_OPS) >> m) & 1u) || ((pl.skip >> m) & 1u)) continue;
            bool ok;
            if (two_phase) {
                ok = ctx->kept_rec[m].nnz_known && kept_matches(ctx, a, pl, m, nullptr, 0);
            } else {
                const void *out[3] = {colptr[m], rowval[m], nzval[m]};
                ok = kept_matches(ctx, a, pl, m, out, capacity[m]);
            }
            if (ok) pl.kept |= 1u << m;
        }
    pl.skip |= pl.kept;
    if (!two_phase) return;
    const otmb_ctx::KeptRecord &tr = ctx->tpat_rec;
    pl.tpat = (((unsigned)a.kept_ops & OTMB_KEPT_T_PATTERN) != 0) && pl.kept == KEPT_OPS && !(pl.skip & 1u) && ctx->tm_next == ctx->tm_first &&
              tr.nnz_known && record_matches(tr, ctx, a, pl, OTMB_T, nullptr, 0);
}
// (two-phase plan, after its counts have arrived) a kept operator's count is that of the write it was kept from; T's record is honoured only
// for the pattern this plan counted (another count: the record is not about these arrays' contents)
void otmb_tm_kept_plan_counts(otmb_ctx *ctx, TmPlan &pl, int64_t nnz[5]) {
    for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m)
        if ((pl.kept >> m) & 1u) nnz[m] = pl.nnz[m] = ctx->kept_rec[m].nnz;
    if (pl.tpat && pl.nnz[0] != ctx->tpat_rec.nnz) pl.tpat = false;
}
// (two-phase fill) a kept operator must be handed the arrays its record names (and nothing has touched the record since the plan); likewise T
// when the plan honoured OTMB_KEPT_T_PATTERN.  A refusal consumes the plan and drops the records.
int32_t otmb_tm_kept_check_fill(otmb_ctx *ctx, TmPlan &pl, int64_t *const colptr[5], int64_t *const rowval[5], double *const nzval[5]) {
    for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m) {
        const void *out[3] = {colptr[m], rowval[m], nzval[m]};
        const otmb_ctx::KeptRecord &r = ctx->kept_rec[m];
        if (((pl.kept >> m) & 1u) && !(kept_matches(ctx, pl.args, pl, m, out, r.cap) && r.nnz_known && r.nnz == pl.nnz[m])) {
            otmb_tm_kept_drop(ctx, 0, false);
            pl.valid = false;
            return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "kept_ops: the output arrays of a kept operator are not the ones its record names (plan again without the bit)");
        }
    }
    if (pl.tpat && !(tpat_matches(ctx, pl.args, pl, colptr[0], rowval[0]) && ctx->tpat_rec.nnz == pl.nnz[0])) {
        otmb_tm_kept_drop(ctx, 0, false);
        otmb_tm_tpat_drop(ctx);
        pl.valid = false;
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "kept_ops: T's arrays are not the ones the OTMB_KEPT_T_PATTERN record names (plan again without the bit)");
    }
    return OTMB_OK;
}
// In front of a fill launch whose outputs are wired into p: the TκH table (kept_htab), then *tpat: does the fill store T's values only
// (tpat_take)?  The two-phase fill may take the record only if its plan honoured the bit (pl.tpat), and drops a record it does not take here,
// because it records its own write only after its flags have been read; the one-pass call overwrites the record right after its enqueue.
int32_t otmb_tm_kept_before_fill(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, TmParams &p, bool two_phase, bool *tpat) {
    *tpat = false;
    int32_t rc;
    if ((rc = kept_htab(ctx, a, pl, p))) return rc;
    if ((rc = kept_vrtab(ctx, a, p))) return rc;
    *tpat = tpat_take(ctx, a, pl, p, two_phase ? pl.tpat : true);
    if (two_phase && !*tpat) otmb_tm_tpat_drop(ctx);  // (T is written in full, or not at all: a clean write records itself, kept_after_sync_fill)
    return OTMB_OK;
}
// (two-phase fill, flags read clean) the operators this fill stored: their records (a synchronous write, count known) -- only when no
// asynchronous step is pending, whose fold would take its counts for the steps that kept from IT
void otmb_tm_kept_after_sync_fill(otmb_ctx *ctx, const TmPlan &pl, const TmParams &p, bool tpat, bool t_cancel) {
    if (ctx->tm_next != ctx->tm_first) return;
    for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m) {
        void *out[3] = {p.colptr[m], p.rowval[m], p.nzval[m]};
        if (!((pl.skip >> m) & 1u)) {
            kept_store(ctx, pl.args, pl, m, out, 0, pl.nnz[m], 0);
            ctx->kept_fold_nnz[m] = pl.nnz[m]; ctx->kept_fold_status[m] = 0;  // (what an asynchronous step that keeps from it reports)
        }
    }
    // T's full pattern, written without cancellation: the record of OTMB_KEPT_T_PATTERN
    if (!tpat && pl.ntiles > 0 && !(pl.skip & 1u) && !t_cancel) tpat_store(ctx, pl.args, pl, p.colptr[0], p.rowval[0], 0, pl.nnz[0]);
}
// (one-pass call, enqueued as step `serial`) a step that wrote T's full pattern is the record's new writer (it counts once folded clean), one
// that left T unwritten drops it; the operators it stored: their records (nnz when the step is folded).  Returns those operators.
unsigned otmb_tm_kept_after_async_enqueue(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, const TmParams &p, const int64_t capacity[5],
                                          uint64_t serial, bool tpat) {
    if (!tpat) tpat_store(ctx, a, pl, pl.ntiles > 0 ? p.colptr[0] : nullptr, pl.ntiles > 0 ? p.rowval[0] : nullptr, serial, -1);
    const unsigned wrote = KEPT_OPS & ~pl.skip;
    for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m) {
        void *out[3] = {p.colptr[m], p.rowval[m], p.nzval[m]};
        if ((wrote >> m) & 1u) kept_store(ctx, a, pl, m, out, capacity[m], -1, serial);
    }
    return wrote;
}
// (fold_pending) the asynchronous step rec has finished with flags f, totals tot and verdict r.status.  A kept operator is what the most recent
// step that wrote it left: r takes that step's count and, if it has none of its own, its failure.
void otmb_tm_kept_on_fold(otmb_ctx *ctx, const otmb_ctx::TmStepRec &rec, const int *f, const i64 *tot, otmb_ctx::TmStepResult &r) {
    for (int m = OTMB_TKH; m <= OTMB_TKVDEEP; ++m) {
        if ((rec.kept >> m) & 1u) {
            r.nnz[m] = ctx->kept_fold_nnz[m];
            if (!r.status && ctx->kept_fold_status[m]) r.status = ctx->kept_fold_status[m];
        } else if ((rec.wrote >> m) & 1u) {
            ctx->kept_fold_nnz[m] = tot[m];
            // (stores that may be incomplete: what relied on them fails alike; the record is dropped on any failure)
            ctx->kept_fold_status[m] = (f[FLAG_NONCANONICAL] || f[FLAG_COUNT_MISMATCH] || f[FLAG_CAPACITY]) ? r.status : 0;
            otmb_ctx::KeptRecord &kr = ctx->kept_rec[m];
            if (kr.valid && kr.serial == rec.serial) {  // (this step is still the record's writer)
                if (r.status) kr.valid = false;
                else { kr.nnz = tot[m]; kr.nnz_known = true; }
            }
        }
    }
    // OTMB_KEPT_T_PATTERN: the record counts once its writer is folded clean; a failed step that used it drops it
    otmb_ctx::KeptRecord &tr = ctx->tpat_rec;
    if (tr.valid && rec.tpat && r.status) otmb_tm_tpat_drop(ctx);
    else if (tr.valid && !rec.tpat && tr.serial == rec.serial) {
        if (r.status || f[FLAG_T_CANCEL]) otmb_tm_tpat_drop(ctx);  // (a cancelling full write leaves its columns left-aligned: not the union pattern)
        else { tr.nnz_known = true; tr.nnz = tot[0]; }
    }
}
// (fold_pending) T in colptrT / rowvalT has been compacted: not the union pattern any more
void otmb_tm_kept_after_fixup(otmb_ctx *ctx, const void *colptrT, const void *rowvalT) {
    if (ctx->tpat_rec.colptr == colptrT || ctx->tpat_rec.rowval == rowvalT) otmb_tm_tpat_drop(ctx);
}
// A change of stream: the next kept step rebuilds the TκH table in place on the new stream.  Fills enqueued on the old one may still read
// it (its NaN word is zeroed before the rebuild), so they finish first.
void otmb_tm_kept_stream_changed(otmb_ctx *ctx) {
    if (ctx->htab_valid) (void)hipStreamSynchronize(ctx->stream);
    htab_drop(ctx);
    ctx->tpat_rec.valid = false;  // (T's values-only fills ride on the table's path)
}
