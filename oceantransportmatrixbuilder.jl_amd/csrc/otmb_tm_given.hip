// otmb_tm_given.hip -- operators the caller passes (otmb_tm_args.given): the comparing pass and its cached verdicts, how a plan treats each
// given operator, and the sparse-add path for a foreign one.
#include <cstdlib>

#include "otmb_tm_column.h"
#include "otmb_tm.h"

// ---- otmb_tm_args.given: the COMPARING pass ------------------------------------------------------------------------------------
// Is a given operator bit for bit what the fill pass would write?  One thread per column builds the column exactly as tm_kernel does
// (fast_column / build_column: the one copy of the arithmetic) and, for every operator m in g.check, reads the given matrix's column:
// same length, same rows in the same order (else: bit m of the verdict), same value BITS (-0.0 is not +0.0, a NaN equals itself; else: bit 8 + m --
// the derived PATTERN with other values, e.g. built with another κ: the fill pass can still read it).  The given arrays may be a depth
// slab's slice: column w holds entries [colptr[w] - colptr[0], colptr[w + 1] - colptr[0]) of rowval / nzval.  Nothing is stored but
// the verdict in flags[FLAG_GIVEN_MISMATCH].  Once per grid and κ (the verdict is cached), so plain wet-rank order, no staging.
struct GivenCmp {
    const i64 *cp[5], *ri[5], *vx[5];  // the given matrices' colptr / rowval / nzval (value bits)
    i64 nnz[5];
    unsigned check;
};
__global__ __launch_bounds__(TM_THREADS, TM_WAVES_PER_SIMD) void tm_given_kernel(const TmParams p, const GivenCmp g) {
    const int tid = threadIdx.x;
    const i64 w0 = (i64)blockIdx.x * TM_THREADS, w = w0 + tid;
    if (w0 >= p.n_own) return;
    const bool valid = w < p.n_own;
    const i64 wlast = (w0 + TM_THREADS - 1 < p.n_own) ? w0 + TM_THREADS - 1 : p.n_own - 1;
    const i64 wcl = valid ? w : wlast;
    const i64 L = p.lwet[wcl] - 1;
    const i64 Lnext = (wcl + 1 < p.n_own) ? p.lwet[wcl + 1] - 1 : p.G;
    const i64 Lmin = p.lwet[w0] - 1, Lmax = p.lwet[wlast] - 1;
    const i64 base_elem = (Lmin > p.P) ? Lmin - p.P : 0;
    const bool span_ok = (Lmax + p.P - base_elem) < (1ll << 28) && Lmin >= 0 && Lmax < p.G && Lmin <= Lmax;
    if (!valid) return;
    if (!span_ok || L < Lmin || L > Lmax || Lnext <= L) {  // not a makeindices result: nothing can be derived from it
        atomicOr(&p.flags[FLAG_GIVEN_MISMATCH], (int)g.check);
        return;
    }
    TileBase tb;
    tb.lw = (const char *)(p.lw + base_elem);
    tb.v = (const char *)(p.v + base_elem);
    tb.thk = (const char *)(p.thk + base_elem);
    tb.rho = p.rho ? (const char *)(p.rho + base_elem) : nullptr;
    tb.pt = (const char *)(p.phi[OTMB_TOP] + base_elem);
    tb.pe = (const char *)(p.phi[OTMB_EAST] + base_elem);
    tb.pw = (const char *)(p.phi[OTMB_WEST] + base_elem);
    tb.pn = (const char *)(p.phi[OTMB_NORTH] + base_elem);
    tb.ps = (const char *)(p.phi[OTMB_SOUTH] + base_elem);
    tb.pb = (const char *)(p.phi[OTMB_BOTTOM] + base_elem);
    tb.pu = tb.pv = tb.mk = nullptr;
    Column col;
    Stamps st;
    const i64 c = p.wet_base + w + 1;
    const Cell cell = cell_of(L, p.nx, p.ny, p.P);
    const unsigned oC = (unsigned)(L - base_elem) * 8u;
    const bool regular = (p.nx >= 3) && !(p.topo == OTMB_TRIPOLAR && cell.j == p.ny - 1);
    bool canonical;
    if (regular) canonical = fast_column<0>(p, tb, oC, cell.i, cell.j, cell.k, c, col, st);
    else {
        canonical = ldi(tb.lw, oC) == c;
        if (canonical) build_column(p, cell, c, col);
    }
    if (!canonical) {
        atomicOr(&p.flags[FLAG_GIVEN_MISMATCH], (int)g.check);
        return;
    }
    const unsigned vslots = (1u << S_A) | (1u << S_SELF) | (1u << S_B);
    const unsigned pm[5] = {0u, col.padv, col.phh, col.pml & vslots, col.pdp & vslots};
    unsigned bad = 0;  // bit m: the column's length or rows differ; bit 8 + m: only values do
#pragma unroll
    for (int m = 1; m < TM_NF; ++m) {
        if (!((g.check >> m) & 1u)) continue;
        const i64 c0 = g.cp[m][0];
        const i64 lo = g.cp[m][w] - c0, hi = g.cp[m][w + 1] - c0;
        bool ok = lo >= 0 && hi <= g.nnz[m] && hi - lo == (i64)__popc(pm[m]), same = true;
        if (w == p.n_own - 1) ok &= hi == g.nnz[m];
        if (ok) {
#pragma unroll
            for (int sl = 0; sl < NSLOT; ++sl) {
                if ((pm[m] >> sl) & 1u) {
                    const i64 q = lo + (i64)__popc(pm[m] & col.bef[sl]);
                    const double v = (m == 1) ? col.adv[sl] : (m == 2) ? col.hh[sl] : (m == 3) ? col.ml[sl] : col.dp[sl];
                    ok &= g.ri[m][q] == col.idx[sl];
                    same &= g.vx[m][q] == __double_as_longlong(v);
                }
            }
        }
        if (!ok) bad |= 1u << m;
        else if (!same) bad |= 0x100u << m;
    }
    if (bad) atomicOr(&p.flags[FLAG_GIVEN_MISMATCH], (int)bad);
}

// ---- otmb_tm_args.given (host side) ---------------------------------------------------------------------------------------------
static unsigned given_mask(const otmb_tm_args &a) {
    unsigned g = 0;
    for (int m = 1; m < 5; ++m)
        if (a.given[m].colptr) g |= 1u << m;
    return g;
}
static bool verdict_matches(const otmb_ctx::GivenVerdict &v, const otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, int m) {
    if (!v.valid || v.epoch != ctx->given_epoch) return false;
    const otmb_csc &g = a.given[m];
    if (v.g.colptr != g.colptr || v.g.rowval != g.rowval || v.g.nzval != g.nzval || v.g.nnz != g.nnz) return false;
    if (v.lwet3d != a.lwet3d || v.lwet != a.lwet || v.v3d != a.v3d || v.nx != a.nx || v.ny != a.ny || v.nz != a.nz || v.n_wet != a.n_wet ||
        v.wet_base != pl.wet_base || v.topo != a.topology)
        return false;
    if (m == OTMB_TKH) {
        if (v.thk != a.thkcello || v.kappa != a.kappa_h) return false;
        for (int d = 0; d < 4; ++d)
            if (v.edge[d] != a.edge_length[d] || v.dist[d] != a.dist_nbr[d]) return false;
    } else {
        if (v.area != a.area2d || v.zt != a.zt || v.kappa != a.kappa_vdeep) return false;
    }
    return true;
}
static void verdict_store(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, int m, bool derived, bool pattern) {
    otmb_ctx::GivenVerdict &v = ctx->given_verdict[m];
    v.valid = true; v.derived = derived; v.pattern = pattern; v.epoch = ctx->given_epoch; v.g = a.given[m];
    v.lwet3d = a.lwet3d; v.lwet = a.lwet; v.v3d = a.v3d; v.thk = a.thkcello; v.area = a.area2d; v.zt = a.zt;
    for (int d = 0; d < 4; ++d) { v.edge[d] = a.edge_length[d]; v.dist[d] = a.dist_nbr[d]; }
    v.nx = a.nx; v.ny = a.ny; v.nz = a.nz; v.n_wet = a.n_wet; v.wet_base = pl.wet_base; v.topo = a.topology;
    v.kappa = (m == OTMB_TKH) ? a.kappa_h : a.kappa_vdeep;
}
// the comparing pass over the operators in `check`; *derived: those that are bit for bit what the fill pass writes; *pattern: those with
// exactly its rows and other values.  Synchronises.
static int32_t verify_given(otmb_ctx *ctx, const otmb_tm_args &a, const TmPlan &pl, unsigned check, unsigned *derived, unsigned *pattern) {
    *derived = *pattern = 0;
    if (a.n_wet == 0) {  // a 0 x 0 matrix: derived iff it is empty
        for (int m = 1; m < 5; ++m)
            if (((check >> m) & 1u) && a.given[m].nnz == 0) *derived |= 1u << m;
        return OTMB_OK;
    }
    TmPlan tmp;
    tmp.wet_base = pl.wet_base;
    tmp.skip = 0;
    TmParams p;
    otmb_tm_fill_params(p, a, ctx, &tmp);
    // TκH / TκVdeep do not look at the fluxes: the six ϕ pointers name v3D (G readable Float64), so that this pass can run for callers
    // whose ϕ arrays do not exist (otmb_step_dev) or are about to be overwritten
    for (int f = 0; f < 6; ++f) p.phi[f] = a.v3d;
    int *dflags = (int *)ctx->flags.p;
    p.flags = dflags;
    GivenCmp g;
    memset(&g, 0, sizeof g);
    g.check = check;
    for (int m = 1; m < 5; ++m) {
        g.cp[m] = (const i64 *)a.given[m].colptr; g.ri[m] = (const i64 *)a.given[m].rowval; g.vx[m] = (const i64 *)a.given[m].nzval;
        g.nnz[m] = a.given[m].nnz;
    }
    HIP_TRY(ctx, hipMemsetAsync(dflags, 0, OTMB_TM_STATE_BYTES, ctx->stream));
    const i64 ntiles = (a.n_wet + TM_THREADS - 1) / TM_THREADS;
    hipLaunchKernelGGL(tm_given_kernel, dim3((unsigned)ntiles), dim3(TM_THREADS), 0, ctx->stream, p, g);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_flags, dflags, OTMB_NFLAGS_TM * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(dflags, 0, OTMB_TM_STATE_BYTES, ctx->stream));  // (whatever the columns' arithmetic flagged is the real pass's to report)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const unsigned differs = (unsigned)ctx->h_flags[FLAG_GIVEN_MISMATCH], rows = differs & 0xffu, values = (differs >> 8) & 0xffu;
    *derived = check & ~rows & ~values;
    *pattern = check & ~rows & values;
    ctx->given_checks += 1;
    return OTMB_OK;
}
// Which operators does the caller pass, and how is each treated?  Sets pl.given / derived / read / foreign / skip and ctx->given_state.
int32_t otmb_tm_classify_given(otmb_ctx *ctx, const otmb_tm_args &a, TmPlan &pl) {
    // (OTMB_GIVEN_PATTERN=0: an operator with the derived rows and other values is treated as any foreign matrix -- A/B, tests of the sparse-add path)
    static const bool env_pattern = [] { const char *e = getenv("OTMB_GIVEN_PATTERN"); return !(e && e[0] == '0'); }();
    pl.given = given_mask(a);
    pl.derived = pl.foreign = pl.read = 0;
    for (int m = 0; m < 5; ++m) { ctx->given_state[m] = 0; pl.built_nnz[m] = 0; }
    pl.skip = (a.only_t ? 0x1eu : 0u) | ((unsigned)a.skip_ops & 0x1fu);
    pl.want_t = !(pl.skip & 1u);
    if (a.given[OTMB_T].colptr) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "given[OTMB_T]: T is never passed in (src/matrixbuilding.jl:133-138)");
    if (!pl.given) return OTMB_OK;
    unsigned check = 0;
    for (int m = 1; m < 5; ++m) {
        if (!((pl.given >> m) & 1u)) continue;
        const otmb_csc &g = a.given[m];
        if (g.nnz < 0 || (g.nnz > 0 && (!g.rowval || !g.nzval))) return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "given operator: arrays / nnz");
        if (m == OTMB_TKH || m == OTMB_TKVDEEP) {  // functions of the grid and κ alone: worth a verdict that is kept
            if (verdict_matches(ctx->given_verdict[m], ctx, a, pl, m)) {
                if (ctx->given_verdict[m].derived) pl.derived |= 1u << m;
                if (ctx->given_verdict[m].pattern) pl.read |= 1u << m;
            } else {
                check |= 1u << m;
            }
        }
    }
    if (check) {
        unsigned d = 0, pt = 0;
        int32_t rc;
        if ((rc = verify_given(ctx, a, pl, check, &d, &pt))) return rc;
        for (int m = 1; m < 5; ++m)
            if ((check >> m) & 1u) verdict_store(ctx, a, pl, m, (d >> m) & 1u, (pt >> m) & 1u);
        pl.derived |= d;
        pl.read |= pt;
    }
    // the derived rows with other values: not materialised either -- the fill pass reads the values where they lie
    if (!env_pattern) pl.read = 0;
    pl.derived |= pl.read;
    pl.foreign = pl.given & ~pl.derived;
    if (pl.foreign && pl.want_t && (pl.skip & 0x1eu & ~pl.given))
        return otmb_fail(ctx, OTMB_ERR_INVALID_ARG, "only_t / skip_ops with a foreign given operator: T is then a sum of materialised matrices");
    // nothing given is built; with a foreign operand T is not the kernel's business either (it is the device sparse add of the four)
    pl.skip |= pl.given | (pl.foreign ? 1u : 0u);
    for (int m = 1; m < 5; ++m)
        if ((pl.given >> m) & 1u) ctx->given_state[m] = ((pl.read >> m) & 1u) ? 3 : (((pl.derived >> m) & 1u) ? 1 : 2);
    return OTMB_OK;
}

// The foreign path of otmb_tm_args.given: T = ((Tadv + TκH) + TκVML) + TκVdeep (:147) from four materialised operands -- the ones the fill
// pass has just written into the caller's arrays and the GIVEN ones where they lie -- by SparseArrays' `+` on the device (otmb_spadd.hip:
// per column a sorted merge, a missing operand is +0.0, exact-zero results are dropped), left to right, through two temporaries.
int32_t otmb_tm_foreign_sum(otmb_ctx *ctx, TmPlan &pl, const TmParams &p) {
    const otmb_tm_args &a = pl.args;
    const i64 n = a.n_wet;
    if (pl.wet_base != 0 || pl.nnz_base[0] != 0) return otmb_fail(ctx, OTMB_ERR_GIVEN_FOREIGN, "depth slab");
    otmb_csc op[5];
    for (int m = 1; m < 5; ++m) {
        if ((pl.given >> m) & 1u) op[m] = a.given[m];
        else { op[m].colptr = p.colptr[m]; op[m].rowval = p.rowval[m]; op[m].nzval = p.nzval[m]; op[m].nnz = pl.built_nnz[m]; }
    }
    int32_t rc;
    otmb_csc acc = op[1];
    for (int step = 2; step < 5; ++step) {
        int64_t k = 0;
        if ((rc = otmb_spadd_plan_dev(ctx, n, acc.colptr, acc.rowval, acc.nzval, op[step].colptr, op[step].rowval, op[step].nzval, &k))) return rc;
        i64 *Cp, *Ci;
        double *Cx;
        if (step == 4) {  // the last add lands in the caller's T arrays (planned at the sum of the operands' counts: k cannot exceed it)
            if (k > pl.nnz[0]) return otmb_fail(ctx, OTMB_ERR_CAPACITY, "T");
            Cp = p.colptr[0]; Ci = p.rowval[0]; Cx = p.nzval[0];
        } else {
            DevBuf *t = &ctx->given_tmp[(step - 2) * 3];
            if ((rc = otmb_reserve(ctx, t[0], (size_t)(n + 1) * 8)) || (rc = otmb_reserve(ctx, t[1], (size_t)(k > 0 ? k : 1) * 8)) ||
                (rc = otmb_reserve(ctx, t[2], (size_t)(k > 0 ? k : 1) * 8)))
                return rc;
            Cp = (i64 *)t[0].p; Ci = (i64 *)t[1].p; Cx = (double *)t[2].p;
        }
        if ((rc = otmb_spadd_fill_dev(ctx, n, acc.colptr, acc.rowval, acc.nzval, op[step].colptr, op[step].rowval, op[step].nzval, Cp, Ci, Cx))) return rc;
        acc.colptr = Cp; acc.rowval = Ci; acc.nzval = Cx; acc.nnz = k;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    pl.nnz[0] = acc.nnz;
    return OTMB_OK;
}
