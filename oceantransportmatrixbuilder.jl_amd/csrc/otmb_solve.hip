// otmb_solve.hip -- (σ·I + diag(d) + A)·X = B and (σ·I + diag(d) + Aᵀ)·X = B on a resident operator: BiCGStab, right-preconditioned with
// P = diag(M) (Jacobi) or with M's part on the operator's lines.  The reference's use: Γ_c = (T_c + M_c) \ (LUMP * ones(N)),
// test/local_full.jl:151-188.  Entry points: otmb_op_solve_pc[_dev], the preconditioner its last argument (otmb_op_solve[_dev] are this call
// with OTMB_PRECOND_JACOBI), and otmb_op_precond[_dev], P⁻¹ alone; the host variants stage B, X and d (otmb_op.h) around the _dev ones.
//
// Per column (k columns advance together, every one with its own scalars; a stopped column is frozen: nothing of it is written again):
//     r = b - M·x (x = x0 or 0), r̂ = r, ρ = r̂·r, restart
//     p = restart ? r : r + β·(p - ω·v);  p̂ = p ./ diag                                (kernel 1, sv_p_kernel)
//     v = M·p̂;  α = ρ / (r̂·v)                                                          (kernel 2, sv_rows / sv_cols / sv_long, mode 0)
//     s = r - α·v;  ŝ = s ./ diag;  ‖s‖²                                               (kernel 3, sv_s_kernel)
//     t = M·ŝ;  ω = (t·s) / (t·t), or 0 when ‖s‖ ≤ rtol·‖b‖ already                    (kernel 4, mode 1)
//     x = (x + α·p̂) + ω·ŝ;  r = s - ω·t;  ρ' = r̂·r, ‖r‖²;  β = (ρ'/ρ)·(α/ω)            (kernel 5, sv_x_kernel)
//     ‖r‖ ≤ rtol·‖b‖: r = b - M·x again (mode 2): the column stops as converged when that TRUE residual passes, otherwise it goes on from
//     the true residual with r̂ = r (restart).
//     |ρ'| ≤ 2⁻⁵²·‖r̂‖·‖r‖: ρ' is no more than the rounding error of its own sum (exactly zero included), and β, the next p and α would be
//     noise.  The column takes the same path: true residual, r̂ = r.  This is not rare here: the transport matrix conserves mass (1ᵀ·T = 0),
//     so for B = 1 and M = σ·I + T the first r̂ is a left eigenvector of M, r̂·r_j is σ-polynomial times ‖b‖² in exact arithmetic and BiCG's
//     shadow space never grows; measured on the CPU restatement (tests/solve_ref.py), the one-month system on tiny_bipolar stalls at
//     ‖r‖/‖b‖ = 3.2e-6 with |ρ| ~ 1e-20 and then meets ρ = 0 exactly at iteration 284 without this rule, and converges in 253 with it.
// M·z is the operator's product with the (σ + d_i)·z_i term added last, in the same lane: one fold per row (adjoint: per column) in
// storage order, over the same layouts by the same walks as the products (otmb_op_fold.h; the layouts: the head of otmb_spmv.hip).  The
// long rows' kernel runs before the slices' kernel, which then takes their finished value into its dot products.  No FMA
// (-ffp-contract=off).
//
// Every reduction is deterministic: the grid of a kernel depends on n alone, a workgroup sums with a fixed tree (xor shuffles inside a
// wave, the four waves in order: otmb_op_sum.h, the one copy, which the periodic state's kernels use as well), writes ONE partial per
// column and quantity, and one workgroup per column (sv_scalar_kernel) folds the partials -- lane t takes t, t + 256, ... in index
// order, then the same tree -- and computes α, β, ω, ρ and the column's state in device memory, where the next kernel reads them.  No
// floating-point atomics.  A column's arithmetic never sees another column: column c of a k-column solve has the bits of that column
// solved alone.
//
// The host enqueues SV_POLL iterations (plain stream launches), then reads the k column records; it stops when every column has.
// A column stops with: converged (true residual checked) | maxiter | breakdown (r̂·v = 0, t·t = 0, ω = 0) | nonfinite (any scalar).
// X then holds the LAST iterate (a stop between kernels 2 and 5 leaves the previous one: x and r are only ever written together).
//
// otmb_op_solve_pc with OTMB_PRECOND_LINES: P is the part of M on the operator's lines (otmb_op_set_lines; otmb_solve_lines.hip states the
// factorisation and the sweep).  Kernels 1 and 3 then leave p̂ and ŝ to a line sweep launched after them (p̂ = P⁻¹·p, ŝ = P⁻¹·s); ‖s‖² still
// comes from kernel 3's own grid.  Everything else, the Jacobi path's bits included, is as above.
//
// otmb_op_solve_dk[_dev], otmb_op_precond_dk[_dev]: every column with its own d (D, n x k with leading dimension ldd; SvD).  The
// preconditioner's arrays are then per column (SvPrec: column c at + c·cs, cs = n), and the kernels that read sh or diag take that stride
// and are templates on PC (sv_pc, otmb_solve.h): with one d for all columns (ldd = 0: the exports above, which are these calls) the host
// launches the PC = false instantiation, which reads the one sh[i] or diag[i] once for its register block and does not use the stride.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cmath>

#include "otmb_op_fold.h"
#include "otmb_op_sum.h"
#include "otmb_solve.h"

#define SV_POLL 16  // iterations enqueued between two reads of the column records

enum { SV_S_INIT = 0, SV_S_VERIFY, SV_S_ALPHA, SV_S_OMEGA, SV_S_RHO };

// ---- sums: the workgroup's tree and its place in the partials are otmb_op_sum.h's (op_wave_sum, op_block_sum, op_put) ------------------------
template <int KB>
__device__ __forceinline__ bool sv_any(const SvCol *__restrict__ cs, int want) {
    bool any = false;
#pragma unroll
    for (int c = 0; c < KB; ++c) any |= cs[c].state == want;
    return any;
}

// ---- setup ---------------------------------------------------------------------------------------------------------------------
// sh = σ + d, diag = sh + the stored entries (i, i) of column i in storage order, for tracer column blockIdx.y + c0 (its d at + column·ldd,
// its sh and diag at + column·cs); bad = the smallest (column << 32 | i) whose diag is zero or not finite: with one d for all, the first i
__global__ __launch_bounds__(256) void sv_diag_kernel(const i64 *__restrict__ cp, const int *__restrict__ rv, const double *__restrict__ nz, i64 n,
                                                      const double *__restrict__ d, i64 ldd, double sigma, double *__restrict__ sh,
                                                      double *__restrict__ diag, i64 cs, i64 c0, unsigned long long *__restrict__ bad) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long c = (unsigned long long)(c0 + blockIdx.y);
    const double s0 = d ? sigma + d[i + (i64)c * ldd] : sigma;
    double acc = s0;
    for (i64 j = cp[i] - 1; j < cp[i + 1] - 1; ++j)
        if (rv[j] == (int)i) acc = acc + nz[j];
    sh[i + (i64)c * cs] = s0;
    diag[i + (i64)c * cs] = acc;
    if (acc == 0.0 || !isfinite(acc)) atomicMin(bad, c << 32 | (unsigned long long)i);
}
// ‖b‖² partials
template <int KB>
__global__ __launch_bounds__(256) void sv_bnorm_kernel(i64 n, const double *__restrict__ B, i64 ldb, double *__restrict__ part, i64 np) {
    __shared__ double red[4 * KB];
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double q[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        const double b = i < n ? B[i + c * ldb] : 0.0;
        q[c] = b * b;
    }
    op_block_sum<KB>(q, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < KB; ++c) part[(i64)(2 * c) * np + blockIdx.x] = q[c];
    }
}
// x = 0 unless a start was given (and b is not zero: b = 0 gives x = 0)
template <int KB>
__global__ __launch_bounds__(256) void sv_x0_kernel(const SvCol *__restrict__ cs, i64 n, int use_x0, double *__restrict__ X, i64 ldx) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int c = 0; c < KB; ++c)
        if (!use_x0 || cs[c].bzero) X[i + c * ldx] = 0.0;
}

// ---- kernel 1: p = r + β·(p - ω·v), p̂ = p ./ diag (restart: p = r, r̂ = r) ---------------------------------------------------------
// LINES: p̂ is left to the line sweep that follows (ln_sweep: p̂ = P⁻¹·p); likewise ŝ in kernel 3.
// (diag: PC: column c's at + c·ds, as in kernel 3; otherwise one for all)
template <int KB, bool LINES, bool PC>
__global__ __launch_bounds__(256) void sv_p_kernel(const SvCol *__restrict__ cs, i64 n, const double *__restrict__ diag, i64 ds, const double *__restrict__ r,
                                                   double *__restrict__ rh, double *__restrict__ p, const double *__restrict__ v,
                                                   double *__restrict__ ph) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double dg1 = LINES || PC ? 1.0 : diag[i];  // the one divisor of all columns
    double dg[KB];  // (loaded ahead of the loop: the loads are in flight while the records are read)
#pragma unroll
    for (int c = 0; c < KB; ++c) dg[c] = PC && !LINES ? diag[i + c * ds] : dg1;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        if (cs[c].state != SV_ACTIVE) continue;
        const i64 e = i + c * n;
        const double rr = r[e];
        double pn;
        if (cs[c].restart) {
            pn = rr;
            rh[e] = rr;
        } else {
            const double w = cs[c].omega * v[e];
            const double u = cs[c].beta * (p[e] - w);
            pn = rr + u;
        }
        p[e] = pn;
        if (!LINES) ph[e] = pn / dg[c];
    }
}

// ---- kernels 2 and 4, and the true residual: W = M·Z (modes 0, 1) or U - M·Z (mode 2) -------------------------------------------
// mode 0: partial of U·W (U = r̂);  mode 1: partials of W·U (U = s) and W·W;  mode 2: partial of W·W.
// Only columns in state `want` are written.  part: [column][2][np].  sh: PC: column c's σ + d at + c·shs; otherwise one for all.
template <int KB, int MODE>
__device__ __forceinline__ void sv_finish(const SvCol *__restrict__ cs, int want, bool has, bool store, i64 i, const double (&y)[KB],
                                          const double *__restrict__ U, i64 ldu, double *__restrict__ W, i64 ldw, double (&q)[2 * KB]) {
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        q[2 * c] = 0.0;
        q[2 * c + 1] = 0.0;
        if (!has) continue;
        const double u = U[i + c * ldu];
        // a long row's value was finished by sv_long_kernel (store == false): it is taken as it lies
        const double w = store ? (MODE == 2 ? u - y[c] : y[c]) : W[i + c * ldw];
        if (store && cs[c].state == want) W[i + c * ldw] = w;
        if (MODE == 0) q[2 * c] = u * w;
        if (MODE == 1) { q[2 * c] = w * u; q[2 * c + 1] = w * w; }
        if (MODE == 2) q[2 * c] = w * w;
    }
}

template <int KB, int MODE, bool PC>
__global__ __launch_bounds__(256) void sv_rows_kernel(const SvCol *__restrict__ cs, int want, const double *__restrict__ val, const int *__restrict__ col,
                                                      const i64 *__restrict__ sbase, const int *__restrict__ elen, i64 n, const double *__restrict__ sh,
                                                      i64 shs, const double *__restrict__ Z, i64 ldz, const double *__restrict__ U, i64 ldu,
                                                      double *__restrict__ W, i64 ldw, double *__restrict__ part, i64 np) {
    __shared__ double red[4 * 2 * KB];
    if (!sv_any<KB>(cs, want)) return;  // (uniform over the grid)
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const bool has = i < n;
    const int len = has ? elen[i] : 0;
    double y[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) y[c] = 0.0;
    if (has && len >= 0) {
        op_fold_slice_row(val, col, sbase, i, len, [&](double a, i64 j) {
#pragma unroll
            for (int c = 0; c < KB; ++c) y[c] = y[c] + a * Z[j + c * ldz];
        });
#pragma unroll
        for (int c = 0; c < KB; ++c) y[c] = y[c] + sh[i + sv_pc<PC>(c, shs)] * Z[i + c * ldz];
    }
    double q[2 * KB];
    sv_finish<KB, MODE>(cs, want, has, len >= 0, i, y, U, ldu, W, ldw, q);
    op_block_sum<2 * KB>(q, red);
    if (threadIdx.x == 0) op_put<2 * KB>(part, np, q);
}

// one workgroup per long row, lane c folds column c; runs BEFORE sv_rows_kernel, which sums its value
template <int MODE, bool PC>
__global__ __launch_bounds__(64) void sv_long_kernel(const SvCol *__restrict__ cs, int want, const double *__restrict__ val, const int *__restrict__ col,
                                                     const i64 *__restrict__ lrows, const i64 *__restrict__ loff, i64 ell, int k,
                                                     const double *__restrict__ sh, i64 shs, const double *__restrict__ Z, i64 ldz,
                                                     const double *__restrict__ U, i64 ldu, double *__restrict__ W, i64 ldw) {
    __shared__ double sv[SP_TCH];
    __shared__ int sc[SP_TCH];
    const int lane = threadIdx.x;
    const i64 i = lrows[blockIdx.x];
    const i64 b0 = ell + loff[i], len = loff[i + 1] - loff[i];
    for (int c0 = 0; c0 < k; c0 += 64) {
        const int c = c0 + lane;
        const bool on = c < k && cs[c].state == want;
        double acc = 0.0;
        op_fold_long_row(val, col, b0, len, sv, sc, lane, on, [&](double a, i64 j) { acc = acc + a * Z[j + c * ldz]; });
        if (on) {
            const double y = acc + sh[i + sv_pc<PC>(c, shs)] * Z[i + c * ldz];
            W[i + c * ldw] = MODE == 2 ? U[i + c * ldu] - y : y;
        }
    }
}

// the adjoint: one lane per column of A over the CSC copy, 64 columns per workgroup
template <int KB, int MODE, bool PC>
__global__ __launch_bounds__(64) void sv_cols_kernel(const SvCol *__restrict__ cs, int want, const i64 *__restrict__ cp, const int *__restrict__ rv,
                                                     const double *__restrict__ nz, i64 n, const double *__restrict__ sh, i64 shs,
                                                     const double *__restrict__ Z, i64 ldz, const double *__restrict__ U, i64 ldu, double *__restrict__ W, i64 ldw,
                                                     double *__restrict__ part, i64 np) {
    __shared__ double sv[SP_TCH];
    __shared__ int sr[SP_TCH];
    if (!sv_any<KB>(cs, want)) return;
    const int lane = threadIdx.x;
    i64 colm;
    double y[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) y[c] = 0.0;
    const bool has = op_fold_csc_run(cp, rv, nz, n, sv, sr, (i64)blockIdx.x * 64, lane, colm, [&](double a, i64 r) {
#pragma unroll
        for (int c = 0; c < KB; ++c) y[c] = y[c] + a * Z[r + c * ldz];
    });
    if (has) {
#pragma unroll
        for (int c = 0; c < KB; ++c) y[c] = y[c] + sh[colm + sv_pc<PC>(c, shs)] * Z[colm + c * ldz];
    }
    double q[2 * KB];
    sv_finish<KB, MODE>(cs, want, has, true, colm, y, U, ldu, W, ldw, q);
#pragma unroll
    for (int j = 0; j < 2 * KB; ++j) q[j] = op_wave_sum(q[j]);
    if (lane == 0) op_put<2 * KB>(part, np, q);
}

// ---- kernel 3: s = r - α·v, ŝ = s ./ diag, ‖s‖² ------------------------------------------------------------------------------------
template <int KB, bool LINES, bool PC>
__global__ __launch_bounds__(256) void sv_s_kernel(const SvCol *__restrict__ cs, i64 n, const double *__restrict__ diag, i64 ds, const double *__restrict__ r,
                                                   const double *__restrict__ v, double *__restrict__ s, double *__restrict__ sh_, double *__restrict__ part,
                                                   i64 np) {
    __shared__ double red[4 * KB];
    if (!sv_any<KB>(cs, SV_ACTIVE)) return;
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const double dg1 = !LINES && !PC && i < n ? diag[i] : 1.0;  // the one divisor of all columns
    double q[KB], dg[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) dg[c] = PC && !LINES && i < n ? diag[i + c * ds] : dg1;
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        q[c] = 0.0;
        if (i >= n || cs[c].state != SV_ACTIVE) continue;
        const i64 e = i + c * n;
        const double av = cs[c].alpha * v[e];
        const double sn = r[e] - av;
        s[e] = sn;
        if (!LINES) sh_[e] = sn / dg[c];
        q[c] = sn * sn;
    }
    op_block_sum<KB>(q, red);
    if (threadIdx.x == 0) op_put<KB>(part, np, q);
}

// ---- kernel 5: x = (x + α·p̂) + ω·ŝ, r = s - ω·t, partials of r̂·r and ‖r‖² --------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(256) void sv_x_kernel(const SvCol *__restrict__ cs, i64 n, const double *__restrict__ ph, const double *__restrict__ sh_,
                                                   const double *__restrict__ s, const double *__restrict__ t, const double *__restrict__ rh,
                                                   double *__restrict__ r, double *__restrict__ X, i64 ldx, double *__restrict__ part, i64 np) {
    __shared__ double red[4 * 2 * KB];
    if (!sv_any<KB>(cs, SV_ACTIVE)) return;
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    double q[2 * KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) {
        q[2 * c] = 0.0;
        q[2 * c + 1] = 0.0;
        if (i >= n || cs[c].state != SV_ACTIVE) continue;
        const i64 e = i + c * n;
        const double al = cs[c].alpha, om = cs[c].omega;
        const double ap = al * ph[e];
        const double os = om * sh_[e];
        const double x1 = X[i + c * ldx] + ap;
        X[i + c * ldx] = x1 + os;
        const double ot = om * t[e];
        const double rn = s[e] - ot;
        r[e] = rn;
        q[2 * c] = rh[e] * rn;
        q[2 * c + 1] = rn * rn;
    }
    op_block_sum<2 * KB>(q, red);
    if (threadIdx.x == 0) op_put<2 * KB>(part, np, q);
}

// ---- the scalars: workgroup c folds column c's partials and advances its record --------------------------------------------------
__device__ __forceinline__ void sv_stop(SvCol &s, int reason) {
    s.state = SV_STOPPED;
    s.reason = reason;
}
// part: [column][2][np] (nb of them written), parts: [column][np] (kernel 3's ‖s‖², nbs written)
__global__ __launch_bounds__(256) void sv_scalar_kernel(SvCol *__restrict__ cs, int step, const double *__restrict__ part, i64 np, i64 nb,
                                                        const double *__restrict__ parts, i64 nbs, double rtol, i64 maxiter) {
    __shared__ double red[4 * 3];
    SvCol &s = cs[blockIdx.x];
    const int want = step == SV_S_INIT ? -1 : (step == SV_S_VERIFY ? SV_VERIFY : SV_ACTIVE);
    if (want >= 0 && s.state != want) return;  // (uniform over the workgroup)
    const double *p0 = part + (i64)(2 * blockIdx.x) * np, *p1 = p0 + np, *p2 = parts + (i64)blockIdx.x * np;
    double f[3] = {0.0, 0.0, 0.0};
    for (i64 j = threadIdx.x; j < nb; j += 256) {
        f[0] = f[0] + p0[j];
        if (step == SV_S_OMEGA || step == SV_S_RHO) f[1] = f[1] + p1[j];
    }
    if (step == SV_S_OMEGA)
        for (i64 j = threadIdx.x; j < nbs; j += 256) f[2] = f[2] + p2[j];
    op_block_sum<3>(f, red);
    if (threadIdx.x != 0) return;
    const double bn = s.bnorm;
    switch (step) {
        case SV_S_INIT: {  // f[0] = ‖b‖²
            s.bnorm = sqrt(f[0]);
            s.bzero = f[0] == 0.0;
            s.rho = s.alpha = s.omega = 1.0;
            s.beta = 0.0;
            s.relres = 0.0;
            s.iters = 0;
            s.restart = 1;
            s.reason = 0;
            s.state = SV_VERIFY;
            break;
        }
        case SV_S_VERIFY: {  // f[0] = ‖b - M·x‖², explicitly computed
            const double rn = sqrt(f[0]);
            if (s.bzero) {
                s.relres = 0.0;
                sv_stop(s, OTMB_SOLVE_CONVERGED);
                break;
            }
            s.relres = rn / bn;
            if (!isfinite(bn) || !isfinite(rn)) sv_stop(s, OTMB_SOLVE_NONFINITE);
            else if (rn <= rtol * bn) sv_stop(s, OTMB_SOLVE_CONVERGED);
            else if (s.iters >= maxiter) sv_stop(s, OTMB_SOLVE_MAXITER);
            else {  // on from the true residual: r̂ = r, ρ = r·r, p = r
                s.state = SV_ACTIVE;
                s.restart = 1;
                s.rho = f[0];
                s.rhn = rn;
            }
            break;
        }
        case SV_S_ALPHA: {  // f[0] = r̂·v
            if (!isfinite(f[0])) sv_stop(s, OTMB_SOLVE_NONFINITE);
            else if (f[0] == 0.0) sv_stop(s, OTMB_SOLVE_BREAKDOWN);
            else {
                s.alpha = s.rho / f[0];
                if (!isfinite(s.alpha)) sv_stop(s, OTMB_SOLVE_NONFINITE);
            }
            break;
        }
        case SV_S_OMEGA: {  // f[0] = t·s, f[1] = t·t, f[2] = ‖s‖²
            if (!isfinite(f[0]) || !isfinite(f[1]) || !isfinite(f[2])) sv_stop(s, OTMB_SOLVE_NONFINITE);
            else if (sqrt(f[2]) <= rtol * bn) s.omega = 0.0;  // s is already small enough: x += α·p̂, r = s, then the true residual decides
            else if (f[1] == 0.0) sv_stop(s, OTMB_SOLVE_BREAKDOWN);
            else {
                s.omega = f[0] / f[1];
                if (!isfinite(s.omega)) sv_stop(s, OTMB_SOLVE_NONFINITE);
            }
            break;
        }
        case SV_S_RHO: {  // f[0] = r̂·r, f[1] = ‖r‖²: the iteration is complete
            s.iters += 1;
            const double rn = sqrt(f[1]);
            s.relres = rn / bn;
            if (!isfinite(f[0]) || !isfinite(f[1])) sv_stop(s, OTMB_SOLVE_NONFINITE);
            else if (rn <= rtol * bn) s.state = SV_VERIFY;
            else if (s.iters >= maxiter) sv_stop(s, OTMB_SOLVE_MAXITER);
            else if (fabs(f[0]) <= 0x1p-52 * s.rhn * rn) s.state = SV_VERIFY;  // ρ' is lost in the rounding of its own sum (zero included): a new r̂
            else if (s.omega == 0.0) sv_stop(s, OTMB_SOLVE_BREAKDOWN);
            else {
                const double a = f[0] / s.rho, b = s.alpha / s.omega;
                s.beta = a * b;
                s.rho = f[0];
                s.restart = 0;
                if (!isfinite(s.beta)) sv_stop(s, OTMB_SOLVE_NONFINITE);
            }
            break;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct SvWork {  // the solver's device arrays inside op->sw
    SvPrec pc;    // the preconditioner the kernels read: the workspace's own block, or one prepared elsewhere (sv_solve)
    double *r, *rh, *p, *v, *s, *t, *ph, *sh_, *part, *parts;
    SvCol *cs;
    unsigned long long *bad;  // the setup's scratch (sv_precond_setup): [2] flags, the diagonal's and the pivots', then l
    i64 np;
};
// the setup's scratch for a preconditioner of kc columns: two flags and, behind them, the n doubles of l where the factorisation reads l
// from there: the lines with several columns (one column passes l through m: ln_factor)
static size_t sv_setup_doubles(i64 n, bool lines, i64 kc) { return 2 + (lines && kc > 1 ? (size_t)n : 0); }
// selects the operator's device, reserves op->sw and carves it for k columns (k = 0: the preconditioner's arrays alone, otmb_op_precond_dev)
// with np = (n + 63) / 64 partials per column and quantity: the adjoint's kernels write np of them, the rows' and the vector kernels fewer.
// kc: the columns of the workspace's own preconditioner (sv_prec_cols; 0: none, the caller brings a prepared one: sv_solve).  The layout,
// in doubles, every size computed here once:
//     pre (sh | diag | m | piv | u of kc columns) | 8 vectors of n·k | part: 2·np·k | parts: np·k | setup (flags, l) | the k records
// kc = 0 keeps the block of ONE column in front, unused, so that the vectors lie where they lie in a call that makes its own preconditioner.
static int32_t sv_work(otmb_op *op, int32_t precond, i64 k, i64 kc, bool percol, SvWork &w) {
    HIP_TRY(op->ctx, hipSetDevice(op->device));
    const bool lines = precond == OTMB_PRECOND_LINES;
    const i64 pcols = std::max<i64>(kc, 1);
    const size_t n = (size_t)op->n, vec = n * (size_t)k, np = (n + 63) / 64, parts = np * (size_t)k;
    const size_t pre = sv_prec_doubles(op->n, lines, pcols), setup = sv_setup_doubles(op->n, lines, kc);
    int32_t rc;
    if ((rc = otmb_reserve(op->ctx, op->sw, (pre + 8 * vec + 3 * parts + setup) * 8 + (size_t)k * sizeof(SvCol) + 64))) return rc;
    double *q = (double *)op->sw.p;
    w.pc = sv_prec_carve(q, op->n, lines, pcols, percol); q += pre;
    for (double **v : {&w.r, &w.rh, &w.p, &w.v, &w.s, &w.t, &w.ph, &w.sh_}) { *v = q; q += vec; }
    w.part = q; q += 2 * parts;
    w.parts = q; q += parts;
    w.bad = (unsigned long long *)q; q += setup;
    w.cs = (SvCol *)q;
    w.np = (i64)np;
    return OTMB_OK;
}

// Z = Y ./ diag: the Jacobi preconditioner on its own (otmb_op_precond)
template <int KB, bool PC>
__global__ __launch_bounds__(256) void sv_scale_kernel(i64 n, const double *__restrict__ diag, i64 ds, const double *Y, i64 ldy, double *Z, i64 ldz) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double dg[KB];  // (ahead of the stores: Y and Z may be one array, so no load would move across them)
#pragma unroll
    for (int c = 0; c < KB; ++c) dg[c] = diag[i + sv_pc<PC>(c, ds)];
#pragma unroll
    for (int c = 0; c < KB; ++c) Z[i + c * ldz] = Y[i + c * ldy] / dg[c];
}

// p's arrays -- sh and diag and, with lines, u, the multipliers and the pivots, p.kc columns of all but u -- with flags (device:
// sv_setup_doubles of scratch, the two flags first) for the verdict: a singular preconditioner is refused here, before anything of the
// caller's is touched.  Waits for the device.
static int32_t sv_precond_setup(otmb_op *op, int adjoint, int32_t precond, const SvD &d, double sigma, const SvPrec &p, unsigned long long *flags) {
    otmb_ctx *ctx = op->ctx;
    hipStream_t st = ctx->stream;
    const i64 n = op->n;
    HIP_TRY(ctx, hipMemsetAsync(flags, 0xff, 16, st));
    for (i64 c0 = 0; c0 < p.kc; c0 += 65535)  // (a grid's y extent)
        hipLaunchKernelGGL(sv_diag_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min<i64>(p.kc - c0, 65535)), dim3(256), 0, st,
                           (const i64 *)op->cp.p, (const int *)op->rv.p, (const double *)op->nz.p, n, d.p, d.percol() ? d.ld : 0, sigma, p.sh, p.diag, p.cs,
                           c0, flags);
    if (precond == OTMB_PRECOND_LINES) ln_factor(op, adjoint, p, (double *)(flags + 2), flags + 1);
    HIP_TRY(ctx, hipGetLastError());
    unsigned long long bad[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(bad, flags, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    const int lines = precond == OTMB_PRECOND_LINES;  // the flag that decides: the pivots' with lines, otherwise the diagonal's
    if (bad[lines] == ~0ull) return OTMB_OK;
    char msg[128], col[64] = "";
    snprintf(msg, sizeof msg, lines ? "pivot[%lld] of the line factorisation is zero or not finite (1-based; the smallest such index)"
                                    : "diag(M)[%lld] is zero or not finite (1-based; the first such index)", (long long)(bad[lines] & 0xffffffffull) + 1);
    if (p.cs) snprintf(col, sizeof col, " (column %lld of %lld)", (long long)(bad[lines] >> 32) + 1, (long long)p.kc);
    return otmb_fail(ctx, OTMB_ERR_SINGULAR_PRECONDITIONER, (std::string(msg) + col).c_str());
}

int32_t sv_check_d(otmb_op *op, const char *call, const double *D, int64_t ldd) {
    if (!D || ldd == 0 || ldd >= op->n) return OTMB_OK;
    return otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, (std::string(call) + ": ldd must be 0 (the n values at D serve every column) or >= n").c_str());
}

// The same into arrays of the caller's (otmb_op_step keeps one set per slot it visits); op->sw lends the setup's scratch only, at its start
// (it is reserved at the size of a workspace without columns, sv_work's k = 0).
int32_t sv_prec_prepare(otmb_op *op, int adjoint, int32_t precond, const SvD &d, double sigma, const SvPrec &p) {
    const bool lines = precond == OTMB_PRECOND_LINES;
    int32_t rc;
    if ((rc = otmb_reserve(op->ctx, op->sw, (sv_prec_doubles(op->n, lines, p.kc) + sv_setup_doubles(op->n, lines, p.kc)) * 8 + 64))) return rc;
    return sv_precond_setup(op, adjoint, precond, d, sigma, p, (unsigned long long *)op->sw.p);
}

// W = M·Z (modes 0, 1) or U - M·Z (mode 2) for the columns in state `want`, with the partials of the mode's dot products
template <int MODE, bool PC>
static void sv_apply_pc(otmb_op *op, const SvWork &w, int adjoint, i64 k, int want, const double *Z, i64 ldz, const double *U, i64 ldu, double *W, i64 ldw) {
    hipStream_t st = op->ctx->stream;
    const i64 n = op->n;
    if (!adjoint && op->nlong > 0)
        hipLaunchKernelGGL((sv_long_kernel<MODE, PC>), dim3((unsigned)op->nlong), dim3(64), 0, st, (const SvCol *)w.cs, want, (const double *)op->val.p,
                           (const int *)op->col.p, (const i64 *)op->lrows.p, (const i64 *)op->loff.p, op->ell, (int)k, (const double *)w.pc.sh, w.pc.cs, Z, ldz, U,
                           ldu, W, ldw);
    op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
        constexpr int KB = decltype(kb)::value;
        if (adjoint)
            hipLaunchKernelGGL((sv_cols_kernel<KB, MODE, PC>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, (const SvCol *)w.cs + c0, want,
                               (const i64 *)op->cp.p, (const int *)op->rv.p, (const double *)op->nz.p, n, (const double *)w.pc.sh + c0 * w.pc.cs, w.pc.cs, Z + c0 * ldz, ldz,
                               U + c0 * ldu, ldu, W + c0 * ldw, ldw, w.part + 2 * c0 * w.np, w.np);
        else
            hipLaunchKernelGGL((sv_rows_kernel<KB, MODE, PC>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const SvCol *)w.cs + c0, want,
                               (const double *)op->val.p, (const int *)op->col.p, (const i64 *)op->sbase.p, (const int *)op->elen.p, n,
                               (const double *)w.pc.sh + c0 * w.pc.cs, w.pc.cs, Z + c0 * ldz, ldz, U + c0 * ldu, ldu, W + c0 * ldw, ldw,
                               w.part + 2 * c0 * w.np, w.np);
    });
}

template <int MODE>
static void sv_apply(otmb_op *op, const SvWork &w, int adjoint, i64 k, int want, const double *Z, i64 ldz, const double *U, i64 ldu, double *W, i64 ldw) {
    if (w.pc.cs) sv_apply_pc<MODE, true>(op, w, adjoint, k, want, Z, ldz, U, ldu, W, ldw);
    else sv_apply_pc<MODE, false>(op, w, adjoint, k, want, Z, ldz, U, ldu, W, ldw);
}

static void sv_scalar(otmb_op *op, const SvWork &w, i64 k, int step, i64 nb, double rtol, i64 maxiter) {
    hipLaunchKernelGGL(sv_scalar_kernel, dim3((unsigned)k), dim3(256), 0, op->ctx->stream, w.cs, step, (const double *)w.part, w.np, nb,
                       (const double *)w.parts, (op->n + 255) / 256, rtol, maxiter);
}

// r = b - M·x for the columns that wait for it, and their verdict
static void sv_verify(otmb_op *op, const SvWork &w, int adjoint, i64 k, const double *B, i64 ldb, double *X, i64 ldx, double rtol, i64 maxiter) {
    const i64 n = op->n;
    sv_apply<2>(op, w, adjoint, k, SV_VERIFY, X, ldx, B, ldb, w.r, n);
    sv_scalar(op, w, k, SV_S_VERIFY, adjoint ? (n + 63) / 64 : (n + 255) / 256, rtol, maxiter);
}

// The argument checks of otmb_op_solve_pc[_dev] (sv_check) and otmb_op_precond[_dev] (sv_check_apply), in one order: the matrices Y (ldy) and
// Z (ldz) named y and z, then `more`, the caller's first complaint about its other arguments (null: none), then the preconditioner.
static int32_t sv_check_system(otmb_op *op, int32_t precond, const char *what, const char *cols, char y, char z, i64 k, const double *Y, i64 ldy,
                               const double *Z, i64 ldz, const char *more) {
    const auto fail = [&](const std::string &m) { return otmb_fail(op->ctx, OTMB_ERR_INVALID_ARG, m.c_str()); };
    const auto small = [&](char c) { return fail(std::string("ld") + (char)tolower(c) + " is smaller than the rows of " + c); };
    if (op->m != op->n) return fail(std::string(what) + ": the operator's matrix must be square");
    if (k < 1 || k >= (1ll << 31)) return fail(std::string("k (") + cols + ") must be >= 1");
    if (ldy < op->n || ldy < 0) return small(y);
    if (ldz < op->n || ldz < 0) return small(z);
    if (op->n > 0 && (!Y || !Z)) return fail("null argument");
    if (more) return fail(more);
    if (precond != OTMB_PRECOND_JACOBI && precond != OTMB_PRECOND_LINES) return fail("precond must be OTMB_PRECOND_JACOBI or OTMB_PRECOND_LINES");
    if (precond == OTMB_PRECOND_LINES && !op->lines) return fail("OTMB_PRECOND_LINES needs lines: otmb_op_set_lines first");
    return OTMB_OK;
}
static int32_t sv_check(otmb_op *op, int32_t precond, int64_t k, const double *B, int64_t ldb, double *X, int64_t ldx, double rtol, int64_t maxiter,
                        const int64_t *iters, const double *relres, const int32_t *reason) {
    const char *more = !iters || !relres || !reason ? "null argument" : !(rtol > 0.0) ? "rtol must be > 0" : maxiter < 0 ? "maxiter must be >= 0" : nullptr;
    return sv_check_system(op, precond, "solve", "right-hand sides", 'B', 'X', k, B, ldb, X, ldx, more);
}
int32_t sv_check_step(otmb_op *op, int32_t precond, int64_t k, const double *S, int64_t lds, double *X, int64_t ldx, const char *more) {
    return sv_check_system(op, precond, "step", "tracers", 'S', 'X', k, S ? S : X, S ? lds : ldx, X, ldx, more);
}
const char *sv_step_complaint(const otmb_op *op, double rtol, int64_t maxiter, double dt, double theta, bool count_ok, const char *count_text,
                              int64_t first_slot) {
    return !(rtol > 0.0)                                           ? "rtol must be > 0"
           : maxiter < 0                                           ? "maxiter must be >= 0"
           : !(dt > 0.0) || !std::isfinite(dt)                     ? "dt must be > 0 and finite"
           : !(theta > 0.0 && theta <= 1.0)                        ? "theta must be in (0, 1]"
           : !count_ok                                             ? count_text
           : first_slot < 0 || first_slot >= (i64)op->slots.size() ? "first_slot is not a slot of the operator (otmb_op_set_slots)"
                                                                   : nullptr;
}
static int32_t sv_check_apply(otmb_op *op, int32_t precond, int64_t k, const double *Y, int64_t ldy, double *Z, int64_t ldz) {
    return sv_check_system(op, precond, "precond", "columns", 'Y', 'Z', k, Y, ldy, Z, ldz, nullptr);
}

int32_t sv_report_open(otmb_ctx *ctx, const char *fmt, const char *const *names, i64 k, const int32_t *reason, const int64_t *count, const double *value,
                       const std::string &tail, int nnames) {
    i64 open = 0, first = -1;
    for (i64 c = 0; c < k; ++c)
        if (reason[c] != 0 && open++ == 0) first = c;
    if (open == 0) return OTMB_OK;
    char msg[200];
    snprintf(msg, sizeof msg, fmt, (long long)open, (long long)k, (long long)first + 1, names[reason[first] >= 0 && reason[first] < nnames ? reason[first] : 0], (long long)count[first], value[first]);
    return otmb_fail(ctx, OTMB_ERR_NOT_CONVERGED, (msg + tail).c_str());
}

// The solve proper, behind otmb_op_solve_pc_dev and the step: w.pc is a prepared preconditioner (for this adjoint, precond, d, σ and the
// selected values), so a singular one was refused before this, with nothing of X touched.
static int32_t sv_iterate(otmb_op *op, const SvWork &w, int adjoint, i64 k, const double *B, i64 ldb, double *X, i64 ldx, int use_x0, double rtol,
                          i64 maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond) {
    const bool lines = precond == OTMB_PRECOND_LINES, pc = w.pc.cs != 0;  // (with lines kernels 1 and 3 read no diag: PC = false)
    otmb_ctx *ctx = op->ctx;
    hipStream_t st = ctx->stream;
    const i64 n = op->n, nb = (n + 255) / 256, np = w.np;
    const dim3 grid((unsigned)nb), block(256);
    // ‖b‖, the start, its true residual
    op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
        hipLaunchKernelGGL((sv_bnorm_kernel<decltype(kb)::value>), grid, block, 0, st, n, B + c0 * ldb, ldb, w.part + 2 * c0 * np, np);
    });
    sv_scalar(op, w, k, SV_S_INIT, nb, rtol, maxiter);
    op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
        hipLaunchKernelGGL((sv_x0_kernel<decltype(kb)::value>), grid, block, 0, st, (const SvCol *)w.cs + c0, n, (int)use_x0, X + c0 * ldx, ldx);
    });
    sv_verify(op, w, adjoint, k, B, ldb, X, ldx, rtol, maxiter);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<SvCol> h((size_t)k);
    auto running = [&]() -> int32_t {  // reads the records: 1 some column still runs, 0 none, < 0 a HIP error's status (negated)
        if (hipMemcpyAsync(h.data(), w.cs, (size_t)k * sizeof(SvCol), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return -1;
        for (const SvCol &c : h)
            if (c.state != SV_STOPPED) return 1;
        return 0;
    };
    const i64 nbm = adjoint ? np : nb;  // partials the operator's kernels write
    int32_t run = running();
    for (i64 done = 0; run == 1 && done < maxiter;) {
        const i64 batch = std::min<i64>(SV_POLL, maxiter - done);
        for (i64 it = 0; it < batch; ++it) {
            op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
                constexpr int KB = decltype(kb)::value;
                hipLaunchKernelGGL((lines ? sv_p_kernel<KB, true, false> : pc ? sv_p_kernel<KB, false, true> : sv_p_kernel<KB, false, false>), grid, block, 0, st, (const SvCol *)w.cs + c0, n,
                                   (const double *)w.pc.diag + c0 * w.pc.cs, w.pc.cs, (const double *)w.r + c0 * n, w.rh + c0 * n, w.p + c0 * n, (const double *)w.v + c0 * n,
                                   w.ph + c0 * n);
            });
            if (lines) ln_sweep(op, w.cs, k, w.pc, w.p, n, w.ph, n);
            sv_apply<0>(op, w, adjoint, k, SV_ACTIVE, w.ph, n, w.rh, n, w.v, n);
            sv_scalar(op, w, k, SV_S_ALPHA, nbm, rtol, maxiter);
            op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
                constexpr int KB = decltype(kb)::value;
                hipLaunchKernelGGL((lines ? sv_s_kernel<KB, true, false> : pc ? sv_s_kernel<KB, false, true> : sv_s_kernel<KB, false, false>), grid, block, 0, st, (const SvCol *)w.cs + c0, n,
                                   (const double *)w.pc.diag + c0 * w.pc.cs, w.pc.cs, (const double *)w.r + c0 * n, (const double *)w.v + c0 * n, w.s + c0 * n, w.sh_ + c0 * n,
                                   w.parts + c0 * np, np);
            });
            if (lines) ln_sweep(op, w.cs, k, w.pc, w.s, n, w.sh_, n);
            sv_apply<1>(op, w, adjoint, k, SV_ACTIVE, w.sh_, n, w.s, n, w.t, n);
            sv_scalar(op, w, k, SV_S_OMEGA, nbm, rtol, maxiter);
            op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
                hipLaunchKernelGGL((sv_x_kernel<decltype(kb)::value>), grid, block, 0, st, (const SvCol *)w.cs + c0, n, (const double *)w.ph + c0 * n,
                                   (const double *)w.sh_ + c0 * n, (const double *)w.s + c0 * n, (const double *)w.t + c0 * n,
                                   (const double *)w.rh + c0 * n, w.r + c0 * n, X + c0 * ldx, ldx, w.part + 2 * c0 * np, np);
            });
            sv_scalar(op, w, k, SV_S_RHO, nb, rtol, maxiter);
            sv_verify(op, w, adjoint, k, B, ldb, X, ldx, rtol, maxiter);
        }
        HIP_TRY(ctx, hipGetLastError());
        done += batch;
        run = running();
    }
    if (run < 0) return otmb_fail(ctx, OTMB_ERR_HIP, "solve: reading the column records");
    if (run == 1) return otmb_fail(ctx, OTMB_ERR_HIP, "solve: a column was still running after maxiter iterations");  // (cannot happen: sv_scalar_kernel stops it)
    for (i64 c = 0; c < k; ++c) {
        iters[c] = h[(size_t)c].iters;
        relres[c] = h[(size_t)c].relres;
        reason[c] = h[(size_t)c].reason;
    }
    static const char *const names[] = {"converged", "maxiter", "breakdown", "nonfinite"};
    return sv_report_open(ctx, "%lld of %lld columns; the first is column %lld: %s after %lld iterations, relative residual %.3e", names, k, reason, iters,
                          relres);
}

// The solve with a preconditioner prepared elsewhere (sv_prec_prepare): the step's, which keeps one per slot
int32_t sv_solve(otmb_op *op, int adjoint, i64 k, const SvPrec &p, const double *B, i64 ldb, double *X, i64 ldx, int use_x0, double rtol, i64 maxiter,
                 int64_t *iters, double *relres, int32_t *reason, int32_t precond) {
    SvWork w;
    int32_t rc;
    if ((rc = sv_work(op, precond, k, 0, false, w))) return rc;
    w.pc = p;
    return sv_iterate(op, w, adjoint, k, B, ldb, X, ldx, use_x0, rtol, maxiter, iters, relres, reason, precond);
}

extern "C" {

int32_t otmb_op_solve_dk_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double sigma, const double *B, int64_t ldb, double *X,
                             int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sv_check(op, precond, k, B, ldb, X, ldx, rtol, maxiter, iters, relres, reason)) || (rc = sv_check_d(op, "otmb_op_solve_dk", D, ldd))) return rc;
    if (op->n == 0) return sv_report_empty(k, iters, relres, reason);
    const SvD d = {D, ldd};
    SvWork w;
    if ((rc = sv_work(op, precond, k, sv_prec_cols(d, k), d.percol(), w)) || (rc = sv_precond_setup(op, adjoint, precond, d, sigma, w.pc, w.bad))) return rc;
    return sv_iterate(op, w, adjoint, k, B, ldb, X, ldx, use_x0, rtol, maxiter, iters, relres, reason, precond);
}

int32_t otmb_op_solve_dk(otmb_op *op, int32_t adjoint, int64_t k, const double *D, int64_t ldd, double sigma, const double *B, int64_t ldb, double *X,
                         int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sv_check(op, precond, k, B, ldb, X, ldx, rtol, maxiter, iters, relres, reason)) || (rc = sv_check_d(op, "otmb_op_solve_dk", D, ldd))) return rc;
    otmb_ctx *ctx = op->ctx;
    HIP_TRY(ctx, hipSetDevice(op->device));
    const i64 n = op->n;
    SvD dd;
    if ((rc = op_reserve_xy(op, n, n, k)) || (rc = op_stage_dk(op, D, ldd, k, dd.p, dd.ld))) return rc;
    double *db = (double *)op->xs.p, *dx = (double *)op->ys.p;
    if (n > 0) {
        if ((rc = op_upload(ctx, db, B, ldb, n, k))) return rc;
        if (use_x0 && (rc = op_upload(ctx, dx, X, ldx, n, k))) return rc;
    }
    rc = otmb_op_solve_dk_dev(op, adjoint, k, dd.p, dd.ld, sigma, db, n, dx, n, use_x0, rtol, maxiter, iters, relres, reason, precond);
    if (rc != OTMB_OK && rc != OTMB_ERR_NOT_CONVERGED) return rc;
    return op_finish(ctx, rc, X, ldx, dx, n, k);
}

// the calls with one d for every column: ldd = 0
int32_t otmb_op_solve_pc_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X,
                             int64_t ldx, int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond) {
    return otmb_op_solve_dk_dev(op, adjoint, k, d, 0, sigma, B, ldb, X, ldx, use_x0, rtol, maxiter, iters, relres, reason, precond);
}

int32_t otmb_op_solve_pc(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X, int64_t ldx,
                         int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason, int32_t precond) {
    return otmb_op_solve_dk(op, adjoint, k, d, 0, sigma, B, ldb, X, ldx, use_x0, rtol, maxiter, iters, relres, reason, precond);
}

int32_t otmb_op_solve_dev(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X, int64_t ldx,
                          int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason) {
    return otmb_op_solve_pc_dev(op, adjoint, k, d, sigma, B, ldb, X, ldx, use_x0, rtol, maxiter, iters, relres, reason, OTMB_PRECOND_JACOBI);
}

int32_t otmb_op_solve(otmb_op *op, int32_t adjoint, int64_t k, const double *d, double sigma, const double *B, int64_t ldb, double *X, int64_t ldx,
                      int32_t use_x0, double rtol, int64_t maxiter, int64_t *iters, double *relres, int32_t *reason) {
    return otmb_op_solve_pc(op, adjoint, k, d, sigma, B, ldb, X, ldx, use_x0, rtol, maxiter, iters, relres, reason, OTMB_PRECOND_JACOBI);
}

// Z = P⁻¹·Y: the preconditioner of otmb_op_solve_dk on its own
int32_t otmb_op_precond_dk_dev(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *D, int64_t ldd, double sigma, const double *Y,
                               int64_t ldy, double *Z, int64_t ldz) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sv_check_apply(op, precond, k, Y, ldy, Z, ldz)) || (rc = sv_check_d(op, "otmb_op_precond_dk", D, ldd))) return rc;
    otmb_ctx *ctx = op->ctx;
    const i64 n = op->n;
    if (n == 0) return OTMB_OK;
    const SvD d = {D, ldd};
    SvWork w;
    if ((rc = sv_work(op, precond, 0, sv_prec_cols(d, k), d.percol(), w)) || (rc = sv_precond_setup(op, adjoint, precond, d, sigma, w.pc, w.bad))) return rc;
    if (precond == OTMB_PRECOND_LINES)
        ln_sweep(op, nullptr, k, w.pc, Y, ldy, Z, ldz);
    else
        op_blocks<SV_KB>(0, k, [&](auto kb, i64 c0) {
            constexpr int KB = decltype(kb)::value;
            hipLaunchKernelGGL((w.pc.cs ? sv_scale_kernel<KB, true> : sv_scale_kernel<KB, false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n,
                               (const double *)w.pc.diag + c0 * w.pc.cs, w.pc.cs, Y + c0 * ldy, ldy, Z + c0 * ldz, ldz);
        });
    HIP_TRY(ctx, hipGetLastError());
    return OTMB_OK;
}

int32_t otmb_op_precond_dk(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *D, int64_t ldd, double sigma, const double *Y, int64_t ldy,
                           double *Z, int64_t ldz) {
    if (!op) return OTMB_ERR_INVALID_ARG;
    int32_t rc;
    if ((rc = sv_check_apply(op, precond, k, Y, ldy, Z, ldz)) || (rc = sv_check_d(op, "otmb_op_precond_dk", D, ldd))) return rc;
    otmb_ctx *ctx = op->ctx;
    const i64 n = op->n;
    if (n == 0) return OTMB_OK;
    HIP_TRY(ctx, hipSetDevice(op->device));
    SvD dd;
    if ((rc = op_reserve_xy(op, n, n, k)) || (rc = op_stage_dk(op, D, ldd, k, dd.p, dd.ld))) return rc;
    double *dy = (double *)op->xs.p, *dz = (double *)op->ys.p;
    if ((rc = op_upload(ctx, dy, Y, ldy, n, k))) return rc;
    if ((rc = otmb_op_precond_dk_dev(op, adjoint, precond, k, dd.p, dd.ld, sigma, dy, n, dz, n))) return rc;
    return op_finish(ctx, OTMB_OK, Z, ldz, dz, n, k);
}

int32_t otmb_op_precond_dev(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *d, double sigma, const double *Y, int64_t ldy,
                            double *Z, int64_t ldz) {
    return otmb_op_precond_dk_dev(op, adjoint, precond, k, d, 0, sigma, Y, ldy, Z, ldz);
}

int32_t otmb_op_precond(otmb_op *op, int32_t adjoint, int32_t precond, int64_t k, const double *d, double sigma, const double *Y, int64_t ldy, double *Z,
                        int64_t ldz) {
    return otmb_op_precond_dk(op, adjoint, precond, k, d, 0, sigma, Y, ldy, Z, ldz);
}

}  // extern "C"
