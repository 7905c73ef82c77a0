"""A numpy restatement of otmb_op_solve (csrc/otmb_solve.hip, include/otmb.h): BiCGStab, right-preconditioned with the Jacobi
preconditioner P = diag(M), for M = σ·I + diag(d) + A (adjoint: Aᵀ), one column at a time -- the same recurrences, stop rules and
reasons as the device code, with numpy's own summation order (so iteration counts and last bits differ from the device's).

    r = b - M·x, r̂ = r, ρ = r̂·r, restart
    p = restart ? r : r + β·(p - ω·v);  p̂ = p ./ diag;  v = M·p̂;  α = ρ / (r̂·v)
    s = r - α·v;  ŝ = s ./ diag;  t = M·ŝ;  ω = (t·s) / (t·t), or 0 when ‖s‖ ≤ rtol·‖b‖ already
    x = (x + α·p̂) + ω·ŝ;  r = s - ω·t;  ρ' = r̂·r;  β = (ρ'/ρ)·(α/ω)
    ‖r‖ ≤ rtol·‖b‖: the TRUE residual b - M·x decides: converged, or on from the true residual with r̂ = r.
    |ρ'| ≤ 2⁻⁵²·‖r̂‖·‖r‖ (ρ' is lost in the rounding of its own sum, zero included): likewise on from the true residual with r̂ = r.
Also here: the systems of the issue that introduced the solver (age, month, year), the matrices of the tests and the residual bound."""
import numpy as np
import scipy.sparse as sp

REASONS = ("converged", "maxiter", "breakdown", "nonfinite")
EPS = 2.0 ** -53
EPS52 = 2.0 ** -52
DAY = 86400.0


class SingularPreconditioner(ValueError):
    def __init__(self, index):
        super().__init__(f"diag(M)[{index + 1}] is zero or not finite")
        self.index = index


def csc_of(m, n, colptr, rowval, nzval):
    """scipy's CSC over Julia's 1-based arrays; duplicates are kept as stored (never summed)."""
    return sp.csc_matrix((np.asarray(nzval, dtype=np.float64), np.asarray(rowval, dtype=np.int64) - 1, np.asarray(colptr, dtype=np.int64) - 1),
                         shape=(m, n))


def system(A, d=None, sigma=0.0, adjoint=False):
    """M = σ·I + diag(d) + A (or Aᵀ) as a CSR matrix."""
    n = A.shape[0]
    dd = np.full(n, float(sigma)) + (0.0 if d is None else np.asarray(d, dtype=np.float64))
    return (sp.diags(dd) + (A.T if adjoint else A)).tocsr()


def jacobi_diagonal(A, d=None, sigma=0.0):
    """diag(M)[i] = σ + d[i] plus the stored entries (i, i) of A in storage order."""
    A = sp.csc_matrix(A)
    n = A.shape[0]
    diag = np.full(n, float(sigma)) + (0.0 if d is None else np.asarray(d, dtype=np.float64))
    cols = np.repeat(np.arange(n), np.diff(A.indptr))
    on = np.flatnonzero(A.indices == cols)
    np.add.at(diag, cols[on], A.data[on])  # (unbuffered: one addition per stored entry, in storage order)
    return diag


def _solve_column(M, diag, b, x, rtol, maxiter):
    """-> (x, iterations, relres, reason index)."""
    bn = np.sqrt(b @ b)
    if b @ b == 0.0:
        return np.zeros_like(b), 0, 0.0, 0
    it, relres = 0, 0.0
    r = rh = p = v = None
    rho = alpha = omega = 1.0
    beta = 0.0
    verify = True
    while True:
        if verify:  # the true residual decides
            r = b - M @ x
            rn = np.sqrt(r @ r)
            relres = rn / bn
            if not (np.isfinite(bn) and np.isfinite(rn)):
                return x, it, relres, 3
            if rn <= rtol * bn:
                return x, it, relres, 0
            if it >= maxiter:
                return x, it, relres, 1
            restart, rho, rhn, verify = True, r @ r, rn, False
        if restart:
            p, rh = r.copy(), r.copy()
        else:
            p = r + beta * (p - omega * v)
        ph = p / diag
        v = M @ ph
        rv = rh @ v
        if not np.isfinite(rv):
            return x, it, relres, 3
        if rv == 0.0:
            return x, it, relres, 2
        alpha = rho / rv
        if not np.isfinite(alpha):
            return x, it, relres, 3
        s = r - alpha * v
        sh = s / diag
        t = M @ sh
        ts, tt, ss = t @ s, t @ t, s @ s
        if not (np.isfinite(ts) and np.isfinite(tt) and np.isfinite(ss)):
            return x, it, relres, 3
        if np.sqrt(ss) <= rtol * bn:
            omega = 0.0
        elif tt == 0.0:
            return x, it, relres, 2
        else:
            omega = ts / tt
            if not np.isfinite(omega):
                return x, it, relres, 3
        x = (x + alpha * ph) + omega * sh
        r = s - omega * t
        it += 1
        rr, rn2 = rh @ r, r @ r
        rn = np.sqrt(rn2)
        relres = rn / bn
        if not (np.isfinite(rr) and np.isfinite(rn2)):
            return x, it, relres, 3
        if rn <= rtol * bn:
            verify = True
            continue
        if it >= maxiter:
            return x, it, relres, 1
        if abs(rr) <= EPS52 * rhn * rn:  # ρ is lost in the rounding of its own sum: a new shadow residual
            verify = True
            continue
        if omega == 0.0:
            return x, it, relres, 2
        beta = (rr / rho) * (alpha / omega)
        rho, restart = rr, False
        if not np.isfinite(beta):
            return x, it, relres, 3


def solve_ref(A, B, d=None, sigma=0.0, rtol=1e-10, maxiter=10000, x0=None, adjoint=False):
    """A: scipy sparse, square.  -> (X, info) with info = dict(iterations, relres, reason, converged), one entry per column."""
    if A.shape[0] != A.shape[1]:
        raise ValueError("the matrix must be square")
    if not rtol > 0 or maxiter < 0:
        raise ValueError("rtol > 0 and maxiter >= 0 are required")
    diag = jacobi_diagonal(A, d, sigma)
    bad = np.flatnonzero((diag == 0.0) | ~np.isfinite(diag))
    if bad.size:
        raise SingularPreconditioner(int(bad[0]))
    M = system(sp.csc_matrix(A), d, sigma, adjoint)
    B = np.asarray(B, dtype=np.float64)
    B2 = B.reshape(B.shape[0], -1)
    X0 = np.zeros_like(B2) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(B2.shape)
    X = np.zeros(B2.shape, order="F")
    iters, relres, reason = [], [], []
    with np.errstate(all="ignore"):
        for c in range(B2.shape[1]):
            x, it, rr, why = _solve_column(M, diag, B2[:, c], X0[:, c].copy(), rtol, maxiter)
            X[:, c] = x
            iters.append(it)
            relres.append(rr)
            reason.append(REASONS[why])
    info = dict(iterations=np.array(iters), relres=np.array(relres), reason=tuple(reason), converged=np.array([r == "converged" for r in reason]))
    return X.reshape(B.shape), info


# ---- the checked systems -----------------------------------------------------------------------------------------------------------
GRIDS = ("tiny_tripolar", "tiny_bipolar", "odd_nx_fold", "small_rho3d", "90x60x20")
BIG = dict(nx=90, ny=60, nz=20, seed=21)  # "90x60x20": N = 65 817


def grid_T(oracle, name):
    """(T as (colptr, rowval, nzval), N, number of level-1 wet cells) of a tests/helpers.py case or of the 90 x 60 x 20 grid."""
    from helpers import gridmetrics_of, make_case
    from otmb_amd import synthetic

    if name == "90x60x20":
        g = synthetic.make_grid(BIG["nx"], BIG["ny"], BIG["nz"], seed=BIG["seed"])
        gm = gridmetrics_of(g)
    else:
        g, gm = make_case(name)
    idx = oracle.makeindices(gm.v3D)
    phi = oracle.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], g.umo.properties["_FillValue"], gm.gridtopology.kind)
    tm = oracle.transportmatrix(phi, gm, idx, g.rho, g.mlotst)
    nsurf = int(np.count_nonzero(idx["wet3D"][:, :, 0]))
    return tm["T"], int(idx["N"]), nsurf


def shift(which, N, nsurf):
    """(d, σ) of the age system (d = 1 s⁻¹ on the level-1 wet cells, the first nsurf wet indices), a one-month and a one-year shift."""
    if which == "age":
        d = np.zeros(N)
        d[:nsurf] = 1.0
        return d, 0.0
    return None, {"month": 1.0 / (30 * DAY), "year": 1.0 / (365 * DAY)}[which]


def arrow(n=5000, seed=3):
    """Diagonally dominant arrow matrix: dense first row and first column, diagonal = 2·Σ|off-diagonal| of its row.  Julia's arrays."""
    rng = np.random.default_rng(seed)
    A = sp.lil_matrix((n, n))
    A[0, 1:] = rng.uniform(0.5, 1.5, n - 1) * rng.choice([-1.0, 1.0], n - 1)
    A[1:, 0] = (rng.uniform(0.5, 1.5, n - 1) * rng.choice([-1.0, 1.0], n - 1)).reshape(-1, 1)
    A = sp.csr_matrix(A)
    off = np.asarray(abs(A).sum(axis=1)).ravel()
    A = sp.csc_matrix(A + sp.diags(2.0 * off))
    A.sort_indices()
    return A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, A.data.astype(np.float64)


def dominant(n=257, per_row=9, seed=5):
    """Random nonsymmetric, strictly diagonally dominant matrix: per_row - 1 off-diagonal entries per row in random columns (a repeated
    column is summed), diagonal = 2·Σ|off-diagonal| of its row.  n = 257: two workgroups of the row kernels, five of the column kernels,
    a last slice of one row.  Julia's arrays."""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(n), per_row - 1)
    cols = rng.integers(0, n, rows.size)
    vals = rng.uniform(0.5, 1.5, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    keep = rows != cols
    A = sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(n, n))
    off = np.asarray(abs(A).sum(axis=1)).ravel()
    assert (off > 0).all()
    A = sp.csc_matrix(A + sp.diags(2.0 * off))
    A.sort_indices()
    return A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, A.data.astype(np.float64)


def longest(A, adjoint):
    """L of the residual bound: the longest row of M's product -- a row of A (adjoint: a column) and the diagonal term."""
    A = sp.csc_matrix(A)
    return int((np.diff(A.indptr) if adjoint else np.bincount(A.indices, minlength=A.shape[0])).max())


def residual_check(A, X, B, d, sigma, adjoint, rtol):
    """Per column: (‖b - M·x‖₂, rtol·‖b‖₂ + 2·(L + 3)·ε·‖ |M|·|x| + |b| ‖₂), the residual in float64 by scipy.  The second term is the
    standard rounding bound of a residual evaluated twice in different orders (each evaluation: γ_{L+2}·(|M|·|x| + |b|) rowwise)."""
    M = system(sp.csc_matrix(A), d, sigma, adjoint)
    X2, B2 = np.asarray(X).reshape(M.shape[0], -1), np.asarray(B).reshape(M.shape[0], -1)
    L = longest(A, adjoint)
    out = []
    for c in range(B2.shape[1]):
        res = np.linalg.norm(B2[:, c] - M @ X2[:, c])
        bound = rtol * np.linalg.norm(B2[:, c]) + 2 * (L + 3) * EPS * np.linalg.norm(abs(M) @ np.abs(X2[:, c]) + np.abs(B2[:, c]))
        out.append((res, bound))
    return out
