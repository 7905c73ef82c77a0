"""A numpy restatement of the line preconditioner (csrc/otmb_solve_lines.hip, include/otmb.h): the rules of otmb_op_set_lines, the
extraction of u and l, the factorisation and the sweep -- the loop runs over the depth along the lines and is vectorised across the lines;
elementwise float64 numpy is IEEE arithmetic without FMA, so these are the contract's bits -- and the BiCGStab of tests/solve_ref.py with
P⁻¹ in place of `./ diag`.

With j = next[i] (non-adjoint; the adjoint swaps u and l):
    a_i = Jacobi's diag[i];  u_i = Σ stored (i, j) of A,  l_i = Σ stored (j, i) of A, each from +0.0 in storage order
    piv_head = a_head;  m_j = l_i / piv_i;  piv_j = a_j - m_j·u_i
    y'_head = y_head, y'_j = y_j - m_j·y'_i;  z_tail = y'_tail / piv_tail, z_i = (y'_i - u_i·z_j) / piv_i"""
import numpy as np
import scipy.sparse as sp

import solve_ref as R


class InvalidLines(ValueError):
    """index: 0-based, the first offender; rule: "range" (an entry is neither 0 nor in (i, n]) or "twice" (a successor of two unknowns)."""

    def __init__(self, index, rule):
        super().__init__(f"{rule}: index {index + 1}")
        self.index, self.rule = index, rule


class SingularLines(ValueError):
    def __init__(self, index):
        super().__init__(f"pivot[{index + 1}] is zero or not finite")
        self.index = index


def successors(next, n):
    """The C rules, in the C order: -> the 0-based successor of every unknown (-1: none)."""
    nx = np.asarray(next, dtype=np.int64)
    assert nx.shape == (n,)
    i1 = np.arange(1, n + 1)
    bad = np.flatnonzero((nx != 0) & ((nx <= i1) | (nx > n)))
    if bad.size:
        raise InvalidLines(int(bad[0]), "range")
    twice = np.flatnonzero(np.bincount(nx[nx > 0] - 1, minlength=n) > 1)
    if twice.size:
        raise InvalidLines(int(twice[0]), "twice")
    return nx - 1


class Lines:
    """The factored preconditioner of M = σ·I + diag(d) + A (adjoint: Aᵀ) on the lines `next`; apply(y) = P⁻¹·y; `p / lines` is apply(p),
    which is how solve_ref._solve_column takes it in place of its diagonal."""
    __array_ufunc__ = None  # numpy leaves `array / lines` to __rtruediv__

    def __init__(self, A, next, d=None, sigma=0.0, adjoint=False):
        A = sp.csc_matrix(A)
        n = A.shape[0]
        self.n = n
        nxt = self.nxt = successors(next, n)
        self.a = R.jacobi_diagonal(A, d, sigma)
        cols = np.repeat(np.arange(n), np.diff(A.indptr))
        rows = A.indices.astype(np.int64)
        up, lo = np.zeros(n), np.zeros(n)
        e = np.flatnonzero(nxt[rows] == cols)  # stored (i, j): row i, column j = next[i]
        np.add.at(up, rows[e], A.data[e])  # (unbuffered: one addition per stored entry, in storage order)
        e = np.flatnonzero(nxt[cols] == rows)  # stored (j, i): column i, row j = next[i]
        np.add.at(lo, cols[e], A.data[e])
        self.u, self.l = (lo, up) if adjoint else (up, lo)
        heads = np.ones(n, dtype=bool)
        heads[nxt[nxt >= 0]] = False
        self.heads = np.flatnonzero(heads)
        self.levels = []  # per depth: (i, j = next[i]) of every line that goes on
        cur = self.heads
        while True:
            j = nxt[cur]
            cur, j = cur[j >= 0], j[j >= 0]
            if not cur.size:
                break
            self.levels.append((cur, j))
            cur = j
        self.m, self.piv = np.zeros(n), self.a.copy()
        with np.errstate(all="ignore"):
            for i, j in self.levels:
                self.m[j] = self.l[i] / self.piv[i]
                t = self.m[j] * self.u[i]
                self.piv[j] = self.a[j] - t
        bad = np.flatnonzero((self.piv == 0.0) | ~np.isfinite(self.piv))
        if bad.size:
            raise SingularLines(int(bad[0]))

    def apply(self, y):
        y = np.asarray(y, dtype=np.float64)
        col = (slice(None), None) if y.ndim == 2 else slice(None)
        z = y.copy()
        with np.errstate(all="ignore"):
            for i, j in self.levels:
                t = self.m[j][col] * z[i]
                z[j] = y[j] - t
            tails = np.flatnonzero(self.nxt < 0)
            z[tails] = z[tails] / self.piv[tails][col]
            for i, j in reversed(self.levels):
                t = self.u[i][col] * z[j]
                z[i] = (z[i] - t) / self.piv[i][col]
        return z

    def __rtruediv__(self, y):
        return self.apply(y)

    def matrix(self):
        """P, assembled explicitly."""
        i = np.flatnonzero(self.nxt >= 0)
        j = self.nxt[i]
        n = self.n
        return (sp.diags(self.a) + sp.csr_matrix((self.u[i], (i, j)), shape=(n, n)) + sp.csr_matrix((self.l[i], (j, i)), shape=(n, n))).tocsc()

    def lu_bound(self, z):
        """4·ε·‖ |L|·|U|·|z| ‖∞ with L (unit lower bidiagonal, m) and U (upper bidiagonal, piv and u) as factored here: the backward error
        of a bidiagonal-bidiagonal solve (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 9.14: |ΔP| ≤ (4ε + O(ε²))·|L|·|U|),
        as the bound of the residual P·z - y."""
        i = np.flatnonzero(self.nxt >= 0)
        j = self.nxt[i]
        n = self.n
        L = sp.identity(n, format="csr") + sp.csr_matrix((np.abs(self.m[j]), (j, i)), shape=(n, n))
        U = sp.diags(np.abs(self.piv)) + sp.csr_matrix((np.abs(self.u[i]), (i, j)), shape=(n, n))
        return 4 * R.EPS * np.abs(L @ (U @ np.abs(z))).max()


def solve_lines_ref(A, B, next, d=None, sigma=0.0, rtol=1e-10, maxiter=10000, x0=None, adjoint=False):
    """solve_ref.solve_ref with the line preconditioner: -> (X, info)."""
    if A.shape[0] != A.shape[1]:
        raise ValueError("the matrix must be square")
    if not rtol > 0 or maxiter < 0:
        raise ValueError("rtol > 0 and maxiter >= 0 are required")
    P = Lines(A, next, d, sigma, adjoint)
    M = R.system(sp.csc_matrix(A), d, sigma, adjoint)
    B = np.asarray(B, dtype=np.float64)
    B2 = B.reshape(B.shape[0], -1)
    X0 = np.zeros_like(B2) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(B2.shape)
    X = np.zeros(B2.shape, order="F")
    iters, relres, reason = [], [], []
    with np.errstate(all="ignore"):
        for c in range(B2.shape[1]):
            x, it, rr, why = R._solve_column(M, P, B2[:, c], X0[:, c].copy(), rtol, maxiter)
            X[:, c] = x
            iters.append(it)
            relres.append(rr)
            reason.append(R.REASONS[why])
    info = dict(iterations=np.array(iters), relres=np.array(relres), reason=tuple(reason), converged=np.array([r == "converged" for r in reason]))
    return X.reshape(B.shape), info


# ---- the checked systems -----------------------------------------------------------------------------------------------------------
_GRIDS = {}


def grid(oracle, name):
    """(T, N, nsurf, next) of a grid of solve_ref.GRIDS, computed once per session: next = the water columns (api.vertical_lines)."""
    if name not in _GRIDS:
        from helpers import gridmetrics_of, make_case
        from otmb_amd import api, synthetic

        T, N, nsurf = R.grid_T(oracle, name)
        if name == "90x60x20":
            gm = gridmetrics_of(synthetic.make_grid(R.BIG["nx"], R.BIG["ny"], R.BIG["nz"], seed=R.BIG["seed"]))
        else:
            gm = make_case(name)[1]
        nxt = api.vertical_lines(oracle.makeindices(gm.v3D))
        assert nxt.shape == (N,)
        _GRIDS[name] = (T, N, nsurf, nxt)
    return _GRIDS[name]


def random_lines(n, seed):
    """Random valid lines: a random permutation cut into chains, each chain sorted ascending."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    cuts = np.sort(rng.choice(np.arange(1, n), size=int(rng.integers(1, max(2, n // 3))), replace=False))
    nxt = np.zeros(n, dtype=np.int64)
    for chain in np.split(perm, cuts):
        chain = np.sort(chain)
        nxt[chain[:-1]] = chain[1:] + 1
    return nxt


def stride_lines(n, step):
    """next[i] = i + step (0-based successor i + step) while it exists: `step` lines."""
    nxt = np.arange(n, dtype=np.int64) + step + 1
    nxt[nxt > n] = 0
    return nxt
