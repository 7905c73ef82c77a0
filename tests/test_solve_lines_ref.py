"""CPU: tests/solve_lines_ref.py, the numpy restatement of the line preconditioner (otmb_op_set_lines, otmb_op_solve_pc, otmb_op_precond):
its sweep against scipy's sparse LU of the explicitly assembled P, the iteration counts that motivate the preconditioner, and the rules
for `next`."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import solve_lines_ref as LR
import solve_ref as R

RTOL = 1e-10


@pytest.mark.parametrize("which", ["age", "month", "year"])
@pytest.mark.parametrize("name", R.GRIDS)
def test_sweep_against_sparse_lu_of_the_assembled_preconditioner(oracle, name, which):
    """‖P·z - y‖∞ ≤ 4·ε·‖ |L|·|U|·|z| ‖∞ for the restated sweep (Lines.lu_bound: the LU backward error of a bidiagonal L and U, ε = 2⁻⁵³;
    derived, not tuned), P assembled explicitly; scipy's splu of the same P solves the same system, and the two solutions differ by no more
    than the two residuals allow: ‖P·(z - z_lu)‖∞ ≤ bound + ‖P·z_lu - y‖∞."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    A = R.csc_of(N, N, *T)
    d, sigma = R.shift(which, N, nsurf)
    rng = np.random.default_rng(17)
    Y = np.ones((N, 2))
    Y[:, 1] = rng.standard_normal(N)
    for adjoint in (False, True):
        P = LR.Lines(A, nxt, d, sigma, adjoint)
        Pm = P.matrix()
        M = R.system(A, d, sigma, adjoint)
        i = np.flatnonzero(nxt)
        # P is M on the lines: the diagonal and the (i, next[i]), (next[i], i) entries
        assert np.array_equal(Pm.diagonal(), M.diagonal()) or np.allclose(Pm.diagonal(), M.diagonal(), rtol=1e-15, atol=0)
        assert np.allclose(np.asarray(Pm[i, nxt[i] - 1]).ravel(), np.asarray(M[i, nxt[i] - 1]).ravel(), rtol=1e-15, atol=0)
        assert np.allclose(np.asarray(Pm[nxt[i] - 1, i]).ravel(), np.asarray(M[nxt[i] - 1, i]).ravel(), rtol=1e-15, atol=0)
        lu = spla.splu(Pm)
        Z = P.apply(Y)
        for c in range(2):
            z, y = Z[:, c], Y[:, c]
            assert np.array_equal(P.apply(y), z)  # a column alone has the bits of the column in a block
            res = np.abs(Pm @ z - y).max()
            bound = P.lu_bound(z)
            zl = lu.solve(y)
            resl = np.abs(Pm @ zl - y).max()
            print(name, which, "adjoint", adjoint, "column", c, "residual", res, "bound", bound, "splu residual", resl,
                  "max |z - z_lu| / max |z|", np.abs(z - zl).max() / np.abs(z).max())
            assert res <= bound
            assert np.abs(Pm @ (z - zl)).max() <= bound + resl + 4 * R.EPS * np.abs(y).max()  # (the last term: the two products' own rounding)


# iterations of the restated solver with B = 1, rtol = 1e-10: (Jacobi, lines) for A and for Aᵀ, as measured (None: not run here, see the docstring)
TABLE = {
    ("odd_nx_fold", "age"): ((16, 5), (16, 6)), ("odd_nx_fold", "month"): ((193, 3), (159, 3)), ("odd_nx_fold", "year"): ((678, 4), (391, 4)),
    ("tiny_tripolar", "age"): ((30, 12), (26, 11)), ("tiny_tripolar", "month"): ((250, 3), (284, 3)), ("tiny_tripolar", "year"): ((1013, 4), (977, 4)),
    ("tiny_bipolar", "age"): ((32, 14), (29, 14)), ("tiny_bipolar", "month"): ((253, 3), (199, 3)), ("tiny_bipolar", "year"): ((1162, 6), (690, 5)),
    ("small_rho3d", "age"): ((86, 53), (70, 54)), ("small_rho3d", "month"): ((318, 3), (230, 3)), ("small_rho3d", "year"): ((2407, 7), (1268, 8)),
    ("90x60x20", "age"): ((185, 78), (175, 85)), ("90x60x20", "month"): ((894, 6), (626, 6)), ("90x60x20", "year"): ((None, 20), (None, 20)),
}


@pytest.mark.parametrize("which", ["age", "month", "year"])
@pytest.mark.parametrize("name", R.GRIDS)
def test_iteration_counts_of_the_restated_solver(oracle, name, which):
    """The table that motivates the preconditioner (B = 1, rtol = 1e-10; Jacobi -> lines, in brackets Aᵀ), as measured with this restatement:

        grid            N       age                   month                year
        odd_nx_fold     117     16 -> 5 (16 -> 6)     193 -> 3 (159 -> 3)  678 -> 4 (391 -> 4)
        tiny_tripolar   429     30 -> 12 (26 -> 11)   250 -> 3 (284 -> 3)  1013 -> 4 (977 -> 4)
        tiny_bipolar    512     32 -> 14 (29 -> 14)   253 -> 3 (199 -> 3)  1162 -> 6 (690 -> 5)
        small_rho3d     6962    86 -> 53 (70 -> 54)   318 -> 3 (230 -> 3)  2407 -> 7 (1268 -> 8)
        90x60x20        65817   185 -> 78 (175 -> 85) 894 -> 6 (626 -> 6)  14935 -> 20 (maxiter 20000 -> 20)

    Both solvers are run here and both counts must be the table's, with ONE exception: the two Jacobi figures of the year system on
    90x60x20 (14935, and the adjoint's stop at maxiter = 20000) are NOT asserted by this or any other test.  They were measured once
    with solve_ref.solve_ref exactly as the other Jacobi counts here are (14935 iterations, converged, 58 s of numpy; the adjoint:
    maxiter after 20000 iterations, 88 s) -- two and a half minutes that no suite should pay on every run.  The lines counts of that
    system (20 and 20) are asserted.  Every lines solution meets the float64 residual bound of tests/test_solve.py."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    A = R.csc_of(N, N, *T)
    d, sigma = R.shift(which, N, nsurf)
    B = np.ones(N)
    for adjoint, (jac, lin) in zip((False, True), TABLE[name, which]):
        X, info = LR.solve_lines_ref(A, B, nxt, d=d, sigma=sigma, rtol=RTOL, maxiter=2000, adjoint=adjoint)
        print(name, which, "adjoint", adjoint, "lines", info["iterations"][0], info["reason"][0], info["relres"][0])
        assert info["reason"] == ("converged",)
        (res, bound), = R.residual_check(A, X, B, d, sigma, adjoint, RTOL)
        assert res <= bound
        assert info["iterations"][0] == lin
        if jac is not None:
            Xj, ij = R.solve_ref(A, B, d=d, sigma=sigma, rtol=RTOL, maxiter=20000, adjoint=adjoint)
            print(name, which, "adjoint", adjoint, "jacobi", ij["iterations"][0], ij["reason"][0])
            assert ij["reason"] == ("converged",) and ij["iterations"][0] == jac


def test_no_lines_is_jacobi_to_the_bit():
    p, i, v = R.dominant(257)
    A = R.csc_of(257, 257, p, i, v)
    d = np.random.default_rng(13).uniform(0.0, 1.0, 257)
    P = LR.Lines(A, np.zeros(257, dtype=np.int64), d, 0.5)
    Y = np.random.default_rng(1).standard_normal((257, 3))
    assert np.array_equal(P.apply(Y), Y / R.jacobi_diagonal(A, d, 0.5)[:, None])
    B = np.ones((257, 2))
    B[:, 1] = Y[:, 0]
    X1, i1 = LR.solve_lines_ref(A, B, np.zeros(257, dtype=np.int64), d=d, sigma=0.5)
    X2, i2 = R.solve_ref(A, B, d=d, sigma=0.5)
    assert np.array_equal(X1, X2) and np.array_equal(i1["iterations"], i2["iterations"]) and np.array_equal(i1["relres"], i2["relres"])


def test_the_rules_for_next():
    n = 9
    ok = np.array([2, 3, 0, 5, 0, 0, 9, 0, 0])
    nxt = LR.successors(ok, n)
    assert nxt.tolist() == [1, 2, -1, 4, -1, -1, 8, -1, -1]
    for lines in (np.zeros(n, dtype=np.int64), LR.stride_lines(n, 1), LR.stride_lines(n, 4), *(LR.random_lines(n, s) for s in range(5))):
        s = LR.successors(lines, n)
        assert ((s < 0) | (s > np.arange(n))).all() and np.bincount(s[s >= 0], minlength=n).max() <= 1
    # an entry must be 0 or in (i, n] (1-based): itself, an index before it, beyond n, negative -- the first offender is named
    for at, val in ((3, 4), (3, 2), (3, n + 1), (3, -1), (n - 1, n)):
        bad = ok.copy()
        bad[at] = val
        bad[6] = 1  # (a later offender)
        with pytest.raises(LR.InvalidLines) as e:
            LR.successors(bad, n)
        assert (e.value.index, e.value.rule) == (min(at, 6), "range")
    # nobody is the successor of two unknowns: the successor is named
    bad = ok.copy()
    bad[3] = 9
    with pytest.raises(LR.InvalidLines) as e:
        LR.successors(bad, n)
    assert (e.value.index, e.value.rule) == (8, "twice")
    # a zero pivot is refused by its index: a_2 = m_2·u_1 exactly, in powers of two
    import scipy.sparse as sp

    A = sp.csc_matrix(np.array([[2.0, 4.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 1.0]]))
    with pytest.raises(LR.SingularLines) as e:
        LR.Lines(A, np.array([2, 0, 0]))
    assert e.value.index == 1
    LR.Lines(A, np.array([2, 0, 0]), sigma=1.0)
