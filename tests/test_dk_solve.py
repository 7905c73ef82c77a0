"""GPU: otmb_op_solve_dk and otmb_op_precond_dk (csrc/otmb_solve.hip, csrc/otmb_solve_lines.hip): every column with its own d.  Column c of a
per-column call has the bits of the k = 1 call with d = D[:, c] (the existing exports, which are the new ones with ldd = 0); the
preconditioner alone is, column by column, the numpy restatement bit for bit (tests/solve_lines_ref.py, solve_ref.jacobi_diagonal); converged
columns meet the float64 residual bound of tests/test_solve.py for their own system; a singular column is refused by name; and the rules of
ldd at the C ABI."""
import numpy as np
import pytest

import dk_cases as DK
import solve_lines_ref as LR
import solve_ref as R

pytestmark = pytest.mark.gpu

RTOL, MAXITER = 1e-10, 5000
N0 = 257


def _csc(n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(n, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


def _per_column_equals_single_calls(D, A, nxt, Dk, sigma, adjoint, precond, B, what, check_ref=True):
    """solve and precondition with the n x k d against the k calls with k = 1; -> info of the per-column solve."""
    k = B.shape[1]
    X, info = D.solve(B, d=Dk, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
    Z = D.precondition(B, d=Dk, sigma=sigma, adjoint=adjoint, precond=precond)
    print(what, "k", k, "iterations", info.iterations.tolist(), "reason", info.reason)
    for c in range(k):
        dc = np.ascontiguousarray(Dk[:, c])
        x1, i1 = D.solve(B[:, c], d=dc, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
        DK.same_bits(X[:, c], x1, (what, c, "X"))
        assert info.iterations[c] == i1.iterations[0] and info.reason[c] == i1.reason[0], (what, c, info, i1)
        DK.same_bits(info.relres[c], i1.relres[0], (what, c, "relres"))
        DK.same_bits(Z[:, c], D.precondition(B[:, c], d=dc, sigma=sigma, adjoint=adjoint, precond=precond), (what, c, "Z"))
        if check_ref:  # the CPU restatement, which shares no code with the library
            want = LR.Lines(A, nxt, dc, sigma, adjoint).apply(B[:, c]) if precond == "lines" else B[:, c] / R.jacobi_diagonal(A, dc, sigma)
            DK.same_bits(Z[:, c], want, (what, c, "Z against the restatement"))
            if info.converged[c]:
                (res, bound), = R.residual_check(A, X[:, c:c + 1], B[:, c:c + 1], dc, sigma, adjoint, RTOL)
                assert res <= bound, (what, c, res, bound)
    return info


@pytest.fixture(scope="module")
def small(oracle):
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        yield D, R.csc_of(N, N, *T), N, nsurf, nxt


@pytest.mark.parametrize("which", ["month", "age"])
@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
def test_the_cross_product_on_the_small_grid(small, adjoint, precond, which):
    """odd_nx_fold (one workgroup): A and Aᵀ x Jacobi and lines x σ of a month and of zero x k = 1, 3, 7.  The zero column is in D only where
    σ > 0.  The columns do not all take the same number of iterations: some were frozen while others ran."""
    D, A, N, nsurf, nxt = small
    sigma = R.shift("month", N, nsurf)[1] if which == "month" else 0.0
    Dk = DK.columns(N, nsurf, zero=sigma > 0)
    B = DK.rhs(N, DK.K, seed=5 + adjoint)
    for k in (1, 3, 7):
        info = _per_column_equals_single_calls(D, A, nxt, Dk[:, :k], sigma, adjoint, precond, B[:, :k], (which, precond, adjoint))
        if which == "month":
            assert info.converged.all(), info
    assert len(set(info.iterations.tolist())) > 1, info


@pytest.mark.parametrize("name", ["tiny_tripolar", "small_rho3d"])
def test_several_workgroups_and_a_last_partial_block(oracle, name):
    """N = 429 and 6962, lines, a month, k = 7, A and Aᵀ."""
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, name)
    A = R.csc_of(N, N, *T)
    sigma = R.shift("month", N, nsurf)[1]
    Dk = DK.columns(N, nsurf, zero=True)
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        for adjoint in (False, True):
            info = _per_column_equals_single_calls(D, A, nxt, Dk, sigma, adjoint, "lines", DK.rhs(N, DK.K, seed=9), (name, adjoint))
            assert info.converged.all() and len(set(info.iterations.tolist())) > 1, info


@pytest.mark.parametrize("make", [R.dominant, R.arrow], ids=["dominant", "arrow"])
def test_the_long_row_kernel(make):
    """solve_ref.dominant (n = 257) and arrow (a dense first row and column: the long-row kernel and the longest column of Aᵀ), both
    preconditioners (random lines), random non-negative columns of d on very different scales."""
    import otmb_amd.api as api

    p, i, v = make()
    n = len(p) - 1
    A = R.csc_of(n, n, p, i, v)
    rng = np.random.default_rng(31)
    Dk = np.asfortranarray(rng.uniform(0.0, 1.0, (n, DK.K)) * np.array([1.0, 1e-5, 100.0, 0.0, 1e3, 3.0, 0.1]))
    nxt = LR.random_lines(n, 4)
    B = DK.rhs(n, DK.K, seed=2)
    with api.DeviceOperator(_csc(n, p, i, v)) as D:
        D.set_lines(nxt)
        for adjoint in (False, True):
            for precond in ("jacobi", "lines"):
                info = _per_column_equals_single_calls(D, A, nxt, Dk, 0.5, adjoint, precond, B, (make.__name__, adjoint, precond))
                assert info.converged.all(), info


def test_equal_columns_and_ldd_zero_are_the_one_d_call(small):
    """A per-column call whose columns are all the same vector, and a raw call with ldd == 0, equal the 1-D call bit for bit."""
    from otmb_amd import capi

    D, A, N, nsurf, nxt = small
    d, sigma = R.shift("age", N, nsurf)[0], R.shift("month", N, nsurf)[1]
    B = DK.rhs(N, DK.K, seed=3)
    for precond in ("jacobi", "lines"):
        X1, i1 = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond=precond)
        Xk, ik = D.solve(B, d=np.asfortranarray(np.repeat(d[:, None], DK.K, axis=1)), sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond=precond)
        DK.same_bits(Xk, X1, precond)
        assert np.array_equal(ik.iterations, i1.iterations) and ik.reason == i1.reason
        DK.same_bits(ik.relres, i1.relres, "relres")
        X0 = np.zeros((N, DK.K), order="F")
        it, rr, why = np.zeros(DK.K, np.int64), np.zeros(DK.K), np.zeros(DK.K, np.int32)
        rc = capi.lib().otmb_op_solve_dk(D.handle, 0, DK.K, d.ctypes.data, 0, float(sigma), B.ctypes.data, N, X0.ctypes.data, N, 0, RTOL, MAXITER,
                                         it.ctypes.data, rr.ctypes.data, why.ctypes.data, capi.PRECONDS[precond])
        assert rc == 0
        DK.same_bits(X0, X1, (precond, "ldd = 0"))
        assert np.array_equal(it, i1.iterations)
        Z0 = np.zeros((N, DK.K), order="F")
        assert capi.lib().otmb_op_precond_dk(D.handle, 0, capi.PRECONDS[precond], DK.K, d.ctypes.data, 0, float(sigma), B.ctypes.data, N, Z0.ctypes.data, N) == 0
        DK.same_bits(Z0, D.precondition(B, d=d, sigma=sigma, precond=precond), (precond, "precond, ldd = 0"))


def test_a_bad_ldd_is_refused_by_the_library(small):
    """0 < ldd < n and ldd < 0 with a D: INVALID_ARG, the message names the call, X is untouched.  D == NULL ignores ldd."""
    from otmb_amd import capi

    D, A, N, nsurf, nxt = small
    lib = capi.lib()
    Dk = DK.columns(N, nsurf, zero=True)
    B = DK.rhs(N, 3, seed=3)
    it, rr, why = np.zeros(3, np.int64), np.zeros(3), np.zeros(3, np.int32)
    for ldd in (N - 1, 1, -N):
        X = np.full((N, 3), 7.25, order="F")
        rc = lib.otmb_op_solve_dk(D.handle, 0, 3, Dk.ctypes.data, ldd, 1e-6, B.ctypes.data, N, X.ctypes.data, N, 0, RTOL, MAXITER, it.ctypes.data,
                                  rr.ctypes.data, why.ctypes.data, 0)
        assert rc == 11 and "otmb_op_solve_dk" in lib.otmb_last_error(D.ctx.handle).decode() and (X == 7.25).all(), ldd
        rc = lib.otmb_op_precond_dk(D.handle, 0, 0, 3, Dk.ctypes.data, ldd, 1e-6, B.ctypes.data, N, X.ctypes.data, N)
        assert rc == 11 and "otmb_op_precond_dk" in lib.otmb_last_error(D.ctx.handle).decode() and (X == 7.25).all(), ldd
    X = np.zeros((N, 3), order="F")
    rc = lib.otmb_op_solve_dk(D.handle, 0, 3, None, 5, 1e-6, B.ctypes.data, N, X.ctypes.data, N, 0, RTOL, MAXITER, it.ctypes.data, rr.ctypes.data,
                              why.ctypes.data, 0)
    assert rc == 0
    DK.same_bits(X, D.solve(B, sigma=1e-6, rtol=RTOL, maxiter=MAXITER)[0], "D == NULL")


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
def test_a_singular_column_is_named(precond):
    """Column 3 of D cancels the diagonal at two line heads, column 5 at a head of smaller index: SINGULAR_PRECONDITIONER, the message names
    column 3 -- the smallest column -- and its first bad index, which with lines is the pivot the restatement refuses (a head's pivot is its
    diagonal entry; the pivots after it on the line have larger indices); X is untouched."""
    import otmb_amd.api as api
    from otmb_amd import capi

    p, i, v = R.dominant(N0)
    A = R.csc_of(N0, N0, p, i, v)
    diag = A.diagonal()
    nxt = LR.random_lines(N0, 2)
    succ = LR.successors(nxt, N0)
    heads = np.setdiff1d(np.arange(N0), succ[succ >= 0])
    first, later, smaller = int(heads[3]), int(heads[-1]), int(heads[0])
    Dk = np.asfortranarray(np.random.default_rng(8).uniform(0.0, 1.0, (N0, DK.K)))
    Dk[[first, later], 2] = -diag[[first, later]]  # σ = 0: 0 + d is -a exactly, and -a + a is zero
    Dk[smaller, 4] = -diag[smaller]
    if precond == "lines":
        with pytest.raises(LR.SingularLines) as e:
            LR.Lines(A, nxt, Dk[:, 2], 0.0)
        assert e.value.index == first
        text = "pivot[%d] of the line factorisation is zero or not finite (1-based; the smallest such index) (column 3 of 7)"
    else:
        text = "diag(M)[%d] is zero or not finite (1-based; the first such index) (column 3 of 7)"
    index = first + 1
    B = DK.rhs(N0, DK.K, seed=1)
    with api.DeviceOperator(_csc(N0, p, i, v)) as D:
        D.set_lines(nxt)
        for call in (lambda: D.solve(B, d=Dk, precond=precond), lambda: D.precondition(B, d=Dk, precond=precond)):
            with pytest.raises(capi.OtmbError) as err:
                call()
            assert err.value.name == "SINGULAR_PRECONDITIONER" and str(err.value).endswith(text % index), str(err.value)
        X = np.full((N0, DK.K), 7.25, order="F")
        it, rr, why = np.zeros(DK.K, np.int64), np.zeros(DK.K), np.zeros(DK.K, np.int32)
        rc = capi.lib().otmb_op_solve_dk(D.handle, 0, DK.K, Dk.ctypes.data, N0, 0.0, B.ctypes.data, N0, X.ctypes.data, N0, 1, RTOL, MAXITER,
                                         it.ctypes.data, rr.ctypes.data, why.ctypes.data, capi.PRECONDS[precond])
        assert rc == 18 and (X == 7.25).all()
        # the same d for all columns keeps the message existing callers read
        with pytest.raises(capi.OtmbError) as err:
            D.solve(B, d=np.ascontiguousarray(Dk[:, 2]), precond=precond)
        assert str(err.value).endswith((text % index)[:-len(" (column 3 of 7)")]), str(err.value)
