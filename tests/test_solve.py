"""The device solver (csrc/otmb_solve.hip, otmb_op_solve[_dev]): (σ·I + diag(d) + A)·X = B by Jacobi-preconditioned BiCGStab on the
resident operator, through api.DeviceOperator.solve, the C ABI and DeviceAssembler.solve.  Acceptance is a residual recomputed on the
host in float64 (scipy.sparse), never the solver's own word:
    ‖b - M·x‖₂ ≤ rtol·‖b‖₂ + 2·(L + 3)·ε·‖ |M|·|x| + |b| ‖₂,   L the longest row (adjoint: column), ε = 2⁻⁵³
(the second term: the rounding bound of a residual evaluated twice in different orders -- derived, not tuned; solve_ref.residual_check)."""
import ctypes as C

import numpy as np
import pytest

import solve_ref as R
from spmv_ref import bits

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MAXITER = 5000


def _csc(n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(n, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


def _rhs(N, k, seed):
    """ones, then random columns"""
    B = np.ones((N, k), order="F")
    B[:, 1:] = np.random.default_rng(seed).standard_normal((N, k - 1))
    return B


def _check_residual(A, X, B, d, sigma, adjoint, what):
    for c, (res, bound) in enumerate(R.residual_check(A, X, B, d, sigma, adjoint, RTOL)):
        print(what, "column", c, "residual", res, "bound", bound)
        assert res <= bound, (what, c, res, bound)


def _same_bits(a, b, what):
    assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), what


@pytest.mark.parametrize("which", ["age", "month"])
@pytest.mark.parametrize("name", R.GRIDS)
def test_residual_on_the_measured_systems(oracle, name, which):
    import otmb_amd.api as api

    T, N, nsurf = R.grid_T(oracle, name)
    A = R.csc_of(N, N, *T)
    d, sigma = R.shift(which, N, nsurf)
    with api.DeviceOperator(_csc(N, *T)) as D:
        for adjoint in (False, True):
            for k in (1, 3):
                B = _rhs(N, k, seed=k + 10 * adjoint)
                X, info = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
                print(name, which, "adjoint", adjoint, "k", k, info)
                assert info.converged.all() and info.status == 0, info
                assert (info.iterations <= MAXITER).all() and (info.iterations > 0).all()
                _check_residual(A, X, B, d, sigma, adjoint, (name, which, adjoint, k))


def test_determinism_and_column_independence(oracle):
    import otmb_amd.api as api

    T, N, nsurf = R.grid_T(oracle, "small_rho3d")
    d, sigma = R.shift("age", N, nsurf)
    B = _rhs(N, 3, seed=4)
    with api.DeviceOperator(_csc(N, *T)) as D:
        for adjoint in (False, True):
            X1, i1 = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
            X2, i2 = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
            assert i1.converged.all()
            _same_bits(X1, X2, "X twice")
            assert np.array_equal(i1.iterations, i2.iterations) and i1.reason == i2.reason
            _same_bits(i1.relres, i2.relres, "relres twice")
            for c in range(3):
                xc, ic = D.solve(B[:, c], d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
                _same_bits(xc, X1[:, c], ("column alone", adjoint, c))
                assert ic.iterations[0] == i1.iterations[c] and ic.reason[0] == i1.reason[c]
                _same_bits(ic.relres[0], i1.relres[c], ("relres alone", adjoint, c))


def test_long_row_path():
    """An arrow matrix: its first row (5000 entries) is beyond SP_ELL_MAX = 256, so A·x goes through the long-row kernel; the adjoint folds
    the first column (5000 entries) in one lane."""
    import otmb_amd.api as api

    n = 5000
    p, i, v = R.arrow(n)
    A = R.csc_of(n, n, p, i, v)
    assert np.bincount(i - 1, minlength=n).max() > 256  # SP_ELL_MAX
    B = _rhs(n, 3, seed=6)
    with api.DeviceOperator(_csc(n, p, i, v)) as D:
        for adjoint in (False, True):
            X, info = D.solve(B, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
            print("arrow", adjoint, info)
            assert info.converged.all(), info
            _check_residual(A, X, B, None, 0.0, adjoint, ("arrow", adjoint))


def _small_system(which):
    """(n, Julia's arrays, d, σ): the arrow matrix whose row 0 (600 entries) is a long row of two LDS chunks (SP_TCH = 512) and whose
    column 0 is clipped across a chunk edge under the adjoint; the random matrix of two row workgroups, five column workgroups and a last
    slice of one row, with d and σ."""
    if which == "arrow":
        return 600, R.arrow(600), None, 0.0
    return 257, R.dominant(257), np.random.default_rng(13).uniform(0.0, 1.0, 257), 0.5


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("which", ["arrow", "dominant"])
def test_register_blocks_and_tracer_groups(which, adjoint):
    """k = 7 is launched as register blocks of 4 + 2 + 1 columns, k = 65 has a second group of 64 columns in the long-row kernel: the
    residual bound holds for every column, and columns 0, 3, 6 (one of each block) and 64 have the bits of that column solved alone."""
    import otmb_amd.api as api

    n, (p, i, v), d, sigma = _small_system(which)
    A = R.csc_of(n, n, p, i, v)
    if which == "arrow":
        assert np.bincount(i - 1, minlength=n).max() > 512 and np.diff(p).max() > 512  # SP_TCH
    B = _rhs(n, 65, seed=11)
    with api.DeviceOperator(_csc(n, p, i, v)) as D:
        alone = {c: D.solve(B[:, c], d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint) for c in (0, 3, 6, 64)}
        for k in (7, 65):
            X, info = D.solve(B[:, :k], d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
            assert info.converged.all() and info.status == 0, info
            _check_residual(A, X, B[:, :k], d, sigma, adjoint, (which, adjoint, k))
            for c in (0, 3, 6, 64)[: 3 + (k == 65)]:
                xc, ic = alone[c]
                _same_bits(xc, X[:, c], ("column alone", which, adjoint, k, c))
                assert ic.iterations[0] == info.iterations[c] and ic.reason[0] == info.reason[c]
                _same_bits(ic.relres[0], info.relres[c], ("relres alone", which, adjoint, k, c))


def test_time_loop_x0_and_padding(oracle):
    import otmb_amd.api as api
    from otmb_amd import capi

    T, N, nsurf = R.grid_T(oracle, "tiny_tripolar")
    d, sigma = R.shift("month", N, nsurf)
    B = _rhs(N, 2, seed=7)
    with api.DeviceOperator(_csc(N, *T)) as D:
        X, info = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER)
        assert info.converged.all()
        # the time loop: new values, the same pattern; the operator's own products are untouched by a solve
        D.set_values(2.0 * T[2])
        A2 = R.csc_of(N, N, T[0], T[1], 2.0 * T[2])
        X2, info2 = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER)
        assert info2.converged.all()
        _check_residual(A2, X2, B, None, sigma, False, "after set_values")
        _same_bits(D.mul(B[:, 1]), api.DeviceOperator(_csc(N, T[0], T[1], 2.0 * T[2])).mul(B[:, 1]), "mul after solve")
        # a start that already passes: zero iterations, X is the start
        X3, info3 = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER, x0=X2)
        assert (info3.iterations == 0).all() and info3.converged.all(), info3
        _same_bits(X3, X2, "x0")
        # padding rows of B and X (ldb, ldx > n) are neither read nor written: the C entry point on padded arrays
        pad = 5
        Bp = np.full((N + pad, 2), np.nan, order="F")
        Bp[:N] = B
        Xp = np.full((N + pad, 2), 7.25, order="F")
        it, rr, why = np.zeros(2, np.int64), np.zeros(2), np.zeros(2, np.int32)
        rc = capi.lib().otmb_op_solve(D.handle, 0, 2, None, float(sigma), Bp.ctypes.data, N + pad, Xp.ctypes.data, N + pad, 0, RTOL, MAXITER,
                                      it.ctypes.data, rr.ctypes.data, why.ctypes.data)
        assert rc == 0 and (why == 0).all()
        assert (Xp[N:] == 7.25).all() and np.isnan(Bp[N:]).all()
        _same_bits(Xp[:N], X2, "padded call")
        assert np.array_equal(it, info2.iterations)


def test_the_jacobi_wrapper_has_the_bits_of_the_keyword():
    """No binding calls otmb_op_solve any more (they hand precond to otmb_op_solve_pc): the wrapper, on padded arrays, still has the bits of
    DeviceOperator.solve with the default and with precond="jacobi".  n = 257 is one full 256-row workgroup plus one row, k = 7 register
    blocks of 4 + 2 + 1 columns."""
    import otmb_amd.api as api
    from otmb_amd import capi

    n, (p, i, v), d, sigma = _small_system("dominant")
    k, pad = 7, 5
    B = _rhs(n, k, seed=17)
    Bp = np.full((n + pad, k), np.nan, order="F")
    Bp[:n] = B
    with api.DeviceOperator(_csc(n, p, i, v)) as D:
        for adjoint in (0, 1):
            Xp = np.full((n + pad, k), 7.25, order="F")
            it, rr, why = np.zeros(k, np.int64), np.zeros(k), np.zeros(k, np.int32)
            rc = capi.lib().otmb_op_solve(D.handle, adjoint, k, d.ctypes.data, float(sigma), Bp.ctypes.data, n + pad, Xp.ctypes.data, n + pad, 0, RTOL,
                                          MAXITER, it.ctypes.data, rr.ctypes.data, why.ctypes.data)
            assert rc == 0 and (why == 0).all() and (it > 0).all()
            assert (Xp[n:] == 7.25).all()
            for kw in ({}, {"precond": "jacobi"}):
                X, info = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=bool(adjoint), **kw)
                assert info.status == 0 and info.converged.all(), info
                _same_bits(X, Xp[:n], ("X", adjoint, kw))
                assert np.array_equal(info.iterations, it), (adjoint, kw)
                _same_bits(info.relres, rr, ("relres", adjoint, kw))


def test_honest_failures(oracle):
    import otmb_amd.api as api
    from otmb_amd import capi
    from otmb_amd.capi import OtmbError

    T, N, nsurf = R.grid_T(oracle, "tiny_bipolar")
    d, sigma = R.shift("age", N, nsurf)
    B = _rhs(N, 3, seed=8)
    with api.DeviceOperator(_csc(N, *T)) as D:
        Xok, iok = D.solve(B, d=d, rtol=RTOL, maxiter=MAXITER)
        assert iok.converged.all()
        # maxiter
        X, info = D.solve(B, d=d, rtol=RTOL, maxiter=3)
        assert info.status == capi.NOT_CONVERGED == 19 and capi.STATUS_NAMES[19] == "NOT_CONVERGED"
        assert info.reason == ("maxiter",) * 3 and (info.iterations == 3).all() and not info.converged.any()
        assert np.isfinite(X).all() and np.isfinite(info.relres).all()
        msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
        assert msg.startswith("solve: not converged")
        assert msg == (f"{capi.lib().otmb_status_string(capi.NOT_CONVERGED).decode()}: 3 of 3 columns; the first is column 1: maxiter after "
                       f"{int(info.iterations[0])} iterations, relative residual {info.relres[0]:.3e}"), msg
        X, info = D.solve(B, d=d, rtol=RTOL, maxiter=0)
        assert info.reason == ("maxiter",) * 3 and (info.iterations == 0).all() and not X.any()
        # B = 0: X = 0 in zero iterations, whatever the start
        X, info = D.solve(np.zeros((N, 2)), d=d, x0=np.ones((N, 2)))
        assert info.converged.all() and (info.iterations == 0).all() and not X.any() and info.status == 0
        # NaN in one column: that column alone stops as nonfinite, the others have the bits of the clean solve
        Bn = B.copy(order="F")
        Bn[N // 2, 1] = np.nan
        X, info = D.solve(Bn, d=d, rtol=RTOL, maxiter=MAXITER)
        assert info.reason == ("converged", "nonfinite", "converged") and info.status == capi.NOT_CONVERGED, info
        _same_bits(X[:, 0], Xok[:, 0], "beside a NaN column")
        _same_bits(X[:, 2], Xok[:, 2], "beside a NaN column")
        assert np.array_equal(info.iterations[[0, 2]], iok.iterations[[0, 2]])
        # argument errors raise and leave the operator usable
        for kw in (dict(rtol=0.0), dict(rtol=-1.0), dict(rtol=np.nan), dict(maxiter=-1)):
            with pytest.raises(OtmbError) as e:
                D.solve(B, d=d, **kw)
            assert e.value.name == "INVALID_ARG", kw
        with pytest.raises(OtmbError) as e:
            D.solve(B[:-1], d=d)
        assert e.value.name == "INVALID_ARG"
        with pytest.raises(OtmbError) as e:
            D.solve(B, d=d[:-1])
        assert e.value.name == "INVALID_ARG"
        it, rr, why = np.zeros(3, np.int64), np.zeros(3), np.zeros(3, np.int32)
        Xc = np.zeros((N, 3), order="F")
        args = [D.handle, 0, 3, None, 1.0, B.ctypes.data, N, Xc.ctypes.data, N, 0, RTOL, 10, it.ctypes.data, rr.ctypes.data, why.ctypes.data]
        for pos, bad in ((2, 0), (6, N - 1), (8, N - 1), (5, None), (7, None), (12, None), (13, None), (14, None)):
            a = list(args)
            a[pos] = bad
            assert capi.lib().otmb_op_solve(*a) == 11, pos
        assert capi.lib().otmb_op_solve(None, *args[1:]) == 11
        X, info = D.solve(B, d=d, rtol=RTOL, maxiter=MAXITER)
        _same_bits(X, Xok, "after the errors")
    # a zero diagonal entry: refused before iterating, the message names the first (rows 3 and 5 of a 6 x 6 matrix, 1-based)
    p = np.arange(1, 8)
    i = np.arange(1, 7)
    v = np.array([1.0, 2.0, 0.0, 4.0, 0.0, 6.0])
    with api.DeviceOperator(_csc(6, p, i, v)) as Z:
        with pytest.raises(OtmbError) as e:
            Z.solve(np.ones(6))
        assert e.value.name == "SINGULAR_PRECONDITIONER" and e.value.status == 18 and "diag(M)[3]" in str(e.value), str(e.value)
        with pytest.raises(OtmbError) as e:
            Z.solve(np.ones(6), sigma=np.inf)
        assert e.value.name == "SINGULAR_PRECONDITIONER" and "diag(M)[1]" in str(e.value)
        X, info = Z.solve(np.ones(6), sigma=1.0)  # (σ makes it regular: a diagonal system is solved in one iteration)
        assert info.converged.all() and np.allclose(X, 1.0 / (1.0 + v), rtol=1e-9)
    # a rectangular operator
    import otmb_amd.api as api2

    rect = api2.SparseMatrixCSC(3, 2, np.array([1, 2, 3], dtype=np.int64), np.array([1, 2], dtype=np.int64), np.array([1.0, 1.0]))
    with api.DeviceOperator(rect) as Q:
        with pytest.raises(OtmbError) as e:
            Q.solve(np.ones(3))
        assert e.value.name == "INVALID_ARG" and "square" in str(e.value)


def test_device_route_has_the_bits_of_the_host_api():
    """DeviceAssembler.solve on device tensors (otmb_op_solve_dev on torch's memory) against api.DeviceOperator.solve on the downloaded T."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _host, _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    del full
    asm.step(umo, vmo, fill)
    N = asm.N
    T = _host(asm)["T"]
    nsurf = int(np.count_nonzero(asm.wet3d.cpu().numpy().reshape(g.umo.data.shape, order="F")[:, :, 0]))
    d, sigma = R.shift("age", N, nsurf)
    B = _rhs(N, 3, seed=9)
    Bd = torch.from_numpy(B).cuda().t().contiguous().t()
    for adjoint in (False, True):
        Xd, idev = asm.solve("T", Bd, d=torch.from_numpy(d).cuda(), sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
        with api.DeviceOperator(_csc(N, *T)) as D:
            Xh, ihost = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
        assert idev.converged.all() and ihost.converged.all()
        _same_bits(Xd.cpu().numpy(), Xh, ("device route", adjoint))
        assert np.array_equal(idev.iterations, ihost.iterations)
        _same_bits(idev.relres, ihost.relres, "relres")
        _check_residual(R.csc_of(N, N, *T), Xh, B, d, sigma, adjoint, ("device route", adjoint))
    x1, i1 = asm.solve("T", Bd[:, 0].contiguous(), d=torch.from_numpy(d).cuda(), sigma=sigma, rtol=RTOL, maxiter=MAXITER)
    assert x1.dim() == 1 and i1.converged.all()
