"""The line preconditioner on the device (csrc/otmb_solve_lines.hip; otmb_op_set_lines, otmb_op_precond, otmb_op_solve_pc): the sweep bit
for bit against the numpy restatement (tests/solve_lines_ref.py), solves accepted by the float64 residual bound of tests/test_solve.py
(solve_ref.residual_check: never the solver's own word), what the lines buy in iterations, and the refusals."""
import numpy as np
import pytest

import solve_lines_ref as LR
import solve_ref as R
from spmv_ref import bits

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MAXITER = 5000
N0 = 257


def _csc(n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(n, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


def _rhs(N, k, seed):
    B = np.ones((N, k), order="F")
    B[:, 1:] = np.random.default_rng(seed).standard_normal((N, k - 1))
    return B


def _same_bits(a, b, what):
    assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))), what


def _check_residual(A, X, B, d, sigma, adjoint, what):
    for c, (res, bound) in enumerate(R.residual_check(A, X, B, d, sigma, adjoint, RTOL)):
        print(what, "column", c, "residual", res, "bound", bound)
        assert res <= bound, (what, c, res, bound)


@pytest.fixture(scope="module")
def dominant():
    """(A as scipy CSC, Julia's arrays, d, σ) of solve_ref.dominant(257) and one DeviceOperator over it."""
    import otmb_amd.api as api

    p, i, v = R.dominant(N0)
    d = np.random.default_rng(13).uniform(0.0, 1.0, N0)
    with api.DeviceOperator(_csc(N0, p, i, v)) as D:
        yield R.csc_of(N0, N0, p, i, v), D, d, 0.5


LINE_SETS = [("none", lambda: np.zeros(N0, dtype=np.int64)), ("one line of 257", lambda: LR.stride_lines(N0, 1)),
             ("64 lines", lambda: LR.stride_lines(N0, 64)), ("65 lines", lambda: LR.stride_lines(N0, 65))] + \
            [(f"random {s}", (lambda s=s: LR.random_lines(N0, s))) for s in range(20)]


@pytest.mark.parametrize("what,make", LINE_SETS, ids=[w for w, _ in LINE_SETS])
def test_sweep_bits(dominant, what, make):
    """precondition() is the restatement bit for bit: k = 1, 3, 5 (register blocks 1; 2 + 1; 4 + 1), A and Aᵀ, random d and σ = 0.5.
    One line of 257 crosses every workgroup boundary, next[i] = i + 64 steps across waves, 65 lines leave one live lane in the last wave."""
    A, D, d, sigma = dominant
    nxt = make()
    D.set_lines(nxt)
    Y = np.asfortranarray(np.random.default_rng(3).standard_normal((N0, 5)))
    for adjoint in (False, True):
        P = LR.Lines(A, nxt, d, sigma, adjoint)
        assert len(P.heads) == {"none": 257, "one line of 257": 1, "64 lines": 64, "65 lines": 65}.get(what, len(P.heads))
        want = P.apply(Y)
        for k in (1, 3, 5):
            Z = D.precondition(Y[:, :k], d=d, sigma=sigma, adjoint=adjoint)
            _same_bits(Z, want[:, :k], (what, adjoint, k))
        _same_bits(D.precondition(Y[:, 2], d=d, sigma=sigma, adjoint=adjoint), want[:, 2], (what, adjoint, "1-D"))
        if what == "none":
            diag = R.jacobi_diagonal(A, d, sigma)
            _same_bits(want, Y / diag[:, None], "no lines: y ./ diag")
            _same_bits(D.precondition(Y, d=d, sigma=sigma, adjoint=adjoint, precond="jacobi"), Y / diag[:, None], "jacobi")


@pytest.mark.parametrize("which", ["age", "month"])
@pytest.mark.parametrize("name", ["tiny_tripolar", "odd_nx_fold", "small_rho3d"])
def test_sweep_bits_on_water_columns(oracle, name, which):
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, name)
    A = R.csc_of(N, N, *T)
    d, sigma = R.shift(which, N, nsurf)
    Y = _rhs(N, 3, seed=5)
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        for adjoint in (False, True):
            _same_bits(D.precondition(Y, d=d, sigma=sigma, adjoint=adjoint), LR.Lines(A, nxt, d, sigma, adjoint).apply(Y), (name, which, adjoint))


def test_leading_dimensions(dominant):
    """ldy, ldz > n through the C ABI: the padding rows of Y are not read (NaN), those of Z are not written."""
    from otmb_amd import capi

    A, D, d, sigma = dominant
    nxt = LR.random_lines(N0, 3)
    D.set_lines(nxt)
    Y = np.asfortranarray(np.random.default_rng(4).standard_normal((N0, 3)))
    Yp = np.full((N0 + 3, 3), np.nan, order="F")
    Yp[:N0] = Y
    for pc, want in ((1, LR.Lines(A, nxt, d, sigma).apply(Y)), (0, Y / R.jacobi_diagonal(A, d, sigma)[:, None])):
        Zp = np.full((N0 + 7, 3), 7.25, order="F")
        rc = capi.lib().otmb_op_precond(D.handle, 0, pc, 3, d.ctypes.data, float(sigma), Yp.ctypes.data, N0 + 3, Zp.ctypes.data, N0 + 7)
        assert rc == 0
        assert (Zp[N0:] == 7.25).all() and np.isnan(Yp[N0:]).all()
        _same_bits(Zp[:N0], want, ("padded", pc))


@pytest.mark.parametrize("which", ["age", "month"])
@pytest.mark.parametrize("name", R.GRIDS)
def test_solves_with_lines(oracle, name, which):
    """Every grid x {age, month} x {A, Aᵀ} x k in {1, 3} converges with lines and meets the residual bound.  On the month systems both
    preconditioners are run: 4·iterations(lines) ≤ iterations(Jacobi) (the CPU restatement's ratio is at least 50; the factor 4 leaves room
    for the device's summation order)."""
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, name)
    A = R.csc_of(N, N, *T)
    d, sigma = R.shift(which, N, nsurf)
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        for adjoint in (False, True):
            for k in (1, 3):
                B = _rhs(N, k, seed=k + 10 * adjoint)
                X, info = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines")
                print(name, which, "adjoint", adjoint, "k", k, "lines", info)
                assert info.converged.all() and info.status == 0, info
                assert (info.iterations > 0).all()
                _check_residual(A, X, B, d, sigma, adjoint, (name, which, adjoint, k))
                if which == "month" and k == 1:
                    Xj, ij = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
                    print(name, which, "adjoint", adjoint, "iterations: jacobi", ij.iterations[0], "lines", info.iterations[0])
                    assert ij.converged.all()
                    assert 4 * info.iterations[0] <= ij.iterations[0]


@pytest.mark.parametrize("adjoint", [False, True])
def test_year_system_converges_with_lines(oracle, adjoint):
    """σ = 1 / 365 d on 90 x 60 x 20: 14 935 Jacobi iterations (its adjoint: none within 20 000) on the CPU restatement, 20 with lines;
    maxiter = 200 is tenfold that, for the device's summation order."""
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, "90x60x20")
    d, sigma = R.shift("year", N, nsurf)
    B = np.ones(N)
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        X, info = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=200, adjoint=adjoint, precond="lines")
        print("year, adjoint", adjoint, info)
        assert info.converged.all() and info.iterations[0] <= 200
        _check_residual(R.csc_of(N, N, *T), X, B, None, sigma, adjoint, ("year", adjoint))


def test_no_lines_is_jacobi_and_columns_are_independent(oracle):
    import otmb_amd.api as api

    T, N, nsurf, nxt = LR.grid(oracle, "small_rho3d")
    d, sigma = R.shift("age", N, nsurf)
    B = _rhs(N, 3, seed=4)
    with api.DeviceOperator(_csc(N, *T)) as D:
        # next all zero: the bits of the Jacobi solve
        D.set_lines(np.zeros(N, dtype=np.int64))
        for adjoint in (False, True):
            Xj, ij = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint)
            Xl, il = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines")
            assert ij.converged.all()
            _same_bits(Xl, Xj, ("no lines", adjoint))
            assert np.array_equal(il.iterations, ij.iterations) and il.reason == ij.reason
            _same_bits(il.relres, ij.relres, "relres")
        # determinism and column independence with the water columns
        D.set_lines(nxt)
        for adjoint in (False, True):
            X1, i1 = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines")
            X2, i2 = D.solve(B, d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines")
            assert i1.converged.all()
            _same_bits(X1, X2, "X twice")
            assert np.array_equal(i1.iterations, i2.iterations) and i1.reason == i2.reason
            _same_bits(i1.relres, i2.relres, "relres twice")
            for c in range(3):
                xc, ic = D.solve(B[:, c], d=d, sigma=sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond="lines")
                _same_bits(xc, X1[:, c], ("column alone", adjoint, c))
                assert ic.iterations[0] == i1.iterations[c] and ic.reason[0] == i1.reason[c]
                _same_bits(ic.relres[0], i1.relres[c], ("relres alone", adjoint, c))


def test_x0_frozen_column_and_set_values(oracle):
    import otmb_amd.api as api
    from otmb_amd.capi import OtmbError

    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    d, sigma = R.shift("month", N, nsurf)
    A = R.csc_of(N, N, *T)
    B = _rhs(N, 3, seed=7)
    B[:, 1] = 0.0  # a column that stops at once: x = 0, frozen while the others run
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        X, info = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond="lines", x0=np.ones((N, 3)))
        assert info.converged.all() and info.iterations[1] == 0 and not X[:, 1].any() and (info.iterations[[0, 2]] > 0).all()
        _check_residual(A, X, B, None, sigma, False, "b = 0 beside two columns")
        for c in (0, 2):
            xc, ic = D.solve(B[:, c], sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond="lines", x0=np.ones(N))
            _same_bits(xc, X[:, c], ("beside the frozen column", c))
        # a start that already passes: zero iterations, X is the start
        X3, i3 = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond="lines", x0=X)
        assert (i3.iterations == 0).all() and i3.converged.all()
        _same_bits(X3, X, "x0")
        # lines belong to the pattern: they still apply after new values
        D.set_values(2.0 * T[2])
        A2 = R.csc_of(N, N, T[0], T[1], 2.0 * T[2])
        Y = _rhs(N, 2, seed=2)
        _same_bits(D.precondition(Y, sigma=sigma), LR.Lines(A2, nxt, None, sigma).apply(Y), "after set_values")
        X2, i2 = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond="lines")
        assert i2.converged.all()
        _check_residual(A2, X2, B, None, sigma, False, "after set_values")
        # cleared lines are refused afterwards; Jacobi still runs
        D.set_lines(None)
        with pytest.raises(OtmbError) as e:
            D.solve(B, sigma=sigma, precond="lines")
        assert e.value.name == "INVALID_ARG" and "otmb_op_set_lines" in str(e.value)
        with pytest.raises(OtmbError) as e:
            D.precondition(B, sigma=sigma)
        assert e.value.name == "INVALID_ARG"
        assert D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER)[1].converged.all()


def test_refusals(dominant):
    import otmb_amd.api as api
    from otmb_amd import capi
    from otmb_amd.capi import OtmbError

    A, D, d, sigma = dominant
    n = N0
    good = LR.random_lines(n, 1)
    D.set_lines(good)
    Y = _rhs(n, 2, seed=1)
    want = LR.Lines(A, good, d, sigma).apply(Y)
    # each rule, by the first offending 1-based index; the operator keeps the lines it had
    for at, val in ((100, 101), (100, 7), (100, n + 1), (100, -3), (n - 1, n)):
        bad = np.zeros(n, dtype=np.int64)
        bad[at] = val
        bad[200] = 1  # (a later offender)
        with pytest.raises(OtmbError) as e:
            D.set_lines(bad)
        assert e.value.name == "INVALID_ARG" and f"next[{min(at, 200) + 1}]" in str(e.value), str(e.value)
        with pytest.raises(LR.InvalidLines) as r:
            LR.successors(bad, n)
        assert r.value.index == min(at, 200)
    bad = np.zeros(n, dtype=np.int64)
    bad[[3, 5, 10, 11]] = (50, 50, 40, 40)
    with pytest.raises(OtmbError) as e:
        D.set_lines(bad)
    assert e.value.name == "INVALID_ARG" and "index 40 " in str(e.value), str(e.value)
    _same_bits(D.precondition(Y, d=d, sigma=sigma), want, "the lines from before the refusals")
    with pytest.raises(OtmbError) as e:
        D.set_lines(np.zeros(n - 1, dtype=np.int64))
    assert e.value.name == "INVALID_ARG"
    # an unknown preconditioner, at both layers
    with pytest.raises(OtmbError) as e:
        D.solve(Y, precond="ilu")
    assert e.value.name == "INVALID_ARG"
    it, rr, why = np.zeros(2, np.int64), np.zeros(2), np.zeros(2, np.int32)
    Xc = np.full((n, 2), 7.25, order="F")
    args = [D.handle, 0, 2, None, 1.0, Y.ctypes.data, n, Xc.ctypes.data, n, 0, RTOL, 10, it.ctypes.data, rr.ctypes.data, why.ctypes.data]
    assert capi.lib().otmb_op_solve_pc(*args, 2) == 11 and capi.lib().otmb_op_solve_pc(*args, -1) == 11
    assert capi.lib().otmb_op_precond(D.handle, 0, 2, 2, None, 1.0, Y.ctypes.data, n, Xc.ctypes.data, n) == 11
    assert capi.lib().otmb_op_precond(D.handle, 0, 1, 2, None, 1.0, Y.ctypes.data, n - 1, Xc.ctypes.data, n) == 11
    assert capi.lib().otmb_op_set_lines(None, None) == 11 and (Xc == 7.25).all()
    # LINES on an operator that never had lines
    with api.DeviceOperator(_csc(n, *R.dominant(n))) as E:
        with pytest.raises(OtmbError) as e:
            E.solve(Y, precond="lines")
        assert e.value.name == "INVALID_ARG" and "otmb_op_set_lines" in str(e.value)
    # a rectangular operator has no lines
    rect = api.SparseMatrixCSC(3, 2, np.array([1, 2, 3], dtype=np.int64), np.array([1, 2], dtype=np.int64), np.array([1.0, 1.0]))
    with api.DeviceOperator(rect) as Q:
        with pytest.raises(OtmbError) as e:
            Q.set_lines(np.zeros(2, dtype=np.int64))
        assert e.value.name == "INVALID_ARG" and "square" in str(e.value)
    # a zero pivot: [[2, 4], [1, 2]] on the line 1 -> 2 gives m_2 = 1 / 2, piv_2 = 2 - (1 / 2)·4 = 0 exactly; X is not touched
    p, i, v = np.array([1, 3, 5, 6]), np.array([1, 2, 1, 2, 3]), np.array([2.0, 1.0, 4.0, 2.0, 1.0])
    with api.DeviceOperator(_csc(3, p, i, v)) as Z:
        Z.set_lines(np.array([2, 0, 0]))
        B3 = np.ones((3, 1), order="F")
        X3 = np.full((3, 1), 7.25, order="F")
        rc = capi.lib().otmb_op_solve_pc(Z.handle, 0, 1, None, 0.0, B3.ctypes.data, 3, X3.ctypes.data, 3, 0, RTOL, 10, it.ctypes.data, rr.ctypes.data,
                                         why.ctypes.data, 1)
        assert rc == 18 and (X3 == 7.25).all()
        with pytest.raises(OtmbError) as e:
            Z.solve(np.ones(3), precond="lines")
        assert e.value.name == "SINGULAR_PRECONDITIONER" and "pivot[2]" in str(e.value), str(e.value)
        with pytest.raises(OtmbError) as e:
            Z.precondition(np.ones(3))
        assert e.value.name == "SINGULAR_PRECONDITIONER" and "pivot[2]" in str(e.value)
        with pytest.raises(LR.SingularLines) as r:
            LR.Lines(R.csc_of(3, 3, p, i, v), np.array([2, 0, 0]))
        assert r.value.index == 1
        X, info = Z.solve(np.ones(3), sigma=1.0, precond="lines")  # (σ makes it regular; P = M here: one iteration)
        assert info.converged.all() and np.allclose(R.system(R.csc_of(3, 3, p, i, v), None, 1.0) @ X, 1.0, rtol=1e-12)


def test_assembler_solves_with_its_own_water_columns():
    """DeviceAssembler.solve(matrix="T", precond="lines") on device tensors: the lines come from the assembler's own indices (torch ops) and
    are those of api.vertical_lines; the solve has the bits of api.DeviceOperator's on the downloaded T."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _host, _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    del full
    asm.step(umo, vmo, fill)
    N = asm.N
    T = _host(asm)["T"]
    nxt = api.vertical_lines(api.makeindices(gm.v3D))
    assert np.array_equal(asm.vertical_lines().cpu().numpy(), nxt) and np.count_nonzero(nxt) > 0
    sigma = R.shift("month", N, 0)[1]
    B = _rhs(N, 3, seed=9)
    Bd = torch.from_numpy(B).cuda().t().contiguous().t()
    Xd, idev = asm.solve("T", Bd, sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond="lines")
    with api.DeviceOperator(_csc(N, *T)) as D:
        D.set_lines(nxt)
        Xh, ihost = D.solve(B, sigma=sigma, rtol=RTOL, maxiter=MAXITER, precond="lines")
    assert idev.converged.all() and ihost.converged.all()
    _same_bits(Xd.cpu().numpy(), Xh, "device route")
    assert np.array_equal(idev.iterations, ihost.iterations)
    _check_residual(R.csc_of(N, N, *T), Xh, B, None, sigma, False, "device route")
    Zd = asm.operator("T").precondition(Bd, sigma=sigma)
    _same_bits(Zd.cpu().numpy(), LR.Lines(R.csc_of(N, N, *T), nxt, None, sigma).apply(B), "precondition on device tensors")
