"""GPU: the solver's, the preconditioners' and the step's `_dev` entry points (otmb_op_solve_pc_dev, otmb_op_precond_dev, otmb_op_step_dev)
on column-major device arrays whose leading dimension is NOT n.  The host entry points stage compactly and call these with ld = n, and
device.Operator hands over compact results, so every other test of csrc/otmb_solve.hip, otmb_solve_lines.hip and otmb_step.hip runs the
kernels at ld = n only; tests/test_spmv_edges.py::test_padded_leading_dimensions is the same check for otmb_op_mul_dev.

Every padded array is an (n + pad, k) column-major tensor with a pad of its own -- B or Y + 3, X or Z + 5, S + 7 -- so that no swapped or
dropped leading dimension can cancel.  Padding rows of inputs hold NaN, those of outputs the sentinel 7.25.  Asserted per call: status OK,
the outputs' padding keeps its bits, every input keeps its bits (padding included), and rows [:n] have THE BITS of the same call on
compact arrays (a leading dimension changes addresses, never the order of a sum); for the solver also iterations, relres and reasons, and
the float64 residual bound of tests/solve_ref.py against scipy.  No other tolerance appears here.

Fixtures, the smallest that reach every kernel: solve_ref.dominant(257) with solve_lines_ref.random_lines(257, 3) (one full 256-row
workgroup and one row more, five 64-lane column workgroups, a last slice of one row; d uniform(0, 1), σ = 0.5; k = 7: register blocks
4 + 2 + 1) and solve_ref.arrow(600) (a long row of two LDS chunks, under the adjoint a column across a chunk edge; Jacobi; k = 65: a second
group of 64 tracers in the long-row kernels of the solver and of the step)."""
import ctypes as C

import numpy as np
import pytest

import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MAXITER = 5000
SENTINEL = 7.25
PAD_B, PAD_X, PAD_S = 3, 5, 7  # B or Y, X or Z, S
NSTEPS, FIRST, DT = 4, 2, 2.0


def _raw(a):
    """The bit patterns of a float64 array (host, or a device tensor)."""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b, what):
    assert np.array_equal(_raw(a), _raw(b)), what


def _pad(a, pad, fill):
    """An (n + pad, k) column-major device tensor: rows [:n] hold the host array a (n x k), the padding rows `fill`."""
    import torch

    n, k = a.shape
    t = torch.full((k, n + pad), fill, dtype=torch.float64, device="cuda").t()
    t[:n] = torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()
    assert t.stride() == (1, n + pad)
    return t


def _rhs(n, k, seed):
    B = np.ones((n, k), order="F")
    B[:, 1:] = np.random.default_rng(seed).standard_normal((n, k - 1))
    return B


class _System:
    """A device.Operator with the three slots of tests/step_ref.py (slot 0, the matrix itself, selected) on the assembler's context, so that
    torch's stream is the library's; the matrix for scipy; d on both sides; k."""

    def __init__(self, ctx, n, arrays, d, sigma, k, nxt=None):
        import torch

        from otmb_amd.device import Operator

        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
        p, i, v = arrays
        self.n, self.k, self.d, self.sigma = n, k, d, sigma
        self.A = R.csc_of(n, n, p, i, v)
        self.O = Operator(ctx, n, n, t(p, np.int64), t(i, np.int64), t(v, np.float64))
        self.O.set_slots(3)
        for s, vals in enumerate(SR.slot_values(v, seed=1)):
            self.O.set_values_dev(t(vals, np.float64), slot=s)
        if nxt is not None:
            self.O.set_lines(t(nxt, np.int64))
        self.dd = None if d is None else t(d, np.float64)
        self.lib, self.h = self.O.lib, self.O.handle


@pytest.fixture(scope="module")
def systems():
    from otmb_amd.device import DeviceAssembler

    ctx = DeviceAssembler(0).ctx  # (on torch's current stream)
    dom = _System(ctx, 257, R.dominant(257), np.random.default_rng(13).uniform(0.0, 1.0, 257), 0.5, 7, nxt=LR.random_lines(257, 3))
    arr = _System(ctx, 600, R.arrow(600), None, 0.0, 65)
    i = R.arrow(600)[1]
    assert np.bincount(i - 1, minlength=600).max() > 512  # SP_TCH: two chunks
    yield {"dominant": dom, "arrow": arr}
    dom.O.close()
    arr.O.close()


CASES = [("dominant", 0), ("dominant", 1), ("arrow", 0)]  # (fixture, otmb_precond)
IDS = ["dominant-jacobi", "dominant-lines", "arrow-jacobi"]


# ---- otmb_op_solve_pc_dev ----------------------------------------------------------------------------------------------------------------
def _solve(P, adjoint, pc, B, ldb, X, ldx, use_x0):
    k = P.k
    it, rr, why = np.full(k, -7, np.int64), np.full(k, SENTINEL), np.full(k, -7, np.int32)
    rc = P.lib.otmb_op_solve_pc_dev(P.h, adjoint, k, None if P.dd is None else P.dd.data_ptr(), float(P.sigma), B.data_ptr(), ldb, X.data_ptr(),
                                    ldx, use_x0, RTOL, MAXITER, it.ctypes.data, rr.ctypes.data, why.ctypes.data, pc)
    return rc, it, rr, why


@pytest.mark.parametrize("use_x0", [0, 1])
@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("which,pc", CASES, ids=IDS)
def test_solve_pc_dev_padded(systems, which, pc, adjoint, use_x0):
    P = systems[which]
    n, k = P.n, P.k
    B = _rhs(n, k, seed=11)
    # a start is a rough one (the solve must iterate); without one X holds the sentinel everywhere: it is not read
    X0 = np.random.default_rng(12).standard_normal((n, k)) if use_x0 else np.full((n, k), SENTINEL)
    what = (which, pc, adjoint, use_x0)
    Bc, Xc = _pad(B, 0, np.nan), _pad(X0, 0, SENTINEL)
    rc, itc, rrc, whyc = _solve(P, adjoint, pc, Bc, n, Xc, n, use_x0)
    assert rc == 0 and (whyc == 0).all() and (itc > 0).all(), (what, "compact", rc, whyc, itc)
    Bp, Xp = _pad(B, PAD_B, np.nan), _pad(X0, PAD_X, SENTINEL)
    before = Bp.clone()
    rc, it, rr, why = _solve(P, adjoint, pc, Bp, n + PAD_B, Xp, n + PAD_X, use_x0)
    print(what, "iterations", it.tolist())
    assert rc == 0, (what, rc)
    _same(Xp[n:], np.full((PAD_X, k), SENTINEL), (what, "padding rows of X were written"))
    _same(Bp, before, (what, "B was written"))
    _same(Bc, B, (what, "B was written (compact)"))
    _same(Xp[:n], Xc, (what, "X"))
    assert np.array_equal(it, itc) and np.array_equal(why, whyc), (what, it, itc, why, whyc)
    _same(rr, rrc, (what, "relres"))
    for c, (res, bound) in enumerate(R.residual_check(P.A, Xp[:n].cpu().numpy(), B, P.d, P.sigma, bool(adjoint), RTOL)):
        print(what, "column", c, "residual", res, "bound", bound)
        assert res <= bound, (what, c, res, bound)


# ---- otmb_op_precond_dev -----------------------------------------------------------------------------------------------------------------
def _precond(P, adjoint, pc, Y, ldy, Z, ldz):
    return P.lib.otmb_op_precond_dev(P.h, adjoint, pc, P.k, P.dd.data_ptr(), float(P.sigma), Y.data_ptr(), ldy, Z.data_ptr(), ldz)


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("pc", [0, 1], ids=["jacobi", "lines"])
def test_precond_dev_padded(systems, pc, adjoint):
    """Z = P⁻¹·Y out of place at ldy = n + 3, ldz = n + 5, and in place (the header: "Z may be Y") at ldz = ldy = n + 3; the compact call
    they are compared with has the restatement's bits (tests/solve_lines_ref.py; Jacobi: Y ./ diag)."""
    P = systems["dominant"]
    n, k = P.n, P.k
    Y = np.asfortranarray(np.random.default_rng(21).standard_normal((n, k)))
    what = (pc, adjoint)
    Yc, Zc = _pad(Y, 0, np.nan), _pad(np.full((n, k), SENTINEL), 0, SENTINEL)
    assert _precond(P, adjoint, pc, Yc, n, Zc, n) == 0
    nxt = LR.random_lines(n, 3)
    want = LR.Lines(P.A, nxt, P.d, P.sigma, bool(adjoint)).apply(Y) if pc else Y / R.jacobi_diagonal(P.A, P.d, P.sigma)[:, None]
    _same(Zc, want, (what, "compact against the restatement"))
    _same(Yc, Y, (what, "Y was written (compact)"))
    Yp, Zp = _pad(Y, PAD_B, np.nan), _pad(np.full((n, k), SENTINEL), PAD_X, SENTINEL)
    before = Yp.clone()
    assert _precond(P, adjoint, pc, Yp, n + PAD_B, Zp, n + PAD_X) == 0
    _same(Zp[n:], np.full((PAD_X, k), SENTINEL), (what, "padding rows of Z were written"))
    _same(Yp, before, (what, "Y was written"))
    _same(Zp[:n], Zc, (what, "Z"))
    # in place: the array is input and output, its padding (NaN) must keep its bits
    assert _precond(P, adjoint, pc, Yp, n + PAD_B, Yp, n + PAD_B) == 0
    _same(Yp[n:], before[n:], (what, "in place: padding rows were written"))
    _same(Yp[:n], Zc, (what, "in place"))


# ---- otmb_op_step_dev --------------------------------------------------------------------------------------------------------------------
def _step(P, adjoint, pc, theta, k, d, S, lds, X, ldx, nsteps=NSTEPS, first=FIRST):
    it, rr, why = np.full((nsteps, k), -7, np.int64), np.full((nsteps, k), SENTINEL), np.full((nsteps, k), -7, np.int32)
    done = C.c_int64(-7)
    rc = P.lib.otmb_op_step_dev(P.h, adjoint, k, None if d is None else d.data_ptr(), DT, float(theta), nsteps, first,
                                None if S is None else S.data_ptr(), lds, X.data_ptr(), ldx, RTOL, MAXITER, pc, C.byref(done), it.ctypes.data,
                                rr.ctypes.data, why.ctypes.data)
    return rc, done.value, it, rr, why


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("which,pc", CASES, ids=IDS)
def test_step_dev_padded(systems, which, pc, theta, adjoint):
    """4 steps from slot 2 over the 3 slots, δt = 2, with and without S (lds = n + 7) and d, X at ldx = n + 5.  On `arrow` (k = 65) column
    64, the only lane of the long-row kernel's second group of 64 tracers, also has the bits and the iterations of that column stepped
    alone."""
    import torch

    P = systems[which]
    n, k = P.n, P.k
    X0 = _rhs(n, k, seed=31)
    S0 = np.asfortranarray(np.random.default_rng(32).standard_normal((n, k)))
    dstep = torch.from_numpy(np.random.default_rng(33).uniform(0.0, 1.0, n)).cuda()
    for has_s in (True, False):
        for has_d in (True, False):
            what = (which, pc, theta, adjoint, "S" if has_s else "no S", "d" if has_d else "no d")
            d = dstep if has_d else None
            Xc, Sc = _pad(X0, 0, SENTINEL), (_pad(S0, 0, np.nan) if has_s else None)
            rc, done, itc, rrc, whyc = _step(P, adjoint, pc, theta, k, d, Sc, n if has_s else 0, Xc, n)
            assert rc == 0 and done == NSTEPS and (whyc == 0).all() and (itc > 0).any(), (what, "compact", rc, done, whyc, itc)
            Xp, Sp = _pad(X0, PAD_X, SENTINEL), (_pad(S0, PAD_S, np.nan) if has_s else None)
            before = Sp.clone() if has_s else None
            dbefore = dstep.clone()
            rc, done, it, rr, why = _step(P, adjoint, pc, theta, k, d, Sp, n + PAD_S if has_s else 0, Xp, n + PAD_X)
            assert rc == 0 and done == NSTEPS, (what, rc, done)
            _same(Xp[n:], np.full((PAD_X, k), SENTINEL), (what, "padding rows of X were written"))
            if has_s:
                _same(Sp, before, (what, "S was written"))
                _same(Sc, S0, (what, "S was written (compact)"))
            _same(dstep, dbefore, (what, "d was written"))
            _same(Xp[:n], Xc, (what, "X"))
            assert np.array_equal(it, itc) and np.array_equal(why, whyc), (what, it, itc)
            _same(rr, rrc, (what, "relres"))
            assert P.O.slots == (3, 0), what  # the selection is the caller's
            if which == "arrow":
                x1 = _pad(X0[:, 64:65], 0, SENTINEL)
                s1 = _pad(S0[:, 64:65], 0, np.nan) if has_s else None
                rc, done, it1, _, why1 = _step(P, adjoint, pc, theta, 1, d, s1, n if has_s else 0, x1, n)
                assert rc == 0 and done == NSTEPS, (what, "column 64 alone", rc, done)
                _same(Xp[:n, 64:65], x1, (what, "column 64 alone"))
                assert np.array_equal(it1[:, 0], it[:, 64]), (what, "column 64 alone: iterations", it1[:, 0], it[:, 64])


# ---- device.Operator where it can produce ld > n -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,precond", [("dominant", "jacobi"), ("dominant", "lines"), ("arrow", "jacobi")], ids=IDS)
def test_python_device_route_with_row_slices(systems, which, precond):
    """Operator.solve(B=...) and Operator.step(source=...) take a row slice big[:n] of a larger column-major tensor uncopied (_col_major hands
    ld = big.stride(1)): the results have the bits of the same call on a compact copy."""
    from otmb_amd.device import _col_major

    P = systems[which]
    n, k = P.n, P.k
    B = _rhs(n, k, seed=41)
    X0 = _rhs(n, k, seed=42)
    big, bigx = _pad(B, PAD_B, np.nan), _pad(X0, PAD_X, np.nan)
    Bv, Xv = big[:n], bigx[:n]
    assert _col_major(Bv, n)[1] == n + PAD_B and _col_major(Bv, n)[0].data_ptr() == big.data_ptr()
    Bc, Xc = _pad(B, 0, np.nan), _pad(X0, 0, np.nan)
    for adjoint in (False, True):
        kw = dict(d=P.dd, sigma=P.sigma, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
        Xs, i_s = P.O.solve(Bv, x0=Xv, **kw)
        Xw, i_w = P.O.solve(Bc, x0=Xc, **kw)
        assert i_s.status == i_w.status == 0 and np.array_equal(i_s.iterations, i_w.iterations), (which, adjoint, i_s, i_w)
        _same(Xs, Xw, (which, adjoint, "solve"))
        _same(big, _pad(B, PAD_B, np.nan), "B is not modified")
        for theta in (1.0, 0.5):
            kw = dict(dt=DT, theta=theta, nsteps=NSTEPS, first_slot=FIRST, d=P.dd, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
            Xs, i_s = P.O.step(Xv, source=Bv, **kw)
            Xw, i_w = P.O.step(Xc, source=Bc, **kw)
            assert i_s.status == i_w.status == 0 and i_s.steps_done == i_w.steps_done == NSTEPS, (which, adjoint, theta, i_s, i_w)
            assert np.array_equal(i_s.iterations, i_w.iterations)
            _same(Xs, Xw, (which, adjoint, theta, "step"))
            _same(big, _pad(B, PAD_B, np.nan), "the source is not modified")
            _same(bigx, _pad(X0, PAD_X, np.nan), "X is not modified")
