"""GPU: the per-column `_dev` entry points (otmb_op_solve_dk_dev, otmb_op_precond_dk_dev, otmb_op_step_dk_dev, otmb_op_periodic_dk_dev) with
D at a leading dimension above n, in the style of tests/test_op_padded_dev.py: the padding rows of D hold NaN and are not read, ldd odd and
even, D a view at an 8-byte but not 16-byte aligned offset -- every result has THE BITS of the same call with D compact, D keeps its bits,
and device.Operator's 2-D d (a torch tensor with its own leading dimension) is the same call."""
import ctypes as C

import numpy as np
import pytest

import dk_cases as DK
import solve_lines_ref as LR
import solve_ref as R
from test_op_padded_dev import MAXITER, RTOL, SENTINEL, _pad, _rhs, _same, _System

pytestmark = pytest.mark.gpu

N0, K = 257, DK.K
NSTEPS, FIRST, DT = 4, 2, 2.0
Q = 3


@pytest.fixture(scope="module")
def system():
    from otmb_amd.device import DeviceAssembler

    P = _System(DeviceAssembler(0).ctx, N0, R.dominant(N0), None, 0.5, K, nxt=LR.random_lines(N0, 3))
    yield P
    P.O.close()


def _d_layouts():
    """(name, D as a device tensor view, ldd) x the host D: compact; ldd = n + 3 (even) and n + 4 (odd), NaN below row n; and a view that
    starts one double into a 256-byte aligned buffer: 8-byte, not 16-byte aligned."""
    import torch

    D = np.asfortranarray(np.random.default_rng(61).uniform(0.0, 1.0, (N0, K)) * np.array([1.0, 1e-3, 10.0, 0.0, 5.0, 0.3, 2.0]))
    out = [("compact", _pad(D, 0, np.nan), N0)]
    for pad in (3, 4):
        assert (N0 + pad) % 2 == (pad + 1) % 2
        out.append((f"ldd = n + {pad}", _pad(D, pad, np.nan), N0 + pad))
    ld = N0 + 5
    buf = torch.full((K * ld + 1,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].as_strided((N0, K), (1, ld))
    view.copy_(torch.from_numpy(np.ascontiguousarray(D.T)).cuda().t())
    assert view.data_ptr() % 16 == 8
    out.append(("misaligned", view, ld))
    return D, out


def _each_layout(call, what):
    """call(Dt, ldd) -> the call's outputs; every layout of D gives the compact call's bits and leaves D alone."""
    D, layouts = _d_layouts()
    first = None
    for name, Dt, ldd in layouts:
        before = Dt.clone()
        got = call(Dt, ldd)
        _same(Dt, before, (what, name, "D was written"))
        _same(Dt[:N0], D, (what, name, "D"))
        if first is None:
            first = got
        for a, b in zip(got, first):
            if hasattr(a, "cpu") or isinstance(a, np.ndarray) and a.dtype == np.float64:
                _same(a, b, (what, name))
            else:
                assert np.array_equal(a, b), (what, name, a, b)
    return D, first


@pytest.mark.parametrize("adjoint", [0, 1])
@pytest.mark.parametrize("pc", [0, 1], ids=["jacobi", "lines"])
def test_solve_and_precond_dk_dev(system, pc, adjoint):
    P = system
    B = _rhs(N0, K, seed=11)

    def call(Dt, ldd):
        Bp, Xp, Zp = _pad(B, 3, np.nan), _pad(np.full((N0, K), SENTINEL), 5, SENTINEL), _pad(np.full((N0, K), SENTINEL), 5, SENTINEL)
        it, rr, why = np.full(K, -7, np.int64), np.full(K, SENTINEL), np.full(K, -7, np.int32)
        rc = P.lib.otmb_op_solve_dk_dev(P.h, adjoint, K, Dt.data_ptr(), ldd, 0.5, Bp.data_ptr(), N0 + 3, Xp.data_ptr(), N0 + 5, 0, RTOL, MAXITER,
                                        it.ctypes.data, rr.ctypes.data, why.ctypes.data, pc)
        assert rc == 0 and (why == 0).all(), (rc, why)
        assert P.lib.otmb_op_precond_dk_dev(P.h, adjoint, pc, K, Dt.data_ptr(), ldd, 0.5, Bp.data_ptr(), N0 + 3, Zp.data_ptr(), N0 + 5) == 0
        _same(Xp[N0:], np.full((5, K), SENTINEL), "padding rows of X were written")
        _same(Zp[N0:], np.full((5, K), SENTINEL), "padding rows of Z were written")
        return Xp[:N0].clone(), Zp[:N0].clone(), it, rr, why

    D, (X, Z, it, rr, why) = _each_layout(call, ("solve", pc, adjoint))
    print("iterations", it.tolist())
    nxt = LR.random_lines(N0, 3)
    for c in range(K):  # the restatement and the float64 residual, per column with its own d
        want = LR.Lines(P.A, nxt, D[:, c], 0.5, bool(adjoint)).apply(B[:, c]) if pc else B[:, c] / R.jacobi_diagonal(P.A, D[:, c], 0.5)
        _same(Z[:, c], want, ("Z against the restatement", c))
        (res, bound), = R.residual_check(P.A, X[:, c:c + 1].cpu().numpy(), B[:, c:c + 1], D[:, c], 0.5, bool(adjoint), RTOL)
        assert res <= bound, (c, res, bound)
    # device.Operator: a 2-D d with its own leading dimension
    import torch

    Dt = _pad(D, 4, np.nan)[:N0]
    Xo, info = P.O.solve(torch.from_numpy(B.T.copy()).cuda().t(), d=Dt, sigma=0.5, rtol=RTOL, maxiter=MAXITER, adjoint=bool(adjoint),
                         precond="lines" if pc else "jacobi")
    _same(Xo, X, "device.Operator.solve")
    assert np.array_equal(info.iterations, it)
    _same(P.O.precondition(torch.from_numpy(B.T.copy()).cuda().t(), d=Dt, sigma=0.5, adjoint=bool(adjoint), precond="lines" if pc else "jacobi"), Z,
          "device.Operator.precondition")


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("pc,adjoint", [(0, 0), (1, 1), (1, 0)], ids=["jacobi-plain", "lines-adjoint", "lines-plain"])
def test_step_dk_dev(system, pc, adjoint, theta):
    """4 steps from slot 2 over the 3 slots with a source, observers and the mean; against the k = 1 otmb_op_step_obs_dev calls too."""
    import torch

    P = system
    X0, S0 = _rhs(N0, K, seed=31), np.asfortranarray(np.random.default_rng(32).standard_normal((N0, K)))
    W0 = np.asfortranarray(np.random.default_rng(34).uniform(0.0, 1.0, (N0, Q)))
    tw = np.random.default_rng(35).uniform(0.0, 1.0, NSTEPS)

    def run(k, dptr, ldd, X, S, name):
        Xp, Sp, Wp = _pad(X, 5, SENTINEL), _pad(S, 7, np.nan), _pad(W0, 1, np.nan)
        obs = torch.full((Q * k * NSTEPS,), SENTINEL, dtype=torch.float64, device="cuda")
        mean = _pad(np.full((N0, k), SENTINEL), 3, SENTINEL)
        it, rr, why = np.full((NSTEPS, k), -7, np.int64), np.full((NSTEPS, k), SENTINEL), np.full((NSTEPS, k), -7, np.int32)
        done = C.c_int64(-7)
        tail = (DT, float(theta), NSTEPS, FIRST, Sp.data_ptr(), N0 + 7, Xp.data_ptr(), N0 + 5, RTOL, MAXITER, pc, C.byref(done), it.ctypes.data,
                rr.ctypes.data, why.ctypes.data, Q, Wp.data_ptr(), N0 + 1, obs.data_ptr(), tw.ctypes.data, mean.data_ptr(), N0 + 3)
        rc = P.lib.otmb_op_step_dk_dev(P.h, adjoint, k, dptr, ldd, *tail) if name == "dk" else P.lib.otmb_op_step_obs_dev(P.h, adjoint, k, dptr, *tail)
        assert rc == 0 and done.value == NSTEPS, (name, rc, done.value)
        _same(Xp[N0:], np.full((5, k), SENTINEL), "padding rows of X were written")
        _same(mean[N0:], np.full((3, k), SENTINEL), "padding rows of the mean were written")
        return Xp[:N0].clone(), obs.clone().cpu().numpy().reshape(NSTEPS, k, Q), mean[:N0].clone(), it, rr, why

    D, (X, obs, mean, it, rr, why) = _each_layout(lambda Dt, ldd: run(K, Dt.data_ptr(), ldd, X0, S0, "dk"), ("step", pc, adjoint, theta))
    assert P.O.slots == (3, 0)
    for c in (0, 3, 6):  # a column of every register block, alone through the existing export
        dc = torch.from_numpy(np.ascontiguousarray(D[:, c])).cuda()
        x1, o1, m1, it1, rr1, why1 = run(1, dc.data_ptr(), None, X0[:, c:c + 1], S0[:, c:c + 1], "obs")
        _same(X[:, c:c + 1], x1, ("state", c))
        _same(obs[:, c], o1[:, 0], ("observations", c))
        _same(mean[:, c:c + 1], m1, ("mean", c))
        assert np.array_equal(it[:, c], it1[:, 0]) and np.array_equal(why[:, c], why1[:, 0]), c
        _same(rr[:, c], rr1[:, 0], ("relres", c))


def test_periodic_dk_dev(system):
    """outer = mean, lines, k = 7: every layout of D gives the compact call's bits, cycles, defect and mean-solve iterations."""
    P = system
    S0 = _rhs(N0, K, seed=41)

    def call(Dt, ldd):
        Sp, Xp = _pad(S0, 7, np.nan), _pad(np.full((N0, K), SENTINEL), 5, SENTINEL)
        cyc, dft, why, ms = np.full(K, -7, np.int64), np.full(K, SENTINEL), np.full(K, -7, np.int32), np.full(K, -7, np.int64)
        rc = P.lib.otmb_op_periodic_dk_dev(P.h, 0, K, Dt.data_ptr(), ldd, DT, 0.5, 4, FIRST, Sp.data_ptr(), N0 + 7, Xp.data_ptr(), N0 + 5, 0, 1e-12, MAXITER,
                                           1, 1e-8, 7, 200, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data, 1, ms.ctypes.data)
        assert rc == 0 and (why == 0).all(), (rc, why, cyc)
        _same(Xp[N0:], np.full((5, K), SENTINEL), "padding rows of X were written")
        return Xp[:N0].clone(), cyc, dft, ms

    _, (X, cyc, dft, ms) = _each_layout(call, "periodic")
    print("cycles", cyc.tolist(), "mean-solve iterations", ms.tolist())
    assert (dft <= 1e-8).all() and (ms > 0).all() and P.O.slots == (3, 0)
