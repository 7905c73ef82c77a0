"""GPU (no kernel of the library runs): what device.Operator hands the library for precondition, solve, observe, step and periodic
(operator_calls.OperatorCalls over torch tensors).  The library is the recorder of tests/test_operator_calls_host.py: the `_dev` exports are
reached, column-major tensors and row slices of them are passed where they lie with their parent's leading dimension, results are new
column-major tensors, the reports' arrays are host memory, and a host tensor is refused before anything is called."""
import ctypes as C

import numpy as np
import pytest
from operator_calls_rec import CASE_IDS, CASES, K, N, PERIODIC, Ctx, Recorder, has, only, the_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def t():
    import torch

    def cm(rows, cols, start=1.0):  # column-major rows x cols
        return torch.arange(start, start + rows * cols, dtype=torch.float64, device="cuda:0").reshape(cols, rows).t()

    parent = cm(N + 2, K, 100.0)
    return dict(x=torch.arange(1.0, N + 1, dtype=torch.float64, device="cuda:0"), X=cm(N, K), parent=parent, low=parent[:N], mid=parent[1:N + 1],
                d=torch.arange(2.0, N + 2, dtype=torch.float64, device="cuda:0"), D=cm(N, K, 50.0), W=cm(N + 2, 2, 7.0)[:N], cm=cm)


@pytest.fixture()
def op():
    from otmb_amd import device

    O = device.Operator.__new__(device.Operator)  # (no context and no resident matrix: the methods under test only read these)
    O._h, O.shape, O.ctx, O.lib, O.device = C.c_void_p(1), (N, N), Ctx(), Recorder(), 0
    yield O, O.lib
    O._h = C.c_void_p()


def _result(X, like):
    assert tuple(X.shape) == tuple(like.shape) and X.is_cuda and X.stride() == ((1,) if like.dim() == 1 else (1, N)) and X.data_ptr() != like.data_ptr()


@pytest.mark.parametrize("scalars", CASES, ids=CASE_IDS)
def test_precondition_solve_and_observe_reach_the_dev_exports(op, t, scalars):
    O, rec = op
    given, sent = scalars
    for B, d, dk in ((t["x"], None, False), (t["X"], t["d"], False), (t["mid"], t["D"], True), (t["X"], t["low"], True)):
        k, ldb = (1 if B.dim() == 1 else K), (N + 2 if B is t["mid"] else N)
        Z = O.precondition(B, d=d, sigma=0.125, **only(given, "adjoint", "precond"))
        a = the_call(rec, "otmb_op_precond_dk_dev" if dk else "otmb_op_precond_dev")
        has(a, k=k, sigma=0.125, Y=B.data_ptr(), ldy=ldb, Z=Z.data_ptr(), ldz=N, **only(sent, "adjoint", "precond"))
        _result(Z, B)
        for x0 in (None, t["low"] if B.dim() == 2 else 2.0 * t["x"]):
            X, info = O.solve(B, d=d, sigma=0.125, x0=x0, **only(given, "adjoint", "precond", "rtol", "maxiter"))
            a = the_call(rec, "otmb_op_solve_dk_dev" if dk else "otmb_op_solve_pc_dev")
            has(a, k=k, sigma=0.125, B=B.data_ptr(), ldb=ldb, X=X.data_ptr(), ldx=N, use_x0=int(x0 is not None),
                **only(sent, "adjoint", "precond", "rtol", "maxiter"))
            if dk:
                has(a, D=d.data_ptr(), ldd=N + 2 if d is t["low"] else N)
            else:
                has(a, d=None if d is None else d.data_ptr())
            _result(X, B)
            assert np.array_equal(X.cpu().numpy(), np.zeros(tuple(B.shape)) if x0 is None else x0.cpu().numpy())
            # the reports are host arrays: the library writes them through host pointers
            assert a["iters"] == info.iterations.ctypes.data and a["relres"] == info.relres.ctypes.data and info.iterations.shape == (k,)
    for X in (t["x"], t["mid"]):
        for W, q, ldw in ((t["d"], 1, N), (t["W"], 2, N + 2)):
            obs = O.observe(W, X)
            a = the_call(rec, "otmb_op_observe_dev")
            k = 1 if X.dim() == 1 else K
            has(a, k=k, q=q, W=W.data_ptr(), ldw=ldw, X=X.data_ptr(), ldx=N if X.dim() == 1 else N + 2, obs=obs.data_ptr())
            assert obs.is_cuda and tuple(obs.shape) == ((q,) if X.dim() == 1 else (q, k)) and obs.stride(0) == 1


@pytest.mark.parametrize("scalars", CASES, ids=CASE_IDS)
def test_step_and_periodic_reach_the_dev_exports(op, t, scalars):
    O, rec = op
    SCALARS, SENT = scalars
    tw = np.array([0.25, 0.75])
    for X, d, dk in ((t["x"], None, False), (t["X"], t["d"], False), (t["X"], t["low"], True)):
        k = 1 if X.dim() == 1 else K
        S = t["mid"] if X.dim() == 2 else None
        for observe, weights in ((None, None), (t["W"], None), (None, tw), (t["d"], tw)):
            Xn, info = O.step(X, nsteps=2, source=S, d=d, observe=observe, time_weights=weights, **SCALARS)
            record = dk or observe is not None or weights is not None
            a = the_call(rec, "otmb_op_step_dk_dev" if dk else "otmb_op_step_obs_dev" if record else "otmb_op_step_dev")
            has(a, k=k, nsteps=2, X=Xn.data_ptr(), ldx=N, S=None if S is None else S.data_ptr(), lds=N if S is None else N + 2, **SENT)
            _result(Xn, X)
            assert np.array_equal(Xn.cpu().numpy(), X.cpu().numpy())  # the steps run on a copy of X
            if dk:
                has(a, D=d.data_ptr(), ldd=N + 2)
            if record:
                has(a, q=0 if observe is None else 1 if observe.dim() == 1 else 2, W=None if observe is None else observe.data_ptr(),
                    ldw=N + 2 if observe is t["W"] else N, tw=None if weights is None else weights.ctypes.data, ldm=N)
                assert (a["obs"] is None) == (observe is None) and (a["Xbar"] is None) == (weights is None)
            assert a["iters"] == info.iterations.ctypes.data and info.steps_done == 0 and info.mean is None
            assert (info.observations is None) == (observe is None) and (observe is None or info.observations.is_cuda)
        for outer in ("none", "mean"):
            src = t["mid"] if X.dim() == 2 else X
            Xp, info = O.periodic(src, d=d, x0=X, outer=outer, **SCALARS, **PERIODIC)
            a = the_call(rec, "otmb_op_periodic_dk_dev" if dk else "otmb_op_periodic_pc_dev" if outer == "mean" else "otmb_op_periodic_dev")
            has(a, k=k, S=src.data_ptr(), lds=N + 2 if X.dim() == 2 else N, X=Xp.data_ptr(), ldx=N, use_x0=1, **SENT, **PERIODIC)
            if dk or outer == "mean":
                has(a, outer=int(outer == "mean"), msolve_iters=info.msolve_iters.ctypes.data)
            _result(Xp, X)
            assert np.array_equal(Xp.cpu().numpy(), X.cpu().numpy()) and a["cycles"] == info.cycles.ctypes.data and not info.msolve_iters.any()
    assert set(O.ctx.checked) == {0}


def test_a_host_tensor_is_refused_before_anything_is_called(op, t):
    O, rec = op
    X, W = t["X"], t["W"]
    host = lambda a: a.cpu()
    calls = {"B": [lambda: O.solve(host(X)), lambda: O.precondition(host(X)), lambda: O.step(host(X), dt=1.0), lambda: O.periodic(host(X), dt=1.0, ncycle=2),
                   lambda: O.observe(W, host(X))],
             "x0": [lambda: O.solve(X, x0=host(X)), lambda: O.periodic(X, dt=1.0, ncycle=2, x0=host(X))],
             "source": [lambda: O.step(X, dt=1.0, source=host(X))],
             "d": [lambda f=f, d=d: f(X, d=host(d)) for d in (t["d"], t["D"])
                   for f in (O.solve, O.precondition, lambda B, d: O.step(B, dt=1.0, d=d), lambda B, d: O.periodic(B, dt=1.0, ncycle=2, d=d, outer="mean"))],
             "observe": [lambda: O.observe(host(W), X), lambda: O.step(X, dt=1.0, observe=host(W))]}
    names = {"B": r"(B|Y|X|source)"}
    for what, refused in calls.items():
        for call in refused:
            with pytest.raises(ValueError, match=names.get(what, what) + r" must be a tensor on cuda:0 \(got cpu\)"):
                call()
            assert rec.calls == [], what
