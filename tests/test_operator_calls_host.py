"""CPU: what api.DeviceOperator hands the library for precondition, solve, observe, step and periodic (operator_calls.OperatorCalls over numpy
arrays).  The library is a recorder, so no device is needed: every call below must reach exactly one export -- the one the table in
OperatorCalls' methods chooses for this d and these keywords -- with as many arguments as the ctypes mirror declares, every scalar, leading
dimension and pointer at the place include/otmb.h gives it, the caller's own arrays where no copy is due and null where None was given."""
import ctypes as C
import inspect

import numpy as np
import pytest
from operator_calls_rec import CASE_IDS, CASES, K, N, PERIODIC, SIGNATURES, has, host_operator, only, the_call


@pytest.fixture()
def op(monkeypatch):
    D, rec = host_operator(monkeypatch)
    yield D, rec
    D._h = C.c_void_p()


def _f(rows, cols, start=1.0):
    return np.asfortranarray(np.arange(start, start + rows * cols, dtype=np.float64).reshape(rows, cols))


X1, X2 = np.arange(1.0, N + 1), _f(N, K)
PARENT = _f(N + 2, K, 100.0)  # row slices of it keep its leading dimension, N + 2
D_CASES = [("none", None), ("vector", np.arange(2.0, N + 2)), ("matrix", _f(N, K, 50.0)), ("slice", PARENT[:N])]
STATES = [(X, name, d) for X in (X1, X2) for name, d in D_CASES if X.ndim == 2 or np.ndim(d) < 2]  # (a matrix d needs columns)
IDS = [f"{X.ndim}D-{name}" for X, name, d in STATES]


def _d_part(a, d):
    """d's one or two places: the caller's own array (all four cases need no copy), and for a matrix its parent's leading dimension."""
    if np.ndim(d) == 2:
        has(a, D=d.ctypes.data, ldd=d.strides[1] // 8)
    else:
        has(a, d=None if d is None else d.ctypes.data)


def _state_part(a, B, X, state="B", ld="ldb"):
    """The input is the caller's array with its leading dimension, the result a new Fortran-ordered array of its shape with N."""
    k = 1 if B.ndim == 1 else K
    has(a, op=a["op"], k=k, **{state: B.ctypes.data, ld: N})
    assert a["op"].value == 1 and X.shape == B.shape and X.dtype == np.float64 and (X.ndim == 1 or X.flags.f_contiguous)
    return k


@pytest.mark.parametrize("scalars", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("X,name,d", STATES, ids=IDS)
def test_precondition_and_solve(op, X, name, d, scalars):
    D, rec = op
    given, sent = scalars
    keep = X.copy(), None if d is None else d.copy()
    Z = D.precondition(X, d=d, sigma=0.125, **only(given, "adjoint", "precond"))
    a = the_call(rec, "otmb_op_precond" + ("_dk" if np.ndim(d) == 2 else ""))
    _d_part(a, d)
    _state_part(a, X, Z, "Y", "ldy")
    has(a, sigma=0.125, Z=Z.ctypes.data, ldz=N, **only(sent, "adjoint", "precond"))
    for x0 in (None, 2.0 * X):
        Xs, info = D.solve(X, d=d, sigma=0.125, x0=x0, **only(given, "adjoint", "precond", "rtol", "maxiter"))
        a = the_call(rec, "otmb_op_solve" + ("_dk" if np.ndim(d) == 2 else "_pc"))
        _d_part(a, d)
        k = _state_part(a, X, Xs)
        has(a, sigma=0.125, X=Xs.ctypes.data, ldx=N, use_x0=int(x0 is not None), **only(sent, "adjoint", "precond", "rtol", "maxiter"))
        assert np.array_equal(Xs, np.zeros_like(X) if x0 is None else x0) and Xs is not x0  # the start, copied into the result
        assert info.status == 0 and info.iterations.shape == info.relres.shape == (k,) and len(info.reason) == k
        assert a["iters"] == info.iterations.ctypes.data and a["relres"] == info.relres.ctypes.data and D.ctx.checked.pop() == 0
    assert np.array_equal(X, keep[0]) and (d is None or np.array_equal(d, keep[1]))  # nothing of the caller's is written


@pytest.mark.parametrize("scalars", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("X,name,d", STATES, ids=IDS)
def test_step(op, X, name, d, scalars):
    D, rec = op
    SCALARS, SENT = scalars
    per_column = np.ndim(d) == 2
    S = {"none": None, "vector": 2.0 * X}.get(name, PARENT[1:N + 1])  # no source, one of X's layout, a misaligned row slice of a padded parent
    W2 = _f(N + 2, 2, 7.0)[:N]
    tw = np.array([0.25, 0.75])
    for observe, weights in ((None, None), (W2, None), (None, tw), (np.ones(N), tw)):
        keep = X.copy()
        Xn, info = D.step(X, nsteps=2, source=S, d=d, observe=observe, time_weights=weights, **SCALARS)
        record = per_column or observe is not None or weights is not None
        a = the_call(rec, "otmb_op_step" + ("_dk" if per_column else "_obs" if record else ""))
        _d_part(a, d)
        k = 1 if X.ndim == 1 else K
        has(a, k=k, nsteps=2, X=Xn.ctypes.data, ldx=N, **SENT)
        # the steps run on a copy of X: a new array of its shape with its values (the recorder steps nothing)
        assert Xn is not X and a["X"] != X.ctypes.data and np.array_equal(Xn, X) and np.array_equal(X, keep)
        assert Xn.shape == X.shape and (X.ndim == 1 or Xn.flags.f_contiguous)
        if S is None:
            has(a, S=None, lds=N)
        else:  # a row slice is passed where it lies, with its parent's leading dimension; a contiguous array with its own
            has(a, S=S.ctypes.data, lds=N + 2 if S.base is PARENT else N)
        if record:
            q = 0 if observe is None else 1 if observe.ndim == 1 else 2
            has(a, q=q, W=None if observe is None else observe.ctypes.data, ldw=N + 2 if observe is W2 else N, tw=None if weights is None else weights.ctypes.data,
                ldm=N)
            assert (a["obs"] is None) == (observe is None) and (a["Xbar"] is None) == (weights is None)
        assert info.status == 0 and info.steps_done == 0 and info.iterations.shape == (1, k)  # (the recorder completes no step)
        if observe is None and weights is None:
            assert info.observations is None and info.mean is None
        if observe is not None:
            assert info.observations.shape == (0, k, q) and info.observations.base is not None  # the completed steps of (nsteps, k, q)
        assert D.ctx.checked.pop() == 0 and D.ctx.checked == []


@pytest.mark.parametrize("X,name,d", STATES, ids=IDS)
@pytest.mark.parametrize("outer", ["none", "mean"])
@pytest.mark.parametrize("scalars", CASES, ids=CASE_IDS)
def test_periodic(op, scalars, outer, X, name, d):
    D, rec = op
    SCALARS, SENT = scalars
    per_column = np.ndim(d) == 2
    S = PARENT[1:N + 1] if (X.ndim == 2 and name == "none") else X  # (once as a misaligned row slice of a padded parent)
    for x0 in (None, 3.0 * X):
        keep = S.copy()
        Xp, info = D.periodic(S, d=d, x0=x0, outer=outer, **SCALARS, **PERIODIC)
        a = the_call(rec, "otmb_op_periodic" + ("_dk" if per_column else "_pc" if outer == "mean" else ""))
        _d_part(a, d)
        k = 1 if X.ndim == 1 else K
        has(a, k=k, S=S.ctypes.data, lds=N + 2 if S is not X else N, X=Xp.ctypes.data, ldx=N, use_x0=int(x0 is not None), **SENT, **PERIODIC)
        if per_column or outer == "mean":
            has(a, outer=int(outer == "mean"), msolve_iters=info.msolve_iters.ctypes.data)
        assert Xp.shape == X.shape and (X.ndim == 1 or Xp.flags.f_contiguous) and np.array_equal(Xp, np.zeros_like(X) if x0 is None else x0)
        assert np.array_equal(S, keep) and info.status == 0 and info.cycles.shape == (k,) and a["cycles"] == info.cycles.ctypes.data
        assert info.msolve_iters.shape == (k,) and not info.msolve_iters.any()
        assert D.ctx.checked.pop() == 0 and D.ctx.checked == []


@pytest.mark.parametrize("X", [X1, X2], ids=["1D", "2D"])
def test_observe(op, X):
    D, rec = op
    W2 = _f(N + 2, 2, 7.0)[:N]
    for W, q, ldw in ((np.ones(N), 1, N), (W2, 2, N + 2)):
        obs = D.observe(W, X)
        a = the_call(rec, "otmb_op_observe")
        k = 1 if X.ndim == 1 else K
        has(a, k=k, q=q, W=W.ctypes.data, ldw=ldw, X=X.ctypes.data, ldx=N)
        assert obs.shape == ((q,) if X.ndim == 1 else (q, k)) and a["obs"] == obs.ctypes.data and D.ctx.checked.pop() == 0


def test_an_input_that_needs_a_copy_is_copied_into_column_major_order(op):
    D, rec = op
    rows = np.arange(1.0, N * K + 1).reshape(N, K)  # row-major: the library reads columns
    D.solve(rows)
    a = the_call(rec, "otmb_op_solve_pc")
    assert a["B"] != rows.ctypes.data and a["ldb"] == N
    D.precondition(np.arange(N), d=np.arange(N))  # integers: converted
    a = the_call(rec, "otmb_op_precond")
    assert a["d"] is not None and a["ldy"] == N


def test_not_converged_is_reported_and_every_other_status_is_checked(monkeypatch):
    for rc in (19, 11):
        D, rec = host_operator(monkeypatch, rc)
        infos = [D.solve(X2)[1], D.solve(X2, d=X2)[1], D.step(X2, dt=1.0)[1], D.step(X2, dt=1.0, d=X2, time_weights=np.ones(1))[1],
                 D.periodic(X2, dt=1.0, ncycle=2)[1], D.periodic(X2, dt=1.0, ncycle=2, outer="mean")[1], D.periodic(X2, dt=1.0, ncycle=2, d=X2)[1]]
        assert len(rec.calls) == len(infos) and all(info.status == rc for info in infos)
        assert D.ctx.checked == ([] if rc == 19 else [11] * len(infos))  # 19 is an answer; the context raises for the others
        D.precondition(X2)
        D.observe(X1, X2)
        assert D.ctx.checked[-2:] == [rc, rc]  # (calls without a report have no such answer)
        D._h = C.c_void_p()


def test_unknown_keyword_values_and_a_closed_operator_are_refused_before_anything_is_called(op):
    from otmb_amd import capi

    D, rec = op
    for call in (lambda: D.precondition(X2, precond="ilu"), lambda: D.solve(X2, precond="ilu"), lambda: D.step(X2, dt=1.0, precond="ilu"),
                 lambda: D.periodic(X2, dt=1.0, ncycle=2, precond="ilu"), lambda: D.periodic(X2, dt=1.0, ncycle=2, outer="annual"),
                 lambda: D.periodic(np.ones((N + 1, K)), dt=1.0, ncycle=2, outer="annual"), lambda: D.solve(np.ones(N + 1), precond="ilu")):
        with pytest.raises(capi.OtmbError) as err:
            call()
        assert err.value.name == "INVALID_ARG" and err.value.status == 11 and rec.calls == []
    for call in (lambda: D.solve(np.ones(N + 1)), lambda: D.solve(X2, x0=X1), lambda: D.step(X2, dt=1.0, source=X1), lambda: D.observe(np.ones(N + 1), X2),
                 lambda: D.step(X2, dt=1.0, nsteps=2, time_weights=np.ones(3)), lambda: D.solve(X2, d=np.ones(N + 1))):
        with pytest.raises(capi.OtmbError, match="DimensionMismatch") as err:
            call()
        assert err.value.status == 11 and rec.calls == []
    D._h = C.c_void_p()
    for call in (lambda: D.precondition(X2), lambda: D.solve(X2), lambda: D.observe(X1, X2), lambda: D.step(X2, dt=1.0), lambda: D.periodic(X2, dt=1.0, ncycle=2)):
        with pytest.raises(ValueError, match="DeviceOperator is closed"):
            call()
    assert rec.calls == []


def test_both_classes_have_the_documented_signatures():
    from otmb_amd import api, device, operator_calls

    for name, want in SIGNATURES.items():
        for cls in (api.DeviceOperator, device.Operator):
            assert str(inspect.signature(getattr(cls, name))) == want, (cls.__name__, name)
            assert getattr(cls, name) is getattr(operator_calls.OperatorCalls, name)  # one implementation, no wrapper in between
    assert api.SolveInfo is operator_calls.SolveInfo and api.StepInfo is operator_calls.StepInfo and api.PeriodicInfo is operator_calls.PeriodicInfo
    assert api.observers is operator_calls.observers and api.time_weights is operator_calls.time_weights and api.step_arrays is operator_calls.step_arrays


def test_a_shape_refusal_names_its_argument_and_a_scalar_d_is_one_value(op, monkeypatch):
    from otmb_amd import capi

    D, rec = op
    bad = np.ones((N + 1, K))
    for what, call in (("Y", lambda: D.precondition(bad)), ("B", lambda: D.solve(bad)), ("X", lambda: D.step(bad, dt=1.0)),
                       ("source", lambda: D.periodic(bad, dt=1.0, ncycle=2))):
        with pytest.raises(capi.OtmbError, match=r"DimensionMismatch: operator of \(6, 6\), %s of \(7, 3\)" % what):
            call()
    with pytest.raises(capi.OtmbError, match=r"DimensionMismatch: d of \(1,\), expected \(6,\)"):
        D.solve(X2, d=2.0)
    assert rec.calls == []
    D.shape = (1, 1)  # the one operator whose d is one value
    D.solve(np.ones(1), d=2.0)
    assert the_call(rec, "otmb_op_solve_pc")["d"] is not None
