"""CPU: what the Python layer (api.DeviceOperator) does with d before the library is called.  A 2-D d goes to the per-column exports
(otmb_op_*_dk) with D column-major and its leading dimension; a 1-D d, and none, keep calling the existing exports, so nothing about today's
calls moves; a 2-D d with 1-D X, or of another shape than X's, is a DimensionMismatch raised here.  The library is replaced by a recorder:
no device is needed, and no call below reaches one.  DeviceAssembler.solve, .step_tracers and .periodic_tracers hand d and every other
keyword to their operator unchanged."""
import ctypes as C
import re

import numpy as np
import pytest

N, K = 6, 3


class _Recorder:
    """Stands in for the loaded library: every export is a function that records (name, arguments) and returns OTMB_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("otmb_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 0


@pytest.fixture()
def op(monkeypatch):
    from otmb_amd import api, capi

    rec = _Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    D = api.DeviceOperator.__new__(api.DeviceOperator)  # (no context, no device: the methods under test only read these)
    D._h, D.shape = C.c_void_p(1), (N, N)
    D.ctx = type("Ctx", (), {"check": staticmethod(lambda rc: None)})()
    yield D, rec
    D._h = C.c_void_p()


def _calls(D, rec, d, X):
    """The exports the four families call with this d, in order: precondition, solve, step, step with observers, periodic, periodic(mean)."""
    del rec.calls[:]
    kw = dict(dt=1.0)
    D.precondition(X, d=d, precond="jacobi")
    D.solve(X, d=d)
    D.step(X, d=d, **kw)
    D.step(X, d=d, observe=np.ones(N), time_weights=np.ones(1), **kw)
    D.periodic(X, d=d, ncycle=2, **kw)
    D.periodic(X, d=d, ncycle=2, outer="mean", **kw)
    return [name for name, _ in rec.calls]


def test_a_one_dimensional_d_still_calls_the_existing_exports(op):
    D, rec = op
    old = ["otmb_op_precond", "otmb_op_solve_pc", "otmb_op_step", "otmb_op_step_obs", "otmb_op_periodic", "otmb_op_periodic_pc"]
    for X in (np.ones(N), np.ones((N, K), order="F")):
        assert _calls(D, rec, np.ones(N), X) == old
        assert _calls(D, rec, None, X) == old


def test_a_two_dimensional_d_calls_the_per_column_exports_with_its_leading_dimension(op):
    D, rec = op
    X = np.ones((N, K), order="F")
    big = np.asfortranarray(np.arange((N + 2) * K, dtype=np.float64).reshape(N + 2, K))
    for d, ldd, own in ((np.asfortranarray(np.arange(N * K, dtype=np.float64).reshape(N, K)), N, True), (big[:N], N + 2, True),
                        (np.arange(N * K, dtype=np.float64).reshape(N, K), N, False)):  # column-major; a row slice keeps its parent's; row-major is copied
        assert _calls(D, rec, d, X) == ["otmb_op_precond_dk", "otmb_op_solve_dk", "otmb_op_step_dk", "otmb_op_step_dk", "otmb_op_periodic_dk",
                                        "otmb_op_periodic_dk"]
        for (name, args), at in zip(rec.calls, (4, 3, 3, 3, 3, 3)):  # where D and ldd stand in the header's order
            assert args[at + 1] == ldd, (name, args[at + 1], ldd)
            if own:  # the pointer is the caller's array itself (a copy made for the call is gone by now)
                got = np.ctypeslib.as_array(C.cast(args[at], C.POINTER(C.c_double)), shape=(ldd * (K - 1) + N,))
                assert all(np.array_equal(got[c * ldd:c * ldd + N], d[:, c]) for c in range(K)), name
        assert [args[-2] for name, args in rec.calls if name == "otmb_op_periodic_dk"] == [0, 1]  # outer: none, mean


def test_shapes_are_refused_before_the_library_is_called(op):
    from otmb_amd import capi

    D, rec = op
    d2 = np.ones((N, K), order="F")
    for X, d in ((np.ones(N), d2), (np.ones((N, K)), np.ones((N, K + 1))), (np.ones((N, K)), np.ones((N + 1, K))), (np.ones((N, 1)), d2)):
        for call in (lambda: D.precondition(X, d=d), lambda: D.solve(X, d=d), lambda: D.step(X, d=d, dt=1.0),
                     lambda: D.step(X, d=d, dt=1.0, time_weights=np.ones(1)), lambda: D.periodic(X, d=d, dt=1.0, ncycle=2),
                     lambda: D.periodic(X, d=d, dt=1.0, ncycle=2, outer="mean")):
            del rec.calls[:]
            with pytest.raises(capi.OtmbError) as err:
                call()
            want = (r"DimensionMismatch: d of \(6, 3\) is per column, \w+ of \(6,\) has no columns" if X.ndim == 1 else
                    r"DimensionMismatch: d of \(%d, %d\), \w+ of \(%d, %d\)" % (d.shape + X.shape))
            assert err.value.status == 11 and re.fullmatch(want, str(err.value)), str(err.value)  # (the per-column refusals' own wording)
            assert rec.calls == []


def test_the_assembler_forwards_d_and_the_other_keywords_to_its_operator():
    """DeviceAssembler.solve / .step_tracers / .periodic_tracers are one-line forwards to device.Operator: a 2-D d, the observers, the weights
    and outer arrive as given (an operator that records stands in for the resident one)."""
    from otmb_amd.device import DeviceAssembler, OpRecord

    class _Op:
        handle = C.c_void_p(1)

        def __init__(self):
            self.calls = []

        def solve(self, B, **kw):
            self.calls.append(("solve", B, kw))

        def step(self, X, **kw):
            self.calls.append(("step", X, kw))

        def periodic(self, S, **kw):
            self.calls.append(("periodic", S, kw))

    asm, op = DeviceAssembler.__new__(DeviceAssembler), _Op()
    asm._init_state()
    asm._ops = {"T": OpRecord(op)}
    asm.operator = lambda matrix="T": op
    X, d, W, tw = np.ones((N, K)), np.full((N, K), 2.0), np.ones(N), np.ones(2)
    asm.solve("T", X, d=d, sigma=0.5, precond="lines")
    asm.step_tracers(X, d=d, dt=1.0, nsteps=2, observe=W, time_weights=tw)
    asm.periodic_tracers(X, d=d, dt=1.0, ncycle=2, outer="mean")
    (n0, a0, k0), (n1, a1, k1), (n2, a2, k2) = op.calls
    assert (n0, n1, n2) == ("solve", "step", "periodic") and a0 is X and a1 is X and a2 is X
    assert k0["d"] is d and k0["sigma"] == 0.5 and k0["precond"] == "lines"
    assert k1 == dict(d=d, dt=1.0, nsteps=2, observe=W, time_weights=tw) and k1["d"] is d
    assert k2 == dict(d=d, dt=1.0, ncycle=2, outer="mean") and k2["d"] is d
