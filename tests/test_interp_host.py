"""CPU: what the Python layer (operator_calls.OperatorCalls through api.DeviceOperator) does with an interpolated schedule before the library
is called.  step_interp and periodic_interp call otmb_op_step_interp / otmb_op_periodic_interp with slot_a, slot_b and weight marshalled as
Int64 / Int64 / Float64 host arrays in the header's order, nsteps / ncycle being their length; wrong lengths, dtypes, several source blocks
and weights outside [0, 1] are refused here; step, step_sched, periodic and periodic_sched still call what they called.  The library is
replaced by the recorder of tests/operator_calls_rec.py, which records any export by name: no device is needed."""
import ctypes as C
import re

import numpy as np
import pytest
from operator_calls_rec import K, N, has, host_operator, the_call

NSLOTS = 3


@pytest.fixture()
def op(monkeypatch):
    from otmb_amd import api

    D, rec = host_operator(monkeypatch)
    monkeypatch.setattr(api.DeviceOperator, "slots", property(lambda self: (NSLOTS, 0)))
    yield D, rec
    D._h = C.c_void_p()


def _names(rec):
    names = [n for n, _ in rec.calls]
    del rec.calls[:]
    return names


def _host(address, ctype, count):
    return np.ctypeslib.as_array(C.cast(address, C.POINTER(ctype)), shape=(count,)).copy()


def test_the_step_marshals_the_schedule_in_the_headers_order(op):
    D, rec = op
    X, d, S = np.ones((N, K), order="F"), np.arange(1.0, N + 1), np.asfortranarray(np.full((N, K), 2.0))
    a, b, w = np.array([2, 0, 0, 1]), np.array([0, 1, 1, 1]), np.array([0.75, 0.25, 1.0, 1.0 / 3.0])  # Int64, Int64, Float64: passed as they are
    scale = np.arange(1.0, 4 * K + 1).reshape(4, K)
    Xn, info = D.step_interp(X, dt=0.25, theta=0.5, slot_a=a, slot_b=b, weight=w, source=S, source_scale=scale, d=d, rtol=1e-7, maxiter=77, precond="lines")
    c = the_call(rec, "otmb_op_step_interp")
    has(c, adjoint=0, k=K, D=d.ctypes.data, ldd=0, dt=0.25, theta=0.5, nsteps=4, nsrc=1, lds=N, scale=scale.ctypes.data, X=Xn.ctypes.data, ldx=N, rtol=1e-7,
        maxiter=77, precond=1, q=0, W=None, obs=None, tw=None, Xbar=None)
    names = list(c)
    assert names[names.index("nsteps") + 1:names.index("nsrc")] == ["slot_a", "slot_b", "weight"] and "first_slot" not in c and "substeps" not in c
    has(c, slot_a=a.ctypes.data, slot_b=b.ctypes.data, weight=w.ctypes.data)
    assert np.array_equal(_host(c["slot_a"], C.c_int64, 4), a) and np.array_equal(_host(c["slot_b"], C.c_int64, 4), b)
    assert np.array_equal(_host(c["weight"], C.c_double, 4), w)
    assert isinstance(c["S"], C.Array) and [c["S"][0]] == [S.ctypes.data]
    assert info.iterations.shape == (1, K) and Xn.shape == (N, K)  # (steps_done = 0 from the recorder: the first row only)
    # lists and an Int32 array are converted (to arrays of the call's own: Int64 / Int64 / Float64 of the schedule's length)
    D.step_interp(X, dt=1.0, slot_a=[0, 1, 2], slot_b=np.array([1, 2, 0], dtype=np.int32), weight=[0, 1, 0.5])
    c = the_call(rec, "otmb_op_step_interp")
    has(c, nsteps=3)
    assert all(isinstance(c[key], int) and c[key] != 0 for key in ("slot_a", "slot_b", "weight"))
    # no source; a per-column d with its leading dimension; the record; a list of one block; an empty schedule
    big = np.asfortranarray(np.ones((N + 2, K)))
    tw = np.array([0.5, 0.5])
    _, info = D.step_interp(X, dt=1.0, slot_a=[0, 1], slot_b=[1, 1], weight=[0.5, 0.0], d=big[:N], observe=np.ones(N), time_weights=tw, adjoint=True)
    c = the_call(rec, "otmb_op_step_interp")
    has(c, adjoint=1, nsteps=2, nsrc=0, S=None, scale=None, D=big.ctypes.data, ldd=N + 2, q=1, ldw=N, precond=0)
    assert c["tw"] is not None and c["obs"] is not None and c["Xbar"] is not None
    D.step_interp(X, dt=1.0, slot_a=[0], slot_b=[1], weight=[0.5], source=[S])
    c = the_call(rec, "otmb_op_step_interp")
    has(c, nsteps=1, nsrc=1, lds=N)
    assert c["S"][0] == S.ctypes.data
    D.step_interp(np.ones(N), dt=1.0, slot_a=[], slot_b=[], weight=[])
    has(the_call(rec, "otmb_op_step_interp"), k=1, nsteps=0, nsrc=0)


def test_the_periodic_call_marshals_the_schedule(op):
    D, rec = op
    S, d = np.asfortranarray(np.full((N, K), 3.0)), np.arange(1.0, N + 1)
    a, b, w = np.array([2, 0, 0]), np.array([0, 1, 1]), np.array([0.75, 0.25, 0.75])
    X, info = D.periodic_interp(S, dt=0.25, slot_a=a, slot_b=b, weight=w, theta=0.5, d=d, x0=S, rtol=1e-7, maxiter=77, ptol=1e-5, restart=9, maxcycles=55,
                                outer="mean")
    c = the_call(rec, "otmb_op_periodic_interp")
    has(c, adjoint=0, k=K, D=d.ctypes.data, ldd=0, dt=0.25, theta=0.5, ncycle=3, nsrc=1, lds=N, X=X.ctypes.data, ldx=N, use_x0=1, rtol=1e-7, maxiter=77,
        precond=0, ptol=1e-5, restart=9, maxcycles=55, outer=1, msolve_iters=info.msolve_iters.ctypes.data)
    names = list(c)
    assert names[names.index("ncycle") + 1:names.index("nsrc")] == ["slot_a", "slot_b", "weight"] and "scale" not in c and "first_slot" not in c
    has(c, slot_a=a.ctypes.data, slot_b=b.ctypes.data, weight=w.ctypes.data)
    assert a.dtype == b.dtype == np.int64 and w.dtype == np.float64 and c["S"][0] == S.ctypes.data
    x = np.ones(N)
    D.periodic_interp([x], dt=1.0, slot_a=[0], slot_b=[0], weight=[0.0], adjoint=True, precond="lines")
    c = the_call(rec, "otmb_op_periodic_interp")
    has(c, adjoint=1, k=1, ncycle=1, nsrc=1, use_x0=0, outer=0, precond=1)
    assert c["S"][0] == x.ctypes.data


def test_the_schedule_is_refused_before_the_library_is_called(op):
    from otmb_amd import capi

    D, rec = op
    X = np.ones((N, K), order="F")
    ok = dict(dt=1.0, slot_a=[0, 1], slot_b=[1, 2], weight=[0.5, 0.25])
    refused = [
        (dict(ok, weight=[0.5]), r"DimensionMismatch: slot_a of \(2,\), slot_b of \(2,\), weight of \(1,\)"),
        (dict(ok, slot_b=[1, 2, 0]), r"DimensionMismatch: slot_a of \(2,\), slot_b of \(3,\), weight of \(2,\)"),
        (dict(ok, slot_a=[[0, 1]]), r"invalid argument: slot_a must be a 1-D array of integers"),
        (dict(ok, slot_a=[0.0, 1.0]), r"invalid argument: slot_a must be a 1-D array of integers, got float64"),
        (dict(ok, slot_b=np.array([True, False])), r"invalid argument: slot_b must be a 1-D array of integers, got bool"),
        (dict(ok, weight=[0.5 + 0j, 0.25]), r"invalid argument: weight must be a 1-D array of real numbers, got complex128"),
        (dict(ok, weight=["a", "b"]), r"invalid argument: weight must be a 1-D array of real numbers"),
        (dict(ok, slot_a=[0, 3]), r"invalid argument: slot_a holds a slot outside 0\.\.2"),
        (dict(ok, slot_b=[-1, 2]), r"invalid argument: slot_b holds a slot outside 0\.\.2"),
        (dict(ok, weight=[0.5, 1.5]), r"invalid argument: weight must be finite and in \[0, 1\]"),
        (dict(ok, weight=[-1e-300, 0.5]), r"invalid argument: weight must be finite and in \[0, 1\]"),
        (dict(ok, weight=[np.nan, 0.5]), r"invalid argument: weight must be finite and in \[0, 1\]"),
        (dict(ok, weight=[0.5, np.inf]), r"invalid argument: weight must be finite and in \[0, 1\]"),
    ]
    for kw, want in refused:
        for call in (lambda: D.step_interp(X, **kw), lambda: D.periodic_interp(X, **kw)):
            with pytest.raises(capi.OtmbError) as err:
                call()
            assert err.value.status == 11 and re.match(want, str(err.value)), str(err.value)
            assert rec.calls == []
    more = [
        (lambda: D.step_interp(X, source=[X, X, X], **ok), r"DimensionMismatch: 3 source blocks, expected 1 \(a source per slot is not built with interpolation\)"),
        (lambda: D.step_interp(X, source=[], **ok), r"DimensionMismatch: 0 source blocks, expected 1"),
        (lambda: D.periodic_interp([X, X, X], **ok), r"DimensionMismatch: 3 source blocks, expected 1"),
        (lambda: D.periodic_interp([], **ok), r"DimensionMismatch: 0 source blocks, expected 1"),
        (lambda: D.step_interp(X, source=np.ones((N, K + 1)), **ok), r"DimensionMismatch: source of \(6, 4\), X of \(6, 3\)"),
        (lambda: D.step_interp(X, source=X, source_scale=np.ones((3, K)), **ok), r"DimensionMismatch: source_scale of \(3, 3\), expected \(2, 3\)"),
        (lambda: D.step_interp(X, source_scale=np.ones((2, K)), **ok), r"invalid argument: source_scale needs a source"),
        (lambda: D.step_interp(X, time_weights=np.ones(3), **ok), r"DimensionMismatch: time_weights of \(3,\), expected \(2,\)"),
        (lambda: D.step_interp(np.ones((N + 1, K)), **ok), r"DimensionMismatch: operator of \(6, 6\), X of \(7, 3\)"),
        (lambda: D.step_interp(X, d=np.ones(N + 1), **ok), r"DimensionMismatch: d of \(7,\)"),
    ]
    for call, want in more:
        with pytest.raises(capi.OtmbError) as err:
            call()
        assert err.value.status == 11 and re.match(want, str(err.value)), str(err.value)
        assert rec.calls == []
    # the ends of the range are weights like any other
    D.step_interp(X, dt=1.0, slot_a=[0, 2], slot_b=[1, 0], weight=[0.0, 1.0])
    assert _names(rec) == ["otmb_op_step_interp"]


def test_the_other_calls_still_call_what_they_called(op):
    D, rec = op
    X, d2 = np.ones((N, K), order="F"), np.ones((N, K), order="F")
    D.step(X, dt=1.0)
    D.step(X, dt=1.0, source=X, observe=np.ones(N))
    D.step(X, dt=1.0, source=X, d=d2)
    D.step_sched(X, dt=1.0, substeps=2)
    D.step(X, dt=1.0, source=[X, X, X])
    assert _names(rec) == ["otmb_op_step", "otmb_op_step_obs", "otmb_op_step_dk", "otmb_op_step_sched", "otmb_op_step_sched"]
    D.periodic(X, dt=1.0, ncycle=2)
    D.periodic(X, dt=1.0, ncycle=2, outer="mean")
    D.periodic(X, dt=1.0, ncycle=2, d=d2)
    D.periodic_sched(X, dt=1.0, ncycle=2, substeps=4)
    D.periodic([X, X, X], dt=1.0, ncycle=2)
    assert _names(rec) == ["otmb_op_periodic", "otmb_op_periodic_pc", "otmb_op_periodic_dk", "otmb_op_periodic_sched", "otmb_op_periodic_sched"]


def test_the_assembler_forwards_the_interpolated_calls():
    from otmb_amd.device import DeviceAssembler, OpRecord

    class _Op:
        handle = C.c_void_p(1)

        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("step_interp", "periodic_interp"):
                raise AttributeError(name)
            return lambda A, **kw: self.calls.append((name, A, kw))

    asm, op = DeviceAssembler.__new__(DeviceAssembler), _Op()
    asm._init_state()
    asm._ops = {"T": OpRecord(op)}
    asm.operator = lambda matrix="T": op
    X, sched = np.ones((N, K)), dict(slot_a=[0], slot_b=[1], weight=[0.5])
    asm.step_tracers_interp(X, dt=1.0, source=X, **sched)
    asm.periodic_tracers_interp(X, dt=1.0, outer="mean", **sched)
    (n0, a0, k0), (n1, a1, k1) = op.calls
    assert (n0, n1) == ("step_interp", "periodic_interp") and a0 is X and a1 is X
    assert k0 == dict(dt=1.0, source=X, **sched) and k1 == dict(dt=1.0, outer="mean", **sched)
