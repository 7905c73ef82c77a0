"""CPU: what the Python layer (operator_calls.OperatorCalls through api.DeviceOperator) does with the season calls before the library is
called.  step_season and periodic_season call otmb_op_step_season / otmb_op_periodic_season with d as `nd, D (an array of nd pointers), ldd`
and the source as `nsrc, S, lds` in the header's order: d and source may each be None, one array, or a list or tuple of one or nslots
arrays of one shape; blocks whose leading dimensions differ are copied compactly; wrong counts, shapes and schedules are refused here; the
existing methods still call what they called and still refuse a source per slot under interpolation.  The library is replaced by the
recorder of tests/operator_calls_rec.py: no device is needed."""
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


def test_the_step_marshals_d_and_the_source_as_lists_in_the_headers_order(op):
    D, rec = op
    X = np.ones((N, K), order="F")
    ds = [np.arange(1.0, N + 1) * f for f in (1.0, 0.5, 0.125)]
    Ss = [np.asfortranarray(np.full((N, K), f)) for f in (2.0, 3.0, 4.0)]
    a, b, w = np.array([2, 0, 0, 1]), np.array([0, 1, 1, 1]), np.array([0.75, 0.25, 1.0, 1.0 / 3.0])
    scale = np.arange(1.0, 4 * K + 1).reshape(4, K)
    Xn, info = D.step_season(X, dt=0.25, theta=0.5, slot_a=a, slot_b=b, weight=w, d=ds, source=Ss, source_scale=scale, rtol=1e-7, maxiter=77, precond="lines")
    c = the_call(rec, "otmb_op_step_season")
    has(c, adjoint=0, k=K, nd=3, ldd=0, dt=0.25, theta=0.5, nsteps=4, nsrc=3, lds=N, scale=scale.ctypes.data, X=Xn.ctypes.data, ldx=N, rtol=1e-7, maxiter=77,
        precond=1, q=0, W=None, obs=None, tw=None, Xbar=None)
    names = list(c)
    assert names[names.index("k") + 1:names.index("dt")] == ["nd", "D", "ldd"] and names[names.index("nsteps") + 1:names.index("nsrc")] == ["slot_a", "slot_b", "weight"]
    has(c, slot_a=a.ctypes.data, slot_b=b.ctypes.data, weight=w.ctypes.data)
    assert isinstance(c["D"], C.Array) and list(c["D"]) == [x.ctypes.data for x in ds]  # passed as they are: nothing is stacked
    assert isinstance(c["S"], C.Array) and list(c["S"]) == [x.ctypes.data for x in Ss]
    assert info.iterations.shape == (1, K) and Xn.shape == (N, K)
    # no d, no source
    D.step_season(X, dt=1.0, slot_a=[0], slot_b=[1], weight=[0.5])
    has(the_call(rec, "otmb_op_step_season"), nd=0, D=None, ldd=0, nsrc=0, S=None, nsteps=1)
    # one array each is a list of one; a tuple is a list
    D.step_season(X, dt=1.0, slot_a=[0], slot_b=[1], weight=[0.5], d=ds[0], source=Ss[0])
    c = the_call(rec, "otmb_op_step_season")
    has(c, nd=1, ldd=0, nsrc=1, lds=N)
    assert list(c["D"]) == [ds[0].ctypes.data] and list(c["S"]) == [Ss[0].ctypes.data]
    D.step_season(X, dt=1.0, slot_a=[0], slot_b=[1], weight=[0.5], d=(ds[1],), source=(Ss[1],))
    c = the_call(rec, "otmb_op_step_season")
    assert (c["nd"], c["nsrc"]) == (1, 1) and list(c["D"]) == [ds[1].ctypes.data] and list(c["S"]) == [Ss[1].ctypes.data]
    # a d per column and per slot: blocks of X's shape with their common leading dimension ...
    big = [np.asfortranarray(np.full((N + 2, K), f)) for f in (1.0, 2.0, 3.0)]
    D.step_season(X, dt=1.0, slot_a=[0], slot_b=[1], weight=[0.5], d=[x[:N] for x in big], adjoint=True, observe=np.ones(N), time_weights=[1.0])
    c = the_call(rec, "otmb_op_step_season")
    has(c, adjoint=1, nd=3, ldd=N + 2, q=1, ldw=N)
    assert list(c["D"]) == [x.ctypes.data for x in big] and c["tw"] is not None and c["obs"] is not None and c["Xbar"] is not None
    # ... and blocks whose leading dimensions differ are copied compactly: one ldd for all
    mixed = [big[0][:N], np.asfortranarray(np.full((N, K), 5.0)), big[2][:N]]
    D.step_season(X, dt=1.0, slot_a=[0], slot_b=[1], weight=[0.5], d=mixed, source=[big[0][:N], Ss[1], Ss[2]])
    c = the_call(rec, "otmb_op_step_season")
    has(c, nd=3, ldd=N, nsrc=3, lds=N)
    assert c["D"][1] == mixed[1].ctypes.data and c["D"][0] != big[0].ctypes.data and c["S"][1] == Ss[1].ctypes.data and c["S"][0] != big[0].ctypes.data
    # a 1-D state: n values per block
    D.step_season(np.ones(N), dt=1.0, slot_a=[], slot_b=[], weight=[], d=ds, source=[np.ones(N)] * 3)
    has(the_call(rec, "otmb_op_step_season"), k=1, nsteps=0, nd=3, ldd=0, nsrc=3)


def test_the_periodic_call_marshals_the_lists(op):
    D, rec = op
    Ss = [np.asfortranarray(np.full((N, K), f)) for f in (2.0, 3.0, 4.0)]
    Ds = [np.asfortranarray(np.full((N, K), f)) for f in (1.0, 0.5, 0.125)]
    a, b, w = np.array([2, 0, 0]), np.array([0, 1, 1]), np.array([0.75, 0.25, 0.75])
    X, info = D.periodic_season(Ss, dt=0.25, slot_a=a, slot_b=b, weight=w, theta=0.5, d=Ds, x0=Ss[0], rtol=1e-7, maxiter=77, ptol=1e-5, restart=9, maxcycles=55,
                                outer="mean")
    c = the_call(rec, "otmb_op_periodic_season")
    has(c, adjoint=0, k=K, nd=3, ldd=N, dt=0.25, theta=0.5, ncycle=3, nsrc=3, lds=N, X=X.ctypes.data, ldx=N, use_x0=1, rtol=1e-7, maxiter=77, precond=0,
        ptol=1e-5, restart=9, maxcycles=55, outer=1, msolve_iters=info.msolve_iters.ctypes.data)
    names = list(c)
    assert names[names.index("k") + 1:names.index("dt")] == ["nd", "D", "ldd"] and "scale" not in c and "first_slot" not in c
    assert list(c["D"]) == [x.ctypes.data for x in Ds] and list(c["S"]) == [x.ctypes.data for x in Ss]
    has(c, slot_a=a.ctypes.data, slot_b=b.ctypes.data, weight=w.ctypes.data)
    x = np.ones(N)
    D.periodic_season(x, dt=1.0, slot_a=[0], slot_b=[0], weight=[0.0], d=x, adjoint=True, precond="lines")
    c = the_call(rec, "otmb_op_periodic_season")
    has(c, adjoint=1, k=1, ncycle=1, nd=1, ldd=0, nsrc=1, use_x0=0, outer=0, precond=1)
    assert c["S"][0] == x.ctypes.data and c["D"][0] == x.ctypes.data
    D.periodic_season([x], dt=1.0, slot_a=[0], slot_b=[0], weight=[0.0])
    has(the_call(rec, "otmb_op_periodic_season"), nd=0, D=None, nsrc=1)


def test_refusals_are_raised_before_the_library_is_called(op):
    from otmb_amd import capi

    D, rec = op
    X, d = np.ones((N, K), order="F"), np.ones(N)
    ok = dict(dt=1.0, slot_a=[0, 1], slot_b=[1, 2], weight=[0.5, 0.25])
    both = [
        (dict(d=[d, d]), r"DimensionMismatch: 2 d blocks, expected 1 or one per slot \(3\)"),
        (dict(d=[]), r"DimensionMismatch: 0 d blocks, expected 1 or one per slot \(3\)"),
        (dict(d=[d] * 4), r"DimensionMismatch: 4 d blocks, expected 1 or one per slot \(3\)"),
        (dict(d=[d, d, np.ones((N, K))]), r"DimensionMismatch: d blocks of different shapes"),
        (dict(d=[np.ones(N + 1)] * 3), r"DimensionMismatch: d of \(7,\), expected \(6,\)"),
        (dict(d=np.ones((N, K + 1))), r"DimensionMismatch: d of \(6, 4\)"),
        (dict(ok, weight=[0.5]), r"DimensionMismatch: slot_a of \(2,\), slot_b of \(2,\), weight of \(1,\)"),
        (dict(ok, slot_a=[0, 3]), r"invalid argument: slot_a holds a slot outside 0\.\.2"),
        (dict(ok, weight=[0.5, 1.5]), r"invalid argument: weight must be finite and in \[0, 1\]"),
        (dict(ok, slot_b=[1.0, 2.0]), r"invalid argument: slot_b must be a 1-D array of integers, got float64"),
    ]
    for kw, want in both:
        kw = dict(ok, **kw)
        for call in (lambda: D.step_season(X, **kw), lambda: D.periodic_season(X, **kw)):
            with pytest.raises(capi.OtmbError) as err:
                call()
            assert err.value.status == 11 and re.match(want, str(err.value)), str(err.value)
            assert rec.calls == []
    more = [
        (lambda: D.step_season(X, source=[X, X], **ok), r"DimensionMismatch: 2 source blocks, expected 1 or one per slot \(3\)"),
        (lambda: D.step_season(X, source=[], **ok), r"DimensionMismatch: 0 source blocks, expected 1 or one per slot"),
        (lambda: D.periodic_season([X, X], **ok), r"DimensionMismatch: 2 source blocks, expected 1 or one per slot \(3\)"),
        (lambda: D.periodic_season([], **ok), r"DimensionMismatch: 0 source blocks, expected 1 or one per slot"),
        (lambda: D.step_season(X, source=[X, X, np.ones((N, K + 1))], **ok), r"DimensionMismatch: source of \(6, 4\), X of \(6, 3\)"),
        (lambda: D.step_season(X, source=X, source_scale=np.ones((3, K)), **ok), r"DimensionMismatch: source_scale of \(3, 3\), expected \(2, 3\)"),
        (lambda: D.step_season(X, source_scale=np.ones((2, K)), **ok), r"invalid argument: source_scale needs a source"),
        (lambda: D.step_season(X, time_weights=np.ones(3), **ok), r"DimensionMismatch: time_weights of \(3,\), expected \(2,\)"),
        (lambda: D.step_season(np.ones((N + 1, K)), **ok), r"DimensionMismatch: operator of \(6, 6\), X of \(7, 3\)"),
        (lambda: D.step_season(np.ones(N), d=[np.ones((N, K))] * 3, **ok), r"DimensionMismatch: d of \(6, 3\) is per column, X of \(6,\) has no columns"),
    ]
    for call, want in more:
        with pytest.raises(capi.OtmbError) as err:
            call()
        assert err.value.status == 11 and re.match(want, str(err.value)), str(err.value)
        assert rec.calls == []
    D.step_season(X, d=[d, d, d], source=[X, X, X], **ok)
    assert _names(rec) == ["otmb_op_step_season"]


def test_the_existing_methods_call_and_refuse_what_they_did(op):
    from otmb_amd import capi

    D, rec = op
    X, d2 = np.ones((N, K), order="F"), np.ones((N, K), order="F")
    sched = dict(dt=1.0, slot_a=[0, 1], slot_b=[1, 2], weight=[0.5, 0.25])
    D.step(X, dt=1.0)
    D.step(X, dt=1.0, source=X, d=d2)
    D.step_sched(X, dt=1.0, substeps=2)
    D.step(X, dt=1.0, source=[X, X, X])
    D.step_interp(X, source=X, d=d2, **sched)
    assert _names(rec) == ["otmb_op_step", "otmb_op_step_dk", "otmb_op_step_sched", "otmb_op_step_sched", "otmb_op_step_interp"]
    D.periodic(X, dt=1.0, ncycle=2)
    D.periodic(X, dt=1.0, ncycle=2, d=d2)
    D.periodic([X, X, X], dt=1.0, ncycle=2)
    D.periodic_interp(X, **sched)
    assert _names(rec) == ["otmb_op_periodic", "otmb_op_periodic_dk", "otmb_op_periodic_sched", "otmb_op_periodic_interp"]
    for call in (lambda: D.step_interp(X, source=[X, X, X], **sched), lambda: D.periodic_interp([X, X, X], **sched)):
        with pytest.raises(capi.OtmbError) as err:
            call()
        assert "3 source blocks, expected 1 (a source per slot is not built with interpolation)" in str(err.value) and rec.calls == []
    for call in (lambda: D.step_interp(X, d=[d2, d2, d2], **sched), lambda: D.step_sched(X, dt=1.0, d=[d2, d2, d2])):  # d as a list is the season calls' alone
        with pytest.raises(Exception):
            call()
        assert rec.calls == []


def test_the_assembler_forwards_the_season_calls():
    from otmb_amd.device import DeviceAssembler, OpRecord

    class _Op:
        handle = C.c_void_p(1)

        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("step_season", "periodic_season"):
                raise AttributeError(name)
            return lambda A, **kw: self.calls.append((name, A, kw))

    asm, op = DeviceAssembler.__new__(DeviceAssembler), _Op()
    asm._init_state()
    asm._ops = {"T": OpRecord(op)}
    asm.operator = lambda matrix="T": op
    X, sched = np.ones((N, K)), dict(slot_a=[0], slot_b=[1], weight=[0.5])
    asm.step_tracers_season(X, dt=1.0, source=[X], d=[X], **sched)
    asm.periodic_tracers_season([X], dt=1.0, outer="mean", **sched)
    (n0, a0, k0), (n1, a1, k1) = op.calls
    assert (n0, n1) == ("step_season", "periodic_season") and a0 is X and a1[0] is X
    assert set(k0) == {"dt", "source", "d", "slot_a", "slot_b", "weight"} and k1 == dict(dt=1.0, outer="mean", **sched)
