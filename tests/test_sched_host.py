"""CPU: what the Python layer (operator_calls.OperatorCalls through api.DeviceOperator) does with a schedule before the library is called.
step and periodic keep their signatures; with the defaults and a single array they -- and step_sched / periodic_sched -- call the exports
they always called.  A list of source blocks, substeps != 1 or a source_scale go to otmb_op_step_sched / otmb_op_periodic_sched with the
schedule marshalled in the header's order: substeps, nsrc, an array of the blocks' addresses (nothing is stacked), lds, and the scale
step-major.  Shapes are refused here.  The library is replaced by a recorder (tests/operator_calls_rec.py): no device is needed."""
import ctypes as C

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


def _blocks(n=NSLOTS, shape=(N, K)):
    return [np.asfortranarray(np.full(shape, float(j + 1))) for j in range(n)]


def _pointers(a, nsrc):
    assert isinstance(a["S"], C.Array) and len(a["S"]) == nsrc
    return [a["S"][j] for j in range(nsrc)]


def test_the_defaults_call_the_exports_they_always_called(op):
    D, rec = op
    X, d1, d2 = np.ones((N, K), order="F"), np.ones(N), np.ones((N, K), order="F")
    for step in (D.step, D.step_sched):
        step(X, dt=1.0)
        step(X, dt=1.0, source=X, d=d1, nsteps=2)
        step(X, dt=1.0, source=X, observe=np.ones(N))
        step(X, dt=1.0, source=X, d=d2)
        assert _names(rec) == ["otmb_op_step", "otmb_op_step", "otmb_op_step_obs", "otmb_op_step_dk"]
    for periodic in (D.periodic, D.periodic_sched):
        periodic(X, dt=1.0, ncycle=2)
        periodic(X, dt=1.0, ncycle=2, outer="mean")
        periodic(X, dt=1.0, ncycle=2, d=d2)
        assert _names(rec) == ["otmb_op_periodic", "otmb_op_periodic_pc", "otmb_op_periodic_dk"]
    D.step_sched(X, dt=1.0, substeps=1, source_scale=None)
    assert _names(rec) == ["otmb_op_step"]


def test_any_part_of_a_schedule_calls_the_scheduled_exports(op):
    D, rec = op
    X = np.ones((N, K), order="F")
    D.step(X, dt=1.0, source=[X])
    D.step(X, dt=1.0, source=tuple(_blocks()))
    D.step_sched(X, dt=1.0, substeps=2)
    D.step_sched(X, dt=1.0, source=X, source_scale=np.ones((1, K)))
    D.step_sched(X, dt=1.0, source=_blocks(), d=np.ones((N, K), order="F"), observe=np.ones(N), time_weights=np.ones(1))
    assert _names(rec) == ["otmb_op_step_sched"] * 5
    D.periodic(_blocks(), dt=1.0, ncycle=2)
    D.periodic([X], dt=1.0, ncycle=2, outer="mean")
    D.periodic_sched(X, dt=1.0, ncycle=2, substeps=4)
    assert _names(rec) == ["otmb_op_periodic_sched"] * 3


def test_the_step_marshals_the_schedule_in_the_headers_order(op):
    D, rec = op
    X, d = np.ones((N, K), order="F"), np.arange(1.0, N + 1)
    blocks = _blocks()
    scale = np.arange(1.0, 4 * K + 1).reshape(4, K)
    Xn, info = D.step_sched(X, dt=0.25, theta=0.5, nsteps=4, first_slot=2, substeps=3, source=blocks, source_scale=scale, d=d, rtol=1e-7, maxiter=77,
                            precond="lines")
    a = the_call(rec, "otmb_op_step_sched")
    has(a, adjoint=0, k=K, D=d.ctypes.data, ldd=0, dt=0.25, theta=0.5, nsteps=4, first_slot=2, substeps=3, nsrc=NSLOTS, lds=N, scale=scale.ctypes.data,
        X=Xn.ctypes.data, ldx=N, rtol=1e-7, maxiter=77, precond=1, q=0, W=None, obs=None, tw=None, Xbar=None)
    assert _pointers(a, NSLOTS) == [b.ctypes.data for b in blocks]  # the caller's own arrays: nothing is stacked or copied
    # the scale is step-major: entry t·k + c
    got = np.ctypeslib.as_array(C.cast(a["scale"], C.POINTER(C.c_double)), shape=(4 * K,))
    assert np.array_equal(got, [scale[t, c] for t in range(4) for c in range(K)])
    # one block, a per-column d with its leading dimension, no scale; a single array without a list is one block too
    big = np.asfortranarray(np.ones((N + 2, K)))
    D.step(X, dt=1.0, source=[blocks[1]], d=big[:N])
    a = the_call(rec, "otmb_op_step_sched")
    has(a, substeps=1, nsrc=1, lds=N, scale=None, D=big.ctypes.data, ldd=N + 2)
    assert _pointers(a, 1) == [blocks[1].ctypes.data]
    D.step_sched(X, dt=1.0, source=blocks[2], substeps=2)
    a = the_call(rec, "otmb_op_step_sched")
    has(a, substeps=2, nsrc=1, lds=N, D=None, ldd=0)
    assert _pointers(a, 1) == [blocks[2].ctypes.data]
    # no source: nsrc = 0 and a null array
    D.step_sched(X, dt=1.0, substeps=2)
    has(the_call(rec, "otmb_op_step_sched"), substeps=2, nsrc=0, S=None, scale=None)
    # blocks that share a padded leading dimension keep it; blocks that differ are copied compactly
    pads = [np.asfortranarray(np.full((N + 2, K), float(j)))[:N] for j in range(NSLOTS)]
    D.step(X, dt=1.0, source=pads)
    a = the_call(rec, "otmb_op_step_sched")
    has(a, nsrc=NSLOTS, lds=N + 2)
    assert _pointers(a, NSLOTS) == [b.ctypes.data for b in pads]
    D.step(X, dt=1.0, source=[pads[0], blocks[1], np.ones((N, K))])  # a padded, a compact and a row-major block
    a = the_call(rec, "otmb_op_step_sched")
    has(a, nsrc=NSLOTS, lds=N)
    assert _pointers(a, NSLOTS)[1] == blocks[1].ctypes.data and _pointers(a, NSLOTS)[0] != pads[0].ctypes.data


def test_the_scale_of_a_one_dimensional_state(op):
    D, rec = op
    x, hist = np.ones(N), np.array([0.5, 0.0, -2.0])
    Xn, info = D.step_sched(x, dt=1.0, nsteps=3, source=[x], source_scale=hist)
    a = the_call(rec, "otmb_op_step_sched")
    has(a, k=1, nsteps=3, nsrc=1, lds=N, scale=hist.ctypes.data)
    assert Xn.shape == (N,) and _pointers(a, 1) == [x.ctypes.data]


def test_the_periodic_call_marshals_the_schedule(op):
    D, rec = op
    blocks, d = _blocks(), np.arange(1.0, N + 1)
    X, info = D.periodic_sched(blocks, dt=0.25, ncycle=6, theta=0.5, first_slot=2, substeps=2, d=d, x0=blocks[0], rtol=1e-7, maxiter=77, ptol=1e-5,
                               restart=9, maxcycles=55, outer="mean")
    a = the_call(rec, "otmb_op_periodic_sched")
    has(a, adjoint=0, k=K, D=d.ctypes.data, ldd=0, dt=0.25, theta=0.5, ncycle=6, first_slot=2, substeps=2, nsrc=NSLOTS, lds=N, X=X.ctypes.data, ldx=N,
        use_x0=1, rtol=1e-7, maxiter=77, precond=0, ptol=1e-5, restart=9, maxcycles=55, outer=1, msolve_iters=info.msolve_iters.ctypes.data)
    assert _pointers(a, NSLOTS) == [b.ctypes.data for b in blocks] and "scale" not in a
    assert np.array_equal(X, blocks[0]) and X.shape == (N, K)
    x = np.ones(N)
    D.periodic([x], dt=1.0, ncycle=2)
    a = the_call(rec, "otmb_op_periodic_sched")
    has(a, k=1, substeps=1, nsrc=1, lds=N, use_x0=0, outer=0)
    assert _pointers(a, 1) == [x.ctypes.data]


def test_shapes_are_refused_before_the_library_is_called(op):
    from otmb_amd import capi

    D, rec = op
    X = np.ones((N, K), order="F")
    refused = [
        (lambda: D.step(X, dt=1.0, source=_blocks(2)), r"DimensionMismatch: 2 source blocks, expected 1 or one per slot \(3\)"),
        (lambda: D.step(X, dt=1.0, source=[]), r"DimensionMismatch: 0 source blocks, expected 1 or one per slot \(3\)"),
        (lambda: D.step_sched(X, dt=1.0, substeps=2, source=_blocks(4)), r"DimensionMismatch: 4 source blocks"),
        (lambda: D.step(X, dt=1.0, source=_blocks(2) + [np.ones((N, K + 1))]), r"DimensionMismatch: source of \(6, 4\), X of \(6, 3\)"),
        (lambda: D.step(X, dt=1.0, source=[np.ones(N)]), r"DimensionMismatch: source of \(6,\), X of \(6, 3\)"),
        (lambda: D.step_sched(X, dt=1.0, nsteps=2, source=X, source_scale=np.ones((3, K))), r"DimensionMismatch: source_scale of \(3, 3\), expected \(2, 3\)"),
        (lambda: D.step_sched(X, dt=1.0, nsteps=2, source=X, source_scale=np.ones(2)), r"DimensionMismatch: source_scale of \(2,\), expected \(2, 3\)"),
        (lambda: D.step_sched(np.ones(N), dt=1.0, nsteps=2, source=np.ones(N), source_scale=np.ones((2, 1))),
         r"DimensionMismatch: source_scale of \(2, 1\), expected \(2,\)"),
        (lambda: D.step_sched(X, dt=1.0, source_scale=np.ones((1, K))), r"invalid argument: source_scale needs a source"),
        (lambda: D.periodic(_blocks(2), dt=1.0, ncycle=2), r"DimensionMismatch: 2 source blocks, expected 1 or one per slot \(3\)"),
        (lambda: D.periodic([], dt=1.0, ncycle=2), r"DimensionMismatch: 0 source blocks"),
        (lambda: D.periodic_sched([X, X, np.ones((N + 1, K))], dt=1.0, ncycle=2, substeps=2), r"DimensionMismatch: source of \(7, 3\), source of \(6, 3\)"),
    ]
    import re

    for call, want in refused:
        with pytest.raises(capi.OtmbError) as err:
            call()
        assert err.value.status == 11 and re.match(want, str(err.value)), str(err.value)
        assert rec.calls == []


def test_the_assembler_forwards_a_list_of_sources_and_the_schedule():
    from otmb_amd.device import DeviceAssembler, OpRecord

    class _Op:
        handle = C.c_void_p(1)

        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            if name not in ("step", "periodic", "step_sched", "periodic_sched"):
                raise AttributeError(name)
            return lambda A, **kw: self.calls.append((name, A, kw))

    asm, op = DeviceAssembler.__new__(DeviceAssembler), _Op()
    asm._init_state()
    asm._ops = {"T": OpRecord(op)}
    asm.operator = lambda matrix="T": op
    X, blocks, hist = np.ones((N, K)), _blocks(), np.ones((2, K))
    asm.step_tracers(X, dt=1.0, nsteps=2, source=blocks)
    asm.periodic_tracers(blocks, dt=1.0, ncycle=2)
    asm.step_tracers_sched(X, dt=1.0, nsteps=2, substeps=2, source=blocks, source_scale=hist)
    asm.periodic_tracers_sched(blocks, dt=1.0, ncycle=2, substeps=2)
    (n0, a0, k0), (n1, a1, k1), (n2, a2, k2), (n3, a3, k3) = op.calls
    assert (n0, n1, n2, n3) == ("step", "periodic", "step_sched", "periodic_sched")
    assert a0 is X and k0["source"] is blocks and a1 is blocks and a2 is X and a3 is blocks
    assert k2 == dict(dt=1.0, nsteps=2, substeps=2, source=blocks, source_scale=hist) and k2["source_scale"] is hist
    assert k3 == dict(dt=1.0, ncycle=2, substeps=2)
