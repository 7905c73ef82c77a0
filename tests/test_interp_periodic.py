"""GPU: otmb_op_periodic_interp (csrc/otmb_periodic.hip): the periodic state of a cycle of INTERPOLATED steps.  The call has THE BITS of the
restatement (tests/periodic_ref.py, tests/periodic_pc_ref.py, order="device") over this operator's own step_interp() as the cycle map
and, for outer="mean", an operator over the cycle-mean values with tests/interp_ref.py's mean weights, one column per call -- X, cycles,
defect, reasons and msolve_iters (the mean solves' iterations agree only when the device blended the slots with those weights); every
answer is judged by one more cycle; a zero source column is answered with zero and never stepped.  The cases, tolerances and iteration
limits are tests/interp_cases.py's, which tests/test_interp_ref.py shows to converge in the restatement alone; none is dropped here."""
import ctypes as C

import numpy as np
import pytest

import interp_cases as IC
import interp_ref as IR
import periodic_pc_ref as PC
import periodic_ref as PR
from test_step import _csc, _operator, _same_bits

pytestmark = pytest.mark.gpu

SCHED = dict(slot_a=IC.SCHEDULE[0], slot_b=IC.SCHEDULE[1], weight=IC.SCHEDULE[2])
NCYCLE = len(IC.SCHEDULE[2])


@pytest.fixture(scope="module")
def systems(oracle):
    """Per grid: the operator with the tests' three slots and the water columns, for the restated mean solve one over the mean values, and
    the case (N, the pattern and lines, the slots' values, D, S)."""
    import otmb_amd.api as api

    made = {}

    def get(name):
        if name not in made:
            N, (p, i, v, nxt), values, D3, S3 = IC.case(oracle, name)
            M = api.DeviceOperator(_csc(N, p, i, IR.mean_values(values, *IC.SCHEDULE)))
            M.set_lines(nxt)
            made[name] = (_operator(N, p, i, v, nxt=nxt), M)
        return made[name] + IC.case(oracle, name)

    yield get
    for D, M in made.values():
        D.close()
        M.close()


def _restated(D, M, S, d, *, theta, adjoint, outer):
    """The restatement in the device's order over D.step_interp (and M.solve), one column per call; S: n x k; d: n values or n x k."""
    S2 = S.reshape(len(S), -1)
    dcol = (lambda c: d) if d.ndim == 1 else (lambda c: np.ascontiguousarray(d[:, c]))

    def run(c, x, src):
        X, info = D.step_interp(x, dt=IC.DT, theta=theta, source=src, d=dcol(c), rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines", **SCHED)
        return X if info.status == 0 and info.steps_done == NCYCLE else None

    def qinv(c, v):
        q, info = M.solve(v, d=dcol(c), sigma=0.0, rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines")
        return (PC.precondition(v, q, float(NCYCLE) * IC.DT) if info.converged.all() else None), int(info.iterations[0])

    F, Phi = (lambda c, x: run(c, x, np.ascontiguousarray(S2[:, c]))), (lambda c, v: run(c, v, None))
    kw = dict(ptol=IC.PTOL, restart=IC.RESTART, maxcycles=IC.MAXCYCLES, order="device")
    if outer == "mean":
        return PC.periodic_pc_ref(F, Phi, qinv, S2, **kw)
    Xr, ref = PR.periodic_ref(F, Phi, S2, **kw)
    return Xr, dict(ref, msolve_iters=np.zeros(len(ref["cycles"]), dtype=np.int64))


@pytest.mark.parametrize("outer", ["none", "mean"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", IC.GRIDS)
def test_the_call_has_the_bits_of_the_restatement(systems, name, theta, adjoint, outer):
    """3 slots x 2 sub-steps by the convention (six blended steps, the wrap pair first and last), the water columns' preconditioner, δt = a
    month: k = 1 (the age system, s = 1) and k = 3 with a d per column, whose third source column is zero."""
    D, M, N, _, _, D3, S3 = systems(name)
    call = dict(dt=IC.DT, theta=theta, rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines", ptol=IC.PTOL, restart=IC.RESTART,
                maxcycles=IC.MAXCYCLES, outer=outer, **SCHED)
    for S, d in ((np.ascontiguousarray(S3[:, 0]), np.ascontiguousarray(D3[:, 0])), (S3, D3)):
        what = (name, theta, adjoint, outer, S.ndim)
        X, info = D.periodic_interp(S, d=d, **call)
        print(what, "cycles", info.cycles.tolist(), "msolve", info.msolve_iters.tolist(), "defect", info.defect.tolist(), info.reason)
        assert info.status == 0 and info.converged.all() and (info.defect <= IC.PTOL).all(), (what, info)
        Xr, ref = _restated(D, M, S, d, theta=theta, adjoint=adjoint, outer=outer)
        X2 = X.reshape(len(X), -1)
        assert np.array_equal(info.cycles, ref["cycles"]), (what, info.cycles, ref["cycles"])
        assert list(info.reason) == list(ref["reason"]), (what, info.reason, ref["reason"])
        assert np.array_equal(info.msolve_iters, ref["msolve_iters"]), (what, info.msolve_iters, ref["msolve_iters"])
        _same_bits(info.defect, ref["defect"], (what, "defect"))
        for c in range(X2.shape[1]):
            _same_bits(X2[:, c], Xr[:, c], (what, "X, column", c))
        assert (info.msolve_iters[:2] > 0).all() if outer == "mean" else not info.msolve_iters.any()
        if S.ndim == 2:  # the zero column: answered with zero, never stepped
            assert info.cycles[2] == 0 and not X[:, 2].any() and info.defect[2] == 0.0 and (info.cycles[:2] > 2).all()
        # judged by one more cycle from X and one from zero: ‖F(x) - x‖₂ <= ptol·‖g‖₂·(1 + 1e-6) per column
        step = dict(dt=IC.DT, theta=theta, source=S, d=d, rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines", **SCHED)
        FX, si = D.step_interp(X, **step)
        G, sg = D.step_interp(np.zeros_like(X), **step)
        assert si.steps_done == sg.steps_done == NCYCLE
        for c in range(X2.shape[1]):
            defect, g = np.linalg.norm(FX.reshape(X2.shape)[:, c] - X2[:, c]), np.linalg.norm(G.reshape(X2.shape)[:, c])
            assert defect <= IC.PTOL * g * (1 + 1e-6), (what, c, defect, g)
    assert D.slots == (3, 0)


def test_the_mean_weights_are_the_restatements(systems):
    """outer = "mean" on a schedule with plain and blended steps: the restated mean operator is built from interp_ref.mean_weights' fold
    (a plain step adds 1.0, a blended one 1.0 - w then w, acc / ncycle), and the call's X, cycles and msolve_iters are its bits."""
    import otmb_amd.api as api

    D, _, N, (p, i, v, nxt), values, D3, S3 = systems("odd_nx_fold")
    sched = (np.array([0, 0, 1, 2, 2]), np.array([0, 1, 2, 0, 1]), np.array([0.7, 1.0 / 3.0, 1.0, 0.5, 0.0]))
    wt = IR.mean_weights(3, *sched)
    assert np.array_equal(wt, np.array([(1.0 + (1.0 - 1.0 / 3.0) + 0.5) / 5.0, (1.0 / 3.0) / 5.0, (1.0 + 0.5 + 1.0) / 5.0]))
    s, d = np.ascontiguousarray(S3[:, 0]), np.ascontiguousarray(D3[:, 0])
    kw = dict(slot_a=sched[0], slot_b=sched[1], weight=sched[2])
    with api.DeviceOperator(_csc(N, p, i, PC.combine_ref(values, wt))) as M:
        M.set_lines(nxt)
        X, info = D.periodic_interp(s, dt=IC.DT, d=d, rtol=IC.RTOL, maxiter=IC.MAXITER, precond="lines", ptol=IC.PTOL, restart=IC.RESTART,
                                    maxcycles=IC.MAXCYCLES, outer="mean", **kw)
        assert info.status == 0 and info.converged.all()

        def run(c, x, src):
            Y, si = D.step_interp(x, dt=IC.DT, source=src, d=d, rtol=IC.RTOL, maxiter=IC.MAXITER, precond="lines", **kw)
            return Y if si.steps_done == 5 else None

        def qinv(c, vv):
            q, mi = M.solve(vv, d=d, sigma=0.0, rtol=IC.RTOL, maxiter=IC.MAXITER, precond="lines")
            return (PC.precondition(vv, q, 5.0 * IC.DT) if mi.converged.all() else None), int(mi.iterations[0])

        Xr, ref = PC.periodic_pc_ref(lambda c, x: run(c, x, s), lambda c, x: run(c, x, None), qinv, s.reshape(N, 1), ptol=IC.PTOL, restart=IC.RESTART,
                                     maxcycles=IC.MAXCYCLES, order="device")
        assert np.array_equal(info.cycles, ref["cycles"]) and np.array_equal(info.msolve_iters, ref["msolve_iters"]) and info.msolve_iters[0] > 0
        _same_bits(X, Xr[:, 0], "X with the restated mean weights")
        _same_bits(info.defect, ref["defect"], "defect")


def test_refusals_leave_x_untouched(systems):
    """otmb_op_periodic_interp through the C ABI: a null array, a slot and a weight out of range, two source blocks -- refused with the
    export's name before anything is written; the operator stays usable."""
    from otmb_amd import capi

    D, _, N, _, _, D3, S3 = systems("odd_nx_fold")
    S = np.asfortranarray(S3[:, :2])
    lib = capi.lib()

    def call(a, b, w, blocks, ncycle=3):
        X = np.full((N, 2), 7.25, order="F")
        cyc, dfc, why = np.full(2, -7, np.int64), np.full(2, 7.25), np.full(2, -7, np.int32)
        a, b = (None if x is None else np.ascontiguousarray(x, dtype=np.int64) for x in (a, b))
        w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        ptr = lambda x: None if x is None else x.ctypes.data
        arr = (C.c_void_p * len(blocks))(*[s.ctypes.data for s in blocks])
        rc = lib.otmb_op_periodic_interp(D.handle, 0, 2, None, 0, IC.DT, 1.0, ncycle, ptr(a), ptr(b), ptr(w), len(blocks), arr, N, X.ctypes.data, N, 0, IC.RTOL,
                                         IC.MAXITER, 1, IC.PTOL, IC.RESTART, IC.MAXCYCLES, cyc.ctypes.data, dfc.ctypes.data, why.ctypes.data, 1, None)
        return rc, X, cyc, lib.otmb_last_error(D.ctx.handle).decode()

    ok = ([2, 0, 0], [0, 0, 1], [0.5, 0.0, 0.25])
    for a, b, w, blocks, text in ((None, ok[1], ok[2], [S], "slot_a, slot_b or weight is null"), ([2, 0, 3], ok[1], ok[2], [S], "step 2: slot 3 is outside 0..2"),
                                  (ok[0], ok[1], [0.5, 0.0, -0.5], [S], "step 2: the weight -0.5 is not finite or outside [0, 1]"),
                                  (ok[0], ok[1], ok[2], [S, S, S], "nsrc must be 0 or 1")):
        rc, X, cyc, msg = call(a, b, w, blocks)
        assert rc == 11 and (X == 7.25).all() and (cyc == -7).all() and "otmb_op_periodic_interp: " + text in msg, (rc, msg)
    rc, X, cyc, msg = call(*ok, [S])
    assert rc == 0 and (cyc > 0).all() and D.slots == (3, 0), (rc, msg)
