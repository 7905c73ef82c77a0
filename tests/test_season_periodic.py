"""GPU: otmb_op_periodic_season (csrc/otmb_periodic.hip): the periodic state of a cycle whose matrix, d and source follow the slots.  The call
has THE BITS of the restatement (tests/periodic_ref.py, tests/periodic_pc_ref.py, order="device") over this operator's own step_season() as
the cycle map and, for outer="mean", over solve() on an operator that holds combine_slots' mean of the values, with d̄ from the stated fold
(tests/season_ref.py: dbar), one column per call -- X, cycles, defect, reasons and msolve_iters (the mean solves' iterations agree only when
the device folded the d blocks with those weights); the column that is zero in every source block is answered at no cycle.  The cases are
tests/season_cases.py's, which tests/test_season_ref.py shows to converge in the restatement alone; none is dropped here.  A 24-slot
operator takes d̄'s terms through the device table."""
import numpy as np
import pytest

import interp_cases as IC
import interp_ref as IR
import periodic_pc_ref as PC
import periodic_ref as PR
import sched_ref as SC
import season_cases as SE
import season_ref as SN
from test_step import _csc, _operator, _same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def systems(oracle):
    """Per grid: the operator with the tests' three slots and the water columns, and the case (N, the pattern and lines, the slots' values,
    the D blocks, the S blocks)."""
    made = {}

    def get(name):
        if name not in made:
            N, (p, i, v, nxt), values, Ds, Ss = SE.case(oracle, name)
            made[name] = _operator(N, p, i, v, nxt=nxt)
        return (made[name],) + SE.case(oracle, name)

    yield get
    for D in made.values():
        D.close()


def _restated(D, M, sources, d, sched, *, theta, adjoint, outer, dt=IC.DT):
    """The restatement in the device's order over D.step_season (and M.solve with d̄), one column per call; sources, d: lists of blocks, n
    values or n x k each."""
    n = len(sources[0])
    ncycle = len(sched[2])
    kw = dict(slot_a=sched[0], slot_b=sched[1], weight=sched[2])
    dm = SN.dbar(d, *sched)

    def run(c, x, src):
        X, info = D.step_season(x, dt=dt, theta=theta, source=src, d=SN.column(d, c), rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines", **kw)
        return X if info.status == 0 and info.steps_done == ncycle else None

    def qinv(c, v):
        q, info = M.solve(v, d=SN.column([dm], c)[0], sigma=0.0, rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines")
        return (PC.precondition(v, q, float(ncycle) * dt) if info.converged.all() else None), int(info.iterations[0])

    F, Phi = (lambda c, x: run(c, x, SN.column([S.reshape(n, -1) for S in sources], c))), (lambda c, v: run(c, v, None))
    lim = dict(ptol=IC.PTOL, restart=IC.RESTART, maxcycles=IC.MAXCYCLES, order="device")
    zero = SC.all_blocks([S.reshape(n, -1) for S in sources])
    if outer == "mean":
        return PC.periodic_pc_ref(F, Phi, qinv, zero, **lim)
    Xr, ref = PR.periodic_ref(F, Phi, zero, **lim)
    return Xr, dict(ref, msolve_iters=np.zeros(len(ref["cycles"]), dtype=np.int64))


def _same_as_restated(what, X, info, Xr, ref, outer, k):
    X2 = X.reshape(len(X), -1)
    assert np.array_equal(info.cycles, ref["cycles"]), (what, info.cycles, ref["cycles"])
    assert list(info.reason) == list(ref["reason"]), (what, info.reason, ref["reason"])
    assert np.array_equal(info.msolve_iters, ref["msolve_iters"]), (what, info.msolve_iters, ref["msolve_iters"])
    _same_bits(info.defect, ref["defect"], (what, "defect"))
    for c in range(X2.shape[1]):
        _same_bits(X2[:, c], Xr[:, c], (what, "X, column", c))
    assert (info.msolve_iters[:2] > 0).all() if outer == "mean" else not info.msolve_iters.any()
    if k == 3:  # the column that is zero in every block: answered with zero, never stepped
        assert info.cycles[2] == 0 and not X2[:, 2].any() and info.defect[2] == 0.0 and (info.cycles[:2] > 2).all()


@pytest.mark.parametrize("sched", sorted(SE.SCHEDULES))
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("name,theta,outer", SE.CASES)
def test_the_call_has_the_bits_of_the_restatement(systems, name, theta, outer, adjoint, sched):
    """Three slots with D_s = D·(1, 0.5, 0.125) and S_s = S·(1, 0.5, 1.5), the convention's six blended steps and the plain 3 x 2 schedule,
    the water columns' preconditioner, δt = a month: k = 3 with a D per column and per slot (its gathered columns travel with every step
    call), whose third source column is zero in every block, and column 0 alone with n values of d per slot."""
    import otmb_amd.api as api

    D, N, (p, i, v, nxt), values, Ds, Ss = systems(name)
    schedule = SE.SCHEDULES[sched]
    call = dict(dt=IC.DT, theta=theta, rtol=IC.RTOL, maxiter=IC.MAXITER, adjoint=adjoint, precond="lines", ptol=IC.PTOL, restart=IC.RESTART,
                maxcycles=IC.MAXCYCLES, outer=outer, slot_a=schedule[0], slot_b=schedule[1], weight=schedule[2])
    with api.DeviceOperator(_csc(N, p, i, IR.mean_values(values, *schedule))) as M:
        M.set_lines(nxt)
        for k in (3, 1):
            sources, d = SE.columns(Ss, k), SE.columns(Ds, k)
            what = (name, theta, adjoint, outer, sched, k)
            X, info = D.periodic_season(sources, d=d, **call)
            print(what, "cycles", info.cycles.tolist(), "msolve", info.msolve_iters.tolist(), "defect", info.defect.tolist(), info.reason)
            assert info.status == 0 and info.converged.all() and (info.defect <= IC.PTOL).all(), (what, info)
            Xr, ref = _restated(D, M, sources, d, schedule, theta=theta, adjoint=adjoint, outer=outer)
            _same_as_restated(what, X, info, Xr, ref, outer, k)
    # with one block of each the call is periodic_interp's, bit for bit
    s0, d0 = np.ascontiguousarray(Ss[1][:, 0]), np.ascontiguousarray(Ds[1][:, 0])
    X1, i1 = D.periodic_season([s0], d=[d0], **call)
    X2, i2 = D.periodic_interp(s0, d=d0, **call)
    _same_bits(X1, X2, "one block of each: periodic_interp")
    assert np.array_equal(i1.cycles, i2.cycles) and np.array_equal(i1.msolve_iters, i2.msolve_iters)
    assert D.slots == (3, 0)


def test_a_cycle_of_24_slots_takes_the_mean_d_through_the_table(oracle):
    """odd_nx_fold with 24 slots, each plain once (24 terms of 1/24: beyond the 16 that travel as kernel arguments), outer = "mean", k = 3
    with a D per column and per slot: X, cycles and msolve_iters are the restatement's with d̄ from the stated fold over 24 blocks."""
    import otmb_amd.api as api

    nslots = 24
    N, (p, i, v, nxt), _, D3, S3 = IC.case(oracle, "odd_nx_fold")
    rng = np.random.default_rng(24)
    values = [v * f for f in rng.uniform(0.5, 1.0, nslots)]
    Ds = [np.asfortranarray(D3 * f) for f in rng.uniform(0.1, 1.0, nslots)]
    Ss = [np.asfortranarray(S3 * f) for f in rng.uniform(0.5, 1.5, nslots)]
    sched = api.plain_schedule(nslots, nslots)
    wt = IR.mean_weights(nslots, *sched)
    assert (wt != 0.0).all() and len(wt) > 16
    dt = IC.DT / 2
    with api.DeviceOperator(_csc(N, p, i, v)) as D, api.DeviceOperator(_csc(N, p, i, PC.combine_ref(values, wt))) as M:
        D.set_slots(nslots)
        for s, vals in enumerate(values):
            D.set_values(vals, slot=s)
        D.set_lines(nxt)
        M.set_lines(nxt)
        X, info = D.periodic_season(Ss, d=Ds, dt=dt, slot_a=sched[0], slot_b=sched[1], weight=sched[2], rtol=IC.RTOL, maxiter=IC.MAXITER, precond="lines",
                                    ptol=IC.PTOL, restart=IC.RESTART, maxcycles=IC.MAXCYCLES, outer="mean")
        assert info.status == 0 and info.converged.all(), info
        Xr, ref = _restated(D, M, Ss, Ds, sched, theta=1.0, adjoint=False, outer="mean", dt=dt)
        _same_as_restated("24 slots", X, info, Xr, ref, "mean", 3)
        # a d̄ that were another fold would show in the mean solves: with slot 0's block alone they take other iterations
        _, other = D.periodic_season(Ss, d=Ds[:1], dt=dt, slot_a=sched[0], slot_b=sched[1], weight=sched[2], rtol=IC.RTOL, maxiter=IC.MAXITER,
                                     precond="lines", ptol=IC.PTOL, restart=IC.RESTART, maxcycles=IC.MAXCYCLES, outer="mean")
        assert other.converged.all() and D.slots == (nslots, 0)


def test_refusals_leave_x_untouched(systems):
    """otmb_op_periodic_season through the C ABI: two d blocks for three slots, a null block, a bad ldd, two source blocks, a weight out of
    range -- refused with the export's name before anything is written; the operator stays usable, a source per slot being in order."""
    import ctypes as C

    from otmb_amd import capi

    D, N, _, _, Ds, Ss = systems("odd_nx_fold")
    S = [np.asfortranarray(x[:, :2]) for x in Ss]
    Dk = [np.asfortranarray(x[:, :2]) for x in Ds]
    lib = capi.lib()

    def call(w, dblocks, ldd, sblocks):
        X = np.full((N, 2), 7.25, order="F")
        cyc, dfc, why = np.full(2, -7, np.int64), np.full(2, 7.25), np.full(2, -7, np.int32)
        a, b = np.array([2, 0, 0], dtype=np.int64), np.array([0, 0, 1], dtype=np.int64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        arr = lambda L: (C.c_void_p * max(len(L), 1))(*[None if s is None else s.ctypes.data for s in L])
        rc = lib.otmb_op_periodic_season(D.handle, 0, 2, len(dblocks), arr(dblocks), ldd, IC.DT, 1.0, 3, a.ctypes.data, b.ctypes.data, w.ctypes.data,
                                         len(sblocks), arr(sblocks), N, X.ctypes.data, N, 0, IC.RTOL, IC.MAXITER, 1, IC.PTOL, IC.RESTART, IC.MAXCYCLES,
                                         cyc.ctypes.data, dfc.ctypes.data, why.ctypes.data, 1, None)
        return rc, X, cyc, lib.otmb_last_error(D.ctx.handle).decode()

    ok = [0.5, 0.0, 0.25]
    for w, dblocks, ldd, sblocks, text in ((ok, Dk[:2], N, S, "nd must be 0, 1 or the number of slots"), (ok, [Dk[0], None, Dk[2]], N, S, "a d block is null"),
                                           (ok, Dk, N - 1, S, "ldd must be 0 (the n values of a block serve every column) or >= n"),
                                           (ok, Dk, N, S[:2], "nsrc must be 0, 1 or the number of slots"),
                                           ([0.5, 0.0, -0.5], Dk[:2], N, S, "step 2: the weight -0.5 is not finite or outside [0, 1]")):
        rc, X, cyc, msg = call(w, dblocks, ldd, sblocks)
        assert rc == 11 and (X == 7.25).all() and (cyc == -7).all() and "otmb_op_periodic_season: " + text in msg, (rc, msg)
    rc, X, cyc, msg = call(ok, Dk, N, S)
    assert rc == 0 and (cyc > 0).all() and D.slots == (3, 0), (rc, msg)
