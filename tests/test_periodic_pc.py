"""GPU: otmb_op_periodic_pc[_dev] (csrc/otmb_periodic.hip): the periodic state with a choice of preconditioner for the outer GMRES.
OTMB_OUTER_NONE has otmb_op_periodic_dev's bits.  OTMB_OUTER_MEAN -- flexible GMRES preconditioned by the cycle-mean operator -- is judged as
tests/test_periodic.py judges: by step() itself (one more cycle, ‖F(x) - x‖₂ <= ptol·‖g‖₂) and against the dense fixed point, and it takes
fewer cycles than the unpreconditioned call on the same operator; beyond one workgroup and one row pair it has THE BITS of the restatement
(tests/periodic_pc_ref.py in the device's order over the operator's own step() and solve(), as tests/test_periodic_rows.py does); a column of
seven has the bits of the column alone; a NaN column and a starved mean solve stop alone; a singular mean is refused with X untouched; the
caller's slots and selection are untouched; and the assembler's route."""
import numpy as np
import pytest

import periodic_pc_ref as PC
import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_periodic import _judge, _reference
from test_step import _csc, _operator, _same_bits, _start

pytestmark = pytest.mark.gpu

RTOL, PTOL, MAXITER = 1e-12, 1e-8, 5000
FIRST = 2
SENTINEL = 7.25
NONE_CAP = 200  # maxcycles of the unpreconditioned call that is compared against: see test_the_mean_preconditioner_on_the_fixtures


@pytest.fixture(scope="module")
def grids(oracle):
    """odd_nx_fold (N = 117) and tiny_tripolar (N = 429) with the tests' three slots, the water columns, the age d and a source of seven columns."""
    made = {}
    for name in ("odd_nx_fold", "tiny_tripolar"):
        T, N, nsurf, nxt = LR.grid(oracle, name)
        made[name] = (_operator(N, *T, nxt=nxt), N, T, R.shift("age", N, nsurf)[0], _start(N, 7, 101), nxt)
    yield made
    for rec in made.values():
        rec[0].close()


def _slot_reads(D, X):
    """A·X and Aᵀ·X of every slot (both value arrays of each), and the selection: what a call must leave as it was."""
    n, sel = D.slots
    out = []
    for s in range(n):
        D.select(s)
        out += [D.mul(X), D.mul(X, adjoint=True)]
    D.select(sel)
    return out, (n, sel)


def _untouched(D, X, before, what):
    after = _slot_reads(D, X)
    assert after[1] == before[1], what
    for a, b in zip(after[0], before[0]):
        _same_bits(a, b, (what, "the caller's slots"))


# ---- OTMB_OUTER_NONE ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_x0,pc,adjoint", [(0, 1, 0), (1, 0, 1)], ids=["from-zero-lines-plain", "start-jacobi-adjoint"])
def test_outer_none_has_the_bits_of_otmb_op_periodic_dev(oracle, use_x0, pc, adjoint):
    """odd_nx_fold, k = 3, through otmb_op_periodic_pc_dev with OTMB_OUTER_NONE: X, cycles, defect and reason of otmb_op_periodic_dev, and
    msolve_iters zero."""
    from otmb_amd.device import DeviceAssembler
    from test_op_padded_dev import _System, _pad, _same

    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    k = 3
    P = _System(DeviceAssembler(0).ctx, N, T, R.shift("age", N, nsurf)[0], 0.0, k, nxt=nxt)
    S0, X0 = _start(N, k, 141), (_start(N, k, 142) if use_x0 else np.full((N, k), SENTINEL))
    args = lambda S, X: (P.h, adjoint, k, P.dd.data_ptr(), SR.MONTH, 0.5, 7, FIRST, S.data_ptr(), N, X.data_ptr(), N, use_x0, RTOL, MAXITER, pc, PTOL, 5, 1000)
    try:
        out = []
        for pcall in (False, True):
            S, X = _pad(S0, 0, np.nan), _pad(X0, 0, SENTINEL)
            cyc, dft, why, ms = np.full(k, -7, np.int64), np.full(k, SENTINEL), np.full(k, -7, np.int32), np.full(k, -7, np.int64)
            tail = (cyc.ctypes.data, dft.ctypes.data, why.ctypes.data)
            rc = P.lib.otmb_op_periodic_pc_dev(*args(S, X), *tail, 0, ms.ctypes.data) if pcall else P.lib.otmb_op_periodic_dev(*args(S, X), *tail)
            out.append((rc, X, cyc, dft, why, ms))
        (rc0, Xa, cyc0, dft0, why0, _), (rc1, Xb, cyc1, dft1, why1, ms) = out
        print("none", cyc0.tolist(), cyc1.tolist(), dft0.tolist())
        assert rc0 == rc1 == 0 and (cyc0 > 7).all() and np.array_equal(cyc0, cyc1) and np.array_equal(why0, why1) and not ms.any()
        _same(dft0, dft1, "defect")
        _same(Xa, Xb, "X")
        assert P.O.slots == (3, 0)
    finally:
        P.O.close()


# ---- OTMB_OUTER_MEAN on the fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("restart", [5, 20])
@pytest.mark.parametrize("ncycle", [3, 7])
@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("k", [1, 3, 7])
@pytest.mark.parametrize("name", ["odd_nx_fold", "tiny_tripolar"])
def test_the_mean_preconditioner_on_the_fixtures(grids, name, k, theta, adjoint, precond, ncycle, restart):
    """The age d, δt = a month, rtol = 1e-12, ptol = 1e-8, cycles of 3 and 7 steps over the 3 slots from slot 2.  Every answer is judged by
    step() and against the dense x* within tests/test_periodic.py's bound, and every column takes fewer cycles than in the outer="none" call
    on the same operator.  That call is the parent's code path; it runs with maxcycles = 200, so a column that needs more reports 199 or
    200 cycles, a lower bound of what it needs -- the comparison is then the stricter one, and no case waits for a thousand cycles."""
    D, N, T, d, S7, _ = grids[name]
    S = S7[:, :k]
    before = _slot_reads(D, S7[:, :2])
    kw = dict(dt=SR.MONTH, ncycle=ncycle, theta=theta, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond, ptol=PTOL,
              restart=restart)
    X, info = D.periodic(S, outer="mean", maxcycles=1000, **kw)
    _, none = D.periodic(S, outer="none", maxcycles=NONE_CAP, **kw)
    print(name, k, theta, adjoint, precond, ncycle, restart, "cycles", none.cycles.tolist(), "->", info.cycles.tolist(), "mean-solve iterations",
          info.msolve_iters.tolist())
    assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), info
    assert (info.cycles < none.cycles).all(), (info, none)
    assert (info.msolve_iters > 0).all() and not none.msolve_iters.any()
    _untouched(D, S7[:, :2], before, (name, k, theta, adjoint, precond, ncycle, restart))
    _judge(D, X, info, S7, d, _reference(N, T, d, S7, theta, adjoint, ncycle), (name, k, theta, adjoint, precond, ncycle, restart), theta=theta,
           adjoint=adjoint, precond=precond, ncycle=ncycle)


# ---- bits, beyond one workgroup and one row pair ---------------------------------------------------------------------------------------------
DT, THETA, NCYCLE, RESTART, MAXCYCLES, K = 2.0, 0.5, 4, 7, 200, 3
CASES = [(513, True, "jacobi"), (2048, False, "lines"), (2049, False, "lines"), (2049, True, "jacobi"), (4609, True, "lines")]
IDS = [f"{n}-{'adjoint' if a else 'plain'}-{pc}" for n, a, pc in CASES]


def _d(n):
    return np.random.default_rng(13).uniform(0.0, 1.0, n)


def _source(n):
    S = np.zeros((n, K), order="F")
    S[:, 0] = 1.0
    S[:, 1] = np.random.default_rng(1000 + n).standard_normal(n)
    return S


@pytest.fixture(scope="module")
def rows():
    """Per n: the system of tests/test_periodic_rows.py (solve_ref.dominant(n), random lines, three slots) and, beside it, an operator of its
    own over the mean values as combine_ref gives them, for the restatement's mean solve."""
    import otmb_amd.api as api

    made = {}

    def get(n):
        if n not in made:
            p, i, v = R.dominant(n)
            nxt = LR.random_lines(n, 3)
            mean = PC.combine_ref(SR.slot_values(v, seed=1), PC.visit_weights(3, NCYCLE, FIRST))
            M = api.DeviceOperator(_csc(n, p, i, mean))
            M.set_lines(nxt)
            made[n] = (_operator(n, p, i, v, nxt=nxt), M)
        return made[n]

    yield get
    for D, M in made.values():
        D.close()
        M.close()


def _restated(D, M, n, S, adjoint, precond, x0=None, maxiter=MAXITER):
    """tests/periodic_pc_ref.py in the device's order over D.step and M.solve, one column per call."""
    kw = dict(dt=DT, theta=THETA, nsteps=NCYCLE, first_slot=FIRST, d=_d(n), rtol=RTOL, maxiter=maxiter, adjoint=adjoint, precond=precond)

    def run(x, s):
        X, info = D.step(x, source=s, **kw)
        return X if info.status == 0 and info.steps_done == NCYCLE else None

    def qinv(c, v):
        q, info = M.solve(v, d=_d(n), sigma=0.0, rtol=RTOL, maxiter=maxiter, adjoint=adjoint, precond=precond)
        return (PC.precondition(v, q, float(NCYCLE) * DT) if info.converged.all() else None), int(info.iterations[0])

    return PC.periodic_pc_ref(lambda c, x: run(x, S[:, c]), lambda c, v: run(v, None), qinv, S, x0=x0, ptol=PTOL, restart=RESTART, maxcycles=MAXCYCLES,
                              order="device")


def _call(D, n, S, adjoint, precond, x0=None):
    return D.periodic(S, dt=DT, ncycle=NCYCLE, theta=THETA, first_slot=FIRST, d=_d(n), x0=x0, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                      precond=precond, ptol=PTOL, restart=RESTART, maxcycles=MAXCYCLES, outer="mean")


def _has_the_restatements_bits(X, info, Xr, ref, what):
    print(what, "cycles", info.cycles.tolist(), "restated", ref["cycles"].tolist(), "mean-solve iterations", info.msolve_iters.tolist(), "restated",
          ref["msolve_iters"].tolist(), "defect", info.defect.tolist(), "reason", info.reason)
    assert np.array_equal(info.cycles, ref["cycles"]), (what, info.cycles, ref["cycles"])
    assert np.array_equal(info.msolve_iters, ref["msolve_iters"]), (what, info.msolve_iters, ref["msolve_iters"])
    assert list(info.reason) == list(ref["reason"]), (what, info.reason, ref["reason"])
    _same_bits(info.defect, ref["defect"], (what, "defect", info.defect.tolist(), ref["defect"].tolist()))
    for c in range(X.shape[1]):
        _same_bits(X[:, c], Xr[:, c], (what, "X, column", c, float(np.abs(X[:, c] - Xr[:, c]).max())))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_call_has_the_bits_of_the_restatement(rows, case):
    """k = 3 -- ones, a random source, a zero source -- GMRES(7), from zero and then with a start (column 0 from a random state, column 1 from
    the X just returned: one cycle, no mean solve).  n = 513: a lane's second row pair; 2048: a workgroup exactly full; 2049 and 4609: two and
    three workgroups, the last of one row or partly filled.  X, cycles, defect, reason and msolve_iters, bit for bit; the slots untouched."""
    n, adjoint, precond = case
    D, M = rows(n)
    S = _source(n)
    before = _slot_reads(D, S[:, :2])
    X, info = _call(D, n, S, adjoint, precond)
    assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), info
    assert (info.cycles[:2] > 2).all() and (info.msolve_iters[:2] > 0).all(), info
    assert info.cycles[2] == 0 and info.msolve_iters[2] == 0 and not X[:, 2].any()
    Xr, ref = _restated(D, M, n, S, adjoint, precond)
    _has_the_restatements_bits(X, info, Xr, ref, ("from zero",) + case)
    x0 = np.asfortranarray(np.random.default_rng(2000 + n).standard_normal((n, K)))
    x0[:, 1] = X[:, 1]
    X1, info1 = _call(D, n, S, adjoint, precond, x0=x0)
    assert info1.status == 0 and info1.converged.all() and info1.cycles[0] > 2 and info1.cycles[1] == 1 and info1.msolve_iters[1] == 0, info1
    _same_bits(X1[:, 1], X[:, 1], "the returned state is accepted as it is")
    Xr1, ref1 = _restated(D, M, n, S, adjoint, precond, x0=x0)
    _has_the_restatements_bits(X1, info1, Xr1, ref1, ("with a start",) + case)
    _untouched(D, S[:, :2], before, case)
    # judged by step(): one more cycle from X and one from zero
    kw = dict(dt=DT, theta=THETA, nsteps=NCYCLE, first_slot=FIRST, d=_d(n), rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
    FX, _ = D.step(X1, source=S, **kw)
    G, _ = D.step(np.zeros_like(X1), source=S, **kw)
    for c in range(2):
        assert np.linalg.norm(FX[:, c] - X1[:, c]) <= PTOL * np.linalg.norm(G[:, c]) * (1 + 1e-6), (case, c)


@pytest.mark.parametrize("use_x0,pc,adjoint", [(0, 1, 0), (1, 0, 1)], ids=["from-zero-lines-plain", "start-jacobi-adjoint"])
def test_padded_and_misaligned_device_arrays_have_the_compact_calls_bits(use_x0, pc, adjoint):
    """n = 4609, k = 3, GMRES(7), otmb_op_periodic_pc_dev with OTMB_OUTER_MEAN on compact arrays (odd ld: X takes the 8-byte path), on S + 3
    and X + 5 rows (the 16-byte path) and on an X of that leading dimension one element into a larger tensor: rows [:n], cycles, defect,
    reason and msolve_iters have the compact call's bits; the padding, the element in front and S keep theirs."""
    import torch

    from otmb_amd.device import DeviceAssembler
    from test_op_padded_dev import _System, _pad, _same

    n, k = 2 * PR.PD_ROWS + 513, K
    P = _System(DeviceAssembler(0).ctx, n, R.dominant(n), _d(n), 0.5, k, nxt=LR.random_lines(n, 3))
    S0, X0 = _start(n, k, 141), (_start(n, k, 142) if use_x0 else np.full((n, k), SENTINEL))

    def call(S, lds, X, ldx):
        cyc, dft, why, ms = np.full(k, -7, np.int64), np.full(k, SENTINEL), np.full(k, -7, np.int32), np.full(k, -7, np.int64)
        rc = P.lib.otmb_op_periodic_pc_dev(P.h, adjoint, k, P.dd.data_ptr(), DT, THETA, NCYCLE, FIRST, S.data_ptr(), lds, X.data_ptr(), ldx, use_x0, RTOL,
                                           MAXITER, pc, PTOL, RESTART, MAXCYCLES, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data, 1, ms.ctypes.data)
        return rc, cyc, dft, why, ms

    try:
        Sc, Xc = _pad(S0, 0, np.nan), _pad(X0, 0, SENTINEL)
        rc, cyc, dft, why, ms = call(Sc, n, Xc, n)
        print("compact", use_x0, pc, adjoint, rc, cyc.tolist(), dft.tolist(), ms.tolist())
        assert rc == 0 and (why == 0).all() and (dft <= PTOL).all() and (cyc > 2).all() and (ms > 0).all()
        Sp, Xp = _pad(S0, 3, np.nan), _pad(X0, 5, SENTINEL)
        assert (n + 5) % 2 == 0 and Xp.data_ptr() % 16 == 0
        rcp, cycp, dftp, whyp, msp = call(Sp, n + 3, Xp, n + 5)
        assert rcp == 0 and np.array_equal(cycp, cyc) and np.array_equal(whyp, why) and np.array_equal(msp, ms)
        _same(dftp, dft, "padded: defect")
        _same(Xp[:n], Xc, "rows [:n] of the padded call")
        assert (Xp[n:] == SENTINEL).all().item() and Sp[n:].isnan().all().item()
        _same(Sp[:n], S0, "S is not written")
        ld = n + 5
        flat = torch.full((1 + k * ld,), SENTINEL, dtype=torch.float64, device="cuda")
        Xm = flat[1:].view(k, ld).t()
        Xm[:n] = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda().t()
        assert Xm.stride() == (1, ld) and Xm.data_ptr() % 16 == 8
        rcm, cycm, dftm, whym, msm = call(Sp, n + 3, Xm, ld)
        assert rcm == 0 and np.array_equal(cycm, cyc) and np.array_equal(whym, why) and np.array_equal(msm, ms)
        _same(dftm, dft, "misaligned: defect")
        _same(Xm[:n], Xc, "rows [:n] of the misaligned call")
        assert (Xm[n:] == SENTINEL).all().item() and flat[0].item() == SENTINEL
        _same(Sp[:n], S0, "S is not written")
        assert P.O.slots == (3, 0)
    finally:
        P.O.close()


# ---- columns are independent --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta,precond,restart", [(1.0, "lines", 5), (0.5, "jacobi", 20)])
def test_a_column_of_seven_has_the_bits_of_the_column_alone(grids, theta, precond, restart):
    D, N, T, d, S7, _ = grids["odd_nx_fold"]
    kw = dict(dt=SR.MONTH, ncycle=3, theta=theta, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, precond=precond, ptol=PTOL, restart=restart, outer="mean")
    X, info = D.periodic(S7, **kw)
    X2, info2 = D.periodic(S7, **kw)
    assert info.converged.all()
    _same_bits(X, X2, "the same call twice")
    _same_bits(info.defect, info2.defect, "the same call twice: defect")
    assert np.array_equal(info.cycles, info2.cycles) and np.array_equal(info.msolve_iters, info2.msolve_iters)
    for c in (0, 3, 6):
        xc, ic = D.periodic(S7[:, c], **kw)
        print("column", c, "cycles", int(ic.cycles[0]), "of", info.cycles.tolist(), "mean-solve iterations", int(ic.msolve_iters[0]), "of", info.msolve_iters.tolist())
        _same_bits(xc, X[:, c], ("column alone", c))
        _same_bits(ic.defect[0], info.defect[c], ("column alone: defect", c))
        assert ic.cycles[0] == info.cycles[c] and ic.msolve_iters[0] == info.msolve_iters[c]


def test_a_nan_source_column_stops_alone(grids):
    from otmb_amd import capi

    D, N, T, d, S7, _ = grids["odd_nx_fold"]
    S = np.asfortranarray(S7[:, :3].copy())
    S[5, 1] = np.nan
    kw = dict(dt=SR.MONTH, ncycle=3, theta=0.5, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, precond="lines", ptol=PTOL, restart=10, outer="mean")
    X, info = D.periodic(S, **kw)
    msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
    print(info, msg)
    assert info.status == 19 and info.reason[0] == info.reason[2] == "converged" and info.reason[1] in ("step_failed", "nonfinite"), info
    assert "; the step: " in msg and "(step 0, slot 2)" in msg, msg
    assert not X[:, 1].any() and info.msolve_iters[1] == 0
    clean, ic = D.periodic(S[:, [0, 2]], **kw)
    assert ic.converged.all()
    _same_bits(X[:, [0, 2]], clean, "the clean columns")
    _same_bits(info.defect[[0, 2]], ic.defect, "their defects")
    assert np.array_equal(info.cycles[[0, 2]], ic.cycles) and np.array_equal(info.msolve_iters[[0, 2]], ic.msolve_iters)
    assert D.slots == (3, 0)


# ---- a starved mean solve -----------------------------------------------------------------------------------------------------------------------
def _two_blocks(ne=40, nh=40, seed=9):
    """A block-diagonal matrix: a diagonal block (Jacobi is exact on it: every solve takes one iteration) and solve_ref.dominant(nh, 5)."""
    import scipy.sparse as sp

    H = R.csc_of(nh, nh, *R.dominant(nh, per_row=5, seed=seed))
    A = sp.csc_matrix(sp.block_diag([sp.diags(np.random.default_rng(seed).uniform(1.0, 2.0, ne)), H]))
    A.sort_indices()
    return ne + nh, A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, A.data.astype(np.float64)


def test_a_starved_mean_solve_stops_its_column_alone():
    """maxiter = 1.  The case was picked on the CPU restatement (periodic_pc_ref over cycle_maps and mean_maps): two uncoupled blocks, a
    diagonal one and a diagonally dominant one, δt = 1e-9 (σ = 1e9 against entries of order 1 to 16), θ = 1, Jacobi, rtol = 1e-13,
    ptol = 1e-6, three steps from slot 2.  With σ that large every step converges in its one iteration from the warm start, in both blocks;
    the mean solve at σ = 0 takes one iteration on the diagonal block and about ten on the other.  Column 0's source lives on the diagonal
    block, and so do its Krylov vectors: its mean solve survives.  Column 1 is zero.  Column 2's source covers both blocks: its first mean
    solve -- in one call with column 0's, which is then repeated without it -- does not converge: precond_failed on column 2 alone, with
    the state of its last explicit defect, the start.  The restatement over this operator's own step() and solve() gives the same bits."""
    import otmb_amd.api as api
    from otmb_amd import capi

    n, p, i, v = _two_blocks()
    rng = np.random.default_rng(2)
    S = np.zeros((n, 3), order="F")
    S[:40, 0] = rng.uniform(1.0, 2.0, 40)
    S[:, 2] = rng.uniform(1.0, 2.0, n)
    kw = dict(dt=1e-9, ncycle=3, theta=1.0, first_slot=FIRST, rtol=1e-13, precond="jacobi", ptol=1e-6, restart=5, maxcycles=50)
    mean = PC.combine_ref(SR.slot_values(v, seed=1), PC.visit_weights(3, 3, FIRST))
    with _operator(n, p, i, v) as D, api.DeviceOperator(_csc(n, p, i, mean)) as M:
        X, info = D.periodic(S, outer="mean", maxiter=1, **kw)
        msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
        print(info, msg)
        assert info.status == 19 and info.reason == ("converged", "converged", "precond_failed"), info
        assert "precond failed" in msg and "; the mean solve: " in msg and "maxiter after 1 iterations" in msg, msg
        assert info.cycles.tolist()[1:] == [0, 1] and info.msolve_iters.tolist()[1:] == [0, 1] and info.msolve_iters[0] >= 1
        assert not X[:, 2].any() and info.defect[2] == 1.0  # the start, and g's own defect
        assert info.defect[0] <= 1e-6 and D.slots == (3, 0)

        def run(x, s):
            Y, si = D.step(x, source=s, dt=1e-9, theta=1.0, nsteps=3, first_slot=FIRST, rtol=1e-13, maxiter=1, precond="jacobi")
            return Y if si.status == 0 and si.steps_done == 3 else None

        def qinv(c, u):
            q, si = M.solve(u, sigma=0.0, rtol=1e-13, maxiter=1, precond="jacobi")
            return (PC.precondition(u, q, 3.0 * 1e-9) if si.converged.all() else None), int(si.iterations[0])

        Xr, ref = PC.periodic_pc_ref(lambda c, x: run(x, S[:, c]), lambda c, u: run(u, None), qinv, S, ptol=1e-6, restart=5, maxcycles=50, order="device")
        _has_the_restatements_bits(X, info, Xr, ref, "starved")
        # with iterations to spare every column converges, in fewer cycles than without the preconditioner
        X2, info2 = D.periodic(S, outer="mean", maxiter=100, **kw)
        _, none = D.periodic(S, outer="none", maxiter=100, **kw)
        print(info2, none)
        assert info2.status == 0 and info2.converged.all() and (info2.cycles[[0, 2]] < none.cycles[[0, 2]]).all()
        _same_bits(X2[:, 0], X[:, 0], "column 0 is the column of the starved call")


# ---- a singular mean ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", ["jacobi", "lines"])
def test_a_singular_mean_is_refused_with_x_untouched(grids, precond):
    """d chosen so that diag(M̄) has a zero: d_j = -(the mean values' diagonal entry j), in the bits the fold gives it.  No slot is singular
    (the slots' diagonals differ from their mean at j), so the unpreconditioned call runs; the preconditioned one is refused before X or the
    report arrays are written, and the operator goes on working."""
    from otmb_amd import capi
    from test_periodic import _periodic_c

    D, N, T, d, S7, nxt = grids["odd_nx_fold"]
    p, i, v = T
    mean = PC.combine_ref(SR.slot_values(v, seed=1), PC.visit_weights(3, 3, FIRST))
    j = int(np.flatnonzero(~np.isin(np.arange(1, N + 1), nxt))[3])  # the head of a line: its pivot is the diagonal entry itself
    at = np.flatnonzero(i[p[j] - 1:p[j + 1] - 1] == j + 1)
    assert len(at) == 1
    dz = d.copy()
    dz[j] = -mean[p[j] - 1 + at[0]]
    S = np.asfortranarray(S7[:, :2])
    X0 = _start(N, 2, 161)
    before = _slot_reads(D, S)
    pc = capi.PRECONDS[precond]
    X = X0.copy(order="F")
    cyc, dft, why, ms = np.full(2, -7, np.int64), np.full(2, SENTINEL), np.full(2, -7, np.int32), np.full(2, -7, np.int64)
    rc = capi.lib().otmb_op_periodic_pc(D.handle, 0, 2, dz.ctypes.data, SR.MONTH, 1.0, 3, FIRST, S.ctypes.data, N, X.ctypes.data, N, 1, RTOL, MAXITER, pc, PTOL, 10,
                                        100, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data, 1, ms.ctypes.data)
    msg = capi.lib().otmb_last_error(D.ctx.handle).decode()
    print(rc, msg)
    assert rc == 18 and "(the cycle-mean operator)" in msg, (rc, msg)
    assert np.array_equal(X, X0) and (cyc == -7).all() and (dft == SENTINEL).all() and (why == -7).all() and (ms == -7).all()
    with pytest.raises(capi.OtmbError) as e:
        D.periodic(S, dt=SR.MONTH, ncycle=3, first_slot=FIRST, d=dz, precond=precond, outer="mean")
    assert e.value.name == "SINGULAR_PRECONDITIONER"
    _untouched(D, S, before, "after the refusal")
    # an outer that is neither value, and the Python side's own refusal
    X = X0.copy(order="F")
    rc = capi.lib().otmb_op_periodic_pc(D.handle, 0, 2, d.ctypes.data, SR.MONTH, 1.0, 3, FIRST, S.ctypes.data, N, X.ctypes.data, N, 1, RTOL, MAXITER, pc, PTOL, 10,
                                        100, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data, 2, ms.ctypes.data)
    assert rc == 11 and np.array_equal(X, X0) and (cyc == -7).all()
    assert "outer must be OTMB_OUTER_NONE or OTMB_OUTER_MEAN" in capi.lib().otmb_last_error(D.ctx.handle).decode()
    with pytest.raises(capi.OtmbError, match="outer"):
        D.periodic(S, dt=SR.MONTH, ncycle=3, outer="annual")
    assert _periodic_c(D, X, N, 2, S=S, lds=N, d=d, use_x0=1, ptol=0.0)[0] == 11  # (otmb_op_periodic's checks are the wrapper's)
    Xs, info = D.periodic(S, dt=SR.MONTH, ncycle=3, first_slot=FIRST, d=d, precond=precond, rtol=RTOL, outer="mean")
    assert info.converged.all()


# ---- the assembler's route -----------------------------------------------------------------------------------------------------------------------
def test_the_assemblers_route_has_the_operators_bits():
    """DeviceAssembler.periodic_tracers(outer="mean") on three kept months of small_rho3d against api.DeviceOperator.periodic(outer="mean")
    over the same three value sets: X, cycles, defect, reason and msolve_iters, bit for bit."""
    import torch

    import otmb_amd.api as api
    from test_kept_ops import _fields, _host, _pair

    g, gm, asm, other, umo, vmo, fill = _pair("small_rho3d")
    del other
    N = asm.N
    fields = _fields(umo, vmo, 3, seed=5)
    months = []
    for m in range(3):
        asm.step(*fields[m], fill)
        asm.keep_slot(m, nslots=3)
        months.append(_host(asm)["T"])
    S = _start(N, 2, 152)
    d = np.random.default_rng(151).uniform(0.5e-7, 1.5e-7, N)
    Sd = torch.from_numpy(S).cuda().t().contiguous().t()
    kw = dict(dt=SR.MONTH, ncycle=3, theta=1.0, first_slot=1, rtol=1e-10, maxiter=MAXITER, precond="lines", ptol=PTOL, restart=10, maxcycles=40, outer="mean")
    Xa, ia = asm.periodic_tracers(Sd, d=torch.from_numpy(d).cuda(), **kw)
    p, i, _ = months[0]
    with api.DeviceOperator(api.SparseMatrixCSC(N, N, p, i, months[0][2])) as D:
        D.set_lines(asm.vertical_lines().cpu().numpy())
        D.set_slots(3)
        for m in range(1, 3):
            D.set_values(months[m][2], slot=m)
        Xo, io = D.periodic(S, d=d, **kw)
    print("assembler", ia, io)
    assert ia.status == io.status and ia.reason == io.reason and np.array_equal(ia.cycles, io.cycles) and (ia.cycles > 1).all()
    assert np.array_equal(ia.msolve_iters, io.msolve_iters) and (ia.msolve_iters > 0).all()
    _same_bits(Xa.cpu().numpy(), Xo, "periodic_tracers")
    _same_bits(ia.defect, io.defect, "defect")
