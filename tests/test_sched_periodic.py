"""GPU: otmb_op_periodic_sched (csrc/otmb_periodic.hip): the periodic state of the SCHEDULED cycle -- sub-steps inside a slot and a source per
slot.  The call has THE BITS of the restatement (tests/periodic_ref.py, tests/periodic_pc_ref.py, order="device") over this operator's own
step_sched() as the cycle map and, for outer="mean", an operator over the cycle-mean values with the schedule's visit weights, one column
per call; every answer is judged by one more scheduled cycle, ‖F(x) - x‖₂ <= ptol·‖g‖₂; on odd_nx_fold (N = 117) it lies inside the bound
of tests/test_periodic.py around the dense fixed point (I - Φ)⁻¹·g of tests/sched_ref.py; and one case runs at n = 2049 (two workgroups of
the file's kernels) with a d per column.
The bit-for-bit system is that of tests/test_periodic_rows.py: solve_ref.dominant(n) with random lines, d uniform(0, 1), δt = 2, rtol = 1e-12,
ptol = 1e-8; here with three slots x two sub-steps, cycles of 6 and of 7 steps from slot 2, three source blocks and GMRES(5)."""
import numpy as np
import pytest

import periodic_pc_ref as PC
import periodic_ref as PR
import sched_ref as SC
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_step import _csc, _operator, _same_bits

pytestmark = pytest.mark.gpu

RTOL, PTOL, MAXITER = 1e-12, 1e-8, 5000
DT, FIRST, SUBSTEPS, RESTART, MAXCYCLES = 2.0, 2, 2, 5, 200
K = 3


def _d(n):
    return np.random.default_rng(13).uniform(0.0, 1.0, n)


def _blocks(n):
    """Three blocks of three columns: column 0 is ones, twos and a random block; column 1 is zero in two of the three blocks (it must be
    iterated all the same); column 2 is zero in every block (answered with zero, never stepped)."""
    rng = np.random.default_rng(1000 + n)
    S = [np.zeros((n, K), order="F") for _ in range(3)]
    S[0][:, 0], S[1][:, 0], S[2][:, 0] = 1.0, 2.0, rng.standard_normal(n)
    S[1][:, 1] = rng.standard_normal(n)
    return S


@pytest.fixture(scope="module")
def systems():
    """Per (n, ncycle): the operator with the tests' three slots and, for the restated mean solve, one over the mean values of that cycle."""
    import otmb_amd.api as api

    ops, means = {}, {}

    def get(n, ncycle):
        if n not in ops:
            ops[n] = (_operator(n, *R.dominant(n), nxt=LR.random_lines(n, 3)), R.dominant(n))
        if (n, ncycle) not in means:
            p, i, v = ops[n][1]
            M = api.DeviceOperator(_csc(n, p, i, SC.mean_values(SR.slot_values(v, seed=1), ncycle, FIRST, SUBSTEPS)))
            M.set_lines(LR.random_lines(n, 3))
            means[(n, ncycle)] = M
        return ops[n][0], means[(n, ncycle)]

    yield get
    for D, _ in ops.values():
        D.close()
    for M in means.values():
        M.close()


def _restated(D, M, S, d, *, theta, ncycle, adjoint, precond, outer, x0=None):
    """The restatement in the device's order over D.step_sched (and M.solve), one column per call; d: n values or n x k."""
    dcol = (lambda c: d) if d.ndim == 1 else (lambda c: np.ascontiguousarray(d[:, c]))

    def run(c, x, src):
        X, info = D.step_sched(x, dt=DT, theta=theta, nsteps=ncycle, first_slot=FIRST, substeps=SUBSTEPS, source=src, d=dcol(c), rtol=RTOL, maxiter=MAXITER,
                               adjoint=adjoint, precond=precond)
        return X if info.status == 0 and info.steps_done == ncycle else None

    def qinv(c, v):
        q, info = M.solve(v, d=dcol(c), sigma=0.0, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)
        return (PC.precondition(v, q, float(ncycle) * DT) if info.converged.all() else None), int(info.iterations[0])

    F, Phi = (lambda c, x: run(c, x, [B[:, c] for B in S])), (lambda c, v: run(c, v, None))
    kw = dict(x0=x0, ptol=PTOL, restart=RESTART, maxcycles=MAXCYCLES, order="device")
    if outer == "mean":
        return PC.periodic_pc_ref(F, Phi, qinv, SC.all_blocks(S), **kw)
    Xr, ref = PR.periodic_ref(F, Phi, SC.all_blocks(S), **kw)
    return Xr, dict(ref, msolve_iters=np.zeros(len(ref["cycles"]), dtype=np.int64))


def _has_the_restatements_bits(X, info, Xr, ref, what):
    print(what, "cycles", info.cycles.tolist(), "restated", ref["cycles"].tolist(), "msolve", info.msolve_iters.tolist(), "defect", info.defect.tolist(),
          "reason", info.reason)
    assert np.array_equal(info.cycles, ref["cycles"]), (what, info.cycles, ref["cycles"])
    assert list(info.reason) == list(ref["reason"]), (what, info.reason, ref["reason"])
    assert np.array_equal(info.msolve_iters, ref["msolve_iters"]), (what, info.msolve_iters, ref["msolve_iters"])
    _same_bits(info.defect, ref["defect"], (what, "defect", info.defect.tolist(), ref["defect"].tolist()))
    for c in range(X.shape[1]):
        _same_bits(X[:, c], Xr[:, c], (what, "X, column", c, float(np.abs(X[:, c] - Xr[:, c]).max())))


def _judged_by_one_more_cycle(D, X, S, d, what, *, theta, ncycle, adjoint, precond):
    """One more scheduled cycle from X and one from zero: ‖F(x) - x‖₂ <= ptol·‖g‖₂·(1 + 1e-6) per column."""
    kw = dict(dt=DT, theta=theta, nsteps=ncycle, first_slot=FIRST, substeps=SUBSTEPS, source=S, d=d, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
              precond=precond)
    FX, si = D.step_sched(X, **kw)
    G, sg = D.step_sched(np.zeros_like(X), **kw)
    assert si.status == 0 and sg.status == 0
    for c in range(X.shape[1]):
        defect, g = np.linalg.norm(FX[:, c] - X[:, c]), np.linalg.norm(G[:, c])
        print(what, "column", c, "‖F(x) - x‖", defect, "ptol·‖g‖", PTOL * g)
        assert defect <= PTOL * g * (1 + 1e-6), (what, c, defect, g)


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("outer", ["none", "mean"])
@pytest.mark.parametrize("ncycle", [6, 7])
def test_the_call_has_the_bits_of_the_restatement(systems, ncycle, outer, theta, adjoint, precond):
    """n = 513, k = 3: a column with a source in every block, one with a source in one block of three, one without.  ncycle = 7 is no
    multiple of the sub-steps: slot 2 is visited three times (the mean's weights 2/7, 2/7, 3/7)."""
    n = 513
    D, M = systems(n, ncycle)
    S, d = _blocks(n), _d(n)
    kw = dict(theta=theta, ncycle=ncycle, adjoint=adjoint, precond=precond)
    X, info = D.periodic_sched(S, dt=DT, first_slot=FIRST, substeps=SUBSTEPS, d=d, rtol=RTOL, maxiter=MAXITER, ptol=PTOL, restart=RESTART,
                               maxcycles=MAXCYCLES, outer=outer, **kw)
    what = (ncycle, outer, theta, adjoint, precond)
    assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), (what, info)
    assert info.cycles[1] > 2, info  # zero in two blocks of three: iterated all the same
    assert info.cycles[2] == 0 and not X[:, 2].any() and info.defect[2] == 0.0
    assert (info.msolve_iters[:2] > 0).all() if outer == "mean" else not info.msolve_iters.any()
    Xr, ref = _restated(D, M, S, d, outer=outer, **kw)
    _has_the_restatements_bits(X, info, Xr, ref, what)
    _judged_by_one_more_cycle(D, X, S, d, what, **kw)
    assert D.slots == (3, 0)


def test_with_a_start_and_the_list_through_periodic(systems):
    """x0: the first call carries x and 0 side by side, 2k columns with every block's sources twice; from the returned state one cycle is
    enough.  periodic() with a list of blocks is periodic_sched(); a single array with substeps = 1 is the call there was."""
    n, ncycle = 513, 6
    D, M = systems(n, ncycle)
    S, d = _blocks(n), _d(n)
    kw = dict(theta=0.5, ncycle=ncycle, adjoint=False, precond="lines")
    call = dict(dt=DT, first_slot=FIRST, d=d, rtol=RTOL, maxiter=MAXITER, ptol=PTOL, restart=RESTART, maxcycles=MAXCYCLES, **kw)
    X, info = D.periodic_sched(S, substeps=SUBSTEPS, **call)
    x0 = np.asfortranarray(np.random.default_rng(2000 + n).standard_normal((n, K)))
    x0[:, 1] = X[:, 1]
    for outer in ("none", "mean"):
        X1, info1 = D.periodic_sched(S, substeps=SUBSTEPS, x0=x0, outer=outer, **call)
        assert info1.status == 0 and info1.cycles[0] > 2 and info1.cycles[1] == 1 and info1.cycles[2] == 0, info1
        _same_bits(X1[:, 1], X[:, 1], "the returned state is accepted as it is")
        Xr, ref = _restated(D, M, S, d, outer=outer, x0=x0, **kw)
        _has_the_restatements_bits(X1, info1, Xr, ref, ("with a start", outer))
        _judged_by_one_more_cycle(D, X1, S, d, ("with a start", outer), **kw)
    # substeps = 1 and three blocks through periodic(): the list alone makes it the scheduled call
    Xl, il = D.periodic(S, **call)
    Xs, i_s = D.periodic_sched(S, substeps=1, **call)
    _same_bits(Xl, Xs, "periodic() with a list")
    assert np.array_equal(il.cycles, i_s.cycles)
    # one block in a list, substeps = 1: the bits of the call with the array
    Xa, ia = D.periodic(S[0], **call)
    Xb, ib = D.periodic([S[0]], **call)
    _same_bits(Xa, Xb, "a list of one is the array")
    assert np.array_equal(ia.cycles, ib.cycles) and ia.cycles[1] == 0  # (in block 0 alone, column 1 is zero: not stepped)
    _same_bits(ia.defect, ib.defect, "a list of one is the array: defect")


@pytest.mark.parametrize("outer", ["none", "mean"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_against_the_dense_fixed_point_on_the_small_grid(oracle, theta, outer):
    """odd_nx_fold (N = 117), the age d, δt = a month, 3 slots x 2 sub-steps, 6 steps from slot 2, three sources, lines, GMRES(40), ptol = 1e-8,
    rtol = 1e-12: ‖x - x*‖₂ <= ‖(I - Φ)⁻¹‖₂·(ptol·‖g‖₂ + ncycle·rtol·max_t‖b_t‖₂/σ), the bound of tests/test_periodic.py, with x* = (I - Φ)⁻¹·g
    from a dense LU per step."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    d = R.shift("age", N, nsurf)[0]
    rng = np.random.default_rng(61)
    S = [np.asfortranarray(rng.standard_normal((N, 2))) for _ in range(3)]
    for B in S:
        B[:, 0] = 1.0
    values = SR.slot_values(T[2], seed=1)
    with _operator(N, *T, nxt=nxt) as D:
        for adjoint in (False, True):
            DS = SC.DenseSched(N, T[0], T[1], values, dt=SR.MONTH, theta=theta, ncycle=6, first_slot=FIRST, substeps=SUBSTEPS, d=d, adjoint=adjoint)
            xs, gnorm, ninv, bmax = DS.fixed_point(S)
            X, info = D.periodic_sched(S, dt=SR.MONTH, ncycle=6, theta=theta, first_slot=FIRST, substeps=SUBSTEPS, d=d, rtol=RTOL, maxiter=MAXITER,
                                       adjoint=adjoint, precond="lines", ptol=PTOL, restart=40, maxcycles=1000, outer=outer)
            assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), info
            for c in range(2):
                err, bound = np.linalg.norm(X[:, c] - xs[:, c]), ninv * (PTOL * gnorm[c] + 6 * RTOL * bmax[c] / DS.sigma)
                print(theta, outer, adjoint, "column", c, "cycles", int(info.cycles[c]), "error", err, "bound", bound)
                assert err <= bound, (theta, outer, adjoint, c, err, bound)
        assert D.slots == (3, 0)


def test_two_workgroups_and_a_d_per_column(systems):
    """n = 2049: the second workgroup of the periodic kernels holds one row; every column has its own d; outer = "mean", θ = 0.5, lines,
    seven steps a cycle."""
    n, ncycle = 2049, 7
    D, M = systems(n, ncycle)
    S = _blocks(n)
    Dk = np.asfortranarray(np.random.default_rng(17).uniform(0.0, 1.0, (n, K)))
    kw = dict(theta=0.5, ncycle=ncycle, adjoint=False, precond="lines")
    X, info = D.periodic_sched(S, dt=DT, first_slot=FIRST, substeps=SUBSTEPS, d=Dk, rtol=RTOL, maxiter=MAXITER, ptol=PTOL, restart=RESTART,
                               maxcycles=MAXCYCLES, outer="mean", **kw)
    assert info.status == 0 and info.converged.all() and info.cycles[2] == 0 and not X[:, 2].any(), info
    Xr, ref = _restated(D, M, S, Dk, outer="mean", **kw)
    _has_the_restatements_bits(X, info, Xr, ref, ("n = 2049, D",))
    _judged_by_one_more_cycle(D, X, S, Dk, ("n = 2049, D",), **kw)
    assert D.slots == (3, 0)
