"""GPU: csrc/otmb_periodic.hip beyond one workgroup and one row pair.  Every kernel of that file gives a workgroup PD_ROWS = 2048 rows, lane t
the row pairs t, t + 256, t + 512, t + 768 of them; the fixtures of tests/test_periodic.py have n <= 429, where there is one workgroup, one
partial per quantity (np = 1: every `... * np + workgroup` stride collapses, pd_fold_kernel adds nothing) and no lane has a second pair.

Here otmb_op_periodic has THE BITS of the restatement: tests/periodic_ref.py in its device order (order="device": every sum, update, back
substitution and division in the kernels' and GmresLsq's order) over this operator's own step() as the cycle map, one column per call (a
column of k has the bits of the column alone: tests/test_step.py, tests/test_periodic.py).  X, cycles, defect and reason are compared with
np.array_equal; no tolerance appears.  Independently every answer is judged by step(): one more cycle from X and one from zero give
‖F(x) - x‖₂ <= ptol·‖g‖₂·(1 + 1e-6).  Sizes:
    513   lane 0's second row pair (q = 1), a single last row, odd n, one workgroup
    2048  one workgroup exactly full (q = 3 for every lane), even n, np = 1
    2049  np = 2: the second workgroup holds one row beside the padding row
    4609  np = 3, the last workgroup partly filled, odd n (the size of tests/test_periodic_host.py)
The system is the padded test's, grown: solve_ref.dominant(n) with solve_lines_ref.random_lines(n, 3), d uniform(0, 1), δt = 2, θ = 0.5,
four steps a cycle from slot 2, rtol = 1e-12, ptol = 1e-8, GMRES(7) -- seven basis vectors: register blocks 4 + 2 + 1 -- maxcycles = 200.
And otmb_op_periodic_dev on compact, padded and misaligned X at n = 4609."""
import numpy as np
import pytest

import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R
from test_step import _operator, _same_bits

pytestmark = pytest.mark.gpu

RTOL, PTOL, MAXITER = 1e-12, 1e-8, 5000
DT, THETA, NCYCLE, FIRST, RESTART, MAXCYCLES = 2.0, 0.5, 4, 2, 7, 200
SENTINEL = 7.25
K = 3

# (n, adjoint, precond): the four combinations at n = 2049, one each at the other sizes
CASES = [(513, True, "jacobi"), (2048, False, "lines"), (2049, False, "lines"), (2049, False, "jacobi"), (2049, True, "lines"),
         (2049, True, "jacobi"), (4609, True, "lines")]
IDS = [f"{n}-{'adjoint' if a else 'plain'}-{pc}" for n, a, pc in CASES]


def _d(n):
    return np.random.default_rng(13).uniform(0.0, 1.0, n)


def _source(n):
    """Three columns in three phases: ones, random, and a zero source (no cycle, x = 0) beside the two that iterate."""
    S = np.zeros((n, K), order="F")
    S[:, 0] = 1.0
    S[:, 1] = np.random.default_rng(1000 + n).standard_normal(n)
    return S


@pytest.fixture(scope="module")
def operators():
    made = {}

    def get(n):
        if n not in made:
            made[n] = _operator(n, *R.dominant(n), nxt=LR.random_lines(n, 3))
        return made[n]

    yield get
    for D in made.values():
        D.close()


def _step_kw(n, adjoint, precond):
    return dict(dt=DT, theta=THETA, nsteps=NCYCLE, first_slot=FIRST, d=_d(n), rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond)


def _periodic(D, n, S, adjoint, precond, x0=None):
    return D.periodic(S, dt=DT, ncycle=NCYCLE, theta=THETA, first_slot=FIRST, d=_d(n), x0=x0, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                      precond=precond, ptol=PTOL, restart=RESTART, maxcycles=MAXCYCLES)


def _restated(D, n, S, adjoint, precond, x0=None):
    """tests/periodic_ref.py in the device's order over D.step, one column per call."""
    kw = _step_kw(n, adjoint, precond)

    def run(x, s):
        X, info = D.step(x, source=s, **kw)
        return X if info.status == 0 and info.steps_done == NCYCLE else None

    return PR.periodic_ref(lambda c, x: run(x, S[:, c]), lambda c, v: run(v, None), S, x0=x0, ptol=PTOL, restart=RESTART, maxcycles=MAXCYCLES,
                           order="device")


def _has_the_restatements_bits(X, info, Xr, ref, what):
    print(what, "cycles", info.cycles.tolist(), "restated", ref["cycles"].tolist(), "defect", info.defect.tolist(), "reason", info.reason)
    for c, history in enumerate(ref["history"]):
        print("   column", c, "restated explicit defects", history)
    assert np.array_equal(info.cycles, ref["cycles"]), (what, info.cycles, ref["cycles"])
    assert list(info.reason) == list(ref["reason"]), (what, info.reason, ref["reason"])
    _same_bits(info.defect, ref["defect"], (what, "defect", info.defect.tolist(), ref["defect"].tolist()))
    for c in range(K):
        _same_bits(X[:, c], Xr[:, c], (what, "X, column", c, float(np.abs(X[:, c] - Xr[:, c]).max())))


def _judged_by_step(D, n, X, S, adjoint, precond, what):
    """One more cycle of step() from X and one from zero: ‖F(x) - x‖₂ <= ptol·‖g‖₂·(1 + 1e-6) per column."""
    kw = _step_kw(n, adjoint, precond)
    FX, si = D.step(X, source=S, **kw)
    G, sg = D.step(np.zeros_like(X), source=S, **kw)
    assert si.status == 0 and sg.status == 0
    for c in range(K):
        defect, g = np.linalg.norm(FX[:, c] - X[:, c]), np.linalg.norm(G[:, c])
        print(what, "column", c, "‖F(x) - x‖", defect, "ptol·‖g‖", PTOL * g)
        assert defect <= PTOL * g * (1 + 1e-6), (what, c, defect, g)


_FROM_ZERO = {}


def _from_zero(operators, case):
    """The call without a start, once per case: the started test begins from its X."""
    if case not in _FROM_ZERO:
        n, adjoint, precond = case
        _FROM_ZERO[case] = _periodic(operators(n), n, _source(n), adjoint, precond)
    return _FROM_ZERO[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_from_zero_the_call_has_the_bits_of_the_restatement(operators, case):
    """k = 3 without a start: ones, a random source and a ZERO source.  The two that iterate take more than restart + 2 cycles each (the
    basis reached seven vectors -- register blocks 4 + 2 + 1 -- and a restart happened; on the CPU over sparse LU solves: 13 to 14), the
    zero column takes none and is zero."""
    n, adjoint, precond = case
    D, S = operators(n), _source(n)
    X, info = _from_zero(operators, case)
    assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), info
    assert (info.cycles[:2] > RESTART + 2).all(), info
    assert info.cycles[2] == 0 and not X[:, 2].any() and info.defect[2] == 0.0
    Xr, ref = _restated(D, n, S, adjoint, precond)
    assert all(len(h) > 2 for h in ref["history"][:2])  # g, then at least one restart's explicit defect before the accepted one
    _has_the_restatements_bits(X, info, Xr, ref, ("from zero",) + case)
    _judged_by_step(D, n, X, S, adjoint, precond, ("from zero",) + case)
    assert D.slots == (3, 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_with_a_start_the_call_has_the_bits_of_the_restatement(operators, case):
    """k = 3 with x0: column 0 from a random state, column 1 from the X just returned for it (one cycle, accepted as it is), column 2 a zero
    source whatever its start.  The first call is the 2k-column one whose sources lie in the bases, ‖g‖² goes to the second half of the
    column's scalars and pd_defect_kernel subtracts x."""
    n, adjoint, precond = case
    D, S = operators(n), _source(n)
    X, info = _from_zero(operators, case)
    assert info.converged.all()
    x0 = np.asfortranarray(np.random.default_rng(2000 + n).standard_normal((n, K)))
    x0[:, 1] = X[:, 1]
    before = x0.copy()
    X1, info1 = _periodic(D, n, S, adjoint, precond, x0=x0)
    assert np.array_equal(x0, before)
    assert info1.status == 0 and info1.converged.all() and (info1.defect <= PTOL).all(), info1
    assert info1.cycles[0] > 2 and info1.cycles[1] == 1 and info1.cycles[2] == 0, info1
    _same_bits(X1[:, 1], X[:, 1], "the returned state is accepted as it is")
    _same_bits(info1.defect[1], info.defect[1], "on the defect it was accepted on")
    assert not X1[:, 2].any() and info1.defect[2] == 0.0
    Xr, ref = _restated(D, n, S, adjoint, precond, x0=x0)
    _has_the_restatements_bits(X1, info1, Xr, ref, ("with a start",) + case)
    _judged_by_step(D, n, X1, S, adjoint, precond, ("with a start",) + case)
    assert D.slots == (3, 0)


# ---- otmb_op_periodic_dev: compact, padded and misaligned X at three workgroups -------------------------------------------------------------
@pytest.mark.parametrize("use_x0,pc,adjoint", [(0, 1, 0), (1, 0, 1)], ids=["from-zero-lines-plain", "start-jacobi-adjoint"])
def test_padded_and_misaligned_device_arrays_have_the_compact_calls_bits(use_x0, pc, adjoint):
    """n = 4609 (np = 3), k = 3, GMRES(7), otmb_op_periodic_dev on: compact arrays (ld = n, odd: X takes the 8-byte path); S + 3 and X + 5
    rows (ldx even on an aligned base: the 16-byte path); and an X of the same even ldx whose base is 8 bytes off a 16-byte boundary, a view
    one element into a larger tensor (the 8-byte path through the pointer test).  Rows [:n], cycles, defect and reason have the compact
    call's bits, the padding and the element in front of the misaligned X keep the sentinel, S keeps its bits (NaN padding included)."""
    import torch

    from otmb_amd.device import DeviceAssembler
    from test_op_padded_dev import _System, _pad, _same
    from test_step import _start

    n, k = 2 * PR.PD_ROWS + 513, K
    P = _System(DeviceAssembler(0).ctx, n, R.dominant(n), _d(n), 0.5, k, nxt=LR.random_lines(n, 3))
    S0, X0 = _start(n, k, 141), (_start(n, k, 142) if use_x0 else np.full((n, k), SENTINEL))

    def call(S, lds, X, ldx):
        cyc, dft, why = np.full(k, -7, np.int64), np.full(k, SENTINEL), np.full(k, -7, np.int32)
        rc = P.lib.otmb_op_periodic_dev(P.h, adjoint, k, P.dd.data_ptr(), DT, THETA, NCYCLE, FIRST, S.data_ptr(), lds, X.data_ptr(), ldx, use_x0, RTOL, MAXITER,
                                        pc, PTOL, RESTART, MAXCYCLES, cyc.ctypes.data, dft.ctypes.data, why.ctypes.data)
        return rc, cyc, dft, why

    try:
        Sc, Xc = _pad(S0, 0, np.nan), _pad(X0, 0, SENTINEL)
        rc, cyc, dft, why = call(Sc, n, Xc, n)
        print("compact", use_x0, pc, adjoint, rc, cyc.tolist(), dft.tolist())
        assert rc == 0 and (why == 0).all() and (dft <= PTOL).all()
        assert (cyc > (2 if use_x0 else RESTART + 2)).all()  # every column iterates; from zero through a restart
        _same(Sc, S0, "S is not written (compact)")
        # padded: an aligned base and an even leading dimension
        Sp, Xp = _pad(S0, 3, np.nan), _pad(X0, 5, SENTINEL)
        assert (n + 5) % 2 == 0 and Xp.data_ptr() % 16 == 0
        rcp, cycp, dftp, whyp = call(Sp, n + 3, Xp, n + 5)
        assert rcp == 0 and np.array_equal(cycp, cyc) and np.array_equal(whyp, why)
        _same(dftp, dft, "padded: defect")
        _same(Xp[:n], Xc, "rows [:n] of the padded call")
        assert (Xp[n:] == SENTINEL).all().item() and Sp[n:].isnan().all().item()
        _same(Sp[:n], S0, "S is not written")
        # misaligned: the same leading dimension, the base one element into a larger tensor
        ld = n + 5
        flat = torch.full((1 + k * ld,), SENTINEL, dtype=torch.float64, device="cuda")
        Xm = flat[1:].view(k, ld).t()
        Xm[:n] = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda().t()
        assert Xm.stride() == (1, ld) and Xm.data_ptr() == flat.data_ptr() + 8 and Xm.data_ptr() % 16 == 8
        rcm, cycm, dftm, whym = call(Sp, n + 3, Xm, ld)
        assert rcm == 0 and np.array_equal(cycm, cyc) and np.array_equal(whym, why)
        _same(dftm, dft, "misaligned: defect")
        _same(Xm[:n], Xc, "rows [:n] of the misaligned call")
        assert (Xm[n:] == SENTINEL).all().item() and flat[0].item() == SENTINEL
        assert Sp[n:].isnan().all().item()
        _same(Sp[:n], S0, "S is not written")
        assert P.O.slots == (3, 0)
    finally:
        P.O.close()
