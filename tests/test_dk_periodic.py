"""GPU: otmb_op_periodic_dk (csrc/otmb_periodic.hip): the periodic state of k tracers, every one with its own d, in one call.  Every column
equals the k = 1 periodic call with d = D[:, c] (the existing exports: the new ones with ldd = 0) in X, cycles, defect, reason and
msolve_iters; the columns finish after different numbers of cycles and the first to finish is neither the first nor the last column, so the
compact gather of the iterating columns moves columns past it; and every answer is judged against the dense fixed point of its own cycle
(periodic_ref.DenseCycle), which shares no code with the library.

The λ column.  D is dk_cases.columns(zero=False): a column without any sink has no periodic state (the transport matrix conserves mass).
periodic_ref.periodic_ref over DenseCycle, on the CPU, on odd_nx_fold with θ = 1, three steps of a month from slot 2, GMRES(30), ptol = 1e-8
and the source of this test takes, per column, [32, 44, c₂, 14, 31, 20, c₆] cycles, with (c₂, c₆) = (20, 27) at λ = 1e-8, (13, 19) at 5e-8,
(8, 13) at 2e-7, (5, 8) at 1e-6 and (4, 5) at 5e-6 for the columns age + λ and age + λ/4.  At 1e-8 the random column (14 cycles) finishes
before the λ column; from 5e-8 on the λ column, third in its register block, is the first to finish.  λ = 2e-7 is used: 8 cycles against 13
for the last column and 14 for the next, a margin the device's summation order does not close."""
import numpy as np
import pytest

import dk_cases as DK
import periodic_ref as PR
import solve_lines_ref as LR
import step_ref as SR
from test_step import _operator, _start

pytestmark = pytest.mark.gpu

RTOL, PTOL, MAXITER, FIRST = 1e-12, 1e-8, 5000, 2


@pytest.fixture(scope="module")
def grids(oracle):
    made = {}
    for name in ("odd_nx_fold", "tiny_tripolar"):
        T, N, nsurf, nxt = LR.grid(oracle, name)
        made[name] = (_operator(N, *T, nxt=nxt), N, T, DK.columns(N, nsurf, zero=False), _start(N, DK.K, 101))
    yield made
    for rec in made.values():
        rec[0].close()


def _columns_equal_single_calls(D, N, T, Dk, S, what, *, theta, ncycle, restart, adjoint, precond, outer, dense=True):
    kw = dict(dt=SR.MONTH, ncycle=ncycle, theta=theta, first_slot=FIRST, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint, precond=precond, ptol=PTOL,
              restart=restart, maxcycles=400, outer=outer)
    X, info = D.periodic(S, d=Dk, **kw)
    print(what, "cycles", info.cycles.tolist(), "mean-solve iterations", info.msolve_iters.tolist())
    assert info.status == 0 and info.converged.all() and (info.defect <= PTOL).all(), info
    assert D.slots == (3, 0)
    for c in range(S.shape[1]):
        dc = np.ascontiguousarray(Dk[:, c])
        x1, i1 = D.periodic(S[:, c], d=dc, **kw)
        DK.same_bits(X[:, c], x1, (what, c, "X"))
        assert info.cycles[c] == i1.cycles[0] and info.reason[c] == i1.reason[0] and info.msolve_iters[c] == i1.msolve_iters[0], (what, c, info, i1)
        DK.same_bits(info.defect[c], i1.defect[0], (what, c, "defect"))
        if dense:  # ‖x - x*‖₂ <= ‖(I - Φ)⁻¹‖₂·(ptol·‖g‖₂ + ncycle·rtol·max_t‖b_t‖₂/σ): tests/test_periodic.py's bound, for this column's own cycle
            DC = PR.DenseCycle(N, T[0], T[1], SR.slot_values(T[2], seed=1), dt=SR.MONTH, theta=theta, ncycle=ncycle, first_slot=FIRST, d=dc, adjoint=adjoint)
            xs, gnorm, ninv = DC.fixed_point(S[:, c:c + 1])
            bound = ninv * (PTOL * gnorm[0] + ncycle * RTOL * DC.rhs_norms(xs, S[:, c:c + 1])[0] / DC.sigma)
            err = np.linalg.norm(X[:, c] - xs[:, 0])
            print(what, "column", c, "error", err, "bound", bound)
            assert err <= bound, (what, c, err, bound)
    return info


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("outer", ["none", "mean"])
def test_every_column_is_the_single_call_with_its_own_d(grids, outer, precond):
    """odd_nx_fold, k = 7, θ = 1, three steps of a month from slot 2, GMRES(30)."""
    D, N, T, Dk, S = grids["odd_nx_fold"]
    info = _columns_equal_single_calls(D, N, T, Dk, S, (outer, precond), theta=1.0, ncycle=3, restart=30, adjoint=False, precond=precond, outer=outer)
    first = int(np.argmin(info.cycles))
    assert len(set(info.cycles.tolist())) > 1 and 0 < first < DK.K - 1 and (info.cycles > info.cycles[first]).sum() == DK.K - 1, info
    if outer == "none":
        assert first == 2  # the λ column, as on the CPU
    assert (info.msolve_iters > 0).all() == (outer == "mean")


def test_the_adjoint_with_restarts_on_a_larger_grid(grids):
    """tiny_tripolar (N = 429: several workgroups of the solver, one of the periodic kernels), Aᵀ, θ = 0.5, seven steps, GMRES(5), outer =
    mean with lines, k = 7 and k = 3."""
    D, N, T, Dk, S = grids["tiny_tripolar"]
    kw = dict(theta=0.5, ncycle=7, restart=5, adjoint=True, precond="lines", outer="mean")
    info = _columns_equal_single_calls(D, N, T, Dk, S, "tiny_tripolar", dense=False, **kw)
    assert len(set(info.cycles.tolist())) > 1, info
    _columns_equal_single_calls(D, N, T, Dk[:, 2:5], S[:, 2:5], "tiny_tripolar, k = 3", dense=False, **kw)
