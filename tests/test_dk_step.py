"""GPU: otmb_op_step_dk (csrc/otmb_step.hip): θ-steps of k tracers, every one with its own d.  Every column of a per-column call equals the
k = 1 step with d = D[:, c] -- the existing exports, which are the new ones with ldd = 0 -- in state, reports, observations and mean; one
step is checked against the θ-method written down in float64 (step_ref.step_residual_check), which shares no code with the library; and a
step that fails in one column only leaves what the k = 1 calls leave."""
import numpy as np
import pytest

import dk_cases as DK
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR
from test_step import _operator, _start

pytestmark = pytest.mark.gpu

RTOL, MAXITER = 1e-10, 5000
NSTEPS, FIRST, Q = 7, 2, 3


@pytest.fixture(scope="module")
def small(oracle):
    """odd_nx_fold (N = 117) with the three slots of tests/step_ref.py: slot_values and the water columns; D has the zero column (σ > 0)."""
    T, N, nsurf, nxt = LR.grid(oracle, "odd_nx_fold")
    D = _operator(N, *T, nxt=nxt)
    rng = np.random.default_rng(41)
    yield D, N, T, DK.columns(N, nsurf, zero=True), _start(N, DK.K, 42), np.asfortranarray(rng.standard_normal((N, DK.K)) * 1e-7), \
        np.asfortranarray(rng.uniform(0.0, 1.0, (N, Q))), rng.uniform(0.0, 1.0, NSTEPS)
    D.close()


def _columns_equal_single_steps(D, X0, Dk, S, W, tw, what, **kw):
    Xs, info = D.step(X0, d=Dk, source=S, observe=W, time_weights=tw, rtol=RTOL, maxiter=MAXITER, **kw)
    print(what, "steps_done", info.steps_done, "iterations", info.iterations.tolist())
    assert info.status == 0 and info.steps_done == kw["nsteps"], (what, info)
    for c in range(X0.shape[1]):
        x1, i1 = D.step(X0[:, c], d=np.ascontiguousarray(Dk[:, c]), source=None if S is None else S[:, c], observe=W, time_weights=tw, rtol=RTOL,
                        maxiter=MAXITER, **kw)
        DK.same_bits(Xs[:, c], x1, (what, c, "state"))
        assert i1.steps_done == info.steps_done and np.array_equal(info.iterations[:, c], i1.iterations[:, 0]), (what, c)
        assert tuple(r[c] for r in info.reason) == tuple(r[0] for r in i1.reason), (what, c)
        DK.same_bits(info.relres[:, c], i1.relres[:, 0], (what, c, "relres"))
        if W is not None:
            DK.same_bits(info.observations[:, c, :], i1.observations[:, 0, :], (what, c, "observations"))
        if tw is not None:
            DK.same_bits(info.mean[:, c], i1.mean, (what, c, "mean"))
    assert (info.observations is None) == (W is None) and (info.mean is None) == (tw is None)
    return Xs, info


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_every_column_is_the_single_step_with_its_own_d(small, theta, adjoint, precond):
    """k = 7, 7 steps from slot 2 over 3 slots (every slot is visited again: its per-column preconditioner is reused), δt = a month; source and
    no source; observers (q = 3) and the mean on and off."""
    D, N, T, Dk, X7, S7, W, tw = small
    kw = dict(dt=SR.MONTH, theta=theta, nsteps=NSTEPS, first_slot=FIRST, adjoint=adjoint, precond=precond)
    for S in (None, S7):
        for watch in (False, True):
            _, info = _columns_equal_single_steps(D, X7, Dk, S, W if watch else None, tw if watch else None, (theta, adjoint, precond, S is not None, watch), **kw)
    assert len(set(info.iterations[0].tolist())) > 1, info  # the columns are different systems
    assert D.slots == (3, 0)
    # k = 3 (register blocks 2 + 1)
    _columns_equal_single_steps(D, X7[:, :3], Dk[:, 2:5], S7[:, :3], None, None, (theta, adjoint, precond, "k = 3"), **kw)


@pytest.mark.parametrize("name", ["tiny_tripolar", "small_rho3d"])
def test_larger_grids_and_the_float64_residual_of_one_step(oracle, name):
    """N = 429 and 6962: θ = 0.5, A and Aᵀ, lines, k = 7, a source, observers and the mean; and one step from slot 1, every column against the
    θ-method of its own d in float64."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    p, i, v = T
    Dk = DK.columns(N, nsurf, zero=True)
    rng = np.random.default_rng(51)
    S, X0 = np.asfortranarray(rng.standard_normal((N, DK.K)) * 1e-7), _start(N, DK.K, 52)
    W, tw = np.asfortranarray(rng.uniform(0.0, 1.0, (N, Q))), rng.uniform(0.0, 1.0, 3)
    values = SR.slot_values(v, seed=1)
    with _operator(N, p, i, v, nxt=nxt) as D:
        for adjoint in (False, True):
            _columns_equal_single_steps(D, X0, Dk, S, W, tw, (name, adjoint), dt=SR.MONTH, theta=0.5, nsteps=3, first_slot=FIRST, adjoint=adjoint,
                                        precond="lines")
            Xs, info = D.step(X0, d=Dk, source=S, dt=SR.MONTH, theta=0.5, nsteps=1, first_slot=1, rtol=RTOL, maxiter=MAXITER, adjoint=adjoint,
                              precond="lines")
            assert info.status == 0
            A = R.csc_of(N, N, p, i, values[1])
            for c in range(DK.K):
                (res, bound), = SR.step_residual_check(A, X0[:, c], Xs[:, c], S[:, c], Dk[:, c], SR.MONTH, 0.5, adjoint, RTOL)
                print(name, adjoint, "column", c, "residual", res, "bound", bound)
                assert res <= bound, (name, adjoint, c, res, bound)


def test_a_step_that_fails_in_one_column_only(small):
    """Jacobi, θ = 1: the CPU restatement (step_ref.step_ref over solve_ref) says how many iterations every column's first step takes; maxiter
    is put half way between the slowest column and the next, so the first step fails in that column alone.  steps_done, the reports and X
    -- the failing step's last iterates, in every column -- are those of the k = 1 calls.  The column 1e-5·age is replaced by 3·age here: on
    the CPU it takes 257 iterations and the all-zero column 343, but BiCGStab's count on these two nearly singular systems moves with the
    order of the sums by more than their distance (the device needs over 300 for the former), so two slow columns cannot be told apart by
    a count taken on the CPU.  With one slow column the CPU's counts are about 25 for six columns and 343 for the seventh."""
    D, N, T, Dk, X7, S7, W, tw = small
    Dk = Dk.copy(order="F")
    Dk[:, 1] = 3.0 * Dk[:, 0]
    values = SR.slot_values(T[2], seed=1)
    kw = dict(dt=SR.MONTH, theta=1.0, first_slot=FIRST, adjoint=False)
    cpu = [int(SR.step_ref(N, T[0], T[1], values, X7[:, c:c + 1], nsteps=1, source=S7[:, c:c + 1], d=Dk[:, c], rtol=RTOL, maxiter=MAXITER, **kw)[1]
               ["iterations"][0][0]) for c in range(DK.K)]
    order = np.argsort(cpu)
    slowest, gap = int(order[-1]), cpu[order[-1]] - cpu[order[-2]]
    print("iterations of the first step on the CPU", cpu, "slowest column", slowest)
    assert gap >= 200 and cpu[order[-2]] <= 40, cpu  # maxiter then lies 100 iterations from either side
    maxiter = cpu[order[-2]] + gap // 2
    Xs, info = D.step(X7, d=Dk, source=S7, nsteps=NSTEPS, rtol=RTOL, maxiter=maxiter, precond="jacobi", **kw)
    print(info)
    assert info.status == 19 and info.steps_done == 0 and len(info.iterations) == 1
    assert [r != "converged" for r in info.reason[0]] == [c == slowest for c in range(DK.K)], info
    for c in range(DK.K):
        x1, i1 = D.step(X7[:, c], d=np.ascontiguousarray(Dk[:, c]), source=S7[:, c], nsteps=1, rtol=RTOL, maxiter=maxiter, precond="jacobi", **kw)
        DK.same_bits(Xs[:, c], x1, (c, "the failing step's last iterates"))
        assert i1.steps_done == (0 if c == slowest else 1) and i1.iterations[0, 0] == info.iterations[0, c] and i1.reason[0][0] == info.reason[0][c]
        DK.same_bits(i1.relres[0, 0], info.relres[0, c], (c, "relres"))
