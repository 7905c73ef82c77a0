"""CPU: tests/step_ref.py, the numpy restatement of otmb_op_step.  Every step's solution meets the float64 residual bound of the solver's
tests for its own system (solve_ref.residual_check: no new tolerance), every step agrees with scipy's sparse LU of the same system from
the same previous state -- the LU side forming its own right-hand side -- as far as the two residuals allow (a per-step check, not an
independent LU trajectory), and a step that does not converge ends the call."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR

RTOL = 1e-10


def _start(N, k, seed):
    X = np.ones((N, k), order="F")
    X[:, 1:] = np.random.default_rng(seed).standard_normal((N, k - 1))
    return X


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name,lines", [("odd_nx_fold", False), ("odd_nx_fold", True), ("tiny_tripolar", True), ("small_rho3d", True)])
def test_two_cycles_of_three_slots_against_sparse_lu(oracle, name, lines, theta):
    """6 steps (2 cycles of 3 slots) from first_slot = 2, with the age d and a random source, A and Aᵀ.  A PER-STEP check: the LU side starts
    every step from the restatement's previous state (it carries no trajectory of its own, whose drift would need ‖M⁻¹‖ to bound), but
    forms that step's right-hand side itself, b_lu = (σ·x + s/θ) - c·(d∘x + A·x) with scipy's product, and solves its own b_lu.  Per step
    and column, M the step's matrix and b the restatement's right-hand side:
      * |b - b_lu| ≤ (L + 6)·ε·(|σ·x| + |s/θ| + c·(|d|∘|x| + |A|·|x|)) rowwise: the two evaluations differ by their rounding alone (a row's
        product is at most L terms in either order, then at most five more operations) -- a wrong right-hand side in step_ref fails here;
      * ‖b - M·x‖₂ ≤ residual_check's bound (rtol·‖b‖₂ + the rounding of the residual's two evaluations);
      * ‖M·(x - x_lu)‖₂ ≤ that bound + ‖b_lu - M·x_lu‖₂ + ‖b - b_lu‖₂ + 2·(L + 3)·ε·‖ |M|·|x_lu| + |b_lu| ‖₂: the triangle inequality over
        the two residuals and the two right-hand sides, the last term the rounding of the second residual's own evaluation and of the
        product on the left (each γ_{L+2}·(|M|·|x| + |b|) rowwise, as in residual_check)."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    p, i, v = T
    values = SR.slot_values(v, seed=1)
    d = R.shift("age", N, nsurf)[0]
    S = np.random.default_rng(2).standard_normal((N, 2)) * 1e-7
    sigma, cc = SR.constants(SR.MONTH, theta)
    for adjoint in (False, True):
        X0 = _start(N, 2, 3)
        X, info = SR.step_ref(N, p, i, values, X0, dt=SR.MONTH, theta=theta, nsteps=6, first_slot=2, source=S, d=d, rtol=RTOL,
                              maxiter=5000, adjoint=adjoint, next=nxt if lines else None)
        assert info["steps_done"] == 6 and [s for s, _, _ in info["systems"]] == [2, 0, 1, 2, 0, 1]
        assert np.array_equal(X, info["systems"][-1][2])
        Xprev = X0
        for t, (slot, B, Xt) in enumerate(info["systems"]):
            A = R.csc_of(N, N, p, i, values[slot])
            As = sp.csc_matrix(A)
            Aop = (As.T if adjoint else As).tocsr()
            M = R.system(As, d, sigma, adjoint)
            lu = spla.splu(M.tocsc())
            L = R.longest(A, adjoint)
            Blu = (sigma * Xprev + S / theta) - cc * (d[:, None] * Xprev + Aop @ Xprev)
            scale = np.abs(sigma * Xprev) + np.abs(S / theta) + cc * (np.abs(d)[:, None] * np.abs(Xprev) + abs(Aop) @ np.abs(Xprev))
            assert (np.abs(B - Blu) <= (L + 6) * R.EPS * scale).all(), (t, float(np.max(np.abs(B - Blu))))
            for c, (res, bound) in enumerate(R.residual_check(A, Xt, B, d, sigma, adjoint, RTOL)):
                xl = lu.solve(Blu[:, c])
                resl = np.linalg.norm(Blu[:, c] - M @ xl)
                db = np.linalg.norm(B[:, c] - Blu[:, c])
                slack = 2 * (L + 3) * R.EPS * np.linalg.norm(abs(M) @ np.abs(xl) + np.abs(Blu[:, c]))
                diff = np.linalg.norm(M @ (Xt[:, c] - xl))
                print(name, "lines", lines, "theta", theta, "adjoint", adjoint, "step", t, "slot", slot, "column", c, "iterations",
                      info["iterations"][t][c], "residual", res, "bound", bound, "splu residual", resl, "‖b - b_lu‖", db,
                      "‖M·(x - x_lu)‖", diff)
                assert res <= bound
                assert diff <= bound + resl + db + slack
            Xprev = Xt


def test_the_elementwise_line():
    """rhs against a literal loop over Python floats, in the contract's association; θ = 1 reads no product."""
    rng = np.random.default_rng(5)
    n, dt = 9, 7.0
    X, W, S, d = rng.standard_normal((n, 2)), rng.standard_normal((n, 2)), rng.standard_normal((n, 2)), rng.uniform(0, 1, n)
    for theta in (1.0, 0.5, 0.3):
        sigma = 1.0 / (theta * dt)
        c = (1.0 - theta) / theta
        for SS in (None, S):
            for dd in (None, d):
                got = SR.rhs(X, None if theta == 1 else W, SS, dd, dt, theta)
                for r in range(n):
                    for col in range(2):
                        x, w = float(X[r, col]), float(W[r, col])
                        sx = sigma * x
                        if theta == 1:
                            want = sx if SS is None else sx + float(SS[r, col])
                        else:
                            a = sx if SS is None else sx + float(SS[r, col]) / theta
                            e = w if dd is None else float(dd[r]) * x + w
                            want = a - c * e
                        assert got[r, col] == want
    assert np.array_equal(SR.rhs(X[:, 0], W[:, 0], S[:, 0], d, dt, 0.5), SR.rhs(X, W, S, d, dt, 0.5)[:, 0])  # 1-D: the column's bits


def test_a_step_that_does_not_converge_ends_the_call(oracle):
    """maxiter = 1 on the month system (Jacobi needs hundreds of iterations there): the call stops at step 0 with steps_done == 0, reports
    that step's reasons and returns its last iterates."""
    T, N, nsurf, nxt = LR.grid(oracle, "tiny_tripolar")
    p, i, v = T
    X0 = _start(N, 2, 7)
    X, info = SR.step_ref(N, p, i, SR.slot_values(v), X0, dt=SR.MONTH, nsteps=4, rtol=RTOL, maxiter=1)
    assert info["steps_done"] == 0 and len(info["systems"]) == 1 and info["reason"] == [("maxiter", "maxiter")]
    assert [int(x) for x in info["iterations"][0]] == [1, 1]
    B = SR.rhs(X0, None, None, None, SR.MONTH, 1.0)
    Xs, _ = R.solve_ref(R.csc_of(N, N, p, i, v), B, sigma=SR.constants(SR.MONTH, 1.0)[0], rtol=RTOL, maxiter=1, x0=X0)
    assert np.array_equal(X, Xs) and not np.array_equal(X, X0)
    # nsteps = 0 touches nothing; invalid arguments are refused
    X, info = SR.step_ref(N, p, i, SR.slot_values(v), X0, dt=SR.MONTH, nsteps=0)
    assert np.array_equal(X, X0) and info["steps_done"] == 0 and info["systems"] == []
    for bad in (dict(dt=0.0), dict(dt=1.0, theta=0.0), dict(dt=1.0, theta=1.5), dict(dt=1.0, nsteps=-1), dict(dt=1.0, first_slot=3)):
        with pytest.raises(ValueError):
            SR.step_ref(N, p, i, SR.slot_values(v), X0, **bad)


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name,lines", [("odd_nx_fold", False), ("odd_nx_fold", True), ("tiny_tripolar", False), ("tiny_tripolar", True)])
def test_step_residual_check_on_the_restatements_trajectory(oracle, name, lines, theta):
    """step_ref.step_residual_check (the helper tests/test_step.py judges the device's steps with) on the restatement's own four steps from
    slot 2, A and Aᵀ, the age d, a source of scale 1e-7, k = 3: every (X_{t-1}, X_t) pair meets the bound with its slot's matrix.  And the
    helper can tell: with another slot's matrix, with the adjoint flipped, with another θ or without the source the same pair exceeds it."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    p, i, v = T
    values = SR.slot_values(v, seed=1)
    d = R.shift("age", N, nsurf)[0]
    S = np.asfortranarray(np.random.default_rng(11).standard_normal((N, 3)) * 1e-7)
    for adjoint in (False, True):
        X0 = _start(N, 3, 12)
        X, info = SR.step_ref(N, p, i, values, X0, dt=SR.MONTH, theta=theta, nsteps=4, first_slot=2, source=S, d=d, rtol=RTOL, maxiter=5000,
                              adjoint=adjoint, next=nxt if lines else None)
        assert info["steps_done"] == 4
        Xprev = X0
        for t, (slot, _, Xt) in enumerate(info["systems"]):
            assert slot == (2 + t) % 3
            A = R.csc_of(N, N, p, i, values[slot])
            for c, (res, bound) in enumerate(SR.step_residual_check(A, Xprev, Xt, S, d, SR.MONTH, theta, adjoint, RTOL)):
                print(name, "lines", lines, "theta", theta, "adjoint", adjoint, "step", t, "column", c, "residual", res, "bound", bound)
                assert res <= bound
            wrong = [dict(A=R.csc_of(N, N, p, i, values[(slot + 1) % 3])), dict(adjoint=not adjoint), dict(theta=0.75), dict(S=None)]
            for kw in wrong:
                a = dict(A=A, S=S, theta=theta, adjoint=adjoint)
                a.update(kw)
                out = SR.step_residual_check(a["A"], Xprev, Xt, a["S"], d, SR.MONTH, a["theta"], a["adjoint"], RTOL)
                assert all(res > bound for res, bound in out), (t, sorted(kw), out)
            Xprev = Xt


# the (θ, δt) pairs of the fixed-point test (tests/test_step.py: test_a_steady_state_is_a_fixed_point_of_the_step has the same list)
FIXED_POINT_PAIRS = [(theta, dt) for theta in (1.0, 0.5, 0.25) for dt in (R.DAY, SR.MONTH)]


def steady_age(oracle, name="odd_nx_fold"):
    """The steady ideal age on a grid: (T's arrays, N, next, d, s = 1, x*) with x* from scipy's sparse LU of diag(d) + A and one step of
    iterative refinement in float64."""
    T, N, nsurf, nxt = LR.grid(oracle, name)
    d = R.shift("age", N, nsurf)[0]
    M0 = (sp.diags(d) + R.csc_of(N, N, *T)).tocsc()
    lu = spla.splu(M0)
    s = np.ones(N)
    x = lu.solve(s)
    x = x + lu.solve(s - M0 @ x)
    return T, N, nxt, d, s, x


@pytest.mark.parametrize("theta,dt", FIXED_POINT_PAIRS)
def test_a_steady_state_is_a_fixed_point_of_the_step(oracle, theta, dt):
    """The CPU twin of the device test of the same name: with (diag(d) + A)·x* = s, b - M·x* = (s - (diag(d) + A)·x*)/θ whatever σ is, so a
    step from x* needs no iteration -- if the constants are right.  So that the device test can neither fail nor pass for a reason of
    rounding, two margins are asserted here for every (θ, δt) it runs, with rtol = 1e-10:
      * the restatement starts every one of three steps at a relative residual ≤ rtol/100 (and so takes no iteration and returns x*'s bits);
      * (L + c)·ε·‖ |M|·|x*| + |b| ‖₂ ≤ rtol·‖b‖₂/100 with c = step_ref.STEP_LINE_OPS: whatever order the device sums b and M·x* in, its
        residual differs from the restatement's by far less than the margin the first line leaves."""
    T, N, nxt, d, s, x = steady_age(oracle)
    p, i, v = T
    sigma, cc = SR.constants(dt, theta)
    for lines in (False, True):
        X, info = SR.step_ref(N, p, i, [v, v, v], x, dt=dt, theta=theta, nsteps=3, source=s, d=d, rtol=RTOL, next=nxt if lines else None)
        print("theta", theta, "dt", dt, "lines", lines, "relres", [float(r[0]) for r in info["relres"]])
        assert info["steps_done"] == 3 and all(int(it[0]) == 0 for it in info["iterations"])
        assert all(float(r[0]) <= RTOL / 100 for r in info["relres"])
        assert np.array_equal(X, x)
    A = R.csc_of(N, N, p, i, v)
    M = R.system(A, d, sigma, False)
    b = info["systems"][0][1]
    rounding = (R.longest(A, False) + SR.STEP_LINE_OPS) * R.EPS * np.linalg.norm(abs(M) @ np.abs(x) + np.abs(b))
    print("theta", theta, "dt", dt, "rounding bound", rounding, "rtol·‖b‖/100", RTOL * np.linalg.norm(b) / 100)
    assert rounding <= RTOL * np.linalg.norm(b) / 100
