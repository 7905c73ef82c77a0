"""A numpy restatement of otmb_op_step (csrc/otmb_step.hip, include/otmb.h): θ-steps of ∂x/∂t + (diag(d) + A)·x = s through a cycle of
value slots, step t with the matrix of slot (first_slot + t) mod nslots,

    σ = 1 / (θ·δt)  (the product, then its reciprocal)
    θ = 1:  b_i = σ·x_i + s_i
    θ < 1:  w = A·x (tests/spmv_ref.py: α = 1, β = 0);  c = (1 - θ) / θ;  e_i = d_i·x_i + w_i;  b_i = (σ·x_i + s_i/θ) - c·e_i
    (σ·I + diag(d) + A)·x⁺ = b by the restated solver (tests/solve_ref.py, tests/solve_lines_ref.py) from x

(adjoint: Aᵀ; without s its terms are absent, without d e = w).  The elementwise line (`rhs`) is float64 numpy, one operation per
temporary and never fused: those are the contract's bits, and tests/test_step.py builds the device's composition of public calls with it."""
import numpy as np

import solve_lines_ref as LR
import solve_ref as R
from spmv_ref import spmv_ref

MONTH = 30 * R.DAY


def constants(dt, theta):
    """(σ, c) as the C side computes them (Python floats are IEEE doubles)."""
    tdt = float(theta) * float(dt)
    return 1.0 / tdt, (1.0 - float(theta)) / float(theta)


def rhs(X, W, S, d, dt, theta):
    """The step's right-hand side from the state X, the product W = A·X (not read when θ = 1), the source S or None and d or None."""
    sigma, c = constants(dt, theta)
    X = np.asarray(X, dtype=np.float64)
    sx = sigma * X
    if theta == 1:
        return sx if S is None else sx + np.asarray(S, dtype=np.float64)
    a = sx if S is None else sx + np.asarray(S, dtype=np.float64) / float(theta)
    e = np.asarray(W, dtype=np.float64)
    if d is not None:
        dd = np.asarray(d, dtype=np.float64)
        e = (dd if X.ndim == 1 else dd[:, None]) * X + e
    return a - c * e


def slot_values(nzval, seed=0):
    """The three slots of the tests: T, 0.5·T and T with every value perturbed by a seeded factor in [0.9, 1.1]."""
    v = np.asarray(nzval, dtype=np.float64)
    return [v.copy(), 0.5 * v, v * np.random.default_rng(seed).uniform(0.9, 1.1, v.size)]


def step_ref(n, colptr, rowval, values, X, *, dt, theta=1.0, nsteps=1, first_slot=0, source=None, d=None, rtol=1e-10, maxiter=10000,
             adjoint=False, next=None):
    """values: one nzval per slot over the pattern (colptr, rowval); next: the lines (None: Jacobi).
    -> (X after the call, info): info = dict(steps_done, iterations, relres, reason, systems), the middle three one row per step that ran a
    solve, systems = per such step (slot, B, X after it).  A step that leaves a column not converged ends the call; X holds its last iterates."""
    if not (dt > 0 and 0 < theta <= 1 and nsteps >= 0 and 0 <= first_slot < len(values)):
        raise ValueError("dt > 0, 0 < theta <= 1, nsteps >= 0 and 0 <= first_slot < nslots are required")
    sigma, _ = constants(dt, theta)
    X = np.array(X, dtype=np.float64)
    info = dict(steps_done=0, iterations=[], relres=[], reason=[], systems=[])
    for t in range(nsteps):
        slot = (first_slot + t) % len(values)
        W = None if theta == 1 else spmv_ref(n, n, colptr, rowval, values[slot], X, adjoint=adjoint)
        B = rhs(X, W, source, d, dt, theta)
        A = R.csc_of(n, n, colptr, rowval, values[slot])
        if next is None:
            X, si = R.solve_ref(A, B, d=d, sigma=sigma, rtol=rtol, maxiter=maxiter, x0=X, adjoint=adjoint)
        else:
            X, si = LR.solve_lines_ref(A, B, next, d=d, sigma=sigma, rtol=rtol, maxiter=maxiter, x0=X, adjoint=adjoint)
        for key in ("iterations", "relres", "reason"):
            info[key].append(si[key])
        info["systems"].append((slot, B, X.copy()))
        if not si["converged"].all():
            break
        info["steps_done"] = t + 1
    return X, info


STEP_LINE_OPS = 7  # the elementwise operations of st_line (csrc/otmb_step.hip): d·x, + w, c·e, σ·x, s/θ, + (s/θ), - c·e


def step_rhs_scale(A_slot, X_prev, S, d, dt, theta, adjoint):
    """σ·|x| + |s|/θ + ((1 - θ)/θ)·(|d|∘|x| + |A|·|x|): the magnitudes of the terms of a step's right-hand side, per entry."""
    import scipy.sparse as sp

    Aop = sp.csr_matrix(A_slot.T if adjoint else A_slot)
    X = np.abs(np.asarray(X_prev, dtype=np.float64).reshape(Aop.shape[0], -1))
    n, k = X.shape
    s = np.zeros((n, k)) if S is None else np.abs(np.asarray(S, dtype=np.float64).reshape(n, k))
    dd = np.zeros(n) if d is None else np.abs(np.asarray(d, dtype=np.float64))
    return X / (theta * dt) + s / theta + ((1.0 - theta) / theta) * (dd[:, None] * X + abs(Aop) @ X)


def step_residual_check(A_slot, X_prev, X_next, S, d, dt, theta, adjoint, rtol):
    """One θ-step checked without the library's word, per column: -> (‖b(x) - M·x⁺‖₂, bound), everything in float64 with scipy's products.

    The system is written down here from the differential equation, not from the header: the θ-method of ∂x/∂t + (diag(d) + A)·x = s is
    (x⁺ - x)/δt + θ·(diag(d) + A)·x⁺ + (1 - θ)·(diag(d) + A)·x = s; divided by θ,
        M·x⁺ = b(x),   M = I/(θ·δt) + diag(d) + A,   b(x) = x/(θ·δt) + s/θ - ((1 - θ)/θ)·(diag(d)·x + A·x)      (adjoint: Aᵀ for A).
    A_slot: the step's matrix (scipy sparse); X_prev, X_next: the states before and after it; S, d: None or arrays.

    bound = solve_ref.residual_check's for (M, x⁺, b) -- rtol·‖b‖₂ + 2·(L + 3)·ε·‖ |M|·|x⁺| + |b| ‖₂ --
            + 2·(L + c)·ε·‖ σ·|x| + |s|/θ + ((1 - θ)/θ)·(|d|∘|x| + |A|·|x|) ‖₂,   c = STEP_LINE_OPS = 7.
    The second term is what forming b twice, here and on the device, in different orders can differ by.  Its constant is counted on the code,
    not fitted: a term of b goes through the fold of its row (at most L products and L additions: relative error γ_L; only the A·x term),
    then through operations of st_line, each one rounding -- d·x: (d·x), (+ w), (c·e), (a - ce): 4;  A·x: (+ d·x), (c·e), (a - ce): 3;
    σ·x: (σ·x), (+ s/θ), (a - ce): 3;  s/θ: (s/θ), (+), (a - ce): 3 -- and carries the roundings of its constant: σ = 1/(θ·δt) two, c =
    (1 - θ)/θ two (this side may form them in another way, so they count).  The deepest term is A·x with L + 3 + 2 = L + 5 roundings, below
    L + 7 = L + the seven operations st_line has in all; so each side is within γ_{L+5}·scale ≤ (L + 7)·ε·scale entrywise (the two spare ε
    cover γ's second order and the device's rtol·‖b_device‖₂ against this side's rtol·‖b‖₂), and the two sides within twice that.  θ = 1 has
    two operations and no product: the same bound holds with room."""
    import scipy.sparse as sp

    A = sp.csc_matrix(A_slot)
    n = A.shape[0]
    Aop = (A.T if adjoint else A).tocsr()
    Xp = np.asarray(X_prev, dtype=np.float64).reshape(n, -1)
    Xn = np.asarray(X_next, dtype=np.float64).reshape(n, -1)
    sigma = 1.0 / (theta * dt)
    B = Xp / (theta * dt)
    if S is not None:
        B = B + np.asarray(S, dtype=np.float64).reshape(n, -1) / theta
    if theta != 1:
        E = Aop @ Xp
        if d is not None:
            E = E + np.asarray(d, dtype=np.float64)[:, None] * Xp
        B = B - ((1.0 - theta) / theta) * E
    scale = step_rhs_scale(A, Xp, S, d, dt, theta, adjoint)
    L = R.longest(A, adjoint)
    out = []
    for c, (res, bound) in enumerate(R.residual_check(A, Xn, B, d, sigma, adjoint, rtol)):
        out.append((res, bound + 2 * (L + STEP_LINE_OPS) * R.EPS * np.linalg.norm(scale[:, c])))
    return out
