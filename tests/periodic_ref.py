"""A numpy restatement of otmb_op_periodic (csrc/otmb_periodic.hip, include/otmb.h): the periodic state x = F(x) of the stepped cycle,
F(x) = step(x, nsteps = ncycle, first_slot, source), by restarted GMRES on the cycle map, column by column,

    F(x) = Φ·x + g:  Φ·v = the cycle without the source, g = F(0)
    r = F(x) - x, β = ‖r‖;  accepted when β <= ptol·‖g‖ (only on this explicit value);  V_0 = r/β
    iteration i:  w = V_i - Φ·V_i;  h' = Vᵀ·w, w -= V·h';  h'' = Vᵀ·w, w -= V·h'' (CGS2);  H(0..i, i) = h' + h'', H(i+1, i) = ‖w‖;
                  the Givens rotations;  the recursive residual |γ_{i+1}|;  V_{i+1} = w/‖w‖
    at |γ| <= ptol·‖g‖, at i + 1 = restart, at ‖w‖ = 0 and when one cycle of maxcycles is left:  x += V·y, then r = F(x) - x explicitly
    an iteration is begun only when a verifying cycle can follow it: cycles + 2 <= maxcycles

`cycles` counts the cycle calls (step calls) a column takes part in; with a start, F(x) and g come from ONE call of two columns.  The cycle
itself is a pair of callables (cycle_maps: tests/step_ref.py's step_ref, the restated step; dense_cycle: numpy's dense solves of the same
systems, which is what the tests afford for whole convergence histories).  device_dots / device_update restate the ORDER of the device's
sums (a lane's rows, the workgroup's tree, the fold over workgroups): the host program of tests/test_periodic_host.py gives their bits.
With order="device" the whole iteration runs in that order, and over the device's own step() as the cycle it has otmb_op_periodic's bits
(tests/test_periodic_rows.py)."""
import numpy as np

import solve_ref as R
import step_ref as SR

REASONS = ("converged", "maxcycles", "step_failed", "nonfinite")
PD_ROWS = 2048  # csrc/otmb_periodic.hip


def givens_column(h, hn, cs, sn, gv, i):
    """Column i of the Hessenberg matrix -- h = H(0..i, i), hn = H(i + 1, i) = ‖w‖ -- becomes column i of the triangle, in place: the old
    rotations, then the one that clears hn (cs[i], sn[i]; nothing to clear: the identity), applied to the rotated right-hand side gv as
    well.  GmresLsq::push of csrc/otmb_gmres.h in its order; tests/test_gmres_host.py compares the two bit for bit."""
    for j in range(i):
        t = cs[j] * h[j] + sn[j] * h[j + 1]
        h[j + 1] = cs[j] * h[j + 1] - sn[j] * h[j]
        h[j] = t
    rr = float(np.hypot(h[i], hn))
    cs[i], sn[i] = (h[i] / rr, hn / rr) if rr > 0 else (1.0, 0.0)
    h[i] = rr
    gv[i + 1] = -(sn[i] * gv[i])
    gv[i] = cs[i] * gv[i]


def back_substitution(Rm, gv, i):
    """y (i entries) from the triangle Rm[:i, :i] and the rotated right-hand side gv, term by term in GmresLsq::solve's order: s = s - R·y[b],
    b ascending, then the division (numpy's `@` adds in another order and does not agree).  tests/test_gmres_host.py compares the two bit
    for bit."""
    y = np.zeros(i)
    for a in range(i - 1, -1, -1):
        s = gv[a]
        for b in range(a + 1, i):
            t = Rm[a, b] * y[b]
            s = s - t
        y[a] = s / Rm[a, a]
    return y


def periodic_column(F, Phi, n, *, x0=None, ptol=1e-8, restart=30, maxcycles=1000, source_is_zero=False, order="numpy"):
    """One column.  F(x) -> F(x) or None (an inner step did not converge), Phi(v) likewise.
    -> (x, dict(cycles, defect, reason, history)): history = the explicit defects in order.
    order = "numpy": the sums are numpy's (`@`: the order belongs to the BLAS of the machine).  order = "device": every floating-point
    operation in csrc/otmb_periodic.hip's and GmresLsq's order -- the sums by device_sum / device_dots, the updates by device_update, the
    back substitution term by term, everything else elementwise -- so that on the same F and Phi the result has the library's bits."""
    assert order in ("numpy", "device")
    dev = order == "device"
    sumsq = (lambda v: float(device_sum(v * v))) if dev else (lambda v: float(v @ v))
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    info = dict(cycles=0, defect=float("nan"), reason="converged", history=[])
    if source_is_zero:
        info["defect"] = 0.0
        return np.zeros(n), info
    if maxcycles < 1:
        info["reason"] = "maxcycles"
        return x, info
    # the first call: F(x) and, with a start, g beside it
    Fx = F(x)
    g = Fx if x0 is None else F(np.zeros(n))
    if Fx is None or g is None:
        info["reason"] = "step_failed"
        return x, info
    info["cycles"] = 1
    gnorm = float(np.sqrt(sumsq(g)))
    if gnorm == 0.0:
        info["defect"] = 0.0
        return np.zeros(n), info
    if not np.isfinite(gnorm):
        info["reason"] = "nonfinite"
        return x, info
    r = Fx - x
    m = int(restart)
    while True:
        beta = float(np.sqrt(sumsq(r)))
        info["defect"] = beta / gnorm
        info["history"].append(info["defect"])
        if not np.isfinite(beta):
            info["reason"] = "nonfinite"
            return x, info
        if beta <= ptol * gnorm:
            return x, info
        if info["cycles"] + 2 > maxcycles:
            info["reason"] = "maxcycles"
            return x, info
        V = np.zeros((m + 1, n))
        V[0] = r / beta
        Rm, cs, sn, gv = np.zeros((m + 1, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1)
        gv[0] = beta
        i = 0
        while True:
            pv = Phi(V[i])
            if pv is None:
                info["reason"] = "step_failed"
                return x, info
            info["cycles"] += 1
            w = V[i] - pv
            if dev:  # CGS2 as the kernels run it; ‖w‖² of the first pass is read for finiteness only (GmresLsq::push)
                h1, n1 = device_dots(V[:i + 1], w)
                w = device_update(V[:i + 1], h1, w)
                h2, _ = device_dots(V[:i + 1], w)
                w = device_update(V[:i + 1], h2, w)
                n2 = sumsq(w)
            else:
                h1 = V[:i + 1] @ w
                w = w - h1 @ V[:i + 1]
                h2 = V[:i + 1] @ w
                w = w - h2 @ V[:i + 1]
                n1, n2 = 0.0, float(w @ w)
            hn = float(np.sqrt(n2))
            h = h1 + h2
            if not (np.isfinite(h).all() and np.isfinite(n1) and np.isfinite(n2)):
                info["reason"] = "nonfinite"
                return x, info
            givens_column(h, hn, cs, sn, gv, i)
            Rm[:i + 1, i] = h
            i += 1
            if abs(gv[i]) <= ptol * gnorm or i == m or hn == 0.0 or info["cycles"] + 1 >= maxcycles:
                break
            V[i] = w / hn
        if dev:
            y = back_substitution(Rm, gv, i)
        else:
            y = np.zeros(i)
            for a in range(i - 1, -1, -1):
                y[a] = (gv[a] - Rm[a, a + 1:i] @ y[a + 1:]) / Rm[a, a]
        for j in range(i):  # (pd_combine_kernel: j ascending, one product and one addition at a time)
            x = x + y[j] * V[j]
        Fx = F(x)
        if Fx is None:
            info["reason"] = "step_failed"
            return x, info
        info["cycles"] += 1
        r = Fx - x


def periodic_ref(F, Phi, S, *, x0=None, **kw):
    """Every column of the source S (n x k) on its own.  F(c, x), Phi(c, v): column c's maps.
    -> (X, dict(cycles, defect, reason, converged, history))."""
    S = np.asarray(S, dtype=np.float64).reshape(len(S), -1)
    n, k = S.shape
    X = np.zeros((n, k), order="F")
    out = dict(cycles=[], defect=[], reason=[], history=[])
    for c in range(k):
        start = None if x0 is None else np.asarray(x0, dtype=np.float64).reshape(n, -1)[:, c]
        X[:, c], info = periodic_column(lambda x: F(c, x), lambda v: Phi(c, v), n, x0=start, source_is_zero=not S[:, c].any(), **kw)
        for key in out:
            out[key].append(info[key])
    out["cycles"], out["defect"] = np.array(out["cycles"]), np.array(out["defect"])
    out["converged"] = np.array([r == "converged" for r in out["reason"]])
    return X, out


def cycle_maps(n, colptr, rowval, values, S, *, dt, theta, ncycle, first_slot, d=None, rtol=1e-10, maxiter=10000, adjoint=False, next=None):
    """(F, Phi) for periodic_ref on top of step_ref.step_ref, the restated step."""
    S = np.asarray(S, dtype=np.float64).reshape(n, -1)

    def run(x, s):
        X, info = SR.step_ref(n, colptr, rowval, values, x.reshape(n, 1), dt=dt, theta=theta, nsteps=ncycle, first_slot=first_slot,
                              source=None if s is None else s.reshape(n, 1), d=d, rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        return X[:, 0] if info["steps_done"] == ncycle else None

    return (lambda c, x: run(x, S[:, c])), (lambda c, v: run(v, None))


class DenseCycle:
    """The cycle map in dense numpy: step t solves M_t·x⁺ = N_t·x + s/θ with M_t = σ·I + diag(d) + A_t and N_t = σ·I - ((1 - θ)/θ)·(diag(d)
    + A_t) (adjoint: A_tᵀ), A_t the matrix of slot (first_slot + t) mod nslots.  Phi: the n x n matrix of the source-free cycle."""

    def __init__(self, n, colptr, rowval, values, *, dt, theta, ncycle, first_slot, d=None, adjoint=False):
        import scipy.linalg as sla

        self.n, self.theta, self.sigma = n, float(theta), 1.0 / (theta * dt)
        c = (1.0 - theta) / theta
        dd = np.zeros(n) if d is None else np.asarray(d, dtype=np.float64)
        made = {}
        self.steps = []
        for t in range(ncycle):
            slot = (first_slot + t) % len(values)
            if slot not in made:
                A = R.csc_of(n, n, colptr, rowval, values[slot]).toarray()
                A = A.T if adjoint else A
                E = np.diag(dd) + A
                made[slot] = (sla.lu_factor(self.sigma * np.eye(n) + E), self.sigma * np.eye(n) - c * E)
            self.steps.append(made[slot])
        self._sla = sla
        Phi = np.eye(n)
        for lu, N in self.steps:
            Phi = sla.lu_solve(lu, N @ Phi)
        self.Phi = Phi

    def F(self, X, S=None):
        """The cycle from X (n or n x k) with the source S (None: none)."""
        X = np.asarray(X, dtype=np.float64)
        for lu, N in self.steps:
            B = N @ X
            if S is not None:
                B = B + np.asarray(S, dtype=np.float64) / self.theta
            X = self._sla.lu_solve(lu, B)
        return X

    def rhs_norms(self, X, S):
        """max over the cycle's steps of ‖b_t‖₂ per column, along the cycle from X."""
        X = np.asarray(X, dtype=np.float64).reshape(self.n, -1)
        S = np.asarray(S, dtype=np.float64).reshape(self.n, -1)
        top = np.zeros(X.shape[1])
        for lu, N in self.steps:
            B = N @ X + S / self.theta
            top = np.maximum(top, np.linalg.norm(B, axis=0))
            X = self._sla.lu_solve(lu, B)
        return top

    def fixed_point(self, S):
        """(x*, ‖g‖₂ per column, ‖(I - Φ)⁻¹‖₂) for the source S (n x k)."""
        S = np.asarray(S, dtype=np.float64).reshape(self.n, -1)
        G = self.F(np.zeros_like(S), S)
        I = np.eye(self.n) - self.Phi
        return np.linalg.solve(I, G), np.linalg.norm(G, axis=0), 1.0 / np.linalg.svd(I, compute_uv=False)[-1]

    def maps(self, S):
        """(F, Phi) for periodic_ref."""
        S = np.asarray(S, dtype=np.float64).reshape(self.n, -1)
        return (lambda c, x: self.F(x, S[:, c])), (lambda c, v: self.F(v))


# ---- the order of the device's sums ------------------------------------------------------------------------------------------------------
def _lanes(prod):
    """Per workgroup and lane, the accumulator of pd_dots_lane over the products prod (n): pairs t, t + 256, ... of the workgroup's
    PD_ROWS rows, each pair's two rows in order.  -> (workgroups, 256).  (Rows past n add +0.0, which changes no bit of a sum that began
    at +0.0.)"""
    n = len(prod)
    nwg = (n + PD_ROWS - 1) // PD_ROWS
    p = np.zeros(nwg * PD_ROWS)
    p[:n] = prod
    p = p.reshape(nwg, PD_ROWS // 512, 256, 2)
    acc = np.zeros((nwg, 256))
    for q in range(PD_ROWS // 512):
        acc = acc + p[:, q, :, 0]
        acc = acc + p[:, q, :, 1]
    return acc


def _workgroup(acc):
    """op_block_sum (csrc/otmb_op_sum.h): xor shuffles inside each wave of 64, then the four waves in order.  (workgroups, 256) -> (workgroups,)"""
    x = acc.reshape(-1, 4, 64)
    lane = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        x = x + x[:, :, lane ^ dist]
    s = x[:, :, 0]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def _fold(part):
    s = part[0]
    for b in part[1:]:
        s = s + b
    return s


def device_sum(prod):
    """Σ prod in the device's order."""
    return _fold(_workgroup(_lanes(np.asarray(prod, dtype=np.float64))))


def device_dots(V, w):
    """(V_j·w for every row j of V, ‖w‖²) as pd_dots_kernel and pd_fold_kernel add them."""
    return np.array([device_sum(v * w) for v in V]), device_sum(w * w)


def device_update(V, h, w):
    """w - Σ_j h_j·V_j, j ascending, one product and one subtraction at a time (pd_update_kernel)."""
    w = np.array(w, dtype=np.float64)
    for hj, v in zip(h, V):
        w = w - hj * v
    return w
