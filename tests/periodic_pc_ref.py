"""A numpy restatement of otmb_op_combine_slots and of otmb_op_periodic_pc with OTMB_OUTER_MEAN (csrc/otmb_combine.hip, csrc/otmb_periodic.hip,
include/otmb.h), beside tests/periodic_ref.py, which it imports and leaves alone.

    combine_ref(values, w):  per entry, the slots with w[s] != 0 in ascending s: acc = w[s]·v_s, then acc = acc + w[s]·v_s; none: +0.0
    periodic_pc_column:      periodic_ref.periodic_column as flexible right-preconditioned GMRES: in iteration i
                                 Z_i = Qinv(V_i);  w = Z_i - Φ·Z_i;  CGS2 against V, the rotations and V_{i+1} as before;  x += Σ_j y_j·Z_j
                             Qinv(v) -> (z, iterations) or (None, iterations): a failing Qinv stops the column with "precond_failed" and the
                             state of its last explicit defect.  Qinv = identity has periodic_column's bits.
    mean_maps:               Qinv(v) = v + q / P, (diag(d) + Ā)·q = v by the restated BiCGStab (solve_ref / solve_lines_ref) on combine_ref's
                             values with the visit weights count_s / ncycle, P = ncycle·dt: the library's mean solve, bit for bit
    dense_qinv:              the same with a dense inverse of P·M̄
"""
import numpy as np

import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R

REASONS = PR.REASONS + ("precond_failed",)


def combine_ref(values, w):
    """Σ_s w[s]·values[s] in the fold of otmb_op_combine_slots.  values: one array per slot; w: one finite weight per slot."""
    w = np.asarray(w, dtype=np.float64)
    if len(w) != len(values) or not np.isfinite(w).all():
        raise ValueError("one finite weight per slot is required")
    acc = None
    for s in range(len(values)):
        if w[s] != 0.0:
            t = w[s] * np.asarray(values[s], dtype=np.float64)
            acc = t if acc is None else acc + t
    return np.zeros(np.shape(values[0])) if acc is None else acc


def visit_weights(nslots, ncycle, first_slot):
    """count_s / ncycle, count_s the visits of slot s by the steps first_slot .. first_slot + ncycle - 1 (one double division each)."""
    count = np.zeros(nslots)
    for t in range(ncycle):
        count[(first_slot + t) % nslots] += 1.0
    return count / float(ncycle)


def periodic_pc_column(F, Phi, Qinv, n, *, x0=None, ptol=1e-8, restart=30, maxcycles=1000, source_is_zero=False, order="numpy"):
    """periodic_ref.periodic_column with the right preconditioner Qinv(v) -> (z or None, iterations).
    -> (x, dict(cycles, defect, reason, history, msolve_iters))."""
    assert order in ("numpy", "device")
    dev = order == "device"
    sumsq = (lambda v: float(PR.device_sum(v * v))) if dev else (lambda v: float(v @ v))
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    info = dict(cycles=0, defect=float("nan"), reason="converged", history=[], msolve_iters=0)
    if source_is_zero:
        info["defect"] = 0.0
        return np.zeros(n), info
    if maxcycles < 1:
        info["reason"] = "maxcycles"
        return x, info
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
        V, Z = np.zeros((m + 1, n)), np.zeros((m, n))
        V[0] = r / beta
        Rm, cs, sn, gv = np.zeros((m + 1, m)), np.zeros(m), np.zeros(m), np.zeros(m + 1)
        gv[0] = beta
        i = 0
        while True:
            z, its = Qinv(V[i])
            info["msolve_iters"] += int(its)
            if z is None:
                info["reason"] = "precond_failed"
                return x, info
            Z[i] = z
            pv = Phi(Z[i])
            if pv is None:
                info["reason"] = "step_failed"
                return x, info
            info["cycles"] += 1
            w = Z[i] - pv
            if dev:
                h1, n1 = PR.device_dots(V[:i + 1], w)
                w = PR.device_update(V[:i + 1], h1, w)
                h2, _ = PR.device_dots(V[:i + 1], w)
                w = PR.device_update(V[:i + 1], h2, w)
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
            PR.givens_column(h, hn, cs, sn, gv, i)
            Rm[:i + 1, i] = h
            i += 1
            if abs(gv[i]) <= ptol * gnorm or i == m or hn == 0.0 or info["cycles"] + 1 >= maxcycles:
                break
            V[i] = w / hn
        if dev:
            y = PR.back_substitution(Rm, gv, i)
        else:
            y = np.zeros(i)
            for a in range(i - 1, -1, -1):
                y[a] = (gv[a] - Rm[a, a + 1:i] @ y[a + 1:]) / Rm[a, a]
        for j in range(i):  # (pd_combine_kernel on the Z block: j ascending, one product and one addition at a time)
            x = x + y[j] * Z[j]
        Fx = F(x)
        if Fx is None:
            info["reason"] = "step_failed"
            return x, info
        info["cycles"] += 1
        r = Fx - x


def periodic_pc_ref(F, Phi, Qinv, S, *, x0=None, **kw):
    """Every column of the source S (n x k) on its own.  F(c, x), Phi(c, v), Qinv(c, v): column c's maps.
    -> (X, dict(cycles, defect, reason, converged, history, msolve_iters))."""
    S = np.asarray(S, dtype=np.float64).reshape(len(S), -1)
    n, k = S.shape
    X = np.zeros((n, k), order="F")
    out = dict(cycles=[], defect=[], reason=[], history=[], msolve_iters=[])
    for c in range(k):
        start = None if x0 is None else np.asarray(x0, dtype=np.float64).reshape(n, -1)[:, c]
        X[:, c], info = periodic_pc_column(lambda x: F(c, x), lambda v: Phi(c, v), lambda v: Qinv(c, v), n, x0=start,
                                           source_is_zero=not S[:, c].any(), **kw)
        for key in out:
            out[key].append(info[key])
    out["cycles"], out["defect"], out["msolve_iters"] = np.array(out["cycles"]), np.array(out["defect"]), np.array(out["msolve_iters"])
    out["converged"] = np.array([r == "converged" for r in out["reason"]])
    return X, out


def identity(c, v):
    return v, 0


def precondition(v, q, P):
    """pd_precond_kernel: z = v + q / P, one division and one addition."""
    t = q / P
    return v + t


def mean_maps(n, colptr, rowval, values, *, dt, ncycle, first_slot, d=None, rtol=1e-10, maxiter=10000, adjoint=False, next=None):
    """Qinv for periodic_pc_ref on top of the restated solver: the mean values by combine_ref with the visit weights, one solve at σ = 0 from
    zero (next: the lines; None: Jacobi), then precondition()."""
    A = R.csc_of(n, n, colptr, rowval, combine_ref(values, visit_weights(len(values), ncycle, first_slot)))
    P = float(ncycle) * dt

    def Qinv(c, v):
        if next is None:
            q, si = R.solve_ref(A, v, d=d, sigma=0.0, rtol=rtol, maxiter=maxiter, adjoint=adjoint)
        else:
            q, si = LR.solve_lines_ref(A, v, next, d=d, sigma=0.0, rtol=rtol, maxiter=maxiter, adjoint=adjoint)
        its = int(si["iterations"][0])
        return (precondition(v, q, P) if si["converged"].all() else None), its

    return Qinv


def dense_qinv(n, colptr, rowval, values, *, dt, ncycle, first_slot, d=None, adjoint=False):
    """Qinv with a dense inverse of P·M̄, M̄ = diag(d) + Ā (adjoint: Āᵀ) over combine_ref's values.  -> (Qinv, cond(M̄))"""
    A = R.csc_of(n, n, colptr, rowval, combine_ref(values, visit_weights(len(values), ncycle, first_slot))).toarray()
    M = (A.T if adjoint else A) + np.diag(np.zeros(n) if d is None else np.asarray(d, dtype=np.float64))
    inv = np.linalg.inv((float(ncycle) * dt) * M)
    return (lambda c, v: (v + inv @ v, 0)), float(np.linalg.cond(M))
