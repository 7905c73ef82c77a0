"""A numpy restatement of otmb_op_step_interp and otmb_op_periodic_interp (include/otmb.h: matrices interpolated between slots) on top of
tests/step_ref.py, tests/periodic_pc_ref.py (combine_ref), tests/periodic_ref.py and tests/sched_ref.py:

    step t, a = slot_a[t], b = slot_b[t], w = weight[t]
      plain on a    when a == b or w == 0.0
      plain on b    when w == 1.0
      blended       otherwise:  values = combine_ref with 1.0 - w at a, w at b, zero elsewhere  (pa = wa·va, pb = w·vb, v = pa + pb)
    step t        = step_ref.step_ref(nsteps=1) on that one value set, source S·scale[t], from the state step t - 1 left
    mean weights  = acc_s / ncycle, acc over t ascending: a plain step adds 1.0 to its slot, a blended one 1.0 - w to a, then w to b

and interp_schedule, the convention's integer rule (api.interp_schedule is compared with it and with fractions.Fraction in
tests/test_interp_ref.py).  DenseInterp is one cycle in dense numpy with an LU per step, which shares nothing with the restated solver."""
import numpy as np

import periodic_pc_ref as PC
import sched_ref as SC
import solve_ref as R
import step_ref as SR

AT = {"start": 0, "mid": 1, "end": 2}


def interp_schedule(nslots, substeps, *, ncycles=1, first_slot=0, at="mid"):
    """The rule in Python integers, one step at a time.  -> (slot_a, slot_b, weight)"""
    m = int(substeps)
    a, b, w = [], [], []
    for t in range(ncycles * nslots * m):
        g = 2 * t + AT[at] - m + 2 * m * nslots
        a.append((first_slot + g // (2 * m)) % nslots)
        b.append((a[-1] + 1) % nslots)
        w.append(float(g % (2 * m)) / float(2 * m))
    return np.array(a, dtype=np.int64), np.array(b, dtype=np.int64), np.array(w, dtype=np.float64)


def kind(a, b, w):
    """-> ("plain", slot) or ("blend", None)."""
    if a == b or w == 0.0:
        return "plain", int(a)
    if w == 1.0:
        return "plain", int(b)
    return "blend", None


def prec_blocks(kinds):
    """The preconditioners a call keeps for steps of these kinds: one per slot its plain steps visit, and one that every blended step shares."""
    return len({slot for what, slot in kinds if what == "plain"}) + int(any(what == "blend" for what, _ in kinds))


def combine_weights(nslots, a, b, w):
    """The weights of the chain's combine_slots call for a blended step: 1.0 - w at a, w at b, zero elsewhere."""
    wt = np.zeros(nslots)
    wt[a], wt[b] = 1.0 - float(w), float(w)
    return wt


def step_values(values, a, b, w):
    """The value set of step (a, b, w): the slot's own array when the step is plain, the blend otherwise."""
    what, slot = kind(a, b, w)
    return values[slot] if what == "plain" else PC.combine_ref(values, combine_weights(len(values), a, b, w))


def mean_weights(nslots, slot_a, slot_b, weight):
    acc = [0.0] * nslots
    for a, b, w in zip(slot_a, slot_b, weight):
        what, slot = kind(a, b, w)
        if what == "plain":
            acc[slot] = acc[slot] + 1.0
        else:
            wa = 1.0 - float(w)
            acc[a] = acc[a] + wa
            acc[b] = acc[b] + float(w)
    return np.array([x / float(len(weight)) for x in acc])


def interp_ref(n, colptr, rowval, values, X, *, dt, slot_a, slot_b, weight, theta=1.0, source=None, scale=None, d=None, rtol=1e-10, maxiter=10000,
               adjoint=False, next=None):
    """The chain of one-step step_ref calls, each on its step's value set.  -> (X, info) as step_ref gives them; systems holds (the step's
    values, B, X after the step)."""
    X = np.array(X, dtype=np.float64)
    info = dict(steps_done=0, iterations=[], relres=[], reason=[], systems=[])
    for t, (a, b, w) in enumerate(zip(slot_a, slot_b, weight)):
        vals = step_values(values, int(a), int(b), float(w))
        X, one = SR.step_ref(n, colptr, rowval, [vals], X, dt=dt, theta=theta, nsteps=1, first_slot=0,
                             source=SC.s_eff(None if source is None else [source], scale, t, 0), d=d, rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        for key in ("iterations", "relres", "reason"):
            info[key].append(one[key][0])
        info["systems"].append((vals, one["systems"][0][1], one["systems"][0][2]))
        if one["steps_done"] != 1:
            break
        info["steps_done"] = t + 1
    return X, info


def cycle_maps(n, colptr, rowval, values, S, *, dt, theta, slot_a, slot_b, weight, d=None, rtol=1e-10, maxiter=10000, adjoint=False, next=None):
    """(F, Phi) for periodic_ref / periodic_pc_ref: F(c, x) the interpolated cycle with column c of S, Phi(c, v) the same without a source;
    None when a step fails.  d: n values, or n x k (column c's own)."""
    S = np.asarray(S, dtype=np.float64).reshape(n, -1)
    dcol = (lambda c: d) if d is None or np.ndim(d) == 1 else (lambda c: np.asarray(d)[:, c])

    def run(c, x, src):
        X, info = interp_ref(n, colptr, rowval, values, x.reshape(n, 1), dt=dt, theta=theta, slot_a=slot_a, slot_b=slot_b, weight=weight, source=src,
                             d=dcol(c), rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        return X[:, 0] if info["steps_done"] == len(weight) else None

    return (lambda c, x: run(c, x, S[:, c:c + 1])), (lambda c, v: run(c, v, None))


def mean_values(values, slot_a, slot_b, weight):
    return PC.combine_ref(values, mean_weights(len(values), slot_a, slot_b, weight))


def dense_qinv(n, colptr, rowval, values, *, dt, slot_a, slot_b, weight, d=None, adjoint=False):
    """Qinv for periodic_pc_ref with a dense inverse of P·M̄ over mean_values, P = ncycle·δt; d: n values or n x k."""
    A = R.csc_of(n, n, colptr, rowval, mean_values(values, slot_a, slot_b, weight)).toarray()
    A = A.T if adjoint else A
    made = {}

    def qinv(c, v):
        key = 0 if d is None or np.ndim(d) == 1 else c
        if key not in made:
            dd = np.zeros(n) if d is None else np.asarray(d, dtype=np.float64) if np.ndim(d) == 1 else np.asarray(d, dtype=np.float64)[:, c]
            made[key] = np.linalg.inv((float(len(weight)) * dt) * (A + np.diag(dd)))
        return v + made[key] @ v, 0

    return qinv


class DenseInterp:
    """One interpolated cycle in dense numpy, in the manner of sched_ref.DenseSched: step t solves M_t·x⁺ = N_t·x + s/θ with M_t = σ·I + diag(d) +
    A_t, N_t = σ·I - ((1 - θ)/θ)·(diag(d) + A_t) (adjoint: A_tᵀ), A_t = (1 - w)·A_a + w·A_b formed densely, an LU per step."""

    def __init__(self, n, colptr, rowval, values, *, dt, theta, slot_a, slot_b, weight, d=None, adjoint=False):
        import scipy.linalg as sla

        self.n, self.theta, self.sigma, self._sla = n, float(theta), 1.0 / (theta * dt), sla
        c = (1.0 - theta) / theta
        dd = np.zeros(n) if d is None else np.asarray(d, dtype=np.float64)
        dense = [R.csc_of(n, n, colptr, rowval, v).toarray() for v in values]
        self.steps = []
        for a, b, w in zip(slot_a, slot_b, weight):
            A = (1.0 - float(w)) * dense[int(a)] + float(w) * dense[int(b)]
            E = np.diag(dd) + (A.T if adjoint else A)
            self.steps.append((sla.lu_factor(self.sigma * np.eye(n) + E), self.sigma * np.eye(n) - c * E))

    def F(self, X, source=None, rhs_norms=None):
        X = np.asarray(X, dtype=np.float64)
        for lu, N in self.steps:
            B = N @ X
            if source is not None:
                B = B + np.asarray(source, dtype=np.float64).reshape(X.shape) / self.theta
            if rhs_norms is not None:
                rhs_norms.append(np.linalg.norm(B.reshape(self.n, -1), axis=0))
            X = self._sla.lu_solve(lu, B)
        return X
