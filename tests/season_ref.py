"""A numpy restatement of otmb_op_step_season and otmb_op_periodic_season (include/otmb.h: d and the source per slot, blended with the
matrices) on top of tests/step_ref.py, tests/interp_ref.py (kind, step_values, mean_weights) and tests/periodic_pc_ref.py (combine_ref):

    the field of step t (a, b, w), given as a list of blocks
      one block      the block as it is, on every step (never blended with itself)
      per slot       plain step: the slot's block;  blended step: wa = 1.0 - w;  pa = wa * xa;  pb = w * xb;  x = pa + pb
    step t         = step_ref.step_ref(nsteps=1) on interp_ref.step_values, with d_t and s_t·scale[t], from the state step t - 1 left
    d̄              = combine_ref over the d blocks with interp_ref.mean_weights (one block: that block)

DenseSeason is one cycle in dense numpy with an LU per step, d_t and s_t formed densely; it shares nothing with the restated solver."""
import numpy as np

import interp_ref as IR
import periodic_pc_ref as PC
import solve_ref as R
import step_ref as SR


def field(blocks, a, b, w):
    """The field of step (a, b, w); blocks: None or a list of one or nslots arrays."""
    if blocks is None:
        return None
    if len(blocks) == 1:
        return blocks[0]
    what, slot = IR.kind(int(a), int(b), float(w))
    if what == "plain":
        return blocks[slot]
    wa = 1.0 - float(w)
    pa = wa * np.asarray(blocks[int(a)], dtype=np.float64)
    pb = float(w) * np.asarray(blocks[int(b)], dtype=np.float64)
    return pa + pb


def source_of(sources, scale, t, a, b, w):
    """s_t: the field, then the step's scale (None: none)."""
    s = field(sources, a, b, w)
    return s if s is None or scale is None else s * np.asarray(scale, dtype=np.float64)[t]


def column(blocks, c):
    """Column c's own blocks: n values serve every column, an n x k block gives its column c."""
    return None if blocks is None else [b if np.ndim(b) == 1 else np.ascontiguousarray(np.asarray(b)[:, c]) for b in blocks]


def season_ref(n, colptr, rowval, values, X, *, dt, slot_a, slot_b, weight, theta=1.0, d=None, sources=None, scale=None, rtol=1e-10, maxiter=10000,
               adjoint=False, next=None):
    """The chain of one-step step_ref calls; d: None or a list of blocks of n values.  -> (X, info) as interp_ref.interp_ref gives them."""
    X = np.array(X, dtype=np.float64)
    info = dict(steps_done=0, iterations=[], relres=[], reason=[], systems=[])
    for t, (a, b, w) in enumerate(zip(slot_a, slot_b, weight)):
        vals = IR.step_values(values, int(a), int(b), float(w))
        X, one = SR.step_ref(n, colptr, rowval, [vals], X, dt=dt, theta=theta, nsteps=1, first_slot=0, source=source_of(sources, scale, t, a, b, w),
                             d=field(d, a, b, w), rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        for key in ("iterations", "relres", "reason"):
            info[key].append(one[key][0])
        info["systems"].append((vals, one["systems"][0][1], one["systems"][0][2]))
        if one["steps_done"] != 1:
            break
        info["steps_done"] = t + 1
    return X, info


def cycle_maps(n, colptr, rowval, values, sources, *, dt, theta, slot_a, slot_b, weight, d=None, rtol=1e-10, maxiter=10000, adjoint=False, next=None):
    """(F, Phi) for periodic_ref / periodic_pc_ref: F(c, x) the cycle with column c of every source block and of every d block, Phi(c, v) the
    same without sources; None when a step fails."""
    sources = [np.asarray(S, dtype=np.float64).reshape(n, -1) for S in sources]

    def run(c, x, src):
        X, info = season_ref(n, colptr, rowval, values, x.reshape(n, 1), dt=dt, theta=theta, slot_a=slot_a, slot_b=slot_b, weight=weight, sources=src,
                             d=column(d, c), rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        return X[:, 0] if info["steps_done"] == len(weight) else None

    return (lambda c, x: run(c, x, [S[:, c:c + 1] for S in sources])), (lambda c, v: run(c, v, None))


def dbar(d, slot_a, slot_b, weight):
    """d̄ of OTMB_OUTER_MEAN: the given block when there is one, the fold of combine_slots under the mean's weights otherwise."""
    if d is None:
        return None
    return d[0] if len(d) == 1 else PC.combine_ref(d, IR.mean_weights(len(d), slot_a, slot_b, weight))


def dense_qinv(n, colptr, rowval, values, *, dt, slot_a, slot_b, weight, d=None, adjoint=False):
    """interp_ref.dense_qinv over diag(d̄) + Ā."""
    return IR.dense_qinv(n, colptr, rowval, values, dt=dt, slot_a=slot_a, slot_b=slot_b, weight=weight, d=dbar(d, slot_a, slot_b, weight), adjoint=adjoint)


class DenseSeason:
    """One cycle in dense numpy: step t solves M_t·x⁺ = N_t·x + s_t/θ with M_t = σ·I + diag(d_t) + A_t, N_t = σ·I - ((1 - θ)/θ)·(diag(d_t) + A_t)
    (adjoint: A_tᵀ); A_t, d_t and s_t are (1 - w)·(a's) + w·(b's) formed densely in one expression each, an LU per step.  d: a list of
    blocks of n values; sources: a list of n x k blocks."""

    def __init__(self, n, colptr, rowval, values, *, dt, theta, slot_a, slot_b, weight, d=None, sources=None, adjoint=False):
        import scipy.linalg as sla

        self.n, self.theta, self.sigma, self._sla = n, float(theta), 1.0 / (theta * dt), sla
        c = (1.0 - theta) / theta
        dense = [R.csc_of(n, n, colptr, rowval, v).toarray() for v in values]

        def mix(blocks, a, b, w):
            if blocks is None:
                return None
            if len(blocks) == 1:
                return np.asarray(blocks[0], dtype=np.float64)
            return (1.0 - w) * np.asarray(blocks[a], dtype=np.float64) + w * np.asarray(blocks[b], dtype=np.float64)

        self.steps = []
        for a, b, w in zip(slot_a, slot_b, weight):
            a, b, w = int(a), int(b), float(w)
            A = (1.0 - w) * dense[a] + w * dense[b]
            dt_ = mix(d, a, b, w)
            E = (A.T if adjoint else A) + (0.0 if dt_ is None else np.diag(dt_))
            self.steps.append((sla.lu_factor(self.sigma * np.eye(n) + E), self.sigma * np.eye(n) - c * E, mix(sources, a, b, w)))

    def F(self, X, rhs_norms=None):
        X = np.asarray(X, dtype=np.float64)
        for lu, N, s in self.steps:
            B = N @ X
            if s is not None:
                B = B + s.reshape(X.shape) / self.theta
            if rhs_norms is not None:
                rhs_norms.append(np.linalg.norm(B.reshape(self.n, -1), axis=0))
            X = self._sla.lu_solve(lu, B)
        return X
