"""A numpy restatement of otmb_op_step_sched and otmb_op_periodic_sched (include/otmb.h: the schedule) on top of tests/step_ref.py:

    slot(t)  = (first_slot + t // substeps) mod nslots
    source   : nsrc blocks; nsrc = 0 none, 1 block 0 on every step, nslots the block of slot(t)
    S_eff    = S_j * scale[t]   (one multiplication per entry, before anything else touches s; without scale S_j itself)
    step t   = step_ref.step_ref(nsteps=1, first_slot=slot(t), source=S_eff) from the state step t - 1 left

and, for the periodic state, the visit counts of the slots (the cycle-mean operator's weights) and the cycle's maps F and Phi in the form
periodic_ref.periodic_ref / periodic_pc_ref.periodic_pc_ref accept.  DenseSched is the same cycle in dense numpy (an LU per visited slot),
which shares nothing with the restated solver."""
import numpy as np

import solve_ref as R
import step_ref as SR


def slot_of(t, first_slot, substeps, nslots):
    return (int(first_slot) + int(t) // int(substeps)) % int(nslots)


def source_index(nsrc, slot):
    """The block step t takes when its slot is `slot`: None without sources."""
    return None if nsrc == 0 else 0 if nsrc == 1 else slot


def s_eff(sources, scale, t, slot):
    """The source of step t (None: none).  sources: a list of blocks (n or n x k); scale: None or (nsteps, k) / (nsteps,)."""
    j = source_index(0 if sources is None else len(sources), slot)
    if j is None:
        return None
    S = np.asarray(sources[j], dtype=np.float64)
    return S if scale is None else S * np.asarray(scale, dtype=np.float64)[t]


def visit_counts(nslots, ncycle, first_slot, substeps=1):
    count = np.zeros(nslots, dtype=np.int64)
    for t in range(ncycle):
        count[slot_of(t, first_slot, substeps, nslots)] += 1
    return count


def visit_weights(nslots, ncycle, first_slot, substeps=1):
    """w[s] = count_s / ncycle, one double division each (periodic_pc_ref.visit_weights with substeps = 1)."""
    return np.array([float(c) / float(ncycle) for c in visit_counts(nslots, ncycle, first_slot, substeps)])


def sched_ref(n, colptr, rowval, values, X, *, dt, theta=1.0, nsteps=1, first_slot=0, substeps=1, sources=None, scale=None, d=None, rtol=1e-10,
              maxiter=10000, adjoint=False, next=None):
    """The chain of one-step step_ref calls.  -> (X, info) as step_ref gives them; systems holds (slot, B, X after the step) per step."""
    nsrc = 0 if sources is None else len(sources)
    if substeps < 1 or nsrc not in (0, 1, len(values)):
        raise ValueError("substeps >= 1 and 0, 1 or nslots source blocks are required")
    X = np.array(X, dtype=np.float64)
    info = dict(steps_done=0, iterations=[], relres=[], reason=[], systems=[])
    for t in range(nsteps):
        slot = slot_of(t, first_slot, substeps, len(values))
        X, one = SR.step_ref(n, colptr, rowval, values, X, dt=dt, theta=theta, nsteps=1, first_slot=slot, source=s_eff(sources, scale, t, slot), d=d,
                             rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        for key in ("iterations", "relres", "reason", "systems"):
            info[key].append(one[key][0])
        if one["steps_done"] != 1:
            break
        info["steps_done"] = t + 1
    return X, info


def all_blocks(sources):
    """|S_0| + |S_1| + ...: zero exactly where a column is zero in every block (periodic_ref's test for a zero source)."""
    return sum(np.abs(np.asarray(S, dtype=np.float64).reshape(len(S), -1)) for S in sources)


def cycle_maps(n, colptr, rowval, values, sources, *, dt, theta, ncycle, first_slot, substeps=1, d=None, rtol=1e-10, maxiter=10000, adjoint=False,
               next=None):
    """(F, Phi) for periodic_ref / periodic_pc_ref on top of sched_ref: F(c, x) the scheduled cycle with column c of every block, Phi(c, v)
    the same without sources; None when a step fails."""
    blocks = [np.asarray(S, dtype=np.float64).reshape(n, -1) for S in sources]

    def run(x, src):
        X, info = sched_ref(n, colptr, rowval, values, x.reshape(n, 1), dt=dt, theta=theta, nsteps=ncycle, first_slot=first_slot, substeps=substeps,
                            sources=src, d=d, rtol=rtol, maxiter=maxiter, adjoint=adjoint, next=next)
        return X[:, 0] if info["steps_done"] == ncycle else None

    return (lambda c, x: run(x, [S[:, c:c + 1] for S in blocks])), (lambda c, v: run(v, None))


def mean_values(values, ncycle, first_slot, substeps=1):
    """The cycle-mean values: otmb_op_combine_slots' fold (periodic_pc_ref.combine_ref) with the schedule's visit weights."""
    import periodic_pc_ref as PC

    return PC.combine_ref(values, visit_weights(len(values), ncycle, first_slot, substeps))


def dense_qinv(n, colptr, rowval, values, *, dt, ncycle, first_slot, substeps=1, d=None, adjoint=False):
    """Qinv for periodic_pc_ref with a dense inverse of P·M̄, M̄ = diag(d) + Ā (adjoint: Āᵀ) over mean_values, P = ncycle·δt."""
    A = R.csc_of(n, n, colptr, rowval, mean_values(values, ncycle, first_slot, substeps)).toarray()
    M = (A.T if adjoint else A) + np.diag(np.zeros(n) if d is None else np.asarray(d, dtype=np.float64))
    inv = np.linalg.inv((float(ncycle) * dt) * M)
    return lambda c, v: (v + inv @ v, 0)


class DenseSched:
    """The scheduled cycle in dense numpy: step t solves M_t·x⁺ = N_t·x + s_t/θ with M_t = σ·I + diag(d) + A_t, N_t = σ·I - ((1 - θ)/θ)·(diag(d)
    + A_t) (adjoint: A_tᵀ), A_t the matrix of slot(t) and s_t the block of slot(t).  Phi: the n x n matrix of the source-free cycle."""

    def __init__(self, n, colptr, rowval, values, *, dt, theta, ncycle, first_slot, substeps=1, d=None, adjoint=False):
        import scipy.linalg as sla

        self.n, self.theta, self.sigma, self._sla = n, float(theta), 1.0 / (theta * dt), sla
        c = (1.0 - theta) / theta
        dd = np.zeros(n) if d is None else np.asarray(d, dtype=np.float64)
        made, self.steps = {}, []
        for t in range(ncycle):
            slot = slot_of(t, first_slot, substeps, len(values))
            if slot not in made:
                A = R.csc_of(n, n, colptr, rowval, values[slot]).toarray()
                E = np.diag(dd) + (A.T if adjoint else A)
                made[slot] = (sla.lu_factor(self.sigma * np.eye(n) + E), self.sigma * np.eye(n) - c * E)
            self.steps.append((slot,) + made[slot])
        Phi = np.eye(n)
        for _, lu, N in self.steps:
            Phi = sla.lu_solve(lu, N @ Phi)
        self.Phi = Phi

    def F(self, X, sources=None, rhs_norms=None):
        """The cycle from X (n x k) with the blocks `sources` (None: none); rhs_norms: a list that receives ‖b_t‖₂ per column and step."""
        X = np.asarray(X, dtype=np.float64)
        for slot, lu, N in self.steps:
            B = N @ X
            j = source_index(0 if sources is None else len(sources), slot)
            if j is not None:
                B = B + np.asarray(sources[j], dtype=np.float64).reshape(X.shape) / self.theta
            if rhs_norms is not None:
                rhs_norms.append(np.linalg.norm(B.reshape(self.n, -1), axis=0))
            X = self._sla.lu_solve(lu, B)
        return X

    def fixed_point(self, sources):
        """(x* = (I - Φ)⁻¹·g, ‖g‖₂ per column, ‖(I - Φ)⁻¹‖₂, max_t ‖b_t‖₂ per column along the cycle from x*) for blocks of n x k."""
        blocks = [np.asarray(S, dtype=np.float64).reshape(self.n, -1) for S in sources]
        G = self.F(np.zeros_like(blocks[0]), blocks)
        I = np.eye(self.n) - self.Phi
        xs = np.linalg.solve(I, G)
        norms = []
        self.F(xs, blocks, norms)
        return xs, np.linalg.norm(G, axis=0), 1.0 / np.linalg.svd(I, compute_uv=False)[-1], np.max(norms, axis=0)
