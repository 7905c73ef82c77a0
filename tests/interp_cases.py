"""What tests/test_interp_ref.py (CPU) and tests/test_interp_periodic.py (GPU) share: the periodic cases of the interpolated cycle -- the
grids, the schedule (3 slots x 2 sub-steps by the convention), the per-column D, the sources, and the tolerances and iteration limits of
tests/test_sched_periodic.py (rtol = 1e-12, ptol = 1e-8, maxiter = 5000 and, on these grids, GMRES(40) with at most 1000 cycles, δt = a
month).  The CPU file checks that the restatement alone converges in every case within them; the GPU file then drops none."""
import numpy as np

import dk_cases as DK
import interp_ref as IR
import solve_lines_ref as LR
import step_ref as SR

RTOL, PTOL, MAXITER = 1e-12, 1e-8, 5000
RESTART, MAXCYCLES = 40, 1000
DT = SR.MONTH
GRIDS = ["odd_nx_fold", "tiny_tripolar"]
NSLOTS, SUBSTEPS = 3, 2
SCHEDULE = IR.interp_schedule(NSLOTS, SUBSTEPS)  # (2, 0, 0.75) (0, 1, 0.25) (0, 1, 0.75) (1, 2, 0.25) (1, 2, 0.75) (2, 0, 0.25)
K = 3
_CASES = {}


def case(oracle, name):
    """(N, (p, i, v, next), the three slots' values, D (N x 3: the age d, that plus λ, that plus a random column), S (N x 3: ones, a random
    column, zeros)) -- once per session.  Column 0 alone is the k = 1 case: the age system with s = 1."""
    if name not in _CASES:
        (p, i, v), N, nsurf, nxt = LR.grid(oracle, name)
        D = np.asfortranarray(DK.columns(N, nsurf, zero=False)[:, [0, 2, 3]])
        S = np.zeros((N, K), order="F")
        S[:, 0], S[:, 1] = 1.0, np.random.default_rng(61).standard_normal(N)
        _CASES[name] = (N, (p, i, v, nxt), SR.slot_values(v, seed=1), D, S)
    return _CASES[name]
