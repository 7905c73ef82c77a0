"""What tests/test_season_ref.py (CPU) and tests/test_season_periodic.py (GPU) share: the periodic cases of the cycle whose d and source
follow the slots.  The grids, the three slots, D, S, the tolerances and the iteration limits are tests/interp_cases.py's; slot s has
D_s = D·DSCALE[s] and S_s = S·SSCALE[s] (an ice cover that scales the restoring rate and the source); the schedules are the convention's
six blended steps and the plain 3 x 2 schedule.  CASES lists what the GPU file runs, each at k = 3 and for column 0 alone: θ = 1 on both
grids with both outer iterations, θ = 0.5 with both on odd_nx_fold and with outer = "mean" only on tiny_tripolar (the unpreconditioned
iteration takes 733 cycles there, which no test of a few seconds affords).  The CPU file shows that each of them converges in the
restatement alone, in numpy's and in the device's order of sums; the GPU file then drops none."""
import numpy as np

import interp_cases as IC

DSCALE, SSCALE = (1.0, 0.5, 0.125), (1.0, 0.5, 1.5)
_PLAIN = np.repeat(np.arange(IC.NSLOTS, dtype=np.int64), IC.SUBSTEPS)
SCHEDULES = {"blended": IC.SCHEDULE, "plain": (_PLAIN, _PLAIN.copy(), np.zeros(len(_PLAIN)))}
CASES = [(name, theta, outer) for name in IC.GRIDS for theta in (1.0, 0.5) for outer in ("none", "mean")
         if not (name == "tiny_tripolar" and theta == 0.5 and outer == "none")]


def case(oracle, name):
    """(N, (p, i, v, next), the three slots' values, the three D blocks (N x 3 each), the three S blocks (N x 3 each, the third column zero))"""
    N, pattern, values, D, S = IC.case(oracle, name)
    return N, pattern, values, [np.asfortranarray(D * f) for f in DSCALE], [np.asfortranarray(S * f) for f in SSCALE]


def columns(blocks, k):
    """The blocks as the k = 3 call takes them (k = 3), or column 0 alone as n values each (k = 1)."""
    return list(blocks) if k == 3 else [np.ascontiguousarray(b[:, 0]) for b in blocks]
