"""GPU: the ladder of step and periodic exports on ONE operator.  Every family is the one loop of csrc/otmb_step.hip reached with another
call record, so where their arguments say the same thing -- seven steps from slot 1 through three slots, one d, one source -- they give
the same bits: step, step_sched(substeps=1, a list of one block), step_interp(plain_schedule), step_season(one block each); and periodic,
periodic_sched, periodic_interp, periodic_season over a cycle of three steps.  n = 301 with one row of 290 entries (longer than a slice
takes: the long-row kernels), k = 7 (register blocks 4, 2 and 1)."""
import numpy as np
import pytest
import scipy.sparse as sp

import dk_cases as DK
import solve_lines_ref as LR
import step_ref as SR
from test_step import _csc

pytestmark = pytest.mark.gpu

N, K, NSLOTS, NSTEPS, FIRST, DT = 301, 7, 3, 7, 1, 0.05


def _matrix():
    """Strictly diagonally dominant, eight entries a row in random columns, and row 7 with 290."""
    rng = np.random.default_rng(5)
    rows, cols = np.repeat(np.arange(N), 8), rng.integers(0, N, 8 * N)
    vals = rng.uniform(0.5, 1.5, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    rows, cols = np.concatenate([rows, np.full(290, 7)]), np.concatenate([cols, rng.permutation(N)[:290]])
    vals = np.concatenate([vals, rng.uniform(0.01, 0.02, 290)])
    keep = rows != cols
    A = sp.csr_matrix((vals[keep], (rows[keep], cols[keep])), shape=(N, N))
    A = sp.csc_matrix(A + sp.diags(2.0 * np.asarray(abs(A).sum(axis=1)).ravel()))
    A.sort_indices()
    assert np.bincount(A.indices, minlength=N).max() > 256
    return A.indptr.astype(np.int64) + 1, A.indices.astype(np.int64) + 1, A.data.astype(np.float64)


@pytest.fixture(scope="module")
def ladder():
    import otmb_amd.api as api

    p, i, v = _matrix()
    D = api.DeviceOperator(_csc(N, p, i, v))
    D.set_slots(NSLOTS)
    for s, vals in enumerate(SR.slot_values(v, seed=1)):
        D.set_values(vals, slot=s)
    D.set_lines(LR.random_lines(N, 3))
    rng = np.random.default_rng(21)
    yield D, np.asfortranarray(rng.standard_normal((N, K))), np.asfortranarray(rng.standard_normal((N, K)) * 1e-2), rng.uniform(0.0, 1.0, N)
    D.close()


def _same_report(got, want, fields, what):
    assert got.status == want.status == 0, (what, got)
    for name in fields:
        a, b = getattr(got, name), getattr(want, name)
        if isinstance(a, (tuple, int)):
            assert a == b, (what, name)
        else:
            DK.same_bits(a, b, (what, name))


@pytest.mark.parametrize("precond", ["jacobi", "lines"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_step_families_agree_bit_for_bit(ladder, theta, precond):
    import otmb_amd.api as api

    D, X0, S, d = ladder
    kw = dict(dt=DT, theta=theta, rtol=1e-10, maxiter=2000, precond=precond)
    a, b, w = api.plain_schedule(NSLOTS, NSTEPS, first_slot=FIRST)
    X, info = D.step(X0, nsteps=NSTEPS, first_slot=FIRST, source=S, d=d, **kw)
    assert info.steps_done == NSTEPS and all(r == "converged" for row in info.reason for r in row)
    for what, (Xo, other) in (("step_sched", D.step_sched(X0, nsteps=NSTEPS, first_slot=FIRST, substeps=1, source=[S], d=d, **kw)),
                              ("step_interp", D.step_interp(X0, slot_a=a, slot_b=b, weight=w, source=S, d=d, **kw)),
                              ("step_season", D.step_season(X0, slot_a=a, slot_b=b, weight=w, source=[S], d=[d], **kw))):
        DK.same_bits(Xo, X, (what, "state"))
        _same_report(other, info, ("steps_done", "iterations", "relres", "reason"), what)


@pytest.mark.parametrize("outer", ["none", "mean"])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_periodic_families_agree_bit_for_bit(ladder, theta, outer):
    import otmb_amd.api as api

    D, _, S, d = ladder
    kw = dict(dt=DT, theta=theta, rtol=1e-10, maxiter=2000, precond="lines", ptol=1e-8, restart=10, maxcycles=40, outer=outer)
    a, b, w = api.plain_schedule(NSLOTS, 3, first_slot=FIRST)
    X, info = D.periodic(S, ncycle=3, first_slot=FIRST, d=d, **kw)
    assert all(r == "converged" for r in info.reason)
    for what, (Xo, other) in (("periodic_sched", D.periodic_sched([S], ncycle=3, first_slot=FIRST, substeps=1, d=d, **kw)),
                              ("periodic_interp", D.periodic_interp(S, slot_a=a, slot_b=b, weight=w, d=d, **kw)),
                              ("periodic_season", D.periodic_season([S], slot_a=a, slot_b=b, weight=w, d=[d], **kw))):
        DK.same_bits(Xo, X, (what, "state"))
        _same_report(other, info, ("cycles", "defect", "reason", "msolve_iters"), what)
