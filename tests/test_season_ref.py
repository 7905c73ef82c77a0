"""CPU: the restatement of the season calls (tests/season_ref.py) and the helper api.plain_schedule.  One cycle with d and the source per
slot agrees with a dense cycle (an LU per step, d_t and s_t formed densely) within what the inner solves leave,
ncycle·rtol·max_t‖b_t‖₂/σ -- the bound of tests/test_interp_ref.py.  plain_schedule is the scheduled step's rule (sched_ref.slot_of) as
explicit arrays.  And every periodic case of tests/test_season_periodic.py (tests/season_cases.py) converges in the restatement alone, within
that file's limits, in numpy's and in the device's order of sums."""
import numpy as np
import pytest

import interp_cases as IC
import interp_ref as IR
import periodic_pc_ref as PC
import periodic_ref as PR
import sched_ref as SC
import season_cases as SE
import season_ref as SN
import solve_ref as R
import step_ref as SR


def test_the_field_of_a_step():
    v = [np.array([1.0, 3.0]), np.array([5.0, 7.0]), np.array([0.1, 0.7])]
    assert SN.field(None, 0, 1, 0.5) is None
    assert SN.field(v[:1], 0, 1, 0.5) is v[0]  # given once: as it is, never blended with itself
    assert SN.field(v, 1, 2, 1.0) is v[2] and SN.field(v, 1, 2, 0.0) is v[1] and SN.field(v, 0, 0, 0.3) is v[0]
    w = 1.0 / 3.0
    wa = 1.0 - w
    assert np.array_equal(SN.field(v, 2, 0, w), wa * v[2] + w * v[0])
    assert np.array_equal(SN.field(v, 2, 0, 0.25), SN.field(v, 0, 2, 0.75))  # (the order of the two terms cannot matter)
    x = np.array([0.1, 1.0 / 3.0])
    assert not np.array_equal(wa * x + w * x, x)  # why a field given once is not folded
    assert np.array_equal(SN.source_of(v, np.array([[2.0], [3.0]]), 1, 0, 1, 0.5), (0.5 * v[0] + 0.5 * v[1]) * 3.0)  # the blend first, then the scale
    # d̄: one block is that block; per slot, the fold of combine_slots under the mean's weights
    sched = ([0, 1, 2, 2], [0, 2, 0, 1], [0.5, 0.25, 1.0, 1.0 / 3.0])
    wt = IR.mean_weights(3, *sched)
    assert SN.dbar(v[:1], *sched) is v[0] and SN.dbar(None, *sched) is None
    assert np.array_equal(SN.dbar(v, *sched), (wt[0] * v[0] + wt[1] * v[1]) + wt[2] * v[2])


def test_plain_schedule_is_the_scheduled_steps_rule():
    from otmb_amd import api

    for nslots, nsteps, first_slot, substeps in ((3, 6, 0, 2), (3, 7, 2, 1), (12, 48, 0, 4), (12, 30, 11, 4), (1, 5, 0, 3), (4, 0, 1, 1)):
        a, b, w = api.plain_schedule(nslots, nsteps, first_slot=first_slot, substeps=substeps)
        assert a.dtype == b.dtype == np.int64 and w.dtype == np.float64 and a.shape == b.shape == w.shape == (nsteps,)
        assert a.tolist() == b.tolist() == [SC.slot_of(t, first_slot, substeps, nslots) for t in range(nsteps)] and not w.any()
        assert a is not b and all(IR.kind(*s) == ("plain", int(s[0])) for s in zip(a, b, w))
    assert api.plain_schedule(3, 4)[0].tolist() == [0, 1, 2, 0]
    a, _, _ = api.plain_schedule(IC.NSLOTS, IC.NSLOTS * IC.SUBSTEPS, substeps=IC.SUBSTEPS)
    assert np.array_equal(a, SE.SCHEDULES["plain"][0])
    for bad in (dict(nslots=0, nsteps=1), dict(nslots=3, nsteps=-1), dict(nslots=3, nsteps=1, substeps=0), dict(nslots=3, nsteps=1, first_slot=3),
                dict(nslots=3, nsteps=1, first_slot=-1)):
        with pytest.raises(ValueError):
            api.plain_schedule(**bad)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_one_dense_cycle_agrees_with_the_restatement(oracle, theta, adjoint):
    """odd_nx_fold, the convention's six blended steps and a hand-written eight with plain steps among them, d and the source per slot, two
    columns: ‖F_dense(x) - F_ref(x)‖₂ <= ncycle·rtol·max_t‖b_t‖₂/σ per column (every d_t >= 0, so ‖M_t⁻¹‖₂ <= 1/σ as in
    tests/test_interp_ref.py)."""
    N, (p, i, v, nxt), values, Ds, Ss = SE.case(oracle, "odd_nx_fold")
    d, sources, rtol = [np.ascontiguousarray(D[:, 0]) for D in Ds], [S[:, :2] for S in Ss], 1e-12
    assert all((x >= 0.0).all() for x in d)
    X0 = np.ones((N, 2))
    X0[:, 1] = np.random.default_rng(3).standard_normal(N)
    hand = (np.array([0, 0, 1, 2, 2, 1, 0, 1]), np.array([0, 1, 2, 0, 0, 1, 2, 0]), np.array([0.3, 0.25, 0.5, 1.0 / 3.0, 1.0 / 3.0, 0.0, 1.0, 0.0]))
    for sa, sb, w in (IC.SCHEDULE, hand):
        kw = dict(dt=SR.MONTH, theta=theta, slot_a=sa, slot_b=sb, weight=w, d=d, sources=sources, adjoint=adjoint)
        Xr, info = SN.season_ref(N, p, i, values, X0, rtol=rtol, next=nxt, **kw)
        assert info["steps_done"] == len(w)
        DS = SN.DenseSeason(N, p, i, values, **kw)
        norms = []
        Xd = DS.F(X0, norms)
        bmax = np.max(norms, axis=0)
        for c in range(2):
            err, bound = np.linalg.norm(Xd[:, c] - Xr[:, c]), len(w) * rtol * bmax[c] / DS.sigma
            print(theta, adjoint, len(w), "column", c, "error", err, "bound", bound)
            assert err <= bound, (theta, adjoint, c, err, bound)
        # the per-slot fields matter: the cycle with slot 0's fields on every step is another state
        X1, _ = SN.season_ref(N, p, i, values, X0, rtol=rtol, next=nxt, **dict(kw, d=d[:1], sources=sources[:1]))
        assert np.linalg.norm(X1 - Xr) > 1e3 * len(w) * rtol * bmax.max() / DS.sigma
        # every step's state solves the system of ITS values and ITS d within the solver's residual bound
        sigma = SR.constants(SR.MONTH, theta)[0]
        for t, (vals, B, Xt) in enumerate(info["systems"]):
            dt_ = SN.field(d, sa[t], sb[t], w[t])
            for c, (res, bound) in enumerate(R.residual_check(R.csc_of(N, N, p, i, vals), Xt, B, dt_, sigma, adjoint, rtol)):
                assert res <= bound, (t, c, res, bound)


@pytest.mark.parametrize("sched", sorted(SE.SCHEDULES))
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("name,theta", sorted({(n, t) for n, t, _ in SE.CASES}))
def test_the_periodic_cases_converge_in_the_restatement(oracle, name, theta, adjoint, sched):
    """Every case of tests/test_season_periodic.py -- the grids, θ, A and Aᵀ, both schedules, the outer iterations that file runs, the three
    columns with their own D per slot (column 0 alone is the k = 1 case) -- converges within that file's limits in both orders of sums, and
    the column that is zero in every block is answered with zero at no cycle.  With the mean the iteration takes fewer cycles at θ = 1;
    at θ = 0.5 that is not asserted (it does not hold for every column)."""
    N, (p, i, v, nxt), values, Ds, Ss = SE.case(oracle, name)
    sa, sb, w = SE.SCHEDULES[sched]
    kw = dict(dt=IC.DT, slot_a=sa, slot_b=sb, weight=w, d=Ds, adjoint=adjoint)
    F, Phi = SN.cycle_maps(N, p, i, values, Ss, theta=theta, rtol=IC.RTOL, maxiter=IC.MAXITER, next=nxt, **kw)
    zero = SC.all_blocks(Ss)
    for order in ("numpy", "device"):
        lim = dict(ptol=IC.PTOL, restart=IC.RESTART, maxcycles=IC.MAXCYCLES, order=order)
        cycles = {}
        for outer in ("none", "mean"):
            if (name, theta, outer) not in SE.CASES:
                continue
            if outer == "none":
                X, info = PR.periodic_ref(F, Phi, zero, **lim)
            else:
                X, info = PC.periodic_pc_ref(F, Phi, SN.dense_qinv(N, p, i, values, **kw), zero, **lim)
            print(name, theta, adjoint, sched, order, outer, "cycles", info["cycles"].tolist(), "defect", info["defect"].tolist())
            assert info["converged"].all() and (info["defect"] <= IC.PTOL).all(), (order, outer, info["reason"])
            assert (info["cycles"][:2] > 2).all() and info["cycles"][2] == 0 and not X[:, 2].any()
            cycles[outer] = info["cycles"]
        if theta == 1.0:
            assert (cycles["mean"][:2] < cycles["none"][:2]).all(), cycles
