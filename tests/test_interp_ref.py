"""CPU: the convention helper api.interp_schedule and the restatement of the interpolated step and of its periodic state
(tests/interp_ref.py).  The schedule is compared with fractions.Fraction (the exact time of every step against the slots' mid-points); over
one whole cycle every slot's total weight is exactly `substeps`; substeps = 1 at mid-step is the plain schedule.  One interpolated cycle
in dense numpy (an LU per step) agrees with the restatement within the term that tests/test_sched_ref.py derives for what the inner solves
leave, ncycle·rtol·max_t‖b_t‖₂/σ.  And the periodic cases of tests/test_interp_periodic.py converge in the restatement alone, within that
file's tolerances and iteration limits."""
from fractions import Fraction

import numpy as np
import pytest

import interp_cases as IC
import interp_ref as IR
import periodic_pc_ref as PC
import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR

AT = {"start": Fraction(0), "mid": Fraction(1, 2), "end": Fraction(1)}


@pytest.mark.parametrize("at", ["start", "mid", "end"])
@pytest.mark.parametrize("substeps", [1, 2, 3, 4])
@pytest.mark.parametrize("nslots", [1, 2, 3, 12])
def test_the_schedule_against_rationals(nslots, substeps, at):
    """Interval j of the cycle (j = 0 .. nslots - 1, slot (first_slot + j) mod nslots) spans [j, j + 1) in units of one slot and is valid at
    j + 1/2.  Step t is evaluated at τ = (t + at) / substeps; with u = τ - 1/2, its left neighbour is interval floor(u), its weight on the
    right neighbour u - floor(u)."""
    from otmb_amd import api

    for first_slot, ncycles in ((0, 1), (nslots - 1, 2)):
        a, b, w = api.interp_schedule(nslots, substeps, ncycles=ncycles, first_slot=first_slot, at=at)
        ra, rb, rw = IR.interp_schedule(nslots, substeps, ncycles=ncycles, first_slot=first_slot, at=at)
        assert a.dtype == b.dtype == np.int64 and w.dtype == np.float64 and len(a) == len(b) == len(w) == ncycles * nslots * substeps
        assert np.array_equal(a, ra) and np.array_equal(b, rb) and np.array_equal(w.view(np.uint64), rw.view(np.uint64))
        total = [Fraction(0)] * nslots
        for t in range(len(w)):
            u = (Fraction(t) + AT[at]) / substeps - Fraction(1, 2)
            left = u.numerator // u.denominator  # floor, also below zero
            frac = u - left
            assert a[t] == (first_slot + left) % nslots and b[t] == (a[t] + 1) % nslots, (t, a[t], b[t])
            assert w[t] == float(frac) and 0.0 <= w[t] < 1.0, (t, w[t], frac)  # (float(Fraction) is the correctly rounded quotient: one division)
            total[a[t]] += 1 - frac
            total[b[t]] += frac
        # one whole cycle gives every slot exactly `substeps` steps' worth of weight, in rationals
        assert total == [Fraction(ncycles * substeps)] * nslots, total


def test_one_substep_at_mid_step_is_the_plain_schedule():
    from otmb_amd import api

    for nslots in (1, 3, 12):
        a, b, w = api.interp_schedule(nslots, 1, ncycles=2, first_slot=nslots - 1)
        assert not w.any() and np.array_equal(a, (nslots - 1 + np.arange(2 * nslots)) % nslots)
        assert all(IR.kind(*s) == ("plain", s[0]) for s in zip(a, b, w))
    a, b, w = api.interp_schedule(12, 4)
    assert len(w) == 48 and a[:3].tolist() == [11, 11, 0] and b[:3].tolist() == [0, 0, 1] and w[:5].tolist() == [0.625, 0.875, 0.125, 0.375, 0.625]
    for bad in (dict(nslots=0, substeps=1), dict(nslots=3, substeps=0), dict(nslots=3, substeps=1, first_slot=3), dict(nslots=3, substeps=1, at="late")):
        with pytest.raises(ValueError):
            api.interp_schedule(**bad)


def test_the_rule_and_the_mean_weights():
    assert IR.kind(1, 1, 0.5) == ("plain", 1) and IR.kind(1, 2, 0.0) == ("plain", 1) and IR.kind(1, 2, 1.0) == ("plain", 2)
    assert IR.kind(2, 0, 0.25) == ("blend", None)
    v = [np.array([1.0, 3.0]), np.array([5.0, 7.0]), np.array([0.1, 0.7])]
    assert IR.step_values(v, 1, 2, 1.0) is v[2] and IR.step_values(v, 0, 0, 0.3) is v[0]
    w = 1.0 / 3.0
    assert np.array_equal(IR.step_values(v, 2, 0, w), (1.0 - w) * v[2] + w * v[0])
    assert np.array_equal(IR.step_values(v, 2, 0, 0.25), IR.step_values(v, 0, 2, 0.75))  # (the order of the two terms cannot matter)
    # a plain step adds 1.0; a blended step 1.0 - w, then w; acc / ncycle
    a, b, ws = [0, 1, 2, 2], [0, 2, 0, 1], [0.5, 0.25, 1.0, 1.0 / 3.0]
    acc = [1.0 + 1.0, 0.75 + 1.0 / 3.0, 0.25 + (1.0 - 1.0 / 3.0)]
    assert np.array_equal(IR.mean_weights(3, a, b, ws), np.array([x / 4.0 for x in acc]))
    assert np.array_equal(IR.mean_weights(3, *IR.interp_schedule(3, 2)), np.array([2.0 / 6.0] * 3))  # the convention's: every slot its share


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_one_dense_cycle_agrees_with_the_restatement(oracle, theta, adjoint):
    """odd_nx_fold, the convention's six steps (all blended) and a hand-written eight with plain steps among them, the age d, a source, two
    columns: ‖F_dense(x) - F_ref(x)‖₂ <= ncycle·rtol·max_t‖b_t‖₂/σ per column -- the term of tests/test_sched_ref.py's bound that stands for
    what the inner solves leave (a step's solve stops at ‖r‖ <= rtol·‖b_t‖, ‖M_t⁻¹‖₂ <= 1/σ carries that into the state, and no later step
    enlarges it)."""
    N, (p, i, v, nxt), values, D, S = IC.case(oracle, "odd_nx_fold")
    d, rtol = D[:, 0], 1e-12
    X0 = np.ones((N, 2))
    X0[:, 1] = np.random.default_rng(3).standard_normal(N)
    hand = (np.array([0, 0, 1, 2, 2, 1, 0, 1]), np.array([0, 1, 2, 0, 0, 1, 2, 0]), np.array([0.3, 0.25, 0.5, 1.0 / 3.0, 1.0 / 3.0, 0.0, 1.0, 0.0]))
    for sa, sb, w in (IC.SCHEDULE, hand):
        kw = dict(dt=SR.MONTH, theta=theta, slot_a=sa, slot_b=sb, weight=w, d=d, adjoint=adjoint)
        Xr, info = IR.interp_ref(N, p, i, values, X0, source=S[:, :2], rtol=rtol, next=nxt, **kw)
        assert info["steps_done"] == len(w)
        DI = IR.DenseInterp(N, p, i, values, **kw)
        norms = []
        Xd = DI.F(X0, S[:, :2], norms)
        bmax = np.max(norms, axis=0)
        for c in range(2):
            err, bound = np.linalg.norm(Xd[:, c] - Xr[:, c]), len(w) * rtol * bmax[c] / DI.sigma
            print(theta, adjoint, len(w), "column", c, "error", err, "bound", bound)
            assert err <= bound, (theta, adjoint, c, err, bound)
        # every step's state solves the system of ITS values within the solver's residual bound
        sigma = SR.constants(SR.MONTH, theta)[0]
        for t, (vals, B, Xt) in enumerate(info["systems"]):
            for c, (res, bound) in enumerate(R.residual_check(R.csc_of(N, N, p, i, vals), Xt, B, d, sigma, adjoint, rtol)):
                assert res <= bound, (t, c, res, bound)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", IC.GRIDS)
def test_the_periodic_cases_converge_in_the_restatement(oracle, name, theta, adjoint):
    """Every case of tests/test_interp_periodic.py -- both grids, θ, A and Aᵀ, outer none and mean, the three columns with their own d (column
    0 alone is the k = 1 case) -- converges within that file's limits, and the zero column is answered with zero at no cycle."""
    N, (p, i, v, nxt), values, D, S = IC.case(oracle, name)
    sa, sb, w = IC.SCHEDULE
    kw = dict(dt=IC.DT, slot_a=sa, slot_b=sb, weight=w, d=D, adjoint=adjoint)
    F, Phi = IR.cycle_maps(N, p, i, values, S, theta=theta, rtol=IC.RTOL, maxiter=IC.MAXITER, next=nxt, **kw)
    lim = dict(ptol=IC.PTOL, restart=IC.RESTART, maxcycles=IC.MAXCYCLES)
    for outer in ("none", "mean"):
        if outer == "none":
            X, info = PR.periodic_ref(F, Phi, S, **lim)
        else:
            X, info = PC.periodic_pc_ref(F, Phi, IR.dense_qinv(N, p, i, values, **kw), S, **lim)
        print(name, theta, adjoint, outer, "cycles", info["cycles"].tolist(), "defect", info["defect"].tolist())
        assert info["converged"].all() and (info["defect"] <= IC.PTOL).all(), (outer, info["reason"])
        assert (info["cycles"][:2] > 2).all() and info["cycles"][2] == 0 and not X[:, 2].any()
