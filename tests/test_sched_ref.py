"""CPU: the restatement of the scheduled step and of its periodic state (tests/sched_ref.py) on odd_nx_fold (N = 117) and tiny_tripolar
(N = 429): with substeps = 1, one source and no scale it IS step_ref; every step's state meets the solver's float64 residual bound for its own
system; the periodic state of a cycle of 3 slots x 2 sub-steps with three sources is the dense fixed point (I - Φ)⁻¹·g (Φ and g from a
dense LU per step) inside the bound of tests/test_periodic.py; and the outer GMRES preconditioned by the cycle mean with the schedule's
visit weights converges on the explicit defect."""
import numpy as np
import pytest

import periodic_pc_ref as PC
import periodic_ref as PR
import sched_ref as SC
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR

RTOL, PTOL = 1e-12, 1e-8
FIRST, SUBSTEPS, NCYCLE = 2, 2, 6
GRIDS = ["odd_nx_fold", "tiny_tripolar"]
_GRID, _CYCLE = {}, {}


def grid(oracle, name):
    """(N, (p, i, v, next), the three slots' values, the age d, three source blocks of two columns, a scale of 6 x 2) -- once per session."""
    if name not in _GRID:
        (p, i, v), N, nsurf, nxt = LR.grid(oracle, name)
        rng = np.random.default_rng(61)
        sources = [np.asfortranarray(rng.standard_normal((N, 2)) * 1e-7) for _ in range(3)]
        for S in sources:
            S[:, 0] = np.abs(S[:, 0])
        scale = rng.uniform(0.5, 2.0, (NCYCLE, 2))
        scale[1, 0], scale[2, 1], scale[3, 0] = 0.0, -1.5, 1.0
        _GRID[name] = (N, (p, i, v, nxt), SR.slot_values(v, seed=1), R.shift("age", N, nsurf)[0], sources, scale)
    return _GRID[name]


def test_the_schedule_itself():
    assert [SC.slot_of(t, 2, 2, 3) for t in range(8)] == [2, 2, 0, 0, 1, 1, 2, 2]
    assert [SC.slot_of(t, 2, 3, 3) for t in range(8)] == [2, 2, 2, 0, 0, 0, 1, 1]
    assert [SC.slot_of(t, 1, 1, 3) for t in range(5)] == [1, 2, 0, 1, 2]
    assert SC.visit_counts(3, 7, 2, 2).tolist() == [2, 2, 3] and SC.visit_counts(12, 48, 0, 4).tolist() == [4] * 12
    assert np.array_equal(SC.visit_weights(3, 7, 2, 1), PC.visit_weights(3, 7, 2))  # substeps = 1: the rule there was
    assert (SC.source_index(0, 2), SC.source_index(1, 2), SC.source_index(3, 2)) == (None, 0, 2)
    S, f = [np.full((2, 2), 3.0), np.full((2, 2), 5.0), np.full((2, 2), 7.0)], np.arange(8.0).reshape(4, 2)
    assert SC.s_eff(None, None, 0, 1) is None and SC.s_eff(S, None, 3, 1) is S[1]
    assert np.array_equal(SC.s_eff(S, f, 3, 2), [[42.0, 49.0], [42.0, 49.0]]) and np.array_equal(SC.s_eff(S[:1], f, 1, 2), [[6.0, 9.0], [6.0, 9.0]])


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", GRIDS)
def test_substeps_one_one_source_and_no_scale_is_step_ref(oracle, name, theta, adjoint):
    N, (p, i, v, nxt), values, d, sources, _ = grid(oracle, name)
    X0 = np.ones((N, 2))
    kw = dict(dt=SR.MONTH, theta=theta, nsteps=4, first_slot=FIRST, d=d, rtol=1e-10, adjoint=adjoint, next=nxt)
    Xa, ia = SR.step_ref(N, p, i, values, X0, source=sources[0], **kw)
    Xb, ib = SC.sched_ref(N, p, i, values, X0, sources=sources[:1], substeps=1, **kw)
    assert ia["steps_done"] == ib["steps_done"] == 4
    assert np.array_equal(Xa.view(np.uint64), Xb.view(np.uint64))
    assert np.array_equal(np.array(ia["iterations"]), np.array(ib["iterations"]))
    assert np.array_equal(np.array(ia["relres"]).view(np.uint64), np.array(ib["relres"]).view(np.uint64))
    assert [s[0] for s in ia["systems"]] == [s[0] for s in ib["systems"]] == [2, 0, 1, 2]
    # ... and a scale of ones, or no source at all, changes nothing either
    Xc, _ = SC.sched_ref(N, p, i, values, X0, sources=sources[:1], scale=np.ones((4, 2)), **kw)
    assert np.array_equal(Xa.view(np.uint64), Xc.view(np.uint64))
    Xd, _ = SR.step_ref(N, p, i, values, X0, source=None, **kw)
    Xe, _ = SC.sched_ref(N, p, i, values, X0, sources=None, substeps=1, **kw)
    assert np.array_equal(Xd.view(np.uint64), Xe.view(np.uint64))


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", GRIDS)
def test_every_step_meets_the_residual_bound_of_its_own_system(oracle, name, theta, adjoint):
    """6 steps from slot 2, two sub-steps a slot, the source of the slot times the step's scale (a 0.0, a negative value and a 1.0 among
    them): the step's matrix is the schedule's slot's, and its state solves that system within solve_ref.residual_check's bound."""
    N, (p, i, v, nxt), values, d, sources, scale = grid(oracle, name)
    rtol = 1e-10
    X, info = SC.sched_ref(N, p, i, values, np.ones((N, 2)), dt=SR.MONTH, theta=theta, nsteps=NCYCLE, first_slot=FIRST, substeps=SUBSTEPS, sources=sources,
                           scale=scale, d=d, rtol=rtol, adjoint=adjoint, next=nxt)
    assert info["steps_done"] == NCYCLE and [s[0] for s in info["systems"]] == [2, 2, 0, 0, 1, 1]
    sigma = SR.constants(SR.MONTH, theta)[0]
    for t, (slot, B, Xt) in enumerate(info["systems"]):
        for c, (res, bound) in enumerate(R.residual_check(R.csc_of(N, N, p, i, values[slot]), Xt, B, d, sigma, adjoint, rtol)):
            assert res <= bound, (name, theta, adjoint, t, c, res, bound)


# cycles of the restated scheduled cycle (3 slots x 2 sub-steps, three sources; column 0, column 1), GMRES(40), ptol = 1e-8, as this file's
# run on the CPU gave them: (outer = none, outer = mean with the schedule's visit weights).  DESIGN.md §6 quotes the table.  The counts move by
# a few with the order of the machine's dot products, so they are a record; what is asserted is "no more cycles than without" on the rows
# where the table shows it with room (every row but odd_nx_fold at θ = 0.5, where Crank-Nicolson at δt = a month leaves Φ with eigenvalues
# near -1 that the implicit-Euler mean does not see).
CYCLES = {("odd_nx_fold", 1.0, False): ([29, 29], [8, 8]), ("odd_nx_fold", 1.0, True): ([29, 29], [8, 8]),
          ("odd_nx_fold", 0.5, False): ([40, 42], [66, 70]), ("odd_nx_fold", 0.5, True): ([31, 40], [29, 64]),
          ("tiny_tripolar", 1.0, False): ([121, 123], [9, 9]), ("tiny_tripolar", 1.0, True): ([130, 121], [9, 9]),
          ("tiny_tripolar", 0.5, False): ([544, 493], [78, 79]), ("tiny_tripolar", 0.5, True): ([213, 296], [63, 64])}


def _cycle(oracle, name, theta, adjoint):
    """The restated cycle's maps, its dense twin and the periodic states by both outer iterations -- once per case."""
    key = (name, theta, adjoint)
    if key not in _CYCLE:
        N, (p, i, v, nxt), values, d, sources, _ = grid(oracle, name)
        kw = dict(dt=SR.MONTH, theta=theta, ncycle=NCYCLE, first_slot=FIRST, substeps=SUBSTEPS, d=d, adjoint=adjoint)
        F, Phi = SC.cycle_maps(N, p, i, values, sources, rtol=RTOL, next=nxt, **kw)
        DS = SC.DenseSched(N, p, i, values, **kw)
        Sall = SC.all_blocks(sources)
        none = PR.periodic_ref(F, Phi, Sall, ptol=PTOL, restart=40, maxcycles=2000)
        mean = PC.periodic_pc_ref(F, Phi, SC.dense_qinv(N, p, i, values, **{k: kw[k] for k in kw if k != "theta"}), Sall, ptol=PTOL, restart=40,
                                  maxcycles=2000)
        _CYCLE[key] = (N, sources, F, DS, none, mean)
    return _CYCLE[key]


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", GRIDS)
def test_the_periodic_state_is_the_dense_fixed_point(oracle, name, theta, adjoint):
    """‖x - x*‖₂ <= ‖(I - Φ)⁻¹‖₂·(ptol·‖g‖₂ + ncycle·rtol·max_t‖b_t‖₂/σ): the bound of tests/test_periodic.py (_judge), x* = (I - Φ)⁻¹·g with
    Φ and g from the dense LU of every step's own matrix and the source of its slot."""
    N, sources, F, DS, (X, info), _ = _cycle(oracle, name, theta, adjoint)
    xs, gnorm, ninv, bmax = DS.fixed_point(sources)
    print(name, theta, adjoint, "cycles", info["cycles"].tolist(), "defect", info["defect"].tolist(), "‖(I-Φ)⁻¹‖", ninv)
    assert info["converged"].all() and (info["defect"] <= PTOL).all()
    for c in range(2):
        err, bound = np.linalg.norm(X[:, c] - xs[:, c]), ninv * (PTOL * gnorm[c] + NCYCLE * RTOL * bmax[c] / DS.sigma)
        print("  column", c, "error", err, "bound", bound)
        assert err <= bound, (c, err, bound)
        Fx = DS.F(X[:, c:c + 1], [S[:, c:c + 1] for S in sources])[:, 0]
        # (the dense cycle is the restated one to what the inner solves leave: the bound's second term)
        assert np.linalg.norm(Fx - X[:, c]) <= PTOL * gnorm[c] * (1 + 1e-6) + NCYCLE * RTOL * bmax[c] / DS.sigma


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", GRIDS)
def test_the_mean_preconditioner_with_the_visit_weights_converges(oracle, name, theta, adjoint):
    """outer = "mean" over Ā = Σ_s (count_s / ncycle)·A_s with the schedule's counts: accepted on the explicit defect, inside the same bound;
    the cycles are recorded beside those of outer = "none" (CYCLES), and "no more cycles than without" is asserted where the table shows it."""
    N, sources, F, DS, (_, none), (X, info) = _cycle(oracle, name, theta, adjoint)
    xs, gnorm, ninv, bmax = DS.fixed_point(sources)
    print(name, theta, adjoint, "cycles none", none["cycles"].tolist(), "mean", info["cycles"].tolist(), "defect", info["defect"].tolist())
    assert info["converged"].all() and (info["defect"] <= PTOL).all()
    for c in range(2):
        assert np.linalg.norm(X[:, c] - xs[:, c]) <= ninv * (PTOL * gnorm[c] + NCYCLE * RTOL * bmax[c] / DS.sigma)
    want_none, want_mean = CYCLES[(name, theta, adjoint)]
    if all(2 * m <= n for m, n in zip(want_mean, want_none)):
        assert (info["cycles"] <= none["cycles"]).all()
