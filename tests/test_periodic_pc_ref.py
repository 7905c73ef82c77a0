"""CPU: the restatement of otmb_op_combine_slots and of otmb_op_periodic_pc with the cycle-mean preconditioner (tests/periodic_pc_ref.py):
the fold of combine_ref against a plain loop; the preconditioned iteration against the dense fixed point and against the unpreconditioned
one, cycle count by cycle count, in numpy's order of the sums and in the device's; its bookkeeping; Qinv = identity is periodic_column; and
the restated mean solve (BiCGStab + lines on combine_ref's values) in place of the dense inverse."""
import numpy as np
import pytest

import periodic_pc_ref as PC
import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR

PTOL = 1e-9
_DENSE = {}


def dense(oracle, name, theta, ncycle, adjoint, first_slot=0):
    """(DenseCycle, N, the grid's arrays, d, the dense Qinv, cond(M̄)) with the tests' three slots, δt = a month and the age d; once per session."""
    key = (name, theta, ncycle, adjoint, first_slot)
    if key not in _DENSE:
        T, N, nsurf, nxt = LR.grid(oracle, name)
        p, i, v = T
        d = R.shift("age", N, nsurf)[0]
        values = SR.slot_values(v, seed=1)
        DC = PR.DenseCycle(N, p, i, values, dt=SR.MONTH, theta=theta, ncycle=ncycle, first_slot=first_slot, d=d, adjoint=adjoint)
        Qinv, cond = PC.dense_qinv(N, p, i, values, dt=SR.MONTH, ncycle=ncycle, first_slot=first_slot, d=d, adjoint=adjoint)
        _DENSE[key] = (DC, N, (p, i, v, nxt), d, Qinv, cond)
    return _DENSE[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- combine_ref ---------------------------------------------------------------------------------------------------------------------------
def _plain_fold(values, w):
    """The fold written out over Python floats, entry by entry."""
    out = []
    for e in range(len(values[0])):
        acc, first = 0.0, True
        for s in range(len(values)):
            if float(w[s]) != 0.0:
                t = float(w[s]) * float(values[s][e])
                acc = t if first else acc + t
                first = False
        out.append(acc)
    return np.array(out)


@pytest.mark.parametrize("w", [(0.25, 0.0, 0.75), (1 / 3, 1 / 3, 1 / 3), (0.0, 0.0, 0.0), (0.0, -2.0, 0.0), (1e-3, 1e3, -1.0), (3 / 7, 2 / 7, 2 / 7)])
def test_combine_ref_is_the_fold_written_out(w):
    """Bit for bit against the plain loop, on values of mixed sign and magnitude (the order of the additions shows); a zero weight in the
    middle leaves its slot out altogether (a NaN there does not reach the result); all weights zero: +0.0; and with dst among the sources --
    the result written over slot 0, then over slot 2 -- the bits are those of the fold of the values as they were."""
    rng = np.random.default_rng(5)
    values = [rng.standard_normal(301) * 10.0 ** rng.uniform(-8, 8, 301) for _ in range(3)]
    want = _plain_fold(values, w)
    got = PC.combine_ref(values, w)
    assert np.array_equal(_bits(got), _bits(want))
    if w[1] == 0.0:
        poisoned = [values[0], np.full(301, np.nan), values[2]]
        assert np.array_equal(_bits(PC.combine_ref(poisoned, w)), _bits(want))
    if not any(w):
        assert not got.any() and not np.signbit(got).any()
    for dst in (0, 2):  # in place: elementwise, so the result may replace a source
        slots = [v.copy() for v in values]
        slots[dst][...] = PC.combine_ref(slots, w)
        assert np.array_equal(_bits(slots[dst]), _bits(want))
        assert all(np.array_equal(_bits(slots[s]), _bits(values[s])) for s in range(3) if s != dst)


def test_combine_ref_refuses_weights_that_are_not_finite_and_counts_the_visits():
    v = [np.ones(4)] * 3
    for bad in ((1.0, np.nan, 0.0), (np.inf, 0.0, 0.0), (1.0, 2.0)):
        with pytest.raises(ValueError):
            PC.combine_ref(v, bad)
    assert PC.visit_weights(3, 3, 2).tolist() == [1 / 3, 1 / 3, 1 / 3]
    assert PC.visit_weights(3, 7, 2).tolist() == [2 / 7, 2 / 7, 3 / 7]  # slots 2 0 1 2 0 1 2
    assert PC.visit_weights(3, 12, 0).tolist() == [4 / 12] * 3
    assert PC.visit_weights(12, 3, 11).tolist() == [1 / 3, 1 / 3] + [0.0] * 9 + [1 / 3]


# ---- the preconditioned iteration ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["numpy", "device"])
@pytest.mark.parametrize("restart", [5, 20])
@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("ncycle", [3, 7, 12])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", ["odd_nx_fold", "tiny_tripolar", "tiny_bipolar"])
def test_the_mean_preconditioner_cuts_the_cycles(oracle, name, theta, ncycle, adjoint, restart, order):
    """The dense Qinv = I + (P·M̄)⁻¹, s = 1 and the seeded random source, ptol = 1e-9: every column converges on its explicit defect, lies
    inside test_restarted_gmres_reaches_the_dense_fixed_point's bound ‖(I - Φ)⁻¹‖₂·(ptol·‖g‖₂ + 1e-12·‖x*‖₂), takes fewer cycles than the
    unpreconditioned iteration, and at most half of them for θ = 1 and for θ = 0.5 with 3 or 7 steps (Crank-Nicolson over twelve steps is
    the weakest case: its fast modes are not implicit Euler's)."""
    DC, N, _, _, Qinv, cond = dense(oracle, name, theta, ncycle, adjoint)
    S = np.ones((N, 2))
    S[:, 1] = np.random.default_rng(3).standard_normal(N)
    xs, gnorm, ninv = DC.fixed_point(S)
    F, Phi = DC.maps(S)
    kw = dict(ptol=PTOL, restart=restart, maxcycles=4000, order=order)
    _, none = PR.periodic_ref(F, Phi, S, **kw)
    X, info = PC.periodic_pc_ref(F, Phi, Qinv, S, **kw)
    print(name, theta, ncycle, adjoint, restart, order, "cycles", none["cycles"].tolist(), "->", info["cycles"].tolist(), "defect", info["defect"].tolist(),
          "cond(M̄)", cond)
    assert none["converged"].all()
    assert info["converged"].all() and (info["defect"] <= PTOL).all()
    for c in range(2):
        err = np.linalg.norm(X[:, c] - xs[:, c])
        bound = ninv * (PTOL * gnorm[c] + 1e-12 * np.linalg.norm(xs[:, c]))
        print("  column", c, "error", err, "bound", bound)
        assert err <= bound
        assert np.linalg.norm(DC.F(X[:, c], S[:, c]) - X[:, c]) <= PTOL * gnorm[c] * (1 + 1e-6)
        assert info["cycles"][c] < none["cycles"][c]
        if theta == 1.0 or ncycle in (3, 7):
            assert 2 * info["cycles"][c] <= none["cycles"][c]


@pytest.mark.parametrize("order", ["numpy", "device"])
def test_bookkeeping_with_qinv(oracle, order):
    """test_bookkeeping's conditions with the dense Qinv: one cycle from the returned state; a zero source costs nothing; maxcycles is never
    exceeded and the defect is the returned state's; a failing Qinv gives precond_failed with the last verified state."""
    DC, N, _, _, Qinv, _ = dense(oracle, "odd_nx_fold", 1.0, 3, False)
    S = np.ones((N, 1))
    F, Phi = DC.maps(S)
    kw = dict(ptol=1e-8, restart=2, order=order)
    X, info = PC.periodic_pc_ref(F, Phi, Qinv, S, **kw)
    assert info["converged"].all() and len(info["history"][0]) > 2  # several restarts
    X1, info1 = PC.periodic_pc_ref(F, Phi, Qinv, S, x0=X, **kw)
    assert info1["cycles"].tolist() == [1] and info1["converged"].all() and np.array_equal(X1, X) and info1["defect"][0] == info["defect"][0]
    Z, infoz = PC.periodic_pc_ref(F, Phi, Qinv, np.zeros((N, 1)), x0=X, **kw)
    assert infoz["cycles"].tolist() == [0] and infoz["converged"].all() and not Z.any() and infoz["defect"][0] == 0.0
    g = DC.F(np.zeros(N), S[:, 0])
    for maxcycles in (0, 1, 2, 3, 4, 6):
        Xm, im = PC.periodic_pc_ref(F, Phi, Qinv, S, maxcycles=maxcycles, **kw)
        assert im["reason"] == ["maxcycles"] and im["cycles"][0] <= maxcycles
        if maxcycles == 0:
            assert np.isnan(im["defect"][0]) and not Xm.any()
        else:
            assert np.isclose(im["defect"][0], np.linalg.norm(DC.F(Xm[:, 0], S[:, 0]) - Xm[:, 0]) / np.linalg.norm(g), rtol=1e-9)
    assert PC.periodic_pc_ref(F, Phi, Qinv, S, maxcycles=3, **kw)[1]["cycles"].tolist() == [3]  # g, one iteration, its verification
    # a Qinv that fails in its 4th call: the first restart (two iterations) has been verified, the second is under way
    calls = [0]

    def failing(c, v):
        calls[0] += 1
        return (None, 7) if calls[0] == 4 else (Qinv(c, v)[0], 5)

    Xf, inf = PC.periodic_pc_ref(F, Phi, failing, S, **kw)
    Xv, inv = PC.periodic_pc_ref(F, Phi, Qinv, S, maxcycles=4, **kw)  # g, two iterations, their verification: the same state
    assert inf["reason"] == ["precond_failed"] and not inf["converged"].any()
    assert inf["cycles"].tolist() == [5] and inf["msolve_iters"].tolist() == [3 * 5 + 7]  # g, 2 iterations, the verification, 1 iteration
    assert inv["cycles"].tolist() == [4] and np.array_equal(_bits(Xf), _bits(Xv)) and inf["defect"][0] == inv["defect"][0]
    # a Qinv that fails at once: the start is kept, the defect is g's own
    X0, i0 = PC.periodic_pc_ref(F, Phi, lambda c, v: (None, 0), S, **kw)
    assert i0["reason"] == ["precond_failed"] and i0["cycles"].tolist() == [1] and not X0.any() and i0["defect"][0] == 1.0


@pytest.mark.parametrize("order", ["numpy", "device"])
@pytest.mark.parametrize("theta,restart", [(1.0, 5), (0.5, 20)])
def test_qinv_identity_is_periodic_column(oracle, theta, restart, order):
    DC, N, _, _, _, _ = dense(oracle, "odd_nx_fold", theta, 3, False)
    S = np.ones((N, 2))
    S[:, 1] = np.random.default_rng(3).standard_normal(N)
    F, Phi = DC.maps(S)
    x0 = np.random.default_rng(4).standard_normal((N, 2))
    for start in (None, x0):
        X0, i0 = PR.periodic_ref(F, Phi, S, x0=start, ptol=PTOL, restart=restart, maxcycles=2000, order=order)
        X1, i1 = PC.periodic_pc_ref(F, Phi, PC.identity, S, x0=start, ptol=PTOL, restart=restart, maxcycles=2000, order=order)
        assert np.array_equal(_bits(X0), _bits(X1)) and np.array_equal(i0["cycles"], i1["cycles"]) and i0["reason"] == i1["reason"]
        assert np.array_equal(_bits(i0["defect"]), _bits(i1["defect"])) and i0["history"] == i1["history"] and not i1["msolve_iters"].any()


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_on_top_of_the_restated_mean_solve(oracle, theta):
    """mean_maps (the restated BiCGStab with the lines at rtol = 1e-12 on combine_ref's values) in place of the dense inverse, on odd_nx_fold,
    3 steps from slot 2, GMRES(10), over the restated step (cycle_maps, the same rtol): the cycles of the dense Qinv over the dense cycle
    within one, every mean solve converged, and x inside the bound of test_on_top_of_the_restated_step."""
    DC, N, (p, i, v, nxt), d, Qdense, _ = dense(oracle, "odd_nx_fold", theta, 3, False, first_slot=2)
    S = np.ones((N, 1))
    values = SR.slot_values(v, seed=1)
    Q = PC.mean_maps(N, p, i, values, dt=SR.MONTH, ncycle=3, first_slot=2, d=d, rtol=1e-12, next=nxt)
    Xd, idn = PC.periodic_pc_ref(*DC.maps(S), Qdense, S, ptol=1e-8, restart=10, maxcycles=1000)
    F, Phi = PR.cycle_maps(N, p, i, values, S, dt=SR.MONTH, theta=theta, ncycle=3, first_slot=2, d=d, rtol=1e-12, next=nxt)
    X, info = PC.periodic_pc_ref(F, Phi, Q, S, ptol=1e-8, restart=10, maxcycles=1000)
    print(theta, "cycles", info["cycles"], "dense Qinv", idn["cycles"], "mean-solve iterations", info["msolve_iters"])
    assert info["converged"].all() and idn["converged"].all() and info["msolve_iters"][0] > 0
    assert abs(int(info["cycles"][0]) - int(idn["cycles"][0])) <= 1
    xs, gnorm, ninv = DC.fixed_point(S)
    allowance = 3 * 1e-12 * DC.rhs_norms(xs, S)[0] / DC.sigma
    assert np.linalg.norm(X[:, 0] - xs[:, 0]) <= ninv * (1e-8 * gnorm[0] + allowance + 1e-12 * np.linalg.norm(xs))
