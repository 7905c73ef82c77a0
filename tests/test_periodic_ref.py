"""CPU: the restatement of otmb_op_periodic (tests/periodic_ref.py) finds the periodic state of the stepped cycle -- against the dense fixed
point (I - Φ)⁻¹·g, on top of the restated step, and in its bookkeeping (cycles, the start, maxcycles, a failing step)."""
import numpy as np
import pytest

import periodic_ref as PR
import solve_lines_ref as LR
import solve_ref as R
import step_ref as SR

PTOL = 1e-9
_DENSE = {}


def dense(oracle, name, theta, ncycle, adjoint, first_slot=0):
    """(DenseCycle, N, the grid's arrays, d) with the tests' three slots, δt = a month and the age d; made once per session."""
    key = (name, theta, ncycle, adjoint, first_slot)
    if key not in _DENSE:
        T, N, nsurf, nxt = LR.grid(oracle, name)
        p, i, v = T
        d = R.shift("age", N, nsurf)[0]
        DC = PR.DenseCycle(N, p, i, SR.slot_values(v, seed=1), dt=SR.MONTH, theta=theta, ncycle=ncycle, first_slot=first_slot, d=d, adjoint=adjoint)
        _DENSE[key] = (DC, N, (p, i, v, nxt), d)
    return _DENSE[key]


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("ncycle", [3, 12])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", ["odd_nx_fold", "tiny_tripolar"])
def test_restarted_gmres_reaches_the_dense_fixed_point(oracle, name, theta, ncycle, adjoint):
    """GMRES(20), s = 1 and a random source: every column converges with defect <= ptol on its explicit residual, and
    ‖x - x*‖₂ <= ‖(I - Φ)⁻¹‖₂·(ptol·‖g‖₂ + 1e-12·‖x*‖₂): x - x* = (I - Φ)⁻¹·(F(x) - x) exactly, and the second term is what evaluating the
    dense cycle in double can be off by (ncycle LU solves of n <= 429 unknowns: n·ncycle·ε ≈ 6e-13)."""
    DC, N, _, _ = dense(oracle, name, theta, ncycle, adjoint)
    S = np.ones((N, 2))
    S[:, 1] = np.random.default_rng(3).standard_normal(N)
    xs, gnorm, ninv = DC.fixed_point(S)
    F, Phi = DC.maps(S)
    X, info = PR.periodic_ref(F, Phi, S, ptol=PTOL, restart=20, maxcycles=2000)
    print(name, theta, ncycle, adjoint, "cycles", info["cycles"].tolist(), "defect", info["defect"].tolist(), "‖(I-Φ)⁻¹‖", ninv)
    assert info["converged"].all() and (info["defect"] <= PTOL).all()
    for c in range(2):
        err = np.linalg.norm(X[:, c] - xs[:, c])
        bound = ninv * (PTOL * gnorm[c] + 1e-12 * np.linalg.norm(xs[:, c]))
        print("  column", c, "error", err, "bound", bound)
        assert err <= bound
        assert np.linalg.norm(DC.F(X[:, c], S[:, c]) - X[:, c]) <= PTOL * gnorm[c] * (1 + 1e-6)


# iterations of scipy's unrestarted GMRES to 1e-9 on (I - Φ)·x = g, s = 1, A, first_slot = 0 (the issue's table)
UNRESTARTED = {("odd_nx_fold", 1.0, 3): 34, ("odd_nx_fold", 1.0, 12): 26, ("odd_nx_fold", 0.5, 3): 51, ("odd_nx_fold", 0.5, 12): 29,
               ("tiny_tripolar", 1.0, 3): 108, ("tiny_tripolar", 1.0, 12): 76, ("tiny_tripolar", 0.5, 3): 174, ("tiny_tripolar", 0.5, 12): 88}


@pytest.mark.parametrize("case", sorted(UNRESTARTED))
def test_unrestarted_cycle_counts(oracle, case):
    """restart = N: defect <= ptol, and cycles = the table's iterations + 2 -- the cycle that gives g (the first residual) and the one
    verifying cycle; the restatement shows exactly that on all eight rows.  Measured here (cycles; the table's iterations):
        odd_nx_fold   θ = 1:   ncycle 3: 36 (34), 12: 28 (26);   θ = 0.5:  3: 53 (51),  12: 31 (29)
        tiny_tripolar θ = 1:   ncycle 3: 110 (108), 12: 78 (76); θ = 0.5:  3: 176 (174), 12: 90 (88)
    (Aᵀ: 36, 28, 53, 30, 111, 78, 178, 91.)  One iteration either way is allowed: whether the recursive residual crosses ptol·‖g‖ at an
    iteration or the next is decided within the rounding of the dot products, whose order belongs to the BLAS of the machine."""
    name, theta, ncycle = case
    DC, N, _, _ = dense(oracle, name, theta, ncycle, False)
    S = np.ones((N, 1))
    F, Phi = DC.maps(S)
    X, info = PR.periodic_ref(F, Phi, S, ptol=PTOL, restart=N, maxcycles=2000)
    print(case, "cycles", int(info["cycles"][0]), "table", UNRESTARTED[case], "defect", float(info["defect"][0]))
    assert info["converged"].all() and info["defect"][0] <= PTOL
    assert len(info["history"][0]) == 2  # g, then one verification: no restart
    assert abs(int(info["cycles"][0]) - (UNRESTARTED[case] + 2)) <= 1


@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_on_top_of_the_restated_step(oracle, theta):
    """cycle_maps (step_ref.step_ref with the lines, rtol = 1e-12) against the dense cycle on odd_nx_fold, 3 steps from slot 2, GMRES(10):
    the same state within ‖(I - Φ)⁻¹‖·(ptol·‖g‖ + the inner solves' ncycle·rtol·max‖b_t‖/σ) of x*."""
    DC, N, (p, i, v, nxt), d = dense(oracle, "odd_nx_fold", theta, 3, False, first_slot=2)
    S = np.ones((N, 1))
    xs, gnorm, ninv = DC.fixed_point(S)
    rtol = 1e-12
    F, Phi = PR.cycle_maps(N, p, i, SR.slot_values(v, seed=1), S, dt=SR.MONTH, theta=theta, ncycle=3, first_slot=2, d=d, rtol=rtol, next=nxt)
    X, info = PR.periodic_ref(F, Phi, S, ptol=1e-8, restart=10, maxcycles=1000)
    allowance = 3 * rtol * DC.rhs_norms(xs, S)[0] / DC.sigma
    err, bound = np.linalg.norm(X[:, 0] - xs[:, 0]), ninv * (1e-8 * gnorm[0] + allowance + 1e-12 * np.linalg.norm(xs))
    print(theta, "cycles", info["cycles"], "defect", info["defect"], "error", err, "bound", bound)
    assert info["converged"].all() and err <= bound


def test_bookkeeping(oracle):
    """The start, a zero source, maxcycles and a failing step."""
    DC, N, _, _ = dense(oracle, "odd_nx_fold", 1.0, 3, False)
    S = np.ones((N, 1))
    F, Phi = DC.maps(S)
    X, info = PR.periodic_ref(F, Phi, S, ptol=1e-8, restart=5)
    assert info["converged"].all() and len(info["history"][0]) > 2  # several restarts
    # from the returned state: one cycle (F(x) and g side by side), the same state
    X1, info1 = PR.periodic_ref(F, Phi, S, x0=X, ptol=1e-8, restart=5)
    assert info1["cycles"].tolist() == [1] and info1["converged"].all() and np.array_equal(X1, X)
    assert info1["defect"][0] == info["defect"][0]
    # a zero source: x = 0 at no cost, whatever the start
    Z, infoz = PR.periodic_ref(F, Phi, np.zeros((N, 1)), x0=X, ptol=1e-8, restart=5)
    assert infoz["cycles"].tolist() == [0] and infoz["converged"].all() and not Z.any() and infoz["defect"][0] == 0.0
    # maxcycles: never exceeded, and the defect is the returned state's
    for maxcycles in (0, 1, 2, 3, 4, 9):
        Xm, im = PR.periodic_ref(F, Phi, S, ptol=1e-8, restart=5, maxcycles=maxcycles)
        assert im["reason"] == ["maxcycles"] and im["cycles"][0] <= maxcycles
        if maxcycles == 0:
            assert np.isnan(im["defect"][0]) and not Xm.any()
        else:
            g = DC.F(np.zeros(N), S[:, 0])
            assert np.isclose(im["defect"][0], np.linalg.norm(DC.F(Xm[:, 0], S[:, 0]) - Xm[:, 0]) / np.linalg.norm(g), rtol=1e-9)
    assert PR.periodic_ref(F, Phi, S, ptol=1e-8, restart=5, maxcycles=3)[1]["cycles"].tolist() == [3]  # g, one iteration, its verification
    # a step that fails in the 4th call
    calls = [0]

    def failing(c, v):
        calls[0] += 1
        return None if calls[0] == 3 else Phi(c, v)

    Xf, inf = PR.periodic_ref(F, failing, S, ptol=1e-8, restart=5)
    assert inf["reason"] == ["step_failed"] and inf["cycles"].tolist() == [3] and not Xf.any()


def test_the_device_order_of_a_sum_is_a_sum():
    """device_sum / device_dots / device_update (the order of csrc/otmb_periodic.hip's sums) against numpy's, within the bound of any
    order: |Σ̂ - Σ| <= (n - 1)·ε·Σ|p_i|."""
    rng = np.random.default_rng(7)
    for n in (1, 2, 117, 2048, 2049, 4609):
        V, w = rng.standard_normal((3, n)), rng.standard_normal(n)
        h, nrm = PR.device_dots(V, w)
        for j in range(3):
            assert abs(h[j] - V[j] @ w) <= 2 * n * R.EPS * (np.abs(V[j]) @ np.abs(w))
        assert abs(nrm - w @ w) <= 2 * n * R.EPS * (w @ w)
        assert np.allclose(PR.device_update(V, h, w), w - h @ V, rtol=0, atol=1e-12 * np.abs(w).max() * 10)


@pytest.mark.parametrize("adjoint", [False, True])
@pytest.mark.parametrize("ncycle", [3, 12])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_the_device_order_reaches_the_same_fixed_point_in_the_same_cycles(oracle, theta, ncycle, adjoint):
    """order="device" (every sum, update and back substitution in the order of csrc/otmb_periodic.hip and GmresLsq) on odd_nx_fold over the
    dense cycle, GMRES(20), s = 1 and a random source: it converges, in the cycles of the default order, to an X inside the bound of
    test_restarted_gmres_reaches_the_dense_fixed_point (the same ptol, the same ‖(I - Φ)⁻¹‖₂, the same formula)."""
    DC, N, _, _ = dense(oracle, "odd_nx_fold", theta, ncycle, adjoint)
    S = np.ones((N, 2))
    S[:, 1] = np.random.default_rng(3).standard_normal(N)
    xs, gnorm, ninv = DC.fixed_point(S)
    F, Phi = DC.maps(S)
    X0, info0 = PR.periodic_ref(F, Phi, S, ptol=PTOL, restart=20, maxcycles=2000)
    X, info = PR.periodic_ref(F, Phi, S, ptol=PTOL, restart=20, maxcycles=2000, order="device")
    print(theta, ncycle, adjoint, "cycles", info["cycles"].tolist(), "default order", info0["cycles"].tolist(), "defect", info["defect"].tolist())
    assert info["converged"].all() and (info["defect"] <= PTOL).all()
    assert np.array_equal(info["cycles"], info0["cycles"])
    for c in range(2):
        err = np.linalg.norm(X[:, c] - xs[:, c])
        bound = ninv * (PTOL * gnorm[c] + 1e-12 * np.linalg.norm(xs[:, c]))
        print("  column", c, "error", err, "bound", bound)
        assert err <= bound
        assert np.linalg.norm(DC.F(X[:, c], S[:, c]) - X[:, c]) <= PTOL * gnorm[c] * (1 + 1e-6)


def test_the_device_order_keeps_the_bookkeeping(oracle):
    """From the returned state one cycle and the same state and defect; a zero source costs nothing; maxcycles is never exceeded."""
    DC, N, _, _ = dense(oracle, "odd_nx_fold", 1.0, 3, False)
    S = np.ones((N, 1))
    F, Phi = DC.maps(S)
    X, info = PR.periodic_ref(F, Phi, S, ptol=1e-8, restart=5, order="device")
    assert info["converged"].all() and len(info["history"][0]) > 2
    X1, info1 = PR.periodic_ref(F, Phi, S, x0=X, ptol=1e-8, restart=5, order="device")
    assert info1["cycles"].tolist() == [1] and info1["converged"].all() and np.array_equal(X1, X) and info1["defect"][0] == info["defect"][0]
    Z, infoz = PR.periodic_ref(F, Phi, np.zeros((N, 1)), x0=X, ptol=1e-8, restart=5, order="device")
    assert infoz["cycles"].tolist() == [0] and not Z.any() and infoz["defect"][0] == 0.0
    for maxcycles in (0, 1, 2, 3, 4, 9):
        _, im = PR.periodic_ref(F, Phi, S, ptol=1e-8, restart=5, maxcycles=maxcycles, order="device")
        assert im["reason"] == ["maxcycles"] and im["cycles"][0] <= maxcycles
    with pytest.raises(AssertionError):
        PR.periodic_ref(F, Phi, S, order="blas")


def _written_out_sum(p):
    """Σ p as csrc/otmb_periodic.hip adds it, in three plain loops over Python floats: a lane's row pairs (pd_row, pd_dots_lane), the
    workgroup's tree (op_block_sum of csrc/otmb_op_sum.h), the fold over the workgroups (pd_fold_kernel)."""
    p = [float(v) for v in p]
    n = len(p)
    nwg = (n + PR.PD_ROWS - 1) // PR.PD_ROWS
    parts = []
    for wg in range(nwg):
        acc = [0.0] * 256
        for t in range(256):  # the lanes
            for q in range(PR.PD_ROWS // 512):
                i = 2 * (wg * (PR.PD_ROWS // 2) + t + 256 * q)
                if i >= n:
                    break
                acc[t] = acc[t] + p[i]
                if i + 1 < n:
                    acc[t] = acc[t] + p[i + 1]
        waves = []
        for w in range(4):  # the tree: xor shuffles in a wave, every lane at once
            x = acc[64 * w:64 * w + 64]
            for dist in (32, 16, 8, 4, 2, 1):
                x = [x[lane] + x[lane ^ dist] for lane in range(64)]
            waves.append(x[0])
        parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    s = parts[0]
    for b in range(1, nwg):  # the fold
        s = s + parts[b]
    return s, parts


@pytest.mark.parametrize("n", [1, 513, 2048, 2049, 4609])
def test_device_sum_is_the_sum_written_out(n):
    """_lanes / _workgroup / _fold against the three loops, bit for bit, with several workgroups in play (n = 4609: three, the last partly
    filled; 2049: the second holds one row), on terms of mixed sign and magnitude so that the order shows; and the order does show:
    reversing the terms changes the bits."""
    rng = np.random.default_rng(40 + n)
    p = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)
    want, parts = _written_out_sum(p)
    assert len(parts) == (n + 2047) // 2048
    got = PR.device_sum(p)
    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (n, got, want)
    assert np.array_equal(PR._workgroup(PR._lanes(p)).view(np.uint64), np.array(parts).view(np.uint64))
    V = rng.standard_normal((2, n))
    h, nrm = PR.device_dots(V, p)
    assert [float(x) for x in h] == [_written_out_sum(V[j] * p)[0] for j in range(2)] and float(nrm) == _written_out_sum(p * p)[0]
    if n == 4609:
        assert PR.device_sum(p[::-1]) != got
