"""CPU: the numpy restatement of buildTsink and add_matrix (tests/sink_ref.py) is what the contract says it is.

Conservation (seafloor = "closed"): column c of S holds (w_c·a)/v_c on the diagonal and -((w_c·a)/v_b) below.  volᵀ·S sums, per column,
v_c·fl(wa/v_c) + v_b·fl(-(wa/v_b)): each product is wa·(1 + δ)(1 + δ') with |δ|, |δ'| <= ε = 2⁻⁵³, so the column's sum is at most
(4ε + O(ε²))·wa in size and the whole row vector at most 4ε·Σ_c |v_c·S_cc| in the 1-norm (a bottom cell contributes an exact zero to both
sides).  Burial (seafloor = "open"): volᵀ·(S·x) is the flux through the seafloor faces; the two sides are sums of at most N + 2 products
of three factors each, so they agree within 2·(N + 8)·ε·Σ |v_r·S_rc·x_c| (γ_{N+8} on either side, the standard bound of a dot product)."""
import numpy as np
import pytest
import scipy.sparse as sp

import sink_ref as K
import solve_lines_ref as LR
import solve_ref as R
from helpers import CASES, make_case

W = 1.0e-3  # m/s: 86 m per day
RATE = 1.0 / (100 * R.DAY)  # a remineralisation rate: s⁻¹
RTOL = 1e-10

_CASES = {}


def _case(name):
    if name not in _CASES:
        g, gm = make_case(name)
        _CASES[name] = (np.asarray(gm.v3D), np.asarray(gm.area2D))
    return _CASES[name]


def _w3d(v3D, seed=2):
    """A speed per cell: positive on the wet cells, NaN on land (never read)."""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.where(np.isnan(v3D), np.nan, rng.uniform(0.2, 2.0, v3D.shape) * W))


def _scipy(N, S):
    return R.csc_of(N, N, *S)


def _vol(v3D):
    return v3D.ravel(order="F")[~np.isnan(v3D.ravel(order="F"))]


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_closed_seafloor_conserves_the_inventory(name):
    v3D, area = _case(name)
    vol = _vol(v3D)
    N = vol.size
    for w in (W, _w3d(v3D)):
        p, i, v = K.sink_ref(w, v3D, area, "closed")
        col = np.repeat(np.arange(N), np.diff(p))
        terms = vol[i - 1] * v
        sums = np.zeros(N)
        np.add.at(sums, col, terms)
        scale = np.abs(terms[i - 1 == col]).sum()
        print(name, "‖volᵀ·S‖₁ / Σ|v_c·S_cc| =", np.abs(sums).sum() / scale)
        assert scale > 0 and np.abs(sums).sum() <= 4 * R.EPS * scale
        # the bottom cells: a stored +0.0
        bottom = np.diff(p) == 1
        d = v[p[:-1] - 1]
        assert bottom.any() and not d[bottom].any() and not np.signbit(d[bottom]).any() and (d[~bottom] > 0).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_an_open_seafloor_buries_the_flux_through_the_seafloor_faces(name):
    v3D, area = _case(name)
    vol = _vol(v3D)
    N = vol.size
    x = np.random.default_rng(3).uniform(0.5, 1.5, N)
    for w in (W, _w3d(v3D)):
        S = _scipy(N, K.sink_ref(w, v3D, area, "open"))
        lhs = vol @ (S @ x)
        rhs = K.seafloor_flux(w, v3D, area, x)
        bound = 2 * (N + 8) * R.EPS * (vol @ (abs(S) @ x))
        print(name, "volᵀ·S·x", lhs, "seafloor flux", rhs, "difference / bound", abs(lhs - rhs) / bound)
        assert rhs > 0 and abs(lhs - rhs) <= bound
        # and the closed operator differs from it on the bottom cells' diagonals only
        po, io, vo = K.sink_ref(w, v3D, area, "open")
        pc, ic, vc = K.sink_ref(w, v3D, area, "closed")
        assert np.array_equal(po, pc) and np.array_equal(io, ic)
        differ = np.flatnonzero(vo != vc)
        assert np.array_equal(differ, (po[:-1] - 1)[np.diff(po) == 1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_pattern_lies_inside_the_pattern_of_T(oracle, name):
    T, N, nsurf, nxt = LR.grid(oracle, name)
    v3D, area = _case(name)
    p, i, v = K.sink_ref(W, v3D, area)
    assert len(p) == N + 1 == len(T[0])
    wet, L3, n = K.wet_indices(v3D)
    pairs = int((wet[:, :, :-1] & wet[:, :, 1:]).sum())
    assert n == N and len(i) == N + pairs  # a grid constant
    two = np.diff(p) == 2
    assert np.array_equal(i[p[:-1] - 1], np.arange(1, N + 1)) and (i[p[:-1][two]] > i[p[:-1][two] - 1]).all()  # the diagonal, then the cell below
    K.match_positions(T[0], T[1], p, i)  # raises PatternNotContained otherwise
    # ... and the lines of the grid are S's off-diagonals
    mine = np.zeros(N, dtype=np.int64)
    mine[two] = i[p[:-1][two]]
    assert np.array_equal(mine, nxt)


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_column_recursion_agrees_with_the_lines_solver_which_takes_one_iteration(oracle, name):
    """(r·I + S)·x = s: the lines preconditioner is M itself (S is lower bidiagonal along the water columns), so the restated solver stops
    after ONE iteration; its x and the closed-form recursion's both meet solve_ref.residual_check's bound."""
    v3D, area = _case(name)
    N = _vol(v3D).size
    nxt = LR.grid(oracle, name)[3]
    s = np.random.default_rng(5).uniform(0.5, 1.5, N)
    for seafloor in K.SEAFLOORS:
        S = K.sink_ref(_w3d(v3D), v3D, area, seafloor)
        A = _scipy(N, S)
        X, info = LR.solve_lines_ref(A, s, nxt, sigma=RATE, rtol=RTOL)
        assert info["converged"].all() and info["iterations"].tolist() == [1], (name, seafloor, info)
        x = K.column_solve(*S, RATE, s)
        for what, sol in (("lines", X), ("recursion", x)):
            (res, bound), = R.residual_check(A, sol, s, None, RATE, False, RTOL)
            print(name, seafloor, what, "residual", res, "bound", bound)
            assert res <= bound, (name, seafloor, what)


def test_a_dry_cell_inside_a_column_cuts_the_flux():
    v3D, area = K.gap_grid()
    wet, L3, N = K.wet_indices(v3D)
    assert N == sum(len(v) for v in K.GAP_WET.values()) == 16
    w = _w3d(v3D)
    for seafloor in K.SEAFLOORS:
        p, i, v = K.sink_ref(w, v3D, area, seafloor)
        A = _scipy(N, (p, i, v)).toarray()
        for (ci, cj), levels in K.GAP_WET.items():
            for k in levels:
                c = L3[ci, cj, k] - 1
                below = k + 1 in levels
                want = (w[ci, cj, k] * area[ci, cj]) / v3D[ci, cj, k]
                assert p[c + 1] - p[c] == (2 if below else 1), (seafloor, ci, cj, k)
                assert A[c, c] == (want if below or seafloor == "open" else 0.0)
                if below:
                    b = L3[ci, cj, k + 1] - 1
                    assert i[p[c]] == b + 1 and A[b, c] == -((w[ci, cj, k] * area[ci, cj]) / v3D[ci, cj, k + 1])
                # nothing else in the column, nothing from above a gap in the row
                assert np.count_nonzero(A[:, c]) == (2 if below else (1 if seafloor == "open" else 0))
                if k - 1 not in levels:
                    assert np.count_nonzero(A[c, :]) == np.count_nonzero(A[c, c])
    assert len(i) == N + 9  # the vertical pairs of GAP_WET: 4 + 2 + 2 + 0 + 0 + 1


def test_the_three_forms_of_w_give_the_same_bits_and_land_is_never_read():
    v3D, area = _case("tiny_tripolar")
    nz = v3D.shape[2]
    prof = W * np.linspace(0.5, 3.0, nz)
    garbage = np.where(np.isnan(v3D), np.nan, np.broadcast_to(prof, v3D.shape))
    for seafloor in K.SEAFLOORS:
        a, b = K.sink_ref(prof, v3D, area, seafloor), K.sink_ref(garbage, v3D, area, seafloor)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        a, b = K.sink_ref(W, v3D, area, seafloor), K.sink_ref(np.full(nz, W), v3D, area, seafloor)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    wet = ~np.isnan(v3D)
    for bad in (-1e-9, np.nan, np.inf):
        w = np.where(wet, W, np.nan)
        w[tuple(np.argwhere(wet)[7])] = bad
        with pytest.raises(K.BadSpeed):
            K.sink_ref(w, v3D, area)
    area2 = area.copy()
    area2[tuple(np.argwhere(wet[:, :, 0])[3])] = np.nan
    with pytest.raises(K.SinkNaN):
        K.sink_ref(W, v3D, area2)


def test_add_matrix_ref_goes_by_positions():
    """The first stored match wins, B's duplicates are added in B's order, a miss names the first offender and α = 0 still matches."""
    # a 3 x 3 operator whose column 0 stores rows (2, 0, 2): row 2 twice, unsorted (1-based: 3, 1, 3)
    p, i = np.array([1, 4, 5, 6]), np.array([3, 1, 3, 2, 3])
    values = [np.arange(1.0, 6.0), np.arange(10.0, 15.0)]
    B = (np.array([1, 3, 3, 4]), np.array([3, 3, 3]), np.array([0.5, 0.25, 2.0]))  # column 0 names row 3 twice
    out = K.add_matrix_ref(p, i, values, B, alpha=2.0, slots=[1])
    assert np.array_equal(out[0], values[0])
    assert np.array_equal(out[1], [(10.0 + 1.0) + 0.5, 11.0, 12.0, 13.0, 14.0 + 4.0])  # position 0 twice, the second (3, 0) never
    assert all(np.array_equal(a, b) for a, b in zip(K.add_matrix_ref(p, i, values, B, alpha=0.0), values))
    miss = (np.array([1, 2, 3, 4]), np.array([1, 1, 3]), np.ones(3))
    for alpha in (1.0, 0.0):
        with pytest.raises(K.PatternNotContained) as e:
            K.add_matrix_ref(p, i, values, miss, alpha=alpha)
        assert (e.value.entry, e.value.row, e.value.col) == (1, 1, 2)
    # against scipy where scipy's `+` means the same: sorted columns without duplicates
    T = R.dominant(40)
    A = R.csc_of(40, 40, *T)
    Bs = sp.csc_matrix(sp.diags(np.arange(1.0, 41.0)))
    got = K.add_matrix_ref(T[0], T[1], [T[2]], (Bs.indptr + 1, Bs.indices + 1, Bs.data), alpha=-0.5)[0]
    want = sp.csc_matrix(A + (-0.5) * Bs)
    want.sort_indices()
    assert np.array_equal(got, want.data)
