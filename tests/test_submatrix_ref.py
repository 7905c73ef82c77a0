"""CPU: the numpy restatement of otmb_op_submatrix (tests/submatrix_ref.py) is checked against what it restates without the library --
scipy's A[I][:, J] where rows are sorted and distinct, products of the parent on zero-padded vectors where they are not (stored order is
then what tells), api.vertical_lines of the grid with the dropped cells made land for the restricted lines -- and the exact Dirichlet
statement A_II·x_I = 1 is compared with the restoring route it replaces."""
import numpy as np
import pytest
import scipy.sparse as sp

import solve_lines_ref as LR
import solve_ref as R
import spmv_edges as E
import submatrix_ref as SUB
from spmv_ref import bits, spmv_ref


def _half(rng, limit):
    return np.sort(rng.choice(limit, size=limit // 2, replace=False)).astype(np.int64)


def _sorted_cases(oracle):
    out = {"dominant257": (257, *R.dominant(257)), "arrow600": (600, *R.arrow(600))}
    for name in ("odd_nx_fold", "tiny_tripolar"):
        T, N, _ = R.grid_T(oracle, name)
        out[name] = (N, *T)
    return out


def test_first_offender_states_the_refusals():
    assert SUB.first_offender([1, 2, 5], 5) is None and SUB.first_offender([], 5) is None
    assert SUB.first_offender([0, 2], 5) == 0 and SUB.first_offender([1, 6], 5) == 1
    assert SUB.first_offender([1, 4, 3, 2], 5) == 2 and SUB.first_offender([2, 2], 5) == 1


def test_restatement_is_scipy_indexing_on_sorted_distinct_rows(oracle):
    for name, (n, p, i, v) in _sorted_cases(oracle).items():
        A = sp.csc_matrix((v, i - 1, p - 1), shape=(n, n))
        rng = np.random.default_rng(41)
        sels = [(np.arange(n), np.arange(n)), (_half(rng, n), _half(rng, n)), (np.arange(1, n), np.arange(1, n)), (np.array([n // 2]), np.arange(n)),
                (np.zeros(0, dtype=np.int64), np.arange(n)), (np.arange(n), np.zeros(0, dtype=np.int64))]
        for rows, cols in sels:
            cpc, rvc, src = SUB.submatrix_ref(n, n, p, i, rows, cols)
            want = sp.csc_matrix(A[rows][:, cols])
            want.sort_indices()
            assert cpc[0] == 1 and len(cpc) == len(cols) + 1 and cpc[-1] - 1 == len(rvc) == len(src), name
            assert np.array_equal(cpc - 1, want.indptr) and np.array_equal(rvc - 1, want.indices), name
            assert np.array_equal(SUB.submatrix_values(v, src).view(np.int64), want.data.view(np.int64)), name


@pytest.mark.parametrize("name", ["mixed", "size_63x65", "size_129x127", "abs257", "cols_straddle", "long513"])
def test_restatement_keeps_stored_order_on_unsorted_and_duplicate_rows(name):
    """The products of the restated submatrix have the bits of the parent's products on zero-padded vectors, in every output element whose
    dropped terms are all ±0.0 (a dropped NaN or ±Inf entry times zero would be NaN in the parent's fold): a fold from +0.0 does not see
    added zeros, so only the ORDER of the kept terms can tell the two apart."""
    f = E.fixtures()[name]
    m, n, p, i, v = f.A
    nnz = int(p[-1] - 1)
    rng = np.random.default_rng(43)
    rows, cols = _half(rng, m), _half(rng, n)
    cpc, rvc, src = SUB.submatrix_ref(m, n, p, i, rows, cols)
    vc = SUB.submatrix_values(v, src)
    col = np.repeat(np.arange(n), np.diff(p))
    rv = np.asarray(i)[:nnz] - 1
    rsel, csel = np.zeros(m, dtype=bool), np.zeros(n, dtype=bool)
    rsel[rows], csel[cols] = True, True
    wild = ~np.isfinite(np.asarray(v)[:nnz])
    # A·x: row i is comparable when no non-finite entry of it lies in a dropped column; Aᵀ·x: column j likewise for dropped rows
    row_ok = np.bincount(rv[wild & ~csel[col]], minlength=m)[rows] == 0
    col_ok = np.bincount(col[wild & ~rsel[rv]], minlength=n)[cols] == 0
    assert row_ok.sum() > len(rows) // 2 and col_ok.sum() > len(cols) // 2
    x = rng.standard_normal((len(cols), 2)) * 10.0 ** rng.integers(-3, 4, (len(cols), 2))
    xp = np.zeros((n, 2))
    xp[cols] = x
    got, want = spmv_ref(len(rows), len(cols), cpc, rvc, vc, x), spmv_ref(m, n, p, i, v, xp)[rows]
    assert np.array_equal(bits(got[row_ok]), bits(want[row_ok]))
    y = rng.standard_normal((len(rows), 2)) * 10.0 ** rng.integers(-3, 4, (len(rows), 2))
    yp = np.zeros((m, 2))
    yp[rows] = y
    got, want = spmv_ref(len(rows), len(cols), cpc, rvc, vc, y, adjoint=True), spmv_ref(m, n, p, i, v, yp, adjoint=True)[cols]
    assert np.array_equal(bits(got[col_ok]), bits(want[col_ok]))
    # ... and the order does tell on this fixture: the reversed fold of the child's kept terms differs somewhere
    child = E.Fixture(name="child", m=len(rows), n=len(cols), colptr=cpc, rowval=rvc, nzval=np.where(np.isfinite(vc), vc, 1.0),
                      focus={"rows": np.arange(len(rows)), "cols": np.arange(len(cols))})
    assert E.order_sensitive(child, "rows") + E.order_sensitive(child, "cols") > 0


def _grid_lines(oracle, name):
    from helpers import make_case
    from otmb_amd import api

    idx = oracle.makeindices(make_case(name)[1].v3D)
    return np.asarray(idx["Lwet3D"], dtype=np.int64), int(idx["N"]), api.vertical_lines(idx)


@pytest.mark.parametrize("which", ["surface", "random30"])
def test_restricted_lines_are_the_lines_of_the_grid_with_the_dropped_cells_made_land(oracle, which):
    from otmb_amd import api

    L, N, nxt = _grid_lines(oracle, "odd_nx_fold")
    nsurf = int(np.count_nonzero(L[:, :, 0] > 0))
    if which == "surface":
        sel = np.arange(nsurf, N)
    else:
        sel = np.flatnonzero(np.random.default_rng(47).random(N) >= 0.3)
    got = SUB.restrict_lines(nxt, sel)
    LR.successors(got, len(sel))  # otmb_op_set_lines' rules: raises otherwise
    rank = SUB.ranks(sel, N)
    L2 = np.where(L > 0, rank[np.maximum(L, 1) - 1] + 1, 0)  # the dropped cells are land, the others keep their order
    want = api.vertical_lines({"Lwet3D": L2, "N": len(sel)})
    assert np.array_equal(got, want)
    assert np.count_nonzero(got) < np.count_nonzero(nxt) and np.count_nonzero(got) > 0


def test_dirichlet_is_the_limit_of_the_restoring_route(oracle):
    """x_B = 0 on the level-1 cells, A_II·x_I = 1 solved densely, against (diag(d) + A)·x = 1 with d = 1e-3, 1, 1e3 s⁻¹ there: the restoring
    answers come closer as d grows.  No library number takes part.  Measured relative distance: 7.9e-05, 7.9e-08 (d = 1, the README's rate) and 7.9e-11 -- first order in 1/d."""
    (p, i, v), N, nsurf = R.grid_T(oracle, "odd_nx_fold")
    inner = np.arange(nsurf, N)
    cpc, rvc, src = SUB.submatrix_ref(N, N, p, i, inner, inner)
    AII = sp.csc_matrix((SUB.submatrix_values(v, src), rvc - 1, cpc - 1), shape=(len(inner), len(inner))).toarray()
    xd = np.linalg.solve(AII, np.ones(len(inner)))
    A = sp.csc_matrix((v, i - 1, p - 1), shape=(N, N)).toarray()
    dist = []
    for rate in (1e-3, 1.0, 1e3):
        d = np.zeros(N)
        d[:nsurf] = rate
        x = np.linalg.solve(np.diag(d) + A, np.ones(N))
        dist.append(np.linalg.norm(x[inner] - xd) / np.linalg.norm(xd))
        print(f"restoring d = {rate:g} on the level-1 cells: relative distance to the Dirichlet answer {dist[-1]:.3e}")
    assert dist[0] > dist[1] > dist[2]
