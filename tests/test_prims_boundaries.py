"""The shared scan, sort and key-width code (csrc/otmb_prims.*) through its callers, where one merged copy can go wrong where four could not:
the width of a sort key when the largest value is one below, at and one above a power of two, and the caller's temporary buffer when a small
call follows a large one on the same context.  Every result equals its CPU reference exactly; there are no tolerances.

The helpers are internal (no export): sparse() sizes its keys from m and n, the operator plan from its rows m, coarsen's sorted path from
its coarse rows m, lump_and_spray's fill from the number of coarse cells Nc.  Each case has an entry in the last row and the last column, so a
key one bit too narrow loses it.  Empty inputs are asserted where each caller is tested (test_general_path, test_spmv, test_submatrix,
test_coarsen)."""
import numpy as np
import pytest

import lump_grids
from helpers import assert_csc_equal
from spmatmul_ref import coarse_ref
from spmv_ref import bits, spmv_ref
from test_coarsen import _same as _same_coarse
from test_lump_and_spray import _same as _same_lump

pytestmark = pytest.mark.gpu

WIDTHS = (255, 256, 257, 65535, 65536)
LUMP_GRIDS = {255: (17, 15, 1), 256: (16, 16, 1), 257: (257, 1, 1)}  # all wet, 1 x 1 x 1 blocks: Nc = the number of cells


def _csc(m, n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(m, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


def _triplets(v, ln, seed):
    """ln triplets of a v x v matrix with duplicates, the corner (v, v) twice, the first and the last row and column in use."""
    rng = np.random.default_rng(seed)
    I, J = rng.integers(1, v + 1, ln), rng.integers(1, v + 1, ln)
    I[: ln // 4], J[: ln // 4] = I[ln // 4: 2 * (ln // 4)], J[ln // 4: 2 * (ln // 4)]  # duplicates, apart in the input
    I[-4:], J[-4:] = (v, v, 1, v), (v, v, v, 1)
    perm = rng.permutation(ln)
    return I[perm], J[perm], rng.standard_normal(ln)[perm]


def _sparse_case(asm, oracle, v, ln, seed, what):
    import torch

    I, J, V = _triplets(v, ln, seed)
    cp, rv, nz = asm.sparse(torch.from_numpy(I).cuda(), torch.from_numpy(J).cuda(), torch.from_numpy(V).cuda(), v, v)
    got = (cp.cpu().numpy(), rv.cpu().numpy(), nz.cpu().numpy())
    assert got[0][-1] - 1 == got[1].size and got[1][-1] == v  # the corner is the last stored entry
    assert_csc_equal(got, oracle.sparse(I, J, V, v, v), what)


@pytest.fixture(scope="module")
def asm():
    from otmb_amd.device import DeviceAssembler

    return DeviceAssembler(0)


@pytest.mark.parametrize("v", WIDTHS)
def test_sparse_key_width(oracle, asm, v):
    _sparse_case(asm, oracle, v, 48, v, ("sparse", v))


@pytest.mark.parametrize("v", WIDTHS)
def test_operator_key_width(v):
    """A v x 3 operator: the plan's stable transposition sorts by row over the bits v needs."""
    import otmb_amd.api as api

    rng = np.random.default_rng(v)
    rows = [np.sort(rng.choice(np.arange(1, v + 1), 12, replace=False)) for _ in range(3)]
    for r in rows:
        r[-1] = v  # the last row, in every column (the last one included)
    rows[0][0] = 1
    A = _csc(v, 3, [1, 13, 25, 37], np.concatenate(rows), rng.standard_normal(36))
    with api.DeviceOperator(A) as D:
        for adjoint in (False, True):
            X = rng.standard_normal((v if adjoint else 3, 2))
            want = spmv_ref(v, 3, A.colptr, A.rowval, A.nzval, X, 1.0, 0.0, None, adjoint)
            got = np.asarray(D.mul(np.asfortranarray(X), adjoint=adjoint))
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (v, adjoint)


@pytest.mark.parametrize("v", WIDTHS)
def test_coarsen_sorted_path_key_width(v):
    """v coarse rows on the sorted path, reached as test_coarsen_large_columns reaches it: one SPRAY column whose work (the entries of T in its
    fine columns: 3 N - 2 = 2398) exceeds the 2048 contributions the small path holds."""
    import otmb_amd.api as api

    rng = np.random.default_rng(v)
    N = 800
    lrow = rng.integers(1, v + 1, N)
    lrow[[0, N // 2, N - 1]] = (v, 1, v)  # the last coarse row from the first and the last fine cell
    L = _csc(v, N, np.arange(1, N + 2), lrow, rng.standard_normal(N))
    tp = np.concatenate([[1], 1 + np.cumsum([2] + [3] * (N - 2) + [2])])
    ti = np.concatenate([np.arange(max(1, c - 1), min(N, c + 1) + 1) for c in range(1, N + 1)])
    T = _csc(N, N, tp, ti, rng.standard_normal(ti.size))
    S = _csc(N, 2, [1, N + 1, N + 4], np.concatenate([np.arange(1, N + 1), [1, N // 2, N]]), rng.standard_normal(N + 3))
    want = coarse_ref(L, T, S)
    assert want[3][-1] == v and want[2][1] - 1 < want[2][2] - 1  # the last row is stored, in the last column too
    _same_coarse(api.coarsen(L, T, S), want, ("coarsen", v))


def _lump_case(oracle, v, what):
    import otmb_amd.api as api

    wet = np.ones(LUMP_GRIDS[v], dtype=bool, order="F")
    tm = lump_grids.neighbour_pattern(wet, None, keep=1.0, periodic_i=False)
    vol = np.random.default_rng(v).uniform(1.0, 2.0, v)
    want = oracle.lump_and_spray(wet, vol, tm, None, 1, 1, 1)
    assert len(want[2]) == v  # Nc = v: the fill's sort runs over the bits v needs
    got = api.lump_and_spray(wet, vol, api.SparseMatrixCSC(v, v, *tm), None, di=1, dj=1, dk=1)
    _same_lump(got, want, what)


@pytest.mark.parametrize("v", sorted(LUMP_GRIDS))
def test_lump_and_spray_key_width(oracle, v):
    _lump_case(oracle, v, ("lump", v))


def test_temporaries_that_grow_and_shrink(oracle, asm):
    """Smallest, largest, smallest on one context: the second small call finds rocPRIM's temporary (and every scratch array) larger than it needs."""
    for v in (255, 257, 255):
        _lump_case(oracle, v, ("lump, in turn", v))
    for v, ln in ((255, 48), (65536, 20000), (255, 48)):
        _sparse_case(asm, oracle, v, ln, v, ("sparse, in turn", v, ln))
