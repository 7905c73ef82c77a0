"""CPU: the numpy restatement of spmatmul / LUMP * T * SPRAY (tests/spmatmul_ref.py) that the GPU tests of coarsen compare
against -- its values against scipy, its pattern against the structural product, and its two-level summation order."""
import numpy as np
import scipy.sparse as sp

from spmatmul_ref import coarse_ref, flat_ref, spmatmul


def _csc(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return (M.shape[0], M.shape[1], M.indptr.astype(np.int64) + 1, M.indices.astype(np.int64) + 1, M.data.astype(np.float64))


def _scipy(X):
    m, n, p, i, v = X
    return sp.csc_matrix((v, i - 1, p - 1), shape=(m, n))


def _lump(rng, m, N, empty=0.0):
    rows = rng.integers(0, m, N)
    keep = rng.random(N) >= empty
    L = sp.csc_matrix((rng.uniform(0.1, 1.0, keep.sum()), (rows[keep], np.flatnonzero(keep))), shape=(m, N))
    return _csc(L)


def test_spmatmul_matches_scipy_on_random_matrices():
    rng = np.random.default_rng(11)
    for q in range(20):
        m, N, M, n = (int(x) for x in rng.integers(1, 40, 4))
        A = _csc(sp.random(m, N, density=rng.uniform(0.0, 0.5), random_state=rng, data_rvs=lambda k: rng.normal(size=k)))
        B = _csc(sp.random(N, M, density=rng.uniform(0.0, 0.5), random_state=rng, data_rvs=lambda k: rng.normal(size=k)))
        C = spmatmul(A, B)
        assert C[:2] == (m, M)
        assert np.allclose(_scipy(C).toarray(), (_scipy(A) @ _scipy(B)).toarray(), rtol=1e-13, atol=1e-13), q
        L = _lump(rng, m, N, empty=0.2)
        S = _csc(sp.random(M, n, density=rng.uniform(0.0, 0.6), random_state=rng, data_rvs=lambda k: rng.normal(size=k)))
        Cc = coarse_ref(L, B, S)
        want = (_scipy(L) @ _scipy(B)) @ _scipy(S)
        assert Cc[:2] == (m, n)
        assert np.allclose(_scipy(Cc).toarray(), want.toarray(), rtol=1e-13, atol=1e-13), q
        # rows ascending inside every column
        p, i = Cc[2], Cc[3]
        for c in range(n):
            assert np.all(np.diff(i[p[c] - 1: p[c + 1] - 1]) > 0)


def test_pattern_is_the_structural_product_including_exact_cancellation():
    rng = np.random.default_rng(5)
    N, m = 30, 8
    L = _lump(rng, m, N)
    Tm = sp.random(N, N, density=0.2, random_state=rng, format="csc") + sp.identity(N, format="csc")
    Tm = sp.csc_matrix(Tm)
    Tm.sort_indices()
    Tm.data = rng.normal(size=Tm.nnz)
    S = _csc(_scipy(L).T.astype(bool).astype(np.float64))
    T = _csc(Tm)
    C = coarse_ref(L, T, S)
    pattern = (abs(_scipy(L)).astype(bool).astype(float) @ abs(_scipy(T)).astype(bool).astype(float)
               @ abs(_scipy(S)).astype(bool).astype(float))
    pattern = sp.csc_matrix(pattern)
    pattern.sort_indices()
    assert np.array_equal(C[2], pattern.indptr + 1) and np.array_equal(C[3], pattern.indices + 1)
    # exact cancellation: LUMP = [1 1], T = [1 ; -1] in one column, SPRAY = 1 -> the zero is STORED
    L2 = (1, 2, np.array([1, 2, 3]), np.array([1, 1]), np.array([1.0, 1.0]))
    T2 = (2, 1, np.array([1, 3]), np.array([1, 2]), np.array([0.5, -0.5]))
    S2 = (1, 1, np.array([1, 2]), np.array([1]), np.array([1.0]))
    C2 = coarse_ref(L2, T2, S2)
    assert list(C2[2]) == [1, 2] and list(C2[3]) == [1] and C2[4][0] == 0.0 and not np.signbit(C2[4][0])
    # a lone -0.0 survives (first touch copies; 0.0 + -0.0 would give +0.0)
    T3 = (2, 1, np.array([1, 2]), np.array([2]), np.array([-0.0]))
    C3 = coarse_ref(L2, T3, S2)
    assert C3[4][0] == 0.0 and np.signbit(C3[4][0])


def test_two_level_order_differs_from_a_flat_sum_and_the_restatement_gives_the_two_level_value():
    # one coarse row, SPRAY's column holds fine columns 1 and 2; T[:,1] = (1.0), T[:,2] = (2^-53, 2^-53) in two fine rows that
    # LUMP sends to the same coarse row.  Two levels: 1.0 + (2^-53 + 2^-53) = 1 + 2^-52.  Flat: (1.0 + 2^-53) + 2^-53 = 1.0.
    e = 2.0 ** -53
    L = (1, 3, np.array([1, 2, 3, 4]), np.array([1, 1, 1]), np.array([1.0, 1.0, 1.0]))
    T = (3, 2, np.array([1, 2, 4]), np.array([1, 2, 3]), np.array([1.0, e, e]))
    S = (2, 1, np.array([1, 3]), np.array([1, 2]), np.array([1.0, 1.0]))
    C = coarse_ref(L, T, S)
    flat = flat_ref(L, T, S)[(0, 0)]
    assert C[4][0] == 1.0 + 2.0 ** -52
    assert flat == 1.0
    assert C[4][0] != flat
