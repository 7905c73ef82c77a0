"""CPU: tests/spmv_ref.py, the numpy restatement of SparseArrays' 5-argument mul! (Julia 1.10), against a literal triple loop, and a check
that the restatement visibly carries the summation order."""
import itertools

import numpy as np
import pytest

from spmv_ref import bits, random_csc, random_dense, spmv_loop, spmv_ref

ALPHAS = (1.0, 0.0, 2.5)
BETAS = (0.0, 1.0, -0.5)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("adjoint", [False, True])
def test_restatement_equals_the_triple_loop(seed, adjoint):
    rng = np.random.default_rng(seed)
    m, n = int(rng.integers(1, 9)), int(rng.integers(1, 9))
    p, i, v = random_csc(rng, m, n)
    assert np.all(np.diff(p) >= 0)
    for k, alpha, beta in itertools.product((1, 3), ALPHAS, BETAS):
        rx, ry = (m, n) if adjoint else (n, m)
        X = random_dense(rng, rx, k)
        Y = random_dense(rng, ry, k)
        if k == 1:
            X, Y = X[:, 0], Y[:, 0]
        want = spmv_loop(m, n, p, i, v, X, alpha, beta, Y, adjoint)
        got = spmv_ref(m, n, p, i, v, X, alpha, beta, Y, adjoint)
        assert got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), (seed, k, alpha, beta)


def test_the_cases_the_device_tests_rely_on_occur():
    """The random matrices really hold duplicate and unsorted rows, empty rows and columns, stored zeros, -0.0, NaN and Inf."""
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(20):
        p, i, v = random_csc(rng, 8, 8)
        for c in range(8):
            r = i[p[c] - 1:p[c + 1] - 1]
            if len(set(r)) < len(r):
                seen.add("dup")
            if np.any(np.diff(r) < 0):
                seen.add("unsorted")
            if len(r) == 0:
                seen.add("empty column")
        if len(set(i)) < 8:
            seen.add("empty row")
        if np.any((v == 0) & ~np.signbit(v)):
            seen.add("+0")
        if np.any((v == 0) & np.signbit(v)):
            seen.add("-0")
        if np.any(np.isnan(v)):
            seen.add("nan")
        if np.any(np.isinf(v)):
            seen.add("inf")
    assert seen == {"dup", "unsorted", "empty column", "empty row", "+0", "-0", "nan", "inf"}


def test_beta_zero_discards_and_the_fold_starts_from_the_beta_value():
    p, i, v = np.array([1, 2, 3]), np.array([1, 1]), np.array([-0.0, 3.0])
    Y = np.array([np.nan, np.inf])
    # A·x: row 1 = (+0.0 from the β step) + (-0.0 * 1.0) + ... ; row 2 is empty: only the β step
    got = spmv_ref(2, 2, p, i, v, np.array([1.0, 0.0]), 1.0, 0.0, Y)
    assert got[0] == 0.0 and not np.signbit(got[0])  # +0.0 + -0.0 + 0.0 = +0.0
    assert got[1] == 0.0 and not np.signbit(got[1])  # β == 0 discards the Inf
    got = spmv_ref(2, 2, np.array([1, 2, 2]), np.array([1]), np.array([-0.0]), np.array([1.0, 1.0]), 1.0, 0.0)
    assert got[0] == 0.0 and not np.signbit(got[0])  # never "copy the first product" (-0.0)
    # Aᵀ·x of an empty column: Y + (+0.0) * α -- NaN when α is Inf
    got = spmv_ref(2, 2, np.array([1, 1, 1]), np.array([], dtype=np.int64), np.array([]), np.ones(2), np.inf, 1.0, np.array([1.0, 2.0]),
                   adjoint=True)
    assert np.all(np.isnan(got))
    # β == 1 keeps NaN, other β scale it
    got = spmv_ref(2, 2, np.array([1, 1, 1]), np.array([], dtype=np.int64), np.array([]), np.ones(2), 1.0, 1.0, np.array([np.nan, 2.0]))
    assert np.isnan(got[0]) and got[1] == 2.0
    got = spmv_ref(2, 2, np.array([1, 1, 1]), np.array([], dtype=np.int64), np.array([]), np.ones(2), 1.0, -0.5, np.array([4.0, 2.0]))
    assert list(got) == [-2.0, -1.0]


def test_a_reordered_sum_differs_in_the_last_bit():
    """The restatement carries the order: one row whose contributions, summed in storage order and in a flat reversed order, differ."""
    vals = np.array([1.0, 1e-16, -1.0])
    p, i = np.array([1, 2, 3, 4]), np.array([1, 1, 1])
    x = np.ones(3)
    got = spmv_ref(1, 3, p, i, vals, x)
    assert np.array_equal(bits(got), bits(spmv_loop(1, 3, p, i, vals, x)))
    flat = 0.0
    for t in (vals * x)[::-1]:
        flat = flat + t
    assert got[0] == 0.0 and flat != got[0]
    # the same through a random matrix: some reordering of a long row changes the last bit
    rng = np.random.default_rng(3)
    n = 200
    vals = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
    p, i = np.arange(1, n + 2), np.ones(n, dtype=np.int64)
    x = rng.standard_normal(n)
    got = spmv_ref(1, n, p, i, vals, x)[0]
    perm = rng.permutation(n)
    other = 0.0
    for t in (vals * x)[perm]:
        other = other + t
    assert other != got
