"""What the per-column-d tests (tests/test_dk_*.py) share: the D of seven mutually different columns, the operator with the tests' three
slots, and the comparison of one per-column call with the k = 1 calls it must equal bit for bit (include/otmb.h: column c of a per-column
call has the bits of the existing call made with k = 1, that column of B / S / X / x0, and d = D[:, c])."""
import numpy as np

import solve_ref as R
from spmv_ref import bits

LAMBDA = 2.0e-7  # the decay rate of the "radiocarbon" column, s⁻¹ (tests/test_dk_periodic.py says how it was chosen)
K = 7            # register blocks 4 + 2 + 1: a column's place in its block varies


def columns(N, nsurf, zero, lam=LAMBDA, seed=77):
    """D (N x 7, Fortran order): the age d (1 s⁻¹ on the surface cells); that d times 1e-5; that d plus λ on every cell; a random non-negative
    column on top of it; an all-zero column (zero=True: only where σ > 0 makes that regular; otherwise half the age d); and two more mixes."""
    age = R.shift("age", N, nsurf)[0]
    rng = np.random.default_rng(seed)
    cols = [age, 1e-5 * age, age + lam, age + 1e-6 * rng.uniform(0.0, 1.0, N), np.zeros(N) if zero else 0.5 * age,
            2.0 * age + 1e-7 * rng.uniform(0.0, 1.0, N), age + 0.25 * lam]
    D = np.asfortranarray(np.stack(cols, axis=1))
    assert D.shape == (N, K) and (D >= 0).all()
    assert all(not np.array_equal(D[:, a], D[:, b]) for a in range(K) for b in range(a))
    return D


def same_bits(a, b, what):
    assert np.array_equal(bits(np.asarray(a, dtype=np.float64)), bits(np.asarray(b, dtype=np.float64))), what


def rhs(N, k, seed):
    B = np.ones((N, k), order="F")
    B[:, 1:] = np.random.default_rng(seed).standard_normal((N, k - 1))
    return B
