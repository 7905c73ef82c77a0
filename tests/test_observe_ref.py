"""CPU: tests/observe_ref.py, the restatement the GPU tests of otmb_op_observe and otmb_op_step_obs compare bits with, checked without the
library: against math.fsum within the bound the order itself gives, against a plain three-loop statement of the order over Python floats,
and on one input on which that order and a flat left-to-right sum differ -- so a bit comparison with it does say something about the order."""
import math

import numpy as np
import pytest

import observe_ref as OR

SIZES = [1, 2, 511, 512, 513, 2047, 2048, 2049, 2050, 4097]


@pytest.mark.parametrize("n", SIZES)
def test_within_the_orders_own_bound_of_fsum(n):
    """Each product passes through at most roundings(n) additions -- 8 in the lane, 6 shuffle levels, 3 wave additions, one per further
    partial -- so |sum - exact| <= roundings·2⁻⁵³·Σ|w·x| to first order; math.fsum of the same (rounded) products is the exact sum, rounded."""
    rng = np.random.default_rng(n)
    W, X = rng.standard_normal((n, 3)), rng.standard_normal((n, 2)) * 10.0 ** rng.integers(-3, 4, (n, 2))
    obs = OR.observe_ref(W, X)
    assert obs.shape == (3, 2)
    for j in range(3):
        for c in range(2):
            prod = W[:, j] * X[:, c]
            exact, bound = math.fsum(prod), OR.roundings(n) * 2.0 ** -53 * math.fsum(np.abs(prod))
            print(n, j, c, "error", abs(obs[j, c] - exact), "bound", bound)
            assert abs(obs[j, c] - exact) <= bound


def _three_loops(prod):
    n = len(prod)
    parts = []
    for wg in range(OR.workgroups(n)):
        lanes = []
        for t in range(256):
            acc = 0.0
            for p in range(4):
                i = 2 * (wg * 1024 + t + 256 * p)
                if i >= n:
                    break
                acc = acc + float(prod[i])
                if i + 1 < n:
                    acc = acc + float(prod[i + 1])
            lanes.append(acc)
        waves = []
        for w in range(4):
            x = lanes[64 * w:64 * w + 64]
            for dist in (32, 16, 8, 4, 2, 1):
                x = [x[l] + x[l ^ dist] for l in range(64)]
            waves.append(x[0])
        parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    if not parts:
        return 0.0
    s = parts[0]
    for b in parts[1:]:
        s = s + b
    return s


@pytest.mark.parametrize("n", [0, 1, 2, 513, 2049, 4097])
def test_the_vectorised_restatement_is_the_order_written_out(n):
    rng = np.random.default_rng(100 + n)
    W, X = rng.standard_normal((n, 2)), rng.standard_normal((n, 2))
    obs = OR.observe_ref(W, X)
    for j in range(2):
        for c in range(2):
            assert float(obs[j, c]).hex() == float(_three_loops(W[:, j] * X[:, c])).hex(), (n, j, c)
    if n == 0:
        assert not np.signbit(obs).any()


def test_the_order_shows_in_the_last_bit():
    """One input on which the device's order and a left-to-right sum give different doubles."""
    rng = np.random.default_rng(7)
    w, x = rng.standard_normal(4097), rng.standard_normal(4097)
    a, b = float(OR.observe_ref(w, x)[0, 0]), OR.flat_sum(w * x)
    print(a.hex(), b.hex())
    assert a != b and abs(a - b) <= 2.0 ** -40 * abs(a)


def test_signed_zeros_and_the_means_fold():
    n = 2050
    obs = OR.observe_ref(np.full((n, 2), -0.0), np.ones((n, 3)))
    assert (obs == 0).all() and not np.signbit(obs).any()  # +0.0 + -0.0 = +0.0 all the way up
    X = [np.array([1.0, -0.0, 3.0]), np.array([0.1, 0.0, -3.0])]
    tw = [0.5, 0.25]
    m = OR.mean_ref(X, tw)
    assert OR.same_values(m, (0.0 + 0.5 * X[0]) + 0.25 * X[1]) and not np.signbit(m[1])
    assert OR.mean_ref([], []) is None
    assert OR.same_values([np.nan, 1.0], [-np.nan, 1.0]) and not OR.same_values([0.0], [-0.0])
