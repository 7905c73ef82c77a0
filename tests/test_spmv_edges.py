"""GPU: the resident sparse operator (csrc/otmb_spmv.hip) at its layout thresholds, every tracer split, padded leading dimensions and more
than 2^24 rows and columns, against tests/spmv_ref.py by bit pattern (any NaN equals any NaN): A·X and Aᵀ·X, through the host API
(api.DeviceOperator, otmb_op_mul) and the device one (device.Operator, otmb_op_mul_dev).  The fixtures, and which side of each threshold
they lie on, are in tests/spmv_edges.py (checked on the CPU by tests/test_spmv_edges_ref.py).  These tests check results only, never
which path a row took."""
import itertools

import numpy as np
import pytest

import spmv_edges as E
from spmv_ref import bits, random_dense, spmv_ref
from test_spmv import _csc, _same

pytestmark = pytest.mark.gpu

ALPHAS = (1.0, 2.5, -0.0)
BETAS = (0.0, -0.0, 1.0, -0.5, np.nan)
PADS = (1, 5, 64)
PAD_FIXTURES = ("mixed", "size_64x64", "size_256x256", "long1025", "cols_straddle")  # square ones, long rows, Aᵀ runs across chunk edges
SENTINEL = np.int64(0x5A5A5A5A5A5A5A5A).view(np.float64)


@pytest.fixture(scope="module")
def asm():
    from otmb_amd.device import DeviceAssembler

    return DeviceAssembler(0)  # (its context runs on torch's current stream)


def _dev(a):
    """A column-major device copy of a host array (1-D or 2-D)."""
    import torch

    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        return torch.from_numpy(a.copy()).cuda()
    return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t()


class _Pair:
    """The host operator (api.DeviceOperator) and the device one (device.Operator) over the same matrix A = (m, n, colptr, rowval, nzval)."""

    def __init__(self, asm, m, n, p, i, v):
        import torch

        import otmb_amd.api as api
        from otmb_amd.device import Operator

        self.A = (m, n, p, i, v)
        self.host = api.DeviceOperator(_csc(m, n, p, i, v))
        self.dev = Operator(asm.ctx, m, n, *(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (p, i, v)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.host.close()
        self.dev.close()


def _y0(rng, ry, k, beta):
    """Y before the call: NaN, +Inf and -Inf where β is 0 or -0.0 (the β step must discard them); values with specials otherwise."""
    if beta == 0:
        return np.asfortranarray(np.resize(np.array([np.nan, np.inf, -np.inf]), ry * k).reshape(ry, k, order="F"))
    return random_dense(rng, ry, k)


def _x(rng, rows, k):
    """X with NaN, ±Inf and ±0.0 (random_dense) in odd tracers and finite values in even ones (k = 1: either kind).  One NaN or Inf among
    a long row's columns decides that row whatever the order of its fold: the finite tracers are the ones that check the order."""
    X = random_dense(rng, rows, k)
    keep = np.arange(k) % 2 == 0 if k > 1 else np.array([rng.random() < 0.5])
    X[:, keep] = random_dense(rng, rows, k, specials=False)[:, keep]
    return X


def _check(P, rng, adjoint, k, alpha, beta, what, X=None):
    """One product through both APIs, compared with the restatement; returns the restatement's result."""
    m, n = P.A[:2]
    rx, ry = (m, n) if adjoint else (n, m)
    X = _x(rng, rx, k) if X is None else X
    Y = _y0(rng, ry, k, beta)
    if k == 1:
        X, Y = X[:, 0], Y[:, 0]
    want = spmv_ref(*P.A, X, alpha, beta, Y, adjoint)
    what = (what, "Aᵀ" if adjoint else "A", k, alpha, beta)
    _same(np.asarray(P.host.mul(X, alpha=alpha, beta=beta, Y=np.array(Y, order="F"), adjoint=adjoint)), want, ("host",) + what)
    Yd = _dev(Y)
    P.dev.mul(_dev(X), alpha=alpha, beta=beta, Y=Yd, adjoint=adjoint)
    _same(Yd.cpu().numpy(), want, ("device",) + what)
    return want


@pytest.mark.parametrize("name", E.THRESHOLD_FIXTURES)
def test_threshold_fixture(asm, name):
    """Each fixture of a threshold pair (spmv_edges.PAIRS): k in {1, 3, 8}, and 63, 64, 65, 128, 129 where a row is long; every α and β."""
    f = E.fixtures()[name]
    ks = E.K_BASE + (E.K_LONG if "long" in f.focus else ())
    rng = np.random.default_rng(sum(map(ord, name)))
    with _Pair(asm, *f.A) as P:
        for adjoint, k, alpha, beta in itertools.product((False, True), ks, ALPHAS, BETAS):
            _check(P, rng, adjoint, k, alpha, beta, name)


def test_every_tracer_split(asm):
    """k = 1 ... 17 and 24 (every split into register blocks of 8, 4, 2 and 1) on `mixed`: short rows, a long row, an Aᵀ run longer
    than 512, a partial last slice and a partial last wave."""
    f = E.fixtures()["mixed"]
    rng = np.random.default_rng(17)
    with _Pair(asm, *f.A) as P:
        for adjoint, k, (alpha, beta) in itertools.product((False, True), E.K_SPLITS, ((1.0, 0.0), (2.5, -0.5), (-0.0, 1.0))):
            _check(P, rng, adjoint, k, alpha, beta, "mixed")


@pytest.mark.parametrize("px,py", list(itertools.product(PADS, PADS)))
@pytest.mark.parametrize("name", PAD_FIXTURES)
def test_padded_leading_dimensions(asm, name, px, py):
    """X and Y are column-major views into tensors with px and py more rows: ldx = rows + px, ldy = rows + py (square matrices with
    px > py have ldy < ldx).  X's padding is NaN; Y's holds a sentinel whose bits must stay.  k = 1 goes to otmb_op_mul_dev directly
    (device.Operator passes ld = rows for one column); k = 3 and k = 9 (a block of 8, then 1) through device.Operator.mul, which must
    hand the views over uncopied."""
    import torch

    from otmb_amd.device import _col_major

    f = E.fixtures()[name]
    rng = np.random.default_rng(100 * px + py)
    with _Pair(asm, *f.A) as P:
        for adjoint, k, (alpha, beta) in itertools.product((False, True), (1, 3, 9), ((2.5, -0.5), (1.0, 0.0))):
            rx, ry = (f.m, f.n) if adjoint else (f.n, f.m)
            X, Y = _x(rng, rx, k), _y0(rng, ry, k, beta)
            want = spmv_ref(*f.A, X, alpha, beta, Y, adjoint)
            Xb = torch.full((k, rx + px), np.nan, dtype=torch.float64, device="cuda").t()
            Yb = torch.full((k, ry + py), SENTINEL, dtype=torch.float64, device="cuda").t()
            Xb[:rx] = _dev(X)
            Yb[:ry] = _dev(Y)
            what = (name, px, py, "Aᵀ" if adjoint else "A", k, alpha, beta)
            if k == 1:
                asm.ctx.check(P.dev.lib.otmb_op_mul_dev(P.dev.handle, int(adjoint), 1, Xb.data_ptr(), rx + px, Yb.data_ptr(), ry + py, alpha,
                                                        beta))
            else:
                Xv, Yv = Xb[:rx], Yb[:ry]
                assert _col_major(Xv, rx)[1] == rx + px and _col_major(Yv, ry)[1] == ry + py, what
                P.dev.mul(Xv, alpha=alpha, beta=beta, Y=Yv, adjoint=adjoint)
            out = Yb.cpu().numpy()
            _same(out[:ry], want, what)
            assert np.all(out[ry:].view(np.int64) == SENTINEL.view(np.int64)), (what, "padding rows of Y were written")


@pytest.mark.parametrize("name", sorted(E.fixtures()))
def test_alpha_zero_with_infinities_in_x(asm, name):
    """α = 0 and α = -0.0 with +Inf and -Inf in X: mul! forms every product (X[j] * α is NaN), so the result is NaN wherever the
    restatement's is; no product may be skipped."""
    f = E.fixtures()[name]
    rng = np.random.default_rng(5)
    with _Pair(asm, *f.A) as P:
        for adjoint, k, alpha, beta in itertools.product((False, True), (1, 3), (0.0, -0.0), (0.0, 1.0)):
            X = random_dense(rng, f.m if adjoint else f.n, k, specials=False)
            X[::5] = np.inf
            X[2::7] = -np.inf
            want = _check(P, rng, adjoint, k, alpha, beta, (name, "α = 0, Inf in X"), X=X)
            assert beta != 0 or np.isnan(want).any(), (name, adjoint, k, alpha)


@pytest.mark.parametrize("name", sorted(E.fixtures()))
def test_new_values(asm, name):
    """set_values (host) and set_values_dev (device) with new values: the operators equal a freshly created pair and the restatement."""
    import torch

    f = E.fixtures()[name]
    v2 = f.nzval[np.random.default_rng(7).permutation(len(f.nzval))] * -1.5
    A2 = (f.m, f.n, f.colptr, f.rowval, v2)
    with _Pair(asm, *f.A) as P, _Pair(asm, *A2) as F:
        P.host.set_values(v2)
        P.dev.set_values_dev(torch.from_numpy(v2).cuda())
        P.A = A2
        for adjoint, k in itertools.product((False, True), (1, 3, 9)):
            want = _check(P, np.random.default_rng(k), adjoint, k, 2.5, -0.5, (name, "set values"))
            fresh = _check(F, np.random.default_rng(k), adjoint, k, 2.5, -0.5, (name, "fresh"))
            assert np.array_equal(bits(want), bits(fresh))


def test_above_2_24_rows_and_columns():
    """m = n = 2^24 + 197 (spmv_edges.big_matrix): the plan's grid-stride loops go round twice, the last slice holds 5 rows, a long row
    and a column of more than 512 entries lie above 2^24.  A·x and Aᵀ·x for k = 1 and 3 through the host API; the operator is freed
    when the test ends."""
    import otmb_amd.api as api

    m, n, p, i, v = E.big_matrix()
    rng = np.random.default_rng(24)
    with api.DeviceOperator(_csc(m, n, p, i, v)) as D:
        for k in (1, 3):
            X = np.asfortranarray(rng.standard_normal((n, k)) * 10.0 ** rng.integers(-3, 4, (n, k)))
            for adjoint in (False, True):
                x = X[:, 0] if k == 1 else X
                alpha, beta = (1.0, 0.0) if k == 1 else (2.5, -0.5)
                Y = None if k == 1 else np.asfortranarray(rng.standard_normal((n, k)))
                want = spmv_ref(m, n, p, i, v, x, alpha, beta, Y, adjoint)
                got = D.mul(x, alpha=alpha, beta=beta, Y=None if Y is None else Y.copy(order="F"), adjoint=adjoint)
                _same(np.asarray(got), want, ("2^24 + 197", "Aᵀ" if adjoint else "A", k))
