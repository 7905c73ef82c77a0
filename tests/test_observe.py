"""GPU: otmb_op_observe[_dev] (csrc/otmb_observe.hip): obs = Wᵀ·X has THE BITS of tests/observe_ref.py's restatement of the order the header
states, at the sizes where that order can go wrong, across the register blocks' edges, on padded arrays through both load paths, through
the host route (api.DeviceOperator.observe: W and X staged compactly) and the device route (device.Operator.observe on torch tensors).

n:  1 a single row;  2 one full row pair;  511, 512, 513 a lane's second pair begins at row 512;  2047, 2048 one workgroup exactly full;
2049, 2050 a second workgroup of one lone row, then of one pair;  4097 three partials in the fold.
(q, k): (1, 1), (4, 4) one block; (5, 3), (3, 5), (7, 7) across both block edges (4 + 1, 2 + 1, 4 + 2 + 1).
Leading dimensions n, n + 1, n + 2 with NaN in all padding: 16-byte loads need an even one, so whichever of n, n + 1 is odd takes the 8-byte path."""
import ctypes as C

import numpy as np
import pytest

import observe_ref as OR
from test_step import _csc, _same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 511, 512, 513, 2047, 2048, 2049, 2050, 4097]
QK = [(1, 1), (4, 4), (5, 3), (3, 5), (7, 7)]
PADS = [(0, 0), (1, 1), (2, 2), (1, 2)]  # rows of padding under W and under X


def _identity(n):
    return _csc(n, np.arange(1, n + 2), np.arange(1, n + 1), np.ones(n))


@pytest.fixture(scope="module")
def operators():
    """Per n: (api.DeviceOperator, device.Operator) over the identity of that size (the observations read the operator's size alone)."""
    import torch

    import otmb_amd.api as api
    from otmb_amd import device

    ctx = device.DeviceAssembler(0).ctx
    dev = torch.device("cuda", 0)
    made = {}

    def get(n):
        if n not in made:
            A = _identity(n)
            made[n] = (api.DeviceOperator(A), device.Operator(ctx, n, n, *(torch.from_numpy(a).to(dev) for a in (A.colptr, A.rowval, A.nzval))))
        return made[n]

    yield get
    for D, O in made.values():
        D.close()
        O.close()


def _padded(a, pad):
    """a (n, m) as the first n rows of a Fortran-ordered (n + pad, m) array whose other rows are NaN."""
    p = np.full((a.shape[0] + pad, a.shape[1]), np.nan, order="F")
    p[:a.shape[0]] = a
    return p[:a.shape[0]]


def _on_device(view):
    """The padded host view as a device tensor of the same strides."""
    import torch

    n, m = view.shape
    if view.strides[0] != 8:
        view = np.asfortranarray(view)
    ld = view.strides[1] // 8 if m > 1 else n
    flat = np.full(ld * m, np.nan)
    flat.reshape(m, ld)[:, :n] = view.T
    return torch.from_numpy(flat).cuda().as_strided((n, m), (1, ld))


def _inputs(n, q, k):
    rng = np.random.default_rng(1000 * n + 10 * q + k)
    return rng.standard_normal((n, q)), rng.standard_normal((n, k)) * 10.0 ** rng.integers(-2, 3, (n, k))


@pytest.mark.parametrize("n", SIZES)
def test_observe_has_the_bits_of_the_restatement(operators, n):
    D, O = operators(n)
    for q, k in QK:
        W, X = _inputs(n, q, k)
        want = OR.observe_ref(W, X)
        assert want.shape == (q, k)
        for pw, px in PADS:
            Wp, Xp = _padded(W, pw), _padded(X, px)
            _same_bits(D.observe(Wp, Xp), want, ("host route", n, q, k, pw, px))
            _same_bits(O.observe(_on_device(Wp), _on_device(Xp)).cpu().numpy(), want, ("device route", n, q, k, pw, px))
    # entry (j, c) has the bits that observer and that tracer have alone; 1-D in, 1-D out
    W, X = _inputs(n, 7, 7)
    want = OR.observe_ref(W, X)
    for j, c in ((0, 0), (4, 2), (6, 6)):
        alone = D.observe(W[:, j], X[:, c])
        assert alone.shape == (1,)
        _same_bits(alone[0], want[j, c], ("alone", n, j, c))
    _same_bits(D.observe(W, X), D.observe(W, X), "the same call twice")


def test_signed_zeros_infinities_and_nans(operators):
    """All terms -0.0 give +0.0; an Inf in W[i0, j0] and a NaN in X[i1, c1] reach exactly row j0 and column c1 of obs."""
    n, q, k = 2050, 5, 3
    D, O = operators(n)
    obs = D.observe(np.full((n, q), -0.0), np.ones((n, k)))
    assert (obs == 0).all() and not np.signbit(obs).any()
    W, X = _inputs(n, q, k)
    j0, c1 = 3, 1
    W[2049, j0] = np.inf
    X[700, c1] = np.nan
    want = OR.observe_ref(W, X)
    for got in (D.observe(W, X), O.observe(_on_device(W), _on_device(X)).cpu().numpy()):
        assert OR.same_values(got, want)
        special = ~np.isfinite(got)
        expect = np.zeros((q, k), dtype=bool)
        expect[j0, :] = True
        expect[:, c1] = True
        assert np.array_equal(special, expect)
        assert np.isnan(got[:, c1]).all() and np.isinf(got[j0, [0, 2]]).all()


def test_a_noncontiguous_torch_view_gives_the_same_bits(operators):
    import torch

    n, q, k = 2049, 3, 5
    D, O = operators(n)
    W, X = _inputs(n, q, k)
    want = OR.observe_ref(W, X)
    big = torch.full((2 * n, 2 * k), float("nan"), dtype=torch.float64, device="cuda")  # row-major, every other row and column
    big[::2, ::2] = torch.from_numpy(X).cuda()
    Xv = big[::2, ::2]
    assert Xv.stride(0) != 1
    Wv = torch.from_numpy(np.ascontiguousarray(W)).cuda()  # row-major (n, q): stride(0) = q
    _same_bits(O.observe(Wv, Xv).cpu().numpy(), want, "views")
    _same_bits(O.observe(Wv[:, 1], Xv[:, 2]).cpu().numpy(), want[1:2, 2], "1-D views")


def test_refusals_write_nothing_and_leave_the_operator_usable(operators):
    from otmb_amd import capi

    n, q, k = 513, 2, 3
    D, O = operators(n)
    W, X = (np.asfortranarray(a) for a in _inputs(n, q, k))
    lib = capi.lib()
    cases = {"q < 0": (k, -1, W.ctypes.data, n, X.ctypes.data, n, True), "W null": (k, q, None, n, X.ctypes.data, n, True),
             "obs null": (k, q, W.ctypes.data, n, X.ctypes.data, n, False), "ldw < n": (k, q, W.ctypes.data, n - 1, X.ctypes.data, n, True),
             "ldx < n": (k, q, W.ctypes.data, n, X.ctypes.data, n - 1, True), "k < 1": (0, q, W.ctypes.data, n, X.ctypes.data, n, True),
             "X null": (k, q, W.ctypes.data, n, None, n, True)}
    for what, (kk, qq, wp, ldw, xp, ldx, has_obs) in cases.items():
        obs = np.full((q, k), 7.25, order="F")
        rc = lib.otmb_op_observe(D.handle, kk, qq, wp, ldw, xp, ldx, obs.ctypes.data if has_obs else None)
        assert rc == 11, (what, rc)
        with pytest.raises(capi.OtmbError, match="otmb_op_observe"):
            D.ctx.check(rc)
        assert (obs == 7.25).all(), what
    for shape in ((n + 1, q), (n, q, 1)):
        with pytest.raises(capi.OtmbError, match="DimensionMismatch"):
            D.observe(np.zeros(shape), X)
    # q == 0 is no error and touches nothing
    obs = np.full(3, 7.25)
    assert lib.otmb_op_observe(D.handle, k, 0, None, n, X.ctypes.data, n, obs.ctypes.data) == 0 and (obs == 7.25).all()
    _same_bits(D.observe(W, X), OR.observe_ref(W, X), "after the refusals")
    assert D.observe(np.zeros((n, 0)), X).shape == (0, k)
