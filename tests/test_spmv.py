"""The resident sparse operator (csrc/otmb_spmv.hip, otmb_op_*) against tests/spmv_ref.py, the restatement of SparseArrays' 5-argument
mul! (Julia 1.10): every result compared by bit pattern (any NaN equals any NaN), A·X and Aᵀ·X, through the host API (api.DeviceOperator)
and the device-resident one (DeviceAssembler.operator / mul)."""
import itertools

import numpy as np
import pytest

from spmv_ref import bits, random_csc, random_dense, spmv_ref
from test_oracle import lump_inputs

pytestmark = pytest.mark.gpu

OPS = ("T", "Tadv", "TκH", "TκVML", "TκVdeep")
ALPHAS = (1.0, 0.0, 2.5)
BETAS = (0.0, 1.0, -0.5)


def _csc(m, n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(m, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


def _padded(rng, rows, k, pad=3):
    """A (rows, k) column-major view with leading dimension rows + pad, and the whole array (to check that padding stays)."""
    big = random_dense(rng, rows + pad, k)
    return big[:rows], big


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).ravel() != bits(want).ravel())
    assert bad.size == 0, (what, bad[:5], got.ravel()[bad[:5]], want.ravel()[bad[:5]])


def _check_all(A, rng, what, ks=(1, 3, 8), alphas=ALPHAS, betas=BETAS):
    import otmb_amd.api as api

    with api.DeviceOperator(A) as D:
        for adjoint, k, alpha, beta in itertools.product((False, True), ks, alphas, betas):
            rx, ry = (A.m, A.n) if adjoint else (A.n, A.m)
            X, _ = _padded(rng, rx, k)
            Y, Ybig = _padded(rng, ry, k)
            if k == 1:
                X, Y = X[:, 0], Y[:, 0]
            want = spmv_ref(A.m, A.n, A.colptr, A.rowval, A.nzval, X, alpha, beta, Y, adjoint)
            before = Ybig[ry:].copy()
            got = D.mul(X, alpha=alpha, beta=beta, Y=Y, adjoint=adjoint)
            _same(np.asarray(got), want, (what, adjoint, k, alpha, beta))
            assert np.array_equal(bits(Ybig[ry:]), bits(before)), (what, "padding rows of Y were written")


@pytest.mark.parametrize("name", ["tiny_tripolar", "tiny_bipolar", "odd_nx_fold", "small_rho3d", "nx2"])
def test_goldens_all_operators(oracle, name):
    wet, vol, tm, N = lump_inputs(oracle, name)
    rng = np.random.default_rng(len(name))
    for op in OPS:
        _check_all(_csc(N, N, *tm[op]), rng, (name, op))


def test_lump_spray_and_coarse_operator(oracle):
    """LUMP (rows of up to 4096 entries with a 64 x 64 x 1 block: the long-row path), SPRAY and a coarsen result."""
    import otmb_amd.api as api

    wet, vol, tm, N = lump_inputs(oracle, "small_rho3d")
    T = _csc(N, N, *tm["T"])
    rng = np.random.default_rng(5)
    for di, dj, dk in ((2, 2, 1), (64, 64, 1)):
        L, S, vc = api.lump_and_spray(wet, vol, T, None, di=di, dj=dj, dk=dk)
        Nc = len(vc)
        L = _csc(Nc, N, L.colptr, L.rowval, L.nzval)
        S = _csc(N, Nc, S.colptr, S.rowval, S.nzval)
        Tc = api.coarsen(L, T, S)
        for what, A in (("LUMP", L), ("SPRAY", S), ("coarse", Tc)):
            _check_all(A, rng, (di, dj, dk, what), ks=(1, 3), alphas=(1.0, 2.5), betas=(0.0, -0.5))
    assert np.bincount(np.asarray(L.rowval)).max() > 256  # (the 64 x 64 block really made rows for the long-row path, SP_ELL_MAX)


def test_random_noncanonical_rectangular_and_special_values():
    rng = np.random.default_rng(11)
    for q, (m, n) in enumerate(((7, 5), (5, 7), (130, 70), (64, 64), (200, 1), (1, 200))):
        p, i, v = random_csc(rng, m, n, density=0.2 if m * n > 1000 else 0.4)
        _check_all(_csc(m, n, p, i, v), rng, ("random", m, n))


def test_long_row_and_mixed_slices():
    """A row of 5000 entries (longer than 4096), and a slice where one row is far longer than its neighbours."""
    rng = np.random.default_rng(2)
    n = 5000
    A = _csc(3, n, np.arange(1, n + 2), np.ones(n, dtype=np.int64), rng.standard_normal(n))
    _check_all(A, rng, "one long row", ks=(1, 8), alphas=(2.5,), betas=(0.0, -0.5))
    # 130 rows: row 7 in every column, the others one entry each (a long row among short ones), plus duplicates of row 7
    m, n = 130, 400
    rv = np.concatenate([[7, (c % m) + 1] + ([7] if c % 3 == 0 else []) for c in range(n)])
    cnt = np.array([3 if c % 3 == 0 else 2 for c in range(n)])
    p = np.concatenate([[1], 1 + np.cumsum(cnt)])
    A = _csc(m, n, p, rv, rng.standard_normal(len(rv)))
    _check_all(A, rng, "mixed", ks=(1, 3), alphas=(1.0,), betas=(0.0, 1.0))


def test_long_rows_with_more_than_64_tracers():
    """spmv_long_kernel takes tracers in groups of 64 lanes: k = 70 needs two groups (and the row kernels nine register blocks)."""
    rng = np.random.default_rng(12)
    n = 600
    A = _csc(3, n, np.arange(1, n + 2), np.ones(n, dtype=np.int64), rng.standard_normal(n))  # row 1: 600 entries (> 256: long)
    _check_all(A, rng, "k = 70, one long row", ks=(70,), alphas=(1.0, 2.5), betas=(0.0, -0.5))
    m, n = 130, 400
    rv = np.concatenate([[7, (c % m) + 1] for c in range(n)])  # row 7: 400 + entries, the others 3-4
    A = _csc(m, n, np.arange(1, 2 * n + 2, 2), rv, rng.standard_normal(len(rv)))
    _check_all(A, rng, "k = 70, long row among short ones", ks=(65, 70), alphas=(2.5,), betas=(1.0,))


def test_row_far_longer_than_its_slice():
    """A row of about 100 entries among rows of 2-3 (at most SP_ELL_MAX = 256, but longer than 32 and four times its slice's mean: the
    relative rule sends it to the long-row path), in slice 0; slice 1 and the partial slice 2 have none."""
    rng = np.random.default_rng(13)
    m, n = 130, 300
    cols = [[(c % m) + 1] + ([7] if c < 100 else []) for c in range(n)]
    rv = np.concatenate(cols)
    p = np.concatenate([[1], 1 + np.cumsum([len(c) for c in cols])])
    lens = np.bincount(rv, minlength=m + 1)[1:]
    mean0 = -(-lens[:64].sum() // 64)
    assert 32 < lens[6] <= 256 and lens[6] > 4 * mean0 and np.delete(lens, 6).max() <= 3, (lens[6], mean0)
    A = _csc(m, n, p, rv, rng.standard_normal(len(rv)))
    _check_all(A, rng, "row of ~100 in a slice of 2-3", ks=(1, 3, 8, 70), alphas=(1.0, 2.5), betas=(0.0, -0.5))


def test_host_tensors_are_refused():
    """The device operator takes device tensors only: a host tensor's pointer is refused in Python before any kernel sees it."""
    import torch

    from otmb_amd.device import DeviceAssembler, Operator

    asm = DeviceAssembler(0)
    p, i, v = (torch.tensor([1, 2, 3]), torch.tensor([1, 2]), torch.tensor([1.0, 2.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="cuda:0"):
        Operator(asm.ctx, 2, 2, p, i, v)
    op = Operator(asm.ctx, 2, 2, p.cuda(), i.cuda(), v.cuda())
    x = torch.tensor([3.0, 4.0], dtype=torch.float64)
    with pytest.raises(ValueError, match="X must be a tensor on cuda:0"):
        op.mul(x)
    with pytest.raises(ValueError, match="Y must be a tensor on cuda:0"):
        op.mul(x.cuda(), Y=torch.zeros(2, dtype=torch.float64), beta=1.0)
    with pytest.raises(ValueError, match="nzval must be a tensor on cuda:0"):
        op.set_values_dev(v)
    assert op.mul(x.cuda()).cpu().tolist() == [3.0, 8.0]  # (still usable)
    op.close()


def test_empty_matrices():
    rng = np.random.default_rng(1)
    for m, n in ((4, 3), (3, 0), (0, 3), (0, 0)):
        _check_all(_csc(m, n, np.ones(n + 1, dtype=np.int64), [], []), rng, ("empty", m, n), ks=(1, 3), alphas=(1.0, np.inf),
                   betas=(0.0, 1.0, -0.5))


def test_errors_leave_the_operator_usable_and_set_values():
    import otmb_amd.api as api
    from otmb_amd import capi
    from otmb_amd.capi import OtmbError

    rng = np.random.default_rng(4)
    p, i, v = random_csc(rng, 6, 5, specials=False)
    A = _csc(6, 5, p, i, v)
    x = rng.standard_normal(5)
    want = spmv_ref(6, 5, p, i, v, x)
    # invalid matrices: refused before anything is read through them
    for what, bad in (("colptr[1]", _csc(2, 3, [2, 2, 2, 2], [], [])), ("decreasing", _csc(2, 3, [1, 3, 2, 4], [1, 2, 1], [1.0, 1.0, 1.0])),
                      ("row 0", _csc(2, 3, [1, 2, 3, 4], [0, 1, 1], [1.0, 1.0, 1.0])),
                      ("row m + 1", _csc(2, 3, [1, 2, 3, 4], [1, 3, 1], [1.0, 1.0, 1.0]))):
        with pytest.raises(OtmbError) as e:
            api.DeviceOperator(bad)
        assert e.value.name == "INVALID_ARG", what
    D = api.DeviceOperator(A)
    lib, h = capi.lib(), D.handle
    X = np.asfortranarray(rng.standard_normal((5, 2)))
    Y = np.zeros((6, 2), order="F")
    for what, args in (("k = 0", (h, 0, 0, X.ctypes.data, 5, Y.ctypes.data, 6, 1.0, 0.0)),
                       ("ldx", (h, 0, 1, X.ctypes.data, 4, Y.ctypes.data, 6, 1.0, 0.0)),
                       ("ldy", (h, 0, 1, X.ctypes.data, 5, Y.ctypes.data, 5, 1.0, 0.0)),
                       ("ldx adjoint", (h, 1, 1, X.ctypes.data, 5, Y.ctypes.data, 6, 1.0, 0.0)),
                       ("null X", (h, 0, 1, None, 5, Y.ctypes.data, 6, 1.0, 0.0)),
                       ("null Y", (h, 0, 1, X.ctypes.data, 5, None, 6, 1.0, 0.0))):
        assert lib.otmb_op_mul(*args) == 11, what
        assert lib.otmb_last_error(D.ctx.handle).decode().startswith("invalid argument"), what
        _same(D.mul(x), want, ("after", what))
    assert lib.otmb_op_mul(None, 0, 1, X.ctypes.data, 5, Y.ctypes.data, 6, 1.0, 0.0) == 11
    assert lib.otmb_op_set_values(h, v.ctypes.data, len(v) + 1) == 11
    assert lib.otmb_op_set_values(h, None, len(v)) == 11 or len(v) == 0
    with pytest.raises(OtmbError) as e:
        D.mul(rng.standard_normal(6))  # dimension mismatch
    assert e.value.name == "INVALID_ARG"
    with pytest.raises(OtmbError) as e:
        D.set_values(v[:-1])
    assert e.value.name == "INVALID_ARG"
    _same(D.mul(x), want, "after the errors")
    # new values equal a freshly created operator, in both directions
    v2 = rng.standard_normal(len(v))
    D.set_values(v2)
    with api.DeviceOperator(_csc(6, 5, p, i, v2)) as F:
        for adjoint in (False, True):
            z = rng.standard_normal(6 if adjoint else 5)
            _same(D.mul(z, adjoint=adjoint), F.mul(z, adjoint=adjoint), ("set_values", adjoint))
            _same(D.mul(z, adjoint=adjoint), spmv_ref(6, 5, p, i, v2, z, adjoint=adjoint), ("set_values ref", adjoint))
    # the operator owns its copies: the caller's arrays may change
    keep = v2.copy()
    v2[:] = np.nan
    _same(D @ x, spmv_ref(6, 5, p, i, keep, x), "own copy")
    D.close()


def test_device_loop_with_cancellations():
    """DeviceAssembler over slices with exact cancellations (κH = 0, centred weights): after each slice asm.mul("T", x) and the adjoint
    equal the restatement on that slice's downloaded T; both a pattern-kept (set values) and a re-planned slice occur."""
    import torch

    from helpers import make_case
    from test_kept_ops import _host, _pair
    from test_kept_t_pattern import _cancel_fields

    g0, _ = make_case("small_rho3d")
    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d", kappa=(0.0, g0.kappaVML, g0.kappaVdeep), upwind=False)
    del full
    cancel = {2, 5, 6}
    fields = _cancel_fields(umo, vmo, 9, cancel, seed=42)
    rng = np.random.default_rng(8)
    N = asm.N
    replans, reuses = [], []
    for k, (u, v) in enumerate(fields):
        if k in (5, 6):
            asm.step_async(u, v, fill)  # (5 and 6 pipelined: folded by operator())
            if k == 5:
                continue
        else:
            asm.step(u, v, fill)
        r0, s0 = getattr(asm, "op_replans", 0), getattr(asm, "op_reuses", 0)
        x = rng.standard_normal(N)
        X3 = np.asfortranarray(rng.standard_normal((N, 3)))
        y = asm.mul("T", torch.from_numpy(x).cuda()).cpu().numpy()
        yt = asm.mul("T", torch.from_numpy(x).cuda(), adjoint=True).cpu().numpy()
        Y3 = asm.mul("T", torch.from_numpy(X3).cuda().t().contiguous().t(), alpha=2.5).cpu().numpy()
        replans.append(getattr(asm, "op_replans", 0) - r0)
        reuses.append(getattr(asm, "op_reuses", 0) - s0)
        h = _host(asm)["T"]
        _same(y, spmv_ref(N, N, *h, x), ("T x", k))
        _same(yt, spmv_ref(N, N, *h, x, adjoint=True), ("T' x", k))
        _same(Y3, spmv_ref(N, N, *h, X3, alpha=2.5), ("T X3", k))
        for op in ("TκH", "Tadv"):
            _same(asm.mul(op, torch.from_numpy(x).cuda()).cpu().numpy(), spmv_ref(N, N, *_host(asm)[op], x), (op, k))
    assert any(r > 0 for r in replans[1:]) and any(s > 0 and r == 0 for r, s in zip(replans, reuses)), (replans, reuses)
    # The library declines the kept operators while the assembler promises them (forget_given bumps the epoch its records are keyed to):
    # T is written in full and otmb_ctx_kept_t_pattern still holds the previous fill's 1.  The per-fill count does not move: T re-plans.
    asm.step(*fields[8], fill)
    asm.mul("T", torch.from_numpy(x).cuda())
    f0, r0 = asm.ctx.kept_t_pattern_fills(), getattr(asm, "op_replans", 0)
    asm.ctx.forget_given()
    asm.step(*fields[7], fill)
    took = asm.ctx.kept_t_pattern_fills() == f0 + 1
    y = asm.mul("T", torch.from_numpy(x).cuda()).cpu().numpy()
    assert took or getattr(asm, "op_replans", 0) == r0 + 1, (took, asm.ctx.kept_t_pattern())
    _same(y, spmv_ref(N, N, *_host(asm)["T"], x), "after forget_given")


def test_access1deg_divergence_and_volume_checks():
    """The 1 degree preset: T·x, Tᵀ·v (v the wet-cell volumes) and k = 8 random tracers bit for bit; τdiv = ‖e1‖ / ‖T e1‖ and
    τvol = ‖v‖ / ‖Tᵀ v‖ (test/local_full.jl:96-107) from the device vectors equal those from the restatement's."""
    import torch

    import otmb_amd
    from otmb_amd import synthetic
    from otmb_amd.device import DeviceAssembler

    g = synthetic.preset("access1deg", rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, 1e20)
    h = asm.result_to_host()["T"]
    N = asm.N
    wet = asm.wet3d.cpu().numpy() != 0
    vol = np.asarray(gm.v3D).reshape(-1, order="F")[wet]
    e1 = np.ones(N)
    Te1 = asm.mul("T", torch.from_numpy(e1).cuda()).cpu().numpy()
    Tv = asm.mul("T", torch.from_numpy(vol).cuda(), adjoint=True).cpu().numpy()
    want_e1, want_v = spmv_ref(N, N, *h, e1), spmv_ref(N, N, *h, vol, adjoint=True)
    _same(Te1, want_e1, "T e1")
    _same(Tv, want_v, "T' v")
    assert np.linalg.norm(e1) / np.linalg.norm(Te1) == np.linalg.norm(e1) / np.linalg.norm(want_e1)
    assert np.linalg.norm(vol) / np.linalg.norm(Tv) == np.linalg.norm(vol) / np.linalg.norm(want_v)
    X8 = np.asfortranarray(np.random.default_rng(1).standard_normal((N, 8)))
    Y8 = asm.mul("T", torch.from_numpy(X8).cuda().t().contiguous().t()).cpu().numpy()
    _same(Y8, spmv_ref(N, N, *h, X8), "T X8")
    Y8t = asm.mul("T", torch.from_numpy(X8).cuda().t().contiguous().t(), adjoint=True).cpu().numpy()
    _same(Y8t, spmv_ref(N, N, *h, X8, adjoint=True), "T' X8")
