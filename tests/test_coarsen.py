"""coarsen: C = LUMP * T * SPRAY on the GPU (csrc/otmb_coarsen.hip) against the restatement of SparseArrays' (LUMP * T) * SPRAY
(tests/spmatmul_ref.py): colptr, rowval and the BIT PATTERNS of nzval (so that +0.0 and -0.0 differ)."""
import numpy as np
import pytest

from helpers import make_case
from spmatmul_ref import coarse_ref
from test_lump_and_spray import _same as _same_lump
from test_oracle import LUMP_SETTINGS, lump_inputs, lump_mask

pytestmark = pytest.mark.gpu

OPS = ("T", "Tadv", "TκH", "TκVML", "TκVdeep")


def _bits(v):
    v = np.ascontiguousarray(v, dtype=np.float64)
    b = v.view(np.int64).copy()
    b[np.isnan(v)] = 0x7FF8000000000000  # a NaN is a NaN (its payload / sign is the hardware's: not part of the contract)
    return b


def _same(got, want, what):
    m, n, p, i, v = want
    assert got.shape == (m, n), (what, got.shape, (m, n))
    assert np.array_equal(got.colptr, p), (what, "colptr")
    assert np.array_equal(got.rowval, i), (what, "rowval")
    bad = np.flatnonzero(_bits(got.nzval) != _bits(v))
    assert bad.size == 0, (what, "nzval", bad[:5], np.asarray(got.nzval)[bad[:5]], v[bad[:5]])


def _csc(m, n, p, i, v):
    import otmb_amd.api as api

    return api.SparseMatrixCSC(m, n, np.asarray(p, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(v, dtype=np.float64))


@pytest.mark.parametrize("name", ["tiny_tripolar", "tiny_bipolar", "odd_nx_fold", "small_rho3d", "nx2"])
def test_coarsen_matches_spmatmul_bit_for_bit(oracle, name):
    import otmb_amd.api as api

    wet, vol, tm, N = lump_inputs(oracle, name)
    T = api.SparseMatrixCSC(N, N, *tm["T"])
    for q, (di, dj, dk, usemask) in enumerate(LUMP_SETTINGS + [(10, 10, 1, True), (3, 4, 2, True)]):
        mask = lump_mask(wet, q) if usemask else None
        L, S, _ = api.lump_and_spray(wet, vol, T, mask, di=di, dj=dj, dk=dk)
        for op in OPS:
            B = api.SparseMatrixCSC(N, N, *tm[op])
            _same(api.coarsen(L, B, S), coarse_ref(L, B, S), (name, di, dj, dk, usemask, op))


def test_coarsen_large_columns(oracle):
    """Columns above the LDS bound (the sorted path): a block at the 4096-cell limit, an S with every fine cell in one column,
    and S's with empty columns on both paths."""
    import otmb_amd.api as api

    wet, vol, tm, N = lump_inputs(oracle, "small_rho3d")
    T = api.SparseMatrixCSC(N, N, *tm["T"])
    for (di, dj, dk) in ((64, 64, 1), (16, 16, 16)):
        L, S, vc = api.lump_and_spray(wet, vol, T, None, di=di, dj=dj, dk=dk)
        _same_lump((L, S, vc), oracle.lump_and_spray(wet, vol, tm["T"], None, di, dj, dk), ("lump", di, dj, dk))  # a verified input
        for op in ("T", "TκH"):
            B = api.SparseMatrixCSC(N, N, *tm[op])
            _same(api.coarsen(L, B, S), coarse_ref(L, B, S), (di, dj, dk, op))
    L, S, vc = api.lump_and_spray(wet, vol, T)
    Nc = len(vc)
    one = _csc(N, 1, [1, N + 1], np.arange(1, N + 1), np.ones(N))
    _same(api.coarsen(L, T, one), coarse_ref(L, T, one), "one column")
    everything = _csc(1, N, np.arange(1, N + 2), np.ones(N, dtype=np.int64), vol / vol.sum())
    _same(api.coarsen(everything, T, one), coarse_ref(everything, T, one), "one row, one column")
    # empty columns: around every column of SPRAY (small path) and between two halves of the fine cells (sorted path)
    p = np.asarray(S.colptr)
    sp_empty = _csc(N, 2 * Nc, np.repeat(p, 2)[1:], S.rowval, S.nzval)
    _same(api.coarsen(L, T, sp_empty), coarse_ref(L, T, sp_empty), "empty columns, small path")
    h = N // 2
    halves = _csc(N, 4, [1, 1, h + 1, h + 1, N + 1], np.arange(1, N + 1), np.ones(N))
    _same(api.coarsen(L, T, halves), coarse_ref(L, T, halves), "empty columns, sorted path")
    empty = _csc(N, 3, [1, 1, 1, 1], [], [])
    got = api.coarsen(L, T, empty)
    assert got.nnz == 0 and list(got.colptr) == [1, 1, 1, 1]


def test_coarsen_stored_zeros_signed_zeros_cancellation_nan_inf():
    import otmb_amd.api as api

    # LUMP: fine cells 1, 2 -> coarse 1; 3, 4 -> coarse 2; cell 5 in no coarse cell (an empty column)
    L = _csc(2, 5, [1, 2, 3, 4, 5, 5], [1, 1, 2, 2], [0.5, 0.5, 0.25, 0.75])
    # T columns: stored zeros | a lone -0.0 | exact cancellation | NaN and Inf | a cell lumped nowhere
    T = _csc(5, 5, [1, 3, 4, 6, 8, 9],
             [1, 2, 3, 1, 2, 1, 3, 5],
             [0.0, 0.0, -0.0, 3.0, -3.0, np.nan, np.inf, 7.0])
    for S in (_csc(5, 5, np.arange(1, 7), np.arange(1, 6), np.ones(5)),       # the identity: every column on its own
              _csc(5, 2, [1, 3, 6], [1, 2, 3, 4, 5], np.ones(5)),               # two coarse columns
              _csc(5, 1, [1, 6], np.arange(1, 6), [1.0, -1.0, 2.0, 0.5, 1.0])):  # all in one, with weights
        want = coarse_ref(L, T, S)
        got = api.coarsen(L, T, S)
        _same(got, want, S.shape)
    got = api.coarsen(L, T, _csc(5, 5, np.arange(1, 7), np.arange(1, 6), np.ones(5)))
    v = np.asarray(got.nzval)
    assert got.nnz == 5  # column 5 touches nothing: LUMP's column 5 is empty
    assert v[0] == 0.0 and not np.signbit(v[0])       # stored zeros are stored
    assert v[1] == 0.0 and np.signbit(v[1])            # -0.0 * 0.25 stays -0.0 (first touch copies)
    assert v[2] == 0.0 and not np.signbit(v[2])        # 3 * 0.5 + -3 * 0.5: an exact zero, stored
    assert np.isnan(v[3]) and v[4] == np.inf              # NaN and Inf propagate


def test_coarsen_errors_are_invalid_arg():
    import otmb_amd.api as api
    from otmb_amd.capi import OtmbError

    L = _csc(2, 3, [1, 2, 3, 4], [1, 2, 2], [1.0, 1.0, 1.0])
    T = _csc(3, 3, [1, 2, 3, 4], [1, 2, 3], [1.0, 2.0, 3.0])
    S = _csc(3, 2, [1, 2, 4], [1, 2, 3], [1.0, 1.0, 1.0])
    _same(api.coarsen(L, T, S), coarse_ref(L, T, S), "valid")
    two = _csc(2, 3, [1, 3, 4, 5], [1, 2, 2, 1], [1.0, 1.0, 1.0, 1.0])
    with pytest.raises(OtmbError, match="two or more") as e:
        api.coarsen(two, T, S)
    assert e.value.name == "INVALID_ARG"
    with pytest.raises(OtmbError, match="DimensionMismatch") as e:
        api.coarsen(L, _csc(4, 4, [1, 1, 1, 1, 1], [], []), S)
    assert e.value.name == "INVALID_ARG"
    with pytest.raises(OtmbError) as e:
        api.coarsen(L, T, _csc(4, 2, [1, 2, 3], [1, 2], [1.0, 1.0]))
    assert e.value.name == "INVALID_ARG"
    # one rowval past the end, in each matrix: refused by the check that runs before anything is read through it
    for what, args in (("LUMP", (_csc(2, 3, [1, 2, 3, 4], [1, 3, 2], [1.0, 1.0, 1.0]), T, S)),
                       ("T", (L, _csc(3, 3, [1, 2, 3, 4], [1, 4, 3], [1.0, 2.0, 3.0]), S)),
                       ("SPRAY", (L, T, _csc(3, 2, [1, 2, 4], [1, 2, 4], [1.0, 1.0, 1.0])))):
        with pytest.raises(OtmbError, match=what) as e:
            api.coarsen(*args)
        assert e.value.name == "INVALID_ARG"
    _same(api.coarsen(L, T, S), coarse_ref(L, T, S), "valid after the errors")


def test_device_coarsen_on_resident_result(oracle):
    import torch

    import otmb_amd.api as api
    from otmb_amd.device import DeviceAssembler

    g, gm = make_case("small_rho3d")
    wet, vol, tm, N = lump_inputs(oracle, "small_rho3d")
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    asm.step(umo, vmo, g.umo.properties["_FillValue"])
    host = asm.result_to_host()
    mask = lump_mask(wet, 5)
    dm = torch.from_numpy(np.asfortranarray(mask).ravel(order="F").astype(np.uint8)).cuda()
    for m, (di, dj, dk) in ((None, (2, 2, 1)), (dm, (4, 3, 2))):
        L, S, vc = asm.lump_and_spray(m, di, dj, dk)
        Nc = len(vc)
        Lh = _csc(Nc, N, *(t.cpu().numpy() for t in L))
        Sh = _csc(N, Nc, *(t.cpu().numpy() for t in S))
        for op in ("T", "TκVML"):
            Cp, Ci, Cx = asm.coarsen(L, S, op)
            got = api.SparseMatrixCSC(Nc, Nc, Cp.cpu().numpy(), Ci.cpu().numpy(), Cx.cpu().numpy())
            B = api.SparseMatrixCSC(N, N, *host[op])
            want = api.coarsen(Lh, B, Sh)
            _same(got, (want.m, want.n, want.colptr, want.rowval, want.nzval), (di, dj, dk, op))
            _same(got, coarse_ref(Lh, B, Sh), (di, dj, dk, op, "ref"))


def test_coarsen_access1deg_bit_identical(oracle):
    """Full size: the 1 degree preset, 2 x 2 x 1 blocks without a mask and with the reference's SO / NA mask (test/online.jl:126-128)."""
    import torch

    import otmb_amd
    import otmb_amd.api as api
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
    host = asm.result_to_host()
    N = asm.N
    nx, ny, nz = asm.nx, asm.ny, asm.nz
    wet = (asm.wet3d.cpu().numpy() != 0).reshape((nx, ny, nz), order="F")
    vol = np.asarray(gm.v3D).reshape(-1, order="F")[wet.reshape(-1, order="F")]
    lat, lon = np.asarray(g.lat), np.asarray(g.lon) % 360
    so, na = lat < -35, (lat > 50) & ((lon < 100) | (250 < lon))
    somask = np.repeat((~so & ~na)[:, :, None], nz, axis=2)
    T = api.SparseMatrixCSC(N, N, *host["T"])
    for mask in (None, somask):
        L, S, vc = api.lump_and_spray(wet, vol, T, mask, di=2, dj=2, dk=1)
        lump_want = oracle.lump_and_spray(wet, vol, host["T"], mask, 2, 2, 1)
        _same_lump((L, S, vc), lump_want, ("1deg", mask is not None, "host lump"))
        want = coarse_ref(L, T, S)
        _same(api.coarsen(L, T, S), want, ("1deg", mask is not None, "host"))
        dm = None if mask is None else torch.from_numpy(np.asfortranarray(mask).ravel(order="F").astype(np.uint8)).cuda()
        Ld, Sd, vcd = asm.lump_and_spray(dm, 2, 2, 1)
        _same_lump((_csc(len(vcd), N, *(t.cpu().numpy() for t in Ld)), _csc(N, len(vcd), *(t.cpu().numpy() for t in Sd)), vcd.cpu().numpy()),
                   lump_want, ("1deg", mask is not None, "device lump"))
        Cp, Ci, Cx = asm.coarsen(Ld, Sd)
        got = api.SparseMatrixCSC(len(vc), len(vc), Cp.cpu().numpy(), Ci.cpu().numpy(), Cx.cpu().numpy())
        _same(got, want, ("1deg", mask is not None, "device"))
