"""GPU: buildTsink (csrc/otmb_sink.hip) through api.buildTsink (otmb_build_sink, host pointers) and DeviceAssembler.sinking
(otmb_build_sink_dev on the resident grid) against the numpy restatement tests/sink_ref.py, bit for bit: colptr, rowval and nzval.

Grids: nx2 (columns three levels deep: the smallest with a pair below a pair), tiny_tripolar, tiny_bipolar, odd_nx_fold with randomised
metrics, a one-level grid (no off-diagonal at all: nnz = N), the 3 x 2 x 5 gap mask (a dry cell inside a column) and mid_grids' "wide"
(1040 x 512 x 4, ~1.2 M wet cells: the only one whose column-start scan spans more than one block of the scan).  w as a scalar, as nz
values and as an (nx, ny, nz) array with NaN on the dry cells, under both seafloors.  Every refusal leaves the output arrays as they were."""
import ctypes as C

import numpy as np
import pytest

import sink_ref as K
from helpers import make_case

pytestmark = pytest.mark.gpu

W = 1.0e-3
SENTINEL = 7.25
HDIRS = ("west", "east", "south", "north")
CASE_GRIDS = ("nx2", "tiny_tripolar", "tiny_bipolar", "odd_nx_fold")
HAND_GRIDS = {"one_level": K.one_level_grid, "gap": K.gap_grid}

_GRIDS, _ASMS = {}, {}


def _grid(name):
    """(v3D, area2D, what DeviceAssembler.set_grid takes) of a grid, made once."""
    if name not in _GRIDS:
        if name in HAND_GRIDS:
            v3D, area = HAND_GRIDS[name]()
            nx, ny, nz = v3D.shape
            one = np.ones((nx, ny), order="F")
            gm = dict(v3D=v3D, thkcello=np.asfortranarray(np.where(np.isnan(v3D), np.nan, 10.0)), edge_length_2D={d: one for d in HDIRS},
                      distance_to_neighbour_2D={d: one for d in HDIRS}, area2D=area, zt=5.0 + 10.0 * np.arange(nz), gridtopology=0)
            mlotst, rho = np.asfortranarray(np.where(np.isnan(v3D[:, :, 0]), np.nan, 50.0)), 1035.0
        elif name == "wide":
            import mid_grids

            g, gm = mid_grids.case("wide")
            mlotst, rho = g.mlotst, g.rho
        else:
            g, gm = make_case(name)
            mlotst, rho = g.mlotst, g.rho
        _GRIDS[name] = (np.asarray(gm["v3D"]), np.asarray(gm["area2D"]), (gm, mlotst, rho))
    return _GRIDS[name]


def _asm(name):
    if name not in _ASMS:
        from otmb_amd.device import DeviceAssembler

        a = DeviceAssembler(0)
        a.set_grid(*_grid(name)[2])
        _ASMS[name] = a
    return _ASMS[name]


def _speeds(v3D, form, seed=2):
    nz = v3D.shape[2]
    if form == "scalar":
        return W
    if form == "vector":
        return W * np.linspace(0.5, 3.0, nz)
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.where(np.isnan(v3D), np.nan, rng.uniform(0.2, 2.0, v3D.shape) * W))  # garbage (NaN) on the dry cells


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, ref, what):
    assert np.array_equal(np.asarray(got[0]), ref[0]), (what, "colptr")
    assert np.array_equal(np.asarray(got[1]), ref[1]), (what, "rowval")
    assert np.array_equal(_bits(got[2]), _bits(ref[2])), (what, "nzval")


def _host(triple):
    return tuple(t.cpu().numpy() for t in triple)


@pytest.mark.parametrize("seafloor", K.SEAFLOORS)
@pytest.mark.parametrize("form", ["scalar", "vector", "array"])
@pytest.mark.parametrize("name", CASE_GRIDS + tuple(HAND_GRIDS))
def test_both_entry_points_have_the_bits_of_the_restatement(name, form, seafloor):
    import torch

    import otmb_amd.api as api

    v3D, area, _ = _grid(name)
    w = _speeds(v3D, form)
    ref = K.sink_ref(w, v3D, area, seafloor)
    idx = api.makeindices(v3D)
    S = api.buildTsink(w=w, gridmetrics=dict(v3D=v3D, area2D=area), indices=idx, seafloor=seafloor)
    assert S.shape == (idx.N, idx.N) and S.nnz == len(ref[1])
    _same((S.colptr, S.rowval, S.nzval), ref, (name, form, seafloor, "api.buildTsink"))
    asm = _asm(name)
    _same(_host(asm.sinking(w, seafloor)), ref, (name, form, seafloor, "DeviceAssembler.sinking"))
    if form != "scalar":  # a tensor on the device is read where it lies
        wt = torch.from_numpy(np.ascontiguousarray(np.asarray(w).ravel(order="F"))).cuda()
        _same(_host(asm.sinking(wt, seafloor)), ref, (name, form, seafloor, "a device tensor"))
    if form == "array":
        wt = torch.from_numpy(np.ascontiguousarray(w)).cuda()  # (nx, ny, nz), row-major: taken in the grid's order
        _same(_host(asm.sinking(wt, seafloor)), ref, (name, form, seafloor, "a 3-D device tensor"))
    if name == "one_level":
        assert S.nnz == idx.N and np.array_equal(S.colptr, np.arange(1, idx.N + 2))


def test_the_three_forms_agree_in_bits_where_they_agree():
    asm = _asm("tiny_tripolar")
    v3D = _grid("tiny_tripolar")[0]
    prof = _speeds(v3D, "vector")
    for seafloor in K.SEAFLOORS:
        a = _host(asm.sinking(prof, seafloor))
        b = _host(asm.sinking(np.asfortranarray(np.where(np.isnan(v3D), np.nan, np.broadcast_to(prof, v3D.shape))), seafloor))
        _same(a, b, "vector and array")
        _same(_host(asm.sinking(W, seafloor)), _host(asm.sinking(np.full(v3D.shape[2], W), seafloor)), "scalar and vector")


@pytest.mark.parametrize("seafloor", K.SEAFLOORS)
def test_the_wide_grid_spans_more_than_one_block_of_the_scan(seafloor):
    import otmb_amd.api as api

    v3D, area, _ = _grid("wide")
    w = _speeds(v3D, "array")
    ref = K.sink_ref(w, v3D, area, seafloor)
    assert len(ref[0]) - 1 > 1_000_000
    _same(_host(_asm("wide").sinking(w, seafloor)), ref, ("wide", seafloor, "DeviceAssembler.sinking"))
    if seafloor == "open":
        asm = _asm("wide")
        idx = dict(Lwet3D=asm.lwet3d.cpu().numpy().reshape(v3D.shape, order="F"), Lwet=asm.lwet[: asm.N].cpu().numpy(), N=asm.N)
        S = api.buildTsink(w=W, gridmetrics=dict(v3D=v3D, area2D=area), indices=idx)
        _same((S.colptr, S.rowval, S.nzval), K.sink_ref(W, v3D, area), ("wide", "api.buildTsink"))


def _raw_call(dev, v3D, area, idx, w_form, w_scalar, w, cap=None, closed=0):
    """otmb_build_sink[_dev] on sentinel-filled outputs: (rc, nnz, the outputs still hold their sentinels)."""
    import torch

    import otmb_amd.api as api
    from otmb_amd import capi

    ctx = api.context(0)
    N = int(idx["N"])
    nx, ny, nz = v3D.shape
    cap = 2 * N if cap is None else cap
    host = [np.asfortranarray(v3D).ravel(order="F"), np.asfortranarray(area).ravel(order="F"),
            np.asfortranarray(idx["Lwet3D"], dtype=np.int64).ravel(order="F"), np.ascontiguousarray(idx["Lwet"], dtype=np.int64),
            np.zeros(1) if w is None else np.asfortranarray(w, dtype=np.float64).ravel(order="F")]
    outs = [np.full(N + 1, -77, dtype=np.int64), np.full(max(cap, 1), -77, dtype=np.int64), np.full(max(cap, 1), SENTINEL)]
    nnz = C.c_int64(-5)
    if dev:
        dh = [torch.from_numpy(a).cuda() for a in host]
        do = [torch.from_numpy(a).cuda() for a in outs]
        rc = capi.lib().otmb_build_sink_dev(ctx.handle, w_form, float(w_scalar), None if w is None else dh[4].data_ptr(), dh[0].data_ptr(), dh[1].data_ptr(),
                                            dh[2].data_ptr(), dh[3].data_ptr(), N, nx, ny, nz, closed, do[0].data_ptr(), do[1].data_ptr(), do[2].data_ptr(), cap,
                                            C.byref(nnz))
        ctx.synchronize()
        torch.cuda.synchronize()
        outs = [t.cpu().numpy() for t in do]
    else:
        rc = capi.lib().otmb_build_sink(ctx.handle, w_form, float(w_scalar), None if w is None else host[4].ctypes.data, host[0].ctypes.data,
                                        host[1].ctypes.data, host[2].ctypes.data, host[3].ctypes.data, N, nx, ny, nz, closed, outs[0].ctypes.data,
                                        outs[1].ctypes.data, outs[2].ctypes.data, cap, C.byref(nnz))
    untouched = (outs[0] == -77).all() and (outs[1] == -77).all() and (outs[2] == SENTINEL).all()
    return rc, nnz.value, untouched, ctx._lib.otmb_last_error(ctx.handle).decode()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_every_refusal_leaves_the_outputs_unwritten(dev):
    v3D, area, _ = _grid("tiny_tripolar")
    idx = dict(zip(("wet", "Lwet3D", "N"), K.wet_indices(v3D)))
    idx["Lwet"] = np.flatnonzero(idx["wet"].ravel(order="F")) + 1
    nz = v3D.shape[2]
    wet = idx["wet"]
    nnz_ref = len(K.sink_ref(W, v3D, area)[1])
    # the call itself works on these arrays (what the refusals below are compared with)
    rc, nnz, untouched, _ = _raw_call(dev, v3D, area, idx, 0, W, None)
    assert (rc, nnz, untouched) == (0, nnz_ref, False)
    # w on the bottom face of a wet cell: negative, NaN, infinite -- in each of the three forms
    for bad in (-1e-9, np.nan, np.inf, -np.inf):
        w3 = np.where(wet, W, np.nan)
        w3[tuple(np.argwhere(wet)[11])] = bad
        wv = np.full(nz, W)
        wv[max(k for k in range(nz) if wet[:, :, k].any())] = bad  # the deepest level that holds a wet cell
        for form, ws, w in ((0, bad, None), (1, 0.0, wv), (2, 0.0, w3)):
            rc, nnz, untouched, msg = _raw_call(dev, v3D, area, idx, form, ws, w)
            assert rc == 11 and untouched and nnz == -5 and "w must be finite and >= 0" in msg, (bad, form, rc, msg)
    # garbage on a DRY cell is no refusal
    assert _raw_call(dev, v3D, area, idx, 2, 0.0, np.where(wet, W, -np.inf))[0] == 0
    # a NaN in the result (from the metrics): TSINK_NAN
    area2 = area.copy()
    area2[tuple(np.argwhere(wet[:, :, 0])[3])] = np.nan
    rc, nnz, untouched, msg = _raw_call(dev, v3D, area2, idx, 0, W, None)
    assert rc == 20 and untouched and msg == "Tsink contains NaNs."
    # another w_form, a capacity one short (nnz is reported), indices that are not makeindices'
    assert _raw_call(dev, v3D, area, idx, 3, W, None)[::2] == (11, True)
    rc, nnz, untouched, msg = _raw_call(dev, v3D, area, idx, 0, W, None, cap=nnz_ref - 1)
    assert (rc, nnz, untouched) == (14, nnz_ref, True)
    for tamper in ("rank", "lwet", "below"):
        bad = dict(idx, Lwet3D=idx["Lwet3D"].copy(), Lwet=idx["Lwet"].copy())
        if tamper == "rank":
            bad["Lwet3D"][tuple(np.argwhere(wet)[5])] += 1
        elif tamper == "lwet":
            bad["Lwet"][7] = v3D.size + 3  # out of the grid
        else:
            c = np.argwhere(wet[:, :, :-1] & wet[:, :, 1:])[2]
            bad["Lwet3D"][c[0], c[1], c[2] + 1] = idx["N"] + 9  # the cell below: beyond N
        rc, nnz, untouched, msg = _raw_call(dev, v3D, area, bad, 0, W, None)
        assert rc == 13 and untouched, (tamper, rc, msg)


def test_wrong_shapes_and_options_are_refused_before_the_library_is_called():
    import otmb_amd.api as api
    from otmb_amd import capi

    v3D, area, _ = _grid("tiny_tripolar")
    nx, ny, nz = v3D.shape
    idx = api.makeindices(v3D)
    gm = dict(v3D=v3D, area2D=area)
    asm = _asm("tiny_tripolar")
    for w in (np.ones(nz + 1), np.ones((nx, ny)), np.ones((nx, ny, nz + 1)), np.ones((nz, ny, nx))):
        with pytest.raises(capi.OtmbError) as e:
            api.buildTsink(w=w, gridmetrics=gm, indices=idx)
        assert e.value.name == "INVALID_ARG"
        with pytest.raises(capi.OtmbError) as e:
            asm.sinking(w)
        assert e.value.name == "INVALID_ARG"
    for call in (lambda: api.buildTsink(w=W, gridmetrics=gm, indices=idx, seafloor="shut"), lambda: asm.sinking(W, "shut"),
                 lambda: api.buildTsink(w=W, gridmetrics=dict(v3D=v3D, area2D=area[:, :-1]), indices=idx)):
        with pytest.raises(capi.OtmbError) as e:
            call()
        assert e.value.name == "INVALID_ARG"
    with pytest.raises(capi.OtmbError) as e:
        api.buildTsink(w=-W, gridmetrics=gm, indices=idx)
    assert e.value.name == "INVALID_ARG" and "w must be finite" in str(e.value)
    # and both are usable afterwards
    ref = K.sink_ref(W, v3D, area)
    S = api.buildTsink(w=W, gridmetrics=gm, indices=idx)
    _same((S.colptr, S.rowval, S.nzval), ref, "after the refusals")
    _same(_host(asm.sinking(W)), ref, "after the refusals, on the device")
