"""Facefluxes, two levels per wave (facefluxes_pair_kernel; OTMB_FF_PAIRS, otmb_ctx_ff_pairs): lanes 0-31 of a wave take 32 columns at
level k, lanes 32-63 the same columns at level k - 1, and only the continuity recurrence crosses the halves.  Every case runs facefluxes
and the full transportmatrix with OTMB_FF_PAIRS=0 and =1, each in a fresh context, and compares bit for bit: the six ϕ arrays, the two
validity words, the five matrices and their nnz.  The pair kernel must have run, no step may count for itself or find counts that do
not describe the fluxes (OTMB_ERR_PUSH_MASK), and ϕ equals the oracle's."""
import ctypes as C

import numpy as np
import pytest

from helpers import COUNTS_ON, MATS, assert_csc_equal, gridmetrics_of, randomize_metrics

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not COUNTS_ON, reason="OTMB_COUNT_IN_FF=0: the pair kernel is a counting kernel")]

# (nx, ny, nz): the smallest shapes at which each rule can break
SHAPES = [
    (36, 30, 2),   # one step
    (36, 30, 3),   # odd nz: the upper half idles on the last step
    (12, 10, 7),   # the same with several steps and a chunk boundary
    (33, 5, 4),    # a half-wave spans several rows, the periodic wrap falls inside a half
    (70, 9, 5),    # nx above 64 and no multiple of 32
    (64, 40, 9),   # about 13 000 wet cells: tile boundaries of 256 columns fall inside halves at several levels
]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _run(monkeypatch, g, gm, pairs, upwind=True, mlotst=None):
    """One facefluxes + transportmatrix on a fresh context created under OTMB_FF_PAIRS=pairs."""
    import torch

    from otmb_amd.device import DeviceAssembler

    monkeypatch.setenv("OTMB_FF_PAIRS", str(pairs))
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst if mlotst is None else mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=upwind)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    fill = g.umo.properties["_FillValue"]
    phi = asm.facefluxes(umo, vmo, fill)
    ran = asm.ctx.ff_pairs()
    u, v = C.c_int32(-1), C.c_int32(-1)
    asm.ctx.check(asm.lib.otmb_facefluxes_slab_flags(asm.ctx.handle, C.byref(u), C.byref(v)))
    phis = [p.cpu().numpy().copy() for p in phi]
    asm.ctx.timing_enable(True)
    asm.transportmatrix_onepass(phi)
    kernels = asm.ctx.timing_collect()
    asm.ctx.timing_enable(False)
    got = asm.result_to_host()
    return dict(ran=ran, valid=(u.value, v.value), phi=phis, mats=got, nnz=list(asm.nnz), kernels=kernels)


def _compare(monkeypatch, g, gm, oracle=None, expect_pairs=1, **kw):
    a = _run(monkeypatch, g, gm, 0, **kw)
    b = _run(monkeypatch, g, gm, 1, **kw)
    assert a["ran"] == 0 and b["ran"] == expect_pairs, (a["ran"], b["ran"])
    for r in (a, b):
        assert "tm_count_kernel" not in r["kernels"] and "push_mask_kernel" not in r["kernels"], sorted(r["kernels"])
    assert a["valid"] == b["valid"] == (1, 1)
    for f in range(6):
        assert np.array_equal(_bits(a["phi"][f]), _bits(b["phi"][f])), f"ϕ[{f}] differs at {np.flatnonzero(_bits(a['phi'][f]) != _bits(b['phi'][f]))[:5]}"
    assert a["nnz"] == b["nnz"]
    for m in MATS:
        assert_csc_equal(b["mats"][m], a["mats"][m], m)
    if oracle is not None:
        idx = oracle.makeindices(gm.v3D)
        rphi = oracle.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], g.umo.properties["_FillValue"], gm.gridtopology.kind)
        names = ("east", "west", "north", "south", "top", "bottom")
        ref = [np.asfortranarray(rphi[n]).ravel(order="F") for n in names]
        for f in range(6):
            assert np.array_equal(_bits(ref[f]), _bits(b["phi"][f])), f"ϕ{names[f]} differs from the oracle's"
    return a, b


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(oracle, monkeypatch, shape):
    from otmb_amd import synthetic

    g = synthetic.make_grid(*shape, seed=41 + shape[0], rho="array")
    gm = gridmetrics_of(g)
    if shape[0] % 2:  # (odd nx, tripolar: the fold-centre cell is its own north neighbour at distance 0 -- the metrics are data to the kernels)
        randomize_metrics(gm)
    _compare(monkeypatch, g, gm, oracle)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("upwind", [True, False], ids=["upwind", "centred"])
@pytest.mark.parametrize("topology", ["tripolar", "bipolar"])
def test_topology_weighting_and_flux_type(oracle, monkeypatch, topology, upwind, f32):
    """The seam row (tripolar: the fold neighbour's flux and slot) lies inside the grid; 33 columns per row put it across halves."""
    from otmb_amd import synthetic

    g = synthetic.make_grid(33, 6, 5, seed=57, rho="array", topology=topology, dtype_flux=np.float32 if f32 else np.float64)
    _compare(monkeypatch, g, randomize_metrics(gridmetrics_of(g)), oracle, upwind=upwind)  # (odd nx: see test_shapes)


@pytest.mark.parametrize("nz", [6, 7])
def test_mixed_layer_edge_between_the_two_levels_of_a_pair(oracle, monkeypatch, nz):
    """mlotst per column halfway between zt[a] and zt[a + 1], a cycling over the columns: the edge of the mixed layer falls between the
    two levels of a pair and between two pairs, for either parity of nz."""
    from otmb_amd import synthetic

    g = synthetic.make_grid(36, 10, nz, seed=63, rho="array")
    zt = np.asarray(g.lev, dtype=np.float64)
    i, j = np.meshgrid(np.arange(36), np.arange(10), indexing="ij")
    a = (i + 3 * j) % (nz - 1)
    ml = np.asfortranarray(np.where(np.isnan(g.mlotst), np.nan, 0.5 * (zt[a] + zt[a + 1])))
    ra, rb = _compare(monkeypatch, g, gridmetrics_of(g), oracle, mlotst=ml)
    assert rb["nnz"][3] > 0  # TκVML is not empty


def test_nan_and_fill_values_in_the_transports(oracle, monkeypatch):
    from otmb_amd import synthetic

    g = synthetic.make_grid(36, 12, 5, seed=71, rho="array")
    rng = np.random.default_rng(3)
    fill = g.umo.properties["_FillValue"]
    for a in (g.umo.data, g.vmo.data):
        wetcells = np.argwhere(a != fill)
        for q, val in ((wetcells[rng.choice(len(wetcells), 40, replace=False)], np.nan), (wetcells[rng.choice(len(wetcells), 40, replace=False)], fill)):
            a[q[:, 0], q[:, 1], q[:, 2]] = val
    _compare(monkeypatch, g, gridmetrics_of(g), oracle)


def test_dry_cell_above_a_wet_one(monkeypatch):
    """An overhang: the vertical flux of the wet cell below meets land, which both kernels report in the same way (OTMB_ERR_FLUX_INTO_LAND)."""
    import otmb_amd
    from otmb_amd import synthetic
    from otmb_amd._nt import Cube
    from otmb_amd.capi import OtmbError

    g = synthetic.make_grid(36, 30, 6, seed=9, rho="array")
    vol = np.array(g.volcello.data, dtype=np.float64, order="F")
    wet = ~(np.isnan(vol) | (vol == 0))
    for level in (1, 2):  # the land cell in the upper and in the lower half of its step
        cand = np.argwhere(wet[:, 2:-3, level - 1] & wet[:, 2:-3, level] & wet[:, 2:-3, level + 1])
        i, j = (int(x) for x in cand[len(cand) // 2])
        v2 = vol.copy(order="F")
        v2[i, j + 2, level] = 0.0
        gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=Cube(v2, **g.volcello.properties), lon=g.lon, lat=g.lat, lev=g.lev,
                                      lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
        for pairs in (0, 1):
            with pytest.raises(OtmbError) as e:
                _run(monkeypatch, g, gm, pairs)
            assert e.value.name == "FLUX_INTO_LAND", (level, pairs)


def test_one_level_keeps_the_one_level_kernel(oracle, monkeypatch):
    from otmb_amd import synthetic

    g = synthetic.make_grid(36, 30, 1, seed=77, rho="array")
    _compare(monkeypatch, g, gridmetrics_of(g), oracle, expect_pairs=0)
