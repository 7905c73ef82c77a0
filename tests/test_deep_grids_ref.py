"""CPU: the grids of tests/deep_grids.py do put water, tile boundaries, flux signs and the edge of the mixed layer on the levels where the
counting flux kernels change registers (63 / 64) -- the conditions without which tests/test_ff_deep_levels.py would pass vacuously --
for every (shape, seed, topology) that it builds.  numpy and the oracle alone."""
import numpy as np
import pytest

import deep_grids as dg

IDS = [f"{'x'.join(map(str, s))}-{t}" for s, t in dg.GRIDS]
_ref = {}


def _reference(oracle, shape, topology):
    key = (shape, topology)
    if key not in _ref:
        g, gm = dg.case(shape, topology)
        idx = oracle.makeindices(gm.v3D)
        phi = oracle.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], g.umo.properties["_FillValue"], gm.gridtopology.kind)
        _ref[key] = (g, gm, idx, phi)
    return _ref[key]


def _levels_of_nonempty_columns(idx, csc, P):
    """Levels (0-based) of the cells whose column of the matrix holds an entry."""
    colptr = csc[0]
    return np.unique((idx["Lwet"][np.flatnonzero(np.diff(colptr) > 0)] - 1) // P)


@pytest.mark.parametrize("shape,topology", dg.GRIDS, ids=IDS)
def test_the_builder_keeps_its_promises(oracle, shape, topology):
    """The wet mask is the one asked for (makeindices reproduces it), columns are contiguous from the surface, land holds the fill value,
    the bottom cell is partial, and geometry, land mask and surface are make_grid's."""
    from otmb_amd import synthetic

    nx, ny, nz = shape
    g, gm, idx, _ = _reference(oracle, shape, topology)
    base = synthetic.make_grid(nx, ny, nz, seed=dg.SEED[shape], rho="array", topology=topology)
    wet = np.arange(nz)[None, None, :] < g.kb[:, :, None]
    assert np.array_equal(idx["wet3D"] != 0, wet)
    assert np.array_equal(g.kb > 0, np.asarray(base.volcello.data)[:, :, 0] > 0) and np.array_equal(np.isnan(g.mlotst), g.kb == 0)
    assert np.array_equal(g.areacello.data, base.areacello.data) and np.array_equal(g.lon_vertices, base.lon_vertices)
    fill = g.umo.properties["_FillValue"]
    for a in (g.umo.data, g.vmo.data):
        assert np.all(a[~wet] == fill) and np.all(a[wet] != fill)
    assert np.all(np.isnan(g.rho[~wet])) and np.all(np.isfinite(g.rho[wet]))
    _, dz = synthetic.levels(nz)
    thk = np.asarray(g.volcello.data) / np.asarray(g.areacello.data)[:, :, None]
    i, j = np.nonzero(g.kb)
    bottom = thk[i, j, g.kb[i, j] - 1] / dz[g.kb[i, j] - 1]
    assert bottom.min() >= 0.3 - 1e-12 and bottom.max() <= 1.0 + 1e-12 and bottom.min() < 0.5 < bottom.max()
    deep = g.kb[g.kb > 0] >= min(dg.DEEP_FROM, nz)
    assert 0.7 < deep.mean() < 1.0 or nz <= dg.DEEP_FROM  # most columns are deep, some are not
    assert idx["N"] <= 32000  # the GPU tests stay small


@pytest.mark.parametrize("shape,topology", dg.GRIDS, ids=IDS)
def test_water_tiles_and_flux_signs_on_the_upper_registers_levels(oracle, shape, topology):
    nx, ny, nz = shape
    g, gm, idx, phi = _reference(oracle, shape, topology)
    wet = idx["wet3D"] != 0
    if nz < 65:
        assert wet[:, :, nz - 1].any() and wet[:, :, max(nz - 2, 0)].any()
        return
    for k in range(62, nz):
        assert wet[:, :, k].any(), f"no wet cell at level {k}"
    # a boundary between two tiles of 256 columns (0-based wet rank a multiple of 256) on a level held in the upper registers
    P = nx * ny
    first_of_tile = idx["Lwet"][np.arange(0, idx["N"], 256)] - 1
    assert ((first_of_tile // P) >= 64).any()
    top = phi["top"][:, :, 64:][wet[:, :, 64:]]
    assert (top > 0).any() and (top < 0).any()
    if nz % 2:  # the pair step whose halves are at levels 64 and 63
        assert (wet[:, :, 64] & wet[:, :, 63]).any()


@pytest.mark.parametrize("shape,topology", dg.GRIDS, ids=IDS)
@pytest.mark.parametrize("upwind", [True, False], ids=["upwind", "centred"])
def test_the_mixed_layer_edge_cycles_over_the_register_boundary(oracle, shape, topology, upwind):
    """With ml_edge(g): TκVML has a non-empty column in a cell at each of the levels 62 ... 65, where nz allows (the edge lies above the
    last level: the deepest mixed level is nz - 2), and TκVdeep keeps some."""
    nx, ny, nz = shape
    g, gm, idx, phi = _reference(oracle, shape, topology)
    tm = oracle.transportmatrix(phi, gm, idx, g.rho, dg.ml_edge(g), g.kappaH, g.kappaVML, g.kappaVdeep, upwind)
    levels = _levels_of_nonempty_columns(idx, tm["TκVML"], nx * ny)
    for k in (62, 63, 64, 65):
        if k <= nz - 2:
            assert k in levels, f"no column of TκVML at level {k}: {levels}"
    assert len(tm["TκVdeep"][1]) > 0


@pytest.mark.parametrize("edge", [(62, 62), (63, 63), "whole"], ids=["below63", "below64", "whole"])
def test_the_three_mixed_layers_of_36x10x66(oracle, edge):
    """Edge just below level 63, just below level 64, and no edge at all: TκVML is not empty, its deepest column is where the edge says."""
    shape = (36, 10, 66)
    g, gm, idx, phi = _reference(oracle, shape, "tripolar")
    ml = dg.ml_whole_column(g) if edge == "whole" else dg.ml_edge(g, *edge)
    tm = oracle.transportmatrix(phi, gm, idx, g.rho, ml, g.kappaH, g.kappaVML, g.kappaVdeep, True)
    levels = _levels_of_nonempty_columns(idx, tm["TκVML"], 36 * 10)
    assert len(tm["TκVML"][1]) > 0
    assert levels.max() == (65 if edge == "whole" else edge[0])
    assert len(tm["TκVdeep"][1]) > 0  # (the background diffusion acts in the mixed layer too: never empty, says the oracle)
