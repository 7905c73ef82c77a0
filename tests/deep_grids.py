"""Grids with water where the counting flux kernels change registers: a wave of facefluxes_kernel<COUNTS> / facefluxes_pair_kernel keeps its
per-level tables one level per lane, levels 0-63 in one register and 64-127 in a second one (otmb_facefluxes.hip, FFC_MAX_NZ).
synthetic.make_grid stretches its levels over 5800 m whatever nz is, so that on a small plane hardly a column reaches level 63 and the
mixed layer (at most 1000 m) never does.  deep_grid() keeps make_grid's geometry, land mask and surface and fills the ocean columns
down to the deep levels; ml_edge() puts the edge of the mixed layer between two chosen levels."""
import numpy as np

import otmb_amd
from helpers import randomize_metrics
from otmb_amd import synthetic
from otmb_amd._nt import NT, Cube

DEEP_FROM = 60      # most columns end between this level count and nz
SHALLOW_SHARE = 0.15  # the others anywhere between 1 and nz


def deep_grid(nx, ny, nz, seed, topology="tripolar", f32=False):
    """synthetic.make_grid(nx, ny, nz, seed, rho="array") with another bathymetry: every ocean column (wet at the surface there) is wet
    in its first kb levels -- contiguous from the surface, so no overhang -- kb from min(60, nz) .. nz for most columns and from 1 .. nz
    for about 15 % of them, the bottom cell 30-100 % of its level's thickness.  volcello, umo, vmo and rho are drawn anew for that wet
    mask as make_grid draws them (fluxes scale with the cell's thickness, land holds the fill value), from a stream of their own."""
    g = synthetic.make_grid(nx, ny, nz, seed=seed, rho="array", topology=topology)
    rng = np.random.default_rng([seed, 64])
    _, dz = synthetic.levels(nz)
    area = np.asarray(g.areacello.data)
    ocean = np.asarray(g.volcello.data)[:, :, 0] > 0
    deep = rng.integers(min(DEEP_FROM, nz), nz + 1, (nx, ny))
    anywhere = rng.integers(1, nz + 1, (nx, ny))
    kb = np.where(rng.random((nx, ny)) < SHALLOW_SHARE, anywhere, deep)
    kb = np.where(ocean, kb, 0)
    part = rng.uniform(0.3, 1.0, (nx, ny))
    k = np.arange(nz)[None, None, :]
    thk = np.where(k < kb[:, :, None] - 1, dz[None, None, :], 0.0)
    thk = np.where(k == kb[:, :, None] - 1, part[:, :, None] * dz[None, None, :], thk)
    vol = np.asfortranarray(thk * area[:, :, None])
    wet = vol > 0
    sig = 1.0e9 * thk / dz.max()
    umo = np.asfortranarray(rng.standard_normal((nx, ny, nz)) * sig)
    vmo = np.asfortranarray(rng.standard_normal((nx, ny, nz)) * sig)
    umo[~wet] = synthetic.FILL
    vmo[~wet] = synthetic.FILL
    fill = synthetic.FILL
    if f32:
        umo, vmo = np.asfortranarray(umo.astype(np.float32)), np.asfortranarray(vmo.astype(np.float32))
        fill = float(np.float32(synthetic.FILL))
    zc = np.cumsum(thk, axis=2) - 0.5 * thk
    rho = np.asfortranarray(np.where(wet, 1025.0 + 0.004 * zc + 0.1 * rng.standard_normal((nx, ny, nz)), np.nan))
    out = NT(g)
    out.update(volcello=Cube(vol, **g.volcello.properties), umo=Cube(umo, _FillValue=fill), vmo=Cube(vmo, _FillValue=fill), rho=rho, kb=kb)
    return out


def deep_gridmetrics(g):
    """makegridmetrics of the new volcello (as tests/test_ff_pairs.py::test_dry_cell_above_a_wet_one rebuilds them); random 2-D metrics
    where nx is odd (tripolar: the fold-centre cell is its own north neighbour at distance 0 -- the metrics are data to the kernels)."""
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    return randomize_metrics(gm) if g.nx % 2 else gm


def ml_edge(g, lo=60, hi=67):
    """mlotst halfway between zt[a] and zt[a + 1], a = lo + (i + 3 j) % (hi - lo + 1) clipped to nz - 2: the construction of
    tests/test_ff_pairs.py::test_mixed_layer_edge_between_the_two_levels_of_a_pair, moved to the register boundary.  NaN on land."""
    zt = np.asarray(g.lev, dtype=np.float64)
    i, j = np.meshgrid(np.arange(g.nx), np.arange(g.ny), indexing="ij")
    a = np.clip(lo + (i + 3 * j) % (hi - lo + 1), 0, max(g.nz - 2, 0))
    return np.asfortranarray(np.where(np.isnan(g.mlotst), np.nan, 0.5 * (zt[a] + zt[np.minimum(a + 1, g.nz - 1)])))


def ml_whole_column(g):
    """The whole column is mixed: +inf on ocean columns, NaN on land."""
    return np.asfortranarray(np.where(np.isnan(g.mlotst), np.nan, np.inf))


# ---- what tests/test_ff_deep_levels.py runs, and tests/test_deep_grids_ref.py checks on the CPU ------------------------------------------
# (nx, ny, nz): the smallest shapes at which each rule can break
SHAPES = [
    (33, 6, 63),    # control: everything in the lower registers
    (33, 6, 64),    # lane 63 of the lower half; the clamp of the upper half's level index with nothing above
    (33, 6, 65),    # first level in the upper registers; the pair step (64, 63) straddles the boundary; odd nz
    (36, 10, 66),   # pair step (65, 64) entirely above, (63, 62) below; even nz
    (70, 9, 65),    # two column blocks per row; four-row workgroup with rows beyond the grid
    (33, 6, 127),   # odd; last lane but one of the upper half
    (36, 10, 128),  # the limit itself: lane 63 of the upper half
]
BEYOND = [(36, 10, 129), (36, 10, 130)]  # past FFC_MAX_NZ: the plain kernel and a counting pass
OPTION_SHAPES = [(36, 10, 66), (36, 10, 128)]
# seeds chosen on the CPU so that every condition of tests/test_deep_grids_ref.py holds (a tile boundary on the one or two levels above 63
# of a 65- or 66-level grid is the rare one)
SEED = {(33, 6, 63): 163, (33, 6, 64): 164, (33, 6, 65): 170, (36, 10, 66): 167, (70, 9, 65): 265, (33, 6, 127): 227, (36, 10, 128): 228,
        (36, 10, 129): 229, (36, 10, 130): 230}
# every (shape, topology) the GPU tests build
GRIDS = [(s, "tripolar") for s in SHAPES + BEYOND] + [(s, "bipolar") for s in OPTION_SHAPES]
_cache = {}


def case(shape, topology="tripolar", f32=False):
    """(grid, gridmetrics) of a shape of the lists above: built once and left unchanged."""
    key = (tuple(shape), topology, f32)
    if key not in _cache:
        g = deep_grid(*shape, seed=SEED[tuple(shape)], topology=topology, f32=f32)
        _cache[key] = (g, deep_gridmetrics(g))
    return _cache[key]
