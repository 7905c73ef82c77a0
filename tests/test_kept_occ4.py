"""The lean kept fill (csrc/otmb_transportmatrix.hip, tm_kernel's GIVEN bit 6): whenever a kept step reads the {v3D, ρ} table it runs an
instantiation of the fill kernel that fits four waves per SIMD -- the seam row's generic builder loads in stages, row indices are 32-bit in
registers -- and must write, bit for bit, what the three-wave instantiation (OTMB_KEPT_OCC4=0; a child process: the switch is read once per
process) and a full build write: on the grids of kept_vrtab_worker, on a two-tile grid whose last tile ends inside a wave and leaves a wave
empty (tripolar: seam-row columns inside the lean kernel; bipolar), through an exact cancellation, a capacity one short and a NaN ρ
(run with -m gpu).  Unmarked: the two-tile grid is what the GPU cases count on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kept_occ4_worker as K
import kept_vrtab_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- CPU: the grid ----------------------------------------------------------------------------------------------------------------------------


def test_the_two_tile_grid_ends_inside_a_wave_leaves_a_wave_empty_and_wraps():
    masks = {}
    for name in K.GRIDS:
        g, gm = K.grid(name)
        wet = ~np.isnan(np.asarray(gm.v3D))
        nx, ny, nz = wet.shape
        n = int(wet.sum())
        assert 256 < n < 512             # two tiles of 256 columns
        assert n % 64 != 0               # the last tile ends inside a wave ...
        assert 0 < n % 256 <= 192        # ... and leaves at least one of its four waves empty
        assert 16 * n < 2**32
        assert wet[0].any() and wet[nx - 1].any()  # columns at i = 0 and i = nx - 1: the periodic wrap orders
        # ... regular ones among them (off the seam row), with their east / west neighbour across the wrap wet
        assert (wet[0, : ny - 1] & wet[nx - 1, : ny - 1]).any()
        assert wet[:, ny - 1].sum() >= 8  # the seam row (tripolar: the generic builder)
        # the seam row's columns share waves with regular ones: some level holds both among 64 consecutive wet ranks
        rank = np.cumsum(wet.ravel(order="F")).reshape(wet.shape, order="F")
        seam_waves = set(((rank[:, ny - 1][wet[:, ny - 1]] - 1) // 64).tolist())
        regular_waves = set(((rank[:, : ny - 1][wet[:, : ny - 1]] - 1) // 64).tolist())
        assert seam_waves & regular_waves
        masks[name] = wet
    assert np.array_equal(masks["occ4_tripolar"], masks["occ4_bipolar"])
    g, gm = K.grid("occ4_tripolar")
    assert "tripolar" in str(gm.gridtopology.name).lower()
    g, gm = K.grid("occ4_bipolar")
    assert "bipolar" in str(gm.gridtopology.name).lower()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    """Every scenario of kept_occ4_worker, run once in a child process with OTMB_KEPT_OCC4=0."""
    out = str(tmp_path_factory.mktemp("occ4") / "occ4_0.json")
    env = dict(os.environ, OTMB_KEPT_OCC4="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "kept_occ4_worker.py"), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    with open(out) as f:
        return json.load(f)


def _three_ways(rec, zero, min_kept):
    for k in range(len(rec["kept"])):
        assert rec["kept"][k] == rec["full"][k], f"step {k}: lean kernel vs full build"
        assert rec["kept"][k] == zero["kept"][k], f"step {k}: lean kernel vs OTMB_KEPT_OCC4=0"
    assert rec["kept_steps"] == zero["kept_steps"]
    assert sum(rec["kept_steps"]) >= min_kept
    assert rec["kept_occ4"] == 1 and zero["kept_occ4"] == 0
    assert rec["kept_vrtab"] == 1 and zero["kept_vrtab"] == 1
    # step by step: 1 only where the fallback process says 0 (a kept fill), and what that process says everywhere else (-1: no kept fill yet)
    assert all(r == z or (r == 1 and z == 0) for r, z in zip(rec["occ4_steps"], zero["occ4_steps"])), (rec["occ4_steps"], zero["occ4_steps"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,upwind,protocol", W.cases())
def test_lean_three_wave_and_full_builds_are_bit_identical(off, name, upwind, protocol):
    rec = K.run_case(name, upwind, protocol)
    _three_ways(rec, off["cases"][f"{name}|{upwind}|{protocol}"], 1 if protocol == "twophase" else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("name,upwind,protocol", K.own_cases())
def test_two_tile_grid_partial_wave_empty_wave_seam_and_wrap(off, name, upwind, protocol):
    rec = K.run_case(name, upwind, protocol)
    _three_ways(rec, off["cases"][f"{name}|{upwind}|{protocol}"], 1 if protocol == "twophase" else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_tripolar", "nx2"])
def test_scalar_rho_and_nx2_do_not_run_the_lean_kernel(name):
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair(name)
    assert asm.rho is None and asm.ctx.kept_occ4() == -1
    for u, v in _fields(umo, vmo, 3, seed=2):
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        _same(_host(asm), _host(full), name)
    assert asm._kept_last == KEPT and asm.ctx.kept_vrtab() == 0 and asm.ctx.kept_occ4() == 0
    assert full.ctx.kept_occ4() == -1  # (no kept fill on that context)


@pytest.mark.gpu
def test_a_first_depth_slab_does_not_run_the_lean_kernel():
    """test_kept_vrtab's first slab (ranks beyond n_wet: the neighbour table is read, the {v3D, ρ} table is not)."""
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    P = asm.nx * asm.ny
    n_own = int((asm.lwet[: asm.N] <= P * (asm.nz - 2)).sum())
    assert 0 < n_own < asm.N
    for a in (asm, full):
        a.count_in_ff = False
        a.N = n_own
    for u, v in _fields(umo, vmo, 3, seed=4):
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        _same(_host(asm), _host(full), "first slab")
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1 and asm.ctx.kept_vrtab() == 0 and asm.ctx.kept_occ4() == 0


@pytest.mark.gpu
def test_an_exact_cancellation_is_flagged_and_compacted_as_before(off):
    rec, zero = K.run_cancellation(), off["cancel"]
    for k in range(len(rec["kept"])):
        assert rec["nnzT"][k] < rec["union"][k], f"step {k}: nothing cancelled"  # (the compaction ran: T is shorter than its reserved pattern)
        assert rec["kept"][k] == rec["full"][k], f"step {k}: lean kernel vs full build"
        assert rec["kept"][k] == zero["kept"][k], f"step {k}: lean kernel vs OTMB_KEPT_OCC4=0"
    assert rec["nnzT"] == zero["nnzT"] and rec["union"] == zero["union"] and rec["kept_steps"] == zero["kept_steps"]
    assert sum(rec["kept_steps"]) >= 3
    assert rec["occ4_steps"][1:] == [1] * (len(rec["kept"]) - 1) and zero["occ4_steps"][1:] == [0] * (len(rec["kept"]) - 1)


@pytest.mark.gpu
def test_a_capacity_one_short_is_reported_as_before(off):
    from otmb_amd import capi

    rec, zero = K.run_capacity(), off["capacity"]
    assert rec["error"] is not None and rec["error"][0] == capi.CAPACITY, rec["error"]
    assert rec["error"] == zero["error"] and rec["steps"] == zero["steps"]
    assert rec["occ4"] == 1 and zero["occ4"] == 0 and rec["vrtab"] == 1 and zero["vrtab"] == 1  # (the lean kernel is what ran out of room)


@pytest.mark.gpu
def test_a_nan_rho_fails_the_pipeline_as_before(off):
    got = W.run_rho_nan_pipeline()
    assert got["error"] is not None and got["error"][1] == 0, got["error"]
    assert list(got["error"]) == off["nan"]["error"]
    assert got["steps"] == off["nan"]["steps"]
    assert all(s[0] != 0 for s in got["steps"]), got["steps"]
