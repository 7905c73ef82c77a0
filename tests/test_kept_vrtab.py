"""The kept operators' {v3D, ρ} table (csrc/otmb_tm_kept.hip, tm_vrtab_kernel): a step that keeps TκH, TκVML and TκVdeep, reads the neighbour
table and is promised an unchanged 3-D ρ (OTMB_KEPT_RHO) takes the volumes and densities of a regular column and its six neighbours from one
16-byte record per wet column in wet-rank order instead of 7 + 7 gathers in cell order.  Every output array must be bit for bit what the same
steps write with OTMB_KEPT_VRTAB=0 (today's gathers; a child process: the switch is read once per process) and what a full build writes; the
table must be built once while ρ stays, never while ρ changes, and again after every way it can go stale (run with -m gpu).
Unmarked: the table's rule restated in numpy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kept_vrtab_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- CPU: the table's rule ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["vr_20x12x5_land60", "vr_20x12x1_island", "small_rho3d"])
def test_record_rank_minus_one_holds_what_the_cell_order_gather_reads(name):
    """Record w is {v3D, ρ} at the cell of wet rank w + 1.  A regular column reads its own record and, per neighbour, record rank - 1: for a
    present neighbour the very values the gathers v3D[LX], ρ[LX] read; an absent one (rank 0) names the column's own record."""
    from test_kept_nbtab import nbtab_reference

    g, gm = W.grid(name)
    v = np.asarray(gm.v3D).ravel(order="F")
    rho = np.asarray(g.rho).ravel(order="F")
    wet = ~np.isnan(np.asarray(gm.v3D))
    nx, ny, nz = wet.shape
    tripolar = "tripolar" in str(gm.gridtopology.name).lower()
    cols, rank, Lwet, Lwet3D = nbtab_reference(wet, tripolar)
    N = len(Lwet)
    assert 16 * N < 2**32 and N % 64 != 0 and N % 256 != 0
    table = np.stack([v[Lwet], rho[Lwet]], axis=1)  # what tm_vrtab_kernel stores
    assert table.shape == (N, 2) and not np.isnan(table).any()
    P = nx * ny
    read = set()
    isolated = 0
    for q, w in enumerate(cols):
        L = Lwet[w]
        i = L % nx
        LXs = [L - nx, L + nx, L - P, L + P, L + (1 if i + 1 < nx else 1 - nx), L + (-1 if i > 0 else nx - 1)]
        assert table[w, 0] == v[L] and table[w, 1] == rho[L]
        read.add(int(w))
        isolated += not rank[q].any()
        for d, LX in enumerate(LXs):
            r = int(rank[q, d])
            rec = r - 1 if r else int(w)  # (a rank of 0 loads at the column's own rank)
            assert 0 <= rec < N
            read.add(rec)
            if r:
                assert table[rec, 0] == v[LX] and table[rec, 1] == rho[LX]
            else:
                assert rec == w
    # the first and the last record are among those read
    assert min(read) == 0 and max(read) == N - 1
    if name == "vr_20x12x1_island":
        assert isolated >= 1


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------


def _child(tmp_path_factory, value):
    out = str(tmp_path_factory.mktemp("vrtab") / f"vrtab{value}.json")
    env = dict(os.environ, OTMB_KEPT_VRTAB=value)
    r = subprocess.run([sys.executable, os.path.join(HERE, "kept_vrtab_worker.py"), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    """Every scenario of kept_vrtab_worker, run once in a child process with OTMB_KEPT_VRTAB=0."""
    return _child(tmp_path_factory, "0")


@pytest.mark.gpu
@pytest.mark.parametrize("name,upwind,protocol", W.cases())
def test_table_gathers_and_full_builds_are_bit_identical(off, name, upwind, protocol):
    rec = W.run_case(name, upwind, protocol)
    zero = off["cases"][f"{name}|{upwind}|{protocol}"]
    for k in range(len(rec["kept"])):
        assert rec["kept"][k] == rec["full"][k], f"step {k}: table vs full build"
        assert rec["kept"][k] == zero["kept"][k], f"step {k}: table vs OTMB_KEPT_VRTAB=0"
    assert rec["kept_steps"] == zero["kept_steps"]
    assert sum(rec["kept_steps"]) >= (1 if protocol == "twophase" else 4)
    # the table was used here, and never in the fallback process (which still reads the neighbour table)
    assert rec["launches"].get("tm_vrtab_kernel", 0) >= 1
    assert "tm_vrtab_kernel" not in zero["launches"]
    assert rec["launches"]["tm_kernel<fill>"] == zero["launches"]["tm_kernel<fill>"]
    assert rec["kept_vrtab"] == 1 and zero["kept_vrtab"] == 0
    assert rec["kept_nbtab"] == 1 and zero["kept_nbtab"] == 1


@pytest.mark.gpu
def test_the_table_is_built_once_while_rho_stays():
    from test_kept_ops import _fields, _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    assert asm.ctx.kept_vrtab() == -1
    asm.ctx.timing_enable(True)
    for u, v in _fields(umo, vmo, 6, seed=5):
        asm.step_async(u, v, fill)
    asm.finish()
    n = W.launches(asm)
    assert n["tm_kernel<fill>"] == 6 and n["tm_vrtab_kernel"] == 1 and n["tm_nbtab_kernel"] == 1 and n["tm_htab_kernel"] == 1, n
    asm.ctx.timing_enable(False)
    assert asm.ctx.kept_vrtab() == 1 and asm.ctx.kept_nbtab() == 1


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["another_tensor", "in_place"])
def test_the_table_is_never_built_while_rho_changes(how):
    """ρ is another tensor, or is edited in place, before every step: no step can promise it, so no step builds or reads the table."""
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    L = W.wet_regular_cell(asm)
    asm.ctx.timing_enable(True)
    for k, (u, v) in enumerate(_fields(umo, vmo, 4, seed=7)):
        for a in (asm, full):
            if how == "another_tensor":
                a.rho = a.rho.clone()
            else:
                a.rho[L] *= 1.0 + 0.01 * (k + 1)
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        _same(_host(asm), _host(full), f"{how}, step {k}")
        if k:
            assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1 and asm.ctx.kept_vrtab() == 0
    assert "tm_vrtab_kernel" not in W.launches(asm)
    asm.ctx.timing_enable(False)


@pytest.mark.gpu
def test_rho_edited_in_place_skips_the_table_once_and_rebuilds_it():
    """ρ edited in place at one wet cell (torch bumps the tensor's version: the assembler withholds the promise once, the library drops the
    table): the next step gathers, the one after builds the table anew; both equal a full build on the edited ρ and differ from before."""
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    fields = _fields(umo, vmo, 3, seed=23)
    for k in (0, 1):
        _run(asm, "async", *fields[k], fill)
    assert asm._kept_last == KEPT and asm.ctx.kept_vrtab() == 1
    before = _host(asm)
    L = W.wet_regular_cell(asm)
    for a in (asm, full):
        a.rho[L] *= 1.25
    asm.ctx.timing_enable(True)
    for n, k in enumerate((1, 2)):
        _run(asm, "async", *fields[k], fill)
        _run(full, "async", *fields[k], fill)
        _same(_host(asm), _host(full), f"rho, step {k}")
        assert asm._kept_last == KEPT and asm.ctx.kept_vrtab() == n  # (0: gathered, then 1: the table, rebuilt)
        if k == 1:
            assert not np.array_equal(_host(asm)["T"][2], before["T"][2])
    assert W.launches(asm).get("tm_vrtab_kernel", 0) == 1
    asm.ctx.timing_enable(False)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["kappa", "thk", "edge", "v3d", "set_grid", "forget_given", "second_output_set"])
def test_every_invalidation_of_the_hkappa_table_rebuilds_this_table(how):
    """After the edit, the next kept step (the tables built anew) equals a full build on the edited grid."""
    from test_kept_htab import _edit
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    fields = _fields(umo, vmo, 3, seed=17)
    for a in (asm, full):
        _run(a, "async", *fields[0], fill)
    _run(asm, "async", *fields[0], fill)
    assert asm._kept_last == KEPT and asm.ctx.kept_vrtab() == 1  # (the table exists for the old grid)
    asm.ctx.timing_enable(True)
    if how in ("kappa", "thk", "edge", "v3d", "set_grid"):
        for a in (asm, full):
            _edit(a, how, g, gm)
    elif how == "forget_given":
        asm.ctx.forget_given()
    elif how == "second_output_set":
        other = asm.new_output_set()
        asm.transportmatrix_onepass(asm.facefluxes(*fields[1], fill), out=other)
    for k in (1, 2):
        _run(asm, "async", *fields[k], fill)
        _run(full, "async", *fields[k], fill)
        _same(_host(asm), _host(full), f"{how}, step {k}")
    assert asm._kept_last == KEPT and asm.ctx.kept_vrtab() == 1
    n = W.launches(asm)
    assert n.get("tm_vrtab_kernel", 0) == 1 and n.get("tm_htab_kernel", 0) == 1, n
    asm.ctx.timing_enable(False)


@pytest.mark.gpu
def test_a_nan_rho_fails_the_pipeline_as_before(off):
    got = W.run_rho_nan_pipeline()
    assert got["error"] is not None and got["error"][1] == 0, got["error"]
    assert list(got["error"]) == off["nan"]["error"]
    assert got["steps"] == off["nan"]["steps"]
    assert all(s[0] != 0 for s in got["steps"]), got["steps"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_tripolar", "nx2"])
def test_scalar_rho_and_nx2_use_no_table_and_raise_no_error(name):
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair(name)
    assert asm.rho is None  # (a scalar ρ)
    asm.ctx.timing_enable(True)
    for u, v in _fields(umo, vmo, 3, seed=2):
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        _same(_host(asm), _host(full), name)
    assert asm._kept_last == KEPT
    assert asm.ctx.kept_vrtab() == 0 and asm.ctx.kept_nbtab() == (0 if name == "nx2" else 1)
    assert "tm_vrtab_kernel" not in W.launches(asm)
    asm.ctx.timing_enable(False)


@pytest.mark.gpu
def test_a_first_depth_slab_uses_no_table_and_raises_no_error():
    """A first depth slab as the library sees it: wet_base 0, the columns of the upper levels owned, the level below named by Lwet3D as
    neighbours only -- ranks beyond n_wet, of which the table (owned columns only) has no record.  The neighbour table is read, this one is not."""
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    P = asm.nx * asm.ny
    n_own = int((asm.lwet[: asm.N] <= P * (asm.nz - 2)).sum())
    assert 0 < n_own < asm.N
    for a in (asm, full):
        a.count_in_ff = False  # (the counts that come with the fluxes are the whole grid's: the counting pass counts the owned columns)
        a.N = n_own
    asm.ctx.timing_enable(True)
    for u, v in _fields(umo, vmo, 3, seed=4):
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        _same(_host(asm), _host(full), "first slab")
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1 and asm.ctx.kept_vrtab() == 0
    assert "tm_vrtab_kernel" not in W.launches(asm)
    asm.ctx.timing_enable(False)
