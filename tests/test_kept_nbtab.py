"""The kept operators' neighbour table (csrc/otmb_tm_kept.hip, tm_nbtab_kernel): a step that keeps TκH, TκVML and TκVdeep takes the wet ranks of a
regular column's six neighbours from a per-grid table in wet-rank order instead of gathering Lwet3D in cell order.  Every output array must be bit
for bit what the same steps write with OTMB_KEPT_NBTAB=0 (today's gathers; a child process: the switch is read once per process) and what a full
build writes; every way the table can go stale must lead to a rebuild; a non-canonical Lwet3D must fail the step as before (run with -m gpu).
Unmarked: the table's content restated in numpy -- the rule for ranks and presence."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import kept_nbtab_worker as W

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- CPU: the tables' content ---------------------------------------------------------------------------------------------------------------


def nbtab_reference(wet, tripolar):
    """The neighbour table of a grid with wet mask `wet` (nx, ny, nz; Julia's column-major linear order), restated.

    Per regular wet column c (nx >= 3, not on a tripolar grid's last row) and direction d in S, N, A, B, E, W: rank[c, d] is the neighbour's wet
    rank (its Lwet3D) when the neighbour exists (E / W always: periodic wrap; S: j > 0; N: j < ny - 1; A: k > 0; B: k < nz - 1) and is wet, else 0.
    Returns (cols, rank, Lwet, Lwet3D): cols the 0-based wet ranks of the regular columns."""
    nx, ny, nz = wet.shape
    flat = wet.ravel(order="F")
    Lwet = np.flatnonzero(flat)                      # 0-based linear indices, ascending
    Lwet3D = np.where(flat, np.cumsum(flat), 0)      # wet rank (1-based), 0 = dry
    P = nx * ny
    cols, rank = [], []
    for w, L in enumerate(Lwet):
        i, j, k = L % nx, (L // nx) % ny, L // P
        if nx < 3 or (tripolar and j == ny - 1):
            continue
        nbrs = [(j > 0, L - nx), (j + 1 < ny, L + nx), (k > 0, L - P), (k + 1 < nz, L + P),
                (True, L + (1 if i + 1 < nx else 1 - nx)), (True, L + (-1 if i > 0 else nx - 1))]
        cols.append(w)
        rank.append([int(Lwet3D[LX]) if exists else 0 for exists, LX in nbrs])
    return np.array(cols), np.array(rank).reshape(-1, 6), Lwet, Lwet3D


@pytest.mark.parametrize("name", ["nb_20x12x5_land60", "small_rho3d"])
def test_the_table_rule_names_valid_ranks_and_the_neighbours_presence(name):
    import helpers
    from otmb_amd import synthetic

    if name in W.EXTRA:
        kw = dict(W.EXTRA[name][0])
        g = synthetic.make_grid(kw.pop("nx"), kw.pop("ny"), kw.pop("nz"), **kw)
        gm = helpers.gridmetrics_of(g)
    else:
        g, gm = helpers.make_case(name)
    wet = ~np.isnan(np.asarray(gm.v3D))
    nx, ny, nz = wet.shape
    tripolar = "tripolar" in str(gm.gridtopology.name).lower()
    cols, rank, Lwet, Lwet3D = nbtab_reference(wet, tripolar)
    N = len(Lwet)
    present = rank != 0
    assert len(cols) > 0 and present.any() and (~present).any()
    # every stored rank is a rank of the grid, and fits the table's 32-bit word
    assert rank.min() >= 0 and rank.max() <= N < 2**31
    # a present neighbour is another cell than the column's own, and Lwet of its rank is the neighbour's linear index: the row index T gets
    assert not (rank == (cols + 1)[:, None]).any()
    P = nx * ny
    for q, w in enumerate(cols):
        L = Lwet[w]
        i, j, k = L % nx, (L // nx) % ny, L // P
        exists = [j > 0, j + 1 < ny, k > 0, k + 1 < nz, True, True]
        LXs = [L - nx, L + nx, L - P, L + P, L + (1 if i + 1 < nx else 1 - nx), L + (-1 if i > 0 else nx - 1)]
        for d, LX in enumerate(LXs):
            # presence equals Lwet3D != 0 of the neighbour
            assert present[q, d] == bool(exists[d] and Lwet3D[LX] != 0)
            if present[q, d]:
                assert Lwet[rank[q, d] - 1] == LX
    # ranks ascend in the column's row order A, S, (row-mates by index), N, B wherever present: what orders a column's rows
    for q in range(len(cols)):
        S, Nn, A, B = rank[q, :4]
        seq = [r for r in (A, S, cols[q] + 1, Nn, B) if r]
        assert seq == sorted(seq)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------


def _child(tmp_path_factory, value):
    out = str(tmp_path_factory.mktemp("nbtab") / f"nbtab{value}.json")
    env = dict(os.environ, OTMB_KEPT_NBTAB=value)
    r = subprocess.run([sys.executable, os.path.join(HERE, "kept_nbtab_worker.py"), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=1200)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    with open(out) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def off(tmp_path_factory):
    """Every scenario of kept_nbtab_worker, run once in a child process with OTMB_KEPT_NBTAB=0."""
    return _child(tmp_path_factory, "0")


@pytest.mark.gpu
@pytest.mark.parametrize("name,upwind,protocol", W.cases())
def test_table_gathers_and_full_builds_are_bit_identical(off, name, upwind, protocol):
    rec = W.run_case(name, upwind, protocol)
    zero = off["cases"][f"{name}|{upwind}|{protocol}"]
    for k in range(len(rec["kept"])):
        assert rec["kept"][k] == rec["full"][k], f"step {k}: table vs full build"
        assert rec["kept"][k] == zero["kept"][k], f"step {k}: table vs OTMB_KEPT_NBTAB=0"
    assert rec["kept_steps"] == zero["kept_steps"]
    assert sum(rec["kept_steps"]) >= (1 if protocol == "twophase" else 4)
    # the table was used here, and never in the fallback process
    assert rec["launches"].get("tm_nbtab_kernel", 0) >= 1
    assert "tm_nbtab_kernel" not in zero["launches"]
    assert rec["launches"]["tm_kernel<fill>"] == zero["launches"]["tm_kernel<fill>"]
    assert rec["kept_nbtab"] == 1 and zero["kept_nbtab"] == 0


@pytest.mark.gpu
def test_the_table_is_built_once_per_grid():
    from test_kept_ops import _fields, _pair

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    assert asm.ctx.kept_nbtab() == -1
    asm.ctx.timing_enable(True)
    for u, v in _fields(umo, vmo, 6, seed=5):
        asm.step_async(u, v, fill)
    asm.finish()
    n = W.launches(asm)
    assert n["tm_kernel<fill>"] == 6 and n["tm_nbtab_kernel"] == 1 and n["tm_htab_kernel"] == 1, n
    asm.ctx.timing_enable(False)
    assert asm.ctx.kept_nbtab() == 1 and asm.ctx.kept_htab() == 1


@pytest.mark.gpu
def test_nx2_uses_no_table_and_raises_no_error():
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("nx2")
    asm.ctx.timing_enable(True)
    for u, v in _fields(umo, vmo, 3, seed=2):
        _run(asm, "async", u, v, fill)
        _run(full, "async", u, v, fill)
        _same(_host(asm), _host(full), "nx2")
    assert asm._kept_last == KEPT
    assert asm.ctx.kept_nbtab() == 0
    assert "tm_nbtab_kernel" not in W.launches(asm)
    asm.ctx.timing_enable(False)


def _outcome(asm, u, v, fill):
    """One asynchronous step: its matrices on the host, or (error text, step) when it fails."""
    from otmb_amd.capi import OtmbError
    from test_kept_ops import _host, _run

    try:
        _run(asm, "async", u, v, fill)
    except OtmbError as e:
        return (str(e), e.step)
    return _host(asm)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["kappa", "thk", "edge", "v3d", "set_grid", "forget_given", "second_output_set"])
def test_every_invalidation_of_the_hkappa_table_rebuilds_this_table(how):
    """After the edit, the next kept step (the table built anew) equals a full build on the edited grid."""
    from test_kept_htab import _edit
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    fields = _fields(umo, vmo, 3, seed=17)
    for a in (asm, full):
        _run(a, "async", *fields[0], fill)
    _run(asm, "async", *fields[0], fill)
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1  # (the table exists for the old grid)
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
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1
    assert W.launches(asm).get("tm_nbtab_kernel", 0) == 1
    asm.ctx.timing_enable(False)


@pytest.mark.gpu
def test_a_changed_volume_reaches_the_next_kept_steps():
    """v3D edited in place (torch bumps the tensor's version: the assembler withholds the promise once, the library drops its tables (v3D is one of their keys)): the steps
    after it equal a full build on the edited grid -- and differ from what the old volumes gave."""
    from test_kept_ops import KEPT, _fields, _host, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    fields = _fields(umo, vmo, 3, seed=23)
    for k in (0, 1):
        _run(asm, "async", *fields[k], fill)
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1
    before = _host(asm)
    L = W.two_wet_cells(asm)[1]
    for a in (asm, full):
        a.v3d[L] *= 1.25
    for k in (1, 2, 2):
        _run(asm, "async", *fields[k], fill)
        _run(full, "async", *fields[k], fill)
        _same(_host(asm), _host(full), f"v3d, step {k}")
        if k == 1:
            assert not np.array_equal(_host(asm)["T"][2], before["T"][2])
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1


@pytest.mark.gpu
def test_a_changed_lwet3d_reaches_the_next_kept_steps():
    """Lwet3D edited in place, likewise: a dry cell beside a wet one is given a rank, which no longer is what the wet mask says.  The steps after it
    end as a full build's on the edited grid do: with the same matrices, or with the same error and step."""
    from test_kept_ops import KEPT, _fields, _pair, _run, _same

    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    fields = _fields(umo, vmo, 4, seed=29)
    for k in (0, 1):
        _run(asm, "async", *fields[k], fill)
        _run(full, "async", *fields[k], fill)
    assert asm._kept_last == KEPT and asm.ctx.kept_nbtab() == 1
    lw = asm.lwet3d.cpu().numpy()
    nx, ny = asm.nx, asm.ny
    dry = next(int(L) + 1 for L in asm.lwet[: asm.N].cpu().numpy() - 1
               if 0 < (L // nx) % ny < ny - 2 and L % nx + 1 < nx and lw[L + 1] == 0)  # the east neighbour of a wet cell, off the seam row
    for a in (asm, full):
        a.lwet3d[dry] = 1
    for k in (2, 3):
        got, want = _outcome(asm, *fields[k], fill), _outcome(full, *fields[k], fill)
        assert isinstance(got, tuple) == isinstance(want, tuple), (got if isinstance(got, tuple) else None, want if isinstance(want, tuple) else None)
        if isinstance(want, tuple):
            assert got == want
        else:
            _same(got, want, f"lwet3d, step {k}")


@pytest.mark.gpu
def test_a_noncanonical_lwet3d_fails_the_step_as_before(off):
    got = W.run_noncanonical_pipeline()
    assert got["error"] is not None and got["error"][1] == 0, got["error"]
    assert list(got["error"]) == off["noncanonical"]["error"]
    assert got["steps"] == off["noncanonical"]["steps"]
    assert all(s[0] != 0 for s in got["steps"]), got["steps"]
