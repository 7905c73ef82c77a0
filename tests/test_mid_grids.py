"""The fill pass's variants on grids of MORE THAN ONE SCAN GROUP (tests/mid_grids.py; run with -m gpu): default builds, kept steps, exact
cancellation with its compaction, given operators, T alone, single operators, the general path and the one-pass protocol with all scan levels,
each against the oracle, bit for bit -- nothing here carries a tolerance.  tests/test_mid_grids_ref.py asserts on the CPU that the grids span the
scan groups, seam-row tiles and cancellations these tests count on.

Scan groups (1024 tiles each) the paths run with, from the grids' asserted sizes:
  mid  (328 x 100 x 17, ~340 k wet cells): fill pass / tile counts 2 (1327 tiles of 256 columns); spadd 2; sparse() of Tadv's 1.9 M triplets 8 (256 sorted entries a tile);
  wide (1040 x 512 x 4, ~1.2 M wet cells): fill pass 5; makeindices 3 (1024 cells a tile); tfix 2 (1024 columns a tile).
Not reached: tilescan_top's loop beyond 1024 groups needs more than 2^28 elements and stays with the 0.1 degree run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mid_grids as mg
import mid_grids_worker as W
from helpers import COUNTS_ON, MATS, assert_csc_equal
from mid_grids_worker import KEPT, assembler, assert_matrices, dev

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
OPS = MATS[1:]
PROTOCOLS = ["async", "pipeline", "fused", "twophase"]


def _run(asm, protocol, u, v, fill):
    from test_kept_ops import _run as run

    if protocol == "fused" and not COUNTS_ON:
        pytest.skip("the fused step needs the counts in facefluxes")
    run(asm, protocol, u, v, fill)


def _fields(name, which):
    u, v, fill = mg.field(name, which)
    return dev(u), dev(v), fill


def _assert_phi(oracle, asm, name, which):
    """The six ϕ by the sign test of tests/test_baseline_configs.py."""
    rphi = mg.facefluxes(oracle, name, which)
    for q, d in enumerate(oracle.PHI_ORDER):
        got = asm.phi[q].cpu().numpy()
        want = rphi[d].ravel(order="F")
        same = (got == want) & (np.signbit(got) == np.signbit(want))
        assert same.all(), (d, np.flatnonzero(~same)[:3])


def _fold(oracle, ops, N):
    """T = ((Tadv + TκH) + TκVML) + TκVdeep with the oracle's sparse add, as tests/test_given_ops.py folds it."""
    return oracle.spadd(oracle.spadd(oracle.spadd(ops["Tadv"], ops["TκH"], N), ops["TκVML"], N), ops["TκVdeep"], N)


def _to_dev(asm, csc):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(asm.device) for x in csc)


# ---- mid grid: default builds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho", ["array", "scalar"])
@pytest.mark.parametrize("upwind", [True, False])
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_mid_default_build_matches_the_oracle(oracle, protocol, upwind, rho):
    """One step of each protocol on a fresh assembler (nothing kept): two scan groups of tile counts, the group base added by the fill pass
    (async, pipeline, fused) or by the scan's third level (two-phase), tiles whose south / north neighbours lie in other tiles."""
    asm = assembler("mid", rho=rho, upwind=upwind)
    assert asm.N == mg.indices(oracle, "mid")["N"]
    u, v, fill = _fields("mid", "step0")
    _run(asm, protocol, u, v, fill)
    assert asm._kept_last == (KEPT if protocol == "pipeline" else ())  # (a pipeline's second and third step keep what its first one wrote)
    # the counting whole-plane call marches two levels per wave on this grid (ceil(P / 32) far below 16 x CUs)
    assert asm.ctx.ff_pairs() == (1 if COUNTS_ON else 0)
    # two scan groups: the one-pass protocols leave the group base to the fill pass, the two-phase plan scans all levels
    assert asm.ctx.tm_infill() == (1 if protocol != "twophase" and asm.ctx.tm_infill_groups() >= 2 else 0)
    assert_matrices(asm, mg.reference(oracle, "mid", "step0", rho=rho, upwind=upwind), f"mid/{protocol}/upwind={upwind}/rho={rho}")
    if protocol == "async" and upwind and rho == "array":
        _assert_phi(oracle, asm, "mid", "step0")


@pytest.mark.parametrize("protocol", ["async", "fused"])
def test_mid_float32_transports(oracle, protocol):
    import torch

    asm = assembler("mid")
    u, v, fill = _fields("mid", "f32")
    assert u.dtype == torch.float32
    _run(asm, protocol, u, v, fill)
    assert_matrices(asm, mg.reference(oracle, "mid", "f32"), f"mid/f32/{protocol}")
    if protocol == "async":
        _assert_phi(oracle, asm, "mid", "f32")


# ---- mid grid: kept steps against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", PROTOCOLS)
def test_mid_kept_steps_match_the_oracle(oracle, protocol):
    """The kept-step tests elsewhere compare a kept build with a full build of the same library, on grids of one scan group; here every kept step
    is compared with the oracle, with the tables (TκH, neighbour ranks, {v3D, ρ}) and T's kept pattern in use."""
    if protocol == "fused" and not COUNTS_ON:
        pytest.skip("the fused step needs the counts in facefluxes")
    rec = W.kept_sequence(oracle, protocol)
    W.check_kept_record(rec, protocol)
    if protocol != "twophase":
        assert rec["tables"] == {"htab": 1, "nbtab": 1, "vrtab": 1}, rec
    assert rec["infill"] == [1 if protocol != "twophase" and rec["infill_groups"] >= 2 else 0] * len(W.STEPS), rec


# what each switch at "0" leaves of (TκH table, neighbour table, {v3D, ρ} table, T's kept pattern): OTMB_KEPT_HTAB=0 implies the others,
# OTMB_KEPT_NBTAB=0 implies OTMB_KEPT_VRTAB=0 (csrc/otmb_tm_kept.hip)
SWITCHES = {"OTMB_KEPT_NBTAB": (1, 0, 0, 1), "OTMB_KEPT_HTAB": (0, 0, 0, 0), "OTMB_KEPT_VRTAB": (1, 1, 0, 1), "OTMB_KEPT_TPAT": (1, 1, 1, 0)}


CHILD_SECONDS = 300
STOP_AFTER = (134, 139, -6, -11)  # an abort or a segmentation fault of a child: nothing more is started on the GPU


@pytest.fixture(scope="module")
def switched(oracle, tmp_path_factory):
    """The kept-step sequence once per switch at its non-default value (the switches are read once per process): one child process after the
    other, each under its own time limit and comparing with the oracle itself (built by the `oracle` fixture before the first one starts).
    After a child that aborted, faulted or ran out of time no further child is started: the remaining cases fail."""
    d = tmp_path_factory.mktemp("mid_switches")
    res, stopped = {}, None
    for name in SWITCHES:
        out = str(d / f"{name}.json")
        if stopped is not None:
            res[name] = (None, f"not started: the child of {stopped[0]} ended with {stopped[1]}", out)
            continue
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "mid_grids_worker.py"), out], env=dict(os.environ, **{name: "0"}),
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_SECONDS)
            rc, log = r.returncode, r.stdout
        except subprocess.TimeoutExpired as e:
            rc, log = "its time limit", e.stdout or b""
        res[name] = (rc, log.decode(errors="replace")[-3000:], out)
        if rc in STOP_AFTER or rc == "its time limit":
            stopped = (name, rc)
    return res


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_mid_kept_steps_with_a_switch_off_match_the_oracle(switched, switch):
    """The gather paths (no table) at this size: the same sequence, the same oracle, the switch's table not read."""
    rc, log, out = switched[switch]
    assert rc == 0, log
    with open(out) as f:
        res = json.load(f)
    htab, nbtab, vrtab, tpat = SWITCHES[switch]
    assert set(res) == {p for p in PROTOCOLS if p != "fused" or COUNTS_ON}
    for protocol, rec in res.items():
        W.check_kept_record(rec, protocol, tpat_on=bool(tpat))
        if protocol != "twophase":
            assert rec["tables"] == {"htab": htab, "nbtab": nbtab, "vrtab": vrtab}, (protocol, rec)
        assert rec["infill"] == [1 if protocol != "twophase" and rec["infill_groups"] >= 2 else 0] * len(W.STEPS), (protocol, rec)


# ---- mid grid: cancellation and compaction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["alone", "pipeline"])
def test_mid_cancellation_is_compacted_and_the_next_step_written_in_full(oracle, how):
    """κH = 0 with centred weights: plain -> cancelling -> plain.  The cancelling step keeps T's pattern (the fill pass stores values only, across
    two scan groups of tiles), is compacted when it is folded and drops the record: the step after it writes T in full.  Alone, and as the last
    step of a pipeline.  (tfix itself has one scan group here, 332 tiles of 1024 columns: the wide grid gives it two.)"""
    kw = dict(kap="noH", upwind=False)
    asm = assembler("mid", **kw)
    ref = {w: mg.reference(oracle, "mid", w, **kw) for w in ("plain0", "cancel", "plain1")}
    union = mg.union_nnz(ref["cancel"])
    f = {w: _fields("mid", w) for w in ref}
    asm.step_async(*f["plain0"])
    asm.finish()
    assert asm.ctx.kept_t_pattern() == -1
    assert_matrices(asm, ref["plain0"], "first plain step")
    assert asm.nnz[0] == union
    if how == "alone":
        asm.step_async(*f["cancel"])
        assert asm.ctx.kept_t_pattern() == 1
        asm.finish()
    else:
        for w in ("plain1", "plain0", "cancel"):
            asm.step_async(*f[w])
            assert asm.ctx.kept_t_pattern() == 1
        asm.finish()
    assert asm._kept_last == KEPT
    assert asm.nnz[0] < union and asm.nnz[0] == len(ref["cancel"]["T"][1])
    assert_matrices(asm, ref["cancel"], f"cancelling step, {how}")
    asm.step_async(*f["plain1"])
    assert asm._kept_last == KEPT and asm.ctx.kept_t_pattern() == 0  # (the compacted T no longer holds the pattern: written in full)
    asm.finish()
    assert asm.nnz[0] == union
    assert_matrices(asm, ref["plain1"], f"the step after the cancelling one, {how}")
    asm.step_async(*f["plain0"])
    assert asm.ctx.kept_t_pattern() == 1  # ... and kept again after it
    asm.finish()
    assert_matrices(asm, ref["plain0"], f"kept again, {how}")


# ---- mid grid: given operators ---------------------------------------------------------------------------------------------------------------------
def _given_protocols(asm, u, v, fill, foreign=False):
    """Run every protocol that accepts the given operators set on asm; after each, (its name, the host result)."""
    asm.out = None
    asm.transportmatrix(asm.facefluxes(u, v, fill))
    yield "two-phase", asm.result_to_host()
    if foreign:  # (the asynchronous calls raise GIVEN_FOREIGN: tests/test_given_ops.py)
        return
    asm.out = None
    asm.step_async(u, v, fill)
    asm.finish()
    yield "async", asm.result_to_host()
    if COUNTS_ON:
        asm.step_fused_async(u, v, fill)
        asm.finish()
        yield "fused", asm.result_to_host()


def test_mid_given_operators_derived_other_kappa_and_foreign(oracle):
    """set_given on N > 262 144 columns: (a) TκH and TκVdeep exactly as derived (state 1); (b) the same rows built with another κ (state 3: the
    fill pass reads their values); (c) a foreign TκH with one row removed from every seventh column (state 2): T is the device sparse add, the
    second scan group of otmb_spadd_plan_dev.  T against the oracle's left fold over the operands actually used."""
    asm = assembler("mid")
    N = asm.N
    rtm = mg.reference(oracle, "mid", "step0")
    other = mg.reference(oracle, "mid", "step0", kap="other")
    assert_csc_equal(_fold(oracle, rtm, N), rtm["T"], "the oracle's own fold")
    u, v, fill = _fields("mid", "step0")
    # (a)
    asm.set_given(TκH=_to_dev(asm, rtm["TκH"]), TκVdeep=_to_dev(asm, rtm["TκVdeep"]))
    for protocol, got in _given_protocols(asm, u, v, fill):
        assert (asm.ctx.given_state(2), asm.ctx.given_state(4)) == (1, 1), protocol
        assert asm.nnz[2] == 0 and asm.nnz[4] == 0
        for m in ("T", "Tadv", "TκVML"):
            assert_csc_equal(got[m], rtm[m], f"derived, {protocol}: {m}")
    # (b)
    want = _fold(oracle, {**rtm, "TκH": other["TκH"], "TκVdeep": other["TκVdeep"]}, N)
    assert_csc_equal(want, other["T"], "the same as building with those κ")
    asm.set_given(TκH=_to_dev(asm, other["TκH"]), TκVdeep=_to_dev(asm, other["TκVdeep"]))
    for protocol, got in _given_protocols(asm, u, v, fill):
        assert (asm.ctx.given_state(2), asm.ctx.given_state(4)) == (3, 3), protocol
        assert_csc_equal(got["T"], want, f"another κ, {protocol}: T")
        assert not np.array_equal(got["T"][2], rtm["T"][2])
        for m in ("Tadv", "TκVML"):
            assert_csc_equal(got[m], rtm[m], f"another κ, {protocol}: {m}")
    # (c) drop the first row of every seventh column that has at least two
    cp, rv, nz = rtm["TκH"]
    length = np.diff(cp)
    cols = np.flatnonzero(length >= 2)[::7]
    assert (cols < mg.TILE * mg.SCAN_GROUP).any() and (cols >= mg.TILE * mg.SCAN_GROUP).any()
    keep = np.ones(len(rv), bool)
    keep[cp[cols] - 1] = False
    length2 = length.copy()
    length2[cols] -= 1
    H = (np.concatenate([[1], 1 + np.cumsum(length2)]).astype(np.int64), rv[keep], nz[keep])
    want = _fold(oracle, {**rtm, "TκH": H}, N)
    assert len(want[1]) < len(rtm["T"][1])
    asm.set_given(TκH=_to_dev(asm, H), TκVdeep=None)
    for protocol, got in _given_protocols(asm, u, v, fill, foreign=True):
        assert asm.ctx.given_state(2) == 2
        assert_csc_equal(got["T"], want, "foreign TκH: T")
        for m in ("Tadv", "TκVML", "TκVdeep"):
            assert_csc_equal(got[m], rtm[m], f"foreign TκH: {m}")
    asm.set_given(TκH=None)
    asm.out = None
    asm.step(u, v, fill)
    assert_matrices(asm, rtm, "after the given operators were taken back")


# ---- mid grid: T alone and single operators ------------------------------------------------------------------------------------------------------
def test_mid_T_alone(oracle):
    """only_t: the four operators are evaluated and not materialised; T is the oracle's, in every protocol."""
    from otmb_amd.device import DeviceAssembler

    g, gm = mg.case("mid")
    asm = DeviceAssembler(0)
    asm.only_T = True
    asm.set_grid(gm, g.mlotst, g.rho, *mg.kappa("mid"))
    u, v, fill = _fields("mid", "step1")
    rtm = mg.reference(oracle, "mid", "step1")
    for protocol in PROTOCOLS:
        if protocol == "fused" and not COUNTS_ON:
            continue
        _run(asm, protocol, u, v, fill)
        assert asm.nnz[1:] == [0, 0, 0, 0], protocol
        assert_matrices(asm, rtm, f"T alone, {protocol}", mats=("T",))
    asm.only_T = False
    asm.step(u, v, fill)
    assert_matrices(asm, rtm, "all five again")


def test_mid_single_operators(oracle):
    """buildTadv / buildTκH / buildTκVML / buildTκVdeep: the fused build with every other matrix switched off (skip_ops), one at a time."""
    import otmb_amd

    g, gm = mg.case("mid")
    rtm = mg.reference(oracle, "mid", "step0")
    rphi = mg.facefluxes(oracle, "mid", "step0")
    idx = otmb_amd.makeindices(gm.v3D)
    kH, kML, kD = mg.kappa("mid")
    got = {
        "Tadv": otmb_amd.buildTadv(ϕ=rphi, gridmetrics=gm, indices=idx, ρ=g.rho),
        "TκH": otmb_amd.buildTκH(gridmetrics=gm, indices=idx, ρ=g.rho, κH=kH),
        "TκVML": otmb_amd.buildTκVML(mlotst=g.mlotst, gridmetrics=gm, indices=idx, κVML=kML),
        "TκVdeep": otmb_amd.buildTκVdeep(mlotst=g.mlotst, gridmetrics=gm, indices=idx, κVdeep=kD),
    }
    for m in OPS:
        assert_csc_equal(tuple(got[m]), rtm[m], f"mid/{m} alone")


# ---- mid grid: the general path ------------------------------------------------------------------------------------------------------------------
def test_mid_coo_generators_and_sparse_match_the_oracle(oracle):
    """sparse_entries in emission order and sparse(I, J, V, N, N) for the four operators: the one-field tile scan (tilescan_groups, tilescan_top,
    tilescan_add with nf == 1) over more than one group -- Tadv has 1.9 million triplets, eight groups of 256-entry tiles."""
    g, gm = mg.case("mid")
    idx = mg.indices(oracle, "mid")
    N, kind = idx["N"], gm.gridtopology.kind
    rphi = mg.facefluxes(oracle, "mid", "step0")
    kH, kML, kD = mg.kappa("mid")
    Om = oracle.ml_mask(gm.zt, g.mlotst, idx["Lwet"], gm.v3D.shape)
    asm = assembler("mid")
    u, v, fill = _fields("mid", "step0")
    asm.transportmatrix(asm.facefluxes(u, v, fill))
    fused = asm.result_to_host()
    want = {
        "Tadv": lambda: oracle.advection_entries(rphi, gm.v3D, g.rho, idx["Lwet"], idx["Lwet3D"], kind, True),
        "TκH": lambda: oracle.hdiff_entries(gm.v3D, gm.thkcello, gm.edge_length_2D, gm.distance_to_neighbour_2D, idx["Lwet"], idx["Lwet3D"], kind, kH),
        "TκVML": lambda: oracle.vdiff_entries(gm.v3D, gm.area2D, gm.zt, idx["Lwet"], idx["Lwet3D"], kind, kML, Om),
        "TκVdeep": lambda: oracle.vdiff_entries(gm.v3D, gm.area2D, gm.zt, idx["Lwet"], idx["Lwet3D"], kind, kD, None),
    }
    for m in OPS:
        I, J, V = asm.sparse_entries(m)
        wi, wj, wv = want[m]()
        if m == "Tadv":
            assert len(wi) > 4 * mg.SP_GROUP  # (more than four scan groups of sorted entries)
        assert np.array_equal(I.cpu().numpy(), wi) and np.array_equal(J.cpu().numpy(), wj), m  # emission order
        got_v = V.cpu().numpy()
        assert np.array_equal(got_v, wv) and np.array_equal(np.signbit(got_v), np.signbit(wv)), m
        cp, rv, nz = asm.sparse(I, J, V, N, N)
        got = (cp.cpu().numpy(), rv.cpu().numpy(), nz.cpu().numpy())
        assert_csc_equal(got, oracle.sparse(wi, wj, wv, N, N), f"mid/{m} sparse()")
        assert_csc_equal(got, fused[m], f"mid/{m} general path == fused kernel")


def test_sparse_with_runs_of_duplicates_across_a_tile_and_a_group(oracle):
    """sp_heads_kernel at its edges: a run of 300 duplicates that crosses a 256-entry tile and the first 262 144-entry scan group, a head exactly
    on a tile boundary, stored zeros (every eleventh value, and a key whose values sum to 0.0), a lone -0.0.  The placement is checked on the
    host from a stable argsort before the call."""
    import torch

    I, J, V, facts = mg.sparse_triplets()
    mg.check_sparse_triplets(I, J, V, facts)
    asm = assembler("mid")
    cp, rv, nz = asm.sparse(torch.from_numpy(I).cuda(), torch.from_numpy(J).cuda(), torch.from_numpy(V).cuda(), mg.SP_M, mg.SP_N)
    got = (cp.cpu().numpy(), rv.cpu().numpy(), nz.cpu().numpy())
    want = oracle.sparse(I, J, V, mg.SP_M, mg.SP_N)
    assert_csc_equal(got, want, "600 000 triplets")

    def value(key):
        c, r = key // mg.SP_M, key % mg.SP_M + 1
        a, b = got[0][c] - 1, got[0][c + 1] - 1
        q = a + int(np.searchsorted(got[1][a:b], r))
        assert got[1][q] == r
        return got[2][q]

    assert value(facts["zero_key"]) == 0.0 and not np.signbit(value(facts["zero_key"]))  # a stored zero is kept
    assert value(facts["neg_key"]) == 0.0 and np.signbit(value(facts["neg_key"]))        # the first touch copies


# ---- mid grid: the one-pass protocol with all scan levels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups", ["1", "0"])
def test_mid_onepass_with_all_scan_levels(oracle, monkeypatch, groups):
    """OTMB_TM_INFILL_GROUPS below the grid's two scan groups: the one-pass protocol no longer leaves the group bases to the fill pass, as on grids
    of more than 64 groups (16.7 M wet cells).  Counts from facefluxes (tilescan_groups5_packed with all levels) in the asynchronous and the
    fused step; counted by tm_count_kernel and scanned by otmb_launch_tilescan with five fields under OTMB_COUNT_IN_FF=0.  Any value of the
    switch gives the oracle's matrices."""
    monkeypatch.setenv("OTMB_TM_INFILL_GROUPS", groups)
    asm = assembler("mid")
    assert asm.ctx.tm_infill_groups() == int(groups) and asm.ctx.tm_infill() == -1
    u, v, fill = _fields("mid", "step0")
    rtm = mg.reference(oracle, "mid", "step0")
    for protocol in ("async", "fused"):
        if protocol == "fused" and not COUNTS_ON:
            continue
        asm._forget_kept()
        _run(asm, protocol, u, v, fill)
        assert asm._kept_last == ()
        assert asm.ctx.tm_infill() == 0, protocol  # (all scan levels ran)
        assert_matrices(asm, rtm, f"OTMB_TM_INFILL_GROUPS={groups}, {protocol}")
    monkeypatch.setenv("OTMB_COUNT_IN_FF", "0")
    counted = assembler("mid")
    assert not counted.count_in_ff
    counted.ctx.timing_enable(True)
    _run(counted, "async", u, v, fill)
    ran = counted.ctx.timing_collect()
    counted.ctx.timing_enable(False)
    assert "tm_count_kernel" in ran, sorted(ran)
    assert counted.ctx.tm_infill_groups() == int(groups) and counted.ctx.tm_infill() == 0
    assert_matrices(counted, rtm, f"OTMB_TM_INFILL_GROUPS={groups}, OTMB_COUNT_IN_FF=0")


def test_mid_kept_steps_with_all_scan_levels(oracle, monkeypatch):
    monkeypatch.setenv("OTMB_TM_INFILL_GROUPS", "1")
    rec = W.kept_sequence(oracle, "async")
    W.check_kept_record(rec, "async")
    assert rec["infill_groups"] == 1 and rec["infill"] == [0] * len(W.STEPS), rec


def test_mid_other_values_of_the_switch_change_nothing(oracle, monkeypatch):
    """2 covers the grid's two groups (the fill pass adds the group base, as by default); values outside 0 .. 64 are clamped: -5 is 0 (all
    levels), 1000 is 64."""
    u, v, fill = _fields("mid", "step2")
    rtm = mg.reference(oracle, "mid", "step2")
    for value, groups, infill in (("2", 2, 1), ("-5", 0, 0), ("1000", 64, 1)):
        monkeypatch.setenv("OTMB_TM_INFILL_GROUPS", value)
        asm = assembler("mid")
        assert asm.ctx.tm_infill_groups() == groups, value
        _run(asm, "async", u, v, fill)
        assert asm.ctx.tm_infill() == infill, value
        assert_matrices(asm, rtm, f"OTMB_TM_INFILL_GROUPS={value}")
        del asm
    monkeypatch.delenv("OTMB_TM_INFILL_GROUPS")
    asm = assembler("mid")
    assert asm.ctx.tm_infill_groups() == 64


# ---- wide grid -----------------------------------------------------------------------------------------------------------------------------------
def test_wide_makeindices(oracle):
    """otmb_makeindices_dev over 2080 tiles of 1024 cells: three scan groups of its one-field tile scan."""
    import torch

    idx = mg.indices(oracle, "wide")
    asm = assembler("wide")
    assert asm.G / mg.BIG_TILE > 2 * mg.SCAN_GROUP
    assert asm.N == idx["N"]
    assert np.array_equal(asm.lwet[: asm.N].cpu().numpy(), idx["Lwet"])
    assert np.array_equal(asm.lwet3d.cpu().numpy(), idx["Lwet3D"].ravel(order="F"))
    assert np.array_equal(asm.wet3d.cpu().numpy() != 0, idx["wet3D"].ravel(order="F") != 0)
    del asm
    torch.cuda.empty_cache()


def test_wide_default_steps_match_the_oracle(oracle):
    """The asynchronous and the two-phase step over five scan groups of fill tiles, facefluxes in its four-row geometry.  The context does not
    report the rows it ran with; it reports the pair kernel.  Four rows follow from the grid: ff_rows_for picks them where nx * ny >= 2^19 and
    nx >= 512 (both asserted in tests/test_mid_grids_ref.py) unless OTMB_FF_ROWS says otherwise, and a four-row grid never takes the pair
    kernel: ff_pairs() == 0."""
    import torch

    asm = assembler("wide")
    u, v, fill = _fields("wide", "base")
    rtm = mg.reference(oracle, "wide", "base")
    assert mg.scan_groups(mg.fill_tiles(asm.N)) == 5
    for protocol in ("async", "twophase"):
        asm._forget_kept()
        _run(asm, protocol, u, v, fill)
        assert asm.ctx.ff_pairs() == 0
        assert asm.ctx.tm_infill() == (1 if protocol == "async" and asm.ctx.tm_infill_groups() >= 5 else 0)
        assert_matrices(asm, rtm, f"wide/{protocol}")
        if protocol == "async":
            _assert_phi(oracle, asm, "wide", "base")
    del asm, u, v
    torch.cuda.empty_cache()


def test_wide_cancellation_is_compacted_across_two_scan_groups(oracle):
    """A cancelling step, κH = 0 and centred: tfix (1024 columns a tile) runs over two scan groups, with columns shorter than their reserved
    pattern below column 1 048 576 and above it.  Both layouts the fill pass leaves to it: the first step writes T in full (entries
    left-aligned in the reserved slots); after a plain step the same field keeps T's pattern (a cancelled slot holds its zero sum)."""
    import torch

    kw = dict(kap="noH", upwind=False)
    ref = mg.reference(oracle, "wide", "cancel", **kw)
    union = mg.union_colptr(ref)
    short = np.flatnonzero(np.diff(ref["T"][0]) < union)
    assert (short < 1048576).any() and (short >= 1048576).any()
    asm = assembler("wide", **kw)
    assert mg.scan_groups(-(-asm.N // mg.BIG_TILE)) == 2
    f = _fields("wide", "cancel")
    asm.step_async(*f)
    asm.finish()
    assert asm.nnz[0] == len(ref["T"][1]) < union.sum()
    assert_matrices(asm, ref, "wide, cancelling step written in full")
    asm.step_async(*_fields("wide", "plain0"))
    asm.finish()
    assert asm.nnz[0] == union.sum()  # (no face without flux: the whole reserved pattern)
    asm.step_async(*f)
    assert asm._kept_last == KEPT and asm.ctx.kept_t_pattern() == 1
    asm.finish()
    assert asm.nnz[0] == len(ref["T"][1])
    assert_matrices(asm, ref, "wide, cancelling step on the kept pattern")
    del asm, f
    torch.cuda.empty_cache()
