"""The counting flux kernels on grids of 63 to 130 levels.  A wave of facefluxes_kernel<COUNTS> (one-row and four-row geometry) and of
facefluxes_pair_kernel keeps its per-level tables -- the wet-rank bases of its segment and zt -- in registers, lane l holding level l in one
register and level 64 + l in a second one (FFC_MAX_NZ = 128); beyond 128 levels the host falls back to the plain kernel and a counting pass
and otmb_step_dev refuses.  The grids are those of tests/deep_grids.py (water, tile boundaries, both flux signs and the edge of the mixed
layer on levels 62 ... 65 and up to the last one: tests/test_deep_grids_ref.py asserts that on the CPU); every case runs on a fresh
context and is compared with the oracle bit for bit: the six ϕ arrays, the five matrices of the two-call path -- which must not count for
itself -- and ϕtop and the five matrices of the fused step."""
import ctypes as C

import numpy as np
import pytest

import deep_grids as dg
from helpers import COUNTS_ON, MATS, assert_csc_equal

pytestmark = pytest.mark.gpu

NAMES = ("east", "west", "north", "south", "top", "bottom")
# entry: (OTMB_FF_ROWS, OTMB_FF_PAIRS)
GEOMS = {"rows1": (1, 0), "rows4": (4, 0), "pairs": (1, 1)}
_phi, _tm, _dirty = {}, {}, {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _id(shape):
    return "x".join(map(str, shape))


def _grid(shape, topology, f32, dirty):
    """The case's grid; dirty: NaN and fill values scattered into the wet transports of levels >= 60 (a copy, made once)."""
    g, gm = dg.case(shape, topology, f32)
    if not dirty:
        return g, gm
    key = (shape, topology, f32)
    if key not in _dirty:
        from otmb_amd._nt import NT, Cube

        rng = np.random.default_rng(3)
        fill = g.umo.properties["_FillValue"]
        new = {}
        for name in ("umo", "vmo"):
            a = np.array(getattr(g, name).data, order="F")
            cells = np.argwhere(a[:, :, 60:] != fill)
            for q, val in ((cells[rng.choice(len(cells), 40, replace=False)], np.nan), (cells[rng.choice(len(cells), 40, replace=False)], fill)):
                a[q[:, 0], q[:, 1], q[:, 2] + 60] = val
            new[name] = Cube(a, _FillValue=fill)
        _dirty[key] = NT(g, **new)
    return _dirty[key], gm


def _mixed_layer(g, ml):
    return dg.ml_whole_column(g) if ml == "whole" else dg.ml_edge(g, *ml)


def _reference(oracle, shape, topology="tripolar", f32=False, upwind=True, ml=(60, 67), dirty=False):
    """(grid, gridmetrics, mlotst, fill, the oracle's six fluxes, its five matrices): computed once per case and left unchanged."""
    g, gm = _grid(shape, topology, f32, dirty)
    kp = (shape, topology, f32, dirty)
    fill = g.umo.properties["_FillValue"]
    if kp not in _phi:
        idx = oracle.makeindices(gm.v3D)
        _phi[kp] = (idx, oracle.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], fill, gm.gridtopology.kind))  # (Float32: the same Float32 arrays)
    idx, rphi = _phi[kp]
    kt = kp + (upwind, ml)
    mlotst = _mixed_layer(g, ml)
    if kt not in _tm:
        _tm[kt] = oracle.transportmatrix(rphi, gm, idx, g.rho, mlotst, g.kappaH, g.kappaVML, g.kappaVdeep, upwind)
    return g, gm, mlotst, fill, [np.asfortranarray(rphi[n]).ravel(order="F") for n in NAMES], _tm[kt]


def _assembler(monkeypatch, g, gm, mlotst, rows, pairs, upwind=True, only_T=False, nt=None):
    """A fresh context under the geometry's switches, the grid and the transports on the device."""
    import torch

    from otmb_amd.device import DeviceAssembler

    for name, val in (("OTMB_FF_ROWS", rows), ("OTMB_FF_PAIRS", pairs), ("OTMB_FF_NT", nt)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(val))
    asm = DeviceAssembler(0)
    asm.only_T = only_T
    asm.set_grid(gm, mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=upwind)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    return asm, umo, vmo


def _assert_phi(phi, ref):
    for f, name in enumerate(NAMES):
        got = phi[f].cpu().numpy()
        diff = np.flatnonzero(_bits(got) != _bits(ref[f]))
        assert diff.size == 0, f"ϕ{name} differs from the oracle's at {diff[:5]} (of {diff.size}): {got[diff[:5]]} vs {ref[f][diff[:5]]}"


def _assert_mats(asm, rtm, only_T, what=""):
    got = asm.result_to_host()
    for m in (("T",) if only_T else MATS):
        assert_csc_equal(got[m], rtm[m], what + m)
    if only_T:
        assert asm.nnz[1:] == [0, 0, 0, 0]


def _two_calls(asm, umo, vmo, fill):
    """facefluxes_async + transportmatrix_onepass: (ϕ, the kernels the transportmatrix launched)."""
    phi = asm.facefluxes_async(umo, vmo, fill)
    pairs = asm.ctx.ff_pairs()
    u, v = C.c_int32(-1), C.c_int32(-1)
    asm.ctx.check(asm.lib.otmb_facefluxes_slab_flags(asm.ctx.handle, C.byref(u), C.byref(v)))
    assert (u.value, v.value) == (1, 1)
    asm.ctx.timing_enable(True)
    asm.transportmatrix_onepass(phi)
    kernels = asm.ctx.timing_collect()
    asm.ctx.timing_enable(False)
    return phi, pairs, kernels


def _check(oracle, monkeypatch, geom, shape, topology="tripolar", f32=False, upwind=True, ml=(60, 67), dirty=False, only_T=False, nt=None):
    if not COUNTS_ON:
        pytest.skip("OTMB_COUNT_IN_FF=0: no counting kernel runs")
    rows, pairs = GEOMS[geom]
    g, gm, mlotst, fill, ref, rtm = _reference(oracle, shape, topology, f32, upwind, ml, dirty)
    asm, umo, vmo = _assembler(monkeypatch, g, gm, mlotst, rows, pairs, upwind=upwind, only_T=only_T, nt=nt)
    assert umo.element_size() == (4 if f32 else 8)
    phi, ran, kernels = _two_calls(asm, umo, vmo, fill)
    assert ran == (1 if geom == "pairs" else 0)
    _assert_phi(phi, ref)
    assert "tm_count_kernel" not in kernels and "push_mask_kernel" not in kernels, sorted(kernels)
    _assert_mats(asm, rtm, only_T)
    # the fused step: ϕtop only, the other five fluxes re-derived in the fill pass
    asm.ctx.timing_enable(True)
    asm.step_fused_async(umo, vmo, fill)
    asm.finish()
    kernels = asm.ctx.timing_collect()
    asm.ctx.timing_enable(False)
    assert "tm_count_kernel" not in kernels and "push_mask_kernel" not in kernels, sorted(kernels)
    assert asm.ctx.ff_pairs() == (1 if geom == "pairs" else 0)
    top = asm.phi_top.cpu().numpy()
    assert np.array_equal(_bits(top), _bits(ref[4])), "the fused step's ϕtop differs from the oracle's"
    _assert_mats(asm, rtm, only_T, "fused/")
    return rtm


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("shape", dg.SHAPES, ids=_id)
def test_shapes_around_the_register_boundary_and_the_limit(oracle, monkeypatch, shape, geom):
    """Upwind weighting, the edge of the mixed layer cycling over levels 60 ... 67 (clipped to the grid)."""
    _check(oracle, monkeypatch, geom, shape)


# every option once per geometry, alternating between the two shapes (not the full cross product)
OPTIONS = {"centred": dict(upwind=False), "f32": dict(f32=True), "bipolar": dict(topology="bipolar"), "only_T": dict(only_T=True),
           "plain_stores": dict(nt=0)}
OPTION_CASES = [(opt, geom, dg.OPTION_SHAPES[(a + b) % 2]) for a, opt in enumerate(OPTIONS) for b, geom in enumerate(GEOMS)]


@pytest.mark.parametrize("opt,geom,shape", OPTION_CASES, ids=[f"{o}-{g}-{_id(s)}" for o, g, s in OPTION_CASES])
def test_options_on_66_and_128_levels(oracle, monkeypatch, opt, geom, shape):
    _check(oracle, monkeypatch, geom, shape, **OPTIONS[opt])


@pytest.mark.parametrize("geom", list(GEOMS))
def test_nan_and_fill_values_in_the_transports_of_the_deep_levels(oracle, monkeypatch, geom):
    _check(oracle, monkeypatch, geom, (33, 6, 65), dirty=True)


@pytest.mark.parametrize("upwind", [True, False], ids=["upwind", "centred"])
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("ml", [(62, 62), (63, 63), "whole"], ids=["edge_below_63", "edge_below_64", "whole_column"])
def test_mixed_layer_ends_at_the_register_boundary(oracle, monkeypatch, ml, geom, upwind):
    """The edge of the mixed layer just below level 63 (the last level of the lower registers is the first unmixed one), just below level
    64 (the window's three levels lie on both sides), and no edge at all (+inf: every level of the upper registers is mixed)."""
    rtm = _check(oracle, monkeypatch, geom, (36, 10, 66), upwind=upwind, ml=ml)
    assert len(rtm["TκVML"][1]) > 0


@pytest.mark.parametrize("pairs", [1, None], ids=["pairs_asked_for", "pairs_unset"])
@pytest.mark.parametrize("shape", dg.BEYOND, ids=_id)
def test_past_the_limit_the_plain_kernel_and_a_counting_pass(oracle, monkeypatch, shape, pairs):
    """129 and 130 levels: facefluxes takes the plain kernel whatever OTMB_FF_PAIRS says, the transportmatrix counts for itself, the fused
    step is refused -- and leaves the assembler as it was: the two-call path gives the oracle's matrices again, no counts key left behind."""
    from otmb_amd.capi import OtmbError

    g, gm, mlotst, fill, ref, rtm = _reference(oracle, shape)
    asm, umo, vmo = _assembler(monkeypatch, g, gm, mlotst, None, pairs)
    for attempt in range(2):
        phi, ran, kernels = _two_calls(asm, umo, vmo, fill)
        assert ran == 0
        _assert_phi(phi, ref)
        assert kernels.get("tm_count_kernel", (0, 0))[1] > 0, sorted(kernels)
        _assert_mats(asm, rtm, False, f"call {attempt}/")
        if attempt == 0:
            with pytest.raises(OtmbError) as e:
                asm.step_fused_async(umo, vmo, fill)
            assert e.value.name == "INVALID_ARG"
            assert asm.lib.otmb_facefluxes_counts_pending(asm.ctx.handle) == 0
