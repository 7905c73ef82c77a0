"""Every family of flux kernels on one small grid: OTMB_FF_ROWS 1 and 4 x OTMB_FF_NT 0 and 1 x Float64 and Float32 transports x the four
entries that select a family -- otmb_facefluxes_slab_dev (five wet bytes), otmb_facefluxes_flags_dev (the flag byte) and
otmb_facefluxes_counts_dev under OTMB_FF_PAIRS=0 (the one-level counting kernel on a whole grid) and =1 (facefluxes_pair_kernel) -- and,
for the three entries that have the flag byte, the fused step behind them (the ϕtop-only kernels).  Each case on a fresh context.

The grid is 70 x 9 x 5: nx above 64 and no multiple of 64 (two column blocks per row, the second partly beyond it), ny no multiple of 4
(the last four-row workgroup has three rows beyond the grid), nz = 5 (two chunks of FF_KB = 3 levels, the second partial).  Every ϕ array
equals the oracle's bit for bit, the sign of zero included; both validity words are set; after a counting entry the transportmatrix
runs no counting pass and its five matrices equal the oracle's."""
import ctypes as C

import numpy as np
import pytest

from helpers import COUNTS_ON, MATS, assert_csc_equal, gridmetrics_of

pytestmark = pytest.mark.gpu

NAMES = ("east", "west", "north", "south", "top", "bottom")
ENTRIES = ("slab", "flags", "counts", "pairs")
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _case(oracle, topology, f32):
    """Grid, metrics and the oracle's fluxes and matrices, computed once per (topology, transport type) and left unchanged."""
    key = (topology, f32)
    if key not in _cache:
        from otmb_amd import synthetic

        g = synthetic.make_grid(70, 9, 5, seed=111, rho="array", topology=topology, dtype_flux=np.float32 if f32 else np.float64)
        gm = gridmetrics_of(g)
        idx = oracle.makeindices(gm.v3D)
        fill = g.umo.properties["_FillValue"]
        rphi = oracle.facefluxes(g.umo.data, g.vmo.data, idx["wet3D"], fill, gm.gridtopology.kind)  # (Float32 transports: the same Float32 arrays)
        rtm = oracle.transportmatrix(rphi, gm, idx, g.rho, g.mlotst, g.kappaH, g.kappaVML, g.kappaVdeep, True)
        ref = [np.asfortranarray(rphi[n]).ravel(order="F") for n in NAMES]
        _cache[key] = (g, gm, fill, ref, rtm)
    return _cache[key]


def _check(oracle, monkeypatch, rows, nt, f32, entry, topology):
    import torch

    from otmb_amd import capi
    from otmb_amd.device import DeviceAssembler

    if entry in ("counts", "pairs") and not COUNTS_ON:
        pytest.skip("OTMB_COUNT_IN_FF=0: no counting kernel runs")
    g, gm, fill, ref, rtm = _case(oracle, topology, f32)
    monkeypatch.setenv("OTMB_FF_ROWS", str(rows))
    monkeypatch.setenv("OTMB_FF_NT", str(nt))
    if entry in ("counts", "pairs"):
        monkeypatch.setenv("OTMB_FF_PAIRS", "1" if entry == "pairs" else "0")
    else:
        monkeypatch.delenv("OTMB_FF_PAIRS", raising=False)
    asm = DeviceAssembler(0)
    asm.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=True)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    assert umo.element_size() == (4 if f32 else 8)
    if entry in ("counts", "pairs"):
        phi = asm.facefluxes_async(umo, vmo, fill)
    else:  # as tools/ff_ab.py calls them; arrays of ones: a cell the kernel leaves out differs from the oracle's
        phi = [torch.ones(asm.G, dtype=torch.float64, device=asm.device) for _ in range(6)]
        mask = torch.zeros(asm.G, dtype=torch.int16, device=asm.device)
        ptrs = capi.ptr_array(6, [p.data_ptr() for p in phi])
        fn, w = (asm.lib.otmb_facefluxes_flags_dev, asm.wetflags) if entry == "flags" else (asm.lib.otmb_facefluxes_slab_dev, asm.wet3d)
        asm.ctx.check(fn(asm.ctx.handle, umo.data_ptr(), vmo.data_ptr(), int(f32), w.data_ptr(), float(fill), asm.nx, asm.ny, asm.nz, asm.topology,
                         C.byref(ptrs), None, mask.data_ptr()))
    assert asm.ctx.ff_pairs() == (1 if entry == "pairs" and rows == 1 else 0)
    u, v = C.c_int32(-1), C.c_int32(-1)
    asm.ctx.check(asm.lib.otmb_facefluxes_slab_flags(asm.ctx.handle, C.byref(u), C.byref(v)))
    assert (u.value, v.value) == (1, 1)
    for f, name in enumerate(NAMES):
        got = phi[f].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(ref[f])), f"ϕ{name} differs from the oracle's at {np.flatnonzero(_bits(got) != _bits(ref[f]))[:5]}"
    if entry in ("counts", "pairs"):
        asm.ctx.timing_enable(True)
        asm.transportmatrix_onepass(phi)
        kernels = asm.ctx.timing_collect()
        asm.ctx.timing_enable(False)
        assert "tm_count_kernel" not in kernels, sorted(kernels)
        got = asm.result_to_host()
        for m in MATS:
            assert_csc_equal(got[m], rtm[m], m)
    if entry != "slab" and COUNTS_ON:  # the fused step, as tests/test_fused_step.py drives it: ϕtop only
        asm.ctx.timing_enable(True)
        asm.step_fused_async(umo, vmo, fill)
        asm.finish()
        kernels = asm.ctx.timing_collect()
        asm.ctx.timing_enable(False)
        assert "tm_count_kernel" not in kernels and "push_mask_kernel" not in kernels, sorted(kernels)
        top = asm.phi_top.cpu().numpy()
        assert np.array_equal(_bits(top), _bits(ref[4])), "the fused step's ϕtop differs from the oracle's"
        got = asm.result_to_host()
        for m in MATS:
            assert_csc_equal(got[m], rtm[m], f"fused/{m}")


CASES = [(rows, nt, f32, entry, "tripolar") for rows in (1, 4) for nt in (0, 1) for f32 in (False, True) for entry in ENTRIES]
# the same grid bipolar (no fold: the last row has no north neighbour), once per entry, over both wave geometries, stores and types
CASES += [(4, 1, False, "slab", "bipolar"), (1, 0, True, "flags", "bipolar"), (4, 0, False, "counts", "bipolar"), (1, 1, True, "pairs", "bipolar")]


@pytest.mark.parametrize("rows,nt,f32,entry,topology", CASES,
                         ids=[f"rows{r}-{'nt' if n else 'plain'}-{'f32' if f else 'f64'}-{e}-{t}" for r, n, f, e, t in CASES])
def test_every_family_equals_the_oracle(oracle, monkeypatch, rows, nt, f32, entry, topology):
    _check(oracle, monkeypatch, rows, nt, f32, entry, topology)
