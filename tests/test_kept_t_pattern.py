"""OTMB_KEPT_T_PATTERN -- T's reserved pattern (colptr, rowval) is a function of the wet mask and the topology alone: a kept step whose T arrays
still hold the pattern of the context's last clean full write stores T's values only (tm_kernel<FUSED, 12>).  Every output array must be bit for
bit what a full build writes, through exact cancellations and compactions, and every way the promise can go stale must lead to a full write of T
(run with -m gpu; the mirrors are checked without a GPU)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import COUNTS_ON, MATS
from test_kept_ops import KEPT, KEPT_BITS, _fields, _host, _pair, _run, _same

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_bit_is_mirrored():
    from otmb_amd import capi

    header = open(os.path.join(os.path.dirname(HERE), "include", "otmb.h"), encoding="utf-8").read()
    assert "#define OTMB_KEPT_T_PATTERN (1 << 5)" in header
    assert capi.KEPT_T_PATTERN == 1 << 5
    assert not capi.KEPT_T_PATTERN & (KEPT_BITS | 0b11)  # (bits 0-1 mean nothing, 2-4 are the operators)
    assert "otmb_ctx_kept_t_pattern" in capi.SYMBOLS


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_tripolar", "tiny_rho3d", "odd_nx_fold", "even_fold_open", "small_rho3d", "float32_flux"])
@pytest.mark.parametrize("upwind", [True, False])
@pytest.mark.parametrize("protocol", ["async", "pipeline", "fused", "twophase"])
def test_pattern_kept_and_full_builds_are_bit_identical(name, upwind, protocol):
    if protocol == "fused" and not COUNTS_ON:
        pytest.skip("the fused step needs the counts in facefluxes")
    g, gm, asm, full, umo, vmo, fill = _pair(name, upwind=upwind)
    taken = []
    for k, (u, v) in enumerate(_fields(umo, vmo, 5, seed=len(name) + 7)):
        _run(asm, protocol, u, v, fill)
        _run(full, protocol, u, v, fill)
        assert asm.nnz == full.nnz, f"step {k}"
        _same(_host(asm), _host(full), f"step {k}")
        taken.append(asm.ctx.kept_t_pattern())
        if protocol != "twophase":
            assert taken[-1] == 1 or k == 0, f"step {k}: {taken}"  # (every step after the first clean fold)
        elif asm._kept_last == KEPT:
            assert taken[-1] == 1, f"step {k}: {taken}"
    assert full.ctx.kept_t_pattern() == -1
    assert taken.count(1) >= (1 if protocol == "twophase" else 4)


def _union_nnz(h):
    """Entries of the union pattern of the four operators (T's reserved pattern) from host CSC arrays."""
    keys = []
    for m in MATS[1:]:
        cp, rv, _ = h[m]
        cols = np.repeat(np.arange(len(cp) - 1, dtype=np.int64), np.diff(cp))
        keys.append(cols * (1 << 32) + rv)
    return len(np.unique(np.concatenate(keys)))


def _cancel_fields(umo, vmo, n, cancel, seed=0):
    """n (umo, vmo) pairs of non-zero transports (no exact zero on any face: with κH = 0 and centred weights T then keeps every reserved row);
    step k in `cancel` zeroes every fifth transport (faces without flux: T's horizontal rows there are 0.0 + TκH's explicit zero, they cancel)."""
    import torch

    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        pair = []
        for x in (umo, vmo):
            f = rng.uniform(0.5, 1.5, x.numel()) * rng.choice([-1.0, 1.0], x.numel())
            if k in cancel:
                f[::5] = 0.0
            pair.append(torch.from_numpy(f).to(x.device, x.dtype).contiguous())
        out.append(tuple(pair))
    return out


@pytest.mark.gpu
def test_cancellation_superseded_compacted_and_rewritten():
    """κH = 0 with centred weights: fields alternate between steps whose T keeps its whole reserved pattern and steps with exact cancellations.
    (1) a cancelling pattern-kept step alone: compacted at its fold, the record dropped, the next step writes T in full; (2) a cancelling step
    superseded in a pipeline by a pattern-kept one: not compacted, the record stays; (3) a cancelling pattern-kept LAST step of a pipeline:
    compacted at the fold.  Every step against a full build, nnz and per-step results included."""
    from helpers import make_case

    g0, _ = make_case("small_rho3d")
    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d", kappa=(0.0, g0.kappaVML, g0.kappaVdeep), upwind=False)
    # phases: lists of (field index) enqueued before one finish()
    phases = [[0], [1], [2], [3], [4], [5, 6], [7], [8, 9], [10], [11]]
    cancel = {2, 5, 9}
    fields = _cancel_fields(umo, vmo, 12, cancel, seed=42)
    expect = {0: -1, 1: 1, 2: 1, 3: 0, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 1, 10: 0, 11: 1}
    for ph in phases:
        for k in ph:
            for a in (asm, full):
                a.step_async(*fields[k], fill)
            assert asm.ctx.kept_t_pattern() == expect[k], f"step {k}"
        for a in (asm, full):
            a.finish()
        for q in range(len(ph)):
            assert asm.result_step(q) == full.result_step(q), f"phase {ph}, step {q}"
        h, hf = _host(asm), _host(full)
        assert asm.nnz == full.nnz, f"phase {ph}"
        _same(h, hf, f"phase {ph}")
        cancelled = hf["T"][1].size < _union_nnz(hf)
        assert cancelled == (ph[-1] in cancel), f"phase {ph}: the fields do not do what the test needs"


def _raw_step(asm, kept_ops, out=None):
    """otmb_transportmatrix_dev through the C ABI with the given kept_ops (out: an output set, default asm.out), then its result."""
    out = asm.out if out is None else out
    phi = asm.facefluxes(*asm._raw_fields)
    a = asm._args(phi)
    a.kept_ops = kept_ops
    cp, rv, nz = asm._out_ptrs(out)
    caps = (C.c_int64 * 5)(*[asm.N * k + 1 for k in asm.PER_COLUMN_MAX])
    asm.ctx.check(asm.lib.otmb_transportmatrix_dev(asm.ctx.handle, C.byref(a), C.byref(cp), C.byref(rv), C.byref(nz), C.byref(caps)))
    nnz = (C.c_int64 * 5)()
    asm.ctx.check(asm.lib.otmb_transportmatrix_result(asm.ctx.handle, C.byref(nnz)))
    asm.nnz = [int(x) for x in nnz]


def _poison_t_rows(asm, out=None):
    """Overwrite T's rowval through the library (a stream over it): torch does not see it."""
    out = asm.out if out is None else out
    rv = out["T"][1]
    asm.ctx.stream_mix([(asm.v3d.data_ptr(), 8 * asm.v3d.numel())], [(rv.data_ptr(), 8 * rv.numel())], 8)
    asm.ctx.synchronize()


@pytest.mark.gpu
def test_poisoned_rows_stay_with_the_bit_and_are_repaired_without_it():
    from otmb_amd import capi

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    _run(full, "async", umo, vmo, fill)
    ref = _host(full)
    asm._raw_fields = (umo, vmo, fill)
    asm.out = asm.new_output_set()
    asm._out_cap = [asm.N * k + 1 for k in asm.PER_COLUMN_MAX]
    _raw_step(asm, KEPT_BITS | capi.KEPT_T_PATTERN)  # no record at all on this context
    assert asm.ctx.kept_t_pattern() == -1
    _same(_host(asm), ref, "no record")
    _raw_step(asm, KEPT_BITS | capi.KEPT_T_PATTERN)
    assert asm.ctx.kept_t_pattern() == 1
    _same(_host(asm), ref, "pattern kept")
    _poison_t_rows(asm)
    _raw_step(asm, KEPT_BITS | capi.KEPT_T_PATTERN)  # the record matches: the poison stays (the control)
    assert asm.ctx.kept_t_pattern() == 1
    got = _host(asm)
    assert not np.array_equal(got["T"][1], ref["T"][1])
    assert np.array_equal(got["T"][2].view(np.int64), ref["T"][2].view(np.int64))  # (the values are written)
    _raw_step(asm, KEPT_BITS)  # a call without the bit repairs it
    assert asm.ctx.kept_t_pattern() == 0
    _same(_host(asm), ref, "repaired")
    # through the assembler: its first step promises nothing, the second one T's pattern too
    _run(asm, "async", umo, vmo, fill)
    _run(asm, "async", umo, vmo, fill)
    assert asm._kept_last == KEPT and asm._tpat_last and asm.ctx.kept_t_pattern() == 1
    # a torch-visible write to T's rowval: the assembler drops the promise
    _poison_t_rows(asm)
    asm.out["T"][1][0] += 0
    _run(asm, "async", umo, vmo, fill)
    assert asm._kept_last == KEPT and not asm._tpat_last and asm.ctx.kept_t_pattern() == 0
    _same(_host(asm), ref, "torch edit")
    _run(asm, "async", umo, vmo, fill)
    assert asm._tpat_last and asm.ctx.kept_t_pattern() == 1
    _same(_host(asm), ref, "kept again")


@pytest.mark.gpu
def test_the_record_follows_its_arrays():
    """Two output sets alternating; then T arrays the record does not name beside the kept operators' arrays it does: T is written in full."""
    import torch

    from otmb_amd import capi

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_tripolar")
    fields = _fields(umo, vmo, 6, seed=9)
    sets = [asm.new_output_set(), asm.new_output_set()]
    for k, (u, v) in enumerate(fields[:4]):
        o = sets[k % 2]
        asm.transportmatrix_onepass(asm.facefluxes(u, v, fill), out=o)
        _run(full, "async", u, v, fill)
        assert asm.ctx.kept_t_pattern() == -1  # (no step kept: the records name the other set)
        _same(_host(asm, o), _host(full), f"set {k % 2}, step {k}")
    # the record names sets[1]: poison sets[0]'s T rows, a raw call with every bit into sets[0] writes in full
    asm._raw_fields = (*fields[4], fill)
    _run(full, "async", *fields[4], fill)
    _poison_t_rows(asm, sets[0])
    _raw_step(asm, KEPT_BITS | capi.KEPT_T_PATTERN, out=sets[0])
    _same(_host(asm, sets[0]), _host(full), "other set")
    # the kept operators' arrays match, T's are new (garbage): the operators are kept, T is written in full
    _raw_step(asm, KEPT_BITS | capi.KEPT_T_PATTERN, out=sets[0])
    assert asm.ctx.kept_t_pattern() == 1
    mixed = dict(sets[0])
    mixed["T"] = tuple(torch.full_like(t, 7) for t in sets[0]["T"])
    _raw_step(asm, KEPT_BITS | capi.KEPT_T_PATTERN, out=mixed)
    assert asm.ctx.kept_t_pattern() == 0
    _same(_host(asm, mixed), _host(full), "new T arrays")


@pytest.mark.gpu
def test_written_bytes_of_a_pattern_kept_step():
    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    for u, v in _fields(umo, vmo, 3, seed=4):
        _run(asm, "async", u, v, fill)
    assert asm.ctx.kept_t_pattern() == 1
    nT, nA = asm.nnz[0], asm.nnz[1]
    assert asm.algorithmic_bytes_split()[1] == 16 * nA + 8 * (asm.N + 1) + 8 * nT
    asm._forget_kept()  # (the next step writes everything: so does the accounting)
    assert asm.algorithmic_bytes_split()[1] == sum(16 * z + 8 * (asm.N + 1) for z in asm.nnz)


_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.path.dirname({here!r}))
sys.path.insert(0, {here!r})
from test_kept_ops import _fields, _pair, _run
import kept_htab_worker as W
g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
rec = []
for u, v in _fields(umo, vmo, 3, seed=21):
    _run(asm, "async", u, v, fill)
    rec.append(W.digest(asm))
json.dump({{"digests": rec, "tpat": asm.ctx.kept_t_pattern(), "htab": asm.ctx.kept_htab()}}, open(sys.argv[1], "w"))
"""


@pytest.mark.gpu
def test_switch_off_is_the_same_result(tmp_path):
    """OTMB_KEPT_TPAT=0 (read once per process: a child) writes T in full on every step, with the same outputs."""
    import kept_htab_worker as W

    out = str(tmp_path / "off.json")
    env = dict(os.environ, OTMB_KEPT_TPAT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(here=HERE), out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    off = json.load(open(out))
    g, gm, asm, full, umo, vmo, fill = _pair("small_rho3d")
    got = []
    for u, v in _fields(umo, vmo, 3, seed=21):
        _run(asm, "async", u, v, fill)
        got.append(W.digest(asm))
    assert got == off["digests"]
    assert asm.ctx.kept_t_pattern() == 1 and off["tpat"] == 0 and off["htab"] == 1


@pytest.mark.gpu
def test_one_degree_pattern_kept_steps_equal_a_full_build():
    """The headline grid (bench.py access1deg): the third step stores T's values only; all five outputs as a full build's."""
    import torch

    import kept_htab_worker as W
    import otmb_amd
    from otmb_amd import synthetic
    from otmb_amd.device import DeviceAssembler

    nx, ny, nz, lf = synthetic.PRESETS["access1deg"]
    g = synthetic.make_grid(nx, ny, nz, seed=20260501, land_fraction=lf, rho="array")
    gm = otmb_amd.makegridmetrics(areacello=g.areacello, volcello=g.volcello, lon=g.lon, lat=g.lat, lev=g.lev,
                                  lon_vertices=g.lon_vertices, lat_vertices=g.lat_vertices)
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    fill = g.umo.properties["_FillValue"]
    digests = []
    for promise in (True, False):
        a = DeviceAssembler(0)
        a.set_grid(gm, g.mlotst, g.rho, g.kappaH, g.kappaVML, g.kappaVdeep, upwind=True)
        if not promise:
            a._kept_ops = lambda out: (0, ())
        for _ in range(3):
            a.step_async(umo, vmo, fill)
            a.finish()
        assert a.ctx.kept_t_pattern() == (1 if promise else -1)
        digests.append(W.digest(a))
        del a
        torch.cuda.empty_cache()
    assert digests[0] == digests[1]
