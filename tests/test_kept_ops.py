"""otmb_tm_args.kept_ops -- TκH, TκVML and TκVdeep depend on the grid, κ and mlotst alone (src/matrixbuilding.jl:51-120): a step whose output set
still holds what the library last wrote there stores T and Tadv only.  Every output array must be bit for bit what a full build writes, and every
way the promise can go stale must lead to a full write (run with -m gpu; the struct mirrors are checked without a GPU)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from helpers import COUNTS_ON, MATS, assert_csc_equal, make_case

ROOT = Path(__file__).resolve().parents[1]
KEPT = ("TκH", "TκVML", "TκVdeep")
KEPT_BITS = sum(1 << MATS.index(m) for m in KEPT)


def test_kept_ops_is_the_last_field_of_every_mirror():
    from otmb_amd import capi

    header = (ROOT / "include" / "otmb.h").read_text()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} otmb_tm_args;", header, re.S).group(1)
    decls = re.findall(r"^\s*[a-z_0-9 ]+?\**\s*\**(\w+)(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S), re.M)
    assert decls[-1] == "kept_ops"
    assert capi.TmArgs._fields_[-1] == ("kept_ops", C.c_int32)
    shim = (ROOT / "julia" / "OceanTransportMatrixBuilderAMD.jl").read_text()
    jbody = re.search(r"struct TmArgs\n(.*?)\nend", shim, re.S).group(1)
    assert jbody.strip().splitlines()[-1].split("#")[0].strip() == "kept_ops::Int32"
    # the Julia constructor call passes one argument per field: the host path never promises anything
    assert "skip_ops, csc, Int32(0))" in shim
    a = capi.TmArgs()
    assert a.kept_ops == 0  # (a zero-initialised struct is today's behaviour, as in examples/otmb_c_example.c)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------


def _pair(name, kappa=None, upwind=True):
    """Two assemblers on the same grid: one that promises (the default), one that never does."""
    import torch

    from otmb_amd.device import DeviceAssembler

    g, gm = make_case(name)
    kap = kappa or (g.kappaH, g.kappaVML, g.kappaVdeep)
    asms = []
    for _ in range(2):
        a = DeviceAssembler(0)
        a.set_grid(gm, g.mlotst, g.rho, *kap, upwind=upwind)
        asms.append(a)
    asms[1]._kept_ops = lambda out: (0, ())
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    return g, gm, asms[0], asms[1], umo, vmo, g.umo.properties["_FillValue"]


def _fields(umo, vmo, n, seed=0):
    """n (umo, vmo) pairs whose signs and sizes change from step to step (other Tadv patterns), NaN land kept NaN."""
    import torch

    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        fu = torch.from_numpy(rng.uniform(-1.5, 1.5, umo.numel())).to(umo.device, umo.dtype)
        fv = torch.from_numpy(rng.uniform(-1.5, 1.5, vmo.numel())).to(vmo.device, vmo.dtype)
        if k % 3 == 2:
            fu[::5] = 0.0
        out.append(((umo * fu).contiguous(), (vmo * fv).contiguous()))
    return out


def _host(asm, out=None):
    asm.ctx.synchronize()
    out = asm.out if out is None else out
    return {m: (out[m][0].cpu().numpy(), out[m][1][: asm.nnz[k]].cpu().numpy(), out[m][2][: asm.nnz[k]].cpu().numpy())
            for k, m in enumerate(MATS)}


def _same(a, b, where):
    assert set(a) == set(b)
    for m in a:
        assert_csc_equal(a[m], b[m], f"{where} {m}")


def _run(asm, protocol, u, v, fill):
    if protocol == "async":
        asm.step_async(u, v, fill)
        asm.finish()
    elif protocol == "pipeline":  # several steps in flight before one result: only the last one's matrices are compared
        for _ in range(3):
            asm.step_async(u, v, fill)
        asm.finish()
    elif protocol == "fused":
        asm.step_fused_async(u, v, fill)
        asm.finish()
    else:
        asm.step(u, v, fill, onepass=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_tripolar", "tiny_rho3d", "odd_nx_fold", "even_fold_open", "small_rho3d", "float32_flux"])
@pytest.mark.parametrize("upwind", [True, False])
@pytest.mark.parametrize("protocol", ["async", "pipeline", "fused", "twophase"])
def test_kept_and_full_builds_are_bit_identical(name, upwind, protocol):
    if protocol == "fused" and not COUNTS_ON:
        pytest.skip("the fused step needs the counts in facefluxes")
    g, gm, asm, full, umo, vmo, fill = _pair(name, upwind=upwind)
    kept_steps = 0
    for k, (u, v) in enumerate(_fields(umo, vmo, 5, seed=len(name))):
        _run(asm, protocol, u, v, fill)
        _run(full, protocol, u, v, fill)
        kept_steps += asm._kept_last == KEPT
        assert asm.nnz == full.nnz, f"step {k}"
        _same(_host(asm), _host(full), f"step {k}")
        assert asm.algorithmic_bytes_split()[1] <= full.algorithmic_bytes_split()[1]
    # every step after the first kept the three operators (two-phase: unless T / Tadv outgrew the arrays, which are then allocated anew)
    assert kept_steps >= (1 if protocol == "twophase" else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("protocol", ["async", "twophase"])
def test_kept_steps_with_T_cancellation(protocol):
    """κ = 0: every diffusive value is an explicit 0.0, T drops them (the kernel's compaction) while the operators keep them."""
    g, gm, asm, full, umo, vmo, fill = _pair("tiny_tripolar", kappa=(0.0, 0.0, 0.0))
    for k, (u, v) in enumerate(_fields(umo, vmo, 4, seed=3)):
        _run(asm, protocol, u, v, fill)
        _run(full, protocol, u, v, fill)
        assert asm.nnz == full.nnz and asm.nnz[0] < sum(asm.nnz[1:]), f"step {k}"
        _same(_host(asm), _host(full), f"step {k}")
    assert asm._kept_last == KEPT


@pytest.mark.gpu
def test_kept_steps_with_a_scalar_rho():
    import torch

    from otmb_amd.device import DeviceAssembler

    g, gm = make_case("tiny_tripolar")
    asms = []
    for _ in range(2):
        a = DeviceAssembler(0)
        a.set_grid(gm, g.mlotst, 1025.0, g.kappaH, g.kappaVML, g.kappaVdeep)
        asms.append(a)
    asms[1]._kept_ops = lambda out: (0, ())
    umo = torch.from_numpy(np.asfortranarray(g.umo.data).ravel(order="F")).cuda()
    vmo = torch.from_numpy(np.asfortranarray(g.vmo.data).ravel(order="F")).cuda()
    for k, (u, v) in enumerate(_fields(umo, vmo, 3)):
        for a in asms:
            _run(a, "async", u, v, 1e20)
        _same(_host(asms[0]), _host(asms[1]), f"step {k}")
    assert asms[0]._kept_last == KEPT


def _poison(asm, out=None):
    """Overwrite the three kept operators through the library (a stream over their arrays): torch does not see it."""
    out = asm.out if out is None else out
    arrs = [t for m in KEPT for t in out[m]]
    asm.ctx.stream_mix([(asm.v3d.data_ptr(), 8 * asm.v3d.numel())], [(t.data_ptr(), t.element_size() * t.numel()) for t in arrs], 8)
    asm.ctx.synchronize()


@pytest.mark.gpu
def test_the_poison_is_seen_by_a_kept_step():
    """The control of the tests below: a write the assembler is not told about is NOT repaired by a step with the promise (the contract:
    such a write must be followed by a call without it)."""
    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    for a in (asm, full):
        _run(a, "async", umo, vmo, fill)
    ref = _host(full)
    _poison(asm)
    _run(asm, "async", umo, vmo, fill)
    assert asm._kept_last == KEPT
    got = _host(asm)
    _same({m: got[m] for m in ("T", "Tadv")}, {m: ref[m] for m in ("T", "Tadv")}, "T / Tadv")
    assert not all(np.array_equal(got[m][2], ref[m][2]) for m in KEPT)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["torch_edit", "kappa", "given_on_off", "second_output_set", "stream_mix", "failed_step"])
def test_every_invalidation_rewrites_the_operators(how):
    import torch

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    fields = _fields(umo, vmo, 2, seed=11)
    for a in (asm, full):
        _run(a, "async", *fields[0], fill)
    _run(asm, "async", *fields[0], fill)  # (a kept step: the promise is live before the invalidation)
    assert asm._kept_last == KEPT
    _poison(asm)
    if how == "torch_edit":
        asm.out["TκH"][2][2] += 1.0  # (on top of the poison: torch sees this one)
    elif how == "kappa":
        kap = (2.0 * g.kappaH, g.kappaVML, g.kappaVdeep)
        for a in (asm, full):
            a.set_grid(gm, g.mlotst, g.rho, *kap)
        _run(full, "async", *fields[1], fill)
    elif how == "given_on_off":  # bench.py's given_steps sequence
        ops = {m: (full.out[m][0].clone(), full.out[m][1][: full.nnz[MATS.index(m)]].clone(), full.out[m][2][: full.nnz[MATS.index(m)]].clone())
               for m in ("TκH", "TκVdeep")}
        asm.set_given(**ops)
        _run(asm, "async", *fields[1], fill)
        _poison(asm)
        asm.set_given(TκH=None, TκVdeep=None)
    elif how == "second_output_set":
        other = asm.new_output_set()
        asm.transportmatrix_onepass(asm.facefluxes(*fields[1], fill), out=other)
        _poison(asm)  # (the first set: the library's record now names the second)
    elif how == "stream_mix":
        asm.fill_pass_stream_mix()
    elif how == "failed_step":
        from otmb_amd.capi import OtmbError

        L = int(asm.lwet[0].item()) - 1
        saved = asm.rho[L].item()
        asm.rho[L] = float("nan")
        with pytest.raises(OtmbError, match="ρ contains NaNs"):
            _run(asm, "async", *fields[1], fill)
        asm.rho[L] = saved
        _poison(asm)
    if how != "kappa":
        _run(full, "async", *fields[1], fill)
    _run(asm, "async", *fields[1], fill)
    assert asm._kept_last == ()
    assert asm.nnz == full.nnz
    _same(_host(asm), _host(full), how)
    # ... and the step after it may keep again
    _run(asm, "async", *fields[1], fill)
    assert asm._kept_last == KEPT
    _same(_host(asm), _host(full), how + ", kept again")


@pytest.mark.gpu
def test_a_pipeline_step_that_fails_after_a_kept_one_is_reported_as_before():
    """A NaN ρ in step 2 of 4 (stream-ordered edit): step 2 fails with its own error, steps 3 and 4 -- which kept the operators step 1 wrote --
    are fine, as they are in a full build."""
    from otmb_amd.capi import OtmbError

    g, gm, asm, full, umo, vmo, fill = _pair("tiny_rho3d")
    L = int(asm.lwet[0].item()) - 1
    for a in (asm, full):
        saved = a.rho[L].item()
        with pytest.raises(OtmbError, match="ρ contains NaNs") as e:
            for s in range(4):
                a.rho[L] = float("nan") if s == 1 else saved
                a.step_async(umo, vmo, fill)
            a.finish()
        assert e.value.step == 1
        a.rho[L] = saved
    for k in range(4):
        rk, nk = asm.result_step(k)
        rf, nf = full.result_step(k)
        assert (rk, nk) == (rf, nf), f"step {k}"


def _raw_step(asm, kept_ops):
    """otmb_transportmatrix_dev through the C ABI, into asm.out, with the given kept_ops."""
    phi = asm.facefluxes(*asm._raw_fields)
    a = asm._args(phi)
    a.kept_ops = kept_ops
    cp, rv, nz = asm._out_ptrs(asm.out)
    caps = (C.c_int64 * 5)(*[asm.N * k + 1 for k in asm.PER_COLUMN_MAX])
    asm.ctx.check(asm.lib.otmb_transportmatrix_dev(asm.ctx.handle, C.byref(a), C.byref(cp), C.byref(rv), C.byref(nz), C.byref(caps)))
    nnz = (C.c_int64 * 5)()
    asm.ctx.check(asm.lib.otmb_transportmatrix_result(asm.ctx.handle, C.byref(nnz)))
    asm.nnz = [int(x) for x in nnz]


@pytest.mark.gpu
def test_raw_abi_kept_bits_without_a_matching_record_write_in_full():
    g, gm, asm, full, umo, vmo, fill = _pair("tiny_tripolar")
    _run(full, "async", umo, vmo, fill)
    ref = _host(full)
    asm._raw_fields = (umo, vmo, fill)
    asm.out = asm.new_output_set()
    asm._out_cap = [asm.N * k + 1 for k in asm.PER_COLUMN_MAX]
    _poison(asm)
    _raw_step(asm, KEPT_BITS)  # no record at all on this context
    _same(_host(asm), ref, "no record")
    _poison(asm)
    _raw_step(asm, KEPT_BITS)  # the record matches: the poison stays (the control)
    assert not all(np.array_equal(_host(asm)[m][2], ref[m][2]) for m in KEPT)
    _raw_step(asm, 0)  # a call without the promise repairs it
    _same(_host(asm), ref, "repaired")
    _poison(asm)
    asm.ctx.forget_given()  # what a re-upload of a grid array does
    _raw_step(asm, KEPT_BITS)
    _same(_host(asm), ref, "after forget_given")
    # bits for T / Tadv mean nothing
    _poison(asm)
    asm.out["T"][2].fill_(0.0)
    asm.ctx.synchronize()
    _raw_step(asm, 0b11)
    _same(_host(asm), ref, "bits 0-1")


@pytest.mark.gpu
def test_raw_abi_kept_bit_with_other_kappa_writes_in_full():
    g, gm, asm, full, umo, vmo, fill = _pair("tiny_tripolar")
    asm._raw_fields = (umo, vmo, fill)
    asm.out = asm.new_output_set()
    asm._out_cap = [asm.N * k + 1 for k in asm.PER_COLUMN_MAX]
    _raw_step(asm, 0)
    kap = (3.0 * g.kappaH, 2.0 * g.kappaVML, 5.0 * g.kappaVdeep)
    full.set_grid(gm, g.mlotst, g.rho, *kap)
    _run(full, "async", umo, vmo, fill)
    asm.kappa = kap  # (only the arguments change: same arrays, same output set)
    _raw_step(asm, KEPT_BITS)
    _same(_host(asm), _host(full), "other κ")
