"""CPU: otmb_op_periodic_pc[_dev] and otmb_op_combine_slots[_dev] have the same types in the same order in the C prototypes (include/otmb.h),
the ctypes mirror and the Julia shim's ccalls; the shim's `outer` keyword and `combineslots!`, api.DeviceOperator and device.Operator hand the
same values over in the same places; and the unpreconditioned call is still the one tests/test_periodic_shim_static.py pins."""
import inspect
import os
import re

import numpy as np
from operator_calls_rec import CASES, K, N, PERIODIC, has, host_operator, the_call
from test_julia_shim_static import SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_periodic_shim_static import KINDS, ORDER
from test_solve_shim_static import API, CALLS, CODE, ROOT, _header_names, _jl
from test_step_shim_static import _ccall

PC_ORDER = ORDER + ["outer", "msolve_iters"]
PC_KINDS = KINDS + ["i32", "ptr"]
PASSED_JL = ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "Float64(dt)", "Float64(θ)", "Int64(ncycle)", "Int64(firstslot - 1)", "source",
             "lds", "X", "ldx", "Int32(x0)", "Float64(rtol)", "Int64(maxiter)", "pc", "Float64(ptol)", "Int64(restart)", "Int64(maxcycles)", "cycles", "defect",
             "reason", "oc", "msolve"]


def test_header_and_mirror():
    from otmb_amd import capi

    protos = header_prototypes()
    for name in ("otmb_op_periodic_pc", "otmb_op_periodic_pc_dev"):
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] == ["i32"], name
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args == PC_KINDS, name
        assert _header_names(name) == PC_ORDER, name
    # otmb_op_periodic's arguments lead, in its order
    assert protos["otmb_op_periodic_pc"][1][:len(KINDS)] == protos["otmb_op_periodic"][1]
    for name in ("otmb_op_combine_slots", "otmb_op_combine_slots_dev"):
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] == ["i32"] and [k for t in argtypes for k in ctypes_kind(t)[:1]] == args == ["ptr", "ptr", "i64"], name
        assert _header_names(name) == ["op", "w", "dst"], name
    header = open(os.path.join(ROOT, "include", "otmb.h"), encoding="utf-8").read()
    enums = {}
    for name in ("otmb_outer", "otmb_periodic_pc_reason"):
        m = re.search(r"typedef enum \{([^}]*)\} " + name + ";", header)
        enums[name] = dict((a.strip(), int(b)) for a, b in (x.split("=") for x in m.group(1).split(",")))
    assert enums == {"otmb_outer": {"OTMB_OUTER_NONE": 0, "OTMB_OUTER_MEAN": 1}, "otmb_periodic_pc_reason": {"OTMB_PERIODIC_PRECOND_FAILED": 4}}
    assert capi.OUTERS == {"none": 0, "mean": 1}
    assert capi.PERIODIC_PC_REASONS == capi.PERIODIC_REASONS + ("precond_failed",) and capi.PERIODIC_PC_REASONS.index("precond_failed") == 4
    assert "const PERIODIC_PC_REASONS = (PERIODIC_REASONS..., :precond_failed)" in SHIM and "const OUTERS = (:none, :mean)" in SHIM
    # the library: the old entry points are one-line wrappers that pass OTMB_OUTER_NONE and no msolve_iters
    src = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc", "otmb_periodic.hip"), encoding="utf-8").read()
    for name in ("otmb_op_periodic_dev", "otmb_op_periodic"):
        m = re.search(r"\nint32_t " + name + r"\(otmb_op \*op,[^{]*\{\n(.*?)\n\}\n", src, re.S)
        body = " ".join(m.group(1).split())
        assert body.startswith("return " + name.replace("periodic", "periodic_pc") + "(op, adjoint, k, d, dt, theta, ncycle, first_slot, S, lds, X, ldx, use_x0,")
        assert body.endswith("cycles, defect, reason, OTMB_OUTER_NONE, nullptr);") and body.count(";") == 1, body


def test_the_shim_passes_outer_and_calls_the_new_symbols():
    from otmb_amd import capi

    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"periodic!", "periodic", "combineslots!"} <= exported
    # periodic!: the keyword, its default, and where it goes
    plain = _jl("periodic!")
    assert "outer::Symbol = :none, ptol::Real = 1e-8" in plain
    m = re.search(r"outer === :none \|\| return periodicpc!\(X, D, source, outercode\(outer\); (.*?)\)\n", plain, re.S)
    assert m, plain
    handed = dict(tuple(x.strip() for x in a.split("=")) for a in split_top(" ".join(m.group(1).split())))
    names = ["dt", "ncycle", "θ", "firstslot", "d", "x0", "rtol", "maxiter", "precond", "ptol", "restart", "maxcycles"]
    assert handed == {a: a for a in names}  # every keyword of periodic! but outer, under its own name
    assert re.findall(r"sym\(:(otmb_\w+)\)", plain) == ["otmb_op_periodic"]  # :none is the call it was
    code = _jl("outercode")
    assert "findfirst(==(outer), OUTERS)" in code and "return Int32(i - 1)" in code and "throw(ArgumentError(" in code
    body, ret, jargs, passed = _ccall("periodicpc!", "periodic_pc_fn")
    assert "periodic_pc_fn = sym(:otmb_op_periodic_pc)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_periodic_pc"]
    assert (ret, jargs) == header_prototypes()["otmb_op_periodic_pc"]
    assert [k for t in capi.SYMBOLS["otmb_op_periodic_pc"][1] for k in ctypes_kind(t)[:1]] == jargs
    assert passed == PASSED_JL and len(passed) == len(PC_ORDER)
    assert "pc = precondcode(precond)" in body and "rc == 19 || check(rc)" in body and "adjoint = D isa AdjointDeviceOperator" in body
    assert len(re.findall(r"\bccall\(", body)) == 1
    assert "why = [PERIODIC_PC_REASONS[r + 1] for r in reason]" in body and "msolve_iters = msolve)" in body
    assert "msolve_iters = zeros(Int64, k))" in plain  # the same fields either way
    # combineslots!
    assert re.search(r"^function combineslots!\(D::DeviceOperator, w::Vector\{Float64\}, dst::Integer\)", CODE, re.M)
    body = _jl("combineslots!")
    assert "combine_slots_fn = sym(:otmb_op_combine_slots)" in body and body.index("lock(CALL_LOCK) do") < body.index("ccall(")
    assert "the DeviceOperator has been released" in body
    c = re.search(r"ccall\(combine_slots_fn, (\w+), \((.*?)\), (.*?)\)\)\n", body)
    assert (julia_kind(c.group(1))[0], [k for a in split_top(c.group(2)) for k in julia_kind(a)]) == header_prototypes()["otmb_op_combine_slots"]
    assert [" ".join(a.split()) for a in split_top(c.group(3))] == ["D.handle", "w", "Int64(dst - 1)"]  # the shim counts slots from 1
    assert "length(w) == nslots[] || throw(DimensionMismatch(" in body  # the C side cannot know how many weights it was given


def _cls(text, start):
    return text[text.index(start):]


def test_python_makes_the_same_calls(monkeypatch):
    from otmb_amd import api, capi, device, operator_calls

    dev = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "device.py"), encoding="utf-8").read()
    D, rec = host_operator(monkeypatch, rc=19)
    S, d, x0 = np.asfortranarray(np.ones((N + 2, K)))[:N], np.arange(1.0, N + 1), np.full((N, K), 2.0)
    for start, (given, sent) in ((start, case) for start in (x0, None) for case in CASES):  # (no 0/1 argument follows another through all four)
        X, info = D.periodic(S, d=d, x0=start, outer="mean", **given, **PERIODIC)
        a = the_call(rec, "otmb_op_periodic_pc")
        assert list(a) == PC_ORDER
        has(a, k=K, d=d.ctypes.data, S=S.ctypes.data, lds=N + 2, X=X.ctypes.data, ldx=N, use_x0=int(start is not None), cycles=info.cycles.ctypes.data,
            defect=info.defect.ctypes.data, outer=capi.OUTERS["mean"], msolve_iters=info.msolve_iters.ctypes.data, **sent, **PERIODIC)
        assert info.status == 19 and D.ctx.checked == [] and info.msolve_iters.shape == (K,)  # reported, not raised; the same fields either way
    # the keyword on the real method: "none" is the default and the unpreconditioned export, unknown values are refused before anything is called
    D.periodic(S, dt=2.0, ncycle=2)
    D.periodic(S, dt=2.0, ncycle=2, outer="none")
    assert [name for name, _ in rec.calls] == ["otmb_op_periodic", "otmb_op_periodic"]
    del rec.calls[:]
    try:
        D.periodic(S, dt=2.0, ncycle=2, outer="annual")
        raise AssertionError("an unknown outer was accepted")
    except capi.OtmbError as e:
        assert e.name == "INVALID_ARG" and rec.calls == []
    for text, cls, klass, want in ((API, "\nclass DeviceOperator(", api.DeviceOperator, "otmb_op_combine_slots"),
                                   (dev, "\nclass Operator(", device.Operator, "otmb_op_combine_slots_dev")):
        # the public method is the one method of both classes, outer in its own signature
        assert klass.periodic is operator_calls.OperatorCalls.periodic and inspect.signature(klass.periodic).parameters["outer"].default == "none"
        c = re.search(r"\n    def combine_slots\(self, weights, dst\):.*?(?=\n    (?:def |@))", _cls(text, cls), re.S).group(0)
        assert re.findall(r"\.(otmb_op_combine\w+)\(", c) == [want] and "(self._h, w.ctypes.data, int(dst))" in c, want
    assert len(re.findall('"otmb_op_periodic_pc"', CALLS)) == 1 and '"otmb_op_periodic' not in API + dev  # no second route
    assert re.search(r"\n    def combine_slots\(self, weights, dst, matrix=\"T\"\):.*?op\.combine_slots\(weights, dst\)", dev, re.S)
