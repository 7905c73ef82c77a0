"""CPU: otmb_op_periodic and otmb_op_periodic_dev have the same types in the same order in the C prototypes (include/otmb.h), the ctypes mirror
and the Julia shim's ccall, and the shim, api.DeviceOperator and device.Operator hand the same values over in the same places (the Python side
is what the GPU tests execute)."""
import inspect
import os
import re

import numpy as np
from operator_calls_rec import CASES, K, N, PERIODIC, SIGNATURES, has, host_operator, the_call
from test_julia_shim_static import SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_solve_shim_static import API, CALLS, CODE, ROOT, _header_names
from test_step_shim_static import _ccall

ORDER = ["op", "adjoint", "k", "d", "dt", "theta", "ncycle", "first_slot", "S", "lds", "X", "ldx", "use_x0", "rtol", "maxiter", "precond", "ptol",
         "restart", "maxcycles", "cycles", "defect", "reason"]
KINDS = ["ptr", "i32", "i64", "ptr", "f64", "f64", "i64", "i64", "ptr", "i64", "ptr", "i64", "i32", "f64", "i64", "i32", "f64", "i64", "i64", "ptr", "ptr",
         "ptr"]


def test_header_and_mirror():
    from otmb_amd import capi

    protos = header_prototypes()
    for name in ("otmb_op_periodic", "otmb_op_periodic_dev"):
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] == ["i32"], name
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, name
        assert _header_names(name) == ORDER, name
        assert len(args) == len(ORDER)
    assert protos["otmb_op_periodic"] == protos["otmb_op_periodic_dev"]
    # the step's arguments lead, in the step's order, with use_x0 after ldx as in otmb_op_solve_pc
    step = protos["otmb_op_step"][1]
    assert protos["otmb_op_periodic"][1][:12] == step[:12] and protos["otmb_op_periodic"][1][13:16] == step[12:15]
    header = open(os.path.join(ROOT, "include", "otmb.h"), encoding="utf-8").read()
    m = re.search(r"typedef enum \{([^}]*)\} otmb_periodic_reason;", header)
    values = dict((a.strip(), int(b)) for a, b in (x.split("=") for x in m.group(1).split(",")))
    assert values == {"OTMB_PERIODIC_CONVERGED": 0, "OTMB_PERIODIC_MAXCYCLES": 1, "OTMB_PERIODIC_STEP_FAILED": 2, "OTMB_PERIODIC_NONFINITE": 3}
    assert capi.PERIODIC_REASONS == ("converged", "maxcycles", "step_failed", "nonfinite")
    assert "const PERIODIC_REASONS = (:converged, :maxcycles, :step_failed, :nonfinite)" in SHIM


def test_the_shim_defines_exports_and_calls_it():
    from otmb_amd import capi

    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"periodic!", "periodic"} <= exported
    assert re.search(r"^function periodic!\(X::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}, "
                     r"source::StridedVecOrMat\{Float64\}; dt::Real,", CODE, re.M)
    assert re.search(r"^periodic\(D::Union\{DeviceOperator,AdjointDeviceOperator\}, source::StridedVecOrMat\{Float64\}; kwargs\.\.\.\) = "
                     r"periodic!\(zero\(source\), D, source; kwargs\.\.\.\)", CODE, re.M)
    body, ret, jargs, passed = _ccall("periodic!", "periodic_fn")
    assert "periodic_fn = sym(:otmb_op_periodic)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_periodic"]
    assert (ret, jargs) == header_prototypes()["otmb_op_periodic"]
    assert [k for t in capi.SYMBOLS["otmb_op_periodic"][1] for k in ctypes_kind(t)[:1]] == jargs
    assert passed == ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "Float64(dt)", "Float64(θ)", "Int64(ncycle)", "Int64(firstslot - 1)",
                      "source", "lds", "X", "ldx", "Int32(x0)", "Float64(rtol)", "Int64(maxiter)", "pc", "Float64(ptol)", "Int64(restart)",
                      "Int64(maxcycles)", "cycles", "defect", "reason"]
    assert len(passed) == len(ORDER)
    assert "pc = precondcode(precond)" in body and "rc == 19 || check(rc)" in body and "adjoint = D isa AdjointDeviceOperator" in body
    assert len(re.findall(r"\bccall\(", body)) == 1


def test_python_makes_the_same_calls(monkeypatch):
    from otmb_amd import api, device, operator_calls

    D, rec = host_operator(monkeypatch, rc=19)
    S, d, x0 = np.asfortranarray(np.ones((N + 2, K)))[:N], np.arange(1.0, N + 1), np.full((N, K), 2.0)
    for start, (given, sent) in ((start, case) for start in (None, x0) for case in CASES):  # (no 0/1 argument follows another through all four)
        X, info = D.periodic(S, d=d, x0=start, **given, **PERIODIC)
        a = the_call(rec, "otmb_op_periodic")  # outer="none", the default: the unpreconditioned call
        assert list(a) == ORDER
        has(a, k=K, d=d.ctypes.data, S=S.ctypes.data, lds=N + 2, X=X.ctypes.data, ldx=N, use_x0=int(start is not None), cycles=info.cycles.ctypes.data,
            defect=info.defect.ctypes.data, **sent, **PERIODIC)
        assert a["op"] is D._h and np.array_equal(X, np.zeros((N, K)) if start is None else x0) and X.flags.f_contiguous
        assert info.status == 19 and D.ctx.checked == [] and not info.msolve_iters.any()  # reported, not raised
    # both classes: the one method, its keywords in its own signature; device.Operator's reaches otmb_op_periodic_dev
    for cls, suffix in ((api.DeviceOperator, ""), (device.Operator, "_dev")):
        assert cls.periodic is operator_calls.OperatorCalls.periodic and cls._suffix == suffix
        assert str(inspect.signature(cls.periodic)) == SIGNATURES["periodic"] and not hasattr(cls.periodic, "__wrapped__")
    dev = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "device.py"), encoding="utf-8").read()
    assert len(re.findall('"otmb_op_periodic"', CALLS)) == 1 and '"otmb_op_periodic' not in API + dev
    assert re.search(r"\n    def periodic_tracers\(self, source, \*, matrix=\"T\", \*\*kw\):.*?return self\._slotted\(matrix\)\.op\.periodic\(source, \*\*kw\)", dev, re.S)
    # the same defaults on both sides
    assert "ptol::Real = 1e-8, restart::Integer = 30" in SHIM and "maxcycles::Integer = 1000)" in SHIM
    assert "θ::Real = 1.0, firstslot::Integer = 1" in SHIM
    assert KINDS == header_prototypes()["otmb_op_periodic"][1]
