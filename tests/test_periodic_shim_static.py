"""CPU: otmb_op_periodic and otmb_op_periodic_dev have the same types in the same order in the C prototypes (include/otmb.h), the ctypes mirror
and the Julia shim's ccall, and the shim, api.DeviceOperator and device.Operator hand the same values over in the same places (the Python side
is what the GPU tests execute)."""
import os
import re

from test_julia_shim_static import SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_solve_shim_static import API, CODE, ROOT, _header_names
from test_step_shim_static import _ccall, _method

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


def _passed(py, fn, last):
    call = py[py.index(fn + "(") + len(fn) + 1:]
    return split_top(" ".join(call[:call.index(last + ")") + len(last)].split()))


def test_python_makes_the_same_calls():
    sig = '(self, source, *, dt, ncycle, theta=1.0, first_slot=0, d=None, x0=None, rtol=1e-10, maxiter=10000, adjoint=False, precond="jacobi",\n' \
          '                 ptol=1e-8, restart=30, maxcycles=1000):'
    py = _method("periodic")
    assert "\n    def periodic" + sig in py
    assert re.findall(r"lib\.(otmb_\w+)\(", py) == ["otmb_op_periodic"]
    assert _passed(py, "lib.otmb_op_periodic", "reason.ctypes.data") == [
        "self._h", "int(bool(adjoint))", "k", "None if dc is None else dc.ctypes.data", "float(dt)", "float(theta)", "int(ncycle)", "int(first_slot)",
        "Sc.ctypes.data", "lds", "X.ctypes.data", "max(X.shape[0], 1)", "int(x0 is not None)", "float(rtol)", "int(maxiter)", "pc", "float(ptol)",
        "int(restart)", "int(maxcycles)", "cycles.ctypes.data", "defect.ctypes.data", "reason.ctypes.data"]
    assert "pc = capi.precond_code(precond)" in py and "if rc != capi.NOT_CONVERGED:" in py
    dev = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "device.py"), encoding="utf-8").read()
    m = re.search(r"\n    def periodic\(self.*?(?=\n    def )", dev, re.S)
    assert m and "\n    def periodic" + sig in m.group(0)
    assert _passed(m.group(0), "self.lib.otmb_op_periodic_dev", "reason.ctypes.data") == [
        "self._h", "int(bool(adjoint))", "k", "dp", "float(dt)", "float(theta)", "int(ncycle)", "int(first_slot)", "Sc.data_ptr()", "lds", "X.data_ptr()",
        "max(self.shape[0], 1)", "int(x0 is not None)", "float(rtol)", "int(maxiter)", "pc", "float(ptol)", "int(restart)", "int(maxcycles)",
        "cycles.ctypes.data", "defect.ctypes.data", "reason.ctypes.data"]
    assert re.search(r"\n    def periodic_tracers\(self, source, \*, matrix=\"T\", \*\*kw\):.*?return rec\[\"op\"\]\.periodic\(source, \*\*kw\)", dev, re.S)
    # the same defaults on both sides
    assert "ptol::Real = 1e-8, restart::Integer = 30" in SHIM and "maxcycles::Integer = 1000)" in SHIM
    assert "θ::Real = 1.0, firstslot::Integer = 1" in SHIM
    assert KINDS == header_prototypes()["otmb_op_periodic"][1]
