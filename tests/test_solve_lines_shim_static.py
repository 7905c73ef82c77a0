"""CPU: the line preconditioner's entry points (otmb_op_set_lines, otmb_op_solve_pc, otmb_op_precond and their _dev variants) have the same
types in the same order in the C prototypes (include/otmb.h), the ctypes mirrors and the Julia shim's ccalls, and the shim and
api.DeviceOperator hand the same values over in the same places (the Python side is what the GPU tests execute)."""
import inspect
import re

import numpy as np
from operator_calls_rec import CASES, K, N, SIGNATURES, has, host_operator, only, the_call
from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_solve_shim_static import API, C_ORDER, CODE, _header_names, _jl

PRECOND_ORDER = ["op", "adjoint", "precond", "k", "d", "sigma", "Y", "ldy", "Z", "ldz"]


def test_header_mirror_and_enum():
    from otmb_amd import capi

    protos = header_prototypes()
    for name, order in (("otmb_op_set_lines", ["op", "next"]), ("otmb_op_solve_pc", C_ORDER + ["precond"]), ("otmb_op_precond", PRECOND_ORDER)):
        for n in (name, name + "_dev"):
            ret, args = protos[n]
            res, argtypes = capi.SYMBOLS[n]
            assert ctypes_kind(res) == [ret] == ["i32"], n
            assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, n
            assert _header_names(n) == order, n
        assert protos[name] == protos[name + "_dev"]
    # the old entry points are the new one without its last argument
    assert protos["otmb_op_solve_pc"] == (protos["otmb_op_solve"][0], protos["otmb_op_solve"][1] + ["i32"])
    enum = re.search(r"typedef enum \{([^}]*)\} otmb_precond;", HEADER).group(1)
    assert re.findall(r"OTMB_PRECOND_(\w+) = (\d)", enum) == [("JACOBI", "0"), ("LINES", "1")]
    assert capi.PRECONDS == {"jacobi": 0, "lines": 1}
    assert "const PRECONDS = (jacobi = Int32(0), lines = Int32(1))" in SHIM


def test_shim_defines_and_exports_the_lines_api():
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"setlines!", "verticallines", "precondition!", "solve!", "solve"} <= exported
    assert re.search(r"^function setlines!\(D::DeviceOperator, next::Union\{Nothing,Vector\{Int64\}\}\)", CODE, re.M)
    assert re.search(r"^function verticallines\(indices\)", CODE, re.M)
    assert re.search(r"^function precondition!\(Z::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}, Y::StridedVecOrMat\{Float64\};",
                     CODE, re.M)
    # solve! takes the keyword (its single ccall hands the code over: test_solve_shim_static.py)
    assert "precond::Symbol = :jacobi" in _jl("solve!")


def _ccall(fn, var):
    body = _jl(fn)
    m = re.search(r"ccall\(" + var + r", (\w+), \((.*?)\),\n(.*?)\)\)?\n", body, re.S)
    assert m, fn
    jargs = [k for a in split_top(m.group(2).replace("\n", " ")) for k in julia_kind(a)]
    passed = [" ".join(a.split()) for a in split_top(m.group(3).replace("\n", " "))]
    return body, julia_kind(m.group(1))[0], jargs, passed


def test_the_ccalls_have_the_prototypes_and_the_argument_order_of_the_header():
    from otmb_amd import capi

    protos = header_prototypes()
    body, ret, jargs, passed = _ccall("solve!", "solve_fn")
    assert "solve_fn = sym(:otmb_op_solve_pc)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_solve_pc"]
    assert (ret, jargs) == protos["otmb_op_solve_pc"]
    assert [k for t in capi.SYMBOLS["otmb_op_solve_pc"][1] for k in ctypes_kind(t)[:1]] == jargs
    assert passed == ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "Float64(σ)", "B", "ldb", "X", "ldx", "Int32(x0)", "Float64(rtol)",
                      "Int64(maxiter)", "iters", "relres", "reason", "pc"]
    assert "pc = precondcode(precond)" in body and "rc == 19 || check(rc)" in body and body.index("lock(CALL_LOCK) do") < body.index("ccall(")

    body, ret, jargs, passed = _ccall("precondition!", "precond_fn")
    assert "precond_fn = sym(:otmb_op_precond)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_precond"]
    assert (ret, jargs) == protos["otmb_op_precond"]
    assert [k for t in capi.SYMBOLS["otmb_op_precond"][1] for k in ctypes_kind(t)[:1]] == jargs
    assert passed == ["op.handle", "Int32(adjoint)", "pc", "k", "d === nothing ? C_NULL : d", "Float64(σ)", "Y", "ldy", "Z", "ldz"]
    assert len(passed) == len(PRECOND_ORDER) and body.index("lock(CALL_LOCK) do") < body.index("ccall(")

    body = _jl("setlines!")
    assert "set_lines_fn = sym(:otmb_op_set_lines)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_set_lines"]
    m = re.search(r"ccall\(set_lines_fn, (\w+), \((.*?)\), (.*?)\)\)\n", body)
    assert m, "setlines!'s ccall"
    assert (julia_kind(m.group(1))[0], [k for a in split_top(m.group(2)) for k in julia_kind(a)]) == protos["otmb_op_set_lines"]
    assert [" ".join(a.split()) for a in split_top(m.group(3))] == ["D.handle", "next === nothing ? C_NULL : next"]
    assert body.index("lock(CALL_LOCK) do") < body.index("ccall(")


def _method(name):
    cls = API[API.index("\nclass DeviceOperator("):]
    m = re.search(r"\n    def " + name + r"\(self.*?(?=\n    (?:def |@))", cls, re.S)
    assert m, name
    return m.group(0)


def test_python_makes_the_same_calls(monkeypatch):
    from otmb_amd import api

    D, rec = host_operator(monkeypatch, rc=19)
    B, d = np.asfortranarray(np.ones((N, K))), np.arange(1.0, N + 1)
    for given, sent in CASES:  # adjoint with "jacobi" (0), then no adjoint with "lines" (otmb_precond's 1): the two never agree
        X, info = D.solve(B, d=d, sigma=0.125, **only(given, "adjoint", "precond", "rtol", "maxiter"))
        a = the_call(rec, "otmb_op_solve_pc")
        assert list(a) == C_ORDER + ["precond"]
        has(a, k=K, d=d.ctypes.data, sigma=0.125, B=B.ctypes.data, ldb=N, X=X.ctypes.data, ldx=N, use_x0=0, iters=info.iterations.ctypes.data,
            relres=info.relres.ctypes.data, **only(sent, "adjoint", "precond", "rtol", "maxiter"))
        assert info.status == 19 and D.ctx.checked == []
        Z = D.precondition(B, d=d, sigma=0.125, **only(given, "adjoint", "precond"))
        a = the_call(rec, "otmb_op_precond")
        assert list(a) == PRECOND_ORDER
        has(a, k=K, d=d.ctypes.data, sigma=0.125, Y=B.ctypes.data, ldy=N, Z=Z.ctypes.data, ldz=N, **only(sent, "adjoint", "precond"))
        assert D.ctx.checked.pop() == 19 and D.ctx.checked == []  # (no report to put a status in: the context judges it)
    assert inspect.signature(api.DeviceOperator.precondition).parameters["precond"].default == "lines"
    assert "precond::Symbol = :lines)" in SHIM  # the same default on both sides
    py = _method("set_lines")
    assert re.findall(r"lib\.(otmb_\w+)\(", py) == ["otmb_op_set_lines", "otmb_op_set_lines"]
    assert "lib.otmb_op_set_lines(self._h, None)" in py and "lib.otmb_op_set_lines(self._h, nx.ctypes.data)" in py
    # solve carries the keyword in its own signature, Jacobi by default on both sides
    assert str(inspect.signature(api.DeviceOperator.solve)) == SIGNATURES["solve"]
