"""CPU: the line preconditioner's entry points (otmb_op_set_lines, otmb_op_solve_pc, otmb_op_precond and their _dev variants) have the same
types in the same order in the C prototypes (include/otmb.h), the ctypes mirrors and the Julia shim's ccalls, and the shim and
api.DeviceOperator hand the same values over in the same places (the Python side is what the GPU tests execute)."""
import re

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
    cls = API[API.index("\nclass DeviceOperator:"):]
    m = re.search(r"\n    def " + name + r"\(self.*?(?=\n    (?:def |@))", cls, re.S)
    assert m, name
    return m.group(0)


def test_python_makes_the_same_calls():
    py = _method("solve")
    assert re.findall(r"lib\.(otmb_\w+)\(", py) == ["otmb_op_solve_pc"]
    call = py[py.index("lib.otmb_op_solve_pc(") + len("lib.otmb_op_solve_pc("):]
    passed = split_top(" ".join(call[:call.index(", pc)") + len(", pc")].split()))
    assert passed == ["self._h", "int(bool(adjoint))", "k", "None if dc is None else dc.ctypes.data", "float(sigma)", "Bc.ctypes.data", "ldb",
                      "X.ctypes.data", "max(X.shape[0], 1)", "int(x0 is not None)", "float(rtol)", "int(maxiter)", "iters.ctypes.data",
                      "relres.ctypes.data", "reason.ctypes.data", "pc"]
    assert "pc = capi.precond_code(precond)" in py and "if rc != capi.NOT_CONVERGED:" in py
    py = _method("precondition")
    assert re.findall(r"lib\.(otmb_\w+)\(", py) == ["otmb_op_precond"]
    call = py[py.index("lib.otmb_op_precond(") + len("lib.otmb_op_precond("):]
    passed = split_top(" ".join(call[:call.index("max(Z.shape[0], 1)") + len("max(Z.shape[0], 1)")].split()))
    assert passed == ["self._h", "int(bool(adjoint))", "pc", "k", "None if dc is None else dc.ctypes.data", "float(sigma)", "Yc.ctypes.data", "ldy",
                      "Z.ctypes.data", "max(Z.shape[0], 1)"]
    assert 'precond="lines"):' in py.split("\n")[1] and "precond::Symbol = :lines)" in SHIM  # the same default on both sides
    py = _method("set_lines")
    assert re.findall(r"lib\.(otmb_\w+)\(", py) == ["otmb_op_set_lines", "otmb_op_set_lines"]
    assert "lib.otmb_op_set_lines(self._h, None)" in py and "lib.otmb_op_set_lines(self._h, nx.ctypes.data)" in py
    # solve carries the keyword in its own signature, Jacobi by default on both sides
    cls = API[API.index("\nclass DeviceOperator:"):]
    assert '\n    def solve(self, B, d=None, sigma=0.0, rtol=1e-10, maxiter=10000, x0=None, adjoint=False, precond="jacobi"):' in cls
