"""CPU: the Julia shim declares and exports solve! and solve over the resident operator, its one ccall (otmb_op_solve_pc: the preconditioner
is an argument) has the return type, the argument types and the argument ORDER of the C prototype (include/otmb.h) and of the ctypes mirror,
and the shim and api.DeviceOperator.solve hand the same values over in the same places (the Python side is what the GPU tests execute)."""
import inspect
import os
import re

import numpy as np
from operator_calls_rec import CASES, K, N, SIGNATURES, has, host_operator, only, the_call
from operator_calls_rec import header_names as _header_names  # noqa: F401 (the other static tests take it from here)
from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes, julia_kind, split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "api.py"), encoding="utf-8").read()
CALLS = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "operator_calls.py"), encoding="utf-8").read()  # DeviceOperator's solver calls
CODE = "\n".join(l.split("#")[0] for l in SHIM.splitlines())
C_ORDER = ["op", "adjoint", "k", "d", "sigma", "B", "ldb", "X", "ldx", "use_x0", "rtol", "maxiter", "iters", "relres", "reason"]


def _jl(name):
    m = re.search(r"\nfunction " + re.escape(name) + r"\(.*?\n(.*?)\nend\n", SHIM, re.S)
    assert m, name
    return m.group(1)


def test_header_mirror_and_status_codes():
    from otmb_amd import capi

    protos = header_prototypes()
    for name in ("otmb_op_solve", "otmb_op_solve_dev"):
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] == ["i32"], name
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, name
        assert _header_names(name) == C_ORDER, name
    assert protos["otmb_op_solve"] == protos["otmb_op_solve_dev"]
    codes = dict(re.findall(r"(OTMB_ERR_\w+)\s*=\s*(\d+)", HEADER))
    assert codes["OTMB_ERR_SINGULAR_PRECONDITIONER"] == "18" and codes["OTMB_ERR_NOT_CONVERGED"] == "19"
    assert len(set(codes.values())) == len(codes)  # no code is used twice (1-8 carry the reference's error texts)
    assert capi.STATUS_NAMES[18] == "SINGULAR_PRECONDITIONER" and capi.STATUS_NAMES[19] == "NOT_CONVERGED" and capi.NOT_CONVERGED == 19
    reasons = re.search(r"typedef enum \{([^}]*)\} otmb_solve_reason;", HEADER).group(1)
    assert re.findall(r"OTMB_SOLVE_(\w+) = (\d)", reasons) == [("CONVERGED", "0"), ("MAXITER", "1"), ("BREAKDOWN", "2"), ("NONFINITE", "3")]
    assert capi.SOLVE_REASONS == ("converged", "maxiter", "breakdown", "nonfinite")
    assert "const SOLVE_REASONS = (:converged, :maxiter, :breakdown, :nonfinite)" in SHIM
    assert "test/local_full.jl:151-188" in HEADER  # (the reference lines the entry points serve)


def test_shim_defines_and_exports_solve():
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"solve!", "solve"} <= exported
    assert re.search(r"^function solve!\(X::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}, B::StridedVecOrMat\{Float64\};",
                     CODE, re.M)
    sig = CODE[CODE.index("function solve!("):]
    sig = sig[:sig.index(")\n") + 1]
    for kw in ("d::", "σ::", "rtol::", "maxiter::"):
        assert kw in sig, kw
    assert re.search(r"^solve\(D::Union\{DeviceOperator,AdjointDeviceOperator\}, B::StridedVecOrMat\{Float64\}; kwargs\.\.\.\) =\n\s*solve!\(", CODE, re.M)
    # for this module's own types only
    assert "SparseMatrixCSC" not in sig


def test_the_ccall_has_the_prototype_and_the_argument_order_of_the_header():
    from otmb_amd import capi

    body = _jl("solve!")
    assert "solve_fn = sym(:otmb_op_solve_pc)" in body
    assert re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_solve_pc"]  # one route: the preconditioner is an argument
    m = re.search(r"ccall\(solve_fn, (\w+), \((.*?)\),\n(.*?)\)\n", body, re.S)
    assert m, "solve!'s ccall"
    assert len(re.findall(r"\bccall\(", body)) == 1
    jargs = [k for a in split_top(m.group(2).replace("\n", " ")) for k in julia_kind(a)]
    protos = header_prototypes()
    assert (julia_kind(m.group(1))[0], jargs) == protos["otmb_op_solve_pc"]
    res, argtypes = capi.SYMBOLS["otmb_op_solve_pc"]
    assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == jargs
    # the values, place by place, in the header's order
    passed = [" ".join(a.split()) for a in split_top(m.group(3).replace("\n", " "))]
    want = ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "Float64(σ)", "B", "ldb", "X", "ldx", "Int32(x0)", "Float64(rtol)",
            "Int64(maxiter)", "iters", "relres", "reason", "pc"]
    assert passed == want and len(want) == len(C_ORDER) + 1 == 16
    assert "pc = precondcode(precond)" in body and body.index("pc = precondcode(precond)") < body.index("ccall(")
    assert body.index("lock(CALL_LOCK) do") < body.index("ccall(")  # under the module's lock
    assert "rc == 19 || check(rc)" in body  # not converged is an answer; everything else goes through check
    assert "adjoint = D isa AdjointDeviceOperator" in body
    assert "solvepc!" not in SHIM  # no second route beside solve!


def test_python_makes_the_same_call(monkeypatch):
    from otmb_amd import api

    # no decorator: this signature is the one help() shows
    assert str(inspect.signature(api.DeviceOperator.solve)) == SIGNATURES["solve"] and not hasattr(api.DeviceOperator.solve, "__wrapped__")
    D, rec = host_operator(monkeypatch, rc=19)
    B, d = np.asfortranarray(np.ones((N, K))), np.arange(1.0, N + 1)
    for given, sent in CASES:  # (adjoint and the precond code differ in each: neither can stand in the other's place)
        X, info = D.solve(B, d=d, sigma=0.125, **only(given, "adjoint", "precond", "rtol", "maxiter"))
        a = the_call(rec, "otmb_op_solve_pc")  # one call, one route: the preconditioner is an argument
        assert list(a) == C_ORDER + ["precond"] and len(a) == 16  # the values, place by place, in the header's order
        has(a, k=K, d=d.ctypes.data, sigma=0.125, B=B.ctypes.data, ldb=N, X=X.ctypes.data, ldx=N, use_x0=0, iters=info.iterations.ctypes.data,
            relres=info.relres.ctypes.data, **only(sent, "adjoint", "precond", "rtol", "maxiter"))
        assert a["op"] is D._h and info.status == 19 and D.ctx.checked == []  # likewise: reported, not raised
    # no second route beside solve (the twin method was _solve_pc: the name may only occur as the tail of the C symbol's)
    for gone in (r"_precond_keyword", r"(?<!otmb_op)_solve_pc", r"lib\.otmb_op_solve\(", r"\"otmb_op_solve\""):
        assert not re.search(gone, API + CALLS), gone
    # the same defaults on both sides
    assert "rtol::Real = 1e-10, maxiter::Integer = 10000" in SHIM
    assert "precond::Symbol = :jacobi)" in SHIM[SHIM.index("function solve!("):SHIM.index("function solve!(") + 500]
