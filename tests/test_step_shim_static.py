"""CPU: the value slots' and the step's entry points (otmb_op_set_slots, otmb_op_set_values_slot, otmb_op_select_slot, otmb_op_slots,
otmb_op_step and the _dev variants) have the same types in the same order in the C prototypes (include/otmb.h), the ctypes mirror and the
Julia shim's ccalls, and the shim and api.DeviceOperator hand the same values over in the same places (the Python side is what the GPU
tests execute)."""
import inspect
import re

import numpy as np
from operator_calls_rec import CASES, K, N, SIGNATURES, has, host_operator, the_call
from test_julia_shim_static import SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_solve_shim_static import API, CODE, _header_names, _jl

STEP_ORDER = ["op", "adjoint", "k", "d", "dt", "theta", "nsteps", "first_slot", "S", "lds", "X", "ldx", "rtol", "maxiter", "precond", "steps_done",
              "iters", "relres", "reason"]
NAMES = {"otmb_op_set_slots": ["op", "nslots"], "otmb_op_set_values_slot": ["op", "slot", "nzval", "nnz"],
         "otmb_op_set_values_slot_dev": ["op", "slot", "nzval", "nnz"], "otmb_op_select_slot": ["op", "slot"],
         "otmb_op_slots": ["op", "nslots", "selected"], "otmb_op_step": STEP_ORDER, "otmb_op_step_dev": STEP_ORDER}


def test_header_and_mirror():
    from otmb_amd import capi

    protos = header_prototypes()
    for name, order in NAMES.items():
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] == ["i32"], name
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, name
        assert _header_names(name) == order, name
    assert protos["otmb_op_step"] == protos["otmb_op_step_dev"] and protos["otmb_op_set_values_slot"] == protos["otmb_op_set_values_slot_dev"]
    # set_values_slot is set_values with the slot in second place
    assert protos["otmb_op_set_values_slot"][1] == protos["otmb_op_set_values"][1][:1] + ["i64"] + protos["otmb_op_set_values"][1][1:]


def _ccall(fn, var):
    body = _jl(fn)
    m = re.search(r"ccall\(" + var + r", (\w+), \((.*?)\),\s(.*?)\)\)?\n", body, re.S)
    assert m, fn
    jargs = [k for a in split_top(m.group(2).replace("\n", " ")) for k in julia_kind(a)]
    passed = [" ".join(a.split()) for a in split_top(m.group(3).replace("\n", " "))]
    assert body.index("lock(CALL_LOCK) do") < body.index("ccall("), fn
    assert "the DeviceOperator has been released" in body, fn
    return body, julia_kind(m.group(1))[0], jargs, passed


def test_shim_defines_and_exports_the_slots_and_the_step():
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"setslots!", "selectslot!", "slots", "step!"} <= exported
    assert re.search(r"^function setslots!\(D::DeviceOperator, nslots::Integer\)", CODE, re.M)
    assert re.search(r"^function setvalues!\(D::DeviceOperator, nzval::Vector\{Float64\}, slot::Integer\)", CODE, re.M)
    assert re.search(r"^function selectslot!\(D::DeviceOperator, slot::Integer\)", CODE, re.M)
    assert re.search(r"^function step!\(X::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}; dt::Real,", CODE, re.M)
    # `step` is Base's name: a method for this module's own types, not a second function of that name
    assert re.search(r"^Base\.step\(D::Union\{DeviceOperator,AdjointDeviceOperator\}, X::StridedVecOrMat\{Float64\}; kwargs\.\.\.\) = step!\(copy\(X\), D; kwargs\.\.\.\)",
                     CODE, re.M)


def test_the_ccalls_have_the_prototypes_and_the_argument_order_of_the_header():
    from otmb_amd import capi

    protos = header_prototypes()

    def check(fn, var, sym, want):
        body, ret, jargs, passed = _ccall(fn, var)
        assert f"{var} = sym(:{sym})" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == [sym], fn
        assert (ret, jargs) == protos[sym], fn
        assert [k for t in capi.SYMBOLS[sym][1] for k in ctypes_kind(t)[:1]] == jargs, fn
        assert passed == want and len(want) == len(NAMES[sym]), (fn, passed)
        return body

    check("setslots!", "set_slots_fn", "otmb_op_set_slots", ["D.handle", "Int64(nslots)"])
    check("selectslot!", "select_slot_fn", "otmb_op_select_slot", ["D.handle", "Int64(slot - 1)"])  # the shim counts slots from 1
    check("slots", "slots_fn", "otmb_op_slots", ["D.handle", "n", "sel"])
    assert "return (n[], sel[] + 1)" in _jl("slots")
    # setvalues! with a slot: the second method of that name (the first one is test_spmv_shim_static.py's)
    m = re.search(r"\nfunction setvalues!\(D::DeviceOperator, nzval::Vector\{Float64\}, slot::Integer\)\n(.*?)\nend\n", SHIM, re.S)
    body = m.group(1)
    assert "set_values_slot_fn = sym(:otmb_op_set_values_slot)" in body and body.index("lock(CALL_LOCK) do") < body.index("ccall(")
    c = re.search(r"ccall\(set_values_slot_fn, (\w+), \((.*?)\), (.*?)\)\)\n", body)
    assert (julia_kind(c.group(1))[0], [k for a in split_top(c.group(2)) for k in julia_kind(a)]) == protos["otmb_op_set_values_slot"]
    assert [" ".join(a.split()) for a in split_top(c.group(3))] == ["D.handle", "Int64(slot - 1)", "nzval", "length(nzval)"]
    body = check("step!", "step_fn", "otmb_op_step",
                 ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "Float64(dt)", "Float64(θ)", "Int64(nsteps)", "Int64(firstslot - 1)",
                  "source === nothing ? C_NULL : source", "lds", "X", "ldx", "Float64(rtol)", "Int64(maxiter)", "pc", "done", "iters", "relres", "reason"])
    assert "pc = precondcode(precond)" in body and "rc == 19 || check(rc)" in body and "adjoint = D isa AdjointDeviceOperator" in body
    assert len(re.findall(r"\bccall\(", body)) == 1
    # the report arrays are k x nsteps in Julia's column-major order: the C side's step-major nsteps x k
    assert "iters = zeros(Int64, k, nrep)" in body and "reason = zeros(Int32, k, nrep)" in body


def _method(name):
    cls = API[API.index("\nclass DeviceOperator("):]
    m = re.search(r"\n    def " + name + r"\(self.*?(?=\n    (?:def |@))", cls, re.S)
    assert m, name
    return m.group(0)


def test_python_makes_the_same_calls(monkeypatch):
    from otmb_amd import api

    assert str(inspect.signature(api.DeviceOperator.step)) == SIGNATURES["step"]
    D, rec = host_operator(monkeypatch, rc=19)
    X, d = np.asfortranarray(np.ones((N, K))), np.arange(1.0, N + 1)
    S = np.asfortranarray(np.ones((N + 2, K)))[:N]
    for given, sent in CASES:  # (adjoint and the precond code differ in each, and no two integers of a call are equal)
        Xn, info = D.step(X, nsteps=2, source=S, d=d, **given)
        a = the_call(rec, "otmb_op_step")
        assert list(a) == STEP_ORDER
        has(a, k=K, d=d.ctypes.data, nsteps=2, S=S.ctypes.data, lds=N + 2, X=Xn.ctypes.data, ldx=N, iters=info.iterations.ctypes.data,
            relres=info.relres.ctypes.data, **sent)
        assert a["op"] is D._h and a["X"] != X.ctypes.data and np.array_equal(Xn, X)  # the steps run on a copy
        assert info.status == 19 and D.ctx.checked == []  # reported, not raised
    for name, sym in (("set_slots", "otmb_op_set_slots"), ("select", "otmb_op_select_slot"), ("slots", "otmb_op_slots"),
                      ("_set_slot_values", "otmb_op_set_values_slot")):
        assert re.findall(r"lib\(\)\.(otmb_\w+)\(", _method(name)) == [sym], name
    assert "self._set_slot_values(v, slot)" in _method("set_values")
    # the same defaults on both sides
    assert "θ::Real = 1.0, nsteps::Integer = 1" in SHIM and "rtol::Real = 1e-10, maxiter::Integer = 10000, precond::Symbol = :jacobi)" in SHIM
