"""CPU: the observations' entry points (otmb_op_observe, otmb_op_step_obs and the _dev variants) have the same types in the same order in the
C prototypes (include/otmb.h), the ctypes mirror and the Julia shim's ccalls; the first 19 arguments of otmb_op_step_obs are otmb_op_step's;
the shim exports its two new functions; and the Python bindings reach the new entries only when a new keyword is given, so step's own call
stays as tests/test_step_shim_static.py reads it."""
import inspect
import re

import numpy as np
from operator_calls_rec import CASES, K, N, SIGNATURES, has, host_operator, the_call
from test_julia_shim_static import ctypes_kind, header_prototypes, split_top
from test_solve_shim_static import API, CALLS, CODE, _header_names
from test_step_shim_static import STEP_ORDER, _ccall

OBSERVE_ORDER = ["op", "k", "q", "W", "ldw", "X", "ldx", "obs"]
STEP_OBS_ORDER = STEP_ORDER + ["q", "W", "ldw", "obs", "tw", "Xbar", "ldm"]
NAMES = {"otmb_op_observe": OBSERVE_ORDER, "otmb_op_observe_dev": OBSERVE_ORDER, "otmb_op_step_obs": STEP_OBS_ORDER, "otmb_op_step_obs_dev": STEP_OBS_ORDER}


def test_header_and_mirror():
    from otmb_amd import capi

    protos = header_prototypes()
    for name, order in NAMES.items():
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret] == ["i32"], name
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, name
        assert _header_names(name) == order, name
    assert protos["otmb_op_observe"] == protos["otmb_op_observe_dev"] and protos["otmb_op_step_obs"] == protos["otmb_op_step_obs_dev"]
    # the observed step is the step with seven arguments behind its nineteen
    assert protos["otmb_op_step_obs"][1][:19] == protos["otmb_op_step"][1] and _header_names("otmb_op_step_obs")[:19] == _header_names("otmb_op_step")
    assert protos["otmb_op_step_obs"][1][19:] == ["i64", "ptr", "i64", "ptr", "ptr", "ptr", "i64"]
    assert protos["otmb_op_observe"][1] == ["ptr", "i64", "i64", "ptr", "i64", "ptr", "i64", "ptr"]


def test_the_shim_exports_and_calls_them_with_the_headers_types_and_order():
    from otmb_amd import capi

    protos = header_prototypes()
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"observe", "stepobserve!", "step!"} <= exported
    assert re.search(r"^function observe\(D::DeviceOperator, W::StridedVecOrMat\{Float64\}, X::StridedVecOrMat\{Float64\}\)", CODE, re.M)
    assert re.search(r"^function stepobserve!\(X::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}; dt::Real,", CODE, re.M)

    def check(fn, var, sym, want):
        body, ret, jargs, passed = _ccall(fn, var)  # (under CALL_LOCK, behind the released-operator check)
        assert f"{var} = sym(:{sym})" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == [sym], fn
        assert (ret, jargs) == protos[sym], fn
        assert [k for t in capi.SYMBOLS[sym][1] for k in ctypes_kind(t)[:1]] == jargs, fn
        assert passed == want and len(want) == len(NAMES[sym]), (fn, passed)
        assert len(re.findall(r"\bccall\(", body)) == 1
        return body

    check("observe", "observe_fn", "otmb_op_observe", ["D.handle", "k", "q", "W", "ldw", "X", "ldx", "obs"])
    _, _, _, step_passed = _ccall("step!", "step_fn")
    body = check("stepobserve!", "step_obs_fn", "otmb_op_step_obs",
                 step_passed + ["Int64(q)", "observers === nothing ? C_NULL : observers", "ldw", "observers === nothing ? C_NULL : obs",
                                "timeweights === nothing ? C_NULL : timeweights", "Xbar === nothing ? C_NULL : Xbar", "ldm"])
    assert "rc == 19 || check(rc)" in body and "obs = zeros(Float64, q, k, nrep)" in body  # (q, k, nsteps) column-major: the C side's layout
    # step! keeps its own ccall
    assert re.findall(r"sym\(:(otmb_\w+)\)", _ccall("step!", "step_fn")[0]) == ["otmb_op_step"]


def test_python_reaches_the_new_entries_only_when_a_keyword_is_given(monkeypatch):
    from otmb_amd import api, device, operator_calls

    dev = open(device.__file__, encoding="utf-8").read()
    D, rec = host_operator(monkeypatch, rc=19)
    X, W, tw = np.asfortranarray(np.ones((N, K))), np.asfortranarray(np.ones((N + 2, 2)))[:N], np.array([0.25, 0.75])
    for given, sent in CASES:  # (adjoint and the precond code differ in each)
        D.step(X, nsteps=2, **given)
        plain = the_call(rec, "otmb_op_step")  # neither keyword: the plain call as tests/test_step_shim_static.py reads it
        has(plain, k=K, nsteps=2, **sent)
        Xn, info = D.step(X, nsteps=2, observe=W, time_weights=tw, **given)
        a = the_call(rec, "otmb_op_step_obs")
        assert list(a) == STEP_OBS_ORDER and list(a)[:19] == list(plain)
        scalars = [n for n in STEP_ORDER if n not in ("op", "X", "steps_done", "iters", "relres", "reason")]  # (each call has its own state and reports)
        assert [a[n] for n in scalars] == [plain[n] for n in scalars] and a["op"] is plain["op"] is D._h and a["X"] == Xn.ctypes.data
        has(a, q=2, W=W.ctypes.data, ldw=N + 2, tw=tw.ctypes.data, ldm=N)
        assert a["obs"] is not None and a["Xbar"] is not None and info.observations.shape == (0, K, 2) and info.status == 19 and D.ctx.checked == []
        # the keywords' switch: either keyword is the observed call, with null for the other's arrays
        D.step(X, nsteps=2, observe=np.ones(N), **given)
        a = the_call(rec, "otmb_op_step_obs")
        has(a, q=1, ldw=N, tw=None, Xbar=None, ldm=N)
        assert a["W"] is not None and a["obs"] is not None
        _, info = D.step(X, nsteps=2, time_weights=tw, **given)
        a = the_call(rec, "otmb_op_step_obs")
        has(a, q=0, W=None, ldw=N, obs=None, tw=tw.ctypes.data, ldm=N)
        assert a["Xbar"] is not None and info.observations is None
    obs = D.observe(W, X)
    has(the_call(rec, "otmb_op_observe"), k=K, q=2, W=W.ctypes.data, ldw=N + 2, X=X.ctypes.data, ldx=N, obs=obs.ctypes.data)
    # both classes take the keywords in step's own signature and make these calls with the one method: device.Operator's reach the _dev exports
    for cls, suffix in ((api.DeviceOperator, ""), (device.Operator, "_dev")):
        assert cls.step is operator_calls.OperatorCalls.step and cls.observe is operator_calls.OperatorCalls.observe and cls._suffix == suffix
        assert str(inspect.signature(cls.step)) == SIGNATURES["step"] and not hasattr(cls.step, "__wrapped__")
    for name in ("otmb_op_step", "otmb_op_step_obs", "otmb_op_observe"):  # each export is named once, its suffix the class's
        assert len(re.findall('"' + name + '"', CALLS)) == 1 and '"' + name not in API + dev, name
