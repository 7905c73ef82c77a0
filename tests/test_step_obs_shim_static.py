"""CPU: the observations' entry points (otmb_op_observe, otmb_op_step_obs and the _dev variants) have the same types in the same order in the
C prototypes (include/otmb.h), the ctypes mirror and the Julia shim's ccalls; the first 19 arguments of otmb_op_step_obs are otmb_op_step's;
the shim exports its two new functions; and the Python bindings reach the new entries through private methods only when a new keyword is
given, so step's own call site stays as tests/test_step_shim_static.py reads it."""
import re

from test_julia_shim_static import ctypes_kind, header_prototypes, split_top
from test_solve_shim_static import API, CODE, _header_names
from test_step_shim_static import STEP_ORDER, _ccall, _method

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


def test_python_reaches_the_new_entries_through_private_methods():
    from otmb_amd import capi

    dev = open(capi.__file__.replace("capi.py", "device.py"), encoding="utf-8").read()
    assert re.findall(r"lib\.(otmb_\w+)\(", _method("step")) == ["otmb_op_step"]
    obs = _method("_step_obs")
    assert re.findall(r"lib\.(otmb_\w+)\(", obs) == ["otmb_op_step_obs"]
    call = obs[obs.index("lib.otmb_op_step_obs(") + len("lib.otmb_op_step_obs("):]
    passed = split_top(" ".join(call[:call.index("max(n, 1))") + len("max(n, 1)")].split()))
    plain = _method("step")
    plain = plain[plain.index("lib.otmb_op_step(") + len("lib.otmb_op_step("):]
    assert passed[:19] == split_top(" ".join(plain[:plain.index("reason.ctypes.data)") + len("reason.ctypes.data")].split()))
    assert passed[19:] == ["q", "None if Wc is None else Wc.ctypes.data", "ldw", "None if obs is None else obs.ctypes.data",
                           "None if tw is None else tw.ctypes.data", "None if mean is None else mean.ctypes.data", "max(n, 1)"]
    assert re.findall(r"lib\(\)\.(otmb_\w+)\(", _method("observe")) == ["otmb_op_observe"]
    assert "    @capi.observe_keywords\n    def step(self, X, *, dt," in API and "    @capi.observe_keywords\n    def step(self, X, *, dt," in dev
    for text, plain_sym, obs_sym, one in ((dev, "otmb_op_step_dev", "otmb_op_step_obs_dev", "otmb_op_observe_dev"),):
        assert len(re.findall(r"self\.lib\." + plain_sym + r"\(", text)) == 1 and len(re.findall(r"self\.lib\." + obs_sym + r"\(", text)) == 1
        assert len(re.findall(r"self\.lib\." + one + r"\(", text)) == 1
    # the keywords' switch: neither keyword is the plain method as it stands
    calls = []

    class Probe:
        @capi.observe_keywords
        def step(self, X, **kw):
            calls.append(("plain", kw))

        def _step_obs(self, X, observe, weights, **kw):
            calls.append(("obs", observe, weights, kw))

    Probe().step(0, dt=1.0)
    Probe().step(0, dt=1.0, observe="W")
    Probe().step(0, dt=1.0, time_weights="w")
    assert calls == [("plain", {"dt": 1.0}), ("obs", "W", None, {"dt": 1.0}), ("obs", None, "w", {"dt": 1.0})]
