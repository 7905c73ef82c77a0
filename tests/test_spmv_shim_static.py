"""CPU: the Julia shim defines and exports the resident operator (DeviceOperator, setvalues!, mul!, `*` on its own types), every new ccall
matches its C prototype and the ctypes mirror, and the shim makes the same C calls in the same order as api.DeviceOperator (which the GPU
tests execute).  Its finalizer reaches only otmb_op_destroy, which touches no context, and never waits for the module's lock."""
import os
import re

from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes, julia_kind, split_top

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "api.py"), encoding="utf-8").read()
SRC = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "csrc", "otmb_spmv.hip"), encoding="utf-8").read()
CODE = "\n".join(l.split("#")[0] for l in SHIM.splitlines())
NEW = ("otmb_op_create_dev", "otmb_op_create", "otmb_op_set_values_dev", "otmb_op_set_values", "otmb_op_mul_dev", "otmb_op_mul",
       "otmb_op_info", "otmb_op_destroy")


def _jl(name):
    m = re.search(r"\nfunction " + re.escape(name) + r"\(.*?\n(.*?)\nend\n", SHIM, re.S)
    assert m, name
    return m.group(1)


def _py_method(name):
    cls = API[API.index("\nclass DeviceOperator("):]
    cls = cls[:re.search(r"\n(?:def |class )", cls[1:]).start() + 1]
    m = re.search(r"\n    def " + name + r"\(.*?(?=\n    def |\Z)", cls, re.S)
    assert m, name
    return m.group(0)


def test_header_and_mirror_declare_the_operator():
    from otmb_amd import capi

    protos = header_prototypes()
    for name in NEW:
        assert name in protos, name
        ret, args = protos[name]
        res, argtypes = capi.SYMBOLS[name]
        assert ctypes_kind(res) == [ret], name
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, name
    assert "typedef struct otmb_op otmb_op;" in HEADER
    assert "test/local_full.jl:96-107" in HEADER  # (the reference lines the entry points serve)


def test_shim_defines_and_exports_the_operator():
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"DeviceOperator", "setvalues!"} <= exported
    assert re.search(r"^mutable struct DeviceOperator$", CODE, re.M)
    assert re.search(r"^function DeviceOperator\(A::SparseMatrixCSC\{Float64,Int64\}\)", CODE, re.M)
    assert re.search(r"^function setvalues!\(D::DeviceOperator, nzval::Vector\{Float64\}\)", CODE, re.M)
    assert re.search(r"^LinearAlgebra\.mul!\(Y::StridedVecOrMat\{Float64\}, D::DeviceOperator, X::StridedVecOrMat\{Float64\}, α::Number, β::Number\)",
                     CODE, re.M)
    assert re.search(r"^LinearAlgebra\.mul!\(Y::StridedVecOrMat\{Float64\}, A::AdjointDeviceOperator, X::StridedVecOrMat\{Float64\}, α::Number, "
                     r"β::Number\)", CODE, re.M)
    assert "Base.adjoint(D::DeviceOperator) = AdjointDeviceOperator(D)" in CODE
    # `*` and mul! for the module's own types only: nothing on SparseMatrixCSC (no type piracy), `import`, not `using`, LinearAlgebra
    stars = re.findall(r"^Base\.:\*\((.*?)\)\s*=", CODE, re.M)
    assert stars == ["D::Union{DeviceOperator,AdjointDeviceOperator}, X::StridedVecOrMat{Float64}"], stars
    for line in CODE.splitlines():
        if re.match(r"^(LinearAlgebra\.mul!|Base\.:\*)\(", line):
            assert "SparseMatrixCSC" not in line, line
    assert re.search(r"^import LinearAlgebra$", CODE, re.M) and not re.search(r"^using LinearAlgebra", CODE, re.M)
    # `A * x` / `A' * v` are mul!(…, true, false); the shim hands Bool α / β over as Float64 (1.0, 0.0)
    assert "LinearAlgebra.mul!(Y, D, X, true, false)" in CODE and "Float64(α), Float64(β)" in CODE


def test_the_operators_answer_every_size_call_the_shim_makes():
    """DeviceOperator / AdjointDeviceOperator are not AbstractArrays: Base has no size(x, d) for them.  Every size call on them in the shim
    must have a method of its own (the shim cannot be run here: no Julia toolchain)."""
    assert "Base.size(D::DeviceOperator) = (D.m, D.n)" in CODE and "Base.size(A::AdjointDeviceOperator) = (A.parent.n, A.parent.m)" in CODE
    assert re.search(r"^Base\.size\(D::Union\{DeviceOperator,AdjointDeviceOperator\}, d::Integer\) =", CODE, re.M)
    block = CODE[CODE.index("mutable struct DeviceOperator"):CODE.index("function setvalues!")]
    # the operator arguments of the block's methods are D and A; X / Y are StridedVecOrMat (AbstractArrays)
    for call in re.findall(r"\bsize\((\w+(?:\.\w+)?)\s*(,[^)]*)?\)", block):
        var, rest = call
        assert var in ("D", "A", "A.parent", "X", "Y"), call


def test_every_new_ccall_matches_its_prototype():
    from otmb_amd import capi

    protos = header_prototypes()
    calls = re.findall(r"ccall\(\s*sym\(:(otmb_op_\w+)\)\s*,\s*(\w+)\s*,\s*\((.*?)\)\s*,", SHIM, re.S)
    assert sorted({c[0] for c in calls}) == ["otmb_op_create", "otmb_op_mul", "otmb_op_set_values"]
    for name, ret, args in calls:
        jargs = [k for a in split_top(args.replace("\n", " ")) for k in julia_kind(a)]
        assert (julia_kind(ret)[0], jargs) == protos[name], name
        res, argtypes = capi.SYMBOLS[name]
        assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == jargs, name
    # the finalizer's call goes through a pointer resolved in __init__ (finalizers do not look symbols up)
    m = re.search(r"ccall\(op_destroy_fn\[\], (\w+), \((.*?)\), D\.handle\)", SHIM)
    assert m and (julia_kind(m.group(1))[0], [k for a in split_top(m.group(2)) for k in julia_kind(a)]) == protos["otmb_op_destroy"]
    assert "op_destroy_fn[] = Libdl.dlsym(lib[], :otmb_op_destroy)" in SHIM


def test_shim_and_python_make_the_same_calls_in_the_same_order():
    pairs = (("DeviceOperator", "__init__", ["otmb_op_create"]), ("opmul!", "mul", ["otmb_op_mul"]),
             ("setvalues!", "set_values", ["otmb_op_set_values"]))
    for jname, pname, want in pairs:
        jl, py = _jl(jname), _py_method(pname)
        assert re.findall(r"sym\(:(otmb_\w+)\)", jl) == want, jname
        assert re.findall(r"lib\.(otmb_\w+)\(", py) == want, pname
        assert jl.index("lock(CALL_LOCK) do") < jl.index("ccall("), jname  # under the module's lock
    # both pass the length they were given to set_values, and the same ldx / ldy rule (rows of X / Y for a vector or one column)
    assert "length(nzval)" in _jl("setvalues!") and "len(v)" in _py_method("set_values")
    assert "Int32(adjoint), k, X, ldx, Y, ldy" in _jl("opmul!") and "int(bool(adjoint)), k, Xc.ctypes.data, ldx, Yc.ctypes.data, ldy" in _py_method("mul")
    # releasing: the finalizer / close both end in otmb_op_destroy
    assert re.findall(r"lib\(\)\.(otmb_\w+)\(", _py_method("close")) == ["otmb_op_destroy"]
    assert "op_destroy_fn[]" in _jl("release!")


def test_the_finalizer_never_waits_and_touches_no_context():
    rel = _jl("release!")
    assert "trylock(CALL_LOCK)" in rel and "lock(CALL_LOCK) do" not in rel and "context()" not in rel and "ctx[]" not in rel
    assert "sym(" not in rel
    assert re.search(r"finalizer\(D\) do d\n\s*release!\(d\)\n\s*end", _jl("DeviceOperator"))
    assert re.search(r"else\n\s*finalizer\(D\) do d\n\s*release!\(d\)\n\s*end", rel)  # busy lock: registered again
    # the C side keeps the promise: otmb_op_destroy reads nothing of op->ctx
    body = SRC[SRC.index("void otmb_op_destroy(otmb_op *op) {"):]
    body = body[:body.index("\n}\n")]
    assert "ctx" not in body
    free_all = SRC[SRC.index("static void sp_free_all(otmb_op *op) {"):]
    assert "ctx" not in free_all[:free_all.index("\n}\n")]
