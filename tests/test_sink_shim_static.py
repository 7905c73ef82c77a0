"""CPU: otmb_build_sink and otmb_op_add_matrix (and their _dev variants) have the same types in the same order in the C prototypes
(include/otmb.h), the ctypes mirror and the Julia shim's ccalls; the shim defines buildTsink(; w, gridmetrics, indices, seafloor = :open) and
addmatrix!(D, B; alpha = 1.0, slots = nothing), exports addmatrix! (the buildT* functions are unexported, like the reference's), passes the
arguments in the header's order and numbers the slots from 1; the two new status codes have their numbers and texts."""
import re

from operator_calls_rec import header_names
from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes, julia_kind, split_top

CODE = "\n".join(l.split("#")[0] for l in SHIM.splitlines())
SINK_ORDER = ["ctx", "w_form", "w_scalar", "w", "v3d", "area2d", "lwet3d", "lwet", "n_wet", "nx", "ny", "nz", "closed", "colptr", "rowval", "nzval", "cap", "nnz"]
ADD_ORDER = ["op", "m", "n", "colptr", "rowval", "nzval", "alpha", "nsel", "slots"]


def _function(name):
    m = re.search(r"\nfunction " + re.escape(name) + r"\((.*?)\)\n(.*?)\nend\n", SHIM, re.S)
    assert m, name
    return " ".join(m.group(1).split()), m.group(2)


def _ccall(body, var):
    m = re.search(r"ccall\(" + var + r", (\w+),\s*\((.*?)\),\s(.*?)\)\)\n", body, re.S)
    assert m, var
    assert len(re.findall(r"\bccall\(", body)) == 1
    jargs = [k for a in split_top(m.group(2).replace("\n", " ")) for k in julia_kind(a)]
    passed = [" ".join(a.split()) for a in split_top(m.group(3).replace("\n", " "))]
    assert body.index("lock(CALL_LOCK) do") < body.index("ccall(")
    return julia_kind(m.group(1))[0], jargs, passed


def test_header_mirror_and_status_codes():
    from otmb_amd import capi

    protos = header_prototypes()
    for name, order in (("otmb_build_sink", SINK_ORDER), ("otmb_op_add_matrix", ADD_ORDER)):
        for suffix in ("", "_dev"):
            ret, args = protos[name + suffix]
            res, argtypes = capi.SYMBOLS[name + suffix]
            assert ctypes_kind(res) == [ret] == ["i32"], name
            assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, name
            assert header_names(name + suffix) == order, name
        assert protos[name] == protos[name + "_dev"]
    codes = dict(re.findall(r"(OTMB_ERR_\w+)\s*=\s*(\d+)", HEADER))
    assert codes["OTMB_ERR_TSINK_NAN"] == "20" and codes["OTMB_ERR_PATTERN_NOT_CONTAINED"] == "21"
    assert capi.STATUS_NAMES[20] == "TSINK_NAN" and capi.STATUS_NAMES[21] == "PATTERN_NOT_CONTAINED"
    assert capi.lib().otmb_status_string(20).decode() == "Tsink contains NaNs."
    assert "pattern" in capi.lib().otmb_status_string(21).decode()


def test_the_shim_defines_buildTsink_over_otmb_build_sink():
    from otmb_amd import capi

    sig, body = _function("buildTsink")
    assert sig == "; w, gridmetrics, indices, seafloor::Symbol = :open"
    assert "build_sink_fn = sym(:otmb_build_sink)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_build_sink"]
    ret, jargs, passed = _ccall(body, "build_sink_fn")
    assert (ret, jargs) == header_prototypes()["otmb_build_sink"]
    assert [k for t in capi.SYMBOLS["otmb_build_sink"][1] for k in ctypes_kind(t)[:1]] == jargs
    assert len(passed) == len(SINK_ORDER)
    assert passed == ["context()", "wform", "w isa Number ? Float64(w) : 0.0", "wa", "v", "ar", "lw3", "lw", "N", "nx", "ny", "nz", "Int32(seafloor === :closed)",
                      "colptr", "rowval", "nzval", "cap", "k"]
    # the three forms of w, the two seafloors, the result trimmed to nnz
    assert "w isa Number ? Int32(0) : ndims(w) == 1 ? Int32(1) : Int32(2)" in body
    assert "seafloor in (:open, :closed) || throw(ArgumentError(" in body
    assert "size(wa) == (nz,) || size(wa) == (nx, ny, nz) || throw(DimensionMismatch(" in body
    assert "resize!(rowval, k[]); resize!(nzval, k[])" in body and "SparseMatrixCSC{Float64,Int64}(N, N, colptr, rowval, nzval)" in body
    assert "cap = max(2N, 1)" in body


def test_the_shim_defines_and_exports_addmatrix_over_otmb_op_add_matrix():
    from otmb_amd import capi

    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert "addmatrix!" in exported
    sig, body = _function("addmatrix!")
    assert sig == "D::DeviceOperator, B::SparseMatrixCSC{Float64,Int64}; alpha::Real = 1.0, slots::Union{Nothing,Integer,AbstractVector{<:Integer}} = nothing"
    assert "add_matrix_fn = sym(:otmb_op_add_matrix)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_add_matrix"]
    assert "the DeviceOperator has been released" in body
    ret, jargs, passed = _ccall(body, "add_matrix_fn")
    assert (ret, jargs) == header_prototypes()["otmb_op_add_matrix"]
    assert [k for t in capi.SYMBOLS["otmb_op_add_matrix"][1] for k in ctypes_kind(t)[:1]] == jargs
    assert passed == ["D.handle", "D.m", "D.n", "B.colptr", "B.rowval", "B.nzval", "Float64(alpha)", "nsel", "slots === nothing ? C_NULL : sel"]
    # slots are numbered from 1 here, from 0 in C; the sizes are compared before the call
    assert "Int64[s - 1 for s in slots]" in body and "size(B) == size(D) || throw(DimensionMismatch(" in body


def test_python_names_the_same_exports():
    import inspect

    from otmb_amd import api, operator_calls

    assert str(inspect.signature(api.buildTsink)) == "(*, w, gridmetrics, indices, seafloor='open', device=0)"
    assert str(inspect.signature(operator_calls.OperatorCalls.add_matrix)) == "(self, B, alpha=1.0, slots=None)"
    assert api.DeviceOperator.add_matrix is operator_calls.OperatorCalls.add_matrix
    src = inspect.getsource(operator_calls.OperatorCalls.add_matrix)
    assert '"otmb_op_add_matrix"' in src
    assert "otmb_build_sink(" in inspect.getsource(api.buildTsink)
