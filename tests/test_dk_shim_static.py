"""CPU: the per-column exports (otmb_op_solve_dk, otmb_op_precond_dk, otmb_op_step_dk, otmb_op_periodic_dk and the _dev variants) have the
same types in the same order in the C prototypes (include/otmb.h), the ctypes mirror and the Julia shim's ccalls; each is its family's
existing export with `d` replaced by `D, ldd`; the shim's new methods take d as a matrix in the last positional place, call the _dk exports
in the header's argument order and pass stride(d, 2); and the existing methods keep their own ccalls."""
import re

from test_julia_shim_static import SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_solve_shim_static import _header_names

FAMILIES = {"otmb_op_solve_dk": "otmb_op_solve_pc", "otmb_op_precond_dk": "otmb_op_precond", "otmb_op_step_dk": "otmb_op_step_obs",
            "otmb_op_periodic_dk": "otmb_op_periodic_pc"}


def test_header_and_mirror():
    from otmb_amd import capi

    protos = header_prototypes()
    for new, old in FAMILIES.items():
        for suffix in ("", "_dev"):
            ret, args = protos[new + suffix]
            res, argtypes = capi.SYMBOLS[new + suffix]
            assert ctypes_kind(res) == [ret] == ["i32"], new
            assert [k for t in argtypes for k in ctypes_kind(t)[:1]] == args, new
            names, was = _header_names(new + suffix), _header_names(old + suffix)
            at = was.index("d")
            assert names == was[:at] + ["D", "ldd"] + was[at + 1:], (new, names)
            assert args == protos[old + suffix][1][:at] + ["ptr", "i64"] + protos[old + suffix][1][at + 1:], new
        assert protos[new] == protos[new + "_dev"]


def _method_with_matrix_d(name):
    """The body of the shim's method of `name` whose last positional argument is d::StridedMatrix{Float64}."""
    m = re.search(r"\nfunction " + re.escape(name) + r"\(([^;]*?d::StridedMatrix\{Float64\});.*?\)\n(.*?)\nend\n", SHIM, re.S)
    assert m, name
    assert split_top(" ".join(m.group(1).split()))[-1] == "d::StridedMatrix{Float64}", name
    return m.group(2)


def _ccall(body, var):
    m = re.search(r"ccall\(" + var + r", (\w+), \((.*?)\),\s(.*?)\)\)?\n", body, re.S)
    assert m, var
    jargs = [k for a in split_top(m.group(2).replace("\n", " ")) for k in julia_kind(a)]
    passed = [" ".join(a.split()) for a in split_top(m.group(3).replace("\n", " "))]
    assert body.index("lock(CALL_LOCK) do") < body.index("ccall(") and "the DeviceOperator has been released" in body
    return julia_kind(m.group(1))[0], jargs, passed


def test_the_shims_new_methods_call_the_dk_exports_in_the_headers_order():
    from otmb_amd import capi
    from test_step_shim_static import _ccall as first_ccall

    protos = header_prototypes()
    # what the existing methods pass, with d replaced by the matrix and its column stride
    def with_ldd(passed):
        at = passed.index("d === nothing ? C_NULL : d")
        return passed[:at] + ["d", "ldd"] + passed[at + 1:]

    cases = [("solve!", "solve_dk_fn", "otmb_op_solve_dk", first_ccall("solve!", "solve_fn")[3]),
             ("precondition!", "precond_dk_fn", "otmb_op_precond_dk", first_ccall("precondition!", "precond_fn")[3]),
             ("stepobserve!", "step_dk_fn", "otmb_op_step_dk", first_ccall("stepobserve!", "step_obs_fn")[3]),
             ("periodic!", "periodic_dk_fn", "otmb_op_periodic_dk", first_ccall("periodicpc!", "periodic_pc_fn")[3])]
    for fn, var, sym, old_passed in cases:
        body = _method_with_matrix_d(fn)
        ret, jargs, passed = _ccall(body, var)
        assert f"{var} = sym(:{sym})" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == [sym], fn
        assert (ret, jargs) == protos[sym], fn
        assert [k for t in capi.SYMBOLS[sym][1] for k in ctypes_kind(t)[:1]] == jargs, fn
        assert passed == with_ldd(old_passed) and len(passed) == len(_header_names(sym)), (fn, passed)
        assert len(re.findall(r"\bccall\(", body)) == 1 and re.search(r"\bldd = dkdims\(op, d, \w+, \"\w+\"\)", body), fn
        if "rc =" in body:
            assert "rc == 19 || check(rc)" in body, fn
    # ldd is the matrix's column stride, and d has the state's shape
    dims = re.search(r"\nfunction dkdims\(op::DeviceOperator, d::StridedMatrix\{Float64\}, X, xname\)\n(.*?)\nend\n", SHIM, re.S).group(1)
    assert "return Int64(stride(d, 2))" in dims and "size(d) == size(X)" in dims and "stride(d, 1) == 1" in dims and "DimensionMismatch" in dims
    # the plain step is the observed one; the periodic method takes outer itself
    assert re.search(r"^step!\(X::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}, d::StridedMatrix\{Float64\}; kwargs\.\.\.\) = "
                     r"stepobserve!\(X, D, d; kwargs\.\.\.\)", SHIM, re.M)
    assert "oc = outercode(outer)" in _method_with_matrix_d("periodic!")


def test_the_existing_methods_keep_their_own_ccalls():
    from test_solve_shim_static import _jl

    for fn, sym in (("solve!", "otmb_op_solve_pc"), ("precondition!", "otmb_op_precond"), ("step!", "otmb_op_step"), ("stepobserve!", "otmb_op_step_obs"),
                    ("periodic!", "otmb_op_periodic"), ("periodicpc!", "otmb_op_periodic_pc")):
        assert re.findall(r"sym\(:(otmb_\w+)\)", _jl(fn)) == [sym], fn
