"""CPU, static (the Julia shim cannot be executed here): submatrix, D[I, J], takevalues!, sparse(D) and lines(D) are defined and exported,
and each makes ONE ccall of its export with the kinds and order of the header's prototype -- Julia's 1-based slots becoming the library's
0-based ones on the way."""
import re

from test_julia_shim_static import SHIM, _julia_function, header_prototypes, julia_kind, split_top

CALLS = {  # function -> the export it reaches
    "submatrix": "otmb_op_submatrix",
    "takevalues!": "otmb_op_take_values",
    "SparseArrays.sparse": "otmb_op_fetch",
    "lines": "otmb_op_get_lines",
}
CCALL = r"ccall\(\s*(\w+_fn)\s*,\s*(\w+)\s*,\s*\((.*?)\)\s*,"  # (through a pointer resolved under the lock: `x_fn = sym(:otmb_op_x)`, as the shim's other operator calls)


def _body(name):
    return _julia_function(re.escape(name))


def _calls(body):
    """[(export, return type, argument types)] of the ccalls in a function body, each pointer resolved to the symbol it was looked up as."""
    bound = dict(re.findall(r"(\w+_fn) = sym\(:(otmb_\w+)\)", body))
    assert "ccall(sym(" not in body
    return [(bound[fn], ret, args) for fn, ret, args in re.findall(CCALL, body, re.S)]


def test_the_five_functions_are_defined_and_exported():
    code = "\n".join(l.split("#")[0] for l in SHIM.splitlines())
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", code, re.M))))
    for name in ("submatrix", "takevalues!", "lines", "sparse"):
        assert name in exported, name
    for name in CALLS:
        assert re.search(r"^function " + re.escape(name) + r"\(", code, re.M), name
    # D[I, J] is Base.getindex (every module sees it), forwarding to submatrix
    assert re.search(r"^Base\.getindex\(D::DeviceOperator, I::AbstractVector\{<:Integer\}, J::AbstractVector\{<:Integer\}\) = submatrix\(D, I, J\)$", code, re.M)
    assert "function submatrix(D::DeviceOperator, I::AbstractVector{<:Integer}, J::AbstractVector{<:Integer} = I)" in code


def test_each_makes_one_ccall_with_the_headers_kinds_and_order():
    protos = header_prototypes()
    for fn, export in CALLS.items():
        body = _body(fn)
        calls = _calls(body)
        mine = [c for c in calls if c[0] == export]
        assert len(mine) == 1, (fn, [c[0] for c in calls])
        # nothing else of the feature is called from here: submatrix also asks otmb_op_info for the child's nnz, takevalues! otmb_op_slots for the
        # selected slot when none is named
        allowed = {"submatrix": {"otmb_op_info"}, "takevalues!": {"otmb_op_slots"}}.get(fn, set())
        assert {c[0] for c in calls} - {export} <= allowed, (fn, [c[0] for c in calls])
        for name, ret, args in calls:
            assert name in protos, name
            cret, cargs = protos[name]
            assert julia_kind(ret)[0] == cret == "i32", (fn, name)
            assert [k for a in split_top(args.replace("\n", " ")) for k in julia_kind(a)] == cargs, (fn, name, cargs)
        assert "lock(CALL_LOCK) do" in body and body.index("lock(CALL_LOCK) do") < body.index("ccall("), fn
        assert "handle == C_NULL" in body, fn


def test_slots_are_one_based_in_julia_and_the_argument_order_is_the_headers():
    tv = _body("takevalues!")
    assert "child.handle, parent.handle, Int64(ps - 1), Int64(s - 1))" in tv  # (child, parent, parent_slot, child_slot)
    sp_ = _body("SparseArrays.sparse")
    assert "Int64(slot === nothing ? -1 : slot - 1), colptr, rowval, nzval)" in sp_
    assert "SparseMatrixCSC{Float64,Int64}(D.m, D.n, colptr, rowval, nzval)" in sp_
    sub = _body("submatrix")
    assert "D.handle, length(rows), rows, length(cols), cols, h))" in sub and "finalizer(S) do d" in sub
    ln = _body("lines")
    assert "D.handle, next, has))" in ln and "has[] == 0 ? nothing : next" in ln
