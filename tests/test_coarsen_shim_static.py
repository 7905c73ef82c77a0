"""CPU: the Julia shim defines and exports `coarsen`, and calls the library in the same order as api.coarsen (which the GPU
tests execute): plan, the result arrays, fetch."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = open(os.path.join(ROOT, "julia", "OceanTransportMatrixBuilderAMD.jl"), encoding="utf-8").read()
API = open(os.path.join(ROOT, "oceantransportmatrixbuilder.jl_amd", "api.py"), encoding="utf-8").read()


def _body(src, pattern):
    m = re.search(pattern, src, re.S)
    assert m, pattern
    return m.group(1)


def test_shim_defines_and_exports_coarsen():
    code = "\n".join(l.split("#")[0] for l in SHIM.splitlines())
    exported = set(re.findall(r"\b(\w+)\b", " ".join(re.findall(r"^export (.*)$", code, re.M))))
    assert "coarsen" in exported
    assert re.search(r"^function coarsen\(LUMP::SparseMatrixCSC\{Float64,Int64\}, T::SparseMatrixCSC\{Float64,Int64\}, "
                     r"SPRAY::SparseMatrixCSC\{Float64,Int64\}\)", code, re.M)
    assert not re.search(r"Base\.\*|function \*\(|^\*\(", code, re.M)  # `*` stays SparseArrays' (no type piracy)


def test_shim_and_python_call_the_library_in_the_same_order():
    jl = _body(SHIM, r"\nfunction coarsen\(.*?\n(.*?)\nend\n")
    py = _body(API, r"\ndef coarsen\(.*?\n(.*?)(?=\ndef )")
    jl_syms = re.findall(r"sym\(:(otmb_\w+)\)", jl)
    py_syms = re.findall(r"lib\.(otmb_\w+)\(", py)
    assert jl_syms == py_syms == ["otmb_coarsen_plan", "otmb_coarsen_fetch"], (jl_syms, py_syms)
    # the result arrays are sized from the plan's nnz between the two calls, under the lock in Julia
    for body, alloc in ((jl, r"Vector\{Int64\}\(undef, k\[\]\)"), (py, r"np\.empty\(max\(k, 1\)")):
        p, a, f = body.index("otmb_coarsen_plan"), re.search(alloc, body).start(), body.index("otmb_coarsen_fetch")
        assert p < a < f
    assert "lock(CALL_LOCK)" in jl
