"""Static check of the season calls in julia/OceanTransportMatrixBuilderAMD.jl (no Julia toolchain in the build image): stepseason! and
periodicseason! make ONE ccall each, of otmb_op_step_season / otmb_op_periodic_season, with the header's argument kinds and order -- nd, D,
ldd as Int64, Ptr{Ptr{Float64}}, Int64 where the interpolated calls pass D, ldd; plainschedule states the scheduled step's rule; header,
ctypes mirror and exports agree.  The interpolated methods keep their text: tests/test_interp_shim_static.py passes unchanged."""
import re

from operator_calls_rec import header_names
from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes
from test_solve_shim_static import CODE, _jl
from test_step_shim_static import _ccall


def _with_blocks(names):
    at = names.index("D")
    assert names[at:at + 2] == ["D", "ldd"]
    return names[:at] + ["nd", "D", "ldd"] + names[at + 2:]


def test_header_and_mirror_declare_the_season_calls_as_the_interpolated_calls_with_a_list_of_d():
    from otmb_amd import capi

    protos = header_prototypes()
    for base, new in (("otmb_op_step_interp", "otmb_op_step_season"), ("otmb_op_periodic_interp", "otmb_op_periodic_season")):
        for suffix in ("", "_dev"):
            assert header_names(new + suffix) == _with_blocks(header_names(base + suffix)), new + suffix
            ret, kinds = protos[base + suffix]
            at = header_names(base).index("D")
            want = kinds[:at] + ["i64", "ptr", "i64"] + kinds[at + 2:]
            assert protos[new + suffix] == (ret, want), new + suffix
            res, argtypes = capi.SYMBOLS[new + suffix]
            assert ctypes_kind(res) == [ret] and [k for t in argtypes for k in ctypes_kind(t)[:1]] == want, new + suffix
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert len(re.findall(r"int64_t nd, const double \*const \*D, int64_t ldd, double dt, double theta", text)) == 4
    # what is still not built is said where the calls are declared
    block = HEADER[HEADER.index("otmb_op_step_season[_dev] and otmb_op_periodic_season[_dev]"):]
    assert "Not built: a periodic scale, different matrices on the two sides of a θ-step, reuse of a blended preconditioner." in block


def test_the_shim_calls_the_season_exports_with_the_headers_kinds_and_order():
    protos = header_prototypes()
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"stepseason!", "periodicseason!", "plainschedule"} <= exported
    body, ret, jargs, passed = _ccall("stepseason!", "step_season_fn")
    assert re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_step_season"] and body.count("ccall(") == 1
    assert (ret, jargs) == protos["otmb_op_step_season"]
    assert passed == ["op.handle", "Int32(adjoint)", "k", "Int64(length(dptrs))", "isempty(dptrs) ? C_NULL : dptrs", "ldd", "Float64(dt)", "Float64(θ)", "nrep",
                      "sa", "sb", "w", "Int64(length(ptrs))", "isempty(ptrs) ? C_NULL : ptrs", "lds", "scale === nothing ? C_NULL : scale", "X", "ldx",
                      "Float64(rtol)", "Int64(maxiter)", "pc", "done", "iters", "relres", "reason", "Int64(q)", "observers === nothing ? C_NULL : observers", "ldw",
                      "observers === nothing ? C_NULL : obs", "timeweights === nothing ? C_NULL : timeweights", "Xbar === nothing ? C_NULL : Xbar", "ldm"]
    assert len(passed) == len(header_names("otmb_op_step_season"))
    at = header_names("otmb_op_step_season").index("nd")
    assert passed[at:at + 3] == ["Int64(length(dptrs))", "isempty(dptrs) ? C_NULL : dptrs", "ldd"] and "Int64, Int64, Ptr{Ptr{Float64}}, Int64, Float64" in body
    assert "nrep = Int64(length(w))" in body and "sa, sb, w = seasonargs(slota, slotb, weight)" in body and "GC.@preserve dblocks blocks" in body
    body, ret, jargs, passed = _ccall("periodicseason!", "periodic_season_fn")
    assert re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_periodic_season"] and body.count("ccall(") == 1
    assert (ret, jargs) == protos["otmb_op_periodic_season"]
    assert passed == ["op.handle", "Int32(adjoint)", "k", "Int64(length(dptrs))", "isempty(dptrs) ? C_NULL : dptrs", "ldd", "Float64(dt)", "Float64(θ)",
                      "Int64(length(w))", "sa", "sb", "w", "Int64(length(ptrs))", "ptrs", "lds", "X", "ldx", "Int32(x0)", "Float64(rtol)", "Int64(maxiter)", "pc",
                      "Float64(ptol)", "Int64(restart)", "Int64(maxcycles)", "cycles", "defect", "reason", "oc", "msolve"]
    assert len(passed) == len(header_names("otmb_op_periodic_season"))
    assert "oc = outercode(outer)" in body and "GC.@preserve dblocks blocks" in body


def test_the_keywords_the_blocks_and_the_plain_schedule():
    lists = "Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing"
    head = re.search(r"\nfunction stepseason!\((.*?)\)\n    pc = precondcode", SHIM, re.S).group(1)
    for kw in ("slota::AbstractVector{<:Integer}", "slotb::AbstractVector{<:Integer}", "weight::AbstractVector{<:Real}", "θ::Real = 1.0", "d::" + lists,
               "source::" + lists, "sourcescale::Union{Nothing,StridedVecOrMat{Float64}} = nothing", "observers::", "timeweights::"):
        assert kw in head, kw
    assert "nsteps" not in head and "firstslot" not in head and "substeps" not in head  # the schedule's length is the number of steps
    head = re.search(r"\nfunction periodicseason!\((.*?)\)\n    oc = outercode", SHIM, re.S).group(1)
    for kw in ("source::Union{StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}}", "slota::AbstractVector{<:Integer}", "d::" + lists,
               "outer::Symbol = :none", "x0::Bool = false"):
        assert kw in head, kw
    assert "sourcescale" not in head and "ncycle" not in head  # a history is not periodic
    # the blocks: one shape, contiguous columns, one leading dimension (0 for blocks of n values of d), nothing stacked
    src = _jl("seasonblocks")
    for line in ("all(size(B) == size(blocks[1]) for B in blocks) ||", "return Ptr{Float64}[pointer(B) for B in blocks], Int64(0), blocks",
                 "blocks = [ld(B) == max(op.n, 1) ? B : copy(B) for B in blocks]", "isempty(blocks) &&"):
        assert line in src, line
    src = _jl("seasonargs")
    assert "isfinite(w) && 0.0 <= w <= 1.0" in src and "Vector{Int64}(slota) .- 1, Vector{Int64}(slotb) .- 1, Vector{Float64}(weight)" in src
    assert "source blocks, expected 1" not in src  # a source per slot is in order here
    # the scheduled step's rule, 1-based like firstslot, every step plain
    src = _jl("plainschedule")
    for line in ("slota = Int64[mod(firstslot - 1 + fld(t, substeps), nslots) + 1 for t in 0:nsteps-1]", "return slota, copy(slota), zeros(Float64, nsteps)"):
        assert line in src, line
    # the interpolated methods still make their own calls
    for fn, sym in (("stepinterp!", "otmb_op_step_interp"), ("periodicinterp!", "otmb_op_periodic_interp")):
        assert re.findall(r"sym\(:(otmb_\w+)\)", _jl(fn)) == [sym], fn
