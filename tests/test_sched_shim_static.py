"""Static check of the schedule in julia/OceanTransportMatrixBuilderAMD.jl (no Julia toolchain in the build image): stepsched! and
periodicsched! make ONE ccall each, of otmb_op_step_sched / otmb_op_periodic_sched, with the header's argument kinds and order -- the
array of block pointers as Ptr{Ptr{Float64}} -- and carry the keywords substeps and sourcescale; a vector of source blocks dispatches
periodic! to the scheduled call; header, ctypes mirror and exports agree.  The methods there were keep their text: their own static tests
(tests/test_step_shim_static.py and the others) pass unchanged."""
import re

from operator_calls_rec import header_names
from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes, julia_kind, split_top
from test_solve_shim_static import CODE, _jl
from test_step_shim_static import _ccall

STEP_DK = ["op", "adjoint", "k", "D", "ldd", "dt", "theta", "nsteps", "first_slot", "S", "lds", "X", "ldx", "rtol", "maxiter", "precond", "steps_done", "iters",
           "relres", "reason", "q", "W", "ldw", "obs", "tw", "Xbar", "ldm"]
PERIODIC_DK = ["op", "adjoint", "k", "D", "ldd", "dt", "theta", "ncycle", "first_slot", "S", "lds", "X", "ldx", "use_x0", "rtol", "maxiter", "precond", "ptol",
               "restart", "maxcycles", "cycles", "defect", "reason", "outer", "msolve_iters"]


def _with_schedule(names, scale):
    at = names.index("S")
    return names[:at] + ["substeps", "nsrc", "S", "lds"] + (["scale"] if scale else []) + names[at + 2:]


def test_header_and_mirror_declare_the_scheduled_calls_as_the_per_column_calls_with_a_schedule():
    from otmb_amd import capi

    protos = header_prototypes()
    assert header_names("otmb_op_step_dk") == STEP_DK and header_names("otmb_op_periodic_dk") == PERIODIC_DK
    for base, new, scale in (("otmb_op_step_dk", "otmb_op_step_sched", True), ("otmb_op_periodic_dk", "otmb_op_periodic_sched", False)):
        for suffix in ("", "_dev"):
            assert header_names(new + suffix) == _with_schedule(header_names(base), scale), new + suffix
            ret, kinds = protos[base + suffix]
            at = header_names(base).index("S")
            want = kinds[:at] + ["i64", "i64", "ptr", "i64"] + (["ptr"] if scale else []) + kinds[at + 2:]
            assert protos[new + suffix] == (ret, want), new + suffix
            res, argtypes = capi.SYMBOLS[new + suffix]
            assert ctypes_kind(res) == [ret] and [k for t in argtypes for k in ctypes_kind(t)[:1]] == want, new + suffix
    # flat arguments, the blocks as an array of pointers
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert len(re.findall(r"int64_t substeps, int64_t nsrc, const double \*const \*S, int64_t lds", text)) == 4


def test_the_shim_calls_the_scheduled_exports_with_the_headers_kinds_and_order():
    protos = header_prototypes()
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"stepsched!", "periodicsched!"} <= exported
    body, ret, jargs, passed = _ccall("stepsched!", "step_sched_fn")
    assert "step_sched_fn = sym(:otmb_op_step_sched)" in body and re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_slots", "otmb_op_step_sched"]
    assert (ret, jargs) == protos["otmb_op_step_sched"]
    assert passed == ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "ldd", "Float64(dt)", "Float64(θ)", "Int64(nsteps)", "Int64(firstslot - 1)",
                      "Int64(substeps)", "Int64(length(ptrs))", "isempty(ptrs) ? C_NULL : ptrs", "lds", "scale === nothing ? C_NULL : scale", "X", "ldx",
                      "Float64(rtol)", "Int64(maxiter)", "pc", "done", "iters", "relres", "reason", "Int64(q)", "observers === nothing ? C_NULL : observers", "ldw",
                      "observers === nothing ? C_NULL : obs", "timeweights === nothing ? C_NULL : timeweights", "Xbar === nothing ? C_NULL : Xbar", "ldm"]
    assert len(passed) == len(header_names("otmb_op_step_sched"))
    assert "Ptr{Ptr{Float64}}" in body and "GC.@preserve blocks" in body
    body, ret, jargs, passed = _ccall("periodicsched!", "periodic_sched_fn")
    assert re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_slots", "otmb_op_periodic_sched"]
    assert (ret, jargs) == protos["otmb_op_periodic_sched"]
    assert passed == ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "ldd", "Float64(dt)", "Float64(θ)", "Int64(ncycle)", "Int64(firstslot - 1)",
                      "Int64(substeps)", "Int64(length(ptrs))", "ptrs", "lds", "X", "ldx", "Int32(x0)", "Float64(rtol)", "Int64(maxiter)", "pc", "Float64(ptol)",
                      "Int64(restart)", "Int64(maxcycles)", "cycles", "defect", "reason", "oc", "msolve"]
    assert "Ptr{Ptr{Float64}}" in body and "GC.@preserve blocks" in body and "oc = outercode(outer)" in body


def test_the_keywords_and_the_vector_of_sources():
    head = re.search(r"\nfunction stepsched!\((.*?)\)\n    pc = precondcode", SHIM, re.S).group(1)
    for kw in ("substeps::Integer = 1", "sourcescale::Union{Nothing,StridedVecOrMat{Float64}} = nothing", "θ::Real = 1.0, nsteps::Integer = 1",
               "source::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing",
               "d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing", "observers::", "timeweights::"):
        assert kw in head, kw
    head = re.search(r"\nfunction periodicsched!\((.*?)\)\n    oc = outercode", SHIM, re.S).group(1)
    for kw in ("source::Union{StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}}", "substeps::Integer = 1", "outer::Symbol = :none",
               "d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing", "x0::Bool = false"):
        assert kw in head, kw
    assert "sourcescale" not in head  # a history is not periodic
    # a vector of blocks is a schedule by itself: periodic!'s positional source dispatches on it, with and without a matrix d
    assert re.search(r"^periodic!\(X::StridedVecOrMat\{Float64\}, D::Union\{DeviceOperator,AdjointDeviceOperator\}, "
                     r"source::AbstractVector\{<:StridedVecOrMat\{Float64\}\};\n\s+kwargs\.\.\.\) = periodicsched!\(X, D, source; kwargs\.\.\.\)", CODE, re.M)
    assert re.search(r"source::AbstractVector\{<:StridedVecOrMat\{Float64\}\},\n\s+d::StridedMatrix\{Float64\}; kwargs\.\.\.\) = periodicsched!\(X, D, source; d = d, "
                     r"kwargs\.\.\.\)", CODE)
    # the blocks: one or one per slot, X's shape, one leading dimension; the scale is k x nsteps in memory, entry t·k + c
    src = _jl("schedsources")
    assert "length(blocks) in (1, nslots) || throw(DimensionMismatch(" in src and "size(S) == size(X) || throw(DimensionMismatch(" in src
    assert "Ptr{Float64}[pointer(S) for S in blocks]" in src
    assert "(X isa AbstractVector ? (nrep,) : (k, nrep))" in _jl("stepsched!")
    # the methods there were still make their own calls
    for fn, sym in (("step!", "otmb_op_step"), ("stepobserve!", "otmb_op_step_obs"), ("periodic!", "otmb_op_periodic")):
        assert re.findall(r"sym\(:(otmb_\w+)\)", _jl(fn)) == [sym], fn
