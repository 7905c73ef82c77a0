"""Static check of the interpolated calls in julia/OceanTransportMatrixBuilderAMD.jl (no Julia toolchain in the build image): stepinterp! and
periodicinterp! make ONE ccall each, of otmb_op_step_interp / otmb_op_periodic_interp, with the header's argument kinds and order -- slot_a,
slot_b and weight as Ptr{Int64}, Ptr{Int64}, Ptr{Float64} where the scheduled calls pass first_slot and substeps; interpschedule states the
convention's integer rule; header, ctypes mirror and exports agree.  The scheduled methods keep their text: tests/test_sched_shim_static.py
passes unchanged."""
import re

from operator_calls_rec import header_names
from test_julia_shim_static import HEADER, SHIM, ctypes_kind, header_prototypes
from test_solve_shim_static import CODE, _jl
from test_step_shim_static import _ccall


def _with_interp(names):
    at = names.index("first_slot")
    assert names[at:at + 2] == ["first_slot", "substeps"]
    return names[:at] + ["slot_a", "slot_b", "weight"] + names[at + 2:]


def test_header_and_mirror_declare_the_interpolated_calls_as_the_scheduled_calls_with_three_arrays():
    from otmb_amd import capi

    protos = header_prototypes()
    for base, new in (("otmb_op_step_sched", "otmb_op_step_interp"), ("otmb_op_periodic_sched", "otmb_op_periodic_interp")):
        for suffix in ("", "_dev"):
            assert header_names(new + suffix) == _with_interp(header_names(base + suffix)), new + suffix
            ret, kinds = protos[base + suffix]
            at = header_names(base).index("first_slot")
            want = kinds[:at] + ["ptr", "ptr", "ptr"] + kinds[at + 2:]
            assert protos[new + suffix] == (ret, want), new + suffix
            res, argtypes = capi.SYMBOLS[new + suffix]
            assert ctypes_kind(res) == [ret] and [k for t in argtypes for k in ctypes_kind(t)[:1]] == want, new + suffix
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert len(re.findall(r"const int64_t \*slot_a, const int64_t \*slot_b, const double \*weight, int64_t nsrc, const double \*const \*S, int64_t lds", text)) == 4
    # the contract's sentence of the schedule is replaced, and sources at sub-step resolution stay not built
    assert "Not built: interpolation of the matrices" not in HEADER and "Not built: sources at sub-step resolution" in HEADER


def test_the_shim_calls_the_interpolated_exports_with_the_headers_kinds_and_order():
    protos = header_prototypes()
    exported = set(re.findall(r"[\w!]+", " ".join(re.findall(r"^export (.*)$", CODE, re.M))))
    assert {"stepinterp!", "periodicinterp!", "interpschedule"} <= exported
    body, ret, jargs, passed = _ccall("stepinterp!", "step_interp_fn")
    assert re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_step_interp"]
    assert (ret, jargs) == protos["otmb_op_step_interp"]
    assert passed == ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "ldd", "Float64(dt)", "Float64(θ)", "nrep", "sa", "sb", "w",
                      "Int64(length(ptrs))", "isempty(ptrs) ? C_NULL : ptrs", "lds", "scale === nothing ? C_NULL : scale", "X", "ldx",
                      "Float64(rtol)", "Int64(maxiter)", "pc", "done", "iters", "relres", "reason", "Int64(q)", "observers === nothing ? C_NULL : observers", "ldw",
                      "observers === nothing ? C_NULL : obs", "timeweights === nothing ? C_NULL : timeweights", "Xbar === nothing ? C_NULL : Xbar", "ldm"]
    assert len(passed) == len(header_names("otmb_op_step_interp"))
    at = header_names("otmb_op_step_interp").index("slot_a")
    assert passed[at - 1:at + 3] == ["nrep", "sa", "sb", "w"] and "Ptr{Int64}, Ptr{Int64},\n                    Ptr{Float64}, Int64, Ptr{Ptr{Float64}}" in body
    assert "nrep = Int64(length(w))" in body and "sa, sb, w = interpargs(op, slota, slotb, weight, source)" in body and "GC.@preserve blocks" in body
    body, ret, jargs, passed = _ccall("periodicinterp!", "periodic_interp_fn")
    assert re.findall(r"sym\(:(otmb_\w+)\)", body) == ["otmb_op_periodic_interp"]
    assert (ret, jargs) == protos["otmb_op_periodic_interp"]
    assert passed == ["op.handle", "Int32(adjoint)", "k", "d === nothing ? C_NULL : d", "ldd", "Float64(dt)", "Float64(θ)", "Int64(length(w))", "sa", "sb", "w",
                      "Int64(length(ptrs))", "ptrs", "lds", "X", "ldx", "Int32(x0)", "Float64(rtol)", "Int64(maxiter)", "pc", "Float64(ptol)",
                      "Int64(restart)", "Int64(maxcycles)", "cycles", "defect", "reason", "oc", "msolve"]
    assert len(passed) == len(header_names("otmb_op_periodic_interp"))
    assert "oc = outercode(outer)" in body and "GC.@preserve blocks" in body


def test_the_keywords_the_arrays_and_the_convention():
    head = re.search(r"\nfunction stepinterp!\((.*?)\)\n    pc = precondcode", SHIM, re.S).group(1)
    for kw in ("slota::AbstractVector{<:Integer}", "slotb::AbstractVector{<:Integer}", "weight::AbstractVector{<:Real}", "θ::Real = 1.0",
               "source::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing",
               "sourcescale::Union{Nothing,StridedVecOrMat{Float64}} = nothing", "d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing",
               "observers::", "timeweights::"):
        assert kw in head, kw
    assert "nsteps" not in head and "firstslot" not in head and "substeps" not in head  # the schedule's length is the number of steps
    head = re.search(r"\nfunction periodicinterp!\((.*?)\)\n    oc = outercode", SHIM, re.S).group(1)
    for kw in ("source::Union{StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}}", "slota::AbstractVector{<:Integer}",
               "slotb::AbstractVector{<:Integer}", "weight::AbstractVector{<:Real}", "outer::Symbol = :none", "x0::Bool = false"):
        assert kw in head, kw
    assert "sourcescale" not in head and "ncycle" not in head  # a history is not periodic
    # the arrays: one length, finite weights in [0, 1], one source block at the most, Int64 / Int64 / Float64 and 0-based for the library
    src = _jl("interpargs")
    assert "length(slota) == length(slotb) == length(weight) ||" in src and "isfinite(w) && 0.0 <= w <= 1.0" in src
    assert "length(source) != 1 &&" in src and "Vector{Int64}(slota) .- 1, Vector{Int64}(slotb) .- 1, Vector{Float64}(weight)" in src
    # the convention, in integers and with one division
    src = _jl("interpschedule")
    for line in ("off = at === :start ? 0 : at === :mid ? 1 : 2", "g = 2t + off - m + 2m * nslots", "a = mod(firstslot - 1 + fld(g, 2m), nslots)",
                 "slota[t+1], slotb[t+1] = a + 1, mod(a + 1, nslots) + 1", "weight[t+1] = Float64(mod(g, 2m)) / Float64(2m)",
                 "nsteps = Int64(ncycles) * nslots * m"):
        assert line in src, line
    # the scheduled methods still make their own calls
    for fn, sym in (("stepsched!", "otmb_op_step_sched"), ("periodicsched!", "otmb_op_periodic_sched")):
        assert re.findall(r"sym\(:(otmb_\w+)\)", _jl(fn)) == ["otmb_op_slots", sym], fn
