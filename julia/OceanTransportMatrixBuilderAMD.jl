# OceanTransportMatrixBuilderAMD.jl -- Julia host shim over libotmb_hip.so (include/otmb.h).
#
# Drop-in for the hot path of OceanTransportMatrixBuilder.jl v0.8.3: the same exported names, keyword
# arguments, return NamedTuples and error messages as the reference
#   makeindices                 src/matrixbuilding.jl:10-24
#   facefluxesfrommasstransport src/velocities.jl:118-130   (facefluxes :190-255, nofluxboundaries! :154-179)
#   transportmatrix             src/matrixbuilding.jl:128-150
#   velocity2fluxes / fluxes2velocity / facefluxesfromvelocities / interpolateontodefaultCgrid
#                               src/velocities.jl:10-74,140-151, src/gridcellgeometry.jl:103-140 (round 5: bound here too, so that a script
#                               that starts from uo / vo runs THIS module's facefluxes and not the reference's CPU one)
#   lump_and_spray              src/extratools.jl:38-119
#   coarsen                     LUMP * T * SPRAY (src/extratools.jl:14-16)
#   DeviceOperator, setvalues!  T * x, T' * v, mul!(Y, T, X, α, β) on the GPU (test/local_full.jl:96-107; README: ∂x/∂t + T x = …)
#   setslots!, step!, step      a year of monthly matrices resident as value slots, and θ-steps of the tracers through them on the GPU
#   periodic!, periodic         the periodic (cyclo-stationary) state of that stepped cycle, by restarted GMRES on the cycle map
#                               (outer = :mean: preconditioned by the cycle-mean operator)
#   combineslots!               a weighted sum of slots into a slot, on the device (the annual mean of the months)
#   solve!, solve               (σ·I + Diagonal(d) + T) \ B on the GPU: the `\` of the ideal-age problem (test/local_full.jl:151-188)
#   bolus_GM_velocity           src/RediGM.jl:46-79 (unexported and experimental there, unexported here)
#   makegridmetrics             src/gridcellgeometry.jl:265-311: the reference's own by default (its haversines are Julia's libm);
#                               `makegridmetrics(...; gpu = true)` opts into the library's array work (distances within 1e-12)
# Host-side decisions stay the reference's own functions (getgridtopology, vertexpermutation, getarakawagrid), so
# `using OceanTransportMatrixBuilderAMD` replaces `using OceanTransportMatrixBuilder` in a TMIP script.
#
# NOTE: no Julia toolchain exists in the build image, so this file has never been executed there; it is
# kept thin and mechanical (argument flattening + ccall) and mirrors the Python host layer
# oceantransportmatrixbuilder.jl_amd/api.py, which IS exercised by the GPU test-suite through the same C entry points in the
# same order (tests/test_julia_shim_static.py checks struct, prototypes and the call sequences of both layers).
module OceanTransportMatrixBuilderAMD

using SparseArrays
using Libdl
import LinearAlgebra
import OceanTransportMatrixBuilder as OTMB

# the reference's exported names (src/OceanTransportMatrixBuilder.jl:31-36), every one of them defined in THIS module
export makegridmetrics, velocity2fluxes, fluxes2velocity, facefluxesfromvelocities
export makeindices, facefluxesfrommasstransport, facefluxes, transportmatrix, lump_and_spray, coarsen
export DeviceOperator, setvalues!
export solve!, solve
export setlines!, verticallines, precondition!
export setslots!, selectslot!, slots, step!   # (`step` extends Base.step for this module's operators: nothing to export)
export periodic!, periodic, combineslots!, addmatrix!
export observe, stepobserve!
export stepsched!, periodicsched!
export stepinterp!, periodicinterp!, interpschedule
export stepseason!, periodicseason!, plainschedule
export submatrix, takevalues!, lines, sparse   # (`sparse` is SparseArrays' own, extended here and passed on; `D[I, J]` extends Base.getindex)

const LIBPATH = get(ENV, "OTMB_HIP_LIB", joinpath(@__DIR__, "..", "oceantransportmatrixbuilder.jl_amd", "lib", "libotmb_hip.so"))
const lib = Ref{Ptr{Cvoid}}(C_NULL)
const ctx = Ref{Ptr{Cvoid}}(C_NULL)              # the single-GPU context: created by the first call that needs it (`context()`)
const host_free_fn = Ref{Ptr{Cvoid}}(C_NULL)     # otmb_host_free, resolved once: finalizers must not look symbols up
const op_destroy_fn = Ref{Ptr{Cvoid}}(C_NULL)    # otmb_op_destroy, likewise (DeviceOperator's finalizer)
const MGPU = Dict{Vector{Int32},Ptr{Cvoid}}()    # otmb_mgpu objects by device list (`devices = 0:7`)
# A context (and an otmb_mgpu) is "not shared between threads" (include/otmb.h): every public entry point of this module runs
# its C calls under this lock, so tasks on several Julia threads may call the module freely.  Finalizers never take it: the one
# C function they call (otmb_host_free) touches neither the context nor this lock (see `pinned_array`).
const CALL_LOCK = ReentrantLock()
# results in pinned host memory of the library (fast: the DMA writes them in place; the vectors cannot change length) or in
# ordinary Julia vectors (as the reference's: dropzeros!, resize!, T[i,j] = x on a new position all work); per call: `pinned = ...`
const PINNED_RESULTS = Ref(get(ENV, "OTMB_PINNED_RESULTS", "1") != "0")

function __init__()
    # one HIP runtime per process: load ROCm's before the library (AMDGPU.jl users already have it)
    Libdl.dlopen(get(ENV, "OTMB_HIP_RUNTIME", "/opt/rocm/lib/libamdhip64.so"), Libdl.RTLD_GLOBAL)
    lib[] = Libdl.dlopen(LIBPATH)
    host_free_fn[] = Libdl.dlsym(lib[], :otmb_host_free)
    op_destroy_fn[] = Libdl.dlsym(lib[], :otmb_op_destroy)
    # (no context yet: a caller that only ever passes `devices = 4:7` must not have one created on GPU 0 behind its back)
    # Julia runs atexit hooks BEFORE its final finalizer sweep: result arrays that are still alive are finalized AFTER this hook.
    # That is safe by construction: pinned blocks belong to a process-wide pool that no context owns (otmb_ctx_destroy frees none of
    # them) and otmb_host_free ignores its context argument -- the finalizers below pass C_NULL.
    atexit() do
        lock(CALL_LOCK) do
            for h in values(MGPU)
                ccall(Libdl.dlsym(lib[], :otmb_mgpu_destroy), Cvoid, (Ptr{Cvoid},), h)
            end
            empty!(MGPU)
            ctx[] == C_NULL || ccall(Libdl.dlsym(lib[], :otmb_ctx_destroy), Cvoid, (Ptr{Cvoid},), ctx[])
            ctx[] = C_NULL
        end
    end
end

sym(name) = Libdl.dlsym(lib[], name)

# the single-GPU context (ENV["OTMB_DEVICE"], default 0), created on first use -- always called under CALL_LOCK
function context()
    if ctx[] == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall(sym(:otmb_ctx_create), Int32, (Int32, Ptr{Ptr{Cvoid}}), parse(Int32, get(ENV, "OTMB_DEVICE", "0")), h)
        rc == 0 || error("otmb_ctx_create failed (status $rc): is a ROCm GPU visible?")
        ctx[] = h[]
    end
    return ctx[]
end

# OTMB_ERR_GIVEN_FOREIGN: an operator that was passed in is not what the library derives for this grid and κ, and the build that was asked
# (pipelined / multi-slab) cannot add it: transportmatrix falls back to the two-phase call, which can
struct GivenForeign <: Exception end

# status -> the reference's own exception types and texts (include/otmb.h, otmb_status)
function check(rc::Int32)
    rc == 0 && return
    rc == 17 && throw(GivenForeign())
    msg = unsafe_string(ccall(sym(:otmb_last_error), Cstring, (Ptr{Cvoid},), ctx[]))
    rc == 8 && throw(AssertionError(msg))      # velocities.jl:199-200
    rc == 11 && throw(ArgumentError(msg))
    rc == 16 && throw(ArgumentError("Adjacency / distance matrices must be symmetric"))  # Graphs.SimpleGraph, extratools.jl:72
    error(msg)                                 # ErrorException: "Tadv contains NaNs." etc.
end

function check_mgpu(mg::Ptr{Cvoid}, rc::Int32)
    rc == 0 && return
    rc == 17 && throw(GivenForeign())
    rc == 14 && throw(CapacityExceeded())
    msg = unsafe_string(ccall(sym(:otmb_mgpu_last_error), Cstring, (Ptr{Cvoid},), mg))
    rc == 8 && throw(AssertionError(msg))
    rc == 11 && throw(ArgumentError(msg))
    error(msg)
end

# the otmb_mgpu of a device list: created once, kept until exit.  All ids different (RCCL hand-offs over xGMI) or all equal.
function mgpu_of(devices)
    key = Int32[Int32(d) for d in devices]
    get!(MGPU, key) do
        h = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall(sym(:otmb_mgpu_create), Int32, (Int32, Ptr{Int32}, Ptr{Ptr{Cvoid}}), Int32(length(key)), key, h)
        rc == 0 || error("otmb_mgpu_create($(collect(devices))) failed (status $rc)")
        h[]
    end
end

topologykind(g) = g isa OTMB.BipolarGridTopology ? Int32(0) : g isa OTMB.TripolarGridTopology ? Int32(1) : Int32(2)

"""
    makeindices(v3D)

Same return as the reference (matrixbuilding.jl:23): `(; wet3D, L, Lwet, N, Lwet3D, C)`.
"""
function makeindices(v3D)
    v = Array{Float64,3}(v3D)
    nx, ny, nz = size(v)
    lwet3d = Array{Int64,3}(undef, nx, ny, nz)
    lwet = Vector{Int64}(undef, length(v))
    wet = Array{UInt8,3}(undef, nx, ny, nz)
    N = Ref{Int64}(0)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_makeindices), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{UInt8}, Ptr{Int64}),
            context(), v, nx, ny, nz, lwet3d, lwet, wet, N))
    end
    resize!(lwet, N[])
    wet3D = BitArray(wet .!= 0)
    Lwet3D = Array{Union{Int,Missing},3}(missing, nx, ny, nz)   # the reference's element type
    Lwet3D[lwet] .= 1:N[]
    return (; wet3D, L = LinearIndices((nx, ny, nz)), Lwet = lwet, N = N[], Lwet3D, C = CartesianIndices((nx, ny, nz)))
end

"""
    facefluxes(umo, vmo, gridmetrics, indices; FillValue, pinned, devices)

velocities.jl:190-255.  `umo`/`vmo` are not modified.  `devices = 0:7` (extension): depth slabs over several GPUs
(otmb_mgpu_facefluxes), the same six arrays bit for bit.
"""
function facefluxes(umo, vmo, gridmetrics, indices; FillValue, pinned = PINNED_RESULTS[], devices = nothing)
    is32 = eltype(umo) == Float32 && eltype(vmo) == Float32
    T = is32 ? Float32 : Float64
    u = Array{T,3}(umo); v = Array{T,3}(vmo)          # velocities.jl:125-126 happens on the device
    nx, ny, nz = size(u)
    wet = Array{UInt8,3}(indices.wet3D)
    lock(CALL_LOCK) do
        ϕ = [outarray(Float64, pinned, nx, ny, nz) for _ in 1:6]   # east west north south top bottom
        ptrs = [pointer(a) for a in ϕ]
        if devices === nothing
            GC.@preserve ϕ u v wet check(ccall(sym(:otmb_facefluxes), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{UInt8}, Float64, Int64, Int64, Int64, Int32, Ptr{Ptr{Float64}}),
                context(), u, v, Int32(is32), wet, Float64(FillValue), nx, ny, nz, topologykind(gridmetrics.gridtopology), ptrs))
        else
            mg = mgpu_of(devices)
            GC.@preserve ϕ u v wet check_mgpu(mg, ccall(sym(:otmb_mgpu_facefluxes), Int32,
                (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{UInt8}, Float64, Int64, Int64, Int64, Int32, Ptr{Ptr{Float64}}),
                mg, u, v, Int32(is32), wet, Float64(FillValue), nx, ny, nz, topologykind(gridmetrics.gridtopology), ptrs))
        end
        return (east = ϕ[1], west = ϕ[2], north = ϕ[3], south = ϕ[4], top = ϕ[5], bottom = ϕ[6])
    end
end

function facefluxesfrommasstransport(; umo, vmo, gridmetrics, indices, pinned = PINNED_RESULTS[], devices = nothing)
    FillValue = umo.properties["_FillValue"]
    @assert isequal(FillValue, vmo.properties["_FillValue"])     # velocities.jl:121
    return facefluxes(umo, vmo, gridmetrics, indices; FillValue, pinned, devices)
end

# mirror of otmb_csc (include/otmb.h): a SparseMatrixCSC{Float64,Int64} by its three vectors
struct Csc
    colptr::Ptr{Int64}; rowval::Ptr{Int64}; nzval::Ptr{Float64}
    nnz::Int64
end
const NOCSC = Csc(C_NULL, C_NULL, C_NULL, 0)

# mirror of otmb_tm_args (include/otmb.h); isbits, passed by reference
struct TmArgs
    nx::Int64; ny::Int64; nz::Int64
    topology::Int32; upwind::Int32
    n_wet::Int64
    phi::NTuple{6,Ptr{Float64}}
    v3d::Ptr{Float64}; thkcello::Ptr{Float64}
    rho::Ptr{Float64}; rho_scalar::Float64
    lwet3d::Ptr{Int64}; lwet::Ptr{Int64}
    edge_length::NTuple{4,Ptr{Float64}}
    dist_nbr::NTuple{4,Ptr{Float64}}
    area2d::Ptr{Float64}; zt::Ptr{Float64}; mlotst::Ptr{Float64}
    kappa_h::Float64; kappa_vml::Float64; kappa_vdeep::Float64
    push_mask::Ptr{UInt16}        # device-resident callers only; C_NULL here (host arrays)
    only_t::Int32                 # extension: 1 = materialise T alone
    ignore_ops::Int32             # bit m: nothing operator m alone would raise is raised
    skip_ops::Int32               # bit m: matrix m is not wanted -- neither counted, written nor copied home (buildT*)
    given::NTuple{5,Csc}          # operators the caller passes (Tadv = / TκH = / TκVML = / TκVdeep = keywords): not built, added as they are
    kept_ops::Int32               # _dev entry points only (device output sets); always 0 here
end

# Output arrays in pinned host memory of the library (otmb_host_alloc): the DMA writes them in place -- no staging copy, no page
# faults on a gigabyte of fresh vectors -- and the block goes back to the library's pool when Julia collects the array.
# Lifetime by construction: the finalizer calls otmb_host_free with a NULL context through a function pointer resolved at load
# time.  otmb_host_free takes the pool's own lock and nothing else, never dereferences a context, and the pool is never torn
# down -- so the finalizer may run on any thread (julia -t N: whichever thread triggers the collector), while a ccall on the
# context is in flight, and after the atexit hook has destroyed the context.
# What a wrapped vector cannot do is change its length: dropzeros!(T), resize!, and T[i,j] = x at a position that is not stored
# throw where the reference's ordinary vectors work -- `pinned = false` (or ENV["OTMB_PINNED_RESULTS"] = "0") returns ordinary
# Julia vectors instead (the library then stages the copy through its own pinned ring; about a third slower at 1 degree).
# a pinned block of `n` elements that is not a Julia array yet (the one-phase build learns its lengths from the call) ...
function pinned_block(::Type{T}, n) where {T}
    p = Ref{Ptr{Cvoid}}(C_NULL)
    # (NULL context: the pool belongs to no context, and the `devices = ...` path must not create the single-GPU one)
    rc = ccall(sym(:otmb_host_alloc), Int32, (Ptr{Cvoid}, Int64, Ptr{Ptr{Cvoid}}), C_NULL, Int64(max(n, 1) * sizeof(T)), p)
    rc == 0 || error("otmb_host_alloc failed (status $rc)")
    return p[]
end
# ... and the array over its first elements that owns the block from here on: ONE Julia array per block, whose finalizer returns it
function adopt(::Type{T}, block::Ptr{Cvoid}, dims...) where {T}
    a = unsafe_wrap(Array, Ptr{T}(block), dims; own = false)
    finalizer(_ -> ccall(host_free_fn[], Int32, (Ptr{Cvoid}, Ptr{Cvoid}), C_NULL, block), a)
    return a
end
pinned_array(::Type{T}, dims...) where {T} = adopt(T, pinned_block(T, prod(dims)), dims...)
outarray(::Type{T}, usepinned::Bool, dims...) where {T} = usepinned ? pinned_array(T, dims...) : Array{T}(undef, dims...)

# A + B with the library's `+` (otmb_spadd: SparseArrays' map(+): union pattern, exact-zero sums dropped, :147)
function spadd(A::SparseMatrixCSC{Float64,Int64}, B::SparseMatrixCSC{Float64,Int64})
    n = size(A, 2)
    cap = max(1, nnz(A) + nnz(B))
    Cp = Vector{Int64}(undef, n + 1); Ci = Vector{Int64}(undef, cap); Cx = Vector{Float64}(undef, cap)
    k = Ref{Int64}(0)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_spadd), Int32,
            (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
            context(), n, A.colptr, A.rowval, A.nzval, B.colptr, B.rowval, B.nzval, Cp, Ci, Cx, k))
    end
    resize!(Ci, k[]); resize!(Cx, k[])
    return SparseMatrixCSC{Float64,Int64}(size(A, 1), n, Cp, Ci, Cx)
end

# The coarse operator `LUMP * T * SPRAY` of lump_and_spray's docstring (src/extratools.jl:14-16, test/local_full.jl:161) on the
# device: bit for bit SparseArrays' (LUMP * T) * SPRAY (otmb_coarsen_plan / otmb_coarsen_fetch).  `Base.*` stays SparseArrays'.
function coarsen(LUMP::SparseMatrixCSC{Float64,Int64}, T::SparseMatrixCSC{Float64,Int64}, SPRAY::SparseMatrixCSC{Float64,Int64})
    m, N = size(LUMP)
    M, n = size(T, 2), size(SPRAY, 2)
    (size(T, 1) == N && size(SPRAY, 1) == M) ||
        throw(DimensionMismatch("LUMP $(size(LUMP)), T $(size(T)), SPRAY $(size(SPRAY))"))
    k = Ref{Int64}(0)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_coarsen_plan), Int32,
            (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
            context(), m, N, LUMP.colptr, LUMP.rowval, LUMP.nzval, M, T.colptr, T.rowval, T.nzval, n, SPRAY.colptr, SPRAY.rowval, SPRAY.nzval, k))
        Cp = Vector{Int64}(undef, n + 1); Ci = Vector{Int64}(undef, k[]); Cx = Vector{Float64}(undef, k[])
        check(ccall(sym(:otmb_coarsen_fetch), Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}), ctx[], Cp, Ci, Cx))
        return SparseMatrixCSC{Float64,Int64}(m, n, Cp, Ci, Cx)
    end
end

# A sparse operator resident on the GPU (otmb_op_*): `mul!(Y, D, X, α, β)`, `mul!(Y, D', X, α, β)`, `D * x`, `D' * v` bit for bit
# SparseArrays' 5-argument mul! of Julia 1.10 (the β step first, then one fold per output element in storage order, no FMA), for the
# reference's consumer checks (test/local_full.jl:96-107: norm(T * e1), norm(T' * v)) and tracer stepping.  The operator owns device
# copies of the matrix (A may change or go once the constructor returns); `setvalues!` gives it new nzval for the same pattern.  Methods
# are defined for this module's own types only: `*` and `mul!` on a SparseMatrixCSC stay SparseArrays'.
mutable struct DeviceOperator
    handle::Ptr{Cvoid}
    m::Int64
    n::Int64
    nnz::Int64
end
struct AdjointDeviceOperator
    parent::DeviceOperator
end
Base.adjoint(D::DeviceOperator) = AdjointDeviceOperator(D)
Base.adjoint(A::AdjointDeviceOperator) = A.parent
Base.size(D::DeviceOperator) = (D.m, D.n)
Base.size(A::AdjointDeviceOperator) = (A.parent.n, A.parent.m)
# (not AbstractArrays: Base has no size(x, d) for them, so the operators get their own, with an AbstractArray's trailing 1s)
Base.size(D::Union{DeviceOperator,AdjointDeviceOperator}, d::Integer) = d < 1 ? throw(ArgumentError("dimension $d out of range")) :
    d <= 2 ? size(D)[d] : 1
SparseArrays.nnz(D::DeviceOperator) = D.nnz

function DeviceOperator(A::SparseMatrixCSC{Float64,Int64})
    m, n = size(A)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_op_create), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Ptr{Cvoid}}),
            context(), m, n, A.colptr, A.rowval, A.nzval, h))
    end
    D = DeviceOperator(h[], m, n, nnz(A))
    finalizer(D) do d
        release!(d)
    end
    return D
end

# DeviceOperator's finalizer.  otmb_op_destroy touches no context (safe after the atexit hook destroyed it) and is called through a
# pointer resolved in __init__.  A finalizer must not wait for a lock (no task switch inside the collector): when a call holds the
# module's lock, the finalizer is registered again and runs at a later collection.
function release!(D::DeviceOperator)
    D.handle == C_NULL && return nothing
    if trylock(CALL_LOCK)
        try
            ccall(op_destroy_fn[], Cvoid, (Ptr{Cvoid},), D.handle)
            D.handle = C_NULL
        finally
            unlock(CALL_LOCK)
        end
    else
        finalizer(D) do d
            release!(d)
        end
    end
    return nothing
end

function opmul!(Y::StridedVecOrMat{Float64}, D::DeviceOperator, adjoint::Bool, X::StridedVecOrMat{Float64}, α::Number, β::Number)
    rx, ry = adjoint ? (D.m, D.n) : (D.n, D.m)
    (size(X, 1) == rx && size(Y, 1) == ry && size(X, 2) == size(Y, 2)) ||
        throw(DimensionMismatch("$(adjoint ? "A'" : "A") of $((ry, rx)), X $(size(X)), Y $(size(Y))"))
    (stride(X, 1) == 1 && stride(Y, 1) == 1) || throw(ArgumentError("X and Y need contiguous columns"))
    k = size(X, 2)
    ldx = X isa AbstractVector || k <= 1 ? max(rx, 1) : stride(X, 2)
    ldy = Y isa AbstractVector || k <= 1 ? max(ry, 1) : stride(Y, 2)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        check(ccall(sym(:otmb_op_mul), Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Float64, Float64),
            D.handle, Int32(adjoint), k, X, ldx, Y, ldy, Float64(α), Float64(β)))
    end
    return Y
end

LinearAlgebra.mul!(Y::StridedVecOrMat{Float64}, D::DeviceOperator, X::StridedVecOrMat{Float64}, α::Number, β::Number) = opmul!(Y, D, false, X, α, β)
LinearAlgebra.mul!(Y::StridedVecOrMat{Float64}, A::AdjointDeviceOperator, X::StridedVecOrMat{Float64}, α::Number, β::Number) =
    opmul!(Y, A.parent, true, X, α, β)
# `A * x` and `A' * v` are mul!(…, true, false): α = 1.0, β = 0.0
LinearAlgebra.mul!(Y::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, X::StridedVecOrMat{Float64}) =
    LinearAlgebra.mul!(Y, D, X, true, false)
Base.:*(D::Union{DeviceOperator,AdjointDeviceOperator}, X::StridedVecOrMat{Float64}) =
    LinearAlgebra.mul!(X isa AbstractVector ? Vector{Float64}(undef, size(D)[1]) : Matrix{Float64}(undef, size(D)[1], size(X, 2)), D, X, true, false)

# new nzval for the pattern the operator was made with (the library checks the length it is told)
function setvalues!(D::DeviceOperator, nzval::Vector{Float64})
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        check(ccall(sym(:otmb_op_set_values), Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64), D.handle, nzval, length(nzval)))
    end
    return D
end

# (σ·I + Diagonal(d) + A) \ B on the resident operator (otmb_op_solve_pc: preconditioned BiCGStab on the device; include/otmb.h states
# the method, the stop rules and what is deterministic) -- `D'` solves with Aᵀ.  X holds the start when `x0 = true` and the solution
# afterwards.  Returns (X, info): info.iterations, info.relres, info.reason (:converged, :maxiter, :breakdown, :nonfinite) and
# info.converged, one entry per column of B.  A column that does not converge is REPORTED, not thrown (status 19): X then holds its last
# iterate.  Argument errors throw ArgumentError; a zero or non-finite entry of the diagonal throws an ErrorException that names it.
const SOLVE_REASONS = (:converged, :maxiter, :breakdown, :nonfinite)   # otmb_solve_reason
# the checks and leading dimensions solve! (B, X) and precondition! (Y, Z) share: (k, ld of the input, ld of the result)
function systemdims(op::DeviceOperator, B, bname, X, xname, d)
    n = op.n
    (size(B, 1) == n && size(X, 1) == n && size(X, 2) == size(B, 2)) ||
        throw(DimensionMismatch("operator of $((op.m, op.n)), $bname $(size(B)), $xname $(size(X))"))
    (d === nothing || length(d) == n) || throw(DimensionMismatch("d has $(length(d)) values, expected $n"))
    (stride(X, 1) == 1 && stride(B, 1) == 1) || throw(ArgumentError("$xname and $bname need contiguous columns"))
    k = size(B, 2)
    ldb = B isa AbstractVector || k <= 1 ? max(n, 1) : stride(B, 2)
    ldx = X isa AbstractVector || k <= 1 ? max(n, 1) : stride(X, 2)
    return k, ldb, ldx
end
function solve!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, B::StridedVecOrMat{Float64};
                d::Union{Nothing,Vector{Float64}} = nothing, σ::Real = 0.0, rtol::Real = 1e-10, maxiter::Integer = 10000, x0::Bool = false,
                precond::Symbol = :jacobi)
    # precond = :lines (after setlines!): the water columns' tridiagonals instead of the diagonal
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldb, ldx = systemdims(op, B, "B", X, "X", d)
    iters = zeros(Int64, k)
    relres = zeros(Float64, k)
    reason = zeros(Int32, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        solve_fn = sym(:otmb_op_solve_pc)
        rc = ccall(solve_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Float64, Int64,
                Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int32),
            op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, Float64(σ), B, ldb, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter),
            iters, relres, reason, pc)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
    end
    why = [SOLVE_REASONS[r + 1] for r in reason]
    return X, (iterations = iters, relres = relres, reason = why, converged = why .== :converged)
end
solve(D::Union{DeviceOperator,AdjointDeviceOperator}, B::StridedVecOrMat{Float64}; kwargs...) =
    solve!(B isa AbstractVector ? zeros(Float64, size(B, 1)) : zeros(Float64, size(B, 1), size(B, 2)), D, B; kwargs...)

# The line preconditioner (include/otmb.h states its contract): P = the part of σ·I + Diagonal(d) + A on caller-given lines, solved by the
# Thomas recurrence.  `setlines!(D, next)`: next[i] is the successor of unknown i on its line or 0 (`nothing` clears the lines; they survive
# setvalues!); `verticallines(indices)` gives the water columns of a makeindices result; `solve!(...; precond = :lines)` then iterates with
# them, and `precondition!(Z, D, Y; ...)` applies P⁻¹ alone (for a Krylov method of the caller's own).
const PRECONDS = (jacobi = Int32(0), lines = Int32(1))   # otmb_precond
precondcode(p::Symbol) = haskey(PRECONDS, p) ? PRECONDS[p] : throw(ArgumentError("precond must be :jacobi or :lines, not :$p"))

function setlines!(D::DeviceOperator, next::Union{Nothing,Vector{Int64}})
    (next === nothing || length(next) == D.n) || throw(DimensionMismatch("next has $(length(next)) entries, expected $(D.n)"))
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        set_lines_fn = sym(:otmb_op_set_lines)
        check(ccall(set_lines_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}), D.handle, next === nothing ? C_NULL : next))
    end
    return D
end

function verticallines(indices)
    L = indices.Lwet3D
    next = zeros(Int64, indices.N)
    for k in 1:size(L, 3) - 1, j in axes(L, 2), i in axes(L, 1)
        a, b = L[i, j, k], L[i, j, k + 1]
        (ismissing(a) || ismissing(b) || a == 0 || b == 0) && continue
        next[a] = b
    end
    return next
end

function precondition!(Z::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, Y::StridedVecOrMat{Float64};
                       d::Union{Nothing,Vector{Float64}} = nothing, σ::Real = 0.0, precond::Symbol = :lines)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldy, ldz = systemdims(op, Y, "Y", Z, "Z", d)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        precond_fn = sym(:otmb_op_precond)
        check(ccall(precond_fn, Int32, (Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Float64}, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
            op.handle, Int32(adjoint), pc, k, d === nothing ? C_NULL : d, Float64(σ), Y, ldy, Z, ldz))
    end
    return Z
end

# Value slots (include/otmb.h): several value sets over the operator's one pattern, resident together -- the twelve monthly matrices of a
# climatological year.  Slots are numbered from 1 here (the C side counts from 0).  `setslots!(D, n)` grows (new slots are copies of the
# selected one) or shrinks; `setvalues!(D, nzval, slot)` fills one (the slot is positional: `setvalues!(D, nzval)` writes the selected slot);
# `selectslot!(D, slot)` is a pointer switch: `D * x`, `solve!` and `precondition!` read that slot afterwards; `slots(D)` = (n, selected).
function setslots!(D::DeviceOperator, nslots::Integer)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        set_slots_fn = sym(:otmb_op_set_slots)
        check(ccall(set_slots_fn, Int32, (Ptr{Cvoid}, Int64), D.handle, Int64(nslots)))
    end
    return D
end
function setvalues!(D::DeviceOperator, nzval::Vector{Float64}, slot::Integer)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        set_values_slot_fn = sym(:otmb_op_set_values_slot)
        check(ccall(set_values_slot_fn, Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Int64), D.handle, Int64(slot - 1), nzval, length(nzval)))
    end
    return D
end
function selectslot!(D::DeviceOperator, slot::Integer)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        select_slot_fn = sym(:otmb_op_select_slot)
        check(ccall(select_slot_fn, Int32, (Ptr{Cvoid}, Int64), D.handle, Int64(slot - 1)))
    end
    return D
end
# `combineslots!(D, w, dst)`: slot dst = Σ_s w[s]·(slot s) on the device (otmb_op_combine_slots; include/otmb.h states the fold) -- the
# annual mean of the months without downloading one.  w: one finite weight per slot (a zero weight leaves its slot out); dst may be a source.
function combineslots!(D::DeviceOperator, w::Vector{Float64}, dst::Integer)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        combine_slots_fn = sym(:otmb_op_combine_slots)
        nslots = Ref{Int64}(0)
        slots_fn = sym(:otmb_op_slots)
        check(ccall(slots_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), D.handle, nslots, C_NULL))
        length(w) == nslots[] || throw(DimensionMismatch("w has $(length(w)) weights, the operator $(nslots[]) slots"))
        check(ccall(combine_slots_fn, Int32, (Ptr{Cvoid}, Ptr{Float64}, Int64), D.handle, w, Int64(dst - 1)))
    end
    return D
end
# `addmatrix!(D, B; alpha = 1.0, slots = nothing)`: slot = slot + alpha·B in place (otmb_op_add_matrix; include/otmb.h states the contract) for a
# matrix B of D's size whose pattern lies inside D's -- `buildTsink`'s S added to a year of monthly T, or a diffusivity retuned without a
# rebuild (T is linear in κH: B = TκH, alpha = κ′/κ - 1).  slots: `nothing` (every slot), a slot or a vector of different slots, numbered from 1.
# Each stored entry of B goes to the first stored entry of D with its row and column; an entry D does not store throws (status 21, naming the
# first) and leaves every slot untouched; alpha == 0 checks the pattern and writes nothing.  A submatrix does not follow: `takevalues!`.
function addmatrix!(D::DeviceOperator, B::SparseMatrixCSC{Float64,Int64}; alpha::Real = 1.0, slots::Union{Nothing,Integer,AbstractVector{<:Integer}} = nothing)
    size(B) == size(D) || throw(DimensionMismatch("B is $(size(B)), the operator $(size(D))"))
    sel = slots === nothing ? Int64[] : Int64[s - 1 for s in slots]
    nsel = Int64(length(sel))
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        add_matrix_fn = sym(:otmb_op_add_matrix)
        check(ccall(add_matrix_fn, Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Float64, Int64, Ptr{Int64}),
            D.handle, D.m, D.n, B.colptr, B.rowval, B.nzval, Float64(alpha), nsel, slots === nothing ? C_NULL : sel))
    end
    return D
end
function slots(D::DeviceOperator)
    n = Ref{Int64}(0)
    sel = Ref{Int64}(0)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        slots_fn = sym(:otmb_op_slots)
        check(ccall(slots_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), D.handle, n, sel))
    end
    return (n[], sel[] + 1)
end

# The operator's domain (include/otmb.h states the contract).  `submatrix(D, I, J = I)`, also written `D[I, J]`: A[I, J] as a new DeviceOperator on
# the device -- I and J strictly ascending index vectors (or Bool masks), the result bit for bit the operator of SparseArrays' A[I, J] (stored
# order kept), with D's slots, each restricted, D's selection and, when J is I, D's lines restricted.  Permutations and repeated indices are not
# built: the library refuses them and names the first offending position.  `takevalues!(child, parent; slot, parentslot)`: slot `slot` of a
# submatrix (default: its selected slot) becomes slot `parentslot` (default: the same number) of the operator it was taken from, restricted --
# one launch on the device, the refresh after `setvalues!(parent, ...)`.  `sparse(D; slot)`: the operator's matrix back as a SparseMatrixCSC
# (slot: default the selected one).  `lines(D)`: `next` as `setlines!` took it, or `nothing`.
function submatrix(D::DeviceOperator, I::AbstractVector{<:Integer}, J::AbstractVector{<:Integer} = I)
    rows = I isa AbstractVector{Bool} ? Vector{Int64}(findall(I)) : Vector{Int64}(I)
    cols = J === I ? rows : J isa AbstractVector{Bool} ? Vector{Int64}(findall(J)) : Vector{Int64}(J)
    (I isa AbstractVector{Bool} && length(I) != D.m) && throw(DimensionMismatch("row mask of $(length(I)), the operator has $(D.m) rows"))
    (J isa AbstractVector{Bool} && length(J) != D.n) && throw(DimensionMismatch("column mask of $(length(J)), the operator has $(D.n) columns"))
    h = Ref{Ptr{Cvoid}}(C_NULL)
    z = Ref{Int64}(0)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        submatrix_fn = sym(:otmb_op_submatrix)
        info_fn = sym(:otmb_op_info)
        check(ccall(submatrix_fn, Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64, Ptr{Int64}, Ptr{Ptr{Cvoid}}),
            D.handle, length(rows), rows, length(cols), cols, h))
        check(ccall(info_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h[], C_NULL, C_NULL, z))
    end
    S = DeviceOperator(h[], length(rows), length(cols), z[])
    finalizer(S) do d
        release!(d)
    end
    return S
end
Base.getindex(D::DeviceOperator, I::AbstractVector{<:Integer}, J::AbstractVector{<:Integer}) = submatrix(D, I, J)

function takevalues!(child::DeviceOperator, parent::DeviceOperator; slot::Union{Nothing,Integer} = nothing, parentslot::Union{Nothing,Integer} = nothing)
    lock(CALL_LOCK) do
        (child.handle == C_NULL || parent.handle == C_NULL) && throw(ArgumentError("the DeviceOperator has been released"))
        s = slot
        if s === nothing
            sel = Ref{Int64}(0)
            slots_fn = sym(:otmb_op_slots)
            check(ccall(slots_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), child.handle, C_NULL, sel))
            s = sel[] + 1
        end
        ps = parentslot === nothing ? s : parentslot
        take_values_fn = sym(:otmb_op_take_values)
        check(ccall(take_values_fn, Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64), child.handle, parent.handle, Int64(ps - 1), Int64(s - 1)))
    end
    return child
end

function SparseArrays.sparse(D::DeviceOperator; slot::Union{Nothing,Integer} = nothing)
    (slot === nothing || slot >= 1) || throw(ArgumentError("slot must be >= 1"))
    colptr = Vector{Int64}(undef, D.n + 1)
    rowval = Vector{Int64}(undef, D.nnz)
    nzval = Vector{Float64}(undef, D.nnz)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        fetch_fn = sym(:otmb_op_fetch)
        check(ccall(fetch_fn, Int32, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}),
            D.handle, Int64(slot === nothing ? -1 : slot - 1), colptr, rowval, nzval))
    end
    return SparseMatrixCSC{Float64,Int64}(D.m, D.n, colptr, rowval, nzval)
end

function lines(D::DeviceOperator)
    next = Vector{Int64}(undef, D.n)
    has = Ref{Int32}(0)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        get_lines_fn = sym(:otmb_op_get_lines)
        check(ccall(get_lines_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}), D.handle, next, has))
    end
    return has[] == 0 ? nothing : next
end

# θ-steps of ∂x/∂t + (Diagonal(d) + A)·x = source through the slots (otmb_op_step; include/otmb.h states the contract): X is advanced in
# place through `nsteps` steps of length `dt`, step t = 0, 1, ... with slot firstslot + t (cyclically); `D'` steps with Aᵀ.  Returns
# (X, info): info.stepsdone and, per step that ran a solve (rows) and column, info.iterations, info.relres, info.reason, info.converged.
# A step that does not converge ends the call and is REPORTED, not thrown (status 19): X then holds that step's last iterates.
function step!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}; dt::Real, θ::Real = 1.0, nsteps::Integer = 1,
               firstslot::Integer = 1, source::Union{Nothing,StridedVecOrMat{Float64}} = nothing, d::Union{Nothing,Vector{Float64}} = nothing,
               rtol::Real = 1e-10, maxiter::Integer = 10000, precond::Symbol = :jacobi)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    S = source === nothing ? X : source
    k, lds, ldx = systemdims(op, S, "source", X, "X", d)
    nrep = max(Int64(nsteps), 0)
    iters = zeros(Int64, k, nrep)
    relres = zeros(Float64, k, nrep)
    reason = zeros(Int32, k, nrep)
    done = Ref{Int64}(0)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        step_fn = sym(:otmb_op_step)
        rc = ccall(step_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Float64, Float64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                Float64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
            op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, Float64(dt), Float64(θ), Int64(nsteps), Int64(firstslot - 1),
            source === nothing ? C_NULL : source, lds, X, ldx, Float64(rtol), Int64(maxiter), pc, done, iters, relres, reason)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which step and column stopped why
    end
    ran = 1:min(done[] + 1, nrep)
    why = permutedims([SOLVE_REASONS[r + 1] for r in reason[:, ran]])
    return X, (stepsdone = done[], iterations = permutedims(iters[:, ran]), relres = permutedims(relres[:, ran]), reason = why,
               converged = why .== :converged)
end
Base.step(D::Union{DeviceOperator,AdjointDeviceOperator}, X::StridedVecOrMat{Float64}; kwargs...) = step!(copy(X), D; kwargs...)

# Observers W (n x q, or n values: one observer) of an operator with n columns: (q, the leading dimension of W).
function observerdims(op::DeviceOperator, W)
    size(W, 1) == op.n || throw(DimensionMismatch("operator of $((op.m, op.n)), observers $(size(W))"))
    stride(W, 1) == 1 || throw(ArgumentError("the observers need contiguous columns"))
    q = size(W, 2)
    return q, (W isa AbstractVector || q <= 1 ? max(op.n, 1) : stride(W, 2))
end
# Wᵀ·X on the device (otmb_op_observe; include/otmb.h states the order of the sums): the inventory (W = the cell volumes), stations, regional
# means of the state X.  Returns a q x k matrix: entry (j, c) is observer j of tracer c.
function observe(D::DeviceOperator, W::StridedVecOrMat{Float64}, X::StridedVecOrMat{Float64})
    size(X, 1) == D.n || throw(DimensionMismatch("operator of $((D.m, D.n)), X $(size(X))"))
    stride(X, 1) == 1 || throw(ArgumentError("X needs contiguous columns"))
    k = size(X, 2)
    ldx = X isa AbstractVector || k <= 1 ? max(D.n, 1) : stride(X, 2)
    q, ldw = observerdims(D, W)
    obs = zeros(Float64, q, k)
    lock(CALL_LOCK) do
        D.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        observe_fn = sym(:otmb_op_observe)
        check(ccall(observe_fn, Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Ptr{Float64}),
            D.handle, k, q, W, ldw, X, ldx, obs))
    end
    return obs
end
# step! with a record along the way (otmb_op_step_obs): `observers` (n x q) are applied to the state after every completed step, and
# `timeweights` (nsteps values) fold the states into their weighted mean.  X is overwritten as by step!.  Returns (X, info): step!'s fields and
# info.observations (q x k x stepsdone: [j, c, t] is observer j of tracer c after step t; nothing without observers) and info.mean (n x k,
# Σ_t timeweights[t]·X_t over the completed steps; nothing without weights or when no step was completed).
function stepobserve!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}; dt::Real, θ::Real = 1.0, nsteps::Integer = 1,
                      firstslot::Integer = 1, source::Union{Nothing,StridedVecOrMat{Float64}} = nothing, d::Union{Nothing,Vector{Float64}} = nothing,
                      rtol::Real = 1e-10, maxiter::Integer = 10000, precond::Symbol = :jacobi,
                      observers::Union{Nothing,StridedVecOrMat{Float64}} = nothing, timeweights::Union{Nothing,Vector{Float64}} = nothing)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    S = source === nothing ? X : source
    k, lds, ldx = systemdims(op, S, "source", X, "X", d)
    nrep = max(Int64(nsteps), 0)
    iters = zeros(Int64, k, nrep)
    relres = zeros(Float64, k, nrep)
    reason = zeros(Int32, k, nrep)
    done = Ref{Int64}(0)
    q, ldw = observers === nothing ? (0, max(op.n, 1)) : observerdims(op, observers)
    obs = zeros(Float64, q, k, nrep)
    timeweights === nothing || length(timeweights) == nrep || throw(DimensionMismatch("timeweights of $(length(timeweights)), nsteps $nrep"))
    Xbar = timeweights === nothing ? nothing : zeros(Float64, size(X)...)
    ldm = max(op.n, 1)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        step_obs_fn = sym(:otmb_op_step_obs)
        rc = ccall(step_obs_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Float64, Float64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                Float64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Int64),
            op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, Float64(dt), Float64(θ), Int64(nsteps), Int64(firstslot - 1),
            source === nothing ? C_NULL : source, lds, X, ldx, Float64(rtol), Int64(maxiter), pc, done, iters, relres, reason,
            Int64(q), observers === nothing ? C_NULL : observers, ldw, observers === nothing ? C_NULL : obs,
            timeweights === nothing ? C_NULL : timeweights, Xbar === nothing ? C_NULL : Xbar, ldm)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which step and column stopped why
    end
    ran = 1:min(done[] + 1, nrep)
    why = permutedims([SOLVE_REASONS[r + 1] for r in reason[:, ran]])
    return X, (stepsdone = done[], iterations = permutedims(iters[:, ran]), relres = permutedims(relres[:, ran]), reason = why,
               converged = why .== :converged, observations = observers === nothing ? nothing : obs[:, :, 1:done[]],
               mean = done[] > 0 ? Xbar : nothing)
end

const PERIODIC_REASONS = (:converged, :maxcycles, :step_failed, :nonfinite)   # otmb_periodic_reason
# The periodic state of the stepped cycle (otmb_op_periodic; include/otmb.h states the method): X with F(X) = X, F = `ncycle` steps of length
# `dt` from slot `firstslot` with `source`, by restarted GMRES(restart) on the cycle map; `D'` cycles with Aᵀ.  X is overwritten with the state
# at the start of the cycle (x0 = true: X is the start; false: X is not read).  Returns (X, info): per column info.cycles, info.defect
# (‖F(x) - x‖₂ / ‖F(0)‖₂), info.reason, info.converged.  A column that does not converge is REPORTED, not thrown (status 19).
function periodic!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, source::StridedVecOrMat{Float64}; dt::Real,
                   ncycle::Integer, θ::Real = 1.0, firstslot::Integer = 1, d::Union{Nothing,Vector{Float64}} = nothing, x0::Bool = false,
                   rtol::Real = 1e-10, maxiter::Integer = 10000, precond::Symbol = :jacobi, outer::Symbol = :none, ptol::Real = 1e-8, restart::Integer = 30,
                   maxcycles::Integer = 1000)
    outer === :none || return periodicpc!(X, D, source, outercode(outer); dt = dt, ncycle = ncycle, θ = θ, firstslot = firstslot, d = d, x0 = x0,
                                          rtol = rtol, maxiter = maxiter, precond = precond, ptol = ptol, restart = restart, maxcycles = maxcycles)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, lds, ldx = systemdims(op, source, "source", X, "X", d)
    cycles = zeros(Int64, k)
    defect = zeros(Float64, k)
    reason = zeros(Int32, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        periodic_fn = sym(:otmb_op_periodic)
        rc = ccall(periodic_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Float64, Float64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                Int32, Float64, Int64, Int32, Float64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}),
            op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, Float64(dt), Float64(θ), Int64(ncycle), Int64(firstslot - 1),
            source, lds, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), pc, Float64(ptol), Int64(restart), Int64(maxcycles), cycles, defect, reason)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
    end
    why = [PERIODIC_REASONS[r + 1] for r in reason]
    return X, (cycles = cycles, defect = defect, reason = why, converged = why .== :converged, msolve_iters = zeros(Int64, k))
end
const PERIODIC_PC_REASONS = (PERIODIC_REASONS..., :precond_failed)   # ... continued by otmb_periodic_pc_reason
const OUTERS = (:none, :mean)                                       # otmb_outer
function outercode(outer::Symbol)
    i = findfirst(==(outer), OUTERS)
    i === nothing && throw(ArgumentError("outer must be one of $(OUTERS), not :$(outer)"))
    return Int32(i - 1)
end
# periodic! with `outer = :mean` (otmb_op_periodic_pc; include/otmb.h states the method): the outer GMRES is flexible and right-preconditioned
# by the cycle-mean operator -- fewer cycles, one solve with the mean matrix per iteration.  info.msolve_iters: the BiCGStab iterations a
# column spent in those solves; info.reason may be :precond_failed (a mean solve did not converge).
function periodicpc!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, source::StridedVecOrMat{Float64}, oc::Int32; dt::Real,
                     ncycle::Integer, θ::Real, firstslot::Integer, d::Union{Nothing,Vector{Float64}}, x0::Bool, rtol::Real, maxiter::Integer,
                     precond::Symbol, ptol::Real, restart::Integer, maxcycles::Integer)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, lds, ldx = systemdims(op, source, "source", X, "X", d)
    cycles = zeros(Int64, k)
    defect = zeros(Float64, k)
    reason = zeros(Int32, k)
    msolve = zeros(Int64, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        periodic_pc_fn = sym(:otmb_op_periodic_pc)
        rc = ccall(periodic_pc_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Float64, Float64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64,
                Int32, Float64, Int64, Int32, Float64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Int64}),
            op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, Float64(dt), Float64(θ), Int64(ncycle), Int64(firstslot - 1),
            source, lds, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), pc, Float64(ptol), Int64(restart), Int64(maxcycles), cycles, defect, reason,
            oc, msolve)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
    end
    why = [PERIODIC_PC_REASONS[r + 1] for r in reason]
    return X, (cycles = cycles, defect = defect, reason = why, converged = why .== :converged, msolve_iters = msolve)
end
periodic(D::Union{DeviceOperator,AdjointDeviceOperator}, source::StridedVecOrMat{Float64}; kwargs...) = periodic!(zero(source), D, source; kwargs...)

# Per-column d (otmb_op_solve_dk, otmb_op_precond_dk, otmb_op_step_dk, otmb_op_periodic_dk; include/otmb.h states the contract): tracers that
# differ in their sink -- ideal age, radiocarbon with its decay rate, a dye restored over its own patch -- in ONE call.  `d` is a matrix of
# the shape of B / X / source, passed as the last positional argument, one column per tracer; column c of the result has the bits of the call
# above made for that column alone with `d = d[:, c]`.  The keywords and the returned info are those of the methods above.
function dkdims(op::DeviceOperator, d::StridedMatrix{Float64}, X, xname)
    (X isa AbstractMatrix && size(d) == size(X)) || throw(DimensionMismatch("d $(size(d)) is per column, $xname $(size(X))"))
    stride(d, 1) == 1 || throw(ArgumentError("d needs contiguous columns"))
    return Int64(stride(d, 2))   # ldd: a view of some columns, or of the leading rows, of a larger matrix keeps its parent's
end
function solve!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, B::StridedVecOrMat{Float64}, d::StridedMatrix{Float64};
                σ::Real = 0.0, rtol::Real = 1e-10, maxiter::Integer = 10000, x0::Bool = false, precond::Symbol = :jacobi)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldb, ldx = systemdims(op, B, "B", X, "X", nothing)
    ldd = dkdims(op, d, X, "X")
    iters = zeros(Int64, k)
    relres = zeros(Float64, k)
    reason = zeros(Int32, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        solve_dk_fn = sym(:otmb_op_solve_dk)
        rc = ccall(solve_dk_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Float64,
                Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int32),
            op.handle, Int32(adjoint), k, d, ldd, Float64(σ), B, ldb, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), iters, relres, reason, pc)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
    end
    why = [SOLVE_REASONS[r + 1] for r in reason]
    return X, (iterations = iters, relres = relres, reason = why, converged = why .== :converged)
end
function precondition!(Z::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, Y::StridedVecOrMat{Float64},
                       d::StridedMatrix{Float64}; σ::Real = 0.0, precond::Symbol = :lines)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldy, ldz = systemdims(op, Y, "Y", Z, "Z", nothing)
    ldd = dkdims(op, d, Z, "Z")
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        precond_dk_fn = sym(:otmb_op_precond_dk)
        check(ccall(precond_dk_fn, Int32, (Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Float64}, Int64, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
            op.handle, Int32(adjoint), pc, k, d, ldd, Float64(σ), Y, ldy, Z, ldz))
    end
    return Z
end
function stepobserve!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, d::StridedMatrix{Float64}; dt::Real, θ::Real = 1.0,
                      nsteps::Integer = 1, firstslot::Integer = 1, source::Union{Nothing,StridedVecOrMat{Float64}} = nothing, rtol::Real = 1e-10,
                      maxiter::Integer = 10000, precond::Symbol = :jacobi, observers::Union{Nothing,StridedVecOrMat{Float64}} = nothing,
                      timeweights::Union{Nothing,Vector{Float64}} = nothing)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    S = source === nothing ? X : source
    k, lds, ldx = systemdims(op, S, "source", X, "X", nothing)
    ldd = dkdims(op, d, X, "X")
    nrep = max(Int64(nsteps), 0)
    iters = zeros(Int64, k, nrep)
    relres = zeros(Float64, k, nrep)
    reason = zeros(Int32, k, nrep)
    done = Ref{Int64}(0)
    q, ldw = observers === nothing ? (0, max(op.n, 1)) : observerdims(op, observers)
    obs = zeros(Float64, q, k, nrep)
    timeweights === nothing || length(timeweights) == nrep || throw(DimensionMismatch("timeweights of $(length(timeweights)), nsteps $nrep"))
    Xbar = timeweights === nothing ? nothing : zeros(Float64, size(X)...)
    ldm = max(op.n, 1)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        step_dk_fn = sym(:otmb_op_step_dk)
        rc = ccall(step_dk_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64},
                Int64, Float64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64},
                Ptr{Float64}, Int64),
            op.handle, Int32(adjoint), k, d, ldd, Float64(dt), Float64(θ), Int64(nsteps), Int64(firstslot - 1),
            source === nothing ? C_NULL : source, lds, X, ldx, Float64(rtol), Int64(maxiter), pc, done, iters, relres, reason,
            Int64(q), observers === nothing ? C_NULL : observers, ldw, observers === nothing ? C_NULL : obs,
            timeweights === nothing ? C_NULL : timeweights, Xbar === nothing ? C_NULL : Xbar, ldm)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which step and column stopped why
    end
    ran = 1:min(done[] + 1, nrep)
    why = permutedims([SOLVE_REASONS[r + 1] for r in reason[:, ran]])
    return X, (stepsdone = done[], iterations = permutedims(iters[:, ran]), relres = permutedims(relres[:, ran]), reason = why,
               converged = why .== :converged, observations = observers === nothing ? nothing : obs[:, :, 1:done[]],
               mean = done[] > 0 ? Xbar : nothing)
end
# (the plain step is the observed one without observers and weights: info.observations and info.mean are nothing)
step!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, d::StridedMatrix{Float64}; kwargs...) = stepobserve!(X, D, d; kwargs...)
function periodic!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, source::StridedVecOrMat{Float64},
                   d::StridedMatrix{Float64}; dt::Real, ncycle::Integer, θ::Real = 1.0, firstslot::Integer = 1, x0::Bool = false, rtol::Real = 1e-10,
                   maxiter::Integer = 10000, precond::Symbol = :jacobi, outer::Symbol = :none, ptol::Real = 1e-8, restart::Integer = 30,
                   maxcycles::Integer = 1000)
    oc = outercode(outer)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, lds, ldx = systemdims(op, source, "source", X, "X", nothing)
    ldd = dkdims(op, d, X, "X")
    cycles = zeros(Int64, k)
    defect = zeros(Float64, k)
    reason = zeros(Int32, k)
    msolve = zeros(Int64, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        periodic_dk_fn = sym(:otmb_op_periodic_dk)
        rc = ccall(periodic_dk_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Float64},
                Int64, Int32, Float64, Int64, Int32, Float64, Int64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Int64}),
            op.handle, Int32(adjoint), k, d, ldd, Float64(dt), Float64(θ), Int64(ncycle), Int64(firstslot - 1),
            source, lds, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), pc, Float64(ptol), Int64(restart), Int64(maxcycles), cycles, defect, reason,
            oc, msolve)
        rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
    end
    why = [PERIODIC_PC_REASONS[r + 1] for r in reason]
    return X, (cycles = cycles, defect = defect, reason = why, converged = why .== :converged, msolve_iters = msolve)
end

# A schedule for the time axis (otmb_op_step_sched, otmb_op_periodic_sched; include/otmb.h states the contract).  `substeps = m`: step t runs
# with slot firstslot + t ÷ m (cyclically) -- m implicit steps inside January before February begins, each slot's preconditioner made once.
# `source`: nothing, an array of X's shape, or a vector of such arrays, one (every step takes it) or one per slot (step t takes its slot's: a
# seasonal source); the blocks stay where they are, their addresses travel.  `sourcescale` (step only): nothing or a k x nsteps matrix (nsteps
# values for a vector X), entry [c, t] the factor of tracer c's source at step t: a fixed pattern times a history (CFC-11, SF6, bomb
# radiocarbon).  `d`: nothing, n values, or a matrix of X's shape (one d per tracer).  step!, stepobserve! and periodic! keep their methods:
# with substeps = 1, one array and no scale these calls give their bits.  The other keywords and the returned info are theirs.
function schedsources(op::DeviceOperator, source, X, nslots::Integer)
    source === nothing && return Ptr{Float64}[], Int64(max(op.n, 1)), ()
    blocks = source isa AbstractVector{<:StridedVecOrMat{Float64}} ? source : [source]
    length(blocks) in (1, nslots) || throw(DimensionMismatch("$(length(blocks)) source blocks, expected 1 or one per slot ($nslots)"))
    for S in blocks
        size(S) == size(X) || throw(DimensionMismatch("source $(size(S)), X $(size(X))"))
        stride(S, 1) == 1 || throw(ArgumentError("the source blocks need contiguous columns"))
    end
    ld(S) = Int64(S isa AbstractVector || size(S, 2) <= 1 ? max(op.n, 1) : stride(S, 2))
    if !all(ld(S) == ld(blocks[1]) for S in blocks)   # one lds for all: blocks whose leading dimensions differ are copied compactly
        blocks = [ld(S) == max(op.n, 1) ? S : copy(S) for S in blocks]
    end
    return Ptr{Float64}[pointer(S) for S in blocks], ld(blocks[1]), blocks
end
function scheddims(op::DeviceOperator, X, d)
    size(X, 1) == op.n == op.m || throw(DimensionMismatch("operator of $((op.m, op.n)), X $(size(X))"))
    stride(X, 1) == 1 || throw(ArgumentError("X needs contiguous columns"))
    k = Int64(size(X, 2))
    ldx = Int64(X isa AbstractVector || k <= 1 ? max(op.n, 1) : stride(X, 2))
    ldd = d isa AbstractMatrix ? dkdims(op, d, X, "X") : Int64(0)
    d isa AbstractVector && length(d) != op.n && throw(DimensionMismatch("d has $(length(d)) values, the operator $(op.n) columns"))
    return k, ldx, ldd
end
function stepsched!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}; dt::Real, θ::Real = 1.0, nsteps::Integer = 1,
                    firstslot::Integer = 1, substeps::Integer = 1,
                    source::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing,
                    sourcescale::Union{Nothing,StridedVecOrMat{Float64}} = nothing,
                    d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing, rtol::Real = 1e-10, maxiter::Integer = 10000,
                    precond::Symbol = :jacobi, observers::Union{Nothing,StridedVecOrMat{Float64}} = nothing,
                    timeweights::Union{Nothing,Vector{Float64}} = nothing)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldx, ldd = scheddims(op, X, d)
    nrep = max(Int64(nsteps), 0)
    iters = zeros(Int64, k, nrep)
    relres = zeros(Float64, k, nrep)
    reason = zeros(Int32, k, nrep)
    done = Ref{Int64}(0)
    q, ldw = observers === nothing ? (0, max(op.n, 1)) : observerdims(op, observers)
    obs = zeros(Float64, q, k, nrep)
    timeweights === nothing || length(timeweights) == nrep || throw(DimensionMismatch("timeweights of $(length(timeweights)), nsteps $nrep"))
    Xbar = timeweights === nothing ? nothing : zeros(Float64, size(X)...)
    ldm = max(op.n, 1)
    scale = nothing
    if sourcescale !== nothing   # the library reads entry t·k + c: column-major k x nsteps
        source === nothing && throw(ArgumentError("sourcescale needs a source"))
        size(sourcescale) == (X isa AbstractVector ? (nrep,) : (k, nrep)) ||
            throw(DimensionMismatch("sourcescale $(size(sourcescale)), expected $(X isa AbstractVector ? (nrep,) : (k, nrep))"))
        scale = Array{Float64}(sourcescale)
    end
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        nslots = Ref{Int64}(0)
        slots_fn = sym(:otmb_op_slots)
        check(ccall(slots_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), op.handle, nslots, C_NULL))
        ptrs, lds, blocks = schedsources(op, source, X, nslots[])
        step_sched_fn = sym(:otmb_op_step_sched)
        GC.@preserve blocks begin
            rc = ccall(step_sched_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Int64, Int64, Int64,
                    Ptr{Ptr{Float64}}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64},
                    Ptr{Int32}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
                op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, ldd, Float64(dt), Float64(θ), Int64(nsteps), Int64(firstslot - 1),
                Int64(substeps), Int64(length(ptrs)), isempty(ptrs) ? C_NULL : ptrs, lds, scale === nothing ? C_NULL : scale, X, ldx,
                Float64(rtol), Int64(maxiter), pc, done, iters, relres, reason,
                Int64(q), observers === nothing ? C_NULL : observers, ldw, observers === nothing ? C_NULL : obs,
                timeweights === nothing ? C_NULL : timeweights, Xbar === nothing ? C_NULL : Xbar, ldm)
            rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which step and column stopped why
        end
    end
    ran = 1:min(done[] + 1, nrep)
    why = permutedims([SOLVE_REASONS[r + 1] for r in reason[:, ran]])
    return X, (stepsdone = done[], iterations = permutedims(iters[:, ran]), relres = permutedims(relres[:, ran]), reason = why,
               converged = why .== :converged, observations = observers === nothing ? nothing : obs[:, :, 1:done[]],
               mean = (Xbar !== nothing && done[] > 0) ? Xbar : nothing)
end
function periodicsched!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator},
                        source::Union{StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}}; dt::Real, ncycle::Integer, θ::Real = 1.0,
                        firstslot::Integer = 1, substeps::Integer = 1, d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing,
                        x0::Bool = false, rtol::Real = 1e-10, maxiter::Integer = 10000, precond::Symbol = :jacobi, outer::Symbol = :none,
                        ptol::Real = 1e-8, restart::Integer = 30, maxcycles::Integer = 1000)
    oc = outercode(outer)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldx, ldd = scheddims(op, X, d)
    cycles = zeros(Int64, k)
    defect = zeros(Float64, k)
    reason = zeros(Int32, k)
    msolve = zeros(Int64, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        nslots = Ref{Int64}(0)
        slots_fn = sym(:otmb_op_slots)
        check(ccall(slots_fn, Int32, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}), op.handle, nslots, C_NULL))
        ptrs, lds, blocks = schedsources(op, source, X, nslots[])
        periodic_sched_fn = sym(:otmb_op_periodic_sched)
        GC.@preserve blocks begin
            rc = ccall(periodic_sched_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Int64, Int64, Int64,
                    Ptr{Ptr{Float64}}, Int64, Ptr{Float64}, Int64, Int32, Float64, Int64, Int32, Float64, Int64, Int64, Ptr{Int64}, Ptr{Float64},
                    Ptr{Int32}, Int32, Ptr{Int64}),
                op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, ldd, Float64(dt), Float64(θ), Int64(ncycle), Int64(firstslot - 1),
                Int64(substeps), Int64(length(ptrs)), ptrs, lds, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), pc, Float64(ptol),
                Int64(restart), Int64(maxcycles), cycles, defect, reason, oc, msolve)
            rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
        end
    end
    why = [PERIODIC_PC_REASONS[r + 1] for r in reason]
    return X, (cycles = cycles, defect = defect, reason = why, converged = why .== :converged, msolve_iters = msolve)
end
# a vector of source blocks is a schedule by itself: periodic!'s positional source dispatches on it (step! and stepobserve! take their source
# as a keyword, which does not dispatch: their scheduled form is stepsched!)
periodic!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, source::AbstractVector{<:StridedVecOrMat{Float64}};
          kwargs...) = periodicsched!(X, D, source; kwargs...)
periodic!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}, source::AbstractVector{<:StridedVecOrMat{Float64}},
          d::StridedMatrix{Float64}; kwargs...) = periodicsched!(X, D, source; d = d, kwargs...)

# Matrices interpolated between slots (otmb_op_step_interp, otmb_op_periodic_interp; include/otmb.h states the contract).  Step t runs with
# (1 - weight[t])·(slot slota[t]) + weight[t]·(slot slotb[t]) -- the slot itself where the two are one or the weight is 0 or 1; the three vectors
# have one length, which is the number of steps (slots 1-based here, as firstslot is).  interpschedule makes them for the convention of
# offline transport-matrix models (Khatiwala 2007): slot s is valid at the middle of its interval of `substeps` steps and step t is evaluated
# at its start, middle or end.  In integers, m = substeps, t 0-based:  h = 2t + (0, 1, 2)[at];  g = h - m + 2·m·nslots;
# a = (firstslot - 1 + g ÷ 2m) mod nslots;  b = (a + 1) mod nslots;  w = Float64(g mod 2m) / Float64(2m), one division.
# `source`: nothing, an array of X's shape, or a vector of ONE such array (a source per slot is not built with interpolation); everything else
# is stepsched!'s / periodicsched!'s.
function interpschedule(nslots::Integer, substeps::Integer; ncycles::Integer = 1, firstslot::Integer = 1, at::Symbol = :mid)
    (nslots >= 1 && substeps >= 1 && ncycles >= 0 && 1 <= firstslot <= nslots) ||
        throw(ArgumentError("interpschedule: nslots >= 1, substeps >= 1, ncycles >= 0 and 1 <= firstslot <= nslots"))
    at in (:start, :mid, :end) || throw(ArgumentError("interpschedule: at must be :start, :mid or :end"))
    m = Int64(substeps)
    off = at === :start ? 0 : at === :mid ? 1 : 2
    nsteps = Int64(ncycles) * nslots * m
    slota, slotb, weight = zeros(Int64, nsteps), zeros(Int64, nsteps), zeros(Float64, nsteps)
    for t in 0:nsteps-1
        g = 2t + off - m + 2m * nslots
        a = mod(firstslot - 1 + fld(g, 2m), nslots)
        slota[t+1], slotb[t+1] = a + 1, mod(a + 1, nslots) + 1
        weight[t+1] = Float64(mod(g, 2m)) / Float64(2m)
    end
    return slota, slotb, weight
end
function interpargs(op::DeviceOperator, slota, slotb, weight, source)
    length(slota) == length(slotb) == length(weight) ||
        throw(DimensionMismatch("slota of $(length(slota)), slotb of $(length(slotb)), weight of $(length(weight))"))
    all(w -> isfinite(w) && 0.0 <= w <= 1.0, weight) || throw(ArgumentError("weight must be finite and in [0, 1]"))
    source isa AbstractVector{<:StridedVecOrMat{Float64}} && length(source) != 1 &&
        throw(DimensionMismatch("$(length(source)) source blocks, expected 1 (a source per slot is not built with interpolation)"))
    return Vector{Int64}(slota) .- 1, Vector{Int64}(slotb) .- 1, Vector{Float64}(weight)
end
function stepinterp!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}; dt::Real, slota::AbstractVector{<:Integer},
                     slotb::AbstractVector{<:Integer}, weight::AbstractVector{<:Real}, θ::Real = 1.0,
                     source::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing,
                     sourcescale::Union{Nothing,StridedVecOrMat{Float64}} = nothing,
                     d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing, rtol::Real = 1e-10, maxiter::Integer = 10000,
                     precond::Symbol = :jacobi, observers::Union{Nothing,StridedVecOrMat{Float64}} = nothing,
                     timeweights::Union{Nothing,Vector{Float64}} = nothing)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldx, ldd = scheddims(op, X, d)
    sa, sb, w = interpargs(op, slota, slotb, weight, source)
    nrep = Int64(length(w))
    iters = zeros(Int64, k, nrep)
    relres = zeros(Float64, k, nrep)
    reason = zeros(Int32, k, nrep)
    done = Ref{Int64}(0)
    q, ldw = observers === nothing ? (0, max(op.n, 1)) : observerdims(op, observers)
    obs = zeros(Float64, q, k, nrep)
    timeweights === nothing || length(timeweights) == nrep || throw(DimensionMismatch("timeweights of $(length(timeweights)), nsteps $nrep"))
    Xbar = timeweights === nothing ? nothing : zeros(Float64, size(X)...)
    ldm = max(op.n, 1)
    scale = nothing
    if sourcescale !== nothing   # the library reads entry t·k + c: column-major k x nsteps
        source === nothing && throw(ArgumentError("sourcescale needs a source"))
        size(sourcescale) == (X isa AbstractVector ? (nrep,) : (k, nrep)) ||
            throw(DimensionMismatch("sourcescale $(size(sourcescale)), expected $(X isa AbstractVector ? (nrep,) : (k, nrep))"))
        scale = Array{Float64}(sourcescale)
    end
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        ptrs, lds, blocks = schedsources(op, source, X, 1)
        step_interp_fn = sym(:otmb_op_step_interp)
        GC.@preserve blocks begin
            rc = ccall(step_interp_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Ptr{Int64}, Ptr{Int64},
                    Ptr{Float64}, Int64, Ptr{Ptr{Float64}}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, Int32, Ptr{Int64}, Ptr{Int64},
                    Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
                op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, ldd, Float64(dt), Float64(θ), nrep, sa, sb, w,
                Int64(length(ptrs)), isempty(ptrs) ? C_NULL : ptrs, lds, scale === nothing ? C_NULL : scale, X, ldx,
                Float64(rtol), Int64(maxiter), pc, done, iters, relres, reason,
                Int64(q), observers === nothing ? C_NULL : observers, ldw, observers === nothing ? C_NULL : obs,
                timeweights === nothing ? C_NULL : timeweights, Xbar === nothing ? C_NULL : Xbar, ldm)
            rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which step and column stopped why
        end
    end
    ran = 1:min(done[] + 1, nrep)
    why = permutedims([SOLVE_REASONS[r + 1] for r in reason[:, ran]])
    return X, (stepsdone = done[], iterations = permutedims(iters[:, ran]), relres = permutedims(relres[:, ran]), reason = why,
               converged = why .== :converged, observations = observers === nothing ? nothing : obs[:, :, 1:done[]],
               mean = (Xbar !== nothing && done[] > 0) ? Xbar : nothing)
end
function periodicinterp!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator},
                         source::Union{StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}}; dt::Real,
                         slota::AbstractVector{<:Integer}, slotb::AbstractVector{<:Integer}, weight::AbstractVector{<:Real}, θ::Real = 1.0,
                         d::Union{Nothing,Vector{Float64},StridedMatrix{Float64}} = nothing, x0::Bool = false, rtol::Real = 1e-10,
                         maxiter::Integer = 10000, precond::Symbol = :jacobi, outer::Symbol = :none, ptol::Real = 1e-8, restart::Integer = 30,
                         maxcycles::Integer = 1000)
    oc = outercode(outer)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldx, ldd = scheddims(op, X, d)
    sa, sb, w = interpargs(op, slota, slotb, weight, source)
    cycles = zeros(Int64, k)
    defect = zeros(Float64, k)
    reason = zeros(Int32, k)
    msolve = zeros(Int64, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        ptrs, lds, blocks = schedsources(op, source, X, 1)
        periodic_interp_fn = sym(:otmb_op_periodic_interp)
        GC.@preserve blocks begin
            rc = ccall(periodic_interp_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Float64, Float64, Int64, Ptr{Int64}, Ptr{Int64},
                    Ptr{Float64}, Int64, Ptr{Ptr{Float64}}, Int64, Ptr{Float64}, Int64, Int32, Float64, Int64, Int32, Float64, Int64, Int64, Ptr{Int64},
                    Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Int64}),
                op.handle, Int32(adjoint), k, d === nothing ? C_NULL : d, ldd, Float64(dt), Float64(θ), Int64(length(w)), sa, sb, w,
                Int64(length(ptrs)), ptrs, lds, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), pc, Float64(ptol),
                Int64(restart), Int64(maxcycles), cycles, defect, reason, oc, msolve)
            rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
        end
    end
    why = [PERIODIC_PC_REASONS[r + 1] for r in reason]
    return X, (cycles = cycles, defect = defect, reason = why, converged = why .== :converged, msolve_iters = msolve)
end

# d and the source per slot, blended with the matrices (otmb_op_step_season, otmb_op_periodic_season; include/otmb.h states the contract): the
# interpolated calls with `d` nothing, n values, a matrix of X's shape, or a vector of one or nslots such arrays of one shape, and `source`
# likewise with one block or one per slot.  A field given once serves every step as it is; a field given per slot is the slot's block on a plain
# step and (1 - weight[t])·(block slota[t]) + weight[t]·(block slotb[t]) on a blended one.  The library counts the blocks against its slots, so each
# method makes ONE C call.  plainschedule states the scheduled step's rule as explicit vectors: every step plain.
function plainschedule(nslots::Integer, nsteps::Integer; firstslot::Integer = 1, substeps::Integer = 1)
    (nslots >= 1 && nsteps >= 0 && substeps >= 1 && 1 <= firstslot <= nslots) ||
        throw(ArgumentError("plainschedule: nslots >= 1, nsteps >= 0, substeps >= 1 and 1 <= firstslot <= nslots"))
    slota = Int64[mod(firstslot - 1 + fld(t, substeps), nslots) + 1 for t in 0:nsteps-1]
    return slota, copy(slota), zeros(Float64, nsteps)
end
function seasonargs(slota, slotb, weight)
    length(slota) == length(slotb) == length(weight) ||
        throw(DimensionMismatch("slota of $(length(slota)), slotb of $(length(slotb)), weight of $(length(weight))"))
    all(w -> isfinite(w) && 0.0 <= w <= 1.0, weight) || throw(ArgumentError("weight must be finite and in [0, 1]"))
    return Vector{Int64}(slota) .- 1, Vector{Int64}(slotb) .- 1, Vector{Float64}(weight)
end
# (the blocks' addresses, their one leading dimension -- 0 for blocks of n values with `shared` --, what to preserve)
function seasonblocks(op::DeviceOperator, field, X, what::String, shared::Bool)
    field === nothing && return Ptr{Float64}[], Int64(shared ? 0 : max(op.n, 1)), ()
    blocks = field isa AbstractVector{<:StridedVecOrMat{Float64}} ? field : [field]
    isempty(blocks) && throw(DimensionMismatch("0 $what blocks, expected 1 or one per slot"))
    all(size(B) == size(blocks[1]) for B in blocks) || throw(DimensionMismatch("$what blocks of different shapes"))
    if shared && blocks[1] isa AbstractVector
        length(blocks[1]) == op.n || throw(DimensionMismatch("$what has $(length(blocks[1])) values, the operator $(op.n) columns"))
        all(stride(B, 1) == 1 for B in blocks) || throw(ArgumentError("the $what blocks need contiguous columns"))
        return Ptr{Float64}[pointer(B) for B in blocks], Int64(0), blocks
    end
    for B in blocks
        size(B) == size(X) || throw(DimensionMismatch("$what $(size(B)), X $(size(X))"))
        stride(B, 1) == 1 || throw(ArgumentError("the $what blocks need contiguous columns"))
    end
    ld(B) = Int64(B isa AbstractVector || size(B, 2) <= 1 ? max(op.n, 1) : stride(B, 2))
    if !all(ld(B) == ld(blocks[1]) for B in blocks)   # one leading dimension for all: blocks whose own differ are copied compactly
        blocks = [ld(B) == max(op.n, 1) ? B : copy(B) for B in blocks]
    end
    return Ptr{Float64}[pointer(B) for B in blocks], ld(blocks[1]), blocks
end
function stepseason!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator}; dt::Real, slota::AbstractVector{<:Integer},
                     slotb::AbstractVector{<:Integer}, weight::AbstractVector{<:Real}, θ::Real = 1.0,
                     d::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing,
                     source::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing,
                     sourcescale::Union{Nothing,StridedVecOrMat{Float64}} = nothing, rtol::Real = 1e-10, maxiter::Integer = 10000,
                     precond::Symbol = :jacobi, observers::Union{Nothing,StridedVecOrMat{Float64}} = nothing,
                     timeweights::Union{Nothing,Vector{Float64}} = nothing)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldx, _ = scheddims(op, X, nothing)
    sa, sb, w = seasonargs(slota, slotb, weight)
    nrep = Int64(length(w))
    iters = zeros(Int64, k, nrep)
    relres = zeros(Float64, k, nrep)
    reason = zeros(Int32, k, nrep)
    done = Ref{Int64}(0)
    q, ldw = observers === nothing ? (0, max(op.n, 1)) : observerdims(op, observers)
    obs = zeros(Float64, q, k, nrep)
    timeweights === nothing || length(timeweights) == nrep || throw(DimensionMismatch("timeweights of $(length(timeweights)), nsteps $nrep"))
    Xbar = timeweights === nothing ? nothing : zeros(Float64, size(X)...)
    ldm = max(op.n, 1)
    scale = nothing
    if sourcescale !== nothing   # the library reads entry t·k + c: column-major k x nsteps
        source === nothing && throw(ArgumentError("sourcescale needs a source"))
        size(sourcescale) == (X isa AbstractVector ? (nrep,) : (k, nrep)) ||
            throw(DimensionMismatch("sourcescale $(size(sourcescale)), expected $(X isa AbstractVector ? (nrep,) : (k, nrep))"))
        scale = Array{Float64}(sourcescale)
    end
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        dptrs, ldd, dblocks = seasonblocks(op, d, X, "d", true)
        ptrs, lds, blocks = seasonblocks(op, source, X, "source", false)
        step_season_fn = sym(:otmb_op_step_season)
        GC.@preserve dblocks blocks begin
            rc = ccall(step_season_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Ptr{Float64}}, Int64, Float64, Float64, Int64, Ptr{Int64}, Ptr{Int64},
                    Ptr{Float64}, Int64, Ptr{Ptr{Float64}}, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Float64, Int64, Int32, Ptr{Int64}, Ptr{Int64},
                    Ptr{Float64}, Ptr{Int32}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64),
                op.handle, Int32(adjoint), k, Int64(length(dptrs)), isempty(dptrs) ? C_NULL : dptrs, ldd, Float64(dt), Float64(θ), nrep, sa, sb, w,
                Int64(length(ptrs)), isempty(ptrs) ? C_NULL : ptrs, lds, scale === nothing ? C_NULL : scale, X, ldx,
                Float64(rtol), Int64(maxiter), pc, done, iters, relres, reason,
                Int64(q), observers === nothing ? C_NULL : observers, ldw, observers === nothing ? C_NULL : obs,
                timeweights === nothing ? C_NULL : timeweights, Xbar === nothing ? C_NULL : Xbar, ldm)
            rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which step and column stopped why
        end
    end
    ran = 1:min(done[] + 1, nrep)
    why = permutedims([SOLVE_REASONS[r + 1] for r in reason[:, ran]])
    return X, (stepsdone = done[], iterations = permutedims(iters[:, ran]), relres = permutedims(relres[:, ran]), reason = why,
               converged = why .== :converged, observations = observers === nothing ? nothing : obs[:, :, 1:done[]],
               mean = (Xbar !== nothing && done[] > 0) ? Xbar : nothing)
end
function periodicseason!(X::StridedVecOrMat{Float64}, D::Union{DeviceOperator,AdjointDeviceOperator},
                         source::Union{StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}}; dt::Real,
                         slota::AbstractVector{<:Integer}, slotb::AbstractVector{<:Integer}, weight::AbstractVector{<:Real}, θ::Real = 1.0,
                         d::Union{Nothing,StridedVecOrMat{Float64},AbstractVector{<:StridedVecOrMat{Float64}}} = nothing, x0::Bool = false,
                         rtol::Real = 1e-10, maxiter::Integer = 10000, precond::Symbol = :jacobi, outer::Symbol = :none, ptol::Real = 1e-8,
                         restart::Integer = 30, maxcycles::Integer = 1000)
    oc = outercode(outer)
    pc = precondcode(precond)
    adjoint = D isa AdjointDeviceOperator
    op = adjoint ? D.parent : D
    k, ldx, _ = scheddims(op, X, nothing)
    sa, sb, w = seasonargs(slota, slotb, weight)
    cycles = zeros(Int64, k)
    defect = zeros(Float64, k)
    reason = zeros(Int32, k)
    msolve = zeros(Int64, k)
    lock(CALL_LOCK) do
        op.handle == C_NULL && throw(ArgumentError("the DeviceOperator has been released"))
        dptrs, ldd, dblocks = seasonblocks(op, d, X, "d", true)
        ptrs, lds, blocks = seasonblocks(op, source, X, "source", false)
        periodic_season_fn = sym(:otmb_op_periodic_season)
        GC.@preserve dblocks blocks begin
            rc = ccall(periodic_season_fn, Int32, (Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Ptr{Float64}}, Int64, Float64, Float64, Int64, Ptr{Int64}, Ptr{Int64},
                    Ptr{Float64}, Int64, Ptr{Ptr{Float64}}, Int64, Ptr{Float64}, Int64, Int32, Float64, Int64, Int32, Float64, Int64, Int64, Ptr{Int64},
                    Ptr{Float64}, Ptr{Int32}, Int32, Ptr{Int64}),
                op.handle, Int32(adjoint), k, Int64(length(dptrs)), isempty(dptrs) ? C_NULL : dptrs, ldd, Float64(dt), Float64(θ), Int64(length(w)), sa, sb, w,
                Int64(length(ptrs)), ptrs, lds, X, ldx, Int32(x0), Float64(rtol), Int64(maxiter), pc, Float64(ptol),
                Int64(restart), Int64(maxcycles), cycles, defect, reason, oc, msolve)
            rc == 19 || check(rc)      # OTMB_ERR_NOT_CONVERGED is an answer: info says which column stopped why
        end
    end
    why = [PERIODIC_PC_REASONS[r + 1] for r in reason]
    return X, (cycles = cycles, defect = defect, reason = why, converged = why .== :converged, msolve_iters = msolve)
end

const HDIRS = (:west, :east, :south, :north)      # OTMB_DIR_*
f64(a) = Array{Float64}(replace(a, missing => NaN))
# grid-constant arrays go to the library as they are when they already have the C layout: with reuse_grid the library
# recognises an array by its address, which only means something for an array the caller still holds
asis(a) = (a isa Array{Float64} || a isa Array{Int64}) ? a : f64(a)
# indices.Lwet3D is Array{Union{Int,Missing}} in the reference: its Int64 image (0 = missing) is kept between reuse_grid calls
const lwet3d_image = Ref{Any}(nothing)            # (objectid(indices.Lwet3D), Array{Int64,3})
function lwet3d_of(indices, reuse_grid)
    id = objectid(indices.Lwet3D)
    if reuse_grid && lwet3d_image[] !== nothing && lwet3d_image[][1] == id
        return lwet3d_image[][2]
    end
    a = Array{Int64,3}(replace(indices.Lwet3D, missing => 0))
    lwet3d_image[] = reuse_grid ? (id, a) : nothing
    return a
end

"""
    transportmatrix(; ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, Tadv, TκH, TκVML, TκVdeep, upwind)

matrixbuilding.jl:128-150.  Returns `(; T, Tadv, TκH, TκVML, TκVdeep)` as `SparseMatrixCSC{Float64,Int64}`;
the library writes colptr/rowval/nzval straight into the Julia-owned vectors.
"""
function transportmatrix(; ϕ, mlotst, gridmetrics, indices, ρ,
        κH = 500.0, κVML = 0.1, κVdeep = 1.0e-5,
        Tadv = nothing, TκH = nothing, TκVML = nothing, TκVdeep = nothing, upwind = true, operators = true, reuse_grid = false,
        reuse_fluxes = false, pinned = PINNED_RESULTS[], devices = nothing, slabs = nothing)
    # pinned = true (default; ENV["OTMB_PINNED_RESULTS"] = "0" flips it): the five matrices' vectors are pinned memory of the library
    #   (fast; fixed length); pinned = false: ordinary Julia vectors, every in-place operation of the reference's results works
    # devices = 0:7 (extension): the grid is cut into depth slabs, one per listed GPU of this process (otmb_mgpu_*)
    # slabs = S (extension, speed only): the pipelined one-phase build on S depth slabs of the single GPU (or one per entry of `devices`): a slab
    #   uploads while the one above it copies its columns home -- the PCIe link carries both directions at once (otmb_mgpu_transportmatrix_onepass);
    #   slabs = nothing (default): default_slabs() -- 4 on large grids, 0 (the two-phase call) otherwise
    # operators = false (extension, not in the reference): only T is materialised, the four operators return `nothing`
    # reuse_grid = true (extension): the caller promises that gridmetrics / indices are the arrays of the previous call,
    #   unmodified (a loop over time slices); they are then not copied to the GPU again (otmb_ctx_set_reuse_grid)
    # reuse_fluxes = true (extension): ϕ is what facefluxes* returned last, unmodified: its device copy is used
    given = (nothing, Tadv, TκH, TκVML, TκVdeep)    # by matrix: T, Tadv, TκH, TκVML, TκVdeep
    if any(!isnothing, given)
        # matrixbuilding.jl:140-143: an operator that is passed in is NOT built -- nothing it alone would read is read (ϕ / ρ for Tadv, mlotst
        # for TκVML: harmless stand-ins take their place), it is returned as the very object passed (:149), and
        # T = ((Tadv + TκH) + TκVML) + TκVdeep (:147) is formed with it (otmb_tm_args.given): a TκH / TκVdeep with the rows the library
        # derives for this grid -- built with this κ or another -- is neither uploaded again (reuse_grid), counted, stored nor copied home
        # (the fill pass reads or re-derives its values); any other matrix makes T the device sparse add of the four operands (the two-phase
        # call: see the fallback below).
        for (m, A) in enumerate(given)
            (A === nothing || size(A) == (indices.N, indices.N)) || throw(ArgumentError("$(MATNAMES[m]) is $(size(A, 1))x$(size(A, 2)), expected $(indices.N)x$(indices.N)"))
        end
        if !isnothing(Tadv)
            z = zeros(size(gridmetrics.v3D))
            ϕ = (east = z, west = z, north = z, south = z, top = z, bottom = z)
            ρ = 1035.0
        end
        mlotst = something(mlotst, fill(NaN, size(gridmetrics.v3D)[1:2]))
        operators = true    # (the built operators are operands of T and are returned)
    else
        given = nothing
    end
    dev = parse(Int32, get(ENV, "OTMB_DEVICE", "0"))
    two_phase() = fused(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, false, false, Int32(0), pinned, nothing, given)
    fkey = foreign_key(given)
    (given !== nothing && devices === nothing && lock(() -> fkey in FOREIGN_SEEN, CALL_LOCK)) && return two_phase()   # known to need the sparse adds
    try
        if slabs === nothing
            slabs = default_slabs(indices.N, size(gridmetrics.v3D, 3), reuse_fluxes, devices)
            if slabs > 0   # the default's choice between the two protocols is measured (Trial), per kind of call
                key = (Int(dev), Int(indices.N), operators, !(ρ isa Number), reuse_grid, given === nothing ? () : Tuple(m for m in 2:5 if given[m] !== nothing))
                tr = lock(() -> get!(() -> Trial(0, NaN, NaN, true, 0), TRIALS, key), CALL_LOCK)
                t0 = time()
                r = pipelined!(tr) ?
                    fused_onepass(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, Int32(0), pinned, fill(dev, slabs), given) :
                    fused(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, Int32(0), pinned, nothing, given)
                record!(tr, time() - t0)
                return r
            end
        end
        if slabs > 0
            devs = devices === nothing ? fill(dev, clamp(Int(slabs), 1, size(gridmetrics.v3D, 3))) : devices
            return fused_onepass(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, Int32(0), pinned, devs, given)
        end
        return fused(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, Int32(0), pinned, devices, given)
    catch e
        (e isa GivenForeign && given !== nothing) || rethrow()
        # a given operator does not have the rows the library derives (another pattern, Tadv, TκVML): T is then the device sparse add of
        # four materialised operands, which the single-context two-phase call does; remembered for the next time slice
        lock(() -> push!(FOREIGN_SEEN, fkey), CALL_LOCK)
        return two_phase()
    end
end
const MATNAMES = ("T", "Tadv", "TκH", "TκVML", "TκVdeep")
const FOREIGN_SEEN = Set{Any}()
foreign_key(given) = given === nothing ? nothing : Tuple((m, UInt(pointer(given[m].nzval)), length(given[m].rowval)) for m in 2:5 if given[m] !== nothing)

# buildTadv / buildTκH / buildTκVML / buildTκVdeep (src/matrixbuilding.jl:31-120; unexported there and here): ONE operator, by the fused build
# with every other matrix switched off (otmb_tm_args.skip_ops) and nothing the others alone would raise raised (ignore_ops); what the other
# operators would read and this one does not gets harmless stand-ins, as the reference never looks at it.  These are what a caller passes back
# as `TκH = ...` / `TκVdeep = ...` in a loop over time slices.
function build_operator(m::Int; gridmetrics, indices, ϕ = nothing, ρ = 1035.0, mlotst = nothing, κ = (500.0, 0.1, 1.0e-5), upwind = true)
    if ϕ === nothing
        z = zeros(size(gridmetrics.v3D))
        ϕ = (east = z, west = z, north = z, south = z, top = z, bottom = z)
    end
    mlotst = something(mlotst, fill(NaN, size(gridmetrics.v3D)[1:2]))
    others = Int32(0x1e & ~(1 << (m - 1)))
    r = fused(ϕ, mlotst, gridmetrics, indices, ρ, κ[1], κ[2], κ[3], upwind, true, false, false, others, PINNED_RESULTS[], nothing, nothing,
              Int32(0x1f & ~(1 << (m - 1))))
    return r[m]
end
buildTadv(; ϕ, gridmetrics, indices, ρ, upwind = true) = build_operator(2; gridmetrics, indices, ϕ, ρ, upwind)
buildTκH(; gridmetrics, indices, ρ = 1035.0, κH) = build_operator(3; gridmetrics, indices, κ = (κH, 0.1, 1.0e-5))
buildTκVML(; mlotst, gridmetrics, indices, κVML) = build_operator(4; gridmetrics, indices, mlotst, κ = (500.0, κVML, 1.0e-5))
buildTκVdeep(; mlotst = nothing, gridmetrics, indices, κVdeep) = build_operator(5; gridmetrics, indices, κ = (500.0, 0.1, κVdeep))

# `buildTsink(; w, gridmetrics, indices, seafloor = :open)`: the settling operator S of particles that sink at the speed w >= 0 (m/s, positive
# downward), ∂x/∂t + (T + S)·x = … (otmb_build_sink).  No function of the reference builds it: include/otmb.h states the contract.  w: a number,
# nz values (the bottom face of each level) or an (nx, ny, nz) array (`missing` on land is fine: land is never read).  seafloor = :open: what
# reaches the seafloor is buried; :closed: the bottom cell keeps it (a stored 0.0).  S's pattern lies inside T's: `addmatrix!(D, S)`.
function buildTsink(; w, gridmetrics, indices, seafloor::Symbol = :open)
    seafloor in (:open, :closed) || throw(ArgumentError("seafloor must be :open or :closed, not :$seafloor"))
    (; v3D, area2D) = gridmetrics
    nx, ny, nz = size(v3D)
    v = asis(v3D); ar = asis(area2D)
    lw3 = lwet3d_of(indices, false)
    lw = indices.Lwet isa Vector{Int64} ? indices.Lwet : Vector{Int64}(indices.Lwet)
    N = Int64(indices.N)
    wform = w isa Number ? Int32(0) : ndims(w) == 1 ? Int32(1) : Int32(2)
    wa = w isa Number ? Float64[] : f64(w)
    w isa Number || size(wa) == (nz,) || size(wa) == (nx, ny, nz) || throw(DimensionMismatch("w is $(size(wa)), expected a number, ($nz,) or $((nx, ny, nz))"))
    cap = max(2N, 1)
    colptr = Vector{Int64}(undef, N + 1); rowval = Vector{Int64}(undef, cap); nzval = Vector{Float64}(undef, cap)
    k = Ref{Int64}(0)
    lock(CALL_LOCK) do
        build_sink_fn = sym(:otmb_build_sink)
        check(ccall(build_sink_fn, Int32,
            (Ptr{Cvoid}, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64, Int64, Int32, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Int64, Ptr{Int64}),
            context(), wform, w isa Number ? Float64(w) : 0.0, wa, v, ar, lw3, lw, N, nx, ny, nz, Int32(seafloor === :closed), colptr, rowval, nzval, cap, k))
    end
    resize!(rowval, k[]); resize!(nzval, k[])
    return SparseMatrixCSC{Float64,Int64}(N, N, colptr, rowval, nzval)
end

# the arguments of one build, flattened for the C ABI; `keep` holds every converted array alive across the calls
function tmargs(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, ignore_ops::Int32, given = nothing,
                skip_ops::Int32 = Int32(0))
    (; v3D, thkcello, edge_length_2D, distance_to_neighbour_2D, area2D, zt, gridtopology) = gridmetrics
    nx, ny, nz = size(v3D)
    ph = [asis(getproperty(ϕ, d)) for d in (:east, :west, :north, :south, :top, :bottom)]   # as they are: reuse_fluxes knows them by address
    v = asis(v3D); thk = asis(thkcello)
    rho3 = ρ isa Number ? Float64[] : f64(ρ)
    lw3 = lwet3d_of(indices, reuse_grid)
    lw = indices.Lwet isa Vector{Int64} ? indices.Lwet : Vector{Int64}(indices.Lwet)
    el = [asis(edge_length_2D[d]) for d in HDIRS]; dn = [asis(distance_to_neighbour_2D[d]) for d in HDIRS]
    ar = asis(area2D); z = zt isa Vector{Float64} ? zt : Vector{Float64}(zt); ml = f64(Array(mlotst))
    # operators the caller passes: the three vectors of a SparseMatrixCSC{Float64,Int64} as they are (grid constants of a time loop: under the
    # reuse_grid promise the library recognises them by address and neither uploads nor compares them again)
    gv = given === nothing ? nothing : map(A -> A === nothing ? nothing : SparseMatrixCSC{Float64,Int64}(A), given)
    csc = ntuple(m -> (gv === nothing || gv[m] === nothing) ? NOCSC : Csc(pointer(gv[m].colptr), pointer(gv[m].rowval), pointer(gv[m].nzval), length(gv[m].rowval)), 5)
    keep = (ph, v, thk, rho3, lw3, lw, el, dn, ar, z, ml, gv)
    a = TmArgs(nx, ny, nz, topologykind(gridtopology), Int32(upwind), indices.N,
        ntuple(i -> pointer(ph[i]), 6), pointer(v), pointer(thk),
        ρ isa Number ? Ptr{Float64}(C_NULL) : pointer(rho3), ρ isa Number ? Float64(ρ) : 0.0,
        pointer(lw3), pointer(lw), ntuple(i -> pointer(el[i]), 4), ntuple(i -> pointer(dn[i]), 4),
        pointer(ar), pointer(z), pointer(ml), Float64(κH), Float64(κVML), Float64(κVdeep), Ptr{UInt16}(C_NULL),
        Int32(operators ? 0 : 1), ignore_ops, skip_ops, csc, Int32(0))
    return a, keep
end

# plan's count for T is the union-pattern bound; exact-zero sums are dropped (:147).  A shorter T (rare) gets ordinary vectors
# of its own: a COPY of the first `k` entries -- no view into the pinned parent, hence no lifetime to tie (round 3 tied it with a
# WeakKeyDict, whose Array keys compare by CONTENT: two equal trimmed views collided and one parent was freed under its matrix).
trim(x, k) = length(x) == k ? x : x[1:k]
# an operator that was passed in comes back as the very object passed (matrixbuilding.jl:149); what was not asked for is `nothing`
wanted(m, operators, given, skip_ops = Int32(0)) = (operators || m == 1) && (given === nothing || given[m] === nothing) && (skip_ops >> (m - 1)) & 1 == 0
function wrap(N, colptr, rowval, nzval, final, operators, given = nothing, skip_ops = Int32(0))
    mats = Any[(given !== nothing && given[m] !== nothing) ? given[m] :
               wanted(m, operators, given, skip_ops) ? SparseMatrixCSC{Float64,Int64}(N, N, colptr[m], trim(rowval[m], final[m]), trim(nzval[m], final[m])) : nothing
               for m in 1:5]
    return (; T = mats[1], Tadv = mats[2], TκH = mats[3], TκVML = mats[4], TκVdeep = mats[5])
end
# Which engine served the previous host-pointer transportmatrix of a device: the single-GPU context (:ctx) or an otmb_mgpu (its device
# list).  reuse_grid is the caller's promise about THE PREVIOUS CALL, but each engine checks it against ITS OWN previous call: after a change
# of engine (the Trial changes it by itself) the promise is not forwarded -- the new engine's residency keys may describe arrays the caller
# has edited since, legitimately passing reuse_grid = false in between.
const LAST_ENGINE = Dict{Int,Any}()
function reuse_grid_for(device, engine, reuse_grid)
    same = get(LAST_ENGINE, Int(device), nothing) == engine
    LAST_ENGINE[Int(device)] = engine
    return reuse_grid && same
end
ptr_or_null(x, ::Type{T}) where {T} = x === nothing ? Ptr{T}(C_NULL) : Ptr{T}(pointer(x))

# otmb_ctx_set_reuse_grid -> otmb_ctx_set_reuse_fluxes -> otmb_transportmatrix_plan -> otmb_transportmatrix_fetch
function fused(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, ignore_ops::Int32,
               usepinned::Bool, devices, given = nothing, skip_ops::Int32 = Int32(0))
    devices === nothing || return fused_mgpu(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes,
                                              ignore_ops, usepinned, devices, given)
    lock(CALL_LOCK) do
        reuse_grid = reuse_grid_for(parse(Int, get(ENV, "OTMB_DEVICE", "0")), :ctx, reuse_grid)
        check(ccall(sym(:otmb_ctx_set_reuse_grid), Int32, (Ptr{Cvoid}, Int32), context(), Int32(reuse_grid)))
        check(ccall(sym(:otmb_ctx_set_reuse_fluxes), Int32, (Ptr{Cvoid}, Int32), ctx[], Int32(reuse_fluxes)))
        a, keep = tmargs(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, ignore_ops, given, skip_ops)
        N = indices.N
        nnz = zeros(Int64, 5)
        GC.@preserve keep check(ccall(sym(:otmb_transportmatrix_plan), Int32, (Ptr{Cvoid}, Ptr{TmArgs}, Ptr{Int64}), ctx[], Ref(a), nnz))
        want = [wanted(m, operators, given, skip_ops) for m in 1:5]   # (what is not handed out -- a given operator, a skipped matrix -- gets no arrays)
        colptr = [want[m] ? outarray(Int64, usepinned, N + 1) : nothing for m in 1:5]
        rowval = [want[m] ? outarray(Int64, usepinned, nnz[m]) : nothing for m in 1:5]
        nzval = [want[m] ? outarray(Float64, usepinned, nnz[m]) : nothing for m in 1:5]
        final = zeros(Int64, 5)
        cp = [ptr_or_null(x, Int64) for x in colptr]; rv = [ptr_or_null(x, Int64) for x in rowval]; nz = [ptr_or_null(x, Float64) for x in nzval]
        GC.@preserve keep colptr rowval nzval check(ccall(sym(:otmb_transportmatrix_fetch), Int32,
            (Ptr{Cvoid}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}), ctx[], cp, rv, nz, final))
        check(ccall(sym(:otmb_ctx_set_reuse_fluxes), Int32, (Ptr{Cvoid}, Int32), ctx[], Int32(0)))
        return wrap(N, colptr, rowval, nzval, final, operators, given, skip_ops)
    end
end

# otmb_mgpu_set_reuse -> otmb_mgpu_transportmatrix_plan -> otmb_mgpu_transportmatrix_fetch: the same build cut into depth slabs, one per listed GPU
function fused_mgpu(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, ignore_ops::Int32,
                    usepinned::Bool, devices, given = nothing)
    lock(CALL_LOCK) do
        mg = mgpu_of(devices)
        reuse_grid = reuse_grid_for(first(devices), Tuple(Int(d) for d in devices), reuse_grid)
        check_mgpu(mg, ccall(sym(:otmb_mgpu_set_reuse), Int32, (Ptr{Cvoid}, Int32, Int32), mg, Int32(reuse_grid), Int32(reuse_fluxes)))
        a, keep = tmargs(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, ignore_ops, given)
        N = indices.N
        nnz = zeros(Int64, 5)
        GC.@preserve keep check_mgpu(mg, ccall(sym(:otmb_mgpu_transportmatrix_plan), Int32, (Ptr{Cvoid}, Ptr{TmArgs}, Ptr{Int64}), mg, Ref(a), nnz))
        want = [wanted(m, operators, given) for m in 1:5]
        colptr = [want[m] ? outarray(Int64, usepinned, N + 1) : nothing for m in 1:5]
        rowval = [want[m] ? outarray(Int64, usepinned, nnz[m]) : nothing for m in 1:5]
        nzval = [want[m] ? outarray(Float64, usepinned, nnz[m]) : nothing for m in 1:5]
        final = zeros(Int64, 5)
        cp = [ptr_or_null(x, Int64) for x in colptr]; rv = [ptr_or_null(x, Int64) for x in rowval]; nz = [ptr_or_null(x, Float64) for x in nzval]
        GC.@preserve keep colptr rowval nzval check_mgpu(mg, ccall(sym(:otmb_mgpu_transportmatrix_fetch), Int32,
            (Ptr{Cvoid}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}), mg, cp, rv, nz, final))
        return wrap(N, colptr, rowval, nzval, final, operators, given)
    end
end

# otmb_mgpu_set_reuse -> otmb_mgpu_transportmatrix_onepass: the pipelined one-phase build (`slabs = S`): result vectors at their upper bounds
# (a column holds at most 7 / 7 / 5 / 3 / 3 rows, src/matrixbuilding.jl:244-296, :348-415, :450-477), no nnz round trip, every slab's upload beside
# the download of the slab above it.  The pinned blocks become Julia vectors of the FINAL lengths only after the call (no copy, one owner each).
const PER_COLUMN_MAX = (7, 7, 5, 3, 3)
# The default call's choice between the pipelined and the two-phase protocol is MEASURED, because it depends on the host: the pipelined build
# needs the link to carry both directions at once and a few free host threads; where it does not get them it has been seen slower than the
# two-phase call (27.9 against 23.6 ms; usually 20 against 25).  One trial per KIND of call (device, grid size, operators or T alone, scalar
# or 3-D ρ, the reuse_grid promise, which operators are passed in).  Calls 1-2 pipelined (they allocate), 3-4 pipelined and timed, 5 two-phase
# (allocates), 6-7 two-phase and timed; from call 8 on whichever was faster (the minimum of its two samples).  The verdict is not for life:
# every 64th call runs the protocol that lost and refreshes its time, and a chosen protocol that takes more than 1.3 x its recorded time
# three calls in a row (a host that got busy) starts the trial over.  An explicit `slabs =` bypasses this.  (Mirror of api.Trial.)
mutable struct Trial
    n::Int; t1::Float64; t2::Float64; now::Bool; slow::Int
end
const TRIALS = Dict{Any,Trial}()
const REMEASURE_EVERY = 64
decided(tr::Trial) = !isnan(tr.t1) && !isnan(tr.t2)
function pipelined!(tr::Trial)
    lock(CALL_LOCK) do
        tr.n += 1
        best = !decided(tr) || tr.t1 <= tr.t2                                   # (a call that raised was not timed: stay with the pipelined build)
        tr.now = tr.n <= 4 ? true : tr.n <= 7 ? false : (decided(tr) && tr.n % REMEASURE_EVERY == 0) ? !best : best
        return tr.now
    end
end
function record!(tr::Trial, s)
    lock(CALL_LOCK) do
        mine() = tr.now ? tr.t1 : tr.t2
        set!(x) = tr.now ? (tr.t1 = x) : (tr.t2 = x)
        if tr.n in (3, 4, 6, 7)
            set!(isnan(mine()) ? s : min(mine(), s))
        elseif tr.n > 7 && decided(tr)
            if tr.n % REMEASURE_EVERY == 0
                set!(s)
            elseif s > 1.3 * mine()
                tr.slow += 1
                tr.slow >= 3 && (tr.n = 2; tr.t1 = NaN; tr.t2 = NaN; tr.slow = 0)   # this host is not what it was: measure both again
            else
                tr.slow = 0
                set!(s < mine() ? s : 0.9 * mine() + 0.1 * s)
            end
        end
        nothing
    end
end
# slabs = nothing: 4 slabs of the device for grids where the transfers dominate (2^18 wet cells and more, 8 levels and more) -- unless the fluxes
# are promised to be resident on the single-GPU context (reuse_fluxes) or a device list was given.  ENV["OTMB_HOST_SLABS"] overrides the 4.
function default_slabs(N, nz, reuse_fluxes, devices)
    (devices === nothing && !reuse_fluxes) || return 0
    s = parse(Int, get(ENV, "OTMB_HOST_SLABS", "4"))
    # (round 6: no upper limit any more -- the result vectors are sized from the wet mask and the previous slice's counts, ~6 % over what is used,
    # where rounds 4-5 pinned 7N / 7N / 5N / 3N / 3N entries, +30 %, and left grids above 2^25 wet cells to the two-phase call)
    return (s > 0 && N >= (1 << 18) && nz >= 2 * s) ? s : 0
end
# Capacities of the one-phase build's result vectors (mirror of api._capacity_bounds / _capacities): otmb_static_capacity -- entries that always
# suffice, from the wet mask alone, once per indices object -- and, for what varies between time slices (Tadv, TκVML), the previous slice's
# counts with a margin; a slice that outgrows them (OTMB_ERR_CAPACITY) is built again at the mask's bounds.
const STATIC_CAP = Dict{Any,Vector{Int64}}()
const PREV_NNZ = Dict{Any,Vector{Int64}}()
const GROWTH = (1.0, 1.25, 1.0, 1.5, 1.0)
function capacity_bounds(indices, gridmetrics)
    key = (objectid(indices.wet3D), size(indices.wet3D), topologykind(gridmetrics.gridtopology))
    bound = get!(STATIC_CAP, key) do
        wet = Array{UInt8,3}(indices.wet3D)
        out = zeros(Int64, 5)
        rc = ccall(sym(:otmb_static_capacity), Int32, (Ptr{UInt8}, Int64, Int64, Int64, Int32, Ptr{Int64}), wet, size(wet)..., key[3], out)
        rc == 0 || error("otmb_static_capacity failed (status $rc)")
        out
    end
    return key, bound
end
capacities(key, bound) = haskey(PREV_NNZ, key) ? Int64[min(bound[m], floor(Int64, PREV_NNZ[key][m] * GROWTH[m]) + 4096) for m in 1:5] : copy(bound)
struct CapacityExceeded <: Exception end
# one otmb_mgpu_transportmatrix_onepass call into result vectors of `cap` entries (under CALL_LOCK): pinned blocks become Julia vectors of the
# FINAL lengths only after the call (no copy, one owner each); nothing owns them if the call throws
function onepass_call(mg, a, keep, N, cap, usepinned)
    colptr = [outarray(Int64, usepinned, cap[m] > 0 ? N + 1 : 0) for m in 1:5]
    final = zeros(Int64, 5)
    if usepinned
        rvb = Ptr{Cvoid}[]; nzb = Ptr{Cvoid}[]
        try
            for m in 1:5
                push!(rvb, pinned_block(Int64, cap[m])); push!(nzb, pinned_block(Float64, cap[m]))
            end
            cp = [pointer(x) for x in colptr]; rv = [Ptr{Int64}(b) for b in rvb]; nz = [Ptr{Float64}(b) for b in nzb]
            GC.@preserve keep colptr check_mgpu(mg, ccall(sym(:otmb_mgpu_transportmatrix_onepass), Int32,
                (Ptr{Cvoid}, Ptr{TmArgs}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}), mg, Ref(a), cp, rv, nz, cap, final))
        catch
            foreach(b -> ccall(host_free_fn[], Int32, (Ptr{Cvoid}, Ptr{Cvoid}), C_NULL, b), vcat(rvb, nzb))  # nothing owns these blocks yet
            rethrow()
        end
        rowval = [adopt(Int64, rvb[m], Int(final[m])) for m in 1:5]
        nzval = [adopt(Float64, nzb[m], Int(final[m])) for m in 1:5]
    else
        rowval = [Vector{Int64}(undef, cap[m]) for m in 1:5]; nzval = [Vector{Float64}(undef, cap[m]) for m in 1:5]
        cp = [pointer(x) for x in colptr]; rv = [pointer(x) for x in rowval]; nz = [pointer(x) for x in nzval]
        GC.@preserve keep colptr rowval nzval check_mgpu(mg, ccall(sym(:otmb_mgpu_transportmatrix_onepass), Int32,
            (Ptr{Cvoid}, Ptr{TmArgs}, Ptr{Ptr{Int64}}, Ptr{Ptr{Int64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Int64}), mg, Ref(a), cp, rv, nz, cap, final))
        foreach(m -> (resize!(rowval[m], final[m]); resize!(nzval[m], final[m])), 1:5)  # (ordinary vectors shrink in place)
    end
    return colptr, rowval, nzval, final
end
function fused_onepass(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, reuse_fluxes, ignore_ops::Int32,
                       usepinned::Bool, devices, given = nothing)
    lock(CALL_LOCK) do
        mg = mgpu_of(devices)
        reuse_grid = reuse_grid_for(first(devices), Tuple(Int(d) for d in devices), reuse_grid)
        check_mgpu(mg, ccall(sym(:otmb_mgpu_set_reuse), Int32, (Ptr{Cvoid}, Int32, Int32), mg, Int32(reuse_grid), Int32(reuse_fluxes)))
        a, keep = tmargs(ϕ, mlotst, gridmetrics, indices, ρ, κH, κVML, κVdeep, upwind, operators, reuse_grid, ignore_ops, given)
        N = indices.N
        ckey, bound = capacity_bounds(indices, gridmetrics)
        local colptr, rowval, nzval, final
        for attempt in 0:1
            cs = attempt == 0 ? capacities(ckey, bound) : bound
            cap = Int64[wanted(m, operators, given) ? cs[m] + 1 : 0 for m in 1:5]   # (nothing for a given operator: it is not handed out)
            try
                colptr, rowval, nzval, final = onepass_call(mg, a, keep, N, cap, usepinned)
                break
            catch e
                (e isa CapacityExceeded && attempt == 0) || rethrow()
                delete!(PREV_NNZ, ckey)     # this slice outgrew the previous one's counts: once more at the mask's bounds
            end
        end
        all(m -> wanted(m, operators, given), 1:5) && (PREV_NNZ[ckey] = copy(final))
        return wrap(N, colptr, rowval, nzval, final, operators, given)
    end
end

# ---- velocities <-> fluxes (src/velocities.jl:10-74) and facefluxesfromvelocities (:140-151) ------------------------------------
cubedata(x) = x isa AbstractArray ? x : Array(x)

"""
    interpolateontodefaultCgrid(u, u_lon, u_lat, v, v_lon, v_lat, gridmetrics)

gridcellgeometry.jl:103-140.  The Arakawa grid is detected by the reference's own `getarakawagrid` (host, first cell only); C-grid fields
pass through, B-grid fields on the NE corner are averaged onto the east / north faces by the library, anything else raises the
reference's errors.
"""
function interpolateontodefaultCgrid(u, u_lon, u_lat, v, v_lon, v_lat, gridmetrics)
    arakawa = OTMB.getarakawagrid(u_lon, u_lat, v_lon, v_lat, gridmetrics)
    arakawa isa OTMB.CGridCell && return u, u_lon, u_lat, v, v_lon, v_lat
    arakawa isa OTMB.AGridCell && error("Interpolation not implemented for A-grid type")
    (; u_pos, v_pos) = arakawa
    u_pos == v_pos == :NE || error("Interpolation not implemented for this B-grid($u_pos,$v_pos) type")
    FillValue = u.properties["_FillValue"]                      # :111
    is32 = eltype(u) == Float32 && eltype(v) == Float32
    T = is32 ? Float32 : Float64
    a = Array{T,3}(u); b = Array{T,3}(v)
    nx, ny, nz = size(a)
    u2 = Array{Float64,3}(undef, nx, ny, nz); v2 = Array{Float64,3}(undef, nx, ny, nz)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_bgrid_to_cgrid), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Float64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Float64}),
            context(), a, b, Int32(is32), Float64(FillValue), nx, ny, nz, u2, v2))
    end
    (; lon_vertices, lat_vertices) = gridmetrics                # the faces' midpoints, as the reference computes them (:127-137)
    SE = [(lo, la) for (lo, la) in zip(lon_vertices[2, :, :], lat_vertices[2, :, :])]
    NE = [(lo, la) for (lo, la) in zip(lon_vertices[3, :, :], lat_vertices[3, :, :])]
    NW = [(lo, la) for (lo, la) in zip(lon_vertices[4, :, :], lat_vertices[4, :, :])]
    u2p = [OTMB.midpointonsphere(A, B) for (A, B) in zip(NE, SE)]
    v2p = [OTMB.midpointonsphere(A, B) for (A, B) in zip(NW, NE)]
    return u2, [P[1] for P in u2p], [P[2] for P in u2p], v2, [P[1] for P in v2p], [P[2] for P in v2p]
end

# otmb_velocity2fluxes / otmb_fluxes2velocity: the same argument list
function velocityflux(name::Symbol, a, b, gridmetrics, ρ)
    (; thkcello, edge_length_2D, gridtopology) = gridmetrics
    x = cubedata(a); y = cubedata(b)
    is32 = eltype(x) == Float32 && eltype(y) == Float32
    T = is32 ? Float32 : Float64
    x = Array{T,3}(x); y = Array{T,3}(y)
    nx, ny, nz = size(x)
    thk = f64(thkcello); ee = f64(edge_length_2D[:east]); en = f64(edge_length_2D[:north])
    rho3 = ρ isa Number ? Float64[] : f64(ρ)
    oi = Array{Float64,3}(undef, nx, ny, nz); oj = Array{Float64,3}(undef, nx, ny, nz)
    lock(CALL_LOCK) do
        GC.@preserve rho3 check(ccall(sym(name), Int32,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Float64}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int32,
             Ptr{Float64}, Ptr{Float64}),
            context(), x, y, Int32(is32), ρ isa Number ? Ptr{Float64}(C_NULL) : pointer(rho3), ρ isa Number ? Float64(ρ) : 0.0, thk, ee, en,
            nx, ny, nz, topologykind(gridtopology), oi, oj))
    end
    return oi, oj
end

"""
    velocity2fluxes(u, u_lon, u_lat, v, v_lon, v_lat, gridmetrics, ρ)

velocities.jl:10-39 -> `(ϕᵢ, ϕⱼ)`.
"""
function velocity2fluxes(u, u_lon, u_lat, v, v_lon, v_lat, gridmetrics, ρ)
    u, _, _, v, _, _ = interpolateontodefaultCgrid(u, u_lon, u_lat, v, v_lon, v_lat, gridmetrics)
    return velocityflux(:otmb_velocity2fluxes, u, v, gridmetrics, ρ)
end

"""
    fluxes2velocity(ϕᵢ, ϕⱼ, gridmetrics, ρ)

velocities.jl:50-74 -> `(u, v)` on the C-grid.
"""
fluxes2velocity(ϕᵢ, ϕⱼ, gridmetrics, ρ) = velocityflux(:otmb_fluxes2velocity, ϕᵢ, ϕⱼ, gridmetrics, ρ)

"""
    facefluxesfromvelocities(; uo, uo_lon, uo_lat, vo, vo_lon, vo_lat, gridmetrics, indices, ρ)

velocities.jl:140-151: THIS module's velocity2fluxes, then THIS module's facefluxes.
"""
function facefluxesfromvelocities(; uo, uo_lon, uo_lat, vo, vo_lon, vo_lat, gridmetrics, indices, ρ, pinned = PINNED_RESULTS[], devices = nothing)
    FillValue = uo.properties["_FillValue"]
    @assert isequal(FillValue, vo.properties["_FillValue"])      # velocities.jl:143
    umo, vmo = velocity2fluxes(uo, uo_lon, uo_lat, vo, vo_lon, vo_lat, gridmetrics, ρ)
    return facefluxes(umo, vmo, gridmetrics, indices; FillValue, pinned, devices)
end

"""
    bolus_GM_velocity(ρ, gridmetrics, indices; κGM = 600, maxslope = 0.01)

RediGM.jl:46-79 -> `(u, v)`.  Experimental in the reference (never enters T), unexported there and here.
"""
function bolus_GM_velocity(ρ, gridmetrics, indices; κGM = 600, maxslope = 0.01)
    rho = f64(ρ)
    nx, ny, nz = size(rho)
    z3d = f64(gridmetrics.Z3D)
    wet = Array{UInt8,3}(indices.wet3D)
    de = f64(gridmetrics.distance_to_neighbour_2D[:east]); dn = f64(gridmetrics.distance_to_neighbour_2D[:north])
    u = Array{Float64,3}(undef, nx, ny, nz); v = Array{Float64,3}(undef, nx, ny, nz)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_bolus_gm_velocity), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Int64, Int32, Float64, Float64,
             Ptr{Float64}, Ptr{Float64}),
            context(), rho, z3d, wet, de, dn, nx, ny, nz, topologykind(gridmetrics.gridtopology), Float64(κGM), Float64(maxslope), u, v))
    end
    return u, v
end

"""
    makegridmetrics(; areacello, volcello, lon, lat, lev, lon_vertices, lat_vertices, gpu = false)

gridcellgeometry.jl:265-311.  `gpu = false` (default): the reference's own function, unchanged.  `gpu = true` (extension): the replace
rules, divisions, cumulative sums and the twelve haversine arrays are computed by the library (otmb_makegridmetrics); the vertex
permutation and the topology test stay the reference's host functions.  Same 13-field NamedTuple; the distances agree with the
reference's to 1e-12 (another math library), everything else bit for bit.
"""
function makegridmetrics(; areacello, volcello, lon, lat, lev, lon_vertices, lat_vertices, gpu = false)
    gpu || return OTMB.makegridmetrics(; areacello, volcello, lon, lat, lev, lon_vertices, lat_vertices)
    fillof(x) = haskey(x.properties, "_FillValue") ? Float64(x.properties["_FillValue"]) : NaN
    vol = f64(Array{Union{Missing,Float64}}(volcello)); area = f64(Array{Union{Missing,Float64}}(areacello))   # missing -> NaN (:269-280)
    nx, ny, nz = size(vol)
    zt = lev |> Array
    lat = Array{Float64}(lat); lon = Array{Float64}(lon)
    lonv = Array{Float64}(lon_vertices); latv = Array{Float64}(lat_vertices)
    vertexidx = OTMB.vertexpermutation(lonv, latv)                                   # :296
    perm = Int32[Int32(q - 1) for q in vertexidx]                                    # 0-based for the C side, applied while reading
    lon_vertices = lonv[vertexidx, :, :]; lat_vertices = latv[vertexidx, :, :]       # what the NamedTuple carries (:297-298)
    gridtopology = OTMB.getgridtopology(lon_vertices, lat_vertices, zt)              # :302
    area2D = Array{Float64,2}(undef, nx, ny)
    v3D = Array{Float64,3}(undef, nx, ny, nz); thkcello = similar(v3D); Z3D = similar(v3D)
    el = [Array{Float64,2}(undef, nx, ny) for _ in 1:4]; de = [Array{Float64,2}(undef, nx, ny) for _ in 1:4]; dn = [Array{Float64,2}(undef, nx, ny) for _ in 1:4]
    lock(CALL_LOCK) do
        pel = [pointer(a) for a in el]; pde = [pointer(a) for a in de]; pdn = [pointer(a) for a in dn]
        GC.@preserve el de dn check(ccall(sym(:otmb_makegridmetrics), Int32,
            (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32},
             Int64, Int64, Int64, Int32, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}),
            context(), vol, area, fillof(areacello), fillof(volcello), lon, lat, lonv, latv, perm, nx, ny, nz, topologykind(gridtopology),
            area2D, v3D, thkcello, Z3D, pel, pde, pdn))
    end
    bydir(a) = Dict(d => a[k] for (k, d) in enumerate(HDIRS))                        # OTMB_DIR_* order: west, east, south, north
    return (; area2D, v3D, thkcello, lon_vertices, lat_vertices, lon, lat, Z3D, zt, edge_length_2D = bydir(el),
            distance_to_edge_2D = bydir(de), distance_to_neighbour_2D = bydir(dn), gridtopology)
end

"""
    LUMP, SPRAY, vol_c = lump_and_spray(wet3D, vol, T, mask = trues(size(wet3D)); di = 2, dj = 2, dk = 1)

extratools.jl:38-119.  Only the pattern of `T` is read.
"""
function lump_and_spray(wet3D, vol, T, mask = trues(size(wet3D)); di = 2, dj = 2, dk = 1)
    wet = Array{UInt8,3}(wet3D); msk = Array{UInt8,3}(mask)
    nx, ny, nz = size(wet)
    v = Vector{Float64}(vol); N = length(v)
    Tp = Vector{Int64}(T.colptr); Ti = Vector{Int64}(T.rowval)
    lrow = Vector{Int64}(undef, N); lval = Vector{Float64}(undef, N)
    scp = Vector{Int64}(undef, N + 1); srow = Vector{Int64}(undef, N); vc = Vector{Float64}(undef, N)
    Nc = Ref{Int64}(0)
    lock(CALL_LOCK) do
        check(ccall(sym(:otmb_lump_and_spray), Int32,
            (Ptr{Cvoid}, Ptr{UInt8}, Ptr{UInt8}, Int64, Int64, Int64, Ptr{Float64}, Int64, Ptr{Int64}, Ptr{Int64}, Int64, Int64, Int64,
             Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}),
            context(), wet, msk, nx, ny, nz, v, N, Tp, Ti, di, dj, dk, lrow, lval, scp, srow, vc, Nc))
    end
    resize!(scp, Nc[] + 1); resize!(vc, Nc[])
    LUMP = SparseMatrixCSC{Float64,Int64}(Nc[], N, collect(Int64, 1:(N + 1)), lrow, lval)
    SPRAY = SparseMatrixCSC{Float64,Int64}(N, Nc[], scp, srow, ones(N))
    return LUMP, SPRAY, vc
end

end # module
