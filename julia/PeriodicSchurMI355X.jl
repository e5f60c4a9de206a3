# PeriodicSchurMI355X.jl — reference-side binding of libpsd_mi355x.so (include/psd_mi355x.h).
#
# Loaded next to RalphAS/PeriodicSchurDecompositions.jl v0.1.6, this module re-points the package's hot path
# (pschur!/pschur, phessenberg!, gpschur, both ordschur! families, checkpsd, partial_pschur on dense and on sparse
# factors) at the MI355X engine for Float64 and ComplexF64 operands; everything else of the package (the Krylov driver on linear maps, eigvecs,
# generic element types) keeps running the Julia code, which now reaches the engine through these methods wherever it
# calls them.
#
#     using PeriodicSchurDecompositions, LinearAlgebra
#     include("julia/PeriodicSchurMI355X.jl"); using .PeriodicSchurMI355X
#     F = pschur!(A, :R)                      # A::Vector{Matrix{Float64}} -> PeriodicSchur, computed on the GPU
#
# There is no Julia toolchain in the build image of this repository, so this file is reviewed, not executed, here
# (INTEGRATION.md); the tested mirror of the same interface is periodicschurdecompositions.jl_amd/__init__.py.
# Citations are file:line of the reference sources (/root/reference/src, `PSD.jl` = PeriodicSchurDecompositions.jl).
module PeriodicSchurMI355X

using LinearAlgebra
using LinearAlgebra: checksquare
using SparseArrays: SparseMatrixCSC, sparse, getcolptr, rowvals, nonzeros
import PeriodicSchurDecompositions
import PeriodicSchurDecompositions: pschur!, pschur, phessenberg!, gpschur, PeriodicSchur, GeneralizedPeriodicSchur,
                                    checkpsd
const PSD = PeriodicSchurDecompositions
using ArnoldiMethod: ArnoldiMethod

export set_train!, engine_version, pschur_batch!, pschur_batch, gpschur_batch, eigvecs_batch_device, eigcond_batch, subspacecond_batch, psylvester_batch, subspacecond, psylvester, geigvecs_batch_device, ordschur_batch!, checkpsd_batch

const libpsd = get(ENV, "LIBPSD_MI355X", joinpath(@__DIR__, "..", "periodicschurdecompositions.jl_amd", "libpsd_mi355x.so"))

const INFO_NOCONV = 1_000_000
const INFO_NOTIMPL = 2_000_000
const INFO_RUNTIME = 3_000_000

const BlasElt = Union{Float64, ComplexF64}

# ---------------------------------------------------------------------------------------------------------------------
# context: one per task (the C ABI allows one call at a time per context)
mutable struct Ctx
    ptr::Ptr{Cvoid}
    function Ctx(device::Integer = 0)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        rc = ccall((:psd_create, libpsd), Cint, (Ref{Ptr{Cvoid}}, Cint), r, device)
        rc == 0 || error("psd_create failed (info=$rc): no usable MI355X; there is no CPU fallback in the library")
        c = new(r[])
        finalizer(x -> (ccall((:psd_destroy, libpsd), Cint, (Ptr{Cvoid},), x.ptr); nothing), c)
        c
    end
end
const _ctx = Ref{Union{Nothing, Ctx}}(nothing)
ctx() = something(_ctx[], (_ctx[] = Ctx()))

engine_version() = unsafe_string(ccall((:psd_version, libpsd), Cstring, ()))
"bulges per multishift train (0 or 1: the reference's one-shift-one-sweep iteration, sweep for sweep)"
set_train!(m::Integer) = ccall((:psd_set_train, libpsd), Cint, (Ptr{Cvoid}, Cint), ctx().ptr, m)
"period shard of the Schur vectors (one context per GPU, one process each): rank `r` of `w` forms and updates only the Z_j of its slice"
set_shard!(r::Integer, w::Integer) = ccall((:psd_set_shard, libpsd), Cint, (Ptr{Cvoid}, Cint, Cint), ctx().ptr, r, w)
"factor-sliced sweep windows: G workgroups per window, each with the blocks of its slice of the period (clamped to what fits one GPU)"
set_slices!(G::Integer) = ccall((:psd_set_slices, libpsd), Cint, (Ptr{Cvoid}, Cint), ctx().ptr, G)
"1 if this context's Hessenberg reductions take the pipe form (fixed when the context was created)"
hess_pipe() = ccall((:psd_get_hess_pipe, libpsd), Cint, (Ptr{Cvoid},), ctx().ptr)

# info -> the exception the reference throws at the same place
function _throw(info::Integer)
    info == 0 && return nothing
    info < 0 && throw(ArgumentError("libpsd_mi355x: argument $(-info) invalid"))
    info >= INFO_RUNTIME && error("libpsd_mi355x: HIP runtime failure (code $(info - INFO_RUNTIME))")
    info >= INFO_NOTIMPL && throw(PSD.NotImplemented("not implemented in libpsd_mi355x"))          # PSD.jl:30
    info >= INFO_NOCONV && error("convergence failed at level $(info - INFO_NOCONV)")               # PSD.jl:892
    error("libpsd_mi355x: info=$info")
end
# ordschur! codes: 2000 + j  IllConditionedException(j) (ordschur.jl:61), 3000 SingularException (utils.jl:128)
function _throw_ord(info::Integer)
    2000 <= info < 3000 && throw(PSD.IllConditionedException(info - 2000))
    info == 3000 && throw(LinearAlgebra.SingularException(0))
    _throw(info)
end

_ptrs(M::Vector{<:StridedMatrix{T}}) where {T} = Ptr{Float64}[Ptr{Float64}(pointer(m)) for m in M]
function _dense(M::AbstractVector{<:AbstractMatrix{T}}) where {T <: BlasElt}
    # the C ABI takes column-major n x n blocks with ld = n: Matrix{T} as they are, anything else is copied
    Matrix{T}[(m isa Matrix{T}) ? m : Matrix{T}(m) for m in M]
end
function _check(A)
    isempty(A) && throw(DimensionMismatch("empty sequence"))
    n = checksquare(A[1])
    for a in A                                                                                    # PSD.jl:214-222
        checksquare(a) == n || throw(DimensionMismatch("matrices must have equal order"))
    end
    n
end
_values(α, β, sc) = α ./ β .* 2.0 .^ sc                                                           # generalized.jl:74-76

# ---------------------------------------------------------------------------------------------------------------------
# phessenberg!(A) — PSD.jl:213-259: same packed layout (Hessenberg / QR objects over the caller's matrices) and tau
function phessenberg!(A::Vector{Matrix{T}}) where {T <: BlasElt}
    p = length(A); n = _check(A)
    tau = Matrix{T}(undef, n, p); info = Ref{Cint}(0)
    Ap = _ptrs(A)
    f = T <: Real ? :psd_d_phessenberg : :psd_z_phessenberg
    GC.@preserve A tau begin
        if T <: Real
            ccall((:psd_d_phessenberg, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Ap, tau, C_NULL, info)
        else
            ccall((:psd_z_phessenberg, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Ap, Ptr{Float64}(pointer(tau)), C_NULL, info)
        end
    end
    _throw(info[])
    H1 = Hessenberg(A[1], tau[1:(n - 1), 1])                                                      # PSD.jl:249-251
    pH = [LinearAlgebra.QR(A[j], tau[:, j]) for j in 2:p]                                         # PSD.jl:252-256
    return H1, pH
end

# ---------------------------------------------------------------------------------------------------------------------
# pschur!(A, lr; wantZ, wantT, maxitfac), Float64 — PSD.jl:120-152
function pschur!(A::Vector{Matrix{Float64}}, lr::Symbol = :R; wantZ::Bool = true, wantT::Bool = true, maxitfac = 30)
    orient = PSD.char_lr(lr)                                                                      # PSD.jl:155-177
    p = length(A); n = _check(A)
    Z = wantZ ? [Matrix{Float64}(undef, n, n) for _ in 1:p] : Matrix{Float64}[]
    wr = Vector{Float64}(undef, n); wi = similar(wr)
    si = Ref{Cint}(0); info = Ref{Cint}(0)
    Ap = _ptrs(A); Zp = _ptrs(Z)
    GC.@preserve A Z wr wi begin
        ccall((:psd_d_pschur, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Cint, Cint,
               Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64}, Ref{Cint}, Ptr{Cvoid}, Ptr{Int32}, Int64, Ref{Cint}),
              ctx().ptr, n, p, Ap, C_NULL, orient, wantT, wantZ, maxitfac,
              wantZ ? Zp : C_NULL, wr, wi, si, C_NULL, C_NULL, 0, info)
    end
    _throw(info[])
    js = Int(si[])                                       # 1 for :R, p for :L (PSD.jl:1092-1094)
    T1 = A[js]; T = [A[j] for j in 1:p if j != js]
    wantZ || (Z = [similar(T1, 0, 0)])                   # PSD.jl:1074-1076
    PeriodicSchur(T1, T, Z, complex.(wr, wi), orient, js)
end

# pschur_batch!(problems, lr; wantZ, wantT, maxitfac, infos) — no reference equivalent: pschur!(A, lr; ...) (PSD.jl:120-152,
# 1106-1111) for many small problems of equal order and period in ONE call (parameter sweeps, the orbits of a
# multiple-shooting run).  Two methods: Float64 problems (psd_d_pschur_batch) and ComplexF64 problems (psd_z_pschur_batch,
# all signatures +1: one wavefront carries one problem through the whole iteration).  Works in place like pschur!; returns
# a Vector{PeriodicSchur}.  A problem that does not converge throws like pschur! after all have run; with `infos` (a
# Vector{Cint} of length(problems)) the per-problem codes are stored there instead and nothing is thrown for a failed
# problem.
function pschur_batch!(problems::Vector{Vector{Matrix{Float64}}}, lr::Symbol = :R; wantZ::Bool = true, wantT::Bool = true,
                       maxitfac = 30, infos::Union{Nothing, Vector{Cint}} = nothing)
    orient = PSD.char_lr(lr)                                                                      # PSD.jl:155-177
    nb = length(problems)
    nb == 0 && return PeriodicSchur[]
    p = length(problems[1]); n = _check(problems[1])
    for A in problems
        (length(A) == p && _check(A) == n) || throw(DimensionMismatch("the problems of a batch must have equal order and period"))
    end
    flat = reduce(vcat, problems)
    Z = wantZ ? [Matrix{Float64}(undef, n, n) for _ in 1:(nb * p)] : Matrix{Float64}[]
    wr = Matrix{Float64}(undef, n, nb); wi = similar(wr)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    si = Ref{Cint}(0); info = Ref{Cint}(0)
    Ap = _ptrs(flat); Zp = _ptrs(Z)
    GC.@preserve flat Z wr wi codes begin
        ccall((:psd_d_pschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Cchar, Cint, Cint, Cint,
               Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ref{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Ap, orient, wantT, wantZ, maxitfac,
              wantZ ? Zp : C_NULL, wr, wi, codes, si, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])                 # argument / runtime codes end the call
    js = Int(si[])
    out = map(1:nb) do q
        A = problems[q]
        T1 = A[js]; T = [A[j] for j in 1:p if j != js]
        Zq = wantZ ? Z[((q - 1) * p + 1):(q * p)] : [similar(T1, 0, 0)]
        PeriodicSchur(T1, T, Zq, complex.(wr[:, q], wi[:, q]), orient, js)
    end
    infos === nothing && foreach(_throw, codes)
    out
end
function pschur_batch!(problems::Vector{Vector{Matrix{ComplexF64}}}, lr::Symbol = :R; wantZ::Bool = true,
                       wantT::Bool = true, maxitfac = 30, infos::Union{Nothing, Vector{Cint}} = nothing)
    orient = PSD.char_lr(lr)
    nb = length(problems)
    nb == 0 && return PeriodicSchur[]
    p = length(problems[1]); n = _check(problems[1])
    for A in problems
        (length(A) == p && _check(A) == n) || throw(DimensionMismatch("the problems of a batch must have equal order and period"))
    end
    flat = reduce(vcat, problems)
    Z = wantZ ? [Matrix{ComplexF64}(undef, n, n) for _ in 1:(nb * p)] : Matrix{ComplexF64}[]
    α = zeros(ComplexF64, n, nb); β = zeros(Float64, n, nb); sc = zeros(Int32, n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    si = Ref{Cint}(0); info = Ref{Cint}(0)
    Ap = _ptrs(flat); Zp = _ptrs(Z)
    GC.@preserve flat Z α β sc codes begin
        ccall((:psd_z_pschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Cchar, Cint, Cint, Cint,
               Ptr{Ptr{Float64}}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cint}, Ref{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Ap, orient, wantT, wantZ, maxitfac,
              wantZ ? Zp : C_NULL, α, β, sc, codes, si, C_NULL, info)
    end
    # argument codes and call-wide runtime codes end the call (a per-problem code is also the return value: not those)
    (info[] < 0 || (info[] >= INFO_NOTIMPL && !(info[] in codes))) && _throw(info[])
    js = Int(si[])
    out = map(1:nb) do q
        A = problems[q]
        T1 = A[js]; T = [A[j] for j in 1:p if j != js]
        Zq = wantZ ? Z[((q - 1) * p + 1):(q * p)] : [similar(T1, 0, 0)]
        vals = α[:, q] ./ β[:, q] .* 2.0 .^ sc[:, q]                                                 # generalized.jl:74-76
        PeriodicSchur(T1, T, Zq, vals, orient, js)
    end
    infos === nothing && foreach(_throw, codes)
    out
end
pschur_batch(problems::AbstractVector, lr::Symbol = :R; kwargs...) =
    any(A -> any(a -> eltype(a) <: Complex, A), problems) ?
    pschur_batch!([Matrix{ComplexF64}[Matrix{ComplexF64}(a) for a in A] for A in problems], lr; kwargs...) :
    pschur_batch!([Matrix{Float64}[Matrix{Float64}(a) for a in A] for A in problems], lr; kwargs...)

# pschur_batch!(problems, S, lr; wantZ, wantT, maxitfac, infos) — pschur!(A, S, lr) (generalized.jl:108-148) for many small
# ComplexF64 problems of equal order and period and ONE signature S in ONE call (psd_z_gpschur_batch): the signed
# Hessenberg reduction and the signed periodic QZ, one workgroup / one wavefront per problem.  Works in place; returns a
# Vector{GeneralizedPeriodicSchur}.  An all-true S runs the path of pschur_batch!(problems, lr).  Failures and `infos` as
# pschur_batch!(problems, lr).
function pschur_batch!(problems::Vector{Vector{Matrix{ComplexF64}}}, S::AbstractVector{Bool}, lr::Symbol = :R;
                       wantZ::Bool = true, wantT::Bool = true, maxitfac = 30,
                       infos::Union{Nothing, Vector{Cint}} = nothing)
    orient = PSD.char_lr(lr)
    nb = length(problems)
    nb == 0 && return GeneralizedPeriodicSchur[]
    p = length(problems[1]); n = _check(problems[1])
    for A in problems
        (length(A) == p && _check(A) == n) || throw(DimensionMismatch("the problems of a batch must have equal order and period"))
    end
    length(S) == p || throw(DimensionMismatch("one sign per factor"))
    (orient == 'L' ? S[p] : S[1]) || throw(ArgumentError("The leftmost entry in S must be true"))  # generalized.jl:140
    flat = reduce(vcat, problems)
    Z = wantZ ? [Matrix{ComplexF64}(undef, n, n) for _ in 1:(nb * p)] : Matrix{ComplexF64}[]
    α = zeros(ComplexF64, n, nb); β = zeros(Float64, n, nb); sc = zeros(Int32, n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    si = Ref{Cint}(0); info = Ref{Cint}(0)
    Ap = _ptrs(flat); Zp = _ptrs(Z); Sb = UInt8.(S)
    GC.@preserve flat Z α β sc codes Sb begin
        ccall((:psd_z_gpschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Cint, Cint,
               Ptr{Ptr{Float64}}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cint}, Ref{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Ap, Sb, orient, wantT, wantZ, maxitfac,
              wantZ ? Zp : C_NULL, α, β, sc, codes, si, C_NULL, info)
    end
    (info[] < 0 || (info[] >= INFO_NOTIMPL && !(info[] in codes))) && _throw(info[])
    js = Int(si[])
    out = map(1:nb) do q
        A = problems[q]
        T1 = A[js]; Tv = [A[j] for j in 1:p if j != js]
        Zq = wantZ ? Z[((q - 1) * p + 1):(q * p)] : [similar(T1, 0, 0)]
        GeneralizedPeriodicSchur(collect(Bool, S), js, T1, Tv, Zq, α[:, q], complex.(β[:, q]), Int.(sc[:, q]), orient)
    end
    infos === nothing && foreach(_throw, codes)
    out
end
pschur_batch(problems::AbstractVector, S::AbstractVector{Bool}, lr::Symbol = :R; kwargs...) =
    pschur_batch!([Matrix{ComplexF64}[Matrix{ComplexF64}(a) for a in A] for A in problems], S, lr; kwargs...)

# pschur_batch!(problems::Vector{Vector{Matrix{Float64}}}, S, lr; wantZ, wantT, maxitfac, infos) — pschur!(A, S, lr) for
# Float64 (rgeneralized.jl:3-45) for many small real problems of equal order and period and ONE signature S in ONE call
# (psd_d_gpschur_batch): real quasi-triangular T at schurindex, orthogonal Z, conjugate pairs exact conjugates.  Works in
# place; returns a Vector{GeneralizedPeriodicSchur}.  An all-true S runs the same signed kernels (as pschur!(A, S, lr) does
# for real element types).  maxitfac defaults to the reference's 120 for Float64.  Failures and `infos` as the ComplexF64
# method.  (Written by analogy with that method; not run yet.)
function pschur_batch!(problems::Vector{Vector{Matrix{Float64}}}, S::AbstractVector{Bool}, lr::Symbol = :R;
                       wantZ::Bool = true, wantT::Bool = true, maxitfac = 120,
                       infos::Union{Nothing, Vector{Cint}} = nothing)
    orient = PSD.char_lr(lr)
    nb = length(problems)
    nb == 0 && return GeneralizedPeriodicSchur[]
    p = length(problems[1]); n = _check(problems[1])
    for A in problems
        (length(A) == p && _check(A) == n) || throw(DimensionMismatch("the problems of a batch must have equal order and period"))
    end
    length(S) == p || throw(DimensionMismatch("one sign per factor"))
    (orient == 'L' ? S[p] : S[1]) || throw(ArgumentError("The leftmost entry in S must be true"))  # rgeneralized.jl:37
    flat = reduce(vcat, problems)
    Z = wantZ ? [Matrix{Float64}(undef, n, n) for _ in 1:(nb * p)] : Matrix{Float64}[]
    α = zeros(ComplexF64, n, nb); β = zeros(Float64, n, nb); sc = zeros(Int32, n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    si = Ref{Cint}(0); info = Ref{Cint}(0)
    Ap = _ptrs(flat); Zp = _ptrs(Z); Sb = UInt8.(S)
    GC.@preserve flat Z α β sc codes Sb begin
        ccall((:psd_d_gpschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Cint, Cint,
               Ptr{Ptr{Float64}}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cint}, Ref{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Ap, Sb, orient, wantT, wantZ, maxitfac,
              wantZ ? Zp : C_NULL, α, β, sc, codes, si, C_NULL, info)
    end
    (info[] < 0 || (info[] >= INFO_NOTIMPL && !(info[] in codes))) && _throw(info[])
    js = Int(si[])
    out = map(1:nb) do q
        A = problems[q]
        T1 = A[js]; Tv = [A[j] for j in 1:p if j != js]
        Zq = wantZ ? Z[((q - 1) * p + 1):(q * p)] : [similar(T1, 0, 0)]
        GeneralizedPeriodicSchur(collect(Bool, S), js, T1, Tv, Zq, α[:, q], β[:, q], Int.(sc[:, q]), orient)  # (β::Vector{Ty}, Ty real here: generalized.jl:44-58)
    end
    infos === nothing && foreach(_throw, codes)
    out
end

# gpschur_batch(Aslist, Bslist; real = false) — gpschur(As, Bs) (generalized.jl:1191-1211) for many pairs of series of equal
# shape in ONE call: the interleaving of gpschur per problem, then pschur_batch! with the common alternating signature.
# real = true: every matrix must be real, and the interleaving goes to the Float64 method as it is instead of being cast
# to ComplexF64 (a complex matrix is an ArgumentError then).
function gpschur_batch(Aslist::AbstractVector, Bslist::AbstractVector; real::Bool = false, kwargs...)
    length(Aslist) == length(Bslist) || throw(DimensionMismatch("one Bs per As"))
    isempty(Aslist) && return GeneralizedPeriodicSchur[]
    args = [PSD._mkpsargs(collect(As), Bs) for (As, Bs) in zip(Aslist, Bslist)]
    Ss = args[1][2]
    all(a -> a[2] == Ss, args) || throw(DimensionMismatch("the problems of a batch must have equal order and period"))
    if real
        all(a -> all(c -> eltype(c) <: Real, a[1]), args) ||
            throw(ArgumentError("gpschur_batch(real = true): the matrices must be real"))
        return pschur_batch!([Matrix{Float64}[Matrix{Float64}(c) for c in a[1]] for a in args], collect(Bool, Ss); kwargs...)
    end
    pschur_batch!([Matrix{ComplexF64}[Matrix{ComplexF64}(c) for c in a[1]] for a in args], collect(Bool, Ss); kwargs...)
end

# ordschur_batch!(problems, select; wantZ, infos) — no reference equivalent: ordschur!(P, select; wantZ) (rordschur.jl:3-132)
# for many small Float64 decompositions of equal order, period, orientation and schurindex (1 or p) in ONE call
# (psd_d_ordschur_batch), the follow-up of pschur_batch!.  `select`: a Vector{Bool} used for every problem or one per
# problem; one member of a conjugate pair takes its partner along.  Works in place like ordschur! and returns the
# problems with their values in the new order.  A problem whose swap is rejected ends alone, a consistent decomposition
# with its old values: it throws like ordschur! after all have run, or with `infos` (a Vector{Cint} of length(problems))
# the per-problem codes are stored there instead and nothing is thrown for it.
function ordschur_batch!(problems::Vector{<:PeriodicSchur{Float64}}, select::AbstractVector; wantZ::Bool = true,
                         infos::Union{Nothing, Vector{Cint}} = nothing)
    nb = length(problems)
    nb == 0 && return problems
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    (js == 1 || js == p) || throw(ArgumentError("only implemented for schurindex in (1,p)"))     # rordschur.jl:25
    wantZ = wantZ && all(ps -> !isempty(ps.Z) && size(ps.Z[1], 1) == n, problems)
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(DimensionMismatch("select must have one entry per eigenvalue"))
        sel[:, q] .= UInt8.(sq)
    end
    # user order: T1 at schurindex, the others around it
    T = reduce(vcat, [[j == js ? ps.T1 : ps.T[j < js ? j : j - 1] for j in 1:p] for ps in problems])
    Z = wantZ ? reduce(vcat, [ps.Z for ps in problems]) : Matrix{Float64}[]
    wr = zeros(n, nb); wi = zeros(n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z)
    GC.@preserve T Z sel wr wi codes begin
        ccall((:psd_d_ordschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cchar, Cint, Ptr{UInt8}, Cint,
               Ptr{Float64}, Ptr{Float64}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Tp, wantZ ? Zp : C_NULL, orient, js, sel, wantZ, wr, wi, codes, C_NULL, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])                 # argument / runtime codes end the call
    for (q, ps) in enumerate(problems)
        codes[q] == 0 && (ps.values .= complex.(wr[:, q], wi[:, q]))
    end
    infos === nothing && foreach(_throw_ord, codes)
    problems
end

# ordschur_batch!(problems, select; wantZ, infos) for ComplexF64 — ordschur!(P, select; wantZ) (ordschur.jl:11-73) for many
# small complex decompositions of equal order, period, orientation and schurindex (1 or p) in ONE call
# (psd_z_ordschur_batch), the follow-up of pschur_batch! on complex problems.  `select` is used as given (there are no
# conjugate pairs to complete); everything else as the Float64 method above.
# NOT YET RUN: this method has not been executed.  It follows the Float64 method above and the complex branch of
# ordschur! line by line; the C entry it calls is tested through the Python binding.
function ordschur_batch!(problems::Vector{<:PeriodicSchur{ComplexF64}}, select::AbstractVector; wantZ::Bool = true,
                         infos::Union{Nothing, Vector{Cint}} = nothing)
    nb = length(problems)
    nb == 0 && return problems
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    (js == 1 || js == p) || throw(ArgumentError("only implemented for schurindex in (1,p)"))     # ordschur.jl:32
    wantZ = wantZ && all(ps -> !isempty(ps.Z) && size(ps.Z[1], 1) == n, problems)
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(DimensionMismatch("select must have one entry per eigenvalue"))
        sel[:, q] .= UInt8.(sq)
    end
    # user order: T1 at schurindex, the others around it
    T = reduce(vcat, [[j == js ? ps.T1 : ps.T[j < js ? j : j - 1] for j in 1:p] for ps in problems])
    Z = wantZ ? reduce(vcat, [ps.Z for ps in problems]) : Matrix{ComplexF64}[]
    α = zeros(ComplexF64, n, nb); β = zeros(n, nb); sc = zeros(Int32, n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z)
    GC.@preserve T Z sel α β sc codes begin
        ccall((:psd_z_ordschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cchar, Cint, Ptr{UInt8}, Cint,
               Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Tp, wantZ ? Zp : C_NULL, orient, js, sel, wantZ, α, β, sc, codes, C_NULL, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])                 # argument / runtime codes end the call
    for (q, ps) in enumerate(problems)
        codes[q] == 0 && (ps.values .= _values(α[:, q], β[:, q], sc[:, q]))                       # ordschur.jl:118
    end
    infos === nothing && foreach(_throw_ord, codes)
    problems
end

# ordschur_batch!(problems, select; wantZ, infos) for signed ComplexF64 problems — ordschur!(P::GeneralizedPeriodicSchur,
# select; wantZ) (ordschur.jl:11-96, sylswap.jl:638-764) for many small decompositions of equal order, period, orientation,
# schurindex (1 or p) and signature S in ONE call (psd_z_gordschur_batch), the follow-up of pschur_batch!(problems, S, lr)
# and gpschur_batch.  An all-true S runs the path of the method above; everything else as there.
# NOT YET RUN: this method has not been executed.  It follows the ComplexF64 method above and the complex branch of
# ordschur!(P::GeneralizedPeriodicSchur, ...) line by line; the C entry it calls is tested through the Python binding.
function ordschur_batch!(problems::Vector{<:GeneralizedPeriodicSchur{ComplexF64}}, select::AbstractVector;
                         wantZ::Bool = true, infos::Union{Nothing, Vector{Cint}} = nothing)
    nb = length(problems)
    nb == 0 && return problems
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    (js == 1 || js == p) || throw(ArgumentError("only implemented for schurindex in (1,p)"))     # ordschur.jl:32
    wantZ = wantZ && all(ps -> !isempty(ps.Z) && size(ps.Z[1], 1) == n, problems)
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        ps.S == ps1.S || throw(DimensionMismatch("the problems of a batch must have equal signatures S"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(DimensionMismatch("select must have one entry per eigenvalue"))
        sel[:, q] .= UInt8.(sq)
    end
    ps1.S[js] || throw(ArgumentError("The entry of S at schurindex must be true"))                # generalized.jl:182
    T = reduce(vcat, [_userT(ps) for ps in problems])
    Z = wantZ ? reduce(vcat, [ps.Z for ps in problems]) : Matrix{ComplexF64}[]
    α = zeros(ComplexF64, n, nb); β = zeros(n, nb); sc = zeros(Int32, n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z); Sb = UInt8.(ps1.S)
    GC.@preserve T Z Sb sel α β sc codes begin
        ccall((:psd_z_gordschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8}, Cint,
               Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Tp, wantZ ? Zp : C_NULL, Sb, orient, js, sel, wantZ, α, β, sc, codes, C_NULL, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])                 # argument / runtime codes end the call
    for (q, ps) in enumerate(problems)
        codes[q] == 0 || continue
        ps.α .= α[:, q]; ps.β .= complex.(β[:, q]); ps.αscale .= Int.(sc[:, q])                   # ordschur.jl:75-96
    end
    infos === nothing && foreach(_throw_ord, codes)
    problems
end

# ordschur_batch!(problems, select; wantZ, infos) for signed Float64 problems — ordschur!(P::GeneralizedPeriodicSchur{Float64},
# select; wantZ) (rordschur.jl:3-132 with the signed block swaps of sylswap.jl:197-538) for many small real decompositions of
# equal order, period, orientation, schurindex (1 or p) and signature S in ONE call (psd_d_gordschur_batch), the follow-up
# of pschur_batch!(problems, S, lr) on real problems.  One member of a conjugate pair takes its partner along.  Every
# signature, the all-true one included, stays on the signed real kernels; everything else as in the ComplexF64 method.
# NOT YET RUN: this method has not been executed.  It follows the signed ComplexF64 method above and the real branch of
# ordschur!(P::GeneralizedPeriodicSchur, ...) line by line; the C entry it calls is tested through the Python binding.
function ordschur_batch!(problems::Vector{<:GeneralizedPeriodicSchur{Float64}}, select::AbstractVector;
                         wantZ::Bool = true, infos::Union{Nothing, Vector{Cint}} = nothing)
    nb = length(problems)
    nb == 0 && return problems
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    (js == 1 || js == p) || throw(ArgumentError("only implemented for schurindex in (1,p)"))     # rordschur.jl:25
    wantZ = wantZ && all(ps -> !isempty(ps.Z) && size(ps.Z[1], 1) == n, problems)
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        ps.S == ps1.S || throw(DimensionMismatch("the problems of a batch must have equal signatures S"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(DimensionMismatch("select must have one entry per eigenvalue"))
        sel[:, q] .= UInt8.(sq)
    end
    ps1.S[js] || throw(ArgumentError("The entry of S at schurindex must be true"))                # generalized.jl:182
    T = reduce(vcat, [_userT(ps) for ps in problems])
    Z = wantZ ? reduce(vcat, [ps.Z for ps in problems]) : Matrix{Float64}[]
    α = zeros(ComplexF64, n, nb); β = zeros(n, nb); sc = zeros(Int32, n, nb)
    codes = infos === nothing ? Vector{Cint}(undef, nb) : infos
    length(codes) == nb || throw(DimensionMismatch("infos must have one entry per problem"))
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z); Sb = UInt8.(ps1.S)
    GC.@preserve T Z Sb sel α β sc codes begin
        ccall((:psd_d_gordschur_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8}, Cint,
               Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cint}, Ptr{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Tp, wantZ ? Zp : C_NULL, Sb, orient, js, sel, wantZ, α, β, sc, codes, C_NULL, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])                 # argument / runtime codes end the call
    for (q, ps) in enumerate(problems)
        codes[q] == 0 || continue
        ps.α .= α[:, q]; ps.β .= β[:, q]; ps.αscale .= Int.(sc[:, q])                             # ordschur.jl:75-96
    end
    infos === nothing && foreach(_throw_ord, codes)
    problems
end

# eigvecs_batch_device(problems, select; shifted) — no reference equivalent: eigvecs(ps, select; shifted) (vectors.jl:25-138)
# by periodic back-substitution for many small Float64 decompositions of equal order, period, orientation and schurindex in
# ONE call (psd_d_eigvecs_batch), the follow-up of pschur_batch!.  `select`: a Vector{Bool} used for every problem or one per
# problem; completed to conjugate pairs.  A problem whose flags are all false costs nothing and gets n x 0 matrices (skip
# the problems whose pschur_batch! code was non-zero that way).  Returns, per problem, the p (shifted) or 1 matrices of
# eigvecs_device.
# `side`: :R the right eigenvectors; :L the LEFT eigenvectors W in the same shapes (psd_d_leigvecs_batch: with mu the root of
# the right vectors, w_{l+1}' A_l = mu w_l' for orientation 'L' and w_l' A_l = mu w_{l+1}' for 'R'; column j of W belongs to
# the eigenvalue of column j of V and w_l' v_l does not depend on l); :B the pair (V, W).  (The `side` keyword is written by
# analogy with Engine.eigvecs_batch(..., side=...), the tested mirror; not run.)
function eigvecs_batch_device(problems::Vector{<:PeriodicSchur{Float64}}, select::AbstractVector; shifted::Bool = true,
                              side::Symbol = :R)
    side in (:R, :L, :B) || throw(ArgumentError("side must be :R, :L or :B"))
    nb = length(problems)
    nb == 0 && return side == :B ? (Vector{Matrix{ComplexF64}}[], Vector{Matrix{ComplexF64}}[]) : Vector{Matrix{ComplexF64}}[]
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    (isempty(ps1.Z) || size(ps1.Z[1], 1) == 0) && throw(ArgumentError("eigvecs requires Schur vectors in the PSD"))
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(ArgumentError("length of `select` must correspond to rank of Schur (sub-)space"))
        sel[:, q] .= UInt8.(sq)
    end
    # user order: T1 at schurindex, the others around it
    T = reduce(vcat, [[j == js ? ps.T1 : ps.T[j < js ? j : j - 1] for j in 1:p] for ps in problems])
    Z = reduce(vcat, [ps.Z for ps in problems])
    wr = [real(ps.values[i]) for i in 1:n, ps in problems]; wi = [imag(ps.values[i]) for i in 1:n, ps in problems]
    nvec = zeros(Cint, nb); info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z)
    nmat = shifted ? p : 1
    call(Vp, maxvec, left) = left ?
        ccall((:psd_d_leigvecs_batch, libpsd), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64}, Cchar, Cint,
         Ptr{UInt8}, Cint, Ptr{Ptr{ComplexF64}}, Cint, Ptr{Cint}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
        ctx().ptr, nb, n, p, Tp, Zp, wr, wi, orient, js, sel, shifted, Vp, maxvec, nvec, C_NULL, C_NULL, info) :
        ccall((:psd_d_eigvecs_batch, libpsd), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64}, Cchar, Cint,
         Ptr{UInt8}, Cint, Ptr{Ptr{ComplexF64}}, Cint, Ptr{Cint}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
        ctx().ptr, nb, n, p, Tp, Zp, wr, wi, orient, js, sel, shifted, Vp, maxvec, nvec, C_NULL, C_NULL, info)
    GC.@preserve T Z wr wi sel nvec begin
        call(C_NULL, 0, false)                            # size query: select completed, nvec
        info[] != 0 && _throw(info[])
        maxvec = Int(maximum(nvec))
        out = map(side == :B ? (false, true) : (side == :L,)) do left
            V = [zeros(ComplexF64, n, maxvec) for _ in 1:(nb * nmat)]
            Vp = [pointer(v) for v in V]
            GC.@preserve V Vp begin
                call(Vp, maxvec, left)
            end
            info[] != 0 && _throw(info[])
            [[V[(q - 1) * nmat + l][:, 1:nvec[q]] for l in 1:nmat] for q in 1:nb]
        end
        return side == :B ? out : out[1]
    end
end

# eigvecs_batch_device for ComplexF64 decompositions (psd_z_eigvecs_batch), the follow-up of the complex pschur_batch!: the
# contract above, except that `select` is used as given — a complex form has no conjugate pairs to complete.  The
# eigenvalues go in as alpha = values, beta = 1, ascale = NULL.  `side` as above (psd_z_leigvecs_batch; not run).
function eigvecs_batch_device(problems::Vector{<:PeriodicSchur{ComplexF64}}, select::AbstractVector; shifted::Bool = true,
                              side::Symbol = :R)
    side in (:R, :L, :B) || throw(ArgumentError("side must be :R, :L or :B"))
    nb = length(problems)
    nb == 0 && return side == :B ? (Vector{Matrix{ComplexF64}}[], Vector{Matrix{ComplexF64}}[]) : Vector{Matrix{ComplexF64}}[]
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    (isempty(ps1.Z) || size(ps1.Z[1], 1) == 0) && throw(ArgumentError("eigvecs requires Schur vectors in the PSD"))
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(ArgumentError("length of `select` must correspond to rank of Schur (sub-)space"))
        sel[:, q] .= UInt8.(sq)
    end
    # user order: T1 at schurindex, the others around it
    T = reduce(vcat, [[j == js ? ps.T1 : ps.T[j < js ? j : j - 1] for j in 1:p] for ps in problems])
    Z = reduce(vcat, [ps.Z for ps in problems])
    α = ComplexF64[ps.values[i] for i in 1:n, ps in problems]; β = ones(Float64, n, nb)
    nvec = zeros(Cint, nb); info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z)
    nmat = shifted ? p : 1
    call(Vp, maxvec, left) = left ?
        ccall((:psd_z_leigvecs_batch, libpsd), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32},
         Cchar, Cint, Ptr{UInt8}, Cint, Ptr{Ptr{ComplexF64}}, Cint, Ptr{Cint}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
        ctx().ptr, nb, n, p, Tp, Zp, α, β, C_NULL, orient, js, sel, shifted, Vp, maxvec, nvec, C_NULL, C_NULL, info) :
        ccall((:psd_z_eigvecs_batch, libpsd), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32},
         Cchar, Cint, Ptr{UInt8}, Cint, Ptr{Ptr{ComplexF64}}, Cint, Ptr{Cint}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
        ctx().ptr, nb, n, p, Tp, Zp, α, β, C_NULL, orient, js, sel, shifted, Vp, maxvec, nvec, C_NULL, C_NULL, info)
    GC.@preserve T Z α β sel nvec begin
        call(C_NULL, 0, false)                            # size query: nvec
        info[] != 0 && _throw(info[])
        maxvec = Int(maximum(nvec))
        out = map(side == :B ? (false, true) : (side == :L,)) do left
            V = [zeros(ComplexF64, n, maxvec) for _ in 1:(nb * nmat)]
            Vp = [pointer(v) for v in V]
            GC.@preserve V Vp begin
                call(Vp, maxvec, left)
            end
            info[] != 0 && _throw(info[])
            [[V[(q - 1) * nmat + l][:, 1:nvec[q]] for l in 1:nmat] for q in 1:nb]
        end
        return side == :B ? out : out[1]
    end
end

# eigcond_batch(problems, select) — no reference equivalent: the reciprocal condition numbers of the eigenvalues of many
# small decompositions (Float64 or ComplexF64, as eigvecs_batch_device takes them) with respect to every factor, the S of
# xTRSNA in periodic form (psd_eigcond_batch), with the right and left eigenvectors of every factor they are computed
# from.  Returns (s, V, W): V, W as eigvecs_batch_device(problems, select; side = :B) returns them, s[q] a p x nvec_q
# matrix, s[q][l, j] = |w_l' v_l| / (||w_{l+1}|| ||v_l||) for orientation 'L' and |w_l' v_l| / (||w_l|| ||v_{l+1}||) for 'R'
# (l + 1 cyclic): to first order |dλ_j / λ_j| <= sum_l ||dA_l|| / (|μ_j| s[q][l, j]).  A zero eigenvalue gives NaN.
# (Written by analogy with Engine.eigcond_batch, the tested mirror; not run.)
function eigcond_batch(problems::Vector{<:PeriodicSchur}, select::AbstractVector)
    V, W = eigvecs_batch_device(problems, select; shifted = true, side = :B)
    nb = length(problems)
    nb == 0 && return (Matrix{Float64}[], V, W)
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1)
    nvec = Cint[size(V[q][1], 2) for q in 1:nb]
    maxvec = Int(maximum(nvec))
    maxvec == 0 && return ([zeros(Float64, p, 0) for _ in 1:nb], V, W)
    pad(X) = [(B = zeros(ComplexF64, n, maxvec); B[:, 1:size(x, 2)] .= x; B) for Xq in X for x in Xq]
    Vb = pad(V); Wb = pad(W)
    Vp = [pointer(b) for b in Vb]; Wp = [pointer(b) for b in Wb]
    s = zeros(Float64, p, maxvec, nb); info = Ref{Cint}(0)
    GC.@preserve Vb Wb Vp Wp nvec s begin
        ccall((:psd_eigcond_batch, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{ComplexF64}}, Ptr{Ptr{ComplexF64}}, Cchar, Cint, Ptr{Cint}, Ptr{Float64},
               Ref{Cint}),
              ctx().ptr, nb, n, p, Vp, Wp, ps1.orientation, maxvec, nvec, s, info)
    end
    info[] != 0 && _throw(info[])
    return ([s[:, 1:nvec[q], q] for q in 1:nb], V, W)
end

# subspacecond_batch(problems, m; want_x) and psylvester_batch(problems, m; C, trans) — no reference equivalent: the
# periodic form of xTRSEN's S and SEP for the leading m eigenvalues of many small decompositions (Float64 or ComplexF64,
# all-true signature; psd_?_subcond_batch), and the periodic Sylvester solve they are built on (psd_?_psylv_batch).
# Problem q is split at m[q] (`m`: an Int or one per problem; not inside a 2 x 2 block), k = n - m:
# T_l = [T11_l T12_l; 0 T22_l]; with (a, b) = (l + 1, l) cyclically for orientation 'L' and (l, l + 1) for 'R',
#     S(X)_l = T11_l X_b - X_a T22_l.
# psylvester_batch solves S(X) = C, or with trans = true the adjoint system S^H(Y) = C; C = nothing: C_l = -T12_l, and then
# T_l [X_b; I] = [X_a; I] T22_l, so that Y_l = Z_l [X_l; I] spans the complementary periodic invariant subspace.  It
# returns per problem the p matrices X_l (m x k).  subspacecond_batch returns (s, sep) — s a p x nb matrix,
# s[l, q] = 1 / sqrt(1 + ||X_l||_F^2), sep[q] the reciprocal of LAPACK's xLACN2 estimate of ||S^-1||_1 on the p m k stacked
# unknowns — and with want_x = true also X.  m = 0 or n: s = 1, sep = Inf.  A singular problem (T11 and T22 share an
# eigenvalue of the product) gets X = NaN, s = 0, sep = 0, and its code (3000) is thrown after all have run unless `infos`
# is given.  There is no scale factor (xTRSYL carries one); above order 128: NotImplemented (psylvester / subspacecond per problem).
# (Written by analogy with Engine.subspacecond_batch / Engine.psylvester_batch, the tested mirrors; not run.)
function _bsylv_inputs(problems::Vector{<:PeriodicSchur}, m)
    nb = length(problems)
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    for ps in problems
        ps isa GeneralizedPeriodicSchur && !all(ps.S) &&
            throw(PSD.NotImplemented("subspacecond_batch / psylvester_batch: signed GeneralizedPeriodicSchur"))
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
    end
    mm = m isa Integer ? fill(Cint(m), nb) : Cint.(collect(m))
    length(mm) == nb || throw(DimensionMismatch("m must be an Int or one Int per problem"))
    # user order: T1 at schurindex, the others around it
    T = reduce(vcat, [[j == js ? ps.T1 : ps.T[j < js ? j : j - 1] for j in 1:p] for ps in problems])
    xb = max(1, maximum(Int(mq) * (n - Int(mq)) for mq in mm))
    return nb, n, p, js, orient, mm, T, xb
end
_bsylv_blocks(bufs, mm, n, p, q) = [reshape(bufs[(q - 1) * p + l][1:(mm[q] * (n - mm[q]))], Int(mm[q]), n - Int(mm[q])) for l in 1:p]

for (Tv, solve, cond) in ((Float64, :psd_d_psylv_batch, :psd_d_subcond_batch),
                          (ComplexF64, :psd_z_psylv_batch, :psd_z_subcond_batch))
@eval function psylvester_batch(problems::Vector{<:PeriodicSchur{$Tv}}, m; C = nothing, trans::Bool = false,
                                infos::Union{Nothing, Vector{Cint}} = nothing)
    isempty(problems) && return Vector{Matrix{$Tv}}[]
    nb, n, p, js, orient, mm, T, xb = _bsylv_inputs(problems, m)
    bufs = [zeros($Tv, xb) for _ in 1:(nb * p)]
    if C !== nothing
        for q in 1:nb, l in 1:p
            size(C[q][l]) == (mm[q], n - mm[q]) || throw(DimensionMismatch("the right-hand sides of a problem are p matrices m x k"))
            bufs[(q - 1) * p + l][1:length(C[q][l])] .= vec(C[q][l])
        end
    end
    codes = infos === nothing ? zeros(Cint, nb) : infos
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Xp = [pointer(b) for b in bufs]
    GC.@preserve T bufs Xp mm codes begin
        ccall(($(QuoteNode(solve)), libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Cchar, Cint, Ptr{Cint}, Ptr{Ptr{$Tv}}, Int64, Cint, Cint,
               Ptr{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Tp, orient, js, mm, Xp, xb, trans, C === nothing, codes, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])
    out = [_bsylv_blocks(bufs, mm, n, p, q) for q in 1:nb]
    infos === nothing && info[] != 0 && _throw_ord(info[])
    return out
end

@eval function subspacecond_batch(problems::Vector{<:PeriodicSchur{$Tv}}, m; want_x::Bool = false,
                                  infos::Union{Nothing, Vector{Cint}} = nothing)
    isempty(problems) && return want_x ? (zeros(0, 0), Float64[], Vector{Matrix{$Tv}}[]) : (zeros(0, 0), Float64[])
    nb, n, p, js, orient, mm, T, xb = _bsylv_inputs(problems, m)
    bufs = want_x ? [zeros($Tv, xb) for _ in 1:(nb * p)] : Vector{$Tv}[]
    s = zeros(Float64, p, nb); sep = zeros(Float64, nb)
    codes = infos === nothing ? zeros(Cint, nb) : infos
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Xp = [pointer(b) for b in bufs]
    GC.@preserve T bufs Xp mm codes s sep begin
        ccall(($(QuoteNode(cond)), libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Cchar, Cint, Ptr{Cint}, Ptr{Float64}, Ptr{Float64},
               Ptr{Ptr{$Tv}}, Int64, Ptr{Cint}, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, nb, n, p, Tp, orient, js, mm, s, sep, want_x ? pointer(Xp) : C_NULL, xb, codes, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])
    infos === nothing && info[] != 0 && _throw_ord(info[])
    return want_x ? (s, sep, [_bsylv_blocks(bufs, mm, n, p, q) for q in 1:nb]) : (s, sep)
end
end

# psylvester(ps, m; C, trans) and subspacecond(ps, m; want_x) — the same for ONE decomposition of any order
# (psd_?_psylv, psd_?_subcond): the definitions, conventions and codes of the batch methods above, whose kernel stops at
# order 128; the solve is a tiled walk over anti-diagonals of X (tile width PSD_SYL_TILE in the environment, default 16).
# psylvester returns the p matrices X_l (m x k); subspacecond returns (s, sep), s a vector of p numbers, and with
# want_x = true also X.  A singular form: X = NaN, s = 0, sep = 0 and the code 3000 thrown.
# (Written by analogy with Engine.psylvester / Engine.subspacecond, the tested mirrors; not run.)
for (Tv, solve, cond) in ((Float64, :psd_d_psylv, :psd_d_subcond), (ComplexF64, :psd_z_psylv, :psd_z_subcond))
@eval function psylvester(ps::PeriodicSchur{$Tv}, m::Integer; C = nothing, trans::Bool = false)
    nb, n, p, js, orient, mm, T, xb = _bsylv_inputs([ps], m)
    mq = Int(clamp(m, 0, n)); k = n - mq
    bufs = [zeros($Tv, mq, k) for _ in 1:p]
    if C !== nothing
        (length(C) == p && all(size(c) == (mq, k) for c in C)) ||
            throw(DimensionMismatch("the right-hand sides are p matrices m x k"))
        for l in 1:p
            bufs[l] .= C[l]
        end
    end
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Xp = [pointer(b) for b in bufs]
    GC.@preserve T bufs Xp begin
        ccall(($(QuoteNode(solve)), libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Cchar, Cint, Cint, Ptr{Ptr{$Tv}}, Cint, Cint, Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, n, p, Tp, orient, js, m, Xp, trans, C === nothing, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])
    info[] != 0 && _throw_ord(info[])
    return bufs
end

@eval function subspacecond(ps::PeriodicSchur{$Tv}, m::Integer; want_x::Bool = false)
    nb, n, p, js, orient, mm, T, xb = _bsylv_inputs([ps], m)
    mq = Int(clamp(m, 0, n)); k = n - mq
    bufs = want_x ? [zeros($Tv, mq, k) for _ in 1:p] : Matrix{$Tv}[]
    s = zeros(Float64, p); sep = Ref{Float64}(0.0)
    info = Ref{Cint}(0)
    Tp = _ptrs(T); Xp = [pointer(b) for b in bufs]
    GC.@preserve T bufs Xp s begin
        ccall(($(QuoteNode(cond)), libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Cchar, Cint, Cint, Ptr{Float64}, Ref{Float64}, Ptr{Ptr{$Tv}},
               Ptr{Cvoid}, Ref{Cint}),
              ctx().ptr, n, p, Tp, orient, js, m, s, sep, want_x ? pointer(Xp) : C_NULL, C_NULL, info)
    end
    (info[] < 0 || info[] >= INFO_NOTIMPL) && _throw(info[])
    info[] != 0 && _throw_ord(info[])
    return want_x ? (s, sep[], bufs) : (s, sep[])
end
end

# geigvecs_batch_device(problems, select; shifted) — geigvecs_device for many small signed ComplexF64 decompositions of one
# shape and one signature in one call (psd_z_geigvecs_batch), the follow-up of gpschur_batch and of the signed
# ordschur_batch!.  Returns, per problem, (Vs, a) as geigvecs_device does; `select` is used as given; a zero or infinite
# eigenvalue gives a valid column.  (Like the rest of this file it has not been executed: no Julia toolchain; the tested
# mirror is Engine.zgeigvecs_batch.)
#
# The method for GeneralizedPeriodicSchur{Float64} (psd_d_geigvecs_batch) is the follow-up of the real gpschur_batch and
# ordschur_batch!: T and Z stay real, `select` is completed to whole conjugate pairs per problem, a pair gives two
# columns (the partner and its scalars the exact conjugates).  The two entries take the same arguments, so both methods
# are made from one text.  (Not executed either; the tested mirror is Engine.dgeigvecs_batch.)
for (Tv, entry) in ((ComplexF64, :psd_z_geigvecs_batch), (Float64, :psd_d_geigvecs_batch))
@eval function geigvecs_batch_device(problems::Vector{<:GeneralizedPeriodicSchur{$Tv}}, select::AbstractVector;
                                     shifted::Bool = true)
    nb = length(problems)
    nb == 0 && return Tuple{Vector{Matrix{ComplexF64}}, Matrix{ComplexF64}}[]
    ps1 = problems[1]
    p = ps1.period; n = size(ps1.T1, 1); js = ps1.schurindex; orient = ps1.orientation
    S = UInt8.(collect(ps1.S))
    (isempty(ps1.Z) || size(ps1.Z[1], 1) == 0) && throw(ArgumentError("geigvecs requires Schur vectors in the PSD"))
    sel = zeros(UInt8, n, nb)
    for (q, ps) in enumerate(problems)
        (ps.period == p && size(ps.T1, 1) == n && ps.schurindex == js && ps.orientation == orient) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        UInt8.(collect(ps.S)) == S || throw(DimensionMismatch("the problems of a batch must have equal signatures S"))
        sq = select[1] isa Bool ? select : select[q]
        length(sq) == n || throw(ArgumentError("length of `select` must correspond to rank of Schur (sub-)space"))
        sel[:, q] .= UInt8.(sq)
    end
    # user order: T1 at schurindex, the others around it
    T = reduce(vcat, [[j == js ? ps.T1 : ps.T[j < js ? j : j - 1] for j in 1:p] for ps in problems])
    Z = reduce(vcat, [ps.Z for ps in problems])
    nvec = zeros(Cint, nb); info = Ref{Cint}(0)
    Tp = _ptrs(T); Zp = _ptrs(Z)
    nmat = shifted ? p : 1
    call(Vp, maxvec, a) = ccall(($(QuoteNode(entry)), libpsd), Cint,
        (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8}, Cint,
         Ptr{Ptr{ComplexF64}}, Cint, Ptr{ComplexF64}, Ptr{Cint}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
        ctx().ptr, nb, n, p, Tp, Zp, S, orient, js, sel, shifted, Vp, maxvec, a, nvec, C_NULL, C_NULL, info)
    GC.@preserve T Z S sel nvec begin
        call(C_NULL, 0, C_NULL)                           # size query: nvec (Float64: select completed)
        info[] != 0 && _throw(info[])
        maxvec = Int(maximum(nvec))
        V = [zeros(ComplexF64, n, maxvec) for _ in 1:(nb * nmat)]
        a = zeros(ComplexF64, p, maxvec, nb)
        Vp = [pointer(v) for v in V]
        GC.@preserve V Vp a begin
            call(Vp, maxvec, a)
        end
        info[] != 0 && _throw(info[])
        return [([V[(q - 1) * nmat + l][:, 1:nvec[q]] for l in 1:nmat], a[:, 1:nvec[q], q]) for q in 1:nb]
    end
end
end

# pschur!(A, lr; ...), ComplexF64 — PSD.jl:1106-1111 (the all-true signature of generalized.jl:108-137)
function pschur!(A::Vector{Matrix{ComplexF64}}, lr::Symbol = :R; wantZ::Bool = true, wantT::Bool = true, maxitfac = 30)
    gps = pschur!(A, trues(length(A)), lr; wantZ = wantZ, wantT = wantT, maxitfac = maxitfac)
    PeriodicSchur(gps.T1, gps.T, gps.Z, gps.values, gps.orientation, gps.schurindex)              # PSD.jl:1110
end

# pschur!(A, S, lr; wantZ, wantT) — generalized.jl:138-146 (ComplexF64), rgeneralized.jl:3-45 (Float64)
function pschur!(A::Vector{Matrix{T}}, S::AbstractVector{Bool}, lr::Symbol = :R;
                 wantZ::Bool = true, wantT::Bool = true, maxitfac = (T <: Real ? 120 : 30),
                 aggressive::Bool = false) where {T <: BlasElt}
    orient = PSD.char_lr(lr)
    p = length(A); n = _check(A)
    length(S) == p || throw(DimensionMismatch("one sign per factor"))
    (orient == 'L' ? S[p] : S[1]) || throw(ArgumentError("The leftmost entry in S must be true"))  # generalized.jl:140
    Z = wantZ ? [Matrix{T}(undef, n, n) for _ in 1:p] : Matrix{T}[]
    α = zeros(ComplexF64, n); β = zeros(Float64, n); sc = zeros(Int32, n)
    si = Ref{Cint}(0); info = Ref{Cint}(0)
    Ap = _ptrs(A); Zp = _ptrs(Z); Sb = UInt8.(S)
    GC.@preserve A Z α β sc Sb begin
        if T <: Real
            ccall((:psd_d_gpschur, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Cint, Cint, Ptr{Ptr{Float64}},
                   Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ref{Cint}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Ap, Sb, orient, wantT, wantZ, maxitfac, wantZ ? Zp : C_NULL, α, β, sc, si, C_NULL, info)
        else
            ccall((:psd_z_pschur, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Cint, Cint, Ptr{Ptr{Float64}},
                   Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ref{Cint}, Ptr{Cvoid}, Ptr{Int32}, Int64, Ref{Cint}),
                  ctx().ptr, n, p, Ap, Sb, orient, wantT, wantZ, maxitfac, wantZ ? Zp : C_NULL, α, β, sc, si, C_NULL,
                  C_NULL, 0, info)
        end
    end
    _throw(info[])
    js = Int(si[]); T1 = A[js]; Tv = [A[j] for j in 1:p if j != js]
    wantZ || (Z = [similar(T1, 0, 0)])
    βT = T <: Real ? β : complex.(β)
    GeneralizedPeriodicSchur(collect(Bool, S), js, T1, Tv, Z, α, βT, Int.(sc), orient)            # generalized.jl:31-48
end

# pschur (copying) — PSD.jl:108-113, generalized.jl:87-91: the package's generic methods copy and call pschur!,
# which dispatches to the methods above for Matrix{Float64} / Matrix{ComplexF64}; other matrix types are densified
function pschur(A::AbstractVector{<:AbstractMatrix{T}}, lr::Symbol = :R; kwargs...) where {T <: BlasElt}
    pschur!([Matrix{T}(a) for a in A], lr; kwargs...)
end
function pschur(A::AbstractVector{<:AbstractMatrix{T}}, S::AbstractVector{Bool}, lr::Symbol = :R;
                kwargs...) where {T <: BlasElt}
    pschur!([Matrix{T}(a) for a in A], S, lr; kwargs...)
end

# gpschur(As, Bs) — generalized.jl:1191-1211: the pairs interleaved with alternating signature, complexified
function gpschur(As::AbstractVector{<:AbstractMatrix{T}}, Bs::AbstractVector{<:AbstractMatrix{T}};
                 kwargs...) where {T <: BlasElt}
    Cs, Ss = PSD._mkpsargs(collect(As), Bs)
    pschur!(Matrix{ComplexF64}[Matrix{ComplexF64}(c) for c in Cs], Ss; kwargs...)
end

# ---------------------------------------------------------------------------------------------------------------------
# pschur!(H1, Hs; wantT, wantZ, Q, maxitfac, rev), Float64 — PSD.jl:322-330 (callers: :150, krylov.jl:583,591)
function pschur!(H1::StridedMatrix{Float64}, Hs::AbstractVector{<:StridedMatrix{Float64}};
                 wantZ::Bool = true, wantT::Bool = true, Q::Union{Nothing, Vector{<:StridedMatrix{Float64}}} = nothing,
                 maxitfac = 30, rev::Bool = false)
    p = length(Hs) + 1; n = checksquare(H1)
    H = _dense(vcat([H1], collect(Hs)))
    Zs = wantZ ? (Q === nothing ? [Matrix{Float64}(I, n, n) for _ in 1:p] : _dense(Q)) : Matrix{Float64}[]
    wr = Vector{Float64}(undef, n); wi = similar(wr); info = Ref{Cint}(0)
    Hp = _ptrs(H); Qp = _ptrs(Zs)
    GC.@preserve H Zs wr wi begin
        ccall((:psd_d_pschur_hess, libpsd), Cint,
              (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Float64},
               Ptr{Cvoid}, Ptr{Int32}, Int64, Ref{Cint}),
              ctx().ptr, n, p, Hp, wantZ ? Qp : C_NULL, wantT, wantZ, maxitfac, wr, wi, C_NULL, C_NULL, 0, info)
    end
    _throw(info[])
    # results back into the caller's storage (in-place contract), then the orientation bookkeeping of PSD.jl:1078-1092
    H[1] === H1 || copyto!(H1, H[1])
    for l in 1:(p - 1); H[l + 1] === Hs[l] || copyto!(Hs[l], H[l + 1]); end
    wantZ || (Zs = [similar(H1, 0, 0)])
    λ = complex.(wr, wi)
    if rev
        Zr = wantZ ? vcat([Zs[1]], [Zs[p + 2 - l] for l in 2:p]) : Zs
        return PeriodicSchur(H1, [Hs[p - l] for l in 1:(p - 1)], Zr, λ, 'L', p)
    end
    PeriodicSchur(H1, collect(Hs), Zs, λ, 'R', 1)
end

# pschur!(H1, Hs, S; wantT, wantZ, Q, maxitfac, rev) — generalized.jl:166-175 (ComplexF64), rgeneralized.jl:49-59 (Float64)
function pschur!(H1::StridedMatrix{T}, Hs::AbstractVector{<:StridedMatrix{T}}, S::AbstractVector{Bool};
                 wantZ::Bool = true, wantT::Bool = true, Q::Union{Nothing, Vector{<:StridedMatrix{T}}} = nothing,
                 maxitfac = (T <: Real ? 120 : 30), rev::Bool = false, aggressive::Bool = false) where {T <: BlasElt}
    p = length(Hs) + 1; n = checksquare(H1)
    S[1] || throw(ArgumentError("The leftmost entry in S must be true"))
    H = _dense(vcat([H1], collect(Hs)))
    Zs = wantZ ? (Q === nothing ? [Matrix{T}(I, n, n) for _ in 1:p] : _dense(Q)) : Matrix{T}[]
    α = zeros(ComplexF64, n); β = zeros(Float64, n); sc = zeros(Int32, n); info = Ref{Cint}(0)
    Hp = _ptrs(H); Qp = _ptrs(Zs); Sb = UInt8.(S)
    f = T <: Real ? :psd_d_gpschur_hess : :psd_z_pschur_hess
    GC.@preserve H Zs α β sc Sb begin
        if T <: Real
            ccall((:psd_d_gpschur_hess, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Ptr{Ptr{Float64}}, Cint, Cint, Cint,
                   Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Int32}, Int64, Ref{Cint}),
                  ctx().ptr, n, p, Hp, Sb, wantZ ? Qp : C_NULL, wantT, wantZ, maxitfac, α, β, sc, C_NULL, C_NULL, 0, info)
        else
            ccall((:psd_z_pschur_hess, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Ptr{Ptr{Float64}}, Cint, Cint, Cint,
                   Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ptr{Int32}, Int64, Ref{Cint}),
                  ctx().ptr, n, p, Hp, Sb, wantZ ? Qp : C_NULL, wantT, wantZ, maxitfac, α, β, sc, C_NULL, C_NULL, 0, info)
        end
    end
    _throw(info[])
    H[1] === H1 || copyto!(H1, H[1])
    for l in 1:(p - 1); H[l + 1] === Hs[l] || copyto!(Hs[l], H[l + 1]); end
    wantZ || (Zs = [similar(H1, 0, 0)])
    βT = T <: Real ? β : complex.(β)
    if rev                                                                                        # generalized.jl:905-925
        Zr = wantZ ? vcat([Zs[1]], [Zs[p + 2 - l] for l in 2:p]) : Zs
        return GeneralizedPeriodicSchur(reverse(collect(Bool, S)), p, H1, [Hs[p - l] for l in 1:(p - 1)], Zr, α, βT,
                                        Int.(sc), 'L')
    end
    GeneralizedPeriodicSchur(collect(Bool, S), 1, H1, collect(Hs), Zs, α, βT, Int.(sc), 'R')
end

# _phessenberg!(A, S; wantQ) — generalized.jl:988-1082 (signed Hessenberg-triangular reduction)
function PSD._phessenberg!(A::Vector{Matrix{T}}, S::AbstractVector{Bool}; wantQ::Bool = true) where {T <: BlasElt}
    p = length(A); n = _check(A)
    Q = wantQ ? [Matrix{T}(undef, n, n) for _ in 1:p] : Matrix{T}[]
    info = Ref{Cint}(0); Ap = _ptrs(A); Qp = _ptrs(Q); Sb = UInt8.(S)
    GC.@preserve A Q Sb begin
        if T <: Real
            ccall((:psd_d_gphessenberg, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Ptr{Ptr{Float64}}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Ap, Sb, wantQ ? Qp : C_NULL, C_NULL, info)
        else
            ccall((:psd_z_gphessenberg, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{UInt8}, Ptr{Ptr{Float64}}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Ap, Sb, wantQ ? Qp : C_NULL, C_NULL, info)
        end
    end
    _throw(info[])
    return A, Q
end

# _rphessenberg!(Ap, A, Q) — rhessx.jl:55-109 (the Krylov driver's projected problem, krylov.jl:809)
function PSD._rphessenberg!(Ap::Matrix{T}, A::Vector{Matrix{T}}, Q::Union{Nothing, Vector{Matrix{T}}} = nothing) where {T <: BlasElt}
    m, n = size(Ap); p = length(A) + 1
    (m == n || m == n + 1) || throw(ArgumentError("Ap must be n x n or (n+1) x n"))               # rhessx.jl:62
    info = Ref{Cint}(0)
    Apt = _ptrs(A); Qp = Q === nothing ? Ptr{Float64}[] : _ptrs(Q)
    nq, nqc = Q === nothing ? (0, 0) : size(Q[1])
    f = T <: Real ? :psd_d_rphessenberg : :psd_z_rphessenberg
    GC.@preserve Ap A Q begin
        if T <: Real
            ccall((:psd_d_rphessenberg, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cint, Cint, Ref{Cint}),
                  ctx().ptr, m, n, p, Ap, Apt, Q === nothing ? C_NULL : Qp, nq, nqc, info)
        else
            ccall((:psd_z_rphessenberg, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Float64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cint, Cint, Ref{Cint}),
                  ctx().ptr, m, n, p, Ptr{Float64}(pointer(Ap)), Apt, Q === nothing ? C_NULL : Qp, nq, nqc, info)
        end
    end
    _throw(info[])
    return Ap, A, Q
end

# ---------------------------------------------------------------------------------------------------------------------
# ordschur!(P, select; wantZ, Z) — ordschur.jl:11-73 (ComplexF64), rordschur.jl:3-132 (Float64)
_userT(P) = begin                                          # full user-order list of the factors (T1 at schurindex)
    p = P.period; Ts = Vector{typeof(P.T1)}(undef, p); il = 0
    for l in 1:p; Ts[l] = (l == P.schurindex) ? P.T1 : P.T[il += 1]; end
    Ts
end
function LinearAlgebra.ordschur!(P::PeriodicSchur{T}, select::AbstractVector{Bool};
                                 wantZ::Bool = true, Z = nothing) where {T <: BlasElt}
    p = P.period; n = size(P.T1, 1); js = P.schurindex
    length(select) == n || throw(DimensionMismatch("select must have one entry per eigenvalue"))
    js in (1, p) || throw(ArgumentError("only implemented for schurindex in (1,p)"))               # ordschur.jl:32
    if Z !== nothing && P.orientation == 'R'
        throw(PSD.NotImplemented("no logic for reversing supplementary Z"))                        # ordschur.jl:36-38
    end
    Ts = _userT(P); Zs = Z === nothing ? P.Z : Z
    wantZ = wantZ && !isempty(Zs) && size(Zs[1], 1) == n
    info = Ref{Cint}(0); sel = UInt8.(select)
    Tp = _ptrs(Ts); Zp = wantZ ? _ptrs(Zs) : Ptr{Float64}[]
    if T <: Real
        wr = zeros(n); wi = zeros(n)
        GC.@preserve Ts Zs sel wr wi ccall((:psd_d_ordschur, libpsd), Cint,
            (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cchar, Cint, Ptr{UInt8}, Cint,
             Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}, Ref{Cint}),
            ctx().ptr, n, p, Tp, wantZ ? Zp : C_NULL, P.orientation, js, sel, wantZ, wr, wi, C_NULL, info)
        _throw_ord(info[])
        P.values .= complex.(wr, wi)                                                              # rordschur.jl:124-130
    else
        α = zeros(ComplexF64, n); β = zeros(n); sc = zeros(Int32, n)
        GC.@preserve Ts Zs sel α β sc ccall((:psd_z_ordschur, libpsd), Cint,
            (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Cchar, Cint, Ptr{UInt8}, Cint,
             Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
            ctx().ptr, n, p, Tp, wantZ ? Zp : C_NULL, P.orientation, js, sel, wantZ, α, β, sc, C_NULL, info)
        _throw_ord(info[])
        P.values .= _values(α, β, sc)                                                             # ordschur.jl:118
    end
    return P
end

# ordschur!(P::GeneralizedPeriodicSchur, select; wantZ) — ordschur.jl:11-96,206-328 with the signed swaps of
# sylswap.jl:197-538 (2x2 blocks, Float64) and :638-764 (1x1)
function LinearAlgebra.ordschur!(P::GeneralizedPeriodicSchur{T}, select::AbstractVector{Bool};
                                 wantZ::Bool = true) where {T <: BlasElt}
    p = P.period; n = size(P.T1, 1); js = P.schurindex
    length(select) == n || throw(DimensionMismatch("select must have one entry per eigenvalue"))
    js in (1, p) || throw(ArgumentError("only implemented for schurindex in (1,p)"))
    Ts = _userT(P); Zs = P.Z
    wantZ = wantZ && !isempty(Zs) && size(Zs[1], 1) == n
    α = zeros(ComplexF64, n); β = zeros(n); sc = zeros(Int32, n); info = Ref{Cint}(0)
    sel = UInt8.(select); Sb = UInt8.(P.S)
    Tp = _ptrs(Ts); Zp = wantZ ? _ptrs(Zs) : Ptr{Float64}[]
    GC.@preserve Ts Zs sel Sb α β sc begin
        if T <: Real
            ccall((:psd_d_gordschur, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8}, Cint,
                   Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, wantZ ? Zp : C_NULL, Sb, P.orientation, js, sel, wantZ, α, β, sc, C_NULL, info)
        else
            ccall((:psd_z_gordschur, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8}, Cint,
                   Ptr{ComplexF64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, wantZ ? Zp : C_NULL, Sb, P.orientation, js, sel, wantZ, α, β, sc, C_NULL, info)
        end
    end
    _throw_ord(info[])
    P.α .= α; P.β .= (T <: Real ? β : complex.(β)); P.αscale .= Int.(sc)                          # ordschur.jl:75-96
    return P
end

# ---------------------------------------------------------------------------------------------------------------------
# checkpsd(P, As; quiet, thresh, strict) — diagnostics.jl:190-263, evaluated on the device (matrix cores)
function checkpsd(P::PSD.AbstractPeriodicSchur{T}, Hs::AbstractVector{<:AbstractMatrix{T}};
                  quiet = false, thresh = 100, strict = true) where {T <: BlasElt}
    p = length(Hs); n = size(P.T1, 1)
    P.period == p || throw(DimensionMismatch("length of Hs vector must match period of P"))        # diagnostics.jl:194
    for l in 1:p
        checksquare(Hs[l]) == n || throw(DimensionMismatch("size of Hs matrices must match P"))   # :197-202
    end
    Ts = _dense(_userT(P)); Zs = _dense(P.Z); As = _dense(Hs)
    S = P isa GeneralizedPeriodicSchur ? UInt8.(P.S) : fill(0x01, p)
    err = zeros(p); orth = zeros(p); tri = zeros(p); ok = Ref{Cint}(0); info = Ref{Cint}(0)
    Tp = _ptrs(Ts); Zp = _ptrs(Zs); Ap = _ptrs(As)
    GC.@preserve Ts Zs As S err orth tri begin
        if T <: Real
            wi = Float64.(imag.(P.values))
            GC.@preserve wi ccall((:psd_d_checkpsd, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint,
                   Ptr{Float64}, Cdouble, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Cint}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, Zp, Ap, S, P.orientation, P.schurindex, wi, thresh, strict, err, orth, tri, ok, info)
        else
            ccall((:psd_z_checkpsd, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint,
                   Cdouble, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Cint}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, Zp, Ap, S, P.orientation, P.schurindex, thresh, strict, err, orth, tri, ok, info)
        end
    end
    _throw(info[])
    if !quiet                                                                                     # diagnostics.jl:235-259
        cmp = strict ? 0.0 : 10 * eps(Float64) * n
        for l in 1:p
            tri[l] > cmp && @warn "triangularity fails for l=$l"
            orth[l] > 10 * eps(Float64) * n && @warn "orthogonality fails for l=$l"
            err[l] > thresh && @warn "large factorization error ($(err[l]) ϵ‖Aₗ‖₁) for l=$l"
        end
    end
    return ok[] != 0, err
end

# checkpsd_batch(Ps, Hss; thresh, strict): checkpsd for MANY small decompositions of one shape (order, period,
# orientation, schurindex, signature) in ONE call (psd_d_checkpsd_batch / psd_z_checkpsd_batch): up to order 64 one
# launch per group of problems, a workgroup per (problem, factor).  Hss[q] are the factors Ps[q] was computed from.
# Returns (ok, err): the reference's Bool per problem and the p x nb matrix of the normalized factorization errors.
# Nothing is warned about: ask checkpsd about a problem whose verdict is false.
function checkpsd_batch(Ps::Vector{<:PSD.AbstractPeriodicSchur{T}}, Hss::AbstractVector; thresh = 100,
                        strict = true) where {T <: BlasElt}
    nb = length(Ps)
    length(Hss) == nb || throw(DimensionMismatch("one vector of factors per decomposition"))
    nb == 0 && return Bool[], zeros(Float64, 0, 0)
    P1 = Ps[1]
    p = P1.period; n = size(P1.T1, 1); js = P1.schurindex; orient = P1.orientation
    sig(P) = P isa GeneralizedPeriodicSchur ? UInt8.(P.S) : fill(0x01, p)
    S = sig(P1)
    Ts = Matrix{T}[]; Zs = Matrix{T}[]; As = Matrix{T}[]
    for (P, Hs) in zip(Ps, Hss)
        P.period == length(Hs) || throw(DimensionMismatch("length of Hs vector must match period of P"))  # diagnostics.jl:194
        for H in Hs
            checksquare(H) == size(P.T1, 1) || throw(DimensionMismatch("size of Hs matrices must match P"))  # :197-202
        end
        (P.period == p && size(P.T1, 1) == n) ||
            throw(DimensionMismatch("the problems of a batch must have equal order and period"))
        (P.schurindex == js && P.orientation == orient && length(P.Z) == p) ||
            throw(DimensionMismatch("the problems of a batch must have equal order, period, orientation and schurindex"))
        sig(P) == S || throw(DimensionMismatch("the problems of a batch must have equal signatures S"))
        append!(Ts, _dense(_userT(P))); append!(Zs, _dense(P.Z)); append!(As, _dense(Hs))
    end
    err = zeros(p, nb); ok = zeros(Int32, nb); info = Ref{Cint}(0)
    Tp = _ptrs(Ts); Zp = _ptrs(Zs); Ap = _ptrs(As)
    GC.@preserve Ts Zs As S err ok begin
        # (the two entries have one argument list: ctx, nb, n, p, T, Z, A, S, orient, schurindex, thresh, strict, err, orth,
        #  tri, ok, stats, info)
        if T <: Real
            ccall((:psd_d_checkpsd_batch, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar,
                   Cint, Cdouble, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, nb, n, p, Tp, Zp, Ap, S, orient, js, thresh, strict, err, C_NULL, C_NULL, ok, C_NULL, info)
        else
            ccall((:psd_z_checkpsd_batch, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar,
                   Cint, Cdouble, Cint, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}, Ref{Cint}),
                  ctx().ptr, nb, n, p, Tp, Zp, Ap, S, orient, js, thresh, strict, err, C_NULL, C_NULL, ok, C_NULL, info)
        end
    end
    _throw(info[])
    return Bool[o != 0 for o in ok], err
end

# ---------------------------------------------------------------------------------------------------------------------
# partial_pschur(As, nev, which; ...) — krylov.jl:446-487, for dense Float64 / ComplexF64 factors: the Krylov steps run on
# the device (psd_d_partial_pschur / psd_z_partial_pschur); sparse factors have the method further down.  Operators given
# as other linear maps keep the reference's CPU driver (these methods only match Vector{Matrix{T}} and
# Vector{SparseMatrixCSC{T,Int}}).  The reference's `vrand!` keyword is NOT honoured on the device:
# without `u1` the start vector comes from the library's counter-based generator, seeded by `seed`.
const _KTARGET = Dict(ArnoldiMethod.LM => 'M', ArnoldiMethod.LR => 'R', ArnoldiMethod.SR => 'r',
                      ArnoldiMethod.LI => 'I', ArnoldiMethod.SI => 'i')
const INFO_PKSFAIL = 5000

function PSD.partial_pschur(As::Vector{Matrix{T}}, nev::Integer, which::ArnoldiMethod.Target = ArnoldiMethod.LM();
                            mindim::Integer = min(max(10, nev), size(As[1], 1)),
                            maxdim::Integer = min(max(20, 2nev), size(As[1], 1)),
                            u1 = nothing, tol = sqrt(eps(Float64)), tol1 = 100 * eps(Float64),
                            restarts = 100, purgebuffer = 2, seed::Integer = 0) where {T <: BlasElt}
    p = length(As); n = size(As[1], 1)
    for l in 1:p
        checksquare(As[l]) == n || throw(ArgumentError("all As must have the same (square) size"))     # krylov.jl:457-461
    end
    nev < 1 && throw(ArgumentError("nev cannot be less than 1"))                                         # :462-464
    nev ≤ mindim ≤ maxdim ≤ p * n ||
        throw(ArgumentError("nev ≤ mindim ≤ maxdim does not hold, got $nev ≤ $mindim ≤ $maxdim"))        # :465-466
    u = u1 === nothing ? nothing : Vector{T}(u1)
    u === nothing || length(u) == n || throw(ArgumentError("u1 must have length matching first matrix/operator"))
    Ts = [Matrix{T}(undef, maxdim, maxdim) for _ in 1:p]
    Zs = [Matrix{T}(undef, n, maxdim) for _ in 1:p]
    wr = zeros(maxdim); wi = zeros(maxdim)
    nconv = Ref{Cint}(0); info = Ref{Cint}(0)
    st = zeros(UInt8, 96)  # psd_krylov_stats: nprods Int64, nconverged Int32, converged Int32, nev Int32, ...
    Ap = _ptrs(As); Tp = _ptrs(Ts); Zp = _ptrs(Zs)
    fn = T <: Real ? :psd_d_partial_pschur : :psd_z_partial_pschur
    GC.@preserve As Ts Zs u wr wi st begin
        up = u === nothing ? Ptr{Float64}(C_NULL) : Ptr{Float64}(pointer(u))
        args = (ctx().ptr, n, p, Ap, nev, _KTARGET[typeof(which)], mindim, maxdim, up, UInt64(seed), Float64(tol),
                Float64(tol1), restarts, purgebuffer, nconv, Tp, Zp, wr, wi, pointer(st), info)
        if T <: Real
            ccall((:psd_d_partial_pschur, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Cint, Cchar, Cint, Cint, Ptr{Float64}, UInt64, Cdouble,
                   Cdouble, Cint, Cint, Ref{Cint}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64},
                   Ptr{UInt8}, Ref{Cint}), args...)
        else
            ccall((:psd_z_partial_pschur, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Cint, Cchar, Cint, Cint, Ptr{Float64}, UInt64, Cdouble,
                   Cdouble, Cint, Cint, Ref{Cint}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64},
                   Ptr{UInt8}, Ref{Cint}), args...)
        end
    end
    return _partial_result(info[], Int(nconv[]), Ts, Zs, wr, wi, st, nev)
end

# error mapping and result construction of the partial_pschur methods
function _partial_result(info::Integer, k::Int, Ts, Zs, wr, wi, st, nev)
    p = length(Ts)
    info == INFO_PKSFAIL && throw(PSD.PKSFailure("Arnoldi reinitialization failed"))                    # krylov.jl:182
    2000 <= info < 3000 && throw(PSD.IllConditionedException(info - 2000))
    info == -19 && throw(ArgumentError("invalid CSR row pointers"))
    info == -20 && throw(ArgumentError("CSR column index outside [0, n)"))
    _throw(info)
    # T[l] holds the k x k factor with leading dimension k in its first k^2 elements
    Tk = [copy(reshape(view(vec(Ts[l]), 1:(k * k)), k, k)) for l in 1:p]
    Zk = [Zs[l][:, 1:k] for l in 1:p]
    λ = complex.(wr[1:k], wi[1:k])
    nprods = Int(reinterpret(Int64, st[1:8])[1])
    ps = PSD.PartialPeriodicSchur(Tk[p], Tk[1:(p - 1)], Zk, λ)                                         # krylov.jl:796
    return ps, ArnoldiMethod.History(nprods, k, k ≥ nev, nev)
end

# partial_pschur for sparse factors (psd_d_partial_pschur_csr / psd_z_partial_pschur_csr): the products run through the
# device SpMV.  The library takes CSR; the CSR of A is the CSC of transpose(A) (plain transpose, for ComplexF64 too: the
# values are not conjugated), shifted to 0-based, with the row pointers as Int64 and the column indices as Int32.  Other
# linear maps (anything that only implements `mul!`) and lists that mix dense and sparse factors keep the reference's CPU
# driver.
function PSD.partial_pschur(As::Vector{SparseMatrixCSC{T, Int}}, nev::Integer,
                            which::ArnoldiMethod.Target = ArnoldiMethod.LM();
                            mindim::Integer = min(max(10, nev), size(As[1], 1)),
                            maxdim::Integer = min(max(20, 2nev), size(As[1], 1)),
                            u1 = nothing, tol = sqrt(eps(Float64)), tol1 = 100 * eps(Float64),
                            restarts = 100, purgebuffer = 2, seed::Integer = 0) where {T <: BlasElt}
    p = length(As); n = size(As[1], 1)
    for l in 1:p
        checksquare(As[l]) == n || throw(ArgumentError("all As must have the same (square) size"))     # krylov.jl:457-461
    end
    nev < 1 && throw(ArgumentError("nev cannot be less than 1"))                                         # :462-464
    nev ≤ mindim ≤ maxdim ≤ p * n ||
        throw(ArgumentError("nev ≤ mindim ≤ maxdim does not hold, got $nev ≤ $mindim ≤ $maxdim"))        # :465-466
    u = u1 === nothing ? nothing : Vector{T}(u1)
    u === nothing || length(u) == n || throw(ArgumentError("u1 must have length matching first matrix/operator"))
    At = [sparse(transpose(A)) for A in As]
    rowptr = [Int64.(getcolptr(A) .- 1) for A in At]
    colind = [Int32.(rowvals(A) .- 1) for A in At]
    vals = [Vector{T}(nonzeros(A)) for A in At]
    Ts = [Matrix{T}(undef, maxdim, maxdim) for _ in 1:p]
    Zs = [Matrix{T}(undef, n, maxdim) for _ in 1:p]
    wr = zeros(maxdim); wi = zeros(maxdim)
    nconv = Ref{Cint}(0); info = Ref{Cint}(0)
    st = zeros(UInt8, 96)
    Tp = _ptrs(Ts); Zp = _ptrs(Zs)
    GC.@preserve rowptr colind vals Ts Zs u wr wi st begin
        Rp = Ptr{Int64}[pointer(r) for r in rowptr]
        Cp = Ptr{Int32}[pointer(c) for c in colind]
        Vp = Ptr{Float64}[Ptr{Float64}(pointer(v)) for v in vals]
        up = u === nothing ? Ptr{Float64}(C_NULL) : Ptr{Float64}(pointer(u))
        args = (ctx().ptr, n, p, Rp, Cp, Vp, nev, _KTARGET[typeof(which)], mindim, maxdim, up, UInt64(seed),
                Float64(tol), Float64(tol1), restarts, purgebuffer, nconv, Tp, Zp, wr, wi, pointer(st), info)
        if T <: Real
            ccall((:psd_d_partial_pschur_csr, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Int64}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Float64}}, Cint, Cchar, Cint, Cint,
                   Ptr{Float64}, UInt64, Cdouble, Cdouble, Cint, Cint, Ref{Cint}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}},
                   Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ref{Cint}), args...)
        else
            ccall((:psd_z_partial_pschur_csr, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Int64}}, Ptr{Ptr{Int32}}, Ptr{Ptr{Float64}}, Cint, Cchar, Cint, Cint,
                   Ptr{Float64}, UInt64, Cdouble, Cdouble, Cint, Cint, Ref{Cint}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}},
                   Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ref{Cint}), args...)
        end
    end
    return _partial_result(info[], Int(nconv[]), Ts, Zs, wr, wi, st, nev)
end


# ---------------------------------------------------------------------------------------------------------------------
# eigvecs_device(ps, select; shifted) — eigvecs (vectors.jl:25-138) by periodic back-substitution on the device
# (psd_d_eigvecs / psd_z_eigvecs): no reordering, one call for all selected vectors.  `select` is completed to whole
# conjugate pairs; the columns come in the order of the selected eigenvalues from top to bottom; ‖V_1[:, j]‖ = 1 with its
# largest entry real and positive.  A zero eigenvalue gives a column of NaNs.  (Signed generalized decompositions are
# not covered: the C ABI returns PSD_INFO_NOTIMPL for them.)
function eigvecs_device(ps::PeriodicSchur{T}, select::AbstractVector{Bool}; shifted::Bool = true) where {T <: BlasElt}
    isempty(ps.Z) && throw(ArgumentError("eigvecs requires Schur vectors in the PSD"))                 # vectors.jl:30-32
    p = ps.period; n = size(ps.T1, 1)
    length(select) == n ||
        throw(ArgumentError("length of `select` must correspond to rank of Schur (sub-)space"))       # vectors.jl:34-36
    Ts = _userT(ps); Zs = ps.Z
    sel = UInt8.(select); info = Ref{Cint}(0); st = zeros(UInt8, 40)  # psd_evec_stats: nvec Int32 first
    Tp = _ptrs(Ts); Zp = _ptrs(Zs)
    wr = Float64.(real.(ps.values)); wi = Float64.(imag.(ps.values))
    α = ComplexF64.(ps.values); β = ones(n); sc = zeros(Int32, n)
    call(Vp, maxvec) = GC.@preserve Ts Zs sel wr wi α β sc st begin
        if T <: Real
            ccall((:psd_d_eigvecs, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8},
                   Cchar, Cint, Ptr{UInt8}, Cint, Cint, Ptr{Ptr{Float64}}, Cint, Ptr{UInt8}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, Zp, wr, wi, C_NULL, ps.orientation, ps.schurindex, sel, n, shifted, Vp, maxvec,
                  pointer(st), info)
        else
            ccall((:psd_z_eigvecs, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{ComplexF64}, Ptr{Float64},
                   Ptr{Int32}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8}, Cint, Cint, Ptr{Ptr{Float64}}, Cint, Ptr{UInt8},
                   Ref{Cint}),
                  ctx().ptr, n, p, Tp, Zp, α, β, sc, C_NULL, ps.orientation, ps.schurindex, sel, n, shifted, Vp,
                  maxvec, pointer(st), info)
        end
    end
    call(Ptr{Ptr{Float64}}(C_NULL), 0)                                                       # size query: completes select
    _throw(info[])
    nvec = Int(reinterpret(Int32, st[1:4])[1])
    Vs = [Matrix{ComplexF64}(undef, n, nvec) for _ in 1:(shifted ? p : 1)]
    GC.@preserve Vs begin
        call(_ptrs(Vs), nvec)
    end
    _throw(info[])
    return shifted ? Vs : Vs[1]
end

# ---------------------------------------------------------------------------------------------------------------------
# geigvecs_device(P, select; shifted) — eigenvectors of signed and singular periodic products (psd_d_geigvecs /
# psd_z_geigvecs), the periodic form of xTGEVC.  Returns (Vs, a): for every column, l + 1 cyclic,
#   'L': A_l v_l = a_l v_{l+1} if S[l], else A_l v_{l+1} = a_l v_l;  'R': the mirror.
# a_l = T_l[k, k] at the eigenvalue's own row (zero and infinite eigenvalues give valid vectors); a conjugate pair of a
# real decomposition takes sqrt|det B_l|, times exp(±im arg λ_k) at schurindex.  `select` is completed to whole pairs;
# ‖V_1[:, j]‖ = 1 with its largest entry real and positive.
function geigvecs_device(P::Union{PeriodicSchur{T}, GeneralizedPeriodicSchur{T}}, select::AbstractVector{Bool};
                         shifted::Bool = true) where {T <: BlasElt}
    isempty(P.Z) && throw(ArgumentError("geigvecs requires Schur vectors in the PSD"))
    p = P.period; n = size(P.T1, 1)
    length(select) == n ||
        throw(ArgumentError("length of `select` must correspond to rank of Schur (sub-)space"))
    Ts = _userT(P); Zs = P.Z
    S = P isa GeneralizedPeriodicSchur ? UInt8.(P.S) : UInt8[]
    length(S) in (0, p) || throw(DimensionMismatch("length of S must match the period"))
    Sp = isempty(S) ? Ptr{UInt8}(C_NULL) : pointer(S)
    sel = UInt8.(select); info = Ref{Cint}(0); st = zeros(UInt8, 40)  # psd_evec_stats: nvec Int32 first
    Tp = _ptrs(Ts); Zp = _ptrs(Zs)
    call(Vp, maxvec, ap) = GC.@preserve Ts Zs S sel st begin
        if T <: Real
            ccall((:psd_d_geigvecs, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8},
                   Cint, Cint, Ptr{Ptr{Float64}}, Cint, Ptr{ComplexF64}, Ptr{UInt8}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, Zp, Sp, P.orientation, P.schurindex, sel, n, shifted, Vp, maxvec, ap,
                  pointer(st), info)
        else
            ccall((:psd_z_geigvecs, libpsd), Cint,
                  (Ptr{Cvoid}, Cint, Cint, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{UInt8}, Cchar, Cint, Ptr{UInt8},
                   Cint, Cint, Ptr{Ptr{Float64}}, Cint, Ptr{ComplexF64}, Ptr{UInt8}, Ref{Cint}),
                  ctx().ptr, n, p, Tp, Zp, Sp, P.orientation, P.schurindex, sel, n, shifted, Vp, maxvec, ap,
                  pointer(st), info)
        end
    end
    call(Ptr{Ptr{Float64}}(C_NULL), 0, Ptr{ComplexF64}(C_NULL))                      # size query: completes select
    _throw(info[])
    nvec = Int(reinterpret(Int32, st[1:4])[1])
    Vs = [Matrix{ComplexF64}(undef, n, nvec) for _ in 1:(shifted ? p : 1)]
    a = Matrix{ComplexF64}(undef, p, max(nvec, 1))                                  # column-major, ld p: as the ABI
    GC.@preserve Vs a begin
        call(_ptrs(Vs), nvec, pointer(a))
    end
    _throw(info[])
    return (shifted ? Vs : Vs[1]), a[:, 1:nvec]
end

end # module
