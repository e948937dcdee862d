# FastConvHIP.jl -- Julia binding of liblsfc.so (include/lsfc.h) that keeps the reference's
# operator surface, so `gmres!(u, fastconv, rhs, Pl=precond)` and `LinearMap(...)` run unchanged
# (examples/example.jl:54-93, examples/example3D.jl:54-79 of the reference).
#
# UNVERIFIED: Julia is not installed in the build image; this file is the binding a maintainer
# would add, kept declarative over the C ABI.  The tested host side is the Python mirror.
module FastConvHIP

using LinearAlgebra
import Base: *, size, eltype

const liblsfc = get(ENV, "LSFC_LIB", joinpath(@__DIR__, "..", "fast_solver_lippmann_schwinger_amd", "liblsfc.so"))
const QUAD = Dict("trapezoidal" => Cint(0), "Greengard_Vico" => Cint(1))

lasterror() = unsafe_string(ccall((:lsfc_last_error, liblsfc), Cstring, ()))
check(rc) = rc == 0 ? nothing : error("lsfc error $rc: $(lasterror())")

mutable struct FastMHIP            # mirrors FastM / FastM3D field names (src/FastConvolution.jl:11-27)
    plan::Ptr{Cvoid}
    nu::Union{Vector{Float64},Vector{Complex{Float64}}}    # complex: an absorbing medium (beyond the reference's Array{Float64,1})
    n::Int64; m::Int64; l::Int64
    omega::Float64
    quadRule::String
    function FastMHIP(plan, nu, n, m, l, omega, quadRule)
        M = new(plan, nu, n, m, l, omega, quadRule)
        finalizer(M -> ccall((:lsfc_plan_destroy, liblsfc), Cint, (Ptr{Cvoid},), M.plan), M)
        return M
    end
end

# Complex nu (lsfc_plan_set_nu_complex): the creators take a real nu, so a complex operator is created with real.(nu) and then
# handed the (re, im) pairs.  A Vector{Float64} takes the real path exactly as before; a Vector{Complex{Float64}} takes the
# complex path even if every imaginary part is 0.  transpose(M) multiplies by nu itself, M' by conj(nu) (include/lsfc.h).
const NuVector = Union{Vector{Float64},Vector{Complex{Float64}}}
_real_nu(nu::Vector{Float64}) = nu
_real_nu(nu::Vector{Complex{Float64}}) = Vector{Float64}(real.(nu))
_nu_vector(v) = eltype(v) <: Complex ? Vector{Complex{Float64}}(vec(v)) : Vector{Float64}(vec(v))
_upload_complex_nu(plan, nu::Vector{Float64}) = nothing
_upload_complex_nu(plan, nu::Vector{Complex{Float64}}) =
    check(ccall((:lsfc_plan_set_nu_complex, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Cint), plan, nu, 0))

# set_nu!(M, nu): replace the contrast (nu is a mutable field of the reference struct); the element type chooses the path
function set_nu!(M::FastMHIP, nu::Vector{Float64})
    length(nu) == length(M.nu) || throw(DimensionMismatch("nu"))
    check(ccall((:lsfc_plan_set_nu, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Float64}, Cint), M.plan, nu, 0))
    M.nu = nu; M
end
function set_nu!(M::FastMHIP, nu::Vector{Complex{Float64}})
    length(nu) == length(M.nu) || throw(DimensionMismatch("nu"))
    _upload_complex_nu(M.plan, nu)
    M.nu = nu; M
end
function nu_is_complex(M::FastMHIP)
    flag = Ref{Cint}(0)
    check(ccall((:lsfc_plan_nu_is_complex, liblsfc), Cint, (Ptr{Cvoid}, Ref{Cint}), M.plan, flag))
    flag[] != 0
end

# FastM(GFFT,nu,ne,me,n,m,k; quadRule) -- src/FastConvolution.jl:24
function FastM(GFFT::Array{Complex{Float64},2}, nu::NuVector, ne, me, n, m, k; quadRule::String="trapezoidal", flags=0, device=0)
    plan = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_plan_create_2d, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Complex{Float64}}, Float64, Cint, Cuint, Cint),
                plan, n, m, ne, me, _real_nu(nu), GFFT, k, QUAD[quadRule], flags, device))
    _upload_complex_nu(plan[], nu)
    FastMHIP(plan[], nu, n, m, 1, k, quadRule)
end

# FastM3D(GFFT,nu,ne,me,le,n,m,l,k; quadRule) -- src/FastConvolution3D.jl:23
function FastM3D(GFFT::Array{Complex{Float64},3}, nu::NuVector, ne, me, le, n, m, l, k; quadRule::String="Greengard_Vico", flags=0, device=0)
    plan = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_plan_create_3d, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Int64, Int64, Int64, Ptr{Float64}, Ptr{Complex{Float64}}, Float64, Cint, Cuint, Cint),
                plan, n, m, l, ne, me, le, _real_nu(nu), GFFT, k, QUAD[quadRule], flags, device))
    _upload_complex_nu(plan[], nu)
    FastMHIP(plan[], nu, n, m, l, k, quadRule)
end

# buildFastConvolution3D(x,y,z,X,Y,Z,h,k,nu) -- src/FastConvolution3D.jl:68 (symbol generated on the device)
function buildFastConvolution3D(x, y, z, X, Y, Z, h, k, nu; quadRule::String="Greengard_Vico", flags=0, device=0)
    nuv = _nu_vector(nu(X, Y, Z)); plan = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_plan_create_gv3d, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Float64, Float64, Ptr{Float64}, Cuint, Cint),
                plan, length(x), length(y), length(z), abs(x[end] - x[1]) + h, k, _real_nu(nuv), flags, device))
    _upload_complex_nu(plan[], nuv)
    FastMHIP(plan[], nuv, length(x), length(y), length(z), k, quadRule)
end

# The same builder on several GPUs, driven from THIS one Julia process (lsfc_plan_create_gv3d_multi): z-slabs over
# `devices` (0-based HIP device ids), RCCL exchanges over xGMI inside the library.  The returned object is an ordinary
# FastMHIP: `*`, `mul!`, `FFTconvolution`, `gmres_hip!`, `bicgstabl_multi_hip!` take and return full host vectors.
function buildFastConvolution3D(x, y, z, X, Y, Z, h, k, nu, devices::Vector{<:Integer}; quadRule::String="Greengard_Vico", flags=0)
    nuv = Vector{Float64}(nu(X, Y, Z)); plan = Ref{Ptr{Cvoid}}(C_NULL); devs = Cint.(devices)
    check(ccall((:lsfc_plan_create_gv3d_multi, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Int64, Int64, Float64, Float64, Ptr{Float64}, Cuint, Ptr{Cint}, Cint),
                plan, length(x), length(y), length(z), abs(x[end] - x[1]) + h, k, nuv, flags, devs, length(devs)))
    FastMHIP(plan[], nuv, length(x), length(y), length(z), k, quadRule)
end

# buildFastConvolution(x,y,h,k,nu; quadRule) -- src/FastConvolution.jl:170
function buildFastConvolution(x, y, h, k, nu::Function; quadRule::String="trapezoidal", flags=0, device=0)
    n, m = length(x), length(y)
    X = repeat(x, 1, m)[:]; Y = repeat(y', n, 1)[:]
    nuv = _nu_vector(nu(X, Y)); plan = Ref{Ptr{Cvoid}}(C_NULL)
    if quadRule == "trapezoidal"
        D = [1-0.892im, 1-1.35im, 1-1.79im, 1-2.23im, 1-2.67im, 1-3.11im]; D0 = D[round(Int, k*h)]
        check(ccall((:lsfc_plan_create_trap2d, liblsfc), Cint,
                    (Ref{Ptr{Cvoid}}, Int64, Int64, Float64, Float64, Float64, Float64, Float64, Float64, Ptr{Float64}, Cuint, Cint),
                    plan, n, m, x[1], y[1], h, k, real(D0), imag(D0), _real_nu(nuv), flags, device))
    else
        check(ccall((:lsfc_plan_create_gv2d, liblsfc), Cint,
                    (Ref{Ptr{Cvoid}}, Int64, Int64, Float64, Float64, Ptr{Float64}, Cuint, Cint),
                    plan, n, m, abs(x[end] - x[1]) + h, k, _real_nu(nuv), flags, device))
    end
    _upload_complex_nu(plan[], nuv)
    FastMHIP(plan[], nuv, n, m, 1, k, quadRule)
end

# traits -- src/FastConvolution.jl:31-41
Base.size(M::FastMHIP, dim) = length(M.nu)
Base.size(M::FastMHIP) = (size(M.nu), size(M.nu))
Base.eltype(::FastMHIP) = Complex{Float64}

# fastconvolution / * / mul! -- src/FastConvolution.jl:43-107, src/FastConvolution3D.jl:31-37
function fastconvolution(M::FastMHIP, b::AbstractArray{Complex{Float64},1})
    x = Vector{Complex{Float64}}(b); y = similar(x)
    check(ccall((:lsfc_apply, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Cint), M.plan, x, y, 0))
    y
end
*(M::FastMHIP, b::AbstractArray{Complex{Float64},1}) = fastconvolution(M, b)
function LinearAlgebra.mul!(Y::AbstractArray{Complex{Float64},1}, M::FastMHIP, b::AbstractArray{Complex{Float64},1})
    Y[:] = M * b
end
# dense vectors (what gmres! hands over): straight into the caller's memory, no temporaries -- at 512^3 the two 2-GB host copies of
# the generic method above cost more than the apply; Y may alias b
function LinearAlgebra.mul!(Y::Vector{Complex{Float64}}, M::FastMHIP, b::Vector{Complex{Float64}})
    check(ccall((:lsfc_apply, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Cint), M.plan, b, Y, 0))
    Y
end
# page-lock long-lived work vectors of the solver (optional; ~4 ms per 512^3 apply): lsfc_host_register / lsfc_host_unregister
host_register!(v::Vector{Complex{Float64}}) = (check(ccall((:lsfc_host_register, liblsfc), Cint, (Ptr{Cvoid}, Csize_t), v, sizeof(v))); v)
host_unregister!(v::Vector{Complex{Float64}}) = (check(ccall((:lsfc_host_unregister, liblsfc), Cint, (Ptr{Cvoid},), v)); v)
# ... or, preferred, work vectors in page-locked memory owned by the HIP runtime (lsfc_host_alloc): page-aligned, no page shared with the heap
function host_vector(N::Integer)
    p = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_host_alloc, liblsfc), Cint, (Ref{Ptr{Cvoid}}, Csize_t), p, N * sizeof(Complex{Float64})))
    v = unsafe_wrap(Vector{Complex{Float64}}, Ptr{Complex{Float64}}(p[]), N; own = false)
    finalizer(_ -> ccall((:lsfc_host_free, liblsfc), Cint, (Ptr{Cvoid},), p[]), v)
    v
end

# FFTconvolution -- src/FastConvolution.jl:110-154 (nu only in the 2D trapezoidal branch), src/FastConvolution3D.jl:39-63
function FFTconvolution(M::FastMHIP, b::Array{Complex{Float64},1})
    y = similar(b); apply_nu = (M.l == 1 && M.quadRule == "trapezoidal") ? 1 : 0
    check(ccall((:lsfc_convolve, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Cint, Cint), M.plan, b, y, apply_nu, 0))
    y
end

# sampleG3D(k,X,Y,Z,indS,fastconv) / sampleGConv -- src/FastConvolution3D.jl:136-160, src/FastConvolution.jl:278-306
# (1-based indS as in the reference; rows of the result are the responses to the delta sources)
function sampleG3D(k, X, Y, Z, indS, M::FastMHIP)
    N = length(M.nu); ns = length(indS)
    out = Array{Complex{Float64}}(undef, N, ns); src = Int64.(indS .- 1)
    check(ccall((:lsfc_sample_sources, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ptr{Complex{Float64}}, Cint), M.plan, src, ns, out, 0))
    return permutedims(out)          # (ns, N) like the reference's Gc
end
sampleGConv(k, X, Y, indS, M::FastMHIP) = sampleG3D(k, X, Y, nothing, indS, M)

# buildSparseA*/buildSparseAG* assembled on the device -- src/SparsifyingMatrix2D.jl:351-532, :806-966,
# src/SparsifyingMatrix3D.jl:1410-1918 -- and Msp = As + k^2 AG diag(nu) (examples/example.jl:67, example3D.jl:61).
# CSR from the library is the CSC of the transpose: build the transpose's CSC, then transpose back.
using SparseArrays
function _sparsify(M::FastMHIP, which::Symbol)
    N = length(M.nu); nnz = Ref{Int64}(0)
    check(ccall((:lsfc_sparsify_pattern, liblsfc), Cint, (Int64, Int64, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                M.n, M.m, M.l, nnz, C_NULL, C_NULL, C_NULL))
    rowptr = Vector{Int64}(undef, N + 1); col = Vector{Int64}(undef, nnz[]); val = Vector{Complex{Float64}}(undef, nnz[])
    ptrs = [which == w ? pointer(val) : Ptr{Complex{Float64}}(C_NULL) for w in (:As, :AG, :Msp)]
    check(ccall((:lsfc_sparsify_build, liblsfc), Cint,
                (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Ptr{Float64}, Cint),
                M.plan, rowptr, col, ptrs[1], ptrs[2], ptrs[3], C_NULL, 0))
    return copy(transpose(SparseMatrixCSC(N, N, rowptr .+ 1, col .+ 1, val)))
end
function _check_k(k, M::FastMHIP)
    k == M.omega || throw(ArgumentError("k = $k differs from the k of the fast convolution ($(M.omega))"))
end
buildSparseAConv(k, X, Y, M::FastMHIP, n, m) = (_check_k(k, M); _sparsify(M, :As))
buildSparseAGConv(k, X, Y, M::FastMHIP, n, m) = (_check_k(k, M); _sparsify(M, :AG))
buildSparseA3DConv(k, X, Y, Z, M::FastMHIP, n, m, l) = (_check_k(k, M); _sparsify(M, :As))
buildSparseAG3DConv(k, X, Y, Z, M::FastMHIP, n, m, l) = (_check_k(k, M); _sparsify(M, :AG))
# Msp and As of one device call, for SparsifyingPreconditioner(Msp, As) / SparsifyingPreconditionerHIP(Msp, As)
sparsifying_pair(M::FastMHIP) = (_sparsify(M, :Msp), _sparsify(M, :As))
# the direct-sampling builders (sampleG rows with the caller's D0): a trapezoidal plan with nu = 0 on the grid
# (sampleG reads distances only: the plan is made for the same grid centred at the origin, where the builder's kernel is even)
function _direct_plan(k, X, Y, D0, n, m)
    plan = Ref{Ptr{Cvoid}}(C_NULL); nuv = zeros(n * m)
    h = abs(X[2] - X[1])
    check(ccall((:lsfc_plan_create_trap2d, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Int64, Float64, Float64, Float64, Float64, Float64, Float64, Ptr{Float64}, Cuint, Cint),
                plan, n, m, -(n - 1) / 2 * h, -(m - 1) / 2 * h, h, k, real(D0), imag(D0), nuv, 0, 0))
    FastMHIP(plan[], nuv, n, m, 1, k, "trapezoidal")
end
buildSparseA(k, X, Y, D0, n, m) = _sparsify(_direct_plan(k, X, Y, D0, n, m), :As)
buildSparseAG(k, X, Y, D0, n, m) = _sparsify(_direct_plan(k, X, Y, D0, n, m), :AG)

# SparsifyingPreconditioner(Msp, As) with the apply on the device -- src/preconditioner.jl:27-58, 132-170.
# lu(Msp) stays on the host (UMFPACK, as in the reference); its factors go to the device once:
# (F.Rs .* Msp)[F.p, F.q] == F.L * F.U.  CSR arrays of a SparseMatrixCSC X are the CSC arrays of transpose(X).
using SparseArrays
mutable struct SparsifyingPreconditionerHIP
    pc::Ptr{Cvoid}
    N::Int64
end
_csr(X) = (T = sparse(transpose(X)); (Int64.(T.colptr .- 1), Int64.(T.rowval .- 1), Vector{Complex{Float64}}(T.nzval)))
function SparsifyingPreconditionerHIP(Msp::SparseMatrixCSC{Complex{Float64},Int64}, As::SparseMatrixCSC{Complex{Float64},Int64}; device=0)
    F = lu(Msp); N = size(Msp, 1)
    (ap, ac, av) = _csr(As); (lp, lc, lv) = _csr(F.L); (up, uc, uv) = _csr(F.U)
    p = Int64.(F.p .- 1); q = Int64.(F.q .- 1); Rs = Vector{Float64}(F.Rs)
    pc = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_precond_create, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Complex{Float64}}, Ptr{Int64}, Ptr{Int64}, Ptr{Complex{Float64}},
                 Ptr{Int64}, Ptr{Int64}, Ptr{Complex{Float64}}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Cint),
                pc, N, ap, ac, av, lp, lc, lv, up, uc, uv, p, q, Rs, device))
    P = SparsifyingPreconditionerHIP(pc[], N)
    finalizer(P -> ccall((:lsfc_precond_destroy, liblsfc), Cint, (Ptr{Cvoid},), P.pc), P)
    return P
end
# The same object factorised ON THE DEVICE (lsfc_precond_create_blocktri / lsfc_precond_create_from_plan): block-tridiagonal
# elimination with the slowest grid axis as block index instead of lu(Msp).  Msp and As must share one pattern, as
# buildSparseA* / buildSparseAG* return it.  examples/example3D.jl:57-68 in one call: SparsifyingPreconditionerHIP(fastconv).
function _wrap_precond(pc::Ptr{Cvoid}, N)
    P = SparsifyingPreconditionerHIP(pc, N)
    finalizer(P -> ccall((:lsfc_precond_destroy, liblsfc), Cint, (Ptr{Cvoid},), P.pc), P)
    return P
end
# inverse_type: Complex{Float64} (default, LSFC_PRECOND_INV_F64) or Complex{Float32} (LSFC_PRECOND_INV_F32): the storage of the
# dense inverses S_k^{-1}.  The factorisation is fp64 either way; float storage rounds each inverse once and halves the memory.
function _inverse_precision(T)
    T === Complex{Float64} && return Cint(0)
    T === Complex{Float32} && return Cint(1)
    throw(ArgumentError("inverse_type must be Complex{Float64} or Complex{Float32}"))
end
# pivoting: :none (default, LSFC_PRECOND_PIVOT_NONE), :partial (partial row pivoting inside every Schur block) or :auto (without
# pivoting first; after a breakdown the whole factorisation again with :partial).  The options travel as lsfc_blocktri_opts:
# eight Cints (inverse_precision, pivoting, six reserved zeros).
function _blocktri_opts(inverse_type, pivoting)
    piv = pivoting === :none ? Cint(0) : pivoting === :partial ? Cint(1) : pivoting === :auto ? Cint(2) :
          throw(ArgumentError("pivoting must be :none, :partial or :auto"))
    return Cint[_inverse_precision(inverse_type), piv, 0, 0, 0, 0, 0, 0]
end
function SparsifyingPreconditionerHIP(Msp::SparseMatrixCSC{Complex{Float64},Int64}, As::SparseMatrixCSC{Complex{Float64},Int64}, nblocks::Integer;
                                      device=0, inverse_type=Complex{Float64}, pivoting=:none)
    opts = _blocktri_opts(inverse_type, pivoting)
    N = size(Msp, 1)
    (mp, mc, mv) = _csr(Msp); (ap, ac, av) = _csr(As)
    (mp == ap && mc == ac) || throw(DimensionMismatch("Msp and As must share one sparsity pattern"))
    pc = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_precond_create_blocktri_opts, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Int64, Int64, Ptr{Int64}, Ptr{Int64}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Cint, Cint, Ptr{Cint}),
                pc, N, nblocks, mp, mc, av, mv, 0, device, opts))
    return _wrap_precond(pc[], N)
end
function SparsifyingPreconditionerHIP(M::FastMHIP; inverse_type=Complex{Float64}, pivoting=:none)
    opts = _blocktri_opts(inverse_type, pivoting)
    pc = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_precond_create_from_plan_opts, liblsfc), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cint}), pc, M.plan, opts))
    return _wrap_precond(pc[], size(M, 1))
end
# Complex{Float64} or Complex{Float32}: how the object stores its inverses (lsfc_precond_inverse_precision)
function inverse_type(P::SparsifyingPreconditionerHIP)
    prec = Ref{Cint}(-1)
    check(ccall((:lsfc_precond_inverse_precision, liblsfc), Cint, (Ptr{Cvoid}, Ref{Cint}), P.pc, prec))
    return prec[] == 1 ? Complex{Float32} : Complex{Float64}
end
# (blocks, block size, bytes of the inverses, launches per apply, factorisation microseconds, pivoting used), min |pivot| / max|S_k|
function blocktri_info(P::SparsifyingPreconditionerHIP)
    out = zeros(Int64, 6); r = Ref{Float64}(0.0)
    check(ccall((:lsfc_precond_blocktri_info, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ref{Float64}), P.pc, out, r))
    return out, r[]
end
# S_k^{-1} (k 0-based), b x b, as stored (float storage: widened to Complex{Float64})
function blocktri_block(P::SparsifyingPreconditionerHIP, k::Integer)
    b = blocktri_info(P)[1][2]; S = Matrix{Complex{Float64}}(undef, b, b)
    check(ccall((:lsfc_precond_blocktri_get_block, liblsfc), Cint, (Ptr{Cvoid}, Int64, Ptr{Complex{Float64}}, Int64), P.pc, k, S, b * b))
    return S
end
# perm of block k (k 0-based, entries 0-based): perm[i + 1] = row of S_k that became pivot row i; the identity without pivoting
function blocktri_pivots(P::SparsifyingPreconditionerHIP, k::Integer)
    b = blocktri_info(P)[1][2]; perm = Vector{Int64}(undef, b)
    check(ccall((:lsfc_precond_blocktri_get_pivots, liblsfc), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Int64), P.pc, k, perm, b))
    return perm
end
# ldiv!(P, b): host vector in, host vector out (staged over PCIe); inside gmres_hip! the device path is used instead
function LinearAlgebra.ldiv!(P::SparsifyingPreconditionerHIP, b::Vector{Complex{Float64}})
    check(ccall((:lsfc_precond_apply, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Cint), P.pc, b, 0)); b
end
Base.:\(P::SparsifyingPreconditionerHIP, b::Vector{Complex{Float64}}) = ldiv!(P, copy(b))
# ldiv_batch!(P, B): every column of B (N x nrhs) <- Msp^{-1} (As column), lsfc_precond_apply_batch: a block-tridiagonal object
# takes groups of up to 8 columns through one sweep that reads every S_k^{-1} once; a column's result does not depend on the others
function ldiv_batch!(P::SparsifyingPreconditionerHIP, B::Matrix{Complex{Float64}})
    size(B, 1) == P.N && size(B, 2) >= 1 || throw(DimensionMismatch("B must be $(P.N) x nrhs with nrhs >= 1"))
    check(ccall((:lsfc_precond_apply_batch, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Int64, Cint), P.pc, B, size(B, 2), 0)); B
end
# (group sweeps enqueued, vectors that went through them, largest group, bytes of group work buffers)
function batch_info(P::SparsifyingPreconditionerHIP)
    out = zeros(Int64, 4)
    check(ccall((:lsfc_precond_batch_info, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Int64}), P.pc, out))
    return Tuple(out)
end

# Device-side GMRES with a host preconditioner: Pl is anything with the two-argument ldiv!(Pl, v)
# (src/preconditioner.jl:147-170), passed through @cfunction.
# C layout of lsfc_gmres_opts / lsfc_gmres_result (include/lsfc.h), field: byte offset -- tests/test_abi.py compiles the same
# table as static_asserts against the header and checks that this comment agrees with it (Julia lays isbits structs out like C)
# ABI-LAYOUT lsfc_gmres_opts size=64 restart:0 maxiter:8 reltol:16 abstol:24 orth:32 initially_zero:36 precond:40 precond_user:48 precond_on_device:56
# ABI-LAYOUT lsfc_gmres_result size=32 iters:0 mvps:8 converged:16 final_resnorm:24
struct GmresOpts
    restart::Cint; maxiter::Int64; reltol::Float64; abstol::Float64; orth::Cint; initially_zero::Cint
    precond::Ptr{Cvoid}; precond_user::Ptr{Cvoid}; precond_on_device::Cint
end
struct GmresResult
    iters::Int64; mvps::Int64; converged::Cint; final_resnorm::Float64
end
function _precond_trampoline(user::Ptr{Cvoid}, v::Ptr{Float64}, n::Int64)::Cint
    Pl = unsafe_pointer_to_objref(user)[]
    ldiv!(Pl, unsafe_wrap(Array, Ptr{Complex{Float64}}(v), n))
    return Cint(0)
end
# on M itself a wrapper transpose(P) / P' (defined with the operator wrappers below) is a mismatch of ops
_own_on_m(Pl) = Pl isa PrecondHIPView &&
    throw(ArgumentError("transpose(P) and P' approximate the inverses of transpose(M) and M': pass them with the operator wrapper of the same kind"))
function gmres_hip!(x::Vector{Complex{Float64}}, M::FastMHIP, b::Vector{Complex{Float64}}; Pl=nothing, restart=min(20, length(b)),
                    maxiter=length(b), reltol=sqrt(eps(Float64)), abstol=0.0, initially_zero=false)
    _own_on_m(Pl)
    box = Ref{Any}(Pl)
    if Pl isa SparsifyingPreconditionerHIP        # applied on the device by the library itself: no PCIe, no Julia in the loop
        cb = cglobal((:lsfc_precond_callback, liblsfc)); user = Pl.pc; ondev = Cint(1)
    else
        cb = Pl === nothing ? C_NULL : @cfunction(_precond_trampoline, Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64))
        user = Pl === nothing ? C_NULL : pointer_from_objref(box); ondev = Cint(0)
    end
    opts = Ref(GmresOpts(restart, maxiter, reltol, abstol, 0, initially_zero ? 1 : 0, cb, user, ondev))
    res = Ref(GmresResult(0, 0, 0, 0.0)); resnorm = zeros(Float64, maxiter)
    GC.@preserve box begin
        rc = ccall((:lsfc_gmres, liblsfc), Cint,
                   (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Ref{GmresOpts}, Ptr{Float64}, Int64, Ref{GmresResult}, Cint),
                   M.plan, x, b, opts, resnorm, maxiter, res, 0)
        (rc == 0 || rc == -5) || check(rc)
    end
    x, resnorm[1:res[].iters]
end

# The solves of several incident directions (tests/plasma_example.jl:160-176) in lock step, lsfc_gmres_batch: columns of B,
# solutions in the columns of X.  A SparsifyingPreconditionerHIP is applied on the device to all unconverged columns at
# once (one group sweep per step for a block-tridiagonal object); any other Pl gets one host vector at a time.
function gmres_batch_hip!(X::Matrix{Complex{Float64}}, M::FastMHIP, B::Matrix{Complex{Float64}}; Pl=nothing, restart=min(20, size(B, 1)),
                          maxiter=size(B, 1), reltol=sqrt(eps(Float64)), abstol=0.0, initially_zero=false)
    size(X) == size(B) || throw(DimensionMismatch("X and B"))
    nrhs = size(B, 2)
    _own_on_m(Pl)
    box = Ref{Any}(Pl)
    if Pl isa SparsifyingPreconditionerHIP
        cb = cglobal((:lsfc_precond_callback, liblsfc)); user = Pl.pc; ondev = Cint(1)
    else
        cb = Pl === nothing ? C_NULL : @cfunction(_precond_trampoline, Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64))
        user = Pl === nothing ? C_NULL : pointer_from_objref(box); ondev = Cint(0)
    end
    opts = Ref(GmresOpts(restart, maxiter, reltol, abstol, 0, initially_zero ? 1 : 0, cb, user, ondev))
    res = fill(GmresResult(0, 0, 0, 0.0), nrhs); resnorm = zeros(Float64, maxiter, nrhs)
    GC.@preserve box begin
        check(ccall((:lsfc_gmres_batch, liblsfc), Cint,
                    (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Int64, Ref{GmresOpts}, Ptr{Float64}, Int64, Ptr{GmresResult}, Cint),
                    M.plan, X, B, nrhs, opts, resnorm, maxiter, res, 0))
    end
    X, [resnorm[1:res[j].iters, j] for j in 1:nrhs]
end

# Device-side BiCGStab(l), lsfc_bicgstabl: IterativeSolvers.bicgstabl!(x, A, b, l; Pl, max_mv_products, abstol, reltol) with
# the upstream keyword names.  2 l + 3 device work vectors whatever the iteration count (gmres_hip! keeps restart + 2): the
# solver for grids whose Krylov basis does not fit.  Defaults as upstream: l = 2 (1..8 here), reltol sqrt(eps), abstol 0,
# max_mv_products = length(b).  DEPARTURE: the shadow residual is the preconditioned initial residual, not rand -- or the
# keyword r_shadow -- so a solve is reproducible bit for bit.  Returns x and one residual norm per cycle (l BiCG steps and one
# minimal-residual step, 2 l operator applications).  A breakdown (rho, sigma or gamma zero where it divides, or not finite)
# ends the solve with x the last finite iterate; like the cap it shows as a history that stops above the tolerance (rc -5).
# `log` is accepted for the upstream signature: true (the default here, as gmres_hip! always does) returns (x, history), false x alone.
# bicgstabl_multi_hip! (lsfc_bicgstabl_multi) is the same solve on a multi-device plan (buildFastConvolution3D(..., devices)), the
# slabs of the 2 l + 3 work vectors on their devices: x, b, r_shadow are the full host vectors, Pl is nothing or a host
# preconditioner (ldiv!(Pl, v) on the WHOLE vector through the trampoline); a SparsifyingPreconditionerHIP there is refused by the
# library ("a multi-device plan takes a host preconditioner callback").  bicgstabl_hip! and bicgstabl_batch_hip! refuse such a plan, as
# before.  Memory: (2 l + 3 + 2) N / P complex per rank, checked by the library per device.  UNVERIFIED like the rest of this file:
# written against include/lsfc.h.
# ABI-LAYOUT lsfc_bicgstabl_opts size=88 l:0 max_mv_products:8 reltol:16 abstol:24 initially_zero:32 precond:40 precond_user:48 precond_on_device:56 r_shadow:64 reserved:72
struct BicgstablOpts
    l::Cint; max_mv_products::Int64; reltol::Float64; abstol::Float64; initially_zero::Cint
    precond::Ptr{Cvoid}; precond_user::Ptr{Cvoid}; precond_on_device::Cint; r_shadow::Ptr{Cvoid}; reserved::NTuple{4, Cint}
end
function bicgstabl_hip!(x::Vector{Complex{Float64}}, M::FastMHIP, b::Vector{Complex{Float64}}, l::Int=2; Pl=nothing,
                        max_mv_products=length(b), abstol=0.0, reltol=sqrt(eps(Float64)), log::Bool=true, initially_zero=false, r_shadow=nothing,
                        _multi::Bool=false)
    _own_on_m(Pl)
    box = Ref{Any}(Pl)
    if Pl isa SparsifyingPreconditionerHIP        # applied on the device by the library itself: no host code inside the BiCG part
        cb = cglobal((:lsfc_precond_callback, liblsfc)); user = Pl.pc; ondev = Cint(1)
    else
        cb = Pl === nothing ? C_NULL : @cfunction(_precond_trampoline, Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64))
        user = Pl === nothing ? C_NULL : pointer_from_objref(box); ondev = Cint(0)
    end
    shadow = r_shadow === nothing ? Complex{Float64}[] : convert(Vector{Complex{Float64}}, r_shadow)
    r_shadow === nothing || length(shadow) == length(b) || throw(DimensionMismatch("r_shadow"))
    # one history entry per cycle of 2 l operator applications, capped as the Python surface caps it
    cap = max(1, min(div(max_mv_products > 0 ? max_mv_products : length(b), 2 * max(l, 1)) + 2, 1 << 20))
    res = Ref(GmresResult(0, 0, 0, 0.0)); resnorm = zeros(Float64, cap)
    GC.@preserve box shadow begin
        opts = Ref(BicgstablOpts(l, max_mv_products, reltol, abstol, initially_zero ? 1 : 0, cb, user, ondev,
                                 r_shadow === nothing ? C_NULL : Ptr{Cvoid}(pointer(shadow)), (Cint(0), Cint(0), Cint(0), Cint(0))))
        rc = _multi ?
             ccall((:lsfc_bicgstabl_multi, liblsfc), Cint,
                   (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Ref{BicgstablOpts}, Ptr{Float64}, Int64, Ref{GmresResult}, Cint),
                   M.plan, x, b, opts, resnorm, cap, res, 0) :
             ccall((:lsfc_bicgstabl, liblsfc), Cint,
                   (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Ref{BicgstablOpts}, Ptr{Float64}, Int64, Ref{GmresResult}, Cint),
                   M.plan, x, b, opts, resnorm, cap, res, 0)
        (rc == 0 || rc == -5) || check(rc)
    end
    log ? (x, resnorm[1:min(res[].iters, cap)]) : x
end
bicgstabl_multi_hip!(x::Vector{Complex{Float64}}, M::FastMHIP, b::Vector{Complex{Float64}}, l::Int=2; kw...) =
    bicgstabl_hip!(x, M, b, l; _multi=true, kw...)

# bicgstabl_hip! for several right-hand sides in lock step, lsfc_bicgstabl_batch: columns of B, solutions in the columns of
# X, r_shadow (optional) one shadow residual per column.  Every step of a cycle is one launch over the columns still
# running; each column has its own tolerance and stopping test and leaves when it has converged, broken down or reached
# max_mv_products.  A SparsifyingPreconditionerHIP takes the running columns in group sweeps; any other Pl gets one host
# vector at a time.  Returns (X, histories, status): status[:, j] = (LSFC_BICG_* code, cycle) of column j (0 converged,
# 1 max_mv_products, 2..7 the scalar of a breakdown: rho, sigma, beta, alpha, gamma, residual).  At most 64 columns.
function bicgstabl_batch_hip!(X::Matrix{Complex{Float64}}, M::FastMHIP, B::Matrix{Complex{Float64}}, l::Int=2; Pl=nothing,
                              max_mv_products=size(B, 1), abstol=0.0, reltol=sqrt(eps(Float64)), initially_zero=false, r_shadow=nothing)
    size(X) == size(B) || throw(DimensionMismatch("X and B"))
    nrhs = size(B, 2)
    _own_on_m(Pl)
    box = Ref{Any}(Pl)
    if Pl isa SparsifyingPreconditionerHIP
        cb = cglobal((:lsfc_precond_callback, liblsfc)); user = Pl.pc; ondev = Cint(1)
    else
        cb = Pl === nothing ? C_NULL : @cfunction(_precond_trampoline, Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64))
        user = Pl === nothing ? C_NULL : pointer_from_objref(box); ondev = Cint(0)
    end
    shadow = r_shadow === nothing ? zeros(Complex{Float64}, 0, 0) : convert(Matrix{Complex{Float64}}, r_shadow)
    r_shadow === nothing || size(shadow) == size(B) || throw(DimensionMismatch("r_shadow"))
    cap = max(1, min(div(max_mv_products > 0 ? max_mv_products : size(B, 1), 2 * max(l, 1)) + 2, 1 << 20))
    res = fill(GmresResult(0, 0, 0, 0.0), nrhs); resnorm = zeros(Float64, cap, nrhs); status = zeros(Int64, 2, nrhs)
    GC.@preserve box shadow begin
        opts = Ref(BicgstablOpts(l, max_mv_products, reltol, abstol, initially_zero ? 1 : 0, cb, user, ondev,
                                 r_shadow === nothing ? C_NULL : Ptr{Cvoid}(pointer(shadow)), (Cint(0), Cint(0), Cint(0), Cint(0))))
        check(ccall((:lsfc_bicgstabl_batch, liblsfc), Cint,
                    (Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Int64, Ref{BicgstablOpts}, Ptr{Float64}, Int64, Ptr{GmresResult},
                     Ptr{Int64}, Cint), M.plan, X, B, nrhs, opts, resnorm, cap, res, status, 0))
    end
    X, [resnorm[1:min(res[j].iters, cap), j] for j in 1:nrhs], status
end

# transpose(M) and M' -- lsfc_plan_set_op (include/lsfc.h).  omega is real and the Green's matrix is complex symmetric, so
# transpose(M) = I + omega^2 diag(nu) G and M' y = conj(transpose(M) conj(y)) (a complex nu enters M' conjugated): the same pipeline with the nu multiply moved from
# the first x pass to the last, plus two conjugations for M'.  The wrappers hold the parent and an op, no second plan; a call
# through one sets the op of the parent's plan, calls, and restores M (also when the call throws).  The library measures the
# symmetry of G through the plan's own convolution at the first such call and refuses (rc -1) a plan whose symbol is not
# symmetric; distributed and multi-device plans are refused too.  A SparsifyingPreconditionerHIP approximates inv(M), not its
# transpose: with an operator wrapper the solvers take transpose(P) / P' of it (below) and refuse P itself.  conj(M) is not
# offered: transpose(M') and (transpose(M))' throw.
const OP_N = Cint(0); const OP_T = Cint(1); const OP_H = Cint(2)
struct TransposeFastMHIP; parent::FastMHIP; end
struct AdjointFastMHIP; parent::FastMHIP; end
const FastMHIPView = Union{TransposeFastMHIP, AdjointFastMHIP}
_op(::TransposeFastMHIP) = OP_T
_op(::AdjointFastMHIP) = OP_H
LinearAlgebra.transpose(M::FastMHIP) = TransposeFastMHIP(M)
LinearAlgebra.adjoint(M::FastMHIP) = AdjointFastMHIP(M)
LinearAlgebra.transpose(V::TransposeFastMHIP) = V.parent
LinearAlgebra.adjoint(V::AdjointFastMHIP) = V.parent
LinearAlgebra.transpose(::AdjointFastMHIP) = error("conj(M) is not offered (only M, transpose(M) and M')")
LinearAlgebra.adjoint(::TransposeFastMHIP) = error("conj(M) is not offered (only M, transpose(M) and M')")
Base.size(V::FastMHIPView, dim) = size(V.parent, dim)
Base.size(V::FastMHIPView) = size(V.parent)
Base.eltype(::FastMHIPView) = Complex{Float64}
function _with_op(f, V::FastMHIPView)
    check(ccall((:lsfc_plan_set_op, liblsfc), Cint, (Ptr{Cvoid}, Cint), V.parent.plan, _op(V)))
    try
        return f(V.parent)
    finally
        ccall((:lsfc_plan_set_op, liblsfc), Cint, (Ptr{Cvoid}, Cint), V.parent.plan, OP_N)
    end
end
*(V::FastMHIPView, b::AbstractArray{Complex{Float64},1}) = _with_op(M -> fastconvolution(M, b), V)
LinearAlgebra.mul!(Y::AbstractArray{Complex{Float64},1}, V::FastMHIPView, b::AbstractArray{Complex{Float64},1}) = (Y[:] = V * b)
LinearAlgebra.mul!(Y::Vector{Complex{Float64}}, V::FastMHIPView, b::Vector{Complex{Float64}}) = _with_op(M -> mul!(Y, M, b), V)
function symmetry_defect(M::FastMHIP)
    d = Ref{Float64}(0.0)
    check(ccall((:lsfc_plan_symmetry_defect, liblsfc), Cint, (Ptr{Cvoid}, Ref{Float64}), M.plan, d))
    d[]
end

# transpose(P) and P' of a block-tridiagonal SparsifyingPreconditionerHIP -- lsfc_precond_set_op (include/lsfc.h): As^T Msp^-T from
# the same stored inverses, which approximates inv(transpose(M)), and its conjugated form for M'.  Small wrappers, parent plus op, no
# second object: ldiv! through one sets the op of the parent's object, applies, and restores P (also when the call throws).  The
# library refuses (rc -1) an object of the host-LU route.  The solvers take a wrapper as Pl with the operator wrapper of the same
# op (transpose(M) with transpose(P), M' with P') and throw otherwise.  conj(P) is not offered.
# NOTE: like the rest of this binding the wrappers are written against include/lsfc.h and have not been executed (no Julia
# toolchain where the library is built and tested).
struct TransposePrecondHIP; parent::SparsifyingPreconditionerHIP; end
struct AdjointPrecondHIP; parent::SparsifyingPreconditionerHIP; end
const PrecondHIPView = Union{TransposePrecondHIP, AdjointPrecondHIP}
_op(::TransposePrecondHIP) = OP_T
_op(::AdjointPrecondHIP) = OP_H
_op(::Any) = OP_N
LinearAlgebra.transpose(P::SparsifyingPreconditionerHIP) = TransposePrecondHIP(P)
LinearAlgebra.adjoint(P::SparsifyingPreconditionerHIP) = AdjointPrecondHIP(P)
LinearAlgebra.transpose(V::TransposePrecondHIP) = V.parent
LinearAlgebra.adjoint(V::AdjointPrecondHIP) = V.parent
LinearAlgebra.transpose(::AdjointPrecondHIP) = error("conj(P) is not offered (only P, transpose(P) and P')")
LinearAlgebra.adjoint(::TransposePrecondHIP) = error("conj(P) is not offered (only P, transpose(P) and P')")
function _with_op(f, V::PrecondHIPView)
    check(ccall((:lsfc_precond_set_op, liblsfc), Cint, (Ptr{Cvoid}, Cint), V.parent.pc, _op(V)))
    try
        return f(V.parent)
    finally
        ccall((:lsfc_precond_set_op, liblsfc), Cint, (Ptr{Cvoid}, Cint), V.parent.pc, OP_N)
    end
end
LinearAlgebra.ldiv!(V::PrecondHIPView, b::Vector{Complex{Float64}}) = _with_op(P -> ldiv!(P, b), V)
Base.:\(V::PrecondHIPView, b::Vector{Complex{Float64}}) = ldiv!(V, copy(b))
ldiv_batch!(V::PrecondHIPView, B::Matrix{Complex{Float64}}) = _with_op(P -> ldiv_batch!(P, B), V)

# a solver call on the operator wrapper V with Pl: the library's own object needs the op of V (a wrapper of the same kind) and holds it
# for the call; anything else is a caller's ldiv! and passes through
_own_precond(Pl) = Pl isa SparsifyingPreconditionerHIP || Pl isa PrecondHIPView
function _solve_with_ops(f, V, Pl)
    _own_precond(Pl) && _op(Pl) != _op(V) &&
        throw(ArgumentError("Pl approximates the inverse of another form of M than the operator given: use transpose(P) with transpose(M), P' with M'"))
    Pl isa PrecondHIPView || return f(Pl)
    _with_op(P -> f(P), Pl)
end
function gmres_hip!(x::Vector{Complex{Float64}}, V::FastMHIPView, b::Vector{Complex{Float64}}; Pl=nothing, kw...)
    _solve_with_ops(P -> _with_op(M -> gmres_hip!(x, M, b; Pl=P, kw...), V), V, Pl)
end
function gmres_batch_hip!(X::Matrix{Complex{Float64}}, V::FastMHIPView, B::Matrix{Complex{Float64}}; Pl=nothing, kw...)
    _solve_with_ops(P -> _with_op(M -> gmres_batch_hip!(X, M, B; Pl=P, kw...), V), V, Pl)
end
function bicgstabl_hip!(x::Vector{Complex{Float64}}, V::FastMHIPView, b::Vector{Complex{Float64}}, l::Int=2; Pl=nothing, kw...)
    _solve_with_ops(P -> _with_op(M -> bicgstabl_hip!(x, M, b, l; Pl=P, kw...), V), V, Pl)
end
function bicgstabl_batch_hip!(X::Matrix{Complex{Float64}}, V::FastMHIPView, B::Matrix{Complex{Float64}}, l::Int=2; Pl=nothing, kw...)
    _solve_with_ops(P -> _with_op(M -> bicgstabl_batch_hip!(X, M, B, l; Pl=P, kw...), V), V, Pl)
end

# Off-grid sources and receivers -- lsfc_receivers_* (include/lsfc.h): the dense nrecv x N sampling operator R between grid
# vectors and point receivers (points = ...) or far-field directions (directions = ...), never stored.  The reference's drivers
# build u_inc on the host and stop at the total field on the grid (examples/example3D.jl:46-50, :78-81); R * q, transpose(R) * w
# and R' * w are what comes after and before.  x, y[, z]: the axis vectors given to buildFastConvolution[3D]; coordinates: one
# receiver per COLUMN (ndim x nrecv, which is nrecv * ndim doubles receiver after receiver, as the C ABI takes them).
# scattered_field(R, M, u) = -omega^2 R (nu .* u) for the total field u, with the medium of M fused into the kernel.
# NOTE: like the rest of this binding this section is written against include/lsfc.h and has not been executed (no Julia
# toolchain where the library is built and tested).
const RECV_POINTS = Cint(0); const RECV_FARFIELD = Cint(1)
mutable struct ReceiversHIP
    rc::Ptr{Cvoid}
    N::Int64
    nrecv::Int64
    function ReceiversHIP(rc, N, nrecv)
        R = new(rc, N, nrecv)
        finalizer(R -> ccall((:lsfc_receivers_destroy, liblsfc), Cint, (Ptr{Cvoid},), R.rc), R)
        return R
    end
end
function Receivers(x, y, z=nothing; k, points=nothing, directions=nothing, device=0)
    (points === nothing) != (directions === nothing) || throw(ArgumentError("give exactly one of points and directions"))
    axes = z === nothing ? (x, y) : (x, y, z)
    ndim = length(axes)
    h = Float64(x[2] - x[1])
    dims = Int64[length(a) for a in axes]; append!(dims, ones(Int64, 3 - ndim))
    origin = Float64[a[1] for a in axes]; append!(origin, zeros(3 - ndim))
    coords = Matrix{Float64}(points === nothing ? directions : points)
    size(coords, 1) == ndim || throw(DimensionMismatch("coordinates: one receiver per column, $ndim rows"))
    rc = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:lsfc_receivers_create, liblsfc), Cint,
                (Ref{Ptr{Cvoid}}, Cint, Ptr{Int64}, Ptr{Float64}, Float64, Float64, Cint, Ptr{Float64}, Int64, Cint),
                rc, ndim, dims, origin, h, Float64(k), points === nothing ? RECV_FARFIELD : RECV_POINTS, coords, size(coords, 2), device))
    return ReceiversHIP(rc[], prod(dims), size(coords, 2))
end
struct TransposeReceiversHIP; parent::ReceiversHIP; end
struct AdjointReceiversHIP; parent::ReceiversHIP; end
_op(::TransposeReceiversHIP) = OP_T
_op(::AdjointReceiversHIP) = OP_H
LinearAlgebra.transpose(R::ReceiversHIP) = TransposeReceiversHIP(R)
LinearAlgebra.adjoint(R::ReceiversHIP) = AdjointReceiversHIP(R)
Base.size(R::ReceiversHIP) = (R.nrecv, R.N)
Base.size(V::Union{TransposeReceiversHIP,AdjointReceiversHIP}) = (V.parent.N, V.parent.nrecv)
Base.eltype(::Union{ReceiversHIP,TransposeReceiversHIP,AdjointReceiversHIP}) = Complex{Float64}
function receivers_info(R::ReceiversHIP)       # N, nrecv, receivers per thread, receivers per LDS chunk, members per group, table bytes
    out = zeros(Int64, 6)
    check(ccall((:lsfc_receivers_info, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Int64}), R.rc, out))
    return out
end
# columns of B through R (op N), transpose(R) or R'; plan: C_NULL, or the plan whose medium is fused in
function _receivers_apply!(Y::VecOrMat{Complex{Float64}}, R::ReceiversHIP, plan::Ptr{Cvoid}, B::VecOrMat{Complex{Float64}}, op::Cint)
    nin, nout = op == OP_N ? (R.N, R.nrecv) : (R.nrecv, R.N)
    (size(B, 1) == nin && size(Y, 1) == nout && size(B, 2) == size(Y, 2)) || throw(DimensionMismatch("receivers apply"))
    check(ccall((:lsfc_receivers_apply, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Complex{Float64}}, Ptr{Complex{Float64}}, Int64, Cint, Cint),
                R.rc, plan, B, Y, size(B, 2), op, 0))
    return Y
end
_out(R::ReceiversHIP, B, op) = zeros(Complex{Float64}, op == OP_N ? R.nrecv : R.N, size(B)[2:end]...)
*(R::ReceiversHIP, q::VecOrMat{Complex{Float64}}) = _receivers_apply!(_out(R, q, OP_N), R, C_NULL, q, OP_N)
*(V::Union{TransposeReceiversHIP,AdjointReceiversHIP}, w::VecOrMat{Complex{Float64}}) = _receivers_apply!(_out(V.parent, w, _op(V)), V.parent, C_NULL, w, _op(V))
LinearAlgebra.mul!(Y::VecOrMat{Complex{Float64}}, R::ReceiversHIP, q::VecOrMat{Complex{Float64}}) = _receivers_apply!(Y, R, C_NULL, q, OP_N)
LinearAlgebra.mul!(Y::VecOrMat{Complex{Float64}}, V::Union{TransposeReceiversHIP,AdjointReceiversHIP}, w::VecOrMat{Complex{Float64}}) =
    _receivers_apply!(Y, V.parent, C_NULL, w, _op(V))
scattered_field(R::ReceiversHIP, M::FastMHIP, u::VecOrMat{Complex{Float64}}) = _receivers_apply!(_out(R, u, OP_N), R, M.plan, u, OP_N)
adjoint_source(R::ReceiversHIP, M::FastMHIP, w::VecOrMat{Complex{Float64}}) = _receivers_apply!(_out(R, w, OP_H), R, M.plan, w, OP_H)
receivers_set_stream(R::ReceiversHIP, stream::Ptr{Cvoid}) = check(ccall((:lsfc_receivers_set_stream, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), R.rc, stream))

# Linearised scattering -- lsfc_born_* (include/lsfc.h): J = d(data)/d(nu) for data d_s = -omega^2 R (nu .* u_s), M u_s = u_inc_s,
# its adjoint and the misfit gradient, device-resident.  B = Born(M, R, U_inc) solves for the background fields of the columns of
# U_inc; B * dnu is J dnu (nrecv x nsrc), B' * r is J^H r, misfit(B, d_obs) returns (phi, gradient), update!(B, nu) moves the
# medium.  The plan's op and the preconditioner's op are set by the library for the solves and put back.
# Born(...; mode=:reciprocal) or set_mode!(B, :reciprocal): one solve per receiver and medium for the receiver fields V = M^-1 R^T
# (receiver_fields(B)), after which B * dnu and B' * r are contractions of the stored U and V without any solve; it pays when
# (applies per medium) x nsrc > nrecv.  born_contract is the kernel-level entry.  (This part of the binding is written against
# include/lsfc.h and has not been executed: there is no Julia toolchain where the library is built and tested.)
const BORN_ACCUMULATE = Cuint(1); const BORN_REAL = Cuint(2)
const BORN_GMRES = Cint(0); const BORN_BICGSTABL = Cint(1)
const BORN_ADJOINT_STATE = Cint(0); const BORN_RECIPROCAL = Cint(1)
_born_mode(mode::Symbol) = mode == :adjoint_state ? BORN_ADJOINT_STATE : mode == :reciprocal ? BORN_RECIPROCAL :
    throw(ArgumentError("Born: mode must be :adjoint_state or :reciprocal, not $(repr(mode))"))
struct BornOpts                    # lsfc_born_opts
    solver::Cint; restart::Cint; l::Cint; maxiter::Int64; reltol::Float64; abstol::Float64
    precond::Ptr{Cvoid}; chunk::Int64; reserved::NTuple{6,Cint}
end
mutable struct Born
    b::Ptr{Cvoid}
    M::FastMHIP; R::ReceiversHIP; Pl
    U_inc::Matrix{Complex{Float64}}
    converged::Bool
    function Born(M::FastMHIP, R::ReceiversHIP, U_inc::Matrix{Complex{Float64}}; Pl=nothing, solver=:gmres, reltol=1e-8, restart=30, l=2,
                  maxiter=0, chunk=0, mode=:adjoint_state)
        mode_code = _born_mode(mode)
        (Pl === nothing || Pl isa SparsifyingPreconditionerHIP) || throw(ArgumentError("Born: Pl must be a SparsifyingPreconditionerHIP (not a wrapper of one)"))
        opts = Ref(BornOpts(solver == :gmres ? BORN_GMRES : BORN_BICGSTABL, restart, l, maxiter, reltol, 0.0,
                            Pl === nothing ? C_NULL : Pl.pc, chunk, ntuple(_ -> Cint(0), 6)))
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:lsfc_born_create, liblsfc), Cint, (Ref{Ptr{Cvoid}}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{BornOpts}), out, M.plan, R.rc, opts))
        B = new(out[], M, R, Pl, U_inc, true)
        finalizer(B -> ccall((:lsfc_born_destroy, liblsfc), Cint, (Ptr{Cvoid},), B.b), B)
        mode_code == BORN_ADJOINT_STATE || check(ccall((:lsfc_born_set_mode, liblsfc), Cint, (Ptr{Cvoid}, Cint), B.b, mode_code))
        set_background!(B, U_inc)
        return B
    end
end
struct AdjointBorn; parent::Born; end
LinearAlgebra.adjoint(B::Born) = AdjointBorn(B)
LinearAlgebra.adjoint(V::AdjointBorn) = V.parent
LinearAlgebra.transpose(::Born) = throw(ArgumentError("transpose(B) is not offered: J^T r = conj(J' conj(r))"))
nsrc(B::Born) = size(B.U_inc, 2)
Base.size(B::Born) = (B.R.nrecv * nsrc(B), B.R.N)
Base.eltype(::Union{Born,AdjointBorn}) = Complex{Float64}
# LSFC_ENOTCONV (-5) is a result: the outputs are written, B.converged says so and lasterror() names the first source
_born_rc(B::Born, rc) = (rc == 0 || rc == -5) ? (B.converged = rc == 0; nothing) : check(rc)
function set_background!(B::Born, U_inc::Matrix{Complex{Float64}})
    size(U_inc, 1) == B.R.N || throw(DimensionMismatch("U_inc"))
    B.U_inc = U_inc
    _born_rc(B, ccall((:lsfc_born_set_background, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Int64, Cint), B.b, U_inc, size(U_inc, 2), 0))
    return B
end
function data(B::Born)
    d = zeros(Complex{Float64}, B.R.nrecv, nsrc(B))
    check(ccall((:lsfc_born_data, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Cint), B.b, d, 0))
    return d
end
function born_results(B::Born)     # per source: iterations, operator applications, converged, residual of the last call
    out = zeros(Int64, 8); res = Vector{GmresResult}(undef, nsrc(B))
    check(ccall((:lsfc_born_info, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{GmresResult}), B.b, out, res))
    return res
end
function LinearAlgebra.mul!(dd::Matrix{Complex{Float64}}, B::Born, dnu::Union{Vector{Float64},Vector{Complex{Float64}}})
    (length(dnu) == B.R.N && size(dd) == (B.R.nrecv, nsrc(B))) || throw(DimensionMismatch("Born apply"))
    _born_rc(B, ccall((:lsfc_born_apply, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Cint, Ptr{Complex{Float64}}, Cint, Cuint, Cint),
                      B.b, dnu, eltype(dnu) <: Complex ? 1 : 0, dd, OP_N, 0, 0))
    return dd
end
function LinearAlgebra.mul!(g::Union{Vector{Float64},Vector{Complex{Float64}}}, V::AdjointBorn, r::Matrix{Complex{Float64}})
    B = V.parent
    (length(g) == B.R.N && size(r) == (B.R.nrecv, nsrc(B))) || throw(DimensionMismatch("Born adjoint"))
    _born_rc(B, ccall((:lsfc_born_apply, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Complex{Float64}}, Cint, Ptr{Cvoid}, Cint, Cuint, Cint),
                      B.b, r, 1, g, OP_H, eltype(g) <: Complex ? Cuint(0) : BORN_REAL, 0))
    return g
end
*(B::Born, dnu::Union{Vector{Float64},Vector{Complex{Float64}}}) = mul!(zeros(Complex{Float64}, B.R.nrecv, nsrc(B)), B, dnu)
*(V::AdjointBorn, r::Matrix{Complex{Float64}}) = mul!(zeros(Complex{Float64}, V.parent.R.N), V, r)
# (phi, grad): phi = 1/2 sum |d - d_obs|^2, grad = J^H (d - d_obs), its real part when nu is real
function misfit(B::Born, d_obs::Matrix{Complex{Float64}})
    res = data(B) .- d_obs
    g = nu_is_complex(B.M) ? zeros(Complex{Float64}, B.R.N) : zeros(Float64, B.R.N)
    return 0.5 * sum(abs2, res), mul!(g, B', res)
end
update!(B::Born, nu::NuVector) = (set_nu!(B.M, nu); set_background!(B, B.U_inc))
# :reciprocal with a background present solves for the receiver fields now; :adjoint_state releases them
set_mode!(B::Born, mode::Symbol) = (_born_rc(B, ccall((:lsfc_born_set_mode, liblsfc), Cint, (Ptr{Cvoid}, Cint), B.b, _born_mode(mode))); B)
function mode(B::Born)
    m = Ref{Cint}(0); bytes = Ref{Int64}(0)
    check(ccall((:lsfc_born_get_mode, liblsfc), Cint, (Ptr{Cvoid}, Ref{Cint}, Ref{Int64}), B.b, m, bytes))
    return m[] == BORN_RECIPROCAL ? :reciprocal : :adjoint_state
end
# the device pointer of V (N x nrecv, column r the field of receiver r) and nrecv; valid until the next set_background! / update! / set_mode!
function receiver_fields(B::Born)
    p = Ref{Ptr{Complex{Float64}}}(C_NULL); n = Ref{Int64}(0)
    check(ccall((:lsfc_born_receiver_fields, liblsfc), Cint, (Ptr{Cvoid}, Ref{Ptr{Complex{Float64}}}, Ref{Int64}), B.b, p, n))
    return p[], n[]
end
function receiver_results(B::Born)  # (nrecv, batched solves, operator applications, first receiver not converged or -1), per receiver results
    out = zeros(Int64, 4); res = Vector{GmresResult}(undef, B.R.nrecv)
    check(ccall((:lsfc_born_receiver_info, liblsfc), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{GmresResult}), B.b, out, res))
    return out, res
end
# lsfc_born_contract on host arrays: U (N x nsrc), V (N x nrecv); op = OP_N: x of length N -> nrecv x nsrc, out[r, s] = scale sum_i x[i] U[i, s] V[i, r];
# op = OP_H: x (nrecv x nsrc) -> out (length N, real: its real part) = [out +] conj(scale) sum_s conj(U[i, s]) sum_r conj(V[i, r]) x[r, s]
function born_contract(M::FastMHIP, U::Matrix{Complex{Float64}}, V::Matrix{Complex{Float64}}, x::Union{Array{Float64},Array{Complex{Float64}}};
                       op=OP_N, scale=1.0 + 0.0im, real=false, accumulate=nothing)
    N, ns, nr = size(U, 1), size(U, 2), size(V, 2)
    (size(V, 1) == N && length(x) == (op == OP_N ? N : ns * nr)) || throw(DimensionMismatch("born_contract"))
    out = op == OP_N ? zeros(Complex{Float64}, nr, ns) : accumulate !== nothing ? copy(accumulate) : real ? zeros(Float64, N) : zeros(Complex{Float64}, N)
    flags = (real ? BORN_REAL : Cuint(0)) | (accumulate !== nothing ? BORN_ACCUMULATE : Cuint(0))
    check(ccall((:lsfc_born_contract, liblsfc), Cint,
                (Ptr{Cvoid}, Ptr{Complex{Float64}}, Int64, Ptr{Complex{Float64}}, Int64, Ptr{Cvoid}, Cint, Ptr{Cvoid}, Cint, Cuint, Float64, Float64, Cint),
                M.plan, U, ns, V, nr, x, eltype(x) <: Complex ? 1 : 0, out, op, flags, Float64(Base.real(scale)), Float64(imag(scale)), 0))
    return out
end

end # module
